// libmdc_pngw.so (include/mdc_pngw.h): PNG files of device-resident grayscale images, made on the device.  One translation unit on
// top of png_block.h (the DEFLATE block builder, plain C++) and png_encode_core.h (the filter kernel's helpers, stream placement,
// framing and host helpers), both shared with mdc_pnglz.hip; the only thing it takes from another library is mdcz_crc32_device
// (libmdc_zipw.so) for the IDAT chunk's CRC.  What is this file's own: the layout of the per-image words, the kernels' names, its copy
// of the filter kernel's body (png_encode_core.h says why), the Huffman-only scan and pack (codes staged in LDS, plain stores for a
// run's inner words) and the entry points.
// Built with -DMDCP_RGB8_LIBRARY the same unit is libmdc_pngw_rgb.so (include/mdc_pngw_rgb.h) instead: the 8-bit RGB kind, whose pixel is
// one 3-byte sample of the filter kernel, with entry points of its own and none of the gray ones -- so the gray library, its kernels
// and its exported names are what they were, and the two can be loaded side by side.
//
// One call is six kernels and the checksum, with no host round trip between them:
//   pngw_filter_kernel   16 rows per workgroup, one wave per row: the row's filter type (adaptive: all five sums first), the filtered
//                        bytes into the scratch array, their histogram (one LDS histogram per wave, flushed with integer atomics)
//                        and the Adler-32 partial sums (sum d and, reduced mod 65521 per row and lane, sum (F - i) d; 64-bit atomics).
//   pngw_build_kernel    one workgroup per image: the symbols ranked by (count, symbol) by all lanes, then lane 0 alone: code lengths,
//                        canonical codes (stored bit-reversed: the stream is LSB-first), the run-length coded header and its bits,
//                        the dynamic stream's length and the stored/dynamic decision.  build_block() is plain C++ (host and device).
//   pngw_scan_kernel     one workgroup per image: each lane sums the code lengths of 16 filtered bytes (one 16-byte load, consecutive
//                        lanes on consecutive words), a scan gives every such unit its 64-bit bit offset; the words of the output
//                        that the pack kernel will OR into are cleared here.
//   pngw_pack_kernel     a lane packs its unit's codes at its bit offset: its first and last word, shared with the neighbours, by
//                        atomicOr, the words in between by plain stores.  The bit stream starts at byte 43 of the file, at any
//                        alignment: words are counted from the 4-byte boundary at or below it and every offset carries that shift.
//                        A stored image is a byte gather with the 5-byte block headers instead.
//   pngw_finish_kernel   signature, IHDR, IDAT length and tag, zlib header, Adler-32, IEND, d_sizes[f]; then mdcz_crc32_device over
//                        tag + data, and pngw_crc_kernel puts the four bytes in.
#include "../../include/mdc_pngw.h"
#ifdef MDCP_RGB8_LIBRARY
#include "../../include/mdc_pngw_rgb.h"
#endif

#include <new>

#include "../../include/mdc_zipw.h"
#include "png_encode_core.h"

namespace {

static_assert(MDCP_MAX_SYMBOLS == kMaxSym && MDCP_OK == kOk && MDCP_ERR_ARG == kErrArg && MDCP_ERR_HIP == kErrHip && MDCP_ERR_NO_DEVICE == kErrNoDevice &&
                  MDCP_ERR_NOMEM == kErrNoMem,
              "png_block.h and codec_host.h restate these values of include/mdc_pngw.h");

constexpr int kLit = 257;            // literals and end-of-block
constexpr int kSeq = 258;            // code lengths in the header: 257 + one distance code
constexpr int kHdrWords = 128;       // 17 + 57 + 258 * 14 bits at most: 116 words
constexpr int kZeroWords = 296;      // per image, cleared per call: histogram [288], Adler sums as two 64-bit words
constexpr int kTabWords = 400;       // per image: codes [260], header words [128], meta [12]
constexpr int kHdrAt = 260;
constexpr int kMeta = 388;           // meta: 0 stored?, 1 header bits, 2 stream bytes, 3/4 data bits (low, high)
constexpr long long kSmallBytes = 4 * (kZeroWords + kTabWords) + 8;  // + the checksum's length and result

struct Layout {
  static constexpr int zero_words = kZeroWords, adler_at = kMaxSym, tab_words = kTabWords, meta_at = kMeta;
};

// The Huffman-only block: png_block.h's rule and bit writer on this unit's own, smaller work area with the two counts of the header
// fixed at 257 and 1.  png_block.h's build_block gives the same bits (a tested fact), but in pngw_build_kernel it takes 201 VGPRs as it
// stands and, cut down to this case, 0.02 ms more per 1024 noise frames than this text: so this text stays.
struct BuildLds {
  uint32_t hist[kMaxSym];
  uint8_t len[kMaxSym];
  HuffWork work;
  uint32_t codes[260];
  uint8_t sym[kSeq + 2], ext[kSeq + 2];
  uint32_t clhist[19];
  uint8_t cllen[19];
  uint32_t clcodes[19];
  uint32_t hdr[kHdrWords];
  uint32_t meta[12];
};

// everything of one image's dynamic block that does not depend on the byte positions; L.hist[0..256] and L.work.order are filled
PNG_HD void build_block(BuildLds& L, long long F) {
  huff_lengths(L.hist, kLit, 15, L.work, L.len);
  canonical(L.len, kLit, 15, L.work, L.codes);
  L.len[kLit] = 0;  // the one distance code
  for (int i = 0; i < 19; i++) L.clhist[i] = 0;
  int nsyms = 0;
  for (int i = 0; i < kSeq;) {
    const int v = L.len[i];
    int run = 1;
    while (i + run < kSeq && L.len[i + run] == v) run++;
    i += run;
    if (v == 0) {
      while (run >= 11) {
        const int n = run < 138 ? run : 138;
        L.sym[nsyms] = 18, L.ext[nsyms++] = (uint8_t)(n - 11);
        run -= n;
      }
      if (run >= 3) {
        L.sym[nsyms] = 17, L.ext[nsyms++] = (uint8_t)(run - 3);
        run = 0;
      }
    } else {
      L.sym[nsyms] = (uint8_t)v, L.ext[nsyms++] = 0;
      run--;
      while (run >= 3) {
        const int n = run < 6 ? run : 6;
        L.sym[nsyms] = 16, L.ext[nsyms++] = (uint8_t)(n - 3);
        run -= n;
      }
    }
    for (; run > 0; run--) L.sym[nsyms] = (uint8_t)v, L.ext[nsyms++] = 0;
  }
  for (int i = 0; i < nsyms; i++) L.clhist[L.sym[i]]++;
  huff_order(L.clhist, 19, L.work.order, 0, 1);
  huff_lengths(L.clhist, 19, 7, L.work, L.cllen);
  canonical(L.cllen, 19, 7, L.work, L.clcodes);
  const uint8_t clorder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  int hclen = 4;
  for (int i = 4; i < 19; i++)
    if (L.cllen[clorder[i]]) hclen = i + 1;
  for (int i = 0; i < kHdrWords; i++) L.hdr[i] = 0;
  uint32_t bits = 0;
  put_bits(L.hdr, bits, 1, 1);  // BFINAL
  put_bits(L.hdr, bits, 2, 2);  // BTYPE: dynamic
  put_bits(L.hdr, bits, 0, 5);  // HLIT: 257 codes
  put_bits(L.hdr, bits, 0, 5);  // HDIST: 1 code
  put_bits(L.hdr, bits, (uint32_t)(hclen - 4), 4);
  for (int i = 0; i < hclen; i++) put_bits(L.hdr, bits, L.cllen[clorder[i]], 3);
  for (int i = 0; i < nsyms; i++) {
    const int s = L.sym[i];
    put_bits(L.hdr, bits, L.clcodes[s] & 0xffffu, (int)(L.clcodes[s] >> 16));
    if (s >= 16) put_bits(L.hdr, bits, L.ext[i], s == 16 ? 2 : s == 17 ? 3 : 7);
  }
  unsigned long long data = 0;
  for (int s = 0; s < 256; s++) data += (unsigned long long)L.hist[s] * L.len[s];
  const unsigned long long total = bits + data + L.len[256];
  const long long dyn = (long long)((total + 7) >> 3), stored = stored_bytes(F);
  L.meta[0] = dyn < stored ? 0u : 1u;
  L.meta[1] = bits;
  L.meta[2] = (uint32_t)(dyn < stored ? dyn : stored);
  L.meta[3] = (uint32_t)data;
  L.meta[4] = (uint32_t)(data >> 32);
}

// ---------------------------------------------------------------------------------------------------- pixels -> filtered bytes

template <typename T, int BPP>
__global__ __launch_bounds__(256) void pngw_filter_kernel(const T* __restrict__ images, long long stride, long long nimages, int w, int h, int filter,
                                                          uint8_t* __restrict__ filt, long long filt_stride, uint32_t* __restrict__ zeroed) {
  __shared__ uint32_t hist[4][256];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const long long groups = ((long long)h + kRowsPerGroup - 1) / kRowsPerGroup;
  const long long items = nimages * groups;
  const long long rs = 1 + (long long)w * BPP, F = rs * h;  // F < 2^31
  for (long long item = blockIdx.x; item < items; item += gridDim.x) {
    const long long f = item / groups;
    const int y0 = (int)(item - f * groups) * kRowsPerGroup;
    const int y1 = y0 + kRowsPerGroup < h ? y0 + kRowsPerGroup : h;
    for (int i = t; i < 4 * 256; i += 256) (&hist[0][0])[i] = 0;
    __syncthreads();
    const T* __restrict__ img = image_at(images, f, stride);
    uint8_t* __restrict__ out = filt + f * filt_stride;
    unsigned long long s1 = 0, s2 = 0;
    for (int y = y0 + wave; y < y1; y += 4) {
      const T* __restrict__ row = img + (long long)y * w;
      const T* __restrict__ up = row - w;  // read only when y > 0
      int type = filter;
      if (filter == MDCP_FILTER_ADAPTIVE) {
        unsigned long long sum[5] = {0, 0, 0, 0, 0};
        for (int x = lane; x < w; x += 64) {
          const int X = sample_of(row[x]), A = x > 0 ? sample_of(row[x - 1]) : 0;
          const int B = y > 0 ? sample_of(up[x]) : 0, Cc = (x > 0 && y > 0) ? sample_of(up[x - 1]) : 0;
#pragma unroll
          for (int k = 0; k < BPP; k++) {
            const int sh = 8 * (BPP - 1 - k);
            const int xb = (X >> sh) & 255, ab = (A >> sh) & 255, bb = (B >> sh) & 255, cb = (Cc >> sh) & 255;
#pragma unroll
            for (int ty = 0; ty < 5; ty++) {
              const int d = filter_byte(ty, xb, ab, bb, cb);
              sum[ty] += (unsigned)(d < 128 ? d : 256 - d);
            }
          }
        }
        unsigned long long best = 0;
#pragma unroll
        for (int ty = 0; ty < 5; ty++) {
          const unsigned long long v = wave_sum(sum[ty]);
          if (ty == 0 || v < best) best = v, type = ty;
        }
      }
      const long long at = (long long)y * rs;
      unsigned long long r2 = 0;
      if (lane == 0) {
        out[at] = (uint8_t)type;
        atomicAdd(&hist[wave][type], 1u);
        s1 += (unsigned)type;
        r2 += (unsigned long long)(F - at) * (unsigned)type;
      }
      for (int x = lane; x < w; x += 64) {
        const int X = sample_of(row[x]), A = x > 0 ? sample_of(row[x - 1]) : 0;
        const int B = y > 0 ? sample_of(up[x]) : 0, Cc = (x > 0 && y > 0) ? sample_of(up[x - 1]) : 0;
#pragma unroll
        for (int k = 0; k < BPP; k++) {
          const int sh = 8 * (BPP - 1 - k);
          const int d = filter_byte(type, (X >> sh) & 255, (A >> sh) & 255, (B >> sh) & 255, (Cc >> sh) & 255);
          const long long i = at + 1 + (long long)x * BPP + k;
          out[i] = (uint8_t)d;
          atomicAdd(&hist[wave][d], 1u);
          s1 += (unsigned)d;
          r2 += (unsigned long long)(F - i) * (unsigned)d;  // < 2^39 each, fewer than 2^12 per lane and row
        }
      }
      s2 += r2 % kAdlerMod;
    }
    __syncthreads();
    uint32_t* __restrict__ g = zeroed + f * kZeroWords;
    const uint32_t v = hist[0][t] + hist[1][t] + hist[2][t] + hist[3][t];
    if (v) atomicAdd(&g[t], v);
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if (lane == 0 && y0 + wave < y1) {
      unsigned long long* __restrict__ adler = (unsigned long long*)(g + kMaxSym);
      atomicAdd(&adler[0], s1);
      atomicAdd(&adler[1], s2);
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------- the code

__global__ __launch_bounds__(256) void pngw_build_kernel(long long nimages, long long F, const uint32_t* __restrict__ zeroed, uint32_t* __restrict__ tab) {
  __shared__ BuildLds L;
  const int t = threadIdx.x;
  for (long long f = blockIdx.x; f < nimages; f += gridDim.x) {
    L.hist[t] = zeroed[f * kZeroWords + t];
    if (t == 0) L.hist[256] = 1;  // end-of-block
    __syncthreads();
    huff_order(L.hist, kLit, L.work.order, t, 256);
    __syncthreads();
    if (t == 0) build_block(L, F);
    __syncthreads();
    uint32_t* __restrict__ o = tab + f * kTabWords;
    for (int i = t; i < kLit; i += 256) o[i] = L.codes[i];
    if (t < kHdrWords) o[260 + t] = L.hdr[t];
    if (t < 12) o[kMeta + t] = L.meta[t];
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void pngw_lengths_kernel(const uint32_t* __restrict__ hist, int nsym, int limit, uint8_t* __restrict__ lengths) {
  __shared__ BuildLds L;
  const int t = threadIdx.x;
  for (int s = t; s < nsym; s += 256) L.hist[s] = hist[s];
  __syncthreads();
  huff_order(L.hist, nsym, L.work.order, t, 256);
  __syncthreads();
  if (t == 0) huff_lengths(L.hist, nsym, limit, L.work, L.len);
  __syncthreads();
  for (int s = t; s < nsym; s += 256) lengths[s] = L.len[s];
}

// ---------------------------------------------------------------------------------------------------- bit offsets

__device__ __forceinline__ uint32_t unit_bits(const uint4 v, int valid, const uint8_t* __restrict__ lens) {
  const uint32_t d[4] = {v.x, v.y, v.z, v.w};
  uint32_t bits = 0;
#pragma unroll
  for (int k = 0; k < 16; k++) bits += k < valid ? lens[(d[k >> 2] >> (8 * (k & 3))) & 255] : 0u;
  return bits;
}

__global__ __launch_bounds__(1024) void pngw_scan_kernel(long long nimages, long long F, const uint8_t* __restrict__ filt, long long filt_stride,
                                                         const uint32_t* __restrict__ tab, unsigned long long* __restrict__ offsets, uint8_t* out,
                                                         long long slot_bytes) {
  __shared__ uint8_t lens[260];
  const int t = threadIdx.x;
  const long long nunits = (F + 15) >> 4;
  for (long long f = blockIdx.x; f < nimages; f += gridDim.x) {
    const uint32_t* __restrict__ tb = tab + f * kTabWords;
    if (tb[kMeta]) continue;  // stored: nothing is packed
    __syncthreads();
    if (t < kLit) lens[t] = (uint8_t)(tb[t] >> 16);
    const uint4* __restrict__ src = (const uint4*)(filt + f * filt_stride);
    scan_units(slot_of(out, slot_bytes, f), tb[kMeta + 1], F, offsets + f * nunits, lens,
               [&](long long u, int valid) { return unit_bits(src[u], valid, lens); });
  }
}

// ---------------------------------------------------------------------------------------------------- the stream

// Bits least significant first into 32-bit words.  The words are zero where nothing has been written; the first and the last word
// of a run are shared with its neighbours and OR-ed in with integer atomics, the words in between are the run's own.
struct BitPacker {
  uint32_t* __restrict__ word;
  unsigned long long acc = 0;
  int n;
  bool first = true;
  __device__ __forceinline__ BitPacker(uint32_t* words, unsigned long long bit) : word(words + (bit >> 5)), n((int)(bit & 31)) {}
  __device__ __forceinline__ void operator()(uint32_t code) {  // bits | count << 16, count <= 15
    acc |= (unsigned long long)(code & 0xffffu) << n;
    n += (int)(code >> 16);
    if (n >= 32) {
      if (first) atomicOr(word, (uint32_t)acc);
      else *word = (uint32_t)acc;
      first = false;
      word++;
      acc >>= 32;
      n -= 32;
    }
  }
  __device__ __forceinline__ void finish() {
    if (n > 0 && (uint32_t)acc) atomicOr(word, (uint32_t)acc);
  }
};

__global__ __launch_bounds__(256) void pngw_pack_kernel(long long nimages, long long F, int parts, const uint8_t* __restrict__ filt, long long filt_stride,
                                                        const uint32_t* __restrict__ tab, const unsigned long long* __restrict__ offsets, uint8_t* out,
                                                        long long slot_bytes) {
  __shared__ uint32_t codes[kLit];
  const int t = threadIdx.x;
  const long long nunits = (F + 15) >> 4;
  const long long items = nimages * parts;
  for (long long item = blockIdx.x; item < items; item += gridDim.x) {
    const long long f = item / parts;
    const int p = (int)(item - f * parts);
    const uint32_t* __restrict__ tb = tab + f * kTabWords;
    const uint8_t* __restrict__ src = filt + f * filt_stride;
    const Slot sl = slot_of(out, slot_bytes, f);
    if (tb[kMeta]) {
      pack_stored(sl, src, F, p, parts, t);
      continue;
    }
    __syncthreads();
    for (int i = t; i < kLit; i += 256) codes[i] = tb[i];
    __syncthreads();
    if (p == 0) {
      const uint32_t hdr_bits = tb[kMeta + 1];
      for (uint32_t j = t; j < ((hdr_bits + 31) >> 5); j += 256) {
        const uint32_t v = tb[kHdrAt + j];
        if (v << sl.shift) atomicOr(sl.words + j, v << sl.shift);
        if (sl.shift && (v >> (32 - sl.shift))) atomicOr(sl.words + j + 1, v >> (32 - sl.shift));
      }
      if (t == 0) {
        const unsigned long long data = (unsigned long long)tb[kMeta + 3] | ((unsigned long long)tb[kMeta + 4] << 32);
        BitPacker bp(sl.words, (unsigned long long)sl.shift + hdr_bits + data);
        bp(codes[256]);
        bp.finish();
      }
    }
    const uint4* __restrict__ src16 = (const uint4*)src;
    const unsigned long long* __restrict__ off = offsets + f * nunits;
    for (long long u = (long long)p * 256 + t; u < nunits; u += (long long)parts * 256) {
      const uint4 v = src16[u];
      const long long rem = F - u * 16;
      const int valid = rem < 16 ? (int)rem : 16;
      const uint32_t d[4] = {v.x, v.y, v.z, v.w};
      BitPacker bp(sl.words, off[u]);
#pragma unroll
      for (int k = 0; k < 16; k++)
        if (k < valid) bp(codes[(d[k >> 2] >> (8 * (k & 3))) & 255]);
      bp.finish();
    }
  }
}

__global__ __launch_bounds__(256) void pngw_finish_kernel(long long nimages, long long F, const uint8_t* __restrict__ head, const uint32_t* __restrict__ zeroed,
                                                          const uint32_t* __restrict__ tab, uint8_t* out, long long slot_bytes, int32_t* __restrict__ sizes,
                                                          int32_t* __restrict__ crc_len) {
  finish_files<Layout>(nimages, F, head, zeroed, tab, out, slot_bytes, sizes, crc_len);
}

__global__ __launch_bounds__(256) void pngw_crc_kernel(long long nimages, const uint32_t* __restrict__ tab, const uint32_t* __restrict__ crc, uint8_t* out,
                                                       long long slot_bytes) {
  crc_bytes<Layout>(nimages, tab, crc, out, slot_bytes);
}

}  // namespace

// ---------------------------------------------------------------------------------------------------- host side

struct mdcp_encoder {
  int device = -1, w = 0, h = 0, depth = 0, bpp = 0, filter = 0, max_images = 0;  // depth: bits per pixel -- 8, 16, or 24 for 8-bit RGB
  long long F = 0, nunits = 0;
  uint8_t* d_head = nullptr;
  uint8_t* d_filt = nullptr;
  unsigned long long* d_offsets = nullptr;
  uint32_t* d_zeroed = nullptr;
  uint32_t* d_tab = nullptr;
  int32_t* d_crc_len = nullptr;
  uint32_t* d_crc = nullptr;
  uint8_t* d_out = nullptr;  // mdcp_output_device: allocated on demand
  int32_t* d_sizes = nullptr;
};

namespace {

void destroy(mdcp_encoder* enc) {
  if (!enc) return;
  {
    DeviceGuard dg(enc->device);
    (void)hipFree(enc->d_head);
    (void)hipFree(enc->d_filt);
    (void)hipFree(enc->d_offsets);
    (void)hipFree(enc->d_zeroed);
    (void)hipFree(enc->d_tab);
    (void)hipFree(enc->d_crc_len);
    (void)hipFree(enc->d_crc);
    (void)hipFree(enc->d_out);
    (void)hipFree(enc->d_sizes);
  }
  delete enc;
}

// depth = bits per pixel: 8 or 16 (gray), 24 (8-bit RGB)
int create(const char* who, int device, int w, int h, int depth, int filter, int max_images, mdcp_encoder** out) {
  if (filter < 0 || filter > MDCP_FILTER_ADAPTIVE) return fail(MDCP_ERR_ARG, "%s: filter %d is outside 0..%d", who, filter, MDCP_FILTER_ADAPTIVE);
  if (max_images < 1) return fail(MDCP_ERR_ARG, "%s: max_images %d is below 1", who, max_images);
  if (w < 1 || h < 1) return fail(MDCP_ERR_SIZE, "%s: %d x %d: width and height start at 1", who, w, h);
  if (bound_of(w, h, depth / 8) < 0) return fail(MDCP_ERR_SIZE, "%s: a %d x %d image of %d bits passes 2^31 - 1 bytes (sizes are int32_t)", who, w, h, depth);
  const long long F = (1 + (long long)w * (depth / 8)) * h, nunits = (F + 15) / 16;
  const long long per_image = 24 * nunits + kSmallBytes;
  if (per_image > (1ll << 40) / max_images)
    return fail(MDCP_ERR_SIZE, "%s: %d images x %lld bytes of scratch pass 2^40 bytes", who, max_images, per_image);
  if (int rc = resolve_device(who, &device)) return rc;
  DeviceGuard dg(device);
  mdcp_encoder* e = new (std::nothrow) mdcp_encoder;
  if (!e) return fail(MDCP_ERR_NOMEM, "%s: out of host memory", who);
  e->device = device, e->w = w, e->h = h, e->depth = depth, e->bpp = depth / 8, e->filter = filter, e->max_images = max_images;
  e->F = F, e->nunits = nunits;
  const size_t n = (size_t)max_images;
  if (hipMalloc((void**)&e->d_head, 48) != hipSuccess || hipMalloc((void**)&e->d_filt, n * (size_t)nunits * 16) != hipSuccess ||
      hipMalloc((void**)&e->d_offsets, n * (size_t)nunits * 8) != hipSuccess || hipMalloc((void**)&e->d_zeroed, n * kZeroWords * 4) != hipSuccess ||
      hipMalloc((void**)&e->d_tab, n * kTabWords * 4) != hipSuccess || hipMalloc((void**)&e->d_crc_len, n * 4) != hipSuccess ||
      hipMalloc((void**)&e->d_crc, n * 4) != hipSuccess) {
    (void)hipGetLastError();
    destroy(e);
    return fail(MDCP_ERR_NOMEM, "%s: could not allocate the scratch arrays of %d images of %d x %d", who, max_images, w, h);
  }
  uint8_t head[48];
  png_head(head, w, h, depth == 24 ? 8 : depth, depth == 24 ? 2 : 0);  // colour type: truecolour or gray
  if (hipMemcpy(e->d_head, head, sizeof head, hipMemcpyHostToDevice) != hipSuccess) {
    destroy(e);
    return fail(MDCP_ERR_HIP, "%s: copying the header failed", who);
  }
  *out = e;
  return MDCP_OK;
}

template <typename T, int BPP>
int encode(const char* who, mdcp_encoder* e, const T* d_images, int64_t stride, int nimages, uint8_t* d_out, int64_t slot_bytes, int32_t* d_sizes, void* stream) {
  constexpr int kPerElement = BPP == 3 ? 3 : 1;      // an RGB stride is given in bytes, a gray one in elements
  constexpr size_t kAlign = BPP == 3 ? 1 : sizeof(T);  // RGB pixels are bytes
  if (!e) return fail(MDCP_ERR_ARG, "%s: encoder is null", who);
  if (e->depth != 8 * BPP) return fail(MDCP_ERR_ARG, "%s: the encoder was made for %d-bit images", who, e->depth);
  if (nimages < 0 || nimages > e->max_images) return fail(MDCP_ERR_ARG, "%s: %d images, the encoder was made for 0..%d", who, nimages, e->max_images);
  if (nimages == 0) return MDCP_OK;
  if (!d_images || !d_out || !d_sizes) return fail(MDCP_ERR_ARG, "%s: null device pointer", who);
  if ((uintptr_t)d_images % kAlign) return fail(MDCP_ERR_ARG, "%s: d_images %p is not aligned to its %zu-byte elements", who, (const void*)d_images, sizeof(T));
  if (stride < (int64_t)e->w * e->h * kPerElement)
    return fail(MDCP_ERR_ARG, "%s: stride %lld is below %d x %d%s", who, (long long)stride, e->w, e->h, kPerElement == 3 ? " x 3 bytes" : "");
  const int64_t bound = bound_of(e->w, e->h, BPP);
  if (slot_bytes < bound && BPP == 3)
    return fail(MDCP_ERR_SIZE, "%s: slot_bytes %lld is below mdcp_png_bound_rgb8(%d, %d) = %lld", who, (long long)slot_bytes, e->w, e->h, (long long)bound);
  if (slot_bytes < bound)
    return fail(MDCP_ERR_SIZE, "%s: slot_bytes %lld is below mdcp_png_bound(%d, %d, %d) = %lld", who, (long long)slot_bytes, e->w, e->h, e->depth, (long long)bound);
  DeviceGuard dg(e->device);
  hipStream_t s = (hipStream_t)stream;
  const long long n = nimages, F = e->F, fs = e->nunits * 16;
  if (hipMemsetAsync(e->d_zeroed, 0, (size_t)n * kZeroWords * 4, s) != hipSuccess)
    return fail(MDCP_ERR_HIP, "%s: clearing the histograms failed: %s", who, hipGetErrorString(hipGetLastError()));
  const long long groups = ((long long)e->h + kRowsPerGroup - 1) / kRowsPerGroup;
  const long long parts = pack_parts(n, e->nunits);
  pngw_filter_kernel<T, BPP><<<grid_for(n * groups), 256, 0, s>>>(d_images, (long long)stride, n, e->w, e->h, e->filter, e->d_filt, fs, e->d_zeroed);
  pngw_build_kernel<<<grid_for(n), 256, 0, s>>>(n, F, e->d_zeroed, e->d_tab);
  pngw_scan_kernel<<<grid_for(n), 1024, 0, s>>>(n, F, e->d_filt, fs, e->d_tab, e->d_offsets, d_out, (long long)slot_bytes);
  pngw_pack_kernel<<<grid_for(n * parts), 256, 0, s>>>(n, F, (int)parts, e->d_filt, fs, e->d_tab, e->d_offsets, d_out, (long long)slot_bytes);
  pngw_finish_kernel<<<grid_for((n + 255) / 256), 256, 0, s>>>(n, F, e->d_head, e->d_zeroed, e->d_tab, d_out, (long long)slot_bytes, d_sizes, e->d_crc_len);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(MDCP_ERR_HIP, "%s: launch failed: %s", who, hipGetErrorString(err));
  if (mdcz_crc32_device(d_out + 37, slot_bytes, e->d_crc_len, n, e->d_crc, stream) != MDCZ_OK)
    return fail(MDCP_ERR_HIP, "%s: the IDAT checksum failed: %s", who, mdcz_last_error());
  pngw_crc_kernel<<<grid_for((n + 255) / 256), 256, 0, s>>>(n, e->d_tab, e->d_crc, d_out, (long long)slot_bytes);
  if ((err = hipGetLastError()) != hipSuccess) return fail(MDCP_ERR_HIP, "%s: launch failed: %s", who, hipGetErrorString(err));
  return MDCP_OK;
}

}  // namespace

extern "C" {

#ifdef MDCP_RGB8_LIBRARY

int64_t mdcp_png_bound_rgb8(int w, int h) { return bound_of(w, h, 3); }

const char* mdcp_last_error_rgb8(void) { return g_error; }

int mdcp_create_rgb8(int device, int w, int h, int filter, int max_images, mdcp_encoder** out) {
  if (!out) return fail(MDCP_ERR_ARG, "mdcp_create_rgb8: out is null");
  *out = nullptr;
  return create("mdcp_create_rgb8", device, w, h, 24, filter, max_images, out);
}

void mdcp_destroy_rgb8(mdcp_encoder* enc) { destroy(enc); }

int mdcp_encode_rgb8_device(mdcp_encoder* enc, const uint8_t* d_images, int64_t stride_bytes, int nimages, uint8_t* d_out, int64_t slot_bytes,
                            int32_t* d_sizes, void* stream) {
  return encode<Rgb8, 3>("mdcp_encode_rgb8_device", enc, (const Rgb8*)d_images, stride_bytes, nimages, d_out, slot_bytes, d_sizes, stream);
}

int mdcp_output_device_rgb8(mdcp_encoder* enc, uint8_t** d_out, int64_t* slot_bytes, int32_t** d_sizes) {
  return output_device("mdcp_output_device_rgb8", enc, d_out, slot_bytes, d_sizes);
}

#else

int64_t mdcp_png_bound(int w, int h, int depth) {
  if (depth != 8 && depth != 16) return -1;
  return bound_of(w, h, depth / 8);
}

const char* mdcp_last_error(void) { return g_error; }

int mdcp_create(int device, int w, int h, int depth, int filter, int max_images, mdcp_encoder** out) {
  if (!out) return fail(MDCP_ERR_ARG, "mdcp_create: out is null");
  *out = nullptr;
  if (depth != 8 && depth != 16) return fail(MDCP_ERR_ARG, "mdcp_create: depth %d is neither 8 nor 16", depth);
  return create("mdcp_create", device, w, h, depth, filter, max_images, out);
}

void mdcp_destroy(mdcp_encoder* enc) { destroy(enc); }

int mdcp_encode_u8_device(mdcp_encoder* enc, const uint8_t* d_images, int64_t stride, int nimages, uint8_t* d_out, int64_t slot_bytes, int32_t* d_sizes,
                          void* stream) {
  return encode<uint8_t, 1>("mdcp_encode_u8_device", enc, d_images, stride, nimages, d_out, slot_bytes, d_sizes, stream);
}

int mdcp_encode_u16_device(mdcp_encoder* enc, const uint16_t* d_images, int64_t stride, int nimages, uint8_t* d_out, int64_t slot_bytes, int32_t* d_sizes,
                           void* stream) {
  return encode<uint16_t, 2>("mdcp_encode_u16_device", enc, d_images, stride, nimages, d_out, slot_bytes, d_sizes, stream);
}

int mdcp_encode_f32_device(mdcp_encoder* enc, const float* d_images, int64_t stride, int nimages, uint8_t* d_out, int64_t slot_bytes, int32_t* d_sizes,
                           void* stream) {
  return encode<float, 1>("mdcp_encode_f32_device", enc, d_images, stride, nimages, d_out, slot_bytes, d_sizes, stream);
}

int mdcp_output_device(mdcp_encoder* enc, uint8_t** d_out, int64_t* slot_bytes, int32_t** d_sizes) {
  return output_device("mdcp_output_device", enc, d_out, slot_bytes, d_sizes);
}

int mdcp_huffman_lengths_device(const uint32_t* d_hist, int nsym, int limit, uint8_t* d_lengths, void* stream) {
  const char* who = "mdcp_huffman_lengths_device";
  if (!d_hist || !d_lengths) return fail(MDCP_ERR_ARG, "%s: null pointer", who);
  if (nsym < 1 || nsym > kMaxSym) return fail(MDCP_ERR_ARG, "%s: nsym %d is outside 1..%d", who, nsym, kMaxSym);
  if (limit < 1 || limit > 15) return fail(MDCP_ERR_ARG, "%s: limit %d is outside 1..15", who, limit);
  if (nsym > (1 << limit)) return fail(MDCP_ERR_ARG, "%s: %d symbols do not fit codes of at most %d bits", who, nsym, limit);
  pngw_lengths_kernel<<<1, 256, 0, (hipStream_t)stream>>>(d_hist, nsym, limit, d_lengths);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(MDCP_ERR_HIP, "%s: launch failed: %s", who, hipGetErrorString(err));
  return MDCP_OK;
}

#endif  // MDCP_RGB8_LIBRARY

}  // extern "C"
