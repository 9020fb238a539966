// libmdc_pnglz.so (include/mdc_pnglz.h): PNG files of device-resident images with LZ77 matches in the DEFLATE stream, made on the
// device.  One translation unit on top of png_block.h (the DEFLATE block builder, plain C++, also a host test program) and
// png_encode_core.h (the filter kernel's helpers, stream placement, framing and host helpers), both shared with mdc_pngw.hip: the
// code-length rule, the header writer, the bit offsets' scan and the framing are one text for the three libraries.  From another
// library it takes only mdcz_crc32_device (libmdc_zipw.so).  What is this file's own: the layout of the per-image words, the kernels'
// names, its copy of the filter kernel's body (png_encode_core.h says why), the order, match, parse and tally kernels, the token loops
// of the scan and pack kernels, and a BitPacker that ORs every word.
//
// One call is nine kernels and the checksum, with no host round trip between them:
//   pnglz_filter_kernel  as pngw_filter_kernel: filtered bytes, their histogram, the Adler-32 partial sums.
//   pnglz_order_kernel   one workgroup per image: the positions p (p + 2 < F) in the order "by trigram d[p..p+2], then by position", by
//                        three stable counting-sort passes (byte p+2, p+1, p); equal bytes of a 1024-position tile are ranked by
//                        ballots inside a wave and by per-wave counts across waves.
//   pnglz_match_kernel   one lane per position of that order: its predecessors there are its candidates, nearest first; 8 bytes per
//                        comparison step; keeps (length, distance) of the best.
//   pnglz_parse_kernel   one lane per 4096-byte chunk walks it greedily and marks the positions that matches cover.
//   pnglz_tally_kernel   the two histograms of the tokens (LDS histograms, flushed with integer atomics), tokens and matches counted.
//   pnglz_build_kernel   one workgroup per image: lane 0 builds the Huffman-only block, lane 64 the block with matches (build_block,
//                        plain C++), then the choice of form.
//   pnglz_scan_kernel    one workgroup per image: the bits of every 16-position unit's tokens, scanned into 64-bit bit offsets.
//   pnglz_pack_kernel    a lane packs its unit's tokens at its offset, every word by atomicOr into the words the scan cleared (a unit is
//                        17 bits on a smooth frame: few words are a unit's own); the codes are read through the caches; stored: a byte gather.
//   pnglz_finish_kernel  the framing, Adler-32, sizes; then mdcz_crc32_device and pnglz_crc_kernel.
// All integer, no private memory, every loop bounded by F or a constant.
#include "../../include/mdc_pnglz.h"

#include <new>

#include "../../include/mdc_zipw.h"
#include "png_encode_core.h"

namespace {

static_assert(MDCL_OK == kOk && MDCL_ERR_ARG == kErrArg && MDCL_ERR_HIP == kErrHip && MDCL_ERR_NO_DEVICE == kErrNoDevice && MDCL_ERR_NOMEM == kErrNoMem,
              "codec_host.h restates these values of include/mdc_pnglz.h");

constexpr int kHistAt = 0;                    // per image, cleared per call: the filtered bytes' histogram [256]
constexpr int kAdlerAt = 256;                 //   the Adler sums as two 64-bit words
constexpr int kTokAt = 260;                   //   the tokens' histograms [316]
constexpr int kCountAt = kTokAt + kAll;       //   tokens, matches
constexpr int kZeroWords = kCountAt + 4;      // 580
constexpr int kHdrAt = kAll;                  // per image: codes [316], header words [144], meta [12]
constexpr int kMeta = kHdrAt + kHdrWords;     // meta: 0 form, 1 header bits, 2 stream bytes, 3/4 data bits (low, high)
constexpr int kTabWords = kMeta + 12;         // 472
constexpr uint32_t kCovered = 0xffffffffu;    // in the match array after the parse: inside a match, no token starts here
constexpr long long kSmallBytes = 4 * (kZeroWords + kTabWords) + 16 + 8;  // + the form record, the checksum's length and result

struct Layout {
  static constexpr int zero_words = kZeroWords, adler_at = kAdlerAt, tab_words = kTabWords, meta_at = kMeta;
};

// ---------------------------------------------------------------------------------------------------- pixels -> filtered bytes

template <typename T, int BPP>
__global__ __launch_bounds__(256) void pnglz_filter_kernel(const T* __restrict__ images, long long stride, long long nimages, int w, int h, int filter,
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
      if (filter == MDCL_FILTER_ADAPTIVE) {
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
    if (v) atomicAdd(&g[kHistAt + t], v);
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if (lane == 0 && y0 + wave < y1) {
      unsigned long long* __restrict__ adler = (unsigned long long*)(g + kAdlerAt);
      atomicAdd(&adler[0], s1);
      atomicAdd(&adler[1], s2);
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------- candidates

// a = the positions 0 .. F - 3 of image f ordered by (d[p], d[p+1], d[p+2], p); b is the other buffer of the three passes
__global__ __launch_bounds__(1024) void pnglz_order_kernel(long long nimages, long long F, const uint8_t* __restrict__ filt, long long filt_stride,
                                                           uint32_t* idx_a, uint32_t* idx_b) {
  __shared__ uint32_t base[256];
  __shared__ uint32_t wave_count[16][256];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const long long n = F - 2;
  for (long long f = blockIdx.x; f < nimages; f += gridDim.x) {
    const uint8_t* __restrict__ d = filt + f * filt_stride;
    uint32_t* a = idx_a + f * filt_stride;
    uint32_t* b = idx_b + f * filt_stride;
    for (int pass = 0; pass < 3; pass++) {
      const uint32_t* in = pass == 1 ? a : b;  // pass 0 reads the identity
      uint32_t* out = pass == 1 ? b : a;
      const int shift = 2 - pass;
      __syncthreads();
      if (t < 256) base[t] = 0;
      __syncthreads();
      for (long long i = t; i < n; i += 1024) atomicAdd(&base[d[i + shift]], 1u);  // the counts do not depend on the order
      __syncthreads();
      if (wave == 0) {  // exclusive scan of the 256 counts
        const uint32_t c0 = base[4 * lane], c1 = base[4 * lane + 1], c2 = base[4 * lane + 2], c3 = base[4 * lane + 3];
        const uint32_t sum = c0 + c1 + c2 + c3;
        uint32_t inc = sum;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const uint32_t other = __shfl_up(inc, o, 64);
          if (lane >= o) inc += other;
        }
        const uint32_t ex = inc - sum;
        base[4 * lane] = ex, base[4 * lane + 1] = ex + c0, base[4 * lane + 2] = ex + c0 + c1, base[4 * lane + 3] = ex + c0 + c1 + c2;
      }
      __syncthreads();
      for (long long first = 0; first < n; first += 1024) {
        const long long i = first + t;
        const bool valid = i < n;
        const uint32_t p = valid ? (pass == 0 ? (uint32_t)i : in[i]) : 0u;
        const uint32_t digit = valid ? d[p + shift] : 0u;
        unsigned long long peers = __ballot(valid);
#pragma unroll
        for (int bit = 0; bit < 8; bit++) {
          const bool one = (digit >> bit) & 1;
          const unsigned long long bal = __ballot(one);
          peers &= one ? bal : ~bal;
        }
        const uint32_t rank = (uint32_t)__popcll(peers & ((1ull << lane) - 1));
        for (int k = lane; k < 256; k += 64) wave_count[wave][k] = 0;
        if (valid && rank == 0) wave_count[wave][digit] = (uint32_t)__popcll(peers);
        __syncthreads();
        if (t < 256) {
          uint32_t run = base[t];
#pragma unroll
          for (int wv = 0; wv < 16; wv++) {
            const uint32_t c = wave_count[wv][t];
            wave_count[wv][t] = run;
            run += c;
          }
          base[t] = run;
        }
        __syncthreads();
        if (valid) out[wave_count[wave][digit] + rank] = p;
        __syncthreads();
      }
    }
  }
}

__device__ __forceinline__ int common_prefix(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, int cap) {
  int j = 0;
  while (j + 8 <= cap) {
    unsigned long long x, y;
    __builtin_memcpy(&x, a + j, 8);
    __builtin_memcpy(&y, b + j, 8);
    if (x != y) return j + (__builtin_ctzll(x ^ y) >> 3);
    j += 8;
  }
  while (j < cap && a[j] == b[j]) j++;
  return j;
}

__device__ __forceinline__ int cap_at(long long p, long long F) {
  long long cap = F - p;
  const long long in_chunk = kChunk - (p & (kChunk - 1));
  if (in_chunk < cap) cap = in_chunk;
  return cap < kMaxMatch ? (int)cap : kMaxMatch;
}

// match[p] = length << 16 | (distance - 1) of best(p), 0 when none counts
__global__ __launch_bounds__(256) void pnglz_match_kernel(long long nimages, long long F, int chain, const uint8_t* __restrict__ filt, long long filt_stride,
                                                          const uint32_t* __restrict__ idx_a, uint32_t* __restrict__ match) {
  const long long n = F - 2;
  if (n <= 0) return;
  const long long blocks = (n + 255) / 256, items = nimages * blocks;
  for (long long item = blockIdx.x; item < items; item += gridDim.x) {
    const long long f = item / blocks;
    const long long i = (item - f * blocks) * 256 + threadIdx.x;
    if (i >= n) continue;
    const uint8_t* __restrict__ d = filt + f * filt_stride;
    const uint32_t* __restrict__ a = idx_a + f * filt_stride;
    const uint32_t p = a[i];
    const uint32_t tri = (uint32_t)d[p] | ((uint32_t)d[p + 1] << 8) | ((uint32_t)d[p + 2] << 16);
    const int cap = cap_at(p, F);
    int best = 0;
    uint32_t best_dist = 0;
    if (cap >= kMinMatch) {
      for (int k = 1; k <= chain && k <= i; k++) {
        const uint32_t q = a[i - k];
        if (q >= p || p - q > (uint32_t)kWindow) break;
        if (((uint32_t)d[q] | ((uint32_t)d[q + 1] << 8) | ((uint32_t)d[q + 2] << 16)) != tri) break;
        const int len = common_prefix(d + q, d + p, cap);
        if (len > best) best = len, best_dist = p - q;
        if (best == cap) break;
      }
    }
    match[f * filt_stride + p] = best >= kMinMatch ? ((uint32_t)best << 16) | (best_dist - 1) : 0u;
  }
}

// the greedy walk: afterwards match[p] is 0 at a literal, (length, distance) at a match, kCovered inside one
__global__ __launch_bounds__(64) void pnglz_parse_kernel(long long nimages, long long F, long long filt_stride, uint32_t* __restrict__ match) {
  const long long chunks = (F + kChunk - 1) / kChunk, items = nimages * chunks;
  for (long long item = (long long)blockIdx.x * 64 + threadIdx.x; item < items; item += (long long)gridDim.x * 64) {
    const long long f = item / chunks;
    uint32_t* __restrict__ m = match + f * filt_stride;
    long long p = (item - f * chunks) * kChunk;
    const long long end = p + kChunk < F ? p + kChunk : F;
    while (p < end) {
      const uint32_t v = p + 2 < F ? m[p] : 0u;
      int len = (int)(v >> 16);
      if (len > end - p) len = 0;  // cannot happen: the cap keeps a match inside its chunk
      if (len >= kMinMatch) {
        for (int j = 1; j < len; j++) m[p + j] = kCovered;
        p += len;
      } else {
        m[p] = 0;
        p++;
      }
    }
  }
}

__global__ __launch_bounds__(256) void pnglz_tally_kernel(long long nimages, long long F, const uint8_t* __restrict__ filt, long long filt_stride,
                                                          const uint32_t* __restrict__ match, uint32_t* __restrict__ zeroed) {
  __shared__ uint32_t hist[kAll + 4];
  const int t = threadIdx.x;
  constexpr int kSpan = 256 * 16;
  const long long parts = (F + kSpan - 1) / kSpan, items = nimages * parts;
  for (long long item = blockIdx.x; item < items; item += gridDim.x) {
    const long long f = item / parts, first = (item - f * parts) * kSpan;
    for (int i = t; i < kAll + 4; i += 256) hist[i] = 0;
    __syncthreads();
    const uint8_t* __restrict__ d = filt + f * filt_stride;
    const uint32_t* __restrict__ m = match + f * filt_stride;
    uint32_t tokens = 0, matches = 0;
    for (int k = 0; k < 16; k++) {
      const long long p = first + k * 256 + t;
      if (p >= F) break;
      const uint32_t v = m[p];
      if (v == kCovered) continue;
      tokens++;
      if (v == 0) {
        atomicAdd(&hist[d[p]], 1u);
      } else {
        int ls, le, ln, ds, de, dn;
        length_symbol((int)(v >> 16), ls, le, ln);
        distance_symbol((int)(v & 0xffffu) + 1, ds, de, dn);
        atomicAdd(&hist[ls], 1u);
        atomicAdd(&hist[kLitLen + ds], 1u);
        matches++;
      }
    }
    if (tokens) atomicAdd(&hist[kAll], tokens);
    if (matches) atomicAdd(&hist[kAll + 1], matches);
    __syncthreads();
    uint32_t* __restrict__ g = zeroed + f * kZeroWords + kTokAt;
    for (int i = t; i < kAll + 2; i += 256)
      if (hist[i]) atomicAdd(&g[i], hist[i]);
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------- the codes and the form

__global__ __launch_bounds__(256) void pnglz_build_kernel(long long nimages, long long F, const uint32_t* __restrict__ zeroed, uint32_t* __restrict__ tab,
                                                          int32_t* __restrict__ form) {
  __shared__ Block H, L;  // Huffman-only, with matches
  __shared__ uint32_t meta[12];
  const int t = threadIdx.x;
  for (long long f = blockIdx.x; f < nimages; f += gridDim.x) {
    const uint32_t* __restrict__ z = zeroed + f * kZeroWords;
    __syncthreads();
    for (int i = t; i < kAll; i += 256) {
      H.hist[i] = i < 256 ? z[kHistAt + i] : i == kEob ? 1u : 0u;
      L.hist[i] = i == kEob ? 1u : z[kTokAt + i];
    }
    __syncthreads();
    huff_order(H.hist, kLitLen, H.work.order, t, 256);
    huff_order(L.hist, kLitLen, L.work.order, t, 256);
    __syncthreads();
    if (t == 0 || t == 64) build_block(t == 0 ? H : L);  // two waves, side by side
    __syncthreads();
    if (t == 0) {
      const long long stored = stored_bytes(F);
      const int take = (L.bytes < H.bytes && L.bytes < stored) ? MDCL_FORM_MATCHES : H.bytes < stored ? MDCL_FORM_HUFFMAN : MDCL_FORM_STORED;
      const Block& B = take == MDCL_FORM_MATCHES ? L : H;
      meta[0] = (uint32_t)take;
      meta[1] = B.hdr_bits;
      meta[2] = (uint32_t)(take == MDCL_FORM_STORED ? stored : B.bytes);
      meta[3] = (uint32_t)B.data_bits;
      meta[4] = (uint32_t)(B.data_bits >> 32);
      int32_t* __restrict__ fo = form + 4 * f;
      fo[0] = take, fo[1] = (int32_t)z[kCountAt], fo[2] = (int32_t)z[kCountAt + 1];
      fo[3] = (int32_t)(L.bytes < 0x7fffffffll ? L.bytes : 0x7fffffffll);
    }
    __syncthreads();
    const Block& B = meta[0] == MDCL_FORM_MATCHES ? L : H;
    uint32_t* __restrict__ o = tab + f * kTabWords;
    for (int i = t; i < kAll; i += 256) o[i] = B.codes[i];
    if (t < kHdrWords) o[kHdrAt + t] = B.hdr[t];
    if (t < 12) o[kMeta + t] = meta[t];
  }
}

// ---------------------------------------------------------------------------------------------------- bit offsets

// the bits of the tokens that start in one 16-position unit; lens[s] = the code length of symbol s (distances from 286)
__device__ __forceinline__ uint32_t unit_bits(const uint4 bytes, const uint4* __restrict__ m4, bool matches, int valid, const uint8_t* __restrict__ lens) {
  const uint32_t d[4] = {bytes.x, bytes.y, bytes.z, bytes.w};
  uint32_t bits = 0;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    uint4 mv = make_uint4(0, 0, 0, 0);
    if (matches) mv = m4[q];
    const uint32_t m[4] = {mv.x, mv.y, mv.z, mv.w};
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int k = 4 * q + r;
      if (k >= valid || m[r] == kCovered) continue;
      if (m[r] == 0) {
        bits += lens[(d[q] >> (8 * r)) & 255];
      } else {
        int ls, le, ln, ds, de, dn;
        length_symbol((int)(m[r] >> 16), ls, le, ln);
        distance_symbol((int)(m[r] & 0xffffu) + 1, ds, de, dn);
        bits += (uint32_t)(lens[ls] + ln + lens[kLitLen + ds] + dn);
      }
    }
  }
  return bits;
}

__global__ __launch_bounds__(1024) void pnglz_scan_kernel(long long nimages, long long F, const uint8_t* __restrict__ filt, long long filt_stride,
                                                          const uint32_t* __restrict__ match, const uint32_t* __restrict__ tab,
                                                          unsigned long long* __restrict__ offsets, uint8_t* out, long long slot_bytes) {
  __shared__ uint8_t lens[kAll + 4];
  const int t = threadIdx.x;
  const long long nunits = (F + 15) >> 4;
  for (long long f = blockIdx.x; f < nimages; f += gridDim.x) {
    const uint32_t* __restrict__ tb = tab + f * kTabWords;
    const uint32_t form = tb[kMeta];
    if (form == MDCL_FORM_STORED) continue;  // nothing is packed
    __syncthreads();
    if (t < kAll) lens[t] = (uint8_t)(tb[t] >> 16);
    const uint4* __restrict__ src = (const uint4*)(filt + f * filt_stride);
    const uint4* __restrict__ m4 = (const uint4*)(match + f * filt_stride);
    scan_units(slot_of(out, slot_bytes, f), tb[kMeta + 1], F, offsets + f * nunits, lens,
               [&](long long u, int valid) { return unit_bits(src[u], m4 + 4 * u, form == MDCL_FORM_MATCHES, valid, lens); });
  }
}

// ---------------------------------------------------------------------------------------------------- the stream

// Bits least significant first into 32-bit words.  The words are zero where nothing has been written; a run shares its first and
// its last word with its neighbours, and every word is OR-ed in with an integer atomic.
struct BitPacker {
  uint32_t* __restrict__ word;
  unsigned long long acc = 0;
  int n;
  __device__ __forceinline__ BitPacker(uint32_t* words, unsigned long long bit) : word(words + (bit >> 5)), n((int)(bit & 31)) {}
  __device__ __forceinline__ void operator()(uint32_t bits, int count) {  // count <= 16
    acc |= (unsigned long long)bits << n;
    n += count;
    if (n >= 32) {
      if ((uint32_t)acc) atomicOr(word, (uint32_t)acc);
      word++;
      acc >>= 32;
      n -= 32;
    }
  }
  __device__ __forceinline__ void operator()(uint32_t code) { (*this)(code & 0xffffu, (int)(code >> 16)); }
  __device__ __forceinline__ void finish() {
    if (n > 0 && (uint32_t)acc) atomicOr(word, (uint32_t)acc);
  }
};

__global__ __launch_bounds__(256) void pnglz_pack_kernel(long long nimages, long long F, int parts, const uint8_t* __restrict__ filt, long long filt_stride,
                                                         const uint32_t* __restrict__ match, const uint32_t* __restrict__ tab,
                                                         const unsigned long long* __restrict__ offsets, uint8_t* out, long long slot_bytes) {
  const int t = threadIdx.x;
  const long long nunits = (F + 15) >> 4;
  const long long items = nimages * parts;
  for (long long item = blockIdx.x; item < items; item += gridDim.x) {
    const long long f = item / parts;
    const int p = (int)(item - f * parts);
    const uint32_t* __restrict__ tb = tab + f * kTabWords;
    const uint8_t* __restrict__ src = filt + f * filt_stride;
    const Slot sl = slot_of(out, slot_bytes, f);
    const uint32_t form = tb[kMeta];
    if (form == MDCL_FORM_STORED) {
      pack_stored(sl, src, F, p, parts, t);
      continue;
    }
    const uint32_t* __restrict__ codes = tb;  // 316 words per image, read through the caches
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
        bp(codes[kEob]);
        bp.finish();
      }
    }
    const uint4* __restrict__ src16 = (const uint4*)src;
    const uint4* __restrict__ m4 = (const uint4*)(match + f * filt_stride);
    const unsigned long long* __restrict__ off = offsets + f * nunits;
    for (long long u = (long long)p * 256 + t; u < nunits; u += (long long)parts * 256) {
      const uint4 v = src16[u];
      const long long rem = F - u * 16;
      const int valid = rem < 16 ? (int)rem : 16;
      const uint32_t d[4] = {v.x, v.y, v.z, v.w};
      BitPacker bp(sl.words, off[u]);
#pragma unroll
      for (int q = 0; q < 4; q++) {
        uint4 mv = make_uint4(0, 0, 0, 0);
        if (form == MDCL_FORM_MATCHES) mv = m4[4 * u + q];
        const uint32_t m[4] = {mv.x, mv.y, mv.z, mv.w};
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int k = 4 * q + r;
          if (k >= valid || m[r] == kCovered) continue;
          if (m[r] == 0) {
            bp(codes[(d[q] >> (8 * r)) & 255]);
          } else {
            int ls, le, ln, ds, de, dn;
            length_symbol((int)(m[r] >> 16), ls, le, ln);
            distance_symbol((int)(m[r] & 0xffffu) + 1, ds, de, dn);
            bp(codes[ls]);
            bp((uint32_t)le, ln);
            bp(codes[kLitLen + ds]);
            bp((uint32_t)de, dn);
          }
        }
      }
      bp.finish();
    }
  }
}

__global__ __launch_bounds__(256) void pnglz_finish_kernel(long long nimages, long long F, const uint8_t* __restrict__ head, const uint32_t* __restrict__ zeroed,
                                                           const uint32_t* __restrict__ tab, uint8_t* out, long long slot_bytes, int32_t* __restrict__ sizes,
                                                           int32_t* __restrict__ crc_len) {
  finish_files<Layout>(nimages, F, head, zeroed, tab, out, slot_bytes, sizes, crc_len);
}

__global__ __launch_bounds__(256) void pnglz_crc_kernel(long long nimages, const uint32_t* __restrict__ tab, const uint32_t* __restrict__ crc, uint8_t* out,
                                                        long long slot_bytes) {
  crc_bytes<Layout>(nimages, tab, crc, out, slot_bytes);
}

// ---------------------------------------------------------------------------------------------------- host side

int bpp_of(int kind) { return kind == MDCL_GRAY8 ? 1 : kind == MDCL_GRAY16 ? 2 : kind == MDCL_RGB8 ? 3 : 0; }

}  // namespace

struct mdcl_encoder {
  int device = -1, w = 0, h = 0, kind = 0, bpp = 0, filter = 0, chain = 0, max_images = 0;
  long long F = 0, nunits = 0;
  uint8_t* d_head = nullptr;
  uint8_t* d_filt = nullptr;
  uint32_t* d_idx_a = nullptr;  // the positions in trigram order
  uint32_t* d_idx_b = nullptr;  // the sort's other buffer, then every position's match
  unsigned long long* d_offsets = nullptr;
  uint32_t* d_zeroed = nullptr;
  uint32_t* d_tab = nullptr;
  int32_t* d_form = nullptr;
  int32_t* d_crc_len = nullptr;
  uint32_t* d_crc = nullptr;
  uint8_t* d_out = nullptr;  // mdcl_output_device: allocated on demand
  int32_t* d_sizes = nullptr;
  bool profile = false, timed = false;
  hipEvent_t ev[MDCL_KERNELS + 1] = {};
};

namespace {

void destroy(mdcl_encoder* enc) {
  if (!enc) return;
  {
    DeviceGuard dg(enc->device);
    (void)hipFree(enc->d_head);
    (void)hipFree(enc->d_filt);
    (void)hipFree(enc->d_idx_a);
    (void)hipFree(enc->d_idx_b);
    (void)hipFree(enc->d_offsets);
    (void)hipFree(enc->d_zeroed);
    (void)hipFree(enc->d_tab);
    (void)hipFree(enc->d_form);
    (void)hipFree(enc->d_crc_len);
    (void)hipFree(enc->d_crc);
    (void)hipFree(enc->d_out);
    (void)hipFree(enc->d_sizes);
    for (hipEvent_t e : enc->ev)
      if (e) (void)hipEventDestroy(e);
  }
  delete enc;
}

template <typename T, int BPP>
int encode(const char* who, mdcl_encoder* e, const T* d_images, int64_t stride, int nimages, uint8_t* d_out, int64_t slot_bytes, int32_t* d_sizes, void* stream) {
  constexpr int kPerElement = BPP == 3 ? 3 : 1;        // an RGB stride is given in bytes, a gray one in elements
  constexpr size_t kAlign = BPP == 3 ? 1 : sizeof(T);  // RGB pixels are bytes
  static const char* const kinds[4] = {"", "8-bit gray", "16-bit gray", "8-bit RGB"};
  if (!e) return fail(MDCL_ERR_ARG, "%s: encoder is null", who);
  if (bpp_of(e->kind) != BPP) return fail(MDCL_ERR_ARG, "%s: the encoder was made for %s images", who, kinds[bpp_of(e->kind)]);
  if (nimages < 0 || nimages > e->max_images) return fail(MDCL_ERR_ARG, "%s: %d images, the encoder was made for 0..%d", who, nimages, e->max_images);
  if (nimages == 0) return MDCL_OK;
  if (!d_images || !d_out || !d_sizes) return fail(MDCL_ERR_ARG, "%s: null device pointer", who);
  if ((uintptr_t)d_images % kAlign) return fail(MDCL_ERR_ARG, "%s: d_images %p is not aligned to its %zu-byte elements", who, (const void*)d_images, sizeof(T));
  if (stride < (int64_t)e->w * e->h * kPerElement)
    return fail(MDCL_ERR_ARG, "%s: stride %lld is below %d x %d%s", who, (long long)stride, e->w, e->h, kPerElement == 3 ? " x 3 bytes" : "");
  const int64_t bound = bound_of(e->w, e->h, BPP);
  if (slot_bytes < bound)
    return fail(MDCL_ERR_SIZE, "%s: slot_bytes %lld is below mdcl_png_bound(%d, %d, %d) = %lld", who, (long long)slot_bytes, e->w, e->h, e->kind, (long long)bound);
  DeviceGuard dg(e->device);
  hipStream_t s = (hipStream_t)stream;
  const long long n = nimages, F = e->F, fs = e->nunits * 16;
  int stage = 0;
  auto mark = [&]() {
    if (e->profile) (void)hipEventRecord(e->ev[stage++], s);
  };
  mark();
  if (hipMemsetAsync(e->d_zeroed, 0, (size_t)n * kZeroWords * 4, s) != hipSuccess)
    return fail(MDCL_ERR_HIP, "%s: clearing the histograms failed: %s", who, hipGetErrorString(hipGetLastError()));
  const long long groups = ((long long)e->h + kRowsPerGroup - 1) / kRowsPerGroup;
  const long long parts = pack_parts(n, e->nunits);
  const long long chunks = (F + kChunk - 1) / kChunk;
  pnglz_filter_kernel<T, BPP><<<grid_for(n * groups), 256, 0, s>>>(d_images, (long long)stride, n, e->w, e->h, e->filter, e->d_filt, fs, e->d_zeroed);
  mark();
  pnglz_order_kernel<<<grid_for(n), 1024, 0, s>>>(n, F, e->d_filt, fs, e->d_idx_a, e->d_idx_b);
  mark();
  pnglz_match_kernel<<<grid_for(n * ((F + 255) / 256)), 256, 0, s>>>(n, F, e->chain, e->d_filt, fs, e->d_idx_a, e->d_idx_b);
  mark();
  pnglz_parse_kernel<<<grid_for((n * chunks + 63) / 64), 64, 0, s>>>(n, F, fs, e->d_idx_b);
  mark();
  pnglz_tally_kernel<<<grid_for(n * ((F + 4095) / 4096)), 256, 0, s>>>(n, F, e->d_filt, fs, e->d_idx_b, e->d_zeroed);
  mark();
  pnglz_build_kernel<<<grid_for(n), 256, 0, s>>>(n, F, e->d_zeroed, e->d_tab, e->d_form);
  mark();
  pnglz_scan_kernel<<<grid_for(n), 1024, 0, s>>>(n, F, e->d_filt, fs, e->d_idx_b, e->d_tab, e->d_offsets, d_out, (long long)slot_bytes);
  mark();
  pnglz_pack_kernel<<<grid_for(n * parts), 256, 0, s>>>(n, F, (int)parts, e->d_filt, fs, e->d_idx_b, e->d_tab, e->d_offsets, d_out, (long long)slot_bytes);
  mark();
  pnglz_finish_kernel<<<grid_for((n + 255) / 256), 256, 0, s>>>(n, F, e->d_head, e->d_zeroed, e->d_tab, d_out, (long long)slot_bytes, d_sizes, e->d_crc_len);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(MDCL_ERR_HIP, "%s: launch failed: %s", who, hipGetErrorString(err));
  if (mdcz_crc32_device(d_out + 37, slot_bytes, e->d_crc_len, n, e->d_crc, stream) != MDCZ_OK)
    return fail(MDCL_ERR_HIP, "%s: the IDAT checksum failed: %s", who, mdcz_last_error());
  pnglz_crc_kernel<<<grid_for((n + 255) / 256), 256, 0, s>>>(n, e->d_tab, e->d_crc, d_out, (long long)slot_bytes);
  mark();
  e->timed = e->profile;
  if ((err = hipGetLastError()) != hipSuccess) return fail(MDCL_ERR_HIP, "%s: launch failed: %s", who, hipGetErrorString(err));
  return MDCL_OK;
}

}  // namespace

extern "C" {

int64_t mdcl_png_bound(int w, int h, int kind) { return bound_of(w, h, bpp_of(kind)); }

const char* mdcl_last_error(void) { return g_error; }

int mdcl_create(int device, int w, int h, int kind, int filter, int chain, int max_images, mdcl_encoder** out) {
  const char* who = "mdcl_create";
  if (!out) return fail(MDCL_ERR_ARG, "%s: out is null", who);
  *out = nullptr;
  const int bpp = bpp_of(kind);
  if (!bpp) return fail(MDCL_ERR_ARG, "%s: kind %d is none of MDCL_GRAY8, MDCL_GRAY16, MDCL_RGB8", who, kind);
  if (filter < 0 || filter > MDCL_FILTER_ADAPTIVE) return fail(MDCL_ERR_ARG, "%s: filter %d is outside 0..%d", who, filter, MDCL_FILTER_ADAPTIVE);
  if (chain < 1 || chain > MDCL_MAX_CHAIN) return fail(MDCL_ERR_ARG, "%s: chain %d is outside 1..%d", who, chain, MDCL_MAX_CHAIN);
  if (max_images < 1) return fail(MDCL_ERR_ARG, "%s: max_images %d is below 1", who, max_images);
  if (w < 1 || h < 1) return fail(MDCL_ERR_SIZE, "%s: %d x %d: width and height start at 1", who, w, h);
  if (bound_of(w, h, bpp) < 0) return fail(MDCL_ERR_SIZE, "%s: a %d x %d image of %d bytes per pixel passes 2^31 - 1 bytes (sizes are int32_t)", who, w, h, bpp);
  const long long F = (1 + (long long)w * bpp) * h, nunits = (F + 15) / 16;
  const long long per_image = 152 * nunits + kSmallBytes;
  if (per_image > (1ll << 40) / max_images)
    return fail(MDCL_ERR_SIZE, "%s: %d images x %lld bytes of scratch pass 2^40 bytes", who, max_images, per_image);
  if (int rc = resolve_device(who, &device)) return rc;
  DeviceGuard dg(device);
  mdcl_encoder* e = new (std::nothrow) mdcl_encoder;
  if (!e) return fail(MDCL_ERR_NOMEM, "%s: out of host memory", who);
  e->device = device, e->w = w, e->h = h, e->kind = kind, e->bpp = bpp, e->filter = filter, e->chain = chain, e->max_images = max_images;
  e->F = F, e->nunits = nunits;
  const size_t n = (size_t)max_images;
  if (hipMalloc((void**)&e->d_head, 48) != hipSuccess || hipMalloc((void**)&e->d_filt, n * (size_t)nunits * 16) != hipSuccess ||
      hipMalloc((void**)&e->d_idx_a, n * (size_t)nunits * 64) != hipSuccess || hipMalloc((void**)&e->d_idx_b, n * (size_t)nunits * 64) != hipSuccess ||
      hipMalloc((void**)&e->d_offsets, n * (size_t)nunits * 8) != hipSuccess || hipMalloc((void**)&e->d_zeroed, n * kZeroWords * 4) != hipSuccess ||
      hipMalloc((void**)&e->d_tab, n * kTabWords * 4) != hipSuccess || hipMalloc((void**)&e->d_form, n * 16) != hipSuccess ||
      hipMalloc((void**)&e->d_crc_len, n * 4) != hipSuccess || hipMalloc((void**)&e->d_crc, n * 4) != hipSuccess) {
    (void)hipGetLastError();
    destroy(e);
    return fail(MDCL_ERR_NOMEM, "%s: could not allocate the scratch arrays of %d images of %d x %d", who, max_images, w, h);
  }
  uint8_t head[48];
  png_head(head, w, h, kind == MDCL_GRAY16 ? 16 : 8, kind == MDCL_RGB8 ? 2 : 0);  // colour type: truecolour or gray
  if (hipMemcpy(e->d_head, head, sizeof head, hipMemcpyHostToDevice) != hipSuccess) {
    destroy(e);
    return fail(MDCL_ERR_HIP, "%s: copying the header failed", who);
  }
  *out = e;
  return MDCL_OK;
}

void mdcl_destroy(mdcl_encoder* enc) { destroy(enc); }

int mdcl_encode_u8_device(mdcl_encoder* enc, const uint8_t* d_images, int64_t stride, int nimages, uint8_t* d_out, int64_t slot_bytes, int32_t* d_sizes,
                          void* stream) {
  return encode<uint8_t, 1>("mdcl_encode_u8_device", enc, d_images, stride, nimages, d_out, slot_bytes, d_sizes, stream);
}

int mdcl_encode_u16_device(mdcl_encoder* enc, const uint16_t* d_images, int64_t stride, int nimages, uint8_t* d_out, int64_t slot_bytes, int32_t* d_sizes,
                           void* stream) {
  return encode<uint16_t, 2>("mdcl_encode_u16_device", enc, d_images, stride, nimages, d_out, slot_bytes, d_sizes, stream);
}

int mdcl_encode_f32_device(mdcl_encoder* enc, const float* d_images, int64_t stride, int nimages, uint8_t* d_out, int64_t slot_bytes, int32_t* d_sizes,
                           void* stream) {
  return encode<float, 1>("mdcl_encode_f32_device", enc, d_images, stride, nimages, d_out, slot_bytes, d_sizes, stream);
}

int mdcl_encode_rgb8_device(mdcl_encoder* enc, const uint8_t* d_images, int64_t stride_bytes, int nimages, uint8_t* d_out, int64_t slot_bytes,
                            int32_t* d_sizes, void* stream) {
  return encode<Rgb8, 3>("mdcl_encode_rgb8_device", enc, (const Rgb8*)d_images, stride_bytes, nimages, d_out, slot_bytes, d_sizes, stream);
}

int mdcl_output_device(mdcl_encoder* enc, uint8_t** d_out, int64_t* slot_bytes, int32_t** d_sizes) {
  return output_device("mdcl_output_device", enc, d_out, slot_bytes, d_sizes);
}

int mdcl_form_device(mdcl_encoder* enc, int32_t* d_form, int nimages, void* stream) {
  const char* who = "mdcl_form_device";
  if (!enc) return fail(MDCL_ERR_ARG, "%s: encoder is null", who);
  if (nimages < 0 || nimages > enc->max_images) return fail(MDCL_ERR_ARG, "%s: %d images, the encoder was made for 0..%d", who, nimages, enc->max_images);
  if (nimages == 0) return MDCL_OK;
  if (!d_form) return fail(MDCL_ERR_ARG, "%s: d_form is null", who);
  DeviceGuard dg(enc->device);
  if (hipMemcpyAsync(d_form, enc->d_form, (size_t)nimages * 16, hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess)
    return fail(MDCL_ERR_HIP, "%s: the copy failed: %s", who, hipGetErrorString(hipGetLastError()));
  return MDCL_OK;
}

int mdcl_profile(mdcl_encoder* enc, int on) {
  if (!enc) return fail(MDCL_ERR_ARG, "mdcl_profile: encoder is null");
  if (on && !enc->ev[0]) {
    DeviceGuard dg(enc->device);
    for (hipEvent_t& e : enc->ev)
      if (hipEventCreate(&e) != hipSuccess) return fail(MDCL_ERR_HIP, "mdcl_profile: hipEventCreate failed");
  }
  enc->profile = on != 0;
  return MDCL_OK;
}

int mdcl_kernel_ms(mdcl_encoder* enc, float* ms) {
  if (!enc || !ms) return fail(MDCL_ERR_ARG, "mdcl_kernel_ms: null argument");
  if (!enc->timed) return fail(MDCL_ERR_ARG, "mdcl_kernel_ms: no encode call has been timed (mdcl_profile)");
  DeviceGuard dg(enc->device);
  if (hipEventSynchronize(enc->ev[MDCL_KERNELS]) != hipSuccess) return fail(MDCL_ERR_HIP, "mdcl_kernel_ms: waiting for the call failed");
  for (int k = 0; k < MDCL_KERNELS; k++)
    if (hipEventElapsedTime(&ms[k], enc->ev[k], enc->ev[k + 1]) != hipSuccess) return fail(MDCL_ERR_HIP, "mdcl_kernel_ms: reading an event failed");
  return MDCL_OK;
}

}  // extern "C"
