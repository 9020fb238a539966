// What the device PNG encoders share beside the block builder (png_block.h): mdc_pngw.hip (libmdc_pngw.so, libmdc_pngw_rgb.so) and
// mdc_pnglz.hip (libmdc_pnglz.so) include this file, and each keeps its own __global__ kernels under its own names, its own layout
// of the per-image words, its own BitPacker and its own way of fetching the codes in the pack kernel.  Everything here is in the
// including unit's anonymous namespace: no library gains a symbol or a dependency.
//   a layout type `Lay`      the per-image word offsets of a library as constexpr members: zero_words (the words cleared per call), in
//                            them adler_at (the Adler sums, two 64-bit words); tab_words (the build kernel's table), in it meta_at
//                            (0 form, 1 header bits, 2 stream bytes, 3/4 data bits)
//   device                   the sample, filter and wave helpers of the filter kernels; Slot / slot_of; scan_units (the scan kernel's
//                            clearing, wave scan and carry over a "bits of unit u" functor); pack_stored (the pack kernel's stored-block
//                            gather); finish_files and crc_bytes (the bodies of the finish and crc kernels)
//   host                     (codec_host.h: g_error / fail, DeviceGuard, resolve_device) crc32_host, put_be32, bound_of, grid_for, png_head, pack_parts, output_device
// The filter kernel's 80-line body is not here: as a device function template it compiles to other registers than as the kernel itself
// (79 instead of 69 VGPRs for the RGB pixel, past the 72 the tests allow), so each unit keeps its copy and the helpers are shared.
// Nor are the pack kernel's header bits (pngw_pack_kernel came out one instruction longer with them here) and mdc_pngw.hip's
// Huffman-only block builder (it says why).
#ifndef MDC_PNG_ENCODE_CORE_H
#define MDC_PNG_ENCODE_CORE_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "codec_host.h"

#define PNG_HD __host__ __device__ __forceinline__
#include "png_block.h"

namespace {

using namespace png;

constexpr int kStreamAt = 43;        // signature 8, IHDR 25, length 4, "IDAT" 4, zlib header 2
constexpr int kRowsPerGroup = 16;
constexpr int kMaxGrid = 8192;
constexpr uint32_t kAdlerMod = 65521;

// ---------------------------------------------------------------------------------------------------- pixels -> filtered bytes

__device__ __forceinline__ int sample_of(uint8_t v) { return v; }
__device__ __forceinline__ int sample_of(uint16_t v) { return v; }
struct Rgb8 {  // one pixel of an 8-bit RGB image in file order: the filter distance is the pixel, as it is the sample of a gray image
  uint8_t r, g, b;
};
__device__ __forceinline__ int sample_of(Rgb8 v) { return ((int)v.r << 16) | ((int)v.g << 8) | (int)v.b; }
__device__ __forceinline__ int sample_of(float v) {  // as mdcj_encode_f32_device: cv::Mat::convertTo(CV_8U)
  const float r = fminf(fmaxf(rintf(v), 0.0f), 255.0f);
  return v != v ? 0 : (int)r;
}

__device__ __forceinline__ int paeth(int a, int b, int c) {
  const int p = a + b - c;
  const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__device__ __forceinline__ int filter_byte(int type, int x, int a, int b, int c) {
  const int pred = type == 0 ? 0 : type == 1 ? a : type == 2 ? b : type == 3 ? ((a + b) >> 1) : paeth(a, b, c);
  return (x - pred) & 255;
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// image f of a batch: `stride` elements on, for RGB pixels `stride` bytes on (three-byte pixels, images at any byte distance)
template <typename T>
__device__ __forceinline__ const T* image_at(const T* images, long long f, long long stride) { return images + f * stride; }
__device__ __forceinline__ const Rgb8* image_at(const Rgb8* images, long long f, long long stride) {
  return (const Rgb8*)((const uint8_t*)images + f * stride);
}

// ---------------------------------------------------------------------------------------------------- bit offsets

struct Slot {  // where an image's DEFLATE stream goes: 32-bit words from the 4-byte boundary at or below byte 43 of the file
  uint8_t* stream;
  uint32_t* words;
  uint32_t shift;
};

__device__ __forceinline__ Slot slot_of(uint8_t* out, long long slot_bytes, long long f) {
  Slot s;
  s.stream = out + f * slot_bytes + kStreamAt;
  const uint32_t mis = (uint32_t)((uintptr_t)s.stream & 3);
  s.words = (uint32_t*)(s.stream - mis);
  s.shift = 8 * mis;
  return s;
}

// 1024 lanes, one image: unit(u, valid) = the bits of the tokens that start in the 16-position unit u, of which `valid` positions
// are inside the image; off[u] = the unit's bit offset from sl.words.  The words that the pack kernel will OR into are cleared
// here.  lens (LDS) is filled by the caller, who has put a barrier before its own writes; lens[kEob] is read after a barrier.
template <typename UnitBits>
__device__ __forceinline__ void scan_units(const Slot& sl, uint32_t hdr_bits, long long F, unsigned long long* off, const uint8_t* lens,
                                           UnitBits unit) {
  __shared__ uint32_t wave_total[16];
  __shared__ unsigned long long carry_s;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const long long nunits = (F + 15) >> 4;
  const unsigned long long start = (unsigned long long)sl.shift + hdr_bits;
  for (long long wd = t; wd < (long long)((start + 31) >> 5); wd += 1024) sl.words[wd] = 0;
  if (t == 0) carry_s = start;
  __syncthreads();
  for (long long first = 0; first < nunits; first += 1024) {
    const long long u = first + t;
    uint32_t bits = 0;
    if (u < nunits) {
      const long long rem = F - u * 16;
      bits = unit(u, rem < 16 ? (int)rem : 16);
    }
    uint32_t inc = bits;  // inclusive scan inside the wave: at most 1024 * 768
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t other = __shfl_up(inc, o, 64);
      if (lane >= o) inc += other;
    }
    if (lane == 63) wave_total[wave] = inc;
    __syncthreads();
    unsigned long long before = carry_s;
    for (int k = 0; k < wave; k++) before += wave_total[k];
    const unsigned long long at = before + inc - bits;
    if (u < nunits) {
      off[u] = at;
      for (unsigned long long wd = (at + 31) >> 5; wd < ((at + bits + 31) >> 5); wd++) sl.words[wd] = 0;
    }
    __syncthreads();
    if (t == 1023) carry_s = before + inc;
    __syncthreads();
  }
  if (t == 0) {  // the end-of-block code
    const unsigned long long at = carry_s;
    for (unsigned long long wd = (at + 31) >> 5; wd < ((at + lens[kEob] + 31) >> 5); wd++) sl.words[wd] = 0;
  }
}

// ---------------------------------------------------------------------------------------------------- the stream

// part p of `parts` of a stored image, 256 lanes: byte idx of the stream is header byte r < 5 or data byte r - 5 of block idx / 65540
__device__ __forceinline__ void pack_stored(const Slot& sl, const uint8_t* __restrict__ src, long long F, int p, int parts, int t) {
  const long long total = stored_bytes(F);
  const int last = (int)((F - 1) / 65535);
  for (long long idx = (long long)p * 256 + t; idx < total; idx += (long long)parts * 256) {
    const int b = (int)(idx / 65540), r = (int)(idx - (long long)b * 65540);
    uint8_t v;
    if (r >= 5) {
      v = src[(long long)b * 65535 + (r - 5)];
    } else {
      const long long left = F - (long long)b * 65535;
      const uint32_t len = left < 65535 ? (uint32_t)left : 65535u;
      v = r == 0 ? (uint8_t)(b == last) : r == 1 ? (uint8_t)len : r == 2 ? (uint8_t)(len >> 8) : r == 3 ? (uint8_t)~len : (uint8_t)(~len >> 8);
    }
    sl.stream[idx] = v;
  }
}

// one lane per image; head: 33 bytes (signature, IHDR with its CRC) and the 12 of IEND
template <typename Lay>
__device__ __forceinline__ void finish_files(long long nimages, long long F, const uint8_t* __restrict__ head, const uint32_t* __restrict__ zeroed,
                                             const uint32_t* __restrict__ tab, uint8_t* out, long long slot_bytes, int32_t* __restrict__ sizes,
                                             int32_t* __restrict__ crc_len) {
  for (long long f = (long long)blockIdx.x * 256 + threadIdx.x; f < nimages; f += (long long)gridDim.x * 256) {
    uint8_t* __restrict__ o = out + f * slot_bytes;
    const uint32_t stream = tab[f * Lay::tab_words + Lay::meta_at + 2];
    const uint32_t idat = 2 + stream + 4;
    for (int i = 0; i < 33; i++) o[i] = head[i];
    for (int i = 0; i < 4; i++) o[33 + i] = (uint8_t)(idat >> (24 - 8 * i));
    o[37] = 'I', o[38] = 'D', o[39] = 'A', o[40] = 'T', o[41] = 0x78, o[42] = 0x01;
    const unsigned long long* __restrict__ sums = (const unsigned long long*)(zeroed + f * Lay::zero_words + Lay::adler_at);
    const uint32_t s1 = (uint32_t)((1 + sums[0]) % kAdlerMod), s2 = (uint32_t)(((unsigned long long)F + sums[1]) % kAdlerMod);
    const uint32_t adler = (s2 << 16) | s1;
    uint8_t* __restrict__ e = o + kStreamAt + stream;
    for (int i = 0; i < 4; i++) e[i] = (uint8_t)(adler >> (24 - 8 * i));
    for (int i = 0; i < 12; i++) e[8 + i] = head[33 + i];
    sizes[f] = (int32_t)(57 + 6 + stream);
    crc_len[f] = (int32_t)(4 + idat);
  }
}

template <typename Lay>
__device__ __forceinline__ void crc_bytes(long long nimages, const uint32_t* __restrict__ tab, const uint32_t* __restrict__ crc, uint8_t* out,
                                          long long slot_bytes) {
  for (long long f = (long long)blockIdx.x * 256 + threadIdx.x; f < nimages; f += (long long)gridDim.x * 256) {
    uint8_t* __restrict__ e = out + f * slot_bytes + kStreamAt + tab[f * Lay::tab_words + Lay::meta_at + 2] + 4;
    const uint32_t c = crc[f];
    for (int i = 0; i < 4; i++) e[i] = (uint8_t)(c >> (24 - 8 * i));
  }
}

// ---------------------------------------------------------------------------------------------------- host side

uint32_t crc32_host(const uint8_t* p, size_t n) {
  uint32_t c = 0xFFFFFFFFu;
  for (size_t i = 0; i < n; i++) {
    c ^= p[i];
    for (int b = 0; b < 8; b++) c = (c >> 1) ^ ((c & 1) ? 0xEDB88320u : 0u);
  }
  return ~c;
}

void put_be32(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)(v >> 24), p[1] = (uint8_t)(v >> 16), p[2] = (uint8_t)(v >> 8), p[3] = (uint8_t)v;
}

// the stored form's size for rows of 1 + w * bpp bytes; -1 past 2^31 - 1
int64_t bound_of(int w, int h, int bpp) {
  if (w < 1 || h < 1 || bpp < 1) return -1;
  const int64_t row = 1 + (int64_t)w * bpp;  // < 2^33
  if (row > INT32_MAX / (int64_t)h) return -1;
  const int64_t bound = 57 + 6 + stored_bytes(row * h);
  return bound > INT32_MAX ? -1 : bound;
}

int grid_for(long long items) { return (int)(items < 1 ? 1 : items > kMaxGrid ? kMaxGrid : items); }

// what finish_files copies: signature and IHDR with its CRC (33 bytes), then IEND (12); compression, filter method, interlace: 0
void png_head(uint8_t head[48], int w, int h, int bit_depth, int colour_type) {
  const uint8_t start[16] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n', 0, 0, 0, 13, 'I', 'H', 'D', 'R'};
  const uint8_t iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xae, 0x42, 0x60, 0x82};
  memset(head, 0, 48);
  memcpy(head, start, 16);
  put_be32(head + 16, (uint32_t)w);
  put_be32(head + 20, (uint32_t)h);
  head[24] = (uint8_t)bit_depth;
  head[25] = (uint8_t)colour_type;
  put_be32(head + 29, crc32_host(head + 12, 17));
  memcpy(head + 33, iend, 12);
}

// the pack kernel's workgroups per image: 1024 units each, more when few images would not fill the device
long long pack_parts(long long n, long long nunits) {
  long long parts = (nunits + 1023) / 1024;
  if (n * parts < 1024) parts = (1024 + n - 1) / n;
  if (parts > (nunits + 255) / 256) parts = (nunits + 255) / 256;
  return parts > 4096 ? 4096 : parts;
}

// an encoder's own output slots, allocated on the first call; Encoder has device, w, h, bpp, max_images, d_out, d_sizes
template <typename Encoder>
int output_device(const char* who, Encoder* enc, uint8_t** d_out, int64_t* slot_bytes, int32_t** d_sizes) {
  if (!enc || !d_out || !slot_bytes || !d_sizes) return fail(kErrArg, "%s: null argument", who);
  const int64_t bound = bound_of(enc->w, enc->h, enc->bpp);
  if (!enc->d_out) {
    DeviceGuard dg(enc->device);
    uint8_t* o = nullptr;
    int32_t* z = nullptr;
    if (hipMalloc((void**)&o, (size_t)bound * (size_t)enc->max_images) != hipSuccess || hipMalloc((void**)&z, (size_t)enc->max_images * sizeof(int32_t)) != hipSuccess) {
      (void)hipGetLastError();
      (void)hipFree(o);
      return fail(kErrNoMem, "%s: could not allocate %d slots of %lld bytes", who, enc->max_images, (long long)bound);
    }
    enc->d_out = o, enc->d_sizes = z;
  }
  *d_out = enc->d_out, *slot_bytes = bound, *d_sizes = enc->d_sizes;
  return 0;  // MDCP_OK, MDCL_OK
}

}  // namespace
#endif  // MDC_PNG_ENCODE_CORE_H
