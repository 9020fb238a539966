// libmdc_jenc.so -- baseline JPEG encoder for device-resident grayscale frames (include/mdc_jenc.h), gfx950.
// A library of its own: no mdc_ctx, nothing of libmdc_hip.so; functions take a device and a stream.
//
// One call encodes a batch of frames in five launches, all integer, all deterministic (a sixth kernel, jenc_gather_kernel, serves
// mdcj_fetch: the files back to back, so that one copy brings them to the host):
//   jenc_fdct_quant_kernel  pixels -> quantised coefficients, zigzag order, int16 (8 threads per 8x8 block, through LDS)
//   jenc_count_kernel       one thread per block: the number of bits its Huffman code takes
//   jenc_scan_kernel        one workgroup per frame: exclusive scan of the bit counts -> each block's bit offset; zeroes the
//                           frame's part of the bit stream that will be written
//   jenc_pack_kernel        one thread per block: its code words at its bit offset (integer atomicOr where a 32-bit word is
//                           shared with a neighbour block, plain stores inside)
//   jenc_stuff_kernel       one workgroup per frame: header, the stream's bytes with 0x00 after every 0xFF (a scan over
//                           bytes), the 1-bit padding of the last byte, EOI, and the length
// The DC difference needs only the previous block's coefficient, which the first kernel has written, so blocks are independent.
// No kernel keeps a runtime-indexed per-thread array: coefficients live in registers with static indices or in LDS.
#include "../../include/mdc_jenc.h"

#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <new>

namespace {

constexpr int kHeaderBytes = 328;
constexpr int kBitsPerBlockMax = 20 + 63 * 26;  // include/mdc_jenc.h: the bound's derivation
constexpr int kGroupBlocks = 32;                // 8x8 blocks per workgroup of the DCT kernel (8 threads each)
constexpr int kLdsBlockStride = 72;             // dwords between blocks in LDS: 64 + 8, so that a column read meets 32 banks
constexpr int kStuffChunk = 16384;              // stream bytes per iteration of the stuffing workgroup (16 per thread)

// ITU-T T.81 Annex K.1, luminance, natural order
const uint8_t kBaseQ[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                            18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101,
                            72, 92, 95, 98, 112, 100, 103, 99};
// natural index of the k-th coefficient in zigzag order
const uint8_t kZigzag[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                             35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
// zigzag position of natural index n (the inverse of kZigzag)
__constant__ uint8_t kZigzagOfNatural[64] = {0, 1, 5, 6, 14, 15, 27, 28, 2, 4, 7, 13, 16, 26, 29, 42, 3, 8, 12, 17, 25, 30, 41, 43, 9, 11, 18, 24, 31, 40, 44, 53,
                                             10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61,
                                             35, 36, 48, 49, 57, 58, 62, 63};
// Annex K.3: codes per length 1..16, then the symbols in code order
const uint8_t kDcBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
const uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t kAcBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
const uint8_t kAcVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1,
    0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
    0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a,
    0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3,
    0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

// The encoder's constant tables in device memory, one allocation.  A Huffman entry is (length << 16) | code.
struct DeviceTables {
  uint32_t ac[256];
  uint32_t dc[16];
  uint16_t qdiv[64];  // 8 * q, natural order
  uint8_t header[kHeaderBytes];
};

// ---------------------------------------------------------------------------------------------------- pixels -> coefficients

// cv::Mat::convertTo(CV_8U) of a float, then the level shift
__device__ __forceinline__ int level_of(float v) {
  const float r = fminf(fmaxf(rintf(v), 0.0f), 255.0f);
  return (v != v ? 0 : (int)r) - 128;
}
__device__ __forceinline__ int level_of(uint8_t v) { return (int)v - 128; }

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// One pass of jfdctint.c over eight values (CONST_BITS 13, PASS1_BITS 2), in place.  FIRST: the row pass.
template <bool FIRST>
__device__ __forceinline__ void fdct_pass(int (&d)[8]) {
  constexpr int N = FIRST ? 13 - 2 : 13 + 2;
  const int tmp0 = d[0] + d[7], tmp7 = d[0] - d[7], tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
  const int tmp2 = d[2] + d[5], tmp5 = d[2] - d[5], tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
  const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  d[0] = FIRST ? (tmp10 + tmp11) << 2 : descale(tmp10 + tmp11, 2);
  d[4] = FIRST ? (tmp10 - tmp11) << 2 : descale(tmp10 - tmp11, 2);
  const int y1 = (tmp12 + tmp13) * 4433;
  d[2] = descale(y1 + tmp13 * 6270, N);
  d[6] = descale(y1 + tmp12 * (-15137), N);
  int z1 = tmp4 + tmp7, z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
  const int z5 = (z3 + z4) * 9633;
  const int t4 = tmp4 * 2446, t5 = tmp5 * 16819, t6 = tmp6 * 25172, t7 = tmp7 * 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 = z3 * (-16069) + z5;
  z4 = z4 * (-3196) + z5;
  d[7] = descale(t4 + z1 + z3, N);
  d[5] = descale(t5 + z2 + z4, N);
  d[3] = descale(t6 + z2 + z3, N);
  d[1] = descale(t7 + z1 + z4, N);
}

// grid (ceil(nblocks / 32), frames of this launch), 256 threads: thread t works on block t / 8 of the group, first on column
// t % 8 (the load: a wave reads 8 blocks x 8 columns = 64 consecutive pixels of a row), then on row t % 8, then on column t % 8.
template <typename T>
__global__ __launch_bounds__(256) void jenc_fdct_quant_kernel(const T* __restrict__ frames, long long frame_stride, int frame0, int w, int h, int bw,
                                                              int nblocks, const uint16_t* __restrict__ qdiv, int16_t* __restrict__ coef) {
  __shared__ __align__(16) int ws[kGroupBlocks * kLdsBlockStride];
  __shared__ __align__(16) int16_t zq[kGroupBlocks * 64];
  const int t = threadIdx.x, lb = t >> 3, c = t & 7;
  const long long frame = (long long)frame0 + blockIdx.y;
  const int group0 = blockIdx.x * kGroupBlocks;
  const int b = min(group0 + lb, nblocks - 1);  // threads past the last block redo it and store nothing
  const int bx = b % bw, by = b / bw;
  const T* __restrict__ src = frames + frame * frame_stride;
  const int x = min(bx * 8 + c, w - 1);  // edge extension: the last column / row repeated
  int* __restrict__ blk = ws + lb * kLdsBlockStride;
#pragma unroll
  for (int r = 0; r < 8; r++) {
    const int y = min(by * 8 + r, h - 1);
    blk[r * 8 + c] = level_of(src[(long long)y * w + x]);
  }
  __syncthreads();
  int d[8];
#pragma unroll
  for (int k = 0; k < 8; k++) d[k] = blk[c * 8 + k];
  fdct_pass<true>(d);
#pragma unroll
  for (int k = 0; k < 8; k++) blk[c * 8 + k] = d[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 8; k++) d[k] = blk[k * 8 + c];
  fdct_pass<false>(d);
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const int n = k * 8 + c;
    const unsigned div = qdiv[n];
    const unsigned a = ((unsigned)abs(d[k]) + (div >> 1)) / div;
    zq[lb * 64 + kZigzagOfNatural[n]] = (int16_t)(d[k] < 0 ? -(int)a : (int)a);
  }
  __syncthreads();
  // the group's 32 x 128 bytes are contiguous in coef: 16 bytes per thread
  if (group0 + lb < nblocks)
    reinterpret_cast<uint4*>(coef + (frame * nblocks + group0) * 64)[t] = reinterpret_cast<const uint4*>(zq)[t];
}

// ---------------------------------------------------------------------------------------------------- entropy coding

__device__ __forceinline__ int bit_length(int v) { return 32 - __clz(abs(v)); }  // the JPEG size category; 0 for 0
__device__ __forceinline__ uint32_t amplitude(int v, int n) { return (uint32_t)(v < 0 ? v - 1 : v) & ((1u << n) - 1u); }

__device__ __forceinline__ void load_tables(const DeviceTables* __restrict__ tab, uint32_t* s_ac, uint32_t* s_dc) {
  for (int k = threadIdx.x; k < 256; k += blockDim.x) s_ac[k] = tab->ac[k];
  if (threadIdx.x < 16) s_dc[threadIdx.x] = tab->dc[threadIdx.x];
  __syncthreads();
}

// The code words of one block in order, each handed to emit(bits, count) with count <= 26: DC difference, then run / size
// symbols with ZRL for runs past 15 and EOB when the block ends in zeros.  cf: its 64 coefficients in zigzag order, 16-byte
// aligned; they are taken eight at a time from one 16-byte load and unpacked with static indices.
template <class Emit>
__device__ __forceinline__ void walk_block(const int16_t* __restrict__ cf, int prev_dc, const uint32_t* s_ac, const uint32_t* s_dc, Emit& emit) {
  const uint4* __restrict__ p = reinterpret_cast<const uint4*>(cf);
  int run = 0;
  for (int v = 0; v < 8; v++) {
    const uint4 q = p[v];
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const uint32_t pair = (j >> 1) == 0 ? q.x : (j >> 1) == 1 ? q.y : (j >> 1) == 2 ? q.z : q.w;
      const int cv = (int)(int16_t)((j & 1) ? pair >> 16 : pair & 0xffffu);
      if (j == 0 && v == 0) {
        const int diff = cv - prev_dc, n = bit_length(diff);
        const uint32_t e = s_dc[n];
        emit(((e & 0xffffu) << n) | amplitude(diff, n), (int)(e >> 16) + n);
      } else if (cv == 0) {
        run++;
      } else {
        while (run > 15) {
          emit(s_ac[0xf0] & 0xffffu, (int)(s_ac[0xf0] >> 16));
          run -= 16;
        }
        const int n = bit_length(cv);
        const uint32_t e = s_ac[(run << 4) | n];
        emit(((e & 0xffffu) << n) | amplitude(cv, n), (int)(e >> 16) + n);
        run = 0;
      }
    }
  }
  if (run > 0) emit(s_ac[0] & 0xffffu, (int)(s_ac[0] >> 16));
}

struct BitCounter {
  uint32_t bits = 0;
  __device__ __forceinline__ void operator()(uint32_t, int n) { bits += (uint32_t)n; }
};

// Bits most significant first into 32-bit words: bit k of a frame's stream is bit 31 - k % 32 of word k / 32.  The stream is
// zero where nothing has been written, so the words this block shares with its neighbours (its first and its last) are
// OR-ed in with integer atomics -- the result does not depend on the order -- and the words in between, all its own, are stored.
struct BitPacker {
  uint32_t* __restrict__ word;
  unsigned long long acc = 0;
  int n;  // valid low bits of acc
  bool first = true;
  __device__ __forceinline__ BitPacker(uint32_t* stream, uint32_t bit_offset) : word(stream + (bit_offset >> 5)), n((int)(bit_offset & 31u)) {}
  __device__ __forceinline__ void operator()(uint32_t bits, int count) {
    acc = (acc << count) | bits;
    n += count;
    if (n >= 32) {
      const uint32_t full = (uint32_t)(acc >> (n - 32));
      if (first) atomicOr(word, full);
      else *word = full;
      first = false;
      word++;
      n -= 32;
    }
  }
  __device__ __forceinline__ void finish() {
    if (n > 0) atomicOr(word, (uint32_t)(acc << (32 - n)));
  }
};

// one thread per block of the batch; total = frames * nblocks < 2^31
__global__ __launch_bounds__(256) void jenc_count_kernel(const int16_t* __restrict__ coef, int nblocks, int total, const DeviceTables* __restrict__ tab,
                                                         uint32_t* __restrict__ bits) {
  __shared__ uint32_t s_ac[256], s_dc[16];
  load_tables(tab, s_ac, s_dc);
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int prev_dc = (i % nblocks) ? coef[(i - 1) * 64] : 0;
  BitCounter count;
  walk_block(coef + i * 64, prev_dc, s_ac, s_dc, count);
  bits[i] = count.bits;
}

// inclusive scan over the 1024 threads of a workgroup; *total = the sum.  scratch: 16 words of LDS.
__device__ __forceinline__ uint32_t workgroup_scan_1024(uint32_t v, uint32_t* scratch, uint32_t* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t x = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t y = __shfl_up(x, d, 64);
    if (lane >= d) x += y;
  }
  if (lane == 63) scratch[wave] = x;
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (int k = 0; k < 16; k++) {
    const uint32_t s = scratch[k];
    before += k < wave ? s : 0u;
    all += s;
  }
  __syncthreads();  // scratch may be written again
  *total = all;
  return before + x;
}

// one workgroup of 1024 per frame: bits[b] (a count) -> the bit offset of block b in the frame's stream; frame_bits[f] = the sum;
// the words of the stream that jenc_pack_kernel will OR into are cleared (two more than needed, never past the frame's part)
__global__ __launch_bounds__(1024) void jenc_scan_kernel(uint32_t* __restrict__ bits, int nblocks, uint32_t* __restrict__ frame_bits,
                                                         uint32_t* __restrict__ stream, long long stream_words) {
  __shared__ uint32_t scratch[16];
  const int t = threadIdx.x;
  uint32_t* __restrict__ fb = bits + (long long)blockIdx.x * nblocks;
  uint32_t carry = 0;
  for (int base = 0; base < nblocks; base += 1024) {
    const int i = base + t;
    const uint32_t v = i < nblocks ? fb[i] : 0u;
    uint32_t all;
    const uint32_t incl = workgroup_scan_1024(v, scratch, &all);
    if (i < nblocks) fb[i] = carry + incl - v;
    carry += all;
  }
  if (t == 0) frame_bits[blockIdx.x] = carry;
  uint32_t* __restrict__ s = stream + (long long)blockIdx.x * stream_words;
  const long long nz = min((long long)(carry >> 5) + 2, stream_words);
  for (long long k = t; k < nz; k += 1024) s[k] = 0u;
}

__global__ __launch_bounds__(256) void jenc_pack_kernel(const int16_t* __restrict__ coef, int nblocks, int total, const DeviceTables* __restrict__ tab,
                                                        const uint32_t* __restrict__ bit_offset, uint32_t* __restrict__ stream, long long stream_words) {
  __shared__ uint32_t s_ac[256], s_dc[16];
  load_tables(tab, s_ac, s_dc);
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int prev_dc = (i % nblocks) ? coef[(i - 1) * 64] : 0;
  BitPacker pack(stream + (i / nblocks) * stream_words, bit_offset[i]);
  walk_block(coef + i * 64, prev_dc, s_ac, s_dc, pack);
  pack.finish();
}

// one workgroup of 1024 per frame.  Per iteration 16 stream bytes per thread: count the 0xFF among them, scan, lay the stuffed
// bytes out in LDS, copy them out with consecutive threads on consecutive bytes.
__global__ __launch_bounds__(1024) void jenc_stuff_kernel(const uint32_t* __restrict__ stream, long long stream_words, const uint32_t* __restrict__ frame_bits,
                                                          const DeviceTables* __restrict__ tab, uint8_t* __restrict__ out, long long slot_bytes,
                                                          int32_t* __restrict__ sizes) {
  __shared__ uint8_t staged[2 * kStuffChunk];
  __shared__ uint32_t scratch[16];
  const int t = threadIdx.x;
  const uint32_t* __restrict__ s = stream + (long long)blockIdx.x * stream_words;
  uint8_t* __restrict__ o = out + (long long)blockIdx.x * slot_bytes;
  const uint32_t nbits = frame_bits[blockIdx.x];
  const uint32_t nbytes = (nbits + 7u) >> 3;
  const uint32_t pad = (nbits & 7u) ? (0xffu >> (nbits & 7u)) : 0u;  // 1-bits that fill the last byte
  for (int k = t; k < kHeaderBytes; k += 1024) o[k] = tab->header[k];
  uint32_t pos = kHeaderBytes;
  for (uint32_t base = 0; base < nbytes; base += kStuffChunk) {
    const uint32_t byte0 = base + (uint32_t)t * 16u;
    uint32_t wd[4];
    uint32_t ff = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint32_t at = byte0 + 4u * j;  // a multiple of 4
      uint32_t x = at < nbytes ? s[at >> 2] : 0u;
      if (pad && at == ((nbytes - 1u) & ~3u)) x |= pad << (24u - 8u * ((nbytes - 1u) & 3u));
      wd[j] = x;
#pragma unroll
      for (int q = 0; q < 4; q++) ff += (at + q < nbytes && ((x >> (24 - 8 * q)) & 0xffu) == 0xffu) ? 1u : 0u;
    }
    const uint32_t mine = (byte0 < nbytes ? min(16u, nbytes - byte0) : 0u) + ff;
    uint32_t all;
    uint32_t lp = workgroup_scan_1024(mine, scratch, &all) - mine;
#pragma unroll
    for (int j = 0; j < 4; j++) {
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const uint32_t v = (wd[j] >> (24 - 8 * q)) & 0xffu;
        if (byte0 + 4u * j + q < nbytes) {
          staged[lp++] = (uint8_t)v;
          if (v == 0xffu) staged[lp++] = 0;
        }
      }
    }
    __syncthreads();
    for (uint32_t k = t; k < all; k += 1024) o[pos + k] = staged[k];
    pos += all;
    __syncthreads();  // staged is rewritten by the next iteration
  }
  if (t == 0) {
    o[pos] = 0xff;
    o[pos + 1] = 0xd9;
    sizes[blockIdx.x] = (int32_t)(pos + 2);
  }
}

// mdcj_fetch: file f (the first offsets[f + 1] - offsets[f] bytes of slot f; the host has checked them against the slot and the
// capacity) -> packed + offsets[f], so that one copy brings every file to the host.  grid (parts, frames): consecutive threads on
// consecutive bytes.
__global__ __launch_bounds__(256) void jenc_gather_kernel(const uint8_t* __restrict__ out, long long slot_bytes, const long long* __restrict__ offsets,
                                                          uint8_t* __restrict__ packed) {
  const uint8_t* __restrict__ src = out + (long long)blockIdx.y * slot_bytes;
  uint8_t* __restrict__ dst = packed + offsets[blockIdx.y];
  const int n = (int)(offsets[blockIdx.y + 1] - offsets[blockIdx.y]);
  for (int k = blockIdx.x * 256 + threadIdx.x; k < n; k += gridDim.x * 256) dst[k] = src[k];
}

// ---------------------------------------------------------------------------------------------------- host side

thread_local char g_error[256] = "";

int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_error, sizeof g_error, fmt, ap);
  va_end(ap);
  return code;
}

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    if (dev < 0) return;
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) (void)hipSetDevice(dev);
    else prev = -1;
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

void huffman_table(const uint8_t* bits, const uint8_t* vals, uint32_t* out) {  // Annex C: canonical codes
  uint32_t code = 0;
  int k = 0;
  for (int len = 1; len <= 16; len++) {
    for (int i = 0; i < bits[len - 1]; i++) out[vals[k++]] = ((uint32_t)len << 16) | code++;
    code <<= 1;
  }
}

void fill_tables(DeviceTables* t, int w, int h, int quality) {
  memset(t, 0, sizeof *t);
  huffman_table(kAcBits, kAcVals, t->ac);
  huffman_table(kDcBits, kDcVals, t->dc);
  const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;  // jpeg_quality_scaling
  uint8_t q[64];
  for (int i = 0; i < 64; i++) {
    int v = (kBaseQ[i] * scale + 50) / 100;
    q[i] = (uint8_t)(v < 1 ? 1 : v > 255 ? 255 : v);
    t->qdiv[i] = (uint16_t)(8 * q[i]);
  }
  uint8_t* p = t->header;
  auto put = [&p](const void* src, size_t n) {
    memcpy(p, src, n);
    p += n;
  };
  const uint8_t soi_app0[] = {0xff, 0xd8, 0xff, 0xe0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
  put(soi_app0, sizeof soi_app0);
  const uint8_t dqt[] = {0xff, 0xdb, 0, 67, 0};
  put(dqt, sizeof dqt);
  for (int k = 0; k < 64; k++) *p++ = q[kZigzag[k]];
  const uint8_t sof0[] = {0xff, 0xc0, 0, 11, 8, (uint8_t)(h >> 8), (uint8_t)h, (uint8_t)(w >> 8), (uint8_t)w, 1, 1, 0x11, 0};
  put(sof0, sizeof sof0);
  const uint8_t dht_dc[] = {0xff, 0xc4, 0, 31, 0x00};
  put(dht_dc, sizeof dht_dc);
  put(kDcBits, 16);
  put(kDcVals, 12);
  const uint8_t dht_ac[] = {0xff, 0xc4, 0, 181, 0x10};
  put(dht_ac, sizeof dht_ac);
  put(kAcBits, 16);
  put(kAcVals, 162);
  const uint8_t sos[] = {0xff, 0xda, 0, 8, 1, 1, 0x00, 0, 63, 0};
  put(sos, sizeof sos);
  static_assert(20 + 5 + 64 + 13 + 5 + 28 + 5 + 178 + 10 == kHeaderBytes, "header layout");
}

long long blocks_of(int w, int h) { return (long long)((w + 7) / 8) * ((h + 7) / 8); }

}  // namespace

struct mdcj_encoder {
  int device = -1, w = 0, h = 0, quality = 0, max_frames = 0;
  int nblocks = 0;
  long long stream_words = 0;  // per frame
  DeviceTables* d_tab = nullptr;
  int16_t* d_coef = nullptr;
  uint32_t* d_bits = nullptr;
  uint32_t* d_frame_bits = nullptr;
  uint32_t* d_stream = nullptr;
  uint8_t* d_out = nullptr;  // mdcj_output_device: allocated on demand
  int32_t* d_sizes = nullptr;
  uint8_t* d_packed = nullptr;  // mdcj_fetch: the files back to back (grown on demand) and their offsets
  long long packed_capacity = 0;
  long long* d_offsets = nullptr;
};

extern "C" {

int64_t mdcj_jpeg_bound(int w, int h) {
  if (w < 1 || h < 1 || w > 65535 || h > 65535) return -1;
  return 1024 + 416 * blocks_of(w, h);
}

const char* mdcj_last_error(void) { return g_error; }

void mdcj_destroy(mdcj_encoder* enc) {
  if (!enc) return;
  {
    DeviceGuard dg(enc->device);
    (void)hipFree(enc->d_tab);
    (void)hipFree(enc->d_coef);
    (void)hipFree(enc->d_bits);
    (void)hipFree(enc->d_frame_bits);
    (void)hipFree(enc->d_stream);
    (void)hipFree(enc->d_out);
    (void)hipFree(enc->d_sizes);
    (void)hipFree(enc->d_packed);
    (void)hipFree(enc->d_offsets);
  }
  delete enc;
}

int mdcj_create(int device, int w, int h, int quality, int max_frames, mdcj_encoder** out) {
  if (!out) return fail(MDCJ_ERR_ARG, "mdcj_create: out is null");
  *out = nullptr;
  if (w < 1 || h < 1 || w > 65535 || h > 65535) return fail(MDCJ_ERR_SIZE, "mdcj_create: %d x %d is outside 1..65535 (the SOF0 fields are 16-bit)", w, h);
  if (quality < 1 || quality > 100) return fail(MDCJ_ERR_ARG, "mdcj_create: quality %d is outside 1..100", quality);
  if (max_frames < 1) return fail(MDCJ_ERR_ARG, "mdcj_create: max_frames %d is below 1", max_frames);
  const long long nblocks = blocks_of(w, h);
  if (mdcj_jpeg_bound(w, h) > (1ll << 30))
    return fail(MDCJ_ERR_SIZE, "mdcj_create: %d x %d has %lld blocks; a frame's bit offsets are 32-bit (bound <= 2^30)", w, h, nblocks);
  if (nblocks * max_frames > 0x7fffffffll)
    return fail(MDCJ_ERR_SIZE, "mdcj_create: %lld blocks x %d frames per call is 2^31 or more", nblocks, max_frames);
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count < 1) return fail(MDCJ_ERR_NO_DEVICE, "mdcj_create: no HIP device");
  if (device >= count) return fail(MDCJ_ERR_NO_DEVICE, "mdcj_create: device %d of %d", device, count);
  if (device < 0 && hipGetDevice(&device) != hipSuccess) return fail(MDCJ_ERR_HIP, "mdcj_create: hipGetDevice failed");
  DeviceGuard dg(device);
  mdcj_encoder* e = new (std::nothrow) mdcj_encoder;
  if (!e) return fail(MDCJ_ERR_NOMEM, "mdcj_create: out of host memory");
  e->device = device, e->w = w, e->h = h, e->quality = quality, e->max_frames = max_frames;
  e->nblocks = (int)nblocks;
  // ceil(1658 * nblocks / 32) words hold the longest stream; jenc_scan_kernel clears up to two more
  e->stream_words = ((long long)kBitsPerBlockMax * nblocks + 31) / 32 + 2;
  const size_t n = (size_t)nblocks * (size_t)max_frames;
  if (hipMalloc((void**)&e->d_tab, sizeof(DeviceTables)) != hipSuccess || hipMalloc((void**)&e->d_coef, n * 64 * sizeof(int16_t)) != hipSuccess ||
      hipMalloc((void**)&e->d_bits, n * sizeof(uint32_t)) != hipSuccess || hipMalloc((void**)&e->d_frame_bits, (size_t)max_frames * sizeof(uint32_t)) != hipSuccess ||
      hipMalloc((void**)&e->d_stream, (size_t)e->stream_words * (size_t)max_frames * sizeof(uint32_t)) != hipSuccess) {
    (void)hipGetLastError();
    mdcj_destroy(e);
    return fail(MDCJ_ERR_NOMEM, "mdcj_create: could not allocate the scratch arrays of %d frames of %d x %d", max_frames, w, h);
  }
  DeviceTables tab;
  fill_tables(&tab, w, h, quality);
  if (hipMemcpy(e->d_tab, &tab, sizeof tab, hipMemcpyHostToDevice) != hipSuccess) {
    mdcj_destroy(e);
    return fail(MDCJ_ERR_HIP, "mdcj_create: copying the tables failed");
  }
  *out = e;
  return MDCJ_OK;
}

}  // extern "C"

namespace {

template <typename T>
int encode(const char* who, mdcj_encoder* e, const T* d_frames, int64_t frame_stride, int nframes, uint8_t* d_out, int64_t slot_bytes, int32_t* d_sizes,
           void* stream) {
  if (!e) return fail(MDCJ_ERR_ARG, "%s: encoder is null", who);
  if (nframes < 0 || nframes > e->max_frames) return fail(MDCJ_ERR_ARG, "%s: %d frames, the encoder was made for 0..%d", who, nframes, e->max_frames);
  if (nframes == 0) return MDCJ_OK;
  if (!d_frames || !d_out || !d_sizes) return fail(MDCJ_ERR_ARG, "%s: null device pointer", who);
  if (frame_stride < (int64_t)e->w * e->h) return fail(MDCJ_ERR_ARG, "%s: frame_stride %lld is below %d x %d", who, (long long)frame_stride, e->w, e->h);
  const int64_t bound = mdcj_jpeg_bound(e->w, e->h);
  if (slot_bytes < bound) return fail(MDCJ_ERR_SIZE, "%s: slot_bytes %lld is below mdcj_jpeg_bound(%d, %d) = %lld", who, (long long)slot_bytes, e->w, e->h, (long long)bound);
  DeviceGuard dg(e->device);
  hipStream_t s = (hipStream_t)stream;
  const int nblocks = e->nblocks, bw = (e->w + 7) / 8;
  const int total = nblocks * nframes;  // < 2^31: mdcj_create
  const unsigned groups = (unsigned)((nblocks + kGroupBlocks - 1) / kGroupBlocks);
  const uint16_t* d_qdiv = reinterpret_cast<const uint16_t*>(reinterpret_cast<const char*>(e->d_tab) + offsetof(DeviceTables, qdiv));
  for (int f0 = 0; f0 < nframes; f0 += 65535) {  // a grid's y dimension is 16-bit
    const unsigned nf = (unsigned)(nframes - f0 < 65535 ? nframes - f0 : 65535);
    jenc_fdct_quant_kernel<T><<<dim3(groups, nf), 256, 0, s>>>(d_frames, (long long)frame_stride, f0, e->w, e->h, bw, nblocks, d_qdiv, e->d_coef);
  }
  const unsigned per_block_grid = (unsigned)(((long long)total + 255) / 256);
  jenc_count_kernel<<<per_block_grid, 256, 0, s>>>(e->d_coef, nblocks, total, e->d_tab, e->d_bits);
  jenc_scan_kernel<<<(unsigned)nframes, 1024, 0, s>>>(e->d_bits, nblocks, e->d_frame_bits, e->d_stream, e->stream_words);
  jenc_pack_kernel<<<per_block_grid, 256, 0, s>>>(e->d_coef, nblocks, total, e->d_tab, e->d_bits, e->d_stream, e->stream_words);
  jenc_stuff_kernel<<<(unsigned)nframes, 1024, 0, s>>>(e->d_stream, e->stream_words, e->d_frame_bits, e->d_tab, d_out, (long long)slot_bytes, d_sizes);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(MDCJ_ERR_HIP, "%s: launch failed: %s", who, hipGetErrorString(err));
  return MDCJ_OK;
}

}  // namespace

extern "C" {

int mdcj_encode_f32_device(mdcj_encoder* enc, const float* d_frames, int64_t frame_stride, int nframes, uint8_t* d_out, int64_t slot_bytes, int32_t* d_sizes,
                           void* stream) {
  return encode("mdcj_encode_f32_device", enc, d_frames, frame_stride, nframes, d_out, slot_bytes, d_sizes, stream);
}

int mdcj_output_device(mdcj_encoder* enc, uint8_t** d_out, int64_t* slot_bytes, int32_t** d_sizes) {
  if (!enc || !d_out || !slot_bytes || !d_sizes) return fail(MDCJ_ERR_ARG, "mdcj_output_device: null argument");
  const int64_t bound = mdcj_jpeg_bound(enc->w, enc->h);
  if (!enc->d_out) {
    DeviceGuard dg(enc->device);
    uint8_t* o = nullptr;
    int32_t* z = nullptr;
    if (hipMalloc((void**)&o, (size_t)bound * (size_t)enc->max_frames) != hipSuccess || hipMalloc((void**)&z, (size_t)enc->max_frames * sizeof(int32_t)) != hipSuccess) {
      (void)hipGetLastError();
      (void)hipFree(o);
      return fail(MDCJ_ERR_NOMEM, "mdcj_output_device: could not allocate %d slots of %lld bytes", enc->max_frames, (long long)bound);
    }
    enc->d_out = o, enc->d_sizes = z;
  }
  *d_out = enc->d_out, *slot_bytes = bound, *d_sizes = enc->d_sizes;
  return MDCJ_OK;
}

int64_t mdcj_fetch(mdcj_encoder* enc, const uint8_t* d_out, int64_t slot_bytes, const int32_t* d_sizes, int nframes, uint8_t* h_out, int64_t h_capacity,
                   int32_t* h_sizes, void* stream) {
  if (!enc || !d_out || !d_sizes || !h_sizes) return fail(MDCJ_ERR_ARG, "mdcj_fetch: null argument");
  if (nframes < 0 || nframes > enc->max_frames) return fail(MDCJ_ERR_ARG, "mdcj_fetch: %d frames, the encoder was made for 0..%d", nframes, enc->max_frames);
  if (nframes == 0) return 0;
  DeviceGuard dg(enc->device);
  hipStream_t s = (hipStream_t)stream;
  if (hipMemcpyAsync(h_sizes, d_sizes, (size_t)nframes * sizeof(int32_t), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
    return fail(MDCJ_ERR_HIP, "mdcj_fetch: copying the sizes failed: %s", hipGetErrorString(hipGetLastError()));
  int64_t total = 0;
  for (int f = 0; f < nframes; f++) {
    if (h_sizes[f] <= 0 || h_sizes[f] > slot_bytes) return fail(MDCJ_ERR_SIZE, "mdcj_fetch: frame %d has size %d, the slot %lld", f, h_sizes[f], (long long)slot_bytes);
    total += h_sizes[f];
  }
  if (!h_out) return total;
  if (total > h_capacity) return fail(MDCJ_ERR_SIZE, "mdcj_fetch: %lld bytes, room for %lld", (long long)total, (long long)h_capacity);
  // one copy per file costs more than the bytes (a thousand copies of 100 KB): gather on the device, copy once
  if (total > enc->packed_capacity || !enc->d_offsets) {
    (void)hipFree(enc->d_packed);
    enc->d_packed = nullptr, enc->packed_capacity = 0;
    const long long want = total + total / 4 + 4096;
    if (hipMalloc((void**)&enc->d_packed, (size_t)want) != hipSuccess ||
        (!enc->d_offsets && hipMalloc((void**)&enc->d_offsets, ((size_t)enc->max_frames + 1) * sizeof(long long)) != hipSuccess)) {
      (void)hipGetLastError();
      return fail(MDCJ_ERR_NOMEM, "mdcj_fetch: could not allocate %lld bytes for the gathered files", want);
    }
    enc->packed_capacity = want;
  }
  long long* offsets = new (std::nothrow) long long[(size_t)nframes + 1];
  if (!offsets) return fail(MDCJ_ERR_NOMEM, "mdcj_fetch: out of host memory");
  long long at = 0;
  int largest = 0;
  for (int f = 0; f < nframes; f++) {
    offsets[f] = at;
    at += h_sizes[f];
    if (h_sizes[f] > largest) largest = h_sizes[f];
  }
  offsets[nframes] = at;
  hipError_t err = hipMemcpy(enc->d_offsets, offsets, ((size_t)nframes + 1) * sizeof(long long), hipMemcpyHostToDevice);
  delete[] offsets;
  if (err != hipSuccess) return fail(MDCJ_ERR_HIP, "mdcj_fetch: copying the offsets failed: %s", hipGetErrorString(err));
  const unsigned parts = (unsigned)((largest + 16 * 256 - 1) / (16 * 256));  // 16 bytes per thread
  for (int f0 = 0; f0 < nframes; f0 += 65535) {
    const unsigned nf = (unsigned)(nframes - f0 < 65535 ? nframes - f0 : 65535);
    jenc_gather_kernel<<<dim3(parts, nf), 256, 0, s>>>(d_out + (int64_t)f0 * slot_bytes, (long long)slot_bytes, enc->d_offsets + f0, enc->d_packed);
  }
  if ((err = hipGetLastError()) != hipSuccess || (err = hipMemcpyAsync(h_out, enc->d_packed, (size_t)total, hipMemcpyDeviceToHost, s)) != hipSuccess ||
      (err = hipStreamSynchronize(s)) != hipSuccess)
    return fail(MDCJ_ERR_HIP, "mdcj_fetch: gathering the files failed: %s", hipGetErrorString(err));
  return total;
}

int mdcj_encode_u8_device(mdcj_encoder* enc, const uint8_t* d_frames, int64_t frame_stride, int nframes, uint8_t* d_out, int64_t slot_bytes, int32_t* d_sizes,
                          void* stream) {
  return encode("mdcj_encode_u8_device", enc, d_frames, frame_stride, nframes, d_out, slot_bytes, d_sizes, stream);
}

}  // extern "C"
