// jpeg_encode_core.h -- what the two device JPEG encoder libraries share, one copy of the source: mdc_jenc.hip (libmdc_jenc.so, the
// Annex K tables) and mdc_jopt.hip (libmdc_jopt.so, one optimal table pair per frame).  The constant tables, the forward DCT and
// quantisation kernel, the block walker with its bit counter and bit packer, the per-frame scan, the gather kernel of the fetch
// call, and the host side of both libraries, which each parametrises with a Params.  Each library is one translation unit and
// includes this once; everything is in its unnamed namespace.  (The two stuffing kernels differ only in their header lines and
// stay two copies: with the loop in a function here, both compiled to other instructions.)
#ifndef MDC_JPEG_ENCODE_CORE_H
#define MDC_JPEG_ENCODE_CORE_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <new>

#include "codec_host.h"

namespace {

constexpr int kHeaderBytes = 328;
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

// What tells the two libraries' host sides apart, beside the launch sequence of an encode call
struct Params {
  const char* prefix;      // of the functions' names in messages: "mdcj", "mdcjo"
  int bound_per_block;     // *_jpeg_bound: 1024 + this many bytes per block
  int bits_per_block_max;  // the longest code of a block (the public header derives it)
};

// The fields both encoders have.  struct mdcj_encoder and struct mdcjo_encoder derive from it; each adds alloc_extra() and
// free_extra() for what it has beyond them (called with the encoder's device current).
struct Encoder {
  int device = -1, w = 0, h = 0, quality = 0, max_frames = 0;
  int nblocks = 0;
  long long stream_words = 0;  // per frame
  DeviceTables* d_tab = nullptr;
  int16_t* d_coef = nullptr;
  uint32_t* d_bits = nullptr;
  uint32_t* d_frame_bits = nullptr;
  uint32_t* d_stream = nullptr;
  uint8_t* d_out = nullptr;  // output_device: allocated on demand
  int32_t* d_sizes = nullptr;
  uint8_t* d_packed = nullptr;  // fetch: the files back to back (grown on demand) and their offsets
  long long packed_capacity = 0;
  long long* d_offsets = nullptr;
};

int64_t jpeg_bound(const Params& p, int w, int h) {
  if (w < 1 || h < 1 || w > 65535 || h > 65535) return -1;
  return 1024 + p.bound_per_block * blocks_of(w, h);
}

template <class E>
void destroy(E* enc) {
  if (!enc) return;
  {
    DeviceGuard dg(enc->device);
    (void)hipFree(enc->d_tab);
    (void)hipFree(enc->d_coef);
    (void)hipFree(enc->d_bits);
    (void)hipFree(enc->d_frame_bits);
    (void)hipFree(enc->d_stream);
    enc->free_extra();
    (void)hipFree(enc->d_out);
    (void)hipFree(enc->d_sizes);
    (void)hipFree(enc->d_packed);
    (void)hipFree(enc->d_offsets);
  }
  delete enc;
}

template <class E>
int create(const char* who, const Params& p, int device, int w, int h, int quality, int max_frames, E** out) {
  if (!out) return fail(kErrArg, "%s: out is null", who);
  *out = nullptr;
  if (w < 1 || h < 1 || w > 65535 || h > 65535) return fail(kErrSize, "%s: %d x %d is outside 1..65535 (the SOF0 fields are 16-bit)", who, w, h);
  if (quality < 1 || quality > 100) return fail(kErrArg, "%s: quality %d is outside 1..100", who, quality);
  if (max_frames < 1) return fail(kErrArg, "%s: max_frames %d is below 1", who, max_frames);
  const long long nblocks = blocks_of(w, h);
  if (jpeg_bound(p, w, h) > (1ll << 30))
    return fail(kErrSize, "%s: %d x %d has %lld blocks; a frame's bit offsets are 32-bit (bound <= 2^30)", who, w, h, nblocks);
  if (nblocks * max_frames > 0x7fffffffll) return fail(kErrSize, "%s: %lld blocks x %d frames per call is 2^31 or more", who, nblocks, max_frames);
  if (int rc = resolve_device(who, &device)) return rc;
  DeviceGuard dg(device);
  E* e = new (std::nothrow) E;
  if (!e) return fail(kErrNoMem, "%s: out of host memory", who);
  e->device = device, e->w = w, e->h = h, e->quality = quality, e->max_frames = max_frames;
  e->nblocks = (int)nblocks;
  // ceil(bits_per_block_max * nblocks / 32) words hold the longest stream; jenc_scan_kernel clears up to two more
  e->stream_words = ((long long)p.bits_per_block_max * nblocks + 31) / 32 + 2;
  const size_t n = (size_t)nblocks * (size_t)max_frames;
  if (hipMalloc((void**)&e->d_tab, sizeof(DeviceTables)) != hipSuccess || hipMalloc((void**)&e->d_coef, n * 64 * sizeof(int16_t)) != hipSuccess ||
      hipMalloc((void**)&e->d_bits, n * sizeof(uint32_t)) != hipSuccess || hipMalloc((void**)&e->d_frame_bits, (size_t)max_frames * sizeof(uint32_t)) != hipSuccess ||
      hipMalloc((void**)&e->d_stream, (size_t)e->stream_words * (size_t)max_frames * sizeof(uint32_t)) != hipSuccess || !e->alloc_extra()) {
    (void)hipGetLastError();
    destroy(e);
    return fail(kErrNoMem, "%s: could not allocate the scratch arrays of %d frames of %d x %d", who, max_frames, w, h);
  }
  DeviceTables tab;
  fill_tables(&tab, w, h, quality);
  if (hipMemcpy(e->d_tab, &tab, sizeof tab, hipMemcpyHostToDevice) != hipSuccess) {
    destroy(e);
    return fail(kErrHip, "%s: copying the tables failed", who);
  }
  *out = e;
  return kOk;
}

// The argument checks of an encode call.  *go: there are frames to encode.
int check_encode(const char* who, const Params& p, const Encoder* e, const void* d_frames, int64_t frame_stride, int nframes, const uint8_t* d_out, int64_t slot_bytes,
                 const int32_t* d_sizes, bool* go) {
  *go = false;
  if (!e) return fail(kErrArg, "%s: encoder is null", who);
  if (nframes < 0 || nframes > e->max_frames) return fail(kErrArg, "%s: %d frames, the encoder was made for 0..%d", who, nframes, e->max_frames);
  if (nframes == 0) return kOk;
  if (!d_frames || !d_out || !d_sizes) return fail(kErrArg, "%s: null device pointer", who);
  if (frame_stride < (int64_t)e->w * e->h) return fail(kErrArg, "%s: frame_stride %lld is below %d x %d", who, (long long)frame_stride, e->w, e->h);
  const int64_t bound = jpeg_bound(p, e->w, e->h);
  if (slot_bytes < bound)
    return fail(kErrSize, "%s: slot_bytes %lld is below %s_jpeg_bound(%d, %d) = %lld", who, (long long)slot_bytes, p.prefix, e->w, e->h, (long long)bound);
  *go = true;
  return kOk;
}

int output_device(const Params& p, Encoder* enc, uint8_t** d_out, int64_t* slot_bytes, int32_t** d_sizes) {
  if (!enc || !d_out || !slot_bytes || !d_sizes) return fail(kErrArg, "%s_output_device: null argument", p.prefix);
  const int64_t bound = jpeg_bound(p, enc->w, enc->h);
  if (!enc->d_out) {
    DeviceGuard dg(enc->device);
    uint8_t* o = nullptr;
    int32_t* z = nullptr;
    if (hipMalloc((void**)&o, (size_t)bound * (size_t)enc->max_frames) != hipSuccess || hipMalloc((void**)&z, (size_t)enc->max_frames * sizeof(int32_t)) != hipSuccess) {
      (void)hipGetLastError();
      (void)hipFree(o);
      return fail(kErrNoMem, "%s_output_device: could not allocate %d slots of %lld bytes", p.prefix, enc->max_frames, (long long)bound);
    }
    enc->d_out = o, enc->d_sizes = z;
  }
  *d_out = enc->d_out, *slot_bytes = bound, *d_sizes = enc->d_sizes;
  return kOk;
}

int64_t fetch(const Params& p, Encoder* enc, const uint8_t* d_out, int64_t slot_bytes, const int32_t* d_sizes, int nframes, uint8_t* h_out, int64_t h_capacity,
              int32_t* h_sizes, void* stream) {
  if (!enc || !d_out || !d_sizes || !h_sizes) return fail(kErrArg, "%s_fetch: null argument", p.prefix);
  if (nframes < 0 || nframes > enc->max_frames) return fail(kErrArg, "%s_fetch: %d frames, the encoder was made for 0..%d", p.prefix, nframes, enc->max_frames);
  if (nframes == 0) return 0;
  DeviceGuard dg(enc->device);
  hipStream_t s = (hipStream_t)stream;
  if (hipMemcpyAsync(h_sizes, d_sizes, (size_t)nframes * sizeof(int32_t), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
    return fail(kErrHip, "%s_fetch: copying the sizes failed: %s", p.prefix, hipGetErrorString(hipGetLastError()));
  int64_t total = 0;
  for (int f = 0; f < nframes; f++) {
    if (h_sizes[f] <= 0 || h_sizes[f] > slot_bytes)
      return fail(kErrSize, "%s_fetch: frame %d has size %d, the slot %lld", p.prefix, f, h_sizes[f], (long long)slot_bytes);
    total += h_sizes[f];
  }
  if (!h_out) return total;
  if (total > h_capacity) return fail(kErrSize, "%s_fetch: %lld bytes, room for %lld", p.prefix, (long long)total, (long long)h_capacity);
  // one copy per file costs more than the bytes (a thousand copies of 100 KB): gather on the device, copy once
  if (total > enc->packed_capacity || !enc->d_offsets) {
    (void)hipFree(enc->d_packed);
    enc->d_packed = nullptr, enc->packed_capacity = 0;
    const long long want = total + total / 4 + 4096;
    if (hipMalloc((void**)&enc->d_packed, (size_t)want) != hipSuccess ||
        (!enc->d_offsets && hipMalloc((void**)&enc->d_offsets, ((size_t)enc->max_frames + 1) * sizeof(long long)) != hipSuccess)) {
      (void)hipGetLastError();
      return fail(kErrNoMem, "%s_fetch: could not allocate %lld bytes for the gathered files", p.prefix, want);
    }
    enc->packed_capacity = want;
  }
  long long* offsets = new (std::nothrow) long long[(size_t)nframes + 1];
  if (!offsets) return fail(kErrNoMem, "%s_fetch: out of host memory", p.prefix);
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
  if (err != hipSuccess) return fail(kErrHip, "%s_fetch: copying the offsets failed: %s", p.prefix, hipGetErrorString(err));
  const unsigned parts = (unsigned)((largest + 16 * 256 - 1) / (16 * 256));  // 16 bytes per thread
  for (int f0 = 0; f0 < nframes; f0 += 65535) {
    const unsigned nf = (unsigned)(nframes - f0 < 65535 ? nframes - f0 : 65535);
    jenc_gather_kernel<<<dim3(parts, nf), 256, 0, s>>>(d_out + (int64_t)f0 * slot_bytes, (long long)slot_bytes, enc->d_offsets + f0, enc->d_packed);
  }
  if ((err = hipGetLastError()) != hipSuccess || (err = hipMemcpyAsync(h_out, enc->d_packed, (size_t)total, hipMemcpyDeviceToHost, s)) != hipSuccess ||
      (err = hipStreamSynchronize(s)) != hipSuccess)
    return fail(kErrHip, "%s_fetch: gathering the files failed: %s", p.prefix, hipGetErrorString(err));
  return total;
}

}  // namespace

#endif  // MDC_JPEG_ENCODE_CORE_H
