// libmdc_zipw.so (include/mdc_zipw.h): CRC-32, ZIP local headers and the gather of a batch of device-resident files on the
// device; the central directory and the archive file on the host.  One translation unit, independent of libmdc_hip.so.
//
// CRC-32 is linear over GF(2).  With crc0(M) = M(x) * x^32 mod P (the table-driven CRC with initial value 0 and no final XOR),
//   crc0(A || B) = crc0(A) * x^(8 |B|)  ^  crc0(B)          and          crc32(M) = crc0(M) ^ 0xFFFFFFFF * x^(8 |M|) ^ 0xFFFFFFFF,
// all products mod P in zlib's reflected representation (bit 31 of a word is the coefficient of x^0).  A little-endian dword of
// the data is, in that representation, the polynomial of its 32 bits, so a 16-byte word d0 d1 d2 d3 has
// crc0 = d0 x^128 ^ d1 x^96 ^ d2 x^64 ^ d3 x^32.
//
// zipw_crc_parts_kernel: a file is [head < 16 bytes][body: nwords 16-byte-aligned words][tail < 16 bytes].  The body is cut in
// rows of kThreads words (one 16-byte load per lane, consecutive lanes on consecutive words) and the rows in `parts` contiguous
// runs, one workgroup each.  Lane t folds words t, t + kThreads, ... of its run by Horner's rule on the four dwords separately,
// a_i = a_i * K ^ d_i with K = x^(8 * 16 * kThreads): four 256-entry table lookups from LDS per dword (or 32 shift-and-XOR steps,
// VARIANT 1).  At the end of the run the four are folded with x^32 (the slice-by-4 tables of the ordinary CRC), the lane's value
// is multiplied by x^(128 * words behind its last word) from a 256-entry table, the workgroup XORs its lanes (shuffles, then
// four words of LDS), and the run's value is moved to the end of the body with x^(8 * bytes behind the run), a square-and-multiply
// product over the bits of that count taken from x^(2^k), spread over the lanes of one wave.
// zipw_crc_finish_kernel, one wave per file: head bytes bit by bit from 0xFFFFFFFF, times x^(8 * body bytes), XOR the parts, tail
// bytes, final XOR.  No atomics: the parts go through a scratch array.
#include "../../include/mdc_zipw.h"

#include <errno.h>
#include <fcntl.h>
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <new>
#include <string>
#include <vector>

#include "codec_host.h"

namespace {

constexpr uint32_t kPoly = 0xEDB88320u;
constexpr uint32_t kOne = 0x80000000u;  // x^0
constexpr int kWord = 16;               // bytes per load
constexpr int kThreads = 256;           // lanes of a workgroup = words of a row
constexpr int kRowBytes = kWord * kThreads;
constexpr int kRowsPerPartHint = 16;  // a part is meant to take about this many rows of a slot
constexpr int kMaxParts = 1024;
constexpr int kMaxGrid = 8192;

constexpr uint32_t mulmod_c(uint32_t a, uint32_t b) {  // a * b mod P
  uint32_t p = 0;
  for (int i = 0; i < 32; i++) {
    if (a & (kOne >> i)) p ^= b;
    b = (b >> 1) ^ ((b & 1) ? kPoly : 0);
  }
  return p;
}

struct Tables {
  uint32_t k[4][256];    // (byte b of dword position j) * x^(8 * kRowBytes)
  uint32_t x32[4][256];  // ... * x^32
  uint32_t pos[256];     // x^(128 n)
  uint32_t x2n[32];      // x^(2^n); x^(2^32) = x, so the table is periodic
};

constexpr void byte_tables(uint32_t (*t)[256], uint32_t factor) {
  for (int j = 0; j < 4; j++) {
    t[j][0] = 0;
    for (int bit = 0; bit < 8; bit++) t[j][1 << bit] = mulmod_c((uint32_t)1 << (8 * j + bit), factor);
    for (int b = 1; b < 256; b++)
      if (b & (b - 1)) t[j][b] = t[j][b & (b - 1)] ^ t[j][b & -b];
  }
}

constexpr int log2_of(int v) { return v <= 1 ? 0 : 1 + log2_of(v / 2); }

constexpr Tables make_tables() {
  Tables t{};
  uint32_t p = kOne >> 1;  // x
  for (int n = 0; n < 32; n++) {
    t.x2n[n] = p;
    p = mulmod_c(p, p);
  }
  static_assert((kRowBytes & (kRowBytes - 1)) == 0, "a row is a power of two");
  byte_tables(t.k, t.x2n[(3 + log2_of(kRowBytes)) & 31]);
  byte_tables(t.x32, t.x2n[5]);
  t.pos[0] = kOne;
  for (int n = 1; n < 256; n++) t.pos[n] = mulmod_c(t.pos[n - 1], t.x2n[7]);
  return t;
}

__device__ const Tables g_tab = make_tables();
constexpr int kTabWords = sizeof(Tables) / 4;
static_assert(kThreads <= 256, "pos[] covers the words behind a lane's last word: fewer than a row");

__device__ __forceinline__ uint32_t mulmod(uint32_t a, uint32_t b) {
  uint32_t p = 0;
#pragma unroll
  for (int i = 0; i < 32; i++) {
    p ^= (a & (kOne >> i)) ? b : 0u;
    b = (b >> 1) ^ ((b & 1) ? kPoly : 0u);
  }
  return p;
}

__device__ __forceinline__ uint32_t lookup4(const uint32_t* __restrict__ t, uint32_t a) {
  return t[a & 255] ^ t[256 + ((a >> 8) & 255)] ^ t[512 + ((a >> 16) & 255)] ^ t[768 + (a >> 24)];
}

__device__ __forceinline__ uint32_t wave_xor(uint32_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v ^= __shfl_xor(v, off, 64);
  return v;
}

// x^(8 n) mod P, 0 <= n < 2^31, by the 64 lanes of a wave together (every lane gets it): lane i < 31 holds x^(2^(i + 3)) if bit i
// of n is set, every other lane 1; five rounds of pairwise products
__device__ __forceinline__ uint32_t wave_xpow8(const uint32_t* __restrict__ x2n, uint32_t n, int lane) {
  uint32_t f = (lane < 31 && ((n >> lane) & 1)) ? x2n[(lane + 3) & 31] : kOne;
#pragma unroll
  for (int off = 1; off < 32; off <<= 1) f = mulmod(f, __shfl_xor(f, off, 64));
  return f;
}

__device__ __forceinline__ uint32_t crc_bytes(uint32_t c, const uint8_t* __restrict__ p, int n) {  // the byte path: bit by bit
  for (int i = 0; i < n; i++) {
    c ^= p[i];
#pragma unroll
    for (int b = 0; b < 8; b++) c = (c >> 1) ^ ((c & 1) ? kPoly : 0u);
  }
  return c;
}

struct FileCut {
  const uint8_t* base;
  int size, head;
  long long nwords;
};

__device__ __forceinline__ FileCut cut_file(const uint8_t* __restrict__ data, long long slot_bytes, const int32_t* __restrict__ sizes, long long f) {
  FileCut c;
  c.base = data + f * slot_bytes;
  const int s = sizes[f];
  c.size = s < 0 ? 0 : s;
  const int to_word = (int)((16 - ((uintptr_t)c.base & 15)) & 15);
  c.head = to_word < c.size ? to_word : c.size;
  c.nwords = (c.size - c.head) >> 4;
  return c;
}

// rows [r0, r1) of part p
__device__ __forceinline__ void part_rows(long long nwords, int parts, int p, long long* r0, long long* r1) {
  const long long rows = (nwords + kThreads - 1) / kThreads;
  const long long per = (rows + parts - 1) / parts;
  *r0 = (long long)p * per;
  const long long e = *r0 + per;
  *r1 = e < rows ? e : rows;
}

template <int VARIANT>
__global__ __launch_bounds__(kThreads) void zipw_crc_parts_kernel(const uint8_t* __restrict__ data, long long slot_bytes, const int32_t* __restrict__ sizes,
                                                                  long long nfiles, int parts, uint32_t* __restrict__ partial) {
  __shared__ uint32_t lds[kTabWords + 4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const uint32_t* gt = (const uint32_t*)&g_tab;
  for (int i = t; i < kTabWords; i += kThreads) lds[i] = gt[i];
  __syncthreads();
  const uint32_t* tk = lds;
  const uint32_t* t32 = lds + 1024;
  const uint32_t* pos = lds + 2048;
  const uint32_t* x2n = lds + 2304;
  uint32_t* red = lds + kTabWords;
  const uint32_t bigk = x2n[(3 + log2_of(kRowBytes)) & 31];
  const long long items = nfiles * parts;
  for (long long item = blockIdx.x; item < items; item += gridDim.x) {
    const long long f = item / parts;
    const int p = (int)(item - f * parts);
    const FileCut c = cut_file(data, slot_bytes, sizes, f);
    long long r0, r1;
    part_rows(c.nwords, parts, p, &r0, &r1);
    uint32_t result = 0;
    if (r0 < r1) {  // uniform over the workgroup
      const long long w0 = r0 * kThreads;
      const long long w1 = r1 * kThreads < c.nwords ? r1 * kThreads : c.nwords;
      const int nw = (int)(w1 - w0);  // < 2^27
      const uint4* __restrict__ wp = (const uint4*)(c.base + c.head) + w0;
      uint32_t a0 = 0, a1 = 0, a2 = 0, a3 = 0;
      int last = -1;
      const uint4 none = make_uint4(0, 0, 0, 0);
      uint4 d = t < nw ? wp[t] : none;
      for (int idx = t; idx < nw; idx += kThreads) {  // the next word is on its way while this one is folded
        const uint4 next = idx + kThreads < nw ? wp[idx + kThreads] : none;
        if (VARIANT == 0) {
          a0 = lookup4(tk, a0) ^ d.x;
          a1 = lookup4(tk, a1) ^ d.y;
          a2 = lookup4(tk, a2) ^ d.z;
          a3 = lookup4(tk, a3) ^ d.w;
        } else {
          a0 = mulmod(a0, bigk) ^ d.x;
          a1 = mulmod(a1, bigk) ^ d.y;
          a2 = mulmod(a2, bigk) ^ d.z;
          a3 = mulmod(a3, bigk) ^ d.w;
        }
        last = idx;
        d = next;
      }
      uint32_t r = 0;
      if (last >= 0) {
        r = lookup4(t32, a0) ^ a1;
        r = lookup4(t32, r) ^ a2;
        r = lookup4(t32, r) ^ a3;
        r = lookup4(t32, r);
        r = mulmod(r, pos[nw - 1 - last]);  // 0 .. kThreads - 1: last + kThreads >= nw
      }
      r = wave_xor(r);
      if (lane == 0) red[wave] = r;
      __syncthreads();
      if (wave == 0) {
        const uint32_t all = red[0] ^ red[1] ^ red[2] ^ red[3];
        const long long behind = (c.nwords - w1) * kWord;  // < 2^31
        result = behind ? mulmod(all, wave_xpow8(x2n, (uint32_t)behind, lane)) : all;
      }
      __syncthreads();
    }
    if (t == 0) partial[item] = result;
  }
}

__global__ __launch_bounds__(kThreads) void zipw_crc_finish_kernel(const uint8_t* __restrict__ data, long long slot_bytes, const int32_t* __restrict__ sizes,
                                                                   long long nfiles, int parts, const uint32_t* __restrict__ partial,
                                                                   uint32_t* __restrict__ crc) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long step = (long long)gridDim.x * (kThreads / 64);
  for (long long f = (long long)blockIdx.x * (kThreads / 64) + wave; f < nfiles; f += step) {
    const FileCut c = cut_file(data, slot_bytes, sizes, f);
    uint32_t body = 0;
    for (int p = lane; p < parts; p += 64) body ^= partial[f * parts + p];
    body = wave_xor(body);
    uint32_t v = crc_bytes(0xFFFFFFFFu, c.base, c.head);
    if (c.nwords) v = mulmod(v, wave_xpow8(g_tab.x2n, (uint32_t)(c.nwords * kWord), lane)) ^ body;
    const long long done = c.head + c.nwords * kWord;
    v = crc_bytes(v, c.base + done, (int)(c.size - done));
    if (lane == 0) crc[f] = ~v;
  }
}

// ---------------------------------------------------------------------------------------------------- the segment

struct Suffix {  // as four words, so that a byte is picked with selects and the kernel argument stays in registers
  uint32_t w[4];
  int len;
};

__host__ __device__ __forceinline__ uint8_t suffix_byte(const Suffix& s, int j) {
  const uint32_t w = j < 4 ? s.w[0] : j < 8 ? s.w[1] : j < 12 ? s.w[2] : s.w[3];
  return (uint8_t)(w >> (8 * (j & 3)));
}

__device__ __forceinline__ int digits_of(long long v) {  // of %05d
  int n = 1;
  while (v >= 10) {
    v /= 10;
    n++;
  }
  return n < 5 ? 5 : n;
}

// one workgroup: records[f] = {offset of file f's header or -1, crc, size}, records[nfiles].offset = the segment's length;
// an exclusive scan over 30 + name length + size in tiles of the workgroup's width with a 64-bit carry
__global__ __launch_bounds__(1024) void zipw_scan_kernel(const int32_t* __restrict__ sizes, const uint8_t* __restrict__ valid, const uint32_t* __restrict__ crc,
                                                         long long nfiles, long long first_index, int suffix_len, mdcz_record* __restrict__ records) {
  __shared__ long long wave_sum[16];
  __shared__ long long carry_s;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (t == 0) carry_s = 0;
  __syncthreads();
  for (long long first = 0; first < nfiles; first += 1024) {
    const long long f = first + t;
    long long len = 0;
    int size = 0;
    bool in = false;
    if (f < nfiles) {
      size = sizes[f] < 0 ? 0 : sizes[f];
      in = !valid || valid[f];
      if (in) len = 30 + digits_of(first_index + f) + suffix_len + (long long)size;
    }
    long long inc = len;  // inclusive scan inside the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const long long o = __shfl_up(inc, off, 64);
      if (lane >= off) inc += o;
    }
    if (lane == 63) wave_sum[wave] = inc;
    __syncthreads();
    long long before = carry_s;
    for (int w = 0; w < wave; w++) before += wave_sum[w];
    if (f < nfiles) {
      mdcz_record r;
      r.offset = in ? before + inc - len : -1;
      r.crc = crc[f];
      r.size = (uint32_t)size;
      records[f] = r;
    }
    __syncthreads();
    if (t == 1023) carry_s = before + inc;
    __syncthreads();
  }
  if (t == 0) {
    mdcz_record r;
    r.offset = carry_s;
    r.crc = 0;
    r.size = 0;
    records[nfiles] = r;
  }
}

__device__ __forceinline__ uint8_t header_byte(int k, uint32_t crc, uint32_t size, int nd, int name_len, long long index, const Suffix& sfx) {
  if (k >= 30) {
    const int j = k - 30;
    if (j >= nd) return suffix_byte(sfx, (j - nd) & 15);
    long long v = index;
    for (int i = nd - 1 - j; i > 0; i--) v /= 10;
    return (uint8_t)('0' + (int)(v % 10));
  }
  switch (k) {
    case 0: return 'P';
    case 1: return 'K';
    case 2: return 3;
    case 3: return 4;
    case 4: return 20;
    case 12: return 0x21;
    case 14: case 15: case 16: case 17: return (uint8_t)(crc >> (8 * (k - 14)));
    case 18: case 19: case 20: case 21: return (uint8_t)(size >> (8 * (k - 18)));
    case 22: case 23: case 24: case 25: return (uint8_t)(size >> (8 * (k - 22)));
    case 26: return (uint8_t)name_len;
    default: return 0;
  }
}

// file f's header, name and bytes -> segment + records[f].offset.  Workgroup `part` of the file's `parts` takes every parts-th row of
// kThreads 16-byte words of the DESTINATION (16-byte stores on 16-byte boundaries; the source is read with one 16-byte load at
// whatever alignment it has); part 0 also writes the header, the name and the bytes before and behind the destination's words.
__global__ __launch_bounds__(kThreads) void zipw_gather_kernel(const uint8_t* __restrict__ data, long long slot_bytes, const mdcz_record* __restrict__ records,
                                                               long long nfiles, int parts, long long first_index, Suffix sfx, uint8_t* __restrict__ segment,
                                                               long long capacity) {
  if (records[nfiles].offset > capacity) return;
  const int t = threadIdx.x;
  const long long items = nfiles * parts;
  for (long long item = blockIdx.x; item < items; item += gridDim.x) {
    const long long f = item / parts;
    const int p = (int)(item - f * parts);
    const mdcz_record r = records[f];
    if (r.offset < 0) continue;
    const int nd = digits_of(first_index + f), name_len = nd + sfx.len, hdr = 30 + name_len;
    uint8_t* __restrict__ dst = segment + r.offset + hdr;
    const uint8_t* __restrict__ src = data + f * slot_bytes;
    const int size = (int)r.size;
    const int to_word = (int)((16 - ((uintptr_t)dst & 15)) & 15);
    const int head = to_word < size ? to_word : size;
    const int nwords = (size - head) >> 4;
    const int tail = size - head - nwords * 16;
    if (p == 0) {
      if (t < hdr) segment[r.offset + t] = header_byte(t, r.crc, r.size, nd, name_len, first_index + f, sfx);
      if (t >= 64 && t < 64 + head) dst[t - 64] = src[t - 64];
      if (t >= 128 && t < 128 + tail) dst[size - tail + (t - 128)] = src[size - tail + (t - 128)];
    }
    for (long long w = (long long)p * kThreads + t; w < nwords; w += (long long)parts * kThreads) {
      uint4 v;
      __builtin_memcpy(&v, src + head + w * 16, 16);
      *(uint4*)(dst + head + w * 16) = v;
    }
  }
}

// ---------------------------------------------------------------------------------------------------- host side

int parts_for(int64_t slot_bytes, int64_t nfiles) {
  int64_t parts = (slot_bytes + (int64_t)kRowsPerPartHint * kRowBytes - 1) / ((int64_t)kRowsPerPartHint * kRowBytes);
  if (nfiles > 0 && nfiles * parts < kMaxParts) parts = (kMaxParts + nfiles - 1) / nfiles;  // few files: still fill the device
  return (int)(parts < 1 ? 1 : parts > kMaxParts ? kMaxParts : parts);
}

int grid_for(long long items) { return (int)(items < 1 ? 1 : items > kMaxGrid ? kMaxGrid : items); }

int check_suffix(const char* who, const char* suffix, Suffix* out) {
  if (!suffix) return fail(MDCZ_ERR_ARG, "%s: suffix is null", who);
  const size_t n = strlen(suffix);
  if (n > MDCZ_MAX_SUFFIX) return fail(MDCZ_ERR_ARG, "%s: the suffix has %zu bytes, more than %d", who, n, MDCZ_MAX_SUFFIX);
  memset(out, 0, sizeof *out);
  for (size_t i = 0; i < n; i++) {
    if ((unsigned char)suffix[i] >= 0x80) return fail(MDCZ_ERR_ARG, "%s: byte %zu of the suffix is not ASCII (0x%02x)", who, i, (unsigned char)suffix[i]);
    out->w[i >> 2] |= (uint32_t)(unsigned char)suffix[i] << (8 * (i & 3));
  }
  out->len = (int)n;
  return MDCZ_OK;
}

int check_batch(const char* who, const void* d_data, int64_t slot_bytes, const void* d_sizes, int64_t nfiles) {
  if (nfiles < 0) return fail(MDCZ_ERR_ARG, "%s: nfiles %lld is negative", who, (long long)nfiles);
  if (slot_bytes < 0) return fail(MDCZ_ERR_ARG, "%s: slot_bytes %lld is negative", who, (long long)slot_bytes);
  if (!d_data || !d_sizes) return fail(MDCZ_ERR_ARG, "%s: null pointer (d_data %p, d_sizes %p)", who, d_data, d_sizes);
  if (nfiles > (int64_t)1 << 40) return fail(MDCZ_ERR_ARG, "%s: nfiles %lld is above 2^40", who, (long long)nfiles);
  return MDCZ_OK;
}

int check_index(const char* who, int64_t first_index, int64_t nfiles) {
  if (first_index < 0 || first_index > 1000000000000000000ll - nfiles)
    return fail(MDCZ_ERR_ARG, "%s: first_index %lld with %lld files is outside 0..10^18", who, (long long)first_index, (long long)nfiles);
  return MDCZ_OK;
}

int launched(const char* who, const char* what) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MDCZ_OK : fail(MDCZ_ERR_HIP, "%s: launching %s failed: %s", who, what, hipGetErrorString(e));
}

// the scratch of one call, from the stream's pool and back to it when the call's kernels are done
struct Scratch {
  hipStream_t stream;
  void* p = nullptr;
  explicit Scratch(hipStream_t s) : stream(s) {}
  int get(const char* who, size_t bytes) {
    if (hipMallocAsync(&p, bytes ? bytes : 4, stream) != hipSuccess) {
      p = nullptr;
      (void)hipGetLastError();
      return fail(MDCZ_ERR_NOMEM, "%s: could not allocate %zu bytes of scratch", who, bytes);
    }
    return MDCZ_OK;
  }
  ~Scratch() {
    if (p) (void)hipFreeAsync(p, stream);
  }
};

// arguments checked by the caller; partial: nfiles * parts words
int crc_launch(const char* who, int variant, const uint8_t* d_data, int64_t slot_bytes, const int32_t* d_sizes, int64_t nfiles, int parts, uint32_t* partial,
               uint32_t* d_crc, hipStream_t s) {
  if (nfiles == 0) return MDCZ_OK;
  const long long items = (long long)nfiles * parts;
  if (variant == 0)
    hipLaunchKernelGGL(zipw_crc_parts_kernel<0>, dim3(grid_for(items)), dim3(kThreads), 0, s, d_data, (long long)slot_bytes, d_sizes, (long long)nfiles, parts,
                       partial);
  else
    hipLaunchKernelGGL(zipw_crc_parts_kernel<1>, dim3(grid_for(items)), dim3(kThreads), 0, s, d_data, (long long)slot_bytes, d_sizes, (long long)nfiles, parts,
                       partial);
  if (int rc = launched(who, "the checksum kernel")) return rc;
  hipLaunchKernelGGL(zipw_crc_finish_kernel, dim3(grid_for((nfiles + 3) / 4)), dim3(kThreads), 0, s, d_data, (long long)slot_bytes, d_sizes, (long long)nfiles,
                     parts, (const uint32_t*)partial, d_crc);
  return launched(who, "the checksum's last step");
}

int crc_call(const char* who, int variant, const uint8_t* d_data, int64_t slot_bytes, const int32_t* d_sizes, int64_t nfiles, uint32_t* d_crc, void* stream) {
  if (int rc = check_batch(who, d_data, slot_bytes, d_sizes, nfiles)) return rc;
  if (!d_crc) return fail(MDCZ_ERR_ARG, "%s: d_crc is null", who);
  if (variant != 0 && variant != 1) return fail(MDCZ_ERR_ARG, "%s: variant %d is neither 0 nor 1", who, variant);
  if (nfiles == 0) return MDCZ_OK;
  const int parts = parts_for(slot_bytes, nfiles);
  Scratch sc((hipStream_t)stream);
  if (int rc = sc.get(who, (size_t)nfiles * parts * 4)) return rc;
  return crc_launch(who, variant, d_data, slot_bytes, d_sizes, nfiles, parts, (uint32_t*)sc.p, d_crc, (hipStream_t)stream);
}

int segment_call(const char* who, const uint8_t* d_data, int64_t slot_bytes, const int32_t* d_sizes, const uint8_t* d_valid, int64_t nfiles, int64_t first_index,
                 const Suffix& sfx, uint8_t* d_segment, int64_t capacity, mdcz_record* d_records, hipStream_t s) {
  const int parts = parts_for(slot_bytes, nfiles);
  Scratch sc(s);
  const size_t partial_bytes = (size_t)nfiles * parts * 4;
  if (int rc = sc.get(who, partial_bytes + (size_t)nfiles * 4)) return rc;
  uint32_t* partial = (uint32_t*)sc.p;
  uint32_t* d_crc = (uint32_t*)((char*)sc.p + partial_bytes);
  if (int rc = crc_launch(who, 0, d_data, slot_bytes, d_sizes, nfiles, parts, partial, d_crc, s)) return rc;
  hipLaunchKernelGGL(zipw_scan_kernel, dim3(1), dim3(1024), 0, s, d_sizes, d_valid, (const uint32_t*)d_crc, (long long)nfiles, (long long)first_index, sfx.len,
                     d_records);
  if (int rc = launched(who, "the scan kernel")) return rc;
  if (nfiles == 0) return MDCZ_OK;
  hipLaunchKernelGGL(zipw_gather_kernel, dim3(grid_for((long long)nfiles * parts)), dim3(kThreads), 0, s, d_data, (long long)slot_bytes,
                     (const mdcz_record*)d_records, (long long)nfiles, parts, (long long)first_index, sfx, d_segment, (long long)capacity);
  return launched(who, "the gather kernel");
}

int name_of(int64_t index, const Suffix& sfx, char* out) {  // -> length
  const int n = snprintf(out, 24, "%05lld", (long long)index);
  for (int i = 0; i < sfx.len; i++) out[n + i] = (char)suffix_byte(sfx, i);
  out[n + sfx.len] = 0;
  return n + sfx.len;
}

struct Out {  // little-endian fields into a buffer
  uint8_t* p;
  void u16(unsigned v) {
    *p++ = (uint8_t)v;
    *p++ = (uint8_t)(v >> 8);
  }
  void u32(uint32_t v) {
    u16(v & 0xffff);
    u16(v >> 16);
  }
  void u64(uint64_t v) {
    u32((uint32_t)v);
    u32((uint32_t)(v >> 32));
  }
  void bytes(const void* s, size_t n) {
    memcpy(p, s, n);
    p += n;
  }
};

constexpr uint64_t k32 = 0xFFFFFFFFull;
constexpr unsigned kMadeBy = 20 | (3 << 8);  // 2.0, Unix
constexpr unsigned kDosDate = 0x0021;        // 1980-01-01, time 0

bool write_all(int fd, const uint8_t* p, int64_t n) {
  while (n > 0) {
    const ssize_t k = write(fd, p, (size_t)(n > (1ll << 30) ? (1ll << 30) : n));
    if (k < 0) {
      if (errno == EINTR) continue;
      return false;
    }
    p += k;
    n -= k;
  }
  return true;
}

}  // namespace

struct mdcz_writer {
  int fd = -1;
  int device = -1;
  std::string path;
  int64_t cap = 0;
  int64_t file_size = 0;
  std::vector<mdcz_record> entries;  // offsets absolute
  std::vector<char> names;           // MDCZ_NAME_STRIDE each
  uint8_t* d_stage = nullptr;        // [segment | up to 15 bytes | records]
  uint8_t* h_stage = nullptr;        // page-locked, the same layout
  int64_t stage_capacity = 0;
  uint8_t* d_valid = nullptr;
  uint8_t* h_valid = nullptr;  // page-locked
  int64_t valid_capacity = 0;
  std::vector<int32_t> sizes;
};

namespace {

void free_writer(mdcz_writer* w) {
  if (w->d_stage || w->h_stage || w->d_valid || w->h_valid) {
    DeviceGuard dg(w->device);
    (void)hipFree(w->d_stage);
    (void)hipHostFree(w->h_stage);
    (void)hipFree(w->d_valid);
    (void)hipHostFree(w->h_valid);
  }
  if (w->fd >= 0) close(w->fd);
  delete w;
}

int grow(const char* who, mdcz_writer* w, int64_t stage, int64_t nvalid) {
  if (stage > w->stage_capacity) {
    (void)hipFree(w->d_stage);
    (void)hipHostFree(w->h_stage);
    w->d_stage = w->h_stage = nullptr;
    w->stage_capacity = 0;
    if (hipMalloc((void**)&w->d_stage, (size_t)stage) != hipSuccess || hipHostMalloc((void**)&w->h_stage, (size_t)stage, hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError();
      return fail(MDCZ_ERR_NOMEM, "%s: could not allocate the staging buffers of %lld bytes", who, (long long)stage);
    }
    w->stage_capacity = stage;
  }
  if (nvalid > w->valid_capacity) {
    (void)hipFree(w->d_valid);
    (void)hipHostFree(w->h_valid);
    w->d_valid = w->h_valid = nullptr;
    w->valid_capacity = 0;
    if (hipMalloc((void**)&w->d_valid, (size_t)nvalid) != hipSuccess || hipHostMalloc((void**)&w->h_valid, (size_t)nvalid, hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError();
      return fail(MDCZ_ERR_NOMEM, "%s: could not allocate %lld flags", who, (long long)nvalid);
    }
    w->valid_capacity = nvalid;
  }
  return MDCZ_OK;
}

}  // namespace

extern "C" {

const char* mdcz_last_error(void) { return g_error; }

void mdcz_crc_geometry(int64_t slot_bytes, int64_t nfiles, int64_t* out) {
  if (!out) return;
  out[0] = kWord;
  out[1] = kRowBytes;
  out[2] = 64 * kWord;
  out[3] = kRowBytes;
  out[4] = parts_for(slot_bytes < 0 ? 0 : slot_bytes, nfiles);
}

int mdcz_crc32_device(const uint8_t* d_data, int64_t slot_bytes, const int32_t* d_sizes, int64_t nfiles, uint32_t* d_crc, void* stream) {
  return crc_call("mdcz_crc32_device", 0, d_data, slot_bytes, d_sizes, nfiles, d_crc, stream);
}

int mdcz_crc32_variant_device(int variant, const uint8_t* d_data, int64_t slot_bytes, const int32_t* d_sizes, int64_t nfiles, uint32_t* d_crc, void* stream) {
  return crc_call("mdcz_crc32_variant_device", variant, d_data, slot_bytes, d_sizes, nfiles, d_crc, stream);
}

int64_t mdcz_segment_bound(int64_t nfiles, int64_t total_bytes, int max_name_len) {
  if (nfiles < 0 || total_bytes < 0 || max_name_len < 0) return -1;
  const int64_t per = 30 + (int64_t)max_name_len;
  if (nfiles > (INT64_MAX - total_bytes) / per) return -1;
  return nfiles * per + total_bytes;
}

int mdcz_segment_device(const uint8_t* d_data, int64_t slot_bytes, const int32_t* d_sizes, const uint8_t* d_valid, int64_t nfiles, int64_t first_index,
                        const char* suffix, uint8_t* d_segment, int64_t segment_capacity, mdcz_record* d_records, void* stream) {
  const char* who = "mdcz_segment_device";
  if (int rc = check_batch(who, d_data, slot_bytes, d_sizes, nfiles)) return rc;
  if (!d_segment || !d_records) return fail(MDCZ_ERR_ARG, "%s: null pointer (d_segment %p, d_records %p)", who, (void*)d_segment, (void*)d_records);
  if (segment_capacity < 0) return fail(MDCZ_ERR_ARG, "%s: segment_capacity %lld is negative", who, (long long)segment_capacity);
  if (int rc = check_index(who, first_index, nfiles)) return rc;
  Suffix sfx;
  if (int rc = check_suffix(who, suffix, &sfx)) return rc;
  return segment_call(who, d_data, slot_bytes, d_sizes, d_valid, nfiles, first_index, sfx, d_segment, segment_capacity, d_records, (hipStream_t)stream);
}

int64_t mdcz_directory(const mdcz_record* records, int64_t n, const char* names, int64_t segment_base_offset, int64_t directory_offset, uint8_t* out,
                       int64_t capacity) {
  const char* who = "mdcz_directory";
  if (n < 0) return fail(MDCZ_ERR_ARG, "%s: n %lld is negative", who, (long long)n);
  if (n > 0 && (!records || !names)) return fail(MDCZ_ERR_ARG, "%s: null pointer (records %p, names %p)", who, (const void*)records, (const void*)names);
  if (segment_base_offset < 0 || directory_offset < 0)
    return fail(MDCZ_ERR_ARG, "%s: negative offset (segment base %lld, directory %lld)", who, (long long)segment_base_offset, (long long)directory_offset);
  if (out && capacity < 0) return fail(MDCZ_ERR_ARG, "%s: capacity %lld is negative", who, (long long)capacity);
  uint64_t count = 0, dir_size = 0;
  for (int64_t i = 0; i < n; i++) {
    if (records[i].offset < 0) continue;
    const size_t len = strnlen(names + i * MDCZ_NAME_STRIDE, MDCZ_NAME_STRIDE);
    if (len >= MDCZ_NAME_STRIDE) return fail(MDCZ_ERR_ARG, "%s: name %lld is not terminated within %d bytes", who, (long long)i, MDCZ_NAME_STRIDE);
    count++;
    dir_size += 46 + len + ((uint64_t)(segment_base_offset + records[i].offset) >= k32 ? 12 : 0);
  }
  const bool zip64 = count > 65534 || (uint64_t)directory_offset >= k32 || dir_size >= k32;
  const int64_t need = (int64_t)dir_size + (zip64 ? 56 + 20 : 0) + 22;
  if (!out) return need;
  if (capacity < need) return fail(MDCZ_ERR_SIZE, "%s: capacity %lld is below the %lld bytes of the directory", who, (long long)capacity, (long long)need);
  Out o{out};
  for (int64_t i = 0; i < n; i++) {
    if (records[i].offset < 0) continue;
    const char* name = names + i * MDCZ_NAME_STRIDE;
    const size_t len = strlen(name);
    const uint64_t at = (uint64_t)(segment_base_offset + records[i].offset);
    const bool far = at >= k32;
    o.u32(0x02014b50);
    o.u16(kMadeBy);
    o.u16(far ? 45 : 20);
    o.u16(0);  // flags
    o.u16(0);  // stored
    o.u16(0);  // time
    o.u16(kDosDate);
    o.u32(records[i].crc);
    o.u32(records[i].size);
    o.u32(records[i].size);
    o.u16((unsigned)len);
    o.u16(far ? 12 : 0);
    o.u16(0);  // comment
    o.u16(0);  // disk
    o.u16(0);  // internal attributes
    o.u32(0);  // external attributes
    o.u32(far ? (uint32_t)k32 : (uint32_t)at);
    o.bytes(name, len);
    if (far) {
      o.u16(0x0001);
      o.u16(8);
      o.u64(at);
    }
  }
  if (zip64) {
    o.u32(0x06064b50);
    o.u64(44);
    o.u16(kMadeBy);
    o.u16(45);
    o.u32(0);
    o.u32(0);
    o.u64(count);
    o.u64(count);
    o.u64(dir_size);
    o.u64((uint64_t)directory_offset);
    o.u32(0x07064b50);
    o.u32(0);
    o.u64((uint64_t)directory_offset + dir_size);
    o.u32(1);
  }
  o.u32(0x06054b50);
  o.u16(0);
  o.u16(0);
  o.u16((unsigned)(count > 0xFFFF ? 0xFFFF : count));
  o.u16((unsigned)(count > 0xFFFF ? 0xFFFF : count));
  o.u32((uint32_t)(dir_size > k32 ? k32 : dir_size));
  o.u32((uint32_t)((uint64_t)directory_offset > k32 ? k32 : (uint64_t)directory_offset));
  o.u16(0);
  return need;
}

int mdcz_open(const char* path, int device, int64_t staging_cap, mdcz_writer** out) {
  if (!out) return fail(MDCZ_ERR_ARG, "mdcz_open: out is null");
  *out = nullptr;
  if (!path) return fail(MDCZ_ERR_ARG, "mdcz_open: path is null");
  mdcz_writer* w = new (std::nothrow) mdcz_writer;
  if (!w) return fail(MDCZ_ERR_NOMEM, "mdcz_open: out of host memory");
  w->fd = open(path, O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0666);
  if (w->fd < 0) {
    const int e = errno;
    delete w;
    return fail(MDCZ_ERR_IO, "mdcz_open: cannot create %s: %s", path, strerror(e));
  }
  w->path = path;
  w->device = device;
  w->cap = staging_cap > 0 ? staging_cap : (int64_t)256 << 20;
  *out = w;
  return MDCZ_OK;
}

int mdcz_append_device(mdcz_writer* w, const uint8_t* d_data, int64_t slot_bytes, const int32_t* d_sizes, const uint8_t* h_valid, int64_t nfiles,
                       int64_t first_index, const char* suffix, void* stream) {
  const char* who = "mdcz_append_device";
  if (!w) return fail(MDCZ_ERR_ARG, "%s: the writer is null", who);
  if (int rc = check_batch(who, d_data, slot_bytes, d_sizes, nfiles)) return rc;
  if (int rc = check_index(who, first_index, nfiles)) return rc;
  Suffix sfx;
  if (int rc = check_suffix(who, suffix, &sfx)) return rc;
  if (nfiles == 0) return MDCZ_OK;
  if (w->device < 0 && hipGetDevice(&w->device) != hipSuccess) return fail(MDCZ_ERR_NO_DEVICE, "%s: no current HIP device", who);
  DeviceGuard dg(w->device);
  hipStream_t s = (hipStream_t)stream;
  try {
    w->sizes.resize((size_t)nfiles);
  } catch (const std::bad_alloc&) {
    return fail(MDCZ_ERR_NOMEM, "%s: out of host memory for %lld sizes", who, (long long)nfiles);
  }
  if (hipMemcpyAsync(w->sizes.data(), d_sizes, (size_t)nfiles * 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
    return fail(MDCZ_ERR_HIP, "%s: reading the sizes failed: %s", who, hipGetErrorString(hipGetLastError()));
  for (int64_t f = 0; f < nfiles; f++)
    if (w->sizes[(size_t)f] < 0) return fail(MDCZ_ERR_ARG, "%s: the size of file %lld is negative (%d)", who, (long long)f, w->sizes[(size_t)f]);
  for (int64_t first = 0; first < nfiles;) {
    // the longest run of files whose segment and records stay below the cap (one file at least)
    int64_t n = 0, seg = 0;
    while (first + n < nfiles) {
      const int64_t f = first + n;
      char name[MDCZ_NAME_STRIDE];
      const int64_t len = (!h_valid || h_valid[f]) ? 30 + name_of(first_index + f, sfx, name) + (int64_t)w->sizes[(size_t)f] : 0;
      if (n > 0 && ((seg + len + 15) & ~15ll) + (n + 2) * (int64_t)sizeof(mdcz_record) > w->cap) break;
      seg += len;
      n++;
    }
    const int64_t rec_at = (seg + 15) & ~15ll;
    const int64_t stage = rec_at + (n + 1) * (int64_t)sizeof(mdcz_record);
    if (int rc = grow(who, w, stage, h_valid ? n : 0)) return rc;
    if (h_valid) {
      memcpy(w->h_valid, h_valid + first, (size_t)n);
      if (hipMemcpyAsync(w->d_valid, w->h_valid, (size_t)n, hipMemcpyHostToDevice, s) != hipSuccess)
        return fail(MDCZ_ERR_HIP, "%s: copying the flags failed: %s", who, hipGetErrorString(hipGetLastError()));
    }
    if (int rc = segment_call(who, d_data + first * slot_bytes, slot_bytes, d_sizes + first, h_valid ? w->d_valid : nullptr, n, first_index + first, sfx,
                              w->d_stage, seg, (mdcz_record*)(w->d_stage + rec_at), s))
      return rc;
    if (hipMemcpyAsync(w->h_stage, w->d_stage, (size_t)stage, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
      return fail(MDCZ_ERR_HIP, "%s: copying the segment failed: %s", who, hipGetErrorString(hipGetLastError()));
    const mdcz_record* rec = (const mdcz_record*)(w->h_stage + rec_at);
    if (rec[n].offset != seg)
      return fail(MDCZ_ERR_STATE, "%s: the segment is %lld bytes on the device, %lld by the sizes read before: d_sizes changed during the call", who,
                  (long long)rec[n].offset, (long long)seg);
    if (!write_all(w->fd, w->h_stage, seg)) return fail(MDCZ_ERR_IO, "%s: writing %s failed: %s", who, w->path.c_str(), strerror(errno));
    try {
      for (int64_t i = 0; i < n; i++) {
        if (rec[i].offset < 0) continue;
        mdcz_record e = rec[i];
        e.offset += w->file_size;
        w->entries.push_back(e);
        char name[MDCZ_NAME_STRIDE] = {0};
        name_of(first_index + first + i, sfx, name);
        w->names.insert(w->names.end(), name, name + MDCZ_NAME_STRIDE);
      }
    } catch (const std::bad_alloc&) {
      return fail(MDCZ_ERR_NOMEM, "%s: out of host memory for the directory", who);
    }
    w->file_size += seg;
    first += n;
  }
  return MDCZ_OK;
}

int64_t mdcz_close(mdcz_writer* w) {
  const char* who = "mdcz_close";
  if (!w) return fail(MDCZ_ERR_ARG, "%s: the writer is null", who);
  const int64_t n = (int64_t)w->entries.size();
  int64_t rc = mdcz_directory(w->entries.data(), n, w->names.data(), 0, w->file_size, nullptr, 0);
  if (rc >= 0) {
    uint8_t* dir = (uint8_t*)malloc((size_t)rc);
    if (!dir) {
      rc = fail(MDCZ_ERR_NOMEM, "%s: out of host memory for a directory of %lld bytes", who, (long long)rc);
    } else {
      rc = mdcz_directory(w->entries.data(), n, w->names.data(), 0, w->file_size, dir, rc);
      if (rc >= 0 && !write_all(w->fd, dir, rc)) rc = fail(MDCZ_ERR_IO, "%s: writing %s failed: %s", who, w->path.c_str(), strerror(errno));
      free(dir);
    }
  }
  if (rc >= 0) {
    rc += w->file_size;
    const int fd = w->fd;
    w->fd = -1;
    if (close(fd) != 0) rc = fail(MDCZ_ERR_IO, "%s: closing %s failed: %s", who, w->path.c_str(), strerror(errno));
  }
  free_writer(w);
  return rc;
}

void mdcz_abort(mdcz_writer* w) {
  if (!w) return;
  if (w->fd >= 0) {
    close(w->fd);
    w->fd = -1;
    (void)unlink(w->path.c_str());
  }
  free_writer(w);
}

}  // extern "C"
