// What the two device PNG decoder libraries share (libmdc_pngd.so: mdc_pngd.hip, libmdc_pngdx.so: mdc_pngdx.hip), each of which is one
// translation unit that includes this header once: the four kernels of libmdc_pngd.so and the host side of both libraries, which each
// parametrises with a Params and the launch sequence of its call.  Everything is in
// an unnamed namespace: each library gets its own copy, neither exports any of it.
//
//   pngd_front_kernel     one workgroup per image: lane 0 parses the zlib header and the first block header and builds the code
//                         tables in LDS (pngd::classify).  A literal-only final dynamic block is decoded here: every thread owns a
//                         subsequence of the bits, decodes it from a guessed entry, and the entries relax to the sequential
//                         decoder's in at most as many rounds as there are subsequences; a scan over the symbol counts, then a
//                         second pass writes the filtered bytes.  A chain of stored blocks: lane 0 hops the headers, everybody copies.
//                         Anything irregular is left to the next kernel, untouched.
//   pngd_general_kernel   one wave per image that is not done yet: pngd::inflate, symbol by symbol.  Lane 0 parses a block's header and
//                         builds its tables in LDS; after a barrier every lane runs the same symbol decode on them; literals are lane 0's stores, a match is copied by the whole wave (source index modulo the
//                         distance, so an overlapping match reads only bytes from before it).
//   pngd_check_kernel     Adler-32 of the filtered bytes as a reduction, the trailer, the rows' filter types.
//   pngd_unfilter_kernel  one wave per image, 64 rows at a time as an anti-diagonal wavefront: lane r is at column t - r in step t, "up" is
//                         what lane r - 1 produced one step ago, "up-left" what it produced two steps ago (one DPP shift per step);
//                         a band's first row reads the previous band's last from the output.  Writes d_status.
#ifndef MDC_PNG_DECODE_KERNELS_H
#define MDC_PNG_DECODE_KERNELS_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <new>

#include "codec_host.h"
#include "png_inflate_core.h"

namespace {

constexpr int kFrontThreads = 1024;
constexpr int kMinSubBits = 64;  // a subsequence is at least this long (a code is at most 15 bits)
constexpr int kMaxGrid = 8192;
constexpr uint32_t kEnd = 0xffffffffu, kErr = 0xfffffffeu;  // exit states that are no bit position
constexpr int kMetaWords = 4;  // per image: reason, path, the trailer's byte offset, 1 = the filtered bytes are complete and good so far

struct Input {
  const uint8_t* slots;
  long long slot_bytes;
  const int32_t* sizes;
  int skip_head, skip_tail;
};

__device__ __forceinline__ const uint8_t* stream_of(const Input& in, long long f, uint32_t* n) {
  long long size = in.sizes[f];
  if (size > in.slot_bytes) size = in.slot_bytes;
  size -= (long long)in.skip_head + in.skip_tail;
  if (size < 0) size = 0;
  if (size > (long long)pngd::kMaxStreamBytes) size = pngd::kMaxStreamBytes;
  *n = (uint32_t)size;
  return in.slots + f * in.slot_bytes + in.skip_head;
}

// Symbols from bit `entry` until the position reaches `end`, the end-of-block code or something that is no literal.
template <bool WRITE>
__device__ __forceinline__ void span(const pngd::Code& lit, const uint8_t* p, uint32_t n, uint32_t entry, uint32_t end, uint32_t* exit, uint32_t* count,
                                     uint32_t* end_bit, uint8_t* __restrict__ out) {
  pngd::Bits b;
  b.seek(p, n, entry);
  uint32_t c = 0, ex = 0;
  bool open = true;
  while (open && b.bitpos() < end) {  // a round takes at least one bit
    const int s = pngd::decode(lit, b);
    if (s < 0 || s > 256) {
      ex = kErr, open = false;
    } else if (s == 256) {
      ex = kEnd, open = false;
      *end_bit = b.bitpos();
    } else {
      if (WRITE) out[c] = (uint8_t)s;
      c++;
    }
  }
  *exit = open ? b.bitpos() : ex;
  *count = c;
}

__global__ __launch_bounds__(kFrontThreads) void pngd_front_kernel(Input in, long long nimages, uint32_t F, uint8_t* __restrict__ filt, long long filt_stride,
                                                                   uint32_t* __restrict__ meta) {
  __shared__ pngd::Work w;
  __shared__ uint32_t exit_s[kFrontThreads];
  __shared__ uint32_t blk_src[pngd::kMaxStoredBlocks], blk_dst[pngd::kMaxStoredBlocks], blk_len[pngd::kMaxStoredBlocks];
  __shared__ uint32_t wave_total[kFrontThreads / 64];
  __shared__ uint32_t sh_path, sh_data_bit, sh_nblk, sh_end, sh_ok;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  for (long long f = blockIdx.x; f < nimages; f += gridDim.x) {
    uint32_t n;
    const uint8_t* __restrict__ p = stream_of(in, f, &n);
    uint8_t* __restrict__ out = filt + f * filt_stride;
    __syncthreads();
    if (t == 0) {
      uint32_t data_bit = 0;
      int path = pngd::classify(w, p, n, &data_bit);
      uint32_t nblk = 0, end = 0;
      if (path == pngd::PATH_STORED && !pngd::stored_chain(p, n, F, blk_src, blk_dst, blk_len, &nblk, &end)) path = pngd::PATH_GENERAL;
      sh_path = (uint32_t)path, sh_data_bit = data_bit, sh_nblk = nblk, sh_end = end, sh_ok = 0;
    }
    __syncthreads();
    const uint32_t path = sh_path;
    if (path == pngd::PATH_STORED) {
      for (uint32_t k = 0; k < sh_nblk; k++) {
        const uint8_t* __restrict__ src = p + blk_src[k];
        uint8_t* __restrict__ dst = out + blk_dst[k];
        for (uint32_t i = t; i < blk_len[k]; i += kFrontThreads) dst[i] = src[i];
      }
      if (t == 0) meta[f * kMetaWords + 0] = 0, meta[f * kMetaWords + 1] = pngd::PATH_STORED, meta[f * kMetaWords + 2] = sh_end, meta[f * kMetaWords + 3] = 1;
      continue;
    }
    const uint32_t data_bit = sh_data_bit, end_all = n * 8u;
    if (path != pngd::PATH_PARALLEL || data_bit >= end_all) {
      if (t == 0) meta[f * kMetaWords + 0] = 0, meta[f * kMetaWords + 1] = 0, meta[f * kMetaWords + 2] = 0, meta[f * kMetaWords + 3] = 0;
      continue;
    }
    const uint32_t nb = end_all - data_bit;
    uint32_t S = (nb + kFrontThreads - 1) / kFrontThreads;
    if (S < (uint32_t)kMinSubBits) S = kMinSubBits;
    const uint32_t nsub = (nb + S - 1) / S;  // 1 .. kFrontThreads
    const bool mine = (uint32_t)t < nsub;
    const uint32_t start = data_bit + (uint32_t)t * S;
    const uint32_t end = mine ? (end_all - start < S ? end_all : start + S) : 0;
    uint32_t entry = start, my_exit = kErr, my_count = 0, my_end_bit = 0;
    if (mine) span<false>(w.lit, p, n, entry, end, &my_exit, &my_count, &my_end_bit, nullptr);
    for (uint32_t round = 0; round <= nsub; round++) {  // after round k the subsequences 0 .. k hold the sequential decoder's states
      exit_s[t] = my_exit;
      __syncthreads();
      const uint32_t want = t == 0 ? data_bit : exit_s[t - 1];
      const bool changed = mine && want != entry;
      if (!__syncthreads_or(changed ? 1 : 0)) break;
      if (changed) {
        entry = want;
        if (entry >= kErr) my_exit = entry, my_count = 0;
        else span<false>(w.lit, p, n, entry, end, &my_exit, &my_count, &my_end_bit, nullptr);
      }
    }
    // exit_s holds the final states.  The block ended where the one subsequence with a position as entry and kEnd as exit says
    if (mine && entry < kErr && my_exit == kEnd) sh_end = (my_end_bit + 7u) >> 3;
    uint32_t inc = mine ? my_count : 0;  // inclusive scan; the total may wrap only for a stream that is wrong anyway (it cannot: <= nb)
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t other = __shfl_up(inc, o, 64);
      if (lane >= o) inc += other;
    }
    if (lane == 63) wave_total[wave] = inc;
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (int k = 0; k < kFrontThreads / 64; k++) {
      before += k < wave ? wave_total[k] : 0;
      total += wave_total[k];
    }
    const bool ok = exit_s[nsub - 1] == kEnd && total == F;
    if (ok && mine && entry < kErr) {
      uint32_t e2, c2, b2;
      span<true>(w.lit, p, n, entry, end, &e2, &c2, &b2, out + (before + inc - my_count));  // my_count symbols again, all below F
    }
    __syncthreads();
    if (t == 0) {
      meta[f * kMetaWords + 0] = 0, meta[f * kMetaWords + 1] = ok ? (uint32_t)pngd::PATH_PARALLEL : 0u;
      meta[f * kMetaWords + 2] = ok ? sh_end : 0u, meta[f * kMetaWords + 3] = ok ? 1u : 0u;
    }
  }
}

// The sequential decoder's output, written by a wave: every lane runs the same decode, so `pos` is the same in all of them
struct WaveOut {
  uint8_t* out;
  uint32_t pos;
  int lane;
  __device__ __forceinline__ bool builder() const { return lane == 0; }
  __device__ __forceinline__ void barrier() const { __syncthreads(); }  // the workgroup is this one wave; control flow is the same in all lanes
  __device__ __forceinline__ void put(uint8_t v) {
    if (lane == 0) out[pos] = v;
    pos++;
  }
  __device__ __forceinline__ void copy(uint32_t dist, uint32_t len) {
    // The bytes before this match -- lane 0's literals, other lanes' parts of earlier matches -- must be visible to every lane before it
    // loads.  All of them are this wave's own stores through this compute unit's vector cache: the workgroup-scope fence waits for them
    // to be done there, which is enough on gfx950 as built here (no threadgroup-split mode, where a workgroup may span compute units).
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    const uint8_t* src = out + (pos - dist);
    for (uint32_t i = lane; i < len; i += 64) out[pos + i] = src[dist >= len ? i : i % dist];  // len <= 258
    pos += len;
  }
  __device__ __forceinline__ void stored(const uint8_t* __restrict__ src, uint32_t len) {
    for (uint32_t i = lane; i < len; i += 64) out[pos + i] = src[i];  // len <= 65535
    pos += len;
  }
};

__global__ __launch_bounds__(64) void pngd_general_kernel(Input in, long long nimages, uint32_t F, uint8_t* __restrict__ filt, long long filt_stride,
                                                          uint32_t* __restrict__ meta) {
  __shared__ pngd::Work w;
  for (long long f = blockIdx.x; f < nimages; f += gridDim.x) {
    if (meta[f * kMetaWords + 3] != 0) continue;  // done by the front kernel
    uint32_t n, end_byte = 0;
    const uint8_t* p = stream_of(in, f, &n);
    WaveOut out = {filt + f * filt_stride, 0, (int)threadIdx.x};
    const int st = pngd::inflate(w, p, n, out, F, &end_byte);
    if (threadIdx.x == 0) {
      meta[f * kMetaWords + 0] = (uint32_t)st, meta[f * kMetaWords + 1] = pngd::PATH_GENERAL;
      meta[f * kMetaWords + 2] = end_byte, meta[f * kMetaWords + 3] = st == pngd::ST_OK ? 1u : 0u;
    }
  }
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__global__ __launch_bounds__(256) void pngd_check_kernel(Input in, long long nimages, int w, int h, const uint8_t* __restrict__ filt, long long filt_stride,
                                                         uint32_t* __restrict__ meta) {
  __shared__ unsigned long long part[2][4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const uint32_t rs = 1u + (uint32_t)w, F = rs * (uint32_t)h;
  for (long long f = blockIdx.x; f < nimages; f += gridDim.x) {
    if (meta[f * kMetaWords + 3] == 0) continue;  // (the same for the whole workgroup)
    const uint8_t* __restrict__ src = filt + f * filt_stride;
    const uint32_t* __restrict__ src4 = (const uint32_t*)src;  // filt_stride is a multiple of 16: whole words, the last one padded
    unsigned long long s1 = 0, s2 = 0;  // (F - i) d < 2^36, at most 2^20 terms per thread
    for (uint32_t u = t; u < (F + 3) / 4; u += 256) {
      const uint32_t v = src4[u];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const uint32_t i = 4 * u + k, d = i < F ? (v >> (8 * k)) & 255u : 0u;
        s1 += d;
        s2 += (unsigned long long)(F - i) * d;
      }
    }
    int bad = 0;
    for (uint32_t r = t; r < (uint32_t)h; r += 256) bad |= src[r * rs] > 4 ? 1 : 0;
    s1 = wave_sum(s1), s2 = wave_sum(s2 % pngd::kAdlerMod);
    __syncthreads();
    if (lane == 0) part[0][wave] = s1, part[1][wave] = s2;
    bad = __syncthreads_or(bad);
    if (t == 0) {
      uint32_t n;
      const uint8_t* p = stream_of(in, f, &n);
      const uint32_t adler = pngd::adler_of(part[0][0] + part[0][1] + part[0][2] + part[0][3], part[1][0] + part[1][1] + part[1][2] + part[1][3], F);
      int st = pngd::check_trailer(p, n, meta[f * kMetaWords + 2], adler);
      if (st == pngd::ST_OK && bad) st = pngd::ST_FILTER_TYPE;
      meta[f * kMetaWords + 0] = (uint32_t)st;
      meta[f * kMetaWords + 3] = st == pngd::ST_OK ? 1u : 0u;
    }
  }
}

// lane r's value of the previous step, seen from lane r + 1 (lane 0 gets 0): one DPP move, no LDS
__device__ __forceinline__ int from_lane_above(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x138 /* wave_shr:1 */, 0xf, 0xf, false); }

__global__ __launch_bounds__(64) void pngd_unfilter_kernel(long long nimages, int w, int h, const uint8_t* __restrict__ filt, long long filt_stride,
                                                           const uint32_t* __restrict__ meta, uint8_t* frames, long long frame_stride, int32_t* __restrict__ status) {
  const int lane = threadIdx.x;
  const uint32_t rs = 1u + (uint32_t)w;
  for (long long f = blockIdx.x; f < nimages; f += gridDim.x) {
    const uint32_t reason = meta[f * kMetaWords + 0], path = meta[f * kMetaWords + 1], good = meta[f * kMetaWords + 3];
    if (lane == 0) status[f] = (int32_t)(reason | path << 16);
    if (!good) continue;
    const uint8_t* __restrict__ src = filt + f * filt_stride;
    uint8_t* out = frames + f * frame_stride;
    for (int r0 = 0; r0 < h; r0 += 64) {
      const int row = r0 + lane;
      const bool active = row < h;
      const uint8_t* __restrict__ line = src + (size_t)(active ? row : 0) * rs;
      uint8_t* mine = out + (size_t)(active ? row : 0) * w;
      const uint8_t* above = out + (size_t)(r0 > 0 ? r0 - 1 : 0) * w;  // the previous band's last row: lane 0's "up"
      const int type = active ? line[0] : 0;
      int last = 0, up_before = 0;
      int x_next = (active && lane == 0) ? line[1] : 0;  // step 0: lane 0 at column 0
      for (int t = 0; t < w + 63; t++) {
        const int c = t - lane;
        const bool valid = active && c >= 0 && c < w;
        const int x = x_next;
        const int cn = c + 1;  // the next step's byte, asked for before this step's arithmetic
        x_next = (active && cn >= 0 && cn < w) ? line[1 + cn] : 0;
        int up = from_lane_above(last);
        if (lane == 0) up = (r0 > 0 && c < w) ? above[c] : 0;
        const int a = c > 0 ? last : 0, cc = c > 0 ? up_before : 0;
        const int v = pngd::unfilter_px(type, x, a, up, cc);
        if (valid) mine[c] = (uint8_t)v;
        last = valid ? v : 0;
        up_before = up;
      }
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");  // the band's last row is in memory before the next band's lane 0 reads it
    }
  }
}

// ---------------------------------------------------------------------------------------------------- host side

int grid_for(long long items) { return (int)(items < 1 ? 1 : items > kMaxGrid ? kMaxGrid : items); }

long long filt_stride_of(int w, int h) { return (((1ll + w) * h + 15) / 16) * 16; }

// What tells the two libraries' host sides apart, beside the launch sequence of a call (below)
struct Params {
  const char* prefix;  // of the functions' names in messages: "mdci", "mdcx"
  int extra_bytes;     // scratch per filtered byte beyond the byte itself: 0, or 4 for libmdc_pngdx.so's source indices
  int stages;          // timed stages of a call: *_kernel_ms fills that many
};
constexpr int kMaxStages = 5;

// The fields both decoders have.  struct mdci_decoder and struct mdcx_decoder derive from it; each adds extra(): where it keeps its own
// scratch array of Params::extra_bytes per filtered byte, or null when it has none.
struct Decoder {
  int device = -1, w = 0, h = 0, max_images = 0;
  long long F = 0, filt_stride = 0;
  uint8_t* d_filt = nullptr;
  uint32_t* d_meta = nullptr;
  // decode_host: made at its first call
  hipStream_t stream = nullptr;
  uint8_t* h_stage = nullptr;  // pinned: n sizes (padded to 16 bytes), then n slots
  uint8_t* d_stage = nullptr;
  size_t stage_bytes = 0;
  uint8_t* d_out = nullptr;
  int32_t* d_status = nullptr;
  // profile: events around the stages of a call, Params::stages + 1 of them
  bool profile = false, timed = false;
  hipEvent_t ev[kMaxStages + 1] = {};
};

// One decode_device call, as its launch sequence sees it
struct Call {
  Input in;
  long long N;
  uint8_t* frames;
  long long frame_stride;
  int32_t* status;
  hipStream_t s;
};

int64_t scratch_bytes(const Params& p, int w, int h, int max_images) {
  if (w < 1 || h < 1 || max_images < 1) return -1;
  if ((1ll + w) > (1ll << 28) / h) return -1;
  const long long per_image = (1 + p.extra_bytes) * filt_stride_of(w, h) + 4 * kMetaWords;
  if (per_image > (1ll << 40) / max_images) return -1;
  return per_image * max_images;
}

template <class D>
void destroy(D* d) {
  if (!d) return;
  {
    DeviceGuard dg(d->device);
    if (d->stream) (void)hipStreamSynchronize(d->stream);
    (void)hipFree(d->d_filt);
    if (d->extra()) (void)hipFree(*d->extra());
    (void)hipFree(d->d_meta);
    (void)hipFree(d->d_stage);
    (void)hipFree(d->d_out);
    (void)hipFree(d->d_status);
    if (d->h_stage) (void)hipHostFree(d->h_stage);
    if (d->stream) (void)hipStreamDestroy(d->stream);
    for (hipEvent_t e : d->ev)
      if (e) (void)hipEventDestroy(e);
  }
  delete d;
}

template <class D>
int create(const char* who, const Params& p, int device, int w, int h, int max_images, D** out) {
  if (!out) return fail(kErrArg, "%s: out is null", who);
  *out = nullptr;
  if (max_images < 1) return fail(kErrArg, "%s: max_images %d is below 1", who, max_images);
  if (w < 1 || h < 1) return fail(kErrSize, "%s: %d x %d: width and height start at 1", who, w, h);
  if ((1ll + w) > (1ll << 28) / h) return fail(kErrSize, "%s: a %d x %d image has more than 2^28 filtered bytes", who, w, h);
  if (scratch_bytes(p, w, h, max_images) < 0) return fail(kErrSize, "%s: %d images of %d x %d: the scratch passes 2^40 bytes", who, max_images, w, h);
  if (int rc = resolve_device(who, &device)) return rc;
  DeviceGuard dg(device);
  D* d = new (std::nothrow) D;
  if (!d) return fail(kErrNoMem, "%s: out of host memory", who);
  d->device = device, d->w = w, d->h = h, d->max_images = max_images;
  d->F = (1ll + w) * h, d->filt_stride = filt_stride_of(w, h);
  const size_t filt_bytes = (size_t)d->filt_stride * (size_t)max_images;
  if (hipMalloc((void**)&d->d_filt, filt_bytes) != hipSuccess || (d->extra() && hipMalloc(d->extra(), filt_bytes * (size_t)p.extra_bytes) != hipSuccess) ||
      hipMalloc((void**)&d->d_meta, (size_t)max_images * kMetaWords * 4) != hipSuccess) {
    (void)hipGetLastError();
    destroy(d);
    return fail(kErrNoMem, "%s: could not allocate the scratch arrays of %d images of %d x %d", who, max_images, w, h);
  }
  *out = d;
  return kOk;
}

// launch(d, call, mark): the library's kernels of one call in order, with mark() before the first stage and after every stage
template <class D, class Launch>
int decode_device(const Params& p, D* d, const uint8_t* d_slots, int64_t slot_bytes, const int32_t* d_sizes, int skip_head, int skip_tail, int n, uint8_t* d_frames,
                  int64_t frame_stride, int32_t* d_status, void* stream, Launch launch) {
  if (!d) return fail(kErrArg, "%s_decode_device: decoder is null", p.prefix);
  if (n < 0 || n > d->max_images) return fail(kErrArg, "%s_decode_device: %d frames, the decoder was made for 0..%d", p.prefix, n, d->max_images);
  if (n == 0) return kOk;
  if (!d_slots || !d_sizes || !d_frames || !d_status) return fail(kErrArg, "%s_decode_device: null device pointer", p.prefix);
  if ((uintptr_t)d_sizes % 4 || (uintptr_t)d_status % 4) return fail(kErrArg, "%s_decode_device: d_sizes and d_status are arrays of int32_t: 4-byte aligned", p.prefix);
  if (slot_bytes < 0) return fail(kErrArg, "%s_decode_device: slot_bytes %lld is negative", p.prefix, (long long)slot_bytes);
  if (skip_head < 0 || skip_tail < 0) return fail(kErrArg, "%s_decode_device: skip_head %d, skip_tail %d: neither may be negative", p.prefix, skip_head, skip_tail);
  if (frame_stride < (int64_t)d->w * d->h) return fail(kErrArg, "%s_decode_device: frame_stride %lld is below %d x %d", p.prefix, (long long)frame_stride, d->w, d->h);
  DeviceGuard dg(d->device);
  const Call c = {{d_slots, (long long)slot_bytes, d_sizes, skip_head, skip_tail}, n, d_frames, (long long)frame_stride, d_status, (hipStream_t)stream};
  const bool prof = d->profile;
  int stage = 0;
  launch(d, c, [&]() {
    if (prof) (void)hipEventRecord(d->ev[stage++], c.s);
  });
  if (prof) d->timed = true;
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(kErrHip, "%s_decode_device: launch failed: %s", p.prefix, hipGetErrorString(err));
  return kOk;
}

int profile(const Params& p, Decoder* d, int on) {
  if (!d) return fail(kErrArg, "%s_profile: decoder is null", p.prefix);
  DeviceGuard dg(d->device);
  for (int k = 0; k <= p.stages; k++)
    if (on && !d->ev[k] && hipEventCreate(&d->ev[k]) != hipSuccess) {
      d->ev[k] = nullptr;
      d->profile = false;
      return fail(kErrHip, "%s_profile: no event: %s", p.prefix, hipGetErrorString(hipGetLastError()));
    }
  d->profile = on != 0;
  d->timed = false;
  return kOk;
}

int kernel_ms(const Params& p, Decoder* d, float* ms) {
  if (!d || !ms) return fail(kErrArg, "%s_kernel_ms: null argument", p.prefix);
  if (!d->timed) return fail(kErrArg, "%s_kernel_ms: no call has been timed (%s_profile, then %s_decode_device)", p.prefix, p.prefix, p.prefix);
  DeviceGuard dg(d->device);
  if (hipEventSynchronize(d->ev[p.stages]) != hipSuccess) return fail(kErrHip, "%s_kernel_ms: %s", p.prefix, hipGetErrorString(hipGetLastError()));
  for (int k = 0; k < p.stages; k++)
    if (hipEventElapsedTime(&ms[k], d->ev[k], d->ev[k + 1]) != hipSuccess) return fail(kErrHip, "%s_kernel_ms: %s", p.prefix, hipGetErrorString(hipGetLastError()));
  return kOk;
}

void* own_stream(Decoder* d) {
  if (!d) return nullptr;
  if (!d->stream) {
    DeviceGuard dg(d->device);
    if (hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking) != hipSuccess) d->stream = nullptr;
  }
  return d->stream;
}

int synchronize(const Params& p, Decoder* d) {
  if (!d) return fail(kErrArg, "%s_synchronize: decoder is null", p.prefix);
  if (!d->stream) return kOk;
  DeviceGuard dg(d->device);
  const hipError_t err = hipStreamSynchronize(d->stream);
  if (err != hipSuccess) return fail(kErrHip, "%s_synchronize: %s", p.prefix, hipGetErrorString(err));
  return kOk;
}

template <class D, class Launch>
int decode_host(const Params& p, D* d, const void* const* streams, const int64_t* bytes, int n, int* status, const uint8_t** d_frames, Launch launch) {
  if (!d) return fail(kErrArg, "%s_decode_host: decoder is null", p.prefix);
  if (n < 0 || n > d->max_images) return fail(kErrArg, "%s_decode_host: %d frames, the decoder was made for 0..%d", p.prefix, n, d->max_images);
  if (!d_frames) return fail(kErrArg, "%s_decode_host: d_frames is null", p.prefix);
  *d_frames = d->d_out;
  if (n == 0) return kOk;
  if (!streams || !bytes || !status) return fail(kErrArg, "%s_decode_host: null pointer", p.prefix);
  int64_t longest = 0;
  for (int f = 0; f < n; f++) {
    if (bytes[f] < 0 || bytes[f] > INT32_MAX || (bytes[f] > 0 && !streams[f])) return fail(kErrArg, "%s_decode_host: stream %d: %lld bytes at %p", p.prefix, f, (long long)bytes[f], streams[f]);
    if (bytes[f] > longest) longest = bytes[f];
  }
  DeviceGuard dg(d->device);
  const size_t head = ((size_t)n * 4 + 15) / 16 * 16, slot = ((size_t)longest + 15) / 16 * 16, need = head + slot * (size_t)n;
  if (!own_stream(d)) return fail(kErrHip, "%s_decode_host: no stream: %s", p.prefix, hipGetErrorString(hipGetLastError()));
  if (!d->d_out && (hipMalloc((void**)&d->d_out, (size_t)d->max_images * d->w * d->h) != hipSuccess ||
                    hipMalloc((void**)&d->d_status, (size_t)d->max_images * 4) != hipSuccess)) {
    (void)hipGetLastError();
    (void)hipFree(d->d_out);
    d->d_out = nullptr;
    return fail(kErrNoMem, "%s_decode_host: could not allocate %d frames of %d x %d", p.prefix, d->max_images, d->w, d->h);
  }
  if (need > d->stage_bytes) {
    (void)hipStreamSynchronize(d->stream);
    if (d->h_stage) (void)hipHostFree(d->h_stage);
    (void)hipFree(d->d_stage);
    d->h_stage = d->d_stage = nullptr;
    d->stage_bytes = 0;
    const size_t want = need + need / 4;  // some room: the next batch's longest stream is rarely the same
    if (hipHostMalloc((void**)&d->h_stage, want, hipHostMallocDefault) != hipSuccess || hipMalloc((void**)&d->d_stage, want) != hipSuccess) {
      (void)hipGetLastError();
      if (d->h_stage) (void)hipHostFree(d->h_stage);
      d->h_stage = nullptr;
      return fail(kErrNoMem, "%s_decode_host: could not allocate %zu bytes of staging", p.prefix, want);
    }
    d->stage_bytes = want;
  }
  int32_t* sizes = (int32_t*)d->h_stage;
  for (int f = 0; f < n; f++) {
    sizes[f] = (int32_t)bytes[f];
    if (bytes[f]) memcpy(d->h_stage + head + slot * (size_t)f, streams[f], (size_t)bytes[f]);
  }
  *d_frames = d->d_out;
  if (hipMemcpyAsync(d->d_stage, d->h_stage, need, hipMemcpyHostToDevice, d->stream) != hipSuccess)
    return fail(kErrHip, "%s_decode_host: upload failed: %s", p.prefix, hipGetErrorString(hipGetLastError()));
  const int rc = decode_device(p, d, d->d_stage + head, (int64_t)slot, (const int32_t*)d->d_stage, 0, 0, n, d->d_out, (int64_t)d->w * d->h, d->d_status, d->stream, launch);
  if (rc != kOk) return rc;
  if (hipMemcpyAsync(status, d->d_status, (size_t)n * 4, hipMemcpyDeviceToHost, d->stream) != hipSuccess || hipStreamSynchronize(d->stream) != hipSuccess)
    return fail(kErrHip, "%s_decode_host: the decode failed: %s", p.prefix, hipGetErrorString(hipGetLastError()));
  return kOk;
}

}  // namespace
#endif  // MDC_PNG_DECODE_KERNELS_H
