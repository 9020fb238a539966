// libmdc_jopt.so -- the JPEG encoder of libmdc_jenc.so with one optimal Huffman table pair per frame (include/mdc_jopt.h), gfx950.
// A library of its own: it links neither libmdc_jenc.so nor anything of libmdc_hip.so; what it has in common with mdc_jenc.hip
// is one copy of source, csrc/jpeg_encode_core.h.
//
// One call encodes a batch of frames in seven launches and one clear, all integer, all deterministic:
//   jenc_fdct_quant_kernel  (shared) pixels -> quantised coefficients, zigzag order, int16
//   jopt_histogram_kernel   one thread per block walks it and counts its symbols in an LDS histogram of 16 DC and 256 AC bins
//                           per workgroup; the non-zero bins go to the frame's uint32[2][257] with integer atomicAdd
//   jopt_tables_kernel      one workgroup of two waves per frame, wave 0 the DC table and wave 1 the AC table: the rule of
//                           csrc/jpeg_optimal_table.h with its arrays in LDS and the two minimum searches of every merge as wave
//                           reductions -> the frame's (length << 16) | code tables, its two DHT segments and their sizes
//   jopt_count_kernel       one thread per block: the number of bits its code takes with its frame's tables
//   jenc_scan_kernel        (shared) per frame: bit counts -> bit offsets; clears the part of the stream that will be written
//   jopt_pack_kernel        one thread per block: its code words at its bit offset
//   jopt_stuff_kernel       per frame: the 102 fixed header bytes, the frame's DHT segments, SOS, the stuffed stream, EOI, the length
// jenc_gather_kernel (shared) serves mdcjo_fetch and jopt_tables_only_kernel serves mdcjo_optimal_tables_device.
// No kernel keeps a runtime-indexed per-thread array.
#include "../../include/mdc_jopt.h"
#include "jpeg_encode_core.h"
#include "jpeg_optimal_table.h"

namespace {

constexpr Params kParams = {"mdcjo", 418, 27 + 63 * 26};  // include/mdc_jopt.h: the bound's derivation
constexpr int kPrefixBytes = 20 + 5 + 64 + 13;  // SOI, APP0, DQT, SOF0: the same for every frame of an encoder
constexpr int kSosBytes = 10;
constexpr int kDhtMax = 5 + 16 + 256;  // marker, length, class / id, the 16 counts, the symbols
constexpr int kHistWords = 2 * 257;    // per frame: the DC histogram, then the AC histogram

// What jopt_tables_kernel leaves for one frame.  ac and dc as in DeviceTables.
struct FrameTables {
  uint32_t ac[256];
  uint32_t dc[16];
  uint8_t dht[2][kDhtMax + 3];
  int32_t dht_bytes[2];
};

// ---------------------------------------------------------------------------------------------------- symbol counts

// walk_block hands out code words, not symbols.  With tables whose entry for symbol s is the code s of length 0 (DC: 256 + s),
// a word is (symbol << n) | amplitude with count n, and the symbol is word >> count.
struct SymbolCounter {
  uint32_t* hist;  // LDS: [0, 256) AC, [256, 272) DC
  __device__ __forceinline__ void operator()(uint32_t bits, int n) { atomicAdd(&hist[bits >> n], 1u); }
};

// grid (ceil(nblocks / 256), frames of this launch), 256 threads: a workgroup never straddles two frames
__global__ __launch_bounds__(256) void jopt_histogram_kernel(const int16_t* __restrict__ coef, int nblocks, int frame0, uint32_t* __restrict__ hist) {
  __shared__ uint32_t s_ac[256], s_dc[16], s_hist[272];
  const int t = threadIdx.x;
  s_ac[t] = (uint32_t)t;
  s_hist[t] = 0u;
  if (t < 16) s_dc[t] = 256u + (uint32_t)t, s_hist[256 + t] = 0u;
  __syncthreads();
  const long long frame = (long long)frame0 + blockIdx.y;
  const int b = blockIdx.x * 256 + t;
  if (b < nblocks) {
    const long long i = frame * nblocks + b;
    const int prev_dc = b ? coef[(i - 1) * 64] : 0;
    SymbolCounter count{s_hist};
    walk_block(coef + i * 64, prev_dc, s_ac, s_dc, count);
  }
  __syncthreads();
  uint32_t* __restrict__ h = hist + frame * kHistWords;
  const uint32_t v = s_hist[t];
  if (v) atomicAdd(&h[257 + t], v);
  if (t < 16) {
    const uint32_t d = s_hist[256 + t];
    if (d) atomicAdd(&h[t], d);
  }
}

// ---------------------------------------------------------------------------------------------------- tables

// The device's search (csrc/jpeg_optimal_table.h): every lane looks at entries lane, lane + 64, ...; the key orders by count, then
// by descending index, so the least key is libjpeg's winner.
struct WaveSearch {
  __device__ __forceinline__ int operator()(const uint32_t* freq, int exclude) const {
    const int lane = threadIdx.x & 63;
    unsigned long long best = ~0ull;
#pragma unroll
    for (int k = 0; k < 5; k++) {
      const int i = lane + 64 * k;
      if (i < jopt::kSymbols) {
        const uint32_t f = freq[i];
        if (f && f <= jopt::kSearchLimit && i != exclude) {
          const unsigned long long key = ((unsigned long long)f << 9) | (unsigned)(256 - i);
          best = key < best ? key : best;
        }
      }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
      const unsigned long long other = __shfl_xor(best, d, 64);
      best = other < best ? other : best;
    }
    return best == ~0ull ? -1 : 256 - (int)(best & 511u);
  }
};

// The canonical codes (Annex C) of bits / vals into tab[symbol] = (length << 16) | code for symbols below `limit`, by the 64 lanes
// of a wave: position k of vals finds its length by walking the 16 counts.  bits, vals, tab: LDS; tab zeroed by the caller.
__device__ __forceinline__ void assign_codes(const uint8_t* bits, const uint8_t* vals, int nvals, uint32_t* tab, int limit) {
  const int lane = threadIdx.x & 63;
  for (int k = lane; k < nvals; k += 64) {
    uint32_t code = 0, mine = 0;
    int first = 0;
#pragma unroll
    for (int len = 1; len <= 16; len++) {
      const int n = bits[len - 1];
      if (k >= first && k < first + n) mine = ((uint32_t)len << 16) | (code + (uint32_t)(k - first));
      code = (code + (uint32_t)n) << 1;
      first += n;
    }
    const int sym = vals[k];
    if (sym < limit) tab[sym] = mine;
  }
}

// one workgroup of two waves per frame: wave 0 its DC table, wave 1 its AC table
__global__ __launch_bounds__(128) void jopt_tables_kernel(const uint32_t* __restrict__ hist, const DeviceTables* __restrict__ base, FrameTables* __restrict__ out) {
  __shared__ jopt::Work work[2];
  __shared__ uint8_t s_bits[2][16], s_vals[2][256];
  __shared__ uint32_t s_tab[2][256];
  __shared__ int s_status[2];
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  FrameTables* __restrict__ f = out + blockIdx.x;
  for (int k = lane; k < 256; k += 64) s_tab[wave][k] = 0u;
  int nvals, depth;
  const int status = jopt::optimal_table(hist + ((long long)blockIdx.x * 2 + wave) * 257, work[wave], WaveSearch(), s_bits[wave], s_vals[wave], &nvals, &depth);
  if (lane == 0) s_status[wave] = status;
  __syncthreads();
  if (s_status[0] | s_status[1]) {  // a code deeper than 32: the frame is written with the Annex K tables, as the baseline file
    for (int k = t; k < 256; k += 128) f->ac[k] = base->ac[k];
    if (t < 16) f->dc[t] = base->dc[t];
    for (int k = t; k < 33; k += 128) f->dht[0][k] = base->header[kPrefixBytes + k];
    for (int k = t; k < 183; k += 128) f->dht[1][k] = base->header[kPrefixBytes + 33 + k];
    if (t == 0) f->dht_bytes[0] = 33, f->dht_bytes[1] = 183;
    return;
  }
  assign_codes(s_bits[wave], s_vals[wave], nvals, s_tab[wave], wave ? 256 : 16);
  __syncthreads();
  if (wave) {
    for (int k = lane; k < 256; k += 64) f->ac[k] = s_tab[1][k];
  } else if (lane < 16) {
    f->dc[lane] = s_tab[0][lane];
  }
  uint8_t* __restrict__ d = f->dht[wave];
  const int len = 2 + 1 + 16 + nvals;
  if (lane == 0) {
    d[0] = 0xff, d[1] = 0xc4, d[2] = (uint8_t)(len >> 8), d[3] = (uint8_t)len, d[4] = wave ? 0x10 : 0x00;
    f->dht_bytes[wave] = 2 + len;
  }
  if (lane < 16) d[5 + lane] = s_bits[wave][lane];
  for (int k = lane; k < nvals; k += 64) d[21 + k] = s_vals[wave][k];
}

// mdcjo_optimal_tables_device: one wave per histogram
__global__ __launch_bounds__(64) void jopt_tables_only_kernel(const uint32_t* __restrict__ freq, uint8_t* __restrict__ bits, uint8_t* __restrict__ vals,
                                                              int32_t* __restrict__ nvals_out, uint8_t* __restrict__ status_out) {
  __shared__ jopt::Work work;
  __shared__ uint8_t s_bits[16], s_vals[256];
  const int lane = threadIdx.x;
  const long long table = blockIdx.x;
  for (int k = lane; k < 256; k += 64) s_vals[k] = 0;
  int nvals, depth;
  const int status = jopt::optimal_table(freq + table * 257, work, WaveSearch(), s_bits, s_vals, &nvals, &depth);
  if (lane < 16) bits[table * 16 + lane] = s_bits[lane];
  for (int k = lane; k < 256; k += 64) vals[table * 256 + k] = s_vals[k];
  if (lane == 0) nvals_out[table] = nvals, status_out[table] = (uint8_t)status;
}

// ---------------------------------------------------------------------------------------------------- entropy coding with a frame's tables

__device__ __forceinline__ void load_frame_tables(const FrameTables* __restrict__ f, uint32_t* s_ac, uint32_t* s_dc) {
  for (int k = threadIdx.x; k < 256; k += blockDim.x) s_ac[k] = f->ac[k];
  if (threadIdx.x < 16) s_dc[threadIdx.x] = f->dc[threadIdx.x];
  __syncthreads();
}

// grid (ceil(nblocks / 256), frames of this launch), as the histogram's
__global__ __launch_bounds__(256) void jopt_count_kernel(const int16_t* __restrict__ coef, int nblocks, int frame0, const FrameTables* __restrict__ tabs,
                                                         uint32_t* __restrict__ bits) {
  __shared__ uint32_t s_ac[256], s_dc[16];
  const long long frame = (long long)frame0 + blockIdx.y;
  load_frame_tables(tabs + frame, s_ac, s_dc);
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= nblocks) return;
  const long long i = frame * nblocks + b;
  const int prev_dc = b ? coef[(i - 1) * 64] : 0;
  BitCounter count;
  walk_block(coef + i * 64, prev_dc, s_ac, s_dc, count);
  bits[i] = count.bits;
}

__global__ __launch_bounds__(256) void jopt_pack_kernel(const int16_t* __restrict__ coef, int nblocks, int frame0, const FrameTables* __restrict__ tabs,
                                                        const uint32_t* __restrict__ bit_offset, uint32_t* __restrict__ stream, long long stream_words) {
  __shared__ uint32_t s_ac[256], s_dc[16];
  const long long frame = (long long)frame0 + blockIdx.y;
  load_frame_tables(tabs + frame, s_ac, s_dc);
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= nblocks) return;
  const long long i = frame * nblocks + b;
  const int prev_dc = b ? coef[(i - 1) * 64] : 0;
  BitPacker pack(stream + frame * stream_words, bit_offset[i]);
  walk_block(coef + i * 64, prev_dc, s_ac, s_dc, pack);
  pack.finish();
}

// jenc_stuff_kernel of mdc_jenc.hip with a header that is put together per frame: one workgroup of 1024 per frame.  Per
// iteration 16 stream bytes per thread: count the 0xFF among them, scan, lay the stuffed bytes out in LDS, copy them out with
// consecutive threads on consecutive bytes.
__global__ __launch_bounds__(1024) void jopt_stuff_kernel(const uint32_t* __restrict__ stream, long long stream_words, const uint32_t* __restrict__ frame_bits,
                                                          const DeviceTables* __restrict__ tab, const FrameTables* __restrict__ tabs, uint8_t* __restrict__ out,
                                                          long long slot_bytes, int32_t* __restrict__ sizes) {
  __shared__ uint8_t staged[2 * kStuffChunk];
  __shared__ uint32_t scratch[16];
  const int t = threadIdx.x;
  const uint32_t* __restrict__ s = stream + (long long)blockIdx.x * stream_words;
  uint8_t* __restrict__ o = out + (long long)blockIdx.x * slot_bytes;
  const FrameTables* __restrict__ f = tabs + blockIdx.x;
  const uint32_t nbits = frame_bits[blockIdx.x];
  const uint32_t nbytes = (nbits + 7u) >> 3;
  const uint32_t pad = (nbits & 7u) ? (0xffu >> (nbits & 7u)) : 0u;  // 1-bits that fill the last byte
  const int n0 = f->dht_bytes[0], n1 = f->dht_bytes[1];              // 22 .. kDhtMax each
  if (t < kPrefixBytes) o[t] = tab->header[t];
  if (t < n0) o[kPrefixBytes + t] = f->dht[0][t];
  if (t < n1) o[kPrefixBytes + n0 + t] = f->dht[1][t];
  if (t < kSosBytes) o[kPrefixBytes + n0 + n1 + t] = tab->header[kHeaderBytes - kSosBytes + t];
  uint32_t pos = (uint32_t)(kPrefixBytes + n0 + n1 + kSosBytes);
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

}  // namespace

static_assert(MDCJO_OK == kOk && MDCJO_ERR_ARG == kErrArg && MDCJO_ERR_SIZE == kErrSize && MDCJO_ERR_HIP == kErrHip && MDCJO_ERR_NO_DEVICE == kErrNoDevice &&
                  MDCJO_ERR_NOMEM == kErrNoMem,
              "include/mdc_jopt.h and codec_host.h name the same codes");

struct mdcjo_encoder : Encoder {
  uint32_t* d_hist = nullptr;          // per frame uint32[2][257]
  FrameTables* d_frame_tab = nullptr;  // per frame
  bool profile = false, timed = false;
  hipEvent_t ev[MDCJO_KERNELS + 1] = {};
  bool alloc_extra() {
    return hipMalloc((void**)&d_hist, (size_t)max_frames * kHistWords * sizeof(uint32_t)) == hipSuccess &&
           hipMalloc((void**)&d_frame_tab, (size_t)max_frames * sizeof(FrameTables)) == hipSuccess;
  }
  void free_extra() {
    (void)hipFree(d_hist);
    (void)hipFree(d_frame_tab);
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

namespace {

template <typename T>
int encode(const char* who, mdcjo_encoder* e, const T* d_frames, int64_t frame_stride, int nframes, uint8_t* d_out, int64_t slot_bytes, int32_t* d_sizes,
           void* stream) {
  bool go;
  if (int rc = check_encode(who, kParams, e, d_frames, frame_stride, nframes, d_out, slot_bytes, d_sizes, &go); rc || !go) return rc;
  DeviceGuard dg(e->device);
  hipStream_t s = (hipStream_t)stream;
  const int nblocks = e->nblocks, bw = (e->w + 7) / 8;
  const unsigned groups = (unsigned)((nblocks + kGroupBlocks - 1) / kGroupBlocks);
  const unsigned parts = (unsigned)((nblocks + 255) / 256);
  const uint16_t* d_qdiv = reinterpret_cast<const uint16_t*>(reinterpret_cast<const char*>(e->d_tab) + offsetof(DeviceTables, qdiv));
  int stage = 0;
  auto mark = [&]() {
    if (e->profile) (void)hipEventRecord(e->ev[stage++], s);
  };
  // a grid's y dimension is 16-bit: the launches over (parts of a frame, frames) go in chunks of 65,535 frames
  auto chunks = [&](auto&& launch) {
    for (int f0 = 0; f0 < nframes; f0 += 65535) launch(f0, (unsigned)(nframes - f0 < 65535 ? nframes - f0 : 65535));
  };
  mark();
  chunks([&](int f0, unsigned nf) {
    jenc_fdct_quant_kernel<T><<<dim3(groups, nf), 256, 0, s>>>(d_frames, (long long)frame_stride, f0, e->w, e->h, bw, nblocks, d_qdiv, e->d_coef);
  });
  mark();
  if (hipMemsetAsync(e->d_hist, 0, (size_t)nframes * kHistWords * sizeof(uint32_t), s) != hipSuccess)
    return fail(MDCJO_ERR_HIP, "%s: clearing the histograms failed: %s", who, hipGetErrorString(hipGetLastError()));
  chunks([&](int f0, unsigned nf) { jopt_histogram_kernel<<<dim3(parts, nf), 256, 0, s>>>(e->d_coef, nblocks, f0, e->d_hist); });
  mark();
  jopt_tables_kernel<<<(unsigned)nframes, 128, 0, s>>>(e->d_hist, e->d_tab, e->d_frame_tab);
  mark();
  chunks([&](int f0, unsigned nf) { jopt_count_kernel<<<dim3(parts, nf), 256, 0, s>>>(e->d_coef, nblocks, f0, e->d_frame_tab, e->d_bits); });
  mark();
  jenc_scan_kernel<<<(unsigned)nframes, 1024, 0, s>>>(e->d_bits, nblocks, e->d_frame_bits, e->d_stream, e->stream_words);
  mark();
  chunks([&](int f0, unsigned nf) {
    jopt_pack_kernel<<<dim3(parts, nf), 256, 0, s>>>(e->d_coef, nblocks, f0, e->d_frame_tab, e->d_bits, e->d_stream, e->stream_words);
  });
  mark();
  jopt_stuff_kernel<<<(unsigned)nframes, 1024, 0, s>>>(e->d_stream, e->stream_words, e->d_frame_bits, e->d_tab, e->d_frame_tab, d_out, (long long)slot_bytes, d_sizes);
  mark();
  e->timed = e->profile;
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(MDCJO_ERR_HIP, "%s: launch failed: %s", who, hipGetErrorString(err));
  return MDCJO_OK;
}

}  // namespace

extern "C" {

int64_t mdcjo_jpeg_bound(int w, int h) { return jpeg_bound(kParams, w, h); }

const char* mdcjo_last_error(void) { return g_error; }

void mdcjo_destroy(mdcjo_encoder* enc) { destroy(enc); }

int mdcjo_create(int device, int w, int h, int quality, int max_frames, mdcjo_encoder** out) {
  return create("mdcjo_create", kParams, device, w, h, quality, max_frames, out);
}

int mdcjo_encode_f32_device(mdcjo_encoder* enc, const float* d_frames, int64_t frame_stride, int nframes, uint8_t* d_out, int64_t slot_bytes, int32_t* d_sizes,
                            void* stream) {
  return encode("mdcjo_encode_f32_device", enc, d_frames, frame_stride, nframes, d_out, slot_bytes, d_sizes, stream);
}

int mdcjo_encode_u8_device(mdcjo_encoder* enc, const uint8_t* d_frames, int64_t frame_stride, int nframes, uint8_t* d_out, int64_t slot_bytes, int32_t* d_sizes,
                           void* stream) {
  return encode("mdcjo_encode_u8_device", enc, d_frames, frame_stride, nframes, d_out, slot_bytes, d_sizes, stream);
}

int mdcjo_optimal_tables_device(mdcjo_encoder* enc, const uint32_t* d_freq, int ntables, uint8_t* d_bits, uint8_t* d_vals, int32_t* d_nvals, uint8_t* d_status,
                                void* stream) {
  if (!enc) return fail(MDCJO_ERR_ARG, "mdcjo_optimal_tables_device: encoder is null");
  if (ntables < 0) return fail(MDCJO_ERR_ARG, "mdcjo_optimal_tables_device: %d tables", ntables);
  if (ntables == 0) return MDCJO_OK;
  if (!d_freq || !d_bits || !d_vals || !d_nvals || !d_status) return fail(MDCJO_ERR_ARG, "mdcjo_optimal_tables_device: null device pointer");
  DeviceGuard dg(enc->device);
  jopt_tables_only_kernel<<<(unsigned)ntables, 64, 0, (hipStream_t)stream>>>(d_freq, d_bits, d_vals, d_nvals, d_status);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(MDCJO_ERR_HIP, "mdcjo_optimal_tables_device: launch failed: %s", hipGetErrorString(err));
  return MDCJO_OK;
}

int mdcjo_output_device(mdcjo_encoder* enc, uint8_t** d_out, int64_t* slot_bytes, int32_t** d_sizes) { return output_device(kParams, enc, d_out, slot_bytes, d_sizes); }

int64_t mdcjo_fetch(mdcjo_encoder* enc, const uint8_t* d_out, int64_t slot_bytes, const int32_t* d_sizes, int nframes, uint8_t* h_out, int64_t h_capacity,
                    int32_t* h_sizes, void* stream) {
  return fetch(kParams, enc, d_out, slot_bytes, d_sizes, nframes, h_out, h_capacity, h_sizes, stream);
}

int mdcjo_profile(mdcjo_encoder* enc, int on) {
  if (!enc) return fail(MDCJO_ERR_ARG, "mdcjo_profile: encoder is null");
  if (on && !enc->ev[0]) {
    DeviceGuard dg(enc->device);
    for (hipEvent_t& e : enc->ev)
      if (hipEventCreate(&e) != hipSuccess) return fail(MDCJO_ERR_HIP, "mdcjo_profile: hipEventCreate failed");
  }
  enc->profile = on != 0;
  return MDCJO_OK;
}

int mdcjo_kernel_ms(mdcjo_encoder* enc, float* ms) {
  if (!enc || !ms) return fail(MDCJO_ERR_ARG, "mdcjo_kernel_ms: null argument");
  if (!enc->timed) return fail(MDCJO_ERR_ARG, "mdcjo_kernel_ms: no encode call has been timed (mdcjo_profile)");
  DeviceGuard dg(enc->device);
  if (hipEventSynchronize(enc->ev[MDCJO_KERNELS]) != hipSuccess) return fail(MDCJO_ERR_HIP, "mdcjo_kernel_ms: waiting for the call failed");
  for (int k = 0; k < MDCJO_KERNELS; k++)
    if (hipEventElapsedTime(&ms[k], enc->ev[k], enc->ev[k + 1]) != hipSuccess) return fail(MDCJO_ERR_HIP, "mdcjo_kernel_ms: reading an event failed");
  return MDCJO_OK;
}

}  // extern "C"
