// gfx950 (MI355X, CDNA4) kernels for the photometric + FOV undistortion hot path.
//
// What they compute (reference = tum-vision/mono_dataset_code, paths relative to it):
//   unmap   : PhotometricUndistorter::unMapImage      src/PhotometricUndistorter.cpp:193-211
//   remap_* : UndistorterFOV::undistort<T>            src/FOVUndistorter.cpp:341-367
//   fused   : the two composed as DatasetReader::getImage does
//             (src/BenchmarkDatasetReader.h:222-223) without the W*H float intermediate.
//
// Numerics.  The reference is built without FMA (CMakeLists.txt:16-18), so this
// file is compiled with -ffp-contract=off and every expression keeps the
// reference's evaluation order; results are bit-identical, not merely within
// the 1e-4 gate.  The three photometric modes and the overexposure kill are
// folded into ONE 256-entry table chosen by the host:
//   identity : lut[b] = (float)b        gamma : lut[b] = GInv[b]
//   kill     : lut[255] = NaN  (src/PhotometricUndistorter.cpp:208-211 tests the RAW byte)
// and an optional per-pixel factor vinv[i] (gamma+vignette mode, :205).  NaN taps
// propagate through the bilinear sum even under a zero weight, as in the reference.
//
// All kernels are HBM-bound byte/float streaming; there is no contraction, so
// no MFMA.  Frames are batched: a workgroup owns a fixed set of pixels (or one
// output tile) and loops over `fpb` frames, so calibration tables are read once
// per workgroup, not once per frame.
#include "mdc_internal.h"

namespace mdc {

namespace {

constexpr int kLutBytes = 256 * kLutRep * 4;
// Build-time switches: mdc_build_config.h (tuning / debug / diagnosis; diagnosis builds exist only under variants/).
#if MDC_DEBUG_BOUNDS
#define MDC_CHECK(cond)               \
  do {                                \
    if (!(cond)) __builtin_trap();    \
  } while (0)
#else
#define MDC_CHECK(cond) \
  do {                  \
  } while (0)
#endif

typedef float f32x4 __attribute__((ext_vector_type(4)));

// Replicate the 256-entry LUT kLutRep times so that lane l reads replica l%32:
// word address b*32 + (l&31) lies in bank l&31 for every byte value b, i.e. a
// data-dependent table lookup with zero LDS bank conflicts.  Entry e occupies words
// [32e, 32e+32): eight 16-byte stores of (v,v,v,v).
template <int NT>
__device__ __forceinline__ void fill_lut(float* s_lut, const float* __restrict__ lut, int tid) {
  constexpr int N = 256 * (kLutRep / 4);  // 16-byte stores in total
  constexpr int IT = (N + NT - 1) / NT;
  float v[IT];  // every load issued before the first store waits for its value: one memory round trip, not IT
#pragma unroll
  for (int k = 0; k < IT; k++) v[k] = lut[min(tid + k * NT, N - 1) / (kLutRep / 4)];
#pragma unroll
  for (int k = 0; k < IT; k++)
    if (IT * NT == N || tid + k * NT < N) reinterpret_cast<f32x4*>(s_lut)[tid + k * NT] = f32x4{v[k], v[k], v[k], v[k]};
}

// ----------------------------------------------------------------------------
// unMapImage, vector path: npix % 4 == 0, 4-byte aligned bases.
// A workgroup owns 4096 consecutive pixels and loops over its frames.
// ----------------------------------------------------------------------------
// Wave-contiguous dword stores (dword stores reach a higher write rate on this
// memory system than 16-byte ones, tools/hbm_mix.hip).  The raw frame is still read 4 pixels per
// lane (one u32, 256 contiguous bytes per wave-instruction); a wave-private 256-byte LDS scratch
// per access turns "lane t holds pixels 4t..4t+3" into "lane t holds pixels t, t+64, t+128, t+192"
// of the same 256-pixel run, so every store instruction of a wave writes 256 contiguous bytes.
template <bool VIG>
__global__ __launch_bounds__(256) void unmap_xpose_kernel(const uint8_t* __restrict__ in, float* __restrict__ out,
                                                          const float* __restrict__ lut,
                                                          const float* __restrict__ vinv, long long npix, int nframes,
                                                          int fpb) {
  __shared__ __attribute__((aligned(16))) float s_lut[256 * kLutRep];
  __shared__ uint32_t s_raw[4][4][64];  // [wave][access][lane]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  fill_lut<256>(s_lut, lut, tid);
  __syncthreads();
  const float* my_lut = s_lut + (tid & (kLutRep - 1));
  const long long blk = (long long)blockIdx.x * 4096;
  long long run[4];  // first pixel of the 256-pixel run of access k of this wave
  float v[4][4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    run[k] = blk + k * 1024 + wave * 256;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const long long i = run[k] + j * 64 + lane;
      v[k][j] = (VIG && i < npix) ? vinv[i] : 1.f;
    }
  }
  const int f0 = blockIdx.y * fpb;
  const int f1 = min(nframes, f0 + fpb);
  const uint8_t* src = in + (long long)f0 * npix;
  float* dst = out + (long long)f0 * npix;
  typedef const volatile __attribute__((address_space(3))) unsigned char* lds_byte_ptr;
  for (int f = f0; f < f1; f++, src += npix, dst += npix) {
    uint32_t raw[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const long long i = run[k] + 4 * lane;
      raw[k] = i < npix ? __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(src + i)) : 0u;
    }
#pragma unroll
    for (int k = 0; k < 4; k++) s_raw[wave][k][lane] = raw[k];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      lds_byte_ptr b = (lds_byte_ptr)&s_raw[wave][k][0];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        float r = my_lut[(int)b[j * 64 + lane] * kLutRep];
        if (VIG) r = r * v[k][j];
        const long long i = run[k] + j * 64 + lane;
        if (i < npix) __builtin_nontemporal_store(r, dst + i);
      }
    }
  }
}

// unMapImage, scalar path for pixel counts / bases the vector path cannot take.
template <bool VIG>
__global__ __launch_bounds__(256) void unmap_scalar_kernel(const uint8_t* __restrict__ in, float* __restrict__ out,
                                                           const float* __restrict__ lut,
                                                           const float* __restrict__ vinv, long long npix,
                                                           int nframes, int fpb) {
  __shared__ float s_lut[256];
  s_lut[threadIdx.x] = lut[threadIdx.x];
  __syncthreads();
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= npix) return;
  const float v = VIG ? vinv[i] : 1.f;
  const int f0 = blockIdx.y * fpb;
  const int f1 = min(nframes, f0 + fpb);
  for (int f = f0; f < f1; f++) {
    float r = s_lut[in[(long long)f * npix + i]];
    if (VIG) r = r * v;
    out[(long long)f * npix + i] = r;
  }
}

// ----------------------------------------------------------------------------
// Bilinear coefficients of one output pixel, in the reference's operation order
// (src/FOVUndistorter.cpp:352-365).
// ----------------------------------------------------------------------------
struct Bilin {
  int xi, yi;
  float w11, w01, w10, w00;
};
// the four weights from the fractional parts, src/FOVUndistorter.cpp:356,362-365
__device__ __forceinline__ void bilin_weights(Bilin& b, float fx, float fy) {
  const float xxyy = fx * fy;
  b.w11 = xxyy;
  b.w01 = fy - xxyy;
  b.w10 = fx - xxyy;
  b.w00 = ((1.f - fx) - fy) + xxyy;
}
__device__ __forceinline__ Bilin bilin_of(float xx, float yy) {
  Bilin b;
  b.xi = (int)xx;
  b.yi = (int)yy;
  xx -= (float)b.xi;
  yy -= (float)b.yi;
  bilin_weights(b, xx, yy);
  return b;
}
__device__ __forceinline__ float bilin_sum(const Bilin& b, float t00, float t10, float t01, float t11) {
  // xxyy*src[1+W] + (yy-xxyy)*src[W] + (xx-xxyy)*src[1] + (1-xx-yy+xxyy)*src[0], left to right
  return ((b.w11 * t11 + b.w01 * t01) + b.w10 * t10) + b.w00 * t00;
}

// ----------------------------------------------------------------------------
// Generic fused kernel: one output pixel per thread, taps gathered straight from
// global memory.  Legal for every remap and every alignment; used when the tiled
// kernel cannot be planned, and as an in-library cross-check.
// ----------------------------------------------------------------------------
template <bool VIG>
__global__ __launch_bounds__(256) void remap_gather_u8_kernel(const uint8_t* __restrict__ in, float* __restrict__ out,
                                                              RemapArgs a, int nframes, int fpb) {
  __shared__ float s_lut[256];
  s_lut[threadIdx.x] = a.lut[threadIdx.x];
  __syncthreads();
  const int n_out = a.out_w * a.out_h;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= n_out) return;
  const long long n_in = (long long)a.in_w * a.in_h;
  const float xx = a.rx[idx], yy = a.ry[idx];
  const bool black = xx < 0;
  Bilin b = bilin_of(black ? 0.f : xx, black ? 0.f : yy);
  const int s = b.xi + b.yi * a.in_w;
  MDC_CHECK(black || (b.xi >= 0 && b.yi >= 0 && b.xi + 1 < a.in_w && b.yi + 1 < a.in_h));
  float v00 = 1.f, v10 = 1.f, v01 = 1.f, v11 = 1.f;
  if (VIG && !black) {
    v00 = a.vinv[s];
    v10 = a.vinv[s + 1];
    v01 = a.vinv[s + a.in_w];
    v11 = a.vinv[s + a.in_w + 1];
  }
  const int f0 = blockIdx.y * fpb;
  const int f1 = min(nframes, f0 + fpb);
  for (int f = f0; f < f1; f++) {
    float r = 0.f;
    if (!black) {
      const uint8_t* src = in + (long long)f * n_in + s;
      float t00 = s_lut[src[0]], t10 = s_lut[src[1]], t01 = s_lut[src[a.in_w]], t11 = s_lut[src[a.in_w + 1]];
      if (VIG) {
        t00 = t00 * v00;
        t10 = t10 * v10;
        t01 = t01 * v01;
        t11 = t11 * v11;
      }
      r = bilin_sum(b, t00, t10, t01, t11);
    }
    out[(long long)f * n_out + idx] = r;
  }
}

__global__ __launch_bounds__(256) void remap_gather_f32_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                               RemapArgs a, int nframes, int fpb) {
  const int n_out = a.out_w * a.out_h;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= n_out) return;
  const long long n_in = (long long)a.in_w * a.in_h;
  const float xx = a.rx[idx], yy = a.ry[idx];
  const bool black = xx < 0;
  Bilin b = bilin_of(black ? 0.f : xx, black ? 0.f : yy);
  const int s = b.xi + b.yi * a.in_w;
  MDC_CHECK(black || (b.xi >= 0 && b.yi >= 0 && b.xi + 1 < a.in_w && b.yi + 1 < a.in_h));
  const int f0 = blockIdx.y * fpb;
  const int f1 = min(nframes, f0 + fpb);
  for (int f = f0; f < f1; f++) {
    float r = 0.f;
    if (!black) {
      const float* src = in + (long long)f * n_in + s;
      r = bilin_sum(b, src[0], src[1], src[a.in_w], src[a.in_w + 1]);
    }
    out[(long long)f * n_out + idx] = r;
  }
}

// ----------------------------------------------------------------------------
// Tiled fused kernel (the headline path).
//
// Workgroup = one kTileW x (NT/16) output tile, looping over `fpb` frames.
//   once per workgroup : remap -> LDS byte offset + 4 weights per output, the 4
//                        vignette factors of its taps (registers), LUT replicas (LDS);
//   once per frame     : the tile's source window of the raw u8 frame goes HBM -> LDS
//                        directly (buffer_load_dwordx4 ... lds, no VGPR staging, no
//                        ds_write).  The window is the exact footprint of the tile's taps:
//                        per source row the run of aligned 16-byte chunks that covers them
//                        (TilePlan::d_chunks, made on the host); chunk c lands at LDS byte
//                        16*c -- a wave's 64 chunks are 1 KiB contiguous in LDS, as the
//                        LDS-DMA path needs; every byte is fetched by the workgroup once;
//                        then per output 4 byte taps, 4 conflict-free LUT reads,
//                        4 (+4) multiplies, 3 adds, one coalesced store.
// Lane = output column, so the 32 lanes of an LDS access group read ~43
// consecutive source bytes of one row: broadcast within a dword, distinct banks
// across dwords.  Two LDS window buffers: the DMA of frame f+1 is issued before
// frame f is computed; `s_waitcnt vmcnt(#stores)` + one barrier per frame.
//
// Addressing.  Frames and outputs are reached through raw buffer descriptors
// (scalar base, advanced per frame by scalar adds) + a frame-invariant 32-bit
// lane offset: no per-access address arithmetic on the VALU.  The descriptors
// cover exactly one frame, so the hardware range check drops the stores of
// outputs outside the image (their offset is kOutside) and surplus lanes of the
// last staging round read nothing.
//
// XCD placement: the dispatcher deals workgroups round-robin over the 8 XCDs
// (block b -> XCD b%8).  The host hands over a table block -> tile (TilePlan::d_order)
// built so that each XCD owns a contiguous band of tiles; neighbouring tiles share
// source-window halo lines, which then hit in the same L2.  With TilePlan::rotate
// frame group y reads the table shifted by y columns, so the XCDs take the bands
// (and the padding slots of the short ones) in turn.  Speed only -- correctness
// does not depend on placement.
// ----------------------------------------------------------------------------
typedef __attribute__((address_space(3))) void* lds_void_ptr;
// Window buffers are handled as LDS-address-space (32-bit) pointers throughout: a generic pointer would cost a
// 64-bit add, a null compare and a select per tap row to get back to an LDS address.
typedef __attribute__((address_space(3))) unsigned char* lds_u8_ptr;
typedef const volatile __attribute__((address_space(3))) unsigned char* lds_tap_ptr;
typedef const __attribute__((address_space(3))) float* lds_f32_ptr;

constexpr uint32_t kRsrcWord3 = 0x00020000u;  // gfx9 raw buffer: 32-bit data format, no swizzle
#ifdef MDC_EXP_STORE_AUX
constexpr int kStoreAux = MDC_EXP_STORE_AUX;  // gfx94x/gfx950 cache-policy bits: 1 = sc0, 2 = nt, 16 = sc1
#elif MDC_EXP_STORE_NT
constexpr int kStoreAux = 2;  // nt
#else
constexpr int kStoreAux = 0;
#endif
#if MDC_EXP_LOAD_NT
constexpr int kLoadAux = 2;
#else
constexpr int kLoadAux = 0;
#endif

// (a macro, not a function: the descriptor type is only known to the device pass)
#define MDC_FRAME_RSRC(base, bytes) \
  __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(static_cast<const void*>(base)), 0, (int)(bytes), (int)kRsrcWord3)

// Per-thread, frame-invariant state.  The 1024-/960-thread tiles must fit 64 VGPRs (two workgroups per
// CU): their instantiations -- all but the plain two-buffer one (no black outputs, no pyramid, u8 frames), which fits as it is -- are LEAN -- the two tap offsets stay packed in one register (unpacked per
// frame, +2 VALU per output) and only the first row's output offset is kept, rows 1..3 add the row pitch
// (rows below the image then lie beyond the frame's descriptor range and are dropped like kOutside).
constexpr uint32_t kOutsideLean = 0xc0000000u;  // + 3 row pitches still beyond any frame the plan accepts
// RPT = outputs (vertically consecutive rows of one column) per thread: 4, or 8 for the wide tiles (320 x 16, 640 x 8:
// 640 threads), which are LEAN as well.
template <int RPT>
struct TileThread {
  Bilin bl[RPT];             // (!LEAN) weights kept; (LEAN) only the fractional parts are, the weights are redone per frame
  float fx[RPT], fy[RPT];    //  -- the same four IEEE operations either way, so the same bits
  int off0[RPT], off1[RPT];  // LDS byte offsets of taps (xi,yi) and (xi,yi+1) inside the window  (!LEAN)
  uint32_t tap[RPT];         // off0 | off1 << 16                                                  (LEAN)
  uint32_t obyte[RPT];       // byte offset of the output inside a frame, kOutside if not in the image (LEAN: [0] only)
  bool black[RPT];
  float v00[RPT], v10[RPT], v01[RPT], v11[RPT];
  uint32_t p1byte, p2byte;  // fused pyramid: byte offsets of this lane's level-1 / level-2 outputs (p2byte: kOutside if none).
                            // Level 1: even lanes store the box of rows 0-1, odd lanes the box of rows 2-3 of their LEFT neighbour's column pair -- one full store
};

template <bool VIG, bool BLACK, bool F32, bool LEAN, int B, int RPT>
__device__ __forceinline__ void tile_compute(const TileThread<RPT>& t, lds_u8_ptr w, lds_f32_ptr my_lut, float* dst,
                                             uint32_t out_bytes, uint32_t row_bytes, float (&res)[RPT], int win_bytes) {
#if __HIP_DEVICE_COMPILE__  // buffer / LDS-DMA builtins exist in the device pass only
  const auto ro = MDC_FRAME_RSRC(dst, out_bytes);
  // Outputs are processed B at a time: all their byte taps are issued, then all their LUT reads, then the
  // arithmetic -- two LDS latencies per batch instead of two per output.  (B = 2 where registers are short:
  // the 64-VGPR LEAN tiles and the fused pyramid.)
#pragma unroll
  for (int j0 = 0; j0 < RPT; j0 += B) {
    int off0[B], off1[B];
    Bilin bw[B];
#pragma unroll
    for (int u = 0; u < B; u++) {
      const int j = j0 + u;
      // LEAN: the derived values must be REDONE every frame (that is the point: fewer live registers), but they are
      // loop-invariant and the optimiser would hoist them right back -- the empty asm makes the sources opaque.
      uint32_t tap = t.tap[j];
      float fx = t.fx[j], fy = t.fy[j];
      if (LEAN) asm volatile("" : "+v"(tap), "+v"(fx), "+v"(fy));
      off0[u] = LEAN ? (int)(tap & 0xffffu) : t.off0[j];
      off1[u] = LEAN ? (int)(tap >> 16) : t.off1[j];
      bw[u] = t.bl[j];
      if (LEAN) bilin_weights(bw[u], fx, fy);
      // both tap pairs lie inside the window buffer (the host plan's promise)
      MDC_CHECK(off0[u] >= 0 && off1[u] >= 0 && off0[u] + (F32 ? 8 : 2) <= win_bytes && off1[u] + (F32 ? 8 : 2) <= win_bytes);
      MDC_CHECK(!F32 || ((off0[u] | off1[u]) & 3) == 0);
    }
    float tv[B][4];  // t00 t10 t01 t11
    if (F32) {  // float frames (undistort<float>): the taps are the staged floats themselves
#pragma unroll
      for (int u = 0; u < B; u++) {
        lds_f32_ptr p = reinterpret_cast<lds_f32_ptr>(w + off0[u]);
        lds_f32_ptr q = reinterpret_cast<lds_f32_ptr>(w + off1[u]);
        tv[u][0] = p[0];
        tv[u][1] = p[1];
        tv[u][2] = q[0];
        tv[u][3] = q[1];
      }
    } else {
      // explicit byte loads: two adjacent byte loads fused into one ds_read_u16 at an odd
      // address are replayed by the LDS (SQ_LDS_UNALIGNED_STALL), hence volatile
      int b[B][4];
#pragma unroll
      for (int u = 0; u < B; u++) {
        lds_tap_ptr p = (lds_tap_ptr)(w + off0[u]);
        lds_tap_ptr q = (lds_tap_ptr)(w + off1[u]);
        b[u][0] = p[0];
        b[u][1] = p[1];
        b[u][2] = q[0];
        b[u][3] = q[1];
      }
#if MDC_EXP_FAKE_COMPUTE == 2
#pragma unroll
      for (int u = 0; u < B; u++)
        for (int k = 0; k < 4; k++) tv[u][k] = bw[u].w00;
#else
#pragma unroll
      for (int u = 0; u < B; u++)
#pragma unroll
        for (int k = 0; k < 4; k++) tv[u][k] = my_lut[b[u][k] * kLutRep];
#endif
    }
#pragma unroll
    for (int u = 0; u < B; u++) {
      const int j = j0 + u;
      float t00 = tv[u][0], t10 = tv[u][1], t01 = tv[u][2], t11 = tv[u][3];
      if (VIG && !F32) {
        t00 = t00 * t.v00[j];
        t10 = t10 * t.v10[j];
        t01 = t01 * t.v01[j];
        t11 = t11 * t.v11[j];
      }
      float r = bilin_sum(bw[u], t00, t10, t01, t11);
      if (BLACK && t.black[j]) r = 0.f;
      res[j] = r;
#if MDC_EXP_SKIP_STORE
      if (r != -1.2345e30f) continue;
#endif
      const uint32_t obyte = LEAN ? t.obyte[0] + (uint32_t)j * row_bytes : t.obyte[j];
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(r), ro, obyte, 0, kStoreAux);
    }
  }
#endif
}

// ----------------------------------------------------------------------------
// Fused box pyramid (BASELINE.json config 5; not in the reference, definition in DESIGN.md):
// level l+1 pixel = 0.25f*(((a+b)+c)+d), a=(2x,2y) b=(2x+1,2y) c=(2x,2y+1) d=(2x+1,2y+1).
// A thread holds 4 vertically consecutive outputs of one column, the right neighbour column sits
// in the next lane: levels 1 and 2 come out of registers with two DPP quad permutes; level 3
// pairs row groups of different waves and goes through a 16-float LDS row per wave, one frame
// later (the per-frame barrier doubles as its hand-over).
// ----------------------------------------------------------------------------
struct PyramidOut {
  float* l1;  // nframes * (w/2)*(h/2), or nullptr
  float* l2;  // nframes * (w/4)*(h/4), or nullptr
  float* l3;  // nframes * (w/8)*(h/8), or nullptr
#if MDC_EXP_STRIP_FAKE_GRAD
  float* gI;  // diagnosis: level-0 (I, dx, dy) triples / absSquaredGrad written by the strip kernel with the traffic, the sample count
  float* gA;  // and the store shapes a fused level-0 gradient would have -- NOT its values
#endif
};

__device__ __forceinline__ float box4(float a, float b, float c, float d) { return 0.25f * (((a + b) + c) + d); }
template <int CTRL>
__device__ __forceinline__ float dpp_quad(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}

// levels 1 and 2 of frame `f` from this thread's four outputs; this wave's level-2 row -> s_row
__device__ __forceinline__ void pyramid_levels12(const TileThread<4>& t, const float (&r)[4], const PyramidOut& py,
                                                 long long f, uint32_t l1_bytes, uint32_t l2_bytes, float* s_row,
                                                 int lane) {
#if __HIP_DEVICE_COMPILE__
  float v1[2];
#pragma unroll
  for (int p = 0; p < 2; p++) {
    const float b = dpp_quad<0xF5>(r[2 * p]);      // quad_perm [1,1,3,3]: even lanes read their right neighbour
    const float d = dpp_quad<0xF5>(r[2 * p + 1]);
    v1[p] = box4(r[2 * p], b, r[2 * p + 1], d);
  }
  if (py.l1) {
    const auto r1 = MDC_FRAME_RSRC(py.l1 + f * (l1_bytes / 4), l1_bytes);
    // both level-1 rows of the wave in ONE 64-lane store (quad_perm [0,0,2,2]: odd lanes take their left neighbour's
    // second box): a vector-memory instruction less per frame than two half-empty stores
    const float left2 = dpp_quad<0xA0>(v1[1]);  // executed by ALL lanes: a DPP read of a lane that is masked off returns nothing useful
    const float m = (lane & 1) ? left2 : v1[0];
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(m), r1, t.p1byte, 0, kStoreAux);
  }
  const float b2 = dpp_quad<0xAA>(v1[0]);  // quad_perm [2,2,2,2]: lane 4k reads lane 4k+2
  const float d2 = dpp_quad<0xAA>(v1[1]);
  const float v2 = box4(v1[0], b2, v1[1], d2);
  if (py.l2) {
    const auto r2 = MDC_FRAME_RSRC(py.l2 + f * (l2_bytes / 4), l2_bytes);
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v2), r2, t.p2byte, 0, kStoreAux);
  }
  if ((lane & 3) == 0) s_row[lane >> 2] = v2;
#endif
}

// level 3 of frame `f` of this tile from the level-2 rows the waves left in LDS
// (RG = row groups of 4 output rows, each leaving one level-2 row of TW/4 floats)
template <int RG, int TW>
__device__ __forceinline__ void pyramid_level3(const PyramidOut& py, long long f, uint32_t l3_bytes, const float* s_rows,
                                               uint32_t p3byte, int u3) {
#if __HIP_DEVICE_COMPILE__
  constexpr int L2W = TW / 4, L3W = TW / 8;
  if (py.l3 && u3 >= 0 && u3 < L3W * (RG / 2)) {  // u3 = lane of the last wave (negative in the other waves)
    const int m = u3 / L3W, k = u3 % L3W;
    const float* top = s_rows + (2 * m) * L2W + 2 * k;
    const float* bot = s_rows + (2 * m + 1) * L2W + 2 * k;
    const float v3 = box4(top[0], top[1], bot[0], bot[1]);
    const auto r3 = MDC_FRAME_RSRC(py.l3 + f * (l3_bytes / 4), l3_bytes);
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v3), r3, p3byte, 0, kStoreAux);
  }
#endif
}

// One staging pass: the window of the frame at `src` -> LDS buffer `win`.  R = rounds of NT chunks, of which this wave issues
// the first `rw` (the rounds in which its first lane has a chunk: the chunk list is dense).  The condition is WAVE-uniform -- a
// scalar branch, no exec-mask juggling around every load: the lanes of a wave's last, partial round that lie past the window
// carry goff == kOutside, which the descriptor's range check answers with zeros (no memory traffic), written behind the window's
// last chunk -- still inside the buffer, whose size is a whole number of 64-chunk wave rounds (plan_source: win_bytes).
template <int R, int NT>
__device__ __forceinline__ void stage_window(const uint8_t* src, uint32_t in_bytes, lds_u8_ptr win,
                                             const uint32_t (&goff)[R], int wave, int rw) {
#if __HIP_DEVICE_COMPILE__
  const auto ri = MDC_FRAME_RSRC(src, in_bytes);
#pragma unroll
  for (int k = 0; k < R; k++)
    if (k < rw) {
      MDC_CHECK(goff[k] == kOutside || (goff[k] + 16u <= in_bytes && (goff[k] & 15u) == 0));
      __builtin_amdgcn_raw_ptr_buffer_load_lds(ri, (lds_void_ptr)(win + (k * NT + wave * 64) * 16), 16, goff[k], 0,
                                               0, kLoadAux);
    }
  // The hand-counted vmcnt allowances below rely on the issue order "DMA group, then the frame's
  // stores": nothing may be scheduled across this point (the DMA and the stores use different
  // descriptors, so the compiler sees no dependence of its own).
  __builtin_amdgcn_sched_barrier(0);
#endif
}

// s_waitcnt vmcnt(N) ; s_barrier -- hand-placed: the compiler's own barrier (a workgroup fence)
// would wait for EVERY outstanding LDS-DMA, i.e. also for the frames staged ahead.  vmcnt retires
// in issue order on gfx9, loads and stores alike (the compiler's own counting relies on that).
// lgkmcnt(0) rides along: the fused pyramid hands its level-2 row to other waves through LDS
// (ds_write just before this point), and a ds_write must have COMPLETED before the barrier for the
// readers behind it to see it; every other LDS operation of the frame has been consumed by then, so
// the extra wait is free.
template <int N>
__device__ __forceinline__ void wait_vm_barrier() {
  static_assert(N >= 0 && N < 64, "vmcnt is 6 bits");
  asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(N) : "memory");
}
// A = allowance of the per-frame wait for a wave that issues `rw` DMA instructions per frame with D frames staged
// ahead.  Iteration i issues DMA(i+D), then the 4 stores of frame i (the fused pyramid: more).  At the end of iteration
// f the wave needs DMA(f+1), issued in iteration f+1-D; everything issued after it may stay in flight:
// the stores of that iteration (4) and the D-1 later iterations' DMA groups and stores  ->  (D-1)*(rw+4) + 4.
// (Round 1 allowed only (D-1)*rw + 4: with D >= 2 every frame then also waited for the ACKNOWLEDGEMENT of the
// previous frame's stores, which is what deeper staging is meant to avoid.)  More stores than 4 per frame (pyramid)
// only make the wait more conservative.  The count relies on the chunk list being dense: a wave's round k has a
// chunk for its first lane iff wave*64 + k*NT < nch.
#if MDC_EXP_TIMING
__device__ __forceinline__ unsigned long long exp_now() {
  unsigned long long t;
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  return t;
}
#endif
// S = stores a wave issues per frame after its DMA group: 4 (the outputs), or 6 in the fused pyramid when levels 1 and 2
// are both written (1 + 1 more; level 3's single store -- issued by a few threads at the top of the NEXT iteration, before
// that iteration's DMA group -- is left out of the count, which keeps the allowance on the safe side).  Counting the
// pyramid's stores as 4 made every frame wait for the acknowledgement of half of the previous frame's stores.
#if MDC_EXP_TIMING
template <int N>
__device__ __forceinline__ void wait_vm_only() {
  asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(N) : "memory");
}
template <int D, int R, int S = 4>
__device__ __forceinline__ void frame_wait_only(int rw) {
  if (R >= 4 && rw >= 4) wait_vm_only<(D - 1) * (4 + S) + S>();
  else if (R >= 3 && rw == 3) wait_vm_only<(D - 1) * (3 + S) + S>();
  else if (R >= 2 && rw == 2) wait_vm_only<(D - 1) * (2 + S) + S>();
  else if (rw == 1) wait_vm_only<(D - 1) * (1 + S) + S>();
  else wait_vm_only<S>();
}
#endif
template <int D, int R, int S = 4>
__device__ __forceinline__ void frame_barrier(int rw) {
  if constexpr (D == 1) {  // two buffers: the allowance does not depend on rw -- ONE barrier, not a branch maze around five copies of it
    (void)rw;
    wait_vm_barrier<S>();
    return;
  }
  if (R >= 4 && rw >= 4) wait_vm_barrier<(D - 1) * (4 + S) + S>();
  else if (R >= 3 && rw == 3) wait_vm_barrier<(D - 1) * (3 + S) + S>();
  else if (R >= 2 && rw == 2) wait_vm_barrier<(D - 1) * (2 + S) + S>();
  else if (rw == 1) wait_vm_barrier<(D - 1) * (1 + S) + S>();
  else wait_vm_barrier<S>();
}

// Frames [0, nframes) of one tile.  NBUF window buffers, D = NBUF-1 frames staged ahead: the DMA
// of frame f+D is issued before frame f is computed; one barrier per frame.
template <bool VIG, bool BLACK, bool PYR, bool F32, int R, int TW, int NT, int NBUF, int RPT>
__device__ __forceinline__ void tile_frames(const TileThread<RPT>& t, const uint8_t* __restrict__ src,
                                            float* __restrict__ dst, uint32_t in_bytes, uint32_t out_bytes,
                                            int nframes, int nch, const uint32_t (&goff_all)[F32 ? kTileMaxChunksF32 : kTileMaxChunks],
                                            lds_u8_ptr s_win, int win_bytes, lds_f32_ptr my_lut, int tid,
                                            const PyramidOut& py, long long f_first, int fstep, uint32_t p3byte,
                                            uint32_t row_bytes) {
  // iteration i works on frame f_first + i*fstep; src / dst point at that workgroup's first frame
  constexpr int D = NBUF - 1;
  const long long in_step = (long long)fstep * in_bytes;
  const long long out_step = (long long)fstep * (out_bytes / 4);
  uint32_t goff[R];
#pragma unroll
  for (int k = 0; k < R; k++) goff[k] = goff_all[k];  // kOutside past the window
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int rw = 0;  // DMA instructions this wave issues per frame (rounds in which its first lane has a chunk)
#pragma unroll
  for (int k = 0; k < R; k++) rw += (wave * 64 + k * NT < nch) ? 1 : 0;
  lds_u8_ptr w[NBUF];
#pragma unroll
  for (int i = 0; i < NBUF; i++) w[i] = s_win + i * win_bytes;
  const int last = nframes - 1;
#pragma unroll
  for (int d = 0; d < D; d++) {
#if MDC_EXP_SKIP_LOAD
    stage_window<R, NT>(src, in_bytes, w[d], goff, wave, rw);
#else
    stage_window<R, NT>(src + min(d, last) * in_step, in_bytes, w[d], goff, wave, rw);
#endif
  }
  // frame 0 landed: only the D-1 later DMA groups may still be in flight
  if (R >= 4 && rw >= 4) wait_vm_barrier<(D - 1) * 4>();
  else if (R >= 3 && rw == 3) wait_vm_barrier<(D - 1) * 3>();
  else if (R >= 2 && rw == 2) wait_vm_barrier<(D - 1) * 2>();
  else if (rw == 1) wait_vm_barrier<(D - 1) * 1>();
  else wait_vm_barrier<0>();
  constexpr int G = NT / TW;        // row groups of the tile (RPT output rows each; TW/64 waves side by side)
  constexpr bool LEAN = (NT >= 960 && (NBUF != 2 || BLACK || PYR || F32)) || RPT > 4;
  static_assert(!PYR || RPT == 4, "the fused pyramid pairs the 4 rows of a thread");
  constexpr int L2W = TW / 4;       // level-2 pixels per tile row
  float* s_pyr = (float*)(s_win + NBUF * win_bytes);  // [2][G][L2W] level-2 rows (PYR only)
  const int pyr_slot = (wave / (TW / 64)) * L2W + (wave % (TW / 64)) * 16;  // this wave's 16 floats inside one [G][L2W] set
  const uint32_t l1_bytes = out_bytes / 4, l2_bytes = out_bytes / 16, l3_bytes = out_bytes / 64;
  const bool pyr_all_levels = PYR && py.l1 && py.l2;  // workgroup-uniform: 6 stores per wave and frame
#if MDC_EXP_TIMING
  unsigned long long tp[4] = {0, 0, 0, 0};
  const unsigned long long t_begin = exp_now();
#endif
  // the frame staged in iteration f is frame min(f + D, last): a running pointer (one scalar add per frame) instead of a 64-bit
  // multiply per frame
  const uint8_t* stg = src + (long long)min(D, last) * in_step;
  for (int f = 0; f <= last; f++) {
#if MDC_EXP_TIMING
    const unsigned long long t0 = exp_now();
#endif
    if (PYR && f > 0)
      pyramid_level3<G, TW>(py, f_first + (long long)(f - 1) * fstep, l3_bytes, s_pyr + ((f - 1) & 1) * G * L2W, p3byte, tid - (NT - 64));
#if MDC_EXP_SKIP_LOAD
    stage_window<R, NT>(src, in_bytes, w[D], goff, wave, rw);
#else
    stage_window<R, NT>(stg, in_bytes, w[D], goff, wave, rw);
    if (f + D < last) stg += in_step;
#endif
#if MDC_EXP_TIMING
    const unsigned long long t1 = exp_now();
#endif
    float res[RPT];
#if MDC_EXP_PAD_VALU  // diagnosis (right results): N extra VALU instructions per wave and frame -- what does one instruction of the loop cost?
    {
      int pad_v = tid;
#pragma unroll
      for (int q = 0; q < MDC_EXP_PAD_VALU; q++) asm volatile("v_add_u32 %0, %0, %0" : "+v"(pad_v));
    }
#endif
    tile_compute<VIG, BLACK, F32, LEAN, ((LEAN || PYR) ? 2 : 4), RPT>(t, w[0], my_lut, dst, out_bytes, row_bytes, res, win_bytes);
    if constexpr (PYR)
      pyramid_levels12(t, res, py, f_first + (long long)f * fstep, l1_bytes, l2_bytes, s_pyr + (f & 1) * G * L2W + pyr_slot,
                       tid & 63);
    dst += out_step;
    // frame f+1 landed in every wave's part of w[1]; everyone is done reading w[0]
#if MDC_EXP_TIMING
    const unsigned long long t2 = exp_now();
    if (PYR && pyr_all_levels) frame_wait_only<D, R, 6>(rw);
    else frame_wait_only<D, R, RPT>(rw);
    const unsigned long long t3 = exp_now();
    asm volatile("s_barrier" ::: "memory");
    const unsigned long long t4 = exp_now();
    tp[0] += t1 - t0;  // level 3 of the previous frame + DMA issue
    tp[1] += t2 - t1;  // tap reads, LUT reads, arithmetic, store issue (+ levels 1, 2)
    tp[2] += t3 - t2;  // s_waitcnt vmcnt: the wave's DMA of the next frame landed, older stores retired
    tp[3] += t4 - t3;  // s_barrier: the other waves
#else
    // The allowance below counts what iteration f+1-D issued AFTER its DMA group -- but for f < D-1 the DMA of frame f+1
    // was issued by the PROLOGUE, back to back with the other prologue groups and with no stores behind it, so fewer
    // operations follow it than the formula assumes (D = 2, f = 0: rw + S follow, the formula allows rw + 2 S: the wait
    // could pass with DMA(1) still in flight -- never observed, frame 1 has a whole frame's time to land, but not
    // guaranteed).  Those first D-1 iterations wait for everything but the frame's own 4 stores.
    if (D > 1 && f < D - 1) wait_vm_barrier<RPT>();
    else if (PYR && pyr_all_levels) frame_barrier<D, R, 6>(rw);
    else frame_barrier<D, R, RPT>(rw);
#endif
    lds_u8_ptr x = w[0];
#pragma unroll
    for (int i = 0; i < D; i++) w[i] = w[i + 1];
    w[D] = x;
  }
  if (PYR) pyramid_level3<G, TW>(py, f_first + (long long)last * fstep, l3_bytes, s_pyr + (last & 1) * G * L2W, p3byte, tid - (NT - 64));
#if MDC_EXP_TIMING
  if ((tid & 63) == 0 && (wave == 0 || wave == 5) && blockIdx.x % 41 == 3 && blockIdx.y % 7 == 2)
    printf("TIMING block %d,%d wave %d frames %d cycles/frame: issue %.0f compute+stores %.0f vmwait %.0f barrier %.0f total %.0f\n",
           (int)blockIdx.x, (int)blockIdx.y, wave, nframes, (double)tp[0] / nframes, (double)tp[1] / nframes, (double)tp[2] / nframes,
           (double)tp[3] / nframes, (double)(exp_now() - t_begin) / nframes);
#endif
}

// Occupancy is set by LDS (LUT replicas + two window buffers): 3 workgroups of 512 threads or 2 of
// 960/1024 per CU; the register budget follows from that.
// F32: the frames are floats (UndistorterFOV::undistort<float>, no LUT, no vignette); else raw u8.
template <bool VIG, bool BLACK, bool PYR, bool F32, int TW, int NT, int NBUF>
__global__ __launch_bounds__(NT, (NT >= 960 ? 8 : NT == 640 ? 5 : NT == 512 ? (kLutRep < 32 ? 8 : 6) : 4)) void remap_tiled_kernel(
    const uint8_t* __restrict__ in, float* __restrict__ out, RemapArgs a, TilePlan p, PyramidOut py, int nframes, int fpb,
    int interleave, int taper_full, int taper_r) {
  constexpr int RPT = tile_rpt(TW, 0);  // output rows per thread: 8 for the 320- and 640-wide tiles, else 4 (mdc_internal.h)
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];
  float* s_lut = reinterpret_cast<float*>(smem);
  lds_u8_ptr s_win = (lds_u8_ptr)smem + (F32 ? 0 : kLutBytes);

  // host-made placement table (plan_tiles), rotated by the frame group where asked (xcd_placement.h); -1 = padding slot
  const int tile = p.d_order[xcd_table_entry((int)blockIdx.x, (int)blockIdx.y, p.rotate)];
  if (tile < 0) return;                    // whole workgroup leaves before any barrier
  // Frames of this workgroup: group g of G takes frames [g*fpb, (g+1)*fpb), or -- interleaved --
  // frames g, g+G, g+2G, ...  Interleaved, the groups resident at one time (dispatched in order)
  // walk through ADJACENT frames side by side, so the chip's aggregate traffic sweeps the batch
  // linearly instead of touching a few frames each fpb frames apart.
  // Tapered tail (taper_r > 0): groups 0 .. taper_full-1 hold fpb frames, then taper_r groups of fpb/2, taper_r of fpb/4 and
  // groups of fpb/8 for the rest (taper_range(), host side, is the same arithmetic).  Groups are dispatched in order, so the
  // launch ends on short workgroups: the slots that free up when the last long ones finish do not idle for a long
  // workgroup's time (a 4096-frame launch ran 3 % behind a 50,000-frame one per frame).
  const int fstep = interleave ? (int)gridDim.y : 1;
  int f0 = interleave ? (int)blockIdx.y : (int)blockIdx.y * fpb;
  int nf = interleave ? (nframes - f0 + fstep - 1) / fstep : min(nframes, f0 + fpb) - f0;
  if (!interleave && taper_r > 0 && (int)blockIdx.y >= taper_full) {
    const int k = (int)blockIdx.y - taper_full;
    const int lvl = min(k / taper_r, 2);
    const int size = fpb >> (lvl + 1);
    f0 = taper_full * fpb + taper_r * (fpb - (fpb >> lvl)) + (k - lvl * taper_r) * size;
    nf = min(nframes, f0 + size) - f0;
  }
  if (nf <= 0) return;

  const int tid = threadIdx.x;
  const int lane_x = tid % TW;
  const int row0 = (tid / TW) * RPT;
  const int ox = (tile % p.tiles_x) * TW + lane_x;
  constexpr int kTileRows = NT * RPT / TW;  // RPT output rows per thread, TW lanes per row
  constexpr bool LEAN = (NT >= 960 && (NBUF != 2 || BLACK || PYR || F32)) || RPT > 4;
  const int oy0 = (tile / p.tiles_x) * kTileRows + row0;

  // Prologue, ordered for memory-level parallelism: the workgroup's whole start-up is three dependent
  // round trips -- (1) tile id -> (2) chunk list + remap + tap offsets + LUT, all in flight together ->
  // (3) first frames' LDS-DMA + vignette factors -- instead of one round trip per table and output row
  // (a workgroup lives for ~32 frames of ~2 us; a serial prologue was ~7 % of the kernel).
  const int nch = p.d_nch[tile];
  constexpr int RMAX = F32 ? kTileMaxChunksF32 : kTileMaxChunks;
  const uint32_t* chunks = p.d_chunks + (size_t)tile * (RMAX * NT);  // rows are padded with kOutside to RMAX rounds
  uint32_t goff[RMAX];
#pragma unroll
  for (int k = 0; k < RMAX; k++) goff[k] = chunks[tid + k * NT];

  float xx[RPT], yy[RPT];
  uint32_t tp[RPT];
#pragma unroll
  for (int j = 0; j < RPT; j++) {  // unconditional loads (index 0 stands in for outputs outside the image): no branches
    const bool inside = (ox < a.out_w) && (oy0 + j < a.out_h);
    const int oidx = inside ? (oy0 + j) * a.out_w + ox : 0;
    xx[j] = a.rx[oidx];
    yy[j] = a.ry[oidx];
    tp[j] = p.d_taps[oidx];
  }
  if (!F32) fill_lut<NT>(s_lut, a.lut, tid);
  lds_f32_ptr my_lut = (lds_f32_ptr)s_lut + (tid & (kLutRep - 1));

  TileThread<RPT> t;
#pragma unroll
  for (int j = 0; j < RPT; j++) {
    const int oy = oy0 + j;
    const bool inside = (ox < a.out_w) && (oy < a.out_h);
    const int oidx = oy * a.out_w + ox;
    if (LEAN) {  // row j = row 0 + j row pitches; rows below the image fall outside the frame descriptor
      if (j == 0) t.obyte[0] = ox < a.out_w ? (uint32_t)oidx * 4u : kOutsideLean;
    } else {
      t.obyte[j] = inside ? (uint32_t)oidx * 4u : kOutside;
    }
    if (!inside) {
      xx[j] = yy[j] = -1.f;
      tp[j] = 0;
    }
    if (PYR && j == 0)  // level 1: even lanes row oy/2, odd lanes row oy/2 + 1, column ox/2 (whole tiles only, so `inside` holds)
      t.p1byte = (uint32_t)(((oy >> 1) + (lane_x & 1)) * (a.out_w >> 1) + (ox >> 1)) * 4u;
    if (PYR && j == 0) t.p2byte = (lane_x & 3) ? kOutside : (uint32_t)((oy >> 2) * (a.out_w >> 2) + (ox >> 2)) * 4u;
    t.black[j] = xx[j] < 0;  // outputs outside the image count as black: their taps read window byte 0, their store is dropped
    t.bl[j] = bilin_of(t.black[j] ? 0.f : xx[j], t.black[j] ? 0.f : yy[j]);
    t.fx[j] = (t.black[j] ? 0.f : xx[j]) - (float)t.bl[j].xi;
    t.fy[j] = (t.black[j] ? 0.f : yy[j]) - (float)t.bl[j].yi;
    t.tap[j] = tp[j];
    t.off0[j] = (int)(tp[j] & 0xffffu);
    t.off1[j] = (int)(tp[j] >> 16);
  }
#pragma unroll
  for (int j = 0; j < RPT; j++) {
    t.v00[j] = t.v10[j] = t.v01[j] = t.v11[j] = 1.f;
    if (VIG) {  // unconditional gathers: a black output's factors are never used (its result is forced or dropped)
      const int s = t.black[j] ? 0 : t.bl[j].xi + t.bl[j].yi * a.in_w;
      t.v00[j] = a.vinv[s];
      t.v10[j] = a.vinv[s + 1];
      t.v01[j] = a.vinv[s + a.in_w];
      t.v11[j] = a.vinv[s + a.in_w + 1];
    }
  }

  const uint32_t in_bytes = (uint32_t)a.in_w * (uint32_t)a.in_h * (F32 ? 4u : 1u);
  const uint32_t out_bytes = (uint32_t)a.out_w * (uint32_t)a.out_h * 4u;
  const uint8_t* src = in + (long long)f0 * in_bytes;
  float* dst = out + (long long)f0 * (out_bytes / 4);
  // level 3: lane u < (TW/8)*(rows/8) (<= 64 for every tile shape) of the LAST wave owns pixel (u % (TW/8), u / (TW/8)) of the
  // tile's level-3 block.  The last wave, not the first: with small windows (a scale-1 remap stages ~160 chunks) only the
  // first waves have LDS-DMA to issue at the top of a frame, and whoever does level 3 there is the wave everybody else
  // waits for at the frame's barrier (tools/phase_timing.sh: 2600 cycles against 170).
  static_assert(!PYR || (TW / 8) * (kTileRows / 8) <= 64, "level 3 of a tile is one wave's work");
  const int u3 = tid - (NT - 64);
  uint32_t p3byte = kOutside;
  if (PYR && u3 >= 0 && u3 < (TW / 8) * (kTileRows / 8))
    p3byte = (uint32_t)(((tile / p.tiles_x) * (kTileRows / 8) + u3 / (TW / 8)) * (a.out_w >> 3) + (tile % p.tiles_x) * (TW / 8) +
                        u3 % (TW / 8)) * 4u;
  if (nch == 0) {  // every output of the tile is black (or outside): zeros (on every level), no staging
#if __HIP_DEVICE_COMPILE__
    for (int f = 0; f < nf; f++, dst += (long long)fstep * (out_bytes / 4)) {
      const auto ro = MDC_FRAME_RSRC(dst, out_bytes);
#pragma unroll
      for (int j = 0; j < RPT; j++)
        __builtin_amdgcn_raw_buffer_store_b32(0u, ro, LEAN ? t.obyte[0] + (uint32_t)j * (uint32_t)a.out_w * 4u : t.obyte[j], 0, 0);
      if (PYR) {
        const long long fa = (long long)f0 + (long long)f * fstep;
        if (py.l1) {
          const auto r1 = MDC_FRAME_RSRC(py.l1 + fa * (out_bytes / 16), out_bytes / 4);
          __builtin_amdgcn_raw_buffer_store_b32(0u, r1, t.p1byte, 0, 0);
        }
        if (py.l2) __builtin_amdgcn_raw_buffer_store_b32(0u, MDC_FRAME_RSRC(py.l2 + fa * (out_bytes / 64), out_bytes / 16), t.p2byte, 0, 0);
        if (py.l3) __builtin_amdgcn_raw_buffer_store_b32(0u, MDC_FRAME_RSRC(py.l3 + fa * (out_bytes / 256), out_bytes / 64), p3byte, 0, 0);
      }
    }
#endif
    return;
  }
  const int rounds = (nch + NT - 1) / NT;  // workgroup-uniform
  MDC_CHECK(nch * 16 <= p.win_bytes && rounds <= RMAX && (goff[0] == kOutside) == (tid >= nch));  // dense chunk list: the vmcnt allowances count on it
#define MDC_TILE_RUN(R_)                                                                                              \
  tile_frames<VIG, BLACK, PYR, F32, R_, TW, NT, NBUF, RPT>(t, src, dst, in_bytes, out_bytes, nf, nch, goff, s_win, p.win_bytes, \
                                             my_lut, tid, py, (long long)f0, fstep, p3byte, (uint32_t)a.out_w * 4u)
  if (rounds == 1) MDC_TILE_RUN(1);
  else if (rounds == 2) MDC_TILE_RUN(2);
  else if (rounds == 3 || !F32) MDC_TILE_RUN(3);
  else if constexpr (F32) MDC_TILE_RUN(4);  // float windows are 4x the bytes: up to kTileMaxChunksF32 rounds
#undef MDC_TILE_RUN
}

// s_waitcnt vmcnt(N) without a barrier (wave-private windows), and a pointer the compiler cannot prove wave-uniform
// (it is: derived from block indices and loop counters) moved into SGPRs, so that a buffer descriptor built from it needs
// no waterfall loop.
template <int N>
__device__ __forceinline__ void wait_vm() {
  static_assert(N >= 0 && N < 64, "vmcnt is 6 bits");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
template <typename T>
__device__ __forceinline__ T* uniform_ptr(T* p) {
  const unsigned long long v = reinterpret_cast<unsigned long long>(p);
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
  return reinterpret_cast<T*>(((unsigned long long)hi << 32) | lo);
}

// ----------------------------------------------------------------------------
// Wave-private strips: the two-stage idea without any workgroup barrier, 16 outputs per lane.
//
// What round 3's phase timing showed for the scale-1 rectification of config 5 (1280x1024 -> 1280x1024): with the stores
// compiled out both workgroup-tiled kernels still need ~2500 cycles per frame and workgroup for ~140 instructions per
// wave -- a serial chain "DMA landed -> barrier -> LDS round trips -> arithmetic" per FOUR outputs of a thread, with
// three workgroups per CU to hide it.  unMapImage, which runs at the memory system's ceiling, has no barrier and 16
// outputs per thread.  This kernel gives the remap the same shape:
//   * a WAVE owns a 128 x 8 output tile: lane l has columns l and l+64, 8 rows each -> 16 outputs per lane and frame;
//   * its source window (<= 128 chunks, host plan) is staged by the wave itself (LDS-DMA), converted by the wave itself
//     (byte -> lut * vignette, once per source pixel) into its own float window and sampled by the wave itself:
//     no other wave ever touches it -> no s_barrier in the frame loop, only s_waitcnt;
//   * levels 1..3 of the box pyramid come out of the wave's registers: rows are in-lane (8 of them), columns are
//     neighbouring lanes (DPP quad permutes for levels 1 and 2, row_shl:4 for level 3) -- no LDS hand-over;
//   * a workgroup is just W such waves sharing the LUT replicas (W consecutive tiles of a tile row: their windows share
//     128-byte lines, which then meet in the CU's vector L1).
// Same products, same sum order as the direct kernel -> bit-identical (black outputs sample a zero pair with weights
// (0, 0, 0, 1): +0.0f exactly, as the reference's `output = 0`).
// ----------------------------------------------------------------------------
constexpr int kStripLutRep = MDC_EXP_STRIP_LUT_REP;  // LUT replicas of the strip kernel (convert reads only: 0.65 per output)
constexpr int kStripLutBytes = 256 * kStripLutRep * 4;
constexpr int kStripCap = kStripChunkCap;
constexpr int kStripPad = 64;   // bytes behind a float window: the zero pair black outputs sample

template <int NT, int REP>
__device__ __forceinline__ void fill_lut_rep(float* s_lut, const float* __restrict__ lut, int tid) {
  constexpr int N = 256 * (REP / 4);  // 16-byte stores in total; entry e occupies words [REP e, REP e + REP)
  constexpr int IT = (N + NT - 1) / NT;
  float v[IT];
#pragma unroll
  for (int k = 0; k < IT; k++) v[k] = lut[min(tid + k * NT, N - 1) / (REP / 4)];
#pragma unroll
  for (int k = 0; k < IT; k++)
    if (IT * NT == N || tid + k * NT < N) reinterpret_cast<f32x4*>(s_lut)[tid + k * NT] = f32x4{v[k], v[k], v[k], v[k]};
}

template <int CTRL>
__device__ __forceinline__ float dpp_row(float v) {  // row_shl:n = 0x100 + n, row_shr:n = 0x110 + n (within rows of 16 lanes)
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}

// P = convert passes (64 dwords = 256 source pixels each), NBUF = u8 windows (1: the next frame's DMA is issued right
// after the convert, into the window just consumed; 2: one frame ahead), W = waves (tiles) per workgroup
template <bool VIG, bool PYR, int NBUF, int P, int W>
__global__ __launch_bounds__(64 * W, ((PYR || P > 5 || NBUF > 2) ? MDC_EXP_STRIP_WAVES_PER_EU - 1 : MDC_EXP_STRIP_WAVES_PER_EU)) void remap_strip_kernel(const uint8_t* __restrict__ in, float* __restrict__ out, RemapArgs a,
                                                            StripPlan p, PyramidOut py, int nframes, int fpb, int interleave) {
#if __HIP_DEVICE_COMPILE__
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];
  const int win = p.win_bytes;                       // u8 window bytes (multiple of 64)
  const int per_wave = (4 + NBUF) * win + kStripPad;  // [float window 4 win][zero pad][NBUF u8 windows]
  float* s_lut = reinterpret_cast<float*>(smem + W * per_wave);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int group = p.d_order[xcd_table_entry((int)blockIdx.x, (int)blockIdx.y, p.rotate)];
  // the LUT is filled by the whole workgroup before anybody leaves
  fill_lut_rep<64 * W, kStripLutRep>(s_lut, a.lut, tid);
  __syncthreads();
  if (group < 0) return;
  const int tile = group * W + wave;
  if (tile >= p.n_tiles) return;
  const int fstep = interleave ? (int)gridDim.y : 1;
  const int f0 = interleave ? (int)blockIdx.y : (int)blockIdx.y * fpb;
  const int nf = interleave ? (nframes - f0 + fstep - 1) / fstep : min(nframes, f0 + fpb) - f0;
  if (nf <= 0) return;

  lds_u8_ptr s_f32 = (lds_u8_ptr)smem + wave * per_wave;
  lds_u8_ptr s_u8 = s_f32 + 4 * win + kStripPad;
  lds_f32_ptr my_lut = (lds_f32_ptr)s_lut + (lane & (kStripLutRep - 1));
  if (lane < kStripPad / 4) reinterpret_cast<__attribute__((address_space(3))) float*>(s_f32 + 4 * win)[lane] = 0.f;

  const int tx = tile % p.tiles_x, ty = tile / p.tiles_x;
  const int nch = p.d_nch[tile];
  const uint32_t* chunks = p.d_chunks + (size_t)tile * kStripCap;
  uint32_t goff[2];
#pragma unroll
  for (int k = 0; k < 2; k++) goff[k] = chunks[lane + 64 * k];  // kOutside past the window (host padding)
  uint32_t cgoff[P];
  bool cvalid[P];
#pragma unroll
  for (int j = 0; j < P; j++) {
    const int d = j * 64 + lane;
    cvalid[j] = (d >> 2) < nch;
    cgoff[j] = chunks[min(d >> 2, kStripCap - 1)] + (uint32_t)(d & 3) * 4u;
  }
  // 16 outputs: o = 8 h + r, column tx*128 + lane + 64 h, row ty*8 + r
  float fx[16], fy[16];
  uint32_t tap[16];
#pragma unroll
  for (int h = 0; h < 2; h++)
#pragma unroll
    for (int r = 0; r < 8; r++) {
      const int ox = tx * 128 + lane + 64 * h, oy = ty * 8 + r;
      const bool inside = ox < a.out_w && oy < a.out_h;
      const int oidx = inside ? oy * a.out_w + ox : 0;
      float xx = a.rx[oidx], yy = a.ry[oidx];
      uint32_t tp = p.d_taps[oidx];
      const bool black = !inside || xx < 0;  // black (and outside) outputs sample the zero pair with weights (0, 0, 0, 1)
      if (black) {
        xx = yy = 0.f;
        tp = (uint32_t)(4 * win) * 0x00010001u;
      }
      fx[8 * h + r] = xx - (float)(int)xx;  // src/FOVUndistorter.cpp:352-355
      fy[8 * h + r] = yy - (float)(int)yy;
      tap[8 * h + r] = tp;
    }
  f32x4 vin[P];
#pragma unroll
  for (int j = 0; j < P; j++) {
    vin[j] = f32x4{1.f, 1.f, 1.f, 1.f};
    if (VIG && cvalid[j]) vin[j] = *reinterpret_cast<const f32x4*>(a.vinv + cgoff[j]);
  }
  const uint32_t in_bytes = (uint32_t)a.in_w * (uint32_t)a.in_h;
  const uint32_t out_bytes = (uint32_t)a.out_w * (uint32_t)a.out_h * 4u;
  const uint32_t row_bytes = (uint32_t)a.out_w * 4u;
  // store offsets: lane part in a VGPR (kOutsideLean-style sentinel for columns outside the image: still beyond the
  // frame after adding any row's offset), row part as the instruction's scalar offset; rows below the image fall
  // outside the frame's descriptor and are dropped
  uint32_t vo[2];
#pragma unroll
  for (int h = 0; h < 2; h++) {
    const int ox = tx * 128 + lane + 64 * h;
    vo[h] = ox < a.out_w ? (uint32_t)((ty * 8) * a.out_w + ox) * 4u : kOutsideLean;
  }
  // pyramid offsets (whole tiles only, so everything is inside)
  uint32_t p1o[2] = {0, 0}, p2o = kOutside, p3o = kOutside;
  if (PYR) {
#pragma unroll
    for (int h = 0; h < 2; h++)  // level 1: even lanes row 2q (+0), odd lanes row 2q + 1, column (ox >> 1); q adds 2 rows (scalar)
      p1o[h] = (uint32_t)((ty * 4 + (lane & 1)) * (a.out_w >> 1) + ((tx * 128 + lane + 64 * h) >> 1)) * 4u;
    {  // level 2: lane 4k + j stores the value of (h, q) = (j >> 1, j & 1): row ty*2 + q, column tx*32 + 16 h + k
      const int j = lane & 3, k = lane >> 2;
      p2o = (uint32_t)((ty * 2 + (j & 1)) * (a.out_w >> 2) + tx * 32 + 16 * (j >> 1) + k) * 4u;
    }
    if ((lane & 3) == 0) {  // level 3: lane 8 i stores h = 0, lane 8 i + 4 stores h = 1: row ty, column tx*16 + 8 h + i
      const int h = (lane >> 2) & 1, i = lane >> 3;
      p3o = (uint32_t)(ty * (a.out_w >> 3) + tx * 16 + 8 * h + i) * 4u;
    }
  }
  const long long in_step = (long long)fstep * in_bytes;
  const long long out_step = (long long)fstep * (out_bytes / 4);
  const uint8_t* src = in + (long long)f0 * in_bytes;
  float* dst = out + (long long)f0 * (out_bytes / 4);
#if MDC_EXP_STRIP_FAKE_GRAD
  float* s_gt = reinterpret_cast<float*>(smem + W * per_wave + kStripLutBytes) + wave * 384;  // wave-private [2][192] transpose scratch
#endif
  const int last = nf - 1;
  const int rw = nch > 64 ? 2 : 1;  // DMA instructions per frame (wave-uniform)
  const uint32_t l1_bytes = out_bytes / 4, l2_bytes = out_bytes / 16, l3_bytes = out_bytes / 64;

  if (nch == 0) {  // every output of the tile is black: zeros on every level, no staging
    for (int f = 0; f < nf; f++, dst += out_step) {
      const auto ro = MDC_FRAME_RSRC(uniform_ptr(dst), out_bytes);
#pragma unroll
      for (int h = 0; h < 2; h++)
#pragma unroll
        for (int r = 0; r < 8; r++) __builtin_amdgcn_raw_buffer_store_b32(0u, ro, vo[h], r * row_bytes, 0);
      if (PYR) {
        const long long fa = (long long)f0 + (long long)f * fstep;
        if (py.l1) {
          const auto r1 = MDC_FRAME_RSRC(uniform_ptr(py.l1 + fa * (l1_bytes / 4)), l1_bytes);
#pragma unroll
          for (int h = 0; h < 2; h++)
#pragma unroll
            for (int q = 0; q < 2; q++) __builtin_amdgcn_raw_buffer_store_b32(0u, r1, p1o[h], q * row_bytes, 0);
        }
        if (py.l2) __builtin_amdgcn_raw_buffer_store_b32(0u, MDC_FRAME_RSRC(uniform_ptr(py.l2 + fa * (l2_bytes / 4)), l2_bytes), p2o, 0, 0);
        if (py.l3) __builtin_amdgcn_raw_buffer_store_b32(0u, MDC_FRAME_RSRC(uniform_ptr(py.l3 + fa * (l3_bytes / 4)), l3_bytes), p3o, 0, 0);
      }
    }
    return;
  }
  MDC_CHECK(nch <= kStripCap && nch * 16 <= win && 4 * nch <= 64 * P);

  auto stage = [&](int fr, int buf) {
#if MDC_EXP_SKIP_LOAD
    const auto ri = MDC_FRAME_RSRC(uniform_ptr(src + 0 * (long long)min(fr, last) * in_step), in_bytes);
#else
    const auto ri = MDC_FRAME_RSRC(uniform_ptr(src + (long long)min(fr, last) * in_step), in_bytes);
#endif
    lds_u8_ptr u = s_u8 + buf * win;
#pragma unroll
    for (int k = 0; k < 2; k++)
      if (k < rw && goff[k] != kOutside) {
        MDC_CHECK(goff[k] + 16u <= in_bytes && (goff[k] & 15u) == 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(ri, (lds_void_ptr)(u + k * 1024), 16, goff[k], 0, 0, kLoadAux);
      }
    __builtin_amdgcn_sched_barrier(0);
  };
  // S = stores per frame issued after the frame's DMA: 16 (+ 4 + 1 + 1 with all pyramid levels)
  const bool pyr_all = PYR && py.l1 && py.l2 && py.l3;
  // NBUF >= 2: D = NBUF - 1 frames are staged ahead (the u8 windows are small: depth is cheap, and what the read side of
  // this kernel needs is bytes in flight -- its DMA latency is ~2.5 us).  NBUF == 1: the next frame's DMA is issued right
  // after the convert, into the window just consumed.
  constexpr int D = NBUF >= 2 ? NBUF - 1 : 1;
  if (NBUF >= 2) {
#pragma unroll
    for (int d = 0; d < D; d++) stage(d, d);
  } else {
    stage(0, 0);
  }
  int ub = 0;
  for (int f = 0; f <= last; f++) {
    if (NBUF >= 2) {
      int nb = ub + D;
      if (nb >= NBUF) nb -= NBUF;
      stage(f + D, nb);
      // DMA(f) landed.  Issued after it: f >= D: the stores of iteration f-D, then (rw + S) per iteration f-D+1 .. f-1, then
      // this iteration's DMA = D (rw + S); f < D (prologue): at least the D DMA groups.  A count beyond the counter's 63
      // cannot be waited for -- and need not: with 64 younger operations issued the older one has retired (in order).
      constexpr int Sn = 16, Sp = 22;
      if (f < D) {
        if (rw == 2) wait_vm<(2 * D < 63 ? 2 * D : 63)>();
        else wait_vm<D>();
      } else if (pyr_all) {
        if (rw == 2) wait_vm<(D * (2 + Sp) < 63 ? D * (2 + Sp) : 63)>();
        else wait_vm<(D * (1 + Sp) < 63 ? D * (1 + Sp) : 63)>();
      } else {
        if (rw == 2) wait_vm<(D * (2 + Sn) < 63 ? D * (2 + Sn) : 63)>();
        else wait_vm<(D * (1 + Sn) < 63 ? D * (1 + Sn) : 63)>();
      }
    } else {  // single window: DMA(f) was issued after the previous frame's convert, followed by that frame's stores only
      if (f == 0) wait_vm<0>();
      else if (pyr_all) wait_vm<22>();
      else wait_vm<16>();
    }
    // ---- convert: u8 window -> lut (* vignette) -> float window
    lds_u8_ptr ubuf = s_u8 + (NBUF >= 2 ? ub : 0) * win;
#if !MDC_EXP_STRIP_NOCONVERT
    {
      uint32_t word[P];
#pragma unroll
      for (int j = 0; j < P; j++) word[j] = *reinterpret_cast<const volatile __attribute__((address_space(3))) uint32_t*>(ubuf + (j * 64 + lane) * 4);
#pragma unroll
      for (int j = 0; j < P; j++) {
        f32x4 r;
#pragma unroll
        for (int k = 0; k < 4; k++) r[k] = my_lut[(int)((word[j] >> (8 * k)) & 0xffu) * kStripLutRep];
        if (VIG) r = r * vin[j];
        if (cvalid[j]) *reinterpret_cast<__attribute__((address_space(3))) f32x4*>(s_f32 + (j * 64 + lane) * 16) = r;
      }
    }
#endif
    // LDS operations of one wave execute in order: the sample phase's reads see the convert's writes.  (The compiler
    // keeps the order too: same address space, may alias.)
    if (NBUF == 1) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the u8 reads above have returned: the window may be overwritten
      stage(f + 1, 0);
    }
    const auto ro = MDC_FRAME_RSRC(uniform_ptr(dst), out_bytes);
    const long long fa = (long long)f0 + (long long)f * fstep;
    const uint32_t f_base = (uint32_t)(uintptr_t)s_f32;  // LDS byte address of the wave's float window
    float v2[2][2];
#pragma unroll
    for (int h = 0; h < 2; h++)
#pragma unroll
      for (int q = 0; q < 2; q++) {
        float res[4];
        // Two outputs at a time.  Their addresses and weights are REDONE every frame from the packed per-output constants
        // (tap offsets 16 | 16 bits, fx, fy: 48 registers for 16 outputs) -- hoisted out of the frame loop they would be
        // 32 addresses + 64 weights and the kernel would run at 3 waves per SIMD.  volatile asm is what keeps the
        // optimiser from hoisting: v_add_u32_sdwa adds one 16-bit half of the packed offsets to the window base in ONE
        // instruction (no unpack), v_mul / v_sub seed the weight expressions (IEEE single operations, the same the compiler
        // would emit: same bits).
#pragma unroll
        for (int u0 = 0; u0 < 4; u0 += 2) {
          float tv[2][4];
          uint32_t a0[2], a1[2];
#pragma unroll
          for (int u = 0; u < 2; u++) {
            const int o = 8 * h + 4 * q + u0 + u;
            asm volatile("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_0" : "=v"(a0[u]) : "v"(f_base), "v"(tap[o]));
            asm volatile("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_1" : "=v"(a1[u]) : "v"(f_base), "v"(tap[o]));
            MDC_CHECK(a0[u] - f_base + 8 <= (uint32_t)(4 * win + kStripPad) && a1[u] - f_base + 8 <= (uint32_t)(4 * win + kStripPad));
          }
#if MDC_EXP_STRIP_NOSAMPLE
#pragma unroll
          for (int u = 0; u < 2; u++) {
            res[u0 + u] = __uint_as_float(a0[u] ^ a1[u]);
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(res[u0 + u]), ro, vo[h], (uint32_t)(4 * q + u0 + u) * row_bytes, kStoreAux);
          }
          continue;
#endif
#pragma unroll
          for (int u = 0; u < 2; u++) {
            lds_f32_ptr t0 = reinterpret_cast<lds_f32_ptr>((lds_u8_ptr)0 + a0[u]);
            lds_f32_ptr t1 = reinterpret_cast<lds_f32_ptr>((lds_u8_ptr)0 + a1[u]);
            tv[u][0] = t0[0];
            tv[u][1] = t0[1];
            tv[u][2] = t1[0];
            tv[u][3] = t1[1];
          }
#pragma unroll
          for (int u = 0; u < 2; u++) {
            const int o = 8 * h + 4 * q + u0 + u;
            Bilin bw;
            float xxyy, omx;
            asm volatile("v_mul_f32 %0, %1, %2" : "=v"(xxyy) : "v"(fx[o]), "v"(fy[o]));  // xx*yy        src/FOVUndistorter.cpp:356
            asm volatile("v_sub_f32 %0, 1.0, %1" : "=v"(omx) : "v"(fx[o]));              // 1 - xx        :365
            bw.w11 = xxyy;
            bw.w01 = fy[o] - xxyy;
            bw.w10 = fx[o] - xxyy;
            bw.w00 = (omx - fy[o]) + xxyy;
            res[u0 + u] = bilin_sum(bw, tv[u][0], tv[u][1], tv[u][2], tv[u][3]);
#if MDC_EXP_SKIP_STORE
            if (res[u0 + u] != -1.2345e30f) continue;
#endif
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(res[u0 + u]), ro, vo[h], (uint32_t)(4 * q + u0 + u) * row_bytes, kStoreAux);
#if MDC_EXP_STRIP_FAKE_GRAD
            if (py.gI) {  // the stores of a fused level-0 gradient: 192 wave-contiguous floats of triples through a wave-private transpose + absSquaredGrad
              const uint32_t R = (uint32_t)(4 * q + u0 + u);
              float* tt = s_gt + (R & 1u) * 192;
              tt[3 * lane + 0] = res[u0 + u];
              tt[3 * lane + 1] = res[u0 + u] * 0.5f;
              tt[3 * lane + 2] = res[u0 + u] * 0.25f;
              __builtin_amdgcn_wave_barrier();
              const auto rg = MDC_FRAME_RSRC(uniform_ptr(py.gI + fa * (long long)(out_bytes / 4) * 3), out_bytes * 3u);
              const uint32_t rowoff = (uint32_t)(((ty * 8 + (int)R) * a.out_w + tx * 128 + 64 * h) * 12);
#pragma unroll
              for (int k3 = 0; k3 < 3; k3++)
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(tt[k3 * 64 + lane]), rg, rowoff + (uint32_t)(k3 * 64 + lane) * 4u, 0, kStoreAux);
              __builtin_amdgcn_wave_barrier();
              const auto ra = MDC_FRAME_RSRC(uniform_ptr(py.gA + fa * (long long)(out_bytes / 4)), out_bytes);
              __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(res[u0 + u] * res[u0 + u]), ra, vo[h], R * row_bytes, kStoreAux);
            }
#endif
          }
        }
#if MDC_EXP_STRIP_FAKE_GRAD
        if (py.gI && q == 0) {  // the halo's samples: 5 more sample slots per 16 outputs (2 x 128 halo row outputs + 16 halo column outputs per 1024)
          float dummy = 0.f;
#pragma unroll
          for (int e = 0; e < (h == 0 ? 3 : 2); e++) {
            uint32_t b0, b1;
            asm volatile("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_0" : "=v"(b0) : "v"(f_base), "v"(tap[8 * h + e]));
            asm volatile("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_1" : "=v"(b1) : "v"(f_base), "v"(tap[8 * h + e]));
            lds_f32_ptr t0 = reinterpret_cast<lds_f32_ptr>((lds_u8_ptr)0 + b0);
            lds_f32_ptr t1 = reinterpret_cast<lds_f32_ptr>((lds_u8_ptr)0 + b1);
            Bilin bw;
            float xxyy, omx;
            asm volatile("v_mul_f32 %0, %1, %2" : "=v"(xxyy) : "v"(fx[8 * h + e]), "v"(fy[8 * h + e]));
            asm volatile("v_sub_f32 %0, 1.0, %1" : "=v"(omx) : "v"(fx[8 * h + e]));
            bw.w11 = xxyy;
            bw.w01 = fy[8 * h + e] - xxyy;
            bw.w10 = fx[8 * h + e] - xxyy;
            bw.w00 = (omx - fy[8 * h + e]) + xxyy;
            dummy += bilin_sum(bw, t0[0], t0[1], t1[0], t1[1]);
          }
          if (dummy == -1.2345e30f) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(dummy), ro, vo[h], 0, kStoreAux);
        }
#endif
        if (PYR) {  // levels 1 and 2 of this column half / row quad, as pyramid_levels12
          float v1[2];
#pragma unroll
          for (int pp = 0; pp < 2; pp++) {
            const float b = dpp_quad<0xF5>(res[2 * pp]);
            const float d = dpp_quad<0xF5>(res[2 * pp + 1]);
            v1[pp] = box4(res[2 * pp], b, res[2 * pp + 1], d);
          }
          if (py.l1) {
            const auto r1 = MDC_FRAME_RSRC(uniform_ptr(py.l1 + fa * (l1_bytes / 4)), l1_bytes);
            const float left2 = dpp_quad<0xA0>(v1[1]);
            const float mm = (lane & 1) ? left2 : v1[0];
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(mm), r1, p1o[h], (uint32_t)q * row_bytes, kStoreAux);  // 2 level-1 rows = row_bytes
          }
          const float b2 = dpp_quad<0xAA>(v1[0]);
          const float d2 = dpp_quad<0xAA>(v1[1]);
          v2[h][q] = box4(v1[0], b2, v1[1], d2);  // valid in lanes 4k
        }
      }
    if (PYR) {
      if (py.l2) {  // lane 4k + j stores (h, q) = (j >> 1, j & 1): one 64-lane store
        const float a00 = dpp_quad<0x00>(v2[0][0]), a01 = dpp_quad<0x00>(v2[0][1]), a10 = dpp_quad<0x00>(v2[1][0]), a11 = dpp_quad<0x00>(v2[1][1]);
        const int j = lane & 3;
        const float mm = j == 0 ? a00 : j == 1 ? a01 : j == 2 ? a10 : a11;
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(mm), MDC_FRAME_RSRC(uniform_ptr(py.l2 + fa * (l2_bytes / 4)), l2_bytes), p2o, 0, kStoreAux);
      }
      if (py.l3) {  // level 3: lanes 8 i; the right neighbour's level-2 pixel sits 4 lanes up (same row of 16 lanes)
        float v3[2];
#pragma unroll
        for (int h = 0; h < 2; h++) v3[h] = box4(v2[h][0], dpp_row<0x104>(v2[h][0]), v2[h][1], dpp_row<0x104>(v2[h][1]));
        const float up = dpp_row<0x114>(v3[1]);  // lane 8 i + 4 takes h = 1 from lane 8 i
        const float mm = (lane & 4) ? up : v3[0];
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(mm), MDC_FRAME_RSRC(uniform_ptr(py.l3 + fa * (l3_bytes / 4)), l3_bytes), p3o, 0, kStoreAux);
      }
    }
    dst += out_step;
    ub = ub + 1 == NBUF ? 0 : ub + 1;
  }
#endif
}

// ----------------------------------------------------------------------------
// 2x2 box pyramid level (config 5; not in the reference): 0.25f*(((a+b)+c)+d).
// ----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pyramid_level_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                            int w, int h, long long nframes) {
  const int w2 = w >> 1, h2 = h >> 1;
  const long long n2 = (long long)w2 * h2;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n2 * nframes) return;
  const long long f = i / n2;
  const int r = (int)(i - f * n2);
  const int y = r / w2, x = r - y * w2;
  const float* p = src + f * (long long)w * h + (long long)(2 * y) * w + 2 * x;
  dst[i] = 0.25f * (((p[0] + p[1]) + p[w]) + p[w + 1]);
}

// ----------------------------------------------------------------------------
// UndistorterFOV::distortCoordinates on the device (reference src/FOVUndistorter.cpp:280-319), for callers that warp many
// points per frame (vignetteCalib: 10^6 per image, src/main_vignetteCalib.cpp:284).  The per-point arithmetic -- with the
// restatement of the HOST libm's atanf that bit-exactness needs -- lives in fov_point_model.h, a header the host compiler
// takes as well: tests/test_distort_points_cpu.py pins it to the build box's libm and to the class's host path on the CPU.
// ----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void distort_points_kernel(float* __restrict__ xs, float* __restrict__ ys, long long n,
                                                             DistortModel m) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float x = xs[i], y = ys[i];
  fov_distort_point(m, x, y);
  xs[i] = x;
  ys[i] = y;
}

inline int ceil_div(long long a, long long b) { return (int)((a + b - 1) / b); }

}  // namespace

size_t tiled_lds_bytes(int win_bytes, int nbuf, bool lut) { return (lut ? (size_t)kLutBytes : 0) + (size_t)nbuf * win_bytes; }
size_t tiled_pyramid_lds_bytes(int tile_w, int tile_h) { return (size_t)2 * (tile_h / 4) * (tile_w / 4) * sizeof(float); }

hipError_t launch_unmap(const uint8_t* d_in, float* d_out, const float* d_lut, const float* d_vinv, int64_t npix,
                        int64_t nframes, int fpb, hipStream_t s) {
  if (nframes <= 0 || npix <= 0) return hipSuccess;
  const int groups = ceil_div(nframes, fpb);
  const bool vec = (npix % 4 == 0) && ((reinterpret_cast<uintptr_t>(d_in) & 3) == 0);
  if (vec) {
    dim3 grid(ceil_div(npix, 4096), groups);
    if (d_vinv) unmap_xpose_kernel<true><<<grid, 256, 0, s>>>(d_in, d_out, d_lut, d_vinv, npix, (int)nframes, fpb);
    else unmap_xpose_kernel<false><<<grid, 256, 0, s>>>(d_in, d_out, d_lut, d_vinv, npix, (int)nframes, fpb);
  } else {
    dim3 grid(ceil_div(npix, 256), groups);
    if (d_vinv) unmap_scalar_kernel<true><<<grid, 256, 0, s>>>(d_in, d_out, d_lut, d_vinv, npix, (int)nframes, fpb);
    else unmap_scalar_kernel<false><<<grid, 256, 0, s>>>(d_in, d_out, d_lut, d_vinv, npix, (int)nframes, fpb);
  }
  return hipGetLastError();
}

hipError_t launch_remap_gather_u8(const uint8_t* d_in, float* d_out, const RemapArgs& a, int64_t nframes, int fpb,
                                  hipStream_t s) {
  if (nframes <= 0) return hipSuccess;
  dim3 grid(ceil_div((long long)a.out_w * a.out_h, 256), ceil_div(nframes, fpb));
  if (a.vinv) remap_gather_u8_kernel<true><<<grid, 256, 0, s>>>(d_in, d_out, a, (int)nframes, fpb);
  else remap_gather_u8_kernel<false><<<grid, 256, 0, s>>>(d_in, d_out, a, (int)nframes, fpb);
  return hipGetLastError();
}

hipError_t launch_remap_gather_f32(const float* d_in, float* d_out, const RemapArgs& a, int64_t nframes, int fpb,
                                   hipStream_t s) {
  if (nframes <= 0) return hipSuccess;
  dim3 grid(ceil_div((long long)a.out_w * a.out_h, 256), ceil_div(nframes, fpb));
  remap_gather_f32_kernel<<<grid, 256, 0, s>>>(d_in, d_out, a, (int)nframes, fpb);
  return hipGetLastError();
}

struct TiledLaunch {
  const uint8_t* d_in;
  float* d_out;
  RemapArgs a;
  TilePlan p;
  PyramidOut py;
  int64_t nframes;
  int fpb;
  hipStream_t s;
};

// Frame groups of a launch with a tapered tail: see remap_tiled_kernel.  -> number of groups; *full = groups of fpb frames
// (taper_r = 0: no taper, ceil(nframes / fpb) groups).
static int taper_groups(int64_t nframes, int fpb, int taper_r, int* full) {
  *full = 0;
  if (taper_r <= 0) return (int)ceil_div(nframes, fpb);
  const int64_t tail = (int64_t)taper_r * (fpb / 2 + fpb / 4);  // frames of the fpb/2 and fpb/4 groups
  *full = (int)((nframes - tail) / fpb);
  const int64_t rest = nframes - (int64_t)*full * fpb - tail;   // in [0, fpb): groups of fpb/8
  return *full + 2 * taper_r + (int)ceil_div(rest, fpb / 8);
}

template <bool VIG, bool BLACK, bool PYR, bool F32, int TW, int NT, int NBUF>
static hipError_t launch_tiled_variant(const TiledLaunch& l) {
  const size_t lds = tiled_lds_bytes(l.p.win_bytes, NBUF, !F32) + (PYR ? tiled_pyramid_lds_bytes(l.p.tile_w, l.p.tile_h) : 0);
  // taper: about one resident round of workgroups per level; only launches of many rounds, frames per workgroup a multiple of 8
  const int resident = 256 * (int)std::max<size_t>(1, std::min<size_t>(2048 / NT, kLdsPerCU / std::max<size_t>(lds, 1)));
  int taper_r = std::max(2, (resident + l.p.n_blocks / 2) / std::max(1, l.p.n_blocks));
  if (!l.p.taper || l.p.interleave || l.fpb % 8 != 0 || l.fpb < 16 || l.nframes < (int64_t)l.fpb * (4 * taper_r)) taper_r = 0;
  int taper_full = 0;
  dim3 grid(l.p.n_blocks, taper_groups(l.nframes, l.fpb, taper_r, &taper_full));
  if (lds > 64 * 1024) {  // more than 64 KiB of dynamic LDS needs the opt-in
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&remap_tiled_kernel<VIG, BLACK, PYR, F32, TW, NT, NBUF>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  remap_tiled_kernel<VIG, BLACK, PYR, F32, TW, NT, NBUF><<<grid, NT, lds, l.s>>>(l.d_in, l.d_out, l.a, l.p, l.py, (int)l.nframes, l.fpb,
                                                                                 l.p.interleave ? 1 : 0, taper_full, taper_r);
  return hipGetLastError();
}

template <bool VIG, bool BLACK, bool PYR, bool F32, int TW, int NT>
static hipError_t launch_tiled_buf(const TiledLaunch& l) {
  constexpr int RPT = tile_rpt(TW, 0);
  switch (l.p.nbuf) {
    case 2:  // (the 8-rows-per-thread tiles: 3 buffers only -- with 2 the compiler's schedule needs 97 VGPRs, one more than 5 waves per SIMD leave)
      if constexpr (RPT == 4) return launch_tiled_variant<VIG, BLACK, PYR, F32, TW, NT, 2>(l);
      break;
    case 3: return launch_tiled_variant<VIG, BLACK, PYR, F32, TW, NT, 3>(l);
    case 4:
      if constexpr (NT <= 512) return launch_tiled_variant<VIG, BLACK, PYR, F32, TW, NT, 4>(l);  // 4 buffers of a 1024-thread tile never fit
      break;
  }
  return hipErrorInvalidValue;
}

// tile shape -> instantiation.  kTileShapes (mdc_internal.h) lists the legal (tile_w, tile_h) pairs.
template <bool VIG, bool BLACK, bool PYR, bool F32>
static hipError_t launch_tiled_shape(const TiledLaunch& l) {
  switch (l.p.tile_w * 1000 + l.p.tile_h) {
    case 64016: return launch_tiled_buf<VIG, BLACK, PYR, F32, 64, 256>(l);
    case 64032: return launch_tiled_buf<VIG, BLACK, PYR, F32, 64, 512>(l);
    case 64060:  // 15 row groups: no level-3 pairs
      if constexpr (!PYR) return launch_tiled_buf<VIG, BLACK, false, F32, 64, 960>(l);
      break;
    // (the 1024-thread tiles have no fused-pyramid instantiation: at their 64-VGPR budget it spilled 12 bytes; the host
    // runs the per-level passes for them)
    case 64064:
      if constexpr (!PYR) return launch_tiled_buf<VIG, BLACK, false, F32, 64, 1024>(l);
      break;
    case 128016: return launch_tiled_buf<VIG, BLACK, PYR, F32, 128, 512>(l);
    case 128032:
      if constexpr (!PYR) return launch_tiled_buf<VIG, BLACK, false, F32, 128, 1024>(l);
      break;
  }
  return hipErrorInvalidValue;
}

template <bool VIG, bool BLACK>
static hipError_t launch_tiled_nt(const TiledLaunch& l) {
  const bool pyr = l.py.l1 || l.py.l2 || l.py.l3;
  return pyr ? launch_tiled_shape<VIG, BLACK, true, false>(l) : launch_tiled_shape<VIG, BLACK, false, false>(l);
}

// ---- strip kernel: VIG x PYR x NBUF {1..4} x P {2, 3, 4, 5, 8}
size_t strip_lds_bytes(int win_bytes, int nbuf, int waves) {
  return (size_t)waves * ((4 + nbuf) * win_bytes + kStripPad) + kStripLutBytes
#if MDC_EXP_STRIP_FAKE_GRAD
         + (size_t)waves * 1536
#endif
      ;
}
template <bool VIG, bool PYR, int NBUF, int P>
static hipError_t launch_strip_variant(const uint8_t* d_in, float* d_out, const RemapArgs& a, const StripPlan& p, const PyramidOut& py,
                                       int64_t nframes, int fpb, hipStream_t s) {
  constexpr int W = kStripWaves;
  dim3 grid(p.n_blocks, ceil_div(nframes, fpb));
  const size_t lds = strip_lds_bytes(p.win_bytes, NBUF, W);
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&remap_strip_kernel<VIG, PYR, NBUF, P, W>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  remap_strip_kernel<VIG, PYR, NBUF, P, W><<<grid, 64 * W, lds, s>>>(d_in, d_out, a, p, py, (int)nframes, fpb, p.interleave ? 1 : 0);
  return hipGetLastError();
}
template <bool VIG, bool PYR, int NBUF>
static hipError_t launch_strip_passes(const uint8_t* d_in, float* d_out, const RemapArgs& a, const StripPlan& p, const PyramidOut& py,
                                      int64_t nframes, int fpb, hipStream_t s) {
  switch (p.passes) {
    case 2: return launch_strip_variant<VIG, PYR, NBUF, 2>(d_in, d_out, a, p, py, nframes, fpb, s);
    case 3: return launch_strip_variant<VIG, PYR, NBUF, 3>(d_in, d_out, a, p, py, nframes, fpb, s);
    case 4: return launch_strip_variant<VIG, PYR, NBUF, 4>(d_in, d_out, a, p, py, nframes, fpb, s);
    case 5: return launch_strip_variant<VIG, PYR, NBUF, 5>(d_in, d_out, a, p, py, nframes, fpb, s);
    case 8: return launch_strip_variant<VIG, PYR, NBUF, 8>(d_in, d_out, a, p, py, nframes, fpb, s);
  }
  return hipErrorInvalidValue;
}
#if MDC_EXP_STRIP_FAKE_GRAD
float* g_fake_grad_dI = nullptr;  // diagnosis plumbing: set per launch by enqueue_pyramid_gradients (mdc_pyramid.hip)
float* g_fake_grad_abs = nullptr;
#endif
hipError_t launch_remap_strip_u8(const uint8_t* d_in, float* d_out, const RemapArgs& a, const StripPlan& p, int64_t nframes, int fpb,
                                 hipStream_t s, float* d_l1, float* d_l2, float* d_l3) {
  if (nframes <= 0) return hipSuccess;
  if ((int64_t)a.in_w * a.in_h >= (int64_t)kOutside || (int64_t)a.out_w * (a.out_h + 8) * 4 >= 0xc0000000ll) return hipErrorInvalidValue;
#if MDC_EXP_STRIP_FAKE_GRAD
  const PyramidOut py{d_l1, d_l2, d_l3, g_fake_grad_dI, g_fake_grad_abs};
#else
  const PyramidOut py{d_l1, d_l2, d_l3};
#endif
  const bool pyr = d_l1 || d_l2 || d_l3;
#define MDC_STRIP(V_, P_)                                                                                        \
  (p.nbuf == 1   ? launch_strip_passes<V_, P_, 1>(d_in, d_out, a, p, py, nframes, fpb, s)                          \
   : p.nbuf == 2 ? launch_strip_passes<V_, P_, 2>(d_in, d_out, a, p, py, nframes, fpb, s)                          \
   : p.nbuf == 3 ? launch_strip_passes<V_, P_, 3>(d_in, d_out, a, p, py, nframes, fpb, s)                          \
                 : launch_strip_passes<V_, P_, 4>(d_in, d_out, a, p, py, nframes, fpb, s))
  if (a.vinv) return pyr ? MDC_STRIP(true, true) : MDC_STRIP(true, false);
  return pyr ? MDC_STRIP(false, true) : MDC_STRIP(false, false);
#undef MDC_STRIP
}

hipError_t launch_remap_tiled_u8(const uint8_t* d_in, float* d_out, const RemapArgs& a, const TilePlan& p,
                                 int64_t nframes, int fpb, hipStream_t s, float* d_l1, float* d_l2, float* d_l3) {
  if (nframes <= 0) return hipSuccess;
  // frames are addressed through 32-bit buffer offsets
  if ((int64_t)a.in_w * a.in_h >= (int64_t)kOutside || (int64_t)a.out_w * a.out_h * 4 >= (int64_t)kOutside)
    return hipErrorInvalidValue;
  PyramidOut tiled_py{};
  tiled_py.l1 = d_l1, tiled_py.l2 = d_l2, tiled_py.l3 = d_l3;
  const TiledLaunch l{d_in, d_out, a, p, tiled_py, nframes, fpb, s};
  if (a.vinv) return p.has_black ? launch_tiled_nt<true, true>(l) : launch_tiled_nt<true, false>(l);
  return p.has_black ? launch_tiled_nt<false, true>(l) : launch_tiled_nt<false, false>(l);
}

hipError_t launch_remap_tiled_f32(const float* d_in, float* d_out, const RemapArgs& a, const TilePlan& p,
                                  int64_t nframes, int fpb, hipStream_t s) {
  if (nframes <= 0) return hipSuccess;
  if ((int64_t)a.in_w * a.in_h * 4 >= (int64_t)kOutside || (int64_t)a.out_w * a.out_h * 4 >= (int64_t)kOutside)
    return hipErrorInvalidValue;
  const TiledLaunch l{reinterpret_cast<const uint8_t*>(d_in), d_out, a, p, PyramidOut{}, nframes, fpb, s};
  return p.has_black ? launch_tiled_shape<false, true, false, true>(l) : launch_tiled_shape<false, false, false, true>(l);
}

// Software prefetch into the memory-side cache (the 256-MiB Infinity Cache): a LINEAR read of the source rows a chunk of
// frames will be sampled from, issued right before that chunk's remap launch.  The remap kernels read their windows as
// many small row pieces; interleaved with their output stream those reads cost far more HBM time than their bytes (the
// memory system serves reads and writes one after the other, and small scattered reads worst of all: round-3
// experiments 03, 05).  Reading the rows once, linearly, costs bytes / 6 TB/s; the window reads then hit the cache.
__global__ __launch_bounds__(256) void prefetch_rows_kernel(const uint8_t* __restrict__ frames, long long frame_bytes, long long first_byte,
                                                            int row_pitch, int row16, long long rows, long long nframes,
                                                            uint32_t* __restrict__ sink) {
  typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
  const long long per_frame = rows * row16, total = per_frame * nframes;
  uint32_t acc = 0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long f = i / per_frame, r = i - f * per_frame;
    const long long row = r / row16, k = r - row * row16;
    const u32x4_t v = *reinterpret_cast<const u32x4_t*>(frames + f * frame_bytes + first_byte + row * row_pitch + k * 16);
    acc ^= v.x ^ v.y ^ v.z ^ v.w;
  }
  if (acc == 0x9e3779b9u && sink) *sink = acc;  // keeps the loads alive; practically never taken
}

// rows [y0, y1] x byte columns [x0, x1] (widened to whole 128-byte lines) of every frame
hipError_t launch_prefetch_rows(const uint8_t* d_frames, int64_t frame_bytes, int row_pitch, int x0, int x1, int y0, int y1, int64_t nframes,
                                uint32_t* d_sink, hipStream_t s) {
  if (nframes <= 0 || y1 < y0 || x1 < x0) return hipSuccess;
  const int xa = x0 & ~127, xb = std::min(row_pitch, (x1 + 128) & ~127);
  if (xb - xa < 16 || (row_pitch & 15) != 0 || (reinterpret_cast<uintptr_t>(d_frames) & 15) != 0 || (frame_bytes & 15) != 0) return hipSuccess;
  prefetch_rows_kernel<<<4096, 256, 0, s>>>(d_frames, frame_bytes, (long long)y0 * row_pitch + xa, row_pitch, (xb - xa) / 16, (long long)(y1 - y0 + 1),
                                            nframes, d_sink);
  return hipGetLastError();
}

hipError_t launch_pyramid_level(const float* d_src, float* d_dst, int w, int h, int64_t nframes, hipStream_t s) {
  const long long n = (long long)(w >> 1) * (h >> 1) * nframes;
  if (n <= 0) return hipSuccess;
  pyramid_level_kernel<<<ceil_div(n, 256), 256, 0, s>>>(d_src, d_dst, w, h, nframes);
  return hipGetLastError();
}

hipError_t launch_distort_points(float* d_x, float* d_y, int64_t n, const DistortModel& m, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  distort_points_kernel<<<ceil_div(n, 256), 256, 0, s>>>(d_x, d_y, n, m);
  return hipGetLastError();
}

}  // namespace mdc
