// The box pyramid and DSO's gradient images of device frames: the gradient kernel, its launchers, the chunked base + levels
// (+ gradients) pass that the *_to_device pipeline shares (enqueue_pyramid_gradients) and the four mdc_*pyramid* / mdc_gradients*
// entry points.  The box level kernel (launch_pyramid_level) and the remap kernels that write levels 1..3 in the same launch are in
// mdc_kernels.hip; which of them runs is mdc_launch.hip's decision (enqueue_process).
#include "mdc_ctx.h"

namespace mdc {
namespace {

// ---------------------------------------------------------------------------------------------------------
// DSO hand-off (NOT in the reference -- DSO's FrameHessian::makeImages, definition in
// DESIGN.md section 5.5): for one pyramid level, per pixel the triple (I, dx, dy) with central differences
// dx = 0.5f*(I[idx+1] - I[idx-1]), dy = 0.5f*(I[idx+w] - I[idx-w]) over the LINEAR index range [w, w*(h-1)) -- rows
// 1 .. h-2, all columns, so the first and last column difference across the row boundary exactly as DSO's loop
// does --, non-finite differences replaced by 0, and absSquaredGrad = dx*dx + dy*dy.  First and last row: 0.
// A wave handles 64 consecutive columns of kGradRows rows: all of its loads (rows y0-1 .. y0+R of the column, the left and
// right neighbours of the R rows) are issued before the first result is needed -- the first version (one pixel per thread, one
// 256-pixel workgroup per 4 KB of output) ran at the latency of its five loads, 3.5 TB/s of output; per row the wave's 192
// floats (I, dx, dy interleaved) leave as three wave-contiguous dword stores through a wave-private LDS transpose instead
// of three stores at a 12-byte stride.  Up to four pyramid levels of a chunk of frames in ONE launch
// (mdc_process_pyramid_gradients_batch_device): a workgroup finds its level from the first-block table.
// ---------------------------------------------------------------------------------------------------------
constexpr int kGradRows = MDC_EXP_GRAD_ROWS, kGradThreads = 128;
struct GradLevels {
  const float* src[4];
  float* dI[4];
  float* abs2[4];
  int w[4], h[4];
  unsigned bx[4], bands[4];  // workgroups per row band (128 columns each), row bands (kGradRows rows each)
  unsigned first_block[5];   // blocks [first_block[l], first_block[l+1]) belong to level l
  int n;
};
__global__ __launch_bounds__(kGradThreads) void gradients_levels_kernel(GradLevels g) {
  constexpr int R = kGradRows;
  __shared__ float s_t[kGradThreads / 64][2][192];
  int l = 0;
#pragma unroll
  for (int k = 1; k < 4; k++)
    if (k < g.n && blockIdx.x >= g.first_block[k]) l = k;
  const int w = g.w[l], h = g.h[l];
  const unsigned b = blockIdx.x - g.first_block[l], per_frame = g.bx[l] * g.bands[l];
  const unsigned f = b / per_frame, rb = b - f * per_frame, band = rb / g.bx[l], bx = rb - band * g.bx[l];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x0 = (int)bx * kGradThreads + wave * 64;  // first column of this wave
  const int nvalid = min(64, w - x0);                  // wave-uniform
  if (nvalid <= 0) return;
  const int x = min(x0 + lane, w - 1);  // lanes past the row end repeat its last column (loads stay in bounds; nothing stored)
  const int y0 = (int)band * R;
  const int npx = w * h;
  const float* p = g.src[l] + (long long)f * npx;
  float c[R + 2], lf[R], rt[R];
#ifdef MDC_EXP_GRAD_FAKE_READ  // diagnosis (wrong results): every read of the levels comes from the frame's first 16 KB -- what do these reads cost?
#define MDC_GRAD_IDX(i) ((i) & 4095)
#else
#define MDC_GRAD_IDX(i) (i)
#endif
#pragma unroll
  for (int r = -1; r <= R; r++) c[r + 1] = p[MDC_GRAD_IDX(min(max(y0 + r, 0), h - 1) * w + x)];
  // left / right neighbours (linear index +-1): the neighbouring lanes' centre values; only the wave's first lane and its last valid
  // one load theirs (one instruction with two active lanes per row instead of two unaligned row loads)
#pragma unroll
  for (int r = 0; r < R; r++) {
    const int idx = min(y0 + r, h - 1) * w + x;
    float le = 0.f, re = 0.f;
    if (lane == 0) le = p[MDC_GRAD_IDX(max(idx - 1, 0))];
    if (lane == nvalid - 1) re = p[MDC_GRAD_IDX(min(idx + 1, npx - 1))];
    const float up = __shfl_up(c[r + 1], 1), dn = __shfl_down(c[r + 1], 1);
    lf[r] = lane == 0 ? le : up;
    rt[r] = lane == nvalid - 1 ? re : dn;
  }
#undef MDC_GRAD_IDX
  float* dI = g.dI[l] + ((long long)f * npx + (long long)y0 * w + x0) * 3;
  float* abs2 = g.abs2[l] + (long long)f * npx + (long long)y0 * w + x0;
#pragma unroll
  for (int r = 0; r < R; r++) {
    const int y = y0 + r;
    if (y >= h) break;  // wave-uniform
    float dx = 0.f, dy = 0.f;
    if (y >= 1 && y <= h - 2) {  // the linear index range [w, w*(h-1))
      dx = 0.5f * (rt[r] - lf[r]);
      dy = 0.5f * (c[r + 2] - c[r]);
      if (!isfinite(dx)) dx = 0.f;
      if (!isfinite(dy)) dy = 0.f;
    }
    if (lane < nvalid) __builtin_nontemporal_store(dx * dx + dy * dy, abs2 + (long long)r * w + lane);
    float* t = s_t[wave][r & 1];
    t[3 * lane + 0] = c[r + 1];
    t[3 * lane + 1] = dx;
    t[3 * lane + 2] = dy;
    __builtin_amdgcn_wave_barrier();  // wave-private transpose: a wave's LDS operations execute in order
#pragma unroll
    for (int k = 0; k < 3; k++)
      if (k * 64 + lane < 3 * nvalid) __builtin_nontemporal_store(t[k * 64 + lane], dI + (long long)r * w * 3 + k * 64 + lane);
    __builtin_amdgcn_wave_barrier();
  }
}

// (I, dx, dy) triples + absSquaredGrad of up to four levels in one launch
hipError_t launch_gradients_levels(int n_levels, const float* const* d_src, float* const* d_dI, float* const* d_abs2, const int* w,
                                   const int* h, int64_t nframes, hipStream_t s) {
  if (n_levels <= 0 || nframes <= 0) return hipSuccess;
  if (n_levels > 4) return hipErrorInvalidValue;
  GradLevels g;
  uint64_t nb = 0;
  for (int l = 0; l < 4; l++) {
    const bool on = l < n_levels && w[l] > 0 && h[l] > 0;
    g.src[l] = on ? d_src[l] : nullptr;
    g.dI[l] = on ? d_dI[l] : nullptr;
    g.abs2[l] = on ? d_abs2[l] : nullptr;
    g.w[l] = on ? w[l] : 1;
    g.h[l] = on ? h[l] : 1;
    g.bx[l] = (unsigned)((g.w[l] + kGradThreads - 1) / kGradThreads);
    g.bands[l] = (unsigned)((g.h[l] + kGradRows - 1) / kGradRows);
    g.first_block[l] = (unsigned)nb;
    if (on) nb += (uint64_t)g.bx[l] * g.bands[l] * (uint64_t)nframes;
    if ((int64_t)g.w[l] * g.h[l] >= (1ll << 30)) return hipErrorInvalidValue;  // 32-bit pixel indices inside a frame
  }
  if (nb >= (1ull << 31)) return hipErrorInvalidValue;  // callers split such batches (launch_gradients, enqueue_pyramid_gradients)
  g.first_block[4] = (unsigned)nb;
  g.n = n_levels;
  if (nb == 0) return hipSuccess;
  gradients_levels_kernel<<<(unsigned)nb, kGradThreads, 0, s>>>(g);
  return hipGetLastError();
}

// ... of one level
hipError_t launch_gradients(const float* d_level, float* d_dI, float* d_abs2, int w, int h, int64_t nframes, hipStream_t s) {
  if (w <= 0 || h <= 0) return hipSuccess;
  // launches of at most 2^30 workgroups
  const int64_t per_frame = (int64_t)((w + kGradThreads - 1) / kGradThreads) * ((h + kGradRows - 1) / kGradRows);
  const int64_t step = std::max<int64_t>(1, (1ll << 30) / per_frame);
  const int64_t npx = (int64_t)w * h;
  for (int64_t f0 = 0; f0 < nframes; f0 += step) {
    const float* src = d_level + f0 * npx;
    float* dI = d_dI + f0 * npx * 3;
    float* a2 = d_abs2 + f0 * npx;
    hipError_t e = launch_gradients_levels(1, &src, &dI, &a2, &w, &h, std::min(step, nframes - f0), s);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// `levels` counts level 0, the w x h image: a level that would be empty is an argument error of all three pyramid calls, found
// before anything is enqueued
int check_pyramid_levels(mdc_ctx* c, int w, int h, int levels) {
  for (int l = 0; l < levels; l++)
    if (l > 30 || (w >> l) < 1 || (h >> l) < 1) return fail(c, MDC_ERR_ARG, "level %d of a %dx%d image is empty", l, w, h);
  return MDC_OK;
}

// box levels first .. levels-1 of nframes w x h images, each from the level below it (level 0: d_base; level l: d_levels[l - 1])
int enqueue_box_levels(mdc_ctx* c, const float* d_base, float* const* d_levels, int first, int levels, int w, int h, int64_t nframes,
                       hipStream_t s) {
  const float* src = first == 1 ? d_base : d_levels[first - 2];
  for (int l = first; l < levels; l++) {
    MDC_HIP(c, launch_pyramid_level(src, d_levels[l - 1], w >> (l - 1), h >> (l - 1), nframes, s));
    src = d_levels[l - 1];
  }
  return MDC_OK;
}

}  // namespace

// base + box levels (+ gradient images when d_dI / d_abs_squared_grad are given) of nframes device-resident raw frames, in chunks;
// lock held by the caller (mdc_process_pyramid_gradients_batch_device and the *_to_device pipeline, mdc_pipeline.hip)
int enqueue_pyramid_gradients(mdc_ctx* c, const uint8_t* d_in, float* d_base, int levels, float* const* d_levels, float* const* d_dI,
                              float* const* d_abs_squared_grad, int64_t nframes, unsigned flags, int chunk_frames, hipStream_t s) {
  const bool with_gradients = d_dI != nullptr && d_abs_squared_grad != nullptr;
  const bool rect = (flags & MDC_RECTIFY) != 0;
  if (rect && !c->valid_remap) return fail(c, MDC_ERR_STATE, "no remap set (UndistorterFOV invalid)");
  const int w0 = frame_size(c, rect).w, h0 = frame_size(c, rect).h;
  const int iw = (rect || c->in_w <= 0) ? c->rm_in_w : c->in_w, ih = (rect || c->in_h <= 0) ? c->rm_in_h : c->in_h;
  if (w0 <= 0 || h0 <= 0 || iw <= 0 || ih <= 0) return fail(c, MDC_ERR_STATE, "frame size unknown");
  if (int rc = check_pyramid_levels(c, w0, h0, levels)) return rc;
  int lw[8], lh[8];
  size_t level_bytes = 0;
  for (int l = 0; l < levels; l++) {
    lw[l] = w0 >> l;
    lh[l] = h0 >> l;
    level_bytes += (size_t)lw[l] * lh[l] * sizeof(float);
  }
  // Frames per chunk.  Measured (tools/dso_rate.py, 1280 x 1024, 512 frames, profiles/r03_dso_rate.txt): 8 frames per chunk
  // 5.0 ms, 24: 4.2, 96: 3.85-3.89, separate launches over the whole batch: 3.87-3.95 -- the levels are NOT read back from the
  // Infinity Cache (the remap's stores are nontemporal: plain ones evict its prefetched source rows and measured slower in
  // total, experiment 11), the whole path runs at what the memory system gives 34.8 MB of writes + 7.6 MB of reads per
  // frame; chunks exist to bound the launch sizes, and below ~100 frames they lose to their tails.  Round 4, frames/s by chunk:
  // 91: 130.6 k, 6 x 86: 133 k, 96: 137-140 k, one chunk of 512: 134-137 k -- the automatic choice is 96 at 1280 x 1024.
  int64_t chunk = chunk_frames;
  if (chunk <= 0) {  // ~96 frames' worth at 1280 x 1024, a multiple of 32 (the remap launch's frames per workgroup divide it)
    chunk = (int64_t)((672ull << 20) / level_bytes);
    chunk = chunk >= 32 ? chunk / 32 * 32 : std::max<int64_t>(1, chunk);
  }
  {  // a gradient launch holds a chunk's workgroups of up to four levels: fewer than 2^31 (128 x 8 pixels each)
    int64_t wgs = 0;
    for (int l = 0; l < std::min(levels, 4); l++) wgs += (int64_t)((lw[l] + 127) / 128) * ((lh[l] + 7) / 8);
    chunk = std::max<int64_t>(1, std::min<int64_t>(chunk, ((1ll << 31) - 1) / std::max<int64_t>(1, wgs)));
  }
  const size_t npi = (size_t)iw * ih;
  for (int64_t f0 = 0; f0 < nframes; f0 += chunk) {
    const int64_t n = std::min<int64_t>(chunk, nframes - f0);
    float* lv[8];
    for (int l = 1; l < levels; l++) lv[l - 1] = d_levels[l - 1] + (size_t)f0 * lw[l] * lh[l];
    float* base = d_base + (size_t)f0 * w0 * h0;
    float* pyr[3] = {levels > 1 ? lv[0] : nullptr, levels > 2 ? lv[1] : nullptr, levels > 3 ? lv[2] : nullptr};
    bool fused = false;
#if MDC_EXP_STRIP_FAKE_GRAD  // diagnosis: the strip launch writes level 0's gradient images (traffic and shapes only), the gradient launch starts at level 1
    g_fake_grad_dI = with_gradients ? d_dI[0] + (size_t)f0 * w0 * h0 * 3 : nullptr;
    g_fake_grad_abs = with_gradients ? d_abs_squared_grad[0] + (size_t)f0 * w0 * h0 : nullptr;
#endif
    int rc = enqueue_process(c, d_in + (size_t)f0 * npi, base, n, flags, s, levels > 1 ? pyr : nullptr, &fused);
#if MDC_EXP_STRIP_FAKE_GRAD
    g_fake_grad_dI = g_fake_grad_abs = nullptr;
#endif
    if (rc != MDC_OK) return rc;
    if ((rc = enqueue_box_levels(c, base, lv, fused ? std::min(levels, 4) : 1, levels, w0, h0, n, s)) != MDC_OK) return rc;
#if MDC_EXP_STRIP_FAKE_GRAD
    constexpr int kGradFirst = 1;
#else
    constexpr int kGradFirst = 0;
#endif
    for (int l0 = kGradFirst; l0 < levels && with_gradients; l0 += 4) {  // gradients: four levels per launch
      const int nl = std::min(4, levels - l0);
      const float* gs[4];
      float *gd[4], *ga[4];
      for (int k = 0; k < nl; k++) {
        const int l = l0 + k;
        gs[k] = l == 0 ? base : lv[l - 1];
        gd[k] = d_dI[l] + (size_t)f0 * lw[l] * lh[l] * 3;
        ga[k] = d_abs_squared_grad[l] + (size_t)f0 * lw[l] * lh[l];
      }
      MDC_HIP(c, launch_gradients_levels(nl, gs, gd, ga, lw + l0, lh + l0, n, s));
    }
  }
  return MDC_OK;
}

}  // namespace mdc

using namespace mdc;

extern "C" {

int mdc_pyramid_batch_device(mdc_ctx* c, const float* d_base, int w, int h, int levels, float* const* d_levels,
                             int64_t nframes, void* stream) try {
  if (!c) return MDC_ERR_ARG;
  if (!d_base || w <= 0 || h <= 0 || levels < 1 || nframes < 0 || (levels > 1 && !d_levels))
    return fail(c, MDC_ERR_ARG, "mdc_pyramid_batch_device: bad argument");
  for (int l = 1; l < levels; l++)  // before anything is enqueued
    if (!d_levels[l - 1]) return fail(c, MDC_ERR_ARG, "level %d buffer is NULL", l);
  if (int rc = check_pyramid_levels(c, w, h, levels)) return rc;
  ReadLock lk(c->mu);
  DeviceGuard dg(c->device);
  return enqueue_box_levels(c, d_base, d_levels, 1, levels, w, h, nframes, (hipStream_t)stream);
} MDC_CATCH(c)

int mdc_process_pyramid_batch_device(mdc_ctx* c, const uint8_t* d_in, float* d_base, int levels, float* const* d_levels,
                                     int64_t nframes, unsigned flags, void* stream) try {
  if (!c) return MDC_ERR_ARG;
  if (!d_in || !d_base || nframes < 0 || levels < 1 || (levels > 1 && !d_levels))
    return fail(c, MDC_ERR_ARG, "mdc_process_pyramid_batch_device: bad argument");
  for (int l = 1; l < levels; l++)
    if (!d_levels[l - 1]) return fail(c, MDC_ERR_ARG, "level %d buffer is NULL", l);
  ReadLock lk(c->mu);
  DeviceGuard dg(c->device);
  hipStream_t s = (hipStream_t)stream;
  const FrameSize fs = frame_size(c, (flags & MDC_RECTIFY) != 0);
  if (fs.w > 0 && fs.h > 0)  // (an unknown frame size is enqueue_process's to refuse)
    if (int rc = check_pyramid_levels(c, fs.w, fs.h, levels)) return rc;
  float* pyr[3] = {levels > 1 ? d_levels[0] : nullptr, levels > 2 ? d_levels[1] : nullptr, levels > 3 ? d_levels[2] : nullptr};
  bool fused = false;
  int rc = enqueue_process(c, d_in, d_base, nframes, flags, s, levels > 1 ? pyr : nullptr, &fused);
  if (rc != MDC_OK) return rc;
  // levels the launch did not write (no fused path for this geometry, or more than 4 levels)
  return enqueue_box_levels(c, d_base, d_levels, fused ? std::min(levels, 4) : 1, levels, fs.w, fs.h, nframes, s);
} MDC_CATCH(c)

int mdc_gradients_batch_device(mdc_ctx* c, const float* d_level, int w, int h, float* d_dI, float* d_abs_squared_grad,
                               int64_t nframes, void* stream) try {
  if (!c) return MDC_ERR_ARG;
  if (!d_level || !d_dI || !d_abs_squared_grad || w < 1 || h < 1 || nframes < 0 || (int64_t)w * h >= (1ll << 31))
    return fail(c, MDC_ERR_ARG, "mdc_gradients_batch_device: bad argument");
  ReadLock lk(c->mu);
  DeviceGuard dg(c->device);
  MDC_HIP(c, launch_gradients(d_level, d_dI, d_abs_squared_grad, w, h, nframes, (hipStream_t)stream));
  return MDC_OK;
} MDC_CATCH(c)

int mdc_process_pyramid_gradients_batch_device(mdc_ctx* c, const uint8_t* d_in, float* d_base, int levels, float* const* d_levels,
                                               float* const* d_dI, float* const* d_abs_squared_grad, int64_t nframes, unsigned flags,
                                               int chunk_frames, void* stream) try {
  if (!c) return MDC_ERR_ARG;
  if (!d_in || !d_base || nframes < 0 || levels < 1 || levels > 8 || (levels > 1 && !d_levels) || !d_dI || !d_abs_squared_grad || chunk_frames < 0)
    return fail(c, MDC_ERR_ARG, "mdc_process_pyramid_gradients_batch_device: bad argument");
  for (int l = 0; l < levels; l++)
    if ((l && !d_levels[l - 1]) || !d_dI[l] || !d_abs_squared_grad[l]) return fail(c, MDC_ERR_ARG, "level %d has a NULL buffer", l);
  ReadLock lk(c->mu);
  DeviceGuard dg(c->device);
  return enqueue_pyramid_gradients(c, d_in, d_base, levels, d_levels, d_dI, d_abs_squared_grad, nframes, flags, chunk_frames, (hipStream_t)stream);
} MDC_CATCH(c)

}  // extern "C"
