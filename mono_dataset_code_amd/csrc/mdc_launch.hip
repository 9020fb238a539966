// The fused pass over device frames: which kernel of mdc_kernels.hip a call runs (choose_launch: the one place that decides
// it, for the launch itself and for mdc_describe_launch), with how many frames per workgroup, in which chunks -- and the
// C entry points that are that pass and nothing else: mdc_unmap_batch_device, mdc_process_batch_device,
// mdc_undistort_batch_device_f32, mdc_distort_points_device, mdc_describe_launch, mdc_tune_device.
#include "mdc_ctx.h"

namespace mdc {
namespace {

int frames_per_block(const mdc_ctx* c, int64_t nframes, int blocks_per_group, int target_wgs = 4800) {
  if (c->opt_fpb > 0) return (int)std::min<int64_t>(c->opt_fpb, std::max<int64_t>(nframes, 1));
  // enough workgroups to fill 256 CUs several times over (tail), yet >= 8 frames per
  // workgroup so the per-workgroup table reads stay amortised
  int64_t groups = std::max<int64_t>(1, (target_wgs + blocks_per_group - 1) / std::max(1, blocks_per_group));
  groups = std::min<int64_t>(groups, std::max<int64_t>(1, nframes / 8));
  int64_t fpb = (nframes + groups - 1) / groups;
  // few, large tiles (128 x 32: 80 blocks per frame group): not below 32 frames per workgroup as long as
  // that still leaves >= 2048 workgroups -- the per-workgroup prologue costs about two frames' time
  if (fpb < 32 && (int64_t)blocks_per_group * ((nframes + 31) / 32) >= 2048) fpb = 32;
  // ... and not above 64: workgroups that live for hundreds of frames drift apart and fall into lockstep phases
  // (a 50,000-frame launch with 1563 frames per workgroup ran 20 % slower per frame than with 32..64)
  if (target_wgs == 4800 && fpb > 64) fpb = 64;
  return (int)fpb;
}

TilePlan tile_plan(const mdc_ctx* c, int which) {
  const mdc_ctx::SrcPlan& pl = c->plan[which];
  return TilePlan{pl.d_chunks, pl.d_nch, pl.d_taps, pl.d_order, pl.n_blocks, pl.n_tiles, pl.tiles_x, pl.tile_w, pl.tile_h,
                  pl.chunk_cap, pl.win_bytes, pl.nbuf, c->n_black > 0, c->opt_interleave != 0, c->opt_taper != 2, c->opt_xcd_rotate != 0};
}

RemapArgs remap_args(const mdc_ctx* c, const float* lut, const float* vinv) {
  RemapArgs a;
  a.lut = lut;
  a.vinv = vinv;
  a.rx = c->d_rx;
  a.ry = c->d_ry;
  a.in_w = c->rm_in_w;
  a.in_h = c->rm_in_h;
  a.out_w = c->out_w;
  a.out_h = c->out_h;
  return a;
}

// Which remap kernel a rectifying launch runs, and whether that launch writes levels 1..3 of the box pyramid itself.
struct LaunchChoice {
  enum Path { kStrip, kTiled, kGather } path;
  bool fuse_pyr;
};
// f32: float frames (undistort<float>: its own plan, never a pyramid); aligned: the frames start on a 16-byte boundary (the
// LDS-staged kernels load 16-byte chunks); want_pyr: the caller has buffers for levels 1..3.  MDC_KERNEL_TILED is not looked at
// here: the strip kernel, where planned, comes first either way, and what the selector means without a plan is the caller's
// (enqueue_process refuses the call, mdc_describe_launch names the gather kernel).
LaunchChoice choose_launch(const mdc_ctx* c, bool f32, bool aligned, bool want_pyr) {
  const bool staged = aligned && c->opt_kernel != MDC_KERNEL_GATHER;
  if (f32) return {c->plan[1].tiled && staged ? LaunchChoice::kTiled : LaunchChoice::kGather, false};
  if (c->strip.planned && staged)  // wave-private strips (scale >= ~1 remaps)
    return {LaunchChoice::kStrip, want_pyr && c->out_w % kStripTileW == 0};
  if (c->plan[0].tiled && staged) {
    const mdc_ctx::SrcPlan& p = c->plan[0];
    // the fused pyramid adds level-2 hand-over rows to the workgroup's LDS: without room for them the
    // per-level passes run instead
    return {LaunchChoice::kTiled, want_pyr && p.tile_w * p.tile_h <= 2048 && p.tile_h % 8 == 0 && c->out_w % p.tile_w == 0 && c->out_h % p.tile_h == 0 &&
                                      tiled_lds_bytes(p.win_bytes, p.nbuf, true) + tiled_pyramid_lds_bytes(p.tile_w, p.tile_h) <= kLdsPerCU};
  }
  return {LaunchChoice::kGather, false};
}

int64_t strip_resident(bool pyr) { return 256 * (pyr ? 4 : 5); }  // workgroups of kStripWaves waves the chip holds at once
int64_t chunk_groups(const mdc_ctx* c, bool pyr) {
  const int64_t nb = std::max(1, c->strip.n_blocks);
  return std::max<int64_t>(1, (strip_resident(pyr) * 5 / 8 + nb / 2) / nb);
}

}  // namespace

// Strip path, chunked launches with prefetch (enqueue_process): bytes of the source bounding box widened to whole 128-byte
// lines, and the frames per chunk.  48 frames of the bench camera (0.65 MB of box each) measured best -- beyond ~64 frames
// the prefetched lines no longer survive until they are used (the launch's own output passes through the same cache).
int64_t prefetch_box_bytes(const mdc_ctx* c) {
  const int x0 = c->bbox[0], x1 = c->bbox[2], y0 = c->bbox[1], y1 = c->bbox[3];
  return y1 >= y0 ? (int64_t)(y1 - y0 + 1) * std::min(c->rm_in_w, ((x1 + 128) & ~127) - (x0 & ~127)) : 0;
}
// Two streams (MDC_OPT_PREFETCH_STREAMS, the default): the chunks alternate between the caller's stream and a second
// one, so a chunk's tail and the next prefetch run under the other chunk's launch; a launch then holds ~5/8 of the
// workgroups the chip has room for (two of them overlap, staggered), in whole frame groups.  Measured on config 5
// (profiles/r03_experiments/10_*): 40 frames per chunk, 2 groups of 20 -- 1.76 -> 1.52 ms per 1024 frames.
int prefetch_streams(const mdc_ctx* c) { return c->opt_prefetch_streams == 1 ? 1 : 2; }
int64_t prefetch_chunk_frames(const mdc_ctx* c, bool pyr) {
  if (c->opt_prefetch_chunk > 0) return c->opt_prefetch_chunk;
  const int64_t box = std::max<int64_t>(1, prefetch_box_bytes(c));
  if (prefetch_streams(c) == 1) return std::max<int64_t>(16, (31ll << 20) / box);
  const int64_t g = chunk_groups(c, pyr);
  const int64_t per_group = std::max<int64_t>(8, ((26ll << 20) / box + g / 2) / g);  // >= 8 frames per workgroup
  return g * per_group;
}

// UndistorterFOV::undistort<float> over float frames: LDS-tiled kernel when planned, else the gather kernel.
int enqueue_undistort_f32(mdc_ctx* c, const float* d_in, float* d_out, int64_t nframes, hipStream_t s) {
  RemapArgs a = remap_args(c, nullptr, nullptr);
  const bool aligned = (reinterpret_cast<uintptr_t>(d_in) & 15) == 0;
  if (choose_launch(c, true, aligned, false).path == LaunchChoice::kTiled) {
    const int fpb = frames_per_block(c, nframes, c->plan[1].n_blocks);
    MDC_HIP(c, launch_remap_tiled_f32(d_in, d_out, a, tile_plan(c, 1), nframes, fpb, s));
  } else {
    const int fpb = frames_per_block(c, nframes, (c->out_w * c->out_h + 255) / 256);
    MDC_HIP(c, launch_remap_gather_f32(d_in, d_out, a, nframes, fpb, s));
  }
  return MDC_OK;
}

// Enqueue the fused / photometric-only pipeline on `s`.  Lock held by caller.
// pyr (optional): levels 1..3 of the box pyramid; *pyr_done tells whether the launch wrote them.
int enqueue_process(mdc_ctx* c, const uint8_t* d_in, float* d_out, int64_t nframes, unsigned flags, hipStream_t s,
                    float* const* pyr, bool* pyr_done) {
  if (pyr_done) *pyr_done = false;
  bool g, v, o;
  normalise(c, flags, g, v, o);
  const float* lut = lut_for(c, g, o);
  const float* vinv = v ? c->d_vinv : nullptr;
  if (!(flags & MDC_RECTIFY)) {
    const FrameSize fs = frame_size(c, false);
    if (fs.w <= 0 || fs.h <= 0) return fail(c, MDC_ERR_STATE, "frame size unknown: set the photometric tables or a remap first");
    const int64_t npix = (int64_t)fs.w * fs.h;
    int fpb = frames_per_block(c, nframes, (int)((npix + 4095) / 4096), 20000);  // measured best at 8 frames per workgroup,
    if (!c->opt_fpb) fpb = std::min(fpb, 8);                                       // also for launches of thousands of frames
    MDC_HIP(c, launch_unmap(d_in, d_out, lut, vinv, npix, nframes, fpb, s));
    return MDC_OK;
  }
  if (!c->valid_remap) return fail(c, MDC_ERR_STATE, "no remap set (UndistorterFOV invalid)");
  if (vinv && (c->in_w != c->rm_in_w || c->in_h != c->rm_in_h))
    return fail(c, MDC_ERR_SIZE, "vignette is %dx%d but the remap expects %dx%d input", c->in_w, c->in_h, c->rm_in_w,
                c->rm_in_h);
  RemapArgs a = remap_args(c, lut, vinv);
  const LaunchChoice choice = choose_launch(c, false, (reinterpret_cast<uintptr_t>(d_in) & 15) == 0, pyr != nullptr);
  const bool fuse_pyr = choice.fuse_pyr;
  if (choice.path == LaunchChoice::kStrip) {
    const mdc_ctx::Strip& st = c->strip;
    const StripPlan sp{st.d_chunks, st.d_nch, st.d_taps, st.d_order, st.n_blocks, st.n_tiles, st.tiles_x, st.win_bytes, st.passes, st.nbuf,
                       c->opt_interleave != 0, c->opt_xcd_rotate == 2};
    // Large batches go in chunks, each preceded by a linear prefetch of the NEXT chunk's source rows into the Infinity
    // Cache (launch_prefetch_rows): the strips' small window reads then hit the cache instead of interrupting the output
    // stream in HBM.  Chunk = as many frames as keep the prefetched rows (bounding box rows x frame width) within ~96 MiB.
    const int iw = c->rm_in_w;
    const int x0 = c->bbox[0], x1 = c->bbox[2], y0 = c->bbox[1], y1 = c->bbox[3];
    const int64_t frame_in = (int64_t)iw * c->rm_in_h;
    const int64_t box_bytes = prefetch_box_bytes(c);
    int64_t chunk = prefetch_chunk_frames(c, fuse_pyr);
    // Measured (profiles/r03_experiments/08_*, 10_*), ms per 1024 frames of config 5: with the fused pyramid one launch 1.86-1.94,
    // chunks on one stream 1.64-1.70, over two streams 1.47-1.52; without the levels 1.62 / 1.55-1.65 / 1.29.
    const bool prefetch = c->opt_prefetch_chunk >= 0 && (fuse_pyr || c->opt_prefetch_chunk > 0 || prefetch_streams(c) == 2) && box_bytes >= 4096 &&
                          nframes >= 2 * chunk;
    if (!prefetch) chunk = nframes;
    const size_t no = (size_t)c->out_w * c->out_h;
    const int64_t resident = strip_resident(fuse_pyr);
    auto strip = [&](int64_t f0, int64_t n, int fpb, hipStream_t t) {
      return launch_remap_strip_u8(d_in + (size_t)f0 * frame_in, d_out + (size_t)f0 * no, a, sp, n, fpb, t,
                                   fuse_pyr ? pyr[0] + (size_t)f0 * (no / 4) : nullptr, fuse_pyr ? pyr[1] + (size_t)f0 * (no / 16) : nullptr,
                                   fuse_pyr ? pyr[2] + (size_t)f0 * (no / 64) : nullptr);
    };
    hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &capturing) != hipSuccess) {
      (void)hipGetLastError();
      capturing = hipStreamCaptureStatusNone;
    }
    if (prefetch && prefetch_streams(c) == 2 && capturing == hipStreamCaptureStatusNone) {
      // The second stream is a slot's (with its two events), borrowed while the launches are enqueued: what is queued on it
      // stays ordered after the lease ends.  No free slot (every one held by a host call): one stream.  A caller's stream
      // that is being captured into a graph keeps everything on itself (a shared stream must not be drawn into a capture).
      SlotLease side(c, false);
      side.drained();  // a *_device call stays asynchronous: the lease only covers the enqueueing
      mdc_ctx::HostSlot* h = side.s;
      if (h && !h->ev_fork) {
        if (hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming) != hipSuccess) h->ev_fork = nullptr;
        if (h->ev_fork && hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming) != hipSuccess) {
          (void)hipEventDestroy(h->ev_fork);
          h->ev_fork = nullptr;
        }
      }
      if (h && h->ev_fork) {
        const int64_t groups = chunk_groups(c, fuse_pyr);
        MDC_HIP(c, hipEventRecord(h->ev_fork, s));
        MDC_HIP(c, hipStreamWaitEvent(h->stream, h->ev_fork, 0));
        // whatever happens below, the caller's stream waits for what reached the second one
        hipError_t e = hipSuccess;
        int k = 0;
        for (int64_t f0 = 0; f0 < nframes && e == hipSuccess; f0 += chunk, k++) {
          const int64_t n = std::min<int64_t>(chunk, nframes - f0);
          hipStream_t t = (k & 1) ? h->stream : s;
          e = launch_prefetch_rows(d_in + (size_t)f0 * frame_in, frame_in, iw, x0, x1, y0, y1, n, c->d_vcal_max, t);
          const int fpb = c->opt_fpb > 0 ? (int)std::min<int64_t>(c->opt_fpb, n) : (int)((n + groups - 1) / groups);
          if (e == hipSuccess) e = strip(f0, n, fpb, t);
        }
        const hipError_t ej = hipEventRecord(h->ev_join, h->stream);
        const hipError_t ew = ej == hipSuccess ? hipStreamWaitEvent(s, h->ev_join, 0) : ej;
        MDC_HIP(c, e);
        MDC_HIP(c, ew);
        if (pyr_done) *pyr_done = fuse_pyr;
        return MDC_OK;
      }
    }
    if (prefetch) MDC_HIP(c, launch_prefetch_rows(d_in, frame_in, iw, x0, x1, y0, y1, std::min<int64_t>(chunk, nframes), c->d_vcal_max, s));
    for (int64_t f0 = 0; f0 < nframes; f0 += chunk) {
      const int64_t n = std::min<int64_t>(chunk, nframes - f0);
      if (prefetch && f0 + chunk < nframes)
        MDC_HIP(c, launch_prefetch_rows(d_in + (size_t)(f0 + chunk) * frame_in, frame_in, iw, x0, x1, y0, y1, std::min<int64_t>(chunk, nframes - f0 - chunk),
                                        c->d_vcal_max, s));
      // one round of workgroups per chunk where that is possible: a chunk is a launch of its own, its tail is not hidden
      int fpb = frames_per_block(c, n, st.n_blocks);
      if (prefetch && !c->opt_fpb) fpb = (int)std::max<int64_t>(8, (n * st.n_blocks + resident - 1) / resident);
      MDC_HIP(c, strip(f0, n, fpb, s));
    }
    if (pyr_done) *pyr_done = fuse_pyr;
    return MDC_OK;
  }
  if (choice.path == LaunchChoice::kTiled) {
    const TilePlan p = tile_plan(c, 0);
    int fpb = frames_per_block(c, nframes, p.n_blocks);
    // a measured pick (mdc_tune_device) belongs to this plan and to batches of the size it was measured on: small
    // launches (undistort<uchar>, the 16-frame chunks of mdc_process_frames_host) and the unmap path keep their own rule
    if (!c->opt_fpb && c->tuned_fpb > 0 && nframes >= c->tuned_min_frames) fpb = (int)std::min<int64_t>(c->tuned_fpb, nframes);
    MDC_HIP(c, launch_remap_tiled_u8(d_in, d_out, a, p, nframes, fpb, s, fuse_pyr ? pyr[0] : nullptr,
                                     fuse_pyr ? pyr[1] : nullptr, fuse_pyr ? pyr[2] : nullptr));
    if (pyr_done) *pyr_done = fuse_pyr;
  } else {
    if (c->opt_kernel == MDC_KERNEL_TILED)
      return fail(c, MDC_ERR_STATE, "tiled kernel requested but not plannable for this remap / alignment");
    const int fpb = frames_per_block(c, nframes, (c->out_w * c->out_h + 255) / 256);
    MDC_HIP(c, launch_remap_gather_u8(d_in, d_out, a, nframes, fpb, s));
  }
  return MDC_OK;
}

}  // namespace mdc

using namespace mdc;

extern "C" {

int mdc_unmap_batch_device(mdc_ctx* c, const uint8_t* d_in, float* d_out, int64_t nframes, unsigned flags, void* stream) try {
  if (!c) return MDC_ERR_ARG;
  if (!d_in || !d_out || nframes < 0) return fail(c, MDC_ERR_ARG, "mdc_unmap_batch_device: bad argument");
  ReadLock lk(c->mu);
  DeviceGuard dg(c->device);
  return enqueue_process(c, d_in, d_out, nframes, flags & ~MDC_RECTIFY, (hipStream_t)stream);
} MDC_CATCH(c)

int mdc_process_batch_device(mdc_ctx* c, const uint8_t* d_in, float* d_out, int64_t nframes, unsigned flags, void* stream) try {
  if (!c) return MDC_ERR_ARG;
  if (!d_in || !d_out || nframes < 0) return fail(c, MDC_ERR_ARG, "mdc_process_batch_device: bad argument");
  ReadLock lk(c->mu);
  DeviceGuard dg(c->device);
  return enqueue_process(c, d_in, d_out, nframes, flags, (hipStream_t)stream);
} MDC_CATCH(c)

int mdc_undistort_batch_device_f32(mdc_ctx* c, const float* d_in, float* d_out, int64_t nframes, void* stream) try {
  if (!c) return MDC_ERR_ARG;
  if (!d_in || !d_out || nframes < 0) return fail(c, MDC_ERR_ARG, "mdc_undistort_batch_device_f32: bad argument");
  ReadLock lk(c->mu);
  DeviceGuard dg(c->device);
  if (!c->valid_remap) return fail(c, MDC_ERR_STATE, "no remap set (UndistorterFOV invalid)");
  return enqueue_undistort_f32(c, d_in, d_out, nframes, (hipStream_t)stream);
} MDC_CATCH(c)

int mdc_distort_points_device(mdc_ctx* c, const mdc_fov_model* model, float* d_x, float* d_y, int64_t n, void* stream) try {
  if (!c) return MDC_ERR_ARG;
  if (!model || n < 0 || (n > 0 && (!d_x || !d_y))) return fail(c, MDC_ERR_ARG, "mdc_distort_points_device: bad argument");
  ReadLock lk(c->mu);
  DeviceGuard dg(c->device);
  MDC_HIP(c, launch_distort_points(d_x, d_y, n, distort_model(model), (hipStream_t)stream));
  return MDC_OK;
} MDC_CATCH(c)

// The name of the kernel instantiation choose_launch picks for frames on a 16-byte boundary; pyramid_levels == -1: float frames
int mdc_describe_launch(mdc_ctx* c, unsigned flags, int pyramid_levels, char* buf, size_t cap) try {
  if (!c || !buf || cap == 0) return MDC_ERR_ARG;
  ReadLock lk(c->mu);
  bool g, v, o;
  normalise(c, flags, g, v, o);
  const bool f32 = pyramid_levels == -1;  // undistort<float> (mdc_undistort_batch_device_f32): its own plan, no LUT, no vignette
  const char* const vig = v && !f32 ? "true" : "false";
  const char* const black = c->n_black > 0 ? "true" : "false";
  char tmp[160];
  if (!f32 && !(flags & MDC_RECTIFY)) {
    const FrameSize fs = frame_size(c, false);
    snprintf(tmp, sizeof tmp, "%s<%s>", ((int64_t)fs.w * fs.h) % 4 == 0 ? "unmap_xpose_kernel" : "unmap_scalar_kernel", vig);
  } else if (!c->valid_remap) {
    return fail(c, MDC_ERR_STATE, "no remap set (UndistorterFOV invalid)");
  } else {
    const LaunchChoice choice = choose_launch(c, f32, true, pyramid_levels > 1);
    const char* const pyr = choice.fuse_pyr ? "true" : "false";
    const mdc_ctx::SrcPlan& p = c->plan[f32 ? 1 : 0];
    if (choice.path == LaunchChoice::kStrip)
      snprintf(tmp, sizeof tmp, "remap_strip_kernel<%s, %s, %d, %d, %d>", vig, pyr, c->strip.nbuf, c->strip.passes, kStripWaves);
    else if (choice.path == LaunchChoice::kTiled)
      snprintf(tmp, sizeof tmp, "remap_tiled_kernel<%s, %s, %s, %s, %d, %d, %d>", vig, black, pyr, f32 ? "true" : "false", p.tile_w,
               tile_threads(p.tile_w, p.tile_h), p.nbuf);
    else if (f32) snprintf(tmp, sizeof tmp, "remap_gather_f32_kernel");
    else snprintf(tmp, sizeof tmp, "remap_gather_u8_kernel<%s>", vig);
  }
  if (strlen(tmp) + 1 > cap) return fail(c, MDC_ERR_ARG, "mdc_describe_launch: buffer too small");
  memcpy(buf, tmp, strlen(tmp) + 1);
  return MDC_OK;
} MDC_CATCH(c)

// Plan selection by measurement (as FFT / BLAS libraries do): which tile shape and workgroup length is fastest depends on
// the remap (window sizes) and, by a few per cent, on the individual GPU.  Runs the fused pass over the caller's
// batch with every candidate, keeps the fastest as the context's plan.
int mdc_tune_device(mdc_ctx* c, const uint8_t* d_in, float* d_out, int64_t nframes, unsigned flags, void* stream,
                    mdc_tune_result* result) try {
  if (!c) return MDC_ERR_ARG;
  if (!d_in || !d_out || nframes <= 0) return fail(c, MDC_ERR_ARG, "mdc_tune_device: bad argument");
  WriteLock lk(c->mu);
  DeviceGuard dg(c->device);
  if (!(flags & MDC_RECTIFY) || !c->valid_remap) return fail(c, MDC_ERR_STATE, "mdc_tune_device: needs a remap and MDC_RECTIFY");
  hipStream_t s = (hipStream_t)stream;
  static const TileShape shapes[] = {{128, 16}, {64, 32}, {128, 32}};
  static const int fpbs[] = {32, 64, 96, 128};  // (with the tapered tail the longer workgroups pay: 96 measured 1.8 % ahead of 64)
  hipEvent_t e0, e1;
  MDC_HIP(c, hipEventCreate(&e0));
  MDC_HIP(c, hipEventCreate(&e1));
  float best = 1e30f;
  int bw = 0, bh = 0, bf = 0, tried = 0;
  int rc = MDC_OK;
  const int caller_fpb = c->opt_fpb;  // the caller's own override is restored afterwards: the pick goes into tuned_fpb
  for (const TileShape& sh : shapes) {
    c->opt_tile_w = sh.w;
    c->opt_tile_h = sh.h;
    // re-planning frees the plan tables: like every setter that re-plans, wait for the WHOLE device -- kernels that
    // other threads put on other streams through the *_device entry points may still be reading them
    if (hipDeviceSynchronize() != hipSuccess) {
      rc = fail(c, MDC_ERR_HIP, "mdc_tune_device: hipDeviceSynchronize failed");
      break;
    }
    if ((rc = plan_tiles(c)) != MDC_OK) break;
    if (!c->plan[0].tiled) continue;
    for (int fpb : fpbs) {
      c->opt_fpb = fpb;
      float ms[5];
      bool ok = true;
      for (int k = 0; k < 7 && ok; k++) {  // 2 warm-up launches, 5 timed
        if (k >= 2) ok = hipEventRecord(e0, s) == hipSuccess;
        ok = ok && enqueue_process(c, d_in, d_out, nframes, flags, s) == MDC_OK;
        if (k >= 2) ok = ok && hipEventRecord(e1, s) == hipSuccess && hipEventSynchronize(e1) == hipSuccess &&
                         hipEventElapsedTime(&ms[k - 2], e0, e1) == hipSuccess;
      }
      if (!ok) continue;
      std::sort(ms, ms + 5);
      tried++;
      if (ms[2] < best) {
        best = ms[2];
        bw = sh.w;
        bh = sh.h;
        bf = fpb;
      }
    }
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  (void)hipDeviceSynchronize();
  // the winner (or, if nothing could be timed, the automatic choice) becomes the plan
  c->opt_tile_w = bw;
  c->opt_tile_h = bh;
  c->opt_fpb = caller_fpb;
  c->tuned_fpb = bf;
  c->tuned_min_frames = bf ? std::max<int64_t>(nframes / 4, (int64_t)bf * 8) : 0;
  const int rc2 = plan_tiles(c);
  if (rc == MDC_OK) rc = rc2;
  if (result) {
    result->tile_w = bw;
    result->tile_h = bh;
    result->frames_per_block = bf;
    result->ms = tried ? best : 0.f;
    result->candidates = tried;
  }
  return rc;
} MDC_CATCH(c)

}  // extern "C"
