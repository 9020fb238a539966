// lens_points_shell.h -- what libmdc_lens.so (mdc_lens.hip, rectified -> raw) and libmdc_lensinv.so (mdc_lensinv.hip, raw ->
// rectified) have in common: everything but the arithmetic.  The two kernels, the launch loop that cuts a call at 2^31 points, the
// host-pointer call, the table call, the argument checks and the dispatch over kinds, once, over a traits struct per direction:
//
//   Model, Public          the kernels' model (mdc::LensModel / mdc::LensInverseModel) and the header's (mdcn_model / mdcu_model)
//   kKinds                 kinds 0 .. kKinds - 1 are valid: 0 pinhole, 1 RadTan, 2 EquiDistant in both directions, 3 FOV in the inverse
//   point<KIND>(m, x, y)   the direction's point function of lens_point_model.h / lens_inverse_model.h
//   derive(d, m)           what Model holds beyond Public's fields (the inverse's d2t)
//   check_more(who, m)     the direction's model checks after the common ones
//   kTableOverInput        the table has one entry per pixel of the input image, tested against the rectified image's border
//                          (the inverse), or one per rectified pixel, tested against the input image's (the forward direction)
//   kPointsDevice, kPointsHost, kTableDevice   the entry points' names, for the messages
//
// Both kernels are streaming: one point (one table entry) per thread, dword loads and stores that a wave coalesces into 256-byte
// runs whatever the arrays' alignment, no LDS, the model in the kernel arguments (scalar registers).  The kind is a template
// argument down to the point function: nothing in a kernel branches on it.  Each library is one translation unit and includes this
// once; everything is in its unnamed namespace.
#ifndef MDC_LENS_POINTS_SHELL_H
#define MDC_LENS_POINTS_SHELL_H

#include <math.h>
#include <string.h>

#include <type_traits>

#include "codec_host.h"
#include "lens_point_model.h"

namespace {

constexpr int kThreads = 256;
// HIP caps a launch at 2^32 - 1 threads per dimension: 2^23 blocks of 256 = 2^31 points per launch, the rest in further launches.
constexpr int64_t kBlocksPerLaunch = (int64_t)1 << 23;

template <class T, int KIND>
__global__ __launch_bounds__(kThreads) void points_kernel(typename T::Model m, float* __restrict__ xs, float* __restrict__ ys, int64_t first, int64_t n) {
  const int64_t i = first + (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  float x = xs[i], y = ys[i];
  T::template point<KIND>(m, x, y);
  xs[i] = x;
  ys[i] = y;
}

struct Border {
  int in_w, in_h, out_w, out_h;
  float lo, hi_x, hi_y;
};

template <class T, int KIND>
__global__ __launch_bounds__(kThreads) void table_kernel(typename T::Model m, Border b, float* __restrict__ tx, float* __restrict__ ty, int* __restrict__ flag) {
  const int w = T::kTableOverInput ? b.in_w : b.out_w, h = T::kTableOverInput ? b.in_h : b.out_h;
  const int i = blockIdx.x * kThreads + threadIdx.x;  // w * h < 2^31
  if (i >= w * h) return;
  float x = (float)(i % w), y = (float)(i / w);
  T::template point<KIND>(m, x, y);
  const bool went_out = mdc::lens_border_rule(x, y, T::kTableOverInput ? b.out_w : b.in_w, T::kTableOverInput ? b.out_h : b.in_h, b.lo, b.hi_x, b.hi_y);
  tx[i] = x;
  ty[i] = y;
  if (went_out) *flag = 1;  // every writer stores the same value
}

// f(std::integral_constant<int, kind>()) for a kind that check_model has passed
template <class T, class F>
int for_kind(int kind, F f) {
  switch (kind) {
    case 1: return f(std::integral_constant<int, 1>());
    case 2: return f(std::integral_constant<int, 2>());
    case 3:
      if constexpr (T::kKinds > 3) return f(std::integral_constant<int, 3>());
  }
  return f(std::integral_constant<int, 0>());
}

template <class T>
int check_model(const char* who, const typename T::Public* m) {
  if (!m) return fail(kErrArg, "%s: null model", who);
  if (m->kind < 0 || m->kind >= T::kKinds) return fail(kErrArg, "%s: kind %d is no lens model", who, m->kind);
  if (!isfinite(m->ofx) || !isfinite(m->ofy) || m->ofx == 0 || m->ofy == 0)
    return fail(kErrArg, "%s: rectified focal lengths %g %g (finite and not 0)", who, (double)m->ofx, (double)m->ofy);
  return T::check_more(who, m);
}

template <class T>
typename T::Model device_model(const typename T::Public* m) {
  typename T::Model d;
  d.fx = m->fx;
  d.fy = m->fy;
  d.cx = m->cx;
  d.cy = m->cy;
  for (int i = 0; i < 4; i++) d.k[i] = m->k[i];
  d.ofx = m->ofx;
  d.ofy = m->ofy;
  d.ocx = m->ocx;
  d.ocy = m->ocy;
  T::derive(d, *m);
  return d;
}

// n > 0 points of a checked model, in place, enqueued on s
template <class T>
int launch_points(const typename T::Public* model, float* d_x, float* d_y, int64_t n, hipStream_t s) {
  const typename T::Model d = device_model<T>(model);
  return for_kind<T>(model->kind, [&](auto kind) {
    for (int64_t first = 0; first < n; first += kBlocksPerLaunch * kThreads) {
      const int64_t left = n - first;
      const int64_t blocks = left >= kBlocksPerLaunch * kThreads ? kBlocksPerLaunch : (left + kThreads - 1) / kThreads;
      points_kernel<T, decltype(kind)::value><<<dim3((unsigned)blocks), dim3(kThreads), 0, s>>>(d, d_x, d_y, first, n);
      const hipError_t e = hipGetLastError();
      if (e != hipSuccess) return fail(kErrHip, "%s: launch failed: %s", T::kPointsDevice, hipGetErrorString(e));
    }
    return kOk;
  });
}

template <class T>
int points_device(const typename T::Public* model, float* d_x, float* d_y, int64_t n, void* stream) {
  const char* who = T::kPointsDevice;
  const int rc = check_model<T>(who, model);
  if (rc != kOk) return rc;
  if (n < 0) return fail(kErrArg, "%s: n = %lld", who, (long long)n);
  if (n == 0) return kOk;
  if (!d_x || !d_y) return fail(kErrArg, "%s: null coordinate array", who);
  return launch_points<T>(model, d_x, d_y, n, (hipStream_t)stream);
}

// Host arrays: a device buffer, a page-locked buffer for the way back and a stream of the call's own.  The caller's arrays are
// written last, from the page-locked buffer, so a call that fails leaves them untouched.
template <class T>
int points_host(int device, const typename T::Public* model, float* x, float* y, int64_t n) {
  const char* who = T::kPointsHost;
  int rc = check_model<T>(who, model);
  if (rc != kOk) return rc;
  if (n < 0) return fail(kErrArg, "%s: n = %lld", who, (long long)n);
  if (n == 0) return kOk;
  if (!x || !y) return fail(kErrArg, "%s: null coordinate array", who);
  if (n > ((int64_t)1 << 36)) return fail(kErrSize, "%s: %lld points (at most 2^36)", who, (long long)n);
  rc = resolve_device(who, &device);
  if (rc != kOk) return rc;
  DeviceGuard guard(device);
  const size_t bytes = (size_t)n * sizeof(float);
  float* d = nullptr;     // x then y
  float* back = nullptr;  // the results on the host before either array of the caller's is written
  hipStream_t s = nullptr;
  if (hipMalloc((void**)&d, 2 * bytes) != hipSuccess) {
    (void)hipGetLastError();
    return fail(kErrNoMem, "%s: no device memory for %lld points", who, (long long)n);
  }
  if (hipHostMalloc((void**)&back, 2 * bytes, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipFree(d);
    return fail(kErrNoMem, "%s: no page-locked memory for %lld points", who, (long long)n);
  }
  hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipMemcpyAsync(d, x, bytes, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(d + n, y, bytes, hipMemcpyHostToDevice, s);
  rc = kOk;
  if (e == hipSuccess) rc = launch_points<T>(model, d, d + n, n, s);
  if (e == hipSuccess && rc == kOk) e = hipMemcpyAsync(back, d, 2 * bytes, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && rc == kOk) e = hipStreamSynchronize(s);
  if (e != hipSuccess) rc = fail(kErrHip, "%s: %s", who, hipGetErrorString(e));
  if (rc == kOk) {
    memcpy(x, back, bytes);
    memcpy(y, back + n, bytes);
  }
  if (s) (void)hipStreamDestroy(s);
  (void)hipHostFree(back);
  (void)hipFree(d);
  return rc;
}

// The direction's table into device arrays; *d_flag (an int on the device) = 1 if the border rule sent any entry to (-1, -1)
template <class T>
int table_device(const typename T::Public* model, float* d_tx, float* d_ty, int* d_flag, void* stream) {
  const char* who = T::kTableDevice;
  const int rc = check_model<T>(who, model);
  if (rc != kOk) return rc;
  if (!d_tx || !d_ty || !d_flag) return fail(kErrArg, "%s: null output array", who);
  if (model->in_w < 1 || model->in_h < 1 || model->out_w < 1 || model->out_h < 1)
    return fail(kErrArg, "%s: sizes %d x %d -> %d x %d", who, model->in_w, model->in_h, model->out_w, model->out_h);
  const int w = T::kTableOverInput ? model->in_w : model->out_w, h = T::kTableOverInput ? model->in_h : model->out_h;
  const int border_w = T::kTableOverInput ? model->out_w : model->in_w, border_h = T::kTableOverInput ? model->out_h : model->in_h;
  const int64_t n = (int64_t)w * h;
  if (n >= ((int64_t)1 << 31)) return fail(kErrSize, "%s: %d x %d entries (fewer than 2^31)", who, w, h);
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(d_flag, 0, sizeof(int), s) != hipSuccess) return fail(kErrHip, "%s: hipMemsetAsync failed: %s", who, hipGetErrorString(hipGetLastError()));
  const typename T::Model d = device_model<T>(model);
  // the nudge constants are double expressions narrowed, as the host class writes them
  const Border b = {model->in_w, model->in_h, model->out_w, model->out_h, (float)0.01, (float)(border_w - 1.01), (float)(border_h - 1.01)};
  const dim3 grid((unsigned)((n + kThreads - 1) / kThreads)), block(kThreads);
  return for_kind<T>(model->kind, [&](auto kind) {
    table_kernel<T, decltype(kind)::value><<<grid, block, 0, s>>>(d, b, d_tx, d_ty, d_flag);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(kErrHip, "%s: launch failed: %s", who, hipGetErrorString(e));
    return kOk;
  });
}

}  // namespace

#endif  // MDC_LENS_POINTS_SHELL_H
