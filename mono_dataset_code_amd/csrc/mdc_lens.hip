// libmdc_lens.so (include/mdc_lens.h): the pinhole / RadTan / EquiDistant lens models on the device.  One translation unit over
// lens_point_model.h, the header the host class and the CPU test program share: built with -ffp-contract=off -fno-fast-math, so the
// kernels give the host's bits.
//
// Both kernels are streaming: one point (one table entry) per thread, dword loads and stores that a wave coalesces into 256-byte
// runs whatever the arrays' alignment, no LDS, the model in the kernel arguments (scalar registers).
#include "../../include/mdc_lens.h"

#include <math.h>

#include "codec_host.h"
#include "lens_point_model.h"

static_assert(MDCN_OK == kOk && MDCN_ERR_ARG == kErrArg && MDCN_ERR_SIZE == kErrSize && MDCN_ERR_HIP == kErrHip && MDCN_ERR_NO_DEVICE == kErrNoDevice &&
                  MDCN_ERR_NOMEM == kErrNoMem,
              "include/mdc_lens.h and codec_host.h name the same codes");
static_assert(MDCN_PINHOLE == mdc::LENS_PINHOLE && MDCN_RADTAN == mdc::LENS_RADTAN && MDCN_EQUIDISTANT == mdc::LENS_EQUIDISTANT,
              "include/mdc_lens.h and lens_point_model.h name the same kinds");

namespace {

constexpr int kThreads = 256;
// HIP caps a launch at 2^32 - 1 threads per dimension: 2^23 blocks of 256 = 2^31 points per launch, the rest in further launches.
constexpr int64_t kBlocksPerLaunch = (int64_t)1 << 23;

template <int KIND>
__global__ __launch_bounds__(kThreads) void distort_points_kernel(mdc::LensModel m, float* __restrict__ xs, float* __restrict__ ys, int64_t first, int64_t n) {
  const int64_t i = first + (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  float x = xs[i], y = ys[i];
  mdc::lens_distort_point<KIND>(m, x, y);
  xs[i] = x;
  ys[i] = y;
}

struct Border {
  int in_w, in_h, out_w, out_h;
  float lo, hi_x, hi_y;
};

template <int KIND>
__global__ __launch_bounds__(kThreads) void remap_kernel(mdc::LensModel m, Border b, float* __restrict__ rx, float* __restrict__ ry, int* __restrict__ black) {
  const int i = blockIdx.x * kThreads + threadIdx.x;  // out_w * out_h < 2^31
  if (i >= b.out_w * b.out_h) return;
  float x = (float)(i % b.out_w), y = (float)(i / b.out_w);
  mdc::lens_distort_point<KIND>(m, x, y);
  const bool went_black = mdc::lens_border_rule(x, y, b.in_w, b.in_h, b.lo, b.hi_x, b.hi_y);
  rx[i] = x;
  ry[i] = y;
  if (went_black) *black = 1;  // every writer stores the same value
}

int check_model(const char* who, const mdcn_model* m) {
  if (!m) return fail(kErrArg, "%s: null model", who);
  if (m->kind != MDCN_PINHOLE && m->kind != MDCN_RADTAN && m->kind != MDCN_EQUIDISTANT) return fail(kErrArg, "%s: kind %d is no lens model", who, m->kind);
  if (!isfinite(m->ofx) || !isfinite(m->ofy) || m->ofx == 0 || m->ofy == 0)
    return fail(kErrArg, "%s: rectified focal lengths %g %g (finite and not 0)", who, (double)m->ofx, (double)m->ofy);
  return kOk;
}

mdc::LensModel device_model(const mdcn_model* m) {
  mdc::LensModel d;
  d.fx = m->fx;
  d.fy = m->fy;
  d.cx = m->cx;
  d.cy = m->cy;
  for (int i = 0; i < 4; i++) d.k[i] = m->k[i];
  d.ofx = m->ofx;
  d.ofy = m->ofy;
  d.ocx = m->ocx;
  d.ocy = m->ocy;
  return d;
}

template <int KIND>
int launch_points(const mdc::LensModel& d, float* d_x, float* d_y, int64_t n, hipStream_t s) {
  for (int64_t first = 0; first < n; first += kBlocksPerLaunch * kThreads) {
    const int64_t left = n - first;
    const int64_t blocks = left >= kBlocksPerLaunch * kThreads ? kBlocksPerLaunch : (left + kThreads - 1) / kThreads;
    distort_points_kernel<KIND><<<dim3((unsigned)blocks), dim3(kThreads), 0, s>>>(d, d_x, d_y, first, n);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(kErrHip, "mdcn_distort_points_device: launch failed: %s", hipGetErrorString(e));
  }
  return kOk;
}

int distort_points(const mdcn_model* model, float* d_x, float* d_y, int64_t n, hipStream_t s) {
  const mdc::LensModel d = device_model(model);
  switch (model->kind) {
    case MDCN_RADTAN: return launch_points<mdc::LENS_RADTAN>(d, d_x, d_y, n, s);
    case MDCN_EQUIDISTANT: return launch_points<mdc::LENS_EQUIDISTANT>(d, d_x, d_y, n, s);
    default: return launch_points<mdc::LENS_PINHOLE>(d, d_x, d_y, n, s);
  }
}

}  // namespace

extern "C" {

const char* mdcn_last_error(void) { return g_error; }

int mdcn_distort_points_device(const mdcn_model* model, float* d_x, float* d_y, int64_t n, void* stream) {
  const int rc = check_model("mdcn_distort_points_device", model);
  if (rc != kOk) return rc;
  if (n < 0) return fail(kErrArg, "mdcn_distort_points_device: n = %lld", (long long)n);
  if (n == 0) return kOk;
  if (!d_x || !d_y) return fail(kErrArg, "mdcn_distort_points_device: null coordinate array");
  return distort_points(model, d_x, d_y, n, (hipStream_t)stream);
}

int mdcn_distort_points_host(int device, const mdcn_model* model, float* x, float* y, int64_t n) {
  const char* who = "mdcn_distort_points_host";
  int rc = check_model(who, model);
  if (rc != kOk) return rc;
  if (n < 0) return fail(kErrArg, "%s: n = %lld", who, (long long)n);
  if (n == 0) return kOk;
  if (!x || !y) return fail(kErrArg, "%s: null coordinate array", who);
  if (n > ((int64_t)1 << 36)) return fail(kErrSize, "%s: %lld points (at most 2^36)", who, (long long)n);
  rc = resolve_device(who, &device);
  if (rc != kOk) return rc;
  DeviceGuard guard(device);
  const size_t bytes = (size_t)n * sizeof(float);
  float* d = nullptr;   // x then y
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
  if (e == hipSuccess) rc = distort_points(model, d, d + n, n, s);
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

int mdcn_remap_device(const mdcn_model* model, float* d_rx, float* d_ry, int* d_black, void* stream) {
  const char* who = "mdcn_remap_device";
  const int rc = check_model(who, model);
  if (rc != kOk) return rc;
  if (!d_rx || !d_ry || !d_black) return fail(kErrArg, "%s: null output array", who);
  if (model->in_w < 1 || model->in_h < 1 || model->out_w < 1 || model->out_h < 1)
    return fail(kErrArg, "%s: sizes %d x %d -> %d x %d", who, model->in_w, model->in_h, model->out_w, model->out_h);
  const int64_t n = (int64_t)model->out_w * model->out_h;
  if (n >= ((int64_t)1 << 31)) return fail(kErrSize, "%s: %d x %d entries (fewer than 2^31)", who, model->out_w, model->out_h);
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(d_black, 0, sizeof(int), s) != hipSuccess) return fail(kErrHip, "%s: hipMemsetAsync failed: %s", who, hipGetErrorString(hipGetLastError()));
  const mdc::LensModel d = device_model(model);
  // the nudge constants are double expressions narrowed, as the host class writes them
  Border b = {model->in_w, model->in_h, model->out_w, model->out_h, (float)0.01, (float)(model->in_w - 1.01), (float)(model->in_h - 1.01)};
  const dim3 grid((unsigned)((n + kThreads - 1) / kThreads)), block(kThreads);
  switch (model->kind) {
    case MDCN_RADTAN: remap_kernel<mdc::LENS_RADTAN><<<grid, block, 0, s>>>(d, b, d_rx, d_ry, d_black); break;
    case MDCN_EQUIDISTANT: remap_kernel<mdc::LENS_EQUIDISTANT><<<grid, block, 0, s>>>(d, b, d_rx, d_ry, d_black); break;
    default: remap_kernel<mdc::LENS_PINHOLE><<<grid, block, 0, s>>>(d, b, d_rx, d_ry, d_black); break;
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(kErrHip, "%s: launch failed: %s", who, hipGetErrorString(e));
  return kOk;
}

}  // extern "C"
