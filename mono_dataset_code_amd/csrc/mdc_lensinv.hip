// libmdc_lensinv.so (include/mdc_lensinv.h): raw pixel -> rectified pixel through the pinhole / RadTan / EquiDistant / FOV lens
// models on the device.  One translation unit over lens_inverse_model.h, the header the host class and the CPU test program share:
// built with -ffp-contract=off -fno-fast-math, so the kernels give the host's bits.
//
// Both kernels have the forward kernels' shape (mdc_lens.hip): one point (one table entry) per thread, dword loads and stores that a
// wave coalesces into 256-byte runs whatever the arrays' alignment, no LDS, the model in the kernel arguments (scalar registers).
// Pinhole and FOV stream 16 bytes per point; RadTan and EquiDistant run 8 dependent Newton steps with correctly rounded divides and
// are bound by arithmetic.
#include "../../include/mdc_lensinv.h"

#include <math.h>

#include "codec_host.h"
#include "lens_inverse_model.h"

static_assert(MDCU_OK == kOk && MDCU_ERR_ARG == kErrArg && MDCU_ERR_SIZE == kErrSize && MDCU_ERR_HIP == kErrHip && MDCU_ERR_NO_DEVICE == kErrNoDevice &&
                  MDCU_ERR_NOMEM == kErrNoMem,
              "include/mdc_lensinv.h and codec_host.h name the same codes");
static_assert(MDCU_PINHOLE == mdc::LENSINV_PINHOLE && MDCU_RADTAN == mdc::LENSINV_RADTAN && MDCU_EQUIDISTANT == mdc::LENSINV_EQUIDISTANT &&
                  MDCU_FOV == mdc::LENSINV_FOV,
              "include/mdc_lensinv.h and lens_inverse_model.h name the same kinds");
static_assert(sizeof(mdcu_model) == 68, "mdcu_model has mdcn_model's 17 words");

namespace {

constexpr int kThreads = 256;
// HIP caps a launch at 2^32 - 1 threads per dimension: 2^23 blocks of 256 = 2^31 points per launch, the rest in further launches.
constexpr int64_t kBlocksPerLaunch = (int64_t)1 << 23;

template <int KIND>
__global__ __launch_bounds__(kThreads) void undistort_points_kernel(mdc::LensInverseModel m, float* __restrict__ xs, float* __restrict__ ys, int64_t first,
                                                                    int64_t n) {
  const int64_t i = first + (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  float x = xs[i], y = ys[i];
  mdc::lens_undistort_point<KIND>(m, x, y);
  xs[i] = x;
  ys[i] = y;
}

struct Border {
  int in_w, in_h, out_w, out_h;
  float lo, hi_x, hi_y;
};

template <int KIND>
__global__ __launch_bounds__(kThreads) void inverse_remap_kernel(mdc::LensInverseModel m, Border b, float* __restrict__ ux, float* __restrict__ uy,
                                                                 int* __restrict__ outside) {
  const int i = blockIdx.x * kThreads + threadIdx.x;  // in_w * in_h < 2^31
  if (i >= b.in_w * b.in_h) return;
  float x = (float)(i % b.in_w), y = (float)(i / b.in_w);
  mdc::lens_undistort_point<KIND>(m, x, y);
  const bool went_outside = mdc::lens_border_rule(x, y, b.out_w, b.out_h, b.lo, b.hi_x, b.hi_y);
  ux[i] = x;
  uy[i] = y;
  if (went_outside) *outside = 1;  // every writer stores the same value
}

int check_model(const char* who, const mdcu_model* m) {
  if (!m) return fail(kErrArg, "%s: null model", who);
  if (m->kind != MDCU_PINHOLE && m->kind != MDCU_RADTAN && m->kind != MDCU_EQUIDISTANT && m->kind != MDCU_FOV)
    return fail(kErrArg, "%s: kind %d is no lens model", who, m->kind);
  if (!isfinite(m->ofx) || !isfinite(m->ofy) || m->ofx == 0 || m->ofy == 0)
    return fail(kErrArg, "%s: rectified focal lengths %g %g (finite and not 0)", who, (double)m->ofx, (double)m->ofy);
  if (!isfinite(m->fx) || !isfinite(m->fy) || m->fx == 0 || m->fy == 0)
    return fail(kErrArg, "%s: input focal lengths %g %g (finite and not 0)", who, (double)m->fx, (double)m->fy);
  return kOk;
}

mdc::LensInverseModel device_model(const mdcu_model* m) {
  mdc::LensInverseModel d;
  d.fx = m->fx;
  d.fy = m->fy;
  d.cx = m->cx;
  d.cy = m->cy;
  for (int i = 0; i < 4; i++) d.k[i] = m->k[i];
  d.d2t = m->kind == MDCU_FOV ? mdc::lens_inverse_d2t(m->k[0]) : 0.0f;
  d.ofx = m->ofx;
  d.ofy = m->ofy;
  d.ocx = m->ocx;
  d.ocy = m->ocy;
  return d;
}

template <int KIND>
int launch_points(const mdc::LensInverseModel& d, float* d_x, float* d_y, int64_t n, hipStream_t s) {
  for (int64_t first = 0; first < n; first += kBlocksPerLaunch * kThreads) {
    const int64_t left = n - first;
    const int64_t blocks = left >= kBlocksPerLaunch * kThreads ? kBlocksPerLaunch : (left + kThreads - 1) / kThreads;
    undistort_points_kernel<KIND><<<dim3((unsigned)blocks), dim3(kThreads), 0, s>>>(d, d_x, d_y, first, n);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(kErrHip, "mdcu_undistort_points_device: launch failed: %s", hipGetErrorString(e));
  }
  return kOk;
}

int undistort_points(const mdcu_model* model, float* d_x, float* d_y, int64_t n, hipStream_t s) {
  const mdc::LensInverseModel d = device_model(model);
  switch (model->kind) {
    case MDCU_RADTAN: return launch_points<mdc::LENSINV_RADTAN>(d, d_x, d_y, n, s);
    case MDCU_EQUIDISTANT: return launch_points<mdc::LENSINV_EQUIDISTANT>(d, d_x, d_y, n, s);
    case MDCU_FOV: return launch_points<mdc::LENSINV_FOV>(d, d_x, d_y, n, s);
    default: return launch_points<mdc::LENSINV_PINHOLE>(d, d_x, d_y, n, s);
  }
}

}  // namespace

extern "C" {

const char* mdcu_last_error(void) { return g_error; }

int mdcu_undistort_points_device(const mdcu_model* model, float* d_x, float* d_y, int64_t n, void* stream) {
  const int rc = check_model("mdcu_undistort_points_device", model);
  if (rc != kOk) return rc;
  if (n < 0) return fail(kErrArg, "mdcu_undistort_points_device: n = %lld", (long long)n);
  if (n == 0) return kOk;
  if (!d_x || !d_y) return fail(kErrArg, "mdcu_undistort_points_device: null coordinate array");
  return undistort_points(model, d_x, d_y, n, (hipStream_t)stream);
}

int mdcu_undistort_points_host(int device, const mdcu_model* model, float* x, float* y, int64_t n) {
  const char* who = "mdcu_undistort_points_host";
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
  if (e == hipSuccess) rc = undistort_points(model, d, d + n, n, s);
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

int mdcu_inverse_remap_device(const mdcu_model* model, float* d_ux, float* d_uy, int* d_outside, void* stream) {
  const char* who = "mdcu_inverse_remap_device";
  const int rc = check_model(who, model);
  if (rc != kOk) return rc;
  if (!d_ux || !d_uy || !d_outside) return fail(kErrArg, "%s: null output array", who);
  if (model->in_w < 1 || model->in_h < 1 || model->out_w < 1 || model->out_h < 1)
    return fail(kErrArg, "%s: sizes %d x %d -> %d x %d", who, model->in_w, model->in_h, model->out_w, model->out_h);
  const int64_t n = (int64_t)model->in_w * model->in_h;
  if (n >= ((int64_t)1 << 31)) return fail(kErrSize, "%s: %d x %d entries (fewer than 2^31)", who, model->in_w, model->in_h);
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(d_outside, 0, sizeof(int), s) != hipSuccess) return fail(kErrHip, "%s: hipMemsetAsync failed: %s", who, hipGetErrorString(hipGetLastError()));
  const mdc::LensInverseModel d = device_model(model);
  // the nudge constants are double expressions narrowed, as the host class writes them -- here against the rectified image's size
  Border b = {model->in_w, model->in_h, model->out_w, model->out_h, (float)0.01, (float)(model->out_w - 1.01), (float)(model->out_h - 1.01)};
  const dim3 grid((unsigned)((n + kThreads - 1) / kThreads)), block(kThreads);
  switch (model->kind) {
    case MDCU_RADTAN: inverse_remap_kernel<mdc::LENSINV_RADTAN><<<grid, block, 0, s>>>(d, b, d_ux, d_uy, d_outside); break;
    case MDCU_EQUIDISTANT: inverse_remap_kernel<mdc::LENSINV_EQUIDISTANT><<<grid, block, 0, s>>>(d, b, d_ux, d_uy, d_outside); break;
    case MDCU_FOV: inverse_remap_kernel<mdc::LENSINV_FOV><<<grid, block, 0, s>>>(d, b, d_ux, d_uy, d_outside); break;
    default: inverse_remap_kernel<mdc::LENSINV_PINHOLE><<<grid, block, 0, s>>>(d, b, d_ux, d_uy, d_outside); break;
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(kErrHip, "%s: launch failed: %s", who, hipGetErrorString(e));
  return kOk;
}

}  // extern "C"
