// Same-process A/B of kernel shapes for the inverse RadTan / EquiDistant points kernels of libmdc_lensinv.so (an experiment, not part
// of the library): the library's shape (256 threads, one point per thread, csrc/lens_inverse_model.h as it is) against other block
// sizes, two and four points per thread, and -- RadTan -- two divides by the determinant a step instead of the contract's one
// reciprocal.  200 x 10^6 points in place, HIP events, median of 9 after 2 warm-ups; every variant starts from the same raw
// coordinates (restored by a device copy before each run).  profiles/r12_lensinv_kernel_shapes.txt; DESIGN 5.3d.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math tools/lensinv_kernel_shapes.hip -o lensinv_kernel_shapes
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../mono_dataset_code_amd/csrc/lens_inverse_model.h"

#define CHECK(e)                                                                   \
  do {                                                                             \
    hipError_t err_ = (e);                                                         \
    if (err_ != hipSuccess) {                                                      \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, hipGetErrorString(err_)); \
      exit(1);                                                                     \
    }                                                                              \
  } while (0)

// RadTan with two divides per step (NOT the contract's arithmetic: different bits)
__device__ __forceinline__ void radtan_two_divides(const mdc::LensInverseModel& m, float& x, float& y) {
  const float xd = (x - m.cx) / m.fx, yd = (y - m.cy) / m.fy;
  const float k1 = m.k[0], k2 = m.k[1], p1 = m.k[2], p2 = m.k[3];
  float u = xd, v = yd;
  for (int i = 0; i < 8; i++) {
    const float mx2 = u * u, my2 = v * v, mxy = u * v, rho2 = mx2 + my2;
    const float rad = k1 * rho2 + k2 * rho2 * rho2;
    const float dr = k1 + 2.0f * k2 * rho2;
    const float gx = (u + u * rad + 2.0f * p1 * mxy + p2 * (rho2 + 2.0f * mx2)) - xd;
    const float gy = (v + v * rad + 2.0f * p2 * mxy + p1 * (rho2 + 2.0f * my2)) - yd;
    const float j11 = 1.0f + rad + 2.0f * dr * mx2 + 2.0f * p1 * v + 6.0f * p2 * u;
    const float j22 = 1.0f + rad + 2.0f * dr * my2 + 2.0f * p2 * u + 6.0f * p1 * v;
    const float j12 = 2.0f * dr * mxy + 2.0f * p1 * u + 2.0f * p2 * v;
    const float det = j11 * j22 - j12 * j12;
    const float du = (gx * j22 - gy * j12) / det;
    const float dv = (gy * j11 - gx * j12) / det;
    u = u - du;
    v = v - dv;
  }
  const bool outside = !(fabsf(u) < INFINITY && fabsf(v) < INFINITY);
  x = outside ? NAN : m.ofx * u + m.ocx;
  y = outside ? NAN : m.ofy * v + m.ocy;
}

template <int KIND, int THREADS, int PER, bool TWO_DIV>
__global__ __launch_bounds__(THREADS) void variant(mdc::LensInverseModel m, float* __restrict__ xs, float* __restrict__ ys, int64_t n) {
  const int64_t base = (int64_t)blockIdx.x * THREADS * PER + threadIdx.x;
  float x[PER], y[PER];
#pragma unroll
  for (int p = 0; p < PER; p++) {
    const int64_t i = base + (int64_t)p * THREADS;
    if (i < n) x[p] = xs[i], y[p] = ys[i];
  }
#pragma unroll
  for (int p = 0; p < PER; p++) {
    const int64_t i = base + (int64_t)p * THREADS;
    if (i < n) {
      if (TWO_DIV) radtan_two_divides(m, x[p], y[p]);
      else mdc::lens_undistort_point<KIND>(m, x[p], y[p]);
    }
  }
#pragma unroll
  for (int p = 0; p < PER; p++) {
    const int64_t i = base + (int64_t)p * THREADS;
    if (i < n) xs[i] = x[p], ys[i] = y[p];
  }
}

template <int KIND, int THREADS, int PER, bool TWO_DIV>
float run(const char* name, const mdc::LensInverseModel& m, float* x, float* y, const float* x0, const float* y0, int64_t n) {
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  std::vector<float> ms;
  const int64_t per_block = (int64_t)THREADS * PER;
  const unsigned blocks = (unsigned)((n + per_block - 1) / per_block);
  for (int r = 0; r < 11; r++) {
    CHECK(hipMemcpyAsync(x, x0, n * 4, hipMemcpyDeviceToDevice, 0));
    CHECK(hipMemcpyAsync(y, y0, n * 4, hipMemcpyDeviceToDevice, 0));
    CHECK(hipEventRecord(e0, 0));
    variant<KIND, THREADS, PER, TWO_DIV><<<dim3(blocks), dim3(THREADS), 0, 0>>>(m, x, y, n);
    CHECK(hipGetLastError());
    CHECK(hipEventRecord(e1, 0));
    CHECK(hipEventSynchronize(e1));
    float t;
    CHECK(hipEventElapsedTime(&t, e0, e1));
    if (r >= 2) ms.push_back(t);
  }
  std::sort(ms.begin(), ms.end());
  printf("%-44s %8.3f ms  (min %.3f)\n", name, ms[ms.size() / 2], ms[0]);
  fflush(stdout);
  CHECK(hipEventDestroy(e0));
  CHECK(hipEventDestroy(e1));
  return ms[ms.size() / 2];
}

__global__ void fill(float* x, float* y, int64_t n, float w, float h) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  uint32_t a = (uint32_t)i * 2654435761u, b = (uint32_t)i * 2246822519u + 12345u;
  a ^= a >> 15, b ^= b >> 13;
  x[i] = w * (float)(a >> 8) / 16777216.0f;
  y[i] = h * (float)(b >> 8) / 16777216.0f;
}

int main() {
  const int64_t n = 200000000;
  float *x, *y, *x0, *y0;
  CHECK(hipMalloc((void**)&x, n * 4));
  CHECK(hipMalloc((void**)&y, n * 4));
  CHECK(hipMalloc((void**)&x0, n * 4));
  CHECK(hipMalloc((void**)&y0, n * 4));
  printf("inverse points kernels, kernel shapes A/B in one process, %lld points in place, median of 9 (2 warm-ups), HIP events\n", (long long)n);
  {
    mdc::LensInverseModel m = {458.654f, 457.296f, 367.215f, 248.375f, {-0.28340811f, 0.07395907f, 0.00019359f, 1.76187114e-05f}, 0.0f,
                               302.97f, 418.34f, 308.85f, 250.27f};
    fill<<<dim3((unsigned)((n + 255) / 256)), dim3(256)>>>(x0, y0, n, 751.0f, 479.0f);
    CHECK(hipDeviceSynchronize());
    run<mdc::LENSINV_RADTAN, 256, 1, false>("RadTan  256 threads, 1 point  (the library)", m, x, y, x0, y0, n);
    run<mdc::LENSINV_RADTAN, 128, 1, false>("RadTan  128 threads, 1 point", m, x, y, x0, y0, n);
    run<mdc::LENSINV_RADTAN, 512, 1, false>("RadTan  512 threads, 1 point", m, x, y, x0, y0, n);
    run<mdc::LENSINV_RADTAN, 1024, 1, false>("RadTan 1024 threads, 1 point", m, x, y, x0, y0, n);
    run<mdc::LENSINV_RADTAN, 256, 2, false>("RadTan  256 threads, 2 points", m, x, y, x0, y0, n);
    run<mdc::LENSINV_RADTAN, 256, 4, false>("RadTan  256 threads, 4 points", m, x, y, x0, y0, n);
    run<mdc::LENSINV_RADTAN, 256, 1, true>("RadTan  256 threads, 1 point, two divides", m, x, y, x0, y0, n);
    run<mdc::LENSINV_RADTAN, 256, 2, true>("RadTan  256 threads, 2 points, two divides", m, x, y, x0, y0, n);
    run<mdc::LENSINV_RADTAN, 256, 1, false>("RadTan  256 threads, 1 point  (again)", m, x, y, x0, y0, n);
  }
  {
    mdc::LensInverseModel m = {190.978f, 190.973f, 254.931f, 256.897f, {0.003482389f, 0.000715034f, -0.002053236f, 0.000202936f}, 0.0f,
                               60.18f, 60.11f, 251.97f, 264.17f};
    fill<<<dim3((unsigned)((n + 255) / 256)), dim3(256)>>>(x0, y0, n, 511.0f, 511.0f);
    CHECK(hipDeviceSynchronize());
    run<mdc::LENSINV_EQUIDISTANT, 256, 1, false>("EquiDistant  256 threads, 1 point  (the library)", m, x, y, x0, y0, n);
    run<mdc::LENSINV_EQUIDISTANT, 128, 1, false>("EquiDistant  128 threads, 1 point", m, x, y, x0, y0, n);
    run<mdc::LENSINV_EQUIDISTANT, 512, 1, false>("EquiDistant  512 threads, 1 point", m, x, y, x0, y0, n);
    run<mdc::LENSINV_EQUIDISTANT, 1024, 1, false>("EquiDistant 1024 threads, 1 point", m, x, y, x0, y0, n);
    run<mdc::LENSINV_EQUIDISTANT, 256, 2, false>("EquiDistant  256 threads, 2 points", m, x, y, x0, y0, n);
    run<mdc::LENSINV_EQUIDISTANT, 256, 4, false>("EquiDistant  256 threads, 4 points", m, x, y, x0, y0, n);
    run<mdc::LENSINV_EQUIDISTANT, 256, 1, false>("EquiDistant  256 threads, 1 point  (again)", m, x, y, x0, y0, n);
  }
  CHECK(hipFree(x));
  CHECK(hipFree(y));
  CHECK(hipFree(x0));
  CHECK(hipFree(y0));
  return 0;
}
