// libmdc_lensinv.so (include/mdc_lensinv.h): raw pixel -> rectified pixel through the pinhole / RadTan / EquiDistant / FOV lens
// models on the device.  One translation unit over lens_inverse_model.h, the header the host class and the CPU test program share:
// built with -ffp-contract=off -fno-fast-math, so the kernels give the host's bits.
//
// The kernels, the launches and the calls' host side are lens_points_shell.h's, shared with mdc_lens.hip; here are the direction's
// traits and the exported names.  Pinhole and FOV stream 16 bytes per point; RadTan and EquiDistant run 8 dependent Newton steps
// with correctly rounded divides and are bound by arithmetic.
#include "../../include/mdc_lensinv.h"

#include "lens_points_shell.h"  // before the model: it brings the HIP runtime

#include "lens_inverse_model.h"

static_assert(MDCU_OK == kOk && MDCU_ERR_ARG == kErrArg && MDCU_ERR_SIZE == kErrSize && MDCU_ERR_HIP == kErrHip && MDCU_ERR_NO_DEVICE == kErrNoDevice &&
                  MDCU_ERR_NOMEM == kErrNoMem,
              "include/mdc_lensinv.h and codec_host.h name the same codes");
static_assert(MDCU_PINHOLE == mdc::LENSINV_PINHOLE && MDCU_RADTAN == mdc::LENSINV_RADTAN && MDCU_EQUIDISTANT == mdc::LENSINV_EQUIDISTANT &&
                  MDCU_FOV == mdc::LENSINV_FOV,
              "include/mdc_lensinv.h and lens_inverse_model.h name the same kinds");
static_assert(MDCU_PINHOLE == 0 && MDCU_RADTAN == 1 && MDCU_EQUIDISTANT == 2 && MDCU_FOV == 3, "the kinds are lens_points_shell.h's 0 .. kKinds - 1");
static_assert(sizeof(mdcu_model) == 68, "mdcu_model has mdcn_model's 17 words");

namespace {

struct Inverse {
  typedef mdc::LensInverseModel Model;
  typedef mdcu_model Public;
  static constexpr int kKinds = 4;
  static constexpr bool kTableOverInput = true;
  static constexpr const char* kPointsDevice = "mdcu_undistort_points_device";
  static constexpr const char* kPointsHost = "mdcu_undistort_points_host";
  static constexpr const char* kTableDevice = "mdcu_inverse_remap_device";
  template <int KIND>
  static __host__ __device__ void point(const Model& m, float& x, float& y) {
    mdc::lens_undistort_point<KIND>(m, x, y);
  }
  static void derive(Model& d, const Public& m) { d.d2t = m.kind == MDCU_FOV ? mdc::lens_inverse_d2t(m.k[0]) : 0.0f; }
  static int check_more(const char* who, const Public* m) {
    if (!isfinite(m->fx) || !isfinite(m->fy) || m->fx == 0 || m->fy == 0)
      return fail(kErrArg, "%s: input focal lengths %g %g (finite and not 0)", who, (double)m->fx, (double)m->fy);
    return kOk;
  }
};

}  // namespace

extern "C" {

const char* mdcu_last_error(void) { return g_error; }

int mdcu_undistort_points_device(const mdcu_model* model, float* d_x, float* d_y, int64_t n, void* stream) {
  return points_device<Inverse>(model, d_x, d_y, n, stream);
}

int mdcu_undistort_points_host(int device, const mdcu_model* model, float* x, float* y, int64_t n) { return points_host<Inverse>(device, model, x, y, n); }

int mdcu_inverse_remap_device(const mdcu_model* model, float* d_ux, float* d_uy, int* d_outside, void* stream) {
  return table_device<Inverse>(model, d_ux, d_uy, d_outside, stream);
}

}  // extern "C"
