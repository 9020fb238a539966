// libmdc_lens.so (include/mdc_lens.h): the pinhole / RadTan / EquiDistant lens models on the device.  One translation unit over
// lens_point_model.h, the header the host class and the CPU test program share: built with -ffp-contract=off -fno-fast-math, so the
// kernels give the host's bits.
//
// The kernels, the launches and the calls' host side are lens_points_shell.h's, shared with mdc_lensinv.hip; here are the
// direction's traits and the exported names.
#include "../../include/mdc_lens.h"

#include "lens_points_shell.h"

static_assert(MDCN_OK == kOk && MDCN_ERR_ARG == kErrArg && MDCN_ERR_SIZE == kErrSize && MDCN_ERR_HIP == kErrHip && MDCN_ERR_NO_DEVICE == kErrNoDevice &&
                  MDCN_ERR_NOMEM == kErrNoMem,
              "include/mdc_lens.h and codec_host.h name the same codes");
static_assert(MDCN_PINHOLE == mdc::LENS_PINHOLE && MDCN_RADTAN == mdc::LENS_RADTAN && MDCN_EQUIDISTANT == mdc::LENS_EQUIDISTANT,
              "include/mdc_lens.h and lens_point_model.h name the same kinds");
static_assert(MDCN_PINHOLE == 0 && MDCN_RADTAN == 1 && MDCN_EQUIDISTANT == 2, "the kinds are lens_points_shell.h's 0 .. kKinds - 1");

namespace {

struct Forward {
  typedef mdc::LensModel Model;
  typedef mdcn_model Public;
  static constexpr int kKinds = 3;
  static constexpr bool kTableOverInput = false;
  static constexpr const char* kPointsDevice = "mdcn_distort_points_device";
  static constexpr const char* kPointsHost = "mdcn_distort_points_host";
  static constexpr const char* kTableDevice = "mdcn_remap_device";
  template <int KIND>
  static __host__ __device__ void point(const Model& m, float& x, float& y) {
    mdc::lens_distort_point<KIND>(m, x, y);
  }
  static void derive(Model&, const Public&) {}
  static int check_more(const char*, const Public*) { return kOk; }
};

}  // namespace

extern "C" {

const char* mdcn_last_error(void) { return g_error; }

int mdcn_distort_points_device(const mdcn_model* model, float* d_x, float* d_y, int64_t n, void* stream) {
  return points_device<Forward>(model, d_x, d_y, n, stream);
}

int mdcn_distort_points_host(int device, const mdcn_model* model, float* x, float* y, int64_t n) { return points_host<Forward>(device, model, x, y, n); }

int mdcn_remap_device(const mdcn_model* model, float* d_rx, float* d_ry, int* d_black, void* stream) {
  return table_device<Forward>(model, d_rx, d_ry, d_black, stream);
}

}  // extern "C"
