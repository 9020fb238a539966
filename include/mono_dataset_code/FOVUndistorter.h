// Drop-in for the reference's src/FOVUndistorter.h:36-96 (class UndistorterFOV).
//
// Same public surface -- constructor from camera.txt, undistort<T> for float and
// unsigned char, distortCoordinates, the K / calibration / dimension getters,
// isValid -- so src/BenchmarkDatasetReader.h, main_playbackDataset.cpp and
// main_vignetteCalib.cpp compile against it unchanged.  Differences are inside:
// the remap tables are built on the host with the reference's exact float
// operation sequence (they must be bit-identical) and uploaded
// once to the GPU; undistort<T> runs as a HIP kernel on gfx950 through the C ABI
// in include/mdc_hip.h.  There is no CPU fallback for the per-frame work.
#pragma once
#include "ExposureImage.h"
#include "Eigen/Core"

struct mdc_ctx;
struct MdcHostAccess;

#ifndef MDC_API  /* the libraries are built with -fvisibility=hidden: this marks what they export */
#if defined(__GNUC__) || defined(__clang__)
#define MDC_API __attribute__((visibility("default")))
#else
#define MDC_API
#endif
#endif
class MDC_API UndistorterFOV {
 public:
  UndistorterFOV(const char* configFileName);           // parses camera.txt, builds + uploads the remap
  UndistorterFOV();                                     // invalid object (reference :39-44)
  ~UndistorterFOV();

  // Bilinear warp of a in_w*in_h image into out_w*out_h floats (host pointers,
  // blocking).  Silent no-op on an invalid object; prints ERROR and returns on a
  // pixel-count mismatch -- as the reference (src/FOVUndistorter.cpp:325-338).
  template <typename T>
  void undistort(const T* input, float* output, int nPixIn, int nPixOut) const;

  // In place: rectified pixel coordinates -> raw (distorted) pixel coordinates.
  void distortCoordinates(float* in_x, float* in_y, int n);

  // In place, the other way: raw (distorted) pixel coordinates -> rectified pixel coordinates, for every lens kind the class
  // reads (not in the reference).  A point the model cannot bring back -- FOV: raw radius times omega not below pi/2;
  // EquiDistant: an angle outside [0, pi/2); RadTan: an iteration that left the finite numbers -- comes out as NaN in both
  // coordinates.  Calls of at least MDC_UNDISTORT_GPU_MIN points (default 65536) run on the device, with the host loop's bits.
  void undistortCoordinates(float* x, float* y, int n);

  Eigen::Matrix3f getK_rect() const { return k_rect_; }
  Eigen::Matrix3f getK_org() const { return k_org_; }
  float getOmega() const { return calib_in_[4]; }
  const Eigen::VectorXf getOriginalCalibration() const {
    Eigen::VectorXf c(5);
    c[0] = calib_in_[0] * in_w_;
    c[1] = calib_in_[1] * in_h_;
    c[2] = calib_in_[2] * in_w_ - 0.5;
    c[3] = calib_in_[3] * in_h_ - 0.5;
    c[4] = calib_in_[4];
    return c;
  }
  const Eigen::Vector2i getInputDims() const { return Eigen::Vector2i(in_w_, in_h_); }
  const Eigen::Vector2i getOutputDims() const { return Eigen::Vector2i(out_w_, out_h_); }
  bool isValid() const { return valid_; }

  // The lens model line 1 of camera.txt named: 0 = FOV / pinhole (a bare five-number line, `FOV ...`, `Pinhole ...`),
  // 1 = RadTan (k1 k2 p1 p2), 2 = EquiDistant (k1 k2 k3 k4; `KannalaBrandt` is the same polynomial under DSO's other name).
  // For 1 and 2 getOmega() is 0, getOriginalCalibration() / getK_org() give the input pinhole part as for FOV, and
  // lensParameters() the four distortion coefficients (zeros for 0).  Neither is inline, and the class has no data member for
  // them: its size and layout stay what they were before there were lens models (the members below), so a program compiled
  // against an earlier version of this header -- which allocates that many bytes -- runs on this library unchanged.  What a RadTan / EquiDistant object holds beyond the members below lives in the library,
  // keyed by the object (fov_undistorter.cpp: lens_states).
  int lensModel() const;
  const float* lensParameters() const;

 private:
  UndistorterFOV(const UndistorterFOV&);             // owning raw tables: not copyable
  UndistorterFOV& operator=(const UndistorterFOV&);
  friend struct MdcHostAccess;

  Eigen::Matrix3f k_rect_, k_org_;
  float calib_in_[5];   // camera.txt line 1: fx fy cx cy omega, relative to the input size
  float calib_out_[5];  // normalised output intrinsics after construction
  int in_w_, in_h_, out_w_, out_h_;
  float* remap_x_;      // out_w*out_h source x coordinates, -1 = black
  float* remap_y_;
  bool valid_;
  mdc_ctx* gpu_;        // device context holding the uploaded remap (0 if no GPU)
  // (no member may be added, removed or moved: see lensModel())
  const float* lensCamera() const;  // kinds 1 and 2: fx fy cx cy of the input camera in pixels, as line 1 gave or implied them
};

// The task description calls this class "Undistorter"; the reference names it
// UndistorterFOV.  Both spellings work.
typedef UndistorterFOV Undistorter;
