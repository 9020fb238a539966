// Host side of UndistorterFOV (drop-in for the reference's src/FOVUndistorter.cpp).
//
// Everything here runs once per sequence on the CPU: camera.txt parsing, choice
// of the rectified intrinsics, and the remapX/remapY tables.  The tables are the
// sensitive part of the whole path -- a 1-ulp difference in a remap entry moves
// the output by up to 4e-2 relative on a noisy frame -- so they are computed with
// the host libm in single precision with exactly the operation sequence of the
// reference (file:line cited at each step; this translation unit is compiled
// with -ffp-contract=off) and compared bit-for-bit against the reference build
// in tests/test_tables_vs_ref.py.  The per-frame warp itself is NOT here: it is a
// gfx950 kernel behind mdc_undistort_host_* (include/mdc_hip.h).
#include "FOVUndistorter.h"

#include <dlfcn.h>
#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <mutex>
#include <string>

#include "mdc_hip.h"
#include "mdc_lens.h"
#include "host_device.h"
#include "sibling_library.h"
#include "../fov_point_model.h"  // atanf_host_libm: the restatement the device runs, checked against THIS process's libm below
#include "../lens_point_model.h"  // the RadTan / EquiDistant arithmetic and the crop rule, shared with libmdc_lens.so's kernels
#include "mdc_lensinv.h"
#include "../lens_inverse_model.h"  // raw -> rectified for every kind, shared with libmdc_lensinv.so's kernels

namespace {

// The four text lines of camera.txt, decoded (reference :63-123).
struct CameraFile {
  float in[5];   // fx fy cx cy omega (relative to the input size)
  int in_w, in_h;
  int mode;      // kCrop, kFull or kExplicit
  float out[5];  // only for kExplicit
  int out_w, out_h;
};
// What line 1 adds when it names RadTan, EquiDistant or KannalaBrandt (kind 0: it did not).
struct LensLine {
  int kind;
  std::string name;  // the keyword as written
  float k[4];
  float cam[4];  // fx fy cx cy in pixels
};
enum { kExplicit = 0, kCrop = -1, kFull = -2 };
enum ParseResult { kParsed, kUnreadable, kBadHeader, kNoRectification, kBadOutputPars, kBadOutputSize };

// Line 1 in DSO's keyword grammar (the same authors' later reader of the same folder layout):
//   FOV fx fy cx cy omega | Pinhole fx fy cx cy 0 | RadTan fx fy cx cy k1 k2 p1 p2 | EquiDistant fx fy cx cy k1 k2 k3 k4 |
//   KannalaBrandt fx fy cx cy k1 k2 k3 k4
// Units, DSO's rule: cx < 1 && cy < 1 means the four intrinsics are relative to the input size, else they are pixels.  A wrong
// parameter count, a value that is not finite, fx <= 0 or fy <= 0 is a bad header.  FOV / Pinhole end as the bare line's five
// relative numbers in c.in (pixels become relative first, in float), so the object is the bare line's; the new kinds keep their
// pixel intrinsics in c.cam (pixels as they stand; relative ones as fx*w, fy*h, cx*w - 0.5, cy*h - 0.5, the subtraction in double and
// narrowed, as InputModel does) and the relative ones in c.in with c.in[4] = 0.
enum KeywordResult { kNoKeyword, kKeywordBad, kKeywordFov, kKeywordLens };

KeywordResult parse_keyword_line(const std::string& line1, const std::string& line2, CameraFile& c, LensLine& lens) {
  size_t at = line1.find_first_not_of(" \t");
  if (at == std::string::npos || !std::isalpha((unsigned char)line1[at])) return kNoKeyword;
  const size_t end = line1.find_first_of(" \t", at);
  const std::string word = line1.substr(at, end == std::string::npos ? std::string::npos : end - at);
  int kind, want;
  if (word == "FOV" || word == "Pinhole") kind = mdc::LENS_PINHOLE, want = 5;  // the existing path (omega 0 is its pinhole case)
  else if (word == "RadTan") kind = mdc::LENS_RADTAN, want = 8;
  else if (word == "EquiDistant" || word == "KannalaBrandt") kind = mdc::LENS_EQUIDISTANT, want = 8;
  else return kKeywordBad;
  float v[9];
  int n = 0;
  const char* p = end == std::string::npos ? "" : line1.c_str() + end;
  for (;;) {
    while (*p == ' ' || *p == '\t' || *p == '\r') p++;
    if (!*p) break;
    char* q;
    const float x = std::strtof(p, &q);
    if (q == p || n == 9 || !std::isfinite(x)) return kKeywordBad;
    v[n++] = x;
    p = q;
  }
  if (n != want || !(v[0] > 0) || !(v[1] > 0)) return kKeywordBad;
  if (std::sscanf(line2.c_str(), "%d %d", &c.in_w, &c.in_h) != 2) return kKeywordBad;
  const bool relative = v[2] < 1 && v[3] < 1;
  const int w = c.in_w, h = c.in_h;
  if (relative) {
    for (int i = 0; i < 4; i++) c.in[i] = v[i];
  } else {
    c.in[0] = v[0] / w;
    c.in[1] = v[1] / h;
    c.in[2] = (v[2] + 0.5f) / w;
    c.in[3] = (v[3] + 0.5f) / h;
  }
  if (kind == mdc::LENS_PINHOLE) {
    c.in[4] = v[4];
    return kKeywordFov;
  }
  c.in[4] = 0;
  lens.kind = kind;
  lens.name = word;
  for (int i = 0; i < 4; i++) lens.k[i] = v[4 + i];
  if (relative) {
    lens.cam[0] = v[0] * w;
    lens.cam[1] = v[1] * h;
    lens.cam[2] = v[2] * w - 0.5;  // double subtraction, narrowed
    lens.cam[3] = v[3] * h - 0.5;
  } else {
    for (int i = 0; i < 4; i++) lens.cam[i] = v[i];
  }
  return kKeywordLens;
}

ParseResult parse_camera_file(const char* path, CameraFile& c, LensLine& lens) {
  std::ifstream f(path);
  if (!f.good()) return kUnreadable;
  std::string line[4];
  for (int i = 0; i < 4; i++) std::getline(f, line[i]);

  const KeywordResult kw = parse_keyword_line(line[0], line[1], c, lens);
  if (kw == kKeywordBad) return kBadHeader;
  const bool head = kw != kNoKeyword ||
                    (std::sscanf(line[0].c_str(), "%f %f %f %f %f", &c.in[0], &c.in[1], &c.in[2], &c.in[3], &c.in[4]) == 5 &&
                     std::sscanf(line[1].c_str(), "%d %d", &c.in_w, &c.in_h) == 2);
  if (!head) return kBadHeader;
  std::printf("Input resolution: %d %d\n", c.in_w, c.in_h);
  if (kw == kKeywordLens)
    std::printf("Input Calibration (%s fx fy cx cy k): %f %f %f %f %f %f %f %f\n", lens.name.c_str(), lens.cam[0], lens.cam[1], lens.cam[2],
                lens.cam[3], lens.k[0], lens.k[1], lens.k[2], lens.k[3]);
  else
    std::printf("Input Calibration (fx fy cx cy): %f %f %f %f %f\n", c.in_w * c.in[0], c.in_h * c.in[1], c.in_w * c.in[2],
                c.in_h * c.in[3], c.in[4]);

  if (line[2] == "crop") {
    c.mode = kCrop;
    std::printf("Out: Crop\n");
  } else if (line[2] == "full" && kw == kKeywordLens) {
    std::printf("Out: Full is not implemented for this lens model... not rectifying.\n");
    return kBadOutputPars;
  } else if (line[2] == "full") {
    c.mode = kFull;
    std::printf("Out: Full\n");
  } else if (line[2] == "none") {
    std::printf("NO RECTIFICATION\n");
    return kNoRectification;
  } else if (std::sscanf(line[2].c_str(), "%f %f %f %f %f", &c.out[0], &c.out[1], &c.out[2], &c.out[3], &c.out[4]) == 5) {
    c.mode = kExplicit;
    std::printf("Out: %f %f %f %f %f\n", c.out[0], c.out[1], c.out[2], c.out[3], c.out[4]);
  } else {
    std::printf("Out: Failed to Read Output pars... not rectifying.\n");
    return kBadOutputPars;
  }

  if (std::sscanf(line[3].c_str(), "%d %d", &c.out_w, &c.out_h) != 2) {
    std::printf("Out: Failed to Read Output resolution... not rectifying.\n");
    return kBadOutputSize;
  }
  std::printf("Output resolution: %d %d\n", c.out_w, c.out_h);
  return kParsed;
}

// Input pinhole parameters in pixels + the FOV-model constant (reference :131-138 / :289-296).
struct InputModel {
  float omega, d2t, fx, fy, cx, cy;
  InputModel(const float calib[5], int w, int h) {
    omega = calib[4];
    d2t = 2.0f * ::tan((double)(omega / 2.0f));  // double-precision tan (as the reference build binds it), narrowed
    fx = calib[0] * w;
    fy = calib[1] * h;
    cx = calib[2] * w - 0.5;         // double subtraction, narrowed
    cy = calib[3] * h - 0.5;
  }
};

inline float fmax_std(float a, float b) { return a < b ? b : a; }  // std::max

// Undistorted radius of a distorted radius (tan in double, quotient narrowed).
inline float undistorted_radius(float r, const InputModel& m) { return ::tan((double)(r * m.omega)) / m.d2t; }

// Rectified intrinsics (pixels) for the three output modes + the omega == 0 case
// (reference :141-212), returned normalised by the output size (:214-218).
void pick_output_intrinsics(const CameraFile& c, float norm[5]) {
  const InputModel m(c.in, c.in_w, c.in_h);
  float ofx, ofy, ocx, ocy;
  if (c.in[4] == 0) {  // pinhole input: same relative intrinsics at the new size
    ofx = c.in[0] * c.out_w;
    ofy = c.in[1] * c.out_h;
    ocx = (c.in[2] * c.out_w) - 0.5;
    ocy = (c.in[3] * c.out_h) - 0.5;
  } else if (c.mode == kCrop || c.mode == kFull) {
    const float left = m.cx / m.fx;
    const float right = (c.in_w - 1 - m.cx) / m.fx;
    const float top = m.cy / m.fy;
    const float bottom = (c.in_h - 1 - m.cy) / m.fy;
    const float sx = (float)c.out_w / (float)c.in_w, sy = (float)c.out_h / (float)c.in_h;
    if (c.mode == kCrop) {  // largest rectangle with no black pixels: use the edge mid-points
      const float t_left = undistorted_radius(left, m), t_right = undistorted_radius(right, m);
      const float t_top = undistorted_radius(top, m), t_bottom = undistorted_radius(bottom, m);
      ofy = m.fy * ((top + bottom) / (t_top + t_bottom)) * sy;
      ocy = (t_top / top) * ofy * m.cy / m.fy;
      ofx = m.fx * ((left + right) / (t_left + t_right)) * sx;
      ocx = (t_left / left) * ofx * m.cx / m.fx;
    } else {  // every input pixel visible: use the corners
      const float tl = ::sqrt((double)(left * left + top * top)), tr = ::sqrt((double)(right * right + top * top));
      const float bl = ::sqrt((double)(left * left + bottom * bottom)), br = ::sqrt((double)(right * right + bottom * bottom));
      const float t_tl = undistorted_radius(tl, m), t_tr = undistorted_radius(tr, m);
      const float t_bl = undistorted_radius(bl, m), t_br = undistorted_radius(br, m);
      const float hor = fmax_std(br, tr) + fmax_std(bl, tl);
      const float vert = fmax_std(tr, tl) + fmax_std(bl, br);
      const float t_hor = fmax_std(t_br, t_tr) + fmax_std(t_bl, t_tl);
      const float t_vert = fmax_std(t_tr, t_tl) + fmax_std(t_bl, t_br);
      ofy = m.fy * (vert / t_vert) * sy;
      ocy = fmax_std(t_tl / tl, t_tr / tr) * ofy * m.cy / m.fy;
      ofx = m.fx * (hor / t_hor) * sx;
      ocx = fmax_std(t_bl / bl, t_tl / tl) * ofx * m.cx / m.fx;
    }
    std::printf("new K: %f %f %f %f\n", ofx, ofy, ocx, ocy);
    std::printf("old K: %f %f %f %f\n", m.fx, m.fy, m.cx, m.cy);
  } else {
    ofx = c.out[0] * c.out_w;
    ofy = c.out[1] * c.out_h;
    ocx = c.out[2] * c.out_w - 0.5;
    ocy = c.out[3] * c.out_h - 0.5;
  }
  norm[0] = ofx / c.out_w;
  norm[1] = ofy / c.out_h;
  norm[2] = (ocx + 0.5) / c.out_w;
  norm[3] = (ocy + 0.5) / c.out_h;
  norm[4] = 0;
}

// Rectified pixel -> raw pixel through the FOV (atan) lens model, in place
// (reference :289-318).  Single precision, host libm sqrtf/atanf.
void warp_points(const float calib_in[5], int in_w, int in_h, const float calib_out[5], int out_w, int out_h, float* xs,
                 float* ys, int n) {
  const InputModel m(calib_in, in_w, in_h);
  const float ofx = calib_out[0] * out_w, ofy = calib_out[1] * out_h;
  const float ocx = calib_out[2] * out_w - 0.5f, ocy = calib_out[3] * out_h - 0.5f;
  for (int i = 0; i < n; i++) {
    float ix = (xs[i] - ocx) / ofx;
    float iy = (ys[i] - ocy) / ofy;
    const float r = sqrtf(ix * ix + iy * iy);
    const float fac = (r == 0 || m.omega == 0) ? 1 : atanf(r * m.d2t) / (m.omega * r);
    ix = m.fx * fac * ix + m.cx;
    iy = m.fy * fac * iy + m.cy;
    xs[i] = ix;
    ys[i] = iy;
  }
}

// ---- RadTan / EquiDistant (csrc/lens_point_model.h holds the arithmetic) ----------------------------------------------

mdc::LensModel lens_model_of(const float cam[4], const float k[4], const float calib_out[5], int out_w, int out_h) {
  mdc::LensModel m;
  m.fx = cam[0];
  m.fy = cam[1];
  m.cx = cam[2];
  m.cy = cam[3];
  for (int i = 0; i < 4; i++) m.k[i] = k[i];
  mdc::lens_set_rectified(m, calib_out, out_w, out_h);  // pixel units derived from the stored normalised values, by every consumer alike
  return m;
}

// Rectified intrinsics of a RadTan / EquiDistant camera, normalised as pick_output_intrinsics normalises them: `crop` by DSO's search,
// else the explicit relative line 3.  false (after a message): the object stays invalid.
bool pick_output_intrinsics_lens(const CameraFile& c, const LensLine& lens, float norm[5]) {
  float ofx, ofy, ocx, ocy;
  if (c.mode == kCrop) {
    mdc::LensModel m = mdc::LensModel();
    for (int i = 0; i < 4; i++) m.k[i] = lens.k[i];
    m.fx = lens.cam[0];
    m.fy = lens.cam[1];
    m.cx = lens.cam[2];
    m.cy = lens.cam[3];
    mdc::LensCrop crop;
    const int rc = mdc::lens_crop(lens.kind, m, c.in_w, c.in_h, c.out_w, c.out_h, &crop);
    if (rc != mdc::LENS_CROP_OK) {
      std::printf(rc == mdc::LENS_CROP_SIZE ? "Out: Crop needs an output of at least 2 x 2 pixels... not rectifying.\n"
                  : rc == mdc::LENS_CROP_NOTHING_INSIDE ? "Out: Crop found no point of the lens model inside the input image... not rectifying.\n"
                                                        : "Out: Crop did not converge in 500 rounds... not rectifying.\n");
      return false;
    }
    ofx = crop.ofx;
    ofy = crop.ofy;
    ocx = crop.ocx;
    ocy = crop.ocy;
    std::printf("crop rounds: %d\n", crop.rounds);
    std::printf("new K: %f %f %f %f\n", ofx, ofy, ocx, ocy);
    std::printf("old K: %f %f %f %f\n", m.fx, m.fy, m.cx, m.cy);
  } else {
    ofx = c.out[0] * c.out_w;
    ofy = c.out[1] * c.out_h;
    ocx = c.out[2] * c.out_w - 0.5;
    ocy = c.out[3] * c.out_h - 0.5;
  }
  norm[0] = ofx / c.out_w;
  norm[1] = ofy / c.out_h;
  norm[2] = (ocx + 0.5) / c.out_w;
  norm[3] = (ocy + 0.5) / c.out_h;
  norm[4] = 0;
  return true;
}

void warp_points_lens(int kind, const mdc::LensModel& m, float* xs, float* ys, long n) {
  if (kind == mdc::LENS_RADTAN)
    for (long i = 0; i < n; i++) mdc::lens_distort_point<mdc::LENS_RADTAN>(m, xs[i], ys[i]);
  else
    for (long i = 0; i < n; i++) mdc::lens_distort_point<mdc::LENS_EQUIDISTANT>(m, xs[i], ys[i]);
}

// The bulk calls of libmdc_lens.so (distortCoordinates) and libmdc_lensinv.so (undistortCoordinates), loaded at run time the way
// device_lanes.cpp loads the PNG decoders: the file next to this library (or the one `env` names), opened at a direction's first
// bulk call, once per process, and never closed (it holds a HIP module).  mdcn_model and mdcu_model are the same 17 words, so one
// function-pointer type serves both.
static_assert(sizeof(mdcn_model) == 68 && sizeof(mdcu_model) == 68, "the two lens libraries take the same model words");
struct LensLibrary {
  const char* method;                         // UndistorterFOV's, for the messages
  const char *file, *env;                     // the library, and the variable that names another file
  const char *points_host_name, *last_error_name;
  std::once_flag opened;
  int (*points_host)(int, const void*, float*, float*, int64_t);  // 0 when the library is not there
  const char* (*last_error)();
  bool said;
};
LensLibrary g_lens = {"distortCoordinates", "libmdc_lens.so", "MDC_LIB_LENS", "mdcn_distort_points_host", "mdcn_last_error"};
LensLibrary g_lensinv = {"undistortCoordinates", "libmdc_lensinv.so", "MDC_LIB_LENSINV", "mdcu_undistort_points_host", "mdcu_last_error"};

bool lens_library_there(LensLibrary& l) {
  std::call_once(l.opened, [&l] {
    void* lib = mdc_host::open_sibling_library(l.file, l.env);
    if (!lib) return;
    l.last_error = (const char* (*)())dlsym(lib, l.last_error_name);
    if (l.last_error) l.points_host = (int (*)(int, const void*, float*, float*, int64_t))dlsym(lib, l.points_host_name);
  });
  return l.points_host != 0;
}

// A bulk call's way to the device: n points at or past the threshold (0 = never), `guard` (if any) agreeing, the library and a GPU
// context there.  true: the device has written the n points.  false: the caller's host loop does the work -- the bits are the same
// either way (one header, no FMA on either side) --, and where the library or the GPU is missing this says so once per direction.
bool bulk_points_on_device(LensLibrary& l, long gpu_min, bool (*guard)(), mdc_ctx* gpu, const void* model, float* x, float* y, int n) {
  if (!(gpu_min > 0 && n >= gpu_min && (!guard || guard()))) return false;
  const bool there = lens_library_there(l);
  mdc_info info;
  if (there && gpu && mdc_get_info(gpu, &info) == MDC_OK) {
    if (l.points_host(info.device, model, x, y, n) == MDCN_OK) return true;  // == MDCU_OK
    // the call leaves the coordinates untouched when it fails (they are copied back last): say so and do the work on the host
    std::fprintf(stderr, "UndistorterFOV::%s: the GPU call failed (%s); computing %d points on the host\n", l.method, l.last_error(), n);
  } else {
    if (!l.said && there) std::fprintf(stderr, "UndistorterFOV::%s: no GPU context; bulk calls are computed on the host (same results)\n", l.method);
    if (!l.said && !there)
      std::fprintf(stderr, "UndistorterFOV::%s: %s could not be loaded (%s names another file); bulk calls are computed on the host (same results)\n", l.method,
                   l.file, l.env);
    l.said = true;
  }
  return false;
}

// The device's atanf is a restatement of ONE libm's algorithm (glibc's fdlibm atanf).  A process linked against another libm
// -- a newer glibc whose atanf is correctly rounded, musl, a vendor libm -- would get last-bit differences between small
// calls (host loop, ::atanf) and large ones (device): checked once against the libm this process really runs, on a spread of
// arguments through every interval of the algorithm; on any difference bulk calls stay on the host, like the small ones.
// (EquiDistant's host loop runs the restatement itself, so its bits are the device's whatever the libm; the check guards its bulk
// path all the same, so that one rule decides for every lens with an atanf in it.)
bool libm_is_the_restated_one() {
  static const bool same = [] {
    uint32_t bad = 0;
    for (uint32_t u = 0x30000000u; u < 0x4d800000u && !bad; u += 9973u) {  // 2^-31 .. 2^28, ~49,000 arguments, both signs
      const float x = mdc::fov_float(u);
      if (mdc::fov_bits(mdc::atanf_host_libm(x)) != mdc::fov_bits(::atanf(x)) ||
          mdc::fov_bits(mdc::atanf_host_libm(-x)) != mdc::fov_bits(::atanf(-x)))
        bad = u;
    }
    if (bad)
      std::fprintf(stderr, "UndistorterFOV: this process's atanf differs from the algorithm the GPU kernel restates (first at %a): "
                           "distortCoordinates stays on the host for every point count\n", mdc::fov_float(bad));
    return bad == 0;
  }();
  return same;
}

void set_pinhole(Eigen::Matrix3f& k, const float rel[5], int w, int h) {
  k.setIdentity();
  k(0, 0) = rel[0] * w;
  k(1, 1) = rel[1] * h;
  k(0, 2) = rel[2] * w - 0.5;
  k(1, 2) = rel[3] * h - 0.5;
}

// What a RadTan / EquiDistant object holds beyond the class's members.  The class keeps the size and layout it had before (a program
// compiled against an earlier header allocates exactly that many bytes), so this lives here, keyed by the object: made by its constructor,
// dropped by its destructor, and read through pointers that stay put for the object's life (map nodes do not move).  FOV objects
// have no entry.  The table itself is never destroyed: objects with static storage may outlive this file's statics.
struct LensState {
  int kind;
  float k[4];
  float cam[4];  // fx fy cx cy in pixels
};
std::mutex& lens_mutex() {
  static std::mutex* m = new std::mutex;
  return *m;
}
std::map<const UndistorterFOV*, LensState>& lens_states() {
  static std::map<const UndistorterFOV*, LensState>* t = new std::map<const UndistorterFOV*, LensState>;
  return *t;
}
const LensState* find_lens_state(const UndistorterFOV* u) {
  std::lock_guard<std::mutex> lock(lens_mutex());
  const std::map<const UndistorterFOV*, LensState>::const_iterator it = lens_states().find(u);
  return it == lens_states().end() ? 0 : &it->second;
}
void keep_lens_state(const UndistorterFOV* u, const LensLine& lens) {
  LensState s;
  s.kind = lens.kind;
  for (int i = 0; i < 4; i++) {
    s.k[i] = lens.k[i];
    s.cam[i] = lens.cam[i];
  }
  std::lock_guard<std::mutex> lock(lens_mutex());
  lens_states()[u] = s;
}
void drop_lens_state(const UndistorterFOV* u) {
  std::lock_guard<std::mutex> lock(lens_mutex());
  lens_states().erase(u);
}
const float kNoLensParameters[4] = {0, 0, 0, 0};

}  // namespace

int UndistorterFOV::lensModel() const {
  const LensState* s = find_lens_state(this);
  return s ? s->kind : 0;
}
const float* UndistorterFOV::lensParameters() const {
  const LensState* s = find_lens_state(this);
  return s ? s->k : kNoLensParameters;
}
const float* UndistorterFOV::lensCamera() const {
  const LensState* s = find_lens_state(this);
  return s ? s->cam : kNoLensParameters;
}

UndistorterFOV::UndistorterFOV()
    : in_w_(0), in_h_(0), out_w_(0), out_h_(0), remap_x_(0), remap_y_(0), valid_(false), gpu_(0) {
  for (int i = 0; i < 5; i++) calib_in_[i] = calib_out_[i] = 0;
  drop_lens_state(this);  // (memory that held an object which was never destroyed)
}

UndistorterFOV::UndistorterFOV(const char* configFileName)
    : in_w_(0), in_h_(0), out_w_(0), out_h_(0), remap_x_(0), remap_y_(0), valid_(false), gpu_(0) {
  for (int i = 0; i < 5; i++) calib_in_[i] = calib_out_[i] = 0;
  drop_lens_state(this);  // (memory that held an object which was never destroyed)

  CameraFile cam = CameraFile();
  LensLine lens = LensLine();
  const ParseResult pr = parse_camera_file(configFileName, cam, lens);
  if (pr == kUnreadable || pr == kBadHeader) {
    std::printf("Failed to read camera calibration (invalid format?)\nCalibration file: %s\n", configFileName);
    return;
  }
  // the reference keeps whatever it parsed before bailing out (getInputDims() is
  // used by DatasetReader even for an invalid undistorter); its output size is
  // uninitialised in that case, ours is 0.
  for (int i = 0; i < 5; i++) calib_in_[i] = cam.in[i];
  in_w_ = cam.in_w;
  in_h_ = cam.in_h;
  if (lens.kind != 0) keep_lens_state(this, lens);
  if (pr != kParsed) return;
  if (lens.kind != 0 && !pick_output_intrinsics_lens(cam, lens, calib_out_)) {
    for (int i = 0; i < 5; i++) calib_out_[i] = 0;
    return;
  }
  out_w_ = cam.out_w;
  out_h_ = cam.out_h;
  valid_ = true;

  if (lens.kind == 0) pick_output_intrinsics(cam, calib_out_);

  // identity grid pushed through the lens model (:223-232)
  const int n = out_w_ * out_h_;
  remap_x_ = new float[n];
  remap_y_ = new float[n];
  for (int y = 0; y < out_h_; y++)
    for (int x = 0; x < out_w_; x++) {
      remap_x_[x + y * out_w_] = x;
      remap_y_[x + y * out_w_] = y;
    }
  if (lens.kind == 0) warp_points(calib_in_, in_w_, in_h_, calib_out_, out_w_, out_h_, remap_x_, remap_y_, n);
  else warp_points_lens(lens.kind, lens_model_of(lens.cam, lens.k, calib_out_, out_w_, out_h_), remap_x_, remap_y_, n);

  // border rules (:235-251): exact hits on the first/last row or column are
  // nudged inside; everything not strictly inside becomes the black sentinel.
  bool black = false;
  for (int i = 0; i < n; i++) {
    float& x = remap_x_[i];
    float& y = remap_y_[i];
    if (x == 0) x = 0.01;
    if (y == 0) y = 0.01;
    if (x == in_w_ - 1) x = in_w_ - 1.01;
    if (y == in_h_ - 1) y = in_h_ - 1.01;
    if (!(x > 0 && y > 0 && x < in_w_ - 1 && y < in_h_ - 1)) {
      black = true;
      x = -1;
      y = -1;
    }
  }
  if (black) std::printf("\n\nFOV Undistorter: Warning! Image has black pixels.\n\n\n");

  set_pinhole(k_rect_, calib_out_, out_w_, out_h_);
  set_pinhole(k_org_, calib_in_, in_w_, in_h_);

  // one-time upload; a missing GPU is reported here and again on every undistort()
  gpu_ = mdc_host::open_device_context("UndistorterFOV");
  if (gpu_ && mdc_set_remap(gpu_, remap_x_, remap_y_, in_w_, in_h_, out_w_, out_h_) != MDC_OK) {
    std::printf("UndistorterFOV: uploading the remap failed: %s\n", mdc_last_error(gpu_));
    mdc_destroy(gpu_);
    gpu_ = 0;
  }
}

UndistorterFOV::~UndistorterFOV() {
  drop_lens_state(this);
  if (gpu_) mdc_destroy(gpu_);
  delete[] remap_x_;
  delete[] remap_y_;
}

void UndistorterFOV::distortCoordinates(float* in_x, float* in_y, int n) {
  if (!valid_) {
    std::printf("ERROR: invalid UndistorterFOV!\n");
    return;
  }
  // Bulk callers (vignetteCalib: 10^6 plane points per image, src/main_vignetteCalib.cpp:284) go to the device: its kernel
  // restates the host libm's atanf and gives the same bits (csrc/fov_point_model.h; pinned on the CPU against this very
  // loop and on the GPU against the host).  Small counts stay here -- a launch and two copies cost more than the loop --,
  // and so does the constructor's table build, which calls warp_points directly.  MDC_DISTORT_GPU_MIN overrides the
  // threshold (0 = never on the device).
  static const long gpu_min = [] {
    const char* e = std::getenv("MDC_DISTORT_GPU_MIN");
    return e ? std::atol(e) : 65536l;
  }();
  const LensState* const ls = find_lens_state(this);
  if (ls) {
    // RadTan / EquiDistant: the same threshold; the bulk call is libmdc_lens.so's
    const mdc::LensModel lm = lens_model_of(ls->cam, ls->k, calib_out_, out_w_, out_h_);
    mdcn_model m;
    m.kind = ls->kind;
    m.fx = lm.fx, m.fy = lm.fy, m.cx = lm.cx, m.cy = lm.cy;
    for (int i = 0; i < 4; i++) m.k[i] = lm.k[i];
    m.in_w = in_w_, m.in_h = in_h_;
    m.ofx = lm.ofx, m.ofy = lm.ofy, m.ocx = lm.ocx, m.ocy = lm.ocy;
    m.out_w = out_w_, m.out_h = out_h_;
    if (bulk_points_on_device(g_lens, gpu_min, ls->kind == mdc::LENS_EQUIDISTANT ? &libm_is_the_restated_one : 0, gpu_, &m, in_x, in_y, n)) return;
    warp_points_lens(ls->kind, lm, in_x, in_y, n);
    return;
  }
  if (gpu_ && gpu_min > 0 && n >= gpu_min && libm_is_the_restated_one()) {
    mdc_fov_model m;
    for (int i = 0; i < 5; i++) {
      m.in_calib[i] = calib_in_[i];
      m.out_calib[i] = calib_out_[i];
    }
    m.in_w = in_w_;
    m.in_h = in_h_;
    m.out_w = out_w_;
    m.out_h = out_h_;
    if (mdc_distort_points_host(gpu_, &m, in_x, in_y, n) == MDC_OK) return;
    // the call leaves the coordinates untouched when it fails (they are copied back last): say so and do the work here
    std::fprintf(stderr, "UndistorterFOV::distortCoordinates: the GPU call failed (%s); computing %d points on the host\n", mdc_last_error(gpu_), n);
  }
  warp_points(calib_in_, in_w_, in_h_, calib_out_, out_w_, out_h_, in_x, in_y, n);
}

// ---- raw -> rectified points (csrc/lens_inverse_model.h holds the arithmetic) --------------------------------------------

namespace {

void unwarp_points(int kind, const mdc::LensInverseModel& m, float* xs, float* ys, long n) {
  if (kind == mdc::LENSINV_RADTAN)
    for (long i = 0; i < n; i++) mdc::lens_undistort_point<mdc::LENSINV_RADTAN>(m, xs[i], ys[i]);
  else if (kind == mdc::LENSINV_EQUIDISTANT)
    for (long i = 0; i < n; i++) mdc::lens_undistort_point<mdc::LENSINV_EQUIDISTANT>(m, xs[i], ys[i]);
  else
    for (long i = 0; i < n; i++) mdc::lens_undistort_point<mdc::LENSINV_FOV>(m, xs[i], ys[i]);
}

}  // namespace

void UndistorterFOV::undistortCoordinates(float* x, float* y, int n) {
  if (!valid_) {
    std::printf("ERROR: invalid UndistorterFOV!\n");
    return;
  }
  // The same rule as distortCoordinates: small counts run the loop here, bulk calls go to the device, whose kernel runs the same
  // header with the same flags (no libm is involved in this direction: the tangent is the header's own).  MDC_UNDISTORT_GPU_MIN
  // overrides the threshold (0 = never on the device).
  static const long gpu_min = [] {
    const char* e = std::getenv("MDC_UNDISTORT_GPU_MIN");
    return e ? std::atol(e) : 65536l;
  }();
  const LensState* const ls = find_lens_state(this);
  mdcu_model m;
  if (ls) {
    m.kind = ls->kind;  // MDCU_RADTAN / MDCU_EQUIDISTANT == the class's kinds
    m.fx = ls->cam[0], m.fy = ls->cam[1], m.cx = ls->cam[2], m.cy = ls->cam[3];
    for (int i = 0; i < 4; i++) m.k[i] = ls->k[i];
  } else {
    const InputModel im(calib_in_, in_w_, in_h_);
    m.kind = MDCU_FOV;
    m.fx = im.fx, m.fy = im.fy, m.cx = im.cx, m.cy = im.cy;
    m.k[0] = im.omega;
    m.k[1] = m.k[2] = m.k[3] = 0;
  }
  mdc::LensInverseModel lm;
  lm.fx = m.fx, lm.fy = m.fy, lm.cx = m.cx, lm.cy = m.cy;
  for (int i = 0; i < 4; i++) lm.k[i] = m.k[i];
  lm.d2t = m.kind == MDCU_FOV ? mdc::lens_inverse_d2t(m.k[0]) : 0.0f;
  lm.ofx = calib_out_[0] * out_w_;  // pixel units derived from the stored normalised values with lens_set_rectified's float steps
  lm.ofy = calib_out_[1] * out_h_;
  lm.ocx = calib_out_[2] * out_w_ - 0.5f;
  lm.ocy = calib_out_[3] * out_h_ - 0.5f;
  m.in_w = in_w_, m.in_h = in_h_;
  m.ofx = lm.ofx, m.ofy = lm.ofy, m.ocx = lm.ocx, m.ocy = lm.ocy;
  m.out_w = out_w_, m.out_h = out_h_;
  if (bulk_points_on_device(g_lensinv, gpu_min, 0, gpu_, &m, x, y, n)) return;
  unwarp_points(m.kind, lm, x, y, n);
}

namespace {
int run_undistort(mdc_ctx* g, const float* in, float* out, int n_in, int n_out) { return mdc_undistort_host_f32(g, in, out, n_in, n_out); }
int run_undistort(mdc_ctx* g, const unsigned char* in, float* out, int n_in, int n_out) { return mdc_undistort_host_u8(g, in, out, n_in, n_out); }
}  // namespace

template <typename T>
void UndistorterFOV::undistort(const T* input, float* output, int nPixIn, int nPixOut) const {
  if (!valid_) return;
  if (nPixIn != in_w_ * in_h_) {
    std::printf("ERROR: undistort called with wrong input image dismesions (expected %d pixel, got %d pixel)\n", in_w_ * in_h_, nPixIn);
    return;
  }
  if (nPixOut != out_w_ * out_h_) {
    std::printf("ERROR: undistort called with wrong output image dismesions (expected %d pixel, got %d pixel)\n", out_w_ * out_h_, nPixOut);
    return;
  }
  if (!gpu_) {
    std::fprintf(stderr, "ERROR: UndistorterFOV::undistort needs a gfx950 GPU (no HIP device context); output not written\n");
    return;
  }
  if (run_undistort(gpu_, input, output, nPixIn, nPixOut) != MDC_OK)
    std::fprintf(stderr, "ERROR: UndistorterFOV::undistort failed on the GPU: %s\n", mdc_last_error(gpu_));
}
template void UndistorterFOV::undistort<float>(const float*, float*, int, int) const;
template void UndistorterFOV::undistort<unsigned char>(const unsigned char*, float*, int, int) const;
