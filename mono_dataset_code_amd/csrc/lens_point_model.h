// The lens models of DSO's camera.txt grammar beside FOV -- RadTan (OpenCV's radial-tangential polynomial), EquiDistant (the
// Kannala-Brandt fisheye polynomial; DSO's two names "EquiDistant" and "KannalaBrandt" are this one arithmetic) and the plain
// pinhole -- applied to one point, written once for the device kernels (mdc_lens.hip), for the host class (host/fov_undistorter.cpp)
// and for the host compiler alone (tests/native/lens_core.cpp).
//
// THE CONTRACT.  For a rectified pixel (x, y), the rectified camera (ofx, ofy, ocx, ocy) and the input camera (fx, fy, cx, cy,
// k[4]), all in pixels:
//
//   ix = (x - ocx) / ofx;  iy = (y - ocy) / ofy;
//   PINHOLE:     xd = ix;  yd = iy;
//   RADTAN:      (k = k1 k2 p1 p2)
//                mx2 = ix*ix; my2 = iy*iy; mxy = ix*iy; rho2 = mx2 + my2;
//                rad = k1*rho2 + k2*rho2*rho2;
//                xd = ix + ix*rad + 2*p1*mxy + p2*(rho2 + 2*mx2);
//                yd = iy + iy*rad + 2*p2*mxy + p1*(rho2 + 2*my2);
//   EQUIDISTANT: (k = k1 k2 k3 k4)
//                r = sqrtf(ix*ix + iy*iy); th = atanf_host_libm(r); t2 = th*th;
//                thd = th * (1 + t2*(k1 + t2*(k2 + t2*(k3 + t2*k4))));
//                s = r > 1e-8f ? thd / r : 1;   xd = ix*s;  yd = iy*s;
//   x' = fx*xd + cx;   y' = fy*yd + cy;
//
// Every operation is an IEEE single-precision add / multiply / divide / sqrtf, the products and sums associate left to right as
// written ((2*p1)*mxy, (k2*rho2)*rho2, ((ix + ix*rad) + (2*p1)*mxy) + p2*(...)), nothing is contracted into an FMA (both compilers
// run with -ffp-contract=off -fno-fast-math), sqrtf and '/' are correctly rounded on both sides and atanf_host_libm is the restated
// host libm of fov_point_model.h: host and device give the same bits by construction.  NaN in gives NaN out of the coordinate it
// came in on (and of both, for RADTAN); nothing here branches on data except the r > 1e-8f guard.
//
// The automatic `crop` intrinsics (lens_crop below) are host-only, sequential and one-time; they go through the same point function.
#pragma once
#include "fov_point_model.h"

namespace mdc {

enum { LENS_PINHOLE = 0, LENS_RADTAN = 1, LENS_EQUIDISTANT = 2 };  // == MDCN_PINHOLE / _RADTAN / _EQUIDISTANT (include/mdc_lens.h)

struct LensModel {
  float fx, fy, cx, cy, k[4];  // input camera, pixels
  float ofx, ofy, ocx, ocy;    // rectified camera, pixels
};

// The rectified camera in pixels from the normalised intrinsics the class stores, with make_distort_model's float steps.
inline void lens_set_rectified(LensModel& m, const float out_calib[5], int out_w, int out_h) {
  m.ofx = out_calib[0] * out_w;
  m.ofy = out_calib[1] * out_h;
  m.ocx = out_calib[2] * out_w - 0.5f;
  m.ocy = out_calib[3] * out_h - 0.5f;
}

// (x, y) rectified pixel -> raw pixel, in place
template <int KIND>
MDC_HD void lens_distort_point(const LensModel& m, float& x, float& y) {
  const float ix = (x - m.ocx) / m.ofx;
  const float iy = (y - m.ocy) / m.ofy;
  float xd, yd;
  if (KIND == LENS_RADTAN) {
    const float k1 = m.k[0], k2 = m.k[1], p1 = m.k[2], p2 = m.k[3];
    const float mx2 = ix * ix, my2 = iy * iy, mxy = ix * iy, rho2 = mx2 + my2;
    const float rad = k1 * rho2 + k2 * rho2 * rho2;
    xd = ix + ix * rad + 2.0f * p1 * mxy + p2 * (rho2 + 2.0f * mx2);
    yd = iy + iy * rad + 2.0f * p2 * mxy + p1 * (rho2 + 2.0f * my2);
  } else if (KIND == LENS_EQUIDISTANT) {
    const float r = sqrtf(ix * ix + iy * iy);  // correctly rounded (no fast-math)
    const float th = atanf_host_libm(r);
    const float t2 = th * th;
    const float thd = th * (1.0f + t2 * (m.k[0] + t2 * (m.k[1] + t2 * (m.k[2] + t2 * m.k[3]))));
    const float s = r > 1e-8f ? thd / r : 1.0f;
    xd = ix * s;
    yd = iy * s;
  } else {
    xd = ix;
    yd = iy;
  }
  x = m.fx * xd + m.cx;
  y = m.fy * yd + m.cy;
}

MDC_HD void lens_distort_point(int kind, const LensModel& m, float& x, float& y) {
  if (kind == LENS_RADTAN) lens_distort_point<LENS_RADTAN>(m, x, y);
  else if (kind == LENS_EQUIDISTANT) lens_distort_point<LENS_EQUIDISTANT>(m, x, y);
  else lens_distort_point<LENS_PINHOLE>(m, x, y);
}

// The remap tables' border rules on one entry (host/fov_undistorter.cpp, reference src/FOVUndistorter.cpp:235-251): an exact hit on
// the first / last row or column is nudged inside, everything not strictly inside becomes the black sentinel.  lo = (float)0.01,
// hi_x = (float)(in_w - 1.01), hi_y = (float)(in_h - 1.01), narrowed from double by the caller on the host.  true: it went black.
MDC_HD bool lens_border_rule(float& x, float& y, int in_w, int in_h, float lo, float hi_x, float hi_y) {
  if (x == 0) x = lo;
  if (y == 0) y = lo;
  if (x == in_w - 1) x = hi_x;
  if (y == in_h - 1) y = hi_y;
  if (!(x > 0 && y > 0 && x < in_w - 1 && y < in_h - 1)) {
    x = -1;
    y = -1;
    return true;
  }
  return false;
}

// ---- `crop`: the largest rectified rectangle without black pixels, DSO's search ----------------------------------------------
// With the identity rectified camera (ofx = ofy = 1, ocx = ocy = 0) a "rectified pixel" is a normalised image coordinate.
//  1. coarse extent: t_i = (i - 50000.0f) / 10000.0f, i = 0 .. 99999; minX / maxX = the first / last t_i whose (t_i, 0) lands with
//     x' strictly inside (0, in_w - 1); minY / maxY the same with (0, t_i) and y' against (0, in_h - 1); all four times 1.01f.
//  2. rounds: the out_h points of the left and of the right side, (minX | maxX, minY + (maxY - minY) * (float)y / ((float)out_h - 1.0f)),
//     a side is out if any x' is not strictly inside (0, in_w - 1); the out_w points of the top and bottom sides against
//     (0, in_h - 1) likewise.  If a horizontal and a vertical side are both out only the wider dimension shrinks (left / right when
//     maxX - minX > maxY - minY, else top / bottom).  Each side that is out is multiplied by 0.995f.  A round is one pass that
//     shrank something; the search ends with the first pass in which no side is out.  More than 500 rounds: failure.
//  3. ofx = (out_w - 1.0f) / (maxX - minX), ofy = (out_h - 1.0f) / (maxY - minY), ocx = -minX * ofx, ocy = -minY * ofy.
struct LensCrop {
  float ofx, ofy, ocx, ocy;  // pixels
  int rounds;
};
enum { LENS_CROP_OK = 0, LENS_CROP_SIZE = 1, LENS_CROP_NOTHING_INSIDE = 2, LENS_CROP_NO_CONVERGENCE = 3 };

inline int lens_crop(int kind, const LensModel& input, int in_w, int in_h, int out_w, int out_h, LensCrop* out) {
  if (out_w < 2 || out_h < 2) return LENS_CROP_SIZE;
  LensModel m = input;
  m.ofx = m.ofy = 1.0f;
  m.ocx = m.ocy = 0.0f;
  const float wlim = (float)(in_w - 1), hlim = (float)(in_h - 1);
  float minX = 0, maxX = 0, minY = 0, maxY = 0;
  bool anyX = false, anyY = false;
  for (int i = 0; i < 100000; i++) {
    const float t = ((float)i - 50000.0f) / 10000.0f;
    float x = t, y = 0.0f;
    lens_distort_point(kind, m, x, y);
    if (x > 0 && x < wlim) {
      if (!anyX) minX = t;
      maxX = t;
      anyX = true;
    }
    x = 0.0f;
    y = t;
    lens_distort_point(kind, m, x, y);
    if (y > 0 && y < hlim) {
      if (!anyY) minY = t;
      maxY = t;
      anyY = true;
    }
  }
  if (!anyX || !anyY) return LENS_CROP_NOTHING_INSIDE;
  minX *= 1.01f;
  maxX *= 1.01f;
  minY *= 1.01f;
  maxY *= 1.01f;

  bool left = true, right = true, top = true, bottom = true;
  int rounds = 0;
  while (left || right || top || bottom) {
    left = right = top = bottom = false;
    for (int y = 0; y < out_h; y++) {
      const float py = minY + (maxY - minY) * (float)y / ((float)out_h - 1.0f);
      float ax = minX, ay = py, bx = maxX, by = py;
      lens_distort_point(kind, m, ax, ay);
      lens_distort_point(kind, m, bx, by);
      if (!(ax > 0 && ax < wlim)) left = true;
      if (!(bx > 0 && bx < wlim)) right = true;
    }
    for (int x = 0; x < out_w; x++) {
      const float px = minX + (maxX - minX) * (float)x / ((float)out_w - 1.0f);
      float ax = px, ay = minY, bx = px, by = maxY;
      lens_distort_point(kind, m, ax, ay);
      lens_distort_point(kind, m, bx, by);
      if (!(ay > 0 && ay < hlim)) top = true;
      if (!(by > 0 && by < hlim)) bottom = true;
    }
    if ((left || right) && (top || bottom)) {
      if (maxX - minX > maxY - minY) top = bottom = false;
      else left = right = false;
    }
    if (!(left || right || top || bottom)) break;
    if (left) minX *= 0.995f;
    if (right) maxX *= 0.995f;
    if (top) minY *= 0.995f;
    if (bottom) maxY *= 0.995f;
    if (++rounds > 500) return LENS_CROP_NO_CONVERGENCE;
  }
  out->ofx = ((float)out_w - 1.0f) / (maxX - minX);
  out->ofy = ((float)out_h - 1.0f) / (maxY - minY);
  out->ocx = -minX * out->ofx;
  out->ocy = -minY * out->ofy;
  out->rounds = rounds;
  return LENS_CROP_OK;
}

}  // namespace mdc
