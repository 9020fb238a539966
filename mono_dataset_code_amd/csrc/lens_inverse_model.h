// The lens models of camera.txt run backwards -- a raw (distorted) pixel to the rectified image -- for the pinhole, FOV, RadTan and
// EquiDistant / KannalaBrandt cameras, applied to one point and written once for the device kernels (mdc_lensinv.hip), for the host
// class (host/fov_undistorter.cpp) and for the host compiler alone (tests/native/lens_inverse_core.cpp).  The forward direction is
// lens_point_model.h (RadTan, EquiDistant, pinhole) and fov_point_model.h (FOV).
//
// THE CONTRACT.  For a raw pixel (x', y'), the input camera (fx, fy, cx, cy, k[4]) and the rectified camera (ofx, ofy, ocx, ocy),
// all in pixels:
//
//   xd = (x' - cx) / fx;  yd = (y' - cy) / fy;
//   PINHOLE:     ix = xd;  iy = yd;
//   FOV:         (k[0] = omega; d2t = 2 tan(omega / 2), derived on the host as make_distort_model does, with the double tan)
//                rd = sqrtf(xd*xd + yd*yd);  a = rd * omega;  r = tanf_spec(a) / d2t;
//                s = (rd == 0 || omega == 0) ? 1 : r / rd;   ix = xd*s;  iy = yd*s;
//                if !(|a| < pio2_hi): ix = iy = NaN          (the point lies beyond the model's half plane)
//   EQUIDISTANT: (k = k1 k2 k3 k4; Newton on the angle, so there is no arctangent per step)
//                rd = sqrtf(xd*xd + yd*yd);  th = rd;
//                8 times:  t2 = th*th;
//                          f = th * (1 + t2*(k1 + t2*(k2 + t2*(k3 + t2*k4)))) - rd;
//                          d = 1 + t2*(3*k1 + t2*(5*k2 + t2*(7*k3 + t2*(9*k4))));
//                          th = th - f / d;
//                r = tanf_spec(th);  s = rd > 1e-8f ? r / rd : 1;   ix = xd*s;  iy = yd*s;
//                if !(0 <= th && th < pio2_hi): ix = iy = NaN
//   RADTAN:      (k = k1 k2 p1 p2; two-dimensional Newton on the forward polynomial of lens_point_model.h, Cramer's rule with one reciprocal of the determinant)
//                u = xd;  v = yd;
//                8 times:  mx2 = u*u; my2 = v*v; mxy = u*v; rho2 = mx2 + my2;
//                          rad = k1*rho2 + k2*rho2*rho2;   dr = k1 + 2*k2*rho2;              (dr = d rad / d rho2)
//                          gx = (u + u*rad + 2*p1*mxy + p2*(rho2 + 2*mx2)) - xd;
//                          gy = (v + v*rad + 2*p2*mxy + p1*(rho2 + 2*my2)) - yd;
//                          j11 = 1 + rad + 2*dr*mx2 + 2*p1*v + 6*p2*u;
//                          j22 = 1 + rad + 2*dr*my2 + 2*p2*u + 6*p1*v;
//                          j12 = 2*dr*mxy + 2*p1*u + 2*p2*v;                                 (= j21: the Jacobian is symmetric)
//                          inv = 1 / (j11*j22 - j12*j12);                                   (one reciprocal, then two products)
//                          u = u - (gx*j22 - gy*j12) * inv;   v = v - (gy*j11 - gx*j12) * inv;   (both from the step's old u, v)
//                ix = u;  iy = v;   if !(|u| < inf && |v| < inf): ix = iy = NaN
//   x = ofx*ix + ocx;   y = ofy*iy + ocy;
//
//   tanf_spec(x):  (this project's own tangent; the inverse is not in the reference, so there is no libm to match)
//                ax = |x|;  big = ax > pio4;  z = big ? (pio2_hi - ax) + pio2_lo : ax;  z2 = z*z;
//                q = c0 + z2*(c1 + z2*(c2 + z2*(c3 + z2*(c4 + z2*c5))));
//                t = z + z*(z2*q);            (the odd polynomial z * P(z2), P = 1 + z2*q, on |z| <= pi/4)
//                if big: t = 1 / t;           result = x < 0 ? -t : t
//                pio4 = hi[1], pio2_hi = hi[3], pio2_lo = lo[3] of atanf_host_libm's tables (fov_point_model.h); c0 .. c5 below: a
//                weighted least-squares fit of (tan z / z - 1) / z^2 in float64, rounded to float32.  Against float64 tan it stays
//                within 2.4 units in the last place on [2^-12, pi/2) (tests/test_lens_inverse_cpu.py sweeps it; the cap is 4).
//
// Every operation is an IEEE single-precision add / subtract / multiply / divide / sqrtf, products and sums associate left to right
// as written ((2*dr)*mx2, (k2*rho2)*rho2, (((1 + rad) + (2*dr)*mx2) + (2*p1)*v) + (6*p2)*u, ((u + u*rad) + (2*p1)*mxy) + p2*(...)),
// nothing is contracted into an FMA (both compilers run with -ffp-contract=off -fno-fast-math), sqrtf and '/' are correctly rounded on
// both sides: host and device give the same bits by construction.  The loops have the fixed trip count 8 and no exit on data; the
// only data-dependent constructs are the selects written above.  (The count is part of the contract, not "until nothing changes":
// the error against a float64 solve stops falling after 4 - 6 steps on every camera of tests/lens_problems.py, but RadTan never
// becomes bit-stable -- a few points flip a last bit between 10 and 12 steps.)  NaN in gives NaN out of both coordinates for FOV,
// EQUIDISTANT and RADTAN, and of the coordinate it came in on for PINHOLE.
#pragma once
#include "lens_point_model.h"

namespace mdc {

enum { LENSINV_PINHOLE = 0, LENSINV_RADTAN = 1, LENSINV_EQUIDISTANT = 2, LENSINV_FOV = 3 };  // == MDCU_* (include/mdc_lensinv.h)
enum { LENSINV_STEPS = 8 };

struct LensInverseModel {
  float fx, fy, cx, cy, k[4];  // input camera, pixels; FOV: k[0] = omega
  float d2t;                   // FOV only: 2 tan(omega / 2)
  float ofx, ofy, ocx, ocy;    // rectified camera, pixels
};

// d2t of an omega, make_distort_model's step: the double tan of the float half angle, the product narrowed.  Host only.
inline float lens_inverse_d2t(float omega) { return 2.0f * ::tan((double)(omega / 2.0f)); }

MDC_HD float tanf_spec(float x) {
  const float pio4 = 7.8539812565e-01f, pio2_hi = 1.5707962513e+00f, pio2_lo = 7.5497894159e-08f;
  const float c0 = 3.3333155513e-01f, c1 = 1.3338807225e-01f, c2 = 5.3410675377e-02f, c3 = 2.4432351813e-02f, c4 = 3.1162952073e-03f,
              c5 = 9.3875881284e-03f;
  const float ax = fabsf(x);
  const bool big = ax > pio4;
  const float z = big ? (pio2_hi - ax) + pio2_lo : ax;
  const float z2 = z * z;
  const float q = c0 + z2 * (c1 + z2 * (c2 + z2 * (c3 + z2 * (c4 + z2 * c5))));
  float t = z + z * (z2 * q);
  if (big) t = 1.0f / t;
  return x < 0 ? -t : t;
}

// (x, y) raw pixel -> rectified pixel, in place
template <int KIND>
MDC_HD void lens_undistort_point(const LensInverseModel& m, float& x, float& y) {
  const float pio2_hi = 1.5707962513e+00f;
  const float xd = (x - m.cx) / m.fx;
  const float yd = (y - m.cy) / m.fy;
  float ix, iy;
  bool outside = false;
  if (KIND == LENSINV_FOV) {
    const float omega = m.k[0];
    const float rd = sqrtf(xd * xd + yd * yd);  // correctly rounded (no fast-math)
    const float a = rd * omega;
    const float r = tanf_spec(a) / m.d2t;
    const float s = (rd == 0 || omega == 0) ? 1.0f : r / rd;
    ix = xd * s;
    iy = yd * s;
    outside = !(fabsf(a) < pio2_hi);
  } else if (KIND == LENSINV_EQUIDISTANT) {
    const float k1 = m.k[0], k2 = m.k[1], k3 = m.k[2], k4 = m.k[3];
    const float rd = sqrtf(xd * xd + yd * yd);
    float th = rd;
    for (int i = 0; i < LENSINV_STEPS; i++) {
      const float t2 = th * th;
      const float f = th * (1.0f + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4)))) - rd;
      const float d = 1.0f + t2 * (3.0f * k1 + t2 * (5.0f * k2 + t2 * (7.0f * k3 + t2 * (9.0f * k4))));
      th = th - f / d;
    }
    const float r = tanf_spec(th);
    const float s = rd > 1e-8f ? r / rd : 1.0f;
    ix = xd * s;
    iy = yd * s;
    outside = !(0 <= th && th < pio2_hi);
  } else if (KIND == LENSINV_RADTAN) {
    const float k1 = m.k[0], k2 = m.k[1], p1 = m.k[2], p2 = m.k[3];
    float u = xd, v = yd;
    for (int i = 0; i < LENSINV_STEPS; i++) {
      const float mx2 = u * u, my2 = v * v, mxy = u * v, rho2 = mx2 + my2;
      const float rad = k1 * rho2 + k2 * rho2 * rho2;
      const float dr = k1 + 2.0f * k2 * rho2;
      const float gx = (u + u * rad + 2.0f * p1 * mxy + p2 * (rho2 + 2.0f * mx2)) - xd;
      const float gy = (v + v * rad + 2.0f * p2 * mxy + p1 * (rho2 + 2.0f * my2)) - yd;
      const float j11 = 1.0f + rad + 2.0f * dr * mx2 + 2.0f * p1 * v + 6.0f * p2 * u;
      const float j22 = 1.0f + rad + 2.0f * dr * my2 + 2.0f * p2 * u + 6.0f * p1 * v;
      const float j12 = 2.0f * dr * mxy + 2.0f * p1 * u + 2.0f * p2 * v;
      const float inv = 1.0f / (j11 * j22 - j12 * j12);  // one divide a step instead of two: 15 % of the kernel's time
      const float du = (gx * j22 - gy * j12) * inv;
      const float dv = (gy * j11 - gx * j12) * inv;
      u = u - du;
      v = v - dv;
    }
    ix = u;
    iy = v;
    outside = !(fabsf(u) < INFINITY && fabsf(v) < INFINITY);
  } else {
    ix = xd;
    iy = yd;
  }
  x = m.ofx * ix + m.ocx;
  y = m.ofy * iy + m.ocy;
  if (outside) x = y = NAN;
}

MDC_HD void lens_undistort_point(int kind, const LensInverseModel& m, float& x, float& y) {
  if (kind == LENSINV_RADTAN) lens_undistort_point<LENSINV_RADTAN>(m, x, y);
  else if (kind == LENSINV_EQUIDISTANT) lens_undistort_point<LENSINV_EQUIDISTANT>(m, x, y);
  else if (kind == LENSINV_FOV) lens_undistort_point<LENSINV_FOV>(m, x, y);
  else lens_undistort_point<LENSINV_PINHOLE>(m, x, y);
}

}  // namespace mdc
