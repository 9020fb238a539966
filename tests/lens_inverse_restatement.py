"""The lens models run backwards (raw pixel -> rectified pixel) restated in NumPy float32, operation for operation from the CONTRACT
comment of csrc/lens_inverse_model.h and independently of its code: what tests/test_lens_inverse_cpu.py and
tests/test_lens_inverse.py compare the class, the stand-alone program and the kernels with, bit for bit.  Beside it a float64
reference inverse (Newton on lens_restatement.distort64 to convergence, the closed form tan for FOV) for the accuracy checks."""
import math

import numpy as np

import lens_restatement as R

F = np.float32
PINHOLE, RADTAN, EQUIDISTANT, FOV = 0, 1, 2, 3  # MDCU_*
STEPS = 8
PIO4, PIO2_HI, PIO2_LO = F(7.8539812565e-01), F(1.5707962513e+00), F(7.5497894159e-08)
TAN_C = tuple(F(v) for v in (3.3333155513e-01, 1.3338807225e-01, 5.3410675377e-02, 2.4432351813e-02, 3.1162952073e-03, 9.3875881284e-03))

# the FOV camera of SURVEY.md 8c (the sequence every frame test runs), relative units, and a small one for the tables
SURVEY_FOV = ("0.349153 0.436593 0.493140 0.499021 0.933271", "1280 1024", "0.4 0.53 0.5 0.5 0", "640 480")
SMALL_FOV = ("0.55 0.68 0.49 0.51 0.9", "96 80", "0.45 0.6 0.5 0.5 0", "64 48")


def tanf_spec(x):
    x = np.asarray(x, F)
    c0, c1, c2, c3, c4, c5 = TAN_C
    with np.errstate(all="ignore"):
        ax = np.abs(x)
        big = ax > PIO4
        z = np.where(big, (PIO2_HI - ax) + PIO2_LO, ax).astype(F)
        z2 = z * z
        q = c0 + z2 * (c1 + z2 * (c2 + z2 * (c3 + z2 * (c4 + z2 * c5))))
        t = z + z * (z2 * q)
        t = np.where(big, F(1) / t, t).astype(F)
        return np.where(x < 0, -t, t).astype(F)


def d2t_of(omega):
    """2 tan(omega / 2): the double tan of the float half angle, the product narrowed"""
    return F(2.0 * math.tan(float(F(omega) / F(2))))


def undistort(kind, cam, rect, x, y):
    """cam = (fx, fy, cx, cy, k0, k1, k2, k3), rect = (ofx, ofy, ocx, ocy), pixels; x, y float32 raw pixels -> rectified (x, y)"""
    fx, fy, cx, cy, k1, k2, k3, k4 = (F(v) for v in cam)
    ofx, ofy, ocx, ocy = (F(v) for v in rect)
    x, y = np.asarray(x, F), np.asarray(y, F)
    one, two = F(1), F(2)
    with np.errstate(all="ignore"):
        xd = (x - cx) / fx
        yd = (y - cy) / fy
        outside = np.zeros(x.shape, bool)
        if kind == FOV:
            omega = k1
            rd = np.sqrt(xd * xd + yd * yd)
            a = rd * omega
            r = tanf_spec(a) / d2t_of(omega)
            s = np.where((rd == 0) | (omega == 0), one, r / rd).astype(F)
            ix, iy = xd * s, yd * s
            outside = ~(np.abs(a) < PIO2_HI)
        elif kind == EQUIDISTANT:
            rd = np.sqrt(xd * xd + yd * yd)
            th = rd.copy()
            for _ in range(STEPS):
                t2 = th * th
                f = th * (one + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4)))) - rd
                d = one + t2 * (F(3) * k1 + t2 * (F(5) * k2 + t2 * (F(7) * k3 + t2 * (F(9) * k4))))
                th = th - f / d
            r = tanf_spec(th)
            s = np.where(rd > F(1e-8), r / rd, one).astype(F)
            ix, iy = xd * s, yd * s
            outside = ~((th >= 0) & (th < PIO2_HI))
        elif kind == RADTAN:
            p1, p2 = k3, k4
            u, v = xd.copy(), yd.copy()
            for _ in range(STEPS):
                mx2, my2, mxy = u * u, v * v, u * v
                rho2 = mx2 + my2
                rad = k1 * rho2 + k2 * rho2 * rho2
                dr = k1 + two * k2 * rho2
                gx = (u + u * rad + two * p1 * mxy + p2 * (rho2 + two * mx2)) - xd
                gy = (v + v * rad + two * p2 * mxy + p1 * (rho2 + two * my2)) - yd
                j11 = one + rad + two * dr * mx2 + two * p1 * v + F(6) * p2 * u
                j22 = one + rad + two * dr * my2 + two * p2 * u + F(6) * p1 * v
                j12 = two * dr * mxy + two * p1 * u + two * p2 * v
                inv = one / (j11 * j22 - j12 * j12)
                du = (gx * j22 - gy * j12) * inv
                dv = (gy * j11 - gx * j12) * inv
                u, v = u - du, v - dv
            ix, iy = u, v
            outside = ~((np.abs(u) < F(np.inf)) & (np.abs(v) < F(np.inf)))
        else:
            ix, iy = xd, yd
        ox, oy = (ofx * ix + ocx).astype(F), (ofy * iy + ocy).astype(F)
        ox[outside] = F(np.nan)
        oy[outside] = F(np.nan)
        return ox, oy


def undistort64(kind, cam, rect, x, y):
    """The float64 reference: -> (x, y, r) with r the normalised rectified radius; NaN where the model has no inverse (FOV /
    EquiDistant: an angle of pi/2 or more).  RadTan / EquiDistant: Newton on R.distort64 with a numerical Jacobian, 60 steps (far past
    convergence in float64 where it converges at all); FOV: the closed form."""
    cam64 = [float(F(v)) for v in cam]
    fx, fy, cx, cy = cam64[:4]
    ofx, ofy, ocx, ocy = (float(F(v)) for v in rect)
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    xd, yd = (x - cx) / fx, (y - cy) / fy
    with np.errstate(all="ignore"):
        if kind == FOV:
            omega = cam64[4]
            rd = np.hypot(xd, yd)
            if omega == 0:
                s = np.ones_like(rd)
            else:
                d2t = 2.0 * math.tan(omega / 2.0)
                s = np.where(rd == 0, 1.0, np.tan(rd * omega) / d2t / np.where(rd == 0, 1.0, rd))
                s = np.where(rd * omega < math.pi / 2, s, np.nan)
            ix, iy = xd * s, yd * s
        elif kind == EQUIDISTANT:
            k1, k2, k3, k4 = cam64[4:]
            rd = np.hypot(xd, yd)
            th = rd.copy()
            for _ in range(60):
                t2 = th * th
                f = th * (1 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4)))) - rd
                d = 1 + t2 * (3 * k1 + t2 * (5 * k2 + t2 * (7 * k3 + t2 * 9 * k4)))
                th = th - f / d
            s = np.where(rd > 1e-12, np.tan(th) / np.where(rd > 1e-12, rd, 1.0), 1.0)
            s = np.where((th >= 0) & (th < math.pi / 2), s, np.nan)
            ix, iy = xd * s, yd * s
        elif kind == RADTAN:
            ident = (1, 1, 0, 0)
            unit = [1.0, 1.0, 0.0, 0.0] + cam64[4:]  # distort64 with the identity cameras is the polynomial on normalised coordinates
            u, v = xd.copy(), yd.copy()
            h = 1e-6
            for _ in range(60):
                gx, gy = R.distort64(R.RADTAN, unit, ident, u, v)
                ax, ay = R.distort64(R.RADTAN, unit, ident, u + h, v)
                bx, by = R.distort64(R.RADTAN, unit, ident, u, v + h)
                j11, j21, j12, j22 = (ax - gx) / h, (ay - gy) / h, (bx - gx) / h, (by - gy) / h
                gx, gy = gx - xd, gy - yd
                det = j11 * j22 - j12 * j21
                u, v = u - (gx * j22 - gy * j12) / det, v - (gy * j11 - gx * j21) / det
            ix, iy = u, v
        else:
            ix, iy = xd, yd
        return ofx * ix + ocx, ofy * iy + ocy, np.hypot(ix, iy)


def fov_problem(lines, norm=None):
    """-> dict(kind, cam (pixels; k0 = omega), rect (pixels), sizes) of a bare five-number FOV line; `norm`: the object's stored
    normalised rectified intrinsics (UndistorterFOV.intrinsics()["out_calib"]) when line 3 is `crop` / `full`, else line 3 itself."""
    c = [F(v) for v in lines[0].split()]
    in_w, in_h = (int(v) for v in lines[1].split())
    out_w, out_h = (int(v) for v in lines[3].split())
    if norm is None:  # an explicit line 3: to pixels, and back to the normalised values the object stores (R.parse's steps)
        e = [F(v) for v in lines[2].split()]
        ofx, ofy = e[0] * F(out_w), e[1] * F(out_h)
        ocx, ocy = F(np.float64(e[2] * F(out_w)) - 0.5), F(np.float64(e[3] * F(out_h)) - 0.5)
        norm = (ofx / F(out_w), ofy / F(out_h), F((np.float64(ocx) + 0.5) / out_w), F((np.float64(ocy) + 0.5) / out_h))
    norm = [F(v) for v in norm]
    cam = (c[0] * F(in_w), c[1] * F(in_h), F(np.float64(c[2] * F(in_w)) - 0.5), F(np.float64(c[3] * F(in_h)) - 0.5), c[4], F(0), F(0), F(0))
    return {"kind": FOV, "cam": cam, "rect": R.rect_pixels(norm, out_w, out_h), "in_w": in_w, "in_h": in_h, "out_w": out_w, "out_h": out_h}


def inverse_problem(p):
    """a parsed lens_restatement problem (RadTan / EquiDistant) as an inverse problem: the kinds keep their values"""
    return {k: p[k] for k in ("kind", "cam", "rect", "in_w", "in_h", "out_w", "out_h")}


def raw_grid(q):
    y, x = np.mgrid[0:q["in_h"], 0:q["in_w"]]
    return x.astype(F).ravel(), y.astype(F).ravel()


def inverse_tables(q):
    """-> (ux, uy, outside): every raw pixel through the inverse, then the border rules against the OUTPUT size"""
    gx, gy = raw_grid(q)
    x, y = undistort(q["kind"], q["cam"], q["rect"], gx, gy)
    return R.border_rules(x, y, q["out_w"], q["out_h"])
