"""The RadTan / EquiDistant / pinhole lens models of camera.txt restated in NumPy float32, operation for operation from the
specification (the grammar, the point arithmetic, the `crop` search, the tables' border rules) and independently of the C++:
what tests/test_lens_cpu.py and tests/test_lens.py compare the class, the stand-alone program and the kernels with, bit for bit.

atanf is the C library's, called through ctypes element by element (tests/test_distort_points_cpu.py pins the product's
atanf_host_libm to it)."""
import ctypes
import ctypes.util
import math

import numpy as np

F = np.float32
FOV, RADTAN, EQUIDISTANT = 0, 1, 2
KEYWORDS = {"RadTan": RADTAN, "EquiDistant": EQUIDISTANT, "KannalaBrandt": EQUIDISTANT, "FOV": FOV, "Pinhole": FOV}

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.atanf.restype = ctypes.c_float
_libm.atanf.argtypes = [ctypes.c_float]


def atanf(a):
    a = np.asarray(a, F)
    out = np.empty(a.shape, F)
    flat_in, flat_out = a.ravel(), out.reshape(-1)
    for i in range(flat_in.size):
        flat_out[i] = _libm.atanf(float(flat_in[i]))
    return out


def distort(kind, cam, rect, x, y):
    """cam = (fx, fy, cx, cy, k0, k1, k2, k3), rect = (ofx, ofy, ocx, ocy), pixels; x, y float32 arrays -> (x', y').
    kind 0 here is the plain pinhole (no distortion term)."""
    fx, fy, cx, cy, k1, k2, k3, k4 = (F(v) for v in cam)
    ofx, ofy, ocx, ocy = (F(v) for v in rect)
    x, y = np.asarray(x, F), np.asarray(y, F)
    with np.errstate(all="ignore"):
        ix = (x - ocx) / ofx
        iy = (y - ocy) / ofy
        if kind == RADTAN:
            p1, p2 = k3, k4
            mx2, my2, mxy = ix * ix, iy * iy, ix * iy
            rho2 = mx2 + my2
            rad = k1 * rho2 + k2 * rho2 * rho2
            xd = ix + ix * rad + F(2) * p1 * mxy + p2 * (rho2 + F(2) * mx2)
            yd = iy + iy * rad + F(2) * p2 * mxy + p1 * (rho2 + F(2) * my2)
        elif kind == EQUIDISTANT:
            r = np.sqrt(ix * ix + iy * iy)
            th = atanf(r)
            t2 = th * th
            thd = th * (F(1) + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4))))
            s = np.where(r > F(1e-8), thd / r, F(1)).astype(F)
            xd, yd = ix * s, iy * s
        else:
            xd, yd = ix, iy
        return (fx * xd + cx).astype(F), (fy * yd + cy).astype(F)


def distort64(kind, cam, rect, x, y):
    """the same closed formulas in float64, for the restatement's own sanity check"""
    fx, fy, cx, cy, k1, k2, k3, k4 = (float(F(v)) for v in cam)
    ofx, ofy, ocx, ocy = (float(F(v)) for v in rect)
    ix = (np.asarray(x, np.float64) - ocx) / ofx
    iy = (np.asarray(y, np.float64) - ocy) / ofy
    if kind == RADTAN:
        p1, p2 = k3, k4
        rho2 = ix * ix + iy * iy
        rad = k1 * rho2 + k2 * rho2 * rho2
        xd = ix + ix * rad + 2 * p1 * ix * iy + p2 * (rho2 + 2 * ix * ix)
        yd = iy + iy * rad + 2 * p2 * ix * iy + p1 * (rho2 + 2 * iy * iy)
    elif kind == EQUIDISTANT:
        r = np.sqrt(ix * ix + iy * iy)
        th = np.arctan(r)
        t2 = th * th
        thd = th * (1 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4))))
        s = np.where(r > 1e-8, thd / np.where(r > 0, r, 1), 1.0)
        xd, yd = ix * s, iy * s
    else:
        xd, yd = ix, iy
    return fx * xd + cx, fy * yd + cy


def _inside(v, size):
    return (v > F(0)) & (v < F(size - 1))


def crop(kind, cam, in_w, in_h, out_w, out_h):
    """-> ((ofx, ofy, ocx, ocy), rounds) or (None, reason)"""
    if out_w < 2 or out_h < 2:
        return None, "size"
    ident = (1, 1, 0, 0)
    t = ((np.arange(100000, dtype=F) - F(50000.0)) / F(10000.0)).astype(F)
    zero = np.zeros_like(t)
    xs, _ = distort(kind, cam, ident, t, zero)
    _, ys = distort(kind, cam, ident, zero, t)
    ix, iy = np.flatnonzero(_inside(xs, in_w)), np.flatnonzero(_inside(ys, in_h))
    if ix.size == 0 or iy.size == 0:
        return None, "nothing inside"
    minX, maxX = t[ix[0]] * F(1.01), t[ix[-1]] * F(1.01)
    minY, maxY = t[iy[0]] * F(1.01), t[iy[-1]] * F(1.01)
    rounds = 0
    while True:
        py = (minY + (maxY - minY) * np.arange(out_h, dtype=F) / (F(out_h) - F(1.0))).astype(F)
        px = (minX + (maxX - minX) * np.arange(out_w, dtype=F) / (F(out_w) - F(1.0))).astype(F)
        left = not _inside(distort(kind, cam, ident, np.full(out_h, minX, F), py)[0], in_w).all()
        right = not _inside(distort(kind, cam, ident, np.full(out_h, maxX, F), py)[0], in_w).all()
        top = not _inside(distort(kind, cam, ident, px, np.full(out_w, minY, F))[1], in_h).all()
        bottom = not _inside(distort(kind, cam, ident, px, np.full(out_w, maxY, F))[1], in_h).all()
        if (left or right) and (top or bottom):
            if maxX - minX > maxY - minY:
                top = bottom = False
            else:
                left = right = False
        if not (left or right or top or bottom):
            break
        if left:
            minX = minX * F(0.995)
        if right:
            maxX = maxX * F(0.995)
        if top:
            minY = minY * F(0.995)
        if bottom:
            maxY = maxY * F(0.995)
        rounds += 1
        if rounds > 500:
            return None, "no convergence"
    ofx = (F(out_w) - F(1.0)) / (maxX - minX)
    ofy = (F(out_h) - F(1.0)) / (maxY - minY)
    return (ofx, ofy, -minX * ofx, -minY * ofy), rounds


def parse(lines):
    """The four lines of a keyword camera.txt of a new kind -> dict(valid, kind, cam (pixels, 8 floats), rel (relative fx fy cx cy),
    in_w, in_h, out_w, out_h, norm (normalised rectified intrinsics), rect (pixels), rounds, new_k (the printed line), message)."""
    out = {"valid": False, "kind": None, "in_w": 0, "in_h": 0, "out_w": 0, "out_h": 0, "rounds": None, "new_k": None, "message": None}
    bad_header = "Failed to read camera calibration (invalid format?)"
    words = lines[0].split()
    dims = lines[1].split()
    kind = KEYWORDS.get(words[0]) if words else None
    try:
        vals = [F(v) for v in words[1:]]
        in_w, in_h = int(dims[0]), int(dims[1])
    except (ValueError, IndexError):
        vals, in_w, in_h = None, 0, 0
    if kind in (None, FOV) or vals is None or len(vals) != 8 or not all(math.isfinite(float(v)) for v in vals) or vals[0] <= 0 or vals[1] <= 0:
        out["message"] = bad_header
        return out
    out.update(kind=kind, in_w=in_w, in_h=in_h)
    fx, fy, cx, cy = vals[:4]
    if cx < 1 and cy < 1:  # relative to the input size
        rel = (fx, fy, cx, cy)
        cam = (fx * F(in_w), fy * F(in_h), F(np.float64(cx * F(in_w)) - 0.5), F(np.float64(cy * F(in_h)) - 0.5))
    else:
        cam = (fx, fy, cx, cy)
        rel = (fx / F(in_w), fy / F(in_h), (cx + F(0.5)) / F(in_w), (cy + F(0.5)) / F(in_h))
    out["cam"] = tuple(cam) + tuple(vals[4:])
    out["rel"] = rel
    l3 = lines[2]
    if l3 == "none":
        out["message"] = "NO RECTIFICATION"
        return out
    if l3 == "full":
        out["message"] = "Out: Full is not implemented for this lens model... not rectifying."
        return out
    explicit = None
    if l3 != "crop":
        try:
            explicit = [F(v) for v in l3.split()]
        except ValueError:
            explicit = []
        if len(explicit) != 5:
            out["message"] = "Out: Failed to Read Output pars... not rectifying."
            return out
    try:
        out_w, out_h = (int(v) for v in lines[3].split()[:2])
    except ValueError:
        out["message"] = "Out: Failed to Read Output resolution... not rectifying."
        return out
    if explicit is None:
        rect, rounds = crop(kind, out["cam"], in_w, in_h, out_w, out_h)
        if rect is None:
            out["message"] = rounds
            return out
        out["rounds"] = rounds
        out["new_k"] = "new K: %f %f %f %f" % tuple(float(v) for v in rect)
        ofx, ofy, ocx, ocy = rect
    else:
        ofx, ofy = explicit[0] * F(out_w), explicit[1] * F(out_h)
        ocx, ocy = F(np.float64(explicit[2] * F(out_w)) - 0.5), F(np.float64(explicit[3] * F(out_h)) - 0.5)
    norm = (ofx / F(out_w), ofy / F(out_h), F((np.float64(ocx) + 0.5) / out_w), F((np.float64(ocy) + 0.5) / out_h))
    out.update(valid=True, out_w=out_w, out_h=out_h, norm=norm, rect=rect_pixels(norm, out_w, out_h))
    return out


def rect_pixels(norm, out_w, out_h):
    """the rectified camera in pixels every consumer derives from the stored normalised intrinsics"""
    return (norm[0] * F(out_w), norm[1] * F(out_h), norm[2] * F(out_w) - F(0.5), norm[3] * F(out_h) - F(0.5))


def k_rect(norm, out_w, out_h):
    """getK_rect(): the centre's - 0.5 is a double subtraction, narrowed"""
    k = np.eye(3, dtype=F)
    k[0, 0], k[1, 1] = norm[0] * F(out_w), norm[1] * F(out_h)
    k[0, 2], k[1, 2] = F(np.float64(norm[2] * F(out_w)) - 0.5), F(np.float64(norm[3] * F(out_h)) - 0.5)
    return k


def grid(out_w, out_h):
    y, x = np.mgrid[0:out_h, 0:out_w]
    return x.astype(F).ravel(), y.astype(F).ravel()


def tables(p):
    """-> (remap_x, remap_y, black) of a parsed, valid camera: the identity grid through the model, then the border rules"""
    gx, gy = grid(p["out_w"], p["out_h"])
    x, y = distort(p["kind"], p["cam"], p["rect"], gx, gy)
    return border_rules(x, y, p["in_w"], p["in_h"])


def border_rules(x, y, in_w, in_h):
    x, y = x.copy(), y.copy()
    x[x == F(0)] = F(0.01)
    y[y == F(0)] = F(0.01)
    x[x == F(in_w - 1)] = F(in_w - 1.01)
    y[y == F(in_h - 1)] = F(in_h - 1.01)
    with np.errstate(invalid="ignore"):
        black = ~((x > 0) & (y > 0) & (x < F(in_w - 1)) & (y < F(in_h - 1)))
    x[black] = F(-1)
    y[black] = F(-1)
    return x, y, bool(black.any())
