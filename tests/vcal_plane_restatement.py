"""Test-owned NumPy restatement of vignetteCalib's plane -> image coordinates (reference src/main_vignetteCalib.cpp:193-198,
:246-258), the arithmetic mdc_vcal_plane_coords_device claims bit for bit:

  K_p2idx^-1   Eigen's compute_inverse<3> in float: cofactors, det = c00 * m00 + (c10 * m10 + c20 * m20), Kinv(i, j) = c(j, i) * (1 / det)
  HK           float(H) * Kinv, a coefficient as a0 + (a1 + a2) (Eigen >= 3.3's unrolled sum of a lazy product)
  pp           HK * (x, y, 1) the same way, u = pp0 / pp2, v = pp1 / pp2
  H            the exact 4-point homography of the plane points (-0.5, 0.5), (0.5, 0.5), (0.5, -0.5), (-0.5, -0.5) onto the corners:
               the square-to-quad map in double, scaled to H(2,2) = 1

Every operation is an IEEE float32 / float64 add, multiply or divide, so NumPy's results are the device's.
Below them, a literal loop transcription of the same lines (one float32 operation at a time, Eigen's inverse and lazy product spelled out
coefficient by coefficient); tests/test_vcal_plane_coords.py holds the device's results against both."""
import numpy as np

f32 = np.float32
PLANE_POINTS = ((-0.5, 0.5), (0.5, 0.5), (0.5, -0.5), (-0.5, -0.5))  # :250-253


def k_p2idx(gw, gh, facw, fach):
    """:193-197 (gw / 2 is an int division)."""
    return np.array([[f32(gw) / f32(facw), 0, gw // 2], [0, f32(gh) / f32(fach), gh // 2], [0, 0, 1]], np.float32)


def k_inverse(gw, gh, facw, fach):
    m = k_p2idx(gw, gh, facw, fach)
    cof = np.zeros((3, 3), np.float32)
    for i in range(3):
        for j in range(3):
            i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
            cof[i, j] = m[i1, j1] * m[i2, j2] - m[i1, j2] * m[i2, j1]
    det = cof[0, 0] * m[0, 0] + (cof[1, 0] * m[1, 0] + cof[2, 0] * m[2, 0])
    invdet = f32(1) / det
    return (cof.T * invdet).astype(np.float32)


def homography(corners):
    """(n, 4, 2) corners -> (n, 3, 3) float32 H, formed in double (the order of the kernel's expressions)."""
    c = np.asarray(corners, np.float32).astype(np.float64)
    x0, y0, x1, y1, x2, y2, x3, y3 = (c[:, k // 2, k % 2] for k in range(8))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        sx, sy = x0 - x1 + x2 - x3, y0 - y1 + y2 - y3
        dx1, dx2, dy1, dy2 = x1 - x2, x3 - x2, y1 - y2, y3 - y2
        det = dx1 * dy2 - dx2 * dy1
        g, h = (sx * dy2 - dx2 * sy) / det, (dx1 * sy - sx * dy1) / det
        q0 = np.stack([x1 - x0 + g * x1, y1 - y0 + g * y1, g], 1)
        q1 = np.stack([x3 - x0 + h * x3, y3 - y0 + h * y3, h], 1)
        q2 = np.stack([x0, y0, np.ones_like(x0)], 1)
        s = (1.0 / (0.5 * g + 0.5 * h + 1.0))[:, None]
        H = np.stack([q0 * s, -q1 * s, (0.5 * q0 + 0.5 * q1 + q2) * s], 2)
    return H.astype(np.float32)


def hk_of(H, gw, gh, facw, fach):
    """(n, 3, 3) float32 H -> HK = H * K_p2idx^-1 in Eigen's float order."""
    H = np.asarray(H, np.float32)
    ki = k_inverse(gw, gh, facw, fach)
    with np.errstate(invalid="ignore", over="ignore"):
        return (H[:, :, 0, None] * ki[0][None, None, :] + (H[:, :, 1, None] * ki[1][None, None, :] + H[:, :, 2, None] * ki[2][None, None, :])).astype(np.float32)


def project(hk, gw, gh):
    """(n, 3, 3) float32 HK -> (u, v): (n, gw*gh) float32 each, plane point x + y * gw."""
    hk = np.asarray(hk, np.float32)
    y, x = np.divmod(np.arange(gw * gh, dtype=np.int64), gw)
    x, y, one = x.astype(np.float32)[None], y.astype(np.float32)[None], f32(1)
    K = [hk[:, i // 3, i % 3, None] for i in range(9)]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        pp0 = K[0] * x + (K[1] * y + K[2] * one)
        pp1 = K[3] * x + (K[4] * y + K[5] * one)
        pp2 = K[6] * x + (K[7] * y + K[8] * one)
        return (pp0 / pp2).astype(np.float32), (pp1 / pp2).astype(np.float32)


def plane_grid_points(gw, gh, facw, fach):
    """The grid coordinates (x, y) of the 4 plane points, in double: K_p2idx * (X, Y, 1)."""
    k = k_p2idx(gw, gh, facw, fach).astype(np.float64)
    return np.array([[k[0, 0] * X + k[0, 2], k[1, 1] * Y + k[1, 2]] for X, Y in PLANE_POINTS])


def random_corners(rng, n, w, h, side=(40, 400), tilt=0.3):
    """n convex quads inside a w x h frame: a square of the given side range, rotated, each corner moved by up to tilt * side / 2
    along the square's own axes (a perspective-looking view), in the order of the plane points (image y pointing down)."""
    out = np.zeros((n, 4, 2), np.float32)
    for i in range(n):
        s = rng.uniform(*side)
        a = rng.uniform(0, 2 * np.pi)
        R = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
        sq = np.array([[-0.5, -0.5], [0.5, -0.5], [0.5, 0.5], [-0.5, 0.5]]) * s  # image y down: plane Y up
        sq = sq + rng.uniform(-tilt / 2, tilt / 2, (4, 2)) * s
        r = 0.75 * s
        c = np.array([rng.uniform(r, w - r), rng.uniform(r, h - r)]) if w > 2 * r and h > 2 * r else np.array([w / 2, h / 2])
        out[i] = (sq @ R.T + c).astype(np.float32)
    return out


# ---- literal transcription of :193-198, :242-258 ------------------------------------------------------------------------------


def eigen_sum3(a0, a1, a2):
    """Eigen's unrolled redux of 3 terms: func(a0, func(a1, a2))."""
    return f32(a0 + f32(a1 + a2))


def literal_hk(Hd, gw, gh, facw, fach):
    """:193-198 and :242-256 (K_p2idx, its inverse, H as float, HK), one float32 operation at a time."""
    K = [[f32(1), f32(0), f32(0)], [f32(0), f32(1), f32(0)], [f32(0), f32(0), f32(1)]]  # Matrix3f::Identity()
    K[0][0] = f32(gw) / f32(facw)
    K[1][1] = f32(gh) / f32(fach)
    K[0][2] = f32(gw // 2)
    K[1][2] = f32(gh // 2)

    def cofactor(i, j):  # Eigen's cofactor_3x3<i, j>
        i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
        return f32(f32(K[i1][j1] * K[i2][j2]) - f32(K[i1][j2] * K[i2][j1]))

    col0 = [cofactor(0, 0), cofactor(1, 0), cofactor(2, 0)]
    det = eigen_sum3(col0[0] * K[0][0], col0[1] * K[1][0], col0[2] * K[2][0])
    invdet = f32(f32(1) / det)
    Kinv = [[None] * 3 for _ in range(3)]
    Kinv[0] = [f32(c * invdet) for c in col0]  # result.row(0) = cofactors_col0 * invdet
    for (i, j), (ci, cj) in {(1, 0): (0, 1), (1, 1): (1, 1), (2, 0): (0, 2), (2, 1): (1, 2), (2, 2): (2, 2), (1, 2): (2, 1),
                             (0, 2): (2, 0)}.items():
        Kinv[i][j] = f32(cofactor(ci, cj) * invdet)
    H = [[f32(Hd[i][j]) for j in range(3)] for i in range(3)]  # H(i, j) = Hcv.at<double>(i, j)
    return np.array([[eigen_sum3(H[i][0] * Kinv[0][j], H[i][1] * Kinv[1][j], H[i][2] * Kinv[2][j]) for j in range(3)] for i in range(3)],
                    np.float32)


def literal_points(HK, gw, gh, rows):
    """:246-258 for the plane rows `rows` (all of them: range(gh)) -> {idx: (plane2imgX, plane2imgY)}."""
    out = {}
    for y in rows:
        for x in range(gw):
            v = (f32(x), f32(y), f32(1))  # Eigen::Vector3f(x, y, 1)
            pp = [eigen_sum3(HK[r][0] * v[0], HK[r][1] * v[1], HK[r][2] * v[2]) for r in range(3)]
            out[x + y * gw] = (pp[0] / pp[2], pp[1] / pp[2])
    return out
