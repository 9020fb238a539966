"""Problems for the vignetteCalib tests (tests/test_vcal_cpu.py, tests/test_vcal_sizes.py) and the facts about them that the
kernels' results must match: which samples the contribution index lists, how long each group of 64 bins is, and the
compacted form of a problem whose only valid samples are a few (image, plane point) pairs."""
import numpy as np

SLACK_ROWS = 8  # kVcalSlackRows: rows of slack after the lists
ENTRY_BYTES = 16  # sizeof(VcalEntry)


def listed(images, p2x, p2y):
    """The samples the kernels keep (mdc_vcal.hip vcal_sample): coordinate present, 2x2 footprint inside the image (float32
    comparisons, as the kernels make them), all four colour taps non-NaN.  -> (mask (n, np), pixel index ix + iy*w of each
    listed sample, in (image, plane point) order)."""
    n, h, w = images.shape
    with np.errstate(invalid="ignore"):
        inside = (p2x >= 0) & (p2y >= 0) & (p2x < np.float32(w - 1)) & (p2y < np.float32(h - 1))
    ii, pp = np.nonzero(inside)
    b = p2x[ii, pp].astype(np.int64) + p2y[ii, pp].astype(np.int64) * w
    img = images.reshape(n, -1)
    ok = ~(np.isnan(img[ii, b]) | np.isnan(img[ii, b + 1]) | np.isnan(img[ii, b + w]) | np.isnan(img[ii, b + w + 1]))
    mask = np.zeros(inside.shape, bool)
    mask[ii[ok], pp[ok]] = True
    return mask, b[ok]


def bin_counts(b, w, h):
    """entries per image pixel: each listed sample at pixel b adds one to b, b+1, b+w, b+w+1"""
    nb = w * h
    return sum(np.bincount(b + d, minlength=nb) for d in (0, 1, w, w + 1))


def group_rows(counts):
    """rows per group of 64 bins = its longest list (ELL packing)"""
    g = -(-counts.size // 64)
    pad = np.zeros(g * 64, np.int64)
    pad[:counts.size] = counts
    return pad.reshape(g, 64).max(axis=1)


def index_bytes(rows):
    """mdc_vcal_index_bytes for a list of rows rows in all"""
    return (int(rows) + SLACK_ROWS) * 64 * ENTRY_BYTES


def oracle_view(p2x, p2y, mask):
    """The coordinates as the reference's caller would hand them over (:283-300): NaN wherever a sample is not listed.  The
    reference reads out of bounds for a sample whose footprint leaves the image; the kernels drop it; a sample with a NaN colour
    tap is skipped by both sides either way."""
    return np.where(mask, p2x, np.float32(np.nan)), np.where(mask, p2y, np.float32(np.nan))


def compact(images, p2x, p2y, imgs, pts):
    """the problem restricted to images `imgs` and plane points `pts` (both ascending)"""
    return (np.ascontiguousarray(images[imgs]), np.ascontiguousarray(p2x[np.ix_(imgs, pts)]),
            np.ascontiguousarray(p2y[np.ix_(imgs, pts)]))


def pattern(u, v):
    return 60.0 + 40.0 * np.sin(7.0 * u) * np.cos(5.0 * v)


def smooth_problem(seed, n, w, h, gw, gh, warp=0.0, nan_px=0.01, nan_pt=0.02, noise=6.0):
    """n views of a gw x gh calibration plane on w x h images.  Plane point (u, v) in [0, 1]^2 lands at
        x = ox + sx u + warp sx u v,   y = oy + sy v + warp sy u (1 - u)
    (non-affine for warp != 0), spread a little past the image so that some footprints leave it; a fraction nan_pt of the
    samples has no coordinate, nan_px of the pixels is NaN.  The images show the plane pattern through a vignette (the warp
    inverted approximately) plus noise, so the outlier threshold of the solver's second half cuts some samples and not others.
    -> images (n, h, w), p2x, p2y (n, gw*gh) float32."""
    rng = np.random.default_rng(seed)
    gy, gx = np.mgrid[0:gh, 0:gw]
    u = (gx / max(gw - 1, 1)).reshape(-1)
    v = (gy / max(gh - 1, 1)).reshape(-1)
    Y, X = np.mgrid[0:h, 0:w].astype(np.float64)
    r2 = ((X - w / 2) ** 2 + (Y - h / 2) ** 2) / (w * w / 4.0 + h * h / 4.0)
    vig = 1.0 - 0.45 * r2
    images = np.empty((n, h, w), np.float32)
    p2x = np.empty((n, gw * gh), np.float32)
    p2y = np.empty((n, gw * gh), np.float32)
    for i in range(n):
        sx, sy = (w - 1) * rng.uniform(0.9, 1.04), (h - 1) * rng.uniform(0.9, 1.04)
        ox, oy = (w - 1) * rng.uniform(-0.03, 0.06), (h - 1) * rng.uniform(-0.03, 0.06)
        px = ox + sx * u + warp * sx * u * v
        py = oy + sy * v + warp * sy * u * (1 - u)
        bad = rng.random(u.size) < nan_pt
        px[bad] = np.nan
        py[bad] = np.nan
        p2x[i], p2y[i] = px, py
        uu = (X - ox) / sx
        vv = (Y - oy) / sy
        for _ in range(3):  # invert the warp (a few fixed-point steps)
            uu = (X - ox) / (sx * (1 + warp * vv))
            vv = (Y - oy - warp * sy * uu * (1 - uu)) / sy
        img = pattern(uu, vv) * vig + rng.normal(0, noise, (h, w))
        img[rng.random((h, w)) < nan_px] = np.nan
        images[i] = img
    return images, p2x, p2y
