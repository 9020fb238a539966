"""vignetteCalib's kernels (mono_dataset_code_amd/csrc/mdc_vcal.hip) at, below and past every size-dependent branch and index-width
limit, against the C oracle (oracle/mdc_oracle.c, pinned to the reference's own loops in tests/test_vcal.py):

  scan passes of 1024 groups      groups of 64 bins per pass of vcal_index_scan_kernel, carried in s_carry
                                  (1023 / 1024 / 1025 / 2048 / 2049 groups, nbins % 64 in {0, 1, 63}, 1280x1024 = 20480)
  kVcalSlackRows = 8              rows per step of vcal_vignette_gather_kernel, reading into the next group / the slack
                                  (group lengths 0, 1, 7, 8, 9, 15, 16, 17, >= 10^4; ngroups % 4 = 0..3: the partial last workgroup)
  image edges                     footprints at x = 0, y = 0, -0.0, nextafter(w-1, 0), nextafter(h-1, 0) kept; x = w-1, -tiny dropped
                                  by all three paths; 2xh, wx2, 2x2 images: the clamped 3x3 neighbourhood V of the gather
  per-image insertion sort        vcal_index_sort_kernel over >= 32 samples of one image in one bin, plane points numbered at random
  pc = point | corner << 30       n_plane = 2^30 - 1 accepted (its last point listed: corner 3 packs to 0xFFFFFFFE), 2^30 refused
  slots (gbase + k) * 64 + lane   lists past 2^32 bytes and past 2^32 slots (ELL padding, one heavy bin per group)
  stack offsets                   65535 images of 33024 pixels: 2.16e9 elements, 8.7 GB; p2x / p2y 65535 x 40000
  gradient mask y += 256          w = 1280, 1284 (one trip), 1285, 1290, 2048 (two): fronts of more than 256 rows
  grid y = n_images               65535 accepted, 65536 refused by the atomic step, the index, the scaling and the solve
  w * h < 2^31                    refused past it by the plane step and the atomic step too

Bit-identical: plane step, indexed vignette step, solve, gradient mask, coordinate mask, smoothing, scaling.  The atomic vignette
step within 1e-5.  E within 1e-9 relative (tree order against the oracle's sequential sum), R exactly.  The oracle does not drop
samples whose footprint leaves the image, so it sees those masked (vcal_problems.oracle_view).  The stacks too large for the host
are built sparse on the device: only a few (image, plane point) pairs hold coordinates, the other images a sentinel; the oracle runs
on the compacted problem, which gives the same bits (tests/test_vcal_cpu.py).  Large cases are sized from the free device memory
and skipped, saying why, when it is short."""
import ctypes as C

import numpy as np
import pytest

import vcal_problems as P
from conftest import bits_equal

pytestmark = pytest.mark.gpu

BIG_OTH2 = 10000 * 10000
SENTINEL = 1e30
GiB = 2.0 ** 30


@pytest.fixture(scope="module")
def ctx():
    from mono_dataset_code_amd import capi

    return capi.Context(0)


@pytest.fixture(autouse=True)
def _release():
    yield
    import gc

    import torch

    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def need(nbytes, what):
    """skip unless nbytes (+10 %) are free on the device"""
    import torch

    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if 1.1 * nbytes > free:
        pytest.skip("%s needs %.1f GiB + 10 %% of device memory, %.1f GiB free" % (what, nbytes / GiB, free / GiB))


def oth2_of(it, iters, th=15):
    return BIG_OTH2 if it < iters // 2 else th * th  # :397-398


def close_e(e, e_o):
    return abs(e - e_o) <= 1e-9 * abs(e_o) + 1e-9


def check_atomic(ctx, d_img, d_x, d_y, d_pc, d_vf, oth2, want):
    """the atomic vignette step on a copy of d_vf against the oracle's (vf, tt, ct, e, r): 1e-5"""
    vf_o, tt_o, ct_o, e_o, r_o = want
    d_vf_a = d_vf.clone()
    tt, ct, e, r = ctx.vcal_vignette_step(d_img, d_x, d_y, d_pc, d_vf_a, oth2)
    assert r == r_o and abs(e - e_o) <= 1e-6 * abs(e_o) + 1e-6, (e, e_o, r, r_o)
    for name, got, w in (("tt", host(tt), tt_o), ("ct", host(ct), ct_o), ("vf", host(d_vf_a), vf_o)):
        m = ~np.isnan(w)
        g = ~np.isnan(got)
        flip = m != g  # only where TT sits on the threshold 1 (summation order)
        assert np.all(np.abs(tt_o[flip] - 1) <= 1e-5), (name, np.flatnonzero(flip)[:8])
        both = m & g
        assert np.allclose(got[both], w[both], rtol=1e-5, atol=1e-6), (name, np.abs(got[both] - w[both]).max())


class Oracle:
    """the oracle's alternating iteration, remembered step by step"""

    def __init__(self, oracle, images, ox, oy, iters, th=15):
        n, h, w = images.shape
        pc = np.zeros(ox.shape[1], np.float32)
        vf = np.ones(h * w, np.float32)
        self.steps = []
        for it in range(iters):
            oth2 = oth2_of(it, iters, th)
            pc, ff, fc, e1, r1 = oracle.vcal_plane_step(images, ox, oy, pc, vf, oth2)
            vf, tt, ct, e2, r2 = oracle.vcal_vignette_step(images, ox, oy, pc, vf, oth2)
            self.steps.append(dict(oth2=oth2, pc=pc, ff=ff, fc=fc, e1=e1, r1=r1, vf=vf, tt=tt, ct=ct, e2=e2, r2=r2))
        self.pc, self.vf = pc, vf


def check_steps(ctx, want, d_img, d_x, d_y, index, keep=None, atomic_iters=()):
    """The device iteration (plane step + indexed vignette step) from colours 0, factors 1, against the oracle's steps.  keep: the
    device plane points the oracle's compacted problem holds (None = all); the others must end with FF = FC = 0 and a NaN colour.
    atomic_iters: iterations at which the atomic step also runs (on a copy of the factors)."""
    import torch

    npd = d_x.shape[1]
    h, w = d_img.shape[1], d_img.shape[2]
    d_keep = None if keep is None else dev(np.asarray(keep, np.int64))
    d_pc = torch.zeros(npd, dtype=torch.float32, device="cuda")
    d_vf = torch.ones(h * w, dtype=torch.float32, device="cuda")
    sel = (lambda t: host(t)) if keep is None else (lambda t: host(t[d_keep]))
    for it, s in enumerate(want.steps):
        ff, fc, e, r = ctx.vcal_plane_step(d_img, d_x, d_y, d_pc, d_vf, s["oth2"])
        assert bits_equal(sel(ff), s["ff"]) and bits_equal(sel(fc), s["fc"]), (it, "FF FC")
        assert bits_equal(sel(d_pc), s["pc"]), (it, "planeColor")
        assert r == s["r1"] and close_e(e, s["e1"]), (it, e, s["e1"], r, s["r1"])
        if keep is not None:  # the points without a sample, on the device
            k = int(d_keep.numel())
            assert int(torch.count_nonzero(ff)) == int(torch.count_nonzero(ff[d_keep])) and int(torch.count_nonzero(fc)) == int(
                torch.count_nonzero(fc[d_keep])), it
            assert int(torch.isnan(d_pc).sum()) == npd - k + int(np.isnan(s["pc"]).sum()), it
        del ff, fc
        if it in atomic_iters:
            check_atomic(ctx, d_img, d_x, d_y, d_pc, d_vf, s["oth2"], (s["vf"], s["tt"], s["ct"], s["e2"], s["r2"]))
        tt, ct, e, r = ctx.vcal_vignette_step_indexed(index, d_pc, d_vf, s["oth2"])
        assert bits_equal(host(tt), s["tt"]) and bits_equal(host(ct), s["ct"]), (it, "TT CT")
        assert bits_equal(host(d_vf), s["vf"]), (it, "vignetteFactor")
        assert r == s["r2"] and close_e(e, s["e2"]), (it, e, s["e2"], r, s["r2"])
    return d_pc, d_vf


def check_solve(ctx, want, d_img, d_x, d_y, keep=None):
    import torch

    npd = d_x.shape[1]
    h, w = d_img.shape[1], d_img.shape[2]
    iters = len(want.steps)
    d_pc = torch.zeros(npd, dtype=torch.float32, device="cuda")
    d_vf = torch.ones(h * w, dtype=torch.float32, device="cuda")
    er = ctx.vcal_solve(d_img, d_x, d_y, d_pc, d_vf, iters, 15)
    got_pc = host(d_pc) if keep is None else host(d_pc[dev(np.asarray(keep, np.int64))])
    assert bits_equal(got_pc, want.pc) and bits_equal(host(d_vf), want.vf)
    for it, s in enumerate(want.steps):
        assert er[it, 1] == s["r1"] and er[it, 3] == s["r2"], it
        assert close_e(er[it, 0], s["e1"]) and close_e(er[it, 2], s["e2"]), it


def check_index(ctx, d_img, d_x, d_y, images, ox, oy):
    """index over the device arrays; entries and bytes from the (compacted) host problem, exactly -> (index, rows)"""
    n, h, w = images.shape
    mask, b = P.listed(images, ox, oy)
    rows = P.group_rows(P.bin_counts(b, w, h))
    index = ctx.vcal_index(d_img, d_x, d_y)
    assert index.entries == 4 * b.size, (index.entries, 4 * b.size)
    assert index.bytes == P.index_bytes(rows.sum()), (index.bytes, rows.sum())
    return index, rows


def dense_case(ctx, oracle, images, p2x, p2y, iters=4, atomic_iters=(), reps=1):
    """a problem held whole on both sides: GPU arrays as given (footprints leaving the image included), the oracle's masked"""
    mask, _ = P.listed(images, p2x, p2y)
    ox, oy = P.oracle_view(p2x, p2y, mask)
    want = Oracle(oracle, images, ox, oy, iters)
    d_img, d_x, d_y = dev(images), dev(p2x), dev(p2y)
    for _ in range(reps):
        index, rows = check_index(ctx, d_img, d_x, d_y, images, ox, oy)
        check_steps(ctx, want, d_img, d_x, d_y, index, atomic_iters=atomic_iters)
        index.close()
    return want, rows, (d_img, d_x, d_y)


# ---- 1. the scan's carry over passes of 1024 groups ------------------------------------------------------------------------------
# (w, h) -> groups of 64 bins, nbins % 64
SCAN_SHAPES = [(264, 248), (21803, 3), (329, 199),  # 1023 groups: % 64 = 0, 1, 63
               (256, 256), (281, 233), (257, 255), (32768, 2),  # 1024: 0, 1, 63, and 2 rows
               (320, 205),  # 1025: 0 (65537 and 65599 bins have no w x h with h >= 2)
               (512, 256), (43691, 3), (26227, 5),  # 2048: 0; 2049: 1, 63
               (1280, 1024)]  # 20480: 20 passes


@pytest.mark.parametrize("w,h", SCAN_SHAPES, ids=lambda v: str(v))
def test_scan_carry(ctx, oracle, w, h):
    nb = w * h
    g = -(-nb // 64)
    assert g in (1023, 1024, 1025, 2048, 2049, 20480) and nb % 64 in (0, 1, 63)
    s = min(0.9, (150000.0 / nb) ** 0.5)
    gw, gh = max(4, round(w * s)), max(4, round(h * s))
    images, p2x, p2y = P.smooth_problem(nb, 4, w, h, gw, gh, warp=0.05)
    want, rows, _ = dense_case(ctx, oracle, images, p2x, p2y, iters=4)
    assert rows.size == g and np.count_nonzero(rows) > 0.6 * g  # lists in every pass of the scan
    assert want.steps[-1]["r2"] > 0 and np.isfinite(want.vf).sum() > 0.1 * nb


# ---- 2. gather blocks of kVcalSlackRows rows --------------------------------------------------------------------------------------
GATHER_LENGTHS = [0, 1, 7, 8, 9, 15, 16, 17, 10080, 3]  # per pair of image rows: the length of both their groups


def gather_problem(h, n=160, seed=0):
    """w = 64: one group per image row.  Row pair m (rows 2m, 2m+1) gets its samples on image row 2m: GATHER_LENGTHS[m] of them on
    pixel x0 = 3 + 5m, half as many on x0 + 6 (empty bins between).  Sample s of a pixel lies in image s % n and belongs to plane
    point s // 4 of that pixel (4 images per point, <= 63 samples of one image per bin); plane points are numbered at random."""
    rng = np.random.default_rng(seed + h)
    w = 64
    pairs = h // 2
    plan = []  # (x pixel, y pixel, count)
    for m in range(pairs):
        L = GATHER_LENGTHS[m % len(GATHER_LENGTHS)]
        plan += [(3 + 5 * m, 2 * m, L), (9 + 5 * m, 2 * m, L // 2)]
    npts = sum(-(-c // 4) for _, _, c in plan)
    ids = rng.permutation(npts)
    p2x = np.full((n, npts), np.nan, np.float32)
    p2y = np.full((n, npts), np.nan, np.float32)
    base = 0
    for x0, y0, c in plan:
        s = np.arange(c)
        img, pid = s % n, ids[base + s // 4]
        p2x[img, pid] = x0 + 0.99 * rng.random(c)
        p2y[img, pid] = y0 + 0.99 * rng.random(c)
        base += -(-c // 4)
    images = (50 + 30 * rng.random((n, h, w))).astype(np.float32)
    expect = np.zeros(h, np.int64)
    for m in range(pairs):
        expect[2 * m] = expect[2 * m + 1] = GATHER_LENGTHS[m % len(GATHER_LENGTHS)]
    return images, p2x, p2y, expect


@pytest.mark.parametrize("h", [20, 21, 22, 23])
def test_gather_blocks(ctx, oracle, h):
    images, p2x, p2y, expect = gather_problem(h)
    assert h % 4 == h - 20  # ngroups = h: the gather grid's last workgroup holds 4, 1, 2, 3 waves
    want, rows, _ = dense_case(ctx, oracle, images, p2x, p2y, iters=4)
    assert np.array_equal(rows, expect), (rows, expect)
    assert want.steps[-1]["r2"] > 5000


# ---- 3. image edges --------------------------------------------------------------------------------------------------------------
def edge_problem(w, h, n=5, npt=400, seed=0):
    """random footprints inside, and per image a rotating set of edge coordinates: the first column / row, -0.0, the last
    admissible ones (nextafter(w-1, 0), nextafter(h-1, 0)) -- kept -- and w-1, h-1, -tiny -- dropped by every path"""
    rng = np.random.default_rng(seed + 100 * w + h)
    f32 = np.float32
    lx, ly = np.nextafter(f32(w - 1), f32(0)), np.nextafter(f32(h - 1), f32(0))
    tiny = -np.float32(1e-45)
    p2x = rng.uniform(0, w - 1, (n, npt)).astype(f32)
    p2y = rng.uniform(0, h - 1, (n, npt)).astype(f32)
    np.minimum(p2x, lx, out=p2x)
    np.minimum(p2y, ly, out=p2y)
    special = [(0, None), (None, 0), (lx, None), (None, ly), (lx, ly), (0, 0), (f32(-0.0), None), (None, f32(-0.0)), (f32(-0.0), f32(-0.0)),
               (lx, 0), (0, ly), (f32(w - 1), None), (tiny, None), (None, f32(h - 1)), (None, tiny), (f32(w - 1), ly), (tiny, tiny)]
    for i in range(n):
        for j in range(3 * len(special)):
            sx, sy = special[(i + j) % len(special)]
            pi = 7 * j + i
            if sx is not None:
                p2x[i, pi] = sx
            if sy is not None:
                p2y[i, pi] = sy
    p2x[rng.random((n, npt)) < 0.05] = np.nan
    p2y[np.isnan(p2x)] = np.nan
    images = (60 + 30 * rng.random((n, h, w))).astype(f32)
    if w * h > 100:
        images[rng.random((n, h, w)) < 0.01] = np.nan
    return images, p2x, p2y


@pytest.mark.parametrize("w,h", [(2, 9), (11, 2), (2, 2), (37, 23), (64, 3)], ids=lambda v: str(v))
def test_image_edges(ctx, oracle, w, h):
    images, p2x, p2y = edge_problem(w, h)
    mask, _ = P.listed(images, p2x, p2y)
    f32 = np.float32
    dropped = (p2x == f32(w - 1)) | (p2y == f32(h - 1)) | (p2x < 0) | (p2y < 0)
    assert dropped.sum() > 20 and not np.any(mask & dropped)
    kept_edge = mask & ((p2x == np.nextafter(f32(w - 1), f32(0))) | (p2y == np.nextafter(f32(h - 1), f32(0))) | (p2x == 0) | (p2y == 0))
    assert kept_edge.sum() > 20
    dense_case(ctx, oracle, images, p2x, p2y, iters=4, atomic_iters=(0, 1, 2, 3))


# ---- 4. the per-image segment sort ---------------------------------------------------------------------------------------------
def test_segment_sort(ctx, oracle):
    """7 x 7 plane points per pixel (every bin gets ~196 entries of each image), numbered at random: the slot atomics append them
    in no particular order.  Three builds of the index: each gives the oracle's bits."""
    rng = np.random.default_rng(44)
    n, w, h = 3, 24, 20
    gx = (np.arange(7 * (w - 1)) + 0.5) / 7
    gy = (np.arange(7 * (h - 1)) + 0.5) / 7
    X, Y = np.meshgrid(gx, gy)
    X, Y = X.reshape(-1), Y.reshape(-1)
    ids = rng.permutation(X.size)
    p2x = np.empty((n, X.size), np.float32)
    p2y = np.empty((n, X.size), np.float32)
    for i in range(n):
        p2x[i, ids] = np.minimum(X + 0.05 * rng.random(X.size), w - 1.01)
        p2y[i, ids] = np.minimum(Y + 0.05 * rng.random(X.size), h - 1.01)
    images = (60 + 30 * rng.random((n, h, w))).astype(np.float32)
    mask, b = P.listed(images, p2x, p2y)
    per_image_bin = max(np.bincount(b[np.nonzero(mask)[0] == i], minlength=w * h).max() for i in range(n))
    assert per_image_bin >= 32
    dense_case(ctx, oracle, images, p2x, p2y, iters=4, reps=3)


# ---- the sparse construction: a few (image, point) pairs on the device, everything else NaN / sentinel ------------------------
def sparse_device(n, w, h, npd, imgs, pts, images_c, x_c, y_c):
    """device stack of n w x h images (sentinel but `imgs`, which hold images_c) and n x npd coordinates (NaN but imgs x pts,
    which hold x_c / y_c)"""
    import torch

    d_img = torch.full((n, h, w), SENTINEL, dtype=torch.float32, device="cuda")
    d_x = torch.full((n, npd), float("nan"), dtype=torch.float32, device="cuda")
    d_y = torch.full((n, npd), float("nan"), dtype=torch.float32, device="cuda")
    d_i, d_p = dev(np.asarray(imgs, np.int64)), dev(np.asarray(pts, np.int64))
    d_img[d_i] = dev(images_c)
    d_x[d_i[:, None], d_p[None, :]] = dev(x_c)
    d_y[d_i[:, None], d_p[None, :]] = dev(y_c)
    torch.cuda.synchronize()
    return d_img, d_x, d_y


def sparse_problem(seed, imgs, npd, w, h, must, per_image=3000):
    """the compacted problem: len(imgs) images, each holding 80 % of per_image random points plus `must`"""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    k = len(imgs)
    pool = rng.choice(npd, per_image, replace=False)  # most points in most images: FF >= 1 past the first iteration
    chosen = [np.union1d(pool[rng.random(pool.size) < 0.8], must) for _ in range(k)]
    pts = np.unique(np.concatenate(chosen))
    images = P.smooth_problem(seed, k, w, h, 4, 4, nan_px=0.003)[0]

    def draw(shape):  # random positions, not ordered by point
        x = np.minimum(rng.uniform(0, w - 1, shape).astype(f32), np.nextafter(f32(w - 1), f32(0)))
        y = np.minimum(rng.uniform(0, h - 1, shape).astype(f32), np.nextafter(f32(h - 1), f32(0)))
        return x, y

    x, y = draw((k, pts.size))
    for i in range(k):
        off = ~np.isin(pts, chosen[i])
        x[i, off] = np.nan
        y[i, off] = np.nan
    mi = np.searchsorted(pts, must)
    mask, _ = P.listed(images, x, y)
    while not mask[:, mi].all():  # the points that must be listed: away from NaN pixels
        ii, jj = np.nonzero(~mask[:, mi])
        x[ii, mi[jj]], y[ii, mi[jj]] = draw(ii.size)
        mask, _ = P.listed(images, x, y)
    x, y = P.oracle_view(x, y, mask)  # every sample the device gets is listed: the oracle sees them all
    return images, x, y, pts


# ---- 5. 2^30 - 1 plane points ----------------------------------------------------------------------------------------------------
def test_plane_point_width(ctx, oracle):
    """n_plane = 2^30 - 1: the last plane point, 2^30 - 2, is listed (its corner-3 entry packs to 0xFFFFFFFE); steps, index and solve
    equal the oracle on the compacted problem.  2^30 is refused by the index and the solve."""
    from mono_dataset_code_amd import capi

    NP = 2 ** 30 - 1
    n, w, h = 2, 64, 48
    need(4 * NP * (2 * n + 4), "2^30 - 1 plane points")
    must = [0, 1, 2 ** 29, NP - 2, NP - 1]
    images, x, y, pts = sparse_problem(30, [0, 1], NP, w, h, must, per_image=400)
    assert pts[-1] == NP - 1 and ((int(pts[-1]) | 3 << 30) & 0xFFFFFFFF) == 0xFFFFFFFE
    want = Oracle(oracle, images, x, y, 4)
    d_img, d_x, d_y = sparse_device(n, w, h, NP, [0, 1], pts, images, x, y)
    index, _ = check_index(ctx, d_img, d_x, d_y, images, x, y)
    d_pc, d_vf = check_steps(ctx, want, d_img, d_x, d_y, index, keep=pts)
    index.close()
    del d_pc, d_vf
    check_solve(ctx, want, d_img, d_x, d_y, keep=pts)
    for call in ("index", "solve"):
        assert refused(ctx, call, n=2, w=w, h=h, n_plane=2 ** 30) == capi.ERR_ARG, call


# ---- 6. stack offsets past 2^31 elements and 2^32 bytes --------------------------------------------------------------------------
def test_stack_offsets(ctx, oracle):
    """65535 images of 256 x 129 (image 65534 starts at element 2.16e9, byte 8.7e9) and 40000 plane points (p2x row 65534 starts at
    element 2.6e9): only images 0, 1, 32768, 65533 and 65534 have coordinates, the others hold 1e30.  Plane step, atomic step, index
    and indexed step, solve, scaling."""
    import torch

    n, w, h, NP = 65535, 256, 129, 40000
    imgs = [0, 1, 32768, 65533, 65534]
    need(4 * n * (w * h + 2 * NP) + 4 * 1e8, "a 65535-image stack")
    images, x, y, pts = sparse_problem(65535, imgs, NP, w, h, [0, 32767, 32768, NP - 1])
    want = Oracle(oracle, images, x, y, 4)
    d_img, d_x, d_y = sparse_device(n, w, h, NP, imgs, pts, images, x, y)
    assert (n - 1) * w * h >= 2 ** 31 and (n - 1) * NP >= 2 ** 31
    index, _ = check_index(ctx, d_img, d_x, d_y, images, x, y)
    check_steps(ctx, want, d_img, d_x, d_y, index, keep=pts, atomic_iters=(0, 3))
    index.close()
    check_solve(ctx, want, d_img, d_x, d_y, keep=pts)
    del d_x, d_y
    rng = np.random.default_rng(6)
    expo = rng.uniform(0.01, 30.0, n).astype(np.float32)
    expo[[1, 65533]] = 0
    mean = np.float32(3.7)
    ctx.vcal_scale_images(d_img, mean, dev(expo))
    for k, im in list(zip(imgs, images)) + [(2, None), (32767, None), (65532, None)]:
        src = np.full((h, w), np.float32(SENTINEL)) if im is None else im
        e = np.float32(1) if expo[k] == 0 else expo[k]
        assert bits_equal(host(d_img[k]), (mean * src) / e), k
    del d_img
    torch.cuda.empty_cache()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def refused(ctx, call, n, w, h, n_plane):
    """the return code of one entry point for sizes past its limits (arguments only the size checks stop: never launched)"""
    import torch

    L = ctx._L
    cells = max(1, min(n * w * h, 1 << 20))
    buf = torch.zeros(cells + n * min(n_plane, 1 << 10) + 4096, dtype=torch.float32, device="cuda")
    p = buf.data_ptr()
    er = torch.zeros(16, dtype=torch.float64, device="cuda")
    if call == "plane":
        return L.mdc_vcal_plane_step_device(ctx._h, p, p, p, n, w, h, n_plane, p, p, 225, p, p, er.data_ptr(), None)
    if call == "vignette":
        return L.mdc_vcal_vignette_step_device(ctx._h, p, p, p, n, w, h, n_plane, p, p, 225, p, p, er.data_ptr(), None)
    if call == "index":
        out = C.c_void_p()
        rc = L.mdc_vcal_index_create(ctx._h, p, p, p, n, w, h, n_plane, None, C.byref(out))
        if out.value:
            L.mdc_vcal_index_destroy(out)
        return rc
    if call == "solve":
        return L.mdc_vcal_solve_device(ctx._h, p, p, p, n, w, h, n_plane, p, p, 2, 15, None, None)
    if call == "scale":
        return L.mdc_vcal_scale_images_device(ctx._h, p, n, w * h, C.c_float(1.0), p, None)
    raise ValueError(call)


def test_refusals(ctx):
    from mono_dataset_code_amd import capi

    for call in ("vignette", "index", "solve", "scale"):
        assert refused(ctx, call, n=65536, w=2, h=2, n_plane=1) == capi.ERR_ARG, call
    for call in ("plane", "vignette", "index", "solve"):
        assert refused(ctx, call, n=1, w=65536, h=32768, n_plane=1) == capi.ERR_ARG, call
        assert refused(ctx, call, n=1, w=2 ** 31 - 1, h=2, n_plane=1) == capi.ERR_ARG, call


# ---- 7. list slots past 2^32 bytes and past 2^32 ---------------------------------------------------------------------------------
def heavy_problem(n, k, seed):
    """n images of 64 x 64 (one image row = one group); every image puts k samples on pixel 31 of each of rows 0..62, so bins 31 and
    32 of rows 1..62 receive 2k entries per image (rows 0 and 63: k): Σ group lengths = 126 k n rows."""
    rng = np.random.default_rng(seed)
    w = h = 64
    r = np.repeat(np.arange(63), k)
    p2x = (31 + 0.99 * rng.random((n, r.size), dtype=np.float32)).astype(np.float32)
    p2y = (r[None, :] + 0.99 * rng.random((n, r.size), dtype=np.float32)).astype(np.float32)
    images = 50 + 20 * rng.random((n, h, w), dtype=np.float32)
    return images, p2x, p2y


@pytest.mark.parametrize("n,k", [(40000, 1), (65535, 9)], ids=["past_2^32_bytes", "past_2^32_slots"])
def test_list_slots(ctx, oracle, n, k):
    rows = 126 * k * n
    slots = 64 * rows
    if k == 1:
        assert rows > 2 ** 22 * 1.15 and 16 * slots > 2 ** 32 * 1.15 and slots < 2 ** 32
    else:
        assert slots > 2 ** 32 * 1.1
    need(P.index_bytes(rows) + 4 * n * 64 * 64 + 8 * n * 63 * k, "%d list rows" % rows)
    images, p2x, p2y = heavy_problem(n, k, n + k)
    want = Oracle(oracle, images, p2x, p2y, 2)
    d_img, d_x, d_y = dev(images), dev(p2x), dev(p2y)
    index, got_rows = check_index(ctx, d_img, d_x, d_y, images, p2x, p2y)
    assert got_rows.sum() == rows and index.bytes >= 16 * 64 * rows
    check_steps(ctx, want, d_img, d_x, d_y, index)
    index.close()


# ---- 8. gradient mask fronts of more than 256 rows ---------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(1280, 300), (1284, 300), (1285, 300), (1290, 301), (2048, 320), (1280, 1024)], ids=lambda v: str(v))
def test_gradient_mask_wide(ctx, oracle, w, h):
    rng = np.random.default_rng(w + h)
    yy, xx = np.mgrid[0:h, 0:w]
    stack = []
    for k in range(3):
        img = (100 + 30 * np.sin(0.02 * (k + 1) * xx) * np.cos(0.015 * yy) + rng.normal(0, 8, (h, w))).astype(np.float32)
        img[rng.random((h, w)) < 0.02] += 200
        img[rng.random((h, w)) < 0.01] = np.nan
        stack.append(img)
    stack = np.stack(stack)
    d = dev(stack)
    ctx.vcal_gradient_mask(d, 25)
    got = host(d)
    for k in range(3):
        want = oracle.vcal_gradient_mask(stack[k], 25)
        assert bits_equal(got[k], want), (w, h, k)
        # masked pixels in rows >= 258, which a front of more than 256 rows (w >= 1285) reaches on the loop's second trip
        assert np.isnan(want[258:]).sum() > 100


# ---- 9. coordinate mask and smoothing at size --------------------------------------------------------------------------------------
def test_coordinate_mask_and_smoothing_full_frame(ctx, oracle):
    rng = np.random.default_rng(9)
    w, h, N = 1280, 1024, 10 ** 6
    x = rng.uniform(-8, w + 8, N).astype(np.float32)
    y = rng.uniform(-8, h + 8, N).astype(np.float32)
    x[::97], y[5::89], x[7::101] = np.nan, np.inf, -np.inf
    d_x, d_y = dev(x), dev(y)
    ctx.vcal_mask_coords(d_x, d_y, w, h)
    wx, wy = oracle.vcal_mask_coords(x, y, w, h)
    assert bits_equal(host(d_x), wx) and bits_equal(host(d_y), wy)
    v = rng.random(w * h).astype(np.float32)
    v[rng.random(w * h) < 0.3] = np.nan
    v.reshape(h, w)[100:140, 200:260] = np.nan
    v[: 3 * w] = np.nan
    tt, ct = ctx.vcal_smooth(dev(v), w, h)
    want_tt, want_ct = oracle.vcal_smooth(v, w, h)
    assert bits_equal(host(tt), want_tt) and bits_equal(host(ct), want_ct)


def test_coordinate_mask_past_2_31(ctx, oracle):
    """2^31 + 1000 coordinate pairs holding an inside constant, random values in windows around 0, 2^31 - 1, 2^31 and the end:
    the windows equal the oracle, the rest comes back unchanged (a reduction on the device)"""
    import torch

    N = 2 ** 31 + 1000
    w, h = 1280, 1024
    need(8 * N, "2^31 + 1000 coordinate pairs")
    d_x = torch.full((N,), 5.0, dtype=torch.float32, device="cuda")
    d_y = torch.full((N,), 7.0, dtype=torch.float32, device="cuda")
    rng = np.random.default_rng(31)
    windows = [(0, 1024), (2 ** 31 - 600, 2 ** 31 + 400), (N - 500, N)]  # disjoint: N - 500 = 2^31 + 500
    vals = []
    for a, b in windows:
        x = rng.uniform(-4, w + 4, b - a).astype(np.float32)
        y = rng.uniform(-4, h + 4, b - a).astype(np.float32)
        x[::13] = np.nan
        d_x[a:b] = dev(x)
        d_y[a:b] = dev(y)
        vals.append((x, y))
    ctx.vcal_mask_coords(d_x, d_y, w, h)
    for (a, b), (x, y) in zip(windows, vals):
        wx, wy = oracle.vcal_mask_coords(x, y, w, h)
        assert np.isnan(wx).sum() > 20
        assert bits_equal(host(d_x[a:b]), wx) and bits_equal(host(d_y[a:b]), wy), (a, b)
        d_x[a:b] = 5.0
        d_y[a:b] = 7.0
    assert bool((d_x == 5.0).all()) and bool((d_y == 7.0).all())
    del d_x, d_y
    torch.cuda.empty_cache()


# ---- 10. the whole solve at production scale ---------------------------------------------------------------------------------------
def test_production_solve(ctx, oracle):
    """1280 x 1024, 16 images, 1000 x 1000 plane points through a non-affine map, 4 iterations (2 each side of the outlier switch):
    the solve equals the oracle's loop bit for bit; the atomic step at that size within 1e-5"""
    import torch

    n, w, h = 16, 1280, 1024
    images, p2x, p2y = P.smooth_problem(1280, n, w, h, 1000, 1000, warp=0.08)
    mask, _ = P.listed(images, p2x, p2y)
    ox, oy = P.oracle_view(p2x, p2y, mask)
    want = Oracle(oracle, images, ox, oy, 4)
    d_img, d_x, d_y = dev(images), dev(p2x), dev(p2y)
    check_solve(ctx, want, d_img, d_x, d_y)
    s = want.steps[0]
    d_pc = dev(s["pc"])
    d_vf = torch.ones(w * h, dtype=torch.float32, device="cuda")
    check_atomic(ctx, d_img, d_x, d_y, d_pc, d_vf, s["oth2"], (s["vf"], s["tt"], s["ct"], s["e2"], s["r2"]))
    assert want.steps[-1]["r1"] > 0.5 * mask.sum()
