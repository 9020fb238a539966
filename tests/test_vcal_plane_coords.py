"""mdc_vcal_plane_coords_device: vignetteCalib's plane -> image coordinates (reference src/main_vignetteCalib.cpp:230-258, :284,
:345-357) on the device, against the test-owned restatement tests/vcal_plane_restatement.py (pinned to a literal transcription of
the reference's loops, in the same file) and against the separate entry points it fuses:

  literal loops       HK and the projection bit for bit a literal transcription of the reference's lines (tests/vcal_plane_restatement.py),
                      Eigen's K_p2idx^-1 with its last-bit quirk included
  HK from corners     bit for bit the restatement's (double square-to-quad map, float Eigen-order product with K_p2idx^-1)
  4-point fit         HK within float rounding of the one a general 8 x 8 DLT solve gives; the corners reprojected through HK within 1e-3 px
  projection          model = None: bit for bit the restatement's pp0 / pp2, pp1 / pp2, at grid sizes around the 256-point blocks
  distort + mask      bit for bit mdc_distort_points_device followed by mdc_vcal_mask_coords_device on the projection
  limits              n <= 65535, gw * gh < 2^31, missing buffers: MDC_ERR_ARG; n = 0: nothing written"""
import os

import numpy as np
import pytest

import vcal_plane_restatement as V
from conftest import bits_equal

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def ctx():
    from mono_dataset_code_amd import capi

    return capi.Context(0)


def model_of(calib_dirs, name):
    from mono_dataset_code_amd import capi

    fov = capi.UndistorterFOV(os.path.join(calib_dirs[name], "camera.txt"))
    m = fov.model()
    fov.close()
    return m


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy()


@pytest.mark.parametrize("gw,gh,facw,fach", [(1000, 1000, 5, 5), (37, 29, 5, 5), (40, 31, 3.7, 6.1), (1, 1, 5, 5), (7, 2, 0.5, 2)])
def test_device_equals_literal_loops(ctx, gw, gh, facw, fach):
    """:193-198 and :246-258 as loops (every plane point of the small grids, five whole rows of 1000 x 1000) against the device, and the
    vectorised restatement against both."""
    rng = np.random.default_rng(gw * 7 + gh)
    corners = V.random_corners(rng, 3, 640, 480)
    p2x, p2y, hk = ctx.vcal_plane_coords(None, gw, gh, facw, fach, corners=dev(corners))
    got_hk, got_x, got_y = host(hk), host(p2x), host(p2y)
    H = V.homography(corners)
    u, v = V.project(V.hk_of(H, gw, gh, facw, fach), gw, gh)
    assert bits_equal(got_x, u) and bits_equal(got_y, v)
    rows = range(gh) if gw * gh <= 4000 else (0, 1, gh // 2, gh - 2, gh - 1)
    for f in range(3):
        HKl = V.literal_hk(H[f].astype(np.float64), gw, gh, facw, fach)
        assert bits_equal(got_hk[f], HKl), f
        pts = V.literal_points(HKl, gw, gh, rows)
        idx = np.array(sorted(pts))
        assert bits_equal(got_x[f][idx], [pts[i][0] for i in idx]) and bits_equal(got_y[f][idx], [pts[i][1] for i in idx]), f


def test_device_keeps_eigens_k_inverse(ctx):
    """Eigen's Kinv(0, 0) = b * (1 / (a * b)) and Kinv(2, 2) = (a * b) * (1 / (a * b)), not 1 / a and 1: on grids where the two differ
    in the last bit, the device's HK is the one with Eigen's inverse (the reference's), not the one with the exact inverse."""
    grids = []
    for gw in range(900, 1100):
        gh = 1000 + gw % 7
        ki = V.k_inverse(gw, gh, 5, 5)
        if ki[0, 0] != f32(1) / (f32(gw) / f32(5)) or ki[2, 2] != f32(1):
            grids.append((gw, gh))
    assert len(grids) >= 5
    corners = V.random_corners(np.random.default_rng(9), 4, 640, 480)
    H = V.homography(corners)
    differs = 0
    for gw, gh in grids[:12]:
        _, _, hk = ctx.vcal_plane_coords(None, gw, gh, 5, 5, corners=dev(corners))
        got = host(hk)
        assert bits_equal(got, V.hk_of(H, gw, gh, 5, 5)), (gw, gh)
        k = V.k_p2idx(gw, gh, 5, 5)
        exact = np.array([[f32(1) / k[0, 0], 0, -k[0, 2] / k[0, 0]], [0, f32(1) / k[1, 1], -k[1, 2] / k[1, 1]], [0, 0, 1]], np.float32)
        naive = (H[:, :, 0, None] * exact[0] + (H[:, :, 1, None] * exact[1] + H[:, :, 2, None] * exact[2])).astype(np.float32)
        differs += not bits_equal(got, naive)
    assert differs > 0


def test_device_hk_equals_a_general_dlt(ctx):
    """The device's HK against HK from the 8 x 8 DLT system (h22 = 1) solved by LAPACK in double: equal within float rounding."""
    rng = np.random.default_rng(3)
    corners = V.random_corners(rng, 200, 1280, 1024, side=(20, 900), tilt=0.6)
    _, _, hk = ctx.vcal_plane_coords(None, 1000, 1000, 5, 5, corners=dev(corners))
    got = host(hk).astype(np.float64)
    Hs = []
    for f in range(len(corners)):
        A, b = [], []
        for (X, Y), (x, y) in zip(V.PLANE_POINTS, corners[f].astype(np.float64)):
            A.append([X, Y, 1, 0, 0, 0, -x * X, -x * Y])
            b.append(x)
            A.append([0, 0, 0, X, Y, 1, -y * X, -y * Y])
            b.append(y)
        Hs.append(np.append(np.linalg.solve(np.array(A), np.array(b)), 1.0).reshape(3, 3))
    want = np.array(Hs) @ V.k_inverse(1000, 1000, 5, 5).astype(np.float64)
    for f in range(len(corners)):
        assert np.allclose(got[f], want[f], rtol=1e-5, atol=1e-5 * np.abs(want[f]).max()), f


@pytest.mark.parametrize("n", [1, 7, 64, 65])
def test_hk_from_corners_equals_restatement(ctx, n):
    rng = np.random.default_rng(n)
    corners = V.random_corners(rng, n, 640, 480, side=(40, 400), tilt=0.5)
    for gw, gh, facw, fach in ((1000, 1000, 5, 5), (333, 257, 3.3, 7.9)):
        _, _, hk = ctx.vcal_plane_coords(None, gw, gh, facw, fach, corners=dev(corners))
        want = V.hk_of(V.homography(corners), gw, gh, facw, fach)
        assert bits_equal(host(hk), want), (gw, gh)


def test_fit_reprojects_the_corners(ctx):
    """The 4 plane points through the device's HK land on the corners within 1e-3 px, for markers of 40-400 px in the 640 x 480 frame.
    What remains is HK's float rounding (the reference forms HK in float too): on one MI355X the worst of these 500 was 6.6e-4 px;
    with sides up to 900 px and steeper views on 1280 x 1024 it reached 1.5e-3 px."""
    rng = np.random.default_rng(1)
    corners = V.random_corners(rng, 500, 640, 480, side=(40, 400), tilt=0.5)
    gw, gh, facw, fach = 1000, 1000, 5, 5
    _, _, hk = ctx.vcal_plane_coords(None, gw, gh, facw, fach, corners=dev(corners))
    hk = host(hk).astype(np.float64)
    g = V.plane_grid_points(gw, gh, facw, fach)
    p = np.einsum("fij,kj->fki", hk, np.concatenate([g, np.ones((4, 1))], 1))
    worst = np.abs(p[..., :2] / p[..., 2:] - corners).max()
    print("worst corner reprojection %.3g px" % worst)
    assert worst < 1e-3


@pytest.mark.parametrize("gw,gh", [(1000, 1000), (256, 1), (257, 3), (255, 2), (1, 1), (37, 29), (1, 300)])
def test_projection_bits_for_given_hk(ctx, gw, gh):
    rng = np.random.default_rng(gw + 1000 * gh)
    n = 3
    hk = V.hk_of(V.homography(V.random_corners(rng, n, 640, 480)), gw, gh, 5, 5)
    hk[2] = rng.normal(0, 1, (3, 3)).astype(np.float32)  # any matrix: negative and zero denominators, points behind the camera
    hk[2, 2, 2] = 0
    p2x, p2y, hk_back = ctx.vcal_plane_coords(None, gw, gh, hk=dev(hk))
    u, v = V.project(hk, gw, gh)
    assert bits_equal(host(p2x), u) and bits_equal(host(p2y), v)
    assert bits_equal(host(hk_back), hk)  # given HK is read, not rewritten


@pytest.mark.parametrize("name", ["full_1280_to_640", "small_explicit", "small_pinhole", "ragged", "full_1280_wide"])
def test_distort_and_mask_equal_the_separate_calls(ctx, calib_dirs, name):
    m = model_of(calib_dirs, name)
    rng = np.random.default_rng(len(name))
    n = 5
    gw, gh = (1000, 1000) if name == "full_1280_to_640" else (301, 207)
    # views that cover the frame, leave it, and see the plane from a steep angle: some points masked, some not
    corners = V.random_corners(rng, n, m.out_w, m.out_h, side=(0.3 * m.out_w, 1.5 * m.out_w), tilt=0.6)
    p2x, p2y, hk = ctx.vcal_plane_coords(m, gw, gh, 5, 5, corners=dev(corners))
    u, v = V.project(host(hk), gw, gh)
    d_u, d_v = dev(u), dev(v)
    ctx.distort_points_device(m, d_u.data_ptr(), d_v.data_ptr(), d_u.numel())
    ctx.vcal_mask_coords(d_u, d_v, m.in_w, m.in_h)
    got_x, got_y, want_x, want_y = host(p2x), host(p2y), host(d_u), host(d_v)
    assert bits_equal(got_x, want_x) and bits_equal(got_y, want_y)
    kept = np.isfinite(got_x).mean()
    assert 0.01 < kept < 0.999, kept  # both sides of the mask were exercised
    # the corners path and the given-HK path agree
    p2x2, p2y2, _ = ctx.vcal_plane_coords(m, gw, gh, 5, 5, hk=hk.clone())
    assert bits_equal(host(p2x2), got_x) and bits_equal(host(p2y2), got_y)


def test_degenerate_corners_are_masked(ctx, calib_dirs):
    m = model_of(calib_dirs, "small_explicit")
    c = np.array([[[5, 5], [0, 0], [10, 0], [20, 0]]], np.float32)  # corners 1, 2, 3 on a line
    p2x, p2y, hk = ctx.vcal_plane_coords(m, 40, 30, corners=dev(c))
    assert not np.isfinite(host(hk)).all()
    assert np.isnan(host(p2x)).all() and np.isnan(host(p2y)).all()


def test_feeds_the_solver(ctx, calib_dirs):
    """The coordinates go straight into the solver's slots: the plane step over them equals the plane step over the same
    coordinates made by the separate calls."""
    import torch

    m = model_of(calib_dirs, "small_explicit")
    rng = np.random.default_rng(5)
    n, gw, gh = 4, 120, 90
    corners = V.random_corners(rng, n, m.out_w, m.out_h, side=(60, 110), tilt=0.3)
    p2x, p2y, hk = ctx.vcal_plane_coords(m, gw, gh, 5, 5, corners=dev(corners))
    u, v = V.project(host(hk), gw, gh)
    d_u, d_v = dev(u), dev(v)
    ctx.distort_points_device(m, d_u.data_ptr(), d_v.data_ptr(), d_u.numel())
    ctx.vcal_mask_coords(d_u, d_v, m.in_w, m.in_h)
    images = dev(rng.uniform(10, 200, (n, m.in_h, m.in_w)).astype(np.float32))
    vig = torch.ones(m.in_h * m.in_w, dtype=torch.float32, device="cuda")
    pc_a = torch.zeros(gw * gh, dtype=torch.float32, device="cuda")
    pc_b = pc_a.clone()
    ff_a, fc_a, e_a, r_a = ctx.vcal_plane_step(images, p2x, p2y, pc_a, vig, 10000 * 10000)
    ff_b, fc_b, e_b, r_b = ctx.vcal_plane_step(images, d_u, d_v, pc_b, vig, 10000 * 10000)
    assert bits_equal(host(pc_a), host(pc_b)) and bits_equal(host(ff_a), host(ff_b)) and r_a == r_b and r_a > 1000


def test_limits(ctx):
    import ctypes as C

    from mono_dataset_code_amd import capi

    L = capi.hip_lib()
    hk = dev(np.tile(np.eye(3, dtype=np.float32), (2, 1, 1)))
    xs, ys = dev(np.zeros(2 * 4, np.float32)), dev(np.zeros(2 * 4, np.float32))

    def call(n, gw, gh, hk_ptr=hk.data_ptr(), x=xs.data_ptr(), y=ys.data_ptr()):
        return L.mdc_vcal_plane_coords_device(ctx._h, None, None, hk_ptr, n, gw, gh, C.c_float(5), C.c_float(5), x, y, None)

    assert call(0, 2, 2, hk_ptr=None, x=None, y=None) == capi.OK  # nothing to do
    assert call(-1, 2, 2) == capi.ERR_ARG
    assert call(65536, 2, 2) == capi.ERR_ARG
    assert call(2, 0, 2) == capi.ERR_ARG and call(2, 2, 0) == capi.ERR_ARG
    assert call(2, 1 << 16, 1 << 15) == capi.ERR_ARG  # gw * gh = 2^31
    assert call(2, 2, 2, hk_ptr=None) == capi.ERR_ARG and call(2, 2, 2, x=None) == capi.ERR_ARG and call(2, 2, 2, y=None) == capi.ERR_ARG
    assert not host(xs).any() and not host(ys).any()  # the refused calls wrote nothing
    assert call(2, 2, 2) == capi.OK
    u, v = V.project(np.tile(np.eye(3, dtype=np.float32), (2, 1, 1)), 2, 2)
    assert bits_equal(host(xs), u) and bits_equal(host(ys), v)
