"""Raw pixel -> rectified pixel on the GPU: libmdc_lensinv.so's kernels and the class's bulk path against the NumPy restatement
(tests/lens_inverse_restatement.py) bit for bit, the round trip through the forward kernels, and the frame kernels on inverse tables
(rectified frames re-distorted into raw geometry) against the oracle."""
import os

import numpy as np
import pytest

import lens_inverse_restatement as V
import lens_problems as LP
import lens_restatement as R
from conftest import bits_equal
from test_lens_inverse_cpu import INV_CAM, INV_RECT, INV_SEED, KINDS, TABLE_PROBLEMS, inverse_points, round_trip_cap

pytestmark = pytest.mark.gpu
F = np.float32


def inverse_of(kind):
    from mono_dataset_code_amd import capi

    return capi.LensInverse(capi.LensModel.make(kind, INV_CAM[kind], INV_RECT))


def model_of(q):
    from mono_dataset_code_amd import capi

    return capi.LensModel.make(q["kind"], q["cam"], q["rect"], (q["in_w"], q["in_h"]), (q["out_w"], q["out_h"]))


@pytest.fixture(scope="module")
def problems():
    """the small problems and the small FOV camera, restated once, with their inverse tables"""
    out = {}
    for name in TABLE_PROBLEMS:
        q = V.fov_problem(V.SMALL_FOV) if name == "fov_small" else V.inverse_problem(R.parse(LP.PROBLEMS[name]))
        out[name] = (q,) + V.inverse_tables(q)
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_undistort_points_device_equals_the_restatement(kind):
    """n = 0, 1, 255, 256, 257, 65 537; arrays offset by one float; a stream of its own; NaN, infinities, the principal point,
    rd <= 1e-8 and points outside the domain are points 0 .. 9"""
    import torch

    inv = inverse_of(kind)
    stream = torch.cuda.Stream()
    for n in (0, 1, 255, 256, 257, 65537):
        x, y = inverse_points(INV_SEED[kind], np.arange(n), INV_CAM[kind])
        wx, wy = V.undistort(kind, INV_CAM[kind], INV_RECT, x, y)
        d_x, d_y = torch.full((n + 3,), -7.0, device="cuda"), torch.full((n + 3,), -7.0, device="cuda")
        d_x[1:n + 1], d_y[1:n + 1] = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            inv.undistort_points_device(d_x.data_ptr() + 4, d_y.data_ptr() + 4, n, stream.cuda_stream)
        stream.synchronize()
        gx, gy = d_x.cpu().numpy(), d_y.cpu().numpy()
        assert bits_equal(gx[1:n + 1], wx) and bits_equal(gy[1:n + 1], wy), (kind, n)
        assert gx[0] == -7 and gy[0] == -7 and (gx[n + 1:] == -7).all() and (gy[n + 1:] == -7).all(), (kind, n)  # nothing outside the n points
        if n == 65537:
            assert 1000 < np.isfinite(wx).sum() < n, kind  # both outcomes are among the points


def test_undistort_points_device_past_the_32_bit_index():
    """n = 2^31 + 257 points filled on the device (two launches): the first and last 1024 points and a stride of 2^20 + 1"""
    import torch

    kind, n = V.FOV, 2 ** 31 + 257
    d_x, d_y = torch.empty(n, dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.float32, device="cuda")
    step = 2 ** 27
    for a in range(0, n, step):
        i = torch.arange(a, min(n, a + step), device="cuda", dtype=torch.int64)
        d_x[a:a + step] = (i % 8191).float() * 0.015625 - 64.0
        d_y[a:a + step] = (i % 8179).float() * 0.015625 - 60.0
        del i
    idx = np.unique(np.concatenate([np.arange(1024), np.arange(n - 1024, n), np.arange(0, n, 2 ** 20 + 1)]))
    x = ((idx % 8191).astype(F) * F(0.015625) - F(64.0)).astype(F)
    y = ((idx % 8179).astype(F) * F(0.015625) - F(60.0)).astype(F)
    t_idx = torch.from_numpy(idx).cuda()
    assert bits_equal(d_x[t_idx].cpu().numpy(), x) and bits_equal(d_y[t_idx].cpu().numpy(), y)
    inverse_of(kind).undistort_points_device(d_x.data_ptr(), d_y.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    wx, wy = V.undistort(kind, INV_CAM[kind], INV_RECT, x, y)
    assert np.isfinite(wx).all()  # the whole square lies inside the model's half plane
    assert bits_equal(d_x[t_idx].cpu().numpy(), wx) and bits_equal(d_y[t_idx].cpu().numpy(), wy)


@pytest.mark.parametrize("name", TABLE_PROBLEMS)
def test_inverse_remap_device_equals_the_restatement(name, problems):
    import torch

    from mono_dataset_code_amd import capi

    q, wx, wy, woutside = problems[name]
    n = q["in_w"] * q["in_h"]
    d_ux, d_uy = torch.full((n + 1,), -7.0, device="cuda"), torch.full((n + 1,), -7.0, device="cuda")
    d_outside = torch.full((1,), 5, dtype=torch.int32, device="cuda")
    capi.LensInverse(model_of(q)).inverse_remap_device(d_ux.data_ptr(), d_uy.data_ptr(), d_outside.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    gx, gy = d_ux.cpu().numpy(), d_uy.cpu().numpy()
    assert bits_equal(gx[:n], wx) and bits_equal(gy[:n], wy) and gx[n] == -7 and gy[n] == -7
    assert int(d_outside.item()) == int(woutside) == int((wx == -1).any())


@pytest.mark.parametrize("name", ["barrel_crop", "fisheye_crop", "fov_small"])
def test_class_bulk_path_on_both_sides_of_the_threshold(name, problems, tmp_path):
    from mono_dataset_code_amd import capi

    q = problems[name][0]
    fov = capi.UndistorterFOV(LP.write_camera(tmp_path, LP.PROBLEMS.get(name) or V.SMALL_FOV))
    assert fov.is_valid() and fov.has_gpu()
    rng = np.random.default_rng(11)
    for n in (65536, 65535):
        x, y = rng.uniform(-20, q["in_w"] + 20, n).astype(F), rng.uniform(-20, q["in_h"] + 20, n).astype(F)
        wx, wy = V.undistort(q["kind"], q["cam"], q["rect"], x, y)
        fov.undistort_coordinates(x, y)
        assert bits_equal(x, wx) and bits_equal(y, wy), (name, n)
        assert np.isfinite(wx).sum() > n // 4, (name, n)
    inv = capi.LensInverse(fov.inverse_model())
    gx, gy = V.raw_grid(q)
    wx, wy = V.undistort(q["kind"], q["cam"], q["rect"], gx, gy)
    inv.undistort_points_host(gx, gy)
    assert bits_equal(gx, wx) and bits_equal(gy, wy)


@pytest.mark.parametrize("name", list(LP.SMALL) + ["fov_small"])
def test_round_trip_on_the_device(name, problems, tmp_path):
    """the rectified grid through distort_points_device, then undistort_points_device: back within the inverse's cap plus the forward
    one (tests/test_lens_inverse_cpu.py: round_trip_cap)"""
    import torch

    from mono_dataset_code_amd import capi

    q = problems[name][0]
    gx, gy = R.grid(q["out_w"], q["out_h"])
    n = gx.size
    d_x, d_y = torch.from_numpy(gx).cuda(), torch.from_numpy(gy).cuda()
    st = torch.cuda.current_stream().cuda_stream
    if q["kind"] == V.FOV:  # the forward FOV kernel is libmdc_hip.so's
        fov = capi.UndistorterFOV(LP.write_camera(tmp_path, V.SMALL_FOV))
        ctx = capi.Context(0)
        ctx.distort_points_device(fov.model(), d_x.data_ptr(), d_y.data_ptr(), n, st)
        inv = capi.LensInverse(fov.inverse_model())
    else:
        capi.Lens(model_of(q)).distort_points_device(d_x.data_ptr(), d_y.data_ptr(), n, st)
        inv = capi.LensInverse(model_of(q))
    inv.undistort_points_device(d_x.data_ptr(), d_y.data_ptr(), n, st)
    torch.cuda.synchronize()
    bx, by = d_x.cpu().numpy(), d_y.cpu().numpy()
    err = max(np.abs(bx - gx).max(), np.abs(by - gy).max())
    cap = round_trip_cap(q, max(gx.max(), gy.max()))
    print("%s: round trip %.3g px (cap %.3g)" % (name, err, cap))
    assert err <= cap, (name, err, cap)


@pytest.mark.parametrize("name", ["barrel_crop", "fisheye_crop"])
def test_frames_through_the_inverse_tables(name, problems, oracle):
    """the inverse tables loaded as remap tables, the two sizes swapped: three rectified frames re-distorted into raw geometry by
    the existing frame kernels equal the oracle's warp on the same tables"""
    import torch

    from mono_dataset_code_amd import capi

    q, ux, uy, _ = problems[name]
    W, H, w, h = q["in_w"], q["in_h"], q["out_w"], q["out_h"]
    ctx = capi.Context(0)
    ctx.set_remap(ux, uy, w, h, W, H)  # source: the rectified w x h image; result: the raw W x H one
    rng = np.random.default_rng(31)
    yy, xx = np.mgrid[0:h, 0:w]
    frames = np.stack([(rng.random(w * h) * 255).astype(F), (xx * 2.5 + yy * 1.25).astype(F).ravel(), np.full(w * h, 200.0, F)])
    d_in = torch.from_numpy(frames).cuda()
    d_out = torch.full((3, W * H), -7.0, dtype=torch.float32, device="cuda")
    ctx.undistort_batch_f32(d_in.data_ptr(), d_out.data_ptr(), 3, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    want = np.stack([oracle.undistort(f, ux, uy, w) for f in frames])
    assert bits_equal(d_out.cpu().numpy(), want), name
    assert (np.abs(want[2] - 200) < 0.01).sum() > W * H // 4  # a good part of the raw image is covered
    ctx.close()
