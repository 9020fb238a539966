"""RadTan / EquiDistant / pinhole cameras on the GPU: libmdc_lens.so's kernels and the class's bulk path against the NumPy
restatement (tests/lens_restatement.py), and the frame kernels -- the planned tile kernel and the gather kernel -- on the tables of
such cameras (pincushion, tangential skew, fisheye) against the oracle.  Bit for bit throughout."""
import os
import subprocess

import numpy as np
import pytest

import lens_problems as LP
import lens_restatement as R
from conftest import bits_equal, test_frames as make_frames
from test_lens_cpu import R_CAM, R_RECT, R_SEED, random_points

pytestmark = pytest.mark.gpu
F = np.float32
KINDS = (0, R.RADTAN, R.EQUIDISTANT)


def lens_of(kind):
    from mono_dataset_code_amd import capi

    return capi.Lens(capi.LensModel.make(kind, R_CAM[kind], R_RECT))


@pytest.mark.parametrize("kind", KINDS)
def test_distort_points_device_equals_the_restatement(kind):
    """n = 0, 1, 255, 256, 257, 65 537; arrays offset by one float; a stream of its own"""
    import torch

    lens = lens_of(kind)
    stream = torch.cuda.Stream()
    for n in (0, 1, 255, 256, 257, 65537):
        x, y = random_points(R_SEED[kind], np.arange(n), R_RECT)
        wx, wy = R.distort(kind, R_CAM[kind], R_RECT, x, y)
        d_x, d_y = torch.full((n + 3,), -7.0, device="cuda"), torch.full((n + 3,), -7.0, device="cuda")
        d_x[1:n + 1], d_y[1:n + 1] = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            lens.distort_points_device(d_x.data_ptr() + 4, d_y.data_ptr() + 4, n, stream.cuda_stream)
        stream.synchronize()
        gx, gy = d_x.cpu().numpy(), d_y.cpu().numpy()
        assert bits_equal(gx[1:n + 1], wx) and bits_equal(gy[1:n + 1], wy), (kind, n)
        assert gx[0] == -7 and gy[0] == -7 and (gx[n + 1:] == -7).all() and (gy[n + 1:] == -7).all(), (kind, n)  # nothing outside the n points


def test_distort_points_device_past_the_32_bit_index():
    """n = 2^31 + 257 points filled on the device (two launches): the first and last 1024 points and a stride of 2^20 + 1"""
    import torch

    kind, n = R.EQUIDISTANT, 2 ** 31 + 257
    d_x, d_y = torch.empty(n, dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.float32, device="cuda")
    step = 2 ** 27
    for a in range(0, n, step):
        i = torch.arange(a, min(n, a + step), device="cuda", dtype=torch.int64)
        d_x[a:a + step] = (i % 8191).float() * 0.03125 - 20.0
        d_y[a:a + step] = (i % 8179).float() * 0.03125 - 30.0
        del i
    idx = np.unique(np.concatenate([np.arange(1024), np.arange(n - 1024, n), np.arange(0, n, 2 ** 20 + 1)]))
    x = ((idx % 8191).astype(F) * F(0.03125) - F(20.0)).astype(F)
    y = ((idx % 8179).astype(F) * F(0.03125) - F(30.0)).astype(F)
    t_idx = torch.from_numpy(idx).cuda()
    assert bits_equal(d_x[t_idx].cpu().numpy(), x) and bits_equal(d_y[t_idx].cpu().numpy(), y)
    lens_of(kind).distort_points_device(d_x.data_ptr(), d_y.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    wx, wy = R.distort(kind, R_CAM[kind], R_RECT, x, y)
    assert bits_equal(d_x[t_idx].cpu().numpy(), wx) and bits_equal(d_y[t_idx].cpu().numpy(), wy)


@pytest.fixture(scope="module")
def objects(tmp_path_factory):
    """name -> (UndistorterFOV, PhotometricUndistorter, folder) of every problem, made once"""
    from mono_dataset_code_amd import capi, synth

    out = {}
    for name, lines in LP.PROBLEMS.items():
        d = synth.write_sequence_calibration(str(tmp_path_factory.mktemp(name)), lines)
        fov = capi.UndistorterFOV(os.path.join(d, "camera.txt"))
        W, H, _, _ = fov.dims()
        photo = capi.PhotometricUndistorter(os.path.join(d, "pcalib.txt"), os.path.join(d, "vignette.png"), W, H)
        assert fov.is_valid() and fov.has_gpu() and photo.valid() == 3, name
        out[name] = (fov, photo, d)
    return out


@pytest.mark.parametrize("name", list(LP.PROBLEMS))
def test_remap_device_equals_the_class_tables(name, objects):
    import torch

    from mono_dataset_code_amd import capi

    fov = objects[name][0]
    rx, ry = fov.remap()
    m = fov.mdcn_model()
    n = m.out_w * m.out_h
    d_rx, d_ry = torch.full((n + 1,), -7.0, device="cuda"), torch.full((n + 1,), -7.0, device="cuda")
    d_black = torch.full((1,), 5, dtype=torch.int32, device="cuda")
    capi.Lens(m).remap_device(d_rx.data_ptr(), d_ry.data_ptr(), d_black.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    gx, gy = d_rx.cpu().numpy(), d_ry.cpu().numpy()
    assert bits_equal(gx[:n], rx) and bits_equal(gy[:n], ry) and gx[n] == -7 and gy[n] == -7
    assert int(d_black.item()) == int((rx == -1).any()) == int(name == "pincushion_explicit_black")


@pytest.mark.parametrize("name", ["barrel_crop", "pincushion_explicit_black", "fisheye_crop"])
def test_class_bulk_path_on_both_sides_of_the_threshold(name, objects):
    from mono_dataset_code_amd import capi

    fov = objects[name][0]
    p = R.parse(LP.PROBLEMS[name])
    rng = np.random.default_rng(11)
    for n in (65536, 65535):
        x, y = rng.uniform(-20, 90, n).astype(F), rng.uniform(-20, 70, n).astype(F)
        wx, wy = R.distort(p["kind"], p["cam"], p["rect"], x, y)
        fov.distort_coordinates(x, y)
        assert bits_equal(x, wx) and bits_equal(y, wy), (name, n)
    x, y = np.arange(4, dtype=F), np.arange(4, dtype=F)
    for bad in (capi.LensModel.make(7, R_CAM[R.RADTAN], R_RECT), capi.LensModel.make(capi.LENS_RADTAN, R_CAM[R.RADTAN], (0.0, 1.0, 0.0, 0.0))):
        with pytest.raises(capi.MdcError) as e:
            capi.Lens(bad).distort_points_host(x, y)
        assert e.value.code == capi.ERR_ARG and x.tolist() == [0, 1, 2, 3]
    good = capi.Lens(fov.mdcn_model())
    gx, gy = R.grid(p["out_w"], p["out_h"])
    wx, wy = R.distort(p["kind"], p["cam"], p["rect"], gx, gy)
    good.distort_points_host(gx, gy)
    assert bits_equal(gx, wx) and bits_equal(gy, wy)


def run_frames(name, objects, oracle, trials, rng):
    import torch

    from mono_dataset_code_amd import capi

    fov, photo, _ = objects[name]
    W, H, w, h = fov.dims()
    rx, ry = fov.remap()
    ginv, vinv = photo.ginv(), photo.vignette()[1]
    ctx = capi.Context(0)
    ctx.bind(fov, photo)
    frames = np.stack(make_frames(W, H, n_noise=2))
    n = len(frames)
    d_in = torch.from_numpy(frames).cuda()
    st = torch.cuda.current_stream().cuda_stream
    want = {}
    for trial in range(trials):
        if rng is not None:
            rows = int(rng.choice([16, 32, 60, 64]))
            cols = int(rng.choice([64, 128])) if rows in (16, 32) else 64
            ctx.set_option(capi.OPT_TILE_COLS, cols)
            ctx.set_option(capi.OPT_TILE_ROWS, rows)
            ctx.set_option(capi.OPT_WINDOW_BUFFERS, int(rng.choice([0, 2, 3, 4])))
            ctx.set_option(capi.OPT_FRAME_INTERLEAVE, int(rng.integers(0, 2)))
            g, v, o = (int(x) for x in rng.integers(0, 2, 3))
            levels = int(rng.integers(1, 5))
        else:
            rows = cols = 0
            g, v, o, levels = 1, 1, 1, 3
        flags = capi.RECTIFY | (capi.GAMMA * g) | (capi.VIGNETTE * v) | (capi.KILL_OVEREXPOSED * o)
        if (g, v, o) not in want:
            want[(g, v, o)] = np.stack([oracle.get_image(f, W, H, w, h, ginv, vinv, True, True, rx, ry, 1, g, v, o) for f in frames])
        d_out = torch.full((n, w * h), -7.0, dtype=torch.float32, device="cuda")
        lv = [torch.full((n * (w >> l) * (h >> l),), -7.0, dtype=torch.float32, device="cuda") for l in range(1, levels)]
        ctx.process_pyramid_batch(d_in.data_ptr(), d_out.data_ptr(), levels, [t.data_ptr() for t in lv], n, flags, st)
        torch.cuda.synchronize()
        info = ctx.info()
        tag = (name, trial, rows, cols, info.tiled, g, v, o, levels)
        assert bool(info.tiled) == (W % 16 == 0), tag  # the planned tile kernel really ran on these tables (the gather kernel where it cannot)
        assert bits_equal(d_out.cpu().numpy(), want[(g, v, o)]), tag
        for f in range(n):
            src, cw, ch = want[(g, v, o)][f], w, h
            for l in range(levels - 1):
                nxt = oracle.pyramid_level(src, cw, ch)
                assert bits_equal(lv[l].view(n, -1)[f].cpu().numpy(), nxt), tag + (f, l + 1)
                src, cw, ch = nxt, cw // 2, ch // 2
        if trial % 2 == 0:
            fin = np.stack([oracle.unmap(f, ginv, vinv, True, True, 1, 1, 1) for f in frames[:3]])
            d_f = torch.from_numpy(fin).cuda()
            d_u = torch.full((3, w * h), -7.0, dtype=torch.float32, device="cuda")
            ctx.undistort_batch_f32(d_f.data_ptr(), d_u.data_ptr(), 3, st)
            torch.cuda.synchronize()
            assert bits_equal(d_u.cpu().numpy(), np.stack([oracle.undistort(x, rx, ry, W) for x in fin])), tag
    ctx.close()


@pytest.mark.parametrize("name", list(LP.SMALL) + ["barrel_ragged"])
def test_frames_through_random_tile_options(name, objects, oracle):
    """six seeded combinations of the tile options tests/test_gpu_random.py draws from, per camera"""
    run_frames(name, objects, oracle, 6, np.random.default_rng(sorted(LP.PROBLEMS).index(name) + 2000))


@pytest.mark.parametrize("name", list(LP.FULL))
def test_frames_at_full_size_with_default_options(name, objects, oracle):
    run_frames(name, objects, oracle, 1, None)


@pytest.mark.parametrize("name", ["barrel_crop", "pincushion_explicit_black", "fisheye_crop"])
def test_bounds_checked_kernels_on_lens_tables(name, objects):
    """the bounds-checking build (every LDS tap, staging chunk and gather index checked in the kernel): no check fires, and the
    results are the product build's"""
    import importlib.util

    import torch

    from mono_dataset_code_amd import build, capi

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("capi_debug_lens", os.path.join(root, "mono_dataset_code_amd", "capi.py"))
    dbg_capi = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(dbg_capi)
    dbg_capi.LIB_HIP_PATH = build.build_debug()
    fov, photo, _ = objects[name]
    W, H, w, h = fov.dims()
    blob = capi.pack_tables(fov, photo)
    prod, dbg = capi.Context(0), dbg_capi.Context(0)
    prod.import_tables(blob)
    dbg.import_tables(blob)
    frames = np.stack(make_frames(W, H, n_noise=2))
    n = len(frames)
    d_in = torch.from_numpy(frames).cuda()
    st = torch.cuda.current_stream().cuda_stream
    fin = torch.rand((n, W * H), device="cuda") * 255
    for cols, rows in ((64, 16), (64, 32), (64, 60), (64, 64), (128, 16), (128, 32), (0, 0)):
        for c, m in ((prod, capi), (dbg, dbg_capi)):
            c.set_option(m.OPT_TILE_COLS, cols)
            c.set_option(m.OPT_TILE_ROWS, rows)
        for kernel in (capi.KERNEL_AUTO, capi.KERNEL_GATHER):
            prod.set_option(capi.OPT_KERNEL, kernel)
            dbg.set_option(dbg_capi.OPT_KERNEL, kernel)
            for flags in (15, 8):
                a = torch.full((n, w * h), -7.0, device="cuda")
                b = torch.full((n, w * h), -7.0, device="cuda")
                prod.process_batch(d_in.data_ptr(), a.data_ptr(), n, flags, st)
                dbg.process_batch(d_in.data_ptr(), b.data_ptr(), n, flags, st)
                torch.cuda.synchronize()  # a trapped kernel surfaces here as a HIP error
                assert bits_equal(a.cpu().numpy(), b.cpu().numpy()), (name, cols, rows, kernel, flags)
            a = torch.full((n, w * h), -7.0, device="cuda")
            b = torch.full((n, w * h), -7.0, device="cuda")
            prod.undistort_batch_f32(fin.data_ptr(), a.data_ptr(), n, st)
            dbg.undistort_batch_f32(fin.data_ptr(), b.data_ptr(), n, st)
            torch.cuda.synchronize()
            assert bits_equal(a.cpu().numpy(), b.cpu().numpy()), (name, cols, rows, kernel, "f32")


def test_rectify_dataset_round_trip(tmp_path):
    """rectifyDataset on a 4-frame RadTan dataset: the export's camera.txt is the rectified pinhole (a bare line, omega 0), it opens
    again with identity tables, getImagesDevice returns the exported frames, and on the source getImagesDevice equals getImages"""
    import torch

    from mono_dataset_code_amd import build, capi, synth

    lines = (LP.BARREL, LP.SMALL_IN, "crop", LP.SMALL_OUT)
    W, H, w, h = 96, 80, 64, 48
    d, out = str(tmp_path / "seq"), str(tmp_path / "rect")
    synth.write_sequence_calibration(d, lines, vignette_bits=16, n_times=4)
    os.makedirs(os.path.join(d, "images"))
    for i in range(4):
        f = synth.noise_frames(11, 1, W * H)[0] if i == 1 else synth.smooth_frame(W, H, 0.7 + i, blobs=i % 2 == 0)
        synth.write_png_gray(os.path.join(d, "images", "%05d.png" % i), f.reshape(H, W))
    r = subprocess.run([build.RECTIFY_DATASET, d, out, "frames=png"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    src_fov = capi.UndistorterFOV(os.path.join(d, "camera.txt"))
    K = src_fov.intrinsics()["K_rect"]
    cam = open(os.path.join(out, "camera.txt")).read().splitlines()
    want1 = "%.9g %.9g %.9g %.9g 0" % (K[0, 0] / F(w), K[1, 1] / F(h), (K[0, 2] + F(0.5)) / F(w), (K[1, 2] + F(0.5)) / F(h))
    assert cam[:4] == [want1, "%d %d" % (w, h), "crop", "%d %d" % (w, h)]
    exp_fov = capi.UndistorterFOV(os.path.join(out, "camera.txt"))
    assert exp_fov.is_valid() and exp_fov.lens_model()[0] == 0 and exp_fov.dims() == (w, h, w, h) and exp_fov.intrinsics()["omega"] == 0
    rx, ry = (t.reshape(h, w) for t in exp_fov.remap())
    gx, gy = (t.reshape(h, w) for t in R.grid(w, h))
    # identity: (x - c) / f * f + c in float is x to a few units in the last place of 64; the first / last row and column are nudged by 0.01
    assert np.abs(rx - gx)[:, 1:-1].max() <= 64 * 2.0 ** -20 and np.abs(ry - gy)[1:-1, :].max() <= 64 * 2.0 ** -20
    assert np.abs(rx - gx).max() <= 0.0101 and np.abs(ry - gy).max() <= 0.0101 and (rx > 0).all() and (ry > 0).all()
    # the source: device results are the host-array results
    src = capi.DatasetReader(d)
    assert len(src) == 4 and (src.in_w, src.in_h, src.out_w, src.out_h) == (W, H, w, h)
    host, ok, got = src.get_images(0, 4, True, True, True, False)
    assert got == 4 and ok.all()
    d_base = torch.full((4, w * h), -7.0, dtype=torch.float32, device="cuda:%d" % src.device())
    valid, got = src.get_images_device(0, 4, True, True, True, False, capi.DeviceOutputs.make(d_base.data_ptr()))
    torch.cuda.synchronize()
    assert got == 4 and valid.all() and bits_equal(d_base.cpu().numpy(), host)
    from pngw_restatement import f32_to_u8

    plain = [f32_to_u8(src.get_image(i, True, False, False, False)[0]) for i in range(4)]
    src.close()
    # the export: its raw frames are the rectified frames, and getImagesDevice hands them back
    exp = capi.DatasetReader(out)
    assert len(exp) == 4 and (exp.in_w, exp.in_h) == (w, h)
    for i in range(4):
        assert np.array_equal(exp.get_raw(i), plain[i]), i
    d_raw = torch.full((4, w * h), -7.0, dtype=torch.float32, device="cuda:%d" % exp.device())
    valid, got = exp.get_images_device(0, 4, False, False, False, False, capi.DeviceOutputs.make(d_raw.data_ptr()))
    torch.cuda.synchronize()
    assert got == 4 and valid.all()
    assert np.array_equal(d_raw.cpu().numpy().reshape(4, h, w), np.stack(plain).astype(F))
    exp.close()
