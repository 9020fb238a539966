"""The calibration tools' result images on the GPU: mdc_rcal_plot_e_device, mdc_rcal_plot_g_device, mdc_vcal_plot_plane_device and
mdc_vcal_vignette_u16_device (include/mdc_hip.h) equal tests/plots_restatement.py bit for bit; the 8-bit RGB kind of the device PNG
encoder (include/mdc_pngw_rgb.h, libmdc_pngw_rgb.so) equals the restatement's file byte for byte and PIL reads it back; bin/responseCalib leaves the
reference's files, each the restatement's render of the restatement's E or G of its iteration."""
import io
import os
import re
import subprocess

import numpy as np
import pytest

import plots_restatement as Q
import pngw_restatement as P
import rcal_restatement as R
from plots_restatement import bits, irradiance, plane_inputs, plot_g_inputs, vignette_inputs

pytestmark = pytest.mark.gpu
PATTERN = 0xA5
# one pass of rcal_plot_e_range_kernel's grid covers kPlotBlocks * kRcalThreads = 256 * 256 pixels (mdc_rcal.hip): one more takes the
# grid-stride loop's second round in exactly one lane
ONE_PASS = 256 * 256


@pytest.fixture(scope="module")
def ctx():
    from mono_dataset_code_amd import capi

    return capi.Context(0)


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def u16(t):
    return t.cpu().numpy().view(np.uint16)


# ---- plotE ------------------------------------------------------------------------------------------------------------------------


def check_plot_e(ctx, E, w, h):
    rgb, e16, rng = ctx.rcal_plot_e(dev(E), w, h)
    wrgb, we16, wrng = Q.plot_e(E)
    got = rgb.cpu().numpy().reshape(-1, 3)
    assert np.array_equal(got, wrgb), (w, h, int((got != wrgb).any(axis=1).sum()), np.flatnonzero((got != wrgb).any(axis=1))[:5])
    assert np.array_equal(u16(e16).reshape(-1), we16), (w, h)
    assert np.array_equal(bits(rng), bits(wrng)), (w, h, rng, wrng)


@pytest.mark.parametrize("w,h", [(1, 1), (2, 1), (63, 1), (8, 8), (5, 13), (257, 1), (33, 31), (32, 32), (41, 25), (ONE_PASS + 1, 1), (640, 480)])
def test_plot_e_equals_the_restatement(ctx, w, h):
    check_plot_e(ctx, irradiance(w * h, 100 + w), w, h)


@pytest.mark.parametrize("name", ["all_nan", "constant", "minus_zero_first", "plus_zero_first"])
def test_plot_e_degenerate_images(ctx, name):
    n = 1025
    E = {"all_nan": np.full(n, np.nan), "constant": np.full(n, 42.0)}.get(name)
    if E is None:  # equal zeros of both signs in different workgroups' shares: the first in index order is the minimum
        E = irradiance(ONE_PASS + 300, 7) + 1.0
        first, second = (-0.0, 0.0) if name == "minus_zero_first" else (0.0, -0.0)
        E[[700, ONE_PASS + 44]] = first
        E[[200 * 256 + 5, 701]] = second
        E[690] = first
        n = len(E)
    check_plot_e(ctx, E, n, 1)
    _, _, rng = ctx.rcal_plot_e(dev(E), n, 1)
    if name == "all_nan":
        assert rng == (1e10, -1e10)
    if name == "minus_zero_first":
        assert "%f" % rng[0] == "-0.000000"
    if name == "plus_zero_first":
        assert "%f" % rng[0] == "0.000000"


# ---- plotG ------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name,G", plot_g_inputs()[:3], ids=[n for n, _ in plot_g_inputs()[:3]])
def test_plot_g_equals_the_restatement(ctx, name, G):
    img, rng = ctx.rcal_plot_g(dev(G))
    want, wrng = Q.plot_g(G)
    assert np.array_equal(img.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert np.array_equal(bits(rng), bits(wrng))


# ---- displayImage -----------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("gw,gh", [(1, 1), (7, 5), (1000, 1000)])
def test_plot_plane_equals_the_restatement(ctx, gw, gh):
    rng = np.random.default_rng(gw)
    I = rng.uniform(-2.0, 120.0, gw * gh).astype(np.float32)
    if gw * gh > 1:
        I[rng.choice(gw * gh, max(2, gw * gh // 50), replace=False)] = np.nan
    rgb, r = ctx.vcal_plot_plane(dev(I), gw, gh)
    want, wr = Q.plot_plane(I)
    assert np.array_equal(rgb.cpu().numpy().reshape(-1, 3), want)
    assert np.array_equal(bits(r, np.float32), bits(wr, np.float32))


@pytest.mark.parametrize("name,I", plane_inputs(), ids=[n for n, _ in plane_inputs()])
def test_plot_plane_directed_inputs(ctx, name, I):
    rgb, r = ctx.vcal_plot_plane(dev(I), len(I), 1)
    want, wr = Q.plot_plane(I)
    assert np.array_equal(rgb.cpu().numpy().reshape(-1, 3), want)
    assert np.array_equal(bits(r, np.float32), bits(wr, np.float32))


# ---- vignette.png's quantisation --------------------------------------------------------------------------------------------------


def test_vignette_u16_equals_the_restatement(ctx):
    import torch

    I = vignette_inputs()
    assert np.array_equal(u16(ctx.vcal_vignette_u16(dev(I))), Q.vignette_u16(I))
    big = np.random.default_rng(8).uniform(0.0, 1.02, 1280 * 1024).astype(np.float32)
    big[::1001] = np.nan
    assert np.array_equal(u16(ctx.vcal_vignette_u16(dev(big))), Q.vignette_u16(big))
    # an odd count from an odd element of both arrays; nothing outside the range is written
    n = 1001
    d_in = dev(big[:n + 8])
    d_out = torch.full((n + 8,), 0x5A5A, dtype=torch.int16, device="cuda")
    ctx.vcal_vignette_u16(d_in[3:3 + n], d_out[1:1 + n])
    out = u16(d_out)
    assert np.array_equal(out[1:1 + n], Q.vignette_u16(big[3:3 + n])) and out[0] == 0x5A5A and (out[1 + n:] == 0x5A5A).all()


# ---- the RGB kind of the PNG encoder ----------------------------------------------------------------------------------------------


def rgb_encode(images, filt, in_offset=0, out_offset=0, slot=None, stride=None):
    """images: equal-shaped (h, w, 3) arrays, one call; `stride` bytes apart from byte in_offset, files `slot` bytes apart from byte
    out_offset of a pattern-filled array -> the files; nothing but [f * slot, f * slot + size) is written"""
    import torch

    from mono_dataset_code_amd import capi

    n, (h, w, _) = len(images), images[0].shape
    stride = stride or 3 * w * h
    enc = capi.PngEncoder(w, h, filter=filt, max_images=n, device=0, rgb=True)
    assert enc.bound == Q.png_bound_rgb8(w, h)
    slot = slot or enc.bound
    host_in = np.full(in_offset + n * stride + 64, PATTERN, np.uint8)
    for i, img in enumerate(images):
        host_in[in_offset + i * stride:in_offset + i * stride + 3 * w * h] = img.reshape(-1)
    d_in = torch.from_numpy(host_in).cuda()
    d_out = torch.full((out_offset + n * slot + 64,), PATTERN, dtype=torch.uint8, device="cuda")
    d_sizes = torch.full((n + 4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    enc.encode(d_in.data_ptr() + in_offset, n, kind="rgb8", stride=stride, d_out=d_out.data_ptr() + out_offset, slot_bytes=slot, d_sizes=d_sizes.data_ptr())
    torch.cuda.synchronize()
    enc.close()
    sizes, out = d_sizes.cpu().numpy(), d_out.cpu().numpy()
    assert (sizes[n:] == 0x5A5A5A5A).all() and (out[:out_offset] == PATTERN).all() and (d_in.cpu().numpy() == host_in).all()
    files = []
    for f in range(n):
        size, at = int(sizes[f]), out_offset + f * slot
        assert 0 < size <= enc.bound
        end = at + slot if f + 1 < n else len(out)
        assert (out[at + size:end] == PATTERN).all(), "file %d: written behind its size" % f
        files.append(out[at:at + size].tobytes())
    return files


def check_rgb(files, images, filt, stored=None):
    from PIL import Image

    for f, (got, img) in enumerate(zip(files, images)):
        want, was_stored = Q.encode_rgb(img, filt)
        assert got == want, (f, img.shape, filt, len(got), len(want), [i for i in range(min(len(got), len(want))) if got[i] != want[i]][:8])
        assert ((got[43] >> 1) & 3) == (0 if was_stored else 2)  # BTYPE of the first block
        if stored is not None:
            assert was_stored == stored[f], (f, was_stored)
        im = Image.open(io.BytesIO(got))
        assert im.mode == "RGB" and np.array_equal(np.array(im), img)


def rgb_contents(w, h, seed):
    """noise (the stored form), a smooth picture (the dynamic form), one colour"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    smooth = np.stack([xx * 2 + yy, xx + yy * 3, (xx * yy) // 16], axis=2).astype(np.uint8)
    return [rng.integers(0, 256, (h, w, 3)).astype(np.uint8), smooth, np.full((h, w, 3), (9, 200, 77), np.uint8)]


@pytest.mark.parametrize("filt", [0, 1, 2, 3, 4, P.ADAPTIVE])
@pytest.mark.parametrize("w,h", [(1, 1), (2, 3), (5, 4), (7, 1), (97, 31)])  # w = 5: a row is 16 filtered bytes, the scratch arrays' unit
def test_rgb_files_equal_the_restatement(w, h, filt):
    images = rgb_contents(w, h, w * 10 + filt)
    check_rgb(rgb_encode(images, filt), images, filt, stored=[True, False, False] if (w, h) == (97, 31) else None)


def test_rgb_batch_strides_and_odd_addresses():
    w, h = 33, 9
    images = rgb_contents(w, h, 1)
    bound = Q.png_bound_rgb8(w, h)
    files = rgb_encode(images, P.ADAPTIVE, in_offset=5, out_offset=3, slot=bound + (bound % 2 == 0) + 6, stride=3 * w * h + 7)
    check_rgb(files, images, P.ADAPTIVE, stored=[True, False, False])


def test_rgb_encoder_and_gray_entry_points_refuse_each_other():
    import torch

    from mono_dataset_code_amd import capi

    d = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    rgb, gray = capi.PngEncoder(4, 4, rgb=True, device=0), capi.PngEncoder(4, 4, depth=8, device=0)
    with pytest.raises(capi.MdcError):
        rgb.encode(d.data_ptr(), 1, kind="u8")
    with pytest.raises(capi.MdcError):
        gray.encode(d.data_ptr(), 1, kind="rgb8")
    with pytest.raises(capi.MdcError):
        rgb.encode(d.data_ptr(), 1, kind="rgb8", stride=3 * 16 - 1)
    assert capi.pngw_rgb_lib().mdcp_png_bound_rgb8(0, 4) == -1 and capi.pngw_rgb_lib().mdcp_png_bound_rgb8(1 << 20, 1 << 10) == -1
    rgb.close()
    gray.close()


# ---- bin/responseCalib ------------------------------------------------------------------------------------------------------------


def write_sweep(d, stack, t):
    from PIL import Image

    os.makedirs(os.path.join(d, "images"))
    for i, img in enumerate(stack):
        Image.fromarray(img).save(os.path.join(d, "images", "%05d.png" % i), "PNG")
    with open(os.path.join(d, "times.txt"), "w") as f:
        for i, ti in enumerate(t):
            f.write("%d %.6f %.9g\n" % (i, 1000.0 + i / 20.0, ti))


def run_program(d, run, *args):
    from mono_dataset_code_amd import build

    os.makedirs(run)
    p = subprocess.run([build.RESPONSE_CALIB, d, "iterations=3"] + list(args), cwd=run, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    return p.stdout


def test_response_calib_writes_the_reference_files(tmp_path):
    from PIL import Image

    w, h, n, its = 64, 48, 8, 3
    stack, t, _ = R.synthetic_sweep(np.random.default_rng(31), n, w, h, t_lo=0.4, t_hi=40.0, noise=1.5)
    stack[:, 1, 2] = 255  # saturated in every frame: E is NaN there after the E step, a black pixel
    t = t.astype(np.float32).astype(np.float64)  # getExposure is a float
    d = str(tmp_path / "sweep")
    write_sweep(d, stack, t)
    out1 = run_program(d, str(tmp_path / "plots1"))
    out0 = run_program(d, str(tmp_path / "plots0"), "plots=0")
    res1, res0 = tmp_path / "plots1" / "photoCalibResult", tmp_path / "plots0" / "photoCalibResult"

    names = ["E-0.png", "E-016.png", "log.txt", "pcalib.txt"] + [s % k for k in range(1, its + 1) for s in ("G-%d.png", "E-%d.png", "E-%d16.png")]
    assert sorted(os.listdir(res1)) == sorted(names)
    assert sorted(os.listdir(res0)) == ["log.txt", "pcalib.txt"] and "Irradiance" not in out0 and "Inv. Response" not in out0
    for name in ("log.txt", "pcalib.txt"):
        assert open(res1 / name, "rb").read() == open(res0 / name, "rb").read(), name

    def check_e(E, stem):
        rgb, e16, rng = Q.plot_e(E)
        im = Image.open(res1 / (stem + ".png"))
        assert im.mode == "RGB" and np.array_equal(np.array(im), rgb.reshape(h, w, 3)), stem
        assert open(res1 / (stem + ".png"), "rb").read() == Q.encode_rgb(rgb.reshape(h, w, 3), P.ADAPTIVE)[0], stem
        assert np.array_equal(np.array(Image.open(res1 / (stem + "16.png"))).astype(np.uint16), e16.reshape(h, w)), stem
        return "Irradiance %f - %f" % rng

    padded = R.leak_pad(stack, w, h, 2)
    E, G = R.init_e(padded), np.zeros(256)
    lines = [check_e(E, "E-0")]
    for k in range(1, its + 1):
        G = R.g_step(E, t, padded)
        img, rng = Q.plot_g(G)
        assert np.array_equal(np.array(Image.open(res1 / ("G-%d.png" % k))), P.f32_to_u8(img)), k
        lines.append("Inv. Response %f - %f" % rng)
        E = R.e_step(G, t, padded)
        assert np.isnan(E[1 * w + 2])
        lines.append(check_e(E, "E-%d" % k))
        G, E, _ = R.rescale(G, E)
    assert re.findall(r"(?:Irradiance|Inv\. Response) \S+ - \S+", out1) == lines
    # the reference's order: every picture's line follows its RMSE fragment (:272-273, :307-310, :342-345)
    marks = re.findall(r"init RMSE|optG RMSE|OptE RMSE|resc RMSE|Irradiance|Inv\. Response", out1)
    assert marks == ["init RMSE", "Irradiance"] + ["optG RMSE", "Inv. Response", "OptE RMSE", "Irradiance", "resc RMSE"] * its
    assert "init RMSE = " in out1 and re.search(r"init RMSE = \S+! \tIrradiance", out1) and re.search(r"optG RMSE = \S+! \tInv\. Response", out1)


def test_response_calib_direct_order_with_plots(tmp_path):
    """order=direct through the step calls: the direct G step is deterministic, not bitwise the reference's, so the pictures are held to
    their names, kinds and sizes, and the text files to the plots=0 run of the same order, byte for byte"""
    from PIL import Image

    w, h, n, its = 64, 48, 8, 3
    stack, t, _ = R.synthetic_sweep(np.random.default_rng(32), n, w, h, t_lo=0.4, t_hi=40.0, noise=1.5)
    d = str(tmp_path / "sweep")
    write_sweep(d, stack, t.astype(np.float32).astype(np.float64))
    out1 = run_program(d, str(tmp_path / "plots1"), "order=direct")
    run_program(d, str(tmp_path / "plots0"), "order=direct", "plots=0")
    res1, res0 = tmp_path / "plots1" / "photoCalibResult", tmp_path / "plots0" / "photoCalibResult"
    for name in ("log.txt", "pcalib.txt"):
        assert open(res1 / name, "rb").read() == open(res0 / name, "rb").read(), name
    kinds = {"E-0.png": ("RGB", (w, h)), "E-016.png": ("I;16", (w, h))}
    for k in range(1, its + 1):
        kinds.update({"G-%d.png" % k: ("L", (256, 256)), "E-%d.png" % k: ("RGB", (w, h)), "E-%d16.png" % k: ("I;16", (w, h))})
    assert sorted(os.listdir(res1)) == sorted(list(kinds) + ["log.txt", "pcalib.txt"])
    for name, (mode, size) in kinds.items():
        im = Image.open(res1 / name)
        im.load()
        assert (im.mode, im.size) == (mode, size), (name, im.mode, im.size)
    assert len(re.findall(r"Irradiance \S+ - \S+", out1)) == its + 1 and len(re.findall(r"Inv\. Response \S+ - \S+", out1)) == its
