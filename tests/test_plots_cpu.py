"""tests/plots_restatement.py, CPU side: every vectorised render equals a literal scalar transcription of the reference's loop
(src/main_responseCalib.cpp:72-146, src/main_vignetteCalib.cpp:72-94, :568-583; C's conversions spelt out as x86 performs them) on
small inputs with NaN pixels, an all-NaN image, a constant image, a plane whose maximum lands on either side of 255 and vignette values
at 0, at exact ties, past the 16-bit range and NaN; every RGB file of the restatement inflates (zlib) to its filtered bytes, is read by
PIL as mode RGB with the input's pixels, and has the size the bound promises in the stored form."""
import io
import math
import zlib

import numpy as np
import pytest

import plots_restatement as Q
import pngw_restatement as P

F = np.float32
D = np.float64


def c_int(v):
    """(int)v of a float or double on x86"""
    v = float(v)
    if v != v or not (-2147483649.0 < v < 2147483648.0):
        return Q.INT_MIN
    return int(v)


# ---- literal transcriptions -----------------------------------------------------------------------------------------------------


def scalar_plot_e(E):
    offset = 20.0
    mn, mx, Emin, Emax = 1e10, -1e10, 1e10, -1e10
    for v in E:
        le = Q.c_log(v + offset)
        if le < mn:
            mn = le
        if le > mx:
            mx = le
        if v < Emin:
            Emin = v
        if v > Emax:
            Emax = v
    rgb, e16 = [], []
    with np.errstate(all="ignore"):
        for v in E:
            val = F(3 * (D(Q.c_exp(float((D(Q.c_log(v + offset)) - D(mn)) / (D(mx) - D(mn))))) - 1) / 1.7183)
            icP = c_int(val)
            ifP = F(val - F(icP))
            icP = int(math.fmod(icP, 3))
            color = (0, 0, 0)  # cv::Vec3b(): B, G, R
            if icP == 0:
                color = (0, 0, c_int(F(255) * ifP) & 255)
            if icP == 1:
                color = (0, c_int(F(255) * ifP) & 255, 255)
            if icP == 2:
                color = (c_int(F(255) * ifP) & 255, 255, 255)
            rgb.append(color[::-1])  # the file holds R, G, B
            e16.append(c_int(D(255 * 255) * (D(v) - D(Emin)) / (D(Emax) - D(Emin))) & 0xFFFF)
    return np.array(rgb, np.uint8).reshape(-1, 3), np.array(e16, np.uint16), (Emin, Emax)


def scalar_plot_g(G):
    img = np.zeros((256, 256), np.float32)
    mn, mx = 1e10, -1e10
    for i in range(256):
        if G[i] < mn:
            mn = G[i]
        if G[i] > mx:
            mx = G[i]
    with np.errstate(all="ignore"):
        for i in range(256):
            val = D(256) * (D(G[i]) - D(mn)) / (D(mx) - D(mn))
            for k in range(256):
                if val < k:
                    img[k, i] = F(k - val)
    return img * F(255), (mn, mx)


def scalar_plot_plane(I):
    vmin, vmax = F(1e10), F(-1e10)
    for v in I:
        if vmin > v:
            vmin = v
        if vmax < v:
            vmax = v
    rgb = []
    with np.errstate(all="ignore"):
        for v in I:
            if v != v:
                rgb.append((255, 0, 0))  # Vec3b(0, 0, 255) is B, G, R
            else:
                c = c_int((F(255) * (v - vmin)) / (vmax - vmin)) & 255
                rgb.append((c, c, c))
    return np.array(rgb, np.uint8).reshape(-1, 3), (vmin, vmax)


def scalar_vignette_u16(I):
    s = F(254.9 * 254.9)
    out = []
    with np.errstate(all="ignore"):
        for v in I:
            x = F(v) * s
            if x != x:
                out.append(0)
                continue
            r = float(np.rint(x))  # cvRound: the nearest integer, ties to even
            out.append(int(min(max(r, 0.0), 65535.0)))
    return np.array(out, np.uint16)


# ---- the renders ----------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name,E", Q.plot_e_inputs(), ids=[n for n, _ in Q.plot_e_inputs()])
def test_plot_e_equals_the_transcription(name, E):
    rgb, e16, rng = Q.plot_e(E)
    wrgb, we16, wrng = scalar_plot_e([float(v) for v in E])
    assert np.array_equal(rgb, wrgb) and np.array_equal(e16, we16)
    assert np.array_equal(Q.bits(rng), Q.bits(wrng))
    if name == "all_nan":
        assert rng == (1e10, -1e10) and not rgb.any() and not e16.any()
    if name == "constant":
        assert not rgb.any() and not e16.any()  # max == min: val is NaN, the quotient too
    if name == "minus_zero_first":
        assert math.copysign(1.0, rng[0]) == -1.0 and "%f" % rng[0] == "-0.000000"
    if name == "plus_zero_first":
        assert math.copysign(1.0, rng[0]) == 1.0
    if name.startswith("random"):
        assert len({tuple(p) for p in rgb}) > 10 and e16.max() == 65025


def test_plot_e_covers_the_three_colour_bands():
    E = np.linspace(0.0, 300.0, 200)
    rgb, _, _ = Q.plot_e(E)
    assert (rgb[:, 1] == 0).any() and ((rgb[:, 0] == 255) & (rgb[:, 2] == 0)).any() and ((rgb[:, 1] == 255) & (rgb[:, 0] == 255)).any()
    assert np.array_equal(rgb, scalar_plot_e([float(v) for v in E])[0])


@pytest.mark.parametrize("name,G", Q.plot_g_inputs(), ids=[n for n, _ in Q.plot_g_inputs()])
def test_plot_g_equals_the_transcription(name, G):
    img, rng = Q.plot_g(G)
    want, wrng = scalar_plot_g([float(v) for v in G])
    assert img.dtype == np.float32 and np.array_equal(img.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(Q.bits(rng), Q.bits(wrng))
    if name in ("constant", "all_nan"):
        assert not img.any()
    if name == "nan_0_1_200":
        assert not img[:, [0, 1, 200]].any() and img[:, 2].any()


@pytest.mark.parametrize("name,I", Q.plane_inputs(), ids=[n for n, _ in Q.plane_inputs()])
def test_plot_plane_equals_the_transcription(name, I):
    rgb, rng = Q.plot_plane(I)
    want, wrng = scalar_plot_plane(list(I))
    assert np.array_equal(rgb, want)
    assert np.array_equal(Q.bits(rng, np.float32), Q.bits(wrng, np.float32))
    if name == "max_gives_254":
        assert tuple(rgb[2]) == (254, 254, 254)
    if name == "max_gives_255":
        assert tuple(rgb[2]) == (255, 255, 255)
    if name == "all_nan":
        assert (rgb == (255, 0, 0)).all() and rng == (F(1e10), F(-1e10))
    if name == "zeros":
        assert math.copysign(1.0, float(rng[0])) == -1.0


def test_vignette_u16_equals_the_transcription():
    I = Q.vignette_inputs()
    got = Q.vignette_u16(I)
    assert np.array_equal(got, scalar_vignette_u16(list(I)))
    s = F(254.9 * 254.9)
    assert float(s) == float(F(64974.01)) and got[0] == 0 and got[2] == 64974 and got[7] == 65535 and got[9] == 65535 and got[10] == 0 and got[12] == 0
    for k, v in Q.vignette_ties().items():
        assert Q.vignette_u16(np.array([v]))[0] == (k if k % 2 == 0 else k + 1)  # ties to even


# ---- the RGB file ---------------------------------------------------------------------------------------------------------------


def rgb_images():
    rng = np.random.default_rng(6)
    yy, xx = np.mgrid[0:31, 0:97]
    smooth = np.stack([xx * 2 + yy, xx + yy * 3, (xx * yy) // 16], axis=2).astype(np.uint8)
    out = [("noise_%dx%d" % (w, h), rng.integers(0, 256, (h, w, 3)).astype(np.uint8)) for w, h in ((1, 1), (2, 3), (5, 4), (7, 1), (97, 31))]
    return out + [("smooth_97x31", smooth), ("black_5x5", np.zeros((5, 5, 3), np.uint8))]


@pytest.mark.parametrize("filt", [0, 1, 2, 3, 4, P.ADAPTIVE])
def test_rgb_files_inflate_decode_and_keep_the_bound(filt):
    from PIL import Image

    seen = set()
    for name, img in rgb_images():
        h, w, _ = img.shape
        png, stored = Q.encode_rgb(img, filt)
        data = Q.filtered_rgb(img, filt).tobytes()
        assert len(data) == h * (1 + 3 * w)
        assert zlib.decompress(P.idat_of(png)) == data, name
        im = Image.open(io.BytesIO(png))
        assert im.mode == "RGB" and im.size == (w, h) and np.array_equal(np.array(im), img), name
        assert ((png[43] >> 1) & 3) == (0 if stored else 2)
        if stored:
            assert len(png) == Q.png_bound_rgb8(w, h), name
        else:
            assert len(png) < Q.png_bound_rgb8(w, h), name
        seen.add(stored)
    assert seen == {True, False}  # the noise takes the stored form, the smooth image does not


# ---- libmdc_pngw_rgb.so: header, library, table ---------------------------------------------------------------------------------


def test_rgb_header_library_and_table_are_one_set(tmp_path):
    import ctypes
    import os
    import subprocess

    from mono_dataset_code_amd import build, capi
    from test_abi import declared, exported, prototypes, signature_mismatches

    names = declared("mdc_pngw_rgb.h", "mdcp_")
    assert len(names) == 6 and all("rgb8" in n for n in names)
    assert exported(build.LIB_PNGW_RGB) == names == sorted(capi.PNGW_RGB_API)
    protos = prototypes("mdc_pngw_rgb.h", "mdcp_")
    assert sorted(protos) == names and signature_mismatches(capi.PNGW_RGB_API, protos) == []
    L = capi.pngw_rgb_lib()
    assert sorted(vars(L)) == names
    # the gray library is what it was: none of these names, and neither library needs the other
    assert not set(names) & set(exported(build.LIB_PNGW))
    for lib in (build.LIB_PNGW, build.LIB_PNGW_RGB):
        needed = subprocess.run(["readelf", "-d", lib], stdout=subprocess.PIPE, text=True, check=True).stdout
        assert sorted({w.strip("[]") for line in needed.splitlines() if "NEEDED" in line for w in line.split() if "libmdc_" in w}) == ["libmdc_zipw.so"]
    src = tmp_path / "abi.c"
    src.write_text('#include "mdc_pngw_rgb.h"\nint main(void){ mdcp_encoder* e = 0; (void)e; return MDCP_OK + (mdcp_png_bound_rgb8(1, 1) < 0); }\n')
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    for cmd in (["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I" + inc, str(src)],
                ["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", "-I" + inc, str(src)]):
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
    # the bound and the argument checks, all before any HIP call
    for w, h in ((1, 1), (5, 4), (97, 31), (640, 480), (21845, 3)):
        assert L.mdcp_png_bound_rgb8(w, h) == Q.png_bound_rgb8(w, h)
    assert L.mdcp_png_bound_rgb8(0, 1) == -1 and L.mdcp_png_bound_rgb8(26755, 26755) == -1 and L.mdcp_png_bound_rgb8(2 ** 31 - 1, 1) == -1
    h_ = ctypes.c_void_p()
    err = lambda: L.mdcp_last_error_rgb8().decode()  # noqa: E731
    assert L.mdcp_create_rgb8(0, 4, 4, 0, 1, None) == -1 and "null" in err()
    assert L.mdcp_create_rgb8(0, 4, 4, 6, 1, ctypes.byref(h_)) == -1 and "filter" in err() and not h_.value
    assert L.mdcp_create_rgb8(0, 4, 4, 0, 0, ctypes.byref(h_)) == -1 and "max_images" in err()
    assert L.mdcp_create_rgb8(0, 0, 4, 0, 1, ctypes.byref(h_)) == -3 and L.mdcp_create_rgb8(0, 30000, 30000, 0, 1, ctypes.byref(h_)) == -3 and "2^31" in err()
    p = ctypes.c_void_p(4096)  # never dereferenced on the host
    assert L.mdcp_encode_rgb8_device(None, p, 48, 1, p, 1 << 20, p, None) == -1 and "null" in err()
    assert L.mdcp_output_device_rgb8(None, None, None, None) == -1
    L.mdcp_destroy_rgb8(None)
