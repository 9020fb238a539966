"""The result images of the two calibration tools restated with NumPy: plotE and plotG of src/main_responseCalib.cpp:72-146,
displayImage of src/main_vignetteCalib.cpp:72-94 and the 16-bit quantisation of its vignette files (:568-583) -- what
mdc_rcal_plot_e_device, mdc_rcal_plot_g_device, mdc_vcal_plot_plane_device and mdc_vcal_vignette_u16_device (include/mdc_hip.h)
compute -- and the 8-bit RGB PNG file of include/mdc_pngw_rgb.h, built on tests/pngw_restatement.py with bpp = 3 and colour type 2.
log and exp in double are this machine's libm, through math.log / math.exp.  The bit-for-bit oracle of tests/test_plots.py; itself
pinned by literal scalar transcriptions, zlib and PIL in tests/test_plots_cpu.py."""
import math
import struct
import zlib

import numpy as np

import pngw_restatement as P

INT_MIN = -(1 << 31)
F = np.float32


def x86_int(v):
    """(int)v as x86's cvttss2si / cvttsd2si leave it: truncation, INT_MIN for a NaN or a value outside int -> int64 array"""
    v = np.asarray(v)
    ok = (v > -2147483649.0) & (v < 2147483648.0) if v.dtype == np.float64 else (v > np.float32(-2147483648.0)) & (v < np.float32(2147483648.0))
    with np.errstate(invalid="ignore"):
        return np.where(ok, np.trunc(np.where(ok, v, 0)).astype(np.int64), INT_MIN)


def first_min_max(a):
    """min / max as the sequential loops leave them: from 1e10 / -1e10 (in a's type), replaced under a strict comparison only -- a NaN is
    never taken, of equal values (zeros of either sign) the first in index order stays"""
    a = np.asarray(a).reshape(-1)
    ty = a.dtype.type
    lo, hi = ty(1e10), ty(-1e10)
    if len(a):
        b = np.where(np.isnan(a), ty(np.inf), a)
        i = int(np.argmin(b))  # the first of the smallest
        if b[i] < lo:
            lo = a[i]
        b = np.where(np.isnan(a), ty(-np.inf), a)
        i = int(np.argmax(b))
        if b[i] > hi:
            hi = a[i]
    return lo, hi


def c_log(x):
    if x != x or x < 0:
        return math.nan
    if x == 0:
        return -math.inf
    return math.log(x)


def c_exp(x):
    if x != x:
        return math.nan
    try:
        return math.exp(x)
    except OverflowError:
        return math.inf


def plot_e(E):
    """-> (rgb (n, 3) uint8 in file order R, G, B, e16 (n,) uint16, (Emin, Emax))"""
    E = np.asarray(E, np.float64).reshape(-1)
    le = np.array([c_log(float(v) + 20.0) for v in E], np.float64)
    lmin, lmax = first_min_max(le)
    emin, emax = first_min_max(E)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ratio = (le - lmin) / (lmax - lmin)
        ex = np.array([c_exp(float(v)) for v in ratio], np.float64)
        val = (3 * (ex - 1) / 1.7183).astype(np.float32)
        icp = x86_int(val)
        ifp = val - icp.astype(np.float32)
        icp = np.fmod(icp, 3)  # C's %: the sign of the dividend
        c = (x86_int(np.float32(255) * ifp) & 255).astype(np.uint8)
        e16 = (x86_int(65025.0 * (E - emin) / (emax - emin)) & 0xFFFF).astype(np.uint16)
    # B, G, R = (0, 0, c) / (0, c, 255) / (c, 255, 255) for icP 0 / 1 / 2, zeros otherwise; here in file order
    r = np.where(icp == 0, c, np.where((icp == 1) | (icp == 2), 255, 0))
    g = np.where(icp == 1, c, np.where(icp == 2, 255, 0))
    b = np.where(icp == 2, c, 0)
    return np.stack([r, g, b], axis=1).astype(np.uint8), e16, (emin, emax)


def plot_g(G):
    """-> (GImg * 255 as (256, 256) float32, row k, column i; (min, max))"""
    G = np.asarray(G, np.float64).reshape(256)
    gmin, gmax = first_min_max(G)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        val = 256 * (G - gmin) / (gmax - gmin)
        k = np.arange(256, dtype=np.float64)[:, None]
        img = np.where(val[None, :] < k, (k - val[None, :]).astype(np.float32) * np.float32(255), np.float32(0))
    return img.astype(np.float32), (gmin, gmax)


def plot_plane(I):
    """-> (rgb (n, 3) uint8 in file order, (vmin, vmax) float32)"""
    I = np.asarray(I, np.float32).reshape(-1)
    vmin, vmax = first_min_max(I)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        c = (x86_int((np.float32(255) * (I - vmin)) / (vmax - vmin)) & 255).astype(np.uint8)
    rgb = np.repeat(c[:, None], 3, axis=1)
    rgb[np.isnan(I)] = (255, 0, 0)
    return rgb, (vmin, vmax)


def vignette_u16(I):
    """saturate_cast<ushort>(cvRound(I * s)), s = (float)(254.9 * 254.9): ties to even, clamped, NaN -> 0"""
    I = np.asarray(I, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        v = I * np.float32(254.9 * 254.9)
        r = np.clip(np.rint(v), 0, 65535)
    return np.where(np.isnan(v), 0, r).astype(np.uint16)


# ------------------------------------------------------------------------------------------------ the RGB file


def filtered_rgb(img, filt):
    """P.filtered with the filter distance of a pixel, bpp = 3: (h, 1 + 3 w) bytes"""
    img = np.asarray(img, np.uint8)
    h, w, _ = img.shape
    raw = img.reshape(h, 3 * w).astype(np.int32)
    a = np.zeros_like(raw)
    a[:, 3:] = raw[:, :-3]
    b = np.zeros_like(raw)
    b[1:] = raw[:-1]
    c = np.zeros_like(raw)
    c[1:, 3:] = raw[:-1, :-3]
    cand = np.stack([raw, raw - a, raw - b, raw - ((a + b) >> 1), raw - P.paeth(a, b, c)]) & 255
    if filt == P.ADAPTIVE:
        types = np.argmin(np.where(cand < 128, cand, 256 - cand).sum(axis=2), axis=0)
    else:
        assert 0 <= filt <= 4
        types = np.full(h, filt)
    out = np.empty((h, 1 + 3 * w), np.uint8)
    out[:, 0] = types
    out[:, 1:] = cand[types, np.arange(h)]
    return out


def encode_rgb(img, filt):
    """(h, w, 3) uint8 -> (the file, True if its image is stored): P.encode with IHDR colour type 2, depth 8"""
    img = np.asarray(img, np.uint8)
    h, w, ch = img.shape
    assert ch == 3
    data = filtered_rgb(img, filt).tobytes()
    stream, stored = P.deflate(data)
    idat = b"\x78\x01" + stream + struct.pack(">I", zlib.adler32(data))
    ihdr = struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)
    return P.SIGNATURE + P.chunk(b"IHDR", ihdr) + P.chunk(b"IDAT", idat) + P.chunk(b"IEND", b""), stored


def png_bound_rgb8(w, h):
    return 57 + 6 + P.stored_size(h * (1 + 3 * w))


# ------------------------------------------------------------------------------------------------ shared test inputs


def irradiance(n, seed, nans=3):
    rng = np.random.default_rng(seed)
    E = rng.uniform(0.0, 300.0, n)
    if n > nans:
        E[rng.choice(n, nans, replace=False)] = np.nan
    return E


def plot_e_inputs():
    zeros = np.array([3.0, -0.0, 0.0, 7.5, 0.0, -0.0])  # the minimum is the FIRST zero: -0
    zeros2 = zeros[[0, 2, 1, 3, 4, 5]]                   # ... +0
    return [("random_37", irradiance(37, 1)), ("one_pixel", np.array([12.5])), ("two_pixels", np.array([0.0, 255.0])),
            ("all_nan", np.full(9, np.nan)), ("constant", np.full(11, 42.0)), ("minus_zero_first", zeros), ("plus_zero_first", zeros2),
            ("nan_and_inf", np.array([1.0, np.inf, np.nan, 5.0])), ("random_300", irradiance(300, 2, 9))]


def plot_g_inputs():
    mono = np.cumsum(np.random.default_rng(3).uniform(0.1, 2.0, 256))
    holes = mono.copy()
    holes[[0, 1, 200]] = np.nan
    return [("monotone", mono), ("nan_0_1_200", holes), ("constant", np.full(256, 17.25)), ("all_nan", np.full(256, np.nan))]


def both_sides_of_255():
    """d with (255 * d) / d below 255 in float (the byte is 254) and one with it at or above (255)"""
    rng = np.random.default_rng(4)
    below = above = None
    for d in rng.uniform(0.5, 200.0, 4000).astype(np.float32):
        q = (F(255) * d) / d
        if q < F(255) and below is None:
            below = d
        if q >= F(255) and above is None:
            above = d
    assert below is not None and above is not None
    return below, above


def plane_inputs():
    below, above = both_sides_of_255()
    rng = np.random.default_rng(5)
    p = rng.uniform(-3.0, 90.0, 35).astype(np.float32)
    p[[4, 20]] = np.nan
    return [("random_7x5", p), ("one", np.array([2.5], np.float32)), ("all_nan", np.full(6, np.nan, np.float32)),
            ("constant", np.full(8, 3.0, np.float32)), ("max_gives_254", np.array([0, below / 3, below], np.float32)),
            ("max_gives_255", np.array([0, above / 3, above], np.float32)), ("zeros", np.array([5, -0.0, 0.0], np.float32))]


def vignette_ties():
    """floats I with I * s exactly at k + 0.5, for even and odd k"""
    s = F(254.9 * 254.9)
    found = {}
    for k in range(0, 400):
        I = F((k + 0.5) / float(s))
        for _ in range(8):
            I = np.nextafter(I, F(0))
        for _ in range(17):
            if I * s == F(k + 0.5):
                found.setdefault(k, I)
            I = np.nextafter(I, F(1))
    assert any(k % 2 == 0 for k in found) and any(k % 2 == 1 for k in found), found
    return found


def vignette_inputs():
    s = F(254.9 * 254.9)
    ties = vignette_ties()
    vals = [0.0, -0.0, 1.0, 0.5, 1e-6, F(65535.0) / s, np.nextafter(F(65535.0) / s, F(2)), 1.5, 100.0, np.inf, -0.3, -np.inf, np.nan]
    return np.array(vals + list(ties.values())[:24], np.float32)


def bits(a, ty=np.float64):
    return np.asarray(a, ty).view(np.uint64 if ty == np.float64 else np.uint32)
