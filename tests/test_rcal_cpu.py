"""responseCalib, CPU side: the NumPy restatement (tests/rcal_restatement.py) against a literal transcription of the reference's
loops, its quirks, the recovery of a known response, and the C entries without a GPU."""
import ctypes
import math

import numpy as np
import pytest

import rcal_restatement as R


def div(a, b):  # IEEE division as in C (x / 0 = +-inf, 0 / 0 = NaN)
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


# ---- literal transcription of src/main_responseCalib.cpp (loops as written, Python floats = doubles) -------------------------
def lit_leak(data, w, h, leak):
    data = list(data)
    for _ in range(leak):
        data2 = list(data)
        for y in range(1, h - 1):
            for x in range(1, w - 1):
                if data[x + y * w] == 255:
                    for dy in (-1, 0, 1):
                        for dx in (-1, 0, 1):
                            data2[x + dx + w * (y + dy)] = 255
        data = data2
    return data


def lit_rmse(G, E, t, data, wh):
    import decimal

    e = decimal.Decimal(0)  # wider than long double: the order of the sums does not matter at 1e-12
    num = 0
    for i in range(len(data)):
        for k in range(wh):
            if data[i][k] == 255:
                continue
            with np.errstate(all="ignore"):
                r = float(np.float64(G[data[i][k]]) - np.float64(t[i]) * np.float64(E[k]))
            if not math.isfinite(r):
                continue
            e += decimal.Decimal(r * r * 1e-10)
            num += 1
    if num == 0:
        return float("nan"), 0.0
    return 1e5 * math.sqrt(float(e / num)), float(num)


def lit_solve(data, t, wh, nits):
    n = len(data)
    E = [0.0] * wh
    En = [0.0] * wh
    for i in range(n):
        for k in range(wh):
            E[k] += data[i][k]
            En[k] += 1
    E = [div(E[k], En[k]) for k in range(wh)]
    G = [0.0] * 256
    out = []
    for _ in range(nits):
        GSum, GNum = [0.0] * 256, [0.0] * 256
        for i in range(n):
            for k in range(wh):
                b = data[i][k]
                if b == 255:
                    continue
                GNum[b] += 1
                GSum[b] += E[k] * t[i]
        for i in range(256):
            G[i] = div(GSum[i], GNum[i])
            if not math.isfinite(G[i]) and i > 1:
                G[i] = G[i - 1] + (G[i - 1] - G[i - 2])
        ESum, ENum = [0.0] * wh, [0.0] * wh
        for i in range(n):
            for k in range(wh):
                b = data[i][k]
                if b == 255:
                    continue
                ENum[k] += t[i] * t[i]
                ESum[k] += G[b] * t[i]
        for i in range(wh):
            E[i] = div(ESum[i], ENum[i])
            if E[i] < 0:
                E[i] = 0.0
        f = div(255.0, G[255])
        for i in range(wh):
            E[i] *= f
            if i < 256:
                G[i] *= f
        out.append((list(G), list(E), lit_rmse(G, E, t, data, wh)))
    return out


def bits(a):
    a = np.asarray(a, np.float64)
    b = a.copy()
    b[np.isnan(b)] = np.nan  # one NaN payload
    return b.view(np.uint64)


def tiny_stack(rng, n, w, h):
    s = rng.integers(0, 256, (n, h, w)).astype(np.uint8)
    s[rng.random((n, h, w)) < 0.15] = 255
    return s


@pytest.mark.parametrize("n,w,h,seed", [(4, 6, 5, 1), (3, 7, 3, 2), (5, 17, 16, 3)])
def test_restatement_equals_literal_loops(n, w, h, seed):
    rng = np.random.default_rng(seed)
    stack = tiny_stack(rng, n, w, h)
    t = rng.uniform(0.3, 9.0, n)
    padded = R.leak_pad(stack, w, h, 2)
    lit = [lit_leak(stack[i].reshape(-1).tolist(), w, h, 2) for i in range(n)]
    assert np.array_equal(padded.reshape(n, -1), np.array(lit, np.uint8))
    G, E, log = R.solve(padded, t, 3)
    ref = lit_solve(lit, t.tolist(), w * h, 3)
    for it, (g, e, rm) in enumerate(ref):
        assert np.array_equal(bits(log["G"][it]), bits(g)), it
        assert np.array_equal(bits(log["E"][it]), bits(e)), it
        got = log["iters"][it]
        assert got["num_resc"] == rm[1]
        assert got["rmse_resc"] == pytest.approx(rm[0], rel=1e-12, nan_ok=True)


def test_partial_rescale_when_fewer_pixels_than_bins():
    """w*h < 256: the rescale loop (:352-356) scales only G[0 .. w*h-1]."""
    G = np.arange(256, dtype=np.float64) + 1.0
    E = np.ones(5 * 4)
    G2, E2, f = R.rescale(G, E)
    assert f == 255.0 / 256.0
    assert np.array_equal(G2[:20], G[:20] * f) and np.array_equal(G2[20:], G[20:])
    assert np.array_equal(E2, E * f)


def test_pixels_saturated_everywhere_and_empty_bins():
    rng = np.random.default_rng(7)
    n, w, h = 4, 9, 7
    stack = rng.integers(0, 180, (n, h, w)).astype(np.uint8)
    stack[:, 2, 3] = 255  # every image: E stays NaN after the E step
    t = rng.uniform(1, 3, n)
    G, E, log = R.solve(stack, t, 2)
    assert np.isnan(E[2 * w + 3]) and np.isfinite(np.delete(E, 2 * w + 3)).all()
    # bins 180..255 are empty: extrapolated linearly from the last two (:301-302)
    G1 = R.g_step(R.init_e(stack), t, stack)
    assert np.all(np.isfinite(G1[2:]))
    assert G1[200] - G1[199] == G1[199] - G1[198]


def test_leak_padding_borders():
    """Border pixels are never seeds but can be set (:214-215)."""
    w, h = 6, 5
    img = np.zeros((1, h, w), np.uint8)
    img[0, 0, 0] = 255       # corner: no seed
    img[0, 4, 3] = 255       # bottom row: no seed
    img[0, 1, 4] = 255       # interior, next to the right border: sets column 5
    out = R.leak_pad(img, w, h, 1)[0]
    assert out[0, 0] == 255 and out[1, 1] == 0
    assert out[3, 3] == 0
    assert out[0, 5] == 255 and out[2, 5] == 255 and out[0, 3] == 255 and out[2, 3] == 255
    assert np.array_equal(out.reshape(-1), np.array(lit_leak(img.reshape(-1).tolist(), w, h, 1), np.uint8))


def test_recovers_a_known_response():
    """A noise-free sweep through f(x) = 255 (x / 400)^(1/2.2): after 10 iterations G / 255 follows f^-1 up to scale.  Measured:
    the largest deviation over the bins 20..250 is 0.011 of full scale (quantisation to bytes and the unknown scale); the bound
    is 0.02."""
    rng = np.random.default_rng(11)
    stack, t, _ = R.synthetic_sweep(rng, 24, 64, 48)
    stack = R.leak_pad(stack, 64, 48, 2)
    G, E, _ = R.solve(stack, t, 10)
    b = np.arange(20, 251)
    want = (b / 255.0) ** 2.2
    got = G[b] / G[255]
    scale = np.dot(got, want) / np.dot(got, got)
    assert np.max(np.abs(got * scale - want)) < 0.02
    assert np.all(np.diff(G[b]) > 0)


def test_pcalib_text_format():
    assert R.pcalib_text(np.array([0.0, 1.0 / 3.0, 255.0, np.nan])) == "0 0.333333333333333 255 nan \n"


def test_c_entries_without_gpu():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from mono_dataset_code_amd import capi

    L = capi.hip_lib()
    buf = ctypes.c_void_p(1)
    assert L.mdc_rcal_leak_pad_device(None, buf, 1, 4, 4, 2, None) == capi.ERR_NO_DEVICE
    assert L.mdc_rcal_init_e_device(None, buf, 1, 4, 4, buf, None) == capi.ERR_NO_DEVICE
    assert L.mdc_rcal_rmse_device(None, buf, buf, 1, 4, 4, buf, buf, buf, None) == capi.ERR_NO_DEVICE
    assert L.mdc_rcal_g_step_device(None, buf, buf, 1, 4, 4, buf, buf, None) == capi.ERR_NO_DEVICE
    out = ctypes.c_void_p()
    assert L.mdc_rcal_index_create(None, buf, 1, 4, 4, None, ctypes.byref(out)) == capi.ERR_NO_DEVICE
    assert L.mdc_rcal_g_step_indexed_device(None, buf, buf, buf, buf, None) == capi.ERR_NO_DEVICE
    assert L.mdc_rcal_e_step_device(None, buf, buf, 1, 4, 4, buf, buf, None, None) == capi.ERR_NO_DEVICE
    assert L.mdc_rcal_rescale_device(None, buf, buf, 1, 4, 4, buf, buf, None, None, None) == capi.ERR_NO_DEVICE
    assert L.mdc_rcal_solve_device(None, buf, buf, 1, 4, 4, 1, capi.RCAL_EXACT_ORDER, buf, buf, None, None) == capi.ERR_NO_DEVICE
    assert L.mdc_copy_to_device(None, buf, buf, 0) == capi.ERR_NO_DEVICE
    assert L.mdc_rcal_index_entries(None) == 0 and L.mdc_rcal_index_longest_chain(None) == 0


def test_program_is_built():
    import os

    from mono_dataset_code_amd import build

    assert os.access(build.RESPONSE_CALIB, os.X_OK)


# ---- the large-stack forms of the restatement (tests/test_rcal_sizes.py) against the plain ones ----------------------------
def sparse_stack(rng, n, w, h, listed):
    """a stack that is 255 except at `listed` random positions -> (stack, positions in a shuffled order, their bytes)"""
    pos = rng.choice(n * w * h, listed, replace=False)
    vals = rng.integers(0, 255, listed).astype(np.uint8)
    stack = np.full(n * w * h, 255, np.uint8)
    stack[pos] = vals
    return stack.reshape(n, h, w), pos, vals


def wide_range(rng, size, lo=-8.0, hi=8.0):
    return 10.0 ** rng.uniform(lo, hi, size)


@pytest.mark.parametrize("n,w,h,listed,seed", [(5, 9, 7, 200, 1), (3, 31, 17, 900, 2), (12, 16, 16, 40, 3), (1, 300, 1, 299, 4)])
def test_sparse_forms_equal_the_plain_ones(n, w, h, listed, seed):
    rng = np.random.default_rng(seed)
    stack, pos, vals = sparse_stack(rng, n, w, h, listed)
    t = wide_range(rng, n, -3, 3)
    E = wide_range(rng, w * h)
    E[rng.random(w * h) < 0.05] = np.nan
    assert np.array_equal(bits(R.init_e_sparse(pos, vals, n, w * h)), bits(R.init_e(stack)))
    G = R.g_step(E, t, stack)
    assert np.array_equal(bits(R.g_step_sparse(pos, vals, E, t, w * h)), bits(G))
    G[rng.random(256) < 0.1] = np.nan
    assert np.array_equal(bits(R.e_step_sparse(pos, vals, G, t, w * h)), bits(R.e_step(G, t, stack)))
    E2 = R.e_step(G, t, stack)
    for g, e in ((G, E), (G, E2)):
        got, want = R.rmse_sparse(pos, vals, g, e, t, w * h), R.rmse(g, e, t, stack)
        assert got[1] == want[1] and bits([got[0]]) == bits([want[0]])


@pytest.mark.parametrize("n,w,h,seed", [(4, 6, 5, 1), (9, 33, 17, 2), (2, 256, 3, 3)])
def test_g_step_by_image_equals_g_step(n, w, h, seed):
    rng = np.random.default_rng(seed)
    stack = tiny_stack(rng, n, w, h)
    t = wide_range(rng, n, -3, 3)
    E = wide_range(rng, w * h)
    E[0] = np.nan
    assert np.array_equal(bits(R.g_step_by_image(E, t, stack)), bits(R.g_step(E, t, stack)))
    _, _, a = R.solve(stack, t, 2)
    _, _, b = R.solve(stack, t, 2, g=R.g_step_by_image)
    for it in range(2):
        assert np.array_equal(bits(a["G"][it]), bits(b["G"][it])) and np.array_equal(bits(a["E"][it]), bits(b["E"][it]))
        assert a["iters"][it] == b["iters"][it]


def test_sparse_g_step_sees_the_order():
    """The forms above would not notice a reordered sum if every order gave the same bits: on these products it does not."""
    rng = np.random.default_rng(5)
    prod = wide_range(rng, 1537)
    seq = np.cumsum(np.concatenate([[0.0], prod]))[-1]
    assert seq != np.cumsum(prod[::-1])[-1] and seq != np.sum(prod) and seq != math.fsum(prod)
