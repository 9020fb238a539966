"""responseCalib's kernels (mono_dataset_code_amd/csrc/mdc_rcal.hip) at, below and past every size-dependent limit, against the
test-owned restatement (tests/rcal_restatement.py):

  kRcalChunk = 65536        samples per counting-sort chunk (hist, scatter; the scatter's last wave may be partial)
  scan passes of 1024       chunks per pass of rcal_hist_scan_kernel, carried in s_carry
  kRcalWalkChunk = 1536     products per LDS buffer of the exact-order walk (double buffer, partial last buffer)
  kRcalLeakImages = 64      images per ping-pong chunk of the leak padding (odd leak ends in a copy back)
  256 workgroup partials    per thread of rcal_rmse_final_kernel / rcal_bins_final_kernel
  RcalIndex::wide           8-byte positions from n*w*h >= 2^32 on
  pass_width                one pixel per lane when w*h % 4 != 0 or the stack does not start on 4 bytes

Bit-identical: leak padding, initial E, E step, the indexed G step, the rescale.  rmse: exact counts, values to 1e-9 relative
(double-double partials against one long double chain).  Direct G: the error bound its arithmetic gives (direct_bound)."""
import math
from fractions import Fraction

import numpy as np
import pytest

import rcal_restatement as R

pytestmark = pytest.mark.gpu

CHUNK = 65536
WALK = 1536
LEAK_IMAGES = 64
U = 2.0 ** -53  # unit roundoff of a double


def bits(a):
    a = np.array(a, np.float64)
    a[np.isnan(a)] = np.nan  # any NaN payload
    return a.view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def ctx():
    from mono_dataset_code_amd import capi

    return capi.Context(0)


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def wide_range(rng, size, lo=-8.0, hi=8.0):
    """values spread over 10^lo .. 10^hi: the order of a sum of their products shows in its bits"""
    return 10.0 ** rng.uniform(lo, hi, size)


def random_stack(rng, n, w, h, p255=0.1):
    s = rng.integers(0, 255, (n, h, w)).astype(np.uint8)
    s[rng.random((n, h, w)) < p255] = 255
    return s


def assert_rmse(got, want):
    assert got[1] == want[1], (got, want)
    if want[1] == 0:
        assert math.isnan(got[0]), got  # 0 / 0
    else:
        assert got[0] == pytest.approx(want[0], rel=1e-9), (got, want)


# ---- the direct G step's error bound ---------------------------------------------------------------------------------------
def direct_scale(E, t, N):
    """rcal_scale_kernel: m = max finite |E| * max finite |t| < 2^em, N < 2^en -> scale = 125 - em - en (0 when m is 0)."""
    e = np.abs(E[np.isfinite(E)])
    tt = np.abs(t[np.isfinite(t)])
    m = float(e.max() if e.size else 0.0) * float(tt.max() if tt.size else 0.0)
    if not (m > 0 and math.isfinite(m)):
        return 0
    return 125 - math.frexp(m)[1] - int(N).bit_length()


def direct_bound(E, t, stack, Gd, rel=None):
    """Per bin b with GNum = c > 0 samples and finite products: what rcal_pass_kernel<kGDirect> + rcal_bins_final_kernel +
    rcal_g_finalize_kernel can be off by.  Each product x is added as trunc(|x| 2^s) with x's sign (an error below one unit
    2^-s, toward zero); the 128-bit integer sums are exact; the conversion back rounds hi, lo and their sum (3 roundings, at
    most (2u + u^2) of the sum) and G = GSum / c rounds once more.  With S = fsum of the bin's products (correctly rounded):
        |G - S / c|  <=  2^-s  +  (4 + 2^-20) u (|S| / c + 2^-s),        u = 2^-53.
    Asserted exactly (rationals); with rel, also |G - S / c| <= rel |S / c|.  Returns the bins where that relative bound fails."""
    n = stack.shape[0]
    d = stack.reshape(n, -1)
    s = direct_scale(E, t, d.size)
    unit = Fraction(2) ** -s
    b = d.reshape(-1)
    keep = b != 255
    with np.errstate(all="ignore"):
        prod = (E[None, :] * t[:, None]).reshape(-1)[keep]
    b = b[keep]
    order = np.argsort(b, kind="stable")
    b, prod = b[order], prod[order]
    cut = np.searchsorted(b, np.arange(257))
    slack = (4 + Fraction(2) ** -20) * Fraction(U)
    rel_fail = []
    for v in range(255):
        p = prod[cut[v]:cut[v + 1]]
        c = len(p)
        if c == 0 or not np.all(np.isfinite(p)):
            continue
        S = Fraction(math.fsum(p.tolist()))
        mean = S / c
        err = abs(Fraction(float(Gd[v])) - mean)
        assert err <= unit + slack * (abs(mean) + unit), (v, c, float(Gd[v]), float(mean), s)
        if rel is not None and err > Fraction(rel) * abs(mean):
            rel_fail.append(v)
    return rel_fail


def check_direct(ctx, d_stack, d_t, E, stack, t, G_ref, rel=1e-9):
    """direct G: deterministic, non-finite where the reference is, within direct_bound and (realistic data) rel per bin"""
    Gs = []
    for _ in range(2):
        d_G = dev(np.full(256, -1.0))
        ctx.rcal_g_step(d_stack, d_t, dev(E), d_G)
        Gs.append(d_G.cpu().numpy())
    assert same_bits(Gs[0], Gs[1])
    Gd = Gs[0]
    assert np.array_equal(np.isfinite(Gd), np.isfinite(G_ref))
    fails = direct_bound(E, t, stack, Gd, rel)
    if rel is not None:
        assert not fails, fails
    return Gd


# ---- every step on one device stack -----------------------------------------------------------------------------------------
def check_steps(ctx, d_stack, stack, t, leak=2):
    """leak padding (in place on d_stack), initial E, rmse, index, indexed G, direct G, E step, rescale -- each against the
    restatement -> the device results."""
    n, h, w = stack.shape
    d_t = dev(t)
    out = {}
    ctx.rcal_leak_pad(d_stack, leak)
    padded = R.leak_pad(stack, w, h, leak)
    assert np.array_equal(d_stack.cpu().numpy(), padded)
    E0 = R.init_e(padded)
    d_E = ctx.rcal_init_e(d_stack)
    out["E0"] = d_E.cpu().numpy()
    assert same_bits(out["E0"], E0)
    G0 = np.zeros(256)
    out["rmse0"] = ctx.rcal_rmse(d_stack, d_t, dev(G0), d_E)
    assert_rmse(out["rmse0"], R.rmse(G0, E0, t, padded))

    G1 = R.g_step(E0, t, padded)
    index = ctx.rcal_index(d_stack)
    listed = padded[padded != 255]
    assert index.entries == listed.size
    assert index.longest_chain == (int(np.bincount(listed, minlength=256).max()) if listed.size else 0)
    assert index.bytes == 4 * listed.size
    d_G = dev(np.full(256, -1.0))
    ctx.rcal_g_step_indexed(index, d_t, d_E, d_G)
    index.close()
    out["G1"] = d_G.cpu().numpy()
    assert same_bits(out["G1"], G1)
    out["Gd"] = check_direct(ctx, d_stack, d_t, E0, padded, t, G1)

    E1 = R.e_step(G1, t, padded)
    out["rmse_g"] = ctx.rcal_e_step(d_stack, d_t, d_G, d_E)
    assert_rmse(out["rmse_g"], R.rmse(G1, E0, t, padded))
    out["E1"] = d_E.cpu().numpy()
    assert same_bits(out["E1"], E1)

    G2, E2, _ = R.rescale(G1, E1)
    out["rmse_e"], out["rmse_resc"] = ctx.rcal_rescale(d_stack, d_t, d_G, d_E)
    out["G2"], out["E2"] = d_G.cpu().numpy(), d_E.cpu().numpy()
    assert same_bits(out["G2"], G2)
    assert same_bits(out["E2"], E2)
    assert_rmse(out["rmse_e"], R.rmse(G1, E1, t, padded))
    assert_rmse(out["rmse_resc"], R.rmse(G2, E2, t, padded))
    return out


# ---- counting-sort chunks and the scatter's partial last wave ---------------------------------------------------------------
# N = n*w*h: one below, on and one past one chunk, and 3 chunks -1 / 0 / +1 (65535, 196607 and 196609 are not multiples of 64)
CHUNK_SHAPES = [(3, 85, 257), (16, 64, 64), (1, 65537, 1), (1, 467, 421), (3, 256, 256), (7, 28087, 1)]


@pytest.mark.parametrize("n,w,h", CHUNK_SHAPES, ids=lambda v: str(v))
def test_sort_chunks_and_scatter_tail(ctx, n, w, h):
    N = n * w * h
    assert N in (CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK - 1, 3 * CHUNK, 3 * CHUNK + 1)
    rng = np.random.default_rng(N)
    stack = random_stack(rng, n, w, h)
    ends = [p for p in (0, CHUNK - 1, CHUNK, N - 1) if p < N]
    stack.reshape(-1)[ends] = 3  # both ends of the first chunk, the first of the second, the last sample: listed
    t = wide_range(rng, n, -2, 2)
    E = wide_range(rng, w * h)
    d_stack, d_t = dev(stack), dev(t)
    index = ctx.rcal_index(d_stack)
    listed = stack[stack != 255]
    assert index.entries == listed.size
    assert index.longest_chain == int(np.bincount(listed, minlength=256).max())
    for e in (E, R.init_e(stack)):
        d_G = dev(np.full(256, -1.0))
        ctx.rcal_g_step_indexed(index, d_t, dev(e), d_G)
        assert same_bits(d_G.cpu().numpy(), R.g_step(e, t, stack))
    index.close()


# ---- the scan's carry over passes of 1024 chunks: a real-size sweep ---------------------------------------------------------
def test_scan_carry_real_frame_solve(ctx):
    """1280x1024, n = 52: 68,157,440 samples = 1040 chunks (two scan passes), 1280 pass workgroups.  Leak padding, then a
    2-iteration exact-order solve; G, E, the counts and rescale factors bit for bit, the rmse values to 1e-9."""
    from mono_dataset_code_amd import capi

    n, w, h = 52, 1280, 1024
    assert -(-n * w * h // CHUNK) == 1040
    rng = np.random.default_rng(52)
    stack, t, _ = R.synthetic_sweep(rng, n, w, h, t_lo=0.05, t_hi=40.0, noise=1.5)
    stack[:, 100, 200:260] = 255  # saturated everywhere: E is NaN there
    d_stack, d_t = dev(stack), dev(t)
    ctx.rcal_leak_pad(d_stack, 2)
    padded = R.leak_pad(stack, w, h, 2)
    assert np.array_equal(d_stack.cpu().numpy(), padded)
    del stack
    index = ctx.rcal_index(d_stack)
    listed = np.bincount(padded.reshape(-1), minlength=256)[:255]
    assert index.entries == int(listed.sum()) and index.longest_chain == int(listed.max())
    index.close()
    G, E, log = ctx.rcal_solve(d_stack, d_t, 2, capi.RCAL_EXACT_ORDER)
    Gr, Er, ref = R.solve(padded, t, 2, g=R.g_step_by_image)
    assert same_bits(G.cpu().numpy(), Gr)
    assert same_bits(E.cpu().numpy(), Er)
    assert log["init_num"] == ref["init"][1] and log["init_rmse"] == pytest.approx(ref["init"][0], rel=1e-9)
    for k in range(2):
        for key in ("num_G", "num_E", "num_resc"):
            assert log["iters"][k][key] == ref["iters"][k][key], (k, key)
        for key in ("rmse_G", "rmse_E", "rmse_resc"):
            assert log["iters"][k][key] == pytest.approx(ref["iters"][k][key], rel=1e-9), (k, key)
        assert same_bits([log["iters"][k]["rescale"]], [ref["iters"][k]["rescale"]])


# ---- sparse stacks generated on the device: more than 2048 chunks, and the wide index ----------------------------------------
def check_sparse(ctx, flat, n, w, h, seed, special):
    """A stack that is 255 everywhere (never listed) but at a few thousand positions -- random ones, `special` ones and both
    ends -- built in the device buffer `flat` and restored to 255 afterwards.  Index size, initial E, indexed G step, E step and
    rmse against the sparse restatement."""
    import torch

    wh, N = w * h, n * w * h
    rng = np.random.default_rng(seed)
    special = np.array([p for p in special if 0 <= p < N], np.int64)
    pos = np.unique(np.concatenate([rng.integers(0, N, 4000), special, [0, N - 1]]))
    vals = np.where(rng.random(pos.size) < 0.5, rng.integers(0, 6, pos.size), rng.integers(0, 255, pos.size)).astype(np.uint8)
    d_pos = torch.from_numpy(pos).cuda()
    view = flat[:N]
    view[d_pos] = torch.from_numpy(vals).cuda()
    try:
        d_stack = view.view(n, h, w)
        t = wide_range(rng, n, -2, 2)
        d_t = dev(t)
        assert same_bits(ctx.rcal_init_e(d_stack).cpu().numpy(), R.init_e_sparse(pos, vals, n, wh))
        index = ctx.rcal_index(d_stack)
        assert index.entries == pos.size
        assert index.longest_chain == int(np.bincount(vals, minlength=256).max())
        assert index.bytes == pos.size * (8 if N >= 2 ** 32 else 4)
        E = wide_range(rng, wh)
        G1 = R.g_step_sparse(pos, vals, E, t, wh)
        d_G, d_E = dev(np.full(256, -1.0)), dev(E)
        ctx.rcal_g_step_indexed(index, d_t, d_E, d_G)
        index.close()
        assert same_bits(d_G.cpu().numpy(), G1)
        rg = ctx.rcal_e_step(d_stack, d_t, d_G, d_E)
        assert rg[1] == pos.size
        assert_rmse(rg, R.rmse_sparse(pos, vals, G1, E, t, wh))
        E1 = R.e_step_sparse(pos, vals, G1, t, wh)
        assert same_bits(d_E.cpu().numpy(), E1)
        assert_rmse(ctx.rcal_rmse(d_stack, d_t, d_G, d_E), R.rmse_sparse(pos, vals, G1, E1, t, wh))
    finally:
        view[d_pos] = 255
        torch.cuda.synchronize()


def edges(*points):
    return [p + d for p in points for d in (-1, 0, 1)]


def test_scan_carry_past_2048_chunks(ctx):
    """256x256, n = 2100: 2100 chunks, three scan passes; listed samples on both sides of every pass edge"""
    import torch

    n, w, h = 2100, 256, 256
    N = n * w * h
    flat = torch.full((N,), 255, dtype=torch.uint8, device="cuda")
    check_sparse(ctx, flat, n, w, h, 2100, edges(*(c * CHUNK for c in (1, 1023, 1024, 1025, 2047, 2048, 2049, N // CHUNK))))
    del flat
    torch.cuda.empty_cache()


# ---- the exact-order walk's LDS buffers --------------------------------------------------------------------------------------
WALK_COUNTS = {10: 0, 11: 1, 12: WALK - 1, 13: WALK, 14: WALK + 1, 20: 2 * WALK, 21: 2 * WALK + 1}


def test_walk_buffers(ctx):
    """Bins of exactly 0, 1, 1535, 1536, 1537, 3072 and 3073 samples, products over 22 decades: each chain's bits depend on its
    order (shown below for every bin that has one), so a walk that reorders a buffer or drops or repeats a product fails."""
    rng = np.random.default_rng(1536)
    n, w, h = 4, 97, 61
    wh, N = w * h, n * w * h
    flat = np.full(N, 255, np.uint8)
    perm = rng.permutation(N)
    o = 0
    for b, c in WALK_COUNTS.items():
        flat[perm[o:o + c]] = b
        o += c
    flat[perm[o:o + 5000]] = rng.integers(100, 200, 5000)  # other bins, shorter chains
    stack = flat.reshape(n, h, w)
    t = wide_range(rng, n, -3, 3)
    E = wide_range(rng, wh)
    for b, c in WALK_COUNTS.items():
        q = np.flatnonzero(flat == b)  # position order = the reference's
        assert q.size == c
        if c < 2:
            continue
        p = E[q % wh] * t[q // wh]
        seq = np.cumsum(np.concatenate([[0.0], p]))[-1]
        back = np.concatenate([p[j:j + WALK][::-1] for j in range(0, c, WALK)])  # every buffer back to front
        assert seq != np.cumsum(p[::-1])[-1] and seq != np.sum(p) and seq != np.cumsum(back)[-1], b
    G = R.g_step(E, t, stack)
    d_stack, d_t = dev(stack), dev(t)
    index = ctx.rcal_index(d_stack)
    assert index.entries == int((flat != 255).sum()) and index.longest_chain == 2 * WALK + 1
    d_G = dev(np.full(256, -1.0))
    ctx.rcal_g_step_indexed(index, d_t, dev(E), d_G)
    index.close()
    got = d_G.cpu().numpy()
    assert same_bits(got, G)


# ---- leak padding's chunks of 64 images ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [LEAK_IMAGES - 1, LEAK_IMAGES, LEAK_IMAGES + 1, 2 * LEAK_IMAGES + 1])
def test_leak_chunks(ctx, n):
    import torch

    w, h = 23, 17
    N = n * w * h
    rng = np.random.default_rng(n)
    stack = random_stack(rng, n, w, h, p255=0.04)
    for leak in range(4):
        flat = torch.full((N + 4096,), 7, dtype=torch.uint8, device="cuda")  # 4 KB guard after the stack
        d_stack = flat[:N].view(n, h, w)
        d_stack.copy_(dev(stack))
        ctx.rcal_leak_pad(d_stack, leak)
        assert np.array_equal(d_stack.cpu().numpy(), R.leak_pad(stack, w, h, leak)), leak
        assert bool((flat[N:] == 7).all()), leak


# ---- more than 256 workgroup partials per finalising thread --------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(640, 480), (641, 481)])
def test_many_workgroup_partials(ctx, w, h):
    """640x480: 300 workgroups at 4 pixels per lane; 641x481: 1205 at 1 -- rmse, E step, rescale and the direct G step finalise
    over all of them"""
    n = 5
    rng = np.random.default_rng(w)
    stack, t, _ = R.synthetic_sweep(rng, n, w, h, t_lo=0.3, t_hi=30.0, noise=1.0)
    stack[:, 7, 9] = 255
    check_steps(ctx, dev(stack), stack, t)


# ---- a stack that does not start on 4 bytes ----------------------------------------------------------------------------------
@pytest.mark.parametrize("off", [1, 2, 3])
def test_misaligned_base(ctx, off):
    """w*h % 4 == 0 but the base is off by 1..3: one pixel per lane.  Every step equals the restatement, and the aligned copy's
    results bit for bit (the direct G sums are integers, so its workgroup split does not matter); the bytes around the view stay."""
    import torch

    n, w, h = 7, 64, 48
    N = n * w * h
    rng = np.random.default_rng(40 + off)
    stack, t, _ = R.synthetic_sweep(rng, n, w, h, t_lo=0.4, t_hi=40.0, noise=1.5)
    stack[:, 1, 2] = 255
    aligned = check_steps(ctx, dev(stack), stack, t)
    flat = torch.full((off + N + 64,), 7, dtype=torch.uint8, device="cuda")
    d_stack = flat[off:off + N].view(n, h, w)
    assert d_stack.data_ptr() % 4 == off
    d_stack.copy_(dev(stack))
    got = check_steps(ctx, d_stack, stack, t)
    for key in ("E0", "G1", "Gd", "E1", "G2", "E2"):
        assert same_bits(got[key], aligned[key]), key
    for key in ("rmse0", "rmse_g", "rmse_e", "rmse_resc"):
        assert got[key][1] == aligned[key][1], key
    assert bool((flat[:off] == 7).all()) and bool((flat[off + N:] == 7).all())


# ---- degenerate frames ---------------------------------------------------------------------------------------------------------
# w or h of 1 or 2, w*h = 1, w*h = 255 / 256 / 257 (the rescale of G is partial below 256 pixels), n = 1
DEGENERATE = [(9, 1, 1), (5, 1, 13), (5, 13, 1), (7, 2, 2), (4, 2, 11), (4, 11, 2), (3, 15, 17), (3, 16, 16), (3, 257, 1), (1, 64, 48),
              (1, 1, 1)]


@pytest.mark.parametrize("n,w,h", DEGENERATE, ids=lambda v: str(v))
def test_degenerate_frames(ctx, n, w, h):
    rng = np.random.default_rng(1000 * n + 10 * w + h)
    stack = random_stack(rng, n, w, h)
    N = n * w * h
    if N == 1:
        stack[:] = 77  # every bin but 77 empty: G, E and the rmse are NaN from the first G step on
    else:  # bins 0 and 1 populated: the empty ones extrapolate to finite values, so G[255] and the rescale are finite
        q = rng.permutation(N)[:max(2, N // 8)]
        stack.reshape(-1)[q] = np.arange(q.size) % 2
    t = rng.uniform(0.2, 8.0, n)
    check_steps(ctx, dev(stack), stack, t)


# ---- the direct G step's bound -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,w,h,seed", [(7, 33, 17, 1), (13, 64, 48, 2), (40, 160, 120, 3)])
def test_direct_g_bound_on_sweeps(ctx, n, w, h, seed):
    """realistic sweeps: per bin within the absolute bound and 1e-9 relative of that bin's own exact mean"""
    rng = np.random.default_rng(seed)
    stack, t, _ = R.synthetic_sweep(rng, n, w, h, t_lo=1e-3, t_hi=40.0, noise=1.5)
    padded = R.leak_pad(stack, w, h, 2)
    d_stack, d_t = dev(padded), dev(t)
    E = R.init_e(padded)
    for _ in range(2):  # the initial E, then the E of one iteration
        check_direct(ctx, d_stack, d_t, E, padded, t, R.g_step(E, t, padded))
        E = R.e_step(R.g_step(E, t, padded), t, padded)


def test_direct_g_bound_wide_dynamic_range(ctx):
    """E over 40 decades: the scale follows max|E| max|t|, so the bins made only of small products lose all of their digits --
    the per-bin relative claim does not hold there, the absolute bound does."""
    n, w, h = 6, 48, 40
    rng = np.random.default_rng(77)
    stack = rng.integers(0, 100, (n, h, w)).astype(np.uint8)
    big = rng.random((h, w)) < 0.5
    stack[:, big] += 100  # bins 100..199: pixels of E ~ 1e20; bins 0..99: E ~ 1e-20
    stack[rng.random((n, h, w)) < 0.05] = 255
    E = np.where(big, wide_range(rng, (h, w), 19, 21), wide_range(rng, (h, w), -21, -19)).reshape(-1)
    t = rng.uniform(0.5, 5.0, n)
    G = R.g_step(E, t, stack)
    Gd = check_direct(ctx, dev(stack), dev(t), E, stack, t, G, rel=None)
    fails = direct_bound(E, t, stack, Gd, rel=1e-9)
    assert fails and all(v < 100 for v in fails), fails


# ---- the wide index (8-byte positions) and the largest narrow one ------------------------------------------------------------
WIDE = [(255, 65537, 257),   # 2^32 - 1: narrow, the last position is 2^32 - 2; w*h odd -> one pixel per lane, 65,793 workgroups
        (256, 4096, 4096),   # 2^32: the first wide stack
        (3277, 1280, 1024)]  # 2^32 + 262,144, w*h not a power of two


@pytest.fixture(scope="module")
def wide_buffer():
    import torch

    N = max(n * w * h for n, w, h in WIDE)
    flat = torch.full((N,), 255, dtype=torch.uint8, device="cuda")
    yield flat
    del flat
    torch.cuda.empty_cache()


@pytest.mark.parametrize("n,w,h", WIDE, ids=lambda v: str(v))
def test_wide_index(ctx, wide_buffer, n, w, h):
    N = n * w * h
    assert (N >= 2 ** 32) == (N != 2 ** 32 - 1)
    check_sparse(ctx, wide_buffer, n, w, h, n, edges(2 ** 31, 2 ** 32, N - 1, (N // CHUNK) * CHUNK))
