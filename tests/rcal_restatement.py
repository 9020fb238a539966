"""Test-owned NumPy restatement of the reference's responseCalib (src/main_responseCalib.cpp:189-380), in the reference's order of
operations: the pin of tests/test_rcal*.py.

  G step (:285-304): np.bincount with weights adds sequentially in input order -- the i-major flattened stack, products E[k]*t_i
                     formed in float64 first, exactly the reference's GSum chain;
  E step (:319-339): an explicit loop over the images, per pixel ENum += t*t, ESum += G[b]*t where b != 255;
  rmse   (:50-69)  : terms r*r*1e-10 in float64, summed sequentially (cumsum) in np.longdouble.

Forms for stacks too large for one pass over the host (same order, same bits; tests/test_rcal_cpu.py pins them to the above):
  g_step_by_image: the G step accumulated image by image with np.add.at (unbuffered, in index order);
  *_sparse       : a stack that is 255 everywhere except at the listed positions i*w*h + k -- 255 is never a term, so the G step,
                   the E step, the rmse and the initial E need only the listed samples."""
import numpy as np


def leak_pad(stack, w, h, leak):
    """:208-233, per image `leak` passes: every interior 255 sets its 3 x 3 neighbourhood."""
    out = stack.reshape(-1, h, w).copy()
    for _ in range(leak):
        src = out.copy()
        seed = np.zeros_like(src, dtype=bool)
        seed[:, 1:h - 1, 1:w - 1] = src[:, 1:h - 1, 1:w - 1] == 255
        grow = np.zeros_like(seed)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                # a pixel (y, x) is set when the seed (y - dy, x - dx) is
                ys, yd = (slice(0, h - dy), slice(dy, h)) if dy >= 0 else (slice(-dy, h), slice(0, h + dy))
                xs, xd = (slice(0, w - dx), slice(dx, w)) if dx >= 0 else (slice(-dx, w), slice(0, w + dx))
                grow[:, yd, xd] |= seed[:, ys, xs]
        out = np.where(grow, np.uint8(255), src)
    return out.reshape(stack.shape)


def init_e(stack):
    """:250-258: mean over all images, 255 included."""
    n = stack.shape[0]
    return stack.reshape(n, -1).astype(np.float64).sum(axis=0) / float(n)  # integer sums: exact


def rmse(G, E, t, stack):
    """:50-69 -> (1e5 * sqrt(e / num), num)."""
    n = stack.shape[0]
    d = stack.reshape(n, -1)
    terms = []
    for i in range(n):
        b = d[i]
        m = b != 255
        with np.errstate(all="ignore"):
            r = G[b[m]] - t[i] * E[m]
        r = r[np.isfinite(r)]
        with np.errstate(all="ignore"):
            terms.append(r * r * 1e-10)
    return _rmse_of_terms(terms)


def _rmse_of_terms(terms):
    """terms in the reference's order, as a list of arrays: one sequential long double chain (carried from array to array)."""
    e = np.longdouble(0)
    num = 0
    for r in terms:
        if len(r):
            e = np.cumsum(np.concatenate([np.array([e], np.longdouble), r.astype(np.longdouble)]))[-1]
            num += len(r)
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.longdouble(1e5) * np.sqrt(e / np.longdouble(num))), float(num)


def _g_of_sums(gsum, gnum):
    """:298-304: G = GSum / GNum, non-finite entries from 2 on extrapolated in order."""
    with np.errstate(invalid="ignore", divide="ignore"):
        G = gsum / gnum
    for i in range(2, 256):
        if not np.isfinite(G[i]):
            G[i] = G[i - 1] + (G[i - 1] - G[i - 2])
    return G


def g_step(E, t, stack):
    """:285-304 -> G (256,)."""
    n = stack.shape[0]
    d = stack.reshape(n, -1)
    b = d.reshape(-1).astype(np.int64)
    with np.errstate(all="ignore"):
        prod = (E[None, :] * t[:, None]).reshape(-1)  # E[k] * exposureVec[i], float64, i-major
    keep = b != 255
    gsum = np.bincount(b[keep], weights=prod[keep], minlength=256)
    gnum = np.bincount(b[keep], minlength=256).astype(np.float64)
    return _g_of_sums(gsum, gnum)


def g_step_by_image(E, t, stack):
    """g_step without the whole stack's products in memory: per image np.add.at in pixel order -> the same chains."""
    n = stack.shape[0]
    d = stack.reshape(n, -1)
    gsum = np.zeros(256)
    gnum = np.zeros(256)
    for i in range(n):
        m = d[i] != 255
        b = d[i][m]
        with np.errstate(all="ignore"):
            np.add.at(gsum, b, E[m] * t[i])
        gnum += np.bincount(b, minlength=256)
    return _g_of_sums(gsum, gnum)


def e_step(G, t, stack):
    """:319-339 -> E (w*h,)."""
    n = stack.shape[0]
    d = stack.reshape(n, -1)
    esum = np.zeros(d.shape[1])
    enum = np.zeros(d.shape[1])
    for i in range(n):
        m = d[i] != 255
        np.add(enum, t[i] * t[i], out=enum, where=m)
        with np.errstate(all="ignore"):
            np.add(esum, G[d[i]] * t[i], out=esum, where=m)
    with np.errstate(invalid="ignore", divide="ignore"):
        E = esum / enum
    E[E < 0] = 0
    return E


def _sparse(pos, vals, wh):
    """listed samples in position order -> (image, pixel, byte); 255 is never listed"""
    pos = np.asarray(pos, np.int64)
    vals = np.asarray(vals, np.uint8)
    o = np.argsort(pos, kind="stable")
    pos, vals = pos[o], vals[o]
    assert np.all(np.diff(pos) > 0) and not np.any(vals == 255)
    return pos // wh, pos % wh, vals.astype(np.int64)


def init_e_sparse(pos, vals, n, wh):
    """init_e of the sparse stack: the exact integer column sums 255 * n - sum(255 - v), one division."""
    _, k, v = _sparse(pos, vals, wh)
    s = np.full(wh, 255 * n, np.int64)
    np.subtract.at(s, k, 255 - v)
    return s.astype(np.float64) / float(n)


def g_step_sparse(pos, vals, E, t, wh):
    """g_step of the sparse stack: per bin one np.cumsum of its products E[k]*t_i in position order, from +0."""
    i, k, v = _sparse(pos, vals, wh)
    with np.errstate(all="ignore"):
        prod = E[k] * t[i]
    gsum = np.zeros(256)
    for b in np.unique(v):
        gsum[b] = np.cumsum(np.concatenate([[0.0], prod[v == b]]))[-1]
    return _g_of_sums(gsum, np.bincount(v, minlength=256).astype(np.float64))


def e_step_sparse(pos, vals, G, t, wh):
    """e_step of the sparse stack: np.add.at in position order, so every pixel's sums run over its images in order."""
    i, k, v = _sparse(pos, vals, wh)
    esum = np.zeros(wh)
    enum = np.zeros(wh)
    np.add.at(enum, k, t[i] * t[i])
    with np.errstate(all="ignore"):
        np.add.at(esum, k, G[v] * t[i])
        E = esum / enum
    E[E < 0] = 0
    return E


def rmse_sparse(pos, vals, G, E, t, wh):
    """rmse of the sparse stack (the listed samples in position order)."""
    i, k, v = _sparse(pos, vals, wh)
    with np.errstate(all="ignore"):
        r = G[v] - t[i] * E[k]
    r = r[np.isfinite(r)]
    with np.errstate(all="ignore"):
        return _rmse_of_terms([r * r * 1e-10])


def rescale(G, E):
    """:349-356: f = 255 / G[255]; E *= f; G[i] *= f only for i < min(256, w*h)."""
    with np.errstate(all="ignore"):
        f = np.float64(255.0) / G[255]
        E = E * f
        G = G.copy()
        lim = min(256, E.size)
        G[:lim] = G[:lim] * f
    return G, E, f


def solve(stack, t, iterations, g=g_step):
    """:250-358 on an already leak-padded stack -> (G, E, log); log = dict(init=(rmse, num), iters=[dict(...)]),
    and the G / E after every iteration in log['G'], log['E'].  g: g_step or g_step_by_image."""
    E = init_e(stack)
    G = np.zeros(256)
    log = {"init": rmse(G, E, t, stack), "iters": [], "G": [], "E": []}
    for _ in range(iterations):
        G = g(E, t, stack)
        rg = rmse(G, E, t, stack)
        E = e_step(G, t, stack)
        re = rmse(G, E, t, stack)
        G, E, f = rescale(G, E)
        rr = rmse(G, E, t, stack)
        log["iters"].append({"rmse_G": rg[0], "num_G": rg[1], "rmse_E": re[0], "num_E": re[1], "rmse_resc": rr[0], "num_resc": rr[1],
                             "rescale": f})
        log["G"].append(G.copy())
        log["E"].append(E.copy())
    return G, E, log


def pcalib_text(G):
    """pcalib.txt as the reference's ofstream writes it (precision 15, default float field = %.15g; nan / -nan / inf)."""
    def one(v):
        if np.isnan(v):
            return "-nan" if np.signbit(v) else "nan"
        if np.isinf(v):
            return "-inf" if v < 0 else "inf"
        return "%.15g" % v
    return " ".join(one(v) for v in G) + " \n"


def synthetic_sweep(rng, n, w, h, curve=None, t_lo=0.5, t_hi=20.0, noise=0.0):
    """A sweep of a static scene with irradiance E_true under exposures t: byte = round(f(E*t)) with a known response f
    (inverse: G_true), clipped to 0..255 -> (stack (n, h, w) uint8, t (n,) float64, f)."""
    if curve is None:
        def curve(x):
            return 255.0 * np.clip(x / 400.0, 0, 1) ** (1 / 2.2)
    yy, xx = np.mgrid[0:h, 0:w]
    E_true = 2.0 + 40.0 * (0.5 + 0.5 * np.sin(xx / max(w, 1) * 6.0) * np.cos(yy / max(h, 1) * 5.0)) + rng.random((h, w)) * 10.0
    t = np.exp(np.linspace(np.log(t_lo), np.log(t_hi), n))
    imgs = []
    for i in range(n):
        v = curve(E_true * t[i]) + (rng.normal(0, noise, (h, w)) if noise else 0)
        imgs.append(np.clip(np.rint(v), 0, 255).astype(np.uint8))
    return np.stack(imgs), t.astype(np.float64), curve
