"""Test-owned NumPy restatement of the reference's responseCalib (src/main_responseCalib.cpp:189-380), in the reference's order of
operations: the pin of tests/test_rcal*.py.

  G step (:285-304): np.bincount with weights adds sequentially in input order -- the i-major flattened stack, products E[k]*t_i
                     formed in float64 first, exactly the reference's GSum chain;
  E step (:319-339): an explicit loop over the images, per pixel ENum += t*t, ESum += G[b]*t where b != 255;
  rmse   (:50-69)  : terms r*r*1e-10 in float64, summed sequentially (cumsum) in np.longdouble."""
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
    terms = np.concatenate(terms) if terms else np.zeros(0)
    num = len(terms)
    e = np.cumsum(terms.astype(np.longdouble))[-1] if num else np.longdouble(0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.longdouble(1e5) * np.sqrt(e / np.longdouble(num))), float(num)


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
    with np.errstate(invalid="ignore", divide="ignore"):
        G = gsum / gnum
    for i in range(2, 256):
        if not np.isfinite(G[i]):
            G[i] = G[i - 1] + (G[i - 1] - G[i - 2])
    return G


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


def rescale(G, E):
    """:349-356: f = 255 / G[255]; E *= f; G[i] *= f only for i < min(256, w*h)."""
    with np.errstate(all="ignore"):
        f = np.float64(255.0) / G[255]
        E = E * f
        G = G.copy()
        lim = min(256, E.size)
        G[:lim] = G[:lim] * f
    return G, E, f


def solve(stack, t, iterations):
    """:250-358 on an already leak-padded stack -> (G, E, log); log = dict(init=(rmse, num), iters=[dict(...)]),
    and the G / E after every iteration in log['G'], log['E']."""
    E = init_e(stack)
    G = np.zeros(256)
    log = {"init": rmse(G, E, t, stack), "iters": [], "G": [], "E": []}
    for _ in range(iterations):
        G = g_step(E, t, stack)
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
