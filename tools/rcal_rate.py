"""responseCalib solver rates (include/mdc_hip.h: mdc_rcal_*) on a synthetic exposure sweep held in HBM.

Per size: the exact-order index build, the whole solve in both modes (ms per iteration = (solve(K) - solve(0) [- index]) / K),
and the single steps (each step call allocates its scratch and synchronises: its time is an upper bound of the pass), with the
bytes every streaming pass reads and the fraction of 8 TB/s that makes.  The longest bin chain bounds the exact-order G step.

  python tools/rcal_rate.py [--sizes 1000x1280x1024,200x640x480] [--iterations 4] [--json out.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8.0e12  # bytes/s, MI355X HBM3E peak


def make_sweep(n, w, h, device):
    """A static scene under n log-spaced exposures through a gamma-like response, noise from a fixed generator."""
    import torch

    g = torch.Generator(device=device)
    g.manual_seed(1234)
    yy, xx = torch.meshgrid(torch.arange(h, device=device, dtype=torch.float32), torch.arange(w, device=device, dtype=torch.float32), indexing="ij")
    E = 2.0 + 40.0 * (0.5 + 0.5 * torch.sin(xx / w * 6.0) * torch.cos(yy / h * 5.0))
    t = torch.exp(torch.linspace(float(torch.log(torch.tensor(1e-3))), float(torch.log(torch.tensor(40.0))), n, dtype=torch.float64, device=device))
    stack = torch.empty((n, h, w), dtype=torch.uint8, device=device)
    for i in range(n):
        v = 255.0 * torch.clamp(E * float(t[i]) / 400.0, 0, 1) ** (1 / 2.2) + torch.randn((h, w), generator=g, device=device) * 1.5
        stack[i] = torch.clamp(torch.round(v), 0, 255).to(torch.uint8)
    return stack, t


def timed(fn, reps=1):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()  # warm-up
    torch.cuda.synchronize()
    best = None
    for _ in range(reps):
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b)
        best = ms if best is None else min(best, ms)
    return best


def measure(ctx, n, w, h, iterations):
    import torch

    from mono_dataset_code_amd import capi

    stack, t = make_sweep(n, w, h, "cuda")
    ctx.rcal_leak_pad(stack, 2)
    N = n * w * h
    res = {"n": n, "w": w, "h": h, "samples": N, "iterations": iterations}
    index = ctx.rcal_index(stack)
    res["index_bytes"] = index.bytes
    res["index_entries"] = index.entries
    res["longest_chain"] = index.longest_chain
    res["longest_chain_fraction"] = index.longest_chain / max(index.entries, 1)
    res["index_build_ms"] = timed(lambda: ctx.rcal_index(stack).close())
    E = ctx.rcal_init_e(stack)
    G = torch.zeros(256, dtype=torch.float64, device="cuda")
    ctx.rcal_g_step_indexed(index, t, E, G)
    res["g_step_exact_ms"] = timed(lambda: ctx.rcal_g_step_indexed(index, t, E, G), 3)
    res["g_step_direct_ms"] = timed(lambda: ctx.rcal_g_step(stack, t, E, G), 3)
    E2 = E.clone()
    res["e_step_ms"] = timed(lambda: ctx.rcal_e_step(stack, t, G, E2), 3)
    res["rmse_ms"] = timed(lambda: ctx.rcal_rmse(stack, t, G, E), 3)
    index.close()
    # streaming passes read the stack once (+ E once, 8 bytes per pixel, + E written once by the E step)
    pass_bytes = N + 8 * w * h
    res["pass_bytes"] = pass_bytes
    for k in ("g_step_direct_ms", "e_step_ms", "rmse_ms"):
        res[k.replace("_ms", "_hbm_fraction")] = pass_bytes / (res[k] * 1e-3) / PEAK
    res["g_step_exact_adds_per_ns"] = res["longest_chain"] / (res["g_step_exact_ms"] * 1e6)
    for mode, name in ((capi.RCAL_EXACT_ORDER, "exact"), (capi.RCAL_DIRECT, "direct")):
        t0 = timed(lambda: ctx.rcal_solve(stack, t, 0, mode))
        tk = timed(lambda: ctx.rcal_solve(stack, t, iterations, mode))
        per = (tk - t0 - (res["index_build_ms"] if mode == capi.RCAL_EXACT_ORDER else 0.0)) / iterations
        res["solve_%s_ms" % name] = tk
        res["iteration_%s_ms" % name] = per
    del stack
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000x1280x1024,200x640x480")
    ap.add_argument("--iterations", type=int, default=4)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    from mono_dataset_code_amd import capi

    ctx = capi.Context(0)
    out = []
    for s in a.sizes.split(","):
        n, w, h = (int(x) for x in s.split("x"))
        r = measure(ctx, n, w, h, a.iterations)
        out.append(r)
        print(json.dumps(r), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
