#!/usr/bin/env python3
"""In-process A/B of MDC_OPT_XCD_ROTATE on the bench camera: rotation off (each XCD runs the same tiles in every frame group) against on,
alternating, in ONE process on ONE pair of the allocator's buffers after an adaptive pre-roll -- boxes and processes differ by more than
the effect.  Per alternation the median of --launches single launches (one event pair each).  Decision rule: rotation counts as faster
only where the median of the on-medians lies below the median of the off-medians by more than three times the spread (largest minus
smallest) of the off-medians of this process.

  python tools/xcd_rotate_ab.py --frames 4096 --plans tuned,128x16 [--orders 0] [--alternations 5] [--launches 40]
  python tools/xcd_rotate_ab.py --frames 50000 --plans tuned --launches 12        # the sequence
  python tools/xcd_rotate_ab.py --workload undistort_f32 --frames 1024 --plans 128x16
  python tools/xcd_rotate_ab.py --workload pyramid --frames 1024 --plans builtin     # config 5: the strip kernel, chunked
A plan is `tuned` (mdc_tune_device's pick, measured with rotation off), `builtin` (no tuning, automatic frames per workgroup) or
COLSxROWS[xFPB] (default 128 frames per workgroup)."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mono_dataset_code_amd import capi, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--plans", default="tuned,128x16")
    ap.add_argument("--orders", default="0", help="MDC_ORDER_* modes, comma list")
    ap.add_argument("--workload", default="fused", choices=["fused", "undistort_f32", "pyramid"])
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--settle", type=float, default=0.3, help="seconds of untimed launches after every re-plan")
    ap.add_argument("--json", default="", help="append one JSON line per comparison to this file")
    a = ap.parse_args()
    f32, pyr = a.workload == "undistort_f32", a.workload == "pyramid"  # pyramid: the scale-1 camera, base + levels 1..3 (strip kernel)
    B, npi, npo = a.frames, 1280 * 1024, (1280 * 1024 if pyr else 640 * 480)
    d = synth.write_sequence_calibration(tempfile.mkdtemp(prefix="mdc_rotab_"), synth.camera_lines(1280, 1024, 1280, 1024) if pyr else synth.CAMERA_1280_TO_640)
    fov = capi.UndistorterFOV(os.path.join(d, "camera.txt"))
    photo = capi.PhotometricUndistorter(os.path.join(d, "pcalib.txt"), os.path.join(d, "vignette.png"), 1280, 1024)
    ctx = capi.Context(0)
    ctx.import_tables(capi.pack_tables(fov, photo))
    st = torch.cuda.Stream(device=torch.device("cuda", 0))
    torch.cuda.set_stream(st)
    s = st.cuda_stream
    flags = capi.GAMMA | capi.VIGNETTE | capi.KILL_OVEREXPOSED | capi.RECTIFY
    pb = ctx.alloc_placed(B, flags, capi.PLACE_AUTO, s, in_bytes=B * npi * 4 if f32 else 0)
    if f32:
        raw = torch.empty(B * npi, dtype=torch.uint8, device="cuda")
        ctx.synth_frames(raw.data_ptr(), 0, B, npi, synth.SEED, s)
        ctx.unmap_batch(raw.data_ptr(), pb.d_in, B, flags & ~capi.RECTIFY, s)
        torch.cuda.synchronize()
        del raw
    else:
        ctx.synth_frames(pb.d_in, 0, B, npi, synth.SEED, s)
    print("device %s pci %s, %d frames, workload %s, code_id %s" % (torch.cuda.get_device_name(0), ctx.pci_bus_id(), B, a.workload, capi.code_id()))
    print("buffers:", pb.describe()["how"])

    lv = [torch.empty(B * (npo >> (2 * l)), dtype=torch.float32, device="cuda") for l in range(1, 4)] if pyr else []

    def launch():
        if pyr:
            ctx.process_pyramid_batch(pb.d_in, pb.d_out, 4, [t.data_ptr() for t in lv], B, flags, s)
        elif f32:
            ctx.undistort_batch_f32(pb.d_in, pb.d_out, B, s)
        else:
            ctx.process_batch(pb.d_in, pb.d_out, B, flags, s)

    def window(seconds):
        t0 = time.perf_counter()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        n = 0
        e0.record()
        while True:
            for _ in range(4):
                launch()
            n += 4
            torch.cuda.synchronize()
            if time.perf_counter() - t0 >= seconds:
                break
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    def preroll():  # windows of 50 ms until five in a row agree within 1 %, at least 0.3 s, at most 8 s
        t0, wins = time.perf_counter(), []
        while True:
            wins.append(window(0.05))
            el = time.perf_counter() - t0
            last = wins[-5:]
            if (len(wins) > 5 and max(last) - min(last) <= 0.01 * min(last) and el >= 0.3) or el >= 8.0:
                return el, len(wins)

    def sample(frames):
        out = []
        for f in frames:
            out.append(ctx.copy_to_host(pb.d_out + 4 * npo * f, npo, np.float32).view(np.int32).copy())
        return out

    failed = False
    for plan in a.plans.split(","):
        for order in [int(x) for x in a.orders.split(",")]:
            ctx.set_option(capi.OPT_XCD_ROTATE, 0)
            ctx.set_option(capi.OPT_TILE_ORDER, order)
            ctx.set_option(capi.OPT_TILE_COLS, 0)
            ctx.set_option(capi.OPT_TILE_ROWS, 0)
            ctx.set_option(capi.OPT_FRAMES_PER_BLOCK, 0)
            if plan == "tuned" and not f32 and not pyr:
                t = ctx.tune(pb.d_in, pb.d_out, min(B, 4096), flags, s)
                cols, rows, fpb = t.tile_w, t.tile_h, t.frames_per_block
            elif plan == "builtin":
                cols = rows = fpb = 0
            else:
                p = [int(x) for x in plan.split("x")]
                cols, rows, fpb = p[0], p[1], (p[2] if len(p) > 2 else 128)
            # the plan is pinned by options, so that switching the rotation (which re-plans and forgets a tuned frame count) changes nothing else
            ctx.set_option(capi.OPT_TILE_COLS, cols)
            ctx.set_option(capi.OPT_TILE_ROWS, rows)
            ctx.set_option(capi.OPT_FRAMES_PER_BLOCK, fpb)
            info = ctx.info()
            el, nw = preroll()
            med = {0: [], 1: []}
            outs = {}
            picks = sorted({0, 1, B // 3, B // 2, B - 2, B - 1} & set(range(B)))
            for alt in range(a.alternations):
                for rot in (0, 1):
                    ctx.set_option(capi.OPT_XCD_ROTATE, (2 if pyr else 1) if rot else 0)  # the strip kernel rotates at 2 only
                    launch()
                    torch.cuda.synchronize()
                    if alt == 0:
                        outs[rot] = sample(picks)
                    t_s = time.perf_counter()
                    while time.perf_counter() - t_s < a.settle:
                        for _ in range(4):
                            launch()
                        torch.cuda.synchronize()
                    ts = []
                    for _ in range(a.launches):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        launch()
                        e1.record()
                        e1.synchronize()
                        ts.append(e0.elapsed_time(e1))
                    med[rot].append(float(np.median(ts)))
            same = all(np.array_equal(x, y) for x, y in zip(outs[0], outs[1]))
            off, on = float(np.median(med[0])), float(np.median(med[1]))
            spread = max(med[0]) - min(med[0])
            gain = off - on > 3 * spread
            rec = {"workload": a.workload, "frames": B, "plan": plan, "tile": [info.tile_w, info.tile_h], "frames_per_workgroup": fpb, "order": order,
                   "off_medians_ms": [round(x, 4) for x in med[0]], "on_medians_ms": [round(x, 4) for x in med[1]], "off_ms": round(off, 4), "on_ms": round(on, 4),
                   "on_over_off": round(on / off, 4), "off_spread_ms": round(spread, 4), "gain_by_rule": bool(gain), "sampled_frames_bit_equal": bool(same),
                   "preroll_s": round(el, 2), "preroll_windows": nw}
            print(json.dumps(rec), flush=True)
            if a.json:
                with open(a.json, "a") as f:
                    f.write(json.dumps(rec) + "\n")
            failed = failed or not same
    if failed:
        print("RESULTS DIFFER between rotation off and on")
        sys.exit(1)


if __name__ == "__main__":
    main()
