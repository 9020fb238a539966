#!/usr/bin/env python3
"""Points per second of the lens-model kernels: libmdc_lens.so's three kinds (pinhole, RadTan, EquiDistant) and libmdc_hip.so's FOV
kernel, each on the same 200 x 10^6 device-resident points, in place, timed with HIP events on the stream; the median of the runs.

    python tools/lens_rate.py [--points 200000000] [--runs 11] [--out profiles/r11_lens_rate.txt]

Every kernel reads and writes 16 bytes per point; the last column is that traffic as a share of 8 TB/s."""
import argparse
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=200 * 10 ** 6)
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch

    from mono_dataset_code_amd import capi, synth

    n = a.points
    st = torch.cuda.current_stream().cuda_stream
    cam = [458.654, 457.296, 367.215, 248.375]
    rect = (302.97, 418.34, 308.85, 250.27)
    cases = [("pinhole", capi.Lens(capi.LensModel.make(capi.LENS_PINHOLE, cam + [0, 0, 0, 0], rect))),
             ("RadTan", capi.Lens(capi.LensModel.make(capi.LENS_RADTAN, cam + [-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05], rect))),
             ("EquiDistant", capi.Lens(capi.LensModel.make(capi.LENS_EQUIDISTANT, [190.978, 190.973, 254.931, 256.897, 0.003482389, 0.000715034, -0.002053236,
                                                                                  0.000202936], (60.18, 60.11, 251.97, 264.17))))]
    d = synth.write_sequence_calibration(tempfile.mkdtemp(prefix="mdc_lens_rate_"))
    fov = capi.UndistorterFOV(os.path.join(d, "camera.txt"))
    ctx = capi.Context(0)
    model = fov.model()
    cases.append(("FOV (libmdc_hip.so)", None))
    lines = ["lens-model kernels, %d points in place, %d runs each, HIP events, median" % (n, a.runs),
             "device: %s" % torch.cuda.get_device_name(0), "%-22s %10s %14s %10s" % ("kernel", "ms", "points/s", "of 8 TB/s")]
    for name, lens in cases:
        ms = []
        for run in range(a.runs + 2):
            x = torch.rand(n, device="cuda") * 640.0  # fresh rectified pixel coordinates every run: the kernels work in place
            y = torch.rand(n, device="cuda") * 480.0
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            if lens is None:
                ctx.distort_points_device(model, x.data_ptr(), y.data_ptr(), n, st)
            else:
                lens.distort_points_device(x.data_ptr(), y.data_ptr(), n, st)
            e1.record()
            e1.synchronize()
            if run >= 2:  # two warm-up runs
                ms.append(e0.elapsed_time(e1))
            del x, y
        med = float(np.median(ms))
        lines.append("%-22s %10.3f %14.4g %10.3f" % (name, med, n / (med * 1e-3), 16.0 * n / (med * 1e-3) / 8e12))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
