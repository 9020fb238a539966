#!/usr/bin/env python3
"""Points per second of the inverse lens kernels (libmdc_lensinv.so: pinhole, RadTan, EquiDistant, FOV), each beside the forward
kernel of its kind in the same process (libmdc_lens.so; libmdc_hip.so for FOV) on the same number of device-resident points, in
place, timed with HIP events on the stream; the median of the runs.  Then UndistorterFOV::undistortCoordinates on host arrays, with
the device path forced and with the host loop forced (child processes: the threshold is read once per process), at point counts on
both sides of the default threshold.

    python tools/lens_inverse_rate.py [--points 200000000] [--runs 11] [--out profiles/r12_lensinv_rate.txt]

Every kernel reads and writes 16 bytes per point; the last column is that traffic as a share of 8 TB/s."""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CAMERAS = {  # name -> camera.txt lines: the two public cameras of the lens tests and the FOV camera every frame test runs
    "RadTan": ("RadTan 458.654 457.296 367.215 248.375 -0.28340811 0.07395907 0.00019359 1.76187114e-05", "752 480", "crop", "640 480"),
    "EquiDistant": ("EquiDistant 190.978 190.973 254.931 256.897 0.003482389 0.000715034 -0.002053236 0.000202936", "512 512", "crop", "512 512"),
    "FOV": ("0.349153 0.436593 0.493140 0.499021 0.933271", "1280 1024", "0.4 0.53 0.5 0.5 0", "640 480"),
}
CLASS_COUNTS = (4096, 16384, 65535, 65536, 262144, 1048576)


def write_camera(lines):
    d = tempfile.mkdtemp(prefix="mdc_lensinv_rate_")
    path = os.path.join(d, "camera.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return path


def child(name):
    """one camera, the threshold as the environment set it: ms per call of the class method (median of 7) at every count"""
    import time

    import numpy as np

    from mono_dataset_code_amd import capi

    fov = capi.UndistorterFOV(write_camera(CAMERAS[name]))
    W, H = fov.dims()[:2]
    rng = np.random.default_rng(3)
    out = []
    for n in CLASS_COUNTS:
        x0, y0 = rng.uniform(0, W - 1, n).astype(np.float32), rng.uniform(0, H - 1, n).astype(np.float32)
        ms = []
        for run in range(9):
            x, y = x0.copy(), y0.copy()
            t = time.perf_counter()
            fov.undistort_coordinates(x, y)
            if run >= 2:
                ms.append((time.perf_counter() - t) * 1e3)
        out.append("%.4f" % float(np.median(ms)))
    print("CLASS " + " ".join(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=200 * 10 ** 6)
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    import numpy as np
    import torch

    from mono_dataset_code_amd import capi

    n = a.points
    st = torch.cuda.current_stream().cuda_stream
    ctx = capi.Context(0)
    objects = {name: capi.UndistorterFOV(write_camera(lines)) for name, lines in CAMERAS.items()}
    pin = objects["RadTan"].inverse_model()
    pin.kind = capi.LENSINV_PINHOLE
    cases = [("pinhole", pin, capi.Lens(pin), None)]
    for name in ("RadTan", "EquiDistant"):
        m = objects[name].inverse_model()
        cases.append((name, m, capi.Lens(m), None))
    cases.append(("FOV", objects["FOV"].inverse_model(), None, objects["FOV"].model()))
    lines = ["inverse lens kernels beside the forward ones, %d points in place, %d runs each, HIP events, median; measured on this device" % (n, a.runs),
             "device: %s" % torch.cuda.get_device_name(0),
             "%-28s %10s %14s %10s" % ("kernel", "ms", "points/s", "of 8 TB/s")]
    for name, m, lens, fov_model in cases:
        inv = capi.LensInverse(m)
        for direction in ("forward", "inverse"):
            ms = []
            for run in range(a.runs + 2):
                # fresh coordinates every run (the kernels work in place): rectified pixels for the forward kernel, raw ones for the inverse
                w, h = (m.out_w, m.out_h) if direction == "forward" else (m.in_w, m.in_h)
                x = torch.rand(n, device="cuda") * float(w - 1)
                y = torch.rand(n, device="cuda") * float(h - 1)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                if direction == "inverse":
                    inv.undistort_points_device(x.data_ptr(), y.data_ptr(), n, st)
                elif lens is None:
                    ctx.distort_points_device(fov_model, x.data_ptr(), y.data_ptr(), n, st)
                else:
                    lens.distort_points_device(x.data_ptr(), y.data_ptr(), n, st)
                e1.record()
                e1.synchronize()
                if run >= 2:  # two warm-up runs
                    ms.append(e0.elapsed_time(e1))
                del x, y
            med = float(np.median(ms))
            lines.append("%-28s %10.3f %14.4g %10.3f" % (name + " " + direction, med, n / (med * 1e-3), 16.0 * n / (med * 1e-3) / 8e12))
    lines += ["", "UndistorterFOV::undistortCoordinates on host arrays, ms per call (median of 7), measured on this device and its host:",
              "%-14s %-8s " % ("camera", "path") + " ".join("%10d" % c for c in CLASS_COUNTS)]
    for name in ("RadTan", "EquiDistant", "FOV"):
        for path, gpu_min in (("device", "1"), ("host", "0")):
            env = dict(os.environ, MDC_UNDISTORT_GPU_MIN=gpu_min)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, env=env,
                               timeout=300)
            got = [l for l in r.stdout.splitlines() if l.startswith("CLASS ")]
            vals = got[0].split()[1:] if r.returncode == 0 and got else ["failed"] * len(CLASS_COUNTS)
            lines.append("%-14s %-8s " % (name, path) + " ".join("%10s" % v for v in vals))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
