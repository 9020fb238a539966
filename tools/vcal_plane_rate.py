#!/usr/bin/env python3
"""vignetteCalib's plane -> image coordinates (reference src/main_vignetteCalib.cpp:230-258, :284, :345-357) at the tool's real size --
gw x gh = 1000 x 1000 plane points, rectified 640 x 480 of a 1280 x 1024 FOV camera -- for n frames at once: mdc_vcal_plane_coords_device
(corners -> HK -> projection -> distortCoordinates -> coordinate mask, one pass) against the same result from the projection plus the
two separate entry points (mdc_distort_points_device, mdc_vcal_mask_coords_device).  HIP events, median of the repetitions.
usage: python tools/vcal_plane_rate.py [n_frames] [repetitions]"""
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import vcal_plane_restatement as V  # noqa: E402
from mono_dataset_code_amd import capi, synth  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 200
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
gw = gh = 1000
d = synth.write_sequence_calibration(tempfile.mkdtemp(prefix="mdc_vpr_"))
fov = capi.UndistorterFOV(os.path.join(d, "camera.txt"))
m = fov.model()
ctx = capi.Context(0)
corners = torch.from_numpy(V.random_corners(np.random.default_rng(1), N, m.out_w, m.out_h, side=(60, 300), tilt=0.4)).cuda()


def timed(fn):
    ts = []
    for _ in range(REPS + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts[1:])), out


fused_ms, (p2x, p2y, hk) = timed(lambda: ctx.vcal_plane_coords(m, gw, gh, 5, 5, corners=corners))


def separate():
    x, y, _ = ctx.vcal_plane_coords(None, gw, gh, hk=hk)
    ctx.distort_points_device(m, x.data_ptr(), y.data_ptr(), x.numel())
    ctx.vcal_mask_coords(x, y, m.in_w, m.in_h)
    return x, y


sep_ms, (x, y) = timed(separate)
same = bool(torch.equal(torch.isnan(p2x), torch.isnan(x)) and torch.equal(p2x.nan_to_num(-1e30).view(torch.int32), x.nan_to_num(-1e30).view(torch.int32))
            and torch.equal(p2y.nan_to_num(-1e30).view(torch.int32), y.nan_to_num(-1e30).view(torch.int32)))
gb = 2 * 4 * N * gw * gh / 1e9
print("code_id %s build_flags %r device %s" % (capi.code_id(), capi.build_flags(), torch.cuda.get_device_name(0)))
print("VCAL_PLANE n=%d frames x %d plane points: fused %.3f ms (%.1f us / frame, %.2f TB/s of coordinates written); "
      "projection + distort + mask as three calls %.3f ms; equal bit for bit: %s; points kept %.3f"
      % (N, gw * gh, fused_ms, 1e3 * fused_ms / N, gb / fused_ms, sep_ms, same, float(torch.isfinite(p2x).float().mean())))
