#!/usr/bin/env python3
"""Rate of the device JPEG encoder (include/mdc_jenc.h) on device-resident rectified frames of the synthetic sequence.
  python tools/jenc_rate.py [frames=1024] [repeats=10] [pil_frames=256]
Workload: `frames` synthetic 1280x1024 frames rectified to 640x480 float (the fused pass with MDC_RECTIFY only: what
playDataset saves), left in HBM.  Reported, each the median of `repeats` timed runs after two warm-up runs:
  encode only           HIP events around mdcj_encode_f32_device
  encode + copy-out     host clock around encode + mdcj_fetch into page-locked memory (ends in a stream synchronise)
  float copy-out alone  HIP events around one device -> page-locked copy of the float frames (what a host encoder needs first)
  PIL on one thread     Image.save(JPEG, quality=95) of the same frames, rounded to 8 bit beforehand, on this machine's host
The first frames' files are compared with PIL's byte for byte before anything is timed.  One process, no retries: an error
or a fault ends the run with a non-zero status.  (Per-kernel times: run it under `rocprofv3 --kernel-trace --stats`.)"""
import io
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

from mono_dataset_code_amd import capi, synth  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
reps = max(10, int(sys.argv[2])) if len(sys.argv) > 2 else 10
n_pil = min(n, int(sys.argv[3]) if len(sys.argv) > 3 else 256)
W, H, w, h, Q = 1280, 1024, 640, 480, 95
npix = w * h

d = synth.write_sequence_calibration(tempfile.mkdtemp(prefix="mdc_jenc_rate_"))
fov = capi.UndistorterFOV(os.path.join(d, "camera.txt"))
photo = capi.PhotometricUndistorter(os.path.join(d, "pcalib.txt"), os.path.join(d, "vignette.png"), W, H)
ctx = capi.Context(0)
ctx.bind(fov, photo)
s = 0  # the default stream throughout
d_frames = torch.empty(n * npix, dtype=torch.float32, device="cuda:0")
chunk = 128
d_raw = torch.empty(chunk * W * H, dtype=torch.uint8, device="cuda:0")
for first in range(0, n, chunk):
    m = min(chunk, n - first)
    ctx.synth_frames(d_raw.data_ptr(), first, m, W * H, synth.SEED, s)
    ctx.process_batch(d_raw.data_ptr(), d_frames.data_ptr() + first * npix * 4, m, capi.RECTIFY, s)
torch.cuda.synchronize()
del d_raw
torch.cuda.empty_cache()

enc = capi.JpegEncoder(w, h, Q, max_frames=n, device=0)
d_out, slot, d_sizes = enc.output()
L = capi.jenc_lib()
sizes = np.zeros(n, np.int32)


def encode():
    rc = L.mdcj_encode_f32_device(enc._h, d_frames.data_ptr(), npix, n, d_out, slot, d_sizes, None)
    if rc != 0:
        raise RuntimeError(L.mdcj_last_error().decode())


encode()
total = L.mdcj_fetch(enc._h, d_out, slot, d_sizes, n, None, 0, sizes.ctypes.data, None)
if total < 0:
    raise RuntimeError(L.mdcj_last_error().decode())
pinned = capi.PinnedArray((int(total) + 4096,), np.uint8)


def encode_and_fetch():
    encode()
    got = L.mdcj_fetch(enc._h, d_out, slot, d_sizes, n, pinned.array.ctypes.data, pinned.array.size, sizes.ctypes.data, None)
    if got != total:
        raise RuntimeError("fetch: %d, expected %d (%s)" % (got, total, L.mdcj_last_error().decode()))


def pil_bytes(u8):
    buf = io.BytesIO()
    Image.fromarray(u8, "L").save(buf, "JPEG", quality=Q)
    return buf.getvalue()


# correctness before speed: the first frames, byte for byte
encode_and_fetch()
at = np.concatenate([[0], np.cumsum(sizes.astype(np.int64))])
host_f = d_frames[: n_pil * npix].cpu().numpy().reshape(n_pil, h, w)
with np.errstate(invalid="ignore"):
    host_u8 = np.where(np.isnan(host_f), 0, np.clip(np.rint(host_f), 0, 255)).astype(np.uint8)
for i in range(min(8, n_pil)):
    if pinned.array[at[i]:at[i + 1]].tobytes() != pil_bytes(host_u8[i]):
        raise SystemExit("frame %d differs from PIL's file" % i)


def events(fn):
    fn()
    fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def clock(fn):
    fn()
    fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


t_enc = events(encode)
t_both = clock(encode_and_fetch)
host_pinned = torch.empty(n * npix, dtype=torch.float32).pin_memory()
t_float = events(lambda: host_pinned.copy_(d_frames, non_blocking=True))
ts = []
for i in range(n_pil):
    t0 = time.perf_counter()
    pil_bytes(host_u8[i])
    ts.append(time.perf_counter() - t0)
t_pil = float(np.median(ts)) * 1e3

print("device JPEG encoder, %d rectified %d x %d float frames of the synthetic sequence in HBM, quality %d, %d timed repeats (median [min .. max])"
      % (n, w, h, Q, reps))
print("  encoded size          : %.1f KB per frame (float frame %.1f KB: %.1f x smaller), first %d files == PIL's"
      % (total / n / 1e3, npix * 4 / 1e3, npix * 4 * n / total, min(8, n_pil)))
for name, (med, lo, hi) in (("encode only          ", t_enc), ("encode + copy-out    ", t_both), ("float copy-out alone ", t_float)):
    print("  %s : %9.3f ms [%9.3f .. %9.3f] = %8.0f frames/s, %7.2f us per frame" % (name, med, lo, hi, n / med * 1e3, med / n * 1e3))
print("  PIL, one host thread  : %9.3f ms per frame (median of %d frames) = %8.0f frames/s" % (t_pil, n_pil, 1e3 / t_pil))
print("  encode + copy-out vs float copy-out alone: %.2f x; vs PIL on one thread: %.0f x" % (t_float[0] / t_both[0], t_pil * n / t_both[0]))
enc.close()
ctx.close()
