#!/usr/bin/env python3
"""Rate of the device ZIP writer (include/mdc_zipw.h) on the encoder's own workload (tools/jenc_rate.py's).
  python tools/zipw_rate.py [frames=1024] [repeats=10]
Workload: `frames` synthetic 1280x1024 frames rectified to 640x480 float, encoded once at quality 95 by mdcj_encode_f32_device and
left in their slots in HBM.  Reported, each the median of `repeats` timed runs after two warm-up runs:
  mdcj_fetch                  host clock: the encoder's gather + one copy into page-locked memory (the path before this library)
  append to /dev/shm          host clock around mdcz_append_device on a fresh writer whose file is on /dev/shm
  append to /dev/null         the same with the write() going nowhere: append minus the file write
  CRC, tables / shift-XOR     HIP events around mdcz_crc32_device and its 32-step variant
  CRC + scan + gather         HIP events around mdcz_segment_device (scan + gather = this minus the CRC line; kernel by kernel: run
                              the tool under `rocprofv3 --kernel-trace --stats`)
  zlib.crc32, one thread      host clock over the same bytes
The archive of the first append is compared with zipfile and zlib before anything is timed.  One process, no retries: an error or a
fault ends the run with a non-zero status."""
import os
import sys
import tempfile
import time
import zipfile
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mono_dataset_code_amd import capi, synth  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
reps = max(3, int(sys.argv[2])) if len(sys.argv) > 2 else 10
W, H, w, h, Q = 1280, 1024, 640, 480, 95
npix = w * h

d = synth.write_sequence_calibration(tempfile.mkdtemp(prefix="mdc_zipw_rate_"))
fov = capi.UndistorterFOV(os.path.join(d, "camera.txt"))
photo = capi.PhotometricUndistorter(os.path.join(d, "pcalib.txt"), os.path.join(d, "vignette.png"), W, H)
ctx = capi.Context(0)
ctx.bind(fov, photo)
d_frames = torch.empty(n * npix, dtype=torch.float32, device="cuda:0")
chunk = 128
d_raw = torch.empty(chunk * W * H, dtype=torch.uint8, device="cuda:0")
for first in range(0, n, chunk):
    m = min(chunk, n - first)
    ctx.synth_frames(d_raw.data_ptr(), first, m, W * H, synth.SEED, 0)
    ctx.process_batch(d_raw.data_ptr(), d_frames.data_ptr() + first * npix * 4, m, capi.RECTIFY, 0)
torch.cuda.synchronize()
del d_raw
torch.cuda.empty_cache()

enc = capi.JpegEncoder(w, h, Q, max_frames=n, device=0)
d_out, slot, d_sizes = enc.output()
J, Zl = capi.jenc_lib(), capi.zipw_lib()
if J.mdcj_encode_f32_device(enc._h, d_frames.data_ptr(), npix, n, d_out, slot, d_sizes, None) != 0:
    raise RuntimeError(J.mdcj_last_error().decode())
sizes = np.zeros(n, np.int32)
total = J.mdcj_fetch(enc._h, d_out, slot, d_sizes, n, None, 0, sizes.ctypes.data, None)
if total < 0:
    raise RuntimeError(J.mdcj_last_error().decode())
pinned = capi.PinnedArray((int(total) + 4096,), np.uint8)


def fetch():
    got = J.mdcj_fetch(enc._h, d_out, slot, d_sizes, n, pinned.array.ctypes.data, pinned.array.size, sizes.ctypes.data, None)
    if got != total:
        raise RuntimeError("fetch: %d, expected %d (%s)" % (got, total, J.mdcj_last_error().decode()))


# correctness before speed: one archive through zipfile, members against the fetched bytes
fetch()
at = np.concatenate([[0], np.cumsum(sizes.astype(np.int64))])
shm = "/dev/shm/mdc_zipw_rate_%d.zip" % os.getpid()
wr = capi.ZipWriter(shm, device=0)
wr.append(d_out, slot, d_sizes, n)
size = wr.close()
with zipfile.ZipFile(shm) as z:
    if z.namelist() != ["%05d.jpg" % i for i in range(n)] or z.testzip() is not None:
        raise SystemExit("the archive does not read back")
    for i in (0, n // 2, n - 1):
        if z.read("%05d.jpg" % i) != pinned.array[at[i]:at[i + 1]].tobytes():
            raise SystemExit("member %d differs from the fetched file" % i)
os.unlink(shm)
writers = {}


def append_to(path):
    def run():
        writers[path].append(d_out, slot, d_sizes, n)
    return run


def clock(fn, before=None, after=None):
    ts = []
    for k in range(reps + 2):
        if before:
            before()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        if after:
            after()
        if k >= 2:
            ts.append((t1 - t0) * 1e3)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def events(fn):
    ts = []
    for k in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if k >= 2:
            ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def fresh(path):
    # one writer per path for the whole measurement (its staging buffers are allocated by the warm-up runs, as mdcj_fetch's are);
    # the file is cut back to nothing before every append so that /dev/shm holds one archive at a time
    def run():
        if path not in writers:
            writers[path] = capi.ZipWriter(path, device=0)
        else:
            os.truncate(path, 0) if path != "/dev/null" else None
    return run


t_fetch = clock(fetch)
t_shm = clock(append_to(shm), before=fresh(shm))
t_null = clock(append_to("/dev/null"), before=fresh("/dev/null"))
for wr in writers.values():
    wr.abort()
d_crc = torch.zeros(n, dtype=torch.int32, device="cuda:0")
t_crc = events(lambda: capi.crc32_device(d_out, slot, d_sizes, n, d_crc.data_ptr()))
crc_tables = d_crc.cpu().numpy().view(np.uint32).copy()
t_crc1 = events(lambda: capi.crc32_device(d_out, slot, d_sizes, n, d_crc.data_ptr(), variant=1))
if not (crc_tables == d_crc.cpu().numpy().view(np.uint32)).all():
    raise SystemExit("the two checksum variants disagree")
bound = Zl.mdcz_segment_bound(n, int(total), 9)
d_seg = torch.empty(int(bound), dtype=torch.uint8, device="cuda:0")
d_rec = torch.empty((n + 1) * 2, dtype=torch.int64, device="cuda:0")


def segment():
    if Zl.mdcz_segment_device(d_out, slot, d_sizes, None, n, 0, b".jpg", d_seg.data_ptr(), int(bound), d_rec.data_ptr(), None) != 0:
        raise RuntimeError(Zl.mdcz_last_error().decode())


t_seg = events(segment)
host = [pinned.array[at[i]:at[i + 1]] for i in range(n)]
ts = []
for _ in range(3):
    t0 = time.perf_counter()
    crcs = [zlib.crc32(b) for b in host]
    ts.append((time.perf_counter() - t0) * 1e3)
t_zlib = float(np.median(ts))
if not (np.array(crcs, np.uint32) == crc_tables).all():
    raise SystemExit("the device checksums differ from zlib's")

parts = capi.crc32_geometry(slot, n)[4]
print("device ZIP writer, %d encoded 640 x 480 noise frames (quality %d) in their slots in HBM: %.1f MB, %.1f KB per file, slot %d bytes, %d parts per file;"
      " %d timed repeats (median [min .. max])" % (n, Q, total / 1e6, total / n / 1e3, slot, parts, reps))
print("  archive               : %d bytes, read back by zipfile, members == mdcj_fetch's, checksums == zlib's" % size)
rows = (("mdcj_fetch (gather + copy)  ", t_fetch), ("append to /dev/shm         ", t_shm), ("append to /dev/null        ", t_null),
        ("CRC-32, LDS tables         ", t_crc), ("CRC-32, 32 shift-XOR steps ", t_crc1), ("CRC + scan + gather        ", t_seg))
for name, (med, lo, hi) in rows:
    print("  %s : %9.3f ms [%9.3f .. %9.3f] = %7.1f GB/s of file bytes" % (name, med, lo, hi, total / med / 1e6))
print("  scan + gather (difference)  : %9.3f ms" % (t_seg[0] - t_crc[0]))
print("  zlib.crc32, one host thread : %9.3f ms = %7.2f GB/s" % (t_zlib, total / t_zlib / 1e6))
print("  append minus the file write vs mdcj_fetch: %+.1f %%; the file write (/dev/shm - /dev/null): %.3f ms; zlib.crc32 vs the device CRC: %.0f x"
      % ((t_null[0] / t_fetch[0] - 1) * 100, t_shm[0] - t_null[0], t_zlib / t_crc[0]))
enc.close()
ctx.close()
