#!/usr/bin/env python3
"""Rate and file sizes of the device PNG encoder (include/mdc_pngw.h) on the JPEG encoder's workload (tools/jenc_rate.py's).
  python tools/pngw_rate.py [frames=1024] [repeats=10] [workloads=noise,smooth] [filters=adaptive,0]
Two workloads of `frames` rectified 640x480 float frames in HBM: "noise", the synthetic 1280x1024 sequence rectified (what
tools/jenc_rate.py and tools/zipw_rate.py encode), and "smooth", 32 different smooth 640x480 frames (synth.smooth_frame) repeated.
Reported per workload, each the median of `repeats` timed runs after two warm-up runs:
  encode, adaptive / filter 0   HIP events around mdcp_encode_f32_device (kernel by kernel: run the tool under
                                `rocprofv3 --kernel-trace --stats -- python tools/pngw_rate.py 1024 3 noise adaptive`)
  encode + append to /dev/null  host clock around mdcp_encode_f32_device + mdcz_append_device(".png") on a writer whose write()
                                goes nowhere: the whole way out of HBM, lossless
  JPEG: encode + append         the same through mdcj_encode_f32_device at quality 95 (the lossy route)
  float frames to the host      host clock around one copy of the float frames into page-locked memory (the lossless route before)
  PIL level 1 / level 6         Image.save(..., 'PNG', compress_level=...) of 16 of the frames on one host thread: time and size
Three files of every workload are decoded by PIL and compared with the converted frames before anything is timed.  One process, no
retries: an error or a fault ends the run with a non-zero status."""
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
reps = max(3, int(sys.argv[2])) if len(sys.argv) > 2 else 10
workloads = sys.argv[3].split(",") if len(sys.argv) > 3 else ["noise", "smooth"]
filters = sys.argv[4].split(",") if len(sys.argv) > 4 else ["adaptive", "0"]
W, H, w, h, Q = 1280, 1024, 640, 480, 95
npix = w * h
ADAPTIVE = capi.PNG_FILTER_ADAPTIVE


def noise_frames():
    d = synth.write_sequence_calibration(tempfile.mkdtemp(prefix="mdc_pngw_rate_"))
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
    ctx.close()
    return d_frames


def smooth_frames():
    base = np.stack([synth.smooth_frame(w, h, 0.3 * k, blobs=k % 2 == 0).reshape(-1).astype(np.float32) for k in range(32)])
    return torch.from_numpy(base).to("cuda:0").repeat((n + 31) // 32, 1)[:n].contiguous().view(-1)


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


def clock(fn):
    ts = []
    for k in range(reps + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k >= 2:
            ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def measure(name, d_frames):
    P, J = capi.pngw_lib(), capi.jenc_lib()
    host16 = d_frames[:16 * npix].cpu().numpy().reshape(16, h, w)
    with np.errstate(invalid="ignore"):
        u8 = np.where(np.isnan(host16), 0, np.clip(np.rint(host16), 0, 255)).astype(np.uint8)
    rows, sizes_by = [], {}
    for label, filt in [(f if f == "adaptive" else "filter " + f, ADAPTIVE if f == "adaptive" else int(f)) for f in filters]:
        enc = capi.PngEncoder(w, h, depth=8, filter=filt, max_images=n, device=0)
        slot = enc.bound
        out_t = torch.empty(n * slot, dtype=torch.uint8, device="cuda:0")
        sizes_t = torch.zeros(n, dtype=torch.int32, device="cuda:0")
        d_out, d_sizes = out_t.data_ptr(), sizes_t.data_ptr()

        def encode():
            if P.mdcp_encode_f32_device(enc._h, d_frames.data_ptr(), npix, n, d_out, slot, d_sizes, None) != 0:
                raise RuntimeError(P.mdcp_last_error().decode())

        encode()
        torch.cuda.synchronize()
        sizes = sizes_t.cpu().numpy()
        for i in (0, 7, 15):  # correctness before speed
            data = out_t[i * slot:i * slot + int(sizes[i])].cpu().numpy()
            if not np.array_equal(np.array(Image.open(io.BytesIO(data.tobytes()))), u8[i]):
                raise SystemExit("%s, %s: file %d does not decode to its frame" % (name, label, i))
        sizes_by[label] = sizes
        rows.append(("encode, %s" % label, events(encode), int(sizes.sum())))
        if filt == ADAPTIVE:
            wr = capi.ZipWriter("/dev/null", device=0)

            def whole():
                encode()
                wr.append(d_out, slot, d_sizes, n, suffix=".png")

            rows.append(("encode + append to /dev/null", clock(whole), int(sizes.sum())))
            wr.abort()
        enc.close()
        del out_t, sizes_t
    jenc = capi.JpegEncoder(w, h, Q, max_frames=n, device=0)
    j_out, j_slot, j_sizes = jenc.output()
    wr = capi.ZipWriter("/dev/null", device=0)

    def jpeg():
        if J.mdcj_encode_f32_device(jenc._h, d_frames.data_ptr(), npix, n, j_out, j_slot, j_sizes, None) != 0:
            raise RuntimeError(J.mdcj_last_error().decode())
        wr.append(j_out, j_slot, j_sizes, n, suffix=".jpg")

    jsizes = jenc.encode(d_frames.data_ptr(), n)[1]
    rows.append(("JPEG q95: encode + append", clock(jpeg), int(jsizes.sum())))
    wr.abort()
    jenc.close()
    pinned = capi.PinnedArray((n * npix,), np.float32)
    dst = torch.from_numpy(pinned.array)
    rows.append(("float frames to the host", clock(lambda: dst.copy_(d_frames)), n * npix * 4))
    print("%s: %d frames of %d x %d, %d timed repeats (median [min .. max])" % (name, n, w, h, reps))
    for label, (med, lo, hi), nbytes in rows:
        print("  %-30s: %9.3f ms [%9.3f .. %9.3f]  %8.1f MB out = %6.1f KB per frame, %6.2f GB/s of pixels"
              % (label, med, lo, hi, nbytes / 1e6, nbytes / n / 1e3, n * npix / med / 1e6))
    first = next(iter(sizes_by))
    ours = float(sizes_by[first][:16].mean())
    for level in (1, 6):
        t0 = time.perf_counter()
        total = 0
        for img in u8:
            buf = io.BytesIO()
            Image.fromarray(img).save(buf, "PNG", compress_level=level)
            total += buf.tell()
        ms = (time.perf_counter() - t0) * 1e3 / 16
        print("  PIL compress_level=%d, one thread: %7.2f ms per frame (%.0f ms per %d), %6.1f KB per frame; the device's files (%s) are %.2f x that"
              % (level, ms, ms * n, n, total / 16 / 1e3, first, ours / (total / 16)))


if "noise" in workloads:
    measure("noise (the synthetic sequence, rectified)", noise_frames())
    torch.cuda.empty_cache()
if "smooth" in workloads:
    measure("smooth (32 smooth frames, repeated)", smooth_frames())
