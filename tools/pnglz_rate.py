#!/usr/bin/env python3
"""Rate, file sizes and forms of the device PNG encoder with LZ77 matches (include/mdc_pnglz.h) beside the Huffman-only encoder
(include/mdc_pngw.h) and PIL, on tools/pngw_rate.py's workloads.
  python tools/pnglz_rate.py [frames=1024] [repeats=10] [workloads=noise,smooth] [chains=1,4,16,64]
Two workloads of `frames` rectified 640x480 float frames in HBM: "noise", the synthetic 1280x1024 sequence rectified, and "smooth",
32 different smooth 640x480 frames (synth.smooth_frame) repeated.  Reported per workload, each the median of `repeats` timed runs
after two warm-up runs, in one process:
  Huffman-only                 HIP events around mdcp_encode_f32_device (adaptive filter), bytes per file
  chain K                      HIP events around mdcl_encode_f32_device, bytes per file, the share of images per form, the ratio of
                               time and size to the Huffman-only encoder's, and the nine stages from the encoder's own events
                               (mdcl_profile / mdcl_kernel_ms; timed in runs of their own, not the ones the whole is taken from)
  PIL compress_level=6         Image.save of 16 of the frames on one host thread: bytes per file
Three files of every chain are decoded by PIL and compared with the converted frames before anything is timed.  One process, no
retries: an error or a fault ends the run with a non-zero status."""
import io
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

from mono_dataset_code_amd import capi, synth  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
reps = max(3, int(sys.argv[2])) if len(sys.argv) > 2 else 10
workloads = sys.argv[3].split(",") if len(sys.argv) > 3 else ["noise", "smooth"]
chains = [int(c) for c in sys.argv[4].split(",")] if len(sys.argv) > 4 else [1, 4, 16, 64]
W, H, w, h = 1280, 1024, 640, 480
npix = w * h
STAGES = ("filter", "order", "match", "parse", "tally", "build", "scan", "pack", "finish+crc")


def noise_frames():
    d = synth.write_sequence_calibration(tempfile.mkdtemp(prefix="mdc_pnglz_rate_"))
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


def measure(name, d_frames):
    host16 = d_frames[:16 * npix].cpu().numpy().reshape(16, h, w)
    with np.errstate(invalid="ignore"):
        u8 = np.where(np.isnan(host16), 0, np.clip(np.rint(host16), 0, 255)).astype(np.uint8)
    print("%s: %d frames of %d x %d, %d timed repeats (median [min .. max])" % (name, n, w, h, reps))
    base_ms = base_bytes = None
    for chain in [None] + chains:
        enc = capi.PngEncoder(w, h, depth=8, max_images=n, device=0, **({} if chain is None else {"compress": "lz77", "chain": chain}))
        slot = enc.bound
        out_t = torch.empty(n * slot, dtype=torch.uint8, device="cuda:0")
        sizes_t = torch.zeros(n, dtype=torch.int32, device="cuda:0")

        def encode():
            enc.encode(d_frames.data_ptr(), n, kind="f32", d_out=out_t.data_ptr(), slot_bytes=slot, d_sizes=sizes_t.data_ptr())

        encode()
        torch.cuda.synchronize()
        sizes = sizes_t.cpu().numpy()
        for i in (0, 7, 15):  # correctness before speed
            data = out_t[i * slot:i * slot + int(sizes[i])].cpu().numpy()
            if not np.array_equal(np.array(Image.open(io.BytesIO(data.tobytes()))), u8[i]):
                raise SystemExit("%s, chain %s: file %d does not decode to its frame" % (name, chain, i))
        med, lo, hi = events(encode)
        per_file = float(sizes.mean())
        if chain is None:
            base_ms, base_bytes = med, per_file
            print("  Huffman-only : %9.3f ms [%9.3f .. %9.3f]  %7.1f KB per file" % (med, lo, hi, per_file / 1e3))
        else:
            form_t = torch.zeros((n, 4), dtype=torch.int32, device="cuda:0")
            enc.form_device(form_t.data_ptr(), n)
            torch.cuda.synchronize()
            forms = form_t.cpu().numpy()
            share = [float((forms[:, 0] == f).mean()) for f in (0, 1, 2)]
            print("  chain %-2d     : %9.3f ms [%9.3f .. %9.3f]  %7.1f KB per file; stored %.3f, Huffman-only %.3f, matches %.3f of the images; "
                  "%.2f x the Huffman-only encoder's time, %.3f x its size; %.0f tokens, %.0f matches per image"
                  % (chain, med, lo, hi, per_file / 1e3, share[0], share[1], share[2], med / base_ms, per_file / base_bytes, forms[:, 1].mean(), forms[:, 2].mean()))
            enc.profile(True)
            per = []
            for k in range(reps + 2):
                encode()
                ms = enc.kernel_ms()
                if k >= 2:
                    per.append(ms)
            enc.profile(False)
            per = np.median(np.asarray(per), axis=0)
            print("               " + ", ".join("%s %.3f" % (s, v) for s, v in zip(STAGES, per)) + " ms (sum %.3f)" % per.sum())
        enc.close()
        del out_t, sizes_t
        torch.cuda.empty_cache()
    total = 0
    for img in u8:
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, "PNG", compress_level=6)
        total += buf.tell()
    print("  PIL compress_level=6 (16 of the frames): %7.1f KB per file" % (total / 16 / 1e3))


if "noise" in workloads:
    measure("noise (the synthetic sequence, rectified)", noise_frames())
    torch.cuda.empty_cache()
if "smooth" in workloads:
    measure("smooth (32 smooth frames, repeated)", smooth_frames())
