#!/usr/bin/env python3
"""Rate of the device PNG decoder with the parallel inflate (include/mdc_pngdx.h) on streams with matches, against the
wave-per-image inflate of include/mdc_pngd.h and against the host decoder.
  python tools/pngdx_rate.py [frames=256] [repeats=5] [dataset_frames=256]
(a) In one process, on `frames` files in HBM, of 640x480 and of 1280x1024, smooth frames (with three bits of noise: the camera-like
    case), clean frames (the same without the noise: what a rectified export looks like to an encoder, and where compress=lz77 takes
    its match form) and noise frames, in three stream kinds -- zlib level 6 (as PIL writes them), zlib level 1, this project's compress=lz77 files at chain 4:
      mdcx_decode_device   HIP events around the call and, by the library's own events, around its five stages
      mdci_decode_device   the same streams through libmdc_pngd.so: its general path, the yardstick
    The median of `repeats` calls after two warm-ups.  There are 16 different frames of each kind, repeated; every decoded frame is
    compared with its image.
(b) getImagesDevice (rectified, all corrections) over a zipped 1280x1024 dataset of `dataset_frames` frames, smooth and clean, PIL
    level 6 and compress=lz77, with MDC_GPU_PNG=0 (the host decoder on the CPUs the process may use: 16 on the measurement box), 2 and 3, each in
    a child process of its own: frames per second over `repeats` calls after one warm-up call.
One process per measurement, no retries: an error or a fault ends the run with a non-zero status."""
import io
import json
import os
import subprocess
import sys
import tempfile
import time
import zipfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

K = 16  # different frames of a kind


def frames_of(w, h, kind):
    from mono_dataset_code_amd import synth

    out = []
    for i in range(K):
        noise = synth.noise_frames(i, 1, w * h)[0].reshape(h, w)
        if kind == "noise":
            out.append(noise.astype(np.uint8))
            continue
        f = synth.smooth_frame(w, h, 0.3 + 0.37 * i, blobs=i % 3 == 0).reshape(h, w).astype(np.int32)
        if kind == "clean":
            out.append(f.astype(np.uint8))
            continue
        out.append(np.clip(f + (noise.astype(np.int32) & 7) - 3, 0, 255).astype(np.uint8))
    return out


def pil_png(img, level):
    from PIL import Image

    b = io.BytesIO()
    Image.fromarray(img).save(b, "PNG", compress_level=level)
    return b.getvalue()


def lz77_export(imgs):
    """the files of capi.PngEncoder(compress="lz77", chain=4), as bin/rectifyDataset frames=png compress=lz77 writes them"""
    import torch

    from mono_dataset_code_amd import capi

    h, w = imgs[0].shape
    enc = capi.PngEncoder(w, h, depth=8, filter=capi.PNG_FILTER_ADAPTIVE, max_images=len(imgs), device=0, compress="lz77", chain=4)
    d_in = torch.from_numpy(np.stack(imgs)).to("cuda:0")
    d_out = torch.zeros(len(imgs) * enc.bound, dtype=torch.uint8, device="cuda:0")
    d_sizes = torch.zeros(len(imgs), dtype=torch.int32, device="cuda:0")
    enc.encode(d_in.data_ptr(), len(imgs), d_out=d_out.data_ptr(), slot_bytes=enc.bound, d_sizes=d_sizes.data_ptr())
    torch.cuda.synchronize()
    sizes, host, bound = d_sizes.cpu().numpy(), d_out.cpu().numpy(), enc.bound
    enc.close()
    return [host[f * bound:f * bound + int(sizes[f])].tobytes() for f in range(len(imgs))]


def stream_kinds(imgs):
    """[(name, the K files)]"""
    return [("zlib level 6", [pil_png(img, 6) for img in imgs]), ("zlib level 1", [pil_png(img, 1) for img in imgs]), ("lz77 chain 4", lz77_export(imgs))]


def timed_calls(dec, args, n, d_frames, d_status, reps):
    import torch

    ms, kernels = [], []
    for r in range(reps + 2):
        d_frames.zero_()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dec.decode_device(args[0], args[1], args[2], n, d_frames.data_ptr(), d_status.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
        kernels.append(dec.kernel_ms())
    return float(np.median(ms[2:])), np.median(np.asarray(kernels[2:]), axis=0), ms[2:]


def part_a(n, reps):
    import torch

    from mono_dataset_code_amd import capi

    print("(a) mdcx_decode_device against mdci_decode_device, %d frames in HBM (%d different), median of %d calls after 2 warm-ups" % (n, K, reps))
    for w, h in ((640, 480), (1280, 1024)):
        decx = capi.PngDecoder(w, h, max_images=n, device=0, matches="parallel")
        deci = capi.PngDecoder(w, h, max_images=n, device=0)
        decx.profile(True)
        deci.profile(True)
        d_frames = torch.zeros((n, h, w), dtype=torch.uint8, device="cuda:0")
        d_status = torch.zeros(n, dtype=torch.int32, device="cuda:0")
        for kind in ("smooth", "clean", "noise"):
            imgs = frames_of(w, h, kind)
            want = torch.from_numpy(np.stack(imgs)).to("cuda:0")
            for name, files in stream_kinds(imgs):
                streams = [capi.png_stream(f)[2] for f in files]
                slot = (max(len(s) for s in streams) + 15) // 16 * 16
                host = np.zeros(n * slot, np.uint8)
                for i in range(n):
                    s = streams[i % K]
                    host[i * slot:i * slot + len(s)] = np.frombuffer(s, np.uint8)
                d_slots = torch.from_numpy(host).to("cuda:0")
                d_sizes = torch.tensor([len(streams[i % K]) for i in range(n)], dtype=torch.int32, device="cuda:0")
                args = (d_slots.data_ptr(), slot, d_sizes.data_ptr())
                res = {}
                for key, dec, names in (("mdcx", decx, capi.PNGDX_PATHS), ("mdci", deci, capi.PNGD_PATHS)):
                    t, km, runs = timed_calls(dec, args, n, d_frames, d_status, reps)
                    reasons, paths = capi.PngDecoder.status_fields(d_status.cpu().numpy())
                    assert not reasons.any(), (key, reasons)
                    assert all(bool((d_frames[i] == want[i % K]).all()) for i in range(n)), (key, name)
                    res[key] = (t, km, sorted({names[int(p)] for p in paths}), runs)
                tx, kx, px, rx = res["mdcx"]
                ti, ki, pi, ri = res["mdci"]
                print("  %4d x %4d %-6s %-12s %8.0f bytes per frame" % (w, h, kind, name, np.mean([len(s) for s in streams])))
                print("      mdcx %-22s %9.3f ms per call (%.3f .. %.3f), %8.0f frames/s: front %.3f, tokens %.3f, general %.3f, Adler-32 and checks %.3f, unfilter %.3f ms" %
                      (px, tx, min(rx), max(rx), n / tx * 1e3, kx[0], kx[1], kx[2], kx[3], kx[4]))
                print("      mdci %-22s %9.3f ms per call (%.3f .. %.3f), %8.0f frames/s: front %.3f, general %.3f, Adler-32 and checks %.3f, unfilter %.3f ms; mdcx is x %.2f" %
                      (pi, ti, min(ri), max(ri), n / ti * 1e3, ki[0], ki[1], ki[2], ki[3], ti / tx))
        decx.close()
        deci.close()


def write_dataset(folder, files):
    from mono_dataset_code_amd import synth

    synth.write_sequence_calibration(folder, n_times=len(files))
    with zipfile.ZipFile(os.path.join(folder, "images.zip"), "w", zipfile.ZIP_STORED) as z:
        for i, b in enumerate(files):
            z.writestr("%05d.png" % i, b)


def child(folder, reps):
    import torch

    from mono_dataset_code_amd import capi

    r = capi.DatasetReader(folder)
    n = len(r)
    d_base = torch.zeros((n, r.out_w * r.out_h), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    outs = capi.DeviceOutputs.make(d_base.data_ptr())
    times = []
    for k in range(reps + 1):
        t0 = time.perf_counter()
        valid, got = r.get_images_device(0, n, 1, 1, 1, 1, outs)
        times.append(time.perf_counter() - t0)
        assert got == n and valid.all(), r.last_error()
    print(json.dumps({"frames": n, "fps": n / float(np.median(times[1:])), "device_frames": r.png_device_frames() // (reps + 1)}))
    r.close()


def part_b(m, reps):
    w, h = 1280, 1024
    root = tempfile.mkdtemp(prefix="mdc_pngdx_rate_")
    print("(b) getImagesDevice, zipped dataset of %d PNG frames of %d x %d (%d different), rectified to 640 x 480, median of %d calls after 1 warm-up" %
          (m, w, h, K, reps))
    for kind in ("smooth", "clean"):
        imgs = frames_of(w, h, kind)
        sets = (("zlib level 6", os.path.join(root, kind + "_pil"), [pil_png(img, 6) for img in imgs]),
                ("lz77 chain 4", os.path.join(root, kind + "_lz77"), lz77_export(imgs)))
        for name, folder, files in sets:
            write_dataset(folder, [files[i % K] for i in range(m)])
            rates = {}
            for mode in ("0", "2", "3"):
                env = dict(os.environ, MDC_GPU_PNG=mode)
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", folder, str(reps)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                   text=True, timeout=900)
                if p.returncode != 0:
                    sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                    sys.exit(1)
                rates[mode] = json.loads(p.stdout.strip().splitlines()[-1])
            base = rates["0"]["fps"]
            for mode in ("0", "2", "3"):
                v = rates[mode]
                print("  %-6s %-12s %8.0f bytes per file  MDC_GPU_PNG=%s: %8.0f frames/s (x %.2f), %d of %d frames on the device decoder" %
                      (kind, name, np.mean([len(f) for f in files]), mode, v["fps"], v["fps"] / base, v["device_frames"], v["frames"]))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], int(sys.argv[3]))
        sys.exit(0)
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    reps = max(3, int(sys.argv[2])) if len(sys.argv) > 2 else 5
    m = int(sys.argv[3]) if len(sys.argv) > 3 else 256
    if n:
        part_a(n, reps)
    if m:
        part_b(m, reps)
