#!/usr/bin/env python3
"""Rate of the device PNG decoder (include/mdc_pngd.h) and of getImagesDevice on PNG datasets with and without it.
  python tools/pngd_rate.py [frames=1024] [repeats=5] [dataset_frames=512]
(a) mdci_decode_device on `frames` 640x480 files in HBM: HIP events around the call and, by the library's own events (mdci_profile),
    around each of its four kernels; the median of `repeats` runs after two warm-ups:
      own export     the files mdcp_encode_u8_device wrote, read where it left them (skip_head 41, skip_tail 16): the parallel path
      PIL level 6    the same frames written by PIL at compress_level=6 (their IDAT streams): the general path
    The frames are 64 different smooth frames with three bits of noise, repeated.  Every frame of both kinds is compared with its image.
(b) getImagesDevice (rectified, all corrections) over a zipped 1280x1024 dataset of `dataset_frames` PNG files of each kind, with
    MDC_GPU_PNG=0 (the host decoder: the path before the device decoder existed), 1 (the default) and 2 (every eligible stream), each
    in a child process of its own: frames per second over `repeats` calls after one warm-up call, and the frames the device decoder
    took.  The decode pool uses the CPUs the process may use (16 on the measurement box).
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


def frames_of(w, h, k):
    from mono_dataset_code_amd import synth

    out = []
    for i in range(k):
        f = synth.smooth_frame(w, h, 0.3 + 0.37 * i, blobs=i % 3 == 0).reshape(h, w).astype(np.int32)
        noise = synth.noise_frames(i, 1, w * h)[0].reshape(h, w).astype(np.int32)
        out.append(np.clip(f + (noise & 7) - 3, 0, 255).astype(np.uint8))
    return out


def pil_png(img):
    from PIL import Image

    b = io.BytesIO()
    Image.fromarray(img).save(b, "PNG", compress_level=6)
    return b.getvalue()


def own_export(imgs):
    """the device encoder's files of imgs -> (device tensor of slots, slot bytes, device tensor of sizes, the files)"""
    import torch

    from mono_dataset_code_amd import capi

    h, w = imgs[0].shape
    enc = capi.PngEncoder(w, h, depth=8, filter=capi.PNG_FILTER_ADAPTIVE, max_images=len(imgs), device=0)
    d_in = torch.from_numpy(np.stack(imgs)).to("cuda:0")
    d_out = torch.zeros(len(imgs) * enc.bound, dtype=torch.uint8, device="cuda:0")
    d_sizes = torch.zeros(len(imgs), dtype=torch.int32, device="cuda:0")
    enc.encode(d_in.data_ptr(), len(imgs), d_out=d_out.data_ptr(), slot_bytes=enc.bound, d_sizes=d_sizes.data_ptr())
    torch.cuda.synchronize()
    sizes = d_sizes.cpu().numpy()
    host = d_out.cpu().numpy()
    files = [host[f * enc.bound:f * enc.bound + int(sizes[f])].tobytes() for f in range(len(imgs))]
    slot = enc.bound
    enc.close()
    return d_out, slot, d_sizes, files


def part_a(n, reps):
    import torch

    from mono_dataset_code_amd import capi

    w, h, k = 640, 480, 64
    imgs = frames_of(w, h, k)
    want = torch.from_numpy(np.stack(imgs)).to("cuda:0")
    dec = capi.PngDecoder(w, h, max_images=n, device=0)
    dec.profile(True)
    d_frames = torch.zeros((n, h, w), dtype=torch.uint8, device="cuda:0")
    d_status = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    d_own, slot, d_sizes, own = own_export([imgs[i % k] for i in range(n)])
    streams = [capi.png_stream(pil_png(img))[2] for img in imgs]
    pslot = (max(len(s) for s in streams) + 15) // 16 * 16
    host = np.zeros(n * pslot, np.uint8)
    for i in range(n):
        s = streams[i % k]
        host[i * pslot:i * pslot + len(s)] = np.frombuffer(s, np.uint8)
    d_pil = torch.from_numpy(host).to("cuda:0")
    d_psizes = torch.tensor([len(streams[i % k]) for i in range(n)], dtype=torch.int32, device="cuda:0")
    print("(a) mdci_decode_device, %d frames of %d x %d in HBM, median of %d" % (n, w, h, reps))
    for name, args, mean in (("own export", (d_own.data_ptr(), slot, d_sizes.data_ptr(), 41, 16), np.mean([len(f) for f in own])),
                             ("PIL level 6", (d_pil.data_ptr(), pslot, d_psizes.data_ptr(), 0, 0), np.mean([len(s) for s in streams]))):
        ms, kernels = [], []
        for r in range(reps + 2):
            d_frames.zero_()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dec.decode_device(args[0], args[1], args[2], n, d_frames.data_ptr(), d_status.data_ptr(), skip_head=args[3], skip_tail=args[4],
                              stream=torch.cuda.current_stream().cuda_stream)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
            kernels.append(dec.kernel_ms())
        reasons, paths = capi.PngDecoder.status_fields(d_status.cpu().numpy())
        assert not reasons.any(), reasons
        assert all(bool((d_frames[i] == want[i % k]).all()) for i in range(n)), name
        t = float(np.median(ms[2:]))
        print("  %-12s %8.0f bytes per frame, paths %s: %8.3f ms per call, %9.0f frames/s, %6.2f GB/s of pixels" %
              (name, mean, sorted({capi.PNGD_PATHS[int(p)] for p in paths}), t, n / t * 1e3, n * w * h / t / 1e6))
        km = np.median(np.asarray(kernels[2:]), axis=0)
        print("  %-12s per kernel: front (header, parallel and stored paths) %.3f ms, wave-per-image inflate %.3f ms, Adler-32 and checks %.3f ms, unfilter %.3f ms" %
              ("", km[0], km[1], km[2], km[3]))
    dec.close()


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
    w, h, k = 1280, 1024, 32
    imgs = frames_of(w, h, k)
    root = tempfile.mkdtemp(prefix="mdc_pngd_rate_")
    own = own_export(imgs)[3]
    pil = [pil_png(img) for img in imgs]
    sets = (("own export", os.path.join(root, "own"), own), ("PIL level 6", os.path.join(root, "pil"), pil))
    print("(b) getImagesDevice, zipped dataset of %d PNG frames of %d x %d (%d different), rectified to 640 x 480, median of %d calls" % (m, w, h, k, reps))
    for name, folder, files in sets:
        write_dataset(folder, [files[i % k] for i in range(m)])
        rates = {}
        for mode in ("0", "1", "2"):
            env = dict(os.environ, MDC_GPU_PNG=mode)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", folder, str(reps)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                               timeout=900)
            if p.returncode != 0:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                sys.exit(1)
            rates[mode] = json.loads(p.stdout.strip().splitlines()[-1])
        base = rates["0"]["fps"]
        for mode in ("0", "1", "2"):
            v = rates[mode]
            print("  %-12s %8.0f bytes per file  MDC_GPU_PNG=%s: %8.0f frames/s (x %.2f), %d of %d frames on the device decoder" %
                  (name, np.mean([len(f) for f in files]), mode, v["fps"], v["fps"] / base, v["device_frames"], v["frames"]))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], int(sys.argv[3]))
        sys.exit(0)
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    reps = max(3, int(sys.argv[2])) if len(sys.argv) > 2 else 5
    m = int(sys.argv[3]) if len(sys.argv) > 3 else 512
    if n:
        part_a(n, reps)
    if m:
        part_b(m, reps)
