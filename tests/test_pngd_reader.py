"""getImagesDevice with the device PNG decoder behind it (csrc/host/batch_run.cpp: PngFrames; libmdc_pngd.so loaded at run time):
bit for bit what the same call gives with MDC_GPU_PNG=0, for the base, the levels, the gradient images and all 16 switch
combinations, with the same valid flags and error notes; frames the device decoder does not take or refuses go the way they went
before; the counter shows that the device decoder did take the eligible frames; a library that cannot be loaded means the host
decoder and the same results.  Each setting of the environment runs in a child process of its own (the variables are read when a
reader is made, the library is loaded once per process)."""
import hashlib
import io
import json
import os
import subprocess
import sys
import zipfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
W, H, N = 1280, 1024, 40  # the synthetic camera (synth.CAMERA_1280_TO_640): 1280 x 1024 frames rectified to 640 x 480


def SUB(n):
    """the frames of a sub-range call, from frame 3 on"""
    return min(n - 5, 12)


def frame(i):
    from mono_dataset_code_amd import synth

    f = synth.smooth_frame(W, H, 0.3 + 0.37 * i, blobs=i % 3 == 0).reshape(H, W).astype(np.int32)
    noise = synth.noise_frames(i, 1, W * H)[0].reshape(H, W).astype(np.int32)
    return np.clip(f + (noise & 7) - 3, 0, 255).astype(np.uint8)


def pil_png(img, **kw):
    from PIL import Image

    b = io.BytesIO()
    Image.fromarray(img).save(b, "PNG", **kw)
    return b.getvalue()


def write_dataset(folder, files, zipped):
    """files: [(name, bytes)]"""
    from mono_dataset_code_amd import synth

    synth.write_sequence_calibration(folder, n_times=len(files))
    if zipped:
        with zipfile.ZipFile(os.path.join(folder, "images.zip"), "w", zipfile.ZIP_STORED) as z:
            for n, b in files:
                z.writestr(n, b)
    else:
        os.makedirs(os.path.join(folder, "images"))
        for n, b in files:
            open(os.path.join(folder, "images", n), "wb").write(b)
    return folder


def device_export(imgs):
    """the device encoder's files of imgs (adaptive filter), as bin/rectifyDataset frames=png writes them"""
    import torch

    from mono_dataset_code_amd import capi

    enc = capi.PngEncoder(W, H, depth=8, filter=capi.PNG_FILTER_ADAPTIVE, max_images=len(imgs), device=0)
    d_in = torch.from_numpy(np.stack(imgs)).to("cuda:0")
    d_out = torch.zeros(len(imgs) * enc.bound, dtype=torch.uint8, device="cuda:0")
    d_sizes = torch.zeros(len(imgs), dtype=torch.int32, device="cuda:0")
    enc.encode(d_in.data_ptr(), len(imgs), d_out=d_out.data_ptr(), slot_bytes=enc.bound, d_sizes=d_sizes.data_ptr())
    torch.cuda.synchronize()
    sizes, host, bound = d_sizes.cpu().numpy(), d_out.cpu().numpy(), enc.bound
    enc.close()
    return [host[f * bound:f * bound + int(sizes[f])].tobytes() for f in range(len(imgs))]


def flip_in_the_stream(data, bit):
    """one bit of an IDAT body near the middle of the file flipped (the host decoder checks no chunk CRC: the stream is what is damaged)"""
    at, offsets = 0, []
    while True:
        at = data.find(b"IDAT", at + 1)
        if at < 0:
            break
        offsets.append(at)
    out = bytearray(data)
    out[offsets[len(offsets) // 2] + 1000] ^= bit
    return bytes(out)


def make_datasets(root):
    """own: the device encoder's files, zipped; pil: PIL's, a folder; mixed: both kinds with a JPEG, a 16-bit PNG, a PNG of another
    size and two PNGs with a flipped stream bit between them"""
    from PIL import Image

    imgs = [frame(i) for i in range(N)]
    own = device_export(imgs)
    assert all(f[43] & 7 == 5 for f in own)  # every one a single final dynamic block: the parallel path's form
    pil = [pil_png(img, compress_level=6) for img in imgs]
    write_dataset(os.path.join(root, "own"), [("%05d.png" % i, b) for i, b in enumerate(own)], True)
    write_dataset(os.path.join(root, "pil"), [("%05d.png" % i, b) for i, b in enumerate(pil)], False)
    b = io.BytesIO()
    Image.fromarray(imgs[2]).save(b, "JPEG", quality=92)
    deep = pil_png((imgs[3].astype(np.uint16) * 257))
    small = pil_png(imgs[4][:80, :100].copy())
    flipped, flipped_pil = flip_in_the_stream(own[5], 0x20), flip_in_the_stream(pil[6], 0x04)
    mixed = [("00000.png", own[0]), ("00001.png", pil[1]), ("00002.jpg", b.getvalue()), ("00003.png", deep), ("00004.png", small), ("00005.png", bytes(flipped)),
             ("00006.png", bytes(flipped_pil)), ("00007.png", own[7]), ("00008.png", own[8]), ("00009.png", pil[9]), ("00010.png", np.random.default_rng(1).bytes(300)),
             ("00011.png", own[11])]
    write_dataset(os.path.join(root, "mixed"), mixed, False)
    return {"own": N, "pil": N, "mixed": len(mixed)}


def child(root, out_path):
    """every call of the matrix on the three datasets -> {call: [sha256 of every output array, valid flags, produced, last error]}"""
    import torch

    from mono_dataset_code_amd import capi

    def digest(t):
        torch.cuda.synchronize()
        return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()

    result = {}
    for name in ("own", "pil", "mixed"):
        r = capi.DatasetReader(os.path.join(root, name))
        n, ow, oh = len(r), r.out_w, r.out_h
        # all 16 switch combinations on the own export; the whole range once, a sub-range (positions and frame ids differ) otherwise
        combos = [tuple((k >> b) & 1 for b in range(3, -1, -1)) for k in range(15, -1, -1)] if name == "own" else [(1, 1, 1, 1), (0, 1, 0, 0)]
        for fl in combos:
            first, count = (0, n) if fl == (1, 1, 1, 1) else (3, SUB(n))
            npo = ow * oh if fl[0] else W * H
            d_base = torch.full((count, npo), -3.0, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            valid, got = r.get_images_device(first, count, *fl, capi.DeviceOutputs.make(d_base.data_ptr()))
            result["%s base %s" % (name, fl)] = [digest(d_base), valid.tolist(), got, r.last_error()]
        for levels, grads in ((2, False), (3, False), (4, False), (4, True), (1, True)):
            dims = [(ow >> l, oh >> l) for l in range(levels)]
            m = SUB(n)
            d_base = torch.full((m, ow * oh), -3.0, dtype=torch.float32, device="cuda")
            d_lv = [torch.full((m, a * b), -3.0, dtype=torch.float32, device="cuda") for a, b in dims[1:]]
            d_dI = [torch.full((m, a * b * 3), -3.0, dtype=torch.float32, device="cuda") for a, b in dims] if grads else []
            d_ab = [torch.full((m, a * b), -3.0, dtype=torch.float32, device="cuda") for a, b in dims] if grads else []
            torch.cuda.synchronize()
            outs = capi.DeviceOutputs.make(d_base.data_ptr(), levels, [t.data_ptr() for t in d_lv], [t.data_ptr() for t in d_dI], [t.data_ptr() for t in d_ab])
            valid, got = r.get_images_device(3, m, 1, 1, 1, 1, outs)
            result["%s levels %d grads %d" % (name, levels, grads)] = [[digest(t) for t in [d_base] + d_lv + d_dI + d_ab], valid.tolist(), got, r.last_error()]
        result["%s device frames" % name] = r.png_device_frames()
        r.close()
    with open(out_path, "w") as f:
        json.dump(result, f)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """the datasets, and the matrix under each setting"""
    root = str(tmp_path_factory.mktemp("pngd_reader"))
    counts = make_datasets(root)
    out, children = {}, []
    for key, env in (("off", {"MDC_GPU_PNG": "0"}), ("all", {"MDC_GPU_PNG": "2"}), ("default", {}), ("absent", {"MDC_GPU_PNG": "2", "MDC_LIB_PNGD": os.path.join(root, "no_such_library.so")})):
        e = {k: v for k, v in os.environ.items() if k not in ("MDC_GPU_PNG", "MDC_LIB_PNGD")}
        e.update(env)
        path = os.path.join(root, key + ".json")
        children.append((key, path, subprocess.Popen([sys.executable, os.path.abspath(__file__), root, path], env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)))
    for key, path, p in children:  # the four run side by side: each is a reader of its own on the same files
        stdout, stderr = p.communicate(timeout=600)
        assert p.returncode == 0, (key, stdout[-2000:], stderr[-3000:])
        out[key] = (json.load(open(path)), stdout, stderr)
    return counts, out


def results_only(run):
    return {k: v for k, v in run.items() if not k.endswith("device frames")}


def test_results_equal_the_host_decoders_bit_for_bit(runs):
    counts, out = runs
    off = results_only(out["off"][0])
    assert len(off) == (16 + 5) + 2 * (2 + 5)
    for key in ("all", "default"):
        on = results_only(out[key][0])
        assert sorted(on) == sorted(off)
        for call in off:
            assert on[call] == off[call], (key, call, on[call][1:], off[call][1:])
    # what the host decoder makes of the three sets: every frame of own and pil; of mixed all but the wrong size, the two flipped ones and the noise
    for call, (digests, valid, got, err) in off.items():
        if call == "mixed base (1, 1, 1, 1)":
            assert valid == [True, True, True, True, False, False, False, True, True, True, False, True] and got == 8, (call, valid)
        elif call.startswith("mixed"):
            assert valid == [True, False, False, False, True, True, True] and got == 4, (call, valid)  # frames 3 .. 9
        else:
            assert all(valid) and got == len(valid), call


def test_the_device_decoder_took_the_eligible_frames(runs):
    """fails without the feature: the counter does not exist and nothing is decoded on the device"""
    counts, out = runs
    off, everything, default = out["off"][0], out["all"][0], out["default"][0]
    calls_own = N + (15 + 5) * SUB(N)
    calls_other = N + (1 + 5) * SUB(N)
    assert [off["%s device frames" % n] for n in ("own", "pil", "mixed")] == [0, 0, 0]
    assert everything["own device frames"] == calls_own  # every frame of every call
    assert everything["pil device frames"] == calls_other
    # mixed: frames 0, 1, 7, 8, 9, 11 are eligible and good (one call over all of them, six over frames 3 .. 9); 5 and 6 are eligible and refused
    assert everything["mixed device frames"] == 6 + 6 * 3
    # the default takes the classes that won the measurement: the encoder's own form always; zlib's streams only with MDC_GPU_PNG=2
    assert default["own device frames"] == calls_own
    assert default["pil device frames"] == 0  # zlib's streams lost the measurement and stay on the host


def test_a_missing_library_means_the_host_decoder_and_the_same_results(runs):
    counts, out = runs
    absent, stdout, stderr = out["absent"]
    assert results_only(absent) == results_only(out["off"][0])
    assert [absent["%s device frames" % n] for n in ("own", "pil", "mixed")] == [0, 0, 0]
    assert "no_such_library" not in stdout + stderr and "libmdc_pngd" not in stdout + stderr  # nothing is printed about it


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    child(sys.argv[1], sys.argv[2])
