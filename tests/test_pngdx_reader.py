"""getImagesDevice with MDC_GPU_PNG=3: every PNG class goes to libmdc_pngdx.so (include/mdc_pngdx.h), loaded at run time like
libmdc_pngd.so.  Bit for bit what the same calls give with MDC_GPU_PNG=0, for the base, the levels and the gradient images, with
the same valid flags and error notes, on a dataset PIL wrote (zlib level 6) and on one exported with compress=lz77; the counter
shows that the device decoder took every frame; a damaged file goes the host decoder's way; a library that cannot be loaded means
the host decoder and the same results; the default and the modes 1 and 2 count what they counted before.  Each setting of the
environment runs in a child process of its own, as in tests/test_pngd_reader.py."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import pngd_restatement as R
from test_pngd_reader import H, W, flip_in_the_stream, pil_png, write_dataset

pytestmark = pytest.mark.gpu
N, FIRST, M = 12, 3, 8  # frames per dataset; the sub-range calls take M frames from FIRST on
DAMAGED = 5
SETS = ("pil", "lz77", "damaged")


def frame(i):
    from mono_dataset_code_amd import synth

    return np.clip(synth.smooth_frame(W, H, 0.3 + 0.37 * i, blobs=i % 3 == 0).reshape(H, W), 0, 255).astype(np.uint8)


def lz77_export(imgs):
    """the files of bin/rectifyDataset frames=png compress=lz77 (chain 4, adaptive filter)"""
    import torch

    from mono_dataset_code_amd import capi

    enc = capi.PngEncoder(W, H, depth=8, filter=capi.PNG_FILTER_ADAPTIVE, max_images=len(imgs), device=0, compress="lz77", chain=4)
    d_in = torch.from_numpy(np.stack(imgs)).to("cuda:0")
    d_out = torch.zeros(len(imgs) * enc.bound, dtype=torch.uint8, device="cuda:0")
    d_sizes = torch.zeros(len(imgs), dtype=torch.int32, device="cuda:0")
    enc.encode(d_in.data_ptr(), len(imgs), d_out=d_out.data_ptr(), slot_bytes=enc.bound, d_sizes=d_sizes.data_ptr())
    torch.cuda.synchronize()
    sizes, host, bound = d_sizes.cpu().numpy(), d_out.cpu().numpy(), enc.bound
    enc.close()
    return [host[f * bound:f * bound + int(sizes[f])].tobytes() for f in range(len(imgs))]


def make_datasets(root):
    """-> {set: [the class of every file's stream: R.PARALLEL, R.STORED, R.GENERAL, or None for the damaged file]}"""
    imgs = [frame(i) for i in range(N)]
    pil = [pil_png(img, compress_level=6) for img in imgs]
    lz = lz77_export(imgs)
    damaged = list(pil)
    damaged[DAMAGED] = flip_in_the_stream(pil[DAMAGED], 0x04)
    classes = {}
    for name, files in zip(SETS, (pil, lz, damaged)):
        write_dataset(os.path.join(root, name), [("%05d.png" % i, b) for i, b in enumerate(files)], name == "lz77")
        streams = [R.png_stream(b)[2] for b in files]
        classes[name] = [R.first_path(s, H * (1 + W)) for s in streams]
    classes["damaged"][DAMAGED] = None
    assert set(classes["pil"]) == {R.GENERAL}  # zlib's streams: matches
    assert classes["lz77"].count(R.GENERAL) >= N // 2  # the match form (a frame on which it gains nothing keeps the Huffman-only form)
    assert not R.host_accepts(R.png_stream(damaged[DAMAGED])[2], W, H)
    return classes


def child(root, out_path):
    """every call on the three datasets -> {call: [sha256 of every output array, valid flags, produced, last error]}"""
    import torch

    from mono_dataset_code_amd import capi

    def digest(t):
        torch.cuda.synchronize()
        return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()

    result = {}
    for name in SETS:
        r = capi.DatasetReader(os.path.join(root, name))
        n, ow, oh = len(r), r.out_w, r.out_h
        for fl in ((1, 1, 1, 1), (0, 1, 0, 0)):
            first, count = (0, n) if fl == (1, 1, 1, 1) else (FIRST, M)
            npo = ow * oh if fl[0] else W * H
            d_base = torch.full((count, npo), -3.0, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            valid, got = r.get_images_device(first, count, *fl, capi.DeviceOutputs.make(d_base.data_ptr()))
            result["%s base %s" % (name, fl)] = [digest(d_base), valid.tolist(), got, r.last_error()]
        for levels, grads in ((3, False), (4, True)):
            dims = [(ow >> l, oh >> l) for l in range(levels)]
            d_base = torch.full((M, ow * oh), -3.0, dtype=torch.float32, device="cuda")
            d_lv = [torch.full((M, a * b), -3.0, dtype=torch.float32, device="cuda") for a, b in dims[1:]]
            d_dI = [torch.full((M, a * b * 3), -3.0, dtype=torch.float32, device="cuda") for a, b in dims] if grads else []
            d_ab = [torch.full((M, a * b), -3.0, dtype=torch.float32, device="cuda") for a, b in dims] if grads else []
            torch.cuda.synchronize()
            outs = capi.DeviceOutputs.make(d_base.data_ptr(), levels, [t.data_ptr() for t in d_lv], [t.data_ptr() for t in d_dI], [t.data_ptr() for t in d_ab])
            valid, got = r.get_images_device(FIRST, M, 1, 1, 1, 1, outs)
            result["%s levels %d grads %d" % (name, levels, grads)] = [[digest(t) for t in [d_base] + d_lv + d_dI + d_ab], valid.tolist(), got, r.last_error()]
        result["%s device frames" % name] = r.png_device_frames()
        r.close()
    with open(out_path, "w") as f:
        json.dump(result, f)


SETTINGS = (("off", {"MDC_GPU_PNG": "0"}), ("tokens", {"MDC_GPU_PNG": "3"}), ("default", {}), ("one", {"MDC_GPU_PNG": "1"}), ("two", {"MDC_GPU_PNG": "2"}),
            ("absent", {"MDC_GPU_PNG": "3", "MDC_LIB_PNGDX": "no_such_library.so"}))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """the datasets, and the calls under each setting"""
    root = str(tmp_path_factory.mktemp("pngdx_reader"))
    classes = make_datasets(root)
    out, children = {}, []
    for key, env in SETTINGS:
        e = {k: v for k, v in os.environ.items() if k not in ("MDC_GPU_PNG", "MDC_LIB_PNGD", "MDC_LIB_PNGDX")}
        e.update({k: os.path.join(root, v) if k == "MDC_LIB_PNGDX" else v for k, v in env.items()})
        path = os.path.join(root, key + ".json")
        children.append((key, path, subprocess.Popen([sys.executable, os.path.abspath(__file__), root, path], env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)))
    for key, path, p in children:  # side by side: each is a reader of its own on the same files
        stdout, stderr = p.communicate(timeout=600)
        assert p.returncode == 0, (key, stdout[-2000:], stderr[-3000:])
        out[key] = (json.load(open(path)), stdout, stderr)
    return classes, out


def results_only(run):
    return {k: v for k, v in run.items() if not k.endswith("device frames")}


def counted(classes, taken):
    """the counter after child()'s calls when the device decodes the frames whose class is in `taken`: one call over all frames,
    three over the sub-range"""
    sub = classes[FIRST:FIRST + M]
    return sum(1 for c in classes if c in taken) + 3 * sum(1 for c in sub if c in taken)


def test_mode_3_equals_the_host_decoder_bit_for_bit(runs):
    classes, out = runs
    off = results_only(out["off"][0])
    assert len(off) == 3 * 4
    for key in ("tokens", "default", "one", "two"):
        on = results_only(out[key][0])
        assert sorted(on) == sorted(off)
        for call in off:
            assert on[call] == off[call], (key, call, on[call][1:], off[call][1:])  # digests, valid flags, produced, lastError()
    for call, (digests, valid, got, err) in off.items():
        if call.startswith("damaged"):
            bad = DAMAGED if "(1, 1, 1, 1)" in call and "base" in call else DAMAGED - FIRST
            assert valid == [i != bad for i in range(len(valid))] and got == len(valid) - 1 and err, (call, valid)
        else:
            assert all(valid) and got == len(valid), call


def test_mode_3_sends_every_frame_to_the_device(runs):
    """fails without the feature: mode 3 is clamped to 2 there, and zlib's streams take the wave-per-image path of libmdc_pngd.so --
    the counters of mode 2 are the same, so the library in use is shown by the run with MDC_LIB_PNGDX pointing nowhere"""
    classes, out = runs
    everything = (R.PARALLEL, R.STORED, R.GENERAL)
    tokens, absent = out["tokens"][0], out["absent"][0]
    for name in SETS:
        assert tokens["%s device frames" % name] == counted(classes[name], everything) > 0, name  # (the damaged file is refused: host)
        assert absent["%s device frames" % name] == 0, name
    assert tokens["pil device frames"] == N + 3 * M and tokens["damaged device frames"] == N - 1 + 3 * (M - 1)


def test_a_missing_library_means_the_host_decoder_and_the_same_results(runs):
    classes, out = runs
    absent, stdout, stderr = out["absent"]
    assert results_only(absent) == results_only(out["off"][0])
    assert "no_such_library" not in stdout + stderr and "libmdc_pngdx" not in stdout + stderr  # nothing is printed about it


def test_the_default_and_modes_1_and_2_count_what_they_counted(runs):
    classes, out = runs
    for name in SETS:
        assert out["off"][0]["%s device frames" % name] == 0
        assert out["two"][0]["%s device frames" % name] == counted(classes[name], (R.PARALLEL, R.STORED, R.GENERAL)), name
        for key in ("default", "one"):  # the Huffman-only form alone
            assert out[key][0]["%s device frames" % name] == counted(classes[name], (R.PARALLEL,)), (key, name)
    assert out["default"][0]["pil device frames"] == 0  # zlib's streams stay on the host unless asked for


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    child(sys.argv[1], sys.argv[2])
