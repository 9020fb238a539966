"""bin/rectifyDataset with compress=lz77 (include/mdc_pnglz.h behind the frames and vignette.png) beside the same command without it,
in one test: entry by entry equal pixels and no entry larger, an equal vignette, a folder that opens as a dataset whose frames on
the device are those of the Huffman-only export bit for bit; and the bad values, refused with one line and nothing created."""
import io
import os
import subprocess
import zipfile

import numpy as np
import pytest

from test_pngw_dataset import run, write_sequence

pytestmark = pytest.mark.gpu


def frames_on_the_device(folder):
    import torch

    from mono_dataset_code_amd import capi

    r = capi.DatasetReader(folder)
    n, npix = len(r), r.out_w * r.out_h
    d_base = torch.full((n, npix), -3.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    valid, got = r.get_images_device(0, n, 1, 1, 1, 1, capi.DeviceOutputs.make(d_base.data_ptr()))
    torch.cuda.synchronize()
    r.close()
    assert got == n and valid.all()
    return d_base.cpu().numpy()


def test_lz77_export_beside_the_huffman_export(tmp_path):
    from PIL import Image

    d = write_sequence(str(tmp_path / "seq"), "full")
    lz, plain = str(tmp_path / "lz"), str(tmp_path / "plain")
    stdout = run([d, lz, "frames=png", "vignette=1", "compress=lz77"], str(tmp_path))
    assert "LZ77 matches of depth 4" in stdout
    run([d, plain, "frames=png", "vignette=1"], str(tmp_path))
    assert sorted(os.listdir(lz)) == sorted(os.listdir(plain)) == ["camera.txt", "images.zip", "pcalib.txt", "times.txt", "vignette.png"]
    smaller = 0
    with zipfile.ZipFile(os.path.join(lz, "images.zip")) as a, zipfile.ZipFile(os.path.join(plain, "images.zip")) as b:
        assert a.testzip() is None and a.namelist() == b.namelist() == ["%05d.png" % i for i in range(7)]
        for name in a.namelist():
            x, y = a.read(name), b.read(name)
            assert np.array_equal(np.array(Image.open(io.BytesIO(x))), np.array(Image.open(io.BytesIO(y)))), name
            assert len(x) <= len(y), (name, len(x), len(y))
            smaller += len(x) < len(y)
            print(name, len(x), len(y))
    assert smaller >= 6  # every smooth frame inside its black border; frame 1 is noise
    va, vb = (open(os.path.join(f, "vignette.png"), "rb").read() for f in (lz, plain))
    assert np.array_equal(np.array(Image.open(io.BytesIO(va))), np.array(Image.open(io.BytesIO(vb)))) and len(va) < len(vb)
    for name in ("camera.txt", "pcalib.txt", "times.txt"):
        assert open(os.path.join(lz, name), "rb").read() == open(os.path.join(plain, name), "rb").read(), name
    got, want = frames_on_the_device(lz), frames_on_the_device(plain)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # chain=1 is another depth: still the same pixels
    c1 = str(tmp_path / "c1")
    run([d, c1, "compress=lz77", "chain=1", "frames=png"], str(tmp_path))
    with zipfile.ZipFile(os.path.join(c1, "images.zip")) as a, zipfile.ZipFile(os.path.join(plain, "images.zip")) as b:
        for name in a.namelist():
            assert np.array_equal(np.array(Image.open(io.BytesIO(a.read(name)))), np.array(Image.open(io.BytesIO(b.read(name))))), name
            assert len(a.read(name)) <= len(b.read(name))


def test_bad_values_are_refused_with_one_line_and_nothing_created(tmp_path):
    from mono_dataset_code_amd import build

    for bad in (["compress=gzip"], ["compress=lz77", "frames=png", "chain=0"], ["compress=lz77", "frames=png", "chain=65"], ["compress=lz77", "frames=jpg"]):
        r = subprocess.run([build.RECTIFY_DATASET, str(tmp_path / "seq"), str(tmp_path / "out")] + bad, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                           timeout=60, cwd=str(tmp_path))
        assert r.returncode != 0 and r.stdout == "" and len(r.stderr.splitlines()) == 1, (bad, r.stderr)
        assert ("chain" if "chain" in bad[-1] else "compress") in r.stderr
    assert os.listdir(str(tmp_path)) == []
