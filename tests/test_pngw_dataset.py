"""bin/rectifyDataset with frames=png and vignette=1 (include/mdc_pngw.h behind both): the archive's PNG entries are the rectified
frames without loss, the folder opens as a dataset with a valid vignette, vignette.png is the map the program's header comment
defines, the default run is what it was, and a source without a vignette is said to have none."""
import io
import os
import shutil
import subprocess
import zipfile

import numpy as np
import pytest

import pngw_restatement as P

pytestmark = pytest.mark.gpu
CAMERAS = {"crop": ("0.349153 0.436593 0.493140 0.499021 0.933271", "320 256", "crop", "192 144"),
           "full": ("0.349153 0.436593 0.493140 0.499021 0.933271", "320 256", "full", "192 144")}
NOT_EXPORTED = "vignette.png is not exported (a rectified vignette is out of scope): the dataset opens without a vignette."


def write_sequence(folder, camera):
    from mono_dataset_code_amd import synth

    synth.write_sequence_calibration(folder, CAMERAS[camera], vignette_bits=16, n_times=7)
    os.makedirs(os.path.join(folder, "images"))
    for i in range(7):
        f = synth.noise_frames(11, 1, 320 * 256)[0] if i == 1 else synth.smooth_frame(320, 256, 0.7 + i, blobs=i % 2 == 0)
        synth.write_png_gray(os.path.join(folder, "images", "%05d.png" % i), f.reshape(256, 320))
    return folder


def run(args, cwd):
    from mono_dataset_code_amd import build

    r = subprocess.run([build.RECTIFY_DATASET] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120, cwd=cwd)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout


def expected_vignette(d):
    """the definition, from the source's normalised map and the host-side undistort<float> -> (uint16 image, the black mask)"""
    from mono_dataset_code_amd import capi

    photo = capi.PhotometricUndistorter(os.path.join(d, "pcalib.txt"), os.path.join(d, "vignette.png"), 320, 256)
    assert photo.valid() & 2
    V = photo.vignette()[0]
    photo.close()
    fov = capi.UndistorterFOV(os.path.join(d, "camera.txt"))
    R = np.zeros(192 * 144, np.float32)
    fov.undistort(V, R)
    black = (fov.remap()[0] == -1).reshape(144, 192)
    fov.close()
    good = np.isfinite(R) & (R > 0)
    m = R[good].max()
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.clip(np.rint(R / m * np.float32(65535)), 1, 65535)
    return np.where(good, q, 65535).astype(np.uint16).reshape(144, 192), black


@pytest.mark.parametrize("camera", ["crop", "full"])
def test_png_frames_and_vignette(tmp_path, camera):
    from PIL import Image

    from mono_dataset_code_amd import capi

    d, out = write_sequence(str(tmp_path / "seq"), camera), str(tmp_path / "rect")
    stdout = run([d, out, "frames=png", "vignette=1"], str(tmp_path))
    assert "(PNG, 8-bit, lossless)" in stdout and "JPEG" not in stdout and "not exported" not in stdout
    assert sorted(os.listdir(out)) == ["camera.txt", "images.zip", "pcalib.txt", "times.txt", "vignette.png"]
    src = capi.DatasetReader(d)
    want = [P.f32_to_u8(src.get_image(i, True, False, False, False)[0]) for i in range(7)]
    src.close()
    assert want[0].shape == (144, 192)
    with zipfile.ZipFile(os.path.join(out, "images.zip")) as z:
        assert z.testzip() is None
        assert z.namelist() == ["%05d.png" % i for i in range(7)]
        members = [z.read(n) for n in z.namelist()]
    for i, m in enumerate(members):
        img = Image.open(io.BytesIO(m))
        assert img.mode == "L" and np.array_equal(np.array(img), want[i]), i
        assert m == P.encode(want[i], 8, P.ADAPTIVE)[0], i
    reader = capi.DatasetReader(out)  # the lossless claim: the exported dataset's raw frames are the rectified frames
    assert len(reader) == 7 and (reader.in_w, reader.in_h) == (192, 144)
    for j in range(7):
        raw = reader.get_raw(j)
        assert raw is not None, reader.last_error()
        assert np.array_equal(raw, want[j]), j
    reader.close()
    # vignette.png: 16-bit, the definition, 65535 exactly where the remap is -1
    png = open(os.path.join(out, "vignette.png"), "rb").read()
    img = Image.open(io.BytesIO(png))
    got = np.array(img)
    assert img.size == (192, 144) and png[24] == 16 and got.dtype == np.uint16
    exp, black = expected_vignette(d)
    assert np.array_equal(got, exp), int((got != exp).sum())
    assert (got[black] == 65535).all() and got.min() >= 1 and got.max() == 65535
    if camera == "full":
        assert black.any() and not black.all()
        assert np.array_equal(got == 65535, black | (exp == 65535)) and (exp[~black] == 65535).sum() <= 4  # the maximum itself, nothing else
    assert png == P.encode(exp, 16, P.ADAPTIVE)[0]
    photo = capi.PhotometricUndistorter(os.path.join(out, "pcalib.txt"), os.path.join(out, "vignette.png"), 192, 144)
    assert photo.valid() == 3  # validGamma and validVignette, as the reader of the exported folder finds them
    vmap, vinv = photo.vignette()
    assert vmap.max() == 1 and vmap.min() > 0 and np.isfinite(vinv).all()
    photo.close()
    assert "vignette.png: 192 x 144, 16-bit, %d bytes, %d border pixels at 65535" % (len(png), int(black.sum())) in stdout


def test_default_run_is_unchanged_and_a_missing_vignette_is_said(tmp_path):
    d, out, out2 = write_sequence(str(tmp_path / "seq"), "crop"), str(tmp_path / "plain"), str(tmp_path / "none")
    stdout = run([d, out], str(tmp_path))
    assert sorted(os.listdir(out)) == ["camera.txt", "images.zip", "pcalib.txt", "times.txt"]
    lines = stdout.splitlines()
    assert "Rectifying %s/: 7 frames of 192 x 144 into %s (JPEG quality 95)" % (d, out) in lines
    assert lines[-1] == NOT_EXPORTED and len([l for l in lines if "not exported" in l]) == 1
    size = os.path.getsize(os.path.join(out, "images.zip"))
    assert lines[-2] == "images.zip: 7 frames, %d bytes" % size
    with zipfile.ZipFile(os.path.join(out, "images.zip")) as z:
        assert z.namelist() == ["%05d.jpg" % i for i in range(7)]
        assert z.read("00000.jpg")[:2] == b"\xff\xd8"
    # the same with the arguments spelt out, in another order: the same files
    out3 = str(tmp_path / "spelt")
    run([d, out3, "vignette=0", "95", "frames=jpg"], str(tmp_path))
    for name in os.listdir(out):
        assert open(os.path.join(out, name), "rb").read() == open(os.path.join(out3, name), "rb").read(), name
    # no vignette in the source: nothing written, one line, status 0
    os.remove(os.path.join(d, "vignette.png"))
    stdout = run([d, out2, "vignette=1"], str(tmp_path))
    assert sorted(os.listdir(out2)) == ["camera.txt", "images.zip", "pcalib.txt", "times.txt"]
    assert len([l for l in stdout.splitlines() if "nothing written" in l]) == 1 and "not exported" not in stdout
    assert "vignette.png: the source has no valid vignette: nothing written" in stdout.splitlines()
    shutil.rmtree(out2)
