"""The device JPEG encoder on the GPU (include/mdc_jenc.h, capi.JpegEncoder, bin/playDataset): every file equals the one
libjpeg-turbo writes through PIL for the same 8-bit pixels at the same quality, byte for byte -- no tolerance.  Shapes are
chosen where the encoder can go wrong (one block, the DC chain both ways, edge extension, a block count that is no multiple
of a wave or of the DCT kernel's group, one frame at the real size with several scan iterations), contents where the entropy
coder can (all-EOB blocks, both ends of the DC range, the largest AC amplitudes, ZRL runs, long codes and 0xFF bytes)."""
import os
import subprocess

import numpy as np
import pytest

import jenc_restatement as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERN, GUARD = 0xA5, 4096
_pil = {}


def pil_file(kind, w, h, index, quality):
    """the pin, computed once per case and shared"""
    key = (kind, w, h, index, quality)
    if key not in _pil:
        _pil[key] = R.pil_encode(R.to_u8(R.content(kind, w, h, index)), quality)
    return _pil[key]


def encode(frames, w, h, quality, u8=False, extra_stride=0, extra_slot=0, max_frames=None):
    """frames (each h x w) through capi.JpegEncoder into pattern-filled slots of the test's own -> the files; checks the sizes
    against the bound and every byte outside the files against the pattern."""
    import torch

    from mono_dataset_code_amd import capi

    n, stride = len(frames), w * h + extra_stride
    host = np.full((n, stride), np.nan if not u8 else 77, np.uint8 if u8 else np.float32)
    for i, f in enumerate(frames):
        host[i, :w * h] = np.asarray(f).reshape(-1)
    d_in = torch.from_numpy(host).to("cuda:0")
    enc = capi.JpegEncoder(w, h, quality, max_frames or n, device=0)
    assert enc.bound == R.bound(w, h)
    slot = enc.bound + extra_slot
    d_out = torch.full((n * slot + GUARD,), PATTERN, dtype=torch.uint8, device="cuda:0")
    d_sizes = torch.full((n + 16,), -77, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    p, sizes = enc.encode(d_in.data_ptr(), n, frame_stride=stride, u8=u8, d_out=d_out.data_ptr(), slot_bytes=slot, d_sizes=d_sizes.data_ptr())
    assert p == d_out.data_ptr()
    files = enc.files()
    enc.close()
    out, dsz = d_out.cpu().numpy(), d_sizes.cpu().numpy()
    assert (dsz[:n] == sizes).all() and (dsz[n:] == -77).all()
    assert (out[n * slot:] == PATTERN).all(), "guard region behind the last slot"
    for i in range(n):
        assert 0 < sizes[i] <= enc.bound, (i, sizes[i])
        assert (out[i * slot + sizes[i]:(i + 1) * slot] == PATTERN).all(), "slot %d written past its file" % i
        assert files[i] == out[i * slot:i * slot + sizes[i]].tobytes()
    return files


@pytest.mark.parametrize("quality", R.QUALITIES)
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "%dx%d" % s)
def test_every_content_equals_libjpeg(shape, quality):
    """one batch of all eight contents per shape and quality: each file == PIL's, float input"""
    w, h = shape
    files = encode([R.content(k, w, h) for k in R.CONTENTS], w, h, quality)
    for k, got in zip(R.CONTENTS, files):
        want = pil_file(k, w, h, 0, quality)
        assert got == want, (w, h, k, quality, len(got), len(want))
    if shape == (640, 480) and quality == 95:
        assert b"\xff\x00" in pil_file("noise", w, h, 0, 95)[328:-2]  # the stuffing path did run


@pytest.mark.parametrize("n", [1, 3, 65])
def test_batches_strides_and_the_8bit_entry(n):
    """frames of different content in one call: sizes differ, every slot is its own frame's file, a frame stride above w * h and a
    slot above the bound work, an encoder made for more frames than the call has works, and the 8-bit entry writes the same files"""
    w, h = 72, 40  # 45 blocks: two groups of the DCT kernel, no multiple of either
    kinds = [(R.CONTENTS[i % len(R.CONTENTS)], i) for i in range(n)]
    frames = [R.content(k, w, h, i) for k, i in kinds]
    want = [pil_file(k, w, h, i, 95) for k, i in kinds]
    got = encode(frames, w, h, 95, extra_stride=13, extra_slot=24, max_frames=n + 2)
    assert got == want
    if n > 1:
        assert len({len(g) for g in got}) > 1
    assert encode([R.to_u8(f) for f in frames], w, h, 95, u8=True, extra_stride=5) == want
    if n == 65:  # a slot does not depend on its neighbours: frame 40 alone
        assert encode(frames[40:41], w, h, 95) == want[40:41]


def test_round_trip_through_the_projects_decoders(tmp_path):
    """a file of the encoder through the host decoder (capi.decode_gray8) and through the device JPEG path
    (process_jpeg_streams_host): the pixels PIL decodes from PIL's file"""
    from mono_dataset_code_amd import capi, synth

    w, h = 320, 256
    frame = R.content("ramp", w, h) * 0.5 + R.content("noise", w, h) * 0.5
    ours = encode([frame], w, h, 95)[0]
    pixels = R.pil_decode(R.pil_encode(R.to_u8(frame), 95))
    assert np.array_equal(capi.decode_gray8(ours), pixels)
    d = synth.write_sequence_calibration(str(tmp_path), ("0.349153 0.436593 0.493140 0.499021 0.933271", "320 256", "crop", "192 144"), vignette_bits=16)
    fov = capi.UndistorterFOV(os.path.join(d, "camera.txt"))
    photo = capi.PhotometricUndistorter(os.path.join(d, "pcalib.txt"), os.path.join(d, "vignette.png"), w, h)
    ctx = capi.Context(0)
    ctx.bind(fov, photo)
    pin = capi.PinnedArray(((capi.JPEG_STREAM_HEADER_BYTES + len(ours) + 64 + 15) & ~15,), np.uint8)
    used = capi.jpeg_stream(ours, pin.array)[0]
    got, want = np.full(w * h, -7.0, np.float32), np.zeros(w * h, np.float32)
    assert ctx.process_jpeg_streams_host([pin.array], [used], [got], 7) == [0]
    ctx.process_host(np.ascontiguousarray(pixels.reshape(-1)), want, 7)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    ctx.close()


def test_argument_errors_launch_nothing():
    import torch

    from mono_dataset_code_amd import capi

    for args, code in (((8, 8, 0), capi.ERR_ARG), ((8, 8, 101), capi.ERR_ARG), ((0, 8, 95), capi.ERR_SIZE)):
        with pytest.raises(capi.MdcError) as e:
            capi.JpegEncoder(*args, max_frames=1, device=0)
        assert e.value.code == code and "mdcj_create" in str(e.value)
    w, h = 16, 8
    enc = capi.JpegEncoder(w, h, 95, max_frames=2, device=0)
    d_in = torch.zeros(3 * w * h, dtype=torch.float32, device="cuda:0")
    d_out = torch.full((3 * enc.bound,), PATTERN, dtype=torch.uint8, device="cuda:0")
    d_sizes = torch.full((3,), -77, dtype=torch.int32, device="cuda:0")
    for kw, code, word in ((dict(nframes=2, slot_bytes=enc.bound - 1), capi.ERR_SIZE, "slot_bytes"), (dict(nframes=3, slot_bytes=enc.bound), capi.ERR_ARG, "3 frames"),
                           (dict(nframes=2, slot_bytes=enc.bound, frame_stride=w * h - 1), capi.ERR_ARG, "frame_stride")):
        with pytest.raises(capi.MdcError) as e:
            enc.encode(d_in.data_ptr(), d_out=d_out.data_ptr(), d_sizes=d_sizes.data_ptr(), **kw)
        assert e.value.code == code and word in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == PATTERN).all() and (d_sizes.cpu().numpy() == -77).all()
    # the encoder is still good, and its own output arrays work
    p, sizes = enc.encode(d_in.data_ptr(), 2)
    assert enc.files() == [pil_file("zero", w, h, 0, 95)] * 2 and p == enc.output()[0]
    enc.close()


def test_play_dataset_saves_what_imwrite_would(tmp_path):
    """bin/playDataset <sequence> x in an empty directory: %05d.jpg of every frame == PIL's encoding of the rounded
    getImage(i, true, false, false, false) frame at quality 95; one undecodable frame is skipped with a message; the reader's
    lines on stdout are those of tests/dropin/playback_headless (where oracle/_ref has it) and the reference's header frames them."""
    from mono_dataset_code_amd import build, capi, synth

    d, out = str(tmp_path / "seq"), tmp_path / "out"
    out.mkdir()
    synth.write_sequence_calibration(d, ("0.349153 0.436593 0.493140 0.499021 0.933271", "320 256", "crop", "192 144"), vignette_bits=16, n_times=6)
    os.makedirs(os.path.join(d, "images"))
    for i in range(6):
        f = synth.noise_frames(11, 1, 320 * 256)[0] if i == 1 else synth.smooth_frame(320, 256, 0.7 + i, blobs=i % 2 == 0)
        synth.write_png_gray(os.path.join(d, "images", "%05d.png" % i), f.reshape(256, 320))
    with open(os.path.join(d, "images", "00004.png"), "wb") as f:  # five good frames and one the reader cannot decode
        f.write(b"not a png")
    r = subprocess.run([build.PLAY_DATASET, d, "x"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120, cwd=str(out))
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "no GPU context" not in r.stdout + r.stderr
    assert sorted(os.listdir(str(out))) == ["%05d.jpg" % i for i in (0, 1, 2, 3, 5)]
    reader = capi.DatasetReader(d)
    for i in (0, 1, 2, 3, 5):
        img = reader.get_image(i, 1, 0, 0, 0)[0]
        assert img.shape == (144, 192)
        assert (out / ("%05d.jpg" % i)).read_bytes() == R.pil_encode(R.to_u8(img), 95), i
    assert reader.get_image(4, 1, 0, 0, 0) is None
    reader.close()
    lines = r.stdout.splitlines()
    assert lines[0] == "Playback dataset %s!" % d
    at = lines.index("Rectified Images: 192 x 144. K:")
    assert [l.split() for l in lines[at + 1:at + 4]] == [["23.2996", "0", "88.0573"], ["0", "40.0524", "71.3648"], ["0", "0", "1"]]
    org = lines.index("Original Images: 320 x 256. omega=0.933271 K:")
    assert [l.split() for l in lines[org + 1:org + 4]] == [["111.729", "0", "157.305"], ["0", "111.768", "127.249"], ["0", "0", "1"]]
    sav = lines.index("Saving undistorted Dataset to here!")
    assert at < org < sav and any("frame 4 could not be read: skipped" in l for l in lines[sav:])
    headless = os.path.join(ROOT, "oracle", "_ref", "playback_mdc")
    if os.path.exists(headless):
        h = subprocess.run([headless, d, str(tmp_path / "h.bin"), "1000"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, timeout=120)
        hl = h.stdout.splitlines()
        assert hl[:[i for i, l in enumerate(hl) if l.startswith("PLAYBACK")][0]] == lines[1:at]
