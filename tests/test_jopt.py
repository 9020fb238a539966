"""The device JPEG encoder with per-frame optimal Huffman tables on the GPU (include/mdc_jopt.h, capi.JpegEncoder(huffman="optimal"),
bin/rectifyDataset huffman=optimal): every file equals the one libjpeg-turbo writes with optimize_coding through PIL for the same 8-bit
pixels at the same quality, and the restatement's, byte for byte -- no tolerance."""
import io
import os
import subprocess
import zipfile

import numpy as np
import pytest

import jenc_restatement as R
import jopt_device as D
import jopt_problems as J
import jopt_restatement as O

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("quality", R.QUALITIES)
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "%dx%d" % s)
def test_every_content_equals_libjpeg_optimize(shape, quality):
    """one batch of all eight contents per shape and quality, through the float and through the 8-bit entry"""
    w, h = shape
    frames = [R.content(k, w, h) for k in R.CONTENTS]
    want = [D.pil(k, w, h, 0, quality) for k in R.CONTENTS]
    assert want == [O.encode_f32(f, quality) for f in frames]
    enc = D.encoder(w, h, quality, max_frames=len(frames))
    for batch in (frames, [R.to_u8(f) for f in frames]):
        got = D.run(enc, batch)
        for k, g, x in zip(R.CONTENTS, got, want):
            assert g == x, (w, h, k, quality, len(g), len(x))
    enc.close()


@pytest.mark.parametrize("shape", [(13, 21), (64, 48)], ids=lambda s: "%dx%d" % s)
def test_different_tables_in_one_batch(shape):
    """13 frames of different content: frame f's tables come from frame f alone; a frame stride above w * h, a slot above the
    bound, input and output bases that are not aligned, an encoder made for more frames than the call has"""
    w, h = shape
    frames = J.thirteen(w, h)
    want = [O.pil_encode(R.to_u8(f), 95) for f in frames]
    assert len({tuple(O.dht_segments(x)) for x in want}) >= 2
    enc = D.encoder(w, h, 95, max_frames=16)
    assert D.run(enc, frames, extra_stride=13, extra_slot=23, offset=3, out_offset=5) == want
    assert D.run(enc, [R.to_u8(f) for f in frames], extra_stride=5, extra_slot=1, offset=1, out_offset=3) == want
    assert D.run(enc, frames[7:8]) == want[7:8]  # a slot does not depend on its neighbours
    assert D.run(enc, frames[::-1]) == want[::-1]
    enc.close()


def test_reuse_without_residue():
    """one encoder: a rich frame, a flat one, the rich one again -- histograms, tables and DHT segments of a call hold the call before"""
    w, h = 72, 40
    rich, flat = R.content("noise", w, h), R.content("mid", w, h)
    want_rich, want_flat = D.pil("noise", w, h, 0, 95), D.pil("mid", w, h, 0, 95)
    assert [len(x) for x in O.dht_segments(want_flat)] == [22, 22] and len(O.dht_segments(want_rich)[1]) >= 21 + 16
    enc = D.encoder(w, h, 95, max_frames=2)
    for frames, want in (([rich], [want_rich]), ([flat], [want_flat]), ([rich], [want_rich]), ([flat, rich], [want_flat, want_rich]), ([rich, flat], [want_rich, want_flat])):
        assert D.run(enc, frames) == want
    enc.close()


def test_optimal_tables_device_on_the_directed_histograms():
    """mdcjo_optimal_tables_device == the restatement on every directed histogram, status 1 (deeper than 32) included; nothing is
    written outside the tables' rows.  (No histogram can be injected into an encode call, so the fallback to the Annex K tables of a
    frame with such a table is not run here: no frame reaches that depth, and the tables call is what shows the status.)"""
    named = J.histograms()
    freq = np.stack([f for _, f in named]).astype(np.uint32)
    freq[:, 256] = 0xFFFFFFFF  # ignored
    enc = D.encoder(8, 8, 95)
    bits, vals, nvals, status = enc.optimal_tables(freq)
    for i, (name, f) in enumerate(named):
        s, b, v, n = J.expected_table(f)
        assert (int(status[i]), bits[i].tolist(), vals[i].tolist(), int(nvals[i])) == (s, b, v, n), name
    assert status.tolist().count(1) == 1 and dict(zip([n for n, _ in named], status.tolist()))["deeper_than_32"] == 1
    # the same histogram many times over, in one call: every wave gives the same table
    again = enc.optimal_tables(np.repeat(freq[11:12], 300, axis=0))
    assert all((a == a[0]).all() for a in again) and again[0][0].tolist() == bits[11].tolist()
    enc.close()


def test_round_trip_through_the_projects_decoders(tmp_path):
    """files with per-frame tables through the host decoder (capi.decode_gray8) and through the device JPEG path
    (process_jpeg_streams_host): the pixels of the standard-table files of the same frames"""
    from mono_dataset_code_amd import capi, synth

    w, h = 320, 256
    frame = R.content("ramp", w, h) * 0.5 + R.content("noise", w, h) * 0.5
    ours = D.once(R.to_u8(frame), 95)
    standard = R.pil_encode(R.to_u8(frame), 95)
    assert ours == O.pil_encode(R.to_u8(frame), 95) and len(ours) < len(standard)
    pixels = R.pil_decode(standard)
    assert np.array_equal(capi.decode_gray8(ours), pixels) and np.array_equal(capi.decode_gray8(ours), capi.decode_gray8(standard))
    d = synth.write_sequence_calibration(str(tmp_path), ("0.349153 0.436593 0.493140 0.499021 0.933271", "320 256", "crop", "192 144"), vignette_bits=16)
    fov = capi.UndistorterFOV(os.path.join(d, "camera.txt"))
    photo = capi.PhotometricUndistorter(os.path.join(d, "pcalib.txt"), os.path.join(d, "vignette.png"), w, h)
    ctx = capi.Context(0)
    ctx.bind(fov, photo)
    results = []
    for data in (ours, standard):
        pin = capi.PinnedArray(((capi.JPEG_STREAM_HEADER_BYTES + len(data) + 64 + 15) & ~15,), np.uint8)
        used = capi.jpeg_stream(data, pin.array)[0]
        got = np.full(w * h, -7.0, np.float32)
        assert ctx.process_jpeg_streams_host([pin.array], [used], [got], 7) == [0]
        results.append(got)
    want = np.zeros(w * h, np.float32)
    ctx.process_host(np.ascontiguousarray(pixels.reshape(-1)), want, 7)
    assert np.array_equal(results[0].view(np.uint32), want.view(np.uint32)) and np.array_equal(results[0].view(np.uint32), results[1].view(np.uint32))
    ctx.close()


def test_jpeg_encoder_selects_the_library():
    """capi.JpegEncoder(huffman="optimal") returns the bytes of the raw mdcjo_ calls; huffman="standard", and no argument, today's"""
    import torch

    from mono_dataset_code_amd import capi

    w, h = 72, 40
    frames = [R.content(k, w, h) for k in ("noise", "ramp", "mid")]
    d_in = torch.from_numpy(np.stack([f.reshape(-1) for f in frames])).to("cuda:0")
    raw = D.run(D.encoder(w, h, 95, max_frames=3), frames)
    files = {}
    for name, kw in (("optimal", dict(huffman="optimal")), ("standard", dict(huffman="standard")), ("default", {})):
        enc = capi.JpegEncoder(w, h, 95, max_frames=3, device=0, **kw)
        p, sizes = enc.encode(d_in.data_ptr(), 3)
        files[name] = enc.files()
        assert p == enc.output()[0] and enc.output()[1] == enc.bound and [len(f) for f in files[name]] == sizes.tolist()
        assert enc.bound == (O.bound(w, h) if name == "optimal" else R.bound(w, h))
        if name != "optimal":
            with pytest.raises(capi.MdcError):
                enc.optimal_tables(np.zeros((1, 257), np.uint32))
        enc.close()
    assert files["optimal"] == raw == [O.pil_encode(R.to_u8(f), 95) for f in frames]
    assert files["standard"] == files["default"] == [R.pil_encode(R.to_u8(f), 95) for f in frames]
    with pytest.raises(capi.MdcError) as e:
        capi.JpegEncoder(0, 8, 95, device=0, huffman="optimal")
    assert e.value.code == capi.ERR_SIZE and "mdcjo_create" in str(e.value)


def test_argument_errors_launch_nothing():
    import torch

    from mono_dataset_code_amd import capi

    w, h = 16, 8
    enc = D.encoder(w, h, 95, max_frames=2)
    d_in = torch.zeros(3 * w * h, dtype=torch.float32, device="cuda:0")
    d_out = torch.full((3 * enc.bound,), D.PATTERN, dtype=torch.uint8, device="cuda:0")
    d_sizes = torch.full((3,), -77, dtype=torch.int32, device="cuda:0")
    for kw, code, word in ((dict(nframes=2, slot_bytes=enc.bound - 1), capi.ERR_SIZE, "slot_bytes"), (dict(nframes=3, slot_bytes=enc.bound), capi.ERR_ARG, "3 frames"),
                           (dict(nframes=2, slot_bytes=enc.bound, frame_stride=w * h - 1), capi.ERR_ARG, "frame_stride")):
        with pytest.raises(capi.MdcError) as e:
            enc.encode(d_in.data_ptr(), d_out=d_out.data_ptr(), d_sizes=d_sizes.data_ptr(), **kw)
        assert e.value.code == code and word in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == D.PATTERN).all() and (d_sizes.cpu().numpy() == -77).all()
    enc.encode(d_in.data_ptr(), 2)
    assert enc.files() == [D.pil("zero", w, h, 0, 95)] * 2
    L = capi.jopt_lib()
    assert L.mdcjo_profile(enc._h, 1) == 0
    ms = (capi.C.c_float * 7)()
    assert L.mdcjo_kernel_ms(enc._h, ms) == capi.ERR_ARG and "timed" in L.mdcjo_last_error().decode()
    enc.encode(d_in.data_ptr(), 2)
    assert L.mdcjo_kernel_ms(enc._h, ms) == 0 and all(0 <= x < 1000 for x in ms)
    assert enc.files() == [D.pil("zero", w, h, 0, 95)] * 2
    enc.close()


CAMERA = ("0.349153 0.436593 0.493140 0.499021 0.933271", "320 256", "crop", "192 144")


def test_rectify_dataset_with_optimal_tables(tmp_path):
    """bin/rectifyDataset <in> <out> huffman=optimal on a synthetic sequence of 5 frames: the folder opens with the reader, every
    entry is PIL's optimize=True file of the rectified frame, the pixels are those of the huffman=standard export, and the archive is
    smaller; huffman=optimal frames=png is refused with the usage text before anything is written"""
    from PIL import Image

    from mono_dataset_code_amd import build, capi, synth

    d = str(tmp_path / "seq")
    synth.write_sequence_calibration(d, CAMERA, vignette_bits=16, n_times=5)
    os.makedirs(os.path.join(d, "images"))
    for i in range(5):
        f = synth.noise_frames(11, 1, 320 * 256)[0] if i == 1 else synth.smooth_frame(320, 256, 0.7 + i, blobs=i % 2 == 0)
        synth.write_png_gray(os.path.join(d, "images", "%05d.png" % i), f.reshape(256, 320))
    outs = {}
    for mode in ("optimal", "standard"):
        out = str(tmp_path / mode)
        r = subprocess.run([build.RECTIFY_DATASET, d, out, "huffman=" + mode], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120, cwd=str(tmp_path))
        assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
        assert ("optimal Huffman tables" in r.stdout) == (mode == "optimal")
        with zipfile.ZipFile(os.path.join(out, "images.zip")) as z:
            assert z.testzip() is None and z.namelist() == ["%05d.jpg" % i for i in range(5)]
            outs[mode] = [z.read(n) for n in z.namelist()]
    src = capi.DatasetReader(d)
    for i in range(5):
        u8 = R.to_u8(src.get_image(i, 1, 0, 0, 0)[0])
        assert outs["optimal"][i] == O.pil_encode(u8, 95), i
        assert outs["standard"][i] == R.pil_encode(u8, 95), i
    src.close()
    assert os.path.getsize(str(tmp_path / "optimal" / "images.zip")) < os.path.getsize(str(tmp_path / "standard" / "images.zip"))
    reader = capi.DatasetReader(str(tmp_path / "optimal"))
    assert len(reader) == 5 and (reader.out_w, reader.out_h) == (192, 144)
    for i in range(5):
        raw = reader.get_raw(i)
        assert raw is not None, reader.last_error()
        assert np.array_equal(raw, np.array(Image.open(io.BytesIO(outs["standard"][i])))), i
    reader.close()
    r = subprocess.run([build.RECTIFY_DATASET, d, str(tmp_path / "refused"), "huffman=optimal", "frames=png"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=60, cwd=str(tmp_path))
    assert r.returncode != 0 and "usage: " in r.stderr and "[huffman=standard|optimal]" in r.stderr and "needs frames=jpg" in r.stderr
    assert not os.path.exists(str(tmp_path / "refused"))
