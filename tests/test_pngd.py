"""The device PNG decoder on the GPU (include/mdc_pngd.h, capi.PngDecoder).  Every decoded frame equals PIL's decode of the same
file byte for byte; reason and path of every frame equal the restatement's (tests/pngd_restatement.py; tests/test_pngd_cpu.py
proves every input called valid here valid for zlib, and every damaged one refused by it).  On valid inputs no frame may come back
with a reason: the share allowed is zero.  Sentinel bytes stand behind every frame and around the status array."""
import ctypes
import zlib

import numpy as np
import pytest

import pngd_restatement as R
import pngw_restatement as P

pytestmark = pytest.mark.gpu
PATTERN = 0xA5
GAP = 24  # sentinel bytes between two frames


def torch_():
    import torch

    return torch


def device_decode(w, h, streams, dec=None, max_images=None, stream=None, slot_offset=0, head=b"", tail=b"", slot=None):
    """one call: stream f (wrapped in head / tail, skipped again by skip_head / skip_tail) in slot f from byte slot_offset of a
    pattern-filled device array -> ([frame or None], reasons, paths).  Checks every sentinel."""
    from mono_dataset_code_amd import capi

    torch = torch_()
    n = len(streams)
    own = dec is None
    if own:
        dec = capi.PngDecoder(w, h, max_images=max_images or n, device=0)
    files = [head + bytes(s) + tail for s in streams]
    slot = slot or max(len(f) for f in files) + 3
    host = np.full(slot_offset + n * slot + 64, PATTERN, np.uint8)
    for f, data in enumerate(files):
        host[slot_offset + f * slot:slot_offset + f * slot + len(data)] = np.frombuffer(data, np.uint8)
    d_slots = torch.from_numpy(host).to("cuda:0")
    d_sizes = torch.tensor([len(f) for f in files], dtype=torch.int32, device="cuda:0")
    stride = w * h + GAP
    d_frames = torch.full((GAP + n * stride,), PATTERN, dtype=torch.uint8, device="cuda:0")
    d_status = torch.full((n + 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    dec.decode_device(d_slots.data_ptr() + slot_offset, slot, d_sizes.data_ptr(), n, d_frames.data_ptr() + GAP, d_status.data_ptr() + 16, skip_head=len(head),
                      skip_tail=len(tail), frame_stride=stride, stream=stream)
    torch.cuda.synchronize()
    if own:
        dec.close()
    assert (d_slots.cpu().numpy() == host).all(), "the input was written to"
    status = d_status.cpu().numpy()
    assert (status[:4] == 0x5A5A5A5A).all() and (status[4 + n:] == 0x5A5A5A5A).all()
    reasons, paths = capi.PngDecoder.status_fields(status[4:4 + n])
    out = d_frames.cpu().numpy()
    assert (out[:GAP] == PATTERN).all()
    frames = []
    for f in range(n):
        at = GAP + f * stride
        assert (out[at + w * h:at + stride] == PATTERN).all(), "frame %d: written behind its %d x %d bytes" % (f, w, h)
        if reasons[f] == 0:
            frames.append(out[at:at + w * h].reshape(h, w).copy())
        else:
            frames.append(None)
            assert (out[at:at + w * h] == PATTERN).all(), "frame %d has a reason and pixels" % f
    return frames, reasons.tolist(), paths.tolist()


def check_valid(w, h, named, **kw):
    """named: [(name, stream)] of one size, one call: no reason anywhere, PIL's pixels, the restatement's paths -> the paths"""
    frames, reasons, paths = device_decode(w, h, [s for _, s in named], **kw)
    assert reasons == [0] * len(named), [(n, R.REASONS[r]) for (n, _), r in zip(named, reasons) if r]  # the cap: no frame at all
    for (name, s), frame, path in zip(named, frames, paths):
        want_reason, want_path, _ = R.decode(s, w, h, pixels=False)
        assert want_reason == 0 and path == want_path, (name, path, want_path)
        assert np.array_equal(frame, R.pil_pixels(w, h, s)), (name, w, h)
    return paths


# ------------------------------------------------------------------------------------------------ unfilter


@pytest.mark.parametrize("w", [1, 2, 3, 63, 64, 65, 130])
def test_unfilter_every_type_at_the_band_edges(w):
    """h around one and two bands of 64 rows (a band's first row reads the previous band's last), w around the skew's ramp-up and
    ramp-down; types forced, mixed per row, Paeth ties, Average with carries, noise as filtered bytes"""
    for h in (1, 2, 63, 64, 65, 129):
        paths = check_valid(w, h, R.unfilter_cases(w, h))
        assert set(paths) >= {R.STORED, R.GENERAL}


# ------------------------------------------------------------------------------------------------ the parallel path


def by_size(cases):
    groups = {}
    for name, w, h, s in cases:
        groups.setdefault((w, h), []).append((name, s))
    return groups


def test_parallel_path_literal_streams():
    """the restatement's encoder in its dynamic form: forced and adaptive filters, a constant image, codes of 15 bits, streams of fewer
    subsequences than threads, of one per thread and of longer ones"""
    for (w, h), named in by_size(R.parallel_cases()).items():
        assert check_valid(w, h, named) == [R.PARALLEL] * len(named), (w, h)


@pytest.mark.parametrize("filt", [0, 2, 4, P.ADAPTIVE])
def test_round_trip_in_device_memory(filt):
    """capi.PngEncoder's files, decoded where the encoder left them: skip_head 41, skip_tail 16"""
    from mono_dataset_code_amd import capi

    torch = torch_()
    w, h = 96, 70
    rng = np.random.default_rng(filt)
    yy, xx = np.mgrid[0:h, 0:w]
    imgs = [R.test_image(w, h, 1), np.full((h, w), 31, np.uint8), rng.integers(0, 256, (h, w)).astype(np.uint8), ((xx // 4 + yy // 2) & 255).astype(np.uint8)]
    n = len(imgs)
    enc = capi.PngEncoder(w, h, depth=8, filter=filt, max_images=n, device=0)
    dec = capi.PngDecoder(w, h, max_images=n, device=0)
    d_in = torch.from_numpy(np.stack(imgs)).to("cuda:0")
    d_out, slot, d_sizes = enc.encode(d_in.data_ptr(), n)
    d_frames = torch.full((n * w * h + 64,), PATTERN, dtype=torch.uint8, device="cuda:0")
    d_status = torch.full((n + 4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    dec.decode_device(d_out, slot, d_sizes, n, d_frames.data_ptr(), d_status.data_ptr(), skip_head=41, skip_tail=16)
    torch.cuda.synchronize()
    status = d_status.cpu().numpy()
    reasons, paths = capi.PngDecoder.status_fields(status[:n])
    assert reasons.tolist() == [0] * n and (status[n:] == 0x5A5A5A5A).all()
    stored = [P.encode(img, 8, filt)[1] for img in imgs]
    assert paths.tolist() == [R.STORED if s else R.PARALLEL for s in stored] and True in stored and False in stored
    out = d_frames.cpu().numpy()
    assert (out[n * w * h:] == PATTERN).all()
    assert np.array_equal(out[:n * w * h].reshape(n, h, w), np.stack(imgs))
    enc.close()
    dec.close()


def test_stored_streams():
    """F below and above 65535 (300 x 300), exactly 65535 and exactly 2 x 65535"""
    for (w, h), named in by_size(R.stored_cases()).items():
        assert check_valid(w, h, named) == [R.STORED] * len(named), (w, h)


# ------------------------------------------------------------------------------------------------ the general path


def test_general_path_streams():
    """zlib at levels 1, 6, 9; Z_RLE, Z_FIXED, Z_HUFFMAN_ONLY (several blocks: not the parallel path); stored and compressed blocks
    mixed; empty stored blocks in the middle; distance 1 chains of length 258; a match at distance 32125; 70 stored blocks"""
    seen = {}
    for (w, h), named in by_size(R.general_cases()).items():
        for (name, _), path in zip(named, check_valid(w, h, named)):
            seen[name] = path
    assert seen.pop("empty_stored_in_the_middle") == R.STORED  # a chain of stored blocks for this decoder
    assert set(seen.values()) == {R.GENERAL} and seen["huffman_only"] == R.GENERAL and len(seen) == 11


# ------------------------------------------------------------------------------------------------ damaged streams


def test_damaged_streams_come_back_with_the_restatements_reason():
    cases = R.damaged_cases()
    w, h = cases[0][1], cases[0][2]
    frames, reasons, paths = device_decode(w, h, [c[3] for c in cases])
    for (name, _, _, s, want), frame, reason, path in zip(cases, frames, reasons, paths):
        r_reason, r_path, _ = R.decode(s, w, h, pixels=False)
        assert reason == want == r_reason and frame is None, (name, R.REASONS[reason], R.REASONS[want])
        assert path == r_path, (name, path, r_path)
    assert set(reasons) == set(range(1, 11))


# ------------------------------------------------------------------------------------------------ call shapes


def mixed_batch():
    """40 x 12: all three paths and the damaged streams, interleaved"""
    img = R.test_image(40, 12, 3)
    raw = P.filtered(img, 8, P.ADAPTIVE).tobytes()
    good = [("literal", R.literal_stream(raw)), ("stored", R.stored_stream(raw)), ("zlib", R.zstream(raw)), ("fixed", R.zstream(raw, strategy=zlib.Z_FIXED))]
    out = []
    for k, c in enumerate(R.damaged_cases()):
        out.append((c[0], c[3], c[4]))
        out.append(good[k % 4] + (0,))
    return img, out


def test_a_batch_mixing_all_paths_with_failures():
    from mono_dataset_code_amd import capi

    torch = torch_()
    img, batch = mixed_batch()
    n = len(batch)
    dec = capi.PngDecoder(40, 12, max_images=n, device=0)  # n = max_images
    want_paths = [R.decode(s, 40, 12, pixels=False)[1] for _, s, _ in batch]
    side = torch.cuda.Stream()
    for kw in ({}, {"slot_offset": 1}, {"slot_offset": 3, "slot": max(len(s) for _, s, _ in batch) + 2}, {"stream": side.cuda_stream}):  # a reused decoder
        frames, reasons, paths = device_decode(40, 12, [s for _, s, _ in batch], dec=dec, **kw)
        assert reasons == [r for _, _, r in batch], kw
        assert paths == want_paths and {R.PARALLEL, R.STORED, R.GENERAL} == {p for p, r in zip(paths, reasons) if r == 0}
        assert all(np.array_equal(f, img) for f, r in zip(frames, reasons) if r == 0)
    frames, reasons, paths = device_decode(40, 12, [batch[1][1]], dec=dec)  # n = 1
    assert reasons == [0] and np.array_equal(frames[0], img)
    frames, reasons, paths = device_decode(40, 12, [batch[1][1], batch[3][1]], dec=dec, head=b"\x01" * 41, tail=b"\x02" * 16)
    assert reasons == [0, 0] and paths == [R.PARALLEL, R.STORED]
    dec.close()


def test_decode_host_uploads_decodes_and_reports():
    from mono_dataset_code_amd import capi

    img, batch = mixed_batch()
    dec = capi.PngDecoder(40, 12, max_images=len(batch) + 3, device=0)
    for part in (batch[:5], batch, batch[1:2]):  # the staging arrays grow and are reused
        status, d_frames = dec.decode_host([s for _, s, _ in part])
        reasons, paths = capi.PngDecoder.status_fields(status)
        assert reasons.tolist() == [r for _, _, r in part]
        assert paths.tolist() == [R.decode(s, 40, 12, pixels=False)[1] for _, s, _ in part]
        got = device_bytes(d_frames, len(part) * 480).reshape(len(part), 12, 40)  # the decoder's own dense array
        assert all(np.array_equal(got[f], img) for f, (_, _, r) in enumerate(part) if r == 0)
    status, d_frames = dec.decode_host([])
    assert len(status) == 0
    dec.close()


def device_bytes(address, nbytes):
    """nbytes at a device address, as a host array"""
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    out = np.zeros(nbytes, np.uint8)
    assert hip.hipMemcpy(out.ctypes.data, ctypes.c_void_p(address), nbytes, 2) == 0  # hipMemcpyDeviceToHost
    return out


def test_argument_limits_are_refused_with_messages():
    from mono_dataset_code_amd import capi

    torch = torch_()
    dec = capi.PngDecoder(8, 8, max_images=2, device=0)
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    p = buf.data_ptr()
    for kw, word in ((dict(n=3), "0..2"), (dict(n=-1), "0..2"), (dict(frame_stride=63), "frame_stride"), (dict(skip_head=-1), "skip_head"), (dict(skip_tail=-1), "skip_tail"),
                     (dict(slot_bytes=-1), "slot_bytes"), (dict(d_sizes=p + 2), "aligned"), (dict(d_status=p + 1), "aligned"), (dict(d_frames=0), "null")):
        a = dict(d_slots=p, slot_bytes=100, d_sizes=p + 1024, n=2, d_frames=p + 2048, d_status=p + 3072)
        a.update(kw)
        with pytest.raises(capi.MdcError) as e:
            dec.decode_device(**a)
        assert word in str(e.value), (kw, str(e.value))
    with pytest.raises(capi.MdcError) as e:
        dec.decode_host([b"x"] * 3)
    assert "0..2" in str(e.value)
    dec.decode_device(p, 100, p + 1024, 0, p + 2048, p + 3072)  # no frames: nothing to do
    with pytest.raises(capi.MdcError) as e:
        capi.PngDecoder(8, 8, max_images=1, device=99)
    assert "device 99" in str(e.value)
    torch.cuda.synchronize()
    assert int(buf.sum().item()) == 0
    dec.close()
