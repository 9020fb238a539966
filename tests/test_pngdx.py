"""The device PNG decoder with the parallel inflate on the GPU (include/mdc_pngdx.h, capi.PngDecoder(matches="parallel")).  Every
decoded frame equals PIL's decode of the same file byte for byte; reason and path of every frame are the expected ones
(tests/pngdx_problems.py; tests/test_pngdx_cpu.py proves every input called valid here valid for zlib, and every damaged one
refused by it).  On valid inputs no frame may come back with a reason, and none with the sequential path: both shares are zero.
Sentinel bytes stand behind every frame and around the status array; the input is checked unwritten.  Damaged streams are refusals
the decoder must report -- nothing here is meant to make the device fault."""
import faulthandler
import zlib

import numpy as np
import pytest

import pngd_restatement as R
import pngdx_problems as X
import pngw_restatement as P

pytestmark = pytest.mark.gpu
PATTERN = 0xA5
GAP = 24  # sentinel bytes between two frames
LIMIT = 120  # seconds a case may take before the process is ended with a traceback (a case takes a few)


@pytest.fixture(autouse=True)
def time_limit():
    faulthandler.dump_traceback_later(LIMIT, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def torch_():
    import torch

    return torch


def device_decode(w, h, streams, dec=None, matches="parallel", max_images=None, stream=None, slot_offset=0, head=b"", tail=b"", slot=None, gap=GAP):
    """one call: stream f (wrapped in head / tail, skipped again by skip_head / skip_tail) in slot f from byte slot_offset of a
    pattern-filled device array -> ([frame or None], reasons, paths).  Checks every sentinel."""
    from mono_dataset_code_amd import capi

    torch = torch_()
    n = len(streams)
    own = dec is None
    if own:
        dec = capi.PngDecoder(w, h, max_images=max_images or n, device=0, matches=matches)
    files = [head + bytes(s) + tail for s in streams]
    slot = slot or max(len(f) for f in files) + 3
    host = np.full(slot_offset + n * slot + 64, PATTERN, np.uint8)
    for f, data in enumerate(files):
        host[slot_offset + f * slot:slot_offset + f * slot + len(data)] = np.frombuffer(data, np.uint8)
    d_slots = torch.from_numpy(host).to("cuda:0")
    d_sizes = torch.tensor([len(f) for f in files], dtype=torch.int32, device="cuda:0")
    stride = w * h + gap
    d_frames = torch.full((gap + n * stride,), PATTERN, dtype=torch.uint8, device="cuda:0")
    d_status = torch.full((n + 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    dec.decode_device(d_slots.data_ptr() + slot_offset, slot, d_sizes.data_ptr(), n, d_frames.data_ptr() + gap, d_status.data_ptr() + 16, skip_head=len(head),
                      skip_tail=len(tail), frame_stride=stride, stream=stream)
    torch.cuda.synchronize()
    if own:
        dec.close()
    assert (d_slots.cpu().numpy() == host).all(), "the input was written to"
    status = d_status.cpu().numpy()
    assert (status[:4] == 0x5A5A5A5A).all() and (status[4 + n:] == 0x5A5A5A5A).all()
    reasons, paths = capi.PngDecoder.status_fields(status[4:4 + n])
    out = d_frames.cpu().numpy()
    assert (out[:gap] == PATTERN).all()
    frames = []
    for f in range(n):
        at = gap + f * stride
        assert (out[at + w * h:at + stride] == PATTERN).all(), "frame %d: written behind its %d x %d bytes" % (f, w, h)
        if reasons[f] == 0:
            frames.append(out[at:at + w * h].reshape(h, w).copy())
        else:
            frames.append(None)
            assert (out[at:at + w * h] == PATTERN).all(), "frame %d has a reason and pixels" % f
    return frames, reasons.tolist(), paths.tolist()


def check_valid(w, h, cases, **kw):
    """cases: [(name, w, h, stream)] of one size, one call: no reason anywhere, PIL's pixels, the expected paths, path 3 nowhere"""
    frames, reasons, paths = device_decode(w, h, [c[3] for c in cases], **kw)
    assert reasons == [0] * len(cases), [(c[0], R.REASONS[r]) for c, r in zip(cases, reasons) if r]  # the cap: no frame at all
    assert R.GENERAL not in paths, [c[0] for c, p in zip(cases, paths) if p == R.GENERAL]  # the cap: no frame at all
    for c, frame, path in zip(cases, frames, paths):
        want_reason, want_path, px = X.expected(w, h, c[3], pixels=True)
        assert want_reason == 0 and path == want_path, (c[0], path, want_path)
        assert np.array_equal(frame, px), (c[0], w, h)
    return paths


# ------------------------------------------------------------------------------------------------ valid streams


@pytest.mark.parametrize("size", X.SIZES, ids=lambda s: "%dx%d" % s)
def test_zlibs_streams_at_every_level_strategy_and_flush(size):
    """levels 1, 6, 9, memLevel 1 (dozens of blocks), Z_FIXED, Z_RLE, Z_HUFFMAN_ONLY, sync, full and partial flushes in the middle; on
    smooth, noise, constant and periodic images"""
    w, h = size
    paths = check_valid(w, h, X.zlib_cases(w, h))
    assert X.TOKENS in paths  # (a noise image may come as stored blocks, or as one literal-only dynamic block: the front kernel's)


def test_zlibs_streams_at_640x480():
    paths = check_valid(640, 480, X.large_valid_cases())
    assert paths.count(X.TOKENS) >= 12 and set(paths) <= {X.TOKENS, R.STORED}  # (zlib stores noise)


def test_hand_built_streams():
    """empty blocks; an end-of-block code and a match at the edges of a subsequence and of a window; lengths 3 and 258; distance 1 over
    a whole image as one chain; distance 32768; distances below the length; sources in earlier blocks, windows and stored blocks; a
    chain through every match; 15-bit codes; a one-bit distance code; 70 stored blocks between Huffman blocks"""
    cases = X.hand_cases()
    for (w, h), group in X.by_size(cases).items():
        assert set(check_valid(w, h, group)) == {X.TOKENS}, (w, h)


def test_this_projects_lz77_files_at_chain_1_4_and_64():
    for (w, h), group in X.by_size(X.lz_cases()).items():
        assert set(check_valid(w, h, group)) == {X.TOKENS}, (w, h)


def test_round_trip_with_the_lz77_encoder_in_device_memory():
    """capi.PngEncoder(compress="lz77")'s files, decoded where the encoder left them: skip_head 41, skip_tail 16"""
    from mono_dataset_code_amd import capi

    torch = torch_()
    w, h = 96, 70
    yy, xx = np.mgrid[0:h, 0:w]
    imgs = [R.test_image(w, h, 1), np.full((h, w), 31, np.uint8), ((xx // 4 + yy // 2) & 255).astype(np.uint8), ((xx % 9) * 20).astype(np.uint8)]
    n = len(imgs)
    enc = capi.PngEncoder(w, h, depth=8, filter=P.ADAPTIVE, max_images=n, device=0, compress="lz77", chain=4)
    dec = capi.PngDecoder(w, h, max_images=n, device=0, matches="parallel")
    d_in = torch.from_numpy(np.stack(imgs)).to("cuda:0")
    d_out, slot, d_sizes = enc.encode(d_in.data_ptr(), n)
    d_frames = torch.full((n * w * h + 64,), PATTERN, dtype=torch.uint8, device="cuda:0")
    d_status = torch.full((n + 4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    dec.decode_device(d_out, slot, d_sizes, n, d_frames.data_ptr(), d_status.data_ptr(), skip_head=41, skip_tail=16)
    torch.cuda.synchronize()
    status = d_status.cpu().numpy()
    reasons, paths = capi.PngDecoder.status_fields(status[:n])
    assert reasons.tolist() == [0] * n and (status[n:] == 0x5A5A5A5A).all()
    assert R.GENERAL not in paths.tolist() and X.TOKENS in paths.tolist()
    out = d_frames.cpu().numpy()
    assert (out[n * w * h:] == PATTERN).all()
    assert np.array_equal(out[:n * w * h].reshape(n, h, w), np.stack(imgs))
    enc.close()
    dec.close()


def test_every_stream_of_the_first_decoders_tests_with_both_libraries():
    """R.all_valid_cases(): the same streams through libmdc_pngd.so in the same process give the same pixels and reasons; the paths
    differ only where the sequential decoder's streams now take the token path"""
    for (w, h), group in X.by_size(X.restatement_valid_cases()).items():
        paths = check_valid(w, h, group)
        frames_i, reasons_i, paths_i = device_decode(w, h, [c[3] for c in group], matches="wave")
        frames_x, reasons_x, _ = device_decode(w, h, [c[3] for c in group])
        assert reasons_i == reasons_x == [0] * len(group)
        assert all(np.array_equal(a, b) for a, b in zip(frames_i, frames_x)), (w, h)
        assert [X.TOKENS if p == R.GENERAL else p for p in paths_i] == paths, (w, h)


# ------------------------------------------------------------------------------------------------ damaged streams


def damaged_batches():
    """{(w, h): [(name, stream, reason)]}: every damaged stream with a valid neighbour of its size behind it"""
    out = {}
    for name, w, h, s, reason in X.damaged_cases():
        raw = P.filtered(R.test_image(w, h, 3), 8, P.ADAPTIVE).tobytes()
        good = [R.zstream(raw), R.literal_stream(raw), R.zstream(raw, strategy=zlib.Z_FIXED), R.stored_stream(raw), R.zstream(raw, X.deflated(raw, mem=1))]
        batch = out.setdefault((w, h), [])
        batch.append((name, s, reason))
        batch.append(("good", good[(len(batch) // 2) % len(good)], 0))
    return out


def test_damaged_streams_among_valid_neighbours():
    """the expected reason, the sequential path (or the front kernel's where the sum, not the stream, is wrong), the frame untouched,
    the neighbours good"""
    seen = set()
    for (w, h), batch in damaged_batches().items():
        img = R.test_image(w, h, 3)
        frames, reasons, paths = device_decode(w, h, [s for _, s, _ in batch])
        for (name, s, want), frame, reason, path in zip(batch, frames, reasons, paths):
            e_reason, e_path, _ = X.expected(w, h, s)
            assert reason == want == e_reason, (name, R.REASONS[reason], R.REASONS[want])
            assert path == e_path, (name, path, e_path)
            if want:
                assert frame is None and path != X.TOKENS, name  # (device_decode has checked that its bytes are untouched)
                seen.add((reason, path))
            else:
                assert np.array_equal(frame, img), name
        assert X.TOKENS in paths
    assert {r for r, _ in seen} == set(range(1, 11)) and {p for _, p in seen} == {R.PARALLEL, R.STORED, R.GENERAL}
    later = [c for c in X.damaged_cases() if c[0].startswith("later_")]
    assert all(X.expected(w, h, s)[1] == R.GENERAL for _, w, h, s, _ in later)  # all of these went to the token path first


# ------------------------------------------------------------------------------------------------ call shapes


def test_more_images_than_the_grid_in_one_call():
    """the kernels' grids end at 8192 workgroups: 8200 frames of 3 x 2, token path, stored and literal-only streams and damaged ones"""
    cases = X.zlib_cases(3, 2)
    raw = zlib.decompress(cases[0][3])
    pool = [c[3] for c in cases] + [R.stored_stream(raw), R.literal_stream(raw), cases[0][3][:-1], cases[1][3][:5]]
    want = [X.expected(3, 2, s, pixels=True) for s in pool]
    n = 8200
    frames, reasons, paths = device_decode(3, 2, [pool[(f * 7) % len(pool)] for f in range(n)], gap=2)
    for f in range(n):
        reason, path, px = want[(f * 7) % len(pool)]
        assert (reasons[f], paths[f]) == (reason, path), f
        assert frames[f] is None if reason else np.array_equal(frames[f], px), f
    assert {X.TOKENS, R.PARALLEL, R.STORED, R.GENERAL} == set(paths)


def test_call_shapes_on_one_decoder():
    """max_images 1; a decoder reused with odd slot offsets and strides, on a non-default stream, with head and tail bytes to skip"""
    torch = torch_()
    from mono_dataset_code_amd import capi

    w, h = 64, 64
    cases = [c for c in X.zlib_cases(w, h) if "smooth" in c[0] or "periodic" in c[0]]
    want = [X.expected(w, h, c[3], pixels=True) for c in cases]
    one = capi.PngDecoder(w, h, max_images=1, device=0, matches="parallel")
    for c, (reason, path, px) in list(zip(cases, want))[:3]:
        frames, reasons, paths = device_decode(w, h, [c[3]], dec=one)
        assert (reasons, paths) == ([0], [path]) and np.array_equal(frames[0], px), c[0]
    one.close()
    dec = capi.PngDecoder(w, h, max_images=len(cases) + 2, device=0, matches="parallel")
    side = torch.cuda.Stream()
    longest = max(len(c[3]) for c in cases)
    for kw in ({}, {"slot_offset": 1}, {"slot_offset": 3, "slot": longest + 1}, {"stream": side.cuda_stream}, {"gap": 7}, {"head": b"\x01" * 41, "tail": b"\x02" * 16, "slot_offset": 5}):
        frames, reasons, paths = device_decode(w, h, [c[3] for c in cases], dec=dec, **kw)
        assert reasons == [0] * len(cases) and paths == [p for _, p, _ in want], kw
        assert all(np.array_equal(f, px) for f, (_, _, px) in zip(frames, want)), kw
    status, d_frames = dec.decode_host([c[3] for c in cases[:5]])
    assert capi.PngDecoder.status_fields(status)[1].tolist() == [p for _, p, _ in want[:5]]
    dec.profile(True)
    device_decode(w, h, [c[3] for c in cases], dec=dec)
    ms = dec.kernel_ms()
    assert len(ms) == 5 and all(v >= 0 for v in ms) and ms[1] > 0  # front, tokens, general, checks, unfilter
    dec.close()
