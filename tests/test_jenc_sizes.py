"""The device JPEG encoder (mono_dataset_code_amd/csrc/mdc_jenc.hip) at, below and past every loop, chunk and index-width limit.
Every file equals PIL's (libjpeg-turbo), byte for byte; past libjpeg's 65500 pixels per side it equals the restatement's, which
tests/test_jenc_sizes_cpu.py pins to PIL at 65500 both ways.  Sizes and every byte outside the files are checked too.

  the clear of jenc_scan_kernel           min((bits >> 5) + 2, stream_words) words: one encoder over many calls, dense noise, then
                                          zero / mid / ramp inside and just behind it, fewer frames, another seed, one frame; at
                                          640x480 a stream 1, 2 and 3 words shorter than the call before (3825909 bits, then
                                          3825887 / 3825855 / 3825818); output() and test-owned slots in turn on the live encoder
  d_packed, packed_capacity               files() after a small call, after one more than 1.25 x + 4096 larger, after a smaller one;
                                          mdcj_fetch one byte short (MDCJ_ERR_SIZE, h_out untouched), h_out NULL, nframes 0
  f0 += 65535 in encode() and mdcj_fetch  65537 frames of 8x8, frame f = content f % 13 (65535 % 13 = 2): frame0 + blockIdx.y,
                                          d_out + f0 * slot_bytes, d_offsets + f0; float and 8-bit entry
  i % nblocks, 256 threads                nblocks * nframes = 255, 256, 257 with nblocks 3, 1, 1, and 17 frames of 15: the block in
                                          front of a workgroup's thread 0 belongs to another frame
  kStuffChunk = 16384, 16 per thread      unstuffed lengths 1, 15, 16, 17, 16383 .. 16386 (all nbytes % 4: the pad's shift 24 - 8 *
                                          ((nbytes - 1) & 3)), 32767 .. 32769; nbits % 8 = 0 (no pad), 1, 7; a padded last byte that
                                          is 0xFF (FF 00 FF D9); 0xFF as byte 16383 of a chunk and as byte 15 of a thread's 16
  staged[2 * kStuffChunk]                 0/255 noise at quality 100: the densest window of 16384 stream bytes among 300 seeds holds
                                          589 bytes 0xFF.  The array is sized for 16384, every byte 0xFF, which no pixels produce:
                                          that bound is argued in include/mdc_jenc.h, not reached here.
  walk_block: while (run > 15), EOB       a lone coefficient at zigzag 63 (three ZRL, no EOB) and at 62 (EOB), zero runs of 15, 16,
                                          31, 32, 47, 48, every run 0..15, all 63 AC coefficients non-zero, AC sizes 1..10 and DC
                                          differences of sizes 0..11 with both signs (first block of a frame: all but +11, which 8-bit
                                          pixels cannot give): all 162 AC symbols are coded
  kGroupBlocks = 32, scan loop of 1024    nblocks 31, 32, 33 (248, 256, 264 x 8), 1023, 1024, 1025 (264x248, 256x256, 328x200), 256
                                          blocks in a row (2048x8), 2056x16; widths 1..7 x 64; widths 57, 63, 65, 71 (bw 8 and 9: a
                                          wave's eight blocks over two block rows with edge extension)
  by = b / bw, (long long)y * w + x, SOF0 65500x1, 1x65500 (PIL); 65535x1, 1x65535, 65535x8, 9x65535 (restatement)
  fill_tables: scale                      qualities 1, 2, 24, 25, 49, 50, 51, 99
  uint32_t bit offsets, pos, nbytes       one 12544x12544 frame of 0/255 noise at quality 100, 2458624 blocks at 935.4 bits per block
                                          before stuffing (964.5 after): 2.30e9 bits, past 2^31
  mdcj_create: bound <= 2^30, < 2^31      506 x 5101 = 2581106 blocks accepted and encoded; 65536 blocks x 32767 frames: past the
                                          argument checks, MDCJ_ERR_NOMEM unless it fits (refusals: tests/test_jenc_sizes_cpu.py)
  stream, device, pointers, values        two encoders on two streams with interleaved calls; an encode behind the copy of its input;
                                          device -1; device 1 while 0 is current; input bases 1 and 3 elements / bytes into the
                                          allocation, odd slot_bytes, frame_stride w * h + 1; |v| >= 2^31, +-FLT_MAX, denormals, -nan

The large cases are sized from the free device memory and skipped, saying why, when it is short."""
import ctypes as C
import functools

import numpy as np
import pytest

import jenc_problems as P
import jenc_restatement as R

pytestmark = pytest.mark.gpu
PATTERN, GUARD = 0xA5, 4096
GiB = 2.0 ** 30
DENSEST_FF = 589
AC_SYMBOLS_REACHED = 162


@pytest.fixture(autouse=True)
def _release():
    yield
    import gc

    import torch

    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def need(nbytes, what):
    """skip unless nbytes (+10 %) are free on the device"""
    import torch

    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if 1.1 * nbytes > free:
        pytest.skip("%s needs %.1f GiB + 10 %% of device memory, %.1f GiB free" % (what, nbytes / GiB, free / GiB))


@functools.lru_cache(None)
def pil(kind, w, h, index, quality):
    return P.expected(R.to_u8(R.content(kind, w, h, index)), quality)


def encoder(w, h, quality, max_frames=1, device=0):
    from mono_dataset_code_amd import capi

    enc = capi.JpegEncoder(w, h, quality, max_frames, device=device)
    assert enc.bound == R.bound(w, h)
    return enc


class Call:
    pass


def launch(enc, frames, extra_stride=0, extra_slot=0, offset=0, stream=None, device="cuda:0", d_in=None):
    """Enqueues one encode of `frames` (a list of h x w arrays or an (n, w * h) array; float32 or uint8 chooses the entry) into
    pattern-filled slots of the test's own with a guard region behind them.  Nothing waits; the encoder is the caller's."""
    import torch

    from mono_dataset_code_amd import capi

    c = Call()
    host = frames if isinstance(frames, np.ndarray) and frames.ndim == 2 else np.stack([np.asarray(f).reshape(-1) for f in frames])
    assert host.dtype in (np.uint8, np.float32) and host.shape[1] == enc.w * enc.h
    c.enc, c.n, c.u8, c.stream = enc, host.shape[0], host.dtype == np.uint8, stream
    c.stride, c.slot = enc.w * enc.h + extra_stride, enc.bound + extra_slot
    with torch.cuda.stream(stream) if stream is not None else torch.cuda.device(device):
        if d_in is None:
            padded = np.full((c.n, c.stride), 77 if c.u8 else np.nan, host.dtype)
            padded[:, :enc.w * enc.h] = host
            d_in = torch.empty(c.n * c.stride + offset, dtype=torch.uint8 if c.u8 else torch.float32, device=device)
            d_in[offset:].copy_(torch.from_numpy(padded.reshape(-1)))
        c.d_in = d_in
        c.d_out = torch.full((c.n * c.slot + GUARD,), PATTERN, dtype=torch.uint8, device=device)
        c.d_sizes = torch.full((c.n + 16,), -77, dtype=torch.int32, device=device)
    L = capi.jenc_lib()
    fn = L.mdcj_encode_u8_device if c.u8 else L.mdcj_encode_f32_device
    rc = fn(enc._h, d_in.data_ptr() + offset * d_in.element_size(), c.stride, c.n, c.d_out.data_ptr(), c.slot, c.d_sizes.data_ptr(),
            stream.cuda_stream if stream is not None else None)
    assert rc == 0, L.mdcj_last_error()
    return c


def collect(c):
    """waits for the call's stream -> the files; checks the sizes and every byte outside the files against the pattern"""
    import torch

    if c.stream is not None:
        c.stream.synchronize()
    else:
        torch.cuda.synchronize(c.d_out.device)
    out, dsz = c.d_out.cpu().numpy(), c.d_sizes.cpu().numpy()
    n, slot = c.n, c.slot
    sizes = dsz[:n].astype(np.int64)
    assert (dsz[n:] == -77).all(), "sizes written past the last frame"
    assert (sizes > P.HEADER).all() and (sizes <= c.enc.bound).all(), (sizes.min(), sizes.max())
    assert (out[n * slot:] == PATTERN).all(), "guard region behind the last slot"
    body = out[:n * slot].reshape(n, slot)
    if n <= 64:
        for i in range(n):
            assert (body[i, sizes[i]:] == PATTERN).all(), "slot %d written past its file" % i
    else:
        assert ((body == PATTERN) | (np.arange(slot)[None, :] < sizes[:, None])).all(), "a slot written past its file"
    c.sizes = sizes
    return [body[i, :sizes[i]].tobytes() for i in range(n)]


def run(enc, frames, **kw):
    return collect(launch(enc, frames, **kw))


def own(enc, frames):
    """the same through the encoder's own output() arrays and files()"""
    import torch

    host = np.stack([np.asarray(f).reshape(-1) for f in frames])
    d_in = torch.from_numpy(host).to("cuda:0")
    p, sizes = enc.encode(d_in.data_ptr(), len(frames), u8=host.dtype == np.uint8)
    assert p == enc.output()[0] and enc.output()[1] == enc.bound
    files = enc.files()
    assert [len(f) for f in files] == sizes.tolist()
    return files


def once(u8, quality, **kw):
    """one 8-bit frame on an encoder of its own"""
    h, w = u8.shape
    enc = encoder(w, h, quality)
    got = run(enc, [u8], **kw)[0]
    enc.close()
    return got


# ---------------------------------------------------------------------------------------------------- 1. one encoder, many calls

def test_one_encoder_over_many_calls():
    """the scratch arrays of a call hold the call before: the words the packer ORs into must be cleared, whatever was there"""
    w, h, q = 72, 40, 95
    enc = encoder(w, h, q, max_frames=8)
    noise = lambda first: ([R.content("noise", w, h, first + i) for i in range(8)], [pil("noise", w, h, first + i, q) for i in range(8)])
    frames, want = noise(0)
    assert min(len(f) for f in want) > 2500  # dense: long streams
    assert run(enc, frames) == want
    for kind in ("zero", "mid", "ramp"):  # much shorter streams: stale words inside and just behind
        assert len(pil(kind, w, h, 0, q)) + 12 < min(len(f) for f in want)
        assert run(enc, [R.content(kind, w, h, i) for i in range(8)]) == [pil(kind, w, h, i, q) for i in range(8)], kind
    assert run(enc, frames[:3]) == want[:3]
    assert own(enc, [R.content("ramp", w, h, i) for i in range(8)]) == [pil("ramp", w, h, i, q) for i in range(8)]
    frames, want = noise(50)
    assert run(enc, frames) == want
    assert own(enc, frames[5:6]) == want[5:6]
    assert run(enc, [R.to_u8(R.content("checker1", w, h))]) == [pil("checker1", w, h, 0, q)]
    enc.close()


def test_one_encoder_at_the_real_size_and_streams_a_few_words_shorter():
    """640x480 noise at quality 100, then `mid`, then for d = 1, 2, 3 the noise again and a frame whose stream is d words
    shorter: the partial last word and the one behind it held the longer stream's bits (the `+ 2` of the clear)"""
    a, shorter, bits = P.shorter_by_words()
    enc = encoder(640, 480, 100)
    want_a = R.pil_encode(a, 100)
    assert (bits[0] + 7) // 8 == len(P.unstuffed(want_a))
    assert run(enc, [a]) == [want_a]
    assert run(enc, [R.content("mid", 640, 480)]) == [pil("mid", 640, 480, 0, 100)]
    for d in (1, 2, 3):
        assert (bits[0] >> 5) - (bits[d] >> 5) == d
        assert run(enc, [a]) == [want_a]
        assert run(enc, [shorter[d]]) == [R.pil_encode(shorter[d], 100)], d
    enc.close()


def test_fetch_grows_shrinks_and_refuses_without_harm():
    from mono_dataset_code_amd import capi

    import torch

    w, h, q = 72, 40, 95
    L = capi.jenc_lib()
    enc = encoder(w, h, q, max_frames=8)
    small, small_want = [R.content("mid", w, h)], [pil("mid", w, h, 0, q)]
    big, big_want = [R.content("noise", w, h, i) for i in range(8)], [pil("noise", w, h, i, q) for i in range(8)]

    def still_good():
        assert run(enc, big[2:5]) == big_want[2:5]

    assert own(enc, small) == small_want
    assert sum(map(len, big_want)) > 1.25 * len(small_want[0]) + 4096  # the gathered buffer has to grow
    assert own(enc, big) == big_want
    assert own(enc, small) == small_want
    assert own(enc, big[:2]) == big_want[:2]
    # the C function itself, on slots of the test's own
    c = launch(enc, big)
    assert collect(c) == big_want
    total = sum(map(len, big_want))
    args = (enc._h, c.d_out.data_ptr(), c.slot, c.d_sizes.data_ptr())
    h_sizes = np.zeros(8, np.int32)
    h_out = np.full(total + 64, 0x5A, np.uint8)
    assert L.mdcj_fetch(*args, 8, h_out.ctypes.data, total - 1, h_sizes.ctypes.data, None) == capi.ERR_SIZE
    assert "room for %d" % (total - 1) in L.mdcj_last_error().decode() and (h_out == 0x5A).all()
    assert h_sizes.tolist() == [len(f) for f in big_want]
    still_good()
    assert L.mdcj_fetch(*args, 8, None, 0, h_sizes.ctypes.data, None) == total and (h_out == 0x5A).all()
    still_good()
    h_sizes[:] = -5
    assert L.mdcj_fetch(*args, 0, h_out.ctypes.data, total, h_sizes.ctypes.data, None) == 0
    assert (h_out == 0x5A).all() and (h_sizes == -5).all()
    still_good()
    assert L.mdcj_fetch(*args, 8, h_out.ctypes.data, total, h_sizes.ctypes.data, None) == total  # exactly enough room
    assert h_out[:total].tobytes() == b"".join(big_want) and (h_out[total:] == 0x5A).all()
    # nframes = 0 on the encode entry: nothing is touched
    d_sizes = torch.full((4,), -77, dtype=torch.int32, device="cuda:0")
    assert L.mdcj_encode_f32_device(enc._h, None, w * h, 0, None, enc.bound, d_sizes.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert (d_sizes.cpu().numpy() == -77).all()
    still_good()
    enc.close()


# ---------------------------------------------------------------------------------------------------- 2. more than 65535 frames

def test_more_frames_than_a_grid_has_rows():
    """65537 one-block frames, frame f = content f % 13: the second launch of the DCT kernel and of the gather kernel must go on at
    frame 65535 (content 2) and at its slot"""
    n = 65537
    need(n * (64 * 4 + 2 * 1440 + 340) + 2 ** 28, "65537 frames")
    thirteen = P.thirteen()
    want13 = [R.pil_encode(R.to_u8(f), 95) for f in thirteen]
    assert len(set(want13)) == 13 and (n - 2) % 13 == 2
    which = np.arange(n) % 13
    f32 = np.stack([f.reshape(-1) for f in thirteen])[which]
    enc = encoder(8, 8, 95, max_frames=n)
    for host in (f32, np.stack([R.to_u8(f).reshape(-1) for f in thirteen])[which]):
        c = launch(enc, host)
        got = collect(c)
        assert (c.sizes == np.array([len(f) for f in want13])[which]).all()
        bad = [f for f in range(n) if got[f] != want13[f % 13]]
        assert not bad, (len(bad), bad[:4])
    # the gather kernel's second trip: files() on the encoder's own arrays
    import torch

    d_in = torch.from_numpy(f32).to("cuda:0")
    enc.encode(d_in.data_ptr(), n)
    files = enc.files()
    bad = [f for f in range(n) if files[f] != want13[f % 13]]
    assert not bad, (len(bad), bad[:4])
    enc.close()


@pytest.mark.parametrize("nframes,w,h", [(85, 24, 8), (256, 8, 8), (257, 8, 8), (17, 40, 24)], ids=lambda v: str(v))
def test_frames_end_at_the_edges_of_a_workgroup(nframes, w, h):
    """nblocks * nframes = 255, 256, 257 (and 17 x 15): thread 0 of the second workgroup of the count and pack kernels starts a frame
    or sits inside one, and the DC predictor restarts at every frame"""
    assert P.nblocks(w, h) * nframes in (255, 256, 257)
    frames = P.small_batch(nframes, w, h)
    want = [R.pil_encode(R.to_u8(f), 95) for f in frames]
    assert all(R.coefficients(R.to_u8(f), 95)[-1, 0] != 0 for f in frames[:4])  # a predictor carried over would show
    enc = encoder(w, h, 95, max_frames=nframes)
    assert run(enc, frames) == want
    enc.close()


# ---------------------------------------------------------------------------------------------------- 3. stuffing chunks and the tail

@pytest.mark.parametrize("nbytes", P.LENGTHS)
def test_stream_lengths_around_the_stuffing_chunk(nbytes):
    u8, nbits = P.strip_of_length(nbytes)
    want = R.pil_encode(u8, P.STRIP_Q)
    assert len(P.unstuffed(want)) == nbytes == (nbits + 7) // 8
    assert once(u8, P.STRIP_Q) == want


@pytest.mark.parametrize("nbytes,residue", P.RESIDUES)
def test_pad_bits_of_the_last_byte(nbytes, residue):
    u8, nbits = P.strip_of_length(nbytes, residue)
    want = R.pil_encode(u8, P.STRIP_Q)
    assert nbits % 8 == residue and len(P.unstuffed(want)) == nbytes
    assert once(u8, P.STRIP_Q) == want


def test_ff_bytes_at_the_tail_and_at_the_seams():
    u8 = P.padded_ff()
    want = R.pil_encode(u8, 95)
    assert want.endswith(b"\xff\x00\xff\xd9")
    assert once(u8, 95) == want
    for (u8, p), where in ((P.ff_at_chunk_end(), P.CHUNK - 1), (P.ff_at_thread_end(), None)):
        want = R.pil_encode(u8, P.STRIP_Q)
        s = P.unstuffed(want)
        assert s[p] == 0xFF and len(s) > p + 1 and p % 16 == 15 and (where is None or p == where)
        assert once(u8, P.STRIP_Q) == want


def test_the_densest_ff_pixels_give():
    u8, count = P.densest_ff()
    want = R.pil_encode(u8, 100)
    assert count == DENSEST_FF == P.densest_window(P.unstuffed(want))
    assert once(u8, 100) == want


# ---------------------------------------------------------------------------------------------------- 4. directed blocks

def test_directed_runs_zrl_and_eob():
    frames = P.run_frames()
    k = P.walk(R.coefficients(frames[50], 50))
    assert (k["run"] >> 4).max() == 3 and set(range(16)) | {31, 32, 47, 48, 61, 62} <= set(k["run"].tolist()) and not k["eob"].all()
    assert (R.coefficients(frames[100], 100)[:, 1:] != 0).all()
    for q, u8 in frames.items():
        assert once(u8, q) == R.pil_encode(u8, q), q


def test_directed_ac_symbols():
    frames, _ = P.symbol_frames()
    seen = P.ac_symbols(R.coefficients(P.run_frames()[50], 50))
    for q, u8 in frames.items():
        seen |= P.ac_symbols(R.coefficients(u8, q))
        assert once(u8, q) == R.pil_encode(u8, q), q
    assert len(seen) == AC_SYMBOLS_REACHED


def test_directed_dc_differences():
    frames = P.dc_frames()
    diffs = np.concatenate([P.walk(R.coefficients(u8, 100))["diff"] for u8 in frames])
    assert set(zip(P.category(diffs).tolist(), np.sign(diffs).tolist())) == {(0, 0)} | {(s, g) for s in range(1, 12) for g in (1, -1)}
    enc = encoder(24, 8, 100, max_frames=len(frames))
    assert run(enc, frames) == [R.pil_encode(u8, 100) for u8 in frames]
    enc.close()


# ---------------------------------------------------------------------------------------------------- 5. shapes and qualities

@pytest.mark.parametrize("shape", P.SHAPES_PIL + P.SHAPES_RESTATED + P.SHAPES_GRID, ids=lambda s: "%dx%d" % s)
def test_block_grid_and_header_limits(shape):
    w, h = shape
    frames = [R.content(kind, w, h) for kind in P.SHAPE_CONTENTS]
    want = [pil(kind, w, h, 0, 95) for kind in P.SHAPE_CONTENTS]
    at = want[0].index(b"\xff\xc0") + 5
    assert want[0][at:at + 4] == bytes([h >> 8, h & 255, w >> 8, w & 255])
    enc = encoder(w, h, 95, max_frames=2)
    assert run(enc, frames) == want
    enc.close()


@pytest.mark.parametrize("quality", P.QUALITIES)
def test_qualities_at_the_scaling_rules_edges(quality):
    assert once(R.to_u8(R.content("noise", 24, 16)), quality) == pil("noise", 24, 16, 0, quality)


# ---------------------------------------------------------------------------------------------------- 6. 32-bit offsets past 2^31

def test_bit_offsets_past_two_to_the_31():
    """one frame whose stream is 2.3e9 bits long: every 32-bit offset, count and position in scan, pack and stuff passes 2^31"""
    import torch

    n = P.BIG
    blocks = P.nblocks(n, n)
    need(blocks * (128 + 4 + 208 + 64) + 2 * R.bound(n, n), "the 12544 x 12544 frame")
    u8 = P.binary_noise(0, n, n)
    want = R.pil_encode(u8, 100)
    assert 8 * (len(want) - 330) > 2 ** 31
    assert 2 ** 31 < 8 * (len(want) - 330 - want.count(b"\xff\x00", P.HEADER)) < 2 ** 32  # before stuffing too
    enc = encoder(n, n, 100)
    c = launch(enc, u8.reshape(1, -1))
    del u8
    torch.cuda.synchronize()
    assert int(c.d_sizes[0]) == len(want)
    got = c.d_out.cpu().numpy()
    assert (got[len(want):] == PATTERN).all()
    assert got[:len(want)].tobytes() == want
    enc.close()


def test_create_just_below_two_to_the_31_blocks():
    """65536 blocks x 32767 frames = 2^31 - 65536: past the argument checks, so the scratch arrays (0.7 TB) are asked for; where they
    do not fit that is MDCJ_ERR_NOMEM, nothing is left behind, and the next encoder is good"""
    from mono_dataset_code_amd import capi

    L = capi.jenc_lib()
    h_ = C.c_void_p()
    rc = L.mdcj_create(0, 2048, 2048, 95, 32767, C.byref(h_))
    if rc == 0:
        L.mdcj_destroy(h_)
    else:
        assert rc == capi.ERR_NOMEM and not h_.value and "allocate" in L.mdcj_last_error().decode(), L.mdcj_last_error()
    assert once(R.to_u8(R.content("ramp", 16, 8)), 95) == pil("ramp", 16, 8, 0, 95)


def test_the_largest_frame_create_accepts():
    """the most blocks a frame may have (bound <= 2^30): scratch arrays and slot at their largest, a tiny stream"""
    bw, bh = P.largest_accepted()
    w, h = 8 * bw, 8 * bh
    assert R.bound(w, h) <= 2 ** 30 < R.bound(w, h) + 416 * 8
    need(bw * bh * (128 + 4 + 208 + 64) + 2 * R.bound(w, h), "the %d x %d frame" % (w, h))
    u8 = np.full((h, w), 128, np.uint8)
    want = R.pil_encode(u8, 95)
    enc = encoder(w, h, 95)
    assert collect(launch(enc, u8.reshape(1, -1))) == [want]
    enc.close()


# ---------------------------------------------------------------------------------------------------- 7. streams, devices, pointers, values

def test_two_encoders_on_two_streams_interleaved():
    import torch

    s1, s2 = torch.cuda.Stream(device=0), torch.cuda.Stream(device=0)
    e1, e2 = encoder(72, 40, 95, max_frames=4), encoder(40, 24, 75, max_frames=3)
    calls = []
    for i in range(3):  # several encodes each before anything waits; an encoder's calls are ordered by its stream
        calls.append((launch(e1, [R.content("noise", 72, 40, 4 * i + j) for j in range(4)], stream=s1), [pil("noise", 72, 40, 4 * i + j, 95) for j in range(4)]))
        calls.append((launch(e2, [R.content("ramp", 40, 24, 3 * i + j) for j in range(3)], stream=s2), [pil("ramp", 40, 24, 3 * i + j, 75) for j in range(3)]))
    assert s1.cuda_stream != 0 and s2.cuda_stream != 0 and s1.cuda_stream != s2.cuda_stream
    for c, want in calls:
        assert collect(c) == want
    e1.close()
    e2.close()


def test_encode_behind_the_copy_of_its_input():
    """the input arrives by an asynchronous copy on the encoder's stream; the encode is enqueued behind it without a host wait"""
    import torch

    w, h = 640, 480
    s = torch.cuda.Stream(device=0)
    enc = encoder(w, h, 95, max_frames=2)
    host = torch.from_numpy(np.stack([R.content(k, w, h).reshape(-1) for k in ("noise", "ramp")])).pin_memory()
    with torch.cuda.stream(s):
        d_in = torch.zeros(2 * w * h, dtype=torch.float32, device="cuda:0")
        d_in.copy_(host.reshape(-1), non_blocking=True)
    c = launch(enc, host.numpy(), stream=s, d_in=d_in)
    assert collect(c) == [pil("noise", w, h, 0, 95), pil("ramp", w, h, 0, 95)]
    enc.close()


def test_current_device_and_another_device():
    import torch

    torch.cuda.set_device(0)
    enc = encoder(72, 40, 95, device=-1)
    assert run(enc, [R.content("noise", 72, 40)]) == [pil("noise", 72, 40, 0, 95)]
    enc.close()
    assert torch.cuda.current_device() == 0
    if torch.cuda.device_count() < 2:
        pytest.skip("one device: an encoder on device 1 while device 0 is current needs two")
    enc = encoder(72, 40, 95, max_frames=2, device=1)
    assert torch.cuda.current_device() == 0
    got = run(enc, [R.content("noise", 72, 40), R.content("ramp", 72, 40)], device="cuda:1")
    assert torch.cuda.current_device() == 0
    assert got == [pil("noise", 72, 40, 0, 95), pil("ramp", 72, 40, 0, 95)]
    enc.close()
    assert torch.cuda.current_device() == 0


@pytest.mark.parametrize("offset", [1, 3])
def test_unaligned_bases_odd_slots_and_strides(offset):
    w, h = 72, 40
    frames = [R.content(k, w, h) for k in ("noise", "ramp", "special")]
    want = [pil(k, w, h, 0, 95) for k in ("noise", "ramp", "special")]
    enc = encoder(w, h, 95, max_frames=3)
    assert enc.bound % 2 == 0
    assert run(enc, frames, offset=offset, extra_slot=1, extra_stride=1) == want
    assert run(enc, [R.to_u8(f) for f in frames], offset=offset, extra_slot=3, extra_stride=1) == want
    enc.close()


def test_values_far_outside_eight_bits():
    """|v| >= 2^31, +-FLT_MAX, denormals, both NaN signs: clamped by their sign, NaN -> 0 (include/mdc_jenc.h)"""
    w, h = 24, 16
    f = P.special2(w, h)
    assert (np.abs(f[np.isfinite(f)]) >= 2.0 ** 31).any() and np.isnan(f).any()
    enc = encoder(w, h, 95)
    assert run(enc, [f]) == [R.pil_encode(R.to_u8(f), 95)]
    enc.close()
