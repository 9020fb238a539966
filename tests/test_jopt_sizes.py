"""The device JPEG encoder with per-frame optimal Huffman tables (include/mdc_jopt.h) at its launch limits and on the directed
frames of tests/jopt_problems.py, on the GPU.  Every file is compared with PIL's optimize=True file byte for byte.
  grid (ceil(nblocks / 256), frames)   255, 256 and 257 blocks a frame, several frames: the last workgroup of a frame is full, has one
                                       thread, or one idle; frames that end at a workgroup's edge; the DC predictor restarts per frame
  f0 += 65535                          65,537 frames of 8x8: the second launch of the histogram, count and pack kernels goes on at
                                       frame 65535 with that frame's histogram and tables
  tables                               a tree deeper than 16 (folded back), one symbol per table, ties, no EOB, every reachable AC
                                       symbol, DC differences of size 11
  slot                                 the densest 0xFF content of the baseline's tests stays within mdcjo_jpeg_bound"""
import numpy as np
import pytest

import jenc_problems as P
import jenc_restatement as R
import jopt_device as D
import jopt_problems as J
import jopt_restatement as O

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _release():
    yield
    import gc

    import torch

    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("nframes,w,h", [(3, 2040, 8), (3, 2048, 8), (3, 2056, 8), (2, 128, 128), (5, 64, 64), (2, 512, 64)], ids=lambda v: str(v))
def test_block_counts_around_a_workgroup(nframes, w, h):
    """255, 256, 257, 256, 64 and 512 blocks a frame: a frame's last workgroup with one idle thread, full, with one thread; frames
    that end where a workgroup ends; fewer blocks than a workgroup has threads"""
    assert P.nblocks(w, h) in (255, 256, 257, 64, 512)
    frames = P.small_batch(nframes, w, h)
    want = [O.pil_encode(R.to_u8(f), 95) for f in frames]
    assert all(R.coefficients(R.to_u8(f), 95)[-1, 0] != 0 for f in frames)  # a predictor carried over a frame boundary would show
    assert len({tuple(O.dht_segments(x)) for x in want}) == nframes
    enc = D.encoder(w, h, 95, max_frames=nframes)
    assert D.run(enc, frames) == want
    assert D.run(enc, [R.to_u8(f) for f in frames]) == want
    enc.close()


def test_more_frames_than_a_grid_has_rows():
    """65,537 one-block frames, frame f = content f % 13 (65535 % 13 = 2): every launch over (parts, frames) goes on at frame 65535"""
    n = 65537
    thirteen = P.thirteen()
    want13 = [O.pil_encode(R.to_u8(f), 95) for f in thirteen]
    assert len(set(want13)) == 13 and (n - 2) % 13 == 2
    which = np.arange(n) % 13
    enc = D.encoder(8, 8, 95, max_frames=n)
    for host in (np.stack([f.reshape(-1) for f in thirteen])[which], np.stack([R.to_u8(f).reshape(-1) for f in thirteen])[which]):
        got = D.run(enc, host)
        bad = [f for f in range(n) if got[f] != want13[f % 13]]
        assert not bad, (len(bad), bad[:4])
    # mdcjo_fetch's second trip of the gather kernel: files() on the encoder's own arrays
    import torch

    d_in = torch.from_numpy(np.stack([f.reshape(-1) for f in thirteen])[which]).to("cuda:0")
    enc.encode(d_in.data_ptr(), n)
    files = enc.files()
    bad = [f for f in range(n) if files[f] != want13[f % 13]]
    assert not bad, (len(bad), bad[:4])
    enc.close()


@pytest.mark.parametrize("case", J.directed_frames(), ids=lambda c: c[0])
def test_directed_frames(case):
    """the Fibonacci frame (AC tree 20 deep before limiting, 17,792 blocks), one symbol per table, ties, no EOB, every reachable AC
    symbol, DC differences up to size 11"""
    _, u8, q = case
    want = O.pil_encode(u8, q)
    assert D.once(u8, q) == want
    assert D.once(u8.astype(np.float32), q) == want


def test_directed_frames_in_one_batch_with_their_neighbours():
    """the 24 DC frames (24 x 8, quality 100) in one call: 24 different table pairs side by side"""
    frames = P.dc_frames()
    want = [O.pil_encode(u8, 100) for u8 in frames]
    enc = D.encoder(24, 8, 100, max_frames=len(frames))
    assert D.run(enc, frames) == want
    enc.close()


def test_the_densest_ff_pixels_stay_within_the_bound():
    """d_sizes[f] <= mdcjo_jpeg_bound on the densest content the baseline's tests use (D.run asserts the size against the bound)"""
    u8, _ = P.densest_ff()
    want = O.pil_encode(u8, 100)
    assert len(want) <= O.bound(P.FF_W, P.FF_H)
    assert D.once(u8, 100) == want
    noise = P.binary_noise(0, 64, 64)  # 0 / 255 noise at quality 100: the longest codes 8-bit pixels give
    assert D.once(noise, 100) == O.pil_encode(noise, 100)


def test_stream_lengths_around_the_stuffing_chunk():
    """the stuffing kernel is a copy of the baseline's with a header of its own length: streams of one, two and three chunks and a tail"""
    for index, (w, h) in enumerate(((640, 8), (1280, 16), (640, 480))):
        u8 = R.to_u8(R.content("noise", w, h, index))
        want = O.pil_encode(u8, 95)
        assert D.once(u8, 95) == want
    assert b"\xff\x00" in want
