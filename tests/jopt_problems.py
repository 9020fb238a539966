"""Directed inputs for the JPEG encoder with per-frame optimal Huffman tables (include/mdc_jopt.h), shared by tests/test_jopt_cpu.py
and the GPU tests, and the facts about them that the tests rely on.  Everything is computed with the restatements or PIL, never
with the library under test; tests/test_jopt_cpu.py asserts that each input does what it claims."""
import functools

import numpy as np

import jenc_problems as P
import jenc_restatement as R
import jopt_restatement as O


# ---------------------------------------------------------------------------------------------------- frames

FIB_Q = 50
FIB_ROW = 128  # blocks a row


def fibonacci(n, a=1, b=2):
    out = []
    for _ in range(n):
        out.append(a)
        a, b = b, a + b
    return out


@functools.lru_cache(None)
def fibonacci_frame():
    """-> u8, 1024 x 1112 at quality 50: the 19 AC symbols (run r, size 1), r = 0..15, and (run r, size 2), r = 0..2, one per block,
    used 1, 2, 3, 5, 8, ... times, padded with flat blocks of 128 to 128 blocks a row: an AC tree deeper than 16 before limiting"""
    kinds = [P.block_of(P.single(r + 1, 1), FIB_Q) for r in range(16)] + [P.block_of(P.single(r + 1, 2), FIB_Q) for r in range(3)]
    blocks = [b for b, n in zip(kinds, fibonacci(len(kinds))) for _ in range(n)]
    flat = np.full((8, 8), 128, np.uint8)
    blocks += [flat] * (-len(blocks) % FIB_ROW)
    return np.concatenate([P.row_of(blocks[i:i + FIB_ROW]) for i in range(0, len(blocks), FIB_ROW)], axis=0)


def flat_frames():
    """one used symbol per table: DC difference 0 only after the first block, EOB only.  (The first has one more DC symbol.)"""
    return [(np.full((16, 24), 128, np.uint8), 95), (np.full((8, 8), 128, np.uint8), 75), (np.full((21, 13), 0, np.uint8), 95)]


@functools.lru_cache(None)
def tied_frame():
    """-> (u8, quality): a small noise frame for which the tie-break among equal counts decides the file"""
    for index in range(32):
        u8 = R.to_u8(R.content("noise", 24, 16, 300 + index))
        if O.encode_u8(u8, 75) != O.encode_u8(u8, 75, strict=True):
            return u8, 75
    raise LookupError("no frame whose file depends on the tie-break")


def no_eob_frame():
    """every block ends in a non-zero coefficient 63: the AC table has no EOB"""
    return P.run_frames()[100], 100


@functools.lru_cache(None)
def directed_frames():
    """-> [(name, u8, quality)]: every directed frame (the Fibonacci frame is the largest, 17,792 blocks)"""
    out = [("fibonacci", fibonacci_frame(), FIB_Q)]
    out += [("flat%d" % i, u8, q) for i, (u8, q) in enumerate(flat_frames())]
    out.append(("tied",) + tied_frame())
    out.append(("no_eob",) + no_eob_frame())
    out.append(("runs50", P.run_frames()[50], 50))
    out += [("symbols%d" % q, u8, q) for q, u8 in sorted(P.symbol_frames()[0].items())]
    out += [("dc%02d" % i, u8, 100) for i, u8 in enumerate(P.dc_frames())]
    return out


# ---------------------------------------------------------------------------------------------------- histograms for the tables call

def _hist(counts, symbols=None):
    f = np.zeros(257, np.int64)
    f[list(range(len(counts))) if symbols is None else symbols] = counts
    return f


@functools.lru_cache(None)
def histograms():
    """-> [(name, 257 counts)].  deeper_than_32: status 1.  The others build."""
    rng = np.random.RandomState(3)
    out = [("deeper_than_32", _hist(fibonacci(34))),
           ("depth_32", _hist(fibonacci(32))),
           ("depth_32_scattered", _hist(fibonacci(32), sorted(rng.choice(256, 32, replace=False).tolist()))),
           ("equal_256", _hist([7] * 256)),
           ("ones_256", _hist([1] * 256)),
           ("ones_40", _hist([1] * 40, list(range(3, 250, 6))[:40])),
           ("one_large", _hist([165000000] + [1] * 30)),
           ("one_symbol", _hist([5], [255])),
           ("two_symbols", _hist([1, 1], [0, 255])),
           ("empty", _hist([]))]
    for name, (_, u8, q) in (("fibonacci_frame_ac", directed_frames()[0]), ("tied_frame_ac", directed_frames()[4])):
        out.append((name, O.histograms(R.coefficients(u8, q))[1]))
    u8 = R.to_u8(R.content("noise", 64, 48))
    dc, ac = O.histograms(R.coefficients(u8, 95))
    return out + [("noise_dc", dc), ("noise_ac", ac)]


def expected_table(freq):
    """-> (status, bits[16], vals padded to 256, nvals) as mdcjo_optimal_tables_device gives them"""
    bits, vals, _ = O.optimal_table(freq)
    if bits is None:
        return 1, [0] * 16, [0] * 256, 0
    return 0, list(bits), list(vals) + [0] * (256 - len(vals)), len(vals)


# ---------------------------------------------------------------------------------------------------- batches

def thirteen(w, h):
    """13 frames of different content (float32): frame f's tables must come from frame f alone"""
    kinds = [("zero", 0), ("mid", 0), ("white", 0), ("checker1", 0), ("checker8", 1), ("ramp", 0), ("ramp", 3), ("special", 0)] + [("noise", i) for i in range(5)]
    return [R.content(k, w, h, i) for k, i in kinds]
