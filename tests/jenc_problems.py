"""Inputs for the device JPEG encoder's limit tests (tests/test_jenc_sizes_cpu.py, tests/test_jenc_sizes.py) and the facts about
them that the tests rely on: the symbols the entropy coder has to emit for a frame, the exact length of its stream in bits, where
its 0xFF bytes lie.  Everything is computed with tests/jenc_restatement.py or PIL, never with the library under test.  The
searches are bounded and deterministic; a search that finds nothing raises, so an input cannot quietly lose its property."""
import functools

import numpy as np

import jenc_restatement as R

HEADER = 328  # bytes in front of the entropy-coded segment; EOI is 2 more
CHUNK = 16384  # kStuffChunk
ZRL_BITS, EOB_BITS = 11, 4

_DC = R.huffman_codes(R.DC_BITS, R.DC_VALS)
_AC = R.huffman_codes(R.AC_BITS, R.AC_VALS)
_DC_LEN = np.array([_DC[s][1] for s in range(12)])
_AC_LEN = np.zeros(256, np.int64)
for _s, (_c, _n) in _AC.items():
    _AC_LEN[_s] = _n


# ---------------------------------------------------------------------------------------------------- what a frame codes to

def category(v):
    """the JPEG size category of integers: bits of |v|, 0 for 0 (exact, no logarithm)"""
    a = np.abs(np.asarray(v, np.int64))
    c = np.zeros(a.shape, np.int64)
    for k in range(16):
        c += (a >> k) > 0
    return c


def walk(zz):
    """The symbols of a coefficient array (blocks x 64, zigzag), as the coder of include/mdc_jenc.h must emit them:
    diff (per block: DC difference), bi / ki / v (block, zigzag position and value of every non-zero AC coefficient, in order),
    run (zeros in front of it since the previous non-zero one or the DC: 0..62), eob (per block: it ends with EOB)."""
    zz = np.asarray(zz, np.int64)
    nb = zz.shape[0]
    diff = zz[:, 0] - np.concatenate([[0], zz[:-1, 0]])
    bi, ki = np.nonzero(zz[:, 1:])
    ki = ki + 1
    first = np.concatenate([[True], bi[1:] != bi[:-1]]) if bi.size else np.zeros(0, bool)
    prev = np.where(first, 0, np.concatenate([[0], ki[:-1]]))
    last = np.zeros(nb, np.int64)
    last[bi] = ki
    return dict(diff=diff, bi=bi, ki=ki, v=zz[bi, ki], run=ki - prev - 1, eob=last < 63)


def block_bits(zz):
    """bits each block's code takes"""
    k = walk(zz)
    dcat, acat = category(k["diff"]), category(k["v"])
    bits = _DC_LEN[dcat] + dcat + EOB_BITS * k["eob"]
    np.add.at(bits, k["bi"], _AC_LEN[((k["run"] & 15) << 4) | acat] + acat + ZRL_BITS * (k["run"] >> 4))
    return bits


def frame_bits(u8, quality):
    """the length of the frame's stream in bits, before padding and stuffing (jenc_scan_kernel's frame_bits)"""
    return int(block_bits(R.coefficients(np.asarray(u8), quality)).sum())


def ac_symbols(zz):
    """the set of AC symbols (run << 4 | size, 0xF0, 0x00) the array's code uses"""
    k = walk(zz)
    s = set((((k["run"] & 15) << 4) | category(k["v"])).tolist())
    if (k["run"] > 15).any():
        s.add(0xF0)
    if k["eob"].any():
        s.add(0x00)
    return s


def unstuffed(jpeg):
    """the stream's bytes as jenc_stuff_kernel reads them: the entropy-coded segment of a file without its stuffed zeros"""
    return jpeg[HEADER:-2].replace(b"\xff\x00", b"\xff")


def expected(u8, quality):
    """the reference file: PIL's wherever libjpeg takes the size (<= 65500), the restatement's past it"""
    h, w = u8.shape
    return R.pil_encode(u8, quality) if max(w, h) <= 65500 else R.encode_u8(u8, quality)


# ---------------------------------------------------------------------------------------------------- item 2: batches

def thirteen():
    """13 distinct 8x8 frames (float): frame f of the long batch is number f % 13"""
    kinds = [("zero", 0), ("mid", 0), ("white", 0), ("checker1", 0), ("checker1", 1), ("ramp", 0), ("ramp", 3), ("special", 0)] + [("noise", i) for i in range(5)]
    return [R.content(k, 8, 8, i) for k, i in kinds]


def small_batch(nframes, w, h):
    """noise frames with a large first DC coefficient each, so a DC predictor carried over a frame boundary shows"""
    return [(R.content("noise", w, h, 100 + i) * 0.3 + (20, 60, 170)[i % 3]).astype(np.float32) for i in range(nframes)]


# ---------------------------------------------------------------------------------------------------- item 3: exact lengths

STRIP_Q = 95
STRIP_MAX_BLOCKS = 560


@functools.lru_cache(None)
def _noise_strip(seed):
    u8 = np.random.RandomState(seed).uniform(0, 255, (8, 8 * STRIP_MAX_BLOCKS)).astype(np.uint8)
    zz = R.coefficients(u8, STRIP_Q)
    return u8, zz, np.concatenate([[0], np.cumsum(block_bits(zz))])


def strip(seed, k, nblocks, lead=0):
    """8 rows, `lead` blocks of 128, then the first k blocks of the seed's noise strip, then 128 up to nblocks blocks"""
    u8 = np.full((8, 8 * nblocks), 128, np.uint8)
    u8[:, 8 * lead:8 * (lead + k)] = _noise_strip(seed)[0][:, :8 * k]
    return u8


@functools.lru_cache(None)
def strip_of_bits(lo, hi, residue=None):
    """-> (u8, nbits): a strip (seed 0) whose stream has lo <= nbits <= hi bits (and nbits % 8 == residue where given).  Every
    constant block after the first adds 6 bits (DC difference 0: `00`, EOB: `1010`), so the search is over k, the number of
    noise blocks, downwards from the most that fit, and the constant blocks follow from arithmetic."""
    _, zz, cum = _noise_strip(0)
    kmax = min(int(np.searchsorted(cum, hi, side="right")) - 1, STRIP_MAX_BLOCKS)
    for k in range(kmax, max(kmax - 24, -1), -1):
        if k == 0:
            first = 6
        else:
            d = int(category(-int(zz[k - 1, 0])))
            first = int(_DC_LEN[d]) + d + EOB_BITS
        base = int(cum[k]) + first  # k noise blocks and one constant block
        m0 = max(0, -((base - lo) // 6))
        for m in range(m0, m0 + 4):
            n = base + 6 * m
            if lo <= n <= hi and (residue is None or n % 8 == residue) and k + 1 + m <= 8191:
                return strip(0, k, k + 1 + m), n
    raise LookupError("no strip with %d..%d bits, residue %r" % (lo, hi, residue))


def strip_of_length(nbytes, residue=None):
    """a strip whose unstuffed stream is exactly nbytes long"""
    return strip_of_bits(8 * nbytes - 7, 8 * nbytes, residue)


LENGTHS = [1, 15, 16, 17, 16383, 16384, 16385, 16386, 32767, 32768, 32769]  # 16383..16386: all four values of nbytes % 4
RESIDUES = [(16384, 0), (16384, 7), (16384, 1), (3, 0)]  # (length, nbits % 8): no pad, one pad bit, seven


@functools.lru_cache(None)
def padded_ff():
    """a 16x8 noise frame whose padded last byte is 0xFF: the file ends FF 00 FF D9"""
    for index in range(64):
        u8 = R.to_u8(R.content("noise", 16, 8, index))
        if frame_bits(u8, 95) % 8 and R.encode_u8(u8, 95).endswith(b"\xff\x00\xff\xd9"):
            return u8
    raise LookupError("no padded 0xFF")


FF_STRIP_BLOCKS = 300


def _ff_candidates():
    for seed in range(1, 33):
        s = unstuffed(R.pil_encode(strip(seed, FF_STRIP_BLOCKS, FF_STRIP_BLOCKS + 1), STRIP_Q))
        for p0 in [i for i, b in enumerate(s[:-8]) if b == 0xFF]:
            yield seed, p0


def _moved(seed, m):
    """Four leading blocks of 128 are 24 bits (`00` `1010` each): 4 m of them move the noise's stream by 3 m whole bytes."""
    return strip(seed, FF_STRIP_BLOCKS, 4 * m + FF_STRIP_BLOCKS + 1, lead=4 * m)


@functools.lru_cache(None)
def ff_at_chunk_end():
    """-> (u8, p): a strip whose unstuffed byte p = 16383, the last of the stuffing kernel's first chunk, is 0xFF, and whose stream
    goes on behind it.  The search is over seeds and over the 0xFF bytes of the seed's noise strip, moved by leading blocks."""
    for seed, p0 in _ff_candidates():
        m, rest = divmod(CHUNK - 1 - p0, 3)
        if p0 < CHUNK and rest == 0 and 4 * m + FF_STRIP_BLOCKS + 1 <= 8191:
            return _moved(seed, m), CHUNK - 1
    raise LookupError("no 0xFF to move to the end of a chunk")


@functools.lru_cache(None)
def ff_at_thread_end():
    """-> (u8, p): unstuffed byte p is 0xFF, the last of a thread's 16 (p % 16 == 15) and not the last of a chunk"""
    for seed, p0 in _ff_candidates():
        for m in range(16):
            p = p0 + 3 * m
            if p % 16 == 15 and p % CHUNK != CHUNK - 1:
                return _moved(seed, m), p
    raise LookupError("no 0xFF to move to the end of a thread's bytes")


FF_SEEDS = 300
FF_W, FF_H = 4096, 8


def binary_noise(seed, w, h):
    return (np.random.RandomState(seed).randint(0, 2, (h, w)) * 255).astype(np.uint8)


def densest_window(stream, width=CHUNK):
    """the most 0xFF bytes in any `width` consecutive bytes of the unstuffed stream"""
    ff = np.concatenate([[0], np.cumsum(np.frombuffer(stream, np.uint8) == 0xFF)])
    if len(stream) <= width:
        return int(ff[-1])
    return int((ff[width:] - ff[:-width]).max())


@functools.lru_cache(None)
def densest_ff():
    """-> (u8, count): among FF_SEEDS frames of 0/255 noise at quality 100, the one whose densest 16384-byte window holds the most
    0xFF bytes"""
    best = (-1, None)
    for seed in range(FF_SEEDS):
        n = densest_window(unstuffed(R.pil_encode(binary_noise(seed, FF_W, FF_H), 100)))
        if n > best[0]:
            best = (n, seed)
    return binary_noise(best[1], FF_W, FF_H), best[0]


# ---------------------------------------------------------------------------------------------------- item 4: directed blocks

_k = np.arange(8)
_BASIS = np.sqrt(0.25) * np.cos((2 * _k[None, :] + 1) * _k[:, None] * np.pi / 16)  # [u, x], orthonormal DCT-II
_BASIS[0] /= np.sqrt(2)


def block_of(zz, quality):
    """8x8 pixels of a block with the quantised coefficients zz (64, zigzag): dequantised, float inverse DCT, + 128, rounded,
    clipped.  What the encoder finds in it is asked of R.coefficients, not assumed."""
    nat = np.zeros(64)
    nat[R.ZIGZAG] = np.asarray(zz, np.float64)
    f = (nat * R.quant_table(quality)).reshape(8, 8)  # [v, u]
    return np.clip(np.rint(_BASIS.T @ f @ _BASIS + 128), 0, 255).astype(np.uint8)


def square_block(position, amplitude):
    """128 +- amplitude with the sign of the basis function of zigzag `position`: the largest coefficient 8 bits can hold there"""
    nat = int(R.ZIGZAG[position])
    s = np.sign(np.outer(_BASIS[nat // 8], _BASIS[nat % 8]))
    return np.clip(np.rint(128 + amplitude * s), 0, 255).astype(np.uint8)


def row_of(blocks):
    return np.concatenate(blocks, axis=1)


def single(position, value):
    zz = np.zeros(64, np.int64)
    zz[position] = value
    return zz


@functools.lru_cache(None)
def run_frames():
    """-> {quality: u8 strip}: one coefficient at zigzag 63 / 62 alone, at 16, 17, 32, 33, 48, 49 (zero runs of 15, 16, 31, 32,
    47, 48 in front), pairs with every run 0..15 between them, and a block with all 63 AC coefficients non-zero -- at quality
    50, where the rounding of the pixels quantises away"""
    blocks = [block_of(single(p, s), 50) for p in (63, 62, 16, 17, 32, 33, 48, 49) for s in (1, -1)]
    for r in range(16):
        zz = single(1, 2)
        zz[2 + r] = -1 if r % 2 else 1
        blocks.append(block_of(zz, 50))
    rng = np.random.RandomState(5)
    dense = rng.choice([-3, 3], 64)
    dense[0] = 0
    return {50: row_of(blocks), 100: row_of([block_of(dense, 100), block_of(-dense, 100)])}


SYMBOL_QUALITIES = (50, 75, 90, 100)


@functools.lru_cache(None)
def symbol_frames():
    """-> ({quality: u8 strip}, set of run / size symbols): a bounded greedy search for as many distinct AC symbols as 8-bit pixels give.
    Candidates per quality: one coefficient of every size 1..10 and sign at every run 0..15 (sizes 9 and 10 at quality 100 in many
    magnitudes: the rounding of the pixels leaves stray +-1 there, and few magnitudes keep the run clean), the same behind a first coefficient,
    and the square waves of the first 20 basis functions (sizes 9 and 10).  A candidate is kept if its block, as R.coefficients
    finds it, uses a symbol, or a symbol with a sign, not reached before."""
    frames, reached = {}, set()
    for q in SYMBOL_QUALITIES:
        cands = []
        for r in range(16):
            for s in range(1, 11):
                for sign in (1, -1):
                    for mag in [(1 << s) - 1] + list(range(1 << (s - 1), (1 << s) - 1, (3 if s == 10 else 41) if s >= 9 and q == 100 else 1 << s)):
                        cands.append(block_of(single(r + 1, sign * mag), q))
                        zz = single(1, -sign)
                        zz[r + 2] = sign * mag
                        cands.append(block_of(zz, q))
        if q == 100:
            for p in range(1, 21):
                for amp in (127, 100, 64):
                    cands += [square_block(p, amp), square_block(p, -amp)]
        k = walk(R.coefficients(row_of(cands), q))  # (walk's DC differences are not looked at: they are no AC symbols)
        code = ((((k["run"] & 15) << 4) | category(k["v"])) << 1 | (k["v"] < 0)).tolist()  # symbol and sign
        ends = np.searchsorted(k["bi"], np.arange(len(cands) + 1))
        kept = []
        for i in range(len(cands)):
            new = set(code[ends[i]:ends[i + 1]]) - reached
            if new:
                reached |= new
                kept.append(cands[i])
        if kept:
            frames[q] = row_of(kept)
    return frames, frozenset(c >> 1 for c in reached)


def dc_block(dc):
    """a block whose DC coefficient at quality 100 is dc (-1024..1016): flat, with dc * 8 % 64 pixels one higher"""
    s = 8 * dc
    b = np.full(64, 128 + s // 64, np.int64)
    b[:s % 64] += 1
    assert 0 <= b.min() and b.max() <= 255
    return b.reshape(8, 8).astype(np.uint8)


def dc_frames():
    """24 frames of 24x8 at quality 100.  Frame (s, sign): first block at DC a = sign * 2^(s - 1) (-1024 for s = 11 and sign -;
    +1016, size 10, for sign +: 8-bit pixels give no first difference of size +11), then a block at a - sign * m, then a again:
    differences -sign * m and sign * m with m = 2^s - 1 (2040 for s = 11)."""
    out = []
    for s in range(12):
        for sign in (1, -1):
            if s < 11:
                a = sign * (1 << s >> 1)
                b = a - sign * ((1 << s) - 1)
            else:
                a, b = (1016, -1024) if sign > 0 else (-1024, 1016)
            out.append(row_of([dc_block(a), dc_block(b), dc_block(a)]))
    return out


# ---------------------------------------------------------------------------------------------------- item 1: stale words

@functools.lru_cache(None)
def shorter_by_words():
    """-> (a, {d: b_d}, bits): 640x480 noise a at quality 100 and, for d = 1, 2, 3, the same frame with its last block faded
    towards 128 until the stream is d 32-bit words shorter (nbits >> 5)."""
    w, h, q = 640, 480, 100
    a = R.to_u8(R.content("noise", w, h))
    tail = a[h - 8:, w - 16:].astype(np.float64)  # the last two blocks: the DC predictor and the block that varies
    bits_a = frame_bits(a, q)
    last_a = int(block_bits(R.coefficients(a[h - 8:, w - 16:], q))[1])
    found, bits = {}, {0: bits_a}
    for step in range(1, 400):
        t = tail.copy()
        t[:, 8:] = np.rint(128 + (tail[:, 8:] - 128) * (1 - step / 400.0))
        t = t.astype(np.uint8)
        n = bits_a - last_a + int(block_bits(R.coefficients(t, q))[1])
        d = (bits_a >> 5) - (n >> 5)
        if d in (1, 2, 3) and d not in found:
            b = a.copy()
            b[h - 8:, w - 16:] = t
            found[d], bits[d] = b, n
        if len(found) == 3:
            return a, found, bits
    raise LookupError("no frame 1, 2 and 3 words shorter: %r" % sorted(found))


# ---------------------------------------------------------------------------------------------------- item 5: shapes

SHAPES_PIL = [(65500, 1), (1, 65500)]
SHAPES_RESTATED = [(65535, 1), (1, 65535), (65535, 8), (9, 65535)]
SHAPES_GRID = [(2048, 8), (2056, 16), (248, 8), (256, 8), (264, 8), (264, 248), (256, 256), (328, 200)] + [(w, 64) for w in range(1, 8)] + \
    [(57, 24), (63, 24), (65, 24), (71, 24)]  # bw = 8 (57, 63) and 9 (65, 71): a wave's 8 blocks straddle two block rows
SHAPE_CONTENTS = ["noise", "ramp"]
QUALITIES = [1, 2, 24, 25, 49, 50, 51, 99]


def nblocks(w, h):
    return ((w + 7) // 8) * ((h + 7) // 8)


# ---------------------------------------------------------------------------------------------------- item 6: limits of mdcj_create

BIG = 12544  # 1568 x 1568 blocks


def largest_accepted():
    """-> (bw, bh): the most blocks bw x bh (both <= 8191) with 1024 + 416 * bw * bh <= 2^30"""
    top = ((1 << 30) - 1024) // 416
    return max(((bw, min(top // bw, 8191)) for bw in range(316, 8192)), key=lambda p: p[0] * p[1])


def smallest_refused():
    """-> (bw, bh): the fewest blocks bw x bh with 1024 + 416 * bw * bh > 2^30"""
    top = ((1 << 30) - 1024) // 416
    return min(((bw, top // bw + 1) for bw in range(316, 8192) if top // bw + 1 <= 8191), key=lambda p: p[0] * p[1])


# ---------------------------------------------------------------------------------------------------- item 7: values

def special2(w, h):
    """values far outside 8 bits among ordinary pixels: |v| >= 2^31, the ends of the float range, denormals, both NaN signs, ties"""
    f = np.random.RandomState(7).uniform(-40, 300, (h, w)).astype(np.float32)
    flat = f.reshape(-1)
    fmax = np.finfo(np.float32).max
    vals = np.array([3e9, -3e9, 1e38, -1e38, fmax, -fmax, 1e-45, -1e-45, 1e-39, np.nan, -np.nan, 254.5, 255.5, 2147483648.0, -2147483648.0, 4294967296.0], np.float32)
    vals[10] = np.array([0xFFC00000], np.uint32).view(np.float32)[0]  # -nan: the sign bit set
    flat[::2] = vals[np.arange(flat[::2].size) % vals.size]
    return f
