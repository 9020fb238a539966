"""The inputs of tests/test_pngd_sizes.py: zlib streams written symbol by symbol, so that the device PNG decoder (include/mdc_pngd.h)
meets what zlib's own encoder rarely or never emits -- matches at chosen distances and lengths, codes of 15 bits in both alphabets, a
distance code of one bit, chains of stored blocks at their limit, bytes after the trailer, a filter type that only a late row has,
Adler sums of many large terms, single-bit damage -- and the eight small streams, one of each kind, that a workgroup decodes one
after the other.  Every case is (name, w, h, stream, reason, path): what the restatement (tests/pngd_restatement.py) has to give.
tests/test_pngd_sizes_cpu.py pins all of it to zlib and PIL and runs it through the kernels' core under the sanitizers."""
import functools
import struct
import zlib

import numpy as np

import pngd_restatement as R
import pngw_restatement as P

# ------------------------------------------------------------------------------------------------ blocks from symbols
# ops: an int is a literal, (distance, length) a match, ("length", n) the length part of a match alone, ("bits", value, count) raw bits


def length_symbol(n):
    """-> (symbol, extra value, extra bits): the symbol with the largest base not above n"""
    i = max(k for k in range(29) if R.LENGTH_BASE[k] <= n)
    assert 3 <= n <= 258 and n - R.LENGTH_BASE[i] < 1 << R.LENGTH_EXTRA[i]
    return 257 + i, n - R.LENGTH_BASE[i], R.LENGTH_EXTRA[i]


def distance_symbol(d):
    i = max(k for k in range(30) if R.DIST_BASE[k] <= d)
    assert 1 <= d <= 32768 and d - R.DIST_BASE[i] < 1 << R.DIST_EXTRA[i]
    return i, d - R.DIST_BASE[i], R.DIST_EXTRA[i]


def _symbols(bits, out, ops, lit_lengths, dist_lengths):
    lit_codes, dist_codes = P.canonical_codes(list(lit_lengths)), P.canonical_codes(list(dist_lengths))

    def put(lengths, codes, s):
        assert s < len(lengths) and lengths[s], "symbol %d has no code" % s
        bits.put_code(codes[s], lengths[s])

    for op in ops:
        if isinstance(op, int):
            put(lit_lengths, lit_codes, op)
            out.append(op)
        elif op[0] == "bits":
            bits.put(op[1], op[2])
        else:
            s, extra, nextra = length_symbol(op[1])
            put(lit_lengths, lit_codes, s)
            bits.put(extra, nextra)
            if op[0] == "length":
                continue
            d, n = op
            s, extra, nextra = distance_symbol(d)
            put(dist_lengths, dist_codes, s)
            bits.put(extra, nextra)
            assert d <= len(out), "distance %d after %d bytes" % (d, len(out))
            for _ in range(n):
                out.append(out[-d])
    put(lit_lengths, lit_codes, 256)


def _emit(bits, out, block, final):
    kind = block[0]
    bits.put(int(final), 1)
    if kind == "stored":
        data = bytes(block[1])
        bits.put(0, 2)
        bits.put(0, -bits.n % 8)
        bits.put(len(data), 16)
        bits.put(len(data) ^ 0xffff, 16)
        for v in data:
            bits.put(v, 8)
        out += data
    elif kind == "fixed":
        bits.put(1, 2)
        _symbols(bits, out, block[1], R.FIXED_LIT, [5] * 30)
    else:
        _, lit_lengths, dist_lengths, ops = block
        hlit, hdist = len(lit_lengths), len(dist_lengths)
        assert 257 <= hlit <= 286 and 1 <= hdist <= 30
        pairs = P.run_length_code(list(lit_lengths) + list(dist_lengths))
        clhist = [0] * 19
        for s, _ in pairs:
            clhist[s] += 1
        cllen = P.huffman_lengths(clhist, 7)
        clcodes = P.canonical_codes(cllen)
        hclen = max([4] + [i + 1 for i in range(19) if cllen[P.CL_ORDER[i]]])
        bits.put(2, 2)
        bits.put(hlit - 257, 5)
        bits.put(hdist - 1, 5)
        bits.put(hclen - 4, 4)
        for i in range(hclen):
            bits.put(cllen[P.CL_ORDER[i]], 3)
        for s, extra in pairs:
            bits.put_code(clcodes[s], cllen[s])
            if s >= 16:
                bits.put(extra, {16: 2, 17: 3, 18: 7}[s])
        _symbols(bits, out, ops, lit_lengths, dist_lengths)


def _bytes(bits):
    return bits.value.to_bytes((bits.n + 7) // 8, "little")


def deflate(blocks, check=True):
    """blocks: ("stored", bytes) | ("fixed", ops) | ("dynamic", literal/length code lengths, distance code lengths, ops), the last one
    final -> (the DEFLATE stream, the bytes it decodes to); zlib has to read the same bytes from it"""
    bits, out = P.Bits(), bytearray()
    for k, block in enumerate(blocks):
        _emit(bits, out, block, k == len(blocks) - 1)
    body, out = _bytes(bits), bytes(out)
    if check:
        assert zlib.decompress(R.zstream(out, body)) == out
    return body, out


def _one_block(block, final, before, check):
    bits, out = P.Bits(), bytearray(before)
    _emit(bits, out, block, final)
    if check:  # wrapped: what came before as a stored block, an empty final block behind a block that is not final
        _, whole = deflate(([("stored", before)] if before else []) + [block] + ([] if final else [("fixed", [])]))
        assert whole == bytes(out)
    return _bytes(bits), bytes(out[len(before):])


def fixed_block(ops, final, before=b""):
    """one block with the fixed codes, from bit 0 of its first byte -> (bytes, the bytes it decodes to after `before`)"""
    return _one_block(("fixed", ops), final, before, True)


def dynamic_block(lit_lengths, dist_lengths, ops, final, before=b"", check=True):
    """one dynamic block; HLIT and HDIST are the lengths of the two lists.  check=False: a block zlib is meant to refuse"""
    return _one_block(("dynamic", list(lit_lengths), list(dist_lengths), ops), final, before, check)


def walk(data):
    """[(block type, the output bytes before the block, [literal | (distance, length)])] of a valid stream, by the restatement's readers"""
    r, pos, blocks = R.Reader(bytes(data), 16), 0, []
    while True:
        hdr = r.take(3)
        btype, start, ops = hdr >> 1, pos, []
        if btype == 0:
            r.pos = (r.pos + 7) & ~7
            n = r.take(32) & 0xffff
            r.pos += 8 * n
            pos += n
        else:
            lit, dist = (R.make_code(R.FIXED_LIT), R.make_code([5] * 32)) if btype == 1 else R.dynamic_header(r)[:2]
            while True:
                s = R.symbol(lit, r)
                if s == 256:
                    break
                if s < 256:
                    ops.append(s)
                    pos += 1
                    continue
                n = R.LENGTH_BASE[s - 257] + r.take(R.LENGTH_EXTRA[s - 257])
                d = R.symbol(dist, r)
                ops.append((R.DIST_BASE[d] + r.take(R.DIST_EXTRA[d]), n))
                pos += n
        blocks.append((btype, start, ops))
        if hdr & 1:
            return blocks


def one_row(name, body, raw, reason=R.OK, path=R.GENERAL):
    """a case whose filtered bytes are one row: its type byte (0) and w = F - 1 pixels"""
    assert raw[0] == 0 and 2 <= len(raw) <= 65536
    return name, len(raw) - 1, 1, R.zstream(raw, body), reason, path


# ------------------------------------------------------------------------------------------------ matches the whole wave copies

GRID_DISTANCES = (1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 257, 258, 259)
GRID_LENGTHS = (3, 4, 10, 63, 64, 65, 66, 127, 128, 129, 130, 257, 258)


@functools.lru_cache(maxsize=None)
def match_grid():
    """per distance d one fixed-Huffman stream: the type byte, d literals, then for every length n the match (d, n) and a fresh literal --
    so that the next match's source ends in the byte lane 0 has just stored, and every match longer than d overlaps itself"""
    out = []
    for d in GRID_DISTANCES:
        ops = [0] + [1 + (37 * i) % 251 for i in range(d)]  # (no period below d: 37 and 251 are coprime)
        for k, n in enumerate(GRID_LENGTHS):
            ops += [(d, n), 252 + k % 4]  # 252..255: in no run of literals above
        body, raw = deflate([("fixed", ops)])
        out.append(one_row("grid_distance_%d" % d, body, raw))
    return out


def two_block_code():
    """a small dynamic code: literals 0..15, end-of-block, lengths 3..6 and 258; distances 1..4, 9..16 and 49..64"""
    hist = [0] * 286
    for s, c in zip(list(range(16)) + [256, 257, 258, 259, 260, 285], (9, 8, 7, 9, 6, 5, 9, 4, 8, 7, 6, 5, 9, 3, 2, 8, 1, 12, 5, 3, 2, 6)):
        hist[s] = c
    dist = [0] * 12
    for s, c in zip((0, 1, 2, 3, 6, 7, 11), (3, 1, 4, 1, 5, 9, 2)):
        dist[s] = c
    return P.huffman_lengths(hist, 15), P.huffman_lengths(dist, 15)


@functools.lru_cache(maxsize=None)
def cross_block_matches():
    """a match whose source another block wrote: stored() before a fixed block, an earlier dynamic block, zlib's own across a flush"""
    out = []
    first = bytes([0] + [(11 * i + 3) % 256 for i in range(99)])
    body, raw = deflate([("stored", first), ("fixed", [(100, 100)])])
    assert raw == first + first
    out.append(one_row("stored_then_match_100_100", body, raw))
    ll, dl = two_block_code()
    a = [0] + [(5 * i + 1) % 16 for i in range(40)] + [(3, 6), 7, (16, 258)]
    b = [(50, 258), 3, (64, 5), (1, 3), 9, (2, 4)]  # the first symbol of the block reaches 50 bytes into the block before it
    body, raw = deflate([("dynamic", ll, dl, a), ("dynamic", ll, dl, b)])
    blocks = walk(R.zstream(raw, body))
    assert [t for t, _, _ in blocks] == [2, 2] and blocks[1][2][0] == (50, 258) and blocks[1][1] > 258
    out.append(one_row("two_dynamic_blocks", body, raw))
    half = np.random.default_rng(21).integers(0, 256, 400, dtype=np.uint8)
    half[0] = 0
    raw = half.tobytes() * 2
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    body = co.compress(raw[:450]) + co.flush(zlib.Z_SYNC_FLUSH) + co.compress(raw[450:]) + co.flush()
    blocks = walk(R.zstream(raw, body))
    last_type, last_start, last_ops = blocks[-1]
    at, crossing = last_start, []
    for op in last_ops:
        if not isinstance(op, int):
            if op[0] > at - last_start:
                crossing.append(op)
            at += op[1] - 1
        at += 1
    assert len(blocks) == 3 and blocks[1][0] == 0 and last_start == 450 and crossing and crossing[0][0] == 400, blocks  # over the flush
    out.append(one_row("zlib_match_over_a_sync_flush", body, raw))
    return out


# ------------------------------------------------------------------------------------------------ codes past the fast table

DEEP_LITERALS = (0, 1, 2, 3, 4) + tuple(10 + 12 * k for k in range(15))
DEEP_LENGTHS = (257, 259, 264, 265, 270, 275, 280, 284, 285)  # no extra bits, 1 .. 5 extra bits, 258
DEEP_DISTANCES = (0, 1, 2, 3, 4, 5, 7, 8, 10, 11, 13, 14, 16, 17, 19, 20, 23, 26, 28, 29)
FAST_BITS = 9  # csrc/png_inflate_core.h, kFastBits: longer codes are found by walking the counts


def deep_code_lengths():
    """-> (literal/length code lengths, distance code lengths): Fibonacci counts over 30 and 20 symbols, in a seeded order"""
    rng = np.random.default_rng(15)
    hist = [0] * 286
    for s, c in zip(rng.permutation(DEEP_LITERALS + (256,) + DEEP_LENGTHS), P.fibonacci(30)):
        hist[int(s)] = c
    dist = [0] * 30
    for s, c in zip(rng.permutation(DEEP_DISTANCES), P.fibonacci(20)):
        dist[int(s)] = c
    return P.huffman_lengths(hist, 15), P.huffman_lengths(dist, 15)


def small_code():
    hist = [0] * 286
    for s, c in zip(list(range(8)) + [256, 258, 285], (10, 9, 8, 10, 7, 6, 10, 5, 1, 5, 3)):
        hist[s] = c
    return P.huffman_lengths(hist, 15)


@functools.lru_cache(maxsize=None)
def deep_codes():
    out = []
    ll, dl = deep_code_lengths()
    used = [l for l in ll if l], [l for l in dl if l]
    for lengths in used:  # both codes reach 15 bits and use almost every length on the way
        assert max(lengths) == 15 and len(set(lengths)) >= 13, sorted(lengths)
    assert max(ll[s] for s in DEEP_LITERALS) > FAST_BITS and max(ll[s] for s in DEEP_LENGTHS) > FAST_BITS and min(ll[s] for s in DEEP_LENGTHS) <= FAST_BITS
    ops, size = list(DEEP_LITERALS), len(DEEP_LITERALS)
    for k, s in enumerate(DEEP_LENGTHS):  # every length symbol, with its largest extra value
        n = R.LENGTH_BASE[s - 257] + (1 << R.LENGTH_EXTRA[s - 257]) - 1
        ops += [((1, 2, 3, 4, 5, 7, 13, 17, 19)[k], n), DEEP_LITERALS[k + 1]]
        size += n + 1
    back, k = 19, 0
    for d in DEEP_DISTANCES:  # every distance symbol, once the output is long enough for it
        lo = R.DIST_BASE[d]
        while size < lo:  # grow by copies at the last distance, a literal between them so that the phase moves
            ops += [(back, 258), DEEP_LITERALS[k % 20]]
            size, k = size + 259, k + 1
        back = min(lo + (1 << R.DIST_EXTRA[d]) - 1, size)
        s = DEEP_LENGTHS[k % 9]
        n = R.LENGTH_BASE[s - 257] + k % (1 << R.LENGTH_EXTRA[s - 257])
        ops += [(back, n), DEEP_LITERALS[k % 20]]
        size, k = size + n + 1, k + 1
    body, raw = deflate([("dynamic", ll, dl, ops)])
    met_l, met_d = set(), set()
    for _, _, block in walk(R.zstream(raw, body)):
        for op in block:
            if isinstance(op, int):
                met_l.add(op)
            else:
                met_l.add(length_symbol(op[1])[0])
                met_d.add(distance_symbol(op[0])[0])
    assert met_l == set(DEEP_LITERALS + DEEP_LENGTHS) and met_d == set(DEEP_DISTANCES) and len(raw) == size
    out.append(one_row("fibonacci_codes_15_bits", body, raw))
    # a distance code of one symbol, one bit long: incomplete, and valid by zlib's rule
    ll = small_code()
    ops = [0, 1, 2, 3, 4, 5, 6, 7, (4, 4), (4, 258), 3, (4, 4)]
    body, raw = deflate([("dynamic", ll, [0, 0, 0, 1], ops)])
    out.append(one_row("one_distance_code_of_one_bit", body, raw))
    # ... and the bit that is no code of it: fifteen bits are read before the decoder knows
    body, _ = dynamic_block(ll, [0, 0, 0, 1], [0, 1, 2, 3, 4, 5, 6, 7, ("length", 4), ("bits", 1, 1), 3, 5], True, check=False)
    out.append(("the_other_one_bit_distance_code", len(raw) - 1, 1, R.zstream(raw, body), R.UNDEFINED_SYMBOL, R.GENERAL))
    # no distance code at all, so the parallel path tries it; a length symbol has a code and is used
    hist = [0] * 258
    for s, c in zip(list(range(8)) + [256, 257], (10, 9, 8, 10, 7, 6, 10, 5, 1, 4)):
        hist[s] = c
    body, _ = dynamic_block(P.huffman_lengths(hist, 15), [0], [0, 1, 2, 3, ("length", 3), 4, 5, 6, 7, 0, 1], True, check=False)
    s = R.zstream(raw, body)
    assert R.first_path(s, len(raw)) == R.PARALLEL
    out.append(("length_symbol_in_a_literal_only_block", len(raw) - 1, 1, s, R.UNDEFINED_SYMBOL, R.GENERAL))
    return out


# ------------------------------------------------------------------------------------------------ stored chains


def stored_block(data, final):
    return struct.pack("<BHH", int(final), len(data), len(data) ^ 0xffff) + bytes(data)


@functools.lru_cache(maxsize=None)
def stored_chains():
    out = []
    for nblk, path in ((63, R.STORED), (64, R.STORED), (65, R.GENERAL)):  # R.MAX_STORED_BLOCKS and its neighbours
        rows = np.random.default_rng(nblk).integers(0, 5, (nblk, 4), dtype=np.uint8)
        body = b"".join(stored_block(rows[y].tobytes(), y == nblk - 1) for y in range(nblk))
        out.append(("stored_%d_blocks" % nblk, 3, nblk, R.zstream(rows.tobytes(), body), R.OK, path))
    raw = P.filtered(R.test_image(40, 12, 31), 8, P.ADAPTIVE).tobytes()
    half = len(raw) // 2
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    out.append(("stored_then_compressed", 40, 12, R.zstream(raw, stored_block(raw[:half], False) + co.compress(raw[half:]) + co.flush()), R.OK, R.GENERAL))
    rows = np.random.default_rng(66).integers(0, 5, (64, 4), dtype=np.uint8)
    body = b"".join(stored_block(rows[y].tobytes(), False) for y in range(64)) + b"\x03\x00"  # final, fixed, end-of-block
    out.append(("stored_64_blocks_then_an_empty_final_block", 3, 64, R.zstream(rows.tobytes(), body), R.OK, R.GENERAL))
    return out


# ------------------------------------------------------------------------------------------------ after the trailer, late rows, large sums


def three_kinds(raw):
    return (("literal", R.literal_stream(raw), R.PARALLEL), ("stored", R.stored_stream(raw), R.STORED), ("zlib", R.zstream(raw), R.GENERAL))


@functools.lru_cache(maxsize=None)
def trailing_bytes():
    """bytes after the Adler-32 are ignored: one, 8000 seeded random ones, 8000 zero bytes.  On the parallel path the threads behind the
    end-of-block decode them as symbols until the end state reaches them, one subsequence a round.  Random bits hold the end-of-block
    code every few hundred symbols, and behind it the state is the end state already; zero bits are one literal's code for ever, so
    that the end state has to cross every subsequence of them itself"""
    raw = P.filtered(R.test_image(40, 12, 3), 8, P.ADAPTIVE).tobytes()
    out = []
    for kind, s, path in three_kinds(raw):
        for name, junk in (("1_byte", b"\x5c"), ("8000_bytes", np.random.default_rng(8000).integers(0, 256, 8000, dtype=np.uint8).tobytes()), ("8000_zero_bytes", bytes(8000))):
            out.append(("%s_and_%s" % (kind, name), 40, 12, s + junk, R.OK, path))
    return out


LATE_ROWS = (0, 255, 256, 299)  # the check kernel's 256 threads scan the rows 256 apart


@functools.lru_cache(maxsize=None)
def late_filter_types():
    out = []
    for row in LATE_ROWS:
        rows = np.random.default_rng(row).integers(0, 256, (300, 4), dtype=np.uint8)
        rows[:, 0] = np.arange(300) % 5
        rows[row, 0] = 5
        for kind, s, path in three_kinds(rows.tobytes()):
            out.append(("type_5_in_row_%d_%s" % (row, kind), 3, 300, s, R.FILTER_TYPE, path))
    return out


HEAVY_W, HEAVY_H = 1023, 1024


def heavy_raw():
    rows = np.full((HEAVY_H, 1 + HEAVY_W), 255, np.uint8)
    rows[:, 0] = np.arange(HEAVY_H) % 3
    return rows.tobytes()


@functools.lru_cache(maxsize=None)
def heavy_adler():
    """2^20 filtered bytes, all of them 0xFF but the type bytes: the largest terms the check kernel's sums can be given per byte"""
    raw = heavy_raw()
    return [("heavy_stored", HEAVY_W, HEAVY_H, R.stored_stream(raw), R.OK, R.STORED), ("heavy_literal", HEAVY_W, HEAVY_H, R.literal_stream(raw), R.OK, R.PARALLEL)]


# ------------------------------------------------------------------------------------------------ single-bit damage

MUTATION_SEED, MUTATION_COUNT = 1, 1024


def mixed_good():
    """the four good streams of tests/test_pngd.py's mixed batch"""
    raw = P.filtered(R.test_image(40, 12, 3), 8, P.ADAPTIVE).tobytes()
    return [("literal", R.literal_stream(raw)), ("stored", R.stored_stream(raw)), ("zlib", R.zstream(raw)), ("fixed", R.zstream(raw, strategy=zlib.Z_FIXED))]


@functools.lru_cache(maxsize=None)
def mutations(seed=MUTATION_SEED, count=MUTATION_COUNT):
    """the four good 40 x 12 streams in turn, one bit flipped at a seeded position; reason and path are what the restatement gives"""
    good = mixed_good()
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        kind, s = good[k % 4]
        bit = int(rng.integers(0, 8 * len(s)))
        s = bytearray(s)
        s[bit >> 3] ^= 1 << (bit & 7)
        reason, path, _ = R.decode(bytes(s), 40, 12, pixels=False)
        out.append(("%s_bit_%d" % (kind, bit), 40, 12, bytes(s), reason, path))
    return out


# ------------------------------------------------------------------------------------------------ one workgroup, image after image

CYCLE_W, CYCLE_H = 5, 3


@functools.lru_cache(maxsize=None)
def class_cycle():
    """eight streams of eight images: four valid ones, one per path and kind of table, and four refused ones"""
    w, h = CYCLE_W, CYCLE_H
    raws = [P.filtered(R.test_image(w, h, 50 + k), 8, 0).tobytes() for k in range(8)]
    near = np.full((h, w), 200, np.uint8)
    near[1, 3] = 17
    raws[2] = P.filtered(near, 8, 0).tobytes()
    two = np.where(R.test_image(w, h, 53) & 1, 9, 250).astype(np.uint8)  # two values: zlib's dynamic block is its shortest
    raws[3] = P.filtered(two, 8, 0).tobytes()
    assert len(set(raws)) == 8
    out = [("literal", w, h, R.literal_stream(raws[0]), R.OK, R.PARALLEL), ("stored", w, h, R.stored_stream(raws[1]), R.OK, R.STORED)]
    s = R.zstream(raws[2])
    assert any(not isinstance(op, int) for _, _, ops in walk(s) for op in ops)  # it holds matches
    out.append(("zlib_with_matches", w, h, s, R.OK, R.GENERAL))
    s = R.zstream(raws[3], strategy=zlib.Z_HUFFMAN_ONLY)
    assert [t for t, _, _ in walk(s)] == [2]  # one block with a table of its own -- and two distance codes, so not the parallel path's
    out.append(("huffman_only", w, h, s, R.OK, R.GENERAL))
    lit = bytearray(R.literal_stream(raws[4]))
    lit[-6] ^= 0x10  # in the last symbols
    reason, path, _ = R.decode(bytes(lit), w, h, pixels=False)
    assert reason != R.OK
    out.append(("literal_bit_flipped", w, h, bytes(lit), reason, path))
    out.append(("bad_zlib_header", w, h, b"\x78\x02" + R.zstream(raws[5])[2:], R.ZLIB_HEADER, R.GENERAL))
    sto = bytearray(R.stored_stream(raws[6]))
    sto[12] ^= 0x20
    out.append(("stored_byte_flipped", w, h, bytes(sto), R.ADLER, R.STORED))
    z = R.zstream(raws[7])
    out.append(("cut_in_the_symbols", w, h, z[:len(z) // 2], R.TRUNCATED, R.GENERAL))
    return out


def cycle_class(f, reverse=False):
    """the class of frame f: workgroup b of 8192 meets class b % 8, then b // 8 % 8, then b // 64 % 8"""
    c = (f % 8192) // 8 ** (f // 8192) % 8
    return 7 - c if reverse else c


CYCLE_FRAMES = 2 * 8192 + 64

# ------------------------------------------------------------------------------------------------ stream placement

CLAMP_SLOT = 301  # a slot that holds the mixed batch's zlib and literal streams and cuts its fixed and stored ones (and is no multiple of 4)
SLOT_FILL = 0xA5  # what tests/test_pngd.py fills the slots with behind a stream


def mixed_batch():
    """[(name, stream, reason)]: tests/test_pngd.py's mixed batch of 40 x 12 streams"""
    good = mixed_good()
    out = []
    for k, c in enumerate(R.damaged_cases()):
        out.append((c[0], c[3], c[4]))
        out.append(good[k % 4] + (0,))
    return out


@functools.lru_cache(maxsize=None)
def clamped():
    """the mixed batch as a decoder sees it when every slot has CLAMP_SLOT bytes and every size says more: each stream is its whole slot,
    cut there or followed by the fill bytes"""
    out = []
    for k, (name, s, _) in enumerate(mixed_batch()):
        s = (s + bytes([SLOT_FILL]) * CLAMP_SLOT)[:CLAMP_SLOT]
        reason, path, _ = R.decode(s, 40, 12, pixels=False)
        out.append(("clamped_%d_%s" % (k, name), 40, 12, s, reason, path))
    return out


def all_cases():
    """every stream tests/test_pngd_sizes.py sends, the 2^20-byte pair last"""
    return (match_grid() + cross_block_matches() + deep_codes() + stored_chains() + trailing_bytes() + late_filter_types() + mutations() + class_cycle() + clamped()
            + heavy_adler())
