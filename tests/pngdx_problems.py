"""The inputs of the device PNG decoder with the parallel inflate (include/mdc_pngdx.h, libmdc_pngdx.so) and what it must make of
them.  Plain functions: tests/test_pngdx_cpu.py runs them through the core program, tests/test_pngdx.py through the library.

Expected pixels: PIL's (R.pil_pixels), or zlib.decompress + R.unfilter.  Expected reason: R.decode's, the sequential rule of
tests/pngd_restatement.py.  Expected path: R's where that is PARALLEL or STORED; otherwise TOKENS if the reason is 0; otherwise
GENERAL.  No valid stream may come back with GENERAL."""
import functools
import zlib

import numpy as np

import pngd_restatement as R
import pnglz_restatement as Z
import pngw_restatement as P

TOKENS = 4
SUB_BITS, WINDOW_BITS = 64, 65536
SIZES = ((1, 1), (3, 2), (64, 64), (130, 129))


def expected(w, h, stream, pixels=False):
    """-> (reason, path, pixels or None).  The restatement inflates bit by bit in Python: above 130 x 129 pixels a stream that zlib
    accepts is taken as the reason 0 it is (tests/test_pngd_cpu.py pins the restatement to zlib on valid streams) with the path of
    the restatement's classification, which only reads the first block's header."""
    stream = bytes(stream)
    if w * h > 130 * 129 and R.host_accepts(stream, w, h):
        reason, path = R.OK, R.first_path(stream, h * (1 + w))
    else:
        reason, path, _ = R.decode(stream, w, h, pixels=False)
    if path not in (R.PARALLEL, R.STORED):
        path = TOKENS if reason == R.OK else R.GENERAL
    return reason, path, R.pil_pixels(w, h, stream) if pixels and reason == R.OK else None


def filtered_hash(data):
    """the hash tests/native/pngdx_core.cpp prints of the filtered bytes"""
    return zlib.crc32(bytes(data))


# ------------------------------------------------------------------------------------------------ zlib's streams


def images(w, h):
    rng = np.random.default_rng(1000 * w + h)
    yy, xx = np.mgrid[0:h, 0:w]
    return (("smooth", R.test_image(w, h, w + h), P.ADAPTIVE), ("noise", rng.integers(0, 256, (h, w), dtype=np.uint8), 0),
            ("constant", np.full((h, w), 77, np.uint8), 0), ("periodic", ((xx % 7) * 30 + (yy % 3)).astype(np.uint8), 1))


def deflated(raw, level=6, mem=9, strategy=zlib.Z_DEFAULT_STRATEGY, flush=None):
    """a raw DEFLATE stream of zlib's; flush: that kind of flush after half of the bytes"""
    co = zlib.compressobj(level, zlib.DEFLATED, -15, mem, strategy)
    if flush is None:
        return co.compress(raw) + co.flush()
    half = len(raw) // 2
    return co.compress(raw[:half]) + co.flush(flush) + co.compress(raw[half:]) + co.flush()


VARIANTS = (("level1", dict(level=1)), ("level6", dict(level=6)), ("level9", dict(level=9)), ("mem1", dict(level=6, mem=1)),
            ("fixed", dict(strategy=zlib.Z_FIXED)), ("rle", dict(strategy=zlib.Z_RLE)), ("huffman_mem1", dict(strategy=zlib.Z_HUFFMAN_ONLY, mem=1)),
            ("sync_flush", dict(flush=zlib.Z_SYNC_FLUSH)), ("full_flush", dict(flush=zlib.Z_FULL_FLUSH)), ("partial_flush", dict(flush=zlib.Z_PARTIAL_FLUSH)))


def zlib_cases(w, h, variants=VARIANTS):
    out = []
    for kind, img, filt in images(w, h):
        raw = P.filtered(img, 8, filt).tobytes()
        for name, how in variants:
            out.append(("zlib_%dx%d_%s_%s" % (w, h, kind, name), w, h, R.zstream(raw, deflated(raw, **how))))
    return out


def lz_cases():
    """this project's own compress=lz77 files (tests/pnglz_restatement.py) at every chain length the exports use"""
    out = []
    for w, h in ((64, 64), (130, 129)):
        yy, xx = np.mgrid[0:h, 0:w]
        img = ((xx * 5 + yy * 3 + (xx * yy) // 64) & 255).astype(np.uint8)  # smooth: the match form is the smallest
        for chain in (1, 4, 64):
            f, (form, _, nmatch, _) = Z.encode(img, Z.GRAY8, P.ADAPTIVE, chain)
            assert form == Z.MATCHES and nmatch > 0
            out.append(("pnglz_%dx%d_chain%d" % (w, h, chain), w, h, f[41:-16]))
    return out


# ------------------------------------------------------------------------------------------------ hand-built streams


def canonical(lengths):
    """{symbol: (code, length)} of RFC 1951 3.2.2"""
    count = [0] * 17
    for l in lengths.values():
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * 17
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = {}
    for s in sorted(lengths):
        if lengths[s]:
            out[s] = (nxt[lengths[s]], lengths[s])
            nxt[lengths[s]] += 1
    return out


FIXED_LL = canonical({s: l for s, l in enumerate(R.FIXED_LIT)})
FIXED_D = canonical({s: 5 for s in range(32)})


class Deflater:
    """DEFLATE blocks from tokens: an int is a literal, (length, distance) a match; for damaged streams ("code", (code, bits)) is a
    Huffman code as it stands and ("raw", value, bits) are plain bits.  Keeps the bytes a valid stream decodes to."""

    def __init__(self):
        self.bits, self.raw = [], bytearray()

    def put(self, v, n):  # least significant bit first
        self.bits += [(v >> i) & 1 for i in range(n)]

    def code(self, cn):  # a Huffman code: most significant bit first
        c, n = cn
        self.bits += [(c >> i) & 1 for i in range(n - 1, -1, -1)]

    def tokens(self, toks, ll, d, end=True):
        for t in toks:
            if isinstance(t, tuple) and t[0] == "raw":
                self.put(t[1], t[2])
            elif isinstance(t, tuple) and t[0] == "code":
                self.code(t[1])
            elif isinstance(t, tuple):
                n, back = t
                i = max(k for k in range(29) if R.LENGTH_BASE[k] <= n) if n < 258 else 28
                self.code(ll[257 + i])
                self.put(n - R.LENGTH_BASE[i], R.LENGTH_EXTRA[i])
                j = max(k for k in range(30) if R.DIST_BASE[k] <= back)
                self.code(d[j])
                self.put(back - R.DIST_BASE[j], R.DIST_EXTRA[j])
                for _ in range(n if back <= len(self.raw) else 0):  # (a distance before byte 0: a damaged stream, nothing to keep)
                    self.raw.append(self.raw[-back])
            else:
                self.code(ll[t])
                self.raw.append(t)
        if end:
            self.code(ll[256])
        return self

    def fixed(self, toks, final=False, end=True):
        self.put(int(final), 1)
        self.put(1, 2)
        return self.tokens(toks, FIXED_LL, FIXED_D, end)

    def dynamic(self, toks, ll_len, d_len, final=False):
        """ll_len, d_len: {symbol: length}.  The code-length code gives every length 0 .. 15 four bits and uses no repeat codes."""
        hlit, hdist = max(max(ll_len) + 1, 257), max(max(d_len) + 1, 1)
        self.put(int(final), 1)
        self.put(2, 2)
        self.put(hlit - 257, 5)
        self.put(hdist - 1, 5)
        self.put(19 - 4, 4)
        for s in P.CL_ORDER:
            self.put(4 if s < 16 else 0, 3)
        cl = canonical({s: 4 for s in range(16)})
        for s in range(hlit):
            self.code(cl[ll_len.get(s, 0)])
        for s in range(hdist):
            self.code(cl[d_len.get(s, 0)])
        return self.tokens(toks, canonical(ll_len), canonical(d_len))

    def stored(self, data, final=False):
        self.put(int(final), 1)
        self.put(0, 2)
        self.bits += [0] * (-len(self.bits) % 8)
        self.put(len(data), 16)
        self.put(len(data) ^ 0xffff, 16)
        for b in bytes(data):
            self.put(b, 8)
        self.raw += bytes(data)
        return self

    def body(self):
        return np.packbits(np.array(self.bits, np.uint8), bitorder="little").tobytes()

    def stream(self):
        return R.zstream(bytes(self.raw), self.body())


def row_case(name, d):
    """a one-row image of filter type 0: its filtered bytes are what `d` decodes to"""
    assert d.raw[0] == 0 and 2 <= len(d.raw) <= 65536, name
    return name, len(d.raw) - 1, 1, d.stream()


def noise_literals(n, seed, top=144):
    return [int(v) for v in np.random.default_rng(seed).integers(1, top, n)]


def hand_cases():
    out = []
    # a block of no tokens: first, in the middle and as the final block
    out.append(row_case("empty_blocks", Deflater().fixed([]).fixed([0, 5, 6]).fixed([]).dynamic([], {256: 1}, {0: 1}).fixed([7, (3, 2)]).fixed([], final=True)))
    # the first block's data starts at bit 19 of the stream: 19 + 3 header bits.  Literals below 144 take 8 bits, the end-of-block code 7
    for name, bits in (("subsequence", 2 * SUB_BITS), ("window", WINDOW_BITS)):
        d = Deflater().fixed([0] + noise_literals((bits - 7) // 8 - 2, bits) + [200], final=False)  # 8 (n - 1) + 9 + 7 bits
        assert len(d.bits) == 3 + bits
        out.append(row_case("end_of_block_is_the_last_bit_of_a_%s" % name, d.fixed([1, 2, (4, 3), 9], final=True)))
    # ... and of the stream's last byte, in the final block
    d = Deflater().fixed([0] + noise_literals(12, 5) + [200] * 6, final=True)  # 3 + 8 * 13 + 9 * 6 + 7 bits
    assert len(d.bits) % 8 == 0
    out.append(row_case("end_of_block_is_the_last_bit_of_the_stream", d))
    # a match (8 + 5 + 5 + 13 bits) that starts ten bits before the end of a subsequence, and of a window
    for name, bits in (("subsequence", 3 * SUB_BITS), ("window", WINDOW_BITS)):
        lits = [0] + noise_literals((bits - 10 - 54) // 8 - 1, bits + 1) + [200] * 6
        d = Deflater().fixed(lits + [(258 - 31, len(lits) - 1)] + noise_literals(40, 7), final=True, end=True)
        assert 8 * (len(lits) - 6) + 54 == bits - 10
        out.append(row_case("match_straddles_a_%s" % name, d))
    out.append(row_case("length_258_and_length_3", Deflater().fixed([0, 1, 2, 3, 4, (258, 4), 9, (3, 1), (3, 263), (258, 258)], final=True)))
    out.append(row_case("distance_below_length", Deflater().fixed([0, 1, 2, 3, (100, 3), (7, 2), 5, (258, 1), (200, 257)], final=True)))
    # a constant image as one chain: literal 0, then distance 1 and length 258 over and over -- two bits a match, a distance code of one
    # code of one bit, 4064 matches in one window
    w, h = 1023, 1024
    d = Deflater().dynamic([0] + [(258, 1)] * 4064 + [0] * 63, {0: 2, 256: 2, 285: 1}, {0: 1}, final=True)
    assert len(d.raw) == h * (1 + w) and not any(d.raw)
    out.append(("distance_1_length_258_over_the_whole_image", w, h, d.stream()))
    out.append(row_case("single_distance_code_of_one_bit", Deflater().dynamic([0, 3, 3, (5, 1), 3, (3, 1)], {0: 2, 3: 2, 256: 2, 259: 3, 257: 3}, {0: 1}, final=True)))
    far = [0] + noise_literals(32767, 11, 256)
    out.append(row_case("distance_32768", Deflater().fixed(far + [(258, 32768), 1, (3, 32768), (10, 32767)], final=True)))
    # sources in the previous block, in the previous window (70 000 bits of literals are more than a window), in a stored block
    first = [0] + noise_literals(300, 12)
    d = Deflater().fixed(first).fixed([(50, 301), (20, 20), 7, (9, 350)]).stored(bytes(range(40))).fixed([(30, 40), (258, 400)])
    long_ = noise_literals(70000 // 8, 13)
    d.fixed(long_ + [(100, len(long_)), (40, 8000), (258, len(d.raw) + len(long_) + 140)], final=True)
    out.append(row_case("sources_in_earlier_blocks_and_windows", d))
    out.append(row_case("every_match_reads_the_one_before", Deflater().fixed([0, 1, 2, 3] + [(4, 4)] * 700 + [(5, 3)] * 300, final=True)))
    # codes of 1 .. 15 bits: two length symbols and two distance symbols with fifteen
    ll = {s: s + 1 for s in range(13)}
    ll.update({256: 14, 257: 15, 270: 15})
    dd = {s: s + 1 for s in range(14)}
    dd.update({14: 15, 15: 15})
    toks = [0] + noise_literals(260, 14, 13) + [(3, 130), (23, 200), (24, 255), (3, 1), 5, (26, 129)]
    out.append(row_case("fifteen_bit_length_and_distance_codes", Deflater().dynamic(toks, ll, dd, final=True)))
    # more stored blocks than the stored path's 64, mixed with Huffman blocks
    d = Deflater()
    for k in range(70):
        d.stored(bytes([0, k, k + 1, 255 - k])).fixed([k, (3, 4), (6, 2)], final=k == 69)
    out.append(row_case("seventy_stored_blocks_between_huffman_blocks", d))
    return out


# ------------------------------------------------------------------------------------------------ damaged streams


def _damaged_later():
    """(name, w, h, stream, reason): the faults a DEFLATE stream can have, in the second or a later block and inside a match"""
    tail = b"\x00\x00\x00\x00"
    lits = [0] + noise_literals(39, 21)  # the 40 x 1 image's 41 bytes would need one more: every case below fails before that matters
    out = []

    def add(name, d, reason, pad=4, keep=None):
        body = d.body() if keep is None else d.body()[:keep]
        out.append((name, b"\x78\x01" + body + bytes(pad) + tail, reason))

    add("distance_before_byte_0_in_block_2", Deflater().fixed(lits[:20]).fixed([1, 2, (5, 23)], final=True), R.DISTANCE)
    add("distance_before_byte_0_behind_a_stored_block", Deflater().fixed(lits[:10]).stored(b"\x01\x02").fixed([(3, 13)], final=True), R.DISTANCE)
    add("output_past_f_in_block_3", Deflater().fixed(lits[:20]).fixed(lits[20:40]).fixed([1, 2], final=True), R.OUTPUT_SIZE)
    add("match_past_f_in_block_2", Deflater().fixed(lits[:30]).fixed([(258, 7)], final=True), R.OUTPUT_SIZE)
    add("stored_past_f_in_block_2", Deflater().fixed(lits[:30]).stored(bytes(12), final=True), R.OUTPUT_SIZE)
    add("fewer_than_f_after_block_2", Deflater().fixed(lits[:30]).fixed([1, 2], final=True), R.OUTPUT_SIZE)
    add("block_type_3_as_block_2", Deflater().fixed(lits[:30]).tokens([("raw", 7, 3)], FIXED_LL, FIXED_D, end=False), R.BLOCK_TYPE)
    bad = Deflater().fixed(lits[:30]).stored(bytes(5))
    bad.bits[-5 * 8 - 16] ^= 1  # a bit of NLEN
    add("stored_len_mismatch_behind_a_huffman_block", bad, R.STORED_LEN)
    add("stored_block_cut_behind_a_huffman_block", Deflater().fixed(lits[:30]).stored(bytes(30)), R.TRUNCATED, pad=0, keep=40)
    over = Deflater().fixed(lits[:30])
    over.put(1, 1), over.put(2, 2), over.put(0, 5), over.put(0, 5), over.put(15, 4)
    for _ in range(19):
        over.put(1, 3)  # nineteen codes of one bit
    add("over_subscribed_code_in_block_2", over, R.BAD_CODE, pad=8)
    inc = Deflater().fixed(lits[:30])
    inc.put(1, 1), inc.put(2, 2), inc.put(0, 5), inc.put(0, 5), inc.put(0, 4)
    for v in (2, 2, 0, 0):
        inc.put(v, 3)  # two codes of two bits
    add("incomplete_code_in_block_2", inc, R.BAD_CODE, pad=8)
    # an incomplete literal/length code: {0: 1 bit, 256: 2 bits}, nothing for the pattern 11
    add("incomplete_literal_code_in_block_2", Deflater().fixed(lits[:30]).dynamic([0], {0: 1, 256: 2}, {0: 1}, final=True), R.BAD_CODE)
    add("length_symbol_286_in_block_2", Deflater().fixed(lits[:30]).fixed([1, ("code", FIXED_LL[286])], final=True), R.UNDEFINED_SYMBOL)
    add("distance_symbol_30_in_block_2", Deflater().fixed(lits[:30]).fixed([1, ("code", FIXED_LL[257]), ("code", FIXED_D[30])], final=True), R.UNDEFINED_SYMBOL)
    # a distance code of one code of one bit: the other bit is no code
    add("unused_bit_of_a_one_bit_distance_code", Deflater().fixed(lits[:30]).dynamic([3, ("code", (3, 2)), ("raw", 1, 1)], {3: 1, 257: 2, 256: 2}, {0: 1}, final=True),
        R.UNDEFINED_SYMBOL)
    # a dynamic block without a distance code, and a length symbol in it
    add("match_without_a_distance_code", Deflater().fixed(lits[:30]).dynamic([3, ("code", (3, 2)), ("raw", 0, 1)], {3: 1, 257: 2, 256: 2}, {0: 0}, final=True),
        R.UNDEFINED_SYMBOL)
    # the input ends inside a token: in the length's extra bits, in the distance code, in the distance's extra bits (no trailer either)
    for name, drop in (("length_extra_bits", 26), ("distance_code", 20), ("distance_extra_bits", 9)):
        d = Deflater().fixed(lits[:30]).fixed([1] * 5 + [(200, 33)], final=True, end=False)  # 8 + 5 length bits, 5 + 13 distance bits
        d.bits = d.bits[:-drop]
        d.bits = d.bits[:len(d.bits) // 8 * 8]
        out.append(("input_ends_in_the_%s" % name, b"\x78\x01" + d.body(), R.TRUNCATED))
    big = P.filtered(R.test_image(64, 64, 2), 8, P.ADAPTIVE).tobytes()  # dozens of blocks at memLevel 1
    s = R.zstream(big, deflated(big, mem=1))
    out.append(("cut_in_a_late_block", s[:len(s) * 3 // 4], R.TRUNCATED))
    out.append(("one_byte_more_after_dozens_of_blocks", R.zstream(big + b"\x00", deflated(big + b"\x00", mem=1)), R.OUTPUT_SIZE))
    flipped = bytearray(s)
    flipped[-2] ^= 4
    out.append(("trailer_flipped_after_dozens_of_blocks", bytes(flipped), R.ADLER))
    bad_type = bytearray(big)
    bad_type[65 * 40] = 7
    out.append(("filter_type_7_after_dozens_of_blocks", R.zstream(bytes(bad_type), deflated(bytes(bad_type), mem=1)), R.FILTER_TYPE))
    return [(n, 40, 1, s_, r) for n, s_, r in out[:-4]] + [(n, 64, 64, s_, r) for n, s_, r in out[-4:]]


@functools.lru_cache(maxsize=None)
def damaged_cases():
    """(name, w, h, stream, reason)"""
    return [tuple(c) for c in R.damaged_cases()] + [("later_" + n, w, h, s, r) for n, w, h, s, r in _damaged_later()]


# ------------------------------------------------------------------------------------------------ the groups


@functools.lru_cache(maxsize=None)
def small_valid_cases():
    """(name, w, h, stream): everything but the 640 x 480 group and R.all_valid_cases()"""
    out = []
    for w, h in SIZES:
        out += zlib_cases(w, h)
    return out + lz_cases() + hand_cases()


@functools.lru_cache(maxsize=None)
def large_valid_cases():
    return zlib_cases(640, 480, (("level1", dict(level=1)), ("level6", dict(level=6)), ("rle", dict(strategy=zlib.Z_RLE)), ("mem1", dict(level=6, mem=1))))


@functools.lru_cache(maxsize=None)
def restatement_valid_cases():
    return [tuple(c) for c in R.all_valid_cases()]


def all_valid_cases():
    return small_valid_cases() + large_valid_cases() + restatement_valid_cases()


def by_size(cases):
    """{(w, h): [case]}: a decoder has one size"""
    out = {}
    for c in cases:
        out.setdefault((c[1], c[2]), []).append(c)
    return out


def filtered_bytes(stream):
    return zlib.decompress(bytes(stream))


def pixels(w, h, stream):
    return R.unfilter(filtered_bytes(stream), w, h)

