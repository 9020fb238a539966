"""The device PNG decoder's rules (include/mdc_pngd.h), restated sequentially from RFC 1950, RFC 1951 and the PNG specification:
the chunk walk that yields a frame's zlib stream, inflate with the reason it gives for refusing a stream, the rule that says which
decode path a stream takes, the Adler-32 and filter-type checks in their order, and the unfilter.  Plus the inputs the tests share:
valid streams of every kind the decoder has a path for, and damaged ones for every reason code.  tests/test_pngd_cpu.py pins all of
it to zlib and PIL."""
import io
import struct
import zlib

import numpy as np

import pngw_restatement as P

OK, TRUNCATED, ZLIB_HEADER, BLOCK_TYPE, STORED_LEN, BAD_CODE, UNDEFINED_SYMBOL, DISTANCE, OUTPUT_SIZE, FILTER_TYPE, ADLER = range(11)
REASONS = ("ok", "truncated", "zlib_header", "block_type", "stored_len", "bad_code", "undefined_symbol", "distance", "output_size", "filter_type", "adler")
PARALLEL, STORED, GENERAL = 1, 2, 3
MAX_STORED_BLOCKS = 64
CL_ORDER = P.CL_ORDER


class Refused(Exception):
    def __init__(self, reason):
        Exception.__init__(self, REASONS[reason])
        self.reason = reason


# ------------------------------------------------------------------------------------------------ the chunk walk


def png_stream(data):
    """-> (w, h, the IDAT bodies concatenated) of an 8-bit grayscale non-interlaced file, None for any other file.  The walk ends at
    IEND, at the end of the file, or at a chunk that runs past it (then: None)."""
    data = bytes(data)
    if len(data) < 8 or data[:8] != P.SIGNATURE:
        return None
    at, ihdr, idat = 8, None, []
    while at + 12 <= len(data):
        (n,), tag = struct.unpack(">I", data[at:at + 4]), data[at + 4:at + 8]
        if at + 12 + n > len(data):
            return None
        body = data[at + 8:at + 8 + n]
        if tag == b"IHDR" and n >= 13:
            ihdr = struct.unpack(">IIBBBBB", body[:13])
        elif tag == b"IDAT":
            idat.append(body)
        elif tag == b"IEND":
            break
        at += 12 + n
    if ihdr is None:
        return None
    w, h, depth, ctype, _, _, interlace = ihdr
    if depth != 8 or ctype != 0 or interlace != 0 or not (1 <= w <= 65535 and 1 <= h <= 65535):
        return None
    return w, h, b"".join(idat)


def png_file(w, h, stream, split=None, extra=(), depth=8, ctype=0, interlace=0):
    """a PNG file around a zlib stream: IDAT chunks of `split` bytes (None: one), `extra` = (tag, body) chunks put between them"""
    out = [P.SIGNATURE, P.chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, interlace))]
    parts = [stream] if not split else [stream[i:i + split] for i in range(0, len(stream), split)]
    extra = list(extra)
    for k, part in enumerate(parts):
        out.append(P.chunk(b"IDAT", part))
        if extra and k < len(parts) - 1:
            out.append(P.chunk(*extra.pop(0)))
    for e in extra:
        out.append(P.chunk(*e))
    out.append(P.chunk(b"IEND", b""))
    return b"".join(out)


# ------------------------------------------------------------------------------------------------ inflate


class Reader:
    def __init__(self, data, bit):
        self.d, self.pos, self.end = data, bit, 8 * len(data)

    def left(self):
        return self.end - self.pos

    def bit(self):
        v = (self.d[self.pos >> 3] >> (self.pos & 7)) & 1
        self.pos += 1
        return v

    def take(self, k):
        if self.left() < k:
            raise Refused(TRUNCATED)
        v = 0
        for i in range(k):
            v |= self.bit() << i
        return v


def make_code(lengths, is_cl=False):
    """RFC 1951 3.2.2 -> {(length, code): symbol}; over-subscribed or incomplete sets refused by zlib's rule: an incomplete set passes
    only when it codes nothing at all, or (not the code-length code) its one code has one bit"""
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0] = 0
    left, maxl = 1, 0
    for l in range(1, 16):
        if count[l]:
            maxl = l
        left = 2 * left - count[l]
        if left < 0:
            raise Refused(BAD_CODE)
    if left > 0 and maxl != 0 and (is_cl or maxl != 1):
        raise Refused(BAD_CODE)
    code, nxt = 0, [0] * 16
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    table = {}
    for s, l in enumerate(lengths):
        if l:
            table[(l, nxt[l])] = s
            nxt[l] += 1
    return table


def symbol(table, r):
    code = 0
    for l in range(1, 16):
        if r.left() < 1:
            raise Refused(TRUNCATED)
        code = (code << 1) | r.bit()
        s = table.get((l, code))
        if s is not None:
            return s
    raise Refused(UNDEFINED_SYMBOL)


def dynamic_header(r):
    """-> (literal/length table, distance table, the number of distance symbols that have a code)"""
    v = r.take(14)
    hlit, hdist, hclen = 257 + (v & 31), 1 + ((v >> 5) & 31), 4 + (v >> 10)
    if hlit > 286 or hdist > 30:
        raise Refused(BAD_CODE)
    cl = [0] * 19
    for i in range(hclen):
        cl[CL_ORDER[i]] = r.take(3)
    cltab = make_code(cl, True)
    lens = []
    while len(lens) < hlit + hdist:
        s = symbol(cltab, r)
        if s < 16:
            lens.append(s)
            continue
        if s == 16:
            if not lens:
                raise Refused(BAD_CODE)
            val, rep = lens[-1], 3 + r.take(2)
        elif s == 17:
            val, rep = 0, 3 + r.take(3)
        else:
            val, rep = 0, 11 + r.take(7)
        if len(lens) + rep > hlit + hdist:
            raise Refused(BAD_CODE)
        lens += [val] * rep
    if lens[256] == 0:
        raise Refused(BAD_CODE)
    return make_code(lens[:hlit]), make_code(lens[hlit:]), sum(1 for l in lens[hlit:] if l)


FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LENGTH_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]


def zlib_header(data):
    if len(data) < 2:
        raise Refused(TRUNCATED)
    cmf, flg = data[0], data[1]
    if (cmf & 15) != 8 or (cmf >> 4) > 7 or ((cmf << 8) | flg) % 31 or (flg & 32):
        raise Refused(ZLIB_HEADER)


def inflate(data, F):
    """-> (the F bytes, the byte offset of the trailer, the block types met); Refused(reason) at the first thing wrong"""
    zlib_header(data)
    r = Reader(data, 16)
    out = bytearray()
    while True:
        hdr = r.take(3)
        btype = hdr >> 1
        if btype == 3:
            raise Refused(BLOCK_TYPE)
        if btype == 0:
            r.pos = (r.pos + 7) & ~7
            v = r.take(32)
            n = v & 0xffff
            if n != (~(v >> 16) & 0xffff):
                raise Refused(STORED_LEN)
            at = r.pos >> 3
            if n > len(data) - at:
                raise Refused(TRUNCATED)
            if n > F - len(out):
                raise Refused(OUTPUT_SIZE)
            out += data[at:at + n]
            r.pos = 8 * (at + n)
        else:
            if btype == 1:
                lit, dist = make_code(FIXED_LIT), make_code([5] * 32)
            else:
                lit, dist, _ = dynamic_header(r)
            while True:
                s = symbol(lit, r)
                if s < 256:
                    if len(out) >= F:
                        raise Refused(OUTPUT_SIZE)
                    out.append(s)
                    continue
                if s == 256:
                    break
                if s > 285:
                    raise Refused(UNDEFINED_SYMBOL)
                n = LENGTH_BASE[s - 257] + (r.take(LENGTH_EXTRA[s - 257]) if LENGTH_EXTRA[s - 257] else 0)
                d = symbol(dist, r)
                if d > 29:
                    raise Refused(UNDEFINED_SYMBOL)
                back = DIST_BASE[d] + (r.take(DIST_EXTRA[d]) if DIST_EXTRA[d] else 0)
                if back > len(out):
                    raise Refused(DISTANCE)
                if n > F - len(out):
                    raise Refused(OUTPUT_SIZE)
                for _ in range(n):
                    out.append(out[-back])
        if hdr & 1:
            break
    if len(out) != F:
        raise Refused(OUTPUT_SIZE)
    return bytes(out), (r.pos + 7) >> 3


def first_path(data, F):
    """the path that tries the stream first: PARALLEL for a single final dynamic block without a distance code, STORED for a chain of at
    most MAX_STORED_BLOCKS stored blocks that is right in every respect, else GENERAL"""
    try:
        zlib_header(data)
        r = Reader(data, 16)
        hdr = r.take(3)
        if hdr >> 1 == 0:
            at, total = 2, 0
            for _ in range(MAX_STORED_BLOCKS):
                if at + 5 > len(data):
                    return GENERAL
                h, n, nn = data[at], data[at + 1] | data[at + 2] << 8, data[at + 3] | data[at + 4] << 8
                if (h >> 1) & 3 or n != (~nn & 0xffff) or n > len(data) - (at + 5) or n > F - total:
                    return GENERAL
                total += n
                at += 5 + n
                if h & 1:
                    return STORED if total == F else GENERAL
            return GENERAL
        if hdr != 5:
            return GENERAL
        _, _, ndist = dynamic_header(r)
        return GENERAL if ndist else PARALLEL
    except Refused:
        return GENERAL


def unfilter(data, w, h):
    rows = np.frombuffer(data, np.uint8).reshape(h, 1 + w)
    out = np.zeros((h, w), np.uint8)
    zero = np.zeros(w, np.int64)
    for y in range(h):
        t, x = int(rows[y, 0]), rows[y, 1:].astype(np.int64)
        up = out[y - 1].astype(np.int64) if y else zero
        if t == 0:
            out[y] = x
        elif t == 1:
            out[y] = np.cumsum(x) & 255
        elif t == 2:
            out[y] = (x + up) & 255
        else:
            a = c = 0
            line = [0] * w
            for i in range(w):
                b = int(up[i])
                if t == 3:
                    pred = (a + b) >> 1
                else:
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
                a, c = (int(x[i]) + pred) & 255, b
                line[i] = a
            out[y] = line
    return out


def decode(data, w, h, pixels=True):
    """-> (reason, path, the image or None), in the order of include/mdc_pngd.h"""
    data = bytes(data)
    F = h * (1 + w)
    path = first_path(data, F)
    try:
        raw, end = inflate(data, F)
    except Refused as e:
        return e.reason, GENERAL, None  # whatever another path gives up on, the sequential decoder decides
    if len(data) - end < 4:
        return TRUNCATED, path, None
    if struct.unpack(">I", data[end:end + 4])[0] != P.adler32(raw):
        return ADLER, path, None
    if any(raw[y * (1 + w)] > 4 for y in range(h)):
        return FILTER_TYPE, path, None
    return OK, path, unfilter(raw, w, h) if pixels else None


def host_accepts(data, w, h):
    """what the host decoder (png_gray8) makes of the stream: zlib's uncompress into F bytes gives Z_OK and exactly F, and every row's
    filter type is one of the five"""
    try:
        raw = zlib.decompress(bytes(data))
    except zlib.error:
        return False
    return len(raw) == h * (1 + w) and all(raw[y * (1 + w)] <= 4 for y in range(h))


# ------------------------------------------------------------------------------------------------ making streams


def filter_rows(img, types):
    """the filtered bytes of `img` with row y filtered by types[y]"""
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    x = img.astype(np.int32)
    a = np.concatenate([np.zeros((h, 1), np.int32), x[:, :-1]], 1)
    b = np.concatenate([np.zeros((1, w), np.int32), x[:-1]], 0)
    c = np.concatenate([np.zeros((h, 1), np.int32), b[:, :-1]], 1)
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    cand = [np.zeros_like(x), a, b, (a + b) >> 1, paeth]
    out = np.zeros((h, 1 + w), np.uint8)
    for y in range(h):
        out[y, 0] = types[y]
        out[y, 1:] = (x[y] - cand[types[y]][y]) & 255
    return out.tobytes()


def zstream(raw, body=None, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, header=b"\x78\x01"):
    """a zlib stream of the filtered bytes `raw`: `body` = a DEFLATE stream made elsewhere, else zlib's at level / strategy"""
    if body is None:
        co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
        body = co.compress(raw) + co.flush()
    return header + body + struct.pack(">I", zlib.adler32(raw))


def literal_stream(raw):
    """the parallel path's form: one final dynamic block of literals, as libmdc_pngw writes it"""
    return zstream(raw, P.dynamic_block(raw)[0])


def stored_stream(raw):
    return zstream(raw, P.stored_blocks(raw))


class BitWriter:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, v, n):  # least significant bit first
        self.v |= v << self.n
        self.n += n
        return self

    def code(self, c, n):  # a Huffman code: most significant bit first
        for i in range(n - 1, -1, -1):
            self.put((c >> i) & 1, 1)
        return self

    def fixed_literal(self, s):
        return self.code(0x30 + s, 8) if s < 144 else self.code(0x190 + s - 144, 9) if s < 256 else self.code(s - 256, 7) if s < 280 else self.code(0xc0 + s - 280, 8)

    def bytes(self, pad=0):
        return self.v.to_bytes((self.n + 7) // 8 + pad, "little")


def test_image(w, h, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    return ((xx * 5 + yy * 3 + rng.integers(0, 9, (h, w))) & 255).astype(np.uint8)


def unfilter_cases(w, h):
    """(name, stream) for one size: every type forced, mixed per row, Paeth ties and Average with carries"""
    img = test_image(w, h, 100 * w + h)
    out = [("type%d" % t, zstream(filter_rows(img, [t] * h))) for t in range(5)]
    mixed = [(y * 7 + y // 3) % 5 for y in range(h)]
    out.append(("mixed", literal_stream(filter_rows(img, mixed))))
    out.append(("mixed_reversed", zstream(filter_rows(img, mixed[::-1]), level=1)))
    ties = np.full((h, w), 200, np.uint8)  # a == b == c: every Paeth distance ties
    ties[::2, ::3] = 100
    out.append(("paeth_ties", zstream(filter_rows(ties, [4] * h))))
    carry = np.full((h, w), 255, np.uint8)  # a + b = 510: the average needs nine bits
    carry[1::2, 1::2] = 254
    out.append(("average_carries", zstream(filter_rows(carry, [3] * h))))
    rng = np.random.default_rng(w + 1000 * h)  # filtered bytes that are noise: every type on arbitrary input, wrapping sums
    noise = rng.integers(0, 256, (h, 1 + w), dtype=np.uint8)
    noise[:, 0] = rng.integers(0, 5, h)
    out.append(("noise_rows", stored_stream(noise.tobytes())))
    return out


UNFILTER_SIZES = [(w, h) for w in (1, 2, 3, 63, 64, 65, 130) for h in (1, 2, 63, 64, 65, 129)]


def noise_row(nbytes, seed, top=256):
    v = np.random.default_rng(seed).integers(0, top, nbytes, dtype=np.uint8)
    v[0] = 0
    return v.tobytes()


def parallel_cases():
    """(name, w, h, stream): literal-only streams at the parallel path's edges.  Subsequences are max(64, ceil(bits / 1024)) bits long:
    fewer subsequences than threads below 65536 bits of symbols, one per thread from there on, longer ones past it"""
    out = []
    for filt in (0, 1, 2, 3, 4, P.ADAPTIVE):
        img = test_image(70, 33, 40 + filt)
        out.append(("image_filter%d" % filt, 70, 33, literal_stream(P.filtered(img, 8, filt).tobytes())))
    out.append(("constant", 50, 20, literal_stream(P.filtered(np.full((20, 50), 77, np.uint8), 8, 0).tobytes())))  # two symbols and end-of-block
    out.append(("one_pixel", 1, 1, literal_stream(b"\x00\x09")))
    # 17 values that occur 2, 3, 5, ... 4181 times: with the type byte and the end-of-block the counts are the first 19 Fibonacci
    # numbers, Huffman's own tree is 18 deep and the code is cut to 15 bits
    vals = np.repeat(np.arange(10, 27, dtype=np.uint8), P.fibonacci(19)[2:])
    raw = b"\x00" + np.random.default_rng(8).permutation(vals).tobytes()
    assert max(P.dynamic_block(raw)[1]) == 15
    out.append(("length_15", len(raw) - 1, 1, literal_stream(raw)))
    for name, nbytes in (("few_bits", 6), ("below_thread_count", 700), ("one_per_thread_minus", 8150), ("one_per_thread_plus", 8260),
                         ("two_per_thread_minus", 16350), ("two_per_thread_plus", 16450)):
        raw = noise_row(nbytes, nbytes)  # ~8 bits a symbol: 8192 bytes are 65536 bits
        out.append((name, nbytes - 1, 1, literal_stream(raw)))
    skew = noise_row(9000, 5, top=3)  # short codes: many symbols per subsequence
    out.append(("short_codes", 8999, 1, literal_stream(skew)))
    return out


def stored_cases():
    out = []
    for name, w, h in (("small", 9, 5), ("below_65535", 254, 257), ("exactly_65535", 4368, 15), ("300x300", 300, 300), ("exactly_2x65535", 4368, 30)):
        F = h * (1 + w)
        raw = np.random.default_rng(F).integers(0, 256, (h, 1 + w), dtype=np.uint8)
        raw[:, 0] = np.arange(h) % 5
        out.append((name, w, h, stored_stream(raw.tobytes())))
    assert 15 * 4369 == 65535
    return out


def general_cases():
    out = []
    img = test_image(96, 40, 7)
    raw = P.filtered(img, 8, P.ADAPTIVE).tobytes()
    for level in (1, 6, 9):
        out.append(("level%d" % level, 96, 40, zstream(raw, level=level)))
    for name, st in (("rle", zlib.Z_RLE), ("fixed", zlib.Z_FIXED)):
        out.append((name, 96, 40, zstream(raw, strategy=st)))
    # Z_HUFFMAN_ONLY: no matches, but more than one block -- not the parallel path's form
    big = test_image(200, 180, 8)
    co = zlib.compressobj(6, zlib.DEFLATED, -15, 1, zlib.Z_HUFFMAN_ONLY)  # memLevel 1: a block every 127 symbols or so
    rawb = P.filtered(big, 8, 1).tobytes()
    out.append(("huffman_only", 200, 180, zstream(rawb, co.compress(rawb) + co.flush())))
    # level 0 mixed with compressed blocks
    parts = []
    c0 = zlib.compressobj(0, zlib.DEFLATED, -15)
    third = len(raw) // 3
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    parts.append(co.compress(raw[:third]) + co.flush(zlib.Z_FULL_FLUSH))  # (a full flush ends with an empty stored block)
    parts.append(c0.compress(raw[third:2 * third]) + c0.flush(zlib.Z_FULL_FLUSH))
    co = zlib.compressobj(9, zlib.DEFLATED, -15)
    parts.append(co.compress(raw[2 * third:]) + co.flush())
    out.append(("stored_and_compressed", 96, 40, zstream(raw, b"".join(parts))))
    # an empty stored block in the middle of stored blocks: not a plain chain for zlib, a chain for us
    half = len(raw) // 2
    body = struct.pack("<BHH", 0, half, half ^ 0xffff) + raw[:half] + struct.pack("<BHH", 0, 0, 0xffff) + struct.pack("<BHH", 1, len(raw) - half, (len(raw) - half) ^ 0xffff) + raw[half:]
    out.append(("empty_stored_in_the_middle", 96, 40, zstream(raw, body)))
    # an empty stored block between two compressed blocks
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    body = co.compress(raw[:half]) + co.flush(zlib.Z_SYNC_FLUSH) + co.compress(raw[half:]) + co.flush()
    out.append(("sync_flush_in_the_middle", 96, 40, zstream(raw, body)))
    const = P.filtered(np.full((60, 300), 9, np.uint8), 8, 0).tobytes()  # distance 1, length 258 chains
    out.append(("constant", 300, 60, zstream(const, level=9)))
    # 256 x 200 whose second half repeats the first: matches at distance 100 * 257 = 25700 ... and, with a 32 KiB window, up to it
    top = np.random.default_rng(9).integers(0, 256, (125, 256), dtype=np.uint8)
    far = np.concatenate([top, top[:75]])  # rows 125..199 repeat rows 0..74 at distance 125 * 257 = 32125
    rawf = filter_rows(far, [0] * 200)
    s = zstream(rawf, level=9)
    out.append(("distance_32125", 256, 200, s))
    # more than MAX_STORED_BLOCKS stored blocks
    rows = np.random.default_rng(10).integers(0, 5, (70, 4), dtype=np.uint8)
    body = b"".join(struct.pack("<BHH", int(y == 69), 4, 4 ^ 0xffff) + rows[y].tobytes() for y in range(70))
    out.append(("seventy_stored_blocks", 3, 70, zstream(rows.tobytes(), body)))
    return out


def damaged_cases():
    """(name, w, h, stream, the reason): what the restatement and zlib both refuse, every reason at least once"""
    img = test_image(40, 12, 3)
    raw = P.filtered(img, 8, P.ADAPTIVE).tobytes()
    F = len(raw)
    good, lit, sto = zstream(raw), literal_stream(raw), stored_stream(raw)
    out = [("cut_in_the_symbols", good[:len(good) // 2], TRUNCATED), ("cut_in_the_trailer", good[:-2], TRUNCATED), ("no_bytes", b"", TRUNCATED),
           ("one_byte", b"\x78", TRUNCATED), ("header_only", b"\x78\x01", TRUNCATED), ("literal_cut", lit[:len(lit) // 2], TRUNCATED),
           ("literal_cut_in_the_header", lit[:9], TRUNCATED), ("stored_cut", sto[:len(sto) // 2], TRUNCATED), ("stored_cut_in_the_header", sto[:5], TRUNCATED),
           ("method_9", b"\x79\x01" + good[2:], ZLIB_HEADER), ("bad_check_bits", b"\x78\x02" + good[2:], ZLIB_HEADER),
           ("preset_dictionary", b"\x78\x20" + good[2:], ZLIB_HEADER), ("window_too_large", b"\x88\x1c" + good[2:], ZLIB_HEADER),
           ("block_type_3", b"\x78\x01" + bytes([7]) + good[3:], BLOCK_TYPE),
           ("stored_len_mismatch", sto[:5] + bytes([sto[5] ^ 1]) + sto[6:], STORED_LEN),
           ("trailer_flipped", good[:-1] + bytes([good[-1] ^ 1]), ADLER), ("literal_trailer_flipped", lit[:-3] + bytes([lit[-3] ^ 0x40]) + lit[-2:], ADLER),
           ("stored_byte_flipped", sto[:40] + bytes([sto[40] ^ 0x10]) + sto[41:], ADLER)]
    bad = bytearray(raw)
    bad[41 * 3] = 5
    out.append(("filter_type_5", zstream(bytes(bad)), FILTER_TYPE))
    bad[41 * 3] = 255
    out.append(("filter_type_255_stored", stored_stream(bytes(bad)), FILTER_TYPE))
    out.append(("one_byte_more", zstream(raw + b"\x00"), OUTPUT_SIZE))
    out.append(("one_byte_more_literal", literal_stream(raw + b"\x00"), OUTPUT_SIZE))
    out.append(("one_byte_more_stored", stored_stream(raw + b"\x00"), OUTPUT_SIZE))
    out.append(("one_byte_less", zstream(raw[:-1]), OUTPUT_SIZE))
    out.append(("one_byte_less_literal", literal_stream(raw[:-1]), OUTPUT_SIZE))
    out.append(("match_past_the_end", zstream(bytes(F + 200), level=9), OUTPUT_SIZE))
    tail = b"\x00\x00\x00\x00"
    w19 = BitWriter().put(1, 1).put(2, 2).put(0, 5).put(0, 5).put(15, 4)
    for _ in range(19):
        w19.put(1, 3)  # nineteen codes of one bit
    out.append(("code_length_code_over_subscribed", b"\x78\x01" + w19.bytes(8) + tail, BAD_CODE))
    inc = BitWriter().put(1, 1).put(2, 2).put(0, 5).put(0, 5).put(0, 4).put(2, 3).put(2, 3).put(0, 3).put(0, 3)  # two codes of two bits
    out.append(("code_length_code_incomplete", b"\x78\x01" + inc.bytes(8) + tail, BAD_CODE))
    # the code-length code {0: 1 bit, 16: 1 bit}: a repeat with nothing before it
    rep = BitWriter().put(1, 1).put(2, 2).put(0, 5).put(0, 5).put(0, 4).put(1, 3).put(0, 3).put(0, 3).put(1, 3).code(1, 1).put(0, 2)
    out.append(("repeat_without_a_length", b"\x78\x01" + rep.bytes(8) + tail, BAD_CODE))
    # {0: 1 bit, 18: 1 bit}: 138 zeros three times pass 258 lengths
    far = BitWriter().put(1, 1).put(2, 2).put(0, 5).put(0, 5).put(0, 4).put(0, 3).put(0, 3).put(1, 3).put(1, 3)
    for _ in range(3):
        far.code(1, 1).put(127, 7)
    out.append(("repeat_past_the_last_length", b"\x78\x01" + far.bytes(8) + tail, BAD_CODE))
    # ... and twice 129 zeros: 258 lengths, all zero, no end-of-block code
    none = BitWriter().put(1, 1).put(2, 2).put(0, 5).put(0, 5).put(0, 4).put(0, 3).put(0, 3).put(1, 3).put(1, 3)
    for _ in range(2):
        none.code(1, 1).put(118, 7)
    out.append(("no_end_of_block_code", b"\x78\x01" + none.bytes(8) + tail, BAD_CODE))
    fx = BitWriter().put(1, 1).put(1, 2).fixed_literal(0).fixed_literal(286)
    out.append(("fixed_length_symbol_286", b"\x78\x01" + fx.bytes(4) + tail, UNDEFINED_SYMBOL))
    fx = BitWriter().put(1, 1).put(1, 2).fixed_literal(0).fixed_literal(257).code(30, 5)
    out.append(("fixed_distance_symbol_30", b"\x78\x01" + fx.bytes(4) + tail, UNDEFINED_SYMBOL))
    fx = BitWriter().put(1, 1).put(1, 2).fixed_literal(0).fixed_literal(257).code(1, 5)  # one byte written, distance 2
    out.append(("distance_before_byte_0", b"\x78\x01" + fx.bytes(4) + tail, DISTANCE))
    fx = BitWriter().put(1, 1).put(1, 2).fixed_literal(257).code(0, 5)  # nothing written, distance 1
    out.append(("match_as_the_first_symbol", b"\x78\x01" + fx.bytes(4) + tail, DISTANCE))
    # the literal-only stream with a bit of its symbols flipped: whatever it decodes to, its sum or its size is wrong
    flipped = bytearray(lit)
    flipped[len(lit) // 2] ^= 0x08
    r = decode(bytes(flipped), 40, 12, pixels=False)[0]
    out.append(("literal_bit_flipped", bytes(flipped), r))
    return [(n, 40, 12, s, r) for n, s, r in out]


def all_valid_cases():
    out = [("unfilter_%dx%d_%s" % (w, h, n), w, h, s) for w, h in UNFILTER_SIZES for n, s in unfilter_cases(w, h)]
    out += [("parallel_" + n, w, h, s) for n, w, h, s in parallel_cases()]
    out += [("stored_" + n, w, h, s) for n, w, h, s in stored_cases()]
    out += [("general_" + n, w, h, s) for n, w, h, s in general_cases()]
    return out


def pil_pixels(w, h, stream):
    from PIL import Image

    return np.array(Image.open(io.BytesIO(png_file(w, h, stream))))
