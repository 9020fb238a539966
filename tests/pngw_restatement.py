"""include/mdc_pngw.h restated with NumPy and struct: the five filters and the adaptive choice, the histogram, the code lengths (the
two-queue Huffman construction and the two repair loops), canonical codes, the run-length coded block header, the LSB-first bit
stream, the stored fallback, Adler-32 and the chunk CRCs -- the whole file from an array.  The byte-for-byte oracle of
tests/test_pngw.py; itself pinned by zlib and PIL in tests/test_pngw_cpu.py."""
import struct
import zlib  # encode() uses its adler32 and crc32 for speed; both are restated below and compared with it in tests/test_pngw_cpu.py

import numpy as np

ADAPTIVE = 5
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
SIGNATURE = b"\x89PNG\r\n\x1a\n"


def crc32(data):
    table = getattr(crc32, "table", None)
    if table is None:
        table = []
        for n in range(256):
            c = n
            for _ in range(8):
                c = (c >> 1) ^ (0xEDB88320 if c & 1 else 0)
            table.append(c)
        crc32.table = table
    c = 0xFFFFFFFF
    for b in bytes(data):
        c = table[(c ^ b) & 255] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


def adler32(data):
    """s1 = 1 + sum d, s2 = n + sum (n - i) d, both mod 65521 (the sums the device keeps)"""
    d = np.frombuffer(bytes(data), np.uint8).astype(object)
    n = len(d)
    s1 = (1 + int(d.sum())) % 65521 if n else 1
    s2 = (n + sum(int(v) * (n - i) for i, v in enumerate(d) if v)) % 65521
    return (s2 << 16) | s1


def f32_to_u8(a):
    """cv::Mat::convertTo(CV_8U): rint (ties to even), clamped to 0..255, NaN -> 0"""
    a = np.asarray(a, np.float32)
    with np.errstate(invalid="ignore"):
        r = np.clip(np.rint(a), 0, 255)
    return np.where(np.isnan(a), 0, r).astype(np.uint8)


def raw_bytes(img, depth):
    img = np.asarray(img)
    assert img.ndim == 2 and depth in (8, 16)
    if depth == 8:
        return np.ascontiguousarray(img, np.uint8)
    return np.ascontiguousarray(img.astype(">u2")).view(np.uint8).reshape(img.shape[0], img.shape[1] * 2)


def paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filtered(img, depth, filt):
    """the filtered image as (h, 1 + w * bpp) bytes: the type, then the row filtered from the raw neighbours"""
    raw = raw_bytes(img, depth).astype(np.int32)
    h, rb = raw.shape
    bpp = depth // 8
    a = np.zeros_like(raw)
    a[:, bpp:] = raw[:, :-bpp]
    b = np.zeros_like(raw)
    b[1:] = raw[:-1]
    c = np.zeros_like(raw)
    c[1:, bpp:] = raw[:-1, :-bpp]
    cand = np.stack([raw, raw - a, raw - b, raw - ((a + b) >> 1), raw - paeth(a, b, c)]) & 255  # (5, h, rb)
    if filt == ADAPTIVE:
        cost = np.where(cand < 128, cand, 256 - cand).sum(axis=2)  # (5, h)
        types = np.argmin(cost, axis=0)  # the first minimum: ties go to the lowest type
    else:
        assert 0 <= filt <= 4
        types = np.full(h, filt)
    out = np.empty((h, 1 + rb), np.uint8)
    out[:, 0] = types
    out[:, 1:] = cand[types, np.arange(h)]
    return out


def huffman_lengths(hist, limit):
    """include/mdc_pngw.h, "Code lengths\""""
    hist = [int(v) for v in hist]
    lengths = [0] * len(hist)
    order = sorted((s for s in range(len(hist)) if hist[s] > 0), key=lambda s: (hist[s], s))
    n = len(order)
    if n == 0:
        return lengths
    if n == 1:
        lengths[order[0]] = 1
        return lengths
    assert n <= 1 << limit
    wt = [hist[s] for s in order] + [0] * (n - 1)
    parent = [0] * (2 * n - 1)
    leaf, inner, nxt = 0, n, n
    while nxt < 2 * n - 1:
        total = 0
        for _ in range(2):
            if leaf < n and (inner >= nxt or wt[leaf] <= wt[inner]):
                node, leaf = leaf, leaf + 1
            else:
                node, inner = inner, inner + 1
            total += wt[node]
            parent[node] = nxt
        wt[nxt] = total
        nxt += 1
    depth = [0] * (2 * n - 1)
    for node in range(2 * n - 3, -1, -1):
        depth[node] = depth[parent[node]] + 1
    full = 1 << limit
    for i, s in enumerate(order):
        lengths[s] = min(depth[i], limit)
    kraft = sum(1 << (limit - lengths[s]) for s in order)
    while kraft > full:
        for s in order:  # the rarest first
            if kraft <= full:
                break
            if lengths[s] < limit:
                lengths[s] += 1
                kraft -= 1 << (limit - lengths[s])
    while kraft < full:
        room = full - kraft
        s = next(s for s in reversed(order) if lengths[s] > 1 and (1 << (limit - lengths[s])) <= room)  # the most frequent first
        kraft += 1 << (limit - lengths[s])
        lengths[s] -= 1
    return lengths


def canonical_codes(lengths):
    """RFC 1951 3.2.2 -> code per symbol (most significant bit first)"""
    top = max(lengths) if lengths else 0
    count = [0] * (top + 2)
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * (top + 2), 0
    for b in range(1, top + 1):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    codes = []
    for l in lengths:
        codes.append(nxt[l] if l else 0)
        if l:
            nxt[l] += 1
    return codes


def reverse_bits(v, n):
    r = 0
    for _ in range(n):
        r, v = (r << 1) | (v & 1), v >> 1
    return r


def run_length_code(seq):
    """the 258 code lengths as (symbol, extra value) pairs, greedily from the left"""
    out, i = [], 0
    while i < len(seq):
        v, run = seq[i], 1
        while i + run < len(seq) and seq[i + run] == v:
            run += 1
        i += run
        if v == 0:
            while run >= 11:
                n = min(run, 138)
                out.append((18, n - 11))
                run -= n
            if run >= 3:
                out.append((17, run - 3))
                run = 0
        else:
            out.append((v, 0))
            run -= 1
            while run >= 3:
                n = min(run, 6)
                out.append((16, n - 3))
                run -= n
        out.extend([(v, 0)] * run)
    return out


class Bits:
    """LSB-first"""

    def __init__(self):
        self.value, self.n = 0, 0

    def put(self, v, n):
        assert 0 <= v < (1 << n) or n == 0
        self.value |= v << self.n
        self.n += n

    def put_code(self, code, length):
        self.put(reverse_bits(code, length), length)


def dynamic_block(data):
    """one dynamic block, BFINAL 1, Huffman only -> (bytes, the literal/length code lengths)"""
    d = np.frombuffer(bytes(data), np.uint8)
    hist = np.bincount(d, minlength=257).tolist()
    hist[256] = 1
    lengths = huffman_lengths(hist, 15)
    codes = canonical_codes(lengths)
    pairs = run_length_code(lengths + [0])  # + the one distance code, of length 0
    clhist = [0] * 19
    for s, _ in pairs:
        clhist[s] += 1
    cllen = huffman_lengths(clhist, 7)
    clcodes = canonical_codes(cllen)
    hclen = max([4] + [i + 1 for i in range(19) if cllen[CL_ORDER[i]]])
    bits = Bits()
    bits.put(1, 1)
    bits.put(2, 2)
    bits.put(0, 5)
    bits.put(0, 5)
    bits.put(hclen - 4, 4)
    for i in range(hclen):
        bits.put(cllen[CL_ORDER[i]], 3)
    for s, extra in pairs:
        bits.put_code(clcodes[s], cllen[s])
        if s >= 16:
            bits.put(extra, {16: 2, 17: 3, 18: 7}[s])
    # the data: every byte's reversed code at the running sum of the lengths before it
    lens = np.asarray(lengths[:256], np.int64)
    rev = np.asarray([reverse_bits(codes[s], lengths[s]) for s in range(256)], np.int64)
    ls, rs = lens[d], rev[d]
    at = bits.n + np.concatenate(([0], np.cumsum(ls)[:-1])) if len(d) else np.zeros(0, np.int64)
    end = bits.n + int(ls.sum())
    total = end + lengths[256]
    stream = np.zeros((total + 7) // 8 * 8, np.uint8)
    head = np.frombuffer(bits.value.to_bytes((bits.n + 7) // 8, "little"), np.uint8)
    stream[:bits.n] = np.unpackbits(head, bitorder="little")[:bits.n]
    for k in range(15):
        m = ls > k
        stream[at[m] + k] = (rs[m] >> k) & 1
    eob = reverse_bits(codes[256], lengths[256])
    for k in range(lengths[256]):
        stream[end + k] = (eob >> k) & 1
    return np.packbits(stream, bitorder="little").tobytes(), lengths


def stored_blocks(data):
    data = bytes(data)
    out = []
    nblocks = (len(data) + 65534) // 65535
    for b in range(nblocks):
        part = data[b * 65535:(b + 1) * 65535]
        out.append(struct.pack("<BHH", int(b == nblocks - 1), len(part), len(part) ^ 0xFFFF) + part)
    return b"".join(out)


def stored_size(nbytes):
    return nbytes + 5 * ((nbytes + 65534) // 65535)


def deflate(data):
    """-> (the DEFLATE stream, True if stored): dynamic only when strictly shorter"""
    dyn, _ = dynamic_block(data)
    if len(dyn) < stored_size(len(data)):
        return dyn, False
    return stored_blocks(data), True


def chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", crc32(tag + data))


def encode(img, depth, filt):
    """-> (the file, True if its image is stored)"""
    img = np.asarray(img)
    h, w = img.shape
    data = filtered(img, depth, filt).tobytes()
    stream, stored = deflate(data)
    idat = b"\x78\x01" + stream + struct.pack(">I", zlib.adler32(data))
    crc = zlib.crc32(b"IDAT" + idat)
    ihdr = struct.pack(">IIBBBBB", w, h, depth, 0, 0, 0, 0)
    out = SIGNATURE + chunk(b"IHDR", ihdr) + struct.pack(">I", len(idat)) + b"IDAT" + idat + struct.pack(">I", crc) + chunk(b"IEND", b"")
    return out, stored


def png_bound(w, h, depth):
    return 57 + 6 + stored_size(h * (1 + w * depth // 8))


def idat_of(png):
    """the single IDAT's data, after checking the chunk sequence IHDR IDAT IEND and every CRC with the restated crc32"""
    assert png[:8] == SIGNATURE
    at, tags, idat = 8, [], None
    while at < len(png):
        (n,), tag = struct.unpack(">I", png[at:at + 4]), png[at + 4:at + 8]
        body = png[at + 8:at + 8 + n]
        assert struct.unpack(">I", png[at + 8 + n:at + 12 + n])[0] == crc32(tag + body), tag
        tags.append(tag)
        if tag == b"IDAT":
            idat = body
        at += 12 + n
    assert tags == [b"IHDR", b"IDAT", b"IEND"] and at == len(png), tags
    return idat


def unfilter(data, w, h, depth):
    """the decoder's side, byte by byte as the PNG specification has it -> the image"""
    bpp = depth // 8
    rb = w * bpp
    rows = np.frombuffer(bytes(data), np.uint8).reshape(h, 1 + rb)
    out = np.zeros((h, rb), np.int32)
    for y in range(h):
        t = int(rows[y, 0])
        for x in range(rb):
            a = out[y, x - bpp] if x >= bpp else 0
            b = out[y - 1, x] if y else 0
            c = out[y - 1, x - bpp] if (y and x >= bpp) else 0
            pred = (0, a, b, (a + b) >> 1, int(paeth(np.int32(a), np.int32(b), np.int32(c))))[t]
            out[y, x] = (int(rows[y, x + 1]) + pred) & 255
    raw = out.astype(np.uint8)
    return raw if depth == 8 else raw.view(">u2").astype(np.uint16).reshape(h, w)


# ------------------------------------------------------------------------------------------------ shared test inputs


def fibonacci(n):
    a = [1, 1]
    while len(a) < n:
        a.append(a[-1] + a[-2])
    return a[:n]


def directed_histograms():
    """(name, counts, limit) for the code builder: Fibonacci counts (Huffman's own tree is deeper than the limit: 39 levels for 40
    symbols, 18 for the 19 of the code-length alphabet), one used symbol, two, all 286 equal, nothing but end-of-block, and more"""
    eob_only = [0] * 256 + [1]
    one = [0] * 286
    one[65] = 9
    two = [0] * 286
    two[0], two[256] = 1000, 1
    return [("fibonacci_40", fibonacci(40), 15), ("fibonacci_19", fibonacci(19), 7), ("one_symbol", one, 15), ("two_symbols", two, 15),
            ("all_286_equal", [5] * 286, 15), ("end_of_block_only", eob_only, 15),
            ("fibonacci_40_shuffled", [int(v) for v in np.random.default_rng(6).permutation(fibonacci(40))], 15), ("nineteen_equal", [3] * 19, 7),
            ("288_symbols_limit_9", list(range(1, 289)), 9)]


def every_value_image(rows=8):
    """255 x rows, 8-bit: every row a permutation of 1..255, so that with the type bytes of filter 0 every byte value occurs `rows` times"""
    return np.stack([np.random.default_rng(y).permutation(np.arange(1, 256, dtype=np.uint8)) for y in range(rows)])
