"""A NumPy / plain Python restatement of the JPEG encoder with per-frame optimal Huffman tables that include/mdc_jopt.h specifies
(tests/test_jopt_cpu.py pins it to libjpeg-turbo's optimize_coding through PIL, byte for byte), on top of tests/jenc_restatement.py:
the symbol counts of a frame, jpeg_gen_optimal_table of jchuff.c transcribed line by line, the DHT segments that list only the
symbols used, and the scan coded with those tables.  Nothing here is fast; it is the specification in executable form."""
import io

import numpy as np

import jenc_restatement as R

MAX_CLEN = 32
SEARCH_LIMIT = 1000000000


def _category(v):
    """the JPEG size category: bits of |v|, 0 for 0 (exact, no logarithm)"""
    a = np.abs(np.asarray(v, np.int64))
    c = np.zeros(a.shape, np.int64)
    for k in range(16):
        c += (a >> k) > 0
    return c


def symbols(zz):
    """the code of a coefficient array (blocks x 64, zigzag) as items (block, key, table, symbol, amplitude bits, their count),
    key ordering the items inside a block; table 0 = DC, 1 = AC"""
    zz = np.asarray(zz, np.int64)
    nb = zz.shape[0]
    diff = zz[:, 0] - np.concatenate([[0], zz[:-1, 0]])
    cat = _category(diff)
    amp = np.where(diff < 0, diff - 1, diff) & ((1 << cat) - 1)
    items = [(np.arange(nb), np.zeros(nb, np.int64), np.zeros(nb, np.int64), cat, amp, cat)]
    bi, ki = np.nonzero(zz[:, 1:])
    ki = ki + 1
    v = zz[bi, ki]
    first = np.concatenate([[True], bi[1:] != bi[:-1]]) if bi.size else np.zeros(0, bool)
    prev = np.where(first, 0, np.concatenate([[0], ki[:-1]]))
    run = ki - prev - 1
    cat = _category(v)
    amp = np.where(v < 0, v - 1, v) & ((1 << cat) - 1)
    one = np.ones(bi.size, np.int64)
    items.append((bi, ki * 4 + 3, one, ((run & 15) << 4) | cat, amp, cat))
    for z in range(3):  # up to three ZRL in front of a coefficient
        m = run // 16 > z
        n = int(m.sum())
        items.append((bi[m], ki[m] * 4 + z, np.ones(n, np.int64), np.full(n, 0xF0), np.zeros(n, np.int64), np.zeros(n, np.int64)))
    last = np.zeros(nb, np.int64)
    last[bi] = ki
    m = last < 63
    n = int(m.sum())
    items.append((np.nonzero(m)[0], np.full(n, 64 * 4), np.ones(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)))
    blk, key, tab, sym, amp, n = [np.concatenate([it[i] for it in items]).astype(np.int64) for i in range(6)]
    order = np.lexsort((key, blk))
    return tab[order], sym[order], amp[order], n[order]


def histograms(zz):
    """-> (dc, ac): 257 counts each (entry 256 is 0), what the frame's code uses of every symbol"""
    tab, sym, _, _ = symbols(zz)
    dc = np.bincount(sym[tab == 0], minlength=257).astype(np.int64)
    ac = np.bincount(sym[tab == 1], minlength=257).astype(np.int64)
    return dc, ac


def optimal_table(freq, strict=False):
    """jpeg_gen_optimal_table (jchuff.c, libjpeg 6b / libjpeg-turbo), line by line.  freq: 257 counts, entry 256 ignored.
    -> (bits[16], vals, depth before limiting), or (None, None, depth) where libjpeg aborts (a code deeper than 32).
    strict: the searches with `<` instead of `<=` (the smallest index among equal counts) -- NOT libjpeg's rule; tests use it to
    show that the tie-break decides the file."""
    freq = [int(x) for x in freq[:256]] + [1]
    bits = [0] * (MAX_CLEN + 1)
    codesize = [0] * 257
    others = [-1] * 257

    def least(exclude):
        """libjpeg's loop `for i in 0..256: if freq[i] && freq[i] <= v && i != exclude: v = freq[i]; c = i` with v starting at the
        limit: the least count, and among equal counts the last index (strict: the first)"""
        f = np.array(freq, np.int64)
        i = np.nonzero((f > 0) & (f <= SEARCH_LIMIT) & (np.arange(257) != exclude))[0]
        if i.size == 0:
            return -1
        i = i[f[i] == f[i].min()]
        return int(i[0] if strict else i[-1])

    while True:
        c1 = least(-1)
        c2 = least(c1)
        if c2 < 0:
            break
        freq[c1] += freq[c2]
        freq[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    depth = max(codesize)
    if depth > MAX_CLEN:
        return None, None, depth
    for i in range(257):
        if codesize[i]:
            bits[codesize[i]] += 1
    if depth == 0:  # no symbol at all: libjpeg never gets here
        return [0] * 16, [], 0
    for i in range(MAX_CLEN, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1
    vals = [j for i in range(1, MAX_CLEN + 1) for j in range(256) if codesize[j] == i]
    return bits[1:17], vals, depth


def dht(table_class, bits, vals):
    return b"\xff\xc4" + (2 + 1 + 16 + len(vals)).to_bytes(2, "big") + bytes([table_class << 4]) + bytes(bits) + bytes(vals)


def encode_u8(u8, quality, strict=False):
    """the file of include/mdc_jopt.h; a frame with a table deeper than 32 is the baseline file"""
    h, w = u8.shape
    zz = R.coefficients(u8, quality)
    tab, sym, amp, n = symbols(zz)
    fdc, fac = histograms(zz)
    dbits, dvals, _ = optimal_table(fdc, strict)
    abits, avals, _ = optimal_table(fac, strict)
    if dbits is None or abits is None:
        return R.encode_u8(u8, quality)
    code, length = np.zeros((2, 256), np.int64), np.zeros((2, 256), np.int64)
    for t, (b, v) in enumerate(((dbits, dvals), (abits, avals))):
        for s, (c, ln) in R.huffman_codes(b, v).items():
            code[t, s], length[t, s] = c, ln
    assert (length[tab, sym] > 0).all()
    val = (code[tab, sym] << n) | amp
    n = n + length[tab, sym]
    total = int(n.sum())
    start = np.cumsum(n) - n
    pos = np.arange(total) - np.repeat(start, n)
    bit = (np.repeat(val, n) >> (np.repeat(n, n) - 1 - pos)) & 1
    bit = np.concatenate([bit, np.ones(-total % 8, np.int64)])
    scan = np.packbits(bit.astype(np.uint8)).tobytes().replace(b"\xff", b"\xff\x00")
    head = R.header(w, h, quality)
    return head[:102] + dht(0, dbits, dvals) + dht(1, abits, avals) + head[-10:] + scan + b"\xff\xd9"


def encode_f32(f, quality):
    return encode_u8(R.to_u8(f), quality)


def bound(w, h):
    """mdcjo_jpeg_bound: 1024 + 418 per block"""
    return 1024 + 418 * ((w + 7) // 8) * ((h + 7) // 8)


def dht_segments(jpeg):
    """the DHT segments of a file, in order"""
    out, at = [], 2
    while jpeg[at:at + 2] != b"\xff\xda":
        n = int.from_bytes(jpeg[at + 2:at + 4], "big")
        if jpeg[at:at + 2] == b"\xff\xc4":
            out.append(jpeg[at:at + 2 + n])
        at += 2 + n
    return out


def pil_encode(u8, quality):
    """the pin: libjpeg-turbo through PIL with optimize_coding"""
    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(u8), "L").save(buf, "JPEG", quality=quality, optimize=True)
    return buf.getvalue()
