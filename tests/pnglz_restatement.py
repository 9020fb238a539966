"""include/mdc_pnglz.h restated with NumPy on top of tests/pngw_restatement.py (and tests/plots_restatement.py for the RGB kind): the
candidates of every position, the greedy parse inside 4096-byte chunks, the two codes, the block header, the choice between the match
form, the Huffman-only form and the stored form, and the whole file.  Follows the header's words only.  The byte-for-byte oracle of
tests/test_pnglz.py; itself pinned by zlib and PIL in tests/test_pnglz_cpu.py."""
import struct
import zlib

import numpy as np

import plots_restatement as Q
import pngw_restatement as P

STORED, HUFFMAN, MATCHES = 0, 1, 2
GRAY8, GRAY16, RGB8 = 0, 1, 2
MIN_MATCH, MAX_MATCH, WINDOW, CHUNK, MAX_CHAIN = 4, 258, 32768, 4096, 64

# RFC 1951 3.2.5: (first value, extra bits) of the length symbols 257.. and the distance symbols 0..
LENGTH_BASE = [(3, 0), (4, 0), (5, 0), (6, 0), (7, 0), (8, 0), (9, 0), (10, 0), (11, 1), (13, 1), (15, 1), (17, 1), (19, 2), (23, 2), (27, 2), (31, 2),
               (35, 3), (43, 3), (51, 3), (59, 3), (67, 4), (83, 4), (99, 4), (115, 4), (131, 5), (163, 5), (195, 5), (227, 5), (258, 0)]
DIST_BASE = [(1, 0), (2, 0), (3, 0), (4, 0), (5, 1), (7, 1), (9, 2), (13, 2), (17, 3), (25, 3), (33, 4), (49, 4), (65, 5), (97, 5), (129, 6), (193, 6),
             (257, 7), (385, 7), (513, 8), (769, 8), (1025, 9), (1537, 9), (2049, 10), (3073, 10), (4097, 11), (6145, 11), (8193, 12), (12289, 12),
             (16385, 13), (24577, 13)]


def length_symbol(length):
    """-> (symbol, extra value, extra bits); 258 is symbol 285, not 284 with extra 31"""
    assert MIN_MATCH <= length <= MAX_MATCH
    if length == 258:
        return 285, 0, 0
    k = max(i for i, (base, _) in enumerate(LENGTH_BASE[:-1]) if base <= length)
    return 257 + k, length - LENGTH_BASE[k][0], LENGTH_BASE[k][1]


def distance_symbol(dist):
    assert 1 <= dist <= WINDOW
    k = max(i for i, (base, _) in enumerate(DIST_BASE) if base <= dist)
    return k, dist - DIST_BASE[k][0], DIST_BASE[k][1]


def order_and_rank(data):
    """-> (key, order, rank) of the positions p with p + 2 < F: key[p] the trigram as a number, order the positions "by trigram, then
    by position", rank its inverse (rank[order[i]] = i): the candidates of p are order[rank[p] - 1], order[rank[p] - 2], ..."""
    d = np.frombuffer(bytes(data), np.uint8)
    n = max(len(d) - 2, 0)
    key = (d[:n].astype(np.int64) << 16) | (d[1:n + 1].astype(np.int64) << 8) | d[2:n + 2]
    order = np.argsort(key, kind="stable")
    rank = np.empty(n, np.int64)
    rank[order] = np.arange(n)
    return key, order, rank


def tokens(data, chain, *, window=WINDOW, max_match=MAX_MATCH, chunk=CHUNK, candidate=None, length_of=None):
    """-> [(position, length, distance)]: length 1 and distance 0 for a literal.  The candidates of p are its up to `chain`
    predecessors in the order "by trigram, then by position", as long as they share its trigram and lie within the window.
    The keyword arguments are for tests that restate a wrong encoder, and their defaults are the header's rule: candidate(r, k) says
    whether the position of rank r may look at rank r - k (False ends its search), length_of(length, cap) replaces a common length."""
    assert 1 <= chain <= MAX_CHAIN
    d = np.frombuffer(bytes(data), np.uint8)
    F = len(d)
    n = max(F - 2, 0)
    if n:
        key, order, rank = order_and_rank(data)
        order_l, key_l = order.tolist(), key.tolist()
    raw = bytes(data)
    out, p = [], 0
    for start in range(0, F, chunk):
        end = min(F, start + chunk)
        p = start
        while p < end:
            best, best_dist = 0, 0
            cap = min(max_match, F - p, chunk - p % chunk)
            if p + 2 < F and cap >= MIN_MATCH:
                r = int(rank[p])
                for k in range(1, chain + 1):
                    if r - k < 0 or (candidate is not None and not candidate(r, k)):
                        break
                    q = order_l[r - k]
                    if key_l[q] != key_l[p] or p - q > window:
                        break
                    assert q < p
                    if raw[q + 3] != raw[p + 3]:
                        continue  # length 3: never the best that counts
                    a, b = d[q:q + cap], d[p:p + cap]
                    diff = np.flatnonzero(a != b)
                    length = int(diff[0]) if diff.size else cap
                    if length_of is not None:
                        length = length_of(length, cap)
                    if length > best:  # of equal lengths the nearest, which came first
                        best, best_dist = length, p - q
                    if best == cap:
                        break
            if best >= MIN_MATCH:
                out.append((p, best, best_dist))
                p += best
            else:
                out.append((p, 1, 0))
                p += 1
    return out


def block_codes(ll_hist, d_hist):
    """both codes and the block header of the two histograms -> (literal/length lengths, distance lengths, the header's Bits)"""
    ll_len, d_len = P.huffman_lengths(ll_hist, 15), P.huffman_lengths(d_hist, 15)
    nlit = max([257] + [s + 1 for s in range(257, 286) if ll_len[s]])
    ndist = max([1] + [s + 1 for s in range(30) if d_len[s]])
    pairs = P.run_length_code(ll_len[:nlit] + d_len[:ndist])
    clhist = [0] * 19
    for s, _ in pairs:
        clhist[s] += 1
    cllen = P.huffman_lengths(clhist, 7)
    clcodes = P.canonical_codes(cllen)
    hclen = max([4] + [i + 1 for i in range(19) if cllen[P.CL_ORDER[i]]])
    bits = P.Bits()
    bits.put(1, 1)
    bits.put(2, 2)
    bits.put(nlit - 257, 5)
    bits.put(ndist - 1, 5)
    bits.put(hclen - 4, 4)
    for i in range(hclen):
        bits.put(cllen[P.CL_ORDER[i]], 3)
    for s, extra in pairs:
        bits.put_code(clcodes[s], cllen[s])
        if s >= 16:
            bits.put(extra, {16: 2, 17: 3, 18: 7}[s])
    return ll_len, d_len, bits


def match_block(data, toks):
    """one dynamic block with the matches of `toks` -> bytes"""
    d = np.frombuffer(bytes(data), np.uint8)
    ll_hist, d_hist = [0] * 286, [0] * 30
    ll_hist[256] = 1
    pieces = []  # (kind, value, extra value, extra bits): kind 0 literal/length symbol, 1 distance symbol
    for p, length, dist in toks:
        if dist == 0:
            ll_hist[int(d[p])] += 1
            pieces.append((0, int(d[p]), 0, 0))
        else:
            s, e, nb = length_symbol(length)
            ll_hist[s] += 1
            pieces.append((0, s, e, nb))
            s, e, nb = distance_symbol(dist)
            d_hist[s] += 1
            pieces.append((1, s, e, nb))
    ll_len, d_len, bits = block_codes(ll_hist, d_hist)
    ll_codes, d_codes = P.canonical_codes(ll_len), P.canonical_codes(d_len)
    # the data: every piece is a reversed code and then its extra bits, LSB-first
    rev = [[P.reverse_bits(ll_codes[s], ll_len[s]) for s in range(286)], [P.reverse_bits(d_codes[s], d_len[s]) for s in range(30)]]
    lens = [ll_len, d_len]
    vals, counts = [], []
    for kind, s, e, nb in pieces:
        assert lens[kind][s] > 0
        vals.append(rev[kind][s] | (e << lens[kind][s]))
        counts.append(lens[kind][s] + nb)
    vals.append(rev[0][256])
    counts.append(ll_len[256])
    vals, counts = np.asarray(vals, np.int64), np.asarray(counts, np.int64)
    at = bits.n + np.concatenate(([0], np.cumsum(counts)[:-1]))
    total = bits.n + int(counts.sum())
    stream = np.zeros((total + 7) // 8 * 8, np.uint8)
    head = np.frombuffer(bits.value.to_bytes((bits.n + 7) // 8, "little"), np.uint8)
    stream[:bits.n] = np.unpackbits(head, bitorder="little")[:bits.n]
    for k in range(int(counts.max())):
        m = counts > k
        stream[at[m] + k] = (vals[m] >> k) & 1
    return np.packbits(stream, bitorder="little").tobytes()


def deflate(data, chain, **wrong):
    """-> (the DEFLATE stream, the form, tokens, matches, L): the choice of form of the header (wrong: see tokens)"""
    data = bytes(data)
    toks = tokens(data, chain, **wrong)
    nmatch = sum(1 for t in toks if t[2])
    with_matches = match_block(data, toks)
    huffman, _ = P.dynamic_block(data)
    L, H, S = len(with_matches), len(huffman), P.stored_size(len(data))
    if nmatch == 0:
        assert with_matches == huffman
    if L < H and L < S:
        return with_matches, MATCHES, len(toks), nmatch, L
    if H < S:
        return huffman, HUFFMAN, len(toks), nmatch, L
    return P.stored_blocks(data), STORED, len(toks), nmatch, L


def filtered(img, kind, filt):
    if kind == RGB8:
        return Q.filtered_rgb(img, filt)
    return P.filtered(img, 16 if kind == GRAY16 else 8, filt)


def encode(img, kind, filt, chain, **wrong):
    """-> (the file, (form, tokens, matches, L)); wrong: see tokens"""
    img = np.asarray(img)
    h, w = img.shape[:2]
    data = filtered(img, kind, filt).tobytes()
    stream, form, ntok, nmatch, L = deflate(data, chain, **wrong)
    idat = b"\x78\x01" + stream + struct.pack(">I", zlib.adler32(data))
    ihdr = struct.pack(">IIBBBBB", w, h, 16 if kind == GRAY16 else 8, 2 if kind == RGB8 else 0, 0, 0, 0)
    out = P.SIGNATURE + P.chunk(b"IHDR", ihdr) + struct.pack(">I", len(idat)) + b"IDAT" + idat + struct.pack(">I", zlib.crc32(b"IDAT" + idat)) + P.chunk(b"IEND", b"")
    return out, (form, ntok, nmatch, L)


def huffman_only(img, kind, filt):
    """the file of libmdc_pngw.so / libmdc_pngw_rgb.so for the same pixels, restated"""
    if kind == RGB8:
        return Q.encode_rgb(img, filt)[0]
    return P.encode(img, 16 if kind == GRAY16 else 8, filt)[0]
