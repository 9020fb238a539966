"""The directed inputs of the LZ77 PNG encoder (include/mdc_pnglz.h), each small.  A problem is (name, image, kind, filter, property):
the property is a predicate over the restatement's token lists {chain: [(position, length, distance)]} and forms {chain: form} of
the filtered bytes -- the case the problem exists for.  tests/test_pnglz_cpu.py asserts it, so a problem cannot silently stop
exercising its case; tests/test_pnglz.py runs every problem on the device."""
import numpy as np

import pnglz_restatement as Z

CHAINS = (1, 4, 64)
ADAPTIVE = 5


def matches(toks):
    return [t for t in toks if t[2]]


def row_image(content):
    """a 1-row 8-bit image whose filtered bytes under filter 0 are 0 (the type) and then `content`"""
    return np.asarray(content, np.uint8).reshape(1, -1)


def unique_filler(rng, n, avoid=()):
    """n random bytes 16..255 (directed patterns use the values below 16)"""
    return rng.integers(16, 256, n).astype(np.uint8)


def flat_row(F):
    return row_image(np.full(F - 1, 7, np.uint8))


def ends_at(toks, where):
    return any(t[2] and t[0] + t[1] == where for t in toks)


def window_problem():
    """256 x 130, filter 0, F = 33 410: (1, 2, 3, 4) at 300 and 300 + 32768 (taken), (9, 8, 7, 6) at 600 and 600 + 32769 (not)"""
    rng = np.random.default_rng(43)
    data = unique_filler(rng, 130 * 257)
    data[0::257] = 0
    for at, pat in ((300, (1, 2, 3, 4)), (300 + 32768, (1, 2, 3, 4)), (600, (9, 8, 7, 6)), (600 + 32769, (9, 8, 7, 6))):
        assert at % 257 and (at + 3) // 257 == at // 257
        data[at:at + 4] = pat
    return data.reshape(130, 257)[:, 1:].copy()


def second_nearest_problem():
    """... a b c d e f g h ... a b c d Q ... a b c d e f g h: the nearest candidate gives 4, the one behind it 8"""
    rng = np.random.default_rng(2)
    long_, short = [1, 2, 3, 4, 5, 6, 7, 8], [1, 2, 3, 4, 15]
    return row_image(np.concatenate([unique_filler(rng, 20), long_, unique_filler(rng, 20), short, unique_filler(rng, 20), long_, unique_filler(rng, 9)]))


def equal_lengths_problem():
    """a b c d X ... a b c d Y ... a b c d Z: both candidates give 4, the nearest wins"""
    rng = np.random.default_rng(3)
    return row_image(np.concatenate([unique_filler(rng, 10), [1, 2, 3, 4, 11], unique_filler(rng, 30), [1, 2, 3, 4, 12], unique_filler(rng, 17), [1, 2, 3, 4, 13],
                                     unique_filler(rng, 5)]))


def overlap_problem():
    rng = np.random.default_rng(4)
    return row_image(np.concatenate([unique_filler(rng, 8), [1] * 20, unique_filler(rng, 8), [2, 3] * 10, unique_filler(rng, 8), [4, 5, 6] * 8, unique_filler(rng, 8)]))


def every_symbol_problem():
    """a match of the first length of every length symbol 258..285 (257 is length 3, below the minimum) out of a block of random bytes,
    then matches of length 4 at the first distance of the distance symbols 0..21"""
    rng = np.random.default_rng(5)
    parts = [unique_filler(rng, 2700), unique_filler(rng, 1396)]  # the sources lie one behind the other in the first, a byte apart;
    # the second ends at a multiple of 4096, so that no copy is cut
    src = 0
    for base, _ in Z.LENGTH_BASE[1:]:
        parts += [parts[0][src:src + base], np.asarray([int(rng.integers(0, 16))], np.uint8)]
        src += base + 1
    for base, _ in Z.DIST_BASE[:22]:
        if base < 4:
            period = unique_filler(rng, base)
            parts += [np.tile(period, 8)[:base + 6], np.asarray([int(rng.integers(0, 16))], np.uint8)]
        else:
            block = unique_filler(rng, base)
            parts += [block, block[:4], np.asarray([int(rng.integers(0, 16))], np.uint8)]
    return row_image(np.concatenate(parts))


def skewed_noise():
    """sixteen values at random: Huffman's 4 bits a byte beat the stored form, and the many short matches cost more than they save"""
    return np.random.default_rng(6).integers(0, 16, (48, 64)).astype(np.uint8) * 17


def bordered(kind, w, h, seed):
    """a smooth image inside a flat border: the files this encoder is for"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == Z.GRAY16:
        img = (xx * 301 + yy * 77 + rng.integers(0, 3, (h, w))).astype(np.uint16)
        img[:3], img[-3:], img[:, :4], img[:, -4:] = 0, 0, 0, 0
        return img
    img = np.stack([xx * 2 + yy, xx + yy * 3, (xx * yy) // 16], axis=2).astype(np.uint8)
    img[:3], img[-3:], img[:, :4], img[:, -4:] = 0, 0, 0, 0
    return img


def lengths_of(R):
    return {Z.length_symbol(t[1])[0] for t in matches(R["tokens"][64])}


def distances_of(R, chain=64):
    return {Z.distance_symbol(t[2])[0] for t in matches(R["tokens"][chain])}


def problems():
    T = lambda R, c=4: R["tokens"][c]  # noqa: E731
    out = [
        ("F4095", flat_row(4095), Z.GRAY8, 0, lambda R: ends_at(T(R), 4095)),
        ("F4096", flat_row(4096), Z.GRAY8, 0, lambda R: ends_at(T(R), 4096)),
        ("F4097", flat_row(4097), Z.GRAY8, 0, lambda R: ends_at(T(R), 4096) and T(R)[-1] == (4096, 1, 0)),
        ("flat_64x64_F4160", np.full((64, 64), 7, np.uint8), Z.GRAY8, 0, lambda R: ends_at(T(R), 4096) and any(t[0] == 4096 and t[2] for t in T(R))),
        ("flat_row_600", flat_row(601), Z.GRAY8, 0, lambda R: [t[1] for t in T(R)] == [1, 1, 258, 258, 83]),
        ("1x1", np.array([[9]], np.uint8), Z.GRAY8, 0, lambda R: T(R) == [(0, 1, 0), (1, 1, 0)]),
        ("2x1", np.array([[9, 9]], np.uint8), Z.GRAY8, 0, lambda R: not matches(T(R)) and len(T(R)) == 3),
        ("1x2", np.array([[0], [0]], np.uint8), Z.GRAY8, 0, lambda R: T(R) == [(0, 1, 0), (1, 1, 0), (2, 1, 0), (3, 1, 0)]),
        ("window_32768_and_32769", window_problem(), Z.GRAY8, 0, lambda R: all(matches(T(R, c)) == [(300 + 32768, 4, 32768)] for c in CHAINS)),
        ("second_nearest_is_longer", second_nearest_problem(), Z.GRAY8, 0,
         lambda R: [t[1:] for t in matches(T(R, 1))] == [(4, 28), (4, 25), (4, 53)] and [t[1:] for t in matches(T(R, 4))] == [(4, 28), (8, 53)]),
        ("equal_lengths_nearest_wins", equal_lengths_problem(), Z.GRAY8, 0, lambda R: [t[1:] for t in matches(T(R))] == [(4, 35), (4, 22)]),
        ("overlapping_source", overlap_problem(), Z.GRAY8, 0, lambda R: [t[1:] for t in matches(T(R))] == [(19, 1), (18, 2), (21, 3)]),
        ("one_distance_symbol", np.zeros((8, 8), np.uint8), Z.GRAY8, 0, lambda R: T(R) == [(0, 1, 0), (1, 71, 1)] and R["form"][4] == Z.MATCHES),
        ("every_length_symbol_22_distance_symbols", every_symbol_problem(), Z.GRAY8, 0,
         lambda R: lengths_of(R) >= set(range(258, 286)) and len(distances_of(R)) >= 20),
        ("noise_is_stored", np.random.default_rng(7).integers(0, 256, (64, 64)).astype(np.uint8), Z.GRAY8, 0,
         lambda R: all(R["form"][c] == Z.STORED for c in CHAINS)),
        ("skewed_noise_stays_huffman_only", skewed_noise(), Z.GRAY8, 0, lambda R: all(R["form"][c] == Z.HUFFMAN and matches(T(R, c)) for c in CHAINS)),
    ]
    for kind, name, w, h in ((Z.GRAY16, "gray16", 40, 24), (Z.RGB8, "rgb8", 33, 17)):
        for filt in (0, 1, 2, 3, 4, ADAPTIVE):
            out.append(("%s_filter%d" % (name, filt), bordered(kind, w, h, filt), kind, filt, lambda R: R["form"][4] == Z.MATCHES and matches(T(R))))
    return out


_restated = {}


def restated(name):
    """the restatement's answers for a problem, computed once: {"data", "tokens": {chain: list}, "form": {chain: form}, "file": {chain:
    bytes}, "info": {chain: (form, tokens, matches, L)}, "huffman_only": the file of the Huffman-only encoder}"""
    if name not in _restated:
        _, img, kind, filt, _ = next(p for p in problems() if p[0] == name)
        data = Z.filtered(img, kind, filt).tobytes()
        R = {"data": data, "tokens": {}, "form": {}, "file": {}, "info": {}, "huffman_only": Z.huffman_only(img, kind, filt)}
        for c in CHAINS:
            R["tokens"][c] = Z.tokens(data, c)
            R["file"][c], R["info"][c] = Z.encode(img, kind, filt, c)
            R["form"][c] = R["info"][c][0]
        _restated[name] = R
    return _restated[name]
