"""tests/pnglz_limits.py without a GPU: every input keeps the property it exists for on the restatement, so none can silently stop
reaching its tile edge, chain bound, length, distance or unit; zlib inflates every file to the filtered bytes and PIL reads it back to
the pixels; the batches are what tests/test_pnglz_sizes.py takes them for (forms, sizes, the pack kernel's split, the parse kernel's
loop count); and wrong encoders, restated through the keyword arguments of pnglz_restatement.tokens, each change the file of the
input named beside them -- an input that no plausible mistake changes would test nothing."""
import io
import zlib

import numpy as np
import pytest

import pnglz_limits as M
import pnglz_problems as Q
import pnglz_restatement as Z
import pngw_restatement as P


def read_back(png, img, data):
    from PIL import Image

    assert zlib.decompress(P.idat_of(png)) == data
    back = np.array(Image.open(io.BytesIO(png)))
    assert back.shape == img.shape and np.array_equal(back.astype(np.uint16), img.astype(np.uint16))


@pytest.mark.parametrize("name", M.names())
def test_limit_keeps_its_property_and_its_files_are_read(name):
    _, img, kind, filt, chains, prop = M.limit(name)
    R = M.restated(name)
    assert prop(R), name
    F = len(R["data"])
    assert F == img.shape[0] * (1 + img.shape[1] * (1, 2, 3)[kind]) and len(R["rank"]) == F - 2
    for chain in chains:
        at = 0
        for p, length, dist in R["tokens"][chain]:  # the invariants
            assert p == at and (dist == 0 and length == 1 or 4 <= length <= 258 and 1 <= dist <= 32768 and dist <= p)
            assert p // 4096 == (p + length - 1) // 4096
            at += length
        assert at == F
        form, ntok, nmatch, L = R["info"][chain]
        assert ntok == len(R["tokens"][chain]) and nmatch == len(Q.matches(R["tokens"][chain]))
        read_back(R["file"][chain], img, R["data"])
        if form == Z.MATCHES:
            assert len(R["file"][chain]) == 63 + L


def test_order_and_rank_are_the_candidates_of_tokens():
    data = b"\0" + M.phrase_bytes(700, 1).tobytes()
    key, order, rank = Z.order_and_rank(data)
    assert sorted(order.tolist()) == list(range(len(data) - 2)) and (rank[order] == np.arange(len(order))).all()
    pairs = [(int(key[p]), int(p)) for p in order]
    assert pairs == sorted(pairs)
    for p, length, dist in Q.matches(Z.tokens(data, 1)):  # chain 1: the source is the position one rank below
        assert rank[p - dist] == rank[p] - 1


# ------------------------------------------------------------------------------------------------ the batches


def test_pack_batches_are_in_the_many_large_images_regime():
    """parts = ceil(nunits / 1024) = 2, where every lane of the pack kernel loops over up to three units; the 16 frames of
    test_pnglz.py::test_batch_of_640x480_frames are in the other branch (64 parts)"""
    F = 128 * 129
    nunits = (F + 15) // 16
    assert (F, nunits) == (16512, 1032)
    for n in M.PACK_CALLS:
        assert n >= 1024 and M.pack_parts(n, nunits) == 2 == -(-nunits // 1024)
        assert -(-nunits // (2 * 256)) == 3
    assert M.pack_parts(16, (480 * 641 + 15) // 16) == 64
    assert M.pack_parts(1, 5) == 1 and M.pack_parts(1, 1 << 26) == 4096 and M.pack_parts(70000, 2) == 1
    files = set()
    for k in range(4):
        img, png, (form, ntok, nmatch, L) = M.pack_frame(k)
        assert form == Z.MATCHES and 1000 < ntok < 4000 and len(png) < 4000
        read_back(png, img, P.filtered(img, 8, P.ADAPTIVE).tobytes())
        files.add(png)
    assert len(files) == 4


def test_parse_batch_passes_the_grid_of_the_parse_kernel():
    contents = M.parse_contents()
    assert M.PARSE_IMAGES * 1 > 8192 * 64 and M.PARSE_IMAGES % 16 and all(c[0].shape == (3, 5) for c in contents)  # one chunk an image
    assert {c[2][0] for c in contents} == {Z.STORED, Z.HUFFMAN} and any(c[2][2] for c in contents)
    assert M.PARSE_IMAGES * (152 * 2 + 4232) < 2.5e9 and max(len(c[1]) for c in contents) <= P.png_bound(5, 3, 8)
    for img, png, _ in contents:
        read_back(png, img, P.filtered(img, 8, P.ADAPTIVE).tobytes())


@pytest.mark.parametrize("w,h", M.STORED_SHAPES)
def test_stored_batches_are_stored_and_split(w, h):
    F = h * (1 + w)
    assert F == {(254, 257): 65535, (255, 256): 65536, (509, 257): 131070, (131070, 1): 131071}[(w, h)]
    assert M.pack_parts(3, (F + 15) // 16) == (16 if F < 70000 else 32)  # the stored bytes are gathered by several workgroups
    for img, png, (form, ntok, nmatch, L) in M.stored_images(w, h)[:2]:
        assert form == Z.STORED and len(png) == P.png_bound(w, h, 8) == 63 + F + 5 * ((F + 65534) // 65535)
        assert png == Z.huffman_only(img, Z.GRAY8, 0)
        read_back(png, img, P.filtered(img, 8, 0).tobytes())


def test_reuse_calls_change_form_and_count():
    calls = M.reuse_calls()
    assert [len(c) for c in calls] == [5, 3, 5]
    assert [c[2][0] for c in calls[0]] == [Z.MATCHES] * 5 and [c[2][0] for c in calls[1]] == [Z.STORED] * 3
    assert [c[2][0] for c in calls[2]] == [Z.MATCHES, Z.STORED, Z.MATCHES, Z.STORED, Z.MATCHES]
    assert len({c[1] for call in calls for c in call}) == 12  # the flat image twice
    for call in calls:
        for img, png, _ in call:
            read_back(png, img, P.filtered(img, 8, P.ADAPTIVE).tobytes())


def test_f32_image_has_every_special_value_in_the_edge_columns():
    a = M.f32_image()
    assert a.shape == (19, 130)
    for col in M.SPECIAL_COLUMNS:
        assert {v.tobytes() for v in a[:, col]} <= {v.tobytes() for v in M.SPECIAL_F32}
    assert {v.tobytes() for col in M.SPECIAL_COLUMNS for v in a[:, col]} == {v.tobytes() for v in M.SPECIAL_F32}
    as_u8 = P.f32_to_u8(a)
    png, (form, _, nmatch, _) = Z.encode(as_u8, Z.GRAY8, P.ADAPTIVE, 4)
    assert form == Z.MATCHES and nmatch > 30
    read_back(png, as_u8, P.filtered(as_u8, 8, P.ADAPTIVE).tobytes())


# ------------------------------------------------------------------------------------------------ wrong encoders


def within(size):
    return {"candidate": lambda r, k: (r - k) // size == r // size}


def not_the_last_rank(name):
    n = len(M.restated(name)["rank"])
    return {"candidate": lambda r, k: r != n - 1}


# (the mistake, the keyword arguments that restate it, the chain's change, the inputs whose file it changes, inputs it leaves alone)
WRONG = [
    ("candidates do not cross a 1024-rank edge (a sort tile of pnglz_order_kernel)", lambda name: within(1024), 0,
     ["sort_pair_1024_first_of_tile", "sort_pair_3072_first_of_tile"], ["sort_pair_1024_last_of_tile", "rank_pair_768_first_of_tile"]),
    ("candidates do not cross a 256-rank edge (a block of pnglz_match_kernel)", lambda name: within(256), 0,
     ["rank_pair_768_first_of_tile", "rank_pair_1280_first_of_tile", "sort_pair_1024_first_of_tile"], ["rank_pair_768_last_of_tile"]),
    ("chain - 1 candidates are searched", lambda name: {}, -1, ["chain4_reaches_candidate_4", "chain64_reaches_candidate_64"],
     ["chain4_stops_before_candidate_5", "chain64_stops_before_candidate_65"]),
    ("chain + 1 candidates are searched", lambda name: {}, 1, ["chain4_stops_before_candidate_5"], ["chain4_reaches_candidate_4"]),
    ("the length is rounded down to a multiple of 8 when the cap is not one (no byte tail in common_prefix)",
     lambda name: {"length_of": lambda length, cap: length - length % 8 if cap % 8 else length}, 0,
     ["match_ends_at_F_cap_%d" % (8 + r) for r in range(1, 8)] + ["every_length_4_to_258"], []),
    ("length 258 is capped to 256", lambda name: {"max_match": 256}, 0, ["every_length_4_to_258", "scan_flat_F16384"], ["distance_symbols_22_to_29"]),
    ("the window is 32767", lambda name: {"window": 32767}, 0, ["distance_symbols_22_to_29"], ["every_length_4_to_258"]),
    ("the position that sorts last is dropped", not_the_last_rank, 0, ["sort_last_rank_alone_in_its_tile"], ["sort_pair_1024_first_of_tile"]),
    ("a match may cross a chunk edge", lambda name: {"chunk": 1 << 40}, 0, ["scan_flat_F16384", "scan_flat_F32769", "scan_phrase_F16393"],
     ["sort_phrase_n3073"]),
]


@pytest.mark.parametrize("mistake", [w[0] for w in WRONG])
def test_a_wrong_encoder_changes_the_named_inputs_file(mistake):
    _, wrong, step, changed, same = next(w for w in WRONG if w[0] == mistake)
    for name, differs in [(n, True) for n in changed] + [(n, False) for n in same]:
        _, img, kind, filt, chains, _ = M.limit(name)
        chain = 4 if 4 in chains else chains[0]
        got = Z.encode(img, kind, filt, chain + step, **wrong(name))[0]
        assert (got != M.restated(name)["file"][chain]) == differs, (mistake, name)
        if differs:  # and it is still a file of the pixels: a mistake of the search, not of the format
            read_back(got, img, M.restated(name)["data"])


def test_a_window_of_32769_changes_the_existing_window_problems_tokens():
    """the one wrong encoder that no new input is needed for: tests/pnglz_problems.py has the pattern at distance 32769"""
    _, img, kind, filt, _ = next(p for p in Q.problems() if p[0] == "window_32768_and_32769")
    R = Q.restated("window_32768_and_32769")
    for chain in Q.CHAINS:  # the wrong encoder's match has no distance symbol: its tokens differ, a file of them cannot be written
        wrong = Z.tokens(R["data"], chain, window=32769)
        assert wrong != R["tokens"][chain] and (600 + 32769, 4, 32769) in wrong
        with pytest.raises(AssertionError):
            Z.encode(img, kind, filt, chain, window=32769)


def test_dropping_the_last_position_is_no_mistake():
    """position F - 3 has the last trigram, but only 3 bytes before F: it starts no match and is no earlier position's candidate, so
    an encoder that leaves it out of the sort writes the same files; the mistake that counts is the last *rank* (above)"""
    for name in ("sort_last_rank_alone_in_its_tile", "match_ends_at_F_cap_9", "sort_phrase_n1025"):
        R = M.restated(name)
        F = len(R["data"])
        assert all(p != F - 3 and p - dist != F - 3 for c in R["tokens"] for p, _, dist in Q.matches(R["tokens"][c]))
