"""The host image decoders pinned on a corpus (no GPU): every file of tests/golden/codecs/ -- baseline and progressive JPEG,
every PNG flavour, PGM -- intact, truncated, with single bits flipped and with bytes forced to 0xFF, plus hand-made files for
the places where the three JPEG paths of the reader (device Huffman stream, coefficient record, host pixels) judge a file
differently.  Each case goes through capi.decode_gray8, capi.decode_jpeg_record and capi.jpeg_stream; accepted or refused, size,
a digest of the output bytes and the exact error text must equal tests/golden/codecs/expected.npz, recorded by
tests/golden/codecs/make_codecs.py from the decoders as they were before their shared parts were merged."""
import hashlib
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "codecs")

FILES = (
    "b_gray.jpg", "b_444.jpg", "b_422.jpg", "b_420.jpg", "b_411.jpg", "b_opt.jpg", "b_rst_blocks.jpg", "b_rst_rows.jpg", "b_odd.jpg",
    "b_odd_420.jpg", "b_rgb_adobe.jpg", "p_gray.jpg", "p_420.jpg", "p_rst.jpg",
    "g1.png", "g2.png", "g4.png", "g8.png", "g16.png", "ga.png", "rgb8.png", "rgb16.png", "rgba.png", "pal4.png", "pal8.png",
    "lace_g8.png", "lace_rgb16.png", "g8.pgm", "g16.pgm")
ENTRIES = ("decode_gray8", "decode_jpeg_record", "jpeg_stream")
MAX_SIDE = 96            # no fixture is larger; the record buffer is sized for it
STREAM_CAP = 96 * 1024   # header + two chroma tables + the entropy-coded bytes of an 8-KB file
N_TRUNC, N_FLIP, N_FF = 15, 32, 8


def lcg(state):
    """The generator of the mutations: explicit, so that no library's version decides which bits are flipped."""
    return (state * 1103515245 + 12345) & 0x7FFFFFFF


def mutations(data, index):
    """-> [(label, bytes)]: the file itself, 15 truncations at len * t / 16, 32 single-bit flips, 8 bytes forced to 0xFF"""
    out = [("intact", data)]
    out += [("cut%02d" % t, data[: len(data) * t // 16]) for t in range(1, N_TRUNC + 1)]
    s = 20240607 + 7919 * index
    for k in range(N_FLIP):
        s = lcg(s)
        bit = (s >> 4) % (len(data) * 8)
        b = bytearray(data)
        b[bit >> 3] ^= 1 << (bit & 7)
        out.append(("flip%02d@%d.%d" % (k, bit >> 3, bit & 7), bytes(b)))
    for k in range(N_FF):
        s = lcg(s)
        at = (s >> 4) % len(data)
        b = bytearray(data)
        b[at] = 0xFF
        out.append(("ff%02d@%d" % (k, at), bytes(b)))
    return out


def segment(data, marker, nth=0):
    """-> offset of the nth FF <marker> among the segments of a JPEG file (the marker's FF byte)"""
    p = 2
    while p + 4 <= len(data):
        assert data[p] == 0xFF
        m = data[p + 1]
        if m == marker:
            if nth == 0:
                return p
            nth -= 1
        assert m != 0xDA, "marker %02x not found before the scan" % marker
        p += 2 + (data[p + 2] << 8 | data[p + 3])
    raise AssertionError("marker %02x not found" % marker)


def patched(data, at, new):
    return data[:at] + bytes(new) + data[at + len(new):]


def png_with_filter_type(data, row, ft):
    """the non-interlaced PNG `data` with the filter-type byte of one row replaced (the row's bytes stay)"""
    import struct
    import zlib

    chunks, p = [], 8
    while p < len(data):
        n = struct.unpack(">I", data[p: p + 4])[0]
        chunks.append((data[p + 4: p + 8], data[p + 8: p + 8 + n]))
        p += 12 + n
    w, _, depth, ctype = struct.unpack(">IIBB", chunks[0][1][:10])
    raw = bytearray(zlib.decompress(b"".join(body for tag, body in chunks if tag == b"IDAT")))
    raw[row * (1 + (w * {0: 1, 2: 3}[ctype] * depth + 7) // 8)] = ft
    out, done = data[:8], False
    for tag, body in chunks:
        if tag == b"IDAT":
            if done:
                continue
            body, done = zlib.compress(bytes(raw), 6), True
        out += struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body) & 0xFFFFFFFF)
    return out


def hand_made(files):
    """-> [(label, bytes)]: one file for each place where the decoders' rules differ, and for each kind of broken table or header"""
    out = []
    # PNG compression-method byte (IHDR byte 10 = file offset 26): the 8-bit-gray fast path does not look at it, the general decoder refuses
    for name in ("g8.png", "rgb8.png"):
        out.append(("compression_method_1:" + name, patched(files[name], 26, [1])))
        out.append(("filter_method_1:" + name, patched(files[name], 27, [1])))
        # filter types: each one on the first row (no row above) and on a later one, without re-filtering; 5 is no filter type
        for row in (0, 3):
            for ft in (1, 2, 3, 4, 5):
                out.append(("row%d_filter_type_%d:%s" % (row, ft, name), png_with_filter_type(files[name], row, ft)))
    for name in ("b_gray.jpg", "b_444.jpg", "p_gray.jpg", "p_420.jpg"):
        d = files[name]
        sof = segment(d, 0xC2 if name.startswith("p_") else 0xC0)
        sos = segment(d, 0xDA)
        dht = segment(d, 0xC4)
        ns = d[sos + 4]
        # a stray RST0 between two segments: jpeg_stream refuses, the others skip it
        out.append(("stray_rst0:" + name, d[:2] + b"\xff\xd0" + d[2:]))
        out.append(("stray_rst0_before_sos:" + name, d[:sos] + b"\xff\xd0" + d[sos:]))
        # frames of 2 and 4 components: each decoder's own "unsupported frame header"
        out.append(("sof_2_components:" + name, patched(d, sof + 9, [2])))
        out.append(("sof_4_components:" + name, patched(d, sof + 9, [4])))
        # a frame header cut to 6 bytes: no room for a component; jpeg_stream calls that a sample-size fault, the decoders a frame fault
        out.append(("sof_6_bytes:" + name, d[:sof + 2] + b"\x00\x08" + d[sof + 4: sof + 10] + d[sof + 2 + (d[sof + 2] << 8 | d[sof + 3]):]))
        out.append(("sof_12_bit:" + name, patched(d, sof + 4, [12])))
        out.append(("sof_sampling_5x1:" + name, patched(d, sof + 11, [0x51])))
        # Huffman table definitions: counts that run past the segment, counts no prefix code has
        out.append(("dht_counts_past_segment:" + name, patched(d, dht + 5 + 15, [0xFF])))
        counts = list(d[dht + 5: dht + 21])
        big = max(range(1, 16), key=lambda i: counts[i])
        assert counts[0] < 3 and counts[big] >= 3 - counts[0]
        counts[big] -= 3 - counts[0]  # (the number of symbols stays)
        counts[0] = 3
        out.append(("dht_three_codes_of_one_bit:" + name, patched(d, dht + 5, counts)))
        out.append(("dht_table_class_2:" + name, patched(d, dht + 4, [0x20])))
        # a scan that names tables no DHT defined
        out.append(("sos_missing_tables:" + name, patched(d, sos + 6, [0x33])))
        out.append(("sos_table_index_4:" + name, patched(d, sos + 6, [0x44])))
        out.append(("sos_unknown_component:" + name, patched(d, sos + 5, [9])))
        if ns == 3:  # scan components out of frame order
            out.append(("sos_components_swapped:" + name, patched(d, sos + 5, [d[sos + 9], d[sos + 6], d[sos + 7], d[sos + 8], d[sos + 5]])))
        dqt = segment(d, 0xDB)
        out.append(("dqt_table_index_4:" + name, patched(d, dqt + 4, [0x04])))
        out.append(("no_dqt:" + name, d[:dqt] + d[dqt + 2 + (d[dqt + 2] << 8 | d[dqt + 3]):]))
        out.append(("no_dht:" + name, d[:dht] + d[dht + 2 + (d[dht + 2] << 8 | d[dht + 3]):]))
        out.append(("sos_before_sof:" + name, d[:sof] + d[sos:]))
        out.append(("eoi_only:" + name, d[:sos] + b"\xff\xd9"))
    return out


def digest(a):
    return int.from_bytes(hashlib.blake2b(a.tobytes(), digest_size=6).digest(), "little")


def run_case(data):
    """-> for each of ENTRIES: (ok, w, h, digest of the output bytes, error text)"""
    from mono_dataset_code_amd import capi

    res = []
    try:
        a = capi.decode_gray8(data)
        res.append((1, a.shape[1], a.shape[0], digest(a), ""))
    except ValueError as e:
        res.append((0, 0, 0, 0, str(e)))
    rec_bytes, pitch, _ = capi.jpeg_record_bytes(MAX_SIDE, MAX_SIDE)
    rec = np.zeros(rec_bytes, np.uint8)
    try:
        w, h, bw, rows = capi.decode_jpeg_record(data, rec, pitch)
        res.append((1, w, h, digest(rec[: 128 + bw * rows * 128]), ""))  # quantisation table + coefficients
    except ValueError as e:
        res.append((0, 0, 0, 0, str(e)))
    stream = np.zeros(STREAM_CAP, np.uint8)
    try:
        used, w, h = capi.jpeg_stream(data, stream)
        res.append((1, w, h, digest(stream[:used]), ""))
    except ValueError as e:
        res.append((0, 0, 0, 0, str(e)))
    return res


def read_files():
    return {name: open(os.path.join(GOLDEN, name), "rb").read() for name in FILES}


def groups():
    """-> [(group name, [(label, bytes)])] in the order of expected.npz: one group per file, then the hand-made files"""
    files = read_files()
    return [(name, mutations(files[name], i)) for i, name in enumerate(FILES)] + [("hand_made", hand_made(files))]


@pytest.fixture(scope="module")
def expected():
    e = np.load(os.path.join(GOLDEN, "expected.npz"), allow_pickle=False)
    return {k: e[k] for k in e.files}


@pytest.fixture(scope="module")
def corpus():
    return groups()


def test_corpus_is_what_was_recorded(expected, corpus):
    assert [g for g, _ in corpus] == list(expected["groups"])
    assert [len(c) for _, c in corpus] == list(expected["group_sizes"])
    assert all(len(c) == 1 + N_TRUNC + N_FLIP + N_FF for _, c in corpus[:-1])
    assert all(len(open(os.path.join(GOLDEN, f), "rb").read()) <= 8192 for f in FILES)


@pytest.mark.parametrize("group", range(len(FILES) + 1), ids=list(FILES) + ["hand_made"])
def test_decoders_on_the_corpus(group, expected, corpus):
    first = int(np.sum(expected["group_sizes"][:group]))
    msgs = list(expected["messages"])
    wrong = []
    for k, (label, data) in enumerate(corpus[group][1]):
        for e, got in enumerate(run_case(data)):
            code = int(expected["code"][first + k, e])
            want = (1, int(expected["w"][first + k, e]), int(expected["h"][first + k, e]), int(expected["digest"][first + k, e]), "") if code == 0 \
                else (0, 0, 0, 0, msgs[code - 1])
            if got != want:
                wrong.append((label, ENTRIES[e], got, want))
    assert not wrong, "%d results differ, the first: %r" % (len(wrong), wrong[:3])


def test_the_divergences_stay(expected, corpus):
    """What the hand-made files are there for, stated (not only recorded): the three paths keep their own rules and texts."""
    first = int(np.sum(expected["group_sizes"][:-1]))
    msgs = [""] + list(expected["messages"])
    got = {label: tuple(msgs[int(c)] for c in expected["code"][first + k]) for k, (label, _) in enumerate(corpus[-1][1])}
    assert got["compression_method_1:g8.png"][0] == "" and got["compression_method_1:rgb8.png"][0] == "PNG: unknown compression / filter method"
    assert all(got["row%d_filter_type_5:%s" % (r, f)][0] == "PNG: bad filter type" for r in (0, 3) for f in ("g8.png", "rgb8.png"))
    assert all(got["row%d_filter_type_%d:%s" % (r, t, f)][0] == "" for r in (0, 3) for t in (1, 2, 3, 4) for f in ("g8.png", "rgb8.png"))
    assert got["stray_rst0:b_gray.jpg"] == ("", "", "JPEG: restart marker outside a scan")
    assert got["sof_2_components:b_444.jpg"] == ("JPEG: unsupported frame header",) * 2 + ("JPEG stream: unsupported frame header",)
    assert got["sof_4_components:p_420.jpg"] == ("JPEG: unsupported frame header",) * 2 + ("JPEG stream: not a sequential Huffman file",)
    assert got["sof_6_bytes:b_gray.jpg"] == ("JPEG: unsupported frame header",) * 2 + ("JPEG: only 8-bit samples are supported",)
    assert got["sos_components_swapped:b_444.jpg"] == ("JPEG: unexpected component order",) * 2 + ("JPEG stream: scan components out of frame order",)
    assert got["dht_counts_past_segment:b_gray.jpg"] == ("JPEG: bad DHT",) * 3
    assert got["dht_three_codes_of_one_bit:b_gray.jpg"] == ("JPEG: bad Huffman table",) * 3
    assert got["sos_missing_tables:b_gray.jpg"] == ("JPEG: scan refers to a missing table",) * 3
