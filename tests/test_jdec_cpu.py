"""The hand-built JPEG files of tests/jdec_problems.py through the host half of the device Huffman path, WITHOUT a GPU: the host decoder's
record (mdch_decode_jpeg_record) and the record a sequential decoder makes of the device tables (mdch_jpeg_stream +
test_jpeg_stream_cpu.sequential_decode) both equal the coefficient grid the writer encoded, over the whole MCU-padded luma grid;
the host decoder's pixels equal Pillow's where libjpeg is a reference.  The kernels' own run of the same cases: tests/test_jdec.py."""
import collections
import io

import numpy as np
import pytest
from PIL import Image

import jdec_problems as P
from test_jpeg_stream_cpu import parse_header, sequential_decode
from test_reader import islow_idct_reference


def pil_gray(data):
    im = Image.open(io.BytesIO(data))
    im.draft("L", im.size)
    return np.asarray(im.convert("L"))


def quant_of(data):
    at = data.index(b"\xff\xdb")
    zz = np.frombuffer(data[at + 5: at + 69], np.uint8).astype(np.uint16)
    q = np.zeros(64, np.uint16)
    q[P.ZIGZAG] = zz
    return q


def grid_of(record, pitch, rows):
    return record[128:128 + rows * pitch * 128].view(np.int16).reshape(rows, pitch, 64)


@pytest.mark.parametrize("group", list(P.GROUPS))
def test_hand_built_files_decode_to_the_grid_they_encode(group):
    from mono_dataset_code_amd import capi

    w, h, _ = P.GROUPS[group]
    rec_bytes, pitch, rows = capi.jpeg_record_bytes(w, h)
    cap = P.stream_cap(group)
    counts = collections.Counter()
    for c in P.by_group()[group]:
        assert (c.w, c.h) == (w, h)
        counts[c.expect] += 1
        rec = np.full(rec_bytes, 0x5A, np.uint8)
        stream = np.zeros(cap, np.uint8)
        if c.expect == "damaged":
            with pytest.raises(ValueError):
                capi.decode_jpeg_record(c.data, rec, pitch)
            with pytest.raises(ValueError):
                capi.decode_gray8(c.data)
            capi.jpeg_stream(c.data, stream)  # the stream builds: the kernels report such a frame
            continue
        assert capi.decode_jpeg_record(c.data, rec, pitch)[:3] == (w, h, pitch), c.name
        gr, gc = c.grid.shape[:2]
        assert gr <= rows and gc <= pitch and gr >= (h + 7) // 8 and gc >= (w + 7) // 8
        assert np.array_equal(rec[:128].view(np.uint16), quant_of(c.data)), c.name
        g = grid_of(rec, pitch, rows)[:gr, :gc]
        assert np.array_equal(g, c.grid), (c.name, "host record", np.argwhere((g != c.grid).any(-1))[:4].tolist())
        pixels = capi.decode_gray8(c.data)
        assert pixels.shape == (h, w)
        if c.pil:
            assert np.array_equal(pixels, pil_gray(c.data)), (c.name, "pixels against Pillow")
        else:  # no libjpeg to compare with: the pixels are the inverse DCT of the record (what the device makes of it)
            assert np.array_equal(pixels, islow_idct_reference(rec, w, h, pitch, rows)), (c.name, "pixels against the record's inverse DCT")
        if c.expect == "stream_refused":
            with pytest.raises(ValueError, match="too many long Huffman codes"):
                capi.jpeg_stream(c.data, stream)
            continue
        used, sw, sh = capi.jpeg_stream(c.data, stream)
        assert (sw, sh) == (w, h) and used <= cap
        got = sequential_decode(stream, pitch, rows)
        assert np.array_equal(got[:128], rec[:128]), c.name
        g = grid_of(got, pitch, rows)[:gr, :gc]
        assert np.array_equal(g, c.grid), (c.name, "device tables", np.argwhere((g != c.grid).any(-1))[:4].tolist())
    print("%s: %s" % (group, dict(counts)))


def test_pillow_is_set_aside_for_exactly_two_named_sets():
    """pil is False for the cases with more than 10 blocks per MCU and for those with AC sizes above 10, and for nothing else."""
    off = sorted(c.name for c in P.cases() if not c.pil)
    print("no Pillow reference:", off)
    many_blocks = sorted("luma%dx%d_dri%d_pad%d" % (hy, vy, dri, pad) for hy in range(1, 5) for vy in range(1, 5) if hy * vy + 2 > 10
                         for dri, pad in ((0, 1), (2, 0), ((50 + 8 * hy - 1) // (8 * hy), 1)))
    big_ac = ["ac_sizes_11_15", "dc_category_11_wraps_ac_size_11"]
    assert off == sorted(many_blocks + big_ac)
    for c in P.cases():
        if c.name in many_blocks:
            with pytest.raises(Exception):
                pil_gray(c.data)  # libjpeg refuses the file: JPEG allows ten blocks per MCU
        if c.grid is not None and c.name not in many_blocks:  # AC sizes above 10 = a luma AC coefficient outside +-1023
            ac = np.abs(c.grid.reshape(-1, 64)[:, 1:].astype(np.int32)).max()
            assert (ac > 1023) == (c.name in big_ac), c.name


def test_stream_properties_the_cases_were_built_for():
    """Read back from the built streams: the subtable counts of the prefix cases, the lengths at which the subsequence length
    steps, the average interval bits at which the number of parts per interval steps."""
    from mono_dataset_code_amd import capi

    by_name = {c.name: c for c in P.cases()}

    def header(name):
        c = by_name[name]
        stream = np.zeros(P.stream_cap(c.group), np.uint8)
        capi.jpeg_stream(c.data, stream)
        return parse_header(stream), stream

    assert P.long_prefixes(header("prefixes_32")[1], 1) == 32
    assert P.long_prefixes(header("ac_all_16bit")[1], 1) == 6 and P.long_prefixes(header("ac_all_11bit")[1], 1) == 0
    assert P.long_prefixes(header("every_length_1_16")[1], 1) == 1
    # (33 prefixes: the stream does not build; the prefixes are counted from the table's canonical codes)
    assert len({code >> 1 for code, ln in P.huff_codes(*P.prefix_table(66)).values() if ln == 12}) == 33
    for name, c in by_name.items():
        if c.group in ("len1", "len2", "len4", "lds"):
            want = int(name.rsplit("_", 1)[1])
            hd = header(name)[0]
            assert hd["ecs"] == want, name
            nbits = 8 * want
            if c.group == "len1":
                S = max(256, ((nbits + 1023) // 1024 + 31) & ~31)
                assert S == (288 if want > P.one_workgroup_step_bytes() else 256), name
            else:
                G = {"len2": 2, "len4": 4, "lds": 4}[c.group]
                sw = max(9, (((nbits + 1024 * G - 1) // (1024 * G) + 31) // 32) | 1)
                if c.group == "lds":
                    assert "_sw%d_" % sw in name, (name, sw)
                    lds = (72 if hd["ncomp"] == 3 else 96) * 1024
                    assert ((1024 * sw + 64) * 4 <= lds) == (sw in (17, 23)), name
                else:
                    assert sw == (11 if want > P.split_step_bytes(G) else 9), name
    for lt in range(1, 7):
        for tag in ("gray", "2x1"):
            for side in ("below", "at"):
                hd = header("iv_%s_T%d_%s" % (tag, 1 << lt, side))[0]
                avg = hd["ecs"] * 8 // hd["n_iv"]
                got = 0
                while got < 6 and avg >> (got + 1) >= 384:
                    got += 1
                assert got == (lt if side == "at" else lt - 1) and 0 <= (384 << lt) - avg <= 8 * (side == "below"), (lt, tag, side, avg)
    assert header("many_gray_dri1")[0]["n_iv"] == 1089 and header("iv_gray_dri_above_mcus")[0]["n_iv"] == 1
    assert header("iv_gray_dri5_fill")[0]["n_iv"] == 26 and header("iv_2x1_dri5_fill")[0]["n_iv"] == 13
