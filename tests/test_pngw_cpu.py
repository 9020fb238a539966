"""The device PNG encoder (include/mdc_pngw.h, libmdc_pngw.so) as far as it can be checked without a GPU: the restatement
(tests/pngw_restatement.py) is pinned by zlib and PIL; header, library and ctypes table declare the same functions; the library
links libmdc_zipw.so and nothing else of ours, and leaves the product's build identity untouched; argument errors are statuses;
mdcp_png_bound is the formula; the kernels compile without scratch; the code builder's rule on directed histograms."""
import ctypes
import io
import json
import math
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import pngw_restatement as P
from test_abi import declared, exported, prototypes, signature_mismatches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILTERS = (0, 1, 2, 3, 4, P.ADAPTIVE)


def images(depth, seed=3):
    """small images of every shape class: one pixel, one row, one column, odd sizes, and a 64 x 48; noise, a ramp and a constant"""
    rng = np.random.default_rng(seed)
    top = (1 << depth) - 1
    dt = np.uint8 if depth == 8 else np.uint16
    out = []
    for h, w in ((1, 1), (1, 3), (5, 1), (2, 17), (5, 3), (48, 64)):
        yy, xx = np.mgrid[0:h, 0:w]
        out.append(rng.integers(0, top + 1, (h, w)).astype(dt))
        out.append(((xx * 3 + yy * 5) * (top // 255) + (xx * yy) % 7).astype(dt))
        out.append(np.full((h, w), top // 3, dt))
    return out


@pytest.mark.parametrize("depth", [8, 16])
@pytest.mark.parametrize("filt", FILTERS)
def test_restatement_is_read_by_zlib_and_pil(depth, filt):
    from PIL import Image

    for img in images(depth):
        h, w = img.shape
        png, stored = P.encode(img, depth, filt)
        assert len(png) <= P.png_bound(w, h, depth)
        idat = P.idat_of(png)  # the chunk sequence and every CRC, by the restated crc32
        assert idat[:2] == b"\x78\x01"
        data = zlib.decompress(idat)  # header, DEFLATE stream and Adler-32, by zlib
        want = P.filtered(img, depth, filt).tobytes()
        assert data == want
        assert (idat[2] & 6) == (0 if stored else 4)  # BTYPE of the first block
        assert np.array_equal(P.unfilter(data, w, h, depth), img)
        got = np.array(Image.open(io.BytesIO(png)))
        assert got.shape == img.shape and np.array_equal(got.astype(np.uint16), img.astype(np.uint16)), (img.shape, filt)
        if filt != P.ADAPTIVE:
            assert set(np.frombuffer(data, np.uint8).reshape(h, -1)[:, 0]) == {filt}


def test_restated_checksums_equal_zlibs():
    rng = np.random.default_rng(4)
    for n in (0, 1, 2, 5552, 5553, 70000):
        d = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert P.crc32(d) == zlib.crc32(d) and P.adler32(d) == zlib.adler32(d), n
    assert P.adler32(b"\xff" * 70000) == zlib.adler32(b"\xff" * 70000)


def test_adaptive_choice_is_the_smallest_signed_sum_lowest_type_on_ties():
    flat = np.full((3, 8), 77, np.uint8)  # row 0: sub leaves one byte (77), up leaves eight; rows 1, 2: up leaves none -- and sub, paeth tie above it
    rows = P.filtered(flat, 8, P.ADAPTIVE)
    assert rows[:, 0].tolist() == [1, 2, 2]
    assert P.filtered(np.zeros((2, 4), np.uint8), 8, P.ADAPTIVE)[:, 0].tolist() == [0, 0]  # every type gives zeros: type 0


def test_f32_conversion_is_convert_to_8u():
    v = np.array([np.nan, np.inf, -np.inf, -0.4, 0.5, 1.5, 2.5, 254.5, 255.5, 1e10, -1e10, 127.49], np.float32)
    assert P.f32_to_u8(v).tolist() == [0, 255, 0, 0, 0, 2, 2, 254, 255, 255, 0, 127]


# ------------------------------------------------------------------------------------------------ the code builder's rule


def unlimited_depths(hist):
    import heapq

    heap = [(c, i, [i]) for i, c in enumerate(hist) if c]
    depth = {i: 0 for _, i, _ in heap}
    heapq.heapify(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for s in a[2] + b[2]:
            depth[s] += 1
        heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
    return depth


@pytest.mark.parametrize("name,hist,limit", P.directed_histograms(), ids=[c[0] for c in P.directed_histograms()])
def test_code_lengths_respect_the_limit_and_are_complete(name, hist, limit):
    lengths = P.huffman_lengths(hist, limit)
    used = [s for s, c in enumerate(hist) if c]
    assert all((lengths[s] > 0) == (hist[s] > 0) for s in range(len(hist)))
    assert max(lengths) <= limit
    kraft = sum(2 ** (limit - lengths[s]) for s in used)
    if len(used) >= 2:
        assert kraft == 2 ** limit  # complete
    else:
        assert [lengths[s] for s in used] == [1] * len(used)
    flat = max(1, math.ceil(math.log2(len(used)))) if used else 0
    assert flat <= limit
    cost = sum(hist[s] * lengths[s] for s in used)
    assert cost <= sum(hist[s] for s in used) * flat, (cost, flat)
    if name.startswith("fibonacci"):  # the limit is active: Huffman's own tree is deeper
        assert max(unlimited_depths(hist).values()) > limit and max(lengths) == limit
    codes = P.canonical_codes(lengths)  # prefix-free: no code is the start of another
    words = sorted(format(codes[s], "0%db" % lengths[s]) for s in used)
    assert all(not b.startswith(a) for a, b in zip(words, words[1:]))


def test_run_length_code_covers_every_branch():
    seq = [0] * 139 + [5] * 8 + [0] * 2 + [7] + [0] * 10 + [3] * 4 + [0] * 3
    pairs = P.run_length_code(seq)
    assert pairs == [(18, 127), (0, 0), (5, 0), (16, 3), (5, 0), (0, 0), (0, 0), (7, 0), (17, 7), (3, 0), (16, 0), (17, 0)]
    back = []
    for s, e in pairs:
        back += [back[-1]] * (e + 3) if s == 16 else [0] * (e + 3) if s == 17 else [0] * (e + 11) if s == 18 else [s]
    assert back == seq


def test_stored_fallback_is_taken_only_when_not_strictly_shorter():
    every = np.tile(np.arange(256, dtype=np.uint8), 4).tobytes()  # every value equally often: 8 bits per byte plus a header
    stream, stored = P.deflate(every)
    assert stored and len(stream) == P.stored_size(len(every)) and zlib.decompress(stream, -15) == every
    stream, stored = P.deflate(bytes(1000))
    assert not stored and len(stream) < 200 and zlib.decompress(stream, -15) == bytes(1000)
    big = bytes(range(256)) * 512  # 131072 bytes: three stored blocks, the last of 2
    blocks = P.stored_blocks(big)
    assert len(blocks) == len(big) + 15 and blocks[0] == 0 and blocks[2 * 65540] == 1 and zlib.decompress(blocks, -15) == big


# ------------------------------------------------------------------------------------------------ header, library, table


def test_header_parses_as_c99_and_cxx(tmp_path):
    src = tmp_path / "pngw_abi.c"
    src.write_text('#include "mdc_pngw.h"\nint main(void){ mdcp_encoder* e = 0; (void)e;'
                   ' return MDCP_OK + (mdcp_png_bound(1, 1, 8) < 0) + MDCP_FILTER_ADAPTIVE + MDCP_MAX_SYMBOLS; }\n')
    inc = os.path.join(ROOT, "include")
    for cmd in (["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I" + inc, str(src)],
                ["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", "-I" + inc, str(src)]):
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout


def test_header_library_and_table_are_one_set():
    from mono_dataset_code_amd import build, capi

    names = declared("mdc_pngw.h", "mdcp_")
    assert len(names) == 9 and {"mdcp_encode_u16_device", "mdcp_huffman_lengths_device", "mdcp_png_bound"} <= set(names)
    assert exported(build.LIB_PNGW) == names == sorted(capi.PNGW_API)
    protos = prototypes("mdc_pngw.h", "mdcp_")
    assert sorted(protos) == names
    assert signature_mismatches(capi.PNGW_API, protos) == []
    # the check can fail
    wrong = dict(capi.PNGW_API, mdcp_png_bound=(ctypes.c_int64, [ctypes.c_int, ctypes.c_int64, ctypes.c_int]))
    assert len(signature_mismatches(wrong, protos)) == 1
    L = capi.pngw_lib()
    assert sorted(vars(L)) == names
    for n, (restype, argtypes) in capi.PNGW_API.items():
        assert getattr(L, n).restype is restype and list(getattr(L, n).argtypes) == argtypes, n
    hdr = open(os.path.join(ROOT, "include", "mdc_pngw.h")).read()
    assert "#define MDCP_FILTER_ADAPTIVE %d\n" % capi.PNG_FILTER_ADAPTIVE in hdr and capi.PNG_FILTER_ADAPTIVE == P.ADAPTIVE


def test_library_links_the_zip_writer_and_nothing_links_it():
    from mono_dataset_code_amd import build

    for lib in (build.LIB_HIP, build.LIB_HOST, build.LIB_MULTI, build.LIB_BENCH, build.LIB_JENC, build.LIB_ZIPW):
        assert "mdcp_" not in subprocess.run(["nm", "-D", lib], stdout=subprocess.PIPE, text=True, check=True).stdout, lib
        assert "libmdc_pngw" not in subprocess.run(["readelf", "-d", lib], stdout=subprocess.PIPE, text=True, check=True).stdout, lib
    needed = subprocess.run(["readelf", "-d", build.LIB_PNGW], stdout=subprocess.PIPE, text=True, check=True).stdout
    ours = sorted({w.strip("[]") for line in needed.splitlines() if "NEEDED" in line for w in line.split() if "libmdc_" in w})
    assert ours == ["libmdc_zipw.so"], ours
    assert "$ORIGIN" in needed
    undefined = subprocess.run(["nm", "-D", "--undefined-only", build.LIB_PNGW], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert sorted(w for w in undefined.split() if w.startswith("mdc")) == ["mdcz_crc32_device", "mdcz_last_error"]


def test_product_build_identity_is_unchanged():
    from mono_dataset_code_amd import build

    assert build.code_id() == json.load(open(os.path.join(ROOT, "profiles", "r06_fused_summary.json")))["code_id"]
    deps = set(build.HIP_DEPS) | set(build.HOST_DEPS)
    for f in (build.PNGW_SOURCE, build.PNG_BLOCK, build.PNG_ENCODE_CORE, build.PNGW_EXPORT_MAP, os.path.join(ROOT, "include", "mdc_pngw.h")):
        assert os.path.exists(f) and f not in deps, f


def test_program_links_the_encoder_and_names_the_arguments(tmp_path):
    from mono_dataset_code_amd import build

    needed = subprocess.run(["readelf", "-d", build.RECTIFY_DATASET], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "libmdc_pngw.so" in needed
    r = subprocess.run([build.RECTIFY_DATASET, str(tmp_path / "seq")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60, cwd=str(tmp_path))
    assert r.returncode != 0 and r.stdout == "" and len(r.stderr.splitlines()) == 1
    assert "[frames=jpg|png]" in r.stderr and "[vignette=0|1]" in r.stderr
    for bad in ("frames=gif", "vignette=2", "colour=1"):  # refused before anything is opened or created
        r = subprocess.run([build.RECTIFY_DATASET, str(tmp_path / "seq"), str(tmp_path / "out"), bad], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                           timeout=60, cwd=str(tmp_path))
        assert r.returncode != 0 and r.stdout == "" and bad.split("=")[0] in r.stderr, (bad, r.stderr)
    assert os.listdir(str(tmp_path)) == []


def _err(L):
    return L.mdcp_last_error().decode()


def test_bound_is_the_formula_and_the_stored_size():
    from mono_dataset_code_amd import capi

    L = capi.pngw_lib()
    for depth in (8, 16):
        for w in (1, 2, 3, 17, 254, 255, 509, 640, 65535):
            for h in (1, 2, 5, 256, 257, 480):
                F = h * (1 + w * depth // 8)
                want = 57 + 6 + F + 5 * ((F + 65534) // 65535)
                assert L.mdcp_png_bound(w, h, depth) == want == P.png_bound(w, h, depth), (w, h, depth)
                if F <= 200000:  # the restatement's stored file, built
                    assert 57 + 6 + len(P.stored_blocks(bytes(F))) == want
    # a stored file, whole: rows of the values 1..255 and their type byte 0 hold every byte value equally often
    img = P.every_value_image()
    png, stored = P.encode(img, 8, 0)
    assert stored and len(png) == L.mdcp_png_bound(255, 8, 8)
    # outside the limits: -1
    assert L.mdcp_png_bound(0, 1, 8) == -1 and L.mdcp_png_bound(1, 0, 8) == -1 and L.mdcp_png_bound(1, 1, 12) == -1 and L.mdcp_png_bound(-5, 3, 16) == -1
    assert L.mdcp_png_bound(46338, 46338, 8) == 57 + 6 + P.stored_size(46338 * 46339) == 2147420475  # the largest square
    assert L.mdcp_png_bound(46339, 46339, 8) == -1 and L.mdcp_png_bound(2 ** 31 - 1, 2 ** 31 - 1, 16) == -1 and L.mdcp_png_bound(2 ** 31 - 1, 1, 8) == -1


def test_argument_errors_without_a_device():
    """every check below comes before any HIP call: a status and a message, never a fault"""
    from mono_dataset_code_amd import capi

    L = capi.pngw_lib()
    h = ctypes.c_void_p()
    assert L.mdcp_create(0, 4, 4, 8, 0, 1, None) == -1 and "null" in _err(L)
    assert L.mdcp_create(0, 4, 4, 12, 0, 1, ctypes.byref(h)) == -1 and "depth" in _err(L) and not h.value
    assert L.mdcp_create(0, 4, 4, 8, 6, 1, ctypes.byref(h)) == -1 and "filter" in _err(L)
    assert L.mdcp_create(0, 4, 4, 8, -1, 1, ctypes.byref(h)) == -1 and "filter" in _err(L)
    assert L.mdcp_create(0, 4, 4, 8, 0, 0, ctypes.byref(h)) == -1 and "max_images" in _err(L)
    assert L.mdcp_create(0, 0, 4, 8, 0, 1, ctypes.byref(h)) == -3 and "start at 1" in _err(L)
    assert L.mdcp_create(0, 4, -1, 8, 0, 1, ctypes.byref(h)) == -3
    assert L.mdcp_create(0, 46341, 46341, 8, 0, 1, ctypes.byref(h)) == -3 and "2^31" in _err(L)
    assert L.mdcp_create(0, 20000, 20000, 16, 0, 2000, ctypes.byref(h)) == -3 and "2^40" in _err(L) and not h.value
    p = ctypes.c_void_p(4096)  # never dereferenced on the host
    for fn in (L.mdcp_encode_u8_device, L.mdcp_encode_u16_device, L.mdcp_encode_f32_device):
        assert fn(None, p, 16, 1, p, 1 << 20, p, None) == -1 and "null" in _err(L)
    assert L.mdcp_output_device(None, None, None, None) == -1
    L.mdcp_destroy(None)
    assert L.mdcp_huffman_lengths_device(None, 4, 15, p, None) == -1 and "null" in _err(L)
    assert L.mdcp_huffman_lengths_device(p, 4, 15, None, None) == -1
    assert L.mdcp_huffman_lengths_device(p, 0, 15, p, None) == -1 and "nsym" in _err(L)
    assert L.mdcp_huffman_lengths_device(p, 289, 15, p, None) == -1 and "nsym" in _err(L)
    assert L.mdcp_huffman_lengths_device(p, 4, 0, p, None) == -1 and "limit" in _err(L)
    assert L.mdcp_huffman_lengths_device(p, 4, 16, p, None) == -1 and "limit" in _err(L)
    assert L.mdcp_huffman_lengths_device(p, 20, 4, p, None) == -1 and "do not fit" in _err(L)


def test_kernels_have_no_scratch_and_no_mfma():
    """the budget reached: 132 VGPRs for the code builder (one workgroup per image, lane 0 does the serial part), 72 for the others"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_stats

    ks = isa_stats.kernels(isa_stats.device_asm("mdc_pngw.hip"))
    names = sorted(k["pretty"] for k in ks)
    assert names == ["pngw_build_kernel", "pngw_crc_kernel", "pngw_filter_kernel<float, 1>", "pngw_filter_kernel<unsigned char, 1>",
                     "pngw_filter_kernel<unsigned short, 2>", "pngw_finish_kernel", "pngw_lengths_kernel", "pngw_pack_kernel", "pngw_scan_kernel"], names
    for k in ks:
        assert k["scratch"] == 0, (k["pretty"], k["scratch"])
        assert not any(n.startswith("v_mfma") for n in k["counts"]), k["pretty"]
        assert k["vgpr"] <= (132 if k["pretty"] == "pngw_build_kernel" else 72), (k["pretty"], k["vgpr"])
        assert k["lds"] <= 12288, (k["pretty"], k["lds"])
    by = {k["pretty"]: k["counts"] for k in ks}
    # the loads the design asks for: 16 bytes per lane where the filtered bytes are read; integer atomics only
    assert by["pngw_scan_kernel"].get("global_load_dwordx4", 0) >= 1 and by["pngw_pack_kernel"].get("global_load_dwordx4", 0) >= 1
    assert by["pngw_pack_kernel"].get("global_atomic_or", 0) >= 1
    for k in ks:
        assert not any("atomic" in n and ("f32" in n or "f64" in n or "cmpswap" in n) for n in k["counts"]), (k["pretty"], k["counts"])
