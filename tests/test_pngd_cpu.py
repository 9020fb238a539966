"""The device PNG decoder (include/mdc_pngd.h, libmdc_pngd.so) as far as it can be checked without a GPU: the restatement
(tests/pngd_restatement.py) is pinned by zlib and PIL on every input the GPU tests use; the core the kernels are made of
(csrc/png_inflate_core.h) runs the same inputs, valid and damaged, as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer and gives the restatement's pixels, reasons and paths; header, library and ctypes table declare the same
functions; the library links nothing of ours and leaves the product's build identity untouched; argument errors are statuses; the
kernels compile without scratch."""
import ctypes
import functools
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import pngd_restatement as R
from test_abi import declared, exported, prototypes, signature_mismatches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def corpus():
    """[(name, w, h, stream, expected reason or None)] -- valid inputs first"""
    return [(n, w, h, s, None) for n, w, h, s in R.all_valid_cases()] + R.damaged_cases()


@functools.lru_cache(maxsize=None)
def restated():
    return [R.decode(s, w, h) for _, w, h, s, _ in corpus()]


def test_restatement_equals_zlib_and_pil_on_every_valid_input():
    import zlib

    seen = set()
    for (name, w, h, s, _), (reason, path, px) in zip(corpus(), restated()):
        if _ is not None:
            continue
        F = h * (1 + w)
        assert R.host_accepts(s, w, h), name  # valid for zlib: the GPU test's cap of zero refused frames rests on this
        assert reason == R.OK, (name, R.REASONS[reason])
        raw, end = R.inflate(s, F)
        assert raw == zlib.decompress(s) and end == len(s) - 4, name
        assert np.array_equal(px, R.pil_pixels(w, h, s)), name
        family = name.split("_")[0]
        want = {"parallel": R.PARALLEL, "stored": R.STORED, "general": R.GENERAL}.get(family)
        if name == "general_empty_stored_in_the_middle":
            want = R.STORED  # a chain of stored blocks, one of them empty
        if want is not None:
            assert path == want, (name, path)
        seen.add(path)
    assert seen == {R.PARALLEL, R.STORED, R.GENERAL}


def test_unfilter_cases_cover_every_type_at_every_size():
    for w, h in R.UNFILTER_SIZES:
        types = set()
        for name, s in R.unfilter_cases(w, h):
            raw, _ = R.inflate(s, h * (1 + w))
            types |= set(raw[::1 + w])
        assert types == {0, 1, 2, 3, 4}, (w, h)


def test_damaged_inputs_are_refused_by_the_restatement_and_by_zlib():
    reasons = set()
    for (name, w, h, s, want), (reason, path, px) in zip(corpus(), restated()):
        if want is None:
            continue
        assert not R.host_accepts(s, w, h), name
        assert reason == want != R.OK and px is None, (name, R.REASONS[reason], R.REASONS[want])
        reasons.add(reason)
    assert reasons == set(range(1, 11))  # every reason code


def test_shared_core_under_sanitizers_equals_the_restatement(tmp_path):
    """csrc/png_inflate_core.h in a program of its own, with its own main: nothing is loaded into python"""
    from mono_dataset_code_amd import build

    exe = build.build_pngd_core_program(str(tmp_path / "pngd_core"))
    items = corpus()
    with open(tmp_path / "corpus.bin", "wb") as f:
        f.write(struct.pack("<i", len(items)))
        for _, w, h, s, _ in items:
            f.write(struct.pack("<iii", w, h, len(s)) + s)
    r = subprocess.run([exe, str(tmp_path / "corpus.bin"), str(tmp_path / "results.bin")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout == "", r.stdout[-3000:]  # a sanitizer report is output and a non-zero exit
    got = open(tmp_path / "results.bin", "rb").read()
    at = 0
    for (name, w, h, s, _), (reason, path, px) in zip(items, restated()):
        st, pa = struct.unpack_from("<ii", got, at)
        at += 8
        assert (st, pa) == (reason, path), (name, R.REASONS[st], pa, R.REASONS[reason], path)
        if st == 0:
            assert got[at:at + w * h] == px.tobytes(), name
            at += w * h
    assert at == len(got)


def test_png_stream_equals_the_restated_chunk_walk():
    """mdch_png_stream: one IDAT, IDAT split into chunks of 1, 7 and 8192 bytes, ancillary chunks between; other flavours refused"""
    import io

    from PIL import Image

    from mono_dataset_code_amd import capi

    img = R.test_image(130, 77, 5)
    b = io.BytesIO()
    Image.fromarray(img).save(b, "PNG")
    w, h, stream = R.png_stream(b.getvalue())
    assert (w, h) == (130, 77) and capi.png_stream(b.getvalue()) == (w, h, stream)
    extra = [(b"tEXt", b"Comment\x00between"), (b"tIME", bytes(7)), (b"zzZz", b"")]
    for split in (None, 1, 7, 8192):
        for ex in ((), extra):
            f = R.png_file(w, h, stream, split=split, extra=ex)
            assert R.png_stream(f) == (w, h, stream) and capi.png_stream(f) == (w, h, stream), (split, len(ex))
            if not ex:  # (chunks between IDAT chunks are against the specification: the reader's walk takes them, PIL stops there)
                assert np.array_equal(np.array(Image.open(io.BytesIO(f))), img)
    f = R.png_file(w, h, stream, split=7, extra=extra)
    assert capi.png_stream(f, cap=len(stream))[2] == stream
    with pytest.raises(ValueError):
        capi.png_stream(f, cap=len(stream) - 1)  # does not fit: the caller decodes to pixels
    own = P_encode(img)
    assert capi.png_stream(own)[2] == own[41:-16] == R.png_stream(own)[2]  # skip_head 41, skip_tail 16
    refused = {"16-bit": Image.fromarray(img.astype(np.uint16) * 257), "palette": Image.fromarray(img).convert("P"), "rgb": Image.fromarray(img).convert("RGB"),
               "gray+alpha": Image.fromarray(img).convert("LA")}
    for name, im in refused.items():
        b = io.BytesIO()
        im.save(b, "PNG")
        assert R.png_stream(b.getvalue()) is None, name
        with pytest.raises(ValueError):
            capi.png_stream(b.getvalue())
    one = R.png_file(w, h, stream)
    for bad in (R.png_file(w, h, stream, interlace=1), one[:len(one) // 2], b"", b"\x89PNG\r\n\x1a\n", b"\xff\xd8\xff\xd9", f[:8] + f[33:]):
        assert R.png_stream(bad) is None
        with pytest.raises(ValueError):
            capi.png_stream(bad)


def P_encode(img):
    import pngw_restatement as P

    return P.encode(img, 8, P.ADAPTIVE)[0]


# ------------------------------------------------------------------------------------------------ header, library, table


def test_header_parses_as_c99_and_cxx(tmp_path):
    src = tmp_path / "pngd_abi.c"
    src.write_text('#include "mdc_pngd.h"\nint main(void){ mdci_decoder* d = 0; (void)d;'
                   ' return MDCI_OK + (mdci_scratch_bytes(1, 1, 1) < 0) + MDCI_STATUS_PATH(MDCI_PATH_GENERAL << 16 | MDCI_ST_ADLER) + MDCI_MAX_STORED_BLOCKS; }\n')
    inc = os.path.join(ROOT, "include")
    for cmd in (["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I" + inc, str(src)],
                ["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", "-I" + inc, str(src)]):
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout


def test_header_library_and_table_are_one_set():
    from mono_dataset_code_amd import build, capi

    names = declared("mdc_pngd.h", "mdci_")
    assert len(names) == 10 and {"mdci_decode_device", "mdci_decode_host", "mdci_scratch_bytes"} <= set(names)
    assert exported(build.LIB_PNGD) == names == sorted(capi.PNGD_API)
    protos = prototypes("mdc_pngd.h", "mdci_")
    assert sorted(protos) == names
    assert signature_mismatches(capi.PNGD_API, protos) == []
    L = capi.pngd_lib()
    assert sorted(vars(L)) == names
    hdr = open(os.path.join(ROOT, "include", "mdc_pngd.h")).read()
    for i, n in enumerate(R.REASONS):
        assert "#define MDCI_ST_%s %d\n" % (n.upper(), i) in hdr
    for n, v in (("PARALLEL", R.PARALLEL), ("STORED", R.STORED), ("GENERAL", R.GENERAL)):
        assert "#define MDCI_PATH_%s %d\n" % (n, v) in hdr
    assert "#define MDCI_MAX_STORED_BLOCKS %d\n" % R.MAX_STORED_BLOCKS in hdr


def test_library_links_nothing_of_ours_and_nothing_links_it():
    from mono_dataset_code_amd import build

    for lib in (build.LIB_HIP, build.LIB_HOST, build.LIB_MULTI, build.LIB_BENCH, build.LIB_JENC, build.LIB_ZIPW, build.LIB_PNGW):
        assert "mdci_" not in subprocess.run(["nm", "-D", lib], stdout=subprocess.PIPE, text=True, check=True).stdout, lib
        assert "libmdc_pngd" not in subprocess.run(["readelf", "-d", lib], stdout=subprocess.PIPE, text=True, check=True).stdout, lib
    needed = subprocess.run(["readelf", "-d", build.LIB_PNGD], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert not any("libmdc_" in line for line in needed.splitlines() if "NEEDED" in line), needed
    undefined = subprocess.run(["nm", "-D", "--undefined-only", build.LIB_PNGD], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert [w for w in undefined.split() if w.startswith("mdc")] == []


def test_product_build_identity_is_unchanged():
    from mono_dataset_code_amd import build

    assert build.code_id() == json.load(open(os.path.join(ROOT, "profiles", "r06_fused_summary.json")))["code_id"]
    deps = set(build.HIP_DEPS)
    for f in (build.PNGD_SOURCE, build.PNGD_CORE, build.PNGD_EXPORT_MAP, os.path.join(ROOT, "include", "mdc_pngd.h")):
        assert os.path.exists(f) and f not in deps, f


def _err(L):
    return L.mdci_last_error().decode()


def test_scratch_bytes_is_the_formula():
    from mono_dataset_code_amd import capi

    L = capi.pngd_lib()
    for w, h, n in ((1, 1, 1), (640, 480, 7), (1280, 1024, 128), (3, 5, 2)):
        F = h * (1 + w)
        assert L.mdci_scratch_bytes(w, h, n) == n * ((F + 15) // 16 * 16 + 16)
    assert L.mdci_scratch_bytes(0, 1, 1) == -1 and L.mdci_scratch_bytes(1, 0, 1) == -1 and L.mdci_scratch_bytes(1, 1, 0) == -1
    assert L.mdci_scratch_bytes(16383, 16384, 1) > 0 and L.mdci_scratch_bytes(16384, 16384, 1) == -1  # F <= 2^28
    assert L.mdci_scratch_bytes(16383, 16384, 5000) == -1  # 2^40


def test_argument_errors_without_a_device():
    """every check below comes before any HIP call: a status and a message, never a fault"""
    from mono_dataset_code_amd import capi

    L = capi.pngd_lib()
    h = ctypes.c_void_p()
    assert L.mdci_create(0, 4, 4, 1, None) == -1 and "null" in _err(L)
    assert L.mdci_create(0, 4, 4, 0, ctypes.byref(h)) == -1 and "max_images" in _err(L) and not h.value
    assert L.mdci_create(0, 0, 4, 1, ctypes.byref(h)) == -3 and "start at 1" in _err(L)
    assert L.mdci_create(0, 4, -1, 1, ctypes.byref(h)) == -3
    assert L.mdci_create(0, 16384, 16384, 1, ctypes.byref(h)) == -3 and "2^28" in _err(L)
    assert L.mdci_create(0, 16383, 16384, 5000, ctypes.byref(h)) == -3 and "2^40" in _err(L) and not h.value
    p = ctypes.c_void_p(4096)  # never dereferenced on the host
    assert L.mdci_decode_device(None, p, 100, p, 0, 0, 1, p, 16, p, None) == -1 and "null" in _err(L)
    assert L.mdci_decode_host(None, None, None, 1, None, None) == -1 and "null" in _err(L)
    L.mdci_destroy(None)


def test_kernels_have_no_scratch_and_no_mfma():
    """the budget reached: 100 VGPRs for the front kernel (1024 threads: 128 is the most it may have), 90 for the wave-per-image
    inflate, 40 for the two others"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_stats

    ks = isa_stats.kernels(isa_stats.device_asm("mdc_pngd.hip"))
    assert sorted(k["pretty"] for k in ks) == ["pngd_check_kernel", "pngd_front_kernel", "pngd_general_kernel", "pngd_unfilter_kernel"]
    budget = {"pngd_front_kernel": 104, "pngd_general_kernel": 92, "pngd_check_kernel": 40, "pngd_unfilter_kernel": 40}
    for k in ks:
        assert k["scratch"] == 0, (k["pretty"], k["scratch"])
        assert not any(n.startswith("v_mfma") for n in k["counts"]), k["pretty"]
        assert k["vgpr"] <= budget[k["pretty"]], (k["pretty"], k["vgpr"])
