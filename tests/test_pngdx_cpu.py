"""The device PNG decoder with the parallel inflate (include/mdc_pngdx.h, libmdc_pngdx.so) as far as it can be checked without a
GPU: the token path (csrc/png_tokens_core.h) runs every problem of tests/pngdx_problems.py, valid and damaged, as a stand-alone
program under AddressSanitizer and UndefinedBehaviorSanitizer, its phases once in ascending and once in descending thread order, and
gives the expected reason, path, end byte and filtered bytes both times; every stream called valid is valid for zlib and every
damaged one is refused by it; header, library and ctypes table declare the same functions; the library links nothing of ours and
leaves the product's build identity and libmdc_pngd.so's kernels untouched; argument errors are statuses; the kernels compile without
scratch."""
import ctypes
import functools
import json
import os
import struct
import subprocess
import sys
import zlib

import pytest

import pngd_restatement as R
import pngdx_problems as X
from test_abi import declared, exported, prototypes, signature_mismatches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def corpus():
    """[(name, w, h, stream, the damaged case's reason or None)] -- valid inputs first"""
    return [(n, w, h, s, None) for n, w, h, s in X.all_valid_cases()] + list(X.damaged_cases())


def test_valid_streams_are_zlibs_and_damaged_ones_are_refused_by_it():
    paths, reasons = set(), set()
    for name, w, h, s, want in corpus():
        reason, path, _ = X.expected(w, h, s)
        if want is None:
            assert R.host_accepts(s, w, h) and reason == R.OK, name  # the cap of zero frames on path 3 rests on this
            raw = zlib.decompress(s)
            assert len(raw) == h * (1 + w) and struct.unpack(">I", s[-4:])[0] == zlib.adler32(raw), name
            paths.add(path)
        else:
            assert not R.host_accepts(s, w, h), name
            assert reason == want != R.OK, (name, R.REASONS[reason], R.REASONS[want])
            assert path in (R.PARALLEL, R.STORED, R.GENERAL), (name, path)  # never TOKENS: that is a written frame's path
            reasons.add(reason)
    assert {R.PARALLEL, R.STORED, X.TOKENS} <= paths and R.GENERAL not in paths
    assert reasons == set(range(1, 11))  # every reason code
    later = [c for c in X.damaged_cases() if c[0].startswith("later_")]
    assert {c[4] for c in later} >= {R.TRUNCATED, R.BLOCK_TYPE, R.STORED_LEN, R.BAD_CODE, R.UNDEFINED_SYMBOL, R.DISTANCE, R.OUTPUT_SIZE}


def test_the_streams_the_issue_names_belong_to_the_token_path():
    """zlib at levels 1 and 6, memLevel 1, Z_RLE, Z_FIXED, Z_HUFFMAN_ONLY, a flush in the middle, a constant image: valid, and not
    the front kernel's"""
    cases = {n: (w, h, s) for n, w, h, s in X.small_valid_cases()}
    for kind in ("level1", "level6", "mem1", "rle", "fixed", "huffman_mem1", "sync_flush", "full_flush", "partial_flush"):
        for image in ("smooth", "constant"):
            w, h, s = cases["zlib_64x64_%s_%s" % (image, kind)]
            assert X.expected(w, h, s)[:2] == (R.OK, X.TOKENS), (image, kind)
    blocks = [n for n, w, h, s in X.small_valid_cases() if n.startswith("zlib_64x64_smooth_mem1")]
    assert blocks  # dozens of blocks: see pngdx_problems._damaged_later, which cuts the same stream in a late block
    for n, w, h, s in X.hand_cases() + X.lz_cases():
        reason, path, _ = X.expected(w, h, s)
        assert reason == R.OK and path in (X.TOKENS, R.PARALLEL), (n, R.REASONS[reason], path)


def test_token_core_under_sanitizers_in_both_thread_orders(tmp_path):
    """csrc/png_tokens_core.h in a program of its own, with its own main: nothing is loaded into python"""
    from mono_dataset_code_amd import build

    exe = build.build_pngdx_core_program(str(tmp_path / "pngdx_core"))
    items = corpus()
    with open(tmp_path / "corpus.bin", "wb") as f:
        f.write(struct.pack("<i", len(items)))
        for _, w, h, s, _ in items:
            f.write(struct.pack("<iii", w, h, len(s)) + s)
    r = subprocess.run([exe, str(tmp_path / "corpus.bin"), str(tmp_path / "results.txt")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout == "", r.stdout[-3000:]  # a sanitizer report is output and a non-zero exit
    lines = [tuple(int(v) for v in line.split()) for line in open(tmp_path / "results.txt")]
    assert [(k, o) for k, o, _, _, _, _ in lines] == [(k, o) for k in range(len(items)) for o in (0, 1)]
    for up, down in zip(lines[0::2], lines[1::2]):
        name, w, h, s, _ = items[up[0]]
        assert up[2:] == down[2:], (name, up, down)  # the thread order is nothing the result depends on
        reason, path, _ = X.expected(w, h, s)
        assert up[2:4] == (reason, path), (name, R.REASONS[up[2]], up[3], R.REASONS[reason], path)
        if reason == R.OK:
            assert up[4] == len(s) - 4 and up[5] == X.filtered_hash(zlib.decompress(s)), name
        elif reason in (R.ADLER, R.FILTER_TYPE):
            assert up[5] == X.filtered_hash(zlib.decompressobj(-15).decompress(s[2:])), name  # inflated, then refused
    assert sum(1 for l in lines if l[3] == X.TOKENS) > 400


# ------------------------------------------------------------------------------------------------ header, library, table


def test_header_parses_as_c99_and_cxx(tmp_path):
    src = tmp_path / "pngdx_abi.c"
    src.write_text('#include "mdc_pngdx.h"\n#include "mdc_pngd.h"\nint main(void){ mdcx_decoder* d = 0; float ms[5]; (void)d; (void)ms;'
                   ' return MDCX_OK + (mdcx_scratch_bytes(1, 1, 1) < 0) + MDCX_STATUS_PATH(MDCX_PATH_TOKENS << 16 | MDCX_ST_ADLER) + MDCX_MAX_STORED_BLOCKS; }\n')
    inc = os.path.join(ROOT, "include")
    for cmd in (["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I" + inc, str(src)],
                ["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", "-I" + inc, str(src)]):
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout


def test_header_library_and_table_are_one_set_and_mirror_mdc_pngd():
    from mono_dataset_code_amd import build, capi

    names = declared("mdc_pngdx.h", "mdcx_")
    assert len(names) == 10 and names == [n.replace("mdci_", "mdcx_") for n in declared("mdc_pngd.h", "mdci_")]
    assert exported(build.LIB_PNGDX) == names == sorted(capi.PNGDX_API)
    protos = prototypes("mdc_pngdx.h", "mdcx_")
    assert sorted(protos) == names
    assert signature_mismatches(capi.PNGDX_API, protos) == []
    # function for function and argument for argument: the text of every prototype, the decoder's name and the five times aside
    theirs = prototypes("mdc_pngd.h", "mdci_")
    for name, (ret, params) in protos.items():
        ret_i, params_i = theirs[name.replace("mdcx_", "mdci_")]
        same = [p.replace("mdci_decoder", "mdcx_decoder").replace("ms[4]", "ms[5]") for p in params_i]
        assert (ret, list(params)) == (ret_i.replace("mdci_decoder", "mdcx_decoder"), same), name
    L = capi.pngdx_lib()
    assert sorted(vars(L)) == names
    hdr = open(os.path.join(ROOT, "include", "mdc_pngdx.h")).read()
    for i, n in enumerate(R.REASONS):
        assert "#define MDCX_ST_%s %d\n" % (n.upper(), i) in hdr
    for n, v in (("PARALLEL", R.PARALLEL), ("STORED", R.STORED), ("GENERAL", R.GENERAL), ("TOKENS", X.TOKENS)):
        assert "#define MDCX_PATH_%s %d\n" % (n, v) in hdr
    assert {k: v for k, v in capi.PNGDX_PATHS.items() if k != X.TOKENS} == capi.PNGD_PATHS and capi.PNGDX_PATHS[X.TOKENS] == "tokens"


def test_library_links_nothing_of_ours_and_nothing_links_it():
    from mono_dataset_code_amd import build

    for lib in (build.LIB_HIP, build.LIB_HOST, build.LIB_MULTI, build.LIB_BENCH, build.LIB_JENC, build.LIB_ZIPW, build.LIB_PNGW, build.LIB_PNGLZ, build.LIB_PNGD):
        assert "mdcx_" not in subprocess.run(["nm", "-D", lib], stdout=subprocess.PIPE, text=True, check=True).stdout, lib
        assert "libmdc_pngdx" not in subprocess.run(["readelf", "-d", lib], stdout=subprocess.PIPE, text=True, check=True).stdout, lib
    needed = subprocess.run(["readelf", "-d", build.LIB_PNGDX], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert not any("libmdc_" in line for line in needed.splitlines() if "NEEDED" in line), needed
    undefined = subprocess.run(["nm", "-D", "--undefined-only", build.LIB_PNGDX], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert [w for w in undefined.split() if w.startswith("mdc")] == []


def test_product_build_identity_is_unchanged():
    from mono_dataset_code_amd import build

    assert build.code_id() == json.load(open(os.path.join(ROOT, "profiles", "r06_fused_summary.json")))["code_id"]
    deps = set(build.HIP_DEPS)
    for f in (build.PNGDX_SOURCE, build.PNGDX_CORE, build.PNG_DECODE_KERNELS, build.PNGDX_EXPORT_MAP, os.path.join(ROOT, "include", "mdc_pngdx.h")):
        assert os.path.exists(f) and f not in deps, f


def _err(L):
    return L.mdcx_last_error().decode()


def test_scratch_bytes_is_the_formula_and_covers_the_source_indices():
    from mono_dataset_code_amd import capi

    L, Li = capi.pngdx_lib(), capi.pngd_lib()
    for w, h, n in ((1, 1, 1), (640, 480, 7), (1280, 1024, 128), (3, 5, 2)):
        F = h * (1 + w)
        assert L.mdcx_scratch_bytes(w, h, n) == n * (5 * ((F + 15) // 16 * 16) + 16)  # a byte and a 32-bit index per filtered byte
        assert L.mdcx_scratch_bytes(w, h, n) == Li.mdci_scratch_bytes(w, h, n) + n * 4 * ((F + 15) // 16 * 16)
    assert L.mdcx_scratch_bytes(0, 1, 1) == -1 and L.mdcx_scratch_bytes(1, 0, 1) == -1 and L.mdcx_scratch_bytes(1, 1, 0) == -1
    assert L.mdcx_scratch_bytes(16383, 16384, 1) > 0 and L.mdcx_scratch_bytes(16384, 16384, 1) == -1  # F <= 2^28
    assert L.mdcx_scratch_bytes(16383, 16384, 819) > 0 and L.mdcx_scratch_bytes(16383, 16384, 820) == -1  # 2^40, the indices included


def test_argument_errors_without_a_device():
    """every check below comes before any HIP call: a status and a message, never a fault"""
    from mono_dataset_code_amd import capi

    L = capi.pngdx_lib()
    h = ctypes.c_void_p()
    assert L.mdcx_create(0, 4, 4, 1, None) == -1 and "null" in _err(L)
    assert L.mdcx_create(0, 4, 4, 0, ctypes.byref(h)) == -1 and "max_images" in _err(L) and not h.value
    assert L.mdcx_create(0, 0, 4, 1, ctypes.byref(h)) == -3 and "start at 1" in _err(L)
    assert L.mdcx_create(0, 4, -1, 1, ctypes.byref(h)) == -3
    assert L.mdcx_create(0, 16384, 16384, 1, ctypes.byref(h)) == -3 and "2^28" in _err(L)
    assert L.mdcx_create(0, 16383, 16384, 820, ctypes.byref(h)) == -3 and "2^40" in _err(L) and not h.value
    p = ctypes.c_void_p(4096)  # never dereferenced on the host
    assert L.mdcx_decode_device(None, p, 100, p, 0, 0, 1, p, 16, p, None) == -1 and "null" in _err(L)
    assert L.mdcx_decode_host(None, None, None, 1, None, None) == -1 and "null" in _err(L)
    L.mdcx_destroy(None)
    with pytest.raises(ValueError):
        capi.PngDecoder(4, 4, matches="sometimes")


def test_kernels_have_no_scratch_and_share_libmdc_pngds():
    """the token kernel has 1024 threads: 128 VGPRs is the most it may have.  The four shared kernels are libmdc_pngd.so's: the same
    names, registers and LDS in both libraries."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_stats

    ks = {k["pretty"]: k for k in isa_stats.kernels(isa_stats.device_asm("mdc_pngdx.hip"))}
    assert sorted(ks) == ["pngd_check_kernel", "pngd_front_kernel", "pngd_general_kernel", "pngd_unfilter_kernel", "pngdx_settle_kernel", "pngdx_tokens_kernel"]
    for k in ks.values():
        assert k["scratch"] == 0, (k["pretty"], k["scratch"])
        assert not any(n.startswith("v_mfma") for n in k["counts"]), k["pretty"]
    assert ks["pngdx_tokens_kernel"]["vgpr"] <= 128 and ks["pngdx_tokens_kernel"]["lds"] <= 32 * 1024
    theirs = {k["pretty"]: k for k in isa_stats.kernels(isa_stats.device_asm("mdc_pngd.hip"))}
    for name, k in theirs.items():
        assert (ks[name]["vgpr"], ks[name]["lds"], ks[name]["counts"]) == (k["vgpr"], k["lds"], k["counts"]), name
