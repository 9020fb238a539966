"""The device JPEG encoder with per-frame optimal Huffman tables (include/mdc_jopt.h, libmdc_jopt.so) as far as it can be checked
without a GPU: its specification, restated in tests/jopt_restatement.py, equals libjpeg-turbo's optimize_coding through PIL byte for
byte; the directed problems of tests/jopt_problems.py do what they claim; the table rule the device runs (csrc/jpeg_optimal_table.h)
equals the restatement as a stand-alone program under the sanitizers; header, library and ctypes table declare the same functions;
the kernels compile without scratch and without MFMA; libmdc_jenc.so and the product's build identity are untouched."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import jenc_restatement as R
import jopt_problems as J
import jopt_restatement as O
from test_abi import declared, exported, prototypes, signature_mismatches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------- the restatement == PIL

@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "%dx%d" % s)
def test_restatement_equals_libjpeg_optimize(shape):
    w, h = shape
    for kind in R.CONTENTS:
        u8 = R.to_u8(R.content(kind, w, h))
        for q in R.QUALITIES:
            got, want = O.encode_u8(u8, q), O.pil_encode(u8, q)
            assert got == want, (w, h, kind, q, len(got), len(want))
            assert len(got) <= O.bound(w, h)
            assert len(got) <= len(R.encode_u8(u8, q))  # never larger than the Annex K file


def test_restatement_equals_libjpeg_optimize_at_every_quality():
    u8 = R.to_u8(R.content("noise", 24, 16))
    for q in range(1, 101):
        assert O.encode_u8(u8, q) == O.pil_encode(u8, q), q


@pytest.mark.parametrize("case", J.directed_frames(), ids=lambda c: c[0])
def test_restatement_equals_libjpeg_optimize_on_the_directed_frames(case):
    _, u8, q = case
    assert O.encode_u8(u8, q) == O.pil_encode(u8, q)
    assert O.encode_f32(u8.astype(np.float32), q) == O.pil_encode(u8, q)


def test_the_file_has_the_coefficients_of_the_baseline_file():
    """the pixels a decoder gets are those of the Annex K file"""
    for kind in ("noise", "ramp", "special"):
        u8 = R.to_u8(R.content(kind, 64, 48))
        assert (R.pil_decode(O.encode_u8(u8, 95)) == R.pil_decode(R.encode_u8(u8, 95))).all()


# ---------------------------------------------------------------------------------------------------- the directed problems do what they claim

def _depths(u8, q):
    dc, ac = O.histograms(R.coefficients(u8, q))
    return O.optimal_table(dc)[2], O.optimal_table(ac)[2], dc, ac


def test_fibonacci_frame_is_deeper_than_16():
    u8 = J.fibonacci_frame()
    assert u8.shape == (1112, 1024)
    _, depth, _, ac = _depths(u8, J.FIB_Q)
    assert depth > 16, depth
    assert sorted(ac[ac > 0].tolist())[:19] == J.fibonacci(19)  # the 19 symbols' counts; EOB is the 20th
    bits, vals, _ = O.optimal_table(ac)
    assert sum(bits) == len(vals) == 20 and bits[15] > 0  # folded back to 16


def test_flat_frames_use_one_symbol_per_table():
    u8, q = J.flat_frames()[0]
    d, a, dc, ac = _depths(u8, q)
    assert (d, a) == (1, 1) and (dc > 0).sum() == 1 and (ac > 0).sum() == 1 and ac[0] > 0
    segs = O.dht_segments(O.encode_u8(u8, q))
    assert [len(s) for s in segs] == [22, 22]  # one symbol each


def test_tied_frame_depends_on_the_tie_break():
    u8, q = J.tied_frame()
    assert O.encode_u8(u8, q) != O.encode_u8(u8, q, strict=True)
    assert O.encode_u8(u8, q) == O.pil_encode(u8, q)


def test_no_eob_frame_has_no_eob():
    u8, q = J.no_eob_frame()
    _, _, _, ac = _depths(u8, q)
    assert ac[0] == 0 and ac.sum() == 63 * 2
    assert 0 not in O.optimal_table(ac)[1]


def test_symbol_and_dc_frames_reach_what_8_bits_reach():
    import jenc_problems as P

    frames, reached = P.symbol_frames()
    seen = set()
    for q, u8 in frames.items():
        seen |= set(np.nonzero(O.histograms(R.coefficients(u8, q))[1])[0].tolist())
    assert reached <= seen and len(seen) >= 150
    sizes = set()
    for u8 in P.dc_frames():
        sizes |= set(np.nonzero(O.histograms(R.coefficients(u8, 100))[0])[0].tolist())
    assert sizes == set(range(12))


def test_directed_histograms():
    h = dict(J.histograms())
    depth = {name: O.optimal_table(f)[2] for name, f in h.items()}
    assert depth["deeper_than_32"] > 32 and O.optimal_table(h["deeper_than_32"])[0] is None
    assert depth["depth_32"] == 32 and depth["depth_32_scattered"] == 32 and O.optimal_table(h["depth_32"])[0] is not None
    assert depth["fibonacci_frame_ac"] > 16 and depth["empty"] == 0
    bits, vals, _ = O.optimal_table(h["equal_256"])
    assert sum(bits) == 256 == len(vals)
    assert (h["ones_256"][:256] == 1).all() and h["one_large"].max() == 165000000
    assert len(h) == len(J.histograms())  # the names are distinct


def test_thirteen_frames_have_different_tables():
    for w, h in ((13, 21), (64, 48)):
        segs = {tuple(O.dht_segments(O.encode_f32(f, 95))) for f in J.thirteen(w, h)}
        assert len(segs) >= 2, (w, h)


# ---------------------------------------------------------------------------------------------------- the table rule the device runs

@pytest.fixture(scope="module")
def table_program(tmp_path_factory):
    from mono_dataset_code_amd import build

    return build.build_jopt_table_program(str(tmp_path_factory.mktemp("jopt") / "jopt_table"))


def _run_tables(program, hists):
    text = "%d\n" % len(hists) + "\n".join(" ".join(str(int(x)) for x in f) for f in hists) + "\n"
    r = subprocess.run([program], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = []
    for line in r.stdout.splitlines():
        v = [int(x) for x in line.split()]
        out.append((v[0], v[1], v[2], v[3:19], v[19:]))
    assert len(out) == len(hists)
    return out


def test_table_rule_equals_the_restatement_under_the_sanitizers(table_program):
    """csrc/jpeg_optimal_table.h with the host's search, built with -fsanitize=address,undefined as a program of its own"""
    hists = [f for _, f in J.histograms()]
    rng = np.random.RandomState(11)
    for n in (2, 3, 12, 162, 256):  # random counts with many ties
        for top in (2, 9, 100000):
            f = np.zeros(257, np.int64)
            f[rng.choice(256, n, replace=False)] = rng.randint(1, top, n)
            hists.append(f)
    for _, u8, q in J.directed_frames()[:12]:
        hists += list(O.histograms(R.coefficients(u8, q)))
    f = np.zeros(257, np.int64)  # outside what a frame gives: counts above libjpeg's search limit are never merged
    f[:3] = (2000000000, 1500000000, 7)
    got = _run_tables(table_program, hists + [f])
    assert got[-1][0] == 1
    for f, (status, depth, nvals, bits, vals) in zip(hists, got):
        want_bits, want_vals, want_depth = O.optimal_table(f)
        assert depth == want_depth
        if want_bits is None:
            assert status == 1 and nvals == 0 and bits == [0] * 16
        else:
            assert status == 0 and bits == list(want_bits) and vals == list(want_vals) and nvals == len(want_vals)
    f = np.copy(hists[0])  # entry 256 is ignored
    f[256] = 12345
    assert _run_tables(table_program, [f])[0] == got[0]


def test_table_program_refuses_bad_input(table_program):
    for text in ("", "1\n1 2 3\n", "5000\n", "1\n" + " ".join(["4294967296"] * 257)):
        r = subprocess.run([table_program], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
        assert r.returncode == 2 and "jopt_table" in r.stderr, text[:20]


# ---------------------------------------------------------------------------------------------------- header, exports, table

def test_header_parses_as_c99_and_cxx(tmp_path):
    src = tmp_path / "jopt_abi.c"
    src.write_text('#include "mdc_jopt.h"\nint main(void){ mdcjo_encoder* e = 0; (void)e; return MDCJO_OK + MDCJO_KERNELS - 7 + (mdcjo_jpeg_bound(8, 8) < 0); }\n')
    inc = os.path.join(ROOT, "include")
    for cmd in (["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I" + inc, str(src)],
                ["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", "-I" + inc, str(src)]):
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout


def test_header_library_and_table_are_one_set():
    from mono_dataset_code_amd import build, capi

    names = declared("mdc_jopt.h", "mdcjo_")
    mirrored = sorted(n.replace("mdcj_", "mdcjo_") for n in declared("mdc_jenc.h", "mdcj_"))
    assert set(mirrored) <= set(names) and set(names) - set(mirrored) == {"mdcjo_optimal_tables_device", "mdcjo_profile", "mdcjo_kernel_ms"}
    assert exported(build.LIB_JOPT) == names == sorted(capi.JOPT_API)
    protos = prototypes("mdc_jopt.h", "mdcjo_")
    assert sorted(protos) == names
    assert signature_mismatches(capi.JOPT_API, protos) == []
    for n in mirrored:  # one to one: the same arguments as mdc_jenc.h
        assert capi.JOPT_API[n] == capi.JENC_API[n.replace("mdcjo_", "mdcj_")], n
    wrong = dict(capi.JOPT_API, mdcjo_jpeg_bound=(ctypes.c_int, [ctypes.c_int, ctypes.c_int]))
    assert len(signature_mismatches(wrong, protos)) == 1
    L = capi.jopt_lib()
    assert sorted(vars(L)) == names
    # a library of its own: it links neither the product nor the baseline encoder, and no other library mentions it
    needed = subprocess.run(["readelf", "-d", build.LIB_JOPT], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "libmdc_h" not in needed and "libmdc_jenc" not in needed and "libmdc_" not in needed
    for lib in (build.LIB_HIP, build.LIB_HOST, build.LIB_MULTI, build.LIB_BENCH, build.LIB_JENC):
        assert "mdcjo_" not in subprocess.run(["nm", "-D", lib], stdout=subprocess.PIPE, text=True, check=True).stdout, lib
        assert "libmdc_jopt" not in subprocess.run(["readelf", "-d", lib], stdout=subprocess.PIPE, text=True, check=True).stdout, lib


def test_bound_and_argument_errors_without_a_device():
    from mono_dataset_code_amd import capi

    L = capi.jopt_lib()
    for w, h in R.SHAPES + [(65535, 65535), (1024, 1112)]:
        assert L.mdcjo_jpeg_bound(w, h) == O.bound(w, h)
    for w, h in ((0, 8), (8, 0), (65536, 8), (8, 65536), (-1, -1)):
        assert L.mdcjo_jpeg_bound(w, h) == -1
    for args, code, word in (((8, 8, 0, 1), -1, "quality"), ((8, 8, 101, 1), -1, "quality"), ((0, 8, 95, 1), -3, "65535"),
                             ((8, 65536, 95, 1), -3, "65535"), ((8, 8, 95, 0), -1, "max_frames"), ((65535, 65535, 95, 1), -3, "2^30"),
                             ((8192, 8192, 95, 4096), -3, "2^31")):
        h = ctypes.c_void_p()
        assert L.mdcjo_create(0, *args, ctypes.byref(h)) == code and not h.value, args
        assert word in L.mdcjo_last_error().decode(), (args, L.mdcjo_last_error())
    assert L.mdcjo_encode_f32_device(None, None, 64, 1, None, 1 << 20, None, None) == -1 and "null" in L.mdcjo_last_error().decode()
    assert L.mdcjo_encode_u8_device(None, None, 64, 1, None, 1 << 20, None, None) == -1
    assert L.mdcjo_optimal_tables_device(None, None, 1, None, None, None, None, None) == -1 and "null" in L.mdcjo_last_error().decode()
    assert L.mdcjo_fetch(None, None, 0, None, 1, None, 0, None, None) == -1
    assert L.mdcjo_profile(None, 1) == -1 and L.mdcjo_kernel_ms(None, None) == -1
    with pytest.raises(capi.MdcError):
        capi.JpegEncoder(8, 8, huffman="best")


def test_the_bound_keeps_bit_offsets_in_32_bits():
    """include/mdc_jopt.h: 1665 bits per block at most, 1024 + 418 B <= 2^30"""
    blocks = ((1 << 30) - 1024) // 418
    assert 1024 + 418 * blocks <= 1 << 30 < 1024 + 418 * (blocks + 1)
    assert (27 + 63 * 26) * blocks < 1 << 32
    assert 2 * -(-(27 + 63 * 26) // 8) <= 418 and 102 + (21 + 12) + (21 + 162) + 10 + 2 <= 1024
    assert 64 * blocks < O.SEARCH_LIMIT  # no count of a frame reaches libjpeg's search limit


# ---------------------------------------------------------------------------------------------------- kernels, build identity

JENC_KERNELS = ["jenc_count_kernel", "jenc_fdct_quant_kernel<float>", "jenc_fdct_quant_kernel<unsigned char>", "jenc_gather_kernel",
                "jenc_pack_kernel", "jenc_scan_kernel", "jenc_stuff_kernel"]


def test_kernels_have_no_scratch_and_no_mfma():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_stats

    ks = isa_stats.kernels(isa_stats.device_asm("mdc_jopt.hip"))
    names = sorted(k["pretty"] for k in ks)
    assert names == ["jenc_fdct_quant_kernel<float>", "jenc_fdct_quant_kernel<unsigned char>", "jenc_gather_kernel", "jenc_scan_kernel",
                     "jopt_count_kernel", "jopt_histogram_kernel", "jopt_pack_kernel", "jopt_stuff_kernel", "jopt_tables_kernel",
                     "jopt_tables_only_kernel"], names
    lds_atomic = ("ds_add", "ds_sub", "ds_inc", "ds_dec", "ds_min", "ds_max", "ds_and", "ds_or", "ds_xor", "ds_cmpst", "ds_wrxchg", "ds_pk_add")
    for k in ks:
        assert k["scratch"] == 0, (k["pretty"], k["scratch"])
        assert not any(n.startswith("v_mfma") for n in k["counts"]), k["pretty"]
        # the only atomics: the integer add of the histogram (LDS, then global) and the integer OR of the bit packer
        for n in k["counts"]:
            if "atomic" in n:
                assert n.startswith("global_atomic_add") and "f32" not in n and "f64" not in n or n.startswith("global_atomic_or"), (k["pretty"], n)
            if n.startswith(lds_atomic):
                assert n == "ds_add_u32", (k["pretty"], n)
        # what the build shows: 83 for the stuffing kernel (1024 threads: 128 is the most a workgroup of 16 waves can have), 45 at most
        # for the others, which are launched with 256 threads or fewer and stay at 64 as the baseline's
        assert k["vgpr"] <= (128 if k["pretty"] in ("jopt_stuff_kernel", "jenc_scan_kernel") else 64), (k["pretty"], k["vgpr"])
    by = {k["pretty"]: k["counts"] for k in ks}
    assert by["jopt_histogram_kernel"].get("ds_add_u32") and any(n.startswith("global_atomic_add") for n in by["jopt_histogram_kernel"])
    assert sorted(k["pretty"] for k in isa_stats.kernels(isa_stats.device_asm("mdc_jenc.hip"))) == JENC_KERNELS


def test_product_build_identity_is_unchanged():
    from mono_dataset_code_amd import build

    assert build.code_id() == json.load(open(os.path.join(ROOT, "profiles", "r06_fused_summary.json")))["code_id"]
    deps = set(build.HIP_DEPS) | set(build.HOST_DEPS)
    for f in (build.JOPT_SOURCE, build.JOPT_EXPORT_MAP, build.JOPT_TABLE, build.JPEG_ENCODE_CORE, os.path.join(ROOT, "include", "mdc_jopt.h")):
        assert os.path.exists(f) and f not in deps, f


def test_the_two_encoders_share_one_source():
    """mdc_jenc.hip and mdc_jopt.hip include csrc/jpeg_encode_core.h, and neither defines what it holds -- nor what that header takes
    from csrc/codec_host.h, the one place of every codec library's error buffer and device guard"""
    from mono_dataset_code_amd import build

    core = open(build.JPEG_ENCODE_CORE).read()
    shared = open(build.CODEC_HOST).read()
    assert '#include "codec_host.h"' in core and "struct DeviceGuard" in shared and "struct DeviceGuard" not in core
    for src in (build.JENC_SOURCE, build.JOPT_SOURCE):
        text = open(src).read()
        assert '#include "jpeg_encode_core.h"' in text and "struct DeviceGuard" not in text
        for name in ("void walk_block(", "struct BitPacker", "struct BitCounter", "void jenc_scan_kernel(", "void jenc_gather_kernel(", "void fdct_pass(",
                     "kAcVals[162]", "void huffman_table(", "long long blocks_of(", "struct Encoder", "int64_t fetch(", "int output_device("):
            assert name in core and name not in text, (src, name)
