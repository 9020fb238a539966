"""The device JPEG encoder (include/mdc_jenc.h, libmdc_jenc.so) as far as it can be checked without a GPU: its specification,
restated in NumPy (tests/jenc_restatement.py), equals libjpeg-turbo through PIL byte for byte; its header, library and ctypes
table declare the same functions; its kernels compile without scratch and without MFMA; and the product library's build
identity is untouched by it."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import jenc_restatement as R
from test_abi import declared, exported, prototypes, signature_mismatches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pil_is_libjpeg_turbo():
    from PIL import features

    assert features.check("jpg")


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "%dx%d" % s)
def test_restatement_equals_libjpeg(shape):
    """Every stage as include/mdc_jenc.h prescribes it == the file PIL writes, for every shape, content and quality of the GPU test."""
    w, h = shape
    for kind in R.CONTENTS:
        u8 = R.to_u8(R.content(kind, w, h))
        for q in R.QUALITIES:
            got, want = R.encode_u8(u8, q), R.pil_encode(u8, q)
            assert got == want, (w, h, kind, q, len(got), len(want))
            assert len(got) <= R.bound(w, h)


def test_noise_case_needs_byte_stuffing():
    scan = R.pil_encode(R.to_u8(R.content("noise", 640, 480)), 95)[328:-2]
    assert b"\xff\x00" in scan


def test_float_to_8bit_rule():
    """cv::Mat::convertTo(CV_8U): nearest, ties to even, clamped, NaN -> 0"""
    got = R.to_u8(np.array([-0.5, 0.5, 1.5, 2.5, 254.5, 255.5, -3, 300, np.nan], np.float32))
    assert got.tolist() == [0, 0, 2, 2, 254, 255, 0, 255, 0]


def test_header_parses_as_c99_and_cxx(tmp_path):
    src = tmp_path / "jenc_abi.c"
    src.write_text('#include "mdc_jenc.h"\nint main(void){ mdcj_encoder* e = 0; (void)e; return MDCJ_OK + (mdcj_jpeg_bound(8, 8) < 0); }\n')
    inc = os.path.join(ROOT, "include")
    for cmd in (["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I" + inc, str(src)],
                ["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", "-I" + inc, str(src)]):
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout


def test_header_library_and_table_are_one_set():
    from mono_dataset_code_amd import build, capi

    names = declared("mdc_jenc.h", "mdcj_")
    assert len(names) >= 6 and "mdcj_encode_f32_device" in names and "mdcj_encode_u8_device" in names
    assert exported(build.LIB_JENC) == names == sorted(capi.JENC_API)
    protos = prototypes("mdc_jenc.h", "mdcj_")
    assert sorted(protos) == names
    assert signature_mismatches(capi.JENC_API, protos) == []
    # the check can fail
    wrong = dict(capi.JENC_API, mdcj_jpeg_bound=(ctypes.c_int, [ctypes.c_int, ctypes.c_int]))
    assert len(signature_mismatches(wrong, protos)) == 1
    L = capi.jenc_lib()
    assert sorted(vars(L)) == names
    for n, (restype, argtypes) in capi.JENC_API.items():
        assert getattr(L, n).restype is restype and list(getattr(L, n).argtypes) == argtypes, n
    # a library of its own: the product neither links nor exports it, and it does not link the product
    for lib in (build.LIB_HIP, build.LIB_HOST, build.LIB_MULTI, build.LIB_BENCH):
        assert "mdcj_" not in subprocess.run(["nm", "-D", lib], stdout=subprocess.PIPE, text=True, check=True).stdout, lib
        assert "libmdc_jenc" not in subprocess.run(["readelf", "-d", lib], stdout=subprocess.PIPE, text=True, check=True).stdout, lib
    assert "libmdc_h" not in subprocess.run(["readelf", "-d", build.LIB_JENC], stdout=subprocess.PIPE, text=True, check=True).stdout


def test_bound_and_argument_errors_without_a_device():
    """mdcj_jpeg_bound, and the argument checks that come before any HIP call: a status and a message, never a fault."""
    from mono_dataset_code_amd import capi

    L = capi.jenc_lib()
    for w, h in R.SHAPES + [(65535, 65535)]:
        assert L.mdcj_jpeg_bound(w, h) == R.bound(w, h)
    for w, h in ((0, 8), (8, 0), (65536, 8), (8, 65536), (-1, -1)):
        assert L.mdcj_jpeg_bound(w, h) == -1
    for args, code, word in (((8, 8, 0, 1), -1, "quality"), ((8, 8, 101, 1), -1, "quality"), ((0, 8, 95, 1), -3, "65535"),
                             ((8, 65536, 95, 1), -3, "65535"), ((8, 8, 95, 0), -1, "max_frames"), ((65535, 65535, 95, 1), -3, "2^30"),
                             ((8192, 8192, 95, 4096), -3, "2^31")):
        h = ctypes.c_void_p()
        assert L.mdcj_create(0, *args, ctypes.byref(h)) == code and not h.value, args
        assert word in L.mdcj_last_error().decode(), (args, L.mdcj_last_error())
    assert L.mdcj_encode_f32_device(None, None, 64, 1, None, 1 << 20, None, None) == -1 and "null" in L.mdcj_last_error().decode()


def test_kernels_have_no_scratch_and_no_mfma():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_stats

    ks = isa_stats.kernels(isa_stats.device_asm("mdc_jenc.hip"))
    names = sorted(k["pretty"] for k in ks)
    assert names == ["jenc_count_kernel", "jenc_fdct_quant_kernel<float>", "jenc_fdct_quant_kernel<unsigned char>", "jenc_gather_kernel",
                     "jenc_pack_kernel", "jenc_scan_kernel", "jenc_stuff_kernel"], names
    for k in ks:
        assert k["scratch"] == 0, (k["pretty"], k["scratch"])
        assert not any(n.startswith("v_mfma") for n in k["counts"]), k["pretty"]
        # no floating-point atomics: the only atomic is the integer OR of the bit packer
        assert all(n.startswith("global_atomic_or") for n in k["counts"] if "atomic" in n), (k["pretty"], k["counts"])
        assert k["vgpr"] <= 64, (k["pretty"], k["vgpr"])


def test_product_build_identity_is_unchanged():
    """The encoder is outside build.HIP_DEPS: the product library is the build the committed profiles were measured on."""
    from mono_dataset_code_amd import build

    assert build.code_id() == json.load(open(os.path.join(ROOT, "profiles", "r06_fused_summary.json")))["code_id"]
    deps = set(build.HIP_DEPS) | set(build.HOST_DEPS)
    for f in (build.JENC_SOURCE, build.JENC_EXPORT_MAP, os.path.join(ROOT, "include", "mdc_jenc.h"), build.PLAY_DATASET_SOURCE):
        assert os.path.exists(f) and f not in deps, f


def test_program_is_built_and_prints_the_reference_header(tmp_path):
    """bin/playDataset with one argument: the reference's header lines (:55-70) around the reader's own, then the viewer note, exit 0.
    (No frame is touched, so this runs without a GPU.)"""
    from mono_dataset_code_amd import build, synth

    d = str(tmp_path / "seq")
    synth.write_sequence_calibration(d, ("0.349153 0.436593 0.493140 0.499021 0.933271", "320 256", "crop", "192 144"), vignette_bits=16, n_times=1)
    os.makedirs(os.path.join(d, "images"))
    synth.write_png_gray(os.path.join(d, "images", "00000.png"), synth.smooth_frame(320, 256, 0.7).reshape(256, 320))
    r = subprocess.run([build.PLAY_DATASET, d], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout
    lines = r.stdout.splitlines()
    assert lines[0] == "Playback dataset %s!" % d
    at = lines.index("Rectified Images: 192 x 144. K:")
    assert [l.split() for l in lines[at + 1:at + 4]] == [["23.2996", "0", "88.0573"], ["0", "40.0524", "71.3648"], ["0", "0", "1"]]
    assert len({len(l) for l in lines[at + 1:at + 4]}) == 1 and lines[at + 4] == "" and lines[at + 5].startswith("Original Images: 320 x 256. omega=0.933271 K:")
    assert "viewer is not built" in lines[-1] and "Saving undistorted" not in r.stdout
    assert not [f for f in os.listdir(str(tmp_path)) if f.endswith(".jpg")]
