"""What the eight device codec libraries have in one copy (csrc/codec_host.h, the host sides in png_decode_kernels.h and
jpeg_encode_core.h, build.py's one rule), as far as it can be checked without a GPU: sibling libraries answer the same argument errors
with the same status and, their prefix aside, the same message; the error buffer, fail() and the device guard are defined once; every
library's build rule depends on codec_host.h and libmdc_hip.so's identity does not."""
import ctypes
import os

import pytest

from mono_dataset_code_amd import build, capi

CODECS = {"jenc": build.LIB_JENC, "jopt": build.LIB_JOPT, "zipw": build.LIB_ZIPW, "pngw": build.LIB_PNGW, "pngw_rgb": build.LIB_PNGW_RGB,
          "pnglz": build.LIB_PNGLZ, "pngd": build.LIB_PNGD, "pngdx": build.LIB_PNGDX}


def _decoder_errors(L, pre):
    """(status, message) of every argument error of a decoder that is reported before any HIP call: the cases of
    test_argument_errors_without_a_device in test_pngd_cpu.py and test_pngdx_cpu.py, and each one's other limit of the scratch"""
    fn = lambda name: getattr(L, pre + name)
    h = ctypes.c_void_p()
    p = ctypes.c_void_p(4096)  # never dereferenced on the host
    calls = [lambda: fn("create")(0, 4, 4, 1, None),
             lambda: fn("create")(0, 4, 4, 0, ctypes.byref(h)),
             lambda: fn("create")(0, 0, 4, 1, ctypes.byref(h)),
             lambda: fn("create")(0, 4, -1, 1, ctypes.byref(h)),
             lambda: fn("create")(0, 16384, 16384, 1, ctypes.byref(h)),
             lambda: fn("create")(0, 16383, 16384, 5000, ctypes.byref(h)),
             lambda: fn("decode_device")(None, p, 100, p, 0, 0, 1, p, 16, p, None),
             lambda: fn("decode_host")(None, None, None, 1, None, None),
             lambda: fn("profile")(None, 1),
             lambda: fn("kernel_ms")(None, None),
             lambda: fn("synchronize")(None)]
    out = []
    for call in calls:
        rc = call()
        out.append((rc, fn("last_error")().decode()))
        assert rc < 0 and not h.value, out[-1]
    assert fn("stream")(None) is None
    fn("destroy")(None)
    return out


def test_the_two_png_decoders_report_argument_errors_alike():
    a = _decoder_errors(capi.pngd_lib(), "mdci_")
    b = _decoder_errors(capi.pngdx_lib(), "mdcx_")
    assert [rc for rc, _ in a] == [rc for rc, _ in b] == [-1, -1, -3, -3, -3, -3, -1, -1, -1, -1, -1]
    assert [m for _, m in a] == [m.replace("mdcx_", "mdci_") for _, m in b]
    assert all(m.startswith("mdci_") for _, m in a) and all(m.startswith("mdcx_") for _, m in b)


def _encoder_errors(L, pre):
    """the same for a JPEG encoder: create, encode_*, output_device and fetch (test_bound_and_argument_errors_without_a_device in
    test_jenc_cpu.py and test_jopt_cpu.py)"""
    fn = lambda name: getattr(L, pre + name)
    h = ctypes.c_void_p()
    calls = [lambda: fn("create")(0, 8, 8, 95, 1, None)]
    for args in ((8, 8, 0, 1), (8, 8, 101, 1), (0, 8, 95, 1), (8, 65536, 95, 1), (8, 8, 95, 0), (65535, 65535, 95, 1), (8192, 8192, 95, 4096)):
        calls.append(lambda args=args: fn("create")(0, *args, ctypes.byref(h)))
    calls += [lambda: fn("encode_f32_device")(None, None, 64, 1, None, 1 << 20, None, None),
              lambda: fn("encode_u8_device")(None, None, 64, 1, None, 1 << 20, None, None),
              lambda: fn("output_device")(None, None, None, None),
              lambda: fn("fetch")(None, None, 0, None, 1, None, 0, None, None)]
    out = []
    for call in calls:
        rc = call()
        out.append((rc, fn("last_error")().decode()))
        assert rc < 0 and not h.value, out[-1]
    fn("destroy")(None)
    return out


def test_the_two_jpeg_encoders_report_argument_errors_alike():
    a = _encoder_errors(capi.jenc_lib(), "mdcj_")
    b = _encoder_errors(capi.jopt_lib(), "mdcjo_")
    assert [rc for rc, _ in a] == [rc for rc, _ in b] == [-1, -1, -1, -3, -3, -1, -3, -3, -1, -1, -1, -1]
    assert [m for _, m in a] == [m.replace("mdcjo_", "mdcj_") for _, m in b]
    assert all(m.startswith("mdcj_") for _, m in a) and all(m.startswith("mdcjo_") for _, m in b)


@pytest.fixture(scope="module")
def rules():
    """library -> the dependency list its build rule hands to build._stale, recorded without building anything"""
    seen = {}
    real = build._stale
    build._stale = lambda target, deps: seen.setdefault(target, list(deps)) and False
    try:
        for name in CODECS:
            getattr(build, "build_" + name)()
    finally:
        build._stale = real
    assert set(seen) == set(CODECS.values())
    return seen


def test_every_codec_rule_depends_on_codec_host_and_the_product_identity_does_not(rules):
    assert os.path.exists(build.CODEC_HOST) and os.path.basename(build.CODEC_HOST) == "codec_host.h"
    for lib, deps in rules.items():
        assert build.CODEC_HOST in deps, lib
        assert all(os.path.exists(d) for d in deps if not d.endswith(".so")), lib
    assert build.CODEC_HOST not in build.HIP_DEPS


def test_error_buffer_fail_and_device_guard_are_defined_once(rules):
    sources = sorted({d for deps in rules.values() for d in deps if d.startswith(build.CSRC + os.sep) and d.endswith((".h", ".hip"))})
    assert len(sources) >= 8 + 7  # the eight libraries' seven units, and at least the shared headers there were before
    for text in ("struct DeviceGuard", "thread_local char g_error", "vsnprintf(g_error"):
        holders = [os.path.basename(s) for s in sources if text in open(s, encoding="utf-8").read()]
        assert holders == ["codec_host.h"], (text, holders)


def _stale_after_touching(rules, touched, monkeypatch):
    """the libraries build._stale calls out of date when `touched` alone is newer than every library"""
    stale = []
    for lib, deps in rules.items():
        assert os.path.exists(lib), "%s: run `python -m mono_dataset_code_amd.build`" % lib
        monkeypatch.setattr(os.path, "getmtime", lambda p, lib=lib: 2.0 if p == touched else 1.0 if p == lib else 0.0)
        if build._stale(lib, deps):
            stale.append(lib)
        monkeypatch.undo()
    return sorted(stale)


def test_touching_a_shared_header_makes_its_libraries_stale_and_no_other(rules, monkeypatch):
    assert _stale_after_touching(rules, build.CODEC_HOST, monkeypatch) == sorted(CODECS.values())
    assert _stale_after_touching(rules, build.PNG_DECODE_KERNELS, monkeypatch) == sorted([build.LIB_PNGD, build.LIB_PNGDX])
    assert _stale_after_touching(rules, build.JPEG_ENCODE_CORE, monkeypatch) == sorted([build.LIB_JENC, build.LIB_JOPT])
    assert _stale_after_touching(rules, os.path.join(build.CSRC, "mdc_kernels.hip"), monkeypatch) == []
