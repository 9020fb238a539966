"""The XCD placement arithmetic of the remap kernels (mono_dataset_code_amd/csrc/xcd_placement.h: the table block -> tile for the four
MDC_ORDER_* modes, the even split of the rotated bands, the entry block (x, y) reads) under g++ over every tile grid 1..12 x 1..40,
rotation off and on, 1..40 frame groups -- no GPU.  Once as it is, once under AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHECKS = ("entry formula ok", "rotation off is the parent's table ok", "5x15 and 5x30 literals ok", "even split of the rotated bands ok",
          "every group covers every tile once ok", "shares keep the neighbourhood ok", "equal totals at multiples of 8 groups ok",
          "band totals within groups mod 8 ok", "headline shares ok")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_xcd_placement_arithmetic(tmp_path, sanitize):
    exe = str(tmp_path / "xcd_placement_cpu")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"] if sanitize else []
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + san +
                       ["-I" + os.path.join(ROOT, "mono_dataset_code_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "native", "xcd_placement_cpu.cpp"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "FAIL" not in r.stdout, r.stdout
    for c in CHECKS:
        assert c in r.stdout, (c, r.stdout)
    assert " 0 failures" in r.stdout, r.stdout
