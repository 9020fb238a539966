"""class UndistorterFOV is a drop-in class: programs compiled against an earlier FOVUndistorter.h (the drop-in drivers of
oracle/Makefile, a user's own build) allocate the class's earlier size and must keep running on today's libmdc_host.so.  The lens
models therefore add no data member: tests/native/lens_layout.cpp asserts the size at compile time and constructs FOV, RadTan
and EquiDistant objects in buffers of exactly that size with guard bytes behind them."""
import os
import subprocess

import lens_problems as LP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_class_has_not_grown_and_nothing_is_written_past_it(tmp_path):
    from mono_dataset_code_amd import build

    build.build_host()
    exe = str(tmp_path / "lens_layout")
    inc = os.path.join(ROOT, "include")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++11", "-Wall", "-Werror", "-I" + inc, "-I" + os.path.join(inc, "mono_dataset_code"), "-I" + build.eigen_include(),
                        os.path.join(ROOT, "tests", "native", "lens_layout.cpp"), "-L" + build.PKG, "-lmdc_host", "-lmdc_hip", "-Wl,-rpath," + build.PKG, "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    cams = []
    for name, lines in (("fov", ("0.349153 0.436593 0.493140 0.499021 0.933271", "320 256", "crop", "192 144")), ("radtan", LP.PROBLEMS["barrel_crop"]),
                        ("fisheye", LP.PROBLEMS["fisheye_explicit"]), ("bad_line3", LP.MALFORMED["full"][0])):
        (tmp_path / name).mkdir()
        cams.append(LP.write_camera(tmp_path / name, lines))
    r = subprocess.run([exe] + cams, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    said = [l for l in r.stderr.splitlines() if l.startswith("lens_layout:")]
    assert r.returncode == 0 and len(said) == 4 and all(", 0 bytes written past" in l for l in said), r.stderr[-3000:]
    assert ["lens %d," % k in l for k, l in zip((0, 1, 2, 1), said)] == [True] * 4, said
