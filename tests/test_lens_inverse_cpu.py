"""Raw pixel -> rectified pixel for every lens kind, without a GPU: the NumPy restatement of csrc/lens_inverse_model.h's contract
(tests/lens_inverse_restatement.py) against a float64 inverse, its tangent against float64 tan, the arithmetic header as a
stand-alone program under the sanitizers, libmdc_lensinv.so's interface and argument checks, and undistortCoordinates' host path."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import lens_inverse_restatement as V
import lens_problems as LP
import lens_restatement as R
from conftest import bits_equal
from test_abi import declared, exported, prototypes, signature_mismatches
from test_lens_cpu import _fmix32, _hex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def problems():
    """name -> inverse problem (kind, cameras in pixels, sizes) of every camera of lens_problems and the two FOV cameras"""
    out = {}
    for name, lines in LP.PROBLEMS.items():
        p = R.parse(lines)
        assert p["valid"], name
        out[name] = V.inverse_problem(p)
    out["fov_survey"] = V.fov_problem(V.SURVEY_FOV)
    out["fov_small"] = V.fov_problem(V.SMALL_FOV)
    return out


TABLE_PROBLEMS = list(LP.SMALL) + ["barrel_ragged", "fov_small"]


@pytest.fixture(scope="module")
def tables(problems):
    """the inverse tables of the small problems, once"""
    return {name: V.inverse_tables(problems[name]) for name in TABLE_PROBLEMS}


def test_inverse_restatement_stays_close_to_float64(problems):
    """40 000 seeded raw points inside each camera's raw image: the float32 restatement against the float64 inverse wherever that
    one's normalised rectified radius is at most 2 (beyond, the tangent amplifies by 1 + r^2 and absolute pixels mean nothing),
    within 2^-16 * S pixels, S the largest rectified coordinate magnitude among the compared points.  TUM-VI's corners lie past 90
    degrees and come out NaN."""
    for i, (name, q) in enumerate(problems.items()):
        rng = np.random.default_rng(4000 + i)
        x = rng.uniform(0, q["in_w"] - 1, 40000).astype(F)
        y = rng.uniform(0, q["in_h"] - 1, 40000).astype(F)
        gx, gy = V.undistort(q["kind"], q["cam"], q["rect"], x, y)
        wx, wy, r = V.undistort64(q["kind"], q["cam"], q["rect"], x, y)
        with np.errstate(invalid="ignore"):
            keep = r <= 2.0
        assert keep.sum() > 20000, (name, int(keep.sum()))
        S = max(np.abs(wx[keep]).max(), np.abs(wy[keep]).max())
        err = max(np.abs(gx[keep] - wx[keep]).max(), np.abs(gy[keep] - wy[keep]).max())
        cap = 2.0 ** -16 * S
        print("%s: %.3g px at S = %.4g (cap %.3g, 2^%.1f S), %d of 40000 compared" % (name, err, S, cap, np.log2(max(err, 1e-30) / S), int(keep.sum())))
        assert err <= cap, (name, err, cap)
    q = problems["tumvi"]
    cx, cy = np.array([0, q["in_w"] - 1, 0, q["in_w"] - 1], F), np.array([0, 0, q["in_h"] - 1, q["in_h"] - 1], F)
    gx, gy = V.undistort(q["kind"], q["cam"], q["rect"], cx, cy)
    assert np.isnan(gx).all() and np.isnan(gy).all()
    assert np.isnan(V.undistort64(q["kind"], q["cam"], q["rect"], cx, cy)[0]).all()


def test_inverse_undoes_the_forward_restatement(problems):
    """a wrong sign or swapped p1 / p2 in the inverse cannot hide behind a float64 inverse written the same way: rectified grid
    points through R.distort and back land where they started, within the two directions' caps"""
    for name in LP.SMALL:
        q = problems[name]
        gx, gy = R.grid(q["out_w"], q["out_h"])
        x, y = R.distort(q["kind"], q["cam"], q["rect"], gx, gy)
        bx, by = V.undistort(q["kind"], q["cam"], q["rect"], x, y)
        err = max(np.abs(bx - gx).max(), np.abs(by - gy).max())
        cap = round_trip_cap(q, max(np.abs(gx).max(), np.abs(gy).max()))
        print("%s: round trip %.3g px (cap %.3g)" % (name, err, cap))
        assert err <= cap, (name, err, cap)


def round_trip_cap(q, S):
    """rectified -> raw -> rectified: the inverse's cap above, 2^-16 * S with S the largest rectified coordinate magnitude among the
    points, plus the forward cap of test_lens_cpu.test_restatement_stays_close_to_float64, max(in_w, in_h) * 2^-19"""
    return 2.0 ** -16 * S + max(q["in_w"], q["in_h"]) * 2.0 ** -19


def test_tanf_spec_against_float64_tan():
    """every float32 in [2^-12, pi/2) whose bit pattern is a multiple of 64, all floats within 4096 ulps of pi/4 and the last 4096
    below pio2_hi: within 4 units in the last place of float64 tan"""
    lo, hi = int(F(2.0 ** -12).view(np.uint32)), int(V.PIO2_HI.view(np.uint32))
    p4 = int(V.PIO4.view(np.uint32))
    bits = np.unique(np.concatenate([np.arange((lo + 63) // 64 * 64, hi, 64, dtype=np.uint32), np.arange(p4 - 4096, p4 + 4097, dtype=np.uint32),
                                     np.arange(hi - 4096, hi, dtype=np.uint32)]))
    x = bits.view(F)
    assert x.size > 1.5e6 and x[-1] < V.PIO2_HI and float(x[-1]) < np.pi / 2
    want = np.tan(x.astype(np.float64))
    got = V.tanf_spec(x)
    ulps = np.abs(got.astype(np.float64) - want) / np.spacing(want.astype(F)).astype(np.float64)
    print("tanf_spec: %.3f ulp at %r, %d arguments" % (ulps.max(), float(x[ulps.argmax()]), x.size))
    assert ulps.max() <= 4.0
    assert bits_equal(V.tanf_spec(-x[::1000]), -got[::1000]) and V.tanf_spec(F(0)) == 0 and np.isnan(V.tanf_spec(F(np.nan)))


INV_SEED = {V.PINHOLE: 111, V.RADTAN: 222, V.EQUIDISTANT: 333, V.FOV: 444}
# principal point at 0: points within rd <= 1e-8 of it exist in float
INV_CAM = {V.PINHOLE: [60, 58, 0, 0, 0, 0, 0, 0], V.RADTAN: [60, 58, 0, 0] + [float(v) for v in LP.BARREL.split()[5:]],
           V.EQUIDISTANT: [40, 40, 0, 0] + [float(v) for v in LP.FISHEYE.split()[5:]], V.FOV: [55, 60, 0, 0, 0.9, 0, 0, 0]}
INV_RECT = (37.25, 41.5, 31.5, 23.5)
KINDS = (V.PINHOLE, V.RADTAN, V.EQUIDISTANT, V.FOV)
N_RANDOM = 10 ** 6


def inverse_points(seed, idx, cam):
    """raw points `idx` (an int64 array) of the R job with this seed, as tests/native/lens_inverse_core.cpp documents them"""
    idx = np.asarray(idx, np.int64)
    fx, fy, cx, cy = (F(v) for v in cam[:4])

    def value(c):
        h = _fmix32((c & 0xFFFFFFFF).astype(np.uint32))
        uniform = (F(-64.0) + F(256.0) * (h >> np.uint32(8)).astype(F) / F(16777216.0)).astype(F)
        return np.where(idx % 2 == 0, h.view(F), uniform).astype(F)

    x, y = value(seed + 2 * idx), value(seed + 2 * idx + 1)
    special = [(F(np.nan), F(1)), (F(np.inf), F(2)), (F(3), F(-np.inf)), (F(0), F(0)), (cx, cy), (cx + fx * F(5e-9), cy), (cx, cy - fy * F(9e-9)),
               (cx + fx * F(1e-12), cy + fy * F(1e-12)), (cx + fx * F(3), cy + fy * F(3)), (cx - fx * F(40), cy + fy * F(0.5))]
    for i, (sx, sy) in enumerate(special):
        x[idx == i], y[idx == i] = sx, sy
    return x, y


def test_specials_come_out_as_the_contract_says():
    idx = np.arange(10)
    for kind in KINDS:
        x, y = inverse_points(INV_SEED[kind], idx, INV_CAM[kind])
        gx, gy = V.undistort(kind, INV_CAM[kind], INV_RECT, x, y)
        assert np.isnan(gx[0]) and (kind == V.PINHOLE or np.isnan(gy[0])), kind  # NaN in, NaN out
        assert bits_equal(gx[3:8], np.full(5, INV_RECT[2], F)) and bits_equal(gy[3:8], np.full(5, INV_RECT[3], F)), kind  # the centre
        if kind in (V.EQUIDISTANT, V.FOV):  # rd = 4.2 and 40: past the half plane
            assert np.isnan(gx[8:]).all() and np.isnan(gy[8:]).all() and np.isnan(gx[1:3]).all(), kind


def test_inverse_header_as_a_sanitized_program(tmp_path, problems, tables):
    """tests/native/lens_inverse_core.cpp (its own main, ASan + UBSan, nothing preloaded): the inverse tables of every small problem,
    and 10^6 seeded points per kind with NaN, infinities, the principal point, rd <= 1e-8 and points outside the domain among them,
    against the restatement bit for bit (the points on a 4096-point sample per kind); a clean exit."""
    from mono_dataset_code_amd import build

    exe = build.build_lens_inverse_core_program(str(tmp_path / "lens_inverse_core"), sanitize=True)
    jobs = []
    for name in TABLE_PROBLEMS:
        q = problems[name]
        jobs.append(" ".join(["T", str(q["kind"])] + [_hex(v) for v in q["cam"]] + [_hex(v) for v in q["rect"]] + [str(q[k]) for k in ("in_w", "in_h", "out_w", "out_h")]))
    for kind in KINDS:
        jobs.append(" ".join(["R", str(kind)] + [_hex(v) for v in INV_CAM[kind]] + [_hex(v) for v in INV_RECT] + [str(INV_SEED[kind]), str(N_RANDOM)]))
    (tmp_path / "jobs.txt").write_text("\n".join(jobs) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([exe, str(tmp_path / "jobs.txt"), str(tmp_path / "out.bin")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)
    assert r.returncode == 0 and r.stderr == "" and "lens_inverse_core: %d jobs" % len(jobs) in r.stdout, (r.returncode, r.stderr[-2000:])
    raw = np.fromfile(str(tmp_path / "out.bin"), np.uint8)
    at = 0

    def take(dtype, n):
        nonlocal at
        a = raw[at:at + 4 * n].view(dtype)
        at += 4 * n
        return a

    for name in TABLE_PROBLEMS:
        q = problems[name]
        wx, wy, woutside = tables[name]
        n = q["in_w"] * q["in_h"]
        assert bool(take(np.int32, 1)[0]) == woutside, name
        assert bits_equal(take(F, n), wx) and bits_equal(take(F, n), wy), name
    rng = np.random.default_rng(7)
    for kind in KINDS:
        gx, gy = take(F, N_RANDOM), take(F, N_RANDOM)
        idx = np.unique(np.concatenate([np.arange(16), rng.integers(0, N_RANDOM, 4096 - 16)]))
        x, y = inverse_points(INV_SEED[kind], idx, INV_CAM[kind])
        wx, wy = V.undistort(kind, INV_CAM[kind], INV_RECT, x, y)
        assert idx[0] == 0 and np.isnan(wx[0]) and np.isnan(gx[0]), kind
        assert bits_equal(gx[idx], wx) and bits_equal(gy[idx], wy), kind
        assert np.isfinite(wx).sum() > 500, kind  # the sample is not all NaN
    assert at == raw.size


def test_inverse_tables_are_what_they_claim(problems, tables):
    """every raw pixel of a small problem is outside the rectified image or strictly inside it, some of both"""
    for name in TABLE_PROBLEMS:
        q = problems[name]
        ux, uy, outside = tables[name]
        black = ux == -1
        assert outside == bool(black.any()) and not black.all() and np.array_equal(black, uy == -1), name
        if LP.PROBLEMS.get(name, ("", "", ""))[2] == "crop":  # a cropped rectified image shows less than the raw one
            assert outside, name
        assert (ux[~black] > 0).all() and (ux[~black] < q["out_w"] - 1).all() and (uy[~black] > 0).all() and (uy[~black] < q["out_h"] - 1).all(), name


def make_fov(tmp_path, lines):
    from mono_dataset_code_amd import capi

    return capi.UndistorterFOV(LP.write_camera(tmp_path, lines))


@pytest.mark.parametrize("name", list(LP.PROBLEMS) + ["fov_survey", "fov_small"])
def test_class_host_path_equals_the_restatement(name, tmp_path, problems):
    """small calls of undistortCoordinates run the host loop over the header; inverse_model() hands the same cameras over"""
    from mono_dataset_code_amd import capi

    lines = LP.PROBLEMS.get(name) or {"fov_survey": V.SURVEY_FOV, "fov_small": V.SMALL_FOV}[name]
    q = problems[name]
    fov = make_fov(tmp_path, lines)
    assert fov.is_valid()
    m = fov.inverse_model()
    assert (m.kind, m.in_w, m.in_h, m.out_w, m.out_h) == (q["kind"], q["in_w"], q["in_h"], q["out_w"], q["out_h"])
    assert bits_equal([m.fx, m.fy, m.cx, m.cy] + list(m.k), np.array(q["cam"], F)) and bits_equal([m.ofx, m.ofy, m.ocx, m.ocy], np.array(q["rect"], F))
    rng = np.random.default_rng(21)
    x, y = rng.uniform(-10, q["in_w"] + 10, 5000).astype(F), rng.uniform(-10, q["in_h"] + 10, 5000).astype(F)
    x[0], y[1] = np.nan, np.inf
    wx, wy = V.undistort(q["kind"], q["cam"], q["rect"], x, y)
    fov.undistort_coordinates(x, y)
    assert bits_equal(x, wx) and bits_equal(y, wy)
    assert np.isfinite(wx).sum() > 2500


def test_invalid_object_prints_and_touches_nothing(tmp_path, capfd):
    from mono_dataset_code_amd import capi

    fov = make_fov(tmp_path, LP.MALFORMED["full"][0])
    assert not fov.is_valid()
    x = np.array([1.0, 2.0], F)
    ctypes.CDLL(None).fflush(None)
    capfd.readouterr()
    fov.undistort_coordinates(x, x.copy())
    ctypes.CDLL(None).fflush(None)
    assert "ERROR: invalid UndistorterFOV!" in capfd.readouterr().out and x.tolist() == [1.0, 2.0]
    with pytest.raises(capi.MdcError):
        fov.inverse_model()


def test_libmdc_lensinv_interface(tmp_path):
    from mono_dataset_code_amd import build, capi

    names = declared("mdc_lensinv.h", "mdcu_")
    assert exported(build.LIB_LENSINV) == names == sorted(capi.LENSINV_API) and "mdcu_inverse_remap_device" in names
    assert signature_mismatches(capi.LENSINV_API, prototypes("mdc_lensinv.h", "mdcu_")) == []
    needed = subprocess.run(["readelf", "-d", build.LIB_LENSINV], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "libmdc_" not in needed  # it links nothing of this project
    assert "libmdc_lensinv" not in subprocess.run(["readelf", "-d", build.LIB_HOST], stdout=subprocess.PIPE, text=True, check=True).stdout
    src = tmp_path / "abi.c"
    src.write_text('#include "mdc_lensinv.h"\nint main(void){ mdcu_model m; m.kind = MDCU_FOV; (void)m; return sizeof(mdcu_model) == 68 ? MDCU_OK : 1; }\n')
    inc = os.path.join(ROOT, "include")
    for cmd in (["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I" + inc, str(src)],
                ["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", "-I" + inc, str(src)]):
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-std=c99", "-I" + inc, str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)]).returncode == 0  # sizeof(mdcu_model) is 68
    assert ctypes.sizeof(capi.LensModel) == 68
    assert (capi.LENSINV_PINHOLE, capi.LENSINV_RADTAN, capi.LENSINV_EQUIDISTANT, capi.LENSINV_FOV) == (0, 1, 2, 3) == KINDS
    for f in ("lens_inverse_model.h", "mdc_lensinv.hip", "mdc_lensinv_exports.map"):
        assert os.path.join(build.CSRC, f) not in build.HIP_DEPS, f
    assert os.path.join(build.INC, "mdc_lensinv.h") not in build.HIP_DEPS


def test_argument_errors_and_no_device():
    import torch

    from mono_dataset_code_amd import capi

    L = capi.lensinv_lib()
    cam = INV_CAM[V.RADTAN]
    good = capi.LensModel.make(capi.LENSINV_RADTAN, cam, INV_RECT)
    x, y = np.arange(8, dtype=F), np.arange(8, dtype=F) + F(100)
    x0, y0 = x.copy(), y.copy()
    nan = float("nan")
    for bad in (capi.LensModel.make(7, cam, INV_RECT), capi.LensModel.make(-1, cam, INV_RECT),
                capi.LensModel.make(capi.LENSINV_RADTAN, cam, (0.0, 41.5, 0, 0)), capi.LensModel.make(capi.LENSINV_FOV, cam, (1.0, nan, 0, 0)),
                capi.LensModel.make(capi.LENSINV_RADTAN, [0.0] + cam[1:], INV_RECT), capi.LensModel.make(capi.LENSINV_EQUIDISTANT, [60, nan] + cam[2:], INV_RECT)):
        with pytest.raises(capi.MdcError) as e:
            capi.LensInverse(bad).undistort_points_host(x, y)
        assert e.value.code == capi.ERR_ARG and "mdcu_undistort_points_host" in str(e.value)
        assert L.mdcu_undistort_points_device(ctypes.byref(bad), None, None, 0, None) == capi.ERR_ARG
        assert L.mdcu_inverse_remap_device(ctypes.byref(bad), None, None, None, None) == capi.ERR_ARG
    assert L.mdcu_undistort_points_host(0, None, None, None, 1) == capi.ERR_ARG
    assert L.mdcu_undistort_points_host(0, ctypes.byref(good), None, None, -1) == capi.ERR_ARG
    assert L.mdcu_undistort_points_host(0, ctypes.byref(good), None, None, 4) == capi.ERR_ARG
    assert L.mdcu_undistort_points_device(ctypes.byref(good), None, None, 4, None) == capi.ERR_ARG
    assert L.mdcu_undistort_points_device(ctypes.byref(good), None, None, -1, None) == capi.ERR_ARG
    assert L.mdcu_undistort_points_host(0, ctypes.byref(good), None, None, 0) == capi.OK  # n = 0: a no-op before any device is looked for
    assert L.mdcu_undistort_points_device(ctypes.byref(good), None, None, 0, None) == capi.OK
    assert L.mdcu_inverse_remap_device(ctypes.byref(good), None, None, None, None) == capi.ERR_ARG
    assert bits_equal(x, x0) and bits_equal(y, y0)
    if not torch.cuda.is_available():
        with pytest.raises(capi.MdcError) as e:
            capi.LensInverse(good).undistort_points_host(x, y)
        assert e.value.code == capi.ERR_NO_DEVICE
        assert bits_equal(x, x0) and bits_equal(y, y0)


CHILD = r"""
import os, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
from mono_dataset_code_amd import capi
import lens_restatement as R
import lens_inverse_restatement as V
fov = capi.UndistorterFOV(sys.argv[2])
assert fov.is_valid()
lines = open(sys.argv[2]).read().splitlines()
q = V.inverse_problem(R.parse(lines)) if lines[0][0].isalpha() else V.fov_problem(lines)
n = 70000
rng = np.random.default_rng(5)
x = rng.uniform(-20, q["in_w"] + 20, n).astype(np.float32)
y = rng.uniform(-20, q["in_h"] + 20, n).astype(np.float32)
for _ in range(2):  # two bulk calls, one message
    gx, gy = x.copy(), y.copy()
    fov.undistort_coordinates(gx, gy)
    wx, wy = V.undistort(q["kind"], q["cam"], q["rect"], x, y)
    nan = np.isnan(wx)
    assert np.array_equal(nan, np.isnan(gx)) and np.array_equal(np.isnan(wy), np.isnan(gy)) and not nan.all()
    assert np.array_equal(gx[~nan].view(np.uint32), wx[~nan].view(np.uint32)) and np.array_equal(gy[~nan].view(np.uint32), wy[~nan].view(np.uint32))
print("child ok")
"""


@pytest.mark.parametrize("name", ["barrel_crop", "fisheye_explicit", "fov_small"])
def test_bulk_undistort_without_the_library_runs_the_host_loop(name, tmp_path):
    """MDC_LIB_LENSINV pointing nowhere, n above the threshold: the host loop's bits, and one message (a child process: the library
    is looked for once per process)"""
    cam = LP.write_camera(tmp_path, LP.PROBLEMS.get(name) or V.SMALL_FOV)
    env = dict(os.environ, MDC_LIB_LENSINV=str(tmp_path / "no_such_library.so"))
    env.pop("MDC_UNDISTORT_GPU_MIN", None)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, cam], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stderr[-2000:]
    said = [l for l in r.stderr.splitlines() if "undistortCoordinates" in l and "computed on the host" in l]
    assert len(said) == 1 and "libmdc_lensinv.so could not be loaded" in said[0], r.stderr[-2000:]
