"""The device ZIP writer (include/mdc_zipw.h, libmdc_zipw.so) as far as it can be checked without a GPU: header, library and
ctypes table declare the same functions; the library stands alone and leaves the product's build identity untouched; argument
errors are statuses; its kernels compile without scratch, MFMA and atomics; and mdcz_directory, a pure host function, equals the
restatement (tests/zipw_restatement.py) byte for byte and is read back by zipfile, also past 2^32."""
import ctypes
import io
import json
import os
import subprocess
import sys
import zipfile
import zlib

import numpy as np
import pytest

import zipw_restatement as Z
from test_abi import declared, exported, prototypes, signature_mismatches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_is_read_by_zipfile():
    """the oracle itself: names in order, members intact, also with a hole and with 5- and 6-digit names"""
    rng = np.random.default_rng(5)
    files = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (0, 1, 70, 4099)]
    data = Z.archive([(files, 99998, b".jpg", None), (files, 7, b".bin", [1, 0, 1, 1])])
    z = zipfile.ZipFile(io.BytesIO(data))
    assert z.testzip() is None
    assert z.namelist() == ["99998.jpg", "99999.jpg", "100000.jpg", "100001.jpg", "00007.bin", "00009.bin", "00010.bin"]
    assert [z.read(n) for n in z.namelist()] == files + [files[0], files[2], files[3]]
    info = z.getinfo("00009.bin")
    assert info.date_time == (1980, 1, 1, 0, 0, 0) and info.compress_type == zipfile.ZIP_STORED and info.create_system == 3
    assert info.extract_version == 20 and info.create_version == 20 and info.external_attr == 0 and info.flag_bits == 0


def test_header_parses_as_c99_and_cxx(tmp_path):
    src = tmp_path / "zipw_abi.c"
    src.write_text('#include "mdc_zipw.h"\nint main(void){ mdcz_writer* w = 0; mdcz_record r; r.offset = 0; (void)w;'
                   ' return MDCZ_OK + (int)r.offset + (mdcz_segment_bound(1, 1, MDCZ_MAX_SUFFIX) < 0); }\n')
    inc = os.path.join(ROOT, "include")
    for cmd in (["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I" + inc, str(src)],
                ["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", "-I" + inc, str(src)]):
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout


def test_header_library_and_table_are_one_set():
    from mono_dataset_code_amd import build, capi

    names = declared("mdc_zipw.h", "mdcz_")
    assert len(names) >= 10 and {"mdcz_crc32_device", "mdcz_segment_device", "mdcz_directory", "mdcz_append_device"} <= set(names)
    assert exported(build.LIB_ZIPW) == names == sorted(capi.ZIPW_API)
    protos = prototypes("mdc_zipw.h", "mdcz_")
    assert sorted(protos) == names
    assert signature_mismatches(capi.ZIPW_API, protos) == []
    # the check can fail
    wrong = dict(capi.ZIPW_API, mdcz_segment_bound=(ctypes.c_int64, [ctypes.c_int64, ctypes.c_int, ctypes.c_int]))
    assert len(signature_mismatches(wrong, protos)) == 1
    L = capi.zipw_lib()
    assert sorted(vars(L)) == names
    for n, (restype, argtypes) in capi.ZIPW_API.items():
        assert getattr(L, n).restype is restype and list(getattr(L, n).argtypes) == argtypes, n
    assert capi.ZIPW_RECORD.itemsize == 16 and capi.ZIPW_NAME_STRIDE == Z.NAME_STRIDE
    hdr = open(os.path.join(ROOT, "include", "mdc_zipw.h")).read()
    assert "#define MDCZ_NAME_STRIDE %d " % capi.ZIPW_NAME_STRIDE in hdr


def test_library_stands_alone():
    """no product library exports mdcz_ or links libmdc_zipw, and libmdc_zipw.so links no libmdc_*"""
    from mono_dataset_code_amd import build

    for lib in (build.LIB_HIP, build.LIB_HOST, build.LIB_MULTI, build.LIB_BENCH, build.LIB_JENC):
        assert "mdcz_" not in subprocess.run(["nm", "-D", lib], stdout=subprocess.PIPE, text=True, check=True).stdout, lib
        assert "libmdc_zipw" not in subprocess.run(["readelf", "-d", lib], stdout=subprocess.PIPE, text=True, check=True).stdout, lib
    assert "libmdc_" not in subprocess.run(["readelf", "-d", build.LIB_ZIPW], stdout=subprocess.PIPE, text=True, check=True).stdout


def test_product_build_identity_is_unchanged():
    from mono_dataset_code_amd import build

    assert build.code_id() == json.load(open(os.path.join(ROOT, "profiles", "r06_fused_summary.json")))["code_id"]
    deps = set(build.HIP_DEPS) | set(build.HOST_DEPS)
    for f in (build.ZIPW_SOURCE, build.ZIPW_EXPORT_MAP, os.path.join(ROOT, "include", "mdc_zipw.h"), build.RECTIFY_DATASET_SOURCE):
        assert os.path.exists(f) and f not in deps, f


def _err(L):
    return L.mdcz_last_error().decode()


def test_argument_errors_without_a_device(tmp_path):
    """every check below comes before any HIP call: a status and a message, never a fault"""
    from mono_dataset_code_amd import capi

    L = capi.zipw_lib()
    p = ctypes.c_void_p(4096)  # never dereferenced on the host
    assert L.mdcz_crc32_device(None, 16, p, 1, p, None) == -1 and "null" in _err(L)
    assert L.mdcz_crc32_device(p, 16, None, 1, p, None) == -1 and "null" in _err(L)
    assert L.mdcz_crc32_device(p, 16, p, 1, None, None) == -1 and "null" in _err(L)
    assert L.mdcz_crc32_device(p, 16, p, -1, p, None) == -1 and "negative" in _err(L)
    assert L.mdcz_crc32_device(p, -16, p, 1, p, None) == -1 and "slot_bytes" in _err(L)
    assert L.mdcz_crc32_variant_device(2, p, 16, p, 1, p, None) == -1 and "variant" in _err(L)
    seg = lambda nfiles=1, first=0, suffix=b".jpg", d_segment=p, d_records=p, cap=1 << 20: L.mdcz_segment_device(  # noqa: E731
        p, 16, p, None, nfiles, first, suffix, d_segment, cap, d_records, None)
    assert seg(nfiles=-1) == -1 and "negative" in _err(L)
    assert seg(d_segment=None) == -1 and "null" in _err(L)
    assert seg(d_records=None) == -1 and "null" in _err(L)
    assert seg(suffix=None) == -1 and "null" in _err(L)
    assert seg(suffix=b"x" * 16) == -1 and "16 bytes" in _err(L)
    assert seg(suffix=b".jp\x80") == -1 and "ASCII" in _err(L)
    assert seg(first=-1) == -1 and "first_index" in _err(L)
    assert seg(cap=-1) == -1 and "capacity" in _err(L)
    assert L.mdcz_segment_bound(3, 100, 9) == Z.segment_bound(3, 100, 9) == 217
    assert L.mdcz_segment_bound(-1, 0, 9) == -1 and L.mdcz_segment_bound(1, -1, 9) == -1 and L.mdcz_segment_bound(1 << 62, 0, 9) == -1
    # the directory: a capacity below the bound, null arrays, a negative count
    rec = np.zeros(1, capi.ZIPW_RECORD)
    names = np.zeros((1, capi.ZIPW_NAME_STRIDE), np.uint8)
    names[0, :9] = np.frombuffer(b"00000.jpg", np.uint8)
    need = L.mdcz_directory(rec.ctypes.data, 1, names.ctypes.data, 0, 39, None, 0)
    assert need == len(Z.directory([(0, 0, 0, b"00000.jpg")], 39)) == 46 + 9 + 22
    out = np.zeros(need, np.uint8)
    assert L.mdcz_directory(rec.ctypes.data, 1, names.ctypes.data, 0, 39, out.ctypes.data, need - 1) == -3 and "capacity" in _err(L)
    assert not out.any()
    assert L.mdcz_directory(None, 1, names.ctypes.data, 0, 0, None, 0) == -1 and "null" in _err(L)
    assert L.mdcz_directory(rec.ctypes.data, -1, names.ctypes.data, 0, 0, None, 0) == -1 and "negative" in _err(L)
    names[0, :] = 65
    assert L.mdcz_directory(rec.ctypes.data, 1, names.ctypes.data, 0, 0, None, 0) == -1 and "terminated" in _err(L)
    # the writer: an unwritable path, null arguments, and (on an open writer) the batch checks
    h = ctypes.c_void_p()
    bad = os.path.join(str(tmp_path), "no_such_folder", "images.zip")
    assert L.mdcz_open(os.fsencode(bad), 0, 0, ctypes.byref(h)) == -7 and not h.value
    assert "No such file or directory" in _err(L) and "no_such_folder" in _err(L)
    assert L.mdcz_open(None, 0, 0, ctypes.byref(h)) == -1 and L.mdcz_open(b"x", 0, 0, None) == -1
    assert L.mdcz_append_device(None, p, 16, p, None, 1, 0, b".jpg", None) == -1 and "null" in _err(L)
    path = os.path.join(str(tmp_path), "empty.zip")
    assert L.mdcz_open(os.fsencode(path), 0, 0, ctypes.byref(h)) == 0 and h.value
    assert L.mdcz_append_device(h, None, 16, p, None, 1, 0, b".jpg", None) == -1 and "null" in _err(L)
    assert L.mdcz_append_device(h, p, 16, p, None, -1, 0, b".jpg", None) == -1 and "negative" in _err(L)
    assert L.mdcz_append_device(h, p, 16, p, None, 1, 0, b"." + b"j" * 15, None) == -1 and "16 bytes" in _err(L)
    assert L.mdcz_append_device(h, p, 16, p, None, 1, 0, b"\xff", None) == -1 and "ASCII" in _err(L)
    assert L.mdcz_append_device(h, p, 16, p, None, 0, 0, b".jpg", None) == 0  # nothing to do, nothing touched
    assert L.mdcz_close(h) == 22  # an archive without entries is its end record
    assert open(path, "rb").read() == Z.directory([], 0) and zipfile.ZipFile(path).namelist() == []
    assert L.mdcz_close(None) == -1
    L.mdcz_abort(None)
    assert L.mdcz_open(os.fsencode(path), 0, 0, ctypes.byref(h)) == 0
    L.mdcz_abort(h)
    assert not os.path.exists(path)


def test_kernels_have_no_scratch_no_mfma_no_atomics():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_stats

    ks = isa_stats.kernels(isa_stats.device_asm("mdc_zipw.hip"))
    names = sorted(k["pretty"] for k in ks)
    assert names == ["zipw_crc_finish_kernel", "zipw_crc_parts_kernel<0>", "zipw_crc_parts_kernel<1>", "zipw_gather_kernel", "zipw_scan_kernel"], names
    for k in ks:
        assert k["scratch"] == 0, (k["pretty"], k["scratch"])
        assert not any(n.startswith("v_mfma") for n in k["counts"]), k["pretty"]
        assert not any("atomic" in n for n in k["counts"]), (k["pretty"], k["counts"])
        assert k["vgpr"] <= 64, (k["pretty"], k["vgpr"])
    # the loads the design asks for: 16 bytes per lane in the checksum and in the gather
    by = {k["pretty"]: k["counts"] for k in ks}
    assert by["zipw_crc_parts_kernel<0>"].get("global_load_dwordx4", 0) >= 1 and by["zipw_gather_kernel"].get("global_store_dwordx4", 0) >= 1


def _library_directory(entries, directory_offset, base=0):
    from mono_dataset_code_amd import capi

    rec = np.zeros(len(entries), capi.ZIPW_RECORD)
    for i, (at, crc, size, _) in enumerate(entries):
        rec[i] = (at - base if at >= 0 else -1, crc, size)
    return capi.zip_directory(rec, [e[3] for e in entries], segment_base_offset=base, directory_offset=directory_offset)


@pytest.mark.parametrize("n", [0, 1, 65534, 65535])
def test_directory_equals_the_restatement(n):
    """names of 9 and 10 bytes (the entries from 99,998 on); the ZIP64 end record and locator appear with the 65,535th entry"""
    first = 99998 if n == 1 else 99990 if n else 0
    entries, at = [], 0
    for i in range(n):
        name = Z.name_of(first + i)
        size = (i * 7919) % 41
        entries.append((at, zlib.crc32(b"%d" % i), size, name))
        at += 30 + len(name) + size
    if n > 10:
        assert {len(e[3]) for e in entries} == {9, 10}
    want = Z.directory(entries, at)
    got = _library_directory(entries, at)
    assert got == want
    assert (b"PK\6\6" in got[-100:]) == (b"PK\6\7" in got[-50:]) == (n == 65535)
    assert len(got) == sum(46 + len(e[3]) for e in entries) + 22 + (76 if n == 65535 else 0)


def test_directory_skips_left_out_records_and_adds_the_base():
    entries = [(1000, 1, 5, b"00000.jpg"), (-1, 2, 6, b"00001.jpg"), (1044, 3, 7, b"00002.jpg")]
    assert _library_directory(entries, 2000, base=1000) == Z.directory([entries[0], entries[2]], 2000)


FAR_OFFSETS = (0xFFFFFFFE, 0xFFFFFFFF, 0x100000000)


def test_directory_with_64_bit_offsets_equals_the_restatement():
    """entries at 0xFFFFFFFE, 0xFFFFFFFF and 0x100000000: the ZIP64 extra field and version 45 on the last two only"""
    entries = [(at, zlib.crc32(b"%d" % i), 3 + i, Z.name_of(i)) for i, at in enumerate(FAR_OFFSETS)]
    end = FAR_OFFSETS[-1] + 100
    got = _library_directory(entries, end)
    assert got == Z.directory(entries, end)
    assert got.count(b"\x01\x00\x08\x00") == 2 and got.count(b"PK\1\2\x14\x03\x2d\x00") == 2 and got.count(b"PK\1\2\x14\x03\x14\x00") == 1
    assert b"PK\6\6" in got  # the directory's own offset does not fit either


@pytest.mark.parametrize("far", FAR_OFFSETS, ids=hex)
def test_sparse_archive_past_4g_is_read_by_zipfile(tmp_path, far):
    """A sparse file with one entry at 0 and one whose header starts at `far` (two headers cannot start one byte apart, so each of the
    three offsets gets a file of its own): the restatement's local headers and payloads at their places, the library's directory
    behind them; zipfile reads every member back."""
    path = str(tmp_path / "far.zip")
    payload = [b"first entry", bytes(range(256)) * 3]
    entries = [(0, zlib.crc32(payload[0]), len(payload[0]), Z.name_of(0)), (far, zlib.crc32(payload[1]), len(payload[1]), Z.name_of(123456))]
    end = far + 30 + len(entries[1][3]) + len(payload[1])
    with open(path, "wb") as f:
        for (at, _, _, name), data in zip(entries, payload):
            f.seek(at)
            f.write(Z.local_header(name, data) + data)
        assert f.tell() == end
        f.write(_library_directory(entries, end))
    if os.stat(path).st_blocks * 512 > 64 << 20:
        os.unlink(path)
        pytest.skip("the file system makes no holes: a 4 GiB archive would be written out")
    with zipfile.ZipFile(path) as z:
        assert z.testzip() is None
        assert z.namelist() == ["00000.jpg", "123456.jpg"]
        assert [z.read(n) for n in z.namelist()] == payload
        assert z.getinfo("123456.jpg").header_offset == far
    os.unlink(path)


def test_program_is_built_and_prints_its_usage(tmp_path):
    """bin/rectifyDataset with one argument: a usage line, a non-zero status, nothing created (no frame is touched: no GPU needed)"""
    from mono_dataset_code_amd import build

    assert os.access(build.RECTIFY_DATASET, os.X_OK)
    needed = subprocess.run(["readelf", "-d", build.RECTIFY_DATASET], stdout=subprocess.PIPE, text=True, check=True).stdout
    for lib in ("libmdc_host.so", "libmdc_hip.so", "libmdc_jenc.so", "libmdc_zipw.so"):
        assert lib in needed, lib
    r = subprocess.run([build.RECTIFY_DATASET, str(tmp_path / "seq")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60, cwd=str(tmp_path))
    assert r.returncode != 0 and r.stdout == ""
    assert r.stderr.startswith("usage: ") and "<dataset folder> <output folder> [quality=95]" in r.stderr and len(r.stderr.splitlines()) == 1
    assert os.listdir(str(tmp_path)) == []
