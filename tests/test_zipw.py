"""The device ZIP writer on the GPU (include/mdc_zipw.h, capi.crc32_device / capi.ZipWriter, bin/rectifyDataset): the checksum
kernel against zlib.crc32 at every boundary of its own decomposition, alignment and index width; the segment, the records and whole
archives byte for byte against tests/zipw_restatement.py and through zipfile; the program's output folder as a dataset."""
import io
import os
import subprocess
import zipfile
import zlib

import numpy as np
import pytest

import zipw_restatement as Z

pytestmark = pytest.mark.gpu
PATTERN = 0xA5


def torch_():
    import torch

    return torch


# ------------------------------------------------------------------------------------------------ the checksum kernel

N_CONTENT_EXTRA = 15  # 3 sizes x (zeros, 0xFF, random behind 1 / 17 / 4097 zero bytes)
_cases = {}


def boundary_files():
    """The files of the checksum tests, computed once with their zlib.crc32: random bytes of sizes 0..70, of every boundary of the
    kernel's decomposition at -1, 0, +1 (the 16-byte word, a wave's span, a lane's stride = a workgroup's span, and the places where
    a file's parts meet when each part takes one row and when it takes two), one file of three rows per part, and the other contents.
    The geometry is asked of the library (mdcz_crc_geometry) for the slot size and file count the test then uses."""
    if "files" in _cases:
        return _cases["files"]
    from mono_dataset_code_amd import capi

    rng = np.random.default_rng(20)
    word, lane_stride, wave_span, wg_span, _ = capi.crc32_geometry(0, 1)
    assert (word, wave_span) == (16, 64 * 16) and lane_stride == wg_span and wg_span % wave_span == 0

    def sizes_for(parts):
        s = list(range(71))
        split = [wg_span * k for k in (1, 2, parts - 1, parts, parts + 1, 2 * parts - 2, 2 * parts)]  # where parts meet: 1 and 2 rows each
        for b in [word, wave_span, wg_span] + split:
            s += [b - 1, b, b + 1]
        s.append(3 * parts * wg_span + 5 * wave_span + 7)  # several workgroups' worth, each several rows
        return s

    parts, slot = 4, 0
    for _ in range(8):  # the parts depend on the slot size, the sizes on the parts: settle
        sizes = sizes_for(parts)
        nfiles = len(sizes) + N_CONTENT_EXTRA
        slot = max(sizes) + 4097 + 32
        now = capi.crc32_geometry(slot, nfiles)[4]
        if now == parts:
            break
        parts = now
    assert capi.crc32_geometry(slot, nfiles)[4] == parts and parts >= 3 and max(sizes) < 64 << 20, (parts, slot)
    files = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in sizes]
    for n in (70, wg_span + 17, 2 * parts * wg_span + 33):
        files += [bytes(n), b"\xff" * n] + [bytes(z) + rng.integers(1, 256, n, dtype=np.uint8).tobytes() for z in (1, 17, 4097)]
    assert len(files) == nfiles and max(len(f) for f in files) <= slot
    _cases["files"] = (files, [zlib.crc32(f) for f in files], slot, parts)
    return _cases["files"]


def device_crc(files, slot, base_offset=0, variant=0, stream=None):
    """files laid out slot bytes apart from base_offset of a pattern-filled device array -> the kernel's CRCs"""
    from mono_dataset_code_amd import capi

    torch = torch_()
    n = len(files)
    host = np.full(base_offset + n * slot + 64, PATTERN, np.uint8)
    for i, f in enumerate(files):
        host[base_offset + i * slot:base_offset + i * slot + len(f)] = np.frombuffer(f, np.uint8)
    d_data = torch.from_numpy(host).to("cuda:0")
    assert d_data.data_ptr() % 256 == 0
    d_sizes = torch.tensor([len(f) for f in files], dtype=torch.int32, device="cuda:0")
    d_crc = torch.full((n + 4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    capi.crc32_device(d_data.data_ptr() + base_offset, slot, d_sizes.data_ptr(), n, d_crc.data_ptr(), stream=stream, variant=variant)
    torch.cuda.synchronize()
    got = d_crc.cpu().numpy().view(np.uint32)
    assert (got[n:] == 0x5A5A5A5A).all()
    assert (d_data.cpu().numpy() == host).all(), "the input was written to"
    return got[:n].tolist()


@pytest.mark.parametrize("variant", [0, 1], ids=["tables", "shift_xor"])
def test_crc32_at_every_boundary_in_one_launch(variant):
    files, want, slot, parts = boundary_files()
    got = device_crc(files, slot, variant=variant)
    bad = [(i, len(files[i]), hex(got[i]), hex(want[i])) for i in range(len(files)) if got[i] != want[i]]
    assert not bad, (parts, bad[:10])
    assert got[0] == 0  # the empty file


def test_crc32_odd_slots_and_every_base_alignment():
    files, want, slot, _ = boundary_files()
    odd = slot | 1
    for k in range(1, 16):
        got = device_crc(files, odd + 2 * (k % 3), base_offset=k)
        bad = [(i, len(files[i])) for i in range(len(files)) if got[i] != want[i]]
        assert not bad, (k, bad[:10])


def test_crc32_of_more_than_65535_files():
    rng = np.random.default_rng(21)
    sizes = rng.integers(0, 41, 70000)
    blob = rng.integers(0, 256, 70000 * 40, dtype=np.uint8)
    files = [blob[i * 40:i * 40 + sizes[i]].tobytes() for i in range(70000)]
    assert device_crc(files, 40) == [zlib.crc32(f) for f in files]


@pytest.fixture(scope="module")
def two_gib():
    """2^31 + 16 + 8192 random bytes on the device, shared by the two index-width cases"""
    torch = torch_()
    n = (1 << 31) + 16 + 8192
    g = torch.Generator(device="cuda:0")
    g.manual_seed(22)
    d = torch.randint(-(1 << 62), 1 << 62, (n // 8,), dtype=torch.int64, device="cuda:0", generator=g).view(torch.uint8)
    assert d.numel() == n
    yield d
    del d
    torch.cuda.empty_cache()


def test_crc32_of_one_file_of_2_to_31_minus_1_bytes(two_gib):
    """the largest size, from an odd address: a head, 2^27 - 1 words over every part, a tail"""
    from mono_dataset_code_amd import capi

    torch = torch_()
    size = (1 << 31) - 1
    d_sizes = torch.tensor([size], dtype=torch.int32, device="cuda:0")
    d_crc = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    capi.crc32_device(two_gib.data_ptr() + 3, 0, d_sizes.data_ptr(), 1, d_crc.data_ptr())
    torch.cuda.synchronize()
    host = two_gib[3:3 + size].cpu().numpy()
    assert int(d_crc.cpu().numpy().view(np.uint32)[0]) == zlib.crc32(host)


def test_crc32_with_a_slot_offset_past_2_to_31(two_gib):
    """two files, slot_bytes = 2^31 + 16: f * slot_bytes does not fit in 32 bits"""
    from mono_dataset_code_amd import capi

    torch = torch_()
    slot, sizes = (1 << 31) + 16, [5001, 3003]
    d_sizes = torch.tensor(sizes, dtype=torch.int32, device="cuda:0")
    d_crc = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    capi.crc32_device(two_gib.data_ptr(), slot, d_sizes.data_ptr(), 2, d_crc.data_ptr())
    torch.cuda.synchronize()
    want = [zlib.crc32(two_gib[f * slot:f * slot + sizes[f]].cpu().numpy()) for f in range(2)]
    assert d_crc.cpu().numpy().view(np.uint32).tolist() == want


# ------------------------------------------------------------------------------------------------ the segment


def to_device(files, slot):
    torch = torch_()
    host = np.full(len(files) * slot + 64, PATTERN, np.uint8)
    for i, f in enumerate(files):
        host[i * slot:i * slot + len(f)] = np.frombuffer(f, np.uint8)
    return torch.from_numpy(host).to("cuda:0"), torch.tensor([len(f) for f in files], dtype=torch.int32, device="cuda:0")


def device_segment(files, first_index, suffix, valid, capacity=None, slot=None, shift=0):
    """-> (the segment's bytes, the records as tuples); checks that nothing at or past the segment's length is written.
    shift: the segment starts that many bytes into its array, so that the 16-byte stores of the gather meet every alignment."""
    from mono_dataset_code_amd import capi

    torch = torch_()
    L = capi.zipw_lib()
    n = len(files)
    slot = slot if slot is not None else max([len(f) for f in files] + [1]) + 3
    d_data, d_sizes = to_device(files, slot)
    bound = L.mdcz_segment_bound(n, sum(len(f) for f in files), 19 + len(suffix))
    assert bound == Z.segment_bound(n, sum(len(f) for f in files), 19 + len(suffix))
    d_seg = torch.full((shift + bound + 4096,), PATTERN, dtype=torch.uint8, device="cuda:0")
    d_rec = torch.full(((n + 1) * 2 + 4,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device="cuda:0")
    d_valid = None if valid is None else torch.tensor(valid, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    rc = L.mdcz_segment_device(d_data.data_ptr(), slot, d_sizes.data_ptr(), d_valid.data_ptr() if d_valid is not None else None, n, first_index, suffix,
                               d_seg.data_ptr() + shift, bound if capacity is None else capacity, d_rec.data_ptr(), None)
    assert rc == 0, L.mdcz_last_error()
    torch.cuda.synchronize()
    rec_raw = d_rec.cpu().numpy()
    assert (rec_raw[(n + 1) * 2:] == -0x5A5A5A5A5A5A5A5B).all()
    rec = rec_raw[:(n + 1) * 2].view(capi.ZIPW_RECORD)
    seg = d_seg.cpu().numpy()
    total = int(rec[n]["offset"])
    assert (seg[:shift] == PATTERN).all()
    written = total if capacity is None or total <= capacity else 0
    assert (seg[shift + written:] == PATTERN).all(), "written at or past the segment's end"
    return seg[shift:shift + written].tobytes(), [(int(r["offset"]), int(r["crc"]), int(r["size"])) for r in rec]


def mixed_files(seed, sizes):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in sizes]


SEGMENT_SIZES = [0, 1, 15, 16, 17, 0, 31, 4095, 4096, 4097, 70001, 0, 33, 8193, 2]


@pytest.mark.parametrize("case", ["all", "holes", "names_of_5_and_6_digits", "suffix_of_15_bytes", "shifted"])
def test_segment_and_records_equal_the_restatement(case):
    files, first, suffix, valid, shifts = mixed_files(30, SEGMENT_SIZES), 0, b".jpg", None, (0,)
    if case == "holes":  # the first, a middle and the last position left out
        valid = [0 if i in (0, 7, len(files) - 1) else 1 for i in range(len(files))]
        first = 41
    elif case == "names_of_5_and_6_digits":
        files, first = mixed_files(31, [100, 0, 5000, 77]), 99998
    elif case == "suffix_of_15_bytes":
        suffix = b".fifteen_bytes_"
        assert len(suffix) == 15
    elif case == "shifted":
        shifts = range(1, 16)
    for shift in shifts:
        want_seg, want_rec = Z.segment(files, first, suffix, valid)
        got_seg, got_rec = device_segment(files, first, suffix, valid, shift=shift)
        assert got_rec == want_rec
        assert got_seg == want_seg, [i for i in range(min(len(got_seg), len(want_seg))) if got_seg[i] != want_seg[i]][:8]
    if case == "names_of_5_and_6_digits":
        assert [want_seg[r[0] + 30:r[0] + 30 + 6 + 4 - (i < 2)] for i, r in enumerate(want_rec[:4])] == [b"99998.jpg", b"99999.jpg", b"100000.jpg", b"100001.jpg"]


def test_segment_larger_than_its_capacity_is_not_written():
    files = mixed_files(32, [100, 200, 300])
    want_seg, want_rec = Z.segment(files, 0, b".jpg", None)
    got_seg, got_rec = device_segment(files, 0, b".jpg", None, capacity=len(want_seg) - 1)
    assert got_seg == b"" and got_rec == want_rec


# ------------------------------------------------------------------------------------------------ the writer


def check_archive(path, batches):
    """the file == the restatement's archive; zipfile gives the names in order and every member's bytes"""
    data = open(path, "rb").read()
    want = Z.archive(batches)
    assert len(data) == len(want) and data == want
    names, members = [], []
    for files, first, suffix, valid in batches:
        for f, b in enumerate(files):
            if valid is None or valid[f]:
                names.append(Z.name_of(first + f, suffix).decode())
                members.append(b)
    with zipfile.ZipFile(path) as z:
        assert z.namelist() == names
        assert z.testzip() is None
        assert [z.read(n) for n in names] == members


def test_two_writers_three_appends_each_on_one_stream(tmp_path):
    from mono_dataset_code_amd import capi

    torch = torch_()
    stream = torch.cuda.Stream(device="cuda:0")
    a_batches = [(mixed_files(40, [0, 5, 70000, 33]), 0, b".jpg", None),
                 (mixed_files(41, [4096] * 9 + [1]), 4, b".jpg", [1, 1, 0, 1, 1, 1, 1, 0, 1, 1]),
                 (mixed_files(42, [123456]), 14, b".jpg", None)]
    b_batches = [(mixed_files(43, [17, 0]), 99999, b".bin", None), (mixed_files(44, [9000, 1, 2, 3, 4]), 0, b".dat", [0, 1, 1, 1, 0]),
                 (mixed_files(45, [64]), 5, b".bin", None)]
    pa, pb = str(tmp_path / "a.zip"), str(tmp_path / "b.zip")
    wa, wb = capi.ZipWriter(pa, device=0), capi.ZipWriter(pb, device=0)
    keep = []
    for batch_a, batch_b in zip(a_batches, b_batches):
        for w, (files, first, suffix, valid) in ((wa, batch_a), (wb, batch_b)):
            slot = max(len(f) for f in files) + 5
            d_data, d_sizes = to_device(files, slot)
            keep.append((d_data, d_sizes))
            torch.cuda.synchronize()
            w.append(d_data.data_ptr(), slot, d_sizes.data_ptr(), len(files), first_index=first, suffix=suffix, valid=valid, stream=stream.cuda_stream)
    size_a, size_b = wa.close(), wb.close()
    assert (size_a, size_b) == (os.path.getsize(pa), os.path.getsize(pb))
    check_archive(pa, a_batches)
    check_archive(pb, b_batches)


def test_archive_of_70000_entries_opens_through_zip64(tmp_path):
    from mono_dataset_code_amd import capi

    rng = np.random.default_rng(46)
    sizes = rng.integers(0, 41, 70000)
    blob = rng.integers(0, 256, 70000 * 40, dtype=np.uint8)
    files = [blob[i * 40:i * 40 + sizes[i]].tobytes() for i in range(70000)]
    d_data, d_sizes = to_device(files, 40)
    path = str(tmp_path / "many.zip")
    w = capi.ZipWriter(path, device=0)
    w.append(d_data.data_ptr(), 40, d_sizes.data_ptr(), 70000, first_index=0, suffix=".jpg")
    assert w.close() == os.path.getsize(path)
    data = open(path, "rb").read()
    assert data == Z.archive([(files, 0, b".jpg", None)])
    assert b"PK\6\6" in data[-120:] and b"PK\6\7" in data[-60:]
    with zipfile.ZipFile(path) as z:
        assert len(z.namelist()) == 70000 and z.namelist()[69999] == "69999.jpg"
        assert z.read("00000.jpg") == files[0] and z.read("65536.jpg") == files[65536] and z.read("69999.jpg") == files[69999]


def test_batch_larger_than_the_staging_cap_is_split_inside(tmp_path):
    """a staging cap of 64 KiB against a batch of 400 KB with one file larger than the cap: several segments, the same bytes"""
    from mono_dataset_code_amd import capi

    sizes = [30000, 30000, 30000, 100000, 0, 5, 65000, 600, 70000, 40000, 20000, 14000]
    files = mixed_files(47, sizes)
    valid = [1] * len(files)
    valid[2] = valid[11] = 0
    slot = 100001
    d_data, d_sizes = to_device(files, slot)
    for cap, name in ((64 << 10, "split.zip"), (0, "whole.zip")):
        path = str(tmp_path / name)
        w = capi.ZipWriter(path, device=0, staging_cap=cap)
        w.append(d_data.data_ptr(), slot, d_sizes.data_ptr(), len(files), first_index=7, suffix=".jpg", valid=valid)
        w.close()
        check_archive(path, [(files, 7, b".jpg", valid)])
    assert open(str(tmp_path / "split.zip"), "rb").read() == open(str(tmp_path / "whole.zip"), "rb").read()


# ------------------------------------------------------------------------------------------------ the program

CAMERA = ("0.349153 0.436593 0.493140 0.499021 0.933271", "320 256", "crop", "192 144")


def ulps(a, b):
    a, b = np.float32(a), np.float32(b)
    return abs(float(a) - float(b)) / float(np.spacing(max(abs(a), abs(b), np.float32(1e-30))))


def test_rectify_dataset_writes_a_dataset(tmp_path):
    """bin/rectifyDataset on a synthetic sequence of 7 frames whose middle frame's file is truncated: images.zip holds the files
    bin/playDataset saves (tests/test_jenc.py pins those to PIL), the unreadable frame is absent from the archive and from times.txt,
    camera.txt is the rectified pinhole, and the folder opens as a dataset of 6 frames with the source's times and (within 4 ulp:
    + 0.5, / w, %.9g (exact), * w, - 0.5 round four times) its rectified K."""
    from PIL import Image

    from mono_dataset_code_amd import build, capi, synth

    d, out, loose = str(tmp_path / "seq"), str(tmp_path / "rect" / "sub"), tmp_path / "loose"
    loose.mkdir()
    synth.write_sequence_calibration(d, CAMERA, vignette_bits=16, n_times=7)
    os.makedirs(os.path.join(d, "images"))
    for i in range(7):
        f = synth.noise_frames(11, 1, 320 * 256)[0] if i == 1 else synth.smooth_frame(320, 256, 0.7 + i, blobs=i % 2 == 0)
        synth.write_png_gray(os.path.join(d, "images", "%05d.png" % i), f.reshape(256, 320))
    middle = os.path.join(d, "images", "00003.png")
    whole = open(middle, "rb").read()
    with open(middle, "wb") as f:
        f.write(whole[:len(whole) // 2])
    kept = [0, 1, 2, 4, 5, 6]
    r = subprocess.run([build.RECTIFY_DATASET, d, out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "frame 3 could not be read: left out" in r.stdout
    assert len([l for l in r.stdout.splitlines() if "not exported" in l]) == 1 and "vignette.png is not exported" in r.stdout
    assert sorted(os.listdir(out)) == ["camera.txt", "images.zip", "pcalib.txt", "times.txt"]
    p = subprocess.run([build.PLAY_DATASET, d, "x"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120, cwd=str(loose))
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    assert sorted(os.listdir(str(loose))) == ["%05d.jpg" % i for i in kept]
    with zipfile.ZipFile(os.path.join(out, "images.zip")) as z:
        assert z.testzip() is None
        assert z.namelist() == ["%05d.jpg" % i for i in kept]
        members = [z.read(n) for n in z.namelist()]
    for i, m in zip(kept, members):
        assert m == (loose / ("%05d.jpg" % i)).read_bytes(), i
    src_times = open(os.path.join(d, "times.txt")).read().splitlines()
    assert open(os.path.join(out, "times.txt")).read().splitlines() == [src_times[i] for i in kept]
    assert open(os.path.join(out, "pcalib.txt"), "rb").read() == open(os.path.join(d, "pcalib.txt"), "rb").read()
    src_fov = capi.UndistorterFOV(os.path.join(d, "camera.txt"))
    K = src_fov.intrinsics()["K_rect"]
    cam = open(os.path.join(out, "camera.txt")).read().splitlines()
    assert cam[1:] == ["192 144", "crop", "192 144"] and len(cam) == 4
    fw, fh, half = np.float32(192), np.float32(144), np.float32(0.5)
    assert cam[0] == "%.9g %.9g %.9g %.9g 0" % (K[0, 0] / fw, K[1, 1] / fh, (K[0, 2] + half) / fw, (K[1, 2] + half) / fh)
    out_fov = capi.UndistorterFOV(os.path.join(out, "camera.txt"))
    assert out_fov.is_valid() and out_fov.dims() == (192, 144, 192, 144) and out_fov.intrinsics()["omega"] == 0
    K2 = out_fov.intrinsics()["K_rect"]
    for rr in range(3):
        for cc in range(3):
            assert ulps(K[rr, cc], K2[rr, cc]) <= 4, (rr, cc, K[rr, cc], K2[rr, cc])
    src_fov.close()
    out_fov.close()
    src, reader = capi.DatasetReader(d), capi.DatasetReader(out)
    assert len(src) == 7 and len(reader) == 6
    assert (reader.in_w, reader.in_h, reader.out_w, reader.out_h) == (192, 144, 192, 144)
    for j, i in enumerate(kept):
        assert reader.timestamp(j) == src.timestamp(i) and reader.exposure(j) == src.exposure(i) and reader.exposure(j) > 0
        raw = reader.get_raw(j)
        assert raw is not None, reader.last_error()
        assert np.array_equal(raw, np.array(Image.open(io.BytesIO(members[j])))), i
    src.close()
    reader.close()
