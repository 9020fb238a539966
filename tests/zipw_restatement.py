"""include/mdc_zipw.h restated with struct and zlib: the segment (local headers, names, bytes), its records, the central directory
with the ZIP64 pieces, and the whole archive, from a list of byte strings.  The byte-for-byte oracle of tests/test_zipw_cpu.py and
tests/test_zipw.py; itself checked against zipfile there."""
import struct
import zlib

DOS_TIME, DOS_DATE = 0, 0x0021  # 1980-01-01 00:00:00
MADE_BY = 20 | (3 << 8)  # 2.0, Unix
FAR = 0xFFFFFFFF
NAME_STRIDE = 40


def name_of(index, suffix=b".jpg"):
    return b"%05d" % index + suffix


def local_header(name, data=None, crc=None, size=None):
    crc = zlib.crc32(data) if crc is None else crc
    size = len(data) if size is None else size
    return struct.pack("<4sHHHHHIIIHH", b"PK\3\4", 20, 0, 0, DOS_TIME, DOS_DATE, crc, size, size, len(name), 0) + name


def segment(files, first_index=0, suffix=b".jpg", valid=None):
    """-> (bytes, records): records[f] = (offset of file f's header in the segment or -1, crc, size), one more with the length"""
    out, records = bytearray(), []
    for f, data in enumerate(files):
        if valid is not None and not valid[f]:
            records.append((-1, zlib.crc32(data), len(data)))
            continue
        records.append((len(out), zlib.crc32(data), len(data)))
        out += local_header(name_of(first_index + f, suffix), data) + data
    records.append((len(out), 0, 0))
    return bytes(out), records


def segment_bound(nfiles, total_bytes, max_name_len):
    return nfiles * (30 + max_name_len) + total_bytes


def directory(entries, directory_offset):
    """entries: (absolute header offset, crc, size, name) -> the central directory, the ZIP64 end record and locator where the
    format needs them, the end record"""
    out = bytearray()
    for at, crc, size, name in entries:
        far = at >= FAR
        extra = struct.pack("<HHQ", 1, 8, at) if far else b""
        out += struct.pack("<4sHHHHHHIIIHHHHHII", b"PK\1\2", MADE_BY, 45 if far else 20, 0, 0, DOS_TIME, DOS_DATE, crc, size, size, len(name),
                           len(extra), 0, 0, 0, 0, FAR if far else at) + name + extra
    n, size = len(entries), len(out)
    if n > 65534 or directory_offset >= FAR or size >= FAR:
        out += struct.pack("<4sQHHIIQQQQ", b"PK\6\6", 44, MADE_BY, 45, 0, 0, n, n, size, directory_offset)
        out += struct.pack("<4sIQI", b"PK\6\7", 0, directory_offset + size, 1)
    out += struct.pack("<4sHHHHIIH", b"PK\5\6", 0, 0, min(n, 0xFFFF), min(n, 0xFFFF), min(size, FAR), min(directory_offset, FAR), 0)
    return bytes(out)


def archive(batches):
    """batches: (files, first_index, suffix, valid) per append -> the archive's bytes"""
    out, entries = bytearray(), []
    for files, first_index, suffix, valid in batches:
        seg, records = segment(files, first_index, suffix, valid)
        for f, (at, crc, size) in enumerate(records[:-1]):
            if at >= 0:
                entries.append((len(out) + at, crc, size, name_of(first_index + f, suffix)))
        out += seg
    return bytes(out + directory(entries, len(out)))
