#!/usr/bin/env python3
"""Generates the corpus of tests/test_codecs_corpus_cpu.py.

  python tests/golden/codecs/make_codecs.py --fixtures   writes the image files (needs PIL; its libjpeg / libpng decide the bytes,
                                                         which is why the files are committed and not made at test time)
  python tests/golden/codecs/make_codecs.py --record     runs the decoders of THIS checkout's build over the corpus (files, their
                                                         mutations, the hand-made files) and writes expected.npz

expected.npz was recorded from the decoders before their shared parts were merged (one marker parser, one bit reader, one PNG
unfilter); re-record only for a change that is meant to alter what a decoder accepts or returns, and say so.
  --dump DIR  additionally writes DIR/cases.bin ([u32 length][bytes] per case) and DIR/results.txt (one line per case and entry
              point with a CRC-32 of the output) for a stand-alone C++ driver to reproduce under other compiler flags."""
import os
import struct
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_codecs_corpus_cpu as corpus  # noqa: E402


def fixtures():
    import io

    from PIL import Image

    from test_reader_cpu import _png_chunks, interlaced_png, png_bytes, raw_png, textured

    def jpeg(img, **kw):
        b = io.BytesIO()
        Image.fromarray(img).save(b, "JPEG", **kw)
        return b.getvalue()

    def jpeg_411(planes, quality):
        """Luma sampled 4 x 1, chroma 1 x 1 (PIL writes no such file): tests/jenc_restatement.py's baseline encoder, its blocks put
        in MCU order (Y Y Y Y Cb Cr), one quantisation table and one Huffman table pair for all three components."""
        import jenc_restatement as je

        h, w = planes.shape[:2]
        mx, my = (w + 31) // 32, (h + 7) // 8
        padded = np.pad(planes, ((0, my * 8 - h), (0, mx * 32 - w), (0, 0)), mode="edge")
        y = je.coefficients(padded[..., 0], quality).reshape(my, mx, 4, 64)
        c = [je.coefficients(padded[..., k].reshape(my * 8, mx * 8, 4).mean(-1).astype(np.uint8), quality).reshape(my, mx, 1, 64) for k in (1, 2)]
        zz = np.concatenate([y] + c, 2).reshape(-1, 64).copy()
        comp = np.tile([0, 0, 0, 0, 1, 2], my * mx)
        for k in range(3):  # scan_bytes() codes each DC against the block before it: make that difference the component's own
            dc = zz[comp == k, 0]
            zz[comp == k, 0] = dc - np.concatenate([[0], dc[:-1]])
        zz[:, 0] = np.cumsum(zz[:, 0])
        head = je.header(w, h, quality)
        sof = head.index(b"\xff\xc0")
        dht = head.index(b"\xff\xc4")
        return (head[:sof] + b"\xff\xc0\x00\x11\x08" + bytes([h >> 8, h & 255, w >> 8, w & 255]) + b"\x03\x01\x41\x00\x02\x11\x00\x03\x11\x00" +
                head[dht:head.index(b"\xff\xda")] + b"\xff\xda\x00\x0c\x03\x01\x00\x02\x00\x03\x00\x00\x3f\x00" + je.scan_bytes(zz) + b"\xff\xd9")

    img = textured(40, 48, 11)
    rgb = np.stack([img, np.roll(img, 3, 1), 255 - img], -1)
    odd = textured(23, 17, 12)
    odd_rgb = np.stack([odd, odd[::-1], 255 - odd], -1)
    small = textured(20, 27, 13)  # PNG: a width that is no multiple of 8 (bit depths below 8 end a row inside a byte)
    small_rgb = np.stack([small, np.roll(small, 2, 0), 255 - small], -1)
    rng_state = [99]

    def noise(shape):  # low bytes for the 16-bit files, from the corpus' own generator
        out = np.empty(int(np.prod(shape)), np.uint16)
        for i in range(out.size):
            rng_state[0] = corpus.lcg(rng_state[0])
            out[i] = (rng_state[0] >> 12) & 15
        return out.reshape(shape)

    def packed_gray(a, depth):  # filter type 0, `depth` bits per sample, most significant first
        rows = []
        for r in a >> (8 - depth):
            bits = "".join(format(int(v), "0%db" % depth) for v in r)
            bits += "0" * (-len(bits) % 8)
            rows.append(b"\0" + bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8)))
        return _png_chunks(a.shape[1], a.shape[0], depth, 0, 0, b"".join(rows))

    g16 = (small.astype(np.uint16) << 8) | noise(small.shape)
    rgb16 = (small_rgb.astype(np.uint16) << 8) | noise(small_rgb.shape)
    la = np.stack([small, 255 - small], -1)
    rgba = np.concatenate([small_rgb, (small // 2)[..., None]], -1)
    out = {
        "b_gray.jpg": jpeg(img, quality=85),
        "b_444.jpg": jpeg(rgb, quality=85, subsampling=0),
        "b_422.jpg": jpeg(rgb, quality=85, subsampling=1),
        "b_420.jpg": jpeg(rgb, quality=85, subsampling=2),
        "b_411.jpg": jpeg_411(rgb, 85),
        "b_opt.jpg": jpeg(img, quality=60, optimize=True),
        "b_rst_blocks.jpg": jpeg(img, quality=80, restart_marker_blocks=5),
        "b_rst_rows.jpg": jpeg(rgb, quality=80, subsampling=2, restart_marker_rows=1),
        "b_odd.jpg": jpeg(odd, quality=90),
        "b_odd_420.jpg": jpeg(odd_rgb, quality=75, subsampling=2),
        "b_rgb_adobe.jpg": jpeg(rgb, quality=85, keep_rgb=True),
        "p_gray.jpg": jpeg(img, quality=85, progressive=True),
        "p_420.jpg": jpeg(rgb, quality=80, progressive=True, subsampling=2),
        "p_rst.jpg": jpeg(rgb, quality=80, progressive=True, subsampling=2, restart_marker_blocks=4),
        "g1.png": png_bytes(Image.fromarray(((small > 127) * 255).astype(np.uint8)).convert("1")),
        "g2.png": packed_gray(small, 2),
        "g4.png": packed_gray(small, 4),
        "g8.png": png_bytes(small),
        "g16.png": raw_png(g16),
        "ga.png": png_bytes(Image.fromarray(la, "LA")),
        "rgb8.png": png_bytes(small_rgb),
        "rgb16.png": raw_png(rgb16),
        "rgba.png": png_bytes(Image.fromarray(rgba, "RGBA")),
        "pal4.png": png_bytes(Image.fromarray(small_rgb).quantize(colors=13), bits=4),
        "pal8.png": png_bytes(Image.fromarray(small_rgb).quantize(colors=200)),
        "lace_g8.png": interlaced_png(small),
        "lace_rgb16.png": interlaced_png(rgb16),
        "g8.pgm": b"P5\n# corpus\n27 20\n255\n" + small.tobytes(),
        "g16.pgm": b"P5\n27 20\n65535\n" + g16.astype(">u2").tobytes(),
    }
    assert sorted(out) == sorted(corpus.FILES)
    d = out["b_411.jpg"]
    sof = corpus.segment(d, 0xC0)
    assert d[sof + 11] == 0x41, "luma sampling of the 4:1:1 file"
    assert out["b_rgb_adobe.jpg"].find(b"Adobe") > 0 and b"\xff\xc2" in out["p_rst.jpg"] and b"\xff\xdd" in out["p_rst.jpg"]
    assert out["g2.png"][24] == 2 and out["g4.png"][24] == 4 and out["pal4.png"][24:26] == b"\x04\x03" and out["lace_rgb16.png"][24:29] == b"\x10\x02\0\0\x01"
    for name, data in out.items():
        assert len(data) <= 8192, (name, len(data))
        with open(os.path.join(HERE, name), "wb") as f:
            f.write(data)
        print("%-18s %5d bytes" % (name, len(data)))


def record(dump=None):
    groups = corpus.groups()
    cases = [(g + ":" + label, data) for g, c in groups for label, data in c]
    results = [corpus.run_case(data) for _, data in cases]
    messages = sorted({r[4] for res in results for r in res if not r[0]})
    assert len(messages) < 255
    n = len(cases)
    code = np.zeros((n, 3), np.uint8)  # 0 = decoded, k = refused with messages[k - 1]
    w, h = np.zeros((n, 3), np.uint32), np.zeros((n, 3), np.uint32)
    dig = np.zeros((n, 3), np.uint64)
    for i, res in enumerate(results):
        for e, (ok, ww, hh, dd, msg) in enumerate(res):
            if ok:
                w[i, e], h[i, e], dig[i, e] = ww, hh, dd
            else:
                code[i, e] = 1 + messages.index(msg)
    path = os.path.join(HERE, "expected.npz")
    np.savez_compressed(path, groups=np.array([g for g, _ in groups]), group_sizes=np.array([len(c) for _, c in groups], np.int32),
                        messages=np.array(messages), code=code, w=w, h=h, digest=dig)
    print("%d cases, %d decoded results, %d messages, %d bytes" % (n, int((code == 0).sum()), len(messages), os.path.getsize(path)))
    assert os.path.getsize(path) <= 64 * 1024
    if dump:
        dump_for_driver(dump, cases)


def dump_for_driver(folder, cases):
    """The same calls with a CRC-32 in place of the digest, as text, and the cases as one file: a C++ program that makes these calls
    on the host sources (whatever its compiler flags) must print results.txt."""
    from mono_dataset_code_amd import capi

    with open(os.path.join(folder, "cases.bin"), "wb") as f:
        for _, data in cases:
            f.write(struct.pack("<I", len(data)) + data)
    rec_bytes, pitch, _ = capi.jpeg_record_bytes(corpus.MAX_SIDE, corpus.MAX_SIDE)
    with open(os.path.join(folder, "results.txt"), "w") as f:
        for i, (_, data) in enumerate(cases):
            try:
                a = capi.decode_gray8(data)
                f.write("%d gray8 1 %d %d %08x\n" % (i, a.shape[1], a.shape[0], zlib.crc32(a.tobytes())))
            except ValueError as e:
                f.write("%d gray8 0 %s\n" % (i, e))
            rec = np.zeros(rec_bytes, np.uint8)
            try:
                ww, hh, bw, rows = capi.decode_jpeg_record(data, rec, pitch)
                f.write("%d record 1 %d %d %08x\n" % (i, ww, hh, zlib.crc32(rec[: 128 + bw * rows * 128].tobytes())))
            except ValueError as e:
                f.write("%d record 0 %s\n" % (i, e))
            stream = np.zeros(corpus.STREAM_CAP, np.uint8)
            try:
                used, ww, hh = capi.jpeg_stream(data, stream)
                f.write("%d stream 1 %d %d %08x\n" % (i, ww, hh, zlib.crc32(stream[:used].tobytes())))
            except ValueError as e:
                f.write("%d stream 0 %s\n" % (i, e))


if __name__ == "__main__":
    if "--fixtures" in sys.argv:
        fixtures()
    if "--record" in sys.argv:
        record(sys.argv[sys.argv.index("--dump") + 1] if "--dump" in sys.argv else None)
