"""A NumPy restatement of the baseline JPEG encoder that include/mdc_jenc.h specifies (tests/test_jenc_cpu.py pins it to
libjpeg-turbo through PIL, byte for byte): float -> 8 bit as cv::Mat::convertTo, edge extension, level shift, the integer
forward DCT of jfdctint.c, the quantisation of jcdctmgr.c, Huffman coding with the Annex K luminance tables, byte
stuffing, and the JFIF header.  Nothing here is fast; it is the specification in executable form, and the content
generators the CPU and the GPU tests share."""
import io

import numpy as np

# ITU-T T.81 Annex K.1 (luminance), natural order
BASE_Q = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                   18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101,
                   72, 92, 95, 98, 112, 100, 103, 99], np.int64)
# natural index of the k-th coefficient in zigzag order
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
# Annex K.3: code counts per length 1..16, then the symbols in code order
DC_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
DC_VALS = list(range(12))
AC_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D]
AC_VALS = [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91,
           0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A,
           0x25, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53,
           0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79,
           0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5,
           0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9,
           0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2,
           0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA]

SHAPES = [(8, 8), (16, 8), (8, 16), (1, 1), (9, 9), (13, 21), (520, 24), (640, 480)]  # w, h
QUALITIES = [95, 75, 100, 10]
CONTENTS = ["zero", "mid", "white", "checker1", "checker8", "noise", "ramp", "special"]


def to_u8(f):
    """cv::Mat::convertTo(CV_8U) of a CV_32F image: round to nearest even, clamp to 0..255, NaN -> 0 (and, outside the contract,
    |v| >= 2^31 clamped like any other value)."""
    f = np.asarray(f, np.float32)
    with np.errstate(invalid="ignore"):
        r = np.rint(f)
        return np.where(np.isnan(f), np.float32(0), np.clip(r, 0, 255)).astype(np.uint8)


def content(kind, w, h, index=0):
    """A float32 frame h x w of the named content; `index` varies it (the frames of a batch differ)."""
    y, x = np.mgrid[0:h, 0:w]
    if kind in ("zero", "mid", "white"):
        return np.full((h, w), {"zero": 0.0, "mid": 128.0, "white": 255.0}[kind], np.float32)
    if kind in ("checker1", "checker8"):
        p = 1 if kind == "checker1" else 8
        return ((((x // p) + (y // p) + index) & 1) * 255).astype(np.float32)
    if kind == "noise":
        return np.random.RandomState(1234 + index).uniform(0, 255, (h, w)).astype(np.float32)
    if kind == "ramp":
        return ((x * 0.37 + y * 0.61 + 11.25 * index) % 256).astype(np.float32)
    if kind == "special":  # NaN, infinities, out-of-range values and exact ties among ordinary pixels
        f = np.random.RandomState(99 + index).uniform(-40, 300, (h, w)).astype(np.float32)
        flat = f.reshape(-1)
        vals = np.array([np.nan, -np.inf, np.inf, -0.5, 0.5, 1.5, 2.5, 254.5, 255.5, -3, 300, 1e9, -1e9, -0.0], np.float32)
        flat[::3] = vals[np.arange(flat[::3].size) % vals.size]
        return f
    raise ValueError(kind)


def quant_table(quality):
    """jpeg_quality_scaling + jpeg_add_quant_table(force_baseline): natural order"""
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((BASE_Q * scale + 50) // 100, 1, 255)


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_pass(d, first):
    """one pass of jfdctint.c (CONST_BITS 13, PASS1_BITS 2) along the last axis of d (..., 8), int64 holding 32-bit values"""
    d0, d1, d2, d3, d4, d5, d6, d7 = [d[..., i] for i in range(8)]
    t0, t7, t1, t6, t2, t5, t3, t4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 13 - 2 if first else 13 + 2
    o = [None] * 8
    if first:
        o[0], o[4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        o[0], o[4] = _descale(t10 + t11, 2), _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    o[2] = _descale(z1 + t13 * 6270, n)
    o[6] = _descale(z1 + t12 * (-15137), n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * (-7373), z2 * (-20995), z3 * (-16069) + z5, z4 * (-3196) + z5
    o[7], o[5], o[3], o[1] = _descale(t4 + z1 + z3, n), _descale(t5 + z2 + z4, n), _descale(t6 + z2 + z3, n), _descale(t7 + z1 + z4, n)
    return np.stack(o, -1)


def coefficients(u8, quality):
    """quantised coefficients (blocks in raster order, 64 in zigzag order) of an 8-bit image"""
    h, w = u8.shape
    H, W = (h + 7) // 8 * 8, (w + 7) // 8 * 8
    p = np.pad(u8, ((0, H - h), (0, W - w)), mode="edge").astype(np.int64) - 128
    b = p.reshape(H // 8, 8, W // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 8, 8)
    b = _fdct_pass(b, True)  # rows
    b = _fdct_pass(b.transpose(0, 2, 1), False).transpose(0, 2, 1)  # columns
    assert np.abs(b).max() < 2 ** 31
    div = (quant_table(quality) * 8).reshape(8, 8)
    q = np.sign(b) * ((np.abs(b) + div // 2) // div)
    return q.reshape(-1, 64)[:, ZIGZAG]


def huffman_codes(bits, vals):
    """symbol -> (code, length), the canonical assignment of Annex C"""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def _category(v):
    a = np.abs(v)
    return np.where(a == 0, 0, np.floor(np.log2(np.maximum(a, 1))).astype(np.int64) + 1)


def scan_bytes(zz):
    """the entropy-coded segment of the coefficient array (before EOI): code + amplitude bits, most significant first, the last
    byte padded with ones, 0x00 after every 0xFF"""
    dc, ac = huffman_codes(DC_BITS, DC_VALS), huffman_codes(AC_BITS, AC_VALS)
    dc_code, dc_len = np.array([dc[s][0] for s in range(12)]), np.array([dc[s][1] for s in range(12)])
    ac_code, ac_len = np.zeros(256, np.int64), np.zeros(256, np.int64)
    for s, (c, n) in ac.items():
        ac_code[s], ac_len[s] = c, n
    nb = zz.shape[0]
    # every emitted item as (block, position key, value, bit count); the key orders them inside the block
    diff = zz[:, 0] - np.concatenate([[0], zz[:-1, 0]])
    cat = _category(diff)
    amp = np.where(diff < 0, diff - 1, diff) & ((1 << cat) - 1)
    items = [(np.arange(nb), np.zeros(nb, np.int64), (dc_code[cat] << cat) | amp, dc_len[cat] + cat)]
    bi, ki = np.nonzero(zz[:, 1:])
    ki = ki + 1
    v = zz[bi, ki]
    first = np.concatenate([[True], bi[1:] != bi[:-1]]) if bi.size else np.zeros(0, bool)
    prev = np.where(first, 0, np.concatenate([[0], ki[:-1]]))
    run = ki - prev - 1
    cat = _category(v)
    amp = np.where(v < 0, v - 1, v) & ((1 << cat) - 1)
    sym = ((run & 15) << 4) | cat
    items.append((bi, ki * 4 + 3, (ac_code[sym] << cat) | amp, ac_len[sym] + cat))
    for z in range(3):  # up to three ZRL in front of a coefficient
        m = run // 16 > z
        items.append((bi[m], ki[m] * 4 + z, np.full(m.sum(), ac_code[0xF0]), np.full(m.sum(), ac_len[0xF0])))
    last = np.zeros(nb, np.int64)
    last[bi] = ki  # ascending, so the last write per block is its last non-zero coefficient
    m = last < 63
    items.append((np.nonzero(m)[0], np.full(m.sum(), 64 * 4), np.full(m.sum(), ac_code[0]), np.full(m.sum(), ac_len[0])))
    blk, key, val, n = [np.concatenate([it[i] for it in items]).astype(np.int64) for i in range(4)]
    order = np.lexsort((key, blk))
    val, n = val[order], n[order]
    total = int(n.sum())
    start = np.cumsum(n) - n
    pos = np.arange(total) - np.repeat(start, n)
    bit = (np.repeat(val, n) >> (np.repeat(n, n) - 1 - pos)) & 1
    bit = np.concatenate([bit, np.ones(-total % 8, np.int64)])
    return np.packbits(bit.astype(np.uint8)).tobytes().replace(b"\xff", b"\xff\x00")


def header(w, h, quality):
    """SOI, JFIF APP0 (version 1.01, unit 0, density 1:1, no thumbnail), DQT, SOF0, the two DHT, SOS -- as libjpeg writes them"""
    q = quant_table(quality)[ZIGZAG]
    out = b"\xff\xd8" + b"\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"
    out += b"\xff\xdb\x00\x43\x00" + bytes(int(x) for x in q)
    out += b"\xff\xc0\x00\x0b\x08" + bytes([h >> 8, h & 255, w >> 8, w & 255]) + b"\x01\x01\x11\x00"
    out += b"\xff\xc4\x00\x1f\x00" + bytes(DC_BITS) + bytes(DC_VALS)
    out += b"\xff\xc4\x00\xb5\x10" + bytes(AC_BITS) + bytes(AC_VALS)
    return out + b"\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00"


def encode_u8(u8, quality):
    h, w = u8.shape
    return header(w, h, quality) + scan_bytes(coefficients(u8, quality)) + b"\xff\xd9"


def encode_f32(f, quality):
    return encode_u8(to_u8(f), quality)


def bound(w, h):
    """mdcj_jpeg_bound: 1024 + 416 per block"""
    return 1024 + 416 * ((w + 7) // 8) * ((h + 7) // 8)


def pil_encode(u8, quality):
    """the pin: libjpeg-turbo through PIL, default settings"""
    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(u8), "L").save(buf, "JPEG", quality=quality)
    return buf.getvalue()


def pil_decode(data):
    from PIL import Image

    return np.array(Image.open(io.BytesIO(data)).convert("L"))
