"""Hand-built baseline JPEG files for the device Huffman decoder (csrc/mdc_jpeg.hip, csrc/host/image_codecs_jpeg_stream.cpp) and what
it must make of them.  Plain functions: tests/test_jdec_cpu.py runs the cases through the host decoder and a sequential decoder of
the device tables, tests/test_jdec.py through the kernels at every launch form.

The reference of a case is the coefficient grid the writer itself encoded -- the whole MCU-padded luma grid, natural order, int16
after the DC predictor's wrap -- not a second decoder: Pillow's encoder cannot write most of what the parser and the kernels accept
(luma sampling beyond 2 x 2, tables with 16-bit codes everywhere, AC sizes above 10, end-of-block symbols other than 0x00)."""
import collections
import functools

import numpy as np

import jenc_restatement as J

ZIGZAG = J.ZIGZAG
STD_DC, STD_AC = (list(J.DC_BITS), list(J.DC_VALS)), (list(J.AC_BITS), list(J.AC_VALS))

# Quantisation tables (natural order) under which Pillow's pixels stay a reference.  libjpeg-turbo runs its inverse DCT in 16-bit SIMD
# arithmetic where it can: dequantised coefficients are taken modulo 2^16 and the first pass's results saturate at 16 bits, where
# the C code -- and this project's decoders -- are exact.  Dense blocks of 63 coefficients of size 10 stay clear of that with
# magnitudes 512 .. SAFE_AC under UNIT_Q (measured on 4096 random dense blocks: none differs up to 560, 6 pixels differ at 600);
# smaller sizes keep their whole range.  SPARSE_Q is for blocks of a few coefficients.
UNIT_Q = np.ones(64, np.int64)
UNIT_Q[0] = 2
SPARSE_Q = 1 + np.arange(64) % 2
SAFE_AC = 540


def safe_bits(rng, size):
    """random magnitude bits of a coefficient of `size` bits, |value| <= SAFE_AC"""
    lo = 1 << (size - 1)
    v = int(rng.integers(lo, min(1 << size, SAFE_AC + 1))) if size else 0
    return magnitude(v if rng.random() < 0.5 else -v)[1]


Case = collections.namedtuple("Case", "name w h data grid expect pil group")
# launch forms of launch_jpeg_huffman by batch size: 1, 16: 8 workgroups per frame; 17, 47: 4, the stream words in LDS; 48, 64: 4, staged
# blocks; 65, 128: 2, whole-block staging without zero-fill; 129: one workgroup per frame (and one slice per frame of intervals)
ALL_FORMS = (1, 16, 17, 47, 48, 64, 65, 128, 129)
# group -> (w, h, batch sizes): a launch has one size
GROUPS = collections.OrderedDict([
    ("sampling", (50, 37, ALL_FORMS)), ("tables", (56, 40, ALL_FORMS)), ("dcwrap", (72, 48, ALL_FORMS)), ("dense", (64, 48, ALL_FORMS)),
    ("twobit", (640, 480, ALL_FORMS)), ("onebyte", (8, 8, ALL_FORMS)),
    ("len1", (128, 96, (129,))), ("len2", (192, 128, (65, 128))), ("len4", (256, 192, (17, 47, 48, 64))), ("lds", (512, 240, (17, 47))),
    ("intervals", (128, 64, ALL_FORMS)), ("many", (264, 264, (1, 16, 129))),
])


def huff_codes(bits, vals):
    """(BITS, VALS) of a DHT segment -> {symbol: (code, length)}, the canonical codes of T.81 Annex C"""
    assert len(bits) == 16 and sum(bits) == len(vals) and len(set(vals)) == len(vals)
    out, code, k = {}, 0, 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            assert code < (1 << ln) - 1, "the all-ones code of a length stays free"
            out[vals[k]] = (code, ln)
            code += 1
            k += 1
        code <<= 1
    return out


def extend(bits, size):
    return bits if size == 0 or bits >> (size - 1) else bits - (1 << size) + 1


def magnitude(v):
    """a value -> (size, the `size` bits that code it)"""
    size = int(abs(int(v))).bit_length()
    return size, int(v) if v >= 0 else int(v) + (1 << size) - 1


def symbols_of(zz, pred):
    """64 zig-zag coefficients (DC absolute) -> the symbol list a baseline encoder writes: (symbol, magnitude bits) entries"""
    size, bits = magnitude(int(zz[0]) - pred)
    out = [(size, bits)]
    run = 0
    for k in range(1, 64):
        v = int(zz[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            out.append((0xF0, 0))
            run -= 16
        size, bits = magnitude(v)
        out.append((run << 4 | size, bits))
        run = 0
    if run:
        out.append((0x00, 0))
    return out


class Writer:
    """A baseline JPEG file of (w, h) with components [(h, v), ...] (one or three; luma first), Huffman tables `dht`
    {(class, id): (BITS, VALS)} (luma uses id 0, chroma id 1; id 1 defaults to id 0's), restart interval `dri` in MCUs, the bit that
    pads an interval to a byte, and `fill` FF bytes in front of every RSTn and of EOI.  encode(blocks): the blocks in scan order, each
    64 zig-zag coefficients or a list of (symbol, magnitude bits) and ("raw", value, nbits) entries; the scan is FF00-stuffed.
    Afterwards: .grid, the luma coefficients as encoded (MCU-padded, natural order, int16 after the predictor's wrap; None where a
    block does not decode: raw bits, a run past 63, a block that does not end), .ecs_bytes, the scan's length without stuffing, markers
    and fill, and .interval_bytes."""

    def __init__(self, w, h, comps, dht=None, dri=0, pad_bit=1, fill=0, quant=None, sof_comps=None):
        assert len(comps) in (1, 3)
        self.w, self.h, self.comps, self.dri, self.pad_bit, self.fill = w, h, list(comps), dri, pad_bit, fill
        self.sof_comps = list(sof_comps or comps)
        dht = dict(dht or {(0, 0): STD_DC, (1, 0): STD_AC})
        if len(comps) == 3:
            dht.setdefault((0, 1), dht[(0, 0)])
            dht.setdefault((1, 1), dht[(1, 0)])
        self.dht = dht
        self.codes = {k: huff_codes(*v) for k, v in dht.items()}
        self.quant = np.asarray(UNIT_Q if quant is None else quant, np.int64)
        hy, vy = comps[0] if len(comps) == 3 else (1, 1)  # (a one-component scan is not interleaved: one block per MCU)
        self.hy, self.vy = hy, vy
        self.mx, self.my = (w + 8 * hy - 1) // (8 * hy), (h + 8 * vy - 1) // (8 * vy)
        self.per_mcu = hy * vy + (2 if len(comps) == 3 else 0)
        self.nblocks = self.mx * self.my * self.per_mcu

    def cost(self, entry, cls, tid=0):
        """bits an entry takes"""
        if entry[0] == "raw":
            return entry[2]
        sym = entry[0]
        return self.codes[(cls, tid)][sym][1] + (sym if cls == 0 else sym & 15)

    def header(self):
        def seg(marker, body):
            return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + bytes(body)

        out = b"\xff\xd8" + seg(0xDB, [0] + [int(self.quant[ZIGZAG[k]]) for k in range(64)])
        n = len(self.sof_comps)
        sof = [8] + list(self.h.to_bytes(2, "big")) + list(self.w.to_bytes(2, "big")) + [n]
        for i, (ch, cv) in enumerate(self.sof_comps):
            sof += [i + 1, ch << 4 | cv, 0]
        out += seg(0xC0, sof)
        for (cls, tid), (bits, vals) in sorted(self.dht.items()):
            out += seg(0xC4, [cls << 4 | tid] + list(bits) + list(vals))
        if self.dri:
            out += seg(0xDD, list(self.dri.to_bytes(2, "big")))
        sos = [n]
        for i in range(n):
            sos += [i + 1, 0x00 if i == 0 else 0x11]
        return out + seg(0xDA, sos + [0, 63, 0])

    def encode(self, blocks, nblocks=None):
        """-> the file.  nblocks: fewer blocks than the frame has (a scan cut short)"""
        want = self.nblocks if nblocks is None else nblocks
        assert len(blocks) == want, (len(blocks), want)
        grid = np.zeros((self.my * self.vy, self.mx * self.hy, 64), np.int16)
        valid = want == self.nblocks
        hv = self.hy * self.vy
        pred = [0, 0, 0]
        scan = bytearray()
        self.interval_bytes = []
        acc, nacc, cur = 0, 0, bytearray()

        def close_interval():
            nonlocal acc, nacc, cur
            if nacc:
                pad = 8 - nacc
                acc = acc << pad | ((1 << pad) - 1 if self.pad_bit else 0)
                cur.append(acc)
            acc, nacc = 0, 0
            self.interval_bytes.append(len(cur))
            scan.extend(bytes(cur).replace(b"\xff", b"\xff\x00"))
            cur = bytearray()

        for q, blk in enumerate(blocks):
            m, u = divmod(q, self.per_mcu)
            if self.dri and u == 0 and m and m % self.dri == 0:
                close_interval()
                scan.extend(b"\xff" * self.fill + bytes([0xFF, 0xD0 + (m // self.dri - 1) % 8]))
                pred = [0, 0, 0]
            luma = u < hv
            c = 0 if luma else 1 + u - hv
            tid = 0 if luma else 1
            if not isinstance(blk, list):
                blk = symbols_of(blk, pred[c])
            out = grid[(m // self.mx) * self.vy + u // self.hy, (m % self.mx) * self.hy + u % self.hy] if luma else np.zeros(64, np.int16)
            z = 0
            for e in blk:
                if e[0] == "raw":
                    valid = False
                    v, n = e[1], e[2]
                else:
                    sym, mag = e
                    assert z < 64, "symbols after the end of the block"
                    code, ln = self.codes[(0 if z == 0 else 1, tid)][sym]
                    size = sym if z == 0 else sym & 15
                    assert 0 <= mag < (1 << size) or size == 0 and mag == 0
                    v, n = code << size | mag, ln + size
                    if z == 0:
                        valid = valid and size <= 11  # (a DC category above 11 is no baseline symbol)
                        pred[c] += extend(mag, size)
                        out[0] = ((pred[c] + 32768) & 0xFFFF) - 32768
                        z = 1
                    elif size == 0:
                        z = z + 16 if sym >> 4 == 15 else 64
                    else:
                        z += sym >> 4
                        if z > 63:
                            valid = False
                        else:
                            out[ZIGZAG[z]] = extend(mag, size)
                        z += 1
                acc, nacc = acc << n | v, nacc + n
                while nacc >= 8:
                    nacc -= 8
                    cur.append(acc >> nacc)
                    acc &= (1 << nacc) - 1
            if z < 64:
                valid = False
        close_interval()
        self.grid = grid if valid else None
        self.ecs_bytes = sum(self.interval_bytes)
        return self.header() + bytes(scan) + b"\xff" * self.fill + b"\xff\xd9"


# ------------------------------------------------------------------------------------------------ content


def sparse_blocks(rng, n, max_size=10, fill=0.15, dc=200):
    """n blocks of random sparse coefficients (zig-zag order, DC absolute)"""
    out = []
    for _ in range(n):
        zz = np.zeros(64, np.int64)
        zz[0] = rng.integers(-dc, dc + 1)
        for k in np.nonzero(rng.random(63) < fill * rng.random())[0] + 1:
            size = int(rng.integers(1, max_size + 1))
            zz[k] = int(rng.integers(1 << (size - 1), 1 << size if max_size > 10 else min(1 << size, SAFE_AC + 1))) * (1 if rng.random() < 0.5 else -1)
        out.append(zz)
    return out


def symbol_blocks(rng, wr, n, dc_syms=None, stop=0.08):
    """n blocks as random symbol lists over the symbols the writer's luma tables hold; blocks end with an end-of-block symbol, with a
    ZRL that passes coefficient 63 or with a coefficient at 63.  (Which symbols get drawn is chance: walk_blocks is what uses them all.)"""
    dc_syms = sorted(wr.codes[(0, 0)]) if dc_syms is None else dc_syms
    ac_syms = sorted(wr.codes[(1, 0)])
    eobs = [s for s in ac_syms if s & 15 == 0 and s >> 4 != 15]
    out = []
    for _ in range(n):
        size = int(dc_syms[rng.integers(len(dc_syms))])
        blk = [(size, int(rng.integers(1 << size)))]
        z = 1
        while z < 64:
            s = int(ac_syms[rng.integers(len(ac_syms))])
            run, size = s >> 4, s & 15
            if size == 0 and run != 15:
                if rng.random() > stop * 4:
                    continue
                blk.append((s, 0))
                break
            if size == 0:
                blk.append((s, 0))
                z += 16
                continue
            if z + run > 63 or rng.random() < stop and eobs:
                blk.append((eobs[rng.integers(len(eobs))], 0))
                break
            blk.append((s, safe_bits(rng, size)))
            z += run + 1
        out.append(blk)
    return out


def walk_blocks(rng, wr, n):
    """n blocks that use EVERY symbol of the writer's luma tables: the first blocks walk the AC table's symbol list -- each block takes,
    in table order, the coefficient symbols and ZRLs not used yet that still fit before coefficient 63, and ends with the next
    end-of-block symbol in turn --, then one short block per end-of-block symbol, which ends it before coefficient 48 (so a decoder that
    took the symbol for a ZRL would go on), DC categories in turn, DC terms kept within the category's range of 0; random blocks behind."""
    dc_syms, ac_syms = sorted(wr.codes[(0, 0)]), list(wr.dht[(1, 0)][1])
    eobs = [s for s in ac_syms if s & 15 == 0 and s >> 4 != 15]
    todo = [s for s in ac_syms if s not in eobs]
    first = min((s for s in todo if s & 15), key=lambda s: s >> 4)  # the coefficient symbol of the shortest run
    early = list(eobs)
    out, pred, ends = [], 0, 0
    while todo or early or len(out) < len(dc_syms):
        size = dc_syms[len(out) % len(dc_syms)]
        v = int(rng.integers(1 << size >> 1, 1 << size)) * (-1 if pred > 0 else 1) if size else 0
        pred += v
        blk, z = [(size, magnitude(v)[1])], 1
        if not todo and early:
            blk += [(first, safe_bits(rng, first & 15)), (early.pop(0), 0)]
            assert 1 + (first >> 4) + 1 + 16 <= 63
            out.append(blk)
            continue
        for s in list(todo):
            run, size = s >> 4, s & 15
            if size == 0 and z + 16 <= 63:  # ZRL
                blk.append((s, 0))
                z += 16
                todo.remove(s)
            elif size and z + run <= 63:
                blk.append((s, safe_bits(rng, size)))
                z += run + 1
                todo.remove(s)
        if z < 64:
            blk.append((eobs[ends % len(eobs)], 0))
            ends += 1
        out.append(blk)
    assert len(out) <= n, (len(out), n)
    for blk in symbol_blocks(rng, wr, n - len(out)):  # (their DC terms: a category up to 6, pulled towards 0 as well)
        size = min(blk[0][0], 6)
        v = int(rng.integers(1 << size >> 1, 1 << size)) * (-1 if pred > 0 else 1) if size else 0
        pred += v
        out.append([(size, magnitude(v)[1])] + blk[1:])
    used = {e[0] for blk in out for e in blk[1:]}
    assert used == set(ac_syms) and {blk[0][0] for blk in out} == set(dc_syms), "every symbol of both tables is in the scan"
    return out


def filled_blocks(rng, wr, n, target_bits, dense_sizes=(10, 11)):
    """n blocks in scan order (standard codes, luma and chroma alike) of target_bits - 7 .. target_bits bits in all: dense blocks -- every
    coefficient set, sizes 6..10 -- while the budget lasts, the last dense block trimmed symbol by symbol, blocks of one end-of-block
    behind it"""
    dc, ac = wr.codes[(0, 0)], wr.codes[(1, 0)]
    eob = ac[0x00][1]
    least = dc[0][1] + eob  # a block of DC category 0 and an end-of-block
    used, out = 0, []
    pred = [0, 0, 0]  # (n blocks from the start of a restart interval or of the scan: DC terms kept near 0)
    for q in range(n):
        room = target_bits - used - least * (n - q - 1)
        size = int(rng.integers(0, 7))
        if dc[size][1] + size + eob > room:
            size = 0
        u = q % wr.per_mcu
        c = 0 if u < wr.hy * wr.vy else 1 + u - wr.hy * wr.vy
        v = int(rng.integers(1 << size >> 1, 1 << size)) * (-1 if pred[c] > 0 else 1) if size else 0
        pred[c] += v
        blk = [(size, magnitude(v)[1])]
        room -= dc[size][1] + size
        z = 1
        while z < 64:
            tail = 0 if z == 63 else eob  # (a coefficient at 63 ends the block by itself)
            for size in [int(rng.integers(*dense_sizes))] + list(range(5, 0, -1)):
                if ac[size][1] + size + tail <= room:
                    break
            else:
                break
            blk.append((size, safe_bits(rng, size)))
            room -= ac[size][1] + size
            z += 1
        if z < 64:
            blk.append((0x00, 0))
            room -= eob
        used = target_bits - room - least * (n - q - 1)
        out.append(blk)
    assert target_bits - 7 <= used <= target_bits, (used, target_bits)
    return out


def _case(name, group, wr, blocks, expect="ok", pil=True, nblocks=None):
    w, h, _ = GROUPS[group]
    assert (wr.w, wr.h) == (w, h), name
    data = wr.encode(blocks, nblocks)
    assert (wr.grid is not None) == (expect != "damaged"), name
    return Case(name, w, h, data, wr.grid, expect, pil, group)


# ------------------------------------------------------------------------------------------------ sampling


def sampling_cases():
    """Luma hY x vY, 1..4 each, Cb and Cr 1 x 1 (scan_geo, luma_block and the position u inside the MCU, 0..17): without restart
    intervals (jpeg_huffman_kernel<true>, jpeg_huffman_split_kernel<true>) and with (jpeg_huffman_intervals_kernel<true>)."""
    w, h, _ = GROUPS["sampling"]
    out = []
    for hy in range(1, 5):
        for vy in range(1, 5):
            for kind in range(3):
                rng = np.random.default_rng(100 * hy + 10 * vy + kind)
                mx = (w + 8 * hy - 1) // (8 * hy)
                dri, pad = ((0, 1), (2, 0), (mx, 1))[kind]
                wr = Writer(w, h, [(hy, vy), (1, 1), (1, 1)], dri=dri, pad_bit=pad, quant=SPARSE_Q)
                # Pillow (libjpeg) refuses more than 10 blocks per MCU; the project's decoders take them
                out.append(_case("luma%dx%d_dri%d_pad%d" % (hy, vy, dri, pad), "sampling", wr, sparse_blocks(rng, wr.nblocks), pil=hy * vy + 2 <= 10))
    wr = Writer(w, h, [(1, 1)], sof_comps=[(2, 2)])  # one component: the frame header's factors mean nothing, the host sets 1 x 1
    out.append(_case("gray_declared_2x2", "sampling", wr, sparse_blocks(np.random.default_rng(7), wr.nblocks)))
    return out


# ------------------------------------------------------------------------------------------------ tables and symbols

ALL_AC = [0x00, 0xF0] + [r << 4 | s for r in range(16) for s in range(1, 11)]  # the 162 symbols of a baseline AC table


def flat_table(vals, length):
    bits = [0] * 16
    bits[length - 1] = len(vals)
    return bits, list(vals)


def prefix_table(n12):
    """162 AC symbols: n12 of them with 12-bit codes -- two per 11-bit prefix, so ceil(n12 / 2) device subtables -- the others 8 bits"""
    bits = [0] * 16
    bits[7], bits[11] = 162 - n12, n12
    return bits, ALL_AC


def long_prefixes(stream, table):
    """t1 entries of the stream's decode table `table` (0 DC, 1 AC) that point to a subtable (length field 31) -> how many"""
    t1 = np.asarray(stream[160 + table * 12288: 160 + table * 12288 + 8192]).view(np.uint32)
    return int(((t1 & 31) == 31).sum())


def table_cases():
    out = []
    w, h, _ = GROUPS["tables"]

    def gray(name, ac=STD_AC, dc=STD_DC, blocks=None, seed=0, group="tables", **kw):
        gw, gh, _ = GROUPS[group]
        quant = kw.pop("quant", None)
        wr = Writer(gw, gh, [(1, 1)], dht={(0, 0): dc, (1, 0): ac}, quant=quant)
        rng = np.random.default_rng(seed + 1000)
        b = blocks(rng, wr) if blocks else walk_blocks(rng, wr, wr.nblocks)  # (every symbol of both tables, asserted there)
        gray.wr = wr
        return _case(name, group, wr, b, **kw)

    # every AC symbol behind a code of 8, 11 (the longest in t1) and 16 bits (subtables)
    for ln in (8, 11, 16):
        out.append(gray("ac_all_%dbit" % ln, ac=flat_table(ALL_AC, ln), seed=ln))
    # one code of every length 1..16 (16 symbols; the 16-bit code 1111111111111110)
    every = [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x21, 0xF0, 0x05, 0x12, 0x31, 0x06, 0x41, 0x07, 0x08, 0x0A]
    out.append(gray("every_length_1_16", ac=([1] * 16, every), dc=([1] * 12 + [0] * 4, list(range(12))), seed=3))
    # long codes under exactly 32 prefixes of 11 bits (MDC_JPEG_HUFF_SUBTABLES) and under 33
    out.append(gray("prefixes_32", ac=prefix_table(64), seed=4))
    codes = huff_codes(*prefix_table(64))  # (walk_blocks has used all 64 long codes: every one of the 32 prefixes occurs in the scan)
    assert len({c >> 1 for c, ln in codes.values() if ln == 12}) == 32 and len({c >> 1 for c, ln in huff_codes(*prefix_table(66)).values() if ln == 12}) == 33
    out.append(gray("prefixes_33", ac=prefix_table(66), seed=5, expect="stream_refused"))
    # code lengths 2..10 with len + size == 11 (the value sits in the table entry, bit 13) and == 12 (read behind the code)
    bits, vals = [0] * 16, []
    for ln in range(2, 11):
        bits[ln - 1] = 2
        vals += [0x00 | (11 - ln), 0x10 | (12 - ln)]
    bits[9] += 1
    vals.append(0x00)
    out.append(gray("value_in_entry_11_12", ac=(bits, vals), seed=6))
    # AC sizes 11..15: 242 symbols behind 9-bit codes, the extreme values of int16
    big = [0x00, 0xF0] + [r << 4 | s for r in range(16) for s in range(1, 16)]

    def extremes(rng, wr):
        blocks = sparse_blocks(rng, wr.nblocks, max_size=15, fill=0.5)
        for k, v in enumerate((32767, -32767, 16384, -16384, 1024, -2047, 4096, -8191)):
            blocks[k % len(blocks)][1 + k] = v
            blocks[-1 - k % len(blocks)][63 - k] = -v
        return blocks

    # (libjpeg's inverse DCT is not defined on such input: Pillow's pixels are no reference for AC sizes above 10)
    out.append(gray("ac_sizes_11_15", ac=flat_table(big, 9), blocks=extremes, pil=False))

    # DC category 11, the predictor past +32767 and past -32768: the record keeps its low 16 bits.  (No decoder's pixels are a
    # reference for such a DC term; every block carries an AC coefficient of size 11, which puts the case into that set.)
    def dc_walk(rng, wr):
        diffs = [2047] * 17 + [-2047] * 34 + [2047] * 3
        assert len(diffs) == wr.nblocks and max(np.cumsum(diffs)) > 32767 and min(np.cumsum(diffs)) < -32768
        return [[(11, magnitude(d)[1]), (0x0B, int(rng.integers(2048))), (0x00, 0)] for d in diffs]

    out.append(gray("dc_category_11_wraps_ac_size_11", ac=flat_table(big, 9), blocks=dc_walk, group="dcwrap", pil=False))
    # 0x50 and 0xE0 (run != 0 and != 15, size 0) end a block as 0x00 does
    out.append(gray("eob_0x50_0xE0", ac=flat_table(ALL_AC + [0x50, 0xE0], 8), seed=8))

    # a ZRL from z >= 48 passes coefficient 63: the block ends without an end-of-block
    def zrl_past(rng, wr):
        blocks = []
        for q in range(wr.nblocks):
            at = 47 + q % 15  # a coefficient at 47 .. 61: z = at + 1 >= 48 behind it, a ZRL gives z + 16 >= 64
            zrls, run = divmod(at - 1, 16)
            assert at <= 62 and 1 + 16 * zrls + run == at
            blocks.append([(3, 5)] + [(0xF0, 0)] * zrls + [(run << 4 | 2, 3), (0xF0, 0)])
        blocks[1] = [(0, 0)] + [(0xF0, 0)] * 4  # a fourth ZRL: 1 + 64
        return blocks

    out.append(gray("zrl_past_63", blocks=zrl_past))

    # three ZRLs, then a run that lands exactly on 63
    def lands_on_63(rng, wr):
        z = 2 + 48  # DC, one coefficient at index 1, three ZRLs
        run = 63 - z
        assert run == 13 and z + 12 == 62
        return [[(2, 3), (0x01, 1), (0xF0, 0), (0xF0, 0), (0xF0, 0), (run << 4 | 3, int(rng.integers(8)))] for _ in range(wr.nblocks)]

    out.append(gray("run_lands_on_63", blocks=lands_on_63))

    # blocks of 63 coefficients, 16-bit codes + 10 bits each: ~1650 bits, a block spans five and more subsequences of 256 or 288 bits
    def dense16(rng, wr):
        return [[magnitude(int(rng.integers(-40, 41)))] + [(0x0A, safe_bits(rng, 10)) for _ in range(63)] for _ in range(wr.nblocks)]

    out.append(gray("dense_16bit_codes", ac=flat_table(ALL_AC, 16), blocks=dense16, group="dense"))
    # DC category 0 and end-of-block behind 1-bit codes, a flat frame: 2 bits per block, 4800 blocks in 1200 bytes -- one
    # subsequence completes a hundred blocks
    dc1 = ([1, 0, 0, 0, 11] + [0] * 11, list(range(12)))
    ac1 = ([1] + [0] * 7 + [161] + [0] * 7, ALL_AC)
    c = gray("two_bit_blocks", ac=ac1, dc=dc1, blocks=lambda rng, wr: [[(0, 0), (0x00, 0)]] * wr.nblocks, group="twobit")
    assert gray.wr.ecs_bytes == 1200 and gray.wr.nblocks == 4800
    out.append(c)
    c = gray("one_byte_scan", blocks=lambda rng, wr: [[(0, 0), (0x00, 0)]], group="onebyte")
    assert c.data.endswith(b"\x00\x3f\x00" + bytes([0b00101011]) + b"\xff\xd9")
    out.append(c)
    return out


# ------------------------------------------------------------------------------------------------ stream lengths

K = 1024  # threads of a Huffman workgroup = subsequences of a segment (kHuffThreads)


def one_workgroup_step_bytes():
    """jpeg_huffman_kernel: S = max(256, ceil(nbits / 1024) rounded up to 32) bits -- 256 while nbits <= 256 * 1024"""
    return 256 * K // 8


def split_step_bytes(G):
    """jpeg_huffman_split_kernel: sw = max(9, ceil(ceil(nbits / (1024 G)) / 32) | 1) words -- 9 while nbits <= 9 * 32 * 1024 G"""
    return 9 * 32 * K * G // 8


def lds_step(tables, G=4):
    """The split kernel copies a segment's words to LDS while have * 4 <= lds_stream_bytes, have = 1024 sw + 64 words for a segment
    the stream fills; lds_stream_bytes = 96 KB with two tables, 72 KB with four.  -> (the largest odd sw that fits, the most
    ecs_bytes with that sw: nbits <= sw * 32 * 1024 G)"""
    words = (96 if tables == 2 else 72) * 1024 // 4
    sw = (words - 64) // K
    sw -= 1 - sw % 2
    assert K * sw + 64 <= words < K * (sw + 2) + 64
    return sw, sw * 32 * K * G // 8


def length_case(name, group, nbytes, colour=False, seed=0):
    w, h, _ = GROUPS[group]
    wr = Writer(w, h, [(2, 1), (1, 1), (1, 1)] if colour else [(1, 1)])
    c = _case(name, group, wr, filled_blocks(np.random.default_rng(seed), wr, wr.nblocks, 8 * nbytes))
    assert wr.ecs_bytes == nbytes, (name, wr.ecs_bytes, nbytes)
    return c


def length_cases():
    out = []
    for group, B in (("len1", one_workgroup_step_bytes()), ("len2", split_step_bytes(2)), ("len4", split_step_bytes(4))):
        for d in (-1, 0, 1):
            out.append(length_case("%s_%d" % (group, B + d), group, B + d, seed=B + d))
    for colour in (False, True):
        sw, B = lds_step(4 if colour else 2)
        assert sw == (17 if colour else 23)
        for d in (0, 1):
            out.append(length_case("lds_%s_sw%d_%d" % ("2x1" if colour else "gray", sw + 2 * d, B + d), "lds", B + d, colour, seed=B + d))
    return out


# ------------------------------------------------------------------------------------------------ restart intervals


def interval_case(name, colour, dri, sizes, group="intervals", seed=0, fill=0, pad_bit=1, edit=None, **kw):
    """sizes: bytes of every interval, or None for random sparse blocks"""
    w, h, _ = GROUPS[group]
    wr = Writer(w, h, [(2, 1), (1, 1), (1, 1)] if colour else [(1, 1)], dri=dri, fill=fill, pad_bit=pad_bit)
    rng = np.random.default_rng(seed)
    mcus = wr.mx * wr.my
    if sizes is None:
        blocks = sparse_blocks(rng, wr.nblocks, fill=0.3)
    else:
        blocks = []
        for i, nbytes in enumerate(sizes):
            n = (min(mcus, (i + 1) * dri) - i * dri) * wr.per_mcu
            blocks += filled_blocks(rng, wr, n, 8 * nbytes, dense_sizes=(6, 11))
        assert len(blocks) == wr.nblocks
    if edit:
        edit(blocks, wr)
    c = _case(name, group, wr, blocks, **kw)
    if sizes is not None and not edit:
        assert wr.interval_bytes == list(sizes), name
    return c, wr


def interval_cases():
    """jpeg_huffman_intervals_kernel<false> and <true>: an interval is cut into T = 2^lT parts, lT the largest with
    (ecs_bytes * 8 / n_intervals) >> lT >= 384, at most 6."""
    out = []
    w, h, _ = GROUPS["intervals"]
    for colour in (False, True):
        tag = "2x1" if colour else "gray"
        mcus = (w // 16 if colour else w // 8) * (h // 8)
        dri = mcus // 4
        for lt in range(1, 7):
            step = 384 << lt  # average bits per interval at which lT becomes lt: 768, 1536, ... 24576
            for d in (-1, 0):
                total = step * 4 // 8 + d  # bytes of the four intervals: the average is step - 2 bits, or step
                sizes = [total // 4 + (1 if i < total % 4 else 0) for i in range(4)]
                c, wr = interval_case("iv_%s_T%d_%s" % (tag, 1 << lt, "below" if d else "at"), colour, dri, sizes, seed=lt * 4 + d + 2)
                assert (wr.ecs_bytes * 8 // 4 >= step) == (d == 0) and wr.ecs_bytes * 8 // 4 >= step - 8
                out.append(c)
        # an interval of a single flat MCU (one byte, gray; three bytes, 2 x 1 colour) -- the last, DRI = MCUs - 1 -- behind one of
        # 6.5 KB: T = 64, the flat interval's parts 1..63 are empty
        flat = (6 * (4 if colour else 1) + 7) // 8
        c, wr = interval_case("iv_%s_flat_interval_T64" % tag, colour, mcus - 1, [6500, flat], seed=50)
        assert wr.ecs_bytes * 8 // 2 >> 6 >= 384 and wr.interval_bytes[1] == flat
        out.append(c)
        out.append(interval_case("iv_%s_dri_above_mcus" % tag, colour, mcus + 5, None, seed=51)[0])
        # 5 does not divide the MCU count; 13 and 26 intervals: RST7 is followed by RST0; FF fill bytes before RSTn and EOI
        assert mcus % 5 and mcus // 5 >= 9
        out.append(interval_case("iv_%s_dri5_fill" % tag, colour, 5, None, seed=52, fill=2, pad_bit=0)[0])

        # a stuffed FF as an interval's first byte (DC category 11: 111111110 ...) and as the scan's last (ten 1-bits at coefficient 63)
        def ff_edges(blocks, wr):
            for m in range(0, wr.mx * wr.my, 5):
                blocks[m * wr.per_mcu] = [(11, 1024 + m), (0x00, 0)]
            blocks[-1] = [(1, 1), (0xF0, 0), (0xF0, 0), (0xF0, 0), (0xEA, 1023)]

        c, wr = interval_case("iv_%s_ff_first_and_last" % tag, colour, 5, None, seed=53, edit=ff_edges)
        scan = c.data[c.data.index(b"\xff\xda"):]
        assert scan.endswith(b"\xff\x00\xff\xd9") and scan.count(b"\xd0\xff\x00") >= 1
        out.append(c)
    # DRI 1 on 1089 MCUs: more than 1024 parts, a workgroup takes a second chunk
    c, wr = interval_case("many_gray_dri1", False, 1, None, group="many", seed=60)
    assert wr.mx * wr.my > 1024
    out.append(c)
    w, h, _ = GROUPS["many"]
    wr = Writer(w, h, [(1, 1), (1, 1), (1, 1)], dri=1, pad_bit=0)
    out.append(_case("many_1x1_dri1", "many", wr, sparse_blocks(np.random.default_rng(61), wr.nblocks, fill=0.3)))
    return out


# ------------------------------------------------------------------------------------------------ damaged

# A DC table whose all-zero code is symbol 12: the zero bits the host decoder reads behind the end of a scan are no DC code, so a scan
# that is short of blocks is an error for the host decoder too ("bad DC code"), as it is for the kernels (too few blocks).
DC_ZERO_IS_12 = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0], [12] + list(range(12)))


def damaged_cases():
    """Status 1 on the device, an exception from the host decoder.  The kernels' paths, read in csrc/mdc_jpeg.hip: coefficients are
    written only through `cur`, which is null or luma_block(q) of a q < nluma; the bit reader clamps every word index to the stream's
    words (BitReader::raw); every symbol, wrong ones included, consumes at least one bit, so huff_run ends at its subsequence's end."""
    out = []
    w, h, _ = GROUPS["tables"]
    rng = np.random.default_rng(77)
    # huff_symbol: z + run > 63 with size != 0 -> `over`: nothing is written (at = -1), the block ends (z >= 64), *wrong_out -> huff_run
    # sets *bad in the write pass (cur != nullptr) -> s_flag / the segment's flag bit 1 -> status 1.  Host: "coefficient index out of range".
    wr = Writer(w, h, [(1, 1)])
    blocks = sparse_blocks(rng, wr.nblocks)
    blocks[7] = [(2, 3), (0xF0, 0), (0xF0, 0), (0xF0, 0), (0xF3, 5)]  # z = 49, run 15: index 64
    out.append(_case("run_past_63", "tables", wr, blocks, expect="damaged"))
    # one block short: the prefix sum over the subsequences' completed blocks gives total < nluma -> status 1 (jpeg_huffman_kernel:
    # `total < g.nluma`; split: blocks_incl of the last segment in jpeg_split_status_kernel).  The padding bits are 0s: symbol 12 again.
    wr = Writer(w, h, [(1, 1)], dht={(0, 0): DC_ZERO_IS_12, (1, 0): STD_AC}, pad_bit=0)
    blocks = sparse_blocks(rng, wr.nblocks)
    out.append(_case("one_block_short", "tables", wr, blocks[:-1], expect="damaged", nblocks=wr.nblocks - 1))
    # DC symbol 12 in a scan that is complete otherwise: huff_symbol: `!ac && size > 11` -> wrong: one bit skipped, no value; the
    # write pass of the subsequence that holds the symbol meets it on the true path with cur != nullptr -> *bad -> status 1, whatever
    # the bits behind it decode to (writes through cur, q < nluma).  Host: "bad DC code".
    with12 = list(blocks)
    with12[5] = [(12, 0xABC), (0x00, 0)]
    out.append(_case("dc_symbol_12", "tables", wr, with12, expect="damaged"))
    # RST0 one byte early: the last symbol of interval 0 -- a coefficient at 63 whose one magnitude bit, 0, begins the interval's last
    # byte (padding 0s) -- now ends in the first byte of interval 1.  jpeg_huffman_intervals_kernel, lT == 0 (short intervals, under 768
    # bits on average: one thread per interval, huff_run<true> from the interval's start byte to the next one's): the block completes,
    # nb == expected, but `ob > hi && oz == 0` -> bad -> atomicOr(status, 1); interval 1 begins with the moved byte 00 = DC symbol 12:
    # wrong as well.  Writes go through cur = luma_block(q), q < gi.nluma.  Host: the missing bit reads as the 0 it was, the next
    # interval begins with symbol 12: "bad DC code".
    wi = Writer(w, h, [(1, 1)], dht={(0, 0): DC_ZERO_IS_12, (1, 0): STD_AC}, dri=5, pad_bit=0)
    head = filled_blocks(rng, wi, 4, 300, dense_sizes=(1, 6))
    bits0 = sum(wi.cost(e, 0 if k == 0 else 1) for blk in head for k, e in enumerate(blk))
    last = None
    for filler in ([], [(0x01, 1)]):
        for c in range(12):
            z = 1 + len(filler) + 48
            blk = [(c, (1 << c) - 1 if c else 0)] + filler + [(0xF0, 0)] * 3 + [((63 - z) << 4 | 1, 0)]
            if last is None and (bits0 + sum(wi.cost(e, 0 if k == 0 else 1) for k, e in enumerate(blk))) % 8 == 1:
                last = blk
    whole = wi.encode(head + [last] + sparse_blocks(rng, wi.nblocks - 5))
    at = whole.index(b"\xff\xd0", whole.index(b"\xff\xda"))
    assert wi.ecs_bytes * 8 // len(wi.interval_bytes) < 768  # lT == 0
    assert wi.grid is not None and whole[at - 1] == 0x00 and whole[at - 2] != 0xFF
    out.append(Case("restart_marker_one_byte_early", w, h, whole[:at - 1] + b"\xff\xd0\x00" + whole[at + 2:], None, "damaged", True, "tables"))
    # cut in the middle of a symbol of block 9 (16-bit code, 4 of its 10 magnitude bits; 0-bits pad the byte): block 9
    # never completes, the prefix sum gives total = 9 < nluma -> status 1, the path of one_block_short.  Host: the zeros behind the
    # end are DC symbol 12 in the next block: "bad DC code".
    wr = Writer(w, h, [(1, 1)], dht={(0, 0): DC_ZERO_IS_12, (1, 0): STD_AC}, pad_bit=0)
    code, ln = wr.codes[(1, 0)][0x0A]
    cut = blocks[:9] + [[(0, 0), (0x0A, 1023), ("raw", code << 4 | 0xA, ln + 4)]]
    out.append(_case("cut_mid_symbol", "tables", wr, cut, expect="damaged", nblocks=10))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    out = sampling_cases() + table_cases() + length_cases() + interval_cases() + damaged_cases()
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def by_group():
    g = collections.OrderedDict((k, []) for k in GROUPS)
    for c in cases():
        g[c.group].append(c)
    return g


def stream_cap(group):
    """bytes of a stream buffer that holds every case of the group"""
    from mono_dataset_code_amd import capi

    w, h, _ = GROUPS[group]
    return (2 * capi.JPEG_STREAM_HEADER_BYTES + 4 * ((w + 7) // 8) * ((h + 7) // 8) + max(len(c.data) for c in by_group()[group]) + 64 + 15) & ~15
