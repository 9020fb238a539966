// The PNG decoder's core that both compilers take (hipcc for libmdc_pngd.so's kernels, g++ for tests/native/pngd_core.cpp): the bit
// reader, the canonical-code builder, the sequential inflate (RFC 1950 / 1951), the rule that says which decode path a stream may
// take, and the per-pixel unfilter rule (PNG specification, 9.2).  Plain integer C++, no allocation, no recursion; every array lives in
// a struct the caller places (LDS on the device, the stack on the host).  Every loop consumes at least one input bit per iteration or
// has a constant bound, and nothing is written at or past the output's F bytes, whatever the stream says.
//
// What is refused is what zlib's inflate refuses (the window size in the header is not enforced, as in zlib's default build): the
// status says why.  The order of the checks is part of the interface (tests/pngd_restatement.py restates it):
//   inflate (first failure in stream order; a byte past F is ST_OUTPUT_SIZE at the symbol that would write it)  ->  fewer than F
//   bytes: ST_OUTPUT_SIZE  ->  no room for the 4-byte trailer: ST_TRUNCATED  ->  ST_ADLER  ->  ST_FILTER_TYPE.
#ifndef MDC_PNG_INFLATE_CORE_H
#define MDC_PNG_INFLATE_CORE_H
#include <stdint.h>

#if defined(__HIPCC__)
#define PNGD_HD __host__ __device__ __forceinline__
#else
#define PNGD_HD inline
#endif

namespace pngd {

enum {  // = MDCI_ST_* of include/mdc_pngd.h
  ST_OK = 0,
  ST_TRUNCATED = 1,
  ST_ZLIB_HEADER = 2,
  ST_BLOCK_TYPE = 3,
  ST_STORED_LEN = 4,
  ST_BAD_CODE = 5,
  ST_UNDEFINED_SYMBOL = 6,
  ST_DISTANCE = 7,
  ST_OUTPUT_SIZE = 8,
  ST_FILTER_TYPE = 9,
  ST_ADLER = 10
};
enum { PATH_NONE = 0, PATH_PARALLEL = 1, PATH_STORED = 2, PATH_GENERAL = 3 };  // = MDCI_PATH_*

constexpr int kFastBits = 9;
constexpr int kMaxStoredBlocks = 64;       // = MDCI_MAX_STORED_BLOCKS: longer chains of stored blocks take the general path
constexpr uint32_t kMaxStreamBytes = 0x1fffffffu;  // bit positions are 32-bit
constexpr uint32_t kAdlerMod = 65521;

// Bits least significant first.  `cnt` valid bits in `acc`; a refill loads at most 8 bytes.
struct Bits {
  const uint8_t* p;
  uint32_t n, next;
  uint64_t acc;
  int cnt;
  PNGD_HD void refill() {
    for (int k = 0; k < 8; k++)
      if (cnt <= 56 && next < n) {
        acc |= (uint64_t)p[next++] << cnt;
        cnt += 8;
      }
  }
  PNGD_HD void seek(const uint8_t* p_, uint32_t n_, uint32_t bit) {
    p = p_, n = n_, next = bit >> 3, acc = 0, cnt = 0;
    if (next > n) next = n;
    refill();
    const int k = (int)(bit & 7);
    if (k <= cnt) acc >>= k, cnt -= k;
    else acc = 0, cnt = 0;
  }
  PNGD_HD uint32_t bitpos() const { return next * 8u - (uint32_t)cnt; }
  PNGD_HD bool take(int k, uint32_t& v) {  // k <= 32
    refill();
    if (cnt < k) return false;
    v = (uint32_t)(acc & ((1ull << k) - 1));
    acc >>= k, cnt -= k;
    return true;
  }
  PNGD_HD void align() {
    const int k = cnt & 7;
    acc >>= k, cnt -= k;
  }
};

struct Code {
  uint16_t count[16], offs[16];
  uint16_t sym[288];
  uint16_t fast[1 << kFastBits];  // length << 9 | symbol for codes of at most kFastBits bits, by the next bits of the stream; 0: none
};

struct Work {
  Code lit, dist;
  uint8_t lens[320];
  uint8_t cl[19];
  uint32_t built_status, built_bit;  // what the builder of a block's tables hands to those who only read them (inflate)
};

PNGD_HD uint32_t reverse_bits(uint32_t v, int n) {
  uint32_t r = 0;
  for (int i = 0; i < 15; i++)
    if (i < n) r = (r << 1) | ((v >> i) & 1);
  return r;
}

// The canonical code of len[0 .. n).  Over-subscribed: refused.  Incomplete: refused unless no symbol is coded at all, or (not for the
// code-length code) the only code has one bit -- zlib's rule.
PNGD_HD int build(Code& c, const uint8_t* len, int n, bool is_cl) {
  for (int i = 0; i < 16; i++) c.count[i] = 0;
  for (int i = 0; i < n; i++) c.count[len[i]]++;
  c.count[0] = 0;
  for (int i = 0; i < (1 << kFastBits); i++) c.fast[i] = 0;
  int maxl = 0, left = 1;
  for (int l = 1; l <= 15; l++) {
    if (c.count[l]) maxl = l;
    left = (left << 1) - (int)c.count[l];
    if (left < 0) return ST_BAD_CODE;
  }
  if (left > 0 && maxl != 0 && (is_cl || maxl != 1)) return ST_BAD_CODE;
  c.offs[0] = c.offs[1] = 0;
  for (int l = 1; l < 15; l++) c.offs[l + 1] = (uint16_t)(c.offs[l] + c.count[l]);
  for (int i = 0; i < n; i++)
    if (len[i]) c.sym[c.offs[len[i]]++] = (uint16_t)i;
  uint32_t code = 0;
  int idx = 0;
  for (int l = 1; l <= kFastBits; l++) {
    for (int k = 0; k < (int)c.count[l]; k++) {
      const uint32_t s = c.sym[idx++];
      for (uint32_t j = reverse_bits(code, l); j < (1u << kFastBits); j += 1u << l) c.fast[j] = (uint16_t)((l << 9) | s);
      code++;
    }
    code <<= 1;
  }
  return ST_OK;
}

// The next symbol, or -ST_TRUNCATED / -ST_UNDEFINED_SYMBOL.  Codes longer than kFastBits walk the counts (first code of each length).
PNGD_HD int decode(const Code& c, Bits& b) {
  b.refill();
  const uint32_t e = c.fast[(uint32_t)b.acc & ((1u << kFastBits) - 1)];
  if (e) {
    const int l = (int)(e >> 9);
    if (l > b.cnt) return -ST_TRUNCATED;
    b.acc >>= l, b.cnt -= l;
    return (int)(e & 511);
  }
  int code = 0, first = 0, index = 0;
  for (int l = 1; l <= 15; l++) {
    if (l > b.cnt) return -ST_TRUNCATED;
    code |= (int)((b.acc >> (l - 1)) & 1);
    const int count = c.count[l];
    if (code - count < first) {
      b.acc >>= l, b.cnt -= l;
      return c.sym[index + (code - first)];
    }
    index += count;
    first = (first + count) << 1;
    code <<= 1;
  }
  return -ST_UNDEFINED_SYMBOL;
}

PNGD_HD int zlib_header(const uint8_t* p, uint32_t n) {
  if (n < 2) return ST_TRUNCATED;
  const uint32_t cmf = p[0], flg = p[1];
  if ((cmf & 15) != 8 || (cmf >> 4) > 7 || ((cmf << 8) | flg) % 31 != 0 || (flg & 32)) return ST_ZLIB_HEADER;
  return ST_OK;
}

// The header of a dynamic block, after its three type bits: w.lit and w.dist; *dist_codes = the number of distance symbols with a code.
PNGD_HD int dynamic_header(Work& w, Bits& b, int* dist_codes) {
  const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  uint32_t v;
  if (!b.take(14, v)) return ST_TRUNCATED;
  const int hlit = 257 + (int)(v & 31), hdist = 1 + (int)((v >> 5) & 31), hclen = 4 + (int)(v >> 10);
  if (hlit > 286 || hdist > 30) return ST_BAD_CODE;
  for (int i = 0; i < 19; i++) w.cl[i] = 0;
  for (int i = 0; i < 19; i++)
    if (i < hclen) {
      if (!b.take(3, v)) return ST_TRUNCATED;
      w.cl[order[i]] = (uint8_t)v;
    }
  if (build(w.dist, w.cl, 19, true) != ST_OK) return ST_BAD_CODE;  // (the code-length code borrows w.dist)
  const int total = hlit + hdist;
  for (int idx = 0; idx < total;) {  // every round takes at least one bit
    const int s = decode(w.dist, b);
    if (s < 0) return -s;
    if (s < 16) {
      w.lens[idx++] = (uint8_t)s;
      continue;
    }
    int rep, val = 0;
    if (s == 16) {
      if (idx == 0) return ST_BAD_CODE;
      val = w.lens[idx - 1];
      if (!b.take(2, v)) return ST_TRUNCATED;
      rep = 3 + (int)v;
    } else if (s == 17) {
      if (!b.take(3, v)) return ST_TRUNCATED;
      rep = 3 + (int)v;
    } else {
      if (!b.take(7, v)) return ST_TRUNCATED;
      rep = 11 + (int)v;
    }
    if (idx + rep > total) return ST_BAD_CODE;
    for (int k = 0; k < rep; k++) w.lens[idx++] = (uint8_t)val;  // rep <= 138
  }
  if (w.lens[256] == 0) return ST_BAD_CODE;  // no end-of-block code
  int nd = 0;
  for (int i = 0; i < 30; i++)
    if (i < hdist && w.lens[hlit + i]) nd++;
  *dist_codes = nd;
  if (build(w.lit, w.lens, hlit, false) != ST_OK) return ST_BAD_CODE;
  if (build(w.dist, w.lens + hlit, hdist, false) != ST_OK) return ST_BAD_CODE;
  return ST_OK;
}

PNGD_HD void fixed_codes(Work& w) {
  for (int i = 0; i < 288; i++) w.lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
  for (int i = 0; i < 32; i++) w.lens[288 + i] = 5;
  (void)build(w.lit, w.lens, 288, false);
  (void)build(w.dist, w.lens + 288, 32, false);
}

// Which path may try a stream first (the device's classify step and the restatement's): PATH_PARALLEL for a single final dynamic
// block in which no distance symbol has a code (*data_bit = where its symbols start; w.lit is its code), PATH_STORED when the first
// block is stored, PATH_GENERAL for everything else, a damaged header included: the sequential decoder says what is wrong with it.
PNGD_HD int classify(Work& w, const uint8_t* p, uint32_t n, uint32_t* data_bit) {
  if (zlib_header(p, n) != ST_OK) return PATH_GENERAL;
  Bits b;
  b.seek(p, n, 16);
  uint32_t hdr;
  if (!b.take(3, hdr)) return PATH_GENERAL;
  if ((hdr >> 1) == 0) return PATH_STORED;
  if (hdr != 5) return PATH_GENERAL;  // not (final, dynamic)
  int nd = 0;
  if (dynamic_header(w, b, &nd) != ST_OK || nd != 0) return PATH_GENERAL;
  *data_bit = b.bitpos();
  return PATH_PARALLEL;
}

// A chain of stored blocks from byte 2 on, as the stored path copies it: block k is len[k] bytes from src[k] of the stream to dst[k] of
// the output.  true: at most kMaxStoredBlocks blocks, all stored, all inside the stream, F bytes in all, the last one final; *end_byte
// = where the trailer starts.  false: the sequential decoder is to look at the stream.
PNGD_HD bool stored_chain(const uint8_t* p, uint32_t n, uint32_t F, uint32_t* src, uint32_t* dst, uint32_t* len, uint32_t* nblk, uint32_t* end_byte) {
  uint32_t o = 2, total = 0;
  *nblk = 0;
  for (int k = 0; k < kMaxStoredBlocks; k++) {
    if (n < 5 || o > n - 5) return false;
    const uint32_t hdr = p[o], l = p[o + 1] | (uint32_t)p[o + 2] << 8, nl = p[o + 3] | (uint32_t)p[o + 4] << 8;
    if (((hdr >> 1) & 3) != 0 || l != (~nl & 0xffffu) || l > n - (o + 5) || l > F - total) return false;
    src[k] = o + 5, dst[k] = total, len[k] = l;
    *nblk = (uint32_t)k + 1;
    total += l;
    o += 5 + l;
    if (hdr & 1) {
      *end_byte = o;
      return total == F;
    }
  }
  return false;
}

// Out: pos (bytes written so far), put(byte), copy(distance, length), stored(source, length); inflate() has checked the room.
// inflate() may be run by several lanes at once on ONE Work (a wave on the device): only the lane for which out.builder() is true
// writes to it -- it parses a block's header and builds the tables --, out.barrier() orders that against the others' reads, and all of
// them go on from the bit position it reached.  One lane: builder() is true and barrier() does nothing.
template <class Out>
PNGD_HD int inflate(Work& w, const uint8_t* p, uint32_t n, Out& out, uint32_t F, uint32_t* end_byte) {
  const int zh = zlib_header(p, n);
  if (zh != ST_OK) return zh;
  Bits b;
  b.seek(p, n, 16);
  for (;;) {  // a block takes at least its three header bits
    uint32_t hdr, v;
    if (!b.take(3, hdr)) return ST_TRUNCATED;
    const uint32_t type = hdr >> 1;
    if (type == 3) return ST_BLOCK_TYPE;
    if (type == 0) {
      b.align();
      if (!b.take(32, v)) return ST_TRUNCATED;
      const uint32_t len = v & 0xffffu;
      if (len != ((~v >> 16) & 0xffffu)) return ST_STORED_LEN;
      const uint32_t at = b.bitpos() >> 3;
      if (len > n - at) return ST_TRUNCATED;
      if (len > F - out.pos) return ST_OUTPUT_SIZE;
      out.stored(p + at, len);
      b.seek(p, n, (at + len) * 8u);
    } else {
      const uint32_t at = b.bitpos();
      out.barrier();  // nobody still reads the previous block's tables
      if (out.builder()) {
        int nd, st = ST_OK;
        if (type == 1) fixed_codes(w);
        else st = dynamic_header(w, b, &nd);
        w.built_status = (uint32_t)st, w.built_bit = type == 1 ? at : b.bitpos();
      }
      out.barrier();
      if (w.built_status != ST_OK) return (int)w.built_status;
      b.seek(p, n, w.built_bit);
      for (;;) {  // a symbol takes at least one bit
        const int s = decode(w.lit, b);
        if (s < 0) return -s;
        if (s < 256) {
          if (out.pos >= F) return ST_OUTPUT_SIZE;
          out.put((uint8_t)s);
          continue;
        }
        if (s == 256) break;
        if (s > 285) return ST_UNDEFINED_SYMBOL;
        const int i = s - 257;
        const int lx = i < 8 || i == 28 ? 0 : (i >> 2) - 1;
        uint32_t len = i < 8 ? (uint32_t)i + 3u : i == 28 ? 258u : ((4u + (uint32_t)(i & 3)) << lx) + 3u;
        if (lx) {
          if (!b.take(lx, v)) return ST_TRUNCATED;
          len += v;
        }
        const int d = decode(w.dist, b);
        if (d < 0) return -d;
        if (d > 29) return ST_UNDEFINED_SYMBOL;
        const int dx = d < 4 ? 0 : (d >> 1) - 1;
        uint32_t dist = d < 4 ? (uint32_t)d + 1u : ((2u + (uint32_t)(d & 1)) << dx) + 1u;
        if (dx) {
          if (!b.take(dx, v)) return ST_TRUNCATED;
          dist += v;
        }
        if (dist > out.pos) return ST_DISTANCE;
        if (len > F - out.pos) return ST_OUTPUT_SIZE;
        out.copy(dist, len);
      }
    }
    if (hdr & 1) break;
  }
  *end_byte = (b.bitpos() + 7u) >> 3;
  return out.pos == F ? ST_OK : ST_OUTPUT_SIZE;
}

// The Adler-32 of the F filtered bytes from s1 = sum d[i] and s2 = sum (F - i) d[i] (any representatives mod 65521 will do)
PNGD_HD uint32_t adler_of(uint64_t s1, uint64_t s2, uint32_t F) {
  const uint32_t a = (uint32_t)((1 + s1 % kAdlerMod) % kAdlerMod), b = (uint32_t)((F % kAdlerMod + s2 % kAdlerMod) % kAdlerMod);
  return (b << 16) | a;
}

// The trailer: four bytes, big-endian, at end_byte
PNGD_HD int check_trailer(const uint8_t* p, uint32_t n, uint32_t end_byte, uint32_t adler) {
  if (end_byte > n || n - end_byte < 4) return ST_TRUNCATED;
  const uint32_t want = (uint32_t)p[end_byte] << 24 | (uint32_t)p[end_byte + 1] << 16 | (uint32_t)p[end_byte + 2] << 8 | p[end_byte + 3];
  return want == adler ? ST_OK : ST_ADLER;
}

// One pixel: x = the filtered byte, a = the pixel to the left, b = the one above, c = the one above a (0 where there is none).  All five
// candidates are computed and the row's type selects one: no branch.
PNGD_HD int unfilter_px(int type, int x, int a, int b, int c) {
  const int p = a + b - c;
  const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
  const int paeth = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
  const int pred = type == 1 ? a : type == 2 ? b : type == 3 ? ((a + b) >> 1) : type == 4 ? paeth : 0;
  return (x + pred) & 255;
}

}  // namespace pngd
#endif  // MDC_PNG_INFLATE_CORE_H
