// The DEFLATE block builder of the device PNG encoders (include/mdc_pngw.h, include/mdc_pngw_rgb.h, include/mdc_pnglz.h), in plain
// C++ with no HIP types: the code-length rule, canonical codes, the symbol maps and the run-length coded block header.  The same text
// runs on one lane of pngw_build_kernel and pngw_lengths_kernel (mdc_pngw.hip: the rule, the codes and the bit writer; its Huffman-only
// header writer is its own), on two lanes of pnglz_build_kernel (mdc_pnglz.hip) and in the stand-alone host program
// tests/native/pnglz_block.cpp (under the sanitizers).
#ifndef MDC_PNG_BLOCK_H
#define MDC_PNG_BLOCK_H
#include <stdint.h>

#ifndef PNG_HD
#define PNG_HD inline
#endif

namespace png {

constexpr int kLitLen = 286;     // literals, end-of-block, length symbols
constexpr int kDist = 30;        // distance symbols
constexpr int kAll = kLitLen + kDist;
constexpr int kEob = 256;
constexpr int kMaxSym = 288;     // the largest alphabet huff_lengths takes: MDCP_MAX_SYMBOLS of include/mdc_pngw.h
constexpr int kHdrWords = 144;   // 17 + 57 + 316 * 14 bits at most: 141 words
constexpr int kMinMatch = 4, kMaxMatch = 258, kWindow = 32768, kChunk = 4096;

struct HuffWork {
  unsigned long long wt[2 * kMaxSym];
  uint16_t parent[2 * kMaxSym];
  uint16_t depth[2 * kMaxSym];
  uint16_t order[kMaxSym];
  uint32_t count[16], next[16];
};

struct Block {
  uint32_t hist[kAll];   // in: literal/length counts [0, 286) with hist[256] = 1, distance counts [286, 316)
  uint8_t len[kAll + 4];
  HuffWork work;         // in: work.order = the literal/length symbols ranked by huff_order
  uint32_t codes[kAll];  // out: bit-reversed code | length << 16, the distance codes from 286
  uint8_t sym[kAll + 4], ext[kAll + 4];
  uint32_t clhist[19];
  uint8_t cllen[19];
  uint32_t clcodes[19];
  uint32_t hdr[kHdrWords];  // out: the block header's bits
  uint32_t hdr_bits;
  unsigned long long data_bits;  // out: every token's bits, the end-of-block code not counted
  long long bytes;               // out: the whole stream, padded to a byte
};

// the length symbol of a match of `length` 4..258, its extra bits and their count
PNG_HD void length_symbol(int length, int& sym, int& extra, int& nextra) {
  const int l = length - 3;
  if (length == kMaxMatch) {
    sym = 285, extra = 0, nextra = 0;
    return;
  }
  if (l < 4) {
    sym = 257 + l, extra = 0, nextra = 0;
    return;
  }
  const int top = 31 - __builtin_clz((unsigned)l);  // the highest set bit: 2..7
  nextra = top - 2;
  sym = 257 + 4 * (nextra + 1) + ((l >> nextra) & 3);
  extra = l & ((1 << nextra) - 1);
}

// the distance symbol of `distance` 1..32768
PNG_HD void distance_symbol(int distance, int& sym, int& extra, int& nextra) {
  const int d = distance - 1;
  if (d < 4) {
    sym = d, extra = 0, nextra = 0;
    return;
  }
  const int top = 31 - __builtin_clz((unsigned)d);  // 2..14
  nextra = top - 1;
  sym = 2 * (nextra + 1) + ((d >> nextra) & 1);
  extra = d & ((1 << nextra) - 1);
}

PNG_HD int length_extra_bits(int sym) { return (sym < 265 || sym == 285) ? 0 : (sym - 261) >> 2; }
PNG_HD int distance_extra_bits(int sym) { return sym < 4 ? 0 : (sym - 2) >> 1; }

// order[r] = the used symbol of rank r by (count, symbol); lanes tid, tid + nthr, ... of the caller take their symbols
PNG_HD void huff_order(const uint32_t* hist, int nsym, uint16_t* order, int tid, int nthr) {
  for (int s = tid; s < nsym; s += nthr) {
    const uint32_t c = hist[s];
    if (!c) continue;
    int r = 0;
    for (int j = 0; j < nsym; j++) {
      const uint32_t o = hist[j];
      r += (o && (o < c || (o == c && j < s))) ? 1 : 0;
    }
    order[r] = (uint16_t)s;
  }
}

// include/mdc_pngw.h, "Code lengths"; nsym <= kMaxSym, k.order is filled
PNG_HD void huff_lengths(const uint32_t* hist, int nsym, int limit, HuffWork& k, uint8_t* len) {
  int n = 0;
  for (int s = 0; s < nsym; s++) {
    len[s] = 0;
    n += hist[s] ? 1 : 0;
  }
  if (n == 0) return;
  if (n == 1) {
    len[k.order[0]] = 1;
    return;
  }
  for (int i = 0; i < n; i++) k.wt[i] = hist[k.order[i]];
  int leaf = 0, inner = n, next = n;
  while (next < 2 * n - 1) {
    unsigned long long sum = 0;
    for (int pick = 0; pick < 2; pick++) {
      int node;
      if (leaf < n && (inner >= next || k.wt[leaf] <= k.wt[inner])) node = leaf++;
      else node = inner++;
      sum += k.wt[node];
      k.parent[node] = (uint16_t)next;
    }
    k.wt[next++] = sum;
  }
  k.depth[2 * n - 2] = 0;
  for (int node = 2 * n - 3; node >= 0; node--) k.depth[node] = (uint16_t)(k.depth[k.parent[node]] + 1);
  const uint32_t full = 1u << limit;
  uint32_t kraft = 0;
  for (int i = 0; i < n; i++) {
    const int d = k.depth[i] < limit ? k.depth[i] : limit;
    len[k.order[i]] = (uint8_t)d;
    kraft += 1u << (limit - d);
  }
  while (kraft > full) {
    bool any = false;
    for (int i = 0; i < n && kraft > full; i++) {
      const int s = k.order[i];
      if (len[s] < limit) {
        len[s]++;
        kraft -= 1u << (limit - len[s]);
        any = true;
      }
    }
    if (!any) break;  // n > 2^limit: refused before the launch, and no alphabet of a block is that large
  }
  while (kraft < full) {
    const uint32_t room = full - kraft;
    int i = n - 1;
    while (i >= 0 && !(len[k.order[i]] > 1 && (1u << (limit - len[k.order[i]])) <= room)) i--;
    if (i < 0) break;  // cannot happen for n >= 2 (include/mdc_pngw.h's argument)
    const int s = k.order[i];
    kraft += 1u << (limit - len[s]);
    len[s]--;
  }
}

// codes[s] = the canonical code of symbol s, bit-reversed, | length << 16
PNG_HD void canonical(const uint8_t* len, int nsym, int limit, HuffWork& k, uint32_t* codes) {
  for (int b = 0; b <= limit; b++) k.count[b] = 0;
  for (int s = 0; s < nsym; s++) k.count[len[s]]++;
  k.count[0] = 0;
  uint32_t code = 0;
  for (int b = 1; b <= limit; b++) {
    code = (code + k.count[b - 1]) << 1;
    k.next[b] = code;
  }
  for (int s = 0; s < nsym; s++) {
    const int l = len[s];
    uint32_t c = l ? k.next[l]++ : 0, r = 0;
    for (int i = 0; i < l; i++) {
      r = (r << 1) | (c & 1);
      c >>= 1;
    }
    codes[s] = r | ((uint32_t)l << 16);
  }
}

PNG_HD void put_bits(uint32_t* words, uint32_t& nbits, uint32_t v, int n) {
  const uint32_t at = nbits & 31;
  words[nbits >> 5] |= v << at;
  if (at + n > 32) words[(nbits >> 5) + 1] |= v >> (32 - at);
  nbits += n;
}

PNG_HD long long stored_bytes(long long F) { return F + 5 * ((F + 65534) / 65535); }

// One dynamic block from the two histograms: both codes, the header and the stream's size.  With no length and no distance symbol
// used this is include/mdc_pngw.h's Huffman-only block bit for bit (HLIT 257 codes, one distance code of length 0), which
// mdc_pngw.hip builds with a text of its own.
PNG_HD void build_block(Block& B) {
  huff_lengths(B.hist, kLitLen, 15, B.work, B.len);
  canonical(B.len, kLitLen, 15, B.work, B.codes);
  huff_order(B.hist + kLitLen, kDist, B.work.order, 0, 1);
  huff_lengths(B.hist + kLitLen, kDist, 15, B.work, B.len + kLitLen);
  canonical(B.len + kLitLen, kDist, 15, B.work, B.codes + kLitLen);
  int nlit = 257, ndist = 1;
  for (int s = 257; s < kLitLen; s++)
    if (B.len[s]) nlit = s + 1;
  for (int s = 1; s < kDist; s++)
    if (B.len[kLitLen + s]) ndist = s + 1;
  const int nseq = nlit + ndist;
  for (int i = 0; i < 19; i++) B.clhist[i] = 0;
  int nsyms = 0;
  for (int i = 0; i < nseq;) {
    const int v = B.len[i < nlit ? i : kLitLen + (i - nlit)];
    int run = 1;
    while (i + run < nseq && B.len[i + run < nlit ? i + run : kLitLen + (i + run - nlit)] == v) run++;
    i += run;
    if (v == 0) {
      while (run >= 11) {
        const int n = run < 138 ? run : 138;
        B.sym[nsyms] = 18, B.ext[nsyms++] = (uint8_t)(n - 11);
        run -= n;
      }
      if (run >= 3) {
        B.sym[nsyms] = 17, B.ext[nsyms++] = (uint8_t)(run - 3);
        run = 0;
      }
    } else {
      B.sym[nsyms] = (uint8_t)v, B.ext[nsyms++] = 0;
      run--;
      while (run >= 3) {
        const int n = run < 6 ? run : 6;
        B.sym[nsyms] = 16, B.ext[nsyms++] = (uint8_t)(n - 3);
        run -= n;
      }
    }
    for (; run > 0; run--) B.sym[nsyms] = (uint8_t)v, B.ext[nsyms++] = 0;
  }
  for (int i = 0; i < nsyms; i++) B.clhist[B.sym[i]]++;
  huff_order(B.clhist, 19, B.work.order, 0, 1);
  huff_lengths(B.clhist, 19, 7, B.work, B.cllen);
  canonical(B.cllen, 19, 7, B.work, B.clcodes);
  const uint8_t clorder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  int hclen = 4;
  for (int i = 4; i < 19; i++)
    if (B.cllen[clorder[i]]) hclen = i + 1;
  for (int i = 0; i < kHdrWords; i++) B.hdr[i] = 0;
  uint32_t bits = 0;
  put_bits(B.hdr, bits, 1, 1);  // BFINAL
  put_bits(B.hdr, bits, 2, 2);  // BTYPE: dynamic
  put_bits(B.hdr, bits, (uint32_t)(nlit - 257), 5);
  put_bits(B.hdr, bits, (uint32_t)(ndist - 1), 5);
  put_bits(B.hdr, bits, (uint32_t)(hclen - 4), 4);
  for (int i = 0; i < hclen; i++) put_bits(B.hdr, bits, B.cllen[clorder[i]], 3);
  for (int i = 0; i < nsyms; i++) {
    const int s = B.sym[i];
    put_bits(B.hdr, bits, B.clcodes[s] & 0xffffu, (int)(B.clcodes[s] >> 16));
    if (s >= 16) put_bits(B.hdr, bits, B.ext[i], s == 16 ? 2 : s == 17 ? 3 : 7);
  }
  unsigned long long data = 0;
  for (int s = 0; s < kLitLen; s++)
    if (s != kEob) data += (unsigned long long)B.hist[s] * (unsigned)(B.len[s] + (s > kEob ? length_extra_bits(s) : 0));
  for (int s = 0; s < kDist; s++) data +=(unsigned long long)B.hist[kLitLen + s] * (unsigned)(B.len[kLitLen + s] + distance_extra_bits(s));
  B.hdr_bits = bits;
  B.data_bits = data;
  B.bytes = (long long)((bits + data + B.len[kEob] + 7) >> 3);
}

}  // namespace png
#endif  // MDC_PNG_BLOCK_H
