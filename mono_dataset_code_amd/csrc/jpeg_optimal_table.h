// jpeg_optimal_table.h -- the table rule of libmdc_jopt.so (include/mdc_jopt.h), plain C++: jpeg_gen_optimal_table of libjpeg 6b /
// libjpeg-turbo (jchuff.c), restated.  One source for the device (mdc_jopt.hip: one wave per table, the arrays in LDS) and for the
// CPU test program (tests/native/jopt_table.cpp, under the sanitizers).  The two differ in one thing only, the search for the
// least frequent symbol, which is handed in as `Search`: a loop on the host, a wave reduction on the device.  Everything else
// is executed as written -- on the device by every lane of the wave alike (same addresses, same values), so no lane reads what
// another lane alone has written.
//
// The rule:
//   - symbol 256 is added with count 1, so that no real symbol gets the all-ones code;
//   - the two least frequent symbols with a non-zero count are merged until one is left: among equal counts the LARGEST index wins
//     (libjpeg's `<=` while scanning upwards), the second search leaves out the first's winner, counts above 1,000,000,000 are
//     never chosen; the merged count stays with the first winner, and `others` chains the symbols of a tree, each of which gets
//     one bit longer at every merge of its tree;
//   - a code longer than 32 bits is libjpeg's JERR_HUFF_CLEN_OVERFLOW: status 1, no table (so is a histogram with counts above the
//     search limit that leaves more than one tree: libjpeg's result for it is no prefix code);
//   - lengths above 16 are folded back (Annex K.3: take two codes of length i, put one at i - 1, and split a code of the longest
//     shorter length j into two of j + 1), then the pseudo-symbol's code point is taken from the longest length in use;
//   - the symbols are listed by (unlimited length, value).
// An all-zero histogram (libjpeg never sees one: it would read bits[-1]) gives no symbols and status 0.
#ifndef MDC_JPEG_OPTIMAL_TABLE_H
#define MDC_JPEG_OPTIMAL_TABLE_H

#include <stdint.h>

#ifdef __HIPCC__
#define JOPT_HD __host__ __device__ __forceinline__
#else
#define JOPT_HD inline
#endif

namespace jopt {

constexpr int kSymbols = 257;  // 256 and the pseudo-symbol
constexpr int kMaxClen = 32;   // libjpeg's MAX_CLEN
constexpr uint32_t kSearchLimit = 1000000000u;

// The working arrays of one table: 2.4 KB.
struct Work {
  uint32_t freq[kSymbols];
  int16_t codesize[kSymbols];
  int16_t others[kSymbols];
  uint16_t bits[kMaxClen + 1];   // codes per length after limiting; [0] unused
  uint16_t start[kMaxClen + 2];  // first position in vals of the symbols of each unlimited length
};

// The host's search: the index of the least freq[i] with 0 < freq[i] <= limit and i != exclude, the largest such i among equals; -1 if none.
struct SerialSearch {
  JOPT_HD int operator()(const uint32_t* freq, int exclude) const {
    int c = -1;
    uint32_t v = kSearchLimit;
    for (int i = 0; i < kSymbols; i++)
      if (freq[i] && freq[i] <= v && i != exclude) v = freq[i], c = i;
    return c;
  }
};

// freq_in: 257 counts, entry 256 ignored.  -> bits[16] (codes of length 1..16), vals[0 .. *nvals), *depth = the longest code
// before limiting (0: no symbol).  Returns the status: 0 built, 1 not built (deeper than 32).
template <class Search>
JOPT_HD int optimal_table(const uint32_t* freq_in, Work& w, const Search& search, uint8_t* bits, uint8_t* vals, int* nvals, int* depth) {
  for (int i = 0; i < 256; i++) w.freq[i] = freq_in[i], w.codesize[i] = 0, w.others[i] = -1;
  w.freq[256] = 1, w.codesize[256] = 0, w.others[256] = -1;
  for (;;) {
    int c1 = search(w.freq, -1);
    int c2 = search(w.freq, c1);
    if (c2 < 0) break;
    w.freq[c1] += w.freq[c2];
    w.freq[c2] = 0;
    w.codesize[c1]++;
    while (w.others[c1] >= 0) {
      c1 = w.others[c1];
      w.codesize[c1]++;
    }
    w.others[c1] = (int16_t)c2;
    w.codesize[c2]++;
    while (w.others[c2] >= 0) {
      c2 = w.others[c2];
      w.codesize[c2]++;
    }
  }
  int deepest = 0, trees = 0;
  for (int i = 0; i < kSymbols; i++) {
    if (w.codesize[i] > deepest) deepest = w.codesize[i];
    trees += w.freq[i] != 0;  // more than one is left only where counts above the search limit were never merged
  }
  *depth = deepest;
  *nvals = 0;
  for (int i = 0; i < 16; i++) bits[i] = 0;
  if (deepest > kMaxClen || trees > 1) return 1;
  for (int i = 0; i <= kMaxClen; i++) w.bits[i] = 0;
  for (int i = 0; i < kSymbols; i++)
    if (w.codesize[i]) w.bits[w.codesize[i]]++;
  // the symbols by (unlimited length, value): a counting sort, the order of libjpeg's 32 x 256 double loop
  int at = 0;
  for (int i = 1; i <= kMaxClen; i++) {
    w.start[i] = (uint16_t)at;
    at += w.bits[i] - (i == w.codesize[256] ? 1 : 0);  // the pseudo-symbol is counted in its length and not listed
  }
  *nvals = at;
  for (int j = 0; j < 256; j++)
    if (w.codesize[j]) vals[w.start[w.codesize[j]]++] = (uint8_t)j;
  for (int i = kMaxClen; i > 16; i--) {
    while (w.bits[i] > 0) {
      int j = i - 2;
      while (w.bits[j] == 0) j--;
      w.bits[i] -= 2;
      w.bits[i - 1]++;
      w.bits[j + 1] += 2;
      w.bits[j]--;
    }
  }
  int i = 16;
  while (i > 0 && w.bits[i] == 0) i--;
  if (i > 0) w.bits[i]--;
  for (int k = 0; k < 16; k++) bits[k] = (uint8_t)w.bits[k + 1];
  return 0;
}

}  // namespace jopt

#endif  // MDC_JPEG_OPTIMAL_TABLE_H
