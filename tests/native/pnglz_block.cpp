// csrc/png_block.h (the code builder and header writer of the device PNG encoder libraries) as a stand-alone program, built under
// AddressSanitizer and UndefinedBehaviorSanitizer by tests/test_pnglz_cpu.py.
// Without arguments -- standard input: one line of 316 counts per case (286 literal/length counts, 30 distance counts).  Standard
// output, per case: the 316 code lengths, the header's bit count, the stream's bytes, the data bits, then the header's words in
// hexadecimal.
// With the argument "lengths" -- standard input, per case: nsym, limit, then nsym counts.  huff_order and huff_lengths run on heap
// arrays of exactly nsym entries; standard output, per case: the nsym code lengths.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "png_block.h"

static int lengths_mode() {
  png::HuffWork* work = new png::HuffWork();
  int nsym, limit;
  while (scanf("%d %d", &nsym, &limit) == 2) {
    if (nsym < 1 || nsym > png::kMaxSym || limit < 1 || limit > 15) return 2;
    uint32_t* hist = new uint32_t[nsym];
    uint8_t* len = new uint8_t[nsym];
    for (int s = 0; s < nsym; s++) {
      unsigned long v;
      if (scanf("%lu", &v) != 1) return 2;
      hist[s] = (uint32_t)v;
    }
    png::huff_order(hist, nsym, work->order, 0, 1);
    png::huff_lengths(hist, nsym, limit, *work, len);
    for (int s = 0; s < nsym; s++) printf("%d ", len[s]);
    printf("\n");
    delete[] hist;
    delete[] len;
  }
  delete work;
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1) return strcmp(argv[1], "lengths") == 0 ? lengths_mode() : 2;
  png::Block* B = new png::Block();  // on the heap: the sanitizer sees every index past an array's end
  for (;;) {
    for (int s = 0; s < png::kAll; s++) {
      unsigned long v;
      if (scanf("%lu", &v) != 1) {
        delete B;
        return s == 0 ? 0 : 2;
      }
      B->hist[s] = (uint32_t)v;
    }
    png::huff_order(B->hist, png::kLitLen, B->work.order, 0, 1);
    png::build_block(*B);
    for (int s = 0; s < png::kAll; s++) printf("%d ", B->len[s]);
    printf("| %u %lld %llu |", B->hdr_bits, B->bytes, B->data_bits);
    for (uint32_t w = 0; w < (B->hdr_bits + 31) / 32; w++) printf(" %08x", B->hdr[w]);
    printf("\n");
    // the symbol maps, every value
    for (int l = png::kMinMatch; l <= png::kMaxMatch; l++) {
      int s, e, n;
      png::length_symbol(l, s, e, n);
      if (s < 258 || s > 285 || n != png::length_extra_bits(s) || e >= (1 << n)) return 3;
    }
    for (int d = 1; d <= png::kWindow; d++) {
      int s, e, n;
      png::distance_symbol(d, s, e, n);
      if (s < 0 || s > 29 || n != png::distance_extra_bits(s) || e >= (1 << n)) return 4;
    }
  }
}
