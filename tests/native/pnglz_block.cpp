// csrc/pnglz_block.h (the code builder and header writer of libmdc_pnglz.so) as a stand-alone program, built under
// AddressSanitizer and UndefinedBehaviorSanitizer by tests/test_pnglz_cpu.py.  Standard input: one line of 316 counts per case (286
// literal/length counts, 30 distance counts).  Standard output, per case: the 316 code lengths, the header's bit count, the
// stream's bytes, the data bits, then the header's words in hexadecimal.
#include <cstdio>
#include <cstdlib>
#include <new>

#include "pnglz_block.h"

int main() {
  pnglz::Block* B = new pnglz::Block();  // on the heap: the sanitizer sees every index past an array's end
  for (;;) {
    for (int s = 0; s < pnglz::kAll; s++) {
      unsigned long v;
      if (scanf("%lu", &v) != 1) {
        delete B;
        return s == 0 ? 0 : 2;
      }
      B->hist[s] = (uint32_t)v;
    }
    pnglz::huff_order(B->hist, pnglz::kLitLen, B->work.order, 0, 1);
    pnglz::build_block(*B);
    for (int s = 0; s < pnglz::kAll; s++) printf("%d ", B->len[s]);
    printf("| %u %lld %llu |", B->hdr_bits, B->bytes, B->data_bits);
    for (uint32_t w = 0; w < (B->hdr_bits + 31) / 32; w++) printf(" %08x", B->hdr[w]);
    printf("\n");
    // the symbol maps, every value
    for (int l = pnglz::kMinMatch; l <= pnglz::kMaxMatch; l++) {
      int s, e, n;
      pnglz::length_symbol(l, s, e, n);
      if (s < 258 || s > 285 || n != pnglz::length_extra_bits(s) || e >= (1 << n)) return 3;
    }
    for (int d = 1; d <= pnglz::kWindow; d++) {
      int s, e, n;
      pnglz::distance_symbol(d, s, e, n);
      if (s < 0 || s > 29 || n != pnglz::distance_extra_bits(s) || e >= (1 << n)) return 4;
    }
  }
}
