// jopt_table: csrc/jpeg_optimal_table.h -- the table rule of libmdc_jopt.so -- as a stand-alone host program, so that it can run
// under AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_jopt_cpu.py builds it through build.build_jopt_table_program).
//   jopt_table < histograms
// input: the number of tables, then 257 counts per table (entry 256 is ignored), whitespace-separated decimal;
// output, one line per table: status depth nvals, the 16 length counts, the nvals symbols.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "jpeg_optimal_table.h"

int main() {
  int ntables = 0;
  if (scanf("%d", &ntables) != 1 || ntables < 0 || ntables > 4096) {
    fprintf(stderr, "jopt_table: the number of tables (0..4096) first\n");
    return 2;
  }
  for (int t = 0; t < ntables; t++) {
    // heap arrays of the exact sizes, so that the sanitizer sees a step outside any of them
    std::vector<uint32_t> freq(257);
    for (int i = 0; i < 257; i++) {
      unsigned long long v;
      if (scanf("%llu", &v) != 1 || v > 0xffffffffull) {
        fprintf(stderr, "jopt_table: table %d, count %d is missing or not a 32-bit number\n", t, i);
        return 2;
      }
      freq[i] = (uint32_t)v;
    }
    std::vector<jopt::Work> work(1);
    std::vector<uint8_t> bits(16), vals(256);
    int nvals = -1, depth = -1;
    const int status = jopt::optimal_table(freq.data(), work[0], jopt::SerialSearch(), bits.data(), vals.data(), &nvals, &depth);
    printf("%d %d %d", status, depth, nvals);
    for (int i = 0; i < 16; i++) printf(" %d", bits[i]);
    for (int i = 0; i < nvals; i++) printf(" %d", vals[i]);
    printf("\n");
  }
  return 0;
}
