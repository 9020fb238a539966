// csrc/png_tokens_core.h on the CPU, as a program of its own (tests/test_pngdx_cpu.py builds it with -fsanitize=address,undefined):
// libmdc_pngdx.so's rules in the order its kernels apply them -- classify and the stored chain (the front kernel), the token path for
// every other stream, the sequential decoder for what the token path gave up on, the Adler-32, the trailer, the filter types.
//
// The token path's team is a loop here: every phase runs for t = 0 .. 1023 before the next one starts, once in ascending and once in
// descending order of t.  Nothing a phase computes may depend on that order.
//
//   pngdx_core <corpus> <results>
//   corpus:  int32 count, then per stream int32 w, h, bytes and the bytes
//   results: text, per stream and order one line: index order(0 ascending, 1 descending) reason path end_byte hash, where end_byte is
//            the trailer's offset and hash the CRC-32 of the F filtered bytes (both 0 unless the stream inflated)
// Every buffer is a heap allocation of exactly the size the core may touch: a read or write outside it is a sanitizer report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "png_tokens_core.h"

namespace {

struct SeqOut {
  uint8_t* out;
  uint32_t pos;
  bool builder() const { return true; }
  void barrier() const {}
  void put(uint8_t v) { out[pos++] = v; }
  void copy(uint32_t dist, uint32_t len) {
    for (uint32_t i = 0; i < len; i++, pos++) out[pos] = out[pos - dist];
  }
  void stored(const uint8_t* src, uint32_t len) {
    memcpy(out + pos, src, len);
    pos += len;
  }
};

struct LoopTeam {
  bool descending;
  template <class Fn>
  void each(Fn fn) const {
    for (int k = 0; k < pngx::kThreads; k++) fn(descending ? pngx::kThreads - 1 - k : k);
  }
  template <class Fn>
  bool each_or(Fn fn) const {
    bool any = false;
    for (int k = 0; k < pngx::kThreads; k++) any = fn(descending ? pngx::kThreads - 1 - k : k) || any;
    return any;
  }
};

bool read_i32(FILE* f, int32_t* v) { return fread(v, 4, 1, f) == 1; }

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: pngdx_core <corpus> <results>\n");
    return 2;
  }
  FILE* in = fopen(argv[1], "rb");
  FILE* res = fopen(argv[2], "w");
  int32_t count = 0;
  if (!in || !res || !read_i32(in, &count)) return 2;
  pngx::Shared* S = new pngx::Shared;
  for (int32_t k = 0; k < count; k++) {
    int32_t w, h, bytes;
    if (!read_i32(in, &w) || !read_i32(in, &h) || !read_i32(in, &bytes) || w < 1 || h < 1 || bytes < 0) return 2;
    uint8_t* p = (uint8_t*)malloc(bytes ? (size_t)bytes : 1);  // exactly the stream
    if (bytes && fread(p, 1, (size_t)bytes, in) != (size_t)bytes) return 2;
    const uint32_t n = (uint32_t)bytes, rs = 1u + (uint32_t)w, F = rs * (uint32_t)h;
    for (int order = 0; order < 2; order++) {
      uint8_t* filt = (uint8_t*)malloc(F);  // exactly F
      uint32_t* src = (uint32_t*)malloc((size_t)F * 4);
      memset(S, 0xa5, sizeof *S);
      memset(filt, 0xa5, F);
      memset(src, 0xa5, (size_t)F * 4);
      uint32_t data_bit = 0, end_byte = 0;
      int path = pngd::classify(S->w, p, n, &data_bit);
      if (path == pngd::PATH_STORED) {
        uint32_t bs[pngd::kMaxStoredBlocks], bd[pngd::kMaxStoredBlocks], bl[pngd::kMaxStoredBlocks], nblk = 0, e = 0;
        if (!pngd::stored_chain(p, n, F, bs, bd, bl, &nblk, &e)) path = pngd::PATH_GENERAL;
      }
      int st = pngd::ST_OK;
      bool inflated = false;
      if (path == pngd::PATH_GENERAL) {  // not the front kernel's: the token path first
        const LoopTeam team = {order == 1};
        const pngx::Image im = {p, n, F, filt, src};
        if (pngx::decode_image(team, *S, im, &end_byte)) path = pngx::PATH_TOKENS, inflated = true;
      }
      if (!inflated) {  // (the front kernel's paths write what the sequential decoder writes: tests/test_pngd_cpu.py)
        SeqOut out = {filt, 0};
        st = pngd::inflate(S->w, p, n, out, F, &end_byte);
        if (st != pngd::ST_OK) path = pngd::PATH_GENERAL;
      }
      uint32_t hash = 0;
      if (st == pngd::ST_OK) {
        uint64_t s1 = 0, s2 = 0;
        uint32_t crc = 0xffffffffu;
        for (uint32_t i = 0; i < F; i++) {
          s1 += filt[i];
          s2 = (s2 + (uint64_t)(F - i) * filt[i]) % pngd::kAdlerMod;
          crc ^= filt[i];
          for (int b = 0; b < 8; b++) crc = (crc >> 1) ^ (0xedb88320u & (0u - (crc & 1u)));
        }
        hash = crc ^ 0xffffffffu;
        st = pngd::check_trailer(p, n, end_byte, pngd::adler_of(s1, s2, F));
      } else {
        end_byte = 0;
      }
      if (st == pngd::ST_OK)
        for (int32_t r = 0; r < h; r++)
          if (filt[(size_t)r * rs] > 4) st = pngd::ST_FILTER_TYPE;
      if (st != pngd::ST_OK && path == pngx::PATH_TOKENS) path = pngd::PATH_GENERAL;  // pngdx_settle_kernel
      fprintf(res, "%d %d %d %d %u %u\n", (int)k, order, st, path, end_byte, hash);
      free(src);
      free(filt);
    }
    free(p);
  }
  delete S;
  fclose(in);
  return fclose(res) == 0 ? 0 : 2;
}
