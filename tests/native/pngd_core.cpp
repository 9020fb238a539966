// csrc/png_inflate_core.h on the CPU, as a program of its own (tests/test_pngd_cpu.py builds it with -fsanitize=address,undefined):
// the device decoder's rules -- classify, the stored chain, inflate, the Adler-32, the trailer, the filter types, the per-pixel unfilter --
// in the order the kernels of csrc/mdc_pngd.hip apply them, one stream after another.
//
//   pngd_core <corpus> <results>
//   corpus:  int32 count, then per stream int32 w, h, bytes and the bytes
//   results: per stream int32 reason, path, then (reason 0) the w * h pixels
// Every buffer is a heap allocation of exactly the size the core may touch: a read or write outside it is a sanitizer report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "png_inflate_core.h"

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

bool read_i32(FILE* f, int32_t* v) { return fread(v, 4, 1, f) == 1; }

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: pngd_core <corpus> <results>\n");
    return 2;
  }
  FILE* in = fopen(argv[1], "rb");
  FILE* res = fopen(argv[2], "wb");
  int32_t count = 0;
  if (!in || !res || !read_i32(in, &count)) return 2;
  pngd::Work* work = new pngd::Work;
  for (int32_t k = 0; k < count; k++) {
    int32_t w, h, bytes;
    if (!read_i32(in, &w) || !read_i32(in, &h) || !read_i32(in, &bytes) || w < 1 || h < 1 || bytes < 0) return 2;
    uint8_t* p = (uint8_t*)malloc(bytes ? (size_t)bytes : 1);  // exactly the stream
    if (bytes && fread(p, 1, (size_t)bytes, in) != (size_t)bytes) return 2;
    const uint32_t n = (uint32_t)bytes, rs = 1u + (uint32_t)w, F = rs * (uint32_t)h;
    uint8_t* filt = (uint8_t*)malloc(F);  // exactly F
    memset(work, 0xa5, sizeof *work);
    uint32_t data_bit = 0, end_byte = 0;
    int path = pngd::classify(*work, p, n, &data_bit);
    if (path == pngd::PATH_STORED) {
      uint32_t src[pngd::kMaxStoredBlocks], dst[pngd::kMaxStoredBlocks], len[pngd::kMaxStoredBlocks], nblk = 0, e = 0;
      if (!pngd::stored_chain(p, n, F, src, dst, len, &nblk, &e)) path = pngd::PATH_GENERAL;
    }
    SeqOut out = {filt, 0};
    int st = pngd::inflate(*work, p, n, out, F, &end_byte);
    if (st != pngd::ST_OK) path = pngd::PATH_GENERAL;  // whatever one of the other paths gives up on, the sequential decoder decides
    if (st == pngd::ST_OK) {
      uint64_t s1 = 0, s2 = 0;
      for (uint32_t i = 0; i < F; i++) {
        s1 += filt[i];
        s2 = (s2 + (uint64_t)(F - i) * filt[i]) % pngd::kAdlerMod;
      }
      st = pngd::check_trailer(p, n, end_byte, pngd::adler_of(s1, s2, F));
    }
    if (st == pngd::ST_OK)
      for (int32_t r = 0; r < h; r++)
        if (filt[(size_t)r * rs] > 4) st = pngd::ST_FILTER_TYPE;
    const int32_t head[2] = {st, path};
    fwrite(head, 4, 2, res);
    if (st == pngd::ST_OK) {
      uint8_t* px = (uint8_t*)malloc((size_t)w * h);
      for (int32_t r = 0; r < h; r++)
        for (int32_t c = 0; c < w; c++) {
          const int a = c ? px[(size_t)r * w + c - 1] : 0, b = r ? px[(size_t)(r - 1) * w + c] : 0, cc = (r && c) ? px[(size_t)(r - 1) * w + c - 1] : 0;
          px[(size_t)r * w + c] = (uint8_t)pngd::unfilter_px(filt[(size_t)r * rs], filt[(size_t)r * rs + 1 + c], a, b, cc);
        }
      fwrite(px, 1, (size_t)w * h, res);
      free(px);
    }
    free(filt);
    free(p);
  }
  delete work;
  fclose(in);
  return fclose(res) == 0 ? 0 : 2;
}
