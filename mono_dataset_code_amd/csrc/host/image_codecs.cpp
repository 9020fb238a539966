#include "image_codecs.h"
#include "image_codecs_internal.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace mdc_host {

bool read_file(const std::string& path, std::vector<unsigned char>& buf) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return false;
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  if (n < 0) {
    fclose(f);
    return false;
  }
  buf.resize((size_t)n);
  const bool ok = n == 0 || fread(buf.data(), 1, (size_t)n, f) == (size_t)n;
  fclose(f);
  return ok;
}

namespace {

// ---------------------------------------------------------------------------------------------
// PGM (P5, maxval <= 255)
// ---------------------------------------------------------------------------------------------
bool pgm_gray8(const unsigned char* d, size_t n, unsigned char* out, size_t cap, int* w, int* h, std::string* err) {
  // header: "P5" ws width ws height ws maxval single-ws, '#' comments allowed between tokens
  size_t p = 2;
  int vals[3] = {0, 0, 0};
  for (int k = 0; k < 3; k++) {
    for (;;) {
      while (p < n && (d[p] == ' ' || d[p] == '\t' || d[p] == '\r' || d[p] == '\n')) p++;
      if (p < n && d[p] == '#') {
        while (p < n && d[p] != '\n') p++;
        continue;
      }
      break;
    }
    if (p >= n || d[p] < '0' || d[p] > '9') return fail(err, "PGM: bad header");
    long v = 0;
    while (p < n && d[p] >= '0' && d[p] <= '9' && v < 100000000) v = v * 10 + (d[p++] - '0');
    vals[k] = (int)v;
  }
  p++;  // the single whitespace byte after maxval
  if (vals[0] <= 0 || vals[1] <= 0) return fail(err, "PGM: bad size");
  *w = vals[0];
  *h = vals[1];
  if (vals[2] != 65535 && (vals[2] > 255 || vals[2] <= 0)) return fail(err, "PGM: only maxval <= 255 or 65535 is supported");
  const size_t px = (size_t)vals[0] * vals[1];
  if (px > cap) return fail(err, "frame larger than the buffer");
  if (vals[2] == 65535) {  // 16-bit samples (big endian): the high byte, as OpenCV's 8-bit read of such a file
    if (p + 2 * px > n) return fail(err, "PGM: truncated");
    for (size_t i = 0; i < px; i++) out[i] = d[p + 2 * i];
    return true;
  }
  if (p + px > n) return fail(err, "PGM: truncated");
  memcpy(out, d + p, px);
  return true;
}

}  // namespace

bool decode_gray8(const unsigned char* d, size_t n, unsigned char* out, size_t cap, int* w, int* h, std::string* err) {
  *w = *h = 0;
  static const unsigned char png_sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
  if (n >= 16 && !memcmp(d, png_sig, 8)) return png_gray8(d, n, out, cap, w, h, err);
  if (n >= 4 && d[0] == 0xff && d[1] == 0xd8) return jpeg_gray8(d, n, out, cap, w, h, err);
  if (n >= 8 && d[0] == 'P' && d[1] == '5') return pgm_gray8(d, n, out, cap, w, h, err);
  return fail(err, "unknown image format (PNG, PGM P5 and JPEG are supported)");
}

}  // namespace mdc_host
