// PNG on the host, what cv::imread(..., CV_LOAD_IMAGE_GRAYSCALE) accepts for a frame (reference
// src/BenchmarkDatasetReader.h:252,274) and cv::imread(..., CV_LOAD_IMAGE_UNCHANGED) for the vignette
// (src/PhotometricUndistorter.cpp:120), without OpenCV:
//
//   every colour type (gray, gray + alpha, RGB, RGBA, palette), every bit depth (1, 2, 4, 8, 16), Adam7 interlacing.
//   Conversion to 8-bit gray as OpenCV's PNG reader configures libpng for a grayscale read:
//     16-bit samples      -> the high byte                 (png_set_strip_16; after the colour conversion)
//     alpha               -> dropped                       (png_set_strip_alpha)
//     1/2/4-bit gray      -> scaled to 8 bits (x 255, 85, 17)  (png_set_expand_gray_1_2_4_to_8)
//     palette             -> RGB, then as RGB              (png_set_palette_to_rgb)
//     RGB                 -> libpng's png_set_rgb_to_gray(1, 0.299, 0.587): 15-bit fixed point with TRUNCATED
//                            coefficients 9797 / 19234 / 3737 (sum 32768); 8-bit samples
//                            (9797 R + 19234 G + 3737 B) >> 15 (no rounding), 16-bit samples + 16384 before the
//                            shift; R == G == B passes through.  (Not PIL's "L": (19595 R + 38470 G + 7471 B
//                            + 32768) >> 16 -- the two differ by at most 1; tests/test_reader_cpu.py states both.)
//   The common case -- 8-bit gray, non-interlaced, what the dataset's lossless frames are -- is decoded in place (png_gray8).
#include <zlib.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "image_codecs.h"
#include "image_codecs_internal.h"

namespace mdc_host {
namespace {

unsigned be32(const unsigned char* p) { return (unsigned)p[0] << 24 | (unsigned)p[1] << 16 | (unsigned)p[2] << 8 | p[3]; }

// What the chunks of a file say; whether that is acceptable is the decoder's to decide.
struct PngChunks {
  bool have_ihdr = false;
  unsigned W = 0, H = 0;
  int depth = 0, ctype = -1, interlace = 0;
  bool method_bytes = false;  // an IHDR named a compression or filter method other than 0
  bool truncated = false;     // a chunk runs past the end of the file: the walk ended there
};
// Walks the chunks up to IEND: the IHDR fields, the IDAT bodies appended to `idat`, the last PLTE body in *plte (where asked for).
PngChunks png_chunks(const unsigned char* d, size_t n, std::vector<unsigned char>& idat, std::vector<unsigned char>* plte) {
  PngChunks c;
  size_t pos = 8;
  while (pos + 12 <= n) {
    const unsigned len = be32(d + pos);
    const unsigned char* tag = d + pos + 4;
    if (len > n || pos + 12 + (size_t)len > n) {
      c.truncated = true;
      break;
    }
    const unsigned char* body = d + pos + 8;
    if (!memcmp(tag, "IHDR", 4) && len >= 13) {
      c.have_ihdr = true;
      c.W = be32(body);
      c.H = be32(body + 4);
      c.depth = body[8];
      c.ctype = body[9];
      c.interlace = body[12];
      if (body[10] != 0 || body[11] != 0) c.method_bytes = true;
    } else if (!memcmp(tag, "PLTE", 4)) {
      if (plte) plte->assign(body, body + len);
    } else if (!memcmp(tag, "IDAT", 4)) {
      idat.insert(idat.end(), body, body + len);
    } else if (!memcmp(tag, "IEND", 4)) {
      break;
    }
    pos += 12 + (size_t)len;
  }
  return c;
}

int paeth(int a, int b, int c) {
  const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// One row: `n` filtered bytes at `in` -> `cur`; `prev` = the row above (nullptr: there is none), bpp = bytes per pixel (at least 1).
// false: no such filter type.
bool png_unfilter_row(int ft, const unsigned char* in, const unsigned char* prev, unsigned char* cur, size_t n, size_t bpp) {
  // a = the byte one pixel to the left, b = the byte above, c = the byte above a; 0 where there is none
  switch (ft) {
    case 0: memcpy(cur, in, n); return true;
    case 1:
      for (size_t i = 0; i < n; i++) cur[i] = (unsigned char)(in[i] + (i >= bpp ? cur[i - bpp] : 0));
      return true;
    case 2:
      for (size_t i = 0; i < n; i++) cur[i] = (unsigned char)(in[i] + (prev ? prev[i] : 0));
      return true;
    case 3:
      for (size_t i = 0; i < n; i++) {
        const int a = i >= bpp ? cur[i - bpp] : 0, b = prev ? prev[i] : 0;
        cur[i] = (unsigned char)(in[i] + ((a + b) >> 1));
      }
      return true;
    case 4:
      for (size_t i = 0; i < n; i++) {
        const int a = i >= bpp ? cur[i - bpp] : 0, b = prev ? prev[i] : 0, c = (i >= bpp && prev) ? prev[i - bpp] : 0;
        cur[i] = (unsigned char)(in[i] + paeth(a, b, c));
      }
      return true;
    default: return false;
  }
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------
// 8-bit grayscale, non-interlaced: decoded in place; every other flavour through the general decoder
// ---------------------------------------------------------------------------------------------------------
bool png_gray8(const unsigned char* d, size_t n, unsigned char* out, size_t cap, int* w, int* h, std::string* err) {
  // scratch that survives between frames of one thread: fresh multi-megabyte vectors per frame mean an mmap, page
  // faults and an munmap each, and the kernel's address-space lock then serialises the decode threads
  static thread_local std::vector<unsigned char> idat, raw;
  idat.clear();
  const PngChunks c = png_chunks(d, n, idat, nullptr);  // (the method bytes are not looked at here)
  if (c.truncated) return fail(err, "PNG: truncated chunk");
  const unsigned W = c.W, H = c.H;
  if (W == 0 || H == 0 || W > 65535 || H > 65535) return fail(err, "PNG: no IHDR");
  *w = (int)W;
  *h = (int)H;
  if ((size_t)W * H > cap) return fail(err, "frame larger than the buffer");
  if (c.ctype != 0 || c.depth != 8 || c.interlace != 0) {  // any other PNG flavour: general decoder + OpenCV's conversion to 8-bit gray
    PngAny im;
    if (!png_decode_any(d, n, im, err)) return false;
    png_any_to_gray8(im, out);
    return true;
  }
  const size_t stride = W;
  raw.resize((stride + 1) * H);
  uLongf got = (uLongf)raw.size();
  if (uncompress(raw.data(), &got, idat.data(), (uLong)idat.size()) != Z_OK || got != raw.size()) return fail(err, "PNG: bad IDAT stream");
  for (unsigned y = 0; y < H; y++) {
    const unsigned char* line = &raw[(stride + 1) * y];
    unsigned char* cur = out + (size_t)y * W;
    if (!png_unfilter_row(line[0], line + 1, y ? cur - W : nullptr, cur, stride, 1)) return fail(err, "PNG: bad filter type");
  }
  return true;
}

bool png_stream(const unsigned char* d, size_t n, unsigned char* stream, size_t cap, size_t* used, int* w, int* h, std::string* err) {
  static thread_local std::vector<unsigned char> idat;
  idat.clear();
  if (n < 8 || memcmp(d, "\x89PNG\r\n\x1a\n", 8) != 0) return fail(err, "PNG: no signature");
  const PngChunks c = png_chunks(d, n, idat, nullptr);
  if (c.truncated) return fail(err, "PNG: truncated chunk");
  if (!c.have_ihdr || c.W == 0 || c.H == 0 || c.W > 65535 || c.H > 65535) return fail(err, "PNG: no IHDR");
  if (c.ctype != 0 || c.depth != 8 || c.interlace != 0) return fail(err, "PNG: not 8-bit grayscale, non-interlaced");
  if (!stream || idat.size() > cap) return fail(err, "PNG: the stream does not fit the buffer");
  if (!idat.empty()) memcpy(stream, idat.data(), idat.size());
  *used = idat.size();
  *w = (int)c.W;
  *h = (int)c.H;
  return true;
}

// ---------------------------------------------------------------------------------------------------------
// PNG, general
// ---------------------------------------------------------------------------------------------------------
bool png_decode_any(const unsigned char* d, size_t n, PngAny& im, std::string* err) {
  im = PngAny();
  std::vector<unsigned char> idat, plte;
  const PngChunks c = png_chunks(d, n, idat, &plte);
  if (c.method_bytes) return fail(err, "PNG: unknown compression / filter method");
  if (c.truncated) return fail(err, "PNG: truncated chunk");
  const unsigned W = c.W, H = c.H;
  const int depth = c.depth, ctype = c.ctype, interlace = c.interlace;
  if (!c.have_ihdr || W == 0 || H == 0 || W > 65535 || H > 65535) return fail(err, "PNG: no IHDR");
  im.w = (int)W;
  im.h = (int)H;
  int fch;  // channels in the file
  switch (ctype) {
    case 0: fch = 1; if (depth != 1 && depth != 2 && depth != 4 && depth != 8 && depth != 16) return fail(err, "PNG: bad bit depth"); break;
    case 2: fch = 3; if (depth != 8 && depth != 16) return fail(err, "PNG: bad bit depth"); break;
    case 3: fch = 1; if (depth != 1 && depth != 2 && depth != 4 && depth != 8) return fail(err, "PNG: bad bit depth"); break;
    case 4: fch = 2; if (depth != 8 && depth != 16) return fail(err, "PNG: bad bit depth"); break;
    case 6: fch = 4; if (depth != 8 && depth != 16) return fail(err, "PNG: bad bit depth"); break;
    default: return fail(err, "PNG: bad colour type");
  }
  if (interlace > 1) return fail(err, "PNG: bad interlace method");
  if (ctype == 3 && plte.size() < 3) return fail(err, "PNG: palette image without PLTE");
  im.channels = ctype == 3 ? 3 : fch;
  im.bits = depth == 16 ? 16 : 8;
  im.palette = ctype == 3;
  if ((size_t)W * H * (size_t)im.channels > ((size_t)1 << 28)) return fail(err, "PNG: image too large");
  // passes: non-interlaced = one pass over the whole image
  static const int X0[7] = {0, 4, 0, 2, 0, 1, 0}, Y0[7] = {0, 0, 4, 0, 2, 0, 1}, DX[7] = {8, 8, 4, 4, 2, 2, 1}, DY[7] = {8, 8, 8, 4, 4, 2, 2};
  const int npass = interlace ? 7 : 1;
  size_t total = 0;
  unsigned pw[7], ph[7];
  for (int p = 0; p < npass; p++) {
    pw[p] = interlace ? (W + DX[p] - 1 - X0[p]) / DX[p] : W;
    ph[p] = interlace ? (H + DY[p] - 1 - Y0[p]) / DY[p] : H;
    if (interlace && ((unsigned)X0[p] >= W || (unsigned)Y0[p] >= H)) pw[p] = ph[p] = 0;
    if (pw[p] && ph[p]) total += (size_t)ph[p] * (1 + ((size_t)pw[p] * fch * depth + 7) / 8);
  }
  std::vector<unsigned char> raw(total);
  uLongf got = (uLongf)raw.size();
  if (idat.empty() || uncompress(raw.data(), &got, idat.data(), (uLong)idat.size()) != Z_OK || got != raw.size())
    return fail(err, "PNG: bad IDAT stream");
  im.px.assign((size_t)W * H * im.channels, 0);
  const size_t bpp = std::max<size_t>(1, (size_t)fch * depth / 8);
  size_t off = 0;
  std::vector<unsigned char> prev, cur;
  for (int p = 0; p < npass; p++) {
    if (!pw[p] || !ph[p]) continue;
    const size_t stride = ((size_t)pw[p] * fch * depth + 7) / 8;
    prev.assign(stride, 0);
    cur.assign(stride, 0);
    for (unsigned y = 0; y < ph[p]; y++) {
      const unsigned char* line = &raw[off];
      off += stride + 1;
      if (!png_unfilter_row(line[0], line + 1, prev.data(), cur.data(), stride, bpp)) return fail(err, "PNG: bad filter type");
      const size_t oy = interlace ? (size_t)Y0[p] + (size_t)y * DY[p] : y;
      for (unsigned x = 0; x < pw[p]; x++) {
        const size_t ox = interlace ? (size_t)X0[p] + (size_t)x * DX[p] : x;
        uint16_t* o = &im.px[(oy * W + ox) * im.channels];
        if (depth == 16) {
          for (int ch = 0; ch < fch; ch++) o[ch] = (uint16_t)(cur[((size_t)x * fch + ch) * 2] << 8 | cur[((size_t)x * fch + ch) * 2 + 1]);
        } else if (depth == 8) {
          if (ctype == 3) {
            const size_t idx = cur[x];
            if (idx * 3 + 2 >= plte.size()) return fail(err, "PNG: palette index out of range");
            o[0] = plte[idx * 3];
            o[1] = plte[idx * 3 + 1];
            o[2] = plte[idx * 3 + 2];
          } else {
            for (int ch = 0; ch < fch; ch++) o[ch] = cur[(size_t)x * fch + ch];
          }
        } else {  // 1, 2, 4 bits: one channel (gray or palette index), most significant bits first
          const size_t bit = (size_t)x * depth;
          const unsigned v = (cur[bit >> 3] >> (8 - depth - (bit & 7))) & ((1u << depth) - 1);
          if (ctype == 3) {
            if ((size_t)v * 3 + 2 >= plte.size()) return fail(err, "PNG: palette index out of range");
            o[0] = plte[v * 3];
            o[1] = plte[v * 3 + 1];
            o[2] = plte[v * 3 + 2];
          } else {
            o[0] = (uint16_t)(v * (255u / ((1u << depth) - 1)));  // x 255, 85, 17
          }
        }
      }
      prev.swap(cur);
    }
  }
  return true;
}

// 8-bit gray as OpenCV's grayscale read of that PNG (see the file comment)
void png_any_to_gray8(const PngAny& im, unsigned char* out) {
  const size_t npx = (size_t)im.w * im.h;
  const int ch = im.channels;
  for (size_t i = 0; i < npx; i++) {
    const uint16_t* s = &im.px[i * ch];
    unsigned v;
    if (ch <= 2) {
      v = s[0];
    } else {
      const unsigned r = s[0], g = s[1], b = s[2];
      if (r == g && r == b) v = r;
      else if (im.bits == 16) v = (9797u * r + 19234u * g + 3737u * b + 16384u) >> 15;
      else v = (9797u * r + 19234u * g + 3737u * b) >> 15;
    }
    out[i] = (unsigned char)(im.bits == 16 ? v >> 8 : v);
  }
}

}  // namespace mdc_host
