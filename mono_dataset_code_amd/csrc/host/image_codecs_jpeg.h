// What the three JPEG readers share (image_codecs_jpeg.cpp: baseline and progressive decoder; image_codecs_jpeg_stream.cpp: the
// device's Huffman stream): the walk from marker to marker, the tables and the frame header a file defines, the Huffman table and
// the bit reader.  This code reports what a file says; whether that is acceptable, and the words to refuse it with, is each
// reader's own (decode_pool.cpp falls from one reader to the next where one refuses).  Header-only: the decoders' inner loops
// inline Bits and decode_sym.  Not installed.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace mdc_host {
namespace jpeg {

static const unsigned char kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                          41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                          30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Huff {
  bool present = false;
  unsigned char vals[256];
  uint16_t look[512];  // codes of <= 9 bits: (length << 8) | symbol, 0 = longer code
  int maxcode[18];     // largest code of length l (or -1), maxcode[17] = sentinel
  int valoff[17];      // vals index of the first code of length l minus that code
  // AC tables only: for a 9-bit window that holds a whole (code, magnitude bits) pair: value << 8 | run << 4 | bits used;
  // 0 = not such a window (long code, long magnitude, EOB or ZRL)
  int16_t fast_ac[512];
  unsigned char def[16 + 256];  // the table as the file defines it (16 counts + the symbols): identity of the table
  int def_len = 0;
};

inline bool build_huff(Huff& t, const unsigned char* bits /*[1..16] at bits[0..15]*/, const unsigned char* vals, int nvals) {
  memset(t.look, 0, sizeof t.look);
  memcpy(t.vals, vals, (size_t)nvals);
  memcpy(t.def, bits, 16);
  memcpy(t.def + 16, vals, (size_t)nvals);
  t.def_len = 16 + nvals;
  int code = 0, k = 0;
  for (int l = 1; l <= 16; l++) {
    t.valoff[l] = k - code;
    const int cnt = bits[l - 1];
    if (k + cnt > 256 || code + cnt > (1 << l)) return false;
    for (int i = 0; i < cnt; i++, k++, code++)
      if (l <= 9) {
        const int first = code << (9 - l);
        for (int f = 0; f < (1 << (9 - l)); f++) t.look[first + f] = (uint16_t)(l << 8 | vals[k]);
      }
    t.maxcode[l] = cnt ? code - 1 : -1;
    code <<= 1;
  }
  t.maxcode[17] = 0x7fffffff;
  t.present = k == nvals;
  for (int w = 0; w < 512; w++) {
    t.fast_ac[w] = 0;
    const int e = t.look[w];
    if (!e) continue;
    const int len = e >> 8, rs = e & 255, run = rs >> 4, sz = rs & 15;
    if (sz == 0 || len + sz > 9) continue;
    int v = (w >> (9 - len - sz)) & ((1 << sz) - 1);  // the magnitude bits that follow the code inside the window
    if (v < (1 << (sz - 1))) v += (int)((~0u) << sz) + 1;  // EXTEND
    if (v >= -128 && v <= 127) t.fast_ac[w] = (int16_t)(v * 256 + run * 16 + (len + sz));
  }
  return t.present;
}

struct Bits {  // entropy-coded segment reader: FF00 unstuffing, stops (feeding zeros) at a marker
  const unsigned char* p;
  const unsigned char* end;
  uint64_t acc = 0;
  int cnt = 0;
  bool hit_marker = false;
  void fill() {
    while (cnt <= 56) {
      unsigned b = 0;
      if (!hit_marker && p < end) {
        b = *p;
        if (b == 0xff) {
          if (p + 1 < end && p[1] == 0) p += 2;
          else {
            hit_marker = true;
            b = 0;
          }
        } else p++;
      }
      acc |= (uint64_t)b << (56 - cnt);
      cnt += 8;
    }
  }
  int peek(int n) { return (int)(acc >> (64 - n)); }
  void skip(int n) {
    acc <<= n;
    cnt -= n;
  }
  int get(int n) {
    if (n == 0) return 0;
    if (cnt < n) fill();
    const int v = peek(n);
    skip(n);
    return v;
  }
  // RSTn: on to the byte after the next restart marker (false: there is none)
  bool restart() {
    const unsigned char* q = p;
    while (q + 1 < end && !(q[0] == 0xff && q[1] >= 0xd0 && q[1] <= 0xd7)) q++;
    if (q + 1 >= end) return false;
    p = q + 2;
    acc = 0;
    cnt = 0;
    hit_marker = false;
    return true;
  }
};

inline int decode_sym(Bits& b, const Huff& t) {
  if (b.cnt < 16) b.fill();
  const int e = t.look[b.peek(9)];
  if (e) {
    b.skip(e >> 8);
    return e & 255;
  }
  int code = b.peek(10), l = 10;
  while (code > t.maxcode[l]) {
    if (++l > 16) return -1;
    code = b.peek(l);
  }
  b.skip(l);
  const int idx = code + t.valoff[l];
  return (idx >= 0 && idx < 256) ? t.vals[idx] : -1;
}

inline int extend(int v, int t) { return v < (1 << (t - 1)) ? v - (1 << t) + 1 : v; }

struct Comp {
  int id = 0, h = 1, v = 1, tq = 0;  // the frame header's
  int td = 0, ta = 0, pred = 0;      // a scan's: the decoder's to fill and use
};

// What the segments before a scan define.  A read_* function returns nullptr, or what is wrong with the segment.
struct Header {
  uint16_t qt[4][64];  // natural order
  bool have_qt[4] = {false, false, false, false};
  Huff dc[4], ac[4];
  bool have_sof = false;
  int W = 0, H = 0, ncomp = 0;
  Comp comp[4];
  int restart = 0;
  bool jfif = false, adobe = false;
  int adobe_transform = 0;

  // Colour space of a three-component file as libjpeg decides it (jdapimin.c: default_decompress_parms): a JFIF marker means YCbCr;
  // else an Adobe marker's transform byte (0 = RGB, 1 = YCbCr); else the component ids (1 2 3 = YCbCr, 'R' 'G' 'B' = RGB); else YCbCr.
  // For an RGB file cv::imread(..., GRAYSCALE) returns 0.299 R + 0.587 G + 0.114 B (libjpeg's rgb_gray_convert), not component 0.
  bool is_rgb() const {
    if (ncomp != 3 || jfif) return false;
    if (adobe) return adobe_transform == 0;
    return comp[0].id == 'R' && comp[1].id == 'G' && comp[2].id == 'B';
  }

  // DQT, DHT, DRI, APP0 and APP14: taken in; any other segment is left to the caller
  const char* read_tables(int m, const unsigned char* s, size_t sl) {
    if (m == 0xdb) return read_dqt(s, sl);
    if (m == 0xc4) return read_dht(s, sl);
    if (m == 0xdd && sl >= 2) restart = s[0] << 8 | s[1];
    if (m == 0xe0 && sl >= 14 && s[0] == 'J' && s[1] == 'F' && s[2] == 'I' && s[3] == 'F' && s[4] == 0) jfif = true;
    if (m == 0xee && sl >= 12 && s[0] == 'A' && s[1] == 'd' && s[2] == 'o' && s[3] == 'b' && s[4] == 'e') {
      adobe = true;
      adobe_transform = s[11];
    }
    return nullptr;
  }
  const char* read_dqt(const unsigned char* s, size_t sl) {
    size_t q = 0;
    while (q < sl) {
      const int pq = s[q] >> 4, tq = s[q] & 15;
      q++;
      if (tq > 3 || q + (pq ? 128 : 64) > sl) return "JPEG: bad DQT";
      for (int i = 0; i < 64; i++, q += pq ? 2 : 1) qt[tq][kZigzag[i]] = pq ? (uint16_t)(s[q] << 8 | s[q + 1]) : s[q];
      have_qt[tq] = true;
    }
    return nullptr;
  }
  const char* read_dht(const unsigned char* s, size_t sl) {
    size_t q = 0;
    while (q + 17 <= sl) {
      const int tc = s[q] >> 4, th = s[q] & 15;
      int cnt = 0;
      for (int i = 0; i < 16; i++) cnt += s[q + 1 + i];
      if (th > 3 || tc > 1 || cnt > 256 || q + 17 + (size_t)cnt > sl) return "JPEG: bad DHT";
      if (!build_huff(tc ? ac[th] : dc[th], s + q + 1, s + q + 17, cnt)) return "JPEG: bad Huffman table";
      q += 17 + (size_t)cnt;
    }
    return nullptr;
  }
  // Frame header of 8-bit samples, one or three components; `unsupported` is the reader's own text for any other component count.
  const char* read_sof(const unsigned char* s, size_t sl, const char* unsupported) {
    if (sl < 6 || s[0] != 8) return "JPEG: only 8-bit samples are supported";
    H = s[1] << 8 | s[2];
    W = s[3] << 8 | s[4];
    ncomp = s[5];
    if ((ncomp != 1 && ncomp != 3) || sl < 6 + 3 * (size_t)ncomp || W <= 0 || H <= 0) return unsupported;
    for (int i = 0; i < ncomp; i++) {
      comp[i].id = s[6 + 3 * i];
      comp[i].h = s[7 + 3 * i] >> 4;
      comp[i].v = s[7 + 3 * i] & 15;
      comp[i].tq = s[8 + 3 * i] & 3;
      if (comp[i].h < 1 || comp[i].h > 4 || comp[i].v < 1 || comp[i].v > 4) return "JPEG: bad sampling factors";
    }
    have_sof = true;
    return nullptr;
  }
};

// a frame header of any kind (SOF0 .. SOF15; C4, C8 and CC are DHT, JPG and DAC)
inline bool is_sof(int m) { return m >= 0xc0 && m <= 0xcf && m != 0xc4 && m != 0xc8 && m != 0xcc; }

// From marker to marker through the segments of a file (after SOI).  next() -> true: `marker` with its payload s[0..sl) -- a
// restart marker met between segments comes with sl = 0; false: the end of the file or EOI (error == nullptr), or a malformed
// file (error says how).  SOI, TEM and fill bytes are passed over.
struct Segments {
  const unsigned char* d;
  size_t n;
  // where the next marker is looked for: the byte after the segment next() returned -- after SOS that is the entropy-coded data,
  // and a reader that goes on to further segments moves p past them
  size_t p = 2;
  int marker = 0;
  const unsigned char* s = nullptr;
  size_t sl = 0;
  const char* error = nullptr;
  Segments(const unsigned char* data, size_t size) : d(data), n(size) {}

  bool next() {
    for (;;) {
      if (p + 4 > n) return false;
      if (d[p] != 0xff) return error = "JPEG: marker expected", false;
      while (p < n && d[p] == 0xff) p++;  // fill bytes
      if (p >= n) return false;
      marker = d[p++];
      if (marker == 0xd8 || marker == 0x01) continue;
      if (marker == 0xd9) return false;
      s = d + p;
      sl = 0;
      if (marker >= 0xd0 && marker <= 0xd7) return true;
      if (p + 2 > n) return error = "JPEG: truncated", false;
      const size_t len = (size_t)d[p] << 8 | d[p + 1];
      if (len < 2 || p + len > n) return error = "JPEG: bad segment length", false;
      s = d + p + 2;
      sl = len - 2;
      p += len;
      return true;
    }
  }
};

}  // namespace jpeg
}  // namespace mdc_host
