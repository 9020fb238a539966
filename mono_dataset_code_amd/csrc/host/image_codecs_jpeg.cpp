// JPEG on the host: the baseline decoder (sequential DCT, Huffman, 8-bit; the dataset's lossy frames) and the progressive one
// (SOF2): spectral selection + successive approximation, DC / AC first and refinement scans, restart intervals; luma only for
// YCbCr files (libjpeg's JCS_GRAYSCALE), chroma-only scans are skipped, the interleaved DC scans are parsed for all components to
// stay in step.  Coefficients -> libjpeg's islow inverse DCT -> bit-identical to libjpeg / libjpeg-turbo.  Both also deliver the
// quantised luma coefficients without the inverse DCT (decode_jpeg_coefs).  Markers, tables and bits: image_codecs_jpeg.h.
#include <algorithm>
#include <cstdint>
#include <cstring>

#include "image_codecs.h"
#include "image_codecs_internal.h"
#include "image_codecs_jpeg.h"

namespace mdc_host {
namespace {

using namespace jpeg;

// libjpeg's jidctint.c ("islow"), 8x8: the accurate integer inverse DCT every libjpeg / libjpeg-turbo
// build uses by default -- same constants, same two passes, same rounding, so the samples agree bit for bit.
inline int descale(long x, int n) { return (int)((x + (1L << (n - 1))) >> n); }
inline unsigned char clamp_sample(int x) {
  x += 128;
  return (unsigned char)(x < 0 ? 0 : (x > 255 ? 255 : x));
}
void idct_islow(const int* coef /* dequantised, natural order */, unsigned char* out, size_t stride, bool dc_only) {
  if (dc_only) {  // both passes collapse: DESCALE(dc << 2, 5) everywhere (the shortcuts of jidctint.c applied twice)
    const unsigned char v = clamp_sample(descale((long)coef[0] * 4, 5));
    for (int r = 0; r < 8; r++) memset(out + (size_t)r * stride, v, 8);
    return;
  }
  const long F0_298 = 2446, F0_390 = 3196, F0_541 = 4433, F0_765 = 6270, F0_899 = 7373, F1_175 = 9633, F1_501 = 12299,
             F1_847 = 15137, F1_961 = 16069, F2_053 = 16819, F2_562 = 20995, F3_072 = 25172;
  const int CB = 13, P1 = 2;
  int ws[64];
  for (int c = 0; c < 8; c++) {
    const int* in = coef + c;
    if (!(in[8] | in[16] | in[24] | in[32] | in[40] | in[48] | in[56])) {
      const int dc = in[0] * (1 << P1);
      for (int r = 0; r < 8; r++) ws[r * 8 + c] = dc;
      continue;
    }
    long z2 = in[16], z3 = in[48];
    long z1 = (z2 + z3) * F0_541;
    long tmp2 = z1 + z3 * (-F1_847), tmp3 = z1 + z2 * F0_765;
    z2 = in[0];
    z3 = in[32];
    long tmp0 = (z2 + z3) * (1L << CB), tmp1 = (z2 - z3) * (1L << CB);
    const long tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = in[56];
    tmp1 = in[40];
    tmp2 = in[24];
    tmp3 = in[8];
    z1 = tmp0 + tmp3;
    z2 = tmp1 + tmp2;
    z3 = tmp0 + tmp2;
    long z4 = tmp1 + tmp3;
    const long z5 = (z3 + z4) * F1_175;
    tmp0 *= F0_298;
    tmp1 *= F2_053;
    tmp2 *= F3_072;
    tmp3 *= F1_501;
    z1 *= -F0_899;
    z2 *= -F2_562;
    z3 *= -F1_961;
    z4 *= -F0_390;
    z3 += z5;
    z4 += z5;
    tmp0 += z1 + z3;
    tmp1 += z2 + z4;
    tmp2 += z2 + z3;
    tmp3 += z1 + z4;
    ws[0 * 8 + c] = descale(tmp10 + tmp3, CB - P1);
    ws[7 * 8 + c] = descale(tmp10 - tmp3, CB - P1);
    ws[1 * 8 + c] = descale(tmp11 + tmp2, CB - P1);
    ws[6 * 8 + c] = descale(tmp11 - tmp2, CB - P1);
    ws[2 * 8 + c] = descale(tmp12 + tmp1, CB - P1);
    ws[5 * 8 + c] = descale(tmp12 - tmp1, CB - P1);
    ws[3 * 8 + c] = descale(tmp13 + tmp0, CB - P1);
    ws[4 * 8 + c] = descale(tmp13 - tmp0, CB - P1);
  }
  for (int r = 0; r < 8; r++) {
    const int* w = ws + r * 8;
    unsigned char* o = out + (size_t)r * stride;
    if (!(w[1] | w[2] | w[3] | w[4] | w[5] | w[6] | w[7])) {  // jidctint.c's row shortcut: same value as the full pass
      memset(o, clamp_sample(descale(w[0], 5)), 8);
      continue;
    }
    long z2 = w[2], z3 = w[6];
    long z1 = (z2 + z3) * F0_541;
    long tmp2 = z1 + z3 * (-F1_847), tmp3 = z1 + z2 * F0_765;
    long tmp0 = ((long)w[0] + w[4]) * (1L << CB), tmp1 = ((long)w[0] - w[4]) * (1L << CB);
    const long tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = w[7];
    tmp1 = w[5];
    tmp2 = w[3];
    tmp3 = w[1];
    z1 = tmp0 + tmp3;
    z2 = tmp1 + tmp2;
    z3 = tmp0 + tmp2;
    long z4 = tmp1 + tmp3;
    const long z5 = (z3 + z4) * F1_175;
    tmp0 *= F0_298;
    tmp1 *= F2_053;
    tmp2 *= F3_072;
    tmp3 *= F1_501;
    z1 *= -F0_899;
    z2 *= -F2_562;
    z3 *= -F1_961;
    z4 *= -F0_390;
    z3 += z5;
    z4 += z5;
    tmp0 += z1 + z3;
    tmp1 += z2 + z4;
    tmp2 += z2 + z3;
    tmp3 += z1 + z4;
    const int S = CB + P1 + 3;
    o[0] = clamp_sample(descale(tmp10 + tmp3, S));
    o[7] = clamp_sample(descale(tmp10 - tmp3, S));
    o[1] = clamp_sample(descale(tmp11 + tmp2, S));
    o[6] = clamp_sample(descale(tmp11 - tmp2, S));
    o[2] = clamp_sample(descale(tmp12 + tmp1, S));
    o[5] = clamp_sample(descale(tmp12 - tmp1, S));
    o[3] = clamp_sample(descale(tmp13 + tmp0, S));
    o[4] = clamp_sample(descale(tmp13 - tmp0, S));
  }
}

// ---------------------------------------------------------------------------------------------------------
// Progressive JPEG (luma only)
// ---------------------------------------------------------------------------------------------------------
bool jpeg_progressive_gray8(const unsigned char* d, size_t n, unsigned char* out, size_t cap, int* w, int* h, std::string* err, JpegCoefSink* sink) {
  Header hdr;
  Comp* const comp = hdr.comp;
  bool saw_luma_scan = false;
  int hmax = 1, vmax = 1, mx = 0, my = 0;  // MCU grid
  int lbw = 0, lbh = 0;                    // luma blocks: allocated grid (MCU padded)
  int lcw = 0, lch = 0;                    // luma blocks a non-interleaved luma scan covers
  std::vector<int16_t> coef;               // luma coefficients, [block][64] natural order
  Segments seg(d, n);
  while (seg.next()) {
    const int m = seg.marker;
    const unsigned char* const s = seg.s;
    const size_t sl = seg.sl;
    if (m >= 0xd0 && m <= 0xd7) continue;  // a restart marker between segments: passed over
    if (const char* bad = hdr.read_tables(m, s, sl)) return fail(err, bad);
    if (m == 0xc2) {
      if (const char* bad = hdr.read_sof(s, sl, "JPEG: unsupported frame header")) return fail(err, bad);
      for (int i = 0; i < hdr.ncomp; i++) {
        hmax = std::max(hmax, comp[i].h);
        vmax = std::max(vmax, comp[i].v);
      }
      if (hdr.ncomp == 1) comp[0].h = comp[0].v = hmax = vmax = 1;
      if (comp[0].h != hmax || comp[0].v != vmax) return fail(err, "JPEG: luma is subsampled; unsupported");
      *w = hdr.W;
      *h = hdr.H;
      if (!sink && (size_t)hdr.W * hdr.H > cap) return fail(err, "frame larger than the buffer");
      mx = (hdr.W + 8 * hmax - 1) / (8 * hmax);
      my = (hdr.H + 8 * vmax - 1) / (8 * vmax);
      lbw = mx * hmax;
      lbh = my * vmax;
      lcw = (hdr.W + 7) / 8;
      lch = (hdr.H + 7) / 8;
      if (sink) {  // checked BEFORE the scans' coefficient store is sized from the header (65535 x 65535 would ask for 8.6 GB)
        if (sink->pitch_blocks && sink->pitch_blocks < lbw) return fail(err, "coefficient row pitch too small for this file");
        if ((size_t)(sink->pitch_blocks ? sink->pitch_blocks : lbw) * lbh > sink->cap_blocks) return fail(err, "frame larger than the coefficient buffer");
      }
      coef.assign((size_t)lbw * lbh * 64, 0);
    } else if (is_sof(m)) {
      return fail(err, "JPEG: not a progressive Huffman file");
    } else if (m == 0xda) {
      // only component 0 is kept below: wrong for an RGB-encoded file (cv::imread weighs R, G and B) -> refused, loudly
      if (hdr.is_rgb()) return fail(err, "JPEG: progressive RGB-encoded files (Adobe transform 0 / component ids R G B) are not supported");
      if (!hdr.have_sof) return fail(err, "JPEG: scan before frame header");
      const int ns = sl ? s[0] : 0;
      if (ns < 1 || ns > hdr.ncomp || sl < 1 + 2 * (size_t)ns + 3) return fail(err, "JPEG: bad scan header");
      int sc[4];
      bool has_luma = false;
      for (int i = 0; i < ns; i++) {
        int k = -1;
        for (int c = 0; c < hdr.ncomp; c++)
          if (comp[c].id == s[1 + 2 * i]) k = c;
        if (k < 0) return fail(err, "JPEG: scan names an unknown component");
        sc[i] = k;
        comp[k].td = s[2 + 2 * i] >> 4;
        comp[k].ta = s[2 + 2 * i] & 15;
        if (comp[k].td > 3 || comp[k].ta > 3) return fail(err, "JPEG: bad table index");
        if (k == 0) has_luma = true;
      }
      const int Ss = s[1 + 2 * ns], Se = s[2 + 2 * ns], Ah = s[3 + 2 * ns] >> 4, Al = s[3 + 2 * ns] & 15;
      if (Ss > Se || Se > 63 || (Ss == 0 && Se != 0) || (Ss > 0 && ns != 1) || Al > 13) return fail(err, "JPEG: bad progression parameters");
      const unsigned char* ecs = d + seg.p;
      if (has_luma) {
        saw_luma_scan = true;
        Bits b;
        b.p = ecs;
        b.end = d + n;
        for (int c = 0; c < hdr.ncomp; c++) comp[c].pred = 0;
        int eobrun = 0, to_restart = hdr.restart;
        auto do_restart = [&]() -> bool {
          if (!b.restart()) return false;
          for (int c = 0; c < hdr.ncomp; c++) comp[c].pred = 0;
          eobrun = 0;
          to_restart = hdr.restart;
          return true;
        };
        if (Ss == 0) {  // DC scan: interleaved over the scan's components (MCU order) or luma alone
          for (int i = 0; i < ns; i++)
            if (!Ah && !hdr.dc[comp[sc[i]].td].present) return fail(err, "JPEG: scan refers to a missing table");
          const bool inter = ns > 1;
          const int bw = inter ? mx : lcw, bh = inter ? my : lch;
          for (int y = 0; y < bh; y++)
            for (int x = 0; x < bw; x++) {
              if (hdr.restart && to_restart == 0 && !do_restart()) return fail(err, "JPEG: missing restart marker");
              for (int i = 0; i < ns; i++) {
                Comp& cc = comp[sc[i]];
                const int nb = inter ? cc.h * cc.v : 1;
                for (int k = 0; k < nb; k++) {
                  int16_t* blk = nullptr;
                  if (sc[i] == 0) {
                    const int bx = inter ? x * cc.h + k % cc.h : x, by = inter ? y * cc.v + k / cc.h : y;
                    blk = &coef[((size_t)by * lbw + bx) * 64];
                  }
                  if (!Ah) {
                    const int t = decode_sym(b, hdr.dc[cc.td]);
                    if (t < 0 || t > 11) return fail(err, "JPEG: bad DC code");
                    cc.pred += t ? extend(b.get(t), t) : 0;
                    if (blk) blk[0] = (int16_t)(cc.pred * (1 << Al));
                  } else {
                    const int bit = b.get(1);
                    if (blk && bit) blk[0] = (int16_t)(blk[0] | (1 << Al));
                  }
                }
              }
              if (hdr.restart) to_restart--;
            }
        } else {  // AC scan of the luma component alone
          const Huff& act = hdr.ac[comp[0].ta];
          if (!act.present) return fail(err, "JPEG: scan refers to a missing table");
          const int p1 = 1 << Al, m1 = -(1 << Al);
          for (int y = 0; y < lch; y++)
            for (int x = 0; x < lcw; x++) {
              if (hdr.restart && to_restart == 0 && !do_restart()) return fail(err, "JPEG: missing restart marker");
              int16_t* blk = &coef[((size_t)y * lbw + x) * 64];
              if (!Ah) {  // first pass over this band
                if (eobrun > 0) eobrun--;
                else
                  for (int k = Ss; k <= Se; k++) {
                    const int rs = decode_sym(b, act);
                    if (rs < 0) return fail(err, "JPEG: bad AC code");
                    const int r = rs >> 4, sz = rs & 15;
                    if (sz) {
                      k += r;
                      if (k > Se) return fail(err, "JPEG: coefficient index out of range");
                      blk[kZigzag[k]] = (int16_t)(extend(b.get(sz), sz) * (1 << Al));
                    } else if (r == 15) {
                      k += 15;
                    } else {
                      eobrun = (1 << r) - 1;
                      if (r) eobrun += b.get(r);
                      break;
                    }
                  }
              } else {  // refinement (ITU T.81 G.1.2.3, as libjpeg's decode_mcu_AC_refine)
                int k = Ss;
                if (eobrun == 0) {
                  for (; k <= Se; k++) {
                    const int rs = decode_sym(b, act);
                    if (rs < 0) return fail(err, "JPEG: bad AC code");
                    int r = rs >> 4, sz = rs & 15;
                    if (sz) {
                      if (sz != 1) return fail(err, "JPEG: bad refinement code");
                      sz = b.get(1) ? p1 : m1;
                    } else if (r != 15) {
                      eobrun = 1 << r;
                      if (r) eobrun += b.get(r);
                      break;
                    }
                    do {
                      int16_t* cf = &blk[kZigzag[k]];
                      if (*cf != 0) {
                        if (b.get(1) && (*cf & p1) == 0) *cf = (int16_t)(*cf + (*cf >= 0 ? p1 : m1));
                      } else if (--r < 0) {
                        break;
                      }
                      k++;
                    } while (k <= Se);
                    if (sz && k <= Se) blk[kZigzag[k]] = (int16_t)sz;
                  }
                }
                if (eobrun > 0) {
                  for (; k <= Se; k++) {
                    int16_t* cf = &blk[kZigzag[k]];
                    if (*cf != 0 && b.get(1) && (*cf & p1) == 0) *cf = (int16_t)(*cf + (*cf >= 0 ? p1 : m1));
                  }
                  eobrun--;
                }
              }
              if (hdr.restart) to_restart--;
            }
        }
      }
      // on to the next marker after the entropy-coded segment (RSTn and stuffed FF00 belong to it)
      size_t q = (size_t)(ecs - d);
      while (q + 1 < n && !(d[q] == 0xff && d[q + 1] != 0 && !(d[q + 1] >= 0xd0 && d[q + 1] <= 0xd7))) q++;
      seg.p = q;
      continue;
    }
  }
  if (seg.error) return fail(err, seg.error);
  if (!hdr.have_sof || !saw_luma_scan) return fail(err, "JPEG: no scan found");
  if (!hdr.have_qt[comp[0].tq]) return fail(err, "JPEG: scan refers to a missing table");
  const uint16_t* q = hdr.qt[comp[0].tq];
  if (sink) {  // coefficient output (see JpegCoefSink): the scans' result as it is
    sink->w = hdr.W;
    sink->h = hdr.H;
    if (sink->pitch_blocks && sink->pitch_blocks < lbw) return fail(err, "coefficient row pitch too small for this file");
    sink->blocks_w = sink->pitch_blocks ? sink->pitch_blocks : lbw;
    sink->blocks_rows = lbh;
    if ((size_t)sink->blocks_w * lbh > sink->cap_blocks) return fail(err, "frame larger than the coefficient buffer");
    for (int r = 0; r < lbh; r++)
      memcpy(sink->coef + (size_t)r * sink->blocks_w * 64, coef.data() + (size_t)r * lbw * 64, (size_t)lbw * 64 * sizeof(int16_t));
    for (int i = 0; i < 64; i++) sink->quant[i] = q[i];
    return true;
  }
  // coefficients -> samples: dequantise, islow IDCT, crop
  std::vector<unsigned char> rows((size_t)lbw * 8 * 8);
  int cf[64];
  for (int by = 0; by < lch; by++) {
    for (int bx = 0; bx < lcw; bx++) {
      const int16_t* blk = &coef[((size_t)by * lbw + bx) * 64];
      bool dc_only = true;
      for (int i = 0; i < 64; i++) {
        cf[i] = blk[i] * q[i];
        if (i && blk[i]) dc_only = false;
      }
      idct_islow(cf, rows.data() + (size_t)bx * 8, (size_t)lbw * 8, dc_only);
    }
    const int y0 = by * 8, ny = std::min(8, hdr.H - y0);
    for (int r = 0; r < ny; r++) memcpy(out + (size_t)(y0 + r) * hdr.W, rows.data() + (size_t)r * lbw * 8, (size_t)hdr.W);
  }
  return true;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------
// Baseline JPEG
// ---------------------------------------------------------------------------------------------------------

bool jpeg_gray8(const unsigned char* d, size_t n, unsigned char* out, size_t cap, int* w, int* h, std::string* err, JpegCoefSink* sink) {
  Header hdr;
  Comp* const comp = hdr.comp;
  Segments seg(d, n);
  while (seg.next()) {
    const int m = seg.marker;
    const unsigned char* const s = seg.s;
    const size_t sl = seg.sl;
    if (m >= 0xd0 && m <= 0xd7) continue;  // a restart marker between segments: passed over
    if (const char* bad = hdr.read_tables(m, s, sl)) return fail(err, bad);
    if (m == 0xc0 || m == 0xc1) {  // SOF0 / SOF1: sequential, Huffman
      if (const char* bad = hdr.read_sof(s, sl, "JPEG: unsupported frame header")) return fail(err, bad);
      *w = hdr.W;
      *h = hdr.H;
    } else if (m == 0xc2) {  // progressive: its own decoder
      return jpeg_progressive_gray8(d, n, out, cap, w, h, err, sink);
    } else if (is_sof(m)) {
      return fail(err, "JPEG: lossless, hierarchical and arithmetic-coded files are not supported");
    } else if (m == 0xda) {  // SOS: the one scan of a baseline file
      const int ncomp = hdr.ncomp, W = hdr.W, H = hdr.H, restart = hdr.restart;
      if (!hdr.have_sof) return fail(err, "JPEG: scan before frame header");
      if (!sink && (size_t)W * H > cap) return fail(err, "frame larger than the buffer");
      const int ns = sl ? s[0] : 0;
      if (ns != ncomp || sl < 1 + 2 * (size_t)ns + 3) return fail(err, "JPEG: only single-scan files are supported");
      for (int i = 0; i < ns; i++) {
        int k = -1;
        for (int c = 0; c < ncomp; c++)
          if (comp[c].id == s[1 + 2 * i]) k = c;
        if (k != i) return fail(err, "JPEG: unexpected component order");
        comp[k].td = s[2 + 2 * i] >> 4;
        comp[k].ta = s[2 + 2 * i] & 15;
        if (comp[k].td > 3 || comp[k].ta > 3 || !hdr.dc[comp[k].td].present || !hdr.ac[comp[k].ta].present || !hdr.have_qt[comp[k].tq])
          return fail(err, "JPEG: scan refers to a missing table");
        comp[k].pred = 0;
      }
      // geometry: a single-component scan is non-interleaved (one block per MCU)
      const int hmax = ncomp == 1 ? 1 : std::max(comp[0].h, std::max(comp[1].h, comp[2].h));
      const int vmax = ncomp == 1 ? 1 : std::max(comp[0].v, std::max(comp[1].v, comp[2].v));
      const int yh = ncomp == 1 ? 1 : comp[0].h, yv = ncomp == 1 ? 1 : comp[0].v;
      if (ncomp == 3 && (yh != hmax || yv != vmax)) return fail(err, "JPEG: luma is subsampled; unsupported");
      // An RGB-encoded file (Adobe transform 0, or component ids R G B): gray is a weighted sum of ALL three components, not
      // component 0 -- no luma record for the device, and on the host every component is inverted (1 x 1 sampling only).
      const bool rgb = hdr.is_rgb();
      if (rgb && sink) return fail(err, "JPEG: RGB-encoded file: no luma coefficient record");
      if (rgb && (hmax != 1 || vmax != 1)) return fail(err, "JPEG: RGB-encoded file with subsampled components is not supported");
      const int mcu_w = 8 * hmax, mcu_h = 8 * vmax;
      const int mx = (W + mcu_w - 1) / mcu_w, my = (H + mcu_h - 1) / mcu_h;
      const size_t pw = (size_t)mx * mcu_w;  // padded luma row (luma has the full resolution)
      static thread_local std::vector<unsigned char> rows;
      if (!sink) rows.resize(pw * mcu_h * (rgb ? 3 : 1));  // rgb: the R, G and B block rows one after the other
      if (sink) {  // coefficient output: quantised luma coefficients, natural order, [block row][block][64]; no inverse DCT here
        sink->w = W;
        sink->h = H;
        if (sink->pitch_blocks && sink->pitch_blocks < mx * yh) return fail(err, "coefficient row pitch too small for this file");
        sink->blocks_w = sink->pitch_blocks ? sink->pitch_blocks : mx * yh;
        sink->blocks_rows = my * yv;
        if ((size_t)sink->blocks_w * sink->blocks_rows > sink->cap_blocks) return fail(err, "frame larger than the coefficient buffer");
        for (int i = 0; i < 64; i++) sink->quant[i] = hdr.qt[comp[0].tq][i];
      }
      Bits b;
      b.p = d + seg.p;
      b.end = d + n;
      int coef[64];
      int to_restart = restart;
      for (int y = 0; y < my; y++) {
        for (int x = 0; x < mx; x++) {
          if (restart && to_restart == 0) {  // RSTn: byte-align, skip the marker, reset predictions
            if (!b.restart()) return fail(err, "JPEG: missing restart marker");
            for (int c = 0; c < ncomp; c++) comp[c].pred = 0;
            to_restart = restart;
          }
          for (int c = 0; c < ncomp; c++) {
            const int nb = ncomp == 1 ? 1 : comp[c].h * comp[c].v;
            for (int k = 0; k < nb; k++) {
              const bool luma = c == 0 || rgb;  // the component is kept (rgb: all three; then sink == nullptr)
              int16_t* blk = nullptr;  // (coefficient output) this luma block
              if (luma && sink) {
                const int bx = ncomp == 1 ? 0 : k % comp[c].h, by = ncomp == 1 ? 0 : k / comp[c].h;
                blk = sink->coef + ((size_t)(y * yv + by) * sink->blocks_w + (size_t)x * yh + bx) * 64;
                memset(blk, 0, 64 * sizeof(int16_t));
              } else if (luma) {
                memset(coef, 0, sizeof coef);
              }
              const uint16_t* q = hdr.qt[comp[c].tq];
              int t = decode_sym(b, hdr.dc[comp[c].td]);
              if (t < 0 || t > 11) return fail(err, "JPEG: bad DC code");
              comp[c].pred += t ? extend(b.get(t), t) : 0;
              if (blk) blk[0] = (int16_t)comp[c].pred;
              else if (luma) coef[0] = (int16_t)comp[c].pred * q[0];  // (the coefficient is the predictor's low 16 bits, as in the record and in libjpeg's JCOEF)
              bool dc_only = true;
              const Huff& act = hdr.ac[comp[c].ta];
              for (int i = 1; i < 64;) {
                if (b.cnt < 16) b.fill();
                const int fa = act.fast_ac[b.peek(9)];
                if (fa) {  // code + magnitude in one lookup
                  i += (fa >> 4) & 15;
                  if (i > 63) return fail(err, "JPEG: coefficient index out of range");
                  b.skip(fa & 15);
                  if (blk) blk[kZigzag[i]] = (int16_t)(fa >> 8);
                  else if (luma) coef[kZigzag[i]] = (fa >> 8) * q[kZigzag[i]];
                  dc_only = false;
                  i++;
                  continue;
                }
                const int rs = decode_sym(b, act);
                if (rs < 0) return fail(err, "JPEG: bad AC code");
                const int r = rs >> 4, sz = rs & 15;
                if (sz == 0) {
                  if (r != 15) break;  // EOB
                  i += 16;
                  continue;
                }
                i += r;
                if (i > 63) return fail(err, "JPEG: coefficient index out of range");
                const int v = extend(b.get(sz), sz);
                if (blk) blk[kZigzag[i]] = (int16_t)v;
                else if (luma) coef[kZigzag[i]] = v * q[kZigzag[i]];
                dc_only = false;
                i++;
              }
              if (luma && !sink) {
                const int bx = ncomp == 1 ? 0 : k % comp[c].h, by = ncomp == 1 ? 0 : k / comp[c].h;
                idct_islow(coef, rows.data() + (rgb ? (size_t)c * pw * mcu_h : 0) + (size_t)by * 8 * pw + (size_t)x * mcu_w + (size_t)bx * 8, pw, dc_only);
              }
            }
          }
          if (restart) to_restart--;
        }
        const int y0 = y * mcu_h, ny = std::min(mcu_h, H - y0);
        if (!sink && !rgb)
          for (int r = 0; r < ny; r++) memcpy(out + (size_t)(y0 + r) * W, rows.data() + (size_t)r * pw, (size_t)W);
        if (!sink && rgb)  // libjpeg's rgb_gray_convert (jdcolor.c): (FIX(0.299) R + FIX(0.587) G + FIX(0.114) B + ONE_HALF) >> 16
          for (int r = 0; r < ny; r++) {
            const unsigned char *R = rows.data() + (size_t)r * pw, *G = R + pw * mcu_h, *B = G + pw * mcu_h;
            unsigned char* o = out + (size_t)(y0 + r) * W;
            for (int xx = 0; xx < W; xx++) o[xx] = (unsigned char)((19595 * R[xx] + 38470 * G[xx] + 7471 * B[xx] + 32768) >> 16);
          }
      }
      return true;
    }
  }
  return fail(err, seg.error ? seg.error : "JPEG: no scan found");
}

bool decode_jpeg_coefs(const unsigned char* d, size_t n, JpegCoefSink* sink, std::string* err) {
  if (!sink || !sink->coef) return fail(err, "no coefficient buffer");
  if (n < 4 || d[0] != 0xff || d[1] != 0xd8) return fail(err, "not a JPEG file");
  int w = 0, h = 0;
  return jpeg_gray8(d, n, nullptr, 0, &w, &h, err, sink);
}

}  // namespace mdc_host
