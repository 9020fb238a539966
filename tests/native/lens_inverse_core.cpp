// csrc/lens_inverse_model.h as a stand-alone program (pure host code, built under AddressSanitizer and UndefinedBehaviorSanitizer by
// build.build_lens_inverse_core_program; tests/test_lens_inverse_cpu.py compares what it writes with the NumPy restatement bit for bit).
//
//   lens_inverse_core <jobs.txt> <out.bin>
//
// jobs.txt, one job per line, floats as C hex literals (kind: 0 pinhole, 1 RadTan, 2 EquiDistant, 3 FOV with k0 = omega):
//   T kind fx fy cx cy k0 k1 k2 k3 ofx ofy ocx ocy in_w in_h out_w out_h    the inverse tables: every raw pixel, then the border rules
//     -> int32 outside, float ux[in_w * in_h], float uy[in_w * in_h]                             against the output size
//   R kind fx fy cx cy k0 k1 k2 k3 ofx ofy ocx ocy seed n                    n seeded raw points through the inverse
//     -> float x[n], float y[n]
// The points of an R job: point i has x = value(seed + 2 i), y = value(seed + 2 i + 1), value(c) = the bits fmix32(c) as a float
// for even i (every exponent, NaN, infinities, denormals) and -64 + 256 * (fmix32(c) >> 8) / 2^24 for odd i; points 0 .. 9 are NaN,
// +inf, -inf, 0, the principal point itself, three points within rd <= 1e-8 of it and two far outside every model's domain.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "lens_inverse_model.h"

static uint32_t fmix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}

static float value(uint32_t c, int64_t i) {
  const uint32_t h = fmix32(c);
  if (i % 2 == 0) return mdc::fov_float(h);
  return -64.0f + 256.0f * (float)(h >> 8) / 16777216.0f;
}

static bool put(FILE* f, const void* p, size_t bytes) { return fwrite(p, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: lens_inverse_core jobs.txt out.bin\n");
    return 2;
  }
  FILE* in = fopen(argv[1], "r");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) {
    fprintf(stderr, "lens_inverse_core: cannot open the files\n");
    return 2;
  }
  char line[1024];
  int jobs = 0;
  while (fgets(line, sizeof line, in)) {
    std::vector<char*> w;
    for (char* t = strtok(line, " \t\r\n"); t; t = strtok(0, " \t\r\n")) w.push_back(t);
    if (w.empty()) continue;
    if (w.size() < 16) {
      fprintf(stderr, "lens_inverse_core: short job line\n");
      return 2;
    }
    const int kind = atoi(w[1]);
    mdc::LensInverseModel m = mdc::LensInverseModel();
    m.fx = strtof(w[2], 0);
    m.fy = strtof(w[3], 0);
    m.cx = strtof(w[4], 0);
    m.cy = strtof(w[5], 0);
    for (int i = 0; i < 4; i++) m.k[i] = strtof(w[6 + i], 0);
    m.d2t = kind == mdc::LENSINV_FOV ? mdc::lens_inverse_d2t(m.k[0]) : 0.0f;
    m.ofx = strtof(w[10], 0);
    m.ofy = strtof(w[11], 0);
    m.ocx = strtof(w[12], 0);
    m.ocy = strtof(w[13], 0);
    bool ok = true;
    if (w[0][0] == 'T') {
      if (w.size() < 18) return 2;
      const int in_w = atoi(w[14]), in_h = atoi(w[15]), out_w = atoi(w[16]), out_h = atoi(w[17]);
      const size_t n = (size_t)in_w * in_h;
      std::vector<float> x(n), y(n);
      int32_t outside = 0;
      for (int r = 0; r < in_h; r++)
        for (int c = 0; c < in_w; c++) {
          float& px = x[(size_t)r * in_w + c];
          float& py = y[(size_t)r * in_w + c];
          px = (float)c;
          py = (float)r;
          mdc::lens_undistort_point(kind, m, px, py);
          if (mdc::lens_border_rule(px, py, out_w, out_h, (float)0.01, (float)(out_w - 1.01), (float)(out_h - 1.01))) outside = 1;
        }
      ok = put(out, &outside, 4) && put(out, x.data(), n * 4) && put(out, y.data(), n * 4);
    } else if (w[0][0] == 'R') {
      const uint32_t seed = (uint32_t)strtoul(w[14], 0, 10);
      const int64_t n = atoll(w[15]);
      std::vector<float> x((size_t)n), y((size_t)n);
      for (int64_t i = 0; i < n; i++) {
        x[(size_t)i] = value(seed + (uint32_t)(2 * i), i);
        y[(size_t)i] = value(seed + (uint32_t)(2 * i + 1), i);
      }
      const float special[10][2] = {{NAN, 1.0f}, {INFINITY, 2.0f}, {3.0f, -INFINITY}, {0.0f, 0.0f}, {m.cx, m.cy},
                                    {m.cx + m.fx * 5e-9f, m.cy}, {m.cx, m.cy - m.fy * 9e-9f}, {m.cx + m.fx * 1e-12f, m.cy + m.fy * 1e-12f},
                                    {m.cx + m.fx * 3.0f, m.cy + m.fy * 3.0f}, {m.cx - m.fx * 40.0f, m.cy + m.fy * 0.5f}};
      for (int i = 0; i < 10 && i < n; i++) {
        x[(size_t)i] = special[i][0];
        y[(size_t)i] = special[i][1];
      }
      for (int64_t i = 0; i < n; i++) mdc::lens_undistort_point(kind, m, x[(size_t)i], y[(size_t)i]);
      ok = put(out, x.data(), (size_t)n * 4) && put(out, y.data(), (size_t)n * 4);
    } else {
      fprintf(stderr, "lens_inverse_core: unknown job %s\n", w[0]);
      return 2;
    }
    if (!ok) {
      fprintf(stderr, "lens_inverse_core: write failed\n");
      return 2;
    }
    jobs++;
  }
  fclose(in);
  if (fclose(out) != 0) return 2;
  printf("lens_inverse_core: %d jobs\n", jobs);
  return 0;
}
