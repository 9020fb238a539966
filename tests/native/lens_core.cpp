// csrc/lens_point_model.h as a stand-alone program (pure host code, built under AddressSanitizer and UndefinedBehaviorSanitizer by
// build.build_lens_core_program; tests/test_lens_cpu.py compares what it writes with the NumPy restatement bit for bit).
//
//   lens_core <jobs.txt> <out.bin>
//
// jobs.txt, one job per line, floats as C hex literals:
//   P kind fx fy cx cy k0 k1 k2 k3 in_w in_h out_w out_h crop            the crop search, then the tables
//   P kind fx fy cx cy k0 k1 k2 k3 in_w in_h out_w out_h norm n0 n1 n2 n3  tables for these normalised rectified intrinsics
//     -> int32 status (LENS_CROP_*), int32 rounds, float norm[4], int32 black, float x[out_w * out_h], float y[out_w * out_h]
//        (after a status != 0 nothing more of the job is written)
//   R kind fx fy cx cy k0 k1 k2 k3 ofx ofy ocx ocy seed n                n seeded points through the model
//     -> float x[n], float y[n]
// The points of an R job: point i has x = value(seed + 2 i), y = value(seed + 2 i + 1), value(c) = the bits fmix32(c) as a float
// for even i (every exponent, NaN, infinities, denormals) and -64 + 256 * (fmix32(c) >> 8) / 2^24 for odd i; points 0 .. 7 are NaN,
// +inf, -inf, 0, the rectified centre itself and three points within r <= 1e-8 of it.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "lens_point_model.h"

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
    fprintf(stderr, "usage: lens_core jobs.txt out.bin\n");
    return 2;
  }
  FILE* in = fopen(argv[1], "r");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) {
    fprintf(stderr, "lens_core: cannot open the files\n");
    return 2;
  }
  char line[1024];
  int jobs = 0;
  while (fgets(line, sizeof line, in)) {
    std::vector<char*> w;
    for (char* t = strtok(line, " \t\r\n"); t; t = strtok(0, " \t\r\n")) w.push_back(t);
    if (w.empty()) continue;
    if (w.size() < 15) {
      fprintf(stderr, "lens_core: short job line\n");
      return 2;
    }
    const int kind = atoi(w[1]);
    mdc::LensModel m = mdc::LensModel();
    m.fx = strtof(w[2], 0);
    m.fy = strtof(w[3], 0);
    m.cx = strtof(w[4], 0);
    m.cy = strtof(w[5], 0);
    for (int i = 0; i < 4; i++) m.k[i] = strtof(w[6 + i], 0);
    bool ok = true;
    if (w[0][0] == 'P') {
      const int in_w = atoi(w[10]), in_h = atoi(w[11]), out_w = atoi(w[12]), out_h = atoi(w[13]);
      float norm[5] = {0, 0, 0, 0, 0};
      int32_t status = 0, rounds = 0;
      if (!strcmp(w[14], "crop")) {
        mdc::LensCrop c;
        status = mdc::lens_crop(kind, m, in_w, in_h, out_w, out_h, &c);
        if (status == mdc::LENS_CROP_OK) {  // normalised as the class stores them
          rounds = c.rounds;
          norm[0] = c.ofx / out_w;
          norm[1] = c.ofy / out_h;
          norm[2] = (c.ocx + 0.5) / out_w;
          norm[3] = (c.ocy + 0.5) / out_h;
        }
      } else {
        if (w.size() < 19) return 2;
        for (int i = 0; i < 4; i++) norm[i] = strtof(w[15 + i], 0);
      }
      ok = put(out, &status, 4) && put(out, &rounds, 4) && put(out, norm, 16);
      if (status == 0) {
        mdc::lens_set_rectified(m, norm, out_w, out_h);
        const size_t n = (size_t)out_w * out_h;
        std::vector<float> x(n), y(n);
        int32_t black = 0;
        for (int r = 0; r < out_h; r++)
          for (int c = 0; c < out_w; c++) {
            float& px = x[(size_t)r * out_w + c];
            float& py = y[(size_t)r * out_w + c];
            px = (float)c;
            py = (float)r;
            mdc::lens_distort_point(kind, m, px, py);
            if (mdc::lens_border_rule(px, py, in_w, in_h, (float)0.01, (float)(in_w - 1.01), (float)(in_h - 1.01))) black = 1;
          }
        ok = ok && put(out, &black, 4) && put(out, x.data(), n * 4) && put(out, y.data(), n * 4);
      }
    } else if (w[0][0] == 'R') {
      if (w.size() < 16) return 2;
      m.ofx = strtof(w[10], 0);
      m.ofy = strtof(w[11], 0);
      m.ocx = strtof(w[12], 0);
      m.ocy = strtof(w[13], 0);
      const uint32_t seed = (uint32_t)strtoul(w[14], 0, 10);
      const int64_t n = atoll(w[15]);
      std::vector<float> x((size_t)n), y((size_t)n);
      for (int64_t i = 0; i < n; i++) {
        x[(size_t)i] = value(seed + (uint32_t)(2 * i), i);
        y[(size_t)i] = value(seed + (uint32_t)(2 * i + 1), i);
      }
      const float special[8][2] = {{NAN, 1.0f}, {INFINITY, 2.0f}, {3.0f, -INFINITY}, {0.0f, 0.0f}, {m.ocx, m.ocy},
                                   {m.ocx + m.ofx * 5e-9f, m.ocy}, {m.ocx, m.ocy - m.ofy * 9e-9f}, {m.ocx + m.ofx * 1e-12f, m.ocy + m.ofy * 1e-12f}};
      for (int i = 0; i < 8 && i < n; i++) {
        x[(size_t)i] = special[i][0];
        y[(size_t)i] = special[i][1];
      }
      for (int64_t i = 0; i < n; i++) mdc::lens_distort_point(kind, m, x[(size_t)i], y[(size_t)i]);
      ok = put(out, x.data(), (size_t)n * 4) && put(out, y.data(), (size_t)n * 4);
    } else {
      fprintf(stderr, "lens_core: unknown job %s\n", w[0]);
      return 2;
    }
    if (!ok) {
      fprintf(stderr, "lens_core: write failed\n");
      return 2;
    }
    jobs++;
  }
  fclose(in);
  if (fclose(out) != 0) return 2;
  printf("lens_core: %d jobs\n", jobs);
  return 0;
}
