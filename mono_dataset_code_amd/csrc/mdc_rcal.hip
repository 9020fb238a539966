// gfx950 kernels and C entry points of the responseCalib solver (reference src/main_responseCalib.cpp:177-380): from an
// exposure sweep of n 8-bit w x h frames with exposure times t_i, the inverse response G (256 doubles, what pcalib.txt holds)
// and the scene irradiance E (w*h doubles) by alternating least squares.  The reference makes about five sequential passes
// over the n*w*h byte stack per iteration on one core; here a lane owns 4 adjacent pixels (or 1 when w*h is not a multiple of
// 4) and walks the images in order, so every per-pixel quantity keeps the reference's summation order.
//
// Numerics (this file is built with -ffp-contract=off, division correctly rounded):
//   leak padding, initial E : exact (integer work, one division)                                -> bit-identical;
//   E step                  : per pixel the images in order, same double expressions           -> bit-identical whenever G is;
//   G step, exact order     : per bin the reference's (i, k) order, kept by an index built once: a stable counting sort of the
//                             stack by byte value (RcalIndex).  Per iteration one workgroup per bin: three waves fetch list
//                             entries and E[k] and form the products E[k]*t_i in parallel, one lane adds them in list order
//                             -> GSum, G, E and pcalib.txt bit-identical.  Bounded by the longest bin chain;
//   G step, direct          : one streaming pass, per-workgroup bin sums in 128-bit fixed point (integer LDS atomics:
//                             order-free), combined over the workgroups in a fixed order -> deterministic, not bitwise;
//   rmse                    : per lane double partials over at most 4 x n terms, then double-double in a fixed tree and a
//                             fixed slab order; the count is an exact integer.
// No float atomics anywhere.
//
// The result images (plotE / plotG, :72-146) are rendered at the end of this file: a (value, index) min/max reduction
// (minmax_first.h) and one lane per pixel that evaluates the reference's expression in its order.
#include "mdc_ctx.h"
#include "minmax_first.h"

namespace mdc {
namespace {

constexpr int kRcalThreads = 256;
constexpr int kRcalUnroll = 8;          // images whose loads a lane has in flight
constexpr int kRcalChunk = 65536;       // samples per counting-sort chunk (one wave each)
constexpr int kRcalWalkChunk = 1536;    // products per LDS buffer of the exact-order walk (192 producer lanes x 8)
constexpr int kRcalLeakImages = 64;     // images per ping-pong chunk of the leak padding

enum RcalMode { kInit = 0, kRmse = 1, kEStep = 2, kResc = 3, kGDirect = 4 };

struct RcalPartial {  // one workgroup's rmse partial: e = h + l (double-double), exact term count
  double h, l;
  unsigned long long c;
};
struct RcalBinPartial {  // one workgroup's bin sum: 128-bit fixed point (two's complement), count, non-finite seen
  unsigned long long lo, hi;
  unsigned cnt, nonfinite;
};

__device__ __forceinline__ void dd_add(double& ah, double& al, double bh, double bl) {
  const double s = ah + bh;
  const double bb = s - ah;
  double e = (ah - (s - bb)) + (bh - bb);
  e += al + bl;
  const double h = s + e;
  al = e - (h - s);
  ah = h;
}

// fixed-order tree over the workgroup: thread 0 ends with the sum
__device__ __forceinline__ void block_dd(double& h, double& l, unsigned long long& c) {
  __shared__ double s_h[kRcalThreads], s_l[kRcalThreads];
  __shared__ unsigned long long s_c[kRcalThreads];
  s_h[threadIdx.x] = h;
  s_l[threadIdx.x] = l;
  s_c[threadIdx.x] = c;
  __syncthreads();
  for (int k = kRcalThreads / 2; k > 0; k >>= 1) {
    if ((int)threadIdx.x < k) {
      double a = s_h[threadIdx.x], b = s_l[threadIdx.x];
      dd_add(a, b, s_h[threadIdx.x + k], s_l[threadIdx.x + k]);
      s_h[threadIdx.x] = a;
      s_l[threadIdx.x] = b;
      s_c[threadIdx.x] += s_c[threadIdx.x + k];
    }
    __syncthreads();
  }
  h = s_h[0];
  l = s_l[0];
  c = s_c[0];
  __syncthreads();
}

// rmse term (:58-65): skips 255 (by the caller) and a non-finite residual
__device__ __forceinline__ void rmse_term(double g, double t, double e, double& acc, unsigned& cnt) {
  const double r = g - t * e;
  if (isfinite(r)) {
    acc += r * r * 1e-10;
    cnt++;
  }
}

// One pass over the stack, pixel-major: lane = P adjacent pixels, images walked in order, kRcalUnroll loads in flight.
//   kInit   : E = (sum of the bytes, 255 included) / n                                        (:250-258)
//   kRmse   : rmse terms of (G, E)                                                             (:50-69)
//   kEStep  : ENum += t*t, ESum += G[b]*t over b != 255, E = max(ESum/ENum, 0)  + rmse of (G, E_old)  (:319-339)
//   kResc   : E' = E*f, G' = G*f on i < min(256, w*h), f = 255/G[255]; rmse of (G, E) and of (G', E')  (:349-356)
//   kGDirect: GSum[b] += E[k]*t_i, GNum[b]++ over b != 255, in 128-bit fixed point scaled by 2^scale  (:285-304)
template <int MODE, int P>
__global__ __launch_bounds__(kRcalThreads) void rcal_pass_kernel(const uint8_t* __restrict__ images, const double* __restrict__ texp, int n,
                                                                 unsigned wh, const double* __restrict__ G, double* __restrict__ E,
                                                                 RcalPartial* __restrict__ slab, RcalBinPartial* __restrict__ bins,
                                                                 const int* __restrict__ scale) {
  __shared__ double s_g[2][256];
  __shared__ unsigned long long s_lo[256], s_hi[256];
  __shared__ unsigned s_cnt[256], s_nf[256];
  const unsigned k0 = (blockIdx.x * kRcalThreads + threadIdx.x) * P;
  const bool live = k0 < wh;  // (wh is a multiple of P)
  double f = 0.0;
  if (MODE == kRmse || MODE == kEStep || MODE == kResc) {
    if (MODE == kResc) f = 255.0 / G[255];
    const unsigned lim = wh < 256u ? wh : 256u;
    for (int i = threadIdx.x; i < 256; i += kRcalThreads) {
      s_g[0][i] = G[i];
      if (MODE == kResc) s_g[1][i] = (unsigned)i < lim ? G[i] * f : G[i];
    }
  }
  if (MODE == kGDirect)
    for (int i = threadIdx.x; i < 256; i += kRcalThreads) {
      s_lo[i] = s_hi[i] = 0;
      s_cnt[i] = s_nf[i] = 0;
    }
  __syncthreads();
  int sc = 0;
  if (MODE == kGDirect) sc = *scale;
  double e0[P], e1[P], esum[P], enm[P];
  unsigned isum[P];
#pragma unroll
  for (int j = 0; j < P; j++) {
    e0[j] = e1[j] = esum[j] = enm[j] = 0.0;
    isum[j] = 0;
    if (MODE != kInit && live) {
      e0[j] = E[k0 + j];
      if (MODE == kResc) e1[j] = e0[j] * f;
    }
  }
  double acc0 = 0.0, acc1 = 0.0;
  unsigned cnt0 = 0, cnt1 = 0;
  if (live) {
    for (int i0 = 0; i0 < n; i0 += kRcalUnroll) {
      unsigned raw[kRcalUnroll];
#pragma unroll
      for (int u = 0; u < kRcalUnroll; u++) {
        raw[u] = 0;
        if (i0 + u < n) {
          const uint8_t* p = images + (size_t)(i0 + u) * wh + k0;
          raw[u] = P == 4 ? __builtin_nontemporal_load(reinterpret_cast<const unsigned*>(p)) : (unsigned)*p;
        }
      }
#pragma unroll
      for (int u = 0; u < kRcalUnroll; u++) {
        if (i0 + u >= n) break;  // wave-uniform
        const double t = texp[i0 + u];
        const double tt = t * t;
#pragma unroll
        for (int j = 0; j < P; j++) {
          const unsigned b = (raw[u] >> (8 * j)) & 255u;
          if (MODE == kInit) {
            isum[j] += b;
            continue;
          }
          if (b == 255u) continue;
          if (MODE == kRmse) rmse_term(s_g[0][b], t, e0[j], acc0, cnt0);
          if (MODE == kEStep) {
            enm[j] += tt;
            esum[j] += s_g[0][b] * t;
            rmse_term(s_g[0][b], t, e0[j], acc0, cnt0);
          }
          if (MODE == kResc) {
            rmse_term(s_g[0][b], t, e0[j], acc0, cnt0);
            rmse_term(s_g[1][b], t, e1[j], acc1, cnt1);
          }
          if (MODE == kGDirect) {
            atomicAdd(&s_cnt[b], 1u);
            const double x = e0[j] * t;
            if (!isfinite(x)) {
              s_nf[b] = 1;
            } else if (x != 0.0) {
              const double v = ldexp(fabs(x), sc);  // < 2^125 by the choice of sc (rcal_scale_kernel)
              const double hd = floor(v * 0x1p-64);
              unsigned long long hi = (unsigned long long)hd;
              unsigned long long lo = (unsigned long long)(v - hd * 0x1p64);
              if (x < 0) {
                lo = ~lo + 1;
                hi = ~hi + (lo == 0 ? 1 : 0);
              }
              const unsigned long long old = atomicAdd(&s_lo[b], lo);
              atomicAdd(&s_hi[b], hi + (old + lo < old ? 1ull : 0ull));
            }
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < P; j++) {
      if (MODE == kInit) E[k0 + j] = (double)isum[j] / (double)n;
      if (MODE == kEStep) {
        double e = esum[j] / enm[j];
        if (e < 0) e = 0;
        E[k0 + j] = e;
      }
      if (MODE == kResc) E[k0 + j] = e1[j];
    }
  }
  if (MODE == kRmse || MODE == kEStep || MODE == kResc) {
    double h = acc0, l = 0.0;
    unsigned long long c = cnt0;
    block_dd(h, l, c);
    if (threadIdx.x == 0) slab[(size_t)blockIdx.x * 2] = RcalPartial{h, l, c};
    if (MODE == kResc) {
      h = acc1;
      l = 0.0;
      c = cnt1;
      block_dd(h, l, c);
      if (threadIdx.x == 0) slab[(size_t)blockIdx.x * 2 + 1] = RcalPartial{h, l, c};
    }
  }
  if (MODE == kGDirect) {
    __syncthreads();
    for (int i = threadIdx.x; i < 256; i += kRcalThreads)
      bins[(size_t)blockIdx.x * 256 + i] = RcalBinPartial{s_lo[i], s_hi[i], s_cnt[i], s_nf[i]};
  }
}

// slab entries `which` of nblk workgroups (stride 2) -> out = {1e5 * sqrt(e / num), num}  (:68)
__global__ __launch_bounds__(kRcalThreads) void rcal_rmse_final_kernel(const RcalPartial* __restrict__ slab, int nblk, int which,
                                                                       double* __restrict__ out) {
  double h = 0.0, l = 0.0;
  unsigned long long c = 0;
  for (int b = threadIdx.x; b < nblk; b += kRcalThreads) {
    const RcalPartial p = slab[(size_t)b * 2 + which];
    dd_add(h, l, p.h, p.l);
    c += p.c;
  }
  block_dd(h, l, c);
  if (threadIdx.x == 0) {
    const double num = (double)c;
    out[0] = 1e5 * sqrt((h + l) / num);
    out[1] = num;
  }
}

// the largest finite |E| and |t| -> the fixed-point scale: every product E[k]*t_i times 2^scale, summed over all n*w*h samples,
// stays below 2^125 (max-reductions are order-free)
__global__ __launch_bounds__(kRcalThreads) void rcal_scale_kernel(const double* __restrict__ E, unsigned wh, const double* __restrict__ texp,
                                                                  int n, int* __restrict__ scale) {
  __shared__ double s_m[2][kRcalThreads];
  double me = 0.0, mt = 0.0;
  for (unsigned k = threadIdx.x; k < wh; k += kRcalThreads) {
    const double a = fabs(E[k]);
    if (isfinite(a) && a > me) me = a;
  }
  for (int i = threadIdx.x; i < n; i += kRcalThreads) {
    const double a = fabs(texp[i]);
    if (isfinite(a) && a > mt) mt = a;
  }
  s_m[0][threadIdx.x] = me;
  s_m[1][threadIdx.x] = mt;
  __syncthreads();
  for (int k = kRcalThreads / 2; k > 0; k >>= 1) {
    if ((int)threadIdx.x < k) {
      s_m[0][threadIdx.x] = fmax(s_m[0][threadIdx.x], s_m[0][threadIdx.x + k]);
      s_m[1][threadIdx.x] = fmax(s_m[1][threadIdx.x], s_m[1][threadIdx.x + k]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double m = s_m[0][0] * s_m[1][0];
    int s = 0;
    if (m > 0 && isfinite(m)) {
      int em = 0;
      (void)frexp(m, &em);  // m < 2^em
      const unsigned long long N = (unsigned long long)n * wh;
      const int en = 64 - __clzll((long long)N);  // N < 2^en
      s = 125 - em - en;
    }
    *scale = s;
  }
}

// per bin: the workgroups' fixed-point sums in order -> GSum (double), GNum
__global__ __launch_bounds__(256) void rcal_bins_final_kernel(const RcalBinPartial* __restrict__ bins, int nblk, const int* __restrict__ scale,
                                                              double* __restrict__ gsum, unsigned long long* __restrict__ gnum) {
  const int b = threadIdx.x;
  unsigned long long lo = 0, hi = 0, cnt = 0;
  unsigned nf = 0;
  for (int k = 0; k < nblk; k++) {
    const RcalBinPartial p = bins[(size_t)k * 256 + b];
    const unsigned long long o = lo;
    lo += p.lo;
    hi += p.hi + (lo < o ? 1ull : 0ull);
    cnt += p.cnt;
    nf |= p.nonfinite;
  }
  const bool neg = (long long)hi < 0;
  if (neg) {
    lo = ~lo + 1;
    hi = ~hi + (lo == 0 ? 1 : 0);
  }
  double v = ldexp((double)hi * 0x1p64 + (double)lo, -*scale);
  if (neg) v = -v;
  gsum[b] = nf ? __builtin_nan("") : v;
  gnum[b] = b == 255 ? 0 : cnt;
}

// :298-304 (G = GSum / GNum, non-finite entries from 2 on extrapolated, sequentially) and the rescale factor 255 / G[255] (:350)
__global__ __launch_bounds__(256) void rcal_g_finalize_kernel(const double* __restrict__ gsum, const unsigned long long* __restrict__ gnum,
                                                              double* __restrict__ G, double* __restrict__ factor) {
  __shared__ double s_g[256];
  s_g[threadIdx.x] = gsum[threadIdx.x] / (double)gnum[threadIdx.x];
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 2; i < 256; i++)
      if (!isfinite(s_g[i])) s_g[i] = s_g[i - 1] + (s_g[i - 1] - s_g[i - 2]);
    if (factor) *factor = 255.0 / s_g[255];
  }
  __syncthreads();
  G[threadIdx.x] = s_g[threadIdx.x];
}

// :352-356, the G half: only indices below min(256, w*h) are scaled (the loop bound is w*h)
__global__ __launch_bounds__(256) void rcal_rescale_g_kernel(double* __restrict__ G, unsigned wh) {
  __shared__ double s_f;
  if (threadIdx.x == 0) s_f = 255.0 / G[255];
  __syncthreads();
  if (threadIdx.x < wh) G[threadIdx.x] *= s_f;
}

// one leak-padding pass (:211-233): a pixel becomes 255 if it is 255 or an interior 255 (1 <= x <= w-2, 1 <= y <= h-2) is among
// its 3 x 3 neighbours -- the scatter of the reference as a gather, so passes need only a ping-pong copy
__global__ __launch_bounds__(256) void rcal_leak_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, long long total, int w,
                                                        int h) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const long long wh = (long long)w * h;
  const long long img = idx / wh;
  const int p = (int)(idx - img * wh);
  const int y = p / w, x = p - y * w;
  const uint8_t* s = src + img * wh;
  uint8_t v = s[p];
  if (v != 255) {
    for (int dy = -1; dy <= 1 && v != 255; dy++)
      for (int dx = -1; dx <= 1; dx++) {
        const int xx = x + dx, yy = y + dy;
        if (xx >= 1 && xx <= w - 2 && yy >= 1 && yy <= h - 2 && s[yy * w + xx] == 255) {
          v = 255;
          break;
        }
      }
  }
  dst[idx] = v;
}

// ---- the exact-order index: a stable counting sort of the stack by byte value ------------------------------------
// chunk c = samples [c*kRcalChunk, (c+1)*kRcalChunk) of the i-major flattened stack; hist[c][b] = its samples of value b
__global__ __launch_bounds__(256) void rcal_hist_kernel(const uint8_t* __restrict__ images, unsigned long long N,
                                                        unsigned long long* __restrict__ hist) {
  __shared__ unsigned s_h[256];
  s_h[threadIdx.x] = 0;
  __syncthreads();
  const unsigned long long c0 = (unsigned long long)blockIdx.x * kRcalChunk;
  const unsigned long long c1 = c0 + kRcalChunk < N ? c0 + kRcalChunk : N;
  for (unsigned long long q = c0 + threadIdx.x; q < c1; q += 256) atomicAdd(&s_h[images[q]], 1u);  // integer counts: order-free
  __syncthreads();
  hist[(size_t)blockIdx.x * 256 + threadIdx.x] = s_h[threadIdx.x];
}

// one workgroup per bin: exclusive scan of hist[.][b] over the chunks (in place), the bin's total into tot[b]
__global__ __launch_bounds__(1024) void rcal_hist_scan_kernel(unsigned long long* __restrict__ hist, int nchunks,
                                                              unsigned long long* __restrict__ tot) {
  __shared__ unsigned long long s_sum[1024];
  __shared__ unsigned long long s_carry;
  const int b = blockIdx.x;
  if (threadIdx.x == 0) s_carry = 0;
  __syncthreads();
  for (int c0 = 0; c0 < nchunks; c0 += 1024) {
    const int c = c0 + threadIdx.x;
    const unsigned long long m = c < nchunks ? hist[(size_t)c * 256 + b] : 0;
    s_sum[threadIdx.x] = m;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
      const unsigned long long v = (int)threadIdx.x >= d ? s_sum[threadIdx.x - d] : 0;
      __syncthreads();
      s_sum[threadIdx.x] += v;
      __syncthreads();
    }
    if (c < nchunks) hist[(size_t)c * 256 + b] = s_carry + s_sum[threadIdx.x] - m;
    __syncthreads();
    if (threadIdx.x == 1023) s_carry += s_sum[1023];
    __syncthreads();
  }
  if (threadIdx.x == 0) tot[b] = s_carry;
}

// bins 0..254 back to back (255 is never listed, :292): start[b] = sum of the totals before it; start[255] = list length
__global__ __launch_bounds__(256) void rcal_bin_start_kernel(const unsigned long long* __restrict__ tot, unsigned long long* __restrict__ start,
                                                             unsigned long long* __restrict__ counts) {
  if (threadIdx.x == 0) {
    unsigned long long s = 0;
    for (int b = 0; b < 256; b++) {
      start[b] = s;
      if (b < 255) s += tot[b];
    }
    start[256] = s;
  }
  counts[threadIdx.x] = threadIdx.x == 255 ? 0 : tot[threadIdx.x];
}

// one wave per chunk, 64 samples at a time in order: a sample's slot = its bin's start + the chunk's offset in that bin + the
// samples of the same value before it in the chunk (lanes with equal bytes found by 8 ballots) -> stable
template <typename IdxT>
__global__ __launch_bounds__(64) void rcal_scatter_kernel(const uint8_t* __restrict__ images, unsigned long long N,
                                                          const unsigned long long* __restrict__ hist, const unsigned long long* __restrict__ start,
                                                          IdxT* __restrict__ list) {
  __shared__ unsigned long long s_cur[256];
  const int lane = threadIdx.x;
  for (int b = lane; b < 256; b += 64) s_cur[b] = start[b] + hist[(size_t)blockIdx.x * 256 + b];
  __syncthreads();
  const unsigned long long c0 = (unsigned long long)blockIdx.x * kRcalChunk;
  const unsigned long long c1 = c0 + kRcalChunk < N ? c0 + kRcalChunk : N;
  const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
  for (unsigned long long q0 = c0; q0 < c1; q0 += 64) {
    const unsigned long long q = q0 + lane;
    const bool in = q < c1;
    const unsigned b = in ? images[q] : 256u;
    unsigned long long same = __ballot(in);
#pragma unroll
    for (int bit = 0; bit < 8; bit++) {
      const unsigned long long m = __ballot(in && ((b >> bit) & 1));
      same &= ((b >> bit) & 1) ? m : ~m;
    }
    unsigned long long slot = 0;
    if (in) slot = s_cur[b] + __popcll(same & below);
    __builtin_amdgcn_wave_barrier();
    if (in && b != 255u && (same & below) == 0) s_cur[b] += __popcll(same);  // the group's first lane moves the cursor
    __builtin_amdgcn_wave_barrier();
    if (in && b != 255u) list[slot] = (IdxT)q;
  }
}

// the G sums in the reference's order: workgroup = bin; waves 1..3 fetch positions and E[k] and form E[k]*t_i into one LDS
// buffer while lane 0 of wave 0 adds the previous buffer front to back -- one sequential double chain per bin
template <typename IdxT>
__global__ __launch_bounds__(256) void rcal_g_walk_kernel(const IdxT* __restrict__ list, const unsigned long long* __restrict__ start,
                                                          const double* __restrict__ E, const double* __restrict__ texp, unsigned wh,
                                                          double* __restrict__ gsum) {
  constexpr int kPer = kRcalWalkChunk / 192;
  __shared__ double s_buf[2][kRcalWalkChunk];
  const int b = blockIdx.x;
  const unsigned long long beg = start[b], len = start[b + 1] - beg;
  const unsigned long long nch = (len + kRcalWalkChunk - 1) / kRcalWalkChunk;
  const int wave = threadIdx.x >> 6;
  double s = 0.0;  // GSum[b] starts at +0 (:287)
  for (unsigned long long c = 0; c <= nch; c++) {
    if (wave != 0 && c < nch) {
      const int p = threadIdx.x - 64;
      IdxT pos[kPer];
#pragma unroll
      for (int u = 0; u < kPer; u++) {
        const unsigned long long j = c * kRcalWalkChunk + u * 192 + p;
        pos[u] = j < len ? list[beg + j] : (IdxT)0;
      }
      double ev[kPer], tv[kPer];
#pragma unroll
      for (int u = 0; u < kPer; u++) {
        const unsigned long long i = (unsigned long long)pos[u] / wh;
        const unsigned long long k = (unsigned long long)pos[u] - i * wh;
        ev[u] = E[k];
        tv[u] = texp[i];
      }
#pragma unroll
      for (int u = 0; u < kPer; u++) s_buf[c & 1][u * 192 + p] = ev[u] * tv[u];  // :295, E[k] * exposureVec[i]
    }
    if (threadIdx.x == 0 && c > 0) {
      const double* q = s_buf[(c - 1) & 1];
      const unsigned long long rest = len - (c - 1) * kRcalWalkChunk;
      const int m = rest < (unsigned long long)kRcalWalkChunk ? (int)rest : kRcalWalkChunk;
      for (int j = 0; j < m; j++) s += q[j];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) gsum[b] = s;
}

inline unsigned blocks_of(long long n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

// ---- launchers -------------------------------------------------------------------------------------------------------

struct RcalIndex {
  int n = 0, w = 0, h = 0;
  bool wide = false;                        // 8-byte positions (n*w*h >= 2^32)
  void* d_list = nullptr;                   // positions i*w*h + k of the samples of bins 0..254, bin after bin, each in (i, k) order
  unsigned long long* d_start = nullptr;    // 257: first entry of each bin; [255] = [256] = list length
  unsigned long long* d_counts = nullptr;   // 256: GNum (:291), [255] = 0
  unsigned long long entries = 0, longest = 0;
};

void rcal_index_free(RcalIndex* ix) {
  if (!ix) return;
  (void)hipFree(ix->d_list);
  (void)hipFree(ix->d_start);
  (void)hipFree(ix->d_counts);
  delete ix;
}

// Pass geometry: 4 pixels per lane when the frame size and the base allow dword loads, else 1.
static int pass_width(const uint8_t* d_images, unsigned wh) { return (wh % 4 == 0 && ((uintptr_t)d_images & 3) == 0) ? 4 : 1; }
static unsigned pass_blocks(unsigned wh, int P) { return blocks_of(wh / P, kRcalThreads); }

template <int MODE>
static hipError_t launch_pass(const uint8_t* d_images, const double* d_t, int n, unsigned wh, const double* d_G, double* d_E,
                              RcalPartial* slab, RcalBinPartial* bins, const int* scale, hipStream_t s) {
  const int P = pass_width(d_images, wh);
  const unsigned nb = pass_blocks(wh, P);
  if (P == 4)
    rcal_pass_kernel<MODE, 4><<<nb, kRcalThreads, 0, s>>>(d_images, d_t, n, wh, d_G, d_E, slab, bins, scale);
  else
    rcal_pass_kernel<MODE, 1><<<nb, kRcalThreads, 0, s>>>(d_images, d_t, n, wh, d_G, d_E, slab, bins, scale);
  return hipGetLastError();
}

// Scratch of the passes for a w*h frame: the rmse slab (2 entries per workgroup), the bin slab of the direct G step (256 per
// workgroup), GSum / GNum, the fixed-point scale.
struct RcalWork {
  RcalPartial* slab = nullptr;
  RcalBinPartial* bins = nullptr;
  double* gsum = nullptr;
  unsigned long long* gnum = nullptr;
  int* scale = nullptr;
  unsigned nblk = 0;
  hipError_t alloc(unsigned wh, bool direct) {
    nblk = pass_blocks(wh, 1);  // the most any pass width needs
    hipError_t e;
    if ((e = hipMalloc(&slab, (size_t)nblk * 2 * sizeof(RcalPartial))) != hipSuccess) return e;
    if (direct && (e = hipMalloc(&bins, (size_t)nblk * 256 * sizeof(RcalBinPartial))) != hipSuccess) return e;
    if ((e = hipMalloc(&gsum, 256 * sizeof(double))) != hipSuccess) return e;
    if ((e = hipMalloc(&gnum, 256 * sizeof(unsigned long long))) != hipSuccess) return e;
    return hipMalloc(&scale, sizeof(int));
  }
  ~RcalWork() {
    for (void* p : {(void*)slab, (void*)bins, (void*)gsum, (void*)gnum, (void*)scale}) (void)hipFree(p);
  }
};

static hipError_t rmse_final(const RcalWork& w, const uint8_t* d_images, unsigned wh, int which, double* d_out, hipStream_t s) {
  if (!d_out) return hipSuccess;
  rcal_rmse_final_kernel<<<1, kRcalThreads, 0, s>>>(w.slab, (int)pass_blocks(wh, pass_width(d_images, wh)), which, d_out);
  return hipGetLastError();
}

hipError_t rcal_leak_pad(uint8_t* d_images, int n, int w, int h, int leak, hipStream_t s) {
  if (leak <= 0 || n <= 0) return hipSuccess;
  const long long wh = (long long)w * h;
  const int per = std::min(n, kRcalLeakImages);
  uint8_t* tmp = nullptr;
  hipError_t e = hipMalloc(&tmp, (size_t)per * wh);
  if (e != hipSuccess) return e;
  for (int i0 = 0; i0 < n && e == hipSuccess; i0 += per) {
    const int cnt = std::min(per, n - i0);
    uint8_t* a = d_images + (size_t)i0 * wh;
    const long long total = (long long)cnt * wh;
    for (int it = 0; it < leak; it++) {
      rcal_leak_kernel<<<blocks_of(total, 256), 256, 0, s>>>(it & 1 ? tmp : a, it & 1 ? a : tmp, total, w, h);
    }
    if (leak & 1) e = hipMemcpyAsync(a, tmp, (size_t)total, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipGetLastError();
  }
  const hipError_t e2 = hipStreamSynchronize(s);  // the scratch is freed below
  (void)hipFree(tmp);
  return e != hipSuccess ? e : e2;
}

// Builds the stable counting sort: counts and offsets, one synchronisation for the list size (checked against free memory),
// then the scatter.  Set-up work, once per solve.
hipError_t rcal_index_build(const uint8_t* d_images, int n, int w, int h, hipStream_t s, RcalIndex** out, std::string* why) {
  *out = nullptr;
  RcalIndex* ix = new RcalIndex;
  ix->n = n;
  ix->w = w;
  ix->h = h;
  const unsigned long long N = (unsigned long long)n * w * h;
  ix->wide = N >= (1ull << 32);
  const unsigned long long nch = (N + kRcalChunk - 1) / kRcalChunk;
  unsigned long long *d_hist = nullptr, *d_tot = nullptr;
  hipError_t e;
  auto bail = [&](hipError_t err) {
    (void)hipStreamSynchronize(s);
    (void)hipFree(d_hist);
    (void)hipFree(d_tot);
    rcal_index_free(ix);
    return err;
  };
  if (nch >= (1ull << 31)) return bail(hipErrorInvalidValue);
  if ((e = hipMalloc(&ix->d_start, 257 * sizeof(unsigned long long))) != hipSuccess) return bail(e);
  if ((e = hipMalloc(&ix->d_counts, 256 * sizeof(unsigned long long))) != hipSuccess) return bail(e);
  if ((e = hipMalloc(&d_tot, 256 * sizeof(unsigned long long))) != hipSuccess) return bail(e);
  if ((e = hipMalloc(&d_hist, (size_t)std::max<unsigned long long>(nch, 1) * 256 * sizeof(unsigned long long))) != hipSuccess) return bail(e);
  if ((e = hipMemsetAsync(d_tot, 0, 256 * sizeof(unsigned long long), s)) != hipSuccess) return bail(e);
  if (nch) {
    rcal_hist_kernel<<<(unsigned)nch, 256, 0, s>>>(d_images, N, d_hist);
    rcal_hist_scan_kernel<<<256, 1024, 0, s>>>(d_hist, (int)nch, d_tot);
  }
  rcal_bin_start_kernel<<<1, 256, 0, s>>>(d_tot, ix->d_start, ix->d_counts);
  if ((e = hipGetLastError()) != hipSuccess) return bail(e);
  unsigned long long tot[256];
  if ((e = hipMemcpyAsync(tot, d_tot, sizeof tot, hipMemcpyDeviceToHost, s)) != hipSuccess) return bail(e);
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return bail(e);
  for (int b = 0; b < 255; b++) {
    ix->entries += tot[b];
    ix->longest = std::max(ix->longest, tot[b]);
  }
  const size_t bytes = (size_t)std::max<unsigned long long>(ix->entries, 1) * (ix->wide ? 8 : 4);
  size_t free_b = 0, total_b = 0;
  if ((e = hipMemGetInfo(&free_b, &total_b)) != hipSuccess) return bail(e);
  if (bytes + (64ull << 20) > free_b) {
    if (why) {
      char buf[256];
      snprintf(buf, sizeof buf, "the exact-order index needs %.2f GB of device memory for %llu samples, %.2f GB are free "
               "(use the direct G step, or fewer frames)", bytes / 1e9, ix->entries, free_b / 1e9);
      *why = buf;
    }
    return bail(hipErrorOutOfMemory);
  }
  if ((e = hipMalloc(&ix->d_list, bytes)) != hipSuccess) return bail(e);
  if (nch) {
    if (ix->wide)
      rcal_scatter_kernel<unsigned long long><<<(unsigned)nch, 64, 0, s>>>(d_images, N, d_hist, ix->d_start, (unsigned long long*)ix->d_list);
    else
      rcal_scatter_kernel<unsigned><<<(unsigned)nch, 64, 0, s>>>(d_images, N, d_hist, ix->d_start, (unsigned*)ix->d_list);
  }
  if ((e = hipGetLastError()) != hipSuccess) return bail(e);
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return bail(e);  // d_hist is freed below
  (void)hipFree(d_hist);
  (void)hipFree(d_tot);
  *out = ix;
  return hipSuccess;
}

static hipError_t g_step_indexed(const RcalIndex* ix, const double* d_t, const double* d_E, double* d_G, const RcalWork& w, double* d_factor,
                                 hipStream_t s) {
  const unsigned wh = (unsigned)ix->w * ix->h;
  hipError_t e = hipMemsetAsync(w.gsum, 0, 256 * sizeof(double), s);  // bin 255: 0 / 0
  if (e != hipSuccess) return e;
  if (ix->wide)
    rcal_g_walk_kernel<unsigned long long><<<255, 256, 0, s>>>((const unsigned long long*)ix->d_list, ix->d_start, d_E, d_t, wh, w.gsum);
  else
    rcal_g_walk_kernel<unsigned><<<255, 256, 0, s>>>((const unsigned*)ix->d_list, ix->d_start, d_E, d_t, wh, w.gsum);
  rcal_g_finalize_kernel<<<1, 256, 0, s>>>(w.gsum, ix->d_counts, d_G, d_factor);
  return hipGetLastError();
}

static hipError_t g_step_direct(const uint8_t* d_images, const double* d_t, int n, unsigned wh, const double* d_E, double* d_G,
                                const RcalWork& w, double* d_factor, hipStream_t s) {
  rcal_scale_kernel<<<1, kRcalThreads, 0, s>>>(d_E, wh, d_t, n, w.scale);
  hipError_t e = launch_pass<kGDirect>(d_images, d_t, n, wh, nullptr, const_cast<double*>(d_E), nullptr, w.bins, w.scale, s);
  if (e != hipSuccess) return e;
  rcal_bins_final_kernel<<<1, 256, 0, s>>>(w.bins, (int)pass_blocks(wh, pass_width(d_images, wh)), w.scale, w.gsum, w.gnum);
  rcal_g_finalize_kernel<<<1, 256, 0, s>>>(w.gsum, w.gnum, d_G, d_factor);
  return hipGetLastError();
}

// E step (+ rmse of the new G with the old E, d_rmse_g may be NULL)
static hipError_t e_step(const uint8_t* d_images, const double* d_t, int n, unsigned wh, const double* d_G, double* d_E, const RcalWork& w,
                         double* d_rmse_g, hipStream_t s) {
  hipError_t e = launch_pass<kEStep>(d_images, d_t, n, wh, d_G, d_E, w.slab, nullptr, nullptr, s);
  if (e != hipSuccess) return e;
  return rmse_final(w, d_images, wh, 0, d_rmse_g, s);
}

// rescale of E and G (+ rmse before and after it: d_rmse_e, d_rmse_resc may be NULL)
static hipError_t rescale(const uint8_t* d_images, const double* d_t, int n, unsigned wh, double* d_G, double* d_E, const RcalWork& w,
                          double* d_rmse_e, double* d_rmse_resc, hipStream_t s) {
  hipError_t e = launch_pass<kResc>(d_images, d_t, n, wh, d_G, d_E, w.slab, nullptr, nullptr, s);
  if (e != hipSuccess) return e;
  if ((e = rmse_final(w, d_images, wh, 0, d_rmse_e, s)) != hipSuccess) return e;
  if ((e = rmse_final(w, d_images, wh, 1, d_rmse_resc, s)) != hipSuccess) return e;
  rcal_rescale_g_kernel<<<1, 256, 0, s>>>(d_G, wh);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------- plotE / plotG (:72-146)

constexpr int kPlotBlocks = 256;  // one pass of the range kernel's grid covers kPlotBlocks * kRcalThreads = 65536 pixels

// part[b] = workgroup b's range of le = log(E + 20), part[gridDim.x + b] = its range of E
__global__ __launch_bounds__(kRcalThreads) void rcal_plot_e_range_kernel(const double* __restrict__ E, long long n, MinMaxFirst<double>* __restrict__ part) {
  __shared__ MinMaxFirst<double> s_m[kRcalThreads];
  MinMaxFirst<double> le = mm_start<double>(), e = mm_start<double>();
  for (long long i = (long long)blockIdx.x * kRcalThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kRcalThreads) {
    const double v = E[i];
    mm_take(le, log(v + 20.0), i);
    mm_take(e, v, i);
  }
  le = mm_block<double, kRcalThreads>(le, s_m);
  e = mm_block<double, kRcalThreads>(e, s_m);
  if (threadIdx.x == 0) {
    part[blockIdx.x] = le;
    part[gridDim.x + blockIdx.x] = e;
  }
}

// workgroup q: range[2q], range[2q + 1] = the minimum and maximum over part[q * nparts .. (q + 1) * nparts)
__global__ __launch_bounds__(kRcalThreads) void rcal_plot_range_final_kernel(const MinMaxFirst<double>* __restrict__ part, int nparts, double* __restrict__ range) {
  __shared__ MinMaxFirst<double> s_m[kRcalThreads];
  MinMaxFirst<double> m = mm_start<double>();
  for (int i = threadIdx.x; i < nparts; i += kRcalThreads) {
    const MinMaxFirst<double> o = part[(long long)blockIdx.x * nparts + i];
    mm_take_lo(m, o.lo, o.ilo);
    mm_take_hi(m, o.hi, o.ihi);
  }
  m = mm_block<double, kRcalThreads>(m, s_m);
  if (threadIdx.x == 0) {
    range[2 * blockIdx.x] = m.lo;
    range[2 * blockIdx.x + 1] = m.hi;
  }
}

// range = {min, max of le, Emin, Emax}; rgb in file order (the reference's Vec3b is B, G, R)
__global__ __launch_bounds__(kRcalThreads) void rcal_plot_e_kernel(const double* __restrict__ E, long long n, const double* __restrict__ range,
                                                                   uint8_t* __restrict__ rgb, uint16_t* __restrict__ e16) {
  const double lmin = range[0], lmax = range[1], emin = range[2], emax = range[3];
  for (long long i = (long long)blockIdx.x * kRcalThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kRcalThreads) {
    const double v = E[i];
    const float val = (float)(3 * (exp((log(v + 20.0) - lmin) / (lmax - lmin)) - 1) / 1.7183);  // :96
    int icP = x86_int(val);
    const float ifP = val - (float)icP;
    icP = icP % 3;
    const uint8_t c = (uint8_t)x86_int(255 * ifP);
    uint8_t r = 0, g = 0, b = 0;  // cv::Vec3b() is zeros: no branch fires for a NaN or a negative val
    if (icP == 0) r = c;
    if (icP == 1) r = 255, g = c;
    if (icP == 2) r = 255, g = 255, b = c;
    rgb[3 * i] = r;
    rgb[3 * i + 1] = g;
    rgb[3 * i + 2] = b;
    e16[i] = (uint16_t)x86_int(255 * 255 * (v - emin) / (emax - emin));  // :108
  }
}

// one workgroup, lane i = column i of the 256 x 256 image: GImg * 255 as cv::imwrite receives it (:120-145)
__global__ __launch_bounds__(256) void rcal_plot_g_kernel(const double* __restrict__ G, float* __restrict__ img, double* __restrict__ range) {
  __shared__ MinMaxFirst<double> s_m[256];
  const int i = threadIdx.x;
  const double g = G[i];
  MinMaxFirst<double> m = mm_start<double>();
  mm_take(m, g, (long long)i);
  m = mm_block<double, 256>(m, s_m);
  if (i == 0) range[0] = m.lo, range[1] = m.hi;
  const double val = 256 * (g - m.lo) / (m.hi - m.lo);
  for (int k = 0; k < 256; k++) img[k * 256 + i] = val < k ? (float)(k - val) * 255.0f : 0.0f;
}

static hipError_t plot_e(const double* d_E, long long n, uint8_t* d_rgb, uint16_t* d_e16, double* range_host, hipStream_t s) {
  const int blocks = (int)std::min<long long>(kPlotBlocks, (n + kRcalThreads - 1) / kRcalThreads);
  MinMaxFirst<double>* d_part = nullptr;
  double* d_range = nullptr;
  hipError_t e = hipMalloc(&d_part, 2 * (size_t)blocks * sizeof(MinMaxFirst<double>));
  if (e == hipSuccess) e = hipMalloc(&d_range, 4 * sizeof(double));
  double range[4] = {0, 0, 0, 0};
  if (e == hipSuccess) {
    rcal_plot_e_range_kernel<<<blocks, kRcalThreads, 0, s>>>(d_E, n, d_part);
    rcal_plot_range_final_kernel<<<2, kRcalThreads, 0, s>>>(d_part, blocks, d_range);
    rcal_plot_e_kernel<<<(int)std::min<long long>(4096, (n + kRcalThreads - 1) / kRcalThreads), kRcalThreads, 0, s>>>(d_E, n, d_range, d_rgb, d_e16);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(range, d_range, sizeof range, hipMemcpyDeviceToHost, s);
  const hipError_t e2 = hipStreamSynchronize(s);  // the scratch is freed below
  (void)hipFree(d_part);
  (void)hipFree(d_range);
  if (e == hipSuccess && e2 == hipSuccess) range_host[0] = range[2], range_host[1] = range[3];
  return e != hipSuccess ? e : e2;
}

static hipError_t plot_g(const double* d_G, float* d_img, double* range_host, hipStream_t s) {
  double* d_range = nullptr;
  hipError_t e = hipMalloc(&d_range, 2 * sizeof(double));
  double range[2] = {0, 0};
  if (e == hipSuccess) {
    rcal_plot_g_kernel<<<1, 256, 0, s>>>(d_G, d_img, d_range);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(range, d_range, sizeof range, hipMemcpyDeviceToHost, s);
  const hipError_t e2 = hipStreamSynchronize(s);
  (void)hipFree(d_range);
  if (e == hipSuccess && e2 == hipSuccess) range_host[0] = range[0], range_host[1] = range[1];
  return e != hipSuccess ? e : e2;
}

}  // namespace mdc

using namespace mdc;

struct mdc_rcal_index {
  mdc::RcalIndex* ix;
  int device;
};

namespace {

bool stack_ok(const void* d_images, const double* d_t, int n, int w, int h) {
  return d_images && d_t && n >= 1 && w >= 1 && h >= 1 && (long long)w * h < (1ll << 31) && (long long)n * w * h < (1ll << 46);
}

}  // namespace

extern "C" {

int mdc_rcal_leak_pad_device(mdc_ctx* c, uint8_t* d_images, int n_images, int w, int h, int leak_padding, void* stream) try {
  if (!c) return no_ctx();
  if (!d_images || n_images < 1 || w < 1 || h < 1 || (long long)w * h >= (1ll << 31))
    return fail(c, MDC_ERR_ARG, "mdc_rcal_leak_pad_device: bad argument");
  ReadLock lk(c->mu);
  DeviceGuard dg(c->device);
  MDC_HIP(c, rcal_leak_pad(d_images, n_images, w, h, leak_padding, (hipStream_t)stream));
  return MDC_OK;
} MDC_CATCH(c)

int mdc_rcal_init_e_device(mdc_ctx* c, const uint8_t* d_images, int n_images, int w, int h, double* d_E, void* stream) try {
  if (!c) return no_ctx();
  if (!d_images || !d_E || n_images < 1 || w < 1 || h < 1 || (long long)w * h >= (1ll << 31) || n_images >= (1 << 24))
    return fail(c, MDC_ERR_ARG, "mdc_rcal_init_e_device: bad argument");
  ReadLock lk(c->mu);
  DeviceGuard dg(c->device);
  MDC_HIP(c, launch_pass<kInit>(d_images, nullptr, n_images, (unsigned)w * h, nullptr, d_E, nullptr, nullptr, nullptr, (hipStream_t)stream));
  return MDC_OK;
} MDC_CATCH(c)

int mdc_rcal_rmse_device(mdc_ctx* c, const uint8_t* d_images, const double* d_exposure, int n_images, int w, int h, const double* d_G,
                         const double* d_E, double* d_out, void* stream) try {
  if (!c) return no_ctx();
  if (!stack_ok(d_images, d_exposure, n_images, w, h) || !d_G || !d_E || !d_out) return fail(c, MDC_ERR_ARG, "mdc_rcal_rmse_device: bad argument");
  ReadLock lk(c->mu);
  DeviceGuard dg(c->device);
  hipStream_t s = (hipStream_t)stream;
  const unsigned wh = (unsigned)w * h;
  RcalWork wk;
  MDC_HIP(c, wk.alloc(wh, false));
  MDC_HIP(c, launch_pass<kRmse>(d_images, d_exposure, n_images, wh, d_G, const_cast<double*>(d_E), wk.slab, nullptr, nullptr, s));
  MDC_HIP(c, rmse_final(wk, d_images, wh, 0, d_out, s));
  MDC_HIP(c, hipStreamSynchronize(s));  // the scratch goes
  return MDC_OK;
} MDC_CATCH(c)

int mdc_rcal_g_step_device(mdc_ctx* c, const uint8_t* d_images, const double* d_exposure, int n_images, int w, int h, const double* d_E,
                           double* d_G, void* stream) try {
  if (!c) return no_ctx();
  if (!stack_ok(d_images, d_exposure, n_images, w, h) || !d_G || !d_E) return fail(c, MDC_ERR_ARG, "mdc_rcal_g_step_device: bad argument");
  ReadLock lk(c->mu);
  DeviceGuard dg(c->device);
  hipStream_t s = (hipStream_t)stream;
  RcalWork wk;
  MDC_HIP(c, wk.alloc((unsigned)w * h, true));
  MDC_HIP(c, g_step_direct(d_images, d_exposure, n_images, (unsigned)w * h, d_E, d_G, wk, nullptr, s));
  MDC_HIP(c, hipStreamSynchronize(s));
  return MDC_OK;
} MDC_CATCH(c)

int mdc_rcal_index_create(mdc_ctx* c, const uint8_t* d_images, int n_images, int w, int h, void* stream, mdc_rcal_index** out) try {
  if (!c) return no_ctx();
  if (!out) return fail(c, MDC_ERR_ARG, "mdc_rcal_index_create: out is NULL");
  *out = nullptr;
  if (!d_images || n_images < 1 || w < 1 || h < 1 || (long long)w * h >= (1ll << 31) || (long long)n_images * w * h >= (1ll << 46))
    return fail(c, MDC_ERR_ARG, "mdc_rcal_index_create: bad argument");
  ReadLock lk(c->mu);
  DeviceGuard dg(c->device);
  mdc::RcalIndex* ix = nullptr;
  std::string why;
  const hipError_t e = mdc::rcal_index_build(d_images, n_images, w, h, (hipStream_t)stream, &ix, &why);
  if (e != hipSuccess) {
    if (!why.empty()) return fail(c, MDC_ERR_NOMEM, "mdc_rcal_index_create: %s", why.c_str());
    return fail(c, MDC_ERR_HIP, "mdc_rcal_index_create: %s", hipGetErrorString(e));
  }
  *out = new mdc_rcal_index{ix, c->device};
  return MDC_OK;
} MDC_CATCH(c)

void mdc_rcal_index_destroy(mdc_rcal_index* index) {
  if (!index) return;
  DeviceGuard dg(index->device);
  mdc::rcal_index_free(index->ix);
  delete index;
}

int64_t mdc_rcal_index_bytes(const mdc_rcal_index* index) {
  return index ? (int64_t)(index->ix->entries * (index->ix->wide ? 8 : 4)) : 0;
}
int64_t mdc_rcal_index_entries(const mdc_rcal_index* index) { return index ? (int64_t)index->ix->entries : 0; }
int64_t mdc_rcal_index_longest_chain(const mdc_rcal_index* index) { return index ? (int64_t)index->ix->longest : 0; }

int mdc_rcal_g_step_indexed_device(mdc_ctx* c, const mdc_rcal_index* index, const double* d_exposure, const double* d_E, double* d_G,
                                   void* stream) try {
  if (!c) return no_ctx();
  if (!index || !d_exposure || !d_E || !d_G) return fail(c, MDC_ERR_ARG, "mdc_rcal_g_step_indexed_device: bad argument");
  if (index->device != c->device) return fail(c, MDC_ERR_ARG, "mdc_rcal_g_step_indexed_device: index built on another device");
  ReadLock lk(c->mu);
  DeviceGuard dg(c->device);
  hipStream_t s = (hipStream_t)stream;
  RcalWork wk;
  MDC_HIP(c, wk.alloc((unsigned)index->ix->w * index->ix->h, false));
  MDC_HIP(c, g_step_indexed(index->ix, d_exposure, d_E, d_G, wk, nullptr, s));
  MDC_HIP(c, hipStreamSynchronize(s));
  return MDC_OK;
} MDC_CATCH(c)

int mdc_rcal_e_step_device(mdc_ctx* c, const uint8_t* d_images, const double* d_exposure, int n_images, int w, int h, const double* d_G,
                           double* d_E, double* d_rmse_g, void* stream) try {
  if (!c) return no_ctx();
  if (!stack_ok(d_images, d_exposure, n_images, w, h) || !d_G || !d_E) return fail(c, MDC_ERR_ARG, "mdc_rcal_e_step_device: bad argument");
  ReadLock lk(c->mu);
  DeviceGuard dg(c->device);
  hipStream_t s = (hipStream_t)stream;
  RcalWork wk;
  MDC_HIP(c, wk.alloc((unsigned)w * h, false));
  MDC_HIP(c, e_step(d_images, d_exposure, n_images, (unsigned)w * h, d_G, d_E, wk, d_rmse_g, s));
  MDC_HIP(c, hipStreamSynchronize(s));
  return MDC_OK;
} MDC_CATCH(c)

int mdc_rcal_rescale_device(mdc_ctx* c, const uint8_t* d_images, const double* d_exposure, int n_images, int w, int h, double* d_G,
                            double* d_E, double* d_rmse_e, double* d_rmse_resc, void* stream) try {
  if (!c) return no_ctx();
  if (!stack_ok(d_images, d_exposure, n_images, w, h) || !d_G || !d_E) return fail(c, MDC_ERR_ARG, "mdc_rcal_rescale_device: bad argument");
  ReadLock lk(c->mu);
  DeviceGuard dg(c->device);
  hipStream_t s = (hipStream_t)stream;
  RcalWork wk;
  MDC_HIP(c, wk.alloc((unsigned)w * h, false));
  MDC_HIP(c, rescale(d_images, d_exposure, n_images, (unsigned)w * h, d_G, d_E, wk, d_rmse_e, d_rmse_resc, s));
  MDC_HIP(c, hipStreamSynchronize(s));
  return MDC_OK;
} MDC_CATCH(c)

int mdc_rcal_plot_e_device(mdc_ctx* c, const double* d_E, int w, int h, uint8_t* d_rgb, uint16_t* d_e16, double* range_host, void* stream) try {
  if (!c) return no_ctx();
  if (!d_E || !d_rgb || !d_e16 || !range_host || w < 1 || h < 1 || (long long)w * h >= (1ll << 31) || ((uintptr_t)d_e16 & 1))
    return fail(c, MDC_ERR_ARG, "mdc_rcal_plot_e_device: bad argument");
  ReadLock lk(c->mu);
  DeviceGuard dg(c->device);
  MDC_HIP(c, plot_e(d_E, (long long)w * h, d_rgb, d_e16, range_host, (hipStream_t)stream));
  return MDC_OK;
} MDC_CATCH(c)

int mdc_rcal_plot_g_device(mdc_ctx* c, const double* d_G, float* d_img, double* range_host, void* stream) try {
  if (!c) return no_ctx();
  if (!d_G || !d_img || !range_host) return fail(c, MDC_ERR_ARG, "mdc_rcal_plot_g_device: bad argument");
  ReadLock lk(c->mu);
  DeviceGuard dg(c->device);
  MDC_HIP(c, plot_g(d_G, d_img, range_host, (hipStream_t)stream));
  return MDC_OK;
} MDC_CATCH(c)

int mdc_rcal_solve_device(mdc_ctx* c, const uint8_t* d_images, const double* d_exposure, int n_images, int w, int h, int iterations,
                          unsigned mode, double* d_G, double* d_E, mdc_rcal_log* log, void* stream) try {
  if (!c) return no_ctx();
  if (!stack_ok(d_images, d_exposure, n_images, w, h) || !d_G || !d_E || iterations < 0 || n_images >= (1 << 24) ||
      (mode != MDC_RCAL_EXACT_ORDER && mode != MDC_RCAL_DIRECT) || (log && iterations > 0 && !log->iters))
    return fail(c, MDC_ERR_ARG, "mdc_rcal_solve_device: bad argument");
  const bool direct = mode == MDC_RCAL_DIRECT;
  mdc_rcal_index* index = nullptr;
  if (!direct && iterations > 0) {
    const int rc = mdc_rcal_index_create(c, d_images, n_images, w, h, stream, &index);
    if (rc != MDC_OK) return rc;
  }
  ReadLock lk(c->mu);
  DeviceGuard dg(c->device);
  hipStream_t s = (hipStream_t)stream;
  const unsigned wh = (unsigned)w * h;
  RcalWork wk;
  double* d_log = nullptr;  // [0..1] init rmse, num; per iteration 8: rmse_G, num_G, rmse_E, num_E, rmse_resc, num_resc, factor, 0
  const size_t log_bytes = (2 + 8 * (size_t)iterations) * sizeof(double);
  auto done = [&](int code) {
    (void)hipStreamSynchronize(s);
    (void)hipFree(d_log);
    mdc_rcal_index_destroy(index);
    return code;
  };
#define MDC_RSOLVE(call_)                                                                               \
  do {                                                                                                  \
    hipError_t e_ = (call_);                                                                            \
    if (e_ != hipSuccess) return done(fail(c, MDC_ERR_HIP, "%s: %s", #call_, hipGetErrorString(e_))); \
  } while (0)
  MDC_RSOLVE(wk.alloc(wh, direct));
  MDC_RSOLVE(hipMalloc(&d_log, log_bytes));
  MDC_RSOLVE(hipMemsetAsync(d_log, 0, log_bytes, s));
  MDC_RSOLVE(hipMemsetAsync(d_G, 0, 256 * sizeof(double), s));  // :248
  MDC_RSOLVE(launch_pass<kInit>(d_images, nullptr, n_images, wh, nullptr, d_E, nullptr, nullptr, nullptr, s));
  MDC_RSOLVE(launch_pass<kRmse>(d_images, d_exposure, n_images, wh, d_G, d_E, wk.slab, nullptr, nullptr, s));  // :270
  MDC_RSOLVE(rmse_final(wk, d_images, wh, 0, d_log, s));
  for (int it = 0; it < iterations; it++) {
    double* row = d_log + 2 + 8 * (size_t)it;
    if (direct) MDC_RSOLVE(g_step_direct(d_images, d_exposure, n_images, wh, d_E, d_G, wk, row + 6, s));
    else MDC_RSOLVE(g_step_indexed(index->ix, d_exposure, d_E, d_G, wk, row + 6, s));
    MDC_RSOLVE(e_step(d_images, d_exposure, n_images, wh, d_G, d_E, wk, row + 0, s));
    MDC_RSOLVE(rescale(d_images, d_exposure, n_images, wh, d_G, d_E, wk, row + 2, row + 4, s));
  }
  std::vector<double> h_log(log_bytes / sizeof(double));
  MDC_RSOLVE(hipMemcpyAsync(h_log.data(), d_log, log_bytes, hipMemcpyDeviceToHost, s));
  MDC_RSOLVE(hipStreamSynchronize(s));
#undef MDC_RSOLVE
  if (log) {
    log->init_rmse = h_log[0];
    log->init_num = h_log[1];
    for (int it = 0; it < iterations; it++) {
      const double* r = &h_log[2 + 8 * (size_t)it];
      log->iters[it] = mdc_rcal_iter{r[0], r[1], r[2], r[3], r[4], r[5], r[6]};
    }
  }
  return done(MDC_OK);
} MDC_CATCH(c)

}  // extern "C"
