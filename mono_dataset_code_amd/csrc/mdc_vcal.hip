// gfx950 kernels, their launchers and the C entry points (mdc_vcal_*) of the vignetteCalib solver's accumulate loops (reference
// src/main_vignetteCalib.cpp:395-527):
// the alternating least-squares iteration that estimates the calibration plane's colour (one value per plane
// point, gw*gh = 10^6 of them) and the per-pixel vignette factor from n images (up to ~1000) of the plane.
// Per half-iteration the reference makes n*gw*gh bilinear gathers from the image stack and from the current
// factor map on ONE core; here a thread owns a plane point (plane step) or a (plane point, image) pair
// (vignette step).  Same arithmetic family as the hot path: FOV-warped coordinates + bilinear taps, f32, no FMA.
//
// Numerics (this file is built with -ffp-contract=off, division correctly rounded):
//   plane step    : every plane point sums over the images in the reference's order -> FF, FC and the new
//                   planeColor are BIT-IDENTICAL to the reference;
//   vignette step : a scatter-add into the image grid.  As written (vcal_vignette_accumulate_kernel, concurrent float
//                   atomics) the reference's sequential order cannot be kept: TT / CT / vignetteFactor agree to ~1e-6
//                   relative (tests/test_vcal.py: 1e-5).  Inverted into an ordered gather over a prebuilt index
//                   (VcalIndex, vcal_vignette_gather_kernel) it is BIT-IDENTICAL and has no atomics on the data path;
//   E (printed only, :449,:523): double sums in tree order instead of sequential order; R is an exact count.
#include "mdc_ctx.h"
#include "minmax_first.h"

namespace mdc {
namespace {

// getInterpolatedElement, src/main_vignetteCalib.cpp:52-70
__device__ __forceinline__ float interp(const float* __restrict__ mat, float x, float y, int width) {
  const int ix = (int)x, iy = (int)y;
  const float dx = x - ix, dy = y - iy, dxdy = dx * dy;
  const float* bp = mat + ix + iy * width;
  return dxdy * bp[1 + width] + (dy - dxdy) * bp[width] + (dx - dxdy) * bp[1] + (1 - dx - dy + dxdy) * bp[0];
}

__device__ __forceinline__ void block_add_er(double e, double r, double* er) {
  __shared__ double s_e[256], s_r[256];
  s_e[threadIdx.x] = e;
  s_r[threadIdx.x] = r;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if ((int)threadIdx.x < k) {
      s_e[threadIdx.x] += s_e[threadIdx.x + k];
      s_r[threadIdx.x] += s_r[threadIdx.x + k];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0 && (s_e[0] != 0 || s_r[0] != 0)) {
    atomicAdd(er, s_e[0]);
    atomicAdd(er + 1, s_r[0]);
  }
}

// the 2x2 footprint of a sample lies inside the image (also false for NaN coordinates)
__device__ __forceinline__ bool vcal_inside(float x, float y, int wI, int hI) {
  return x >= 0.f && y >= 0.f && x < (float)(wI - 1) && y < (float)(hI - 1);
}

// "optimize planeColor" (:400-448): one thread per plane point, images in order
__global__ __launch_bounds__(256) void vcal_plane_kernel(const float* __restrict__ images, const float* __restrict__ p2x,
                                                         const float* __restrict__ p2y, int n, int wI, int hI, int np,
                                                         float* __restrict__ plane_color, const float* __restrict__ vig,
                                                         double oth2, float* __restrict__ FF, float* __restrict__ FC,
                                                         double* __restrict__ er) {
  const int pi = blockIdx.x * 256 + threadIdx.x;
  double E = 0, R = 0;
  if (pi < np) {
    const float pc = plane_color[pi];
    float ff = 0.f, fc = 0.f;
    const size_t img_px = (size_t)wI * hI;
    for (int img = 0; img < n; img++) {
      const float x = p2x[(size_t)img * np + pi];
      if (isnan(x)) continue;
      const float y = p2y[(size_t)img * np + pi];
      // a sample whose 2x2 footprint leaves the image: the reference relies on its caller's mask (:345-357) and would read
      // out of bounds; dropped here, exactly as the contribution index drops it (vcal_sample), so both half-iterations
      // always see the same sample set
      if (!vcal_inside(x, y, wI, hI)) continue;
      const float color = interp(images + img * img_px, x, y, wI);
      const float fac = interp(vig, x, y, wI);
      if (isnan(fac)) continue;
      if (isnan(color)) continue;
      const double residual = (double)((color - pc * fac) * (color - pc * fac));
      if (fabs(residual) > oth2) {
        E += oth2;
        R += 1;
        continue;
      }
      ff += fac * fac;
      fc += color * fac;
      if (isnan(pc)) continue;
      E += residual;
      R += 1;
    }
    FF[pi] = ff;
    FC[pi] = fc;
    plane_color[pi] = ff < 1 ? __builtin_nanf("") : fc / ff;  // :441-447
  }
  block_add_er(E, R, er);
}

// "optimize vignette", accumulation (:461-509): one thread per (plane point, image), bilinear scatter by float atomics
__global__ __launch_bounds__(256) void vcal_vignette_accumulate_kernel(const float* __restrict__ images,
                                                                       const float* __restrict__ p2x,
                                                                       const float* __restrict__ p2y, int wI, int hI, int np,
                                                                       const float* __restrict__ plane_color,
                                                                       const float* __restrict__ vig, double oth2,
                                                                       float* __restrict__ TT, float* __restrict__ CT,
                                                                       double* __restrict__ er) {
  const int pi = blockIdx.x * 256 + threadIdx.x;
  const int img = blockIdx.y;
  double E = 0, R = 0;
  if (pi < np) {
    const float x = p2x[(size_t)img * np + pi];
    const float colorPlane = plane_color[pi];
    const float y = isnan(x) ? 0.f : p2y[(size_t)img * np + pi];
    if (!isnan(x) && !isnan(colorPlane) && vcal_inside(x, y, wI, hI)) {  // (footprint outside the image: dropped, see vcal_plane_kernel)
      const float colorImage = interp(images + (size_t)img * wI * hI, x, y, wI);
      if (!isnan(colorImage)) {
        const float fac = interp(vig, x, y, wI);
        const double residual = (double)((colorImage - colorPlane * fac) * (colorImage - colorPlane * fac));
        if (fabs(residual) > oth2) {
          E = oth2;
          R = 1;
        } else {
          const int ix = (int)x, iy = (int)y;
          const float dx = x - ix, dy = y - iy, dxdy = dx * dy;
          float* tt = TT + ix + iy * wI;
          float* ct = CT + ix + iy * wI;
          unsafeAtomicAdd(tt + 0, (1 - dx - dy + dxdy) * colorPlane * colorPlane);  // :495-498
          unsafeAtomicAdd(tt + 1, (dx - dxdy) * colorPlane * colorPlane);
          unsafeAtomicAdd(tt + wI, (dy - dxdy) * colorPlane * colorPlane);
          unsafeAtomicAdd(tt + 1 + wI, dxdy * colorPlane * colorPlane);
          unsafeAtomicAdd(ct + 0, (1 - dx - dy + dxdy) * colorImage * colorPlane);  // :500-503
          unsafeAtomicAdd(ct + 1, (dx - dxdy) * colorImage * colorPlane);
          unsafeAtomicAdd(ct + wI, (dy - dxdy) * colorImage * colorPlane);
          unsafeAtomicAdd(ct + 1 + wI, dxdy * colorImage * colorPlane);
          if (!isnan(fac)) {
            E = residual;
            R = 1;
          }
        }
      }
    }
  }
  block_add_er(E, R, er);
}

// ---------------------------------------------------------------------------------------------------------
// "optimize vignette" WITHOUT atomics, bit-identical to the reference: the scatter turned into a gather.
// plane2img coordinates and image colours do not change between iterations (:395 ff. only updates planeColor and
// vignetteFactor), so which (image, plane point, corner) lands in which image pixel is fixed.  Built once
// (VcalIndex, below): for every image pixel ("bin") the list of its contributions in the REFERENCE'S ORDER
// (image-major, plane point ascending = the order of the sequential loop :461-509).  Per iteration one lane walks
// one bin's list front to back and adds exactly the terms the reference adds, in the same order, with the same f32
// expressions -> TT, CT and the new vignetteFactor equal the reference's bit for bit, and nothing is atomic.
// Memory layout sized for HBM, not for a cache: 4 entries of 16 bytes per valid (image, point) sample (200 images x
// 10^6 points -> 12.8 GB), ELL-packed per group of 64 consecutive bins (entry k of the 64 bins is one 1-KB line
// group, so a wave's k-th load is one coalesced dwordx4 per lane); a group is as long as its longest bin.
// ---------------------------------------------------------------------------------------------------------
struct __attribute__((aligned(16))) VcalEntry {
  float x, y;     // plane2img coordinates of the sample
  float color;    // interpolated image colour (:473), constant over the iterations
  unsigned pc;    // plane point | corner << 30 (corner 0..3 = +0, +1, +w, +1+w of :495-503)
};
constexpr unsigned kCornerShift = 30;
constexpr int kVcalSlackRows = 8;  // rows a walking wave may read past a group's last row (= its loads in flight)

// validity that does not depend on the iteration: coordinate present (:468), taps inside the image (the reference
// relies on its caller for that, :283-300 -- a sample whose 2x2 footprint leaves the image is dropped here instead
// of writing out of bounds), colour not NaN (:478)
__device__ __forceinline__ bool vcal_sample(const float* __restrict__ images, const float* __restrict__ p2x,
                                            const float* __restrict__ p2y, int img, int pi, int wI, int hI, int np, float* x,
                                            float* y, float* color) {
  *x = p2x[(size_t)img * np + pi];
  if (isnan(*x)) return false;
  *y = p2y[(size_t)img * np + pi];
  if (!vcal_inside(*x, *y, wI, hI)) return false;
  *color = interp(images + (size_t)img * wI * hI, *x, *y, wI);
  return !isnan(*color);
}

__global__ __launch_bounds__(256) void vcal_index_count_kernel(const float* __restrict__ images, const float* __restrict__ p2x,
                                                               const float* __restrict__ p2y, int wI, int hI, int np,
                                                               unsigned* __restrict__ counts) {
  const int pi = blockIdx.x * 256 + threadIdx.x;
  if (pi >= np) return;
  float x, y, c;
  if (!vcal_sample(images, p2x, p2y, blockIdx.y, pi, wI, hI, np, &x, &y, &c)) return;
  unsigned* b = counts + (int)x + (int)y * wI;
  atomicAdd(b, 1u);  // integer counts: the result does not depend on the order
  atomicAdd(b + 1, 1u);
  atomicAdd(b + wI, 1u);
  atomicAdd(b + 1 + wI, 1u);
}

// group g = bins 64g .. 64g+63: length = longest list; exclusive scan of the lengths by one workgroup
__global__ __launch_bounds__(1024) void vcal_index_scan_kernel(const unsigned* __restrict__ counts, int nbins, int ngroups,
                                                               unsigned* __restrict__ glen, unsigned long long* __restrict__ gbase) {
  __shared__ unsigned long long s_sum[1024];
  __shared__ unsigned long long s_carry;
  if (threadIdx.x == 0) s_carry = 0;
  __syncthreads();
  for (int g0 = 0; g0 < ngroups; g0 += 1024) {
    const int g = g0 + threadIdx.x;
    unsigned m = 0;
    if (g < ngroups)
      for (int k = 0; k < 64; k++) {
        const int b = g * 64 + k;
        if (b < nbins) m = max(m, counts[b]);
      }
    if (g < ngroups) glen[g] = m;
    s_sum[threadIdx.x] = m;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {  // Hillis-Steele inclusive scan
      const unsigned long long v = (int)threadIdx.x >= d ? s_sum[threadIdx.x - d] : 0;
      __syncthreads();
      s_sum[threadIdx.x] += v;
      __syncthreads();
    }
    if (g < ngroups) gbase[g] = s_carry + s_sum[threadIdx.x] - m;
    __syncthreads();
    if (threadIdx.x == 1023) s_carry += s_sum[1023];
    __syncthreads();
  }
  if (threadIdx.x == 0) gbase[ngroups] = s_carry;  // total number of 64-entry rows
}

__device__ __forceinline__ size_t vcal_slot(const unsigned long long* __restrict__ gbase, int bin, unsigned k) {
  return ((size_t)gbase[bin >> 6] + k) * 64 + (bin & 63);
}

// entries of ONE image appended to the lists (launched image by image, so lists stay image-major); within the
// image's segment the order is whatever the slot atomics gave -- vcal_index_sort_kernel puts it right
__global__ __launch_bounds__(256) void vcal_index_fill_kernel(const float* __restrict__ images, const float* __restrict__ p2x,
                                                              const float* __restrict__ p2y, int img, int wI, int hI, int np,
                                                              const unsigned long long* __restrict__ gbase,
                                                              unsigned* __restrict__ cursor, VcalEntry* __restrict__ entries) {
  const int pi = blockIdx.x * 256 + threadIdx.x;
  if (pi >= np) return;
  VcalEntry e;
  if (!vcal_sample(images, p2x, p2y, img, pi, wI, hI, np, &e.x, &e.y, &e.color)) return;
  const int bin0 = (int)e.x + (int)e.y * wI;
#pragma unroll
  for (unsigned c = 0; c < 4; c++) {
    const int bin = bin0 + (c & 1) + (c >> 1) * wI;
    e.pc = (unsigned)pi | c << kCornerShift;
    entries[vcal_slot(gbase, bin, atomicAdd(cursor + bin, 1u))] = e;
  }
}

// one lane per bin: the segment [seg_begin, cursor) this image appended, ordered by plane point (insertion sort;
// a pixel receives a handful of samples per image)
__global__ __launch_bounds__(256) void vcal_index_sort_kernel(const unsigned long long* __restrict__ gbase,
                                                              const unsigned* __restrict__ seg_begin,
                                                              const unsigned* __restrict__ cursor, int nbins,
                                                              VcalEntry* __restrict__ entries) {
  const int bin = blockIdx.x * 256 + threadIdx.x;
  if (bin >= nbins) return;
  const unsigned a = seg_begin[bin], b = cursor[bin];
  for (unsigned i = a + 1; i < b; i++) {
    const VcalEntry e = entries[vcal_slot(gbase, bin, i)];
    const unsigned key = e.pc & ((1u << kCornerShift) - 1);
    unsigned j = i;
    while (j > a) {
      const VcalEntry p = entries[vcal_slot(gbase, bin, j - 1)];
      if ((p.pc & ((1u << kCornerShift) - 1)) <= key) break;
      entries[vcal_slot(gbase, bin, j)] = p;
      j--;
    }
    if (j != i) entries[vcal_slot(gbase, bin, j)] = e;
  }
}

// the accumulation (:461-509) as a gather: a wave owns a group of 64 bins, lane = bin, lists walked front to back
__global__ __launch_bounds__(256) void vcal_vignette_gather_kernel(const VcalEntry* __restrict__ entries,
                                                                   const unsigned long long* __restrict__ gbase,
                                                                   const unsigned* __restrict__ glen,
                                                                   const unsigned* __restrict__ counts, int nbins, int wI,
                                                                   const float* __restrict__ plane_color,
                                                                   const float* __restrict__ vig, double oth2,
                                                                   float* __restrict__ TT, float* __restrict__ CT,
                                                                   double* __restrict__ er) {
  const int lane = threadIdx.x & 63;
  const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int bin = g * 64 + lane;
  double E = 0, R = 0;
  if (g * 64 < nbins) {  // wave-uniform
    const unsigned len = bin < nbins ? counts[bin] : 0;
    const unsigned rows = __builtin_amdgcn_readfirstlane(glen[g]);  // wave-uniform trip count
    typedef unsigned v4u __attribute__((ext_vector_type(4)));
    const v4u* row = reinterpret_cast<const v4u*>(entries) + (size_t)gbase[g] * 64 + lane;
    float tt = 0.f, ct = 0.f;  // :457-458
    // Every sample in this bin's list has its 2x2 footprint (:52-70) inside the 3x3 pixels around the bin: the
    // current factors of that neighbourhood live in registers, the taps of interp(vignetteFactor, x, y) are picked
    // from them by the entry's corner.  (Neighbours outside the image are never picked: clamped addresses.)
    float V[3][3];
    {
      const int bx = bin % wI, by = bin / wI, hI = nbins / wI;
#pragma unroll
      for (int r = 0; r < 3; r++)
#pragma unroll
        for (int q = 0; q < 3; q++) {
          const int yy = min(max(by + r - 1, 0), hI - 1), xx = min(max(bx + q - 1, 0), wI - 1);
          V[r][q] = vig[bin < nbins ? yy * wI + xx : 0];
        }
    }
    // Branch-free body: an entry that the reference skips adds +0.0f, which leaves a sum that started at +0 unchanged
    // bit for bit (x + 0 == x for every x but -0, and a sum that starts at +0 never becomes -0).  Loads are
    // unconditional too: the lists are allocated with kVcalSlackRows rows of slack, rows beyond a bin's own length hold
    // padding that `live` masks.
    unsigned Rn = 0;
    for (unsigned k0 = 0; k0 < rows; k0 += kVcalSlackRows) {
      v4u raw[kVcalSlackRows];
#pragma unroll
      for (int u = 0; u < kVcalSlackRows; u++) raw[u] = __builtin_nontemporal_load(row + (size_t)(k0 + u) * 64);
#pragma unroll
      for (int u = 0; u < kVcalSlackRows; u++) {
        const bool live = k0 + u < len;
        const float x = __uint_as_float(raw[u].x), y = __uint_as_float(raw[u].y), colorImage = __uint_as_float(raw[u].z);
        const unsigned corner = raw[u].w >> kCornerShift;
        const float colorPlane = plane_color[live ? raw[u].w & ((1u << kCornerShift) - 1) : 0u];
        const int ix = (int)x, iy = (int)y;
        const float dx = x - ix, dy = y - iy, dxdy = dx * dy;
        // the sample's pixel (ix, iy) is the bin minus the corner offset: rows (1 - cy, 2 - cy), columns (1 - cx, 2 - cx)
        const bool cx = corner & 1, cy = corner >> 1;
        const float a0 = cy ? V[0][0] : V[1][0], a1 = cy ? V[0][1] : V[1][1], a2 = cy ? V[0][2] : V[1][2];
        const float b0 = cy ? V[1][0] : V[2][0], b1 = cy ? V[1][1] : V[2][1], b2 = cy ? V[1][2] : V[2][2];
        const float t00 = cx ? a0 : a1, t01 = cx ? a1 : a2, t10 = cx ? b0 : b1, t11 = cx ? b1 : b2;
        const float w0 = 1 - dx - dy + dxdy, w1 = dx - dxdy, w2 = dy - dxdy;
        const float fac = dxdy * t11 + w2 * t10 + w1 * t01 + w0 * t00;  // getInterpolatedElement, :52-70
        const float diff = colorImage - colorPlane * fac;
        const double residual = (double)(diff * diff);  // :480
        const bool seen = live && !isnan(colorPlane);   // :468 and :478 were settled when the index was built, :477 here
        const bool outlier = fabs(residual) > oth2;     // :481-486 (false for a NaN residual, as in the reference)
        const bool adds = seen && !outlier;
        const float w = cy ? (cx ? dxdy : w2) : (cx ? w1 : w0);
        tt += adds ? w * colorPlane * colorPlane : 0.f;  // :495-498
        ct += adds ? w * colorImage * colorPlane : 0.f;  // :500-503
        // E and R once per sample (its corner-0 entry): oth2 for an outlier, else the residual unless fac is NaN (:505-507)
        const bool counted = seen && corner == 0 && (outlier || !isnan(fac));
        E += counted ? (outlier ? oth2 : residual) : 0.0;
        Rn += counted;
      }
    }
    R = (double)Rn;
    if (bin < nbins) {
      TT[bin] = tt;
      CT[bin] = ct;
    }
  }
  block_add_er(E, R, er);
}

// :511-521: the new factor and its maximum (NaN where fewer than 1 unit of weight arrived)
__global__ __launch_bounds__(256) void vcal_vignette_update_kernel(const float* __restrict__ TT, const float* __restrict__ CT,
                                                                   float* __restrict__ vig, int npix, unsigned* max_bits) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  float v = 0.f;
  if (i < npix) {
    if (TT[i] < 1) vig[i] = __builtin_nanf("");
    else {
      v = CT[i] / TT[i];
      vig[i] = v;
    }
  }
  if (!(v > 0.f)) v = 0.f;  // maxFac starts at 0 and only larger values replace it; NaN never does
  // positive floats order like their bit patterns
  __shared__ unsigned s_m[256];
  s_m[threadIdx.x] = __float_as_uint(v);
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if ((int)threadIdx.x < k) s_m[threadIdx.x] = max(s_m[threadIdx.x], s_m[threadIdx.x + k]);
    __syncthreads();
  }
  if (threadIdx.x == 0 && s_m[0]) atomicMax(max_bits, s_m[0]);
}
// :526-527
__global__ __launch_bounds__(256) void vcal_vignette_normalise_kernel(float* __restrict__ vig, int npix, const unsigned* max_bits) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < npix) vig[i] = vig[i] / __uint_as_float(*max_bits);
}

// :286-291: image = meanExposure * getImage(i, false, true, false, false) / exposure_time (0 counts as 1), float
__global__ __launch_bounds__(256) void vcal_scale_images_kernel(float* __restrict__ images, long long npix, float mean_exposure,
                                                                const float* __restrict__ exposure) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= npix) return;
  float e = exposure[blockIdx.y];
  if (e == 0) e = 1;
  float* p = images + (size_t)blockIdx.y * npix + i;
  *p = mean_exposure * *p / e;
}

// :293-301, the gradient mask of a calibration image: a pixel and a 5 x 5 neighbour that differ by more than maxAbsGrad
// both become NaN -- IN PLACE and in raster order, so a pixel an earlier one masked no longer takes part.  The result
// depends on that order, but only between pixels whose 5 x 5 neighbourhoods intersect (|dx| <= 4, |dy| <= 4), and for
// every such pair the later one in raster order also has the larger t = x + 5*y.  Pixels of equal t are 5 columns apart
// per row -- their neighbourhoods are disjoint -- so sweeping t upwards with all pixels of one t in parallel replays the
// sequential loop exactly.  One workgroup per image (the images of a stack run side by side), a barrier per step.
__global__ __launch_bounds__(256) void vcal_gradient_mask_kernel(float* __restrict__ images, int wI, int hI, float max_abs_grad) {
  volatile float* img = images + (size_t)blockIdx.x * wI * hI;  // volatile: every step sees the NaNs of the steps before
  const int t_last = (wI - 3) + 5 * (hI - 3);
  for (int t = 2 + 5 * 2; t <= t_last; t++) {
    // rows with a pixel on this front: 2 <= x = t - 5y <= wI-3
    const int y_lo = max(2, (t - (wI - 3) + 4) / 5), y_hi = min(hI - 3, (t - 2) / 5);
    for (int y = y_lo + (int)threadIdx.x; y <= y_hi; y += 256) {
      const int x = t - 5 * y;
      const int p = x + y * wI;
      float vp = img[p];
      if (!isnan(vp)) {
        for (int deltax = -2; deltax < 3 && !isnan(vp); deltax++)
          for (int deltay = -2; deltay < 3; deltay++) {
            const int q = p + deltax + deltay * wI;
            if (fabsf(vp - img[q]) > max_abs_grad) {  // false for a NaN neighbour
              vp = __builtin_nanf("");
              img[p] = vp;
              img[q] = vp;
              break;  // image[x+y*wI] is NaN from here on: no later comparison of this pixel can be true
            }
          }
      }
    }
    __syncthreads();
  }
}

// :345-357: plane points whose image position, rounded as (int)(v + 0.5) (float + double), is not strictly inside
// (1, w-2) x (1, h-2) lose both coordinates.  (NaN / out-of-range conversions saturate here and give INT_MIN on the
// reference's x86 -- either way the test fails and the point is masked.)
__device__ __forceinline__ bool vcal_coord_inside(float x, float y, int wI, int hI) {
  const int u_d = (int)(x + 0.5);
  const int v_d = (int)(y + 0.5);
  return u_d > 1 && v_d > 1 && u_d < wI - 2 && v_d < hI - 2;
}

__global__ __launch_bounds__(256) void vcal_mask_coords_kernel(float* __restrict__ x, float* __restrict__ y, long long n, int wI, int hI) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (!vcal_coord_inside(x[i], y[i], wI, hI)) {
    x[i] = __builtin_nanf("");
    y[i] = __builtin_nanf("");
  }
}

// :230-258: one lane per frame turns the marker's 4 corners into HK = float(H) * K_p2idx^-1.  H maps the plane points
// (-0.5, 0.5), (0.5, 0.5), (0.5, -0.5), (-0.5, -0.5) onto the corners exactly: for 4 points the DLT's solution is the
// square-to-quad map (Heckbert 1989), formed here in double and scaled to H(2,2) = 1 as cv::findHomography leaves it.
// K_p2idx^-1 and the product are Eigen's float expressions (>= 3.3): the 3 x 3 inverse as cofactors times 1 / det, a
// coefficient of a product as a0 + (a1 + a2).  Corners 1, 2, 3 on a line give a non-finite HK, other degenerate quads a singular one.
__global__ __launch_bounds__(64) void vcal_plane_homography_kernel(const float* __restrict__ corners, float* __restrict__ hk, int n,
                                                                   int gw, int gh, float facw, float fach) {
  const int f = blockIdx.x * 64 + threadIdx.x;
  if (f >= n) return;
  const float* c = corners + (long long)f * 8;
  const double x0 = c[0], y0 = c[1], x1 = c[2], y1 = c[3], x2 = c[4], y2 = c[5], x3 = c[6], y3 = c[7];
  const double sx = x0 - x1 + x2 - x3, sy = y0 - y1 + y2 - y3;
  const double dx1 = x1 - x2, dx2 = x3 - x2, dy1 = y1 - y2, dy2 = y3 - y2;
  const double det = dx1 * dy2 - dx2 * dy1;
  const double g = (sx * dy2 - dx2 * sy) / det, h = (dx1 * sy - sx * dy1) / det;
  // unit square (u, v) -> image: columns q0 (u), q1 (v), q2 (1); the plane point (X, Y) is (u, v) = (X + 0.5, 0.5 - Y)
  const double q0[3] = {x1 - x0 + g * x1, y1 - y0 + g * y1, g};
  const double q1[3] = {x3 - x0 + h * x3, y3 - y0 + h * y3, h};
  const double q2[3] = {x0, y0, 1.0};
  const double s = 1.0 / (0.5 * g + 0.5 * h + 1.0);
  float H[3][3];
  for (int i = 0; i < 3; i++) {
    H[i][0] = (float)(q0[i] * s);
    H[i][1] = (float)(-q1[i] * s);
    H[i][2] = (float)((0.5 * q0[i] + 0.5 * q1[i] + q2[i]) * s);
  }
  // K_p2idx (:193-197; gw / 2 is an int division) and Eigen's compute_inverse<3>
  const float K[3][3] = {{gw / facw, 0.f, (float)(gw / 2)}, {0.f, gh / fach, (float)(gh / 2)}, {0.f, 0.f, 1.f}};
  float cof[3][3];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
      cof[i][j] = K[i1][j1] * K[i2][j2] - K[i1][j2] * K[i2][j1];
    }
  const float kdet = cof[0][0] * K[0][0] + (cof[1][0] * K[1][0] + cof[2][0] * K[2][0]);
  const float invdet = 1.0f / kdet;
  float* o = hk + (long long)f * 9;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++)  // Kinv(k, j) = cof(j, k) * invdet
      o[i * 3 + j] = H[i][0] * (cof[j][0] * invdet) + (H[i][1] * (cof[j][1] * invdet) + H[i][2] * (cof[j][2] * invdet));
}

// :246-258, :284, :345-357 in one pass: frame blockIdx.y, plane point idx = x + y * gw; pp = HK * (x, y, 1) in Eigen's
// order, u = pp0 / pp2, v = pp1 / pp2, then (with a lens model) distortCoordinates and the coordinate mask of
// vcal_mask_coords_kernel, written straight into the solver's p2x / p2y rows.
template <bool DISTORT>
__global__ __launch_bounds__(256) void vcal_plane_coords_kernel(const float* __restrict__ hk, int gw, int np, DistortModel m, int wI,
                                                                int hI, float* __restrict__ p2x, float* __restrict__ p2y) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= np) return;
  const float* K = hk + (long long)blockIdx.y * 9;
  const int y = idx / gw, x = idx - y * gw;
  const float fx = (float)x, fy = (float)y;
  const float pp0 = K[0] * fx + (K[1] * fy + K[2] * 1.0f);
  const float pp1 = K[3] * fx + (K[4] * fy + K[5] * 1.0f);
  const float pp2 = K[6] * fx + (K[7] * fy + K[8] * 1.0f);
  float u = pp0 / pp2, v = pp1 / pp2;
  if (DISTORT) {
    fov_distort_point(m, u, v);
    if (!vcal_coord_inside(u, v, wI, hI)) u = v = __builtin_nanf("");
  }
  const long long o = (long long)blockIdx.y * np + idx;
  p2x[o] = u;
  p2y[o] = v;
}

// "dilate & smoothe vignette by 4 pixel for output" (:541-566): one pass of the NaN-aware 3 x 3 mean, src -> dst; the nine
// conditional adds in the reference's order, float sum / float count; a pixel without a finite neighbour keeps its value
__global__ __launch_bounds__(256) void vcal_smooth_pass_kernel(const float* __restrict__ src, float* __restrict__ dst, int wI, int hI) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= wI * hI) return;
  const int y = idx / wI, x = idx - y * wI;
  float sum = 0, num = 0;
  const bool xr = x < wI - 1, xl = x > 0, yd = y < hI - 1, yu = y > 0;
  float v;
  if (xr && yd && !isnan(v = src[idx + 1 + wI])) { sum += v; num++; }  // :551-562
  if (xr && !isnan(v = src[idx + 1])) { sum += v; num++; }
  if (xr && yu && !isnan(v = src[idx + 1 - wI])) { sum += v; num++; }
  if (yd && !isnan(v = src[idx + wI])) { sum += v; num++; }
  const float own = src[idx];
  if (!isnan(own)) { sum += own; num++; }
  if (yu && !isnan(v = src[idx - wI])) { sum += v; num++; }
  if (yd && xl && !isnan(v = src[idx - 1 + wI])) { sum += v; num++; }
  if (xl && !isnan(v = src[idx - 1])) { sum += v; num++; }
  if (yu && xl && !isnan(v = src[idx - 1 - wI])) { sum += v; num++; }
  dst[idx] = num > 0 ? sum / num : own;  // :563
}

inline int blocks(long long n) { return (int)((n + 255) / 256); }

// ---- the result images: displayImage (:72-94) and the 16-bit vignette files (:568-583)

constexpr int kVcalPlotBlocks = 256;  // one pass of the range kernel's grid covers 256 * 256 = 65536 plane points

__global__ __launch_bounds__(256) void vcal_plot_range_kernel(const float* __restrict__ I, long long n, MinMaxFirst<float>* __restrict__ part) {
  __shared__ MinMaxFirst<float> s_m[256];
  MinMaxFirst<float> m = mm_start<float>();
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) mm_take(m, I[i], i);
  m = mm_block<float, 256>(m, s_m);
  if (threadIdx.x == 0) part[blockIdx.x] = m;
}

__global__ __launch_bounds__(256) void vcal_plot_range_final_kernel(const MinMaxFirst<float>* __restrict__ part, int nparts, float* __restrict__ range) {
  __shared__ MinMaxFirst<float> s_m[256];
  MinMaxFirst<float> m = mm_start<float>();
  for (int i = threadIdx.x; i < nparts; i += 256) {
    const MinMaxFirst<float> o = part[i];
    mm_take_lo(m, o.lo, o.ilo);
    mm_take_hi(m, o.hi, o.ihi);
  }
  m = mm_block<float, 256>(m, s_m);
  if (threadIdx.x == 0) range[0] = m.lo, range[1] = m.hi;
}

// rgb in file order: the reference's NaN colour Vec3b(0, 0, 255) is B, G, R
__global__ __launch_bounds__(256) void vcal_plot_plane_kernel(const float* __restrict__ I, long long n, const float* __restrict__ range, uint8_t* __restrict__ rgb) {
  const float vmin = range[0], vmax = range[1];
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const float v = I[i];
    const uint8_t c = (uint8_t)x86_int((255 * (v - vmin)) / (vmax - vmin));  // :88, float -> uchar as the Vec3b arguments convert
    const bool nan = v != v;
    rgb[3 * i] = nan ? 255 : c;
    rgb[3 * i + 1] = nan ? 0 : c;
    rgb[3 * i + 2] = nan ? 0 : c;
  }
}

// cv::Mat(h, w, CV_32F, I) * 254.9 * 254.9 -> convertTo(CV_16U): one float scale, saturate_cast<ushort>(cvRound(v))
__global__ __launch_bounds__(256) void vcal_vignette_u16_kernel(const float* __restrict__ I, long long n, uint16_t* __restrict__ out) {
  const float scale = (float)(254.9 * 254.9);
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const float v = I[i] * scale;
    const float r = fminf(fmaxf(rintf(v), 0.0f), 65535.0f);
    out[i] = v != v ? (uint16_t)0 : (uint16_t)(int)r;
  }
}

// vignetteCalib's result images: displayImage's colour picture of the plane (:72-94; range_host = vmin, vmax) and the 16-bit
// quantisation of vignette.png / vignetteSmoothed.png (:568-583); both synchronise `s`
hipError_t launch_vcal_plot_plane(const float* d_plane, long long n, uint8_t* d_rgb, float* range_host, hipStream_t s) {
  const int nparts = (int)std::min<long long>(kVcalPlotBlocks, blocks(n));
  MinMaxFirst<float>* d_part = nullptr;
  float* d_range = nullptr;
  hipError_t e = hipMalloc(&d_part, (size_t)nparts * sizeof(MinMaxFirst<float>));
  if (e == hipSuccess) e = hipMalloc(&d_range, 2 * sizeof(float));
  float range[2] = {0.f, 0.f};
  if (e == hipSuccess) {
    vcal_plot_range_kernel<<<nparts, 256, 0, s>>>(d_plane, n, d_part);
    vcal_plot_range_final_kernel<<<1, 256, 0, s>>>(d_part, nparts, d_range);
    vcal_plot_plane_kernel<<<(int)std::min<long long>(4096, blocks(n)), 256, 0, s>>>(d_plane, n, d_range, d_rgb);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(range, d_range, sizeof range, hipMemcpyDeviceToHost, s);
  const hipError_t e2 = hipStreamSynchronize(s);  // the scratch is freed below
  (void)hipFree(d_part);
  (void)hipFree(d_range);
  if (e == hipSuccess && e2 == hipSuccess) range_host[0] = range[0], range_host[1] = range[1];
  return e != hipSuccess ? e : e2;
}

hipError_t launch_vcal_vignette_u16(const float* d_vignette, int64_t n, uint16_t* d_out, hipStream_t s) {
  if (n > 0) vcal_vignette_u16_kernel<<<(int)std::min<long long>(8192, (n + 255) / 256), 256, 0, s>>>(d_vignette, n, d_out);
  const hipError_t e = hipGetLastError();
  const hipError_t e2 = hipStreamSynchronize(s);
  return e != hipSuccess ? e : e2;
}

// the solver's half-iterations (:400-448, :455-527); d_er = {E, R}
hipError_t launch_vcal_plane_step(const float* d_images, const float* d_p2x, const float* d_p2y, int n, int wI, int hI, int np,
                                  float* d_plane_color, const float* d_vig, int oth2, float* d_ff, float* d_fc, double* d_er,
                                  hipStream_t s) {
  hipError_t e = hipMemsetAsync(d_er, 0, 2 * sizeof(double), s);
  if (e != hipSuccess) return e;
  if (np <= 0) return hipSuccess;
  vcal_plane_kernel<<<blocks(np), 256, 0, s>>>(d_images, d_p2x, d_p2y, n, wI, hI, np, d_plane_color, d_vig, (double)oth2, d_ff, d_fc,
                                               d_er);
  return hipGetLastError();
}

hipError_t launch_vcal_vignette_step(const float* d_images, const float* d_p2x, const float* d_p2y, int n, int wI, int hI, int np,
                                     const float* d_plane_color, float* d_vig, int oth2, float* d_tt, float* d_ct, double* d_er,
                                     unsigned* d_max_bits, hipStream_t s) {
  const size_t img_bytes = (size_t)wI * hI * sizeof(float);
  hipError_t e;
  if ((e = hipMemsetAsync(d_er, 0, 2 * sizeof(double), s)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(d_tt, 0, img_bytes, s)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(d_ct, 0, img_bytes, s)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(d_max_bits, 0, sizeof(unsigned), s)) != hipSuccess) return e;
  if (np > 0 && n > 0)
    vcal_vignette_accumulate_kernel<<<dim3(blocks(np), n), 256, 0, s>>>(d_images, d_p2x, d_p2y, wI, hI, np, d_plane_color, d_vig,
                                                                        (double)oth2, d_tt, d_ct, d_er);
  vcal_vignette_update_kernel<<<blocks((long long)wI * hI), 256, 0, s>>>(d_tt, d_ct, d_vig, wI * hI, d_max_bits);
  vcal_vignette_normalise_kernel<<<blocks((long long)wI * hI), 256, 0, s>>>(d_vig, wI * hI, d_max_bits);
  return hipGetLastError();
}

struct VcalIndex {
  int n = 0, wI = 0, hI = 0, np = 0, nbins = 0, ngroups = 0;
  unsigned* d_counts = nullptr;           // entries per bin
  unsigned* d_glen = nullptr;             // rows (of 64 entries) per group of 64 bins
  unsigned long long* d_gbase = nullptr;  // first row of each group; [ngroups] = total rows
  VcalEntry* d_entries = nullptr;
  unsigned long long rows = 0, samples4 = 0;
};

void vcal_index_free(VcalIndex* ix) {
  if (!ix) return;
  (void)hipFree(ix->d_counts);
  (void)hipFree(ix->d_glen);
  (void)hipFree(ix->d_gbase);
  (void)hipFree(ix->d_entries);
  delete ix;
}

long long vcal_index_bytes(const VcalIndex* ix) { return ix ? (long long)((ix->rows + kVcalSlackRows) * 64 * sizeof(VcalEntry)) : 0; }
long long vcal_index_entries(const VcalIndex* ix) { return ix ? (long long)ix->samples4 : 0; }

// Synchronises the stream twice (list sizes come back to the host before the entries can be allocated): set-up work,
// once per calibration run.
hipError_t vcal_index_build(const float* d_images, const float* d_p2x, const float* d_p2y, int n, int wI, int hI, int np,
                            hipStream_t s, VcalIndex** out) {
  *out = nullptr;
  VcalIndex* ix = new VcalIndex;
  ix->n = n;
  ix->wI = wI;
  ix->hI = hI;
  ix->np = np;
  ix->nbins = wI * hI;
  ix->ngroups = (ix->nbins + 63) / 64;
  unsigned *d_cursor = nullptr, *d_seg = nullptr;
  const size_t bin_bytes = (size_t)ix->nbins * sizeof(unsigned);
  hipError_t e;
  auto bail = [&](hipError_t err) {
    (void)hipFree(d_cursor);
    (void)hipFree(d_seg);
    vcal_index_free(ix);
    return err;
  };
  if ((e = hipMalloc(&ix->d_counts, bin_bytes)) != hipSuccess) return bail(e);
  if ((e = hipMalloc(&ix->d_glen, (size_t)ix->ngroups * sizeof(unsigned))) != hipSuccess) return bail(e);
  if ((e = hipMalloc(&ix->d_gbase, ((size_t)ix->ngroups + 1) * sizeof(unsigned long long))) != hipSuccess) return bail(e);
  if ((e = hipMalloc(&d_cursor, bin_bytes)) != hipSuccess) return bail(e);
  if ((e = hipMalloc(&d_seg, bin_bytes)) != hipSuccess) return bail(e);
  if ((e = hipMemsetAsync(ix->d_counts, 0, bin_bytes, s)) != hipSuccess) return bail(e);
  if ((e = hipMemsetAsync(d_cursor, 0, bin_bytes, s)) != hipSuccess) return bail(e);
  if (np > 0 && n > 0)  // an empty problem has empty lists: every bin keeps the reference's memset value
    vcal_index_count_kernel<<<dim3(blocks(np), n), 256, 0, s>>>(d_images, d_p2x, d_p2y, wI, hI, np, ix->d_counts);
  vcal_index_scan_kernel<<<1, 1024, 0, s>>>(ix->d_counts, ix->nbins, ix->ngroups, ix->d_glen, ix->d_gbase);
  if ((e = hipGetLastError()) != hipSuccess) return bail(e);
  if ((e = hipMemcpyAsync(&ix->rows, ix->d_gbase + ix->ngroups, sizeof(unsigned long long), hipMemcpyDeviceToHost, s)) != hipSuccess)
    return bail(e);
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return bail(e);
  if (ix->rows) {
    if ((e = hipMalloc(&ix->d_entries, ((size_t)ix->rows + kVcalSlackRows) * 64 * sizeof(VcalEntry))) != hipSuccess) return bail(e);
    for (int img = 0; img < n; img++) {
      if ((e = hipMemcpyAsync(d_seg, d_cursor, bin_bytes, hipMemcpyDeviceToDevice, s)) != hipSuccess) return bail(e);
      vcal_index_fill_kernel<<<blocks(np), 256, 0, s>>>(d_images, d_p2x, d_p2y, img, wI, hI, np, ix->d_gbase, d_cursor, ix->d_entries);
      vcal_index_sort_kernel<<<blocks(ix->nbins), 256, 0, s>>>(ix->d_gbase, d_seg, d_cursor, ix->nbins, ix->d_entries);
    }
    if ((e = hipGetLastError()) != hipSuccess) return bail(e);
  }
  // number of list entries (4 per valid sample): sum of the counts, on the host (set-up)
  {
    std::vector<unsigned> h((size_t)ix->nbins);
    if ((e = hipMemcpyAsync(h.data(), ix->d_counts, bin_bytes, hipMemcpyDeviceToHost, s)) != hipSuccess) return bail(e);
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return bail(e);
    for (unsigned v : h) ix->samples4 += v;
  }
  (void)hipFree(d_cursor);
  (void)hipFree(d_seg);
  *out = ix;
  return hipSuccess;
}

hipError_t launch_vcal_vignette_step_indexed(const VcalIndex* ix, const float* d_plane_color, float* d_vig, int oth2, float* d_tt,
                                             float* d_ct, double* d_er, unsigned* d_max_bits, hipStream_t s) {
  hipError_t e;
  if ((e = hipMemsetAsync(d_er, 0, 2 * sizeof(double), s)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(d_max_bits, 0, sizeof(unsigned), s)) != hipSuccess) return e;
  // every bin is written by its lane (empty lists write the reference's memset value 0)
  vcal_vignette_gather_kernel<<<(ix->ngroups + 3) / 4, 256, 0, s>>>(ix->d_entries, ix->d_gbase, ix->d_glen, ix->d_counts, ix->nbins,
                                                                    ix->wI, d_plane_color, d_vig, (double)oth2, d_tt, d_ct, d_er);
  vcal_vignette_update_kernel<<<blocks(ix->nbins), 256, 0, s>>>(d_tt, d_ct, d_vig, ix->nbins, d_max_bits);
  vcal_vignette_normalise_kernel<<<blocks(ix->nbins), 256, 0, s>>>(d_vig, ix->nbins, d_max_bits);
  return hipGetLastError();
}

hipError_t launch_vcal_scale_images(float* d_images, int n, int64_t npix, float mean_exposure, const float* d_exposure,
                                    hipStream_t s) {
  if (n <= 0 || npix <= 0) return hipSuccess;
  vcal_scale_images_kernel<<<dim3(blocks(npix), n), 256, 0, s>>>(d_images, npix, mean_exposure, d_exposure);
  return hipGetLastError();
}

hipError_t launch_vcal_gradient_mask(float* d_images, int n, int wI, int hI, int max_abs_grad, hipStream_t s) {
  if (n <= 0 || wI < 5 || hI < 5) return hipSuccess;  // the loops :293-294 are empty
  vcal_gradient_mask_kernel<<<n, 256, 0, s>>>(d_images, wI, hI, (float)max_abs_grad);
  return hipGetLastError();
}

hipError_t launch_vcal_mask_coords(float* d_x, float* d_y, int64_t n, int wI, int hI, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  vcal_mask_coords_kernel<<<blocks(n), 256, 0, s>>>(d_x, d_y, n, wI, hI);
  return hipGetLastError();
}

// plane -> image coordinates of n frames (:230-258, :284, :345-357); d_corners (n x 8) -> d_hk (n x 9) first when given;
// m == nullptr: the projection only
hipError_t launch_vcal_plane_coords(const float* d_corners, float* d_hk, int n, int gw, int gh, float facw, float fach,
                                    const DistortModel* m, int wI, int hI, float* d_p2x, float* d_p2y, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (d_corners) vcal_plane_homography_kernel<<<(n + 63) / 64, 64, 0, s>>>(d_corners, d_hk, n, gw, gh, facw, fach);
  const int np = gw * gh;
  if (m)
    vcal_plane_coords_kernel<true><<<dim3(blocks(np), n), 256, 0, s>>>(d_hk, gw, np, *m, wI, hI, d_p2x, d_p2y);
  else
    vcal_plane_coords_kernel<false><<<dim3(blocks(np), n), 256, 0, s>>>(d_hk, gw, np, DistortModel{}, 0, 0, d_p2x, d_p2y);
  return hipGetLastError();
}

// four passes, d_vig -> d_ct -> d_tt -> d_ct -> d_tt: d_tt ends as the smoothed map, d_ct as the input of the last pass
// (the reference's TT and CT after :541-566)
hipError_t launch_vcal_smooth(const float* d_vig, int wI, int hI, float* d_tt, float* d_ct, hipStream_t s) {
  const int n = wI * hI;
  vcal_smooth_pass_kernel<<<blocks(n), 256, 0, s>>>(d_vig, d_ct, wI, hI);
  vcal_smooth_pass_kernel<<<blocks(n), 256, 0, s>>>(d_ct, d_tt, wI, hI);
  vcal_smooth_pass_kernel<<<blocks(n), 256, 0, s>>>(d_tt, d_ct, wI, hI);
  vcal_smooth_pass_kernel<<<blocks(n), 256, 0, s>>>(d_ct, d_tt, wI, hI);
  return hipGetLastError();
}

}  // namespace
}  // namespace mdc

using namespace mdc;

struct mdc_vcal_index {
  mdc::VcalIndex* ix;
  int device;
};

extern "C" {

int mdc_vcal_plane_step_device(mdc_ctx* c, const float* d_images, const float* d_p2x, const float* d_p2y, int n_images, int w, int h,
                               int n_plane, float* d_plane_color, const float* d_vignette_factor, int oth2, float* d_ff,
                               float* d_fc, double* d_er, void* stream) try {
  if (!c) return MDC_ERR_ARG;
  if (!d_images || !d_p2x || !d_p2y || !d_plane_color || !d_vignette_factor || !d_ff || !d_fc || !d_er || n_images < 0 || w < 2 ||
      h < 2 || n_plane < 0 || (long long)w * h >= (1ll << 31))  // int pixel indices in the kernel
    return fail(c, MDC_ERR_ARG, "mdc_vcal_plane_step_device: bad argument");
  ReadLock lk(c->mu);
  DeviceGuard dg(c->device);
  MDC_HIP(c, launch_vcal_plane_step(d_images, d_p2x, d_p2y, n_images, w, h, n_plane, d_plane_color, d_vignette_factor, oth2, d_ff,
                                    d_fc, d_er, (hipStream_t)stream));
  return MDC_OK;
} MDC_CATCH(c)

int mdc_vcal_vignette_step_device(mdc_ctx* c, const float* d_images, const float* d_p2x, const float* d_p2y, int n_images, int w,
                                  int h, int n_plane, const float* d_plane_color, float* d_vignette_factor, int oth2, float* d_tt,
                                  float* d_ct, double* d_er, void* stream) try {
  if (!c) return MDC_ERR_ARG;
  if (!d_images || !d_p2x || !d_p2y || !d_plane_color || !d_vignette_factor || !d_tt || !d_ct || !d_er || n_images < 0 ||
      n_images > 65535 || w < 2 || h < 2 || n_plane < 0 || (long long)w * h >= (1ll << 31))  // grid y = n_images; int pixel indices
    return fail(c, MDC_ERR_ARG, "mdc_vcal_vignette_step_device: bad argument");
  ReadLock lk(c->mu);
  DeviceGuard dg(c->device);
  MDC_HIP(c, launch_vcal_vignette_step(d_images, d_p2x, d_p2y, n_images, w, h, n_plane, d_plane_color, d_vignette_factor, oth2,
                                       d_tt, d_ct, d_er, c->d_vcal_max + (c->vcal_max_next++ % mdc_ctx::kVcalMaxWords), (hipStream_t)stream));
  return MDC_OK;
} MDC_CATCH(c)

int mdc_vcal_index_create(mdc_ctx* c, const float* d_images, const float* d_p2x, const float* d_p2y, int n_images, int w, int h,
                          int n_plane, void* stream, mdc_vcal_index** out) try {
  if (!c) return MDC_ERR_ARG;
  if (!out) return fail(c, MDC_ERR_ARG, "mdc_vcal_index_create: out is NULL");
  *out = nullptr;
  if (!d_images || !d_p2x || !d_p2y || n_images < 0 || n_images > 65535 || w < 2 || h < 2 || n_plane < 0 || n_plane >= (1 << 30) ||
      (long long)w * h >= (1ll << 31))
    return fail(c, MDC_ERR_ARG, "mdc_vcal_index_create: bad argument");
  ReadLock lk(c->mu);
  DeviceGuard dg(c->device);
  mdc::VcalIndex* ix = nullptr;
  MDC_HIP(c, mdc::vcal_index_build(d_images, d_p2x, d_p2y, n_images, w, h, n_plane, (hipStream_t)stream, &ix));
  *out = new mdc_vcal_index{ix, c->device};
  return MDC_OK;
} MDC_CATCH(c)

void mdc_vcal_index_destroy(mdc_vcal_index* index) {
  if (!index) return;
  DeviceGuard dg(index->device);
  mdc::vcal_index_free(index->ix);
  delete index;
}

int64_t mdc_vcal_index_bytes(const mdc_vcal_index* index) { return index ? mdc::vcal_index_bytes(index->ix) : 0; }
int64_t mdc_vcal_index_entries(const mdc_vcal_index* index) { return index ? mdc::vcal_index_entries(index->ix) : 0; }

int mdc_vcal_vignette_step_indexed_device(mdc_ctx* c, const mdc_vcal_index* index, const float* d_plane_color,
                                          float* d_vignette_factor, int oth2, float* d_tt, float* d_ct, double* d_er, void* stream) try {
  if (!c) return MDC_ERR_ARG;
  if (!index || !d_plane_color || !d_vignette_factor || !d_tt || !d_ct || !d_er)
    return fail(c, MDC_ERR_ARG, "mdc_vcal_vignette_step_indexed_device: bad argument");
  if (index->device != c->device) return fail(c, MDC_ERR_ARG, "mdc_vcal_vignette_step_indexed_device: index built on another device");
  ReadLock lk(c->mu);
  DeviceGuard dg(c->device);
  MDC_HIP(c, mdc::launch_vcal_vignette_step_indexed(index->ix, d_plane_color, d_vignette_factor, oth2, d_tt, d_ct, d_er,
                                                    c->d_vcal_max + (c->vcal_max_next++ % mdc_ctx::kVcalMaxWords), (hipStream_t)stream));
  return MDC_OK;
} MDC_CATCH(c)

int mdc_vcal_scale_images_device(mdc_ctx* c, float* d_images, int n_images, int64_t npix, float mean_exposure,
                                 const float* d_exposure_times, void* stream) try {
  if (!c) return MDC_ERR_ARG;
  if (n_images < 0 || n_images > 65535 || npix < 0 || (n_images > 0 && npix > 0 && (!d_images || !d_exposure_times)))
    return fail(c, MDC_ERR_ARG, "mdc_vcal_scale_images_device: bad argument");
  ReadLock lk(c->mu);
  DeviceGuard dg(c->device);
  MDC_HIP(c, launch_vcal_scale_images(d_images, n_images, npix, mean_exposure, d_exposure_times, (hipStream_t)stream));
  return MDC_OK;
} MDC_CATCH(c)

int mdc_vcal_gradient_mask_device(mdc_ctx* c, float* d_images, int n_images, int w, int h, int max_abs_grad, void* stream) try {
  if (!c) return MDC_ERR_ARG;
  if (n_images < 0 || (n_images > 0 && !d_images) || w < 1 || h < 1 || (long long)w * h >= (1ll << 31) || max_abs_grad < 0)
    return fail(c, MDC_ERR_ARG, "mdc_vcal_gradient_mask_device: bad argument");
  ReadLock lk(c->mu);
  DeviceGuard dg(c->device);
  MDC_HIP(c, launch_vcal_gradient_mask(d_images, n_images, w, h, max_abs_grad, (hipStream_t)stream));
  return MDC_OK;
} MDC_CATCH(c)

int mdc_vcal_mask_coords_device(mdc_ctx* c, float* d_x, float* d_y, int64_t n, int w, int h, void* stream) try {
  if (!c) return MDC_ERR_ARG;
  if (n < 0 || (n > 0 && (!d_x || !d_y)) || w < 1 || h < 1) return fail(c, MDC_ERR_ARG, "mdc_vcal_mask_coords_device: bad argument");
  ReadLock lk(c->mu);
  DeviceGuard dg(c->device);
  MDC_HIP(c, launch_vcal_mask_coords(d_x, d_y, n, w, h, (hipStream_t)stream));
  return MDC_OK;
} MDC_CATCH(c)

int mdc_vcal_plane_coords_device(mdc_ctx* c, const mdc_fov_model* model, const float* d_corners, float* d_hk, int n, int gw, int gh,
                                 float facw, float fach, float* d_p2x, float* d_p2y, void* stream) try {
  if (!c) return MDC_ERR_ARG;
  if (n < 0 || n > 65535 || gw < 1 || gh < 1 || (long long)gw * gh >= (1ll << 31) ||
      (n > 0 && (!d_hk || !d_p2x || !d_p2y)) || (model && (model->in_w < 1 || model->in_h < 1)))
    return fail(c, MDC_ERR_ARG, "mdc_vcal_plane_coords_device: bad argument");
  ReadLock lk(c->mu);
  DeviceGuard dg(c->device);
  DistortModel m;
  if (model) m = distort_model(model);
  MDC_HIP(c, launch_vcal_plane_coords(d_corners, d_hk, n, gw, gh, facw, fach, model ? &m : nullptr, model ? model->in_w : 0,
                                      model ? model->in_h : 0, d_p2x, d_p2y, (hipStream_t)stream));
  return MDC_OK;
} MDC_CATCH(c)

int mdc_vcal_smooth_device(mdc_ctx* c, const float* d_vignette_factor, int w, int h, float* d_smoothed, float* d_scratch,
                           void* stream) try {
  if (!c) return MDC_ERR_ARG;
  if (!d_vignette_factor || !d_smoothed || !d_scratch || w < 1 || h < 1 || (long long)w * h >= (1ll << 31) ||
      d_smoothed == d_scratch || d_vignette_factor == d_scratch)
    return fail(c, MDC_ERR_ARG, "mdc_vcal_smooth_device: bad argument");
  ReadLock lk(c->mu);
  DeviceGuard dg(c->device);
  MDC_HIP(c, launch_vcal_smooth(d_vignette_factor, w, h, d_smoothed, d_scratch, (hipStream_t)stream));
  return MDC_OK;
} MDC_CATCH(c)

int mdc_vcal_plot_plane_device(mdc_ctx* c, const float* d_plane, int gw, int gh, uint8_t* d_rgb, float* range_host, void* stream) try {
  if (!c) return no_ctx();
  if (!d_plane || !d_rgb || !range_host || gw < 1 || gh < 1 || (long long)gw * gh >= (1ll << 31))
    return fail(c, MDC_ERR_ARG, "mdc_vcal_plot_plane_device: bad argument");
  ReadLock lk(c->mu);
  DeviceGuard dg(c->device);
  MDC_HIP(c, launch_vcal_plot_plane(d_plane, (long long)gw * gh, d_rgb, range_host, (hipStream_t)stream));
  return MDC_OK;
} MDC_CATCH(c)

int mdc_vcal_vignette_u16_device(mdc_ctx* c, const float* d_vignette, int64_t n, uint16_t* d_out, void* stream) try {
  if (!c) return no_ctx();
  if (n < 0 || (n > 0 && (!d_vignette || !d_out)) || ((uintptr_t)d_out & 1) || ((uintptr_t)d_vignette & 3))
    return fail(c, MDC_ERR_ARG, "mdc_vcal_vignette_u16_device: bad argument");
  ReadLock lk(c->mu);
  DeviceGuard dg(c->device);
  MDC_HIP(c, launch_vcal_vignette_u16(d_vignette, n, d_out, (hipStream_t)stream));
  return MDC_OK;
} MDC_CATCH(c)

int mdc_vcal_solve_device(mdc_ctx* c, const float* d_images, const float* d_p2x, const float* d_p2y, int n_images, int w, int h,
                          int n_plane, float* d_plane_color, float* d_vignette_factor, int max_iterations, int outlier_th,
                          double* er_out, void* stream) try {
  if (!c) return MDC_ERR_ARG;
  if (!d_plane_color || !d_vignette_factor || max_iterations < 0 || outlier_th < 0 || outlier_th > 46340)
    return fail(c, MDC_ERR_ARG, "mdc_vcal_solve_device: bad argument");
  if (max_iterations == 0) return MDC_OK;
  mdc_vcal_index* index = nullptr;
  int rc = mdc_vcal_index_create(c, d_images, d_p2x, d_p2y, n_images, w, h, n_plane, stream, &index);
  if (rc != MDC_OK) return rc;
  ReadLock lk(c->mu);
  DeviceGuard dg(c->device);
  hipStream_t s = (hipStream_t)stream;
  float *d_ff = nullptr, *d_fc = nullptr, *d_tt = nullptr, *d_ct = nullptr;
  double* d_er = nullptr;
  const size_t plane_bytes = (size_t)std::max(n_plane, 1) * sizeof(float), img_bytes = (size_t)w * h * sizeof(float);
  const size_t er_bytes = (size_t)max_iterations * 4 * sizeof(double);
  auto done = [&](int code) {
    (void)hipStreamSynchronize(s);
    for (void* p : {(void*)d_ff, (void*)d_fc, (void*)d_tt, (void*)d_ct, (void*)d_er}) (void)hipFree(p);
    mdc_vcal_index_destroy(index);
    return code;
  };
#define MDC_SOLVE(call_)                                                  \
  do {                                                                    \
    hipError_t e_ = (call_);                                              \
    if (e_ != hipSuccess) return done(fail(c, MDC_ERR_HIP, "%s: %s", #call_, hipGetErrorString(e_))); \
  } while (0)
  MDC_SOLVE(hipMalloc(&d_ff, plane_bytes));
  MDC_SOLVE(hipMalloc(&d_fc, plane_bytes));
  MDC_SOLVE(hipMalloc(&d_tt, img_bytes));
  MDC_SOLVE(hipMalloc(&d_ct, img_bytes));
  MDC_SOLVE(hipMalloc(&d_er, er_bytes));
  for (int it = 0; it < max_iterations; it++) {
    const int oth2 = it < max_iterations / 2 ? 10000 * 10000 : outlier_th * outlier_th;  // :397-398
    MDC_SOLVE(launch_vcal_plane_step(d_images, d_p2x, d_p2y, n_images, w, h, n_plane, d_plane_color, d_vignette_factor, oth2, d_ff,
                                     d_fc, d_er + 4 * it, s));
    MDC_SOLVE(mdc::launch_vcal_vignette_step_indexed(index->ix, d_plane_color, d_vignette_factor, oth2, d_tt, d_ct, d_er + 4 * it + 2,
                                                     c->d_vcal_max + (c->vcal_max_next++ % mdc_ctx::kVcalMaxWords), s));
  }
  if (er_out) MDC_SOLVE(hipMemcpyAsync(er_out, d_er, er_bytes, hipMemcpyDeviceToHost, s));
#undef MDC_SOLVE
  return done(MDC_OK);
} MDC_CATCH(c)

}  // extern "C"
