// The minimum and maximum of a sequence as the reference's plotting loops leave them (src/main_responseCalib.cpp:77-89, 125-131,
// src/main_vignetteCalib.cpp:74-81): both start from 1e10 / -1e10 and are replaced under a strict comparison only, so a NaN is never
// taken and, among equal values, the FIRST in index order stays -- which matters for zeros, whose sign shows in the printed "%f".
// A parallel reduction returns that element by carrying the index: (value, index) pairs under "smaller value, then smaller index" are
// totally ordered, so the result does not depend on how the reduction is grouped.  The start value carries the largest index: an
// element equal to it may replace it, with the same bits.
// Beside it, the other thing those loops' pictures need on the device and C does not give: x86's float -> int conversion (x86_int).
#pragma once
#include <hip/hip_runtime.h>

namespace mdc {

template <typename T>
struct MinMaxFirst {
  T lo, hi;
  long long ilo, ihi;
};

template <typename T>
__device__ __forceinline__ MinMaxFirst<T> mm_start() {
  MinMaxFirst<T> m;
  m.lo = (T)1e10;
  m.hi = (T)-1e10;
  m.ilo = m.ihi = 0x7fffffffffffffffll;
  return m;
}

template <typename T>
__device__ __forceinline__ void mm_take_lo(MinMaxFirst<T>& m, T v, long long i) {
  if (v < m.lo || (v == m.lo && i < m.ilo)) m.lo = v, m.ilo = i;
}
template <typename T>
__device__ __forceinline__ void mm_take_hi(MinMaxFirst<T>& m, T v, long long i) {
  if (v > m.hi || (v == m.hi && i < m.ihi)) m.hi = v, m.ihi = i;
}
template <typename T>
__device__ __forceinline__ void mm_take(MinMaxFirst<T>& m, T v, long long i) {
  mm_take_lo(m, v, i);
  mm_take_hi(m, v, i);
}

// over a workgroup of THREADS (a power of two) lanes: every lane returns the result; `s` is THREADS entries of LDS
template <typename T, int THREADS>
__device__ __forceinline__ MinMaxFirst<T> mm_block(MinMaxFirst<T> m, MinMaxFirst<T>* s) {
  s[threadIdx.x] = m;
  __syncthreads();
  for (int k = THREADS / 2; k > 0; k >>= 1) {
    if ((int)threadIdx.x < k) {
      MinMaxFirst<T> a = s[threadIdx.x];
      const MinMaxFirst<T> b = s[threadIdx.x + k];
      mm_take_lo(a, b.lo, b.ilo);
      mm_take_hi(a, b.hi, b.ihi);
      s[threadIdx.x] = a;
    }
    __syncthreads();
  }
  m = s[0];
  __syncthreads();
  return m;
}

// (int)v as x86's cvttss2si / cvttsd2si leave it: truncation, and INT_MIN ("integer indefinite") for a NaN or a value outside int
template <typename T>
__device__ __forceinline__ int x86_int(T v) {
  return (v > (T)-2147483649.0 && v < (T)2147483648.0) ? (int)v : (int)0x80000000;
}

}  // namespace mdc
