// What the classical pansharpening baselines share (MTF-GLP: metrics.hip, fusion.hip; component substitution: cs_fusion.hip;
// BDSD: bdsd.hip): the Gram tile of the fp64 matrix instruction, the root-free Cholesky solve, the loads and stores of a lane's
// four pixels, the dispatch over the band count and the extent check.  Each contract is written here and nowhere else.
#pragma once
#include <algorithm>
#include <type_traits>

#include "stats.h"

namespace tmdiff {

// ---- THE Gram tile.  v_mfma_f64_16x16x4_f64 keeps a 16 x 16 tile in four doubles per lane: entry (row, col) is register reg of
// lane l with col = l & 15, row = (l >> 4) + 4 reg.  The kernels issue the instruction themselves (their operands differ, and the
// order of issue is part of their summation order); a wave's finished tile then goes to red[wave * LD + base + row * 16 + col],
// from where waves_in_order (stats.h) adds the waves' tiles entry by entry.
typedef double gram_tile __attribute__((ext_vector_type(4)));

template <int LD>
__device__ __forceinline__ void store_gram_tile(double* red, int wave, int base, int lane, const gram_tile& acc) {
#pragma unroll
  for (int r = 0; r < 4; ++r) red[wave * LD + base + ((lane >> 4) + 4 * r) * 16 + (lane & 15)] = acc[r];
}

// ---- THE solve: the unpivoted Cholesky factorisation in its root-free form, A = L D L' with a unit lower triangle, and the two
// triangular solves, in the loop order of metrics._ldl_factor / _ldl_solve: every loop ascends (the back substitution descends
// over i and ascends over k), and every product and every difference is rounded on its own.  The pragma stands inside these
// bodies because it is lexical: one in the calling kernel does not reach an inlined helper, and a contracted
// t - a * (b * p) turns the pivot of a duplicated row from exactly non-positive into a rounding residue.  One lane runs them;
// fac (leading dimension LD), piv, z and x live in LDS.

// The factor of the n x n matrix a (leading dimension lda; the lower triangle is read): L into fac below the diagonal, D into
// piv.  Returns whether a pivot was not positive (NaN counts); the factor is then not to be used.
template <int LD>
__device__ __forceinline__ bool ldl_factor(const double* a, int lda, int n, double* fac, double* piv) {
#pragma clang fp contract(off)
  bool bad = false;
  for (int j = 0; j < n; ++j) {
    double dj = a[j * lda + j];
    for (int k = 0; k < j; ++k) dj = dj - fac[j * LD + k] * (fac[j * LD + k] * piv[k]);
    bad = bad || !(dj > 0.0);
    piv[j] = dj;
    for (int i = j + 1; i < n; ++i) {
      double t = a[i * lda + j];
      for (int k = 0; k < j; ++k) t = t - fac[i * LD + k] * (fac[j * LD + k] * piv[k]);
      fac[i * LD + j] = t / dj;
    }
  }
  return bad;
}

// x = A^-1 r for the right-hand side r[i * stride], i < n:  L z = r,  w = z / d,  L' x = w.
template <int LD>
__device__ __forceinline__ void ldl_solve(const double* r, int stride, int n, const double* fac, const double* piv, double* z,
                                          double* x) {
#pragma clang fp contract(off)
  for (int i = 0; i < n; ++i) {
    double t = r[i * stride];
    for (int k = 0; k < i; ++k) t = t - fac[i * LD + k] * z[k];
    z[i] = t;
  }
  for (int i = n - 1; i >= 0; --i) {
    double t = z[i] / piv[i];
    for (int k = i + 1; k < n; ++k) t = t - fac[k * LD + i] * x[k];
    x[i] = t;
  }
}

// ---- Pixel quads: a lane's four consecutive pixels of a plane.  With `vec` they are one 16-byte access at p + off[0] (the
// host has checked that the four lie together at an aligned address); otherwise the first cnt <= 4 of them are scalar accesses
// at p + off[e], with the same values.  A load leaves 0 in the pixels past cnt; a store leaves them alone.
__device__ __forceinline__ void load_quad(const float* p, const int (&off)[4], bool vec, int cnt, float (&v)[4]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = 0.f;
  if (vec) *reinterpret_cast<float4*>(v) = *reinterpret_cast<const float4*>(p + off[0]);
  else
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (e < cnt) v[e] = p[off[e]];
}
__device__ __forceinline__ void store_quad(float* p, const int (&off)[4], bool vec, int cnt, const float (&v)[4]) {
  if (vec) *reinterpret_cast<float4*>(p + off[0]) = *reinterpret_cast<const float4*>(v);
  else
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (e < cnt) p[off[e]] = v[e];
}
// The four are contiguous from p on: the offsets are constants and cost nothing.
__device__ __forceinline__ void load_quad(const float* p, bool vec, int cnt, float (&v)[4]) {
  const int off[4] = {0, 1, 2, 3};
  load_quad(p, off, vec, cnt, v);
}
__device__ __forceinline__ void store_quad(float* p, bool vec, int cnt, const float (&v)[4]) {
  const int off[4] = {0, 1, 2, 3};
  store_quad(p, off, vec, cnt, v);
}

// The four pixels from px on of a flat plane of n pixels as fp64 differences from the plane's pilot (its first pixel):
// d = (double)v - pilot, exact for fp32 data of one binade range.  A pixel past the end is the pilot itself, so d == 0 there.
// `real` false: a filler row that reads nothing, whose pilot is 0 and whose pixels inside the plane are `fill` (the Gram tile's
// row of ones, and the zero rows past it).  `vec`: n % 4 == 0 and the plane is 16-byte aligned, so the four lie inside together.
__device__ __forceinline__ void load_quad_minus_pilot(const float* plane, bool real, float pilot, float fill, long px, int n,
                                                      bool vec, double (&d)[4]) {
  float v[4];
  if (real && vec && px < n) {
    *reinterpret_cast<float4*>(v) = *reinterpret_cast<const float4*>(plane + px);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = px + e < n ? (real ? plane[px + e] : fill) : pilot;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) d[e] = (double)v[e] - (double)pilot;
}

// Blocks of bx pixels across in an image w pixels wide: the offset of pixel q (row-major inside the block, q = row bx + col)
// of the block of n pixels whose first pixel is at org.  q is clamped to the block, so the offset is always a valid one.
__device__ __forceinline__ int block_offset(int org, long q, int n, int bx, int w) {
  const int qe = (int)min(q, (long)n - 1);
  return org + (qe / bx) * w + qe % bx;
}

// ---- Host side.

// launch(std::integral_constant<int, C>) for C == bands, 1 <= C <= MAXC; nothing for another band count (the extent check has
// refused it before).
template <int MAXC, int C = 1, class F>
void dispatch_bands(int bands, F&& launch) {
  if constexpr (C <= MAXC) {
    if (bands == C) launch(std::integral_constant<int, C>{});
    else dispatch_bands<MAXC, C + 1>(bands, launch);
  }
}

// The extents every entry point of the baselines accepts: [B, C, H, W] images with B >= 0, 1 <= C <= maxc, H, W >= 1 and fewer
// than 2^31 elements.
inline bool planes_ok(int B, int C, int maxc, int H, int W) {
  return B >= 0 && C >= 1 && C <= maxc && H >= 1 && W >= 1 && fits_int32((double)std::max(B, 1) * C * H * W);
}

}  // namespace tmdiff
