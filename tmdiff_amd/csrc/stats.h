// Device helpers of the fp64 image-statistics kernels (metrics.hip, loss.hip, ssim_loss.hip; the gradient norm of sampler.hip):
// the fixed-order workgroup sum, the walk over a launch's partial sums, and the two LDS tile stagers.
#pragma once
#include "common.h"

namespace tmdiff {

// ---- THE summation order.  A workgroup's sum of one value per lane is: inside each wave the xor butterfly with offsets 32, 16,
// ..., 1 (every lane then holds the wave's total); lane 0 of each wave stores the total to LDS; after a barrier the totals are
// added in ascending wave index, left to right: ((w0 + w1) + w2) + w3.  Every kernel that promises bit-for-bit reproducible sums
// adds through the functions below, so the order is written here and nowhere else.  (One butterfly is narrower than a wave and
// stays where it is used: group_sum of metrics.hip, whose waves are then added by waves_in_order like everyone's.)

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// Column k of the totals that waves w0 .. w0 + nw - 1 stored at red[wave * LD + k], added in ascending wave index.
template <int LD>
__device__ __forceinline__ double waves_in_order(const double* red, int k, int w0, int nw) {
  double s = red[w0 * LD + k];
  for (int i = 1; i < nw; ++i) s += red[(w0 + i) * LD + k];
  return s;
}

// First half of the sum of N values per lane: the butterflies, then lane 0 of wave w stores red[w * LD + k], k < N.  The caller
// syncs (before, if earlier readers of red may be behind, and after) and reads column k with wg_sum_col: in one lane per column
// (metrics_pair_kernel, loss_kernel, which store the columns) or through wg_sum in every lane.
template <int N, int LD>
__device__ __forceinline__ void wg_sum_store(const double (&v)[N], double* red) {
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const double s = wave_sum(v[k]);
    if ((threadIdx.x & 63) == 0) red[(threadIdx.x >> 6) * LD + k] = s;
  }
}
template <int WAVES, int LD>
__device__ __forceinline__ double wg_sum_col(const double* red, int k) {
  return waves_in_order<LD>(red, k, 0, WAVES);
}

// The sum over a workgroup of WAVES waves of N values per lane, in every lane.  No leading barrier.
template <int WAVES, int N, int LD>
__device__ __forceinline__ void wg_sum(double (&v)[N], double* red) {
  wg_sum_store<N, LD>(v, red);
  __syncthreads();
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = wg_sum_col<WAVES, LD>(red, k);
}

// One value per lane over 256 threads (red: 4 doubles).
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
  double a[1] = {v};
  wg_sum<4, 1, 1>(a, red);
  return a[0];
}

// src[i * stride] for i = first, first + step, ... below n, added in ascending i: a finalize kernel's lane `first` of `step` adds
// its share of the partial sums a launch left in its workspace, so the order depends on n alone.
__device__ __forceinline__ double strided_sum(const double* src, long n, long stride, long first, long step) {
  double s = 0.0;
  for (long i = first; i < n; i += step) s += src[i * stride];
  return s;
}

// ---- LDS tile stagers ------------------------------------------------------------------------------------------------------

// Rows yy0 .. yy0 + LH - 1 and columns xx0 .. xx0 + LW - 1 of the H x W planes pa and pb into sa and sb (row stride LS), zero
// outside the image, by NT threads.  T = float stages the values; T = double stages the fp64 sums pa + pm and pb + pm.  `vec`:
// 16-byte loads; the caller has checked W % 4 == 0 and the planes' alignment, and xx0 and LW are multiples of 4, so that four
// columns lie inside the image or outside it together.  Otherwise scalar loads, where a lane outside the image reads element
// (0, 0), always a valid one.  A plane has fewer than 2^31 elements.
template <class T, int LH, int LW, int LS, int NT>
__device__ __forceinline__ void stage_halo_tile(T* sa, T* sb, const float* pa, const float* pb, const float* pm, int yy0, int xx0,
                                                int H, int W, bool vec) {
  constexpr bool MS = std::is_same<T, double>::value;
  auto staged = [](float v, float m) -> T {
    if constexpr (MS) return (double)v + (double)m;
    else return v;
  };
  if (LW % 4 == 0 && LS % 4 == 0 && vec) {
    for (int i = threadIdx.x; i < LH * (LW / 4); i += NT) {
      const int ly = i / (LW / 4), lq = i - ly * (LW / 4);
      const int yy = yy0 + ly, xx = xx0 + 4 * lq;
      float4 va = make_float4(0.f, 0.f, 0.f, 0.f), vb = va, vm = va;
      if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
        const int off = yy * W + xx;
        va = *reinterpret_cast<const float4*>(pa + off);
        vb = *reinterpret_cast<const float4*>(pb + off);
        if constexpr (MS) vm = *reinterpret_cast<const float4*>(pm + off);
      }
      T* da = sa + ly * LS + 4 * lq;
      T* db = sb + ly * LS + 4 * lq;
      da[0] = staged(va.x, vm.x); da[1] = staged(va.y, vm.y); da[2] = staged(va.z, vm.z); da[3] = staged(va.w, vm.w);
      db[0] = staged(vb.x, vm.x); db[1] = staged(vb.y, vm.y); db[2] = staged(vb.z, vm.z); db[3] = staged(vb.w, vm.w);
    }
  } else {
    for (int i = threadIdx.x; i < LH * LW; i += NT) {
      const int ly = i / LW, lx = i - ly * LW;
      const int yy = yy0 + ly, xx = xx0 + lx;
      const bool in = yy >= 0 && yy < H && xx >= 0 && xx < W;
      const int off = in ? yy * W + xx : 0;
      const float va = pa[off], vb = pb[off];
      float vm = 0.f;
      if constexpr (MS) vm = pm[off];
      sa[ly * LS + lx] = in ? staged(va, vm) : (T)0;
      sb[ly * LS + lx] = in ? staged(vb, vm) : (T)0;
    }
  }
}

// The block x block windows of Q2n and of the block-wise D_s: block is 8, 16 or 32.
__device__ __forceinline__ int log2_block(int block) { return block == 8 ? 3 : block == 16 ? 4 : 5; }

// The window at (y0, x0) of K images into LDS by NT threads in one walk, mirrored at the bottom and the right: row H + k is row
// H - 1 - k, and columns likewise (the host checked that the mirror stays inside the image).  BANDS: bands 0 .. Cp - 1 of image j
// (channel stride sC[j]), band c at dst[j] + c * bs, the bands from C on zero.  Otherwise one band, and sC, C, Cp, bs are not read.
template <int NT, bool BANDS, int K>
__device__ __forceinline__ void stage_mirrored(float* const (&dst)[K], const float* const (&src)[K], const long (&sC)[K], int C, int Cp,
                                               int bs, int block, int y0, int x0, int H, int W) {
  const int lb = log2_block(block), n = block * block;
  for (int i = threadIdx.x; i < (BANDS ? Cp * n : n); i += NT) {
    const int c = BANDS ? i >> (2 * lb) : 0, px = BANDS ? i & (n - 1) : i;
    int yy = y0 + (px >> lb), xx = x0 + (px & (block - 1));
    yy = yy < H ? yy : 2 * H - 1 - yy;
    xx = xx < W ? xx : 2 * W - 1 - xx;
    const bool in = !BANDS || c < C;
    const int cc = in ? c : 0, off = yy * W + xx, at = BANDS ? c * bs + px : px;
    float v[K];
#pragma unroll
    for (int j = 0; j < K; ++j) v[j] = src[j][(BANDS ? (long)cc * sC[j] : 0) + off];
#pragma unroll
    for (int j = 0; j < K; ++j) dst[j][at] = in ? v[j] : 0.f;
  }
}

}  // namespace tmdiff
