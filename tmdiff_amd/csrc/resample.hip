// Resampling of full-resolution scenes on gfx950: the Gaussian pyramid step that makes the low-resolution PAN of the QNR metrics
// (pyr_down; the reference's cv2.pyrDown(cv2.pyrDown(pan)), core/metrics.py:328-329) and the bilinear x2 / x4 upsampling that makes
// MS from raw multispectral data (upsample_bilinear; cv2.resize(INTER_LINEAR), data/LRHR_dataset.py:59-84).  Both work on dense
// fp32 planes [planes, H, W] with 32-bit element offsets, use plain vector loads and stores and no atomics.
//
// pyr_down, one level (OpenCV's defaults): the separable 5-tap filter [1 4 6 4 1] / 16, horizontal pass then vertical pass, border
// BORDER_REFLECT_101 (-1 -> 1, -2 -> 2, L -> L - 2, L + 1 -> L - 3), output extent (L + 1) / 2 sampled at the even coordinates.
// Every 5-tap sum is tap5() below, written with explicit roundings, so a pixel's value does not depend on which kernel or which
// workgroup made it.  Two levels run as ONE kernel: a workgroup owns a t x t tile of the level-2 image, stages the input patch
// it needs in LDS, builds its level-1 patch there (reflected at level 1's own borders) and filters that again.  Level 1 -- a
// quarter of the input -- never goes to HBM, and the result equals two one-level calls bit for bit.
//
// Patches hold ACTUAL coordinates: the rows (columns) of the source image between the reflected extremes of what the tile's
// valid outputs need, at most 2n + 3 for n outputs; a tap reads patch[reflect(coordinate) - origin].  With every extent >= 3
// the reflection of a coordinate a tile needs lies inside its own patch (the mirror of L + 1 is L - 3 = 2 (last output) - 2).
//
// LDS budget (256 lanes per workgroup):
//   two levels, t = 16: input patch (4t + 9)^2 = 73 x 73, horizontal pass 73 x (2t + 3) = 73 x 35 (reused by level 2's 35 x 16),
//                       level-1 patch 35 x 35: (5329 + 2555 + 1225) * 4 = 36436 bytes -> 4 workgroups per CU (160 KiB)
//   one level,  t = 32: input patch (2t + 3)^2 = 67 x 67, horizontal pass 67 x 32: (4489 + 2144) * 4 = 26532 bytes -> 6 per CU
// The horizontal pass reads LDS at a stride of two dwords (2-way bank conflicts on ds_read_b32); at 16 input bytes per output
// pixel the LDS traffic stays far below what HBM delivers to a CU.
//
// upsample_bilinear: half-pixel centres, src = (dst + 0.5) / ratio - 0.5 clamped to [0, L - 1] (F.interpolate(mode="bilinear",
// align_corners=False)).  With ratio 2 or 4 every weight is a multiple of 1/8.  A lerp is fma(f, b - a, a): a clamped sample
// has a == b and returns a exactly.  One lane writes four neighbouring pixels of an output row (16 bytes) from the 3 (x4) or 4
// (x2) source columns they touch in two source rows; the scalar form (odd w at x2, unaligned tensors) computes the same values.
//
// upsample_poly23: the Pansharpening Toolbox's interp23tap, which makes the `lms` of the PanCollection files: per x2 stage zero
// insertion and the 23-tap half-band kernel h[d] = 2 c_|d| with circular borders, along H then along W.  h[0] = 1 and the other
// even taps are 0, so a stage copies its input to every second output and sets the outputs between to
// sum_j a_j (s[lo - j] + s[lo + 1 + j]), a_j = 2 c_(2j+1), j = 0..5, over the six samples either side: poly23() below, the pair
// sums first, then a chain of six fused multiply-adds from j = 5 down to 0, every rounding explicit.  Phase 1 puts the samples
// at the odd outputs (S_1), phase 0 at the even ones (S_0); x4 is a phase-1 stage followed by a phase-0 stage, which places
// x[i, j] at y[4i + 2, 4j + 2].
//
// In the coordinates of a tile every stage reads the same way.  With n outputs along an axis and the source patch starting at
// (first output) / 2 - 5 - q, unit u of a line is
//     out[2u + q] = s[u + 5 + q]        out[2u + 1 - q] = poly23(s[u .. u + 11])
// (q: the phase of the stage).  Only the staging of the input patch wraps coordinates (a true modulus, so an extent below the
// reach wraps as often as it must); the passes work on unwrapped patch coordinates, and as every value is one poly23 of values
// that do not depend on the tile, a pixel's bits do not depend on tile, grid, or fused against staged execution.
//
// A 256-lane workgroup owns a 64 x 64 tile of the output.  x2: patch 43 x 43 (32 + 11), H pass into 64 x 43, W pass to global.
// x4 is ONE kernel: the x2 image is 1/4 of the output and never goes to HBM.  The first stage runs in front, in LDS -- input
// patch 32 x 32 (the 43 x2 rows start at an odd coordinate, 32 t - 5, so in patch coordinates that stage reads as q = 0 too),
// H pass into 43 x 32, W pass into the 43 x 43 patch of the second stage.
// LDS (row stride 44 where a pass writes or reads pairs of floats): x2 (43 + 64) * 44 * 4 = 18832 bytes;
//   x4 adds (32 * 32 + 43 * 32) * 4 = 9600: 28432 bytes -> 5 workgroups per CU (160 KiB).
// A lane of an H pass makes the two rows of a unit at one column (consecutive lanes, consecutive columns: no bank conflict); a
// lane of the last W pass makes four neighbouring pixels of an output row (two units) from 14 floats read as 7 x 8 bytes
// (consecutive lanes 8 bytes apart: no bank conflict) and writes 16 bytes; the scalar form (odd w at x2, unaligned output)
// makes one unit per lane with the same poly23 calls, hence the same bits.
#include <algorithm>

#include "common.h"

namespace {

__device__ __forceinline__ int reflect101(int i, int L) { return i < 0 ? -i : (i >= L ? 2 * L - 2 - i : i); }

// (a + e) / 16 + (b + d) / 4 + c * 3 / 8: five roundings (the products by powers of two are exact), the same in every kernel
__device__ __forceinline__ float tap5(float a, float b, float c, float d, float e) {
  const float inner = __fmaf_rn(__fadd_rn(b, d), 0.25f, __fmul_rn(c, 0.375f));
  return __fmaf_rn(__fadd_rn(a, e), 0.0625f, inner);
}

// extent of the patch of a source axis of length L that the outputs [o0, o1] of one level need
struct Span {
  int lo, n;
};
__device__ __forceinline__ Span source_span(int o0, int o1, int L) {
  const int lo = max(2 * o0 - 2, 0), hi = min(2 * o1 + 2, L - 1);
  return {lo, hi - lo + 1};
}

// One level on a patch in LDS.  src: rows sy.lo.. / columns sx.lo.. of an SH x SW image, row stride SS.  tmp (row stride TS)
// receives the horizontal pass: the source rows, the output columns [ox0, ox0 + ow).  put(i, j, v) takes output
// (oy0 + i, ox0 + j).  TS is also the (constant) divisor of the index decode, so ow <= TS.
template <int SS, int TS, class Put>
__device__ __forceinline__ void level_pass(const float* src, float* tmp, Span sy, Span sx, int SH, int SW, int oy0, int oh, int ox0,
                                           int ow, Put put) {
  for (int idx = threadIdx.x; idx < sy.n * TS; idx += 256) {
    const int r = idx / TS, j = idx - r * TS;
    if (j >= ow) continue;
    const float* row = src + r * SS - sx.lo;
    const int x = 2 * (ox0 + j);
    tmp[r * TS + j] = tap5(row[reflect101(x - 2, SW)], row[reflect101(x - 1, SW)], row[x], row[reflect101(x + 1, SW)],
                           row[reflect101(x + 2, SW)]);
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < oh * TS; idx += 256) {
    const int i = idx / TS, j = idx - i * TS;
    if (j >= ow) continue;
    const float* col = tmp + j - sy.lo * TS;
    const int y = 2 * (oy0 + i);
    put(i, j, tap5(col[reflect101(y - 2, SH) * TS], col[reflect101(y - 1, SH) * TS], col[y * TS], col[reflect101(y + 1, SH) * TS],
                   col[reflect101(y + 2, SH) * TS]));
  }
}

template <int LEVELS>
struct PyrTile {
  static constexpr int T = LEVELS == 2 ? 16 : 32;    // edge of the output tile
  static constexpr int P1 = 2 * T + 3;                // level-1 patch of a two-level tile (and the one-level input patch)
  static constexpr int P0 = LEVELS == 2 ? 2 * P1 + 3 : P1;   // input patch: 4t + 9 / 2t + 3
  static constexpr int TW = LEVELS == 2 ? P1 : T;     // columns of the first horizontal pass
};

// y[pl, oy, ox] of the level-LEVELS image.  blockIdx.x is the tile of a plane, blockIdx.y walks the planes.
template <int LEVELS>
__global__ void __launch_bounds__(256) pyr_down_kernel(const float* __restrict__ x, float* __restrict__ y, int planes, int H, int W) {
  using K = PyrTile<LEVELS>;
  __shared__ float s_in[K::P0 * K::P0];
  __shared__ float s_tmp[K::P0 * K::TW];
  __shared__ float s_l1[LEVELS == 2 ? K::P1 * K::P1 : 1];
  const int H1 = (H + 1) / 2, W1 = (W + 1) / 2;
  const int HO = LEVELS == 2 ? (H1 + 1) / 2 : H1, WO = LEVELS == 2 ? (W1 + 1) / 2 : W1;
  const int tiles_x = (WO + K::T - 1) / K::T;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int oy0 = ty * K::T, ox0 = tx * K::T;
  const int oh = min(K::T, HO - oy0), ow = min(K::T, WO - ox0);
  // the spans of the last level's source, and (two levels) of the input under it
  const Span ly = source_span(oy0, oy0 + oh - 1, LEVELS == 2 ? H1 : H), lx = source_span(ox0, ox0 + ow - 1, LEVELS == 2 ? W1 : W);
  const Span iy = LEVELS == 2 ? source_span(ly.lo, ly.lo + ly.n - 1, H) : ly;
  const Span ix = LEVELS == 2 ? source_span(lx.lo, lx.lo + lx.n - 1, W) : lx;
  for (int pl = blockIdx.y; pl < planes; pl += gridDim.y) {
    const float* xp = x + (pl * H + iy.lo) * W + ix.lo;
    for (int idx = threadIdx.x; idx < iy.n * K::P0; idx += 256) {
      const int r = idx / K::P0, c = idx - r * K::P0;
      if (c < ix.n) s_in[idx] = xp[r * W + c];
    }
    __syncthreads();
    float* yp = y + (pl * HO + oy0) * WO + ox0;
    const auto store = [&](int i, int j, float v) { yp[i * WO + j] = v; };
    if constexpr (LEVELS == 2) {
      level_pass<K::P0, K::TW>(s_in, s_tmp, iy, ix, H, W, ly.lo, ly.n, lx.lo, lx.n, [&](int i, int j, float v) { s_l1[i * K::P1 + j] = v; });
      __syncthreads();
      level_pass<K::P1, K::T>(s_l1, s_tmp, ly, lx, H1, W1, oy0, oh, ox0, ow, store);
    } else {
      level_pass<K::P0, K::TW>(s_in, s_tmp, iy, ix, H, W, oy0, oh, ox0, ow, store);
    }
    __syncthreads();   // the next plane overwrites the patches
  }
}

// Source taps of an output coordinate: the two clamped source indices and the weight of the second.
__device__ __forceinline__ void bilinear_taps(int dst, int ratio, int L, int& i0, int& i1, float& f) {
  const float src = fmaxf(((float)dst + 0.5f) / (float)ratio - 0.5f, 0.f);   // exact: ratio is a power of two
  i0 = min((int)src, L - 1);
  i1 = min(i0 + 1, L - 1);
  f = src - (float)i0;
}
__device__ __forceinline__ float lerp(float a, float b, float f) { return __fmaf_rn(f, __fsub_rn(b, a), a); }

// y[pl, Y, X] for X in [V g, V g + V) of output row Y: the horizontal lerp in the two source rows, then the vertical one.
template <int RATIO, int V>
__global__ void __launch_bounds__(256) upsample_bilinear_kernel(const float* __restrict__ x, float* __restrict__ y, int planes, int h,
                                                                int w) {
  const int HO = RATIO * h, WO = RATIO * w, wv = WO / V;
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= HO * wv) return;
  const int Y = g / wv, X = (g - Y * wv) * V;
  int y0, y1;
  float fy;
  bilinear_taps(Y, RATIO, h, y0, y1, fy);
  // V == 4: the source columns base .. base + NC - 1 (clamped) serve the four pixels; pixel k lerps columns T0[k], T0[k] + 1
  constexpr int NC = V == 1 ? 2 : (RATIO == 4 ? 3 : 4);
  int col[NC];
  float fx1 = 0.f;
  if constexpr (V == 1) {
    bilinear_taps(X, RATIO, w, col[0], col[1], fx1);
  } else {
    const int base = X / RATIO - 1;
#pragma unroll
    for (int i = 0; i < NC; ++i) col[i] = min(max(base + i, 0), w - 1);
  }
  for (int pl = blockIdx.y; pl < planes; pl += gridDim.y) {
    const float* r0 = x + (pl * h + y0) * w;
    const float* r1 = x + (pl * h + y1) * w;
    float a[NC], b[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) a[i] = r0[col[i]], b[i] = r1[col[i]];
    const int dst = (pl * HO + Y) * WO + X;
    if constexpr (V == 1) {
      y[dst] = lerp(lerp(a[0], a[1], fx1), lerp(b[0], b[1], fx1), fy);
    } else if constexpr (RATIO == 4) {   // src = q - 3/8, q - 1/8, q + 1/8, q + 3/8 around source column q = base + 1
      float4 o;
      o.x = lerp(lerp(a[0], a[1], 0.625f), lerp(b[0], b[1], 0.625f), fy);
      o.y = lerp(lerp(a[0], a[1], 0.875f), lerp(b[0], b[1], 0.875f), fy);
      o.z = lerp(lerp(a[1], a[2], 0.125f), lerp(b[1], b[2], 0.125f), fy);
      o.w = lerp(lerp(a[1], a[2], 0.375f), lerp(b[1], b[2], 0.375f), fy);
      *reinterpret_cast<float4*>(y + dst) = o;
    } else {                             // src = m - 1/4, m + 1/4, m + 3/4, m + 5/4 around source column m = base + 1
      float4 o;
      o.x = lerp(lerp(a[0], a[1], 0.75f), lerp(b[0], b[1], 0.75f), fy);
      o.y = lerp(lerp(a[1], a[2], 0.25f), lerp(b[1], b[2], 0.25f), fy);
      o.z = lerp(lerp(a[1], a[2], 0.75f), lerp(b[1], b[2], 0.75f), fy);
      o.w = lerp(lerp(a[2], a[3], 0.25f), lerp(b[2], b[3], 0.25f), fy);
      *reinterpret_cast<float4*>(y + dst) = o;
    }
  }
}

// sum_j a_j (v[5 - j] + v[6 + j]): six pair sums, then six fused multiply-adds from j = 5 down to 0 -- twelve roundings, the same
// wherever a pixel is made.  2 sum_j a_j = 0.999999999596.
__device__ __forceinline__ float poly23(const float (&v)[12]) {
  constexpr float A[6] = {0.61066818237f, -0.145397186478f, 0.043619155884f, -0.010385513306f, 0.001615524292f, -0.000120162964f};
  float acc = 0.f;
#pragma unroll
  for (int j = 5; j >= 0; --j) acc = __fmaf_rn(A[j], __fadd_rn(v[5 - j], v[6 + j]), acc);
  return acc;
}
template <int S>
__device__ __forceinline__ float poly23_at(const float* s) {
  float v[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) v[i] = s[i * S];
  return poly23(v);
}

__device__ __forceinline__ int wrap(int i, int L) {
  const int m = i % L;
  return m < 0 ? m + L : m;
}

struct Poly23Tile {
  static constexpr int T = 64;            // edge of the output tile
  static constexpr int PM = T / 2 + 11;   // patch of the last stage: 43
  static constexpr int PI = PM / 2 + 11;  // x4: input patch under the 43 x2 samples: 32
  static constexpr int MS = 44;           // row stride of the arrays that are written or read as pairs
};

// rows [0, nr) x columns [0, nc) of the image at x, from (r0, c0) on with wrapped coordinates, into dst (row stride DS)
template <int DS>
__device__ __forceinline__ void stage_wrapped(const float* __restrict__ x, float* dst, int h, int w, int r0, int c0, int nr, int nc) {
  for (int idx = threadIdx.x; idx < nr * DS; idx += 256) {
    const int r = idx / DS, c = idx - r * DS;
    if (c < nc) dst[idx] = x[wrap(r0 + r, h) * w + wrap(c0 + c, w)];
  }
}

// One stage along the rows: src rows (nout + 1) / 2 + 11, dst rows [0, nout), both over columns [0, nc).  DS is also the
// (constant) divisor of the index decode, so nc <= DS.
template <int Q, int SS, int DS>
__device__ __forceinline__ void poly23_rows(const float* src, float* dst, int nout, int nc) {
  for (int idx = threadIdx.x; idx < (nout + 1) / 2 * DS; idx += 256) {
    const int u = idx / DS, c = idx - u * DS;
    if (c >= nc) continue;
    const float* s = src + u * SS + c;
    if (2 * u + Q < nout) dst[(2 * u + Q) * DS + c] = s[(5 + Q) * SS];
    if (2 * u + 1 - Q < nout) dst[(2 * u + 1 - Q) * DS + c] = poly23_at<SS>(s);
  }
}

// One stage with Q = 0 along the columns, LDS to LDS (the first stage of x4): src columns (nout + 1) / 2 + 11, dst columns
// [0, nout) written in pairs (dst has a column to spare when nout is odd), rows [0, nr).
template <int SS, int DS, int NU>
__device__ __forceinline__ void poly23_cols(const float* src, float* dst, int nr, int nout) {
  for (int idx = threadIdx.x; idx < nr * NU; idx += 256) {
    const int r = idx / NU, u = idx - r * NU;
    if (2 * u >= nout) continue;
    const float* s = src + r * SS + u;
    float2 o;
    o.x = s[5];
    o.y = 2 * u + 1 < nout ? poly23_at<1>(s) : 0.f;
    *reinterpret_cast<float2*>(dst + r * DS + 2 * u) = o;
  }
}

// y[pl, Y, X] of the 64 x 64 tile blockIdx.x; blockIdx.y walks the planes.  Q: the phase of the (last) stage; V: units a lane
// of the last pass makes (2: one 16-byte store, 1: two scalar stores).
template <int RATIO, int Q, int V>
__global__ void __launch_bounds__(256) upsample_poly23_kernel(const float* __restrict__ x, float* __restrict__ y, int planes, int h,
                                                              int w) {
  using K = Poly23Tile;
  static_assert(RATIO == 2 || Q == 0, "x4 ends with a phase-0 stage");
  __shared__ __attribute__((aligned(16))) float s_a[K::PM * K::MS];   // patch of the last stage
  __shared__ __attribute__((aligned(16))) float s_b[K::T * K::MS];    // its H pass
  __shared__ float s_in[RATIO == 4 ? K::PI * K::PI : 1];
  __shared__ float s_1[RATIO == 4 ? K::PM * K::PI : 1];
  const int HO = RATIO * h, WO = RATIO * w;
  const int tiles_x = (WO + K::T - 1) / K::T;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int Y0 = ty * K::T, X0 = tx * K::T;
  const int oh = min(K::T, HO - Y0), ow = min(K::T, WO - X0);   // even; multiples of 4 at x4
  const int ph = oh / 2 + 11, pw = ow / 2 + 11;                  // the last stage's patch, from (Y0 / 2 - 5 - Q, X0 / 2 - 5 - Q)
  for (int pl = blockIdx.y; pl < planes; pl += gridDim.y) {
    const float* xp = x + pl * h * w;
    if constexpr (RATIO == 4) {
      // ph, pw are odd: units 0 .. (ph - 1) / 2 of the first stage read the input from Y0 / 4 - 8 on, (ph - 1) / 2 + 11 rows
      stage_wrapped<K::PI>(xp, s_in, h, w, Y0 / 4 - 8, X0 / 4 - 8, ph / 2 + 11, pw / 2 + 11);
      __syncthreads();
      poly23_rows<0, K::PI, K::PI>(s_in, s_1, ph, pw / 2 + 11);
      __syncthreads();
      poly23_cols<K::PI, K::MS, (K::PM + 1) / 2>(s_1, s_a, ph, pw);
    } else {
      stage_wrapped<K::MS>(xp, s_a, h, w, Y0 / 2 - 5 - Q, X0 / 2 - 5 - Q, ph, pw);
    }
    __syncthreads();
    poly23_rows<Q, K::MS, K::MS>(s_a, s_b, oh, pw);
    __syncthreads();
    float* yp = y + (pl * HO + Y0) * WO + X0;
    if constexpr (V == 2) {
      constexpr int NQ = K::T / 4;
      for (int idx = threadIdx.x; idx < oh * NQ; idx += 256) {
        const int r = idx / NQ, g = idx - r * NQ;
        if (4 * g >= ow) continue;
        const float2* s = reinterpret_cast<const float2*>(s_b + r * K::MS + 2 * g);
        float v[14];
#pragma unroll
        for (int i = 0; i < 7; ++i) v[2 * i] = s[i].x, v[2 * i + 1] = s[i].y;
        const float i0 = poly23(reinterpret_cast<const float(&)[12]>(v[0])), i1 = poly23(reinterpret_cast<const float(&)[12]>(v[1]));
        const float4 o = Q ? make_float4(i0, v[6], i1, v[7]) : make_float4(v[5], i0, v[6], i1);
        *reinterpret_cast<float4*>(yp + r * WO + 4 * g) = o;
      }
    } else {
      constexpr int NU = K::T / 2;
      for (int idx = threadIdx.x; idx < oh * NU; idx += 256) {
        const int r = idx / NU, u = idx - r * NU;
        if (2 * u >= ow) continue;
        const float* s = s_b + r * K::MS + u;
        yp[r * WO + 2 * u + Q] = s[5 + Q];
        yp[r * WO + 2 * u + 1 - Q] = poly23_at<1>(s);
      }
    }
    __syncthreads();   // the next plane overwrites the patches
  }
}

template <int LEVELS>
void launch_pyr(const float* x, float* y, int planes, int H, int W, hipStream_t st) {
  constexpr int T = PyrTile<LEVELS>::T;
  int HO = (H + 1) / 2, WO = (W + 1) / 2;
  if (LEVELS == 2) HO = (HO + 1) / 2, WO = (WO + 1) / 2;
  const dim3 grid((unsigned)(((HO + T - 1) / T) * ((WO + T - 1) / T)), (unsigned)std::min(planes, 65535));
  pyr_down_kernel<LEVELS><<<grid, 256, 0, st>>>(x, y, planes, H, W);
}

template <int RATIO>
void launch_up(const float* x, float* y, int planes, int h, int w, hipStream_t st) {
  const bool vec = (RATIO * w) % 4 == 0 && tmdiff::aligned16(y);
  const long per_plane = (long)RATIO * h * (RATIO * w / (vec ? 4 : 1));
  const dim3 grid((unsigned)((per_plane + 255) / 256), (unsigned)std::min(planes, 65535));
  if (vec) upsample_bilinear_kernel<RATIO, 4><<<grid, 256, 0, st>>>(x, y, planes, h, w);
  else upsample_bilinear_kernel<RATIO, 1><<<grid, 256, 0, st>>>(x, y, planes, h, w);
}

template <int RATIO, int Q>
void launch_poly23(const float* x, float* y, int planes, int h, int w, hipStream_t st) {
  constexpr int T = Poly23Tile::T;
  const bool vec = (RATIO * w) % 4 == 0 && tmdiff::aligned16(y);
  const dim3 grid((unsigned)(((RATIO * h + T - 1) / T) * ((RATIO * w + T - 1) / T)), (unsigned)std::min(planes, 65535));
  if (vec) upsample_poly23_kernel<RATIO, Q, 2><<<grid, 256, 0, st>>>(x, y, planes, h, w);
  else upsample_poly23_kernel<RATIO, Q, 1><<<grid, 256, 0, st>>>(x, y, planes, h, w);
}

}  // namespace

extern "C" {

int tmdiff_pyr_down(const float* x, float* y, int32_t planes, int32_t H, int32_t W, int32_t levels, tmdiff_stream_t stream) {
  TMDIFF_REQUIRE(planes >= 0 && H > 0 && W > 0, "pyr_down: bad extents planes=%d H=%d W=%d", planes, H, W);
  const int least = levels == 2 ? 5 : 3;   // every level's input extent >= 3 (reflect-101 of a 5-tap filter)
  if ((levels != 1 && levels != 2) || H < least || W < least)
    return tmdiff::fail(TMDIFF_E_UNSUPPORTED, "pyr_down: levels=%d H=%d W=%d (levels 1 or 2; H, W >= 3 for one level, >= 5 for two)",
                        levels, H, W);
  if ((double)planes * H * W > 2147483647.0)
    return tmdiff::fail(TMDIFF_E_UNSUPPORTED, "pyr_down: planes=%d H=%d W=%d exceeds 32-bit element offsets (planes * H * W <= 2^31 - 1)",
                        planes, H, W);
  if (planes == 0) return TMDIFF_OK;
  TMDIFF_REQUIRE(x && y, "pyr_down: null tensor");
  if (levels == 2) launch_pyr<2>(x, y, planes, H, W, tmdiff::as_stream(stream));
  else launch_pyr<1>(x, y, planes, H, W, tmdiff::as_stream(stream));
  return tmdiff::check_launch("pyr_down");
}

int tmdiff_upsample_bilinear(const float* x, float* y, int32_t planes, int32_t h, int32_t w, int32_t ratio, tmdiff_stream_t stream) {
  TMDIFF_REQUIRE(planes >= 0 && h > 0 && w > 0, "upsample_bilinear: bad extents planes=%d h=%d w=%d", planes, h, w);
  if (ratio != 2 && ratio != 4) return tmdiff::fail(TMDIFF_E_UNSUPPORTED, "upsample_bilinear: ratio=%d (2 or 4)", ratio);
  if ((double)planes * h * w * ratio * ratio > 2147483647.0)
    return tmdiff::fail(TMDIFF_E_UNSUPPORTED,
                        "upsample_bilinear: planes=%d h=%d w=%d ratio=%d exceeds 32-bit element offsets (planes * ratio^2 * h * w <= 2^31 - 1)",
                        planes, h, w, ratio);
  if (planes == 0) return TMDIFF_OK;
  TMDIFF_REQUIRE(x && y, "upsample_bilinear: null tensor");
  if (ratio == 4) launch_up<4>(x, y, planes, h, w, tmdiff::as_stream(stream));
  else launch_up<2>(x, y, planes, h, w, tmdiff::as_stream(stream));
  return tmdiff::check_launch("upsample_bilinear");
}

int tmdiff_upsample_poly23(const float* x, float* y, int32_t planes, int32_t h, int32_t w, int32_t ratio, int32_t phase,
                           tmdiff_stream_t stream) {
  const char* limits = "ratio 2 or 4; phase 0 or 1, 1 at ratio 4; planes >= 0, h, w >= 1; planes * ratio^2 * h * w <= 2^31 - 1";
  if ((ratio != 2 && ratio != 4) || (phase != 0 && phase != 1) || (ratio == 4 && phase != 1))
    return tmdiff::fail(TMDIFF_E_UNSUPPORTED, "upsample_poly23: ratio=%d phase=%d (%s)", ratio, phase, limits);
  if (planes < 0 || h <= 0 || w <= 0)
    return tmdiff::fail(TMDIFF_E_UNSUPPORTED, "upsample_poly23: bad extents planes=%d h=%d w=%d (%s)", planes, h, w, limits);
  if ((double)planes * h * w * ratio * ratio > 2147483647.0)
    return tmdiff::fail(TMDIFF_E_UNSUPPORTED, "upsample_poly23: planes=%d h=%d w=%d ratio=%d exceeds 32-bit element offsets (%s)",
                        planes, h, w, ratio, limits);
  if (planes == 0) return TMDIFF_OK;
  TMDIFF_REQUIRE(x && y, "upsample_poly23: null tensor");
  if (ratio == 4) launch_poly23<4, 0>(x, y, planes, h, w, tmdiff::as_stream(stream));
  else if (phase == 1) launch_poly23<2, 1>(x, y, planes, h, w, tmdiff::as_stream(stream));
  else launch_poly23<2, 0>(x, y, planes, h, w, tmdiff::as_stream(stream));
  return tmdiff::check_launch("upsample_poly23");
}

}  // extern "C"
