// FIR filtering with decimation on gfx950: the primitive of Wald's protocol (low-pass every band with a filter matched to the
// sensor's MTF, keep every ratio-th sample) and of everything else that is built from an MTF-matched filter.  Host definition:
// tmdiff_amd/metrics.py, fir_decimate.  Dense fp32 planes [planes, H, W] with 32-bit element offsets, plain vector loads and
// stores, no atomics; nothing is allocated or read back, so a call can be captured into a graph.
//
//   y[p, i, j] = sum_{u, v} taps[p % T, u, v] * x[p, clamp(ratio i + oy - R + u, 0, H - 1), clamp(ratio j + ox - R + v, 0, W - 1)]
//
// a correlation (no flip) with a K x K table per band, R = (K - 1) / 2, K odd and at most 41, ratio 1, 2 or 4, the border
// replicated (imfilter(..., 'replicate')), the output extent ceil((L - o) / ratio) per axis (MATLAB's o + 1 : ratio : end).  The
// tap table holds T bands and repeats over the planes, T dividing their count.  Arbitrary taps: no symmetry is assumed.
//
// Only the kept samples are computed: K^2 / ratio^2 multiply-adds per input pixel, 105 at 41 x 41 and x4.
//
// SUMMATION ORDER of an output pixel, the same wherever it is made: acc = 0, then the taps in row-major order, u = 0 .. K - 1
// outermost and v = 0 .. K - 1 inside, one fused multiply-add each, acc = fma(taps[u][v], x[..], acc): K^2 roundings.  It does
// not depend on the tile, the grid, the plane loop, the ratio or on which instantiation runs (K = 41 is compiled with the row
// loop unrolled, every other K with run-time loops over the same order), so the ratio-4 result at offset (2, 2) is the ratio-1
// result at [2::4, 2::4] bit for bit.
//
// A 256-lane workgroup owns a 16 x 16 tile of the OUTPUT, one pixel per lane, and stages the clamped input patch of
// 15 ratio + K rows and columns in LDS.  Coordinates are clamped while staging and nowhere else.  Lanes of an output row read
// input columns `ratio` apart, which as plain rows would be a ratio-way bank conflict on ds_read_b32; so a patch row is stored
// SPLIT BY COLUMN PHASE: column c sits at (c % ratio) * PW + c / ratio, and lane j reads tap v at (v % ratio) * PW + j + v / ratio
// -- consecutive lanes, consecutive dwords.  A ds_read_b32 serves 32 lanes = two output rows, `ratio` patch rows apart; the row
// stride RS is chosen with ratio * RS = 16 (mod 32), so the second row's sixteen lanes take the other sixteen banks:
//   ratio 4: patch 101 x 101, PW 27, RS 108 -> 43632 bytes of LDS, 3 workgroups per CU (160 KiB)
//   ratio 2: patch  71 x  71, PW 36, RS  72 -> 20448 bytes         ratio 1: patch 56 x 56, RS 80 -> 17920 bytes
// The taps are the same for every lane of a workgroup: they are read through a wave-uniform address (scalar loads into SGPRs,
// straight into the multiply-add's scalar operand) and never enter the vector path.  One LDS read per multiply-add remains: the
// kernel is bound by the LDS read rate (profiles/mtf_degrade.txt).
//
// THE FILTER BANK, tmdiff_fir_decimate_bank: y[b, t] = fir_decimate(x[b], taps[t]) for ONE plane per image and T tables (the PAN
// seen through every MS band's filter, metrics.pan_lowpass_bands).  The same kernel body: the workgroup stages the clamped
// patch of x[b] once and walks the T tables over it, so the input is read once instead of T times and no T-fold copy of it
// exists.  Tile, patch layout, scalar tap loads and the summation order of an output pixel are the ones above: y[b, t] equals
// tmdiff_fir_decimate on the expanded copy bit for bit.
//
// THE ADJOINT, tmdiff_fir_decimate_adjoint: dx = beta * base + alpha * A^T g for the operator A above (host definition:
// metrics.fir_decimate_adjoint), the clamp included -- a border pixel collects every position that the replicated border
// mapped onto it:
//
//   (A^T g)[p, y, x] = sum over (i, u, j, v) with clamp(ratio i + oy - R + u, 0, H - 1) == y and
//                      clamp(ratio j + ox - R + v, 0, W - 1) == x   of   taps[p % T, u, v] * g[p, i, j]
//
// A gather: every dx pixel is made by one lane, no atomics, so the same bits come out of every run and of a graph replay.
//
// SUMMATION ORDER of a dx pixel, the same wherever it is made: acc = 0, then the terms of the sum above in lexicographic
// order of (i, u, j, v) -- i outermost, v innermost, each ascending -- one fused multiply-add each,
// acc = fma(taps[u][v], g[i][j], acc).  Away from the border a pixel has one u per i and one v per j: the g samples in
// row-major order, with the tap that reaches the pixel from each.  It does not depend on the tile, the grid, the plane loop or
// the ratio's instantiation (K is a run-time value in all three).  The kernel also walks positions (i, j) outside g, staged as zeros, and fma(t, 0, acc) == acc for every
// finite tap t (acc starts at +0 and a sum that starts there never becomes -0): those steps change no bit.  The epilogue is
// r = alpha * acc rounded once, then, when beta != 0, fma(beta, base, r); beta == 0 never reads base.
//
// A 256-lane workgroup owns 16 x 16 BLOCKS of ratio x ratio dx pixels (64 x 64 pixels at x4), a block -- every phase of the
// decimation -- per lane.  For a block row b and a g row i = b - d the pixel rows of the block take the taps
// u = ratio d + a + (R - oy), a = 0 .. ratio - 1: the same d, and so the same taps, for every lane.  The taps stay wave-uniform
// scalar loads that feed the multiply-add's scalar operand, and ONE ds_read_b32 of a g sample feeds ratio^2 multiply-adds (the
// forward: one).  The loop runs d and e (columns) downwards, which is i and j upwards.  Steps whose ratio x ratio taps all lie
// inside the table take a path without checks; the one or two d (e) at either end check each tap, uniformly.  The g patch of
// a tile is 16 + (K + ratio - 2) / ratio rows and columns (26 at x4 and K = 41), with a row stride of 16 (mod 32) dwords so that
// the two block rows a ds_read_b32 serves take disjoint banks.  A row of a block is one 16-byte store at x4 (8 at x2) when the
// row length and the pointers allow it, single dwords otherwise, with the same values.
//
// THE FOLDED BORDER lives in a path that interior tiles do not enter.  A tile that touches the image border stages the band's
// taps in LDS as well, and up to 4 x 16 ratio lanes each sum one border pixel of the tile in the order above, from the g patch
// (it holds every sample such a pixel needs: rows i <= (R - oy) / ratio for y = 0 lie below the patch's last row
// b0 + 15 - dmin, rows i >= (H - 1 - oy - R) / ratio for y = H - 1 above its first, b0 - dmax).  The sums go through LDS to the
// lanes that own the pixels, which store them with the rest of their block.
#include <algorithm>

#include "common.h"

namespace {

template <int R>
struct FirPatch {
  static constexpr int T = 16;                                   // edge of the output tile
  static constexpr int KMAX = 41;
  static constexpr int PC = (T - 1) * R + KMAX;                  // rows and columns of the patch at K = 41
  static constexpr int PW = R == 4 ? 27 : (R == 2 ? 36 : 80);    // columns of one phase (>= ceil(PC / R))
  static constexpr int RS = R * PW;                              // row stride: R * RS = 16 (mod 32)
  static_assert(PW * R >= PC && (R * RS) % 32 == 16, "patch layout");
};

// y[pl, oy0 + i, ox0 + j] of the 16 x 16 tile blockIdx.x; blockIdx.y walks the staged planes.  KC: K at compile time, 0 = kr.
// One body serves the two entry points; what differs is which output planes a staged input plane q feeds and with which table:
//   BANK = false (fir_decimate):       `groups` = planes; plane q makes y[q] with table q % period
//   BANK = true  (fir_decimate_bank):  `groups` = images; plane q makes y[q * period + t] with table t, t = 0 .. period - 1,
//                                      from ONE staging of the patch
template <bool BANK> __device__ __forceinline__ int fir_tables(int period) { return BANK ? period : 1; }
template <bool BANK> __device__ __forceinline__ int fir_table(int q, int t, int period) { return BANK ? t : q % period; }
template <bool BANK> __device__ __forceinline__ int fir_out_plane(int q, int t, int period) { return BANK ? q * period + t : q; }

template <int R, int KC, bool BANK>
__global__ void __launch_bounds__(256) fir_decimate_kernel(const float* __restrict__ x, const float* __restrict__ taps,
                                                           float* __restrict__ y, int groups, int period, int H, int W, int kr, int off_y,
                                                           int off_x) {
  using P = FirPatch<R>;
  __shared__ float s[P::PC * P::RS];
  const int K = KC ? KC : kr, rad = K / 2;
  const int HO = (H - off_y + R - 1) / R, WO = (W - off_x + R - 1) / R;
  const int tiles_x = (WO + P::T - 1) / P::T;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int oy0 = ty * P::T, ox0 = tx * P::T;
  const int oh = min(P::T, HO - oy0), ow = min(P::T, WO - ox0);
  const int nr = (oh - 1) * R + K, nc = (ow - 1) * R + K;              // the patch of the tile's valid outputs
  const int gy0 = R * oy0 + off_y - rad, gx0 = R * ox0 + off_x - rad;  // its first row and column in the image
  const int i = threadIdx.x >> 4, j = threadIdx.x & 15;
  const bool live = i < oh && j < ow;
  for (int q = blockIdx.y; q < groups; q += gridDim.y) {
    const float* xp = x + q * H * W;
    for (int idx = threadIdx.x; idx < nr * P::PC; idx += 256) {
      const int r = idx / P::PC, c = idx - r * P::PC;
      if (c >= nc) continue;
      const int gy = min(max(gy0 + r, 0), H - 1), gx = min(max(gx0 + c, 0), W - 1);
      s[r * P::RS + (c % R) * P::PW + c / R] = xp[gy * W + gx];
    }
    __syncthreads();
    if (live) {
      const float* sp = s + R * i * P::RS + j;
      for (int t = 0; t < fir_tables<BANK>(period); ++t) {
        const float* tp = taps + fir_table<BANK>(q, t, period) * K * K;
        float acc = 0.f;
        for (int u = 0; u < K; ++u) {
#pragma unroll
          for (int v = 0; v < K; ++v) acc = __fmaf_rn(tp[u * K + v], sp[u * P::RS + (v % R) * P::PW + v / R], acc);
        }
        y[(fir_out_plane<BANK>(q, t, period) * HO + oy0 + i) * WO + ox0 + j] = acc;
      }
    }
    __syncthreads();   // the next plane overwrites the patch
  }
}

template <int R, bool BANK>
void launch_fir(const float* x, const float* taps, float* y, int groups, int period, int H, int W, int K, int off_y, int off_x,
                hipStream_t st) {
  constexpr int T = FirPatch<R>::T;
  const int HO = (H - off_y + R - 1) / R, WO = (W - off_x + R - 1) / R;
  const dim3 grid((unsigned)(((HO + T - 1) / T) * ((WO + T - 1) / T)), (unsigned)std::min(groups, 65535));
  if (K == 41) fir_decimate_kernel<R, 41, BANK><<<grid, 256, 0, st>>>(x, taps, y, groups, period, H, W, K, off_y, off_x);
  else fir_decimate_kernel<R, 0, BANK><<<grid, 256, 0, st>>>(x, taps, y, groups, period, H, W, K, off_y, off_x);
}

template <bool BANK>
void launch_fir_ratio(const float* x, const float* taps, float* y, int groups, int period, int H, int W, int K, int ratio, int off_y,
                      int off_x, hipStream_t st) {
  if (ratio == 4) launch_fir<4, BANK>(x, taps, y, groups, period, H, W, K, off_y, off_x, st);
  else if (ratio == 2) launch_fir<2, BANK>(x, taps, y, groups, period, H, W, K, off_y, off_x, st);
  else launch_fir<1, BANK>(x, taps, y, groups, period, H, W, K, off_y, off_x, st);
}

template <int R>
struct AdjPatch {
  static constexpr int B = 16;                                   // blocks of R x R dx pixels along an edge of the tile
  static constexpr int TS = B * R;                               // pixels along an edge of the tile
  static constexpr int KMAX = 41;
  static constexpr int ND = (KMAX + R - 2) / R + 1;              // most values of d (of e) that reach a block
  static constexpr int PR = B + ND - 1;                          // rows and columns of the g patch at K = 41
  static constexpr int PS = PR <= 48 ? 48 : 80;                  // row stride: 16 (mod 32)
  static_assert(PS >= PR && PS % 32 == 16 && 4 * TS <= 256, "patch layout");
};

template <int R> struct FirVec { using type = float; };
template <> struct FirVec<2> { using type = float2; };
template <> struct FirVec<4> { using type = float4; };

// The u (or v) of the terms that row (column) `pos` of an image of `len` rows collects from sample i, whose tap 0 sits at p0.
__device__ __forceinline__ void fir_fold_range(int pos, int len, int p0, int K, int& lo, int& hi) {
  lo = hi = pos - p0;
  if (pos == 0) lo = 0;                  // every position <= 0 was clamped onto row 0
  if (pos == len - 1) hi = K - 1;        // every position >= len - 1 onto the last row
  lo = max(lo, 0);
  hi = min(hi, K - 1);
}

// dx[pl] of the tile blockIdx.x, 16 x 16 blocks of R x R pixels; blockIdx.y walks the planes.  K is a run-time value: no loop
// here gains from unrolling over it.
// base may alias dx: a lane reads base where it then writes dx and nowhere else.
template <int R>
__global__ void __launch_bounds__(256) fir_adjoint_kernel(const float* __restrict__ g, const float* __restrict__ taps, const float* base,
                                                          float* dx, float alpha, float beta, int planes, int period, int H, int W,
                                                          int K, int off_y, int off_x, int vec) {
  using P = AdjPatch<R>;
  using V = typename FirVec<R>::type;
  __shared__ float s[P::PR * P::PS];
  __shared__ float st[P::KMAX * P::KMAX];   // border tiles: the band's taps
  __shared__ float se[4 * P::TS];           // border tiles: the sums of the tile's border pixels
  const int rad = K / 2;
  const int HO = (H - off_y + R - 1) / R, WO = (W - off_x + R - 1) / R;
  const int cy = rad - off_y, cx = rad - off_x;                            // u = R d + a + cy, v = R e + a + cx
  const int dmax = (K - 1 - cy) / R, dmin = -((cy + R - 1) / R);           // the d with a tap inside the table for some a
  const int emax = (K - 1 - cx) / R, emin = -((cx + R - 1) / R);
  const int tiles_x = ((W + R - 1) / R + P::B - 1) / P::B;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int i0 = ty * P::B - dmax, j0 = tx * P::B - emax;                  // the g sample at the patch's origin
  const int nr = P::B + dmax - dmin, nc = P::B + emax - emin;              // rows and columns of the patch
  const int ylo = ty * P::TS, yhi = min(ylo + P::TS, H) - 1, xlo = tx * P::TS, xhi = min(xlo + P::TS, W) - 1;
  const bool border = ylo == 0 || yhi == H - 1 || xlo == 0 || xhi == W - 1;
  const int ly = threadIdx.x >> 4, lx = threadIdx.x & 15;
  const int y0 = ylo + R * ly, x0 = xlo + R * lx;
  for (int pl = blockIdx.y; pl < planes; pl += gridDim.y) {
    const float* gp = g + pl * HO * WO;
    const float* tp = taps + (pl % period) * K * K;
    for (int idx = threadIdx.x; idx < nr * nc; idx += 256) {
      const int r = idx / nc, c = idx - r * nc;
      const int i = i0 + r, j = j0 + c;
      s[r * P::PS + c] = (i >= 0 && i < HO && j >= 0 && j < WO) ? gp[i * WO + j] : 0.f;
    }
    if (border)
      for (int idx = threadIdx.x; idx < K * K; idx += 256) st[idx] = tp[idx];
    __syncthreads();
    float acc[R][R];
#pragma unroll
    for (int a = 0; a < R; ++a)
#pragma unroll
      for (int c = 0; c < R; ++c) acc[a][c] = 0.f;
    const float* sp = s + ly * P::PS + lx;
    for (int dd = 0; dd <= dmax - dmin; ++dd) {                 // d = dmax - dd: the g rows upwards
      const int ub = R * (dmax - dd) + cy;
      const bool rows_in = ub >= 0 && ub + R <= K;
      for (int ee = 0; ee <= emax - emin; ++ee) {
        const int vb = R * (emax - ee) + cx;
        const float gv = sp[dd * P::PS + ee];
        const float* t = tp + ub * K + vb;
        if (rows_in && vb >= 0 && vb + R <= K) {
#pragma unroll
          for (int a = 0; a < R; ++a)
#pragma unroll
            for (int c = 0; c < R; ++c) acc[a][c] = __fmaf_rn(t[a * K + c], gv, acc[a][c]);
        } else {
#pragma unroll
          for (int a = 0; a < R; ++a)
#pragma unroll
            for (int c = 0; c < R; ++c)
              if ((unsigned)(ub + a) < (unsigned)K && (unsigned)(vb + c) < (unsigned)K) acc[a][c] = __fmaf_rn(t[a * K + c], gv, acc[a][c]);
        }
      }
    }
    if (border) {                                               // uniform: interior tiles skip all of it
      const int seg = threadIdx.x / P::TS, k = threadIdx.x - seg * P::TS;
      int y = ylo + k, x = xlo + k;
      bool have = false;
      if (seg == 0) { y = 0; have = ylo == 0 && x <= xhi; }
      else if (seg == 1) { y = H - 1; have = yhi == H - 1 && H > 1 && x <= xhi; }
      else if (seg == 2) { x = 0; have = xlo == 0 && y <= yhi && y != 0 && y != H - 1; }
      else if (seg == 3) { x = W - 1; have = xhi == W - 1 && W > 1 && y <= yhi && y != 0 && y != H - 1; }
      if (have) {
        const int ia = max(i0, 0), ib = min(i0 + nr, HO) - 1, ja = max(j0, 0), jb = min(j0 + nc, WO) - 1;
        float e = 0.f;
        for (int i = ia; i <= ib; ++i) {
          int ulo, uhi;
          fir_fold_range(y, H, R * i + off_y - rad, K, ulo, uhi);
          for (int u = ulo; u <= uhi; ++u)
            for (int j = ja; j <= jb; ++j) {
              int vlo, vhi;
              fir_fold_range(x, W, R * j + off_x - rad, K, vlo, vhi);
              const float gv = s[(i - i0) * P::PS + j - j0];
              const float* tr = st + u * K;
              int v = vlo;
              for (; v + 3 <= vhi; v += 4) {                    // four taps in flight ahead of the chain; the order stays
                const float t0 = tr[v], t1 = tr[v + 1], t2 = tr[v + 2], t3 = tr[v + 3];
                e = __fmaf_rn(t0, gv, e);
                e = __fmaf_rn(t1, gv, e);
                e = __fmaf_rn(t2, gv, e);
                e = __fmaf_rn(t3, gv, e);
              }
              for (; v <= vhi; ++v) e = __fmaf_rn(tr[v], gv, e);
            }
        }
        se[threadIdx.x] = e;
      }
      __syncthreads();
    }
    if (y0 < H && x0 < W) {
#pragma unroll
      for (int a = 0; a < R; ++a) {
        const int y = y0 + a;
        if (y >= H) break;
        if (border) {
#pragma unroll
          for (int c = 0; c < R; ++c) {
            const int x = x0 + c;
            if (x < W && (y == 0 || y == H - 1 || x == 0 || x == W - 1))
              acc[a][c] = se[y == 0 ? x - xlo : (y == H - 1 ? P::TS + x - xlo : (x == 0 ? 2 * P::TS + y - ylo : 3 * P::TS + y - ylo))];
          }
        }
        const int o = (pl * H + y) * W + x0;
        float r[R], b[R];
        if (vec) {                                              // W is a multiple of R here: the row of the block is whole
          if (beta != 0.f) *reinterpret_cast<V*>(b) = *reinterpret_cast<const V*>(base + o);
#pragma unroll
          for (int c = 0; c < R; ++c) {
            r[c] = __fmul_rn(alpha, acc[a][c]);
            if (beta != 0.f) r[c] = __fmaf_rn(beta, b[c], r[c]);
          }
          *reinterpret_cast<V*>(dx + o) = *reinterpret_cast<const V*>(r);
        } else {
#pragma unroll
          for (int c = 0; c < R; ++c) {
            if (x0 + c >= W) break;
            r[c] = __fmul_rn(alpha, acc[a][c]);
            if (beta != 0.f) r[c] = __fmaf_rn(beta, base[o + c], r[c]);
            dx[o + c] = r[c];
          }
        }
      }
    }
    __syncthreads();   // the next plane overwrites the patch, the taps and the border sums
  }
}

template <int R>
void launch_fir_adjoint(const float* g, const float* taps, const float* base, float* dx, float alpha, float beta, int planes, int period,
                        int H, int W, int K, int off_y, int off_x, hipStream_t st) {
  constexpr int TS = AdjPatch<R>::TS;
  const dim3 grid((unsigned)(((H + TS - 1) / TS) * ((W + TS - 1) / TS)), (unsigned)std::min(planes, 65535));
  const uintptr_t align = reinterpret_cast<uintptr_t>(dx) | (beta != 0.f ? reinterpret_cast<uintptr_t>(base) : 0);
  const int vec = R > 1 && W % R == 0 && align % (4 * R) == 0;
  fir_adjoint_kernel<R><<<grid, 256, 0, st>>>(g, taps, base, dx, alpha, beta, planes, period, H, W, K, off_y, off_x, vec);
}

// The limits of both entry points, checked in the header's order; TMDIFF_OK when the extents are taken.
int fir_limits(const char* name, int K, int ratio, int off_y, int off_x, int H, int W, int planes, int taps_period) {
  const char* limits = "K odd, 1 <= K <= 41; ratio 1, 2 or 4; 0 <= off_y, off_x < ratio; H, W >= 1; planes >= 0; taps_period >= 1 and "
                       "a divisor of planes; planes * H * W <= 2^31 - 1";
  if (K < 1 || K > 41 || K % 2 == 0) return tmdiff::fail(TMDIFF_E_UNSUPPORTED, "%s: K=%d (%s)", name, K, limits);
  if (ratio != 1 && ratio != 2 && ratio != 4) return tmdiff::fail(TMDIFF_E_UNSUPPORTED, "%s: ratio=%d (%s)", name, ratio, limits);
  if (off_y < 0 || off_y >= ratio || off_x < 0 || off_x >= ratio)
    return tmdiff::fail(TMDIFF_E_UNSUPPORTED, "%s: offset off_y=%d off_x=%d at ratio=%d (%s)", name, off_y, off_x, ratio, limits);
  if (H < 1 || W < 1 || planes < 0)
    return tmdiff::fail(TMDIFF_E_UNSUPPORTED, "%s: bad extents planes=%d H=%d W=%d (%s)", name, planes, H, W, limits);
  if (taps_period < 1 || planes % taps_period)
    return tmdiff::fail(TMDIFF_E_UNSUPPORTED, "%s: taps_period=%d with planes=%d (%s)", name, taps_period, planes, limits);
  if ((double)planes * H * W > 2147483647.0)
    return tmdiff::fail(TMDIFF_E_UNSUPPORTED, "%s: planes=%d H=%d W=%d exceeds 32-bit element offsets (%s)", name, planes, H, W, limits);
  return TMDIFF_OK;
}

}  // namespace

extern "C" {

int tmdiff_fir_decimate(const float* x, const float* taps, float* y, int32_t planes, int32_t taps_period, int32_t H, int32_t W,
                        int32_t K, int32_t ratio, int32_t off_y, int32_t off_x, tmdiff_stream_t stream) {
  if (const int rc = fir_limits("fir_decimate", K, ratio, off_y, off_x, H, W, planes, taps_period)) return rc;
  if (planes == 0 || H <= off_y || W <= off_x) return TMDIFF_OK;   // no plane, or no sample at o + ratio * i inside the image
  TMDIFF_REQUIRE(x && taps && y, "fir_decimate: null tensor");
  launch_fir_ratio<false>(x, taps, y, planes, taps_period, H, W, K, ratio, off_y, off_x, tmdiff::as_stream(stream));
  return tmdiff::check_launch("fir_decimate");
}

int tmdiff_fir_decimate_bank(const float* x, const float* taps, float* y, int32_t images, int32_t tables, int32_t H, int32_t W,
                             int32_t K, int32_t ratio, int32_t off_y, int32_t off_x, tmdiff_stream_t stream) {
  if (images < 0 || tables < 1 || (double)images * tables > 2147483647.0)
    return tmdiff::fail(TMDIFF_E_UNSUPPORTED, "fir_decimate_bank: images=%d tables=%d (images >= 0, tables >= 1, and the limits of "
                        "fir_decimate on images * tables planes)", images, tables);
  // the output [images, tables] has the most planes: its element count bounds the input's
  if (const int rc = fir_limits("fir_decimate_bank", K, ratio, off_y, off_x, H, W, images * tables, tables)) return rc;
  if (images == 0 || H <= off_y || W <= off_x) return TMDIFF_OK;
  TMDIFF_REQUIRE(x && taps && y, "fir_decimate_bank: null tensor");
  launch_fir_ratio<true>(x, taps, y, images, tables, H, W, K, ratio, off_y, off_x, tmdiff::as_stream(stream));
  return tmdiff::check_launch("fir_decimate_bank");
}

int tmdiff_fir_decimate_adjoint(const float* g, const float* taps, const float* base, float* dx, float alpha, float beta, int32_t planes,
                                int32_t taps_period, int32_t H, int32_t W, int32_t K, int32_t ratio, int32_t off_y, int32_t off_x,
                                tmdiff_stream_t stream) {
  if (const int rc = fir_limits("fir_decimate_adjoint", K, ratio, off_y, off_x, H, W, planes, taps_period)) return rc;
  if (planes == 0) return TMDIFF_OK;
  TMDIFF_REQUIRE(taps && dx && (base || beta == 0.f), "fir_decimate_adjoint: null tensor");
  TMDIFF_REQUIRE(g || H <= off_y || W <= off_x, "fir_decimate_adjoint: null tensor");   // an operator without samples has no g
  const hipStream_t st = tmdiff::as_stream(stream);
  if (ratio == 4) launch_fir_adjoint<4>(g, taps, base, dx, alpha, beta, planes, taps_period, H, W, K, off_y, off_x, st);
  else if (ratio == 2) launch_fir_adjoint<2>(g, taps, base, dx, alpha, beta, planes, taps_period, H, W, K, off_y, off_x, st);
  else launch_fir_adjoint<1>(g, taps, base, dx, alpha, beta, planes, taps_period, H, W, K, off_y, off_x, st);
  return tmdiff::check_launch("fir_decimate_adjoint");
}

}  // extern "C"
