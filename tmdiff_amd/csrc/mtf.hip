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

// y[pl, oy0 + i, ox0 + j] of the 16 x 16 tile blockIdx.x; blockIdx.y walks the planes.  KC: K at compile time, 0 = kr.
template <int R, int KC>
__global__ void __launch_bounds__(256) fir_decimate_kernel(const float* __restrict__ x, const float* __restrict__ taps,
                                                           float* __restrict__ y, int planes, int period, int H, int W, int kr, int off_y,
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
  for (int pl = blockIdx.y; pl < planes; pl += gridDim.y) {
    const float* xp = x + pl * H * W;
    for (int idx = threadIdx.x; idx < nr * P::PC; idx += 256) {
      const int r = idx / P::PC, c = idx - r * P::PC;
      if (c >= nc) continue;
      const int gy = min(max(gy0 + r, 0), H - 1), gx = min(max(gx0 + c, 0), W - 1);
      s[r * P::RS + (c % R) * P::PW + c / R] = xp[gy * W + gx];
    }
    __syncthreads();
    if (live) {
      const float* tp = taps + (pl % period) * K * K;
      const float* sp = s + R * i * P::RS + j;
      float acc = 0.f;
      for (int u = 0; u < K; ++u) {
#pragma unroll
        for (int v = 0; v < K; ++v) acc = __fmaf_rn(tp[u * K + v], sp[u * P::RS + (v % R) * P::PW + v / R], acc);
      }
      y[(pl * HO + oy0 + i) * WO + ox0 + j] = acc;
    }
    __syncthreads();   // the next plane overwrites the patch
  }
}

template <int R>
void launch_fir(const float* x, const float* taps, float* y, int planes, int period, int H, int W, int K, int off_y, int off_x,
                hipStream_t st) {
  constexpr int T = FirPatch<R>::T;
  const int HO = (H - off_y + R - 1) / R, WO = (W - off_x + R - 1) / R;
  const dim3 grid((unsigned)(((HO + T - 1) / T) * ((WO + T - 1) / T)), (unsigned)std::min(planes, 65535));
  if (K == 41) fir_decimate_kernel<R, 41><<<grid, 256, 0, st>>>(x, taps, y, planes, period, H, W, K, off_y, off_x);
  else fir_decimate_kernel<R, 0><<<grid, 256, 0, st>>>(x, taps, y, planes, period, H, W, K, off_y, off_x);
}

}  // namespace

extern "C" {

int tmdiff_fir_decimate(const float* x, const float* taps, float* y, int32_t planes, int32_t taps_period, int32_t H, int32_t W,
                        int32_t K, int32_t ratio, int32_t off_y, int32_t off_x, tmdiff_stream_t stream) {
  const char* limits = "K odd, 1 <= K <= 41; ratio 1, 2 or 4; 0 <= off_y, off_x < ratio; H, W >= 1; planes >= 0; taps_period >= 1 and "
                       "a divisor of planes; planes * H * W <= 2^31 - 1";
  if (K < 1 || K > 41 || K % 2 == 0) return tmdiff::fail(TMDIFF_E_UNSUPPORTED, "fir_decimate: K=%d (%s)", K, limits);
  if (ratio != 1 && ratio != 2 && ratio != 4) return tmdiff::fail(TMDIFF_E_UNSUPPORTED, "fir_decimate: ratio=%d (%s)", ratio, limits);
  if (off_y < 0 || off_y >= ratio || off_x < 0 || off_x >= ratio)
    return tmdiff::fail(TMDIFF_E_UNSUPPORTED, "fir_decimate: offset off_y=%d off_x=%d at ratio=%d (%s)", off_y, off_x, ratio, limits);
  if (H < 1 || W < 1 || planes < 0)
    return tmdiff::fail(TMDIFF_E_UNSUPPORTED, "fir_decimate: bad extents planes=%d H=%d W=%d (%s)", planes, H, W, limits);
  if (taps_period < 1 || planes % taps_period)
    return tmdiff::fail(TMDIFF_E_UNSUPPORTED, "fir_decimate: taps_period=%d with planes=%d (%s)", taps_period, planes, limits);
  if ((double)planes * H * W > 2147483647.0)
    return tmdiff::fail(TMDIFF_E_UNSUPPORTED, "fir_decimate: planes=%d H=%d W=%d exceeds 32-bit element offsets (%s)", planes, H, W,
                        limits);
  if (planes == 0 || H <= off_y || W <= off_x) return TMDIFF_OK;   // no plane, or no sample at o + ratio * i inside the image
  TMDIFF_REQUIRE(x && taps && y, "fir_decimate: null tensor");
  const hipStream_t st = tmdiff::as_stream(stream);
  if (ratio == 4) launch_fir<4>(x, taps, y, planes, taps_period, H, W, K, off_y, off_x, st);
  else if (ratio == 2) launch_fir<2>(x, taps, y, planes, taps_period, H, W, K, off_y, off_x, st);
  else launch_fir<1>(x, taps, y, planes, taps_period, H, W, K, off_y, off_x, st);
  return tmdiff::check_launch("fir_decimate");
}

}  // extern "C"
