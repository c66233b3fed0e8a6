// A-trous wavelet pansharpening on gfx950 (host definitions: tmdiff_amd/metrics.py, atrous_lowpass / awlp_inject / awlp): the
// approximation plane of the undecimated "a trous" transform with the B3-spline filter, and the ATWT / AWLP injection.  Nothing is
// read on the host, nothing is allocated, no atomics: the same bits on every run and in a graph replay; a batch equals its samples.
//
//  THE TRANSFORM         c_0 = x, c_l = h_l * c_{l-1}; h_l is the separable (1, 4, 6, 4, 1) / 16 with its taps at the offsets
//                        -2d, -d, 0, d, 2d, d = 2^(l-1).  An index outside the plane is clamped into it at EVERY level: level l
//                        reads c_{l-1} at clamped coordinates.  Along W first,
//                          r = ((((t_0 v_0 + t_1 v_1) + t_2 v_2) + t_3 v_3) + t_4 v_4)
//                        in fp64 with every product and every sum rounded on its own (contraction is off; the products of the
//                        row pass are exact anyway, the taps having at most two significant bits), then the same along H on r,
//                        which stays in fp64.  A level's output is rounded to fp32 once, where it is stored for the next level.
//  atrous_lowpass_kernel one workgroup of 256 per 32 x 32 tile of one plane (grid.y walks the B * C planes), all LEVELS levels in
//                        one launch.  (A launch may also start at a later level, FIRST > 1: every dilation and halo below is
//                        then 2^(FIRST-1) times as large.  That is how single levels are chained.)  With R_l = 2 (2^LEVELS - 2^l) -- the halo still needed after level l: 14, 12, 8, 0 at three
//                        levels -- the tile and R_0 pixels around it are staged in LDS (f, fp32); level l then forms its row pass
//                        on the rows of the R_{l-1} region and the columns of the R_l region into r (fp64), and its column pass
//                        on the R_l region, which goes back into f, or from the last level to `out`.  ONLY cells inside the plane
//                        are staged or computed, and every read clamps its global coordinate first and turns it into an LDS
//                        index afterwards.  A clamped coordinate lies between the cell and the tile, so it is inside the region
//                        that the level before computed: the result equals LEVELS single-level launches bit for bit, also where a
//                        tile touches the border and where H or W is smaller than the halo.
//                        LDS: 12 (32 + 2 R_0)^2 bytes: 15,552 / 23,232 / 43,200 at one / two / three levels.
//                        HBM traffic: the plane in and out once; the halo is read again by the neighbours, mostly from L2.
//  ALIASING              x is read with a halo that another workgroup owns: `out` must not overlap x.  The entry point refuses it.
//  awlp_inject_kernel    a lane owns four consecutive pixels of an image and all C bands of them (cs_inject_kernel's layout; 16-byte
//                        accesses when H W % 4 == 0 and the pointers allow it, scalar ones otherwise, the same values).  The first C
//                        lanes of the workgroup form a_c = sqrt(mom[c][c] / mom[C][C]) from the float64 moments
//                        [B, C + 1, C + 2] of plane_moments(ms_exp, pan_lp).  Per pixel, in fp64 after the loads, contraction off:
//                          D = P - L;   I = (sum_k M_k from 0, k ascending) / C
//                          mode 0 "atwt":  F_c = M_c + a_c D
//                          mode 1 "awlp":  F_c = M_c + ((M_c / I) a_c) D,  and F_c = M_c where I == 0
//                        rounded to fp32 once.  A lane loads all its bands before it stores any and nobody else touches its pixels:
//                        `out` may be ms_exp.  2 C + 2 planes of traffic.
#include "classical.h"

namespace {

constexpr int AT_T = 32;                              // the side of the tile a workgroup owns
constexpr int AT_MAX_LEVELS = 3;
constexpr int AWLP_MAXC = 14;                         // the limit of plane_moments
constexpr double AT_T0 = 1.0 / 16.0, AT_T1 = 4.0 / 16.0, AT_T2 = 6.0 / 16.0;

// a launch runs the levels first .. first + levels - 1 of the transform: its own level l has the dilation 2^(first - 1 + l - 1)
constexpr int at_halo(int levels, int l, int first) { return (2 * ((1 << levels) - (1 << l))) << (first - 1); }
constexpr int at_side(int levels, int first) { return AT_T + 2 * at_halo(levels, 0, first); }
constexpr size_t at_lds_bytes(int levels, int first) {
  return (size_t)at_side(levels, first) * at_side(levels, first) * (sizeof(double) + sizeof(float));
}

inline bool atrous_ok(int B, int C, int H, int W, int levels, int first) {
  // H, W <= 2^30: a tile's coordinates with their halo stay inside int
  return B >= 1 && C >= 1 && H >= 1 && W >= 1 && H <= (1 << 30) && W <= (1 << 30) && tmdiff::fits_int32((double)B * C * H * W) &&
         levels >= 1 && first >= 1 && first <= AT_MAX_LEVELS && levels <= AT_MAX_LEVELS + 1 - first;
}

struct AtrousArgs {
  const float* x;       // [planes, H, W]
  float* out;           // [planes, H, W]
  int planes, H, W, tiles_x;
};

__device__ __forceinline__ int at_clamp(int v, int n) { return min(max(v, 0), n - 1); }

// the five taps at v[base + at(k)], k = -2 .. 2, in the one order
template <class T, class At>
__device__ __forceinline__ double at_taps(const T* v, int base, At&& at) {
#pragma clang fp contract(off)
  double acc = AT_T0 * (double)v[base + at(-2)];
  acc = acc + AT_T1 * (double)v[base + at(-1)];
  acc = acc + AT_T2 * (double)v[base + at(0)];
  acc = acc + AT_T1 * (double)v[base + at(1)];
  acc = acc + AT_T0 * (double)v[base + at(2)];
  return acc;
}

// Level L of LEVELS on the staged tile: f holds c_{L-1} on the R_{L-1} region, and c_L on the R_L region afterwards (or `dst`, the
// plane of the output, after the last level).  Cell (ly, lx) of f and r is the pixel (y0 - R_0 + ly, x0 - R_0 + lx).
template <int LEVELS, int FIRST, int L>
__device__ __forceinline__ void atrous_level(float* f, double* r, int y0, int x0, int H, int W, int t, float* dst) {
  constexpr int R0 = at_halo(LEVELS, 0, FIRST), RP = at_halo(LEVELS, L - 1, FIRST), RL = at_halo(LEVELS, L, FIRST);
  constexpr int D = 1 << (FIRST - 1 + L - 1), LW = at_side(LEVELS, FIRST), PH = AT_T + 2 * RP, PW = AT_T + 2 * RL;
  for (int e = t; e < PH * PW; e += 256) {            // along W: the rows the column pass will read, the columns it keeps
    const int iy = e / PW, ix = e - iy * PW, gy = y0 - RP + iy, gx = x0 - RL + ix;
    if (gy < 0 || gy >= H || gx < 0 || gx >= W) continue;
    const int row = (gy - y0 + R0) * LW;
    r[row + (gx - x0 + R0)] = at_taps(f, row, [&](int k) { return at_clamp(gx + k * D, W) - x0 + R0; });
  }
  __syncthreads();
  for (int e = t; e < PW * PW; e += 256) {            // along H
    const int iy = e / PW, ix = e - iy * PW, gy = y0 - RL + iy, gx = x0 - RL + ix;
    if (gy < 0 || gy >= H || gx < 0 || gx >= W) continue;
    const int col = gx - x0 + R0;
    const float v = (float)at_taps(r, col, [&](int k) { return (at_clamp(gy + k * D, H) - y0 + R0) * LW; });
    if (L == LEVELS) dst[gy * W + gx] = v;
    else f[(gy - y0 + R0) * LW + col] = v;
  }
  if (L < LEVELS) __syncthreads();
}

template <int LEVELS, int FIRST>
__global__ void __launch_bounds__(256) atrous_lowpass_kernel(AtrousArgs a) {
  extern __shared__ double at_lds[];                  // r [LW][LW] fp64 | f [LW][LW] fp32
  constexpr int R0 = at_halo(LEVELS, 0, FIRST), LW = at_side(LEVELS, FIRST);
  double* r = at_lds;
  float* f = reinterpret_cast<float*>(r + LW * LW);
  const int H = a.H, W = a.W, t = threadIdx.x;
  const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
  const int y0 = ty * AT_T, x0 = tx * AT_T;
  const long plane = (long)H * W;
  for (long p = blockIdx.y; p < a.planes; p += gridDim.y) {
    const float* X = a.x + p * plane;
    __syncthreads();                                  // the plane before may still read the LDS
    for (int e = t; e < LW * LW; e += 256) {
      const int ly = e / LW, lx = e - ly * LW, gy = y0 - R0 + ly, gx = x0 - R0 + lx;
      if (gy >= 0 && gy < H && gx >= 0 && gx < W) f[e] = X[gy * W + gx];
    }
    __syncthreads();
    float* dst = a.out + p * plane;
    atrous_level<LEVELS, FIRST, 1>(f, r, y0, x0, H, W, t, dst);
    if constexpr (LEVELS >= 2) atrous_level<LEVELS, FIRST, 2>(f, r, y0, x0, H, W, t, dst);
    if constexpr (LEVELS >= 3) atrous_level<LEVELS, FIRST, 3>(f, r, y0, x0, H, W, t, dst);
  }
}

// ---- the injection ------------------------------------------------------------------------------------------------------------
struct AwlpArgs {
  const float* m;       // ms_exp [B, C, n]
  const float* p;       // pan    [B, n]
  const float* l;       // pan_lp [B, n]
  const double* mom;    // [B, C + 1, C + 2]
  float* out;           // [B, C, n]; may be m
  int B, n, mode, vec;
};

template <int C>
__global__ void __launch_bounds__(256) awlp_inject_kernel(AwlpArgs a) {
#pragma clang fp contract(off)
  __shared__ double ac[AWLP_MAXC];
  const long px = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  for (int b = blockIdx.y; b < a.B; b += gridDim.y) {
    __syncthreads();                            // the image before may still read ac
    if ((int)threadIdx.x < C) {
      const double* mo = a.mom + (long)b * (C + 1) * (C + 2);
      ac[threadIdx.x] = sqrt(mo[threadIdx.x * (C + 2) + threadIdx.x] / mo[C * (C + 2) + C]);
    }
    __syncthreads();
    if (px >= a.n) continue;
    const int cnt = (int)min((long)4, a.n - px);
    float pv[4], lv[4], mv[C][4];
    tmdiff::load_quad(a.p + (long)b * a.n + px, a.vec, cnt, pv);
    tmdiff::load_quad(a.l + (long)b * a.n + px, a.vec, cnt, lv);
#pragma unroll
    for (int c = 0; c < C; ++c) tmdiff::load_quad(a.m + ((long)b * C + c) * a.n + px, a.vec, cnt, mv[c]);
    double d[4], in[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int e = 0; e < 4; ++e) d[e] = (double)pv[e] - (double)lv[e];
    if (a.mode == 1) {
#pragma unroll
      for (int c = 0; c < C; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) in[e] = in[e] + (double)mv[c][e];
#pragma unroll
      for (int e = 0; e < 4; ++e) in[e] = in[e] / (double)C;
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const double g = ac[c];
      float f[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double mc = (double)mv[c][e];
        const double r = a.mode == 1 ? (in[e] == 0.0 ? mc : mc + ((mc / in[e]) * g) * d[e]) : mc + g * d[e];
        f[e] = (float)r;
      }
      tmdiff::store_quad(a.out + ((long)b * C + c) * a.n + px, a.vec, cnt, f);
    }
  }
}

inline bool at_overlap(const void* p, size_t pn, const void* q, size_t qn) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return a < b + qn && b < a + pn;
}

}  // namespace

extern "C" {

int tmdiff_atrous_supported(int32_t B, int32_t C, int32_t H, int32_t W, int32_t levels, int32_t first) {
  return atrous_ok(B, C, H, W, levels, first);
}

int tmdiff_atrous_lowpass(const float* x, float* out, int32_t B, int32_t C, int32_t H, int32_t W, int32_t levels, int32_t first,
                          tmdiff_stream_t stream) {
  if (!atrous_ok(B, C, H, W, levels, first))
    return tmdiff::fail(TMDIFF_E_UNSUPPORTED, "atrous_lowpass: B=%d C=%d H=%d W=%d levels=%d first=%d (B, C, H, W >= 1, H, W <= 2^30, "
                        "fewer than 2^31 elements, first >= 1, levels >= 1, first + levels <= 4)", B, C, H, W, levels, first);
  TMDIFF_REQUIRE(x && out, "atrous_lowpass: null tensor");
  const size_t n = (size_t)B * C * H * W * sizeof(float);
  TMDIFF_REQUIRE(!at_overlap(out, n, x, n), "atrous_lowpass: out overlaps x (x is read with a halo that other workgroups own)");
  const int tiles_x = (W + AT_T - 1) / AT_T;
  const long tiles = (long)((H + AT_T - 1) / AT_T) * tiles_x;
  if (const int rc = tmdiff::check_grid(tiles, "atrous_lowpass", TMDIFF_E_UNSUPPORTED)) return rc;
  const int planes = B * C;
  const AtrousArgs a{x, out, planes, H, W, tiles_x};
  const dim3 grid((unsigned)tiles, (unsigned)std::min(planes, 65535));
  const hipStream_t st = tmdiff::as_stream(stream);
  const auto launch = [&](auto lv, auto fs) {
    constexpr int LV = decltype(lv)::value, FS = decltype(fs)::value;
    atrous_lowpass_kernel<LV, FS><<<grid, 256, at_lds_bytes(LV, FS), st>>>(a);
  };
  using std::integral_constant;
  switch (10 * levels + first) {                      // the six pairs atrous_ok lets through
    case 11: launch(integral_constant<int, 1>{}, integral_constant<int, 1>{}); break;
    case 21: launch(integral_constant<int, 2>{}, integral_constant<int, 1>{}); break;
    case 31: launch(integral_constant<int, 3>{}, integral_constant<int, 1>{}); break;
    case 12: launch(integral_constant<int, 1>{}, integral_constant<int, 2>{}); break;
    case 22: launch(integral_constant<int, 2>{}, integral_constant<int, 2>{}); break;
    default: launch(integral_constant<int, 1>{}, integral_constant<int, 3>{}); break;
  }
  return tmdiff::check_launch("atrous_lowpass");
}

int tmdiff_awlp_inject(const float* ms_exp, const float* pan, const float* pan_lp, const double* moments, float* out, int32_t B,
                       int32_t C, int32_t H, int32_t W, int32_t mode, tmdiff_stream_t stream) {
  if (B < 1 || !tmdiff::planes_ok(B, C, AWLP_MAXC, H, W) || mode < 0 || mode > 1)
    return tmdiff::fail(TMDIFF_E_UNSUPPORTED, "awlp_inject: B=%d C=%d H=%d W=%d mode=%d (B >= 1, 1 <= C <= 14, H, W >= 1, fewer than "
                        "2^31 elements; mode 0 atwt, 1 awlp)", B, C, H, W, mode);
  TMDIFF_REQUIRE(ms_exp && pan && pan_lp && moments && out, "awlp_inject: null tensor");
  TMDIFF_REQUIRE((reinterpret_cast<uintptr_t>(moments) & 7u) == 0, "awlp_inject: moments must be 8-byte aligned");
  const int n = H * W;
  const int vec = n % 4 == 0 && tmdiff::aligned16(ms_exp) && tmdiff::aligned16(pan) && tmdiff::aligned16(pan_lp) && tmdiff::aligned16(out);
  const AwlpArgs a{ms_exp, pan, pan_lp, moments, out, B, n, mode, vec};
  const dim3 grid((unsigned)(((long)n + 1023) / 1024), (unsigned)std::min(B, 65535));
  const hipStream_t st = tmdiff::as_stream(stream);
  tmdiff::dispatch_bands<AWLP_MAXC>(C, [&](auto c) { awlp_inject_kernel<decltype(c)::value><<<grid, 256, 0, st>>>(a); });
  return tmdiff::check_launch("awlp_inject");
}

}  // extern "C"
