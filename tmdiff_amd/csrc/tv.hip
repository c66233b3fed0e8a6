// TV pansharpening on gfx950 (host definitions: tmdiff_amd/metrics.py, tv_pd_step / tv_norm / tv_pansharpen): the band-coupled
// part of one Condat-Vu iteration on  J(x) = 1/2 ||A x - lr_ms||^2 + gamma/2 ||sum_c w_c x_c + w_C - pan||^2 + lam TV(x)  with
// the vector total variation TV(x) = sum over pixels of sqrt(sum_c (Dh x_c)^2 + (Dv x_c)^2), and the value of TV.  Nothing is read
// on the host, nothing is allocated, no atomics: the same bits on every run and in a graph replay; a batch equals its samples.
//
//  DIFFERENCES           (Dh x)[i, j] = x[i, j + 1] - x[i, j] for j < W - 1 and 0 at j = W - 1; (Dv x)[i, j] = x[i + 1, j] - x[i, j]
//                        for i < H - 1 and 0 at i = H - 1.  The transpose is masked,
//                          (D^T p)[i, j] = ph[i, j-1] [j > 0] - ph[i, j] [j < W-1] + pv[i-1, j] [i > 0] - pv[i, j] [i < H-1],
//                        added left to right; a masked term is not loaded.
//  tv_pd_step_kernel     one workgroup of 256 per 16 x 32 tile of one image (grid.y walks the batch), all C bands.  The caller made
//                        u = x - tau A^T (A x - lr_ms).  Three phases, fp64 after the loads, every stored value rounded once:
//                     A  over the tile plus one column to the right and one row below (17 x 33 pixels, lane t takes t, t + 256,
//                        t + 512): s = sum_c w_c x_c (one chain of fused multiply-adds, c ascending, from 0) + w_C - pan, formed once
//                        per pixel; then per band  x' = (float)(u - tau ((gamma w_c) s + D^T p)).  The tile's owner stores x'; the
//                        extra column and row are recomputed from the neighbours' inputs and never stored.  LDS keeps
//                        xbar = 2 x' - x per band and pixel in fp64, from x' AS STORED (exact for fp32 data within 2^29 of each
//                        other).  A pixel outside the image holds 0 and is never used: the masks of D come first.
//                     B  lane t owns the pixels (t >> 5, t & 31) and (8 + (t >> 5), t & 31) of the tile: per band
//                        qh = ph + sigma Dh xbar, qv = pv + sigma Dv xbar, n^2 = one chain of fused multiply-adds over c ascending,
//                        h before v; then r = 1 / max(1, sqrt(n^2) / lam).
//                     C  the bands again: qh, qv are recomputed (ph, pv are read a second time, from cache; 2 C values per pixel
//                        would not fit the registers) and ph' = (float)(qh r), pv' = (float)(qv r); lam == 0 stores 0.
//                        LDS: (561 C + 17) doubles, 71,944 bytes at C = 16 (two workgroups per CU), 18,088 at C = 4.
//                        HBM traffic: u, x, ph, pv in and x', ph', pv' out per band, and the PAN: 7 C + 1 planes.
//  ALIASING              u, x, ph and pv are all read with a halo that another workgroup owns, so NO output may overlap any input:
//                        the solver ping-pongs x and p.  The entry point refuses an overlap.
//  tv_norm_kernel        the same tiles and pixel ownership; per pixel n^2 as above from Dh x, Dv x, then sqrt; a lane adds its two
//                        pixels (upper first), the workgroup adds its lanes (block_sum_f64, stats.h) and stores one partial sum per
//                        tile; tv_norm_finalize_kernel, one workgroup per image, adds the tiles (strided_sum, then block_sum_f64).
#include "classical.h"

namespace {

constexpr int TV_MAXC = 16;
constexpr int TV_TH = 16, TV_TW = 32;                 // the tile a workgroup owns
constexpr int TV_EW = TV_TW + 1, TV_EXT = (TV_TH + 1) * TV_EW;   // ... and the pixels it computes x' on

inline long tv_tiles(int H, int W) { return (long)((H + TV_TH - 1) / TV_TH) * ((W + TV_TW - 1) / TV_TW); }
inline bool tv_ok(int B, int C, int H, int W) {
  return tmdiff::planes_ok(B, C, TV_MAXC, H, W) && tv_tiles(H, W) <= 0x7fffffffL;
}
inline size_t tv_lds_bytes(int C) { return ((size_t)C * TV_EXT + TV_MAXC + 1) * sizeof(double); }
inline size_t tv_norm_bytes(int B, int H, int W) { return (size_t)B * tv_tiles(H, W) * sizeof(double); }

struct TvStepArgs {
  const float* u;       // [B, C, H, W]
  const float* x;       // [B, C, H, W]
  const float* pan;     // [B, H, W]
  const float* ph;      // [B, C, H, W]
  const float* pv;      // [B, C, H, W]
  const double* wts;    // [B, C + 1]
  float* xo;            // [B, C, H, W]
  float* pho;           // [B, C, H, W]
  float* pvo;           // [B, C, H, W]
  double tau, sigma, lam, gamma;
  int B, C, H, W, tiles_x;
};

__global__ void __launch_bounds__(256) tv_pd_step_kernel(TvStepArgs a) {
  extern __shared__ double tv_lds[];                  // xbar [C][TV_EXT] | weights [TV_MAXC + 1]
  const int C = a.C, H = a.H, W = a.W, t = threadIdx.x;
  double* xb = tv_lds;
  double* wt = xb + C * TV_EXT;
  const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
  const int y0 = ty * TV_TH, x0 = tx * TV_TW;
  const long plane = (long)H * W;
  // the lane's two pixels of the tile
  int pe[2], poff[2];
  bool pin[2], pmr[2], pmd[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int ly = (t >> 5) + 8 * k, lx = t & 31, gy = y0 + ly, gx = x0 + lx;
    pe[k] = ly * TV_EW + lx;
    pin[k] = gy < H && gx < W;
    poff[k] = pin[k] ? gy * W + gx : 0;
    pmr[k] = gx < W - 1;
    pmd[k] = gy < H - 1;
  }
  for (int b = blockIdx.y; b < a.B; b += gridDim.y) {
    const float* U = a.u + (long)b * C * plane;
    const float* X = a.x + (long)b * C * plane;
    const float* PH = a.ph + (long)b * C * plane;
    const float* PV = a.pv + (long)b * C * plane;
    const float* P = a.pan + (long)b * plane;
    float* XO = a.xo + (long)b * C * plane;
    float* PHO = a.pho + (long)b * C * plane;
    float* PVO = a.pvo + (long)b * C * plane;
    __syncthreads();                                  // the image before may still read the LDS
    if (t <= C) wt[t] = a.wts[(long)b * (C + 1) + t];
    __syncthreads();
    // ---- A: x' and xbar on the tile and its right column and lower row
    for (int e = t; e < TV_EXT; e += 256) {
      const int ly = e / TV_EW, lx = e - ly * TV_EW, gy = y0 + ly, gx = x0 + lx;
      if (gy >= H || gx >= W) {
        for (int c = 0; c < C; ++c) xb[c * TV_EXT + e] = 0.0;
        continue;
      }
      const int off = gy * W + gx;
      double acc = 0.0;
      for (int c = 0; c < C; ++c) {
        const double xv = (double)X[c * plane + off];
        xb[c * TV_EXT + e] = xv;
        acc = fma(wt[c], xv, acc);
      }
      const double s = acc + wt[C] - (double)P[off];
      const bool own = ly < TV_TH && lx < TV_TW;
      const bool ml = gx > 0, mr = gx < W - 1, mu = gy > 0, md = gy < H - 1;
      for (int c = 0; c < C; ++c) {
        const float* hp = PH + c * plane + off;
        const float* vp = PV + c * plane + off;
        const double h0 = ml ? (double)hp[-1] : 0.0, h1 = mr ? (double)hp[0] : 0.0;
        const double v0 = mu ? (double)vp[-W] : 0.0, v1 = md ? (double)vp[0] : 0.0;
        const double dtp = ((h0 - h1) + v0) - v1;
        const float xn = (float)((double)U[c * plane + off] - a.tau * ((a.gamma * wt[c]) * s + dtp));
        if (own) XO[c * plane + off] = xn;
        xb[c * TV_EXT + e] = 2.0 * (double)xn - xb[c * TV_EXT + e];
      }
    }
    __syncthreads();
    // ---- B: the norm of q over the 2 C components of a pixel
    double n2[2] = {0.0, 0.0};
    for (int c = 0; c < C; ++c) {
      const double* xc = xb + c * TV_EXT;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        if (!pin[k]) continue;
        const double ctr = xc[pe[k]];
        const double qh = (double)PH[c * plane + poff[k]] + a.sigma * (pmr[k] ? xc[pe[k] + 1] - ctr : 0.0);
        const double qv = (double)PV[c * plane + poff[k]] + a.sigma * (pmd[k] ? xc[pe[k] + TV_EW] - ctr : 0.0);
        n2[k] = fma(qh, qh, n2[k]);
        n2[k] = fma(qv, qv, n2[k]);
      }
    }
    double r[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) r[k] = a.lam > 0.0 ? 1.0 / fmax(1.0, sqrt(n2[k]) / a.lam) : 0.0;
    // ---- C: q again, projected
    for (int c = 0; c < C; ++c) {
      const double* xc = xb + c * TV_EXT;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        if (!pin[k]) continue;
        const double ctr = xc[pe[k]];
        const double qh = (double)PH[c * plane + poff[k]] + a.sigma * (pmr[k] ? xc[pe[k] + 1] - ctr : 0.0);
        const double qv = (double)PV[c * plane + poff[k]] + a.sigma * (pmd[k] ? xc[pe[k] + TV_EW] - ctr : 0.0);
        PHO[c * plane + poff[k]] = a.lam > 0.0 ? (float)(qh * r[k]) : 0.f;
        PVO[c * plane + poff[k]] = a.lam > 0.0 ? (float)(qv * r[k]) : 0.f;
      }
    }
  }
}

struct TvNormArgs {
  const float* x;       // [B, C, H, W]
  double* part;         // [B, tiles]
  double* out;          // [B]
  int B, C, H, W, tiles_x, tiles;
};

__global__ void __launch_bounds__(256) tv_norm_kernel(TvNormArgs a) {
  __shared__ double red[4];
  const int C = a.C, H = a.H, W = a.W, t = threadIdx.x;
  const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
  const long plane = (long)H * W;
  for (int b = blockIdx.y; b < a.B; b += gridDim.y) {
    const float* X = a.x + (long)b * C * plane;
    double v = 0.0;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int gy = ty * TV_TH + (t >> 5) + 8 * k, gx = tx * TV_TW + (t & 31);
      if (gy >= H || gx >= W) continue;
      const int off = gy * W + gx;
      const bool mr = gx < W - 1, md = gy < H - 1;
      double n2 = 0.0;
      for (int c = 0; c < C; ++c) {
        const float* xp = X + c * plane + off;
        const double ctr = (double)xp[0];
        const double dh = mr ? (double)xp[1] - ctr : 0.0, dv = md ? (double)xp[W] - ctr : 0.0;
        n2 = fma(dh, dh, n2);
        n2 = fma(dv, dv, n2);
      }
      v += sqrt(n2);
    }
    __syncthreads();                                  // the image before may still read red
    v = tmdiff::block_sum_f64(v, red);
    if (t == 0) a.part[(long)b * a.tiles + blockIdx.x] = v;
  }
}

__global__ void __launch_bounds__(256) tv_norm_finalize_kernel(TvNormArgs a) {
  __shared__ double red[4];
  for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
    double v = tmdiff::strided_sum(a.part + (long)b * a.tiles, a.tiles, 1, threadIdx.x, 256);
    __syncthreads();
    v = tmdiff::block_sum_f64(v, red);
    if (threadIdx.x == 0) a.out[b] = v;
  }
}

inline bool tv_overlap(const void* p, size_t pn, const void* q, size_t qn) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return a < b + qn && b < a + pn;
}

const char* const TV_LIMITS = "B >= 0, 1 <= C <= 16, H, W >= 1, fewer than 2^31 elements";

}  // namespace

extern "C" {

int tmdiff_tv_supported(int32_t B, int32_t C, int32_t H, int32_t W) { return tv_ok(B, C, H, W); }

int tmdiff_tv_pd_step(const float* u, const float* x, const float* pan, const float* ph, const float* pv, const double* weights,
                      double tau, double sigma, double lam, double gamma, float* x_out, float* ph_out, float* pv_out, int32_t B,
                      int32_t C, int32_t H, int32_t W, tmdiff_stream_t stream) {
  if (!tv_ok(B, C, H, W)) return tmdiff::fail(TMDIFF_E_UNSUPPORTED, "tv_pd_step: B=%d C=%d H=%d W=%d (%s)", B, C, H, W, TV_LIMITS);
  TMDIFF_REQUIRE(tau > 0.0 && sigma >= 0.0 && lam >= 0.0 && gamma >= 0.0, "tv_pd_step: tau=%g sigma=%g lam=%g gamma=%g (tau > 0, the "
                 "others >= 0)", tau, sigma, lam, gamma);
  if (B == 0) return TMDIFF_OK;
  TMDIFF_REQUIRE(u && x && pan && ph && pv && weights && x_out && ph_out && pv_out, "tv_pd_step: null tensor");
  TMDIFF_REQUIRE((reinterpret_cast<uintptr_t>(weights) & 7u) == 0, "tv_pd_step: weights must be 8-byte aligned");
  const size_t n = (size_t)B * C * H * W * sizeof(float);
  const void* ins[6] = {u, x, ph, pv, pan, weights};
  const size_t in_bytes[6] = {n, n, n, n, (size_t)B * H * W * sizeof(float), (size_t)B * (C + 1) * sizeof(double)};
  const void* outs[3] = {x_out, ph_out, pv_out};
  for (int o = 0; o < 3; ++o) {
    for (int i = 0; i < 6; ++i)
      TMDIFF_REQUIRE(!tv_overlap(outs[o], n, ins[i], in_bytes[i]), "tv_pd_step: an output overlaps an input (every input is read with "
                     "a halo: ping-pong)");
    for (int k = o + 1; k < 3; ++k) TMDIFF_REQUIRE(!tv_overlap(outs[o], n, outs[k], n), "tv_pd_step: two outputs overlap");
  }
  const int tiles_x = (W + TV_TW - 1) / TV_TW;
  const long tiles = tv_tiles(H, W);
  if (const int rc = tmdiff::check_grid(tiles, "tv_pd_step", TMDIFF_E_UNSUPPORTED)) return rc;
  const size_t lds = tv_lds_bytes(C);
  if (lds > 48 * 1024) {
    // more dynamic LDS than a launch gets by default: raise the kernel's limit once per device
    static bool raised[64] = {false};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return tmdiff::fail(TMDIFF_E_LAUNCH, "tv_pd_step: no current device");
    if (!raised[dev]) {
      const size_t most = tv_lds_bytes(TV_MAXC);
      const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(tv_pd_step_kernel),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)most);
      if (e != hipSuccess) return tmdiff::fail(TMDIFF_E_LAUNCH, "tv_pd_step: %zu bytes of LDS: %s", most, hipGetErrorString(e));
      raised[dev] = true;
    }
  }
  const TvStepArgs a{u, x, pan, ph, pv, weights, x_out, ph_out, pv_out, tau, sigma, lam, gamma, B, C, H, W, tiles_x};
  tv_pd_step_kernel<<<dim3((unsigned)tiles, (unsigned)std::min(B, 65535)), 256, lds, tmdiff::as_stream(stream)>>>(a);
  return tmdiff::check_launch("tv_pd_step");
}

size_t tmdiff_tv_norm_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W) {
  return tv_ok(B, C, H, W) ? tv_norm_bytes(B, H, W) : 0;
}

int tmdiff_tv_norm(const float* x, int32_t B, int32_t C, int32_t H, int32_t W, double* out, void* workspace, size_t workspace_bytes,
                   tmdiff_stream_t stream) {
  if (!tv_ok(B, C, H, W)) return tmdiff::fail(TMDIFF_E_UNSUPPORTED, "tv_norm: B=%d C=%d H=%d W=%d (%s)", B, C, H, W, TV_LIMITS);
  if (B == 0) return TMDIFF_OK;
  TMDIFF_REQUIRE(x && out && workspace, "tv_norm: null tensor");
  if (const int rc = tmdiff::check_workspace("tv_norm", workspace, workspace_bytes, tv_norm_bytes(B, H, W), "; out too", out)) return rc;
  const long tiles = tv_tiles(H, W);
  if (const int rc = tmdiff::check_grid(tiles, "tv_norm", TMDIFF_E_UNSUPPORTED)) return rc;
  const hipStream_t st = tmdiff::as_stream(stream);
  const TvNormArgs a{x, static_cast<double*>(workspace), out, B, C, H, W, (W + TV_TW - 1) / TV_TW, (int)tiles};
  tv_norm_kernel<<<dim3((unsigned)tiles, (unsigned)std::min(B, 65535)), 256, 0, st>>>(a);
  if (const int rc = tmdiff::check_launch("tv_norm")) return rc;
  tv_norm_finalize_kernel<<<dim3((unsigned)std::min(B, 65535)), 256, 0, st>>>(a);
  return tmdiff::check_launch("tv_norm (finalize)");
}

}  // extern "C"
