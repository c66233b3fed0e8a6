// Component-substitution pansharpening on gfx950 (host definitions: tmdiff_amd/metrics.py, plane_moments / cs_coeffs / cs_inject /
// cs_fuse): the joint second moments of all bands and the PAN, the constants of GS / GSA / Brovey made from them on the device,
// and the injection.  Nothing is read on the host, nothing is allocated, no atomics: the same bits on every run and in a graph
// replay.
//
//  plane_gram_kernel     The planes of an image are its C bands, the PAN and a plane of ones: C + 2 <= 16 rows of a 16 x 16 tile.
//                        One workgroup of 256 takes a chunk of GRAM_PIX consecutive flattened pixels of one image, wave w the
//                        GRAM_PIX / 4 pixels from chunk + w GRAM_PIX / 4 on, in steps of 16 pixels.  In a step, lane l holds
//                        plane p = l & 15 at the four pixels step + 4 (l >> 4) + e, e = 0 .. 3 (load_quad_minus_pilot,
//                        classical.h: 64 contiguous bytes per plane and step), as fp64 minus the plane's pilot; 1.0 on the
//                        ones row; 0.0 on rows >= C + 2 and on pixels past the end.  It then issues v_mfma_f64_16x16x4_f64
//                        four times, e ascending, with that register as both A and B: instruction e adds to G[i][j] the
//                        products of planes i and j at the pixels step + 4 k + e, k = 0 .. 3 being the instruction's K index
//                        (the order inside it is the hardware's and is fixed).  The tile's layout: classical.h.
//  SUMMATION ORDER of one entry G[i][j]: inside a wave one accumulator chain over the steps in ascending order and e ascending
//                        inside a step; the four waves' tiles through LDS in ascending wave index (waves_in_order, stats.h);
//                        the chunk's tile goes to the workspace; plane_gram_finalize_kernel, one workgroup per image with lane
//                        t owning entry t, adds the chunks in ascending order.
//  plane_gram_finalize_kernel  then keeps the raw sums at the head of the workspace, [B, C + 2, C + 2] with rows and columns in
//                        the order bands, PAN, ones (so column C + 1 holds the sums of d = value - pilot and the corner holds
//                        n), and forms with m_i = G[i][ones] / n: mean_i = pilot_i + m_i, cov_ij = G[i][j] / n - m_i m_j for
//                        i <= j, mirrored into the lower triangle: the output is exactly symmetric.
//  CONDITIONING: as glp_moments (metrics.hip): moments about a pilot, one pass; a constant plane has d == 0 everywhere and a
//                        variance and covariances of exactly 0.
//  cs_coeffs_kernel      one wave per image; lane 0 solves S_lr alpha = c_lr by ldl_factor and ldl_solve (classical.h) and forms
//                        the other constants in the loop order of metrics.cs_coeffs, every product and sum rounded on its own.
//  cs_inject_kernel<C>   elementwise: the 2 C + 3 constants go to LDS once per image, a lane owns four consecutive pixels,
//                        reads all C bands of them into registers (load_quad, classical.h), forms I = sum_k alpha_k M_k in fp64
//                        in ascending k, evaluates the formula in fp64 and rounds to fp32 once.  `out` may be ms_exp: a lane has
//                        read every band of its pixels before it writes any and nobody else touches them.  Traffic: 2 C + 1
//                        planes.
#include "classical.h"

namespace {

constexpr int CS_MAXC = 14;
constexpr int GRAM_PIX = 4096;                  // pixels of a workgroup's chunk
constexpr int GRAM_STEPS = GRAM_PIX / 4 / 16;   // steps of 16 pixels per wave
constexpr int GRAM_DEPTH = 8;                   // steps whose loads are issued together
constexpr int GRAM_AHEAD = 32;                  // chunks whose partial sums the finalize kernel loads together
static_assert(GRAM_STEPS % GRAM_DEPTH == 0, "whole batches");

inline int gram_chunks(long n) { return (int)((n + GRAM_PIX - 1) / GRAM_PIX); }
inline size_t gram_bytes(int B, int C, int H, int W) {
  return ((size_t)B * (C + 2) * (C + 2) + (size_t)B * gram_chunks((long)H * W) * 256) * sizeof(double);
}

struct GramArgs {
  const float* ms;    // [B, C, n]
  const float* pan;   // [B, n]
  int B, C, n, chunks, vec;
  double* sums;       // [B, C + 2, C + 2]
  double* part;       // [B, chunks, 256]
  double* out;        // [B, C + 1, C + 2]
};

__global__ void __launch_bounds__(256) plane_gram_kernel(GramArgs a) {
  __shared__ double red[4 * 256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, p = lane & 15;
  const long px0 = (long)blockIdx.x * GRAM_PIX + (long)wave * (GRAM_PIX / 4) + 4 * (lane >> 4);
  for (int b = blockIdx.y; b < a.B; b += gridDim.y) {
    const float* plane = p < a.C ? a.ms + ((long)b * a.C + p) * a.n : p == a.C ? a.pan + (long)b * a.n : nullptr;
    const float pilot = plane ? plane[0] : 0.f, fill = p == a.C + 1 ? 1.f : 0.f;
    tmdiff::gram_tile acc = {0.0, 0.0, 0.0, 0.0};
    double cur[GRAM_DEPTH][4], nxt[GRAM_DEPTH][4];
#pragma unroll
    for (int s = 0; s < GRAM_DEPTH; ++s)
      tmdiff::load_quad_minus_pilot(plane, plane != nullptr, pilot, fill, px0 + 16 * s, a.n, a.vec, cur[s]);
#pragma unroll
    for (int s0 = 0; s0 < GRAM_STEPS; s0 += GRAM_DEPTH) {
      if (s0 + GRAM_DEPTH < GRAM_STEPS) {
#pragma unroll
        for (int s = 0; s < GRAM_DEPTH; ++s)
          tmdiff::load_quad_minus_pilot(plane, plane != nullptr, pilot, fill, px0 + 16 * (s0 + GRAM_DEPTH + s), a.n, a.vec, nxt[s]);
      }
#pragma unroll
      for (int s = 0; s < GRAM_DEPTH; ++s)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(cur[s][e], cur[s][e], acc, 0, 0, 0);
#pragma unroll
      for (int s = 0; s < GRAM_DEPTH; ++s)
#pragma unroll
        for (int e = 0; e < 4; ++e) cur[s][e] = nxt[s][e];
    }
    __syncthreads();                                              // the image before may still read red
    tmdiff::store_gram_tile<256>(red, wave, 0, lane, acc);
    __syncthreads();
    const int row = threadIdx.x >> 4, col = threadIdx.x & 15;
    if (row < a.C + 2 && col < a.C + 2)
      a.part[((long)b * a.chunks + blockIdx.x) * 256 + threadIdx.x] = tmdiff::waves_in_order<256>(red, threadIdx.x, 0, 4);
  }
}

__global__ void __launch_bounds__(256) plane_gram_finalize_kernel(GramArgs a) {
  __shared__ double g[256];
  const int t = threadIdx.x, row = t >> 4, col = t & 15, k = a.C + 2;
  for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
    __syncthreads();                                              // the image before may still read g
    if (row < k && col < k) {
      // the chunks in ascending order, from 0.0; the loads of GRAM_AHEAD chunks are issued together, the additions stay in order
      const double* src = a.part + (long)b * a.chunks * 256 + t;
      double s = 0.0;
      int i = 0;
      for (; i + GRAM_AHEAD <= a.chunks; i += GRAM_AHEAD) {
        double v[GRAM_AHEAD];
#pragma unroll
        for (int u = 0; u < GRAM_AHEAD; ++u) v[u] = src[(long)(i + u) * 256];
#pragma unroll
        for (int u = 0; u < GRAM_AHEAD; ++u) s += v[u];
      }
      for (; i < a.chunks; ++i) s += src[(long)i * 256];
      g[t] = s;
      a.sums[((long)b * k + row) * k + col] = s;
    }
    __syncthreads();
    if (row <= a.C && col < k) {
      const double n = (double)a.n;
      double v;
      if (col == a.C + 1) {
        const float* plane = row < a.C ? a.ms + ((long)b * a.C + row) * a.n : a.pan + (long)b * a.n;
        v = (double)plane[0] + g[row * 16 + a.C + 1] / n;
      } else {
        const int i = min(row, col), j = max(row, col);
        const double mi = g[i * 16 + a.C + 1] / n, mj = g[j * 16 + a.C + 1] / n;
        v = g[i * 16 + j] / n - mi * mj;
      }
      a.out[((long)b * (a.C + 1) + row) * k + col] = v;
    }
  }
}

// ---- the constants ------------------------------------------------------------------------------------------------------------
struct CoefArgs {
  const double* full;   // [B, C + 1, C + 2]
  const double* low;    // the same at the reduced scale; null unless mode 1
  double* out;          // [B, 2 C + 3]: alpha, g, a, mean_I, mean_P
  int B, C, mode;
};

__global__ void __launch_bounds__(64) cs_coeffs_kernel(CoefArgs a) {
#pragma clang fp contract(off)
  __shared__ double fac[CS_MAXC * CS_MAXC], piv[CS_MAXC], y[CS_MAXC], alpha[CS_MAXC], sa[CS_MAXC];
  if (threadIdx.x != 0) return;
  const int C = a.C, ld = C + 2;
  for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
    const double* full = a.full + (long)b * (C + 1) * ld;
    double* out = a.out + (long)b * (2 * C + 3);
    bool bad = false;
    if (a.mode == 1) {                                            // S_lr alpha = c_lr, column C of low
      const double* low = a.low + (long)b * (C + 1) * ld;
      bad = tmdiff::ldl_factor<CS_MAXC>(low, ld, C, fac, piv);
      tmdiff::ldl_solve<CS_MAXC>(low + C, ld, C, fac, piv, y, alpha);
    } else {
      for (int k = 0; k < C; ++k) alpha[k] = 1.0 / (double)C;
    }
    for (int i = 0; i < C; ++i) {
      double s = 0.0;
      for (int k = 0; k < C; ++k) s = s + full[i * ld + k] * alpha[k];
      sa[i] = s;
    }
    double var_i = 0.0, mean_i = 0.0;
    for (int k = 0; k < C; ++k) {
      var_i = var_i + alpha[k] * sa[k];
      mean_i = mean_i + alpha[k] * full[k * ld + C + 1];
    }
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    for (int k = 0; k < C; ++k) {
      out[k] = bad ? nan : alpha[k];
      out[C + k] = bad ? nan : sa[k] / var_i;
    }
    out[2 * C] = bad ? nan : sqrt(var_i / full[C * ld + C]);
    out[2 * C + 1] = bad ? nan : mean_i;
    out[2 * C + 2] = bad ? nan : full[C * ld + C + 1];
  }
}

// ---- the injection ------------------------------------------------------------------------------------------------------------
struct CsInjectArgs {
  const float* m;       // ms_exp [B, C, n]
  const float* p;       // pan    [B, n]
  const double* coef;   // [B, 2 C + 3]
  float* out;           // [B, C, n]; may be m
  int B, n, mode, vec;
};

template <int C>
__global__ void __launch_bounds__(256) cs_inject_kernel(CsInjectArgs a) {
  __shared__ double cst[2 * CS_MAXC + 3];
  const long px = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  for (int b = blockIdx.y; b < a.B; b += gridDim.y) {
    __syncthreads();                            // the image before may still read cst
    if ((int)threadIdx.x < 2 * C + 3) cst[threadIdx.x] = a.coef[(long)b * (2 * C + 3) + threadIdx.x];
    __syncthreads();
    if (px >= a.n) continue;
    const int cnt = (int)min((long)4, a.n - px);
    float pv[4], mv[C][4];
    tmdiff::load_quad(a.p + (long)b * a.n + px, a.vec, cnt, pv);
#pragma unroll
    for (int c = 0; c < C; ++c) tmdiff::load_quad(a.m + ((long)b * C + c) * a.n + px, a.vec, cnt, mv[c]);
    double in[4] = {0.0, 0.0, 0.0, 0.0}, pi[4];
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
      for (int e = 0; e < 4; ++e) in[e] += cst[c] * (double)mv[c][e];
#pragma unroll
    for (int e = 0; e < 4; ++e) pi[e] = cst[2 * C] * ((double)pv[e] - cst[2 * C + 2]) + cst[2 * C + 1];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const double gc = cst[C + c];
      float f[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double r = a.mode == 2 ? (double)mv[c][e] * pi[e] / (in[e] + 0x1p-52) : (double)mv[c][e] + gc * (pi[e] - in[e]);
        f[e] = (float)r;
      }
      tmdiff::store_quad(a.out + ((long)b * C + c) * a.n + px, a.vec, cnt, f);
    }
  }
}

}  // namespace

extern "C" {

size_t tmdiff_plane_gram_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W) {
  return tmdiff::planes_ok(B, C, CS_MAXC, H, W) ? gram_bytes(B, C, H, W) : 0;
}

int tmdiff_plane_gram(const float* ms, const float* pan, int32_t B, int32_t C, int32_t H, int32_t W, double* out, void* workspace,
                      size_t workspace_bytes, tmdiff_stream_t stream) {
  if (!tmdiff::planes_ok(B, C, CS_MAXC, H, W))
    return tmdiff::fail(TMDIFF_E_UNSUPPORTED, "plane_gram: B=%d C=%d H=%d W=%d (B >= 0, 1 <= C <= 14, H, W >= 1, fewer than 2^31 "
                        "elements)", B, C, H, W);
  if (B == 0) return TMDIFF_OK;
  TMDIFF_REQUIRE(ms && pan && out && workspace, "plane_gram: null tensor");
  TMDIFF_REQUIRE((reinterpret_cast<uintptr_t>(out) & 7u) == 0, "plane_gram: out must be 8-byte aligned");
  if (const int rc = tmdiff::check_workspace("plane_gram", workspace, workspace_bytes, gram_bytes(B, C, H, W))) return rc;
  const hipStream_t st = tmdiff::as_stream(stream);
  const int n = H * W, chunks = gram_chunks(n);
  double* ws = static_cast<double*>(workspace);
  const int vec = n % 4 == 0 && tmdiff::aligned16(ms) && tmdiff::aligned16(pan);
  const GramArgs a{ms, pan, B, C, n, chunks, vec, ws, ws + (size_t)B * (C + 2) * (C + 2), out};
  plane_gram_kernel<<<dim3((unsigned)chunks, (unsigned)std::min(B, 65535)), 256, 0, st>>>(a);
  if (const int rc = tmdiff::check_launch("plane_gram")) return rc;
  plane_gram_finalize_kernel<<<dim3((unsigned)std::min(B, 65535)), 256, 0, st>>>(a);
  return tmdiff::check_launch("plane_gram (finalize)");
}

int tmdiff_cs_coeffs(const double* full, const double* low, double* out, int32_t B, int32_t C, int32_t mode,
                     tmdiff_stream_t stream) {
  if (B < 0 || C < 1 || C > CS_MAXC || mode < 0 || mode > 2)
    return tmdiff::fail(TMDIFF_E_UNSUPPORTED, "cs_coeffs: B=%d C=%d mode=%d (B >= 0, 1 <= C <= 14; mode 0 gs, 1 gsa, 2 brovey)", B, C,
                        mode);
  if (B == 0) return TMDIFF_OK;
  TMDIFF_REQUIRE(full && out && (low || mode != 1), "cs_coeffs: null tensor (low is needed by mode 1, gsa)");
  TMDIFF_REQUIRE(((reinterpret_cast<uintptr_t>(full) | reinterpret_cast<uintptr_t>(low) | reinterpret_cast<uintptr_t>(out)) & 7u) == 0,
                 "cs_coeffs: tensors must be 8-byte aligned");
  const CoefArgs a{full, low, out, B, C, mode};
  cs_coeffs_kernel<<<dim3((unsigned)std::min(B, 65535)), 64, 0, tmdiff::as_stream(stream)>>>(a);
  return tmdiff::check_launch("cs_coeffs");
}

int tmdiff_cs_inject(const float* ms_exp, const float* pan, const double* coef, float* out, int32_t B, int32_t C, int32_t H,
                     int32_t W, int32_t mode, tmdiff_stream_t stream) {
  if (!tmdiff::planes_ok(B, C, CS_MAXC, H, W) || mode < 0 || mode > 2)
    return tmdiff::fail(TMDIFF_E_UNSUPPORTED, "cs_inject: B=%d C=%d H=%d W=%d mode=%d (B >= 0, 1 <= C <= 14, H, W >= 1, fewer than "
                        "2^31 elements; mode 0 gs, 1 gsa, 2 brovey)", B, C, H, W, mode);
  if (B == 0) return TMDIFF_OK;
  TMDIFF_REQUIRE(ms_exp && pan && coef && out, "cs_inject: null tensor");
  TMDIFF_REQUIRE((reinterpret_cast<uintptr_t>(coef) & 7u) == 0, "cs_inject: coef must be 8-byte aligned");
  const int n = H * W;
  const int vec = n % 4 == 0 && tmdiff::aligned16(ms_exp) && tmdiff::aligned16(pan) && tmdiff::aligned16(out);
  const CsInjectArgs a{ms_exp, pan, coef, out, B, n, mode, vec};
  const dim3 grid((unsigned)(((long)n + 1023) / 1024), (unsigned)std::min(B, 65535));
  const hipStream_t st = tmdiff::as_stream(stream);
  tmdiff::dispatch_bands<CS_MAXC>(C, [&](auto c) { cs_inject_kernel<decltype(c)::value><<<grid, 256, 0, st>>>(a); });
  return tmdiff::check_launch("cs_inject");
}

}  // extern "C"
