// The injection of MTF-GLP on gfx950 (host definition: tmdiff_amd/metrics.py, mtf_glp / glp_inject): the fused image from
// M = ms_exp [B, C, H, W], P = pan [B, H, W], L = pan_lp [B, C, H, W] and the moments that glp_moments_kernel (metrics.hip) left
// on the device, float64 [B, C, 7] in the order of metrics.GLP_MOMENT_FIELDS.  Nothing is read on the host: the first C lanes of
// a workgroup form the band constants in fp64 from the moments,
//   a_c = sqrt(var(M_c) / var(L_c)),   g_c = cov(M_c, L_c) / (a_c var(L_c))  ("cbd"; 1 otherwise)
// and every lane then evaluates, in fp64 after the loads and rounded to fp32 once,
//   P_c = a_c (P - mean(P)) + mean(M_c),   PL_c = a_c (L_c - mean(P)) + mean(M_c)
//   "glp", "cbd":  F_c = M_c + g_c (P_c - PL_c)          "hpm":  F_c = M_c P_c / (PL_c + 2^-52)
// No sum runs over pixels here, so there is no summation order to state: a pixel is a fixed expression of its own three
// inputs and the band's constants.  A band with var(L_c) == 0 is NaN or inf throughout, as the definition has it.
//
// A lane owns four consecutive pixels of a plane and walks the bands with the four PAN values in registers: P is read once,
// M_c and L_c once each, F_c written once -- 3 C + 1 planes of traffic.  16-byte loads and stores when W % 4 == 0 and the
// pointers allow it, scalar ones otherwise, with the same values.  `out` may be ms_exp: a lane reads a pixel of M before it
// writes that pixel and nobody else touches it.  The quads keep their own text, not load_quad / store_quad of classical.h:
// with that form the compiler merges the fourth pixel of the two paths and turns each of this kernel's 16-byte accesses into
// one of 12 and one of 4 bytes (profiles/classical_refactor.txt, section 2).
#include "classical.h"

namespace {

constexpr int MAXC = 16;

struct InjectArgs {
  const float* m;
  const float* p;
  const float* l;
  const double* mom;
  float* out;
  int B, C, n, mode, vec;
};

__global__ void __launch_bounds__(256) glp_inject_kernel(InjectArgs a) {
  __shared__ double cst[MAXC][4];               // a_c, g_c, mean(M_c), mean(P)
  const long px = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  for (int b = blockIdx.y; b < a.B; b += gridDim.y) {
    __syncthreads();                            // the image before may still read cst
    if ((int)threadIdx.x < a.C) {
      const double* mo = a.mom + ((long)b * a.C + threadIdx.x) * 7;
      const double ac = sqrt(mo[3] / mo[4]);
      cst[threadIdx.x][0] = ac;
      cst[threadIdx.x][1] = a.mode == 1 ? mo[5] / (ac * mo[4]) : 1.0;
      cst[threadIdx.x][2] = mo[0];
      cst[threadIdx.x][3] = mo[2];
    }
    __syncthreads();
    if (px >= a.n) continue;
    const int cnt = (int)min((long)4, a.n - px);
    const float* pp = a.p + (long)b * a.n + px;
    float pv[4] = {0.f, 0.f, 0.f, 0.f};
    if (a.vec) *reinterpret_cast<float4*>(pv) = *reinterpret_cast<const float4*>(pp);
    else
      for (int e = 0; e < cnt; ++e) pv[e] = pp[e];
    for (int c = 0; c < a.C; ++c) {
      const long o = ((long)b * a.C + c) * a.n + px;
      const double ac = cst[c][0], gc = cst[c][1], mean_m = cst[c][2], mean_p = cst[c][3];
      float mv[4] = {0.f, 0.f, 0.f, 0.f}, lv[4] = {0.f, 0.f, 0.f, 0.f}, f[4];
      if (a.vec) {
        *reinterpret_cast<float4*>(mv) = *reinterpret_cast<const float4*>(a.m + o);
        *reinterpret_cast<float4*>(lv) = *reinterpret_cast<const float4*>(a.l + o);
      } else {
        for (int e = 0; e < cnt; ++e) mv[e] = a.m[o + e], lv[e] = a.l[o + e];
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double pc = ac * ((double)pv[e] - mean_p) + mean_m;
        const double plc = ac * ((double)lv[e] - mean_p) + mean_m;
        const double r = a.mode == 2 ? (double)mv[e] * pc / (plc + 0x1p-52) : (double)mv[e] + gc * (pc - plc);
        f[e] = (float)r;
      }
      if (a.vec) *reinterpret_cast<float4*>(a.out + o) = *reinterpret_cast<const float4*>(f);
      else
        for (int e = 0; e < cnt; ++e) a.out[o + e] = f[e];
    }
  }
}

}  // namespace

extern "C" {

int tmdiff_glp_inject(const float* ms_exp, const float* pan, const float* pan_lp, const double* moments, float* out, int32_t B,
                      int32_t C, int32_t H, int32_t W, int32_t mode, tmdiff_stream_t stream) {
  if (!tmdiff::planes_ok(B, C, MAXC, H, W) || mode < 0 || mode > 2)
    return tmdiff::fail(TMDIFF_E_UNSUPPORTED, "glp_inject: B=%d C=%d H=%d W=%d mode=%d (B >= 0, 1 <= C <= 16, H, W >= 1, fewer than "
                        "2^31 elements; mode 0 glp, 1 cbd, 2 hpm)", B, C, H, W, mode);
  if (B == 0) return TMDIFF_OK;
  TMDIFF_REQUIRE(ms_exp && pan && pan_lp && moments && out, "glp_inject: null tensor");
  TMDIFF_REQUIRE((reinterpret_cast<uintptr_t>(moments) & 7u) == 0, "glp_inject: moments must be 8-byte aligned");
  const int n = H * W;
  const int vec = W % 4 == 0 && tmdiff::aligned16(ms_exp) && tmdiff::aligned16(pan) && tmdiff::aligned16(pan_lp) && tmdiff::aligned16(out);
  const InjectArgs a{ms_exp, pan, pan_lp, moments, out, B, C, n, mode, vec};
  const dim3 grid((unsigned)(((long)n + 1023) / 1024), (unsigned)std::min(B, 65535));
  glp_inject_kernel<<<grid, 256, 0, tmdiff::as_stream(stream)>>>(a);
  return tmdiff::check_launch("glp_inject");
}

}  // extern "C"
