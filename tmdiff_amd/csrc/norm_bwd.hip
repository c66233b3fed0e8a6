// Backward of the memory-bound operators around the attention core (core/Attention.py :69-96, :108-109, :279-281), so that the
// transformer blocks built on them can be trained: LayerNorm, GroupNorm and GEGLU / GELU.  fp32 throughout, 64-bit element
// offsets, no atomics and no host synchronisation: every sum has a fixed order, so results repeat bit for bit.
//   layer_norm_bwd_kernel : one wave per row (as the forward).  With g = dy * gamma and xhat = (x - mean) * rstd,
//                           dx = rstd * (g - mean_D(g) - xhat * mean_D(g * xhat)).  A workgroup owns a fixed block of rows; its
//                           lanes keep the column sums of dy * xhat and dy over those rows in registers and write them as one
//                           row of partials, which col_sum_parts_kernel adds up in block order (dgamma, dbeta).
//   group_norm_bwd_kernel : one workgroup per (b, group) (as the forward).  Pass 1 forms the per-channel sums of dy and
//                           dy * xhat -- they are the [B, C] partials of dbeta / dgamma, and weighted by gamma they add up to
//                           the two group sums -- pass 2 writes dx.  col_sum_parts_kernel sums the partials over b.
//   geglu_bwd_kernel      : elementwise, float4 where the row length allows.
// Parameter gradients are two-stage rather than atomic: an atomic float add commits in arrival order, so the sum would differ
// from run to run in its last bits; the partials cost 2 * D floats per block of rows (1 / rows-per-block of the traffic).
#include <algorithm>

#include "common.h"

namespace {

using namespace tmdiff;

constexpr int kLnMaxD = 4096;

// out[j] = sum over p of part[p * cols + j] in a fixed order: a workgroup takes 32 columns, its eight 32-thread segments each
// add a contiguous eighth of the partials in order, thread by thread, and segment 0 adds the eight results in order.
// blockIdx.y selects dgamma (0) / dbeta (1), whose partials lie `second` floats apart.  An output that is not wanted is NULL.
__global__ void __launch_bounds__(256) col_sum_parts_kernel(const float* __restrict__ part, long second, long nparts, int cols,
                                                            float* __restrict__ out0, float* __restrict__ out1) {
  __shared__ float red[8][32];
  float* out = blockIdx.y ? out1 : out0;
  if (!out) return;      // (uniform)
  const int l = threadIdx.x & 31, seg = threadIdx.x >> 5, j = blockIdx.x * 32 + l;
  const long per = (nparts + 7) / 8, lo = seg * per, hi = min(lo + per, nparts);
  float s = 0.f;
  if (j < cols) {
    const float* p = part + (blockIdx.y ? second : 0) + j;
    for (long i = lo; i < hi; ++i) s += p[i * cols];
  }
  red[seg][l] = s;
  __syncthreads();
  if (seg == 0 && j < cols) {
    float t = red[0][l];
#pragma unroll
    for (int k = 1; k < 8; ++k) t += red[k][l];
    out[j] = t;
  }
}

// ---------------------------------------------------------------------------------------------------------
// LayerNorm.  NV = columns per lane (column lane + 64 i); rows of at most 1024 columns are held in registers between the
// reduction and the dx pass (x and dy are read once), longer ones are read again (the row has just been read: cache hits).
// Wave w of the workgroup takes rows r0 + w, r0 + w + 4, ... of its block of `rpb` rows.
// ---------------------------------------------------------------------------------------------------------
template <int NV>
__global__ void __launch_bounds__(256) layer_norm_bwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                             const float* __restrict__ dy, const float* __restrict__ mean,
                                                             const float* __restrict__ rstd, float* __restrict__ dx,
                                                             float* __restrict__ part, long rows, int D, int rpb) {
  constexpr bool kHold = NV <= 16;
  __shared__ float red[2][4][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long r0 = (long)blockIdx.x * rpb, r1 = min(r0 + rpb, rows);
  const float inv_d = 1.f / (float)D;
  float gam[NV], acc_g[NV], acc_b[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane + 64 * i;
    gam[i] = c < D ? gamma[c] : 0.f;
    acc_g[i] = acc_b[i] = 0.f;
  }
  for (long row = r0 + wv; row < r1; row += 4) {
    const float* xs = x + row * D;
    const float* gs = dy + row * D;
    const float mu = mean[row], rs = rstd[row];
    float xh[kHold ? NV : 1], gv[kHold ? NV : 1];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = lane + 64 * i;
      const bool ok = c < D;
      const float xhat = ok ? (xs[c] - mu) * rs : 0.f;
      const float d = ok ? gs[c] : 0.f;
      const float g = __fmul_rn(d, gam[i]);     // (a rounded product: g - mean(g) below must not fuse into an fma)
      s1 += g;
      s2 += g * xhat;
      acc_g[i] += d * xhat;
      acc_b[i] += d;
      if constexpr (kHold) xh[i] = xhat, gv[i] = g;
    }
    const float c1 = wave_sum(s1) * inv_d, c2 = wave_sum(s2) * inv_d;
    if (dx) {
      float* ds = dx + row * D;
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int c = lane + 64 * i;
        if (c < D) {
          float xhat, g;
          if constexpr (kHold) {
            xhat = xh[i], g = gv[i];
          } else {
            xhat = (xs[c] - mu) * rs, g = __fmul_rn(gs[c], gam[i]);
          }
          ds[c] = rs * ((g - c1) - xhat * c2);
        }
      }
    }
  }
  if (!part) return;     // (uniform: no parameter gradient is wanted)
  // partials of this block of rows: the four waves' column sums added in wave order
  float* pg = part + (long)blockIdx.x * D;
  float* pb = part + (long)gridDim.x * D + (long)blockIdx.x * D;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    if (64 * i >= D) break;
    __syncthreads();
    red[0][wv][lane] = acc_g[i];
    red[1][wv][lane] = acc_b[i];
    __syncthreads();
    const int c = lane + 64 * i;
    if (wv < 2 && c < D) {
      const float t = ((red[wv][0][lane] + red[wv][1][lane]) + red[wv][2][lane]) + red[wv][3][lane];
      (wv ? pb : pg)[c] = t;
    }
  }
}

// rows per workgroup: 8 (two per wave) up to 4096 rows, then as many as keep the grid at 512 blocks (a multiple of 4): two
// workgroups per CU, and at most 512 rows of partials for the second stage
int ln_rows_per_block(long rows) {
  const long rpb = (rows + 511) / 512;
  return rpb <= 8 ? 8 : (int)((rpb + 3) / 4 * 4);
}

bool ln_bwd_ok(long rows, int D) { return rows >= 0 && D >= 1 && D <= kLnMaxD && rows * (long)D < (1L << 31); }

// ---------------------------------------------------------------------------------------------------------
// GroupNorm.  x / dy [B, C, P]; the group of a workgroup is one contiguous run of cpg * P elements.
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void block_sum2(float& a, float& b, float (*red)[4]) {
  a = wave_sum(a);
  b = wave_sum(b);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[0][threadIdx.x >> 6] = a, red[1][threadIdx.x >> 6] = b;
  __syncthreads();
  a = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
  b = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
}

__global__ void __launch_bounds__(256) group_norm_bwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                             const float* __restrict__ dy, const float* __restrict__ mean,
                                                             const float* __restrict__ rstd, float* __restrict__ dx,
                                                             float* __restrict__ part, int B, int C, long P, int groups) {
  __shared__ float red[2][4];
  const int g = blockIdx.x, b = blockIdx.y, cpg = C / groups;
  const long n = (long)cpg * P, base = ((long)b * C + (long)g * cpg) * P;
  const float* xs = x + base;
  const float* gs = dy + base;
  const float mu = mean[(long)b * groups + g], rs = rstd[(long)b * groups + g];
  float G1 = 0.f, G2 = 0.f;      // sum of dy * gamma and of dy * gamma * xhat over the group (the same in every thread)
  for (int cc = 0; cc < cpg; ++cc) {
    const int c = g * cpg + cc;
    const float* xc = xs + (long)cc * P;
    const float* gc = gs + (long)cc * P;
    float s1 = 0.f, s2 = 0.f;
    for (long i = threadIdx.x; i < P; i += 256) {
      const float d = gc[i];
      s1 += d;
      s2 += d * ((xc[i] - mu) * rs);
    }
    block_sum2(s1, s2, red);
    if (part && threadIdx.x == 0) {
      part[(long)b * C + c] = s2;                    // dgamma partial of sample b
      part[(long)B * C + (long)b * C + c] = s1;      // dbeta partial
    }
    const float gm = gamma ? gamma[c] : 1.f;
    G1 += __fmul_rn(gm, s1);
    G2 += __fmul_rn(gm, s2);
  }
  if (!dx) return;
  const float inv_n = 1.f / (float)n;
  const float m1 = G1 * inv_n, m2 = G2 * inv_n;
  float* ds = dx + base;
  for (int cc = 0; cc < cpg; ++cc) {
    const float gm = gamma ? gamma[g * cpg + cc] : 1.f;
    const long o = (long)cc * P;
    for (long i = threadIdx.x; i < P; i += 256) {
      const float xhat = (xs[o + i] - mu) * rs;
      const float t = __fmul_rn(gm, gs[o + i]);     // (rounded: t - m1 must not fuse into an fma, see the n = 1 group)
      ds[o + i] = rs * ((t - m1) - xhat * m2);
    }
  }
}

bool gn_bwd_ok(int B, int C, long P, int groups) {
  return B >= 1 && B <= 65535 && C >= 1 && P >= 1 && groups >= 1 && C % groups == 0 && (long)B * C < (1L << 31) &&
         P < (1L << 31) && (long)B * C * P < (1L << 31);
}

// ---------------------------------------------------------------------------------------------------------
// GEGLU / GELU.  gelu(t) = t Phi(t) with the exact erf form of the forward; gelu'(t) = Phi(t) + t phi(t).
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float gelu_f(float t) { return 0.5f * t * (1.f + erff(t * 0.70710678118654752440f)); }
__device__ __forceinline__ float gelu_grad_f(float t) {
  const float Phi = 0.5f * (1.f + erff(t * 0.70710678118654752440f));
  const float phi = 0.39894228040143267794f * expf(-0.5f * t * t);
  return Phi + t * phi;
}

// V = 4: one float4 of a row per thread (inner % 4 == 0, 16-byte aligned tensors); V = 1: one element.
template <int V>
__global__ void __launch_bounds__(256) geglu_bwd_kernel(const float* __restrict__ u, const float* __restrict__ dy,
                                                        float* __restrict__ du, long rows, int inner, int gelu_only) {
  const int per_row = inner / V;
  const long total = rows * per_row;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long r = i / per_row;
    const int j = (int)(i % per_row) * V;
    const long og = gelu_only ? r * inner + j : r * 2 * inner + inner + j;   // the gate, and where its gradient goes
    float gate[V], d[V], a[V], da[V], dg[V];
    if constexpr (V == 4) {
      const float4 t = *reinterpret_cast<const float4*>(u + og), e = *reinterpret_cast<const float4*>(dy + r * inner + j);
      gate[0] = t.x, gate[1] = t.y, gate[2] = t.z, gate[3] = t.w;
      d[0] = e.x, d[1] = e.y, d[2] = e.z, d[3] = e.w;
      if (!gelu_only) {
        const float4 s = *reinterpret_cast<const float4*>(u + r * 2 * inner + j);
        a[0] = s.x, a[1] = s.y, a[2] = s.z, a[3] = s.w;
      }
    } else {
      gate[0] = u[og], d[0] = dy[r * inner + j];
      if (!gelu_only) a[0] = u[r * 2 * inner + j];
    }
#pragma unroll
    for (int k = 0; k < V; ++k) {
      if (gelu_only) {
        dg[k] = d[k] * gelu_grad_f(gate[k]);
      } else {
        da[k] = d[k] * gelu_f(gate[k]);
        dg[k] = d[k] * a[k] * gelu_grad_f(gate[k]);
      }
    }
    if constexpr (V == 4) {
      *reinterpret_cast<float4*>(du + og) = make_float4(dg[0], dg[1], dg[2], dg[3]);
      if (!gelu_only) *reinterpret_cast<float4*>(du + r * 2 * inner + j) = make_float4(da[0], da[1], da[2], da[3]);
    } else {
      du[og] = dg[0];
      if (!gelu_only) du[r * 2 * inner + j] = da[0];
    }
  }
}

}  // namespace

extern "C" int tmdiff_layer_norm_bwd_supported(int64_t rows, int32_t D) { return ln_bwd_ok(rows, D) ? 1 : 0; }

extern "C" size_t tmdiff_layer_norm_bwd_workspace_bytes(int64_t rows, int32_t D) {
  if (!ln_bwd_ok(rows, D) || rows == 0) return 0;
  const int rpb = ln_rows_per_block(rows);
  return (size_t)((rows + rpb - 1) / rpb) * 2 * D * sizeof(float);
}

extern "C" int tmdiff_layer_norm_bwd(const float* x, const float* gamma, const float* dy, const float* mean, const float* rstd,
                                     float* dx, float* dgamma, float* dbeta, void* workspace, int64_t rows, int32_t D,
                                     tmdiff_stream_t stream) {
  using namespace tmdiff;
  if (!ln_bwd_ok(rows, D)) return fail(TMDIFF_E_UNSUPPORTED, "layer_norm_bwd: rows=%ld D=%d (1 <= D <= 4096, rows * D < 2^31)", (long)rows, D);
  const bool params = dgamma || dbeta;
  hipStream_t st = as_stream(stream);
  if (rows > 0) {
    TMDIFF_REQUIRE(x && gamma && dy && mean && rstd && (!params || workspace), "layer_norm_bwd: NULL pointer");
    const int rpb = ln_rows_per_block(rows);
    const unsigned blocks = (unsigned)((rows + rpb - 1) / rpb);
    float* part = params ? static_cast<float*>(workspace) : nullptr;
#define TMDIFF_LN_BWD(NV) layer_norm_bwd_kernel<NV><<<blocks, 256, 0, st>>>(x, gamma, dy, mean, rstd, dx, part, rows, D, rpb)
    if (D <= 64) TMDIFF_LN_BWD(1);
    else if (D <= 128) TMDIFF_LN_BWD(2);
    else if (D <= 256) TMDIFF_LN_BWD(4);
    else if (D <= 512) TMDIFF_LN_BWD(8);
    else if (D <= 1024) TMDIFF_LN_BWD(16);
    else if (D <= 2048) TMDIFF_LN_BWD(32);
    else TMDIFF_LN_BWD(64);
#undef TMDIFF_LN_BWD
    if (const int rc = check_launch("layer_norm_bwd")) return rc;
    if (!params) return TMDIFF_OK;
    col_sum_parts_kernel<<<dim3((D + 31) / 32, 2), 256, 0, st>>>(part, (long)blocks * D, blocks, D, dgamma, dbeta);
    return check_launch("layer_norm_bwd(sum)");
  }
  if (!params) return TMDIFF_OK;     // no rows: the sums over them are 0
  col_sum_parts_kernel<<<dim3((D + 31) / 32, 2), 256, 0, st>>>(nullptr, 0, 0, D, dgamma, dbeta);
  return check_launch("layer_norm_bwd(sum)");
}

extern "C" int tmdiff_group_norm_bwd_supported(int32_t B, int32_t C, int64_t P, int32_t groups) {
  return gn_bwd_ok(B, C, P, groups) ? 1 : 0;
}

extern "C" size_t tmdiff_group_norm_bwd_workspace_bytes(int32_t B, int32_t C, int64_t P, int32_t groups) {
  return gn_bwd_ok(B, C, P, groups) ? (size_t)B * C * 2 * sizeof(float) : 0;
}

extern "C" int tmdiff_group_norm_bwd(const float* x, const float* gamma, const float* dy, const float* mean, const float* rstd,
                                     float* dx, float* dgamma, float* dbeta, void* workspace, int32_t B, int32_t C, int64_t P,
                                     int32_t groups, tmdiff_stream_t stream) {
  using namespace tmdiff;
  if (!gn_bwd_ok(B, C, P, groups))
    return fail(TMDIFF_E_UNSUPPORTED, "group_norm_bwd: B=%d C=%d P=%ld groups=%d (groups divides C, B <= 65535, B * C * P < 2^31)", B,
                C, (long)P, groups);
  const bool params = dgamma || dbeta;
  TMDIFF_REQUIRE(x && dy && mean && rstd && (!params || workspace), "group_norm_bwd: NULL pointer");
  if (!dx && !params) return TMDIFF_OK;
  hipStream_t st = as_stream(stream);
  float* part = params ? static_cast<float*>(workspace) : nullptr;
  group_norm_bwd_kernel<<<dim3(groups, B), 256, 0, st>>>(x, gamma, dy, mean, rstd, dx, part, B, C, P, groups);
  if (const int rc = check_launch("group_norm_bwd")) return rc;
  if (!params) return TMDIFF_OK;
  col_sum_parts_kernel<<<dim3((C + 31) / 32, 2), 256, 0, st>>>(part, (long)B * C, B, C, dgamma, dbeta);
  return check_launch("group_norm_bwd(sum)");
}

extern "C" int tmdiff_geglu_bwd(const float* u, const float* dy, float* du, int64_t rows, int32_t inner, int32_t gelu_only,
                                tmdiff_stream_t stream) {
  using namespace tmdiff;
  TMDIFF_REQUIRE(rows >= 0 && inner > 0, "geglu_bwd: bad arguments (rows=%ld inner=%d)", (long)rows, inner);
  if (rows == 0) return TMDIFF_OK;   // (empty tensors have no storage: NULL is fine)
  TMDIFF_REQUIRE(u && dy && du, "geglu_bwd: NULL pointer");
  const bool vec = inner % 4 == 0 && aligned16(u) && aligned16(dy) && aligned16(du);
  const long total = rows * (long)(vec ? inner / 4 : inner);
  const unsigned blocks = (unsigned)std::min<long>((total + 255) / 256, 1L << 20);
  if (vec) geglu_bwd_kernel<4><<<blocks, 256, 0, as_stream(stream)>>>(u, dy, du, rows, inner, gelu_only);
  else geglu_bwd_kernel<1><<<blocks, 256, 0, as_stream(stream)>>>(u, dy, du, rows, inner, gelu_only);
  return check_launch("geglu_bwd");
}
