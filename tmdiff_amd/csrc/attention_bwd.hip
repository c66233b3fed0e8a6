// Backward of the attention core (attention.hip: softmax(Q K^T * scale [key mask]) V) on gfx950, fp32 MFMA
// (v_mfma_f32_32x32x2_f32), no atomics: every output element is summed by one wave in a fixed order.
//   attn_delta_kernel  : Delta[b, h, q] = sum_d dO[q, d] O[q, d] into the caller's workspace (one thread per query row)
//   attn_bwd_dkv_kernel: one workgroup per 128 keys (a wave per 32); it walks the query tiles and keeps dK^T, dV^T in registers
//   attn_bwd_dq_kernel : one workgroup per 128 queries (a wave per 32); it walks the key tiles and keeps dQ^T in registers
// Both re-form P = exp(S - LSE) from the statistics tmdiff_attn_fwd_lse stored, with S summed exactly as the forward sums it
// (queries pre-scaled, head dim in ascending pairs), so P differs from the forward's only by the rounding of LSE and exp.
//
// Layout: as in the forward, the first product of a kernel is oriented so that the later ones sum over its REGISTER index and
// take it from the accumulator without any lane movement.  The dQ kernel forms S^T[key, query] = K Q^T and dP^T = V dO^T: a
// lane owns one query (its LSE and Delta are two scalars), its 16 registers are 16 keys, and dQ^T[d, query] += K^T dS^T reads
// dS^T from those registers.  The dK/dV kernel forms S[query, key] = Q K^T and dP = dO V^T: a lane owns one key (its K and V
// rows are its MFMA operands for the whole walk, in registers), its registers are 16 queries, and dV^T[d, key] += dO^T P,
// dK^T[d, key] += (scale Q)^T dS sum over them.  Register r of half-wave h is row (r&3) + 8(r>>2) + 4h.
//
// Masked keys score -FLT_MAX in the forward (the reference's masked_fill): here their P is 0, exactly, so their dK / dV rows
// are.  A sample whose keys are ALL masked has LSE == -FLT_MAX (log Nk is lost in the rounding); its P is 1/Nk on every key
// and its dS is 0, because masked_fill passes no gradient to the scores.
#include "common.h"

namespace {

using namespace tmdiff;

constexpr float kMaskFill = -3.4028234e38f;

struct AttnBwdArgs {
  const float* q; const float* k; const float* v; const float* o; const float* dout; const float* lse;
  const unsigned char* mask;  // [B, Nk] key mask (1 = keep) or NULL
  float* dq; float* dk; float* dv;   // each may be NULL: not wanted
  float* delta;               // workspace [B, H, Nq]
  long q_bs, q_hs, q_rs, k_bs, k_hs, k_rs, v_bs, v_hs, v_rs, o_bs, o_hs, o_rs;   // batch / head / row strides (elements)
  int H, Nq, Nk, D;
  float scale;
};

__device__ __forceinline__ int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// rows [r0, r0 + R) of a strided [n, D] matrix -> dst[R][DP] (row stride KS), times `mul`; rows at or beyond n and columns at or
// beyond D are zero-filled (no address is formed for them)
template <int R, int DP, int KS>
__device__ __forceinline__ void stage_rows(float* dst, const float* src, long rs, int r0, int n, int D, float mul, int tid) {
  for (int e = tid; e < R * DP; e += 256) {
    const int r = e / DP, c = e % DP;
    dst[r * KS + c] = (r0 + r < n && c < D) ? src[(long)(r0 + r) * rs + c] * mul : 0.f;
  }
}

// this lane's row of a staged [..][KS] tile, elements 2j + h, as MFMA operands in registers
template <int DP, int KS>
__device__ __forceinline__ void row_to_regs(float (&reg)[DP / 2], const float* row_h) {
#pragma unroll
  for (int j = 0; j < DP / 2; ++j) reg[j] = row_h[2 * j];
}

// acc^T tiles [DT][32 d][32 rows of this wave] -> ot[row][d] (the wave's 32 rows of a [..][KS] image), times `mul`
template <int DT, int KS>
__device__ __forceinline__ void acc_to_lds(float* ot, const f32x16 (&acc)[DT], float mul, int l31, int h) {
#pragma unroll
  for (int t = 0; t < DT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) ot[l31 * KS + t * 32 + acc_row(r, h)] = acc[t][r] * mul;
}

template <int DP, int KS>
__device__ __forceinline__ void store_rows(float* dst, long rs, const float* src, int r0, int n, int D, int tid) {
  for (int e = tid; e < 128 * DP; e += 256) {
    const int r = e / DP, c = e % DP;
    if (r0 + r < n && c < D) dst[(long)(r0 + r) * rs + c] = src[r * KS + c];
  }
}

// One thread per query row, and a fused-multiply-add chain over d in ascending order from 0: the order in which the MFMA sums
// dP = dO V^T.  With a single key (O == V, P == 1) Delta therefore equals dP bit for bit and dS = P (dP - Delta) is exactly 0, as
// it is in exact arithmetic; a tree reduction over the lanes would leave rounding noise where the true gradient is 0.
__global__ void __launch_bounds__(256) attn_delta_kernel(const AttnBwdArgs a, const long rows) {
  const long row = blockIdx.x * 256L + threadIdx.x;
  if (row >= rows) return;
  const long bh = row / a.Nq;
  const int qi = (int)(row % a.Nq), b = (int)(bh / a.H), hd = (int)(bh % a.H);
  const long off = b * a.o_bs + hd * a.o_hs + (long)qi * a.o_rs;
  float s = 0.f;
  for (int d = 0; d < a.D; ++d) s = fmaf(a.dout[off + d], a.o[off + d], s);
  a.delta[row] = s;
}

// ---------------------------------------------------------------------------------------------------------
// dQ[q, d] = scale * sum_key dS[q, key] K[key, d].  128 queries per workgroup; Q (pre-scaled) and dO rows of a lane's query
// live in registers, K / V tiles of 32 keys are staged in LDS once per workgroup and tile.  The 128-row buffer that stages Q
// and dO in the prologue holds the K / V tiles during the walk and the dQ transpose at the end.
// ---------------------------------------------------------------------------------------------------------
template <int DT>  // DT = ceil(D / 32)
__global__ void __launch_bounds__(256) attn_bwd_dq_kernel(const AttnBwdArgs a) {
  constexpr int DP = DT * 32, KS = DP + 1;
  __shared__ float lds[128 * KS + 32];
  float* const ks = lds;
  float* const vs = lds + 32 * KS;
  float* const kept = lds + 128 * KS;   // [32] of the current key tile: 1 = a kept key, 0 = masked / beyond Nk
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l31 = lane & 31, h = lane >> 5;
  const int bh = blockIdx.y, b = bh / a.H, hd = bh % a.H;
  const int q0 = blockIdx.x * 128;
  const float* kb = a.k + b * a.k_bs + hd * a.k_hs;
  const float* vb = a.v + b * a.v_bs + hd * a.v_hs;

  float qreg[DP / 2], greg[DP / 2];
  stage_rows<128, DP, KS>(lds, a.q + b * a.q_bs + hd * a.q_hs, a.q_rs, q0, a.Nq, a.D, a.scale, tid);
  __syncthreads();
  row_to_regs<DP, KS>(qreg, lds + (wv * 32 + l31) * KS + h);
  __syncthreads();
  stage_rows<128, DP, KS>(lds, a.dout + b * a.o_bs + hd * a.o_hs, a.o_rs, q0, a.Nq, a.D, 1.f, tid);
  __syncthreads();
  row_to_regs<DP, KS>(greg, lds + (wv * 32 + l31) * KS + h);
  const int qi = q0 + wv * 32 + l31;
  const bool qok = qi < a.Nq;
  const float lse = qok ? a.lse[(long)bh * a.Nq + qi] : 0.f;
  const float delta = qok ? a.delta[(long)bh * a.Nq + qi] : 0.f;
  const bool all_masked = lse == kMaskFill;

  f32x16 acc[DT];
#pragma unroll
  for (int t = 0; t < DT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  for (int k0 = 0; k0 < a.Nk; k0 += 32) {
    __syncthreads();
    stage_rows<32, DP, KS>(ks, kb, a.k_rs, k0, a.Nk, a.D, 1.f, tid);
    stage_rows<32, DP, KS>(vs, vb, a.v_rs, k0, a.Nk, a.D, 1.f, tid);
    if (tid < 32) kept[tid] = (k0 + tid < a.Nk && (!a.mask || a.mask[(long)b * a.Nk + k0 + tid] != 0)) ? 1.f : 0.f;
    __syncthreads();
    f32x16 s, dp;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f, dp[r] = 0.f;
    const float* krow = ks + l31 * KS + h;
    const float* vrow = vs + l31 * KS + h;
#pragma unroll
    for (int j = 0; j < DP / 2; ++j) s = __builtin_amdgcn_mfma_f32_32x32x2f32(krow[2 * j], qreg[j], s, 0, 0, 0);
#pragma unroll
    for (int j = 0; j < DP / 2; ++j) dp = __builtin_amdgcn_mfma_f32_32x32x2f32(vrow[2 * j], greg[j], dp, 0, 0, 0);
    // dS^T[key, query] = P (dP - Delta); all keys masked: no gradient reaches the scores
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float p = kept[acc_row(r, h)] != 0.f ? expf(s[r] - lse) : 0.f;
      s[r] = all_masked ? 0.f : p * (dp[r] - delta);
    }
    // dQ^T[d, query] += sum_key K[key, d] dS^T[key, query]
#pragma unroll
    for (int t = 0; t < DT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(ks[acc_row(r, h) * KS + t * 32 + l31], s[r], acc[t], 0, 0, 0);
  }
  __syncthreads();
  acc_to_lds<DT, KS>(lds + wv * 32 * KS, acc, a.scale, l31, h);
  __syncthreads();
  store_rows<DP, KS>(a.dq + b * a.q_bs + hd * a.q_hs, a.q_rs, lds, q0, a.Nq, a.D, tid);
}

// ---------------------------------------------------------------------------------------------------------
// dV[key, d] = sum_q P[q, key] dO[q, d], dK[key, d] = sum_q dS[q, key] (scale Q)[q, d].  128 keys per workgroup; the K and V
// rows of a lane's key live in registers, (pre-scaled) Q / dO tiles of 32 queries with their LSE and Delta are staged in LDS
// once per workgroup and tile.  A wave whose 32 keys all lie beyond Nk only helps staging.
// ---------------------------------------------------------------------------------------------------------
template <int DT>
__global__ void __launch_bounds__(256) attn_bwd_dkv_kernel(const AttnBwdArgs a) {
  constexpr int DP = DT * 32, KS = DP + 1;
  __shared__ float lds[128 * KS];
  float* const qs = lds;
  float* const gs = lds + 32 * KS;
  float* const lse_s = lds + 64 * KS;    // [32] of the current query tile
  float* const delta_s = lse_s + 32;     // [32]
  static_assert(64 * KS + 64 <= 128 * KS, "the tile buffers alias the 128-row staging / transpose buffer");
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int bh = blockIdx.y, b = bh / a.H, hd = bh % a.H;
  const int k0 = blockIdx.x * 128;
  const float* qb = a.q + b * a.q_bs + hd * a.q_hs;
  const float* gb = a.dout + b * a.o_bs + hd * a.o_hs;

  float kreg[DP / 2], vreg[DP / 2];
  stage_rows<128, DP, KS>(lds, a.k + b * a.k_bs + hd * a.k_hs, a.k_rs, k0, a.Nk, a.D, 1.f, tid);
  __syncthreads();
  row_to_regs<DP, KS>(kreg, lds + (wv * 32 + l31) * KS + h);
  __syncthreads();
  stage_rows<128, DP, KS>(lds, a.v + b * a.v_bs + hd * a.v_hs, a.v_rs, k0, a.Nk, a.D, 1.f, tid);
  __syncthreads();
  row_to_regs<DP, KS>(vreg, lds + (wv * 32 + l31) * KS + h);
  const int key = k0 + wv * 32 + l31;
  const bool key_ok = key < a.Nk;
  const bool key_kept = key_ok && (!a.mask || a.mask[(long)b * a.Nk + key] != 0);
  const bool wave_on = k0 + wv * 32 < a.Nk;   // (uniform)
  const float uniform_p = 1.f / (float)a.Nk;

  f32x16 dk[DT], dv[DT];
#pragma unroll
  for (int t = 0; t < DT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) dk[t][r] = 0.f, dv[t][r] = 0.f;

  for (int q0 = 0; q0 < a.Nq; q0 += 32) {
    __syncthreads();
    stage_rows<32, DP, KS>(qs, qb, a.q_rs, q0, a.Nq, a.D, a.scale, tid);
    stage_rows<32, DP, KS>(gs, gb, a.o_rs, q0, a.Nq, a.D, 1.f, tid);
    if (tid < 32) {
      const bool ok = q0 + tid < a.Nq;
      lse_s[tid] = ok ? a.lse[(long)bh * a.Nq + q0 + tid] : 0.f;
      delta_s[tid] = ok ? a.delta[(long)bh * a.Nq + q0 + tid] : 0.f;
    }
    __syncthreads();
    if (!wave_on) continue;
    f32x16 s, dp;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f, dp[r] = 0.f;
    const float* qrow = qs + l31 * KS + h;
    const float* grow = gs + l31 * KS + h;
#pragma unroll
    for (int j = 0; j < DP / 2; ++j) s = __builtin_amdgcn_mfma_f32_32x32x2f32(qrow[2 * j], kreg[j], s, 0, 0, 0);
#pragma unroll
    for (int j = 0; j < DP / 2; ++j) dp = __builtin_amdgcn_mfma_f32_32x32x2f32(grow[2 * j], vreg[j], dp, 0, 0, 0);
    // P[query, key] -> s, dS[query, key] -> dp; a query row at or beyond Nq contributes nothing
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ql = acc_row(r, h);
      const float lse = lse_s[ql];
      const bool all_masked = lse == kMaskFill;
      float p = all_masked ? (key_ok ? uniform_p : 0.f) : (key_kept ? expf(s[r] - lse) : 0.f);
      p = q0 + ql < a.Nq ? p : 0.f;
      s[r] = p;
      dp[r] = all_masked ? 0.f : p * (dp[r] - delta_s[ql]);
    }
#pragma unroll
    for (int t = 0; t < DT; ++t) {
#pragma unroll
      for (int r = 0; r < 16; ++r)
        dv[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(gs[acc_row(r, h) * KS + t * 32 + l31], s[r], dv[t], 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 16; ++r)
        dk[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(qs[acc_row(r, h) * KS + t * 32 + l31], dp[r], dk[t], 0, 0, 0);
    }
  }
  // the queries were pre-scaled, so dK already carries the factor `scale`
  if (a.dk) {
    __syncthreads();
    acc_to_lds<DT, KS>(lds + wv * 32 * KS, dk, 1.f, l31, h);
    __syncthreads();
    store_rows<DP, KS>(a.dk + b * a.k_bs + hd * a.k_hs, a.k_rs, lds, k0, a.Nk, a.D, tid);
  }
  if (a.dv) {
    __syncthreads();
    acc_to_lds<DT, KS>(lds + wv * 32 * KS, dv, 1.f, l31, h);
    __syncthreads();
    store_rows<DP, KS>(a.dv + b * a.v_bs + hd * a.v_hs, a.v_rs, lds, k0, a.Nk, a.D, tid);
  }
}

// extents the kernels take: see tmdiff_hip.h
bool attn_bwd_ok(long B, long H, long Nq, long Nk, long D) {
  if (B <= 0 || H <= 0 || Nq <= 0 || Nk <= 0 || D < 2 || D > 128 || D % 2 != 0 || B * H > 65535) return false;
  return B * H * Nq * D <= 0x7fffffffL && B * H * Nk * D <= 0x7fffffffL;
}

}  // namespace

extern "C" int tmdiff_attn_bwd_supported(int32_t B, int32_t H, int32_t Nq, int32_t Nk, int32_t D) {
  return attn_bwd_ok(B, H, Nq, Nk, D) ? 1 : 0;
}

extern "C" size_t tmdiff_attn_bwd_workspace_bytes(int32_t B, int32_t H, int32_t Nq, int32_t Nk, int32_t D) {
  return attn_bwd_ok(B, H, Nq, Nk, D) ? (size_t)B * H * Nq * sizeof(float) : 0;
}

extern "C" int tmdiff_attn_bwd(const float* q, const float* k, const float* v, const float* out, const float* dout,
                               const float* lse, const unsigned char* key_mask, float* dq, float* dk, float* dv, void* workspace,
                               int32_t B, int32_t H, int32_t Nq, int32_t Nk, int32_t D, const int64_t q_strides[3],
                               const int64_t k_strides[3], const int64_t v_strides[3], const int64_t o_strides[3], float scale,
                               tmdiff_stream_t stream) {
  using namespace tmdiff;
  TMDIFF_REQUIRE(B > 0 && H > 0 && Nq > 0 && Nk > 0, "attn_bwd: bad extents");
  TMDIFF_REQUIRE(D >= 2 && D <= 128 && D % 2 == 0, "attn_bwd: head dim %d (even, <= 128)", D);
  if (!attn_bwd_ok(B, H, Nq, Nk, D))
    return fail(TMDIFF_E_UNSUPPORTED, "attn_bwd: B*H = %ld (<= 65535), %ld / %ld elements (<= 2^31 - 1)", (long)B * H,
                (long)B * H * Nq * D, (long)B * H * Nk * D);
  TMDIFF_REQUIRE(q && k && v && out && dout && lse && workspace && q_strides && k_strides && v_strides && o_strides,
                 "attn_bwd: NULL pointer");
  if (!dq && !dk && !dv) return TMDIFF_OK;
  AttnBwdArgs a;
  a.q = q; a.k = k; a.v = v; a.o = out; a.dout = dout; a.lse = lse; a.mask = key_mask;
  a.dq = dq; a.dk = dk; a.dv = dv; a.delta = static_cast<float*>(workspace);
  a.q_bs = q_strides[0]; a.q_hs = q_strides[1]; a.q_rs = q_strides[2];
  a.k_bs = k_strides[0]; a.k_hs = k_strides[1]; a.k_rs = k_strides[2];
  a.v_bs = v_strides[0]; a.v_hs = v_strides[1]; a.v_rs = v_strides[2];
  a.o_bs = o_strides[0]; a.o_hs = o_strides[1]; a.o_rs = o_strides[2];
  a.H = H; a.Nq = Nq; a.Nk = Nk; a.D = D; a.scale = scale;
  hipStream_t st = as_stream(stream);
  const long rows = (long)B * H * Nq;
  attn_delta_kernel<<<(unsigned)((rows + 255) / 256), 256, 0, st>>>(a, rows);
  const dim3 gq((Nq + 127) / 128, B * H), gk((Nk + 127) / 128, B * H);
  const int dt = (D + 31) / 32;
  if (dq) {
    switch (dt) {
      case 1: attn_bwd_dq_kernel<1><<<gq, 256, 0, st>>>(a); break;
      case 2: attn_bwd_dq_kernel<2><<<gq, 256, 0, st>>>(a); break;
      case 3: attn_bwd_dq_kernel<3><<<gq, 256, 0, st>>>(a); break;
      default: attn_bwd_dq_kernel<4><<<gq, 256, 0, st>>>(a); break;
    }
  }
  if (dk || dv) {
    switch (dt) {
      case 1: attn_bwd_dkv_kernel<1><<<gk, 256, 0, st>>>(a); break;
      case 2: attn_bwd_dkv_kernel<2><<<gk, 256, 0, st>>>(a); break;
      case 3: attn_bwd_dkv_kernel<3><<<gk, 256, 0, st>>>(a); break;
      default: attn_bwd_dkv_kernel<4><<<gk, 256, 0, st>>>(a); break;
    }
  }
  return check_launch("attn_bwd");
}
