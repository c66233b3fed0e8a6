// BDSD pansharpening on gfx950 (host definitions: tmdiff_amd/metrics.py, bdsd_moments / bdsd_coeffs / bdsd_inject / bdsd): the
// normal equations of the band-dependent regression per image block at the reduced scale, their solution, and the injection of a
// different linear combination of all bands and the PAN into every band.  Nothing is read on the host, nothing is allocated, no
// atomics: the same bits on every run and in a graph replay.
//
//  BLOCKS                An image of h x w pixels is cut into nby x nbx non-overlapping blocks of by x bx pixels (the whole image
//                        is one block of h x w); block (iy, ix) has the index iy nbx + ix, and its pixels are numbered in row-major
//                        order, q = row bx + col.
//  bdsd_gram_kernel      The regressors of a block are its C low-pass bands and the reduced PAN: C + 1 <= 16 rows Hm of a 16 x 16
//                        tile; the targets are D_c = low_ms_c - low_lp_c, formed in fp64 after the loads (exact).  One workgroup
//                        of 256 takes a chunk of BG_PIX consecutive pixels q of one block of one image, in steps of 16 pixels;
//                        wave w takes the steps w, w + 4, w + 8, ... of the chunk.  In a step, lane l holds regressor p = l & 15
//                        and target p at the four pixels step + 4 (l >> 4) + e, e = 0 .. 3 (one 16-byte load per plane where the
//                        four lie in one row at an aligned address -- bx % 4 == 0, w % 4 == 0, aligned bases -- else four scalar
//                        loads with the same values); 0.0 on rows past the last regressor / target and on pixels past the end.
//                        For each e it issues v_mfma_f64_16x16x4_f64 twice with the regressor register as A: once with the same
//                        register as B (N += Hm' Hm) and once with the target register as B (R += Hm' D); instruction e adds the
//                        products at the pixels step + 4 k + e, k = 0 .. 3 being the instruction's K index.  The two tiles'
//                        layout: classical.h.
//  SUMMATION ORDER of one entry of N or R: inside a wave one accumulator chain over its steps in ascending order and e ascending
//                        inside a step; the four waves' tiles through LDS in ascending wave index (waves_in_order, stats.h); the
//                        chunk's entries go to the workspace; bdsd_gram_finalize_kernel, one workgroup per (image, block) with
//                        lane t owning entry t, adds the chunks in ascending order (strided_sum, stats.h) and writes N | R with
//                        N's upper triangle mirrored: exactly symmetric.
//  WHY THE MATRIX PIPE   The layout of plane_gram_kernel (cs_fusion.hip) extends directly: the second product shares the A operand,
//                        so the targets cost one more instruction per e and no further loads of the regressors.
//  bdsd_solve_kernel     one wave per (image, block); lane 0 factors N once (ldl_factor, classical.h) and solves per column of R
//                        (ldl_solve).  A pivot that is not positive: NaN for that block.
//  bdsd_inject_kernel<C> A workgroup's tile is 1024 consecutive pixels q of one full-scale block, so one set of weights serves it:
//                        the block's (C + 1) x C weights go to LDS (at most 1920 bytes).  A lane owns four consecutive q, reads
//                        all C bands and the PAN of them into fp32 registers before it writes anything (`out` may be ms_exp),
//                        and evaluates per band one fp64 chain  acc = M_c;  acc = fma(gamma[k][c], M_k, acc), k = 0 .. C - 1;
//                        acc = fma(gamma[C][c], P, acc), rounded to fp32 once.  Quads (classical.h) as 16-byte accesses where the
//                        four pixels lie in one row at an aligned address (block width % 4 == 0, W % 4 == 0, aligned bases).
//                        Traffic: 2 C + 1 planes.
#include "classical.h"

namespace {

constexpr int BDSD_MAXC = 15;
constexpr int BG_PIX = 4096;                    // pixels of a workgroup's chunk
constexpr int BG_STEPS = BG_PIX / 16 / 4;       // steps of 16 pixels per wave

// (by, bx) of a block: the whole image with bs == 0.  False when bs does not tile the image.
inline bool bdsd_sides(int h, int w, int bs, int& by, int& bx) {
  by = bs ? bs : h;
  bx = bs ? bs : w;
  return bs >= 0 && by >= 1 && bx >= 1 && h % by == 0 && w % bx == 0;
}
inline bool bdsd_ok(int B, int C, int H, int W, int bs) {
  int by, bx;
  return tmdiff::planes_ok(B, C, BDSD_MAXC, H, W) && bdsd_sides(H, W, bs, by, bx);
}
inline int bdsd_entries(int C) { return (C + 1) * (2 * C + 1); }
inline int bdsd_chunks(long n) { return (int)((n + BG_PIX - 1) / BG_PIX); }
inline size_t bdsd_gram_bytes(int B, int C, int h, int w, int bs) {
  int by, bx;
  bdsd_sides(h, w, bs, by, bx);
  return (size_t)B * (h / by) * (w / bx) * bdsd_chunks((long)by * bx) * bdsd_entries(C) * sizeof(double);
}

struct BdsdGramArgs {
  const float* lp;    // [B, C, h, w]
  const float* pan;   // [B, h, w]
  const float* ms;    // [B, C, h, w]
  int B, C, h, w, by, bx, nbx, nblk, chunks, vec;
  double* part;       // [B, nblk, chunks, (C + 1) (2 C + 1)]
  double* out;        // [B, nblk, C + 1, 2 C + 1]
};

// The lane's four values of `plane` (null: zeros) at the pixels q .. q + 3 of the block whose first pixel is plane[org]; 0 past the
// block's n pixels.
__device__ __forceinline__ void bdsd_load(const float* plane, int org, long q, int n, int bx, int w, bool vec, float (&v)[4]) {
  if (plane && vec && q < n) {                                    // bx % 4 == 0 here: the four lie inside one row together
    *reinterpret_cast<float4*>(v) = *reinterpret_cast<const float4*>(plane + tmdiff::block_offset(org, q, n, bx, w));
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = plane && q + e < n ? plane[tmdiff::block_offset(org, q + e, n, bx, w)] : 0.f;
  }
}

__global__ void __launch_bounds__(256) bdsd_gram_kernel(BdsdGramArgs a) {
  __shared__ double red[4 * 512];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), p = lane & 15;
  const int blk = blockIdx.x / a.chunks, chunk = blockIdx.x - blk * a.chunks;
  const int org = (blk / a.nbx) * a.by * a.w + (blk % a.nbx) * a.bx, n = a.by * a.bx;
  const int k1 = a.C + 1, ld = 2 * a.C + 1;
  const long plane = (long)a.h * a.w;
  for (int b = blockIdx.y; b < a.B; b += gridDim.y) {
    const float* reg = p < a.C ? a.lp + ((long)b * a.C + p) * plane : p == a.C ? a.pan + (long)b * plane : nullptr;
    const float* raw = p < a.C ? a.ms + ((long)b * a.C + p) * plane : nullptr;
    tmdiff::gram_tile accn = {0.0, 0.0, 0.0, 0.0}, accr = {0.0, 0.0, 0.0, 0.0};
    // the wave's steps that begin inside the block: the same count in every lane of the wave
    const long left = (long)n - (long)chunk * BG_PIX - 16 * wave;
    const int steps = left <= 0 ? 0 : (int)min((long)BG_STEPS, (left + 63) / 64);
    for (int i = 0; i < steps; ++i) {
      const long q0 = (long)chunk * BG_PIX + 16 * (wave + 4 * i);
      float hv[4], mv[4];
      bdsd_load(reg, org, q0 + 4 * (lane >> 4), n, a.bx, a.w, a.vec, hv);
      bdsd_load(raw, org, q0 + 4 * (lane >> 4), n, a.bx, a.w, a.vec, mv);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double x = (double)hv[e], d = raw ? (double)mv[e] - x : 0.0;
        accn = __builtin_amdgcn_mfma_f64_16x16x4f64(x, x, accn, 0, 0, 0);
        accr = __builtin_amdgcn_mfma_f64_16x16x4f64(x, d, accr, 0, 0, 0);
      }
    }
    __syncthreads();                                              // the image before may still read red
    tmdiff::store_gram_tile<512>(red, wave, 0, lane, accn);
    tmdiff::store_gram_tile<512>(red, wave, 256, lane, accr);
    __syncthreads();
    const int row = threadIdx.x >> 4, col = threadIdx.x & 15;
    double* dst = a.part + (((long)b * a.nblk + blk) * a.chunks + chunk) * (k1 * ld) + row * ld;
    if (row < k1 && col < k1) dst[col] = tmdiff::waves_in_order<512>(red, threadIdx.x, 0, 4);
    if (row < k1 && col < a.C) dst[k1 + col] = tmdiff::waves_in_order<512>(red, 256 + threadIdx.x, 0, 4);
  }
}

__global__ void __launch_bounds__(512) bdsd_gram_finalize_kernel(BdsdGramArgs a) {
  __shared__ double g[512];
  const int t = threadIdx.x, k1 = a.C + 1, ld = 2 * a.C + 1, entries = k1 * ld;
  const int row = t / ld, col = t - row * ld;
  const long systems = (long)a.B * a.nblk;
  for (long s = blockIdx.x; s < systems; s += gridDim.x) {
    __syncthreads();                                              // the block before may still read g
    if (t < entries) g[t] = tmdiff::strided_sum(a.part + s * a.chunks * entries + t, a.chunks, entries, 0, 1);
    __syncthreads();
    if (t < entries) a.out[s * entries + t] = col < k1 ? g[min(row, col) * ld + max(row, col)] : g[t];
  }
}

// ---- the weights --------------------------------------------------------------------------------------------------------------
struct BdsdSolveArgs {
  const double* mo;     // [systems, C + 1, 2 C + 1]
  double* out;          // [systems, C + 1, C]
  int systems, C;
};

__global__ void __launch_bounds__(64) bdsd_solve_kernel(BdsdSolveArgs a) {
  constexpr int K = BDSD_MAXC + 1;
  __shared__ double fac[K * K], piv[K], z[K], gam[K];
  if (threadIdx.x != 0) return;
  const int C = a.C, k1 = C + 1, ld = 2 * C + 1;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  for (int s = blockIdx.x; s < a.systems; s += gridDim.x) {
    const double* mo = a.mo + (long)s * k1 * ld;
    double* out = a.out + (long)s * k1 * C;
    const bool bad = tmdiff::ldl_factor<K>(mo, ld, k1, fac, piv);
    for (int col = 0; col < C; ++col) {                           // N gamma_c = R_c, column k1 + col of mo
      tmdiff::ldl_solve<K>(mo + k1 + col, ld, k1, fac, piv, z, gam);
      for (int i = 0; i < k1; ++i) out[i * C + col] = bad ? nan : gam[i];
    }
  }
}

// ---- the injection ------------------------------------------------------------------------------------------------------------
struct BdsdInjectArgs {
  const float* m;       // ms_exp [B, C, H, W]
  const float* p;       // pan    [B, H, W]
  const double* gamma;  // [B, nblk, C + 1, C]
  float* out;           // [B, C, H, W]; may be m
  int B, H, W, bh, bw, nbx, nblk, tiles, vec;
};

template <int C>
__global__ void __launch_bounds__(256) bdsd_inject_kernel(BdsdInjectArgs a) {
  __shared__ double wt[(C + 1) * C];
  const int blk = blockIdx.x / a.tiles, tile = blockIdx.x - blk * a.tiles;
  const int org = (blk / a.nbx) * a.bh * a.W + (blk % a.nbx) * a.bw, n = a.bh * a.bw;
  const long q = ((long)tile * 256 + threadIdx.x) * 4;
  const long plane = (long)a.H * a.W;
  int off[4];                                   // a pixel past the block's end is never accessed: its offset is the block's last
#pragma unroll
  for (int e = 0; e < 4; ++e) off[e] = tmdiff::block_offset(org, q + e, n, a.bw, a.W);
  const int cnt = (int)max((long)0, min((long)4, n - q));
  for (int b = blockIdx.y; b < a.B; b += gridDim.y) {
    __syncthreads();                            // the image before may still read wt
    if ((int)threadIdx.x < (C + 1) * C) wt[threadIdx.x] = a.gamma[((long)b * a.nblk + blk) * ((C + 1) * C) + threadIdx.x];
    __syncthreads();
    if (cnt == 0) continue;
    float pv[4], mv[C][4];
    tmdiff::load_quad(a.p + (long)b * plane, off, a.vec, cnt, pv);
#pragma unroll
    for (int c = 0; c < C; ++c) tmdiff::load_quad(a.m + ((long)b * C + c) * plane, off, a.vec, cnt, mv[c]);
#pragma unroll
    for (int c = 0; c < C; ++c) {
      double acc[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = (double)mv[c][e];
#pragma unroll
      for (int k = 0; k < C; ++k) {
        const double g = wt[k * C + c];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = fma(g, (double)mv[k][e], acc[e]);
      }
      const double gp = wt[C * C + c];
      float f[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) f[e] = (float)fma(gp, (double)pv[e], acc[e]);
      tmdiff::store_quad(a.out + ((long)b * C + c) * plane, off, a.vec, cnt, f);
    }
  }
}

const char* const BDSD_LIMITS = "B >= 0, 1 <= C <= 15, H, W >= 1, fewer than 2^31 elements; the block side 0 (the whole image) or a "
                                "divisor of H and W";

}  // namespace

extern "C" {

size_t tmdiff_bdsd_gram_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W, int32_t bs) {
  return bdsd_ok(B, C, H, W, bs) ? bdsd_gram_bytes(B, C, H, W, bs) : 0;
}

int tmdiff_bdsd_gram(const float* low_lp, const float* low_pan, const float* low_ms, int32_t B, int32_t C, int32_t H, int32_t W,
                     int32_t bs, double* out, void* workspace, size_t workspace_bytes, tmdiff_stream_t stream) {
  if (!bdsd_ok(B, C, H, W, bs))
    return tmdiff::fail(TMDIFF_E_UNSUPPORTED, "bdsd_gram: B=%d C=%d H=%d W=%d bs=%d (%s)", B, C, H, W, bs, BDSD_LIMITS);
  if (B == 0) return TMDIFF_OK;
  TMDIFF_REQUIRE(low_lp && low_pan && low_ms && out && workspace, "bdsd_gram: null tensor");
  TMDIFF_REQUIRE((reinterpret_cast<uintptr_t>(out) & 7u) == 0, "bdsd_gram: out must be 8-byte aligned");
  if (const int rc = tmdiff::check_workspace("bdsd_gram", workspace, workspace_bytes, bdsd_gram_bytes(B, C, H, W, bs))) return rc;
  int by, bx;
  bdsd_sides(H, W, bs, by, bx);
  const int nbx = W / bx, nblk = (H / by) * nbx, chunks = bdsd_chunks((long)by * bx);
  if (const int rc = tmdiff::check_grid((long)nblk * chunks, "bdsd_gram", TMDIFF_E_UNSUPPORTED)) return rc;
  const hipStream_t st = tmdiff::as_stream(stream);
  const int vec = bx % 4 == 0 && W % 4 == 0 && tmdiff::aligned16(low_lp) && tmdiff::aligned16(low_pan) && tmdiff::aligned16(low_ms);
  const BdsdGramArgs a{low_lp, low_pan, low_ms, B, C, H, W, by, bx, nbx, nblk, chunks, vec, static_cast<double*>(workspace), out};
  bdsd_gram_kernel<<<dim3((unsigned)(nblk * chunks), (unsigned)std::min(B, 65535)), 256, 0, st>>>(a);
  if (const int rc = tmdiff::check_launch("bdsd_gram")) return rc;
  bdsd_gram_finalize_kernel<<<dim3((unsigned)std::min((long)B * nblk, 1L << 20)), 512, 0, st>>>(a);
  return tmdiff::check_launch("bdsd_gram (finalize)");
}

int tmdiff_bdsd_solve(const double* moments, double* out, int32_t systems, int32_t C, tmdiff_stream_t stream) {
  if (systems < 0 || C < 1 || C > BDSD_MAXC)
    return tmdiff::fail(TMDIFF_E_UNSUPPORTED, "bdsd_solve: systems=%d C=%d (systems >= 0, 1 <= C <= 15)", systems, C);
  if (systems == 0) return TMDIFF_OK;
  TMDIFF_REQUIRE(moments && out, "bdsd_solve: null tensor");
  TMDIFF_REQUIRE(((reinterpret_cast<uintptr_t>(moments) | reinterpret_cast<uintptr_t>(out)) & 7u) == 0,
                 "bdsd_solve: tensors must be 8-byte aligned");
  const BdsdSolveArgs a{moments, out, systems, C};
  bdsd_solve_kernel<<<dim3((unsigned)std::min(systems, 1 << 20)), 64, 0, tmdiff::as_stream(stream)>>>(a);
  return tmdiff::check_launch("bdsd_solve");
}

int tmdiff_bdsd_inject(const float* ms_exp, const float* pan, const double* gamma, float* out, int32_t B, int32_t C, int32_t H,
                       int32_t W, int32_t block, tmdiff_stream_t stream) {
  if (!bdsd_ok(B, C, H, W, block))
    return tmdiff::fail(TMDIFF_E_UNSUPPORTED, "bdsd_inject: B=%d C=%d H=%d W=%d block=%d (%s)", B, C, H, W, block, BDSD_LIMITS);
  if (B == 0) return TMDIFF_OK;
  TMDIFF_REQUIRE(ms_exp && pan && gamma && out, "bdsd_inject: null tensor");
  TMDIFF_REQUIRE((reinterpret_cast<uintptr_t>(gamma) & 7u) == 0, "bdsd_inject: gamma must be 8-byte aligned");
  int bh, bw;
  bdsd_sides(H, W, block, bh, bw);
  const int nbx = W / bw, nblk = (H / bh) * nbx, tiles = (int)(((long)bh * bw + 1023) / 1024);
  if (const int rc = tmdiff::check_grid((long)nblk * tiles, "bdsd_inject", TMDIFF_E_UNSUPPORTED)) return rc;
  const int vec = bw % 4 == 0 && W % 4 == 0 && tmdiff::aligned16(ms_exp) && tmdiff::aligned16(pan) && tmdiff::aligned16(out);
  const BdsdInjectArgs a{ms_exp, pan, gamma, out, B, H, W, bh, bw, nbx, nblk, tiles, vec};
  const dim3 grid((unsigned)(nblk * tiles), (unsigned)std::min(B, 65535));
  const hipStream_t st = tmdiff::as_stream(stream);
  tmdiff::dispatch_bands<BDSD_MAXC>(C, [&](auto c) { bdsd_inject_kernel<decltype(c)::value><<<grid, 256, 0, st>>>(a); });
  return tmdiff::check_launch("bdsd_inject");
}

}  // extern "C"
