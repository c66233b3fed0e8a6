// 3x3x3 convolution with Winograd in TWO dimensions for the deep layers: F(4,3) along the bands (the forward's six planes,
// conv3d_wf.hip) times F(2,3) along the width (four planes) -- 24 planes, 72 multiply-adds per input channel, tile of four
// bands and column pair instead of conv3d_wf's 108.  Built the way wgrad_wino.hip is: the transforms are bandwidth passes over
// Winograd-domain arrays in HBM, the multiply is a plain GEMM per plane with nothing but MFMAs and operand reads in its loop,
// and a workgroup owns ONE plane, so the second dimension costs no accumulators.
//
//   U  [k = kb * 4 + kw][dh][Cin / 4][Cout][4]            (G_band (x) G_w) w, packed once per weight (w2_pack_kernel)
//   x^ [k][Cin / 4][Q * IP][4]                            (B^T_band (x) B^T_w) x' of image q = (b, band tile t), position
//                                                         (hp, tw) of the plane padded by one ZERO row above and below
//                                                         (IP = (H + 2) * W / 2); written whole by w2_input_kernel
//   m^ [k][Q * OP][Cout]                                  sum over the three row taps dh and Cin (OP = H * W / 2)
//   y  = (A^T_band (x) A^T_w) m^ + the epilogue           w2_output_kernel
//
// Channels stand innermost in QUADS, not in 128-byte runs as in wgrad_wino.hip: there the reduction runs over positions and
// a lane is a channel; here it runs over channels and a lane is a position (or an output channel), which in a
// [position][32 channels] image would put the 32 lanes of an operand read on one bank.  With [quad][position][4] one
// ds_read_b128 per lane is conflict-free, gives the operand of FOUR K-steps (lanes 0-31 take quad 2m, lanes 32-63 quad 2m + 1:
// the two K slots of v_mfma_f32_32x32x2_f32), a 16-byte LDS-DMA piece is 64 consecutive positions of one quad -- 1 KB
// contiguous in HBM -- and the three row taps read the SAME staged positions at offsets of one plane row.
#include "bufaddr.h"
#include "common.h"

namespace {

using namespace tmdiff;

constexpr int W2_XP = 384;   // padded positions a GEMM tile stages (whole images)
constexpr int W2_NP = 256;   // output positions of a GEMM tile: 4 waves x 2 blocks of 32
constexpr int W2_KC = 16;    // input channels per stage (four quads)
constexpr int W2_CO = 64;    // output channels per workgroup: 2 blocks of 32

struct W2Plan {
  int T, Q, TW, Hp, IP, OP;  // band tiles; images (b, t); column pairs; padded rows; padded / output positions per image
  int G, ptiles;             // images per GEMM tile; position tiles
  size_t xh_floats, mh_floats;
};

// the extents and the input side: what the input pass and the GEMM take, whatever the epilogue writes
bool w2_extents_ok(const tmdiff_conv3d_desc* d) {
  if (!d || d->ksize != 3 || d->groups != 1 || d->x_bf16 || d->y2_bf16 || d->nseg != 1) return false;
  if (d->B <= 0 || (d->N != 4 && d->N != 8) || d->W < 2 || d->W > 16 || d->W % 2 || d->H < 4 || d->H > 32) return false;
  if (d->Cin < 128 || d->Cin % 32 || d->Cout < 256 || d->Cout % W2_CO || d->seg_c[0] != d->Cin) return false;
  // what the passes do not do: mask / dropout on the input, the side x'
  if (d->in_mask || d->drop_p > 0.f || d->xp_out) return false;
  return true;
}

bool w2_folds(const tmdiff_conv3d_desc* d) { return d->rc_x || d->rc_w || d->rc_cin; }
bool w2_quarter(const tmdiff_conv3d_desc* d) { return d->y_ll || d->y_hi[0] || d->y_hi[1] || d->y_hi[2] || d->y2_s2d; }

// the plain y / y2 / residual epilogue (tmdiff_conv3d_w2_supported): the one-row output pass
bool w2_shape_ok(const tmdiff_conv3d_desc* d) { return w2_extents_ok(d) && !w2_folds(d) && !w2_quarter(d); }

// ... and the epilogues of the row-pair output pass on top (tmdiff_conv3d_w2_epilogue_supported): the folded 1x1x1 under
// conv3d_wf's conditions, the quarter-resolution outputs (LL, Haar, space-to-depth) on 8 bands; both on an even number of rows
bool w2_epilogue_ok(const tmdiff_conv3d_desc* d) {
  if (!w2_extents_ok(d)) return false;
  if (!w2_folds(d) && !w2_quarter(d)) return true;
  if (d->H % 2) return false;
  if (w2_quarter(d) && d->N != 8) return false;
  if (d->y_ll) {       // instead of y: beside a second output, or with the three high bands through its prologue
    const bool dwt = d->y_hi[0] != nullptr;
    if (d->y || (dwt ? (d->y2 || d->y2_s2d || !d->y_hi[1] || !d->y_hi[2]) : !d->y2)) return false;
  } else if (d->y_hi[0] || d->y_hi[1] || d->y_hi[2]) {
    return false;
  }
  if (d->y2_s2d && !d->y2) return false;
  if (w2_folds(d)) {
    if (!d->rc_x || d->rc_cin <= 0 || d->rc_cin % 32 || d->rc_cin > 512 || d->residual) return false;
    if ((long)d->rc_cin * d->N * d->H * d->W >= (1L << 30)) return false;      // (conv3d_wf's wf_rc_fits)
  }
  return true;
}

W2Plan w2_plan(const tmdiff_conv3d_desc* d) {
  W2Plan p;
  p.T = d->N / 4; p.Q = d->B * p.T; p.TW = d->W / 2; p.Hp = d->H + 2;
  p.IP = p.Hp * p.TW; p.OP = d->H * p.TW;
  p.G = W2_NP / p.OP < W2_XP / p.IP ? W2_NP / p.OP : W2_XP / p.IP;     // (H <= 32, W <= 16: at least one image fits)
  if (p.G > p.Q) p.G = p.Q;
  p.ptiles = (p.Q + p.G - 1) / p.G;
  p.xh_floats = (size_t)24 * d->Cin * p.Q * p.IP;
  p.mh_floats = (size_t)24 * d->Cout * p.Q * p.OP;
  return p;
}

bool w2_fits(const tmdiff_conv3d_desc* d, const W2Plan& p) {
  // 32-bit byte offsets inside one plane k of U, x^ and m^; grid limits of the passes; the output pass addresses 32 channels
  // of a sample through one descriptor
  // (32 channels at full resolution = the 128 of the space-to-depth form = four times the 32 of a quarter-size output)
  const size_t xk = p.xh_floats / 24 * 4, mk = p.mh_floats / 24 * 4, uk = (size_t)3 * d->Cin * d->Cout * 4;
  const size_t yk = (size_t)32 * d->N * d->H * d->W * 4;
  return xk < (1ull << 31) && mk < (1ull << 31) && uk < (1ull << 31) && yk < (1ull << 31) && p.Q <= 65535 &&
         (long)p.ptiles * (d->Cout / W2_CO) * 24 < 0x7fffffffL;
}

// ---------------------------------------------------------------------------------------------------------------------
// Weight pack: one thread per (dh, input channel, output channel).
// G_band = [1/4 0 0; -1/6 -1/6 -1/6; -1/6 1/6 -1/6; 1/24 1/12 1/6; 1/24 -1/12 1/6; 0 0 1],  G_w = [1 0 0; 1/2 1/2 1/2; 1/2 -1/2 1/2; 0 0 1]
// ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) w2_pack_kernel(const float* __restrict__ w, float* __restrict__ u, int Cout, int Cin) {
#pragma clang fp contract(off)   // (every product rounded before it is added: a fused multiply-add would carry the factors' rounding into the sums)
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)3 * Cin * Cout) return;
  const int e = idx & 3;
  long r = idx >> 2;
  const int co = r % Cout; r /= Cout;
  const int cq = r % (Cin / 4);
  const int dh = r / (Cin / 4);
  const int ci = cq * 4 + e;
  const float* src = w + ((long)co * Cin + ci) * 27 + dh * 3;      // [dn][dh][dw]
  float t[6][3];
#pragma unroll
  for (int dw = 0; dw < 3; ++dw) {
    const float g0 = src[dw], g1 = src[9 + dw], g2 = src[18 + dw];
    const float s02 = g0 + g2;
    const float ev = g0 + 4.f * g2, od = 2.f * g1;   // (sums first, ONE rounded factor: small-integer weights pack exactly)
    t[0][dw] = 0.25f * g0;
    t[1][dw] = (s02 + g1) * (-1.f / 6.f);
    t[2][dw] = (g1 - s02) * (1.f / 6.f);
    t[3][dw] = (ev + od) * (1.f / 24.f);
    t[4][dw] = (ev - od) * (1.f / 24.f);
    t[5][dw] = g2;
  }
  const long plane = (long)3 * Cin * Cout;
  float* dst = u + (((long)dh * (Cin / 4) + cq) * Cout + co) * 4 + e;
#pragma unroll
  for (int kb = 0; kb < 6; ++kb) {
    const float s02 = t[kb][0] + t[kb][2];
    dst[(kb * 4 + 0) * plane] = t[kb][0];
    dst[(kb * 4 + 1) * plane] = 0.5f * (s02 + t[kb][1]);
    dst[(kb * 4 + 2) * plane] = 0.5f * (s02 - t[kb][1]);
    dst[(kb * 4 + 3) * plane] = t[kb][2];
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Input pass.  One workgroup = one row hp of the padded plane of image q x 32 channels: thread (channel, column pair) loads
// the tile's six input bands of its pair (float2; the pair's left and right neighbour columns come from the neighbour
// lanes), applies the consumer's prologue, transforms along the bands (the shared-sum form of conv3d_wf) and along the
// width, the block turns round in LDS and leaves as 16-byte channel quads, TW consecutive positions per (plane, quad).
// The rows hp = 0 and H + 1 are the zero padding, written like every other row: nothing is cleared beforehand.
// ---------------------------------------------------------------------------------------------------------------------
struct W2InArgs {
  const float* x;
  float* xh;
  const float* in_shift;
  const float* in_scale;
  int shift_stride, scale_stride, in_act;
  int Cin, N, H, W, T, TW, IP;
  long QIP;
};

__global__ void __launch_bounds__(256) w2_input_kernel(const W2InArgs a) {
  __shared__ float tile[24 * 8 * 33];
  const int tid = threadIdx.x;
  const int cc = blockIdx.x, hp = blockIdx.y, q = blockIdx.z;
  const int b = q / a.T, t = q % a.T;
  const int h = hp - 1;
  {
    const int c = tid >> 3, tw = tid & 7;
    const int ch = cc * 32 + c;
    const long hw = (long)a.H * a.W;
    const bool ok = h >= 0 && h < a.H && tw < a.TW;
    const float sh = a.in_shift ? a.in_shift[(long)b * a.shift_stride + ch] : 0.f;
    const float sc = a.in_scale ? a.in_scale[(long)b * a.scale_stride + ch] : 1.f;
    const float* src = a.x + ((long)b * a.Cin + ch) * a.N * hw + (long)h * a.W + 2 * tw;
    float d[6][4];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      const int n = 4 * t - 1 + j;
      float2 v = make_float2(0.f, 0.f);
      if (ok && n >= 0 && n < a.N) {
        v = *reinterpret_cast<const float2*>(src + (long)n * hw);
        v.x += sh, v.y += sh;
        if (a.in_act) v.x = silu_f(v.x), v.y = silu_f(v.y);
        v.x *= sc, v.y *= sc;
      }
      const float left = __shfl_up(v.y, 1, 8), right = __shfl_down(v.x, 1, 8);   // (a lane past the plane holds zeros)
      d[j][0] = tw == 0 ? 0.f : left;
      d[j][1] = v.x, d[j][2] = v.y;
      d[j][3] = tw == 7 ? 0.f : right;
    }
    float o[6][4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {   // B^T_band = [4 0 -5 0 1 0; 0 -4 -4 1 1 0; 0 4 -4 -1 1 0; 0 -2 -1 2 1 0; 0 2 -1 -2 1 0; 0 4 0 -5 0 1]
      const float d0 = d[0][e], d1 = d[1][e], d2 = d[2][e], d3 = d[3][e], d4 = d[4][e], d5 = d[5][e];
      const float a42 = d4 - 4.f * d2, b31 = d3 - 4.f * d1, c42 = d4 - d2, e31 = d3 - d1;
      o[0][e] = (4.f * d0 + d4) - 5.f * d2;
      o[1][e] = a42 + b31;
      o[2][e] = a42 - b31;
      o[3][e] = c42 + 2.f * e31;
      o[4][e] = c42 - 2.f * e31;
      o[5][e] = (4.f * d1 + d5) - 5.f * d3;
    }
#pragma unroll
    for (int kb = 0; kb < 6; ++kb) {   // B^T_w = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1]
      float* dst = tile + (kb * 4 * 8 + tw) * 33 + c;
      dst[0 * 8 * 33] = o[kb][0] - o[kb][2];
      dst[1 * 8 * 33] = o[kb][1] + o[kb][2];
      dst[2 * 8 * 33] = o[kb][2] - o[kb][1];
      dst[3 * 8 * 33] = o[kb][1] - o[kb][3];
    }
  }
  __syncthreads();
  // write-out: thread = (plane, quad, column pair), pairs fastest
  const int n_out = 24 * 8 * a.TW;
  const long pos = (long)q * a.IP + (long)hp * a.TW;
  for (int i = tid; i < n_out; i += 256) {
    const int tw = i % a.TW, r = i / a.TW;
    const int cq = r & 7, k = r >> 3;
    const float* s = tile + (k * 8 + tw) * 33 + cq * 4;
    float* dst = a.xh + (((long)k * (a.Cin / 4) + cc * 8 + cq) * a.QIP + pos + tw) * 4;
    *reinterpret_cast<float4*>(dst) = make_float4(s[0], s[1], s[2], s[3]);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// The GEMM.  Workgroup = 4 waves, one tile of (up to 256 output positions = G whole images) x 64 output channels of ONE
// plane k; K = 3 row taps x Cin in stages of 16 channels.  A stage = the four quads of the tile's 384 padded positions
// (24 KB) and the 3 x 4 x 64 weight quads (12 KB), by 16-byte LDS-DMA through buffer descriptors, double-buffered, one
// barrier per stage (72 KB: two workgroups per CU).  A wave owns two blocks of 32 positions and both channel blocks: four
// accumulators; A = x^ (rows: positions), B = U (columns: output channels), so a lane of the result holds one output channel
// and m^ leaves in 128-byte runs.  Per stage and wave 24 ds_read_b128 and 96 MFMAs; the only vector arithmetic is the
// compiler's address bookkeeping.
// ---------------------------------------------------------------------------------------------------------------------
struct W2GemmArgs {
  const float* xh;
  const float* u;
  float* mh;
  int Cin, Cout, Q, TW, IP, OP, G, ptiles, cotiles;
  unsigned total_blocks;
};

__global__ void __launch_bounds__(256, 2) w2_gemm_kernel(const W2GemmArgs a) {
  constexpr int XS = W2_XP * W2_KC;         // floats of x^ per stage
  constexpr int US = 3 * W2_KC * W2_CO;     // ... of U
  constexpr int STAGE = XS + US;
  __shared__ __attribute__((aligned(16))) float lds[2 * STAGE];
  float* const st0 = lds;
  float* const st1 = lds + STAGE;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, khalf = lane >> 5;

  // channel tiles fastest: the workgroups that read the same x^ tile sit side by side (after the remap: on one XCD's L2)
  unsigned id = xcd_remap(blockIdx.x, a.total_blocks);
  const int co_t = take(id, a.cotiles);
  const int p_t = take(id, a.ptiles);
  const int k = __builtin_amdgcn_readfirstlane(id);
  const int q0 = p_t * a.G;
  const int nvalid = min(a.G, a.Q - q0) * a.OP;
  const long QIP = (long)a.Q * a.IP, QOP = (long)a.Q * a.OP;
  const long xplane = (long)a.Cin * QIP, uplane = (long)3 * a.Cin * a.Cout, mplane = QOP * a.Cout;
  const buf::rsrc rx = buf::make(a.xh + (long)k * xplane, (unsigned)(xplane * 4));
  const buf::rsrc ru = buf::make(a.u + (long)k * uplane, (unsigned)(uplane * 4));
  const buf::rsrc rm = buf::make(a.mh + (long)k * mplane, (unsigned)(mplane * 4));

  // DMA pieces of this wave: quad wv of the stage's x^ (six pieces of 64 positions), three of the twelve weight pieces.
  // (positions past the tile's images belong to the next tile or the next quad, past the plane they read zero: never used)
  unsigned xv[6], uv[3];
#pragma unroll
  for (int c = 0; c < 6; ++c) xv[c] = (unsigned)((q0 * a.IP + c * 64 + lane) * 16);
  const unsigned quad_bytes = (unsigned)(QIP * 16);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int ui = wv * 3 + i, dh = ui >> 2, qd = ui & 3;
    uv[i] = (unsigned)((((long)dh * (a.Cin / 4) + qd) * a.Cout + co_t * W2_CO + lane) * 16);
  }
  const unsigned ustage_bytes = (unsigned)(4 * a.Cout * 16);
  auto issue = [&](int s, float* st) __attribute__((always_inline)) {
    const unsigned xso = (unsigned)(4 * s + wv) * quad_bytes, uso = (unsigned)s * ustage_bytes;
#pragma unroll
    for (int c = 0; c < 6; ++c) buf::dma_b128(rx, xv[c], xso, st + (wv * W2_XP + c * 64) * 4);
#pragma unroll
    for (int i = 0; i < 3; ++i) buf::dma_b128(ru, uv[i], uso, st + XS + (wv * 3 + i) * 256);
  };

  // operand offsets (floats).  A: the lane's position of block pb, padded index = image * IP + (h * TW + tw), tap dh one
  // plane row further; a lane past the tile's positions reads position 0 and is not stored.  B: the lane's output channel.
  int aoff[2][3];
#pragma unroll
  for (int pb = 0; pb < 2; ++pb) {
    int c = (2 * wv + pb) * 32 + l31;
    if (c >= nvalid) c = 0;
    const int padded = (c / a.OP) * a.IP + c % a.OP;
#pragma unroll
    for (int dh = 0; dh < 3; ++dh) aoff[pb][dh] = (khalf * W2_XP + padded + dh * a.TW) * 4;
  }
  const int boff = XS + (khalf * W2_CO + l31) * 4;

  f32x16 acc[2][2];
#pragma unroll
  for (int pb = 0; pb < 2; ++pb)
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[pb][cb][r] = 0.f;

  auto compute = [&](const float* st) __attribute__((always_inline)) {
    static_for<0, 6>([&](auto ic) __attribute__((always_inline)) {
      constexpr int dh = decltype(ic)::value / 2, m = decltype(ic)::value % 2;
      float4 av[2], bv[2];
#pragma unroll
      for (int pb = 0; pb < 2; ++pb) av[pb] = *reinterpret_cast<const float4*>(st + aoff[pb][dh] + m * 2 * W2_XP * 4);
#pragma unroll
      for (int cb = 0; cb < 2; ++cb)
        bv[cb] = *reinterpret_cast<const float4*>(st + boff + ((dh * 4 + 2 * m) * W2_CO + cb * 32) * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float a0 = e == 0 ? av[0].x : e == 1 ? av[0].y : e == 2 ? av[0].z : av[0].w;
        const float a1 = e == 0 ? av[1].x : e == 1 ? av[1].y : e == 2 ? av[1].z : av[1].w;
        const float b0 = e == 0 ? bv[0].x : e == 1 ? bv[0].y : e == 2 ? bv[0].z : bv[0].w;
        const float b1 = e == 0 ? bv[1].x : e == 1 ? bv[1].y : e == 2 ? bv[1].z : bv[1].w;
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
      }
    });
  };

  // ---- stages, double-buffered: the pieces of stage s + 1 are requested before the MFMAs of stage s (Cin % 32 == 0: an
  // even number of stages) --------------------------------------------------------------------------------------------
  const int ns = a.Cin / W2_KC;
  issue(0, st0);
  for (int s = 0; s < ns; s += 2) {
    __builtin_amdgcn_s_waitcnt(0x0F70);      // vmcnt(0): this wave's pieces of the stage have landed ...
    __syncthreads();                         // ... everybody's have, and nobody reads the other stage any more
    issue(s + 1, st1);
    compute(st0);
    __builtin_amdgcn_s_waitcnt(0x0F70);
    __syncthreads();
    if (s + 2 < ns) issue(s + 2, st0);
    compute(st1);
  }

  // ---- m^: register r of a lane is position row (r & 3) + 8 (r >> 2) + 4 khalf of the block, the lane its output channel
#pragma unroll
  for (int pb = 0; pb < 2; ++pb)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int c = (2 * wv + pb) * 32 + (r & 3) + 8 * (r >> 2) + 4 * khalf;
      const unsigned o = c < nvalid ? (unsigned)((((long)q0 * a.OP + c) * a.Cout + co_t * W2_CO + l31) * 4) : buf::kOutside;
      buf::store(rm, o, acc[pb][0][r]);
      buf::store(rm, buf::at(o, 128u), acc[pb][1][r]);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Output pass.  One workgroup = one plane row h of image q x 32 output channels: thread (column pair, channel) reads its 24
// values of m^ (lanes along the channels: 128-byte runs), applies A^T_w = [1 1 1 0; 0 1 -1 -1] and
// A^T_band = [1 1 1 1 1 0; 0 1 -1 2 -2 0; 0 1 1 4 4 0; 0 1 -1 8 -8 1]; the 4 bands x 2 columns turn round in LDS and leave
// as float2 along w through the shared epilogue's arithmetic (epilogue.h: same operations in the same order), addressed
// through buffer descriptors over the sample's 32 channels -- a pair past the plane carries an offset outside: no store
// under a branch.
// ---------------------------------------------------------------------------------------------------------------------
struct W2OutArgs {
  const float* mh;
  const float* bias;
  float bias_scale;
  const float* residual;
  float out_scale;
  float* y;
  float* y2;
  const float* y2_shift;
  const float* y2_scale;
  int y2_shift_stride, y2_scale_stride, y2_act;
  int Cout, N, H, W, T, TW, OP;
  long QOP;
  // the row-pair form only: quarter-resolution outputs, the second output's form, the folded 1x1x1
  float* y_ll;
  float* y_hi[3];
  int y2_s2d;
  const float* rc_x;
  const float* rc_w;
  int rc_cin;
};

template <bool Y, bool RES, bool Y2>
__global__ void __launch_bounds__(256) w2_output_kernel(const W2OutArgs a) {
#pragma clang fp contract(off)   // (the shared epilogue's rounding: epilogue.h)
  __shared__ float tile[4 * 32 * 17];
  const int tid = threadIdx.x;
  const int cc = blockIdx.x, h = blockIdx.y, q = blockIdx.z;
  const int b = q / a.T, t = q % a.T;
  {
    const int co_l = tid & 31, tw = tid >> 5;
    if (tw < a.TW) {
      const float* src = a.mh + ((long)q * a.OP + h * a.TW + tw) * a.Cout + cc * 32 + co_l;
      const long kstride = a.QOP * a.Cout;
      float r[6][2];
#pragma unroll
      for (int kb = 0; kb < 6; ++kb) {
        const float m0 = src[(kb * 4 + 0) * kstride], m1 = src[(kb * 4 + 1) * kstride], m2 = src[(kb * 4 + 2) * kstride],
                    m3 = src[(kb * 4 + 3) * kstride];
        r[kb][0] = (m0 + m1) + m2;
        r[kb][1] = (m1 - m2) - m3;
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const float p12 = r[1][j] + r[2][j], d12 = r[1][j] - r[2][j], p34 = r[3][j] + r[4][j], d34 = r[3][j] - r[4][j];
        float* dst = tile + co_l * 17 + 2 * tw + j;
        dst[0 * 32 * 17] = (r[0][j] + p12) + p34;
        dst[1 * 32 * 17] = d12 + 2.f * d34;
        dst[2 * 32 * 17] = p12 + 4.f * p34;
        dst[3 * 32 * 17] = (d12 + 8.f * d34) + r[5][j];
      }
    }
  }
  __syncthreads();
  const long plane = (long)a.N * a.H * a.W;
  const long cb = ((long)b * a.Cout + cc * 32) * plane;
  const unsigned span = (unsigned)(32 * plane * 4);
  const buf::rsrc ry = buf::make(Y ? a.y + cb : nullptr, Y ? span : 0u);
  const buf::rsrc rr = buf::make(RES ? a.residual + cb : nullptr, RES ? span : 0u);
  const buf::rsrc r2 = buf::make(Y2 ? a.y2 + cb : nullptr, Y2 ? span : 0u);
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int i = tid + 256 * it;
    const int wp = i & 7, band = (i >> 3) & 3, co_l = i >> 5;
    const int co = cc * 32 + co_l;
    const unsigned o = wp < a.TW ? (unsigned)(((co_l * (long)a.N + 4 * t + band) * a.H + h) * a.W + 2 * wp) * 4u : buf::kOutside;
    const float* s = tile + (band * 32 + co_l) * 17 + 2 * wp;
    float v[2] = {s[0], s[1]};
    const float bias_t = a.bias ? a.bias[co] * a.bias_scale : 0.f;
    float2 res = make_float2(0.f, 0.f);
    if constexpr (RES) res = buf::load2(rr, o);
    v[0] = (v[0] + bias_t + res.x) * a.out_scale;
    v[1] = (v[1] + bias_t + res.y) * a.out_scale;
    if constexpr (Y) buf::store2(ry, o, make_float2(v[0], v[1]));
    if constexpr (Y2) {
      const float sh2 = a.y2_shift ? a.y2_shift[(long)b * a.y2_shift_stride + co] : 0.f;
      const float sc2 = a.y2_scale ? a.y2_scale[(long)b * a.y2_scale_stride + co] : 1.f;
      float u[2];
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const float x = v[e] + sh2;
        const float xa = silu_f(x);
        u[e] = (a.y2_act ? xa : x) * sc2;
      }
      buf::store2(r2, o, make_float2(u[0], u[1]));
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Output pass, row-pair form: one workgroup = the plane rows 2 hp, 2 hp + 1 of image q x 32 output channels, so that a
// thread of the write-out holds the whole 2 x 2 block (a b / c d) of a column pair -- what the quarter-resolution outputs
// are made of (tmdiff_hip.h: y_ll, y_hi, y2_s2d).  The transforms are those of the one-row form, once per row, into one LDS
// tile [band][row][channel][column]; every full-resolution value goes through the same operations in the same order
// (bit-identical y / y2), the 2 x 2 sums follow conv3d_wf's epilogue ((a + b) + (c + d) and the like).
// RC: the folded 1x1x1 "residual convolution" (desc.rc_*), added to the tile BEFORE the epilogue arithmetic on the matrix
// pipe, as conv3d_wf does it: wave wv owns band wv = one 32 x 32 block of (channels) x (2 rows x 16 columns); the
// accumulator starts as the tile's values, a K-step is two input channels (lane half = channel parity group), the lane's x
// values come from global memory through a buffer descriptor over the sample's rc_cin channels (rows of 16 floats), its
// weights as float4 straight from the PyTorch-layout [Cout][rc_cin] (16 KB per channel tile at 128 channels: cache
// resident); 32 channels in flight while the previous 32 are multiplied.  Channel order inside a group of 8: lane half 0
// takes 0..3, half 1 takes 4..7 -- any order does, as long as both operands agree.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int W2_RS = 32 * 17 + 16;   // floats per (band, row) block: the two rows of a band sixteen banks apart

template <bool RES, bool RC>
__global__ void __launch_bounds__(256) w2_output2_kernel(const W2OutArgs a) {
#pragma clang fp contract(off)   // (the shared epilogue's rounding: epilogue.h)
  __shared__ float tile[8 * W2_RS];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, khalf = lane >> 5;
  const int cc = blockIdx.x, hp = blockIdx.y, q = blockIdx.z;
  const int b = q / a.T, t = q % a.T;
  const int hw = a.H * a.W;
  const long plane = (long)a.N * hw;

  // ---- the folded 1x1x1's operands: requested first, multiplied after the transforms
  const int ngrp = RC ? a.rc_cin / 32 : 0;
  const buf::rsrc xr = buf::make(RC ? a.rc_x + (long)b * a.rc_cin * plane : nullptr, RC ? (unsigned)((long)a.rc_cin * plane * 4) : 0u);
  const int rrow = l31 >> 4, rcol = l31 & 15;     // MFMA column l31 = (row, column) of band wv
  // (a column past the plane: any valid address, the value is never stored)
  const unsigned xo = (unsigned)((4 * khalf * (int)plane + (rcol < a.W ? ((4 * t + wv) * a.H + 2 * hp + rrow) * a.W + rcol : 0)) * 4);
  const unsigned ch_bytes = (unsigned)(plane * 4);
  const float* wrow = RC ? a.rc_w + (long)(cc * 32 + l31) * a.rc_cin + 4 * khalf : nullptr;
  float4 aw0[4], aw1[4];
  float xv0[16], xv1[16];
  auto fetch = [&](int jg, float4 (&aw)[4], float (&xv)[16]) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 4; ++i) aw[i] = *reinterpret_cast<const float4*>(wrow + jg * 32 + 8 * i);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) xv[4 * i + e] = buf::load(xr, xo, (unsigned)(jg * 32 + 8 * i + e) * ch_bytes);
  };
  if constexpr (RC) fetch(0, aw0, xv0);

  // ---- A^T_w and A^T_band of both rows into the tile (the one-row form's arithmetic)
  {
    const int co_l = tid & 31, tw = tid >> 5;
    if (tw < a.TW) {
      const long kstride = a.QOP * a.Cout;
#pragma unroll
      for (int row = 0; row < 2; ++row) {
        const float* src = a.mh + ((long)q * a.OP + (2 * hp + row) * a.TW + tw) * a.Cout + cc * 32 + co_l;
        float r[6][2];
#pragma unroll
        for (int kb = 0; kb < 6; ++kb) {
          const float m0 = src[(kb * 4 + 0) * kstride], m1 = src[(kb * 4 + 1) * kstride], m2 = src[(kb * 4 + 2) * kstride],
                      m3 = src[(kb * 4 + 3) * kstride];
          r[kb][0] = (m0 + m1) + m2;
          r[kb][1] = (m1 - m2) - m3;
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const float p12 = r[1][j] + r[2][j], d12 = r[1][j] - r[2][j], p34 = r[3][j] + r[4][j], d34 = r[3][j] - r[4][j];
          float* dst = tile + row * W2_RS + co_l * 17 + 2 * tw + j;
          dst[0 * 2 * W2_RS] = (r[0][j] + p12) + p34;
          dst[1 * 2 * W2_RS] = d12 + 2.f * d34;
          dst[2 * 2 * W2_RS] = p12 + 4.f * p34;
          dst[3 * 2 * W2_RS] = (d12 + 8.f * d34) + r[5][j];
        }
      }
    }
  }
  __syncthreads();

  if constexpr (RC) {
    // register r of a lane is channel (r & 3) + 8 (r >> 2) + 4 khalf of the block, the lane its position
    float* const tb = tile + (wv * 2 + rrow) * W2_RS + 4 * khalf * 17 + rcol;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = tb[((r & 3) + 8 * (r >> 2)) * 17];
    auto mma = [&](const float4 (&aw)[4], const float (&xv)[16]) __attribute__((always_inline)) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(aw[i].x, xv[4 * i + 0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(aw[i].y, xv[4 * i + 1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(aw[i].z, xv[4 * i + 2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(aw[i].w, xv[4 * i + 3], acc, 0, 0, 0);
      }
    };
    for (int jg = 0; jg < ngrp; jg += 2) {
      if (jg + 1 < ngrp) fetch(jg + 1, aw1, xv1);
      mma(aw0, xv0);
      if (jg + 1 < ngrp) {
        if (jg + 2 < ngrp) fetch(jg + 2, aw0, xv0);
        mma(aw1, xv1);
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) tb[((r & 3) + 8 * (r >> 2)) * 17] = acc[r];
    __syncthreads();
  }

  // ---- write-out: thread = (channel, band, column pair), pairs fastest; both rows of the pair
  const long cb = ((long)b * a.Cout + cc * 32) * plane;
  const unsigned span = (unsigned)(32 * plane * 4);
  const bool want_y = a.y != nullptr, want_y2 = a.y2 != nullptr, want_ll = a.y_ll != nullptr, want_hi = a.y_hi[0] != nullptr;   // (uniform)
  const buf::rsrc ry = buf::make(want_y ? a.y + cb : nullptr, want_y ? span : 0u);
  const buf::rsrc rr = buf::make(RES ? a.residual + cb : nullptr, RES ? span : 0u);
  // (the space-to-depth form [B, 4 Cout, N, H/2, W/2]: the tile's 128 quarter-size channels start at the same float)
  const buf::rsrc r2 = buf::make(want_y2 ? a.y2 + cb : nullptr, want_y2 ? span : 0u);
  // the quarter-size outputs: the same 32 channels, a quarter plane each
  const long cbq = cb >> 2;
  const unsigned spanq = span >> 2;
  const buf::rsrc rll = buf::make(want_ll ? a.y_ll + cbq : nullptr, want_ll ? spanq : 0u);
  const buf::rsrc rh0 = buf::make(want_hi ? a.y_hi[0] + cbq : nullptr, want_hi ? spanq : 0u);
  const buf::rsrc rh1 = buf::make(want_hi ? a.y_hi[1] + cbq : nullptr, want_hi ? spanq : 0u);
  const buf::rsrc rh2 = buf::make(want_hi ? a.y_hi[2] + cbq : nullptr, want_hi ? spanq : 0u);
  const int hq = a.H >> 1, wq = a.W >> 1;
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int i = tid + 256 * it;
    const int wp = i & 7, band = (i >> 3) & 3, co_l = i >> 5;
    const int co = cc * 32 + co_l;
    const int n = 4 * t + band;
    const bool ok = wp < a.TW;
    const unsigned o0 = ok ? (unsigned)(((co_l * a.N + n) * a.H + 2 * hp) * a.W + 2 * wp) * 4u : buf::kOutside;   // row 2 hp
    const unsigned o1 = buf::at(o0, (unsigned)a.W * 4u);                                                            // row 2 hp + 1
    const unsigned oq = ok ? (unsigned)(((co_l * a.N + n) * hq + hp) * wq + wp) * 4u : buf::kOutside;              // quarter plane
    const float* s = tile + band * 2 * W2_RS + co_l * 17 + 2 * wp;
    float v[4] = {s[0], s[1], s[W2_RS], s[W2_RS + 1]};      // a b / c d
    const float bias_t = a.bias ? a.bias[co] * a.bias_scale : 0.f;
    float2 res0 = make_float2(0.f, 0.f), res1 = make_float2(0.f, 0.f);
    if constexpr (RES) res0 = buf::load2(rr, o0), res1 = buf::load2(rr, o1);
    v[0] = (v[0] + bias_t + res0.x) * a.out_scale;
    v[1] = (v[1] + bias_t + res0.y) * a.out_scale;
    v[2] = (v[2] + bias_t + res1.x) * a.out_scale;
    v[3] = (v[3] + bias_t + res1.y) * a.out_scale;
    if (want_y) {
      buf::store2(ry, o0, make_float2(v[0], v[1]));
      buf::store2(ry, o1, make_float2(v[2], v[3]));
    }
    const float sh2 = a.y2_shift ? a.y2_shift[(long)b * a.y2_shift_stride + co] : 0.f;
    const float sc2 = a.y2_scale ? a.y2_scale[(long)b * a.y2_scale_stride + co] : 1.f;
    if (want_y2) {
      float u[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float x = v[e] + sh2;
        const float xa = silu_f(x);
        u[e] = (a.y2_act ? xa : x) * sc2;
      }
      if (a.y2_s2d) {      // channel 4 co + 2 ph + pw, each a quarter plane
        const unsigned os = ok ? (unsigned)(((4 * co_l * a.N + n) * hq + hp) * wq + wp) * 4u : buf::kOutside;
        const unsigned qplane4 = (unsigned)(plane >> 2) * 4u;
#pragma unroll
        for (int e = 0; e < 4; ++e) buf::store(r2, buf::at(os, (unsigned)e * qplane4), u[e]);
      } else {
        buf::store2(r2, o0, make_float2(u[0], u[1]));
        buf::store2(r2, o1, make_float2(u[2], u[3]));
      }
    }
    if (want_ll) {
      const float ll = ((v[0] + v[1]) + (v[2] + v[3])) * 0.25f;
      if (want_hi) {       // the whole transform: LL / 2 through the second output's prologue, LH, HL, HH
        const float x = ll + sh2;
        const float xa = silu_f(x);
        buf::store(rll, oq, (a.y2_act ? xa : x) * sc2);
        buf::store(rh0, oq, ((v[0] - v[1]) + (v[2] - v[3])) * 0.5f);
        buf::store(rh1, oq, ((v[0] + v[1]) - (v[2] + v[3])) * 0.5f);
        buf::store(rh2, oq, ((v[0] - v[1]) - (v[2] - v[3])) * 0.5f);
      } else {
        buf::store(rll, oq, ll);
      }
    }
  }
}

}  // namespace

/* 1 if tmdiff_conv3d_w2_fwd takes the convolution described by d (else: tmdiff_conv3d_wf_fwd) */
extern "C" int tmdiff_conv3d_w2_supported(const tmdiff_conv3d_desc* d) {
  return w2_shape_ok(d) && w2_fits(d, w2_plan(d)) ? 1 : 0;
}

/* ... and 1 as well for the descriptors whose epilogue the row-pair output pass writes: a folded 1x1x1 (rc_*), y_ll, y_hi, y2_s2d */
extern "C" int tmdiff_conv3d_w2_epilogue_supported(const tmdiff_conv3d_desc* d) {
  return w2_epilogue_ok(d) && w2_fits(d, w2_plan(d)) ? 1 : 0;
}

extern "C" size_t tmdiff_conv3d_w2_workspace_bytes(const tmdiff_conv3d_desc* d) {
  if (!w2_epilogue_ok(d)) return 0;
  const W2Plan p = w2_plan(d);
  return (p.xh_floats + p.mh_floats) * sizeof(float);
}

extern "C" size_t tmdiff_conv3d_w2_packed_bytes(int32_t Cout, int32_t Cin) {
  if (Cout <= 0 || Cin <= 0 || Cin % 4) return 0;
  return (size_t)72 * Cout * Cin * sizeof(float);
}

extern "C" int tmdiff_conv3d_w2_pack_weights(const float* w, float* packed, int32_t Cout, int32_t Cin, tmdiff_stream_t stream) {
  using namespace tmdiff;
  TMDIFF_REQUIRE(w && packed, "conv3d_w2_pack_weights: NULL pointer");
  TMDIFF_REQUIRE(Cout > 0 && Cin > 0 && Cin % 4 == 0 && (size_t)72 * Cout * Cin < (1ull << 31),
                 "conv3d_w2_pack_weights: Cout=%d Cin=%d (Cin %% 4 == 0)", Cout, Cin);
  const long n = (long)3 * Cin * Cout;
  w2_pack_kernel<<<(unsigned)((n + 255) / 256), 256, 0, as_stream(stream)>>>(w, packed, Cout, Cin);
  return check_launch("conv3d_w2_pack_weights");
}

extern "C" int tmdiff_conv3d_w2_fwd(const tmdiff_conv3d_desc* d, void* workspace, int32_t stages, tmdiff_stream_t stream) {
  using namespace tmdiff;
  TMDIFF_REQUIRE(d && workspace, "conv3d_w2_fwd: NULL pointer");
  if (!w2_epilogue_ok(d))
    return fail(TMDIFF_E_UNSUPPORTED, "conv3d_w2_fwd: fp32 3x3x3, groups 1, one input tensor, 4 or 8 bands, even W <= 16, 4 <= H <= 32, "
                                      "Cin >= 128 (%% 32), Cout >= 256 (%% 64); a folded 1x1x1 (rc_cin %% 32 == 0, at most 512, no residual) "
                                      "and LL / Haar / space-to-depth outputs (8 bands) on even H");
  const W2Plan p = w2_plan(d);
  if (!w2_fits(d, p)) return fail(TMDIFF_E_UNSUPPORTED, "conv3d_w2_fwd: tensor too large for 32-bit offsets");
  TMDIFF_REQUIRE(d->seg_x[0] && d->w_packed && (d->y || d->y2 || d->y_ll), "conv3d_w2_fwd: input, weights and an output");
  TMDIFF_REQUIRE(aligned16(d->seg_x[0]) && aligned16(workspace) && aligned16(d->w_packed) && aligned16(d->y) && aligned16(d->y2) &&
                     aligned16(d->residual) && aligned16(d->y_ll) && aligned16(d->y_hi[0]) && aligned16(d->y_hi[1]) &&
                     aligned16(d->y_hi[2]) && aligned16(d->rc_x) && aligned16(d->rc_w),
                 "conv3d_w2_fwd: 16-byte aligned tensors / workspace");
  TMDIFF_REQUIRE(!d->rc_x || d->rc_w, "conv3d_w2_fwd: rc_x without rc_w");
  hipStream_t st = as_stream(stream);
  float* xh = static_cast<float*>(workspace);
  float* mh = xh + p.xh_floats;
  // (timing: `stages` = bit mask of the launches that run -- 1 input pass, 2 GEMM, 4 output pass; 0 = all)
  if (stages == 0) stages = 7;

  if (stages & 1) {
    W2InArgs a;
    a.x = d->seg_x[0]; a.xh = xh;
    a.in_shift = d->in_shift; a.in_scale = d->in_scale;
    a.shift_stride = bank_stride(d->in_shift_stride, d->Cin);
    a.scale_stride = bank_stride(d->in_scale_stride, d->Cin);
    a.in_act = d->in_act;
    a.Cin = d->Cin; a.N = d->N; a.H = d->H; a.W = d->W; a.T = p.T; a.TW = p.TW; a.IP = p.IP;
    a.QIP = (long)p.Q * p.IP;
    w2_input_kernel<<<dim3((unsigned)(d->Cin / 32), (unsigned)p.Hp, (unsigned)p.Q), 256, 0, st>>>(a);
    if (const int rc = check_launch("conv3d_w2_fwd(input pass)")) return rc;
  }
  if (stages & 2) {
    W2GemmArgs a;
    a.xh = xh; a.u = d->w_packed; a.mh = mh;
    a.Cin = d->Cin; a.Cout = d->Cout; a.Q = p.Q; a.TW = p.TW; a.IP = p.IP; a.OP = p.OP; a.G = p.G; a.ptiles = p.ptiles;
    a.cotiles = d->Cout / W2_CO;
    if (const int rc = set_grid(a, (long)p.ptiles * a.cotiles * 24, "conv3d_w2_fwd")) return rc;
    w2_gemm_kernel<<<a.total_blocks, 256, 0, st>>>(a);
    if (const int rc = check_launch("conv3d_w2_fwd")) return rc;
  }
  if (stages & 4) {
    W2OutArgs a;
    a.mh = mh;
    a.bias = d->bias; a.bias_scale = d->bias_scale; a.residual = d->residual; a.out_scale = d->out_scale;
    a.y = d->y; a.y2 = d->y2; a.y2_shift = d->y2_shift; a.y2_scale = d->y2_scale; a.y2_act = d->y2_act;
    a.y2_shift_stride = bank_stride(d->y2_shift_stride, d->Cout);
    a.y2_scale_stride = bank_stride(d->y2_scale_stride, d->Cout);
    a.Cout = d->Cout; a.N = d->N; a.H = d->H; a.W = d->W; a.T = p.T; a.TW = p.TW; a.OP = p.OP;
    a.QOP = (long)p.Q * p.OP;
    a.y_ll = d->y_ll; a.y2_s2d = d->y2 && d->y2_s2d ? 1 : 0;
    for (int i = 0; i < 3; ++i) a.y_hi[i] = d->y_hi[0] ? d->y_hi[i] : nullptr;
    a.rc_x = d->rc_x; a.rc_w = d->rc_w; a.rc_cin = d->rc_cin;
    const dim3 grid((unsigned)(d->Cout / 32), (unsigned)d->H, (unsigned)p.Q);
#define TMDIFF_W2_OUT(Y, R, Y2) w2_output_kernel<Y, R, Y2><<<grid, 256, 0, st>>>(a)
    if (w2_folds(d) || w2_quarter(d)) {      // the row-pair form (w2_epilogue_ok: even H)
      const dim3 grid2((unsigned)(d->Cout / 32), (unsigned)(d->H / 2), (unsigned)p.Q);
      if (d->rc_x) w2_output2_kernel<false, true><<<grid2, 256, 0, st>>>(a);
      else if (d->residual) w2_output2_kernel<true, false><<<grid2, 256, 0, st>>>(a);
      else w2_output2_kernel<false, false><<<grid2, 256, 0, st>>>(a);
    } else if (d->y) {
      if (d->residual) { if (d->y2) TMDIFF_W2_OUT(true, true, true); else TMDIFF_W2_OUT(true, true, false); }
      else             { if (d->y2) TMDIFF_W2_OUT(true, false, true); else TMDIFF_W2_OUT(true, false, false); }
    } else {
      if (d->residual) TMDIFF_W2_OUT(false, true, true); else TMDIFF_W2_OUT(false, false, true);
    }
#undef TMDIFF_W2_OUT
    if (const int rc = check_launch("conv3d_w2_fwd(output pass)")) return rc;
  }
  return TMDIFF_OK;
}
