// Weight gradient of the 3x3x3 convolution with bf16 operands and fp32 accumulation (v_mfma_f32_32x32x16_bf16).  Same contract and result layout as tmdiff_conv3d_wgrad_bias
// (include/tmdiff_hip.h):  dw[co][ci][tap] = sum_{b,pos} g[b,co,pos] * x'[b,ci,pos+tap];  g and x' are rounded to bf16
// (pack_bf16x2, common.h) when they are staged in LDS, the products are exact in fp32 and summed in fp32.
//
// GEMM view per (group, tap):  D[co, ci] = sum_pos G[co][pos] * X'[ci][pos + tap]
//   MFMA rows (A) = 32 output channels, columns (B) = 32 input channels, K = 16 positions: 16 consecutive columns w of one
//   image row, lanes 0-31 the first eight, lanes 32-63 the second eight -- one 16-byte LDS unit per lane and operand.
// The tap's column offset dx is put on g, its band / row offsets (dz, dy) on x':
//   dw[.., (dz,dy,dx)] = sum_{n,h,w'} g[n, h, w' - dx + 1] * x'[n + dz - 1, h + dy - 1, w']
// so the K positions w' are aligned 16-column slices of the x' rows for every tap (no unaligned operand reads): LDS holds
//   xs[3 dz][TH + 2 rows][32 ci][16 w'] : the halo rows of x', once;
//   gs[3 dx][TH rows][32 co][16 w']     : g three times, shifted by dx - 1 columns;
// zero outside the tensor (padding, ragged rows / columns / input-channel tiles), so masked K slices add exact zeros.
// Rows of 32 channels x 16 columns are 1 KB of consecutive units: a wave's ds_read_b128 covers one row without conflicts.
// A workgroup (6 waves) owns one (group, 32 co, 32 ci) tile and a contiguous range of boxes (one band, TH rows, 16 columns);
// wave (dx, half) accumulates the nine (dz, dy) taps of its dx over rows 2 half, 2 half + 1 of every box: one A and nine B
// reads per nine MFMAs.  Every wave writes its accumulators as one slot of fp32 partials [slot][g][tap][co][ci] to the
// workspace (slots = 2 x splits); wgrad_bf16_reduce_kernel adds the slots in slot order (no atomics: same bits every run).
// The bias gradient is summed from the UNROUNDED g by a pass of its own (slices per channel, then slice order).
#include <cstdint>

#include "common.h"

namespace {

using namespace tmdiff;

constexpr int TH = 4;        // rows of a box
constexpr int WT = 16;       // columns of a box = one K slice
constexpr int WAVES = 6;     // (dx, row half)
constexpr int XS_UNITS = 3 * (TH + 2) * 32 * 2;
constexpr int GS_UNITS = 3 * TH * 32 * 2;
constexpr int BIAS_SLICES_MAX = 64;

struct WbArgs {
  int B, N, H, W, Cin, Cout, cin_g, cout_g, groups;
  const float* xp;   // x' [B, Cin, N, H, W]
  const float* g;    // [B, Cout, N, H, W]
  float* ws;         // [slots][groups][27][cout_g][cin_g]
  int nbh, nbw;      // boxes per band plane along h, w
  int tiles_co, tiles_ci;
  int splits, boxes_per_split;
  long total_boxes;
  unsigned total_blocks;
};

struct WbPlan {
  int nbh, nbw, tiles_co, tiles_ci, splits, boxes_per_split, slots, bias_slices;
  long total_boxes;
  WgradWorkspace ws;
};

// eight consecutive columns w0 .. w0 + 7 of a row (NULL row: all zero), columns outside [0, W) zero, as one unit of 8 bf16
__device__ __forceinline__ uint4 stage_unit(const float* row, int w0, int W) {
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int w = w0 + j;
    v[j] = (row != nullptr && w >= 0 && w < W) ? row[w] : 0.f;
  }
  return make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7]));
}

__global__ void __launch_bounds__(64 * WAVES) wgrad_bf16_kernel(const WbArgs a) {
  __shared__ uint4 xs[XS_UNITS];
  __shared__ uint4 gs[GS_UNITS];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wv = tid >> 6;
  const int l31 = lane & 31, kg = lane >> 5;
  const int dx = wv % 3, half = wv / 3;

  unsigned id = blockIdx.x;
  const int split = take(id, a.splits);
  const int ci_t = take(id, a.tiles_ci);
  const int co_t = take(id, a.tiles_co);
  const int grp = __builtin_amdgcn_readfirstlane(id);
  const int ci0 = ci_t * 32, co0 = co_t * 32;
  const long plane = (long)a.N * a.H * a.W;

  f32x16 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  const long box_lo = (long)split * a.boxes_per_split;
  const long box_hi = min(box_lo + a.boxes_per_split, a.total_boxes);
  for (long box = box_lo; box < box_hi; ++box) {
    long r = box;
    const int wb = (int)(r % a.nbw); r /= a.nbw;
    const int hb = (int)(r % a.nbh); r /= a.nbh;
    const int n = (int)(r % a.N);
    const int b = (int)(r / a.N);
    const int h0 = hb * TH, w0 = wb * WT;

    __syncthreads();   // the previous box's operand reads are done
    // x': [dz][row 0 .. TH + 1][ci][2 units]
    for (int u = tid; u < XS_UNITS; u += 64 * WAVES) {
      const int unit = u & 1, ci = (u >> 1) & 31, row = u >> 6;
      const int zz = row / (TH + 2), yy = row % (TH + 2);
      const int nn = n + zz - 1, hh = h0 + yy - 1, c = ci0 + ci;
      const bool valid = nn >= 0 && nn < a.N && hh >= 0 && hh < a.H && c < a.cin_g;
      const float* src = valid ? a.xp + ((long)b * a.Cin + grp * a.cin_g + c) * plane + ((long)nn * a.H + hh) * a.W : nullptr;
      xs[u] = stage_unit(src, w0 + 8 * unit, a.W);
    }
    // g: [dx][row 0 .. TH - 1][co][2 units], copy dx holds g[w' - dx + 1] at column w'
    for (int u = tid; u < GS_UNITS; u += 64 * WAVES) {
      const int unit = u & 1, co = (u >> 1) & 31, rs = u >> 6;
      const int s = rs / TH, rr = rs % TH;
      const int hh = h0 + rr;
      const float* src = hh < a.H ? a.g + ((long)b * a.Cout + grp * a.cout_g + co0 + co) * plane + ((long)n * a.H + hh) * a.W : nullptr;
      gs[u] = stage_unit(src, w0 + 8 * unit - s + 1, a.W);
    }
    __syncthreads();

#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
      const int row = 2 * half + rr;
      union { bf16x8 h; uint4 u; } av, bv;
      av.u = gs[((dx * TH + row) * 32 + l31) * 2 + kg];
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int dz = t / 3, dy = t % 3;
        bv.u = xs[((dz * (TH + 2) + row + dy) * 32 + l31) * 2 + kg];
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av.h, bv.h, acc[t], 0, 0, 0);
      }
    }
  }

  // D layout: column = lane & 31 (ci), row (r & 3) + 8 (r >> 2) + 4 kg (co)
  const int slot = split * 2 + half;
  const int ci = ci0 + l31;
  if (ci < a.cin_g) {
    float* dst = a.ws + (((long)slot * a.groups + grp) * 27) * a.cout_g * a.cin_g;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int tap = t * 3 + dx;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = co0 + (r & 3) + 8 * (r >> 2) + 4 * kg;
        dst[((long)tap * a.cout_g + co) * a.cin_g + ci] = acc[t][r];
      }
    }
  }
}

// bias partials: part[slice][c] = sum over the slice's positions of every sample of g[b, c, .] (fp32 g as it is; fixed order)
__global__ void __launch_bounds__(256) wgrad_bf16_bias_kernel(const float* __restrict__ g, float* __restrict__ part, int B, int C,
                                                              long plane) {
  __shared__ float red[4];
  const int c = blockIdx.x;
  const long per = (plane + gridDim.y - 1) / gridDim.y;
  const long lo = blockIdx.y * per, hi = min(lo + per, plane);
  float s = 0.f;
  for (int b = 0; b < B; ++b) {
    const float* p = g + ((long)b * C + c) * plane;
    for (long i = lo + threadIdx.x; i < hi; i += 256) s += p[i];
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) part[(long)blockIdx.y * C + c] = s;
}

// dw[g*cout_g + co][ci][tap] = sum_slot ws[slot][g][tap][co][ci], slots added in slot order; the last workgroup also finishes
// the bias gradient: dbias[c] = bias_scale * sum_slice part[slice][c]
__global__ void __launch_bounds__(256) wgrad_bf16_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dw, int slots,
                                                                int cout_g, int cin_g, long total, const float* __restrict__ bias_part,
                                                                int bias_slices, int cout, float* __restrict__ dbias,
                                                                float bias_scale) {
  if (dbias && blockIdx.x == gridDim.x - 1) finish_bias_grad(bias_part, bias_slices, cout, dbias, bias_scale);
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += 256L * gridDim.x) {
    float t = 0.f;
    for (int k = 0; k < slots; ++k) t += ws[(long)k * total + i];
    const int ci = (int)(i % cin_g);
    long r = i / cin_g;
    const int co = (int)(r % cout_g); r /= cout_g;
    const int tap = (int)(r % 27);
    const int grp = (int)(r / 27);
    dw[(((long)grp * cout_g + co) * cin_g + ci) * 27 + tap] = t;
  }
}

// x' is not the first segment as it stands: the prologue pass writes it into the workspace first
bool needs_xp(const tmdiff_conv3d_desc* d) { return d->nseg > 1 || input_prologue(d); }

// the descriptors the kernel takes (what _supported() answers; the workspace and slot queries give 0 for any other)
bool shape_ok(const tmdiff_conv3d_desc* d) {
  if (!d || d->ksize != 3 || (d->groups != 1 && d->groups != 3)) return false;
  if (d->B <= 0 || d->N <= 0 || d->H <= 0 || d->W <= 0 || d->Cin <= 0 || d->Cout <= 0) return false;
  if (d->Cin % d->groups || d->Cout % d->groups) return false;
  if ((d->Cin / d->groups) % 8 || (d->Cout / d->groups) % 32) return false;
  // 32-bit box / in-sample offset arithmetic, as tmdiff_conv3d_wgrad
  const long boxes = (long)d->B * d->N * ((d->H + TH - 1) / TH) * ((d->W + WT - 1) / WT);
  if (boxes >= (1L << 31) || (long)d->N * d->H * d->W * 32 >= (1L << 31)) return false;
  // the prologue pass (launch_prologue_apply) has one grid row per (sample, channel): at most 65535
  return !(needs_xp(d) && (long)d->B * d->Cin > 65535);
}

WbPlan plan_wgrad_bf16(const tmdiff_conv3d_desc* d) {
  WbPlan p;
  p.nbh = (d->H + TH - 1) / TH; p.nbw = (d->W + WT - 1) / WT;
  p.total_boxes = (long)d->B * d->N * p.nbh * p.nbw;
  const int cout_g = d->Cout / d->groups, cin_g = d->Cin / d->groups;
  p.tiles_co = cout_g / 32; p.tiles_ci = (cin_g + 31) / 32;
  // about 1024 workgroups (four rounds of the 256 CUs), at most 256 ranges of boxes and never an empty one
  const long tiles = (long)d->groups * p.tiles_co * p.tiles_ci;
  long s = (1024 + tiles - 1) / tiles;
  if (s > 256) s = 256;
  if (s > p.total_boxes) s = p.total_boxes;
  if (s < 1) s = 1;
  p.boxes_per_split = (int)((p.total_boxes + s - 1) / s);
  p.splits = (int)((p.total_boxes + p.boxes_per_split - 1) / p.boxes_per_split);
  p.slots = 2 * p.splits;
  const long plane = (long)d->N * d->H * d->W;
  long bs = (plane + 4095) / 4096;
  p.bias_slices = (int)(bs > BIAS_SLICES_MAX ? BIAS_SLICES_MAX : bs);
  p.ws = wgrad_workspace((size_t)p.slots * d->Cout * cin_g * 27, (size_t)p.bias_slices * d->Cout, needs_xp(d), d);
  return p;
}

}  // namespace

extern "C" int tmdiff_conv3d_wgrad_bf16_supported(const tmdiff_conv3d_desc* d) {
  return shape_ok(d) ? 1 : 0;
}

extern "C" size_t tmdiff_conv3d_wgrad_bf16_workspace_bytes(const tmdiff_conv3d_desc* d) {
  if (!shape_ok(d)) return 0;
  return plan_wgrad_bf16(d).ws.bytes();
}

extern "C" int32_t tmdiff_conv3d_wgrad_bf16_slots(const tmdiff_conv3d_desc* d) {
  return shape_ok(d) ? plan_wgrad_bf16(d).slots : 0;
}

extern "C" int tmdiff_conv3d_wgrad_bf16(const tmdiff_conv3d_desc* d, const float* g, float* dw, float* dbias, void* workspace,
                                        tmdiff_stream_t stream) {
  using namespace tmdiff;
  const char* what = "conv3d_wgrad_bf16";
  TMDIFF_REQUIRE(d && g && dw, "conv3d_wgrad_bf16: NULL pointer");
  // (a group count the fp32 weight gradient takes and this kernel does not is "unsupported", not "invalid")
  if (d->groups >= 1 && d->groups != 1 && d->groups != 3) return fail(TMDIFF_E_UNSUPPORTED, "%s: groups=%d (1 or 3)", what, d->groups);
  if (const int rc = check_head(d, what)) return rc;
  TMDIFF_REQUIRE(d->B > 0, "conv3d_wgrad_bf16: empty batch");
  if (!tmdiff_conv3d_wgrad_bf16_supported(d))
    return fail(TMDIFF_E_UNSUPPORTED, "%s: ksize=%d Cin/g=%d (multiple of 8) Cout/g=%d (multiple of 32), or extents beyond 32-bit offsets",
                what, d->ksize, d->Cin / d->groups, d->Cout / d->groups);
  if (const int rc = check_segments(d, what)) return rc;
  TMDIFF_REQUIRE(workspace != nullptr && aligned16(workspace), "conv3d_wgrad_bf16: NULL / unaligned workspace");
  if (const int rc = check_mask_or_dropout(d, what)) return rc;

  const WbPlan p = plan_wgrad_bf16(d);
  hipStream_t st = as_stream(stream);
  WbArgs a;
  a.B = d->B; a.N = d->N; a.H = d->H; a.W = d->W; a.Cin = d->Cin; a.Cout = d->Cout;
  a.groups = d->groups; a.cin_g = d->Cin / d->groups; a.cout_g = d->Cout / d->groups;
  a.g = g; a.ws = p.ws.partials(workspace);
  float* bias_part = p.ws.bias(workspace);
  // (the pass tmdiff_conv3d_wgrad runs: x', and the concatenation of the segments, as one dense tensor)
  if (const int rc = p.ws.stage_input(d, workspace, st, &a.xp)) return rc;
  a.nbh = p.nbh; a.nbw = p.nbw; a.tiles_co = p.tiles_co; a.tiles_ci = p.tiles_ci;
  a.splits = p.splits; a.boxes_per_split = p.boxes_per_split; a.total_boxes = p.total_boxes;
  const long blocks = (long)d->groups * p.tiles_co * p.tiles_ci * p.splits;
  if (const int rc = set_grid(a, blocks, what)) return rc;
  wgrad_bf16_kernel<<<(unsigned)blocks, 64 * WAVES, 0, st>>>(a);
  if (const int rc = check_launch(what)) return rc;
  const long plane = (long)d->N * d->H * d->W;
  if (dbias) {
    wgrad_bf16_bias_kernel<<<dim3((unsigned)d->Cout, (unsigned)p.bias_slices), 256, 0, st>>>(g, bias_part, d->B, d->Cout, plane);
    if (const int rc = check_launch("conv3d_wgrad_bf16(bias)")) return rc;
  }
  const long total = (long)d->Cout * a.cin_g * 27;
  long rb = (total + 255) / 256;
  if (rb > 8192) rb = 8192;
  wgrad_bf16_reduce_kernel<<<(unsigned)rb, 256, 0, st>>>(a.ws, dw, p.slots, a.cout_g, a.cin_g, total, bias_part, p.bias_slices,
                                                         d->Cout, dbias, d->bias_scale);
  return check_launch("conv3d_wgrad_bf16(reduce)");
}
