// Shared host- and device-side helpers for libtmdiff_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <type_traits>

#include "tmdiff_hip.h"

namespace tmdiff {

constexpr int kWave = 64;  // CDNA wavefront

char* last_error_buf();  // thread-local, 512 bytes (abi.cpp)

inline int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(last_error_buf(), 512, fmt, ap);
  va_end(ap);
  return code;
}

#define TMDIFF_REQUIRE(cond, ...) \
  do {                            \
    if (!(cond)) return tmdiff::fail(TMDIFF_E_INVALID, __VA_ARGS__); \
  } while (0)

inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(TMDIFF_E_LAUNCH, "%s: %s", what, hipGetErrorString(e));
  return TMDIFF_OK;
}

inline hipStream_t as_stream(tmdiff_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

__host__ __device__ inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// Row stride of a per-(sample, channel) shift / scale bank (tmdiff_hip.h): a stride > 0 is used as it is, 0 means dense rows
// of c channels, a negative stride means one row broadcast over the batch (stride 0).
inline int bank_stride(int s, int c) { return s > 0 ? s : (s < 0 ? 0 : c); }

// Experiment switches read from the environment.  Callers keep the value in a function-local static: each switch is read
// once per process.
inline bool env_flag(const char* name) { return getenv(name) != nullptr; }   // set at all
inline bool env_off(const char* name) {                                       // set to "0..."
  const char* e = getenv(name);
  return e && e[0] == '0';
}
inline long env_long(const char* name, long dflt) {
  const char* e = getenv(name);
  return e ? atol(e) : dflt;
}
inline double env_double(const char* name, double dflt) {
  const char* e = getenv(name);
  return e ? atof(e) : dflt;
}

using f32x16 = __attribute__((ext_vector_type(16))) float;   // one 32x32 MFMA accumulator (16 registers per lane)

// bf16 operands of v_mfma_f32_32x32x16_bf16: eight values per lane.  pack_bf16x2 is THE fp32 -> bf16 rounding of the library
// (round to nearest even, the conversion of the __bf16 type): two values as one dword, `lo` in the low half.  conv3d_bf16.hip
// and wgrad_bf16.hip stage their operands through it.
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
__device__ __forceinline__ unsigned pack_bf16x2(float lo, float hi) {
  union { __attribute__((ext_vector_type(2))) __bf16 h; unsigned u; } p;
  p.h[0] = (__bf16)lo, p.h[1] = (__bf16)hi;
  return p.u;
}

// compile-time loop: f(std::integral_constant<int, I>) for I in [B, E) -- indices must be constants so that
// register arrays indexed by them are addressed statically (a runtime index would send them to scratch).
template <int B, int E, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (B < E) {
    f(std::integral_constant<int, B>{});
    static_for<B + 1, E>(f);
  }
}

// XCD-aware block id: blocks b and b+8 share an XCD (round-robin dispatch), so hand each XCD a
// contiguous run of logical tiles -- neighbouring tiles (same input box, other channel tile;
// adjacent boxes sharing halo lines) then hit in that XCD's L2.  Bijective for any grid size.
__device__ __forceinline__ unsigned xcd_remap(unsigned bid, unsigned nwg) {
  const unsigned q = nwg / 8, r = nwg % 8, xcd = bid % 8, k = bid / 8;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
}

// Two workgroups share a CU (LDS-limited) and one matrix pipe per SIMD.  Launched together and with equal tile times they
// stay in lockstep for the whole launch: both run their MFMA phases together (each at half the pipe) and both reach their
// epilogues together -- the pipe idles while every CU of the chip stores its outputs at once (HBM-bound burst: 64 -> 64 at
// 64x64, B = 32 writes / reads 0.8 GB per launch in four bursts).  Delaying the second resident workgroup of every CU ONCE,
// by about an epilogue, puts the pairs in anti-phase for good: one computes at the full pipe rate while its partner stores.
// The second resident is the one whose LDS allocation does not start at 0 (HW_REG_LDS_ALLOC, base field).  Only blocks
// below first_round (resident at launch) wait.  The Winograd kernels take it for experiments (conv3d_wino.hip, conv3d_wf.hip).
__device__ __forceinline__ void stagger_start(int cycles, unsigned first_round) {
  if (cycles <= 0 || blockIdx.x >= first_round) return;
  const unsigned lds_alloc = __builtin_amdgcn_s_getreg(6 | (0 << 6) | (11 << 11));   // hwreg(HW_REG_LDS_ALLOC, 0, 12): LDS_BASE
  if (lds_alloc == 0) return;
  const unsigned long long t0 = __builtin_amdgcn_s_memtime();
  while ((long long)(__builtin_amdgcn_s_memtime() - t0) < (long long)cycles) __builtin_amdgcn_s_sleep(32);
}

// One step of a tile-index decode: the index along an extent of n tiles, and the block id of the outer extents left in id.
// (integer division runs on the VALU; readfirstlane moves the wave-uniform result back to an SGPR)
__device__ __forceinline__ int take(unsigned& id, int n) {
  const int i = __builtin_amdgcn_readfirstlane(id % n);
  id /= n;
  return i;
}

// Per-channel vectors of an MFMA epilogue: lane l (and l + 32) holds, for channel co0 + m*32 + (l & 31) of group g, the bias
// times bias_scale and the second output's shift and scale of sample b (0 / 0 / 1 where absent).  CLAMPED: every load at a
// valid address -- a channel past cout_g reads the group's last one, an absent bias reads a.wp (the fused kernel, whose
// channel tiles may be ragged).  The fields are read into locals and the values gathered in local arrays: a store through
// the caller's arrays could alias a field, and the loads and tests would then stay inside the loop.
template <int MSUB, bool CLAMPED = false, class Args>
__device__ __forceinline__ void load_channel_vectors(const Args& a, int b, int g, int co0, int l31, float (&bias_v)[MSUB],
                                                     float (&sh2_v)[MSUB], float (&sc2_v)[MSUB]) {
  const float* bias = a.bias;
  const float bias_scale = a.bias_scale;
  const int cout_g = a.cout_g;
  const bool has_sh2 = a.y2 && a.y2_shift, has_sc2 = a.y2 && a.y2_scale;
  float bv[MSUB], sv[MSUB], cv[MSUB];
#pragma unroll
  for (int m = 0; m < MSUB; ++m) {
    if constexpr (CLAMPED) {
      const float* bp = bias ? bias + g * cout_g + min(co0 + m * 32 + l31, cout_g - 1) : a.wp;
      const float raw = *bp;
      bv[m] = bias ? bias_scale * raw : 0.f;
    } else {
      bv[m] = bias ? bias[g * cout_g + co0 + m * 32 + l31] * bias_scale : 0.f;
    }
    const int col = CLAMPED ? g * cout_g + min(co0 + m * 32 + l31, cout_g - 1) : g * cout_g + co0 + m * 32 + l31;
    sv[m] = has_sh2 ? a.y2_shift[(long)b * a.y2_shift_stride + col] : 0.f;
    cv[m] = has_sc2 ? a.y2_scale[(long)b * a.y2_scale_stride + col] : 1.f;
  }
#pragma unroll
  for (int m = 0; m < MSUB; ++m) bias_v[m] = bv[m], sh2_v[m] = sv[m], sc2_v[m] = cv[m];
}

// source of zero padding / filler lanes of the LDS-DMA staging (internal linkage: one copy per translation unit)
static __device__ const float4 kZero4 = {0.f, 0.f, 0.f, 0.f};

__device__ __forceinline__ float silu_f(float v) {
  // x * sigmoid(x); __expf -> v_exp_f32 on a pre-scaled argument, 1 ulp-level accurate for our range
  return v / (1.0f + __expf(-v));
}

// Sums over a wave (every lane gets the total; fixed butterfly order) and over a workgroup of 256 threads (red: 4 floats of
// LDS; the leading barrier lets consecutive calls share it).  The norm kernels and their backward (attention.hip, norm_bwd.hip).
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// The same in double, for every workgroup size and any number of values per lane: stats.h.

// dbias[c] = bias_scale * sum_k part[k * cout + c], k ascending (deterministic): one workgroup of 256 threads finishes the bias
// gradient from the [slot][cout] partial sums a weight-gradient kernel left in its workspace (backward.hip, wgrad_bf16.hip).
__device__ __forceinline__ void finish_bias_grad(const float* __restrict__ part, int slots, int cout, float* __restrict__ dbias,
                                                 float bias_scale) {
  for (int c = threadIdx.x; c < cout; c += 256) {
    float t = 0.f;
    for (int k = 0; k < slots; ++k) t += part[(long)k * cout + c];
    dbias[c] = bias_scale * t;
  }
}

// Channel c of an input that is the concatenation of a.nseg (1..3) segments of a.seg_c[] channels (the kernels that read NCDHW
// segments plane by plane): declares seg (the segment), cs (the channel inside it) and segc (the segment's channel count).
// A macro on purpose: every function form tried (reference outputs, a returned struct, scalar arguments) changed the ISA of the
// kernels that use it (prologue_apply_kernel: 529 - 564 instructions where this text gives 563; branches and single-dword scalar
// loads in place of selects); expanded as text, the four kernels compile to the instructions they had with the decode written out.
#define TMDIFF_SEGMENT_OF(a, c, seg, cs, segc)                                     \
  int cs = (c), seg = 0;                                                           \
  if ((a).nseg > 1 && cs >= (a).seg_c[0]) { cs -= (a).seg_c[0]; seg = 1; }         \
  if (seg == 1 && (a).nseg > 2 && cs >= (a).seg_c[1]) { cs -= (a).seg_c[1]; seg = 2; } \
  const int segc = seg == 0 ? (a).seg_c[0] : (seg == 1 ? (a).seg_c[1] : (a).seg_c[2])

// Dropout keep factor of element `idx` under `seed`: 1/(1-p) with probability 1-p, else 0.  Counter-based (splitmix64
// finaliser of idx + seed * golden ratio): every kernel that needs the mask recomputes it.  thresh = p * 2^32.
__device__ __forceinline__ float drop_keep(uint64_t seed, uint64_t idx, uint32_t thresh, float inv_keep) {
  uint64_t z = idx + seed * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (uint32_t)(z >> 32) >= thresh ? inv_keep : 0.f;
}
inline uint32_t drop_threshold(float p) {
  const double t = (double)p * 4294967296.0;
  return t >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)t;
}

// x' = act(x + shift[b,c]) * scale[b,c] * mask of the descriptor's (possibly segmented) input, written densely as
// [B, Cin, N, H, W] (backward.hip).  Used by the weight-gradient kernel and the staged forward convolution.
int launch_prologue_apply(const tmdiff_conv3d_desc* d, float* xp, hipStream_t st);

// The input carries a prologue (shift / scale / mask / activation / dropout): x' is not the raw input.  A kernel that reads one
// dense tensor has x' materialised when this holds -- or, where it cannot walk segments itself, when nseg > 1 (the caller's term).
inline bool input_prologue(const tmdiff_conv3d_desc* d) {
  return d->in_shift || d->in_scale || d->in_mask || d->in_act || d->drop_p > 0.f;
}

// ---- Host path shared by the weight-gradient entry points (backward.hip, wgrad_wino.hip, wgrad_bf16.hip) --------------------

// Split-K over the position boxes of a weight gradient.  `units` workgroups per split, `per_round` of them resident at a time:
// the split count that minimises  rounds x (boxes per workgroup + overhead)  -- overhead: a workgroup's prologue and
// partial-sum stores, in boxes -- among 1 .. smax; ties go to the smaller count (less to reduce), and no split is empty.
struct Splits {
  int splits, boxes_per_split;
};
inline Splits choose_splits(long total_boxes, long units, long per_round, double overhead, long smax) {
  long best_s = 1;
  double best_cost = 1e30;
  if (smax > total_boxes) smax = total_boxes;
  for (long s = 1; s <= smax; ++s) {
    const long bps = (total_boxes + s - 1) / s;
    const long s_eff = (total_boxes + bps - 1) / bps;
    const long rounds = (units * s_eff + per_round - 1) / per_round;
    const double cost = (double)rounds * ((double)bps + overhead);
    if (cost < best_cost - 1e-9) { best_cost = cost; best_s = s_eff; }
  }
  Splits r;
  r.boxes_per_split = (int)((total_boxes + best_s - 1) / best_s);
  r.splits = (int)((total_boxes + r.boxes_per_split - 1) / r.boxes_per_split);
  return r;
}

// Workspace of a weight gradient: [split-K partial sums | bias partials | x'], the first two areas rounded up to 16 bytes; x'
// [B, Cin, N, H, W] only where the kernel cannot read the first segment as it stands (needs_xp).
struct WgradWorkspace {
  size_t partial_floats, bias_floats, xp_floats;
  size_t bytes() const { return (partial_floats + bias_floats + xp_floats) * sizeof(float); }
  float* partials(void* ws) const { return static_cast<float*>(ws); }
  float* bias(void* ws) const { return partials(ws) + partial_floats; }
  // *src = the dense tensor the kernel reads: the first segment, or x' written into the workspace by the prologue pass
  int stage_input(const tmdiff_conv3d_desc* d, void* ws, hipStream_t st, const float** src) const {
    *src = d->seg_x[0];
    if (!xp_floats) return TMDIFF_OK;
    float* xp = bias(ws) + bias_floats;
    *src = xp;
    return launch_prologue_apply(d, xp, st);
  }
};
inline WgradWorkspace wgrad_workspace(size_t partial_floats, size_t bias_floats, bool needs_xp, const tmdiff_conv3d_desc* d) {
  return {(partial_floats + 3) / 4 * 4, (bias_floats + 3) / 4 * 4, needs_xp ? (size_t)d->B * d->Cin * d->N * d->H * d->W : 0};
}

// Tile configuration and split-K factor of a fp32 3x3x3 launch -- one rule for the fused kernel (conv3d.hip), the staged
// kernel (conv3d_dma.hip) and the workspace query, so that the two kernels always split identically.
//   tile 0: 128 positions x 64 channels (2x8x8 box)     tile 1: 256 x 64 (4x8x8)
//   tile 2: 512 positions x 32 channels (4x8x16 box)    tile 3: 256 x 32 (4x8x8)
struct Conv3Plan {
  int tile;
  long blocks;   // workgroups without splitting
  int ksplit;    // 1 = no split; else the chunks (4 input channels each) are divided into ksplit equal ranges
};
Conv3Plan plan_conv3(const tmdiff_conv3d_desc* d);
// The shape rule of the dwordx4 epilogue (epilogue.h) for an output of W columns and `plane` positions: W % 4 == 0, 16-byte
// aligned outputs / residual, planes of at most 2^23 positions (it addresses up to 128 channels of a sample through one
// descriptor of 32-bit offsets).  epilogue_vec_ok: the same, unless TMDIFF_EPILOGUE_VEC=0 (conv3d.hip; experiments).
inline bool epilogue_vec_shape(const tmdiff_conv3d_desc* d, int W, long plane) {
  return W % 4 == 0 && aligned16(d->y) && aligned16(d->residual) && (d->y2_bf16 || aligned16(d->y2)) && plane <= (1L << 23);
}
bool epilogue_vec_ok(const tmdiff_conv3d_desc* d, int W, long plane);

// sum of the split-K partials + epilogue (conv3d.hip)
struct SplitKReduceArgs {
  const float* part;
  int ksplit;
  int B, Cout;
  long plane;
  const float* bias;
  float bias_scale;
  const float* residual;
  float out_scale;
  float* y;
  float* y2;
  const float* y2_shift;
  const float* y2_scale;
  int y2_shift_stride, y2_scale_stride, y2_act;
};
int launch_splitk_reduce(const SplitKReduceArgs& r, hipStream_t st);

// Split-K over a lent workspace (tmdiff_conv3d_desc.splitk_ws): the bytes of partial outputs [ks][B][Cout][plane] a launch split
// `ks` ways writes (0: no split), the workspace when it is lent, large enough and aligned (else NULL: the launch runs unsplit),
// and the reduction that sums the partials and applies the epilogue (bias_scale: the caller's, factors included).
inline size_t splitk_bytes(int ks, const tmdiff_conv3d_desc* d, long plane) {
  return ks > 1 ? (size_t)ks * d->B * d->Cout * plane * sizeof(float) : 0;
}
inline float* lend_splitk(const tmdiff_conv3d_desc* d, int ks, long plane) {
  const bool ok = ks > 1 && d->splitk_ws && (size_t)d->splitk_ws_bytes >= splitk_bytes(ks, d, plane) && aligned16(d->splitk_ws);
  return ok ? static_cast<float*>(d->splitk_ws) : nullptr;
}
template <class Args>
int finish_splitk(const Args& a, const tmdiff_conv3d_desc* d, long plane, float bias_scale, hipStream_t st) {
  const SplitKReduceArgs r{a.part, a.ksplit, d->B, d->Cout, plane, d->bias, bias_scale, d->residual, d->out_scale, d->y, d->y2,
                           d->y2_shift, d->y2_scale, a.y2_shift_stride, a.y2_scale_stride, d->y2_act};
  return launch_splitk_reduce(r, st);
}

// ---- Descriptor checks of the convolution entry points.  Each returns TMDIFF_OK or fails with a message that begins with the
// entry point's name `what`. -----------------------------------------------------------------------------------------------

// extents (B may be 0), ksize 1 or 3, groups 1 or 3, Cin and Cout positive multiples of groups, 1..3 input segments
inline int check_head(const tmdiff_conv3d_desc* d, const char* what) {
  TMDIFF_REQUIRE(d->B >= 0 && d->N > 0 && d->H > 0 && d->W > 0, "%s: bad extents B=%d N=%d H=%d W=%d", what, d->B, d->N, d->H, d->W);
  TMDIFF_REQUIRE(d->ksize == 1 || d->ksize == 3, "%s: ksize=%d (1 or 3)", what, d->ksize);
  TMDIFF_REQUIRE(d->groups == 1 || d->groups == 3, "%s: groups=%d (1 or 3)", what, d->groups);
  TMDIFF_REQUIRE(d->Cin > 0 && d->Cout > 0 && d->Cin % d->groups == 0 && d->Cout % d->groups == 0, "%s: Cin=%d Cout=%d groups=%d",
                 what, d->Cin, d->Cout, d->groups);
  TMDIFF_REQUIRE(d->nseg >= 1 && d->nseg <= 3, "%s: nseg=%d", what, d->nseg);
  return TMDIFF_OK;
}

// the d->nseg segments: non-NULL, non-empty and, with `aligned`, 16-byte aligned; channels summing to Cin.  A segment whose
// channel count is not a multiple of `unit` fails with TMDIFF_E_UNSUPPORTED.
inline int check_segments(const tmdiff_conv3d_desc* d, const char* what, bool aligned = false, int unit = 1) {
  int csum = 0;
  for (int i = 0; i < d->nseg; ++i) {
    TMDIFF_REQUIRE(d->seg_x[i] && d->seg_c[i] > 0 && (!aligned || aligned16(d->seg_x[i])), "%s: segment %d is empty%s", what, i,
                   aligned ? " / unaligned" : "");
    if (d->seg_c[i] % unit) return fail(TMDIFF_E_UNSUPPORTED, "%s: segment of %d channels", what, d->seg_c[i]);
    csum += d->seg_c[i];
  }
  TMDIFF_REQUIRE(csum == d->Cin, "%s: segments hold %d channels, Cin=%d", what, csum, d->Cin);
  return TMDIFF_OK;
}
// the same as a predicate (nseg included; support queries)
inline bool segments_ok(const tmdiff_conv3d_desc* d) {
  if (d->nseg < 1 || d->nseg > 3) return false;
  int csum = 0;
  for (int i = 0; i < d->nseg; ++i) {
    if (!d->seg_x[i] || d->seg_c[i] <= 0) return false;
    csum += d->seg_c[i];
  }
  return csum == d->Cin;
}

// groups = 3 takes one segment or three equal ones
inline int check_group_segments(const tmdiff_conv3d_desc* d, const char* what) {
  TMDIFF_REQUIRE(d->groups != 3 || d->nseg == 1 || (d->nseg == 3 && d->seg_c[0] == d->seg_c[1] && d->seg_c[1] == d->seg_c[2]),
                 "%s: groups=3 wants 1 segment or 3 equal ones", what);
  return TMDIFF_OK;
}

// a mask tensor or in-kernel dropout, not both; check_dropout: and 0 <= drop_p < 1
inline int check_mask_or_dropout(const tmdiff_conv3d_desc* d, const char* what) {
  TMDIFF_REQUIRE(!(d->in_mask && d->drop_p > 0.f), "%s: give either a mask tensor or drop_p, not both", what);
  return TMDIFF_OK;
}
inline int check_dropout(const tmdiff_conv3d_desc* d, const char* what) {
  if (const int rc = check_mask_or_dropout(d, what)) return rc;
  TMDIFF_REQUIRE(d->drop_p >= 0.f && d->drop_p < 1.f, "%s: drop_p=%g (0 <= drop_p < 1)", what, (double)d->drop_p);
  return TMDIFF_OK;
}

// Grid of a tiled launch: `blocks` workgroups, whose ids the kernels decode in 32 bits; set_grid also sets a.total_blocks.  Fails
// with a message that begins with the kernel's name `what`.
inline int check_grid(long blocks, const char* what, int code = TMDIFF_E_INVALID) {
  if (blocks <= 0 || blocks > 0x7fffffffL) return fail(code, "%s: grid of %ld blocks", what, blocks);
  return TMDIFF_OK;
}
template <class Args>
int set_grid(Args& a, long blocks, const char* what) {
  if (const int rc = check_grid(blocks, what)) return rc;
  a.total_blocks = (unsigned)blocks;
  return TMDIFF_OK;
}

// A lent workspace of `bytes` bytes at `ptr`: at least `need` bytes, 8-byte aligned -- and with it the pointers o1, o2 (NULL
// passes) that the message names in `as`.
inline int check_workspace(const char* what, const void* ptr, size_t bytes, size_t need, const char* as = "", const void* o1 = nullptr,
                           const void* o2 = nullptr) {
  const uintptr_t low = reinterpret_cast<uintptr_t>(ptr) | reinterpret_cast<uintptr_t>(o1) | reinterpret_cast<uintptr_t>(o2);
  TMDIFF_REQUIRE(bytes >= need && (low & 7u) == 0, "%s: workspace of %zu bytes, %zu needed (8-byte aligned%s)", what, bytes, need, as);
  return TMDIFF_OK;
}

// an element count the kernels index in 32 bits: fewer than 2^31 elements
inline bool fits_int32(double elements) { return elements <= 2147483647.0; }

// ---- Descriptor fields of the kernels' argument structs (host side).  Each sets only the fields it names. ------------------

// the input segments; the unused ones get (pad_c, pad_x)
template <class Args>
void set_segments(Args& a, const tmdiff_conv3d_desc* d, int pad_c, const float* pad_x) {
  for (int i = 0; i < 3; ++i) {
    a.seg_c[i] = i < d->nseg ? d->seg_c[i] : pad_c;
    a.seg_x[i] = i < d->nseg ? d->seg_x[i] : pad_x;
  }
}
// the input's shift / scale banks (in_act and in_mask are the caller's: not every kernel has them)
template <class Args>
void set_input_prologue(Args& a, const tmdiff_conv3d_desc* d) {
  a.in_shift = d->in_shift; a.in_scale = d->in_scale;
  a.shift_stride = bank_stride(d->in_shift_stride, d->Cin);
  a.scale_stride = bank_stride(d->in_scale_stride, d->Cin);
}
// in-kernel dropout (drop_inv > 0): common.h drop_keep
template <class Args>
void set_dropout(Args& a, const tmdiff_conv3d_desc* d) {
  a.drop_seed = d->drop_seed; a.drop_seed_dev = d->drop_seed_dev; a.drop_thresh = drop_threshold(d->drop_p);
  a.drop_inv = d->drop_p > 0.f ? 1.0f / (1.0f - d->drop_p) : 0.f;
}
// bias and epilogue: out = (conv + bias * bias_scale + residual) * out_scale, the second output y2 = act2(out + shift2) * scale2
// (a caller with a factor on the bias applies it to a.bias_scale afterwards)
template <class Args>
void set_outputs(Args& a, const tmdiff_conv3d_desc* d) {
  a.bias = d->bias; a.bias_scale = d->bias_scale;
  a.residual = d->residual; a.out_scale = d->out_scale; a.y = d->y;
  a.y2 = reinterpret_cast<decltype(a.y2)>(d->y2); a.y2_shift = d->y2_shift; a.y2_scale = d->y2_scale; a.y2_act = d->y2_act;
  a.y2_shift_stride = bank_stride(d->y2_shift_stride, d->Cout);
  a.y2_scale_stride = bank_stride(d->y2_scale_stride, d->Cout);
}

// 1x1x1 forward through the LDS-free bandwidth kernel (conv1.hip); TMDIFF_E_UNSUPPORTED = shape not taken.
int conv1_fp32_try(const tmdiff_conv3d_desc* d, hipStream_t st, bool dry = false);   // dry: no launch, TMDIFF_OK = the 16-byte kernel on a raw input

}  // namespace tmdiff
