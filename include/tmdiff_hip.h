/* tmdiff_hip.h -- C ABI of libtmdiff_hip.so: the MI355X (gfx950) kernels of the TMDiff
 * denoising hot path.
 *
 * The reference (codgodtao/TMDiff) has no FFI of its own: its hot path runs through
 * PyTorch ATen.  Each entry point below therefore replaces the ATen call sequence of one
 * reference site (file:line given per function).  Conventions:
 *   - plain pointers + sizes + a hipStream_t passed as void*; no torch types;
 *   - every function returns int: 0 = TMDIFF_OK, negative = TMDIFF_E_*; nothing throws
 *     across the boundary; tmdiff_last_error_string() describes the last failure of the
 *     calling thread;
 *   - the library never allocates or frees device memory and never synchronises: the
 *     caller owns inputs, outputs and workspaces (so calls are HIP-graph capturable);
 *   - all tensors are dense fp32, 5-D activations are [B, C, N, H, W] (N = spectral
 *     bands = the conv "depth" axis), row-major, 16-byte aligned base pointers.
 */
#ifndef TMDIFF_HIP_H
#define TMDIFF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TMDIFF_ABI_VERSION 6

#define TMDIFF_OK 0
#define TMDIFF_E_INVALID (-1)     /* bad argument / shape */
#define TMDIFF_E_UNSUPPORTED (-2) /* valid but not implemented configuration */
#define TMDIFF_E_LAUNCH (-3)      /* HIP reported an error at launch */

typedef void* tmdiff_stream_t; /* hipStream_t */

int tmdiff_version(void);
const char* tmdiff_last_error_string(void);

/* ------------------------------------------------------------------------------------
 * conv3d, kernel 3x3x3 (pad 1) or 1x1x1 (pad 0), stride 1, groups 1 or 3.
 * Replaces nn.Conv3d / F.conv3d and modulated_conv3d
 * (GeneralModel/Hyper_unet_general.py:51-77, :161-164, :224-231, :260, :344-361) together
 * with the elementwise ops the reference runs around them:
 *   prologue  x' = act(x + in_shift[b,c]) * in_scale[b,c] * in_mask[b,c,n,h,w]
 *             (temb shift :239, :401; Swish :242, :245, :371, :402; modulation :69 folded
 *             from the weights onto the input channels; Dropout mask :243, :246, :403)
 *   epilogue  y = (conv(x') + bias_scale*bias[co] + residual) * out_scale
 *             (bias; skip additions :249, :408; the 2x of convH_0 :381 via bias_scale)
 * The input may be given as up to three channel segments that the reference would
 * torch.cat first (Hyper_unet_general.py:631-634); for groups == 3 segment g is group g's
 * input (the cat of the three wavelet high bands at :381).
 * ------------------------------------------------------------------------------------ */
typedef struct tmdiff_conv3d_desc {
  int32_t B, N, H, W;
  int32_t Cin, Cout;   /* totals over all groups */
  int32_t groups;      /* 1 or 3 */
  int32_t ksize;       /* 1 or 3 */
  int32_t nseg;        /* 1..3 input segments */
  int32_t seg_c[3];    /* channels per segment, sum == Cin (groups==3: each Cin/3) */
  const float* seg_x[3];
  const float* w_packed; /* from tmdiff_conv3d_pack_weights (or _bf16 for tmdiff_conv3d_fwd_bf16) */
  const float* bias;     /* [Cout] or NULL */
  float bias_scale;
  const float* in_shift; /* [B, Cin] (row stride in_shift_stride floats) or NULL */
  const float* in_scale; /* [B, Cin] (row stride in_scale_stride floats) or NULL */
  int32_t in_shift_stride; /* 0 = dense rows (Cin); > 0 = row stride in floats (a layer's slice of a bank of */
  int32_t in_scale_stride; /* projections); -1 = one row broadcast over the batch (one prompt for all samples) */
  const float* in_mask;  /* [B, Cin, N, H, W] multiplicative mask (dropout) or NULL */
  int32_t in_act;        /* 0 = identity, 1 = SiLU */
  const float* residual; /* [B, Cout, N, H, W] or NULL */
  float out_scale;
  float* y;              /* [B, Cout, N, H, W]; may be NULL when only y2 is wanted */
  /* Optional second output: the consumer's prologue applied to this convolution's result,
   *   y2 = act2(y + y2_shift[b,co]) * y2_scale[b,co]
   * so that the consumer reads a plain tensor (e.g. conv20 -> conv21 of a ResBlock, Hyper_unet_general.py:244-248:
   * conv21's SiLU and text modulation are applied where conv20's result is produced).  y2_bf16 == 0: fp32
   * [B, Cout, N, H, W]; != 0: bf16 units of 8 channels [B][Cout/8][N*H*W] as tmdiff_conv3d_fwd_bf16 packs them
   * (only the bf16 entry point writes that form; Cout/groups a multiple of 32).  Strides as in_shift_stride. */
  float* y2;
  const float* y2_shift;
  const float* y2_scale;
  int32_t y2_shift_stride, y2_scale_stride;
  int32_t y2_act;
  int32_t y2_bf16;
  /* != 0: seg_x[0] is not fp32 but the bf16 units [B][Cin/8][N*H*W] a producer wrote as its y2 (prologue already
   * applied): nseg 1, no shift / scale / act / mask.  Only tmdiff_conv3d_fwd_bf16 (3x3x3) accepts it; it then skips
   * its pack pass and needs no workspace. */
  int32_t x_bf16;
  /* Optional split-K workspace (fp32 3x3x3 entry points tmdiff_conv3d_fwd / _fwd_staged only).  A launch whose grid
   * would leave most of the 256 CUs idle (single images: B = 1 at every level of the UNet; the 8x8 / 16x16 levels at
   * small batches) is split over the input channels: `ksplit` workgroups per output tile accumulate disjoint channel
   * ranges into partial outputs [ksplit][B][Cout][N*H*W] here, and a second kernel sums them in a fixed order and
   * applies the epilogue (deterministic; the fused and the staged entry point split identically, so they still agree
   * bit for bit).  NULL = never split.  Size: tmdiff_conv3d_fwd_splitk_workspace_bytes(d) (0 = this launch does not
   * split); 16-byte aligned. */
  void* splitk_ws;
  int64_t splitk_ws_bytes;
  /* In-kernel dropout (training; nn.Dropout(p) at Hyper_unet_general.py:230, :243-246, :349, :403): drop_p > 0 multiplies
   * the prologue output by a Bernoulli(1 - p) keep mask scaled by 1 / (1 - p) that is a pure function of
   * (drop_seed, element index ((b * Cin + c) * N*H*W + pos)) -- a counter-based hash (splitmix64 finaliser), so the
   * forward, tmdiff_conv3d_wgrad and tmdiff_conv3d_prologue_bwd regenerate the same mask from the same descriptor and no
   * mask tensor exists.  in_mask (a caller-supplied mask tensor, parity runs) must then be NULL.  fp32 entry points only. */
  uint64_t drop_seed;
  float drop_p;
  /* Optional DEVICE word added to drop_seed when the kernel starts (NULL: none).  A launch recorded into a HIP graph is
   * replayed with the arguments it was captured with; with the per-step part of the seed in device memory (one 8-byte word
   * the step bumps before the graph runs) every replay still draws a fresh mask -- and forward, weight gradient and
   * prologue backward of one step still agree, since all three read the same word.  (ABI v6) */
  const uint64_t* drop_seed_dev;
  /* Optional folded "residual convolution" (tmdiff_conv3d_wf_fwd, tmdiff_conv3d_w2_fwd; ABI v6): y = (conv(x') + bias + rc_w^T rc_x) * out_scale,
   * i.e. the 1x1x1 res_conv of a ResBlock (Hyper_unet_general.py:231, :248) on the block's RAW input rc_x [B, rc_cin, N, H, W],
   * accumulated on the matrix pipe where its consumer conv21 would have added it -- no launch of its own, its result never
   * written and read back.  rc_w = the weight [Cout, rc_cin, 1, 1, 1] as PyTorch holds it (contiguous, NOT packed); the
   * caller adds res_conv's bias into `bias`.  Needs groups 1, rc_cin % 32 == 0 (at most 512), residual NULL and planes wider
   * than 8 columns; else TMDIFF_E_UNSUPPORTED.  (A grid that splits its input channels adds it to the partial sums of range 0.) */
  const float* rc_x;
  const float* rc_w;
  int32_t rc_cin;
  /* Optional third output (tmdiff_conv3d_wf_fwd, tmdiff_conv3d_w2_fwd; ABI v6): the HALVED LL BAND of y, (a + b + c + d) / 4 over every 2 x 2 pixel
   * block, [B, Cout, N, H/2, W/2] -- all a down block reads of its ResBlock's raw output (its Conv_2 path,
   * Hyper_unet_general.py:374, :390, :396), so that neither y nor an LL-only DWT pass over it is needed.  Needs y == NULL and
   * y2 != NULL, 8 bands, even H, W % 4 == 0, planes wider than 8 columns, an unsplit grid; else TMDIFF_E_UNSUPPORTED. */
  float* y_ll;
  /* ... and with y_hi[0..2] != NULL (then y2 == NULL): the WHOLE Haar transform of y instead of y (tmdiff_conv3d_wf_fwd, tmdiff_conv3d_w2_fwd; ABI v6) --
   * y_hi = LH, HL, HH = (a - b + c - d) / 2, (a + b - c - d) / 2, (a - b - c + d) / 2 of every 2 x 2 block (a b / c d), and y_ll = the
   * halved LL band passed through the second output's prologue, act2(LL / 2 + y2_shift) * y2_scale: what a down block whose high
   * bands are kept makes of its Conv_0 output (DWT, then Conv_1's prologue on the LL band; Hyper_unet_general.py:388-396,
   * DWT_IDWT_Functions.py:47-57) without a full-resolution tensor or a transform pass.  Same shape conditions as y_ll. */
  float* y_hi[3];
  /* Optional by-product of a 1x1x1 convolution on the bandwidth kernel (tmdiff_conv3d_fwd, ksize 1; ABI v6): xp_out [B, Cin, N, H, W]
   * receives act(x + xp_shift[b, c]) of every element of the (possibly segmented) input -- the prologue output that ANOTHER
   * convolution of the same input wants (a ResBlock's conv20 beside its res_conv, Hyper_unet_general.py:243-248: both read the
   * concatenated block input, one raw, one through SiLU(x + Dense(e))), written by the kernel that loads every element anyway.
   * xp_shift: [B, Cin] (row stride xp_shift_stride as in_shift_stride) or NULL; xp_act != 0: SiLU.  Taken by the 16-byte form of
   * the kernel (planes of multiples of 4 positions, 16-byte aligned tensors, at least 512 tiles of 512 positions; any prologue of
   * its own except an activation) and by the small-grid form (fewer than 512 tiles of 256 positions, at least 128 input channels
   * per group, a raw input: no in_shift / in_scale / in_act); a sample of fewer than 2^30 elements.  tmdiff_conv3d_fwd_xp_supported()
   * answers for a descriptor; any other launch: TMDIFF_E_UNSUPPORTED. */
  float* xp_out;
  const float* xp_shift;
  int32_t xp_shift_stride, xp_act;
  /* != 0 (tmdiff_conv3d_wf_fwd: even H, W % 4 == 0, a grid that does not split its input channels; tmdiff_conv3d_w2_fwd: 8 bands,
   * even H): y2 is written in
   * "space to depth" form [B, 4 Cout, N, H/2, W/2], channel 4 co + 2 ph + pw holding y2[co][n][2i + ph][2j + pw] -- the input
   * form of tmdiff_conv3d_wfll_fwd (the down blocks' Conv_0 + LL band, Hyper_unet_general.py:371-372, :389, :396). */
  int32_t y2_s2d;
} tmdiff_conv3d_desc;

/* w [Cout, Cin/groups, k, k, k] (PyTorch layout) -> packed [g][ci][tap][co] used by the
 * kernels.  mode 0: forward weights.  mode 1: weights of the data-gradient convolution
 * (taps flipped, ci/co swapped): conv3d_fwd(dy, packed_mode1) == dL/dx'.
 * packed must hold Cout*Cin/groups*k^3 floats. */
int tmdiff_conv3d_pack_weights(const float* w, float* packed, int32_t Cout, int32_t Cin, int32_t ksize,
                               int32_t groups, int32_t mode, tmdiff_stream_t stream);
/* The same for a whole list of weight tensors in ONE launch, both packings at once (a training step re-packs every weight
 * for its forward and its data-gradient convolution after each optimizer update).  `entries_dev` is a DEVICE array; workgroup
 * k works on entry chunk_tensor_dev[k]; chunk_index_dev[k] = tile number within that entry, with bit 30 set for the tiles of
 * the data-gradient packing: an entry needs tmdiff_conv3d_pack_weights_multi_chunks(...) workgroups, the first *n_type_a of
 * them forward-packing tiles (numbered 0..), the rest data-gradient tiles (numbered 0.. | 1<<30).  ksize 1 or 3.  Either
 * destination may be NULL. */
typedef struct tmdiff_pack_entry {
  const float* w;       /* [Cout, Cin/groups, k, k, k] */
  float* packed_fwd;    /* mode 0 */
  float* packed_dgrad;  /* mode 1 */
  int32_t Cout, Cin, ksize, groups;
} tmdiff_pack_entry;
int32_t tmdiff_conv3d_pack_weights_multi_chunks(int32_t Cout, int32_t Cin, int32_t groups, int32_t* n_type_a);
int tmdiff_conv3d_pack_weights_multi(const tmdiff_pack_entry* entries_dev, const int32_t* chunk_tensor_dev,
                                     const int32_t* chunk_index_dev, int32_t n_chunks, tmdiff_stream_t stream);
int tmdiff_conv3d_fwd(const tmdiff_conv3d_desc* d, tmdiff_stream_t stream);
/* 1 when tmdiff_conv3d_fwd writes the by-product d->xp_out for this descriptor (else it would fail with TMDIFF_E_UNSUPPORTED) */
int tmdiff_conv3d_fwd_xp_supported(const tmdiff_conv3d_desc* d);
/* bytes of d->splitk_ws this convolution would use (0: its grid fills the chip, or the shape is not split) */
size_t tmdiff_conv3d_fwd_splitk_workspace_bytes(const tmdiff_conv3d_desc* d);

/* ---- staged variant of tmdiff_conv3d_fwd (same arithmetic, exact fp32, bit-identical results) ----------------
 * Two launches instead of one: the prologue output x' (and the concatenation of the segments) is written once into
 * `workspace` ([B, Cin, N, H, W] fp32, tmdiff_conv3d_fwd_staged_workspace_bytes(d) bytes; 0 and NULL allowed when
 * the input is a single tensor without shift / scale / act / mask), then a convolution whose operands go
 * L2/HBM -> LDS directly (global_load_lds) so that its instruction stream is MFMAs and operand reads only.
 * The kernel itself is 3-6 % faster than the fused one; with the prologue pass it wins where that pass is absent or
 * amortised (plain inputs such as every data-gradient convolution, >= 128 output channels).  3x3x3 only; shapes it does
 * not take (Cin/groups not a multiple of 4, Cout/groups not a multiple of 32, ksize 1) return TMDIFF_E_UNSUPPORTED --
 * use tmdiff_conv3d_fwd. */
int tmdiff_conv3d_fwd_staged_supported(const tmdiff_conv3d_desc* d);
size_t tmdiff_conv3d_fwd_staged_workspace_bytes(const tmdiff_conv3d_desc* d);
int tmdiff_conv3d_fwd_staged(const tmdiff_conv3d_desc* d, void* workspace, tmdiff_stream_t stream);

/* ---- 3x3x3 convolution followed by the scaled Haar LL band, as one strided convolution (exact fp32) -----------
 * Replaces the pair  h = Conv_0(x') ; hLL = dwt(h).LL * ll_scale  of WaveletUPorDown(down=True) where the high bands are
 * not used (reference GeneralModel/Hyper_unet_general.py:371-372, :389, :396; the main branch of WavBEST.forward).  The LL
 * band is linear and local, so the pair equals a convolution with a 3x4x4 kernel and stride (1,2,2) whose weights are
 * sums of the 3x3x3 ones: 48 instead of 4 x 27 multiply-adds per output, same numbers up to fp32 summation order.
 *   d         : the descriptor of the 3x3x3 convolution (N, H, W = INPUT extents, H and W even; one plain fp32 input
 *               without shift / scale / act / mask; groups 1; Cin % 2 == 0, Cout % 64 == 0; bias as for the convolution);
 *               y / y2 / residual are [B, Cout, N, H/2, W/2] and follow the usual epilogue
 *               out = (LL(conv(x) + bias) * ll_scale + residual) * out_scale,  y2 = act2(out + shift2) * scale2.
 *   w_packed  : from tmdiff_conv3d_ll_pack_weights(w [Cout, Cin, 3, 3, 3], ..., ll_scale)
 *               (tmdiff_conv3d_ll_packed_bytes bytes; 0 = shape not supported).
 * Shapes it does not take return TMDIFF_E_UNSUPPORTED (tmdiff_conv3d_ll_supported says so beforehand): run the
 * convolution and tmdiff_haar_dwt2d instead.
 * Small grids are split over the input channels like tmdiff_conv3d_fwd when d->splitk_ws lends
 * tmdiff_conv3d_ll_splitk_workspace_bytes(d) bytes (0: the grid fills the chip). */
int tmdiff_conv3d_ll_supported(const tmdiff_conv3d_desc* d);
size_t tmdiff_conv3d_ll_splitk_workspace_bytes(const tmdiff_conv3d_desc* d);
size_t tmdiff_conv3d_ll_packed_bytes(int32_t Cout, int32_t Cin);
int tmdiff_conv3d_ll_pack_weights(const float* w, float* packed, int32_t Cout, int32_t Cin, float ll_scale,
                                  tmdiff_stream_t stream);
int tmdiff_conv3d_ll_fwd(const tmdiff_conv3d_desc* d, float ll_scale, tmdiff_stream_t stream);

/* ---- 3x3x3 convolution, Winograd F(4,3) / F(2,3) along the band axis (exact-fp32 matrix cores) --------------------
 * 2x (N % 4 == 0: six transformed planes per four bands) or 1.5x (N % 2 == 0: four planes per two bands) fewer multiply-adds.
 * Same descriptor and epilogue as tmdiff_conv3d_fwd (fp32, groups 1 or 3, N even, W % 4 == 0, Cin/groups % 2 == 0,
 * Cout/groups % 32 == 0, no mask tensor (d->drop_p in-kernel dropout is taken); segments and the shift / scale / act
 * prologue are taken).  `workspace` receives the transformed input (tmdiff_conv3d_wino_workspace_bytes(d) = 1.5-2x the
 * input bytes plus a border); d->w_packed comes from tmdiff_conv3d_wino_pack_weights with planes =
 * tmdiff_conv3d_wino_planes(N) (tmdiff_conv3d_wino_packed_bytes bytes).  Results agree with tmdiff_conv3d_fwd to 1e-6
 * relative L2 (F(4,3)) / 4e-7 (F(2,3)). */
int tmdiff_conv3d_wino_supported(const tmdiff_conv3d_desc* d);
int32_t tmdiff_conv3d_wino_planes(int32_t N);                     /* 6, 4, or 0 (odd N) */
int64_t tmdiff_conv3d_wino_blocks(const tmdiff_conv3d_desc* d);   /* workgroups of its grid (no split-K: keep small grids on tmdiff_conv3d_fwd) */
size_t tmdiff_conv3d_wino_workspace_bytes(const tmdiff_conv3d_desc* d);
size_t tmdiff_conv3d_wino_packed_bytes(int32_t Cout, int32_t Cin, int32_t groups, int32_t planes);
/* mode bit 0 clear: w = [Cout, Cin/groups, 3,3,3] of this convolution; set (data gradient): w is the FORWARD convolution's
 * weight [Cin, Cout/groups, 3,3,3] and this convolution (Cin -> Cout) is its transpose with mirrored taps, as
 * tmdiff_conv3d_pack_weights(mode 1).  mode bit 1 (value 2): natural column order (tmdiff_conv3d_wf_fwd) instead of the
 * interleaved 64-channel tiles of tmdiff_conv3d_wino_fwd */
int tmdiff_conv3d_wino_pack_weights(const float* w, float* packed, int32_t Cout, int32_t Cin, int32_t groups,
                                    int32_t mode, int32_t planes, tmdiff_stream_t stream);
/* Multi-tensor form, ONE launch for every (weight, mode) of a network (the finetune step re-packs the Winograd weights of its
 * ~50 convolutions in both forms after every optimizer step).  `entries_dev` is a DEVICE array; workgroup k packs weight rows
 * [chunk_index_dev[k] * tmdiff_conv3d_wino_pack_weights_multi_chunk(), ...) of entry chunk_tensor_dev[k] (a row = the 27 taps of one
 * (output, input channel) pair: numel(w) / 27 rows per entry).  Cout / Cin / groups are
 * those of the weight tensor w = [Cout, Cin/groups, 3,3,3]; mode / planes as tmdiff_conv3d_wino_pack_weights. */
typedef struct tmdiff_wino_pack_entry {
  const float* w;
  float* packed;
  int32_t Cout, Cin, groups, mode, planes, reserved;
} tmdiff_wino_pack_entry;
int32_t tmdiff_conv3d_wino_pack_weights_multi_chunk(void);
int tmdiff_conv3d_wino_pack_weights_multi(const tmdiff_wino_pack_entry* entries_dev, const int32_t* chunk_tensor_dev,
                                          const int32_t* chunk_index_dev, int32_t n_chunks, tmdiff_stream_t stream);
int tmdiff_conv3d_wino_fwd(const tmdiff_conv3d_desc* d, void* workspace, tmdiff_stream_t stream);
/* stage 1: the input-transform pass alone; stage 2: the convolution alone on a workspace that holds it; 0: both */
int tmdiff_conv3d_wino_fwd_stage(const tmdiff_conv3d_desc* d, void* workspace, int32_t stage, tmdiff_stream_t stream);
/* ... and with the prologue output x' [B, Cin, N, H, W] (in-kernel dropout d->drop_p included) also written to xp_out by the
 * transform pass: the finetune path keeps it for the weight gradient */
int tmdiff_conv3d_wino_fwd_xp(const tmdiff_conv3d_desc* d, void* workspace, int32_t stage, float* xp_out, tmdiff_stream_t stream);
/* ... and with the transform chosen by the caller (planes 6 or 4 = what the weights were packed for; 0 = automatic): F(2,3)
 * has twice the tiles along the bands, so it still fills the chip where F(4,3) would not */
int tmdiff_conv3d_wino_fwd_planes(const tmdiff_conv3d_desc* d, void* workspace, int32_t stage, float* xp_out, int32_t planes,
                                  tmdiff_stream_t stream);

/* ---- 3x3x3 convolution, Winograd F(4,3) along the band axis with the input transform INSIDE the kernel -----------
 * (csrc/conv3d_wf.hip).  The whole band axis lies in one workgroup (N = 8: two tiles, N = 4: one), the kernel reads the plain
 * convolution input and forms v = B^T d in LDS between its MFMAs: no transformed copy of the input in HBM, no transform
 * pass.  Same descriptor and epilogue as tmdiff_conv3d_fwd (fp32, groups 1 or 3, N = 8 or 4, W % 4 == 0, Cin/groups % 2 == 0,
 * Cout/groups % 32 == 0, no mask tensor).  An input that is ONE plain tensor (no prologue / dropout: every convolution whose
 * producer applied the consumer's prologue, every data-gradient convolution) -- or, for groups = 3, three plain segments of
 * Cin/3 channels, one per group -- needs no workspace; otherwise `workspace`
 * (tmdiff_conv3d_wf_workspace_bytes(d) = the input's bytes) receives the prologue output x' first (one elementwise pass,
 * as tmdiff_conv3d_fwd_staged).  d->w_packed = tmdiff_conv3d_wino_pack_weights(..., mode | 2, planes 6): the same
 * transformed weights in natural column order.  Replaces, for the Python reference, the F.conv3d / nn.Conv3d calls of
 * GeneralModel/Hyper_unet_general.py:51-77, :161-164, :224-227, :344-361 on 8- and 4-band tensors. */
int tmdiff_conv3d_wf_supported(const tmdiff_conv3d_desc* d);
int64_t tmdiff_conv3d_wf_blocks(const tmdiff_conv3d_desc* d);     /* workgroups of its grid, split-K included */
/* small grids (single images, the deep levels of a small batch) split the input channels over workgroups when d->splitk_ws
 * lends tmdiff_conv3d_wf_splitk_workspace_bytes(d) bytes (0: the grid needs no split); splitk_reduce_kernel sums the ranges
 * in a fixed order and applies the epilogue, as for tmdiff_conv3d_fwd */
size_t tmdiff_conv3d_wf_splitk_workspace_bytes(const tmdiff_conv3d_desc* d);
size_t tmdiff_conv3d_wf_workspace_bytes(const tmdiff_conv3d_desc* d);
/* The launch plan for a convolution of these extents without a descriptor (host-side routing): returns the split-K factor
 * (1 = none) and writes the number of output tiles (workgroups = tiles x factor); 0 = shape not taken.  llm != 0: the composed
 * Conv_0 + LL mode of tmdiff_conv3d_wfll_fwd (Cin, H, W those of the space-to-depth tensor). */
int32_t tmdiff_conv3d_wf_plan(int32_t B, int32_t Cin, int32_t Cout, int32_t N, int32_t H, int32_t W, int32_t groups, int32_t llm,
                              int64_t* tiles);
int tmdiff_conv3d_wf_fwd(const tmdiff_conv3d_desc* d, void* workspace, tmdiff_stream_t stream);

/* ---- 3x3x3 convolution, Winograd in two dimensions for the deep layers: F(4,3) along the bands x F(2,3) along the width ----
 * (csrc/conv3d_w2.hip).  72 instead of tmdiff_conv3d_wf_fwd's 108 multiply-adds per input channel, four bands and column pair,
 * as three launches over Winograd-domain arrays in `workspace`: an input pass (the consumer's shift / scale / act prologue
 * applied on the way), one GEMM per Winograd plane (24 planes, K = 3 row taps x Cin), an output pass with the usual epilogue
 * out = (conv + bias_scale * bias + residual) * out_scale and second output y2.  Takes: fp32, groups 1, ONE input tensor, no
 * mask / dropout, N = 8 or 4, even W <= 16, 4 <= H <= 32, Cin >= 128 (a multiple of 32), Cout >= 256 (a multiple of 64), no
 * xp_out.  tmdiff_conv3d_w2_supported answers 1 for such a descriptor with none of rc_x / y_ll / y_hi / y2_s2d (the plain
 * epilogue: the output pass takes one plane row per workgroup).  tmdiff_conv3d_w2_epilogue_supported answers 1 for those and
 * for the descriptors whose epilogue the row-pair output pass writes (even H): a folded 1x1x1 (rc_x / rc_w / rc_cin under
 * tmdiff_conv3d_wf_fwd's conditions: rc_cin % 32 == 0, at most 512, residual NULL; accumulated on the matrix pipe inside the
 * output pass), and on 8 bands y_ll (y NULL, y2 set), y_ll + y_hi[0..2] (y and y2 NULL) and y2_s2d, as defined at the fields.
 * tmdiff_conv3d_w2_fwd takes exactly the descriptors of the second query; everything else: TMDIFF_E_UNSUPPORTED (use
 * tmdiff_conv3d_wf_fwd).  `workspace`: tmdiff_conv3d_w2_workspace_bytes(d) bytes (the transformed input and
 * the plane products), 16-byte aligned, lent by the caller.  d->w_packed = tmdiff_conv3d_w2_pack_weights(w [Cout, Cin, 3,3,3])
 * (tmdiff_conv3d_w2_packed_bytes bytes: 72 floats per weight pair).  stages: 0 = the whole convolution; else a bit mask of the
 * launches that run (1 input pass, 2 GEMM, 4 output pass: timing).  Agrees with tmdiff_conv3d_fwd to 2e-5 of the output's
 * largest element. */
int tmdiff_conv3d_w2_supported(const tmdiff_conv3d_desc* d);
int tmdiff_conv3d_w2_epilogue_supported(const tmdiff_conv3d_desc* d);
size_t tmdiff_conv3d_w2_workspace_bytes(const tmdiff_conv3d_desc* d);
size_t tmdiff_conv3d_w2_packed_bytes(int32_t Cout, int32_t Cin);
int tmdiff_conv3d_w2_pack_weights(const float* w, float* packed, int32_t Cout, int32_t Cin, tmdiff_stream_t stream);
int tmdiff_conv3d_w2_fwd(const tmdiff_conv3d_desc* d, void* workspace, int32_t stages, tmdiff_stream_t stream);
/* `Conv_0` (3x3x3) of a down block and the halved Haar LL band of its output as ONE convolution (as tmdiff_conv3d_ll_fwd: same
 * descriptor -- H, W the INPUT extents, outputs at half of them, bias multiplied by 2 * ll_scale) WITH Winograd F(4,3) along the
 * bands on top: the LL band acts on (h, w) only, so the composed 3x4x4 stride-2 kernel keeps its three band taps -- 16 x 6 / 4 =
 * 24 multiply-adds per output instead of 48 (and 108 for the convolution + DWT pair).  seg_x[0] is the producer's SPACE-TO-DEPTH
 * second output (y2_s2d above: [B, 4 Cin, N, H/2, W/2]); on it the composed kernel is a stride-1 convolution with 2 x 2 of the
 * 3 x 3 taps per virtual channel, which the kernel of tmdiff_conv3d_wf_fwd runs with a 24-step K loop.  8- and 4-band tensors, W % 8 == 0,
 * Cout % 32 == 0; weights from tmdiff_conv3d_wfll_pack_weights (Cin x 96 x Cout floats). */
int tmdiff_conv3d_wfll_supported(const tmdiff_conv3d_desc* d);
size_t tmdiff_conv3d_wfll_packed_bytes(int32_t Cout, int32_t Cin);
int tmdiff_conv3d_wfll_pack_weights(const float* w, float* packed, int32_t Cout, int32_t Cin, float ll_scale,
                                    tmdiff_stream_t stream);
size_t tmdiff_conv3d_wfll_splitk_workspace_bytes(const tmdiff_conv3d_desc* d);
int tmdiff_conv3d_wfll_fwd(const tmdiff_conv3d_desc* d, float ll_scale, tmdiff_stream_t stream);

/* ---- bf16 compute / fp32 accumulate (WorldView-3 inference) --------------------------
 * Same descriptor and fused prologue / epilogue as tmdiff_conv3d_fwd; activations, bias, residual and output stay
 * fp32 in memory.  The prologue result x' and the weights are rounded to bf16 (round to nearest even), products
 * are accumulated in fp32 on v_mfma_f32_32x32x16_bf16.  d->w_packed must come from tmdiff_conv3d_pack_weights_bf16
 * (tmdiff_conv3d_packed_bf16_bytes bytes; 0 = shape not supported).
 * Supported: Cin/groups a multiple of 8 (ksize 3) or 16 (ksize 1), every segment a multiple of 8 channels,
 * Cout/groups a multiple of 32, no in_mask; anything else returns TMDIFF_E_UNSUPPORTED and the caller keeps using tmdiff_conv3d_fwd (forward only:
 * the training FORWARD runs in fp32 -- this entry point takes no dropout; the opt-in bf16 gradient arithmetic of the finetune step
 * runs its data gradients, plain convolutions of g, through it with weights from tmdiff_conv3d_pack_weights_bf16_dgrad;
 * tmdiff_conv3d_wgrad_bf16 below is the bf16 weight gradient).
 * workspace NULL: one fused kernel (prologue evaluated while staging, per channel tile).  workspace of
 * tmdiff_conv3d_bf16_workspace_bytes(d) bytes: two kernels -- the prologue output is packed to bf16 once
 * ([B][Cin/8][N*H*W] units of 8 channels), then a convolution whose operands go HBM -> LDS directly
 * (global_load_lds) -- the better choice when several channel tiles share the input.  Same results bit for bit.
 * ksize 1 is a bandwidth kernel without LDS (operands built in registers); it ignores the workspace. */
size_t tmdiff_conv3d_packed_bf16_bytes(int32_t Cout, int32_t Cin, int32_t ksize, int32_t groups);
int tmdiff_conv3d_pack_weights_bf16(const float* w, void* packed, int32_t Cout, int32_t Cin, int32_t ksize,
                                    int32_t groups, tmdiff_stream_t stream);
/* The bf16 counterpart of tmdiff_conv3d_pack_weights(..., mode 1): w = [Cout, Cin/groups, 3,3,3] of the FORWARD convolution ->
 * the layout above for its data-gradient convolution (Cout -> Cin channels), taps mirrored and the two channel axes swapped per
 * group, so that tmdiff_conv3d_fwd_bf16(g, packed) == dL/dx' from bf16-rounded g and w.  ksize 3, Cout/groups a multiple of 8;
 * tmdiff_conv3d_packed_bf16_bytes(Cin, Cout, 3, groups) bytes (the convolution itself also wants Cin/groups % 32 == 0). */
int tmdiff_conv3d_pack_weights_bf16_dgrad(const float* w, void* packed, int32_t Cout, int32_t Cin, int32_t ksize,
                                          int32_t groups, tmdiff_stream_t stream);
size_t tmdiff_conv3d_bf16_workspace_bytes(const tmdiff_conv3d_desc* d);
int tmdiff_conv3d_fwd_bf16(const tmdiff_conv3d_desc* d, void* workspace, tmdiff_stream_t stream);

/* ---- backward of the fused convolution (finetune path) ----------------------------------
 * With x' = prologue(x) and y = (conv(x', w) + bias_scale*bias + residual) * out_scale, and g = dL/dy * out_scale:
 *   dL/dresidual = g;  dL/dbias = bias_scale * sum_{b,pos} g      -> tmdiff_channel_sum
 *   dL/dx'       = conv3d_fwd(g, pack_weights(w, mode 1))          (same kernel, roles of Cin/Cout swapped)
 *   dL/dw        = tmdiff_conv3d_wgrad                             (fp32 MFMA, split over the batch/boxes)
 *   dL/dx, dL/dshift, dL/dscale = tmdiff_conv3d_prologue_bwd(dL/dx', x, ...)
 * ATen computes these inside autograd for F.conv3d / nn.Conv3d (Hyper_unet_general.py:74, :244, :372...). */

/* x'[B, Cin, N, H, W] = act(cat(segments) + shift) * scale * mask (or in-kernel dropout): the prologue of the convolution
 * described by d, on its own (the pass tmdiff_conv3d_fwd_staged and tmdiff_conv3d_wgrad run internally).  The finetune path
 * uses it where the convolution itself is tmdiff_conv3d_ll_fwd, which takes a plain input; x' is then kept for the weight
 * gradient. */
int tmdiff_conv3d_prologue_fwd(const tmdiff_conv3d_desc* d, float* xp, tmdiff_stream_t stream);

/* dw [Cout, Cin/groups, k,k,k] (PyTorch layout) = sum_{b,pos} g[b,co,pos] * x'[b,ci,pos+tap]; x' is formed from
 * the segments / shift / scale / mask / act of `d` exactly as in the forward (d->y, residual, bias, w_packed are
 * ignored).  `g` is [B, Cout, N, H, W].  workspace: tmdiff_conv3d_wgrad_workspace_bytes(d) bytes (partial sums).
 * Unlike the forward entry points it takes any group count that divides Cin and Cout. */
size_t tmdiff_conv3d_wgrad_workspace_bytes(const tmdiff_conv3d_desc* d);
int tmdiff_conv3d_wgrad(const tmdiff_conv3d_desc* d, const float* g, float* dw, void* workspace,
                        tmdiff_stream_t stream);
/* The same, and dbias[Cout] = d->bias_scale * sum_{b,pos} g[b,co,pos] on the side (the kernel reads every g element anyway;
 * this replaces a tmdiff_channel_sum pass over g).  dbias NULL = tmdiff_conv3d_wgrad. */
int tmdiff_conv3d_wgrad_bias(const tmdiff_conv3d_desc* d, const float* g, float* dw, float* dbias, void* workspace,
                             tmdiff_stream_t stream);

/* The same weight gradient in the Winograd domain along the band axis (csrc/wgrad_wino.hip): F(3,4), the transpose of the
 * forward's F(4,3) -- dw = A'^T[(G' g) (.) (B^T x')], half the multiply-adds.  Both operands are first transformed into
 * channels-last zero-padded arrays by one pass each (inside the workspace), the accumulation over positions runs on the matrix
 * pipe per Winograd plane, a reduction kernel sums the split partials in a fixed order and applies A'^T.  Takes fp32 3x3x3,
 * groups 1 or 3, N % 4 == 0 (at most 16 bands), W % 4 == 0, any channel counts; _supported() says so (else: tmdiff_conv3d_wgrad;
 * ATen's conv3d backward: Hyper_unet_general.py:74, :244, :372).  Same arguments and result layout as tmdiff_conv3d_wgrad. */
int tmdiff_conv3d_wgrad_wino_supported(const tmdiff_conv3d_desc* d);
size_t tmdiff_conv3d_wgrad_wino_workspace_bytes(const tmdiff_conv3d_desc* d);
int tmdiff_conv3d_wgrad_wino(const tmdiff_conv3d_desc* d, const float* g, float* dw, void* workspace,
                             tmdiff_stream_t stream);
/* ... and dbias[Cout] = d->bias_scale * sum_{b,pos} g on the side (the pass that transforms g sums it up as it reads; fixed
 * summation order).  dbias NULL = tmdiff_conv3d_wgrad_wino. */
int tmdiff_conv3d_wgrad_wino_bias(const tmdiff_conv3d_desc* d, const float* g, float* dw, float* dbias, void* workspace,
                                  tmdiff_stream_t stream);

/* The weight gradient of a 3x3x3 convolution with bf16 operands (csrc/wgrad_bf16.hip): g and x' -- formed from the descriptor exactly as in the forward, in-kernel dropout included -- are each rounded
 * to bf16 (round to nearest even) when staged, the products are summed in fp32 on v_mfma_f32_32x32x16_bf16; the sum over batch
 * and positions is split over workgroups whose fp32 partials a second kernel adds in a fixed order (no atomics: the same bits on
 * every run and in a graph replay).  Same arguments and result layout as tmdiff_conv3d_wgrad_bias; dbias (optional) =
 * bias_scale * sum g of the UNROUNDED g, in a fixed order.  Takes ksize 3, groups 1 or 3, Cin/groups % 8 == 0, Cout/groups % 32 ==
 * 0, any extents tmdiff_conv3d_wgrad takes; _supported() says so, anything else returns TMDIFF_E_UNSUPPORTED without a launch and
 * the caller keeps the fp32 weight gradient.  _slots(): the number of partial sums per element the second kernel adds. */
int tmdiff_conv3d_wgrad_bf16_supported(const tmdiff_conv3d_desc* d);
size_t tmdiff_conv3d_wgrad_bf16_workspace_bytes(const tmdiff_conv3d_desc* d);
int32_t tmdiff_conv3d_wgrad_bf16_slots(const tmdiff_conv3d_desc* d);
int tmdiff_conv3d_wgrad_bf16(const tmdiff_conv3d_desc* d, const float* g, float* dw, float* dbias, void* workspace,
                             tmdiff_stream_t stream);

/* out[c] = scale * sum_{b, p} x[b, c, p]   (x is [B, C, P]); bias gradients. */
int tmdiff_channel_sum(const float* x, float* out, int32_t B, int32_t C, int64_t P, float scale,
                       tmdiff_stream_t stream);

/* Backward of the prologue x' = act(x + shift[b,c]) * scale[b,c] * mask: given gp = dL/dx' [B,Cin,N,H,W] and the
 * forward descriptor `d` (segments, shift, scale, mask, act), writes dL/dx into dx_seg[i] (same segmenting as
 * d->seg_x; NULL = not needed; accumulate[i] != 0 adds to the existing contents) and the per-(b,c) reductions
 * d_shift[B,Cin], d_scale[B,Cin] (NULL = not needed, dense rows). */
int tmdiff_conv3d_prologue_bwd(const tmdiff_conv3d_desc* d, const float* gp, float* const dx_seg[3],
                               const int32_t accumulate[3], float* d_shift, float* d_scale, tmdiff_stream_t stream);
/* Same, with a workspace of tmdiff_conv3d_prologue_bwd_workspace_bytes(d) bytes (0 = not needed): planes are then cut
 * into several workgroups each when B*Cin alone cannot fill the chip (the full-resolution 32-channel layers at small
 * batches); the per-plane sums are finished in a fixed order (deterministic). */
size_t tmdiff_conv3d_prologue_bwd_workspace_bytes(const tmdiff_conv3d_desc* d);
int tmdiff_conv3d_prologue_bwd_ws(const tmdiff_conv3d_desc* d, const float* gp, float* const dx_seg[3],
                                  const int32_t accumulate[3], float* d_shift, float* d_scale, void* workspace,
                                  tmdiff_stream_t stream);
/* Three-operand form: dx_seg[i] = add_seg[i] + dL/dx_i (add_seg[i] == NULL: just dL/dx_i) -- the gradient ANOTHER consumer of the
 * same segment has produced (a ResBlock's identity residual, Hyper_unet_general.py:248) is read here instead of being summed with
 * this one by a launch of its own.  add_seg[i] is only read; dx_seg[i] is a tensor of its own. */
int tmdiff_conv3d_prologue_bwd_add(const tmdiff_conv3d_desc* d, const float* gp, float* const dx_seg[3],
                                   const float* const add_seg[3], float* d_shift, float* d_scale, void* workspace,
                                   tmdiff_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Stem / head pointwise convolutions (bandwidth kernels):
 *  stem: y[b,co,p] = SiLU(w[co]*x[b,p] + bias[co])            AdaptionModulateBEST.conv20 + act (:169-170)
 *        x is given as pan[b,1,H,W] broadcast over N minus ms[b,N,H,W] when `ms` != NULL
 *        (WavBEST.forward :605-608), else x = xin[b,N,H,W] (to3D(x_t) :609).
 *  head: y[b,p] = sum_c w[c]*scale[b,c]*SiLU(x[b,c,p])         FinalBlock act + modulated conv24 (:270-272)
 * ------------------------------------------------------------------------------------ */
int tmdiff_stem_fwd(const float* xin, const float* pan, const float* ms, const float* w, const float* bias, float* y,
                    int32_t B, int32_t Cout, int32_t N, int32_t H, int32_t W, int32_t apply_silu,
                    tmdiff_stream_t stream);
/* The same with the consumer's per-(b, co) modulation folded in: y *= out_scale[b, co] (row stride as in_scale_stride) --
 * conv21 of the stem block (Hyper_unet_general.py:171) then reads a plain tensor. */
int tmdiff_stem_fwd_scaled(const float* xin, const float* pan, const float* ms, const float* w, const float* bias,
                           const float* out_scale, int32_t out_scale_stride, float* y, int32_t B, int32_t Cout, int32_t N,
                           int32_t H, int32_t W, int32_t apply_silu, tmdiff_stream_t stream);
int tmdiff_stem_fwd_pack_bf16(const float* xin, const float* pan, const float* ms, const float* w, const float* bias,
                              const float* out_scale, int32_t out_scale_stride, void* units, int32_t B, int32_t Cout, int32_t N,
                              int32_t H, int32_t W, int32_t apply_silu, tmdiff_stream_t stream);
int tmdiff_head_fwd(const float* x, const float* w, const float* scale, int32_t scale_stride, float* y, int32_t B,
                    int32_t C, int64_t P, tmdiff_stream_t stream); /* scale_stride as in_scale_stride above */
/* stem backward: with u = w[co]*x + bias[co], y = SiLU(u): dwb[b, co, 0] = sum_p gy*SiLU'(u)*x and
 * dwb[b, co, 1] = sum_p gy*SiLU'(u) (per-sample partials [B, Cout, 2]; the caller sums over b).
 * head backward: dx[b,c,p] = gy[b,p]*w[c]*scale[b,c]*SiLU'(x); dws[b,c] = sum_p gy[b,p]*SiLU(x[b,c,p])
 * (dL/d(w[c]*scale[b,c])); scale rows dense [B,C] or NULL (= 1).
 * B == 0 is a no-op for every stem / head / linear entry point, forward and backward: nothing is read or written and the
 * per-sample pointers may be NULL (an empty tensor has no storage).  The sums over no samples are the caller's to zero
 * (dw / db of tmdiff_linear_bwd; dwb and dws have no rows). */
int tmdiff_stem_bwd(const float* xin, const float* pan, const float* ms, const float* w, const float* bias,
                    const float* gy, float* dwb, int32_t B, int32_t Cout, int32_t N, int32_t H, int32_t W,
                    tmdiff_stream_t stream);
/* stem backward w.r.t. its inputs (WavBEST.forward is differentiable in x_t / PAN / MS in the reference, :605-609):
 * xin form: dx[B,N,H,W] = sum_co gy*SiLU'(u)*w;  (pan, ms) form: dx = d_ms = -that, dpan[B,H,W] = sum over the N bands.
 * Either output may be NULL. */
int tmdiff_stem_bwd_input(const float* xin, const float* pan, const float* ms, const float* w, const float* bias,
                          const float* gy, float* dx, float* dpan, int32_t B, int32_t Cout, int32_t N, int32_t H,
                          int32_t W, tmdiff_stream_t stream);
int tmdiff_head_bwd(const float* x, const float* w, const float* scale, const float* gy, float* dx, float* dws,
                    int32_t B, int32_t C, int64_t P, tmdiff_stream_t stream);

/* ------------------------------------------------------------------------------------
 * 2-D Haar DWT / IDWT on the (H, W) axes of [B*C*N, H, W] planes.
 * Replaces DWT_2D / IDWT_2D (DWT_IDWT/DWT_IDWT_layer.py:256-334, :337-430) and
 * DWTFunction_2D / IDWTFunction_2D (DWT_IDWT/DWT_IDWT_Functions.py:47-69, :89-112).
 *  dwt:  ll = ll_scale * LL(x); lh/hl/hh = hi_scale * {LH,HL,HH}(x) (NULL = band not needed)
 *        (the /2 of WaveletUPorDown :396 is ll_scale = 0.5).
 *  idwt: out_k = IDWT(in_scale * ll_k, lh, hl, hh) for k < n_ll low bands sharing the same
 *        high bands (the two iwt calls with 2*h and 2*x at :383-386 are one launch).  The high
 *        bands may be channel slices of one [B, 3C, N, h, w] tensor (the convH_0 output, :381-384):
 *        hi_planes_per_batch = C*N planes per sample, hi_batch_stride = floats between samples
 *        (0 = dense [planes, h, w] bands; a stride that is no multiple of 4 floats is served by the 4-byte
 *        kernel).  lh/hl/hh may all be NULL = zero high bands (the adjoint of an LL-only dwt).
 * The adjoint of dwt is idwt and vice versa (orthonormal transform), which is how the
 * backward passes are served.
 * ------------------------------------------------------------------------------------ */
/* Producer-side prologue: the DWT's LL band / the IDWT's first reconstruction can be written with the CONSUMER convolution's
 * prologue already applied,  out = act(out + shift[b, c]) * scale[b, c]  (plane = (b * C + c) * n_per_channel + n), so that the
 * consumer (Conv_1 of a wavelet block, Hyper_unet_general.py:400-406) reads a plain tensor: same bits as applying the
 * prologue on the consumer side.  Strides as tmdiff_conv3d_desc::in_shift_stride (0 dense = C, > 0 floats, -1 broadcast row). */
typedef struct tmdiff_plane_prologue {
  const float* shift; /* [B, C] or NULL */
  const float* scale; /* [B, C] or NULL */
  int32_t shift_stride, scale_stride;
  int32_t C, n_per_channel;
  int32_t act; /* 0 identity, 1 SiLU */
} tmdiff_plane_prologue;
int tmdiff_haar_dwt2d_pro(const float* x, float* ll, float* lh, float* hl, float* hh, int64_t planes, int32_t H, int32_t W,
                          float ll_scale, float hi_scale, const tmdiff_plane_prologue* ll_prologue, tmdiff_stream_t stream);
int tmdiff_haar_idwt2d_pro(const float* const ll[2], int32_t n_ll, const float* lh, const float* hl, const float* hh,
                           int64_t hi_planes_per_batch, int64_t hi_batch_stride, float* const out[2], int64_t planes,
                           int32_t h, int32_t w, float in_scale, const tmdiff_plane_prologue* out0_prologue,
                           tmdiff_stream_t stream);
/* bf16-mode producers: the LL band / first reconstruction (x, ll0, ll1: [B, C, N, ., .] fp32; stacked_bands [B, 3C, N, h, w])
 * written as the packed bf16 units [B][C/8][N*h*w] of 8 channels (16 bytes) that tmdiff_conv3d_fwd_bf16 reads with x_bf16 = 1,
 * prologue applied in fp32 and rounded to nearest even exactly as that entry point's own pack pass does.  C % 8 == 0.
 * The kernels move fp32 pairs as 8 bytes: x (dwt) and out1 (idwt) must be 8-byte aligned, the units 16-byte aligned; any other
 * base is TMDIFF_E_INVALID without a launch ("... must be 8-byte aligned" in tmdiff_last_error_string()). */
int tmdiff_haar_dwt2d_pack_bf16(const float* x, void* ll_units, float* lh, float* hl, float* hh, int32_t B, int32_t C,
                                int32_t N, int32_t H, int32_t W, float ll_scale, float hi_scale,
                                const tmdiff_plane_prologue* ll_prologue, tmdiff_stream_t stream);
int tmdiff_haar_idwt2d_pack_bf16(const float* ll0, const float* ll1, const float* stacked_bands, void* out0_units, float* out1,
                                 int32_t B, int32_t C, int32_t N, int32_t h, int32_t w, float in_scale,
                                 const tmdiff_plane_prologue* out0_prologue, tmdiff_stream_t stream);
int tmdiff_haar_dwt2d(const float* x, float* ll, float* lh, float* hl, float* hh, int64_t planes, int32_t H,
                      int32_t W, float ll_scale, float hi_scale, tmdiff_stream_t stream);
int tmdiff_haar_idwt2d(const float* const ll[2], int32_t n_ll, const float* lh, const float* hl, const float* hh,
                       int64_t hi_planes_per_batch, int64_t hi_batch_stride, float* const out[2], int64_t planes,
                       int32_t h, int32_t w, float in_scale, tmdiff_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Small dense layers: y[b,o] = act(sum_i x[b,i]*w[o,i] + bias[o]); nn.Linear (+Swish) of the
 * embedding MLPs and every Dense() modulation projection (Hyper_unet_general.py:100-108,
 * :529-532).  One launch serves a whole bank of projections: w is [O_total, I].
 * gamma_embedding (:80-97): emb[b, :half] = cos(t*f), emb[b, half:2*half] = sin(t*f), zero pad if dim is
 * odd; freqs[half] is the host-computed fp32 table exp(-ln(1e4)*k/half) (a 1-ulp difference in f
 * would be amplified by t ~ 1000, so the table is not recomputed on the device).
 * ------------------------------------------------------------------------------------ */
int tmdiff_linear_fwd(const float* x, const float* w, const float* bias, float* y, int32_t B, int32_t I, int32_t O,
                      int32_t act, tmdiff_stream_t stream);
int tmdiff_gamma_embedding(const float* t, const float* freqs, float* emb, int32_t B, int32_t dim,
                           tmdiff_stream_t stream);
/* backward of y = act(x @ w^T + bias): gu = gy * act'(u) with the pre-activation u recomputed into gu_scratch
 * [B, O] (only needed when act != 0); dx[b,i] = sum_o gu[b,o] w[o,i]; dw[o,i] = sum_b gu[b,o] x[b,i];
 * db[o] = sum_b gu[b,o].  Any of dx / dw / db may be NULL.  B == 0: a no-op (dw / db are NOT zeroed; see above). */
int tmdiff_linear_bwd(const float* x, const float* w, const float* bias, const float* gy, float* gu_scratch,
                      float* dx, float* dw, float* db, int32_t B, int32_t I, int32_t O, int32_t act,
                      tmdiff_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Sampler elementwise updates.
 *  ddpm_step: one reverse step of GeneralDiffusion.p_sample (diffusion_general.py:203-208 with
 *    :376-378, :192-194, :134-138):  x0 = clamp(c_recip*x - c_recipm1*eps, -1, 1);
 *    out = coef1*x0 + coef2*x + sigma*noise   (noise may be NULL when sigma == 0)
 *    and optionally img_out = out + ms (res2img, utils/util.py:135-137).
 *  axpby: out = sum_{k<n} coef[k] * in[k], n <= 4: every DPM-Solver update
 *    (core/dpm_solver_pytorch.py:563-927).
 *  x0_from_model: DPM-Solver++ data prediction for an x_start-parameterised network
 *    (dpm_solver_pytorch.py:302-306 then :447-456): eps = (x - alpha*out)/sigma;
 *    x0 = (x - sigma*eps)/alpha.
 *  abs_quantile_clamp: dynamic thresholding (:430-439): per sample s = max(quantile(|x0|, q), max_val)
 *    (linear interpolation between order statistics, as torch.quantile), x0 = clamp(x0,-s,s)/s.
 *    workspace: tmdiff_abs_quantile_workspace_bytes(B, n) bytes (select state; on return its first B floats hold
 *    the per-sample thresholds s).  Runs as a few launches (histogram passes spread over many workgroups).
 * ------------------------------------------------------------------------------------ */
int tmdiff_ddpm_step(const float* x, const float* eps, const float* noise, const float* ms, float* out,
                     float* img_out, int64_t n, float c_recip, float c_recipm1, float coef1, float coef2,
                     float sigma, int32_t clip, tmdiff_stream_t stream);
int tmdiff_axpby(const float* const in[4], const float coef[4], int32_t n_in, float* out, int64_t n,
                 tmdiff_stream_t stream);
/* ddpm_step_dev: the same step with its scalars in DEVICE memory, so that a recorded launch can be replayed from a HIP
 * graph for every timestep: t = *step; row t of coef [T][5] = (c_recip, c_recipm1, coef1, coef2, sigma), built from the
 * same fp32 values tmdiff_ddpm_step is passed (sigma = 0 at t = 0).  x may equal out (in-place update).  noise is not
 * read where sigma is 0.  If frames != NULL and t % frame_every == 0, out + ms is also written to slot
 * tmdiff_ddpm_frame_slot(t, T, frame_every) of frames (slots of n floats: p_sample_loop's frame stack, slot 0 being
 * x_T + ms).  A t outside [0, T) writes nothing.
 * sampler_tick: *step = set_to if set_to >= 0, else *step - 1; then time_in[b] = *step + 1 (fp32) for b < B.  One
 * workgroup; stream-ordered after the step it follows. */
int tmdiff_ddpm_step_dev(const float* x, const float* eps, const float* noise, const float* ms, float* out, float* frames,
                         int64_t n, const int32_t* step, const float* coef, int32_t T, int32_t frame_every, int32_t clip,
                         tmdiff_stream_t stream);
int tmdiff_sampler_tick(int32_t* step, float* time_in, int32_t B, int32_t set_to, tmdiff_stream_t stream);
/* slot index of step t in p_sample_loop's frame stack (host function; -1 for arguments out of range) */
int tmdiff_ddpm_frame_slot(int32_t t, int32_t T, int32_t frame_every);
/* Multi-tensor form, ONE launch for a whole parameter list: out_t = ca * a_t + cb * b_t for every entry (the EMA update of
 * utils/EmaUpdater.py:23-38: out = a = EMA weights, b = live weights).  `tensors_dev` is a DEVICE array of entries;
 * the launch has one workgroup per chunk of tmdiff_multi_axpby_chunk() elements: chunk k works on elements
 * [chunk_index_dev[k] * chunk, ...) of tensor chunk_tensor_dev[k] (both DEVICE int32 arrays of n_chunks entries). */
typedef struct tmdiff_mt_entry {
  float* out;
  const float* a;
  const float* b;
  int64_t n;
} tmdiff_mt_entry;
int32_t tmdiff_multi_axpby_chunk(void);
int tmdiff_multi_axpby(const tmdiff_mt_entry* tensors_dev, const int32_t* chunk_tensor_dev, const int32_t* chunk_index_dev,
                       int32_t n_chunks, float ca, float cb, tmdiff_stream_t stream);
/* AdamW step (torch.optim.AdamW semantics, amsgrad off; reference GeneralModel/model.py:30-31, :43) of a whole list of parameter
 * tensors in ONE launch, chunked like tmdiff_multi_axpby (same chunk size, same two device tables).  lr_dev / step_dev are DEVICE
 * scalars (the learning rate; the step count t of THIS update, already incremented, as a float), so a recorded launch can be
 * replayed from a HIP graph.  In place: p, m (exp_avg), v (exp_avg_sq). */
typedef struct tmdiff_adamw_entry {
  float* p;
  const float* g;
  float* m;
  float* v;
  int64_t n;
} tmdiff_adamw_entry;
int tmdiff_multi_adamw(const tmdiff_adamw_entry* tensors_dev, const int32_t* chunk_tensor_dev, const int32_t* chunk_index_dev,
                       int32_t n_chunks, const float* lr_dev, const float* step_dev, float beta1, float beta2, float eps,
                       float weight_decay, tmdiff_stream_t stream);
/* Global-norm gradient clipping inside that step (torch.nn.utils.clip_grad_norm_, norm_type 2), with no host read and no write
 * to the gradients.  All three take the tables of tmdiff_multi_adamw and want n_chunks > 0.
 *  multi_sqnorm_partial: partials_dev[k] = sum of g^2 over chunk k, accumulated in double; one workgroup per chunk, no atomics.
 *    partials_dev holds tmdiff_multi_sqnorm_workspace_bytes(n_chunks) bytes.  Several parameter groups write at their own
 *    offsets of one buffer.
 *  multi_sqnorm_finish (one workgroup, fixed summation order: the same bits on every run and in a graph replay):
 *    *norm_dev = (float)sqrt(sum of the n_partials partials), *ok_dev = 1 if that is finite, else 0,
 *    *coef_dev = min(1, max_norm / (*norm_dev + 1e-6f)) in fp32, or 0 where *ok_dev is 0.  max_norm > 0.
 *  multi_adamw_scaled: tmdiff_multi_adamw on g * *coef_dev (rounded once, kept in registers: g is only read).  With
 *    *ok_dev == 0 the launch touches nothing: p, m and v keep their bits. */
size_t tmdiff_multi_sqnorm_workspace_bytes(int32_t n_chunks);
int tmdiff_multi_sqnorm_partial(const tmdiff_adamw_entry* tensors_dev, const int32_t* chunk_tensor_dev,
                                const int32_t* chunk_index_dev, int32_t n_chunks, double* partials_dev, tmdiff_stream_t stream);
int tmdiff_multi_sqnorm_finish(const double* partials_dev, int32_t n_partials, float max_norm, float* norm_dev, float* coef_dev,
                               float* ok_dev, tmdiff_stream_t stream);
int tmdiff_multi_adamw_scaled(const tmdiff_adamw_entry* tensors_dev, const int32_t* chunk_tensor_dev,
                              const int32_t* chunk_index_dev, int32_t n_chunks, const float* lr_dev, const float* step_dev,
                              float beta1, float beta2, float eps, float weight_decay, const float* coef_dev, const float* ok_dev,
                              tmdiff_stream_t stream);
int tmdiff_x0_from_model(const float* x, const float* model_out, float* x0, int64_t n, float alpha, float sigma,
                         int32_t model_is_x_start, tmdiff_stream_t stream);
size_t tmdiff_abs_quantile_workspace_bytes(int32_t B, int64_t n_per_sample);
int tmdiff_abs_quantile_clamp(float* x0, int32_t B, int64_t n_per_sample, float q, float max_val, void* workspace,
                              tmdiff_stream_t stream);
/* out = a + b (res2img / img2res with sign), q_sample: out = a[b]*x0 + sqrt(1-a[b]^2)*noise. */
int tmdiff_add(const float* a, const float* b, float* out, int64_t n, float sign_b, tmdiff_stream_t stream);
int tmdiff_q_sample(const float* x0, const float* noise, const float* a, float* out, int32_t B, int64_t n_per_sample,
                    tmdiff_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Overlapped scene tiles (fused large-scene sampling; the reference only tiles without overlap, data/LRHR_dataset.py:17-53).
 * One noisy scene [B, C, H, W] is kept; at every denoise step square tiles of edge `tile` that overlap by `overlap` pixels
 * are cut out of it, the network runs on the tiles, and its outputs are blended back into one scene-sized prediction.
 *  plan (per axis of length L): origins 0, s, 2s, ... with s = tile - overlap while origin + tile <= L, plus one tile pushed
 *    inwards to L - tile when the last regular one does not end at L: origin(i) = min(i * s, L - tile).  Needs tile <= L and
 *    0 <= overlap <= tile / 2.  tmdiff_tile_plan (host function) returns the number of origins and writes the first
 *    `capacity` of them (origins may be NULL); -1 for arguments out of range.  (tile % 8 == 0, which the UNet's three
 *    wavelet levels need, is the caller's rule -- tiling.plan_tiles -- and not checked here: the kernels only copy.)
 *  tiles are [B * ny * nx, C, tile, tile], numbered row-major per scene sample.
 *  tile_gather: tiles[(b, iy, ix), c, y, x] = scene[b, c, oy(iy) + y, ox(ix) + x]  (a copy).
 *  tile_blend : scene[b, c, Y, X] = sum_t w_t v_t / sum_t w_t over the tiles t that cover (Y, X), in row-major tile order, with
 *    w_t = w1(Y - oy) * w1(X - ox), w1(i) = min(i + 1, tile - i, overlap + 1); fp32, no atomics: deterministic.
 * Both use 16-byte accesses when W, tile and tile - overlap are multiples of 4 and the tensors are 16-byte aligned, scalar ones
 * otherwise.  Element offsets are 32-bit: tmdiff_tile_supported is 0 (and the entry points return TMDIFF_E_UNSUPPORTED
 * without launching) when the scene or the tile stack holds more than 2^31 - 1 elements.
 * ------------------------------------------------------------------------------------ */
int32_t tmdiff_tile_plan(int32_t L, int32_t tile, int32_t overlap, int32_t* origins, int32_t capacity);
int tmdiff_tile_supported(int32_t B, int32_t C, int32_t H, int32_t W, int32_t tile, int32_t overlap);
int tmdiff_tile_gather(const float* scene, float* tiles, int32_t B, int32_t C, int32_t H, int32_t W, int32_t tile,
                       int32_t overlap, tmdiff_stream_t stream);
int tmdiff_tile_blend(const float* tiles, float* scene, int32_t B, int32_t C, int32_t H, int32_t W, int32_t tile,
                      int32_t overlap, tmdiff_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Pansharpening quality metrics on the device (csrc/metrics.hip; definitions: tmdiff_amd/metrics.py, reference core/metrics.py).
 * Inputs are fp32 [B, C, H, W] with dense rows and planes; the batch and channel strides (in elements) are arguments, so a
 * channel or batch slice of a larger tensor is scored in place.  Outputs are fp64 [B, K] on the device, one row per image.
 *  metrics_pair : x_pred against x_true.  K = 9 columns: psnr, sam (degrees), ssim (7 x 7 uniform window, K1 = 0.01, K2 = 0.03,
 *    sample covariance, 'valid' region), ergas (per-band MSE over the squared mean of x_pred), rmse (bands summed, divided by
 *    H * W), cc, scc (Pearson correlation of the 'valid' 3 x 3 Laplacians), q (universal quality index, ddof = 1), q4 (NaN unless
 *    C == 4); psnr, ssim, cc, scc and q are means over the bands.  The spectral angle is formed per pixel in fp64 as
 *    acos(dot / |pred| / |true|), a non-finite angle counting as 0; every other non-finite value is left as IEEE gives it.
 *    A band that is constant in an image (least value == greatest value) has variance and covariance exactly 0 there, so
 *    cc and scc are NaN for it (and q, when it is constant in both images), as a two-pass evaluation gives.
 *  metrics_noref: d_lambda, d_s, qnr = (1 - d_lambda)(1 - d_s) of ps [B, C, H, W] and pan [B, 1, H, W] against l_ms
 *    [B, C, h, w] and l_pan [B, 1, h, w]; the quality index with population moments and 1e-8 added to its denominator.
 * All sums are fp64 and no atomics are used: the workgroups store partial sums into `workspace` and one finalize launch adds
 * them in a fixed order (16 runs of consecutive tiles, then the runs), so a call is reproducible bit for bit.  Nothing is allocated, synchronised or copied to the host: a call
 * can be captured into a graph on `stream`.  workspace: 8-byte aligned, tmdiff_metrics_workspace_bytes(B, C, H, W) bytes (H, W:
 * the full-resolution extents), enough for either entry point.
 * Extents: 1 <= C <= 16, H >= 7, W >= 7, B * C * H * W <= 2^31 - 1 (32-bit element offsets inside a plane); for anything else
 * tmdiff_metrics_supported is 0, the workspace size is 0 and the entry points return TMDIFF_E_UNSUPPORTED without launching.
 * ------------------------------------------------------------------------------------ */
int tmdiff_metrics_supported(int32_t B, int32_t C, int32_t H, int32_t W);
size_t tmdiff_metrics_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W);
int tmdiff_metrics_pair(const float* x_true, int64_t true_stride_b, int64_t true_stride_c, const float* x_pred,
                        int64_t pred_stride_b, int64_t pred_stride_c, int32_t B, int32_t C, int32_t H, int32_t W,
                        double data_range, double ratio, double* out, void* workspace, size_t workspace_bytes,
                        tmdiff_stream_t stream);
int tmdiff_metrics_noref(const float* l_ms, int64_t l_ms_stride_b, int64_t l_ms_stride_c, const float* pan,
                         int64_t pan_stride_b, const float* l_pan, int64_t l_pan_stride_b, const float* ps,
                         int64_t ps_stride_b, int64_t ps_stride_c, int32_t B, int32_t C, int32_t H, int32_t W, int32_t h,
                         int32_t w, double* out, void* workspace, size_t workspace_bytes, tmdiff_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Q2n on the device (csrc/metrics.hip; definition: tmdiff_amd/metrics.py q2n): the hypercomplex quality index of Garzelli and
 * Nencini (2009) -- Q4 for four bands, Q8 for eight -- of x_pred against x_true on windows of block x block pixels every `shift`
 * pixels, averaged per image.  ny = ceil(H / shift), nx = ceil(W / shift) windows; the images are mirrored at the bottom and
 * the right (edge sample included) up to (ny - 1) * shift + block, and zero bands are appended up to the next power of two.
 * Tensors, strides, sums, reproducibility and graph capture as for tmdiff_metrics_pair.  out: fp64 [B]; map_out: fp64
 * [B, ny, nx] of the windows' values, or NULL; workspace: 8-byte aligned, tmdiff_metrics_q2n_workspace_bytes(...) bytes.
 * Extents: 1 <= C <= 16, block 8, 16 or 32, 1 <= shift <= block, mirrored rows / columns no more than H / W,
 * B * C * H * W <= 2^31 - 1; for anything else tmdiff_metrics_q2n_supported is 0, the workspace size is 0 and the entry point
 * returns TMDIFF_E_UNSUPPORTED without launching.
 * ------------------------------------------------------------------------------------ */
int tmdiff_metrics_q2n_supported(int32_t B, int32_t C, int32_t H, int32_t W, int32_t block, int32_t shift);
size_t tmdiff_metrics_q2n_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W, int32_t block, int32_t shift);
int tmdiff_metrics_q2n(const float* x_true, int64_t true_stride_b, int64_t true_stride_c, const float* x_pred,
                       int64_t pred_stride_b, int64_t pred_stride_c, int32_t B, int32_t C, int32_t H, int32_t W, int32_t block,
                       int32_t shift, double* out, double* map_out, void* workspace, size_t workspace_bytes,
                       tmdiff_stream_t stream);

/* ------------------------------------------------------------------------------------
 * The spatial term of HQNR on the device (csrc/metrics.hip; definition: tmdiff_amd/metrics.py d_s_block): per band c and per
 * non-overlapping block x block window (the grid and the mirroring of tmdiff_metrics_q2n at shift = block) the universal
 * quality index with sample moments, Q_high = Q(ps_c, pan) and Q_low = Q(ms_exp_c, pan_lp); both are averaged over the
 * windows and D_s = (mean_c |Q_high_c - Q_low_c|^q)^(1/q).  A window that is constant in both images, or whose means are both
 * zero, is NaN (0 / 0) and the NaN reaches D_s: no eps is added.
 * ps, ms_exp: fp32 [B, C, H, W] with batch and channel strides in elements; pan, pan_lp: fp32 [B, 1, H, W] with a batch
 * stride; rows and planes dense.  out: fp64 [B, 2] = D_s, HQNR.  With d_lambda, fp64 [B] on the device, HQNR =
 * (1 - d_lambda)^alpha (1 - D_s)^beta is written; with NULL the second column is left untouched.  maps_out: fp64
 * [B, C, 2, ny, nx] of the windows' Q_high and Q_low, or NULL.  workspace: 8-byte aligned,
 * tmdiff_metrics_dsblock_workspace_bytes(...) bytes.  Sums, reproducibility and graph capture as for tmdiff_metrics_pair.
 * Extents: 1 <= C <= 16, block 8, 16 or 32, mirrored rows / columns no more than H / W, B * C * H * W <= 2^31 - 1, q > 0; for
 * anything else tmdiff_metrics_dsblock_supported is 0, the workspace size is 0 and the entry point returns
 * TMDIFF_E_UNSUPPORTED without launching.
 * ------------------------------------------------------------------------------------ */
int tmdiff_metrics_dsblock_supported(int32_t B, int32_t C, int32_t H, int32_t W, int32_t block);
size_t tmdiff_metrics_dsblock_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W, int32_t block);
int tmdiff_metrics_dsblock(const float* ps, int64_t ps_stride_b, int64_t ps_stride_c, const float* ms_exp, int64_t ms_stride_b,
                           int64_t ms_stride_c, const float* pan, int64_t pan_stride_b, const float* pan_lp,
                           int64_t pan_lp_stride_b, int32_t B, int32_t C, int32_t H, int32_t W, int32_t block, double q,
                           const double* d_lambda, double alpha, double beta, double* out, double* maps_out, void* workspace,
                           size_t workspace_bytes, tmdiff_stream_t stream);

/* ------------------------------------------------------------------------------------
 * The composite finetune loss with its gradient, one pass (csrc/loss.hip; host definition: tmdiff_amd/losses.py):
 *     L = base(xhat, x0) + w_sam * SAM(x0 + ms, xhat + ms) + w_lap * LAP(xhat - x0)
 * on dense fp32 [B, C, H, W] tensors.
 *  base : the mean over B C H W of rho(xhat - x0); base_kind 0 = l1 (|d|), 1 = l2 (d^2), 2 = smooth l1 with beta = 1.
 *  SAM  : the mean over the B H W pixels of the angle in radians between the band vectors u = x0 + ms and v = xhat + ms,
 *    formed as atan2(|cross|, dot) with |cross|^2 = |u|^2 |v|^2 - dot^2.  Its gradient with respect to v is
 *    -(u - (dot / |v|^2) v) / |cross|, a vector of norm 1 / |v|.  A pixel with |u| = 0, |v| = 0 or |cross|^2 <= 0 (u parallel
 *    to v; every pixel when C == 1) contributes its angle (0; pi for antiparallel vectors) and an exactly zero gradient.
 *  LAP  : the mean over the B C (H - 2)(W - 2) interior ('valid') pixels of |Lap d|, d = xhat - x0, Lap the 3 x 3 kernel with
 *    -8 at the centre and 1 on the eight neighbours; its gradient is Lap^T applied to sign(Lap d), sign(0) = 0, taken as 0
 *    outside the interior.
 * g (fp32 [B, C, H, W]) receives dL/dxhat, already weighted by w_sam and w_lap and divided by the counts; g == NULL selects
 * the value-only mode, which writes no gradient.  out64: fp64 [4] = total, base, sam, lap (the unweighted means of the terms,
 * the weighted total; a term whose weight is 0 is not evaluated and reports 0); out32: the total as one float.  ms may be
 * NULL only when w_sam == 0.  Weights must be finite and not negative (else TMDIFF_E_INVALID, as for another base_kind).
 * Every operation after the fp32 loads is fp64 and the gradient is rounded once, at its store (a magnitude past the fp32
 * range saturates at FLT_MAX: nothing non-finite is stored for finite inputs).  No atomics: each workgroup (one per 16 x 32
 * tile of one image) stores three fp64 partial sums into `workspace` and one finalize launch adds them in a fixed order, so a
 * call is reproducible bit for bit.  Nothing is allocated, synchronised or copied: a call can be captured into a graph on
 * `stream`.  16-byte accesses when W % 4 == 0 and the tensors are 16-byte aligned, scalar ones otherwise, with the same values.
 * workspace: 8-byte aligned, tmdiff_loss_workspace_bytes(B, C, H, W, lap) = 24 * B * ceil(H / 16) * ceil(W / 32) bytes.
 * Extents (`lap`: w_lap != 0): B >= 1, 1 <= C <= 16, H, W >= 3 with lap and >= 1 without, B * C * H * W <= 2^31 - 1; for
 * anything else tmdiff_loss_supported is 0, the workspace size is 0 and the entry point returns TMDIFF_E_UNSUPPORTED without
 * launching.  (Added within version 6.)
 * ------------------------------------------------------------------------------------ */
int tmdiff_loss_supported(int32_t B, int32_t C, int32_t H, int32_t W, int32_t lap);
size_t tmdiff_loss_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W, int32_t lap);
int tmdiff_spectral_spatial_loss(const float* x0, const float* xhat, const float* ms, float* g, int32_t base_kind,
                                 double w_sam, double w_lap, double* out64, float* out32, void* workspace,
                                 size_t workspace_bytes, int32_t B, int32_t C, int32_t H, int32_t W,
                                 tmdiff_stream_t stream);

/* ------------------------------------------------------------------------------------
 * The SSIM loss term with its gradient (csrc/ssim_loss.hip; host definition: tmdiff_amd/losses.py ssim_loss_host):
 *     dssim = 1 - SSIM(x_true, x_pred),  x_true = x_true_in (+ ms),  x_pred = x_pred_in (+ ms)
 * on dense fp32 [B, C, H, W] tensors; ms (optional, may be NULL) is added to both after the loads, in fp64.
 *  SSIM : the mean over all B C (H - win + 1)(W - win + 1) windows of S = (A1 A2) / (B1 B2), a uniform win x win window per
 *    band plane over the 'valid' region, n = win^2, k = n / (n - 1), f the window mean, a = x_true, b = x_pred:
 *    ux = f(a), uy = f(b), vx = k (f(a a) - ux^2), vy = k (f(b b) - uy^2), vxy = k (f(a b) - ux uy), A1 = 2 ux uy + c1,
 *    A2 = 2 vxy + c2, B1 = ux^2 + uy^2 + c1, B2 = vx + vy + c2, c1 = (0.01 data_range)^2, c2 = (0.03 data_range)^2: what
 *    tmdiff_metrics_pair scores.  f(a b), f(a a) and f(b b) are formed by one instruction sequence: x_pred == x_true gives
 *    S == 1 and dssim == 0 exactly.
 *  g (fp32 [B, C, H, W]): accumulate == 0 stores weight * d dssim / d x_pred, rounded to fp32 once; accumulate == 1 stores
 *    fl32(g + weight * d dssim / d x_pred) (the term rides on a gradient another kernel has just written); g == NULL selects
 *    the value-only mode, which writes no gradient (accumulate must then be 0, else TMDIFF_E_INVALID).
 *  terms_in == NULL: out64 is fp64 [2] = dssim, ssim and out32 the float of weight * dssim.
 *  terms_in given (fp64 [4], the out64 of tmdiff_spectral_spatial_loss): out64 is fp64 [5] = terms_in[0] + weight * dssim,
 *    terms_in[1], terms_in[2], terms_in[3], dssim and out32 the float of entry 0.  out64 may be terms_in's own storage.
 * Every operation after the fp32 loads is fp64.  No atomics: each workgroup (one per 16 x 32 tile of one band plane) stores one
 * fp64 partial sum into `workspace` and one finalize launch adds them in a fixed order, so a call is reproducible bit for bit.
 * Nothing is allocated, synchronised or copied: a call can be captured into a graph on `stream`.  16-byte accesses when
 * W % 4 == 0 and the tensors are 16-byte aligned, scalar ones otherwise, with the same values.
 * workspace: 8-byte aligned, tmdiff_ssim_loss_workspace_bytes(B, C, H, W, win) = 8 * B * C * ceil(H / 16) * ceil(W / 32) bytes.
 * Limits: B, C >= 1, win odd with 3 <= win <= 11, H, W >= win, B * C * H * W <= 2^31 - 1; for anything else
 * tmdiff_ssim_loss_supported is 0 and the workspace size is 0.  The entry point returns TMDIFF_E_UNSUPPORTED without launching
 * for those, and for a data_range that is not finite and > 0 or a weight that is not finite and >= 0.  (Added within version 6.)
 * ------------------------------------------------------------------------------------ */
int tmdiff_ssim_loss_supported(int32_t B, int32_t C, int32_t H, int32_t W, int32_t win);
size_t tmdiff_ssim_loss_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W, int32_t win);
int tmdiff_ssim_loss(const float* x_true, const float* x_pred, const float* ms, float* g, int32_t win, double data_range,
                     double weight, int32_t accumulate, const double* terms_in, double* out64, float* out32, void* workspace,
                     size_t workspace_bytes, int32_t B, int32_t C, int32_t H, int32_t W, tmdiff_stream_t stream);

/* ------------------------------------------------------------------------------------
 * The local PAN-correlation loss with its gradient (csrc/local_corr.hip; host definition: tmdiff_amd/metrics.py
 * local_corr_loss):
 *     loss = mean over b, c and windows of max(0, rho_max[c] - rho),   D_rho = 1 - mean rho
 * on dense fp32 x [B, C, H, W] and pan [B, 1, H, W].
 *  rho : the correlation coefficient of a band and the PAN inside a win x win window, every window at stride 1, 'valid',
 *    n = win^2, from two-pass centred sums: mx = sum(x) / n, mp = sum(p) / n, then S_xx = sum (x - mx)^2, S_pp = sum (p - mp)^2,
 *    S_xp = sum (x - mx)(p - mp); rho = S_xp / sqrt(S_xx S_pp), and 0 where S_xx S_pp == 0 exactly (no eps: a window that is
 *    constant in either image gives exactly 0 and no gradient).  A window is active iff rho < rho_max[c].
 *  rho_max : fp64 [C] on the device, or NULL for 1.0 in every band.
 *  g (fp32 [B, C, H, W]): accumulate == 0 stores weight * d loss / d x, rounded to fp32 once; accumulate == 1 stores
 *    fl32(g + weight * d loss / d x); g == NULL selects the value-only mode, which writes no gradient (accumulate must then be
 *    0, else TMDIFF_E_INVALID).  pan gets no gradient.
 *  out64 : fp64 [2] = loss, mean rho.  per_image (fp64 [B], may be NULL): the mean rho of each image.  out32 : the float of
 *    weight * loss.
 * Every operation after the fp32 loads is fp64.  No atomics: each workgroup (one per image and 16 x 32 tile, walking the bands
 * with the PAN tile staged once) stores two fp64 partial sums into `workspace` and one finalize launch adds them in a fixed
 * order, image by image, so a call is reproducible bit for bit and an image's mean does not depend on the batch it is in.
 * Nothing is allocated, synchronised or copied: a call can be captured into a graph on `stream`.  16-byte accesses when
 * W % 4 == 0 and the tensors are 16-byte aligned, scalar ones otherwise, with the same values.
 * workspace: 8-byte aligned, tmdiff_local_corr_loss_workspace_bytes(B, C, H, W, win) = 16 * B * ceil(H / 16) * ceil(W / 32) bytes.
 * Limits: B >= 1, 1 <= C <= 16, 2 <= win <= 8 (even and odd), H, W >= win, B * C * H * W <= 2^31 - 1; for anything else
 * tmdiff_local_corr_loss_supported is 0 and the workspace size is 0.  The entry point returns TMDIFF_E_UNSUPPORTED without
 * launching for those, and for a weight that is not finite and >= 0.  (Added within version 6.)
 * ------------------------------------------------------------------------------------ */
int tmdiff_local_corr_loss_supported(int32_t B, int32_t C, int32_t H, int32_t W, int32_t win);
size_t tmdiff_local_corr_loss_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W, int32_t win);
int tmdiff_local_corr_loss(const float* x, const float* pan, float* g, const double* rho_max, int32_t win, double weight,
                           int32_t accumulate, double* out64, double* per_image, float* out32, void* workspace,
                           size_t workspace_bytes, int32_t B, int32_t C, int32_t H, int32_t W, tmdiff_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Resampling of full-resolution scenes (csrc/resample.hip; host definitions: tmdiff_amd/metrics.py).  Dense fp32 planes
 * [planes, H, W]; nothing is allocated or synchronised, so a call can be captured into a graph on `stream`.
 *  pyr_down: `levels` (1 or 2) steps of OpenCV's pyrDown with its defaults -- separable [1 4 6 4 1] / 16, horizontal pass then
 *    vertical pass, border reflect-101, output extent (L + 1) / 2 per axis and level, sampled at the even coordinates.  Each
 *    5-tap sum is (a + e) / 16 + (b + d) / 4 + c * 3 / 8 with fixed roundings; two levels run as one kernel that keeps level 1
 *    in LDS, and equal two one-level calls bit for bit.  y is [planes, H', W'] with L' = (L + 1) / 2 applied `levels` times.
 *    Every level's input extent must be >= 3: H, W >= 3 for one level, >= 5 for two.
 *  upsample_bilinear: y [planes, ratio * h, ratio * w], ratio 2 or 4, half-pixel centres with the edge clamped:
 *    src = (dst + 0.5) / ratio - 0.5 in [0, L - 1] (cv2.resize(INTER_LINEAR); F.interpolate(mode="bilinear",
 *    align_corners=False)).  16-byte stores when ratio * w is a multiple of 4 and y is 16-byte aligned, with the same values.
 *  upsample_poly23: y [planes, ratio * h, ratio * w], ratio 2 or 4: the Pansharpening Toolbox's interp23tap (the `lms` of the
 *    PanCollection files).  Per x2 stage and axis, H then W, with circular borders: the samples go to the outputs of parity
 *    `phase` (u[2k + phase] = x[k], a plain copy) and the outputs between become sum_j a_j (x[lo - j] + x[lo + 1 + j]), j = 0..5,
 *    over the six samples either side, a = {0.61066818237, -0.145397186478, 0.043619155884, -0.010385513306, 0.001615524292,
 *    -0.000120162964} (twice the odd taps of the 23-tap half-band kernel): pair sums first, then fused multiply-adds from j = 5
 *    down to 0.  ratio 4 is a phase-1 stage followed by a phase-0 stage in one kernel that keeps the x2 image in LDS, and equals
 *    the two calls bit for bit: y[4i + 2, 4j + 2] = x[i, j].  `phase` (0 or 1) selects the stage at ratio 2 and must be 1 at
 *    ratio 4.  16-byte stores when ratio * w is a multiple of 4 and y is 16-byte aligned, with the same values.
 * Element offsets are 32-bit: more than 2^31 - 1 input (pyr_down) or output (upsample_*) elements, other `levels` / `ratio` /
 * `phase` or smaller extents return TMDIFF_E_UNSUPPORTED without launching (upsample_poly23: negative `planes` too).
 * ------------------------------------------------------------------------------------ */
int tmdiff_pyr_down(const float* x, float* y, int32_t planes, int32_t H, int32_t W, int32_t levels, tmdiff_stream_t stream);
int tmdiff_upsample_bilinear(const float* x, float* y, int32_t planes, int32_t h, int32_t w, int32_t ratio,
                             tmdiff_stream_t stream);
int tmdiff_upsample_poly23(const float* x, float* y, int32_t planes, int32_t h, int32_t w, int32_t ratio, int32_t phase,
                           tmdiff_stream_t stream);

/* ------------------------------------------------------------------------------------
 * FIR filtering with decimation (csrc/mtf.hip; host definition: tmdiff_amd/metrics.py, fir_decimate): the primitive of Wald's
 * protocol, an MTF-matched low-pass per band followed by keeping every ratio-th sample.  Dense fp32 planes; nothing is
 * allocated or synchronised, so a call can be captured into a graph on `stream`.
 *   y[p, i, j] = sum_{u, v} taps[p % taps_period, u, v] * x[p, clamp(ratio i + off_y - R + u, 0, H - 1),
 *                                                             clamp(ratio j + off_x - R + v, 0, W - 1)],   R = (K - 1) / 2
 * a correlation (the taps are not flipped) with a replicated border; x [planes, H, W], taps [taps_period, K, K],
 * y [planes, ceil((H - off_y) / ratio), ceil((W - off_x) / ratio)].  Only the kept samples are computed.  A pixel is one chain
 * of fused multiply-adds from 0 over the taps in row-major order, whatever the tile, grid, plane or ratio that makes it.
 * Checked in this order, each returning TMDIFF_E_UNSUPPORTED without launching: K odd and 1 <= K <= 41; ratio 1, 2 or 4;
 * 0 <= off_y, off_x < ratio; H, W >= 1 and planes >= 0; taps_period >= 1 and a divisor of planes; planes * H * W <= 2^31 - 1
 * (element offsets are 32-bit).  planes == 0, or an output without samples (H <= off_y or W <= off_x), returns TMDIFF_OK; a
 * null tensor TMDIFF_E_INVALID.
 * ------------------------------------------------------------------------------------ */
int tmdiff_fir_decimate(const float* x, const float* taps, float* y, int32_t planes, int32_t taps_period, int32_t H, int32_t W,
                        int32_t K, int32_t ratio, int32_t off_y, int32_t off_x, tmdiff_stream_t stream);

/* ------------------------------------------------------------------------------------
 * The adjoint of fir_decimate (csrc/mtf.hip; host definition: tmdiff_amd/metrics.py, fir_decimate_adjoint):
 *   dx = beta * base + alpha * A^T g,   g [planes, ceil((H - off_y) / ratio), ceil((W - off_x) / ratio)],   dx, base [planes, H, W]
 *   (A^T g)[p, y, x] = sum over (i, u, j, v) with clamp(ratio i + off_y - R + u, 0, H - 1) == y and
 *                      clamp(ratio j + off_x - R + v, 0, W - 1) == x   of   taps[p % taps_period, u, v] * g[p, i, j]
 * the exact transpose, the replicated border included: a border pixel collects every position that was clamped onto it.  A
 * gather without atomics; a pixel is one chain of fused multiply-adds from 0 over its terms in lexicographic order of
 * (i, u, j, v), whatever the tile, grid or plane that makes it, then r = alpha * acc and, when beta != 0, fma(beta, base, r).
 * `base` may be NULL when beta == 0 (it is not read then) and may be `dx` itself.  Nothing is allocated or synchronised.
 * The limits are fir_decimate's, checked in the same order.  planes == 0 returns TMDIFF_OK; an operator without samples
 * (H <= off_y or W <= off_x) has A^T g = 0 and `g` may be NULL; any other null tensor is TMDIFF_E_INVALID.
 * ------------------------------------------------------------------------------------ */
int tmdiff_fir_decimate_adjoint(const float* g, const float* taps, const float* base, float* dx, float alpha, float beta,
                                int32_t planes, int32_t taps_period, int32_t H, int32_t W, int32_t K, int32_t ratio, int32_t off_y,
                                int32_t off_x, tmdiff_stream_t stream);

/* ------------------------------------------------------------------------------------
 * MTF-GLP pansharpening (host definitions: tmdiff_amd/metrics.py, pan_lowpass_bands / glp_moments / mtf_glp).  Dense fp32
 * tensors; nothing is allocated or synchronised, no atomics, the same bits on every run and on a graph replay.
 *  fir_decimate_bank (csrc/mtf.hip): a filter bank on ONE plane per image, y[b, t] = fir_decimate(x[b], taps[t]); x [images, H, W],
 *             taps [tables, K, K], y [images, tables, H', W'].  The kernel of fir_decimate: a workgroup stages the clamped patch
 *             once and walks the tables over it; a pixel has fir_decimate's summation order, so y equals fir_decimate on the
 *             tables-fold copy of x bit for bit.  Limits: images >= 0, tables >= 1, then fir_decimate's on images * tables
 *             planes, in its order.  images == 0 or an output without samples returns TMDIFF_OK.
 *  glp_moments (csrc/metrics.hip): ms_exp, pan_lp [B, C, H, W], pan [B, H, W] -> out, float64 [B, C, 7]: the population
 *             moments mean(M_c), mean(L_c), mean(P), var(M_c), var(L_c), cov(M_c, L_c), var(P).  One pass; every value has its
 *             plane's first pixel subtracted in fp64 after the load (a pilot), sums and products are fp64; partial sums per
 *             workgroup in `workspace` (8-byte aligned, tmdiff_glp_moments_workspace_bytes), a finalize launch adds them in
 *             index order.  The workspace then starts with the finished sums, float64 [B, C, 7]: S_dm, S_dl, S_dp, S_dm.dm,
 *             S_dl.dl, S_dm.dl, S_dp.dp with d = value - pilot.  Limits: B >= 0, 1 <= C <= 16, H, W >= 1, B * C * H * W <=
 *             2^31 - 1; otherwise TMDIFF_E_UNSUPPORTED and a workspace size of 0.
 *  glp_inject (csrc/fusion.hip): out [B, C, H, W] from ms_exp, pan, pan_lp and the device-resident `moments` of glp_moments;
 *             mode 0 "glp", 1 "cbd", 2 "hpm".  The band's gains are formed on the device, the formula is evaluated in fp64 and
 *             rounded to fp32 once.  out may be ms_exp; it must not overlap pan, pan_lp or moments.  Limits: glp_moments'.
 *             (Added within version 6.)
 * ------------------------------------------------------------------------------------ */
int tmdiff_fir_decimate_bank(const float* x, const float* taps, float* y, int32_t images, int32_t tables, int32_t H, int32_t W,
                             int32_t K, int32_t ratio, int32_t off_y, int32_t off_x, tmdiff_stream_t stream);
size_t tmdiff_glp_moments_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W);
int tmdiff_glp_moments(const float* ms_exp, const float* pan, const float* pan_lp, int32_t B, int32_t C, int32_t H, int32_t W,
                       double* out, void* workspace, size_t workspace_bytes, tmdiff_stream_t stream);
int tmdiff_glp_inject(const float* ms_exp, const float* pan, const float* pan_lp, const double* moments, float* out, int32_t B,
                      int32_t C, int32_t H, int32_t W, int32_t mode, tmdiff_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Component-substitution pansharpening: GS, GSA, Brovey (csrc/cs_fusion.hip; host definitions: tmdiff_amd/metrics.py,
 * plane_moments / cs_coeffs / cs_inject / cs_fuse).  Dense tensors; nothing is allocated or synchronised, no atomics, the same
 * bits on every run and on a graph replay.
 *  plane_gram: ms [B, C, H, W], pan [B, 1, H, W] fp32 -> out, float64 [B, C + 1, C + 2]: the planes are the C bands, then the
 *             PAN; columns 0 .. C are their population covariance matrix (exactly symmetric), column C + 1 their means.  One
 *             pass with v_mfma_f64_16x16x4_f64 over tiles whose rows are the planes, minus their first pixel (a pilot), and a
 *             plane of ones; partial tiles per workgroup in `workspace` (8-byte aligned, tmdiff_plane_gram_workspace_bytes), a
 *             finalize launch adds them in index order.  The workspace then starts with the finished raw sums, float64
 *             [B, C + 2, C + 2] in the order bands, PAN, ones: sums of products of d = value - pilot, column C + 1 the sums of d,
 *             the corner n.  The summation order is written in the source's header.  Limits: B >= 0, 1 <= C <= 14, H, W >= 1,
 *             B * C * H * W <= 2^31 - 1; otherwise TMDIFF_E_UNSUPPORTED and a workspace size of 0.
 *  cs_coeffs: full, low: float64 [B, C + 1, C + 2] of plane_gram at the PAN scale and at the reduced scale (low may be null unless
 *             mode is 1) -> out, float64 [B, 2 C + 3]: alpha[C], g[C], a, mean_I, mean_P.  mode 0 "gs", 1 "gsa", 2 "brovey".
 *             gsa solves S_lr alpha = c_lr by a root-free unpivoted Cholesky factorisation (L D L') in one lane; a pivot <= 0 gives NaN.
 *  cs_inject: out [B, C, H, W] from ms_exp, pan and the device-resident `coef` of cs_coeffs; I = sum_k alpha_k M_k,
 *             P_I = a (P - mean_P) + mean_I; modes 0, 1: F_c = M_c + g_c (P_I - I); mode 2: F_c = M_c P_I / (I + 2^-52), in
 *             fp64, rounded to fp32 once.  out may be ms_exp; it must not overlap pan or coef.  Limits: plane_gram's.
 *             (Added within version 6.)
 * ------------------------------------------------------------------------------------ */
size_t tmdiff_plane_gram_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W);
int tmdiff_plane_gram(const float* ms, const float* pan, int32_t B, int32_t C, int32_t H, int32_t W, double* out, void* workspace,
                      size_t workspace_bytes, tmdiff_stream_t stream);
int tmdiff_cs_coeffs(const double* full, const double* low, double* out, int32_t B, int32_t C, int32_t mode,
                     tmdiff_stream_t stream);
int tmdiff_cs_inject(const float* ms_exp, const float* pan, const double* coef, float* out, int32_t B, int32_t C, int32_t H,
                     int32_t W, int32_t mode, tmdiff_stream_t stream);

/* ------------------------------------------------------------------------------------
 * BDSD pansharpening: band-dependent spatial detail (csrc/bdsd.hip; host definitions: tmdiff_amd/metrics.py, bdsd_moments /
 * bdsd_coeffs / bdsd_inject / bdsd).  Dense tensors; nothing is allocated or synchronised, no atomics, the same bits on every
 * run and on a graph replay.  An H x W image is cut into non-overlapping square blocks of side `bs` / `block` (0: the whole image
 * is one block), block (iy, ix) at index iy * (W / side) + ix.
 *  bdsd_gram:  low_lp, low_ms [B, C, H, W], low_pan [B, 1, H, W] fp32 (the reduced scale) -> out, float64 [B, blocks, C + 1,
 *              2 C + 1] = N | R per block: N = Hm' Hm with Hm = [low_lp_0 .. low_lp_{C-1}, low_pan] over the block's pixels
 *              (exactly symmetric), R = Hm' D with D_c = low_ms_c - low_lp_c formed in fp64.  Raw sums.  One pass with two
 *              v_mfma_f64_16x16x4_f64 per four pixels of each plane that share the A operand; partial sums per workgroup in
 *              `workspace` (8-byte aligned, tmdiff_bdsd_gram_workspace_bytes), a finalize launch adds them in index order.  The
 *              summation order is written in the source's header.  Limits: B >= 0, 1 <= C <= 15, H, W >= 1, B * C * H * W <=
 *              2^31 - 1, bs 0 or a divisor of H and W; otherwise TMDIFF_E_UNSUPPORTED and a workspace size of 0.
 *  bdsd_solve: moments, float64 [systems, C + 1, 2 C + 1] -> out, float64 [systems, C + 1, C]: column c solves N gamma_c = R_c by
 *              a root-free unpivoted Cholesky factorisation (L D L') in one lane per system; a pivot <= 0 gives NaN in that
 *              system.
 *  bdsd_inject: out [B, C, H, W] from ms_exp, pan [B, 1, H, W] and the device-resident weights `gamma` of bdsd_solve, float64
 *              [B, blocks, C + 1, C]: F_c = M_c + sum_k gamma[k][c] M_k + gamma[C][c] P with the weights of the pixel's block,
 *              one fp64 chain of fused multiply-adds in that order, rounded to fp32 once.  out may be ms_exp; it must not
 *              overlap pan or gamma.  Limits: bdsd_gram's, with `block` the full-scale side.
 *              (Added within version 6.)
 * ------------------------------------------------------------------------------------ */
size_t tmdiff_bdsd_gram_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W, int32_t bs);
int tmdiff_bdsd_gram(const float* low_lp, const float* low_pan, const float* low_ms, int32_t B, int32_t C, int32_t H, int32_t W,
                     int32_t bs, double* out, void* workspace, size_t workspace_bytes, tmdiff_stream_t stream);
int tmdiff_bdsd_solve(const double* moments, double* out, int32_t systems, int32_t C, tmdiff_stream_t stream);
int tmdiff_bdsd_inject(const float* ms_exp, const float* pan, const double* gamma, float* out, int32_t B, int32_t C, int32_t H,
                       int32_t W, int32_t block, tmdiff_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Conjugate gradients for Wald's consistency (csrc/cg.hip; host definition: tmdiff_amd/metrics.py, consistency_solve; the
 * driver: tmdiff_amd/ops.py, consistency_solve): per-plane dot products and the vector updates of CGLS with coefficients that
 * stay on the device.  Dense fp32 planes [planes, n]; nothing is allocated or synchronised, no atomics, no fences, the same
 * bits on every run and on a graph replay.  The chunks of a plane, the summation order and the coefficients' rounding are
 * written in the source's header.
 *  plane_dots_partials (host function): the partial sums of a plane of n elements, 1 .. 256, a function of n alone.
 *  plane_dots:    partials0[planes, plane_dots_partials(n0)] of <a0, b0> per plane, summed in fp64, and, when partials1 is not
 *                 NULL, partials1[planes, plane_dots_partials(n1)] of <a1, b1> over planes of n1 elements in the same launch.
 *                 b may be a (a squared norm: the plane is read once).
 *  plane_totals:  out[pl * items + k] = the total of the `count` partial sums at partials + k * item_stride + pl * count, added
 *                 in the order every consumer below adds them.
 *  cg_step:       alpha = gamma / (qq + damp * pp) per plane from the partial sums gamma, pp [planes, partials(n_full)] and qq
 *                 [planes, partials(n_low)] (pp is not read when damp == 0), 0 where the denominator is 0, rounded to float
 *                 once; d = fma(alpha, p, d) over n_full elements (first != 0: d = alpha * p, d is not read), r = fma(-alpha, q, r)
 *                 over n_low elements, and rr [planes, partials(n_low)] = the partial sums of the new <r, r>.
 *  cg_direction:  beta = gamma_new / gamma_old per plane, 0 where gamma_old is 0, rounded to float once; p = fma(beta, p, s); pp
 *                 (may be NULL) = the partial sums of the new <p, p>.
 *                 Limits: planes >= 0, n >= 0, planes * n <= 2^31 - 1, damp >= 0; otherwise TMDIFF_E_UNSUPPORTED.
 *                 (Added within version 6.)
 * ------------------------------------------------------------------------------------ */
int32_t tmdiff_plane_dots_partials(int32_t n);
int tmdiff_plane_dots(const float* a0, const float* b0, int32_t n0, double* partials0, const float* a1, const float* b1, int32_t n1,
                      double* partials1, int32_t planes, tmdiff_stream_t stream);
int tmdiff_plane_totals(const double* partials, double* out, int32_t planes, int32_t count, int32_t items, int64_t item_stride,
                        tmdiff_stream_t stream);
int tmdiff_cg_step(const float* p, const float* q, float* d, float* r, const double* gamma, const double* qq, const double* pp,
                   double damp, double* rr, int32_t planes, int32_t n_full, int32_t n_low, int32_t first, tmdiff_stream_t stream);
int tmdiff_cg_direction(const float* s, float* p, const double* gamma_new, const double* gamma_old, double* pp, int32_t planes,
                        int32_t n_full, tmdiff_stream_t stream);

/* ------------------------------------------------------------------------------------
 * TV pansharpening (csrc/tv.hip; host definitions: tmdiff_amd/metrics.py, tv_pd_step / tv_norm / tv_pansharpen; the driver:
 * tmdiff_amd/ops.py, tv_pansharpen): the band-coupled part of a Condat-Vu iteration and the vector total variation.  Dense fp32
 * images [B, C, H, W], pan [B, 1, H, W], weights float64 [B, C + 1] on the device (the band weights, then an offset).  Forward
 * differences with a zero last column / row; the transpose never reads ph[:, W - 1] nor pv[H - 1, :].  Nothing is allocated or
 * synchronised, no atomics, the same bits on every run and on a graph replay; the summation orders are written in the source's
 * header.
 *  tv_pd_step: with s = sum_c w_c x_c + w_C - pan per pixel,
 *                x'  = u - tau (gamma w_c s + D^T p)            rounded to fp32 once
 *                q   = p + sigma D (2 x' - x)                   from x' as stored, both components, all bands
 *                p'  = q / max(1, |q| / lam)                    |q| over the 2 C components of the pixel; lam == 0: p' = 0
 *              in fp64 after the loads.  One workgroup per 16 x 32 tile computes x' on the tile plus one column and one row and
 *              stores only the tile.  Every input is read with a halo, so no output may overlap an input or another output
 *              (TMDIFF_E_INVALID): the caller ping-pongs x and p.  tau > 0, sigma, lam, gamma >= 0.
 *  tv_norm:    out, float64 [B] = sum over the pixels of sqrt(sum_c (Dh x_c)^2 + (Dv x_c)^2), no eps; one partial sum per tile in
 *              `workspace` (8-byte aligned, tmdiff_tv_norm_workspace_bytes), a finalize launch adds them in index order.
 *              Limits of all three: B >= 0, 1 <= C <= 16, H, W >= 1, B * C * H * W <= 2^31 - 1; otherwise TMDIFF_E_UNSUPPORTED,
 *              a workspace size of 0 and tv_supported == 0.
 *              (Added within version 6.)
 * ------------------------------------------------------------------------------------ */
int tmdiff_tv_supported(int32_t B, int32_t C, int32_t H, int32_t W);
int tmdiff_tv_pd_step(const float* u, const float* x, const float* pan, const float* ph, const float* pv, const double* weights,
                      double tau, double sigma, double lam, double gamma, float* x_out, float* ph_out, float* pv_out, int32_t B,
                      int32_t C, int32_t H, int32_t W, tmdiff_stream_t stream);
size_t tmdiff_tv_norm_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W);
int tmdiff_tv_norm(const float* x, int32_t B, int32_t C, int32_t H, int32_t W, double* out, void* workspace, size_t workspace_bytes,
                   tmdiff_stream_t stream);

/* ------------------------------------------------------------------------------------
 * A-trous wavelet pansharpening (csrc/atrous.hip; host definitions: tmdiff_amd/metrics.py, atrous_lowpass / awlp_inject / awlp; the
 * driver: tmdiff_amd/ops.py, awlp): the approximation plane of the undecimated transform with the B3-spline filter and the ATWT /
 * AWLP injection.  Dense fp32 images.  Nothing is allocated or synchronised, no atomics, the same bits on every run and on a graph
 * replay; the summation order is written in the source's header.
 *  atrous_lowpass: out [B, C, H, W] = c_levels of every plane of x [B, C, H, W]: c_l = h_l * c_{l-1} with the separable
 *              (1, 4, 6, 4, 1) / 16 dilated by 2^(l-1) and every index clamped into the plane at every level; fp64 after the
 *              loads, each level rounded to fp32 once.  x is c_{first-1} (first = 1: the image) and the levels first ..
 *              first + levels - 1 run in one launch (one workgroup per 32 x 32 tile, the halo of 2^first (2^levels - 1) pixels
 *              staged in LDS); they equal `levels` single-level calls, first counting up, bit for bit.  x is read with a halo:
 *              out must not overlap x (TMDIFF_E_INVALID).  Limits: B, C, H, W >= 1, H, W <= 2^30, B * C * H * W <= 2^31 - 1,
 *              first, levels >= 1, first + levels <= 4; otherwise TMDIFF_E_UNSUPPORTED and atrous_supported == 0.
 *  awlp_inject: out [B, C, H, W] from ms_exp [B, C, H, W], pan and pan_lp [B, H, W] (ONE low-pass plane per image) and moments,
 *              float64 [B, C + 1, C + 2] on the device, 8-byte aligned: the layout of tmdiff_plane_gram for (ms_exp, pan_lp), of
 *              which the diagonal is read.  With a_c = sqrt(var(M_c) / var(L)), D = P - L and I = (sum_k M_k) / C:
 *                mode 0 "atwt":  F_c = M_c + a_c D        mode 1 "awlp":  F_c = M_c + ((M_c / I) a_c) D, and M_c where I == 0
 *              in fp64, rounded to fp32 once; var(L) == 0 is non-finite throughout.  out may be ms_exp itself; it must not
 *              overlap anything else (the caller checks).  Limits: B >= 1, 1 <= C <= 14, H, W >= 1, B * C * H * W <= 2^31 - 1,
 *              mode 0 or 1; otherwise TMDIFF_E_UNSUPPORTED.
 *              Both check their extents before the pointers (TMDIFF_E_INVALID for a null one) and before any launch.
 *              (Added within version 6.)
 * ------------------------------------------------------------------------------------ */
int tmdiff_atrous_supported(int32_t B, int32_t C, int32_t H, int32_t W, int32_t levels, int32_t first);
int tmdiff_atrous_lowpass(const float* x, float* out, int32_t B, int32_t C, int32_t H, int32_t W, int32_t levels, int32_t first,
                          tmdiff_stream_t stream);
int tmdiff_awlp_inject(const float* ms_exp, const float* pan, const float* pan_lp, const double* moments, float* out, int32_t B,
                       int32_t C, int32_t H, int32_t W, int32_t mode, tmdiff_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Standalone attention operators of core/Attention.py (imported by nothing in the reference; built because the
 * north star names them).  All fp32.
 *  attn_fwd : out = softmax(q k^T * scale [key mask]) v per (batch, head); fp32 MFMA, online softmax.
 *             q/k/v/out are addressed as base + b*strides[0] + head*strides[1] + row*strides[2] + d (elements),
 *             which covers both the '(b h) n d' split of CrossAttention (:186) and the channel-major
 *             [B, C, HW] tensors of SpatialSelfAttention (:143-153, via a transposed view prepared by the caller).
 *             key_mask [B, Nk] bytes (1 = keep) or NULL; head dim D even, <= 128.  A masked key scores -FLT_MAX (the
 *             reference's masked_fill, :203-204): a sample whose keys are all masked yields the mean of v over its Nk keys.
 *  attn_ctx_queries_per_workgroup (host function): the queries one workgroup of the small-context kernel walks over
 *             (128 per pass of its four waves) when attn_fwd is called with these extents, D == 64, Nk <= 96 and 16-byte
 *             aligned q / out rows; 0 when the extents rule that kernel out.
 *  attn_fwd_lse : attn_fwd, and LSE[b, h, query] = max + log(sum exp) of the scaled (and masked) scores into lse [B, H, Nq].
 *             The forward of the differentiable path: the same kernels on the same extents, each instantiated once more with
 *             the store, so `out` equals attn_fwd's bit for bit.  A sample whose keys are all masked gets LSE = -FLT_MAX.
 *  attn_bwd : dq, dk, dv of attn_fwd_lse from dout (addressed with out's strides; dq / dk / dv with those of q / k / v), `out`
 *             and `lse`; any of dq / dk / dv may be NULL (not wanted).  Three launches on `stream`, no atomics (bitwise
 *             reproducible): Delta = rowsum(dout * out) into `workspace` (attn_bwd_workspace_bytes, never NULL), then one
 *             kernel that walks the key tiles per 128 queries (dq) and one that walks the query tiles per 128 keys (dk, dv);
 *             both re-form P = exp(S - LSE).  Masked keys get dk = dv = 0 exactly; a sample whose keys are all masked gets
 *             dq = dk = 0 and dv = (1 / Nk) * sum over the queries of dout.
 *             Extents (attn_bwd_supported, a host function: 1 / 0): those of attn_fwd (positive, B * H <= 65535, D even and
 *             <= 128), and q / out and k / v hold at most 2^31 - 1 elements each (B * H * Nq * D, B * H * Nk * D): row and
 *             statistics indices are 32-bit, element offsets 64-bit.  Larger extents return TMDIFF_E_UNSUPPORTED without
 *             launching, and the workspace size is 0 for anything refused.
 *             (attn_fwd_lse, attn_bwd, attn_bwd_supported and attn_bwd_workspace_bytes were added within version 6.)
 *  gemm_nt  : C[M,N] = A[M,K] W[N,K]^T + bias[N] + residual[M,N]   (nn.Linear on token-major activations)
 *  group_norm (:108-109, eps 1e-6, affine), layer_norm (:279-281), geglu / gelu (:69-76, :84-87).
 *  layer_norm_stats / group_norm_stats : the forwards of the differentiable path -- layer_norm / group_norm, and the statistics
 *             mean, rstd = 1 / sqrt(var + eps) into mean / rstd ([rows] and [B, groups]).  The same kernels instantiated once
 *             more with the store, so `y` equals the plain entry point's bit for bit.
 *  layer_norm_bwd : with g = dy * gamma and xhat = (x - mean) * rstd, dx = rstd * (g - mean_D(g) - xhat * mean_D(g * xhat)),
 *             dgamma[j] = sum_r dy[r, j] * xhat[r, j], dbeta[j] = sum_r dy[r, j]; any of dx / dgamma / dbeta may be NULL (not
 *             wanted).  One wave per row; each workgroup writes the column sums of its fixed block of rows into `workspace`
 *             (layer_norm_bwd_workspace_bytes; may be NULL when neither dgamma nor dbeta is wanted), a second launch adds
 *             the partials in block order.  No atomics: bitwise reproducible.  Extents (layer_norm_bwd_supported, a host
 *             function: 1 / 0): 1 <= D <= 4096, rows >= 0 and rows * D < 2^31.  Anything else returns TMDIFF_E_UNSUPPORTED
 *             without launching, and its workspace size is 0.
 *  group_norm_bwd : the same for x [B, C, P] normalised per (b, group), gamma / dgamma / dbeta [C] (gamma NULL = 1).  One
 *             workgroup per (b, group): a first pass forms the per-channel sums of dy and dy * xhat -- the [B, C] partials of
 *             dbeta / dgamma in `workspace` (group_norm_bwd_workspace_bytes), and, weighted by gamma, the two group sums --
 *             a second pass writes dx, a tail launch sums the partials over b in order.  Extents (group_norm_bwd_supported):
 *             those of group_norm (groups divides C, B <= 65535) and B * C * P < 2^31; refusals as for layer_norm_bwd.
 *  geglu_bwd : u [rows, 2 * inner] = (a | gate), dy [rows, inner] -> du[:, :inner] = dy * gelu(gate), du[:, inner:] =
 *             dy * a * (Phi(gate) + gate * phi(gate)), the exact erf GELU of the forward; gelu_only = 1: u, dy, du
 *             [rows, inner], du = dy * (Phi(u) + u * phi(u)).  float4 accesses where inner % 4 == 0 (and 16-byte bases).
 *             (layer_norm_stats, group_norm_stats, layer_norm_bwd, group_norm_bwd, geglu_bwd and the *_supported /
 *             *_workspace_bytes functions of the two norms were added within version 6.)
 * ------------------------------------------------------------------------------------ */
int tmdiff_attn_fwd(const float* q, const float* k, const float* v, float* out, const unsigned char* key_mask,
                    int32_t B, int32_t H, int32_t Nq, int32_t Nk, int32_t D, const int64_t q_strides[3],
                    const int64_t k_strides[3], const int64_t v_strides[3], const int64_t o_strides[3], float scale,
                    tmdiff_stream_t stream);
int32_t tmdiff_attn_ctx_queries_per_workgroup(int32_t B, int32_t H, int32_t Nq, int32_t Nk, int32_t D);
int tmdiff_attn_fwd_lse(const float* q, const float* k, const float* v, float* out, const unsigned char* key_mask,
                        int32_t B, int32_t H, int32_t Nq, int32_t Nk, int32_t D, const int64_t q_strides[3],
                        const int64_t k_strides[3], const int64_t v_strides[3], const int64_t o_strides[3], float scale,
                        float* lse, tmdiff_stream_t stream);
int tmdiff_attn_bwd_supported(int32_t B, int32_t H, int32_t Nq, int32_t Nk, int32_t D);
size_t tmdiff_attn_bwd_workspace_bytes(int32_t B, int32_t H, int32_t Nq, int32_t Nk, int32_t D);
int tmdiff_attn_bwd(const float* q, const float* k, const float* v, const float* out, const float* dout, const float* lse,
                    const unsigned char* key_mask, float* dq, float* dk, float* dv, void* workspace, int32_t B, int32_t H,
                    int32_t Nq, int32_t Nk, int32_t D, const int64_t q_strides[3], const int64_t k_strides[3],
                    const int64_t v_strides[3], const int64_t o_strides[3], float scale, tmdiff_stream_t stream);
int tmdiff_gemm_nt(const float* A, const float* Wt, const float* bias, const float* residual, float* C, int64_t M,
                   int32_t N, int32_t K, tmdiff_stream_t stream);
int tmdiff_group_norm(const float* x, const float* gamma, const float* beta, float* y, int32_t B, int32_t C,
                      int64_t P, int32_t groups, float eps, tmdiff_stream_t stream);
int tmdiff_layer_norm(const float* x, const float* gamma, const float* beta, float* y, int64_t rows, int32_t D,
                      float eps, tmdiff_stream_t stream);
int tmdiff_geglu(const float* u, float* y, int64_t rows, int32_t inner, int32_t gelu_only, tmdiff_stream_t stream);
int tmdiff_layer_norm_stats(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                            int64_t rows, int32_t D, float eps, tmdiff_stream_t stream);
int tmdiff_group_norm_stats(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                            int32_t B, int32_t C, int64_t P, int32_t groups, float eps, tmdiff_stream_t stream);
int tmdiff_layer_norm_bwd_supported(int64_t rows, int32_t D);
size_t tmdiff_layer_norm_bwd_workspace_bytes(int64_t rows, int32_t D);
int tmdiff_layer_norm_bwd(const float* x, const float* gamma, const float* dy, const float* mean, const float* rstd, float* dx,
                          float* dgamma, float* dbeta, void* workspace, int64_t rows, int32_t D, tmdiff_stream_t stream);
int tmdiff_group_norm_bwd_supported(int32_t B, int32_t C, int64_t P, int32_t groups);
size_t tmdiff_group_norm_bwd_workspace_bytes(int32_t B, int32_t C, int64_t P, int32_t groups);
int tmdiff_group_norm_bwd(const float* x, const float* gamma, const float* dy, const float* mean, const float* rstd, float* dx,
                          float* dgamma, float* dbeta, void* workspace, int32_t B, int32_t C, int64_t P, int32_t groups,
                          tmdiff_stream_t stream);
int tmdiff_geglu_bwd(const float* u, const float* dy, float* du, int64_t rows, int32_t inner, int32_t gelu_only,
                     tmdiff_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Per-operator names (SURVEY 8b "minimum exports").  Thin, argument-checked fronts of the entry points above for
 * callers that bind one symbol per ATen call they replace:
 *  conv3d_k{3,1}_fwd   = tmdiff_conv3d_fwd with d->ksize required to be 3 / 1            (F.conv3d / nn.Conv3d)
 *  conv3d_k{3,1}_dgrad = the same kernel on mode-1 packed weights: d->seg_x[0] = dL/dy, d->y = dL/dx'
 *  conv3d_k{3,1}_wgrad = tmdiff_conv3d_wgrad
 *  haar_dwt2d_fwd / haar_idwt2d_fwd = the transforms; *_bwd = their adjoints
 *    dwt2d_bwd : dx = IDWT(ll_scale*g_ll, hi_scale*(g_lh, g_hl, g_hh))  (DWTFunction_2D.backward, DWT_IDWT_Functions.py:60-69);
 *                the three high-band gradients must be all NULL (LL-only forward) or all given, and then
 *                hi_scale must be 1 (the hot path only ever scales the LL band, Hyper_unet_general.py:396).
 *    idwt2d_bwd: g_ll = in_scale * LL(g_out), (g_lh, g_hl, g_hh) = high bands of DWT(g_out)               (IDWTFunction_2D.backward, :101-112)
 *  dpm_axpby{2,3,4}: out = sum_k coef_k * in_k with exactly 2 / 3 / 4 terms (dpm_solver_pytorch.py:563-927).
 * ------------------------------------------------------------------------------------ */
int tmdiff_conv3d_k3_fwd(const tmdiff_conv3d_desc* d, tmdiff_stream_t stream);
int tmdiff_conv3d_k3_dgrad(const tmdiff_conv3d_desc* d, tmdiff_stream_t stream);
int tmdiff_conv3d_k3_wgrad(const tmdiff_conv3d_desc* d, const float* g, float* dw, void* workspace,
                           tmdiff_stream_t stream);
int tmdiff_conv3d_k1_fwd(const tmdiff_conv3d_desc* d, tmdiff_stream_t stream);
int tmdiff_conv3d_k1_dgrad(const tmdiff_conv3d_desc* d, tmdiff_stream_t stream);
int tmdiff_conv3d_k1_wgrad(const tmdiff_conv3d_desc* d, const float* g, float* dw, void* workspace,
                           tmdiff_stream_t stream);
int tmdiff_haar_dwt2d_fwd(const float* x, float* ll, float* lh, float* hl, float* hh, int64_t planes, int32_t H,
                          int32_t W, float ll_scale, float hi_scale, tmdiff_stream_t stream);
int tmdiff_haar_dwt2d_bwd(const float* g_ll, const float* g_lh, const float* g_hl, const float* g_hh, float* dx,
                          int64_t planes, int32_t H, int32_t W, float ll_scale, float hi_scale,
                          tmdiff_stream_t stream);
int tmdiff_haar_idwt2d_fwd(const float* ll, const float* lh, const float* hl, const float* hh, float* out,
                           int64_t planes, int32_t h, int32_t w, float in_scale, tmdiff_stream_t stream);
int tmdiff_haar_idwt2d_bwd(const float* g_out, float* g_ll, float* g_lh, float* g_hl, float* g_hh, int64_t planes,
                           int32_t h, int32_t w, float in_scale, tmdiff_stream_t stream);
int tmdiff_dpm_axpby2(const float* x0, float c0, const float* x1, float c1, float* out, int64_t n,
                      tmdiff_stream_t stream);
int tmdiff_dpm_axpby3(const float* x0, float c0, const float* x1, float c1, const float* x2, float c2, float* out,
                      int64_t n, tmdiff_stream_t stream);
int tmdiff_dpm_axpby4(const float* x0, float c0, const float* x1, float c1, const float* x2, float c2,
                      const float* x3, float c3, float* out, int64_t n, tmdiff_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TMDIFF_HIP_H */
