"""Which kernel family runs each 3x3x3 convolution, and what its epilogue additionally does: the ONE place both decisions are
taken (host logic only, no GPU work).

A *family* is a C entry point of libtmdiff_hip.so with the kernel behind it:

  family    C entry point                   kernel (csrc/)                                       executes per output
  --------  ------------------------------  ---------------------------------------------------  -------------------
  wf        tmdiff_conv3d_wf_fwd            conv3d_wf_kernel<2,8,16> (8 bands) / <1,16,16> (4)   13.5 multiply-adds / ci
  wf_pair   tmdiff_conv3d_wf_fwd            conv3d_wf_kernel<2,8,16,PAIR> (8 bands x 8 columns)  13.5
  wfll      tmdiff_conv3d_wfll_fwd          conv3d_wf_kernel<..., LLM> (Conv_0 + LL composed)    24 per quarter-res output
  ll        tmdiff_conv3d_ll_fwd            conv3d_ll_kernel (Conv_0 + LL composed, direct)      48 per quarter-res output
  staged    tmdiff_conv3d_fwd_staged        (prologue_apply_kernel +) conv3d_dma_kernel          27
  fused     tmdiff_conv3d_fwd               conv3d_mfma_kernel (prologue applied while staging)  27
  bf16      tmdiff_conv3d_fwd_bf16          (pack_x_bf16_kernel +) conv3d_bf16_dma_kernel        27, bf16 operands
  wino4/2   tmdiff_conv3d_wino_fwd_planes   wino_input_kernel + conv3d_wino_kernel               13.5 / 18 -- tmdiff_amd.fallback

`conv3_family` decides from the extents alone (plus what the input looks like), so the decision for every layer of every
BASELINE configuration can be tabulated without a GPU: `unet_conv3_layers` enumerates the 3x3x3 convolutions of one WavBEST
forward (reference GeneralModel/Hyper_unet_general.py:600-636 -- 51 of its 73 convolution calls), `unet_table` routes them.
`tools/routing_table.py` writes the table to profiles/ and tests/test_host_logic.py asserts it: every family of the product
path is reached by some BASELINE configuration, and the `fallback` families (band counts other than 4 / 8) by none.

The rules, in order (fp32):
  1. Winograd F(4,3) along the bands with the transform inside the kernel (wf): 8- or 4-band tensors, W % 4 == 0, Cin/g even,
     Cout/g % 32 == 0, no mask tensor; the plan of the kernel itself (tmdiff_conv3d_wf_plan: tiles, split-K factor) must reach
     `config.wino_min_blocks` workgroups and the plane must fill `config.wf_min_fill` of its 8 x 16 / 16 x 16 tiles (8 bands x
     8 columns: two images per tile, pair mode).
  2. other even band counts whose grid is large enough: transform pass + Winograd kernel (wino4 / wino2, tmdiff_amd.fallback).
  3. the direct kernels, whose split-K fills the chip on small grids: staged (operands by LDS-DMA; needs Cin/g % 4 == 0 and
     Cout/g % 32 == 0) where the input is plain or the prologue pass is amortised (Cout/g >= 128, Cin/g >= 384, dropout / mask,
     a kept x'), else fused.
What a launch's epilogue additionally does in the fp32 inference graph is decided here too: the rules below, composed per block
by `resblock_plan` / `down_plan` (WavBEST reads the channel counts and its set of bf16 convolutions off its modules, asks for
the plan and executes it); `unet_fusions` tabulates the plans per block, `tools/routing_table.py --fusions` writes
profiles/fusion_table.txt:

  fusion                        descriptor fields            rule
  ----------------------------  ---------------------------  ------------------------------------------------------------------
  fold a 1x1x1 conv (res_conv,  rc_x, rc_w, rc_cin           fold_k1: one input tensor of 32 .. 512 channels (% 32), consumer on
    Conv_2) into its consumer                                conv3d_wf outside the pair mode (split-K allowed), rc_x size limit
  side x' of a segmented        xp_out, xp_shift, xp_act     side_xp: conv20 on conv3d_wf (pair mode, split-K allowed), res_conv
    res_conv launch                                          on a bandwidth kernel that can (k1_side_xp)
  conv21 writes LL(y) / 2       y_ll                         emit_ll: 8 bands, unsplit conv3d_wf launch outside the pair mode,
  Conv_0 writes the Haar bands  y_ll, y_hi                   even H, W % 4 == 0 (wf_launch and wf_quarter_ok); switch emit_dwt
  second output space-to-depth  y2_s2d                       s2d_handover: conv21 an unsplit conv3d_wf launch, composed weights
    (Conv_0 + LL on "wfll")                                  exist, wfll_route takes the composed convolution
  Conv_0 + LL on "ll"           (tmdiff_conv3d_ll_fwd)       ll_fits: the direct composed kernel's size limit
Each rule also reads its switches (fuse_res_conv, side_xp, emit_ll / emit_dwt, conv2_after_ll, epilogue_fuse, wfll, ll_compose,
winograd) and declines as soon as a convolution involved runs on the bf16 kernels.

The finetune graph (WavBEST.forward_train + backward) takes its decisions here as well: one plan per differentiable convolution
(train_conv_plan, train_ll_plan) and per block (train_down_plan, train_resblock_plan), which tmdiff_amd.autograd and the block
classes' `run` execute; `unet_train_launches` walks forward_train's blocks over the plans and gives the step's launches in the
keys of ops.COUNTS, `tools/routing_table.py --train` writes profiles/train_routing_table.txt.  The rules:
  4. forward and data gradient (a plain-input convolution Cout -> Cin): rules 1-3; 1x1x1 convolutions on the bandwidth kernel.
  5. x' is kept for the weight gradient where dropout (or a mask) forces a prologue pass anyway, the weight wants a gradient
     and the staged kernel takes the weight shape (staged_weight_ok: rule 3's shape test); a kept x' forces a kernel with a pass.
  6. weight gradient (wgrad_family): Winograd F(3,4) along the bands where config.wgrad_wino, 3x3x3 and
     tmdiff_conv3d_wgrad_wino_supported, else direct; the bias gradient rides in it with config.wgrad_bias, or in the
     Winograd kernel's g pass with config.wgrad_wino_bias, else a channel sum of its own.
  6b. config.grad_bf16 (opt-in; the forward is untouched): the data gradient of a 3x3x3 convolution on conv3d_bf16 where
     dgrad_bf16_ok (Cin/g % 32 == 0, Cout/g % 8 == 0): family "bf16" in the plan, whose dgrad_math / wgrad_math name the
     arithmetic.  The weight gradient stays on rule 6's fp32 families in EVERY layer class: measured at local batch 8
     (profiles/train_bf16_grad.txt), the bf16 weight-gradient kernel (csrc/wgrad_bf16.hip, ops.conv3d_wgrad_bf16) is 2.0 - 3.7x
     slower than tmdiff_conv3d_wgrad_wino in all 20 classes of the 32-256 network, so no class is routed to it.
  7. Conv_0 + LL of a main-branch down block is one node where the composed form exists (ll_composable) and ll_fits: on
     conv3d_wf's composed mode with config.train_ll_wino where wfll_route takes it, else on conv3d_ll; Conv_2 after the LL
     band with config.conv2_after_ll.
  8. a ResBlock is one autograd node (config.train_fused_resblock) with its res_conv inside, or, without one, on a
     one-tensor input; else a node per convolution.

Batch-size note (README): the same sample can take different families at B = 1 and B = 32 (rule 1's grid threshold), hence
different fp32 summation orders; tests/test_gpu_configs.py bounds the difference at 1e-5.
"""
import collections
import ctypes as C

from . import _lib
from ._lib import lib

PRODUCT_FAMILIES = ("wf", "wf_pair", "wfll", "ll", "staged", "fused", "bf16")
FALLBACK_FAMILIES = ("wino4", "wino2")


def _config():
    from . import ops
    return ops.config


def _grad_bf16():
    """config.grad_bf16 (a configuration without the field: off)"""
    return bool(getattr(_config(), "grad_bf16", False))


def wino_weight_ok(cout, cin, ksize=3, groups=1):
    """Weight shapes the Winograd kernels (conv3d_wf, fallback.conv3d_wino) take."""
    return (ksize == 3 and groups in (1, 3) and cin % groups == 0 and cout % groups == 0 and (cin // groups) % 2 == 0 and
            (cout // groups) % 32 == 0)


def staged_weight_ok(cout, cin, groups=1):
    """Weight shapes the staged direct kernel (conv3d_dma: operands by LDS-DMA) takes; its prologue pass is what keeps x'."""
    return (groups in (1, 3) and cin % groups == 0 and cout % groups == 0 and (cin // groups) % 4 == 0 and
            (cout // groups) % 32 == 0)


def ll_weight_ok(cout, cin, ksize=3, groups=1):
    """Weight shapes that have the composed Conv_0 + LL forms (conv3d_ll; conv3d_wf's composed-LL mode: Cout % 32, implied)."""
    return ksize == 3 and groups == 1 and cin % 2 == 0 and cout % 64 == 0


_WF_ROUTES = {}      # (the plan is a pure function of the extents and the switches: one library call per distinct shape)


def wf_route(b, cin, cout, n, h, w, groups=1, masked=False, llm=False):
    """(taken, split): whether conv3d_wf runs a convolution of these extents and into how many ranges it splits the input
    channels (1 = no split-K).  llm: the composed Conv_0 + LL mode (cin, h, w those of the space-to-depth tensor)."""
    cfg = _config()
    key = (b, cin, cout, n, h, w, groups, masked, llm, cfg.key())
    r = _WF_ROUTES.get(key)
    if r is None:
        if len(_WF_ROUTES) > 4096:
            _WF_ROUTES.clear()
        r = _WF_ROUTES[key] = _wf_route(cfg, b, cin, cout, n, h, w, groups, masked, llm)
    return r


def _wf_route(cfg, b, cin, cout, n, h, w, groups, masked, llm):
    if cin % groups or cout % groups or masked or not cfg.wf:
        return False, 1
    tiles = C.c_int64(0)
    split = lib.tmdiff_conv3d_wf_plan(b, cin, cout, n, h, w, groups, 1 if llm else 0, C.byref(tiles))
    if split == 0:
        return False, 1
    if not cfg.wf_splitk:
        split = 1
    th = 8 if n == 8 else 16
    pair = n == 8 and w == 8          # two images side by side in one 8 x 16 tile
    if pair and not cfg.wf_pair:
        return False, 1
    fill = (h * w) / float(((h + th - 1) // th) * th * (8 if pair else ((w + 15) // 16) * 16))
    if pair:
        fill *= b / (2.0 * ((b + 1) // 2))        # (an odd batch leaves the last pair's second half empty)
    return bool(tiles.value * split >= cfg.wino_min_blocks and fill >= cfg.wf_min_fill), split


_QUERIES = {}        # (the support queries below are pure functions of the extents and the fields set: one call per shape)


def supported(query, b, cin, cout, n, h, w, groups=1, **fields):
    """The library's support query `query` (e.g. "tmdiff_conv3d_ll_supported") for a 3x3x3 convolution of these extents on one
    input tensor of cin channels -- or, cin a tuple, on segments of that many channels each --, with the descriptor fields
    `fields` set (in_act=1: an input that needs a prologue; rc_x=1, rc_cin=: a folded residual convolution; pointers are
    placeholders, never dereferenced).  Where the size limits of the 32-bit offsets live.
    The answers are cached per process: the library reads the switches they depend on (TMDIFF_WINO_F4 and the like) once
    per process too."""
    key = (query, b, cin, cout, n, h, w, groups, tuple(sorted(fields.items())))
    r = _QUERIES.get(key)
    if r is None:
        if len(_QUERIES) > 4096:
            _QUERIES.clear()
        seg_c = cin if isinstance(cin, tuple) else (cin,)
        d = _lib.Conv3dDesc()
        d.B, d.N, d.H, d.W, d.Cin, d.Cout, d.groups, d.ksize, d.nseg = b, n, h, w, sum(seg_c), cout, groups, 3, len(seg_c)
        for i, c in enumerate(seg_c):
            d.seg_c[i] = c
        for k, v in fields.items():
            setattr(d, k, v)
        r = _QUERIES[key] = bool(getattr(lib, query)(C.byref(d)))
    return r


def wino2d_ok(b, cin, cout, n, h, w, groups=1):
    """The shapes conv3d_w2 (Winograd along the bands and the width: transform passes + one GEMM per plane) takes: the deep
    layers -- fp32, groups 1, 8 or 4 bands, Cout >= 256 (% 64), Cin >= 128 (% 32), planes of even width <= 16 and 4 .. 32 rows,
    Winograd-domain arrays within 32-bit byte offsets per plane.  The mirror of tmdiff_conv3d_w2_supported for a convolution
    on ONE plain-or-prologue input tensor with a y / y2 / residual epilogue (tests/test_conv3d_w2_host.py holds the two together)."""
    if groups != 1 or b <= 0 or n not in (4, 8) or w < 2 or w > 16 or w % 2 or h < 4 or h > 32:
        return False
    if cin < 128 or cin % 32 or cout < 256 or cout % 64:
        return False
    q, tw = b * (n // 4), w // 2
    ip, op = (h + 2) * tw, h * tw
    g = max(1, min(q, 256 // op, 384 // ip))
    return (4 * cin * q * ip < (1 << 31) and 4 * cout * q * op < (1 << 31) and 12 * cin * cout < (1 << 31) and q <= 65535 and
            ((q + g - 1) // g) * (cout // 64) * 24 < 0x7fffffff)


def wino2d_route(b, cin, cout, n, h, w, groups=1):
    """True when a convolution of these extents that conv3_family gave to conv3d_wf runs on conv3d_w2 instead (config.wino2d).
    ops.conv3d_auto adds what it knows of the launch: one input tensor, no mask / dropout; a launch with a folded 1x1x1 or an
    LL / Haar / space-to-depth output asks wino2d_epilogue_route instead."""
    return bool(_config().wino2d and wino2d_ok(b, cin, cout, n, h, w, groups))


def wino2d_epilogue_ok(b, cin, cout, n, h, w, groups=1, rc_cin=0, quarter=False):
    """The launches conv3d_w2 takes beyond wino2d_ok's plain epilogue, on its row-pair output pass: the shapes of wino2d_ok
    with a folded 1x1x1 of rc_cin input channels (rc_cin % 32 == 0, at most 512; no residual tensor beside it) and / or, quarter,
    the quarter-resolution outputs (LL instead of y, the whole Haar transform, the space-to-depth second output: 8 bands) --
    either on an even number of rows.  The mirror of tmdiff_conv3d_w2_epilogue_supported for the descriptors ops.conv3d_w2
    builds (tests/test_conv3d_w2_epilogue_host.py holds the two together); with neither it is wino2d_ok."""
    if not wino2d_ok(b, cin, cout, n, h, w, groups):
        return False
    if not rc_cin and not quarter:
        return True
    if h % 2 or (quarter and n != 8):
        return False
    return not rc_cin or (rc_cin > 0 and rc_cin % 32 == 0 and rc_cin <= 512 and rc_cin * n * h * w < (1 << 30))


def wino2d_epilogue_route(b, cin, cout, n, h, w, groups=1, rc_cin=0, quarter=False):
    """True when a conv3d_wf launch with a folded 1x1x1 and / or quarter-resolution outputs runs on conv3d_w2 instead: both
    switches (config.wino2d, config.wino2d_epilogue) and wino2d_epilogue_ok.  All three classes of the benchmark step
    (256->256 at 8x16x16: LL + folded 1x1x1 with a plain or a space-to-depth second output, the whole Haar transform)
    measured faster than on conv3d_wf (profiles/wino2d_epilogue.txt): none is held back."""
    cfg = _config()
    return bool(cfg.wino2d and cfg.wino2d_epilogue and wino2d_epilogue_ok(b, cin, cout, n, h, w, groups, rc_cin, quarter))


def wfll_route(b, cin, cout, n, h, w):
    """True when conv3d_wf's composed-LL mode takes Conv_0 + LL of a [b, cin, n, h, w] input (h, w: full resolution)."""
    if not (_config().wfll and n in (4, 8) and h % 2 == 0 and w % 8 == 0 and cout % 32 == 0):
        return False
    return wf_route(b, 4 * cin, cout, n, h // 2, w // 2, llm=True)[0]


def wino_plan(b, cout, n, h, w, groups=1, cin=None):
    """(planes, workgroups) of the transform-pass Winograd kernel for these extents; planes 0 = not taken.  cin: also check the
    kernel's size limits (tmdiff_conv3d_wino_supported)."""
    planes = lib.tmdiff_conv3d_wino_planes(int(n))
    if not planes or w % 4:
        return 0, 0
    if cin is not None and not supported("tmdiff_conv3d_wino_supported", b, cin, cout, n, h, w, groups):
        return 0, 0
    cg = cout // groups
    per_tile = b * groups * ((h + 7) // 8) * (((w + 7) // 8) * (cg // 64) if cg % 64 == 0 else ((w + 15) // 16) * (cg // 32))
    blocks = lambda p: per_tile * ((n // (p - 2) + 1) // 2)          # (= tmdiff_conv3d_wino_blocks)
    mn = _config().wino_min_blocks
    if planes == 6 and blocks(6) < mn <= blocks(4):
        planes = 4                   # F(2,3) has twice the tiles along the bands: it still fills the chip here
    return (planes, blocks(planes)) if blocks(planes) >= mn else (0, blocks(planes))


def conv3_family(b, cin, cout, n, h, w, groups=1, plain=True, masked=False, dropout=False, keep_xp=False, math="fp32"):
    """The family that runs a 3x3x3 convolution [b, cin, n, h, w] -> cout.  plain: the input is one tensor (or the three
    tensors of a grouped convolution's three groups) with no prologue; masked: a dropout MASK TENSOR multiplies the input
    (parity runs); dropout: in-kernel dropout; keep_xp: the caller wants the prologue output x' kept (finetune)."""
    cfg = _config()
    if math == "bf16":
        return "bf16"
    if cfg.winograd and not masked and wino_weight_ok(cout, cin, 3, groups):
        # (an input that is not plain goes through conv3d_wf's prologue pass, which has size limits of its own; conservative
        #  for a grouped convolution's three plain segments, which conv3d_wf reads in place: declined at B * Cin > 65535)
        if wf_route(b, cin, cout, n, h, w, groups, masked)[0] and (
                plain or supported("tmdiff_conv3d_wf_supported", b, cin, cout, n, h, w, groups, in_act=1)):
            return "wf_pair" if (n == 8 and w == 8) else "wf"
        planes, _ = wino_plan(b, cout, n, h, w, groups, cin=cin)
        if planes:
            return "wino4" if planes == 6 else "wino2"
    return direct_family(cin, cout, groups, plain, masked, dropout, keep_xp, extents=(b, n, h, w))


def direct_family(cin, cout, groups=1, plain=True, masked=False, dropout=False, keep_xp=False, extents=None):
    """"staged" or "fused" for a 3x3x3 convolution on the direct kernels.  Measured (tools/bench_conv.py, B = 32): the staged
    kernel itself is 3-6 % faster than the fused one, but its prologue pass costs 8 B per input element -- a net win when the
    input needs no pass (one plain tensor: every data-gradient convolution), is shared by >= 2 channel tiles (Cout/g >= 128),
    is wide (Cin/g >= 384), or carries a dropout mask (the fused kernel reads the mask inside its MFMA stream); a kept x'
    (finetune) forces it.  Both give the same bits (tests/test_gpu_kernels.py::test_conv3d_staged_equals_fused).
    extents = (b, n, h, w): also check the staged kernel's size limits (tmdiff_conv3d_fwd_staged_supported)."""
    cin_g, cout_g = cin // groups, cout // groups
    staged_ok = staged_weight_ok(cout, cin, groups)
    if staged_ok and extents is not None:
        b, n, h, w = extents
        staged_ok = supported("tmdiff_conv3d_fwd_staged_supported", b, cin, cout, n, h, w, groups,
                              in_act=0 if plain and not masked and not dropout else 1)
    want = {"0": False, "1": True}.get(_config().fp32_staged, plain or cout_g >= 128 or cin_g >= 384 or masked or dropout)
    return "staged" if staged_ok and (want or keep_xp) else "fused"


def k1_side_xp(b, seg_c, cout, n, h, w, groups=1):
    """True when a 1x1x1 convolution of the segments seg_c (channels each) runs on a form of the bandwidth kernel that can also
    write the prologue output of its input (make_conv_desc side_xp=; csrc/conv1.hip conv1_fp32_try): segments and Cin / groups
    of multiples of 16 channels, Cout / groups % 32 == 0, planes of multiples of 4 positions, and either at least 512 tiles of
    512 positions (the 16-byte kernel) or a small grid of at least 128 input channels per group (the kernel that splits the
    channels over its waves); contiguous torch tensors are 16-byte aligned.  tmdiff_conv3d_fwd_xp_supported is the library's own answer for a filled descriptor."""
    cin, plane = sum(seg_c), n * h * w
    if cin % groups or cout % groups or any(c % 16 for c in seg_c) or (cin // groups) % 16 or (cout // groups) % 32 or plane % 4:
        return False
    cout_g = cout // groups
    co_tiles = cout_g // 64 if cout_g % 64 == 0 else cout_g // 32
    vec = b * groups * ((plane + 511) // 512) * co_tiles >= 512                                   # the 16-byte kernel
    small = b * groups * ((plane + 255) // 256) * co_tiles < 512 and (cin // groups) // 16 >= 8    # channels over the waves
    return (vec or small) and plane * 16 < (1 << 31) and cin * plane < (1 << 30)


def ll_composable(cin, cout, h, w):
    """Conv_0 + LL of a cin -> cout down block on h x w planes has a composed form at all (switch, weight shape, even planes)."""
    return bool(_config().ll_compose and ll_weight_ok(cout, cin) and h % 2 == 0 and w % 2 == 0)


def ll_family(b, cin, cout, n, h, w, producer_s2d=True):
    """Conv_0 + halved LL band of a main-branch down block on a [b, cin, n, h, w] input: "wfll" (the producer hands over its
    second output in space-to-depth form), "ll" (composed, direct), or None (convolution + LL-only DWT)."""
    if not ll_composable(cin, cout, h, w):
        return None
    if _config().winograd and producer_s2d and wfll_route(b, cin, cout, n, h, w):
        return "wfll"
    return "ll" if ll_fits(b, cin, cout, n, h, w) else None


def ll_fits(b, cin, cout, n, h, w):
    """True when conv3d_ll takes Conv_0 + LL of a [b, cin, n, h, w] input (h, w: full resolution), its size limit included."""
    return supported("tmdiff_conv3d_ll_supported", b, cin, cout, n, h, w)


def wf_fold_fits(b, cin, cout, n, h, w, rc_cin):
    """True when conv3d_wf can fold a residual 1x1x1 convolution of rc_cin input channels into its epilogue at these extents
    (the size limit of its rc_x offsets; the whole rule: fold_k1)."""
    return supported("tmdiff_conv3d_wf_supported", b, cin, cout, n, h, w, rc_x=16, rc_cin=rc_cin)


# ---- what a launch's epilogue additionally does: the fusions of the fp32 inference graph -------------------------------------
# Functions of the extents, ops.config and a math string ("bf16" as soon as one of the convolutions involved runs on the bf16
# kernels); WavBEST asks once per block per forward (through the plans below), so the answers are kept per (arguments,
# config.key()) like wf_route's.
_FUSIONS = {}


def _cached(fn):
    def ask(*args):
        key = (fn.__name__, args, _config().key())
        r = _FUSIONS.get(key)
        if r is None:
            if len(_FUSIONS) > 4096:
                _FUSIONS.clear()
            r = _FUSIONS[key] = fn(*args)
        return r
    ask.__name__, ask.__doc__ = fn.__name__, fn.__doc__
    return ask


def wf_launch(b, cin, cout, n, h, w, groups=1, pair_ok=False):
    """The shared core, part 1: the convolution is a conv3d_wf launch ("wf"; its pair mode too with pair_ok) whatever its input
    looks like -- the rules are asked before the input's form is settled, hence plain=False: the prologue pass's size limit
    counts even where the launch ends up reading a plain tensor.  (conv3_family names these families only for a weight with a
    Winograd form: config.winograd and wino_weight_ok.)"""
    return conv3_family(b, cin, cout, n, h, w, groups, plain=False) in (("wf", "wf_pair") if pair_ok else ("wf",))


def wf_quarter_ok(b, cin, cout, n, h, w, groups=1):
    """The shared core, part 2: a conv3d_wf launch of these extents can write at quarter resolution -- its second output in
    space-to-depth form, LL(y) / 2, the Haar transform of y: it does not split its input channels (a split-K launch's epilogue
    sees partial sums), H is even and W a multiple of 4.  ops.conv3d_wf raises where this is False."""
    return wf_route(b, cin, cout, n, h, w, groups)[1] == 1 and h % 2 == 0 and w % 4 == 0


@_cached
def fold_k1(b, cx, cin, cout, n, h, w, groups=1, math="fp32", segments=1):
    """A 1x1x1 convolution of cx input channels (a ResBlock's res_conv, a down block's Conv_2), whose result is only ever the
    residual of the 3x3x3 convolution cin -> cout, rides in that convolution's epilogue (desc.rc_x / rc_w / rc_cin): fp32, ONE
    input tensor of a multiple of 32 channels (at most 512) at the consumer's plane size, the consumer on conv3d_wf but not in
    its pair mode.  A split-K grid is fine: it adds W1^T x to the partial sums of its first range."""
    if not _config().fuse_res_conv or segments != 1 or math == "bf16" or groups != 1 or cx % 32 or cx > 512:
        return False
    return wf_launch(b, cin, cout, n, h, w) and wf_fold_fits(b, cin, cout, n, h, w, cx)


@_cached
def side_xp(b, seg_c, cout, n, h, w, groups=1, math="fp32"):
    """The 1x1x1 res_conv launch of a ResBlock on the segments seg_c (a tuple of channel counts) also writes conv20's prologue
    output (desc.xp_out / xp_shift / xp_act): fp32 with the conv20 -> conv21 epilogue fusion, a segmented input, conv20 on
    conv3d_wf (pair mode and split-K included: its prologue would otherwise be a pass of its own), res_conv on a form of the
    bandwidth kernel that can (k1_side_xp)."""
    cfg = _config()
    if not (cfg.side_xp and cfg.epilogue_fuse) or len(seg_c) < 2 or math == "bf16" or groups != 1:
        return False
    return wf_launch(b, sum(seg_c), cout, n, h, w, pair_ok=True) and k1_side_xp(b, seg_c, cout, n, h, w)


@_cached
def emit_ll(b, cin, cout, n, h, w, groups=1, math="fp32", switch="emit_ll"):
    """The convolution writes the halved LL band of its output instead of the output (desc.y_ll: a ResBlock's conv21 in front
    of a down block) or, switch="emit_dwt", its whole Haar transform (desc.y_ll + y_hi: Conv_0 of a down block whose high bands
    are kept): fp32, 8 bands, the convolution an unsplit conv3d_wf launch outside the pair mode, the conv20 -> conv21 fusion on
    and the down block's Conv_2 after the LL band (config.conv2_after_ll: nothing else reads the full-resolution tensor)."""
    cfg = _config()
    if not (getattr(cfg, switch) and cfg.conv2_after_ll and cfg.epilogue_fuse) or math == "bf16" or n != 8 or groups != 1:
        return False
    return wf_quarter_ok(b, cin, cout, n, h, w) and wf_launch(b, cin, cout, n, h, w)


@_cached
def s2d_handover(b, c21, c0, n, h, w, groups=1, math="fp32"):
    """The ResBlock in front of a main-branch down block hands its second output over in space-to-depth form (desc.y2_s2d), so
    that Conv_0 + LL runs on conv3d_wf's composed-LL mode ("wfll").  c21 = (cin, cout) of the ResBlock's conv21 (groups: its
    groups), c0 = (cin, cout) of Conv_0, math: "bf16" when the network computes in bf16 at all.  The composed weights exist
    (ll_weight_ok), conv21 is an unsplit conv3d_wf launch -- asked of wf_route, not of conv3_family: pair mode is not excluded
    and the prologue pass's size limit not applied (conv21 reads conv20's plain second output here) --, it produces Conv_0's
    input channels, and the composed convolution's own grid is taken by the kernel (wfll_route)."""
    cfg = _config()
    if not (cfg.epilogue_fuse and cfg.ll_compose and cfg.winograd and cfg.wfll) or math == "bf16":
        return False
    if not (ll_weight_ok(c0[1], c0[0]) and wino_weight_ok(c21[1], c21[0], 3, groups)) or c21[1] != c0[0]:
        return False
    return (wf_route(b, c21[0], c21[1], n, h, w, groups)[0] and wf_quarter_ok(b, c21[0], c21[1], n, h, w, groups) and
            wfll_route(b, c0[0], c0[1], n, h, w))


# ---- the rules composed: one plan per block ----------------------------------------------------------------------------------
# Which of the fusions above a ResBlock and a down block take TOGETHER, and in which order they exclude each other: what
# WavBEST._resblock / _down execute and unet_fusions tabulates.  Functions of the same things as the rules (extents, channel
# counts, ops.config, math strings) plus what the caller knows of the block's neighbours; cached like them.
ResBlockPlan = collections.namedtuple("ResBlockPlan", "fold side_xp pair_fused emit_ll s2d")
DownPlan = collections.namedtuple("DownPlan", "conv0 fold")


def _any16(*maths):
    return "bf16" if "bf16" in maths else "fp32"


@_cached
def resblock_plan(b, seg_c, cout, n, h, w, maths, pre, emit, want_ll, to_conv0):
    """A ResBlock on input segments of seg_c channels (a tuple) -> cout at [b, ., n, h, w].  maths = the math of (conv20, conv21,
    res_conv, the network's compute mode); pre: conv20 reads a second output its producer wrote; emit: the block's consumer wants
    a second output; want_ll: nothing but a down block's Conv_2 path reads the raw output; to_conv0: that down block is the main
    branch's, whose Conv_0 + LL can run composed.  fold: res_conv rides in conv21's epilogue; side_xp: else, without `pre`,
    its launch writes conv20's prologue output; pair_fused: conv20's epilogue applies conv21's prologue (one math); emit_ll:
    conv21 writes LL(y) / 2 instead of y; s2d: its second output is in space-to-depth form."""
    m20, m21, mrc, net = maths
    cin, pair_fused = sum(seg_c), bool(_config().epilogue_fuse) and m20 == m21
    fold = cin != cout and fold_k1(b, seg_c[0], cout, cout, n, h, w, 1, _any16(m21, mrc), len(seg_c))      # (cin != cout: a res_conv exists)
    side = cin != cout and not fold and not pre and side_xp(b, seg_c, cout, n, h, w, 1, _any16(m20, m21, mrc))
    return ResBlockPlan(fold, side, pair_fused,
                        bool(want_ll and emit and pair_fused and emit_ll(b, cout, cout, n, h, w, 1, m21)),
                        bool(to_conv0 and emit and s2d_handover(b, (cout, cout), (cout, cout), n, h, w, 1, _any16(net, m20, m21))))


@_cached
def down_plan(b, ch, n, h, w, maths, main, pre, s2d, fuse):
    """A down block of ch channels on a [b, ch, n, h, w] input.  maths = the math of (Conv_0, Conv_1, Conv_2); main: the main
    branch (high bands dropped); pre: a producer-written fp32 second output exists; s2d: in space-to-depth form
    (resblock_plan's s2d); fuse: the wavelet producers apply their consumer's prologue.  conv0: what the Conv_0 launch is --
    "wfll" / "ll" (composed with the LL band, main branch), "dwt" (writes its own Haar transform, high bands kept) or None (a
    convolution, then a DWT pass); fold: Conv_2, after the LL band, rides in Conv_1's epilogue."""
    m0, m1, m2 = maths
    cfg, conv0 = _config(), None
    if main and pre:
        if s2d:
            conv0 = "wfll"
        elif cfg.ll_compose and ll_weight_ok(ch, ch) and ll_fits(b, ch, ch, n, h, w):
            conv0 = "ll"
    elif fuse and pre and emit_ll(b, ch, ch, n, h, w, 1, m0, "emit_dwt"):
        conv0 = "dwt"
    return DownPlan(conv0, bool(cfg.conv2_after_ll and fold_k1(b, ch, ch, ch, n, h // 2, w // 2, 1, _any16(m1, m2), 1)))


# ---- the finetune graph: one plan per differentiable convolution and per block -------------------------------------------------
# What autograd._conv_forward / _conv_backward / _ConvLL and the block classes' `run` execute and unet_train_launches tabulates;
# functions of extents, channel counts, what the input looks like and ops.config, asked once per convolution per step.
class _GradMath:
    """The arithmetic of a plan's two gradient passes, "fp32" or "bf16" (config.grad_bf16): read off their families -- "bf16" is
    the family of a data gradient on conv3d_bf16 (no weight gradient is routed to a bf16 kernel: rule 6b)."""
    __slots__ = ()
    dgrad_math = property(lambda self: "bf16" if self.dgrad == "bf16" else "fp32")
    wgrad_math = property(lambda self: "bf16" if self.wgrad == "bf16" else "fp32")


class TrainConvPlan(_GradMath, collections.namedtuple("TrainConvPlan", "fwd keep_xp dgrad wgrad bias_in_wgrad")):
    __slots__ = ()


class TrainLLPlan(_GradMath, collections.namedtuple("TrainLLPlan", "fwd dgrad wgrad")):
    __slots__ = ()


TrainDownPlan = collections.namedtuple("TrainDownPlan", "conv0 conv2_after_ll")


def dgrad_bf16_ok(b, cin, cout, n, h, w, groups=1, ksize=3):
    """True when the data gradient of a convolution cin -> cout runs on conv3d_bf16 (config.grad_bf16): a plain 3x3x3 convolution
    of g, cout -> cin channels, on weights from tmdiff_conv3d_pack_weights_bf16_dgrad -- the forward kernel's shape rule with the
    two channel counts swapped (Cin/groups % 32 == 0, Cout/groups % 8 == 0) and its 32-bit plane offsets."""
    return bool(_grad_bf16() and ksize == 3 and groups in (1, 3) and cin % groups == 0 and cout % groups == 0 and
                (cin // groups) % 32 == 0 and (cout // groups) % 8 == 0 and n * h * w < (1 << 31))


def wgrad_family(b, seg_c, cout, n, h, w, groups=1, ksize=3, prologue=False, **fields):
    """"wino" (Winograd F(3,4) along the bands, csrc/wgrad_wino.hip) or "direct": the kernel of the fp32 weight gradient of a
    convolution of the segments seg_c (a tuple of channel counts) -> cout.  prologue: the kernel applies the forward's prologue to
    its input itself (no kept x'); fields: further descriptor fields the library's query reads."""
    if not (_config().wgrad_wino and ksize == 3):
        return "direct"
    if prologue:
        fields["in_act"] = 1
    return "wino" if supported("tmdiff_conv3d_wgrad_wino_supported", b, tuple(seg_c), cout, n, h, w, groups, **fields) else "direct"


@_cached
def train_conv_plan(b, seg_c, cout, n, h, w, groups=1, ksize=3, prologue=False, masked=False, dropout=False, need_w=True):
    """One differentiable convolution of the segments seg_c -> cout at [b, ., n, h, w].  prologue: SiLU / shift / scale on the
    input; masked / dropout: as for conv3_family; need_w: the weight wants a gradient.  fwd: the forward family ("k1": a 1x1x1
    convolution, the bandwidth kernel); keep_xp: a 3x3x3 convolution with dropout runs as prologue pass + kernel anyway, so the
    pass writes x' into a tensor of its own and the weight gradient reads that (staged_weight_ok: the direct kernel that has
    such a pass); dgrad: the family of the data gradient, a plain-input convolution cout -> cin; wgrad: wgrad_family on what
    the weight gradient reads; bias_in_wgrad: the bias gradient rides in the weight-gradient kernel (config.wgrad_bias: the
    direct kernel accumulates it; config.wgrad_wino_bias: the Winograd kernel's g pass sums it on the side).  config.grad_bf16:
    dgrad is "bf16" where dgrad_bf16_ok takes the shape (plan.dgrad_math / plan.wgrad_math name the arithmetic of the two gradient
    passes); fwd, keep_xp and wgrad never change."""
    cfg, cin = _config(), sum(seg_c)
    pro = bool(prologue or masked or dropout)
    keep_xp = bool(ksize == 3 and (masked or dropout) and need_w and staged_weight_ok(cout, cin, groups))
    if ksize == 3:
        fwd = conv3_family(b, cin, cout, n, h, w, groups, len(seg_c) == 1 and not pro, masked, dropout, keep_xp)
        dgrad = "bf16" if dgrad_bf16_ok(b, cin, cout, n, h, w, groups) else conv3_family(b, cout, cin, n, h, w, groups)
    else:
        fwd = dgrad = "k1"
    wgrad = wgrad_family(b, (cin,) if keep_xp else seg_c, cout, n, h, w, groups, ksize, pro and not keep_xp)
    return TrainConvPlan(fwd, keep_xp, dgrad, wgrad, bool(cfg.wgrad_bias or (cfg.wgrad_wino_bias and wgrad == "wino")))


@_cached
def train_ll_plan(b, cin, cout, n, h, w):
    """Conv_0 + halved LL band as one differentiable node (autograd._ConvLL) on a [b, cin, n, h, w] input.  fwd: "wfll" (x' once
    more in space-to-depth form for conv3d_wf's composed-LL mode) or "ll"; dgrad / wgrad: the families of the full-resolution
    data gradient (the node offers no transform-pass weights: a fallback family's shape stays direct) and of the weight
    gradient on the kept x'."""
    fwd = "wfll" if _config().train_ll_wino and wfll_route(b, cin, cout, n, h, w) else "ll"
    dgrad = "bf16" if dgrad_bf16_ok(b, cin, cout, n, h, w) else conv3_family(b, cout, cin, n, h, w)
    if dgrad in FALLBACK_FAMILIES:
        dgrad = direct_family(cout, cin, extents=(b, n, h, w))
    return TrainLLPlan(fwd, dgrad, wgrad_family(b, (cin,), cout, n, h, w))


@_cached
def train_down_plan(b, ch, n, h, w, main):
    """A down block of ch channels on a [b, ch, n, h, w] input in the finetune graph; main: the high bands are dropped.  conv0:
    what Conv_0 is -- "wfll" / "ll" (train_ll_plan's node; main branch, composable and within conv3d_ll's size limit whichever
    of the two runs) or None (a convolution, then a DWT); conv2_after_ll: Conv_2 runs on the LL band of the input."""
    conv0 = None
    if main and ll_composable(ch, ch, h, w) and ll_fits(b, ch, ch, n, h, w):
        conv0 = train_ll_plan(b, ch, ch, n, h, w).fwd
    return TrainDownPlan(conv0, bool(_config().conv2_after_ll))


def train_resblock_plan(seg_c, cout):
    """Which autograd node(s) a ResBlock of the segments seg_c -> cout is: "rc" (one node, res_conv inside: conv20's input
    gradients are added to res_conv's), "id" (one node, the input is the residual: one tensor) or "separate" (a node per
    convolution; config.train_fused_resblock off, or a segmented input without a res_conv)."""
    if _config().train_fused_resblock:
        if sum(seg_c) != cout:
            return "rc"
        if len(seg_c) == 1:
            return "id"
    return "separate"


# ---- the network's 3x3x3 convolutions ------------------------------------------------------------------------------------
Layer = collections.namedtuple("Layer", "name cin cout groups h w plain kind")      # kind: "conv" | "conv0_ll"


def unet_conv3_layers(channels, h, w):
    """The 51 3x3x3 convolutions of one WavBEST inference forward at level-0 planes h x w, in the fused (default) graph:
    every convolution reads its producer's second output (plain = ONE plain tensor) except the four three-segment conv20s of
    the up path (prologue pass = concatenation) and convH_0, whose three segments are its three groups' inputs (read in place
    by conv3d_wf, no pass)."""
    c = list(channels)
    lv = [(h >> k, w >> k) for k in range(4)]
    out = []
    add = lambda name, ci, co, k, g=1, plain=True, kind="conv": out.append(Layer(name, ci, co, g, lv[k][0], lv[k][1], plain, kind))
    for stem in ("conv1", "conv2"):
        add(stem + ".conv21", c[0], c[0], 0)
    for suffix, main in (("_1", False), ("", True)):
        for k in range(3):
            blk = f"down{k + 1}{suffix}"
            add(blk + ".conv20.conv20", c[k], c[k + 1], k)
            add(blk + ".conv20.conv21", c[k + 1], c[k + 1], k)
            add(blk + ".down.Conv_0", c[k + 1], c[k + 1], k, kind="conv0_ll" if main else "conv")
            add(blk + ".down.Conv_1", c[k + 1], c[k + 1], k + 1)
    add("middle1.conv20", c[3], c[3], 3)
    add("middle1.conv21", c[3], c[3], 3)
    for k, upn in ((3, "up1"), (2, "up2"), (1, "up3")):
        add(upn + ".conv20.conv20", 3 * c[k], c[k - 1], k, plain=False)
        add(upn + ".conv20.conv21", c[k - 1], c[k - 1], k)
        add(upn + ".up1.Conv_0", c[k - 1], c[k - 1], k)
        add(upn + ".up1.convH_0.0", 3 * c[k], 3 * c[k - 1], k, g=3, plain=False)      # (three tensors: its three groups' inputs)
        add(upn + ".up1.Conv_1", c[k - 1], c[k - 1], k - 1)
    add("final.conv20.conv20", 3 * c[0], c[0], 0, plain=False)
    add("final.conv20.conv21", c[0], c[0], 0)
    for k in (1, 2, 3):
        add(f"final.conv2{k}.conv20", c[0], c[0], 0)
        add(f"final.conv2{k}.conv21", c[0], c[0], 0)
    return out


def unet_table(channels, b, n, h, w, math="fp32"):
    """[(Layer, family)] of one inference forward of a batch of b tiles with n bands."""
    rows = []
    for L in unet_conv3_layers(channels, h, w):
        if L.kind == "conv0_ll" and math == "fp32":
            # (the plans of the fused fp32 graph; the ResBlock's s2d does not depend on its input channels)
            s2d = resblock_plan(b, (L.cin,), L.cin, n, L.h, L.w, ("fp32",) * 4, True, True, True, True).s2d
            fam = down_plan(b, L.cout, n, L.h, L.w, ("fp32",) * 3, True, True, s2d, True).conv0
            if fam is not None:
                rows.append((L, fam))
                continue
        bf = math == "bf16" and L.cin // L.groups % 8 == 0 and L.cout // L.groups % 32 == 0 and (L.plain or L.cin // 3 % 8 == 0)
        rows.append((L, conv3_family(b, L.cin, L.cout, n, L.h, L.w, L.groups, plain=L.plain, math="bf16" if bf else "fp32")))
    return rows


# ---- the network's fusions ---------------------------------------------------------------------------------------------------
Fusion = collections.namedtuple("Fusion", "block kind taken k1 passes")
# kind: "stem" | "resblock" | "down" | "up"; taken: the fusions of this block, of "fold" (res_conv / Conv_2 folded), "side_xp",
# "emit_ll", "s2d" (ResBlocks) and "wfll" | "ll" | "dwt" (what a down block's Conv_0 launch is, beyond a convolution);
# k1: the 1x1x1 launches the block still makes; passes: the prologue (bf16: pack) passes in front of its 3x3x3 convolutions


def unet_fusions(channels, b, n, h, w, math="fp32", fuse=None):
    """[Fusion] of one inference forward (condition branch, then main branch) of a batch of b tiles with n bands: which
    fusions each ResBlock and each wavelet block takes -- the block walk of WavBEST._condition / _forward_infer over the plans
    WavBEST._resblock / _down execute (resblock_plan, down_plan), on extents alone.  math: the network's compute mode; fuse: what
    WavBEST._producer_fuse returns (the default: what it returns in fp32).  tests/test_host_logic.py holds the plans WavBEST
    asks for, from its own module tree, to these rows."""
    from . import ops
    cfg = _config()
    fuse_c, fuse_p = (cfg.producer_fuse and cfg.epilogue_fuse,) * 2 if fuse is None else fuse
    c = list(channels)
    lv = [(h >> k, w >> k) for k in range(4)]
    rows = []

    def m16(cout, cin, ksize=3):          # the math of one convolution (WavBEST._prepare's rule, its segment check included)
        seg = [cin // 3] if cin % 3 == 0 else None
        return "bf16" if math == "bf16" and ops.bf16_conv_supported(cout, cin, ksize, 1, seg) else "fp32"

    def passes(convs):                    # convs: (cin, cout, level, plain) -- a pass in front of every input that is not plain
        return sum(1 for ci, co, k, plain in convs if not plain and conv3_family(
            b, ci, co, n, *lv[k], plain=False, math=m16(co, ci)) in ("wf", "wf_pair", "staged", "bf16"))

    def resblock(name, seg_c, cout, k, pre, emit, want_ll=False, to_conv0=False):
        cin = sum(seg_c)
        p = resblock_plan(b, tuple(seg_c), cout, n, *lv[k], (m16(cout, cin), m16(cout, cout), m16(cout, cin, 1), math),
                          bool(pre), bool(emit), want_ll, to_conv0)
        rows.append(Fusion(name, "resblock", tuple(f for f in ("fold", "side_xp", "emit_ll", "s2d") if getattr(p, f)),
                           int(cin != cout and not p.fold),
                           passes([(cin, cout, k, (pre and p.pair_fused) or p.side_xp), (cout, cout, k, p.pair_fused)])))
        return p.s2d

    def down(name, k, main, pre, s2d):
        ch = c[k + 1]
        p = down_plan(b, ch, n, *lv[k], (m16(ch, ch), m16(ch, ch), m16(ch, ch, 1)), main, bool(pre and math == "fp32"), s2d, bool(fuse_p))
        convs = [(ch, ch, k + 1, bool(fuse_p))] + ([(ch, ch, k, pre)] if p.conv0 in (None, "dwt") else [])
        rows.append(Fusion(name, "down", tuple(t for t in (p.conv0, "fold" if p.fold else None) if t), int(not p.fold), passes(convs)))

    def stem(name):                       # (the stem writes conv21's modulated input where the producers fuse)
        rows.append(Fusion(name, "stem", (), 0, passes([(c[0], c[0], 0, bool(fuse_p))])))

    for branch in ("_1", ""):
        stem("conv2" if not branch else "conv1")
        for k in range(3):
            blk = f"down{k + 1}{branch}"
            s2d = resblock(blk + ".conv20", [c[k]], c[k + 1], k, fuse_c, fuse_c, want_ll=True, to_conv0=not branch)
            down(blk + ".down", k, not branch, fuse_c, s2d)
    resblock("middle1", [c[3]], c[3], 3, fuse_c, False)
    for k, upn in ((3, "up1"), (2, "up2"), (1, "up3")):
        resblock(upn + ".conv20", [c[k]] * 3, c[k - 1], k, False, fuse_c)
        rows.append(Fusion(upn + ".up1", "up", (), 1, passes([(c[k - 1], c[k - 1], k, fuse_c), (c[k - 1], c[k - 1], k - 1, bool(fuse_p))])))
    resblock("final.conv20", [c[0]] * 3, c[0], 0, False, fuse_c)
    for k in (1, 2, 3):
        resblock(f"final.conv2{k}", [c[0]], c[0], 0, fuse_c, fuse_c and k < 3)
    return rows


# ---- the finetune step's launches --------------------------------------------------------------------------------------------
TrainRow = collections.namedtuple("TrainRow", "name cin cout groups ksize h w fwd keep_xp dgrad wgrad bias_in_wgrad")
TrainLaunches = collections.namedtuple("TrainLaunches", "counts convs blocks")
# counts: {key of ops.COUNTS: launches}; convs: [TrainRow], the plan of every convolution; blocks: [(name, plan)] of every
# ResBlock (train_resblock_plan) and down block (train_down_plan)
LAUNCH_KEY = {"wf": "conv3d_wf_fwd", "wf_pair": "conv3d_wf_fwd", "wfll": "conv3d_wfll_fwd", "ll": "conv3d_ll_fwd",
              "staged": "conv3d_fwd_staged", "fused": "conv3d_fwd", "k1": "conv3d_fwd_k1", "wino4": "conv3d_wino4_fwd",
              "wino2": "conv3d_wino2_fwd", "wino": "conv3d_wgrad_wino", "direct": "conv3d_wgrad", "bf16": "conv3d_fwd_bf16"}


def unet_train_launches(channels, b, n, h, w, dropout=False):
    """TrainLaunches of one WavBEST.forward_train plus its backward on a batch of b tiles with n bands, every parameter wanting
    a gradient: the block walk of forward_train over the plans the block classes and tmdiff_amd.autograd execute, on extents
    alone.  dropout: the network is in training mode (in-kernel dropout in front of every ResBlock convolution and every
    Conv_1).  Each convolution is three counted launches: forward, data gradient, weight gradient.  tests/test_host_logic.py
    holds the plans a WavBEST asks for, from its own module tree, to these rows; tests/test_gpu_configs.py ops.COUNTS of a
    step to the counts."""
    c = list(channels)
    lv = [(h >> k, w >> k) for k in range(4)]
    counts, convs, blocks = collections.Counter(), [], []

    def add(name, cin, cout, k, groups, ksize, fwd, keep_xp, dgrad, wgrad, bias):
        convs.append(TrainRow(name, cin, cout, groups, ksize, *lv[k], fwd, keep_xp, dgrad, wgrad, bias))
        counts.update(LAUNCH_KEY[f] for f in (fwd, dgrad, wgrad))

    def conv(name, seg_c, cout, k, ksize=3, groups=1, prologue=False, drop=False):
        p = train_conv_plan(b, tuple(seg_c), cout, n, *lv[k], groups, ksize, prologue, False, bool(drop and dropout), True)
        add(name, sum(seg_c), cout, k, groups, ksize, *p)

    def resblock(name, seg_c, cout, k):
        blocks.append((name, train_resblock_plan(tuple(seg_c), cout)))
        conv(name + ".conv20", seg_c, cout, k, prologue=True, drop=True)
        if sum(seg_c) != cout:
            conv(name + ".res_conv", seg_c, cout, k, ksize=1)
        conv(name + ".conv21", [cout], cout, k, prologue=True, drop=True)

    def down(name, ch, k, main):
        p = train_down_plan(b, ch, n, *lv[k], main)
        blocks.append((name, p))
        if p.conv0:         # (autograd._ConvLL: x' always kept, the bias gradient a pass of its own)
            add(name + ".Conv_0", ch, ch, k, 1, 3, p.conv0, True, *train_ll_plan(b, ch, ch, n, *lv[k])[1:], False)
        else:
            conv(name + ".Conv_0", [ch], ch, k, prologue=True)
        conv(name + ".Conv_2", [ch], ch, k + 1 if p.conv2_after_ll else k, ksize=1)
        conv(name + ".Conv_1", [ch], ch, k + 1, prologue=True, drop=True)

    def up(name, k):
        ch = c[k - 1]
        conv(name + ".Conv_0", [ch], ch, k, prologue=True)
        conv(name + ".Conv_2", [ch], ch, k, ksize=1)
        conv(name + ".convH_0.0", [c[k]] * 3, 3 * ch, k, groups=3)
        conv(name + ".Conv_1", [ch], ch, k - 1, prologue=True, drop=True)

    for branch in ("_1", ""):
        conv(("conv1" if branch else "conv2") + ".conv21", [c[0]], c[0], 0, prologue=True)
        for k in range(3):
            blk = f"down{k + 1}{branch}"
            resblock(blk + ".conv20", [c[k]], c[k + 1], k)
            down(blk + ".down", c[k + 1], k, not branch)
    resblock("middle1", [c[3]], c[3], 3)
    for k, upn in ((3, "up1"), (2, "up2"), (1, "up3")):
        resblock(upn + ".conv20", [c[k]] * 3, c[k - 1], k)
        up(upn + ".up1", k)
    resblock("final.conv20", [c[0]] * 3, c[0], 0)
    for k in (1, 2, 3):
        resblock(f"final.conv2{k}", [c[0]], c[0], 0)
    return TrainLaunches(dict(counts), convs, blocks)


# BASELINE.json configs as (label, channels, batch per GPU, bands, plane) -- B in {1, 8, 32}, N in {4, 8}, 64^2 / 256^2
FULL, WIDE = [32, 64, 128, 256], [64, 128, 256, 512]
BASELINE_CASES = (
    ("configs[0] single tile, T=50", FULL, 1, 8, 64, "fp32"),
    ("configs[1] batch 32 (benchmark)", FULL, 32, 8, 64, "fp32"),
    ("configs[2] WV-3 256x256, ch 64-512, fp32", WIDE, 1, 8, 256, "fp32"),
    ("configs[2] WV-3 256x256, ch 64-512, bf16", WIDE, 1, 8, 256, "bf16"),
    ("configs[3] finetune local batch 8 (the inference graph at that batch)", FULL, 8, 8, 64, "fp32"),
    ("configs[4] GF-2 tiles, batch 32", FULL, 32, 4, 64, "fp32"),
    ("configs[4] WV-3 tiles, batch 32", FULL, 32, 8, 64, "fp32"),
    ("configs[4] GF-2 tiles, batch 8", FULL, 8, 4, 64, "fp32"),
    ("configs[4] GF-2 256x256 tiles, batch 1", FULL, 1, 4, 256, "fp32"),
)
# ... and the widths the reference's constructor defaults to (WavBEST(channels=None) -> [16, 32, 64, 128],
# Hyper_unet_general.py:524-527) / the reference-generated TINY fixtures use: output channels that are not multiples of 32 run on
# the general-shape direct kernel ("fused"), which no BASELINE width needs
OTHER_CASES = (
    ("reference default widths, batch 32", [16, 32, 64, 128], 32, 8, 64, "fp32"),
    ("TINY fixture widths, batch 2", [4, 8, 16, 32], 2, 8, 16, "fp32"),
)
# The finetune step itself (unet_train_launches; tools/routing_table.py --train) as (label, channels, batch, bands, plane, switches):
# configs[3], and the small networks whose step tests/test_gpu_configs.py counts launch by launch
SMALL = [16, 32, 64, 64]        # (16 channels: the general-shape direct kernel; planes down to 8x8 / 16x16: no fallback family)
TRAIN_CASES = (
    ("configs[3] finetune local batch 8", FULL, 8, 8, 64, {}),
    ("reference default widths, batch 8", [16, 32, 64, 128], 8, 8, 64, {}),
    ("small network, 8 bands", SMALL, 2, 8, 64, {"wino_min_blocks": 1}),
    ("small network, 4 bands", SMALL, 2, 4, 128, {"wino_min_blocks": 1}),
    ("small network, 8 bands, Conv_0 + LL on conv3d_ll", SMALL, 2, 8, 64, {"wino_min_blocks": 1, "train_ll_wino": False}),
    ("TINY fixture widths, batch 2", [4, 8, 16, 32], 2, 8, 16, {}),
)
