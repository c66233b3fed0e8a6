"""Thin tensor-level wrappers over the C ABI (include/tmdiff_hip.h).

PyTorch is plumbing here: it owns device memory and the current HIP stream; every FLOP of
these ops runs in libtmdiff_hip.so.  All wrappers require CUDA(HIP) fp32 contiguous
tensors and raise otherwise -- there is no eager fallback.
"""
import collections
import ctypes as C
import math
import os

import numpy as np
import torch

from . import _lib, routing
from ._lib import Conv3dDesc, check, lib



class KernelConfig:
    """Every behaviour switch of the Python side, in one place.  Each field is read ONCE from its environment variable when
    the package is imported and is a plain attribute afterwards: code reads ``ops.config.<field>`` at call time, tests and
    experiments change it with ``with ops.config.override(field=value): ...`` (no re-import, no environment juggling).
    Defaults are the production path; every other value exists for A/B measurements and for the parity tests of the
    alternative paths (tests/test_gpu_configs.py runs the finetune step with each result-changing default switched off).

    field              env var                  default  meaning
    -----------------  -----------------------  -------  ---------------------------------------------------------------------
    winograd           TMDIFF_WINOGRAD          True     3x3x3 convolutions on the Winograd-along-the-bands kernels (conv3d_wf,
                                                         fallback.conv3d_wino); False = direct kernels everywhere
    wf                 TMDIFF_WF                True     ... with the input transform inside the kernel (conv3d_wf) where it applies
    wf_pair            TMDIFF_WF_PAIR           True     8 bands x 8 columns: two images per 8x16 tile (pair mode); False = fallback
    wf_splitk          TMDIFF_WF_SPLITK         True     small conv3d_wf grids split their input channels (+ reduction kernel)
    wf_min_fill        TMDIFF_WF_MIN_FILL       0.7      planes that fill less of conv3d_wf's tiles go to the fallback
    wino_min_blocks    TMDIFF_WINO_MIN_BLOCKS   256      Winograd grids below this many workgroups go to the direct kernels
                                                         (1 = force the production family onto small test batches)
    wino2d             TMDIFF_WINO2D            True     deep layers (routing.wino2d_ok) on conv3d_w2: Winograd along the width as well,
                                                         as transform passes + one GEMM per plane; False = conv3d_wf
    wino2d_epilogue    TMDIFF_WINO2D_EPILOGUE   True     ... also the launches with a folded 1x1x1 / LL / Haar / space-to-depth epilogue
    ll_compose         TMDIFF_LL_COMPOSE        True     main-branch Conv_0 + halved LL band as one composed convolution
    wfll               TMDIFF_WFLL              True     ... with Winograd on top (conv3d_wf's composed-LL mode) in inference
    train_ll_wino      TMDIFF_TRAIN_LL_WINO     True     ... and in the finetune forward; False = conv3d_ll there
    conv2_after_ll     TMDIFF_CONV2_AFTER_LL    True     down blocks: the 1x1x1 Conv_2 after the LL band it commutes with
    epilogue_fuse      TMDIFF_EPILOGUE_FUSE     True     conv20 -> conv21: the producer's epilogue writes the consumer's prologue
    producer_fuse      TMDIFF_PRODUCER_FUSE     True     ... likewise for DWT / IDWT / stem producers
    fp32_staged        TMDIFF_FP32_STAGED       "auto"   direct fp32 kernels: "0" fused only, "1" staged wherever supported
    bf16_pack          TMDIFF_BF16_PACK         "auto"   bf16 mode: "0" fused kernel, "1"/"auto" packed input + DMA kernel
    wgrad_wino         TMDIFF_WGRAD_WINO        True     3x3x3 weight gradients in the Winograd domain (F(3,4)); False = direct
    wgrad_wino_bias    TMDIFF_WGRAD_WINO_BIAS   True     ... whose g pass sums the bias gradient on the side
    wgrad_bias         TMDIFF_WGRAD_BIAS        False    direct weight gradient accumulates the bias gradient in-kernel
    wino_multipack     TMDIFF_WINO_MULTIPACK    True     finetune step: all Winograd weight forms re-packed by one launch
    fuse_res_conv      TMDIFF_FUSE_RES_CONV     True     inference: a ResBlock's 1x1x1 res_conv folded into conv21's epilogue (conv3d_wf)
    emit_ll            TMDIFF_EMIT_LL           True     inference: the ResBlock in front of a down block writes LL(y) / 2 instead of y
    emit_dwt           TMDIFF_EMIT_DWT          True     inference: Conv_0 of a down block whose high bands are kept writes the Haar
                                                         transform of its output instead of the output (no DWT pass)
    side_xp            TMDIFF_SIDE_XP           True     inference: a ResBlock's res_conv launch (segmented input) also writes conv20's
                                                         prologue output (no prologue pass in front of conv20)
    train_fused_resblock TMDIFF_TRAIN_FUSED_RESBLOCK True finetune: a ResBlock with a res_conv is ONE autograd node (conv20's input gradients
                                                         are added to res_conv's by the prologue-backward kernel, not by a sum launch)
    train_graph        TMDIFF_TRAIN_GRAPH       False    (model.DDPM) capture the finetune step into a HIP graph
    train_two_streams  TMDIFF_TRAIN_STREAMS     True     forward_train runs the condition branch on a second stream beside the
                                                         main branch's down path (at a local batch of 8 most launches fill half
                                                         of the CU slots); autograd then runs their backward passes side by side too
    grad_bf16          TMDIFF_GRAD_BF16         False    finetune: the data gradients of the eligible 3x3x3 convolutions from bf16-rounded
                                                         operands with fp32 accumulation (routing.train_conv_plan rule 6b; the forward,
                                                         the loss, the weight gradients, parameters and the optimizer stay fp32)
    sample_graph       TMDIFF_SAMPLE_GRAPH      False    (GeneralDiffusion) p_sample_loop / super_resolution / sample /
                                                         sample_by_dpmsolver capture their steps into HIP graphs and replay them
                                                         (tmdiff_amd.sample_graph; per object: GeneralDiffusion.sample_graphs)

    Library-side experiment variables (read by libtmdiff_hip.so itself, C getenv): TMDIFF_SPLITK, TMDIFF_SPLITK_LONG,
    TMDIFF_WF_STAGGER, TMDIFF_WINO_STAGGER, TMDIFF_WINO_F4, TMDIFF_EPILOGUE_VEC, TMDIFF_SMALLGRID, TMDIFF_WW_PHASES,
    TMDIFF_ATTN_SIMPLE, TMDIFF_CONV1_VEC, TMDIFF_CONV1_DWORD -- timing experiments only; TMDIFF_HIP_LIB selects a diagnostic
    build of the library (_lib.py)."""

    _FLAG = lambda default: (lambda v: (v != "0") if default else (v == "1"))
    _FIELDS = {
        "winograd": ("TMDIFF_WINOGRAD", _FLAG(True), True), "wf": ("TMDIFF_WF", _FLAG(True), True),
        "wf_pair": ("TMDIFF_WF_PAIR", _FLAG(True), True), "wf_splitk": ("TMDIFF_WF_SPLITK", _FLAG(True), True),
        "wf_min_fill": ("TMDIFF_WF_MIN_FILL", float, 0.7), "wino_min_blocks": ("TMDIFF_WINO_MIN_BLOCKS", int, 256),
        "ll_compose": ("TMDIFF_LL_COMPOSE", _FLAG(True), True), "wfll": ("TMDIFF_WFLL", _FLAG(True), True),
        "train_ll_wino": ("TMDIFF_TRAIN_LL_WINO", _FLAG(True), True),
        "conv2_after_ll": ("TMDIFF_CONV2_AFTER_LL", _FLAG(True), True),
        "epilogue_fuse": ("TMDIFF_EPILOGUE_FUSE", _FLAG(True), True), "producer_fuse": ("TMDIFF_PRODUCER_FUSE", _FLAG(True), True),
        "fp32_staged": ("TMDIFF_FP32_STAGED", str, "auto"), "bf16_pack": ("TMDIFF_BF16_PACK", str, "auto"),
        "wgrad_wino": ("TMDIFF_WGRAD_WINO", _FLAG(True), True), "wgrad_wino_bias": ("TMDIFF_WGRAD_WINO_BIAS", _FLAG(True), True),
        "wgrad_bias": ("TMDIFF_WGRAD_BIAS", _FLAG(False), False), "wino_multipack": ("TMDIFF_WINO_MULTIPACK", _FLAG(True), True),
        "fuse_res_conv": ("TMDIFF_FUSE_RES_CONV", _FLAG(True), True), "emit_ll": ("TMDIFF_EMIT_LL", _FLAG(True), True),
        "emit_dwt": ("TMDIFF_EMIT_DWT", _FLAG(True), True), "side_xp": ("TMDIFF_SIDE_XP", _FLAG(True), True),
        "train_fused_resblock": ("TMDIFF_TRAIN_FUSED_RESBLOCK", _FLAG(True), True),
        "train_graph": ("TMDIFF_TRAIN_GRAPH", _FLAG(False), False),
        "train_two_streams": ("TMDIFF_TRAIN_STREAMS", _FLAG(True), True),
        "sample_graph": ("TMDIFF_SAMPLE_GRAPH", _FLAG(False), False),
        "grad_bf16": ("TMDIFF_GRAD_BF16", _FLAG(False), False),
        "wino2d": ("TMDIFF_WINO2D", _FLAG(True), True),
        "wino2d_epilogue": ("TMDIFF_WINO2D_EPILOGUE", _FLAG(True), True),
    }

    def __init__(self, env=None):
        env = os.environ if env is None else env
        for name, (var, parse, default) in self._FIELDS.items():
            object.__setattr__(self, name, parse(env[var]) if var in env else default)

    def __setattr__(self, name, value):
        if name not in self._FIELDS:
            raise AttributeError(f"ops.config has no switch {name!r}")
        object.__setattr__(self, name, value)

    def key(self):
        """The current values as a tuple (cache keys of routing decisions)."""
        return tuple(getattr(self, n) for n in self._FIELDS)

    def as_dict(self):
        return {n: getattr(self, n) for n in self._FIELDS}

    def override(self, **values):
        """Context manager: the given switches take the given values inside the block."""
        import contextlib

        @contextlib.contextmanager
        def ctx():
            old = {k: getattr(self, k) for k in values}
            try:
                for k, v in values.items():
                    setattr(self, k, v)
                yield self
            finally:
                for k, v in old.items():
                    setattr(self, k, v)
        return ctx()


config = KernelConfig()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream_ptr():
    """hipStream_t of torch's current stream on the current device (the raw getter: torch.cuda.current_stream() builds
    a Stream object per call, ~15 us -- 4 ms per training step at ~300 kernel launches)."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def _chk(t, name):
    if t is None:
        return None
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise ValueError(f"{name}: need a contiguous float32 tensor on the GPU, got {t.dtype} {t.device} "
                         f"contiguous={t.is_contiguous()}")
    return t.data_ptr()


def pack_conv_weight(w, groups=1, mode=0):
    """[Cout, Cin/g, k,k,k] -> packed [g][ci][tap][co] (mode 0) or the data-gradient packing (mode 1)."""
    cout, cin_g, k = w.shape[0], w.shape[1], w.shape[2]
    out = torch.empty(w.numel(), device=w.device, dtype=torch.float32)
    check(lib.tmdiff_conv3d_pack_weights(_chk(w.detach(), "w"), out.data_ptr(), cout, cin_g * groups, k, groups, mode,
                                         stream_ptr()), "conv3d_pack_weights")
    return out


class PackedWeights:
    """Forward and data-gradient packings of a list of convolution weights, refreshed by ONE launch
    (tmdiff_conv3d_pack_weights_multi).  ``refresh()`` re-packs when any weight changed (``_version``); ``lookup(w)``
    returns (packed_fwd, packed_dgrad) for a weight whose current version is packed, else None."""

    def __init__(self, convs):
        """convs: list of (weight [Cout, Cin/g, k, k, k] on the GPU, groups)"""
        self.convs = [(w, g) for w, g in convs]
        dev = self.convs[0][0].device
        self.fwd = [torch.empty(w.numel(), device=dev, dtype=torch.float32) for w, _ in self.convs]
        self.dgrad = [torch.empty(w.numel(), device=dev, dtype=torch.float32) for w, _ in self.convs]
        self._table_key, self.versions = None, None
        self._index = {}

    def _build_tables(self):
        ent = bytearray()
        ct, ci = [], []
        import struct
        for k, ((w, g), f, d) in enumerate(zip(self.convs, self.fwd, self.dgrad)):
            _chk(w.detach(), "weight")
            ent += struct.pack("<QQQiiii", w.data_ptr(), f.data_ptr(), d.data_ptr(), w.shape[0], w.shape[1] * g, w.shape[2], g)
            if w.shape[2] not in (1, 3):
                raise ValueError("PackedWeights: kernel size 1 or 3")
            na = C.c_int32(0)
            nck = lib.tmdiff_conv3d_pack_weights_multi_chunks(w.shape[0], w.shape[1] * g, g, C.byref(na))
            ct += [k] * nck
            ci += list(range(na.value)) + [(1 << 30) | t for t in range(nck - na.value)]
        dev = self.convs[0][0].device
        self.entries = torch.frombuffer(bytearray(ent), dtype=torch.uint8).clone().to(dev)
        self.chunk_tensor = torch.tensor(ct, dtype=torch.int32).to(dev)
        self.chunk_index = torch.tensor(ci, dtype=torch.int32).to(dev)
        self.n_chunks = len(ct)
        self._table_key = tuple(w.data_ptr() for w, _ in self.convs)
        self._index = {w.data_ptr(): k for k, (w, _) in enumerate(self.convs)}

    def refresh(self):
        ptrs = tuple(w.data_ptr() for w, _ in self.convs)
        if ptrs != self._table_key:
            self._build_tables()
            self.versions = None
        vers = tuple(w._version for w, _ in self.convs)
        if vers != self.versions:
            check(lib.tmdiff_conv3d_pack_weights_multi(self.entries.data_ptr(), self.chunk_tensor.data_ptr(),
                                                       self.chunk_index.data_ptr(), self.n_chunks, stream_ptr()),
                  "conv3d_pack_weights_multi")
            self.versions = vers
        return self

    def lookup(self, w):
        k = self._index.get(w.data_ptr())
        if k is None or self.versions is None or self.versions[k] != w._version or self.convs[k][0].shape != w.shape:
            return None
        return self.fwd[k], self.dgrad[k]


class WinoPackedWeights:
    """The Winograd (conv3d_wf) packings -- forward (mode 2) / data-gradient (mode 3) form, F(4,3), natural column order -- of the
    3x3x3 weights a finetune step ACTUALLY runs through that kernel, refreshed by ONE launch per step
    (tmdiff_conv3d_wino_pack_weights_multi).  Which (weight, form) pairs those are depends on the tensor sizes (the 8x8 level
    and small grids take other kernels, and the deep levels hold most of the parameters), so the set is learnt: ``get``
    packs a pair it does not hold by itself and registers it; ``refresh`` (once per step, before the forward) re-packs the
    registered pairs whose weight changed.

    ``owner`` = the weights of the network this pack belongs to (WavBEST.forward_train passes its convolution weights): a weight
    that is not among them -- another module's, a test's -- is packed on the spot by ``get`` and NOT registered, so a foreign
    call can neither keep tensors alive here nor dirty the table.  The device table holds raw addresses; it is
    rebuilt whenever the (weight address, packed address) pairs it was built from are not the live ones any more -- a
    ``copy.deepcopy`` of a network that had already trained used to launch the multi-pack on the SOURCE network's memory."""

    def __init__(self, owner=None):
        self.items = {}               # (weight address, mode) -> [weight, groups, packed tensor, packed version]
        self.owner = None if owner is None else list(owner)
        self._owner_ptrs = None
        self._table_key = None
        self.n_chunks = 0

    def _live_key(self):
        return tuple((it[0].data_ptr(), it[2].data_ptr(), mode) for (_, mode), it in self.items.items())

    def _build_tables(self):
        import struct
        chunk = lib.tmdiff_conv3d_wino_pack_weights_multi_chunk()
        ent, ct, ci = bytearray(), [], []
        for n, ((_, mode), (w, g, out, _)) in enumerate(self.items.items()):
            ent += struct.pack("<QQiiiiii", w.data_ptr(), out.data_ptr(), w.shape[0], w.shape[1] * g, g, mode, 6, 0)
            nck = (w.numel() // 27 + chunk - 1) // chunk          # (chunks of weight rows: 27 taps each)
            ct += [n] * nck
            ci += list(range(nck))
        dev = next(iter(self.items.values()))[0].device
        self.entries = torch.frombuffer(bytearray(ent), dtype=torch.uint8).clone().to(dev)
        self.chunk_tensor = torch.tensor(ct, dtype=torch.int32).to(dev)
        self.chunk_index = torch.tensor(ci, dtype=torch.int32).to(dev)
        self.n_chunks = len(ct)
        self._table_key = self._live_key()

    def refresh(self):
        if self.owner is not None:
            self._owner_ptrs = {w.data_ptr() for w in self.owner}
        # a registered weight whose storage moved (module.to(), parameters re-created) is forgotten and re-learnt
        self.items = {k: it for k, it in self.items.items()
                      if it[0].data_ptr() == k[0] and it[0].device == it[2].device}
        if not self.items:
            self._table_key = None
            return self
        if self._table_key != self._live_key():      # new pairs since the table was built
            self._build_tables()
            for it in self.items.values():
                it[3] = None
        if any(it[3] != it[0]._version for it in self.items.values()):
            check(lib.tmdiff_conv3d_wino_pack_weights_multi(self.entries.data_ptr(), self.chunk_tensor.data_ptr(),
                                                            self.chunk_index.data_ptr(), self.n_chunks, stream_ptr()),
                  "conv3d_wino_pack_weights_multi")
            for it in self.items.values():
                it[3] = it[0]._version
        return self

    def __deepcopy__(self, memo):
        """A copy starts empty and is re-learnt by the copy's first step: the packed tensors and the device table belong to
        the tensors of the network they were built from (WavBEST.__getstate__ drops the pack from copies anyway)."""
        return WinoPackedWeights()

    def get(self, w, groups, mode):
        key = (w.data_ptr(), mode)
        it = self.items.get(key)
        if it is not None and it[0].shape != w.shape:
            it = None
        if it is not None and it[3] == w._version:
            return it[2]
        if self.owner is not None and self._owner_ptrs is None:
            self._owner_ptrs = {t.data_ptr() for t in self.owner}
        foreign = self._owner_ptrs is not None and w.data_ptr() not in self._owner_ptrs
        if it is not None:              # registered, but the weight changed since the last refresh
            out = it[2]
        else:
            _chk(w.detach(), "weight")
            out = torch.empty(w.numel() * 2, device=w.device, dtype=torch.float32)   # six planes for three taps
        cout, cin = w.shape[0], w.shape[1] * groups
        if mode & 1:
            cout, cin = cin, cout
        check(lib.tmdiff_conv3d_wino_pack_weights(w.detach().data_ptr(), out.data_ptr(), cout, cin, groups, mode, 6, stream_ptr()),
              "conv3d_wino_pack_weights")
        if not foreign:
            self.items[key] = [w, groups, out, w._version]
        return out


PACKED = None      # the PackedWeights of the network being trained (set by WavBEST.forward_train; autograd.py consults it)
WINO_PACKED = None # ... and its WinoPackedWeights


def bf16_conv_supported(cout, cin, ksize, groups=1, seg_channels=None):
    """Shapes tmdiff_conv3d_fwd_bf16 accepts (include/tmdiff_hip.h); other layers stay on the fp32 kernel."""
    if ksize not in (1, 3) or cin % groups or cout % groups or (cout // groups) % 32:
        return False
    if (cin // groups) % (8 if ksize == 3 else 16):
        return False
    return all(c % 8 == 0 for c in (seg_channels or ()))


def pack_conv_weight_bf16(w, groups=1):
    """[Cout, Cin/g, k,k,k] fp32 -> bf16 packing [g][Cin_g/8][tap slots][Cout_g][8] (returned as an int16 tensor);
    28 tap slots for 3x3x3, one for 1x1x1."""
    cout, cin_g, k = w.shape[0], w.shape[1], w.shape[2]
    nbytes = lib.tmdiff_conv3d_packed_bf16_bytes(cout, cin_g * groups, k, groups) if tuple(w.shape[2:]) == (k, k, k) else 0
    if nbytes == 0:
        raise ValueError(f"conv weight {tuple(w.shape)} (groups={groups}) has no bf16 packing")
    out = torch.empty(nbytes // 2, device=w.device, dtype=torch.int16)
    check(lib.tmdiff_conv3d_pack_weights_bf16(_chk(w.detach(), "w"), out.data_ptr(), cout, cin_g * groups, k, groups,
                                              stream_ptr()), "conv3d_pack_weights_bf16")
    return out


def pack_conv_weight_bf16_dgrad(w, groups=1):
    """[Cout, Cin/g, 3,3,3] fp32 of a FORWARD convolution -> the bf16 packing of its data-gradient convolution (Cout -> Cin
    channels, taps mirrored, channel axes swapped per group; int16 storage): conv3d([g], packed, Cin, 3, math="bf16") == dL/dx'."""
    cout, cin_g = w.shape[0], w.shape[1]
    nbytes = lib.tmdiff_conv3d_packed_bf16_bytes(cin_g * groups, cout, 3, groups) if tuple(w.shape[2:]) == (3, 3, 3) else 0
    if nbytes == 0:
        raise ValueError(f"conv weight {tuple(w.shape)} (groups={groups}) has no bf16 data-gradient packing")
    out = torch.empty(nbytes // 2, device=w.device, dtype=torch.int16)
    check(lib.tmdiff_conv3d_pack_weights_bf16_dgrad(_chk(w.detach(), "w"), out.data_ptr(), cout, cin_g * groups, 3, groups,
                                                    stream_ptr()), "conv3d_pack_weights_bf16_dgrad")
    return out


class Bf16DgradWeights:
    """The bf16 data-gradient packings of the weights a finetune step with config.grad_bf16 runs through conv3d(math="bf16"),
    cached by the parameter's ``_version`` like PackedWeights: ``get`` re-packs a weight (one launch) only when it has changed
    since its packing was made -- once per weight and step after an optimizer update (optim.FusedAdamW bumps the versions of the
    parameters its kernel writes), never per layer call.  The packed tensor of a weight keeps its address across re-packs (a
    captured step replays on it).  ``owner`` = the weights of the network this cache belongs to, as for WinoPackedWeights: a
    weight that is not among them is packed on the spot and not kept."""

    def __init__(self, owner=None):
        self.items = {}          # weight address -> [weight, groups, packed, version]
        self.owner = None if owner is None else {w.data_ptr() for w in owner}

    def get(self, w, groups):
        if self.owner is not None and w.data_ptr() not in self.owner:
            return pack_conv_weight_bf16_dgrad(w, groups)
        it = self.items.get(w.data_ptr())
        if it is not None and (it[0].shape != w.shape or it[1] != groups or it[2].device != w.device):
            it = None
        if it is not None and it[3] == w._version:
            return it[2]
        if it is None:
            out = pack_conv_weight_bf16_dgrad(w, groups)
        else:
            out = it[2]
            check(lib.tmdiff_conv3d_pack_weights_bf16_dgrad(_chk(w.detach(), "w"), out.data_ptr(), w.shape[0], w.shape[1] * groups, 3,
                                                            groups, stream_ptr()), "conv3d_pack_weights_bf16_dgrad")
        _count("conv3d_pack_weights_bf16_dgrad")
        self.items[w.data_ptr()] = [w, groups, out, w._version]
        return out

    def __deepcopy__(self, memo):
        return Bf16DgradWeights()


BF16_DGRAD = None  # the Bf16DgradWeights of the network being trained with config.grad_bf16 (WavBEST.forward_train)


def make_conv_desc(segs, w_packed, cout, ksize, y, groups=1, bias=None, bias_scale=1.0, in_shift=None, in_scale=None,
                   shift_stride=0, scale_stride=0, in_act=False, in_mask=None, residual=None, out_scale=1.0,
                   y2=None, y2_shift=None, y2_scale=None, y2_shift_stride=0, y2_scale_stride=0, y2_act=False,
                   x_bf16_shape=None, drop=None, out_div=1, y2_s2d=False, x_s2d=False, res_conv=None, y_ll=None, y_hi=None,
                   side_xp=None):
    """Fill a tmdiff_conv3d_desc.  `segs` = list of 1..3 tensors [B, c_i, N, H, W] (concat-free input).
    in_shift / in_scale may be tensors or raw (ptr) ints into a projection bank.  y may be None when only the second
    output y2 = act2(y + y2_shift) * y2_scale (the consumer's prologue, same pointer conventions) is wanted.
    A y2 of dtype int16 is written as bf16 units [B, Cout/8, N*H*W, 8]; x_bf16_shape = (N, H, W) says that segs[0] is
    such a tensor (bf16 entry point only).  drop = (seed, p): in-kernel dropout of the prologue output (no mask tensor).
    out_div = 2: outputs / residual at half the H and W of the input (tmdiff_conv3d_ll_fwd).  y2_s2d: y2 in space-to-depth
    form [B, 4 Cout, N, H/2, W/2] (tmdiff_conv3d_wf_fwd / _w2_fwd); x_s2d: segs[0] is such a tensor and the descriptor is that of
    the convolution on the full-resolution tensor it stands for (tmdiff_conv3d_wfll_fwd).  res_conv = (x_raw [B, Cx, N, H, W],
    the 1x1x1 weight [Cout, Cx, 1, 1, 1] itself (contiguous fp32, not packed), Cx): a ResBlock's res_conv folded into the epilogue (tmdiff_conv3d_wf_fwd
    / _w2_fwd; desc.rc_*) -- the caller passes res_conv's bias as `bias` and no residual.  side_xp = dict(out= [B, Cin, N, H, W], shift=, shift_stride=,
    act=): a 1x1x1 convolution on the bandwidth kernel also writes act(x + shift) of its (segmented) input there -- the prologue
    output another convolution of the same input wants (desc.xp_*; routing.k1_side_xp)."""
    d = Conv3dDesc()
    if side_xp is not None:
        so, ssh = side_xp["out"], side_xp.get("shift")
        if ksize != 1 or tuple(so.shape) != (segs[0].shape[0], sum(s.shape[1] for s in segs), *segs[0].shape[2:]):
            raise ValueError("conv3d: side_xp goes with a 1x1x1 convolution; out = [B, Cin, N, H, W]")
        d.xp_out, d.xp_shift = _chk(so, "side_xp out"), (ssh if isinstance(ssh, int) else _chk(ssh, "side_xp shift"))
        d.xp_shift_stride, d.xp_act = int(side_xp.get("shift_stride", 0)), 1 if side_xp.get("act") else 0
    if res_conv is not None:
        rx, rw, rcin = res_conv
        if residual is not None or tuple(rx.shape) != (segs[0].shape[0], rcin, *segs[0].shape[2:]) or rw.numel() != rcin * cout:
            raise ValueError("conv3d: res_conv = (x [B, Cx, N, H, W], weight [Cout, Cx, 1, 1, 1], Cx) and no residual tensor")
        d.rc_x, d.rc_w, d.rc_cin = _chk(rx, "res_conv input"), _chk(rw, "res_conv weights"), int(rcin)
    if drop is not None:
        if in_mask is not None:
            raise ValueError("conv3d: give either in_mask (a mask tensor) or drop=(seed, p)")
        d.drop_seed, d.drop_p = int(drop[0]) & 0xFFFFFFFFFFFFFFFF, float(drop[1])
        if DROP_WORD is not None:         # the per-step part of the seed lives in device memory (HIP-graph replays)
            d.drop_seed_dev = DROP_WORD.data_ptr()
    if x_bf16_shape is not None:
        xp = segs[0]
        if len(segs) != 1 or xp.dtype != torch.int16 or xp.dim() != 4 or xp.shape[3] != 8 or not xp.is_contiguous():
            raise ValueError("conv3d: a bf16-packed input is one contiguous int16 tensor [B, Cin/8, N*H*W, 8]")
        b, (n, h, w) = xp.shape[0], x_bf16_shape
        if xp.shape[2] != n * h * w:
            raise ValueError("conv3d: packed input does not match x_bf16_shape")
        d.B, d.N, d.H, d.W = b, n, h, w
        d.Cin = xp.shape[1] * 8
        d.Cout, d.groups, d.ksize, d.nseg = cout, groups, ksize, 1
        d.seg_c[0], d.seg_x[0], d.x_bf16 = d.Cin, xp.data_ptr(), 1
    elif x_s2d:
        xs = segs[0]
        if len(segs) != 1 or xs.dim() != 5 or xs.shape[1] % 4:
            raise ValueError("conv3d: a space-to-depth input is one tensor [B, 4 Cin, N, H/2, W/2]")
        b, c4, n, h, w = xs.shape
        h, w = 2 * h, 2 * w
        d.B, d.N, d.H, d.W = b, n, h, w
        d.Cin, d.Cout, d.groups, d.ksize, d.nseg = c4 // 4, cout, groups, ksize, 1
        d.seg_c[0], d.seg_x[0] = c4 // 4, _chk(xs, "segment 0")
    else:
        b, _, n, h, w = segs[0].shape
        d.B, d.N, d.H, d.W = b, n, h, w
        d.Cin = sum(s.shape[1] for s in segs)
        d.Cout, d.groups, d.ksize, d.nseg = cout, groups, ksize, len(segs)
        for i, s in enumerate(segs):
            if tuple(s.shape[2:]) != (n, h, w) or s.shape[0] != b:
                raise ValueError("conv3d: input segments disagree on [B, N, H, W]")
            d.seg_c[i] = s.shape[1]
            d.seg_x[i] = _chk(s, f"segment {i}")
    if not isinstance(w_packed, int) and not (w_packed.is_cuda and w_packed.is_contiguous()):
        raise ValueError("w_packed: need a contiguous packed-weight tensor on the GPU")
    d.w_packed = w_packed if isinstance(w_packed, int) else w_packed.data_ptr()
    d.bias = _chk(bias, "bias")
    d.bias_scale = bias_scale
    d.in_shift = in_shift if isinstance(in_shift, int) else _chk(in_shift, "in_shift")
    d.in_scale = in_scale if isinstance(in_scale, int) else _chk(in_scale, "in_scale")
    d.in_shift_stride, d.in_scale_stride = shift_stride, scale_stride
    d.in_mask = _chk(in_mask, "in_mask")
    d.in_act = 1 if in_act else 0
    oshape = (b, cout, n, h // out_div, w // out_div)
    if residual is not None and tuple(residual.shape) != oshape:
        raise ValueError("conv3d: residual shape != output shape")
    d.residual = _chk(residual, "residual")
    d.out_scale = out_scale
    y2_packed = y2 is not None and y2.dtype == torch.int16
    for t, nm in ((y, "y"), (None if y2_packed else y2, "y2")):
        want = (b, 4 * cout, n, h // (2 * out_div), w // (2 * out_div)) if (y2_s2d and nm == "y2") else oshape
        if t is not None and tuple(t.shape) != want:
            raise ValueError(f"conv3d: {nm} shape {tuple(t.shape)} != {want}")
    if y2_packed and (tuple(y2.shape) != (b, cout // 8, n * h * w, 8) or not (y2.is_cuda and y2.is_contiguous())):
        raise ValueError(f"conv3d: packed y2 shape {tuple(y2.shape)} != {(b, cout // 8, n * h * w, 8)}")
    if y is None and y2 is None and not (y_ll is not None and y_hi is not None):
        raise ValueError("conv3d: no output")
    d.y = _chk(y, "y")
    d.y2 = y2.data_ptr() if y2_packed else _chk(y2, "y2")
    d.y2_shift = y2_shift if isinstance(y2_shift, int) else _chk(y2_shift, "y2_shift")
    d.y2_scale = y2_scale if isinstance(y2_scale, int) else _chk(y2_scale, "y2_scale")
    d.y2_shift_stride, d.y2_scale_stride = y2_shift_stride, y2_scale_stride
    d.y2_act = 1 if y2_act else 0
    d.y2_bf16 = 1 if y2_packed else 0
    d.y2_s2d = 1 if (y2_s2d and y2 is not None) else 0
    if y_ll is not None:       # third output: the halved LL band of y (tmdiff_conv3d_wf_fwd; y itself not written) ...
        q = (b, cout, n, h // 2, w // 2)
        if y is not None or (y2 is None) == (y_hi is None) or tuple(y_ll.shape) != q:
            raise ValueError("conv3d: y_ll [B, Cout, N, H/2, W/2] goes with y=None and EITHER a second output OR the three high bands")
        d.y_ll = _chk(y_ll, "y_ll")
        if y_hi is not None:   # ... or, with the three high bands, the whole Haar transform (LL through the y2 prologue constants)
            if len(y_hi) != 3 or any(tuple(t.shape) != q for t in y_hi):
                raise ValueError("conv3d: y_hi = (LH, HL, HH), each [B, Cout, N, H/2, W/2]")
            for i, t in enumerate(y_hi):
                d.y_hi[i] = _chk(t, "y_hi")
    return d


class ConvTimer:
    """Optional per-launch HIP-event timing of tmdiff_conv3d_fwd (used by bench.py for the roofline
    object).  Events are recorded on the launch stream; ``summary()`` resolves them after a sync."""

    def __init__(self):
        self.records = []        # (start_event, end_event, flops, ksize, entry point, _tag[, bytes])

    def summary(self, by_entry=False):
        """{ksize: (launches, ms, flops)}; with by_entry the key is (ksize, C entry point that served the launch)."""
        torch.cuda.synchronize()
        out = {}
        for e0, e1, fl, k, what, tag, *_ in self.records:
            key = (k, what, tag) if by_entry == "layer" else ((k, what) if by_entry else k)
            n, ms, f = out.get(key, (0, 0.0, 0.0))
            out[key] = (n + 1, ms + e0.elapsed_time(e1), f + fl)
        return out

    def bytes_summary(self, ksize=1):
        """(launches, ms, algorithmic HBM bytes) of the launches of one kernel size that recorded their bytes (the 1x1x1
        convolutions: input + output (+ residual) tensors once -- they are bandwidth kernels, priced against the copy rate)."""
        torch.cuda.synchronize()
        n, ms, nbytes = 0, 0.0, 0.0
        for rec in self.records:
            if rec[3] == ksize and len(rec) > 6:
                n, ms, nbytes = n + 1, ms + rec[0].elapsed_time(rec[1]), nbytes + rec[6]
        return n, ms, nbytes


def _tag(d):
    """Shape label of a launch for ConvTimer.summary(by_entry="layer"): channels, plane, what the epilogue reads / writes."""
    return (f"{d.Cin}->{d.Cout} g{d.groups} {d.N}x{d.H}x{d.W} b{d.B}" + (" seg%d" % d.nseg if d.nseg > 1 else "") +
            (" pro" if (d.in_act or d.in_shift or d.in_scale) else "") + (" +res" if d.residual else "") +
            (" y" if d.y else "") + (" y2" if d.y2 else "") + (" dwt" if d.y_hi[0] else (" ll" if d.y_ll else "")))


TIMER = None      # set to a ConvTimer() to time every conv launch
COUNTS = None     # set to a collections.Counter() to count convolution launches per C entry point ("conv3d_fwd",
                  # "conv3d_fwd_staged", "conv3d_fwd_bf16", "conv3d_wino4_fwd", "conv3d_wino2_fwd", "conv3d_ll_fwd"): the
                  # tests and bench.py's parity leg assert from it WHICH kernel family produced a result


DROP_WORD = None  # an int64 [1] device tensor: its value is added to every in-kernel dropout seed when the kernel starts
                  # (tmdiff_conv3d_desc.drop_seed_dev).  The captured finetune step (tmdiff_amd.model) sets it and bumps it
                  # inside the graph, so that replays of the same recorded launches draw fresh masks.


FLOPS = None      # set to [0.0] to add up the multiply-add FLOPs the convolution launches EXECUTE on the matrix pipe (Winograd
                  # and composed kernels execute fewer than the reference's operator order): bench.py's train_step object


def _count(what, flops=0.0):
    if COUNTS is not None:
        COUNTS[what] += 1
    if FLOPS is not None:
        FLOPS[0] += flops


_WS = {}     # (device index, stream) -> grow-only scratch tensor (prologue outputs / bf16-packed conv inputs); launches
             # on one stream are ordered, so consecutive convolutions can reuse it; other streams get their own


def scratch_like(segs, tag):
    """A [B, sum of channels, N, H, W] fp32 view of the per-stream scratch `tag` (contents live until its next user on the stream)."""
    b, _, n, h, w = segs[0].shape
    shape = (b, sum(s.shape[1] for s in segs), n, h, w)
    numel = shape[0] * shape[1] * n * h * w
    return _workspace(segs[0].device, numel * 4, tag).view(torch.float32)[:numel].view(shape)


def _workspace(device, nbytes, tag="x"):
    key = (device.index, stream_ptr(), tag)
    ws = _WS.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = _WS[key] = torch.empty(nbytes, device=device, dtype=torch.uint8)
    return ws


# The launch steps every forward-convolution wrapper (conv3d, conv3d_wf, conv3d_ll, conv3d_wf_ll, fallback.conv3d_wino) shares.

def _outputs(what, dev, y_shape, keep_y, emit, y2_shape, y2_dtype=torch.float32, out=None):
    """(y, y2): y = `out`, else a fresh tensor unless keep_y=False; y2 when `emit` asks for it and y2_shape is given."""
    y = out if out is not None else (torch.empty(*y_shape, device=dev, dtype=torch.float32) if keep_y else None)
    if emit is None and y is None:
        raise ValueError(f"{what}: keep_y=False needs emit=")
    return y, (torch.empty(*y2_shape, device=dev, dtype=y2_dtype) if emit is not None and y2_shape is not None else None)


def _emit_kw(emit):
    """make_conv_desc keywords of the second output y2 = act(y + shift) * scale that `emit` describes."""
    return {} if emit is None else dict(y2_act=emit.get("act", False), y2_shift=emit.get("shift"), y2_scale=emit.get("scale"),
                                        y2_shift_stride=emit.get("shift_stride", 0), y2_scale_stride=emit.get("scale_stride", 0))


def _result(y, y2):
    """The return convention of the wrappers: y, (y, y2), or y2 alone (keep_y=False)."""
    return y if y2 is None else ((y, y2) if y is not None else y2)


def _plain(segs, kw):
    """One input tensor that the kernel reads as it stands: no prologue, mask or dropout."""
    return len(segs) == 1 and not (kw.get("in_act") or kw.get("in_shift") is not None or kw.get("in_scale") is not None or
                                   kw.get("in_mask") is not None or kw.get("drop") is not None)


def _lend_splitk(d, dev, nbytes):
    """Lend the split-K workspace a small grid asks for (nbytes 0: the launch runs unsplit)."""
    if nbytes:
        d.splitk_ws, d.splitk_ws_bytes = _workspace(dev, nbytes, "splitk").data_ptr(), nbytes


def _xp_target(what, xp_out, nbytes, dev):
    """Address the prologue pass writes x' (nbytes) to: the caller's xp_out, else the shared scratch (None: no pass)."""
    if not nbytes:
        return None
    if xp_out is None:
        return _workspace(dev, nbytes).data_ptr()
    if not (xp_out.is_cuda and xp_out.is_contiguous() and xp_out.numel() * 4 == nbytes):
        raise ValueError(f"{what}: xp_out must be a contiguous fp32 [B, Cin, N, H, W] tensor")
    return xp_out.data_ptr()


def _launch(fn, d, args, what, key, flops, ksize=3, suffix="", bytes_of=None):
    """Count the launch (COUNTS[key] unless key is None, FLOPS += flops), then run fn(&d, *args, stream), checked as `what`.
    With TIMER set the launch is bracketed by HIP events and recorded as (e0, e1, flops, ksize, what, tag[, bytes_of(d)])."""
    if key is not None:
        _count(key, flops)
    if TIMER is None:
        check(fn(C.byref(d), *args, stream_ptr()), what)
        return
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    check(fn(C.byref(d), *args, stream_ptr()), what)
    e1.record()
    rec = (e0, e1, flops, ksize, what, _tag(d) + suffix)
    TIMER.records.append(rec if bytes_of is None else rec + (bytes_of(d),))


def _conv3d_bytes(d):
    """Algorithmic HBM bytes of a conv3d launch: input once (2 B per element for packed bf16 units, else 4), outputs and
    residual once (+ the by-product x' of a side_xp launch: Cin more channels written)."""
    y2_b = 0.0 if not d.y2 else (2.0 if d.y2_bf16 else 4.0)
    return d.B * d.N * d.H * d.W * ((2.0 if d.x_bf16 else 4.0) * d.Cin +
                                    d.Cout * (4.0 * ((1 if d.y else 0) + (1 if d.residual else 0)) + y2_b) +
                                    (4.0 * d.Cin if d.xp_out else 0.0))


def conv3d(segs, w_packed, cout, ksize, out=None, math="fp32", pack_input=None, staged=None, emit=None, keep_y=True,
           x_bf16_shape=None, xp_out=None, **kw):
    """math="fp32": exact-fp32 MFMA kernel (w_packed from pack_conv_weight); "bf16": bf16 operands / fp32
    accumulation (w_packed from pack_conv_weight_bf16).  pack_input (bf16 only): True = pack the prologue output to
    bf16 once and run the staging-free kernel (default), False = one fused kernel.  staged (fp32 only): True = prologue
    pass + global_load_lds staged kernel (default where the shape allows), False = the fused kernel.
    emit = dict(act=, shift=, scale=, shift_stride=, scale_stride=): also produce y2 = act(y + shift) * scale, the
    consumer's prologue applied in this convolution's epilogue; returns (y, y2), or y2 alone with keep_y=False.  In the
    bf16 mode y2 is the packed bf16 tensor [B, Cout/8, N*H*W, 8] (int16 storage) that a following bf16 convolution takes
    as its input with x_bf16_shape=(N, H, W), skipping its pack pass.
    xp_out (fp32, 3x3x3): a [B, Cin, N, H, W] tensor that receives the prologue output x' (forces the staged kernel, whose
    prologue pass writes it there instead of the shared scratch) -- the training path keeps it for the weight gradient."""
    if kw.get("res_conv") is not None or kw.get("y_ll") is not None or (emit is not None and (emit.get("ll") or emit.get("dwt"))):
        raise ValueError("conv3d: only conv3d_wf / conv3d_w2 fold a residual convolution into their epilogue / write the LL band")
    b, _, n, h, w = segs[0].shape if x_bf16_shape is None else (segs[0].shape[0], None, *x_bf16_shape)
    dev = segs[0].device
    bf16 = math == "bf16"
    y, y2 = _outputs("conv3d", dev, (b, cout, n, h, w), keep_y, emit,
                     (b, cout // 8, n * h * w, 8) if bf16 else (b, cout, n, h, w), torch.int16 if bf16 else torch.float32, out)
    d = make_conv_desc(segs, w_packed, cout, ksize, y, y2=y2, x_bf16_shape=x_bf16_shape, **kw, **_emit_kw(emit))
    if d.xp_out and (math != "fp32" or not lib.tmdiff_conv3d_fwd_xp_supported(C.byref(d))):
        raise ValueError("conv3d: side_xp needs the 16-byte 1x1x1 bandwidth kernel (ask routing.k1_side_xp first)")
    if bf16:
        if w_packed.dtype != torch.int16:
            raise TypeError("conv3d(math='bf16') needs weights from pack_conv_weight_bf16")
        if pack_input is None:
            pack_input = {"0": False, "1": True}.get(config.bf16_pack, True)   # measured: the two-kernel variant wins on every production layer
        nb = lib.tmdiff_conv3d_bf16_workspace_bytes(C.byref(d))      # (0: the pack pass's grid cannot hold B * Cin / 8 rows)
        ws = _workspace(dev, nb).data_ptr() if pack_input and ksize == 3 and x_bf16_shape is None and nb else None
        fn, args, what = lib.tmdiff_conv3d_fwd_bf16, (ws,), "conv3d_fwd_bf16"
    elif math == "fp32":
        if not isinstance(w_packed, int) and w_packed.dtype != torch.float32:
            raise TypeError("conv3d(math='fp32') needs weights from pack_conv_weight")
        if ksize == 3:      # (split-K: small grids only -- B = 1, the 8x8 / 16x16 levels at small batches)
            _lend_splitk(d, dev, lib.tmdiff_conv3d_fwd_splitk_workspace_bytes(C.byref(d)))
        if staged is None:       # (the rule and its measurements: routing.direct_family)
            staged = ksize == 3 and routing.direct_family(d.Cin, cout, d.groups, _plain(segs, kw), kw.get("in_mask") is not None,
                                                          kw.get("drop") is not None, extents=(b, n, h, w)) == "staged"
        if xp_out is not None:
            staged = True
            if not lib.tmdiff_conv3d_fwd_staged_supported(C.byref(d)):
                raise ValueError("conv3d: xp_out needs the staged kernel, which does not take this shape")
        if staged and lib.tmdiff_conv3d_fwd_staged_supported(C.byref(d)):
            nb = lib.tmdiff_conv3d_fwd_staged_workspace_bytes(C.byref(d))
            fn, args, what = lib.tmdiff_conv3d_fwd_staged, (_xp_target("conv3d", xp_out, nb, dev),), "conv3d_fwd_staged"
        else:
            fn, args, what = lib.tmdiff_conv3d_fwd, (), "conv3d_fwd"
    else:
        raise ValueError(f"conv3d: unknown math {math!r}")
    _launch(fn, d, args, what, what if ksize == 3 else what + "_k1",
            2.0 * b * cout * (d.Cin // d.groups) * ksize ** 3 * n * h * w, ksize, " +xp" if d.xp_out else "", _conv3d_bytes)
    return _result(y, y2)


def conv3d_prologue(segs, **kw):
    """x' = the prologue output of a convolution of `segs` (kw: make_conv_desc's in_act / in_shift / in_scale / in_mask / drop),
    [B, Cin, N, H, W], as a tensor of its own."""
    b, _, n, h, w = segs[0].shape
    cin = sum(s.shape[1] for s in segs)
    xp = torch.empty(b, cin, n, h, w, device=segs[0].device, dtype=torch.float32)
    d = make_conv_desc(segs, 0, cin, 1, xp, **kw)      # (the pass reads the extents, the segments and the prologue fields)
    check(lib.tmdiff_conv3d_prologue_fwd(C.byref(d), xp.data_ptr(), stream_ptr()), "conv3d_prologue_fwd")
    return xp


def pack_conv_weight_wino(w, groups=1, mode=0, planes=6):
    """[Cout, Cin/groups, 3, 3, 3] -> the transformed, packed weights of the Winograd-along-n convolution (conv3d_wino);
    planes = wino_planes(N) of the tensors it will run on.  mode bit 0: the weights of the DATA-GRADIENT convolution
    (Cout -> Cin channels, transposed, taps mirrored) of the forward convolution whose weight w is; mode bit 1 (value 2):
    natural column order, the form conv3d_wf takes (conv3d_wino: interleaved 64-channel tiles)."""
    cout, cin = w.shape[0], w.shape[1] * groups
    if mode & 1:
        cout, cin = cin, cout
    nb = lib.tmdiff_conv3d_wino_packed_bytes(cout, cin, groups, planes)
    if tuple(w.shape[2:]) != (3, 3, 3) or nb == 0:
        raise ValueError(f"pack_conv_weight_wino: weight shape {tuple(w.shape)} (groups {groups}, mode {mode}, planes {planes}) not supported")
    out = torch.empty(nb // 4, device=w.device, dtype=torch.float32)
    check(lib.tmdiff_conv3d_wino_pack_weights(_chk(w.detach(), "w"), out.data_ptr(), cout, cin, groups, mode, planes, stream_ptr()),
          "conv3d_wino_pack_weights")
    return out


# routing lives in tmdiff_amd/routing.py; these names stay importable from ops (tests, tools)
wino_conv_supported = routing.wino_weight_ok
ll_conv_supported = routing.ll_weight_ok       # (shapes tmdiff_conv3d_ll_fwd takes)
wf_route = routing.wf_route
wfll_route = routing.wfll_route


class ConvWeights:
    """The packed forms of one 3x3x3 convolution weight, each produced on first use: direct() (pack_conv_weight), wf()
    (pack_conv_weight_wino mode | 2, planes 6), wino(planes) (fallback kernels).  Any callable may be None: that family is
    then not offered for this weight (conv3d_auto falls through to the next rule)."""

    def __init__(self, direct, wf=None, wino=None, w2=None):
        self.direct, self.wf, self.wino, self.w2 = direct, wf, wino, w2      # w2(): pack_conv_weight_w2 (conv3d_w2)


def conv3d_auto(segs, weights, cout, groups=1, math="fp32", emit=None, keep_y=True, xp_out=None, x_bf16_shape=None, family=None,
                **kw):
    """A 3x3x3 convolution on the kernel family routing.conv3_family picks for its extents (same keyword arguments and
    return convention as conv3d): conv3d_wf, the direct kernels (staged / fused), the bf16 kernel, or -- band counts other
    than 4 / 8 -- tmdiff_amd.fallback.conv3d_wino.  family: that answer, where the caller holds it already (the finetune
    graph's plans, routing.train_conv_plan)."""
    if math == "bf16" or x_bf16_shape is not None:
        return conv3d(segs, weights.direct(), cout, 3, groups=groups, math=math, emit=emit, keep_y=keep_y,
                      x_bf16_shape=x_bf16_shape, **kw)
    b, _, n, h, w = segs[0].shape
    cin = sum(s_.shape[1] for s_ in segs)
    masked, dropout, plain = kw.get("in_mask") is not None, kw.get("drop") is not None, _plain(segs, kw)
    fam = family or routing.conv3_family(b, cin, cout, n, h, w, groups, plain=plain, masked=masked, dropout=dropout,
                                         keep_xp=xp_out is not None)
    if (fam in ("wf", "wf_pair") and weights.w2 is not None and family is None and xp_out is None and len(segs) == 1 and
            not masked and not dropout):
        rc = kw.get("res_conv")
        quarter = bool(emit is not None and (emit.get("s2d") or emit.get("ll") or emit.get("dwt")))
        if (routing.wino2d_epilogue_route(b, cin, cout, n, h, w, groups, int(rc[2]) if rc is not None else 0, quarter)
                if (rc is not None or quarter) else routing.wino2d_route(b, cin, cout, n, h, w, groups)):
            return conv3d_w2(segs[0], weights.w2(), cout, emit=emit, keep_y=keep_y, **kw)
    if fam in ("wf", "wf_pair") and weights.wf is not None:
        return conv3d_wf(segs, weights.wf(), cout, emit=emit, keep_y=keep_y, groups=groups, xp_out=xp_out, **kw)
    if fam in ("wino4", "wino2") and weights.wino is not None:
        from . import fallback
        planes = 6 if fam == "wino4" else 4
        return fallback.conv3d_wino(segs, weights.wino(planes), cout, planes, emit=emit, keep_y=keep_y, groups=groups,
                                    xp_out=xp_out, **kw)
    if (emit is not None and (emit.get("s2d") or emit.get("ll") or emit.get("dwt"))) or kw.get("res_conv") is not None:
        raise ValueError("conv3d_auto: only conv3d_wf / conv3d_w2 write a space-to-depth second output / fold a residual convolution "
                         "(ask routing.wf_route first)")
    if fam not in ("staged", "fused"):      # (a direct family named by conv3_family is direct_family's answer already)
        fam = routing.direct_family(cin, cout, groups, plain, masked, dropout, xp_out is not None, extents=(b, n, h, w))
    return conv3d(segs, weights.direct(), cout, 3, groups=groups, staged=fam == "staged", emit=emit, keep_y=keep_y,
                  xp_out=xp_out, **kw)


def conv3d_wf(segs, w_packed, cout, emit=None, keep_y=True, groups=1, xp_out=None, **kw):
    """conv3d(segs, ...) (fp32, 3x3x3) through the Winograd F(4,3)-along-the-bands kernel that transforms its input INSIDE the
    kernel (csrc/conv3d_wf.hip; 8- or 4-band tensors, the whole band axis in one workgroup): no transformed copy of the input,
    no transform pass -- an input that is one plain tensor is read as it stands, any other (prologue, segments, dropout) goes
    through one elementwise prologue pass first (its output lands in xp_out when given: the finetune path keeps it for the
    weight gradient).  Same keyword arguments and return convention as conv3d; w_packed = the weights from
    pack_conv_weight_wino(w, groups, mode | 2, planes=6).  Runs whatever the grid size (routing.conv3_family is where small
    grids are sent elsewhere); raises for shapes the kernel does not take."""
    b, _, n, h, w = segs[0].shape
    dev = segs[0].device
    s2d = bool(emit is not None and emit.get("s2d"))
    want_ll = bool(emit is not None and emit.get("ll"))      # third output: LL(y) / 2 instead of y (returns (y2, y_ll))
    want_dwt = bool(emit is not None and emit.get("dwt"))    # the whole Haar transform of y instead of y: returns (LL', LH, HL, HH),
    if want_dwt and (s2d or want_ll):                        # LL' = the halved LL band through the `emit` prologue
        raise ValueError("conv3d_wf: emit dwt=True excludes s2d / ll")
    want_ll = want_ll or want_dwt
    if s2d or want_ll:
        cin = sum(s_.shape[1] for s_ in segs)
        if not routing.wf_quarter_ok(b, cin, cout, n, h, w, groups):
            raise ValueError("conv3d_wf: this launch cannot write a space-to-depth / LL output (ask routing.wf_quarter_ok first)")
    if want_ll and keep_y:
        raise ValueError("conv3d_wf: the LL output replaces y (keep_y=False)")
    # what the library would refuse only after the launch has been counted: the pair mode (8 bands x 8 columns) writes no LL /
    # Haar output and folds no residual convolution, the LL / Haar output needs 8 bands, the fold groups 1 and 32 k <= 512 channels
    pair = n == 8 and w == 8
    if want_ll and (pair or n != 8):
        raise ValueError("conv3d_wf: the LL / Haar output needs 8 bands and planes wider than 8 columns")
    rc = kw.get("res_conv")
    if rc is not None and (pair or groups != 1 or int(rc[2]) <= 0 or int(rc[2]) % 32 or int(rc[2]) > 512):
        raise ValueError("conv3d_wf: a folded residual convolution needs groups 1, rc_cin % 32 == 0 (at most 512) and planes "
                         "wider than 8 columns")
    q = (b, cout, n, h // 2, w // 2)       # (allocated before y and y2 -- y is None whenever y_ll is wanted)
    y_ll = torch.empty(*q, device=dev, dtype=torch.float32) if want_ll else None
    y_hi = [torch.empty(*q, device=dev, dtype=torch.float32) for _ in range(3)] if want_dwt else None
    y, y2 = _outputs("conv3d_wf", dev, (b, cout, n, h, w), keep_y, emit,
                     None if want_dwt else ((b, 4 * cout, n, h // 2, w // 2) if s2d else (b, cout, n, h, w)))
    d = make_conv_desc(segs, w_packed, cout, 3, y, y2=y2, groups=groups, y2_s2d=s2d, y_ll=y_ll, y_hi=y_hi, **kw,
                       **_emit_kw(emit))
    if not lib.tmdiff_conv3d_wf_supported(C.byref(d)):
        raise ValueError("conv3d_wf: shape not supported")
    # (a launch that writes an LL / Haar / space-to-depth output runs unsplit: no workspace is lent)
    _lend_splitk(d, dev, lib.tmdiff_conv3d_wf_splitk_workspace_bytes(C.byref(d)) if (config.wf_splitk and not want_ll) else 0)
    nws = lib.tmdiff_conv3d_wf_workspace_bytes(C.byref(d))
    ws = _xp_target("conv3d_wf", xp_out, nws, dev)
    if xp_out is not None and not nws:          # plain input: x' IS the input
        xp_out.copy_(segs[0] if len(segs) == 1 else torch.cat(segs, 1))
    # EXECUTED flops: 54 multiply-adds per (ci, co) and tile of four output bands (the direct kernel: 27 per band), plus the
    # folded res_conv's rc_cin multiply-adds per output
    flops = 2.0 * b * cout * ((d.Cin // groups) * 13.5 + d.rc_cin) * n * h * w
    _launch(lib.tmdiff_conv3d_wf_fwd, d, (ws,), "conv3d_wf_fwd", "conv3d_wf_fwd", flops, 3, f" +rc{d.rc_cin}" if d.rc_cin else "")
    return (y_ll, *y_hi) if want_dwt else (y2, y_ll) if want_ll else _result(y, y2)


def pack_conv_weight_w2(w):
    """[Cout, Cin, 3, 3, 3] -> the weights of conv3d_w2: (G_band (x) G_w) w as [24 planes][dh][Cin / 4][Cout][4] floats."""
    cout, cin = w.shape[0], w.shape[1]
    nb = lib.tmdiff_conv3d_w2_packed_bytes(cout, cin)
    if tuple(w.shape[2:]) != (3, 3, 3) or nb == 0:
        raise ValueError(f"pack_conv_weight_w2: weight shape {tuple(w.shape)} not supported")
    out = torch.empty(nb // 4, device=w.device, dtype=torch.float32)
    check(lib.tmdiff_conv3d_w2_pack_weights(_chk(w.detach(), "w"), out.data_ptr(), cout, cin, stream_ptr()), "conv3d_w2_pack_weights")
    return out


def conv3d_w2(x, w_packed, cout, emit=None, keep_y=True, stages=0, **kw):
    """conv3d([x], ...) (fp32, 3x3x3, groups 1) with Winograd along the bands AND the width (csrc/conv3d_w2.hip): an input pass
    (the prologue keywords in_shift / in_scale / in_act are applied on the way), one GEMM per Winograd plane, an output pass with
    bias / residual / out_scale / emit as in conv3d -- and, as conv3d_wf (same checks, same return conventions), emit's s2d /
    ll / dwt outputs and res_conv= (the folded 1x1x1, multiplied inside the output pass).  The Winograd-domain arrays live in
    the per-stream scratch "w2", lent to the library like the split-K workspace.  w_packed from pack_conv_weight_w2; shapes:
    routing.wino2d_ok, with those epilogues routing.wino2d_epilogue_ok.  stages: a bit mask of the launches that run (1 input
    pass, 2 GEMM, 4 output pass; timing), 0 = all."""
    b, _, n, h, w = x.shape
    dev = x.device
    s2d = bool(emit is not None and emit.get("s2d"))
    want_ll = bool(emit is not None and emit.get("ll"))      # third output: LL(y) / 2 instead of y (returns (y2, y_ll))
    want_dwt = bool(emit is not None and emit.get("dwt"))    # the whole Haar transform instead of y: returns (LL', LH, HL, HH)
    if want_dwt and (s2d or want_ll):
        raise ValueError("conv3d_w2: emit dwt=True excludes s2d / ll")
    want_ll = want_ll or want_dwt
    if want_ll and keep_y:
        raise ValueError("conv3d_w2: the LL output replaces y (keep_y=False)")
    rc = kw.get("res_conv")
    if rc is not None and kw.get("residual") is not None:
        raise ValueError("conv3d_w2: res_conv excludes a residual tensor")
    if (s2d or want_ll or rc is not None) and not routing.wino2d_epilogue_ok(b, x.shape[1], cout, n, h, w, 1,
                                                                             int(rc[2]) if rc is not None else 0, s2d or want_ll):
        raise ValueError("conv3d_w2: this launch cannot fold a 1x1x1 / write a space-to-depth / LL output "
                         "(ask routing.wino2d_epilogue_ok first)")
    q = (b, cout, n, h // 2, w // 2)
    y_ll = torch.empty(*q, device=dev, dtype=torch.float32) if want_ll else None
    y_hi = [torch.empty(*q, device=dev, dtype=torch.float32) for _ in range(3)] if want_dwt else None
    y, y2 = _outputs("conv3d_w2", dev, (b, cout, n, h, w), keep_y, emit,
                     None if want_dwt else ((b, 4 * cout, n, h // 2, w // 2) if s2d else (b, cout, n, h, w)))
    d = make_conv_desc([x], w_packed, cout, 3, y, y2=y2, y2_s2d=s2d, y_ll=y_ll, y_hi=y_hi, **kw, **_emit_kw(emit))
    if not lib.tmdiff_conv3d_w2_epilogue_supported(C.byref(d)):
        raise ValueError("conv3d_w2: shape not supported (routing.wino2d_ok / wino2d_epilogue_ok)")
    nws = lib.tmdiff_conv3d_w2_workspace_bytes(C.byref(d))
    ws = _workspace(dev, nws, "w2").data_ptr()
    # EXECUTED flops: 24 planes x 3 row taps per tile of four bands and two columns = 9 multiply-adds per (ci, co, output), plus
    # the folded res_conv's rc_cin multiply-adds per output
    flops = 2.0 * b * cout * (d.Cin * 9.0 + d.rc_cin) * n * h * w
    _launch(lib.tmdiff_conv3d_w2_fwd, d, (ws, int(stages)), "conv3d_w2_fwd", "conv3d_w2_fwd", flops, 3,
            f" +rc{d.rc_cin}" if d.rc_cin else "")
    return (y_ll, *y_hi) if want_dwt else (y2, y_ll) if want_ll else _result(y, y2)


def pack_conv_weight_ll(w, ll_scale=0.5):
    """[Cout, Cin, 3, 3, 3] -> the composed, packed weights of `3x3x3 convolution, then LL band * ll_scale` (conv3d_ll)."""
    cout, cin = w.shape[0], w.shape[1]
    nb = lib.tmdiff_conv3d_ll_packed_bytes(cout, cin)
    if tuple(w.shape[2:]) != (3, 3, 3) or nb == 0:
        raise ValueError(f"pack_conv_weight_ll: weight shape {tuple(w.shape)} not supported")
    out = torch.empty(nb // 4, device=w.device, dtype=torch.float32)
    check(lib.tmdiff_conv3d_ll_pack_weights(_chk(w.detach(), "w"), out.data_ptr(), cout, cin, float(ll_scale), stream_ptr()),
          "conv3d_ll_pack_weights")
    return out


def conv3d_ll(x, w_packed, cout, ll_scale=0.5, emit=None, keep_y=True, **kw):
    """haar_dwt2d(conv3d(x, w), want_high=False, ll_scale)[0] as ONE strided convolution (csrc/conv3d_ll.hip): x is one
    plain fp32 tensor [B, Cin, N, H, W] (H, W even), the result [B, Cout, N, H/2, W/2].  bias / residual / out_scale / emit
    as in conv3d (residual and the outputs at the halved size); returns y, (y, y2) or y2 alone (keep_y=False)."""
    b, _, n, h, w = x.shape
    dev = x.device
    oshape = (b, cout, n, h // 2, w // 2)
    y, y2 = _outputs("conv3d_ll", dev, oshape, keep_y, emit, oshape)
    d = make_conv_desc([x], w_packed, cout, 3, y, y2=y2, out_div=2, **kw, **_emit_kw(emit))
    if not lib.tmdiff_conv3d_ll_supported(C.byref(d)):
        raise ValueError("conv3d_ll: shape not supported (ll_conv_supported)")
    _lend_splitk(d, dev, lib.tmdiff_conv3d_ll_splitk_workspace_bytes(C.byref(d)))
    # EXECUTED flops: 48 multiply-adds per (ci, co, output position) -- the pair it replaces would execute 4 x 27
    _launch(lib.tmdiff_conv3d_ll_fwd, d, (float(ll_scale),), "conv3d_ll_fwd", "conv3d_ll_fwd",
            2.0 * b * cout * d.Cin * 48 * n * (h // 2) * (w // 2))
    return _result(y, y2)


def pack_conv_weight_wfll(w, ll_scale=0.5):
    """Weights of conv3d_wf_ll: the composed 3x4x4 kernel of conv3d_ll split by row / column parity (2 x 2 taps per virtual
    channel of the space-to-depth input) and transformed along the bands (F(4,3)): [Cin, 2, 2, 4, 6, Cout] floats."""
    cout, cin = w.shape[0], w.shape[1]
    out = torch.empty(cin * 96 * cout, device=w.device, dtype=torch.float32)
    check(lib.tmdiff_conv3d_wfll_pack_weights(_chk(w.detach(), "w"), out.data_ptr(), cout, cin, float(ll_scale), stream_ptr()),
          "conv3d_wfll_pack_weights")
    return out


def conv3d_wf_ll(x_s2d, w_packed, cout, ll_scale=0.5, emit=None, keep_y=True, **kw):
    """conv3d_ll (Conv_0 + halved LL band as one convolution) with Winograd F(4,3) along the bands on top
    (tmdiff_conv3d_wfll_fwd): x_s2d is the producer's space-to-depth second output [B, 4 Cin, N, H/2, W/2]
    (conv3d_wf(..., emit=dict(..., s2d=True))), w_packed from pack_conv_weight_wfll; result and conventions as conv3d_ll."""
    b, c4, n, h2, w2 = x_s2d.shape
    dev = x_s2d.device
    oshape = (b, cout, n, h2, w2)
    y, y2 = _outputs("conv3d_wf_ll", dev, oshape, keep_y, emit, oshape)
    d = make_conv_desc([x_s2d], w_packed, cout, 3, y, y2=y2, out_div=2, x_s2d=True, **kw, **_emit_kw(emit))
    if not lib.tmdiff_conv3d_wfll_supported(C.byref(d)):
        raise ValueError("conv3d_wf_ll: shape not supported")
    _lend_splitk(d, dev, lib.tmdiff_conv3d_wfll_splitk_workspace_bytes(C.byref(d)) if config.wf_splitk else 0)
    # EXECUTED flops: 16 taps x 6 planes per tile of four bands = 24 multiply-adds per (ci, co, output position)
    _launch(lib.tmdiff_conv3d_wfll_fwd, d, (float(ll_scale),), "conv3d_wfll_fwd", "conv3d_wfll_fwd",
            2.0 * b * cout * d.Cin * 24 * n * h2 * w2)
    return _result(y, y2)


def stem(w, bias, out_channels, xin=None, pan=None, ms=None, silu=True, out=None, out_scale=None, out_scale_stride=0,
         pack_bf16=False):
    """out_scale (tensor [B, C0] or a raw pointer into a projection bank, row stride out_scale_stride): the consumer's
    modulation folded into the stem's output.  pack_bf16: the result as packed bf16 units [B, C0/8, N*H*W, 8] (int16
    storage), the input form of a bf16 convolution (x_bf16_shape=(N, H, W))."""
    ref = ms if ms is not None else xin
    b, n, h, wd = ref.shape
    osc = out_scale if isinstance(out_scale, int) else _chk(out_scale, "out_scale")
    if pack_bf16:
        units = torch.empty(b, out_channels // 8, n * h * wd, 8, device=ref.device, dtype=torch.int16)
        check(lib.tmdiff_stem_fwd_pack_bf16(_chk(xin, "xin"), _chk(pan, "pan"), _chk(ms, "ms"), _chk(w, "w"), _chk(bias, "bias"),
                                            osc, out_scale_stride, units.data_ptr(), b, out_channels, n, h, wd,
                                            1 if silu else 0, stream_ptr()), "stem_fwd_pack_bf16")
        return units
    y = out if out is not None else torch.empty(b, out_channels, n, h, wd, device=ref.device, dtype=torch.float32)
    osc = out_scale if isinstance(out_scale, int) else _chk(out_scale, "out_scale")
    check(lib.tmdiff_stem_fwd_scaled(_chk(xin, "xin"), _chk(pan, "pan"), _chk(ms, "ms"), _chk(w, "w"), _chk(bias, "bias"),
                                     osc, out_scale_stride, _chk(y, "y"), b, out_channels, n, h, wd, 1 if silu else 0,
                                     stream_ptr()), "stem_fwd")
    return y


def head(x, w, scale, scale_stride=0, out=None):
    b, c, n, h, wd = x.shape
    y = out if out is not None else torch.empty(b, n, h, wd, device=x.device, dtype=torch.float32)
    check(lib.tmdiff_head_fwd(_chk(x, "x"), _chk(w, "w"), scale if isinstance(scale, int) else _chk(scale, "scale"),
                              scale_stride, _chk(y, "y"), b, c, n * h * wd, stream_ptr()), "head_fwd")
    return y


def _plane_prologue(pro, channels, n_per_channel):
    """pro = dict(act=, shift=, scale=, shift_stride=, scale_stride=) (tensors or raw bank pointers) -> ctypes struct"""
    if pro is None:
        return None
    q = _lib.PlanePrologue()
    q.shift = pro.get("shift") if isinstance(pro.get("shift"), int) else _chk(pro.get("shift"), "prologue shift")
    q.scale = pro.get("scale") if isinstance(pro.get("scale"), int) else _chk(pro.get("scale"), "prologue scale")
    q.shift_stride, q.scale_stride = pro.get("shift_stride", 0), pro.get("scale_stride", 0)
    q.C, q.n_per_channel, q.act = channels, n_per_channel, 1 if pro.get("act") else 0
    return C.byref(q)


def haar_dwt2d(x, want_high=True, ll_scale=1.0, hi_scale=1.0, outs=None, ll_prologue=None, pack_bf16=False):
    """x [..., H, W] -> (ll, lh, hl, hh); the high bands are None when want_high is False.
    ll_prologue (x must then be [B, C, N, H, W]): the consumer convolution's prologue applied to the LL band as it is
    written -- dict(act=, shift=, scale=, shift_stride=, scale_stride=), per (b, c)."""
    hh_, ww = x.shape[-2:]
    planes = x.numel() // (hh_ * ww)
    shape = (*x.shape[:-2], hh_ // 2, ww // 2)
    if pack_bf16:     # bf16 mode: LL as packed bf16 units [B, C/8, N*h*w, 8] (int16 storage), high bands fp32
        b, c, n = x.shape[:3]
        units = torch.empty(b, c // 8, n * (hh_ // 2) * (ww // 2), 8, device=x.device, dtype=torch.int16)
        hi = [torch.empty(shape, device=x.device, dtype=torch.float32) for _ in range(3)] if want_high else [None] * 3
        pro = _plane_prologue(ll_prologue, c, n) if ll_prologue is not None else None
        check(lib.tmdiff_haar_dwt2d_pack_bf16(_chk(x, "x"), units.data_ptr(), *[_chk(t, "band") for t in hi], b, c, n, hh_, ww,
                                              ll_scale, hi_scale, pro, stream_ptr()), "haar_dwt2d_pack_bf16")
        return (units, *hi)
    if outs is None:
        outs = [torch.empty(shape, device=x.device, dtype=torch.float32) for _ in range(4 if want_high else 1)]
    ptrs = [_chk(o, "band") for o in outs] + [None] * (4 - len(outs))
    pro = _plane_prologue(ll_prologue, x.shape[1], x.shape[2]) if ll_prologue is not None else None
    check(lib.tmdiff_haar_dwt2d_pro(_chk(x, "x"), *ptrs, planes, hh_, ww, ll_scale, hi_scale, pro, stream_ptr()),
          "haar_dwt2d")
    return tuple(outs) + (None,) * (4 - len(outs))


def haar_idwt2d(lls, lh, hl, hh, in_scale=1.0, outs=None, stacked_bands=None, out0_prologue=None, pack_bf16=False):
    """lls: list of 1 or 2 low bands sharing the high bands; returns a list of reconstructions.
    ``stacked_bands`` [B, 3C, N, h, w] (the convH_0 output) supplies lh/hl/hh as channel slices
    without copying them out.  out0_prologue (lls[0] must then be [B, C, N, h, w]): the consumer convolution's prologue
    applied to the first reconstruction as it is written (see haar_dwt2d)."""
    ll0 = lls[0]
    h, w = ll0.shape[-2:]
    planes = ll0.numel() // (h * w)
    if pack_bf16:     # bf16 mode: first reconstruction as packed bf16 units, second one fp32; stacked bands only
        if len(lls) != 2 or stacked_bands is None:
            raise ValueError("haar_idwt2d(pack_bf16=True) takes two low bands and stacked high bands")
        b, c, n = ll0.shape[:3]
        units = torch.empty(b, c // 8, n * 4 * h * w, 8, device=ll0.device, dtype=torch.int16)
        out1 = torch.empty(b, c, n, 2 * h, 2 * w, device=ll0.device, dtype=torch.float32)
        pro = _plane_prologue(out0_prologue, c, n) if out0_prologue is not None else None
        check(lib.tmdiff_haar_idwt2d_pack_bf16(_chk(ll0, "ll0"), _chk(lls[1], "ll1"), _chk(stacked_bands, "bands"),
                                               units.data_ptr(), out1.data_ptr(), b, c, n, h, w, in_scale, pro, stream_ptr()),
              "haar_idwt2d_pack_bf16")
        return [units, out1]
    if outs is None:
        outs = [torch.empty((*ll0.shape[:-2], 2 * h, 2 * w), device=ll0.device, dtype=torch.float32) for _ in lls]
    llp = (C.c_void_p * 2)(*[_chk(t, "ll") for t in lls], *([None] * (2 - len(lls))))
    outp = (C.c_void_p * 2)(*[_chk(t, "out") for t in outs], *([None] * (2 - len(outs))))
    if stacked_bands is not None:
        b = stacked_bands.shape[0]
        ppb = planes // b
        if stacked_bands.numel() != 3 * planes * h * w:
            raise ValueError("haar_idwt2d: stacked bands must be [B, 3C, N, h, w]")
        base = _chk(stacked_bands, "bands")
        step = 4 * ppb * h * w
        hp = (base, base + step, base + 2 * step, ppb, 3 * ppb * h * w)
    else:
        hp = (_chk(lh, "lh"), _chk(hl, "hl"), _chk(hh, "hh"), 0, 0)
    pro = _plane_prologue(out0_prologue, ll0.shape[1], ll0.shape[2]) if out0_prologue is not None else None
    check(lib.tmdiff_haar_idwt2d_pro(llp, len(lls), *hp, outp, planes, h, w, in_scale, pro, stream_ptr()), "haar_idwt2d")
    return outs


def linear(x, w, bias=None, act=False, out=None):
    b, i = x.shape
    o = w.shape[0]
    y = out if out is not None else torch.empty(b, o, device=x.device, dtype=torch.float32)
    check(lib.tmdiff_linear_fwd(_chk(x, "x"), _chk(w, "w"), _chk(bias, "bias"), _chk(y, "y"), b, i, o,
                                1 if act else 0, stream_ptr()), "linear_fwd")
    return y


def gamma_embedding(t, freqs, dim, out=None):
    b = t.shape[0]
    y = out if out is not None else torch.empty(b, dim, device=t.device, dtype=torch.float32)
    check(lib.tmdiff_gamma_embedding(_chk(t, "t"), _chk(freqs, "freqs"), _chk(y, "emb"), b, dim, stream_ptr()),
          "gamma_embedding")
    return y


def ddpm_step(x, eps, noise, c_recip, c_recipm1, coef1, coef2, sigma, clip=True, ms=None, out=None, img_out=None):
    y = out if out is not None else torch.empty_like(x)
    check(lib.tmdiff_ddpm_step(_chk(x, "x"), _chk(eps, "eps"), _chk(noise, "noise"), _chk(ms, "ms"), _chk(y, "out"),
                               _chk(img_out, "img_out"), x.numel(), c_recip, c_recipm1, coef1, coef2, sigma,
                               1 if clip else 0, stream_ptr()), "ddpm_step")
    return y


def ddpm_step_dev(x, eps, noise, step, coef, ms=None, out=None, frames=None, frame_every=1, clip=True):
    """ddpm_step with the timestep and its coefficients read on the device: t = step[0] (int32), coefficients = row t of
    coef [T, 5] (fp32).  ``out`` may be ``x`` (in-place).  frames: [slots, *x.shape] stack written at t % frame_every == 0."""
    y = out if out is not None else torch.empty_like(x)
    if step.dtype != torch.int32 or not step.is_cuda or coef.dim() != 2 or coef.shape[1] != 5:
        raise ValueError("ddpm_step_dev: step must be an int32 device word and coef a [T, 5] table")
    check(lib.tmdiff_ddpm_step_dev(_chk(x, "x"), _chk(eps, "eps"), _chk(noise, "noise"), _chk(ms, "ms"), _chk(y, "out"),
                                   _chk(frames, "frames"), x.numel(), step.data_ptr(), _chk(coef, "coef"), coef.shape[0],
                                   frame_every, 1 if clip else 0, stream_ptr()), "ddpm_step_dev")
    return y


def sampler_tick(step, time_in, set_to=-1):
    """step[0] = set_to (>= 0) or step[0] - 1; then time_in[:] = step[0] + 1 (fp32), on the device.  time_in may be None
    (no time input to write: only the step word moves)."""
    if step.dtype != torch.int32 or not step.is_cuda:
        raise ValueError("sampler_tick: step must be an int32 device word")
    check(lib.tmdiff_sampler_tick(step.data_ptr(), _chk(time_in, "time_in"), 0 if time_in is None else time_in.numel(),
                                  int(set_to), stream_ptr()), "sampler_tick")


def axpby(tensors, coefs, out=None):
    n_in = len(tensors)
    y = out if out is not None else torch.empty_like(tensors[0])
    ptrs = (C.c_void_p * 4)(*[_chk(t, "in") for t in tensors], *([None] * (4 - n_in)))
    cf = (C.c_float * 4)(*[float(c) for c in coefs], *([0.0] * (4 - n_in)))
    check(lib.tmdiff_axpby(ptrs, cf, n_in, _chk(y, "out"), y.numel(), stream_ptr()), "axpby")
    return y


def chunk_tables(rows, sizes, device, pinned):
    """The device tables of the multi-tensor kernels (tmdiff_multi_axpby, tmdiff_multi_adamw, tmdiff_multi_sqnorm_partial): per tensor
    one row of int64 (its pointers, then its element count: tmdiff_mt_entry / tmdiff_adamw_entry), and per chunk of
    tmdiff_multi_axpby_chunk() elements its tensor and its index within that tensor (int32).  ``pinned``: pinned host tensors,
    returned last for the caller to keep alive, and non-blocking uploads -- legal inside a HIP-graph capture, whose replay copies
    the same bytes again; else plain copies.  Returns (entries, chunk_tensor, chunk_index, n_chunks, host or None)."""
    chunk = lib.tmdiff_multi_axpby_chunk()
    ct, ci = [], []
    for k, n in enumerate(sizes):
        nck = (n + chunk - 1) // chunk
        ct += [k] * nck
        ci += list(range(nck))
    host = [torch.tensor([v for row in rows for v in row], dtype=torch.int64), torch.tensor(ct, dtype=torch.int32),
            torch.tensor(ci, dtype=torch.int32)]
    if pinned:
        host = [h.pin_memory() for h in host]
    devt = [h.to(device, non_blocking=pinned) for h in host]
    return devt[0], devt[1], devt[2], len(ct), host if pinned else None


class MultiAxpby:
    """out_t = ca * a_t + cb * b_t over a fixed list of (out, a, b) tensor triples in ONE launch (tmdiff_multi_axpby).
    The device tables are built once from the tensors' addresses; ``stale()`` says whether they moved."""

    def __init__(self, triples):
        triples = [(o, a, b) for o, a, b in triples if o.numel() > 0]
        for o, a, b in triples:
            for t in (o, a, b):
                _chk(t, "multi_axpby tensor")
            if not (o.numel() == a.numel() == b.numel()):
                raise ValueError("multi_axpby: out / a / b sizes differ")
        if not triples:                    # nothing but empty tensors: no tables, run() launches nothing
            self.key, self.n_chunks, self._keep = (), 0, []
            self.entries = self.chunk_tensor = self.chunk_index = None
            return
        dev = triples[0][0].device
        self.key = tuple(t.data_ptr() for tr in triples for t in tr)
        self.entries, self.chunk_tensor, self.chunk_index, self.n_chunks, _ = chunk_tables(
            [(o.data_ptr(), a.data_ptr(), b.data_ptr(), o.numel()) for o, a, b in triples], [o.numel() for o, _, _ in triples],
            dev, pinned=False)
        self._keep = triples

    def stale(self, triples):
        return self.key != tuple(t.data_ptr() for tr in triples for t in tr if tr[0].numel() > 0)

    def run(self, ca, cb):
        if self.n_chunks == 0:
            return
        check(lib.tmdiff_multi_axpby(self.entries.data_ptr(), self.chunk_tensor.data_ptr(), self.chunk_index.data_ptr(),
                                     self.n_chunks, float(ca), float(cb), stream_ptr()), "multi_axpby")


def x0_from_model(x, model_out, alpha, sigma, model_is_x_start=True, out=None):
    y = out if out is not None else torch.empty_like(x)
    check(lib.tmdiff_x0_from_model(_chk(x, "x"), _chk(model_out, "model_out"), _chk(y, "x0"), x.numel(), alpha, sigma,
                                   1 if model_is_x_start else 0, stream_ptr()), "x0_from_model")
    return y


def abs_quantile_clamp_(x0, q=0.995, max_val=1.0):
    """In place: per sample s = max(quantile(|x0|, q), max_val); x0 = clamp(x0, -s, s) / s.  Returns s [B]."""
    b = x0.shape[0]
    n = x0.numel() // b
    ws = torch.empty(max(1, lib.tmdiff_abs_quantile_workspace_bytes(b, n) // 4), device=x0.device, dtype=torch.float32)
    check(lib.tmdiff_abs_quantile_clamp(_chk(x0, "x0"), b, n, q, max_val, ws.data_ptr(), stream_ptr()),
          "abs_quantile_clamp")
    return ws[:b]


def add(a, b, sign_b=1.0, out=None):
    y = out if out is not None else torch.empty_like(a)
    check(lib.tmdiff_add(_chk(a, "a"), _chk(b, "b"), _chk(y, "out"), a.numel(), sign_b, stream_ptr()), "add")
    return y


def q_sample(x0, noise, a, out=None):
    b = x0.shape[0]
    y = out if out is not None else torch.empty_like(x0)
    check(lib.tmdiff_q_sample(_chk(x0, "x0"), _chk(noise, "noise"), _chk(a, "a"), _chk(y, "out"), b,
                              x0.numel() // b, stream_ptr()), "q_sample")
    return y


# ---- overlapped scene tiles (csrc/tiles.hip; plan and blend weights: tmdiff_amd/tiling.py) ---------------------------
def _tile_grid(h, w, tile, overlap):
    ny, nx = (lib.tmdiff_tile_plan(int(n), int(tile), int(overlap), None, 0) for n in (h, w))
    if ny < 0 or nx < 0:
        raise ValueError(f"no tile plan for a {h} x {w} scene with tile={tile}, overlap={overlap}: need tile <= extent and "
                         f"0 <= overlap <= tile // 2")
    return ny, nx


def tile_supported(b, c, h, w, tile, overlap):
    """True when tile_gather / tile_blend take these extents (a valid plan whose 32-bit element offsets fit)."""
    return bool(lib.tmdiff_tile_supported(b, c, h, w, tile, overlap))


def tile_gather(scene, tile, overlap, out=None):
    """scene [B, C, H, W] -> tiles [B * ny * nx, C, tile, tile], row-major per sample."""
    if scene.dim() != 4:
        raise ValueError(f"scene: need [B, C, H, W], got {tuple(scene.shape)}")
    b, c, h, w = scene.shape
    ny, nx = _tile_grid(h, w, tile, overlap)
    shape = (b * ny * nx, c, tile, tile)
    y = out if out is not None else torch.empty(shape, device=scene.device, dtype=torch.float32)
    if tuple(y.shape) != shape:
        raise ValueError(f"tiles: need {shape}, got {tuple(y.shape)}")
    check(lib.tmdiff_tile_gather(_chk(scene, "scene"), _chk(y, "tiles"), b, c, h, w, tile, overlap, stream_ptr()), "tile_gather")
    return y


def tile_blend(tiles, batch, h, w, overlap, out=None):
    """tiles [batch * ny * nx, C, tile, tile] -> scene [batch, C, h, w]: the weighted mean over the covering tiles."""
    if tiles.dim() != 4 or tiles.shape[2] != tiles.shape[3]:
        raise ValueError(f"tiles: need [N, C, tile, tile], got {tuple(tiles.shape)}")
    n, c, tile, _ = tiles.shape
    ny, nx = _tile_grid(h, w, tile, overlap)
    if n != batch * ny * nx:
        raise ValueError(f"tiles: {n} tiles, the plan has {batch} x {ny} x {nx}")
    shape = (batch, c, h, w)
    y = out if out is not None else torch.empty(shape, device=tiles.device, dtype=torch.float32)
    if tuple(y.shape) != shape:
        raise ValueError(f"scene: need {shape}, got {tuple(y.shape)}")
    check(lib.tmdiff_tile_blend(_chk(tiles, "tiles"), _chk(y, "scene"), batch, c, h, w, tile, overlap, stream_ptr()), "tile_blend")
    return y


# ---- quality metrics (csrc/metrics.hip; definitions and column order: tmdiff_amd/metrics.py) -------------------------
def metrics_supported(b, c, h, w):
    """True when metrics_pair / metrics_noref take a [b, c, h, w] image batch: 1 <= c <= 16, h, w >= 7, 32-bit offsets."""
    return bool(lib.tmdiff_metrics_supported(int(b), int(c), int(h), int(w)))


def metrics_workspace(b, c, h, w, device):
    """A workspace either metrics entry point accepts for [b, c, h, w] images (reusable; captured calls must keep it alive)."""
    return torch.empty(max(1, lib.tmdiff_metrics_workspace_bytes(b, c, h, w) // 8), device=device, dtype=torch.float64)


def _planes(t, name, c=None):
    """(pointer, batch stride, channel stride) of a float32 GPU tensor [B, C, H, W] whose rows and planes are dense."""
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 4):
        raise ValueError(f"{name}: need a float32 [B, C, H, W] tensor on the GPU")
    _, ch, h, w = t.shape
    sb, sc, sh, sw = t.stride()
    if c is not None and ch != c:
        raise ValueError(f"{name}: {ch} channels, need {c}")
    if (w > 1 and sw != 1) or (h > 1 and sh != w) or (ch > 1 and sc < h * w):
        raise ValueError(f"{name}: rows and planes must be dense (strides {t.stride()} for shape {tuple(t.shape)})")
    return t.data_ptr(), (sb if t.shape[0] > 1 else 0), (sc if ch > 1 else h * w)


def _f64(name, arg, t, shape, device, contiguous=True):
    """``t``, or with None a new tensor: a contiguous float64 tensor of ``shape`` on the GPU, the call's argument ``arg``.  A
    number as ``shape`` asks for that many elements in any shape."""
    count = isinstance(shape, int)
    y = t if t is not None else torch.empty(shape, device=device, dtype=torch.float64)
    if not (y.is_cuda and y.dtype == torch.float64 and (y.is_contiguous() or not contiguous)
            and (y.numel() == shape if count else tuple(y.shape) == tuple(shape))):
        raise ValueError(f"{name}: {arg} must be a {'contiguous ' if contiguous else ''}float64 {[shape] if count else list(shape)} "
                         f"tensor on the GPU")
    return y


def _lent(name, workspace, need, make):
    """(workspace, its bytes): the lent tensor, or with None ``make()``; on the GPU, contiguous, at least ``need`` bytes."""
    ws = workspace if workspace is not None else make()
    nbytes = ws.numel() * ws.element_size()
    if not (ws.is_cuda and ws.is_contiguous() and nbytes >= need):
        raise ValueError(f"{name}: workspace of {nbytes} bytes, need {need}")
    return ws, nbytes


def _grad_target(name, grad, like):
    """The tensor a loss writes its gradient to: True allocates one like ``like``, a tensor receives it, False or None selects the
    value-only mode (None)."""
    if grad is False or grad is None:
        return None
    g = torch.empty_like(like) if grad is True else grad
    if g.shape != like.shape:
        raise ValueError(f"{name}: g {tuple(g.shape)}, need {tuple(like.shape)}")
    return g


def _total32(name, total, device):
    """The one-element float32 tensor a loss writes its total to: ``total``, or with None a new scalar."""
    y32 = total if total is not None else torch.empty((), device=device, dtype=torch.float32)
    if y32.numel() != 1:
        raise ValueError(f"{name}: total must hold one float32")
    return y32


def _metrics_buffers(name, k, b, c, h, w, device, out, workspace):
    if not metrics_supported(b, c, h, w):
        raise ValueError(f"{name}: B={b} C={c} H={h} W={w} is not supported (1 <= C <= 16, H, W >= 7, fewer than 2^31 elements)")
    y = _f64(name, "out", out, (b, k), device)
    ws, nbytes = _lent(name, workspace, lib.tmdiff_metrics_workspace_bytes(b, c, h, w), lambda: metrics_workspace(b, c, h, w, device))
    return y, ws, nbytes


def metrics_pair(x_true, x_pred, data_range=1.0, ratio=0.25, out=None, workspace=None):
    """x_pred against x_true, both float32 [B, C, H, W]: float64 [B, 9] in the column order of metrics.PAIR_FIELDS."""
    if x_true.shape != x_pred.shape:
        raise ValueError(f"metrics_pair: shapes {tuple(x_true.shape)} and {tuple(x_pred.shape)} differ")
    pa, asb, asc = _planes(x_true, "x_true")
    pb, bsb, bsc = _planes(x_pred, "x_pred")
    b, c, h, w = x_true.shape
    y, ws, nbytes = _metrics_buffers("metrics_pair", 9, b, c, h, w, x_true.device, out, workspace)
    check(lib.tmdiff_metrics_pair(pa, asb, asc, pb, bsb, bsc, b, c, h, w, float(data_range), float(ratio), y.data_ptr(),
                                  ws.data_ptr(), nbytes, stream_ptr()), "metrics_pair")
    return y


def metrics_noref(l_ms, pan, l_pan, ps, out=None, workspace=None):
    """Full-resolution set of ps [B, C, H, W] and pan [B, 1, H, W] against l_ms [B, C, h, w] and l_pan [B, 1, h, w]: float64
    [B, 3] in the column order of metrics.NOREF_FIELDS."""
    pp, psb, psc = _planes(ps, "ps")
    b, c, h, w = ps.shape
    pl, lsb, lsc = _planes(l_ms, "l_ms", c)
    lh, lw = l_ms.shape[2:]
    pn, nsb, _ = _planes(pan, "pan", 1)
    pq, qsb, _ = _planes(l_pan, "l_pan", 1)
    if tuple(pan.shape) != (b, 1, h, w) or tuple(l_pan.shape) != (b, 1, lh, lw) or l_ms.shape[0] != b or lh < 1 or lw < 1:
        raise ValueError(f"metrics_noref: ps {tuple(ps.shape)}, pan {tuple(pan.shape)}, l_ms {tuple(l_ms.shape)}, "
                         f"l_pan {tuple(l_pan.shape)} do not belong together")
    y, ws, nbytes = _metrics_buffers("metrics_noref", 3, b, c, h, w, ps.device, out, workspace)
    check(lib.tmdiff_metrics_noref(pl, lsb, lsc, pn, nsb, pq, qsb, pp, psb, psc, b, c, h, w, lh, lw, y.data_ptr(), ws.data_ptr(),
                                   nbytes, stream_ptr()), "metrics_noref")
    return y


# ---- composite finetune loss (csrc/loss.hip; definition: tmdiff_amd/losses.py) ---------------------------------------
LOSS_BASE_KINDS = {"l1": 0, "l2": 1, "smooth_l1": 2}
_LOSS_LIMITS = "B >= 1, 1 <= C <= 16, H, W >= 3 with a Laplacian term and >= 1 without, fewer than 2^31 elements"


def loss_supported(b, c, h, w, lap=True):
    """True when spectral_spatial_loss takes [b, c, h, w] tensors (`lap`: with a Laplacian term)."""
    return bool(lib.tmdiff_loss_supported(int(b), int(c), int(h), int(w), int(bool(lap))))


def spectral_spatial_loss(x0, xhat, ms=None, base="l1", w_sam=0.0, w_lap=0.0, grad=True, terms=None, total=None, workspace=None):
    """base(xhat, x0) + w_sam * SAM(x0 + ms, xhat + ms) + w_lap * LAP(xhat - x0) of float32 [B, C, H, W] tensors, two launches.
    Returns (terms, total, g): terms float64 [4] = total, base, sam, lap (unweighted means; a term of weight 0 reports 0), total
    float32 [], and g = dL/dxhat (float32, the shape of xhat).  `grad`: True allocates g, a tensor receives it, False selects the
    value-only mode (g is None, nothing is written).  ms may be None only when w_sam == 0."""
    if base not in LOSS_BASE_KINDS:
        raise ValueError(f"spectral_spatial_loss: base {base!r}, need one of {sorted(LOSS_BASE_KINDS)}")
    w_sam, w_lap = float(w_sam), float(w_lap)
    if not (0.0 <= w_sam < float("inf") and 0.0 <= w_lap < float("inf")):
        raise ValueError(f"spectral_spatial_loss: weights must be finite and not negative, got w_sam={w_sam}, w_lap={w_lap}")
    if ms is None and w_sam != 0.0:
        raise ValueError("spectral_spatial_loss: ms is needed when w_sam != 0")
    if x0.dim() != 4 or x0.shape != xhat.shape or (ms is not None and ms.shape != x0.shape):
        raise ValueError(f"spectral_spatial_loss: need three [B, C, H, W] tensors of one shape, got {tuple(x0.shape)}, "
                         f"{tuple(xhat.shape)}, {None if ms is None else tuple(ms.shape)}")
    b, c, h, w = x0.shape
    lap = w_lap != 0.0
    if not loss_supported(b, c, h, w, lap):
        raise ValueError(f"spectral_spatial_loss: B={b} C={c} H={h} W={w} is not supported ({_LOSS_LIMITS})")
    px, ph, pm = _chk(x0, "x0"), _chk(xhat, "xhat"), _chk(ms, "ms")
    dev = x0.device
    g = _grad_target("spectral_spatial_loss", grad, xhat)
    y = _f64("spectral_spatial_loss", "terms", terms, 4, dev)
    y32 = _total32("spectral_spatial_loss", total, dev)
    need = lib.tmdiff_loss_workspace_bytes(b, c, h, w, int(lap))
    ws, nbytes = _lent("spectral_spatial_loss", workspace, need, lambda: _workspace(dev, need, "loss"))
    check(lib.tmdiff_spectral_spatial_loss(px, ph, pm, _chk(g, "g"), LOSS_BASE_KINDS[base], w_sam, w_lap, y.data_ptr(),
                                           _chk(y32, "total"), ws.data_ptr(), nbytes, b, c, h, w, stream_ptr()),
          "spectral_spatial_loss")
    _count("spectral_spatial_loss")
    return y, y32, g


# ---- SSIM loss term (csrc/ssim_loss.hip; definition: tmdiff_amd/losses.py ssim_loss_host) ------------------------------
_SSIM_LIMITS = "B, C >= 1, win odd with 3 <= win <= 11, H, W >= win, fewer than 2^31 elements"


def ssim_loss_supported(b, c, h, w, win=7):
    """True when ssim_loss takes [b, c, h, w] tensors with a win x win window."""
    return bool(lib.tmdiff_ssim_loss_supported(int(b), int(c), int(h), int(w), int(win)))


def ssim_loss(x_true, x_pred, win=7, data_range=1.0, weight=1.0, grad=True, accumulate=False, terms_in=None, out=None, total=None,
              workspace=None, ms=None):
    """dssim = 1 - SSIM(x_true, x_pred) of float32 [B, C, H, W] tensors over uniform win x win windows, two launches.  Returns
    (out, total32, g).  Without `terms_in`: out float64 [2] = dssim, ssim and total32 the float32 of weight * dssim.  With
    `terms_in` (the float64 [4] of spectral_spatial_loss): out float64 [5] = terms_in[0] + weight * dssim, base, sam, lap, dssim
    and total32 the float32 of entry 0.  g = weight * d dssim / d x_pred (float32, the shape of x_pred).  `grad`: True allocates g,
    a tensor receives it, False selects the value-only mode (g is None, nothing is written).  `accumulate` adds the gradient to
    the tensor given as `grad`.  `ms` (optional): the kernel scores x_true + ms against x_pred + ms, summed in fp64."""
    win, data_range, weight = int(win), float(data_range), float(weight)
    if not 0.0 < data_range < float("inf"):
        raise ValueError(f"ssim_loss: data_range must be finite and > 0, got {data_range}")
    if not 0.0 <= weight < float("inf"):
        raise ValueError(f"ssim_loss: weight must be finite and not negative, got {weight}")
    if x_true.dim() != 4 or x_true.shape != x_pred.shape or (ms is not None and ms.shape != x_true.shape):
        raise ValueError(f"ssim_loss: need [B, C, H, W] tensors of one shape, got {tuple(x_true.shape)}, {tuple(x_pred.shape)}, "
                         f"{None if ms is None else tuple(ms.shape)}")
    b, c, h, w = x_true.shape
    if not ssim_loss_supported(b, c, h, w, win):
        raise ValueError(f"ssim_loss: B={b} C={c} H={h} W={w} win={win} is not supported ({_SSIM_LIMITS})")
    if accumulate and not torch.is_tensor(grad):
        raise ValueError("ssim_loss: accumulate=True needs the gradient tensor to add to as `grad`")
    pa, pb, pm = _chk(x_true, "x_true"), _chk(x_pred, "x_pred"), _chk(ms, "ms")
    dev = x_true.device
    g = _grad_target("ssim_loss", grad, x_pred)
    if terms_in is not None:
        _f64("ssim_loss", "terms_in", terms_in, 4, dev)
    y = _f64("ssim_loss", "out", out, 2 if terms_in is None else 5, dev)
    y32 = _total32("ssim_loss", total, dev)
    need = lib.tmdiff_ssim_loss_workspace_bytes(b, c, h, w, win)
    ws, nbytes = _lent("ssim_loss", workspace, need, lambda: _workspace(dev, need, "ssim_loss"))
    check(lib.tmdiff_ssim_loss(pa, pb, pm, _chk(g, "g"), win, data_range, weight, int(bool(accumulate)),
                               None if terms_in is None else terms_in.data_ptr(), y.data_ptr(), _chk(y32, "total"),
                               ws.data_ptr(), nbytes, b, c, h, w, stream_ptr()), "ssim_loss")
    _count("ssim_loss")
    return y, y32, g


# ---- local PAN-correlation loss (csrc/local_corr.hip; definition: tmdiff_amd/metrics.py local_corr_loss) ----------------
_LCORR_LIMITS = "B >= 1, 1 <= C <= 16, 2 <= win <= 8, H, W >= win, fewer than 2^31 elements"
LOCAL_CORR_TILE = (16, 32)     # rows x columns of the kernel's tile (TH, TW of csrc/local_corr.hip), for every window size
_LCORR_RHO_MAX = {}            # (values, device) -> the uploaded float64 [C] table; the last _LCORR_RHO_MAX_TABLES, oldest dropped first
_LCORR_RHO_MAX_TABLES = 8


def local_corr_loss_supported(b, c, h, w, win=4):
    """True when local_corr_loss takes x [b, c, h, w] with a win x win window."""
    return bool(lib.tmdiff_local_corr_loss_supported(int(b), int(c), int(h), int(w), int(win)))


def _rho_max_table(rho_max, c, device):
    """None, or the float64 [C] device table of ``rho_max`` (a number or C numbers), made once per (values, device): call once
    before capturing.  The cache keeps the last few tables, so sweeping ``rho_max`` does not pile up device memory; as with the
    scaled tap tables of ``_mtf_taps``, a captured graph reads the table it recorded, so more than _LCORR_RHO_MAX_TABLES other
    values must not pass through here between its capture and its last replay."""
    if rho_max is None:
        return None
    vals = tuple(float(v) for v in rho_max) if isinstance(rho_max, (list, tuple)) or hasattr(rho_max, "__len__") else (float(rho_max),)
    vals = vals * c if len(vals) == 1 else vals
    if len(vals) != c or not all(v == v and abs(v) < float("inf") for v in vals):
        raise ValueError(f"local_corr_loss: rho_max={rho_max!r} (None, a finite number, or one per band: {c})")
    key = (vals, device)
    if key not in _LCORR_RHO_MAX:
        _LCORR_RHO_MAX[key] = torch.tensor(vals, dtype=torch.float64).to(device)
        while len(_LCORR_RHO_MAX) > _LCORR_RHO_MAX_TABLES:
            del _LCORR_RHO_MAX[next(iter(_LCORR_RHO_MAX))]          # dicts keep insertion order: the oldest
    return _LCORR_RHO_MAX[key]


def local_corr_loss(x, pan, win=4, rho_max=None, weight=1.0, grad=True, accumulate=False, out=None, per_image=None, total=None,
                    workspace=None):
    """The mean over b, c and all win x win windows ('valid', stride 1) of max(0, rho_max_c - rho), rho the correlation
    coefficient of band c of x [B, C, H, W] with pan [B, 1, H, W] inside the window (float32 on the GPU; definition:
    ``metrics.local_corr_loss``), two launches.  Returns (out, total32, g): out float64 [2] = loss, mean rho; total32 the
    float32 of weight * loss; g = weight * d loss / d x (float32, the shape of x; the PAN gets none).  ``rho_max``: None (1.0), a
    number or C numbers, kept on the device as a cached float64 table.  ``grad``: True allocates g, a tensor receives it, False
    selects the value-only mode (g is None, nothing is written).  ``accumulate`` adds the gradient to the tensor given as
    ``grad``.  ``per_image``: a float64 [B] tensor that receives each image's mean rho (1 - D_rho)."""
    win, weight = int(win), float(weight)
    if not 0.0 <= weight < float("inf"):
        raise ValueError(f"local_corr_loss: weight must be finite and not negative, got {weight}")
    if x.dim() != 4 or pan.dim() != 4 or tuple(pan.shape) != (x.shape[0], 1, *x.shape[2:]):
        raise ValueError(f"local_corr_loss: need x [B, C, H, W] and pan [B, 1, H, W], got {tuple(x.shape)}, {tuple(pan.shape)}")
    b, c, h, w = x.shape
    if not local_corr_loss_supported(b, c, h, w, win):
        raise ValueError(f"local_corr_loss: B={b} C={c} H={h} W={w} win={win} is not supported ({_LCORR_LIMITS})")
    if accumulate and not torch.is_tensor(grad):
        raise ValueError("local_corr_loss: accumulate=True needs the gradient tensor to add to as `grad`")
    px, pp = _chk(x, "x"), _chk(pan, "pan")
    dev = x.device
    table = _rho_max_table(rho_max, c, dev)
    g = _grad_target("local_corr_loss", grad, x)
    y = _f64("local_corr_loss", "out", out, 2, dev)
    if per_image is not None:
        _f64("local_corr_loss", "per_image", per_image, (b,), dev)
    y32 = _total32("local_corr_loss", total, dev)
    need = lib.tmdiff_local_corr_loss_workspace_bytes(b, c, h, w, win)
    ws, nbytes = _lent("local_corr_loss", workspace, need, lambda: _workspace(dev, need, "local_corr_loss"))
    check(lib.tmdiff_local_corr_loss(px, pp, _chk(g, "g"), None if table is None else table.data_ptr(), win, weight,
                                     int(bool(accumulate)), y.data_ptr(), None if per_image is None else per_image.data_ptr(),
                                     _chk(y32, "total"), ws.data_ptr(), nbytes, b, c, h, w, stream_ptr()), "local_corr_loss")
    _count("local_corr_loss")
    return y, y32, g


_Q2N_LIMITS = "1 <= C <= 16, block 8, 16 or 32, 1 <= shift <= block, mirror padding no longer than the axis, fewer than 2^31 elements"


def q2n_grid(h, w, block=32, shift=32):
    """(ny, nx) of the windows of metrics_q2n: ceil(h / shift), ceil(w / shift)."""
    if shift < 1:
        raise ValueError(f"q2n_grid: shift={shift} ({_Q2N_LIMITS})")
    return -(-int(h) // int(shift)), -(-int(w) // int(shift))


def metrics_q2n_supported(b, c, h, w, block=32, shift=32):
    """True when metrics_q2n takes a [b, c, h, w] image batch with these windows."""
    return bool(lib.tmdiff_metrics_q2n_supported(int(b), int(c), int(h), int(w), int(block), int(shift)))


def metrics_q2n_workspace(b, c, h, w, device, block=32, shift=32):
    """A workspace metrics_q2n accepts for [b, c, h, w] images (reusable; captured calls must keep it alive)."""
    nbytes = lib.tmdiff_metrics_q2n_workspace_bytes(int(b), int(c), int(h), int(w), int(block), int(shift))
    return torch.empty(max(1, nbytes // 8), device=device, dtype=torch.float64)


def metrics_q2n(x_true, x_pred, block=32, shift=32, out=None, map_out=None, workspace=None):
    """Q2n (Q4 / Q8; definition: ``metrics.q2n``) of x_pred against x_true, both float32 [B, C, H, W]: float64 [B].  ``map_out``,
    a float64 [B, ny, nx] tensor (``q2n_grid``), receives the windows' values."""
    if x_true.shape != x_pred.shape:
        raise ValueError(f"metrics_q2n: shapes {tuple(x_true.shape)} and {tuple(x_pred.shape)} differ")
    pa, asb, asc = _planes(x_true, "x_true")
    pb, bsb, bsc = _planes(x_pred, "x_pred")
    b, c, h, w = x_true.shape
    block, shift = int(block), int(shift)
    if not metrics_q2n_supported(b, c, h, w, block, shift):
        raise ValueError(f"metrics_q2n: B={b} C={c} H={h} W={w} block={block} shift={shift} is not supported ({_Q2N_LIMITS})")
    ny, nx = q2n_grid(h, w, block, shift)
    dev = x_true.device
    y = _f64("metrics_q2n", "out", out, (b,), dev)
    if map_out is not None:
        _f64("metrics_q2n", "map_out", map_out, (b, ny, nx), dev)
    ws, nbytes = _lent("metrics_q2n", workspace, lib.tmdiff_metrics_q2n_workspace_bytes(b, c, h, w, block, shift),
                       lambda: metrics_q2n_workspace(b, c, h, w, dev, block, shift))
    check(lib.tmdiff_metrics_q2n(pa, asb, asc, pb, bsb, bsc, b, c, h, w, block, shift, y.data_ptr(),
                                 map_out.data_ptr() if map_out is not None else None, ws.data_ptr(), nbytes, stream_ptr()),
          "metrics_q2n")
    return y


# ---- resampling of full-resolution scenes (csrc/resample.hip; definitions: tmdiff_amd/metrics.py) --------------------
def _resample_args(name, x, shape_of, out, limits):
    """(x pointer, y, y pointer) of a resampling call: x float32 [B, C, H, W] on the GPU, contiguous, fewer than 2^31 elements
    either side; ``shape_of(h, w)`` is the output's (H', W') or None when the extents are not taken."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous()):
        raise ValueError(f"{name}: need a contiguous float32 [B, C, H, W] tensor on the GPU ({limits})")
    b, c, h, w = x.shape
    hw = shape_of(h, w)
    if hw is None or max(x.numel(), b * c * hw[0] * hw[1]) > 2 ** 31 - 1:
        raise ValueError(f"{name}: shape {tuple(x.shape)} is not supported ({limits})")
    shape = (b, c, *hw)
    y = out if out is not None else torch.empty(shape, device=x.device, dtype=torch.float32)
    if tuple(y.shape) != shape:
        raise ValueError(f"{name}: out must be {shape}, got {tuple(y.shape)}")
    return x.data_ptr(), y, _chk(y, "out")


def pyr_down_shape(h, w, levels=2):
    """(H', W') of ``pyr_down``: (L + 1) // 2 per axis and level."""
    for _ in range(levels):
        h, w = (h + 1) // 2, (w + 1) // 2
    return h, w


def pyr_down(x, levels=2, out=None):
    """``levels`` (1 or 2) steps of OpenCV's pyrDown on x [B, C, H, W]: [1 4 6 4 1] / 16 along both axes, reflect-101 border,
    every second pixel -> [B, C, H', W'] with L' = (L + 1) // 2 per level.  Two levels are one kernel and equal two one-level
    calls bit for bit.  With ``out=`` nothing is allocated or synchronised (graph capture)."""
    limits = "levels 1 or 2; H, W >= 3 for one level, >= 5 for two; fewer than 2^31 elements"
    if levels not in (1, 2):
        raise ValueError(f"pyr_down: levels={levels} ({limits})")
    least = 5 if levels == 2 else 3
    px, y, py = _resample_args("pyr_down", x, lambda h, w: pyr_down_shape(h, w, levels) if min(h, w) >= least else None, out, limits)
    b, c, h, w = x.shape
    check(lib.tmdiff_pyr_down(px, py, b * c, h, w, levels, stream_ptr()), "pyr_down")
    return y


def upsample_bilinear(x, ratio=4, out=None):
    """x [B, C, h, w] -> [B, C, ratio * h, ratio * w], ratio 2 or 4: bilinear with half-pixel centres and a clamped edge
    (cv2.resize(INTER_LINEAR), F.interpolate(mode="bilinear", align_corners=False)).  With ``out=`` nothing is allocated or
    synchronised (graph capture)."""
    limits = "ratio 2 or 4; fewer than 2^31 output elements"
    if ratio not in (2, 4):
        raise ValueError(f"upsample_bilinear: ratio={ratio} ({limits})")
    px, y, py = _resample_args("upsample_bilinear", x, lambda h, w: (ratio * h, ratio * w) if min(h, w) >= 1 else None, out, limits)
    b, c, h, w = x.shape
    check(lib.tmdiff_upsample_bilinear(px, py, b * c, h, w, ratio, stream_ptr()), "upsample_bilinear")
    return y


def upsample_poly23(x, ratio=4, out=None, phase=1):
    """x [B, C, h, w] -> [B, C, ratio * h, ratio * w], ratio 2 or 4: the Pansharpening Toolbox's interp23tap, which makes the
    ``lms`` of the PanCollection files (definition: ``metrics.upsample_poly23``).  Per x2 stage the 23-tap half-band polynomial
    kernel with circular borders, along H then W; ``phase`` 1 puts the samples at the odd outputs, 0 at the even ones.  Ratio 4
    is a phase-1 stage followed by a phase-0 stage in one kernel, bit for bit the two calls: ``y[..., 2::4, 2::4] == x``;
    ``phase`` must be 1 there.  With ``out=`` nothing is allocated or synchronised (graph capture)."""
    limits = "ratio 2 or 4; phase 0 or 1, 1 at ratio 4; fewer than 2^31 output elements"
    if ratio not in (2, 4) or phase not in (0, 1) or (ratio == 4 and phase != 1):
        raise ValueError(f"upsample_poly23: ratio={ratio} phase={phase} ({limits})")
    px, y, py = _resample_args("upsample_poly23", x, lambda h, w: (ratio * h, ratio * w) if min(h, w) >= 1 else None, out, limits)
    b, c, h, w = x.shape
    check(lib.tmdiff_upsample_poly23(px, py, b * c, h, w, ratio, phase, stream_ptr()), "upsample_poly23")
    return y


# ---- MTF-matched filtering and decimation (csrc/mtf.hip; definitions: tmdiff_amd/metrics.py) -------------------------
_FIR_LIMITS = "taps float32 [T, K, K] on the GPU, K odd and at most 41, T a divisor of B * C; ratio 1, 2 or 4; 0 <= offset < ratio"
_MTF_TAPS = {}          # (gains, ratio, device) -> the uploaded [bands, 41, 41] table
_MTF_STEP_TAPS = {}     # (gains, ratio, device, scales) -> a scaled copy; the last _MTF_STEP_TAPS_MAX of them, oldest dropped first
_MTF_STEP_TAPS_MAX = 8


def fir_decimate_shape(h, w, ratio=1, offset=None):
    """(H', W') of ``fir_decimate``: ceil((L - o) / ratio) per axis; ``offset`` None is ratio // 2 on both axes."""
    from .metrics import fir_decimate_shape as shape_of
    return shape_of(h, w, ratio, offset)[0]


def fir_decimate(x, taps, ratio=1, offset=None, out=None):
    """FIR filtering with decimation of x [B, C, H, W] (definition: ``metrics.fir_decimate``): plane p is correlated with
    taps[p % T] ([T, K, K], or [K, K] for one table), the border replicated, and sampled at ``offset`` + ratio * i -> [B, C,
    ceil((H - oy) / ratio), ceil((W - ox) / ratio)].  ``offset`` None is ratio // 2 on both axes, where ``upsample_poly23`` puts
    the samples; a number serves both axes.  Only the kept samples are computed.  With ``out=`` nothing is allocated or
    synchronised (graph capture).  Differentiable in x: with grad mode on and ``x.requires_grad`` the result carries a backward
    that is the adjoint kernel (``fir_decimate_adjoint``); the taps get no gradient and ``out=`` is refused.  Otherwise the call
    is the plain one."""
    from .metrics import fir_decimate_shape as shape_of
    if torch.is_tensor(x) and x.requires_grad and torch.is_grad_enabled():
        # differentiable in x: the backward is the adjoint kernel (autograd.FirDecimateFn); no gradient flows to the taps
        if out is not None:
            raise ValueError("fir_decimate: out= cannot be given for an input that requires grad (the result joins the autograd graph)")
        from .autograd import FirDecimateFn
        return FirDecimateFn.apply(x, taps, ratio, offset)
    t, k, (oy, ox) = _fir_taps("fir_decimate", taps, ratio, offset)
    px, y, py = _resample_args("fir_decimate", x, lambda h, w: shape_of(h, w, ratio, offset)[0], out, _FIR_LIMITS)
    b, c, h, w = x.shape
    if (b * c) % t or taps.device != x.device:
        raise ValueError(f"fir_decimate: taps {tuple(taps.shape)} on {taps.device} for {b * c} planes on {x.device} ({_FIR_LIMITS})")
    check(lib.tmdiff_fir_decimate(px, taps.data_ptr(), py, b * c, t, h, w, k, ratio, oy, ox, stream_ptr()), "fir_decimate")
    return y


def _fir_taps(name, taps, ratio, offset):
    """(T, K, (oy, ox)) of a FIR call after the checks that do not need the image."""
    from .metrics import fir_decimate_shape as shape_of
    if ratio not in (1, 2, 4):
        raise ValueError(f"{name}: ratio={ratio} ({_FIR_LIMITS})")
    if not (torch.is_tensor(taps) and taps.is_cuda and taps.dtype == torch.float32 and taps.dim() in (2, 3) and taps.is_contiguous()):
        raise ValueError(f"{name}: bad taps ({_FIR_LIMITS})")
    t, k = (1 if taps.dim() == 2 else taps.shape[0]), taps.shape[-1]
    if taps.shape[-2] != k or k % 2 == 0 or k > 41 or t < 1:
        raise ValueError(f"{name}: taps {tuple(taps.shape)} ({_FIR_LIMITS})")
    return t, k, shape_of(1, 1, ratio, offset)[1]


def fir_decimate_adjoint(g, taps, shape, ratio=1, offset=None, out=None, base=None, alpha=1.0, beta=0.0):
    """``beta * base + alpha * A^T g`` for A = ``fir_decimate(., taps, ratio, offset)`` on [B, C, H, W] images with ``shape`` =
    (H, W) (definition: ``metrics.fir_decimate_adjoint``): g [B, C, H', W'] with (H', W') = ``fir_decimate_shape(H, W, ratio,
    offset)`` -> [B, C, H, W], the exact transpose, the replicated border included.  ``base`` [B, C, H, W] is needed when
    ``beta != 0``, is not read when ``beta == 0``, and may be ``out`` itself; ``out`` must not overlap ``g`` or ``taps`` (other
    tiles still read them).  One kernel, a gather without atomics: the same bits on every run.  With ``out=`` nothing is
    allocated or synchronised (graph capture)."""
    from .metrics import fir_decimate_shape as shape_of
    name = "fir_decimate_adjoint"
    t, k, (oy, ox) = _fir_taps(name, taps, ratio, offset)
    h, w = (int(n) for n in shape)
    if h < 1 or w < 1:
        raise ValueError(f"{name}: shape {(h, w)} (extents >= 1)")
    if not (torch.is_tensor(g) and g.is_cuda and g.dtype == torch.float32 and g.dim() == 4 and g.is_contiguous()):
        raise ValueError(f"{name}: need a contiguous float32 [B, C, H', W'] tensor on the GPU ({_FIR_LIMITS})")
    b, c = g.shape[:2]
    if tuple(g.shape[2:]) != shape_of(h, w, ratio, offset)[0]:
        raise ValueError(f"{name}: g {tuple(g.shape)} is not [B, C, {shape_of(h, w, ratio, offset)[0]}], the extent of fir_decimate "
                         f"on {h} x {w} at ratio {ratio}, offset ({oy}, {ox})")
    if b * c * h * w > 2 ** 31 - 1:
        raise ValueError(f"{name}: shape {(b, c, h, w)} is not supported ({_FIR_LIMITS}; fewer than 2^31 elements)")
    if (b * c) % t or taps.device != g.device:
        raise ValueError(f"{name}: taps {tuple(taps.shape)} on {taps.device} for {b * c} planes on {g.device} ({_FIR_LIMITS})")
    full = (b, c, h, w)
    y = out if out is not None else torch.empty(full, device=g.device, dtype=torch.float32)
    if tuple(y.shape) != full:
        raise ValueError(f"{name}: out must be {full}, got {tuple(y.shape)}")
    for other, what in ((g, "g"), (taps, "taps")):
        lo, hi = other.data_ptr(), other.data_ptr() + 4 * other.numel()
        if y.data_ptr() < hi and lo < y.data_ptr() + 4 * y.numel():
            raise ValueError(f"{name}: out overlaps {what}")
    alpha, beta = float(alpha), float(beta)
    if beta != 0.0 and (base is None or tuple(base.shape) != full):
        raise ValueError(f"{name}: beta={beta} needs base of shape {full}")
    pb = _chk(base, "base") if beta != 0.0 else None
    check(lib.tmdiff_fir_decimate_adjoint(g.data_ptr(), taps.data_ptr(), pb, _chk(y, "out"), alpha, beta, b * c, t, h, w, k, ratio,
                                          oy, ox, stream_ptr()), name)
    return y


def mtf_degrade(x, gains_or_sensor, ratio=4, pan=False, out=None):
    """Wald's degradation of x [B, C, H, W] (definition: ``metrics.mtf_degrade``): band c low-passed with the 41 x 41 MTF-matched
    filter of its Nyquist gain and decimated by ``ratio`` at the offset ratio // 2 -> [B, C, ceil((H - o) / ratio), ...].
    ``gains_or_sensor``: a sensor name (``metrics.mtf_gains``; with ``pan`` its PAN gain, for a one-band image), one gain per
    band, or a number for every band.  The tap table is made on the host once per (gains, ratio, device) and kept on the
    device: call once before capturing into a graph.  Differentiable in x as ``fir_decimate`` is."""
    from . import metrics
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 4):
        raise ValueError(f"mtf_degrade: need a float32 [B, C, H, W] tensor on the GPU ({_FIR_LIMITS})")
    if ratio not in (1, 2, 4):
        raise ValueError(f"mtf_degrade: ratio={ratio} ({_FIR_LIMITS})")
    gains = metrics.band_gains(gains_or_sensor, x.shape[1], pan)
    return fir_decimate(x, _mtf_taps(gains, ratio, x.device), ratio, None, out)


def mtf_degrade_adjoint(g, gains_or_sensor, shape, ratio=4, pan=False, out=None, base=None, alpha=1.0, beta=0.0):
    """``beta * base + alpha * A^T g`` for A = ``mtf_degrade(., gains_or_sensor, ratio, pan)`` on [B, C, H, W] images with
    ``shape`` = (H, W) (definition: ``metrics.mtf_degrade_adjoint``): g [B, C, H', W'] -> [B, C, H, W] through
    ``fir_decimate_adjoint`` with the cached tap table of ``mtf_degrade``: call once before capturing into a graph."""
    from . import metrics
    if not (torch.is_tensor(g) and g.is_cuda and g.dim() == 4):
        raise ValueError(f"mtf_degrade_adjoint: need a float32 [B, C, H', W'] tensor on the GPU ({_FIR_LIMITS})")
    if ratio not in (1, 2, 4):
        raise ValueError(f"mtf_degrade_adjoint: ratio={ratio} ({_FIR_LIMITS})")
    gains = metrics.band_gains(gains_or_sensor, g.shape[1], pan)
    return fir_decimate_adjoint(g, _mtf_taps(gains, ratio, g.device), shape, ratio, None, out, base, alpha, beta)


def _mtf_taps(gains, ratio, device, scales=None):
    """The [bands, 41, 41] float32 table of ``metrics.mtf_kernel`` on the device, made once per (gains, ratio, device).
    ``scales``: a factor per band, applied in float64 before the rounding (the per-band step of ``tiling.consistency_refine``);
    such tables live in a cache of their own that keeps the last few, so sweeping ``relax`` does not pile up device memory."""
    from . import metrics
    cache = _MTF_TAPS if scales is None else _MTF_STEP_TAPS
    key = (tuple(gains), ratio, device) if scales is None else (tuple(gains), ratio, device, tuple(scales))
    taps = cache.get(key)
    if taps is None:
        host = np.stack([metrics.mtf_kernel(g, ratio) * (1.0 if scales is None else scales[i]) for i, g in enumerate(gains)])
        taps = cache[key] = torch.from_numpy(host.astype(np.float32)).to(device)
        while scales is not None and len(cache) > _MTF_STEP_TAPS_MAX:
            del cache[next(iter(cache))]          # dicts keep insertion order: the oldest
    return taps


# ---- Wald consistency as a CGLS solve (csrc/cg.hip; definition: metrics.consistency_solve) ---------------------------
def plane_dots_partials(n):
    """The partial sums ``plane_dots`` keeps for a plane of n elements (1 .. 256, a function of n alone)."""
    return int(lib.tmdiff_plane_dots_partials(int(n)))


def _dot_planes(name, t, like=None):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.is_contiguous()):
        raise ValueError(f"{name}: need contiguous float32 [B, C, H, W] tensors on the GPU")
    if like is not None and (t.shape != like.shape or t.device != like.device):
        raise ValueError(f"{name}: operands {tuple(like.shape)} and {tuple(t.shape)} do not belong together")
    if t.numel() > 2 ** 31 - 1:
        raise ValueError(f"{name}: shape {tuple(t.shape)} is not supported (fewer than 2^31 elements)")
    return t.detach()


def _launch_dots(name, ops2, planes):
    """One launch for up to two dots: ops2 = [(a, b, partial sums)], the planes of each pair of their own extent."""
    (a0, b0, p0), (a1, b1, p1) = ops2[0], (ops2[1] if len(ops2) > 1 else (None, None, None))
    n = lambda t: 0 if t is None else t.shape[2] * t.shape[3]
    ptr = lambda t: None if t is None else t.data_ptr()
    check(lib.tmdiff_plane_dots(ptr(a0), ptr(b0), n(a0), ptr(p0), ptr(a1), ptr(b1), n(a1), ptr(p1), planes, stream_ptr()), name)


def plane_dots(a, b=None, out=None, workspace=None):
    """Per-plane inner products <a, b> of float32 [B, C, H, W] tensors, float64 [B, C]; ``b`` None: the squared norms <a, a>.
    ``a`` (and ``b``) may be a pair of tensors with the same [B, C] and extents of their own: both dots are made by one launch and
    the result is float64 [2, B, C].  Summed in fp64 in one fixed order that depends on the plane's extent alone (csrc/cg.hip):
    each workgroup writes the partial sum of its chunk into ``workspace`` (float64, B * C * ``plane_dots_partials(H * W)`` elements
    per dot), a second launch adds a plane's partials.  No atomics, no host read: the same bits on every run; with ``out=`` and
    ``workspace=`` nothing is allocated or synchronised."""
    name = "plane_dots"
    pair = isinstance(a, (tuple, list))
    aa = list(a) if pair else [a]
    bb = [None] * len(aa) if b is None else (list(b) if pair and isinstance(b, (tuple, list)) else [b])
    if len(aa) not in (1, 2) or len(bb) != len(aa):
        raise ValueError(f"{name}: one tensor or a pair of them, and b to match")
    aa = [_dot_planes(name, t) for t in aa]
    bb = [x if y is None else _dot_planes(name, y, x) for x, y in zip(aa, bb)]
    bc = tuple(aa[0].shape[:2])
    if any(tuple(t.shape[:2]) != bc or t.device != aa[0].device for t in aa):
        raise ValueError(f"{name}: the operands of a pair share [B, C] and the device")
    planes = bc[0] * bc[1]
    counts = [plane_dots_partials(t.shape[2] * t.shape[3]) for t in aa]
    need = planes * sum(counts)
    ws, _ = _lent(name, workspace, 8 * need, lambda: torch.empty(max(1, need), device=aa[0].device, dtype=torch.float64))
    if ws.dtype != torch.float64:
        raise ValueError(f"{name}: workspace must be float64")
    y = _f64(name, "out", out, (2, *bc) if pair else bc, aa[0].device)
    parts, lo = [], 0
    for cnt in counts:
        parts.append(ws.view(-1)[lo:lo + planes * cnt])
        lo += planes * cnt
    _launch_dots(name, list(zip(aa, bb, parts)), planes)
    for k, (cnt, part) in enumerate(zip(counts, parts)):
        check(lib.tmdiff_plane_totals(part.data_ptr(), (y[k] if pair else y).data_ptr(), planes, cnt, 1, 0, stream_ptr()), name)
    return y


def consistency_solve_workspace(b, c, h, w, ratio, iters, device):
    """The buffers ``consistency_solve`` accepts for [b, c, h, w] scenes at ``ratio`` and up to ``iters`` iterations (reusable;
    captured calls must keep them alive): the float32 vectors r, q (low resolution) and d, s, p (full resolution) and the float64
    partial sums of the dots."""
    lh, lw = fir_decimate_shape(h, w, ratio)
    planes = b * c
    cf, cl = plane_dots_partials(h * w), plane_dots_partials(lh * lw)
    f32 = lambda *shape: torch.empty(shape, device=device, dtype=torch.float32)
    return {"r": f32(b, c, lh, lw), "q": f32(b, c, lh, lw), "d": f32(b, c, h, w), "s": f32(b, c, h, w), "p": f32(b, c, h, w),
            "partials": torch.empty(planes * (3 * cf + (int(iters) + 2) * cl), device=device, dtype=torch.float64)}


def consistency_solve(f0, lr_ms, taps, ratio, iters, damp=0.0, out=None, correction_out=None, info_out=None, workspace=None):
    """Wald's consistency as a solve (definition: ``metrics.consistency_solve``): ``iters`` steps of CGLS, per plane, on
    min ||A f - lr_ms||^2 + damp ||f - f0||^2 for A = ``fir_decimate(., taps, ratio)`` at the offset ratio // 2, started from the
    correction d = 0; returns f = f0 + d in ``out`` (allocated when None; may be ``f0``).  f0 [B, C, H, W], lr_ms [B, C, H', W']
    the extent of ``fir_decimate``, taps as ``fir_decimate`` takes them.  ``correction_out`` receives d, ``info_out`` (float64
    [B, C, iters + 1]) the squared residual norm ||r||^2 per plane before the first iteration and after every one, as the
    recurrence carries it.  With damp = 0 the iterates converge to f0 + A^+ (lr_ms - A f0), the projection onto the consistent
    scenes.  An iteration is six launches: ``fir_decimate`` (q = A p), the dot <q, q>, the step (d += alpha p, r -= alpha q and the
    partial sums of ||r||^2), ``fir_decimate_adjoint`` (s = A^T r - damp d), the dot <s, s> and the direction (p = s + beta p);
    alpha and beta are formed on the device from the partial sums, 0 where their denominator is 0, so a plane that is already
    consistent comes back as it went in and no plane sees another.  The last iteration's direction is not formed: nothing reads
    it.  With ``out``, ``workspace`` (``consistency_solve_workspace``) and whichever of ``correction_out`` / ``info_out`` is wanted
    given, nothing is allocated or synchronised and the call can be captured into a graph.  Limits: ``fir_decimate``'s."""
    name = "consistency_solve"
    if int(iters) != iters or iters < 0 or not float(damp) >= 0.0:
        raise ValueError(f"{name}: iters={iters} damp={damp} (iters a whole number >= 0, damp >= 0)")
    iters, damp = int(iters), float(damp)
    _fir_taps(name, taps, ratio, None)
    f0 = _dot_planes(name, f0)
    b, c, h, w = f0.shape
    low = (b, c, *fir_decimate_shape(h, w, ratio))
    if not (torch.is_tensor(lr_ms) and lr_ms.is_cuda and lr_ms.dtype == torch.float32 and lr_ms.is_contiguous()) or tuple(lr_ms.shape) != low:
        raise ValueError(f"{name}: lr_ms must be a contiguous float32 {list(low)} tensor on the GPU, the degradation of f0 "
                         f"{tuple(f0.shape)} at ratio {ratio}")
    y = out if out is not None else torch.empty_like(f0)
    ws = workspace if workspace is not None else consistency_solve_workspace(b, c, h, w, ratio, iters, f0.device)
    d = correction_out if correction_out is not None else ws["d"]
    for t, what in ((y, "out"), (d, "correction_out"), (ws["s"], "workspace s"), (ws["p"], "workspace p")):
        if tuple(t.shape) != tuple(f0.shape):
            raise ValueError(f"{name}: {what} must be {tuple(f0.shape)}, got {tuple(t.shape)}")
        _chk(t, what)
    r, q, s, p = ws["r"], ws["q"], ws["s"], ws["p"]
    if tuple(r.shape) != low or tuple(q.shape) != low:
        raise ValueError(f"{name}: workspace r, q must be {low}")
    planes, nf, nl = b * c, h * w, low[2] * low[3]
    cf, cl = plane_dots_partials(nf), plane_dots_partials(nl)
    part = ws["partials"]
    if not (part.is_cuda and part.dtype == torch.float64 and part.is_contiguous() and part.numel() >= planes * (3 * cf + (iters + 2) * cl)):
        raise ValueError(f"{name}: workspace partials: float64, at least {planes * (3 * cf + (iters + 2) * cl)} elements")
    part = part.view(-1)
    gam = [part[:planes * cf], part[planes * cf:2 * planes * cf]]
    pp = part[2 * planes * cf:3 * planes * cf]
    qq = part[3 * planes * cf:3 * planes * cf + planes * cl]
    rr0 = 3 * planes * cf + planes * cl
    rr = [part[rr0 + k * planes * cl:rr0 + (k + 1) * planes * cl] for k in range(iters + 1)]
    info = None if info_out is None else _f64(name, "info_out", info_out, (b, c, iters + 1), f0.device)
    lr = lr_ms.detach()
    fir_decimate(f0, taps, ratio, None, q)
    add(lr, q, -1.0, out=r)                                         # r = lr - A f0
    if iters == 0:
        if info is not None:
            _launch_dots(name, [(r, r, rr[0])], planes)
        if correction_out is not None:
            d.zero_()
    else:
        fir_decimate_adjoint(r, taps, (h, w), ratio, None, p)       # s = A^T r (d = 0) and p = s
        _launch_dots(name, [(r, r, rr[0]), (p, p, gam[0])], planes)
    for k in range(iters):
        fir_decimate(p, taps, ratio, None, q)
        _launch_dots(name, [(q, q, qq)], planes)
        ppk = None if damp == 0.0 else (gam[0] if k == 0 else pp)  # <p, p>: at the start p = s
        check(lib.tmdiff_cg_step(p.data_ptr(), q.data_ptr(), d.data_ptr(), r.data_ptr(), gam[k % 2].data_ptr(), qq.data_ptr(),
                                 None if ppk is None else ppk.data_ptr(), damp, rr[k + 1].data_ptr(), planes, nf, nl, int(k == 0),
                                 stream_ptr()), name)
        if k + 1 < iters:
            fir_decimate_adjoint(r, taps, (h, w), ratio, None, s, d, 1.0, -damp)
            _launch_dots(name, [(s, s, gam[(k + 1) % 2])], planes)
            check(lib.tmdiff_cg_direction(s.data_ptr(), p.data_ptr(), gam[(k + 1) % 2].data_ptr(), gam[k % 2].data_ptr(),
                                          None if damp == 0.0 else pp.data_ptr(), planes, nf, stream_ptr()), name)
    if iters:
        add(f0, d, out=y)
    elif y.data_ptr() != f0.data_ptr():
        y.copy_(f0)
    if info is not None:
        check(lib.tmdiff_plane_totals(rr[0].data_ptr(), info.data_ptr(), planes, cl, iters + 1, planes * cl, stream_ptr()), name)
    return y


# ---- HQNR: Khan's D_lambda, block-wise D_s (csrc/metrics.hip, csrc/mtf.hip; definitions: tmdiff_amd/metrics.py) ------
_DSBLOCK_LIMITS = "1 <= C <= 16, block 8, 16 or 32, mirror padding no longer than the axis, fewer than 2^31 elements, q > 0"


def metrics_dsblock_supported(b, c, h, w, block=32):
    """True when metrics_dsblock takes a [b, c, h, w] image batch with these windows."""
    return bool(lib.tmdiff_metrics_dsblock_supported(int(b), int(c), int(h), int(w), int(block)))


def metrics_dsblock_workspace(b, c, h, w, device, block=32):
    """A workspace metrics_dsblock accepts for [b, c, h, w] images (reusable; captured calls must keep it alive)."""
    nbytes = lib.tmdiff_metrics_dsblock_workspace_bytes(int(b), int(c), int(h), int(w), int(block))
    return torch.empty(max(1, nbytes // 8), device=device, dtype=torch.float64)


def metrics_dsblock(ps, ms_exp, pan, pan_lp, block=32, q=1.0, out=None, maps_out=None, workspace=None, d_lambda=None, alpha=1.0,
                    beta=1.0):
    """The block-wise D_s of HQNR (definition: ``metrics.d_s_block``) of ps and ms_exp, float32 [B, C, H, W], with pan and
    pan_lp, float32 [B, 1, H, W]: float64 [B].  ``out`` is a float64 [B, 2] tensor whose first column is returned; with
    ``d_lambda``, a contiguous float64 [B] device tensor, its second column receives (1 - d_lambda)^alpha (1 - D_s)^beta and is
    otherwise left alone.  ``maps_out``, float64 [B, C, 2, ny, nx] (``q2n_grid`` at shift = block), receives the windows'
    Q(ps_c, pan) and Q(ms_exp_c, pan_lp).  A window constant in both images is NaN there and in D_s."""
    if ps.shape != ms_exp.shape:
        raise ValueError(f"metrics_dsblock: shapes {tuple(ps.shape)} and {tuple(ms_exp.shape)} differ")
    pa, asb, asc = _planes(ps, "ps")
    pb, bsb, bsc = _planes(ms_exp, "ms_exp")
    b, c, h, w = ps.shape
    pp, psb, _ = _planes(pan, "pan", 1)
    pq, qsb, _ = _planes(pan_lp, "pan_lp", 1)
    if tuple(pan.shape) != (b, 1, h, w) or tuple(pan_lp.shape) != (b, 1, h, w):
        raise ValueError(f"metrics_dsblock: pan {tuple(pan.shape)} and pan_lp {tuple(pan_lp.shape)} must be [{b}, 1, {h}, {w}]")
    block, q = int(block), float(q)
    if not metrics_dsblock_supported(b, c, h, w, block) or not q > 0.0:
        raise ValueError(f"metrics_dsblock: B={b} C={c} H={h} W={w} block={block} q={q} is not supported ({_DSBLOCK_LIMITS})")
    ny, nx = q2n_grid(h, w, block, block)
    dev = ps.device
    y = _f64("metrics_dsblock", "out", out, (b, 2), dev)
    if maps_out is not None:
        _f64("metrics_dsblock", "maps_out", maps_out, (b, c, 2, ny, nx), dev)
    if d_lambda is not None:
        _f64("metrics_dsblock", "d_lambda", d_lambda, (b,), dev)
    ws, nbytes = _lent("metrics_dsblock", workspace, lib.tmdiff_metrics_dsblock_workspace_bytes(b, c, h, w, block),
                       lambda: metrics_dsblock_workspace(b, c, h, w, dev, block))
    check(lib.tmdiff_metrics_dsblock(pa, asb, asc, pb, bsb, bsc, pp, psb, pq, qsb, b, c, h, w, block, q,
                                     d_lambda.data_ptr() if d_lambda is not None else None, float(alpha), float(beta),
                                     y.data_ptr(), maps_out.data_ptr() if maps_out is not None else None, ws.data_ptr(), nbytes,
                                     stream_ptr()), "metrics_dsblock")
    return y[:, 0]


def pan_lowpass(pan, sensor_or_gain, ratio=4, out=None, low=None):
    """The PAN [B, 1, H, W] at the resolution of the MS, on its own grid (definition: ``metrics.pan_lowpass``):
    ``upsample_poly23(mtf_degrade(pan, ..., ratio, pan=True), ratio)``; ratio 2 or 4, H and W multiples of it.  ``low``
    lends the [B, 1, H / ratio, W / ratio] stage; with it and ``out=`` nothing is allocated (the tap table is cached as
    ``mtf_degrade`` caches it: call once before capturing into a graph)."""
    if not (torch.is_tensor(pan) and pan.is_cuda and pan.dim() == 4 and pan.shape[1] == 1):
        raise ValueError("pan_lowpass: need a float32 [B, 1, H, W] tensor on the GPU")
    if ratio not in (2, 4) or pan.shape[2] % ratio or pan.shape[3] % ratio or min(pan.shape[2:]) < ratio:
        raise ValueError(f"pan_lowpass: shape {tuple(pan.shape)} ratio={ratio} (ratio 2 or 4, H and W multiples of it)")
    # a metric's stage, not a differentiable degradation: pan.requires_grad changes nothing here
    return upsample_poly23(mtf_degrade(pan.detach(), sensor_or_gain, ratio, pan=True, out=low), ratio, out=out)


def metrics_hqnr_buffers(b, c, h, w, device, ratio=4, block=32):
    """Every scratch tensor of ``metrics_hqnr`` for [b, c, h, w] images: with them a second call allocates nothing and can be
    captured into a graph.  "filtered": the MTF-filtered fused image; "pan_lp" and "pan_low": the low-pass PAN and its
    low-resolution stage; "q2n", "d_lambda", "d_s": the chain's float64 results; "q2n_ws", "ds_ws": the kernels' workspaces."""
    if ratio not in (2, 4) or h % ratio or w % ratio:
        raise ValueError(f"metrics_hqnr: H={h} W={w} ratio={ratio} (ratio 2 or 4, H and W multiples of it)")
    if not metrics_dsblock_supported(b, c, h, w, block):
        raise ValueError(f"metrics_hqnr: B={b} C={c} H={h} W={w} block={block} is not supported ({_DSBLOCK_LIMITS})")
    f32 = dict(device=device, dtype=torch.float32)
    f64 = lambda arg, *shape: _f64("metrics_hqnr", arg, None, shape, device)
    return {"shape": (b, c, h, w, ratio, block),
            "filtered": torch.empty(b, c, h, w, **f32), "pan_lp": torch.empty(b, 1, h, w, **f32),
            "pan_low": torch.empty(b, 1, h // ratio, w // ratio, **f32),
            "q2n": f64("q2n", b), "d_lambda": f64("d_lambda", b), "d_s": f64("d_s", b, 2),
            "q2n_ws": metrics_q2n_workspace(b, c, h, w, device, block, block),
            "ds_ws": metrics_dsblock_workspace(b, c, h, w, device, block)}


def metrics_hqnr(ps, ms_exp, pan, sensor, ratio=4, block=32, alpha=1.0, beta=1.0, q=1.0, pan_lp=None, out=None, buffers=None):
    """Khan's D_lambda, the block-wise D_s and HQNR (definition: ``metrics.hqnr``) of the fused ps [B, C, H, W] with pan
    [B, 1, H, W] against ms_exp, the MS interpolated to the PAN grid: float64 [B, 3] in the column order of
    metrics.HQNR_FIELDS.  ps is filtered at full scale with the sensor's 41 x 41 MTF filters (``fir_decimate`` at ratio 1) and
    scored against ms_exp with ``metrics_q2n``; ``pan_lp`` None is ``pan_lowpass(pan, sensor's PAN gain, ratio)``;
    ``metrics_dsblock`` then forms D_s and the product.  ``sensor``: a name or a pair (MS gains, PAN gain), as
    ``metrics.mtf_gains`` takes them.  With ``buffers`` (``metrics_hqnr_buffers``) and ``out=`` nothing is allocated or
    synchronised; the tap tables are cached as ``mtf_degrade`` caches its own: call once before capturing into a graph."""
    from . import metrics
    if not (torch.is_tensor(ps) and ps.is_cuda and ps.dim() == 4) or ps.shape != ms_exp.shape:
        raise ValueError("metrics_hqnr: ps and ms_exp must be float32 [B, C, H, W] tensors of one shape on the GPU")
    b, c, h, w = ps.shape
    block = int(block)
    buf = buffers if buffers is not None else metrics_hqnr_buffers(b, c, h, w, ps.device, ratio, block)
    if buf["shape"] != (b, c, h, w, ratio, block) or buf["filtered"].device != ps.device:
        raise ValueError(f"metrics_hqnr: buffers made for {buf['shape']}, the call is {(b, c, h, w, ratio, block)}")
    ms_gains, pan_gain = metrics.mtf_gains(sensor, c)
    y = _f64("metrics_hqnr", "out", out, (b, 3), ps.device, contiguous=False)
    # the metric is not differentiable: ps.requires_grad changes nothing here
    filtered = fir_decimate(ps.detach(), _mtf_taps(ms_gains, ratio, ps.device), 1, None, buf["filtered"])
    metrics_q2n(ms_exp, filtered, block, block, out=buf["q2n"], workspace=buf["q2n_ws"])
    torch.neg(buf["q2n"], out=buf["d_lambda"]).add_(1.0)                       # 1 - Q2n, as the host rounds it
    if pan_lp is None:
        pan_lp = pan_lowpass(pan, pan_gain, ratio, out=buf["pan_lp"], low=buf["pan_low"])
    metrics_dsblock(ps, ms_exp, pan, pan_lp, block, q, out=buf["d_s"], workspace=buf["ds_ws"], d_lambda=buf["d_lambda"],
                    alpha=alpha, beta=beta)
    y[:, 0].copy_(buf["d_lambda"])
    y[:, 1:].copy_(buf["d_s"])
    return y


# ---- MTF-GLP: the classical baselines (csrc/mtf.hip, csrc/metrics.hip, csrc/fusion.hip; definitions: tmdiff_amd/metrics.py)
_GLP_LIMITS = ("contiguous float32 tensors on the GPU, ms_exp and pan_lp [B, C, H, W], pan [B, 1, H, W]; 1 <= C <= 16; ratio 2 or 4, "
               "H and W multiples of it; fewer than 2^31 elements")


# What the wrappers of the three families (MTF-GLP here, component substitution and BDSD below) check alike.  A family is the name
# its messages give the MS image, its largest C and its limits text.
_Family = collections.namedtuple("_Family", "ms max_c limits")
_GLP = _Family("ms_exp", 16, _GLP_LIMITS)


def _dense(fam, name, arg, t, shape=None):
    """``t`` must be dense float32 device memory, of ``shape`` when that is given."""
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise ValueError(f"{name}: {arg} must be a contiguous float32 tensor on the GPU ({fam.limits})")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: {arg} is {tuple(t.shape)}, need {tuple(shape)} ({fam.limits})")
    return t


def _extents(fam, name, b, c, h, w, ratio=None, block=None):
    """(B, C, H, W, blocks down, blocks across) after the checks on the extents; ``block`` (BDSD) is a side at the images' scale."""
    b, c, h, w = int(b), int(c), int(h), int(w)
    if not 1 <= c <= fam.max_c or min(b, h, w) < 1 or b * c * h * w > 2 ** 31 - 1:
        raise ValueError(f"{name}: B={b} C={c} H={h} W={w} is not supported ({fam.limits})")
    if ratio is not None and (ratio not in (2, 4) or h % ratio or w % ratio):
        raise ValueError(f"{name}: H={h} W={w} ratio={ratio} is not supported ({fam.limits})")
    if block is not None and (isinstance(block, bool) or int(block) != block or block < 1 or block % (ratio or 1) or h % block or w % block):
        raise ValueError(f"{name}: block={block!r} for H={h} W={w} ratio={ratio or 1} is not supported ({fam.limits})")
    return b, c, h, w, (1 if block is None else h // int(block)), (1 if block is None else w // int(block))


def _images(fam, name, ms, pan, ratio=None, block=None):
    """The extents of ``_extents`` after the checks on the MS image [B, C, H, W] and the PAN [B, 1, H, W] of a call."""
    _dense(fam, name, fam.ms, ms)
    if ms.dim() != 4:
        raise ValueError(f"{name}: {fam.ms} is {tuple(ms.shape)}, need [B, C, H, W] ({fam.limits})")
    extents = _extents(fam, name, *ms.shape, ratio, block)
    _dense(fam, name, "pan", pan, (extents[0], 1, *extents[2:4]))
    return extents


def _glp_images(name, ms_exp, pan, pan_lp=None, ratio=None):
    """(B, C, H, W) of a GLP call after the checks on its images."""
    b, c, h, w = _images(_GLP, name, ms_exp, pan, ratio)[:4]
    if pan_lp is not None:
        _dense(_GLP, name, "pan_lp", pan_lp, (b, c, h, w))
    return b, c, h, w


def _overlaps(a, b):
    """True when the bytes of two dense tensors intersect."""
    lo, hi = b.data_ptr(), b.data_ptr() + b.numel() * b.element_size()
    return a.data_ptr() < hi and lo < a.data_ptr() + a.numel() * a.element_size()


def _chain_out(fam, name, out, shape, others):
    """The rule on the ``out`` of a whole chain, when one is given: of ``shape`` and clear of every tensor in ``others``, pairs
    (tensor or None, its name).  That it may be ms_exp itself, and nothing else of ms_exp, is left to the injection."""
    if out is not None:
        _dense(fam, name, "out", out, shape)
        for other, what in others:
            if other is not None and _overlaps(out, other):
                raise ValueError(f"{name}: out overlaps {what}")
    return out


def _inject_out(fam, name, out, ms_exp, others):
    """The output of an injection, ``out`` or a new tensor: it may be ms_exp itself (in place) and must not overlap anything else."""
    y = _chain_out(fam, name, out if out is not None else torch.empty_like(ms_exp), tuple(ms_exp.shape), others)
    if y.data_ptr() != ms_exp.data_ptr() and _overlaps(y, ms_exp):
        raise ValueError(f"{name}: out overlaps ms_exp without being ms_exp")
    return y


def _chain_buffers(name, buffers, make, shape, probe, device):
    """``buffers`` of a chain, or with None ``make()``: they must have been made for ``shape`` on ``device`` (``probe`` names one)."""
    buf = buffers if buffers is not None else make()
    if buf["shape"] != shape or buf[probe].device != device:
        raise ValueError(f"{name}: buffers made for {buf['shape']}, the call is {shape}")
    return buf


def _reduced_ms(fam, name, ms_exp, lr_ms, ratio, stage):
    """The reduced-scale MS of a chain: ``lr_ms`` [B, C, H / ratio, W / ratio], or with None the samples
    ms_exp[..., ratio // 2::ratio, ratio // 2::ratio] copied into ``stage``."""
    if lr_ms is None:
        stage.copy_(ms_exp[..., ratio // 2::ratio, ratio // 2::ratio])
        return stage
    b, c, h, w = ms_exp.shape
    return _dense(fam, name, "lr_ms", lr_ms, (b, c, h // ratio, w // ratio)).detach()


def fir_decimate_bank(x, taps, ratio=1, offset=None, out=None):
    """A filter bank on one plane per image (definition: ``metrics.fir_decimate`` of each pair): x [B, H, W] or [B, 1, H, W],
    taps [T, K, K] -> y [B, T, H', W'] with y[b, t] = ``fir_decimate(x[b], taps[t], ratio, offset)``, bit for bit what
    ``fir_decimate`` gives on ``x.expand(B, T, H, W).contiguous()`` -- without that T-fold copy: a workgroup stages a patch of
    x[b] once and walks the T tables over it.  With ``out=`` nothing is allocated or synchronised (graph capture).  Not
    differentiable: x is detached."""
    from .metrics import fir_decimate_shape as shape_of
    name = "fir_decimate_bank"
    t, k, (oy, ox) = _fir_taps(name, taps, ratio, offset)
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
            and (x.dim() == 3 or (x.dim() == 4 and x.shape[1] == 1))):
        raise ValueError(f"{name}: need a contiguous float32 [B, H, W] or [B, 1, H, W] tensor on the GPU ({_FIR_LIMITS})")
    x = x.detach()
    b, (h, w) = x.shape[0], x.shape[-2:]
    if min(h, w) < 1 or taps.device != x.device or b * t * h * w > 2 ** 31 - 1:
        raise ValueError(f"{name}: x {tuple(x.shape)} on {x.device} with taps {tuple(taps.shape)} on {taps.device} is not supported "
                         f"({_FIR_LIMITS}; fewer than 2^31 elements in B * T * H * W)")
    shape = (b, t, *shape_of(h, w, ratio, offset)[0])
    y = out if out is not None else torch.empty(shape, device=x.device, dtype=torch.float32)
    if tuple(y.shape) != shape:
        raise ValueError(f"{name}: out must be {shape}, got {tuple(y.shape)}")
    py = _chk(y, "out")
    if _overlaps(y, x) or _overlaps(y, taps):
        raise ValueError(f"{name}: out overlaps x or taps")
    check(lib.tmdiff_fir_decimate_bank(x.data_ptr(), taps.data_ptr(), py, b, t, h, w, k, ratio, oy, ox, stream_ptr()), name)
    return y


def pan_lowpass_bands(pan, sensor_or_gains, bands, ratio=4, out=None, low=None):
    """The PAN [B, 1, H, W] seen through every MS band's MTF (definition: ``metrics.pan_lowpass_bands``): [B, C, H, W] with band
    c = ``upsample_poly23(fir_decimate(pan, mtf_kernel(g_c, ratio), ratio), ratio)``, g_c the gains of the MS bands
    (``metrics.band_gains(sensor_or_gains, bands)``), not the PAN gain as in ``pan_lowpass``.  ``fir_decimate_bank`` filters the
    one PAN plane with the C tables.  The float64 definition sets the PAN's mean aside before this chain and adds it back (the
    interpolator loses 1.21e-9 of a constant); that is a fiftieth of float32's resolution, and the device runs the chain as
    it stands.  ``low`` lends the [B, C, H / ratio, W / ratio] stage; with it and ``out=`` nothing is
    allocated (the tap table is cached as ``mtf_degrade`` caches it: call once before capturing into a graph).  Not
    differentiable: pan is detached."""
    from . import metrics
    name = "pan_lowpass_bands"
    if not (torch.is_tensor(pan) and pan.is_cuda and pan.dim() == 4 and pan.shape[1] == 1):
        raise ValueError(f"{name}: need a float32 [B, 1, H, W] tensor on the GPU ({_GLP_LIMITS})")
    bands = int(bands)
    if ratio not in (2, 4) or pan.shape[2] % ratio or pan.shape[3] % ratio or min(pan.shape[2:]) < ratio or not 1 <= bands <= 16:
        raise ValueError(f"{name}: shape {tuple(pan.shape)} ratio={ratio} bands={bands} is not supported ({_GLP_LIMITS})")
    gains = metrics.band_gains(sensor_or_gains, bands)
    return upsample_poly23(fir_decimate_bank(pan, _mtf_taps(gains, ratio, pan.device), ratio, None, low), ratio, out=out)


def glp_moments_workspace(b, c, h, w, device):
    """A workspace ``glp_moments`` accepts for [b, c, h, w] images (reusable; captured calls must keep it alive).  After a call
    its first b * c * 7 doubles are the finished sums about the pilots (include/tmdiff_hip.h)."""
    return torch.empty(max(1, lib.tmdiff_glp_moments_workspace_bytes(int(b), int(c), int(h), int(w)) // 8), device=device,
                       dtype=torch.float64)


def glp_moments(ms_exp, pan, pan_lp, out=None, workspace=None):
    """The injection statistics of MTF-GLP (definition: ``metrics.glp_moments``): float64 [B, C, 7] in the column order of
    ``metrics.GLP_MOMENT_FIELDS`` -- the population means, variances and covariance of ms_exp and pan_lp per band, the mean and
    variance of pan -- from one pass over the three images, as device values.  Sums in fp64 in one fixed order, no atomics: the
    same bits on every run.  With ``out=`` and ``workspace=`` nothing is allocated or synchronised.  Not differentiable: the
    inputs are detached."""
    b, c, h, w = _glp_images("glp_moments", ms_exp, pan, pan_lp)
    y = _f64("glp_moments", "out", out, (b, c, 7), ms_exp.device)
    ws, nbytes = _lent("glp_moments", workspace, lib.tmdiff_glp_moments_workspace_bytes(b, c, h, w),
                       lambda: glp_moments_workspace(b, c, h, w, ms_exp.device))
    check(lib.tmdiff_glp_moments(ms_exp.detach().data_ptr(), pan.detach().data_ptr(), pan_lp.detach().data_ptr(), b, c, h, w,
                                 y.data_ptr(), ws.data_ptr(), nbytes, stream_ptr()), "glp_moments")
    return y


def glp_inject(ms_exp, pan, pan_lp, moments, mode, out=None):
    """The injection of MTF-GLP (definition: ``metrics.glp_inject``, the formulas of ``metrics.mtf_glp``): the fused [B, C, H, W]
    from ms_exp, pan, pan_lp and ``moments``, the float64 [B, C, 7] device tensor of ``glp_moments``; ``mode`` "glp", "cbd" or
    "hpm".  The band gains are formed on the device from the moments -- nothing is read on the host -- and every pixel is
    evaluated in fp64 and rounded to fp32 once.  ``out`` may be ms_exp itself (in place); it must not overlap pan, pan_lp or
    moments.  With ``out=`` nothing is allocated or synchronised.  Not differentiable: the inputs are detached."""
    from . import metrics
    if mode not in metrics.GLP_MODES:
        raise ValueError(f"glp_inject: mode={mode!r} (one of {metrics.GLP_MODES})")
    b, c, h, w = _glp_images("glp_inject", ms_exp, pan, pan_lp)
    mo = _f64("glp_inject", "moments", moments, (b, c, 7), ms_exp.device)
    y = _inject_out(_GLP, "glp_inject", out, ms_exp, ((pan, "pan"), (pan_lp, "pan_lp"), (mo, "moments")))
    check(lib.tmdiff_glp_inject(ms_exp.detach().data_ptr(), pan.detach().data_ptr(), pan_lp.detach().data_ptr(), mo.data_ptr(),
                                y.data_ptr(), b, c, h, w, metrics.GLP_MODES.index(mode), stream_ptr()), "glp_inject")
    return y


def mtf_glp_buffers(b, c, h, w, device, ratio=4):
    """Every scratch tensor of ``mtf_glp`` for [b, c, h, w] images: with them and ``out=`` a call allocates nothing and can be
    captured into a graph.  "pan_lp" and "pan_low": the per-band low-pass PAN and its low-resolution stage; "moments": the
    float64 [b, c, 7] statistics; "ws": the workspace of ``glp_moments``."""
    b, c, h, w = int(b), int(c), int(h), int(w)
    if not 1 <= c <= 16 or min(b, h, w) < 1 or ratio not in (2, 4) or h % ratio or w % ratio or b * c * h * w > 2 ** 31 - 1:
        raise ValueError(f"mtf_glp: B={b} C={c} H={h} W={w} ratio={ratio} is not supported ({_GLP_LIMITS})")
    f32 = dict(device=device, dtype=torch.float32)
    return {"shape": (b, c, h, w, ratio), "pan_lp": torch.empty(b, c, h, w, **f32),
            "pan_low": torch.empty(b, c, h // ratio, w // ratio, **f32),
            "moments": torch.empty(b, c, 7, device=device, dtype=torch.float64), "ws": glp_moments_workspace(b, c, h, w, device)}


def mtf_glp(ms_exp, pan, sensor, ratio=4, mode="hpm", pan_lp=None, out=None, buffers=None):
    """MTF-GLP pansharpening on the device (definition: ``metrics.mtf_glp``): the fused [B, C, H, W] from ms_exp, the MS
    interpolated to the PAN grid, and pan [B, 1, H, W]; ``mode`` "glp" (additive), "cbd" (regression gain) or "hpm"
    (multiplicative).  ``pan_lp`` None is ``pan_lowpass_bands(pan, MS gains of sensor, C, ratio)``; ``glp_moments`` then leaves
    the statistics on the device and ``glp_inject`` forms the gains there and writes the result.  ``sensor``: a name or a pair
    (MS gains, PAN gain), as ``metrics.mtf_gains`` takes them.  ``out`` may be ms_exp.  With ``buffers`` (``mtf_glp_buffers``) and
    ``out=`` nothing is allocated or synchronised; the tap table is cached as ``mtf_degrade`` caches its own: call once before
    capturing into a graph.  Not differentiable: the inputs are detached."""
    from . import metrics
    if mode not in metrics.GLP_MODES:
        raise ValueError(f"mtf_glp: mode={mode!r} (one of {metrics.GLP_MODES})")
    b, c, h, w = _glp_images("mtf_glp", ms_exp, pan, pan_lp, ratio)
    _chain_out(_GLP, "mtf_glp", out, (b, c, h, w), ((pan, "pan"), (pan_lp, "pan_lp")))
    buf = _chain_buffers("mtf_glp", buffers, lambda: mtf_glp_buffers(b, c, h, w, ms_exp.device, ratio), (b, c, h, w, ratio), "pan_lp",
                         ms_exp.device)
    if pan_lp is None:
        pan_lp = pan_lowpass_bands(pan, metrics.mtf_gains(sensor, c)[0], c, ratio, out=buf["pan_lp"], low=buf["pan_low"])
    mo = glp_moments(ms_exp, pan, pan_lp, out=buf["moments"], workspace=buf["ws"])
    return glp_inject(ms_exp, pan, pan_lp, mo, mode, out=out)


# ---- component substitution: GS, GSA, Brovey (csrc/cs_fusion.hip; definitions: tmdiff_amd/metrics.py) ---------------------------
_CS_LIMITS = ("contiguous float32 tensors on the GPU, ms [B, C, H, W], pan [B, 1, H, W]; 1 <= C <= 14; ratio 2 or 4, H and W "
              "multiples of it; fewer than 2^31 elements")


_CS = _Family("ms", 14, _CS_LIMITS)


def _cs_mode(name, method):
    from . import metrics
    if method not in metrics.CS_METHODS:
        raise ValueError(f"{name}: method={method!r} (one of {metrics.CS_METHODS})")
    return metrics.CS_METHODS.index(method)


def plane_moments_workspace(b, c, h, w, device):
    """A workspace ``plane_moments`` accepts for [b, c, h, w] images (reusable; captured calls must keep it alive).  After a call
    its first b * (c + 2)^2 doubles are the finished raw sums about the pilots (include/tmdiff_hip.h)."""
    return torch.empty(max(1, lib.tmdiff_plane_gram_workspace_bytes(int(b), int(c), int(h), int(w)) // 8), device=device,
                       dtype=torch.float64)


def plane_moments(ms, pan, out=None, workspace=None):
    """The joint second moments of all bands and the PAN (definition: ``metrics.plane_moments``): float64 [B, C + 1, C + 2], the
    population covariance matrix of the planes (the C bands of ms, then pan) and, in the last column, their means, as device
    values from one pass over the images: the (C + 2) x (C + 2) Gram matrix of the planes and a plane of ones is accumulated
    with the fp64 matrix instruction.  Sums in fp64 in one fixed order, no atomics: the same bits on every run; the matrix is
    exactly symmetric.  With ``out=`` and ``workspace=`` nothing is allocated or synchronised.  Not differentiable: the inputs
    are detached."""
    b, c, h, w = _images(_CS, "plane_moments", ms, pan)[:4]
    y = _f64("plane_moments", "out", out, (b, c + 1, c + 2), ms.device)
    ws, nbytes = _lent("plane_moments", workspace, lib.tmdiff_plane_gram_workspace_bytes(b, c, h, w),
                       lambda: plane_moments_workspace(b, c, h, w, ms.device))
    check(lib.tmdiff_plane_gram(ms.detach().data_ptr(), pan.detach().data_ptr(), b, c, h, w, y.data_ptr(), ws.data_ptr(), nbytes,
                                stream_ptr()), "plane_moments")
    return y


def cs_coeffs(full, low, method, out=None):
    """The constants of a component-substitution fusion (definition: ``metrics.cs_coeffs``): float64 [B, 2 C + 3] = alpha, g, a,
    mean_I, mean_P from ``full``, the float64 [B, C + 1, C + 2] device tensor of ``plane_moments`` at the PAN scale, and for
    "gsa" ``low``, the same at the reduced scale (None otherwise).  "gsa" solves its C x C system by a root-free unpivoted Cholesky
    factorisation on the device; a singular system gives NaN.  Nothing is read on the host; with ``out=`` nothing is allocated."""
    mode = _cs_mode("cs_coeffs", method)
    if not (torch.is_tensor(full) and full.dim() == 3 and full.shape[2] == full.shape[1] + 1 and 2 <= full.shape[1] <= 15):
        raise ValueError("cs_coeffs: full must be a float64 [B, C + 1, C + 2] tensor on the GPU, 1 <= C <= 14")
    b, c = full.shape[0], full.shape[1] - 1
    full = _f64("cs_coeffs", "full", full, (b, c + 1, c + 2), None)
    if method == "gsa":
        if low is None:
            raise ValueError("cs_coeffs: method 'gsa' needs the reduced-scale moments `low`")
        low = _f64("cs_coeffs", "low", low, (b, c + 1, c + 2), None)
        if low.device != full.device:
            raise ValueError("cs_coeffs: full and low are on different devices")
    else:
        low = None
    y = _f64("cs_coeffs", "out", out, (b, 2 * c + 3), full.device)
    for other, what in ((full, "full"), (low, "low")):
        if other is not None and _overlaps(y, other):
            raise ValueError(f"cs_coeffs: out overlaps {what}")
    check(lib.tmdiff_cs_coeffs(full.detach().data_ptr(), low.detach().data_ptr() if low is not None else None, y.data_ptr(), b, c, mode,
                               stream_ptr()), "cs_coeffs")
    return y


def cs_inject(ms_exp, pan, coef, method, out=None):
    """The injection of component substitution (definition: ``metrics.cs_inject``): the fused [B, C, H, W] from ms_exp, pan and
    ``coef``, the float64 [B, 2 C + 3] device tensor of ``cs_coeffs``; ``method`` "gs", "gsa" or "brovey".  Every pixel is
    evaluated in fp64 and rounded to fp32 once.  ``out`` may be ms_exp itself (in place); it must not overlap pan or coef.
    With ``out=`` nothing is allocated or synchronised.  Not differentiable: the inputs are detached."""
    mode = _cs_mode("cs_inject", method)
    b, c, h, w = _images(_CS, "cs_inject", ms_exp, pan)[:4]
    co = _f64("cs_inject", "coef", coef, (b, 2 * c + 3), ms_exp.device)
    y = _inject_out(_CS, "cs_inject", out, ms_exp, ((pan, "pan"), (co, "coef")))
    check(lib.tmdiff_cs_inject(ms_exp.detach().data_ptr(), pan.detach().data_ptr(), co.detach().data_ptr(), y.data_ptr(), b, c, h, w,
                               mode, stream_ptr()), "cs_inject")
    return y


def cs_fuse_buffers(b, c, h, w, device, ratio=4):
    """Every scratch tensor of ``cs_fuse`` for [b, c, h, w] images: with them and ``out=`` a call allocates nothing and can be
    captured into a graph.  "full", "low": the float64 [b, c + 1, c + 2] moments at the two scales; "coef": the float64
    [b, 2 c + 3] constants; "ms_low", "pan_low": the reduced-scale pair of "gsa"; "ws", "ws_low": the workspaces of
    ``plane_moments``."""
    b, c, h, w = int(b), int(c), int(h), int(w)
    if not 1 <= c <= 14 or min(b, h, w) < 1 or ratio not in (2, 4) or h % ratio or w % ratio or b * c * h * w > 2 ** 31 - 1:
        raise ValueError(f"cs_fuse: B={b} C={c} H={h} W={w} ratio={ratio} is not supported ({_CS_LIMITS})")
    f32, f64 = dict(device=device, dtype=torch.float32), dict(device=device, dtype=torch.float64)
    return {"shape": (b, c, h, w, ratio), "full": torch.empty(b, c + 1, c + 2, **f64), "low": torch.empty(b, c + 1, c + 2, **f64),
            "coef": torch.empty(b, 2 * c + 3, **f64), "ms_low": torch.empty(b, c, h // ratio, w // ratio, **f32),
            "pan_low": torch.empty(b, 1, h // ratio, w // ratio, **f32), "ws": plane_moments_workspace(b, c, h, w, device),
            "ws_low": plane_moments_workspace(b, c, h // ratio, w // ratio, device)}


def cs_fuse(ms_exp, pan, sensor=None, ratio=4, method="gsa", lr_ms=None, out=None, buffers=None):
    """Component-substitution pansharpening on the device (definition: ``metrics.cs_fuse``): the fused [B, C, H, W] from ms_exp,
    the MS interpolated to the PAN grid, and pan [B, 1, H, W]; ``method`` "gs" (Gram-Schmidt, mean intensity), "gsa" (adaptive
    Gram-Schmidt) or "brovey".  ``plane_moments`` leaves the joint moments on the device, ``cs_coeffs`` forms the constants
    there and ``cs_inject`` writes the result.  "gsa" regresses the reduced-scale PAN, ``mtf_degrade(pan, PAN gain of sensor,
    ratio)``, on the reduced-scale MS: ``lr_ms`` [B, C, H / ratio, W / ratio], or with None the samples
    ms_exp[..., ratio // 2::ratio, ratio // 2::ratio], which are the raw MS when ms_exp came from ``upsample_poly23``.  ``sensor``
    (a name or a pair (MS gains, PAN gain), as ``metrics.mtf_gains`` takes them) is needed for "gsa" only.  ``out`` may be
    ms_exp.  With ``buffers`` (``cs_fuse_buffers``) and ``out=`` nothing is allocated or synchronised; the tap table is cached as
    ``mtf_degrade`` caches its own: call once before capturing into a graph.  Not differentiable: the inputs are detached."""
    from . import metrics
    _cs_mode("cs_fuse", method)
    b, c, h, w = _images(_CS, "cs_fuse", ms_exp, pan, ratio)[:4]
    ms_exp, pan = ms_exp.detach(), pan.detach()
    _chain_out(_CS, "cs_fuse", out, (b, c, h, w), ((pan, "pan"),))
    buf = _chain_buffers("cs_fuse", buffers, lambda: cs_fuse_buffers(b, c, h, w, ms_exp.device, ratio), (b, c, h, w, ratio), "full",
                         ms_exp.device)
    low = None
    if method == "gsa":
        if sensor is None:
            raise ValueError("cs_fuse: method 'gsa' needs the sensor whose PAN gain shapes the reduced-scale PAN")
        gain = metrics.mtf_gains(sensor, c)[1]
        ms_low = _reduced_ms(_CS, "cs_fuse", ms_exp, lr_ms, ratio, buf["ms_low"])
        pan_low = mtf_degrade(pan, gain, ratio, out=buf["pan_low"])
        low = plane_moments(ms_low, pan_low, out=buf["low"], workspace=buf["ws_low"])
    full = plane_moments(ms_exp, pan, out=buf["full"], workspace=buf["ws"])
    return cs_inject(ms_exp, pan, cs_coeffs(full, low, method, out=buf["coef"]), method, out=out)


# ---- BDSD: block-wise regression and injection (csrc/bdsd.hip; definitions: tmdiff_amd/metrics.py) ---------------------------------
_BDSD_LIMITS = ("contiguous float32 tensors on the GPU, ms [B, C, H, W], pan [B, 1, H, W]; 1 <= C <= 15; ratio 2 or 4, H and W "
                "multiples of it; block None or a multiple of the ratio that divides H and W; fewer than 2^31 elements")


_BDSD = _Family("ms", 15, _BDSD_LIMITS)


def bdsd_moments_workspace(b, c, h, w, device, bs=None):
    """A workspace ``bdsd_moments`` accepts for [b, c, h, w] reduced-scale images in blocks of side ``bs`` (reusable; captured
    calls must keep it alive)."""
    b, c, h, w, _, _ = _extents(_BDSD, "bdsd_moments", b, c, h, w, None, bs)
    return torch.empty(max(1, lib.tmdiff_bdsd_gram_workspace_bytes(b, c, h, w, int(bs or 0)) // 8), device=device, dtype=torch.float64)


def bdsd_moments(low_lp, low_pan, low_ms, bs=None, out=None, workspace=None):
    """The normal equations of BDSD per block (definition: ``metrics.bdsd_moments``): float64 [B, nby, nbx, C + 1, 2 C + 1] = N | R
    from the reduced-scale images low_lp, low_ms [B, C, h, w] and low_pan [B, 1, h, w], N = Hm' Hm over the regressors (the C
    low-pass bands, then the PAN) and R = Hm' D over the targets D_c = low_ms_c - low_lp_c, as device values from one pass: both
    products are accumulated with the fp64 matrix instruction.  ``bs``: the side of the blocks at this scale, None for the whole
    image.  Sums in fp64 in one fixed order, no atomics: the same bits on every run; N is exactly symmetric.  With ``out=`` and
    ``workspace=`` nothing is allocated or synchronised.  Not differentiable: the inputs are detached."""
    b, c, h, w, nby, nbx = _images(_BDSD, "bdsd_moments", low_lp, low_pan, None, bs)
    _dense(_BDSD, "bdsd_moments", "low_ms", low_ms, (b, c, h, w))
    y = _f64("bdsd_moments", "out", out, (b, nby, nbx, c + 1, 2 * c + 1), low_lp.device)
    ws, nbytes = _lent("bdsd_moments", workspace, lib.tmdiff_bdsd_gram_workspace_bytes(b, c, h, w, int(bs or 0)),
                       lambda: bdsd_moments_workspace(b, c, h, w, low_lp.device, bs))
    check(lib.tmdiff_bdsd_gram(low_lp.detach().data_ptr(), low_pan.detach().data_ptr(), low_ms.detach().data_ptr(), b, c, h, w,
                               int(bs or 0), y.data_ptr(), ws.data_ptr(), nbytes, stream_ptr()), "bdsd_moments")
    return y


def bdsd_coeffs(moments, out=None):
    """The weights of BDSD (definition: ``metrics.bdsd_coeffs``): float64 [B, nby, nbx, C + 1, C] from ``moments``, the float64
    [B, nby, nbx, C + 1, 2 C + 1] device tensor of ``bdsd_moments``; column c solves N gamma_c = R[:, c] by a root-free unpivoted
    Cholesky factorisation on the device, one block per wave; a singular block gets NaN, the others are left alone.  Nothing is
    read on the host; with ``out=`` nothing is allocated."""
    if not (torch.is_tensor(moments) and moments.dim() == 5 and moments.shape[4] == 2 * moments.shape[3] - 1 and 2 <= moments.shape[3] <= 16):
        raise ValueError("bdsd_coeffs: moments must be a float64 [B, nby, nbx, C + 1, 2 C + 1] tensor on the GPU, 1 <= C <= 15")
    b, nby, nbx, k = moments.shape[:4]
    mo = _f64("bdsd_coeffs", "moments", moments, tuple(moments.shape), None)
    y = _f64("bdsd_coeffs", "out", out, (b, nby, nbx, k, k - 1), mo.device)
    if _overlaps(y, mo):
        raise ValueError("bdsd_coeffs: out overlaps moments")
    if b * nby * nbx > 2 ** 31 - 1:
        raise ValueError(f"bdsd_coeffs: {b * nby * nbx} blocks (fewer than 2^31)")
    check(lib.tmdiff_bdsd_solve(mo.detach().data_ptr(), y.data_ptr(), b * nby * nbx, k - 1, stream_ptr()), "bdsd_coeffs")
    return y


def bdsd_inject(ms_exp, pan, gamma, block=None, out=None):
    """The injection of BDSD (definition: ``metrics.bdsd_inject``): the fused [B, C, H, W] from ms_exp, pan and ``gamma``, the
    float64 [B, nby, nbx, C + 1, C] device tensor of ``bdsd_coeffs``: F_c = M_c + sum_k gamma[k, c] M_k + gamma[C, c] P with the
    weights of the block the pixel lies in (``block``: the full-scale side, None for one block), evaluated in fp64 and rounded to
    fp32 once.  ``out`` may be ms_exp itself (in place); it must not overlap pan or gamma.  With ``out=`` nothing is allocated or
    synchronised.  Not differentiable: the inputs are detached."""
    b, c, h, w, nby, nbx = _images(_BDSD, "bdsd_inject", ms_exp, pan, None, block)
    g = _f64("bdsd_inject", "gamma", gamma, (b, nby, nbx, c + 1, c), ms_exp.device)
    y = _inject_out(_BDSD, "bdsd_inject", out, ms_exp, ((pan, "pan"), (g, "gamma")))
    check(lib.tmdiff_bdsd_inject(ms_exp.detach().data_ptr(), pan.detach().data_ptr(), g.detach().data_ptr(), y.data_ptr(), b, c, h, w,
                                 int(block or 0), stream_ptr()), "bdsd_inject")
    return y


def bdsd_buffers(b, c, h, w, device, ratio=4, block=None):
    """Every scratch tensor of ``bdsd`` for [b, c, h, w] images: with them and ``out=`` a call allocates nothing and can be
    captured into a graph.  "ms_low", "lp_low", "pan_low": the reduced-scale MS, its low-pass and the reduced PAN; "moments",
    "gamma": the float64 normal equations and weights per block; "ws": the workspace of ``bdsd_moments``."""
    b, c, h, w, nby, nbx = _extents(_BDSD, "bdsd", b, c, h, w, ratio, block)
    f32, f64 = dict(device=device, dtype=torch.float32), dict(device=device, dtype=torch.float64)
    bs = None if block is None else int(block) // ratio
    return {"shape": (b, c, h, w, ratio, block), "ms_low": torch.empty(b, c, h // ratio, w // ratio, **f32),
            "lp_low": torch.empty(b, c, h // ratio, w // ratio, **f32), "pan_low": torch.empty(b, 1, h // ratio, w // ratio, **f32),
            "moments": torch.empty(b, nby, nbx, c + 1, 2 * c + 1, **f64), "gamma": torch.empty(b, nby, nbx, c + 1, c, **f64),
            "ws": bdsd_moments_workspace(b, c, h // ratio, w // ratio, device, bs)}


def bdsd(ms_exp, pan, sensor, ratio=4, block=None, lr_ms=None, out=None, buffers=None):
    """BDSD pansharpening on the device (definition: ``metrics.bdsd``): the fused [B, C, H, W] from ms_exp, the MS interpolated to
    the PAN grid, and pan [B, 1, H, W].  The reduced scale is made by the existing filters in float32: the reduced MS is ``lr_ms``
    [B, C, H / ratio, W / ratio], or with None the samples ms_exp[..., ratio // 2::ratio, ratio // 2::ratio] (the raw MS when ms_exp
    came from ``upsample_poly23``); its low-pass is ``fir_decimate`` with the MS bands' MTF table at ratio 1; the reduced PAN is
    ``mtf_degrade(pan, PAN gain of sensor, ratio)``.  ``bdsd_moments`` then leaves the normal equations of every block on the
    device, ``bdsd_coeffs`` solves them there and ``bdsd_inject`` writes the result.  ``block``: the full-scale side of the blocks
    that get weights of their own, a multiple of ``ratio`` that divides H and W; None fits one set to the whole image.
    ``sensor``: a name or a pair (MS gains, PAN gain), as ``metrics.mtf_gains`` takes them.  ``out`` may be ms_exp.  With
    ``buffers`` (``bdsd_buffers``) and ``out=`` nothing is allocated or synchronised; the tap tables are cached as ``mtf_degrade``
    caches its own: call once before capturing into a graph.  Not differentiable: the inputs are detached."""
    from . import metrics
    b, c, h, w, _, _ = _images(_BDSD, "bdsd", ms_exp, pan, ratio, block)
    ms_exp, pan = ms_exp.detach(), pan.detach()
    _chain_out(_BDSD, "bdsd", out, (b, c, h, w), ((pan, "pan"),))
    buf = _chain_buffers("bdsd", buffers, lambda: bdsd_buffers(b, c, h, w, ms_exp.device, ratio, block), (b, c, h, w, ratio, block),
                         "moments", ms_exp.device)
    ms_gains, pan_gain = metrics.mtf_gains(sensor, c)
    ms_low = _reduced_ms(_BDSD, "bdsd", ms_exp, lr_ms, ratio, buf["ms_low"])
    lp_low = fir_decimate(ms_low, _mtf_taps(ms_gains, ratio, ms_exp.device), 1, None, buf["lp_low"])
    pan_low = mtf_degrade(pan, pan_gain, ratio, out=buf["pan_low"])
    mo = bdsd_moments(lp_low, pan_low, ms_low, None if block is None else int(block) // ratio, out=buf["moments"], workspace=buf["ws"])
    return bdsd_inject(ms_exp, pan, bdsd_coeffs(mo, out=buf["gamma"]), block, out=out)


# ---- TV pansharpening: the variational row (csrc/tv.hip; definitions: tmdiff_amd/metrics.py) --------------------------------------
_TV_LIMITS = ("contiguous float32 tensors on the GPU, images [B, C, H, W], pan [B, 1, H, W]; weights None, [C + 1], [B, C + 1] or a "
              "float64 [B, C + 1] tensor on the GPU; 1 <= C <= 16; fewer than 2^31 elements")
_TV = _Family("x", 16, _TV_LIMITS)
_TV_WEIGHTS = {}        # (values, B, device) -> the uploaded float64 [B, C + 1] table; the last _TV_WEIGHTS_MAX of them
_TV_WEIGHTS_MAX = 8


def tv_supported(b, c, h, w):
    """True when ``tv_pd_step`` / ``tv_norm`` take [b, c, h, w] images: 1 <= c <= 16, h, w >= 1, fewer than 2^31 elements."""
    return bool(lib.tmdiff_tv_supported(int(b), int(c), int(h), int(w)))


def _tv_weights(name, weights, b, c, device):
    """(the float64 [B, C + 1] device table, its host copy or None): host values are uploaded once per (values, B, device)."""
    from . import metrics
    if torch.is_tensor(weights) and weights.is_cuda:
        return _f64(name, "weights", weights, (b, c + 1), device).detach(), None
    try:
        host = metrics.tv_weights(weights, b, c, name)
    except (TypeError, ValueError):
        raise ValueError(f"{name}: weights for {b} images of {c} bands ({_TV_LIMITS})") from None
    key = (host.tobytes(), b, device)
    table = _TV_WEIGHTS.get(key)
    if table is None:
        table = _TV_WEIGHTS[key] = torch.from_numpy(np.array(host)).to(device)
        while len(_TV_WEIGHTS) > _TV_WEIGHTS_MAX:
            del _TV_WEIGHTS[next(iter(_TV_WEIGHTS))]          # dicts keep insertion order: the oldest
    return table, host


def _tv_scalars(name, tau, sigma, lam, gamma):
    tau, sigma, lam, gamma = float(tau), float(sigma), float(lam), float(gamma)
    if not (tau > 0.0 and sigma >= 0.0 and lam >= 0.0 and gamma >= 0.0) or float("inf") in (tau, sigma, lam, gamma):
        raise ValueError(f"{name}: tau={tau} sigma={sigma} lam={lam} gamma={gamma} (tau > 0, the others >= 0, all finite)")
    return tau, sigma, lam, gamma


def tv_pd_step(u, x, ph, pv, pan, weights, tau, sigma, lam, gamma, out_x=None, out_p=None):
    """The band-coupled part of one Condat-Vu iteration of TV pansharpening (definition: ``metrics.tv_pd_step`` with
    storage=np.float32), one launch: with u = x - tau A^T (A x - lr_ms) made by the caller and s = sum_c w_c x_c + w_C - pan,
      x' = u - tau (gamma w_c s + D^T p);   q = p + sigma D (2 x' - x);   p' = q / max(1, |q| / lam)   (lam == 0: p' = 0)
    with |q| over the 2 C components of a pixel; fp64 after the loads, every stored value rounded once.  u, x, ph, pv [B, C, H, W],
    pan [B, 1, H, W]; ``weights``: None (1 / C per band, offset 0), a length C + 1 sequence or a [B, C + 1] array (uploaded once
    and kept), or a float64 [B, C + 1] tensor on the GPU.  Returns (x', ph', pv'); ``out_x`` and ``out_p`` = (ph', pv') receive
    them.  NO ALIASING: a workgroup computes x' on its tile plus one column and one row and reads p one pixel further, so every
    input is read where another workgroup stores; an output that overlaps an input or another output raises ValueError, and a
    loop ping-pongs x and p (``tv_pansharpen`` does).  With the outputs given nothing is allocated or synchronised (graph
    capture).  No atomics: the same bits on every run, and a batch equals its samples."""
    name = "tv_pd_step"
    b, c, h, w = _images(_TV, name, x, pan)[:4]
    for t, what in ((u, "u"), (ph, "ph"), (pv, "pv")):
        _dense(_TV, name, what, t, (b, c, h, w))
    tau, sigma, lam, gamma = _tv_scalars(name, tau, sigma, lam, gamma)
    wts, _ = _tv_weights(name, weights, b, c, x.device)
    xo = _dense(_TV, name, "out_x", out_x if out_x is not None else torch.empty_like(x), (b, c, h, w))
    if out_p is not None and len(out_p) != 2:
        raise ValueError(f"{name}: out_p is the pair (ph', pv')")
    pho, pvo = out_p if out_p is not None else (torch.empty_like(x), torch.empty_like(x))
    _dense(_TV, name, "out_p[0]", pho, (b, c, h, w))
    _dense(_TV, name, "out_p[1]", pvo, (b, c, h, w))
    ins = ((u, "u"), (x, "x"), (ph, "ph"), (pv, "pv"), (pan, "pan"), (wts, "weights"))
    outs = ((xo, "out_x"), (pho, "out_p[0]"), (pvo, "out_p[1]"))
    for i, (o, what) in enumerate(outs):
        for other, which in ins + outs[i + 1:]:
            if _overlaps(o, other):
                raise ValueError(f"{name}: {what} overlaps {which} (every input is read with a halo: ping-pong)")
    check(lib.tmdiff_tv_pd_step(u.detach().data_ptr(), x.detach().data_ptr(), pan.detach().data_ptr(), ph.detach().data_ptr(),
                                pv.detach().data_ptr(), wts.data_ptr(), tau, sigma, lam, gamma, xo.data_ptr(), pho.data_ptr(),
                                pvo.data_ptr(), b, c, h, w, stream_ptr()), name)
    return xo, pho, pvo


def tv_norm_workspace(b, c, h, w, device):
    """A workspace ``tv_norm`` accepts for [b, c, h, w] images (reusable; captured calls must keep it alive)."""
    b, c, h, w = _extents(_TV, "tv_norm", b, c, h, w)[:4]
    return torch.empty(max(1, lib.tmdiff_tv_norm_workspace_bytes(b, c, h, w) // 8), device=device, dtype=torch.float64)


def tv_norm(x, out=None, workspace=None):
    """The vector total variation per image (definition: ``metrics.tv_norm``): float64 [B] = sum over the pixels of
    sqrt(sum_c (Dh x_c)^2 + (Dv x_c)^2) for x [B, C, H, W], forward differences with a zero last column / row, no eps.  fp64
    after the loads; one partial sum per 16 x 32 tile in ``workspace``, added in a fixed order by a second launch: the same bits
    on every run.  With ``out=`` and ``workspace=`` (``tv_norm_workspace``) nothing is allocated or synchronised."""
    _dense(_TV, "tv_norm", "x", x)
    if x.dim() != 4:
        raise ValueError(f"tv_norm: x is {tuple(x.shape)}, need [B, C, H, W] ({_TV_LIMITS})")
    b, c, h, w = _extents(_TV, "tv_norm", *x.shape)[:4]
    y = _f64("tv_norm", "out", out, (b,), x.device)
    ws, nbytes = _lent("tv_norm", workspace, lib.tmdiff_tv_norm_workspace_bytes(b, c, h, w), lambda: tv_norm_workspace(b, c, h, w, x.device))
    check(lib.tmdiff_tv_norm(x.detach().data_ptr(), b, c, h, w, y.data_ptr(), ws.data_ptr(), nbytes, stream_ptr()), "tv_norm")
    return y


def tv_buffers(b, c, h, w, device, ratio=4):
    """Every scratch tensor of ``tv_pansharpen`` for [b, c, h, w] full-scale images: with them and ``out=`` a call allocates
    nothing and can be captured.  "x": the second scene of the ping-pong (the other is ``out``); "u": the scene after the
    gradient step on the data term; "p": the dual variable twice over, [2 (ping-pong), 2 (h, v), B, C, H, W]; "low", "r": A x and
    the residual at the reduced scale."""
    b, c, h, w = _extents(_TV, "tv_buffers", b, c, h, w, ratio)[:4]
    f32 = lambda *shape: torch.empty(shape, device=device, dtype=torch.float32)
    return {"shape": (b, c, h, w, ratio), "x": f32(b, c, h, w), "u": f32(b, c, h, w), "p": f32(2, 2, b, c, h, w),
            "low": f32(b, c, h // ratio, w // ratio), "r": f32(b, c, h // ratio, w // ratio)}


def tv_pansharpen(lr_ms, pan, sensor, ratio=4, iters=100, lam=1e-3, gamma=1.0, weights=None, x0=None, out=None, buffers=None):
    """TV pansharpening on the device (definition: ``metrics.tv_pansharpen`` with storage=np.float32): ``iters`` Condat-Vu
    iterations on  J = 1/2 ||A x - lr_ms||^2 + gamma/2 ||sum_c w_c x_c + w_C - pan||^2 + lam TV(x),  A = ``mtf_degrade(., sensor,
    ratio)``, for lr_ms [B, C, h, w] and pan [B, 1, ratio h, ratio w], started from ``upsample_poly23(lr_ms, ratio)`` unless ``x0``
    [B, C, ratio h, ratio w] is given, with p = 0 and the steps of ``metrics.tv_step_sizes``.  ``sensor``: a name or one gain per
    band (``metrics.band_gains``).  Four launches per iteration: ``fir_decimate``, ``add`` (the residual),
    ``fir_decimate_adjoint`` with base = x, alpha = -tau, beta = 1 into u, and ``tv_pd_step``, which ping-pongs x between ``out``
    and a buffer so that the last iterate lands in ``out``.  ``weights`` as ``tv_pd_step`` takes them; host values cost nothing
    per call, while a device tensor is read back once to size the steps (that synchronises: give host values to capture).
    ``lam`` = 1e-3 for data in [0, 1] is an UNTUNED default.  With ``buffers`` (``tv_buffers``) and ``out`` a call allocates
    nothing, reads nothing on the host and can be captured after one warm-up call (the tap table and the weights are cached on
    first use).  ``out`` may be ``x0``; it must not overlap anything else."""
    from . import metrics
    name = "tv_pansharpen"
    _dense(_TV, name, "lr_ms", lr_ms)
    if lr_ms.dim() != 4 or ratio not in (2, 4):
        raise ValueError(f"{name}: lr_ms is {tuple(lr_ms.shape)} at ratio {ratio}, need [B, C, h, w] and ratio 2 or 4 ({_TV_LIMITS})")
    if int(iters) != iters or iters < 0:
        raise ValueError(f"{name}: iters={iters} (a whole number >= 0)")
    b, c, h, w = _extents(_TV, name, lr_ms.shape[0], lr_ms.shape[1], ratio * lr_ms.shape[2], ratio * lr_ms.shape[3], ratio)[:4]
    _dense(_TV, name, "pan", pan, (b, 1, h, w))
    lr, pan, iters = lr_ms.detach(), pan.detach(), int(iters)
    gains = metrics.band_gains(sensor, c)
    wts, host = _tv_weights(name, weights, b, c, lr.device)
    tau, sigma = metrics.tv_step_sizes(gains, ratio, host if host is not None else wts.cpu().numpy(), gamma)
    tau, sigma, lam, gamma = _tv_scalars(name, tau, sigma, lam, gamma)
    others = [(pan, "pan"), (lr, "lr_ms"), (wts, "weights")]
    if x0 is not None:
        _dense(_TV, name, "x0", x0, (b, c, h, w))
        x0 = x0.detach()
    y = _chain_out(_TV, name, out if out is not None else torch.empty(b, c, h, w, device=lr.device), (b, c, h, w), others)
    if x0 is not None and y.data_ptr() != x0.data_ptr() and _overlaps(y, x0):
        raise ValueError(f"{name}: out overlaps x0 without being x0")
    buf = _chain_buffers(name, buffers, lambda: tv_buffers(b, c, h, w, lr.device, ratio), (b, c, h, w, ratio), "x", lr.device)
    taps = _mtf_taps(gains, ratio, lr.device)
    xs = (y, buf["x"]) if iters % 2 == 0 else (buf["x"], y)               # iterate k lives in xs[k % 2]: the last one in out
    if x0 is None:
        upsample_poly23(lr, ratio, out=xs[0])
    elif xs[0].data_ptr() != x0.data_ptr():
        xs[0].copy_(x0)
    if iters:
        buf["p"][0].zero_()
    for k in range(iters):
        x, (ph, pv) = xs[k % 2], buf["p"][k % 2]
        fir_decimate(x, taps, ratio, None, buf["low"])
        add(buf["low"], lr, -1.0, out=buf["r"])
        fir_decimate_adjoint(buf["r"], taps, (h, w), ratio, None, buf["u"], x, -tau, 1.0)
        tv_pd_step(buf["u"], x, ph, pv, pan, wts, tau, sigma, lam, gamma, out_x=xs[(k + 1) % 2], out_p=tuple(buf["p"][(k + 1) % 2]))
    return y


# ---- a-trous wavelet pansharpening: ATWT and AWLP (csrc/atrous.hip; definitions: tmdiff_amd/metrics.py) ---------------------------
_AWLP_LIMITS = ("contiguous float32 tensors on the GPU, ms_exp [B, C, H, W], pan and pan_lp [B, 1, H, W]; 1 <= C <= 14; ratio 2 or 4; "
                "fewer than 2^31 elements")
_AWLP = _Family("ms_exp", 14, _AWLP_LIMITS)
_ATROUS_LIMITS = ("a contiguous float32 [B, C, H, W] or [B, H, W] tensor on the GPU; B, C, H, W >= 1, H, W <= 2^30, fewer than 2^31 "
                  "elements; first, levels >= 1, first + levels <= 4")


def atrous_supported(b, c, h, w, levels=2, first=1):
    """True when ``atrous_lowpass`` takes [b, c, h, w] images at ``levels`` from ``first``: every extent >= 1, fewer than 2^31
    elements, first and levels >= 1, first + levels <= 4."""
    return bool(lib.tmdiff_atrous_supported(int(b), int(c), int(h), int(w), int(levels), int(first)))


def atrous_lowpass(x, levels=2, out=None, first=1):
    """The approximation plane of the a-trous transform of every plane of x [B, C, H, W], [B, 1, H, W] or [B, H, W] (definition:
    ``metrics.atrous_lowpass`` with storage=np.float32): ``levels`` (1 .. 3) passes of the separable B3 filter (1, 4, 6, 4, 1) / 16
    with its taps 2^(l-1) apart, indices clamped into the plane at every level; fp64 after the loads, every level rounded to
    fp32 once.  All levels run in ONE launch on a tile staged with its halo of 2 (2^levels - 1) pixels, and equal ``levels``
    single-level calls bit for bit: ``first`` > 1 takes x for c_{first-1} and runs the levels first .. first + levels - 1, so
    ``atrous_lowpass(atrous_lowpass(x, 1), 1, first=2)`` is ``atrous_lowpass(x, 2)``.  Returns a tensor of x's shape.  x is read with a halo that other workgroups own: ``out`` must
    not overlap x (ValueError).  With ``out=`` nothing is allocated or synchronised (graph capture).  No atomics: the same bits
    on every run, and a batch equals its samples.  Not differentiable: x is detached."""
    from . import metrics
    name = "atrous_lowpass"
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() in (3, 4)):
        raise ValueError(f"{name}: x must be {_ATROUS_LIMITS}")
    try:
        levels, first = metrics._atrous_levels(name, levels, first)
    except TypeError:
        raise ValueError(f"{name}: levels={levels!r} first={first!r} (whole numbers >= 1, first + levels <= 4)") from None
    x = x.detach()
    b, c, (h, w) = x.shape[0], (x.shape[1] if x.dim() == 4 else 1), x.shape[-2:]
    if not lib.tmdiff_atrous_supported(b, c, h, w, levels, first):
        raise ValueError(f"{name}: x {tuple(x.shape)} levels={levels} is not supported ({_ATROUS_LIMITS})")
    y = out if out is not None else torch.empty_like(x)
    if not (torch.is_tensor(y) and y.is_cuda and y.dtype == torch.float32 and y.is_contiguous() and y.shape == x.shape
            and y.device == x.device):
        raise ValueError(f"{name}: out must be a contiguous float32 {tuple(x.shape)} tensor on x's device")
    if _overlaps(y, x):
        raise ValueError(f"{name}: out overlaps x (x is read with a halo that other workgroups own)")
    check(lib.tmdiff_atrous_lowpass(x.data_ptr(), y.data_ptr(), b, c, h, w, levels, first, stream_ptr()), name)
    return y


def _awlp_mode(name, mode):
    from . import metrics
    if mode not in metrics.ATROUS_MODES:
        raise ValueError(f"{name}: mode={mode!r} (one of {metrics.ATROUS_MODES})")
    return metrics.ATROUS_MODES.index(mode)


def awlp_inject(ms_exp, pan, pan_lp, moments, mode, out=None):
    """The injection of a-trous wavelet pansharpening (definition: ``metrics.awlp_inject``): the fused [B, C, H, W] from ms_exp, pan
    and pan_lp [B, 1, H, W] -- ONE low-pass plane per image -- and ``moments``, the float64 [B, C + 1, C + 2] device tensor of
    ``plane_moments(ms_exp, pan_lp)``.  With a_c = sqrt(var(M_c) / var(L)) formed on the device from the moments' diagonal
    (nothing is read on the host), D = P - L and I = (sum_k M_k) / C:
      "atwt":  F_c = M_c + a_c D          "awlp":  F_c = M_c + ((M_c / I) a_c) D,  and F_c = M_c where I == 0
    in fp64, rounded to fp32 once; a constant pan_lp gives a non-finite result throughout.  ``out`` may be ms_exp itself (in
    place: a lane reads all bands of its pixels before it stores any); it must not overlap pan, pan_lp or moments.  With ``out=``
    nothing is allocated or synchronised.  Not differentiable: the inputs are detached."""
    name = "awlp_inject"
    m = _awlp_mode(name, mode)
    b, c, h, w = _images(_AWLP, name, ms_exp, pan)[:4]
    _dense(_AWLP, name, "pan_lp", pan_lp, (b, 1, h, w))
    mo = _f64(name, "moments", moments, (b, c + 1, c + 2), ms_exp.device)
    y = _inject_out(_AWLP, name, out, ms_exp, ((pan, "pan"), (pan_lp, "pan_lp"), (mo, "moments")))
    check(lib.tmdiff_awlp_inject(ms_exp.detach().data_ptr(), pan.detach().data_ptr(), pan_lp.detach().data_ptr(), mo.detach().data_ptr(),
                                 y.data_ptr(), b, c, h, w, m, stream_ptr()), name)
    return y


def awlp_buffers(b, c, h, w, device, ratio=4):
    """Every scratch tensor of ``awlp`` for [b, c, h, w] images: with them and ``out=`` a call allocates nothing and can be captured
    into a graph.  "pan_lp": the a-trous low-pass PAN [b, 1, h, w]; "moments": the float64 [b, c + 1, c + 2] moments of the bands
    and that plane; "ws": the workspace of ``plane_moments``."""
    b, c, h, w = _extents(_AWLP, "awlp_buffers", b, c, h, w)[:4]
    if ratio not in (2, 4):
        raise ValueError(f"awlp_buffers: ratio={ratio} is not supported ({_AWLP_LIMITS})")
    return {"shape": (b, c, h, w, ratio), "pan_lp": torch.empty(b, 1, h, w, device=device, dtype=torch.float32),
            "moments": torch.empty(b, c + 1, c + 2, device=device, dtype=torch.float64), "ws": plane_moments_workspace(b, c, h, w, device)}


def awlp(ms_exp, pan, ratio=4, mode="awlp", out=None, buffers=None):
    """A-trous wavelet pansharpening on the device (definition: ``metrics.awlp`` with storage=np.float32): the fused [B, C, H, W]
    from ms_exp, the MS interpolated to the PAN grid, and pan [B, 1, H, W]; ``mode`` "atwt" (additive) or "awlp" (proportional,
    Otazu et al. 2005).  Three launches and a finalize: ``atrous_lowpass(pan, log2(ratio))`` makes the one low-pass plane L,
    ``plane_moments(ms_exp, L)`` leaves the variances on the device, ``awlp_inject`` forms the gains there and writes the result.
    No sensor is involved.  ``out`` may be ms_exp.  With ``buffers`` (``awlp_buffers``) and ``out=`` nothing is allocated or
    synchronised and the call can be captured into a graph.  Not differentiable: the inputs are detached."""
    name = "awlp"
    _awlp_mode(name, mode)
    b, c, h, w = _images(_AWLP, name, ms_exp, pan)[:4]
    if ratio not in (2, 4):
        raise ValueError(f"{name}: ratio={ratio} is not supported ({_AWLP_LIMITS})")
    ms_exp, pan = ms_exp.detach(), pan.detach()
    _chain_out(_AWLP, name, out, (b, c, h, w), ((pan, "pan"),))
    buf = _chain_buffers(name, buffers, lambda: awlp_buffers(b, c, h, w, ms_exp.device, ratio), (b, c, h, w, ratio), "pan_lp",
                         ms_exp.device)
    low = atrous_lowpass(pan, 1 if ratio == 2 else 2, out=buf["pan_lp"])
    mo = plane_moments(ms_exp, low, out=buf["moments"], workspace=buf["ws"])
    return awlp_inject(ms_exp, pan, low, mo, mode, out=out)


# ---- backward-side wrappers (finetune path) -----------------------------------------------------------


def wgrad_wino_takes(desc):
    """True when conv3d_wgrad runs this weight gradient in the Winograd domain (its g pass then sums the bias gradient on
    the side for free): routing.wgrad_family's answer for the descriptor's extents, segments and prologue."""
    pro = bool(desc.in_act or desc.in_shift or desc.in_scale or desc.in_mask or desc.drop_p > 0.0)
    return routing.wgrad_family(desc.B, tuple(desc.seg_c[:desc.nseg]), desc.Cout, desc.N, desc.H, desc.W, desc.groups, desc.ksize, pro,
                                **({"x_bf16": 1} if desc.x_bf16 else {})) == "wino"


def _wgrad(entry, workspace_query, desc, g, weight_shape, want_bias, count_key, flops):
    """The host path of every weight-gradient kernel: dw (with want_bias: (dw, db)) from lib.<entry>(desc, g, dw, db or NULL,
    workspace, stream) on a workspace of lib.<workspace_query>(desc) bytes; counted as count_key with `flops` executed FLOPs."""
    dw = torch.empty(weight_shape, device=g.device, dtype=torch.float32)
    _count(count_key, flops)
    ws = _workspace(g.device, max(16, getattr(lib, workspace_query)(C.byref(desc))), "wgrad")
    db = torch.empty(weight_shape[0], device=g.device, dtype=torch.float32) if want_bias else None
    check(getattr(lib, entry)(C.byref(desc), _chk(g, "g"), dw.data_ptr(), _chk(db, "db"), ws.data_ptr(), stream_ptr()), count_key)
    return (dw, db) if want_bias else dw


def conv3d_wgrad(desc, g, weight_shape, want_bias=False, family=None):
    """dL/dw [Cout, Cin/g, k,k,k] for the convolution described by `desc` (a filled Conv3dDesc) given g = dL/dy; with
    want_bias also dL/dbias = desc.bias_scale * sum_{b,pos} g, accumulated inside the same kernel: returns (dw, dbias).
    family: "wino" / "direct", the kernel a routing plan has chosen (plan.wgrad); None asks routing here (wgrad_wino_takes).
    family="wino" on a convolution the Winograd kernel does not take raises ValueError before anything is allocated or counted."""
    if family is None:
        family = "wino" if wgrad_wino_takes(desc) else "direct"
    elif family == "wino" and not lib.tmdiff_conv3d_wgrad_wino_supported(C.byref(desc)):
        raise ValueError("conv3d_wgrad: family='wino' needs fp32 3x3x3, groups 1 or 3, N % 4 == 0 (at most 16), W % 4 == 0")
    macs = desc.B * desc.Cout * (desc.Cin // desc.groups) * desc.N * desc.H * desc.W
    if family == "wino":
        # Winograd F(3,4) along the bands (csrc/wgrad_wino.hip): 13.5 executed multiply-adds per element instead of 27
        return _wgrad("tmdiff_conv3d_wgrad_wino_bias", "tmdiff_conv3d_wgrad_wino_workspace_bytes", desc, g, weight_shape, want_bias,
                      "conv3d_wgrad_wino", 2.0 * macs * 13.5)
    if family != "direct":
        raise ValueError(f"conv3d_wgrad: family={family!r} (wino, direct or None)")
    return _wgrad("tmdiff_conv3d_wgrad_bias", "tmdiff_conv3d_wgrad_workspace_bytes", desc, g, weight_shape, want_bias,
                  "conv3d_wgrad", 2.0 * macs * desc.ksize ** 3)


def wgrad_bf16_supported(desc):
    """True when tmdiff_conv3d_wgrad_bf16 takes the descriptor (3x3x3, groups 1 or 3, Cin/groups % 8 == 0, Cout/groups % 32 == 0)."""
    return bool(lib.tmdiff_conv3d_wgrad_bf16_supported(C.byref(desc)))


def conv3d_wgrad_bf16(desc, g, weight_shape, want_bias=False):
    """conv3d_wgrad with bf16 operands: g and the prologue output x' of `desc` rounded to bf16 (nearest even), products summed
    in fp32 (csrc/wgrad_bf16.hip; deterministic).  want_bias: also dL/dbias = desc.bias_scale * sum g of the unrounded g.
    A descriptor the kernel does not take raises (TMDIFF_E_UNSUPPORTED): ask wgrad_bf16_supported / routing first."""
    return _wgrad("tmdiff_conv3d_wgrad_bf16", "tmdiff_conv3d_wgrad_bf16_workspace_bytes", desc, g, weight_shape, want_bias,
                  "conv3d_wgrad_bf16", 2.0 * desc.B * desc.Cout * (desc.Cin // max(desc.groups, 1)) * 27 * desc.N * desc.H * desc.W)


def channel_sum(x, scale=1.0):
    """x [B, C, ...] -> [C]: scale * sum over batch and positions."""
    b, c = x.shape[:2]
    out = torch.empty(c, device=x.device, dtype=torch.float32)
    check(lib.tmdiff_channel_sum(_chk(x, "x"), out.data_ptr(), b, c, math.prod(x.shape[2:]), scale, stream_ptr()),
          "channel_sum")
    return out


def conv3d_prologue_bwd(desc, gp, dx_segs, accumulate, want_shift, want_scale, add_segs=None):
    """dL/dx (per segment, into dx_segs; accumulate[i]: added to what dx_segs[i] holds), dL/dshift, dL/dscale of a convolution's
    prologue from dL/dx'.  add_segs (then accumulate must be all False): dx_segs[i] = add_segs[i] + dL/dx_i -- another consumer's
    gradient of the same segment, only read (tmdiff_conv3d_prologue_bwd_add)."""
    b, cin = desc.B, desc.Cin
    d_shift = torch.empty(b, cin, device=gp.device, dtype=torch.float32) if want_shift else None
    d_scale = torch.empty(b, cin, device=gp.device, dtype=torch.float32) if want_scale else None
    dxp = (C.c_void_p * 3)(*[_chk(t, "dx") for t in dx_segs], *([None] * (3 - len(dx_segs))))
    acc = (C.c_int32 * 3)(*[1 if a else 0 for a in accumulate], *([0] * (3 - len(accumulate))))
    nws = lib.tmdiff_conv3d_prologue_bwd_workspace_bytes(C.byref(desc))
    ws = _workspace(gp.device, nws, "prologue_bwd").data_ptr() if nws else None
    if add_segs is not None:
        if any(accumulate):
            raise ValueError("conv3d_prologue_bwd: add_segs goes with accumulate all False")
        addp = (C.c_void_p * 3)(*[_chk(t, "add") for t in add_segs], *([None] * (3 - len(add_segs))))
        check(lib.tmdiff_conv3d_prologue_bwd_add(C.byref(desc), _chk(gp, "gp"), dxp, addp, _chk(d_shift, "d_shift"),
                                                 _chk(d_scale, "d_scale"), ws, stream_ptr()), "conv3d_prologue_bwd_add")
        return d_shift, d_scale
    check(lib.tmdiff_conv3d_prologue_bwd_ws(C.byref(desc), _chk(gp, "gp"), dxp, acc, _chk(d_shift, "d_shift"),
                                            _chk(d_scale, "d_scale"), ws, stream_ptr()), "conv3d_prologue_bwd")
    return d_shift, d_scale


def stem_bwd(w, bias, gy, xin=None, pan=None, ms=None):
    b, c0, n, h, wd = gy.shape
    dwb = torch.empty(b, c0, 2, device=gy.device, dtype=torch.float32)
    check(lib.tmdiff_stem_bwd(_chk(xin, "xin"), _chk(pan, "pan"), _chk(ms, "ms"), _chk(w, "w"), _chk(bias, "bias"),
                              _chk(gy, "gy"), dwb.data_ptr(), b, c0, n, h, wd, stream_ptr()), "stem_bwd")
    return dwb


def stem_bwd_input(w, bias, gy, xin=None, pan=None, ms=None, need_x=True, need_pan=False):
    """Gradients w.r.t. the stem's inputs: (d_xin, None) or (d_ms, d_pan)."""
    b, c0, n, h, wd = gy.shape
    dx = torch.empty(b, n, h, wd, device=gy.device, dtype=torch.float32) if need_x else None
    dpan = torch.empty(b, 1, h, wd, device=gy.device, dtype=torch.float32) if (need_pan and ms is not None) else None
    check(lib.tmdiff_stem_bwd_input(_chk(xin, "xin"), _chk(pan, "pan"), _chk(ms, "ms"), _chk(w, "w"), _chk(bias, "bias"),
                                    _chk(gy, "gy"), _chk(dx, "dx"), _chk(dpan, "dpan"), b, c0, n, h, wd, stream_ptr()),
          "stem_bwd_input")
    return dx, dpan


def head_bwd(x, w, scale, gy, need_dx=True):
    b, c, n, h, wd = x.shape
    dx = torch.empty_like(x) if need_dx else None
    dws = torch.empty(b, c, device=x.device, dtype=torch.float32)
    check(lib.tmdiff_head_bwd(_chk(x, "x"), _chk(w, "w"), _chk(scale, "scale"), _chk(gy, "gy"), _chk(dx, "dx"),
                              dws.data_ptr(), b, c, n * h * wd, stream_ptr()), "head_bwd")
    return dx, dws


def linear_bwd(x, w, bias, gy, act=False, need_dx=True, need_dw=True, need_db=True):
    b, i = x.shape
    o = w.shape[0]
    dx = torch.empty(b, i, device=x.device, dtype=torch.float32) if need_dx else None
    new = torch.zeros if b == 0 else torch.empty       # (no rows: the kernels do not run, the sums over them are 0)
    dw = new(o, i, device=x.device, dtype=torch.float32) if need_dw else None
    db = new(o, device=x.device, dtype=torch.float32) if need_db else None
    gu = torch.empty(b, o, device=x.device, dtype=torch.float32) if act else None
    check(lib.tmdiff_linear_bwd(_chk(x, "x"), _chk(w, "w"), _chk(bias, "bias"), _chk(gy, "gy"), _chk(gu, "gu"),
                                _chk(dx, "dx"), _chk(dw, "dw"), _chk(db, "db"), b, i, o, 1 if act else 0,
                                stream_ptr()), "linear_bwd")
    return dx, dw, db


# ---- standalone attention operators (core/Attention.py) ----------------------------------------------------
def attention(q, k, v, scale, heads=1, key_mask=None, layout="bnd"):
    """softmax(q k^T * scale) v.  layout 'bnd': q [B, Nq, H*D], k/v [B, Nk, H*D] (heads split along the last
    dim, as CrossAttention's 'b n (h d)'); returns [B, Nq, H*D]."""
    assert layout == "bnd"
    b, nq, hd = q.shape
    nk = k.shape[1]
    d = hd // heads
    out = torch.empty_like(q)
    st = lambda n: (C.c_int64 * 3)(n * hd, d, hd)          # batch, head, row strides in elements
    m = None
    if key_mask is not None:
        m = key_mask.to(device=q.device, dtype=torch.uint8).contiguous()
    check(lib.tmdiff_attn_fwd(_chk(q, "q"), _chk(k, "k"), _chk(v, "v"), out.data_ptr(),
                              m.data_ptr() if m is not None else None, b, heads, nq, nk, d, st(nq), st(nk), st(nk),
                              st(nq), scale, stream_ptr()), "attn_fwd")
    return out


def _attn_extents(q, k, heads):
    b, nq, hd = q.shape
    nk, d = k.shape[1], hd // heads
    st = lambda n: (C.c_int64 * 3)(n * hd, d, hd)          # batch, head, row strides in elements
    return b, nq, nk, d, st(nq), st(nk)


def _key_mask(key_mask, device):
    return None if key_mask is None else key_mask.to(device=device, dtype=torch.uint8).contiguous()


def attention_lse(q, k, v, scale, heads=1, key_mask=None):
    """attention() for the differentiable path: (out, lse), lse [B, heads, Nq] = logsumexp of the scaled (masked) scores.
    `out` equals attention()'s bit for bit (the same kernels, instantiated once more with the store of lse)."""
    b, nq, nk, d, sq, sk = _attn_extents(q, k, heads)
    out = torch.empty_like(q)
    lse = torch.empty(b, heads, nq, device=q.device, dtype=torch.float32)
    m = _key_mask(key_mask, q.device)
    check(lib.tmdiff_attn_fwd_lse(_chk(q, "q"), _chk(k, "k"), _chk(v, "v"), out.data_ptr(),
                                  m.data_ptr() if m is not None else None, b, heads, nq, nk, d, sq, sk, sk, sq, scale,
                                  lse.data_ptr(), stream_ptr()), "attn_fwd_lse")
    return out, lse


def attention_bwd(q, k, v, out, dout, lse, scale, heads=1, key_mask=None, need=(True, True, True)):
    """(dq, dk, dv) of attention_lse from dout; None where `need` is False.  No atomics: bitwise reproducible."""
    b, nq, nk, d, sq, sk = _attn_extents(q, k, heads)
    if not lib.tmdiff_attn_bwd_supported(b, heads, nq, nk, d):
        raise ValueError(f"attention_bwd: extents B={b} H={heads} Nq={nq} Nk={nk} D={d} are not supported")
    dq = torch.empty_like(q) if need[0] else None
    dk = torch.empty_like(k) if need[1] else None
    dv = torch.empty_like(v) if need[2] else None
    ws = _workspace(q.device, lib.tmdiff_attn_bwd_workspace_bytes(b, heads, nq, nk, d), "attn_bwd")
    m = _key_mask(key_mask, q.device)
    check(lib.tmdiff_attn_bwd(_chk(q, "q"), _chk(k, "k"), _chk(v, "v"), _chk(out, "out"), _chk(dout, "dout"), _chk(lse, "lse"),
                              m.data_ptr() if m is not None else None, _chk(dq, "dq"), _chk(dk, "dk"), _chk(dv, "dv"),
                              ws.data_ptr(), b, heads, nq, nk, d, sq, sk, sk, sq, scale, stream_ptr()), "attn_bwd")
    return dq, dk, dv


def gemm_nt(a, w, bias=None, residual=None):
    """a [..., K] @ w[N, K]^T + bias + residual -> [..., N]"""
    k = a.shape[-1]
    n = w.shape[0]
    out = torch.empty(*a.shape[:-1], n, device=a.device, dtype=torch.float32)
    m = out[..., 0].numel() if n else 0                    # rows: the leading dims folded (K = 0 / N = 0 are the library's to refuse)
    check(lib.tmdiff_gemm_nt(_chk(a, "a"), _chk(w, "w"), _chk(bias, "bias"), _chk(residual, "residual"),
                             out.data_ptr(), m, n, k, stream_ptr()), "gemm_nt")
    return out


def group_norm(x, gamma, beta, groups=32, eps=1e-6):
    b, c = x.shape[:2]
    y = torch.empty_like(x)
    check(lib.tmdiff_group_norm(_chk(x, "x"), _chk(gamma, "gamma"), _chk(beta, "beta"), y.data_ptr(), b, c,
                                x.numel() // (b * c), groups, eps, stream_ptr()), "group_norm")
    return y


def layer_norm(x, gamma, beta, eps=1e-5):
    d = x.shape[-1]
    y = torch.empty_like(x)
    check(lib.tmdiff_layer_norm(_chk(x, "x"), _chk(gamma, "gamma"), _chk(beta, "beta"), y.data_ptr(),
                                x.numel() // d, d, eps, stream_ptr()), "layer_norm")
    return y


def geglu(u, gelu_only=False):
    inner = u.shape[-1] if gelu_only else u.shape[-1] // 2
    y = torch.empty(*u.shape[:-1], inner, device=u.device, dtype=torch.float32)
    check(lib.tmdiff_geglu(_chk(u, "u"), y.data_ptr(), u.numel() // u.shape[-1], inner, 1 if gelu_only else 0,
                           stream_ptr()), "geglu")
    return y


# ---- the differentiable path of the norm / GEGLU operators (csrc/norm_bwd.hip) ---------------------------------
def layer_norm_stats(x, gamma, beta, eps=1e-5):
    """layer_norm() for the differentiable path: (y, mean, rstd), the statistics per row.  `y` equals layer_norm()'s bit for
    bit (the same kernel, instantiated once more with the store of the statistics)."""
    d = x.shape[-1]
    rows = x.numel() // d
    y = torch.empty_like(x)
    mean = torch.empty(rows, device=x.device, dtype=torch.float32)
    rstd = torch.empty(rows, device=x.device, dtype=torch.float32)
    check(lib.tmdiff_layer_norm_stats(_chk(x, "x"), _chk(gamma, "gamma"), _chk(beta, "beta"), y.data_ptr(), mean.data_ptr(),
                                      rstd.data_ptr(), rows, d, eps, stream_ptr()), "layer_norm_stats")
    return y, mean, rstd


def group_norm_stats(x, gamma, beta, groups=32, eps=1e-6):
    """group_norm() for the differentiable path: (y, mean, rstd), the statistics [B, groups]; `y` as group_norm()'s."""
    b, c = x.shape[:2]
    y = torch.empty_like(x)
    mean = torch.empty(b, groups, device=x.device, dtype=torch.float32)
    rstd = torch.empty(b, groups, device=x.device, dtype=torch.float32)
    check(lib.tmdiff_group_norm_stats(_chk(x, "x"), _chk(gamma, "gamma"), _chk(beta, "beta"), y.data_ptr(), mean.data_ptr(),
                                      rstd.data_ptr(), b, c, x.numel() // (b * c), groups, eps, stream_ptr()), "group_norm_stats")
    return y, mean, rstd


def layer_norm_bwd(x, gamma, dy, mean, rstd, need=(True, True, True)):
    """(dx, dgamma, dbeta) of layer_norm_stats from dy; None where `need` is False.  No atomics: bitwise reproducible."""
    d = x.shape[-1]
    rows = x.numel() // d
    if not lib.tmdiff_layer_norm_bwd_supported(rows, d):
        raise ValueError(f"layer_norm_bwd: extents rows={rows} D={d} are not supported")
    dx = torch.empty_like(x) if need[0] else None
    dgamma = torch.empty(d, device=x.device, dtype=torch.float32) if need[1] else None
    dbeta = torch.empty(d, device=x.device, dtype=torch.float32) if need[2] else None
    nws = lib.tmdiff_layer_norm_bwd_workspace_bytes(rows, d) if (need[1] or need[2]) else 0
    ws = _workspace(x.device, nws, "norm_bwd").data_ptr() if nws else None
    check(lib.tmdiff_layer_norm_bwd(_chk(x, "x"), _chk(gamma, "gamma"), _chk(dy, "dy"), _chk(mean, "mean"), _chk(rstd, "rstd"),
                                    _chk(dx, "dx"), _chk(dgamma, "dgamma"), _chk(dbeta, "dbeta"), ws, rows, d, stream_ptr()),
          "layer_norm_bwd")
    return dx, dgamma, dbeta


def group_norm_bwd(x, gamma, dy, mean, rstd, groups=32, need=(True, True, True)):
    """(dx, dgamma, dbeta) of group_norm_stats from dy (gamma None = 1); None where `need` is False.  No atomics."""
    b, c = x.shape[:2]
    p = x.numel() // (b * c) if b * c else 0
    if not lib.tmdiff_group_norm_bwd_supported(b, c, p, groups):
        raise ValueError(f"group_norm_bwd: extents B={b} C={c} P={p} groups={groups} are not supported")
    dx = torch.empty_like(x) if need[0] else None
    dgamma = torch.empty(c, device=x.device, dtype=torch.float32) if need[1] else None
    dbeta = torch.empty(c, device=x.device, dtype=torch.float32) if need[2] else None
    nws = lib.tmdiff_group_norm_bwd_workspace_bytes(b, c, p, groups) if (need[1] or need[2]) else 0
    ws = _workspace(x.device, nws, "norm_bwd").data_ptr() if nws else None
    check(lib.tmdiff_group_norm_bwd(_chk(x, "x"), _chk(gamma, "gamma"), _chk(dy, "dy"), _chk(mean, "mean"), _chk(rstd, "rstd"),
                                    _chk(dx, "dx"), _chk(dgamma, "dgamma"), _chk(dbeta, "dbeta"), ws, b, c, p, groups,
                                    stream_ptr()), "group_norm_bwd")
    return dx, dgamma, dbeta


def geglu_bwd(u, dy, gelu_only=False):
    """du of geglu(u, gelu_only) from dy: [..., 2 * inner] (or [..., inner] with gelu_only)."""
    inner = u.shape[-1] if gelu_only else u.shape[-1] // 2
    du = torch.empty_like(u)
    check(lib.tmdiff_geglu_bwd(_chk(u, "u"), _chk(dy, "dy"), du.data_ptr(), u.numel() // u.shape[-1], inner,
                               1 if gelu_only else 0, stream_ptr()), "geglu_bwd")
    return du
