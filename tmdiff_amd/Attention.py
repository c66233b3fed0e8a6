"""The attention operators of the reference's core/Attention.py on the HIP kernels.

Every module here is trainable: ``CrossAttention`` (with ``mask``, ``context=None`` and ``residual``), ``GEGLU``, ``FeedForward``,
``SpatialSelfAttention``, ``BasicTransformerBlock``, ``SpatialTransformer`` and ``AttnBlockpp``.  Each ``forward`` dispatches as
``CrossAttention.forward`` does: under ``torch.no_grad()``, or when neither a parameter nor an input requires grad, the
inference path; otherwise the differentiable path -- the same kernels in the same order, wrapped in the autograd Functions of
``autograd`` (``gemm_nt``, ``AttentionFn``: tmdiff_attn_fwd_lse / tmdiff_attn_bwd, ``layer_norm`` / ``group_norm``: the *_stats
forwards and tmdiff_layer_norm_bwd / tmdiff_group_norm_bwd, ``geglu``: tmdiff_geglu_bwd, ``conv1x1``: the 1x1 convolution's
data and weight gradients), with differentiable torch views / copies for the reshapes and transposes between them.  Its output
equals the inference path's bit for bit.  ``BasicTransformerBlock`` hands its inputs to its ``CrossAttention`` layers, which
dispatch themselves.  Dropout inside the blocks has no differentiable path: ``nn.Dropout`` with ``p > 0`` in training mode raises
``NotImplementedError`` (the reference configurations all use ``p = 0``); the reference's ``checkpoint=True`` is ignored (no
recomputation).

``core/Attention.py`` is imported by nothing in TMDiff and WavBEST contains no attention layer;
these classes exist because BASELINE's north star names them.  Module tree and parameter names follow the
reference (GEGLU :69-76, FeedForward :79-96, SpatialSelfAttention :112-162, CrossAttention :165-214,
BasicTransformerBlock :266-296, SpatialTransformer :299-362), so its state_dicts load; ``NIN`` / ``AttnBlockpp`` are
the DDPM++ attention block that GeneralModel/Hyper_unet_general.py defines (:471-515) and never instantiates.  Only the vanilla softmax
path exists (the reference falls back to it when xformers is absent, :31-35, :267-274).  nn.Linear / nn.Conv2d /
norm modules are parameter containers: the arithmetic is tmdiff_gemm_nt, tmdiff_conv3d_fwd (1x1), tmdiff_attn_fwd,
tmdiff_group_norm, tmdiff_layer_norm, tmdiff_geglu.
"""
import torch
from torch import nn

from . import autograd, ops


def _conv1x1(conv, x, residual=None):
    """nn.Conv2d(kernel 1) on [B, C, H, W] through the conv3d MFMA kernel (N = 1)."""
    b, c, h, w = x.shape
    wt = conv.weight.detach().reshape(conv.out_channels, c, 1, 1, 1).contiguous()
    wp = ops.pack_conv_weight(wt)
    res = None if residual is None else residual.reshape(b, conv.out_channels, 1, h, w)
    y = ops.conv3d([x.reshape(b, c, 1, h, w)], wp, conv.out_channels, 1,
                   bias=conv.bias.detach() if conv.bias is not None else None, residual=res)
    return y.reshape(b, conv.out_channels, h, w)


def _linear(lin, x, residual=None):
    return ops.gemm_nt(x.contiguous(), lin.weight.detach(), lin.bias.detach() if lin.bias is not None else None,
                       residual)


def _wants_grad(module, *tensors):
    """The dispatch of every forward here: grad mode on, and a parameter of `module` or one of `tensors` requires grad."""
    return torch.is_grad_enabled() and (any(p.requires_grad for p in module.parameters()) or any(
        torch.is_tensor(t) and t.requires_grad for t in tensors))


def _refuse_dropout(module):
    """The differentiable paths have no dropout: refused before anything is launched."""
    if module.training and any(isinstance(m, nn.Dropout) and m.p > 0 for m in module.modules()):
        raise NotImplementedError(f"{type(module).__name__}: dropout (p > 0) has no differentiable path; the reference "
                                  "configurations all use p = 0")


def _lin(m, t, residual=None):
    """nn.Linear on the differentiable path (the kernel of _linear)."""
    return autograd.gemm_nt(t, m.weight, m.bias, residual)


def _conv(m, t, residual=None):
    """nn.Conv2d(kernel 1) on the differentiable path (the kernel of _conv1x1)."""
    return autograd.conv1x1(t, m.weight, m.bias, residual)


def _gn(m, t):
    return autograd.group_norm(t, m.weight, m.bias, m.num_groups, m.eps)


def Normalize(in_channels):
    return nn.GroupNorm(num_groups=32, num_channels=in_channels, eps=1e-6, affine=True)


class GEGLU(nn.Module):
    def __init__(self, dim_in, dim_out):
        super().__init__()
        self.proj = nn.Linear(dim_in, dim_out * 2)

    def forward(self, x):
        if _wants_grad(self, x):
            return autograd.geglu(_lin(self.proj, x))
        with torch.no_grad():
            return ops.geglu(_linear(self.proj, x))


class FeedForward(nn.Module):
    def __init__(self, dim, dim_out=None, mult=4, glu=False, dropout=0.0):
        super().__init__()
        inner = int(dim * mult)
        first = GEGLU(dim, inner) if glu else nn.Sequential(nn.Linear(dim, inner), nn.GELU())
        self.net = nn.Sequential(first, nn.Dropout(dropout), nn.Linear(inner, dim_out or dim))

    def forward(self, x, residual=None):
        first = self.net[0]
        if _wants_grad(self, x, residual):
            _refuse_dropout(self)
            h = first(x) if isinstance(first, GEGLU) else autograd.geglu(_lin(first[0], x), gelu_only=True)
            return _lin(self.net[2], h, residual)
        with torch.no_grad():
            h = first(x) if isinstance(first, GEGLU) else ops.geglu(_linear(first[0], x), gelu_only=True)
            return _linear(self.net[2], h, residual)


class SpatialSelfAttention(nn.Module):
    def __init__(self, in_channels):
        super().__init__()
        self.in_channels = in_channels
        self.norm = Normalize(in_channels)
        self.q = nn.Conv2d(in_channels, in_channels, 1)
        self.k = nn.Conv2d(in_channels, in_channels, 1)
        self.v = nn.Conv2d(in_channels, in_channels, 1)
        self.proj_out = nn.Conv2d(in_channels, in_channels, 1)

    def forward(self, x):
        if _wants_grad(self, x):
            return self.forward_train(x)
        with torch.no_grad():
            return self._forward_infer(x)

    def _forward_infer(self, x):
        b, c, h, w = x.shape
        x = x.contiguous()
        y = ops.group_norm(x, self.norm.weight.detach(), self.norm.bias.detach(), 32, self.norm.eps)
        tok = lambda t: t.reshape(b, c, h * w).transpose(1, 2).contiguous()         # [B, HW, C] token-major
        q, k, v = tok(_conv1x1(self.q, y)), tok(_conv1x1(self.k, y)), tok(_conv1x1(self.v, y))
        o = ops.attention(q, k, v, float(int(c) ** -0.5), heads=1)                  # [B, HW, C]
        o = o.transpose(1, 2).reshape(b, c, h, w).contiguous()
        return _conv1x1(self.proj_out, o, residual=x)

    def forward_train(self, x):
        """The same arithmetic as the inference path, with an autograd graph."""
        b, c, h, w = x.shape
        x = x.contiguous()
        y = _gn(self.norm, x)
        tok = lambda t: t.reshape(b, c, h * w).transpose(1, 2).contiguous()
        q, k, v = tok(_conv(self.q, y)), tok(_conv(self.k, y)), tok(_conv(self.v, y))
        o = autograd.attention(q, k, v, float(int(c) ** -0.5), heads=1)
        o = o.transpose(1, 2).reshape(b, c, h, w).contiguous()
        return _conv(self.proj_out, o, residual=x)


class CrossAttention(nn.Module):
    def __init__(self, query_dim, context_dim=None, heads=8, dim_head=64, dropout=0.0):
        super().__init__()
        inner = dim_head * heads
        context_dim = context_dim or query_dim
        self.scale, self.heads = dim_head ** -0.5, heads
        self.to_q = nn.Linear(query_dim, inner, bias=False)
        self.to_k = nn.Linear(context_dim, inner, bias=False)
        self.to_v = nn.Linear(context_dim, inner, bias=False)
        self.to_out = nn.Sequential(nn.Linear(inner, query_dim), nn.Dropout(dropout))

    def forward(self, x, context=None, mask=None, residual=None):
        """Under ``torch.no_grad()`` (or with nothing that requires grad) the inference path; with grad mode on and a
        parameter or an input that requires grad the differentiable path, as ``WavBEST.forward`` dispatches."""
        if _wants_grad(self, x, context, residual):
            return self.forward_train(x, context, mask, residual)
        with torch.no_grad():
            return self._forward_infer(x, context, mask, residual)

    def _forward_infer(self, x, context, mask, residual):
        ctx = x if context is None else context
        q, k, v = _linear(self.to_q, x), _linear(self.to_k, ctx), _linear(self.to_v, ctx)
        if mask is not None:
            mask = mask.reshape(mask.shape[0], -1)
        o = ops.attention(q, k, v, float(self.scale), heads=self.heads, key_mask=mask)
        return _linear(self.to_out[0], o, residual)

    def forward_train(self, x, context=None, mask=None, residual=None):
        """The same arithmetic as the inference path, with an autograd graph."""
        drop = self.to_out[1]
        if self.training and drop.p > 0:
            raise NotImplementedError("CrossAttention: dropout (p > 0) has no differentiable path; the reference "
                                      "configurations all use p = 0")
        ctx = x if context is None else context
        lin = lambda m, t, res=None: autograd.gemm_nt(t, m.weight, m.bias, res)
        q, k, v = lin(self.to_q, x), lin(self.to_k, ctx), lin(self.to_v, ctx)
        if mask is not None:
            mask = mask.reshape(mask.shape[0], -1)
        o = autograd.attention(q, k, v, float(self.scale), heads=self.heads, key_mask=mask)
        return lin(self.to_out[0], o, residual)


class BasicTransformerBlock(nn.Module):
    def __init__(self, dim, n_heads, d_head, dropout=0.0, context_dim=None, gated_ff=True, checkpoint=True,
                 disable_self_attn=False):
        super().__init__()
        self.disable_self_attn = disable_self_attn
        self.attn1 = CrossAttention(dim, context_dim if disable_self_attn else None, n_heads, d_head, dropout)
        self.ff = FeedForward(dim, dropout=dropout, glu=gated_ff)
        self.attn2 = CrossAttention(dim, context_dim, n_heads, d_head, dropout)
        self.norm1, self.norm2, self.norm3 = nn.LayerNorm(dim), nn.LayerNorm(dim), nn.LayerNorm(dim)

    def forward(self, x, context=None):
        if _wants_grad(self, x, context):
            _refuse_dropout(self)
            ln = lambda m, t: autograd.layer_norm(t, m.weight, m.bias, m.eps)
            return self._blocks(ln, x, context)
        with torch.no_grad():
            return self._blocks(lambda m, t: ops.layer_norm(t, m.weight.detach(), m.bias.detach(), m.eps), x, context)

    def _blocks(self, ln, x, context):
        """Both paths: the attention and feed-forward layers dispatch on grad mode themselves."""
        x = x.contiguous()
        x = self.attn1(ln(self.norm1, x), context=context if self.disable_self_attn else None, residual=x)
        x = self.attn2(ln(self.norm2, x), context=context, residual=x)
        return self.ff(ln(self.norm3, x), residual=x)


class SpatialTransformer(nn.Module):
    def __init__(self, in_channels, n_heads, d_head, depth=1, dropout=0.0, context_dim=None, disable_self_attn=False,
                 use_linear=False, use_checkpoint=True):
        super().__init__()
        if context_dim is not None and not isinstance(context_dim, list):
            context_dim = [context_dim]
        inner = n_heads * d_head
        self.in_channels, self.use_linear = in_channels, use_linear
        self.norm = Normalize(in_channels)
        self.proj_in = nn.Linear(in_channels, inner) if use_linear else nn.Conv2d(in_channels, inner, 1)
        self.transformer_blocks = nn.ModuleList(
            BasicTransformerBlock(inner, n_heads, d_head, dropout, context_dim[d], disable_self_attn=disable_self_attn)
            for d in range(depth))
        self.proj_out = nn.Linear(in_channels, inner) if use_linear else nn.Conv2d(inner, in_channels, 1)
        for p in self.proj_out.parameters():        # zero_module (:99-105)
            p.detach().zero_()

    def forward(self, x, context=None):
        ctx = context if isinstance(context, list) else [context]
        if _wants_grad(self, x, *ctx):
            return self.forward_train(x, ctx)
        with torch.no_grad():
            return self._forward_infer(x, ctx)

    def forward_train(self, x, ctx):
        """The same arithmetic as the inference path, with an autograd graph."""
        _refuse_dropout(self)
        b, c, h, w = x.shape
        x = x.contiguous()
        y = _gn(self.norm, x)
        if not self.use_linear:
            y = _conv(self.proj_in, y)
        y = y.reshape(b, y.shape[1], h * w).transpose(1, 2).contiguous()
        if self.use_linear:
            y = _lin(self.proj_in, y)
        for i, blk in enumerate(self.transformer_blocks):
            y = blk(y, context=ctx[i])
        if self.use_linear:
            y = _lin(self.proj_out, y)
        y = y.transpose(1, 2).reshape(b, -1, h, w).contiguous()
        if not self.use_linear:
            return _conv(self.proj_out, y, residual=x)
        return autograd.add(y, x)

    def _forward_infer(self, x, ctx):
        b, c, h, w = x.shape
        x = x.contiguous()
        y = ops.group_norm(x, self.norm.weight.detach(), self.norm.bias.detach(), 32, self.norm.eps)
        if not self.use_linear:
            y = _conv1x1(self.proj_in, y)
        y = y.reshape(b, y.shape[1], h * w).transpose(1, 2).contiguous()
        if self.use_linear:
            y = _linear(self.proj_in, y)
        for i, blk in enumerate(self.transformer_blocks):
            y = blk(y, context=ctx[i])
        if self.use_linear:
            y = _linear(self.proj_out, y)
        y = y.transpose(1, 2).reshape(b, -1, h, w).contiguous()
        if not self.use_linear:
            return _conv1x1(self.proj_out, y, residual=x)
        return ops.add(y, x)


class NIN(nn.Module):
    """y[b, :, h, w] = x[b, :, h, w] @ W + b (Hyper_unet_general.py:471-480); W is [in, out]."""

    def __init__(self, in_dim, num_units, init_scale=0.1):
        super().__init__()
        w = torch.empty(in_dim, num_units)
        # DDPM default_init (ref :417-454): fan-avg uniform variance scaling
        bound = (3.0 * max(init_scale, 1e-10) / ((in_dim + num_units) / 2.0)) ** 0.5
        self.W = nn.Parameter(w.uniform_(-bound, bound))
        self.b = nn.Parameter(torch.zeros(num_units))


class AttnBlockpp(nn.Module):
    """Hyper_unet_general.py:483-515 on the HIP kernels.  ``channels`` is the FOLDED channel count C*N (the block
    folds 'b c n h w -> b (c n) h w' before its GroupNorm); the softmax scale uses the unfolded C, as there."""

    def __init__(self, channels, skip_rescale=True, init_scale=0.0):
        super().__init__()
        self.GroupNorm_0 = nn.GroupNorm(num_groups=min(channels // 4, 32), num_channels=channels, eps=1e-6)
        self.NIN_0 = NIN(channels, channels)
        self.NIN_1 = NIN(channels, channels)
        self.NIN_2 = NIN(channels, channels)
        self.NIN_3 = NIN(channels, channels, init_scale=init_scale)
        self.skip_rescale = skip_rescale

    def forward(self, x):
        if _wants_grad(self, x):
            return self.forward_train(x)
        with torch.no_grad():
            return self._forward_infer(x)

    def forward_train(self, x):
        """The same arithmetic as the inference path, with an autograd graph (the NIN weights through gemm_nt on W.t())."""
        b, c, n, h, w = x.shape
        cf = c * n
        xf = x.contiguous().reshape(b, cf, h, w)
        t = _gn(self.GroupNorm_0, xf)
        tok = t.reshape(b, cf, h * w).transpose(1, 2).contiguous()
        nin = lambda m, a, res=None: autograd.gemm_nt(a, m.W.t(), m.b, res)
        q, k, v = nin(self.NIN_0, tok), nin(self.NIN_1, tok), nin(self.NIN_2, tok)
        o = autograd.attention(q, k, v, float(int(c) ** -0.5), heads=1)
        x_tok = xf.reshape(b, cf, h * w).transpose(1, 2).contiguous()
        y = nin(self.NIN_3, o, x_tok)
        if self.skip_rescale:
            y = autograd.scale(y, 2.0 ** -0.5)
        return y.transpose(1, 2).reshape(b, c, n, h, w).contiguous()

    def _forward_infer(self, x):
        b, c, n, h, w = x.shape
        cf = c * n
        xf = x.contiguous().reshape(b, cf, h, w)
        gn = self.GroupNorm_0
        t = ops.group_norm(xf, gn.weight.detach(), gn.bias.detach(), gn.num_groups, gn.eps)
        tok = t.reshape(b, cf, h * w).transpose(1, 2).contiguous()                        # [B, HW, CF] token-major
        nin = lambda m, a, res=None: ops.gemm_nt(a, m.W.detach().t().contiguous(), m.b.detach(), res)
        q, k, v = nin(self.NIN_0, tok), nin(self.NIN_1, tok), nin(self.NIN_2, tok)
        o = ops.attention(q, k, v, float(int(c) ** -0.5), heads=1)                        # [B, HW, CF]
        x_tok = xf.reshape(b, cf, h * w).transpose(1, 2).contiguous()
        y = nin(self.NIN_3, o, x_tok)                                                     # x + NIN_3(h), token-major
        if self.skip_rescale:
            y = ops.axpby([y], [2.0 ** -0.5])
        return y.transpose(1, 2).reshape(b, c, n, h, w).contiguous()
