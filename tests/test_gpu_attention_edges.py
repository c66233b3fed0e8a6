"""The attention operators (csrc/attention.hip) on the paths test_gpu_attention.py never reaches: several query blocks per
wave in the small-context kernel, masks that drop key 0 or every key, strided / misaligned calls through the C ABI, stressed
logits, and the small operators (gemm_nt, group_norm, layer_norm, geglu) at their edges.

The reference throughout is plain fp64 PyTorch on the CPU, softmax(q k^T * scale + fill) v per head, with the mask applied the
way the reference does it (core/Attention.py:203-204): masked_fill(-finfo(float32).max).  A sample whose keys are all masked
then has equal scores, i.e. the mean of v over its Nk keys -- not SDPA's NaN.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close, rel_err
from oracle.make_golden import randn

pytestmark = pytest.mark.gpu

FILL = -torch.finfo(torch.float32).max
EPS32 = float(torch.finfo(torch.float32).eps)

# Bound of the stressed cases: MARGIN x (error of a plain fp32 CPU evaluation of the same formula against fp64) + fp32 epsilon.
# Chosen from what the kernels do that the CPU fp32 path does not, before any kernel error was looked at:
#   * a dot product of length D (<= 128) is ONE sequential fp32 fma chain in the MFMA, where the CPU sums in 8 or 16 vector
#     lanes and then across them: in the random-walk model the chain's rounding error is up to sqrt(16) = 4 x larger, and a
#     logit's ABSOLUTE error is the softmax weight's RELATIVE error, so this factor goes straight into the output;
#   * __expf is exp2(x * log2(e)): the product's rounding adds |x| * 2^-24 of relative error; terms that still count against
#     fp32 epsilon have |x| <= 16.6, so at most ~1e-6, a few ulp where the CPU's expf is good to one;
#   * the running-max rescale rounds the accumulator once per 32-key tile (<= 7 tiles here).
# The norms at a large mean share the first effect (each thread's sequential partial sum of values near 1000 against the CPU's
# vectorised cascade sum).  4 x for the summation order, 2 x for the rest: 8.
MARGIN = 8.0


def cu(t):
    return t.cuda().contiguous()


def split(t, h):
    """[B, N, H*D] -> [B, H, N, D]"""
    return t.reshape(t.shape[0], t.shape[1], h, -1).permute(0, 2, 1, 3)


def merge(t):
    """[B, H, N, D] -> [B, N, H*D]"""
    return t.permute(0, 2, 1, 3).reshape(t.shape[0], t.shape[2], -1)


def attention_ref(q, k, v, scale, mask=None, dtype=torch.float64):
    """q [B, H, Nq, D], k / v [B, H, Nk, D], mask [B, Nk] bool (True = keep) -> [B, H, Nq, D] in `dtype`, one sample at a time."""
    out = torch.empty(q.shape, dtype=dtype)
    for b in range(q.shape[0]):
        sim = torch.matmul(q[b].to(dtype), k[b].to(dtype).transpose(-1, -2)) * scale
        if mask is not None:
            sim = sim.masked_fill(~mask[b][None, None, :], FILL)
        out[b] = torch.matmul(sim.softmax(dim=-1), v[b].to(dtype))
    return out


def run_ops(q, k, v, h, mask=None):
    """ops.attention on contiguous [B, N, H*D] inputs -> [B, H, Nq, D] on the CPU"""
    from tmdiff_amd import ops
    d = q.shape[-1] // h
    return split(ops.attention(cu(q), cu(k), cu(v), d ** -0.5, heads=h, key_mask=mask).cpu(), h)


# ---- A1: several query blocks per wave in the small-context kernel ----------------------------------------------------------
# (B, H, Nq, Nk, queries per workgroup the launcher must pick)
MULTI_BLOCK = [
    (16, 8, 2048, 77, 256),    # 2 blocks per wave, 80 key rows in LDS
    (32, 8, 2100, 77, 512),    # 4 blocks; the last workgroup has 52 queries: wave 0 full, wave 1 ragged, waves 2-3 idle
    (64, 8, 1025, 77, 1024),   # 8 blocks; the second workgroup has one query
    (32, 8, 2100, 96, 512),    # 96 key rows, three key tiles
    (32, 8, 2100, 81, 512),    # 96 key rows, ragged third tile
]


def ctx_qpw(b, h, nq, nk, d=64):
    from tmdiff_amd import _lib
    return _lib.lib.tmdiff_attn_ctx_queries_per_workgroup(b, h, nq, nk, d)


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("b,h,nq,nk,qpw", MULTI_BLOCK)
def test_ctx_kernel_several_blocks_per_wave(b, h, nq, nk, qpw, masked):
    """Each wave of attn_ctx_kernel walks qpw / 128 query blocks: the prefetch of the next block under the MFMAs, the re-use of
    the wave's staging tile and the trailing wave barrier all run.  The shapes only reach that code while the launcher's
    heuristic picks these qpw values, so that is asserted first: retune the heuristic and this fails until new shapes are chosen."""
    d = 64
    assert ctx_qpw(b, h, nq, nk) == qpw, "the launcher's queries-per-workgroup choice changed: pick shapes that reach it again"
    q, k, v = randn(21, b, nq, h * d), randn(22, b, nk, h * d), randn(23, b, nk, h * d)
    mask = None
    if masked:
        mask = torch.rand(b, nk, generator=torch.Generator().manual_seed(2)) > 0.3
        assert bool(mask.any(dim=1).all())
    got = run_ops(q, k, v, h, mask)
    want = attention_ref(split(q, h), split(k, h), split(v, h), d ** -0.5, mask)
    assert bool(torch.isfinite(got).all())
    assert_close(got, want, 1e-5, 1e-5, f"attention, {qpw // 128} query blocks per wave")
    if qpw == 1024:
        # one (batch, head) of the same data run alone is one block per wave; lane for lane the same operations on the same
        # operands in the same order, so the same bits
        bi, hi = 37, 5
        sl = lambda t: t[bi:bi + 1, :, hi * d:(hi + 1) * d].contiguous()
        assert ctx_qpw(1, 1, nq, nk) == 128
        alone = run_ops(sl(q), sl(k), sl(v), 1, None if mask is None else mask[bi:bi + 1])
        assert torch.equal(alone[0, 0], got[bi, hi]), \
            f"8 blocks per wave vs 1: {int((alone[0, 0] != got[bi, hi]).sum())} of {alone.numel()} elements differ"


# ---- A2: masks that drop every key, the whole first key tile(s), all but the last key ---------------------------------------
@pytest.mark.parametrize("h,nq,nk,d,lead", [
    (2, 150, 77, 16, 32),     # generic kernel
    (2, 150, 200, 32, 32),    # generic kernel, 7 key tiles
    (2, 150, 200, 64, 32),    # DMA kernel
    (2, 150, 200, 64, 64),    # DMA kernel, the first two key tiles masked
    (2, 150, 77, 128, 32),    # DMA kernel, d_head 128
    (2, 150, 77, 64, 32),     # small-context kernel
], ids=["generic-d16", "generic-d32", "dma-d64", "dma-d64-lead64", "dma-d128", "ctx-d64"])
def test_masks_without_key_zero(h, nq, nk, d, lead):
    """Sample 0: every key masked (the mean of v over exactly Nk keys); sample 1: the first `lead` keys masked; sample 2: only
    the last key kept.  Nk is no multiple of 32, so the last key tile has padding slots that must stay out of the mean."""
    assert nk % 32 != 0
    q, k, v = randn(31, 3, nq, h * d), randn(32, 3, nk, h * d), randn(33, 3, nk, h * d)
    mask = torch.zeros(3, nk, dtype=torch.bool)
    mask[1, lead:] = True
    mask[2, -1] = True
    got = run_ops(q, k, v, h, mask)
    assert bool(torch.isfinite(got).all()), \
        f"non-finite output: {int((~torch.isfinite(got)).sum())} elements, samples {(~torch.isfinite(got)).flatten(1).any(1).tolist()}"
    want = attention_ref(split(q, h), split(k, h), split(v, h), d ** -0.5, mask)
    mean_v = split(v, h)[0].double().mean(dim=1, keepdim=True).expand(h, nq, d)
    assert_close(want[0], mean_v, 1e-12, 1e-12, "the reference on a fully masked sample is the mean of v")
    assert_close(got[0], mean_v, 1e-5, 1e-5, "fully masked sample vs the mean of v over Nk keys")
    assert_close(got[2], split(v, h)[2][:, -1:, :].expand(h, nq, d), 1e-5, 1e-5, "only the last key kept")
    for i, what in enumerate(("fully masked", f"first {lead} keys masked", "only the last key kept")):
        assert_close(got[i], want[i], 1e-5, 1e-5, what)


# ---- A3: strides and alignment through the C ABI --------------------------------------------------------------------------------
SENTINEL = -777.25
TAIL = 128      # floats behind every buffer: a store past the last row's D columns lands on sentinels, not outside the buffer


class Layout:
    """Where a [B, H, N, D] tensor lies in a flat buffer: (batch, head, row) strides, offset and buffer size, in elements."""

    def __init__(self, name, fn):
        self.name, self.fn = name, fn

    def view(self, flat_factory, b, h, n, d):
        bs, hs, rs, off, total = self.fn(b, h, n, d)
        flat = flat_factory(total + TAIL)
        return flat, flat.as_strided((b, h, n, d), (bs, hs, rs, 1), off)


def fused(slot):           # one of the three slices of a fused [B, N, 3*H*D] projection
    return Layout(f"fused{slot}", lambda b, h, n, d: (n * 3 * h * d, d, 3 * h * d, slot * h * d, b * n * 3 * h * d))


def padded_rows(pad):      # [B, N, H*D + pad]
    return Layout(f"rowpad{pad}", lambda b, h, n, d: (n * (h * d + pad), d, h * d + pad, 0, b * n * (h * d + pad)))


def shifted(off):          # contiguous [B, N, H*D], `off` floats into the buffer
    return Layout(f"shift{off}", lambda b, h, n, d: (n * h * d, d, h * d, off, b * n * h * d + off))


BND = shifted(0)
HEAD_MAJOR = Layout("headmajor", lambda b, h, n, d: (h * n * d, n * d, d, 4, b * h * n * d + 4))   # [B, H, N, D] behind 4 guard floats

STRIDED = [
    # (H, Nq, Nk, D, q layout, k / v layout, out layout)
    (4, 150, 150, 32, fused(0), fused(1), fused(2)),             # generic kernel
    (4, 150, 150, 64, fused(0), fused(1), fused(2)),             # DMA kernel
    (2, 150, 150, 128, fused(0), fused(2), fused(1)),            # DMA kernel, d_head 128
    (4, 300, 77, 64, fused(0), fused(1), fused(1)),              # small-context kernel: aligned 16-byte row pieces, stays there
    (4, 150, 100, 32, HEAD_MAJOR, HEAD_MAJOR, HEAD_MAJOR),
    (4, 150, 200, 64, HEAD_MAJOR, HEAD_MAJOR, HEAD_MAJOR),
    (2, 130, 77, 128, HEAD_MAJOR, HEAD_MAJOR, HEAD_MAJOR),
    (4, 300, 77, 64, HEAD_MAJOR, HEAD_MAJOR, HEAD_MAJOR),
    # d_head 64 with at most 96 keys, but rows the float4 kernel cannot address: must leave it and still be right
    (4, 300, 77, 64, padded_rows(1), BND, BND),                  # odd query row stride
    (4, 300, 77, 64, BND, BND, padded_rows(1)),                  # odd output row stride
    (4, 300, 77, 64, padded_rows(1), padded_rows(3), padded_rows(1)),
    (4, 300, 77, 64, padded_rows(2), BND, padded_rows(2)),       # 8-byte aligned rows only
    (4, 300, 77, 64, shifted(1), BND, BND),                      # q one float off a 16-byte boundary
    (4, 300, 77, 64, BND, BND, shifted(1)),                      # out one float off
    (4, 300, 96, 64, shifted(3), shifted(2), shifted(1)),
    # head dims that are no multiple of 32: the padded columns of the tiles must not reach memory
    (3, 150, 100, 48, BND, BND, padded_rows(3)),
    (3, 150, 77, 80, padded_rows(1), fused(1), padded_rows(5)),
    (2, 70, 45, 2, BND, BND, padded_rows(1)),
    (1, 33, 200, 126, BND, padded_rows(1), padded_rows(2)),
]


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("h,nq,nk,d,ql,kl,ol", STRIDED,
                         ids=[f"d{c[3]}-nk{c[2]}-{c[4].name}-{c[5].name}-{c[6].name}" for c in STRIDED])
def test_strided_and_misaligned_calls(h, nq, nk, d, ql, kl, ol, masked):
    """tmdiff_attn_fwd addresses q / k / v / out as base + b * strides[0] + head * strides[1] + row * strides[2] + d.  The
    inputs lie in buffers whose other elements are NaN (a read outside the [N, D] rows of a head poisons the result), the
    output in a buffer of sentinels, every one of which must survive outside the [Nq, D] rows of each head."""
    from tmdiff_amd import _lib, ops
    b = 2
    nan_buf = lambda n: torch.full((n,), float("nan"), device="cuda")
    data = {}
    for name, seed, lay, n in (("q", 41, ql, nq), ("k", 42, kl, nk), ("v", 43, kl, nk)):
        x = randn(seed, b, h, n, d)
        flat, view = lay.view(nan_buf, b, h, n, d)
        view.copy_(x.cuda())
        data[name] = (x, flat, view)
    out_flat, out = ol.view(lambda n: torch.full((n,), SENTINEL, device="cuda"), b, h, nq, d)
    gap_flat, gap = ol.view(lambda n: torch.ones(n, dtype=torch.bool, device="cuda"), b, h, nq, d)
    gap.fill_(False)
    assert int((~gap_flat).sum()) == b * h * nq * d, "the output view overlaps itself"
    mask = m = None
    if masked:
        mask = torch.rand(b, nk, generator=torch.Generator().manual_seed(3)) > 0.3
        mask[0, :33] = False                       # (the first key tile of sample 0 entirely masked)
        m = mask.to(device="cuda", dtype=torch.uint8).contiguous()
    st = lambda t: (C.c_int64 * 3)(*t.stride()[:3])
    qv, kv, vv = data["q"][2], data["k"][2], data["v"][2]
    _lib.check(_lib.lib.tmdiff_attn_fwd(qv.data_ptr(), kv.data_ptr(), vv.data_ptr(), out.data_ptr(),
                                        m.data_ptr() if m is not None else None, b, h, nq, nk, d, st(qv), st(kv), st(vv),
                                        st(out), d ** -0.5, ops.stream_ptr()), "attn_fwd")
    torch.cuda.synchronize()
    assert torch.equal(out_flat[gap_flat], torch.full_like(out_flat[gap_flat], SENTINEL)), \
        f"{int((out_flat[gap_flat] != SENTINEL).sum())} elements outside the output rows were written"
    got = out.cpu()
    assert bool(torch.isfinite(got).all()), "non-finite output: something outside the input rows was read"
    want = attention_ref(data["q"][0], data["k"][0], data["v"][0], d ** -0.5, mask)
    assert_close(got, want, 1e-5, 1e-5, "strided attention")
    for name in ("q", "k", "v"):                   # and the inputs are untouched
        assert torch.equal(data[name][2].cpu(), data[name][0]), name


# ---- A4: stressed logits --------------------------------------------------------------------------------------------------------
def stressed_inputs(kind, b, h, nq, nk, d):
    """[B, H, N, D] inputs whose scores q k^T * d^-0.5 leave the O(1) range of the other tests."""
    q, k, v = randn(51, b, h, nq, d), randn(52, b, h, nk, d), randn(53, b, h, nk, d)
    if kind == "peaked":          # score standard deviation 30: a near one-hot softmax
        q = q * 30.0
    elif kind == "offset":        # every score of a query near +500 or near -500: q_0 = +-20, k_0 = 25 sqrt(d) + N(0,1)
        sign = torch.where(randn(54, b, h, nq) >= 0, 1.0, -1.0)
        q[..., 0] = 20.0 * sign
        k[..., 0] += 25.0 * d ** 0.5
    elif kind == "mixed":         # per-query magnitudes from 1e-3 to 1e2
        q = q * 10.0 ** (5.0 * torch.rand(b, h, nq, 1, generator=torch.Generator().manual_seed(55)) - 3.0)
    else:
        raise ValueError(kind)
    return q.contiguous(), k.contiguous(), v


def stress_yardstick(kind, b, h, nq, nk, d):
    """(inputs, fp64 reference, (max-rel, rel-L2) of the plain fp32 CPU evaluation against it)"""
    q, k, v = stressed_inputs(kind, b, h, nq, nk, d)
    want = attention_ref(q, k, v, d ** -0.5)
    yard = rel_err(attention_ref(q, k, v, d ** -0.5, dtype=torch.float32), want)
    return (q, k, v), want, yard


STRESS_SHAPES = [(2, 3, 150, 100, 32), (2, 2, 150, 77, 80), (2, 2, 150, 200, 64), (2, 2, 130, 150, 128), (2, 2, 300, 77, 64)]
STRESS_IDS = ["generic-d32", "generic-d80", "dma-d64", "dma-d128", "ctx-d64"]


@pytest.mark.parametrize("kind", ["peaked", "offset", "mixed"])
@pytest.mark.parametrize("b,h,nq,nk,d", STRESS_SHAPES, ids=STRESS_IDS)
def test_stressed_logits(b, h, nq, nk, d, kind):
    """Large, offset and mixed-magnitude logits: the max-subtraction and __expf at arguments far from 0.  The bound is MARGIN x
    the error of the plain fp32 evaluation of the same formula on the CPU, measured here, plus fp32 epsilon."""
    (q, k, v), want, yard = stress_yardstick(kind, b, h, nq, nk, d)
    assert bool(torch.isfinite(want).all()) and float(want.abs().amax(dim=-1).min()) > 0, "degenerate reference"
    assert all(0 < y < float("inf") for y in yard), f"degenerate fp32 yardstick {yard}"
    got = run_ops(merge(q), merge(k), merge(v), h)
    assert bool(torch.isfinite(got).all())
    err = rel_err(got, want)
    print(f"\nstressed logits {kind:7s} D={d:3d} Nk={nk:3d}: fp32 yardstick max-rel {yard[0]:.3e} rel-L2 {yard[1]:.3e}; "
          f"kernel max-rel {err[0]:.3e} rel-L2 {err[1]:.3e}; ratio {err[0] / yard[0]:.2f} / {err[1] / yard[1]:.2f}")
    assert_close(got, want, MARGIN * yard[0] + EPS32, MARGIN * yard[1] + EPS32, f"attention, {kind} logits")


# ---- A5: the small operators at their edges ---------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("res", [False, True], ids=["nores", "res"])
def test_gemm_nt_edges(bias, res):
    """Every bias / residual combination at tile edges of M, N (64 x 64 tiles) and K (32-wide steps)."""
    from tmdiff_amd import ops
    for m in (0, 1, 63, 64, 65):
        for n in (1, 63, 64, 65, 129):
            for k in (1, 2, 31, 32, 33, 1280):
                a, w = randn(61, m, k), randn(62, n, k) / k ** 0.5
                bv = randn(63, n) if bias else None
                r = randn(64, m, n) if res else None
                got = ops.gemm_nt(cu(a), cu(w), None if bv is None else cu(bv), None if r is None else cu(r)).cpu()
                assert got.shape == (m, n)
                if m == 0:
                    continue
                want = F.linear(a.double(), w.double(), None if bv is None else bv.double())
                want = want if r is None else want + r.double()
                if m * n == 1:
                    # one output element: max|want| is that element, which can be small by cancellation.  The forward error
                    # of a dot product is relative to sum |a_k w_k| (+ |bias| + |residual|): the same 1e-5 against that
                    size = float((a.double().abs() * w.double().abs()).sum()) + (abs(float(bv)) if bias else 0) + \
                        (abs(float(r)) if res else 0)
                    assert abs(float(got) - float(want)) <= 1e-5 * size, (m, n, k)
                else:
                    assert_close(got, want, 1e-5, 1e-5, f"gemm_nt M={m} N={n} K={k}")
    # leading dims are folded into M
    a, w, bv = randn(65, 2, 3, 5, 33), randn(66, 70, 33) / 33 ** 0.5, randn(67, 70)
    r = randn(68, 2, 3, 5, 70)
    got = ops.gemm_nt(cu(a), cu(w), cu(bv) if bias else None, cu(r) if res else None).cpu()
    want = F.linear(a.double(), w.double(), bv.double() if bias else None) + (r.double() if res else 0)
    assert got.shape == (2, 3, 5, 70)
    assert_close(got, want, 1e-5, 1e-5, "gemm_nt [2, 3, 5, K]")


def gn_ref(x, groups, g, be, dtype=torch.float64):
    return F.group_norm(x.to(dtype), groups, g.to(dtype), be.to(dtype), 1e-6)


@pytest.mark.parametrize("groups", [1, 8, 32])
@pytest.mark.parametrize("cpg", [1, 2, 5])
def test_group_norm_edges(groups, cpg):
    from tmdiff_amd import ops
    c = groups * cpg
    g, be = 1 + 0.1 * randn(71, c), 0.1 * randn(72, c)
    for p in (1, 7, 256, 4099):
        x = randn(73, 2, c, p)
        assert_close(ops.group_norm(cu(x), cu(g), cu(be), groups, 1e-6).cpu(), gn_ref(x, groups, g, be), 2e-5, 2e-5,
                     f"group_norm C={c} groups={groups} P={p}")
    # 5-D, as AttnBlockpp passes it ([B, C, N, H, W]), and inputs whose variance is of the order of eps
    x = randn(74, 2, c, 3, 5, 7)
    assert_close(ops.group_norm(cu(x), cu(g), cu(be), groups, 1e-6).cpu(), gn_ref(x, groups, g, be), 2e-5, 2e-5, "5-D")
    x = 1e-3 * randn(75, 2, c, 3, 5, 7)
    assert_close(ops.group_norm(cu(x), cu(g), cu(be), groups, 1e-6).cpu(), gn_ref(x, groups, g, be), 2e-5, 2e-5, "x ~ 1e-3")


def test_group_norm_large_mean():
    """x = 1000 + N(0,1): the deviations are 1e-3 of the values summed.  Bound: the A4 yardstick (the fp32 CPU operator against
    fp64) x MARGIN + fp32 epsilon, over many (sample, group) rows so that the yardstick is no single mean's luck."""
    from tmdiff_amd import ops
    for c, groups, shape in ((64, 32, (16, 16)), (40, 8, (4099,)), (32, 1, (3, 5, 7))):
        g, be = 1 + 0.1 * randn(76, c), 0.1 * randn(77, c)
        x = 1000.0 + randn(78, 8, c, *shape)
        want = gn_ref(x, groups, g, be)
        yard = rel_err(gn_ref(x, groups, g, be, torch.float32), want)
        assert all(0 < y < float("inf") for y in yard), yard
        got = ops.group_norm(cu(x), cu(g), cu(be), groups, 1e-6).cpu()
        err = rel_err(got, want)
        print(f"\ngroup_norm x=1000+randn C={c} groups={groups} P={x[0, 0].numel()}: fp32 yardstick max-rel {yard[0]:.3e} "
              f"rel-L2 {yard[1]:.3e}; kernel max-rel {err[0]:.3e} rel-L2 {err[1]:.3e}")
        assert_close(got, want, MARGIN * yard[0] + EPS32, MARGIN * yard[1] + EPS32, f"group_norm, mean 1000, C={c}")


def ln_ref(x, g, be, dtype=torch.float64):
    return F.layer_norm(x.to(dtype), x.shape[-1:], g.to(dtype), be.to(dtype))


@pytest.mark.parametrize("d", [1, 7, 63, 64, 65, 100, 768, 1280])
def test_layer_norm_edges(d):
    """One wave per row, four rows per workgroup: row counts around 4, D around the wave width."""
    from tmdiff_amd import ops
    g, be = 1 + 0.1 * randn(81, d), 0.1 * randn(82, d)
    for rows in (0, 1, 3, 4, 5, 1001):
        x = randn(83, rows, d)
        got = ops.layer_norm(cu(x), cu(g), cu(be)).cpu()
        assert got.shape == (rows, d)
        if rows:
            assert_close(got, ln_ref(x, g, be), 2e-5, 2e-5, f"layer_norm rows={rows} D={d}")


def test_layer_norm_large_mean():
    from tmdiff_amd import ops
    for d in (64, 100, 768, 1280):
        g, be = 1 + 0.1 * randn(84, d), 0.1 * randn(85, d)
        x = 1000.0 + randn(86, 1001, d)
        want = ln_ref(x, g, be)
        yard = rel_err(ln_ref(x, g, be, torch.float32), want)
        assert all(0 < y < float("inf") for y in yard), yard
        got = ops.layer_norm(cu(x), cu(g), cu(be)).cpu()
        err = rel_err(got, want)
        print(f"\nlayer_norm x=1000+randn D={d}: fp32 yardstick max-rel {yard[0]:.3e} rel-L2 {yard[1]:.3e}; "
              f"kernel max-rel {err[0]:.3e} rel-L2 {err[1]:.3e}")
        assert_close(got, want, MARGIN * yard[0] + EPS32, MARGIN * yard[1] + EPS32, f"layer_norm, mean 1000, D={d}")


@pytest.mark.parametrize("inner", [1, 7, 33, 321])
def test_geglu_edges(inner):
    """Odd inner widths, row counts 0 / 1 / 257 (the grid is ceil(rows * inner / 256)), both modes, and gates of +-30 where erf
    has long saturated: gelu(30) = 30, gelu(-30) = -0."""
    from tmdiff_amd import ops
    for rows in (0, 1, 257):
        u = randn(91, rows, 2 * inner)
        sat = u.clone()
        sat[:, ::3] = 30.0
        sat[:, 1::3] = -30.0
        for x in (u, sat):
            got = ops.geglu(cu(x)).cpu()
            got1 = ops.geglu(cu(x), gelu_only=True).cpu()
            assert got.shape == (rows, inner) and got1.shape == (rows, 2 * inner)
            if rows:
                a, gate = x.double().chunk(2, -1)
                assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(got1).all())
                assert_close(got, a * F.gelu(gate), 1e-6, 1e-6, f"geglu rows={rows} inner={inner}")
                assert_close(got1, F.gelu(x.double()), 1e-6, 1e-6, f"gelu rows={rows} inner={inner}")


def test_argument_checks():
    """What the operators do not support is an error, never a launch."""
    from tmdiff_amd import ops
    from tmdiff_amd._lib import TmdiffError
    z = lambda *s: torch.zeros(*s, device="cuda")
    with pytest.raises(TmdiffError, match="head dim"):
        ops.attention(z(1, 8, 33), z(1, 8, 33), z(1, 8, 33), 1.0, heads=1)          # odd D
    with pytest.raises(TmdiffError, match="head dim"):
        ops.attention(z(1, 8, 130), z(1, 8, 130), z(1, 8, 130), 1.0, heads=1)       # D > 128
    with pytest.raises(TmdiffError, match="extents"):
        ops.attention(z(1, 1, 131072), z(1, 1, 131072), z(1, 1, 131072), 1.0, heads=65536)   # B * H > 65535
    with pytest.raises(TmdiffError, match="group_norm"):
        ops.group_norm(z(2, 10, 8), z(10), z(10), 4)                                # C % groups != 0
    with pytest.raises(TmdiffError, match="gemm_nt"):
        ops.gemm_nt(z(4, 0), z(8, 0))                                               # K = 0
    assert ctx_qpw(1, 1, 8, 8, 33) == 0 and ctx_qpw(1, 65536, 8, 8, 64) == 0
