"""The bf16 data gradient: ops.conv3d(math="bf16") of g on weights from ops.pack_conv_weight_bf16_dgrad
(tmdiff_conv3d_pack_weights_bf16_dgrad) against the fp64 transposed convolution.  The kernel is the inference mode's; the packing
is new, so a wrong tap mirror or channel swap is what these tests catch."""
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from oracle.make_golden import randn

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
CASES = [(32, 8, 1, 2, (5, 6, 12)), (32, 40, 1, 2, (5, 6, 12)), (96, 24, 3, 2, (4, 8, 8))]     # Cin -> Cout of the FORWARD convolution


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from tmdiff_amd import ops as _ops
    return _ops


def worst_ratio(err, bound):
    err, bound = err.double(), bound.double()
    assert bool((err[bound == 0] == 0).all()), "an error where every term is zero"
    live = bound > 0
    return float((err[live] / bound[live]).max()) if bool(live.any()) else 0.0


def rne(t):
    return t.float().to(torch.bfloat16).double()


def dgrad64(g, w, groups):
    """dL/dx' of y = conv3d(x', w, padding 1, groups) for dL/dy = g, in fp64"""
    return F.conv_transpose3d(g, w, padding=1, groups=groups)


@pytest.mark.parametrize("cin,cout,groups,b,shp", CASES, ids=[f"{c[0]}to{c[1]}g{c[2]}" for c in CASES])
def test_dgrad_bf16_vs_fp64(ops, cin, cout, groups, b, shp):
    """Exact model: g and w rounded to bf16 on the host, the transposed convolution in fp64; every output sums K = 27 * Cout/groups
    exact products in fp32: |err| <= K * 2^-24 * A (A: the same convolution of |g_r|, |w_r|) -- and inside the budget the bf16
    forward test applies (tests/test_gpu_bf16.py: relative L2 <= 1e-2, max error / max value <= 5e-2), here against the exact
    model.  Against the unrounded operands: + (2^-8 + 2^-16) * A_unrounded.  Measured: profiles/train_bf16_grad.txt."""
    w = randn(400, cout, cin // groups, 3, 3, 3) * (1.0 / math.sqrt(27 * cin // groups))
    g = randn(401, b, cout, *shp)
    wp = ops.pack_conv_weight_bf16_dgrad(w.cuda(), groups)
    got = ops.conv3d([g.cuda()], wp, cin, 3, groups=groups, math="bf16").cpu().double()
    K = 27 * cout // groups
    gr, wr = rne(g), rne(w)
    ref_r, A_r = dgrad64(gr, wr, groups), dgrad64(gr.abs(), wr.abs(), groups)
    ratio = worst_ratio((got - ref_r).abs(), K * U24 * A_r)
    m_r, l_r = rel_err(got, ref_r)
    g64, w64 = g.double(), w.double()
    ref, A = dgrad64(g64, w64, groups), dgrad64(g64.abs(), w64.abs(), groups)
    ratio_u = worst_ratio((got - ref).abs(), (2.0 ** -8 + 2.0 ** -16) * A + K * U24 * A_r)
    print(f"\ndgrad_bf16 {cin}->{cout} g{groups}: K={K}: worst |err| / bound exact model {ratio:.3e} (max-rel {m_r:.2e}, rel-L2 {l_r:.2e}), "
          f"unrounded {ratio_u:.3e}")
    assert ratio <= 1.0, f"exact model: {ratio:.3e} of the bound {K} * 2^-24 * A"
    assert l_r <= 1e-2 and m_r <= 5e-2
    assert ratio_u <= 1.0, f"unrounded: {ratio_u:.3e} of the bound"


@pytest.mark.parametrize("cin,cout,groups,b,shp", CASES, ids=[f"{c[0]}to{c[1]}g{c[2]}" for c in CASES])
def test_dgrad_packing_is_the_flipped_transpose(ops, cin, cout, groups, b, shp):
    """The packing, unpacked on the host, is exactly w.flip(2, 3, 4) with the channel axes swapped per group, rounded to bf16 --
    layout [g][Cout_g / 8][28 tap slots][Cin_g][8], slot 27 zero (include/tmdiff_hip.h)."""
    from tmdiff_amd import _lib
    w = randn(402, cout, cin // groups, 3, 3, 3)
    wp = ops.pack_conv_weight_bf16_dgrad(w.cuda(), groups)
    assert wp.dtype == torch.int16 and wp.numel() * 2 == _lib.lib.tmdiff_conv3d_packed_bf16_bytes(cin, cout, 3, groups)
    cin_g, cout_g = cin // groups, cout // groups
    u = wp.cpu().view(torch.bfloat16).view(groups, cout_g // 8, 28, cin_g, 8)
    assert bool((u[:, :, 27] == 0).all())
    # the data-gradient convolution's weight [Cin, Cout_g, taps]: w_d[g*cin_g + ci][co][tap] = w[g*cout_g + co][ci][26 - tap]
    wd = w.view(groups, cout_g, cin_g, 27).flip(3).transpose(1, 2)                 # [g][ci][co][tap]
    want = wd.to(torch.bfloat16).view(groups, cin_g, cout_g // 8, 8, 27).permute(0, 2, 4, 1, 3)     # [g][chunk][tap][ci][8]
    assert torch.equal(u[:, :, :27].contiguous().view(torch.int16), want.contiguous().view(torch.int16))
