"""A-trous wavelet pansharpening on the GPU (csrc/atrous.hip, ``ops.atrous_lowpass`` / ``awlp_inject`` / ``awlp``,
``tiling.awlp_fuse``, the "atwt" and "awlp" baselines of ``evaluate.val_dataset``).

The low-pass and the injection are held elementwise to their definitions on the same float32 inputs: one float32 ulp of the
expected value plus 2^-40 -- half an ulp for the single rounding, half for a tie that the fp64 operation order may flip, the
absolute term for cancellation in fp64 (the helper of tests/test_gpu_tv.py, restated).  On 8-bit integer images at two levels
and on binary images at three every level is exact in float32 (tests/test_atrous_host.py checks that claim), and the device
must give the float64 definition's bits.  The fused launch must equal the chain of single-level launches bit for bit at every
shape.  The whole chain's cases and its tolerance come from tests/test_atrous_host.py (``awlp_tol_u``: 4 times the distance of
the float32-storage restatement from the float64 run, rounded up: 5 / 5 / 7 u).  Measured on the MI355X: DESIGN.md section 5."""
import functools

import numpy as np
import pytest
import torch

from test_atrous_host import AWLP_CASES, awlp_error_u, awlp_scene, awlp_tol_u

pytestmark = pytest.mark.gpu

T_H, T_W = 32, 32                                                                     # the tile of csrc/atrous.hip
# the last: smaller than the 14-pixel halo of three levels in both axes
LOWPASS_SHAPES = [(1, 1, 1, 1), (1, 1, 3, 5), (2, 3, T_H, T_W), (1, 2, T_H + 1, T_W + 1), (1, 1, T_H - 1, 2 * T_W + 3), (2, 1, 1, 70),
                  (1, 2, 70, 1), (1, 2, 9, 11)]
INJECT_BANDS = (1, 4, 8, 14)


@pytest.fixture(autouse=True)
def _inference_mode():
    with torch.no_grad():
        yield


def cu(a):
    return torch.from_numpy(np.array(a)).cuda()


def _within_an_ulp(got, want, what):
    got, want = got.cpu().numpy().astype(np.float64), want.astype(np.float64)
    bound = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) + 2.0 ** -40
    worst = float((np.abs(got - want) / bound).max())
    assert np.isfinite(got).all() and worst <= 1.0, (what, worst)
    return worst


@functools.lru_cache(maxsize=None)
def lowpass_input(shape):
    x = np.random.default_rng(shape[2] * 1000 + shape[3]).random(shape).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def lowpass_wanted(shape, levels):
    """metrics.atrous_lowpass(storage=np.float32) of the shape's input, computed once and shared (read-only)."""
    from tmdiff_amd import metrics
    want = metrics.atrous_lowpass(lowpass_input(shape), levels, storage=np.float32)
    want.setflags(write=False)
    return want


# ---- atrous_lowpass ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", LOWPASS_SHAPES)
def test_lowpass_against_the_definition(shape):
    from tmdiff_amd import ops
    dx = cu(lowpass_input(shape))
    for levels in (1, 2, 3):
        got = ops.atrous_lowpass(dx, levels)
        worst = _within_an_ulp(got, lowpass_wanted(shape, levels), (shape, levels))
        print(f"atrous_lowpass {shape} levels={levels}: at most {worst:.3f} of the bound")
        # the fused launch is the chain of single-level launches, bit for bit
        chain = dx
        for first in range(1, levels + 1):
            chain = ops.atrous_lowpass(chain, 1, first=first)
        assert torch.equal(got, chain), (shape, levels)
        if levels == 3:
            assert torch.equal(ops.atrous_lowpass(ops.atrous_lowpass(dx, 1), 2, first=2), got)
        # a batch equals its samples; a second call gives the same bits
        assert torch.equal(ops.atrous_lowpass(dx, levels), got)
        assert torch.equal(ops.atrous_lowpass(dx[shape[0] - 1:].contiguous(), levels), got[shape[0] - 1:])
        assert torch.equal(ops.atrous_lowpass(dx[:, shape[1] - 1].contiguous(), levels), got[:, shape[1] - 1])      # [B, H, W]


@pytest.mark.parametrize("shape", [(2, 2, T_H + 5, 2 * T_W + 3), (1, 1, 9, 11)])
def test_lowpass_is_exact_on_integer_images(shape):
    from tmdiff_amd import metrics, ops
    rng = np.random.default_rng(shape[2])
    x8 = rng.integers(0, 256, shape).astype(np.float32)
    x1 = rng.integers(0, 2, shape).astype(np.float32)
    for x, levels in ((x8, 1), (x8, 2), (x1, 3)):
        want = metrics.atrous_lowpass(x, levels)
        assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
        assert torch.equal(ops.atrous_lowpass(cu(x), levels), cu(want.astype(np.float32))), (shape, levels)
    flat = torch.full(shape, 0.37, device="cuda")
    assert torch.equal(ops.atrous_lowpass(flat, 3), flat)                             # a float32 constant is reproduced exactly


def test_lowpass_graph_replay_out_and_refusals():
    from tmdiff_amd import ops
    shape = (1, 2, T_H + 1, T_W + 1)
    x = cu(lowpass_input(shape))
    eager = ops.atrous_lowpass(x, 3)
    src, out = torch.zeros_like(x), torch.empty_like(x)
    assert ops.atrous_lowpass(src, 3, out=out) is out
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    ops.atrous_lowpass(src, 3, out=out)
    assert torch.cuda.memory_allocated() == before
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.atrous_lowpass(src, 3, out=out)
    src.copy_(x)
    for _ in range(2):
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
    flat = torch.zeros(2 * x.numel() - 4, device="cuda")
    for call in (lambda: ops.atrous_lowpass(x, 3, out=x),
                 lambda: ops.atrous_lowpass(flat[:x.numel()].view(shape), 2, out=flat[x.numel() - 4:].view(shape)),   # 4 floats shared
                 lambda: ops.atrous_lowpass(x, 0),
                 lambda: ops.atrous_lowpass(x, 4),
                 lambda: ops.atrous_lowpass(x, 2, first=3),
                 lambda: ops.atrous_lowpass(x, 2, out=torch.empty(1, 2, T_H + 1, T_W, device="cuda")),
                 lambda: ops.atrous_lowpass(x.double(), 2),
                 lambda: ops.atrous_lowpass(x.cpu(), 2),
                 lambda: ops.atrous_lowpass(x[..., ::2], 2),
                 lambda: ops.atrous_lowpass(x[0, 0], 2),
                 lambda: ops.atrous_lowpass(torch.empty(1, 1, 0, 4, device="cuda"), 2)):
        with pytest.raises(ValueError):
            call()
    assert ops.atrous_supported(1, 1, 1, 1, 3) and not ops.atrous_supported(1, 1, 4, 4, 4) and not ops.atrous_supported(1, 1, 4, 4, 2, 3)


# ---- awlp_inject ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inject_inputs(c):
    """Float32 (ms_exp, pan, pan_lp) for C bands: 2 images of 19 x 23 (H W % 4 != 0: the scalar path) at C = 1, of 20 x 24 (the
    16-byte path) otherwise; pan_lp is the definition's low-pass PAN rounded to float32."""
    from tmdiff_amd import metrics
    h, w = (19, 23) if c == 1 else (20, 24)
    rng = np.random.default_rng(c)
    ms = (0.1 + 0.8 * rng.random((2, c, h, w))).astype(np.float32)
    pan = (ms.mean(axis=1, keepdims=True) + 0.1 * rng.random((2, 1, h, w))).astype(np.float32)
    low = metrics.atrous_lowpass(pan, 2, storage=np.float32)
    for a in (ms, pan, low):
        a.setflags(write=False)
    return ms, pan, low


@pytest.mark.parametrize("c", INJECT_BANDS)
def test_inject_against_the_definition(c):
    from tmdiff_amd import metrics, ops
    ms, pan, low = inject_inputs(c)
    dms, dpan, dlow = cu(ms), cu(pan), cu(low)
    mo = ops.plane_moments(dms, dlow)
    for mode in metrics.ATROUS_MODES:
        want = metrics.awlp_inject(ms, pan, low, mo.cpu().numpy(), mode)                 # the device's own moments
        got = ops.awlp_inject(dms, dpan, dlow, mo, mode)
        worst = _within_an_ulp(got, want, (c, mode))
        print(f"awlp_inject C={c} {mode}: at most {worst:.3f} of the bound")
        work = dms.clone()
        assert ops.awlp_inject(work, dpan, dlow, mo, mode, out=work) is work and torch.equal(work, got)     # in place
        assert torch.equal(ops.awlp_inject(dms[1:].contiguous(), dpan[1:].contiguous(), dlow[1:].contiguous(), mo[1:].contiguous(),
                                           mode), got[1:])                                # a batch equals its samples
    if c == 1:
        assert torch.equal(ops.awlp_inject(dms, dpan, dlow, mo, "awlp"), ops.awlp_inject(dms, dpan, dlow, mo, "atwt"))   # M / I == 1


def test_inject_edge_values_and_refusals():
    from tmdiff_amd import metrics, ops
    ms, pan, low = inject_inputs(4)
    ms = ms.copy()
    ms[0, :, 3, 5] = (0.25, -0.25, 0.5, -0.5)                                          # I == 0: the pixel is returned unchanged
    dms, dpan, dlow = cu(ms), cu(pan), cu(low)
    mo = ops.plane_moments(dms, dlow)
    got = ops.awlp_inject(dms, dpan, dlow, mo, "awlp")
    assert torch.isfinite(got).all() and torch.equal(got[0, :, 3, 5], dms[0, :, 3, 5])
    _within_an_ulp(got, metrics.awlp_inject(ms, pan, low, mo.cpu().numpy(), "awlp"), "I == 0")
    flat = torch.full_like(dlow, 0.4)                                                   # var(L) == 0: non-finite throughout
    plain = cu(inject_inputs(4)[0])                                                     # ... on a scene without an I == 0 pixel
    mo0 = ops.plane_moments(plain, flat)
    assert float(mo0[0, 4, 4]) == 0.0
    for mode in metrics.ATROUS_MODES:
        assert not torch.isfinite(ops.awlp_inject(plain, dpan, flat, mo0, mode)).any()
    for call in (lambda: ops.awlp_inject(dms, dpan, dlow, mo, "hpm"),
                 lambda: ops.awlp_inject(dms, dpan, dlow, mo, "awlp", out=dpan.expand_as(dms)),
                 lambda: ops.awlp_inject(dms, dpan, dlow, mo, "awlp", out=dms[:, :, :-1]),
                 lambda: ops.awlp_inject(dms, dpan, dlow[..., :-1].contiguous(), mo, "awlp"),
                 lambda: ops.awlp_inject(dms, dpan, dlow, mo.float(), "awlp"),
                 lambda: ops.awlp_inject(dms, dpan, dlow, mo[:, :-1].contiguous(), "awlp"),
                 lambda: ops.awlp_inject(torch.zeros(1, 15, 4, 4, device="cuda"), torch.zeros(1, 1, 4, 4, device="cuda"),
                                         torch.zeros(1, 1, 4, 4, device="cuda"), torch.zeros(1, 16, 17, device="cuda", dtype=torch.float64),
                                         "awlp"),
                 lambda: ops.awlp(dms, dpan, 3),
                 lambda: ops.awlp(dms, dpan, 4, "cbd"),
                 lambda: ops.awlp(dms, dpan, 4, out=dpan.expand_as(dms)),
                 lambda: ops.awlp(dms, dpan, 4, buffers=ops.awlp_buffers(2, 4, 20, 28, "cuda")),
                 lambda: ops.awlp_buffers(1, 15, 8, 8, "cuda"),
                 lambda: ops.awlp_buffers(1, 4, 8, 8, "cuda", 3)):
        with pytest.raises(ValueError):
            call()


# ---- the whole chain ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fused64(name):
    """(ms_exp, pan, the float64 definition's result) of a case, computed once and shared (read-only)."""
    from tmdiff_amd import metrics
    case = AWLP_CASES[name]
    ms, pan = awlp_scene(name)
    want = metrics.awlp(ms, pan, case["ratio"], case["mode"])
    for a in (ms, pan, want):
        a.setflags(write=False)
    return ms, pan, want


@pytest.mark.parametrize("name", list(AWLP_CASES))
def test_chain_against_the_definition(name):
    from tmdiff_amd import ops
    case = AWLP_CASES[name]
    ms, pan, want = fused64(name)
    dms, dpan = cu(ms), cu(pan)
    got = ops.awlp(dms, dpan, case["ratio"], case["mode"])
    err = awlp_error_u(got.cpu().numpy(), want)
    print(f"awlp {name}: |F - F64| = {err:.3f} float32 ulps of max |F64| (tolerance {awlp_tol_u(name):.0f})")
    assert torch.isfinite(got).all() and err <= awlp_tol_u(name)
    assert torch.equal(ops.awlp(dms, dpan, case["ratio"], case["mode"]), got)          # a second call
    low = ops.atrous_lowpass(dpan, 1 if case["ratio"] == 2 else 2)
    assert torch.equal(ops.awlp_inject(dms, dpan, low, ops.plane_moments(dms, low), case["mode"]), got)
    work = dms.clone()
    assert ops.awlp(work, dpan, case["ratio"], case["mode"], out=work) is work and torch.equal(work, got)      # in place
    if case["shape"][0] > 1:                                                            # a batch equals its samples
        assert torch.equal(ops.awlp(dms[1:].contiguous(), dpan[1:].contiguous(), case["ratio"], case["mode"]), got[1:])
    # "atwt" is the additive MTF-GLP on the one low-pass plane; the two take their variances from different moment kernels
    atwt = ops.awlp(dms, dpan, case["ratio"], "atwt")
    glp = ops.mtf_glp(dms, dpan, None, case["ratio"], mode="glp", pan_lp=low.expand_as(dms).contiguous())
    _within_an_ulp(atwt, glp.cpu().numpy(), (name, "atwt against glp"))


def test_chain_graph_replay_and_no_allocation():
    from tmdiff_amd import ops
    name = "3 bands x2 34x66 awlp"
    case = AWLP_CASES[name]
    ms, pan, _ = fused64(name)
    eager = ops.awlp(cu(ms), cu(pan), case["ratio"], case["mode"])
    buf, out = ops.awlp_buffers(*case["shape"], "cuda", case["ratio"]), torch.empty(case["shape"], device="cuda")
    dms, dpan = torch.zeros_like(cu(ms)), torch.zeros_like(cu(pan))
    ops.awlp(dms, dpan, case["ratio"], case["mode"], out=out, buffers=buf)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    ops.awlp(dms, dpan, case["ratio"], case["mode"], out=out, buffers=buf)
    assert torch.cuda.memory_allocated() == before
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.awlp(dms, dpan, case["ratio"], case["mode"], out=out, buffers=buf)
    dms.copy_(cu(ms))
    dpan.copy_(cu(pan))
    for _ in range(2):
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


# ---- users ----------------------------------------------------------------------------------------------------------------------
def test_tiling_awlp_fuse():
    from tmdiff_amd import metrics as M, ops
    from tmdiff_amd.tiling import awlp_fuse, consistency_refine
    g = torch.Generator().manual_seed(12)
    lr, pan = (0.1 + 0.8 * torch.rand(1, 4, 16, 16, generator=g)), (0.1 + 0.8 * torch.rand(1, 1, 64, 64, generator=g))
    host = awlp_fuse(lr, pan)                                                           # host data: the float64 definition
    assert host.dtype == torch.float64 and np.array_equal(host.numpy(), M.awlp(M.upsample_poly23(lr.numpy(), 4), pan.numpy(), 4))
    lr, pan = lr.cuda(), pan.cuda()
    for mode in M.ATROUS_MODES:
        base = ops.awlp(ops.upsample_poly23(lr, 4), pan, 4, mode)
        assert torch.equal(awlp_fuse(lr, pan, mode=mode), base)
    scene, score = awlp_fuse(lr, pan, score=True)
    want = M.quality_fullres(lr, pan, scene)
    assert torch.equal(scene, base) and set(score) == set(want) and all(torch.equal(score[k], want[k]) for k in want)
    refined = awlp_fuse(lr, pan, "QB", consistency={"iters": 2})
    assert torch.equal(refined, consistency_refine(base, lr, "QB", 4, iters=2))
    scene, hq = awlp_fuse(lr, pan, "QB", score="hqnr")
    want = M.quality_hqnr(ops.upsample_poly23(lr, 4), pan, scene, "QB", 4)
    assert torch.equal(scene, base) and set(hq) == set(M.HQNR_FIELDS) and all(torch.equal(hq[k], want[k]) for k in want)
    with pytest.raises(ValueError):
        awlp_fuse(lr, pan, score="hqnr")


def test_val_dataset_atrous_baselines(tmp_path):
    from test_bdsd_host import bdsd_inputs
    from test_gpu_bdsd import _Trainer
    from tmdiff_amd import evaluate, metrics as M, ops
    loader = []
    for seed in (31, 32):
        ms, pan = bdsd_inputs(seed, 1, 4, 64, 64)
        hr = (0.5 * ms + 0.5 * pan).clamp(0, 1)
        loader.append({"MS": ms.cuda(), "PAN": pan.cuda(), "LR": ms[..., 2::4, 2::4].contiguous().cuda(), "HR": hr.cuda()})
    kw = dict(device_metrics=True, log=lambda *a: None)
    base = evaluate.val_dataset(_Trainer(), "QB", loader, str(tmp_path / "base"), baselines=("exp",), **kw)
    got = evaluate.val_dataset(_Trainer(), "QB", loader, str(tmp_path / "awlp"), baselines=("exp", "awlp", "atwt"), **kw)
    fields = ("ssim", "sam", "psnr", "ergas", "scc", "cc", "q")
    assert set(got) == set(base) | {f"{k}_QB@{m}" for k in fields for m in ("awlp", "atwt")}
    assert all(got[k] == base[k] for k in base if k != "sec_per_item")                # the @exp keys and the plain keys are unchanged
    for mode in ("awlp", "atwt"):
        rows = [ops.metrics_pair(d["HR"], ops.awlp(d["MS"], d["PAN"], 4, mode), 1.0)[0].cpu().numpy() for d in loader]
        want = dict(zip(M.PAIR_FIELDS, np.mean(rows, 0)))
        for k in fields:
            assert np.isfinite(got[f"{k}_QB@{mode}"]) and abs(got[f"{k}_QB@{mode}"] - want[k]) <= 1e-9 * max(1.0, abs(want[k])), (k, mode)
    assert evaluate.ATROUS_BASELINES == ("atwt", "awlp")
    plain = evaluate.val_dataset(_Trainer(), "QB", loader, str(tmp_path / "plain"), baselines=(), **kw)
    assert set(plain) == {k for k in base if "@" not in k} and all(plain[k] == base[k] for k in plain if k != "sec_per_item")
