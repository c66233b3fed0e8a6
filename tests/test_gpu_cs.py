"""Component substitution on the device: the joint moments (plane_gram_kernel, the fp64 matrix instruction), the constants
(cs_coeffs_kernel), the injection (cs_inject_kernel), ``ops.cs_fuse`` and its users (csrc/cs_fusion.hip), against the float64 host
definitions of tmdiff_amd/metrics.py and, where bits are promised, against the device's own other route.

Shapes and inputs come from tests/test_cs_host.py.  Bounds:
  gram      exact on integer images (every product and partial sum is an integer below 2^53); on general images each raw sum
            against numpy's fp64 sum of the same terms within (n + 2) 2^-53 sum |terms|, the worst case of any order with one
            rounding per product and per addition; the finished moments within 1e-12 of the definition; exactly symmetric;
            the same bits from two calls and a graph replay.
  coeffs    on the host's float64 moments: 64 C^2 cond(S_lr) 2^-53 max|coef| for gsa, 64 C 2^-53 max|coef| otherwise.
  inject    one float32 ulp, taken at the largest magnitude among the pixel's operands (M_c, I, P_I and the result), of the
            float64 formula on the device's own constants.
  whole     max |device - float64 definition| at most twice that of the float32 restatement (the reduced-scale PAN filtered in
            float32 numpy in the kernel's order, everything else in float64, rounded once) at the same shape.
The measured worst values are in profiles/cs_fuse.txt."""
import numpy as np
import pytest
import torch

from test_cs_host import CS_CASES, cs_inputs
from test_glp_host import U, fma32

pytestmark = pytest.mark.gpu

CASE_IDS = ["72x100x4", "64x64x8", "36x70x3@x2", "8x8x1", "9x7x14", "17x241x3", "64x64x8+4B"]
WHOLE = [0, 1, 2, 3, 6]                          # the cases with a ratio
_CACHE = {}


def _shifted(t):
    """A copy of t that starts 4 bytes off a 16-byte boundary: the kernels take their scalar path."""
    pad = torch.zeros(t.numel() + 1, device="cuda")
    view = pad[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4
    return view


def _case(i):
    """Everything the tests share about case i, made once: inputs on both sides, the device's moments (of the inputs and of a
    second pair that stands for the reduced scale) and the raw sums its workspace keeps."""
    if i not in _CACHE:
        from tmdiff_amd import ops
        (b, c, h, w), ratio, sensor = CS_CASES[i]
        ms, pan = cs_inputs(200 + i, b, c, h, w)
        ms2, pan2 = cs_inputs(300 + i, b, c, h, w)
        dms, dpan = ms.cuda(), pan.cuda()
        if i == 6:
            dms = _shifted(dms)
        ws = ops.plane_moments_workspace(b, c, h, w, "cuda")
        dmo = ops.plane_moments(dms, dpan, workspace=ws)
        sums = ws[:b * (c + 2) ** 2].reshape(b, c + 2, c + 2).cpu().numpy()
        dlow = ops.plane_moments(ms2.cuda(), pan2.cuda())
        _CACHE[i] = dict(shape=(b, c, h, w), ratio=ratio, sensor=sensor, ms=ms, pan=pan, dms=dms, dpan=dpan, dmo=dmo, dlow=dlow,
                         sums=sums, mo=dmo.cpu().numpy())
    return _CACHE[i]


def _planes(ms, pan):
    """[B, C + 2, n] float64: the bands and the PAN minus their first pixels, and the plane of ones."""
    b, c, h, w = ms.shape
    x = np.concatenate([ms.reshape(b, c, -1), pan.reshape(b, 1, -1)], 1).astype(np.float64)
    return np.concatenate([x - x[..., :1], np.ones((b, 1, h * w))], 1)


# ---- the moments ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(7), ids=CASE_IDS)
def test_gram_is_exact_on_integers(i):
    from tmdiff_amd import ops
    b, c, h, w = CS_CASES[i][0]
    g = torch.Generator().manual_seed(i)
    ms = torch.randint(0, 16, (b, c, h, w), generator=g).float()
    pan = torch.randint(0, 16, (b, 1, h, w), generator=g).float()
    ws = ops.plane_moments_workspace(b, c, h, w, "cuda")
    ops.plane_moments(_shifted(ms.cuda()) if i == 6 else ms.cuda(), pan.cuda(), workspace=ws)
    x = _planes(ms.numpy(), pan.numpy()).astype(np.int64)
    want = x @ x.transpose(0, 2, 1)
    got = ws[:b * (c + 2) ** 2].reshape(b, c + 2, c + 2).cpu().numpy()
    assert np.array_equal(got, want.astype(np.float64)), np.argwhere(got != want)[:8]


@pytest.mark.parametrize("i", range(7), ids=CASE_IDS)
def test_gram_within_the_worst_case_of_any_order(i):
    from tmdiff_amd import metrics as M
    case = _case(i)
    b, c, h, w = case["shape"]
    n = h * w
    x = _planes(case["ms"].numpy(), case["pan"].numpy())
    want = np.einsum("bin,bjn->bij", x, x)
    bound = (n + 2) * 2.0 ** -53 * np.einsum("bin,bjn->bij", np.abs(x), np.abs(x))
    err = np.abs(case["sums"] - want)
    print(f"gram {CASE_IDS[i]}: worst error / bound {np.max(err / np.maximum(bound, 1e-300)):.3e}")
    assert (err <= bound).all(), (err, bound)
    mo = case["mo"]
    worst = np.abs(mo - M.plane_moments(case["ms"].numpy(), case["pan"].numpy())).max()
    print(f"moments {CASE_IDS[i]}: worst |device - definition| {worst:.3e}")
    assert worst <= 1e-12
    assert np.array_equal(mo[..., :c + 1], mo[..., :c + 1].transpose(0, 2, 1))        # exactly symmetric


def test_moments_repeat_bit_for_bit():
    from tmdiff_amd import ops
    case = _case(0)
    b, c, h, w = case["shape"]
    ws, out = ops.plane_moments_workspace(b, c, h, w, "cuda"), torch.empty(b, c + 1, c + 2, device="cuda", dtype=torch.float64)
    assert torch.equal(ops.plane_moments(case["dms"], case["dpan"]), case["dmo"])
    ops.plane_moments(case["dms"], case["dpan"], out=out, workspace=ws)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.plane_moments(case["dms"], case["dpan"], out=out, workspace=ws)
    out.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, case["dmo"])


# ---- the constants --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(6), ids=CASE_IDS[:6])
def test_coeffs_on_the_host_moments(i):
    from tmdiff_amd import metrics as M, ops
    case = _case(i)
    b, c, h, w = case["shape"]
    full = M.plane_moments(case["ms"].numpy(), case["pan"].numpy())
    low = M.plane_moments(*(t.numpy() for t in cs_inputs(300 + i, b, c, h, w)))
    cond = max(np.linalg.cond(low[k, :c, :c]) for k in range(b))
    dfull, dlow = torch.from_numpy(full).cuda(), torch.from_numpy(low).cuda()
    for method in M.CS_METHODS:
        want = M.cs_coeffs(full, low, method)
        got = ops.cs_coeffs(dfull, dlow if method == "gsa" else None, method).cpu().numpy()
        bound = 64 * (c * c * cond if method == "gsa" else c) * 2.0 ** -53 * np.abs(want).max()
        err = np.abs(got - want).max()
        print(f"coeffs {CASE_IDS[i]} {method}: cond {cond:.1f}, worst error / bound {err / bound:.3e}")
        assert np.isfinite(want).all() and err <= bound, (method, err, bound)


def test_coeffs_of_a_singular_system_are_nan():
    from tmdiff_amd import metrics as M, ops
    case = _case(0)
    ms, pan = case["ms"].numpy().copy(), case["pan"].numpy()
    full = M.plane_moments(ms, pan)
    ms[0, 2] = ms[0, 0]                                                               # image 0: a duplicated band
    low = M.plane_moments(ms, pan)
    got = ops.cs_coeffs(torch.from_numpy(full).cuda(), torch.from_numpy(low).cuda(), "gsa").cpu().numpy()
    assert np.isnan(got[0]).all() and np.isfinite(got[1]).all()
    assert np.isnan(M.cs_coeffs(full, low, "gsa")[0]).all()


# ---- the injection --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ("gs", "gsa", "brovey"))
@pytest.mark.parametrize("i", range(7), ids=CASE_IDS)
def test_inject_within_one_ulp(i, method):
    from tmdiff_amd import metrics as M, ops
    case = _case(i)
    b, c, h, w = case["shape"]
    ms, pan = case["ms"].numpy().astype(np.float64), case["pan"].numpy().astype(np.float64)
    dcoef = ops.cs_coeffs(case["dmo"], case["dlow"], method)
    coef = dcoef.cpu().numpy()
    want = M.cs_inject(ms, pan, coef, method)
    inten = (coef[:, :c, None, None] * ms).sum(1, keepdims=True)
    pi = coef[:, 2 * c, None, None, None] * (pan - coef[:, 2 * c + 2, None, None, None]) + coef[:, 2 * c + 1, None, None, None]
    mag = np.maximum.reduce([np.abs(ms), np.broadcast_to(np.abs(inten), ms.shape), np.broadcast_to(np.abs(pi), ms.shape), np.abs(want)])
    ulp = 2.0 ** (np.floor(np.log2(mag)) - 23)
    got = ops.cs_inject(case["dms"], case["dpan"], dcoef, method)
    err = np.abs(got.cpu().numpy().astype(np.float64) - want) / ulp
    print(f"inject {CASE_IDS[i]} {method}: worst error {err.max():.3f} ulp")
    assert np.isfinite(want).all() and err.max() <= 1.0
    inplace = case["dms"].clone()
    assert ops.cs_inject(inplace, case["dpan"], dcoef, method, out=inplace) is inplace
    assert torch.equal(inplace, got)
    if (h * w) % 4 == 0:                                                              # the other path: the same values
        other = case["dms"].clone() if i == 6 else _shifted(case["dms"])
        assert torch.equal(ops.cs_inject(other, case["dpan"], dcoef, method), got)


# ---- end to end -----------------------------------------------------------------------------------------------------------------
def degrade_float32(pan, gain, ratio):
    """``mtf_degrade`` of a PAN in float32 in the device's documented order: one chain of fused multiply-adds from 0 over the
    taps in row-major order (csrc/mtf.hip).  pan float32 [B, 1, H, W] -> float32 [B, 1, H / ratio, W / ratio]."""
    from tmdiff_amd import metrics as M
    pan = np.asarray(pan, dtype=np.float32)
    b, _, h, w = pan.shape
    taps = M.mtf_kernel(gain, ratio).astype(np.float32)
    k, rad, o = taps.shape[-1], taps.shape[-1] // 2, ratio // 2
    ho, wo = h // ratio, w // ratio
    xp = np.pad(pan[:, 0], ((0, 0), (rad, rad), (rad, rad)), mode="edge")
    low = np.zeros((b, 1, ho, wo), np.float32)
    for u in range(k):
        for v in range(k):
            win = xp[:, None, o + u:o + u + ratio * (ho - 1) + 1:ratio, o + v:o + v + ratio * (wo - 1) + 1:ratio]
            low = fma32(np.broadcast_to(taps[u, v], low.shape), win, low)
    return low


@pytest.mark.parametrize("i", WHOLE, ids=[CASE_IDS[i] for i in WHOLE])
def test_cs_fuse_against_the_definition(i):
    from tmdiff_amd import metrics as M, ops
    case = _case(i)
    ms, pan, ratio, sensor = case["ms"].numpy(), case["pan"].numpy(), case["ratio"], case["sensor"]
    c = ms.shape[1]
    full = M.plane_moments(ms, pan)
    low32 = M.plane_moments(ms[..., ratio // 2::ratio, ratio // 2::ratio], degrade_float32(pan, M.mtf_gains(sensor, c)[1], ratio))
    for method in M.CS_METHODS:
        want = M.cs_fuse(ms, pan, sensor, ratio, method)
        rest = M.cs_inject(ms, pan, M.cs_coeffs(full, low32, method), method).astype(np.float32)
        got = ops.cs_fuse(case["dms"], case["dpan"], sensor, ratio, method).cpu().numpy()
        unit = U * np.abs(want).max()
        e_dev, e_rest = np.abs(got - want).max() / unit, np.abs(rest - want).max() / unit
        print(f"cs_fuse {CASE_IDS[i]} {method}: device {e_dev:.3f} restatement {e_rest:.3f} u max|F|")
        assert np.isfinite(got).all() and e_dev <= 2.0 * e_rest, (method, e_dev, e_rest)
    lr = case["dms"][..., ratio // 2::ratio, ratio // 2::ratio].contiguous()
    assert torch.equal(ops.cs_fuse(case["dms"], case["dpan"], sensor, ratio, "gsa", lr_ms=lr),
                       ops.cs_fuse(case["dms"], case["dpan"], sensor, ratio, "gsa"))


def test_capture_and_no_allocation():
    from tmdiff_amd import ops
    case = _case(0)
    b, c, h, w = case["shape"]
    want = ops.cs_fuse(case["dms"], case["dpan"], "QB", 4, "gsa")
    buf, out = ops.cs_fuse_buffers(b, c, h, w, "cuda"), torch.empty(b, c, h, w, device="cuda")
    ms, pan = torch.zeros_like(case["dms"]), torch.zeros_like(case["dpan"])
    ops.cs_fuse(ms, pan, "QB", 4, "gsa", out=out, buffers=buf)                       # warm: the tap table is cached
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    ops.cs_fuse(ms, pan, "QB", 4, "gsa", out=out, buffers=buf)
    assert torch.cuda.memory_allocated() == before
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.cs_fuse(ms, pan, "QB", 4, "gsa", out=out, buffers=buf)
    ms.copy_(case["dms"])
    pan.copy_(case["dpan"])
    out.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)


def test_arguments():
    from tmdiff_amd import ops
    case = _case(0)
    b, c, h, w = case["shape"]
    ms, pan, mo = case["dms"], case["dpan"], case["dmo"]
    coef = ops.cs_coeffs(mo, None, "gs")
    with pytest.raises(ValueError, match="overlaps pan"):
        ops.cs_inject(ms[:1, :1], pan[:1], coef[:1, [0, c, 2 * c, 2 * c + 1, 2 * c + 2]].contiguous(), "gs", out=pan[:1])
    with pytest.raises(ValueError, match="overlaps pan"):
        ops.cs_fuse(ms[:1, :1], pan[:1], method="gs", out=pan[:1])
    both = torch.empty(b * (2 * c + 3) * 2 + b * c * h * w, device="cuda")            # coef and out in one allocation
    co_in = both[:b * (2 * c + 3) * 2].view(torch.float64).view(b, 2 * c + 3)
    with pytest.raises(ValueError, match="overlaps coef"):
        ops.cs_inject(ms, pan, co_in, "gs", out=both[7:7 + b * c * h * w].view(b, c, h, w))
    with pytest.raises(ValueError, match="overlaps full"):
        ops.cs_coeffs(mo, None, "gs", out=mo.view(-1)[:b * (2 * c + 3)].view(b, 2 * c + 3))
    wide, wpan = torch.rand(1, 15, 8, 8, device="cuda"), torch.rand(1, 1, 8, 8, device="cuda")
    for call in (lambda: ops.cs_fuse(wide, wpan, method="gs"),
                 lambda: ops.plane_moments(wide, wpan),
                 lambda: ops.cs_inject(wide, wpan, torch.zeros(1, 33, device="cuda", dtype=torch.float64), "gs"),
                 lambda: ops.cs_fuse_buffers(1, 15, 8, 8, "cuda")):
        with pytest.raises(ValueError, match="C <= 14"):
            call()
    with pytest.raises(ValueError, match="C <= 14"):
        ops.cs_coeffs(torch.zeros(1, 16, 17, device="cuda", dtype=torch.float64), None, "gs")
    for call in (lambda: ops.cs_fuse(ms, pan[..., :96].contiguous(), "QB"),           # wrong shapes
                 lambda: ops.cs_fuse(ms, pan[:, 0], "QB"),
                 lambda: ops.plane_moments(ms, pan[:1]),
                 lambda: ops.cs_inject(ms, pan, coef[:, :5].contiguous(), "gs"),
                 lambda: ops.cs_coeffs(mo, mo[:1], "gsa"),
                 lambda: ops.cs_coeffs(mo, None, "gsa"),                              # gsa without its reduced-scale moments
                 lambda: ops.cs_fuse(ms, pan, method="gsa"),                          # ... and without a sensor
                 lambda: ops.cs_fuse(ms[..., :70, :].contiguous(), pan[..., :70, :].contiguous(), "QB"),   # 70 % 4 != 0
                 lambda: ops.cs_fuse(ms, pan, "QB", ratio=3),
                 lambda: ops.cs_fuse(ms, pan, "QB", lr_ms=ms[..., :18, :24].contiguous()),
                 lambda: ops.cs_fuse(ms, pan, "QB", out=torch.empty(b, c, h, w + 4, device="cuda")),
                 lambda: ops.cs_fuse(ms, pan, "QB", buffers=ops.cs_fuse_buffers(1, c, h, w, "cuda")),
                 lambda: ops.plane_moments(ms, pan, out=torch.empty(b, c + 1, c + 1, device="cuda", dtype=torch.float64)),
                 lambda: ops.plane_moments(ms, pan, workspace=torch.empty(8, device="cuda", dtype=torch.float64)),
                 lambda: ops.cs_fuse(ms.transpose(2, 3), pan.transpose(2, 3), "QB"),  # not contiguous
                 lambda: ops.plane_moments(ms, pan.transpose(2, 3)),
                 lambda: ops.cs_inject(ms, pan, coef.t().contiguous().t(), "gs"),
                 lambda: ops.cs_coeffs(mo.transpose(1, 2), None, "gs"),
                 lambda: ops.cs_fuse(ms.cpu(), pan.cpu(), "QB"),                      # host tensors
                 lambda: ops.plane_moments(ms, pan.cpu()),
                 lambda: ops.cs_coeffs(mo.cpu(), None, "gs"),
                 lambda: ops.cs_fuse(ms, pan, "QB", method="hpm"),                    # the methods of the other family
                 lambda: ops.cs_inject(ms, pan, coef, "glp"),
                 lambda: ops.cs_coeffs(mo, None, "cbd"),
                 lambda: ops.cs_fuse(ms.double(), pan.double(), "QB"),                # wrong dtypes
                 lambda: ops.plane_moments(ms, pan.double()),
                 lambda: ops.cs_coeffs(mo.float(), None, "gs"),
                 lambda: ops.cs_inject(ms, pan, coef.float(), "gs")):
        with pytest.raises(ValueError):
            call()


# ---- users ----------------------------------------------------------------------------------------------------------------------
def test_tiling_cs_fuse_on_the_device():
    from tmdiff_amd import metrics as M, ops
    from tmdiff_amd.tiling import consistency_refine, cs_fuse
    g = torch.Generator().manual_seed(11)
    lr, pan = (0.1 + 0.8 * torch.rand(1, 4, 16, 16, generator=g)).cuda(), (0.1 + 0.8 * torch.rand(1, 1, 64, 64, generator=g)).cuda()
    ms_exp = ops.upsample_poly23(lr, 4)
    assert torch.equal(ms_exp[..., 2::4, 2::4], lr)
    for method in M.CS_METHODS:
        assert torch.equal(cs_fuse(lr, pan, "QB", method=method), ops.cs_fuse(ms_exp, pan, "QB", 4, method))
    scene, score = cs_fuse(lr, pan, "QB", score="hqnr")
    want = M.quality_hqnr(ms_exp, pan, scene, "QB", 4)
    assert set(score) == set(M.HQNR_FIELDS) and all(torch.equal(score[k], want[k]) for k in want)
    scene, score = cs_fuse(lr, pan, "QB", score=True)
    want = M.quality_fullres(lr, pan, scene)
    assert all(torch.equal(score[k], want[k]) for k in want)
    refined = cs_fuse(lr, pan, "QB", consistency={"iters": 2})
    assert torch.equal(refined, consistency_refine(ops.cs_fuse(ms_exp, pan, "QB"), lr, "QB", 4, iters=2))


def test_val_dataset_cs_baselines(tmp_path):
    from test_gpu_glp import _Trainer
    from tmdiff_amd import evaluate, metrics as M, ops
    loader = []
    for seed in (21, 22):
        ms, pan = cs_inputs(seed, 1, 4, 64, 64)
        hr = (0.5 * ms + 0.5 * pan).clamp(0, 1)
        loader.append({"MS": ms.cuda(), "PAN": pan.cuda(), "LR": ms[..., 2::4, 2::4].contiguous().cuda(), "HR": hr.cuda()})
    kw = dict(full_resolution=True, protocol="hqnr", log=lambda *a: None)
    base = evaluate.val_dataset(_Trainer(), "QB", loader, str(tmp_path / "base"), baselines=("exp", "hpm"), **kw)
    got = evaluate.val_dataset(_Trainer(), "QB", loader, str(tmp_path / "cs"), baselines=("exp", "hpm", "cs-gsa"), **kw)
    assert set(got) == set(base) | {f"{k}_QB@cs-gsa" for k in M.HQNR_FIELDS}
    assert all(got[k] == base[k] for k in base if k != "sec_per_item")                # the other baselines are unchanged
    rows = [ops.metrics_hqnr(ops.cs_fuse(d["MS"], d["PAN"], "QB", 4, "gsa"), d["MS"], d["PAN"], "QB")[0].cpu().numpy() for d in loader]
    want = np.mean(rows, 0)
    for k, field in enumerate(M.HQNR_FIELDS):
        assert abs(got[f"{field}_QB@cs-gsa"] - want[k]) <= 1e-9 * max(1.0, abs(want[k])), field
