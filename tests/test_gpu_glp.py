"""MTF-GLP on the device: the filter bank (fir_decimate_kernel<BANK>, csrc/mtf.hip), the injection statistics
(glp_moments_kernel, csrc/metrics.hip), the injection (glp_inject_kernel, csrc/fusion.hip), ``ops.mtf_glp`` and its users, against
the float64 host definitions of tmdiff_amd/metrics.py and, where bits are promised, against the device's own other route.

Shapes, inputs and the float32 restatement of the low-pass stage come from tests/test_glp_host.py.  Bounds:
  bank      torch.equal with ``fir_decimate`` on the expanded copy; exact against float64 on integer images with dyadic taps.
  moments   each sum about its pilot against numpy's fp64 sum of the same terms within n 2^-53 sum |terms|, the worst case of
            any order; the same bits from two calls and a graph replay.
  inject    one float32 ulp, taken at the largest magnitude among the pixel's operands (M, P_c, PL_c and the result), of the
            float64 formula on the device's own L and moments.
  whole     max |device - float64 definition| at most twice that of the float32 restatement (filter and interpolation in
            float32 numpy in the kernels' orders, statistics and injection in float64) at the same shape.  Measured, in units
            of u max|F| (glp / cbd / hpm, device then restatement): see profiles/mtf_glp.txt."""
import os

import numpy as np
import pytest
import torch

from test_glp_host import GLP_CASES, U, glp_inputs, lowpass_float32

pytestmark = pytest.mark.gpu

CASE_IDS = ["72x100x4", "64x64x8", "36x70x3@x2", "8x8x1"]
_CACHE = {}


def _case(i):
    """Everything the tests share about case i, made once: inputs on both sides, the device's low-pass PAN and moments."""
    if i not in _CACHE:
        from tmdiff_amd import metrics as M, ops
        (b, c, h, w), ratio, sensor = GLP_CASES[i]
        ms, pan = glp_inputs(100 + i, b, c, h, w)
        dms, dpan = ms.cuda(), pan.cuda()
        gains = M.mtf_gains(sensor, c)[0]
        dlp = ops.pan_lowpass_bands(dpan, gains, c, ratio)
        ws = ops.glp_moments_workspace(b, c, h, w, "cuda")
        dmo = ops.glp_moments(dms, dpan, dlp, workspace=ws)
        _CACHE[i] = dict(shape=(b, c, h, w), ratio=ratio, sensor=sensor, gains=gains, ms=ms, pan=pan, dms=dms, dpan=dpan, dlp=dlp,
                         dmo=dmo, sums=ws[:b * c * 7].reshape(b, c, 7).cpu().numpy(), lp=dlp.cpu().numpy(), mo=dmo.cpu().numpy())
    return _CACHE[i]


# ---- the filter bank ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (41, 7))
@pytest.mark.parametrize("i", range(4), ids=CASE_IDS)
def test_bank_equals_the_expanded_copy(i, k):
    from tmdiff_amd import ops
    case = _case(i)
    b, c, h, w = case["shape"]
    taps = torch.randn(c, k, k, generator=torch.Generator().manual_seed(k + i)).cuda()
    for ratio in (1, 2, 4):
        want = ops.fir_decimate(case["dpan"].expand(b, c, h, w).contiguous(), taps, ratio)
        got = ops.fir_decimate_bank(case["dpan"], taps, ratio)
        assert got.shape == want.shape and torch.equal(got, want), (ratio, k)
        assert torch.equal(ops.fir_decimate_bank(case["dpan"][:, 0], taps, ratio), want)           # pan as [B, H, W]
    off = ops.fir_decimate_bank(case["dpan"], taps, 4, offset=(1, 3))
    assert torch.equal(off, ops.fir_decimate(case["dpan"].expand(b, c, h, w).contiguous(), taps, 4, offset=(1, 3)))


@pytest.mark.parametrize("k", (41, 7))
def test_bank_is_exact_on_integers(k):
    from tmdiff_amd import metrics as M, ops
    g = torch.Generator().manual_seed(3)
    x = torch.randint(0, 16, (2, 1, 37, 50), generator=g).float()
    taps = torch.randint(-8, 9, (3, k, k), generator=g).float() / 64.0             # 41^2 * 15 * 8 < 2^24: every partial sum is exact
    for ratio in (1, 2, 4):
        want = M.fir_decimate(np.broadcast_to(x.numpy(), (2, 3, 37, 50)), taps.numpy(), ratio)
        got = ops.fir_decimate_bank(x.cuda(), taps.cuda(), ratio).cpu().numpy().astype(np.float64)
        assert np.array_equal(got, want), ratio


# ---- the moments ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(4), ids=CASE_IDS)
def test_moment_sums_within_the_worst_case_of_any_order(i):
    from tmdiff_amd import metrics as M
    case = _case(i)
    b, c, h, w = case["shape"]
    n = h * w
    ms, lp, pan = case["ms"].numpy().astype(np.float64), case["lp"].astype(np.float64), case["pan"].numpy().astype(np.float64)
    dm, dl, dp = ms - ms[..., :1, :1], lp - lp[..., :1, :1], np.broadcast_to(pan - pan[..., :1, :1], ms.shape)
    terms = [dm, dl, dp, dm * dm, dl * dl, dm * dl, dp * dp]                        # the order of the workspace's sums
    for k, t in enumerate(terms):
        want, bound = t.sum((-2, -1)), n * 2.0 ** -53 * np.abs(t).sum((-2, -1))
        err = np.abs(case["sums"][..., k] - want)
        print(f"case {i} sum {k}: worst error / bound {np.max(err / np.maximum(bound, 1e-300)):.3e}")
        assert (err <= bound).all(), (k, err, bound)
    # and the moments made from them are the definition's: both sides are fp64 and centred, (range / sigma)^2 < 20 here
    want = M.glp_moments(ms, pan, lp)
    assert np.abs(case["mo"] - want).max() <= 1e-12, np.abs(case["mo"] - want).max()


def test_moments_repeat_bit_for_bit():
    from tmdiff_amd import ops
    case = _case(0)
    b, c, h, w = case["shape"]
    ws, out = ops.glp_moments_workspace(b, c, h, w, "cuda"), torch.empty(b, c, 7, device="cuda", dtype=torch.float64)
    again = ops.glp_moments(case["dms"], case["dpan"], case["dlp"])
    assert torch.equal(again, case["dmo"])
    ops.glp_moments(case["dms"], case["dpan"], case["dlp"], out=out, workspace=ws)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.glp_moments(case["dms"], case["dpan"], case["dlp"], out=out, workspace=ws)
    out.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, case["dmo"])


# ---- the injection --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ("glp", "cbd", "hpm"))
@pytest.mark.parametrize("i", range(4), ids=CASE_IDS)
def test_inject_within_one_ulp(i, mode):
    from tmdiff_amd import metrics as M, ops
    case = _case(i)
    ms, pan = case["ms"].numpy().astype(np.float64), case["pan"].numpy().astype(np.float64)
    lp, mo = case["lp"].astype(np.float64), case["mo"]
    want = M.glp_inject(ms, pan, lp, mo, mode)
    a = np.sqrt(mo[..., 3] / mo[..., 4])[..., None, None]
    pc = a * (pan - mo[..., 2, None, None]) + mo[..., 0, None, None]
    plc = a * (lp - mo[..., 2, None, None]) + mo[..., 0, None, None]
    mag = np.maximum.reduce([np.abs(ms), np.abs(pc), np.abs(plc), np.abs(want)])
    ulp = 2.0 ** (np.floor(np.log2(mag)) - 23)
    got = ops.glp_inject(case["dms"], case["dpan"], case["dlp"], case["dmo"], mode)
    err = np.abs(got.cpu().numpy().astype(np.float64) - want) / ulp
    print(f"case {i} {mode}: worst error {err.max():.3f} ulp")
    assert np.isfinite(want).all() and err.max() <= 1.0
    inplace = case["dms"].clone()
    assert ops.glp_inject(inplace, case["dpan"], case["dlp"], case["dmo"], mode, out=inplace) is inplace
    assert torch.equal(inplace, got)
    if case["shape"][3] % 4 == 0:                                                    # the scalar path: the same values
        b, c, h, w = case["shape"]
        pad = torch.zeros(b * c * h * w + 1, device="cuda")
        shifted = pad[1:].view(b, c, h, w)                                            # 4 bytes off a 16-byte boundary
        shifted.copy_(case["dms"])
        assert torch.equal(ops.glp_inject(shifted, case["dpan"], case["dlp"], case["dmo"], mode), got)


# ---- end to end -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(4), ids=CASE_IDS)
def test_mtf_glp_against_the_definition(i):
    from tmdiff_amd import metrics as M, ops
    case = _case(i)
    ms, pan = case["ms"].numpy(), case["pan"].numpy()
    lp32 = lowpass_float32(pan, case["gains"], case["ratio"])
    mo32 = M.glp_moments(ms, pan, lp32)
    for mode in M.GLP_MODES:
        want = M.mtf_glp(ms, pan, case["sensor"], case["ratio"], mode)
        rest = M.glp_inject(ms, pan, lp32, mo32, mode).astype(np.float32)
        got = ops.mtf_glp(case["dms"], case["dpan"], case["sensor"], case["ratio"], mode).cpu().numpy()
        unit = U * np.abs(want).max()
        e_dev, e_rest = np.abs(got - want).max() / unit, np.abs(rest - want).max() / unit
        print(f"mtf_glp {CASE_IDS[i]} {mode}: device {e_dev:.3f} restatement {e_rest:.3f} u max|F|")
        assert np.isfinite(got).all() and e_dev <= 2.0 * e_rest, (mode, e_dev, e_rest)
    given = ops.mtf_glp(case["dms"], case["dpan"], case["sensor"], case["ratio"], "hpm", pan_lp=case["dlp"])
    assert torch.equal(given, ops.glp_inject(case["dms"], case["dpan"], case["dlp"], case["dmo"], "hpm"))


def test_capture_and_no_allocation():
    from tmdiff_amd import ops
    case = _case(0)
    b, c, h, w = case["shape"]
    want = ops.mtf_glp(case["dms"], case["dpan"], "QB", 4, "cbd")
    buf, out = ops.mtf_glp_buffers(b, c, h, w, "cuda"), torch.empty(b, c, h, w, device="cuda")
    ms, pan = torch.zeros_like(case["dms"]), torch.zeros_like(case["dpan"])
    ops.mtf_glp(ms, pan, "QB", 4, "cbd", out=out, buffers=buf)                       # warm: the tap table is cached
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    ops.mtf_glp(ms, pan, "QB", 4, "cbd", out=out, buffers=buf)
    assert torch.cuda.memory_allocated() == before
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.mtf_glp(ms, pan, "QB", 4, "cbd", out=out, buffers=buf)
    ms.copy_(case["dms"])
    pan.copy_(case["dpan"])
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)


def test_arguments():
    from tmdiff_amd import ops
    case = _case(0)
    b, c, h, w = case["shape"]
    ms, pan, lp, mo = case["dms"], case["dpan"], case["dlp"], case["dmo"]
    with pytest.raises(ValueError, match="overlaps pan"):
        ops.glp_inject(ms[:1, :1], pan[:1], lp[:1, :1], mo[:1, :1], "glp", out=pan[:1])
    with pytest.raises(ValueError, match="overlaps pan_lp"):
        ops.glp_inject(ms, pan, lp, mo, "glp", out=lp)
    with pytest.raises(ValueError, match="overlaps pan_lp"):
        ops.mtf_glp(ms, pan, "QB", pan_lp=lp, out=lp)
    with pytest.raises(ValueError, match="overlaps pan"):
        ops.mtf_glp(ms[:1, :1], pan[:1], ((0.3,), 0.15), out=pan[:1])
    both = torch.empty(b * c * 7 * 2 + b * c * h * w, device="cuda")                 # moments and out in one allocation
    mo_in = both[:b * c * 7 * 2].view(torch.float64).view(b, c, 7)
    with pytest.raises(ValueError, match="overlaps moments"):
        ops.glp_inject(ms, pan, lp, mo_in, "glp", out=both[7:7 + b * c * h * w].view(b, c, h, w))
    wide = torch.rand(1, 17, 8, 8, device="cuda")
    for call in (lambda: ops.mtf_glp(wide, pan[:1, :, :8, :8].contiguous(), (tuple([0.3] * 17), 0.15)),
                 lambda: ops.glp_moments(wide, pan[:1, :, :8, :8].contiguous(), wide),
                 lambda: ops.pan_lowpass_bands(pan, 0.3, 17),
                 lambda: ops.mtf_glp_buffers(1, 17, 8, 8, "cuda")):
        with pytest.raises(ValueError, match="C <= 16"):
            call()
    for call in (lambda: ops.mtf_glp(ms, pan[..., :96].contiguous(), "QB"),           # wrong shapes
                 lambda: ops.mtf_glp(ms, pan[:, 0], "QB"),
                 lambda: ops.glp_moments(ms, pan, lp[:, :2].contiguous()),
                 lambda: ops.glp_inject(ms, pan, lp, mo[:, :2].contiguous(), "glp"),
                 lambda: ops.mtf_glp(ms[..., :70, :].contiguous(), pan[..., :70, :].contiguous(), "QB"),   # 70 % 4 != 0
                 lambda: ops.mtf_glp(ms, pan, "QB", ratio=3),
                 lambda: ops.mtf_glp(ms, pan, "QB", out=torch.empty(b, c, h, w + 4, device="cuda")),
                 lambda: ops.mtf_glp(ms, pan, "QB", buffers=ops.mtf_glp_buffers(1, c, h, w, "cuda")),
                 lambda: ops.mtf_glp(ms.transpose(2, 3), pan.transpose(2, 3), "QB"),  # not contiguous
                 lambda: ops.glp_inject(ms, pan, lp.transpose(2, 3), mo, "glp"),
                 lambda: ops.mtf_glp(ms.cpu(), pan.cpu(), "QB"),                      # host tensors
                 lambda: ops.glp_moments(ms, pan.cpu(), lp),
                 lambda: ops.fir_decimate_bank(pan.cpu(), torch.ones(2, 3, 3, device="cuda")),
                 lambda: ops.fir_decimate_bank(pan, torch.ones(2, 4, 4, device="cuda")),
                 lambda: ops.fir_decimate_bank(ms, torch.ones(2, 3, 3, device="cuda")),          # more than one plane per image
                 lambda: ops.mtf_glp(ms, pan, "QB", mode="gsa"),
                 lambda: ops.glp_inject(ms, pan, lp, mo, "gsa"),
                 lambda: ops.mtf_glp(ms.double(), pan.double(), "QB")):
        with pytest.raises(ValueError):
            call()


# ---- users ----------------------------------------------------------------------------------------------------------------------
def test_classical_fuse_on_the_device():
    from tmdiff_amd import metrics as M, ops
    from tmdiff_amd.tiling import classical_fuse, consistency_refine
    g = torch.Generator().manual_seed(11)
    lr, pan = (0.1 + 0.8 * torch.rand(1, 4, 16, 16, generator=g)).cuda(), (0.1 + 0.8 * torch.rand(1, 1, 64, 64, generator=g)).cuda()
    ms_exp = ops.upsample_poly23(lr, 4)
    for mode in M.GLP_MODES:
        assert torch.equal(classical_fuse(lr, pan, "QB", mode=mode), ops.mtf_glp(ms_exp, pan, "QB", 4, mode))
    scene, score = classical_fuse(lr, pan, "QB", score="hqnr")
    want = M.quality_hqnr(ms_exp, pan, scene, "QB", 4)
    assert set(score) == set(M.HQNR_FIELDS) and all(torch.equal(score[k], want[k]) for k in want)
    scene, score = classical_fuse(lr, pan, "QB", score=True)
    want = M.quality_fullres(lr, pan, scene)
    assert all(torch.equal(score[k], want[k]) for k in want)
    refined = classical_fuse(lr, pan, "QB", consistency={"iters": 2})
    assert torch.equal(refined, consistency_refine(ops.mtf_glp(ms_exp, pan, "QB"), lr, "QB", 4, iters=2))


class _Trainer:
    keys = ("MS", "PAN", "LR", "HR")

    def feed_data(self, d):
        self.d = d

    def test(self, continous=False, prompt="QB"):
        fused = (0.6 * self.d["MS"] + 0.4 * self.d["PAN"]).clamp(0, 1)
        self.SR = torch.cat([torch.zeros_like(fused), fused])                        # a stack; the last image is the result

    def get_current_visuals(self):
        return {"SR": self.SR, **{k: self.d[k] for k in self.keys}}


def test_val_dataset_baselines(tmp_path):
    from tmdiff_amd import evaluate, metrics as M, ops
    loader = []
    for seed in (21, 22):
        ms, pan = glp_inputs(seed, 1, 4, 64, 64)
        hr = (0.5 * ms + 0.5 * pan).clamp(0, 1)
        loader.append({"MS": ms.cuda(), "PAN": pan.cuda(), "LR": ms[..., 2::4, 2::4].contiguous().cuda(), "HR": hr.cuda()})
    quiet = dict(log=lambda *a: None)
    modes = {"hqnr": (dict(full_resolution=True, protocol="hqnr"), M.HQNR_FIELDS,
                      lambda d, f: ops.metrics_hqnr(f, d["MS"], d["PAN"], "QB")[0]),
             "qnr": (dict(full_resolution=True), M.NOREF_FIELDS,
                     lambda d, f: ops.metrics_noref(d["LR"], d["PAN"], ops.pyr_down(d["PAN"], 2), f)[0]),
             "pair": (dict(device_metrics=True), ("ssim", "sam", "psnr", "ergas", "scc", "cc", "q"),
                      lambda d, f: ops.metrics_pair(d["HR"], f, 1.0)[0][[M.PAIR_FIELDS.index(k) for k in
                                                                        ("ssim", "sam", "psnr", "ergas", "scc", "cc", "q")]])}
    for name, (kw, fields, row) in modes.items():
        plain = evaluate.val_dataset(_Trainer(), "QB", loader, str(tmp_path / f"{name}_plain"), **kw, **quiet)
        empty = evaluate.val_dataset(_Trainer(), "QB", loader, str(tmp_path / f"{name}_empty"), baselines=(), **kw, **quiet)
        got = evaluate.val_dataset(_Trainer(), "QB", loader, str(tmp_path / f"{name}_base"), baselines=("exp", "hpm"), **kw, **quiet)
        assert set(plain) == set(empty) == {f"{k}_QB" for k in fields} | {"sec_per_item"}
        assert all(plain[k] == empty[k] == got[k] for k in plain if k != "sec_per_item")
        assert set(got) == set(plain) | {f"{k}_QB@{b}" for k in fields for b in ("exp", "hpm")}
        for b in ("exp", "hpm"):
            rows = [row(d, d["MS"] if b == "exp" else ops.mtf_glp(d["MS"], d["PAN"], "QB", 4, b)).cpu().numpy() for d in loader]
            want = np.mean(rows, 0)
            for k, field in enumerate(fields):
                assert abs(got[f"{field}_QB@{b}"] - want[k]) <= 1e-9 * max(1.0, abs(want[k])), (name, b, field)
    with pytest.raises(ValueError, match="baselines"):
        evaluate.val_dataset(_Trainer(), "QB", loader, str(tmp_path / "host"), baselines=("hpm",), **quiet)
    no_ms = _Trainer()
    no_ms.keys = ("PAN", "LR", "HR")
    with pytest.raises(ValueError, match="MS"):
        evaluate.val_dataset(no_ms, "QB", loader, str(tmp_path / "no_ms"), device_metrics=True, baselines=("exp",), **quiet)
    assert os.path.exists(os.path.join(str(tmp_path / "pair_base"), "QB", "output_mulExm_1.mat"))
