"""BDSD on the device: the normal equations per block (bdsd_gram_kernel, the fp64 matrix instruction), the weights
(bdsd_solve_kernel), the injection (bdsd_inject_kernel), ``ops.bdsd`` and its users (csrc/bdsd.hip), against the float64 host
definitions of tmdiff_amd/metrics.py and, where bits are promised, against the device's own other route.

Scene shapes and inputs come from tests/test_bdsd_host.py.  Bounds:
  gram      exact on integer images (values 0 .. 15 in all three inputs: every product and partial sum is an integer below 2^53);
            on general images each raw sum against numpy's fp64 sum of the same terms within (n + 2) 2^-53 sum |terms|, the worst
            case of any order with one rounding per product and per addition; N exactly symmetric; the same bits from two calls
            and a graph replay.
  solve     on the host's float64 moments: 64 (C + 1)^2 cond(N) 2^-53 max|gamma| per block; cond(N) <= 1e6 in every block.
  inject    one float32 ulp, taken at the largest magnitude among the pixel's operands (M_c, the products gamma[k, c] M_k and
            gamma[C, c] P) and the result, of the float64 formula on the device's own weights.
  whole     max |device - float64 definition| at most twice that of the float32 restatement (the two filters in float32 numpy in
            the kernels' order, everything else in float64, rounded once) at the same shape.
The measured worst values are in profiles/bdsd.txt."""
import numpy as np
import pytest
import torch

from test_bdsd_host import BDSD_CASES, BDSD_IDS, COND_MAX, bdsd_inputs, reduced_inputs, singular_moments, worst_cond
from test_glp_host import U, fma32

pytestmark = pytest.mark.gpu

# reduced-scale shapes given directly to ops.bdsd_moments: [B, C, h, w], block side, viewed off a 16-byte boundary
GRAM_CASES = [
    ((2, 15, 9, 7), None, False),               # the widest tile; 63 pixels: a tail inside a K group and inside a 16-byte load
    ((1, 3, 17, 241), None, False),             # 4097 pixels: whole chunks plus one pixel
    ((1, 4, 16, 24), 8, False),                 # six blocks, aligned rows
    ((1, 8, 18, 27), 9, False),                 # odd block rows: the scalar path inside a block
    ((1, 8, 16, 16), 8, True),                  # 16-byte loads ruled out by the base address alone
]
GRAM_IDS = ["9x7x15", "17x241x3", "16x24x4/8", "18x27x8/9", "16x16x8/8+4B"]
# shapes given directly to ops.bdsd_inject beside the scenes: [B, C, H, W], block
INJECT_CASES = [((1, 3, 18, 27), 9), ((2, 15, 8, 12), None), ((1, 2, 40, 64), 8)]
INJECT_IDS = ["18x27x3/9", "8x12x15", "40x64x2/8"]
_CACHE = {}


def _shifted(t):
    """A copy of t that starts 4 bytes off a 16-byte boundary: the kernels take their scalar path."""
    pad = torch.zeros(t.numel() + 1, device="cuda", dtype=t.dtype)
    view = pad[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4
    return view


def _tiles(x, bs):
    """x [B, K, h, w] -> [B, nby, nbx, K, n]: the blocks of side bs (None: the image), their pixels in row-major order."""
    b, k, h, w = x.shape
    by, bx = (h, w) if bs is None else (bs, bs)
    return x.reshape(b, k, h // by, by, w // bx, bx).transpose(0, 2, 4, 1, 3, 5).reshape(b, h // by, w // bx, k, by * bx)


def _scene(i):
    """Everything the tests share about scene i, made once: the inputs on both sides, the device's chain stage by stage and the
    float64 definition."""
    if i not in _CACHE:
        from tmdiff_amd import metrics as M, ops
        (b, c, h, w), ratio, sensor, block = BDSD_CASES[i]
        ms, pan = bdsd_inputs(400 + i, b, c, h, w)
        dms, dpan = ms.cuda(), pan.cuda()
        buf = ops.bdsd_buffers(b, c, h, w, "cuda", ratio, block)
        fused = ops.bdsd(dms, dpan, sensor, ratio, block, buffers=buf)
        torch.cuda.synchronize()
        _CACHE[i] = dict(shape=(b, c, h, w), ratio=ratio, sensor=sensor, block=block, ms=ms, pan=pan, dms=dms, dpan=dpan, buf=buf,
                         fused=fused, want=M.bdsd(ms.numpy(), pan.numpy(), sensor, ratio, block))
    return _CACHE[i]


# ---- the normal equations -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(5), ids=GRAM_IDS)
def test_gram_is_exact_on_integers(i):
    from tmdiff_amd import ops
    (b, c, h, w), bs, shift = GRAM_CASES[i]
    g = torch.Generator().manual_seed(i)
    lp, pan, ms = (torch.randint(0, 16, (b, k, h, w), generator=g).float() for k in (c, 1, c))
    dev = [(_shifted(t.cuda()) if shift else t.cuda()) for t in (lp, pan, ms)]
    got = ops.bdsd_moments(*dev, bs).cpu().numpy()
    hm = _tiles(torch.cat([lp, pan], 1).numpy().astype(np.int64), bs)
    d = _tiles((ms - lp).numpy().astype(np.int64), bs)
    want = np.concatenate([hm @ hm.swapaxes(-1, -2), hm @ d.swapaxes(-1, -2)], -1)
    assert got.shape == want.shape and np.array_equal(got, want.astype(np.float64)), np.argwhere(got != want)[:8]


@pytest.mark.parametrize("i", range(5), ids=GRAM_IDS)
def test_gram_within_the_worst_case_of_any_order(i):
    from tmdiff_amd import ops
    (b, c, h, w), bs, shift = GRAM_CASES[i]
    lp, pan, ms = reduced_inputs(500 + i, b, c, h, w)
    dev = [(_shifted(t.cuda()) if shift else t.cuda()) for t in (lp, pan, ms)]
    got = ops.bdsd_moments(*dev, bs).cpu().numpy()
    hm = _tiles(torch.cat([lp, pan], 1).numpy().astype(np.float64), bs)
    d = _tiles(ms.numpy().astype(np.float64) - lp.numpy().astype(np.float64), bs)
    n = hm.shape[-1]
    want = np.concatenate([np.einsum("...in,...jn->...ij", hm, hm), np.einsum("...in,...jn->...ij", hm, d)], -1)
    bound = (n + 2) * 2.0 ** -53 * np.concatenate([np.einsum("...in,...jn->...ij", np.abs(hm), np.abs(hm)),
                                                   np.einsum("...in,...jn->...ij", np.abs(hm), np.abs(d))], -1)
    err = np.abs(got - want)
    print(f"gram {GRAM_IDS[i]}: worst error / bound {np.max(err / np.maximum(bound, 1e-300)):.3e}, worst cond(N) {worst_cond(got):.3e}")
    assert (err <= bound).all(), (err, bound)
    assert worst_cond(got) <= COND_MAX
    assert np.array_equal(got[..., :c + 1], got[..., :c + 1].swapaxes(-1, -2))       # exactly symmetric


def test_moments_repeat_bit_for_bit():
    from tmdiff_amd import ops
    (b, c, h, w), bs, _ = GRAM_CASES[2]
    dev = [t.cuda() for t in reduced_inputs(502, b, c, h, w)]
    first = ops.bdsd_moments(*dev, bs)
    ws, out = ops.bdsd_moments_workspace(b, c, h, w, "cuda", bs), torch.empty_like(first)
    assert torch.equal(ops.bdsd_moments(*dev, bs), first)
    ops.bdsd_moments(*dev, bs, out=out, workspace=ws)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.bdsd_moments(*dev, bs, out=out, workspace=ws)
    out.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, first)


# ---- the weights ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(5), ids=BDSD_IDS)
def test_solve_on_the_host_moments(i):
    from tmdiff_amd import metrics as M, ops
    case = _scene(i)
    c, ratio, block = case["shape"][1], case["ratio"], case["block"]
    mo = M.bdsd_moments(*M.bdsd_reduced(case["ms"].numpy(), case["pan"].numpy(), case["sensor"], ratio), block and block // ratio)
    want = M.bdsd_coeffs(mo)
    got = ops.bdsd_coeffs(torch.from_numpy(mo).cuda()).cpu().numpy()
    cond = np.linalg.cond(mo[..., :c + 1])
    bound = 64 * (c + 1) ** 2 * cond * 2.0 ** -53 * np.abs(want).max((-2, -1))
    err = np.abs(got - want).max((-2, -1))
    print(f"solve {BDSD_IDS[i]}: worst cond(N) {cond.max():.3e}, worst error / bound {np.max(err / bound):.3e}, "
          f"bits equal to the host's: {np.array_equal(got, want)}")
    assert cond.max() <= COND_MAX and np.isfinite(want).all() and (err <= bound).all(), (err, bound)


def test_solve_of_a_singular_block_is_nan_there_only():
    from tmdiff_amd import metrics as M, ops
    _, _, mo = singular_moments()
    got = ops.bdsd_coeffs(torch.from_numpy(mo).cuda()).cpu().numpy()
    bad = np.isnan(got).all((-2, -1))
    assert bad[0, 1, 0] and bad.sum() == 1 and np.isfinite(got[~bad]).all()
    want = M.bdsd_coeffs(mo)
    assert np.array_equal(np.isnan(want), np.isnan(got))
    print(f"singular block: the other blocks' bits equal the host's: {np.array_equal(got[~bad], want[~bad])}")


# ---- the injection --------------------------------------------------------------------------------------------------------------
def _inject_check(tag, ms, pan, dms, dpan, dgamma, block):
    from tmdiff_amd import metrics as M, ops
    c, (h, w) = ms.shape[1], ms.shape[2:]
    gamma = dgamma.cpu().numpy()
    m64, p64 = ms.numpy().astype(np.float64), pan.numpy().astype(np.float64)
    want = M.bdsd_inject(m64, p64, gamma, block)
    by, bx = (h, w) if block is None else (block, block)
    at = np.repeat(np.repeat(gamma, by, 1), bx, 2)                                   # [B, H, W, C + 1, C]
    planes = np.concatenate([m64, p64], 1)                                           # [B, C + 1, H, W]
    terms = np.zeros_like(m64)                                                       # the largest |product| of the pixel's chain
    for k in range(c + 1):
        terms = np.maximum(terms, np.abs(at[..., k, :].transpose(0, 3, 1, 2) * planes[:, k:k + 1]))
    mag = np.maximum.reduce([np.abs(m64), terms, np.abs(want)])
    ulp = 2.0 ** (np.floor(np.log2(mag)) - 23)
    got = ops.bdsd_inject(dms, dpan, dgamma, block)
    err = np.abs(got.cpu().numpy().astype(np.float64) - want) / ulp
    print(f"inject {tag}: worst error {err.max():.3f} ulp")
    assert np.isfinite(want).all() and err.max() <= 1.0
    inplace = dms.clone()
    assert ops.bdsd_inject(inplace, dpan, dgamma, block, out=inplace) is inplace
    assert torch.equal(inplace, got)
    if w % 4 == 0 and bx % 4 == 0:                                                    # the other path: the same values
        assert torch.equal(ops.bdsd_inject(_shifted(dms), dpan, dgamma, block), got)


@pytest.mark.parametrize("i", range(5), ids=BDSD_IDS)
def test_inject_within_one_ulp(i):
    case = _scene(i)
    _inject_check(BDSD_IDS[i], case["ms"], case["pan"], case["dms"], case["dpan"], case["buf"]["gamma"], case["block"])


@pytest.mark.parametrize("i", range(3), ids=INJECT_IDS)
def test_inject_on_given_weights(i):
    (b, c, h, w), block = INJECT_CASES[i]
    ms, pan = bdsd_inputs(600 + i, b, c, h, w)
    nby, nbx = (1, 1) if block is None else (h // block, w // block)
    gamma = 0.5 * torch.randn(b, nby, nbx, c + 1, c, generator=torch.Generator().manual_seed(i), dtype=torch.float64)
    _inject_check(INJECT_IDS[i], ms, pan, ms.cuda(), pan.cuda(), gamma.cuda(), block)


# ---- end to end -----------------------------------------------------------------------------------------------------------------
def fir_float32(x, taps, ratio):
    """``fir_decimate`` in float32 in the device's documented order: one chain of fused multiply-adds from 0 over the taps in
    row-major order (csrc/mtf.hip), the border replicated, sampled at ratio // 2.  x float32 [B, C, H, W], taps [C, K, K]."""
    x, taps = np.asarray(x, dtype=np.float32), np.asarray(taps).astype(np.float32)
    b, c, h, w = x.shape
    k, rad, o = taps.shape[-1], taps.shape[-1] // 2, ratio // 2
    ho, wo = h // ratio, w // ratio
    xp = np.pad(x, ((0, 0), (0, 0), (rad, rad), (rad, rad)), mode="edge")
    low = np.zeros((b, c, ho, wo), np.float32)
    for u in range(k):
        for v in range(k):
            win = xp[:, :, o + u:o + u + ratio * (ho - 1) + 1:ratio, o + v:o + v + ratio * (wo - 1) + 1:ratio]
            low = fma32(np.broadcast_to(taps[None, :, u, v, None, None], low.shape), win, low)
    return low


@pytest.mark.parametrize("i", range(5), ids=BDSD_IDS)
def test_bdsd_against_the_definition(i):
    from tmdiff_amd import metrics as M, ops
    case = _scene(i)
    ms, pan, ratio, sensor, block = case["ms"].numpy(), case["pan"].numpy(), case["ratio"], case["sensor"], case["block"]
    c = ms.shape[1]
    ms_gains, pan_gain = M.mtf_gains(sensor, c)
    low = ms[..., ratio // 2::ratio, ratio // 2::ratio]
    lp32 = fir_float32(low, np.stack([M.mtf_kernel(g, ratio) for g in ms_gains]), 1)
    pan32 = fir_float32(pan, M.mtf_kernel(pan_gain, ratio)[None], ratio)
    mo = M.bdsd_moments(lp32, pan32, low, block and block // ratio)
    rest = M.bdsd_inject(ms, pan, M.bdsd_coeffs(mo), block).astype(np.float32)
    want, got = case["want"], case["fused"].cpu().numpy()
    unit = U * np.abs(want).max()
    e_dev, e_rest = np.abs(got - want).max() / unit, np.abs(rest - want).max() / unit
    print(f"bdsd {BDSD_IDS[i]}: device {e_dev:.3f} restatement {e_rest:.3f} u max|F|, worst cond(N) {worst_cond(mo):.3e}")
    assert np.isfinite(got).all() and e_dev <= 2.0 * e_rest, (e_dev, e_rest)
    lr = case["dms"][..., ratio // 2::ratio, ratio // 2::ratio].contiguous()
    assert torch.equal(ops.bdsd(case["dms"], case["dpan"], sensor, ratio, block, lr_ms=lr), case["fused"])


def test_capture_and_no_allocation():
    from tmdiff_amd import ops
    case = _scene(1)
    b, c, h, w = case["shape"]
    buf, out = ops.bdsd_buffers(b, c, h, w, "cuda", 4, 32), torch.empty(b, c, h, w, device="cuda")
    ms, pan = torch.zeros_like(case["dms"]), torch.zeros_like(case["dpan"])
    ops.bdsd(ms, pan, "QB", 4, 32, out=out, buffers=buf)                             # warm: the tap tables are cached
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    ops.bdsd(ms, pan, "QB", 4, 32, out=out, buffers=buf)
    assert torch.cuda.memory_allocated() == before
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.bdsd(ms, pan, "QB", 4, 32, out=out, buffers=buf)
    ms.copy_(case["dms"])
    pan.copy_(case["dpan"])
    out.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, case["fused"])


def test_arguments():
    from tmdiff_amd import ops
    case = _scene(1)
    b, c, h, w = case["shape"]
    ms, pan, gamma = case["dms"], case["dpan"], case["buf"]["gamma"]
    wide, wpan = torch.rand(1, 16, 8, 8, device="cuda"), torch.rand(1, 1, 8, 8, device="cuda")
    for call in (lambda: ops.bdsd(wide, wpan, "none"), lambda: ops.bdsd_moments(wide, wpan, wide),
                 lambda: ops.bdsd_inject(wide, wpan, torch.zeros(1, 1, 1, 17, 16, device="cuda", dtype=torch.float64)),
                 lambda: ops.bdsd_buffers(1, 16, 8, 8, "cuda"),
                 lambda: ops.bdsd_coeffs(torch.zeros(1, 1, 1, 17, 33, device="cuda", dtype=torch.float64))):
        with pytest.raises(ValueError, match="C <= 15"):
            call()
    with pytest.raises(ValueError, match="ratio 2 or 4"):
        ops.bdsd(ms, pan, "QB", ratio=3)
    with pytest.raises(ValueError, match="multiple of the ratio that divides H and W"):
        ops.bdsd(ms, pan, "QB", block=24)                                             # 64 % 24 != 0
    with pytest.raises(ValueError, match="multiple of the ratio that divides H and W"):
        ops.bdsd(ms, pan, "QB", block=2)                                              # 2 % 4 != 0
    with pytest.raises(ValueError, match="overlaps pan"):
        ops.bdsd(ms[:, :1].contiguous(), pan, "none", out=pan)
    for call in (lambda: ops.bdsd(ms, pan[..., :32].contiguous(), "QB"),              # wrong shapes
                 lambda: ops.bdsd(ms[..., :62, :].contiguous(), pan[..., :62, :].contiguous(), "QB"),
                 lambda: ops.bdsd(ms, pan, "QB", lr_ms=ms[..., :16, :8].contiguous()),
                 lambda: ops.bdsd(ms, pan, "QB", out=torch.empty(b, c, h, w + 4, device="cuda")),
                 lambda: ops.bdsd(ms, pan, "QB", block=32, buffers=ops.bdsd_buffers(b, c, h, w, "cuda")),
                 lambda: ops.bdsd_inject(ms, pan, gamma),                             # weights of 2 x 2 blocks for one block
                 lambda: ops.bdsd_moments(ms, pan, ms, workspace=torch.empty(8, device="cuda", dtype=torch.float64)),
                 lambda: ops.bdsd(ms.transpose(2, 3), pan.transpose(2, 3), "QB"),     # not contiguous
                 lambda: ops.bdsd(ms.cpu(), pan.cpu(), "QB"),                         # host tensors
                 lambda: ops.bdsd(ms.double(), pan.double(), "QB"),                   # wrong dtypes
                 lambda: ops.bdsd_coeffs(case["buf"]["moments"].float()),
                 lambda: ops.bdsd_inject(ms, pan, gamma.float(), 32)):
        with pytest.raises(ValueError):
            call()


# ---- users ----------------------------------------------------------------------------------------------------------------------
def test_tiling_bdsd_fuse_on_the_device():
    from tmdiff_amd import metrics as M, ops
    from tmdiff_amd.tiling import bdsd_fuse, consistency_refine
    g = torch.Generator().manual_seed(11)
    lr, pan = (0.1 + 0.8 * torch.rand(1, 4, 16, 16, generator=g)).cuda(), (0.1 + 0.8 * torch.rand(1, 1, 64, 64, generator=g)).cuda()
    ms_exp = ops.upsample_poly23(lr, 4)
    for block in (None, 32):
        assert torch.equal(bdsd_fuse(lr, pan, "QB", block=block), ops.bdsd(ms_exp, pan, "QB", 4, block, lr_ms=lr))
    scene, score = bdsd_fuse(lr, pan, "QB", block=32, score="hqnr")
    want = M.quality_hqnr(ms_exp, pan, scene, "QB", 4)
    assert set(score) == set(M.HQNR_FIELDS) and all(torch.equal(score[k], want[k]) for k in want)
    refined = bdsd_fuse(lr, pan, "QB", consistency={"iters": 2})
    assert torch.equal(refined, consistency_refine(ops.bdsd(ms_exp, pan, "QB", lr_ms=lr), lr, "QB", 4, iters=2))


class _Trainer:
    """Stands for the network: the "fused" image is a fixed mix of the visuals."""

    def feed_data(self, d):
        self.d = d

    def test(self, continous=False, prompt="QB"):
        fused = (0.6 * self.d["MS"] + 0.4 * self.d["PAN"]).clamp(0, 1)
        self.SR = torch.cat([torch.zeros_like(fused), fused])                        # a stack; the last image is the result

    def get_current_visuals(self):
        return {"SR": self.SR, **{k: self.d[k] for k in ("MS", "PAN", "LR", "HR")}}


def test_val_dataset_bdsd_baselines(tmp_path):
    from tmdiff_amd import evaluate, metrics as M, ops
    loader = []
    for seed in (21, 22):
        ms, pan = bdsd_inputs(seed, 1, 4, 64, 64)
        hr = (0.5 * ms + 0.5 * pan).clamp(0, 1)
        loader.append({"MS": ms.cuda(), "PAN": pan.cuda(), "LR": ms[..., 2::4, 2::4].contiguous().cuda(), "HR": hr.cuda()})
    kw = dict(device_metrics=True, log=lambda *a: None)
    base = evaluate.val_dataset(_Trainer(), "QB", loader, str(tmp_path / "base"), baselines=("exp",), **kw)
    got = evaluate.val_dataset(_Trainer(), "QB", loader, str(tmp_path / "bdsd"), baselines=("exp", "bdsd"), **kw)
    fields = ("ssim", "sam", "psnr", "ergas", "scc", "cc", "q")
    assert set(got) == set(base) | {f"{k}_QB@bdsd" for k in fields}
    assert all(got[k] == base[k] for k in base if k != "sec_per_item")                # every other key is unchanged
    rows = [ops.metrics_pair(d["HR"], ops.bdsd(d["MS"], d["PAN"], "QB"), 1.0)[0].cpu().numpy() for d in loader]
    want = dict(zip(M.PAIR_FIELDS, np.mean(rows, 0)))
    for k in fields:
        assert np.isfinite(got[f"{k}_QB@bdsd"]) and abs(got[f"{k}_QB@bdsd"] - want[k]) <= 1e-9 * max(1.0, abs(want[k])), k
    with pytest.raises(ValueError, match=r"64, 64.*128"):
        evaluate.val_dataset(_Trainer(), "QB", loader, str(tmp_path / "local"), baselines=("bdsd-local",), **kw)
