"""Fused tiled sampling on the GPU: the gather / blend kernels against the fp64 restatement of tests/test_tiling_host.py, the
tiled denoiser and whole chains against the CPU oracle run tile by tile, and the public switch ``sample_tiled(overlap=)``."""
import collections

import numpy as np
import pytest
import torch

from conftest import assert_close, rel_err
from oracle import unet_ref as U
from oracle.diffusion_ref import GeneralDiffusionRef
from oracle.make_golden import FULL, TINY, case_inputs
from test_tiling_host import JUMP_PLANS, blend_ref, constant_tiles, gather_ref, max_jump

pytestmark = pytest.mark.gpu

# at most 9 products, 9 sums and one division, each rounding at 2^-24: about 1.1e-6 of max|v|
BLEND_TOL = 2e-6


@pytest.fixture(autouse=True)
def _inference_mode():
    with torch.no_grad():
        yield


def cu(t):
    return t.detach().cuda().contiguous()


def cpu_noise(like):
    return torch.randn(like.shape, dtype=torch.float32)


def _pair(channels):
    from tmdiff_amd.Hyper_unet_general import WavBEST
    ref = U.fill_weights_(U.WavBESTRef(channels=channels)).eval()
    net = WavBEST(channels=channels)
    net.load_state_dict(ref.state_dict())
    return ref, net.cuda().eval()


@pytest.fixture(scope="module")
def tiny():
    return _pair(TINY)


class OracleTiled(torch.nn.Module):
    """The CPU statement of TiledDenoiser: the oracle UNet on every tile, blended in fp64."""

    def __init__(self, ref_net, tile, overlap):
        super().__init__()
        self.ref_net, self.tile, self.overlap = ref_net, tile, overlap

    def forward(self, x_t, t_input, PAN=None, MS=None, prompt=None):
        b, _, h, w = x_t.shape
        t = t_input.reshape(-1)
        t = t if t.numel() == b else t.expand(b)
        outs = []
        for i in range(b):
            xs, ps, ms = (torch.from_numpy(gather_ref(a[i:i + 1].numpy(), self.tile, self.overlap)) for a in (x_t, PAN, MS))
            pr = prompt[i] if isinstance(prompt, (list, tuple)) else prompt
            outs.append(self.ref_net(xs, t[i:i + 1].expand(xs.shape[0]).reshape(-1, 1), ps, ms, pr))
        return torch.from_numpy(blend_ref(torch.cat(outs).numpy(), b, h, w, self.overlap)).float()


# ---- 1. kernels against the restatement ------------------------------------------------------------------------------
@pytest.mark.parametrize("b,c,h,w,tile,overlap", [
    (2, 4, 72, 100, 32, 8), (2, 8, 72, 100, 32, 16), (2, 4, 72, 98, 32, 8),      # W % 4 != 0: the scalar path
    (2, 8, 75, 100, 32, 12), (2, 4, 48, 80, 32, 6),                                # step % 4 != 0: the scalar path
    (2, 1, 72, 100, 32, 16), (2, 4, 96, 64, 32, 0), (1, 4, 512, 512, 64, 32), (4, 4, 32, 32, 32, 16), (2, 8, 100, 100, 32, 16)])
def test_gather_and_blend_against_the_restatement(b, c, h, w, tile, overlap):
    from tmdiff_amd import ops
    from tmdiff_amd.tiling import merge_tiles, plan_tiles, split_tiles
    g = torch.Generator().manual_seed(h * 1000 + w + overlap)
    x = torch.randn(b, c, h, w, generator=g)
    rows, cols = plan_tiles(h, w, tile, overlap)
    tiles = ops.tile_gather(cu(x), tile, overlap)
    assert tiles.shape == (b * len(rows) * len(cols), c, tile, tile)
    assert torch.equal(tiles.cpu(), torch.from_numpy(gather_ref(x.numpy(), tile, overlap)))
    v = torch.randn(tiles.shape, generator=g) * 3.0
    got = ops.tile_blend(cu(v), b, h, w, overlap).cpu().double().numpy()
    want = blend_ref(v.numpy(), b, h, w, overlap)
    err = np.abs(got - want).max() / float(v.abs().max())
    print(f"blend [{b},{c},{h},{w}] tile {tile} overlap {overlap}: max error {err:.3e} of max|v|")
    assert err <= BLEND_TOL
    back = ops.tile_blend(tiles, b, h, w, overlap).cpu()
    assert float((back - x).abs().max() / x.abs().max()) <= BLEND_TOL
    if overlap == 0 and h % tile == 0 and w % tile == 0:
        split = split_tiles(cu(x), tile, tile)
        assert torch.equal(tiles, split)
        assert torch.equal(ops.tile_blend(cu(v), b, h, w, 0), merge_tiles(cu(v), h // tile, w // tile))
        assert torch.equal(back, x)


@pytest.mark.parametrize("L,tile,overlap", JUMP_PLANS)
def test_constant_tiles_blend_without_a_jump_on_the_device(L, tile, overlap):
    from tmdiff_amd import ops
    from tmdiff_amd.tiling import plan_tiles
    rows, cols = plan_tiles(L, L, tile, overlap)
    rng = np.random.default_rng(L + 7 * overlap)
    tiles, vals = constant_tiles(rng, 2 * len(rows) * len(cols), 4, tile)
    scene = ops.tile_blend(cu(torch.from_numpy(tiles).float()), 2, L, L, overlap).cpu().numpy()
    bound = (vals.max() - vals.min()) / (overlap + 1) + 2 * BLEND_TOL * np.abs(vals).max()   # two rounded pixels per difference
    assert max_jump(scene) <= bound


def test_wrappers_check_their_arguments():
    from tmdiff_amd import ops
    x = torch.zeros(1, 4, 64, 64)
    with pytest.raises(ValueError):
        ops.tile_gather(x, 32, 8)                                  # not on the GPU
    with pytest.raises(ValueError):
        ops.tile_gather(cu(x), 32, 17)
    with pytest.raises(ValueError):
        ops.tile_gather(cu(x), 128, 0)
    with pytest.raises(ValueError):
        ops.tile_blend(cu(torch.zeros(5, 4, 32, 32)), 1, 64, 64, 0)   # the plan has 4 tiles
    with pytest.raises(ValueError):
        ops.tile_gather(cu(x).double(), 32, 8)


# ---- 2. denoiser against the oracle -----------------------------------------------------------------------------------
def _scene(seed, b, c, h, w):
    d = case_inputs(seed, b, c, h, w)
    return d, {k: cu(v) for k, v in d.items()}


def test_tiled_denoiser_against_the_oracle(tiny):
    from tmdiff_amd.tiling import TiledDenoiser
    ref, net = tiny
    d, dc = _scene(5100, 2, 4, 48, 80)
    prompts = ["GF2", "QB"]
    t = torch.tensor([[321], [77]])
    want = OracleTiled(ref, 32, 16)(d["x_t"], t, d["PAN"], d["MS"], prompts)
    one = TiledDenoiser(net, 32, 16, max_batch=32)(dc["x_t"], t.cuda(), dc["PAN"], dc["MS"], prompts)
    m, l2 = rel_err(one, want)
    print(f"tiled denoiser vs oracle: max-rel {m:.3e} rel-L2 {l2:.3e}")
    assert m <= 1e-4 and l2 <= 1e-5
    several = TiledDenoiser(net, 32, 16, max_batch=4)(dc["x_t"], t.cuda(), dc["PAN"], dc["MS"], prompts)
    assert torch.equal(several, one)
    # a single prompt and a [B] time input take the same path
    same = TiledDenoiser(net, 32, 16)(dc["x_t"], torch.tensor([321, 321]).cuda(), dc["PAN"], dc["MS"], "GF2")
    assert_close(same, OracleTiled(ref, 32, 16)(d["x_t"], torch.tensor([321, 321]), d["PAN"], d["MS"], "GF2"), 1e-4, 1e-5, "one prompt")


def _count(fn):
    from tmdiff_amd import ops
    ops.COUNTS = collections.Counter()
    try:
        fn()
        return sum(ops.COUNTS.values())
    finally:
        ops.COUNTS = None


def test_condition_branch_runs_once_per_chunk_per_run(tiny):
    """16 tiles in 4 chunks of 4, 3 steps inside begin / end_condition_cache: chunks x (c + 3 x) convolution launches."""
    from tmdiff_amd import ops
    from tmdiff_amd.tiling import TiledDenoiser
    _, net = tiny
    d, dc = _scene(5101, 2, 4, 48, 80)
    prompts = ["GF2", "QB"]
    t = torch.full((2, 1), 500.0).cuda()
    chunk = [cu(a) for a in (ops.tile_gather(dc[k], 32, 16)[:4] for k in ("x_t", "PAN", "MS"))]
    tc, pc = torch.full((4, 1), 500.0).cuda(), ["GF2"] * 4
    both = _count(lambda: net(chunk[0], tc, chunk[1], chunk[2], pc))
    net.begin_condition_cache(chunk[1], chunk[2], pc)
    x = _count(lambda: net(chunk[0], tc, chunk[1], chunk[2], pc))
    net.end_condition_cache()
    c = both - x
    assert c > 0 and x > 0
    tiled = TiledDenoiser(net, 32, 16, max_batch=4)

    def run():
        tiled.begin_condition_cache(dc["PAN"], dc["MS"], prompts)
        try:
            return [tiled(dc["x_t"], t, dc["PAN"], dc["MS"], prompts) for _ in range(3)]
        finally:
            tiled.end_condition_cache()
    assert _count(run) == 4 * (c + 3 * x)
    assert net._cond is None
    # outside a cache every step pays for the condition branch, and gives the same numbers
    plain = tiled(dc["x_t"], t, dc["PAN"], dc["MS"], prompts)
    assert torch.equal(plain, run()[0])
    assert _count(lambda: tiled(dc["x_t"], t, dc["PAN"], dc["MS"], prompts)) == 4 * (c + x)
    # ... and the sampler's own cache context reaches it: a 3-step DDPM loop costs the same launches
    from tmdiff_amd.diffusion_general import GeneralDiffusion
    diff = GeneralDiffusion(tiled, "l1", noise_fn=cpu_noise).cuda()
    diff.set_new_noise_schedule({"schedule": "cosine", "n_timestep": 3}, "cuda")
    assert _count(lambda: diff.p_sample_loop(dict(dc), continous=False, prompt=prompts)) == 4 * (c + 3 * x)
    assert tiled._run is None and net._cond is None


# ---- 3. chains ---------------------------------------------------------------------------------------------------------
def test_fused_chains_against_the_oracle(tiny):
    """p_sample_loop (T = 10) and sample_by_dpmsolver(steps=5) over a tiled denoiser, 8-band 32 x 48 scene, tile 32, overlap
    16 (one row of two tiles), noise drawn on the CPU on both sides.  Bounds of tests/test_gpu_sampling.py for chains of these
    lengths: max|d| <= 2e-3, PSNR >= 60 dB."""
    from tmdiff_amd.diffusion_general import GeneralDiffusion
    from tmdiff_amd.tiling import TiledDenoiser
    from tmdiff_amd.util import psnr
    ref, net = tiny
    d, dc = _scene(5102, 1, 8, 32, 48)
    for T, run in ((10, lambda g: g.p_sample_loop(dict(g.inputs), continous=False, prompt="WV3")),
                   (1000, lambda g: g.sample_by_dpmsolver(dict(g.inputs), "WV3", steps=5))):
        ora = GeneralDiffusionRef(OracleTiled(ref, 32, 16), "l1", noise_fn=cpu_noise)
        ora.set_new_noise_schedule({"schedule": "cosine", "n_timestep": T}, "cpu")
        got = GeneralDiffusion(TiledDenoiser(net, 32, 16), "l1", noise_fn=cpu_noise).cuda()
        got.set_new_noise_schedule({"schedule": "cosine", "n_timestep": T}, "cuda")
        ora.inputs, got.inputs = d, dc
        torch.manual_seed(T)
        want = run(ora)
        torch.manual_seed(T)
        have = run(got).cpu()
        diff, db = float((have - want).abs().max()), float(psnr(have, want))
        print(f"fused chain T={T}: max|d| {diff:.3e}, PSNR {db:.1f} dB")
        assert have.shape == want.shape and diff <= 2e-3 and db >= 60.0
        assert got.denoise_fn._run is None and net._cond is None


# ---- 4. public switch --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full():
    return _pair(FULL)[1]


def test_sample_tiled_fused_mode(full):
    from tmdiff_amd.diffusion_general import GeneralDiffusion
    from tmdiff_amd.tiling import sample_tiled
    diff = GeneralDiffusion(full, "l1", noise_fn=cpu_noise).cuda()
    diff.set_new_noise_schedule({"schedule": "cosine", "n_timestep": 1000}, "cuda")
    keys = list(diff.state_dict().keys())
    d = case_inputs(5103, 1, 4, 128)
    scene = {"MS": cu(d["MS"]), "PAN": cu(d["PAN"])}
    torch.manual_seed(8)
    fused = sample_tiled(diff, scene, "GF2", tile=64, method="dpmsolver", steps=3, max_batch=32, overlap=16)
    assert fused.shape == (1, 4, 128, 128) and torch.isfinite(fused).all()
    assert diff.denoise_fn is full and list(diff.state_dict().keys()) == keys and full._cond is None
    diff.sample_graphs = True
    try:
        torch.manual_seed(8)
        graph = sample_tiled(diff, scene, "GF2", tile=64, method="dpmsolver", steps=3, max_batch=32, overlap=16)
    finally:
        diff.sample_graphs = None
    assert torch.equal(graph, fused)
    # scene extents that are no multiple of the tile, several chunks, the DDPM method
    short = GeneralDiffusion(full, "l1", noise_fn=cpu_noise).cuda()
    short.set_new_noise_schedule({"schedule": "cosine", "n_timestep": 2}, "cuda")
    d2 = case_inputs(5104, 1, 4, 72, 100)
    odd = sample_tiled(short, {"MS": cu(d2["MS"]), "PAN": cu(d2["PAN"])}, "QB", tile=64, method="ddpm", max_batch=2, overlap=8)
    assert odd.shape == (1, 4, 72, 100) and torch.isfinite(odd).all()
    # the object is restored when sampling raises, and bad plans are refused before anything is swapped
    with pytest.raises(AttributeError):
        sample_tiled(diff, scene, "no such prompt", tile=64, steps=3, overlap=16)
    assert diff.denoise_fn is full and list(diff.state_dict().keys()) == keys and full._cond is None
    with pytest.raises(ValueError):
        sample_tiled(diff, scene, "GF2", tile=64, steps=3, overlap=40)
    assert diff.denoise_fn is full


def test_sample_tiled_independent_mode_is_unchanged(full):
    """overlap=None: split_tiles -> diffusion.sample in batches of max_batch -> merge_tiles, done by hand with the same seed."""
    from tmdiff_amd.diffusion_general import GeneralDiffusion
    from tmdiff_amd.tiling import merge_tiles, sample_tiled, split_tiles
    diff = GeneralDiffusion(full, "l1", noise_fn=cpu_noise).cuda()
    diff.set_new_noise_schedule({"schedule": "cosine", "n_timestep": 1000}, "cuda")
    d = case_inputs(5105, 1, 4, 128)
    scene = {"MS": cu(d["MS"]), "PAN": cu(d["PAN"])}
    torch.manual_seed(9)
    got = sample_tiled(diff, scene, "GF2", tile=64, method="dpmsolver", steps=3, max_batch=3)
    tiles = {"MS": split_tiles(scene["MS"], 64, 64), "PAN": split_tiles(scene["PAN"], 64, 64)}
    tiles["Res"] = torch.zeros_like(tiles["MS"])
    torch.manual_seed(9)
    outs = [diff.sample({k: v[lo:lo + 3].contiguous() for k, v in tiles.items()}, "GF2", method="dpmsolver", steps=3)
            for lo in range(0, 4, 3)]
    assert torch.equal(got, merge_tiles(torch.cat(outs), 2, 2))


def test_fused_mode_refuses_more_than_one_rank(tiny, monkeypatch):
    from tmdiff_amd import tiling
    from tmdiff_amd.diffusion_general import GeneralDiffusion
    diff = GeneralDiffusion(tiny[1], "l1").cuda()
    monkeypatch.setattr(tiling.tdist.dist, "is_initialized", lambda: True)
    monkeypatch.setattr(tiling.tdist.dist, "get_world_size", lambda *a: 2)
    scene = {"MS": torch.zeros(1, 4, 64, 64).cuda(), "PAN": torch.zeros(1, 1, 64, 64).cuda()}
    with pytest.raises(ValueError, match="independent"):
        tiling.sample_tiled(diff, scene, "GF2", tile=32, overlap=8)


# ---- 5. degenerate plan ------------------------------------------------------------------------------------------------
def test_scene_of_one_tile_is_the_network_itself(tiny):
    from tmdiff_amd.tiling import TiledDenoiser
    _, net = tiny
    d, dc = _scene(5106, 2, 8, 32, 32)
    t = torch.tensor([[400], [9]]).cuda()
    want = net(dc["x_t"], t, dc["PAN"], dc["MS"], "WV3")
    got = TiledDenoiser(net, 32, 16)(dc["x_t"], t, dc["PAN"], dc["MS"], "WV3")
    assert float((got - want).abs().max()) <= BLEND_TOL * float(want.abs().max())
