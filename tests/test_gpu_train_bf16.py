"""The finetune step with ops.config.grad_bf16 (bf16 gradient arithmetic of the 3x3x3 convolutions; forward, loss, parameters and
AdamW stay fp32) on the narrowest network whose every body convolution is eligible: WavBEST(channels [32, 32, 32, 32]), 4 bands,
16x16, B = 2, dropout on with a fixed seed, wino_min_blocks=1 (the production families on a small batch)."""
import collections

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CH, B, BANDS, SIZE = [32, 32, 32, 32], 2, 4, 16
SEEDS = (0, 1, 2)
# profiles/train_bf16_grad.txt (tools/bench_train_bf16.py --agreement, MI355X): the largest per-tensor relative L2 difference
# between the bf16- and the fp32-arithmetic gradients over the three seeds.  The bound is four times that: the margin is for the
# seed-to-seed spread of rounding noise through up to 50 layers.
TABLE_MAX = 6.509e-3
REL_L2_BOUND = 4.0 * TABLE_MAX


def _step(seed, bf16, counts=None):
    """(loss, {name: gradient}) of one forward + backward; everything that is random is seeded (the dropout seeds come from the
    host generator)."""
    from tmdiff_amd import ops
    from tmdiff_amd.Hyper_unet_general import WavBEST
    from tmdiff_amd.diffusion_general import GeneralDiffusion
    from tmdiff_amd.util import fill_weights_, synthetic_tile_batch
    net = fill_weights_(WavBEST(channels=CH), seed=seed).cuda().train()
    diff = GeneralDiffusion(net, "l1").cuda()
    diff.set_loss("cuda")
    diff.set_new_noise_schedule({"schedule": "cosine", "n_timestep": 1000}, "cuda")
    d = synthetic_tile_batch(5000 + seed, B, BANDS, SIZE, device=torch.device("cuda"))
    t = np.random.RandomState(seed).randint(1, 1001, size=B)
    t_dev = torch.from_numpy(t).view(B, 1).cuda()
    a_dev = torch.tensor(diff.sqrt_alphas_cumprod_prev[t], dtype=torch.float32).cuda()
    noise = torch.randn(B, BANDS, SIZE, SIZE, generator=torch.Generator().manual_seed(seed)).cuda()
    torch.manual_seed(seed)
    keep = ops.COUNTS
    try:
        ops.COUNTS = counts
        with ops.config.override(wino_min_blocks=1, grad_bf16=bf16):
            loss = diff.p_losses_with(d, "WV3", t_dev, a_dev, noise).sum()
            loss.backward()
    finally:
        ops.COUNTS = keep
    return float(loss), {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in net.named_parameters()}


@pytest.fixture(scope="module")
def runs():
    """{seed: (fp32 result, bf16 result, launch counts of the bf16 step)}, computed once"""
    assert torch.cuda.is_available(), "these tests need the MI355X"
    out = {}
    for s in SEEDS:
        counts = collections.Counter()
        out[s] = (_step(s, False), _step(s, True, counts), counts)
    return out


def test_loss_is_bit_identical_and_the_same_parameters_get_gradients(runs):
    for s, ((l32, g32), (l16, g16), _) in runs.items():
        assert l32 == l16, (s, l32, l16)            # the forward is untouched (and drew the same dropout masks)
        assert [k for k, g in g32.items() if g is None] == [k for k, g in g16.items() if g is None]
        assert sum(g is not None for g in g16.values()) > 100 and any(g is None for g in g16.values())
        assert any(not torch.equal(g16[k], g32[k]) for k in g32 if g32[k] is not None), "the switch changed nothing"


def test_plans_are_bf16_for_every_body_convolution(runs):
    """routing's plans for this network: the data gradient of every 3x3x3 convolution is bf16, of the 1x1x1 ones fp32; the weight
    gradients stay on their fp32 families (the bf16 weight-gradient kernel is slower than them in every measured layer class,
    profiles/train_bf16_grad.txt) -- and the step launches exactly what the table says (ops.COUNTS)."""
    from tmdiff_amd import ops, routing
    with ops.config.override(wino_min_blocks=1):
        off = routing.unet_train_launches(CH, B, BANDS, SIZE, SIZE, True)
    with ops.config.override(wino_min_blocks=1, grad_bf16=True):
        table = routing.unet_train_launches(CH, B, BANDS, SIZE, SIZE, True)
        p3 = routing.train_conv_plan(B, (32,), 32, BANDS, SIZE, SIZE, 1, 3, True, False, True, True)
        p1 = routing.train_conv_plan(B, (32,), 32, BANDS, SIZE, SIZE, 1, 1)
    assert (p3.dgrad_math, p3.wgrad_math) == ("bf16", "fp32") and (p1.dgrad_math, p1.wgrad_math) == ("fp32", "fp32")
    n3 = sum(1 for c in table.convs if c.ksize == 3)
    assert n3 >= 50
    for c, c0 in zip(table.convs, off.convs):
        assert c.dgrad == ("bf16" if c.ksize == 3 else "k1") and (c.fwd, c.keep_xp, c.wgrad) == (c0.fwd, c0.keep_xp, c0.wgrad), c
    counts = runs[0][2]
    for key in ("conv3d_fwd_bf16", "conv3d_wgrad_bf16", "conv3d_wgrad", "conv3d_wgrad_wino"):
        assert counts.get(key, 0) == table.counts.get(key, 0), (key, dict(counts), table.counts)
    assert counts["conv3d_fwd_bf16"] == n3 and counts.get("conv3d_wgrad_bf16", 0) == 0
    assert counts["conv3d_pack_weights_bf16_dgrad"] == n3          # one packing launch per weight and step


def test_gradients_agree_with_the_fp32_step(runs):
    """Per parameter tensor the relative L2 difference to the fp32-arithmetic gradient stays within four times the largest value
    measured over three seeds (TABLE_MAX, profiles/train_bf16_grad.txt); independently of that measurement no tensor exceeds 5e-2
    and the cosine between the two full gradient vectors is above 0.999."""
    for s, ((_, g32), (_, g16), _) in runs.items():
        names = [k for k, g in g32.items() if g is not None]
        rows = sorted(((float((g16[k] - g32[k]).norm() / g32[k].norm().clamp_min(1e-30)), k) for k in names), reverse=True)
        a, b = torch.cat([g32[k].reshape(-1) for k in names]).double(), torch.cat([g16[k].reshape(-1) for k in names]).double()
        cos = float((a @ b) / (a.norm() * b.norm()))
        print(f"\nseed {s}: worst relative L2 {rows[0][0]:.3e} ({rows[0][1]}), cosine {cos:.6f}")
        assert rows[0][0] <= REL_L2_BOUND, rows[:3]
        assert rows[0][0] <= 5e-2, rows[:3]
        assert cos > 0.999, cos


def _trainer():
    from tmdiff_amd.model import DDPM
    from tmdiff_amd.util import fill_weights_
    opt = {"phase": "train", "gpu_ids": [0], "distributed": False, "path": {"resume": None},
           "model": {"unet": {"channel_multiplier": list(CH)}, "diffusion": {"loss_type": "l1"}, "init_type": "orthogonal"},
           "train": {"optimizer": {"lr": 1e-2}, "max_iter": 1000, "hip_graph": True, "grad_compute": "bf16"}}
    m = DDPM(opt)
    assert m.grad_compute == "bf16" and m.use_graph
    fill_weights_(m.netG.denoise_fn)
    m.netG.denoise_fn.invalidate_prepared()
    m.set_new_noise_schedule({"schedule": "cosine", "n_timestep": 1000}, "train")
    return m


def test_captured_step_replays_to_the_eager_bits():
    """model.DDPM with train.grad_compute = "bf16" and train.hip_graph: after the two eager warm-up steps, two CapturedStep replays
    (forward, backward, FusedAdamW) leave the same PARAMETER bits as the same two steps run eagerly -- the recorded function itself
    (CapturedStep._step + the optimizer step, one stream as the recording) from the same parameters, AdamW state, learning rates,
    dropout word and seeds, timesteps and noise.  And the recorded step re-makes the bf16 data-gradient packings: after the second
    replay the cached packing of a weight is the packing of that weight as the first replay's AdamW step left it, not of the
    initial weight (FusedAdamW writes through raw pointers; it bumps the parameter versions the caches are keyed on)."""
    from tmdiff_amd import ops
    from tmdiff_amd.util import synthetic_tile_batch
    m = _trainer()
    net = m.netG.denoise_fn
    d = synthetic_tile_batch(5100, B, BANDS, SIZE, device=torch.device("cuda"))
    d["LR"] = d["MS"]
    gen = torch.Generator().manual_seed(9)
    noises = [torch.randn(B, BANDS, SIZE, SIZE, generator=gen) for _ in range(4)]
    order = []
    m.netG.noise_fn = lambda like: order.pop(0)
    w = net.middle1.conv20.weight
    pack0 = ops.pack_conv_weight_bf16_dgrad(w, 1).clone()
    keep_word = ops.DROP_WORD
    try:
        with ops.config.override(wino_min_blocks=1):
            order[:] = noises[:2]
            np.random.seed(1)
            torch.manual_seed(1)
            for _ in range(2):                       # the eager warm-up steps
                m.feed_data(dict(d))
                m.optimize_parameters("WV3")
            cache = net.__dict__["_train_pack_bf16"]
            assert len(cache.items) >= 50 and w.data_ptr() in cache.items
            params = list(m.netG.parameters())
            lr = m.optG.param_groups[0]["lr"]
            assert torch.is_tensor(lr)
            snap_p = [p.detach().clone() for p in params]
            snap_s = [{k: v.clone() for k, v in m.optG.state[p].items() if torch.is_tensor(v)} if p in m.optG.state else {} for p in params]
            word = ops.DROP_WORD.clone()
            lrs, loss_g, loss_e, w_before = [], [], [], []
            order[:] = noises[2:]
            np.random.seed(2)
            for _ in range(2):                       # capture + replay, replay
                lrs.append(lr.clone())
                w_before.append(w.detach().clone())
                torch.manual_seed(7)                 # (the dropout seeds are drawn when the step is recorded)
                m.feed_data(dict(d))
                m.optimize_parameters("WV3")
                loss_g.append(float(next(iter(m._captured.values())).loss))
            step = next(iter(m._captured.values()))
            assert len(m._captured) == 1 and step.replays == 2
            torch.cuda.synchronize()
            got = [p.detach().clone() for p in params]
            assert not torch.equal(w_before[0], w_before[1]) and not torch.equal(w_before[1], w), "AdamW moved nothing"
            cached = cache.items[w.data_ptr()][2]
            assert torch.equal(cached, ops.pack_conv_weight_bf16_dgrad(w_before[1], 1)), "the replay did not re-pack the weight"
            assert not torch.equal(cached, pack0) and not torch.equal(cached, ops.pack_conv_weight_bf16_dgrad(w_before[0], 1))
            # the same two steps eagerly, from the same state
            with torch.no_grad():
                for p, sp, ss in zip(params, snap_p, snap_s):
                    p.copy_(sp)
                    for k, v in ss.items():
                        m.optG.state[p][k].copy_(v)
                ops.DROP_WORD.copy_(word)
            order[:] = noises[2:]
            np.random.seed(2)
            for i in range(2):
                lr.copy_(lrs[i])
                step.load(d)
                m.netG.zero_grad(set_to_none=True)
                torch.manual_seed(7)
                with ops.config.override(train_two_streams=False, grad_bf16=True):
                    loss = step._step()
                    m.optG.step()
                loss_e.append(float(loss.detach()))
            torch.cuda.synchronize()
            off = [k for (k, _), a, p in zip(m.netG.named_parameters(), got, params) if not torch.equal(a, p)]
            print(f"\nreplays {loss_g}, eager {loss_e}, {len(off)} of {len(params)} parameter tensors differ in bits {off[:4]}")
            assert loss_g == loss_e, (loss_g, loss_e)
            assert not off, off[:8]
    finally:
        ops.DROP_WORD = keep_word


def test_bf16_packing_follows_the_eager_optimizer_step():
    """The eager trainer (FusedAdamW, no graph): at every step the bf16 data-gradient packing a layer uses is the packing of the
    weight as the previous optimizer step left it, and so is the fp32 forward packing of ops.PackedWeights."""
    from tmdiff_amd import ops
    from tmdiff_amd.util import synthetic_tile_batch
    m = _trainer()
    m.use_graph = False
    net = m.netG.denoise_fn
    d = synthetic_tile_batch(5101, B, BANDS, SIZE, device=torch.device("cuda"))
    d["LR"] = d["MS"]
    w = net.middle1.conv20.weight
    np.random.seed(3)
    torch.manual_seed(3)
    with ops.config.override(wino_min_blocks=1):
        for it in range(3):
            before = w.detach().clone()
            m.feed_data(dict(d))
            m.optimize_parameters("WV3")
            torch.cuda.synchronize()
            cache, pk = net.__dict__["_train_pack_bf16"], net.__dict__["_train_pack"]
            assert torch.equal(cache.items[w.data_ptr()][2], ops.pack_conv_weight_bf16_dgrad(before, 1)), it
            assert torch.equal(pk.fwd[pk._index[w.data_ptr()]], ops.pack_conv_weight(before, 1, 0)), it
            assert it == 0 or not torch.equal(before, w), "AdamW moved nothing"      # (the warm-up schedule starts at lr = 0)
