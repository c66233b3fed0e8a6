"""HQNR on the device: the block-wise D_s (metrics_dsblock_kernel, csrc/metrics.hip), ``ops.pan_lowpass``, ``ops.metrics_hqnr`` and
their users, against the float64 host definitions of tmdiff_amd/metrics.py (d_s_block, q2n, hqnr), never against the device.

Tolerance: 1e-9 * max(1, |want|), the bound tests/test_gpu_q2n.py derives: both sides work in fp64 on the same fp32 values and
take sums of at most 1024 exact products, which differ by their order alone (about 1e-13 at the most).  For ``metrics_hqnr`` the
host is evaluated on the device's own filtered image and low-pass PAN, read back from the buffers: those intermediates are fp32
and are held to their own bounds by tests/test_gpu_mtf.py and tests/test_gpu_poly23.py; the distance to the all-float64 chain
``metrics.hqnr`` is printed, not asserted."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-9


def _uniform(seed, b, c, h, w):
    """(ps, ms_exp, pan, pan_lp) in [0, 1], the bands correlated with their PAN as real bands are."""
    g = torch.Generator().manual_seed(seed)
    pan, pan_lp = torch.rand(b, 1, h, w, generator=g), torch.rand(b, 1, h, w, generator=g)
    ps = 0.5 * torch.rand(b, c, h, w, generator=g) + 0.5 * pan
    ms = 0.6 * torch.rand(b, c, h, w, generator=g) + 0.4 * pan_lp
    return ps, ms, pan, pan_lp


def _sensor(seed, b, c, h, w):
    """Sensor scale: mean 1000, sigma 5, the PAN the band mean plus noise.  A raw second moment is 4e4 times the variance here."""
    g = torch.Generator().manual_seed(seed)
    ps, ms = (1000.0 + 5.0 * torch.randn(b, c, h, w, generator=g) for _ in range(2))
    pan = ps.mean(1, keepdim=True) + 2.0 * torch.randn(b, 1, h, w, generator=g)
    pan_lp = ms.mean(1, keepdim=True) + 2.0 * torch.randn(b, 1, h, w, generator=g)
    return ps, ms, pan, pan_lp


def _host(ps, ms, pan, pan_lp, block, q):
    """(D_s [B], maps [B, C, 2, ny, nx]) of the host definition."""
    from tmdiff_amd import metrics as M
    vals, maps = [], []
    for i in range(ps.shape[0]):
        v, hi, lo = M.d_s_block(ps[i].numpy(), ms[i].numpy(), pan[i].numpy(), pan_lp[i].numpy(), block, q, return_maps=True)
        vals.append(v)
        maps.append(np.stack([hi, lo], 1))
    return np.array(vals), np.stack(maps)


def _close(got, want):
    with np.errstate(invalid="ignore"):
        return np.abs(got - want) <= TOL * np.maximum(1.0, np.abs(want))


def _check(tensors, block, q, what, dev=None):
    from tmdiff_amd import ops
    ps, ms, pan, pan_lp = tensors
    want, want_maps = _host(ps, ms, pan, pan_lp, block, q)
    b, c, h, w = ps.shape
    dps, dms, dpan, dlp = dev if dev is not None else (t.cuda() for t in tensors)
    maps = torch.full((b, c, 2, *ops.q2n_grid(h, w, block, block)), float("nan"), device="cuda", dtype=torch.float64)
    got = ops.metrics_dsblock(dps, dms, dpan, dlp, block, q, maps_out=maps)
    assert got.shape == (b,) and got.dtype == torch.float64 and got.is_cuda
    got, got_maps = got.cpu().numpy(), maps.cpu().numpy()
    assert got_maps.shape == want_maps.shape, what
    print(f"{what}: device {got.tolist()} host {want.tolist()} |diff| {np.abs(got - want).max():.2e}; "
          f"worst window |diff| {np.abs(got_maps - want_maps).max():.2e}")
    assert np.isfinite(want).all() and np.isfinite(want_maps).all(), what
    assert _close(got, want).all(), (what, got, want)
    assert _close(got_maps, want_maps).all(), (what, np.argwhere(~_close(got_maps, want_maps)))
    return got, got_maps


SHAPES = {"b2_c4_64x96": (2, 4, 64, 96, 32),               # exact grid, 2 x 3 windows
          "c8_40x72": (1, 8, 40, 72, 32),                  # 24 mirrored rows and columns
          "c1_32x32": (1, 1, 32, 32, 32),                  # one band, one window
          "b3_c5_16x24_8": (3, 5, 16, 24, 8),              # 64 pixels per window: one wave of the four holds them
          "c16_48x48_16": (1, 16, 48, 48, 16)}             # the most bands; 256 pixels per window


@pytest.mark.parametrize("q", [1, 2])
@pytest.mark.parametrize("data", ["uniform", "sensor"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_dsblock(name, data, q):
    b, c, h, w, block = SHAPES[name]
    tensors = (_uniform if data == "uniform" else _sensor)(31, b, c, h, w)
    got, _ = _check(tensors, block, q, f"{name} {data} q={q}")
    assert (got > 0.0).all() and (got < 1.0).all()


def test_strided_inputs_are_scored_in_place():
    """ps and ms_exp as channel slices of wider tensors and as every other batch item; pan and pan_lp as every other item."""
    wide = [t for t in _sensor(32, 4, 6, 40, 72)]
    dev = [t.cuda() for t in wide]
    pick = lambda t: (t[::2, 1:5], t[::2])
    tensors = (pick(wide[0])[0], pick(wide[1])[0], pick(wide[2])[1], pick(wide[3])[1])
    views = (pick(dev[0])[0], pick(dev[1])[0], pick(dev[2])[1], pick(dev[3])[1])
    assert not views[0].is_contiguous() and views[0].stride(0) == 2 * 6 * 40 * 72 and views[2].stride(0) == 2 * 40 * 72
    _check(tensors, 32, 1, "strided", dev=views)
    from tmdiff_amd import ops
    dense = ops.metrics_dsblock(*(v.contiguous() for v in views))
    assert torch.equal(ops.metrics_dsblock(*views).view(torch.int64), dense.view(torch.int64))
    with pytest.raises(ValueError):
        ops.metrics_dsblock(dev[0][..., ::2], dev[1][..., ::2], dev[2][..., ::2], dev[3][..., ::2])   # rows must be dense


def test_reproducible_and_capturable():
    """Two calls agree bit for bit; a call captured on one stream and replayed three times equals the eager call; out=, maps_out=
    and workspace= are the tensors written."""
    from tmdiff_amd import ops
    ps, ms, pan, lp = (t.cuda() for t in _sensor(33, 2, 8, 40, 72))
    same = lambda a, b: torch.equal(a.view(torch.int64), b.view(torch.int64))
    maps1, maps2 = (torch.zeros(2, 8, 2, 2, 3, device="cuda", dtype=torch.float64) for _ in range(2))
    first, second = ops.metrics_dsblock(ps, ms, pan, lp, maps_out=maps1), ops.metrics_dsblock(ps, ms, pan, lp, maps_out=maps2)
    assert same(first, second) and same(maps1, maps2)
    ws = ops.metrics_dsblock_workspace(*ps.shape, ps.device)
    assert ws.numel() == 2 * 8 * 2 * 6
    ws.fill_(-1.0)
    out, maps = torch.full((2, 2), -7.0, device="cuda", dtype=torch.float64), torch.zeros_like(maps1)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        got = ops.metrics_dsblock(ps, ms, pan, lp, out=out, maps_out=maps, workspace=ws)       # warm-up on the capture stream
    stream.synchronize()
    assert got.data_ptr() == out.data_ptr() and same(out[:, 0], first) and same(maps, maps1)
    assert (out[:, 1] == -7.0).all()                                         # no D_lambda given: the second column is left alone
    assert same(ws.view(2, 8, 2, 2, 3), maps1)                                 # the lent workspace is the one used
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        ops.metrics_dsblock(ps, ms, pan, lp, out=out, maps_out=maps, workspace=ws)
    for _ in range(3):
        out.zero_()
        maps.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert same(out[:, 0], first) and same(maps, maps1)
    with pytest.raises(ValueError, match="workspace"):
        ops.metrics_dsblock(ps, ms, pan, lp, workspace=torch.empty(2 * 8 * 2 * 6 - 1, device="cuda", dtype=torch.float64))
    with pytest.raises(ValueError, match="out"):
        ops.metrics_dsblock(ps, ms, pan, lp, out=torch.empty(2, device="cuda", dtype=torch.float64))
    with pytest.raises(ValueError, match="maps_out"):
        ops.metrics_dsblock(ps, ms, pan, lp, maps_out=torch.empty(2, 8, 2, 6, device="cuda", dtype=torch.float64))


def test_constant_window_is_nan_on_both_sides():
    from tmdiff_amd import ops
    ps, ms, pan, lp = _uniform(34, 1, 3, 32, 64)
    ps[0, 1, :, 32:] = 0.25
    pan[0, 0, :, 32:] = 0.5
    want, want_maps = _host(ps, ms, pan, lp, 32, 1)
    maps = torch.zeros(1, 3, 2, 1, 2, device="cuda", dtype=torch.float64)
    got = ops.metrics_dsblock(ps.cuda(), ms.cuda(), pan.cuda(), lp.cuda(), maps_out=maps).cpu().numpy()
    got_maps = maps.cpu().numpy()
    assert np.isnan(want_maps[0, 1, 0, 0, 1]) and np.isnan(want_maps).sum() == 1
    assert np.array_equal(np.isnan(got_maps), np.isnan(want_maps))
    assert _close(got_maps[~np.isnan(want_maps)], want_maps[~np.isnan(want_maps)]).all()
    assert np.isnan(want[0]) and np.isnan(got[0])


def _scene(seed, b, c, h, w, sensor, ratio):
    """(ps, ms_exp, pan) on the host: a PAN, bands mixed from noise and its low-pass version, a fused image between the two."""
    from tmdiff_amd import metrics as M
    g = torch.Generator().manual_seed(seed)
    pan = torch.rand(b, 1, h, w, generator=g)
    low = torch.from_numpy(np.stack([M.pan_lowpass(pan[i].numpy(), sensor, ratio) for i in range(b)])).float()
    ms = 0.6 * torch.rand(b, c, h, w, generator=g) + 0.4 * low
    ps = 0.6 * ms + 0.4 * pan
    return ps, ms, pan


@pytest.mark.parametrize("case", ["qb_128x128", "wv3_b2_96x160", "qb_ratio2"])
def test_metrics_hqnr(case):
    from tmdiff_amd import metrics as M, ops
    b, c, h, w, sensor, ratio, alpha, beta, q = {"qb_128x128": (1, 4, 128, 128, "QB", 4, 1.0, 1.0, 1.0),
                                                  "wv3_b2_96x160": (2, 8, 96, 160, "WV3", 4, 2.0, 0.5, 2.0),
                                                  "qb_ratio2": (1, 4, 64, 64, "QB", 2, 1.0, 1.0, 1.0)}[case]
    ps, ms, pan = _scene(35, b, c, h, w, sensor, ratio)
    buf = ops.metrics_hqnr_buffers(b, c, h, w, "cuda", ratio, 32)
    got = ops.metrics_hqnr(ps.cuda(), ms.cuda(), pan.cuda(), sensor, ratio, 32, alpha, beta, q, buffers=buf)
    assert got.shape == (b, 3) and got.dtype == torch.float64 and got.is_cuda
    got = got.cpu().numpy()
    filtered, pan_lp = buf["filtered"].cpu().numpy(), buf["pan_lp"].cpu().numpy()
    assert filtered.shape == (b, c, h, w) and pan_lp.shape == (b, 1, h, w)
    for i in range(b):
        dl = 1.0 - M.q2n(ms[i].numpy(), filtered[i], 32, 32, hwc=False)
        ds = M.d_s_block(ps[i].numpy(), ms[i].numpy(), pan[i].numpy(), pan_lp[i], 32, q)
        want = np.array([dl, ds, (1.0 - dl) ** alpha * (1.0 - ds) ** beta])
        full = M.hqnr(ps[i].numpy(), ms[i].numpy(), pan[i].numpy(), sensor, ratio, 32, alpha, beta, q)
        print(f"{case}[{i}]: device {got[i].tolist()} host on the device's intermediates {want.tolist()} "
              f"|diff| {np.abs(got[i] - want).max():.2e}; all-float64 chain (d_lambda_k, d_s, hqnr) "
              f"{[full[1], full[2], full[0]]} |diff| {np.abs(got[i] - np.array([full[1], full[2], full[0]])).max():.2e}")
        assert (want > 0.0).all() and (want < 1.0).all()
        assert _close(got[i], want).all(), (case, i, got[i], want)
    # with the buffers a second call writes the same numbers into out= (and, with the tap tables cached, allocates nothing)
    out = torch.zeros(b, 3, device="cuda", dtype=torch.float64)
    dps, dms, dpan = ps.cuda(), ms.cuda(), pan.cuda()
    allocations = lambda: torch.cuda.memory_stats()["allocation.all.allocated"]
    before = allocations()
    again = ops.metrics_hqnr(dps, dms, dpan, sensor, ratio, 32, alpha, beta, q, out=out, buffers=buf)
    assert allocations() == before
    assert again.data_ptr() == out.data_ptr() and np.array_equal(out.cpu().numpy(), got)
    fields = M.quality_hqnr(ms.cuda(), pan.cuda(), ps.cuda(), sensor, ratio, 32, alpha, beta, q)
    assert tuple(fields) == M.HQNR_FIELDS
    for k, name in enumerate(M.HQNR_FIELDS):
        assert fields[name].shape == (b,) and np.array_equal(fields[name].cpu().numpy(), got[:, k]), name


def test_metrics_hqnr_identical_pairs_and_capture():
    from tmdiff_amd import ops
    ps, ms, pan = (t.cuda() for t in _scene(36, 1, 4, 64, 64, "QB", 4))
    got = ops.metrics_hqnr(ms, ms, pan, "QB", pan_lp=pan).cpu().numpy()
    assert got[0, 1] == 0.0 and 0.0 < got[0, 0] < 1.0 and got[0, 2] == 1.0 - got[0, 0]
    buf, out = ops.metrics_hqnr_buffers(1, 4, 64, 64, "cuda"), torch.zeros(1, 3, device="cuda", dtype=torch.float64)
    eager = ops.metrics_hqnr(ps, ms, pan, "QB", buffers=buf).clone()           # also uploads the tap tables
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        ops.metrics_hqnr(ps, ms, pan, "QB", out=out, buffers=buf)
    stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        ops.metrics_hqnr(ps, ms, pan, "QB", out=out, buffers=buf)
    for _ in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int64), eager.view(torch.int64))


def test_pan_lowpass():
    """The composition of two operators that have their own bounds: bit for bit the two calls, the samples where the interpolator
    puts them."""
    from tmdiff_amd import ops
    pan = torch.rand(2, 1, 32, 48, generator=torch.Generator().manual_seed(37)).cuda()
    for ratio in (2, 4):
        low = ops.mtf_degrade(pan, "QB", ratio, pan=True)
        got = ops.pan_lowpass(pan, "QB", ratio)
        assert got.shape == pan.shape and torch.equal(got, ops.upsample_poly23(low, ratio))
        assert torch.equal(got[..., ratio // 2::ratio, ratio // 2::ratio], low)
        out, stage = torch.zeros_like(pan), torch.zeros_like(low)
        assert ops.pan_lowpass(pan, 0.15, ratio, out=out, low=stage).data_ptr() == out.data_ptr()
        assert torch.equal(out, got) and torch.equal(stage, low)                 # 0.15 is QB's PAN gain
    for bad, ratio in ((pan[..., :30, :], 4), (pan[..., :46], 4), (pan, 3), (pan.expand(2, 2, 32, 48), 4)):
        with pytest.raises(ValueError):
            ops.pan_lowpass(bad.contiguous(), "QB", ratio)


def test_unsupported_shapes():
    """Refused in the wrapper: nothing is launched."""
    from tmdiff_amd import ops
    for c, h, w, block, match in ((17, 32, 32, 32, "C <= 16"), (4, 32, 32, 12, "block 8, 16 or 32"), (4, 8, 8, 32, "mirror")):
        assert not ops.metrics_dsblock_supported(1, c, h, w, block)
        t, p = torch.rand(1, c, h, w, device="cuda"), torch.rand(1, 1, h, w, device="cuda")
        with pytest.raises(ValueError, match=match):
            ops.metrics_dsblock(t, t, p, p, block)
    assert ops.metrics_dsblock_supported(1, 16, 32, 32, 32) and ops.metrics_dsblock_supported(2, 4, 40, 72)
    t, p = torch.rand(1, 4, 32, 32, device="cuda"), torch.rand(1, 1, 32, 32, device="cuda")
    with pytest.raises(ValueError):
        ops.metrics_dsblock(t, t[:, :3], p, p)                                  # shapes differ
    with pytest.raises(ValueError):
        ops.metrics_dsblock(t, t, t, p)                                         # a PAN has one band
    with pytest.raises(ValueError, match="q > 0"):
        ops.metrics_dsblock(t, t, p, p, q=0.0)
    with pytest.raises(ValueError):
        ops.metrics_hqnr(torch.rand(1, 17, 32, 32, device="cuda"), torch.rand(1, 17, 32, 32, device="cuda"), p, "QB")
    with pytest.raises(ValueError):
        ops.metrics_hqnr(t, t, p, "WV3")                                        # eight gains for four bands
    with pytest.raises(ValueError):
        ops.metrics_hqnr(t[..., :30, :].contiguous(), t[..., :30, :].contiguous(), p[..., :30, :].contiguous(), "QB")
    with pytest.raises(ValueError, match="buffers"):
        ops.metrics_hqnr(t, t, p, "QB", buffers=ops.metrics_hqnr_buffers(1, 4, 64, 64, "cuda"))


def test_val_dataset_hqnr(tmp_path):
    from tmdiff_amd import evaluate, ops

    class Trainer:
        def feed_data(self, d):
            self.d = d

        def test(self, continous=False, prompt="QB"):
            fused = (0.6 * self.d["MS"] + 0.4 * self.d["PAN"]).clamp(0, 1)
            self.SR = torch.cat([torch.zeros_like(fused), fused])              # a stack; the last image is the result

        def get_current_visuals(self):
            return {"SR": self.SR, **{k: self.d[k] for k in self.keys}}

        keys = ("MS", "PAN", "LR")

    loader = []
    for seed in (38, 39):
        _, ms, pan = _scene(seed, 1, 4, 64, 64, "QB", 4)
        loader.append({"MS": ms.cuda(), "PAN": pan.cuda(), "LR": ms[..., 2::4, 2::4].contiguous().cuda()})
    kw = dict(log=lambda *a: None, full_resolution=True)
    before = evaluate.val_dataset(Trainer(), "QB", loader, str(tmp_path / "before"), **kw)
    got = evaluate.val_dataset(Trainer(), "QB", loader, str(tmp_path / "hqnr"), protocol="hqnr", sensor="QB", **kw)
    named = evaluate.val_dataset(Trainer(), "QB", loader, str(tmp_path / "named"), protocol="hqnr", **kw)     # QB has a row
    after = evaluate.val_dataset(Trainer(), "QB", loader, str(tmp_path / "after"), **kw)
    qnr = evaluate.val_dataset(Trainer(), "QB", loader, str(tmp_path / "qnr"), protocol="qnr", **kw)
    today = {"d_lambda_QB", "d_s_QB", "qnr_QB", "sec_per_item"}
    assert set(before) == set(after) == set(qnr) == today
    for k in today - {"sec_per_item"}:
        assert before[k] == after[k] == qnr[k], k
    assert set(got) == {"d_lambda_k_QB", "d_s_QB", "hqnr_QB", "sec_per_item"} == set(named)
    rows = []
    for d in loader:
        trainer = Trainer()
        trainer.feed_data(d)
        trainer.test()
        rows.append(ops.metrics_hqnr(evaluate._to_nchw01(trainer.SR[-1]), d["MS"], d["PAN"], "QB")[0].cpu().numpy())
    want = np.mean(rows, 0)
    for k, name in enumerate(("d_lambda_k_QB", "d_s_QB", "hqnr_QB")):
        print(f"{name}: val_dataset {got[name]!r} mean of the items {want[k]!r}")
        assert 0.0 < want[k] < 1.0 and abs(got[name] - want[k]) <= TOL and named[name] == got[name]
    for folder in ("hqnr", "before"):
        for idx in (0, 1):
            assert os.path.exists(os.path.join(str(tmp_path / folder), "QB", f"output_mulExm_{idx}.mat"))
    no_ms = Trainer()
    no_ms.keys = ("PAN", "LR")
    with pytest.raises(ValueError, match="MS"):
        evaluate.val_dataset(no_ms, "QB", loader, str(tmp_path / "no_ms"), protocol="hqnr", **kw)


def test_fuse_scene_hqnr():
    """The set-up of tests/test_gpu_resample.py::test_fuse_scene: the tiny network, 8 bands, 32 x 48, tile 32, overlap 16."""
    from oracle import unet_ref as U
    from oracle.make_golden import TINY
    from tmdiff_amd import metrics as M, ops
    from tmdiff_amd.Hyper_unet_general import WavBEST
    from tmdiff_amd.diffusion_general import GeneralDiffusion
    from tmdiff_amd.tiling import fuse_scene
    ref = U.fill_weights_(U.WavBESTRef(channels=TINY)).eval()
    net = WavBEST(channels=TINY)
    net.load_state_dict(ref.state_dict())
    net = net.cuda().eval()
    diff = GeneralDiffusion(net, "l1", noise_fn=lambda like: torch.randn(like.shape, dtype=torch.float32)).cuda()
    diff.set_new_noise_schedule({"schedule": "cosine", "n_timestep": 1000}, "cuda")
    g = torch.Generator().manual_seed(70)
    lr_ms, pan = torch.rand(1, 8, 8, 12, generator=g).cuda(), torch.rand(1, 1, 32, 48, generator=g).cuda()
    kw = dict(tile=32, method="dpmsolver", steps=3, overlap=16)
    ms_exp = ops.upsample_poly23(lr_ms, 4)
    for interp in ("poly23", "bilinear"):
        torch.manual_seed(11)
        plain = fuse_scene(diff, lr_ms, pan, "WV3", interp=interp, **kw)
        torch.manual_seed(11)
        scene, scores = fuse_scene(diff, lr_ms, pan, "WV3", interp=interp, score="hqnr", sensor="WV3", **kw)
        assert torch.equal(scene, plain) and tuple(scores) == M.HQNR_FIELDS
        again = M.quality_hqnr(ms_exp, pan, scene.float().contiguous(), "WV3")
        for k in M.HQNR_FIELDS:
            assert scores[k].shape == (1,) and torch.equal(scores[k].view(torch.int64), again[k].view(torch.int64)), k
    with pytest.raises(ValueError, match="sensor"):
        fuse_scene(diff, lr_ms, pan, "WV3", score="hqnr", **kw)
    with pytest.raises(ValueError, match="score"):
        fuse_scene(diff, lr_ms, pan, "WV3", score="khan", sensor="WV3", **kw)
