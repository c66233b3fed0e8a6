"""MTF-matched filtering and decimation on the GPU (csrc/mtf.hip: ``ops.fir_decimate``, ``ops.mtf_degrade``) and
``data.wald_pair`` / ``LRHRDataset(reduce=...)`` on top of it.

Inputs (tests/test_mtf_host.py): 2 x 3 planes at (1, 1), (3, 5) -- below the filter radius, coordinates clamp many times --,
(64, 64) -- exactly one 16 x 16 output tile per axis at x4 --, (67, 131) -- tile remainders on both axes, extents that are no
multiples of the ratio --, (40, 24); a tap table per band (period 3) and one for all (period 1); K in {1, 3, 7, 41} (41 is the
unrolled instantiation of the kernel, the others the run-time one); ratio 1, 2, 4 with every offset pair on the diagonal and one
off it.

Exact arithmetic catches indexing errors: integer taps in [-3, 3] and integer images in [-8, 8] keep every product and partial
sum below 2^24 (at most 1681 * 24), so the device must equal the float64 definition bit for bit.  The tolerance test cannot do
that: the far taps of an MTF kernel are below 1e-8.

Tolerance against ``metrics.fir_decimate`` with asymmetric randn taps and randn images, elementwise in units of u S, u = 2^-24,
S = |taps| correlated with |x|: a float32 restatement of the kernel's summation order on the CPU (``fir_float32``) measured at
most 0.998 (K = 1), 3.668 (K = 3), 4.660 (K = 7), 5.088 (K = 41) and, for the real MTF kernels with their float64 taps rounded to
float32, 45.556 u S.  The device is held to 4 x that, rounded up -- 19, 21 and 183 u S -- and never to more than the a-priori
bound (K^2 + 1) u / (1 - (K^2 + 1) u) S, which any summation order meets: 2 u S at K = 1, 10 u S at K = 3.

Everything else is bit for bit: ``out=`` (aligned or not: the kernel has one store path), the ratio-4 result against the
ratio-1 result sliced (the same pixel made by another grid), a batch against its planes one at a time, a graph replay against
the eager call, and in ``wald_pair`` the samples ``MS[..., 2::4, 2::4] == LR`` and ``Res == HR - MS``."""
import numpy as np
import pytest
import torch

from test_mtf_host import (MTF_GPU_SHAPES, MTF_KS, MTF_OFFSETS, MTF_PERIODS, MTF_REAL_CASES, U, apriori_u, gpu_tol_u, mtf_input,
                           mtf_real_input, mtf_taps)

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _inference_mode():
    with torch.no_grad():
        yield


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _off_by_one(shape):
    """A contiguous float32 view of ``shape`` whose first element sits 4 bytes past a 16-byte boundary."""
    buf = torch.full((int(np.prod(shape)) + 1,), float("nan"), device="cuda")
    view = buf[1:].view(shape)
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4
    return view


def _combos():
    return [(ratio, off) for ratio, offsets in MTF_OFFSETS.items() for off in offsets]


@pytest.mark.parametrize("k", MTF_KS)
@pytest.mark.parametrize("h,w", MTF_GPU_SHAPES)
def test_fir_decimate_exact_arithmetic(h, w, k):
    from tmdiff_amd import metrics, ops
    x = mtf_input(h, w, integer=True)
    xd = x.cuda()
    for t in MTF_PERIODS:
        taps = mtf_taps(t, k, integer=True)
        td = taps.cuda()
        # a pixel of the definition does not depend on the ratio: every (ratio, offset) is a slice of the ratio-1 result
        full = metrics.fir_decimate(x, taps)
        assert np.abs(full).max() < 2 ** 24
        assert np.array_equal(metrics.fir_decimate(x, taps, 4, (1, 3)), full[..., 1::4, 3::4])
        for ratio, (oy, ox) in _combos():
            got = ops.fir_decimate(xd, td, ratio, (oy, ox))
            want = full[..., oy::ratio, ox::ratio]
            assert got.dtype == torch.float32 and tuple(got.shape) == want.shape == (2, 3, *ops.fir_decimate_shape(h, w, ratio, (oy, ox)))
            bad = int((got.cpu().double().numpy() != want).sum())
            assert bad == 0, f"{h} x {w} K={k} period {t} ratio {ratio} offset ({oy}, {ox}): {bad} of {want.size} pixels differ"


@pytest.mark.parametrize("k", MTF_KS)
@pytest.mark.parametrize("h,w", MTF_GPU_SHAPES)
def test_fir_decimate_against_the_definition(h, w, k):
    from tmdiff_amd import metrics, ops
    x = mtf_input(h, w)
    xd = x.cuda()
    tol = gpu_tol_u(k)
    assert tol <= apriori_u(k)
    worst = 0.0
    for t in MTF_PERIODS:
        taps = mtf_taps(t, k)
        td = taps.cuda()
        full = metrics.fir_decimate(x, taps)
        scale = metrics.fir_decimate(x.abs(), taps.abs())
        assert scale.min() > 0.0
        for ratio, (oy, ox) in _combos():
            got = ops.fir_decimate(xd, td, ratio, (oy, ox)).cpu().double().numpy()
            assert got.shape == full[..., oy::ratio, ox::ratio].shape
            if got.size == 0:                  # no sample at o + ratio * i inside the image
                continue
            err = float((np.abs(got - full[..., oy::ratio, ox::ratio]) / (U * scale[..., oy::ratio, ox::ratio])).max())
            worst = max(worst, err)
            assert err <= tol, f"{h} x {w} K={k} period {t} ratio {ratio} offset ({oy}, {ox}): {err:.3f} u S, tolerance {tol}"
    print(f"fir_decimate {h} x {w} K={k}: worst error {worst:.3f} u S (tolerance {tol:.3f}, a-priori {apriori_u(k):.3f})")


@pytest.mark.parametrize("name,sensor,ratio,pan,shape", MTF_REAL_CASES, ids=[c[0] for c in MTF_REAL_CASES])
def test_mtf_degrade_against_the_definition(name, sensor, ratio, pan, shape):
    from tmdiff_amd import metrics, ops
    x = mtf_real_input(shape)
    got = ops.mtf_degrade(x.cuda(), sensor, ratio, pan=pan)
    want = metrics.mtf_degrade(x, sensor, ratio, pan)
    taps = np.stack([metrics.mtf_kernel(g, ratio) for g in metrics.band_gains(sensor, shape[1], pan)])
    scale = metrics.fir_decimate(x.abs(), np.abs(taps), ratio)
    assert tuple(got.shape) == want.shape == (*shape[:2], *ops.fir_decimate_shape(shape[2], shape[3], ratio, None))
    err = float((np.abs(got.cpu().double().numpy() - want) / (U * scale)).max())
    tol = gpu_tol_u("mtf")
    print(f"mtf_degrade {name} x{ratio} {shape}: {err:.3f} u S (tolerance {tol}, a-priori {apriori_u(41):.1f})")
    assert tol <= apriori_u(41) and err <= tol
    # the table is uploaded once per (gains, ratio, device)
    cached = dict(ops._MTF_TAPS)
    assert _same(ops.mtf_degrade(x.cuda(), sensor, ratio, pan=pan), got) and set(ops._MTF_TAPS) == set(cached)
    assert all(ops._MTF_TAPS[key] is cached[key] for key in cached)
    # ... and is what fir_decimate takes
    gains = metrics.band_gains(sensor, shape[1], pan)
    assert _same(ops.fir_decimate(x.cuda(), ops._MTF_TAPS[(gains, ratio, torch.device("cuda", torch.cuda.current_device()))], ratio), got)


@pytest.mark.parametrize("k", (7, 41))
@pytest.mark.parametrize("h,w", [(67, 131), (3, 5), (64, 64)])
def test_fir_decimate_bitwise_properties(h, w, k):
    from tmdiff_amd import ops
    xd, td = mtf_input(h, w).cuda(), mtf_taps(3, k).cuda()
    full = ops.fir_decimate(xd, td)
    for ratio, (oy, ox) in _combos():
        got = ops.fir_decimate(xd, td, ratio, (oy, ox))
        # the same pixel made by another grid, tile and patch
        assert _same(got, full[..., oy::ratio, ox::ratio])
        # out=: the same object, the same bits; one element off 16-byte alignment too
        out = torch.full_like(got, float("nan"))
        assert ops.fir_decimate(xd, td, ratio, (oy, ox), out=out) is out and _same(out, got)
        if got.numel():
            off = _off_by_one(got.shape)
            assert ops.fir_decimate(xd, td, ratio, (oy, ox), out=off) is off and _same(off, got)
    # the default offset is where upsample_poly23 puts the samples
    assert _same(ops.fir_decimate(xd, td, 4), full[..., 2::4, 2::4]) and _same(ops.fir_decimate(xd, td, 2), full[..., 1::2, 1::2])
    # a batch is its planes one at a time (plane p takes taps[p % 3])
    got = ops.fir_decimate(xd, td, 4)
    for b in range(2):
        for c in range(3):
            assert _same(ops.fir_decimate(xd[b:b + 1, c:c + 1].contiguous(), td[c].contiguous(), 4), got[b:b + 1, c:c + 1])


def test_fir_decimate_limits():
    from tmdiff_amd import ops
    x, taps = torch.zeros(1, 3, 8, 8, device="cuda"), torch.zeros(3, 3, 3, device="cuda")
    for bad in (dict(ratio=3), dict(offset=4, ratio=4), dict(offset=(0, -1)), dict(out=torch.empty(1, 3, 8, 4, device="cuda")),
                dict(taps=torch.zeros(2, 3, 3, device="cuda")), dict(taps=torch.zeros(3, 4, 4, device="cuda")),
                dict(taps=torch.zeros(3, 43, 43, device="cuda")), dict(taps=taps.cpu()), dict(taps=taps.double()),
                dict(x=x.double()), dict(x=x[..., ::2])):
        with pytest.raises(ValueError):
            ops.fir_decimate(**{**dict(x=x, taps=taps), **bad})
    with pytest.raises(ValueError):
        ops.mtf_degrade(x, "QB")                                            # 4 gains, 3 bands
    assert ops.fir_decimate(torch.zeros(0, 3, 8, 8, device="cuda"), taps, 4).shape == (0, 3, 2, 2)
    c = ops.mtf_degrade(torch.full((1, 4, 67, 131), 3.25, device="cuda"), "QB")
    assert float((c / 3.25 - 1.0).abs().max()) <= gpu_tol_u("mtf") * U


def test_fir_decimate_captures_into_a_graph():
    """With out= nothing is allocated or synchronised."""
    from tmdiff_amd import ops
    xd, td = mtf_input(67, 131).cuda(), mtf_taps(3, 41).cuda()
    want = ops.fir_decimate(xd, td, 4)
    src, out = torch.zeros_like(xd), torch.zeros_like(want)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        ops.fir_decimate(src, td, 4, out=out)               # warm-up on the capture stream
    stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        ops.fir_decimate(src, td, 4, out=out)
    src.copy_(xd)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert _same(out, want)


def test_wald_pair_on_the_device():
    from tmdiff_amd import metrics, ops
    from tmdiff_amd.data import wald_pair
    g = torch.Generator().manual_seed(64)
    ms, pan = torch.rand(2, 4, 64, 64, generator=g), torch.rand(2, 1, 256, 256, generator=g)
    got = wald_pair(ms.cuda(), pan.cuda(), "QB")
    want = wald_pair(ms, pan, "QB")
    assert set(got) == set(want) == {"LR", "PAN", "MS", "HR", "Res"}
    for key in got:
        assert got[key].is_cuda and got[key].dtype == torch.float32 and got[key].shape == want[key].shape, key
    assert _same(got["HR"], ms.cuda())
    tol = gpu_tol_u("mtf")
    ms_gains, pan_gain = metrics.mtf_gains("QB", 4)
    for key, x, gains in (("LR", ms, ms_gains), ("PAN", pan, (pan_gain,))):
        scale = metrics.fir_decimate(x, np.abs(np.stack([metrics.mtf_kernel(gn, 4) for gn in gains])), 4)
        err = float((np.abs(got[key].cpu().double().numpy() - want[key].numpy()) / (U * scale)).max())
        print(f"wald_pair {key}: {err:.3f} u S (tolerance {tol})")
        assert err <= tol
    # MS: the interpolator (held to 9 eps m by tests/test_gpu_poly23.py) on an LR that is itself within tol u S; its L1 gain per
    # pass is 1.6236, four passes at x4
    lr_err = float((got["LR"].cpu().double() - want["LR"]).abs().max())
    bound = 1.6236 ** 4 * lr_err + 9 * U * float(want["LR"].abs().max())
    for key in ("MS", "Res"):
        assert float((got[key].cpu().double() - want[key]).abs().max()) <= bound + (U if key == "Res" else 0.0), key
    assert _same(got["MS"][..., 2::4, 2::4], got["LR"])
    assert _same(got["MS"], ops.upsample_poly23(got["LR"], 4)) and _same(got["Res"], got["HR"] - got["MS"])


def test_finetune_step_on_a_reduced_raw_scene():
    """One optimizer step of the finetune driver's model on items of LRHRDataset(reduce="QB"), as
    tests/test_gpu_training.py::test_finetune_driver_end_to_end does with npz sets."""
    from tmdiff_amd.data import create_dataloader, create_dataset
    from tmdiff_amd.model import DDPM
    g = np.random.default_rng(3)
    raw = {"ms": g.integers(0, 2047, (4, 4, 64, 64)), "pan": g.integers(0, 2047, (4, 1, 256, 256))}
    ds_opt = dict(dataroot=raw, data_len=-1, batch_size=2, num_workers=0, use_shuffle=True, reduce="QB")
    ds = create_dataset(ds_opt, "train")
    assert ds.has_gt is True and len(ds) == 4 and tuple(ds[0]["LR"].shape) == (4, 16, 16) and tuple(ds[0]["HR"].shape) == (4, 64, 64)
    loader = create_dataloader(ds, ds_opt, "train", generator=torch.Generator().manual_seed(0))
    batch = next(iter(loader))
    assert {k: tuple(v.shape) for k, v in batch.items()} == {"LR": (2, 4, 16, 16), "PAN": (2, 1, 64, 64), "MS": (2, 4, 64, 64),
                                                             "HR": (2, 4, 64, 64), "Res": (2, 4, 64, 64)}
    opt = {"phase": "train", "gpu_ids": [0], "distributed": False, "path": {"resume": None, "checkpoint": None},
           "model": {"unet": {"channel_multiplier": [8, 16, 32, 64]}, "diffusion": {"loss_type": "l1"}, "init_type": "orthogonal"},
           "train": {"optimizer": {"lr": 1e-4}, "max_iter": 4}}
    torch.manual_seed(3407)
    with torch.enable_grad():
        model = DDPM(opt)
        model.set_new_noise_schedule({"schedule": "cosine", "n_timestep": 1000}, "train")
        model.feed_data(batch)
        model.optimize_parameters("QB")
        torch.cuda.synchronize()
        loss = float(model.get_current_log()["l_pix"])
    print(f"finetune step on a reduced raw scene: l_pix {loss:.4f}")
    assert np.isfinite(loss) and loss > 0.0
