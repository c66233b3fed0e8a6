"""Q2n on the device (metrics_q2n_kernel, csrc/metrics.hip) against the float64 host definition metrics.q2n, image by image and
block by block.

Tolerance: 1e-9 * max(1, |want|), that of the other fp64 device metrics (tests/test_gpu_metrics.py).  Both sides work in fp64
on the same fp32 values.  The kernel sums centred products and forms the normalised moments from them, the host normalises every
pixel first: the same numbers up to the rounding of sums of at most 1024 terms, about 1e-13 at the most.  The definition itself is
unpinned (tests/test_q2n_host.py holds it to independent statements)."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-9


def _pair(seed, b, c, h, w, noise=0.05):
    g = torch.Generator().manual_seed(seed)
    t = torch.rand(b, c, h, w, generator=g)
    p = (t + noise * torch.randn(b, c, h, w, generator=g)).clamp(0, 1)
    return t, p


def _host(t, p, block=32, shift=32):
    """(values [B], maps [B, ny, nx]) of the host definition."""
    from tmdiff_amd import metrics as M
    rows = [M.q2n(t[i].numpy(), p[i].numpy(), block, shift, hwc=False, return_map=True) for i in range(t.shape[0])]
    return np.array([r[0] for r in rows]), np.stack([r[1] for r in rows])


def _device(t, p, block=32, shift=32):
    from tmdiff_amd import ops
    b, _, h, w = t.shape
    vals = torch.full((b, *ops.q2n_grid(h, w, block, shift)), float("nan"), device="cuda", dtype=torch.float64)
    got = ops.metrics_q2n(t.cuda(), p.cuda(), block, shift, map_out=vals)
    assert got.shape == (b,) and got.dtype == torch.float64 and got.is_cuda
    return got.cpu().numpy(), vals.cpu().numpy()


def _check(t, p, block=32, shift=32, what=""):
    want, want_map = _host(t, p, block, shift)
    got, got_map = _device(t, p, block, shift)
    assert got_map.shape == want_map.shape, what
    err, err_map = np.abs(got - want), np.abs(got_map - want_map)
    print(f"{what}: device {got.tolist()} host {want.tolist()} |diff| {err.max():.2e}; worst block |diff| {err_map.max():.2e}")
    assert np.isfinite(got).all() and np.isfinite(got_map).all(), what
    assert (err <= TOL * np.maximum(1.0, np.abs(want))).all(), (what, got, want)
    assert (err_map <= TOL * np.maximum(1.0, np.abs(want_map))).all(), (what, np.argwhere(err_map > TOL))
    return got, got_map


SHAPES = {"b2_c8_40x72": (2, 8, 40, 72, 32, 32),            # ragged in both axes
          "c4_64x64": (1, 4, 64, 64, 32, 32),               # exact grid
          "b3_c3_33x32": (3, 3, 33, 32, 32, 32),            # band padding; one row past a block: 31 mirrored rows
          "c16_32x40": (1, 16, 32, 40, 32, 32),             # the largest LDS footprint
          "b2_c1_32x32": (2, 1, 32, 32, 32, 32),            # a single band
          "c6_35x70": (1, 6, 35, 70, 32, 32),               # band padding to 8
          "b2_c8_20x28_8_4": (2, 8, 20, 28, 8, 4),          # overlapping blocks
          "c4_12x20_16": (1, 4, 12, 20, 16, 16),            # an image smaller than one block
          "c2_264x264_8_4": (1, 2, 264, 264, 8, 4)}         # 66 x 66 = 4356 blocks: 18 per lane of the finalize kernel


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes(name):
    from tmdiff_amd import ops
    b, c, h, w, block, shift = SHAPES[name]
    t, p = _pair(21, b, c, h, w)
    got, got_map = _check(t, p, block, shift, name)
    assert got_map.shape[1:] == (math.ceil(h / shift), math.ceil(w / shift)) == ops.q2n_grid(h, w, block, shift)
    assert (got > 0.5).all() and (got < 1.0).all()
    means = got_map.reshape(b, -1).mean(1)
    assert (np.abs(means - got) <= 1e-12).all()


def test_sensor_scale_data():
    t, p = _pair(22, 2, 8, 40, 72)
    _check(t * 2047.0, p * 2047.0, what="sensor scale")


def test_identical_inputs():
    for c, h, w in ((8, 40, 72), (3, 33, 32), (16, 32, 40)):
        t, _ = _pair(23, 1, c, h, w)
        got, got_map = _device(t, t.clone())
        print(f"identical c={c}: {got.tolist()}")
        assert abs(got[0] - 1.0) <= 1e-12 and np.abs(got_map - 1.0).max() <= 1e-12


def constant_pair(h=32, w=64):
    """Images constant in every band whose blocks take the t3 == 0 branch exactly, and the bias they score (the inputs and the
    reasoning of tests/test_q2n_host.py constant_pair)."""
    t, p = np.zeros((4, h, w)), np.zeros((4, h, w))
    p[0], p[1] = 0.25, 1.0
    t[2] = p[2] = 0.75
    t[3] = p[3] = 1.0
    e1, e2 = 4.0, 1.25 ** 2 + 2.0 ** 2 + 2.0
    return t, p, 2.0 * math.sqrt(e1 * e2) / (e1 + e2)


def test_degenerate_bands():
    """The host's conventions: a constant band of the ground truth (divisor 2^-52: finite, next to nothing), an all-zero band
    (shift only), and images constant in every band (t3 == 0: the bias)."""
    t, p = _pair(24, 1, 4, 40, 72)
    t1 = t.clone()
    t1[:, 2] = 0.5
    got, _ = _check(t1, p, what="constant band")
    assert 0.0 <= got[0] < 1e-20
    t2 = t.clone()
    t2[:, 1] = 0.0
    got, _ = _check(t2, p, what="zero band")
    assert 0.5 < got[0] < 1.0
    both = t.clone()
    both[:, 1] = 0.0
    p2 = p.clone()
    p2[:, 1] = 0.0
    _check(both, p2, what="zero band in both")
    for block in (8, 16, 32):
        tc, pc, bias = constant_pair()
        tc, pc = torch.from_numpy(tc).float()[None], torch.from_numpy(pc).float()[None]
        got, got_map = _check(tc, pc, block, block, what=f"constant images, block {block}")
        assert got[0] == bias and (got_map == bias).all()


def test_views_are_scored_in_place():
    from tmdiff_amd import ops
    t, p = _pair(25, 3, 8, 40, 72)
    tc, pc = t.cuda(), p.cuda()
    ts, ps = tc[:, 1:5], pc[:, 1:5]
    assert not ts.is_contiguous()
    got = ops.metrics_q2n(ts, ps)
    assert torch.equal(got.view(torch.int64), ops.metrics_q2n(ts.contiguous(), ps.contiguous()).view(torch.int64))
    want, _ = _host(t[:, 1:5], p[:, 1:5])
    assert (np.abs(got.cpu().numpy() - want) <= TOL).all()
    one = tc[:1].expand(3, -1, -1, -1)                                    # batch stride 0
    assert one.stride(0) == 0
    got = ops.metrics_q2n(one, pc)
    assert torch.equal(got.view(torch.int64), ops.metrics_q2n(one.contiguous(), pc).view(torch.int64))
    want, _ = _host(t[:1].expand(3, -1, -1, -1), p)
    assert (np.abs(got.cpu().numpy() - want) <= TOL).all()
    with pytest.raises(ValueError):
        ops.metrics_q2n(tc[..., ::2], pc[..., ::2])                       # rows must be dense


def test_reproducible_and_capturable():
    """Two calls are bit-identical; a call captured on one stream (one linear graph) and replayed twice equals the eager result."""
    from tmdiff_amd import ops
    t, p = _pair(26, 2, 8, 40, 72)
    t, p = t.cuda(), p.cuda()
    first_map, second_map = (torch.zeros(2, 2, 3, device="cuda", dtype=torch.float64) for _ in range(2))
    first, second = ops.metrics_q2n(t, p, map_out=first_map), ops.metrics_q2n(t, p, map_out=second_map)
    assert torch.equal(first.view(torch.int64), second.view(torch.int64))
    assert torch.equal(first_map.view(torch.int64), second_map.view(torch.int64))
    ws, out = ops.metrics_q2n_workspace(*t.shape, t.device), torch.zeros(2, device="cuda", dtype=torch.float64)
    vals = torch.zeros(2, 2, 3, device="cuda", dtype=torch.float64)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        ops.metrics_q2n(t, p, out=out, map_out=vals, workspace=ws)        # warm-up on the capture stream
    stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        ops.metrics_q2n(t, p, out=out, map_out=vals, workspace=ws)
    for _ in range(2):
        out.zero_()
        vals.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int64), first.view(torch.int64))
        assert torch.equal(vals.view(torch.int64), first_map.view(torch.int64))


def test_quality_switch():
    from tmdiff_amd import metrics as M, ops
    t, p = _pair(27, 2, 8, 40, 72)
    t, p = t.cuda(), p.cuda()
    plain, full = M.quality(t, p), M.quality(t, p, q2n=True)
    assert tuple(plain) == M.PAIR_FIELDS and tuple(full) == M.PAIR_FIELDS + ("q2n",)
    for k in M.PAIR_FIELDS:
        assert torch.equal(plain[k].view(torch.int64), full[k].view(torch.int64)), k
    assert full["q2n"].shape == (2,) and full["q2n"].dtype == torch.float64 and full["q2n"].is_cuda
    assert torch.equal(full["q2n"].view(torch.int64), ops.metrics_q2n(t, p).view(torch.int64))


def test_val_dataset_q2n(tmp_path):
    from tmdiff_amd import evaluate, metrics

    class Trainer:
        def feed_data(self, d):
            self.d = d

        def test(self, continous=False, prompt="QB"):
            self.SR = torch.cat([torch.zeros_like(self.d["HR"]), self.d["HR"] * 0.9 + 0.02 * self.d["N"]])   # stack; last = result

        def get_current_visuals(self):
            return {"SR": self.SR, "HR": self.d["HR"]}

    g = torch.Generator().manual_seed(5)
    loader = [{"HR": (0.1 + 0.8 * torch.rand(1, 8, 40, 36, generator=g)).cuda(), "N": torch.randn(1, 8, 40, 36, generator=g).cuda()}
              for _ in range(2)]
    kw = dict(log=lambda *a: None, device_metrics=True)
    plain = evaluate.val_dataset(Trainer(), "WV3", loader, str(tmp_path / "plain"), **kw)
    off = evaluate.val_dataset(Trainer(), "WV3", loader, str(tmp_path / "off"), q2n=False, **kw)
    full = evaluate.val_dataset(Trainer(), "WV3", loader, str(tmp_path / "q2n"), q2n=True, **kw)
    today = {"sec_per_item"} | {f"{k}_WV3" for k in ("ssim", "sam", "psnr", "ergas", "scc", "cc", "q")}
    assert set(plain) == set(off) == today and set(full) == today | {"q2n_WV3"}
    for k in today - {"sec_per_item"}:
        assert plain[k] == off[k] == full[k], k
    want = []
    for d in loader:
        trainer = Trainer()
        trainer.feed_data(d)
        trainer.test()
        sr = evaluate._to_nchw01(trainer.SR[-1]).cpu()
        want.append(metrics.q2n(d["HR"][0].cpu().numpy(), sr[0].numpy(), hwc=False))
    print(f"q2n_WV3 device {full['q2n_WV3']!r} host {np.mean(want)!r}")
    assert abs(full["q2n_WV3"] - np.mean(want)) <= TOL
    assert os.path.exists(os.path.join(str(tmp_path / "q2n"), "WV3", "output_mulExm_1.mat"))


def test_value_errors():
    """Refused in the wrapper: nothing is launched."""
    from tmdiff_amd import ops
    t = torch.rand(1, 4, 32, 32, device="cuda")
    with pytest.raises(ValueError):
        ops.metrics_q2n(t, t[:, :3])                                        # shapes differ
    big = torch.zeros(1, 17, 32, 32, device="cuda")
    with pytest.raises(ValueError, match="C <= 16"):
        ops.metrics_q2n(big, big)
    with pytest.raises(ValueError, match="block 8, 16 or 32"):
        ops.metrics_q2n(t, t, block=12, shift=12)
    with pytest.raises(ValueError, match="shift <= block"):
        ops.metrics_q2n(t, t, shift=0)
    with pytest.raises(ValueError, match="mirror"):
        ops.metrics_q2n(t[:, :, :15], t[:, :, :15])                         # 17 mirrored rows of 15
    with pytest.raises(ValueError, match="workspace"):
        ops.metrics_q2n(torch.rand(1, 4, 64, 64, device="cuda"), torch.rand(1, 4, 64, 64, device="cuda"),
                        workspace=torch.empty(3, device="cuda", dtype=torch.float64))
    with pytest.raises(ValueError):
        ops.metrics_q2n(t.double(), t.double())                             # not float32
    with pytest.raises(ValueError):
        ops.metrics_q2n(t, t, map_out=torch.empty(1, 2, 2, device="cuda", dtype=torch.float64))
    with pytest.raises(ValueError):
        ops.metrics_q2n(t, t, out=torch.empty(1, device="cuda"))
