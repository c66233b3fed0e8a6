"""Device quality metrics (csrc/metrics.hip) against the float64 host definitions of tmdiff_amd/metrics.py.

Tolerance: 1e-9, relative or absolute, whichever is larger.  Both sides add exact fp32 values (and exact products of two of
them) in fp64, so they differ by the order of summation only: below N * 2^-53, about 3e-12 for the 8 x 512 x 512 scene, and the
cancellation in a variance at sensor scale (second moment / variance = 4e4) costs a few more digits of that.  The host SAM is
called on [C, H, W] arrays (hwc=False): NumPy then adds the bands one after the other, as the kernel does, which matters for
identical and parallel spectra whose angle is a rounding error of the cosine."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-9


def _host_pair(a, b, data_range=1.0, ratio=0.25):
    """PAIR_FIELDS of one image pair (float32 CPU tensors [C, H, W]) from the host functions."""
    from tmdiff_amd import metrics as M
    a64, b64 = a.double().numpy(), b.double().numpy()
    with np.errstate(all="ignore"):
        row = [M.mpsnr(a, b, data_range, hwc=False), M.sam(a64, b64, hwc=False), M.ssim(a, b, data_range, hwc=False),
               M.ergas(a64, b64, ratio, hwc=False), M.rmse(a64, b64, hwc=False), M.cc(a64, b64, hwc=False),
               M.scc(a64, b64, hwc=False), M.q_index(a64, b64, hwc=False),
               M.q4(a64, b64, hwc=False) if a.shape[0] == 4 else float("nan")]
    return row


def _check_rows(got, want, what):
    from tmdiff_amd.metrics import PAIR_FIELDS, NOREF_FIELDS
    names = PAIR_FIELDS if len(want[0]) == len(PAIR_FIELDS) else NOREF_FIELDS
    got = got.cpu().tolist()
    assert len(got) == len(want), what
    bad = []
    for i, (g_row, w_row) in enumerate(zip(got, want)):
        for k, g, w in zip(names, g_row, w_row):
            if math.isnan(w) or math.isinf(w):
                ok = (math.isnan(g) and math.isnan(w)) or g == w
                err = float("nan")
            else:
                err = abs(g - w)
                ok = err <= TOL * max(1.0, abs(w))
            print(f"{what}[{i}] {k}: device {g!r} host {w!r} |diff| {err:.2e}")
            if not ok:
                bad.append((i, k, g, w))
    assert not bad, (what, bad)


def _pair(seed, b, c, h, w, noise=0.05):
    g = torch.Generator().manual_seed(seed)
    t = torch.rand(b, c, h, w, generator=g)
    p = (t + noise * torch.randn(b, c, h, w, generator=g)).clamp(0, 1)
    return t, p


def _score(t, p, **kw):
    from tmdiff_amd import ops
    return ops.metrics_pair(t.cuda(), p.cuda(), **kw)


def _golden_pair(golden, tag):
    g = golden("metrics")
    chw = lambda x: torch.from_numpy(np.ascontiguousarray(np.moveaxis(x, -1, 0)))[None]
    return chw(g[f"{tag}_hr"]), chw(g[f"{tag}_sr"])


@pytest.mark.parametrize("tag", ["wv3_f32", "gf2_f32"])
def test_golden_cases_with_degenerate_pixels(golden, tag):
    """24 x 20 x 8 and 16 x 16 x 4: smaller than a tile, ragged; pixels with a zero spectrum in either image, identical and
    parallel spectra (oracle/make_golden.py).  The device also lands on the reference's own numbers."""
    t, p = _golden_pair(golden, tag)
    got = _score(t, p)
    _check_rows(got, [_host_pair(t[0], p[0])], tag)
    from tmdiff_amd.metrics import PAIR_FIELDS
    gs = golden("metrics_suite")
    for k in ("rmse", "ergas", "cc", "scc", "q") + (("q4",) if t.shape[1] == 4 else ()):
        want = float(gs[f"{tag}_{k}"])
        assert abs(float(got[0, PAIR_FIELDS.index(k)]) - want) <= TOL * max(1.0, abs(want)), k


SHAPES = {"b3_c8_70x45": (3, 8, 70, 45),          # crosses tile borders both ways, ragged edges, batch index in every offset
          "c4_64x64": (1, 4, 64, 64),             # tile-exact, Q4 on
          "c1_7x7": (1, 1, 7, 7),                 # exactly one SSIM window, a 5 x 5 Laplacian
          "c16_9x33": (1, 16, 9, 33),
          "scene_8x512x512": (1, 8, 512, 512)}


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes(name):
    b, c, h, w = SHAPES[name]
    t, p = _pair(11, b, c, h, w)
    got = _score(t, p)
    assert got.shape == (b, 9) and got.dtype == torch.float64 and got.is_cuda
    _check_rows(got, [_host_pair(t[i], p[i]) for i in range(b)], name)
    assert bool(torch.isnan(got[:, 8]).all()) == (c != 4)


def test_non_contiguous_inputs():
    """A channel slice of a 9-channel tensor and every second batch entry are scored in place."""
    from tmdiff_amd import ops
    t9, p9 = _pair(12, 4, 9, 40, 70)
    tc, pc = t9.cuda(), p9.cuda()
    ts, ps = tc[::2, 2:6], pc[::2, 2:6]
    assert not ts.is_contiguous()
    got = ops.metrics_pair(ts, ps)
    _check_rows(got, [_host_pair(t9[i, 2:6], p9[i, 2:6]) for i in (0, 2)], "slices")
    assert torch.equal(got, ops.metrics_pair(ts.contiguous(), ps.contiguous()))
    with pytest.raises(ValueError):
        ops.metrics_pair(tc[..., ::2], pc[..., ::2])                 # rows must be dense
    with pytest.raises(ValueError):
        ops.metrics_pair(tc[:, :, :6], pc[:, :, :6])                 # H = 6
    big = torch.zeros(1, 17, 8, 8, device="cuda")
    with pytest.raises(ValueError):
        ops.metrics_pair(big, big)                                    # C = 17


def test_sensor_scale_data():
    """mean 1000, sigma 5, data_range 2047: the variances are 4e-5 of the second moments -- fp32 sums would return noise."""
    g = torch.Generator().manual_seed(13)
    t = 1000.0 + 5.0 * torch.randn(2, 4, 40, 70, generator=g)
    p = t + 2.0 * torch.randn(2, 4, 40, 70, generator=g)
    got = _score(t, p, data_range=2047.0)
    _check_rows(got, [_host_pair(t[i], p[i], 2047.0) for i in range(2)], "sensor")


def test_identical_inputs():
    """Identical images: psnr inf, sam / rmse / ergas 0, ssim / cc / q 1."""
    t, _ = _pair(14, 1, 4, 20, 70)
    _check_rows(_score(t, t.clone()), [_host_pair(t[0], t[0])], "identical")


@pytest.mark.parametrize("value", [0.5, 0.7, 0.1, 0.0, 1000.3])
@pytest.mark.parametrize("h,w", [(40, 70), (70, 45)])
def test_constant_band(value, h, w):
    """A constant band: NaN in the host's columns.  0.5 and 0 are the values whose raw second moments are exact; for 0.7, 0.1
    and 1000.3 n v^2 rounds, so the raw-moment variance of the band is a rounding residue and not 0.  Ragged shapes of several
    tiles."""
    t, p = _pair(14, 1, 4, h, w)
    p1 = p.clone()
    p1[:, 2] = value                                 # constant in the prediction only: cc and scc NaN, q finite
    want = _host_pair(t[0], p1[0])
    assert math.isnan(want[5]) and math.isnan(want[6]) and not math.isnan(want[7])
    _check_rows(_score(t, p1), [want], f"band of {value} in one image")
    t2 = t.clone()
    t2[:, 2] = value                                 # constant in both: q NaN too
    want = _host_pair(t2[0], p1[0])
    assert math.isnan(want[5]) and math.isnan(want[6]) and math.isnan(want[7])
    _check_rows(_score(t2, p1), [want], f"band of {value} in both images")
    t3 = t.clone()
    t3[:, 0] = value                                 # constant in the target only, another band
    want = _host_pair(t3[0], p[0])
    assert math.isnan(want[5]) and math.isnan(want[6])
    _check_rows(_score(t3, p), [want], f"band of {value} in the target")


@pytest.mark.parametrize("c,h,w", [(4, 64, 64), (8, 76, 132)])
def test_quality_noref(c, h, w):
    """4 and 8 bands, l_ms at H / 4; 76 x 132 is no multiple of any tile or chunk."""
    from tmdiff_amd import metrics as M
    g = torch.Generator().manual_seed(15)
    b = 2
    ps = torch.rand(b, c, h, w, generator=g)
    pan = (ps.mean(1, keepdim=True) + 0.05 * torch.randn(b, 1, h, w, generator=g)).clamp(0, 1)
    l_ms = torch.nn.functional.avg_pool2d(ps + 0.03 * torch.randn(b, c, h, w, generator=g), 4)
    l_pan = torch.nn.functional.avg_pool2d(pan, 4)
    got = M.quality_noref(l_ms.cuda(), pan.cuda(), l_pan.cuda(), ps.cuda())
    assert tuple(got) == M.NOREF_FIELDS and all(v.shape == (b,) and v.dtype == torch.float64 and v.is_cuda for v in got.values())
    want = [[M.d_lambda(l_ms[i], ps[i], hwc=False), M.d_s(l_ms[i], pan[i], l_pan[i], ps[i], hwc=False),
             M.qnr(l_ms[i], pan[i], l_pan[i], ps[i], hwc=False)] for i in range(b)]
    _check_rows(torch.stack([got[k] for k in M.NOREF_FIELDS], 1), want, f"noref c={c}")


def test_noref_golden(golden):
    from tmdiff_amd import ops
    gs, g = golden("metrics_suite"), golden("metrics")
    for tag in ("wv3_f32", "gf2_f32"):
        f32 = lambda x: torch.from_numpy(np.ascontiguousarray(np.moveaxis(x if x.ndim == 3 else x[..., None], -1, 0)).astype(np.float32))[None]
        got = ops.metrics_noref(f32(gs[f"{tag}_l_ms"]).cuda(), f32(gs[f"{tag}_pan"]).cuda(), f32(gs[f"{tag}_l_pan"]).cuda(),
                                f32(g[f"{tag}_sr"]).cuda())
        _check_rows(got, [[float(gs[f"{tag}_{k}"]) for k in ("d_lambda", "d_s", "qnr")]], f"noref {tag}")


def test_reproducible_and_capturable():
    """Two calls are bit-identical; a call captured on one stream and replayed twice equals the eager result bit for bit."""
    from tmdiff_amd import metrics as M, ops
    t, p = _pair(16, 2, 8, 70, 45)
    t, p = t.cuda(), p.cuda()
    first, second = ops.metrics_pair(t, p), ops.metrics_pair(t, p)
    assert torch.equal(first.view(torch.int64), second.view(torch.int64))
    q = M.quality(t, p)
    assert tuple(q) == M.PAIR_FIELDS and torch.equal(q["ergas"].view(torch.int64), first[:, 3].view(torch.int64))
    ws, out = ops.metrics_workspace(*t.shape, t.device), torch.zeros(2, 9, device="cuda", dtype=torch.float64)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        ops.metrics_pair(t, p, out=out, workspace=ws)                 # warm-up on the capture stream
    stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        ops.metrics_pair(t, p, out=out, workspace=ws)
    for _ in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int64), first.view(torch.int64))


def test_val_dataset_device_metrics(tmp_path, golden):
    import scipy.io as scio
    from tmdiff_amd import evaluate, metrics

    class Trainer:
        def feed_data(self, d):
            self.d = d

        def test(self, continous=False, prompt="QB"):
            self.SR = torch.cat([torch.zeros_like(self.d["HR"]), self.d["HR"] * 1.5 - 0.2])   # stack; last = result

        def get_current_visuals(self):
            return {"SR": self.SR, "HR": self.d["HR"]}

    g = torch.Generator().manual_seed(3)
    loader = [{"HR": torch.rand(1, 4, 16, 16, generator=g).cuda()} for _ in range(2)]
    host = evaluate.val_dataset(Trainer(), "GF2", loader, str(tmp_path / "host"), log=lambda *a: None)
    dev = evaluate.val_dataset(Trainer(), "GF2", loader, str(tmp_path / "dev"), log=lambda *a: None, device_metrics=True)
    assert set(host) == {"ssim_GF2", "sam_GF2", "sec_per_item"}
    assert set(dev) == set(host) | {f"{k}_GF2" for k in ("psnr", "ergas", "scc", "cc", "q")}
    # SAM: the host path works in float32 as the reference does, the device in float64; the allowance is 4x the distance between
    # the two on the golden inputs, taken from the fixture (the reference's float32 value) and the host float64 evaluation
    gm = golden("metrics")
    hr, sr = gm["wv3_f32_hr"], gm["wv3_f32_sr"]
    gap = abs(metrics.sam(sr.astype(np.float64), hr.astype(np.float64)) - float(gm["wv3_f32_sam"]))
    print(f"ssim host {host['ssim_GF2']!r} device {dev['ssim_GF2']!r}; sam host {host['sam_GF2']!r} device {dev['sam_GF2']!r}; "
          f"float32 / float64 gap on wv3_f32 {gap:.3e}")
    assert 0 < gap < 1e-4
    assert abs(dev["ssim_GF2"] - host["ssim_GF2"]) <= 1e-6
    assert abs(dev["sam_GF2"] - host["sam_GF2"]) <= 4 * gap
    assert all(math.isfinite(dev[f"{k}_GF2"]) for k in ("psnr", "ergas", "scc", "cc", "q"))
    for i in range(2):
        a = scio.loadmat(os.path.join(str(tmp_path / "host"), "GF2", f"output_mulExm_{i}.mat"))["sr"]
        b = scio.loadmat(os.path.join(str(tmp_path / "dev"), "GF2", f"output_mulExm_{i}.mat"))["sr"]
        assert a.dtype == b.dtype and np.array_equal(a, b)
