"""Captured-graph sampling (tmdiff_amd.sample_graph): every public sampling call with graphs switched on returns exactly
(torch.equal) what the eager path returns, captured samplers are reused and recaptured when they must be, and the
recorded step holds no copy."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import unet_ref as U
from oracle.make_golden import TINY, case_inputs

pytestmark = pytest.mark.gpu

FULL = [32, 64, 128, 256]


@pytest.fixture(autouse=True)
def _inference_mode():
    with torch.no_grad():
        yield


def cpu_noise(like):
    return torch.randn(like.shape, dtype=torch.float32)


def dev_inputs(d):
    return {k: v.cuda().contiguous() for k, v in d.items()}


def _net(channels, seed=0):
    from tmdiff_amd.Hyper_unet_general import WavBEST
    ref = U.fill_weights_(U.WavBESTRef(channels=channels), seed=seed)
    net = WavBEST(channels=channels)
    net.load_state_dict(ref.state_dict())
    return net.cuda().eval()


@pytest.fixture(scope="module")
def tiny_net():
    return _net(TINY)


def _diff(net, T, noise_fn=cpu_noise):
    from tmdiff_amd.diffusion_general import GeneralDiffusion
    diff = GeneralDiffusion(net, "l1", noise_fn=noise_fn).cuda()
    diff.set_new_noise_schedule({"schedule": "cosine", "n_timestep": T}, "cuda")
    return diff


def _both(diff, call, seed):
    """(eager, graph) results of call(diff) from the same seed."""
    diff.sample_graphs = False
    torch.manual_seed(seed)
    eager = call(diff)
    diff.sample_graphs = True
    torch.manual_seed(seed)
    graph = call(diff)
    diff.sample_graphs = None
    return eager, graph


def _equal(a, b):
    assert a.shape == b.shape and a.stride() == b.stride(), (a.shape, b.shape, a.stride(), b.stride())
    assert torch.equal(a, b), float((a - b).abs().max())


@pytest.mark.parametrize("T", [10, 50])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("continous", [True, False])
def test_ddpm_graph_equals_eager(tiny_net, T, B, continous):
    diff = _diff(tiny_net, T)
    d = dev_inputs(case_inputs(140 + T, B, 8, 16))
    eager, graph = _both(diff, lambda g: g.p_sample_loop(d, continous=continous, prompt="WV3"), T)
    _equal(eager, graph)
    assert diff.sample_graph_captures == 1
    # super_resolution (the reference driver's validation path) and the clean entry point go through it too
    eager, graph = _both(diff, lambda g: g.super_resolution(d, False, "WV3", 3.0), T + 1)
    _equal(eager, graph)
    eager, graph = _both(diff, lambda g: g.sample(d, "WV3"), T + 2)
    _equal(eager, graph)


@pytest.mark.parametrize("T", [10, 50])
def test_ddpm_graph_against_golden(tiny_net, golden, T):
    from tmdiff_amd.util import psnr
    g = golden("ddpm")
    diff = _diff(tiny_net, T)
    diff.sample_graphs = True
    d = dev_inputs(case_inputs(140 + T, 2, 8, 16))
    torch.manual_seed(T)
    stack = diff.super_resolution(d, False, "WV3", 3.0).cpu()
    assert list(stack.shape) == list(g[f"T{T}_stack_shape"])
    assert np.abs(stack[-2:].numpy() - g[f"T{T}_final"]).max() <= 2e-3
    assert psnr(stack[-2:], torch.tensor(g[f"T{T}_final"])) >= 60.0
    assert np.abs(stack[2:6].numpy() - g[f"T{T}_mid"]).max() <= 2e-3
    torch.manual_seed(T)
    last = diff.p_sample_loop(d, continous=False, prompt="WV3").cpu()
    assert np.abs(last.numpy() - g[f"T{T}_last_only"]).max() <= 2e-3


def test_ddpm_graph_full_width_production_kernels(monkeypatch):
    from tmdiff_amd import ops
    monkeypatch.setattr(ops.config, "wino_min_blocks", 1)
    diff = _diff(_net(FULL), 50)
    d = dev_inputs(case_inputs(171, 2, 8, 32))
    eager, graph = _both(diff, lambda g: g.p_sample_loop(d, continous=False, prompt="WV3"), 50)
    _equal(eager, graph)
    eager, graph = _both(diff, lambda g: g.super_resolution(d, False, "WV3", 3.0), 51)
    _equal(eager, graph)


def test_reuse_and_recapture():
    net = _net(TINY)
    diff = _diff(net, 10, noise_fn=None)          # the device generator: seeded draws in eager's order
    d1, d2 = dev_inputs(case_inputs(1, 2, 8, 16)), dev_inputs(case_inputs(2, 2, 8, 16))
    run = lambda d, prompt="WV3": (lambda g: g.p_sample_loop(d, continous=True, prompt=prompt))
    for k, d in enumerate((d1, d2, d1)):
        eager, graph = _both(diff, run(d), 7 + k)
        _equal(eager, graph)
    assert diff.sample_graph_captures == 1
    eager, graph = _both(diff, run(d1, "GF2"), 11)                  # another prompt: another key
    _equal(eager, graph)
    assert diff.sample_graph_captures == 2
    net.load_state_dict(_net(TINY, seed=5).state_dict())            # new weights: new packed weights, recapture
    eager, graph = _both(diff, run(d1), 12)
    _equal(eager, graph)
    assert diff.sample_graph_captures == 3
    net.invalidate_prepared()                                        # (what the EMA update does)
    eager, graph = _both(diff, run(d1), 13)
    _equal(eager, graph)
    assert diff.sample_graph_captures == 4
    net.set_compute_dtype("bf16")
    try:
        eager, graph = _both(diff, run(d1), 14)
        _equal(eager, graph)
        assert diff.sample_graph_captures == 5
    finally:
        net.set_compute_dtype("fp32")
    diff.release_sample_graphs()
    eager, graph = _both(diff, run(d1), 15)
    _equal(eager, graph)
    assert diff.sample_graph_captures == 6


def test_lru_eviction(tiny_net):
    diff = _diff(tiny_net, 10)
    inputs = [dev_inputs(case_inputs(20 + b, b, 8, 16)) for b in (1, 2, 3)]      # three batch shapes: three keys
    call = lambda d: (lambda g: g.p_sample_loop(d, continous=True, prompt="QB"))
    for k, d in enumerate(inputs):
        eager, graph = _both(diff, call(d), 30 + k)
        _equal(eager, graph)
    assert diff.sample_graph_captures == 3 and len(diff._sample_graph_cache) == 2
    eager, graph = _both(diff, call(inputs[0]), 40)          # evicted: captured again, still exact
    _equal(eager, graph)
    assert diff.sample_graph_captures == 4
    eager, graph = _both(diff, call(inputs[2]), 41)          # still cached: its scratch outlived the eviction
    _equal(eager, graph)
    assert diff.sample_graph_captures == 4


@pytest.mark.parametrize("steps", [6, 20])
def test_dpmsolver_graph_equals_eager(tiny_net, steps):
    diff = _diff(tiny_net, 1000)
    d = dev_inputs(case_inputs(150 + steps, 2, 8, 16))
    diff.sample_graphs = False
    torch.manual_seed(steps)
    eager = diff.sample_by_dpmsolver(d, "WV3", steps=steps)
    nfe, trace = diff.last_solver.nfe, list(diff.last_solver.trace)
    diff.sample_graphs = True
    for rep in range(2):                   # first call captures, second replays
        torch.manual_seed(steps)
        graph = diff.sample_by_dpmsolver(d, "WV3", steps=steps)
        _equal(eager, graph)
        assert diff.last_solver.nfe == nfe == steps + 1 and diff.last_solver.trace == trace
    assert diff.sample_graph_captures == 1
    torch.manual_seed(steps)
    via_sample = diff.sample(d, "WV3", method="dpmsolver", steps=steps)
    _equal(eager, via_sample)


def test_sample_tiled_graph_equals_eager(tiny_net):
    from tmdiff_amd.tiling import sample_tiled
    diff = _diff(tiny_net, 1000)
    d = case_inputs(9, 1, 4, 64)
    scene = {"MS": d["MS"].cuda(), "PAN": d["PAN"].cuda()}
    eager, graph = _both(diff, lambda g: sample_tiled(g, scene, "GF2", tile=16, method="dpmsolver", steps=6, max_batch=8), 4)
    _equal(eager, graph)


def _hip():
    """The HIP runtime this process already uses (torch's), by path."""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return ctypes.CDLL(line.split()[-1])
    raise RuntimeError("libamdhip64 is not loaded")


def _node_types(graph):
    hip = _hip()
    raw = graph.raw_cuda_graph()
    g = ctypes.c_void_p(raw if isinstance(raw, int) else int(raw))
    n = ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(g, None, ctypes.byref(n)) == 0
    nodes = (ctypes.c_void_p * n.value)()
    assert hip.hipGraphGetNodes(g, nodes, ctypes.byref(n)) == 0
    types = []
    for k in range(n.value):
        t = ctypes.c_int(-1)
        assert hip.hipGraphNodeGetType(ctypes.c_void_p(nodes[k]), ctypes.byref(t)) == 0
        types.append(t.value)
    return types


@pytest.mark.parametrize("channels", ["tiny", "full"])
def test_recorded_graphs_hold_no_copy(monkeypatch, channels):
    from tmdiff_amd import ops
    from tmdiff_amd import sample_graph as sg
    KERNEL, MEMCPY, MEMCPY_FROM_SYMBOL, MEMCPY_TO_SYMBOL = 0, 1, 12, 13
    monkeypatch.setattr(sg, "_new_graph", lambda: torch.cuda.CUDAGraph(keep_graph=True))
    if channels == "full":
        monkeypatch.setattr(ops.config, "wino_min_blocks", 1)
    diff = _diff(_net(FULL if channels == "full" else TINY), 10)
    diff.sample_graphs = True
    d = dev_inputs(case_inputs(3, 1, 8, 16))
    torch.manual_seed(0)
    diff.p_sample_loop(d, continous=True, prompt="WV3")
    diff.sample_by_dpmsolver(d, "WV3", steps=6)
    (_, ddpm), (_, dpm) = list(diff._sample_graph_cache._entries)
    for graph in (ddpm.cond_graph, ddpm.step_graph, dpm.graph):
        types = _node_types(graph)
        assert types.count(KERNEL) > 0
        assert not {MEMCPY, MEMCPY_FROM_SYMBOL, MEMCPY_TO_SYMBOL} & set(types), sorted(set(types))
