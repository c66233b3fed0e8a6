"""Captured-graph sampling for GeneralDiffusion (opt-in: ``ops.config.sample_graph`` / ``TMDIFF_SAMPLE_GRAPH=1``, or per
object ``GeneralDiffusion.sample_graphs = True``).

At small batches a sampling step is bound by the host: ~170 kernel launches per UNet evaluation issued one by one from
Python.  Here the launches of a sampling run are recorded into HIP graphs once per key and replayed; the recorded
launches are the eager ones (same kernels, same arguments, same order), so the results are bit-identical.

DDPM (``p_sample_loop``; hence ``super_resolution`` and ``sample(method="ddpm")``): two graphs over static buffers.
  * condition graph: ``begin_condition_cache`` on the static PAN / MS (the step-invariant half of the UNet);
  * step graph: UNet forward on the cached condition, ``tmdiff_ddpm_step_dev`` (the timestep, its five coefficients and
    the frame slot come from a device step word and a [T, 5] table, so one recording serves every timestep; x is
    updated in place), then ``tmdiff_sampler_tick`` (step word -1, time input of the next evaluation = t + 1).
  Per run the host copies PAN / MS in, replays the condition graph, sets the step word, draws x_T (and writes frame 0),
  then per step draws that step's noise (none at t = 0) and replays the step graph: the random draws happen in eager's
  order, so seeded runs and ``noise_fn`` give the same chain.

DPM-Solver++ (``sample_by_dpmsolver``; hence ``sample(method="dpmsolver")`` and ``tiling.sample_tiled``): the whole
singlestep solve is one graph per key.  Its per-step scalars are host constants of (schedule, steps, order); the time
input of each network evaluation, which eager copies host -> device per call, is read from a device table built before
the capture from the times an eager warm-up run records.  x_T is drawn outside the graph into a static buffer.

Capture rules: an eager warm-up on the capture stream precedes every capture (packed weights, device copies of
constants and the per-stream scratch ``ops._WS`` exist by then, so the capture allocates nothing from the host and
records no copy); one stream; every scratch tensor a graph may have recorded is referenced by its cache entry, so
evicting one entry never frees memory another one reads.
"""
import collections

import torch

from . import ops
from ._lib import lib

_STREAMS = {}      # device index -> the side stream sampling graphs are warmed up and captured on


def _capture_stream(device):
    s = _STREAMS.get(device.index)
    if s is None:
        s = _STREAMS[device.index] = torch.cuda.Stream(device=device)
    return s


def frame_every(T, continous):
    """Stride of the frames p_sample_loop keeps (continous: every ``1 | T // 10``-th step; otherwise only t = 0 is needed)."""
    return (1 | (T // 10)) if continous else T


def frame_slot(t, T, every):
    """Slot of step t in the frame stack (slot 0 = x_T + MS); the library's own definition, the one the kernel uses."""
    return lib.tmdiff_ddpm_frame_slot(t, T, every)


def frame_count(T, every):
    return 2 + (T - 1) // every


def coef_table(step_coef, device):
    """[T, 5] fp32 (c_recip, c_recipm1, coef1, coef2, sigma) from GeneralDiffusion._step_coef: the fp32 values the eager
    step is passed, with sigma = 0 at t = 0 (eager adds no noise there)."""
    rows = [list(c[:4]) + [c[4] if t > 0 else 0.0] for t, c in enumerate(step_coef)]
    return torch.tensor(rows, dtype=torch.float32, device=device)


def _draw(diff, dst, like):
    """dst <- the draw eager's ``diff._noise(like)`` makes (same generator, same order)."""
    if diff.noise_fn is None:
        dst.normal_()
    else:
        dst.copy_(diff._noise(like))


def _new_graph():
    return torch.cuda.CUDAGraph()


def _static_like(t):
    return torch.zeros(t.shape, dtype=torch.float32, device=t.device)


class _Entry:
    """What every captured sampler keeps alive besides its graphs: the packed weights it was recorded with, the device
    copies of the prompt embeddings and every per-stream scratch tensor that existed when it was captured."""

    def _capture(self, net, warmup, record):
        s = _capture_stream(self.device)
        s.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(s):
            warmup()
        torch.cuda.current_stream(self.device).wait_stream(s)
        record(s)
        self.keep = (net._prepare(), dict(net.__dict__.get("_emb_dev", {})), list(ops._WS.values()))


class DdpmGraphs(_Entry):
    def __init__(self, diff, x_in, prompt, continous):
        net = diff.denoise_fn
        res = x_in["Res"]
        self.device, self.shape = res.device, tuple(res.shape)
        self.T = diff.num_timesteps
        self.every = frame_every(self.T, continous)
        self.continous = continous
        self.x, self.noise = _static_like(res), _static_like(res)
        self.pan, self.ms = _static_like(x_in["PAN"]), _static_like(x_in["MS"])
        self.time_in = torch.zeros(res.shape[0], 1, dtype=torch.float32, device=self.device)
        self.step = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.coef = coef_table(diff._step_coef, self.device)
        self.frames = torch.zeros((frame_count(self.T, self.every),) + self.shape, dtype=torch.float32, device=self.device)
        self.cond_graph, self.step_graph = _new_graph(), _new_graph()
        self.pan.copy_(x_in["PAN"])
        self.ms.copy_(x_in["MS"])

        def warmup():
            net.begin_condition_cache(self.pan, self.ms, prompt)
            try:
                ops.sampler_tick(self.step, self.time_in, set_to=self.T - 1)
                self._step(net, prompt)
            finally:
                net.end_condition_cache()

        def record(s):
            with torch.cuda.graph(self.cond_graph, stream=s):
                net.begin_condition_cache(self.pan, self.ms, prompt)
            self.cond = net._cond                 # outputs of the condition graph: the step graph reads them
            try:
                with torch.cuda.graph(self.step_graph, stream=s):
                    self._step(net, prompt)
            finally:
                net.end_condition_cache()

        self._capture(net, warmup, record)

    def _step(self, net, prompt):
        eps = net(self.x, self.time_in, self.pan, self.ms, prompt)
        ops.ddpm_step_dev(self.x, eps, self.noise, self.step, self.coef, ms=self.ms, out=self.x, frames=self.frames,
                          frame_every=self.every)
        ops.sampler_tick(self.step, self.time_in)

    def run(self, diff, x_in):
        self.pan.copy_(x_in["PAN"])
        self.ms.copy_(x_in["MS"])
        self.cond_graph.replay()
        ops.sampler_tick(self.step, self.time_in, set_to=self.T - 1)
        _draw(diff, self.x, x_in["Res"])
        if self.continous:
            ops.add(self.x, self.ms, out=self.frames[0])
        for t in reversed(range(self.T)):
            if t > 0:
                _draw(diff, self.noise, self.x)
            self.step_graph.replay()
        if self.continous:            # torch.cat(frames, dim=0)
            return self.frames.view((-1,) + self.shape[1:]).clone()
        return self.frames[-1][-1].clone()     # the reference's frames[-1][-1]


class DpmGraphs(_Entry):
    def __init__(self, diff, x_in, prompt, steps, order):
        net = diff.denoise_fn
        res = x_in["Res"]
        self.device = res.device
        self.x_T, self.pan, self.ms = _static_like(res), _static_like(x_in["PAN"]), _static_like(x_in["MS"])
        self.pan.copy_(x_in["PAN"])
        self.ms.copy_(x_in["MS"])
        self.graph = _new_graph()
        ns = diff._dpm_schedule()
        self.times = None

        def solve(times=None):
            static = {"Res": self.x_T, "PAN": self.pan, "MS": self.ms}
            net.begin_condition_cache(self.pan, self.ms, prompt)
            try:
                return diff._solve(static, prompt, "x_start", {"PAN": self.pan, "MS": self.ms, "prompt": prompt}, steps,
                                   order, "singlestep", x_T=self.x_T, ns=ns, time_table=times)
            finally:
                net.end_condition_cache()

        def warmup():
            solve()
            # the time input of every network evaluation, in call order: host values as eager computes them
            s = diff.last_solver
            host = torch.stack([s.model.host_time(t, res.shape[0]) for t in s.trace])
            self.times = (host, host.to(self.device))

        def record(s):
            with torch.cuda.graph(self.graph, stream=s):
                self.out = solve(self.times)
            self.solver = diff.last_solver

        self._capture(net, warmup, record)

    def run(self, diff, x_in):
        self.pan.copy_(x_in["PAN"])
        self.ms.copy_(x_in["MS"])
        _draw(diff, self.x_T, x_in["Res"])
        self.graph.replay()
        diff.last_solver = self.solver
        return self.out.clone()


class _Key:
    """Cache key: plain values compared with ==, objects (packed weights, schedule tables) compared with ``is``."""

    def __init__(self, plain, objs):
        self.plain, self.objs = plain, objs

    def __eq__(self, other):
        return self.plain == other.plain and len(self.objs) == len(other.objs) and all(
            a is b for a, b in zip(self.objs, other.objs))


class SampleGraphCache:
    """LRU of captured samplers (bounded by GeneralDiffusion.sample_graph_capacity).  Copies and pickles start empty."""

    def __init__(self):
        self._entries = collections.deque()      # (key, sampler), most recently used last

    def lookup(self, key):
        for i, (k, v) in enumerate(self._entries):
            if k == key:
                del self._entries[i]
                self._entries.append((k, v))
                return v
        return None

    def insert(self, key, sampler, capacity):
        self._entries.append((key, sampler))
        while len(self._entries) > max(1, capacity):
            self._entries.popleft()

    def clear(self):
        self._entries.clear()

    def __len__(self):
        return len(self._entries)

    def __deepcopy__(self, memo):
        return SampleGraphCache()

    def __reduce__(self):
        return SampleGraphCache, ()


def _prompt_key(prompt):
    return tuple(prompt) if isinstance(prompt, (list, tuple)) else prompt


def _base_key(diff, x_in, prompt):
    net = diff.denoise_fn
    dev = x_in["Res"].device
    plain = (tuple(x_in["Res"].shape), tuple(x_in["PAN"].shape), tuple(x_in["MS"].shape), _prompt_key(prompt),
             net.compute_dtype, ops.config.key(), (dev.type, dev.index))
    return plain, (net._prepare(),)


def usable(diff, x_in):
    """Graph mode applies: switched on, no host-side instrumentation, a HIP UNet on the GPU."""
    on = ops.config.sample_graph if diff.sample_graphs is None else diff.sample_graphs
    net = diff.denoise_fn
    return (bool(on) and ops.TIMER is None and ops.COUNTS is None and x_in["Res"].is_cuda
            and hasattr(net, "begin_condition_cache") and hasattr(net, "_prepare"))


def _get(diff, key, make):
    cache = diff.__dict__.get("_sample_graph_cache")
    if cache is None:
        cache = diff.__dict__["_sample_graph_cache"] = SampleGraphCache()
    sampler = cache.lookup(key)
    if sampler is None:
        sampler = make()
        cache.insert(key, sampler, diff.sample_graph_capacity)
        diff.sample_graph_captures += 1
    return sampler


def ddpm(diff, x_in, prompt, continous):
    plain, objs = _base_key(diff, x_in, prompt)
    key = _Key(("ddpm", diff.num_timesteps, True, bool(continous)) + plain, objs + (diff._step_coef,))
    return _get(diff, key, lambda: DdpmGraphs(diff, x_in, prompt, bool(continous))).run(diff, x_in)


def dpmsolver(diff, x_in, prompt, steps, order=3):
    plain, objs = _base_key(diff, x_in, prompt)
    key = _Key(("dpmsolver", steps, order, diff.betas._version) + plain, objs + (diff.betas,))
    return _get(diff, key, lambda: DpmGraphs(diff, x_in, prompt, steps, order)).run(diff, x_in)
