"""conv3d_wf (csrc/conv3d_wf.hip) on the paths test_gpu_kernels.py never runs: planes lower than a tile (H = 1, 2, 3), a ragged
last row tile, last column tiles of one, two and three quads, W = 4 (narrower than the raw box's left margin), pair mode at
H = 1 / 3 / 9 with B = 1 / 2 / 3 and on grouped segments, one chunk, odd chunk counts, split-K ranges of two chunks, the doubling
branch of the split rule, 128 chunks unsplit, folds of 32 / 96 / 512 channels (on 4 bands, on a ragged plane, on a grid that
splits), the quarter outputs at H = 2, the prologue pass in every form, dropout with a kept x', the data-gradient packing and the
composed-LL mode in its three geometries (conv3d_wf_refs.CASES; test_conv3d_wf_refs_host.py asserts what each case reaches).
Every call goes through ops.conv3d_wf / ops.conv3d_wf_ll; ops.COUNTS shows that launch key alone; every output tensor lies
between two guards of sentinel floats and starts as NaN.

Exact tier.  On lattice inputs (x integers in [-2, 2], w = 24 j, integer bias / residual / shifts, power-of-two scales; no SiLU
in the prologue) no fp32 operation of the launch rounds (conv3d_wf_refs.exactness_ok, proved on the host), so every output
must EQUAL the fp64 reference, bit for bit -- split-K sums and folds included: one lost, doubled or misplaced term is an error of
at least one lattice step whatever the sizes.  Outputs that went through SiLU (y2 with act, LL' of the Haar form) are compared
with SiLU in fp64 of the exact argument at SILU_MAX / SILU_L2; everything else in that launch stays exact.  Each case that uses
the prologue or the split-K workspace runs on workspaces filled with NaN and again after the launches with the largest
workspaces (stale finite values): same bits.

Rounding tier.  On normal data, the cases marked R: maximum error over the maximum of the fp64 reference.  Measured on the
MI355X (profiles/wf_edges.txt; the direct kernel on the same inputs for information):
    case              conv3d_wf    conv3d (direct)
    h1-w12            4.347e-07    1.020e-07
    h9-w4             8.208e-07    2.808e-07
    pair-h8-b3        8.369e-07    3.102e-07
    long-sum-16x16    4.303e-07    2.048e-07
    doubling          8.946e-07    3.457e-07
    cin256-unsplit    3.391e-06    1.236e-06
    fold512-split     7.803e-07    3.603e-07
BOUND = 2 x the worst conv3d_wf figure (3.391e-6: 128 chunks summed in one range), rounded up, under the 2e-5 ceiling of the
existing conv3d_wf tests.  The SiLU outputs of the exact tier measure at most 5.450e-9 (max-rel) / 4.272e-9 (rel-L2) against
fp64 (same file); SILU_MAX / SILU_L2 = 4 x those, rounded up -- the factor allows for the spread of fp32 exp rounding over other
data -- under the 2e-5 / 2e-6 ceiling.

"long-sum-16x16" is the shape at which the doubling branch of the split rule was expected (Cin/g = 128 on a 16 x 16 x 8 plane,
B = 1, Cout = 32); its two tiles end at 32 ranges of two chunks and cannot take the branch, "doubling" is the smallest grid
that does (conv3d_wf_refs.py).
"""
import collections
import functools
import math

import pytest
import torch

import conv3d_wf_refs as R
from conftest import rel_err

pytestmark = pytest.mark.gpu

BOUND = 7e-6                        # 2 x 3.391e-6 (profiles/wf_edges.txt), rounded up; the ceiling is 2e-5
SILU_MAX, SILU_L2 = 2.5e-8, 2e-8    # 4 x 5.450e-9 / 4 x 4.272e-9 (profiles/wf_edges.txt), rounded up; the ceiling is 2e-5 / 2e-6
assert BOUND <= 2e-5 and SILU_MAX <= 2e-5 and SILU_L2 <= 2e-6
NAN = float("nan")
GUARD, SENTINEL = 4096, 12345.0
PLANS = {c.name: R.case_plan(c) for c in R.CASES}
LARGEST_SPLITK = max(R.CASES, key=lambda c: PLANS[c.name].splitk_bytes).name
LARGEST_PRO = max((c for c in R.CASES if not c.opt["drop"]), key=lambda c: PLANS[c.name].prologue_bytes).name
WS_TAGS = (("splitk", PLANS[LARGEST_SPLITK].splitk_bytes), ("x", PLANS[LARGEST_PRO].prologue_bytes))


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from tmdiff_amd import ops as _ops
    return _ops


def cu(t):
    return None if t is None else t.cuda().contiguous()


class Guarded:
    """While active, every fp32 tensor the wrappers allocate on the GPU (their outputs) is NaN between two guards of sentinels."""

    def __enter__(self):
        self.bufs, self.real = [], torch.empty

        def empty(*shape, **kw):
            if kw.get("dtype") is torch.float32 and "device" in kw and torch.device(kw["device"]).type == "cuda":
                shape = tuple(shape[0]) if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)) else shape
                n = math.prod(shape)
                buf = self.real(n + 2 * GUARD, **kw)
                buf.fill_(SENTINEL)
                buf[GUARD:GUARD + n].fill_(NAN)
                self.bufs.append((buf, n))
                return buf[GUARD:GUARD + n].view(*shape)
            return self.real(*shape, **kw)

        torch.empty = empty
        return self

    def __exit__(self, *exc):
        torch.empty = self.real

    def guarded(self, *shape):
        return torch.empty(*shape, device="cuda", dtype=torch.float32)

    def check(self, what):
        torch.cuda.synchronize()
        for buf, n in self.bufs:
            assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all()), f"{what}: a store landed outside an output"


def pack(ops, c, w):
    if c.opt["llm"]:
        return ops.pack_conv_weight_wfll(w, c.opt["ll_scale"])
    return ops.pack_conv_weight_wino(w, groups=c.groups, mode=3 if c.opt["dgrad"] else 2, planes=6)


def launch_args(ops, c, t):
    """(input tensors, packed weights, keywords of ops.conv3d_wf / conv3d_wf_ll) for a case on the CPU tensors t"""
    o = c.opt
    kw = dict(bias=cu(t["bias"]), bias_scale=o["bias_scale"], residual=cu(t["res"]), out_scale=o["out_scale"], keep_y=o["keep_y"])
    if o["pro"] is not None:
        kw.update(in_shift=cu(t["sh"]), in_scale=cu(t["sc"]), in_act=t["pro_act"])
    if o["drop"]:
        kw["drop"] = R.DROP
    if o["y2"] is not None:
        kw["emit"] = dict(act=o["y2"]["act"], shift=cu(t["sh2"]), scale=cu(t["sc2"]), s2d=o["s2d"], ll=o["ll"], dwt=o["dwt"])
    if o["rc"]:
        kw["res_conv"] = (cu(t["rc_x"]), cu(t["rc_w"]), o["rc"])
    xs = [cu(R.s2d(t["xs"][0]))] if o["llm"] else [cu(x) for x in t["xs"]]
    return xs, pack(ops, c, cu(t["w"])), kw


def launch(ops, c, xs, wp, kw, **extra):
    """One launch inside the guards: {output name: device tensor}; COUNTS shows the launch key alone"""
    keep, ops.COUNTS = ops.COUNTS, collections.Counter()
    try:
        with Guarded() as g:
            if c.opt["llm"]:
                out = ops.conv3d_wf_ll(xs[0], wp, c.cout, c.opt["ll_scale"], **kw)
            else:
                out = ops.conv3d_wf(xs, wp, c.cout, groups=c.groups, **kw, **extra)
        counts = dict(ops.COUNTS)
    finally:
        ops.COUNTS = keep
    assert counts == {"conv3d_wfll_fwd" if c.opt["llm"] else "conv3d_wf_fwd": 1}, counts
    g.check(c.name)
    out = out if isinstance(out, (tuple, list)) else (out,)
    names = R.outputs_of(c)
    assert len(out) == len(names) == len(g.bufs), (len(out), names, len(g.bufs))
    return dict(zip(names, out))


@functools.lru_cache(maxsize=None)
def device_case(name, kind):
    """the device tensors of a case's lattice / real inputs, made once"""
    from tmdiff_amd import ops as _ops
    t = (R.lattice_case if kind == "lattice" else R.real_case)(name)[0]
    return launch_args(_ops, R.CASE[name], t)


def workspaces(ops):
    """float32 views of the two per-stream workspaces, each at least as large as its largest user among the cases"""
    dev = torch.device("cuda", torch.cuda.current_device())
    out = []
    for tag, nbytes in WS_TAGS:
        ws = ops._workspace(dev, nbytes, tag)
        out.append(ws[:ws.numel() // 4 * 4].view(torch.float32))
    return out


def compare(name, got, ref, worst):
    c = R.CASE[name]
    silu = R.silu_outputs(c)
    for k in R.outputs_of(c):
        want = ref[k]
        assert got[k].shape == want.shape, (k, got[k].shape, want.shape)
        assert not bool(torch.isnan(got[k]).any()), f"{name}: {k} holds NaN (an element never written, or read from a poisoned workspace)"
        if k in silu:
            m, l2 = rel_err(got[k], want)
            worst.append((m, l2))
            print(f"conv3d_wf edges silu [{name}] {k}: max-rel {m:.3e} rel-L2 {l2:.3e}")
            assert m <= SILU_MAX and l2 <= SILU_L2, (name, k, m, l2)
        else:
            bad = got[k].double() != want
            assert not bool(bad.any()), (f"{name}: {k} differs from the fp64 reference in {int(bad.sum())} of {bad.numel()} elements, "
                                         f"first at {tuple(bad.nonzero()[0].tolist())}, largest {float((got[k].double() - want).abs().max())}")
            assert torch.equal(got[k], want.float())


@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_exact_on_lattice_inputs_whatever_the_workspaces_hold(ops, name):
    c, p = R.CASE[name], PLANS[name]
    t, ref = R.lattice_case(name)
    xs, wp, kw = device_case(name, "lattice")
    extra = {}
    if c.opt["drop"]:      # x' as the kernel keeps it: the direct kernels' keep mask on the prologue output, kept values * 1.25
        xp_out = torch.full((c.B, sum(c.segs), c.N, c.H, c.W), NAN, device="cuda")
        extra["xp_out"] = xp_out
    for ws in workspaces(ops):
        ws.fill_(NAN)
    got = {k: v.cpu() for k, v in launch(ops, c, xs, wp, kw, **extra).items()}
    if c.opt["drop"]:
        xp, x0 = xp_out.cpu(), R.prologue64(t).float()
        assert torch.equal(xp, ops.conv3d_prologue(xs, in_shift=kw["in_shift"], drop=R.DROP).cpu()), "xp_out is not the direct kernels' x'"
        keep = (xp != 0) | (x0 == 0)
        assert torch.equal(xp, torch.where(keep, 1.25 * x0, torch.zeros_like(x0))), "x' is not 0 or 1.25 (x + shift)"
        assert 0.1 < float(((xp == 0) & (x0 != 0)).float().sum() / (x0 != 0).float().sum()) < 0.3
        assert R.exactness_ok(c, t, xp)[0]
        ref = R.reference(c, t, xp=xp)
    worst = []
    compare(name, got, ref, worst)
    if p.prologue_bytes or p.splitk_bytes:
        for big in (LARGEST_SPLITK, LARGEST_PRO):                      # leave stale finite values in both workspaces
            launch(ops, R.CASE[big], *device_case(big, "lattice"))
        if c.opt["drop"]:
            xp_out.fill_(NAN)
        again = {k: v.cpu() for k, v in launch(ops, c, xs, wp, kw, **extra).items()}
        for k in got:
            assert torch.equal(got[k], again[k]), f"{name}: {k} depends on what the workspaces held"


@pytest.mark.parametrize("name", [c.name for c in R.CASES if c.opt["dgrad"] or c.opt["llm"]] + ["h3-w28", "pair-grouped", "doubling"])
def test_packed_lattice_weights_are_g_w_bit_for_bit(ops, name):
    """mode 2, mode 3 and pack_conv_weight_wfll on the lattice: the fp32 products with 1/6, 1/12, 1/24 round to the exact value"""
    c = R.CASE[name]
    w = R.lattice_case(name)[0]["w"]
    got = pack(ops, c, cu(w)).cpu()
    want = R.packed_ref_wfll(w, c.opt["ll_scale"]) if c.opt["llm"] else R.packed_ref(c, w)
    assert got.shape == want.shape
    assert bool((want * 2 == torch.round(want * 2)).all()), "G w is not on the half-integer lattice"
    assert torch.equal(got.double(), want), f"{name}: {int((got.double() != want).sum())} packed weights differ from G w"


ROUNDING = [c.name for c in R.CASES if c.rounding]


def _direct(ops, c, t):
    """the direct kernel on the same inputs (a fold as its two-launch form); None where it refuses the launch"""
    o = c.opt
    kw = dict(bias=cu(t["bias"]), bias_scale=o["bias_scale"], residual=cu(t["res"]), out_scale=o["out_scale"], keep_y=o["keep_y"])
    if o["y2"] is not None:
        kw["emit"] = dict(act=o["y2"]["act"], shift=cu(t["sh2"]), scale=cu(t["sc2"]))
    try:
        if o["rc"]:
            kw["residual"] = ops.conv3d([cu(t["rc_x"])], ops.pack_conv_weight(cu(t["rc_w"])), c.cout, 1, bias=cu(t["bias"]))
            kw["bias"] = None
        out = ops.conv3d([cu(x) for x in t["xs"]], ops.pack_conv_weight(cu(t["w"]), groups=c.groups), c.cout, 3, groups=c.groups, **kw)
    except (ValueError, RuntimeError):
        return None
    out = out if isinstance(out, (tuple, list)) else (out,)
    return dict(zip(R.outputs_of(c), out))


def _err(got, ref):
    return max(float((got[k].double().cpu() - ref[k]).abs().max() / ref[k].abs().max()) for k in ref)


@pytest.mark.parametrize("name", ROUNDING)
def test_rounding_on_normal_data(ops, name):
    c = R.CASE[name]
    assert not (c.opt["ll"] or c.opt["dwt"] or c.opt["s2d"] or c.opt["llm"] or c.opt["dgrad"] or c.opt["pro"])
    t, ref = R.real_case(name)
    got = launch(ops, c, *device_case(name, "real"))
    e_wf = _err(got, ref)
    was = _direct(ops, c, t)
    torch.cuda.synchronize()
    e_was = "refused" if was is None else f"{_err(was, ref):.3e}"
    print(f"wf edges error [{name}]: conv3d_wf {e_wf:.3e}  conv3d (direct) {e_was}")
    assert e_wf <= BOUND, (name, e_wf)


def test_refusals_launch_nothing(ops):
    """Each raises ValueError before the library is asked to run (test_conv3d_wf_refs_host.py asks the same of the library's
    queries and the routing rules without a GPU); the packed weights are zeros of the full size."""
    z = lambda *s: torch.zeros(*s, device="cuda")

    def plain(b=2, cin=2, cout=32, n=8, h=8, w=16, groups=1):
        return [z(b, cin, n, h, w)], z(54 * cin // groups * cout), cout

    em = dict(act=True, shift=z(2, 32), scale=z(2, 32))
    fold = lambda b, n, h, w, rc=32: (z(b, rc, n, h, w), z(32, rc, 1, 1, 1), rc)
    calls = {
        "a fold next to a residual": (plain(), dict(residual=z(2, 32, 8, 8, 16), res_conv=fold(2, 8, 8, 16))),
        "a fold in pair mode": (plain(w=8), dict(res_conv=fold(2, 8, 8, 8))),
        "a fold of 48 channels": (plain(), dict(res_conv=fold(2, 8, 8, 16, 48))),
        "a fold of 544 channels": (plain(), dict(res_conv=fold(2, 8, 8, 16, 544))),
        "LL on a split grid": (plain(b=1, cin=8), dict(emit=dict(em, ll=True), keep_y=False)),
        "Haar on a split grid": (plain(b=1, cin=8), dict(emit=dict(em, dwt=True), keep_y=False)),
        "LL on pair planes": (plain(w=8), dict(emit=dict(em, ll=True), keep_y=False)),
        "Haar on pair planes": (plain(w=8), dict(emit=dict(em, dwt=True), keep_y=False)),
        "LL on odd H": (plain(h=7), dict(emit=dict(em, ll=True), keep_y=False)),
        "Haar on odd H": (plain(h=7), dict(emit=dict(em, dwt=True), keep_y=False)),
        "LL on 4 bands": (plain(n=4), dict(emit=dict(em, ll=True), keep_y=False)),
        "LL beside y": (plain(), dict(emit=dict(em, ll=True))),
        "s2d on a split grid": (plain(b=1, cin=8), dict(emit=dict(em, s2d=True))),
        "s2d on odd H": (plain(h=7), dict(emit=dict(em, s2d=True))),
        "N = 6": (plain(n=6), {}), "W = 6": (plain(w=6), {}), "an odd Cin": (plain(cin=3), {}),
        "an odd Cin / groups": (plain(cin=9, cout=96, groups=3), dict(groups=3)),
    }
    keep, ops.COUNTS = ops.COUNTS, collections.Counter()
    try:
        for what, ((xs, wp, cout), kw) in calls.items():
            with pytest.raises(ValueError):
                ops.conv3d_wf(xs, wp, cout, **kw)
                pytest.fail(f"conv3d_wf took: {what}")
        counts = dict(ops.COUNTS)
    finally:
        ops.COUNTS = keep
    assert counts == {}, counts
