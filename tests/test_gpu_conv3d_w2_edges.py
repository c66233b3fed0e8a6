"""conv3d_w2 (csrc/conv3d_w2.hip) on the paths test_gpu_conv3d_w2.py and test_gpu_conv3d_w2_epilogue.py never run: a last GEMM
tile with fewer images than G (lanes that fall back to position 0, stores that go outside, DMA pieces that read past the
tile's images), an odd number of rows, the 32 x 16 plane, seven column pairs, one column pair, Cin = 160 / 256 / 512, Cout = 320,
B = 1 / 3 / 5, every one-row output template, bank rows shared over the batch, bias_scale, prologues with and without SiLU, folds
of 32 / 96 / 512 channels, a fold on 4 bands, quarter outputs on a partial tile and at the largest plane
(conv3d_w2_refs.CASES; test_conv3d_w2_refs_host.py asserts what each case reaches), a poisoned and a stale scratch, what the
entry point refuses, and the `stages` mask.  Every call goes through ops.conv3d_w2; ops.COUNTS shows conv3d_w2_fwd alone.

Exact tier.  On lattice inputs (x integers in [-2, 2], w = 48 j, integer bias / residual / shifts, power-of-two scales; no SiLU
in the prologue) no fp32 operation of the three passes rounds (conv3d_w2_refs.exactness_ok, proved on the host), so every
output must EQUAL the fp64 reference, bit for bit: one lost, doubled or misplaced term is an error of at least 12 * 0.25,
whatever the sizes.  Outputs that went through SiLU (y2, LL' of the Haar form) are compared at the 2e-6 / 1e-6 of the Haar
test, the fp64 reference supplying the argument; everything else in that launch stays exact.  Each case runs on a scratch
filled with NaN and again after a launch of the largest case (stale finite values): same bits.

Rounding tier.  On normal data, the cases marked R: maximum error over the maximum of the fp64 reference, as
test_gpu_conv3d_w2.py judges.  Measured on the MI355X (profiles/wino2d_edges.txt; the kernel that served the shape before, on
the same inputs, for information):
    case             conv3d_w2    before
    partial-tile     3.153e-06    conv3d (direct) 1.022e-06
    cin160-cout320   3.126e-06    conv3d_wf       9.389e-07
    cin256           2.715e-06    conv3d_wf       6.667e-07
    cin512           5.674e-06    conv3d_wf       1.303e-06
    rc512-min        1.892e-06    conv3d (direct) 2.628e-07
BOUND = 2 x the worst conv3d_w2 figure (5.674e-6, Cin = 512), rounded up, under the 2e-5 ceiling of the Winograd forward
kernels.  No case measures above 1e-5; Cin = 512 has 1.8 times the error of Cin = 128 for a sum four times as long (K = 3 Cin
products per plane, added in sequence: square-root growth).
"""
import collections
import functools

import pytest
import torch

import conv3d_w2_refs as R
from conftest import rel_err

pytestmark = pytest.mark.gpu

BOUND = 1.2e-5     # 2 x 5.674e-6 (profiles/wino2d_edges.txt), rounded up; the ceiling is 2e-5
assert BOUND <= 2e-5
NAN = float("nan")
LARGEST = max(R.CASES, key=lambda c: R.case_plan(c).workspace_bytes).name


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from tmdiff_amd import ops as _ops
    return _ops


def cu(t):
    return None if t is None else t.cuda().contiguous()


def _stride(v):
    """a [C] row is a bank of one row shared over the batch (stride < 0 -> 0)"""
    return -1 if v is not None and v.dim() == 1 else 0


def launch_kw(ops, c, t):
    """(x, packed weights, keywords of ops.conv3d_w2) for a case on the CPU tensors t"""
    e = c.epi
    kw = dict(bias=cu(t["bias"]), bias_scale=e["bias_scale"], residual=cu(t["res"]), out_scale=e["out_scale"], keep_y=e["keep_y"])
    if e["pro"] is not None:
        kw.update(in_shift=cu(t["sh"]), in_scale=cu(t["sc"]), in_act=t["pro_act"], shift_stride=_stride(t["sh"]),
                  scale_stride=_stride(t["sc"]))
    if e["y2"] is not None:
        kw["emit"] = dict(act=e["y2"]["act"], shift=cu(t["sh2"]), scale=cu(t["sc2"]), shift_stride=_stride(t["sh2"]),
                          scale_stride=_stride(t["sc2"]), s2d=e["s2d"], ll=e["ll"], dwt=e["dwt"])
    if e["rc"]:
        kw["res_conv"] = (cu(t["rc_x"]), cu(t["rc_w"]), e["rc"])
    return cu(t["x"]), ops.pack_conv_weight_w2(cu(t["w"])), kw


def launch(ops, c, x, wp, kw, stages=0):
    """One ops.conv3d_w2 launch: {output name: device tensor}; COUNTS shows conv3d_w2_fwd alone"""
    keep, ops.COUNTS = ops.COUNTS, collections.Counter()
    try:
        out = ops.conv3d_w2(x, wp, c.cout, stages=stages, **kw)
        counts = dict(ops.COUNTS)
    finally:
        ops.COUNTS = keep
    assert counts == {"conv3d_w2_fwd": 1}, counts
    out = out if isinstance(out, (tuple, list)) else (out,)
    names = R.outputs_of(c)
    assert len(out) == len(names)
    return dict(zip(names, out))


@functools.lru_cache(maxsize=None)
def device_case(name, kind):
    """the device tensors of a case's lattice / real inputs, made once"""
    from tmdiff_amd import ops as _ops
    c = R.CASE[name]
    t = (R.lattice_case if kind == "lattice" else R.real_case)(name)[0]
    return launch_kw(_ops, c, t)


def scratch(ops, c):
    """the float32 view of the whole per-stream scratch "w2", at least the case's workspace"""
    nbytes = R.case_plan(c).workspace_bytes
    ws = ops._workspace(torch.device("cuda", torch.cuda.current_device()), nbytes, "w2")
    return ws[:ws.numel() // 4 * 4].view(torch.float32)


@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_exact_on_lattice_inputs_whatever_the_scratch_holds(ops, name):
    c = R.CASE[name]
    _, ref = R.lattice_case(name)
    x, wp, kw = device_case(name, "lattice")
    scratch(ops, c).fill_(NAN)
    got = {k: v.cpu() for k, v in launch(ops, c, x, wp, kw).items()}
    big = R.CASE[LARGEST]
    launch(ops, big, *device_case(LARGEST, "lattice"))                 # leaves its x^ and m^ behind: stale finite values
    assert scratch(ops, c).numel() * 4 >= R.case_plan(big).workspace_bytes
    again = {k: v.cpu() for k, v in launch(ops, c, x, wp, kw).items()}
    silu = R.silu_outputs(c)
    for k in R.outputs_of(c):
        want = ref[k]
        assert got[k].shape == want.shape, (k, got[k].shape, want.shape)
        assert not bool(torch.isnan(got[k]).any()), f"{name}: {k} holds NaN from the poisoned scratch"
        if k in silu:
            m, l2 = rel_err(got[k], want)
            print(f"conv3d_w2 edges [{name}] {k} (SiLU): max-rel {m:.3e} rel-L2 {l2:.3e}")
            assert m <= 2e-6 and l2 <= 1e-6, (name, k, m, l2)
        else:
            bad = got[k].double() != want
            assert not bool(bad.any()), (f"{name}: {k} differs from the fp64 reference in {int(bad.sum())} of {bad.numel()} elements, "
                                         f"first at {tuple(bad.nonzero()[0].tolist())}, largest {float((got[k].double() - want).abs().max())}")
            assert torch.equal(got[k], want.float())
        assert torch.equal(got[k], again[k]), f"{name}: {k} depends on what the scratch held"


ROUNDING = [c.name for c in R.CASES if c.rounding]


def _before(ops, c, t):
    """The kernel that served the shape before conv3d_w2 on the same inputs: conv3d_wf where W % 4 == 0, else the direct kernel;
    a fold as its two-launch form where that kernel does not fold.  None where it refuses the launch."""
    e = c.epi
    x, w = cu(t["x"]), cu(t["w"])
    kw = dict(bias=cu(t["bias"]), bias_scale=e["bias_scale"], residual=cu(t["res"]), out_scale=e["out_scale"], keep_y=e["keep_y"])
    if e["pro"] is not None:
        kw.update(in_shift=cu(t["sh"]), in_scale=cu(t["sc"]), in_act=t["pro_act"], shift_stride=_stride(t["sh"]),
                  scale_stride=_stride(t["sc"]))
    if e["y2"] is not None:
        kw["emit"] = dict(act=e["y2"]["act"], shift=cu(t["sh2"]), scale=cu(t["sc2"]), shift_stride=_stride(t["sh2"]),
                          scale_stride=_stride(t["sc2"]))
    if e["rc"]:
        kw["residual"] = ops.conv3d([cu(t["rc_x"])], ops.pack_conv_weight(cu(t["rc_w"])), c.cout, 1, bias=cu(t["bias"]))
        kw["bias"] = None
    try:
        if c.W % 4 == 0:
            out = ops.conv3d_wf([x], ops.pack_conv_weight_wino(w, mode=2, planes=6), c.cout, **kw)
        else:
            out = ops.conv3d([x], ops.pack_conv_weight(w), c.cout, 3, **kw)
    except (ValueError, RuntimeError):
        return None
    out = out if isinstance(out, (tuple, list)) else (out,)
    return dict(zip(R.outputs_of(c), out))


def _err(got, ref):
    return max(float((got[k].double().cpu() - ref[k]).abs().max() / ref[k].abs().max()) for k in ref)


@pytest.mark.parametrize("name", ROUNDING)
def test_rounding_on_normal_data(ops, name):
    c = R.CASE[name]
    assert not (c.epi["ll"] or c.epi["dwt"] or c.epi["s2d"])            # (the kernels before write none of these here)
    t, ref = R.real_case(name)
    got = launch(ops, c, *device_case(name, "real"))
    e_w2 = _err(got, ref)
    was = _before(ops, c, t)
    torch.cuda.synchronize()
    e_was = "refused" if was is None else f"{_err(was, ref):.3e}"
    print(f"wino2d edges error [{name}]: conv3d_w2 {e_w2:.3e}  {'conv3d_wf' if c.W % 4 == 0 else 'conv3d (direct)'} {e_was}")
    assert e_w2 <= BOUND, (name, e_w2)


def _plain(b=2, cin=128, cout=256, n=8, h=8, w=8):
    return torch.zeros(b, cin, n, h, w, device="cuda"), torch.zeros(72 * cout * cin, device="cuda"), cout


def test_refusals_launch_nothing(ops):
    """Each raises ValueError before the library is asked to run (test_conv3d_w2_refs_host.py asks the same of the mirrors
    and the library's queries without a GPU); the packed weights are zeros of the full size."""
    z = lambda *s: torch.zeros(*s, device="cuda")
    em = dict(act=True, shift=z(2, 256), scale=z(2, 256))
    calls = {
        "H = 3": (_plain(h=3), {}), "H = 33": (_plain(h=33), {}), "W = 18": (_plain(w=18), {}), "odd W": (_plain(w=7), {}),
        "Cin = 96": (_plain(cin=96), {}), "Cin = 144": (_plain(cin=144), {}),
        "Cout = 192": (_plain(cout=192), {}), "Cout = 288": (_plain(cout=288), {}), "N = 6": (_plain(n=6), {}),
        "odd H with a fold": (_plain(h=7), dict(res_conv=(z(2, 32, 8, 7, 8), z(256, 32, 1, 1, 1), 32))),
        "odd H with an LL output": (_plain(h=7), dict(emit=dict(em, ll=True), keep_y=False)),
        "rc_cin = 48": (_plain(), dict(res_conv=(z(2, 48, 8, 8, 8), z(256, 48, 1, 1, 1), 48))),
        "rc_cin = 544": (_plain(), dict(res_conv=(z(2, 544, 8, 8, 8), z(256, 544, 1, 1, 1), 544))),
        "residual beside res_conv": (_plain(), dict(residual=z(2, 256, 8, 8, 8), res_conv=(z(2, 32, 8, 8, 8), z(256, 32, 1, 1, 1), 32))),
        "LL on 4 bands": (_plain(n=4), dict(emit=dict(em, ll=True), keep_y=False)),
        "space-to-depth on 4 bands": (_plain(n=4), dict(emit=dict(em, s2d=True))),
        "Haar on 4 bands": (_plain(n=4), dict(emit=dict(em, dwt=True), keep_y=False)),
        "a mask": (_plain(), dict(in_mask=z(2, 128, 8, 8, 8))),
        "dropout": (_plain(), dict(drop=(1234, 0.1))),
    }
    keep, ops.COUNTS = ops.COUNTS, collections.Counter()
    try:
        for what, ((x, wp, cout), kw) in calls.items():
            with pytest.raises(ValueError):
                ops.conv3d_w2(x, wp, cout, **kw)
                pytest.fail(f"conv3d_w2 took: {what}")
        counts = dict(ops.COUNTS)
    finally:
        ops.COUNTS = keep
    assert counts == {}, counts


@pytest.mark.parametrize("name", ["partial-tile", "rc96-partial"])
def test_the_stages_mask_runs_the_three_launches_one_by_one(ops, name):
    """stages = 1, then 2, then 4 on the same scratch: the bits of stages = 0 (the output pass alone writes the outputs)."""
    c = R.CASE[name]
    x, wp, kw = device_case(name, "lattice")
    whole = launch(ops, c, x, wp, kw)
    scratch(ops, c).fill_(NAN)
    launch(ops, c, x, wp, kw, stages=1)
    launch(ops, c, x, wp, kw, stages=2)
    parts = launch(ops, c, x, wp, kw, stages=4)
    for k in whole:
        assert torch.equal(whole[k], parts[k]), (name, k)
