"""GPU tests of the elementwise kernels of csrc/sampler.hip (DDPM step with host and device scalars, sampler tick, axpby,
multi-tensor axpby, x0 prediction, add, q_sample) and of the one-launch AdamW on unaligned tensors, at the sizes where each
kernel changes path: the scalar and the 16-byte instantiations, one misaligned operand, the grid-stride loop past the cap of
2048 workgroups, the frame stack, more samples than one workgroup, the chunk tail of the multi-tensor kernels.

Every result is compared with the fp64 statement of tests/sampler_refs.py (|got - ref| <= r 2^-24 M; r and M per
kernel in that file and in each docstring here) and, where the kernel is +, -, * only, bit for bit with the fp32 restatement
evaluated by torch on the device (axpby: with its fma statement).  Outputs are filled with NaN and sit between sentinels in one allocation, so a dropped or a
misplaced store fails even where the kernel would have written the right value."""
import ctypes as C

import pytest
import torch

from sampler_refs import (AXPBY_COEFS, DDPM_LATE, DDPM_MID, DDPM_ROWS, DDPM_TABLE, EMA_COEFS, Q_A, R, X0_COEFS,
                         add_ref64, add_restate, add_terms, axpby_fused_restate, axpby_ref64, axpby_restate,
                         axpby_terms, ddpm_ref64, ddpm_restate, ddpm_terms, f32, frame_count_ref, frame_slot_ref,
                         make_inputs, q_ref64, q_sb, q_terms, same_bits, units, x0_ref64, x0_terms, SMALL)

pytestmark = pytest.mark.gpu

FRONT, GUARD = 4, 64              # sentinel floats in front of (4, or 5 for a misaligned view) and after every tensor
SENTINEL = 12345.0
CAP_VEC = 2 * 2048 * 256 * 4 + 1028            # two full sweeps of the capped grid and a ragged third, 16 bytes per lane
CAP_SCALAR = 2 * 2048 * 256 + 3                # the same for the scalar kernel (n % 4 != 0 takes it)
WORST = {}                                     # kernel -> worst error seen, in units of 2^-24 M


@pytest.fixture(scope="module")
def ops():
    from tmdiff_amd import ops
    yield ops
    torch.cuda.synchronize()
    for name in sorted(WORST):
        print(f"\nWORST {name}: {WORST[name]:.3f} units of 2^-24 M")


class G:
    """A float tensor of n elements inside one allocation: FRONT (+ off) sentinels, the tensor, GUARD sentinels.  off = 0: the
    tensor is 16-byte aligned; off = 1: it starts one float past a 16-byte boundary."""

    def __init__(self, n, off=0, values=None, dtype=torch.float32):
        self.lo = FRONT + off
        self.buf = torch.full((self.lo + n + GUARD,), SENTINEL, device="cuda", dtype=dtype)
        self.t = self.buf[self.lo:self.lo + n]
        if values is None:
            self.t.fill_(float("nan"))
        else:
            self.t.copy_(values.reshape(-1))
        assert self.t.data_ptr() % 16 == 4 * off and self.t.is_contiguous()

    def check(self, what=""):
        assert bool((self.buf[:self.lo] == SENTINEL).all()), f"{what}: a store landed in front of the tensor"
        assert bool((self.buf[self.lo + self.t.numel():] == SENTINEL).all()), f"{what}: a store landed past the end of the tensor"


def put(v, off=0):
    return G(v.numel(), off, v.cuda())


def within(name, got, ref, terms, r, what=""):
    assert not bool(torch.isnan(got).any()), f"{name} {what}: an element was never written (NaN left)"
    w = units(got, ref, terms)
    WORST[name] = max(WORST.get(name, 0.0), w)
    assert w <= r, f"{name} {what}: {w:.3f} units of 2^-24 M, bound r = {r}"


def refused(ops, status):
    from tmdiff_amd._lib import TmdiffError
    with pytest.raises(TmdiffError):
        ops.check(status, "refusal")


def ddpm_inputs(n, seed=11):
    return [v.cuda() for v in make_inputs(n, seed, 4)]            # x, eps, noise, ms


def kf(k):
    return [float(c) for c in k]


# ---- ddpm_step ---------------------------------------------------------------------------------------------------------------
def run_ddpm(ops, vals, k, clip=True, noise=True, img=True, offs=None):
    """ddpm_step on fresh guarded tensors; offs: operand name -> 1 to misalign it.  Returns (out, img or None), guards checked."""
    offs = offs or {}
    x, e, nz, ms = (put(v, offs.get(name, 0)) for v, name in zip(vals, ("x", "eps", "noise", "ms")))
    n = vals[0].numel()
    out, im = G(n, offs.get("out", 0)), G(n, offs.get("img_out", 0)) if img else None
    ops.ddpm_step(x.t, e.t, nz.t if noise else None, *kf(k), clip=clip, ms=ms.t if img else None, out=out.t,
                  img_out=im.t if img else None)
    torch.cuda.synchronize()
    for g in (x, e, nz, ms, out) + ((im,) if img else ()):
        g.check("ddpm_step")
    return out.t, im.t if img else None


def check_ddpm(vals, k, clip, noise, out, im, what):
    x, e, nz, ms = vals
    nz = nz if noise else None
    within("ddpm_step", out, ddpm_ref64(x, e, nz, k, clip), ddpm_terms(x, e, nz, k), R["ddpm"], what)
    want = ddpm_restate(x, e, nz, k, clip)
    assert same_bits(out, want), f"ddpm_step {what}: differs from the fp32 restatement in {int((out != want).sum())} elements"
    if im is not None:
        assert same_bits(im, want + ms), f"ddpm_step {what}: img_out is not out + ms"


@pytest.mark.parametrize("n", SMALL)
def test_ddpm_step_sizes_clip_noise_and_image(ops, n):
    """r = 8, M = |c1| (|a x| + |b e|) + |c2 x| + |sigma nz|.  n % 4 == 0 runs the 16-byte kernel, every other n the scalar one;
    clip on and off with rows that leave x0 far outside [-1, 1]; sigma = 0 without noise; with and without ms / img_out."""
    vals = ddpm_inputs(n)
    for row, k in sorted(DDPM_ROWS.items()):
        for clip in (True, False):
            for noise in ((True, False) if float(k[4]) == 0.0 else (True,)):
                for img in (True, False):
                    out, im = run_ddpm(ops, vals, k, clip, noise, img)
                    check_ddpm(vals, k, clip, noise, out, im, f"n={n} row={row} clip={clip} noise={noise} img={img}")
    if n >= 12:
        x0 = DDPM_LATE[0].cuda() * vals[0] - DDPM_LATE[1].cuda() * vals[1]
        assert float(x0[12:].abs().max()) > 10.0                    # the clamp has work to do
        assert not same_bits(run_ddpm(ops, vals, DDPM_LATE, True)[0], run_ddpm(ops, vals, DDPM_LATE, False)[0])


@pytest.mark.parametrize("which", ["x", "eps", "noise", "ms", "out", "img_out"])
def test_ddpm_step_one_misaligned_operand_takes_the_scalar_kernel(ops, which):
    vals = ddpm_inputs(1024)
    for k, clip in ((DDPM_MID, True), (DDPM_LATE, False)):
        base = run_ddpm(ops, vals, k, clip)
        got = run_ddpm(ops, vals, k, clip, offs={which: 1})
        assert same_bits(got[0], base[0]) and same_bits(got[1], base[1]), which
        check_ddpm(vals, k, clip, True, got[0], got[1], f"{which} misaligned")


@pytest.mark.parametrize("n", [CAP_VEC, CAP_SCALAR], ids=["vector", "scalar"])
def test_ddpm_step_past_the_grid_cap(ops, n):
    vals = ddpm_inputs(n, 12)
    out, im = run_ddpm(ops, vals, DDPM_MID, True)
    check_ddpm(vals, DDPM_MID, True, True, out, im, f"n={n}")


def test_ddpm_step_refusals_and_empty(ops):
    x, e = put(torch.ones(8)), put(torch.ones(8))
    out, im = G(8), G(8)
    L, st = ops.lib, ops.stream_ptr()
    p = lambda g: g.t.data_ptr()
    refused(ops, L.tmdiff_ddpm_step(p(x), p(e), None, None, p(out), None, 8, 1.0, 0.5, 0.5, 0.5, 0.25, 1, st))   # sigma != 0
    refused(ops, L.tmdiff_ddpm_step(p(x), p(e), p(e), None, p(out), p(im), 8, 1.0, 0.5, 0.5, 0.5, 0.25, 1, st))  # img, no ms
    ops.check(L.tmdiff_ddpm_step(p(x), p(e), p(e), p(e), p(out), p(im), 0, 1.0, 0.5, 0.5, 0.5, 0.25, 1, st), "n = 0")
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.t).all()) and bool(torch.isnan(im.t).all())
    for g in (out, im):
        g.check("refused / empty ddpm_step")


# ---- ddpm_step_dev -------------------------------------------------------------------------------------------------------------
T = len(DDPM_TABLE)


def table():
    return torch.stack([torch.stack(list(row)) for row in DDPM_TABLE]).cuda().contiguous()


def step_word(t):
    return torch.tensor([t], dtype=torch.int32, device="cuda")


def run_dev(ops, vals, t, in_place=False, frames=None, frame_every=1, clip=True, offs=None, nan_noise=False, ms=True):
    offs = offs or {}
    x, e, nz, m = (put(v, offs.get(name, 0)) for v, name in zip(vals, ("x", "eps", "noise", "ms")))
    if nan_noise:
        nz.t.fill_(float("nan"))
    out = x if in_place else G(vals[0].numel(), offs.get("out", 0))
    ops.ddpm_step_dev(x.t, e.t, nz.t, step_word(t), table(), ms=m.t if ms else None, out=out.t, frames=frames,
                      frame_every=frame_every, clip=clip)
    torch.cuda.synchronize()
    for g in (x, e, nz, m, out):
        g.check("ddpm_step_dev")
    return out.t


@pytest.mark.parametrize("n", SMALL + (1027,))
def test_ddpm_step_dev_is_ddpm_step_of_row_t(ops, n):
    """For every t the device-scalar step equals ddpm_step with row t's five values bit for bit (one body), out of place and
    in place; at t = 0 (sigma = 0) the noise is all NaN and must not be read."""
    vals = ddpm_inputs(n, 13)
    for t in range(T):
        k = DDPM_TABLE[t]
        for clip in (True, False):
            want, _ = run_ddpm(ops, vals, k, clip, noise=t > 0, img=False)
            check_ddpm(vals, k, clip, t > 0, want, None, f"row {t}")
            for in_place in (False, True):
                got = run_dev(ops, vals, t, in_place, clip=clip, nan_noise=t == 0, ms=False)
                assert bool(torch.isfinite(got).all()), f"t={t}: the noise was read"
                assert same_bits(got, want), f"t={t} clip={clip} in_place={in_place}"


@pytest.mark.parametrize("which", ["x", "eps", "noise", "ms", "out", "frames"])
def test_ddpm_step_dev_one_misaligned_operand(ops, which):
    n, t = 1024, 2
    vals = ddpm_inputs(n, 14)
    want, _ = run_ddpm(ops, vals, DDPM_TABLE[t], True, img=False)
    slots = frame_count_ref(T, 1)
    fr = G(slots * n, 1 if which == "frames" else 0)
    got = run_dev(ops, vals, t, frames=fr.t.view(slots, n), offs={which: 1})
    fr.check("frames")
    assert same_bits(got, want), which
    assert same_bits(fr.t.view(slots, n)[frame_slot_ref(t, T, 1)], want + vals[3]), which


@pytest.mark.parametrize("t", [-1, T])
def test_ddpm_step_dev_out_of_range_step_is_a_no_op(ops, t):
    for n in (1028, 1027):
        vals = ddpm_inputs(n, 15)
        slots = frame_count_ref(T, 1)
        marks = torch.randn(n + slots * n).cuda()
        out, fr = put(marks[:n]), put(marks[n:])
        x, e, nz, ms = (put(v) for v in vals)
        ops.ddpm_step_dev(x.t, e.t, nz.t, step_word(t), table(), ms=ms.t, out=out.t, frames=fr.t.view(slots, n), frame_every=1)
        torch.cuda.synchronize()
        assert same_bits(out.t, marks[:n]) and same_bits(fr.t, marks[n:]), "an out-of-range step wrote"
        out.check()
        fr.check()


@pytest.mark.parametrize("n", [1028, 1027], ids=["vector", "scalar"])
@pytest.mark.parametrize("every", [1, 2, 3])
def test_ddpm_step_dev_fills_exactly_its_frame_slot(ops, n, every):
    """Step t writes out + ms into the slot p_sample_loop would append it to (frame_slot_ref walks that loop; the export
    tmdiff_ddpm_frame_slot must name the same slot) and into no other; a step with t % every != 0 writes no frame."""
    vals = ddpm_inputs(n, 16)
    slots = frame_count_ref(T, every)
    for t in range(T):
        fr = G(slots * n)
        frames = fr.t.view(slots, n)
        got = run_dev(ops, vals, t, frames=frames, frame_every=every)
        fr.check("frames")
        want, _ = run_ddpm(ops, vals, DDPM_TABLE[t], True, noise=t > 0, img=False)
        assert same_bits(got, want)
        slot = frame_slot_ref(t, T, every)
        if slot is not None:
            assert ops.lib.tmdiff_ddpm_frame_slot(t, T, every) == slot
        for s in range(slots):
            if s == slot:
                assert same_bits(frames[s], want + vals[3]), f"t={t} every={every}: slot {s} is not out + ms"
            else:
                assert bool(torch.isnan(frames[s]).all()), f"t={t} every={every}: slot {s} was written (the step's slot is {slot})"


def test_ddpm_step_dev_without_frames_and_refusals(ops):
    vals = ddpm_inputs(1028, 17)
    want, _ = run_ddpm(ops, vals, DDPM_TABLE[3], True, img=False)
    assert same_bits(run_dev(ops, vals, 3, frames=None), want)
    assert same_bits(run_dev(ops, vals, 3, frames=None, ms=False), want)
    x, e, nz, ms = (put(v) for v in vals)
    out, fr = G(1028), G(frame_count_ref(T, 1) * 1028)
    L, st, p = ops.lib, ops.stream_ptr(), (lambda g: g.t.data_ptr())
    tab, word = table(), step_word(3)
    args = lambda ms_, every: (p(x), p(e), p(nz), ms_, p(out), p(fr), 1028, word.data_ptr(), tab.data_ptr(), T, every, 1, st)
    refused(ops, L.tmdiff_ddpm_step_dev(*args(None, 1)))           # frames without ms
    refused(ops, L.tmdiff_ddpm_step_dev(*args(p(ms), 0)))          # frames with frame_every = 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.t).all()) and bool(torch.isnan(fr.t).all())


# ---- sampler_tick --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [0, 1, 63, 64, 65, 255, 256, 257, 600])
def test_sampler_tick(ops, B):
    """One workgroup of 256 lanes walks the B samples: past one wave (64) and past the workgroup (256) the loop must go on."""
    for start, set_to, want_step, want_time in ((3, 7, 7, 8.0), (3, -1, 2, 3.0), (0, -1, -1, 0.0), (-1, 0, 0, 1.0)):
        step, tm = step_word(start), G(B)
        ops.sampler_tick(step, tm.t.view(B, 1), set_to)
        torch.cuda.synchronize()
        assert int(step) == want_step, (start, set_to)
        assert bool((tm.t == want_time).all()), (B, start, set_to, tm.t[:4])
        tm.check("time_in")
    step = step_word(3)
    if B == 0:
        ops.sampler_tick(step, None, -1)
        assert int(step) == 2


# ---- axpby -------------------------------------------------------------------------------------------------------------------
def run_axpby(ops, vs, k, offs=None):
    offs = offs or {}
    ins = [put(v, offs.get(i, 0)) for i, v in enumerate(vs)]
    out = G(vs[0].numel(), offs.get("out", 0))
    ops.axpby([g.t for g in ins], kf(k), out=out.t)
    torch.cuda.synchronize()
    for g in ins + [out]:
        g.check("axpby")
    return out.t


def check_axpby(vs, k, got, what):
    within("axpby", got, axpby_ref64(vs, k), axpby_terms(vs, k), R["axpby"](len(vs)), what)
    assert same_bits(got, axpby_fused_restate(vs, k)), f"axpby {what}: not fma(c3, v3, fma(c2, v2, fma(c1, v1, c0 v0)))"
    if len(vs) > 1:
        assert not same_bits(got, axpby_restate(vs, k)) or vs[0].numel() < 64      # (the fma is not mul, add: see axpby_kernel)


@pytest.mark.parametrize("n_in", [1, 2, 3, 4])
def test_axpby_sizes_and_misaligned_operands(ops, n_in):
    """r = 2 n_in - 1, M = sum |c_k v_k|; accumulation order ((c0 v0 + c1 v1) + c2 v2) + c3 v3 (each sum fused with its product)."""
    k = AXPBY_COEFS[:n_in]
    for n in SMALL:
        vs = [v.cuda() for v in make_inputs(n, 21, n_in)]
        check_axpby(vs, k, run_axpby(ops, vs, k), f"n_in={n_in} n={n}")
    vs = [v.cuda() for v in make_inputs(1024, 22, n_in)]
    base = run_axpby(ops, vs, k)
    for which in list(range(n_in)) + ["out"]:
        got = run_axpby(ops, vs, k, {which: 1})
        assert same_bits(got, base), which
        check_axpby(vs, k, got, f"n_in={n_in} operand {which} misaligned")


@pytest.mark.parametrize("n", [CAP_VEC, CAP_SCALAR], ids=["vector", "scalar"])
def test_axpby_past_the_grid_cap(ops, n):
    vs = [v.cuda() for v in make_inputs(n, 23, 4)]
    check_axpby(vs, AXPBY_COEFS, run_axpby(ops, vs, AXPBY_COEFS), f"n={n}")


def test_axpby_refusals(ops):
    ins, out = [put(torch.ones(8)) for _ in range(4)], G(8)
    L, st = ops.lib, ops.stream_ptr()
    cf = (C.c_float * 4)(1.0, 1.0, 1.0, 1.0)
    ptrs = lambda *skip: (C.c_void_p * 4)(*[None if i in skip else g.t.data_ptr() for i, g in enumerate(ins)])
    refused(ops, L.tmdiff_axpby(ptrs(), cf, 0, out.t.data_ptr(), 8, st))
    refused(ops, L.tmdiff_axpby(ptrs(), cf, 5, out.t.data_ptr(), 8, st))
    refused(ops, L.tmdiff_axpby(ptrs(1), cf, 2, out.t.data_ptr(), 8, st))
    refused(ops, L.tmdiff_axpby(ptrs(2), cf, 4, out.t.data_ptr(), 8, st))
    ops.check(L.tmdiff_axpby(ptrs(2, 3), cf, 2, out.t.data_ptr(), 0, st), "n = 0")
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.t).all())
    out.check()


# ---- multi_axpby ---------------------------------------------------------------------------------------------------------------
def test_multi_axpby_chunk_tails_alignment_and_in_place(ops):
    """The EMA update, r = 3, M = |ca a| + |cb b|: one launch over tensors around the chunk of 16384 (a block's 16-byte loop,
    its tail of n % 4 elements, a second and a third chunk), aligned and with out / a / b in turn one float off, in place
    (out is a) and out of place; an empty tensor is dropped."""
    chunk = ops.lib.tmdiff_multi_axpby_chunk()
    assert chunk == 16384
    sizes = [1, 3, 4, 5, chunk - 1, chunk, chunk + 1, 2 * chunk + 7, 0, 4, 5, chunk + 1, 2 * chunk + 7, chunk, chunk - 1, 2 * chunk + 7]
    #        aligned ........................................ | one operand misaligned: (out, a, b) offsets
    offs = [(0, 0, 0)] * 9 + [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 0, 0), (0, 1, 0), (1, 1, 1), (0, 0, 1)]
    ca, cb = EMA_COEFS
    for in_place in (True, False):
        triples, keep = [], []
        for i, (n, (oo, oa, ob)) in enumerate(zip(sizes, offs)):
            a, b = (v.cuda() for v in make_inputs(n, 30 + i, 2))
            ga, gb = put(a, oo if in_place else oa), put(b, ob)
            go = ga if in_place else G(n, oo)
            triples.append((go.t, ga.t, gb.t))
            keep.append((a, b, go, ga, gb))
        m = ops.MultiAxpby(triples)
        assert m.n_chunks == sum((n + chunk - 1) // chunk for n in sizes) and len(m._keep) == len(sizes) - 1
        m.run(float(ca), float(cb))
        torch.cuda.synchronize()
        for i, (a, b, go, ga, gb) in enumerate(keep):
            what = f"tensor {i} ({sizes[i]} elements, offsets {offs[i]}, in_place={in_place})"
            for g in (go, ga, gb):
                g.check(what)
            if sizes[i] == 0:
                continue
            within("multi_axpby", go.t, axpby_ref64([a, b], EMA_COEFS), axpby_terms([a, b], EMA_COEFS), R["multi_axpby"], what)
            assert same_bits(go.t, axpby_restate([a, b], EMA_COEFS)), f"{what}: not ca a + cb b in fp32"
            assert same_bits(gb.t, b) and (in_place or same_bits(ga.t, a)), f"{what}: an input changed"


# ---- x0_from_model -------------------------------------------------------------------------------------------------------------
def run_x0(ops, x, m, k, is_x_start, offs=None):
    offs = offs or {}
    gx, gm, out = put(x, offs.get("x", 0)), put(m, offs.get("model_out", 0)), G(x.numel(), offs.get("out", 0))
    ops.x0_from_model(gx.t, gm.t, float(k[0]), float(k[1]), is_x_start, out=out.t)
    torch.cuda.synchronize()
    for g in (gx, gm, out):
        g.check("x0_from_model")
    return out.t


@pytest.mark.parametrize("k", X0_COEFS, ids=lambda k: f"alpha{float(k[0]):.4g}")
@pytest.mark.parametrize("is_x_start", [True, False], ids=["x_start", "noise"])
def test_x0_from_model(ops, k, is_x_start):
    """x_start mode: r = 6, M = (2 |x| + |alpha m|) / alpha; noise mode: r = 3, M = (|x| + |sigma m|) / alpha."""
    name = "x0_start" if is_x_start else "x0_noise"
    for n in SMALL:
        x, m = (v.cuda() for v in make_inputs(n, 41, 2))
        within(name, run_x0(ops, x, m, k, is_x_start), x0_ref64(x, m, k, is_x_start), x0_terms(x, m, k, is_x_start), R[name], f"n={n}")
    x, m = (v.cuda() for v in make_inputs(1024, 42, 2))
    base = run_x0(ops, x, m, k, is_x_start)
    for which in ("x", "model_out", "out"):
        got = run_x0(ops, x, m, k, is_x_start, {which: 1})
        assert same_bits(got, base), which
        within(name, got, x0_ref64(x, m, k, is_x_start), x0_terms(x, m, k, is_x_start), R[name], f"{which} misaligned")


# ---- add -----------------------------------------------------------------------------------------------------------------------
def run_add(ops, a, b, s, offs=None):
    offs = offs or {}
    ga, gb, out = put(a, offs.get("a", 0)), put(b, offs.get("b", 0)), G(a.numel(), offs.get("out", 0))
    ops.add(ga.t, gb.t, s, out=out.t)
    torch.cuda.synchronize()
    for g in (ga, gb, out):
        g.check("add")
    return out.t


def check_add(a, b, s, got, what):
    within("add", got, add_ref64(a, b, s), add_terms(a, b), R["add"], what)
    assert same_bits(got, add_restate(a, b, s)), f"add {what}"


@pytest.mark.parametrize("s", [1.0, -1.0])
def test_add_sizes_misaligned_operands_and_grid_cap(ops, s):
    """r = 1 (the product with +-1 is exact), M = |a| + |b|."""
    for n in SMALL + (CAP_VEC, CAP_SCALAR):
        a, b = (v.cuda() for v in make_inputs(n, 51, 2))
        check_add(a, b, s, run_add(ops, a, b, s), f"n={n}")
    a, b = (v.cuda() for v in make_inputs(1024, 52, 2))
    base = run_add(ops, a, b, s)
    for which in ("a", "b", "out"):
        got = run_add(ops, a, b, s, {which: 1})
        assert same_bits(got, base), which
        check_add(a, b, s, got, f"{which} misaligned")


# ---- q_sample ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_per", [1, 255, 257, 65536 + 5, 3 * 65536 + 1])
@pytest.mark.parametrize("B", [1, 3])
def test_q_sample(ops, B, n_per):
    """r = 3, M = |a x0| + |sb nz| with sb = (1 - a a).sqrt() as torch forms it in fp32.  Past 65536 elements per sample the 256
    workgroups of a sample stride; a per sample walks through Q_A; x0 aligned and one float off."""
    first = {1: 0, 255: 1, 257: 3, 65536 + 5: 4, 3 * 65536 + 1: 5}[n_per] + (0 if B == 1 else 1)
    a = torch.tensor([Q_A[(first + 2 * i) % len(Q_A)] for i in range(B)], dtype=torch.float32).cuda()
    x0, nz = (v.cuda().view(B, n_per) for v in make_inputs(B * n_per, 61, 2))
    for off in (0, 1):
        gx, gn, out = put(x0, off), put(nz), G(B * n_per)
        ops.q_sample(gx.t.view(B, n_per), gn.t.view(B, n_per), a, out=out.t.view(B, n_per))
        torch.cuda.synchronize()
        for g in (gx, gn, out):
            g.check("q_sample")
        within("q_sample", out.t.view(B, n_per), q_ref64(x0, nz, a), q_terms(x0, nz, a), R["q_sample"], f"B={B} n_per={n_per} a={a.tolist()}")


def test_q_sample_sb_is_within_one_ulp_of_torch(ops):
    """x0 = 0, noise = 1: the output is the kernel's own sb, for every a of Q_A (two samples past the first workgroup row)."""
    a = torch.tensor(Q_A, dtype=torch.float32).cuda()
    B, n_per = len(Q_A), 300
    out = G(B * n_per)
    ops.q_sample(torch.zeros(B, n_per, device="cuda"), torch.ones(B, n_per, device="cuda"), a, out=out.t.view(B, n_per))
    torch.cuda.synchronize()
    out.check()
    got, want = out.t.view(B, n_per), q_sb(a)
    assert bool((got == got[:, :1]).all())
    ulps = (got[:, 0].contiguous().view(torch.int32) - want.view(torch.int32)).abs()
    print(f"\nSB kernel {got[:, 0].tolist()} torch {want.tolist()} ulps {ulps.tolist()} bit-equal {bool((ulps == 0).all())}")
    assert int(ulps.max()) <= 1, ulps.tolist()


# ---- FusedAdamW on unaligned tensors ---------------------------------------------------------------------------------------------
def test_fused_adamw_on_unaligned_views(ops):
    """Parameters, gradients and both moments as contiguous views one float into larger buffers (5 and 16385 elements) plus an
    aligned control: one plain step, one clipped step.  Against the fp64 formula above adamw_coef in csrc/sampler.hip with
    the measure and limit of test_fused_adamw_is_torch_adamw (max |x - y| / max |x| <= 2e-6 per tensor); the norm against fp64
    (<= 2^-23 relative, as test_norm_matches_fp64_on_the_host); guards around p, m, v, g; and the same values in aligned
    tensors give the same bits."""
    from tmdiff_amd.optim import FusedAdamW
    sizes, lr, wd, b1, b2, eps = (5, 16385, 16385), 1e-3, 1e-2, 0.9, 0.999, 1e-8
    layouts = {"views": (1, 1, 0), "aligned": (0, 0, 0)}
    p0 = [torch.randn(n, generator=torch.Generator().manual_seed(70 + i)) for i, n in enumerate(sizes)]
    grads = [[torch.randn(n, generator=torch.Generator().manual_seed(80 + 10 * s + i)) * (1.0 + 3.0 * s) for i, n in enumerate(sizes)]
             for s in range(2)]
    state = {}
    for name, offs in layouts.items():
        P = [put(v, o) for v, o in zip(p0, offs)]
        Gr = [put(torch.zeros(n), o) for n, o in zip(sizes, offs)]
        M = [put(torch.zeros(n), o) for n, o in zip(sizes, offs)]
        V = [put(torch.zeros(n), o) for n, o in zip(sizes, offs)]
        params = [torch.nn.Parameter(g.t) for g in P]
        for q, g in zip(params, P):
            assert q.data_ptr() == g.t.data_ptr()
        opt = FusedAdamW(params, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
        for q, gr, m, v in zip(params, Gr, M, V):
            q.grad = gr.t
            opt.state[q]["exp_avg"], opt.state[q]["exp_avg_sq"] = m.t, v.t
        norms = []
        for s in range(2):
            for gr, val in zip(Gr, grads[s]):
                gr.t.copy_(val)
            opt.max_grad_norm = None if s == 0 else 0.5 * float(torch.cat(grads[1]).double().norm())
            opt.step()
            torch.cuda.synchronize()
            for q, gr, m, v in zip(params, Gr, M, V):
                assert q.data_ptr() % 16 == gr.t.data_ptr() % 16 == m.t.data_ptr() % 16 == v.t.data_ptr() % 16
                assert opt.state[q]["exp_avg"].data_ptr() == m.t.data_ptr() and q.grad.data_ptr() == gr.t.data_ptr()
            if s == 1:
                norms.append(opt.last_grad_norm.clone())
                assert float(opt.last_step_ok) == 1.0 and 0.0 < float(opt.last_clip_coef) < 1.0
        for g in P + Gr + M + V:
            g.check(f"FusedAdamW ({name})")
        for gr, val in zip(Gr, grads[1]):
            assert same_bits(gr.t, val.cuda()), "the step wrote to a gradient"
        state[name] = ([g.t.clone() for g in P], [g.t.clone() for g in M], [g.t.clone() for g in V], norms[0], float(opt.max_grad_norm))
    # fp64: p *= 1 - lr wd; m += (1 - b1) (g - m); v = b2 v + (1 - b2) g^2; p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)
    lr_, b1_, b2_, eps_, wd_ = (float(f32(c)) for c in (lr, b1, b2, eps, wd))
    want_norm = float(torch.cat(grads[1]).double().norm())
    max_norm = state["views"][4]
    p, m, v = [t.double() for t in p0], [torch.zeros(n, dtype=torch.float64) for n in sizes], [torch.zeros(n, dtype=torch.float64) for n in sizes]
    for s in range(2):
        coef = 1.0 if s == 0 else min(max_norm / (want_norm + 1e-6), 1.0)
        t = s + 1
        for i in range(len(sizes)):
            g = grads[s][i].double() * coef
            p[i] = p[i] * (1.0 - lr_ * wd_)
            m[i] = m[i] + (1.0 - b1_) * (g - m[i])
            v[i] = b2_ * v[i] + (1.0 - b2_) * g * g
            p[i] = p[i] - (lr_ / (1.0 - b1_ ** t)) * m[i] / (v[i].sqrt() / (1.0 - b2_ ** t) ** 0.5 + eps_)
    for name in layouts:
        gp, gm, gv, norm, _ = state[name]
        assert abs(float(norm) - want_norm) <= 2.0 ** -23 * want_norm, (name, float(norm), want_norm)
        for what, got, want in (("p", gp, p), ("exp_avg", gm, m), ("exp_avg_sq", gv, v)):
            for i, (x, y) in enumerate(zip(want, got)):
                rel = float((y.double().cpu() - x).abs().max() / x.abs().max())
                print(f"FusedAdamW {name} {what}[{i}] ({sizes[i]}): {rel:.2e}")
                assert rel <= 2e-6, (name, what, i, rel)
    assert same_bits(state["views"][3], state["aligned"][3]), "the norm of unaligned gradients differs from the aligned one"
    for k, what in enumerate(("p", "exp_avg", "exp_avg_sq")):
        for i, (x, y) in enumerate(zip(state["views"][k], state["aligned"][k])):
            assert same_bits(x, y), f"{what}[{i}] ({sizes[i]} elements): the unaligned step differs from the aligned one"
