"""The helpers of wgrad_wino_refs.py, proved on the CPU: the restated plan, the exactness of the lattice inputs, the fp64
restatement of the Winograd algorithm against F.conv3d's autograd, and the power of the two tiers of
test_gpu_wgrad_wino_edges.py against deliberate faults.

Power of the checks.  Seven faults are injected into the restatement (wgrad_wino_refs.winograd64): the last box of the last
split range dropped, the band halo between two tiles dropped, the last image column written as padding, two channels of a tile
swapped, the centre tap reading its left neighbour's column, the second 64-channel chunk skipped in the reduction, CoP in place
of cout_g in the dbias index.  On lattice inputs EVERY one of them changes the result, in every case where it applies, and the
exact tier allows no difference at all.  On N(0, 1) data, against the rounding bound c * 2^-24 * M of the rounding tier
(test_rounding_bound_against_faults_on_random_data prints the worst |fault - ref| / bound per case), the bound catches every
one of them too on these shapes -- a fault of this size moves an element by a whole term, 1e3 to 1e5 bounds -- but what the
bound cannot see is a fault that costs LESS than c * 2^-24 * M: a single position lost from one plane of a 128-position box
moves an element by about M / (positions x 6 planes), which at the production layers (2e5 positions and more per element) is
below the bound (test_one_lost_position_hides_below_the_rounding_bound shows the crossover on a restated sum: the same loss is
over 200 bounds at 128 positions and 4e-4 of one at 2^17 positions).  The exact tier sees it at any size.  That is why
both tiers exist: the exact tier for lost, doubled or misplaced terms, the rounding tier for precision on real-valued data
(a kernel that rounded x^ to bf16 would pass the exact tier, whose x^ are small integers).
"""
import functools

import pytest
import torch

import wgrad_wino_refs as R
from oracle.make_golden import randn

PLAN_TABLE = {
    # name: (T, bw, Hb, Wb, tiles_ci, tiles_co, reduce chunks, transform chunks, boxes, splits, bps, boxes of the last range)
    "smallest": (1, 8, 8, 8, 1, 1, 1, 1, 1, 1, 1, 1),
    "box8x8-six-padding-rows": (1, 8, 8, 8, 1, 1, 1, 1, 1, 1, 1, 1),
    "W4-Hb16-two-tiles": (2, 8, 16, 8, 1, 1, 1, 1, 8, 8, 1, 1),
    "four-band-tiles": (4, 16, 8, 16, 1, 1, 1, 1, 4, 4, 1, 1),
    "three-tiles-ragged-W12": (3, 16, 8, 16, 1, 1, 1, 1, 3, 3, 1, 1),
    "W64-one-chunk": (1, 16, 8, 64, 1, 1, 1, 1, 4, 4, 1, 1),
    "W68-two-chunks": (1, 16, 8, 80, 1, 1, 1, 2, 5, 5, 1, 1),
    "cin33-cout33": (1, 8, 8, 8, 2, 2, 1, 1, 1, 1, 1, 1),
    "cin65-ragged-chunk": (1, 8, 8, 8, 3, 1, 2, 1, 1, 1, 1, 1),
    "cin128-full-chunks": (1, 16, 8, 16, 4, 1, 2, 1, 1, 1, 1, 1),
    "groups3-cin8-cout8": (1, 8, 8, 8, 1, 1, 1, 1, 1, 1, 1, 1),
    "groups3-cin40-cout33": (2, 16, 8, 16, 2, 2, 1, 1, 4, 4, 1, 1),
    "segments-5-30-6": (1, 16, 8, 16, 2, 1, 1, 1, 1, 1, 1, 1),
    "segments-31-33": (1, 8, 8, 8, 2, 1, 1, 1, 1, 1, 1, 1),
    "groups3-segments-10-10-4": (1, 8, 8, 8, 1, 1, 1, 1, 1, 1, 1, 1),
    "boxes1": (1, 16, 8, 16, 1, 1, 1, 1, 1, 1, 1, 1),
    "boxes2": (1, 16, 8, 16, 1, 1, 1, 1, 2, 2, 1, 1),
    "boxes3": (1, 16, 8, 16, 1, 1, 1, 1, 3, 3, 1, 1),
    "boxes5": (1, 16, 8, 16, 1, 1, 1, 1, 5, 5, 1, 1),
    "boxes6": (1, 16, 8, 16, 1, 1, 1, 1, 6, 6, 1, 1),
    "boxes7-16-tiles": (1, 16, 8, 16, 4, 4, 2, 1, 7, 4, 2, 1),        # four ranges of two boxes, the last one holds one
    "boxes5-32-tiles": (1, 16, 8, 16, 8, 4, 4, 1, 5, 2, 3, 2),        # two ranges of three boxes (an odd count), the last holds two
    "boxes14-16-tiles": (1, 16, 8, 32, 4, 4, 2, 1, 14, 5, 3, 2),      # five ranges of three boxes, the last holds two
}


def test_split_rule_by_hand():
    """choose_splits on inputs one can follow with a pencil (units workgroups per split, 512 resident, one box of overhead)."""
    cs = R.choose_splits
    assert cs(1, 6, 512, 1.0, 256) == (1, 1)
    # 7 boxes, 96 units: 1 split costs 1 * (7 + 1) = 8; 2 -> 5; 3 -> 4; 4 ranges of 2 -> 1 * 3 = 3; 7 ranges need 672 workgroups,
    # two rounds: 2 * 2 = 4.  Four ranges, the last one of one box.
    assert cs(7, 96, 512, 1.0, 256) == (4, 2)
    # 4 boxes, 256 units: 1 -> 5; 2 ranges of 2 -> 3; 4 ranges -> two rounds of (1 + 1) = 4
    assert cs(4, 256, 512, 1.0, 256) == (2, 2)
    # a tie goes to the smaller count: 2 boxes, 512 units, no overhead: 1 * 2 = 2 * 1
    assert cs(2, 512, 512, 0.0, 256) == (1, 2)
    # smax caps the count; no range is empty: 10 boxes in at most 3 ranges -> 4 + 4 + 2
    assert cs(10, 1, 512, 1.0, 3) == (3, 4)
    # 9 boxes asked into 4 ranges of 3 give 3 ranges: the count is the effective one
    assert cs(9, 1, 512, 1.0, 4) == (3, 3)


@pytest.mark.parametrize("case", R.CASES, ids=[c.name for c in R.CASES])
def test_plan_of_every_case(case):
    """The restated plan gives each case of the GPU module the property it is there for (PLAN_TABLE, asserted)."""
    p = R.case_plan(case)
    got = (p.T, p.bw, p.Hb, p.Wb, p.tiles_ci, p.tiles_co, p.cchunks, p.wchunks, p.nboxes, p.splits, p.bps, p.last_range)
    print(f"\nplan {case.name}: T={p.T} box 8x{p.bw} plane {p.Hb}x{p.Wb} tiles {p.tiles_co}x{p.tiles_ci} reduce chunks {p.cchunks} "
          f"transform chunks {p.wchunks}: {p.nboxes} boxes = {p.splits} splits x {p.bps}, last {p.last_range}; nbias {p.nbias}")
    assert got == PLAN_TABLE[case.name]
    assert 1 <= p.last_range <= p.bps and (p.splits - 1) * p.bps + p.last_range == p.nboxes
    assert p.xh_floats % 4 == 0 and p.gh_floats % 4 == 0
    assert p.workspace_bytes(True) - p.workspace_bytes(False) == 4 * case.B * sum(case.segc) * case.N * case.H * case.W


def test_the_cases_cover_the_split_classes():
    """split counts below four, above four and no multiple of four; 1, 2 and 3 boxes per workgroup (3: an odd count in the
    double-buffered loop); a last range shorter than the others; one and several reduce chunks, a ragged one; one and two
    transform chunks; 1 to 4 band tiles; both box widths; groups = 3 with cout_g < CoP"""
    plans = {c.name: R.case_plan(c) for c in R.CASES}
    splits = {p.splits for p in plans.values()}
    assert {1, 2, 3} <= splits and {5, 6, 8} <= splits and 4 in splits
    assert {p.bps for p in plans.values()} >= {1, 2, 3}
    assert any(p.last_range < p.bps for p in plans.values() if p.bps == 2) and any(p.last_range < p.bps for p in plans.values() if p.bps == 3)
    assert {p.T for p in plans.values()} == {1, 2, 3, 4} and {p.bw for p in plans.values()} == {8, 16}
    assert any(p.cchunks > 1 and p.cin_g % 64 for p in plans.values()) and any(p.cchunks > 1 and p.cin_g % 64 == 0 for p in plans.values())
    assert any(p.groups == 3 and p.cout_g < p.CoP and p.cin_g % 32 for p in plans.values())
    assert any(p.cin_g == 1 and p.cout_g == 1 for p in plans.values()) and any(p.cin_g == 33 and p.cout_g == 33 for p in plans.values())
    assert any(p.cin_g == 65 for p in plans.values())


# ---- lattice inputs ----------------------------------------------------------------------------------------------------------
VARIANTS = {"plain": {}, "all": dict(shift=True, scale="rows", mask=True)}


@functools.lru_cache(maxsize=None)
def lattice(name, variant="plain"):
    c = R.CASE[name]
    d = R.lattice_inputs(1000 + R.CASES.index(c), c.B, c.segc, c.cout, c.N, c.H, c.W, **VARIANTS[variant])
    xp = R.prologue64(d["xs"], d["shift"], d["scale"], d["mask"])
    assert torch.equal(xp.float().double(), xp)
    return xp.float(), d["g"], R.case_plan(c)


LATTICE_RUNS = [(c.name, "plain") for c in R.CASES] + [(n, "all") for n in R.PROLOGUE_CASES]


@pytest.mark.parametrize("name,variant", LATTICE_RUNS, ids=[f"{n}-{v}" for n, v in LATTICE_RUNS])
def test_lattice_inputs_are_exact(name, variant):
    """exactness_ok on every case, and with every exact prologue part at once on the cases the GPU module runs a prologue on;
    zeros are frequent but not everywhere"""
    xp, g, pl = lattice(name, variant)
    assert R.exactness_ok(xp, g, pl)
    zx, zg = float((xp == 0).float().mean()), float((g == 0).float().mean())
    assert 0.2 < zx < 0.8 and 0.1 < zg < 0.6, (zx, zg)
    if variant == "plain":
        assert set(xp.unique().tolist()) <= {-2.0, -1.0, 0.0, 1.0, 2.0}


def test_exactness_check_refuses_inexact_inputs():
    """the check itself has teeth: g = 1 (1/6 rounds) and x = 1/3 + large (B^T x rounds) are refused"""
    c = R.CASE["box8x8-six-padding-rows"]
    xp, g, pl = lattice(c.name)
    with pytest.raises(AssertionError):
        R.exactness_ok(xp, torch.ones_like(g), pl)
    with pytest.raises(AssertionError):
        R.exactness_ok(xp * (1.0 / 3.0) + 1000.0 * (xp != 0), g, pl)


# ---- the fp64 restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CASES, ids=[c.name for c in R.CASES])
def test_winograd_restatement_equals_autograd(case):
    """transform, per-box accumulation, split and chunk bookkeeping, A'^T and the bias path in fp64 equal F.conv3d's weight
    gradient to 1e-12 on N(0, 1) data: the matrices and the tile / halo / padding bookkeeping behind dw_abs64 are right."""
    pl = R.case_plan(case)
    xp = randn(11, case.B, sum(case.segc), case.N, case.H, case.W)
    g = randn(12, case.B, case.cout, case.N, case.H, case.W)
    ref, rb = R.dw_ref64(xp, g, case.groups, -2.0)
    dw, db = R.winograd64(xp, g, pl, -2.0)
    assert float((dw - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    assert float((db - rb).abs().max()) <= 1e-12 * float(rb.abs().max())
    M, Mb = R.dw_abs64(xp, g, pl, -2.0)
    assert bool((M >= ref.abs() * (1 - 1e-12)).all()) and bool((Mb >= rb.abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("case", R.CASES, ids=[c.name for c in R.CASES])
def test_every_fault_is_flagged_on_the_lattice(case):
    """On lattice inputs the restatement equals autograd EXACTLY, and each injected fault changes dw (biasidx: dbias) in every
    case where it applies -- exact comparison is what the GPU module's exact tier does."""
    xp, g, pl = lattice(case.name)
    ref, rb = R.dw_ref64(xp, g, case.groups)
    dw, db = R.winograd64(xp, g, pl)
    assert torch.equal(dw, ref) and torch.equal(db, rb)
    assert torch.equal(ref.float().double(), ref) and torch.equal(rb.float().double(), rb)       # (fp32 holds the reference)
    flagged = []
    for fault in R.FAULTS:
        if not R.fault_applies(fault, pl):
            continue
        fdw, fdb = R.winograd64(xp, g, pl, fault=fault)
        hit = not torch.equal(fdb, rb) if fault == "biasidx" else not torch.equal(fdw, ref)
        assert hit, f"{case.name}: fault {fault} goes unnoticed"
        flagged.append(fault)
    print(f"\nfaults {case.name}: flagged exactly: {', '.join(flagged)}")
    assert {"lastbox", "column", "tap"} <= set(flagged)


def test_every_fault_applies_somewhere():
    for fault in R.FAULTS:
        assert sum(R.fault_applies(fault, R.case_plan(c)) for c in R.CASES) >= 3, fault


@pytest.mark.parametrize("name", R.ROUNDING_CASES)
def test_rounding_bound_against_faults_on_random_data(name):
    """The record the module docstring quotes: on N(0, 1) data every applicable fault exceeds c * 2^-24 * M (dbias: D * 2^-24 *
    sum|g|) somewhere, by the factor printed."""
    c = R.CASE[name]
    pl = R.case_plan(c)
    xp = randn(21, c.B, sum(c.segc), c.N, c.H, c.W)
    g = randn(22, c.B, c.cout, c.N, c.H, c.W)
    ref, rb = R.dw_ref64(xp, g, c.groups)
    M, Mb = R.dw_abs64(xp, g, pl)
    out = []
    for fault in R.FAULTS:
        if R.fault_applies(fault, pl):
            fdw, fdb = R.winograd64(xp, g, pl, fault=fault)
            ratio = float(((fdb - rb).abs() / (pl.bias_depth() * R.U24 * Mb)).max()) if fault == "biasidx" else \
                float(((fdw - ref).abs() / (pl.depth() * R.U24 * M)).max())
            out.append((fault, ratio))
    print(f"\nfaults {name} (c = {pl.depth()}): worst |fault - ref| / bound on N(0,1): " + ", ".join(f"{f} {r:.2e}" for f, r in out))
    assert all(r > 1.0 for _, r in out), out


def test_one_lost_position_hides_below_the_rounding_bound():
    """What the rounding tier cannot see.  One element of dw is a sum of P products per plane; losing ONE product of N(0, 1) data
    costs about one term, the bound is c * 2^-24 times the sum of P * 6 absolute terms with c growing with the positions a
    workgroup adds in sequence (two per K-step).  With c = 32 * P / 128 + 17 (one box of 128 positions per 32 additions) the
    lost term is many bounds at P = 128 and below one bound at P = 2^17: asserted on drawn data."""
    gen = torch.Generator().manual_seed(5)
    ratios = {}
    for P in (128, 2 ** 17):
        terms = (torch.randn(6, P, generator=gen, dtype=torch.float64) * torch.randn(6, P, generator=gen, dtype=torch.float64)).abs()
        c = 32 * P // 128 + 17
        ratios[P] = float(terms[0].median() / (c * R.U24 * terms.sum()))          # a typical term, not a drawn one
    print(f"\none lost typical term / bound: {ratios}")
    assert ratios[128] > 5.0 and ratios[2 ** 17] < 1.0
