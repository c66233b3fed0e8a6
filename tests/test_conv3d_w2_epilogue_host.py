"""conv3d_w2's epilogues on the host: routing.wino2d_epilogue_ok is the mirror of the library's
tmdiff_conv3d_w2_epilogue_supported, the older query keeps refusing those descriptors, and the route needs both switches and
changes no fusion plan."""
from tmdiff_amd import ops, routing

Q = "tmdiff_conv3d_w2_epilogue_supported"
P = 16                  # a placeholder pointer (never dereferenced)
HI = (P, P, P)

# the three launches of the benchmark step (256 -> 256 at 8 x 16 x 16, batch 32) as descriptor fields
LL_RC_S2D = dict(rc_x=P, rc_cin=128, y_ll=P, y2=P, y2_s2d=1)       # down3.conv20.conv21, main branch
LL_RC = dict(rc_x=P, rc_cin=128, y_ll=P, y2=P)                     # ... condition branch
DWT = dict(y_ll=P, y_hi=HI)                                        # down3_1.down.Conv_0
BENCH = (32, 256, 256, 8, 16, 16, 1)

TABLE = [  # ((b, cin, cout, n, h, w, groups), mirror arguments (rc_cin, quarter), descriptor fields)
    (BENCH, (128, True), LL_RC_S2D), (BENCH, (128, True), LL_RC), (BENCH, (0, True), DWT),
    (BENCH, (0, False), {}), (BENCH, (128, False), dict(rc_x=P, rc_cin=128, y=P)), (BENCH, (0, True), dict(y2=P, y2_s2d=1)),
    ((2, 128, 256, 8, 12, 10, 1), (32, True), dict(rc_x=P, rc_cin=32, y_ll=P, y2=P)),
    ((2, 128, 256, 4, 8, 8, 1), (128, False), dict(rc_x=P, rc_cin=128, y=P)),          # 4 bands fold, without quarter outputs
    # one condition broken
    ((32, 256, 256, 4, 16, 16, 1), (128, True), LL_RC), ((32, 256, 256, 4, 16, 16, 1), (0, True), DWT),    # 4 bands with y_ll
    ((32, 256, 256, 8, 15, 16, 1), (128, True), LL_RC), ((32, 256, 256, 8, 15, 16, 1), (0, True), DWT),    # odd H
    ((32, 256, 256, 8, 15, 16, 1), (128, False), dict(rc_x=P, rc_cin=128, y=P)),                           # ... also for the fold alone
    (BENCH, (48, True), dict(LL_RC, rc_cin=48)), (BENCH, (544, True), dict(LL_RC, rc_cin=544)),
    ((32, 256, 128, 8, 16, 16, 1), (128, True), LL_RC), ((32, 256, 256, 8, 16, 32, 1), (128, True), LL_RC),
    ((32, 768, 384, 8, 16, 16, 3), (128, True), LL_RC), ((32, 768, 384, 8, 16, 16, 3), (0, True), DWT),
]

# combinations of pointers that ops.conv3d_w2 never builds (it raises first): the library refuses them by itself
REFUSED = [dict(LL_RC, residual=P), dict(rc_x=P, rc_cin=128, y=P, residual=P),      # residual beside rc_x
           dict(LL_RC, y=P), dict(DWT, y=P),                                        # y beside y_ll
           dict(y_ll=P), dict(DWT, y2=P), dict(y_hi=HI), dict(y2_s2d=1)]            # y_ll without y2; y_hi with y2 / without y_ll; s2d of nothing


def test_epilogue_query_agrees_with_the_python_predicate():
    for ext, (rc_cin, quarter), fields in TABLE:
        want = routing.supported(Q, *ext, **fields)
        assert routing.wino2d_epilogue_ok(*ext, rc_cin=rc_cin, quarter=quarter) == want, (ext, rc_cin, quarter, want)
    assert [routing.wino2d_epilogue_ok(*e, rc_cin=r, quarter=q) for e, (r, q), _ in TABLE] == [True] * 8 + [False] * 11
    for fields in REFUSED:
        assert not routing.supported(Q, *BENCH, **fields), fields
    # every descriptor of the plain query is one of the new query's, and without the new fields the mirrors coincide
    for ext in [BENCH[:6], (2, 128, 256, 8, 12, 10), (2, 128, 256, 8, 11, 10), (32, 64, 256, 8, 16, 16), (32, 256, 256, 6, 16, 16)]:
        plain = routing.supported("tmdiff_conv3d_w2_supported", *ext)
        assert routing.supported(Q, *ext) == plain == routing.wino2d_ok(*ext) == routing.wino2d_epilogue_ok(*ext)


def test_the_plain_query_still_refuses_the_new_descriptors():
    for fields in (LL_RC_S2D, LL_RC, DWT, dict(y_ll=P, y2=P), dict(y2=P, y2_s2d=1), dict(rc_x=P, rc_cin=128, y=P)):
        assert not routing.supported("tmdiff_conv3d_w2_supported", *BENCH, **fields), fields
        assert routing.supported(Q, *BENCH, **fields), fields


def test_epilogue_route_needs_both_switches_and_changes_no_plan():
    args = (32, 256, 256, 8, 16, 16, 1, 128, True)
    for wino2d in (False, True):
        for epi in (False, True):
            with ops.config.override(wino2d=wino2d, wino2d_epilogue=epi):
                assert routing.wino2d_epilogue_route(*args) == (wino2d and epi)
                assert not routing.wino2d_epilogue_route(32, 128, 128, 8, 32, 32, 1, 64, True)
    with ops.config.override(wino2d_epilogue=False):
        off = routing.unet_fusions(routing.FULL, 32, 8, 64, 64)
    with ops.config.override(wino2d_epilogue=True):
        on = routing.unet_fusions(routing.FULL, 32, 8, 64, 64)
    assert on == off
