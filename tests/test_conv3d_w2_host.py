"""conv3d_w2's routing rule on the host: routing.wino2d_ok is the mirror of the library's tmdiff_conv3d_w2_supported, and the
route is taken only with the switch on."""
from tmdiff_amd import ops, routing

TABLE = [  # (b, cin, cout, n, h, w, groups)
    (32, 256, 256, 8, 16, 16, 1), (32, 128, 256, 8, 16, 16, 1), (32, 256, 256, 8, 8, 8, 1), (2, 128, 256, 4, 8, 8, 1),
    (2, 128, 256, 8, 12, 10, 1), (1, 512, 512, 8, 32, 16, 1), (8, 256, 512, 4, 4, 2, 1),
    (32, 128, 128, 8, 32, 32, 1),      # 128 output channels, 32 columns: out of scope
    (32, 64, 256, 8, 16, 16, 1),       # Cin < 128
    (32, 256, 128, 8, 16, 16, 1),      # Cout < 256
    (32, 144, 256, 8, 16, 16, 1),      # Cin not a multiple of 32
    (32, 256, 288, 8, 16, 16, 1),      # Cout not a multiple of 64
    (32, 256, 256, 8, 16, 32, 1),      # too wide
    (32, 256, 256, 8, 16, 15, 1),      # odd width
    (32, 256, 256, 8, 2, 16, 1), (32, 256, 256, 8, 34, 16, 1),     # rows outside 4 .. 32
    (32, 256, 256, 6, 16, 16, 1), (32, 256, 256, 2, 16, 16, 1),    # band counts other than 8 / 4
    (32, 768, 384, 8, 8, 8, 3),        # grouped
    (40000, 256, 256, 8, 8, 8, 1),     # more images than the passes' grids hold
    (4096, 1024, 256, 8, 32, 16, 1),   # a plane of the transformed input beyond 32-bit byte offsets
]


def test_w2_supported_agrees_with_the_python_predicate():
    for b, cin, cout, n, h, w, g in TABLE:
        want = routing.supported("tmdiff_conv3d_w2_supported", b, cin, cout, n, h, w, g)
        assert routing.wino2d_ok(b, cin, cout, n, h, w, g) == want, (b, cin, cout, n, h, w, g, want)
    assert sum(routing.wino2d_ok(*row) for row in TABLE) == 7
    # what the descriptor adds: a folded 1x1x1, a mask, dropout, an LL output, segments are not taken
    for extra in (dict(rc_x=16, rc_cin=128), dict(in_mask=16), dict(drop_p=0.1), dict(y_ll=16), dict(y2_s2d=1)):
        assert not routing.supported("tmdiff_conv3d_w2_supported", 32, 256, 256, 8, 16, 16, 1, **extra)
    assert not routing.supported("tmdiff_conv3d_w2_supported", 32, (128, 128), 256, 8, 16, 16, 1)


def test_w2_route_needs_the_switch():
    with ops.config.override(wino2d=False):
        assert not routing.wino2d_route(32, 256, 256, 8, 16, 16)
    with ops.config.override(wino2d=True):
        assert routing.wino2d_route(32, 256, 256, 8, 16, 16) and not routing.wino2d_route(32, 128, 128, 8, 32, 32)
