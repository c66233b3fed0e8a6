"""Host side of the attention backward: the support rule, the workspace query and the ctypes table (no GPU)."""
import pytest

NEW = ("tmdiff_attn_fwd_lse", "tmdiff_attn_bwd_supported", "tmdiff_attn_bwd_workspace_bytes", "tmdiff_attn_bwd")

SUPPORTED = ((2, 8, 130, 77, 64), (1, 1, 1, 1, 2), (2, 2, 33, 40, 40), (1, 2, 130, 160, 128), (65535, 1, 1, 1, 2),
             (1, 1, 2 ** 24, 7, 126), (1, 1, (2 ** 31 - 1) // 128, 1, 128))
REFUSED = {
    "odd D": ((2, 8, 130, 77, 63), (1, 1, 1, 1, 1)),
    "D > 128": ((2, 8, 130, 77, 130), (1, 1, 4, 4, 256)),
    "zero or negative extents": ((0, 8, 130, 77, 64), (2, 0, 130, 77, 64), (2, 8, 0, 77, 64), (2, 8, 130, 0, 64),
                                 (2, 8, 130, 77, 0), (-1, 8, 130, 77, 64), (2, -8, 130, 77, 64), (2, 8, -130, 77, 64),
                                 (2, 8, 130, -77, 64), (2, 8, 130, 77, -64)),
    "B * H beyond the grid": ((65536, 1, 1, 1, 2), (256, 256, 4, 4, 64)),
    # q / out or k / v of more than 2^31 - 1 elements (tmdiff_hip.h: row and statistics indices are 32-bit)
    "element counts past 2^31 - 1": ((1, 1, 2 ** 30, 1, 2), (1, 1, 1, 2 ** 30, 2), (1, 1, 2 ** 24, 1, 128), (1, 1, 1, 2 ** 24, 128),
                                     (32, 8, 2 ** 17, 77, 64), (32, 8, 77, 2 ** 17, 64), (1, 1, (2 ** 31 - 1) // 128 + 1, 1, 128),
                                     (1, 1, 2 ** 31 - 1, 2 ** 31 - 1, 128)),
}


def test_new_names_are_bound():
    from tmdiff_amd import _lib
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert hasattr(_lib.lib, name), name


@pytest.mark.parametrize("extents", SUPPORTED)
def test_supported_extents(extents):
    from tmdiff_amd import _lib
    assert _lib.lib.tmdiff_attn_bwd_supported(*extents) == 1, extents
    b, h, nq = extents[:3]
    assert _lib.lib.tmdiff_attn_bwd_workspace_bytes(*extents) >= 4 * b * h * nq > 0, extents


@pytest.mark.parametrize("why", sorted(REFUSED))
def test_refused_extents(why):
    from tmdiff_amd import _lib
    for extents in REFUSED[why]:
        assert _lib.lib.tmdiff_attn_bwd_supported(*extents) == 0, (why, extents)
        assert _lib.lib.tmdiff_attn_bwd_workspace_bytes(*extents) == 0, (why, extents)


def test_launch_refuses_without_launching():
    """A refused shape returns a TMDIFF_E_* status before any pointer is looked at or anything is launched (NULL pointers here)."""
    import ctypes as C
    from tmdiff_amd import _lib
    st = (C.c_int64 * 3)(0, 0, 0)
    for extents in ((2, 8, 130, 77, 63), (0, 8, 130, 77, 64), (1, 1, 2 ** 30, 1, 2), (65536, 1, 1, 1, 2)):
        rc = _lib.lib.tmdiff_attn_bwd(None, None, None, None, None, None, None, None, None, None, None, *extents, st, st, st, st,
                                      1.0, None)
        assert rc < 0, extents
        assert b"attn_bwd" in _lib.lib.tmdiff_last_error_string()
    # ... and supported extents with NULL tensors are an invalid-argument error, not a launch
    rc = _lib.lib.tmdiff_attn_bwd(None, None, None, None, None, None, None, None, None, None, None, 2, 8, 130, 77, 64, st, st, st,
                                  st, 1.0, None)
    assert rc == -1
    rc = _lib.lib.tmdiff_attn_fwd_lse(None, None, None, None, None, 2, 8, 130, 77, 64, st, st, st, st, 1.0, None, None)
    assert rc == -1
