"""Host side of the LayerNorm / GroupNorm / GEGLU backward (csrc/norm_bwd.hip): the exported names, the extents the
*_supported functions take and refuse, the entry points' refusals before any launch, and the dropout refusal of the
differentiable transformer block.  Nothing here touches the GPU."""
import pytest
import torch

NEW = ("tmdiff_layer_norm_stats", "tmdiff_group_norm_stats", "tmdiff_layer_norm_bwd_supported",
       "tmdiff_layer_norm_bwd_workspace_bytes", "tmdiff_layer_norm_bwd", "tmdiff_group_norm_bwd_supported",
       "tmdiff_group_norm_bwd_workspace_bytes", "tmdiff_group_norm_bwd", "tmdiff_geglu_bwd")

#           rows  D         (the cases of tests/test_gpu_norm_bwd.py)
LN_TAKEN = ((1, 1), (7, 40), (5, 64), (5, 65), (130, 128), (1030, 320), (3, 4096))
LN_REFUSED = ((4, 0), (4, 4097), (1 << 20, 2048))                                   # D = 0, D > 4096, rows * D = 2^31
#           B  C    P    groups
GN_TAKEN = ((2, 32, 64, 32), (2, 64, 64, 32), (2, 64, 49, 32), (3, 64, 1, 32), (1, 32, 1, 32), (2, 16, 64, 4), (1, 128, 256, 32))
GN_REFUSED = ((2, 30, 64, 4), (65536, 32, 4, 32), (2, 32, 1 << 25, 32))             # C % groups, B = 65536, B * C * P = 2^31


def test_names_are_bound_and_exported():
    from tmdiff_amd import _lib
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert hasattr(_lib.lib, name), name
    assert _lib.ABI_VERSION == 6


@pytest.mark.parametrize("rows,d", LN_TAKEN)
def test_layer_norm_extents_taken(rows, d):
    from tmdiff_amd._lib import lib
    assert lib.tmdiff_layer_norm_bwd_supported(rows, d) == 1
    assert lib.tmdiff_layer_norm_bwd_workspace_bytes(rows, d) >= 2 * d * 4


@pytest.mark.parametrize("rows,d", LN_REFUSED)
def test_layer_norm_extents_refused(rows, d):
    from tmdiff_amd._lib import lib
    assert lib.tmdiff_layer_norm_bwd_supported(rows, d) == 0
    assert lib.tmdiff_layer_norm_bwd_workspace_bytes(rows, d) == 0
    # NULL everywhere: a refusal comes before any pointer is looked at, and nothing is launched
    status = lib.tmdiff_layer_norm_bwd(None, None, None, None, None, None, None, None, None, rows, d, None)
    assert status == -2, status                                                     # TMDIFF_E_UNSUPPORTED
    assert b"layer_norm_bwd" in lib.tmdiff_last_error_string()


def test_layer_norm_largest_extents_taken():
    from tmdiff_amd._lib import lib
    assert lib.tmdiff_layer_norm_bwd_supported((1 << 20) - 1, 2048) == 1            # one row below rows * D = 2^31
    assert lib.tmdiff_layer_norm_bwd_supported(8, 4096) == 1


@pytest.mark.parametrize("b,c,p,groups", GN_TAKEN)
def test_group_norm_extents_taken(b, c, p, groups):
    from tmdiff_amd._lib import lib
    assert lib.tmdiff_group_norm_bwd_supported(b, c, p, groups) == 1
    assert lib.tmdiff_group_norm_bwd_workspace_bytes(b, c, p, groups) == 2 * b * c * 4


@pytest.mark.parametrize("b,c,p,groups", GN_REFUSED)
def test_group_norm_extents_refused(b, c, p, groups):
    from tmdiff_amd._lib import lib
    assert lib.tmdiff_group_norm_bwd_supported(b, c, p, groups) == 0
    assert lib.tmdiff_group_norm_bwd_workspace_bytes(b, c, p, groups) == 0
    status = lib.tmdiff_group_norm_bwd(None, None, None, None, None, None, None, None, None, b, c, p, groups, None)
    assert status == -2, status
    assert b"group_norm_bwd" in lib.tmdiff_last_error_string()


def test_entry_points_refuse_null_pointers_without_launching():
    """Extents that are taken, but NULL tensors: TMDIFF_E_INVALID from the argument check in front of the launch."""
    from tmdiff_amd._lib import lib
    assert lib.tmdiff_layer_norm_bwd(None, None, None, None, None, None, None, None, None, 7, 40, None) == -1
    assert lib.tmdiff_group_norm_bwd(None, None, None, None, None, None, None, None, None, 2, 32, 64, 32, None) == -1
    assert lib.tmdiff_geglu_bwd(None, None, None, 3, 5, 0, None) == -1
    assert lib.tmdiff_geglu_bwd(None, None, None, 3, 0, 0, None) == -1
    assert lib.tmdiff_layer_norm_stats(None, None, None, None, None, None, 7, 40, 1e-5, None) == -1
    assert lib.tmdiff_group_norm_stats(None, None, None, None, None, None, 2, 32, 64, 32, 1e-6, None) == -1


def test_ops_raise_value_error_on_refused_extents():
    """ops.layer_norm_bwd / group_norm_bwd ask *_supported first (meta tensors: no storage, no kernel)."""
    from tmdiff_amd import ops
    x = torch.empty(4, 4097, device="meta")
    with pytest.raises(ValueError, match="layer_norm_bwd"):
        ops.layer_norm_bwd(x, None, x, None, None)
    x = torch.empty(2, 30, 8, 8, device="meta")
    with pytest.raises(ValueError, match="group_norm_bwd"):
        ops.group_norm_bwd(x, None, x, None, None, groups=4)


def test_block_with_dropout_has_no_differentiable_path():
    from tmdiff_amd import Attention as A
    blk = A.BasicTransformerBlock(32, 2, 16, dropout=0.1, context_dim=24).train()
    x, ctx = torch.randn(1, 4, 32), torch.randn(1, 3, 24)
    assert torch.is_grad_enabled()
    with pytest.raises(NotImplementedError, match="dropout"):
        blk(x, context=ctx)                          # CPU tensors: the refusal comes before any kernel is reached
    st = A.SpatialTransformer(32, 2, 16, depth=1, dropout=0.1, context_dim=24).train()
    with pytest.raises(NotImplementedError, match="dropout"):
        st(torch.randn(1, 32, 2, 2), context=ctx)
    ff = A.FeedForward(32, dropout=0.1, glu=True).train()
    with pytest.raises(NotImplementedError, match="dropout"):
        ff(x)
