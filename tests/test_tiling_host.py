"""Host side of fused tiled sampling (tmdiff_amd.tiling.plan_tiles, the blend's definition, the new C exports).  No kernel
is launched here.  ``blend_ref`` is the fp64 NumPy restatement of the blend that the GPU tests compare the kernel against."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

PLANS = [(512, 64, 16), (512, 64, 32), (512, 64, 8), (72, 32, 8), (80, 32, 8), (48, 32, 16), (100, 32, 16), (64, 64, 16),
         (96, 32, 0)]
# plans whose per-axis cover is at most 2: the jump bound holds on these (on (100, 32, 16) a pixel has three covering tiles)
JUMP_PLANS = [(512, 64, 16), (512, 64, 32), (512, 64, 8), (128, 64, 32), (72, 32, 8), (80, 32, 8), (48, 32, 16), (256, 64, 24),
              (136, 64, 16)]


def w1(tile, overlap):
    i = np.arange(tile, dtype=np.float64)
    return np.minimum(np.minimum(i + 1, tile - i), overlap + 1)


def blend_ref(tiles, batch, h, w, overlap):
    """fp64: scene[b, c, y, x] = sum(w v) / sum(w) over the covering tiles; tiles [batch * ny * nx, C, tile, tile], row-major."""
    from tmdiff_amd.tiling import plan_tiles
    tiles = np.asarray(tiles, dtype=np.float64)
    tile = tiles.shape[-1]
    rows, cols = plan_tiles(h, w, tile, overlap)
    assert tiles.shape[0] == batch * len(rows) * len(cols)
    w2 = np.outer(w1(tile, overlap), w1(tile, overlap))
    num, den = np.zeros((batch, tiles.shape[1], h, w)), np.zeros((h, w))
    n = 0
    for b in range(batch):
        for oy in rows:
            for ox in cols:
                num[b, :, oy:oy + tile, ox:ox + tile] += w2 * tiles[n]
                if b == 0:
                    den[oy:oy + tile, ox:ox + tile] += w2
                n += 1
    assert den.min() >= 1.0
    return num / den


def gather_ref(scene, tile, overlap):
    from tmdiff_amd.tiling import plan_tiles
    rows, cols = plan_tiles(scene.shape[2], scene.shape[3], tile, overlap)
    return np.stack([scene[b, :, oy:oy + tile, ox:ox + tile] for b in range(scene.shape[0]) for oy in rows for ox in cols])


def max_jump(scene):
    scene = np.asarray(scene, dtype=np.float64)
    return max(np.abs(np.diff(scene, axis=-1)).max(), np.abs(np.diff(scene, axis=-2)).max())


def constant_tiles(rng, n, c, tile):
    vals = rng.uniform(-1.0, 1.0, size=(n, c))
    return np.broadcast_to(vals[:, :, None, None], (n, c, tile, tile)).copy(), vals


@pytest.mark.parametrize("L,tile,overlap", PLANS)
def test_plan_properties(L, tile, overlap):
    from tmdiff_amd.tiling import plan_tiles
    rows, cols = plan_tiles(L, L, tile, overlap)
    assert rows == cols
    assert rows[0] == 0 and rows[-1] == L - tile
    assert all(0 <= o and o + tile <= L for o in rows)                      # no tile leaves the scene
    assert rows == sorted(set(rows))
    s = tile - overlap
    assert all(b - a == s for a, b in zip(rows[:-2], rows[1:-1]))           # regular spacing up to the pushed-in tile
    assert 0 < rows[-1] - rows[-2] <= s if len(rows) > 1 else True
    cover = np.zeros(L, dtype=int)
    for o in rows:
        cover[o:o + tile] += 1
    assert cover.min() >= 1 and cover.max() <= 3                            # every pixel is covered
    # non-square: the axes are planned independently
    r2, c2 = plan_tiles(L, tile, tile, overlap)
    assert r2 == rows and c2 == [0]


def test_plan_without_overlap_is_the_split_tiles_grid():
    from tmdiff_amd.tiling import plan_tiles, split_tiles
    rows, cols = plan_tiles(96, 64, 32, 0)
    assert rows == [0, 32, 64] and cols == [0, 32]
    x = torch.arange(2 * 3 * 96 * 64, dtype=torch.float32).reshape(2, 3, 96, 64)
    assert np.array_equal(gather_ref(x.numpy(), 32, 0), split_tiles(x, 32, 32).numpy())


@pytest.mark.parametrize("args", [(63, 64, 64, 16), (64, 63, 64, 16), (64, 64, 36, 8), (64, 64, 0, 0), (64, 64, 32, 17),
                                  (64, 64, 32, -1), (40, 40, 64, 16)])
def test_plan_rejects_bad_arguments(args):
    from tmdiff_amd.tiling import plan_tiles
    with pytest.raises(ValueError):
        plan_tiles(*args)


@pytest.mark.parametrize("L,tile,overlap", PLANS)
def test_blend_is_a_partition_of_unity(L, tile, overlap):
    """blend(gather(x)) == x: exactly for a constant scene (constants with a short mantissa, so that the integer-weighted
    sums are exact and the only question is whether the weights divide out), to fp64 rounding for any scene."""
    from tmdiff_amd.tiling import tile_profile
    assert np.array_equal(tile_profile(tile, overlap).numpy(), w1(tile, overlap))
    h, w = L, max(tile, L // 2)
    for value in (1.0, -0.75, 3.0):
        const = np.full((1, 2, h, w), value)
        assert np.array_equal(blend_ref(gather_ref(const, tile, overlap), 1, h, w, overlap), const)
    const = np.full((1, 2, h, w), 0.7)
    assert np.abs(blend_ref(gather_ref(const, tile, overlap), 1, h, w, overlap) - const).max() <= 2.3e-16
    x = np.random.default_rng(L + overlap).normal(size=(2, 2, h, w))
    assert np.abs(blend_ref(gather_ref(x, tile, overlap), 2, h, w, overlap) - x).max() <= 1e-14
    if overlap == 0:
        assert w1(tile, 0).min() == w1(tile, 0).max() == 1.0


@pytest.mark.parametrize("L,tile,overlap", JUMP_PLANS)
def test_constant_tiles_blend_without_a_jump(L, tile, overlap):
    """Constant-valued tiles: neighbouring scene pixels differ by at most (max - min of the tile values) / (overlap + 1)."""
    from tmdiff_amd.tiling import plan_tiles
    rows, cols = plan_tiles(L, L, tile, overlap)
    rng = np.random.default_rng(L * 131 + overlap)
    worst = 0.0
    for _ in range(20):
        tiles, vals = constant_tiles(rng, len(rows) * len(cols), 1, tile)
        bound = (vals.max() - vals.min()) / (overlap + 1)
        jump = max_jump(blend_ref(tiles, 1, L, L, overlap))
        assert jump <= bound * (1 + 1e-12), (jump, bound)
        worst = max(worst, jump / bound)
    assert worst > 0.3                                                       # the bound is of the right size, not slack


def test_new_symbols_are_declared_exported_and_bound():
    from tmdiff_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tmdiff_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("tmdiff_tile_plan", "tmdiff_tile_supported", "tmdiff_tile_gather", "tmdiff_tile_blend"):
        assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared"
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert _lib.ABI_VERSION == 6


@pytest.mark.parametrize("L,tile,overlap", PLANS + JUMP_PLANS + [(4096, 64, 32), (33, 32, 1), (70, 24, 12)])
def test_the_kernels_plan_is_plan_tiles(L, tile, overlap):
    """The library states the plan a second time (origin(i) = min(i * s, L - tile), used by the kernels): same origins."""
    from tmdiff_amd import _lib
    from tmdiff_amd.tiling import _plan_axis
    want = _plan_axis(L, tile, overlap)
    buf = (ctypes.c_int32 * (len(want) + 2))()
    assert _lib.lib.tmdiff_tile_plan(L, tile, overlap, buf, len(buf)) == len(want)
    assert list(buf[:len(want)]) == want
    assert _lib.lib.tmdiff_tile_plan(L, tile, overlap, None, 0) == len(want)


def test_size_limit_is_refused_without_a_launch():
    from tmdiff_amd import _lib, ops
    assert _lib.lib.tmdiff_tile_plan(16, 32, 8, None, 0) == -1 and _lib.lib.tmdiff_tile_plan(64, 32, 17, None, 0) == -1
    assert ops.tile_supported(4, 4, 512, 512, 64, 32)
    assert ops.tile_supported(1, 8, 16384, 16384 - 64, 64, 0)         # the last whole column of tiles under 2^31 elements
    assert not ops.tile_supported(1, 8, 16384, 16384, 64, 0)          # 2^31 elements: the largest offset no longer fits
    assert not ops.tile_supported(1, 4, 16384, 16384, 64, 32)         # the scene fits (2^30), the 4x larger tile stack does not
    assert not ops.tile_supported(1, 4, 64, 64, 64, 33) and not ops.tile_supported(1, 4, 32, 64, 64, 0)
    # the entry points return an error status for such extents before they look at the tensors' contents
    fake = ctypes.c_void_p(4096)
    for fn in (_lib.lib.tmdiff_tile_gather, _lib.lib.tmdiff_tile_blend):
        assert fn(fake, fake, 1, 4, 16384, 16384, 64, 32, None) == -2
        assert b"32-bit" in _lib.lib.tmdiff_last_error_string()
        assert fn(fake, fake, 1, 4, 64, 64, 64, 40, None) == -1
        assert fn(None, None, 0, 4, 64, 64, 64, 16, None) == 0            # an empty batch is no work
