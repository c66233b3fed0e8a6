"""Host side of global-norm gradient clipping inside the AdamW step (csrc/sampler.hip: multi_sqnorm_partial / _finish,
multi_adamw_scaled; tmdiff_amd.optim.FusedAdamW(max_grad_norm=...); train.max_grad_norm of the trainer): the exported names, the
entry points' refusals before any launch, the constructor's refusals, and the trainer's torch.optim.AdamW path against a
hand-written clip_grad_norm_ + step().  Nothing here touches the GPU."""
import copy
import re
import os

import pytest
import torch

NEW = ("tmdiff_multi_sqnorm_workspace_bytes", "tmdiff_multi_sqnorm_partial", "tmdiff_multi_sqnorm_finish",
       "tmdiff_multi_adamw_scaled")
E_INVALID = -1
P = 0x1000          # a non-NULL "pointer": every call below is refused before anything looks at it


def test_names_are_declared_exported_and_bound():
    import ctypes
    from tmdiff_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "tmdiff_hip.h")).read()
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared in include/tmdiff_hip.h"
        assert hasattr(dll, name) and name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["tmdiff_multi_adamw_scaled"][1]) == len(_lib.SIGNATURES["tmdiff_multi_adamw"][1]) + 2
    assert _lib.ABI_VERSION == 6


@pytest.mark.parametrize("n", (1, 2, 255, 256, 257, 5000, 1 << 20))
def test_workspace_holds_one_double_per_chunk(n):
    from tmdiff_amd._lib import lib
    assert lib.tmdiff_multi_sqnorm_workspace_bytes(n) >= 8 * n


def _refused(status, what):
    from tmdiff_amd._lib import lib
    assert status == E_INVALID, (what, status)
    assert what.encode() in lib.tmdiff_last_error_string()


def test_partial_refuses_bad_arguments_before_any_launch():
    from tmdiff_amd._lib import lib
    good = [P, P, P, 4, P]
    for k in (0, 1, 2, 4):                                   # each pointer NULL in turn
        args = list(good)
        args[k] = None
        _refused(lib.tmdiff_multi_sqnorm_partial(*args, None), "multi_sqnorm_partial")
    for n in (0, -1):
        _refused(lib.tmdiff_multi_sqnorm_partial(P, P, P, n, P, None), "multi_sqnorm_partial")


def test_finish_refuses_bad_arguments_before_any_launch():
    from tmdiff_amd._lib import lib
    good = [P, 4, 1.0, P, P, P]
    for k in (0, 3, 4, 5):
        args = list(good)
        args[k] = None
        _refused(lib.tmdiff_multi_sqnorm_finish(*args, None), "multi_sqnorm_finish")
    for n in (0, -3):
        _refused(lib.tmdiff_multi_sqnorm_finish(P, n, 1.0, P, P, P, None), "multi_sqnorm_finish")
    for bad in (0.0, -0.0, -1.0, float("nan"), float("-inf")):
        _refused(lib.tmdiff_multi_sqnorm_finish(P, 4, bad, P, P, P, None), "multi_sqnorm_finish")


def test_scaled_adamw_refuses_bad_arguments_before_any_launch():
    from tmdiff_amd._lib import lib
    good = [P, P, P, 4, P, P, 0.9, 0.999, 1e-8, 1e-2, P, P]
    for k in (0, 1, 2, 4, 5, 10, 11):
        args = list(good)
        args[k] = None
        _refused(lib.tmdiff_multi_adamw_scaled(*args, None), "multi_adamw_scaled")
    for n in (0, -1):
        args = list(good)
        args[3] = n
        _refused(lib.tmdiff_multi_adamw_scaled(*args, None), "multi_adamw_scaled")
    for k, bad in ((6, 1.0), (7, -0.1), (8, -1e-8), (9, -1.0)):          # the checks tmdiff_multi_adamw makes
        args = list(good)
        args[k] = bad
        _refused(lib.tmdiff_multi_adamw_scaled(*args, None), "multi_adamw_scaled")


@pytest.mark.parametrize("bad", (0, 0.0, -1, float("nan")))
def test_fused_adamw_refuses_a_bound_that_is_not_positive(bad):
    from tmdiff_amd.optim import FusedAdamW
    with pytest.raises(ValueError):
        FusedAdamW([torch.nn.Parameter(torch.zeros(3))], max_grad_norm=bad)


def test_fused_adamw_options_are_constructor_arguments_only():
    from tmdiff_amd.optim import FusedAdamW
    p = [torch.nn.Parameter(torch.zeros(3))]
    plain, clip = FusedAdamW(p, lr=1e-3), FusedAdamW(p, lr=1e-3, max_grad_norm=2.0, skip_nonfinite=False)
    assert plain.max_grad_norm is None and plain.skip_nonfinite is True
    assert clip.max_grad_norm == 2.0 and clip.skip_nonfinite is False
    assert clip.last_grad_norm is None and clip.last_step_ok is None
    assert clip.state_dict() == plain.state_dict()                   # neither option is saved


def test_chunk_tables_of_the_multi_tensor_kernels():
    """ops.chunk_tables, the one builder behind MultiAxpby and FusedAdamW: chunk -> (tensor, index within it) at the sizes
    around the chunk, and the entry bytes in both layouts (tmdiff_mt_entry: 4 x int64; tmdiff_adamw_entry: "<QQQQq")."""
    import struct
    from tmdiff_amd import ops
    from tmdiff_amd._lib import lib
    c = lib.tmdiff_multi_axpby_chunk()
    sizes = [1, c - 1, c, c + 1, 2 * c + 5]
    top = (1 << 63) - 16                                   # pointers up to the top of the positive int64 range
    mt = [(0x7F0000001000 + 64 * k, top - 64 * k, 0x10 + k, n) for k, n in enumerate(sizes)]
    adamw = [(0x7F0000001000 + 64 * k, 0x7E0000000004 + 64 * k, top - 64 * k, 0x20 + k, n) for k, n in enumerate(sizes)]
    for rows, fmt in ((mt, "<qqqq"), (adamw, "<QQQQq")):
        entries, chunk_tensor, chunk_index, n_chunks, host = ops.chunk_tables(rows, sizes, "cpu", pinned=False)
        assert host is None and n_chunks == 8
        assert chunk_tensor.dtype == chunk_index.dtype == torch.int32
        assert chunk_tensor.tolist() == [0, 1, 2, 3, 3, 4, 4, 4]
        assert chunk_index.tolist() == [0, 0, 0, 0, 1, 0, 1, 2]
        assert entries.numpy().tobytes() == b"".join(struct.pack(fmt, *row) for row in rows)
    entries, chunk_tensor, chunk_index, n_chunks, _ = ops.chunk_tables([], [], "cpu", pinned=False)
    assert n_chunks == 0 and entries.numel() == chunk_tensor.numel() == chunk_index.numel() == 0


# ---- the trainer on the torch.optim.AdamW path (CPU) -------------------------------------------------------------------------
def _opt(**train):
    return {"phase": "train", "gpu_ids": None, "distributed": False, "path": {"resume": None},
            "model": {"unet": {"channel_multiplier": [4, 8, 16, 32]}, "diffusion": {"loss_type": "l1"}, "init_type": "orthogonal"},
            "train": dict({"optimizer": {"lr": 1e-3}, "max_iter": 100}, **train)}


def _trained(net):
    return [p for n, p in net.named_parameters() if "clip_text" not in n]


def _surrogate_loss(net, it):
    """A loss of the parameters alone (the network's forward needs the GPU): gradients that differ from tensor to tensor and
    from step to step, large enough for the bound below to bite."""
    total = 0.0
    for k, p in enumerate(_trained(net)):
        c = torch.randn(p.shape, generator=torch.Generator().manual_seed(1000 * it + k))
        total = total + (p * c).sum() + 0.5 * (p * p).sum()
    return total


def _trainer(monkeypatch, **train):
    from tmdiff_amd.model import DDPM
    torch.manual_seed(11)
    m = DDPM(_opt(**train))
    assert type(m.optG) is torch.optim.AdamW
    state = {"it": 0}

    def forward(data, prompt):
        state["it"] += 1
        return _surrogate_loss(m.netG, state["it"])
    monkeypatch.setattr(m.netG, "forward", forward)
    return m


def test_trainer_clips_like_clip_grad_norm_on_the_torch_path(monkeypatch):
    from tmdiff_amd.model import linear_warmup_decay
    bound = 3.0
    m = _trainer(monkeypatch, max_grad_norm=bound)
    twin = copy.deepcopy(m.netG)
    opt = torch.optim.AdamW(_trained(twin), lr=1e-3, weight_decay=1e-4)
    sch = linear_warmup_decay(opt, 100, 100)
    norms = []
    for it in range(1, 5):                 # (the warm-up schedule starts at lr = 0: the first step moves nothing)
        m.feed_data({})
        m.optimize_parameters("WV3")
        opt.zero_grad(set_to_none=True)
        _surrogate_loss(twin, it).backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_(_trained(twin), bound)))
        opt.step()
        sch.step()
        log = m.get_current_log()
        assert log["grad_norm"] == norms[-1] and log["skipped"] == 0.0
        assert isinstance(log["grad_norm"], float) and isinstance(log["skipped"], float)
    assert min(norms) > bound                                                # the bound was active
    for (name, p), q in zip(m.netG.named_parameters(), twin.parameters()):
        assert torch.equal(p, q), name
    # ... and the clipped run is not the unclipped one
    free = _trainer(monkeypatch)
    for it in range(1, 5):
        free.feed_data({})
        free.optimize_parameters("WV3")
    assert any(not torch.equal(p, q) for p, q in zip(free.netG.parameters(), m.netG.parameters()))


def test_trainer_without_the_key_never_clips(monkeypatch):
    calls = []
    real = torch.nn.utils.clip_grad_norm_
    monkeypatch.setattr(torch.nn.utils, "clip_grad_norm_", lambda *a, **k: calls.append(1) or real(*a, **k))
    m = _trainer(monkeypatch)
    for _ in range(2):
        m.feed_data({})
        m.optimize_parameters("WV3")
    log = m.get_current_log()
    assert not calls and "grad_norm" not in log and "skipped" not in log and set(log) == {"l_pix", "lr"}
    m = _trainer(monkeypatch, max_grad_norm=1.0)
    m.feed_data({})
    m.optimize_parameters("WV3")
    assert len(calls) == 1
