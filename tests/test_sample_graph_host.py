"""CPU-only tests of captured-graph sampling's host side: the new exports, the frame-slot rule the step kernel follows,
the device coefficient table and the switch.  No kernel is launched here."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

NEW = ("tmdiff_ddpm_step_dev", "tmdiff_sampler_tick", "tmdiff_ddpm_frame_slot")


def test_new_symbols_declared_and_exported():
    from tmdiff_amd import _lib, ops
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tmdiff_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared in include/tmdiff_hip.h"
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert callable(ops.ddpm_step_dev) and callable(ops.sampler_tick)
    assert _lib.ABI_VERSION == 6


def _eager_frame_steps(T, continous):
    """The timesteps whose frames p_sample_loop keeps, in the order it appends them (after x_T + MS)."""
    sample_inter = 1 | (T // 10)
    kept = [i for i in reversed(range(T)) if i % sample_inter == 0]
    return kept if continous else kept[-1:]          # (without continous only frames[-1] is returned)


@pytest.mark.parametrize("T", [1, 2, 10, 50, 1000])
@pytest.mark.parametrize("continous", [True, False])
def test_frame_slots_match_the_eager_loop(T, continous):
    from tmdiff_amd import sample_graph as sg
    every = sg.frame_every(T, continous)
    kept = _eager_frame_steps(T, continous)
    slots = {t: sg.frame_slot(t, T, every) for t in range(T) if t % every == 0}
    assert sorted(slots) == sorted(kept) if continous else 0 in slots
    if continous:
        assert [slots[t] for t in kept] == list(range(1, len(kept) + 1))
        assert sg.frame_count(T, every) == 1 + len(kept)
    else:
        assert slots[0] == sg.frame_count(T, every) - 1 == 1
    assert sg.frame_slot(-1, T, every) == -1 and sg.frame_slot(T, T, every) == -1


@pytest.mark.parametrize("schedule,T", [("cosine", 50), ("linear", 10), ("cosine", 1)])
def test_coef_table_reproduces_step_coef(schedule, T):
    from tmdiff_amd import sample_graph as sg
    from tmdiff_amd.diffusion_general import GeneralDiffusion
    diff = GeneralDiffusion(torch.nn.Identity())
    diff.set_new_noise_schedule({"schedule": schedule, "n_timestep": T}, "cpu")
    tab = sg.coef_table(diff._step_coef, "cpu")
    assert tab.dtype == torch.float32 and tab.shape == (T, 5)
    for t, row in enumerate(diff._step_coef):
        want = torch.tensor(list(row[:4]) + [row[4] if t > 0 else 0.0], dtype=torch.float32)
        assert torch.equal(tab[t], want), t
        assert tab[t].tolist() == [float(v) for v in want]     # the exact fp32 values the eager step is passed
    assert tab[0, 4].item() == 0.0
    if T > 1:
        assert (tab[1:, 4] > 0).all()


def test_sample_graph_switch():
    from tmdiff_amd import ops
    from tmdiff_amd.diffusion_general import GeneralDiffusion
    assert ops.config.sample_graph is False
    assert ops.KernelConfig(env={}).sample_graph is False
    assert ops.KernelConfig(env={"TMDIFF_SAMPLE_GRAPH": "1"}).sample_graph is True
    assert ops.KernelConfig(env={"TMDIFF_SAMPLE_GRAPH": "0"}).sample_graph is False
    assert "TMDIFF_SAMPLE_GRAPH" in ops.KernelConfig.__doc__
    assert GeneralDiffusion.sample_graphs is None and GeneralDiffusion.sample_graph_capacity == 2
    assert GeneralDiffusion.sample_graph_captures == 0


def test_cache_is_lru_and_copies_start_empty():
    import copy
    from tmdiff_amd import sample_graph as sg
    obj = object()
    c = sg.SampleGraphCache()
    keys = [sg._Key(("k", i), (obj,)) for i in range(3)]
    c.insert(keys[0], "a", 2)
    c.insert(keys[1], "b", 2)
    assert c.lookup(sg._Key(("k", 0), (obj,))) == "a"           # 0 becomes the most recent
    assert c.lookup(sg._Key(("k", 0), (object(),))) is None     # packed weights compared by identity
    c.insert(keys[2], "c", 2)                                    # evicts 1
    assert c.lookup(keys[1]) is None and c.lookup(keys[0]) == "a" and c.lookup(keys[2]) == "c"
    assert len(copy.deepcopy(c)) == 0
