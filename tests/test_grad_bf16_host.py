"""Host side of the opt-in bf16 gradient arithmetic (ops.config.grad_bf16): exported symbols, the switch, routing's eligibility
over the BASELINE widths, plans unchanged with the switch off, the trainer option.  No GPU."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("tmdiff_conv3d_wgrad_bf16_supported", "tmdiff_conv3d_wgrad_bf16_workspace_bytes", "tmdiff_conv3d_wgrad_bf16",
               "tmdiff_conv3d_pack_weights_bf16_dgrad")


def test_new_symbols_are_exported_and_declared():
    from tmdiff_amd import _lib
    header = open(os.path.join(ROOT, "include", "tmdiff_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(_lib.lib, name) and name in _lib.SIGNATURES and name + "(" in header, name
    # the byte count of the data-gradient packing is the forward packing's with the channel counts swapped
    assert _lib.lib.tmdiff_conv3d_packed_bf16_bytes(32, 40, 3, 1) == 40 // 8 * 28 * 32 * 16


def test_support_query_without_a_gpu():
    from tmdiff_amd import routing
    q = lambda cin, cout, groups=1, **f: routing.supported("tmdiff_conv3d_wgrad_bf16_supported", 2, cin, cout, 4, 8, 8, groups, **f)
    assert q(8, 32) and q(40, 32) and q(24, 96, 3) and q((8, 8, 16), 64, in_act=1)
    assert not q(4, 32) and not q(8, 16) and not q(12, 96, 3)
    d = __import__("tmdiff_amd")._lib.Conv3dDesc()
    d.B, d.N, d.H, d.W, d.Cin, d.Cout, d.groups, d.ksize, d.nseg = 2, 4, 8, 8, 32, 32, 1, 1, 1
    assert not __import__("tmdiff_amd")._lib.lib.tmdiff_conv3d_wgrad_bf16_supported(C.byref(d))       # 1x1x1
    d.ksize, d.groups, d.Cin = 3, 2, 16
    assert not __import__("tmdiff_amd")._lib.lib.tmdiff_conv3d_wgrad_bf16_supported(C.byref(d))       # groups 2


def test_kernel_config_field():
    from tmdiff_amd import ops
    assert "grad_bf16" in ops.KernelConfig._FIELDS and ops.KernelConfig._FIELDS["grad_bf16"][0] == "TMDIFF_GRAD_BF16"
    assert ops.KernelConfig(env={}).grad_bf16 is False
    assert ops.KernelConfig(env={"TMDIFF_GRAD_BF16": "1"}).grad_bf16 is True
    assert "grad_bf16" in ops.KernelConfig.__doc__
    off = ops.KernelConfig(env={})
    on = ops.KernelConfig(env={"TMDIFF_GRAD_BF16": "1"})
    assert off.key() != on.key() and len(off.key()) == len(ops.KernelConfig._FIELDS)
    with ops.config.override(grad_bf16=True):
        k_on = ops.config.key()
    assert k_on != ops.config.key() or ops.config.grad_bf16


@pytest.mark.parametrize("channels", [[32, 64, 128, 256], [64, 128, 256, 512]])
def test_every_body_convolution_of_the_baseline_widths_is_eligible(channels):
    """Every BASELINE configuration of these widths (routing.BASELINE_CASES: batches 1 / 8 / 32, 4 and 8 bands, 64^2 / 256^2),
    dropout off and on: with the switch on the data gradient of every 3x3x3 convolution is bf16, the 1x1x1 ones never.  The
    weight gradients stay on the families the switch-off plan gives them: the bf16 weight-gradient kernel is eligible for every one
    of these shapes (its support query says so) but measured slower than the fp32 Winograd weight gradient in every layer class
    (profiles/train_bf16_grad.txt), and a slower class is routed to fp32."""
    from tmdiff_amd import ops, routing
    cases = {(b, n, size) for _, ch, b, n, size, _ in routing.BASELINE_CASES if list(ch) == channels}
    assert cases
    for b, n, size in sorted(cases):
        for dropout in (False, True):
            off = routing.unet_train_launches(channels, b, n, size, size, dropout).convs
            with ops.config.override(grad_bf16=True):
                rows = routing.unet_train_launches(channels, b, n, size, size, dropout).convs
                assert sum(r.ksize == 3 for r in rows) >= 50
                for r, r0 in zip(rows, off):
                    assert (r.name, r.fwd, r.keep_xp, r.wgrad, r.bias_in_wgrad) == (r0.name, r0.fwd, r0.keep_xp, r0.wgrad, r0.bias_in_wgrad)
                    if r.ksize == 3:
                        assert r.dgrad == "bf16" and r.wgrad in ("wino", "direct"), (b, n, size, r)
                        assert routing.dgrad_bf16_ok(b, r.cin, r.cout, n, r.h, r.w, r.groups)
                        assert routing.supported("tmdiff_conv3d_wgrad_bf16_supported", b, r.cin, r.cout, n, r.h, r.w, r.groups)
                    else:
                        assert (r.dgrad, r.wgrad) == ("k1", "direct"), r


def _all_plans():
    from tmdiff_amd import routing
    out = []
    for _, ch, b, n, size, switches in routing.TRAIN_CASES:
        for dropout in (False, True):
            r = routing.unet_train_launches(ch, b, n, size, size, dropout)
            out.append((tuple(r.convs), tuple(map(tuple, r.blocks)), tuple(sorted(r.counts.items()))))
    return out


def test_plans_are_unchanged_with_the_switch_off(monkeypatch):
    """train_conv_plan / train_ll_plan for every convolution of every TRAIN_CASES network: the switch off gives what a
    configuration WITHOUT the field gives (the routing code reads it with a default), fwd and keep_xp never depend on it, and no
    plan mentions bf16."""
    from tmdiff_amd import ops, routing
    with ops.config.override(grad_bf16=False):
        off = _all_plans()
    assert "'bf16'" not in repr(off) and "bf16" not in repr([o[2] for o in off])

    class Absent:                                   # ops.config without the field
        def __getattr__(self, name):
            if name == "grad_bf16":
                raise AttributeError(name)
            return getattr(ops.config, name)

        def key(self):
            return ("absent",) + tuple(v for k, v in ops.config.as_dict().items() if k != "grad_bf16")
    monkeypatch.setattr(routing, "_config", lambda: Absent())
    assert _all_plans() == off
    monkeypatch.undo()
    with ops.config.override(grad_bf16=True):
        on = _all_plans()
    for (c0, b0, _), (c1, b1, _) in zip(off, on):
        assert b0 == b1 and [(r.name, r.fwd, r.keep_xp, r.wgrad) for r in c0] == [(r.name, r.fwd, r.keep_xp, r.wgrad) for r in c1]
    p = routing.train_conv_plan(8, (64,), 64, 8, 32, 32, 1, 3, True, False, True, True)
    assert tuple(p) == (p.fwd, p.keep_xp, p.dgrad, p.wgrad, p.bias_in_wgrad) and (p.dgrad_math, p.wgrad_math) == ("fp32", "fp32")


def test_trainer_option_is_parsed(tmp_path):
    import json
    import torch
    from tmdiff_amd import config, ops
    from tmdiff_amd.model import DDPM
    base = {"name": "t", "phase": "train", "gpu_ids": None, "path": {"resume_state": None, "log": "logs"},
            "model": {"unet": {"channel_multiplier": [4, 8, 16, 32]}, "diffusion": {"loss_type": "l1"}, "init_type": "orthogonal",
                      "beta_schedule": {}},
            "datasets": {}, "train": {"optimizer": {"lr": 1e-3}, "max_iter": 100}}
    path = tmp_path / "opt.json"
    for value, ok in (("bf16", True), ("fp32", True), (None, True), ("fp16", False)):
        o = json.loads(json.dumps(base))
        if value is not None:
            o["train"]["grad_compute"] = value
        path.write_text(json.dumps(o))
        if not ok:
            with pytest.raises(ValueError):
                config.parse(str(path), "train", root=str(tmp_path), make_dirs=False)
            continue
        parsed = config.parse(str(path), "train", root=str(tmp_path), make_dirs=False)
        assert parsed["train"]["grad_compute"] == value
    opt = {"phase": "train", "gpu_ids": None, "distributed": False, "path": {"resume": None},
           "model": {"unet": {"channel_multiplier": [4, 8, 16, 32]}, "diffusion": {"loss_type": "l1"}, "init_type": "orthogonal"},
           "train": {"optimizer": {"lr": 1e-3}, "max_iter": 100, "grad_compute": "bf16"}}
    torch.manual_seed(3)
    m = DDPM(opt)
    assert m.grad_compute == "bf16"
    seen = []
    m.netG.forward = lambda data, prompt: (seen.append(ops.config.grad_bf16), sum((p * p).sum() for p in m.netG.parameters()
                                                                                 if p.requires_grad))[1]
    m.feed_data({})
    m.optimize_parameters("WV3")
    assert seen == [True] and ops.config.grad_bf16 is False          # on inside the step, restored after it
    opt["train"].pop("grad_compute")
    assert DDPM(opt).grad_compute is None
    opt["train"]["grad_compute"] = "int8"
    with pytest.raises(ValueError):
        DDPM(opt)
    assert "--grad-bf16" in open(os.path.join(ROOT, "examples", "finetune_synthetic.py")).read()
