#!/usr/bin/env python3
"""The opt-in bf16 gradient arithmetic of the finetune step (ops.config.grad_bf16) against the fp32 step, in ONE process:

  --agreement   per-parameter relative L2 difference of the gradients, bf16 against fp32 arithmetic, on the small network of
                tests/test_gpu_train_bf16.py over three seeds (the table that test's bound is four times the maximum of);
  --layers      per layer class of the 32-256 network at local batch 8: the bf16 weight gradient against
                tmdiff_conv3d_wgrad_wino, the bf16 data gradient against conv3d_wf (HIP events, median of --reps);
  --step        the finetune step of bench.py --full's train_step configuration (local batch 8, 8 bands, 64x64, widths 32-256):
                eager and from the HIP graph, switch off and on, median and spread (max - min) over --reps timed steps.

Without a flag all three run.  Prints the tables; `> profiles/train_bf16_grad.txt` keeps them."""
import argparse
import copy
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from tmdiff_amd import ops, routing
from tmdiff_amd.util import fill_weights_, synthetic_tile_batch

SMALL = dict(channels=[32, 32, 32, 32], b=2, bands=4, size=16)      # tests/test_gpu_train_bf16.py


def small_grads(seed, bf16, loss_type="l1"):
    """(loss, {name: gradient}) of one finetune forward + backward of the small network, dropout on, everything seeded."""
    from tmdiff_amd.Hyper_unet_general import WavBEST
    from tmdiff_amd.diffusion_general import GeneralDiffusion
    c = SMALL
    net = fill_weights_(WavBEST(channels=c["channels"]), seed=seed).cuda().train()
    diff = GeneralDiffusion(net, loss_type).cuda()
    diff.set_loss("cuda")
    diff.set_new_noise_schedule({"schedule": "cosine", "n_timestep": 1000}, "cuda")
    d = synthetic_tile_batch(5000 + seed, c["b"], c["bands"], c["size"], device=torch.device("cuda"))
    t = np.random.RandomState(seed).randint(1, 1001, size=c["b"])
    t_dev = torch.from_numpy(t).view(c["b"], 1).cuda()
    a_dev = torch.tensor(diff.sqrt_alphas_cumprod_prev[t], dtype=torch.float32).cuda()
    noise = torch.randn(c["b"], c["bands"], c["size"], c["size"], generator=torch.Generator().manual_seed(seed)).cuda()
    torch.manual_seed(seed)                      # the dropout seeds are drawn from the host generator
    with ops.config.override(wino_min_blocks=1, grad_bf16=bf16):
        loss = diff.p_losses_with(d, "WV3", t_dev, a_dev, noise).sum()
        loss.backward()
    return float(loss), {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}


def agreement(seeds=(0, 1, 2)):
    print("# gradient agreement, bf16 against fp32 gradient arithmetic: small network " + str(SMALL) + ", dropout on, L1 loss")
    print("# per parameter tensor: relative L2 difference; worst tensors per seed, then the summary")
    worst_all, cos_all = 0.0, 1.0
    for s in seeds:
        l32, g32 = small_grads(s, False)
        l16, g16 = small_grads(s, True)
        assert l32 == l16 and g32.keys() == g16.keys()
        rows = sorted(((float((g16[k] - g32[k]).norm() / g32[k].norm().clamp_min(1e-30)), k) for k in g32), reverse=True)
        a, b = torch.cat([g32[k].reshape(-1) for k in g32]).double(), torch.cat([g16[k].reshape(-1) for k in g32]).double()
        cos = float((a @ b) / (a.norm() * b.norm()))
        worst_all, cos_all = max(worst_all, rows[0][0]), min(cos_all, cos)
        print(f"seed {s}: loss {l32:.6f} (identical bits), {len(rows)} tensors, cosine of the full gradient vectors {cos:.6f}")
        for r, k in rows[:5]:
            print(f"    {r:.3e}  {k}")
        print(f"    median {statistics.median(r for r, _ in rows):.3e}")
    print(f"largest relative L2 difference over the seeds: {worst_all:.3e}; smallest cosine: {cos_all:.6f}")


def _time(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(ts), max(ts) - min(ts)


def layers(reps):
    """One row per distinct (Cin, Cout, groups, plane) of the 3x3x3 convolutions of the 32-256 finetune step at batch 8."""
    from tmdiff_amd import autograd as A
    b, n = 8, 8
    seen = {}
    for r in routing.unet_train_launches(routing.FULL, b, n, 64, 64, True).convs:
        if r.ksize == 3:
            seen.setdefault((r.cin, r.cout, r.groups, r.h, r.w), []).append(r.name)
    print(f"# per layer class (B = {b}, {n} bands), microseconds, median of {reps} (spread = max - min): weight gradient on a kept x'")
    print("# (one plain tensor), data gradient of g;  fp32 = the families the fp32 step runs (wgrad_wino / conv3d_wf ...);  ratio = fp32 /")
    print("# bf16 time: a pass whose ratio is below 1 in a class is routed to fp32 there (routing rule 6b)")
    print(f"{'Cin':>4} {'Cout':>4} {'g':>1} {'plane':>7} {'layers':>6} | {'wgrad fp32':>10} {'bf16':>8} {'spread':>7} {'ratio':>5} | "
          f"{'dgrad fp32':>10} {'bf16':>8} {'spread':>7} {'ratio':>5}")
    for (cin, cout, g, h, w), names in sorted(seen.items(), key=lambda kv: (-kv[0][3], kv[0][0], kv[0][1])):
        x = torch.randn(b, cin, n, h, w, device="cuda")
        gy = torch.randn(b, cout, n, h, w, device="cuda")
        wt = torch.randn(cout, cin // g, 3, 3, 3, device="cuda") * 0.05
        desc = ops.make_conv_desc([x], 0, cout, 3, gy, groups=g)
        wshape = tuple(wt.shape)
        w32, _ = _time(lambda: ops.conv3d_wgrad(desc, gy, wshape), reps)
        w16, ws = _time(lambda: ops.conv3d_wgrad_bf16(desc, gy, wshape), reps)
        fam = routing.conv3_family(b, cout, cin, n, h, w, g)
        wp = ops.pack_conv_weight(wt, g, mode=1)
        weights = ops.ConvWeights(lambda: wp, lambda: ops.pack_conv_weight_wino(wt, g, mode=3, planes=6),
                                  lambda planes: ops.pack_conv_weight_wino(wt, g, mode=1, planes=planes))
        pk = weights.wf() if fam in ("wf", "wf_pair") else None
        if pk is not None:
            weights = ops.ConvWeights(lambda: wp, lambda: pk)
        d32, _ = _time(lambda: ops.conv3d_auto([gy], weights, cin, groups=g, family=fam), reps)
        if routing.dgrad_bf16_ok(b, cin, cout, n, h, w, g) or (cin // g) % 32 == 0 and (cout // g) % 8 == 0:
            wb = ops.pack_conv_weight_bf16_dgrad(wt, g)
            d16, dsp = _time(lambda: ops.conv3d([gy], wb, cin, 3, groups=g, math="bf16"), reps)
        else:
            d16 = dsp = float("nan")
        print(f"{cin:>4} {cout:>4} {g:>1} {h:>3}x{w:<3} {len(names):>6} | {w32:>10.1f} {w16:>8.1f} {ws:>7.1f} {w32 / w16:>5.2f} | "
              f"{d32:>10.1f} {d16:>8.1f} {dsp:>7.1f} {d32 / d16:>5.2f}   {fam}")
        del x, gy, wt


def step_times(reps, warmup):
    from tmdiff_amd.model import DDPM
    print(f"# finetune step, local batch 8, 8 bands, 64x64, widths 32-256, dropout on: milliseconds per step, median of {reps} "
          "(spread = max - min), host-timed with a device synchronisation per step")
    d = synthetic_tile_batch(4000, 8, 8, 64, device=torch.device("cuda"))
    d["LR"] = d["MS"]
    out = {}
    for graph in (False, True):
        for mode in ("fp32", "bf16"):
            opt = {"phase": "train", "gpu_ids": [0], "distributed": False, "path": {"resume": None},
                   "model": {"unet": {"channel_multiplier": list(routing.FULL)}, "diffusion": {"loss_type": "l1"}, "init_type": "orthogonal"},
                   "train": {"optimizer": {"lr": 1e-4}, "max_iter": 150000, "hip_graph": graph, "grad_compute": mode}}
            m = DDPM(opt)
            fill_weights_(m.netG.denoise_fn)
            m.netG.denoise_fn.invalidate_prepared()
            m.set_new_noise_schedule({"schedule": "cosine", "n_timestep": 1000}, "train")
            np.random.seed(3407)
            torch.manual_seed(3407)
            ts = []
            for it in range(warmup + reps):
                m.feed_data(dict(d))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                m.optimize_parameters("WV3")
                torch.cuda.synchronize()
                if it >= warmup:
                    ts.append(1e3 * (time.perf_counter() - t0))
            out[(graph, mode)] = (statistics.median(ts), max(ts) - min(ts), float(m.get_current_log()["l_pix"]))
            print(f"{'graph' if graph else 'eager':>5} {mode}: {out[(graph, mode)][0]:7.2f} ms  spread {out[(graph, mode)][1]:5.2f}  "
                  f"(last loss {out[(graph, mode)][2]:.4f})", flush=True)
            del m
            torch.cuda.empty_cache()
    for graph in (False, True):
        a, b_ = out[(graph, "fp32")], out[(graph, "bf16")]
        gain, noise = a[0] - b_[0], max(a[1], b_[1])
        print(f"{'graph' if graph else 'eager'}: bf16 gradients {'faster' if gain > noise else 'NOT faster'} than fp32 by {gain:.2f} ms "
              f"({a[0] / b_[0]:.2f}x), run-to-run spread {noise:.2f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agreement", action="store_true")
    ap.add_argument("--layers", action="store_true")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=4)
    args = ap.parse_args()
    everything = not (args.agreement or args.layers or args.step)
    if args.agreement or everything:
        agreement()
    if args.layers or everything:
        layers(args.reps)
    if args.step or everything:
        step_times(args.reps, args.warmup)


if __name__ == "__main__":
    main()
