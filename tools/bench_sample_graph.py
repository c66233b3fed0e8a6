#!/usr/bin/env python3
"""Captured-graph sampling against eager sampling through the public API (GeneralDiffusion.sample_graphs off / on), in one
process, alternating the two modes.  The graph side includes everything a user pays per call: input copies, the condition
graph, the per-step noise draw and the step-word set-up.  Also reports the first-call capture cost and checks that the two
modes return identical tensors.  Usage: python tools/bench_sample_graph.py [--reps N]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from tmdiff_amd.Hyper_unet_general import WavBEST  # noqa: E402
from tmdiff_amd.diffusion_general import GeneralDiffusion  # noqa: E402
from tmdiff_amd.util import fill_weights_, synthetic_tile_batch  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def compare(name, diff, call, work, unit, reps):
    """call(diff) in eager and graph mode; work = denoise steps (or NFE) per call.  Median of `reps` alternating runs."""
    diff.sample_graphs = False
    timed(lambda: call(diff))                                  # eager warm-up (packed weights, workspaces)
    diff.sample_graphs = True
    captures = diff.sample_graph_captures
    t_first, _ = timed(lambda: call(diff))                     # capture + first replay
    assert diff.sample_graph_captures == captures + 1
    eager, graph = [], []
    for r in range(reps):
        for mode, acc in ((False, eager), (True, graph)):
            diff.sample_graphs = mode
            torch.manual_seed(r)
            dt, out = timed(lambda: call(diff))
            acc.append((dt, out))
    same = all(torch.equal(e[1], g[1]) for e, g in zip(eager, graph))
    te = sorted(dt for dt, _ in eager)[reps // 2]
    tg = sorted(dt for dt, _ in graph)[reps // 2]
    diff.sample_graphs = None
    print(f"{name}: eager {te * 1e3:8.2f} ms ({work / te:7.1f} {unit}/s) | graph {tg * 1e3:8.2f} ms ({work / tg:7.1f} {unit}/s) "
          f"| x{te / tg:.2f} | first graph call (capture) {t_first * 1e3:.0f} ms | outputs identical: {same}", flush=True)
    return same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    print(f"device: {torch.cuda.get_device_name(0)}; median of {a.reps} alternating runs per mode", flush=True)
    net = fill_weights_(WavBEST(channels=[32, 64, 128, 256])).cuda().eval()
    ok = True
    for B, T in ((1, 50), (4, 10), (32, 10)):
        diff = GeneralDiffusion(net, "l1").cuda()
        diff.set_new_noise_schedule({"schedule": "cosine", "n_timestep": T}, "cuda")
        d = synthetic_tile_batch(3407, B, 8, 64, device="cuda")
        ok &= compare(f"config1 DDPM super_resolution B={B:2d} 8x64x64 T={T}", diff,
                      lambda g: g.super_resolution(d, False, "WV3", 3.0), T, "denoise-steps", a.reps)
    diff = GeneralDiffusion(net, "l1").cuda()
    diff.set_new_noise_schedule({"schedule": "cosine", "n_timestep": 1000}, "cuda")
    d = synthetic_tile_batch(3407, 1, 8, 64, device="cuda")
    ok &= compare("DPM-Solver++ 20 steps (21 NFE) B= 1 8x64x64", diff, lambda g: g.sample_by_dpmsolver(d, "WV3", steps=20),
                  21, "NFE", a.reps)
    if not ok:
        sys.exit("graph and eager outputs differ")


if __name__ == "__main__":
    main()
