#!/usr/bin/env python3
"""Fused tiled sampling (tiling.TiledDenoiser) on a 4-band 512x512 scene at full width, overlap 0 / 8 / 32:
  * ms per denoise step of the fused denoiser (condition branch cached, as inside a sampling run);
  * ms of the same number of tiles through the network alone in batches of 32 (the independent mode's work per step);
  * time and GB/s (algorithmic bytes: tiles read or written + scene written or read) of tile_gather and tile_blend;
  * the seam statistic of a 4-band 256x256 scene after a 5-step DPM-Solver++ run with the same injected scene noise, for
    the independent mode and overlap 8 / 16 / 32: mean |difference| across the 64-pixel tile borders over the mean
    |difference| between all other neighbouring columns and rows (1 = no visible border).
Device events, warm-up, median of --reps repeats.  Usage: python tools/bench_tiled.py [--reps N] [--no-seams]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from tmdiff_amd import ops  # noqa: E402
from tmdiff_amd.Hyper_unet_general import WavBEST  # noqa: E402
from tmdiff_amd.diffusion_general import GeneralDiffusion  # noqa: E402
from tmdiff_amd.tiling import TiledDenoiser, plan_tiles, sample_tiled  # noqa: E402
from tmdiff_amd.util import fill_weights_, synthetic_tile_batch  # noqa: E402


def timed(fn, reps, inner=1):
    """median over `reps` of the device time of `inner` calls, in ms per call"""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / inner)
    return sorted(out)[len(out) // 2]


def seam_ratio(img, tile=64):
    dx, dy = (img[..., :, 1:] - img[..., :, :-1]).abs(), (img[..., 1:, :] - img[..., :-1, :]).abs()
    bx = torch.zeros(dx.shape[-1], dtype=torch.bool, device=img.device)
    by = torch.zeros(dy.shape[-2], dtype=torch.bool, device=img.device)
    bx[tile - 1::tile] = True
    by[tile - 1::tile] = True
    seam = torch.cat([dx[..., :, bx].reshape(-1), dy[..., by, :].reshape(-1)]).mean()
    rest = torch.cat([dx[..., :, ~bx].reshape(-1), dy[..., ~by, :].reshape(-1)]).mean()
    return float(seam / rest)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-seams", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    print(f"device: {torch.cuda.get_device_name(0)}; device events, warm-up, median of {a.reps} repeats", flush=True)
    net = fill_weights_(WavBEST(channels=[32, 64, 128, 256])).cuda().eval()
    d = synthetic_tile_batch(7, 1, 4, 512, device="cuda")
    t = torch.full((1, 1), 500.0, device="cuda")
    with torch.no_grad():
        for overlap in (0, 8, 32):
            rows, cols = plan_tiles(512, 512, 64, overlap)
            n = len(rows) * len(cols)
            tiled = TiledDenoiser(net, 64, overlap, 32)
            tiled.begin_condition_cache(d["PAN"], d["MS"], "GF2")
            step = timed(lambda: tiled(d["x_t"], t, d["PAN"], d["MS"], "GF2"), a.reps)
            tiled.end_condition_cache()
            # the same tiles through the network alone: chunks of 32, each chunk's condition cached in turn
            xt, pan, ms = (ops.tile_gather(d[k], 64, overlap) for k in ("x_t", "PAN", "MS"))
            alone = 0.0
            for lo in range(0, n, 32):
                x_, p_, m_ = xt[lo:lo + 32], pan[lo:lo + 32], ms[lo:lo + 32]
                tt = torch.full((x_.shape[0], 1), 500.0, device="cuda")
                net.begin_condition_cache(p_, m_, "GF2")
                alone += timed(lambda: net(x_, tt, p_, m_, "GF2"), a.reps)
                net.end_condition_cache()
            y = torch.randn_like(xt)
            scene = torch.empty_like(d["x_t"])
            nbytes = (xt.numel() + scene.numel()) * 4
            g_ms = timed(lambda: ops.tile_gather(d["x_t"], 64, overlap, out=xt), a.reps, inner=50)
            b_ms = timed(lambda: ops.tile_blend(y, 1, 512, 512, overlap, out=scene), a.reps, inner=50)
            print(f"512x512x4 overlap {overlap:2d}: {n:3d} tiles | fused step {step:7.2f} ms | tiles through net alone {alone:7.2f} ms "
                  f"| gather {g_ms * 1e3:6.1f} us {nbytes / g_ms / 1e6:6.0f} GB/s | blend {b_ms * 1e3:6.1f} us "
                  f"{nbytes / b_ms / 1e6:6.0f} GB/s | {nbytes / 1e6:.1f} MB each | gather + blend = "
                  f"{(g_ms + b_ms) / step * 100:.2f} % of the step (copy rate of the box: 6290 GB/s, profiles/r04_hbm_kernels.txt)",
                  flush=True)
        if a.no_seams:
            return
        s = synthetic_tile_batch(11, 1, 4, 256, device="cuda")
        scene_in = {"MS": s["MS"], "PAN": s["PAN"]}
        noise = torch.randn(1, 4, 256, 256, generator=torch.Generator().manual_seed(3))
        for overlap in (None, 8, 16, 32):
            if overlap is None:   # the independent mode draws per batch of tiles: hand it the same scene noise, cut into its tiles
                from tmdiff_amd.tiling import split_tiles
                fn = lambda like: split_tiles(noise, 64, 64)[:like.shape[0]]
            else:
                fn = lambda like: noise
            diff = GeneralDiffusion(net, "l1", noise_fn=fn).cuda()
            diff.set_new_noise_schedule({"schedule": "cosine", "n_timestep": 1000}, "cuda")
            out = sample_tiled(diff, scene_in, "GF2", tile=64, method="dpmsolver", steps=5, max_batch=32, overlap=overlap)
            res = out - s["MS"]
            print(f"seam statistic, 256x256x4, DPM-Solver++ 5 steps, {'independent' if overlap is None else f'overlap {overlap:2d}':>11s}: "
                  f"fused image {seam_ratio(out):.3f}, residual (image - MS) {seam_ratio(res):.3f}", flush=True)


if __name__ == "__main__":
    main()
