#!/usr/bin/env python3
"""Device time per scored item of ops.metrics_pair (all nine reduced-resolution metrics from one pass over the two images)
against the wall time of the host path the validation loop uses today (evaluate.to_hwc01 + metrics.ssim + metrics.sam: two of
the nine) on the same data and the same machine.  Needs the GPU; writes profiles/r07_metrics.txt.

    python tools/bench_metrics.py [--out profiles/r07_metrics.txt]

Device time: device events around `reps` back-to-back calls after a warm-up, median of 7 windows.  The byte count is "both
inputs read once" (2 * C * H * W * 4 bytes); the halo re-reads (22 x 70 staged for 16 x 64 owned: 1.50x) are on top of it, so
the achieved rate is a lower bound of what the memory system delivers."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(8, 256, 256), (8, 1024, 1024)]


def device_time(fn, reps, windows=7):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / reps * 1e-3)
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_metrics.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_metrics needs the GPU: nothing is measured without one")
    from tmdiff_amd import evaluate, metrics, ops

    lines = [f"# tools/bench_metrics.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             "# device: ops.metrics_pair (psnr sam ssim ergas rmse cc scc q q4), device events, median [min, max] of 7 windows",
             "# host  : evaluate.to_hwc01 x 2 + metrics.ssim + metrics.sam (the default val_dataset path), wall clock, median of 3",
             "# bytes : both inputs read once = 2 * C * H * W * 4"]
    for c, h, w in SHAPES:
        g = torch.Generator().manual_seed(1)
        hr = torch.rand(1, c, h, w, generator=g)
        sr = (hr + 0.05 * torch.randn(1, c, h, w, generator=g)).clamp(0, 1)
        hr_d, sr_d = hr.cuda(), sr.cuda()
        ws = ops.metrics_workspace(1, c, h, w, hr_d.device)
        out = torch.empty(1, 9, device="cuda", dtype=torch.float64)
        reps = max(20, int(2e8 / (c * h * w)))
        med, lo, hi = device_time(lambda: ops.metrics_pair(hr_d, sr_d, 1.0, out=out, workspace=ws), reps)
        nbytes = 2 * c * h * w * 4
        host = []
        for _ in range(3):
            t0 = time.perf_counter()
            a, b = evaluate.to_hwc01(hr_d), evaluate.to_hwc01(sr_d)          # includes the copy to the host, as the loop does
            s_host, a_host = metrics.ssim(a, b, 1), metrics.sam(a, b)
            host.append(time.perf_counter() - t0)
        host_med = statistics.median(host)
        row = dict(zip(metrics.PAIR_FIELDS, out[0].tolist()))
        lines += [f"{c}x{h}x{w}: device {med * 1e6:9.1f} us/item [{lo * 1e6:.1f}, {hi * 1e6:.1f}] ({reps} calls per window), "
                  f"{nbytes / med / 1e9:7.1f} GB/s of {nbytes / 1e6:.1f} MB; host {host_med * 1e3:9.1f} ms/item; "
                  f"host / device = {host_med / med:.0f}x",
                  f"    ssim device {row['ssim']:.12f} host {s_host:.12f}; sam device {row['sam']:.9f} host(fp32) {a_host:.9f}"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
