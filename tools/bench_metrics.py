#!/usr/bin/env python3
"""Device time per scored item of ops.metrics_pair (all nine reduced-resolution metrics from one pass over the two images)
against the wall time of the host path the validation loop uses today (evaluate.to_hwc01 + metrics.ssim + metrics.sam: two of
the nine) on the same data and the same machine.  Needs the GPU; writes profiles/r07_metrics.txt.

    python tools/bench_metrics.py [--out profiles/r07_metrics.txt] [--q2n-out profiles/r08_q2n.txt] [--leg pair|q2n|all]

The Q2n leg times ops.metrics_q2n (blocks of 32 x 32 every 32 pixels) at 8 x 256 x 256 and 4 x 256 x 256 with B = 1 and B = 32
beside the float64 host metrics.q2n on the same data, and writes profiles/r08_q2n.txt.  Its arithmetic is counted as the C x C
cross products alone, 2 * C^2 flop per pixel of every block, against the MI355X's published fp64 vector peak (78.6 TFLOP/s).

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
Q2N_SHAPES = [(1, 8, 256, 256), (32, 8, 256, 256), (1, 4, 256, 256), (32, 4, 256, 256)]
FP64_VECTOR_PEAK = 78.6e12


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


def write(path, lines):
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(text)


def q2n_leg(path):
    from tmdiff_amd import metrics, ops
    lines = [f"# tools/bench_metrics.py --leg q2n on {torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             "# device: ops.metrics_q2n, block 32, shift 32, borrowed workspace; device events, median [min, max] of 7 windows",
             "# host  : metrics.q2n (float64 NumPy) on the same data, one image, wall clock, median of 3",
             "# flop  : the cross products alone, 2 * C^2 per pixel of every block; peak = 78.6 TFLOP/s fp64 vector"]
    for b, c, h, w in Q2N_SHAPES:
        g = torch.Generator().manual_seed(1)
        hr = torch.rand(b, c, h, w, generator=g)
        sr = (hr + 0.05 * torch.randn(b, c, h, w, generator=g)).clamp(0, 1)
        hr_d, sr_d = hr.cuda(), sr.cuda()
        ws = ops.metrics_q2n_workspace(b, c, h, w, hr_d.device)
        out = torch.empty(b, device="cuda", dtype=torch.float64)
        reps = 200 if b == 1 else 50
        med, lo, hi = device_time(lambda: ops.metrics_q2n(hr_d, sr_d, out=out, workspace=ws), reps)
        ny, nx = ops.q2n_grid(h, w, 32, 32)
        flop = 2.0 * metrics.q2n_bands(c) ** 2 * 1024 * ny * nx * b
        host = []
        for _ in range(3):
            t0 = time.perf_counter()
            v_host = metrics.q2n(hr[0].numpy(), sr[0].numpy(), hwc=False)
            host.append(time.perf_counter() - t0)
        host_med = statistics.median(host)
        lines += [f"B={b:2d} {c}x{h}x{w}: device {med * 1e6:8.1f} us/call [{lo * 1e6:.1f}, {hi * 1e6:.1f}] = {med / b * 1e6:7.2f} us/image "
                  f"({reps} calls per window), {flop / med / 1e12:6.3f} TFLOP/s = {100 * flop / med / FP64_VECTOR_PEAK:5.2f} % of peak; "
                  f"host {host_med * 1e3:7.1f} ms/image; host / device = {host_med / (med / b):.0f}x",
                  f"    q2n device {float(out[0]):.12f} host {v_host:.12f}"]
    write(path, lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_metrics.txt"))
    ap.add_argument("--q2n-out", default=os.path.join(ROOT, "profiles", "r08_q2n.txt"))
    ap.add_argument("--leg", choices=("pair", "q2n", "all"), default="all")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_metrics needs the GPU: nothing is measured without one")
    from tmdiff_amd import evaluate, metrics, ops

    if args.leg in ("q2n", "all"):
        q2n_leg(args.q2n_out)
    if args.leg == "q2n":
        return
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
    write(args.out, lines)


if __name__ == "__main__":
    main()
