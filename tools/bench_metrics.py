#!/usr/bin/env python3
"""Device time per scored item of ops.metrics_pair (all nine reduced-resolution metrics from one pass over the two images)
against the wall time of the host path the validation loop uses today (evaluate.to_hwc01 + metrics.ssim + metrics.sam: two of
the nine) on the same data and the same machine.  Needs the GPU; writes profiles/r07_metrics.txt.

    python tools/bench_metrics.py [--out profiles/r07_metrics.txt] [--q2n-out profiles/r08_q2n.txt] [--hqnr-out profiles/hqnr.txt]
                                  [--leg pair|q2n|hqnr|all]

The Q2n leg times ops.metrics_q2n (blocks of 32 x 32 every 32 pixels) at 8 x 256 x 256 and 4 x 256 x 256 with B = 1 and B = 32
beside the float64 host metrics.q2n on the same data, and writes profiles/r08_q2n.txt.  Its arithmetic is counted as the C x C
cross products alone, 2 * C^2 flop per pixel of every block, against the MI355X's published fp64 vector peak (78.6 TFLOP/s).

The HQNR leg (only with --leg hqnr or all) times ops.metrics_dsblock alone and ops.metrics_hqnr whole at 8 x 1024 x 1024 ("WV3")
and 4 x 2048 x 2048 ("QB"), each replayed from a captured graph with borrowed buffers, then the parts of the chain one by one, and
the same filter and block moments composed from torch operators (replicate F.pad + grouped F.conv2d in fp32, F.unfold-based block
moments in fp64); it writes profiles/hqnr.txt.

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
HQNR_SHAPES = [(1, 8, 1024, 1024, "WV3"), (1, 4, 2048, 2048, "QB")]
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


def graph_time(fn, target=0.25, windows=7):
    """Device time per replay of ``fn`` captured into a graph: warmed up on the capture stream, then device events around enough
    back-to-back replays to fill ``target`` seconds, median / min / max of ``windows`` windows."""
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        fn()
    stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        fn()
    once, _, _ = device_time(graph.replay, 3, windows=1)
    reps = max(3, min(500, int(target / max(once, 1e-6))))
    return device_time(graph.replay, reps, windows) + (reps,)


def eager_time(fn, target=0.25, windows=7):
    once, _, _ = device_time(fn, 2, windows=1)
    reps = max(2, min(500, int(target / max(once, 1e-6))))
    return device_time(fn, reps, windows) + (reps,)


def torch_filter(ps, taps):
    """fir_decimate(ps, taps, 1) from torch operators: the border replicated, then one correlation per band."""
    import torch.nn.functional as F
    return F.conv2d(F.pad(ps, (20, 20, 20, 20), mode="replicate"), taps[:, None], groups=ps.shape[1])


def torch_d_s(ps, ms, pan, pan_lp, block=32):
    """metrics.d_s_block (q = 1, extents multiples of the block) from torch operators in fp64: F.unfold, then two-pass moments."""
    import torch.nn.functional as F

    def windows(x):
        x = x.double()
        return F.unfold(x, block, stride=block).reshape(x.shape[0], x.shape[1], block * block, -1)

    def q_mean(a, b):
        ma, mb = a.mean(2, keepdim=True), b.mean(2, keepdim=True)
        da, db = a - ma, b - mb
        n1 = a.shape[2] - 1.0
        q = 4.0 * ((da * db).sum(2) / n1) * ma[:, :, 0] * mb[:, :, 0] / ((da * da).sum(2) / n1 + (db * db).sum(2) / n1) \
            / (ma[:, :, 0] ** 2 + mb[:, :, 0] ** 2)
        return q.mean(2)

    return (q_mean(windows(ps), windows(pan)) - q_mean(windows(ms), windows(pan_lp))).abs().mean(1)


def hqnr_leg(path):
    from tmdiff_amd import metrics, ops
    fmt = lambda t: f"{t[0] * 1e6:9.1f} us [{t[1] * 1e6:.1f}, {t[2] * 1e6:.1f}] ({t[3]} per window)"
    lines = [f"# tools/bench_metrics.py --leg hqnr on {torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             "# device events around back-to-back calls after a warm-up; median [min, max] of 7 windows; block 32, ratio 4, q = 1",
             "# graph : replays of a captured graph, every buffer borrowed (ops.metrics_hqnr_buffers)",
             "# parts : the operators of the chain one by one, eager, into the same buffers",
             "# torch : the filter (replicate F.pad + grouped F.conv2d, fp32) and the block-wise D_s (F.unfold moments, fp64) from torch",
             "#         operators, eager, given the same low-pass PAN; neither Q2n nor the low-pass PAN is part of it"]
    for b, c, h, w, sensor in HQNR_SHAPES:
        g = torch.Generator().manual_seed(1)
        pan = torch.rand(b, 1, h, w, generator=g).cuda()
        ms = (0.6 * torch.rand(b, c, h, w, generator=g) + 0.4 * torch.rand(b, 1, h, w, generator=g)).cuda()
        ps = (0.6 * ms + 0.4 * pan).contiguous()
        buf = ops.metrics_hqnr_buffers(b, c, h, w, ps.device)
        out = torch.empty(b, 3, device="cuda", dtype=torch.float64)
        ops.metrics_hqnr(ps, ms, pan, sensor, out=out, buffers=buf)                     # uploads the tap tables
        ms_gains, pan_gain = metrics.mtf_gains(sensor, c)
        taps, pan_lp = ops._mtf_taps(ms_gains, 4, ps.device), buf["pan_lp"]
        whole = graph_time(lambda: ops.metrics_hqnr(ps, ms, pan, sensor, out=out, buffers=buf))
        ds = graph_time(lambda: ops.metrics_dsblock(ps, ms, pan, pan_lp, out=buf["d_s"], workspace=buf["ds_ws"]))
        parts = {"fir_decimate (41 x 41, full scale)": eager_time(lambda: ops.fir_decimate(ps, taps, 1, None, buf["filtered"])),
                 "metrics_q2n": eager_time(lambda: ops.metrics_q2n(ms, buf["filtered"], out=buf["q2n"], workspace=buf["q2n_ws"])),
                 "pan_lowpass": eager_time(lambda: ops.pan_lowpass(pan, pan_gain, 4, out=pan_lp, low=buf["pan_low"])),
                 "metrics_dsblock": eager_time(lambda: ops.metrics_dsblock(ps, ms, pan, pan_lp, out=buf["d_s"],
                                                                           workspace=buf["ds_ws"]))}
        t_filter = eager_time(lambda: torch_filter(ps, taps))
        t_ds = eager_time(lambda: torch_d_s(ps, ms, pan, pan_lp))
        want = torch_d_s(ps, ms, pan, pan_lp)
        total = sum(t[0] for t in parts.values())
        lines += [f"B={b} {c}x{h}x{w} {sensor}:",
                  f"  graph  metrics_hqnr whole   {fmt(whole)}",
                  f"  graph  metrics_dsblock      {fmt(ds)}"]
        lines += [f"  parts  {k:36s} {fmt(t)} = {100 * t[0] / total:5.1f} % of the parts" for k, t in parts.items()]
        lines += [f"  torch  pad + grouped conv2d {fmt(t_filter)}; torch / fir_decimate = "
                  f"{t_filter[0] / parts['fir_decimate (41 x 41, full scale)'][0]:.2f}x",
                  f"  torch  unfold D_s (fp64)    {fmt(t_ds)}; torch / metrics_dsblock (graph) = {t_ds[0] / ds[0]:.2f}x",
                  f"  d_lambda_k {float(out[0, 0]):.12f} d_s {float(out[0, 1]):.12f} (torch {float(want[0]):.12f}) hqnr {float(out[0, 2]):.12f}"]
    write(path, lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_metrics.txt"))
    ap.add_argument("--q2n-out", default=os.path.join(ROOT, "profiles", "r08_q2n.txt"))
    ap.add_argument("--hqnr-out", default=os.path.join(ROOT, "profiles", "hqnr.txt"))
    ap.add_argument("--leg", choices=("pair", "q2n", "hqnr", "all"), default="all")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_metrics needs the GPU: nothing is measured without one")
    from tmdiff_amd import evaluate, metrics, ops

    if args.leg in ("q2n", "all"):
        q2n_leg(args.q2n_out)
    if args.leg in ("hqnr", "all"):
        hqnr_leg(args.hqnr_out)
    if args.leg in ("q2n", "hqnr"):
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
