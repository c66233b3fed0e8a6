#!/usr/bin/env python3
"""What the composite finetune loss (tmdiff_amd.losses.SpectralSpatialLoss; csrc/loss.hip) costs.

Per shape ([8, 8, 64, 64], the finetune step's, and [32, 8, 64, 64]) it times
  the kernel pair, gradient mode and value-only mode      (ops.spectral_spatial_loss: loss_kernel + loss_finalize_kernel)
  the same loss and its backward composed from torch operators in fp32 on the device (norms, atan2, conv2d, their autograd)
each as a HIP graph of CALLS back-to-back evaluations replayed REPS times -- the device's time per evaluation, launch gaps
included, without the host's enqueue cost -- and once more eagerly from the host.  Beside the pair: 16 bytes per element (x0,
xhat, MS read, g written) over its time.  Expectation, stated before the run: at 4 - 17 MB the pair is bound by launch latency,
not by HBM (4 MB at 6 TB/s is 0.7 us), so it should sit near the floor of two dependent launches that tile_gather / tile_blend
show (7 - 8 us each, profiles/r06_tiled_fused.txt) and its bytes / time should be far below the copy rate.

With --step it also times the captured finetune step (model.DDPM, ch 32-256, batch 8 of 8 x 64 x 64, HIP graph) with the terms
on against the same step with plain l1 -- in which none of the new code runs -- alternating the two in one process.

--leg ssim times the SSIM term instead (tmdiff_amd.losses.SSIMLoss; csrc/ssim_loss.hip: ssim_loss_kernel + ssim_finalize_kernel,
7 x 7 windows) at the same two shapes against 1 - SSIM composed from five grouped conv2d box filters and their autograd in fp32,
and with --step the captured step with loss_terms = {"dssim": 0.1} against plain l1.  Beside the pair: 12 bytes per element
(x_true, x_pred read, g written) over its time.  Expectation, stated before the run: the kernel reads every staged value
about win + 3 times from LDS and forms 5 n fp64 multiply-adds per window, so unlike the composite pair it is bound by its own
arithmetic and LDS reads, a few tens of microseconds at these sizes, not by launch latency.

--leg lcorr times the local PAN-correlation loss (tmdiff_amd.losses.LocalCorrLoss; csrc/local_corr.hip: local_corr_kernel +
local_corr_finalize, 4 x 4 windows, rho_max 1) at [8, 8, 64, 64] and at [1, 8, 1024, 1024], a full-resolution scene, value-only
and with the gradient, against mean max(0, 1 - rho) composed from five F.avg_pool2d box filters, elementwise operators and their
autograd in fp32 (one-pass moments and a clamp where the kernel has two-pass sums and exact zeros).  Beside the pair: bytes moved
(x and pan read, g written) over its time.  Expectation, stated before the run: the small shape has 64 workgroups of 8 bands
each on 256 CUs and is bound by the latency of two dependent launches plus one workgroup's walk over its bands; the large
shape has 2048 workgroups, reads 36 MB and writes 32 MB (11 us at the copy rate) and does about 100 fp64 operations per window
and band on 1.3 x the windows (the halo), so it should be bound by fp64 arithmetic and LDS reads at a few tens of microseconds.
(Measured, profiles/local_corr.txt: 286 us, ten times the estimate.  The cause is not measured; the leading candidate is
register-limited occupancy, one workgroup per CU at win = 4.)

  python tools/bench_loss.py [--leg composite|ssim|lcorr] [--reps 30] [--calls 50] [--step] [--out profiles/loss_terms.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

COPY_TBS = 6.29            # profiles/r04_hbm_kernels.txt
W_SAM, W_LAP = 0.1, 0.5


def composed(x0, xh, ms, k, w_sam=W_SAM, w_lap=W_LAP):
    """l1 + w_sam * SAM + w_lap * LAP from torch operators, fp32 (the arithmetic a user would write on the device)"""
    d = xh - x0
    u, v = x0 + ms, xh + ms
    dot, nu, nv = (u * v).sum(1), (u * u).sum(1), (v * v).sum(1)
    sam = torch.atan2(torch.sqrt((nu * nv - dot * dot).clamp_min(1e-20)), dot).mean()
    b, c, h, w = d.shape
    lap = F.conv2d(d.reshape(b * c, 1, h, w), k).abs().mean()
    return d.abs().mean() + w_sam * sam + w_lap * lap


def graph_us(fn, calls, reps):
    """median / 10th / 90th percentile of the device time per call, from replays of a graph of `calls` calls"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(calls):
            fn()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        torch.cuda.synchronize()
        ts.append(1e3 * a.elapsed_time(b) / calls)
    ts.sort()
    return statistics.median(ts), ts[len(ts) // 10], ts[-1 - len(ts) // 10]


def eager_us(fn, reps):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(20):
            fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(1e3 * a.elapsed_time(b) / 20)
    ts.sort()
    return statistics.median(ts), ts[len(ts) // 10], ts[-1 - len(ts) // 10]


def bench_shape(shape, calls, reps, lines):
    from tmdiff_amd import ops
    gen = torch.Generator(device="cuda").manual_seed(1)
    x0, xh = (torch.randn(*shape, device="cuda", generator=gen) for _ in range(2))
    ms = torch.rand(*shape, device="cuda", generator=gen)
    n = x0.numel()
    terms, total, g = ops.spectral_spatial_loss(x0, xh, ms, "l1", W_SAM, W_LAP)
    ws = torch.empty(max(1, ops.lib.tmdiff_loss_workspace_bytes(*shape, 1)), device="cuda", dtype=torch.uint8)
    leaf = xh.clone().requires_grad_(True)
    k = torch.tensor([[1.0, 1.0, 1.0], [1.0, -8.0, 1.0], [1.0, 1.0, 1.0]], device="cuda").view(1, 1, 3, 3)

    def pair():
        ops.spectral_spatial_loss(x0, xh, ms, "l1", W_SAM, W_LAP, grad=g, terms=terms, total=total, workspace=ws)

    def value_only():
        ops.spectral_spatial_loss(x0, xh, ms, "l1", W_SAM, W_LAP, grad=False, terms=terms, total=total, workspace=ws)

    def torch_ops():
        leaf.grad = None
        composed(x0, leaf, ms, k).backward()

    # the composition agrees with the kernel (fp32 against fp64 arithmetic)
    torch_ops()
    ref = float(composed(x0, xh, ms, k))
    dg = float((leaf.grad - g).norm() / g.norm())
    lines.append(f"[{', '.join(map(str, shape))}]  {n} elements, {16 * n / 1e6:.1f} MB moved by the pair; kernel total {float(terms[0]):.9f}, "
                 f"torch fp32 composition {ref:.9f}, gradients differ by {dg:.1e} relative L2")
    rows = [("kernel pair (value + gradient)", pair), ("kernel pair (value only)", value_only),
            ("torch operators, loss + backward", torch_ops)]
    for name, fn in rows:
        med, lo, hi = graph_us(fn, calls if fn is not torch_ops else max(1, calls // 10), reps)
        emed, _, _ = eager_us(fn, reps)
        rate = f"   {16 * n / (med * 1e-6) / 1e12:5.2f} TB/s" if fn is pair else ""
        lines.append(f"  {name:<34s} {med:8.1f} us in a graph ({lo:.1f} .. {hi:.1f})   {emed:8.1f} us eager{rate}")
    return graph_us(pair, calls, reps)[0]


def composed_dssim(a, b, box, win=7):
    """1 - SSIM from torch operators, fp32: five box filters as grouped conv2d over the band planes"""
    c = a.shape[1]
    n = win * win
    k = n / (n - 1.0)
    f = lambda t: F.conv2d(t, box, groups=c)
    ux, uy = f(a), f(b)
    vx, vy, vxy = k * (f(a * a) - ux * ux), k * (f(b * b) - uy * uy), k * (f(a * b) - ux * uy)
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    return 1.0 - (((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))).mean()


def bench_ssim_shape(shape, calls, reps, lines):
    from tmdiff_amd import ops
    gen = torch.Generator(device="cuda").manual_seed(1)
    a = torch.rand(*shape, device="cuda", generator=gen)
    b = a + 0.1 * torch.randn(*shape, device="cuda", generator=gen)
    n = a.numel()
    out, total, g = ops.ssim_loss(a, b)
    ws = torch.empty(max(1, ops.lib.tmdiff_ssim_loss_workspace_bytes(*shape, 7)), device="cuda", dtype=torch.uint8)
    leaf = b.clone().requires_grad_(True)
    box = torch.full((shape[1], 1, 7, 7), 1.0 / 49.0, device="cuda")

    def pair():
        ops.ssim_loss(a, b, grad=g, out=out, total=total, workspace=ws)

    def value_only():
        ops.ssim_loss(a, b, grad=False, out=out, total=total, workspace=ws)

    def torch_ops():
        leaf.grad = None
        composed_dssim(a, leaf, box).backward()

    torch_ops()
    ref = float(composed_dssim(a, b, box))
    dg = float((leaf.grad - g).norm() / g.norm())
    lines.append(f"[{', '.join(map(str, shape))}]  {n} elements, {12 * n / 1e6:.1f} MB moved by the pair; kernel dssim {float(out[0]):.9f}, "
                 f"torch fp32 composition {ref:.9f}, gradients differ by {dg:.1e} relative L2")
    res = {}
    for name, fn in (("kernel pair (value + gradient)", pair), ("kernel pair (value only)", value_only),
                     ("torch operators, loss + backward", torch_ops)):
        med, lo, hi = graph_us(fn, calls if fn is not torch_ops else max(1, calls // 10), reps)
        emed, _, _ = eager_us(fn, reps)
        rate = f"   {12 * n / (med * 1e-6) / 1e12:5.2f} TB/s" if fn is pair else ""
        lines.append(f"  {name:<34s} {med:8.1f} us in a graph ({lo:.1f} .. {hi:.1f})   {emed:8.1f} us eager{rate}")
        res[name] = med
    return res["kernel pair (value + gradient)"], res["torch operators, loss + backward"]


def composed_lcorr(x, pan, win=4):
    """mean max(0, 1 - rho) from torch operators, fp32: five box means, one-pass moments, a clamp under the square root"""
    f = lambda t: F.avg_pool2d(t, win, 1)
    mx, mp = f(x), f(pan)
    vxx, vpp, vxp = f(x * x) - mx * mx, f(pan * pan) - mp * mp, f(x * pan) - mx * mp
    rho = vxp / torch.sqrt((vxx * vpp).clamp_min(1e-20))
    return (1.0 - rho).clamp_min(0.0).mean()


def bench_lcorr_shape(shape, calls, reps, lines):
    from tmdiff_amd import ops
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = torch.rand(*shape, device="cuda", generator=gen)
    pan = 0.6 * x.mean(1, keepdim=True) + 0.4 * torch.rand(shape[0], 1, *shape[2:], device="cuda", generator=gen)
    n = x.numel()
    moved = 4 * (2 * n + pan.numel())
    out, total, g = ops.local_corr_loss(x, pan, 4)
    ws = torch.empty(max(1, ops.lib.tmdiff_local_corr_loss_workspace_bytes(*shape, 4)), device="cuda", dtype=torch.uint8)
    leaf = x.clone().requires_grad_(True)

    def pair():
        ops.local_corr_loss(x, pan, 4, grad=g, out=out, total=total, workspace=ws)

    def value_only():
        ops.local_corr_loss(x, pan, 4, grad=False, out=out, total=total, workspace=ws)

    def torch_ops():
        leaf.grad = None
        composed_lcorr(leaf, pan).backward()

    def torch_value():
        with torch.no_grad():
            composed_lcorr(x, pan)

    torch_ops()
    ref = float(composed_lcorr(x, pan))
    dg = float((leaf.grad - g).norm() / g.norm())
    lines.append(f"[{', '.join(map(str, shape))}]  {n} elements, {moved / 1e6:.1f} MB moved by the pair; kernel loss {float(out[0]):.9f}, "
                 f"torch fp32 composition {ref:.9f}, gradients differ by {dg:.1e} relative L2")
    res = {}
    for name, fn in (("kernel pair (value + gradient)", pair), ("kernel pair (value only)", value_only),
                     ("torch operators, loss + backward", torch_ops), ("torch operators, loss only", torch_value)):
        slow = fn in (torch_ops, torch_value)
        med, lo, hi = graph_us(fn, max(1, calls // 10) if slow else calls, reps)
        emed, _, _ = eager_us(fn, reps)
        rate = f"   {moved / (med * 1e-6) / 1e12:5.2f} TB/s" if fn is pair else ""
        lines.append(f"  {name:<34s} {med:8.1f} us in a graph ({lo:.1f} .. {hi:.1f})   {emed:8.1f} us eager{rate}")
        res[name] = med
    return res


def bench_step(reps, rounds, lines, on=None, label=None):
    """the captured finetune step, terms on against plain l1, alternating"""
    on = on or {"sam": W_SAM, "lap": W_LAP}
    label = label or f"l1 + {W_SAM} sam + {W_LAP} lap (the kernel pair)"
    names = ("l_pix", "l_base", "l_sam", "l_lap") + (("l_dssim",) if "dssim" in on else ())
    from tmdiff_amd.model import DDPM
    from tmdiff_amd.util import synthetic_tile_batch

    def trainer(loss_terms):
        opt = {"phase": "train", "gpu_ids": [0], "distributed": False, "path": {"resume": None},
               "model": {"unet": {"channel_multiplier": [32, 64, 128, 256]}, "diffusion": {"loss_type": "l1"}, "init_type": "orthogonal"},
               "train": {"optimizer": {"lr": 1e-4}, "max_iter": 150000, "hip_graph": True}}
        if loss_terms:
            opt["model"]["diffusion"]["loss_terms"] = loss_terms
        torch.manual_seed(3407)
        m = DDPM(opt)
        m.set_new_noise_schedule({"schedule": "cosine", "n_timestep": 1000}, "train")
        for it in range(DDPM.GRAPH_WARMUP + 2):
            m.feed_data(synthetic_tile_batch(it, 8, 8, 64))
            m.optimize_parameters("WV3")
        torch.cuda.synchronize()
        return m, next(iter(m._captured.values()))

    (plain, sp), (terms, st) = trainer(None), trainer(on)

    def timed(step):
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            step.graph.replay()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        return statistics.median(ts)

    a, b = [], []
    for _ in range(rounds):
        a.append(timed(sp))
        b.append(timed(st))
    lines.append(f"captured finetune step (ch 32-256, batch 8 of 8 x 64 x 64, graph replay, device events; {rounds} alternating rounds of "
                 f"{reps} replays, median of the rounds' medians, least .. greatest round):")
    lines.append(f"  plain l1 (torch nn.L1Loss, no new code runs)   {statistics.median(a):8.3f} ms   ({min(a):.3f} .. {max(a):.3f})")
    lines.append(f"  {label:<46s} {statistics.median(b):8.3f} ms   ({min(b):.3f} .. {max(b):.3f})")
    lines.append(f"  difference of the medians                      {1e3 * (statistics.median(b) - statistics.median(a)):8.1f} us")
    log = terms.get_current_log()
    lines.append("  log of the last step with the terms on: " + " ".join(f"{k} {float(log[k]):.5f}" for k in names))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--step", action="store_true", help="also time the captured finetune step with and without the terms")
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", choices=["composite", "ssim", "lcorr"], default="composite",
                    help="ssim: the SSIM term's kernel pair (csrc/ssim_loss.hip); lcorr: the local PAN-correlation loss (csrc/local_corr.hip)")
    args = ap.parse_args(argv)
    if args.reps < 7 or args.rounds < 7:
        raise SystemExit("bench_loss: medians of at least 7 runs")
    if not torch.cuda.is_available():
        raise SystemExit("bench_loss: needs the GPU (a time measured anywhere else says nothing)")
    if args.leg == "ssim":
        return main_ssim(args)
    if args.leg == "lcorr":
        return main_lcorr(args)
    lines = [f"# tools/bench_loss.py on {torch.cuda.get_device_name(0)}: l1 + {W_SAM} * SAM + {W_LAP} * LAP; per row the median over {args.reps} "
             f"replays of a graph of {args.calls} back-to-back evaluations (torch operators: {max(1, args.calls // 10)}), 10th .. 90th "
             f"percentile beside it, and the median of {args.reps} eager runs of 20 evaluations"]
    floor = []
    for shape in ((8, 8, 64, 64), (32, 8, 64, 64)):
        floor.append(bench_shape(shape, args.calls, args.reps, lines))
    verdict = "holds" if all(t <= 24.0 for t in floor) else "does NOT hold"
    lines.append(f"expectation: launch-latency-bound, near two dependent launches of 7 - 8 us each (profiles/r06_tiled_fused.txt) and "
                 f"far below the {COPY_TBS} TB/s copy rate: {verdict} (pair {floor[0]:.1f} us and {floor[1]:.1f} us; 'near' taken as "
                 f"within 1.5 x 16 us)")
    if args.step:
        bench_step(args.reps, args.rounds, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


def main_ssim(args):
    lines = [f"# tools/bench_loss.py --leg ssim on {torch.cuda.get_device_name(0)}: dssim = 1 - SSIM, 7 x 7 windows; per row the median over "
             f"{args.reps} replays of a graph of {args.calls} back-to-back evaluations (torch operators: {max(1, args.calls // 10)}), 10th .. "
             f"90th percentile beside it, and the median of {args.reps} eager runs of 20 evaluations"]
    pairs = [bench_ssim_shape(shape, args.calls, args.reps, lines) for shape in ((8, 8, 64, 64), (32, 8, 64, 64))]
    faster = all(p < t for p, t in pairs)
    lines.append("the pair against the torch composition (both from a graph): " +
                 ", ".join(f"{t / p:.2f} x" for p, t in pairs) + (" -- faster at both shapes" if faster else " -- NOT faster everywhere"))
    if args.step:
        bench_step(args.reps, args.rounds, lines, {"dssim": 0.1}, "l1 + 0.1 dssim (composite pair + SSIM pair)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


def main_lcorr(args):
    lines = [f"# tools/bench_loss.py --leg lcorr on {torch.cuda.get_device_name(0)}: mean max(0, 1 - rho), 4 x 4 windows; per row the median "
             f"over {args.reps} replays of a graph of {args.calls} back-to-back evaluations (torch operators: {max(1, args.calls // 10)}), 10th "
             f".. 90th percentile beside it, and the median of {args.reps} eager runs of 20 evaluations"]
    rows = [bench_lcorr_shape(shape, args.calls, args.reps, lines) for shape in ((8, 8, 64, 64), (1, 8, 1024, 1024))]
    for what, k, t in (("value + gradient", "kernel pair (value + gradient)", "torch operators, loss + backward"),
                       ("value only", "kernel pair (value only)", "torch operators, loss only")):
        ratios = [r[t] / r[k] for r in rows]
        lines.append(f"the pair against the torch composition, {what} (both from a graph): " + ", ".join(f"{v:.2f} x" for v in ratios) +
                     (" -- faster at both shapes" if all(v > 1.0 for v in ratios) else " -- NOT faster everywhere"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
