#!/usr/bin/env python3
"""Achieved bytes per second of the resampling kernels (csrc/resample.hip): algorithmic bytes (input read once + output written
once) over device time, each beside a device-to-device copy that moves the same number of bytes in the same run.

Cases: the fused two-level pyramid step and a single level on PAN [8, 1, 512, 512] and [1, 1, 2048, 2048], the x4 upsampling of MS
[8, 8, 128, 128], and the 23-tap polynomial upsampling (`upsample_poly23`) of MS [8, 8, 128, 128] and [1, 8, 512, 512]: x2, fused x4,
and the two x2 launches the fused kernel replaces, each beside a copy that writes the same number of output bytes (the kernel
reads 1/4 or 1/16 of what it writes, the copy reads as much as it writes; "of copy" is copy time over kernel time either way).
Every working set is far below the 256 MiB Infinity Cache, so these are rates of cache-resident data and of
launches a few microseconds long, not HBM streaming rates: the copy of equal size is the yardstick, and the 6.29 TB/s streaming
copy that bench_hbm_kernels.py quotes is printed for scale only.

Timing: device events around `--reps` back-to-back launches after a warm-up of the same length, repeated `--rounds` times with
the cases interleaved; the median round is reported with the least and the greatest.

`--leg mtf`: MTF-matched filtering and decimation (csrc/mtf.hip), x4 with the 41 x 41 kernels of "WV3", at MS [1, 8, 1024, 1024]
with PAN [1, 1, 4096, 4096] and at MS [32, 8, 256, 256] with PAN [32, 1, 1024, 1024]: the operator (`ops.mtf_degrade`) on the MS
and on the PAN, `data.wald_pair` (both degradations, the 23-tap upsampling and the residual), and the torch composition of the
operator -- replicate `F.pad`, the slice that starts at the offset, grouped `F.conv2d` with the ratio as its stride.  Every case
is captured into a graph of `--graph-calls` calls; a round is the time of one replay over that count.

`--leg adjoint`: the adjoint (`ops.mtf_degrade_adjoint`) at the same four shapes against torch autograd's backward of that
composition, the forward kernel's own time beside it, and `tiling.consistency_refine` (8 steps) at [1, 8, 1024, 1024]; timed the
same way.

`--leg glp`: the MTF-GLP baselines at MS [1, 8, 1024, 1024] "WV3" and [1, 4, 2048, 2048] "QB", PAN of the same extent: the filter
bank (`ops.fir_decimate_bank`) against `ops.fir_decimate` on the expanded PAN with the `expand().contiguous()` inside the timing;
`ops.glp_moments` + `ops.glp_inject` against the same arithmetic composed from torch operators (float64 statistics, float32
injection); `ops.mtf_glp` whole.  The elementwise kernels are printed with the bytes they move and their share of a
device-to-device copy of as many bytes, timed in the same rounds.  Captured and timed as `--leg mtf`.

`--leg cs`: the component-substitution baselines at the same two sizes: `ops.plane_moments` (the fp64 matrix-instruction Gram
kernel) beside a copy that moves the bytes of its C + 1 planes, beside `ops.glp_moments` and its own copy, and against the torch
composition (cast to fp64, centre, `X @ X.T`); `ops.cs_inject` beside a copy that moves its 2 C + 1 planes; `ops.cs_fuse` whole for
each method against the same chain composed from torch operators.  Captured and timed as `--leg mtf`.

`--leg bdsd`: BDSD at the same two sizes, with one set of weights per image and with one per 128 x 128 block: the two filters of
the reduced scale, `ops.bdsd_moments`, `ops.bdsd_coeffs`, `ops.bdsd_inject` beside a copy that moves its 2 C + 1 planes and beside
`ops.cs_inject` at the same shape, and `ops.bdsd` whole against the chain composed from torch operators (the same two filters,
then an fp64 `einsum` Gram, `torch.linalg.solve` and an `einsum` injection per block; launched eagerly, the solve cannot be
captured).  Captured and timed as `--leg mtf`.

`--leg cg`: Wald's consistency as a solve (csrc/cg.hip) at [1, 8, 1024, 1024] and [32, 8, 64, 64], x4 "WV3":
`ops.consistency_solve` (buffers and workspace given) at 8 iterations against `tiling.consistency_refine` at 8 steps in the same
run, the launch kinds of an iteration on their own (degradation, adjoint, the dots, the step, the direction) with the bytes the
elementwise ones move, and the residual ratio ||lr - A f|| / ||lr - A f0|| each method reaches from `upsample_poly23(lr)`.  The
step and the direction are timed with a numerator of exactly 0 (alpha = beta = 0): the same loads, multiply-adds and stores,
and the vectors stay as they are over the replays.  Captured and timed as
`--leg mtf`.

`--leg tv`: TV pansharpening (csrc/tv.hip) at [1, 8, 1024, 1024] "WV3" and [1, 4, 2048, 2048] "QB", x4: `ops.tv_pd_step` alone
against a device-to-device copy of the 7 C + 1 planes it moves, `ops.tv_norm`, `ops.tv_pansharpen` at 100 iterations and the same
iteration composed from torch operators (A as pad + conv2d, A^T as its autograd backward, the coupled part elementwise).
Captured and timed as `--leg mtf`; the 100-iteration calls are captured once per graph.

`--leg atrous`: a-trous wavelet pansharpening (csrc/atrous.hip) at the same two sizes: `ops.atrous_lowpass` of the PAN plane at
two levels against a device-to-device copy of the bytes it moves (one plane in, one out) and against the torch composition
(replicate `F.pad` plus dilated `F.conv2d` per level), `ops.awlp_inject` against a copy of its 2 C + 2 planes with
`ops.cs_inject` in the same run, and `ops.awlp` whole against `ops.mtf_glp(mode="glp")` whole.  Captured and timed as `--leg mtf`.
THE ESTIMATE, written before the first run: both kernels are bound by HBM -- `atrous_lowpass` within 1.5 times its copy (28 LDS
reads and about 50 fp64 operations per pixel should hide behind 8 bytes of traffic), `awlp_inject` at the 0.6 to 0.9 of its copy
that `cs_inject` and `bdsd_inject` reach.  What the run says about it is recorded in profiles/atrous.txt."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tmdiff_amd import ops  # noqa: E402

STREAM_COPY_GBS = 6290.0          # the copy rate tools/bench_hbm_kernels.py measures its kernels against


def time_us(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def captured(fn, calls):
    """A graph of `calls` calls of fn, after a warm-up on the capture stream."""
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        for _ in range(2):
            fn()
    stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        for _ in range(calls):
            fn()
    return graph


def mtf_leg(args):
    import torch.nn.functional as F
    from tmdiff_amd import metrics
    from tmdiff_amd.data import wald_pair
    sensor, ratio, k = "WV3", 4, metrics.MTF_TAPS
    ms_gains, pan_gain = metrics.mtf_gains(sensor, 8)

    def composition(x, gains):
        w = torch.from_numpy(np.stack([metrics.mtf_kernel(g, ratio) for g in gains])).float().cuda()[:, None]
        return lambda: F.conv2d(F.pad(x, (k // 2,) * 4, mode="replicate")[..., ratio // 2:, ratio // 2:], w, stride=ratio, groups=len(gains))

    cases = []          # (name, call, multiply-adds)
    for b, h in ((1, 1024), (32, 256)):
        ms, pan = torch.rand(b, 8, h, h, device="cuda"), torch.rand(b, 1, ratio * h, ratio * h, device="cuda")
        lr, low = ops.mtf_degrade(ms, sensor, ratio), ops.mtf_degrade(pan, sensor, ratio, pan=True)
        for name, x, gains, y, is_pan in (("MS ", ms, ms_gains, lr, False), ("PAN", pan, (pan_gain,), low, True)):
            macs = y.numel() * k * k
            ref = composition(x, gains)
            err = float((ref() - y).abs().max())
            print(f"{name} {list(x.shape)}: max |operator - torch composition| = {err:.3e}", flush=True)
            cases.append((f"mtf_degrade      {name} {list(x.shape)}", lambda x=x, y=y, p=is_pan: ops.mtf_degrade(x, sensor, ratio, pan=p, out=y), macs))
            cases.append((f"pad+slice+conv2d {name} {list(x.shape)}", ref, macs))
        cases.append((f"wald_pair        MS  {list(ms.shape)} + PAN", lambda ms=ms, pan=pan: wald_pair(ms, pan, sensor, ratio),
                      (lr.numel() + low.numel()) * k * k))
    graphs = [captured(fn, args.graph_calls) for _, fn, _ in cases]
    times = [[] for _ in cases]
    for _ in range(args.rounds):
        for graph, t in zip(graphs, times):
            time_us(graph.replay, 1)
            t.append(time_us(graph.replay, 1) / args.graph_calls)
    print(f"{'case':52s} {'us per call (min..max)':>30s} {'GMAC/s':>9s}")
    for (name, _, macs), t in zip(cases, times):
        m = statistics.median(t)
        print(f"{name:52s} {m:10.2f} ({min(t):8.2f}..{max(t):8.2f}) {macs / m / 1e3:9.1f}", flush=True)


def adjoint_leg(args):
    """`--leg adjoint`: ops.mtf_degrade_adjoint at the four shapes of `--leg mtf` against the backward of the torch composition
    (autograd through replicate F.pad, the slice and the grouped strided F.conv2d), with the forward kernel's own time at the
    same shape beside it (the two have the same multiply-adds), the same at a batch of 64 x 64 training patches, where every tile
    is a four-corner tile, and tiling.consistency_refine at [1, 8, 1024, 1024], 8 steps.
    Every case of the project's is a graph of `--graph-calls` calls; torch's backward runs eagerly (see below)."""
    import torch.nn.functional as F
    from tmdiff_amd import metrics
    from tmdiff_amd.tiling import consistency_refine
    sensor, ratio, k = "WV3", 4, metrics.MTF_TAPS
    ms_gains, pan_gain = metrics.mtf_gains(sensor, 8)
    cases = []          # (name, call, multiply-adds)
    shapes = [(name, shape, gains, is_pan) for b, h in ((1, 1024), (32, 256))
              for name, shape, gains, is_pan in (("MS ", (b, 8, h, h), ms_gains, False), ("PAN", (b, 1, ratio * h, ratio * h), (pan_gain,), True))]
    # a batch of training patches, as data.wald_pair and autograd see them: every 64 x 64 tile has all four corners
    shapes.append(("MS ", (32, 8, 64, 64), ms_gains, False))
    for name, shape, gains, is_pan in shapes:
        x = torch.rand(*shape, device="cuda")
        y = ops.mtf_degrade(x, sensor, ratio, pan=is_pan)
        g = torch.randn_like(y)
        dx = ops.mtf_degrade_adjoint(g, sensor, shape[2:], ratio, pan=is_pan)
        w = torch.from_numpy(np.stack([metrics.mtf_kernel(gn, ratio) for gn in gains])).float().cuda()[:, None]
        xr = x.clone().requires_grad_()
        yr = F.conv2d(F.pad(xr, (k // 2,) * 4, mode="replicate")[..., ratio // 2:, ratio // 2:], w, stride=ratio, groups=len(gains))

        def backward(xr=xr, yr=yr, g=g):
            xr.grad = None
            yr.backward(g, retain_graph=True)

        backward()
        err = float((xr.grad - dx).abs().max())
        print(f"{name} {list(shape)}: max |adjoint - torch backward| = {err:.3e}", flush=True)
        macs = y.numel() * k * k
        cases.append((f"mtf_degrade_adjoint      {name} {list(shape)}",
                      lambda g=g, dx=dx, s=shape, p=is_pan: ops.mtf_degrade_adjoint(g, sensor, s[2:], ratio, pan=p, out=dx), macs))
        cases.append((f"mtf_degrade (forward)    {name} {list(shape)}", lambda x=x, y=y, p=is_pan: ops.mtf_degrade(x, sensor, ratio, pan=p, out=y), macs))
        cases.append((f"backward of pad+slice+conv2d {name} {list(shape)}", backward, macs))
    fused = torch.rand(1, 8, 1024, 1024, device="cuda")
    lr = ops.mtf_degrade(torch.rand(1, 8, 1024, 1024, device="cuda"), sensor, ratio)
    out = torch.empty_like(fused)
    consistency_refine(fused, lr, sensor, ratio, iters=1, out=out)          # the tap tables and the operator norms, once
    cases.append(("consistency_refine 8 steps [1, 8, 1024, 1024]", lambda: consistency_refine(fused, lr, sensor, ratio, iters=8, out=out),
                  8 * 2 * lr.numel() * k * k))
    # The project's calls are captured; torch's backward is not: the autograd engine issues its kernels on the stream of the
    # forward pass, not on the capturing one, so it is timed eagerly, `--graph-calls` calls back to back between two events.
    runs = [(lambda fn=fn: [fn() for _ in range(args.graph_calls)]) if name.startswith("backward of") else captured(fn, args.graph_calls).replay
            for name, fn, _ in cases]
    times = [[] for _ in cases]
    for _ in range(args.rounds):
        for run, t in zip(runs, times):
            time_us(run, 1)
            t.append(time_us(run, 1) / args.graph_calls)
    print(f"{'case':56s} {'us per call (min..max)':>30s} {'GMAC/s':>9s}")
    med = {}
    for (name, _, macs), t in zip(cases, times):
        m = med[name] = statistics.median(t)
        print(f"{name:56s} {m:10.2f} ({min(t):8.2f}..{max(t):8.2f}) {macs / m / 1e3:9.1f}", flush=True)
    names = [n for n, _, _ in cases]
    for i in range(0, len(names) - 1, 3):
        a, f, t = (med[n] for n in names[i:i + 3])
        print(f"{names[i][24:]:28s} adjoint / forward kernel {a / f:5.2f}   torch backward / adjoint {t / a:6.1f}", flush=True)


def glp_leg(args):
    """`--leg glp`: see the module's docstring."""
    from tmdiff_amd import metrics
    ratio = 4
    cases = []          # (name, call, bytes moved or 0)
    for sensor, (b, c, h) in (("WV3", (1, 8, 1024)), ("QB", (1, 4, 2048))):
        shape = [b, c, h, h]
        ms, pan = 0.1 + 0.8 * torch.rand(b, c, h, h, device="cuda"), 0.1 + 0.8 * torch.rand(b, 1, h, h, device="cuda")
        gains = metrics.mtf_gains(sensor, c)[0]
        taps = ops._mtf_taps(gains, ratio, pan.device)
        buf, out = ops.mtf_glp_buffers(b, c, h, h, "cuda", ratio), torch.empty_like(ms)
        lp = ops.pan_lowpass_bands(pan, gains, c, ratio, out=buf["pan_lp"], low=buf["pan_low"])
        mo = ops.glp_moments(ms, pan, lp, out=buf["moments"], workspace=buf["ws"])
        low2 = torch.empty_like(buf["pan_low"])

        def expanded(pan=pan, taps=taps, low2=low2, c=c):
            return ops.fir_decimate(pan.expand(-1, c, -1, -1).contiguous(), taps, ratio, None, low2)

        def composed(ms=ms, pan=pan, lp=lp, out=out):
            m64, l64, p64 = ms.double(), lp.double(), pan.double()
            mean_m, mean_l, mean_p = m64.mean((2, 3), keepdim=True), l64.mean((2, 3), keepdim=True), p64.mean((2, 3), keepdim=True)
            var_m, var_l = ((m64 - mean_m) ** 2).mean((2, 3), keepdim=True), ((l64 - mean_l) ** 2).mean((2, 3), keepdim=True)
            a = (var_m / var_l).sqrt()
            pc, plc = a * (p64 - mean_p) + mean_m, a * (l64 - mean_p) + mean_m
            return out.copy_(m64 * pc / (plc + 2.0 ** -52))

        err = float((expanded() - ops.fir_decimate_bank(pan, taps, ratio, None, buf["pan_low"])).abs().max())
        ref = composed().clone()
        got = ops.glp_inject(ms, pan, lp, mo, "hpm", out=out)
        print(f"{sensor} {shape}: max |bank - expanded| = {err:.1e}; max |moments + inject - torch composition| = "
              f"{float((got - ref).abs().max()):.3e}", flush=True)
        plane = 4 * b * h * h
        src, dst = torch.empty((3 * c + 1) * plane // 8, device="cuda"), torch.empty((3 * c + 1) * plane // 8, device="cuda")
        src2, dst2 = torch.empty((2 * c + 1) * plane // 8, device="cuda"), torch.empty((2 * c + 1) * plane // 8, device="cuda")
        cases += [
            (f"fir_decimate_bank            {sensor} {shape}", lambda pan=pan, taps=taps, buf=buf: ops.fir_decimate_bank(pan, taps, ratio, None, buf["pan_low"]), 0),
            (f"expand + fir_decimate        {sensor} {shape}", expanded, 0),
            (f"glp_moments                  {sensor} {shape}", lambda ms=ms, pan=pan, lp=lp, buf=buf: ops.glp_moments(ms, pan, lp, out=buf["moments"], workspace=buf["ws"]), (2 * c + 1) * plane),
            (f"copy of (2 C + 1) planes     {sensor} {shape}", lambda s=src2, d=dst2: d.copy_(s), (2 * c + 1) * plane),
            (f"glp_inject hpm               {sensor} {shape}", lambda ms=ms, pan=pan, lp=lp, mo=mo, out=out: ops.glp_inject(ms, pan, lp, mo, "hpm", out=out), (3 * c + 1) * plane),
            (f"glp_inject cbd               {sensor} {shape}", lambda ms=ms, pan=pan, lp=lp, mo=mo, out=out: ops.glp_inject(ms, pan, lp, mo, "cbd", out=out), (3 * c + 1) * plane),
            (f"copy of (3 C + 1) planes     {sensor} {shape}", lambda s=src, d=dst: d.copy_(s), (3 * c + 1) * plane),
            (f"torch moments + hpm          {sensor} {shape}", composed, 0),
            (f"mtf_glp hpm (whole)          {sensor} {shape}", lambda ms=ms, pan=pan, s=sensor, out=out, buf=buf: ops.mtf_glp(ms, pan, s, ratio, "hpm", out=out, buffers=buf), 0),
        ]
    graphs = [captured(fn, args.graph_calls) for _, fn, _ in cases]
    times = [[] for _ in cases]
    for _ in range(args.rounds):
        for graph, t in zip(graphs, times):
            time_us(graph.replay, 1)
            t.append(time_us(graph.replay, 1) / args.graph_calls)
    print(f"{'case':56s} {'us per call (min..max)':>30s} {'MiB moved':>10s} {'GB/s':>8s}")
    med = {}
    for (name, _, nbytes), t in zip(cases, times):
        m = med[name] = statistics.median(t)
        rate = f"{nbytes / 2 ** 20:10.1f} {nbytes / m / 1e3:8.1f}" if nbytes else ""
        print(f"{name:56s} {m:10.2f} ({min(t):8.2f}..{max(t):8.2f}) {rate}", flush=True)
    names = [n for n, _, _ in cases]
    for i in range(0, len(names), 9):
        n = names[i:i + 9]
        print(f"{n[0][29:]:24s} expanded / bank {med[n[1]] / med[n[0]]:5.2f}   moments: of copy {med[n[3]] / med[n[2]]:5.2f}   "
              f"inject hpm: of copy {med[n[6]] / med[n[4]]:5.2f}   cbd: {med[n[6]] / med[n[5]]:5.2f}   "
              f"torch / (moments + inject) {med[n[7]] / (med[n[2]] + med[n[4]]):6.1f}", flush=True)


def cs_leg(args):
    """`--leg cs`: see the module's docstring."""
    from tmdiff_amd import metrics
    ratio = 4
    cases = []          # (name, call, bytes moved or 0)
    for sensor, (b, c, h) in (("WV3", (1, 8, 1024)), ("QB", (1, 4, 2048))):
        shape = [b, c, h, h]
        ms, pan = 0.1 + 0.8 * torch.rand(b, c, h, h, device="cuda"), 0.1 + 0.8 * torch.rand(b, 1, h, h, device="cuda")
        pan = (0.5 * pan + 0.5 * ms.mean(1, keepdim=True)).contiguous()
        lp = 0.1 + 0.8 * torch.rand(b, c, h, h, device="cuda")
        buf, out = ops.cs_fuse_buffers(b, c, h, h, "cuda", ratio), torch.empty_like(ms)
        gbuf = ops.mtf_glp_buffers(b, c, h, h, "cuda", ratio)
        full = ops.plane_moments(ms, pan, out=buf["full"], workspace=buf["ws"])
        coef = ops.cs_coeffs(full, None, "gs").clone()
        gain = metrics.mtf_gains(sensor, c)[1]
        ops.mtf_degrade(pan, gain, ratio, out=buf["pan_low"])                       # warm: the tap table is cached

        def moments64(x, p):
            """[B, C + 1, C + 2] from torch operators: cast to fp64, centre, X @ X.T."""
            x64 = torch.cat([x, p], 1).double().flatten(2)
            mean = x64.mean(2, keepdim=True)
            d = x64 - mean
            return torch.cat([d @ d.transpose(1, 2) / d.shape[2], mean], 2)

        def inject64(ms, pan, alpha, g, a, mean_i, mean_p, method, out):
            m64, p64 = ms.double(), pan.double()
            inten = (alpha[:, :, None, None] * m64).sum(1, keepdim=True)
            pi = a * (p64 - mean_p) + mean_i
            return out.copy_(m64 * pi / (inten + 2.0 ** -52) if method == "brovey" else m64 + g[:, :, None, None] * (pi - inten))

        def composed(method, ms=ms, pan=pan, out=out, c=c, gain=gain, buf=buf):
            mo = moments64(ms, pan)
            if method == "gsa":
                low = moments64(ms[..., ratio // 2::ratio, ratio // 2::ratio], ops.mtf_degrade(pan, gain, ratio, out=buf["pan_low"]))
                alpha = torch.linalg.solve(low[:, :c, :c], low[:, :c, c])     # not capturable: this row is timed eagerly
            else:
                alpha = torch.full((ms.shape[0], c), 1.0 / c, device=ms.device, dtype=torch.float64)
            sa = (mo[:, :c, :c] @ alpha[:, :, None])[:, :, 0]
            var_i = (alpha * sa).sum(1)
            mean_i = (alpha * mo[:, :c, c + 1]).sum(1)
            return inject64(ms, pan, alpha, sa / var_i[:, None], (var_i / mo[:, c, c]).sqrt()[:, None, None, None],
                            mean_i[:, None, None, None], mo[:, c, c + 1][:, None, None, None], method, out)

        err_m = float((moments64(ms, pan) - full).abs().max())
        errs = []
        for method in metrics.CS_METHODS:
            ref = composed(method).clone()
            errs.append(float((ops.cs_fuse(ms, pan, sensor, ratio, method, out=out, buffers=buf) - ref).abs().max()))
        print(f"{sensor} {shape}: max |plane_moments - torch composition| = {err_m:.3e}; max |cs_fuse - torch composition| = "
              + " / ".join(f"{e:.3e}" for e in errs) + " (gs / gsa / brovey)", flush=True)
        plane = 4 * b * h * h
        src1, dst1 = torch.empty((c + 1) * plane // 8, device="cuda"), torch.empty((c + 1) * plane // 8, device="cuda")
        src2, dst2 = torch.empty((2 * c + 1) * plane // 8, device="cuda"), torch.empty((2 * c + 1) * plane // 8, device="cuda")
        cases += [
            (f"plane_moments                {sensor} {shape}", lambda ms=ms, pan=pan, buf=buf: ops.plane_moments(ms, pan, out=buf["full"], workspace=buf["ws"]), (c + 1) * plane),
            (f"copy moving (C + 1) planes   {sensor} {shape}", lambda s=src1, d=dst1: d.copy_(s), (c + 1) * plane),
            (f"glp_moments                  {sensor} {shape}", lambda ms=ms, pan=pan, lp=lp, g=gbuf: ops.glp_moments(ms, pan, lp, out=g["moments"], workspace=g["ws"]), (2 * c + 1) * plane),
            (f"copy moving (2 C + 1) planes {sensor} {shape}", lambda s=src2, d=dst2: d.copy_(s), (2 * c + 1) * plane),
            (f"torch fp64 X @ X.T           {sensor} {shape}", lambda ms=ms, pan=pan: moments64(ms, pan), 0),
            (f"cs_inject gsa                {sensor} {shape}", lambda ms=ms, pan=pan, coef=coef, out=out: ops.cs_inject(ms, pan, coef, "gsa", out=out), (2 * c + 1) * plane),
            (f"cs_inject brovey             {sensor} {shape}", lambda ms=ms, pan=pan, coef=coef, out=out: ops.cs_inject(ms, pan, coef, "brovey", out=out), (2 * c + 1) * plane),
            (f"copy moving (2 C + 1) planes (again) {sensor} {shape}", lambda s=src2, d=dst2: d.copy_(s), (2 * c + 1) * plane),
            (f"cs_coeffs gsa                {sensor} {shape}", lambda full=full, buf=buf: ops.cs_coeffs(full, full, "gsa", out=buf["coef"]), 0),
        ]
        for method in metrics.CS_METHODS:
            cases += [
                (f"cs_fuse {method:6s} (whole)       {sensor} {shape}", lambda ms=ms, pan=pan, s=sensor, m=method, out=out, buf=buf: ops.cs_fuse(ms, pan, s, ratio, m, out=out, buffers=buf), 0),
                (f"torch composition {method:6s}{' (eager)' if method == 'gsa' else '':8s} {sensor} {shape}", lambda m=method, f=composed: f(m), -1 if method == "gsa" else 0),
            ]
    class Eager:                # a case that cannot be captured: the same number of calls, launched one by one
        def __init__(self, fn):
            self.fn = fn

        def replay(self):
            for _ in range(args.graph_calls):
                self.fn()

    graphs = [Eager(fn) if nbytes < 0 else captured(fn, args.graph_calls) for _, fn, nbytes in cases]
    times = [[] for _ in cases]
    for _ in range(args.rounds):
        for graph, t in zip(graphs, times):
            time_us(graph.replay, 1)
            t.append(time_us(graph.replay, 1) / args.graph_calls)
    print(f"{'case':56s} {'us per call (min..max)':>30s} {'MiB moved':>10s} {'GB/s':>8s}")
    med = {}
    for (name, _, nbytes), t in zip(cases, times):
        m = med[name] = statistics.median(t)
        rate = f"{nbytes / 2 ** 20:10.1f} {nbytes / m / 1e3:8.1f}" if nbytes > 0 else ""
        print(f"{name:56s} {m:10.2f} ({min(t):8.2f}..{max(t):8.2f}) {rate}", flush=True)
    names = [n for n, _, _ in cases]
    for i in range(0, len(names), 15):
        n = names[i:i + 15]
        print(f"{n[0][29:]:24s} plane_moments: of its bytes copied {med[n[1]] / med[n[0]]:5.2f} (glp_moments: {med[n[3]] / med[n[2]]:5.2f})   "
              f"torch X @ X.T / plane_moments {med[n[4]] / med[n[0]]:6.1f}   cs_inject: of copy, gsa {med[n[7]] / med[n[5]]:5.2f} "
              f"brovey {med[n[7]] / med[n[6]]:5.2f}   torch / cs_fuse: gs {med[n[10]] / med[n[9]]:5.1f} gsa {med[n[12]] / med[n[11]]:5.1f} "
              f"brovey {med[n[14]] / med[n[13]]:5.1f}", flush=True)


def bdsd_leg(args):
    """`--leg bdsd`: see the module's docstring."""
    from tmdiff_amd import metrics
    ratio = 4
    cases = []          # (name, call, bytes moved, 0, or -1 for a case that is timed eagerly)
    groups = []         # (title, names of: inject, its copy, cs_inject, whole, torch composition)
    for sensor, (b, c, h) in (("WV3", (1, 8, 1024)), ("QB", (1, 4, 2048))):
        shape = [b, c, h, h]
        ms, pan = 0.1 + 0.8 * torch.rand(b, c, h, h, device="cuda"), 0.1 + 0.8 * torch.rand(b, 1, h, h, device="cuda")
        pan = (0.5 * pan + 0.5 * ms.mean(1, keepdim=True)).contiguous()
        out = torch.empty_like(ms)
        ms_gains, pan_gain = metrics.mtf_gains(sensor, c)
        taps = ops._mtf_taps(ms_gains, ratio, ms.device)
        plane = 4 * b * h * h
        src, dst = torch.empty((2 * c + 1) * plane // 8, device="cuda"), torch.empty((2 * c + 1) * plane // 8, device="cuda")
        cs_buf = ops.cs_fuse_buffers(b, c, h, h, "cuda", ratio)
        coef = ops.cs_coeffs(ops.plane_moments(ms, pan, out=cs_buf["full"], workspace=cs_buf["ws"]), None, "gs").clone()
        for block in (None, 128):
            buf = ops.bdsd_buffers(b, c, h, h, "cuda", ratio, block)
            bs = None if block is None else block // ratio
            tag = f"{sensor} {shape} block {block}"

            def composed(ms=ms, pan=pan, out=out, buf=buf, taps=taps, gain=pan_gain, side=h if block is None else block, c=c):
                """The chain from torch operators: the two filters are the project's, then fp64 einsum Gram, torch.linalg.solve
                and an einsum injection per block."""
                low = buf["ms_low"].copy_(ms[..., ratio // 2::ratio, ratio // 2::ratio])
                lp = ops.fir_decimate(low, taps, 1, None, buf["lp_low"])
                pl = ops.mtf_degrade(pan, gain, ratio, out=buf["pan_low"])

                def tiles(x, s):
                    n, k, hh, ww = x.shape
                    return x.reshape(n, k, hh // s, s, ww // s, s).permute(0, 2, 4, 1, 3, 5)
                hm = tiles(torch.cat([lp, pl], 1).double(), side // ratio).flatten(4)
                d = tiles(low.double() - lp.double(), side // ratio).flatten(4)
                gamma = torch.linalg.solve(torch.einsum("...in,...jn->...ij", hm, hm), torch.einsum("...in,...jn->...ij", hm, d))
                m64 = ms.double()
                f = torch.einsum("byxkc,byxkij->byxcij", gamma, tiles(torch.cat([m64, pan.double()], 1), side))
                return out.copy_(m64 + f.permute(0, 3, 1, 4, 2, 5).reshape(m64.shape))

            ref = composed().clone()
            got = ops.bdsd(ms, pan, sensor, ratio, block, out=out, buffers=buf)
            print(f"{tag}: max |bdsd - torch composition| = {float((got - ref).abs().max()):.3e}", flush=True)
            mo, gamma, low = buf["moments"], buf["gamma"].clone(), buf["ms_low"]
            names = [f"bdsd_inject                  {tag}", f"copy moving (2 C + 1) planes {tag}", f"cs_inject gsa                {tag}",
                     f"bdsd (whole)                 {tag}", f"torch composition (eager)    {tag}"]
            groups.append((tag, names))
            cases += [
                (f"fir_decimate MS x1           {tag}", lambda low=low, taps=taps, buf=buf: ops.fir_decimate(low, taps, 1, None, buf["lp_low"]), 0),
                (f"mtf_degrade PAN              {tag}", lambda pan=pan, g=pan_gain, buf=buf: ops.mtf_degrade(pan, g, ratio, out=buf["pan_low"]), 0),
                (f"bdsd_moments                 {tag}", lambda buf=buf, bs=bs: ops.bdsd_moments(buf["lp_low"], buf["pan_low"], buf["ms_low"], bs, out=buf["moments"], workspace=buf["ws"]), (2 * c + 1) * plane // ratio ** 2),
                (f"bdsd_coeffs                  {tag}", lambda mo=mo, buf=buf: ops.bdsd_coeffs(mo, out=buf["gamma"]), 0),
                (names[0], lambda ms=ms, pan=pan, g=gamma, block=block, out=out: ops.bdsd_inject(ms, pan, g, block, out=out), (2 * c + 1) * plane),
                (names[1], lambda s=src, d=dst: d.copy_(s), (2 * c + 1) * plane),
                (names[2], lambda ms=ms, pan=pan, coef=coef, out=out: ops.cs_inject(ms, pan, coef, "gsa", out=out), (2 * c + 1) * plane),
                (names[3], lambda ms=ms, pan=pan, s=sensor, block=block, out=out, buf=buf: ops.bdsd(ms, pan, s, ratio, block, out=out, buffers=buf), 0),
                (names[4], composed, -1),
            ]

    class Eager:                # a case that cannot be captured: the same number of calls, launched one by one
        def __init__(self, fn):
            self.fn = fn

        def replay(self):
            for _ in range(args.graph_calls):
                self.fn()

    graphs = [Eager(fn) if nbytes < 0 else captured(fn, args.graph_calls) for _, fn, nbytes in cases]
    times = [[] for _ in cases]
    for _ in range(args.rounds):
        for graph, t in zip(graphs, times):
            time_us(graph.replay, 1)
            t.append(time_us(graph.replay, 1) / args.graph_calls)
    print(f"{'case':68s} {'us per call (min..max)':>30s} {'MiB moved':>10s} {'GB/s':>8s}")
    med = {}
    for (name, _, nbytes), t in zip(cases, times):
        m = med[name] = statistics.median(t)
        rate = f"{nbytes / 2 ** 20:10.1f} {nbytes / m / 1e3:8.1f}" if nbytes > 0 else ""
        print(f"{name:68s} {m:10.2f} ({min(t):8.2f}..{max(t):8.2f}) {rate}", flush=True)
    for tag, n in groups:
        print(f"{tag:36s} of copy: bdsd_inject {med[n[1]] / med[n[0]]:5.2f}, cs_inject gsa {med[n[1]] / med[n[2]]:5.2f}   "
              f"torch composition / bdsd {med[n[4]] / med[n[3]]:6.1f}", flush=True)


def cg_leg(args):
    """`--leg cg`: see the module's docstring."""
    from tmdiff_amd import metrics
    from tmdiff_amd._lib import check, lib
    from tmdiff_amd.tiling import consistency_refine
    sensor, ratio, iters = "WV3", 4, 8
    taps = ops._mtf_taps(metrics.band_gains(sensor, 8), ratio, torch.device("cuda", torch.cuda.current_device()))
    cases, groups = [], []          # (name, call, bytes moved or 0); (shape, names)
    for shape in ((1, 8, 1024, 1024), (32, 8, 64, 64)):
        b, c, h, w = shape
        truth = torch.rand(*shape, device="cuda")
        lr = ops.mtf_degrade(truth, sensor, ratio)
        f0 = ops.upsample_poly23(lr, ratio)
        out, out2 = torch.empty_like(f0), torch.empty_like(f0)
        ws = ops.consistency_solve_workspace(b, c, h, w, ratio, iters, "cuda")
        res = lambda f, lr=lr: float((lr - ops.mtf_degrade(f, sensor, ratio)).double().pow(2).sum().sqrt())
        solve = lambda f0=f0, lr=lr, out=out, ws=ws: ops.consistency_solve(f0, lr, taps, ratio, iters, out=out, workspace=ws)
        refine = lambda f0=f0, lr=lr, out2=out2: consistency_refine(f0, lr, sensor, ratio, iters=iters, out=out2)
        solve(), refine()
        print(f"{list(shape)}: residual ratio after {iters} iterations: consistency_solve {res(out) / res(f0):.4f}, "
              f"consistency_refine {res(out2) / res(f0):.4f}", flush=True)
        planes, nf, nl = b * c, h * w, lr.shape[2] * lr.shape[3]
        r, q, d, sv, p, part = ws["r"], ws["q"], ws["d"], ws["s"], ws["p"], ws["partials"]
        cf, cl = ops.plane_dots_partials(nf), ops.plane_dots_partials(nl)
        g0, g1 = part[:planes * cf], part[planes * cf:2 * planes * cf]
        qq = part[3 * planes * cf:3 * planes * cf + planes * cl]
        rr = part[3 * planes * cf + planes * cl:3 * planes * cf + 2 * planes * cl]
        zero = torch.zeros(planes * cf, device="cuda", dtype=torch.float64)          # a numerator of 0: alpha = beta = 0

        def step(p=p, q=q, d=d, r=r, zero=zero, qq=qq, rr=rr, planes=planes, nf=nf, nl=nl):
            check(lib.tmdiff_cg_step(p.data_ptr(), q.data_ptr(), d.data_ptr(), r.data_ptr(), zero.data_ptr(), qq.data_ptr(), None, 0.0,
                                     rr.data_ptr(), planes, nf, nl, 0, ops.stream_ptr()))

        def direction(sv=sv, p=p, zero=zero, g0=g0, planes=planes, nf=nf):
            check(lib.tmdiff_cg_direction(sv.data_ptr(), p.data_ptr(), zero.data_ptr(), g0.data_ptr(), None, planes, nf, ops.stream_ptr()))

        tag = f"{list(shape)}"
        names = [f"{n:28s} {tag}" for n in ("consistency_solve 8 iterations", "consistency_refine 8 steps", "fir_decimate (A p)",
                                            "fir_decimate_adjoint (A^T r)", "dot <q, q> (low)", "dot <s, s> (full)", "cg_step", "cg_direction")]
        groups.append((tag, names))
        cases += [(names[0], solve, 0), (names[1], refine, 0),
                  (names[2], lambda p=p, q=q: ops.fir_decimate(p, taps, ratio, None, q), 0),
                  (names[3], lambda r=r, sv=sv, h=h, w=w: ops.fir_decimate_adjoint(r, taps, (h, w), ratio, None, sv), 0),
                  (names[4], lambda q=q, qq=qq, planes=planes: ops._launch_dots("plane_dots", [(q, q, qq)], planes), 4 * planes * nl),
                  (names[5], lambda sv=sv, g1=g1, planes=planes: ops._launch_dots("plane_dots", [(sv, sv, g1)], planes), 4 * planes * nf),
                  (names[6], step, 4 * planes * (3 * nf + 3 * nl)), (names[7], direction, 4 * planes * 3 * nf)]
    graphs = [captured(fn, args.graph_calls) for _, fn, _ in cases]
    times = [[] for _ in cases]
    for _ in range(args.rounds):
        for graph, t in zip(graphs, times):
            time_us(graph.replay, 1)
            t.append(time_us(graph.replay, 1) / args.graph_calls)
    print(f"{'case':52s} {'us per call (min..max)':>30s} {'MiB moved':>10s} {'GB/s':>8s}")
    med = {}
    for (name, _, nbytes), t in zip(cases, times):
        m = med[name] = statistics.median(t)
        rate = f"{nbytes / 2 ** 20:10.1f} {nbytes / m / 1e3:8.1f}" if nbytes else ""
        print(f"{name:52s} {m:10.2f} ({min(t):8.2f}..{max(t):8.2f}) {rate}", flush=True)
    for tag, n in groups:
        new = med[n[4]] + med[n[5]] + med[n[6]] + med[n[7]]
        print(f"{tag:20s} solve / refine {med[n[0]] / med[n[1]]:5.2f}   per iteration: A + A^T {med[n[2]] + med[n[3]]:8.2f} us, "
              f"dots + step + direction {new:8.2f} us ({new / (med[n[2]] + med[n[3]]):5.2f} of the pair)", flush=True)


def tv_leg(args):
    """`--leg tv`: see the module's docstring."""
    import torch.nn.functional as F
    from tmdiff_amd import metrics
    iters, ratio, lam, gamma, k = 100, 4, 1e-3, 1.0, metrics.MTF_TAPS
    cases, groups = [], []          # (name, call, bytes moved or 0, calls per graph); (tag, names)
    for sensor, shape in (("WV3", (1, 8, 1024, 1024)), ("QB", (1, 4, 2048, 2048))):
        b, c, h, w = shape
        gains = metrics.band_gains(sensor, c)
        truth = torch.rand(*shape, device="cuda")
        lr, pan = ops.mtf_degrade(truth, sensor, ratio), truth.mean(1, keepdim=True).contiguous()
        wt = metrics.tv_weights(None, b, c)
        tau, sigma = metrics.tv_step_sizes(gains, ratio, wt, gamma)
        buf, out = ops.tv_buffers(b, c, h, w, "cuda", ratio), torch.empty(*shape, device="cuda")
        solve = lambda lr=lr, pan=pan, out=out, buf=buf, sensor=sensor: ops.tv_pansharpen(lr, pan, sensor, ratio, iters, lam, gamma, out=out, buffers=buf)
        solve()
        x, u, p0, p1 = out, buf["u"], buf["p"][0], buf["p"][1]
        xn = torch.empty_like(x)
        step = lambda u=u, x=x, p0=p0, p1=p1, pan=pan, xn=xn, tau=tau, sigma=sigma: ops.tv_pd_step(
            u, x, p0[0], p0[1], pan, None, tau, sigma, lam, gamma, out_x=xn, out_p=(p1[0], p1[1]))
        moved = 4 * (7 * c + 1) * b * h * w
        src = torch.empty(moved // 8, device="cuda").normal_()
        dst = torch.empty_like(src)
        val, ws = torch.empty(b, device="cuda", dtype=torch.float64), ops.tv_norm_workspace(b, c, h, w, "cuda")
        # the same iteration from torch operators
        wk = torch.from_numpy(np.stack([metrics.mtf_kernel(g, ratio) for g in gains])).float().cuda()[:, None]
        wv = torch.from_numpy(wt[:, :c]).float().cuda()[:, :, None, None]
        a_of = lambda t, wk=wk, c=c: F.conv2d(F.pad(t, (k // 2,) * 4, mode="replicate")[..., ratio // 2:, ratio // 2:], wk, stride=ratio, groups=c)

        def composed(lr=lr, pan=pan, a_of=a_of, wv=wv, tau=tau, sigma=sigma):
            xt = ops.upsample_poly23(lr, ratio)
            ph, pv = torch.zeros_like(xt), torch.zeros_like(xt)
            for _ in range(iters):
                with torch.enable_grad():
                    xr = xt.detach().requires_grad_(True)
                    g, = torch.autograd.grad(0.5 * (a_of(xr) - lr).pow(2).sum(), xr)
                s = (wv * xt).sum(1, keepdim=True) - pan
                dt = -ph
                dt[..., :, -1] = 0
                dt[..., :, 1:] += ph[..., :, :-1]
                dt[..., :-1, :] -= pv[..., :-1, :]
                dt[..., 1:, :] += pv[..., :-1, :]
                new = xt - tau * (g + gamma * wv * s + dt)
                bar = 2 * new - xt
                qh, qv = ph.clone(), pv.clone()
                qh[..., :, :-1] += sigma * (bar[..., :, 1:] - bar[..., :, :-1])
                qv[..., :-1, :] += sigma * (bar[..., 1:, :] - bar[..., :-1, :])
                scale = ((qh * qh + qv * qv).sum(1, keepdim=True).sqrt() / lam).clamp(min=1.0)
                xt, ph, pv = new, qh / scale, qv / scale
            return xt
        gap = float((composed() - out).abs().max())
        print(f"{list(shape)} {sensor}: max |tv_pansharpen - torch composition| after {iters} iterations = {gap:.3e}; "
              f"tv_norm start {float(ops.tv_norm(ops.upsample_poly23(lr, ratio))[0]):.1f} -> {float(ops.tv_norm(out)[0]):.1f}", flush=True)
        tag = f"{list(shape)}"
        names = [f"{n:30s} {tag}" for n in ("tv_pd_step", "copy of 7 C + 1 planes", "tv_norm", "tv_pansharpen 100 iterations",
                                            "torch composition 100 iterations")]
        groups.append((tag, names))
        cases += [(names[0], step, moved, args.graph_calls), (names[1], lambda src=src, dst=dst: dst.copy_(src), moved, args.graph_calls),
                  (names[2], lambda x=x, val=val, ws=ws: ops.tv_norm(x, out=val, workspace=ws), 4 * c * b * h * w, args.graph_calls),
                  (names[3], solve, 0, 1), (names[4], composed, 0, 1)]
    runs = []                       # a graph's replay; the eager call where torch cannot capture the composition
    for name, fn, _, calls in cases:
        try:
            runs.append((captured(fn, calls).replay, calls))
        except RuntimeError as e:
            torch.cuda.synchronize()
            print(f"{name.strip()}: not captured ({str(e).splitlines()[0][:80]}); timed eagerly", flush=True)
            runs.append((fn, 1))
    times = [[] for _ in cases]
    for _ in range(args.rounds):
        for (run, calls), t in zip(runs, times):
            time_us(run, 1)
            t.append(time_us(run, 1) / calls)
    print(f"{'case':52s} {'us per call (min..max)':>34s} {'MiB moved':>10s} {'GB/s':>8s}")
    med = {}
    for (name, _, nbytes, _), t in zip(cases, times):
        m = med[name] = statistics.median(t)
        rate = f"{nbytes / 2 ** 20:10.1f} {nbytes / m / 1e3:8.1f}" if nbytes else ""
        print(f"{name:52s} {m:12.2f} ({min(t):10.2f}..{max(t):10.2f}) {rate}", flush=True)
    for tag, n in groups:
        print(f"{tag:20s} tv_pd_step / copy {med[n[0]] / med[n[1]]:5.2f}   tv_pd_step share of an iteration {100 * med[n[0]] / med[n[3]]:.2f}   "
              f"torch composition / tv_pansharpen {med[n[4]] / med[n[3]]:5.1f}", flush=True)


def atrous_leg(args):
    """`--leg atrous`: see the module's docstring."""
    import torch.nn.functional as F
    from tmdiff_amd import metrics
    ratio, levels = 4, 2
    cases, groups = [], []          # (name, call, bytes moved or 0); (tag, names)
    taps = torch.tensor(metrics.ATROUS_TAPS, device="cuda")
    kernel = torch.outer(taps, taps)[None, None]

    def composed(pan):
        c = pan
        for level in range(levels):
            d = 1 << level
            c = F.conv2d(F.pad(c, (2 * d,) * 4, mode="replicate"), kernel, dilation=d)
        return c

    for sensor, shape in (("WV3", (1, 8, 1024, 1024)), ("QB", (1, 4, 2048, 2048))):
        b, c, h, w = shape
        ms, pan = torch.rand(*shape, device="cuda"), torch.rand(b, 1, h, w, device="cuda")
        buf, out = ops.awlp_buffers(b, c, h, w, "cuda", ratio), torch.empty(*shape, device="cuda")
        gbuf, gout = ops.mtf_glp_buffers(b, c, h, w, "cuda", ratio), torch.empty(*shape, device="cuda")
        whole = lambda ms=ms, pan=pan, out=out, buf=buf: ops.awlp(ms, pan, ratio, "awlp", out=out, buffers=buf)
        glp = lambda ms=ms, pan=pan, gout=gout, gbuf=gbuf, sensor=sensor: ops.mtf_glp(ms, pan, sensor, ratio, "glp", out=gout, buffers=gbuf)
        whole(), glp()
        low, mo = buf["pan_lp"], buf["moments"]
        gap = float((composed(pan) - low).abs().max())          # replicate padding of c_{l-1} is the clamped read of c_{l-1}
        print(f"{list(shape)}: max |atrous_lowpass - torch composition| = {gap:.3e}", flush=True)
        coef = ops.cs_coeffs(ops.plane_moments(ms, pan), None, "gs")
        cout = torch.empty_like(ms)
        copies = {}
        for planes in (2, 2 * c + 2, 2 * c + 1):
            src = torch.empty(planes * b * h * w // 2, device="cuda").normal_()
            copies[planes] = (src, torch.empty_like(src))
        tag = f"{list(shape)}"
        names = [f"{n:30s} {tag}" for n in ("atrous_lowpass levels 2", "copy of 2 planes", "pad + dilated conv2d x 2", "awlp_inject",
                                            "copy of 2 C + 2 planes", "cs_inject", "copy of 2 C + 1 planes", "awlp whole",
                                            "mtf_glp glp whole")]
        groups.append((tag, names))
        plane = 4 * b * h * w
        cp = lambda k: (lambda s=copies[k][0], d=copies[k][1]: d.copy_(s))
        cases += [(names[0], lambda pan=pan, low=low: ops.atrous_lowpass(pan, levels, out=low), 2 * plane), (names[1], cp(2), 2 * plane),
                  (names[2], lambda pan=pan: composed(pan), 2 * plane),
                  (names[3], lambda ms=ms, pan=pan, low=low, mo=mo, out=out: ops.awlp_inject(ms, pan, low, mo, "awlp", out=out), (2 * c + 2) * plane),
                  (names[4], cp(2 * c + 2), (2 * c + 2) * plane),
                  (names[5], lambda ms=ms, pan=pan, coef=coef, cout=cout: ops.cs_inject(ms, pan, coef, "gs", out=cout), (2 * c + 1) * plane),
                  (names[6], cp(2 * c + 1), (2 * c + 1) * plane), (names[7], whole, 0), (names[8], glp, 0)]
    graphs = [captured(fn, args.graph_calls) for _, fn, _ in cases]
    times = [[] for _ in cases]
    for _ in range(args.rounds):
        for graph, t in zip(graphs, times):
            time_us(graph.replay, 1)
            t.append(time_us(graph.replay, 1) / args.graph_calls)
    print(f"{'case':52s} {'us per call (min..max)':>34s} {'MiB moved':>10s} {'GB/s':>8s}")
    med = {}
    for (name, _, nbytes), t in zip(cases, times):
        m = med[name] = statistics.median(t)
        rate = f"{nbytes / 2 ** 20:10.1f} {nbytes / m / 1e3:8.1f}" if nbytes else ""
        print(f"{name:52s} {m:12.2f} ({min(t):10.2f}..{max(t):10.2f}) {rate}", flush=True)
    for tag, n in groups:
        print(f"{tag:20s} atrous_lowpass / copy {med[n[0]] / med[n[1]]:5.2f}   torch composition / atrous_lowpass {med[n[2]] / med[n[0]]:5.1f}   "
              f"awlp_inject / copy {med[n[3]] / med[n[4]]:5.2f}   cs_inject / copy {med[n[5]] / med[n[6]]:5.2f}   "
              f"awlp / mtf_glp {med[n[7]] / med[n[8]]:5.2f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("resample", "mtf", "adjoint", "glp", "cs", "bdsd", "cg", "tv", "atrous"), default="resample")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--graph-calls", type=int, default=10, help="--leg mtf / adjoint: calls captured into each graph")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_resample.py needs the GPU: a rate cannot be measured without one")
    p = torch.cuda.get_device_properties(0)
    print(f"device: {p.name} ({getattr(p, 'gcnArchName', '?')}), {p.multi_processor_count} CUs, {p.total_memory / 2 ** 30:.0f} GiB; "
          f"torch {torch.__version__}, HIP {torch.version.hip}; reps {args.reps}, rounds {args.rounds}", flush=True)
    if args.leg == "mtf":
        return mtf_leg(args)
    if args.leg == "adjoint":
        return adjoint_leg(args)
    if args.leg == "glp":
        return glp_leg(args)
    if args.leg == "cs":
        return cs_leg(args)
    if args.leg == "bdsd":
        return bdsd_leg(args)
    if args.leg == "cg":
        return cg_leg(args)
    if args.leg == "tv":
        return tv_leg(args)
    if args.leg == "atrous":
        return atrous_leg(args)

    cases = []          # (name, kernel call, bytes, copy call, bytes the copy moves)

    def add(name, x, fn):
        y = fn(x, None)
        nbytes = (x.numel() + y.numel()) * 4
        src = torch.empty(nbytes // 8, device="cuda").normal_()
        dst = torch.empty_like(src)
        cases.append((name, lambda: fn(x, y), nbytes, lambda: dst.copy_(src), nbytes))

    def add_poly23(name, x, y, fn):          # the copy writes y's bytes
        src = torch.empty_like(y).normal_()
        dst = torch.empty_like(y)
        cases.append((name, fn, (x.numel() + y.numel()) * 4, lambda: dst.copy_(src), 2 * y.numel() * 4))

    for shape in ((8, 1, 512, 512), (1, 1, 2048, 2048)):
        pan = torch.rand(*shape, device="cuda")
        add(f"pyr_down 2 levels (fused) {list(shape)}", pan, lambda x, o: ops.pyr_down(x, 2, out=o))
        add(f"pyr_down 1 level          {list(shape)}", pan, lambda x, o: ops.pyr_down(x, 1, out=o))
        # what the fused kernel replaces: two launches with level 1 written and read back
        half = ops.pyr_down(pan, 1)
        quarter = ops.pyr_down(half, 1)
        nbytes = (pan.numel() + quarter.numel()) * 4
        src = torch.empty(nbytes // 8, device="cuda").normal_()
        dst = torch.empty_like(src)
        cases.append((f"pyr_down 1 + 1 levels     {list(shape)}",
                      lambda pan=pan, half=half, quarter=quarter: ops.pyr_down(ops.pyr_down(pan, 1, out=half), 1, out=quarter),
                      nbytes, lambda dst=dst, src=src: dst.copy_(src), nbytes))
    ms = torch.rand(8, 8, 128, 128, device="cuda")
    add("upsample_bilinear x4      [8, 8, 128, 128]", ms, lambda x, o: ops.upsample_bilinear(x, 4, out=o))

    for shape in ((8, 8, 128, 128), (1, 8, 512, 512)):
        ms = torch.randn(*shape, device="cuda")
        half, full = ops.upsample_poly23(ms, 2), ops.upsample_poly23(ms, 4)
        add_poly23(f"upsample_poly23 x2        {list(shape)}", ms, half, lambda ms=ms, half=half: ops.upsample_poly23(ms, 2, out=half))
        add_poly23(f"upsample_poly23 x4 (fused) {list(shape)}", ms, full, lambda ms=ms, full=full: ops.upsample_poly23(ms, 4, out=full))
        # what the fused kernel replaces: two launches with the x2 image written and read back
        add_poly23(f"upsample_poly23 x2 + x2   {list(shape)}", ms, full, lambda ms=ms, half=half, full=full: ops.upsample_poly23(
            ops.upsample_poly23(ms, 2, out=half), 2, out=full, phase=0))

    times = [([], []) for _ in cases]
    for _ in range(args.rounds):
        for (name, fn, nbytes, copy, cbytes), (tk, tc) in zip(cases, times):
            time_us(fn, args.reps)                         # warm-up of this case
            tk.append(time_us(fn, args.reps))
            time_us(copy, args.reps)
            tc.append(time_us(copy, args.reps))
    print(f"{'case':50s} {'MiB':>6s} {'us (min..max)':>22s} {'GB/s':>8s} | {'copy us':>8s} {'copy GB/s':>9s} | "
          f"{'of copy':>7s} {'of 6.29 TB/s':>12s}")
    for (name, _, nbytes, _, cbytes), (tk, tc) in zip(cases, times):
        k, c = statistics.median(tk), statistics.median(tc)
        gbs, cgbs = nbytes / k / 1e3, cbytes / c / 1e3
        print(f"{name:50s} {nbytes / 2 ** 20:6.1f} {k:8.2f} ({min(tk):5.2f}..{max(tk):5.2f}) {gbs:8.1f} | {c:8.2f} {cgbs:9.1f} | "
              f"{100 * c / k:6.1f}% {100 * gbs / STREAM_COPY_GBS:11.1f}%", flush=True)


if __name__ == "__main__":
    main()
