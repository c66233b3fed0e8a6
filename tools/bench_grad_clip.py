#!/usr/bin/env python3
"""What global-norm gradient clipping adds to the AdamW step (tmdiff_amd.optim.FusedAdamW(max_grad_norm=...)).

On the parameter list of WavBEST at the benchmark's widths (ch 32-256; every tensor gets a random gradient) it times, with HIP
events around each repetition and the median over many of them:
  optG.step() without clipping                         (tmdiff_multi_adamw)
  optG.step() with clipping                            (stage 1 + finish + counter add + tmdiff_multi_adamw_scaled)
  stage 1 alone, the finish alone, stage 1 + finish    (tmdiff_multi_sqnorm_partial / _finish)
  the scaled and the plain AdamW launch alone          (tmdiff_multi_adamw_scaled, tmdiff_multi_adamw)
and derives the stage-1 read rate against the copy rate the project records (6.29 TB/s, profiles/r04_hbm_kernels.txt) and the
added time as a share of the finetune step (profiles/r04_bench_train_line.json).

  python tools/bench_grad_clip.py [--reps 300] [--warmup 30] [--out profiles/grad_clip.txt]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

COPY_TBS = 6.29            # profiles/r04_hbm_kernels.txt


def median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) for a, b in ev)
    return statistics.median(ts), ts[len(ts) // 10], ts[-1 - len(ts) // 10]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--channels", type=int, nargs=4, default=[32, 64, 128, 256])
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_grad_clip: needs the GPU (a time measured anywhere else says nothing)")
    from tmdiff_amd import ops
    from tmdiff_amd._lib import check, lib
    from tmdiff_amd.Hyper_unet_general import WavBEST
    from tmdiff_amd.optim import FusedAdamW

    def optimizer(**kw):
        torch.manual_seed(0)
        net = WavBEST(channels=args.channels).cuda()
        params = [p for n, p in net.named_parameters() if "clip_text" not in n]
        for p in params:
            p.grad = torch.randn_like(p) * 1e-2
        return FusedAdamW(params, lr=torch.tensor(1e-4, device="cuda"), weight_decay=1e-4, **kw), params

    plain, _ = optimizer()
    clipped, params = optimizer(max_grad_norm=1.0)
    n_elem = sum(p.numel() for p in params)
    plain.step()
    clipped.step()
    tb, cb = clipped._tables[0], clipped._clip
    group = clipped.param_groups[0]
    step = clipped.state[params[0]]["step"]
    norm, coef, ok = cb["scalars"][0], cb["scalars"][1], cb["scalars"][2]
    tab = (tb["entries"].data_ptr(), tb["chunk_tensor"].data_ptr(), tb["chunk_index"].data_ptr(), tb["n_chunks"])

    def stage1():
        check(lib.tmdiff_multi_sqnorm_partial(*tab, cb["partials"].data_ptr(), ops.stream_ptr()), "multi_sqnorm_partial")

    def finish():
        check(lib.tmdiff_multi_sqnorm_finish(cb["partials"].data_ptr(), cb["total"], clipped.max_grad_norm, norm.data_ptr(),
                                             coef.data_ptr(), ok.data_ptr(), ops.stream_ptr()), "multi_sqnorm_finish")

    def both():
        stage1()
        finish()

    def scaled():
        clipped._launch(0, group, params, step, tb, coef, ok)

    def unscaled():
        clipped._launch(0, group, params, step, tb)

    rows = [("step(), no clipping", plain.step), ("step(), max_grad_norm", clipped.step), ("stage 1 (partial sums)", stage1),
            ("finish", finish), ("stage 1 + finish", both), ("scaled AdamW launch", scaled), ("plain AdamW launch", unscaled)]
    res = {name: median_ms(fn, args.reps, args.warmup) for name, fn in rows}
    with open(os.path.join(ROOT, "profiles", "r04_bench_train_line.json")) as f:
        step_ms = json.load(f)["ms_per_step"]
    added = res["step(), max_grad_norm"][0] - res["step(), no clipping"][0]
    rate = 4.0 * n_elem / (res["stage 1 (partial sums)"][0] * 1e-3) / 1e12
    lines = [f"# tools/bench_grad_clip.py on {torch.cuda.get_device_name(0)}: {len(params)} tensors, {n_elem} elements "
             f"({4 * n_elem / 1e6:.1f} MB of gradients), {tb['n_chunks']} chunks; HIP events per repetition, "
             f"median of {args.reps} after {args.warmup} warm-up calls (10th / 90th percentile beside it)"]
    for name, _ in rows:
        med, lo, hi = res[name]
        lines.append(f"{name:<26s} {1e3 * med:9.1f} us   ({1e3 * lo:.1f} .. {1e3 * hi:.1f})")
    lines.append(f"stage-1 read rate          {rate:9.2f} TB/s ({100 * rate / COPY_TBS:.0f}% of the {COPY_TBS} TB/s copy rate, "
                 f"profiles/r04_hbm_kernels.txt)")
    dev = res["stage 1 + finish"][0] + res["scaled AdamW launch"][0] - res["plain AdamW launch"][0]
    lines.append(f"added on the device        {1e3 * dev:9.1f} us = {100 * dev / step_ms:.2f}% of the {step_ms} ms finetune step "
                 f"(profiles/r04_bench_train_line.json): stage 1 + finish + (scaled - plain launch); what a graph replay pays")
    lines.append(f"added to an eager step()   {1e3 * added:9.1f} us = {100 * added / step_ms:.2f}% of that step (an eager step() is bound "
                 f"by its host loop over the tensors, not by its kernels)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    return res


if __name__ == "__main__":
    main()
