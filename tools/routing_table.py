#!/usr/bin/env python3
"""Layer -> kernel family for every 3x3x3 convolution of the BASELINE configurations (host logic only: runs without a GPU).

    python tools/routing_table.py > profiles/r04_routing_table.txt

One block per case of tmdiff_amd.routing.BASELINE_CASES (BASELINE.json configs[0..4]; B in {1, 8, 32}, 4 and 8 bands, 64^2 and
256^2 planes), one line per convolution of one inference forward (reference GeneralModel/Hyper_unet_general.py:600-636), then the
families each case reaches and -- last -- which families NO case reaches.  tests/test_host_logic.py asserts the same.

    python tools/routing_table.py --fusions > profiles/fusion_table.txt

What the epilogues of the same forwards additionally do (tmdiff_amd.routing.unet_fusions): one line per ResBlock / wavelet block
with the fusions it takes, and per case the 1x1x1 launches and prologue passes that remain.

    python tools/routing_table.py --train > profiles/train_routing_table.txt

The finetune step itself (tmdiff_amd.routing.unet_train_launches over TRAIN_CASES): per case and per dropout setting the counted
launches of one forward_train plus backward, then one line per convolution with its forward, data-gradient and weight-gradient
families, and one per block with its plan."""
import collections
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tmdiff_amd import ops, routing  # noqa: E402


def main():
    reached, other = collections.Counter(), collections.Counter()
    print("# kernel family per 3x3x3 convolution (tmdiff_amd/routing.py; switches: defaults of ops.config)")
    print("# family -> C entry point / kernel: see the table at the top of tmdiff_amd/routing.py")
    for label, ch, b, n, size, math in routing.BASELINE_CASES + routing.OTHER_CASES:
        rows = routing.unet_table(ch, b, n, size, size, math)
        fams = collections.Counter(f for _, f in rows)
        (reached if (label, ch, b, n, size, math) in routing.BASELINE_CASES else other).update(fams)
        print(f"\n== {label}: channels {ch}, B = {b}, {n} bands, {size}x{size}, {math} -- "
              + ", ".join(f"{k} x{v}" for k, v in sorted(fams.items())))
        for L, fam in rows:
            split = ""
            if fam in ("wf", "wf_pair"):
                s = routing.wf_route(b, L.cin, L.cout, n, L.h, L.w, L.groups)[1]
                split = f" split-K {s}" if s > 1 else ""
            print(f"  {L.name:24s} {L.cin:4d}->{L.cout:<4d} g{L.groups} {n}x{L.h}x{L.w:<4d}"
                  f"{'' if L.plain else ' (segments)':11s} {fam}{split}")
    print("\n== families reached by the BASELINE cases: " + ", ".join(f"{k} ({v} layer instances)" for k, v in sorted(reached.items())))
    never = [f for f in routing.PRODUCT_FAMILIES + routing.FALLBACK_FAMILIES if f not in reached]
    print("== families reached by NO BASELINE case: " + (", ".join(never) if never else "none"))
    print("==   of these, reached by the reference's default / fixture widths (general-shape kernel, product path): "
          + (", ".join(f for f in never if f in other) or "none"))
    print("==   reached by neither (tmdiff_amd/fallback.py: even band counts other than 4 / 8, `fallback` test marker): "
          + (", ".join(f for f in never if f not in other) or "none"))


def fusions():
    print("# fusions per block of one inference forward (tmdiff_amd/routing.py unet_fusions; switches: defaults of ops.config)")
    print("# fold = res_conv / Conv_2 in the consumer's epilogue, side_xp = res_conv also writes conv20's prologue output,")
    print("# emit_ll = conv21 writes LL(y) / 2, s2d = second output in space-to-depth form, wfll / ll = Conv_0 + LL composed,")
    print("# dwt = Conv_0 writes the Haar transform; k1 = 1x1x1 launches left, passes = prologue passes left")
    for label, ch, b, n, size, math in routing.BASELINE_CASES + routing.OTHER_CASES:
        fuse = None
        if math == "bf16":      # (WavBEST._producer_fuse: only if every convolution runs on the bf16 kernels)
            all16 = all(c % 16 == 0 for c in ch) and all(
                ops.bf16_conv_supported(L.cout, L.cin, 3, L.groups, [L.cin // 3] if L.cin % 3 == 0 else None)
                for L in routing.unet_conv3_layers(ch, size, size))
            fuse = (all16 and ops.config.producer_fuse and ops.config.epilogue_fuse,) * 2
        rows = routing.unet_fusions(ch, b, n, size, size, math, fuse)
        print(f"\n== {label}: channels {ch}, B = {b}, {n} bands, {size}x{size}, {math} -- 1x1x1 launches left: "
              f"{sum(r.k1 for r in rows)} of 19, prologue passes left: {sum(r.passes for r in rows)}")
        for r in rows:
            print(f"  {r.block:16s} {r.kind:9s} k1 {r.k1} passes {r.passes}  {' '.join(r.taken) or '-'}")


def train():
    print("# launches of one finetune step, forward_train + backward (tmdiff_amd/routing.py unet_train_launches; switches: defaults of")
    print("# ops.config plus the ones named per case).  Per convolution: forward family / data-gradient family / weight-gradient")
    print("# kernel; +xp = the forward keeps x' for the weight gradient, +db = the bias gradient rides in the weight gradient (where")
    print("# there is a bias).  eval = dropout off (net.eval()), train = in-kernel dropout (net.train()).")
    for label, ch, b, n, size, switches in routing.TRAIN_CASES:
        with ops.config.override(**switches):
            runs = [(mode, routing.unet_train_launches(ch, b, n, size, size, mode == "train")) for mode in ("eval", "train")]
        print(f"\n== {label}: channels {ch}, B = {b}, {n} bands, {size}x{size}"
              + "".join(f", {k}={v}" for k, v in sorted(switches.items())))
        for mode, r in runs:
            print(f"  {mode:5s} " + ", ".join(f"{k} x{v}" for k, v in sorted(r.counts.items())))
        for name, plan in runs[0][1].blocks:
            what = plan if isinstance(plan, str) else f"Conv_0 {plan.conv0 or 'conv'}, Conv_2 {'after' if plan.conv2_after_ll else 'before'} LL"
            print(f"  {name:24s} {what}")
        for e, t in zip(runs[0][1].convs, runs[1][1].convs):
            cell = lambda r: f"{r.fwd}/{r.dgrad}/{r.wgrad}" + ("+xp" if r.keep_xp else "") + ("+db" if r.bias_in_wgrad else "")
            print((f"  {e.name:24s} {e.cin:4d}->{e.cout:<4d} g{e.groups} k{e.ksize} {n}x{e.h}x{e.w:<4d} {cell(e):24s}"
                   + ("" if cell(t) == cell(e) else f" train: {cell(t)}")).rstrip())


if __name__ == "__main__":
    {"--fusions": fusions, "--train": train}[sys.argv[1]]() if sys.argv[1:] else main()
