#!/usr/bin/env python3
"""Micro-benchmark of the standalone fp32 attention kernel (tmdiff_attn_fwd) and gemm_nt against the fp32 MFMA peak.
--backward: instead, the forward that stores LSE (tmdiff_attn_fwd_lse) and the backward (tmdiff_attn_bwd) at the shapes the
forward is reported at; the backward in TFLOP/s on the algorithmic count of five GEMMs of 2 Nq Nk D each (the two kernels
execute seven: each re-forms S and dP) and as a multiple of the forward's time.
--transformer: the memory-bound backward kernels around the attention core (tmdiff_layer_norm_bwd, tmdiff_group_norm_bwd,
tmdiff_geglu_bwd) at the shapes of one transformer block -- time and achieved bytes/s on the algorithmic traffic (every tensor
once), against the device copy rate measured in the same run -- and the forward / forward + backward time of one
BasicTransformerBlock (dim 512, 8 heads x 64, 1024 tokens, a 77 x 768 context)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from tmdiff_amd import ops

def timeit(fn, reps=10):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps

def backward_leg():
    for b, h, nq, nk, d in ((32, 8, 1024, 1024, 64), (32, 1, 1024, 1024, 128), (32, 8, 4096, 77, 64)):
        q, k, v, g = (torch.randn(b, n, h * d, device="cuda") for n in (nq, nk, nk, nq))
        sc = d ** -0.5
        out, lse = ops.attention_lse(q, k, v, sc, heads=h)
        fwd = timeit(lambda: ops.attention(q, k, v, sc, heads=h), 20)
        fwd_lse = timeit(lambda: ops.attention_lse(q, k, v, sc, heads=h), 20)
        bwd = timeit(lambda: ops.attention_bwd(q, k, v, out, g, lse, sc, heads=h), 20)
        bwd_q = timeit(lambda: ops.attention_bwd(q, k, v, out, g, lse, sc, heads=h, need=(True, False, False)), 20)
        bwd_kv = timeit(lambda: ops.attention_bwd(q, k, v, out, g, lse, sc, heads=h, need=(False, True, True)), 20)
        gemm = 2.0 * b * h * nq * nk * d
        print(f"attention backward B={b} H={h} Nq={nq} Nk={nk} D={d}: fwd {fwd:7.3f} ms, fwd+lse {fwd_lse:7.3f} ms, "
              f"bwd {bwd:7.3f} ms = {bwd / fwd:4.2f} x fwd, {5 * gemm / bwd / 1e9:6.1f} TFLOP/s algorithmic (5 GEMMs, "
              f"{5 * gemm / bwd / 1e9 / 157.3 * 100:4.1f}% of fp32 MFMA peak), {7 * gemm / bwd / 1e9:6.1f} TFLOP/s executed (7 GEMMs); "
              f"delta + dq {bwd_q:7.3f} ms, delta + dk/dv {bwd_kv:7.3f} ms", flush=True)


def transformer_leg(batch=32):
    from tmdiff_amd import Attention as A
    src = torch.randn(64 << 20, device="cuda")          # 256 MiB
    dst = torch.empty_like(src)
    ms = timeit(lambda: dst.copy_(src), 20)
    copy = 2 * src.numel() * 4 / ms / 1e9               # TB/s: read + write
    print(f"device copy of 256 MiB: {ms:7.3f} ms, {copy:5.2f} TB/s (read + write)", flush=True)
    del src, dst

    def report(what, ms, nbytes, note=""):
        rate = nbytes / ms / 1e9
        print(f"{what}: {ms:7.3f} ms, {rate:5.2f} TB/s = {rate / copy * 100:5.1f}% of the copy rate{note}", flush=True)

    rows, d = batch * 1024, 512
    x, dy = torch.randn(rows, d, device="cuda"), torch.randn(rows, d, device="cuda")
    gamma, beta = torch.randn(d, device="cuda"), torch.randn(d, device="cuda")
    _, mean, rstd = ops.layer_norm_stats(x, gamma, beta)
    n = rows * d * 4
    report(f"layer_norm_bwd rows={rows} D={d} (dx, dgamma, dbeta)", timeit(lambda: ops.layer_norm_bwd(x, gamma, dy, mean, rstd), 20), 3 * n)
    report(f"layer_norm_bwd rows={rows} D={d} (dx only)",
           timeit(lambda: ops.layer_norm_bwd(x, gamma, dy, mean, rstd, need=(True, False, False)), 20), 3 * n)
    report(f"layer_norm_bwd rows={rows} D={d} (dgamma, dbeta only)",
           timeit(lambda: ops.layer_norm_bwd(x, gamma, dy, mean, rstd, need=(False, True, True)), 20), 2 * n)
    x4, dy4 = x.view(batch, d, 32, 32), dy.view(batch, d, 32, 32)
    _, mean, rstd = ops.group_norm_stats(x4, gamma, beta, 32)
    report(f"group_norm_bwd B={batch} C={d} P=1024 groups=32 (dx, dgamma, dbeta)",
           timeit(lambda: ops.group_norm_bwd(x4, gamma, dy4, mean, rstd, 32), 20), 3 * n,
           " (x and dy are read by both passes: counted once)")
    report(f"group_norm_bwd B={batch} C={d} P=1024 groups=32 (dgamma, dbeta only: pass 1)",
           timeit(lambda: ops.group_norm_bwd(x4, gamma, dy4, mean, rstd, 32, need=(False, True, True)), 20), 2 * n)
    inner = 4 * d
    u, dyu = torch.randn(rows, 2 * inner, device="cuda"), torch.randn(rows, inner, device="cuda")
    report(f"geglu_bwd rows={rows} inner={inner}", timeit(lambda: ops.geglu_bwd(u, dyu), 20), 5 * rows * inner * 4)
    report(f"gelu_bwd rows={rows} inner={inner}", timeit(lambda: ops.geglu_bwd(dyu, dyu, gelu_only=True), 20), 3 * rows * inner * 4)
    del u, dyu
    blk = A.BasicTransformerBlock(512, 8, 64, context_dim=768).cuda()
    xb, ctx, g = torch.randn(batch, 1024, 512, device="cuda"), torch.randn(batch, 77, 768, device="cuda"), torch.randn(batch, 1024, 512, device="cuda")
    with torch.no_grad():
        fwd = timeit(lambda: blk(xb, context=ctx), 10)

    def step():
        blk.zero_grad(set_to_none=True)
        blk(xb, context=ctx).backward(g)
    both = timeit(step, 10)
    print(f"BasicTransformerBlock dim 512, 8 x 64, B={batch} x 1024 tokens, context 77 x 768: forward {fwd:7.3f} ms, "
          f"forward + backward (parameter gradients) {both:7.3f} ms = {both / fwd:4.2f} x forward", flush=True)


if "--transformer" in sys.argv[1:]:
    transformer_leg()
    sys.exit(0)
if "--backward" in sys.argv[1:]:
    backward_leg()
    sys.exit(0)

for b, h, nq, nk, d in ((32, 8, 1024, 1024, 64), (32, 1, 1024, 1024, 128), (32, 8, 4096, 77, 64), (32, 8, 4096, 4096, 32)):
    q, k, v = (torch.randn(b, n, h * d, device="cuda") for n in (nq, nk, nk))
    ms = timeit(lambda: ops.attention(q, k, v, d ** -0.5, heads=h))
    fl = 4.0 * b * h * nq * nk * d
    print(f"attention B={b} H={h} Nq={nq} Nk={nk} D={d}: {ms:7.3f} ms {fl / ms / 1e9:6.1f} TFLOP/s ({fl / ms / 1e9 / 157.3 * 100:4.1f}% of fp32 MFMA peak)", flush=True)
for m, n, k in ((32768, 512, 512), (32768, 1024, 128), (32 * 77, 512, 768)):
    a, w = torch.randn(m, k, device="cuda"), torch.randn(n, k, device="cuda")
    ms = timeit(lambda: ops.gemm_nt(a, w))
    fl = 2.0 * m * n * k
    print(f"gemm_nt M={m} N={n} K={k}: {ms:7.3f} ms {fl / ms / 1e9:6.1f} TFLOP/s ({fl / ms / 1e9 / 157.3 * 100:4.1f}%)", flush=True)
