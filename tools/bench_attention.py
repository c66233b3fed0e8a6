#!/usr/bin/env python3
"""Micro-benchmark of the standalone fp32 attention kernel (tmdiff_attn_fwd) and gemm_nt against the fp32 MFMA peak.
--backward: instead, the forward that stores LSE (tmdiff_attn_fwd_lse) and the backward (tmdiff_attn_bwd) at the shapes the
forward is reported at; the backward in TFLOP/s on the algorithmic count of five GEMMs of 2 Nq Nk D each (the two kernels
execute seven: each re-forms S and dP) and as a multiple of the forward's time."""
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
