#!/usr/bin/env python3
"""Generate tests/golden/metrics_suite.npz: the REFERENCE's own reduced- and full-resolution quality metrics
(core/metrics.py: ERGAS_numpy, RMSE_numpy, CC_numpy, UIQC_numpy, Q4_numpy, SCC_torch band by band, QIndex_torch,
D_lambda_torch, D_s_torch) on the hr / sr arrays of tests/golden/metrics.npz cast to float64, plus a small pan, l_pan and l_ms
built from them.  Results and the three derived inputs only are stored; run it where the reference checkout exists:

    python tools/make_metrics_golden.py
"""
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shims  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = ("wv3_f32", "gf2_f32", "wv3_f64")


def block_mean4(x):
    """[H, W, ...] -> [H // 4, W // 4, ...]: mean of 4 x 4 blocks of the top-left multiple-of-4 crop, rounded to float32."""
    h, w = x.shape[0] // 4 * 4, x.shape[1] // 4 * 4
    y = x[:h, :w].reshape(h // 4, 4, w // 4, 4, *x.shape[2:]).mean(axis=(1, 3))
    return y.astype(np.float32).astype(np.float64)


def nchw(x):
    """[H, W, C] or [H, W] float64 -> [1, C, H, W] tensor"""
    x = x[..., None] if x.ndim == 2 else x
    return torch.from_numpy(np.ascontiguousarray(np.moveaxis(x, -1, 0)))[None]


def main():
    ref_shims.install_metrics_stand_ins()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        from core import metrics as RM
    src = np.load(os.path.join(GOLDEN, "metrics.npz"))
    out = {}
    for tag in CASES:
        hr, sr = src[f"{tag}_hr"].astype(np.float64), src[f"{tag}_sr"].astype(np.float64)
        c = hr.shape[-1]
        # full-resolution stand-ins: pan = band mean of the target, the low-resolution pair = 4 x 4 block means
        pan = hr.mean(axis=-1).astype(np.float32).astype(np.float64)
        l_pan, l_ms = block_mean4(pan), block_mean4(hr)
        out[f"{tag}_pan"], out[f"{tag}_l_pan"], out[f"{tag}_l_ms"] = pan, l_pan, l_ms
        with np.errstate(all="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out[f"{tag}_rmse"] = np.float64(RM.RMSE_numpy(hr, sr))
            out[f"{tag}_ergas"] = np.float64(RM.ERGAS_numpy(hr, sr))
            out[f"{tag}_ergas_swapped"] = np.float64(RM.ERGAS_numpy(sr, hr, ratio=0.5))
            out[f"{tag}_cc"] = np.float64(RM.CC_numpy(hr, sr))
            out[f"{tag}_q"] = np.float64(RM.UIQC_numpy(hr, sr))
            if c == 4:
                out[f"{tag}_q4"] = np.float64(RM.Q4_numpy(hr, sr))
            out[f"{tag}_scc"] = np.float64(np.mean([float(RM.SCC_torch(nchw(hr[..., k]), nchw(sr[..., k]))) for k in range(c)]))
            t_lms, t_pan, t_lpan, t_ps = nchw(l_ms), nchw(pan), nchw(l_pan), nchw(sr)
            dl = float(RM.D_lambda_torch(t_lms, t_ps))
            ds = float(RM.D_s_torch(t_lms, t_pan, t_lpan, t_ps))
            out[f"{tag}_q_pop01"] = np.float64(float(RM.QIndex_torch(t_ps[:, 0], t_ps[:, 1])))
            out[f"{tag}_d_lambda"], out[f"{tag}_d_s"], out[f"{tag}_qnr"] = np.float64(dl), np.float64(ds), np.float64((1 - dl) * (1 - ds))
    out["torch_version"] = np.asarray(torch.__version__)
    path = os.path.join(GOLDEN, "metrics_suite.npz")
    np.savez_compressed(path, **out)
    print(f"metrics_suite: {os.path.getsize(path) / 1024:.1f} KiB, {len(out) - 1} arrays")


if __name__ == "__main__":
    main()
