#!/usr/bin/env python3
"""BASELINE config 4 shaped finetune loop on synthetic PAN/MS tiles: global batch 64 = 8 GPUs x 8, ch 32-256,
AdamW lr 1e-4, dropout on, SUM gradient all-reduce over RCCL, EMA.  Single GPU:  python examples/finetune_synthetic.py
8 GPUs: python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 examples/finetune_synthetic.py"""
import argparse, copy, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from tmdiff_amd import dist as tdist
from tmdiff_amd.model import DDPM, EmaUpdater
from tmdiff_amd.util import synthetic_tile_batch

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--local-batch", type=int, default=8)
ap.add_argument("--channels", type=int, nargs=4, default=[32, 64, 128, 256])
ap.add_argument("--max-grad-norm", type=float, default=None, help="clip the global gradient norm inside the AdamW step")
ap.add_argument("--grad-bf16", action="store_true", help="gradients of the 3x3x3 convolutions from bf16-rounded operands (fp32 sums)")
ap.add_argument("--sam-weight", type=float, default=None, help="add w * (mean spectral angle of the fused image) to the loss")
ap.add_argument("--lap-weight", type=float, default=None, help="add w * (mean |Laplacian| of the residual error) to the loss")
ap.add_argument("--dssim-weight", type=float, default=None, help="add w * (1 - SSIM of the fused image, 7 x 7 windows) to the loss")
args = ap.parse_args()
world = tdist.init_from_env()
rank = int(os.environ.get("RANK", "0"))
torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
opt = {"phase": "train", "gpu_ids": [0], "distributed": world > 1, "path": {"resume": None, "checkpoint": "/tmp/tmdiff_ckpt"},
       "model": {"unet": {"channel_multiplier": args.channels}, "diffusion": {"loss_type": "l1"}, "init_type": "orthogonal"},
       "train": {"optimizer": {"lr": 1e-4}, "max_iter": 150000}}
if args.max_grad_norm is not None:
    opt["train"]["max_grad_norm"] = args.max_grad_norm
if args.grad_bf16:
    opt["train"]["grad_compute"] = "bf16"
terms = {k: w for k, w in (("sam", args.sam_weight), ("lap", args.lap_weight), ("dssim", args.dssim_weight)) if w is not None}
if terms:                                   # the composite loss of tmdiff_amd.losses: HIP kernel pairs, value and gradient
    opt["model"]["diffusion"]["loss_terms"] = terms
torch.manual_seed(3407)                     # identical initial weights on every rank
model = DDPM(opt)
ema = EmaUpdater(model, copy.deepcopy(model))
model.set_new_noise_schedule({"schedule": "cosine", "n_timestep": 1000}, "train")
for it in range(args.iters):
    model.feed_data(synthetic_tile_batch(1000 * rank + it, args.local_batch, 8, 64))
    torch.cuda.synchronize(); t0 = time.perf_counter()
    model.optimize_parameters("WV3")
    ema.update(it)
    torch.cuda.synchronize()
    if rank == 0:
        log = model.get_current_log()
        clip = f" grad_norm {log['grad_norm']:.3f} skipped {log['skipped']:.0f}" if "grad_norm" in log else ""
        parts = "".join(f" {k} {float(log[k]):.4f}" for k in ("l_base", "l_sam", "l_lap", "l_dssim") if k in log)
        print(f"iter {it}: l_pix {float(log['l_pix']):.4f}{parts} lr {log['lr']:.2e}{clip} {1e3 * (time.perf_counter() - t0):.1f} ms", flush=True)
