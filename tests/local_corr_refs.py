"""Inputs shared by tests/test_local_corr_host.py and tests/test_gpu_local_corr.py, and the slowest possible statement of the
local correlation coefficient: one window at a time."""
import numpy as np
import torch

U = 2.0 ** -53


def triple_loop(x, pan, win):
    """rho of every window from plain Python loops over (plane, row, column): two passes per window, 0 where S_xx S_pp == 0."""
    x, pan = np.asarray(x, dtype=np.float64), np.asarray(pan, dtype=np.float64)
    b, c, h, w = x.shape
    out = np.zeros((b, c, h - win + 1, w - win + 1))
    for i in range(b):
        for k in range(c):
            for y in range(h - win + 1):
                for z in range(w - win + 1):
                    a, p = x[i, k, y:y + win, z:z + win].ravel(), pan[i, 0, y:y + win, z:z + win].ravel()
                    da, dp = a - a.sum() / a.size, p - p.sum() / p.size
                    den2 = float(da @ da) * float(dp @ dp)
                    out[i, k, y, z] = 0.0 if den2 == 0.0 else float(da @ dp) / np.sqrt(den2)
    return out


def random_pair(seed, shape, mix=0.6):
    """float32 x [B, C, H, W] ~ U[0, 1) and pan = mix * (band mean of x) + (1 - mix) * U[0, 1): correlated with every band, rho
    well inside (-1, 1)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(*shape, generator=g)
    pan = mix * x.mean(1, keepdim=True) + (1.0 - mix) * torch.rand(shape[0], 1, *shape[2:], generator=g)
    return x, pan


def grid_pair(seed, shape, mix_num=3):
    """A correlated pair on the grid of multiples of 2^-10 in [0, 1]: pan = k / 1024, x_c = the rounding down to the grid of
    (mix_num * pan + (8 - mix_num) * noise_c) / 8, so every band has rho around 0.5.  Every window sum of such values is exact
    in float64 in any order for win in {2, 4, 8}: the means are multiples of 2^-16, the centred values too, their products
    multiples of 2^-32 below 1, and 64 of them fit 53 bits."""
    g = torch.Generator().manual_seed(seed)
    kp = torch.randint(0, 1025, (shape[0], 1, *shape[2:]), generator=g)
    kn = torch.randint(0, 1025, shape, generator=g)
    kx = (mix_num * kp + (8 - mix_num) * kn) // 8
    return (kx.double() / 1024.0).float(), (kp.double() / 1024.0).float()


def smooth_scene(seed=5, shape=(1, 4, 48, 48)):
    """The scene of the structure_refine tests: bands of 3 x 3 box-smoothed uniform noise, and a PAN that is the band mean plus
    noise of a third of its spread: float32 in [0, 1]."""
    g = torch.Generator().manual_seed(seed)
    b, c, h, w = shape
    raw = torch.rand(b, c, h + 2, w + 2, generator=g)
    x = torch.nn.functional.avg_pool2d(raw, 3, 1)
    pan = x.mean(1, keepdim=True)
    pan = pan + (float(pan.std()) / 3.0) * torch.randn(b, 1, h, w, generator=g)
    return x.contiguous(), pan.clamp(0.0, 1.0).contiguous()


def window_spread(x, win):
    """min over the windows of (max - min) / max|value|: the per-window spread relative to the magnitude"""
    v = np.lib.stride_tricks.sliding_window_view(np.asarray(x, dtype=np.float64), (win, win), axis=(2, 3))
    return float(((v.max((-2, -1)) - v.min((-2, -1))) / np.abs(v).max((-2, -1))).min())
