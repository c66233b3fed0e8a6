"""The opt-in composite finetune objective: today's residual loss plus a spectral-angle and a Laplacian term.

    L = base(x_hat, x0) + w_sam * SAM(x0 + MS, x_hat + MS) + w_lap * LAP(x_hat - x0)

``x0`` is the residual the network is trained to predict (``x_in["Res"]``), ``x_hat`` its output and ``MS`` the upsampled
multispectral image, all [B, C, H, W].  The reference carries such terms beside its ``set_loss`` without reaching them
(utils/util.py:756-770 ``sam`` / ``lap_loss``, core/mylib.py:1024 ``SAMLoss``); here they are what ``metrics.quality`` scores:

 * ``base``: the mean over all elements of rho(x_hat - x0): ``l1``, ``l2`` or ``smooth_l1`` with beta = 1 (torch's three).
 * ``SAM``: the mean over the B H W pixels of the angle in radians between the band vectors u = x0 + MS and v = x_hat + MS --
   on the images, not on the residuals -- as atan2(|cross|, dot) with |cross|^2 = |u|^2 |v|^2 - dot^2, which keeps small
   angles accurate where acos does not.  A pixel with |u| = 0, |v| = 0 or |cross|^2 <= 0 (u parallel to v) contributes its
   angle (0, or pi for antiparallel vectors) and no gradient; with one band every pixel does.
 * ``LAP``: the mean over the B C (H - 2)(W - 2) interior pixels of |Lap (x_hat - x0)|, Lap the 3 x 3 kernel with -8 at the
   centre and 1 on the eight neighbours: the 'valid' region ``metrics.scc`` uses.

``spectral_spatial_loss_host`` is the definition, in float64 torch operations (any device) whose autograd gives the yardstick
gradient.  ``SpectralSpatialLoss`` is the product: one HIP kernel pair (csrc/loss.hip) that evaluates the terms and dL/dx_hat
together, in fp64, without atomics.  A term whose weight is 0 is not evaluated and reports 0.
"""
import math

import torch
from torch import nn

BASE_KINDS = ("l1", "l2", "smooth_l1")
TERM_FIELDS = ("total", "base", "sam", "lap")          # entries of SpectralSpatialLoss.last_terms


def check_weights(base, w_sam, w_lap):
    if base not in BASE_KINDS:
        raise NotImplementedError(f"loss base {base!r}: one of {BASE_KINDS}")
    for name, w in (("sam", w_sam), ("lap", w_lap)):
        if not (isinstance(w, (int, float)) and not isinstance(w, bool) and 0.0 <= float(w) < math.inf):
            raise ValueError(f"loss term {name!r}: the weight must be a finite number >= 0, got {w!r}")
    return float(w_sam), float(w_lap)


def parse_loss_terms(loss_terms):
    """``{"sam": w, "lap": w}`` (either key optional) -> (w_sam, w_lap); ValueError for another key or a negative weight."""
    unknown = sorted(set(loss_terms) - {"sam", "lap"})
    if unknown:
        raise ValueError(f"loss_terms: unknown key(s) {unknown}; the terms are 'sam' and 'lap'")
    return check_weights("l1", loss_terms.get("sam", 0.0) or 0.0, loss_terms.get("lap", 0.0) or 0.0)


def spectral_spatial_loss_host(x0, xhat, ms, base="l1", w_sam=0.0, w_lap=0.0):
    """(total, base, sam, lap) as float64 scalars, differentiable in ``xhat``: the definition the kernel is held to."""
    w_sam, w_lap = check_weights(base, w_sam, w_lap)
    x0, xhat = x0.double(), xhat.double()
    d = xhat - x0
    ad = d.abs()
    if base == "l1":
        l_base = ad.mean()
    elif base == "l2":
        l_base = (d * d).mean()
    else:
        l_base = torch.where(ad < 1.0, 0.5 * d * d, ad - 0.5).mean()
    zero = torch.zeros((), dtype=torch.float64, device=d.device)
    l_sam = l_lap = zero
    if w_sam != 0.0:
        m = ms.double()
        u, v = x0 + m, xhat + m
        dot, nu, nv = (u * v).sum(1), (u * u).sum(1), (v * v).sum(1)
        cr2 = nu * nv - dot * dot
        ok = (nu > 0) & (nv > 0) & (cr2 > 0)
        if u.shape[1] == 1:                 # one band: u and v are parallel, whatever the rounding of the two products says
            ok = torch.zeros_like(ok)
        # the arguments of the pixels left out are replaced before sqrt / atan2 see them, so that their gradient is 0, not NaN
        ang = torch.atan2(torch.sqrt(torch.where(ok, cr2, torch.ones_like(cr2))), torch.where(ok, dot, torch.ones_like(dot)))
        flat = torch.where(dot.detach() < 0, torch.full_like(dot, math.pi), torch.zeros_like(dot))
        l_sam = torch.where(ok, ang, flat).mean()
    if w_lap != 0.0:
        h, w = d.shape[-2:]
        if h < 3 or w < 3:
            raise ValueError(f"the Laplacian term needs H, W >= 3, got {h} x {w}")
        ring = sum(d[..., 1 + i:h - 1 + i, 1 + j:w - 1 + j] for i in (-1, 0, 1) for j in (-1, 0, 1) if (i, j) != (0, 0))
        l_lap = (ring - 8.0 * d[..., 1:-1, 1:-1]).abs().mean()
    return l_base + w_sam * l_sam + w_lap * l_lap, l_base, l_sam, l_lap


class SpectralSpatialLoss(nn.Module):
    """``forward(x_start, x_recon, ms)`` -> the float32 scalar loss, differentiable in ``x_recon``, from the HIP kernel pair
    (float32 tensors on the GPU; there is no host path behind it).  ``last_terms``: the float64 [4] device tensor (TERM_FIELDS)
    of the last call -- no host read happens here; inside a captured graph it is the tensor the replays refill."""

    def __init__(self, base="l1", w_sam=0.0, w_lap=0.0):
        super().__init__()
        self.w_sam, self.w_lap = check_weights(base, w_sam, w_lap)
        self.base = base
        self.last_terms = None

    def extra_repr(self):
        return f"base={self.base!r}, w_sam={self.w_sam}, w_lap={self.w_lap}"

    def forward(self, x_start, x_recon, ms=None):
        from . import autograd
        total, terms = autograd.spectral_spatial_loss(x_start, x_recon, ms if self.w_sam != 0.0 else None, self.base,
                                                      self.w_sam, self.w_lap)
        self.last_terms = terms
        return total
