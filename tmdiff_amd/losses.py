"""The opt-in composite finetune objective: today's residual loss plus a spectral-angle, a Laplacian and an SSIM term.

    L = base(x_hat, x0) + w_sam * SAM(x0 + MS, x_hat + MS) + w_lap * LAP(x_hat - x0) + w_dssim * (1 - SSIM(x0 + MS, x_hat + MS))

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
 * ``SSIM``: ``metrics.ssim`` of the images (a uniform 7 x 7 window per band plane, 'valid', sample covariance, data range 1),
   the mean over all windows; the term minimised is the dissimilarity ``dssim = 1 - SSIM`` (``ssim_loss_host``).

``spectral_spatial_loss_host`` is the definition, in float64 torch operations (any device) whose autograd gives the yardstick
gradient.  ``SpectralSpatialLoss`` is the product: one HIP kernel pair (csrc/loss.hip) that evaluates the terms and dL/dx_hat
together, in fp64, without atomics.  A term whose weight is 0 is not evaluated and reports 0.  With ``w_dssim > 0`` a second
kernel pair (csrc/ssim_loss.hip) adds the SSIM term's gradient to the one the first pair wrote and composes the values on the
device.  ``SSIMLoss`` is that second pair on its own.
"""
import math

import torch
import torch.nn.functional as F
from torch import nn

BASE_KINDS = ("l1", "l2", "smooth_l1")
TERM_FIELDS = ("total", "base", "sam", "lap")          # entries of SpectralSpatialLoss.last_terms
TERM_FIELDS5 = TERM_FIELDS + ("dssim",)                # ... with w_dssim > 0
TERM_KEYS = ("sam", "lap", "dssim")                    # keys of the loss_terms option


def check_weight(name, w):
    if not (isinstance(w, (int, float)) and not isinstance(w, bool) and 0.0 <= float(w) < math.inf):
        raise ValueError(f"loss term {name!r}: the weight must be a finite number >= 0, got {w!r}")
    return float(w)


def check_weights(base, w_sam, w_lap):
    if base not in BASE_KINDS:
        raise NotImplementedError(f"loss base {base!r}: one of {BASE_KINDS}")
    return check_weight("sam", w_sam), check_weight("lap", w_lap)


def parse_loss_terms(loss_terms):
    """``{"sam": w, "lap": w, "dssim": w}`` (every key optional) -> (w_sam, w_lap); ValueError for another key or a negative
    weight, the one of ``dssim`` included.  ``dssim_weight`` returns the third weight."""
    unknown = sorted(set(loss_terms) - set(TERM_KEYS))
    if unknown:
        raise ValueError(f"loss_terms: unknown key(s) {unknown}; the terms are 'sam', 'lap' and 'dssim'")
    dssim_weight(loss_terms)
    return check_weights("l1", loss_terms.get("sam", 0.0) or 0.0, loss_terms.get("lap", 0.0) or 0.0)


def dssim_weight(loss_terms):
    """The weight of the SSIM term in a ``loss_terms`` mapping (0 when absent)."""
    return check_weight("dssim", loss_terms.get("dssim", 0.0) or 0.0)


def ssim_loss_host(x_true, x_pred, win=7, data_range=1.0):
    """(dssim, ssim) as float64 scalars, differentiable in ``x_pred``: ``metrics.ssim``'s statistics (a uniform win x win mean
    per band plane over the 'valid' region, covariances scaled by n / (n - 1), n = win^2) on [B, C, H, W] tensors, ssim the mean
    of S over all B C (H - win + 1)(W - win + 1) windows.  The definition csrc/ssim_loss.hip is held to."""
    if x_true.dim() != 4 or x_true.shape != x_pred.shape:
        raise ValueError(f"ssim_loss_host: need two [B, C, H, W] tensors of one shape, got {tuple(x_true.shape)}, {tuple(x_pred.shape)}")
    h, w = x_true.shape[-2:]
    if win < 2 or h < win or w < win:
        raise ValueError(f"ssim_loss_host: a {win} x {win} window on {h} x {w} planes")
    a, b = x_true.double().reshape(-1, 1, h, w), x_pred.double().reshape(-1, 1, h, w)
    n = win * win
    box = torch.ones(1, 1, win, win, dtype=torch.float64, device=a.device) / n
    f = lambda t: F.conv2d(t, box)
    k = n / (n - 1.0)
    ux, uy = f(a), f(b)
    vx = k * (f(a * a) - ux * ux)
    vy = k * (f(b * b) - uy * uy)
    vxy = k * (f(a * b) - ux * uy)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
    ssim = s.mean()
    return 1.0 - ssim, ssim


def ssim_grad_closed_form(x_true, x_pred, win=7, data_range=1.0):
    """d dssim / d x_pred (float64) from the three per-window maps the kernel forms and the adjoint box filter: with
    A1 = 2 ux uy + c1, A2 = 2 vxy + c2, B1 = ux^2 + uy^2 + c1, B2 = vx + vy + c2, S = A1 A2 / (B1 B2) and k = n / (n - 1),
        Q = 2 k A1 / (B1 B2),  R = -k S / B2,  P = 2 ux A2 / (B1 B2) - 2 k ux A1 / (B1 B2) - 2 uy S / B1 + 2 k uy S / B2,
        grad[p] = -(1 / (n Nwin)) (sum P + x_true[p] sum Q + 2 x_pred[p] sum R), the sums over the windows that contain p."""
    shape = x_true.shape
    h, w = shape[-2:]
    a, b = x_true.detach().double().reshape(-1, 1, h, w), x_pred.detach().double().reshape(-1, 1, h, w)
    n = win * win
    ones = torch.ones(1, 1, win, win, dtype=torch.float64, device=a.device)
    f = lambda t: F.conv2d(t, ones / n)
    k = n / (n - 1.0)
    ux, uy = f(a), f(b)
    vx, vy, vxy = k * (f(a * a) - ux * ux), k * (f(b * b) - uy * uy), k * (f(a * b) - ux * uy)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    a1, a2, b1, b2 = 2 * ux * uy + c1, 2 * vxy + c2, ux * ux + uy * uy + c1, vx + vy + c2
    s = a1 * a2 / (b1 * b2)
    q = 2 * k * a1 / (b1 * b2)
    r = -k * s / b2
    p = 2 * ux * a2 / (b1 * b2) - 2 * k * ux * a1 / (b1 * b2) - 2 * uy * s / b1 + 2 * k * uy * s / b2
    adj = lambda t: F.conv_transpose2d(t, ones)          # the adjoint of the 'valid' box sum: a sum over the windows around p
    return (-(adj(p) + a * adj(q) + 2 * b * adj(r)) / (n * s.numel())).reshape(shape)


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
    of the last call -- no host read happens here; inside a captured graph it is the tensor the replays refill.  With
    ``w_dssim > 0`` the SSIM pair (7 x 7 window, data range 1, on x_start + ms and x_recon + ms) runs after the composite pair,
    adds its gradient to the composite one and writes ``last_terms`` as float64 [5] (TERM_FIELDS5); at 0 nothing changes."""

    def __init__(self, base="l1", w_sam=0.0, w_lap=0.0, w_dssim=0.0):
        super().__init__()
        self.w_sam, self.w_lap = check_weights(base, w_sam, w_lap)
        self.w_dssim = check_weight("dssim", w_dssim)
        self.base = base
        self.last_terms = None

    def extra_repr(self):
        more = f", w_dssim={self.w_dssim}" if self.w_dssim != 0.0 else ""
        return f"base={self.base!r}, w_sam={self.w_sam}, w_lap={self.w_lap}{more}"

    def forward(self, x_start, x_recon, ms=None):
        from . import autograd
        if self.w_dssim != 0.0:
            if ms is None:
                raise ValueError("SpectralSpatialLoss: the SSIM term scores x_start + ms against x_recon + ms and needs ms")
            total, terms = autograd.spectral_spatial_ssim_loss(x_start, x_recon, ms, self.base, self.w_sam, self.w_lap, self.w_dssim)
        else:
            total, terms = autograd.spectral_spatial_loss(x_start, x_recon, ms if self.w_sam != 0.0 else None, self.base,
                                                          self.w_sam, self.w_lap)
        self.last_terms = terms
        return total


class SSIMLoss(nn.Module):
    """``forward(x_true, x_pred)`` -> the float32 scalar ``dssim = 1 - SSIM``, differentiable in ``x_pred``, from the HIP kernel
    pair of csrc/ssim_loss.hip (float32 [B, C, H, W] tensors on the GPU; there is no host path behind it).  ``last_terms``: the
    float64 [2] device tensor (dssim, ssim) of the last call; no host read happens here."""

    def __init__(self, win=7, data_range=1.0):
        super().__init__()
        if not (isinstance(win, int) and win % 2 == 1 and 3 <= win <= 11):
            raise ValueError(f"SSIMLoss: win must be odd with 3 <= win <= 11, got {win!r}")
        if not 0.0 < float(data_range) < math.inf:
            raise ValueError(f"SSIMLoss: data_range must be finite and > 0, got {data_range!r}")
        self.win, self.data_range = win, float(data_range)
        self.last_terms = None

    def extra_repr(self):
        return f"win={self.win}, data_range={self.data_range}"

    def forward(self, x_true, x_pred):
        from . import autograd
        total, terms = autograd.ssim_loss(x_true, x_pred, self.win, self.data_range)
        self.last_terms = terms
        return total


class LocalCorrLoss(nn.Module):
    """``forward(x, pan)`` -> the float32 scalar mean of max(0, rho_max_c - rho) over the bands and all win x win windows, rho the
    local correlation coefficient of a band of x [B, C, H, W] with pan [B, 1, H, W] (``metrics.local_corr_loss``), differentiable
    in ``x``, from the HIP kernel pair of csrc/local_corr.hip (float32 tensors on the GPU; there is no host path behind it).
    ``rho_max``: None (1.0), a number, or one per band.  ``last_terms``: the float64 [2] device tensor (loss, mean rho) of the
    last call; no host read happens here."""

    def __init__(self, win=4, rho_max=None):
        super().__init__()
        if not (isinstance(win, int) and 2 <= win <= 8):
            raise ValueError(f"LocalCorrLoss: win must be a whole number with 2 <= win <= 8, got {win!r}")
        if rho_max is not None:
            rho_max = tuple(float(v) for v in rho_max) if hasattr(rho_max, "__len__") else float(rho_max)
            if not all(math.isfinite(v) for v in (rho_max if isinstance(rho_max, tuple) else (rho_max,))):
                raise ValueError(f"LocalCorrLoss: rho_max must be finite, got {rho_max!r}")
        self.win, self.rho_max = win, rho_max
        self.last_terms = None

    def extra_repr(self):
        return f"win={self.win}, rho_max={self.rho_max}"

    def forward(self, x, pan):
        from . import autograd
        total, terms = autograd.local_corr_loss(x, pan, self.win, self.rho_max)
        self.last_terms = terms
        return total
