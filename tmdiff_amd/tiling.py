"""Tile helpers for large scenes (SURVEY 5 "long context", 8f N3; reference data/LRHR_dataset.py:17-53).

``invPatch`` / ``patch_16`` / ``unpatch_16`` keep the reference's names and row-major tile order; ``split_tiles`` /
``merge_tiles`` generalise them to any grid.  ``sample_tiled`` is BASELINE config 5: a large scene is cut into
independent tiles that are sharded over the ranks of the process group (no collective during sampling, one
all-gather at the end).  WavBEST is fully convolutional with zero padding, so tiled output differs from
full-frame output within 3x3x3-receptive-field distance of the tile seams -- same as the reference's tiling.

Fused mode (``sample_tiled(..., overlap=k)``, ``TiledDenoiser``): ONE noisy scene is kept; at every denoise step
overlapping tiles are cut out of it (``ops.tile_gather``), the network runs on the tiles and its outputs are blended
back into one scene-sized prediction (``ops.tile_blend``) that the sampler steps as a whole, so noise, clamp and
dynamic thresholding act per scene and a tile's influence fades towards its border.  ``plan_tiles`` is the tile plan.
"""
import numpy as np
import torch
from torch import nn

from . import dist as tdist
from . import ops


def _plan_axis(length, tile, overlap):
    step = tile - overlap
    origins = list(range(0, length - tile + 1, step))
    if origins[-1] != length - tile:
        origins.append(length - tile)          # the last tile is pushed inwards: no tile leaves the scene, no padding
    return origins


def plan_tiles(h, w, tile, overlap):
    """(row origins, column origins) of the overlapped tiles of an h x w scene: per axis 0, s, 2s, ... with
    s = tile - overlap while origin + tile <= L, plus L - tile if the last one does not end at L.  Tiles are numbered
    row-major per scene sample, as ``split_tiles`` does.  ``tile % 8 == 0`` (three wavelet levels)."""
    if tile <= 0 or tile % 8:
        raise ValueError(f"tile={tile}: need a positive multiple of 8 (three wavelet levels)")
    if not 0 <= overlap <= tile // 2:
        raise ValueError(f"overlap={overlap}: need 0 <= overlap <= tile // 2 = {tile // 2}")
    if h < tile or w < tile:
        raise ValueError(f"a {h} x {w} scene is smaller than one {tile} x {tile} tile")
    return _plan_axis(h, tile, overlap), _plan_axis(w, tile, overlap)


def tile_profile(tile, overlap):
    """1-D blend weights w1(i) = min(i + 1, tile - i, overlap + 1), float64; a tile's 2-D weight is w1(y) * w1(x) and a scene
    pixel is sum(w v) / sum(w) over the tiles that cover it."""
    i = torch.arange(tile, dtype=torch.float64)
    return torch.minimum(torch.minimum(i + 1, tile - i), torch.full_like(i, overlap + 1))


class TiledDenoiser(nn.Module):
    """Scene-shaped outside, tile-shaped inside: ``forward`` has ``WavBEST.forward``'s signature, takes scene tensors
    [B, C, H, W] and returns the scene-sized blend of ``net``'s predictions on the overlapped tiles, run in chunks of at
    most ``max_batch`` tiles.  Inside ``begin_condition_cache`` / ``end_condition_cache`` the PAN / MS tiles are gathered
    once and ``net``'s condition branch runs once per chunk for the whole run."""

    def __init__(self, net, tile=64, overlap=16, max_batch=32):
        super().__init__()
        plan_tiles(tile, tile, tile, overlap)             # argument check
        if max_batch < 1:
            raise ValueError(f"max_batch={max_batch}")
        self.net, self.tile, self.overlap, self.max_batch = net, tile, overlap, max_batch
        self._run = None

    @staticmethod
    def _key(PAN, MS, prompt):
        k = lambda t: (t.data_ptr(), t._version, tuple(t.shape), tuple(t.stride()))
        return k(PAN), k(MS), tuple(prompt) if isinstance(prompt, (list, tuple)) else prompt

    def _chunks(self, PAN, MS, prompt):
        """[(PAN tiles, MS tiles, prompt)] per chunk of at most max_batch tiles."""
        b, _, h, w = MS.shape
        rows, cols = plan_tiles(h, w, self.tile, self.overlap)
        per = len(rows) * len(cols)
        pan_t = ops.tile_gather(PAN.float().contiguous(), self.tile, self.overlap)
        ms_t = ops.tile_gather(MS.float().contiguous(), self.tile, self.overlap)
        if isinstance(prompt, (list, tuple)):
            if len(prompt) != b:
                raise ValueError("per-sample prompt list must have one entry per batch element")
            prompts = [p for p in prompt for _ in range(per)]
        out = []
        for lo in range(0, b * per, self.max_batch):
            hi = min(lo + self.max_batch, b * per)
            out.append((pan_t[lo:hi], ms_t[lo:hi], prompts[lo:hi] if isinstance(prompt, (list, tuple)) else prompt))
        return out

    def begin_condition_cache(self, PAN, MS, prompt):
        self.end_condition_cache()
        chunks = self._chunks(PAN, MS, prompt)
        self._run = (self._key(PAN, MS, prompt), chunks)
        if hasattr(self.net, "add_condition_cache"):
            try:
                for i, (pan, ms, pr) in enumerate(chunks):
                    (self.net.begin_condition_cache if i == 0 else self.net.add_condition_cache)(pan, ms, pr)
            except BaseException:
                self.end_condition_cache()        # nothing half-open is left behind
                raise

    def end_condition_cache(self):
        if self._run is not None and hasattr(self.net, "end_condition_cache"):
            self.net.end_condition_cache()
        self._run = None

    @torch.no_grad()
    def forward(self, x_t, t_input, PAN=None, MS=None, prompt=None):
        b, _, h, w = x_t.shape
        rows, cols = plan_tiles(h, w, self.tile, self.overlap)
        per = len(rows) * len(cols)
        if self._run is not None and self._run[0] == self._key(PAN, MS, prompt):
            chunks = self._run[1]
        else:
            chunks = self._chunks(PAN, MS, prompt)
        x_tiles = ops.tile_gather(x_t.float().contiguous(), self.tile, self.overlap)
        t = t_input.reshape(-1)
        t = (t if t.numel() == b else t.expand(b)).repeat_interleave(per)
        outs, lo = [], 0
        for pan, ms, pr in chunks:
            hi = lo + pan.shape[0]
            outs.append(self.net(x_tiles[lo:hi], t[lo:hi].reshape(-1, 1), pan, ms, pr))
            lo = hi
        y = outs[0] if len(outs) == 1 else torch.cat(outs)
        return ops.tile_blend(y.contiguous(), b, h, w, self.overlap)


def split_tiles(img, th, tw):
    """[B, C, H, W] -> [B * (H/th) * (W/tw), C, th, tw], tiles in row-major order per image."""
    b, c, h, w = img.shape
    assert h % th == 0 and w % tw == 0, "scene must be a whole number of tiles"
    t = img.reshape(b, c, h // th, th, w // tw, tw).permute(0, 2, 4, 1, 3, 5)
    return t.reshape(-1, c, th, tw).contiguous()


def merge_tiles(tiles, rows, cols):
    """inverse of split_tiles: [B*rows*cols, C, th, tw] -> [B, C, rows*th, cols*tw]"""
    n, c, th, tw = tiles.shape
    b = n // (rows * cols)
    t = tiles.reshape(b, rows, cols, c, th, tw).permute(0, 3, 1, 4, 2, 5)
    return t.reshape(b, c, rows * th, cols * tw).contiguous()


def invPatch(img_MS):
    """(1, c, h, w) -> (4, c, h/2, w/2): the four quadrants (reference :17-25)."""
    return split_tiles(img_MS, img_MS.shape[2] // 2, img_MS.shape[3] // 2)


def patch_16(img_MSs):
    """(16, c, h, w) -> (c, 4h, 4w) (reference :28-37)."""
    return merge_tiles(torch.as_tensor(img_MSs), 4, 4)[0]


def unpatch_16(patch):
    """(c, 4h, 4w) -> (16, c, h, w) (reference :40-53)."""
    p = torch.as_tensor(patch)
    return split_tiles(p[None], p.shape[1] // 4, p.shape[2] // 4)


_IN_LOOP_NEEDS_FUSED = ("consistency inside the sampler steps needs the fused tile mode (overlap=k), where the sampler steps the scene "
                        "as a whole: in the independent mode a tile's border is not the scene's replicate border")


@torch.no_grad()
def sample_tiled(diffusion, scene, prompt, tile=64, method="dpmsolver", steps=20, max_batch=32, overlap=None, consistency=None):
    """Fuse a large scene tile by tile.  ``scene`` = {'MS': [B,C,H,W], 'PAN': [B,1,H,W]} (Res optional).

    ``overlap=None`` (independent mode): disjoint tiles, one diffusion chain per tile with its own noise and its own
    dynamic threshold, outputs butted together.  Tiles are sharded over the ranks; each rank samples its share in
    batches of ``max_batch`` and the fused tiles are gathered and stitched on every rank.  The scene must be a whole
    number of tiles.

    ``overlap=k >= 0`` (fused mode): the scene is sampled as ONE chain by ``diffusion.sample`` with a ``TiledDenoiser``
    in place of ``diffusion.denoise_fn`` for the duration of the call: tiles that overlap by k pixels are cut out of the
    noisy scene at every step and the network's outputs are blended, so clamp and dynamic thresholding act per scene
    and no seam is left.  Scene extents need not be multiples of the tile.  The UNet work grows by about
    (tile / (tile - k))^2.  Not covered: more than one rank (ValueError; use the independent mode -- sharding tiles per
    step needs an all-gather per step), captured-graph sampling (the fused mode runs eagerly, with the same result, also
    when ``sample_graph`` is on), the gather folded into the stem kernel, training.

    ``consistency``: the in-loop projection of ``GeneralDiffusion.sample_by_dpmsolver``, handed to ``diffusion.sample``; fused
    mode only, because there the sampler steps the scene as a whole -- a tile's border is not the scene's replicate border, so
    the independent mode raises ValueError."""
    if consistency is not None and overlap is None:
        raise ValueError(_IN_LOOP_NEEDS_FUSED)
    if overlap is not None:
        if tdist.dist.is_initialized() and tdist.dist.get_world_size() > 1:
            raise ValueError("sample_tiled: the fused mode (overlap=k) runs on one rank only; use the independent mode "
                             "(overlap=None) under a process group")
        ms = scene["MS"]
        plan_tiles(ms.shape[2], ms.shape[3], tile, overlap)
        x_in = {"MS": ms, "PAN": scene["PAN"], "Res": scene["Res"] if "Res" in scene else torch.zeros_like(ms)}
        net = diffusion.denoise_fn
        wrapped = TiledDenoiser(net, tile, overlap, max_batch)
        diffusion.denoise_fn = wrapped
        try:
            return diffusion.sample(x_in, prompt, method=method, **({"steps": steps} if method == "dpmsolver" else {}),
                                    **({} if consistency is None else {"consistency": consistency}))
        finally:
            diffusion.denoise_fn = net
            wrapped.end_condition_cache()
    ms, pan = scene["MS"], scene["PAN"]
    rows, cols = ms.shape[2] // tile, ms.shape[3] // tile
    tiles = {"MS": split_tiles(ms, tile, tile), "PAN": split_tiles(pan, tile, tile)}
    tiles["Res"] = split_tiles(scene["Res"], tile, tile) if "Res" in scene else torch.zeros_like(tiles["MS"])
    n = tiles["MS"].shape[0]
    world = tdist.dist.get_world_size() if tdist.dist.is_initialized() else 1
    rank = tdist.dist.get_rank() if tdist.dist.is_initialized() else 0
    pad = (-n) % world                                   # equal shares so that the final all-gather is regular
    if pad:
        tiles = {k: torch.cat([v, v[:pad]]) for k, v in tiles.items()}
    mine = tdist.shard_batch(tiles, rank, world) if world > 1 else tiles
    outs = []
    for lo in range(0, mine["MS"].shape[0], max_batch):
        part = {k: v[lo:lo + max_batch].contiguous() for k, v in mine.items()}
        outs.append(diffusion.sample(part, prompt, method=method, **({"steps": steps} if method == "dpmsolver" else {})))
    fused = tdist.gather_images(torch.cat(outs))[:n]
    return merge_tiles(fused, rows, cols)


@torch.no_grad()
def consistency_refine(fused, lr_ms, sensor, ratio=4, iters=8, relax=1.0, out=None):
    """Pull a fused scene towards Wald's consistency property A(fused) = lr_ms, A = ``mtf_degrade(., sensor, ratio)``: ``iters``
    Landweber steps on 1/2 ||A f - lr_ms||^2,
      r = A f - lr_ms;   f <- f - (relax / ||A_c||^2) A_c^T r      per band c, ||A_c||^2 = ``metrics.mtf_opnorm2(gain_c, ratio)``
    with 0 < relax < 2 (inside it the residual norm cannot grow) and iters >= 0; fused [B, C, H, W], lr_ms [B, C, H', W'] the
    extent of ``mtf_degrade``; ``sensor`` is looked up through ``metrics.band_gains``.  Tensors on the GPU go through the
    operators, three launches per step: ``ops.mtf_degrade``, ``ops.add`` (the subtraction) and ``ops.mtf_degrade_adjoint`` with
    alpha = -1, beta = 1 and the scene as its own base.  The per-band step goes in as a SCALED COPY OF THE TAP TABLE (the
    kernel's alpha is one number), made in float64 and cached beside the plain table: call once before capturing; nothing is
    read back, so the loop can be captured.  Host tensors and arrays go through the float64 definitions.  ``out`` (device):
    receives the result and may be ``fused``; otherwise ``fused`` is left as it is.
    Convergence: A is ill-conditioned (squared singular values from about 0.08 down to 1e-4 at x4), so the steps remove the
    smooth part of the residual quickly and the rest slowly: on a 4 x 48 x 48 white-noise scene started from
    ``upsample_poly23`` the residual RMS falls to 0.78 of its start in one step at relax = 1 and to 0.30 in 8
    (tests/test_mtf_adjoint_host.py), each step gaining less than the one before.  It is a refinement, not a solve."""
    from . import metrics
    if not 0.0 < float(relax) < 2.0 or int(iters) != iters or iters < 0:
        raise ValueError(f"consistency_refine: relax={relax} iters={iters} (0 < relax < 2, iters a whole number >= 0)")
    if len(fused.shape) != 4 or tuple(lr_ms.shape) != (*fused.shape[:2], *metrics.fir_decimate_shape(*fused.shape[2:], ratio)[0]):
        raise ValueError(f"consistency_refine: fused {tuple(fused.shape)} and lr_ms {tuple(lr_ms.shape)} ([B, C, H, W] and its "
                         f"degradation at ratio {ratio})")
    gains = metrics.band_gains(sensor, fused.shape[1])
    steps = tuple(float(relax) / metrics.mtf_opnorm2(g, ratio) for g in gains)
    if torch.is_tensor(fused) and fused.is_cuda:
        f = fused.float().contiguous()
        lr = lr_ms.float().contiguous()
        if out is None:
            out = f.clone() if f.data_ptr() == fused.data_ptr() else f
        elif out is not fused:
            out.copy_(f)
        if ratio not in (1, 2, 4):
            raise ValueError(f"consistency_refine: ratio={ratio} (1, 2 or 4 on the device)")
        taps, scaled = ops._mtf_taps(gains, ratio, out.device), ops._mtf_taps(gains, ratio, out.device, steps)
        low, r = torch.empty_like(lr), torch.empty_like(lr)
        for _ in range(iters):
            ops.fir_decimate(out, taps, ratio, None, low)
            ops.add(low, lr, -1.0, out=r)
            ops.fir_decimate_adjoint(r, scaled, out.shape[2:], ratio, None, out, out, -1.0, 1.0)
        return out
    f = np.array(fused.detach().numpy() if torch.is_tensor(fused) else fused, dtype=np.float64)
    lr = np.asarray(lr_ms.detach().numpy() if torch.is_tensor(lr_ms) else lr_ms, dtype=np.float64)
    step = np.asarray(steps)[:, None, None]
    for _ in range(iters):
        f = f - step * metrics.mtf_degrade_adjoint(metrics.mtf_degrade(f, gains, ratio) - lr, gains, f.shape[2:], ratio)
    return torch.from_numpy(f) if torch.is_tensor(fused) else f


@torch.no_grad()
def consistency_solve(fused, lr_ms, sensor, ratio=4, iters=8, damp=0.0, out=None):
    """Solve for Wald's consistency A(fused) = lr_ms where ``consistency_refine`` refines towards it: ``iters`` steps of conjugate
    gradients on the normal equations (CGLS) of min ||A f - lr_ms||^2 + damp ||f - fused||^2, per plane, started at ``fused``
    (definition: ``metrics.consistency_solve``).  An iteration costs one A and one A^T, as a Landweber step does, and eight of
    them leave 6 to 9 times less residual than eight Landweber steps (0.055 against 0.32 of the start on the 4 x 48 x 48
    white-noise scene of tests/test_consistency_cg_host.py).  With damp = 0 the iterates converge to the projection of ``fused``
    onto the consistent scenes; damp > 0 keeps the result near ``fused`` at the price of a residual that settles above zero.
    Arguments and checks are ``consistency_refine``'s, with ``damp`` >= 0 in place of ``relax``.  Tensors on the GPU go through
    ``ops.consistency_solve`` (nothing is read back; the tap table is cached on first use: call once before capturing); host
    tensors and arrays go through the float64 definition.  ``out`` (device): receives the result and may be ``fused``."""
    from . import metrics
    if not float(damp) >= 0.0 or int(iters) != iters or iters < 0:
        raise ValueError(f"consistency_solve: damp={damp} iters={iters} (damp >= 0, iters a whole number >= 0)")
    if len(fused.shape) != 4 or tuple(lr_ms.shape) != (*fused.shape[:2], *metrics.fir_decimate_shape(*fused.shape[2:], ratio)[0]):
        raise ValueError(f"consistency_solve: fused {tuple(fused.shape)} and lr_ms {tuple(lr_ms.shape)} ([B, C, H, W] and its "
                         f"degradation at ratio {ratio})")
    gains = metrics.band_gains(sensor, fused.shape[1])
    if torch.is_tensor(fused) and fused.is_cuda:
        if ratio not in (1, 2, 4):
            raise ValueError(f"consistency_solve: ratio={ratio} (1, 2 or 4 on the device)")
        f = fused.detach().float().contiguous()
        if out is None:
            out = torch.empty_like(f)
        return ops.consistency_solve(f, lr_ms.detach().float().contiguous(), ops._mtf_taps(gains, ratio, f.device), ratio, iters,
                                     damp, out=out)
    f = metrics.consistency_solve(fused, lr_ms, gains, ratio, iters, damp)
    return torch.from_numpy(f) if torch.is_tensor(fused) else f


def _structure_checks(name, step, iters, win):
    import numbers

    def whole(v):
        return isinstance(v, numbers.Real) and not isinstance(v, bool) and float(v) == int(v)
    if not (isinstance(step, numbers.Real) and not isinstance(step, bool) and 0.0 <= float(step) < float("inf")):
        raise ValueError(f"{name}: step={step!r} (a finite number >= 0; it has no default)")
    if not (whole(iters) and iters >= 0):
        raise ValueError(f"{name}: iters={iters!r} (a whole number >= 0)")
    if not (whole(win) and 2 <= win <= 8):
        raise ValueError(f"{name}: win={win!r} (a whole number with 2 <= win <= 8)")


@torch.no_grad()
def structure_refine(fused, pan, step, iters=4, win=4, rho_max=None, lr_ms=None, sensor=None, ratio=4, relax=1.0, out=None):
    """Pull a fused scene towards the PAN's spatial structure: ``iters`` gradient steps on the local PAN-correlation loss
    L(f) = mean max(0, rho_max_c - rho) of ``metrics.local_corr_loss`` (win x win windows; ``rho_max``: None (1.0), a number or one
    per band),
      f <- f - step * N * grad L(f),        N = B C (H - win + 1)(W - win + 1), the window count of the batch.
    ``step`` multiplies the gradient of the window SUM N L, not of the mean, so a given step moves a pixel as far in a large
    scene as in a small one; it has no default, because the right size depends on the data's scale (on a 48 x 48 scene of smoothed noise in
    [0, 1] with a noisy PAN, step = 1e-3 lowers the loss from 0.576 to 0.243 in four steps, each below the one before:
    tests/test_local_corr_host.py; rho does not change when the band is scaled by s, so the gradient scales by 1 / s and a
    comparable step by s^2).  fused [B, C, H, W], pan [B, 1, H, W].  When ``lr_ms`` is given, each of these steps is followed
    by one Landweber step of ``consistency_refine(f, lr_ms, sensor, ratio, iters=1, relax=relax)``, so the spectral consistency
    the structure step disturbs is restored as it goes; ``sensor`` is then required.  Tensors on the GPU go through the
    operators (``ops.local_corr_loss`` with weight = step * N, then ``ops.add``): nothing is read back, and the loop can be captured
    after a first call (the rho_max table and the tap tables are cached on first use).  Host tensors and arrays go through the
    float64 definitions.  ``out`` (device): receives the result and may be ``fused``; otherwise ``fused`` is left as it is."""
    from . import metrics
    _structure_checks("structure_refine", step, iters, win)
    if len(fused.shape) != 4 or len(pan.shape) != 4 or tuple(pan.shape) != (fused.shape[0], 1, *fused.shape[2:]):
        raise ValueError(f"structure_refine: fused {tuple(fused.shape)} and pan {tuple(pan.shape)} ([B, C, H, W] and [B, 1, H, W])")
    if fused.shape[2] < win or fused.shape[3] < win:
        raise ValueError(f"structure_refine: a {win} x {win} window on a {fused.shape[2]} x {fused.shape[3]} scene")
    if lr_ms is not None and sensor is None:
        raise ValueError("structure_refine(lr_ms=...) needs the sensor whose MTF gains shape the degradation")
    iters, win = int(iters), int(win)
    b, c, h, w = fused.shape
    scale = float(step) * (b * c * (h - win + 1) * (w - win + 1))
    if torch.is_tensor(fused) and fused.is_cuda:
        f = fused.detach().float().contiguous()
        p = pan.detach().float().contiguous()
        if out is None:
            out = f.clone() if f.data_ptr() == fused.data_ptr() else f
        elif out is not fused:
            out.copy_(f)
        g = torch.empty_like(out)
        for _ in range(iters):
            ops.local_corr_loss(out, p, win, rho_max, scale, grad=g)
            ops.add(out, g, -1.0, out=out)
            if lr_ms is not None:
                consistency_refine(out, lr_ms, sensor, ratio, 1, relax, out=out)
        return out
    f = np.array(fused.detach().numpy() if torch.is_tensor(fused) else fused, dtype=np.float64)
    p = np.asarray(pan.detach().numpy() if torch.is_tensor(pan) else pan, dtype=np.float64)
    for _ in range(iters):
        f = f - metrics.local_corr_loss(f, p, win, rho_max, scale)[2]
        if lr_ms is not None:
            f = consistency_refine(f, lr_ms, sensor, ratio, 1, relax)
    return torch.from_numpy(f) if torch.is_tensor(fused) else f


def _structure_options(name, structure):
    """The ``structure`` option of ``fuse_scene``, checked: None, or the keyword arguments of ``structure_refine``."""
    if structure is None:
        return None
    keys = {"step", "iters", "win", "rho_max"}
    if not isinstance(structure, dict) or set(structure) - keys or "step" not in structure:
        raise ValueError(f"{name}: structure={structure!r} (None or a dict with 'step' and optionally 'iters', 'win', 'rho_max')")
    _structure_checks(f"{name}(structure=...)", structure["step"], structure.get("iters", 4), structure.get("win", 4))
    return dict(structure)


def _consistency_options(name, consistency, in_loop_allowed=False):
    """The ``consistency`` option of the fuse functions, checked: None, or (method, keyword arguments of the post-hoc call or None
    when it is switched off, options of the in-loop projection or None).  "method" is "landweber" (the default: ``consistency_refine``
    with "iters" and "relax") or "cg" (``consistency_solve`` with "iters" and "damp"; in ``fuse_scene`` also "in_loop" and
    "iters_post")."""
    if consistency is None:
        return None
    keys = {"method", "iters", "relax", "damp"} | ({"in_loop", "iters_post"} if in_loop_allowed else set())
    if not isinstance(consistency, dict) or set(consistency) - keys:
        raise ValueError(f"{name}: consistency={consistency!r} (None or a dict with 'iters' and 'relax', or with 'method': 'cg', "
                         f"'iters' and 'damp'{', in_loop and iters_post' if in_loop_allowed else ''})")
    method = consistency.get("method", "landweber")
    if method not in ("landweber", "cg"):
        raise ValueError(f"{name}: consistency method {method!r} ('landweber' or 'cg')")
    refused = {"landweber": ("damp", "in_loop", "iters_post"), "cg": ("relax",)}[method]
    if any(k in consistency for k in refused):
        raise ValueError(f"{name}: consistency={consistency!r}: method {method!r} does not take {' / '.join(repr(k) for k in refused)}")
    if method == "landweber":
        return method, {k: consistency[k] for k in ("iters", "relax") if k in consistency}, None
    post = {k: consistency[k] for k in ("iters", "damp") if k in consistency}
    loop = None
    if consistency.get("in_loop"):
        loop = dict(post)
        if "iters_post" in consistency:
            post["iters"] = consistency["iters_post"]
    elif "iters_post" in consistency:
        raise ValueError(f"{name}: consistency 'iters_post' goes with 'in_loop': True")
    for opts in (post, loop or {}):
        if "iters" in opts and (int(opts["iters"]) != opts["iters"] or opts["iters"] < 0) or not float(opts.get("damp", 0.0)) >= 0.0:
            raise ValueError(f"{name}: consistency={consistency!r} (iters whole numbers >= 0, damp >= 0)")
    return method, (None if loop is not None and post.get("iters", 8) == 0 else post), loop


def _apply_consistency(options, scene, lr_ms, sensor, ratio, **kw):
    method, post, _ = options
    if post is None:
        return scene
    return (consistency_refine if method == "landweber" else consistency_solve)(scene, lr_ms, sensor, ratio, **post, **kw)


@torch.no_grad()
def fuse_scene(diffusion, lr_ms, pan, prompt, ratio=4, score=False, interp="bilinear", sensor=None, consistency=None,
               structure=None, **sample_tiled_kwargs):
    """From the raw pair to the fused scene: lr_ms [B, C, h, w] is upsampled by ``ratio`` (2 or 4) on the device into the ``MS``
    the network is conditioned on -- ``interp="bilinear"``: ``ops.upsample_bilinear``, the reference's cv2.resize(INTER_LINEAR);
    ``interp="poly23"``: ``ops.upsample_poly23``, the interpolator that made the ``lms`` of the PanCollection files, for any
    checkpoint trained on them -- and ``sample_tiled`` fuses {"MS", "PAN"} with pan [B, 1, ratio * h, ratio * w]; the other
    keyword arguments are ``sample_tiled``'s.
    ``score=True`` returns (scene, ``metrics.quality_fullres(lr_ms, pan, scene)``): D_lambda, D_s and QNR, which takes ratio 4
    (the low-resolution PAN is two pyramid levels of pan).
    ``score="hqnr"`` returns (scene, ``metrics.quality_hqnr(ms_exp, pan, scene, sensor, ratio)``): Khan's D_lambda, the block-wise
    D_s and HQNR, the set the PanCollection tables report.  ms_exp is ``ops.upsample_poly23(lr_ms, ratio)`` whatever ``interp``
    is (the conditioning ``MS`` itself with "poly23"); ``sensor`` names the row of ``metrics.MTF_GAINS`` and is required.
    ``consistency={"iters": n, "relax": w}`` (either key optional) refines the stitched scene with ``consistency_refine`` against
    lr_ms before it is returned or scored, and needs ``sensor``; ``None`` changes nothing.  The refinement lowers the residual
    A(scene) - lr_ms, fast in its smooth part and slowly in the rest (see ``consistency_refine``); it does not solve for it.
    ``consistency={"method": "cg", "iters": n, "damp": w}`` solves for it instead, with ``consistency_solve``; "method" defaults
    to "landweber", the path above, which refuses "damp" as "cg" refuses "relax".  With "cg", ``"in_loop": True`` also hands the
    raw lr_ms to the sampler, which then projects every data prediction of the DPM-Solver run onto A f = lr_ms
    (``GeneralDiffusion.sample_by_dpmsolver``) with the same "iters" and "damp"; that needs the fused tile mode (``overlap=k``) and
    raises ValueError in the independent one.  The post-hoc solve still runs, with "iters_post" iterations when that key is
    given, unless "iters_post" is 0.
    ``structure={"step": s, "iters": n, "win": w, "rho_max": r}`` ("step" required, the others optional) runs ``structure_refine``
    on the stitched scene against pan -- before the post-hoc ``consistency`` option and before scoring -- and hands it lr_ms and
    ``sensor`` when ``sensor`` is given, so that each structure step is followed by one Landweber step; ``None`` changes nothing."""
    if score not in (False, True, "hqnr"):
        raise ValueError(f"fuse_scene: score={score!r} (False, True or 'hqnr')")
    structure = _structure_options("fuse_scene", structure)
    if consistency is not None and sensor is None:
        raise ValueError("fuse_scene(consistency=...) needs the sensor whose MTF gains shape the degradation")
    options = _consistency_options("fuse_scene", consistency, in_loop_allowed=True)
    if options is not None and options[2] is not None and sample_tiled_kwargs.get("overlap") is None:
        raise ValueError(_IN_LOOP_NEEDS_FUSED)          # sample_tiled's refusal, before any device work is done
    if isinstance(score, str) and sensor is None:
        raise ValueError("fuse_scene(score='hqnr') needs the sensor whose MTF gains shape the filters")
    if interp not in ("bilinear", "poly23"):
        raise ValueError(f"fuse_scene: interp={interp!r} ('bilinear' or 'poly23')")
    if lr_ms.dim() != 4 or pan.dim() != 4 or pan.shape[0] != lr_ms.shape[0] or pan.shape[1] != 1 or \
            tuple(pan.shape[2:]) != (ratio * lr_ms.shape[2], ratio * lr_ms.shape[3]):
        raise ValueError(f"fuse_scene: pan {tuple(pan.shape)} is not [B, 1, {ratio} h, {ratio} w] of lr_ms {tuple(lr_ms.shape)}")
    lr_ms, pan = lr_ms.float().contiguous(), pan.float().contiguous()
    ms = ops.upsample_poly23(lr_ms, ratio) if interp == "poly23" else ops.upsample_bilinear(lr_ms, ratio)
    if options is not None and options[2] is not None:
        sample_tiled_kwargs = dict(sample_tiled_kwargs, consistency={"lr_ms": lr_ms, "sensor": sensor, "ratio": ratio, **options[2]})
    scene = sample_tiled(diffusion, {"MS": ms, "PAN": pan}, prompt, **sample_tiled_kwargs)
    if structure is not None:
        scene = structure_refine(scene, pan, lr_ms=lr_ms if sensor is not None else None, sensor=sensor, ratio=ratio, **structure)
    if options is not None:
        scene = _apply_consistency(options, scene, lr_ms, sensor, ratio)
    if not score:
        return scene
    from . import metrics
    if isinstance(score, str):
        ms_exp = ms if interp == "poly23" else ops.upsample_poly23(lr_ms, ratio)
        return scene, metrics.quality_hqnr(ms_exp, pan, scene.float().contiguous(), sensor, ratio)
    return scene, metrics.quality_fullres(lr_ms, pan, scene.float().contiguous())


@torch.no_grad()
def _classical(name, on_device, on_host, lr_ms, pan, sensor, ratio, score, consistency):
    """The body ``classical_fuse`` and ``cs_fuse`` share: the checks, the interpolation, the fusion ``on_device(ms_exp, pan)`` or
    ``on_host(ms_exp, pan)``, ``consistency_refine`` and the scores."""
    from . import metrics
    if score not in (False, True, "hqnr"):
        raise ValueError(f"{name}: score={score!r} (False, True or 'hqnr')")
    options = _consistency_options(name, consistency)
    if (consistency is not None or isinstance(score, str)) and sensor is None:
        raise ValueError(f"{name}: consistency=... and score='hqnr' need the sensor whose MTF gains shape the filters")
    if ratio not in (2, 4) or len(lr_ms.shape) != 4 or len(pan.shape) != 4 or pan.shape[0] != lr_ms.shape[0] or pan.shape[1] != 1 or \
            tuple(pan.shape[2:]) != (ratio * lr_ms.shape[2], ratio * lr_ms.shape[3]):
        raise ValueError(f"{name}: pan {tuple(pan.shape)} is not [B, 1, {ratio} h, {ratio} w] of lr_ms {tuple(lr_ms.shape)} "
                         f"(ratio 2 or 4)")
    if torch.is_tensor(lr_ms) and lr_ms.is_cuda:
        lr_ms, pan = lr_ms.detach().float().contiguous(), pan.detach().float().contiguous()
        ms_exp = ops.upsample_poly23(lr_ms, ratio)
        scene = on_device(ms_exp, pan, lr_ms)
        if options is not None:
            scene = _apply_consistency(options, scene, lr_ms, sensor, ratio, out=scene)
        if not score:
            return scene
        if isinstance(score, str):
            return scene, metrics.quality_hqnr(ms_exp, pan, scene, sensor, ratio)
        return scene, metrics.quality_fullres(lr_ms, pan, scene)
    if score:
        raise ValueError(f"{name}: scores are made on the GPU; score host data with the host functions of metrics")
    scene = on_host(metrics.upsample_poly23(lr_ms, ratio), pan, lr_ms)
    if options is not None:
        scene = _apply_consistency(options, scene, lr_ms, sensor, ratio)
    return torch.from_numpy(scene) if torch.is_tensor(lr_ms) and not torch.is_tensor(scene) else scene


@torch.no_grad()
def classical_fuse(lr_ms, pan, sensor, ratio=4, mode="hpm", score=False, consistency=None):
    """From the raw pair to a classical fused scene, the MTF-GLP row of the tables: lr_ms [B, C, h, w] is interpolated with the
    23-tap polynomial kernel into ms_exp and fused with pan [B, 1, ratio * h, ratio * w] by ``mtf_glp`` in ``mode`` ("glp",
    "cbd" or "hpm"; definition: ``metrics.mtf_glp``).  ``sensor`` names the row of ``metrics.MTF_GAINS`` (or is a pair of
    explicit gains).  Tensors on the GPU go through the operators (``ops.upsample_poly23``, ``ops.mtf_glp``); host tensors and
    arrays go through the float64 definitions.  ``score`` and ``consistency`` mean what they mean in ``fuse_scene``:
    ``score=True`` returns (scene, ``metrics.quality_fullres(lr_ms, pan, scene)``), ``score="hqnr"`` returns (scene,
    ``metrics.quality_hqnr(ms_exp, pan, scene, sensor, ratio)``) with the ms_exp that was already made, and
    ``consistency={"iters": n, "relax": w}`` refines the scene with ``consistency_refine`` against lr_ms first
    (``{"method": "cg", "iters": n, "damp": w}``: solves with ``consistency_solve``).  Scores exist on
    the device only (ValueError for host data).  Not differentiable.  The component-substitution methods are ``cs_fuse``."""
    from . import metrics
    if score not in (False, True, "hqnr"):
        raise ValueError(f"classical_fuse: score={score!r} (False, True or 'hqnr')")
    if mode not in metrics.GLP_MODES:
        raise ValueError(f"classical_fuse: mode={mode!r} (one of {metrics.GLP_MODES})")
    return _classical("classical_fuse", lambda ms_exp, p, lr: ops.mtf_glp(ms_exp, p, sensor, ratio, mode),
                      lambda ms_exp, p, lr: metrics.mtf_glp(ms_exp, p, sensor, ratio, mode), lr_ms, pan, sensor, ratio, score,
                      consistency)


@torch.no_grad()
def cs_fuse(lr_ms, pan, sensor=None, ratio=4, method="gsa", score=False, consistency=None):
    """The sibling of ``classical_fuse`` for the component-substitution row of the tables: lr_ms [B, C, h, w] is interpolated
    with the 23-tap polynomial kernel into ms_exp and fused with pan [B, 1, ratio * h, ratio * w] by ``cs_fuse`` with ``method``
    "gs", "gsa" or "brovey" (definition: ``metrics.cs_fuse``); "gsa" takes lr_ms itself as its reduced-scale MS.  ``sensor`` is
    needed by "gsa", by ``consistency`` and by ``score="hqnr"``.  Device tensors go through ``ops.cs_fuse``, host tensors and
    arrays through the float64 definition; ``score`` and ``consistency`` are ``classical_fuse``'s.  Not differentiable."""
    from . import metrics
    if score not in (False, True, "hqnr"):
        raise ValueError(f"cs_fuse: score={score!r} (False, True or 'hqnr')")
    if method not in metrics.CS_METHODS:
        raise ValueError(f"cs_fuse: method={method!r} (one of {metrics.CS_METHODS})")
    if method == "gsa" and sensor is None:
        raise ValueError("cs_fuse: method 'gsa' needs the sensor whose PAN gain shapes the reduced-scale PAN")
    return _classical("cs_fuse", lambda ms_exp, p, lr: ops.cs_fuse(ms_exp, p, sensor, ratio, method, lr_ms=lr),
                      lambda ms_exp, p, lr: metrics.cs_fuse(ms_exp, p, sensor, ratio, method, lr_ms=lr), lr_ms, pan, sensor, ratio,
                      score, consistency)


@torch.no_grad()
def bdsd_fuse(lr_ms, pan, sensor, ratio=4, block=None, score=False, consistency=None):
    """The sibling of ``cs_fuse`` for the BDSD row of the tables: lr_ms [B, C, h, w] is interpolated with the 23-tap polynomial
    kernel into ms_exp and fused with pan [B, 1, ratio * h, ratio * w] by ``bdsd`` (definition: ``metrics.bdsd``), which takes lr_ms
    itself as its reduced-scale MS.  ``block``: the full-scale side of the blocks that get weights of their own (a multiple of
    ``ratio`` that divides both extents), None for one set of weights per image.  ``sensor`` is always needed: its gains shape the
    reduced scale.  Device tensors go through ``ops.bdsd``, host tensors and arrays through the float64 definition; ``score`` and
    ``consistency`` are ``classical_fuse``'s.  Not differentiable."""
    from . import metrics
    if score not in (False, True, "hqnr"):
        raise ValueError(f"bdsd_fuse: score={score!r} (False, True or 'hqnr')")
    if sensor is None:
        raise ValueError("bdsd_fuse: needs the sensor whose MTF gains shape the reduced-scale images")
    return _classical("bdsd_fuse", lambda ms_exp, p, lr: ops.bdsd(ms_exp, p, sensor, ratio, block, lr_ms=lr),
                      lambda ms_exp, p, lr: metrics.bdsd(ms_exp, p, sensor, ratio, block, lr_ms=lr), lr_ms, pan, sensor, ratio, score,
                      consistency)


def tv_regress_weights(lr_ms, pan, sensor, ratio=4):
    """The weights ``tv_fuse(weights="regress")`` gives the PAN term: float64 [B, C + 1], per image the least-squares fit of
    ``metrics.mtf_degrade(pan, PAN gain of sensor, ratio)`` by the C bands of lr_ms and a constant (the band weights, then the
    offset).  A float64 solve on the host: device tensors are copied there first, which synchronises."""
    from . import metrics
    host = lambda t: np.asarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t, dtype=np.float64)
    lr = host(lr_ms)
    b, c = lr.shape[:2]
    low = metrics.mtf_degrade(host(pan), metrics.mtf_gains(sensor, c)[1], ratio)
    rows = [np.linalg.lstsq(np.concatenate([lr[i].reshape(c, -1), np.ones((1, lr[i][0].size))]).T, low[i].reshape(-1), rcond=None)[0]
            for i in range(b)]
    return np.stack(rows)


@torch.no_grad()
def tv_fuse(lr_ms, pan, sensor, ratio=4, iters=100, lam=1e-3, gamma=1.0, weights="equal", score=False, consistency=None):
    """The sibling of ``bdsd_fuse`` for the variational row of the tables: TV pansharpening of lr_ms [B, C, h, w] with pan
    [B, 1, ratio * h, ratio * w] (definition: ``metrics.tv_pansharpen``): ``iters`` primal-dual iterations on
    1/2 ||A x - lr_ms||^2 + gamma/2 ||sum_c w_c x_c + w_C - pan||^2 + lam TV(x), started from the 23-tap interpolation of lr_ms.
    ``weights``: "equal" (1 / C per band, offset 0), "regress" (``tv_regress_weights``: a host solve per image, which
    synchronises), or an explicit [C + 1] or [B, C + 1] array.  ``lam`` = 1e-3 for data in [0, 1] is an untuned default.
    ``sensor`` is always needed: its gains shape A (a row of ``metrics.MTF_GAINS`` or a pair of explicit gains).  Device tensors go through ``ops.tv_pansharpen``, host tensors and arrays
    through the float64 definition; ``score`` and ``consistency`` are ``classical_fuse``'s.  Not differentiable."""
    from . import metrics
    if score not in (False, True, "hqnr"):
        raise ValueError(f"tv_fuse: score={score!r} (False, True or 'hqnr')")
    if sensor is None:
        raise ValueError("tv_fuse: needs the sensor whose MTF gains shape the degradation")
    if isinstance(weights, str) and weights not in ("equal", "regress"):
        raise ValueError(f"tv_fuse: weights={weights!r} ('equal', 'regress' or an explicit [C + 1] or [B, C + 1] array)")

    def table(lr, p):
        if isinstance(weights, str):
            return None if weights == "equal" else tv_regress_weights(lr, p, sensor, ratio)
        return weights
    gains = lambda lr: metrics.mtf_gains(sensor, lr.shape[1])[0]
    return _classical("tv_fuse", lambda ms_exp, p, lr: ops.tv_pansharpen(lr, p, gains(lr), ratio, iters, lam, gamma, table(lr, p), x0=ms_exp),
                      lambda ms_exp, p, lr: metrics.tv_pansharpen(lr, p, gains(lr), ratio, iters, lam, gamma, table(lr, p), x0=ms_exp),
                      lr_ms, pan, sensor, ratio, score, consistency)


@torch.no_grad()
def awlp_fuse(lr_ms, pan, sensor=None, ratio=4, mode="awlp", score=False, consistency=None):
    """The sibling of ``cs_fuse`` for the wavelet rows of the tables: lr_ms [B, C, h, w] is interpolated with the 23-tap polynomial
    kernel into ms_exp and fused with pan [B, 1, ratio * h, ratio * w] by a-trous wavelet pansharpening in ``mode`` "atwt"
    (additive) or "awlp" (proportional; definition: ``metrics.awlp``).  The method itself involves no sensor: ``sensor`` is needed
    only by ``consistency`` and by ``score="hqnr"``.  Device tensors go through ``ops.awlp``, host tensors and arrays through the
    float64 definition; ``score`` and ``consistency`` are ``classical_fuse``'s.  Not differentiable."""
    from . import metrics
    if score not in (False, True, "hqnr"):
        raise ValueError(f"awlp_fuse: score={score!r} (False, True or 'hqnr')")
    if mode not in metrics.ATROUS_MODES:
        raise ValueError(f"awlp_fuse: mode={mode!r} (one of {metrics.ATROUS_MODES})")
    return _classical("awlp_fuse", lambda ms_exp, p, lr: ops.awlp(ms_exp, p, ratio, mode),
                      lambda ms_exp, p, lr: metrics.awlp(ms_exp, p, ratio, mode), lr_ms, pan, sensor, ratio, score, consistency)
