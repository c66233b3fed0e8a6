"""GeneralDiffusion on MI355X: the reference's diffusion-process API over HIP kernels.

API mirror of the reference's GeneralModel/diffusion_general.py (class ``GeneralDiffusion`` :66-400;
``GaussianDiffusion`` is provided as an alias because BASELINE's north star uses that name).
Schedule tables are built on the host in float64 NumPy exactly as the reference does (:29-63,
:86-132) and registered as the same twelve fp32 buffers, so checkpoints interchange.  What runs on
the GPU per reverse step is the UNet (``denoise_fn``) plus ONE fused elementwise kernel
(``tmdiff_ddpm_step``: predict_start_from_noise :376-378 -> clamp :192-194 -> q_posterior :134-138
-> + sigma*noise :208 -> res2img); the step-invariant half of the UNet is evaluated once per
sampling run (``WavBEST.begin_condition_cache``).

Behaviour kept from the reference on purpose: ``super_resolution(x_in, continous,
prompt, guidance)`` forwards ``prompt`` into ``p_sample_loop``'s ``continous`` slot, so it always
samples with prompt "QB" and returns the whole stack; the network output is used as *noise* during
sampling although training fits x_0.  ``sample(...)`` is the clean entry point beside it.

``noise_fn(like) -> Tensor`` is a hook for parity runs (CPU-drawn noise moved to the device);
throughput runs use the device generator.
"""
import math

import numpy as np
import torch
from torch import nn

from . import losses, ops, sample_graph
from .dpm_solver import DPM_Solver, NoiseScheduleVP, model_wrapper
from .util import res2img  # noqa: F401  (re-exported like the reference module does)


def make_beta_schedule(schedule, n_timestep):
    if schedule == "linear":
        scale = 1000 / n_timestep
        return np.linspace(scale * 1e-6, scale * 1e-2, n_timestep, dtype=np.float64)
    if schedule == "cosine":
        return betas_for_alpha_bar(n_timestep, lambda t: math.cos((t + 0.008) / 1.008 * math.pi / 2) ** 2)
    raise NotImplementedError(schedule)


def betas_for_alpha_bar(num_diffusion_timesteps, alpha_bar, max_beta=0.999):
    n = num_diffusion_timesteps
    return np.array([min(1 - alpha_bar((i + 1) / n) / alpha_bar(i / n), max_beta) for i in range(n)])


class GeneralDiffusion(nn.Module):
    sample_graphs = None           # captured-graph sampling for this object: True / False, None = ops.config.sample_graph
    sample_graph_capacity = 2      # captured samplers kept per object (least recently used dropped first)
    sample_graph_captures = 0      # samplers captured so far by this object

    def __init__(self, denoise_fn, loss_type="l1", noise_fn=None, loss_terms=None):
        """``loss_terms`` (ours, optional): ``{"sam": w, "lap": w, "dssim": w}`` adds a spectral-angle, a Laplacian and / or an
        SSIM (1 - SSIM) term to ``loss_type`` (tmdiff_amd.losses); None or {} keeps the reference's torch loss modules."""
        super().__init__()
        self.denoise_fn = denoise_fn
        self.loss_type = loss_type
        self.noise_fn = noise_fn
        self.loss_terms = dict(loss_terms) if loss_terms else None
        if self.loss_terms is not None:
            losses.parse_loss_terms(self.loss_terms)       # ValueError for an unknown key or a negative weight

    # ---- configuration ------------------------------------------------------------------------------
    def set_loss(self, device):
        if self.loss_terms is not None:
            if self.loss_type not in losses.BASE_KINDS:
                raise NotImplementedError()
            w_sam, w_lap = losses.parse_loss_terms(self.loss_terms)
            self.loss_func = losses.SpectralSpatialLoss(self.loss_type, w_sam, w_lap, losses.dssim_weight(self.loss_terms)).to(device)
        elif self.loss_type == "l1":
            self.loss_func = nn.L1Loss().to(device)
        elif self.loss_type == "l2":
            self.loss_func = nn.MSELoss().to(device)
        elif self.loss_type == "smooth_l1":
            self.loss_func = nn.SmoothL1Loss().to(device)
        else:
            raise NotImplementedError()

    def set_new_noise_schedule(self, schedule_opt, device):
        betas = make_beta_schedule(schedule=schedule_opt["schedule"], n_timestep=schedule_opt["n_timestep"])
        alphas = 1.0 - betas
        ac = np.cumprod(alphas, axis=0)
        ac_prev = np.append(1.0, ac[:-1])
        self.sqrt_alphas_cumprod_prev = np.sqrt(np.append(1.0, ac))
        self.num_timesteps = int(betas.shape[0])
        with np.errstate(divide="ignore"):
            recip, recipm1 = np.sqrt(1.0 / ac), np.sqrt(1.0 / ac - 1)
        self.sqrt_recip_alphas_cumprod, self.sqrt_recipm1_alphas_cumprod = recip, recipm1
        post_var = betas * (1.0 - ac_prev) / (1.0 - ac)
        tables = {
            "betas": betas, "alphas_cumprod": ac, "alphas_cumprod_prev": ac_prev,
            "sqrt_alphas_cumprod": np.sqrt(ac), "sqrt_one_minus_alphas_cumprod": np.sqrt(1.0 - ac),
            "log_one_minus_alphas_cumprod": np.log(1.0 - ac),
            "sqrt_recip_alphas_cumprod_1": recip, "sqrt_recipm1_alphas_cumprod_1": recipm1,
            "posterior_variance": post_var,
            "posterior_log_variance_clipped": np.log(np.maximum(post_var, 1e-20)),
            "posterior_mean_coef1": betas * np.sqrt(ac_prev) / (1.0 - ac),
            "posterior_mean_coef2": (1.0 - ac_prev) * np.sqrt(alphas) / (1.0 - ac),
        }
        host = {}
        for name, arr in tables.items():
            t32 = torch.tensor(arr, dtype=torch.float32)
            host[name] = t32
            self.register_buffer(name, t32.to(device))
        # host-side fp32 copies of what a reverse step reads: no device->host sync inside the loop
        sigma = (0.5 * host["posterior_log_variance_clipped"]).exp()
        self._step_coef = [tuple(float(host[k][i]) for k in ("sqrt_recip_alphas_cumprod_1", "sqrt_recipm1_alphas_cumprod_1",
                                                             "posterior_mean_coef1", "posterior_mean_coef2"))
                           + (float(sigma[i]),) for i in range(self.num_timesteps)]

    # ---- small helpers ----------------------------------------------------------------------------------
    @staticmethod
    def _to_device(t, device):
        """Host -> device without stalling the host: a pageable-memory copy waits for the stream to drain (13 ms per
        training step when it sat in q_sample); pinned + non_blocking just enqueues."""
        if t.device.type == "cpu" and torch.device(device).type == "cuda":
            return t.pin_memory().to(device, non_blocking=True)
        return t.to(device)

    def _noise(self, like):
        if self.noise_fn is not None:
            return self.noise_fn(like).to(like.device).contiguous()
        return torch.randn_like(like)

    def predict_start_from_noise(self, x_t, t, noise):
        a, b = self._step_coef[t][:2]
        return ops.axpby([x_t, noise], [a, -b])

    def q_posterior(self, x_start, x_t, t):
        c1, c2 = self._step_coef[t][2:4]
        return ops.axpby([x_start, x_t], [c1, c2]), self.posterior_log_variance_clipped[t]

    def dynamic_clip(self, x_recon, is_static=True):
        if is_static:
            return x_recon.clamp_(-1.0, 1.0)
        s = torch.max(torch.abs(x_recon))
        s = s if s > 1 else 1.0
        return x_recon / s

    # ---- reverse process ----------------------------------------------------------------------------------
    @torch.no_grad()
    def p_mean_variance(self, x, t, clip_denoised=True, x_in=None, prompt="QB", guidance=1.0):
        time_in = torch.full((x.shape[0], 1), t + 1, device=x.device, dtype=torch.float32)
        eps = self.denoise_fn(x, time_in, x_in["PAN"], x_in["MS"], prompt)
        a, b, c1, c2, _ = self._step_coef[t]
        mean = ops.ddpm_step(x, eps, None, a, b, c1, c2, 0.0, clip=clip_denoised)
        return mean, self.posterior_log_variance_clipped[t]

    @torch.no_grad()
    def p_mean_variance_xo(self, x, t, clip_denoised=True, x_in=None, prompt="QB", guidance=1.0):
        """x0-parameterised twin of ``p_mean_variance`` (ref :173-190, called by nothing there): the network output is
        taken as x_0 directly, clamped, and fed to the posterior.  Same fused kernel with predict_start coefficients
        (0, -1): 0*x + 1*out is exact."""
        time_in = torch.full((x.shape[0], 1), t + 1, device=x.device, dtype=torch.float32)
        x0 = self.denoise_fn(x, time_in, x_in["PAN"], x_in["MS"], prompt)
        _, _, c1, c2, _ = self._step_coef[t]
        mean = ops.ddpm_step(x, x0, None, 0.0, -1.0, c1, c2, 0.0, clip=clip_denoised)
        return mean, self.posterior_log_variance_clipped[t]

    @torch.no_grad()
    def p_sample(self, x, t, clip_denoised=True, condition_x=None, prompt="QB", guidance=1.0, _img_out=None):
        time_in = torch.full((x.shape[0], 1), t + 1, device=x.device, dtype=torch.float32)
        eps = self.denoise_fn(x, time_in, condition_x["PAN"], condition_x["MS"], prompt)
        a, b, c1, c2, sigma = self._step_coef[t]
        noise = self._noise(x) if t > 0 else None
        return ops.ddpm_step(x, eps, noise, a, b, c1, c2, sigma if t > 0 else 0.0, clip=clip_denoised,
                             ms=condition_x["MS"] if _img_out is not None else None, img_out=_img_out)

    def _cached(self, x_in, prompt):
        """Context: evaluate the step-invariant condition branch of the UNet once for a sampling run."""
        net = self.denoise_fn
        outer = self

        class _Ctx:
            def __enter__(self):
                self.on = hasattr(net, "begin_condition_cache")
                if self.on:
                    net.begin_condition_cache(x_in["PAN"], x_in["MS"], prompt)

            def __exit__(self, *exc):
                if self.on:
                    net.end_condition_cache()
                return False

        return _Ctx()

    def release_sample_graphs(self):
        """Drop every captured sampler of this object (graphs, static buffers and what they keep alive)."""
        self.__dict__.pop("_sample_graph_cache", None)

    @torch.no_grad()
    def p_sample_loop(self, x_in, continous=False, prompt="QB", guidance=1.0):
        sample_inter = 1 | (self.num_timesteps // 10)
        x_in = self._prep_inputs(x_in)
        if sample_graph.usable(self, x_in):
            return sample_graph.ddpm(self, x_in, prompt, continous)
        img = self._noise(x_in["Res"])
        frames = [ops.add(img, x_in["MS"])]
        with self._cached(x_in, prompt):
            for i in reversed(range(self.num_timesteps)):
                keep = i % sample_inter == 0
                frame = torch.empty_like(img) if keep else None
                img = self.p_sample(img, i, condition_x=x_in, prompt=prompt, guidance=guidance, _img_out=frame)
                if keep:
                    frames.append(frame)
        return torch.cat(frames, dim=0) if continous else frames[-1][-1]

    @torch.no_grad()
    def super_resolution(self, x_in, continous, prompt, guidance):
        return self.p_sample_loop(x_in, prompt)        # the reference's positional slip, kept (ref :339)

    @torch.no_grad()
    def sample(self, x_in, prompt, return_all=False, method="ddpm", steps=None, consistency=None):
        """Clean entry point: fused image(s) for ``prompt``; method 'ddpm' (T steps) or 'dpmsolver'.  ``consistency``: the
        in-loop projection of ``sample_by_dpmsolver``; 'ddpm' refuses it (its loop treats the network output as noise inside
        the fused ``ddpm_step``)."""
        if method == "dpmsolver":
            kw = {"steps": steps} if steps else {}
            if consistency is not None:
                kw["consistency"] = consistency
            return self.sample_by_dpmsolver(x_in, prompt, **kw)
        if consistency is not None:
            raise ValueError("sample: consistency=... needs method='dpmsolver' (the DDPM loop has no data prediction to project)")
        stack = self.p_sample_loop(x_in, continous=True, prompt=prompt)
        b = x_in["Res"].shape[0]
        return stack if return_all else stack[-b:]

    @staticmethod
    def _prep_inputs(x_in):
        out = dict(x_in)
        for k in ("Res", "MS", "PAN"):
            out[k] = x_in[k].float().contiguous()
        return out

    def _dpm_schedule(self):
        return NoiseScheduleVP(schedule="discrete", betas=self.betas)

    def _solve(self, x_in, prompt, model_type, model_kwargs, steps, order, method, denoise_to_zero=True, x_T=None, ns=None,
               time_table=None, project=None, **wrap_kw):
        """x_T / ns: given by the graph runner (drawn / built outside its capture); time_table: see _WrappedModel; project:
        applied to every data prediction after dynamic thresholding (``_consistency_projection``)."""
        x_T = self._noise(x_in["Res"]) if x_T is None else x_T
        ns = self._dpm_schedule() if ns is None else ns
        model_fn = model_wrapper(self.denoise_fn, ns, model_type=model_type, model_kwargs=model_kwargs, **wrap_kw)
        model_fn.time_table = time_table
        solver = DPM_Solver(model_fn, ns, algorithm_type="dpmsolver++", correcting_x0_fn="dynamic_thresholding")
        if project is not None:
            threshold = solver.correcting_x0_fn
            solver.correcting_x0_fn = lambda x0, t=None: project(threshold(x0, t))
        x = solver.sample(x_T, steps=steps, order=order, skip_type="logSNR", method=method,
                          denoise_to_zero=denoise_to_zero)
        self.last_solver = solver
        return ops.add(x, x_in["MS"])

    @torch.no_grad()
    def sample_by_dpmsolver(self, x_in, prompt, steps=30, consistency=None):
        """ref :227-255: x_start-parameterised DPM-Solver++, singlestep order 3, logSNR grid, dynamic
        thresholding, denoise-to-zero => steps + 1 network evaluations (reference hard-codes steps=30).
        ``consistency={"lr_ms": tensor, "sensor": name, "ratio": 4, "iters": 4, "damp": 0.0}`` (the last three optional) pulls
        every data prediction, the denoise-to-zero one included, onto the known measurement, in the DDNM style: after dynamic
        thresholding the predicted scene f0 = x0 + MS gets the correction d of ``ops.consistency_solve`` against lr_ms
        ([B, C, H', W'], the extent of ``mtf_degrade`` at ``ratio``), and x0 += d.  With damp = 0 the solve converges to the
        minimum-norm correction A^+ (lr_ms - A f0), the projection onto A f = lr_ms.  Buffers are made once per run.  With
        ``consistency`` given the run is eager, also when ``sample_graph`` is on; ``None`` is the call without the argument."""
        x_in = self._prep_inputs(x_in)
        project = None if consistency is None else self._consistency_projection(x_in, consistency)
        if project is None and sample_graph.usable(self, x_in):
            return sample_graph.dpmsolver(self, x_in, prompt, steps)
        with self._cached(x_in, prompt):
            return self._solve(x_in, prompt, "x_start", {"PAN": x_in["PAN"], "MS": x_in["MS"], "prompt": prompt},
                               steps, 3, "singlestep", project=project)

    @staticmethod
    def _consistency_projection(x_in, consistency):
        """x0 -> x0 + d for the ``consistency`` options of ``sample_by_dpmsolver``, with the buffers of the run."""
        from . import metrics
        if not isinstance(consistency, dict) or "lr_ms" not in consistency or "sensor" not in consistency or \
                set(consistency) - {"lr_ms", "sensor", "ratio", "iters", "damp"}:
            raise ValueError(f"sample_by_dpmsolver: consistency needs 'lr_ms' and 'sensor' and takes 'ratio', 'iters' and 'damp', "
                             f"got {sorted(consistency) if isinstance(consistency, dict) else consistency!r}")
        ms = x_in["MS"]
        ratio, iters, damp = consistency.get("ratio", 4), consistency.get("iters", 4), consistency.get("damp", 0.0)
        if ratio not in (1, 2, 4) or int(iters) != iters or iters < 0 or not float(damp) >= 0.0:
            raise ValueError(f"sample_by_dpmsolver: consistency ratio={ratio} iters={iters} damp={damp} (ratio 1, 2 or 4, iters a "
                             f"whole number >= 0, damp >= 0)")
        b, c, h, w = ms.shape
        lr = consistency["lr_ms"]
        if not torch.is_tensor(lr) or tuple(lr.shape) != (b, c, *ops.fir_decimate_shape(h, w, ratio)) or lr.device != ms.device:
            raise ValueError(f"sample_by_dpmsolver: consistency lr_ms must be the degradation of MS {tuple(ms.shape)} at ratio "
                             f"{ratio} on {ms.device}, got {tuple(lr.shape) if torch.is_tensor(lr) else lr!r}")
        lr = lr.detach().float().contiguous()
        taps = ops._mtf_taps(metrics.band_gains(consistency["sensor"], c), ratio, ms.device)
        ws = ops.consistency_solve_workspace(b, c, h, w, ratio, iters, ms.device)
        f0, d = torch.empty_like(ms), torch.empty_like(ms)

        def project(x0):
            # x0 is changed in place, as the thresholding before it does: data_prediction_fn hands both a tensor of their own
            # (ops.x0_from_model allocates its result), never the network's output or the sampler's state
            ops.add(x0, ms, out=f0)
            ops.consistency_solve(f0, lr, taps, ratio, iters, damp, out=f0, correction_out=d, workspace=ws)
            return ops.add(x0, d, out=x0)

        return project

    # The next three exist in the reference (:257-335) but pass arguments WavBEST.forward does not take
    # (a `wav` tensor, swapped PAN/MS order), so they fail there as they do here; kept for the API surface.
    @torch.no_grad()
    def sample_by_dpmsolver_noise(self, x_in, prompt):
        kw = {"PAN": x_in["PAN"], "MS": x_in["MS"], "wav": x_in["wav"], "prompt": prompt}
        return self._solve(x_in, prompt, "noise", kw, 50, 3, "multistep")

    @torch.no_grad()
    def sample_by_regression(self, x_in, prompt):
        x_T = self._noise(x_in["Res"])
        time_in = torch.tensor([1000 + 1] * 1, device=x_T.device).view(1, -1)
        x_recon = self.denoise_fn(x_T, time_in, x_in["PAN"], x_in["MS"], x_in["wav"], prompt)
        return ops.add(x_recon, x_in["MS"])

    @torch.no_grad()
    def sample_by_dpmsolver_guidance(self, x_in, prompt, guidance):
        kw = {"MS": torch.cat([torch.zeros_like(x_in["MS"]), x_in["MS"]]), "prompt": prompt}
        return self._solve(x_in, prompt, "noise", kw, 50, 2, "multistep", denoise_to_zero=False,
                           guidance_type="classifier-free", condition=x_in["PAN"],
                           unconditional_condition=torch.zeros_like(x_in["PAN"]), guidance_scale=guidance)

    @torch.no_grad()
    def classifier_free_guidance_sample(self, x, t_input, x_in, guidance, prompt):
        cond = x_in["MS"]
        e_c = self.denoise_fn(x, t_input, cond, x_in["PAN"], prompt)
        e_u = self.denoise_fn(x, t_input, torch.zeros_like(cond), x_in["PAN"], prompt)
        return ops.axpby([e_c, e_u], [guidance + 1.0, -guidance])

    def classifier_free_guidance_train(self, cond, p_uncond):
        return cond if torch.rand(1) > p_uncond else torch.zeros_like(cond)

    def _scale_timesteps(self, t):
        if self.rescale_timesteps:      # attribute never set by the reference either (:380-383)
            return t.float() * (1000.0 / self.num_timesteps)
        return t

    # ---- forward process / training loss ------------------------------------------------------------------
    def q_sample(self, x_start, continuous_sqrt_alpha_cumprod, noise=None):
        noise = self._noise(x_start) if noise is None else noise
        a = self._to_device(continuous_sqrt_alpha_cumprod.reshape(-1).float(), x_start.device).contiguous()
        if a.numel() == 1 and x_start.shape[0] > 1:
            a = a.expand(x_start.shape[0]).contiguous()
        return ops.q_sample(x_start.contiguous(), noise.contiguous(), a)

    def draw_training_inputs(self, b):
        """The per-step random inputs of p_losses_dynamic that come from the HOST generator, as the reference draws them
        (:353-360): integer timesteps 1..T from NumPy's global RNG and their sqrt(alpha_bar) values.  Returns host tensors
        (int64 [b, 1], float32 [b]); the captured finetune step (tmdiff_amd.model) copies them into fixed device tensors."""
        time_in = np.random.randint(1, self.num_timesteps + 1, size=b)           # host RNG, as the reference (:353)
        a = torch.tensor(np.atleast_1d(self.sqrt_alphas_cumprod_prev[time_in]), dtype=torch.float32)
        return torch.from_numpy(time_in).view(b, -1), a

    def p_losses_dynamic(self, x_in, prompt=None):
        x_start = x_in["Res"].float().contiguous()
        b = x_start.shape[0]
        t_host, a_host = self.draw_training_inputs(b)
        noise = self._noise(x_start)
        return self.p_losses_with(x_in, prompt, self._to_device(t_host, x_start.device),
                                  self._to_device(a_host, x_start.device), noise)

    def p_losses_with(self, x_in, prompt, t_dev, a_dev, noise):
        """p_losses_dynamic (ref :349-370) on given timesteps t_dev [b, 1], sqrt(alpha_bar) values a_dev [b] and noise, all
        on the device: q_sample, the differentiable UNet forward, the loss.  Launches kernels only (no host sync, no host ->
        device copy), so the whole call can be recorded into a HIP graph."""
        x_start = x_in["Res"].float().contiguous()
        a = a_dev.reshape(-1).float()
        if a.numel() == 1 and x_start.shape[0] > 1:
            a = a.expand(x_start.shape[0])
        x_noisy = ops.q_sample(x_start, noise.contiguous(), a.contiguous())
        ms = x_in["MS"].float().contiguous()
        x_recon = self.denoise_fn.forward_train(x_noisy, t_dev.view(x_start.shape[0], -1), x_in["PAN"].float().contiguous(),
                                                ms, prompt)
        if self.loss_terms is not None:                  # the composite loss scores the images x_start + MS, x_recon + MS
            return self.loss_func(x_start, x_recon, ms)
        return self.loss_func(x_start, x_recon)

    def forward(self, x, *args, **kwargs):
        return self.p_losses_dynamic(x, *args, **kwargs)


GaussianDiffusion = GeneralDiffusion
