"""AdamW of the finetune step as ONE HIP launch (tmdiff_multi_adamw).

``FusedAdamW`` IS a ``torch.optim.AdamW`` (reference GeneralModel/model.py:30-31: ``AdamW(optim_params, lr, weight_decay=1e-4)``):
same constructor arguments, same ``param_groups`` / ``state`` layout (``step``, ``exp_avg``, ``exp_avg_sq`` per parameter), so
``state_dict()`` / ``load_state_dict()`` and the ``I{iter}_opt.pth`` files interchange with the reference's optimizer and LR
schedulers drive it unchanged.  Only ``step()`` differs: every parameter that has a gradient is updated by one multi-tensor kernel
that reads the learning rate and the step count from device scalars -- no host read anywhere, so the step can be recorded into a
HIP graph (torch's capturable AdamW does the same update in ~25 multi-tensor / elementwise launches: 3 ms per step of WavBEST's
272 tensors against 0.15 ms).  amsgrad / maximize / fp16 parameters are not supported (the reference uses none of them).

``max_grad_norm`` clips the global gradient norm inside that step (``torch.nn.utils.clip_grad_norm_``): one read pass over the
gradients for the norm (tmdiff_multi_sqnorm_partial / _finish), then an AdamW launch that multiplies each gradient by the clip
coefficient in registers (tmdiff_multi_adamw_scaled) -- the gradients are never rewritten and nothing is read on the host.  With
``skip_nonfinite`` a step whose norm is inf / NaN changes nothing at all, the step counters included."""
import ctypes as C

import torch

from . import ops
from ._lib import check, lib


class FusedAdamW(torch.optim.AdamW):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=None, skip_nonfinite=True,
                 **kw):
        for bad in ("amsgrad", "maximize"):
            if kw.get(bad):
                raise ValueError(f"FusedAdamW: {bad} is not supported")
        if max_grad_norm is not None and not (float(max_grad_norm) > 0.0):          # (a NaN fails the comparison too)
            raise ValueError(f"FusedAdamW: max_grad_norm must be positive, got {max_grad_norm}")
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, **kw)
        # constructor arguments, not part of state_dict()
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.last_grad_norm = None   # device scalars of the last clipped step: the norm before clipping, and 1 / 0 for
        self.last_step_ok = None     # applied / skipped (float(...) them when logging; step() never reads them)
        self.last_clip_coef = None   # ... and the factor the gradients were multiplied by (0 on a skipped step)
        self._clip = None            # partial sums, the scalars, group offsets (see _clip_buffers)
        self._tables = {}        # group index -> dict(key, entries, chunk_tensor, chunk_index, n_chunks, pinned host copies)
        self._lr_dev = {}        # group index -> (device scalar, last host value) when the group's lr is a Python float

    # -- state --------------------------------------------------------------------------------------------------------------
    def _group_step(self, group):
        """ONE device step counter per group, shared by the ``state[p]['step']`` entries of its parameters (torch keeps one
        scalar per parameter: 272 increments per step; shared, the counter is bumped once and every entry sees it)."""
        shared = None
        for p in group["params"]:
            st = self.state.get(p)
            if st and "step" in st and torch.is_tensor(st["step"]) and st["step"].is_cuda:
                shared = st["step"] if shared is None else shared
        return shared

    def _init_state(self, group, params):
        shared = self._group_step(group)
        if shared is None:
            # (after load_state_dict the entries are host / per-parameter scalars: continue from their value)
            t0 = max([float(self.state[p]["step"]) for p in params if self.state.get(p) and "step" in self.state[p]] or [0.0])
            shared = torch.full((), t0, dtype=torch.float32, device=params[0].device)
        for p in group["params"]:
            st = self.state[p] if p in self.state or p.grad is not None else None
            if st is None:
                continue
            st["step"] = shared
            if p.grad is not None and "exp_avg" not in st:
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return shared

    def _table(self, gi, params):
        key = tuple((p.data_ptr(), p.grad.data_ptr(), self.state[p]["exp_avg"].data_ptr(), self.state[p]["exp_avg_sq"].data_ptr(),
                     p.numel()) for p in params)
        tb = self._tables.get(gi)
        if tb is not None and tb["key"] == key:
            return tb
        # pinned host copies + non-blocking uploads (the gradients of a captured step are allocated inside the capture, so their
        # addresses -- hence this table -- are first known there); the pinned tensors stay alive with the table
        entries, chunk_tensor, chunk_index, n_chunks, host = ops.chunk_tables(key, [row[4] for row in key], params[0].device,
                                                                              pinned=True)
        tb = self._tables[gi] = {"key": key, "host": host, "entries": entries, "chunk_tensor": chunk_tensor,
                                 "chunk_index": chunk_index, "n_chunks": n_chunks}
        return tb

    def _lr_scalar(self, gi, group, dev):
        lr = group["lr"]
        if torch.is_tensor(lr):
            if not lr.is_cuda or lr.dtype != torch.float32:
                raise ValueError("FusedAdamW: a tensor learning rate must be a float32 scalar on the GPU")
            return lr
        cur = self._lr_dev.get(gi)
        if cur is None:
            cur = self._lr_dev[gi] = [torch.full((), float(lr), dtype=torch.float32, device=dev), float(lr)]
        elif cur[1] != float(lr):
            cur[0].fill_(float(lr))
            cur[1] = float(lr)
        return cur[0]

    def _clip_buffers(self, work):
        """The partial sums of every group in one buffer (group gi writes n_chunks doubles at its own offset) and the three
        scalars norm / coef / ok, kept like the tables: alive with the optimizer, hence with a graph that recorded them."""
        key = tuple((gi, tb["n_chunks"]) for gi, _, _, tb, _ in work)
        cb = self._clip
        if cb is not None and cb["key"] == key:
            return cb
        dev = work[0][2][0].device
        offsets, total = {}, 0
        for gi, n in key:
            offsets[gi] = total
            total += n
        assert lib.tmdiff_multi_sqnorm_workspace_bytes(total) == 8 * total
        cb = self._clip = {"key": key, "offsets": offsets, "total": total,
                           "partials": torch.zeros(total, dtype=torch.float64, device=dev),
                           "scalars": torch.zeros(3, dtype=torch.float32, device=dev),
                           "one": torch.ones((), dtype=torch.float32, device=dev)}
        return cb

    def state_dict(self):
        """torch's layout, with a step scalar OF ITS OWN per parameter (here they share one device counter; torch.optim.AdamW,
        which a reference-side run may load this checkpoint into, increments every entry and must not find them aliased)."""
        sd = super().state_dict()
        sd["state"] = {k: dict(v) for k, v in sd["state"].items()}       # (the packed state holds the LIVE per-parameter dicts)
        steps = {}
        for st in sd["state"].values():
            if "step" in st and torch.is_tensor(st["step"]):
                key = st["step"].data_ptr()
                if key not in steps:
                    steps[key] = float(st["step"])          # (one host read per group, at checkpoint time only)
                st["step"] = torch.tensor(steps[key], dtype=torch.float32)
        return sd

    # -- the step -------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        work = []
        for gi, group in enumerate(self.param_groups):
            params = [p for p in group["params"] if p.grad is not None]
            if not params:
                continue
            for p in params:
                if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and p.grad.is_contiguous() and
                        p.grad.dtype == torch.float32 and not p.grad.is_sparse):
                    raise RuntimeError("FusedAdamW: parameters and gradients must be dense contiguous float32 tensors on the GPU")
            step = self._init_state(group, params)
            if self.max_grad_norm is None:
                step.add_(1.0)
                self._launch(gi, group, params, step, self._table(gi, params))
            else:
                work.append((gi, group, params, self._table(gi, params), step))
        if work:
            self._clipped_step(work)
        return loss

    def _launch(self, gi, group, params, step, tb, coef=None, ok=None):
        b1, b2 = group["betas"]
        args = (tb["entries"].data_ptr(), tb["chunk_tensor"].data_ptr(), tb["chunk_index"].data_ptr(), tb["n_chunks"],
                self._lr_scalar(gi, group, params[0].device).data_ptr(), step.data_ptr(), float(b1), float(b2), float(group["eps"]),
                float(group["weight_decay"]))
        if coef is None:
            check(lib.tmdiff_multi_adamw(*args, ops.stream_ptr()), "multi_adamw")
        else:
            check(lib.tmdiff_multi_adamw_scaled(*args, coef.data_ptr(), ok.data_ptr(), ops.stream_ptr()), "multi_adamw_scaled")
        # the kernel writes the parameters through raw pointers: tell autograd's version counters, which the packed convolution
        # weights and projection banks are keyed on (ops.PackedWeights, WavBEST._prepare), as an in-place torch update would
        torch.autograd.graph.increment_version(params)

    def _clipped_step(self, work):
        """Norm over ALL groups (one stage-1 launch per group, one finish), then per group: counter += ok, scaled AdamW."""
        cb = self._clip_buffers(work)
        st = ops.stream_ptr()
        for gi, _, _, tb, _ in work:
            check(lib.tmdiff_multi_sqnorm_partial(tb["entries"].data_ptr(), tb["chunk_tensor"].data_ptr(), tb["chunk_index"].data_ptr(),
                                                  tb["n_chunks"], cb["partials"].data_ptr() + 8 * cb["offsets"][gi], st),
                  "multi_sqnorm_partial")
        norm, coef, ok = cb["scalars"][0], cb["scalars"][1], cb["scalars"][2]
        check(lib.tmdiff_multi_sqnorm_finish(cb["partials"].data_ptr(), cb["total"], self.max_grad_norm, norm.data_ptr(),
                                             coef.data_ptr(), ok.data_ptr(), st), "multi_sqnorm_finish")
        if not self.skip_nonfinite:
            # every step is taken, and a NaN norm poisons every parameter as torch's clip_grad_norm_(error_if_nonfinite=False)
            # does (the kernel's coefficient is 0 there; for an infinite norm 0 is torch's value too)
            coef, ok = torch.where(torch.isnan(norm), norm, coef), cb["one"]
        self.last_grad_norm, self.last_clip_coef, self.last_step_ok = norm, coef, ok
        for gi, group, params, tb, step in work:
            step.add_(ok)                  # (a skipped step does not advance the bias corrections)
            self._launch(gi, group, params, step, tb, coef, ok)
