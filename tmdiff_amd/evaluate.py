"""Validation pass around the sampler: what ``val_dataset`` in the reference driver does
(general_sharpening_joint_random_batch_finetune.py:126-152) -- sample every validation item, rescale to the sensor's
digital numbers, write ``output_mulExm_{idx}.mat`` with key ``sr`` (H x W x C), and average SSIM / SAM against HR.
"""
import os
import time

import numpy as np
import scipy.io as scio
import torch

from . import metrics

IMG_SCALE = {"GF2": 1023.0}          # every other sensor: 2047 (ref :134)
BASELINES = ("exp", "glp", "cbd", "hpm")   # val_dataset(baselines=...): the interpolated MS and the three modes of metrics.mtf_glp
CS_BASELINES = ("cs-gs", "cs-gsa", "cs-brovey")   # ... and "cs-" + the methods of metrics.cs_fuse (component substitution)
BDSD_BASELINES = ("bdsd", "bdsd-local")    # ... and metrics.bdsd with one set of weights per image / per 128 x 128 block
BDSD_LOCAL_BLOCK = 128
TV_BASELINES = ("tv",)                     # ... and metrics.tv_pansharpen at its defaults (100 iterations, lam 1e-3, equal weights)
ATROUS_BASELINES = ("atwt", "awlp")        # ... and metrics.awlp in its two modes (a-trous wavelet pansharpening; no sensor involved)


def to_hwc01(img, min_max=(0.0, 1.0)):
    """[1,C,H,W] or [C,H,W] tensor -> clamped, rescaled H x W x C float32 array (ref ``normlization`` :39-42)."""
    lo, hi = min_max
    data = img.detach().squeeze().float().cpu().clamp(lo, hi).numpy()
    return np.transpose((data - lo) / (hi - lo), (1, 2, 0))


def _to_nchw01(img, min_max=(0.0, 1.0)):
    """The clamp and rescale of ``to_hwc01`` on the device: [1,C,H,W] or [C,H,W] tensor -> float32 [1,C,H,W] on the GPU."""
    lo, hi = min_max
    t = img.detach().float()
    t = t if t.is_cuda else t.cuda()
    t = t.reshape(1, *t.shape[-3:])
    return ((t.clamp(lo, hi) - lo) / (hi - lo)).contiguous()


def val_dataset(trainer, dataset, val_loader, result_root, continous=False, log=print, device_metrics=False,
                full_resolution=False, q2n=False, protocol="qnr", sensor=None, baselines=(), d_rho=False):
    """``trainer`` is a ``tmdiff_amd.model.DDPM`` (or the reference's); ``dataset`` is the prompt name.
    Returns ``{"ssim_<dataset>": ..., "sam_<dataset>": ..., "sec_per_item": ...}``.

    ``device_metrics=True`` scores on the GPU instead (``ops.metrics_pair``: one pass per item over the two images, sums kept
    on the device, one synchronising read of the scores after the last item) and adds ``psnr_``, ``ergas_``, ``scc_``, ``cc_``
    and ``q_<dataset>``.  The ``.mat`` files are the same in both modes (writing them is what still brings SR to the host).

    ``full_resolution=True`` is for files without ground truth (``LRHRDataset.has_gt`` is False: ``HR`` is only ``lms`` standing
    in, and SSIM / SAM against it mean nothing).  Each item is scored without a reference on the GPU instead:
    ``ops.metrics_noref(LR, PAN, ops.pyr_down(PAN), SR)``, with the low-resolution PAN and the workspace allocated once per
    shape, sums kept on the device and one synchronising read at the end.  Returns ``{"d_lambda_<dataset>": ...,
    "d_s_<dataset>": ..., "qnr_<dataset>": ..., "sec_per_item": ...}`` and no ``ssim_`` / ``sam_`` keys; the ``.mat`` files
    are written as in the other modes.  ValueError when the visuals carry no ``LR`` or ``PAN``.

    ``q2n=True`` (with ``device_metrics=True`` only, and not with ``full_resolution=True``: ValueError otherwise) adds
    ``q2n_<dataset>``: the mean over the items of ``ops.metrics_q2n`` (Q4 / Q8 on 32 x 32 blocks), accumulated on the device with
    its workspace allocated once per shape and read in the same synchronising read.

    ``protocol="hqnr"`` (with ``full_resolution=True`` only: ValueError otherwise) scores each item with the set the
    PanCollection tables report instead: ``ops.metrics_hqnr(SR, MS, PAN, sensor)`` -- Khan's D_lambda, the block-wise D_s and
    HQNR (``metrics.hqnr``) -- with the buffers made once per shape, sums kept on the device and one synchronising read.  Returns
    ``{"d_lambda_k_<dataset>": ..., "d_s_<dataset>": ..., "hqnr_<dataset>": ..., "sec_per_item": ...}``; ValueError when the
    visuals carry no ``MS`` or ``PAN``.  ``sensor`` names the row of ``metrics.MTF_GAINS`` (or is a pair of explicit gains); it
    defaults to ``dataset`` when that has a row of its own -- a sensor name as it stands, never a prompt name translated -- and
    is required otherwise.  ``protocol="qnr"`` is the behaviour and the keys described above.

    ``baselines``: names out of ``BASELINES`` -- "exp", the interpolated ``MS`` itself, and "glp", "cbd", "hpm", the visuals'
    ``MS`` and ``PAN`` fused classically by ``ops.mtf_glp`` in that mode (``metrics.mtf_glp``; buffers made once per shape).
    Each is scored with the same metric set as the network in the mode that is active (``device_metrics=True``, or
    ``full_resolution=True`` with either protocol; the host-metric mode raises ValueError) under the keys
    ``"<metric>_<dataset>@<baseline>"``; the sums stay on the device and join the single synchronising read.  ``sensor`` is
    resolved as for ``protocol="hqnr"``.  ``baselines=()`` changes nothing: the same keys, values and launches.
    The names of ``CS_BASELINES`` ("cs-gs", "cs-gsa", "cs-brovey") are accepted beside them: the same visuals fused by
    ``ops.cs_fuse`` with that method (``metrics.cs_fuse``; buffers made once per shape), scored and reported the same way
    (``"<metric>_<dataset>@cs-gsa"``).  So are the names of ``BDSD_BASELINES``: "bdsd", ``ops.bdsd`` with one set of weights per
    image, and "bdsd-local", with weights per 128 x 128 block (``"<metric>_<dataset>@bdsd"``); "bdsd-local" raises ValueError
    naming the shape when the visuals' extents are not multiples of 128.  So is "tv" (``TV_BASELINES``): ``ops.tv_pansharpen`` at its
    defaults, with the samples MS[..., 2::4, 2::4] as its lr_ms and MS as its start (``"<metric>_<dataset>@tv"``; buffers made
    once per shape).  So are "atwt" and "awlp" (``ATROUS_BASELINES``): ``ops.awlp`` in that mode (``"<metric>_<dataset>@awlp"``;
    buffers made once per shape).

    ``d_rho=True`` (with ``full_resolution=True`` only: ValueError otherwise) adds ``d_rho_<dataset>``, the local PAN-correlation
    index ``metrics.d_rho`` of SR against PAN with 4 x 4 windows (``ops.local_corr_loss`` in its value-only mode; the sums stay on
    the device and join the single synchronising read), and ``d_rho_<dataset>@<baseline>`` for every baseline."""
    if d_rho and not full_resolution:
        raise ValueError("val_dataset(d_rho=True) scores without ground truth: it needs full_resolution=True")
    baselines = tuple(baselines)
    known = BASELINES + CS_BASELINES + BDSD_BASELINES + TV_BASELINES + ATROUS_BASELINES
    if [b for b in baselines if b not in known] or len(set(baselines)) != len(baselines):
        raise ValueError(f"val_dataset: baselines={baselines!r} (distinct names out of {known})")
    if baselines and not (device_metrics or full_resolution):
        raise ValueError("val_dataset(baselines=...) scores on the GPU: it needs device_metrics=True or full_resolution=True")
    if protocol not in ("qnr", "hqnr"):
        raise ValueError(f"val_dataset: protocol={protocol!r} ('qnr' or 'hqnr')")
    hqnr = protocol == "hqnr"
    if hqnr and not full_resolution:
        raise ValueError("val_dataset(protocol='hqnr') scores without ground truth: it needs full_resolution=True")
    if (hqnr or baselines) and sensor is None:
        if dataset not in metrics.MTF_GAINS:
            raise ValueError(f"val_dataset({'protocol=' + repr('hqnr') if hqnr else 'baselines=...'}): {dataset!r} has no row in "
                             f"metrics.MTF_GAINS: give the sensor")
        sensor = dataset
    if q2n and (full_resolution or not device_metrics):
        raise ValueError("val_dataset(q2n=True) scores on the GPU against ground truth: it needs device_metrics=True and "
                         "full_resolution=False")
    result_path = os.path.join(result_root, dataset)
    os.makedirs(result_path, exist_ok=True)
    scale = IMG_SCALE.get(dataset, 2047.0)
    ssim_sum = sam_sum = 0.0
    n = 0
    dev_sum, dev_ws, q2n_ws = None, {}, {}
    full_sum, full_ws = None, {}
    base_sum, glp_ws, cs_ws, bdsd_ws, tv_ws, awlp_ws = {}, {}, {}, {}, {}, {}

    def score_baselines(ms_d, pan_d, score_row):
        """Adds score_row(fused) of every baseline to its running sum; ms_d, pan_d: the item's MS and PAN in [0, 1]."""
        from . import ops
        for name in baselines:
            fused = ms_d
            if name in CS_BASELINES:
                if ms_d.shape not in cs_ws:
                    cs_ws[ms_d.shape] = (ops.cs_fuse_buffers(*ms_d.shape, ms_d.device), torch.empty_like(ms_d))
                buf, out = cs_ws[ms_d.shape]
                fused = ops.cs_fuse(ms_d, pan_d, sensor, 4, name[3:], out=out, buffers=buf)
            elif name in BDSD_BASELINES:
                block = BDSD_LOCAL_BLOCK if name == "bdsd-local" else None
                if block and (ms_d.shape[2] % block or ms_d.shape[3] % block):
                    raise ValueError(f"val_dataset(baselines=('bdsd-local',)): the visuals are {tuple(ms_d.shape)}; H and W must be "
                                     f"multiples of the block side {block}")
                if (ms_d.shape, block) not in bdsd_ws:
                    bdsd_ws[ms_d.shape, block] = (ops.bdsd_buffers(*ms_d.shape, ms_d.device, 4, block), torch.empty_like(ms_d))
                buf, out = bdsd_ws[ms_d.shape, block]
                fused = ops.bdsd(ms_d, pan_d, sensor, 4, block, out=out, buffers=buf)
            elif name in TV_BASELINES:
                if ms_d.shape not in tv_ws:
                    tv_ws[ms_d.shape] = (ops.tv_buffers(*ms_d.shape, ms_d.device, 4), torch.empty_like(ms_d),
                                         torch.empty_like(ms_d[..., 2::4, 2::4]))
                buf, out, low = tv_ws[ms_d.shape]
                low.copy_(ms_d[..., 2::4, 2::4])
                fused = ops.tv_pansharpen(low, pan_d, sensor, 4, x0=ms_d, out=out, buffers=buf)
            elif name in ATROUS_BASELINES:
                if ms_d.shape not in awlp_ws:
                    awlp_ws[ms_d.shape] = (ops.awlp_buffers(*ms_d.shape, ms_d.device, 4), torch.empty_like(ms_d))
                buf, out = awlp_ws[ms_d.shape]
                fused = ops.awlp(ms_d, pan_d, 4, name, out=out, buffers=buf)
            elif name != "exp":
                if ms_d.shape not in glp_ws:
                    glp_ws[ms_d.shape] = (ops.mtf_glp_buffers(*ms_d.shape, ms_d.device), torch.empty_like(ms_d))
                buf, out = glp_ws[ms_d.shape]
                fused = ops.mtf_glp(ms_d, pan_d, sensor, 4, name, out=out, buffers=buf)
            row = score_row(fused)
            base_sum[name] = row if name not in base_sum else base_sum[name] + row

    def with_d_rho(score_row, pan_d):
        """score_row, or with d_rho=True score_row with 1 - the mean rho of the image appended"""
        if not d_rho:
            return score_row
        from . import ops

        def both(f):
            mean_rho = torch.empty(f.shape[0], device=f.device, dtype=torch.float64)
            ops.local_corr_loss(f, pan_d, 4, grad=False, per_image=mean_rho)
            return torch.cat([score_row(f), 1.0 - mean_rho[:1]])          # image 0, as the rows beside it ([0])
        return both
    t0 = time.time()
    for idx, val_data in enumerate(val_loader):
        trainer.feed_data(val_data)
        trainer.test(continous=continous, prompt=dataset)
        vis = trainer.get_current_visuals()
        if full_resolution and not (("MS" if hqnr else "LR") in vis and "PAN" in vis):
            raise ValueError(f"val_dataset(full_resolution=True): the visuals need '{'MS' if hqnr else 'LR'}' and 'PAN', "
                             f"got {sorted(vis)}")
        if baselines and not ("MS" in vis and "PAN" in vis):
            raise ValueError(f"val_dataset(baselines=...): the visuals need 'MS' and 'PAN', got {sorted(vis)}")
        sr = to_hwc01(vis["SR"][-1])                       # last image of the returned stack (ref :136)
        scio.savemat(os.path.join(result_path, f"output_mulExm_{idx}.mat"), {"sr": sr * scale})
        if hqnr:
            from . import ops
            ms_d, pan_d, sr_d = _to_nchw01(vis["MS"]), _to_nchw01(vis["PAN"]), _to_nchw01(vis["SR"][-1])
            if sr_d.shape not in full_ws:
                full_ws[sr_d.shape] = ops.metrics_hqnr_buffers(*sr_d.shape, sr_d.device)
            score_row = with_d_rho(lambda f: ops.metrics_hqnr(f, ms_d, pan_d, sensor, buffers=full_ws[sr_d.shape])[0], pan_d)
            row = score_row(sr_d)
            full_sum = row if full_sum is None else full_sum + row
            if baselines:
                score_baselines(ms_d, pan_d, score_row)
        elif full_resolution:
            from . import ops
            lr_d, pan_d, sr_d = _to_nchw01(vis["LR"]), _to_nchw01(vis["PAN"]), _to_nchw01(vis["SR"][-1])
            key = (lr_d.shape, sr_d.shape)
            if key not in full_ws:
                full_ws[key] = (torch.empty(1, 1, *ops.pyr_down_shape(*pan_d.shape[2:]), device=pan_d.device),
                                ops.metrics_workspace(*sr_d.shape, sr_d.device))
            l_pan, ws = full_ws[key]
            ops.pyr_down(pan_d, 2, out=l_pan)
            score_row = with_d_rho(lambda f: ops.metrics_noref(lr_d, pan_d, l_pan, f, workspace=ws)[0], pan_d)
            row = score_row(sr_d)
            full_sum = row if full_sum is None else full_sum + row
            if baselines:
                score_baselines(_to_nchw01(vis["MS"]), pan_d, score_row)
        elif "HR" in vis and device_metrics:
            from . import ops
            hr_d, sr_d = _to_nchw01(vis["HR"]), _to_nchw01(vis["SR"][-1])
            if hr_d.shape not in dev_ws:
                dev_ws[hr_d.shape] = ops.metrics_workspace(*hr_d.shape, hr_d.device)
            row = ops.metrics_pair(hr_d, sr_d, 1.0, workspace=dev_ws[hr_d.shape])[0]
            if q2n:
                if hr_d.shape not in q2n_ws:
                    q2n_ws[hr_d.shape] = ops.metrics_q2n_workspace(*hr_d.shape, hr_d.device)
                row = torch.cat([row, ops.metrics_q2n(hr_d, sr_d, workspace=q2n_ws[hr_d.shape])])
            dev_sum = row if dev_sum is None else dev_sum + row
            if baselines:
                def pair_row(f):
                    r = ops.metrics_pair(hr_d, f, 1.0, workspace=dev_ws[hr_d.shape])[0]
                    return torch.cat([r, ops.metrics_q2n(hr_d, f, workspace=q2n_ws[hr_d.shape])]) if q2n else r
                score_baselines(_to_nchw01(vis["MS"]), _to_nchw01(vis["PAN"]), pair_row)
        elif "HR" in vis:
            hr = to_hwc01(vis["HR"])
            ssim_sum += metrics.ssim(hr, sr, 1)
            sam_sum += metrics.sam(hr, sr)
        n += 1
    if full_resolution:
        fields = (metrics.HQNR_FIELDS if hqnr else metrics.NOREF_FIELDS) + (("d_rho",) if d_rho else ())
        if base_sum:                                                                  # the baselines join the one read
            total = torch.cat([full_sum] + [base_sum[b] for b in baselines]).tolist()
        else:
            total = full_sum.tolist() if full_sum is not None else [0.0] * len(fields)   # the one synchronising read
        score = {**{f"{k}_{dataset}": v / max(n, 1) for k, v in zip(fields, total)},
                 "sec_per_item": (time.time() - t0) / max(n, 1)}
        for i, b in enumerate(baselines if base_sum else ()):
            score.update({f"{k}_{dataset}@{b}": v / max(n, 1) for k, v in zip(fields, total[(i + 1) * len(fields):])})
        log(dataset, score)
        return score
    extra = {}
    if dev_sum is not None:
        names = metrics.PAIR_FIELDS + (("q2n",) if q2n else ())
        flat = (torch.cat([dev_sum] + [base_sum[b] for b in baselines]) if base_sum else dev_sum).tolist()   # the one synchronising read
        total = dict(zip(names, flat))
        ssim_sum, sam_sum = total["ssim"], total["sam"]
        kept = ("psnr", "ergas", "scc", "cc", "q") + (("q2n",) if q2n else ())
        extra = {f"{k}_{dataset}": total[k] / max(n, 1) for k in kept}
        for i, b in enumerate(baselines if base_sum else ()):
            part = dict(zip(names, flat[(i + 1) * len(names):]))
            extra.update({f"{k}_{dataset}@{b}": part[k] / max(n, 1) for k in ("ssim", "sam") + kept})
    score = {f"ssim_{dataset}": ssim_sum / max(n, 1), f"sam_{dataset}": sam_sum / max(n, 1),
             "sec_per_item": (time.time() - t0) / max(n, 1), **extra}
    log(dataset, score)
    return score
