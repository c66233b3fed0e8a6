"""PanCollection data either side of the hot path (reference data/__init__.py, data/LRHR_dataset.py:87-133).

``LRHRDataset`` reads the four arrays ``gt`` (absent in full-resolution test files: ``lms`` stands in), ``ms``, ``lms``,
``pan`` ([N, C, h, w] digital numbers) from an ``.h5`` file (needs h5py, which this image does not ship), an ``.npz`` file
or any mapping of arrays, divides by the sensor range (1023 for GaoFen-2 files -- "gf2" in the path -- else 2047) and
serves the dictionaries the trainer consumes: ``LR`` (ms), ``PAN``, ``MS`` (the upsampled lms), ``HR`` (gt),
``Res`` = HR - MS.  A raw file that has ``ms`` and ``pan`` but no ``lms`` gets it once, at construction, from
``metrics.upsample_poly23(ms, pan width // ms width)``: the interpolator that made the ``lms`` of the PanCollection files.

``wald_pair`` makes a reduced-resolution training pair from a raw scene by Wald's protocol (MTF-matched low-pass per band,
decimation by the resolution ratio), and ``LRHRDataset(..., reduce="<sensor>")`` applies it once, at construction, to a raw
file that has ``ms`` and ``pan`` but neither ``gt`` nor ``lms``: the file's own ``ms`` becomes the ground truth.
"""
import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset

from .util import img2res


def _open(dataroot):
    if isinstance(dataroot, dict):
        return dataroot, "<mapping>"
    name = str(dataroot)
    if name.endswith(".npz"):
        return np.load(name), name
    try:
        import h5py
    except ImportError as e:        # pragma: no cover - h5py is absent in the build image
        raise ImportError(f"{name}: reading .h5 files needs h5py (not installed); convert to .npz or pass arrays") from e
    return h5py.File(name, "r"), name


def wald_pair(ms, pan, sensor, ratio=4):
    """A reduced-resolution training pair by Wald's protocol from ms [B, C, H, W] and pan [B, 1, ratio * H, ratio * W], H and W
    multiples of ``ratio``: the trainer's dictionary with HR = ms, LR = mtf_degrade(ms) [H / ratio], PAN = mtf_degrade(pan) with
    the sensor's PAN gain [H], MS = upsample_poly23(LR, ratio) [H] and Res = HR - MS.  ``sensor``: a key of
    ``metrics.MTF_GAINS`` (any other name takes the default row) or explicit gains (MS gains, PAN gain).  Tensors on the GPU go
    through the device operators (float32); host tensors and arrays through the float64 definitions of ``metrics``.  On the
    device LR and PAN are differentiable in ms and pan (``ops.mtf_degrade``: the backward is the adjoint kernel); MS, the
    interpolation of LR, carries no gradient."""
    from . import metrics
    if ratio not in (2, 4):
        raise ValueError(f"wald_pair: ratio={ratio} (2 or 4)")
    if not (len(ms.shape) == 4 and len(pan.shape) == 4 and pan.shape[1] == 1 and pan.shape[0] == ms.shape[0]
            and ms.shape[2] % ratio == 0 and ms.shape[3] % ratio == 0
            and tuple(pan.shape[2:]) == (ratio * ms.shape[2], ratio * ms.shape[3])):
        raise ValueError(f"wald_pair: ms {tuple(ms.shape)}, pan {tuple(pan.shape)} (ms [B, C, H, W] with H, W multiples of "
                         f"{ratio}, pan [B, 1, {ratio} H, {ratio} W])")
    ms_gains, pan_gain = metrics.mtf_gains(sensor, ms.shape[1])
    if torch.is_tensor(ms) and ms.is_cuda:
        from . import ops
        hr = ms.float().contiguous()
        lr = ops.mtf_degrade(hr, ms_gains, ratio)
        low_pan = ops.mtf_degrade(pan.float().contiguous(), (pan_gain,), ratio)
        up = ops.upsample_poly23(lr, ratio)
    else:
        hr = torch.as_tensor(ms).double()
        lr = torch.from_numpy(metrics.mtf_degrade(hr, ms_gains, ratio))
        low_pan = torch.from_numpy(metrics.mtf_degrade(pan, (pan_gain,), ratio))
        up = torch.from_numpy(metrics.upsample_poly23(lr, ratio))
    return {"LR": lr, "PAN": low_pan, "MS": up, "HR": hr, "Res": img2res(hr, up)}


class LRHRDataset(Dataset):
    def __init__(self, dataroot, data_len=-1, phase="train", img_scale=None, reduce=None):
        data, name = _open(dataroot)
        if img_scale is None:
            img_scale = 1023.0 if "gf2" in name else 2047.0
        self.img_scale, self.phase = img_scale, phase
        keys = set(data.keys())
        arr = lambda k: torch.from_numpy(np.array(data[k][...], dtype=np.float32) / img_scale)
        self.has_gt = "gt" in keys          # False: a full-resolution file, to be scored without a reference (evaluate.val_dataset)
        self.ms, self.pan = arr("ms"), arr("pan")
        if reduce is not None and not keys & {"gt", "lms"}:
            # a raw scene becomes a reduced-resolution set with a ground truth: Wald's protocol with the MTF of sensor `reduce`,
            # on the device when there is one, else through the host definitions
            to = (lambda t: t.cuda()) if torch.cuda.is_available() else (lambda t: t)
            pair = wald_pair(to(self.ms), to(self.pan), reduce, self.pan.shape[-1] // self.ms.shape[-1])
            self.ms, self.pan, self.lms, self.gt = (pair[k].float().cpu() for k in ("LR", "PAN", "MS", "HR"))
            self.has_gt = True
        else:
            if "lms" in keys:
                self.lms = arr("lms")
            else:                           # a raw (ms, pan) file: lms as PanCollection makes it
                from .metrics import upsample_poly23
                self.lms = torch.from_numpy(upsample_poly23(self.ms, self.pan.shape[-1] // self.ms.shape[-1])).float()
            self.gt = arr("gt") if self.has_gt else self.lms
        n = self.ms.shape[0]
        self.data_len = n if data_len is None or data_len <= 0 else min(data_len, n)

    def __len__(self):
        return self.data_len

    def __getitem__(self, index):
        hr, ms = self.gt[index].float(), self.lms[index].float()
        return {"LR": self.ms[index].float(), "PAN": self.pan[index].float(), "MS": ms, "HR": hr, "Res": img2res(hr, ms)}


def create_dataset(dataset_opt, phase):
    return LRHRDataset(dataroot=dataset_opt["dataroot"], data_len=dataset_opt["data_len"], phase=phase, reduce=dataset_opt.get("reduce"))


create_dataset2 = create_dataset       # the reference keeps two identical factories (data/__init__.py:22-38)


def create_dataloader(dataset, dataset_opt, phase, generator=None):
    """Training loaders use the option file's batch size / shuffle / workers; validation is one item at a time."""
    if "train" in phase:
        return DataLoader(dataset, batch_size=dataset_opt["batch_size"], shuffle=bool(dataset_opt["use_shuffle"]),
                          num_workers=dataset_opt["num_workers"] or 0, pin_memory=True, generator=generator)
    return DataLoader(dataset, batch_size=1, shuffle=False, num_workers=0, pin_memory=True)


def get_data_generator(loader):
    """Endless iterator over a loader (reference utils/util.py get_data_generator)."""
    while True:
        for batch in loader:
            yield batch
