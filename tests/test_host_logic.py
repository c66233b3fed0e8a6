"""CPU-only tests of the product's host side: the C-ABI library loads and exports what the header
declares, the module tree / checkpoint contract, schedule tables, DPM-Solver host maths, factory
options and error behaviour.  No kernel is launched here."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, assert_close
from oracle import unet_ref as U
from oracle.make_golden import TINY


def test_library_exports_every_declared_symbol():
    from tmdiff_amd import _lib
    header = open(os.path.join(ROOT, "include", "tmdiff_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(tmdiff_[a-z0-9_]+)\s*\(", header))
    declared -= {"tmdiff_conv3d_desc"}
    assert len(declared) >= 15
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} is declared in include/tmdiff_hip.h but not exported"
    assert declared == set(_lib.SIGNATURES), (declared ^ set(_lib.SIGNATURES))
    assert _lib.ABI_VERSION == 6
    assert ctypes.sizeof(_lib.Conv3dDesc) % 8 == 0


def test_attn_ctx_queries_per_workgroup():
    """The host function the attention launcher sizes the small-context kernel's workgroups with: 128 queries (one block per
    wave) doubling up to 1024 while the grid still fills the chip twice over; 0 where that kernel cannot run."""
    from tmdiff_amd import _lib
    qpw = _lib.lib.tmdiff_attn_ctx_queries_per_workgroup
    assert qpw(1, 1, 1, 1, 64) == 128 and qpw(1, 8, 4096, 77, 64) == 128
    assert qpw(16, 8, 2048, 77, 64) == 256 and qpw(32, 8, 2100, 96, 64) == 512
    assert qpw(32, 8, 4096, 77, 64) == 1024 and qpw(64, 8, 100000, 96, 64) == 1024
    for b, h, nq, nk, d in ((32, 8, 4096, 97, 64), (32, 8, 4096, 77, 32), (32, 8, 4096, 77, 128), (0, 8, 4096, 77, 64),
                            (32, 0, 4096, 77, 64), (32, 8, 0, 77, 64), (32, 8, 4096, 0, 64), (8192, 8, 4096, 77, 64)):
        assert qpw(b, h, nq, nk, d) == 0, (b, h, nq, nk, d)
    # whatever the heuristic picks, a workgroup's share is a whole number of 128-query passes, 1024 queries at the most
    for args in ((3, 5, 777, 77, 64), (64, 8, 1025, 77, 64), (1, 1, 5000, 96, 64), (7, 16, 130, 80, 64)):
        v = qpw(*args)
        assert v in (128, 256, 512, 1024), (args, v)


def test_state_dict_contract_and_clip_keys_ignored():
    from tmdiff_amd.Hyper_unet_general import WavBEST
    from tmdiff_amd.diffusion_general import GeneralDiffusion, GaussianDiffusion
    assert GaussianDiffusion is GeneralDiffusion
    ref = U.fill_weights_(U.WavBESTRef(channels=TINY))
    net = WavBEST(channels=TINY)
    assert list(net.state_dict().keys()) == list(ref.state_dict().keys())
    assert len(net.state_dict()) == 272
    for k, v in ref.state_dict().items():
        assert net.state_dict()[k].shape == v.shape, k
    sd = dict(ref.state_dict())
    sd["clip_text_model.transformer.text_model.embeddings.token_embedding.weight"] = torch.zeros(3)
    net.load_state_dict(sd, strict=True)              # reference checkpoints carry the CLIP weights
    diff = GeneralDiffusion(net, "l1")
    diff.set_new_noise_schedule({"schedule": "linear", "n_timestep": 10}, "cpu")
    keys = list(diff.state_dict().keys())
    assert keys[:12] == ["betas", "alphas_cumprod", "alphas_cumprod_prev", "sqrt_alphas_cumprod",
                         "sqrt_one_minus_alphas_cumprod", "log_one_minus_alphas_cumprod",
                         "sqrt_recip_alphas_cumprod_1", "sqrt_recipm1_alphas_cumprod_1", "posterior_variance",
                         "posterior_log_variance_clipped", "posterior_mean_coef1", "posterior_mean_coef2"]
    assert keys[12] == "denoise_fn.embed.0.weight" and len(keys) == 284


def test_schedule_tables_bitwise(golden):
    from tmdiff_amd.diffusion_general import GeneralDiffusion
    g = golden("schedules")
    for sched in ("cosine", "linear"):
        for T in (10, 50, 1000):
            d = GeneralDiffusion(None)
            d.set_new_noise_schedule({"schedule": sched, "n_timestep": T}, "cpu")
            for k, v in d.state_dict().items():
                assert np.array_equal(v.numpy(), g[f"{sched}_{T}_{k}"]), (sched, T, k)
            assert np.array_equal(d.sqrt_alphas_cumprod_prev, g[f"{sched}_{T}_sqrt_alphas_cumprod_prev"])
            assert d.num_timesteps == T and len(d._step_coef) == T
            i = T // 2
            assert d._step_coef[i][0] == float(d.sqrt_recip_alphas_cumprod_1[i])
            assert abs(d._step_coef[i][4] - float((0.5 * d.posterior_log_variance_clipped[i]).exp())) < 1e-12


def test_error_behaviour_matches_reference():
    from tmdiff_amd.diffusion_general import GeneralDiffusion
    from tmdiff_amd.Hyper_unet_general import WavBEST
    d = GeneralDiffusion(None, loss_type="huber")
    with pytest.raises(NotImplementedError):
        d.set_loss("cpu")
    with pytest.raises(NotImplementedError):
        d.set_new_noise_schedule({"schedule": "sigmoid", "n_timestep": 10}, "cpu")
    net = WavBEST(channels=TINY)
    x = torch.zeros(1, 4, 16, 16)
    with pytest.raises(RuntimeError, match="HIP kernels only"):     # no CPU fallback behind the product
        net(x, torch.tensor([[1]]), torch.zeros(1, 1, 16, 16), x, "QB")


def test_dpm_solver_host_math(golden):
    from tmdiff_amd.diffusion_general import GeneralDiffusion
    from tmdiff_amd.dpm_solver import DPM_Solver, NoiseScheduleVP
    g = golden("dpm_solver")
    d = GeneralDiffusion(None)
    d.set_new_noise_schedule({"schedule": "cosine", "n_timestep": 1000}, "cpu")
    ns = NoiseScheduleVP("discrete", betas=d.betas)
    tq = torch.tensor(g["ns_t"])
    assert_close(ns.marginal_log_mean_coeff(tq), g["ns_log_alpha"], 1e-6, 1e-6)
    assert_close(ns.marginal_std(tq), g["ns_std"], 1e-6, 1e-6)
    assert_close(ns.marginal_lambda(tq), g["ns_lambda"], 1e-6, 1e-6)
    assert_close(ns.inverse_lambda(ns.marginal_lambda(tq)), g["ns_inv_lambda"], 1e-5, 1e-5)
    solver = DPM_Solver(lambda x, t: x, ns, algorithm_type="dpmsolver++", correcting_x0_fn="dynamic_thresholding")
    for steps in (20, 30, 31, 32):
        outer, orders = solver.get_orders_and_timesteps_for_singlestep_solver(steps, 3, "logSNR", 1.0, 1e-3)
        assert list(orders) == list(g[f"orders_{steps}"])
        assert_close(outer, g[f"grid_{steps}"], 1e-5, 1e-5, "outer grid")
    with pytest.raises(ValueError):
        NoiseScheduleVP("sigmoid")
    with pytest.raises(ValueError):
        solver.get_time_steps("bogus", 1.0, 1e-3, 5)
    for sched in ("linear", "cosine"):                # continuous schedules: lambda round trip
        nc = NoiseScheduleVP(sched)
        t = torch.tensor([0.05, 0.3, 0.9])
        assert_close(nc.inverse_lambda(nc.marginal_lambda(t)), t, 1e-4, 1e-4, sched)


def test_define_general_reads_reference_options():
    from tmdiff_amd import networks
    opt = {"model": {"unet": {"channel_multiplier": TINY}, "diffusion": {"loss_type": "l2"}, "init_type": "orthogonal"},
           "phase": "train", "gpu_ids": None, "distributed": False}
    net = networks.define_General(opt)
    assert net.loss_type == "l2" and net.denoise_fn.channels == TINY
    assert float(net.denoise_fn.down1.conv20.conv20.bias.abs().sum()) == 0.0      # orthogonal init zeroes biases
    with pytest.raises(NotImplementedError):
        networks.init_weights(net, "xavier")
    opt["phase"] = "val"
    emb = {k: torch.ones(1, 768) * i for i, k in enumerate(("QB", "WV3", "GF2", "WV2", "WV4"))}
    opt["model"]["text_embeddings"] = emb
    net = networks.define_General(opt)
    assert float(net.denoise_fn.get_embeding("GF2")[0, 0]) == 2.0
    assert net.denoise_fn.get_embeding("LANDSAT") is None


def test_psnr_and_res2img():
    from tmdiff_amd.util import img2res, psnr, res2img
    a = torch.rand(2, 4, 8, 8)
    b = a + 0.01
    assert abs(psnr(a, b) - 40.0) < 1e-3          # fp32 (a+0.01)-a is 0.01 only to ~1e-6
    assert psnr(a, a) > 200
    assert torch.equal(img2res(res2img(a, b), b), (a + b) - b)


def test_metrics_against_direct_formulas():
    from tmdiff_amd import metrics as M
    g = torch.Generator().manual_seed(0)
    a = torch.rand(24, 20, 4, generator=g)
    b = (a + 0.05 * torch.randn(24, 20, 4, generator=g)).clamp(0, 1)
    want = np.mean([10 * np.log10(1.0 / float(((a[..., c] - b[..., c]) ** 2).mean())) for c in range(4)])
    assert abs(M.mpsnr(a, b) - want) < 1e-6
    ang = torch.arccos((a * b).sum(-1) / a.norm(dim=-1) / b.norm(dim=-1)).double()
    assert abs(M.sam(a, b) - float(ang.mean() * 180 / np.pi)) < 1e-5
    assert M.sam(a, a) < 0.05 and abs(M.ssim(a, a) - 1.0) < 1e-9
    # SSIM: direct sliding-window evaluation of the skimage definition for one band
    x, y = a[..., 0].double().numpy(), b[..., 0].double().numpy()
    vals = []
    for i in range(x.shape[0] - 6):
        for j in range(x.shape[1] - 6):
            p, q = x[i:i + 7, j:j + 7].ravel(), y[i:i + 7, j:j + 7].ravel()
            ux, uy = p.mean(), q.mean()
            vx, vy, vxy = p.var(ddof=1), q.var(ddof=1), np.cov(p, q, ddof=1)[0, 1]
            vals.append((2 * ux * uy + 1e-4) * (2 * vxy + 9e-4) / ((ux * ux + uy * uy + 1e-4) * (vx + vy + 9e-4)))
    assert abs(M.ssim(a[..., :1], b[..., :1]) - np.mean(vals)) < 1e-9
    assert abs(M.mpsnr(a.permute(2, 0, 1), b.permute(2, 0, 1), hwc=False) - want) < 1e-6


def test_sam_against_the_reference_fixture(golden):
    """N2, the pinnable part: tests/golden/metrics.npz holds SAM_numpy (core/metrics.py:91-112) of the REFERENCE on float32
    and float64 H x W x C arrays with zero / identical / parallel spectra among the pixels.  Same dtype, same operations:
    the float32 cases must agree to float32 rounding of the mean (they agree exactly here), float64 likewise."""
    from tmdiff_amd import metrics as M
    g = golden("metrics")
    for tag in ("wv3_f32", "gf2_f32", "wv3_f64"):
        hr, sr = g[f"{tag}_hr"], g[f"{tag}_sr"]
        assert abs(M.sam(sr, hr) - float(g[f"{tag}_sam"])) <= 1e-12 * max(1.0, float(g[f"{tag}_sam"])), tag
        assert abs(M.sam(hr, sr) - float(g[f"{tag}_sam_swapped"])) <= 1e-12, tag
        # tensors and the [C, H, W] layout go through the same arithmetic
        assert M.sam(torch.from_numpy(sr), torch.from_numpy(hr)) == M.sam(sr, hr)
        assert M.sam(np.moveaxis(sr, -1, 0), np.moveaxis(hr, -1, 0), hwc=False) == M.sam(sr, hr)
    # the dtype matters: the float32 fixture evaluated in float64 is a different number (identical spectra give exactly 0
    # there, a rounding-sized angle or NaN -> 0 in float32)
    hr, sr = g["wv3_f32_hr"], g["wv3_f32_sr"]
    assert M.sam(sr.astype(np.float64), hr.astype(np.float64)) != M.sam(sr, hr)


def test_tiling_helpers_roundtrip():
    from tmdiff_amd import tiling as T
    x = torch.arange(2 * 3 * 8 * 12, dtype=torch.float32).reshape(2, 3, 8, 12)
    t = T.split_tiles(x, 4, 6)
    assert t.shape == (8, 3, 4, 6)
    assert torch.equal(t[1], x[0, :, 0:4, 6:12]) and torch.equal(t[6], x[1, :, 4:8, 0:6])     # row-major tile order
    assert torch.equal(T.merge_tiles(t, 2, 2), x)
    img = torch.rand(1, 4, 16, 16)
    q = T.invPatch(img)
    assert q.shape == (4, 4, 8, 8) and torch.equal(q[3], img[0, :, 8:, 8:])                   # reference order
    cube = torch.rand(5, 32, 32)
    assert torch.equal(T.patch_16(T.unpatch_16(cube)), cube) and T.unpatch_16(cube).shape == (16, 5, 8, 8)


def _tiny_clip_dir(path):
    """A local 1-layer random CLIP text model + character-level tokenizer (stands in for clip-vit-large-patch14)."""
    import json
    from transformers import CLIPTextConfig, CLIPTextModel, CLIPTokenizer
    chars = [chr(c) for c in range(ord("a"), ord("z") + 1)] + list("0123456789.,-():")
    vocab = {}
    for suffix in ("", "</w>"):
        for ch in chars:
            vocab[ch + suffix] = len(vocab)
    vocab["<|startoftext|>"], vocab["<|endoftext|>"] = len(vocab), len(vocab) + 1
    with open(os.path.join(path, "vocab.json"), "w") as f:
        json.dump(vocab, f)
    with open(os.path.join(path, "merges.txt"), "w") as f:
        f.write("#version: 0.2\n")
    CLIPTokenizer(os.path.join(path, "vocab.json"), os.path.join(path, "merges.txt")).save_pretrained(path)
    eos = vocab["<|endoftext|>"]
    cfg = CLIPTextConfig(vocab_size=len(vocab), hidden_size=768, intermediate_size=64, num_hidden_layers=1,
                         num_attention_heads=4, max_position_embeddings=77, bos_token_id=vocab["<|startoftext|>"],
                         eos_token_id=eos, pad_token_id=eos)
    torch.manual_seed(0)
    CLIPTextModel(cfg).eval().save_pretrained(path)


def test_clip_embedder_and_embedding_cache(tmp_path):
    """FrozenCLIPEmbedder (ref core/clip.py:15-59) from a local directory, the five-paragraph cache file, and its
    injection into WavBEST (ref Hyper_unet_general.py:566-598)."""
    from tmdiff_amd import clip
    from tmdiff_amd.prompts import PROMPT_TEXT
    from tmdiff_amd.Hyper_unet_general import WavBEST, PROMPTS
    with pytest.raises(FileNotFoundError):
        clip.FrozenCLIPEmbedder("openai/clip-vit-large-patch14", device="cpu")      # never downloads
    d = str(tmp_path / "clip")
    os.makedirs(d)
    _tiny_clip_dir(d)
    emb = clip.FrozenCLIPEmbedder(d, device="cpu")
    assert not any(p.requires_grad for p in emb.parameters()) and not emb.transformer.training
    z = emb.encode(PROMPT_TEXT["QB"])
    assert z.shape == (1, 768) and torch.equal(z, emb.encode(PROMPT_TEXT["QB"]))
    assert clip.FrozenCLIPEmbedder(d, device="cpu", layer="last").encode("a b").shape == (1, 768)
    assert clip.FrozenCLIPEmbedder(d, device="cpu", layer="hidden", layer_idx=1).encode("a b").shape == (1, 77, 768)
    table = clip.build_text_embeddings(emb)
    assert set(table) == set(PROMPTS) == set(PROMPT_TEXT)
    assert not torch.equal(table["QB"], table["GF2"])           # (77 character-tokens only reach the sensor name here)
    out = str(tmp_path / "emb.pt")
    clip.main(["--clip", d, "--out", out, "--device", "cpu"])
    back = clip.load_text_embeddings(out)
    for k in PROMPTS:
        assert torch.equal(back[k], table[k])
    net = WavBEST([4, 8, 16, 32], text_embeddings=out)
    assert torch.equal(net.get_embeding("WV3"), table["WV3"]) and net.get_embeding("nope") is None
    assert net.get_prompt("WV2").startswith("The GaoFen-2") and net.get_prompt("nope") is None
    torch.save({"QB": table["QB"]}, out)
    with pytest.raises(KeyError):
        clip.load_text_embeddings(out)


def test_val_dataset_writes_mat_and_scores(tmp_path):
    """evaluate.val_dataset (ref driver :126-152) with a stand-in trainer: .mat key/scale/layout and SSIM/SAM."""
    import scipy.io as scio
    from tmdiff_amd import evaluate, metrics

    class Trainer:
        def feed_data(self, d):
            self.d = d

        def test(self, continous=False, prompt="QB"):
            self.prompt = prompt
            self.SR = torch.cat([torch.zeros_like(self.d["HR"]), self.d["HR"] * 1.5 - 0.2])   # stack; last = result

        def get_current_visuals(self):
            return {"SR": self.SR, "HR": self.d["HR"]}

    g = torch.Generator().manual_seed(3)
    loader = [{"HR": torch.rand(1, 4, 16, 16, generator=g)} for _ in range(2)]
    t = Trainer()
    score = evaluate.val_dataset(t, "GF2", loader, str(tmp_path), log=lambda *a: None)
    assert t.prompt == "GF2"
    m = scio.loadmat(os.path.join(str(tmp_path), "GF2", "output_mulExm_1.mat"))["sr"]
    want = evaluate.to_hwc01(loader[1]["HR"] * 1.5 - 0.2)
    assert m.shape == (16, 16, 4) and np.allclose(m, want * 1023.0, rtol=1e-6) and m.min() >= 0 and m.max() <= 1023.0
    hr1 = evaluate.to_hwc01(loader[1]["HR"])
    hr0, sr0 = evaluate.to_hwc01(loader[0]["HR"]), evaluate.to_hwc01(loader[0]["HR"] * 1.5 - 0.2)
    assert abs(score["ssim_GF2"] - (metrics.ssim(hr0, sr0, 1) + metrics.ssim(hr1, want, 1)) / 2) < 1e-12
    assert abs(score["sam_GF2"] - (metrics.sam(hr0, sr0) + metrics.sam(hr1, want)) / 2) < 1e-12
    evaluate.val_dataset(t, "WV3", loader[:1], str(tmp_path), log=lambda *a: None)
    assert np.allclose(scio.loadmat(os.path.join(str(tmp_path), "WV3", "output_mulExm_0.mat"))["sr"], sr0 * 2047.0, rtol=1e-6)


def _write_dataset(path, n, c, h, scale, with_gt=True, seed=0):
    g = np.random.default_rng(seed)
    arrays = {"ms": g.integers(0, scale, (n, c, h // 4, h // 4)).astype(np.float64),
              "lms": g.integers(0, scale, (n, c, h, h)).astype(np.float64),
              "pan": g.integers(0, scale, (n, 1, h, h)).astype(np.float64)}
    if with_gt:
        arrays["gt"] = g.integers(0, scale, (n, c, h, h)).astype(np.float64)
    np.savez(path, **arrays)
    return arrays


def test_config_parse_and_datasets(tmp_path):
    """Option file (ref core/logger.py:20-125) and PanCollection reader (ref data/LRHR_dataset.py:87-133)."""
    from tmdiff_amd import config as Config, data as Data
    cfg = tmp_path / "opt.json"
    cfg.write_text('''{
  "name": "best", // run name
  "phase": "val", "gpu_ids": [0],
  "path": {"log": "logs", "results": "results", "checkpoint": "checkpoint", "resume": "/nowhere/I100000"},
  "datasets": {"train_wv3": {"dataroot": "x.npz", "batch_size": 4, "num_workers": 0, "use_shuffle": true, "data_len": -1},
               "val_WV3": {"dataroot": "y.npz", "data_len": -1}},
  "model": {"beta_schedule": {"train": {"schedule": "cosine", "n_timestep": 1000}, "val": {"schedule": "cosine", "n_timestep": 1000}},
            "unet": {"channel_multiplier": [32, 64, 128, 256]}, "diffusion": {"loss_type": "l1"}, "init_type": "kaiming"},
  "train": {"val_freq": 2000, "save_checkpoint_freq": 2000, "print_freq": 50, "max_iter": 150000, "optimizer": {"lr": 1e-4}}
}''')
    opt = Config.parse(str(cfg), "train", root=str(tmp_path / "exp"))
    assert opt["phase"] == "train" and opt["distributed"] is False and opt["nothing"] is None
    assert opt["path"]["resume"] == "/nowhere/I100000"                       # resume paths are left alone
    assert opt["path"]["results"].startswith(str(tmp_path / "exp" / "best_")) and os.path.isdir(opt["path"]["results"])
    assert opt["model"]["unet"]["missing"] is None and "channel_multiplier" in Config.dict2str(opt)
    dbg = Config.parse(str(cfg), "train", gpu_ids="0,1", debug=True, root=str(tmp_path / "exp"), make_dirs=False)
    assert dbg["name"] == "debug_best" and dbg["distributed"] is True and dbg["gpu_ids"] == [0, 1]
    assert dbg["train"]["val_freq"] == 2 and dbg["model"]["beta_schedule"]["val"]["n_timestep"] == 10
    assert dbg["datasets"]["train_wv3"]["batch_size"] == 2 and dbg["datasets"]["val_WV3"]["data_len"] == 3

    raw = _write_dataset(str(tmp_path / "train_wv3.npz"), 5, 8, 16, 2047)
    ds = Data.LRHRDataset(str(tmp_path / "train_wv3.npz"), data_len=3)
    assert len(ds) == 3 and ds.img_scale == 2047.0
    item = ds[2]
    assert set(item) == {"LR", "PAN", "MS", "HR", "Res"} and item["LR"].shape == (8, 4, 4) and item["PAN"].shape == (1, 16, 16)
    np.testing.assert_allclose(item["HR"].numpy(), raw["gt"][2] / 2047.0, rtol=1e-6)
    np.testing.assert_allclose(item["Res"].numpy(), (raw["gt"][2] - raw["lms"][2]) / 2047.0, rtol=1e-5, atol=1e-7)
    raw2 = _write_dataset(str(tmp_path / "test_gf2_full.npz"), 2, 4, 16, 1023, with_gt=False)
    ds2 = Data.LRHRDataset(str(tmp_path / "test_gf2_full.npz"))
    assert ds2.img_scale == 1023.0 and len(ds2) == 2
    np.testing.assert_allclose(ds2[0]["HR"].numpy(), raw2["lms"][0] / 1023.0, rtol=1e-6)   # no gt: lms stands in
    assert float(ds2[0]["Res"].abs().max()) == 0.0
    loader = Data.create_dataloader(ds, {"batch_size": 2, "use_shuffle": False, "num_workers": 0}, "train_wv3")
    batch = next(Data.get_data_generator(loader))
    assert batch["MS"].shape == (2, 8, 16, 16)
    assert len(Data.create_dataloader(ds, {}, "val_WV3")) == 3


def test_h5_dataset_branch(tmp_path):
    """The PanCollection .h5 reader (reference data/LRHR_dataset.py:87-133) -- runs where h5py exists; this image does
    not ship it, and then the reader must say so instead of failing obscurely."""
    from tmdiff_amd import data as Data
    try:
        import h5py
    except ImportError:
        with pytest.raises(ImportError, match="h5py"):
            Data.LRHRDataset(str(tmp_path / "train_wv3.h5"))
        pytest.skip("h5py is not installed in this image: .h5 branch exercised only up to its error message")
    g = np.random.default_rng(0)
    arrs = {"gt": g.integers(0, 2047, (3, 8, 16, 16)), "lms": g.integers(0, 2047, (3, 8, 16, 16)),
            "ms": g.integers(0, 2047, (3, 8, 4, 4)), "pan": g.integers(0, 2047, (3, 1, 16, 16))}
    with h5py.File(str(tmp_path / "train_wv3.h5"), "w") as f:
        for k, v in arrs.items():
            f.create_dataset(k, data=v.astype(np.float64))
    ds = Data.LRHRDataset(str(tmp_path / "train_wv3.h5"))
    assert len(ds) == 3 and ds.img_scale == 2047.0
    np.testing.assert_allclose(ds[1]["HR"].numpy(), arrs["gt"][1] / 2047.0, rtol=1e-6)
    np.testing.assert_allclose(ds[1]["Res"].numpy(), (arrs["gt"][1] - arrs["lms"][1]) / 2047.0, rtol=1e-5, atol=1e-7)


def test_driver_dataset_sampling():
    """Per-iteration choice of the training set (ref driver :45-53, :158-160): weights 4 / 4 / 8 per batch."""
    from tmdiff_amd import train
    p = train.dataset_probabilities({"train_qb": 100, "train_gf2": 50, "train_wv3": 25})
    assert abs(p["train_qb"] - 400 / 800) < 1e-12 and abs(p["train_gf2"] - 200 / 800) < 1e-12
    assert train.sample_dataset(p, 0.49) == "train_qb" and train.sample_dataset(p, 0.5) == "train_gf2"
    assert train.sample_dataset(p, 0.7499) == "train_gf2" and train.sample_dataset(p, 0.75) == "train_wv3"
    assert train.sample_dataset(train.dataset_probabilities({"train_wv3": 3}), 0.1) == "train_wv3"


def test_winograd_transform_choice_and_sizes():
    """Host-side rules of the Winograd-along-the-bands convolution (no GPU work): F(4,3) for band counts whose tiles fill
    the kernel's pairs of tiles (8, 12, 16), F(2,3) for the other even counts (a single F(4,3) tile would leave half of
    every workgroup idle), nothing for odd counts; packed weights hold 9 x planes values per (ci, co)."""
    from tmdiff_amd import _lib
    lib = _lib.lib
    assert [lib.tmdiff_conv3d_wino_planes(n) for n in (2, 3, 4, 6, 8, 12, 16)] == [4, 0, 4, 4, 6, 6, 6]
    assert lib.tmdiff_conv3d_wino_packed_bytes(64, 32, 1, 6) == 32 * 54 * 64 * 4
    assert lib.tmdiff_conv3d_wino_packed_bytes(64, 32, 1, 4) == 32 * 36 * 64 * 4
    assert lib.tmdiff_conv3d_wino_packed_bytes(96, 192, 3, 6) == 64 * 54 * 96 * 4        # groups = 3: Cin / groups rows
    assert lib.tmdiff_conv3d_wino_packed_bytes(48, 32, 1, 6) == 0                          # Cout / groups not a multiple of 32
    assert lib.tmdiff_conv3d_wino_packed_bytes(64, 32, 1, 5) == 0                          # planes is 4 or 6
    assert lib.tmdiff_conv3d_ll_packed_bytes(64, 32) == 32 * 48 * 64 * 4


def test_routing_table_of_the_baseline_configs():
    """every 3x3x3 convolution of BASELINE configs[0..4] (B in {1, 8, 32}, 4 / 8 bands, 64^2 / 256^2 planes, both
    widths, fp32 and bf16) walked through tmdiff_amd.routing -- the table committed as profiles/r04_routing_table.txt
    (tools/routing_table.py).  Every family of the product path is reached by a BASELINE case, except the general-shape direct
    kernel ("fused"), which the reference's default widths reach; the transform-pass Winograd families (tmdiff_amd.fallback) are
    reached by none."""
    import collections
    from tmdiff_amd import ops, routing
    assert ops.config.as_dict() == ops.KernelConfig(env={}).as_dict(), "this table is that of the default switches"
    reached = collections.Counter()
    for label, ch, b, n, size, math in routing.BASELINE_CASES:
        rows = routing.unet_table(ch, b, n, size, size, math)
        assert len(rows) == 51, label                              # the 51 3x3x3 convolutions of one forward
        assert all(f in routing.PRODUCT_FAMILIES for _, f in rows), (label, [f for _, f in rows if f not in routing.PRODUCT_FAMILIES])
        reached.update(f for _, f in rows)
    assert set(reached) == set(routing.PRODUCT_FAMILIES) - {"fused"}, dict(reached)
    other = collections.Counter(f for _, ch, b, n, size, math in routing.OTHER_CASES for _, f in routing.unet_table(ch, b, n, size, size, math))
    assert "fused" in other and not (set(other) & set(routing.FALLBACK_FAMILIES)), dict(other)
    # the benchmark workload: nothing but conv3d_wf (pair mode at the 8x8 level) and its composed-LL mode
    bench = collections.Counter(f for _, f in routing.unet_table(routing.FULL, 32, 8, 64, 64))
    assert bench == {"wf": 40, "wf_pair": 8, "wfll": 3}, dict(bench)
    # what DOES reach the fallback module: even band counts other than 4 / 8 on grids that fill the chip
    assert routing.conv3_family(32, 64, 64, 12, 64, 64) == "wino4" and routing.conv3_family(32, 64, 64, 6, 64, 64) == "wino2"
    assert routing.conv3_family(1, 64, 64, 12, 16, 16) in ("staged", "fused")          # ... small grids stay direct
    # the committed table is this code's table
    import subprocess, sys
    path = os.path.join(ROOT, "profiles", "r04_routing_table.txt")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "routing_table.py")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-1000:]
    assert out.stdout == open(path).read(), "profiles/r04_routing_table.txt is stale: python tools/routing_table.py > " + path


def test_kernel_routing_rules_and_support_queries():
    """Host-side routing of the round-3 kernels (no GPU): which launches conv3d_wf takes itself and how it splits its input
    channels (the benchmark's shapes), when the composed Conv_0 + LL convolution runs with Winograd on top, the packed sizes of
    its weights, and the support queries of the Winograd-domain weight gradient."""
    import ctypes as C
    from tmdiff_amd import _lib, ops
    L = _lib.lib
    # benchmark batch (B = 32): every level is taken unsplit or with a split that still fills the chip
    assert ops.wf_route(32, 64, 64, 8, 64, 64) == (True, 1)
    assert ops.wf_route(32, 256, 256, 8, 16, 16) == (True, 1)                 # 512 tiles
    taken, split = ops.wf_route(32, 256, 256, 8, 8, 8)                        # pair mode: 16 pairs x 8 channel tiles = 128
    assert taken and split == 4                                               # (to 256, then once more: ranges of 32 chunks are long)
    assert ops.wf_route(32, 64, 64, 8, 16, 16)[1] == 2                        # 128 tiles of a 64-channel layer: short ranges
    assert ops.wf_route(32, 128, 128, 8, 16, 16)[1] == 2                      # 256 tiles, 32-chunk ranges: split once
    assert ops.wf_route(8, 128, 128, 8, 32, 32)[1] == 2 and ops.wf_route(8, 64, 64, 8, 32, 32)[1] == 2
    # a single image at the 8x8 level is half a pair: the fallback kernels; odd band counts and masks too
    assert not ops.wf_route(1, 256, 256, 8, 8, 8)[0]
    assert not ops.wf_route(32, 64, 64, 6, 64, 64)[0] and not ops.wf_route(32, 64, 64, 8, 64, 64, masked=True)[0]
    # composed Conv_0 + LL with Winograd on top: 8 bands, W % 8 == 0, Cout % 32 == 0
    assert ops.wfll_route(32, 64, 64, 8, 64, 64) and ops.wfll_route(32, 256, 256, 8, 16, 16)
    assert ops.wfll_route(32, 64, 64, 4, 64, 64) and not ops.wfll_route(32, 64, 64, 6, 64, 64) and not ops.wfll_route(32, 64, 48, 8, 64, 64)
    assert L.tmdiff_conv3d_wfll_packed_bytes(64, 32) == 32 * 96 * 64 * 4 and L.tmdiff_conv3d_wfll_packed_bytes(48, 32) == 0
    # Winograd-domain weight gradient: N % 4 == 0, W % 4 == 0, 3x3x3
    d = _lib.Conv3dDesc()
    d.B, d.N, d.H, d.W, d.Cin, d.Cout, d.groups, d.ksize, d.nseg = 8, 8, 64, 64, 64, 64, 1, 3, 1
    d.seg_c[0] = 64
    assert L.tmdiff_conv3d_wgrad_wino_supported(C.byref(d)) == 1
    ws = L.tmdiff_conv3d_wgrad_wino_workspace_bytes(C.byref(d))
    xh = 6 * 16 * 66 * 66 * 64 * 4                    # x^: six planes x (b, tile) x padded plane x channels
    gh = 6 * 16 * 64 * 64 * 64 * 4
    assert ws > xh + gh and ws < 2 * (xh + gh)
    for field, bad in (("N", 6), ("W", 62), ("ksize", 1), ("groups", 2)):
        e = _lib.Conv3dDesc.from_buffer_copy(d)
        setattr(e, field, bad)
        assert L.tmdiff_conv3d_wgrad_wino_supported(C.byref(e)) == 0, field


def test_side_prologue_rule_on_the_benchmark_workload():
    """routing.k1_side_xp (which 1x1x1 launches can also write the prologue output of their input: conv1.hip's 16-byte form on
    large grids, the channels-over-the-waves form on small ones): the four three-segment res_conv launches of the benchmark
    workload's up path all qualify -- which is why no prologue pass is left in its step -- and the shapes neither form takes
    do not."""
    from tmdiff_amd import routing
    up_path = [((32, 32, 32), 32, 64, 64), ((64, 64, 64), 32, 32, 32), ((128, 128, 128), 64, 16, 16), ((256, 256, 256), 128, 8, 8)]
    for seg_c, cout, h, w in up_path:
        assert routing.k1_side_xp(32, seg_c, cout, 8, h, w), (seg_c, cout, h, w)
    assert routing.k1_side_xp(1, (256, 256, 256), 128, 8, 8, 8)             # a single tile: still the small-grid form
    assert not routing.k1_side_xp(1, (32, 32, 32), 32, 8, 8, 8)             # a small grid of fewer than 128 input channels
    assert not routing.k1_side_xp(32, (32, 24, 40), 32, 8, 64, 64)          # a segment that is not a multiple of 16 channels
    assert not routing.k1_side_xp(32, (32, 32, 32), 48, 8, 64, 64)          # Cout not a multiple of 32
    assert not routing.k1_side_xp(32, (32, 32, 32), 32, 3, 7, 9)            # a plane that is not a multiple of 4 positions




# ---- descriptor validation of the convolution entry points --------------------------------------------------------------
# Every case below is refused (or, for an empty batch, accepted) before the entry point makes a HIP call.  The child process
# sees no GPU (HIP_VISIBLE_DEVICES=-1), so a case that wrongly got past validation fails on the missing device instead of
# launching on placeholder pointers.  The pointers are placeholders only ("A": 16-byte aligned, "U": not) and are never
# dereferenced.
_VALIDATION_CHILD = r"""
import ctypes as C, json, sys
sys.path.insert(0, sys.argv[1])
from tmdiff_amd import _lib
L = _lib.lib
PTR = {"A": 0x10000, "U": 0x10004}
A = PTR["A"]
dx, acc = (C.c_void_p * 3)(A, A, A), (C.c_int32 * 3)(0, 0, 0)
ENTRIES = {
    "conv3d_fwd": lambda p: L.tmdiff_conv3d_fwd(p, None),
    "conv3d_fwd_xp_supported": lambda p: L.tmdiff_conv3d_fwd_xp_supported(p),
    "conv3d_fwd_staged": lambda p: L.tmdiff_conv3d_fwd_staged(p, A, None),
    "conv3d_fwd_bf16": lambda p: L.tmdiff_conv3d_fwd_bf16(p, None, None),
    "conv3d_fwd_bf16_ws": lambda p: L.tmdiff_conv3d_fwd_bf16(p, A, None),
    "conv3d_ll_fwd": lambda p: L.tmdiff_conv3d_ll_fwd(p, 0.5, None),
    "conv3d_wf_fwd": lambda p: L.tmdiff_conv3d_wf_fwd(p, A, None),
    "conv3d_wfll_fwd": lambda p: L.tmdiff_conv3d_wfll_fwd(p, 0.5, None),
    "conv3d_wino_fwd": lambda p: L.tmdiff_conv3d_wino_fwd(p, A, None),
    "conv3d_prologue_fwd": lambda p: L.tmdiff_conv3d_prologue_fwd(p, A, None),
    "conv3d_wgrad": lambda p: L.tmdiff_conv3d_wgrad_bias(p, A, A, A, A, None),
    "conv3d_wgrad_wino": lambda p: L.tmdiff_conv3d_wgrad_wino_bias(p, A, A, A, A, None),
    "prologue_bwd": lambda p: L.tmdiff_conv3d_prologue_bwd_ws(p, A, dx, acc, None, None, None, None),
}
out = []
for entry, fields in json.loads(sys.argv[2]):
    d = None
    if fields is not None:
        d = _lib.Conv3dDesc()
        d.bias_scale = d.out_scale = 1.0
        for k, v in fields.items():
            if isinstance(v, list):
                for i, x in enumerate(v):
                    getattr(d, k)[i] = PTR.get(x, x)
            else:
                setattr(d, k, PTR.get(v, v))
    assert L.tmdiff_conv3d_pack_weights(None, None, 1, 1, 3, 1, 0, None) != 0   # a known message in the error buffer
    rc = ENTRIES[entry](C.byref(d) if d is not None else None)
    out.append([rc, L.tmdiff_last_error_string().decode()])
print(json.dumps(out))
"""

_BASE_DESC = dict(B=2, N=8, H=16, W=16, Cin=64, Cout=64, groups=1, ksize=3, nseg=1, seg_c=[64], seg_x=["A"], w_packed="A", y="A")
_BAD_DESC = {
    "null": None,
    "nseg0": dict(nseg=0), "nseg4": dict(nseg=4),
    "seg_null": dict(seg_x=[0]),
    "seg_empty": dict(nseg=2, seg_c=[64, 0], seg_x=["A", "A"]),
    "csum": dict(nseg=2, seg_c=[32, 16], seg_x=["A", "A"]),
    "groups3_unequal": dict(groups=3, Cin=96, Cout=96, nseg=3, seg_c=[16, 32, 48], seg_x=["A", "A", "A"]),
    "mask_and_drop": dict(in_mask="A", drop_p=0.1), "drop1": dict(drop_p=1.0),
    "no_weights": dict(w_packed=0), "no_output": dict(y=0),
    "unaligned_x": dict(seg_x=["U"]), "unaligned_w": dict(w_packed="U"), "unaligned_y": dict(y="U"),
    "bad_extents": dict(N=0), "ksize2": dict(ksize=2), "groups2": dict(groups=2), "groups0": dict(groups=0), "indivisible": dict(groups=3),
    "B0": dict(B=0), "B0_seg_null": dict(B=0, seg_x=[0]), "B0_drop1": dict(B=0, drop_p=1.0),
}
# entry -> {case: (return code, prefix of the message)}: -1 = TMDIFF_E_INVALID, -2 = TMDIFF_E_UNSUPPORTED, 0 = accepted.  Cases
# an entry point lets through to its launch are not listed for it.
_INVALID = ("null", "nseg0", "nseg4", "seg_null", "seg_empty", "csum", "no_weights", "no_output", "bad_extents")
_SHAPE = ("nseg0", "nseg4", "mask_and_drop", "drop1", "bad_extents", "ksize2", "groups2", "indivisible")


def _expect(name, invalid=(), unsupported=(), ok=(), **other):
    t = {c: (-1, name) for c in invalid}
    t.update({c: (-2, name) for c in unsupported})
    t.update({c: (0, None) for c in ok})
    t.update(other)
    return t


_VALIDATION = {
    "conv3d_fwd": _expect("conv3d_fwd", _INVALID + ("groups3_unequal", "mask_and_drop", "drop1", "ksize2", "groups2", "indivisible"),
                          ok=("B0", "B0_seg_null", "B0_drop1")),
    "conv3d_fwd_staged": _expect("conv3d_fwd_staged", _INVALID + ("mask_and_drop", "drop1", "unaligned_w"),
                                 ("ksize2", "groups2", "indivisible"), ("B0", "B0_seg_null", "B0_drop1")),
    "conv3d_fwd_bf16": _expect("conv3d_fwd_bf16", _INVALID + ("groups3_unequal", "unaligned_w", "ksize2", "groups2", "indivisible"),
                               ("mask_and_drop", "drop1", "B0_drop1"), ("B0", "B0_seg_null")),
    "conv3d_ll_fwd": _expect("conv3d_ll_fwd", ("null", "seg_null", "no_weights", "no_output", "unaligned_w", "bad_extents"),
                             ("nseg0", "nseg4", "mask_and_drop", "drop1", "ksize2", "groups2", "indivisible", "seg_empty", "csum",
                              "groups3_unequal", "B0_drop1"),
                             ("B0", "B0_seg_null")),
    "conv3d_wf_fwd": _expect("conv3d_wf_fwd", ("null", "seg_null", "seg_empty", "csum", "no_weights", "no_output", "unaligned_x",
                                               "unaligned_w"), _SHAPE + ("unaligned_y", "B0_drop1"), ("B0", "B0_seg_null")),
    # (the composed Conv_0 + LL entry point translates its descriptor and hands it to the conv3d_wf_fwd checks)
    "conv3d_wfll_fwd": _expect("conv3d_wf_fwd", ("seg_null", "no_weights", "no_output", "unaligned_x", "unaligned_w"), ("unaligned_y",),
                               ("B0", "B0_seg_null"), **{c: (-2, "conv3d_wfll_fwd") for c in _SHAPE + (
                                   "null", "seg_empty", "csum", "groups3_unequal", "B0_drop1")}),
    "conv3d_wino_fwd": _expect("conv3d_wino_fwd", ("null", "seg_null", "seg_empty", "csum", "no_weights", "no_output", "unaligned_x",
                                                   "unaligned_w"), _SHAPE + ("B0_drop1",), ("B0", "B0_seg_null")),
    "conv3d_prologue_fwd": _expect("conv3d_prologue_fwd", ("null", "nseg0", "nseg4", "seg_null", "seg_empty", "csum", "bad_extents",
                                                           "B0_seg_null"), ok=("B0", "B0_drop1")),
    # (the direct weight gradient takes any group count that divides the channels: groups = 2 goes through to its launch)
    "conv3d_wgrad": _expect("conv3d_wgrad", ("null", "nseg0", "nseg4", "seg_null", "seg_empty", "csum", "mask_and_drop",
                                             "bad_extents", "ksize2", "groups0", "indivisible", "B0")),
    "conv3d_wgrad_wino": _expect("conv3d_wgrad_wino", ("null", "seg_null", "seg_empty", "csum", "mask_and_drop", "unaligned_x"),
                                 ("nseg0", "nseg4", "bad_extents", "ksize2", "groups2", "indivisible", "B0")),
    "prologue_bwd": _expect("prologue_bwd", ("null", "nseg0", "nseg4", "seg_null", "csum", "mask_and_drop", "B0")),
}


def _run_validation_child(calls):
    import json, subprocess, sys
    env = {k: v for k, v in os.environ.items() if k not in ("ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES")}
    env["HIP_VISIBLE_DEVICES"] = "-1"
    p = subprocess.run([sys.executable, "-c", _VALIDATION_CHILD, ROOT, json.dumps(calls)], capture_output=True, text=True, env=env,
                       timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def _desc(case, **base):
    bad = _BAD_DESC[case]
    return None if bad is None else dict(_BASE_DESC, **base, **bad)


def test_conv_entry_points_validate_descriptors():
    """Return code and message prefix of every convolution entry point for a table of malformed descriptors (NULL descriptor,
    nseg 0 / 4, NULL / empty segments, a channel sum other than Cin, unequal segments of a grouped convolution, a mask with
    drop_p, drop_p = 1, no weights, no output, unaligned pointers where alignment is required, bad extents / ksize / groups) and
    for an empty batch, which some entry points accept before their segment or dropout checks and others after them."""
    table = [(entry, case, want) for entry, cases in _VALIDATION.items() for case, want in cases.items()]
    got = _run_validation_child([[entry, _desc(case)] for entry, case, _ in table])
    bad = [f"{entry} / {case}: want {rc} '{prefix}: ...', got {got_rc} '{msg}'"
           for (entry, case, (rc, prefix)), (got_rc, msg) in zip(table, got)
           if got_rc != rc or (rc != 0 and not msg.startswith(prefix + ":"))]
    assert not bad, "\n".join(bad)


def test_conv_fwd_xp_supported_refuses_malformed_descriptors():
    """tmdiff_conv3d_fwd_xp_supported: 1 for a raw 1x1x1 input the small-grid bandwidth kernel takes, 0 for the malformed forms of
    that descriptor and for an empty batch."""
    xp = dict(ksize=1, Cin=128, seg_c=[128], xp_out="A")
    bad = [None, dict(nseg=0), dict(nseg=4), dict(seg_x=[0]), dict(nseg=2, seg_c=[128, 0], seg_x=["A", "A"]),
           dict(nseg=2, seg_c=[64, 16], seg_x=["A", "A"]), dict(w_packed=0), dict(groups=3), dict(B=0)]
    got = _run_validation_child([["conv3d_fwd_xp_supported", dict(_BASE_DESC, **xp)]] +
                                [["conv3d_fwd_xp_supported", None if b is None else dict(_BASE_DESC, **dict(xp, **b))] for b in bad])
    assert [g[0] for g in got] == [1] + [0] * len(bad), got


def test_splitk_workspace_queries():
    """Bytes of split-K partial outputs the fp32 3x3x3, LL and Winograd entry points ask for: ksplit x B x Cout x output plane x 4
    bytes on small grids, 0 where the grid fills the chip or the descriptor is not taken."""
    import ctypes as C
    from tmdiff_amd import _lib
    L = _lib.lib

    def desc(**f):
        d = _lib.Conv3dDesc()
        for k, v in dict(_BASE_DESC, seg_x=[0], w_packed=0, y=0, **f).items():
            if isinstance(v, list):
                for i, x in enumerate(v):
                    getattr(d, k)[i] = x
            else:
                setattr(d, k, v)
        return C.byref(d)

    small = dict(B=1, H=8, W=8, Cin=256, Cout=256, seg_c=[256])   # 8x8x8: one image leaves most of the chip idle
    out = 256 * 8 * 8 * 8 * 4                                        # B x Cout x output plane x 4 bytes
    assert L.tmdiff_conv3d_fwd_splitk_workspace_bytes(desc(**small)) == 32 * out
    assert L.tmdiff_conv3d_fwd_splitk_workspace_bytes(desc(**dict(small, ksize=1))) == 0
    assert L.tmdiff_conv3d_fwd_splitk_workspace_bytes(desc(B=32, H=64, W=64)) == 0
    assert L.tmdiff_conv3d_fwd_splitk_workspace_bytes(None) == 0
    assert L.tmdiff_conv3d_ll_splitk_workspace_bytes(desc(**dict(small, H=16, W=16))) == 32 * out
    assert L.tmdiff_conv3d_wf_splitk_workspace_bytes(desc(**dict(small, W=16))) == 32 * 2 * out
    assert L.tmdiff_conv3d_wfll_splitk_workspace_bytes(desc(**dict(small, Cin=64, seg_c=[64], H=16, W=16))) == 32 * out


# ---- the 32-bit size limits of the convolution families ------------------------------------------------------------------
# Each case is a descriptor just inside (True) or just past (False) one limit an entry point enforces for its 32-bit offsets
# or its grid.  The support queries must answer 0 exactly where the entry point refuses; a refusal is TMDIFF_E_UNSUPPORTED with
# the entry's message prefix, an accepted descriptor gets past validation and fails on the missing device only.
_RC = dict(rc_x="A", rc_w="A", rc_cin=64)
_SIZE_CASES = [
    # (label, entry, prefix, fields over _BASE_DESC, accepted, support queries)
    ("wf plane 4x2048x2048", "conv3d_wf_fwd", "conv3d_wf_fwd", dict(B=2, N=4, H=2048, W=2048, Cin=4, seg_c=[4]), True, "wf"),
    ("wf plane 4x2048x2052", "conv3d_wf_fwd", "conv3d_wf_fwd", dict(B=2, N=4, H=2048, W=2052, Cin=4, seg_c=[4]), False, "wf"),
    ("wf plane 8x1024x2048", "conv3d_wf_fwd", "conv3d_wf_fwd", dict(N=8, H=1024, W=2048, Cin=4, seg_c=[4]), True, "wf"),
    ("wf plane 8x1024x2052", "conv3d_wf_fwd", "conv3d_wf_fwd", dict(N=8, H=1024, W=2052, Cin=4, seg_c=[4]), False, "wf"),
    ("wf pair (Cin+2) plane < 2^29", "conv3d_wf_fwd", "conv3d_wf_fwd", dict(N=8, H=131071, W=8, Cin=62, seg_c=[62]), True, "wf"),
    ("wf pair (Cin+2) plane = 2^29", "conv3d_wf_fwd", "conv3d_wf_fwd", dict(N=8, H=131072, W=8, Cin=62, seg_c=[62]), False, "wf"),
    ("wf rc_cin plane < 2^30", "conv3d_wf_fwd", "conv3d_wf_fwd", dict(N=4, H=2048, W=2044, **_RC), True, "wf_opt"),
    ("wf rc_cin plane = 2^30", "conv3d_wf_fwd", "conv3d_wf_fwd", dict(N=4, H=2048, W=2048, **_RC), False, "wf_opt"),
    ("wf prologue B*Cin 65472", "conv3d_wf_fwd", "conv3d_wf_fwd", dict(B=1023, in_act=1), True, "wf_opt"),
    ("wf prologue B*Cin 65536", "conv3d_wf_fwd", "conv3d_wf_fwd", dict(B=1024, in_act=1), False, "wf_opt"),
    ("wfll plane 4x2048x2048 (s2d)", "conv3d_wfll_fwd", "conv3d_wf_fwd", dict(N=4, H=4096, W=4096, Cin=1, seg_c=[1]), True, "wfll"),
    ("wfll plane 4x2052x2048 (s2d)", "conv3d_wfll_fwd", "conv3d_wfll_fwd", dict(N=4, H=4096, W=4104, Cin=1, seg_c=[1]), False, "wfll"),
    ("bf16 plane 2^31 - 8", "conv3d_fwd_bf16", "conv3d_fwd_bf16", dict(N=8, H=16384, W=16383), True, "bf16"),
    ("bf16 plane 2^31", "conv3d_fwd_bf16", "conv3d_fwd_bf16", dict(N=8, H=16384, W=16384), False, "bf16"),
    ("bf16 pack B*Cin/8 65535", "conv3d_fwd_bf16_ws", "conv3d_fwd_bf16", dict(B=65535, Cin=8, seg_c=[8]), True, "bf16_ws"),
    ("bf16 pack B*Cin/8 65536", "conv3d_fwd_bf16_ws", "conv3d_fwd_bf16", dict(B=65536, Cin=8, seg_c=[8]), False, "bf16_ws"),
    ("fused plane 2^31 - 8", "conv3d_fwd", "conv3d_fwd", dict(N=8, H=16384, W=16383, Cin=1, Cout=1, seg_c=[1]), True, "fused"),
    ("fused plane 2^31", "conv3d_fwd", "conv3d_fwd", dict(N=8, H=16384, W=16384, Cin=1, Cout=1, seg_c=[1]), False, "fused"),
    ("staged plane 8 < 2^31", "conv3d_fwd_staged", "conv3d_fwd_staged", dict(N=8, H=4096, W=8191, Cin=4, Cout=32, seg_c=[4]), True, "staged"),
    ("staged plane 8 = 2^31", "conv3d_fwd_staged", "conv3d_fwd_staged", dict(N=8, H=4096, W=8192, Cin=4, Cout=32, seg_c=[4]), False, "staged"),
    ("staged prologue B*Cin 65472", "conv3d_fwd_staged", "conv3d_fwd_staged", dict(B=1023, in_act=1), True, "staged"),
    ("staged prologue B*Cin 65536", "conv3d_fwd_staged", "conv3d_fwd_staged", dict(B=1024, in_act=1), False, "staged"),
    ("staged plain B*Cin 65536", "conv3d_fwd_staged", "conv3d_fwd_staged", dict(B=1024), True, "staged"),
    ("ll Cin plane < 2^30", "conv3d_ll_fwd", "conv3d_ll_fwd", dict(N=8, H=1024, W=2046), True, "ll"),
    ("ll Cin plane = 2^30", "conv3d_ll_fwd", "conv3d_ll_fwd", dict(N=8, H=1024, W=2048), False, "ll"),
    ("wino plane 2x2048x2048", "conv3d_wino_fwd", "conv3d_wino_fwd", dict(N=2, H=2048, W=2048, Cin=2, seg_c=[2]), True, "wino"),
    ("wino plane 2x2048x2052", "conv3d_wino_fwd", "conv3d_wino_fwd", dict(N=2, H=2048, W=2052, Cin=2, seg_c=[2]), False, "wino"),
    ("wino input < 2^30", "conv3d_wino_fwd", "conv3d_wino_fwd", dict(N=2, H=1022, W=4088), True, "wino"),
    ("wino input = 2^30", "conv3d_wino_fwd", "conv3d_wino_fwd", dict(N=2, H=1022, W=4092), False, "wino"),
    ("wino B*Cin 65472", "conv3d_wino_fwd", "conv3d_wino_fwd", dict(B=1023), True, "wino"),
    ("wino B*Cin 65536", "conv3d_wino_fwd", "conv3d_wino_fwd", dict(B=1024), False, "wino"),
    ("k1 x' Cin plane < 2^30", "conv3d_fwd", "conv3d_fwd", dict(ksize=1, B=1, N=4, H=2048, W=2047, xp_out="A"), True, "xp"),
    ("k1 x' Cin plane = 2^30", "conv3d_fwd", "conv3d_fwd", dict(ksize=1, B=1, N=4, H=2048, W=2048, xp_out="A"), False, "xp"),
    # (past plane * 16 < 2^31 the bandwidth kernel leaves a 1x1x1 convolution to the general kernel; x' is bounded sooner)
    ("k1 plane 16 = 2^31", "conv3d_fwd", "conv3d_fwd", dict(ksize=1, B=1, N=8, H=4096, W=4096, Cin=16, seg_c=[16]), True, None),
    ("wgrad plane 32 < 2^31", "conv3d_wgrad", "conv3d_wgrad", dict(B=1, N=4, H=4096, W=4095, Cin=4, Cout=32, seg_c=[4]), True, None),
    ("wgrad plane 32 = 2^31", "conv3d_wgrad", "conv3d_wgrad", dict(B=1, N=4, H=4096, W=4096, Cin=4, Cout=32, seg_c=[4]), False, None),
    ("wgrad_wino 2 B T 65534", "conv3d_wgrad_wino", "conv3d_wgrad_wino", dict(B=8191, N=16, H=8, W=8), True, "ww"),
    ("wgrad_wino 2 B T 65536", "conv3d_wgrad_wino", "conv3d_wgrad_wino", dict(B=8192, N=16, H=8, W=8), False, "ww"),
]
_SIZE_QUERIES = {        # family -> the queries that answer 0 exactly where its entry point refuses
    "wf": ("tmdiff_conv3d_wf_supported", "tmdiff_conv3d_wf_blocks", "tmdiff_conv3d_wf_plan"),
    "wf_opt": ("tmdiff_conv3d_wf_supported", "tmdiff_conv3d_wf_blocks"),      # (limits of an optional input: not the plan's)
    "wfll": ("tmdiff_conv3d_wfll_supported",),
    "bf16_ws": ("tmdiff_conv3d_bf16_workspace_bytes",),
    "staged": ("tmdiff_conv3d_fwd_staged_supported",),
    "ll": ("tmdiff_conv3d_ll_supported",),
    "wino": ("tmdiff_conv3d_wino_supported", "tmdiff_conv3d_wino_blocks", "tmdiff_conv3d_wino_workspace_bytes"),
    "xp": ("tmdiff_conv3d_fwd_xp_supported",),
    "ww": ("tmdiff_conv3d_wgrad_wino_supported",),
}
_SIZE_CHILD = r"""
import ctypes as C, json, sys
sys.path.insert(0, sys.argv[1])
from tmdiff_amd import _lib
L = _lib.lib
PTR = {"A": 0x10000}
out = []
for fields, queries in json.loads(sys.argv[2]):
    d = _lib.Conv3dDesc()
    d.bias_scale = d.out_scale = 1.0
    for k, v in fields.items():
        if isinstance(v, list):
            for i, x in enumerate(v):
                getattr(d, k)[i] = PTR.get(x, x)
        else:
            setattr(d, k, PTR.get(v, v))
    r = {}
    for q in queries:
        if q == "tmdiff_conv3d_wf_plan":
            r[q] = L.tmdiff_conv3d_wf_plan(d.B, d.Cin, d.Cout, d.N, d.H, d.W, d.groups, 0, None)
        else:
            r[q] = int(getattr(L, q)(C.byref(d)))
    out.append(r)
print(json.dumps(out))
"""


def _size_desc(fields):
    return dict(_BASE_DESC, **fields)


def test_size_limits_agree_among_entry_points_support_queries_and_routing():
    """Every 32-bit size limit of the convolution families, one descriptor just inside and one just past it: the entry point
    accepts the one (and then fails on the missing device only) and refuses the other with TMDIFF_E_UNSUPPORTED and its own
    message prefix; the support queries, the wf launch plan and the workspace queries answer 0 exactly where the entry point
    refuses; the routing layer never names a family that refuses a shape, and past a limit it falls through to one that
    takes it."""
    import json, subprocess, sys
    from tmdiff_amd import routing
    got = _run_validation_child([[entry, _size_desc(f)] for _, entry, _, f, _, _ in _SIZE_CASES])
    bad = []
    for (label, entry, prefix, f, ok, _), (rc, msg) in zip(_SIZE_CASES, got):
        if ok and rc in (0, -1, -2):
            bad.append(f"{label}: accepted descriptor stopped at validation: {rc} '{msg}'")
        if not ok and (rc != -2 or not msg.startswith(prefix + ":")):
            bad.append(f"{label}: want -2 '{prefix}: ...', got {rc} '{msg}'")
    env = {k: v for k, v in os.environ.items() if k not in ("ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES")}
    env["HIP_VISIBLE_DEVICES"] = "-1"
    calls = [[_size_desc(f), _SIZE_QUERIES[q]] for _, _, _, f, _, q in _SIZE_CASES if q in _SIZE_QUERIES]
    p = subprocess.run([sys.executable, "-c", _SIZE_CHILD, ROOT, json.dumps(calls)], capture_output=True, text=True, env=env,
                       timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    answers = iter(json.loads(p.stdout.strip().splitlines()[-1]))
    for label, _, _, f, ok, q in _SIZE_CASES:
        if q in _SIZE_QUERIES:
            for name, v in next(answers).items():
                if (v != 0) != ok:
                    bad.append(f"{label}: {name} answers {v}, the entry point {'accepts' if ok else 'refuses'}")
    assert not bad, "\n".join(bad)

    # routing: the family named for each case's extents takes them
    def d(label):
        return _size_desc(next(f for l_, _, _, f, _, _ in _SIZE_CASES if l_ == label))

    for label, want in (("wf plane 4x2048x2048", "wf"), ("wf plane 8x1024x2048", "wf")):
        e = d(label)
        assert routing.conv3_family(e["B"], e["Cin"], e["Cout"], e["N"], e["H"], e["W"]) == want, label
    for label in ("wf plane 4x2048x2052", "wf plane 8x1024x2052"):
        e = d(label)
        assert routing.wf_route(e["B"], e["Cin"], e["Cout"], e["N"], e["H"], e["W"]) == (False, 1), label
        assert routing.conv3_family(e["B"], e["Cin"], e["Cout"], e["N"], e["H"], e["W"]) == "staged", label
    # the issue's shapes: plane 2^25 at 32 -> 32 channels falls through to the staged kernel, which takes it
    assert routing.wf_route(1, 32, 32, 8, 2048, 2048) == (False, 1)
    assert routing.conv3_family(1, 32, 32, 8, 2048, 2048) == "staged"
    e = d("wf pair (Cin+2) plane = 2^29")
    assert not routing.wf_route(e["B"], 62, 64, 8, e["H"], 8)[0] and routing.wf_route(e["B"], 62, 64, 8, e["H"] - 1, 8)[0]
    # a prologue pass of B * Cin > 65535 rows: conv3d_wf takes the plain input, not the one with a prologue
    assert routing.conv3_family(1024, 64, 64, 8, 16, 16, plain=True) == "wf"
    assert routing.conv3_family(1024, 64, 64, 8, 16, 16, plain=False) == "fused"
    assert routing.conv3_family(1023, 64, 64, 8, 16, 16, plain=False) == "wf"
    # staged: past its plane limit or prologue grid, the direct route is the fused kernel
    assert routing.direct_family(4, 32, extents=(1, 8, 4096, 8191)) == "staged"
    assert routing.direct_family(4, 32, extents=(1, 8, 4096, 8192)) == "fused"
    assert routing.direct_family(64, 64, plain=False, keep_xp=True, extents=(1023, 8, 16, 16)) == "staged"
    assert routing.direct_family(64, 64, plain=False, keep_xp=True, extents=(1024, 8, 16, 16)) == "fused"
    assert routing.direct_family(64, 64, plain=True, extents=(1024, 8, 16, 16)) == "staged"
    # composed Conv_0 + LL: the direct composed kernel up to its limit, then convolution + DWT; conv3d_wf's composed mode
    assert routing.ll_family(2, 64, 64, 8, 1024, 2046, producer_s2d=False) == "ll" and routing.ll_fits(2, 64, 64, 8, 1024, 2046)
    assert routing.ll_family(2, 64, 64, 8, 1024, 2048, producer_s2d=False) is None
    assert routing.wfll_route(2, 1, 64, 4, 4096, 4096) and not routing.wfll_route(2, 1, 64, 4, 4096, 4104)
    # the transform-pass Winograd kernel: planes 0 past any of its limits
    for label, ok in (("wino plane 2x2048x2048", True), ("wino plane 2x2048x2052", False), ("wino input < 2^30", True),
                      ("wino input = 2^30", False), ("wino B*Cin 65472", True), ("wino B*Cin 65536", False)):
        e = d(label)
        assert bool(routing.wino_plan(e["B"], e["Cout"], e["N"], e["H"], e["W"], cin=e["Cin"])[0]) == ok, label
    assert routing.conv3_family(1024, 64, 64, 12, 64, 64) not in ("wino4", "wino2")      # B * Cin > 65535
    assert routing.conv3_family(1023, 64, 64, 12, 64, 64) == "wino4"
    # the side x' of the 1x1x1 bandwidth kernel: its two limits
    assert routing.k1_side_xp(1, (64,), 64, 4, 2048, 2044) and not routing.k1_side_xp(1, (64,), 64, 4, 2048, 2048)
    assert not routing.k1_side_xp(1, (16,), 64, 8, 4096, 4096)
    # a folded res_conv: the limit of its rc_x offsets
    assert routing.wf_fold_fits(2, 64, 64, 4, 2048, 2044, 64) and not routing.wf_fold_fits(2, 64, 64, 4, 2048, 2048, 64)
    assert routing.wf_fold_fits(2, 64, 64, 4, 2048, 2048, 32)


def test_network_routes_respect_size_limits():
    """WavBEST's own decisions at a plane past the composed-LL and folded-res_conv limits: no LL composition (Conv_0 runs and
    the DWT keeps the LL band) and no res_conv folded into conv3d_wf, while the same network folds / composes at a plane
    inside the limits."""
    from tmdiff_amd.Hyper_unet_general import WavBEST
    net = WavBEST(channels=[64, 128, 128, 128])
    P = {"bf16": set()}

    class X:         # a stand-in with the extents of a tensor (nothing is allocated)
        def __init__(self, *shape):
            self.shape = shape

    fold = lambda *shape: net._resblock_plan(P, "down1.conv20", [X(*shape)], True, True, want_ll=True, to_conv0=True).fold
    assert fold(1, 64, 4, 2048, 2044) and not fold(1, 64, 4, 2048, 2048)           # 64 x 2^24 = 2^30
    assert net.down1.down.Conv_0.in_channels == 128           # 128 x 2^23 = 2^30
    conv0 = lambda *shape: net._down_plan(P, "down1.down", shape, True, True, False, True).conv0
    assert conv0(1, 128, 8, 1024, 1022) == "ll" and conv0(1, 128, 8, 1024, 1024) is None
    # the same four facts asked of the rules themselves: functions of the extents, no network
    from tmdiff_amd import routing
    assert routing.fold_k1(1, 64, 128, 128, 4, 2048, 2044) and not routing.fold_k1(1, 64, 128, 128, 4, 2048, 2048)
    assert routing.ll_fits(1, 128, 128, 8, 1024, 1022) and not routing.ll_fits(1, 128, 128, 8, 1024, 1024)


def test_fusion_table_of_the_baseline_configs():
    """What the epilogues of the inference graph additionally do (tmdiff_amd.routing.unet_fusions), tabulated like the
    families: the table committed as profiles/fusion_table.txt is this code's (tools/routing_table.py --fusions), and the
    benchmark workload (B = 32, 8 bands, 64x64, widths 32-256) has no prologue pass left, its four three-segment res_conv
    launches write conv20's prologue output on the side, its three main-branch Conv_0 run composed with the LL band on
    conv3d_wf's composed mode from a space-to-depth second output, and 9 of its 19 1x1x1 launches remain (DESIGN.md section 1:
    "per step 19 -> 9 1x1x1 launches")."""
    import subprocess, sys
    from tmdiff_amd import ops, routing
    assert ops.config.as_dict() == ops.KernelConfig(env={}).as_dict(), "this table is that of the default switches"
    rows = {r.block: r for r in routing.unet_fusions(routing.FULL, 32, 8, 64, 64)}
    assert len(rows) == 25 and sum(r.passes for r in rows.values()) == 0
    for blk in ("up1.conv20", "up2.conv20", "up3.conv20", "final.conv20"):
        assert rows[blk].taken == ("side_xp",) and rows[blk].k1 == 1, rows[blk]
    for blk in ("down1", "down2", "down3"):
        assert "wfll" in rows[blk + ".down"].taken and "s2d" in rows[blk + ".conv20"].taken, (rows[blk + ".down"], rows[blk + ".conv20"])
    assert sum(r.k1 for r in rows.values()) == 9
    # every fusion is taken by some BASELINE case and declined by some
    seen = [set(t for r in routing.unet_fusions(ch, b, n, size, size, math) for t in r.taken)
            for _, ch, b, n, size, math in routing.BASELINE_CASES if math == "fp32"]
    every = {"fold", "side_xp", "emit_ll", "s2d", "wfll", "ll", "dwt"}
    assert set().union(*seen) == every and set.intersection(*seen) < every, seen
    path = os.path.join(ROOT, "profiles", "fusion_table.txt")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "routing_table.py"), "--fusions"], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr[-1000:]
    assert out.stdout == open(path).read(), "profiles/fusion_table.txt is stale: python tools/routing_table.py --fusions > " + path


def _model_fusions(net, b, n, size):
    """{block: fusions taken} of the plans a CPU WavBEST asks for (_resblock_plan / _down_plan: what _resblock / _down execute),
    on stand-ins with the extents of the tensors of one fp32 inference forward (no _prepare, nothing allocated)."""
    class X:
        def __init__(self, ch, k):
            self.shape = (b, ch, n, size >> k, size >> k)

    P, c, got = {"bf16": set()}, net.channels, {}
    fuse_c, fuse = net._producer_fuse(P)

    def resblock(name, seg_c, k, pre, emit, **kw):
        p = net._resblock_plan(P, name, [X(ch, k) for ch in seg_c], bool(pre), bool(emit), **kw)
        got[name] = tuple(f for f in ("fold", "side_xp", "emit_ll", "s2d") if getattr(p, f))
        return p.s2d

    for branch in ("_1", ""):
        for k in range(3):
            blk = f"down{k + 1}{branch}"
            s2d = resblock(blk + ".conv20", [c[k]], k, fuse_c, fuse_c, want_ll=True, to_conv0=not branch)
            p = net._down_plan(P, blk + ".down", X(c[k + 1], k).shape, not branch, bool(fuse_c), s2d, fuse)
            got[blk + ".down"] = tuple(t for t in (p.conv0, "fold" if p.fold else None) if t)
    resblock("middle1", [c[3]], 3, fuse_c, False)
    for k, upn in ((3, "up1"), (2, "up2"), (1, "up3")):
        resblock(upn + ".conv20", [c[k]] * 3, k, False, fuse_c)
    resblock("final.conv20", [c[0]] * 3, 0, False, fuse_c)
    for k in (1, 2, 3):
        resblock(f"final.conv2{k}", [c[0]], 0, fuse_c, fuse_c and k < 3)
    return got


@pytest.mark.parametrize("channels,b,n,size,switches", [
    ([32, 64, 128, 256], 32, 8, 64, {}),                          # the benchmark workload (a BASELINE width)
    ([16, 32, 64, 128], 32, 8, 64, {}),                           # the reference's default widths: 16 channels fold / emit nothing
    ([32, 64, 128, 128], 4, 8, 64, {"wino_min_blocks": 1}),       # the small case of tests/test_gpu_configs.py's fusion test
    ([32, 64, 128, 256], 32, 4, 64, {"emit_dwt": False, "wfll": False}),
])
def test_model_decisions_equal_the_fusion_rows(channels, b, n, size, switches):
    """The block walk and the channel bookkeeping of routing.unet_fusions against the real module tree: what a CPU WavBEST
    plans for every ResBlock and every down block (through the entry _resblock / _down use, which reads the channel counts off
    its modules) is that block's row."""
    from tmdiff_amd import ops, routing
    from tmdiff_amd.Hyper_unet_general import WavBEST
    net = WavBEST(channels=channels)
    with ops.config.override(**switches):
        got = _model_fusions(net, b, n, size)
        rows = {r.block: r.taken for r in routing.unet_fusions(channels, b, n, size, size) if r.kind in ("resblock", "down")}
    assert got == rows
    assert any(got.values())


# ---- the finetune graph: plans, launches, table ------------------------------------------------------------------------
def test_train_routing_table_is_the_committed_one():
    """The launches of the finetune step (tmdiff_amd.routing.unet_train_launches), tabulated without a GPU: the table
    committed as profiles/train_routing_table.txt is this code's (tools/routing_table.py --train).  The configs[3] step
    (B = 8, 8 bands, 64x64, widths 32-256) runs its three main-branch Conv_0 composed with the LL band on conv3d_wf, every 3x3x3
    weight gradient (51) in the Winograd domain and the 19 1x1x1 ones on the direct kernel; the small 8-band network that
    tests/test_gpu_configs.py counts launch by launch still reaches every family (conv3d_wf with a pair-mode layer at its 8x8
    level, a direct forward family, a composed Conv_0 + LL, both weight-gradient kernels)."""
    import subprocess, sys
    from tmdiff_amd import ops, routing
    assert ops.config.as_dict() == ops.KernelConfig(env={}).as_dict(), "this table is that of the default switches"
    c3 = routing.unet_train_launches(routing.FULL, 8, 8, 64, 64)
    assert len(c3.convs) == 51 + 19 and sum(c3.counts.values()) == 3 * 70
    assert c3.counts["conv3d_wfll_fwd"] == 3 and c3.counts["conv3d_wgrad_wino"] == 51 and c3.counts["conv3d_wgrad"] == 19
    assert c3.counts["conv3d_fwd_k1"] == 2 * 19
    label, ch, b, n, size, switches = routing.TRAIN_CASES[2]
    assert n == 8 and "train_ll_wino" not in switches, label
    with ops.config.override(**switches):
        for dropout in (False, True):
            r = routing.unet_train_launches(ch, b, n, size, size, dropout)
            assert r.counts["conv3d_wf_fwd"] and r.counts["conv3d_wgrad_wino"] and r.counts["conv3d_wgrad"], r.counts
            assert r.counts.get("conv3d_fwd_staged") or r.counts.get("conv3d_fwd"), r.counts
            assert r.counts.get("conv3d_wfll_fwd") or r.counts.get("conv3d_ll_fwd"), r.counts
            assert any("wf_pair" in (c.fwd, c.dgrad) and (c.h, c.w) == (8, 8) for c in r.convs)
        assert any(c.keep_xp and c.fwd in ("wf", "wf_pair") for c in r.convs)
    # (x' kept by the staged kernel's pass: the narrow networks, on the direct kernels under the default switches)
    assert any(c.keep_xp and c.fwd == "staged" for c in routing.unet_train_launches([4, 8, 16, 32], 2, 8, 16, 16, True).convs)
    # the inference table's configs[3] row says what it is
    assert "inference graph" in [c[0] for c in routing.BASELINE_CASES if c[0].startswith("configs[3]")][0]
    path = os.path.join(ROOT, "profiles", "train_routing_table.txt")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "routing_table.py"), "--train"], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr[-1000:]
    assert out.stdout == open(path).read(), "profiles/train_routing_table.txt is stale: python tools/routing_table.py --train > " + path


def _model_train_plans(net, b, n, size, dropout):
    """({convolution: plan}, {block: plan}) a CPU WavBEST asks for in one forward_train: its blocks' train_plan (what their `run`
    executes) and autograd.conv_plan / routing.train_ll_plan (what _conv_forward / _ConvLL execute) with the weight shapes and
    groups of its own modules, on stand-ins with the extents of the tensors (nothing allocated)."""
    from torch import nn
    from tmdiff_amd import autograd as A, routing

    class X:
        def __init__(self, ch, k):
            self.shape = (b, ch, n, size >> k, size >> k)

    c, convs, blocks = net.channels, {}, {}
    drop = A.DropSpec(1, 0.2) if dropout else None

    def conv(name, segs, prologue=False, mask=None):
        m = net.get_submodule(name)
        convs[name] = tuple(A.conv_plan(segs, m.weight.shape, m.groups, prologue, mask, True))

    def resblock(name, seg_c, k):
        rb, segs = net.get_submodule(name), [X(ch, k) for ch in seg_c]
        blocks[name] = rb.train_plan(segs)
        conv(name + ".conv20", segs, True, drop)
        if isinstance(rb.res_conv, nn.Conv3d):
            conv(name + ".res_conv", segs)
        conv(name + ".conv21", [X(rb.conv20.out_channels, k)], True, drop)

    def wavelet(name, k, want_high=True):
        m = net.get_submodule(name)
        x = X(m.in_ch, k)
        p = m.train_plan(x, want_high)
        if m.down:
            blocks[name] = p
        if p.conv0:
            ll = routing.train_ll_plan(b, m.Conv_0.in_channels, m.Conv_0.out_channels, *x.shape[2:])
            convs[name + ".Conv_0"] = (ll.fwd, True, ll.dgrad, ll.wgrad, False)
        else:
            conv(name + ".Conv_0", [x], True)
        conv(name + ".Conv_2", [X(m.in_ch, k + 1 if p.conv2_after_ll else k)])
        if m.up:
            conv(name + ".convH_0.0", [X(m.convH_0[0].in_channels // 3, k)] * 3)
        conv(name + ".Conv_1", [X(m.in_ch, k + 1 if m.down else k - 1)], True, drop)

    for branch in ("_1", ""):
        conv(("conv1" if branch else "conv2") + ".conv21", [X(c[0], 0)], True)
        for k in range(3):
            resblock(f"down{k + 1}{branch}.conv20", [c[k]], k)
            wavelet(f"down{k + 1}{branch}.down", k, want_high=bool(branch))
    resblock("middle1", [c[3]], 3)
    for k, upn in ((3, "up1"), (2, "up2"), (1, "up3")):
        resblock(upn + ".conv20", [c[k]] * 3, k)
        wavelet(upn + ".up1", k)
    resblock("final.conv20", [c[0]] * 3, 0)
    for k in (1, 2, 3):
        resblock(f"final.conv2{k}", [c[0]], 0)
    return convs, blocks


@pytest.mark.parametrize("channels,b,n,size,switches", [
    ([32, 64, 128, 256], 8, 8, 64, {}),                                       # configs[3]
    ([16, 32, 64, 128], 8, 8, 64, {}),                                        # the reference's default widths
    ([16, 32, 64, 64], 2, 8, 64, {"wino_min_blocks": 1}),                     # the small cases of tests/test_gpu_configs.py
    ([16, 32, 64, 64], 2, 4, 128, {"wino_min_blocks": 1}),
    ([16, 32, 64, 64], 2, 8, 64, {"wino_min_blocks": 1, "train_ll_wino": False}),
    ([4, 8, 16, 32], 2, 8, 16, {}),
    ([32, 64, 128, 256], 8, 8, 64, {"wgrad_wino": False}),
    ([32, 64, 128, 256], 8, 8, 64, {"train_fused_resblock": False}),
    ([32, 64, 128, 256], 8, 8, 64, {"conv2_after_ll": False}),
    ([32, 64, 128, 256], 8, 8, 64, {"wgrad_bias": True, "ll_compose": False}),
])
def test_model_train_plans_equal_the_train_rows(channels, b, n, size, switches):
    """The block walk and the channel bookkeeping of routing.unet_train_launches against the real module tree, dropout off and
    on: every convolution's plan and every block's plan, asked through the entries the finetune graph itself uses, is that
    convolution's / block's row."""
    from tmdiff_amd import ops, routing
    from tmdiff_amd.Hyper_unet_general import WavBEST
    net = WavBEST(channels=channels)
    with ops.config.override(**switches):
        for dropout in (False, True):
            convs, blocks = _model_train_plans(net, b, n, size, dropout)
            r = routing.unet_train_launches(channels, b, n, size, size, dropout)
            assert convs == {c.name: tuple(c[7:]) for c in r.convs}
            assert blocks == dict(r.blocks)
            for c in r.convs:           # ... and the module tree's own extents
                m = net.get_submodule(c.name)
                assert (m.in_channels, m.out_channels, m.groups, m.kernel_size[0]) == (c.cin, c.cout, c.groups, c.ksize), c
        nodes = set(p for p in blocks.values() if isinstance(p, str))
    assert nodes == ({"separate"} if switches.get("train_fused_resblock") is False else {"rc", "id"})
    assert all(p.conv2_after_ll == switches.get("conv2_after_ll", True) for p in blocks.values() if not isinstance(p, str))


def test_train_predicates_agree_with_the_rules_they_came_from():
    """One statement per rule: routing.staged_weight_ok is the shape half of direct_family's "staged" on every (cin, cout, groups)
    of every layer of the tabulated cases (a plain input always wants the staged kernel, so the family IS the predicate), and
    ops.wgrad_wino_takes / ops.conv3d_wgrad answer from routing.wgrad_family, which is the library's own query."""
    import ctypes as C
    from tmdiff_amd import _lib, ops, routing
    seen = set()
    for _, ch, b, n, size, _ in routing.BASELINE_CASES + routing.OTHER_CASES:
        for L in routing.unet_conv3_layers(ch, size, size):
            seen.add((L.cin, L.cout, L.groups))
            assert (routing.direct_family(L.cin, L.cout, L.groups) == "staged") == routing.staged_weight_ok(L.cout, L.cin, L.groups), L
            assert (routing.direct_family(L.cin, L.cout, L.groups, plain=False, keep_xp=True) == "staged") == \
                routing.staged_weight_ok(L.cout, L.cin, L.groups), L
    assert {routing.staged_weight_ok(co, ci, g) for ci, co, g in seen} == {True, False}
    d = _lib.Conv3dDesc()
    d.B, d.N, d.H, d.W, d.Cin, d.Cout, d.groups, d.ksize, d.nseg = 8, 8, 64, 64, 64, 64, 1, 3, 1
    d.seg_c[0] = 64
    cases = [d]
    for field, bad in (("N", 6), ("W", 62), ("ksize", 1), ("groups", 2), ("in_act", 1)):
        e = _lib.Conv3dDesc.from_buffer_copy(d)
        setattr(e, field, bad)
        cases.append(e)
    e = _lib.Conv3dDesc.from_buffer_copy(d)         # three segments, as the up path's conv20
    e.Cin, e.nseg = 192, 3
    e.seg_c[0] = e.seg_c[1] = e.seg_c[2] = 64
    cases.append(e)
    for e in cases:
        fam = routing.wgrad_family(e.B, tuple(e.seg_c[:e.nseg]), e.Cout, e.N, e.H, e.W, e.groups, e.ksize, bool(e.in_act))
        lib_says = bool(e.ksize == 3 and _lib.lib.tmdiff_conv3d_wgrad_wino_supported(C.byref(e)))
        assert ops.wgrad_wino_takes(e) == (fam == "wino") == lib_says, (e.N, e.W, e.ksize, e.groups, e.nseg)
    assert ops.wgrad_wino_takes(d) and [ops.wgrad_wino_takes(e) for e in cases[1:5]] == [False] * 4
    with ops.config.override(wgrad_wino=False):
        assert not ops.wgrad_wino_takes(d) and routing.wgrad_family(8, (64,), 64, 8, 64, 64) == "direct"


@pytest.mark.parametrize("channels,b,n,size,switches", [
    ([32, 64, 128, 256], 8, 8, 64, {}),                                       # configs[3]
    ([16, 32, 64, 128], 8, 8, 64, {}),                                        # the reference's default widths
    ([16, 32, 64, 64], 2, 4, 128, {"wino_min_blocks": 1}),                    # a small case of tests/test_gpu_configs.py
])
@pytest.mark.parametrize("wgrad_wino", [True, False])
def test_plan_wgrad_family_is_what_conv3d_wgrad_would_ask_for(channels, b, n, size, switches, wgrad_wino):
    """autograd passes plan.wgrad to ops.conv3d_wgrad(family=) instead of letting it ask routing again: on every row of
    routing.unet_train_launches' convolution table the two answers are the same.  The descriptor is the one _conv_backward /
    _ConvLL.backward hand to ops.conv3d_wgrad: the forward's segments with its prologue, or -- plan.keep_xp, _ConvLL -- the kept x'
    as one plain segment.  (Pointers are placeholders: routing reads which fields are set, nothing is dereferenced.)"""
    import collections
    from tmdiff_amd import _lib, ops, routing

    def desc(seg_c, cout, h, w, groups, ksize, prologue=False, dropout=False):
        d = _lib.Conv3dDesc()
        d.B, d.N, d.H, d.W, d.Cin, d.Cout, d.groups, d.ksize, d.nseg = b, n, h, w, sum(seg_c), cout, groups, ksize, len(seg_c)
        for i, c in enumerate(seg_c):
            d.seg_c[i], d.seg_x[i] = c, 64
        if prologue:
            d.in_act, d.in_shift = 1, 64
        if dropout:
            d.drop_seed, d.drop_p = 1, 0.2
        return d

    asked = []          # (plan.wgrad, the weight gradient's descriptor) of every plan the table asks for
    conv_plan, ll_plan = routing.train_conv_plan, routing.train_ll_plan

    def train_conv_plan(b_, seg_c, cout, n_, h, w, groups=1, ksize=3, prologue=False, masked=False, dropout=False, need_w=True):
        p = conv_plan(b_, seg_c, cout, n_, h, w, groups, ksize, prologue, masked, dropout, need_w)
        kept = desc((sum(seg_c),), cout, h, w, groups, ksize)
        asked.append((p.wgrad, kept if p.keep_xp else desc(seg_c, cout, h, w, groups, ksize, prologue, dropout)))
        return p

    def train_ll_plan(b_, cin, cout, n_, h, w):
        p = ll_plan(b_, cin, cout, n_, h, w)
        asked.append((p.wgrad, desc((cin,), cout, h, w, 1, 3)))
        return p

    with ops.config.override(wgrad_wino=wgrad_wino, **switches):
        for dropout in (False, True):
            del asked[:]
            routing.train_conv_plan, routing.train_ll_plan = train_conv_plan, train_ll_plan
            try:
                rows = routing.unet_train_launches(channels, b, n, size, size, dropout).convs
            finally:
                routing.train_conv_plan, routing.train_ll_plan = conv_plan, ll_plan
            lls = sum(r.fwd in ("ll", "wfll") for r in rows)
            # every row has asked for its plan here (a down block may ask for its Conv_0 + LL plan twice: block and row)
            assert len(asked) >= len(rows) and lls > 0 and collections.Counter(r.wgrad for r in rows) <= collections.Counter(f for f, _ in asked)
            for fam, d in asked:
                assert fam == ("wino" if ops.wgrad_wino_takes(d) else "direct"), (fam, d.Cin, d.Cout, d.H, d.W, d.ksize, d.nseg)
            if wgrad_wino:
                assert {f for f, _ in asked} == {"wino", "direct"}      # both kernels are in the table (1x1x1 rows are direct)
            else:
                assert {f for f, _ in asked} == {"direct"}


def test_wgrad_split_choice_through_the_workspace_queries():
    """choose_splits (csrc/common.h) behind plan_wgrad and ww_plan, seen through tmdiff_conv3d_wgrad_workspace_bytes and
    tmdiff_conv3d_wgrad_wino_workspace_bytes: the partial-sum area is `splits` slots, so the byte counts pin the split count.
    One box in all, a prime number of boxes (7, 13), more than 256 (co, ci) tiles, more boxes than the split maximum, groups 3,
    ragged extents, a 1x1x1 weight and a prologue (x' in the workspace).  The integers are those of the build before the split
    search became one function; 0 = the Winograd kernel does not take the shape."""
    import ctypes as C
    from tmdiff_amd import _lib
    L = _lib.lib
    want = {    # (B, Cin, Cout, N, H, W, groups, ksize, in_act): (direct bytes, Winograd bytes)
        (1, 8, 8, 2, 8, 8, 1, 3, 0): (6944, 0),
        (1, 8, 8, 4, 8, 8, 1, 3, 0): (13888, 348160),
        (1, 32, 32, 2, 8, 56, 1, 3, 0): (775040, 0),
        (1, 32, 32, 4, 8, 104, 1, 3, 0): (2878720, 3113984),
        (13, 16, 16, 4, 8, 8, 1, 3, 0): (720512, 4526080),
        (1, 544, 544, 4, 8, 8, 1, 3, 0): (63926528, 66080768),
        (2, 544, 544, 2, 16, 16, 1, 1, 0): (4743680, 0),
        (8, 64, 64, 8, 64, 64, 1, 3, 0): (28327936, 226557952),
        (2, 96, 96, 8, 16, 16, 3, 3, 0): (10629120, 10678272),
        (3, 24, 40, 5, 12, 20, 1, 3, 0): (5607360, 0),
        (32, 32, 32, 8, 64, 64, 1, 3, 0): (28344320, 434094080),
        (1, 64, 64, 4, 8, 16, 1, 3, 1): (1901568, 1490944),
        (4, 256, 256, 8, 8, 8, 1, 3, 0): (28315648, 22282240),
    }
    for case, bytes_ in want.items():
        d = _lib.Conv3dDesc()
        d.B, d.Cin, d.Cout, d.N, d.H, d.W, d.groups, d.ksize, d.in_act = case
        d.nseg, d.seg_c[0] = 1, case[1]
        got = (L.tmdiff_conv3d_wgrad_workspace_bytes(C.byref(d)), L.tmdiff_conv3d_wgrad_wino_workspace_bytes(C.byref(d)))
        assert got == bytes_, (case, got, bytes_)
