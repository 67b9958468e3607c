"""No GPU: the host half of the DDIM sampler (SpacedDiffusionHIP.ddim_coef_table, the entry points' declarations and argument
checks, the refusals) and the CPU restatement mh_testing/ddim.py against the reference's recorded run
(tests/golden/ddim_xs.npz, tools/make_ddim_golden.py)."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
from mapperatorinator_amd import _lib
from mapperatorinator_amd.dit import DiTHIP, create_diffusion

ETAS = (0.0, 1.0)


@pytest.fixture(scope="module")
def case():
    from mh_testing import DIT_PRESETS, random_dit_state_dict, synthetic_dit_inputs
    from mh_testing.ddim import DDIMOracle
    from oracle import dit as odit
    g = np.load(f"{GOLDEN}/ddim_xs.npz")
    depth, hidden, heads = DIT_PRESETS[str(g["preset"])]
    sd = random_dit_state_dict(depth, hidden, seed=int(g["weight_seed"]))
    T = int(g["T"])
    z, c, y = synthetic_dit_inputs(T, seed=int(g["input_seed"]))
    n = len(g["timestep_map"])
    noise = torch.from_numpy(np.random.default_rng(int(g["noise_seed"])).standard_normal((n, *z.shape)).astype(np.float32))
    return types.SimpleNamespace(g=g, orc=odit.DiTOracle(sd, depth, hidden, heads), od=DDIMOracle(n), z=z, c=c, y=y,
                                 mask=odit.band_mask(T, 128), cfg=float(g["cfg_scale"]), noise=noise)


def diffusion(g):
    return create_diffusion(str(g["respacing"]), noise_schedule="squaredcos_cap_v2", diffusion_steps=1000)


@pytest.mark.parametrize("eta", ETAS)
def test_coef_table_equals_the_reference_tables(case, eta):
    """Every entry is what the reference multiplies by: the fp32-extracted tables exactly, sigma exactly as the reference's
    ddim_sample computed it, the two square roots as its fp32 tensor operations give them from those."""
    g = case.g
    diff = diffusion(g)
    assert diff.timestep_map == list(g["timestep_map"]) == list(range(0, 1000, 50))
    assert np.array_equal(diff.alphas_cumprod, g["alphas_cumprod"]) and np.array_equal(diff.alphas_cumprod_prev, g["alphas_cumprod_prev"])
    tab = diff.ddim_coef_table(eta)
    assert tab.dtype == torch.float32 and tab.shape == (20, 6) and bool(torch.isfinite(tab).all())
    ab, abp = torch.from_numpy(g["alphas_cumprod"]).float(), torch.from_numpy(g["alphas_cumprod_prev"]).float()
    sigma = torch.from_numpy(g[f"sigma_eta{int(eta)}"])
    assert torch.equal(tab[:, 0], torch.from_numpy(np.sqrt(1.0 / g["alphas_cumprod"])).float())
    assert torch.equal(tab[:, 1], torch.from_numpy(np.sqrt(1.0 / g["alphas_cumprod"] - 1)).float())
    assert torch.equal(tab[:, 2], torch.sqrt(abp))
    assert torch.equal(tab[:, 3], sigma)
    assert torch.equal(tab[:, 4], torch.sqrt(1 - abp - sigma ** 2))
    assert torch.equal(tab[:, 5], torch.tensor([0.0] + [1.0] * 19))
    # loop index 0: alpha_bar_prev = 1 -> no noise, no direction term: the last step returns x0
    assert tab[0, 2].item() == 1.0 and tab[0, 3].item() == 0.0 and tab[0, 4].item() == 0.0 and tab[0, 5].item() == 0.0
    assert bool((sigma[1:] > 0).all()) == (eta > 0) and bool((ab < 1).all())
    # the restatement's own schedule agrees with both
    assert case.od.timestep_map == diff.timestep_map
    assert np.array_equal(case.od.alphas_cumprod, g["alphas_cumprod"])
    assert all(case.od.sigma(i, eta).item() == sigma[i].item() for i in range(20))


@pytest.mark.parametrize("eta", ETAS)
def test_restatement_reproduces_the_reference_steps_and_loop_distance_is_recorded(case, eta):
    """One pass (loop indices 11 and 0, from x = z): 2e-5, the gate of the oracle pins for one denoiser pass.  The 20-step loops are
    printed, not gated: this random denoiser pushes about half of the x0 predictions into the clamp and the trajectory amplifies
    fp32 rounding; the two CPU implementations end 0.52 (eta 0) / 1.08 (eta 1) apart at their worst element (in-paint loops
    0.72 / 1.24), median 0 / 9e-3.  tests/test_gpu_ddim.py derives its loop bound from these figures."""
    g, tag = case.g, f"eta{int(eta)}"
    for i in (11, 0):
        t = torch.full((2,), case.od.timestep_map[i], dtype=torch.long)
        mo = case.orc.forward_with_cfg(case.z, t, case.c, case.y, case.cfg, case.mask)
        smp, x0 = case.od.ddim_sample(mo, case.z, i, case.noise[0], eta)
        e1 = (smp - torch.from_numpy(g[f"ddim_sample_i{i}_{tag}"])).abs().max().item()
        e2 = (x0 - torch.from_numpy(g[f"ddim_sample_i{i}_x0_{tag}"])).abs().max().item()
        print(f"eta {eta} loop index {i}: restatement vs reference, sample {e1:.3e} pred_xstart {e2:.3e}")
        assert e1 < 2e-5 and e2 < 2e-5
        if i == 0:
            assert torch.equal(smp, x0)
    imask = torch.ones_like(case.z, dtype=torch.bool)
    imask[:, :, :int(g["frozen"])] = False
    for key, fn in ((f"loop_{tag}", None), (f"loop_inpaint_{tag}", lambda v: torch.where(imask, v, case.z))):
        out = case.od.sample_loop(case.orc, case.z, case.c, case.y, case.cfg, case.mask, case.noise, eta, fn)
        err = (out - torch.from_numpy(g[key])).abs()
        print(f"{key}: restatement vs reference over 20 steps, max abs {err.max().item():.3e} median {err.median().item():.3e} "
              f"p90 {err.flatten().quantile(0.9).item():.3e}")
        assert bool(torch.isfinite(out).all())


def test_symbols_declared_bound_exported_and_abi_unchanged():
    hdr = open(os.path.join(ROOT, "include", "mapperhip.h")).read()
    declared = set(re.findall(r"\b(mh_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name in ("mh_ddim_step", "mh_ddim_sample_loop"):
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert _lib.SYMBOLS["mh_ddim_step"] == _lib.SYMBOLS["mh_ddpm_step"]
    assert _lib.SYMBOLS["mh_ddim_sample_loop"] == _lib.SYMBOLS["mh_ddpm_sample_loop"]
    assert re.search(r"#define MH_ABI_VERSION 11\b", hdr) and _lib.ABI_VERSION == 11 and lib.mh_abi_version() == 11
    assert "gaussian_diffusion.py:563-610" in hdr and "gaussian_diffusion.py:653-735" in hdr


def test_null_arguments_are_refused_before_the_device_is_touched():
    lib = _lib.load()
    assert lib.mh_ddim_step(None, None, None, None, None, None, None, 0, 2, 96, None, None, None) == -1
    assert b"mh_ddim_step" in lib.mh_last_error()
    buf = (C.c_float * 8)()
    p = C.addressof(buf)
    assert lib.mh_ddim_step(p, p, p, p, p, None, None, 0, 1, 1, p, None, None) == -1         # a mask without its reference
    assert b"mask/ref" in lib.mh_last_error()
    assert lib.mh_ddim_step(p, p, p, p, None, None, None, 1, 1, 1, p, None, None) == -1      # raw_pred with nowhere to write
    assert b"raw_pred" in lib.mh_last_error()
    assert lib.mh_ddim_step(p, p, p, p, None, None, None, 0, 0, 1, p, None, None) == -1
    dc = _lib.MhDiTConfig(128, 2, 2, 272, 300, 2, 128, 256, 544, 300)
    assert lib.mh_ddim_sample_loop(C.byref(dc), None, None, None, None, 1.0, 0, 0, 2, 96, 20, None, None, None, None, None, None,
                                   None, 0, None) == -1
    assert b"mh_ddim_sample_loop: null argument" in lib.mh_last_error()
    # the DDPM loop still names itself
    assert lib.mh_ddpm_sample_loop(C.byref(dc), None, None, None, None, 1.0, 0, 0, 2, 96, 20, None, None, None, None, None, None,
                                   None, 0, None) == -1
    assert b"mh_ddpm_sample_loop: null argument" in lib.mh_last_error()


def test_refusals():
    from mapperatorinator_amd.diffusion_pipeline import DiffusionPipelineHIP
    diff = create_diffusion("ddim20", noise_schedule="squaredcos_cap_v2", diffusion_steps=1000)
    dit = DiTHIP.__new__(DiTHIP)          # never reached: every refusal comes before the model is used
    x, t = torch.zeros(2, 2, 8), torch.zeros(2, dtype=torch.long)
    with pytest.raises(ValueError, match="eta"):
        diff.ddim_coef_table(-0.5)
    for kw, exc in ((dict(cond_fn=lambda *a: None), NotImplementedError), (dict(clip_denoised=False), NotImplementedError),
                    (dict(eta=-1.0), ValueError)):
        with pytest.raises(exc, match="cond_fn|eta"):
            diff.ddim_sample(dit, x, t, **kw)
        with pytest.raises(exc, match="cond_fn|eta"):
            diff.ddim_sample_loop(dit, x.shape, x, **kw)
    with pytest.raises(TypeError, match="ddim_sample_loop"):
        diff.ddim_sample_loop(lambda *a: None, x.shape, x)
    with pytest.raises(TypeError, match="ddim_sample:"):
        diff.ddim_sample(lambda *a: None, x, t)
    model = types.SimpleNamespace(device=torch.device("cpu"))
    with pytest.raises(ValueError, match="sampler"):
        DiffusionPipelineHIP(model, timesteps="ddim20", sampler="plms")
    with pytest.raises(ValueError, match="ddim_eta"):
        DiffusionPipelineHIP(model, timesteps="ddim20", sampler="ddim", ddim_eta=-1.0)
    pipe = DiffusionPipelineHIP(model, timesteps="ddim20")
    assert pipe.sampler == "ddpm" and pipe.ddim_eta == 0.0
    assert DiffusionPipelineHIP(model, timesteps="ddim20", sampler="ddim", ddim_eta=0.5).ddim_eta == 0.5
