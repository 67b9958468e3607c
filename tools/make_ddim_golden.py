"""Writes tests/golden/ddim_xs.npz: the reference's DDIM sampler (GaussianDiffusion.ddim_sample / ddim_sample_loop,
osu_diffusion/utils/diffusion/gaussian_diffusion.py:563-610, 653-735) on the seeded DiT-XS of tests/golden/dit_xs.npz.

The unmodified reference is imported through oracle/ref_harness.py (as oracle/make_golden.py does); its per-step gaussian draws
are injected by replacing `randn_like` for the duration of a call, the way oracle/make_golden.py does for the DDPM goldens.  The
replacement also reads the `sigma` the reference has just computed out of the calling frame, so the file records the
reference's own per-step sigma and not a restatement of it.  Respacing "ddim20" (stride 50 over 1000 steps), eta 0 and 1:
the respaced tables, one ddim_sample from x = z at loop index 11 and one at loop index 0, the 20-step loop, and the 20-step
loop with the pipeline's in-paint denoised_fn (first 17 points frozen).  Prints the distance of the CPU restatement
(mh_testing/ddim.py around oracle/dit.py's denoiser) to every recorded loop: the figure the loop tolerance of
tests/test_gpu_ddim.py is derived from.

    python tools/make_ddim_golden.py        (needs the reference checkout; run from the repository root)
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mh_testing import DIT_PRESETS, random_dit_state_dict, synthetic_dit_inputs  # noqa: E402
from mh_testing.ddim import DDIMOracle  # noqa: E402
from oracle import dit as odit  # noqa: E402
from oracle import ref_harness as rh  # noqa: E402

PRESET, T, WSEED, ISEED, CFG_SCALE, RESPACING, FROZEN = "DiT-XS", 96, 21, 5, 1.5, "ddim20", 17
OUT = os.path.join(ROOT, "tests", "golden", "ddim_xs.npz")


def main():
    import sys as _sys
    rh.ref_shims.install()
    from osu_diffusion import create_diffusion
    from osu_diffusion.utils.diffusion import gaussian_diffusion as gd
    from osu_diffusion.utils.models import DiT
    depth, hidden, heads = DIT_PRESETS[PRESET]
    sd = random_dit_state_dict(depth, hidden, seed=WSEED)
    ref = DiT(context_size=272, hidden_size=hidden, depth=depth, num_heads=heads, class_size=300).eval()
    ref.load_state_dict(sd, strict=True)
    z, c, y = synthetic_dit_inputs(T, seed=ISEED)
    mask = odit.band_mask(T, 128)
    diff = create_diffusion(timestep_respacing=RESPACING, diffusion_steps=1000, noise_schedule="squaredcos_cap_v2")
    n = diff.num_timesteps
    noise = torch.from_numpy(np.random.default_rng(600 + ISEED).standard_normal((n, *z.shape)).astype(np.float32))
    kw = dict(c=c, y=y, cfg_scale=CFG_SCALE, attn_mask=mask, key_padding_mask=None)
    imask = torch.ones_like(z, dtype=torch.bool)
    imask[:, :, :FROZEN] = False
    inpaint = lambda x0: torch.where(imask, x0, z)

    def with_draws(draws, fn):
        """run fn() with the reference's randn_like popping from `draws`; -> (result, the sigma of every call)"""
        pending, sigmas = list(draws), []

        def randn_like(v, *a, **k):
            sigmas.append(_sys._getframe(1).f_locals["sigma"].flatten()[0].item())     # ddim_sample's local, just computed
            return pending.pop(0).to(v)
        orig = gd.th.randn_like
        gd.th.randn_like = randn_like
        try:
            with torch.no_grad():
                return fn(), sigmas
        finally:
            gd.th.randn_like = orig

    orc, od = odit.DiTOracle(sd, depth, hidden, heads), DDIMOracle(n)
    assert od.timestep_map == list(diff.timestep_map)
    rec = dict(preset=PRESET, T=T, weight_seed=WSEED, input_seed=ISEED, cfg_scale=CFG_SCALE, respacing=RESPACING,
               noise_seed=600 + ISEED, frozen=FROZEN, timestep_map=np.array(diff.timestep_map),
               alphas_cumprod=diff.alphas_cumprod, alphas_cumprod_prev=diff.alphas_cumprod_prev)
    for eta in (0.0, 1.0):
        tag = f"eta{int(eta)}"
        for i in (11, 0):
            one, _ = with_draws([noise[0]], lambda: diff.ddim_sample(
                ref.forward_with_cfg, z, torch.full((2,), i, dtype=torch.long), clip_denoised=True, model_kwargs=kw, eta=eta))
            rec[f"ddim_sample_i{i}_{tag}"] = one["sample"].numpy()
            rec[f"ddim_sample_i{i}_x0_{tag}"] = one["pred_xstart"].numpy()
        loop = lambda fn: with_draws(noise, lambda: diff.ddim_sample_loop(
            ref.forward_with_cfg, z.shape, z, clip_denoised=True, denoised_fn=fn, model_kwargs=kw, device=z.device, eta=eta))
        full, sig = loop(None)
        rec[f"loop_{tag}"] = full.numpy()
        rec[f"sigma_{tag}"] = np.array(sig[::-1], dtype=np.float32)            # call order -> loop index
        part, _ = loop(inpaint)
        rec[f"loop_inpaint_{tag}"] = part.numpy()
        d0 = (od.sample_loop(orc, z, c, y, CFG_SCALE, mask, noise, eta) - full).abs().max().item()
        d1 = (od.sample_loop(orc, z, c, y, CFG_SCALE, mask, noise, eta, inpaint) - part).abs().max().item()
        print(f"eta {eta}: sample range {full.min().item():.3f} .. {full.max().item():.3f}; CPU restatement vs reference, "
              f"{n}-step loop max abs {d0:.3e}, in-paint loop {d1:.3e}")
    np.savez_compressed(OUT, **rec)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
