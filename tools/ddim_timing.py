"""Sampler timing: B chunks (Tq = 128 points, CFG batch 2B) through the 100-step DDPM loop ("ddpm100") or through
`ddim_sample_loop` at "ddim50" / "ddim25", one replayed hipGraph each (the timer of tools/dit_one_chunk.py: median of 5 loops
after one warm loop).  One configuration per process.
    python tools/ddim_timing.py B preset ddpm100|ddim50|ddim25"""
import os, sys, time, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mapperatorinator_amd.dit import BandMask, DiTHIP, create_diffusion
from mh_testing import DIT_PRESETS, random_dit_state_dict, synthetic_dit_inputs
dev = torch.device("cuda", 0)
B, Tq = int(sys.argv[1]), 128
preset, sampler = sys.argv[2], sys.argv[3]
depth, hidden, heads = DIT_PRESETS[preset]
dit = DiTHIP(random_dit_state_dict(depth, hidden, seed=0), depth, hidden, heads, device=dev)
parts = [synthetic_dit_inputs(Tq, seed=b) for b in range(B)]
z, c, y = [torch.cat([p[j][:1] for p in parts] + [p[j][1:] for p in parts]).to(dev) for j in range(3)]
kw = dict(c=c, y=y, cfg_scale=1.0, attn_mask=BandMask(Tq, 128))
name = sampler[:4]
diff = create_diffusion([100] + [0] * 9 if sampler == "ddpm100" else sampler, noise_schedule="squaredcos_cap_v2", diffusion_steps=1000)
n = diff.num_timesteps
noise = torch.randn(n, *z.shape, device=dev)
loop = diff.p_sample_loop if name == "ddpm" else diff.ddim_sample_loop
run = lambda: loop(dit.forward_with_cfg, z.shape, z, model_kwargs=kw, step_noise=noise)
out = run(); torch.cuda.synchronize()
ts = []
for _ in range(5):
    t = time.perf_counter(); run(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t)
ms = sorted(ts)[2] * 1e3
print(f"{preset} B={B} {name} {n} steps: {ms:.2f} ms per loop, {ms / n * 1e3:.1f} us per step, finite {bool(torch.isfinite(out).all())}")
