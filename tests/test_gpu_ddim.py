"""-m gpu: the DDIM sampler on the HIP path (ddim_step_kernel, mh_ddim_step, mh_ddim_sample_loop, SpacedDiffusionHIP.ddim_sample /
ddim_sample_loop, DiffusionPipelineHIP(sampler="ddim")) vs the CPU restatement mh_testing/ddim.py and the reference's recorded
run tests/golden/ddim_xs.npz (tools/make_ddim_golden.py: DiT-XS, "ddim20", eta 0 and 1).

Tolerances.  One step: 2e-4 abs on sample and pred_xstart, the project's gate for one denoiser pass + one update (fp32
everywhere).  The step kernel alone against the restatement on the same inputs: every operation is the same fp32 operation in
the same order with contraction off, only the division may differ in its last ulps: rtol 1e-6 + atol 2e-6 (4 ulp at the
clamp range).
The 20-step loop: measured on the CPU, the restatement around oracle/dit.py's denoiser against the reference's loop with the
same injected draws ends max abs 0.518 (eta 0) / 1.082 (eta 1) away, with the in-paint denoised_fn 0.718 / 1.236 (median 0 /
9e-3: this random denoiser sends about half of the x0 predictions into the clamp and the trajectory amplifies fp32 rounding
at the other points; tests/test_ddim_cpu.py prints the figures).  That is not 10 x below the project's 5e-2 end-to-end bound,
so the device loop is gated at 10 x the CPU figure of its case -- a bound wider than the clamp range: it catches a
non-finite or unclamped result and nothing finer.  The parity gates are the per-step walk along the restatement's trajectory
(2e-4 at each of the 20 steps, both etas) and, for the graph form, its agreement with the step form on the device (1e-5: the
same kernels on the same inputs)."""
import json
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

ETAS = (0.0, 1.0)
# CPU restatement vs reference over the 20-step loop, max abs (tools/make_ddim_golden.py / tests/test_ddim_cpu.py)
CPU_LOOP_DISTANCE = {("plain", 0.0): 0.518, ("plain", 1.0): 1.082, ("inpaint", 0.0): 0.718, ("inpaint", 1.0): 1.236}


@pytest.fixture(scope="module")
def case():
    from mapperatorinator_amd.dit import DiTHIP, create_diffusion
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
    mask = odit.band_mask(T, 128)
    cs = types.SimpleNamespace(g=g, dit=DiTHIP(sd, depth, hidden, heads, device="cuda"), orc=odit.DiTOracle(sd, depth, hidden, heads),
                               od=DDIMOracle(n), z=z, c=c, y=y, mask=mask, cfg=float(g["cfg_scale"]), noise=noise, n=n,
                               diff=create_diffusion(str(g["respacing"]), noise_schedule="squaredcos_cap_v2", diffusion_steps=1000))
    cs.kw = dict(c=c.cuda(), y=y.cuda(), cfg_scale=cs.cfg, attn_mask=mask, key_padding_mask=None)
    cs.imask = torch.ones_like(z, dtype=torch.bool)
    cs.imask[:, :, :int(g["frozen"])] = False
    return cs


@pytest.mark.parametrize("N,T", [(2, 72), (3, 100)])
@pytest.mark.parametrize("eta", ETAS)
def test_step_kernel_alone_vs_restatement(case, N, T, eta):
    """mh_ddim_step on random inputs, no denoiser: N * 2 * T is no multiple of the 256-thread block (two and three blocks, a
    ragged last one).  Plain, with the in-paint mask, the raw_pred / x0_override pair, at loop indices 19, 7, 1 and 0."""
    from mapperatorinator_amd import _lib
    lib, od = _lib.load(), case.od
    rng = np.random.default_rng(1000 + 10 * N + int(eta))
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))
    mo, x, nz, ref = f(N, 4, T), f(N, 2, T), f(N, 2, T), f(N, 2, T)
    imask = torch.from_numpy(rng.random((N, 2, T)) < 0.6)
    fn = lambda v: torch.where(imask, v, ref)
    tab = case.diff.ddim_coef_table(eta).cuda()
    d = lambda a: a.cuda().contiguous()
    mo_d, x_d, nz_d, ref_d, m8 = d(mo), d(x), d(nz), d(ref), d(imask.to(torch.uint8))
    s = torch.cuda.current_stream().cuda_stream
    worst = 0.0

    def close(got, want):
        nonlocal worst
        worst = max(worst, (got.cpu() - want).abs().max().item())
        torch.testing.assert_close(got.cpu(), want, rtol=1e-6, atol=2e-6)

    for i in (19, 7, 1, 0):
        coef = tab[i].contiguous()
        out, pred = torch.full_like(x_d, 7.0), torch.full_like(x_d, 7.0)
        _lib.check(lib.mh_ddim_step(mo_d.data_ptr(), x_d.data_ptr(), nz_d.data_ptr(), coef.data_ptr(), None, None, None, 0, N, T,
                                    out.data_ptr(), pred.data_ptr(), s), "mh_ddim_step")
        want, want0 = od.ddim_sample(mo, x, i, nz, eta)
        close(out, want), close(pred, want0)
        if i == 0:
            assert torch.equal(out, pred), "loop index 0 returns x0"
        _lib.check(lib.mh_ddim_step(mo_d.data_ptr(), x_d.data_ptr(), nz_d.data_ptr(), coef.data_ptr(), m8.data_ptr(), ref_d.data_ptr(),
                                    None, 0, N, T, out.data_ptr(), pred.data_ptr(), s), "mh_ddim_step")
        want, want0 = od.ddim_sample(mo, x, i, nz, eta, fn)
        close(out, want), close(pred, want0)
        # the two-call protocol: raw eps -> x0 out (x_out untouched), a transformed x0 back in
        out.fill_(7.0)
        raw = torch.empty_like(x_d)
        _lib.check(lib.mh_ddim_step(mo_d.data_ptr(), x_d.data_ptr(), nz_d.data_ptr(), coef.data_ptr(), None, None, None, 1, N, T,
                                    out.data_ptr(), raw.data_ptr(), s), "mh_ddim_step")
        close(raw, od.raw_xstart(mo, x, i))
        assert bool((out == 7.0).all())
        back = d(fn(raw.cpu()))
        _lib.check(lib.mh_ddim_step(mo_d.data_ptr(), x_d.data_ptr(), nz_d.data_ptr(), coef.data_ptr(), None, None, back.data_ptr(), 0,
                                    N, T, out.data_ptr(), None, s), "mh_ddim_step")
        close(out, od.ddim_sample(mo, x, i, nz, eta, x0_override=back.cpu())[0])
    print(f"ddim_step_kernel N={N} T={T} eta={eta}: max abs err vs restatement {worst:.3e}")


@pytest.mark.parametrize("eta", ETAS)
def test_single_steps_vs_reference_golden(case, eta):
    g = case.g
    for i in (11, 0):
        out = case.diff.ddim_sample(case.dit.forward_with_cfg, case.z.cuda(), torch.full((2,), i, dtype=torch.long), model_kwargs=case.kw,
                                    eta=eta, noise=case.noise[0])
        e1 = (out["sample"].cpu() - torch.from_numpy(g[f"ddim_sample_i{i}_eta{int(eta)}"])).abs().max().item()
        e2 = (out["pred_xstart"].cpu() - torch.from_numpy(g[f"ddim_sample_i{i}_x0_eta{int(eta)}"])).abs().max().item()
        print(f"eta {eta} loop index {i}: one ddim_sample vs reference: sample {e1:.3e} pred_xstart {e2:.3e}")
        assert e1 < 2e-4 and e2 < 2e-4


@pytest.mark.parametrize("eta", ETAS)
def test_every_step_along_the_restatement_trajectory(case, eta):
    """The parity gate: the restatement walks all 20 steps on the CPU; the device step from the same x is within 2e-4 at each."""
    traj = []
    case.od.sample_loop(case.orc, case.z, case.c, case.y, case.cfg, case.mask, case.noise, eta, trajectory=traj)
    errs = []
    for i, x, _, nz, x_next in traj:
        out = case.diff.ddim_sample(case.dit.forward_with_cfg, x.cuda(), torch.full((2,), i, dtype=torch.long), model_kwargs=case.kw,
                                    eta=eta, noise=nz)
        errs.append((out["sample"].cpu() - x_next).abs().max().item())
    print(f"eta {eta}: per-step max abs err along the restatement's trajectory, loop index 19..0:", " ".join(f"{e:.1e}" for e in errs))
    assert len(errs) == 20 and max(errs) < 2e-4


@pytest.mark.parametrize("eta", ETAS)
def test_full_loop_graph_vs_golden_step_form_and_inpaint(case, eta):
    from mapperatorinator_amd.dit import InpaintSpec
    g, z, zt, fwd, tag = case.g, case.z, case.z.cuda(), case.dit.forward_with_cfg, f"eta{int(eta)}"
    out = case.diff.ddim_sample_loop(fwd, z.shape, zt, model_kwargs=case.kw, eta=eta, step_noise=case.noise).cpu()
    e = (out - torch.from_numpy(g[f"loop_{tag}"])).abs()
    print(f"eta {eta}: 20-step loop vs reference: max abs {e.max().item():.3e} median {e.median().item():.3e} "
          f"p90 {e.flatten().quantile(0.9).item():.3e} (CPU restatement vs reference: max {CPU_LOOP_DISTANCE['plain', eta]})")
    assert torch.isfinite(out).all() and e.max().item() < 10 * CPU_LOOP_DISTANCE["plain", eta]
    assert torch.equal(zt.cpu(), z), "the caller's noise tensor is not written"
    # the replayed graph against the same 20 steps issued one by one
    x = zt
    for k, i in enumerate(reversed(range(case.n))):
        x = case.diff.ddim_sample(fwd, x, torch.full((2,), i, dtype=torch.long), model_kwargs=case.kw, eta=eta, noise=case.noise[k])["sample"]
    d = (out - x.cpu()).abs().max().item()
    print(f"eta {eta}: graph form vs step form {d:.3e}")
    assert d < 1e-5
    # in-paint (the pipeline's denoised_fn without sliders): the frozen points end on their reference positions, the others move
    spec = InpaintSpec(case.imask, z)
    out2 = case.diff.ddim_sample_loop(fwd, z.shape, zt, denoised_fn=spec, model_kwargs=case.kw, eta=eta, step_noise=case.noise).cpu()
    e2 = (out2 - torch.from_numpy(g[f"loop_inpaint_{tag}"])).abs().max().item()
    print(f"eta {eta}: in-paint loop vs reference: max abs {e2:.3e} (CPU restatement vs reference: {CPU_LOOP_DISTANCE['inpaint', eta]})")
    assert torch.isfinite(out2).all() and e2 < 10 * CPU_LOOP_DISTANCE["inpaint", eta]
    k = int(g["frozen"])
    assert (out2[:, :, :k] - z[:, :, :k]).abs().max().item() < 1e-4 and (out2[:, :, k:] - z[:, :, k:]).abs().mean().item() > 1e-3
    want = torch.from_numpy(g[f"loop_inpaint_{tag}"])
    assert (want[:, :, :k] - z[:, :, :k]).abs().max().item() < 1e-4
    # the generic python denoised_fn path (x0 round trip through the host) agrees with the fused in-paint path
    out3 = case.diff.ddim_sample_loop(fwd, z.shape, zt, denoised_fn=lambda v: spec(v), model_kwargs=case.kw, eta=eta,
                                      step_noise=case.noise).cpu()
    assert (out3 - out2).abs().max().item() < 1e-5


def pipeline_inputs():
    from mapperatorinator_amd.diffusion_pipeline import points_to_sequence
    from mapperatorinator_amd.dit import DiTHIP
    from mh_testing import DIT_PRESETS, random_dit_state_dict, synthetic_hit_objects
    g = np.load(f"{GOLDEN}/dit_pipeline.npz")
    c = json.loads(str(g["case"]))
    depth, hidden, heads = DIT_PRESETS[c["preset"]]
    dit = DiTHIP(random_dit_state_dict(depth, hidden, seed=c["weight_seed"]), depth, hidden, heads, device="cuda")
    x, y, times, dist, typ = synthetic_hit_objects(c["T"], c["point_seed"])
    seq_x, seq_o, seq_c = points_to_sequence(x, y, times, dist, typ)
    cv, ucv = torch.zeros(300), torch.zeros(300)
    cv[c["classes"]] = 1
    ucv[c["null_classes"]] = 1
    return g, c, dit, seq_x, seq_o, seq_c, cv, ucv


@pytest.mark.parametrize("eta", ETAS)
def test_slider_window_graph_form_equals_step_form(eta):
    """The first window of the pipeline fixture with its sliders: the graph's three launches per step (raw x0, mh_slider_project,
    the update from x0_override) against `ddim_sample` called 20 times with the same SliderInpaintSpec."""
    from mapperatorinator_amd.dit import BandMask, InpaintSpec, SliderInpaintSpec, create_diffusion
    from mh_testing import synthetic_sliders
    g, c, dit, seq_x, seq_o, seq_c, cv, ucv = pipeline_inputs()
    k = c["knobs"]
    start, end = 0, k["max_seq_len"]
    sliders = synthetic_sliders(c["T"], c["point_seed"] + 1)
    z = torch.cat([seq_x[None], seq_x[None]], 0)[:, :, start:end].contiguous().cuda()
    mask = torch.ones_like(z, dtype=torch.bool)
    mask[:, :, :k["overlap_buffer"]] = False
    spec = SliderInpaintSpec(mask, z, [sliders], start, end)
    assert spec.n_sliders >= 5
    kw = dict(c=torch.cat([seq_c[None], seq_c[None]], 0)[:, :, start:end].contiguous().cuda(), y=torch.stack([cv, ucv]).cuda(),
              cfg_scale=k["cfg_scale"], attn_mask=BandMask(end - start, k["seq_len"]), key_padding_mask=None)
    diff = create_diffusion("ddim20", noise_schedule="squaredcos_cap_v2", diffusion_steps=1000)
    noise = torch.from_numpy(np.random.default_rng(77).standard_normal((20, *z.shape)).astype(np.float32))
    x0 = spec(z)
    out = diff.ddim_sample_loop(dit.forward_with_cfg, z.shape, x0, denoised_fn=spec, model_kwargs=kw, eta=eta, step_noise=noise)
    x = x0
    for j, i in enumerate(reversed(range(20))):
        x = diff.ddim_sample(dit.forward_with_cfg, x, torch.full((2,), i, dtype=torch.long), denoised_fn=spec, model_kwargs=kw, eta=eta,
                             noise=noise[j])["sample"]
    d = (out - x).abs().max().item()
    print(f"eta {eta}: slider window, graph form vs step form {d:.3e}")
    assert torch.isfinite(out).all() and d < 1e-5
    # the projection acted: without it the slider ends land somewhere else
    plain = diff.ddim_sample_loop(dit.forward_with_cfg, z.shape, x0, denoised_fn=InpaintSpec(mask, z), model_kwargs=kw, eta=eta,
                                  step_noise=noise)
    ends = [s.end_index for s in sliders if s.end_index < end and max(s.seq_indices) < end]
    assert (out[0][:, ends] - plain[0][:, ends]).abs().max().item() > 1e-2


def test_determinism_at_eta_0_and_noise_at_eta_1(case):
    other = torch.from_numpy(np.random.default_rng(4242).standard_normal(tuple(case.noise.shape)).astype(np.float32))
    run = lambda eta, nz: case.diff.ddim_sample_loop(case.dit.forward_with_cfg, case.z.shape, case.z.cuda(), model_kwargs=case.kw, eta=eta,
                                                     step_noise=nz)
    assert torch.equal(run(0.0, case.noise), run(0.0, other))
    assert torch.equal(run(1.0, case.noise), run(1.0, case.noise))
    assert (run(1.0, case.noise) - run(1.0, other)).abs().max().item() > 1e-2


def test_rng_consumption_matches_reference_pattern(case):
    """Without injected noise a 20-step loop draws randn_like(x) 20 times from the global generator -- at eta = 0 too, where the
    reference draws and multiplies by sigma = 0 (gaussian_diffusion.py:601) -- in call order."""
    fwd, zt = case.dit.forward_with_cfg, case.z.cuda()
    for eta in ETAS:
        torch.manual_seed(123)
        a = case.diff.ddim_sample_loop(fwd, case.z.shape, zt, model_kwargs=case.kw, eta=eta)
        after_a = torch.randn_like(zt)
        torch.manual_seed(123)
        noise = torch.stack([torch.randn_like(zt) for _ in range(20)])
        after_20 = torch.randn_like(zt)
        assert torch.equal(after_a, after_20), "the loop must consume exactly 20 draws of x's shape"
        assert torch.equal(a, case.diff.ddim_sample_loop(fwd, case.z.shape, zt, model_kwargs=case.kw, eta=eta, step_noise=noise))
    # one step: one draw
    torch.manual_seed(5)
    case.diff.ddim_sample(fwd, zt, torch.full((2,), 3, dtype=torch.long), model_kwargs=case.kw)
    after = torch.randn_like(zt)
    torch.manual_seed(5)
    torch.randn_like(zt)
    assert torch.equal(after, torch.randn_like(zt))


@pytest.mark.parametrize("eta", ETAS)
def test_pipeline_sampler_option(eta):
    """DiffusionPipelineHIP(sampler="ddim") on the `short` window-pipeline inputs (3 overlapping windows, start / end time, 2 steps +
    1 refine step per window): finite positions of the golden's shape, bit-equal to the window loop of
    `generate_positions_batch` written out by hand over `ddim_sample_loop` (refine steps stay `p_sample` at t = 0);
    sampler="ddpm" is the default constructor's output bit for bit."""
    from mapperatorinator_amd.diffusion_pipeline import DiffusionPipelineHIP
    from mapperatorinator_amd.dit import BandMask, InpaintSpec, create_diffusion
    g, c, dit, seq_x, seq_o, seq_c, cv, ucv = pipeline_inputs()
    k = dict(c["knobs"], timesteps=[2] + [0] * 9, refine_iters=1)
    t0, t1 = float(g["start_time"]), float(g["end_time"])
    common = dict(timesteps=k["timesteps"], seq_len=k["seq_len"], max_seq_len=k["max_seq_len"], overlap_buffer=k["overlap_buffer"],
                  cfg_scale=k["cfg_scale"], refine_model=dit, refine_iters=k["refine_iters"], start_time=t0, end_time=t1)

    def source():
        rng = np.random.default_rng(c["noise_seed"] + 1)
        return lambda n, shape: torch.from_numpy(np.stack([rng.standard_normal(shape).astype(np.float32) for _ in range(n)]))

    run = lambda **kw: DiffusionPipelineHIP(dit, **common, **kw).generate_positions(seq_x, seq_o, seq_c, cv, ucv, noise_source=source())
    pos = run(sampler="ddim", ddim_eta=eta)
    assert pos.shape == (1, *g["positions_short"].shape) == (1, 2, c["T"]) and pos.device.type == "cpu" and torch.isfinite(pos).all()
    if eta == 0.0:
        default = run()
        assert torch.equal(run(sampler="ddpm"), default)
        assert (default[0] - torch.from_numpy(g["positions_short"])).abs().max().item() < 0.05      # and that is still the golden
        assert (pos - default).abs().max().item() > 1.0                                               # another sampler

    # the same windows by hand
    diff = create_diffusion(k["timesteps"], noise_schedule="squaredcos_cap_v2", diffusion_steps=1000)
    src, ob, T, W = source(), k["overlap_buffer"], c["T"], k["max_seq_len"]
    z = torch.cat([seq_x[None], seq_x[None]], 0).cuda()
    cc = torch.cat([seq_c[None], seq_c[None]], 0).cuda()
    y = torch.stack([cv, ucv]).cuda()
    full = z.clone()
    for i in range(0, T - ob * 2, W - ob * 2):
        end = min(i + W, T)
        if i > 0:
            full[:, :, i + ob:i + ob * 2] = z[:, :, i + ob:i + ob * 2]
        z_part = full[:, :, i:end].contiguous()
        mask = torch.full(z_part.shape, False, dtype=torch.bool, device="cuda")
        mask[:, :, (ob if i > 0 else 0):] = True
        o_part = seq_o[i:end].contiguous()
        mask[:, :, :int(torch.searchsorted(o_part, t0, right=False))] = False
        mask[:, :, int(torch.searchsorted(o_part, t1, right=True)):] = False
        assert bool(mask.any())
        spec = InpaintSpec(mask, z_part)
        kw = dict(c=cc[:, :, i:end].contiguous(), y=y, cfg_scale=k["cfg_scale"], attn_mask=BandMask(end - i, k["seq_len"]),
                  key_padding_mask=None)
        smp = diff.ddim_sample_loop(dit.forward_with_cfg, z_part.shape, spec(z_part), denoised_fn=spec, model_kwargs=kw, eta=eta,
                                    step_noise=src(diff.num_timesteps, tuple(z_part.shape)))
        smp = diff.p_sample(dit.forward_with_cfg, smp, torch.tensor([0, 0]), denoised_fn=spec, model_kwargs=kw,
                            noise=src(1, tuple(smp.shape))[0])["sample"]
        full[:, :, i:end] = smp
    want = ((full[:1] + 1) / 2 * torch.tensor([512.0, 384.0], device="cuda")[None, :, None]).cpu()
    assert torch.equal(pos, DiffusionPipelineHIP(dit, **common).to_positions(full)) and (pos - want).abs().max().item() < 1e-3
