"""Beam search throughput (`num_beams = 2`: the reference's timing pass, super_timing_generator.py:28; cache reorder per step,
inference/cache_utils.py:16-20): G windows x 2 beams through mapperatorinator_amd.beam.beam_search on osuT5-base bf16.
Prints one JSON line: tokens/s of the returned hypotheses and ms per beam step.    python tools/beam_bench.py [--chunks 1] [--beams 2]
`--types-first`: the types_first processors with a lookback window (ConditionalTemperature + LookbackBiasLogitsWarper(types_first=True):
the step is mh_beam_step_tf); `--step-path 2`: the streaming kernel instead of the automatic choice (option "beam_step_path").
`--sample`: beam-sample (do_sample, top_p 0.95) instead -- three legs, ms per beam step each with every timed run listed: the draw
inside the step kernel (mh_beam_step_sample, `device_draw=True`), the torch-op bookkeeping drawing with torch.multinomial (what a
beam-sample call runs without the opt-in) and, beside them, the greedy step kernel."""
import argparse, json, os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run_sample(chunks=1, beams=2, new_tokens=128, device="cuda:0", model_tuple=None, repeats=4):
    """The three legs of `--sample`; the first run of a leg warms up and is not timed."""
    from mapperatorinator_amd.server import build_sampling
    from mh_testing import synthetic_audio_varied
    import importlib.util
    spec = importlib.util.spec_from_file_location("small_batch_decode", os.path.join(os.path.dirname(os.path.abspath(__file__)), "small_batch_decode.py"))
    sbd = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sbd)
    dev = torch.device(device)
    tgt = 1 + new_tokens
    model, tok, dims, frames = model_tuple or sbd.build("t5-base", tgt, dev)
    eng = model.engine
    audio = synthetic_audio_varied(chunks, (frames - 1) * 128, seed=5).to(dev)
    prompt = torch.full((chunks, 1), tok.sos_id, dtype=torch.long)
    gk = dict(num_beams=beams, max_length=tgt, temperature=1.0, context_type="map", pad_token_id=0)
    sp_s, _ = build_sampling(tok, dict(gk, do_sample=True, top_p=0.95, seed=1, seed_call_index=0), tgt)
    sp_g, _ = build_sampling(tok, dict(gk, do_sample=False), tgt)
    res = {}
    for name, sp, kw in (("kernel_draw", sp_s, dict(device_draw=True, use_kernel=True)), ("torch_op_multinomial", sp_s, {}),
                         ("greedy_kernel", sp_g, dict(use_kernel=True))):
        times = []
        for r in range(repeats + 1):
            torch.manual_seed(r)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            out = eng.generate_beam(audio, prompt, None, [], sp, beams, **kw)      # no EOS ids: every hypothesis runs to max_length
            torch.cuda.synchronize(dev)
            times.append(time.perf_counter() - t0)
        n = int(out["tokens"].shape[1]) - 1
        per_step = sorted(round(t * 1e3 / max(n, 1), 3) for t in times[1:])
        res[name] = {"ms_per_beam_step": per_step[0], "runs_ms_per_beam_step": per_step, "steps": n}
    res["workload"] = (f"osuT5-base bf16, {chunks} window(s) x {beams} beams: mel + encoder + beam search; kernel_draw = per token mh_t5_step -> "
                       "mh_beam_step_sample -> mh_t5_reorder_cache")
    return res


def run(chunks=1, beams=2, new_tokens=128, device="cuda:0", model_tuple=None, types_first=False):
    from mapperatorinator_amd.server import build_sampling
    from mh_testing import synthetic_audio_varied
    import importlib.util
    spec = importlib.util.spec_from_file_location("small_batch_decode", os.path.join(os.path.dirname(os.path.abspath(__file__)), "small_batch_decode.py"))
    sbd = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sbd)
    dev = torch.device(device)
    tgt = 1 + new_tokens
    model, tok, dims, frames = model_tuple or sbd.build("t5-base", tgt, dev)
    eng = model.engine
    audio = synthetic_audio_varied(chunks, (frames - 1) * 128, seed=5).to(dev)
    prompt = torch.full((chunks, 1), tok.sos_id, dtype=torch.long)
    gk = dict(do_sample=False, num_beams=beams, max_length=tgt, temperature=1.0, context_type="map", pad_token_id=0)
    if types_first:
        gk.update(types_first=True, timing_temperature=0.9, lookback_time=500)
    sp, eos = build_sampling(tok, gk, tgt)
    eos = []          # random-init weights: keep every hypothesis running to max_length
    res = {}
    outs = {}
    for name, uk in (("beam_step_kernel", None), ("torch_op_bookkeeping", False)):
        times = []
        for r in range(3):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            out = eng.generate_beam(audio, prompt, None, eos, sp, beams, use_kernel=uk)
            torch.cuda.synchronize(dev)
            times.append(time.perf_counter() - t0)
        dt = sorted(times[1:])[0]
        n = int(out["tokens"].shape[1]) - 1
        outs[name] = out["tokens"]
        res[name] = {"seconds": round(dt, 4), "ms_per_beam_step": round(dt * 1e3 / max(n, 1), 3), "tokens_per_s": round(chunks * n / dt, 1)}
    res["same_ids"] = bool(torch.equal(outs["beam_step_kernel"], outs["torch_op_bookkeeping"]))
    if types_first:      # a row renormalises after a timed event (the three reductions of the step run for every row either way)
        res["timed_ids_in_best_hypotheses"] = int(torch.from_numpy(sp.host_tok_flags & 1).bool()[outs["beam_step_kernel"][:, 1:-1]].sum())
    res["workload"] = (f"osuT5-base bf16, {chunks} window(s) x {beams} beams, {n} steps: mel + encoder + beam search (per token mh_t5_step -> "
                       "mh_beam_step -> mh_t5_reorder_cache; torch_op_bookkeeping = the ~40 ATen launches per token of round 5)")
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=1)
    ap.add_argument("--beams", type=int, default=2)
    ap.add_argument("--types-first", action="store_true")
    ap.add_argument("--step-path", type=int, default=0, choices=(0, 1, 2))
    ap.add_argument("--sample", action="store_true")
    a = ap.parse_args()
    from mapperatorinator_amd import _lib
    _lib.set_option("beam_step_path", a.step_path)
    if a.sample:
        print(json.dumps(dict(run_sample(a.chunks, a.beams), sample=True, step_path=a.step_path)))
        sys.exit(0)
    print(json.dumps(dict(run(a.chunks, a.beams, types_first=a.types_first), types_first=a.types_first, step_path=a.step_path)))
