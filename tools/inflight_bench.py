"""What in-flight slots (`SequentialWindowScheduler(inflight=True)`, `mh_t5_slots_*`) buy against waves, varwhisper-small bf16 on one GPU.

Workload, a CONSTRUCTED case (how ragged real windows are is not known): 32 songs whose window counts are spread over 6..18; the
new-token count of every window is drawn ONCE from a fixed seed, uniformly in 96..512, and forced through the window's own
`max_length` (= prompt + new) with the EOS sets EMPTIED (server.get_eos_token_id patched in this process), prompts of 2 ids.  A
song's first window has no lookback, its last no lookahead (the reference's `generate_sequential`).

Policies, alternating in one process, round 0 as warm-up, medians of --reps rounds:
  waves         the default: wave w = window w of every song, one call per kwargs group.  Every window has its own `max_length`
                here, so the groups are single windows: batch-1 calls.  (--waves-reps rounds only: it is by far the slowest.)
  merge_kwargs  wave w as ONE row-settings call of up to 32 rows: the call runs until its longest row has ended.
  inflight      32 slots kept full, `--steps` token steps between two looks at the slots.
  inflight_kv8_<mode>  (one per `--kv-fp8 cross|self|both` given) the same over the session's e4m3 K/V caches
                (`SequentialWindowScheduler(inflight_kv_fp8=<mode>)`, `mh_t5_slots_open_kv8`); `vs_inflight` = its wall time against
                plain in-flight.  `--only-inflight` leaves the two wave policies out; `--new-tokens LO HI` moves the drawn range (a
                workload of long windows: with `--tgt` large enough to hold them).
  --guided      the same constructed workload under classifier-free guidance: every window carries a negative prompt (sos alone) and
                cfg_scale = 2.  Two policies at the same `decode_batch` (--slots decode ROWS, so half as many windows): guided_merge_kwargs
                (guided waves, `merge_kwargs=True`: wave w in row-settings calls of slots / 2 pairs) against inflight_guided
                (`SequentialWindowScheduler(inflight=True, inflight_guided=True)`, `mh_t5_slots_open_guided`: slots / 2 pair slots kept
                full).  `ideal_steps` = all new tokens / (slots / 2) pairs.
Reported per policy: wall time of the whole run (encode of all windows + decode), generated tokens/s, the span of the rounds, and the
token steps: DERIVED on the host for the wave policies (sum over calls of the longest row's new tokens: what the call replays, up to
its poll granularity) and COUNTED for in-flight (graph replays, summed over the chains, and per chain).  `ideal_steps` = all new
tokens / 32 slots: what no policy can beat.
    python tools/inflight_bench.py [--reps 5] [--waves-reps 1] [--songs 32] [--steps 16] [--kv-fp8 cross both] [--only-inflight]
                                   [--new-tokens 96 512] [--tgt 640] [--guided] [--out FILE]"""
import argparse, importlib.util, json, os, random, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _sbd():
    spec = importlib.util.spec_from_file_location("small_batch_decode", os.path.join(os.path.dirname(os.path.abspath(__file__)), "small_batch_decode.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _median(xs):
    return sorted(xs)[len(xs) // 2]


def run(model, tok, frames, n_songs, reps, waves_reps, steps, slots, kv_fp8=(), only_inflight=False, new_tokens=(96, 512), guided=False):
    from mapperatorinator_amd import server
    from mapperatorinator_amd.scheduler import SequentialWindowScheduler, SongJob
    from mh_testing import synthetic_audio_varied
    server.get_eos_token_id = lambda *a, **k: []             # every row runs to its cap (see the module docstring)
    counts = [6 + (i * 12) // max(1, n_songs - 1) for i in range(n_songs)]
    rnd = random.Random(7)
    new = [[rnd.randint(*new_tokens) for _ in range(n)] for n in counts]
    audio = synthetic_audio_varied(max(counts), (frames - 1) * 128, seed=5)
    P = 2
    total = sum(sum(r) for r in new)

    def jobs():
        out = []
        for i, n in enumerate(counts):
            def prompt_fn(w, i=i, n=n):
                return dict(decoder_input_ids=torch.tensor([[tok.sos_id, 40 + (i + w) % 50]]),
                            **(dict(negative_prompt=torch.tensor([[tok.sos_id]])) if guided else {}),
                            generate_kwargs=dict(lookback_time=500 if w else 0, lookahead_time=500 if w != n - 1 else 0,
                                                 max_length=P + new[i][w]))
            out.append(SongJob(frames=audio[:n], prompt_fn=prompt_fn, on_result=lambda w, row, st: None,
                               generate_kwargs=dict(do_sample=False, num_beams=1, temperature=1.0, pad_token_id=0,
                                                    **(dict(cfg_scale=2.0) if guided else {}))))
        return out
    waves = [[new[i][w] for i in range(n_songs) if w < counts[i]] for w in range(max(counts))]
    if guided:
        return _run_guided(model, tok, jobs, counts, waves, total, reps, steps, slots, new_tokens)
    res = {"workload": f"{n_songs} songs x {min(counts)}..{max(counts)} windows, {sum(counts)} windows, new tokens per window {new_tokens[0]}..{new_tokens[1]} (seed 7), "
                       f"{total} new tokens, {slots} rows / slots", "window_counts": counts, "new_tokens": total,
           "ideal_steps": -(-total // slots),
           "derived_steps": {"waves": total, "merge_kwargs": sum(max(w) for w in waves),
                             "note": "sum over calls of the longest row: waves = batch-1 calls here (every window its own max_length)"}}
    policies = {"waves": dict(), "merge_kwargs": dict(merge_kwargs=True), "inflight": dict(inflight=True, inflight_steps=steps)}
    if only_inflight:
        policies = {"inflight": policies["inflight"]}
    for mode in kv_fp8:
        policies[f"inflight_kv8_{mode}"] = dict(inflight=True, inflight_steps=steps, inflight_kv_fp8=mode)
    runs = {k: [] for k in policies}
    for r in range(reps + 1):                                 # round 0 warms up (graphs captured, workspaces allocated)
        for name, kw in policies.items():                     # alternating: the policies see the same moment of the box
            if name == "waves" and r > waves_reps:
                continue
            sched = SequentialWindowScheduler(model, tok, encode_batch=32, decode_batch=slots, **kw)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st = sched.run(jobs())
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            assert st["windows"] == sum(counts), st
            if r:
                runs[name].append((wall, dict(st)))
    for name in policies:
        walls = [w for w, _ in runs[name]]
        st = runs[name][0][1]
        res[name] = {"rounds": len(walls), "wall_s": round(_median(walls), 3), "wall_s_span": [round(min(walls), 3), round(max(walls), 3)],
                     "tokens_per_s": round(total / _median(walls), 1), "decode_calls": st["decode_calls"]}
        if name.startswith("inflight"):
            chains = model.engine.lib.mh_t5_decode_chains_cfg(__import__("ctypes").byref(model.engine.packed.cfg), slots)
            res[name].update(admissions=st["admissions"], replays_all_chains=st["decode_steps"], chains=chains,
                             replays_per_chain=round(st["decode_steps"] / max(1, chains), 1))
    for mode in kv_fp8:
        res[f"inflight_kv8_{mode}"]["vs_inflight"] = round(res["inflight"]["wall_s"] / res[f"inflight_kv8_{mode}"]["wall_s"], 3)
    if not only_inflight:
        res["inflight_vs_merge_kwargs"] = round(res["merge_kwargs"]["wall_s"] / res["inflight"]["wall_s"], 3)
        res["note"] = (f"`waves` ran {len(runs['waves'])} round(s), not {reps}: with a max_length per window it is {sum(counts)} batch-1 calls, no "
                       "policy anybody would choose for this workload; the comparison that means something is merge_kwargs against inflight")
    return res


def _run_guided(model, tok, jobs, counts, waves, total, reps, steps, slots, new_tokens):
    """--guided: guided waves (merge_kwargs) against guided slots, alternating, round 0 as warm-up, medians of `reps` rounds"""
    from mapperatorinator_amd.scheduler import SequentialWindowScheduler
    pairs = max(1, slots // 2)
    calls = [w[a:a + pairs] for w in waves for a in range(0, len(w), pairs)]        # a guided wave: calls of slots / 2 windows
    res = {"workload": f"CONSTRUCTED, guided (cfg_scale 2, negative prompt = sos): {len(counts)} songs x {min(counts)}..{max(counts)} windows, "
                       f"{sum(counts)} windows, new tokens per window {new_tokens[0]}..{new_tokens[1]} (seed 7), {total} new tokens, "
                       f"decode_batch {slots} rows = {pairs} pairs", "window_counts": counts, "new_tokens": total,
           "ideal_steps": -(-total // pairs),
           "derived_steps": {"guided_merge_kwargs": sum(max(c) for c in calls), "note": "sum over calls of the longest row"}}
    policies = {"guided_merge_kwargs": dict(merge_kwargs=True),
                "inflight_guided": dict(inflight=True, inflight_guided=True, inflight_steps=steps)}
    runs = {k: [] for k in policies}
    for r in range(reps + 1):
        for name, kw in policies.items():
            sched = SequentialWindowScheduler(model, tok, encode_batch=32, decode_batch=slots, **kw)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st = sched.run(jobs())
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            assert st["windows"] == sum(counts), st
            if r:
                runs[name].append((wall, dict(st)))
    for name in policies:
        walls = [w for w, _ in runs[name]]
        st = runs[name][0][1]
        res[name] = {"rounds": len(walls), "wall_s": round(_median(walls), 3), "wall_s_span": [round(min(walls), 3), round(max(walls), 3)],
                     "tokens_per_s": round(total / _median(walls), 1), "decode_calls": st["decode_calls"]}
    st = runs["inflight_guided"][0][1]
    res["inflight_guided"].update(admissions=st["admissions"], replays=st["decode_steps"], chains=1, pair_slots=pairs)
    res["inflight_guided_vs_guided_merge_kwargs"] = round(res["guided_merge_kwargs"]["wall_s"] / res["inflight_guided"]["wall_s"], 3)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--waves-reps", type=int, default=1)
    ap.add_argument("--songs", type=int, default=32)
    ap.add_argument("--slots", type=int, default=32)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--tgt", type=int, default=640)
    ap.add_argument("--kv-fp8", nargs="*", default=[], choices=["cross", "self", "both"],
                    help="also run in-flight over the session's e4m3 caches, one policy per mode given")
    ap.add_argument("--only-inflight", action="store_true", help="leave the wave policies out")
    ap.add_argument("--new-tokens", type=int, nargs=2, default=[96, 512], metavar=("LO", "HI"))
    ap.add_argument("--guided", action="store_true", help="the workload under classifier-free guidance: guided waves against guided slots")
    ap.add_argument("--out", default="", help="also append the JSON line to this file")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    with torch.no_grad():
        model, tok, dims, frames = _sbd().build("varwhisper-small", a.tgt, dev)
        line = json.dumps({"inflight_decode": run(model, tok, frames, a.songs, a.reps, a.waves_reps, a.steps, a.slots, a.kv_fp8, a.only_inflight,
                                                     tuple(a.new_tokens), a.guided)})
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
