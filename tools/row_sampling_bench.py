"""What the row-settings decode (`mh_t5_generate_rows`, `merge_kwargs`) buys and costs, t5-base bf16 on one GPU.

(a) Ragged songs through SequentialWindowScheduler: 32 songs whose window counts are spread over 6..18.  A song's first window has
    no lookback EOS ids and no lookback mask, its last no lookahead EOS ids (the reference's `generate_sequential`), so every wave in
    which a song ends holds two kwargs groups.  Every row is forced to 384 new tokens: `max_length` = prompt + 384 and the EOS sets are
    EMPTIED here (server.get_eos_token_id patched in this process; the lookback mask and the grouping by kwargs are untouched), prompts
    of equal width.  Run with and without `merge_kwargs`, alternating; reports decode calls, wall time of the whole run (encode of all
    windows + waves) and generated tokens/s.  A CONSTRUCTED case: how often real workloads split waves is not known.
(b) Cost of the row form: the same 32-row uniform workload (384 new tokens, decode loop only, cross K/V resident) through
    `T5Engine.decode(row_sampling=)` and through the plain entry, alternating; ms per token step, with the run-to-run spread of the
    plain entry beside the difference.
    python tools/row_sampling_bench.py [--reps 3] [--songs 32] [--new 384] [--out FILE]"""
import argparse, importlib.util, json, os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _sbd():
    spec = importlib.util.spec_from_file_location("small_batch_decode", os.path.join(os.path.dirname(os.path.abspath(__file__)), "small_batch_decode.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _median(xs):
    return sorted(xs)[len(xs) // 2]


def songs_through_the_scheduler(model, tok, frames, n_songs, new, reps):
    from mapperatorinator_amd import server
    from mapperatorinator_amd.scheduler import SequentialWindowScheduler, SongJob
    from mh_testing import synthetic_audio_varied
    server.get_eos_token_id = lambda *a, **k: []             # every row runs to its cap (see the module docstring)
    counts = [6 + (i * 12) // max(1, n_songs - 1) for i in range(n_songs)]
    audio = synthetic_audio_varied(max(counts), (frames - 1) * 128, seed=5)
    P = 2

    def jobs():
        out = []
        for i, n in enumerate(counts):
            def prompt_fn(w, i=i, n=n):
                return dict(decoder_input_ids=torch.tensor([[tok.sos_id, 40 + (i + w) % 50]]),
                            generate_kwargs=dict(lookback_time=500 if w else 0, lookahead_time=500 if w != n - 1 else 0))
            out.append(SongJob(frames=audio[:n], prompt_fn=prompt_fn, on_result=lambda w, row, st: None,
                               generate_kwargs=dict(do_sample=False, num_beams=1, max_length=P + new, temperature=1.0, pad_token_id=0)))
        return out
    res = {"songs": n_songs, "windows": sum(counts), "waves": max(counts), "window_counts": counts, "new_tokens_per_row": new}
    runs = {False: [], True: []}
    for r in range(reps + 1):                                 # round 0 warms up (graphs captured, workspaces allocated)
        for merge in (False, True):                           # alternating: both policies see the same moment of the box
            sched = SequentialWindowScheduler(model, tok, encode_batch=32, decode_batch=32, merge_kwargs=merge)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st = sched.run(jobs())
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            assert st["windows"] == sum(counts), st
            if merge:
                assert st["decode_calls"] == max(counts), f"merged: {st['decode_calls']} calls for {max(counts)} waves of one guidance state"
            if r:
                runs[merge].append((wall, st["decode_calls"]))
    for merge, name in ((False, "default"), (True, "merge_kwargs")):
        walls = [w for w, _ in runs[merge]]
        res[name] = {"decode_calls": runs[merge][0][1], "wall_s": round(_median(walls), 3), "wall_s_all": [round(w, 3) for w in walls],
                     "tokens_per_s": round(sum(counts) * new / _median(walls), 1)}
    res["speedup"] = round(res["default"]["wall_s"] / res["merge_kwargs"]["wall_s"], 3)
    return res


def cost_of_the_row_form(model, tok, frames, tgt, batch, new, reps):
    from mapperatorinator_amd.server import build_row_sampling, build_sampling
    from mh_testing import synthetic_audio_varied
    eng, dev = model.engine, model.engine.device
    gk = dict(do_sample=False, num_beams=1, max_length=1 + new, temperature=1.0, pad_token_id=0)
    audio = synthetic_audio_varied(batch, (frames - 1) * 128, seed=5).to(dev)
    eng._enter()
    with torch.cuda.stream(eng.stream):
        kv = eng.cross_kv(eng.encode_mel(eng.mel(audio)))
    eng._leave()
    torch.cuda.synchronize(dev)
    prompt = torch.full((batch, 1), tok.sos_id, dtype=torch.int32, device=dev)
    zero = torch.zeros(tok.vocab_size_out, dtype=torch.uint8, device=dev)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times, last = {"plain": [], "rows": []}, {}
    for r in range(reps + 1):
        for name in ("plain", "rows"):
            sp, _ = build_sampling(tok, gk, tgt)
            rs = None
            if name == "rows":
                sp, rows, tables = build_row_sampling(tok, [gk] * batch, tgt)
                rs = (sp, rows, torch.zeros_like(tables))
            eng._enter()
            with torch.cuda.stream(eng.stream):
                ev0.record(eng.stream)
                tokens, _, _ = eng.decode(kv, prompt, None, zero, sp, poll_every=64, row_sampling=rs)
                ev1.record(eng.stream)
            eng._leave()
            torch.cuda.synchronize(dev)
            if r:
                times[name].append(ev0.elapsed_time(ev1) / new)
            last[name] = tokens.cpu()
    assert torch.equal(last["plain"], last["rows"]), "the row form decoded other ids than the plain entry"
    p, q = _median(times["plain"]), _median(times["rows"])
    return {"batch": batch, "new_tokens_per_row": new, "plain_ms_per_step": round(p, 4), "rows_ms_per_step": round(q, 4),
            "difference_us": round((q - p) * 1e3, 2), "plain_spread_us": round((max(times["plain"]) - min(times["plain"])) * 1e3, 2),
            "plain_all": [round(t, 4) for t in times["plain"]], "rows_all": [round(t, 4) for t in times["rows"]]}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--songs", type=int, default=32)
    ap.add_argument("--new", type=int, default=384)
    ap.add_argument("--tgt", type=int, default=512)
    ap.add_argument("--out", default="", help="also append the JSON lines to this file")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    with torch.no_grad():
        model, tok, dims, frames = _sbd().build("t5-base", a.tgt, dev)
        for name, res in (("row_form_cost", cost_of_the_row_form(model, tok, frames, a.tgt, 32, a.new, max(a.reps, 5))),
                          ("ragged_songs", songs_through_the_scheduler(model, tok, frames, a.songs, a.new, a.reps))):
            line = json.dumps({name: res})
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")
