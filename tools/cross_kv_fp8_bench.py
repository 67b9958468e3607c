"""What `cross_kv_fp8` (the token steps stream an e4m3 copy of the cross-attention K / V) buys on the released Whisper-family
shapes: batch-32 greedy decode of varwhisper-small (2048 frames), ropewhisper-small (4096 frames + conditioning channels) and
whisper-small (1024 frames), each with and without the mode, and two-beam decode of one window with and without it.  Decode loop
only (cross K/V resident; the one-off quantisation is timed separately), median of `--reps` runs after one warm-up.
Prints one JSON line.    python tools/cross_kv_fp8_bench.py [--models varwhisper-small,...] [--new-tokens 128] [--out FILE]"""
import argparse, importlib.util, json, os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _sbd():
    spec = importlib.util.spec_from_file_location("small_batch_decode", os.path.join(os.path.dirname(os.path.abspath(__file__)), "small_batch_decode.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def run(model_name, batch=32, new_tokens=128, beams=2, reps=3, device="cuda:0"):
    from mapperatorinator_amd.beam import beam_search
    from mapperatorinator_amd.server import build_sampling
    from mh_testing import synthetic_audio_varied
    dev = torch.device(device)
    tgt = 1 + new_tokens
    model, tok, dims, frames = _sbd().build(model_name, tgt, dev)
    eng = model.engine
    eos_table = torch.zeros(tok.vocab_size_out, dtype=torch.uint8, device=dev)      # random weights: every row runs to max_length
    audio = synthetic_audio_varied(batch, (frames - 1) * 128, seed=5).to(dev)
    res = {"frames": frames, "key_positions": eng.packed.src_len}
    with torch.no_grad():
        eng._enter()
        with torch.cuda.stream(eng.stream):
            cc = getattr(eng.packed, "cond_channels", 0)
            rb = torch.randn(batch, cc, generator=torch.Generator().manual_seed(1)).to(dev) if cc else None
            kv = eng.cross_kv(eng.encode_mel(eng.mel(audio), row_bias=rb))
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            kv8 = eng.cross_kv_fp8(kv)
            ev0.record(eng.stream)
            kv8 = eng.cross_kv_fp8(kv)
            ev1.record(eng.stream)
        eng._leave()
        torch.cuda.synchronize(dev)
        res["quantise_ms"] = round(ev0.elapsed_time(ev1), 3)
        res["cross_kv_mb_per_row"] = round(kv.numel() * 2 / batch / 1e6, 1)
        gk = dict(do_sample=False, num_beams=1, max_length=tgt, temperature=1.0, context_type="map", pad_token_id=0)
        prompt = torch.full((batch, 1), tok.sos_id, dtype=torch.int32, device=dev)
        toks = {}
        for name, copy in (("bf16_kv", None), ("e4m3_kv", kv8)):
            times = []
            for r in range(reps + 1):
                sp, _ = build_sampling(tok, gk, tgt)
                eng._enter()
                with torch.cuda.stream(eng.stream):
                    ev0.record(eng.stream)
                    tokens, _, _ = eng.decode(kv, prompt, None, eos_table, sp, poll_every=64, kv_fp8=copy)
                    ev1.record(eng.stream)
                eng._leave()
                torch.cuda.synchronize(dev)
                if r:
                    times.append(ev0.elapsed_time(ev1))
            ms = sorted(times)[len(times) // 2]
            toks[name] = tokens.cpu()
            res[f"greedy_b{batch}_{name}"] = {"ms": round(ms, 2), "us_per_token_step": round(ms * 1e3 / new_tokens, 1),
                                              "tokens_per_s": round(batch * new_tokens / (ms / 1e3), 1)}
        res[f"greedy_b{batch}_speedup"] = round(res[f"greedy_b{batch}_bf16_kv"]["ms"] / res[f"greedy_b{batch}_e4m3_kv"]["ms"], 3)
        res["greedy_same_ids_fraction"] = round(float((toks["bf16_kv"] == toks["e4m3_kv"]).float().mean()), 3)
        # two beams over ONE window (the reference's timing pass): host-driven steps, wall clock
        gkb = dict(gk, num_beams=beams)
        p1 = torch.full((1, 1), tok.sos_id, dtype=torch.long)
        kv1 = kv[:, :, :1].contiguous()
        for name, copy in (("bf16_kv", None), ("e4m3_kv", True)):
            times = []
            for r in range(reps + 1):
                sp, _ = build_sampling(tok, gkb, tgt)
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                out = beam_search(eng, kv1, p1, None, [], sp, beams, kv_fp8=copy)
                torch.cuda.synchronize(dev)
                if r:
                    times.append(time.perf_counter() - t0)
            dt = sorted(times)[len(times) // 2]
            n = int(out.shape[1]) - 1
            res[f"beam{beams}_1window_{name}"] = {"ms": round(dt * 1e3, 2), "ms_per_beam_step": round(dt * 1e3 / max(n, 1), 3),
                                                 "tokens_per_s": round(n / dt, 1)}
        res[f"beam{beams}_1window_speedup"] = round(res[f"beam{beams}_1window_bf16_kv"]["ms"] / res[f"beam{beams}_1window_e4m3_kv"]["ms"], 3)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="varwhisper-small,ropewhisper-small,whisper-small")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--new-tokens", type=int, default=128)
    ap.add_argument("--beams", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="", help="also append the JSON line of every model to this file as it is measured")
    a = ap.parse_args()
    allres = {}
    for m in a.models.split(","):
        allres[m] = run(m, a.batch, a.new_tokens, a.beams, a.reps)
        line = json.dumps({m: allres[m]})
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        torch.cuda.empty_cache()
