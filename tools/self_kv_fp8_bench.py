"""What `self_kv_fp8` (the token steps attend an e4m3 shadow of the self-attention cache) buys where the self-attention cache is the
larger share of a step's HBM traffic: batch-32 greedy decode to the full target length of varwhisper-small (2048 frames, tgt 2560),
ropewhisper-small (4096 frames + conditioning channels, tgt 2560) and t5-base (1251 frames, tgt 2048), bf16, EOS table zeroed.
Three settings in one process, alternating: plain, `cross_kv_fp8`, and both.  Decode loop only (cross K/V and its e4m3 copy
resident).  Reported: tokens/s of the whole decode and of every quarter of the position range -- a decode to q / 4 of the length is
timed for q = 1 .. 4 and the quarters are the differences (1-token prompt: every position is a token step), median of `--reps`
alternating rounds after one warm-up round.  Prints one JSON line per model.
    python tools/self_kv_fp8_bench.py [--models varwhisper-small,ropewhisper-small,t5-base] [--reps 2] [--out FILE]"""
import argparse, importlib.util, json, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TGT = {"varwhisper-small": 2560, "ropewhisper-small": 2560, "t5-base": 2048}
SETTINGS = (("plain", False, False), ("cross_kv_fp8", True, False), ("cross_kv_fp8+self_kv_fp8", True, True))


def _sbd():
    spec = importlib.util.spec_from_file_location("small_batch_decode", os.path.join(os.path.dirname(os.path.abspath(__file__)), "small_batch_decode.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def run(model_name, batch=32, reps=2, tgt=None, device="cuda:0"):
    from mapperatorinator_amd.server import build_sampling
    from mh_testing import synthetic_audio_varied
    dev = torch.device(device)
    tgt = tgt or TGT[model_name]
    model, tok, dims, frames = _sbd().build(model_name, tgt, dev)
    eng = model.engine
    eos_table = torch.zeros(tok.vocab_size_out, dtype=torch.uint8, device=dev)      # random weights: every row runs to max_length
    audio = synthetic_audio_varied(batch, (frames - 1) * 128, seed=5).to(dev)
    H, L = dims.n_heads, dims.n_dec_layers
    res = {"frames": frames, "key_positions": eng.packed.src_len, "tgt": tgt, "batch": batch,
           "cross_kv_mb_per_row": {"bf16": round(L * 2 * H * eng.packed.src_len * 128 / 1e6, 1), "e4m3": round(L * 2 * H * eng.packed.src_len * 64 / 1e6, 1)},
           "self_kv_kb_per_row_and_position": {"bf16": round(L * 2 * H * 128 / 1e3, 1), "e4m3": round(L * 2 * H * 68 / 1e3, 1)}}
    ends = [tgt * q // 4 for q in (1, 2, 3, 4)]
    with torch.no_grad():
        eng._enter()
        with torch.cuda.stream(eng.stream):
            cc = getattr(eng.packed, "cond_channels", 0)
            rb = torch.randn(batch, cc, generator=torch.Generator().manual_seed(1)).to(dev) if cc else None
            kv = eng.cross_kv(eng.encode_mel(eng.mel(audio), row_bias=rb))
            kv8 = eng.cross_kv_fp8(kv)
        eng._leave()
        torch.cuda.synchronize(dev)
        prompt = torch.full((batch, 1), tok.sos_id, dtype=torch.int32, device=dev)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        times = {name: [[] for _ in ends] for name, _, _ in SETTINGS}
        last = {}
        for r in range(reps + 1):                        # round 0 warms up (graphs captured, workspaces and the shadow allocated)
            for qi, end in enumerate(ends):
                for name, cross8, self8 in SETTINGS:     # alternating: the three settings see the same moment of the box
                    gk = dict(do_sample=False, num_beams=1, max_length=end, temperature=1.0, context_type="map", pad_token_id=0)
                    sp, _ = build_sampling(tok, gk, tgt)
                    eng._enter()
                    with torch.cuda.stream(eng.stream):
                        ev0.record(eng.stream)
                        tokens, _, _ = eng.decode(kv, prompt, None, eos_table, sp, poll_every=64, kv_fp8=kv8 if cross8 else None, self_kv_fp8=self8)
                        ev1.record(eng.stream)
                    eng._leave()
                    torch.cuda.synchronize(dev)
                    if r:
                        times[name][qi].append(ev0.elapsed_time(ev1))
                    if end == tgt:
                        last[name] = tokens.cpu()
        for name, _, _ in SETTINGS:
            ms = [sorted(t)[len(t) // 2] for t in times[name]]
            quarters, prev_ms, prev_end = [], 0.0, 1
            for end, m in zip(ends, ms):
                quarters.append(round(batch * (end - prev_end) / ((m - prev_ms) / 1e3), 1))
                prev_ms, prev_end = m, end
            res[name] = {"ms": round(ms[-1], 1), "tokens_per_s": round(batch * (tgt - 1) / (ms[-1] / 1e3), 1), "tokens_per_s_by_quarter": quarters}
        base = res["plain"]
        for name, _, _ in SETTINGS[1:]:
            res[name]["speedup_vs_plain"] = round(base["ms"] / res[name]["ms"], 3)
            res[name]["speedup_by_quarter"] = [round(a / b, 3) for a, b in zip(res[name]["tokens_per_s_by_quarter"], base["tokens_per_s_by_quarter"])]
            res[name]["same_ids_as_plain_fraction"] = round(float((last[name] == last["plain"]).float().mean()), 3)
        res["self_over_cross_only"] = round(res[SETTINGS[1][0]]["ms"] / res[SETTINGS[2][0]]["ms"], 3)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="varwhisper-small,ropewhisper-small,t5-base")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--tgt", type=int, default=0, help="override the target length (default: the released one per model)")
    ap.add_argument("--out", default="", help="also append the JSON line of every model to this file as it is measured")
    a = ap.parse_args()
    for m in a.models.split(","):
        line = json.dumps({m: run(m, a.batch, a.reps, a.tgt or None)})
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        torch.cuda.empty_cache()
