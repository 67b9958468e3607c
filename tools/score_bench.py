"""Times teacher-forced scoring on the device (`model.score`) against the route it replaces: `model.forward` + the five
MaiMod formulas (processor.py:519-525) as torch ops on the device + the device-to-host copy of what each route returns.
Both routes run in one process on the same inputs; the baseline is the unchanged `forward`.  Median of `--reps` runs after
`--warmup`, stream-synchronised wall clock.  Also times the row kernel alone on one LM-head block (`score_block_rows` x V
fp32, read once) and reports its share of the HBM peak.  Prints one JSON line.

    python tools/score_bench.py [--shape base|v32|both] [--dtype bf16|fp32] [--reps 20] [--warmup 3] [--block-sweep 256,1024]

Shapes: base = osuT5-base dims, 1251 frames, B 32, T 512, the benchmark vocabulary; v32 = the same backbone dims with the
released V32 decoder shape (tgt_seq_len 2560, 3837 output ids), B 32, T 2560.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12        # bytes / s, MI355X


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts)


def torch_route(model, audio_kv, ids, targets):
    logits = model.engine.decoder_forward(audio_kv, ids, None)
    B, T, V = logits.shape
    lg = logits.view(B * T, V)
    probs = lg.softmax(dim=-1)
    entropy = -torch.sum(probs * torch.log2(probs + 1e-10), dim=-1)
    tg = targets.view(-1).clamp(min=0).long()
    surprisal = -torch.log2(probs[torch.arange(B * T, device=lg.device), tg] + 1e-10)
    relative = torch.where(entropy > 0, surprisal / entropy, torch.zeros_like(entropy))
    best = lg.argmax(dim=-1)
    logprob = lg.log_softmax(dim=-1)[torch.arange(B * T, device=lg.device), tg]
    return [t.cpu() for t in (surprisal, entropy, relative, logprob, best)]


def run_shape(name, dtype, reps, warmup, block_sweep=()):
    from mapperatorinator_amd import Tokenizer, _lib
    from mapperatorinator_amd.modeling import MapperatorinatorHIP
    from mapperatorinator_amd.t5_engine import T5_PRESETS, next_token_targets
    from mh_testing import random_t5_state_dict, synthetic_audio_varied
    B, src = 32, 1251
    tok = Tokenizer.benchmark_vocab(src_seq_len=src)
    T, vout = (512, tok.vocab_size_out) if name == "base" else (2560, 3837)
    vin = max(tok.vocab_size_in, vout + 16)
    sd = random_t5_state_dict(T5_PRESETS["base"], vin, vout, seed=1, lm_head_gain=2.0)
    model = MapperatorinatorHIP(sd, T5_PRESETS["base"], vocab_size_in=vin, vocab_size_out=vout, src_seq_len=src, tgt_seq_len=T,
                                dtype=dtype, device="cuda")
    eng = model.engine
    audio = synthetic_audio_varied(B, (src - 1) * 128, seed=2).cuda()
    ids = torch.randint(3, vout, (B, T), generator=torch.Generator().manual_seed(3)).to(torch.int32).cuda()
    with torch.cuda.stream(eng.stream):
        kv = eng.cross_kv(eng.encode_mel(eng.mel(audio)))
    targets = next_token_targets(ids)
    span = torch.full_like(targets, -1)
    span[:, T // 4: T // 2] = targets[:, T // 4: T // 2]          # MaiMod's shape: a quarter of every row is scored
    span_host = span.cpu()

    def ours(tg):
        with torch.cuda.stream(eng.stream):
            out = eng.score(kv, ids, None, tg)
            return [v.cpu() for v in out.values()]          # (the copies are ordered behind the kernels on the engine's stream)

    def theirs():
        with torch.cuda.stream(eng.stream):
            return torch_route(model, kv, ids, targets)

    def forward_and_copy():          # what the reference's model_forward returns: the logits on the host
        with torch.cuda.stream(eng.stream):
            return eng.decoder_forward(kv, ids, None).cpu()

    res = dict(shape=name, dtype=str(dtype).split(".")[-1], B=B, T=T, V=vout, reps=reps)
    torch.cuda.reset_peak_memory_stats()
    base_alloc = torch.cuda.memory_allocated()
    res["score_ms"], res["score_ms_min"] = timed(lambda: ours(targets), reps, warmup)
    res["score_peak_bytes"] = torch.cuda.max_memory_allocated() - base_alloc
    res["score_span_ms"], _ = timed(lambda: ours(span_host), reps, warmup)
    res["score_block_rows"] = int(_lib.load().mh_get_option(b"score_block_rows"))
    sweep = {}
    for rows_per_block in block_sweep:          # the same pass at other block sizes (results do not depend on it)
        old_rows = _lib.set_option("score_block_rows", rows_per_block)
        try:
            sweep[str(rows_per_block)] = timed(lambda: ours(targets), reps, warmup)[0]
        finally:
            _lib.set_option("score_block_rows", old_rows)
    res["score_ms_by_block_rows"] = sweep
    torch.cuda.reset_peak_memory_stats()
    base_alloc = torch.cuda.memory_allocated()
    res["forward_torch_ops_ms"], res["forward_torch_ops_ms_min"] = timed(theirs, reps, warmup)
    res["forward_torch_ops_peak_bytes"] = torch.cuda.max_memory_allocated() - base_alloc
    res["forward_logits_to_host_ms"], _ = timed(forward_and_copy, max(3, reps // 4), 1)
    lib = _lib.load()
    res["score_workspace_bytes"] = int(lib.mh_t5_score_workspace_bytes(C.byref(eng.packed.cfg), B, T))
    res["forward_workspace_bytes"] = int(lib.mh_t5_forward_workspace_bytes(C.byref(eng.packed.cfg), B, T))
    res["logits_bytes"] = B * T * vout * 4
    a, b = ours(targets), theirs()
    on = (targets >= 0).view(-1).cpu()
    res["max_abs_diff_vs_torch_ops"] = {k: float((x.double().view(-1) - y.double().view(-1))[on].abs().max())
                                        for k, x, y in zip(("surprisal", "entropy"), a, b)}

    # the row kernel alone on one block, a fresh block each launch so that it comes from HBM (64 blocks = 250 MB > the caches)
    Cb = int(lib.mh_get_option(b"score_block_rows"))
    n_blk = 64
    blocks = torch.randn(n_blk, Cb, vout, device="cuda")
    tg = torch.randint(0, vout, (Cb,), device="cuda", dtype=torch.int32)
    outs = [torch.empty(Cb, device="cuda") for _ in range(4)] + [torch.empty(Cb, device="cuda", dtype=torch.int32)]
    s = torch.cuda.current_stream().cuda_stream

    def rows():
        for i in range(n_blk):
            lib.mh_score_rows(blocks[i].data_ptr(), vout, Cb, vout, tg.data_ptr(), *[o.data_ptr() for o in outs], s)
    ms, _ = timed(rows, reps, warmup)
    res["row_kernel_us_per_block"] = ms * 1e3 / n_blk
    res["row_kernel_block_bytes"] = Cb * vout * 4
    res["row_kernel_hbm_fraction"] = Cb * vout * 4 / (ms * 1e-3 / n_blk) / HBM_PEAK
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="base", choices=["base", "v32", "both"])
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--block-sweep", default="", help="comma-separated score_block_rows values to time as well")
    a = ap.parse_args()
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    sweep = [int(v) for v in a.block_sweep.split(",") if v]
    shapes = ["base", "v32"] if a.shape == "both" else [a.shape]
    print(json.dumps(dict(bench="score", results=[run_shape(s, dtype, a.reps, a.warmup, sweep) for s in shapes])))


if __name__ == "__main__":
    main()
