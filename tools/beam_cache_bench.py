"""Beam search at long targets: what following the beams costs per token when the self-attention cache is copied
(mh_t5_step + mh_t5_reorder_cache, the default) and when it is followed by index (mh_t5_step_indexed + mh_t5_reorder_index,
`beam_cache="indexed"`), and what the prompt costs token by token and prefilled (`beam_prefill=True`).

    python tools/beam_cache_bench.py [--model varwhisper-small] [--tgt 2560] [--positions 64,512,1024,2048] [--prompt 384]

varwhisper-small dims, bf16, at 1 window x 2 beams and 8 windows x 4 beams.  Per position p three legs alternate in one process,
`--rounds` times each, `--iters` tokens per timing (host clock around a stream synchronise): the plain step at p, step + cache copy of
p + 1 positions, indexed step + table reorder, and indexed step + table reorder over the e4m3 self cache (`self_kv_fp8=True`:
mh_t5_step_indexed_skv8, column `indexed_skv8_ms`; its baseline is the `indexed_ms` column of the same run).  The index table is filled
with a random beam of the row's window per position -- the most scattered table a search can produce.  One JSON line per (shape, position): median ms per token and the min .. max span of the
rounds, beside the bytes each reorder moves, derived from the shapes:
    copy   4 x (2 n_dec rows H 64 (p + 1) element size)   gather read + write, scatter read + write
    index  rows (p + 1) read + rows tgt_len written
Then the time to the first generated token of a `--prompt`-token prompt through beam.beam_search (cross K/V given: no encoder in
the timing), token by token on both routes and prefilled."""
import argparse
import ctypes as C
import importlib.util
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _sbd():
    spec = importlib.util.spec_from_file_location("small_batch_decode", os.path.join(os.path.dirname(os.path.abspath(__file__)), "small_batch_decode.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def reorder_bytes(cfg, es, rows, n_pos):
    copy = 4 * 2 * cfg.n_dec_layers * rows * cfg.n_heads * 64 * n_pos * es
    return dict(copy_bytes=copy, index_bytes=rows * n_pos + rows * cfg.tgt_len)


def per_token(eng, kv, G, nb, positions, iters, rounds):
    from mapperatorinator_amd import _lib
    lib, p, dev = eng.lib, eng.packed, eng.device
    cfg, w, R, V = C.byref(p.cfg), C.byref(p.w), G * nb, p.vocab_out
    es = torch.empty(0, dtype=eng.dtype).element_size()
    out = []
    eng._enter()
    with eng.on_stream():
        s = eng._s()
        ws = torch.zeros(int(lib.mh_t5_decode_workspace_bytes(cfg, R)), dtype=torch.uint8, device=dev)
        scratch = torch.empty(int(lib.mh_t5_reorder_cache_scratch_bytes(cfg, R, max(positions) + 1)), dtype=torch.uint8, device=dev)
        logits = torch.empty((R, V), dtype=torch.float32, device=dev)
        ids = torch.randint(3, V, (R,), generator=torch.Generator().manual_seed(1)).to(dev, torch.int32)
        base = (torch.arange(R) // nb * nb).view(R, 1)
        tabs = [(base + torch.randint(0, nb, (R, p.tgt_len), generator=torch.Generator().manual_seed(2 + i))).to(torch.uint8).to(dev).contiguous()
                for i in range(2)]
        src = (base.view(R) + (torch.arange(R) % nb + 1) % nb).to(dev, torch.int32)      # every beam takes its neighbour's row

        def plain(pos):
            _lib.check(lib.mh_t5_step(cfg, w, kv.data_ptr(), R, nb, ids.data_ptr(), pos, None, 1, logits.data_ptr(), ws.data_ptr(),
                                      ws.numel(), s), "mh_t5_step")

        def copy(pos):
            plain(pos)
            _lib.check(lib.mh_t5_reorder_cache(cfg, R, src.data_ptr(), pos + 1, ws.data_ptr(), ws.numel(), scratch.data_ptr(),
                                               scratch.numel(), s), "mh_t5_reorder_cache")

        def indexed(pos, state=[0]):
            a, b = tabs[state[0]], tabs[state[0] ^ 1]
            _lib.check(lib.mh_t5_step_indexed(cfg, w, kv.data_ptr(), None, R, nb, ids.data_ptr(), pos, None, 1, logits.data_ptr(),
                                              ws.data_ptr(), ws.numel(), a.data_ptr(), s), "mh_t5_step_indexed")
            _lib.check(lib.mh_t5_reorder_index(cfg, R, src.data_ptr(), pos + 1, a.data_ptr(), b.data_ptr(), s), "mh_t5_reorder_index")
            state[0] ^= 1
        # indexed step + table reorder, e4m3 self cache: the same tables, the cached rows read from a shadow (bf16 storage only)
        sh = None
        if eng.dtype == torch.bfloat16:
            sh = torch.zeros(int(lib.mh_t5_self_kv_fp8_bytes(cfg, R)), dtype=torch.uint8, device=dev)

        def indexed_skv8(pos, state=[0]):
            a, b = tabs[state[0]], tabs[state[0] ^ 1]
            _lib.check(lib.mh_t5_step_indexed_skv8(cfg, w, kv.data_ptr(), None, R, nb, ids.data_ptr(), pos, None, 1, logits.data_ptr(),
                                                   ws.data_ptr(), ws.numel(), a.data_ptr(), sh.data_ptr(), s), "mh_t5_step_indexed_skv8")
            _lib.check(lib.mh_t5_reorder_index(cfg, R, src.data_ptr(), pos + 1, a.data_ptr(), b.data_ptr(), s), "mh_t5_reorder_index")
            state[0] ^= 1
        legs = (("plain_step", plain), ("copy", copy), ("indexed", indexed)) + ((("indexed_skv8", indexed_skv8),) if sh is not None else ())
        for pos in positions:
            times = {name: [] for name, _ in legs}
            for r in range(rounds + 1):                        # round 0 warms up
                for name, fn in legs:
                    eng.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(iters):
                        fn(pos)
                    eng.synchronize()
                    if r:
                        times[name].append((time.perf_counter() - t0) * 1e3 / iters)
            row = dict(windows=G, beams=nb, rows=R, position=pos, **reorder_bytes(p.cfg, es, R, pos + 1))
            for name, t in times.items():
                row[name + "_ms"] = dict(median=round(statistics.median(t), 4), min=round(min(t), 4), max=round(max(t), 4))
            out.append(row)
            print(json.dumps(row), flush=True)
    eng._leave()
    return out


def first_token(eng, tok, kv, G, nb, P, repeats):
    """beam_search over a P-token prompt with max_length = P + 1: the search ends with its first step."""
    from mapperatorinator_amd import beam
    from mapperatorinator_amd.server import build_sampling
    sp, _ = build_sampling(tok, dict(do_sample=False, num_beams=nb, max_length=P + 1, temperature=1.0, context_type="map", pad_token_id=0),
                           eng.packed.tgt_len)
    prompt = torch.randint(3, eng.packed.vocab_out, (G, P), generator=torch.Generator().manual_seed(5))
    legs = (("copy_token_by_token", dict()), ("indexed_token_by_token", dict(cache="indexed")),
            ("indexed_prefill", dict(cache="indexed", prefill=True)))
    times = {name: [] for name, _ in legs}
    for r in range(repeats + 1):
        for name, kw in legs:
            eng.synchronize()
            t0 = time.perf_counter()
            ids = beam.beam_search(eng, kv, prompt, None, [], sp, nb, **kw)
            eng.synchronize()
            assert ids.shape[0] == G and ids.shape[1] > P
            if r:
                times[name].append((time.perf_counter() - t0) * 1e3)
    row = dict(windows=G, beams=nb, prompt_tokens=P, what="ms to the first generated token")
    for name, t in times.items():
        row[name + "_ms"] = dict(median=round(statistics.median(t), 2), min=round(min(t), 2), max=round(max(t), 2))
    print(json.dumps(row), flush=True)
    return row


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="varwhisper-small")
    ap.add_argument("--tgt", type=int, default=2560)
    ap.add_argument("--positions", default="64,512,1024,2048")
    ap.add_argument("--prompt", type=int, default=384)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="1x2,8x4")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("beam_cache_bench.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    model, tok, dims, frames = _sbd().build(a.model, a.tgt, dev)
    eng = model.engine
    from mh_testing import synthetic_audio_varied
    positions = [int(x) for x in a.positions.split(",")]
    assert max(positions) < a.tgt and a.prompt < a.tgt
    print(json.dumps(dict(workload=f"{a.model} bf16, tgt_len {a.tgt}: one decoder position for all (window, beam) rows + the reorder that "
                                   f"follows it; {a.iters} tokens per timing, {a.rounds} alternating rounds")), flush=True)
    for shape in a.shapes.split(","):
        G, nb = (int(x) for x in shape.split("x"))
        audio = synthetic_audio_varied(G, (frames - 1) * 128, seed=5).to(dev)
        eng._enter()
        with eng.on_stream():
            kv = eng.cross_kv(eng.encode_mel(eng.mel(audio)))
        eng._leave()
        eng.synchronize()
        per_token(eng, kv, G, nb, positions, a.iters, a.rounds)
        first_token(eng, tok, kv, G, nb, a.prompt, repeats=3)
