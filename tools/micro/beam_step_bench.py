"""Micro-benchmark: one mh_beam_step launch (csrc/beam.hip) on synthetic logits, for a given (G, num_beams, V, #eos, path).

    python tools/micro/beam_step_bench.py --chunks 4 --beams 8 --vocab 3837 --eos 0 --path 2
    python tools/micro/beam_step_bench.py --table          # the shapes of profiles/beam_step_large.txt

`--path`: the option "beam_step_path" (0 = automatic, 1 = LDS kernel, 2 = streaming kernel).  Prints one JSON line per shape: microseconds
per launch from device events around `--launches` back-to-back launches (the step reads the same IN state every time), minimum /
median / maximum over `--repeats` such windows -- the spread to hold a difference against.
`--per-token` adds what a token costs end to end through beam_search on a tiny T5 with that vocabulary, once with the kernel and once
with the torch-op bookkeeping (`use_kernel=False`: ~40 ATen launches and several host round trips): their difference plus the kernel's
own time is the torch-op bookkeeping's cost per token.
`--types-first` times mh_beam_step_tf with the types_first lookback on: every id is flagged as a timed event and the state starts
non-negative, so every beam row renormalises at every launch (the three extra reductions run for every row whether it does or not)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from mapperatorinator_amd import _lib   # noqa: E402


def time_step(G, nb, V, n_eos, path, launches=200, repeats=7, cfg=False, seed=0, types_first=False):
    lib = _lib.load()
    old = _lib.set_option("beam_step_path", path)
    try:
        K = min(max(2, 1 + n_eos) * nb, nb * V)
        chosen = lib.mh_beam_step_path(nb, V, K)
        if chosen == 0:
            return dict(G=G, beams=nb, V=V, eos=n_eos, K=K, path=path, kernel="refused")
        dev = torch.device("cuda")
        gen = torch.Generator().manual_seed(seed)
        P, L = 2, 66
        T = 33                                         # mid-sequence: the state copies move half a hypothesis
        RE = G * nb * (2 if cfg else 1)
        logits = (torch.randn(RE, V, generator=gen) * 6.0).to(dev)
        eos = (torch.randperm(V - 3, generator=gen)[:n_eos] + 3).to(dev)
        eos_table = torch.zeros(V, dtype=torch.uint8, device=dev)
        eos_table[eos] = 1

        def state():
            run = torch.randint(3, V, (G, nb, L), generator=gen).to(torch.int32).to(dev)
            run[:, :, 0] = 1
            return dict(run=run, rs=(-torch.rand(G, nb, generator=gen) * 5).to(dev), rb=torch.zeros((G, nb, L - P), dtype=torch.int32, device=dev),
                        seq=run.clone(), bs=torch.full((G, nb), -1e9, device=dev), bb=torch.full((G, nb, L - P), -1, dtype=torch.int32, device=dev),
                        fin=torch.zeros((G, nb), dtype=torch.uint8, device=dev))
        a, b = state(), state()
        keep = [torch.ones(G, dtype=torch.uint8, device=dev), torch.zeros(RE, dtype=torch.int32, device=dev),
                torch.zeros(RE, dtype=torch.int32, device=dev), torch.zeros((G, 3), dtype=torch.int32, device=dev)]
        sp = _lib.MhSampling()
        sp.top_p, sp.temperature, sp.timeshift_bias, sp.cfg_scale = 1.0, 0.9, 0.3, 1.5 if cfg else 1.0
        sp.ts_start, sp.ts_end, sp.n_sos, sp.max_length = 3, min(3 + 1001, V), 1, L
        sp.sos_ids[0] = 1
        prev = None
        if types_first:      # ids [ts_start, ts_start + 50) are the lookback range; every id counts as timed, id 2 as the warper's eos
            tok_flags = torch.ones(V, dtype=torch.uint8)
            tok_flags[2] |= 16
            tok_flags = tok_flags.to(dev)
            sp.lookback_types_first, sp.lookback_mask_end, sp.tok_flags = 1, sp.ts_start + 50, tok_flags.data_ptr()
            prev = torch.full((G * nb,), 1e-3, dtype=torch.float32, device=dev)
        bs = _lib.MhBeamStep()
        bs.logits, bs.eos_table = logits.data_ptr(), eos_table.data_ptr()
        bs.G, bs.num_beams, bs.V, bs.P, bs.max_length, bs.K, bs.cur_len = G, nb, V, P, L, K, T
        bs.cfg, bs.cfg_scale, bs.length_penalty, bs.early_stopping, bs.sp = int(cfg), sp.cfg_scale, 1.0, 0, sp
        for k in a:
            setattr(bs, k + "_in", a[k].data_ptr())
            setattr(bs, k + "_out", b[k].data_ptr())
        bs.heuristic_open, bs.src, bs.last, bs.flags = (t.data_ptr() for t in keep)
        stream = torch.cuda.current_stream().cuda_stream

        def launch(n):
            for _ in range(n):
                if types_first:
                    _lib.check(lib.mh_beam_step_tf(C.byref(bs), prev.data_ptr(), stream), "mh_beam_step_tf")
                else:
                    _lib.check(lib.mh_beam_step(C.byref(bs), stream), "mh_beam_step")
        launch(20)
        torch.cuda.synchronize()
        us = []
        for _ in range(repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch(launches)
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / launches)
        return dict(G=G, beams=nb, V=V, eos=n_eos, K=K, path=path, kernel={1: "lds", 2: "streaming"}[chosen], types_first=types_first,
                    us_min=round(min(us), 2), us_median=round(statistics.median(us), 2), us_max=round(max(us), 2))
    finally:
        _lib.set_option("beam_step_path", old)


def time_per_token(G, nb, V, new_tokens=96, repeats=4):
    """Per-token wall time of beam_search on a tiny T5 with V output ids: kernel form vs torch-op bookkeeping (no EOS: every step runs)."""
    from mapperatorinator_amd import EventType, Tokenizer
    from mapperatorinator_amd.modeling import MapperatorinatorHIP
    from mapperatorinator_amd.server import build_sampling
    from mapperatorinator_amd.t5_engine import T5_PRESETS
    from mapperatorinator_amd.tokenizer import _TAIL
    from mh_testing import random_t5_state_dict, synthetic_audio_varied
    src, tgt = 64, 1 + new_tokens
    base = Tokenizer.from_ranges([(EventType.TIME_SHIFT, 0, 50), (EventType.SNAPPING, 0, 16), (EventType.DISTANCE, 0, 0)] + _TAIL)
    tok = Tokenizer.from_ranges([(EventType.TIME_SHIFT, 0, 50), (EventType.SNAPPING, 0, 16),
                                 (EventType.DISTANCE, 0, V - base.vocab_size_out)] + _TAIL)
    assert tok.vocab_size_out == V, (tok.vocab_size_out, V)
    sd = random_t5_state_dict(T5_PRESETS["tiny"], tok.vocab_size_in, V, seed=3, lm_head_gain=6.0)
    model = MapperatorinatorHIP(sd, T5_PRESETS["tiny"], vocab_size_in=tok.vocab_size_in, vocab_size_out=V, src_seq_len=src,
                                tgt_seq_len=tgt, dtype=torch.float32, device="cuda")
    audio = synthetic_audio_varied(G, (src - 1) * 128, seed=5).cuda()
    prompt = torch.full((G, 1), tok.sos_id, dtype=torch.long)
    sp, _ = build_sampling(tok, dict(do_sample=False, num_beams=nb, max_length=tgt, temperature=1.0, context_type="map", pad_token_id=0), tgt)
    res = dict(G=G, beams=nb, V=V, steps=new_tokens)
    ids = {}
    for name, uk in (("kernel", True), ("torch_op", False)):
        best = []
        for r in range(repeats + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = model.engine.generate_beam(audio, prompt, None, [], sp, nb, use_kernel=uk)
            torch.cuda.synchronize()
            if r:
                best.append((time.perf_counter() - t0) * 1e6 / (out["tokens"].shape[1] - 1))
        ids[name] = out["tokens"]
        res[name + "_us_per_token"] = [round(min(best), 1), round(statistics.median(best), 1), round(max(best), 1)]
    res["same_ids"] = bool(torch.equal(ids["kernel"], ids["torch_op"]))
    return res


TABLE = [(2, 2080, (1, 2)), (4, 3837, (1, 2)), (8, 3837, (2,)), (8, 4493, (2,)), (8, 8192, (2,))]

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=4)
    ap.add_argument("--beams", type=int, default=8)
    ap.add_argument("--vocab", type=int, default=3837)
    ap.add_argument("--eos", type=int, default=0)
    ap.add_argument("--path", type=int, default=0, choices=(0, 1, 2))
    ap.add_argument("--guidance", action="store_true")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--per-token", action="store_true")
    ap.add_argument("--table", action="store_true")
    ap.add_argument("--types-first", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("beam_step_bench: no GPU (there is nothing to time without one)")
    if a.table:
        # both paths of a shared shape alternate (twice each) so that a drift of the box does not read as a difference between them
        for nb, V, paths in TABLE:
            for rnd in range(2 if len(paths) > 1 else 1):
                for path in paths:
                    print(json.dumps(time_step(a.chunks, nb, V, a.eos, path, a.launches, a.repeats)), flush=True)
        for nb, V, paths in TABLE:
            if paths == (2,):
                print(json.dumps(time_per_token(a.chunks, nb, V)), flush=True)
    else:
        print(json.dumps(time_step(a.chunks, a.beams, a.vocab, a.eos, a.path, a.launches, a.repeats, cfg=a.guidance, types_first=a.types_first)), flush=True)
        if a.per_token:
            print(json.dumps(time_per_token(a.chunks, a.beams, a.vocab)), flush=True)
