"""CPU side of the row-settings decode (`mh_t5_generate_rows`, `server.build_row_sampling`, `merge_kwargs` of the scheduler and the
batcher): symbols, layout, refusals, the host translation and the two batching policies on stub engines.  The device side is
tests/test_gpu_row_sampling.py."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
from mapperatorinator_amd import Tokenizer, _lib
from mapperatorinator_amd.server import (FLAG_COND0, RequestBatcher, build_row_sampling, build_sampling, get_eos_token_id,
                                         row_call_key)
from mh_testing import row_sampling as rs

G = rs.gen_kwargs


def _cfg(dtype):    # d 128, 2 heads, 2 + 2 layers, src 251, tgt 48
    return _lib.MhT5Config(128, 64, 256, 2, 2, 2, 10, 10, 388, 416, 251, 48, dtype, 1e-6)


def test_symbol_and_struct_are_declared_bound_and_exported_at_abi_11():
    hdr = open(os.path.join(ROOT, "include", "mapperhip.h")).read()
    assert re.search(r"#define\s+MH_ABI_VERSION\s+11\b", hdr)
    lib = _lib.load()
    assert re.search(r"\bint\s+mh_t5_generate_rows\s*\(", hdr) and "typedef struct MhRowSampling" in hdr
    assert "mh_t5_generate_rows" in _lib.SYMBOLS and hasattr(lib, "mh_t5_generate_rows")
    # mh_t5_generate_skv8's argument list plus rows, eos_tables, n_eos_sets
    assert list(_lib.SYMBOLS["mh_t5_generate_rows"][1]) == list(_lib.SYMBOLS["mh_t5_generate_skv8"][1]) + [C.c_void_p, C.c_void_p, C.c_int]
    assert _lib.ABI_VERSION == 11 and lib.mh_abi_version() == 11
    assert C.sizeof(_lib.MhRowSampling) == lib.mh_struct_size(8) == 64
    assert lib.mh_struct_size(9) == -1
    # MhSampling keeps its layout; the header lists every field of an entry
    assert C.sizeof(_lib.MhSampling) == lib.mh_struct_size(3)
    body = hdr[hdr.index("typedef struct MhRowSampling"):hdr.index("} MhRowSampling;")]
    for name, _ in _lib.MhRowSampling._fields_:
        assert re.search(r"\b%s\b" % name, body), name


def test_library_refuses_null_and_range_with_a_message():
    lib = _lib.load()
    one, w, sp = C.c_void_p(256), _lib.MhT5Weights(), _lib.MhSampling()
    bf16, f32 = _cfg(_lib.MH_BF16), _cfg(_lib.MH_F32)
    args = (C.byref(w), one, 1, one, None, 1, None, C.byref(sp), one, one, None, None, one, 1 << 40, 16, one)
    assert lib.mh_t5_generate_rows(C.byref(bf16), *args, None, None, one, 1) == -1
    assert b"mh_t5_generate_rows: null argument (rows" in lib.mh_last_error()
    assert lib.mh_t5_generate_rows(C.byref(bf16), *args, None, one, None, 1) == -1
    assert b"mh_t5_generate_rows: null argument (rows" in lib.mh_last_error()
    assert lib.mh_t5_generate_rows(C.byref(bf16), *args, None, one, one, 0) == -1
    assert b"mh_t5_generate_rows: n_eos_sets 0 must be >= 1" in lib.mh_last_error()
    # fp32 storage with a shadow, or with an e4m3 copy of the cross K/V: as the uniform entries
    assert lib.mh_t5_generate_rows(C.byref(f32), *args, one, one, one, 1) == -1
    assert b"bf16 storage" in lib.mh_last_error()
    # what the shared body finds names this entry (stream NULL: checked before anything is followed); eos_table may be NULL
    assert lib.mh_t5_generate_rows(C.byref(bf16), *args[:-1], None, None, one, one, 1) == -1
    assert b"mh_t5_generate_rows: needs a non-default stream" in lib.mh_last_error()
    sp8 = _lib.MhSampling()
    sp8.max_length, sp8.cfg_scale, sp8.cross_kv_fp8 = 8, 1.0, 256
    args8 = args[:7] + (C.byref(sp8),) + args[8:]
    assert lib.mh_t5_generate_rows(C.byref(f32), *args8, None, one, one, 1) == -1
    assert b"mh_t5_generate_rows: cross_kv_fp8 needs bf16 storage" in lib.mh_last_error()
    # the uniform entry still needs its table
    assert lib.mh_t5_generate(C.byref(bf16), *args) == -1
    assert b"mh_t5_generate: null argument" in lib.mh_last_error()


def test_build_row_sampling_equals_build_sampling_for_equal_entries():
    tok = rs.tokenizer("bench")
    tf = Tokenizer.from_json(f"{GOLDEN}/tokenizer_types_first.json")
    cases = [(tok, G(lookahead_time=400, temperature=0.7, timeshift_bias=0.5, context_type="gd", max_length=30)),
             (tok, G(do_sample=True, top_k=20, top_p=0.8, seed=5, seed_call_index=2, rng_row_offset=7, cfg_scale=2.0)),
             (tf, G(types_first=True, timing_temperature=0.5, taiko_hit_temperature=0.9, lookback_time=200, context_type="map"))]
    for t, gk in cases:
        for n in (1, 3):
            want, eos = build_sampling(t, gk, 48)
            sp, rows, tables = build_row_sampling(t, [dict(gk) for _ in range(n)], 48)
            assert bytes(sp) == bytes(want) and getattr(sp, "num_beams", 1) == 1
            assert (sp.host_tok_flags is None) == (want.host_tok_flags is None)
            assert sp.host_tok_flags is None or np.array_equal(sp.host_tok_flags, want.host_tok_flags)
            assert tables.shape == (1, t.vocab_size_out) and tables[0].nonzero().flatten().tolist() == sorted(set(eos))
            assert len(rows) == n
            for i, r in enumerate(rows):
                assert (r.temperature, r.top_k, r.top_p, r.timeshift_bias, r.lookback_mask_end, r.max_length, r.eos_set, r.seed, r.cfg_scale) == \
                    (want.temperature, want.top_k, want.top_p, want.timeshift_bias, want.lookback_mask_end, want.max_length, 0, want.seed,
                     want.cfg_scale)
                assert r.rng_row == want.rng_row0 + i and r.cond_mask == (1 << want.n_cond) - 1
                assert list(r.cond_temp)[:want.n_cond] == list(want.cond_temp)[:want.n_cond]


def test_equal_entries_are_one_group_with_one_seed():
    """N equal dicts with an explicit seed and no call index advance the seed's call count ONCE, as the one uniform call would."""
    from mapperatorinator_amd.server import fresh_seed, reset_seed_calls
    tok = rs.tokenizer("bench")
    gk = G(do_sample=True, seed=77)
    reset_seed_calls()
    sp, rows, _ = build_row_sampling(tok, [gk, G(do_sample=True, seed=78), gk, gk], 48)
    assert rows[0].seed == rows[2].seed == rows[3].seed == fresh_seed(77, 0) and rows[1].seed == fresh_seed(78, 0)
    assert [r.rng_row for r in rows] == [0, 0, 1, 2]
    assert build_sampling(tok, gk, 48)[0].seed == fresh_seed(77, 1)         # the next call with that seed is its second
    reset_seed_calls()


def test_build_row_sampling_deduplicates_eos_sets_and_keeps_row_values():
    tok = rs.tokenizer("bench")
    kinds = [G(lookback_time=300), G(lookahead_time=400, temperature=0.7, timeshift_bias=0.5), G(context_type="gd", max_length=30),
             G(lookahead_time=400, top_k=3)]                                 # the last shares group 1's EOS set, not its kwargs
    sp, rows, tables = build_row_sampling(tok, [kinds[i] for i in (0, 1, 2, 3, 0, 1)], 48)
    assert tables.shape == (3, tok.vocab_size_out) and [r.eos_set for r in rows] == [0, 1, 2, 1, 0, 1]
    for i, k in ((0, 0), (1, 1), (2, 2)):
        kw = {n: kinds[k][n] for n in ("lookback_time", "lookahead_time", "context_type")}
        assert tables[i].nonzero().flatten().tolist() == sorted(set(get_eos_token_id(tok, **kw)))
    assert sp.max_length == 48 and [r.max_length for r in rows] == [48, 48, 30, 48, 48, 48]
    assert [round(r.temperature, 6) for r in rows] == [1.0, 0.7, 1.0, 1.0, 1.0, 0.7] and rows[1].timeshift_bias == 0.5
    assert rows[0].lookback_mask_end == build_sampling(tok, kinds[0], 48)[0].lookback_mask_end > sp.ts_start and rows[1].lookback_mask_end == 0
    assert [r.rng_row for r in rows] == [0, 0, 0, 0, 1, 1] and sp.do_sample == 0 and sp.cfg_scale == 1.0


def test_build_row_sampling_builds_the_rule_mask():
    """Rules are per call (token sets and offsets), temperatures and the mask per row: a rule whose temperature equals the row's base
    one is the reference's dropped rule -- masked out, never present with the base temperature."""
    from mapperatorinator_amd.server import get_beat_type_tokens, get_mania_type_tokens, get_scroll_speed_tokens
    tf = Tokenizer.from_json(f"{GOLDEN}/tokenizer_types_first.json")
    t = dict(types_first=True, context_type="map")
    kinds = [G(**t, timing_temperature=0.5, mania_column_temperature=0.6, lookback_time=200),
             G(**t, temperature=1.1, timing_temperature=1.1, mania_column_temperature=0.3, taiko_hit_temperature=0.9),
             G(**t, temperature=1.2, timing_temperature=0.8),
             G(**t)]
    sp, rows, _ = build_row_sampling(tf, kinds, 48)
    assert sp.n_cond == 3 and list(sp.cond_offset) == [1, 3, 1]
    assert [r.cond_mask for r in rows] == [0b011, 0b110, 0b001, 0]
    assert [round(x, 6) for x in rows[0].cond_temp][:2] == [0.5, 0.6] and [round(x, 6) for x in rows[1].cond_temp][1:] == [0.3, 0.9]
    for j, ids in enumerate((get_beat_type_tokens(tf), get_mania_type_tokens(tf), get_scroll_speed_tokens(tf))):
        assert np.nonzero(sp.host_tok_flags & (FLAG_COND0 << j))[0].tolist() == sorted(ids)
    assert sp.lookback_types_first == 1 and [r.lookback_mask_end > 0 for r in rows] == [True, False, False, False]
    # two rules only (nobody has a mania rule): the taiko rule is rule 1 of the call
    sp, rows, _ = build_row_sampling(tf, [G(**t, taiko_hit_temperature=0.9), G(**t, timing_temperature=0.4)], 48)
    assert sp.n_cond == 2 and list(sp.cond_offset)[:2] == [1, 1] and [r.cond_mask for r in rows] == [0b10, 0b01]
    assert np.nonzero(sp.host_tok_flags & (FLAG_COND0 << 1))[0].tolist() == sorted(get_scroll_speed_tokens(tf))


@pytest.mark.parametrize("key,other", [("do_sample", dict(do_sample=True)), ("cfg_scale", dict(cfg_scale=2.0)),
                                       ("types_first", dict(types_first=True)), ("num_beams", dict(num_beams=2)),
                                       ("pad_token_id", dict(pad_token_id=3)), ("cross_kv_fp8", dict(cross_kv_fp8=True)),
                                       ("self_kv_fp8", dict(self_kv_fp8=True)), ("precision", dict(precision="bf16")),
                                       ("conditional_temperature_per_row", dict(conditional_temperature_per_row=True))])
def test_build_row_sampling_names_the_per_call_key_that_differs(key, other):
    tok = rs.tokenizer("bench")
    with pytest.raises(ValueError, match=key):
        build_row_sampling(tok, [G(), G(**other)], 48)
    if key != "num_beams":
        sp, rows, _ = build_row_sampling(tok, [G(**other), G(**other, temperature=0.5)], 48)   # agreeing rows are fine
        assert len(rows) == 2
        assert row_call_key(G(**other)) != row_call_key(G()) and row_call_key(G(**other, top_k=4)) == row_call_key(G(**other))
    else:
        with pytest.raises(ValueError, match="num_beams"):
            build_row_sampling(tok, [G(**other), G(**other)], 48)
        assert row_call_key(G(**other)) is None
    with pytest.raises(ValueError, match="no rows"):
        build_row_sampling(tok, [], 48)


# ---- the scheduler on a stub engine -----------------------------------------------------------------------------------------------
class _Engine:
    """What SequentialWindowScheduler needs of an engine, on the CPU; `decode` appends one EOS id of each row's own set and records
    what it was called with."""

    def __init__(self, vocab_out):
        import contextlib
        self.device, self.dtype = torch.device("cpu"), torch.bfloat16
        self.packed = types.SimpleNamespace(vocab_out=vocab_out)
        self.calls = []
        self._ctx = contextlib.nullcontext

    def _enter(self): pass
    def _leave(self): pass
    def synchronize(self): pass
    def on_stream(self): return self._ctx()
    def mel(self, audio): return audio
    def encode_mel(self, mel, row_bias=None): return mel

    def cross_kv(self, enc):
        return enc.abs().sum(-1).view(1, 1, -1, 1, 1, 1).expand(1, 2, -1, 1, 1, 64).contiguous()

    def decode(self, kv, prompt, prompt_mask, eos_table, sampling, forced=None, dump_logits=False, poll_every=16, kv_fp8=None,
               self_kv_fp8=False, row_sampling=None):
        B, P = prompt.shape
        R = B // 2 if sampling.cfg_scale > 1.0 else B
        tokens = torch.full((B, sampling.max_length), int(sampling.pad_id), dtype=torch.int32)
        tokens[:, :P] = prompt
        rows = None
        if row_sampling is not None:
            _, rows, tables = row_sampling
            assert len(rows) == R
            for r in range(R):                          # the LAST id of the row's own EOS set
                tokens[B - R + r, P] = int(tables[rows[r].eos_set].nonzero().max())
        else:
            tokens[:, P] = int(eos_table.nonzero().max())
        self.calls.append(dict(B=B, sp=sampling, rows=rows, songs=kv[0, 0, :, 0, 0, 0].tolist()))
        return tokens, torch.tensor([P + 1], dtype=torch.int32), None


def _songs(tok, lengths, got, guided=(), **common):
    """one job per song: window w of song i asks for the reference's EOS windows (no lookback on the first window, no lookahead on
    the last) and a temperature of its own song"""
    from mapperatorinator_amd.scheduler import SongJob
    jobs = []
    for i, n in enumerate(lengths):
        def prompt_fn(w, i=i, n=n):
            ask = dict(decoder_input_ids=torch.tensor([[tok.sos_id] + [40 + i] * (1 + (i + w) % 3)]),
                       generate_kwargs=dict(lookback_time=300 if w else 0, lookahead_time=400 if w != n - 1 else 0))
            if i in guided:
                ask["negative_prompt"] = torch.tensor([[tok.sos_id]])
            return ask
        frames = torch.full((n, 16), float(i + 1)) + torch.arange(n)[:, None] * 100.0      # "K/V" value = 16 * (i + 1 + 100 w)
        jobs.append(SongJob(frames=frames, prompt_fn=prompt_fn, on_result=lambda w, row, st, i=i: got.setdefault((i, w), row.tolist()),
                            generate_kwargs=dict(G(max_length=24, temperature=1.0 + 0.1 * i, seed=9, cfg_scale=2.0 if i in guided else 1.0),
                                                 **common)))
    return jobs


def _run(tok, lengths, merge, **kw):
    from mapperatorinator_amd.scheduler import SequentialWindowScheduler
    eng = _Engine(tok.vocab_size_out)
    model = types.SimpleNamespace(engine=eng, config=types.SimpleNamespace(max_target_positions=24))
    got = {}
    sched = SequentialWindowScheduler(model, tok, decode_batch=8, **({} if merge is None else dict(merge_kwargs=merge)))
    stats = sched.run(_songs(tok, lengths, got, **kw))
    return eng, got, stats


def test_scheduler_merges_the_groups_of_a_wave_into_one_call():
    tok = rs.tokenizer("bench")
    lengths = [1, 2, 3]          # wave 0: three songs, each with its own kwargs; wave 1: a last and a middle window; wave 2: one
    default, got_d, st_d = _run(tok, lengths, None)
    off, got_off, _ = _run(tok, lengths, False)
    merged, got_m, st_m = _run(tok, lengths, True)
    assert [c["B"] for c in default.calls] == [c["B"] for c in off.calls] == [1, 1, 1, 1, 1, 1] and got_d == got_off
    assert all(c["rows"] is None for c in default.calls)
    assert [c["B"] for c in merged.calls] == [3, 2, 1] and st_m["decode_calls"] == 3 and st_d["decode_calls"] == 6
    assert got_m == got_d and len(got_m) == 6                  # every window ends on the last id of ITS EOS set, cut there
    ts1 = [v for k, v in tok.event_end.items() if k.name == "TIME_SHIFT"][0]
    assert got_m[(1, 0)][-1] == ts1 - 1 and got_m[(0, 0)][-1] == tok.eos_id      # lookahead window set / the plain set
    # wave 0 in one call: each row carries the settings of its own window
    call = merged.calls[0]
    assert call["songs"] == [16.0, 32.0, 48.0] and call["sp"].cond_per_row == 1
    assert [round(r.temperature, 6) for r in call["rows"]] == [1.0, 1.1, 1.2]
    assert [r.eos_set for r in call["rows"]] == [0, 1, 1] and [r.max_length for r in call["rows"]] == [24, 24, 24]
    assert [r.lookback_mask_end > 0 for r in merged.calls[1]["rows"]] == [True, True]


def test_scheduler_keeps_the_seed_and_rng_row_of_the_windows_own_group():
    """Sampled rows: what a window draws with must not depend on merge_kwargs.  The default policy makes one call per group, in group
    order, each with the next call index of its seed; rows of a group count from RNG row 0."""
    tok = rs.tokenizer("bench")
    lengths = [2, 2, 2, 3]
    default, _, _ = _run(tok, lengths, False, do_sample=True)
    merged, _, _ = _run(tok, lengths, True, do_sample=True)
    want = {}
    for c in default.calls:
        for r, song in enumerate(c["songs"]):
            want[song] = (c["sp"].seed, c["sp"].rng_row0 + r)
    have = {song: (c["rows"][r].seed, c["rows"][r].rng_row) for c in merged.calls for r, song in enumerate(c["songs"])}
    assert have == want and len({s for s, _ in want.values()}) == len(default.calls) > len(merged.calls)


def test_scheduler_keeps_guided_and_unguided_windows_apart():
    tok = rs.tokenizer("bench")
    merged, got, stats = _run(tok, [1, 1, 1, 1], True, guided=(1, 3))
    assert sorted(c["B"] for c in merged.calls) == [2, 4] and stats["decode_calls"] == 2        # 2 plain rows; 2 pairs
    guided = [c for c in merged.calls if c["B"] == 4][0]
    assert guided["sp"].cfg_scale > 1.0 and guided["songs"] == [32.0, 64.0] and len(guided["rows"]) == 2
    assert all(r.cfg_scale == 2.0 for r in guided["rows"]) and len(got) == 4


def _run_jobs(tok, jobs, engine=None, merge=True):
    from mapperatorinator_amd.scheduler import SequentialWindowScheduler
    eng = engine or _Engine(tok.vocab_size_out)
    model = types.SimpleNamespace(engine=eng, config=types.SimpleNamespace(max_target_positions=24))
    sched = SequentialWindowScheduler(model, tok, decode_batch=8, merge_kwargs=merge)
    return eng, sched.run(jobs)


def test_scheduler_decodes_a_beam_group_by_the_default_route(monkeypatch):
    """Beams have no row form: under merge_kwargs a beam group goes through the beam search as it does by default, and the other groups
    of its wave still share one call."""
    from mapperatorinator_amd import beam
    tok = rs.tokenizer("bench")
    searched = []

    def beam_search(eng, kv, prompts, masks, eos, sp, nb, sample_fn=None, kv_fp8=None):
        searched.append(dict(windows=prompts.shape[0], nb=nb, songs=kv[0, 0, :, 0, 0, 0].tolist()))
        return torch.cat([prompts, torch.full((prompts.shape[0], 1), max(int(e) for e in eos))], 1)
    monkeypatch.setattr(beam, "beam_search", beam_search)
    got = {}
    jobs = _songs(tok, [1, 1, 1], got)
    jobs[1].generate_kwargs["num_beams"] = 2
    eng, stats = _run_jobs(tok, jobs)
    assert searched == [dict(windows=1, nb=2, songs=[32.0])]
    assert [(c["B"], c["songs"]) for c in eng.calls] == [(2, [16.0, 48.0])] and eng.calls[0]["rows"] is not None
    assert stats["decode_calls"] == 2 and len(got) == 3 and got[(1, 0)][-1] == tok.eos_id


def test_scheduler_keeps_a_group_apart_whose_cap_cannot_hold_the_merged_prompt_width():
    """max_length counts columns of the call, the left padding included: song 0 (prompt of 2 ids, max_length 3) decodes among its own
    prompts but not beside song 2's prompt of 4 ids, so it keeps a call of its own; the others merge."""
    tok = rs.tokenizer("bench")
    got = {}
    jobs = _songs(tok, [1, 1, 1], got)                         # prompt widths 2, 3, 4
    jobs[0].generate_kwargs["max_length"] = 3
    eng, stats = _run_jobs(tok, jobs)
    assert [(c["B"], c["songs"], c["rows"] is None) for c in eng.calls] == [(1, [16.0], True), (2, [32.0, 48.0], False)]
    assert stats["decode_calls"] == 2 and got[(0, 0)] == [tok.sos_id, 40, tok.eos_id]


class _NoEosBehindPadding(_Engine):
    """rows that a merged call padded on the left run to the call's last column without an EOS id"""

    def decode(self, kv, prompt, prompt_mask, eos_table, sampling, *a, row_sampling=None, **kw):
        tokens, n, _ = super().decode(kv, prompt, prompt_mask, eos_table, sampling, *a, row_sampling=row_sampling, **kw)
        if row_sampling is not None:
            tokens[prompt_mask[:, 0] == 0, prompt.shape[1]] = 7
        return tokens, n, None


def test_scheduler_redoes_a_merged_row_as_the_default_policy_does():
    """A merged row that ends without an EOS id short of its cap, because of the call's left padding, is decoded again the way the default
    policy redoes a row: in a uniform call of its own group and prompt length, with the NEXT call index of its seed."""
    tok = rs.tokenizer("bench")
    got = {}
    eng, stats = _run_jobs(tok, _songs(tok, [1, 1, 1], got, do_sample=True), engine=_NoEosBehindPadding(tok.vocab_size_out))
    assert [(c["B"], c["songs"], c["rows"] is None) for c in eng.calls] == [(3, [16.0, 32.0, 48.0], False), (1, [16.0], True), (1, [32.0], True)]
    first = eng.calls[0]["rows"]
    for r, c in enumerate(eng.calls[1:]):
        want, _ = build_sampling(tok, dict(G(max_length=24, temperature=1.0 + 0.1 * r, seed=9, do_sample=True), lookback_time=0, lookahead_time=0,
                                           conditional_temperature_per_row=True, seed_call_index=3 + r), 24)
        assert c["sp"].seed == want.seed != first[r].seed and c["sp"].rng_row0 == 0 and round(c["sp"].temperature, 6) == round(1.0 + 0.1 * r, 6)
    assert stats["decode_calls"] == 3 and stats["windows"] == 3 and sorted(got) == [(0, 0), (1, 0), (2, 0)]
    assert got[(0, 0)][-1] == tok.eos_id and got[(2, 0)][-1] == tok.eos_id


# ---- the batcher on a stub generate_fn ----------------------------------------------------------------------------------------------
def _batcher(merge, max_batch_size=8):
    calls = []

    def generate_fn(model, tokenizer, model_kwargs, generate_kwargs):
        calls.append((model_kwargs["decoder_input_ids"].clone(), generate_kwargs))
        ids = model_kwargs["decoder_input_ids"]
        return torch.cat([ids, ids[:, -1:] + 1], 1), dict(generated_tokens_per_sample=[1] * ids.shape[0], elapsed_seconds=0.5)
    tok = rs.tokenizer("bench")
    b = RequestBatcher(None, tok, max_batch_size=max_batch_size, generate_fn=generate_fn, **({} if merge is None else dict(merge_kwargs=merge)))
    b.prefetch = False
    return b, calls


def _request(rows, width, first):
    ids = torch.arange(rows * width).reshape(rows, width) + first
    return dict(inputs=torch.zeros(rows, 4), decoder_input_ids=ids)


def test_batcher_merges_two_kwargs_groups():
    a, c, d = G(temperature=0.8, seed=4), G(lookahead_time=300, seed=4), G(do_sample=True)
    for merge in (None, False):
        b, calls = _batcher(merge)
        recs = [b.submit(_request(2, 3, 100), a), b.submit(_request(3, 2, 200), c), b.submit(_request(1, 3, 300), a)]
        assert b.drain() == 2 and [x[0].shape[0] for x in calls] == [3, 3] and all(isinstance(x[1], dict) for x in calls)
        assert all(r["done"] for r in recs)
    b, calls = _batcher(True)
    recs = [b.submit(_request(2, 3, 100), a), b.submit(_request(3, 2, 200), c), b.submit(_request(1, 3, 300), a),
            b.submit(_request(2, 2, 400), d)]
    assert b.drain() == 2 and [x[0].shape[0] for x in calls] == [6, 2]        # greedy groups merged; the sampled one on its own
    per_row = calls[0][1]
    assert isinstance(per_row, list) and len(per_row) == 6
    # the first group's requests, then the second group's; each group with the next call index of its seed
    assert [g["temperature"] for g in per_row] == [0.8, 0.8, 0.8, 1.0, 1.0, 1.0] and [g["lookahead_time"] for g in per_row] == [0, 0, 0, 300, 300, 300]
    assert [g["seed_call_index"] for g in per_row] == [0, 0, 0, 1, 1, 1]
    assert calls[0][0][:, -1].tolist() == [102, 105, 302, 201, 203, 205] and calls[0][0][3, 0] == 0   # the narrower request is left-padded
    for r, want in zip(recs, ([[100, 101, 102, 103], [103, 104, 105, 106]], [[200, 201, 202], [202, 203, 204], [204, 205, 206]])):
        assert r["done"] and r["result"]["output"].tolist() == want
    assert recs[3]["done"] and isinstance(calls[1][1], list) and calls[1][1][0]["do_sample"] is True
    # no room left after the first group: the second group waits for the next batch
    b, calls = _batcher(True, max_batch_size=2)
    b.submit(_request(2, 3, 100), a), b.submit(_request(1, 2, 200), c)
    assert b.drain() == 2 and [len(x[1]) for x in calls] == [2, 1]


def test_batcher_keeps_a_group_apart_whose_cap_cannot_hold_the_merged_prompt_width():
    """max_length counts columns of the collated batch: a group capped at 3 decodes its own prompts of 2 ids, not beside prompts of 3"""
    short, wide = G(max_length=3), G(lookahead_time=300)
    b, calls = _batcher(True)
    b.submit(_request(2, 2, 100), short), b.submit(_request(2, 3, 200), wide), b.submit(_request(1, 2, 300), G(temperature=0.7))
    assert b.drain() == 2 and [x[0].shape for x in calls] == [(3, 2), (2, 3)]
    assert [g["max_length"] for g in calls[0][1]] == [3, 3, rs.TGT] and [g["lookahead_time"] for g in calls[1][1]] == [300, 300]
    # the same when the capped group comes second
    b, calls = _batcher(True)
    b.submit(_request(2, 3, 200), wide), b.submit(_request(2, 2, 100), short)
    assert b.drain() == 2 and [x[0].shape for x in calls] == [(2, 3), (2, 2)]
