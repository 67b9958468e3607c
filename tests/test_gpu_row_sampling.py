"""-m gpu: the row-settings decode (`mh_t5_generate_rows`, `T5Engine.decode(row_sampling=)`; contract in include/mapperhip.h).

The yardstick is the uniform entry (mh_t5_generate / mh_t5_generate_skv8, pinned to the reference by the goldens): a row decoded in a
mixed call must be BIT-EQUAL to the same row decoded in a uniform call made of the rows that share its kwargs -- token ids up to the
row's end and its rows of the logits dump.  No tolerance anywhere in this file.

Inputs: mh_testing.row_sampling (tiny dims, 251 frames, tgt 48, seeded weights)."""
import ctypes as C
import os

import pytest
import torch

from mh_testing import row_sampling as rs

pytestmark = pytest.mark.gpu
TF_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tokenizer_types_first.json")
G = rs.gen_kwargs


def setup(kind, dtype, B, widths=None):
    tok = rs.tokenizer(kind, TF_JSON)
    m = rs.model(kind, dtype, tok)
    kv = rs.cross_kv(m, kind, B)
    prompt, mask = rs.prompts(tok, widths if widths is not None else [(5 * r) % 7 + 1 for r in range(B)])
    return tok, m, kv, prompt, mask


def check_groups(m, tok, kv, prompt, mask, gks, neg=None, **modes):
    """one mixed call against one uniform call per distinct kwargs dict; returns (mixed, {group index: ends})"""
    mixed = rs.run_rows(m, tok, kv, prompt, mask, gks, neg=neg, **modes)
    P = prompt.shape[1]
    groups = {}
    for r, gk in enumerate(gks):
        groups.setdefault(id(gk), (gk, []))[1].append(r)
    ends = {}
    for n, (gk, rows) in enumerate(groups.values()):
        uni = rs.run_uniform(m, tok, kv, prompt, mask, gk, rows, neg=neg, **modes)
        ends[n] = rs.assert_rows_equal_uniform(mixed, uni, rows, P)
    assert mixed["n_cols"] == max(max(e) for e in ends.values()) + 1
    return mixed, ends


def three_groups():
    """A: the lookback EOS set with the lookback mask; B: the lookahead EOS set, temperature 0.7 and a time-shift bias; C: a context EOS
    set with a smaller max_length"""
    return [G(lookback_time=300), G(lookahead_time=400, temperature=0.7, timeshift_bias=0.5), G(context_type="gd", max_length=30)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("B", [18, 5])
def test_greedy_rows_of_three_groups_equal_their_uniform_calls(B, dtype):
    """18 rows are two chains (the second chain's sampler sees chain-local logits and GLOBAL row entries), 5 rows one; the groups are
    interleaved (row r belongs to group r % 3) and the prompts ragged (1 .. 7 tokens, left-padded with a mask)."""
    tok, m, kv, prompt, mask = setup("bench", dtype, B)
    cfg = m.engine.packed.cfg
    assert m.engine.lib.mh_t5_decode_chains_cfg(C.byref(cfg), 18) == 2 and m.engine.lib.mh_t5_decode_chains_cfg(C.byref(cfg), 5) == 1
    kinds = three_groups()
    mixed, ends = check_groups(m, tok, kv, prompt, mask, [kinds[r % 3] for r in range(B)])
    assert max(ends[2]) <= 29                                           # group C ends at its own cap at the latest
    # the settings matter: group B's rows under group A's settings score differently from their first step on
    other = rs.run_uniform(m, tok, kv, prompt, mask, kinds[0], list(range(1, B, 3)))
    P = prompt.shape[1]
    assert not torch.equal(other["logits"][P], mixed["logits"][P, 1::3])


@pytest.mark.parametrize("kind,dtype", [("bench", torch.float32), ("big", torch.bfloat16)], ids=["bench-fp32", "big-bf16"])
def test_sampled_rows_equal_their_uniform_calls(kind, dtype):
    """Per-row temperature, top_k, top_p, seed and rng_row (two rows per group: RNG rows offset, offset + 1), equal prompt width.
    `bench` is the benchmark vocabulary (the register path), `big` has more than 4096 ids (the memory path)."""
    B = 6
    tok, m, kv, prompt, mask = setup(kind, dtype, B, widths=[3] * B)
    assert (tok.vocab_size_out > 4096) == (kind == "big")
    kinds = [G(do_sample=True, temperature=1.0, top_p=0.9, seed=11, seed_call_index=0),
             G(do_sample=True, temperature=1.4, top_k=20, seed=12, seed_call_index=0, lookahead_time=300),
             G(do_sample=True, temperature=0.8, top_k=50, top_p=0.7, seed=13, seed_call_index=0, rng_row_offset=5, timeshift_bias=0.3)]
    mixed, _ = check_groups(m, tok, kv, prompt, None, [kinds[r % 3] for r in range(B)])
    greedy = rs.run_uniform(m, tok, kv, prompt, None, G(), list(range(B)))
    assert not torch.equal(greedy["tokens"][:, :mixed["n_cols"]], mixed["tokens"][:, :mixed["n_cols"]]), "nothing was drawn"
    # rows of one group share seed and settings and differ in the RNG row alone
    same = rs.run_uniform(m, tok, kv[:, :, [0, 0]], prompt[[0, 0]], None, kinds[0], [0, 1])
    assert not torch.equal(same["tokens"][0], same["tokens"][1])


def test_guided_pairs_with_their_own_scale():
    """9 pairs (18 decoded rows, one chain under guidance); cfg_scale differs per pair, and so do other settings."""
    B = 9
    tok, m, kv, prompt, mask = setup("bench", torch.float32, B)
    neg, _ = rs.prompts(tok, [(5 * r) % 7 + 1 for r in range(B)], seed=4)      # other ids of the same widths
    kinds = [G(cfg_scale=1.5), G(cfg_scale=2.0, lookahead_time=400), G(cfg_scale=3.0, temperature=0.9)]
    mixed, _ = check_groups(m, tok, kv, prompt, mask, [kinds[r % 3] for r in range(B)], neg=neg)
    P = prompt.shape[1]
    other = rs.run_uniform(m, tok, kv, prompt, mask, kinds[0], [1, 4, 7], neg=neg)
    assert not torch.equal(other["logits"][P], mixed["logits"][P, 1::3])


def test_types_first_rows_with_their_own_rules_and_lookback():
    """The types_first tokenizer: per-row conditional temperatures, per-row lookback ends under the renormalising branch, and one
    group whose timing temperature equals its base one -- the reference drops that rule for it, so its rows must go on to the
    mania-column rule (0.3) where the timing rule would have matched first.  Every prompt ends ... CIRCLE, x, BEAT."""
    from mapperatorinator_amd.server import _ev, build_row_sampling
    B = 6
    tok, m, kv, prompt, mask = setup("tf", torch.float32, B, widths=[4, 6, 5, 7, 4, 6])
    prompt[:, -1], prompt[:, -3] = _ev(tok.event_start, "BEAT"), _ev(tok.event_start, "CIRCLE")
    tf = dict(types_first=True, conditional_temperature_per_row=True, context_type="map")
    kinds = [G(**tf, timing_temperature=0.5, mania_column_temperature=0.6, lookback_time=200),
             G(**tf, temperature=1.1, timing_temperature=1.1, mania_column_temperature=0.3, taiko_hit_temperature=0.9),
             G(**tf, temperature=1.2, timing_temperature=0.8, lookback_time=500, lookahead_time=300)]
    gks = [kinds[r % 3] for r in range(B)]
    sp, rows, _ = build_row_sampling(tok, gks, rs.TGT)
    assert sp.n_cond == 3 and [rows[r].cond_mask for r in range(3)] == [0b011, 0b110, 0b001] and sp.lookback_types_first == 1
    mixed, ends = check_groups(m, tok, kv, prompt, mask, gks)
    P = prompt.shape[1]
    # group 1's first step ran at the mania-column temperature: its scores are the raw-temperature ones of group 1 times 1.1 / 0.3
    base = rs.run_uniform(m, tok, kv, prompt, mask, G(**tf, temperature=1.1), [1, 4])
    a, b = mixed["logits"][P, [1, 4]], base["logits"][P]
    fin = torch.isfinite(a)
    assert torch.equal(fin, torch.isfinite(b)) and torch.allclose(a[fin], b[fin] * (1.1 / 0.3), rtol=1e-5)
    # the renormalising branch ran: a lookback row produced a timed event before its end, so its next step renormalised
    timed = torch.as_tensor(sp.host_tok_flags & 1).bool()
    assert any(bool(timed[mixed["tokens"][r, P:e]].any()) for n in (0, 2) for r, e in zip(range(n, B, 3), ends[n]))


def test_rows_with_both_fp8_caches():
    """self_kv_fp8 and cross_kv_fp8 together (bf16 storage): the row form over the e4m3 shadow and the e4m3 cross K/V."""
    B = 5
    tok, m, kv, prompt, mask = setup("bench", torch.bfloat16, B)
    kinds = three_groups()
    gks = [kinds[r % 3] for r in range(B)]
    mixed, _ = check_groups(m, tok, kv, prompt, mask, gks, self_kv_fp8=True, cross_kv_fp8=True)
    plain = rs.run_rows(m, tok, kv, prompt, mask, gks)
    fin = torch.isfinite(plain["logits"][prompt.shape[1]])
    assert not torch.equal(plain["logits"][prompt.shape[1]][fin], mixed["logits"][prompt.shape[1]][fin]), "the fp8 modes were not on"


def test_a_row_ends_at_its_own_max_length():
    """Caps 20, 33 and 48 with the plain EOS set: every row runs to its cap, holds pad_id behind it, and n_steps_out is the largest."""
    B = 6
    tok, m, kv, prompt, mask = setup("bench", torch.float32, B)
    kinds = [G(max_length=20), G(max_length=33), G(max_length=48)]
    mixed, ends = check_groups(m, tok, kv, prompt, mask, [kinds[r % 3] for r in range(B)])
    assert ends == {0: [19, 19], 1: [32, 32], 2: [47, 47]} and mixed["n_cols"] == 48
    assert bool((mixed["tokens"][0::3, 20:] == 0).all()) and bool((mixed["tokens"][1::3, 33:] == 0).all())
    assert bool((mixed["tokens"][2::3, 20:] != 0).any())


def test_step_graph_cache_keys_the_forms_apart_and_follows_the_contents():
    """One engine, in this order: a mixed call; calls at the same pointers with OTHER contents (until the allocator hands the caller's
    buffers out at the addresses of a captured graph: a replay, which must read the new contents); a plain uniform call, which
    must not replay the row form's graph.  Every result equals that of an engine that captures per call (decode_graph_cache = 0)."""
    from mapperatorinator_amd import _lib
    B = 5
    tok = rs.tokenizer("bench")
    one, percall = rs.model("bench", torch.float32, tok, fresh=True), rs.model("bench", torch.float32, tok, options=dict(decode_graph_cache=0))
    prompt, mask = rs.prompts(tok, [(5 * r) % 7 + 1 for r in range(B)])
    kvs = {id(e): rs.cross_kv(e, "bench", B) for e in (one, percall)}
    lib = _lib.load()

    def stats():
        h, mi = C.c_long(0), C.c_long(0)
        lib.mh_t5_step_graph_cache_stats(C.byref(h), C.byref(mi), 0)
        return h.value, mi.value

    def same(a, b):
        return a["n_cols"] == b["n_cols"] and torch.equal(a["tokens"], b["tokens"]) and \
            torch.equal(a["logits"][:a["n_cols"]].nan_to_num(), b["logits"][:b["n_cols"]].nan_to_num())
    kinds = three_groups()
    first, second = [kinds[r % 3] for r in range(B)], [kinds[(r + 1) % 3] for r in range(B)]
    want = {k: rs.run_rows(percall, tok, kvs[id(percall)], prompt, mask, gks) for k, gks in (("first", first), ("second", second))}
    want["uniform"] = rs.run_uniform(percall, tok, kvs[id(percall)], prompt, mask, kinds[0], list(range(B)))
    assert not same(want["first"], want["second"])
    h0, m0 = stats()
    assert same(rs.run_rows(one, tok, kvs[id(one)], prompt, mask, first), want["first"])
    h1, m1 = stats()
    assert (h1, m1) == (h0, m0 + 1), "a new engine's first row-form call captures its one chain"
    for _ in range(6):
        assert same(rs.run_rows(one, tok, kvs[id(one)], prompt, mask, second), want["second"])
        if stats()[0] > h1:
            break
    h2, m2 = stats()
    assert h2 > h1, "the row form never replayed a graph: rows / eos_tables moved, or their contents are part of the key"
    assert same(rs.run_uniform(one, tok, kvs[id(one)], prompt, mask, kinds[0], list(range(B))), want["uniform"])
    h3, m3 = stats()
    assert (h3, m3) == (h2, m2 + 1), "the uniform call must capture its own graph, not replay the row form's"
    assert same(rs.run_rows(one, tok, kvs[id(one)], prompt, mask, first), want["first"])


def test_model_generate_rows_and_the_merging_batcher_equal_model_generate_per_group():
    """The host route on a real engine: `model_generate_rows` (audio -> encoder -> `build_row_sampling` -> `T5Engine.generate(row_sampling=)`)
    on a mixed list, and `RequestBatcher(merge_kwargs=True)` with its default `generate_fn`, against `model_generate` on the rows of each
    group: the ids of a row up to its group's last column, pad_id behind it."""
    from mapperatorinator_amd.server import RequestBatcher, model_generate, model_generate_rows
    from mh_testing import synthetic_audio_varied
    B = 6
    tok = rs.tokenizer("bench")
    m = rs.model("bench", torch.float32, tok)
    audio = synthetic_audio_varied(B, (rs.FRAMES - 1) * 128, seed=6)
    prompt, mask = rs.prompts(tok, [(5 * r) % 7 + 1 for r in range(B)])
    kinds = three_groups()
    gks = [kinds[r % 3] for r in range(B)]
    mixed, stats = model_generate_rows(m, tok, dict(inputs=audio, decoder_input_ids=prompt, decoder_attention_mask=mask), gks)
    mixed = mixed.cpu()
    assert mixed.shape[0] == B and prompt.shape[1] < mixed.shape[1] <= rs.TGT and len(stats["generated_tokens_per_sample"]) == B
    uniform = {}
    for n, gk in enumerate(kinds):
        rows = list(range(n, B, 3))
        uni, _ = model_generate(m, tok, dict(inputs=audio[rows], decoder_input_ids=prompt[rows], decoder_attention_mask=mask[rows]), gk)
        uniform[n] = uni = uni.cpu()
        assert uni.shape[1] <= mixed.shape[1]
        assert torch.equal(mixed[rows, :uni.shape[1]], uni), f"group {n}: ids differ from model_generate on the group alone"
        assert bool((mixed[rows, uni.shape[1]:] == 0).all())
    assert mixed.shape[1] == max(u.shape[1] for u in uniform.values()) and uniform[2].shape[1] <= 30

    # one request per group through the batcher (prompts of one width, no mask): one decode call, every request answered as by itself
    batcher = RequestBatcher(m, tok, max_batch_size=8, merge_kwargs=True)
    wide, _ = rs.prompts(tok, [4] * B)
    asks = [dict(inputs=audio[n::3], decoder_input_ids=wide[n::3]) for n in range(3)]
    recs = [batcher.submit(ask, gk) for ask, gk in zip(asks, kinds)]
    assert batcher.drain() == 1 and all(r["done"] and r["error"] is None for r in recs)
    for ask, gk, rec in zip(asks, kinds, recs):
        uni, _ = model_generate(m, tok, ask, gk)
        out, uni = rec["result"]["output"].cpu(), uni.cpu()
        assert torch.equal(out[:, :uni.shape[1]], uni) and bool((out[:, uni.shape[1]:] == 0).all())
