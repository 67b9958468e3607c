"""-m gpu: the e4m3 self-attention cache under the beam search's index table (`self_kv_fp8` with `beam_cache="indexed"`:
mh_t5_step_indexed_skv8, mh_t5_self_kv_fp8_fill; contract in include/mapperhip.h).

1. The table is followed, bit for bit: the same ids through the new entry with reorders applied to the TABLE, and with the identity table
   while the test itself permutes what a copy route would have copied (bf16 rows, shadow bytes, shadow scales): torch.equal logits.
2. The identity table is the greedy mode: caches and shadow bit-equal to what mh_t5_generate_skv8 leaves for the same forced ids, and
   the raw step logits against the hooked oracle under the project's own gate (GAP 0.25, floor + 0.2: tests/test_gpu_self_kv_fp8.py,
   neither re-fitted; the floor is the plain mh_t5_step_indexed run against the plain oracle, measured in the same test).
3. Prefill plus fill: the fill writes quantize_rows of the prefilled bf16 rows and not one byte more; then prompts of 1 / 4 / 9 tokens
   through prefill, fill and the new steps under gate 2.
4. End to end through model_generate and the scheduler at the tiny golden's inputs with a bf16 model."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from mh_testing import beam_skv8, kv_fp8
from test_gpu_beam_cache import N_POS, assert_same_logits, family, fixed_reorders, gen_kwargs, golden_inputs, prefill_case, random_kv
from test_gpu_self_kv_fp8 import EXCESS, GAP, _device_kv, model_for

pytestmark = pytest.mark.gpu


# ---- 1. the table is followed ---------------------------------------------------------------------------------------------------

def table_case(eng, vocab, n_pos, nb, guided=False, fp8=False, what=""):
    G, P = 2, 8
    R = G * nb * (2 if guided else 1)
    ids = torch.randint(3, vocab, (n_pos, R), generator=torch.Generator().manual_seed(100 + nb))
    mask = torch.ones(G, P, dtype=torch.uint8)
    mask[0, :3] = 0                                                        # a ragged left-padded prompt mask: chunk 0 pads 3 columns
    mask = mask.repeat_interleave(nb, 0)
    if guided:
        mask = torch.cat([mask, mask], 0)
    kv = random_kv(eng, R // nb, seed=3)
    kv8 = None
    if fp8:
        eng._enter()
        with eng.on_stream():
            kv8 = eng.cross_kv_fp8(kv)
        eng._leave()
    srcs = fixed_reorders(n_pos, G, nb, seed=7 + nb, double=guided)
    table = beam_skv8.run_steps(eng, kv, kv8, ids, mask, P, nb, srcs, route="table")["logits"]
    moved = beam_skv8.run_steps(eng, kv, kv8, ids, mask, P, nb, srcs, route="permute")["logits"]
    assert table.shape[0] == n_pos and table.abs().max() > 1.0
    assert_same_logits(table, moved, f"{what} {G} x {nb}{' guided' if guided else ''}{' e4m3 cross' if fp8 else ''}")
    # the reorders mattered: the same ids without them give other logits from early on
    m = min(n_pos, 24)
    still = beam_skv8.run_steps(eng, kv, kv8, ids[:m], mask, P, nb, None)["logits"]
    differs = (still != table[:m]).flatten(1).any(dim=1)
    assert torch.equal(still[0], table[0]) and differs.any() and int(differs.nonzero()[0]) <= 8, differs.nonzero().flatten().tolist()
    # ... and the shadow was what the steps read: the bf16 indexed route gives other logits
    plain = beam_skv8.run_steps(eng, kv, kv8, ids[:m], mask, P, nb, srcs[:m], route="table", shadow=False)["logits"]
    assert not torch.equal(plain[1:], table[1:m])


@pytest.mark.parametrize("nb", [2, 3])
@pytest.mark.parametrize("kind", ["t5", "var", "hf"])
def test_step_logits_follow_the_table_bit_for_bit(kind, nb):
    """300 positions at tgt 320 (the key loop's 128- and 256-key trips and a ragged tail), 2 chunks x 2 / 3 beams, hand-made reorders
    with repeats after every step; `var` has layer 1 local with a window shorter than the run (j_first skips whole passes), `hf` the
    LayerNorm prologues and positions from the mask."""
    tok, model = family(kind, torch.bfloat16)
    table_case(model.engine, tok.vocab_size_out, N_POS, nb, what=kind)


def test_guidance_rows_follow_the_first_half():
    """doubled rows, `src` of the second half pointing into the first (`beam_idx.repeat(2)`)"""
    tok, model = family("var", torch.bfloat16)
    table_case(model.engine, tok.vocab_size_out, N_POS, 2, guided=True, what="var")


def test_step_logits_follow_the_table_over_the_e4m3_cross_copy():
    """the whole K/V cache of the step in fp8: the packed cross copy beside the shadow"""
    tok, model = family("var", torch.bfloat16)
    table_case(model.engine, tok.vocab_size_out, N_POS, 2, fp8=True, what="var")


def test_step_logits_follow_the_table_at_the_released_width():
    """`small` dims (d_model 768: the KC = 6 instantiation of the releases), tgt 32, 2 x 2 rows"""
    model = model_for("var-small")
    tok = kv_fp8.case_inputs("var-small")["tok"]
    assert model.engine.packed.cfg.d_model == 768 and model.engine.packed.tgt_len == 32
    table_case(model.engine, tok.vocab_size_out, 30, 2, what="var-small")


# ---- 2. the identity table is the greedy mode -------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["t5", "var", "hf"])
def test_identity_table_is_the_greedy_mode(name):
    """mh_testing.kv_fp8.CASES[name]: 3 rows, tgt 264, 1-token prompts, kv_group = 1, identity table, the hooked oracle's forced ids.
    (a) bf16 caches and shadow (bytes and scales) bit-equal to those mh_t5_generate_skv8 leaves for the same forced ids;
    (b) raw step logits against the hooked oracle under GAP / EXCESS of tests/test_gpu_self_kv_fp8.py.
    Measured (MI355X), floor / worst |dlogit| (excess; allowed +0.2), near-tie flips, real mismatches 0 everywhere: t5 0.339 / 0.440
    (+0.101), 3 of 789; var 0.081 / 0.083 (+0.002), 0 of 789; hf 0.272 / 0.252 (-0.020), 0 of 789 -- the greedy mode's own figures."""
    from mapperatorinator_amd.server import build_sampling
    r = kv_fp8.oracle_runs(name)
    tok, tgt, B = r["tok"], r["spec"]["tgt"], r["spec"]["rows"]
    eng = model_for(name).engine
    assert r["prompt"].shape[1] == 1
    forced, n = r["forced"], tgt - 1                                       # positions 0 .. tgt - 2 are fed
    sp, _ = build_sampling(tok, gen_kwargs(tgt), tgt)
    eng.generate(r["audio"], r["prompt"], r["mask"], [], sp, forced=forced, self_kv_fp8=True)
    eng.synchronize()
    torch.cuda.synchronize()
    k, v, q8, sc = eng.self_kv_caches(B, shadow=True)
    want = [k[..., :n, :].cpu(), v[..., :n, :].cpu(), q8[..., :n, :].cpu(), sc[..., :n].cpu()]
    kv = _device_kv(eng, r["audio"])
    ids = forced.t()[:n].contiguous()                                      # (n, B): the id fed at every position
    run8 = beam_skv8.run_steps(eng, kv, None, ids, None, 1, 1, None, keep=True)
    run16 = beam_skv8.run_steps(eng, kv, None, ids, None, 1, 1, None, shadow=False)
    k2, v2 = beam_skv8.self_caches(eng, run8["ws"], B)
    q2, s2, _ = beam_skv8.shadow_views(eng, run8["sh"], B)
    got = [k2[..., :n, :].cpu(), v2[..., :n, :].cpu(), q2[..., :n, :].cpu(), s2[..., :n].cpu()]
    assert want[0].float().abs().max() > 0 and want[3].abs().max() > 0
    for what, a, b in zip(("bf16 k", "bf16 v", "shadow bytes", "shadow scales"), got, want):
        assert a.shape == b.shape and torch.equal(a, b), f"{what} differ from mh_t5_generate_skv8's"
    beam_skv8.oracle_gate(name, run8["logits"], run16["logits"], torch.stack(r["scores"]), torch.stack(r["scores_plain"]), GAP, EXCESS)


# ---- 3. prefill plus fill ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["t5", "var", "hf"])
def test_fill_quantises_the_prefilled_rows_and_nothing_else(kind):
    """`test` dims, 3 prompts x 2 beams, P = 21 under ragged left padding, a shadow pre-filled with a marker byte: after
    mh_t5_step_prefill + mh_t5_self_kv_fp8_fill, positions < 20 of rows < 3 are mh_testing.kv_fp8.quantize_rows of the bf16 cache rows
    (bytes and scales, bit for bit) and every other byte of the shadow still holds the marker."""
    G, nb, P = 3, 2, 21
    tok, eng, prompt, mask, kv = prefill_case(kind, torch.bfloat16, G, nb, P, seed=31)
    R, n = G * nb, P - 1
    ids = torch.zeros((n, R), dtype=torch.int64)                           # (no step runs: first = n_pos = n)
    run = beam_skv8.run_steps(eng, kv, None, ids, None, P, nb, None, prefill=(prompt, mask, n), keep=True)
    assert run["logits"].shape[0] == 0
    caches = beam_skv8.self_caches(eng, run["ws"], R)
    q8, sc, slack = beam_skv8.shadow_views(eng, run["sh"], R)
    marker = beam_skv8.MARKER
    assert bool((run["sh"][slack] == marker).all())
    sc_bytes = sc.view(torch.uint8).view(*sc.shape, 4)
    for i, x in enumerate(caches):
        x = x[:, :G, :, :n].cpu()
        assert x.float().abs().max() > 0
        q_ref, s_ref = kv_fp8.quantize_rows(x)
        assert torch.equal(q8[:, i, :G, :, :n].cpu(), q_ref), ("k", "v")[i]
        assert torch.equal(sc[:, i, :G, :, :n].cpu(), s_ref), ("k", "v")[i]
        assert bool((q8[:, i, G:] == marker).all()) and bool((q8[:, i, :G, :, n:] == marker).all()), "bytes outside the prompt rows written"
        assert bool((sc_bytes[:, i, G:] == marker).all()) and bool((sc_bytes[:, i, :G, :, n:] == marker).all()), "scales outside written"


def test_prompted_rows_through_prefill_fill_and_the_new_steps():
    """case `var-prompt9` (prompts of 1 / 4 / 9 tokens, left-padded with a mask; the oracle's hook with P = 9): positions 0 .. 7 through
    mh_t5_step_prefill, quantised by the fill, then every position from 8 on through mh_t5_step_indexed_skv8 with kv_group = 1; gate 2(b).
    Measured (MI355X): floor 0.074, worst |dlogit| 0.102 (+0.028; allowed +0.2), 0 flips of 765 steps."""
    name = "var-prompt9"
    r = kv_fp8.oracle_runs(name)
    tgt, B, P = r["spec"]["tgt"], r["spec"]["rows"], r["prompt"].shape[1]
    eng = model_for(name).engine
    assert P == 9 and torch.equal(r["forced"][:, :P], r["prompt"])
    kv = _device_kv(eng, r["audio"])
    ids = r["forced"].t()[:tgt - 1].contiguous()
    prompts = r["prompt"].to(eng.device, torch.int32).contiguous()
    mask = r["mask"].to(torch.uint8)
    pre = (prompts, mask.to(eng.device).contiguous(), P - 1)
    lg8 = beam_skv8.run_steps(eng, kv, None, ids, mask, P, 1, None, prefill=pre)["logits"]
    lg16 = beam_skv8.run_steps(eng, kv, None, ids, mask, P, 1, None, prefill=pre, shadow=False)["logits"]
    beam_skv8.oracle_gate(name, lg8, lg16, torch.stack(r["scores"]), torch.stack(r["scores_plain"]), GAP, EXCESS)


# ---- 4. end to end ----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def golden_bf16():
    """the inputs of tests/golden/t5_tiny_beam.npz with a bf16 model"""
    from mapperatorinator_amd import Tokenizer
    from mapperatorinator_amd.modeling import MapperatorinatorHIP
    from mapperatorinator_amd.t5_engine import T5_PRESETS
    from mh_testing import DIVERSE_GAINS, random_t5_state_dict, synthetic_audio_varied
    g = np.load(f"{GOLDEN}/t5_tiny_beam.npz")
    src, tgt = int(g["src"]), int(g["tgt"])
    tok = Tokenizer.benchmark_vocab(src_seq_len=src)
    sd = random_t5_state_dict(T5_PRESETS["tiny"], tok.vocab_size_in, tok.vocab_size_out, seed=int(g["wseed"]),
                              lm_head_gain=float(g["gain"]), gains=DIVERSE_GAINS)
    audio = synthetic_audio_varied(g["prompt"].shape[0], int(g["ns"]), seed=int(g["aseed"]))
    model = MapperatorinatorHIP(sd, T5_PRESETS["tiny"], vocab_size_in=tok.vocab_size_in, vocab_size_out=tok.vocab_size_out,
                                src_seq_len=src, tgt_seq_len=tgt, dtype=torch.bfloat16, device="cuda")
    return g, tok, model, audio, tgt


ENTRIES = ("mh_t5_step", "mh_t5_step_fp8", "mh_t5_reorder_cache", "mh_t5_step_indexed", "mh_t5_reorder_index", "mh_t5_step_prefill",
           "mh_t5_step_indexed_skv8", "mh_t5_self_kv_fp8_fill")


def count_calls(monkeypatch, lib):
    """counts per entry (as test_gpu_beam_cache.count_calls, with the two new entries), the row count of every new step, and the
    reorders that permuted (read back: a test-only synchronisation)"""
    from mapperatorinator_amd import beam as _beam
    calls = dict({name: 0 for name in ENTRIES}, permuting=0, rows=[])
    for name in ENTRIES:
        def counted(*a, _f=getattr(lib, name), _n=name):
            calls[_n] += 1
            if _n == "mh_t5_step_indexed_skv8":
                calls["rows"].append(int(a[4]))
            return _f(*a)
        monkeypatch.setattr(lib, name, counted)
    real = _beam._IndexedCache.reorder

    def reorder(self, src, n_pos):
        calls["permuting"] += int(not torch.equal(src.cpu(), torch.arange(src.numel(), dtype=src.dtype)))
        return real(self, src, n_pos)
    monkeypatch.setattr(_beam._IndexedCache, "reorder", reorder)
    return calls


@pytest.mark.parametrize("prefill", [False, True], ids=["indexed", "indexed+prefill"])
@pytest.mark.parametrize("nb", [2, 4])
def test_model_generate_runs_the_new_entries(monkeypatch, nb, prefill):
    """`model_generate(num_beams, beam_cache="indexed", self_kv_fp8=True)`: the new entries ran, none of the others did, the search
    reordered, and the kernel bookkeeping and the torch-op bookkeeping return the same ids; with the default beam_cache the same
    kwargs still raise."""
    from mapperatorinator_amd import _lib
    from mapperatorinator_amd.server import model_generate
    g, tok, model, audio, tgt = golden_bf16()
    mk = golden_inputs(g, audio, False)
    P = mk["decoder_input_ids"].shape[1]
    gk = gen_kwargs(tgt, num_beams=nb, temperature=1.2, beam_cache="indexed", self_kv_fp8=True, beam_prefill=prefill)
    calls = count_calls(monkeypatch, _lib.load())
    got = {}
    for use_kernel in (True, False):
        got[use_kernel], _ = model_generate(model, tok, mk, dict(gk, beam_use_kernel=use_kernel))
    assert torch.equal(got[True], got[False]), (got[True].tolist(), got[False].tolist())
    n_new = got[True].shape[1] - P
    assert n_new > 0 and calls["mh_t5_step_indexed_skv8"] >= 2 * n_new and calls["mh_t5_reorder_index"] >= 2 * n_new
    assert calls["mh_t5_step"] == calls["mh_t5_step_fp8"] == calls["mh_t5_reorder_cache"] == calls["mh_t5_step_indexed"] == 0
    assert calls["mh_t5_step_prefill"] == calls["mh_t5_self_kv_fp8_fill"] == (2 if prefill and P > 1 else 0)
    assert calls["permuting"] >= 1, "the search never reordered: the run shows nothing"
    assert set(calls["rows"]) == {mk["decoder_input_ids"].shape[0] * nb}
    bf16, _ = model_generate(model, tok, mk, dict(gk, self_kv_fp8=False, beam_use_kernel=True))
    assert bf16.shape[0] == got[True].shape[0]                             # (the bf16 indexed route still runs beside it)
    for bad in (dict(gk, beam_cache="copy", beam_prefill=False), {k: v for k, v in gk.items() if k not in ("beam_cache", "beam_prefill")}):
        with pytest.raises(ValueError, match="not built for beam search"):
            model_generate(model, tok, mk, bad)


def test_scheduler_rows_equal_the_windows_decoded_alone(monkeypatch):
    """Batch invariance through the table and the scales: three windows that share one wave of SequentialWindowScheduler (6 rows in
    one call, num_beams = 2, prefill) return exactly what generate_beam returns for each window alone (2 rows)."""
    from mapperatorinator_amd import _lib
    from mapperatorinator_amd.scheduler import SequentialWindowScheduler, SongJob
    from mapperatorinator_amd.server import build_sampling
    from mh_testing import synthetic_audio_varied
    g, tok, model, _, tgt = golden_bf16()
    eng, n = model.engine, 3
    song = synthetic_audio_varied(n, int(g["ns"]), seed=8)
    gk = gen_kwargs(tgt, num_beams=2, beam_cache="indexed", beam_prefill=True, self_kv_fp8=True)
    prompts = [torch.tensor([[tok.sos_id, 5 + 3 * w, 9 + w]]) for w in range(n)]       # equal lengths: no padding in the shared call

    def cut(row, P, eos):
        hit = torch.isin(row[P:], torch.tensor(sorted(eos))).nonzero()
        return row[:P + int(hit[0]) + 1] if hit.numel() else row
    calls = count_calls(monkeypatch, _lib.load())
    want = []
    for w in range(n):
        sp, eos = build_sampling(tok, dict(gk, conditional_temperature_per_row=True), tgt)
        out = eng.generate_beam(song[w:w + 1], prompts[w], None, eos, sp, 2, beam_cache="indexed", beam_prefill=True, beam_self_kv_fp8=True)
        want.append(cut(out["tokens"][0], 3, eos))
    assert set(calls["rows"]) == {2} and calls["mh_t5_self_kv_fp8_fill"] == n
    calls["rows"].clear()
    got = [None] * n
    jobs = [SongJob(frames=song[w:w + 1], prompt_fn=lambda _, w=w: dict(decoder_input_ids=prompts[w]),
                    on_result=lambda _, row, st, w=w: got.__setitem__(w, row), generate_kwargs=gk) for w in range(n)]
    stats = SequentialWindowScheduler(model, tok, encode_batch=4, decode_batch=8).run(jobs)
    assert stats["windows"] == n and set(calls["rows"]) == {6}             # the three windows shared every step
    assert calls["mh_t5_step_indexed"] == calls["mh_t5_step"] == 0
    for w in range(n):
        assert got[w].shape == want[w].shape and torch.equal(got[w], want[w]), (w, got[w].tolist(), want[w].tolist())
    assert len(want[0]) > 4 and len({tuple(x.tolist()) for x in want}) == n     # three different windows, each with tokens of its own
