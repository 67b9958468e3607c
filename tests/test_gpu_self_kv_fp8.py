"""-m gpu: the e4m3 self-attention K/V cache for the token steps (`self_kv_fp8`, mh_t5_generate_skv8; contract in include/mapperhip.h).

Not a parity mode.  The device must compute what the bf16-contract oracle computes when ITS self-attention cache goes through the same
row quantisation at the same moments (mh_testing.kv_fp8.with_self_kv_fp8: a hook on `decoder_step`), the shadow cache must be the
quantised bf16 cache bit for bit, rows must stay batch- and chain-invariant bit for bit, and the default path must be left alone.

Inputs: mh_testing.kv_fp8.CASES (`test` / `tiny` dims, 514 frames, tgt 264, 3 rows: the key loop takes 128 keys per pass and 2 per lane
group, so positions 127 / 128 / 129 and 255 / 256 / 257 are the tails and 263 the last); tests/test_self_kv_fp8_cpu.py asserts on the
same table that at most 10 % of the oracle's steps sit inside the 0.25 gap the gate below leaves out.

The logit gate: worst |dlogit| against the hooked oracle < FLOOR + 0.2, FLOOR = the worst |dlogit| of the plain bf16 device run against
the plain oracle on the same ids, measured in the same test.  0.2 is twice E4M3_TIE_MARGIN of tests/test_gpu_cross_kv_fp8.py; the
largest excess the project has recorded for an e4m3 K/V mode is +0.194 (hfw-small there), and an appended row can land one e4m3 step
from the oracle's for the same reason (the device's and the oracle's bf16 rows differ by bf16 roundings; an element whose two values
straddle an e4m3 boundary lands a whole e4m3 step apart).  The bound is not fitted to the figures below."""
import ctypes as C

import pytest
import torch

from mh_testing import kv_fp8

pytestmark = pytest.mark.gpu
GAP = kv_fp8.GAP
EXCESS = 0.2


def gen_kwargs(tgt, **over):
    kw = dict(precision="fp32", do_sample=False, num_beams=1, top_p=1.0, top_k=0, max_length=tgt, cfg_scale=1.0, timeshift_bias=0,
              types_first=False, temperature=1.0, lookback_time=0, lookahead_time=0, context_type="map", pad_token_id=0)
    kw.update(over)
    return kw


def build_model(name, options=None):
    from mapperatorinator_amd.modeling import MapperatorinatorHIP
    ci = kv_fp8.case_inputs(name)
    tok = ci["tok"]
    return MapperatorinatorHIP(ci["sd"], ci["dims"], vocab_size_in=tok.vocab_size_in, vocab_size_out=tok.vocab_size_out,
                               tgt_seq_len=ci["spec"]["tgt"], dtype=torch.bfloat16, device="cuda", options=options, **ci["model_kwargs"])


_MODELS = {}


def model_for(name, prefill=1):
    """one bf16 model per case (cases that share weights and shape share it); prefill = 0: option decode_prefill = 0 through the
    engine's own option set"""
    c = kv_fp8.CASES[name]
    key = (c["family"], c["size"], c["frames"], c["tgt"], c["seed"], c.get("local_attention"), prefill)
    if key not in _MODELS:
        _MODELS[key] = build_model(name, None if prefill else {"decode_prefill": 0})
    return _MODELS[key]


def device_run(model, r, self8, cross8=False):
    from mapperatorinator_amd.server import build_sampling
    tok, tgt = r["tok"], r["spec"]["tgt"]
    sp, _ = build_sampling(tok, gen_kwargs(tgt), tgt)
    out = model.engine.generate(r["audio"], r["prompt"], r["mask"], [tok.eos_id], sp, forced=r["forced"], dump_logits=True,
                                self_kv_fp8=self8, cross_kv_fp8=cross8)
    return out["tokens"], out["logits"].cpu()


def gate(name, prefill=1):
    """Gate 2 of the module docstring for case `name`; returns (floor, excess, near-tie flips)."""
    r = kv_fp8.oracle_runs(name)
    c = r["spec"]
    model = model_for(name, prefill)
    P, tgt, B = r["prompt"].shape[1], c["tgt"], c["rows"]
    _, lg8 = device_run(model, r, True, bool(c.get("cross")))
    _, lg16 = device_run(model, r, False)
    want = torch.stack(r["scores"])                                      # (tgt - P, B, V): the scores that produce columns P ..
    plain = torch.stack(r["scores_plain"])
    assert want.shape[0] == tgt - P and lg8.shape[0] == tgt
    lg8, lg16 = lg8[P:], lg16[P:]
    fin = torch.isfinite(want)
    assert torch.equal(fin, torch.isfinite(lg8)), "finite patterns differ"
    assert torch.equal(torch.isfinite(plain), torch.isfinite(lg16))
    worst8 = (lg8[fin] - want[fin]).abs().max().item()
    floor = (lg16[torch.isfinite(plain)] - plain[torch.isfinite(plain)]).abs().max().item()
    top2 = want.topk(2, dim=-1).values
    gap = top2[..., 0] - top2[..., 1]                                    # (tgt - P, B)
    miss = lg8.argmax(-1) != want.argmax(-1)
    n_bad, n_tie = int((miss & (gap > GAP)).sum()), int((miss & (gap <= GAP)).sum())
    moved = (lg8[fin] - lg16[fin]).abs().max().item()
    print(f"{name}{'' if prefill else ' (decode_prefill = 0)'}: {gap.numel()} steps ({int((gap <= GAP).sum())} inside the {GAP} gap), {n_tie} near-tie "
          f"flips, {n_bad} real mismatches; worst |dlogit| {worst8:.3f} vs the hooked oracle, floor (plain bf16 run vs the plain oracle on "
          f"the same ids) {floor:.3f}, excess {worst8 - floor:+.3f} (allowed {EXCESS}); the mode moves the logits by up to {moved:.3f}")
    assert moved > 0, "the mode is not on: the logits equal the mode-off run's"
    assert n_bad == 0
    assert worst8 < floor + EXCESS
    return floor, worst8 - floor, n_tie


# measured (MI355X): floor (plain bf16 run vs the plain oracle) / worst |dlogit| vs the hooked oracle (excess; allowed +0.2), near-tie
# flips of the steps, real mismatches 0 everywhere:
#   t5          0.339 / 0.440 (+0.101), 3 of 789     var-small    0.059 / 0.090 (+0.031), 0 of 62
#   var         0.081 / 0.083 (+0.002), 0 of 789     rope-small   0.066 / 0.094 (+0.028), 0 of 62
#   rope        0.089 / 0.108 (+0.019), 0 of 789     hf-small     0.194 / 0.315 (+0.121), 0 of 62
#   hf          0.272 / 0.252 (-0.020), 0 of 789
#   var-prompt9 0.074 / 0.102 (+0.028), 0 of 765     var-prompt1 (decode_prefill = 0) 0.076 / 0.098 (+0.022), 0 of 765
#   var-local   0.085 / 0.125 (+0.040), 0 of 789     var-both (with cross_kv_fp8)     0.081 / 0.140 (+0.059), 0 of 789
# The LayerNorm family and T5 tiny are the most sensitive (the mode itself moves their logits by up to 1.3 / 2.4); every case is well
# inside the bound, which stays floor + 0.2 and is not fitted to these figures.
@pytest.mark.parametrize("name", ["t5", "var", "rope", "hf", "var-small", "rope-small", "hf-small"])
def test_parity_with_the_hooked_oracle(name):
    """1-token prompt (every position is a token step and appends its row), teacher-forced on the hooked oracle's own free run; per
    family at `test` / `tiny` dims and tgt 264, and at `small` dims (d 768: the KC = 6 instantiation of the releases), 2 rows, tgt 32."""
    gate(name)


@pytest.mark.parametrize("prefill", [1, 0])
def test_prompted_rows(prefill, family="var"):
    """Prompts of 1, 4 and 9 tokens, left-padded with a mask.  Batched prefill: positions 0 .. 7 attend each other through the bf16
    cache and are quantised in one pass (the hook with P = 9).  decode_prefill = 0 (through the engine's option set): every prompt
    position is a token step that attends e4m3 rows and appends its own (the hook with P = 1)."""
    gate(f"{family}-prompt{9 if prefill else 1}", prefill)


def test_local_layers_skip_whole_key_passes():
    """varwhisper with global_attn_every_n_layers = 2 and local_attention = 2 (a window of one key back, the smallest there is): from
    position 129 on the local layers skip whole 128-key passes (j_first) and mask the rest of the pass below the window."""
    gate("var-local")


def test_composition_with_cross_kv_fp8():
    """self_kv_fp8 + cross_kv_fp8 against the oracle that has both hooks (its cross K / V quantised per slab as the device's copy)."""
    gate("var-both")


def _caches(eng, B, n):
    k, v, q8, sc = eng.self_kv_caches(B, shadow=True)
    torch.cuda.synchronize()
    return k[..., :n, :], v[..., :n, :], q8[..., :n, :].cpu(), sc[..., :n].cpu()


@pytest.mark.parametrize("name,plen", [("t5", 1), ("var", 1), ("rope", 1), ("hf", 1), ("var", 5), ("t5", 5)])
def test_shadow_cache_is_the_quantised_bf16_cache_bit_for_bit(name, plen):
    """After a mode-on decode the e4m3 bytes and scales of every position < n equal mh_quantize_kv_rows of the bf16 cache of the same
    run (read through mh_t5_decode_self_cache) and the mh_testing restatement of it.  No tolerance.  plen = 1: every row was appended
    by a token step; plen = 5 (left-padded rows of 5, 3 and 1 tokens): rows 0 .. 3 come from the bulk pass after the prefill."""
    from mapperatorinator_amd.server import build_sampling
    ci = kv_fp8.case_inputs(name)
    tok, tgt, B = ci["tok"], ci["spec"]["tgt"], ci["spec"]["rows"]
    model = model_for(name)
    eng = model.engine
    g = torch.Generator().manual_seed(5)
    forced = torch.randint(3, tok.vocab_size_out, (B, tgt), generator=g)
    lens = (5, 3, 1) if plen > 1 else (1,) * B
    mask = torch.arange(plen)[None, :] >= torch.tensor([plen - n for n in lens])[:, None]
    forced[:, :plen] = torch.where(mask, forced[:, :plen], torch.zeros_like(forced[:, :plen]))
    forced[torch.arange(B), torch.tensor([plen - n for n in lens])] = tok.sos_id
    sp, _ = build_sampling(tok, gen_kwargs(tgt), tgt)
    eng.generate(ci["audio"], forced[:, :plen].clone(), mask if plen > 1 else None, [], sp, forced=forced, self_kv_fp8=True)
    n = tgt - 1                                                          # positions 0 .. tgt - 2 were fed
    k, v, q8, sc = _caches(eng, B, n)
    eng._enter()
    with eng.on_stream():
        qk, sk = eng.quantize_kv_rows(k)
        qv, sv = eng.quantize_kv_rows(v)
    eng._leave()
    eng.synchronize()
    assert k.float().abs().max() > 0 and torch.isfinite(k.float()).all() and torch.isfinite(v.float()).all()
    for kv, (q_dev, s_dev, x) in enumerate(((qk, sk, k), (qv, sv, v))):
        assert torch.equal(q8[:, kv], q_dev.cpu()) and torch.equal(sc[:, kv], s_dev.cpu()), ("k", "v")[kv]
        q_ref, s_ref = kv_fp8.quantize_rows(x.cpu())
        assert torch.equal(sc[:, kv], s_ref), ("k", "v")[kv]
        assert torch.equal(q8[:, kv], q_ref), (("k", "v")[kv], int((q8[:, kv] != q_ref).sum()))


def _forced_ids(tok, B, tgt, seed):
    from conftest import ts_range
    ts0, ts1 = ts_range(tok)
    g = torch.Generator().manual_seed(seed)
    forced = torch.randint(ts1, tok.vocab_size_out, (B, tgt), generator=g)
    forced[:, 1::3] = torch.randint(ts0, ts1, forced[:, 1::3].shape, generator=g)     # time shifts too: the monotonic mask moves
    forced[:, 0] = tok.sos_id
    return forced


def _device_kv(eng, audio):
    eng._enter()
    with eng.on_stream():
        kv = eng.cross_kv(eng.encode_mel(eng.mel(audio.to(eng.device, torch.float32))))
    eng._leave()
    eng.synchronize()
    return kv


def test_rows_do_not_depend_on_their_batch_or_chain():
    """18 rows: two chains of 9 (mh_t5_decode_chains_cfg), the second chain's kernels reach the caches, the shadow and its scales
    through b0 offsets.  Logits and tokens of every row must equal, bit for bit, that row decoded alone (one chain, no offsets)."""
    from mapperatorinator_amd.server import build_sampling
    from mh_testing import synthetic_audio_varied
    ci = kv_fp8.case_inputs("var")
    tok, tgt, frames = ci["tok"], ci["spec"]["tgt"], ci["spec"]["frames"]
    eng = model_for("var").engine
    B = 18
    assert eng.lib.mh_t5_decode_chains_cfg(C.byref(eng.packed.cfg), B) == 2 and eng.lib.mh_t5_decode_chains_cfg(C.byref(eng.packed.cfg), 1) == 1
    kv = _device_kv(eng, synthetic_audio_varied(B, (frames - 1) * 128, seed=6))
    forced = _forced_ids(tok, B, tgt, 9).to(eng.device, torch.int32).contiguous()
    eos_table = torch.zeros(tok.vocab_size_out, dtype=torch.uint8, device=eng.device)

    def run(rows):
        sp, _ = build_sampling(tok, gen_kwargs(tgt), tgt)
        eng._enter()
        with eng.on_stream():
            t, _, lg = eng.decode(kv[:, :, rows].contiguous(), forced[rows, :1].contiguous(), None, eos_table, sp, forced[rows].contiguous(),
                                  True, self_kv_fp8=True)
        eng._leave()
        eng.synchronize()
        return t.cpu(), lg[1:].cpu()
    t_all, lg_all = run(slice(0, B))
    assert torch.isfinite(lg_all).any() and not torch.equal(lg_all[:, 0], lg_all[:, B // 2])
    for b in range(B):
        t1, lg1 = run(slice(b, b + 1))
        assert torch.equal(t1[0], t_all[b]) and torch.equal(lg1[:, 0], lg_all[:, b]), f"row {b} depends on its batch"


def test_guidance_pairs_equal_the_two_halves_decoded_as_plain_rows():
    """cfg_scale = 2 with a negative prompt: the doubled rows own their cache rows (bf16 and shadow).  The guided scores must equal, bit
    for bit, uncond + (cond - uncond) * 2 formed in torch from the raw logits of the same [negative | prompt] rows decoded as plain
    rows over the repeated cross K/V."""
    from conftest import ts_range
    from mapperatorinator_amd.server import build_sampling
    ci = kv_fp8.case_inputs("rope")
    tok, tgt, B = ci["tok"], ci["spec"]["tgt"], ci["spec"]["rows"]
    eng = model_for("rope").engine
    ts0, ts1 = ts_range(tok)
    neg_id = ts1 + 3                                        # not a TIME_SHIFT id: both halves keep the same monotonic mask
    forced = _forced_ids(tok, B, tgt, 9)
    prompt2 = torch.cat([torch.full((B, 1), neg_id), forced[:, :1]], 0).to(eng.device, torch.int32).contiguous()
    forced2 = torch.cat([forced, forced], 0).to(eng.device, torch.int32).contiguous()
    eos_table = torch.zeros(tok.vocab_size_out, dtype=torch.uint8, device=eng.device)
    kv = _device_kv(eng, ci["audio"])
    eng._enter()
    with eng.on_stream():
        kv2 = torch.cat([kv, kv], 2).contiguous()
        sp, _ = build_sampling(tok, gen_kwargs(tgt, cfg_scale=2.0), tgt)
        _, _, guided = eng.decode(kv, prompt2, None, eos_table, sp, forced2, True, self_kv_fp8=True)
        sp, _ = build_sampling(tok, gen_kwargs(tgt), tgt)
        _, _, plain = eng.decode(kv2, prompt2, None, eos_table, sp, forced2, True, self_kv_fp8=True)
        sp, _ = build_sampling(tok, gen_kwargs(tgt, cfg_scale=2.0), tgt)
        _, _, guided16 = eng.decode(kv, prompt2, None, eos_table, sp, forced2, True)
    eng._leave()
    eng.synchronize()
    guided, plain, guided16 = guided[1:].cpu(), plain[1:].cpu(), guided16[1:].cpu()
    assert guided.shape == (tgt - 1, B, tok.vocab_size_out) and plain.shape == (tgt - 1, 2 * B, tok.vocab_size_out)
    uncond, cond = plain[:, B:], plain[:, :B]               # HF's processor on the reference's row order: first half = "cond"
    fin = torch.isfinite(guided)
    assert torch.equal(fin, torch.isfinite(uncond)) and torch.equal(fin, torch.isfinite(cond)) and fin.any() and not fin.all()
    want = uncond + (cond - uncond) * 2.0
    assert torch.equal(guided[fin], want[fin]), (guided[fin] - want[fin]).abs().max()
    assert not torch.equal(guided[fin], guided16[fin])      # ... and the shadow was what the guided run read


def test_step_graph_cache_tells_the_modes_apart():
    """One engine: mode on, mode off, mode on, then mode on together with cross_kv_fp8, over the same workspace.  Runs 1 and 3 must be
    bit-equal (a mode-on call after a mode-off call must not replay the other's graph), run 2 bit-equal to a FRESH engine's mode-off
    run (the mode leaves the default path alone), run 4 differs from run 1."""
    r = kv_fp8.oracle_runs("var", plain=False)
    one = build_model("var")
    runs = [device_run(one, r, True), device_run(one, r, False), device_run(one, r, True), device_run(one, r, True, True)]
    fresh = device_run(build_model("var"), r, False)
    fin = torch.isfinite(runs[0][1])
    assert torch.equal(runs[0][0], runs[2][0]) and torch.equal(runs[0][1][fin], runs[2][1][fin])
    assert torch.equal(runs[1][0], fresh[0]) and torch.equal(runs[1][1][fin], fresh[1][fin])
    assert torch.equal(fin, torch.isfinite(runs[1][1])) and torch.equal(fin, torch.isfinite(runs[3][1]))
    assert not torch.equal(runs[0][1][fin], runs[1][1][fin]) and not torch.equal(runs[0][1][fin], runs[3][1][fin])


def test_public_seams():
    """model_generate(generate_kwargs = {"self_kv_fp8": True}) returns the engine call's ids; one two-window song through the
    scheduler returns each window as the engine returns it alone; num_beams = 2 raises."""
    from mapperatorinator_amd.scheduler import SequentialWindowScheduler, SongJob
    from mapperatorinator_amd.server import build_sampling, model_generate
    from mh_testing import synthetic_audio_varied
    ci = kv_fp8.case_inputs("var")
    tok, frames = ci["tok"], ci["spec"]["frames"]
    model = model_for("var")
    eng, tgt, n, tgt_model = model.engine, 40, 2, model.config.max_target_positions
    song = synthetic_audio_varied(n, (frames - 1) * 128, seed=8)
    gk = gen_kwargs(tgt, self_kv_fp8=True)
    prompt = torch.tensor([[1, 40], [0, 1]])
    mk = dict(inputs=song, decoder_input_ids=prompt, decoder_attention_mask=prompt.ne(0))
    ids, _ = model_generate(model, tok, mk, gk)
    sp, eos = build_sampling(tok, gk, tgt_model)
    want = eng.generate(song, prompt, prompt.ne(0), eos, sp, self_kv_fp8=True)["tokens"]
    assert torch.equal(ids, want) and ids.shape[1] > prompt.shape[1]
    with pytest.raises(ValueError, match="not built for beam search"):
        model_generate(model, tok, mk, dict(gk, num_beams=2))

    def prompt_from(prev):
        carry = [] if prev is None else [t for t in prev.tolist() if t > 2][-3:]
        return torch.tensor([[tok.sos_id] + carry])

    def cut(row, P, eos):
        hit = torch.isin(row[P:], torch.tensor(sorted(eos))).nonzero()
        return row[:P + int(hit[0]) + 1] if hit.numel() else row
    want, prev = [], None
    for w in range(n):
        p = prompt_from(prev)
        sp, eos = build_sampling(tok, dict(gk, conditional_temperature_per_row=True), tgt_model)
        row = cut(eng.generate(song[w:w + 1], p, None, eos, sp, self_kv_fp8=True)["tokens"][0], p.shape[1], eos)
        prev = row[p.shape[1]:]
        want.append(row)
    got, state = [None] * n, [None]

    def on_result(w, row, st):
        got[w] = row
        state[0] = row[prompt_from(state[0]).shape[1]:]
    job = SongJob(frames=song, prompt_fn=lambda w: dict(decoder_input_ids=prompt_from(state[0])), on_result=on_result, generate_kwargs=gk)
    stats = SequentialWindowScheduler(model, tok, encode_batch=4, decode_batch=8).run([job])
    assert stats["windows"] == n
    for w in range(n):
        assert got[w].shape == want[w].shape and torch.equal(got[w], want[w]), (w, got[w].tolist(), want[w].tolist())
    assert len(want[0]) > 2
