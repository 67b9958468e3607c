"""-m gpu: osuT5 hot path (mel -> encoder -> AR decode) through the C ABI vs the CPU oracle and vs the
golden vectors produced by the imported reference (tests/golden, oracle/make_golden.py).

Contract checked here:
  fp32 storage : greedy token ids BIT-EXACT vs the reference's own `model_generate` output (golden) and vs
                 the oracle on fresh seeds; encoder hidden states within 2e-4 abs (fp32 rounding only).
  bf16 storage : teacher-forced agreement with the bf16-contract oracle: every step whose oracle top-2 gap
                 exceeds GAP_BF16 must pick the same id; logits within 0.15 abs.
"""
import numpy as np
import pytest
import torch

from conftest import (GOLDEN, assert_scores_close, assert_topk_scores_match, oracle_processor_kwargs, t5_golden_case,
                      ts_range, types_first_case)

pytestmark = pytest.mark.gpu

GAP_BF16 = 0.25


def build(size, tok, sd, src, tgt, dtype):
    from mapperatorinator_amd.modeling import MapperatorinatorHIP
    from mapperatorinator_amd.t5_engine import T5_PRESETS
    return MapperatorinatorHIP(sd, T5_PRESETS[size], vocab_size_in=tok.vocab_size_in, vocab_size_out=tok.vocab_size_out,
                               src_seq_len=src, tgt_seq_len=tgt, dtype=dtype, device="cuda")


def oracle_for(size, sd, rounding=None):
    from mapperatorinator_amd.t5_engine import T5_PRESETS
    from oracle import t5 as ot5
    d = T5_PRESETS[size]
    return ot5.T5Oracle(sd, d.d_model, d.d_ff, d.n_heads, d.n_enc_layers, d.n_dec_layers, rounding=rounding)


def golden_case(name):
    return t5_golden_case(name)


def gen_kwargs(tgt, **over):
    kw = dict(precision="fp32", do_sample=False, num_beams=1, top_p=1.0, top_k=0, max_length=tgt, cfg_scale=1.0,
              timeshift_bias=0, types_first=False, temperature=1.0, lookback_time=0, lookahead_time=0,
              context_type="map", pad_token_id=0)
    kw.update(over)
    return kw


@pytest.mark.parametrize("name", ["t5_tiny", "t5_small", "t5_base", "t5_base_wide", "t5_large"])
def test_fp32_matches_reference_golden(name):
    """t5_base = BASELINE configs[1] dims at their own size (osuT5-base, 1251 frames, ragged prompts, 133 new
    tokens per row): ids bit-exact and the 16 best processed scores of every step within 5e-4 of the reference's.
    t5_base_wide (round 6) = the same dims with 16 ragged rows x 197 new tokens: one full 16-row decode chain of the headline shape.
    t5_large = configs[4]'s backbone (google/t5-v1_1-large dims through the same wrapper: d 1024, 16 heads, 24 + 24
    layers) at 1251 frames, 2 ragged rows, 69 new tokens."""
    from mapperatorinator_amd.server import build_sampling, model_generate
    g, size, tok, sd, audio, src, tgt = golden_case(name)
    model = build(size, tok, sd, src, tgt, torch.float32)
    # encoder hidden states vs the reference's (slice stored in the golden file)
    enc, enc32 = model.engine.encode(audio.cuda(), want_f32=True)
    got = enc32.cpu()[:, ::53, ::17]
    err = np.abs(got.numpy() - g["enc_slice"]).max()
    print(name, "encoder max abs err vs reference", err)
    assert err < 2e-4
    prompt = torch.from_numpy(g["prompt"])
    mk = dict(inputs=audio, decoder_input_ids=prompt, decoder_attention_mask=prompt.ne(0))
    ids, stats = model_generate(model, tok, mk, gen_kwargs(tgt))
    assert ids.dtype == torch.int64 and ids.device.type == "cpu"
    assert ids.shape == g["ids"].shape, (ids.shape, g["ids"].shape)
    assert np.array_equal(ids.numpy(), g["ids"]), f"first mismatch at {np.argwhere(ids.numpy() != g['ids'])[:3]}"
    assert stats["generated_tokens"] == int((g["ids"] != 0).sum() - (g["prompt"] != 0).sum())
    # processors on: temperature, timeshift bias, lookahead EOS window
    ids2, _ = model_generate(model, tok, mk, gen_kwargs(tgt, temperature=0.7, timeshift_bias=0.35, lookahead_time=3000))
    assert ids2.shape == g["ids_processors"].shape and np.array_equal(ids2.numpy(), g["ids_processors"])
    if "top_vals" in g.files:
        sp, eos = build_sampling(tok, gen_kwargs(tgt), tgt)
        out = model.engine.generate(audio, prompt, prompt.ne(0), eos, sp, dump_logits=True)
        assert torch.equal(out["tokens"], ids)
        worst = assert_topk_scores_match(out["logits"], g, prompt.shape[1], 5e-4)
        print(name, "worst |d score| vs the reference over the 16 best ids of every step", worst)


# (a case keeps the id of its place in the original ten-case list when cases before it are removed; a changed case gets a
# new, descriptive id)
@pytest.mark.parametrize("opts", [pytest.param(dict(decode_gemv_cols=16), id="opts1"),
                                  pytest.param(dict(decode_gemv_cols=8), id="opts2"),
                                  pytest.param(dict(decode_gemv_cols=4), id="opts3"),
                                  pytest.param(dict(decode_chains=1), id="opts4"),
                                  pytest.param(dict(decode_chains=3), id="opts5"),
                                  pytest.param(dict(decode_prefill=0), id="prefill0"),
                                  pytest.param(dict(decode_chains=3, decode_gemv_cols=4), id="opts9")])
def test_decode_kernel_variants_reproduce_the_reference_tokens(opts):
    """Every run-time selectable form of the decode step (mh_set_option: 16 / 8 / 4 real columns per GEMV tile, 1 or 3
    row chains, token-by-token prompt feeding) must give the reference's greedy ids bit for bit in fp32 (golden t5_tiny: ragged prompts, 3 rows;
    t5_small: base-like head count)."""
    from mapperatorinator_amd import _lib
    from mapperatorinator_amd.server import model_generate
    old = {k: _lib.set_option(k, v) for k, v in opts.items()}
    try:
        for name in ("t5_tiny", "t5_small"):
            g, size, tok, sd, audio, src, tgt = golden_case(name)
            model = build(size, tok, sd, src, tgt, torch.float32)
            prompt = torch.from_numpy(g["prompt"])
            ids, _ = model_generate(model, tok, dict(inputs=audio, decoder_input_ids=prompt, decoder_attention_mask=prompt.ne(0)),
                                    gen_kwargs(tgt))
            assert np.array_equal(ids.numpy(), g["ids"]), (name, opts, np.argwhere(ids.numpy() != g["ids"])[:3])
    finally:
        for k, v in old.items():
            _lib.set_option(k, v)


@pytest.mark.parametrize("name", ["t5_base", "t5_base_wide"])
def test_bf16_teacher_forced_on_the_reference_bf16_run(name):
    """tests/golden/<name>_bf16ref.npz (t5_base: 4 rows x 133 tokens; t5_base_wide, round 6: 16 rows x 197 tokens -- a full decode
    chain of the headline shape) = the REFERENCE itself in torch.bfloat16 (model.to(bfloat16), the precision
    switch of osuT5/osuT5/utils/model_utils.py:375-376) on the t5_base case.  The HIP bf16 path, teacher-forced on the
    reference's ids, must take the reference's decision on >= 99 % of the steps the reference decided by more than 0.5 (its own
    bf16 logits are spaced 0.06-0.125), and on >= 90 % of all live steps; the recorded rates of the CPU oracles are
    printed next to ours."""
    from mapperatorinator_amd.server import build_sampling
    g, size, tok, sd, audio, src, tgt = golden_case(name)
    r = np.load(f"{GOLDEN}/{name}_bf16ref.npz")
    ids16 = torch.from_numpy(r["ids"])
    n_cols = ids16.shape[1]
    model = build(size, tok, sd, src, tgt, torch.bfloat16)
    prompt = torch.from_numpy(g["prompt"])
    P = prompt.shape[1]
    forced = torch.zeros((ids16.shape[0], tgt), dtype=torch.long)
    forced[:, :n_cols] = ids16
    sp, _ = build_sampling(tok, gen_kwargs(tgt), tgt)
    out = model.engine.generate(audio, prompt, prompt.ne(0), [], sp, forced=forced, dump_logits=True)
    lg = out["logits"].float().cpu()                         # (cols, B, V) processed scores
    pick = lg[P:n_cols].argmax(-1).T                         # (B, steps)
    want = ids16[:, P:]
    gap = torch.from_numpy(r["top_vals"][..., 0] - r["top_vals"][..., 1]).T
    live = want.ne(0)
    dec = live & (gap >= float(r["decisive_gap"]))
    ok = pick == want
    rate_all, rate_dec = ok[live].float().mean().item(), ok[dec].float().mean().item()
    # logit error against the reference's own (bf16-rounded) best scores
    tv, ti = torch.from_numpy(r["top_vals"]), torch.from_numpy(r["top_ids"]).long()
    err = (lg[P:n_cols].gather(-1, ti) - tv).abs()[live.T]
    print(f"HIP bf16 vs the bf16 reference, teacher-forced: top-1 agreement {rate_all:.3f} of {int(live.sum())} live steps, "
          f"{rate_dec:.3f} of {int(dec.sum())} decisive ones (CPU oracles: fp32 {r['agree_fp32_oracle'][:2]}, bf16 contract "
          f"{r['agree_bf16_contract_oracle'][:2]}); |d score| on the reference's 16 best: mean {err.mean():.3f} max {err.max():.3f}")
    assert rate_dec >= 0.99          # (1 of 376 flips with some summation orders: its HIP top-2 gap is below bf16 resolution)
    assert rate_all >= 0.90


def test_bf16_large_teacher_forced_on_the_reference_fp32_run():
    """osuT5-large in the bf16 storage mode (the mode tools/long_song_bench.py and bench.py's config-5 line quote numbers
    for), at the golden's own size (1251 frames), teacher-forced on the ids the fp32 REFERENCE produced
    (tests/golden/t5_large.npz): the reference's decision on >= 99 % of the steps it decided by more than 0.5 and on
    >= 90 % of all live steps; scores of its 16 best ids within the bf16 noise floor."""
    from mapperatorinator_amd.server import build_sampling
    g, size, tok, sd, audio, src, tgt = golden_case("t5_large")
    ids = torch.from_numpy(g["ids"])
    n_cols = ids.shape[1]
    model = build(size, tok, sd, src, tgt, torch.bfloat16)
    prompt = torch.from_numpy(g["prompt"])
    P = prompt.shape[1]
    forced = torch.zeros((ids.shape[0], tgt), dtype=torch.long)
    forced[:, :n_cols] = ids
    sp, _ = build_sampling(tok, gen_kwargs(tgt), tgt)
    out = model.engine.generate(audio, prompt, prompt.ne(0), [], sp, forced=forced, dump_logits=True)
    lg = out["logits"].float().cpu()
    pick = lg[P:n_cols].argmax(-1).T
    want = ids[:, P:]
    gap = torch.from_numpy(g["top_vals"][..., 0] - g["top_vals"][..., 1]).T
    live = want.ne(0)
    dec = live & (gap >= 0.5)
    ok = pick == want
    rate_all, rate_dec = ok[live].float().mean().item(), ok[dec].float().mean().item()
    tv, ti = torch.from_numpy(g["top_vals"]), torch.from_numpy(g["top_ids"]).long()
    err = (lg[P:n_cols].gather(-1, ti) - tv).abs()[live.T]
    print(f"HIP bf16 osuT5-large vs the fp32 reference, teacher-forced: top-1 agreement {rate_all:.3f} of {int(live.sum())} live "
          f"steps, {rate_dec:.3f} of {int(dec.sum())} decisive ones; |d score| on the reference's 16 best: mean {err.mean():.3f} "
          f"max {err.max():.3f}")
    assert rate_dec >= 0.99 and rate_all >= 0.90
    assert err.mean().item() < 0.15


def test_fp8_cross_kv_teacher_forced_vs_oracle_with_quantised_kv():
    """The e4m3 copy of the cross-attention K / V (mh_t5_quantize_cross_kv, MhSampling.cross_kv_fp8; BASELINE
    configs[4]) against the bf16-contract oracle whose cross K / V went through the same quantisation (absmax / 448 per
    (layer, k|v, row, head), torch.float8_e4m3fn): teacher-forced on the t5_base golden ids with a 1-token prompt so that
    every position is a token step.  Gate: the bf16 noise floor of the headline test (mean < 0.06, worst < 0.5); the
    distance to the un-quantised bf16 run is printed (what the mode costs)."""
    from mapperatorinator_amd.server import build_sampling
    g, size, tok, sd, audio, src, tgt = golden_case("t5_base")
    B = audio.shape[0]
    ids = torch.from_numpy(g["ids"]).long()
    T = ids.shape[1]
    ids = ids.clone()
    ids[:, 0] = tok.sos_id                                   # a 1-token prompt: column 0 only
    prompt = ids[:, :1].clone()
    forced = torch.zeros((B, tgt), dtype=torch.long)
    forced[:, :T] = ids
    model = build(size, tok, sd, src, tgt, torch.bfloat16)
    sp, _ = build_sampling(tok, gen_kwargs(tgt), tgt)
    lg8 = model.engine.generate(audio, prompt, None, [], sp, forced=forced, dump_logits=True, cross_kv_fp8=True)["logits"].float().cpu()
    sp, _ = build_sampling(tok, gen_kwargs(tgt), tgt)
    lg16 = model.engine.generate(audio, prompt, None, [], sp, forced=forced, dump_logits=True)["logits"].float().cpu()
    o = oracle_for(size, sd, rounding="bf16")
    ckv = o.cross_kv(o.encode_audio(audio))

    def qdq(x):                                              # (B, H, L, 64): per (row, head) scale
        scale = x.abs().amax(dim=(2, 3), keepdim=True) / 448.0
        scale = torch.where(scale > 0, scale, torch.ones_like(scale))
        return (x / scale).to(torch.float8_e4m3fn).float() * scale
    ckv8 = [(qdq(k), qdq(v)) for k, v in ckv]
    ts0, ts1 = ts_range(tok)
    want = o.monotonic_scores(o.decoder_forward(ids[:, :-1], ckv8), ids[:, :-1], ts0, ts1, [tok.sos_id])   # (B, T-1, V)
    hip8, hip16 = lg8[1:T].transpose(0, 1), lg16[1:T].transpose(0, 1)
    fin = torch.isfinite(want)
    assert torch.equal(fin, torch.isfinite(hip8))
    d8 = (hip8[fin] - want[fin]).abs()
    dmode = (hip8[fin] - hip16[fin]).abs()
    agree = (hip8.argmax(-1) == hip16.argmax(-1)).float().mean().item()
    print(f"fp8 cross K/V vs the oracle with quantised K/V: |dlogit| mean {d8.mean():.4f} worst {d8.max():.3f}; vs the bf16 "
          f"K/V run of the same kernels: mean {dmode.mean():.4f} worst {dmode.max():.3f}, same top-1 on {agree:.3f} of the steps")
    # measured: mean 0.056, worst 0.43 (the bf16 noise floor of the headline test plus e4m3 rounding ties: the device
    # multiplies by 1 / scale where torch divides by the scale); the mode itself moves logits by 0.2 on average and keeps
    # the top-1 of 91 % of the steps
    assert d8.mean().item() < 0.08 and d8.max().item() < 0.6
    assert dmode.max().item() > 0          # the mode is really on
    assert agree > 0.85


def test_bf16_headline_batch_teacher_forced_vs_oracle():
    """BASELINE configs[1] at its own size: osuT5-base, bf16, B = 32 chunks x 384 new tokens.  The free-running HIP ids
    are fed back teacher-forced to the bf16-contract CPU oracle: every step the oracle decides by more than GAP_BF16
    must agree (the real gate), logits within 0.06 on average and 0.5 at worst."""
    from mapperatorinator_amd import Tokenizer
    from mapperatorinator_amd.server import build_sampling
    from mapperatorinator_amd.t5_engine import T5_PRESETS
    from mh_testing import DIVERSE_GAINS, random_t5_state_dict, synthetic_audio_varied
    src, tgt, B = 1251, 385, 32
    tok = Tokenizer.benchmark_vocab(src_seq_len=src)
    sd = random_t5_state_dict(T5_PRESETS["base"], tok.vocab_size_in, tok.vocab_size_out, seed=17, lm_head_gain=4.0,
                              gains=DIVERSE_GAINS)
    model = build("base", tok, sd, src, tgt, torch.bfloat16)
    audio = synthetic_audio_varied(B, 160000, seed=21)
    prompt = torch.tensor([[1]] * B)
    ts0, ts1 = ts_range(tok)
    sp, _ = build_sampling(tok, gen_kwargs(tgt), tgt)
    out = model.engine.generate(audio, prompt, None, [], sp, dump_logits=True)
    got, lg = out["tokens"], out["logits"].float().cpu()
    assert got.shape == (B, tgt)
    o = oracle_for("base", sd, rounding="bf16")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    # all 384 positions of the oracle in ONE teacher-forced pass (oracle.decoder_forward: the step-by-step form takes
    # ~1 s per step at this batch on a CPU), then the always-on MonotonicTimeShift processor
    lgo = o.decoder_forward(got[:, :-1], o.cross_kv(o.encode_audio(audio)))
    scores = o.monotonic_scores(lgo, got[:, :-1], ts0, ts1, [tok.sos_id])          # (B, T-1, V); row t -> column t+1
    top2 = scores.topk(2, dim=-1).values
    gap = top2[..., 0] - top2[..., 1]
    want = scores.argmax(-1)
    hip = lg[1:tgt].transpose(0, 1)                                                  # (B, T-1, V)
    fin = torch.isfinite(scores)
    assert torch.equal(fin, torch.isfinite(hip))
    dl = (hip[fin] - scores[fin]).abs()
    worst, mean = dl.max().item(), dl.mean().item()
    diff = got[:, 1:] != want
    n_cmp = diff.numel()
    n_bad, n_tie = int((diff & (gap > GAP_BF16)).sum()), int((diff & (gap <= GAP_BF16)).sum())
    print(f"base bf16 B=32 x 384 teacher-forced vs the bf16 oracle: {n_cmp} steps, {n_tie} near-tie flips, {n_bad} real "
          f"mismatches, |dlogit| mean {mean:.4f} worst {worst:.3f}; distinct ids {len(set(got.flatten().tolist()))}")
    # a flip needs the two competing logits to err by their gap together: with |dlogit| up to `worst` per logit no flip
    # can sit above 2 * worst, and flips above GAP_BF16 (about the worst single error) must stay isolated events
    # (measured: 0 or 1 of 12 288 steps, depending on the fp32 summation order of the kernel variant)
    assert n_bad <= 3 and float(gap[diff].max() if diff.any() else 0.0) <= 2 * worst + 1e-3
    # 22.7 M logits: the worst one sits at 0.33 (measured) -- two CPU evaluations of the same bf16 contract (stepwise vs
    # batched oracle) already differ by 0.035 at tiny dims; the mean is the stable figure
    assert worst < 0.5 and mean < 0.06      # measured: mean 0.037, worst 0.35 (bf16 operands: 3 significant digits)
    assert n_tie <= 0.05 * n_cmp


@pytest.mark.parametrize("run", ["tf", "cfg", "all"])
def test_fp32_processors_and_cfg_match_reference_golden(run):
    """Row a8: ConditionalTemperature + LookbackBias(types_first=True) ("tf"), classifier-free guidance with a
    negative prompt ("cfg"), and both with TimeshiftBias and the lookback / lookahead EOS windows ("all"):
    greedy ids BIT-EXACT vs the reference's `model_generate`, processed scores of every step within 5e-4."""
    from mapperatorinator_amd.server import build_sampling, model_generate
    g, tok, sd, audio, tgt, runs = types_first_case()
    model = build("tiny", tok, sd, int(g["src"]), tgt, torch.float32)
    prompt, neg = torch.from_numpy(g["prompt"]), torch.from_numpy(g["negative"])
    kw = gen_kwargs(tgt, **runs[run])
    cfg = kw["cfg_scale"] > 1
    mk = dict(inputs=audio, decoder_input_ids=prompt, decoder_attention_mask=prompt.ne(0))
    if cfg:
        mk.update(negative_prompt=neg, negative_prompt_attention_mask=neg.ne(0))
    ids, stats = model_generate(model, tok, mk, kw)
    want = g["ids_" + run]
    assert ids.shape == want.shape and np.array_equal(ids.numpy(), want), np.argwhere(ids.numpy() != want)[:3]
    sp, eos = build_sampling(tok, kw, tgt)
    out = model.engine.generate(audio, prompt, prompt.ne(0), eos, sp, dump_logits=True,
                                negative_prompt=neg if cfg else None)
    assert torch.equal(out["tokens"], ids)
    scores = torch.from_numpy(g["scores_" + run])
    P = prompt.shape[1]
    lg = out["logits"].cpu()
    assert lg.shape[1] == prompt.shape[0]
    worst = 0.0
    for i in range(min(scores.shape[0], out["n_cols"] - P)):
        worst = max(worst, assert_scores_close(lg[P + i], scores[i], 5e-4, sp.ts_start if sp.lookback_types_first else None))
    print(run, "worst |dscore| vs reference", worst)


@pytest.mark.parametrize("size", ["tiny", "base"])
def test_bf16_cfg_and_types_first_teacher_forced(size):
    """bf16 storage under classifier-free guidance + the types_first processors, teacher-forced on the bf16-contract
    oracle's own ids: decisive steps agree; guided scores within 0.15 * (1 + 2 (cfg_scale - 1)) (the guidance
    combination amplifies the per-row logit error by |1 - s| + |s|).  "base" = the BASELINE dims and the 1251-frame
    encoder window (the d_model = 768 instantiations of the fused-projection kernels, K/V rows shared by a pair)."""
    from mapperatorinator_amd.server import build_sampling
    from mapperatorinator_amd.t5_engine import T5_PRESETS
    from mh_testing import boost_timed_rows, random_t5_state_dict, synthetic_audio
    g, tok, sd, audio, tgt, runs = types_first_case()
    src = int(g["src"])
    prompt, neg = torch.from_numpy(g["prompt"]), torch.from_numpy(g["negative"])
    if size == "base":
        src, tgt = 1251, 20
        sd = boost_timed_rows(random_t5_state_dict(T5_PRESETS["base"], tok.vocab_size_in, tok.vocab_size_out, seed=9,
                                                   lm_head_gain=6.0), tok, float(g["timed_gain"]))
        audio = synthetic_audio(2, 160000, seed=12)
        prompt, neg = prompt[:2], neg[:2]
    model = build(size, tok, sd, src, tgt, torch.bfloat16)
    kw = gen_kwargs(tgt, **runs["all"])
    sp, eos = build_sampling(tok, kw, tgt)
    o = oracle_for(size, sd, rounding="bf16")
    enc_o = o.encode_audio(audio)
    okw = oracle_processor_kwargs(sp)
    sos = [sp.sos_ids[i] for i in range(sp.n_sos)]
    free = o.generate(enc_o, prompt, prompt.ne(0), [], tgt, sp.ts_start, sp.ts_end, sos, negative_prompt=neg, **okw)
    forced = torch.zeros((prompt.shape[0], tgt), dtype=torch.long)
    forced[:, :free.shape[1]] = free
    want, scores = o.generate(enc_o, prompt, prompt.ne(0), [], tgt, sp.ts_start, sp.ts_end, sos, forced=forced,
                              return_logits=True, negative_prompt=neg, **okw)
    out = model.engine.generate(audio, prompt, prompt.ne(0), [], sp, forced=forced, dump_logits=True, negative_prompt=neg)
    got, lg = out["tokens"], out["logits"].cpu()
    P = prompt.shape[1]
    tol = 0.15 * (1 + 2 * (sp.cfg_scale - 1)) / min(sp.temperature, *[sp.cond_temp[j] for j in range(sp.n_cond)])
    n_cmp = n_bad = n_tie = 0
    worst = 0.0
    for i, s_ in enumerate(scores):
        col = P + i
        a, b_ = lg[col].clone(), s_.clone()
        a[:, sp.ts_start] = 0
        b_[:, sp.ts_start] = 0      # the eos-extra slot (see conftest.assert_scores_close)
        fin = torch.isfinite(a) & torch.isfinite(b_)
        worst = max(worst, (a[fin] - b_[fin]).abs().max().item())
        top2 = s_.topk(2, dim=-1).values
        gap = top2[:, 0] - top2[:, 1]
        for b in range(prompt.shape[0]):
            n_cmp += 1
            if got[b, col] != want[b, col]:
                if gap[b] > 2 * tol:
                    n_bad += 1
                else:
                    n_tie += 1
    print(f"bf16 cfg+types_first teacher-forced: {n_cmp} steps, {n_tie} near-tie flips, {n_bad} real mismatches, "
          f"worst |dscore| {worst:.3f} (tol {tol:.3f})")
    assert n_bad == 0
    assert worst < tol
    assert n_tie <= 0.1 * n_cmp


@pytest.mark.parametrize("seed", [101, 202])
def test_fp32_fresh_seeds_vs_oracle(seed):
    """ragged left-padded prompts, EOS inside the run, logits dump parity."""
    from mapperatorinator_amd import Tokenizer
    from mapperatorinator_amd.server import build_sampling
    from mapperatorinator_amd.t5_engine import T5_PRESETS
    from mh_testing import random_t5_state_dict, synthetic_audio
    src, tgt = 251, 40
    tok = Tokenizer.benchmark_vocab(src_seq_len=src)
    sd = random_t5_state_dict(T5_PRESETS["tiny"], tok.vocab_size_in, tok.vocab_size_out, seed=seed, lm_head_gain=8.0)
    model = build("tiny", tok, sd, src, tgt, torch.float32)
    audio = synthetic_audio(4, 32000, seed=seed)
    prompt = torch.tensor([[0, 0, 0, 1], [0, 1, 30, 500], [1, 60, 501, 61], [0, 0, 1, 100]])
    mask = prompt.ne(0)
    ts0, ts1 = ts_range(tok)
    o = oracle_for("tiny", sd)
    enc_o = o.encode_audio(audio)
    # choose an EOS set that certainly triggers: the ids the oracle emits around step 10
    free = o.generate(enc_o, prompt, mask, [tok.eos_id], tgt, ts0, ts1, [tok.sos_id])
    eos_extra = [int(free[0, 12]), int(free[2, 20])]
    want, scores = o.generate(enc_o, prompt, mask, [tok.eos_id] + eos_extra, tgt, ts0, ts1, [tok.sos_id], return_logits=True)
    sp, _ = build_sampling(tok, gen_kwargs(tgt), tgt)
    out = model.engine.generate(audio, prompt, mask, [tok.eos_id] + eos_extra, sp, dump_logits=True)
    got = out["tokens"]
    assert got.shape == want.shape, (got.shape, want.shape)
    assert torch.equal(got, want), (got, want)
    P = prompt.shape[1]
    lg = out["logits"].cpu()
    for i, s in enumerate(scores):
        fin = torch.isfinite(s)
        assert torch.equal(fin, torch.isfinite(lg[P + i]))
        assert (lg[P + i][fin] - s[fin]).abs().max().item() < 5e-4


@pytest.mark.parametrize("size,B,src,ns,tgt", [("tiny", 5, 251, 32000, 40), ("small", 2, 1251, 160000, 48),
                                              ("large", 2, 251, 32000, 24)])   # config-5 dims (d 1024, 16 heads, d_ff 2816, 24+24 layers)
def test_bf16_teacher_forced_vs_bf16_oracle(size, B, src, ns, tgt):
    from mapperatorinator_amd import Tokenizer
    from mapperatorinator_amd.server import build_sampling
    from mapperatorinator_amd.t5_engine import T5_PRESETS
    from mh_testing import random_t5_state_dict, synthetic_audio
    tok = Tokenizer.benchmark_vocab(src_seq_len=src)
    sd = random_t5_state_dict(T5_PRESETS[size], tok.vocab_size_in, tok.vocab_size_out, seed=77, lm_head_gain=6.0)
    model = build(size, tok, sd, src, tgt, torch.bfloat16)
    audio = synthetic_audio(B, ns, seed=3)
    prompt = torch.tensor([[1]] * B)
    ts0, ts1 = ts_range(tok)
    o = oracle_for(size, sd, rounding="bf16")
    enc_o = o.encode_audio(audio)
    enc_h = model.engine.encode(audio.cuda()).float().cpu()
    e = (enc_h - enc_o).abs()
    print(size, "bf16 encoder: max abs", e.max().item(), "mean abs", e.mean().item(), "scale", enc_o.abs().max().item())
    assert e.mean().item() < 0.02 and e.max().item() < 0.35
    free = o.generate(enc_o, prompt, None, [tok.eos_id], tgt, ts0, ts1, [tok.sos_id])
    forced = torch.zeros((B, tgt), dtype=torch.long)
    forced[:, :free.shape[1]] = free
    want, scores = o.generate(enc_o, prompt, None, [tok.eos_id], tgt, ts0, ts1, [tok.sos_id], forced=forced, return_logits=True)
    sp, _ = build_sampling(tok, gen_kwargs(tgt), tgt)
    out = model.engine.generate(audio, prompt, None, [tok.eos_id], sp, forced=forced, dump_logits=True)
    got, lg = out["tokens"], out["logits"].cpu()
    n_cmp = n_bad = n_tie = 0
    worst = 0.0
    for i, s in enumerate(scores):
        col = 1 + i
        top2 = s.topk(2, dim=-1).values
        gap = top2[:, 0] - top2[:, 1]
        fin = torch.isfinite(s)
        worst = max(worst, (lg[col][fin] - s[fin]).abs().max().item())
        for b in range(B):
            n_cmp += 1
            if got[b, col] != want[b, col]:
                if gap[b] > GAP_BF16:
                    n_bad += 1
                else:
                    n_tie += 1
    print(f"{size} bf16 teacher-forced: {n_cmp} steps, {n_tie} near-tie flips, {n_bad} real mismatches, worst |dlogit| {worst:.3f}")
    assert n_bad == 0
    assert worst < 0.15
    assert n_tie <= 0.05 * n_cmp


def test_full_size_base_bf16_properties():
    """BASELINE config 2 shape (osuT5-base, bf16, B=32, 10 s chunks): size-independent properties --
    determinism, batch-composition independence (row b of a B=32 run == the same chunk run alone),
    monotone TIME_SHIFTs, pad-after-EOS, stats bookkeeping."""
    from mapperatorinator_amd import Tokenizer
    from mapperatorinator_amd.server import model_generate
    from mapperatorinator_amd.t5_engine import T5_PRESETS
    from mh_testing import random_t5_state_dict, synthetic_audio
    src, tgt, B = 1251, 96, 32
    tok = Tokenizer.benchmark_vocab(src_seq_len=src)
    sd = random_t5_state_dict(T5_PRESETS["base"], tok.vocab_size_in, tok.vocab_size_out, seed=5, lm_head_gain=6.0)
    model = build("base", tok, sd, src, tgt, torch.bfloat16)
    audio = synthetic_audio(B, 160000, seed=8)
    prompt = torch.tensor([[1]] * B)
    ts0, ts1 = ts_range(tok)
    eos = gen_kwargs(tgt, lookahead_time=2000)     # TIME_SHIFT >= 8 s ends a row -> rows finish at different steps
    mk = dict(inputs=audio, decoder_input_ids=prompt, decoder_attention_mask=prompt.ne(0))
    ids, stats = model_generate(model, tok, mk, eos)
    ids_again, _ = model_generate(model, tok, mk, eos)
    assert torch.equal(ids, ids_again), "non-deterministic decode"
    assert ids.shape[0] == B and ids.shape[1] <= tgt
    eos_ids = set([tok.eos_id] + list(range(ts1 - 200, ts1)))
    for b in range(B):
        row = ids[b].tolist()
        hit = [i for i, t in enumerate(row[1:], 1) if t in eos_ids]
        if hit:
            assert all(t == 0 for t in row[hit[0] + 1:]), "tokens after EOS must be pad"
        last = -1
        for t in row[1:]:
            if ts0 <= t < ts1:
                assert t - ts0 >= last, "TIME_SHIFT went backwards"
                last = t - ts0
    assert stats["generated_tokens"] == int((ids != 0).sum().item() - B)
    # batch-composition independence for a few rows (bf16: same kernels, same reduction order per row)
    for b in (0, 13, 31):
        one, _ = model_generate(model, tok, dict(inputs=audio[b:b + 1], decoder_input_ids=prompt[:1],
                                                 decoder_attention_mask=prompt[:1].ne(0)), eos)
        n = one.shape[1]
        assert torch.equal(one[0], ids[b, :n]) and (ids[b, n:] == 0).all(), f"row {b} depends on its batch"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,chains", [(40, 0), (24, 1), (64, 0)])
def test_rows_do_not_depend_on_the_rows_beside_them(dtype, B, chains):
    """Chains of more than 16 rows use the 2- / 4-fragment GEMV (MF >= 2), chains of <= 16 rows the whole-line one
    (MF == 1): both must add a row's products in the same order (k-block pairs per wave), so a chunk decodes to the same
    ids alone (MF 1) and inside a batch of 24 (one chain, MF 2), 40 (two chains of 20, MF 2) or 64 rows (two chains of
    32, MF 2).  Every run decodes from the SAME cross K/V rows (the encoder of the whole batch): the encoder's GEMMs choose
    their tile family -- and with it the fp32 summation order -- by the number of rows, which in bf16 moves near-tie
    decisions of a solo run (documented at option gemm_splitk_tiles); the claim here is about the decode step."""
    from mapperatorinator_amd import Tokenizer, _lib
    from mapperatorinator_amd.server import build_sampling
    from mapperatorinator_amd.t5_engine import T5_PRESETS
    from mh_testing import random_t5_state_dict, synthetic_audio
    src, tgt = 251, 48
    tok = Tokenizer.benchmark_vocab(src_seq_len=src)
    sd = random_t5_state_dict(T5_PRESETS["small"], tok.vocab_size_in, tok.vocab_size_out, seed=9, lm_head_gain=6.0)
    model = build("small", tok, sd, src, tgt, dtype)
    eng = model.engine
    audio = synthetic_audio(B, 32000, seed=12).cuda()
    prompt = torch.tensor([[1]] * B, dtype=torch.int32, device="cuda")
    sp, eos = build_sampling(tok, gen_kwargs(tgt), tgt)
    table = torch.zeros(tok.vocab_size_out, dtype=torch.uint8, device="cuda")
    table[list(eos)] = 1
    kv = eng.cross_kv(eng.encode(audio))
    torch.cuda.synchronize()
    old = _lib.set_option("decode_chains", chains)
    try:
        ids, n_all, _ = eng.decode(kv, prompt, None, table, sp)
    finally:
        _lib.set_option("decode_chains", old)
    ids = ids.cpu()
    rows = sorted(set([0, 7, 17, B - 1] + list(range(3, B, 5))))
    for b in rows:
        one, n_one, _ = eng.decode(kv[:, :, b:b + 1].contiguous(), prompt[:1], None, table, sp)
        n = int(n_one)
        one = one.cpu()
        assert torch.equal(one[0, :n], ids[b, :n]) and (ids[b, n:] == 0).all(), f"row {b} of {B} depends on its batch"



def test_sampling_topk_topp_distribution():
    """do_sample path (row a9): sampling parity is RNG-bound, so it is checked distributionally --
    every sampled id lies inside the top-k / nucleus set of the processed scores of its step, identical rows
    draw from the softmax of the kept set (chi-square), and the stream is a deterministic function of the seed."""
    from mapperatorinator_amd import Tokenizer
    from mapperatorinator_amd.server import build_sampling
    from mapperatorinator_amd.t5_engine import T5_PRESETS
    from mh_testing import random_t5_state_dict, synthetic_audio
    src, tgt, B = 251, 24, 64
    tok = Tokenizer.benchmark_vocab(src_seq_len=src)
    sd = random_t5_state_dict(T5_PRESETS["tiny"], tok.vocab_size_in, tok.vocab_size_out, seed=31, lm_head_gain=2.0)
    model = build("tiny", tok, sd, src, tgt, torch.float32)
    audio = synthetic_audio(1, 32000, seed=2).repeat(B, 1)          # identical rows -> identical step-1 scores
    prompt = torch.tensor([[1]] * B)

    def run(**kw):
        sp, eos = build_sampling(tok, gen_kwargs(tgt, do_sample=True, **kw), tgt)
        out = model.engine.generate(audio, prompt, None, [], sp, dump_logits=True)
        return out["tokens"], out["logits"].cpu()

    from mapperatorinator_amd.server import reset_seed_calls
    reset_seed_calls()
    toks, lg = run(top_k=5, temperature=0.8, seed=1234)
    toks_next, _ = run(top_k=5, temperature=0.8, seed=1234)       # the SECOND call with a seed draws a different stream ...
    reset_seed_calls()
    toks2, _ = run(top_k=5, temperature=0.8, seed=1234)           # ... and the same sequence of calls reproduces itself
    toks3, _ = run(top_k=5, temperature=0.8, seed=99)
    assert torch.equal(toks, toks2) and not torch.equal(toks, toks3) and not torch.equal(toks, toks_next)
    for col in range(1, toks.shape[1]):
        top = lg[col].topk(5, dim=-1)
        assert (toks[:, col, None] == top.indices).any(-1).all(), f"column {col}: id outside the top-k set"
    # chi-square of the first sampled column against softmax over the kept 5 (all rows share the scores)
    top = lg[1][0].topk(5)
    probs = torch.softmax(top.values, -1)
    counts = torch.stack([(toks[:, 1] == i).sum() for i in top.indices]).float()
    # pool several seeds for a usable sample size
    for seed in range(20):
        t, _ = run(top_k=5, temperature=0.8, seed=5000 + seed)
        counts += torch.stack([(t[:, 1] == i).sum() for i in top.indices]).float()
    n = counts.sum()
    chi2 = (((counts - n * probs) ** 2) / (n * probs)).sum().item()
    print("sampling chi2 (4 dof):", chi2, "counts", counts.tolist(), "expected", (n * probs).tolist())
    assert chi2 < 25.0      # p ~ 5e-5 for 4 degrees of freedom
    # nucleus: kept set = smallest prefix of the sorted probabilities whose mass reaches top_p
    toks_p, lg_p = run(top_k=0, top_p=0.6, temperature=1.0, seed=7)
    for col in range(1, toks_p.shape[1]):
        p_sorted, idx = torch.softmax(lg_p[col], -1).sort(-1, descending=True)
        keep = (p_sorted.cumsum(-1) - p_sorted) < 0.6 + 1e-4
        for b in range(0, B, 7):
            allowed = set(idx[b][keep[b]].tolist())
            assert int(toks_p[b, col]) in allowed, f"column {col} row {b}: id outside the nucleus"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_long_left_padded_prompts_batched_prefill(dtype):
    """Sequential-window prompts (lookback context, processor.py:336-342): P = 45 with ragged left padding.
    The batched prefill (MFMA GEMMs + causal flash attention filling the KV caches) must give the same tokens
    as feeding the prompt token by token, and -- in fp32 -- the same tokens as the CPU oracle."""
    from mapperatorinator_amd import Tokenizer
    from mapperatorinator_amd.server import build_sampling
    from mapperatorinator_amd.t5_engine import T5_PRESETS
    from mh_testing import random_t5_state_dict, synthetic_audio
    src, tgt, B, P = 251, 80, 5, 45
    tok = Tokenizer.benchmark_vocab(src_seq_len=src)
    sd = random_t5_state_dict(T5_PRESETS["tiny"], tok.vocab_size_in, tok.vocab_size_out, seed=404, lm_head_gain=8.0)
    model = build("tiny", tok, sd, src, tgt, dtype)
    audio = synthetic_audio(B, 32000, seed=6)
    g = torch.Generator().manual_seed(9)
    prompt = torch.randint(3, tok.vocab_size_out, (B, P), generator=g)
    ts0, ts1 = ts_range(tok)
    for b, npad in enumerate([0, 44, 17, 30, 1]):
        prompt[b, :npad] = 0
        prompt[b, npad] = 1                       # SOS after the padding
    mask = prompt.ne(0)
    sp, _ = build_sampling(tok, gen_kwargs(tgt), tgt)
    from mapperatorinator_amd import _lib
    old = _lib.set_option("decode_prefill", 1)
    try:
        fast = model.engine.generate(audio, prompt, mask, [tok.eos_id], sp)["tokens"]
        _lib.set_option("decode_prefill", 0)
        slow = model.engine.generate(audio, prompt, mask, [tok.eos_id], sp)["tokens"]
    finally:
        _lib.set_option("decode_prefill", old)
    assert fast.shape == slow.shape
    agree = (fast == slow).float().mean().item()
    print(dtype, "prefill vs token-by-token agreement", agree)
    if dtype == torch.float32:
        assert torch.equal(fast, slow)
        o = oracle_for("tiny", sd)
        want = o.generate(o.encode_audio(audio), prompt, mask, [tok.eos_id], tgt, ts0, ts1, [tok.sos_id])
        assert torch.equal(fast, want)
    else:
        assert agree > 0.9      # bf16: the two paths round differently (flash vs single-query softmax)


def test_model_object_generate_and_forward_seam_b2():
    """B2: `model.generate(**model_kwargs, **generate_kwargs, logits_processor=[...], eos_token_id=[...])` as the
    reference's model_generate calls it == our model_generate; `model.forward(frames=, decoder_input_ids=, ...)`
    teacher-forced logits == the oracle's step-by-step logits (fp32, 5e-4) incl. left-padded prompts."""
    from mapperatorinator_amd.server import get_eos_token_id, model_generate
    g, size, tok, sd, audio, src, tgt = golden_case("t5_tiny")
    model = build(size, tok, sd, src, tgt, torch.float32)
    prompt = torch.from_numpy(g["prompt"])
    ts0, ts1 = ts_range(tok)

    class MonotonicTimeShiftLogitsProcessor:      # recognised by class name, like the reference's objects
        time_shift_start, time_shift_end, sos_ids = ts0, ts1, torch.tensor([tok.sos_id])

    class TimeshiftBias:
        timeshift_bias, time_range = 0.35, slice(ts0, ts1)

    class TemperatureLogitsWarper:
        temperature = 0.7

    eos = get_eos_token_id(tok, lookahead_time=3000, context_type="map")
    ids = model.generate(inputs=audio, decoder_input_ids=prompt, decoder_attention_mask=prompt.ne(0), do_sample=False,
                         num_beams=1, top_p=1.0, top_k=0, max_length=tgt, pad_token_id=0, use_cache=True,
                         past_key_values=object(), eos_token_id=eos,
                         logits_processor=[MonotonicTimeShiftLogitsProcessor(), TimeshiftBias(), TemperatureLogitsWarper()])
    assert ids.device.type == "cuda" and ids.dtype == torch.int64
    assert np.array_equal(ids.cpu().numpy(), g["ids_processors"])       # = the reference's own output for these kwargs
    torch.manual_seed(11)       # beam-sample through the HF-style entry: the device's torch.multinomial, repeatable under a seed
    a = model.generate(inputs=audio, decoder_input_ids=prompt, decoder_attention_mask=prompt.ne(0), num_beams=2, do_sample=True,
                       top_p=0.9, max_length=tgt, pad_token_id=0, eos_token_id=eos)
    torch.manual_seed(11)
    b = model.generate(inputs=audio, decoder_input_ids=prompt, decoder_attention_mask=prompt.ne(0), num_beams=2, do_sample=True,
                       top_p=0.9, max_length=tgt, pad_token_id=0, eos_token_id=eos)
    assert torch.equal(a, b) and a.shape[0] == prompt.shape[0] and torch.equal(a[:, :prompt.shape[1]].cpu(), prompt)

    # forward: teacher-forced on the reference's greedy ids
    seq = torch.from_numpy(g["ids"])[:, :-1]
    mask = torch.ones_like(seq, dtype=torch.bool)
    mask[:, :prompt.shape[1]] = prompt.ne(0)
    out = model.forward(frames=audio, decoder_input_ids=seq, decoder_attention_mask=mask)
    lg = out.logits.cpu()
    assert lg.shape == (seq.shape[0], seq.shape[1], tok.vocab_size_out)
    o = oracle_for(size, sd)
    enc_o = o.encode_audio(audio)
    ckv = o.cross_kv(enc_o)
    B, T = seq.shape
    cache = [(torch.zeros(B, o.H, T, 64), torch.zeros(B, o.H, T, 64)) for _ in range(o.nd)]
    worst = 0.0
    valid = mask.clone()
    for pos in range(T):
        want = o.decoder_step(seq[:, pos], pos, cache, ckv, mask)
        rows = valid[:, pos]            # left-pad query rows are unused garbage on both sides
        worst = max(worst, (lg[rows, pos] - want[rows]).abs().max().item())
    print("forward logits worst abs err", worst)
    assert worst < 5e-4


@pytest.mark.parametrize("beams", [1, 2])
def test_window_scheduler_matches_sequential_loop(beams, monkeypatch):
    """`beams` = 2: the reference's timing pass decodes with two beams (processor.py:159 forwards `num_beams`); the scheduler
    must beam-search its waves too (it used to decode them greedily without a word).
    8f rank 1: three songs with 3 / 2 / 4 dependent windows through SequentialWindowScheduler (all windows encoded up
    front, wave w decodes window w of every song as one batch) == the reference-shaped loop (one batch-1
    `model_generate` per window, in order).  Each prompt is built from the previous window's output, so a scheduling
    mistake (wrong K/V row, wrong order, stale prompt) changes the tokens."""
    from mapperatorinator_amd.scheduler import SequentialWindowScheduler, SongJob
    from mapperatorinator_amd.server import model_generate
    g, size, tok, sd, _, src, tgt = golden_case("t5_tiny")
    from mh_testing import synthetic_audio
    model = build(size, tok, sd, src, tgt, torch.float32)
    n_windows = [3, 2, 4]
    songs = [synthetic_audio(n, int(g["n_samples"]), seed=40 + k) for k, n in enumerate(n_windows)]
    ts0, ts1 = ts_range(tok)

    def kwargs_for(w, n):   # first window: no lookback trimming; last: no lookahead (processor.py:327-328)
        return gen_kwargs(tgt, lookback_time=400 if w != 0 else 0, lookahead_time=3000 if w != n - 1 else 0, temperature=0.9,
                          num_beams=beams)

    def prompt_from(prev):  # sos + up to 3 non-special ids of the previous window's output
        if prev is None:
            return torch.tensor([[tok.sos_id]])
        carry = [t for t in prev.tolist() if t > 2][-3:]
        return torch.tensor([[tok.sos_id] + carry])

    # the reference-shaped loop
    want = []
    for k, n in enumerate(n_windows):
        prev, rows = None, []
        for w in range(n):
            prompt = prompt_from(prev)
            ids, _ = model_generate(model, tok, dict(inputs=songs[k][w:w + 1], decoder_input_ids=prompt,
                                                     decoder_attention_mask=prompt.ne(0)), kwargs_for(w, n))
            prev = ids[0, prompt.shape[1]:]
            rows.append(ids[0])
        want.append(rows)

    got = [[None] * n for n in n_windows]
    state = [None] * len(n_windows)

    def make_job(k, n):
        def prompt_fn(w):
            return dict(decoder_input_ids=prompt_from(state[k]), generate_kwargs=kwargs_for(w, n))

        def on_result(w, row, st):
            p = prompt_from(state[k]).shape[1]
            got[k][w] = row
            state[k] = row[p:]
            assert st["generated_tokens"] == int((row[p:] != 0).sum())
        return SongJob(frames=songs[k], prompt_fn=prompt_fn, on_result=on_result)

    from mapperatorinator_amd import beam as beam_mod
    beam_calls = []
    real_beam_search = beam_mod.beam_search

    def counting_beam_search(*a, **k):
        beam_calls.append(a[6] if len(a) > 6 else k.get("num_beams"))
        return real_beam_search(*a, **k)
    monkeypatch.setattr(beam_mod, "beam_search", counting_beam_search)
    sched = SequentialWindowScheduler(model, tok, encode_batch=4, decode_batch=32)
    stats = sched.run([make_job(k, n) for k, n in enumerate(n_windows)])
    # every decode call of the scheduler went through beam search with the asked number of beams -- or none did
    assert beam_calls == ([beams] * stats["decode_calls"] if beams > 1 else [])
    assert stats["windows"] == sum(n_windows) and stats["encode_calls"] == 3
    for k, n in enumerate(n_windows):
        for w in range(n):
            a, b = got[k][w], want[k][w]
            assert a.shape == b.shape and torch.equal(a, b), (k, w, a.tolist(), b.tolist())
    # fewer decode calls than windows: songs were interleaved
    assert stats["decode_calls"] < sum(n_windows)


def test_conditioning_embedders_fp32_match_reference_golden():
    """tests/golden/t5_tiny_cond.npz: the reference wrapper with its difficulty / mapper-style / song-position embedders on
    (modeling_mapperatorinator.py:104-128, 395-414).  `model_generate` with the same `difficulty` / `mapper_idx` /
    `song_position` model kwargs must return the reference's greedy ids bit for bit (fp32 storage): the embedders run on
    the host, their output reaches the device as the per-chunk row bias of the encoder input projection
    (mh_t5_encode_cond).  The encoder states are held to the golden slice."""
    from test_oracle_pinned import _cond_case
    from mapperatorinator_amd.modeling import MapperatorinatorHIP
    from mapperatorinator_amd.server import model_generate
    from mapperatorinator_amd.t5_engine import T5_PRESETS
    g, tok, sd, audio = _cond_case()
    tgt = int(g["tgt_len"])
    model = MapperatorinatorHIP(sd, T5_PRESETS["tiny"], vocab_size_in=tok.vocab_size_in, vocab_size_out=tok.vocab_size_out,
                                src_seq_len=int(g["src_len"]), tgt_seq_len=tgt, dtype=torch.float32)
    assert model.cond.active
    prompt = torch.from_numpy(g["prompt"])
    mk = dict(inputs=audio, decoder_input_ids=prompt, decoder_attention_mask=prompt.ne(0),
              difficulty=torch.from_numpy(g["difficulty"]), mapper_idx=torch.from_numpy(g["mapper_idx"]),
              song_position=torch.from_numpy(g["song_position"]))
    ids, _ = model_generate(model, tok, mk, gen_kwargs(tgt))
    assert ids.shape == g["ids"].shape and np.array_equal(ids.numpy(), g["ids"]), np.argwhere(ids.numpy() != g["ids"])[:3]
    enc = model.get_encoder()(frames=audio, difficulty=mk["difficulty"], mapper_idx=mk["mapper_idx"],
                              song_position=mk["song_position"]).last_hidden_state.float().cpu()
    assert np.abs(enc[:, ::13, ::7].numpy() - g["enc_slice"]).max() < 2e-4
    with pytest.raises(ValueError):
        model_generate(model, tok, dict(inputs=audio, decoder_input_ids=prompt, decoder_attention_mask=prompt.ne(0)), gen_kwargs(tgt))


@pytest.mark.parametrize("run", ["b2", "b3", "b2p", "b3p", "b2g", "b3g", "b2s", "b3s", "b2sg"])
def test_fp32_beam_search_matches_reference_golden(run):
    """`num_beams` 2 / 3 through `model_generate` on the HIP path (mapperatorinator_amd/beam.py over mh_t5_step /
    mh_t5_reorder_cache): the ids the REFERENCE returned for the same inputs through HF beam search and its cache reorder
    (tests/golden/t5_tiny_beam.npz), bit for bit -- hypotheses of different lengths, processors and EOS windows included.  `b2g` /
    `b3g`: classifier-free guidance under beams (doubled rows, HF's processor on log-probabilities, the reference's
    `beam_idx.repeat(2)` cache gather).  `b2s` / `b3s` / `b2sg`: beam-SAMPLE (do_sample under beams; HF's top-k / top-p warpers with
    `min_tokens_to_keep = #eos + 1`, K continuations drawn without replacement and kept in draw order) -- the reference and this
    run draw through the same `testing.SeededMultinomial` (a CPU and a GPU torch generator cannot agree), handed in as
    `generate_kwargs["beam_sample_fn"]`; without it the draw is torch.multinomial on the device (last assertion)."""
    import json
    from mapperatorinator_amd import Tokenizer
    from mapperatorinator_amd.server import model_generate
    from mapperatorinator_amd.t5_engine import T5_PRESETS
    from mh_testing import DIVERSE_GAINS, SeededMultinomial, random_t5_state_dict, synthetic_audio_varied
    g = np.load(f"{GOLDEN}/t5_tiny_beam.npz")
    src, tgt = int(g["src"]), int(g["tgt"])
    tok = Tokenizer.benchmark_vocab(src_seq_len=src)
    sd = random_t5_state_dict(T5_PRESETS["tiny"], tok.vocab_size_in, tok.vocab_size_out, seed=int(g["wseed"]),
                              lm_head_gain=float(g["gain"]), gains=DIVERSE_GAINS)
    audio = synthetic_audio_varied(g["prompt"].shape[0], int(g["ns"]), seed=int(g["aseed"]))
    model = build("tiny", tok, sd, src, tgt, torch.float32)
    prompt = torch.from_numpy(g["prompt"])
    kw = json.loads(str(g["runs"]))[run]
    mk = dict(inputs=audio, decoder_input_ids=prompt, decoder_attention_mask=prompt.ne(0))
    if kw.get("cfg_scale", 1.0) > 1.0:
        neg = torch.from_numpy(g["negative"])
        mk.update(negative_prompt=neg, negative_prompt_attention_mask=neg.ne(0))
    sampler = SeededMultinomial(json.loads(str(g["sample_seeds"]))[run]) if kw.get("do_sample") else None
    ids, stats = model_generate(model, tok, mk, gen_kwargs(tgt, **kw, **({"beam_sample_fn": sampler} if sampler else {})))
    want = g["ids_" + run]
    assert ids.shape == want.shape and np.array_equal(ids.numpy(), want), (ids.tolist(), want.tolist())
    assert ids.dtype == torch.int64 and ids.device.type == "cpu" and stats["generated_tokens"] > 0
    if sampler is None:
        # round 6: the greedy-beam runs above went through mh_beam_step (ONE kernel per token for the whole bookkeeping); the torch-op
        # form of the same algorithm must return the same ids, and forcing the kernel on a beam-sample call must refuse
        from mapperatorinator_amd import beam as _beam
        calls = []
        orig = _beam._beam_search_kernel
        _beam._beam_search_kernel = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
        try:
            ids_k, _ = model_generate(model, tok, mk, gen_kwargs(tgt, **kw))
        finally:
            _beam._beam_search_kernel = orig
        assert calls and np.array_equal(ids_k.numpy(), want)
        ids_t, _ = model_generate(model, tok, mk, gen_kwargs(tgt, beam_use_kernel=False, **kw))
        assert np.array_equal(ids_t.numpy(), want)
    else:
        with pytest.raises(NotImplementedError, match="mh_beam_step"):
            model_generate(model, tok, mk, gen_kwargs(tgt, beam_use_kernel=True, **kw))
    if sampler is not None:
        assert sampler.calls == want.shape[1] - prompt.shape[1]          # one draw of K continuations per step, all chunks at once
        torch.manual_seed(5)
        own, _ = model_generate(model, tok, mk, gen_kwargs(tgt, **kw))       # the device's own torch.multinomial
        torch.manual_seed(5)
        again, _ = model_generate(model, tok, mk, gen_kwargs(tgt, **kw))
        assert torch.equal(own, again) and own.shape[0] == want.shape[0] and not np.array_equal(own.numpy()[:, :want.shape[1]], want)


def test_generate_with_encoder_outputs_of_the_reference_signature():
    """`Mapperatorinator.generate(encoder_outputs=BaseModelOutput(last_hidden_state=...))` -- the route the oracle harness
    itself drives the reference through (oracle/ref_harness.py reference_generate).  The HIP object takes the states `get_encoder()`
    returned and must produce the ids of the audio route."""
    import types as _types
    from mapperatorinator_amd.t5_engine import T5_PRESETS
    g, size, tok, sd, audio, src, tgt = t5_golden_case("t5_tiny")
    model = build(size, tok, sd, src, tgt, torch.float32)
    prompt = torch.from_numpy(g["prompt"])
    enc = model.get_encoder()(frames=audio).last_hidden_state
    assert enc.shape == (audio.shape[0], src, T5_PRESETS[size].d_model)
    kw = dict(decoder_input_ids=prompt, decoder_attention_mask=prompt.ne(0), max_length=tgt, do_sample=False, eos_token_id=[tok.eos_id])
    a = model.generate(inputs=audio, **kw).cpu()
    b = model.generate(encoder_outputs=_types.SimpleNamespace(last_hidden_state=enc), **kw).cpu()
    # (no logits_processor list here, so these are not the golden's ids -- model_generate adds the reference's processors; the two
    # ROUTES must agree bit for bit)
    assert torch.equal(a, b) and a.shape[1] > prompt.shape[1]
    with pytest.raises(ValueError, match="encoder_states"):
        model.generate(encoder_outputs=_types.SimpleNamespace(last_hidden_state=enc[:, :-1]), **kw)
    with pytest.raises(ValueError, match="either inputs"):
        model.generate(**kw)


def test_request_batcher_answers_every_request_like_a_call_of_its_own():
    """`RequestBatcher` (the batching policy of the reference's InferenceServer, server.py:343-424) over the HIP engine:
    six requests with ragged batch sizes and prompt widths in two generate-kwargs groups, max_batch_size 16.  Batches:
    [A 9 rows + B 7] (A left-padded to B's width), [D 16 of 20], [D 4 + E 3], [C 3 + F 1] (C padded to F's width).
    Every request gets back, bit for bit (fp32, greedy), what `model_generate` returns for it alone under the same left
    padding -- rows do not depend on their batch; a different padding WIDTH shifts the key chunking of the attention
    sums, which is an fp32 reordering in the reference as well."""
    from mapperatorinator_amd import Tokenizer
    from mapperatorinator_amd.server import RequestBatcher, model_generate
    from mapperatorinator_amd.t5_engine import T5_PRESETS
    from mh_testing import random_t5_state_dict, synthetic_audio
    src, tgt = 251, 40
    tok = Tokenizer.benchmark_vocab(src_seq_len=src)
    sd = random_t5_state_dict(T5_PRESETS["small"], tok.vocab_size_in, tok.vocab_size_out, seed=21, lm_head_gain=6.0)
    model = build("small", tok, sd, src, tgt, torch.float32)
    g = torch.Generator().manual_seed(4)
    plain, biased = gen_kwargs(tgt), gen_kwargs(tgt, timeshift_bias=0.3)
    reqs, pad_to = [], [3, 3, 4, 2, 2, 4]
    for i, (rows, width, gk) in enumerate([(9, 1, plain), (7, 3, plain), (3, 2, biased), (20, 2, plain), (3, 2, plain), (1, 4, biased)]):
        ids = torch.randint(20, tok.vocab_size_in - 1, (rows, width), generator=g)
        ids[:, 0] = 1
        reqs.append((dict(inputs=synthetic_audio(rows, 32000, seed=50 + i), decoder_input_ids=ids,
                          decoder_attention_mask=torch.ones_like(ids)), gk))
    batcher = RequestBatcher(model, tok, max_batch_size=16)
    records = [batcher.submit(mk, gk) for mk, gk in reqs]
    assert batcher.drain() == 4 and not batcher.pending
    for (mk, gk), rec, width in zip(reqs, records, pad_to):
        pad = width - mk["decoder_input_ids"].shape[1]
        padded = dict(mk, decoder_input_ids=torch.nn.functional.pad(mk["decoder_input_ids"], (pad, 0)),
                      decoder_attention_mask=torch.nn.functional.pad(mk["decoder_attention_mask"], (pad, 0)))
        alone, stats = model_generate(model, tok, padded, gk)
        got = rec["result"]["output"]
        assert rec["done"] and got.shape[0] == mk["inputs"].shape[0]
        n = min(got.shape[1], alone.shape[1] - pad)          # a batch runs until its longest row ends: pad columns may differ
        assert torch.equal(got[:, :n], alone[:, pad:pad + n]) and (got[:, n:] == 0).all() and (alone[:, pad + n:] == 0).all()
        assert rec["result"]["stats"]["generated_tokens"] == stats["generated_tokens"]


def test_sharded_generate_on_rccl_world_1():
    """SURVEY 8e on the backend the N-GPU job uses: an RCCL process group (one rank: what this box offers) carries the token
    streams of `model_generate` and the device-resident coordinates of a DiT refine through ONE all_gather; both must come
    back bit-equal to the plain calls.  Own process: a process group is process-global state (tools/nccl_world1_check.py)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    p = subprocess.run([sys.executable, os.path.join(root, "tools", "nccl_world1_check.py")], env=env, capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-1000:], p.stderr[-3000:])
    line = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")][-1]
    assert line["tokens_equal"] and line["coords_bit_equal"] and line["backend"] == "nccl"


# ---- BASELINE configs[4] "fp8 MFMA": MX-fp8 operands for the encoder blocks and the cross-K/V projection ---------------------
def _mx_model(size, tok, sd, src, tgt):
    from mapperatorinator_amd.modeling import MapperatorinatorHIP
    from mapperatorinator_amd.t5_engine import T5_PRESETS
    return MapperatorinatorHIP(sd, T5_PRESETS[size], vocab_size_in=tok.vocab_size_in, vocab_size_out=tok.vocab_size_out,
                               src_seq_len=src, tgt_seq_len=tgt, dtype=torch.bfloat16, device="cuda", enc_operand_dtype="mx8")


@pytest.mark.parametrize("name", ["t5_tiny", "t5_small"])
def test_mx8_encoder_against_the_mx8_contract_oracle(name):
    """enc_operand_dtype = MH_MX8 computes what it says: encoder states of the HIP path against oracle/t5.py under the same
    contract (bf16 storage; the four block projections on the MX-fp8 images of both operands).  Two implementations of a
    quantised network agree up to the elements whose bf16 / e4m3 rounding flips on fp32-order noise, so the gate is statistical:
    mean error a small fraction of the MX mode's own distance from the bf16 mode."""
    from mapperatorinator_amd.t5_engine import T5_PRESETS
    g, size, tok, sd, audio, src, tgt = golden_case(name)
    d = T5_PRESETS[size]
    mx = _mx_model(size, tok, sd, src, tgt)
    plain = build(size, tok, sd, src, tgt, torch.bfloat16)
    _, e_mx = mx.engine.encode(audio.cuda(), want_f32=True)
    _, e_bf = plain.engine.encode(audio.cuda(), want_f32=True)
    torch.cuda.synchronize()
    from oracle import t5 as ot5
    o_mx = ot5.T5Oracle(sd, d.d_model, d.d_ff, d.n_heads, d.n_enc_layers, d.n_dec_layers, rounding="bf16", enc_mx8=True)
    want = o_mx.encode_audio(audio)
    e_mx, e_bf = e_mx.cpu(), e_bf.cpu()
    err = (e_mx - want).abs()
    dist = (want - e_bf).abs()                      # what the MX mode changes
    print(f"{name}: |HIP mx8 - oracle mx8| mean {err.mean():.4f} max {err.max():.3f}; |oracle mx8 - HIP bf16| mean {dist.mean():.4f} "
          f"max {dist.max():.3f}; state rms {want.pow(2).mean().sqrt():.3f}")
    # measured: tiny (2 layers) 1e-4 against a mode distance of 2e-3; small (8 layers) 4e-3 against 8e-3 -- every layer's
    # re-quantisation amplifies the flips of the layer before it
    assert err.mean() < (0.1 if name == "t5_tiny" else 0.75) * dist.mean() + 1e-4
    assert err.mean() < 0.01 * want.pow(2).mean().sqrt()


@pytest.mark.parametrize("size", ["base", "large"])
def test_mx8_one_encoder_block_against_the_contract_oracle(size):
    """The MX-fp8 mode held to its contract WITHOUT compounding: ONE encoder block (+ the final norm) at the dims config 5 quotes
    (osuT5-base / -large, 1251 frames), HIP against oracle/t5.py under the same contract.  With a single block nothing re-quantises
    the differences of a layer before: what is left are the elements whose bf16 / e4m3 rounding flips on fp32 summation order.
    Measured: mean 7.8e-4 (base) / 9.3e-4 (large) of a state with rms 1.0 -- 0.2 bf16 ulp -- against a mode distance of 3.2e-3; 99.0 % /
    98.7 % of the elements within 2 bf16 ulps, max 0.05-0.06 (a flipped e4m3 element is a 12 % change of one operand element; the matrix
    core's 13-bit product alignment, DESIGN section 2, adds ~2^-11 per output).  Gates at ~1.4 x that: a mis-scaled block or a stale
    operand moves EVERY element by the mode distance or more."""
    import dataclasses
    from mapperatorinator_amd import Tokenizer
    from mapperatorinator_amd.modeling import MapperatorinatorHIP
    from mapperatorinator_amd.t5_engine import T5_PRESETS
    from mh_testing import random_t5_state_dict, synthetic_audio_varied
    from oracle import t5 as ot5
    src, tgt = 1251, 16
    d = dataclasses.replace(T5_PRESETS[size], n_enc_layers=1, n_dec_layers=1)
    tok = Tokenizer.benchmark_vocab(src_seq_len=src)
    sd = random_t5_state_dict(d, tok.vocab_size_in, tok.vocab_size_out, seed=61, lm_head_gain=2.0)
    audio = synthetic_audio_varied(2, (src - 1) * 128, seed=17)
    states = {}
    for mode in ("mx8", None):
        m = MapperatorinatorHIP(sd, d, vocab_size_in=tok.vocab_size_in, vocab_size_out=tok.vocab_size_out, src_seq_len=src, tgt_seq_len=tgt,
                                dtype=torch.bfloat16, device="cuda", **({"enc_operand_dtype": mode} if mode else {}))
        states[mode] = m.engine.encode(audio.cuda(), want_f32=True)[1].cpu()
        del m
    want = ot5.T5Oracle(sd, d.d_model, d.d_ff, d.n_heads, 1, 1, rounding="bf16", enc_mx8=True).encode_audio(audio)
    err, dist = (states["mx8"] - want).abs(), (want - states[None]).abs()
    rms = want.pow(2).mean().sqrt().item()
    ulp = rms * 2.0 ** -8
    print(f"one {size} block: |HIP mx8 - oracle mx8| mean {err.mean():.2e} p99 {err.flatten().quantile(0.99):.2e} max {err.max():.2e}; "
          f"mode distance mean {dist.mean():.2e}; state rms {rms:.3f} (bf16 ulp {ulp:.2e}); share within 2 ulp {(err <= 2 * ulp).float().mean():.4f}")
    assert err.mean() <= 0.4 * dist.mean() and err.mean() <= 1.3e-3 * rms
    assert (err <= 2 * ulp).float().mean() >= 0.98 and err.max() <= 0.1 * rms


@pytest.mark.parametrize("name", ["t5_base", "t5_large"])
def test_mx8_encoder_teacher_forced_on_the_reference_fp32_run(name):
    """The MX-fp8 encoder mode at the sizes config 5 quotes, teacher-forced on the ids the fp32 REFERENCE produced
    (tests/golden/t5_base.npz / t5_large.npz): error bound + agreement rate, like the bf16 mode's gate.  fp8 operands change
    the encoder states by ~2^-5 per element before averaging; the decoder (bf16, untouched) sees them through the cross K/V."""
    from mapperatorinator_amd.server import build_sampling
    g, size, tok, sd, audio, src, tgt = golden_case(name)
    ids = torch.from_numpy(g["ids"])
    n_cols = ids.shape[1]
    prompt = torch.from_numpy(g["prompt"])
    P = prompt.shape[1]
    forced = torch.zeros((ids.shape[0], tgt), dtype=torch.long)
    forced[:, :n_cols] = ids
    want = ids[:, P:]
    gap = torch.from_numpy(g["top_vals"][..., 0] - g["top_vals"][..., 1]).T
    live = want.ne(0)
    tv, ti = torch.from_numpy(g["top_vals"]), torch.from_numpy(g["top_ids"]).long()
    res = {}
    for mode in ("mx8", "bf16"):
        model = _mx_model(size, tok, sd, src, tgt) if mode == "mx8" else build(size, tok, sd, src, tgt, torch.bfloat16)
        sp, _ = build_sampling(tok, gen_kwargs(tgt), tgt)
        out = model.engine.generate(audio, prompt, prompt.ne(0), [], sp, forced=forced, dump_logits=True)
        lg = out["logits"].float().cpu()
        ok = lg[P:n_cols].argmax(-1).T == want
        err = (lg[P:n_cols].gather(-1, ti) - tv).abs()[live.T]
        res[mode] = (ok[live].float().mean().item(), ok[live & (gap >= 0.5)].float().mean().item(), ok[live & (gap >= 1.0)].float().mean().item(),
                     err.mean().item(), err.max().item())
        del model
    n_dec = int((live & (gap >= 0.5)).sum())
    print(f"{name} teacher-forced on the fp32 reference: " + "; ".join(
        f"{m}: top-1 {r[0]:.3f} of {int(live.sum())} live steps, {r[1]:.3f} of the {n_dec} decided by > 0.5, {r[2]:.3f} of those by > 1.0, "
        f"|d score| mean {r[3]:.3f} max {r[4]:.3f}" for m, r in res.items()))
    # measured (random-init weights, lm_head gain 6 -- logits far more sensitive than a trained model's): base 0.787 / 0.910 /
    # 0.974 with |d score| 0.42, large 0.758 / 0.843 / 0.899 with 0.56; the bf16 mode beside it 0.97 / 1.0 / 1.0 with 0.07.  The
    # gate holds the mode to what it delivers today, so that a regression (a mis-scaled block, a stale operand) shows
    mxr = res["mx8"]
    assert mxr[0] >= 0.70 and mxr[1] >= 0.80 and mxr[2] >= 0.85
    assert mxr[3] < 0.75 and mxr[4] < 4.0


def test_engines_own_their_decode_option_sets():
    """ABI 8: two engines in ONE process with different kernel variants (MhT5Config.options), interleaved with a third that
    follows the process-wide values -- every one reproduces the reference's greedy ids, an engine's override wins over
    mh_set_option, and the process-wide value is untouched by the sets."""
    import ctypes as C

    from mapperatorinator_amd import _lib
    from mapperatorinator_amd.modeling import MapperatorinatorHIP
    from mapperatorinator_amd.server import model_generate
    from mapperatorinator_amd.t5_engine import T5_PRESETS
    g, size, tok, sd, audio, src, tgt = golden_case("t5_tiny")
    lib = _lib.load()

    def make(options):
        return MapperatorinatorHIP(sd, T5_PRESETS[size], vocab_size_in=tok.vocab_size_in, vocab_size_out=tok.vocab_size_out,
                                   src_seq_len=src, tgt_seq_len=tgt, dtype=torch.float32, device="cuda", options=options)
    a = make(dict(decode_chains=1, decode_graph_cache=0))
    b = make(dict(decode_chains=3, decode_gemv_cols=4))
    plain = make(None)
    assert a.engine.options["decode_chains"] == 1 and b.engine.options["decode_chains"] == 3
    assert lib.mh_get_option(b"decode_chains") == 0 and plain.engine.options["decode_chains"] == 0
    assert lib.mh_t5_decode_chains_cfg(C.byref(a.engine.packed.cfg), 3) == 1
    assert lib.mh_t5_decode_chains_cfg(C.byref(b.engine.packed.cfg), 3) == 3
    with pytest.raises(RuntimeError, match="unknown option"):
        a.engine.options["no_such_option"] = 1
    prompt = torch.from_numpy(g["prompt"])
    mk = dict(inputs=audio, decoder_input_ids=prompt, decoder_attention_mask=prompt.ne(0))
    for m in (a, b, plain, b, a):
        ids, _ = model_generate(m, tok, mk, gen_kwargs(tgt))
        assert np.array_equal(ids.numpy(), g["ids"])
    old = _lib.set_option("decode_chains", 2)
    try:
        assert plain.engine.options["decode_chains"] == 2 and a.engine.options["decode_chains"] == 1
        assert lib.mh_t5_decode_chains_cfg(C.byref(plain.engine.packed.cfg), 3) == 2
        b.engine.options.clear("decode_chains")
        assert b.engine.options["decode_chains"] == 2 and b.engine.options["decode_gemv_cols"] == 4
        for m in (plain, a, b):
            ids, _ = model_generate(m, tok, mk, gen_kwargs(tgt))
            assert np.array_equal(ids.numpy(), g["ids"])
    finally:
        _lib.set_option("decode_chains", old)


def test_step_graphs_are_replayed_across_generate_calls():
    """Item "cache instantiated step graphs": a second mh_t5_generate whose description (addresses, sizes, sampling fields other
    than the seed, options, weights) is byte for byte the first one's replays the first one's graphs.  Greedy ids stay the
    golden ones; sampled runs with different seeds share the graphs (seed and rng_row0 travel through the device state block)
    and give exactly what an engine that captures per call gives for the same seeds."""
    import ctypes as C

    from mapperatorinator_amd import _lib
    from mapperatorinator_amd.modeling import MapperatorinatorHIP
    from mapperatorinator_amd.server import model_generate
    from mapperatorinator_amd.t5_engine import T5_PRESETS
    g, size, tok, sd, audio, src, tgt = golden_case("t5_small")
    lib = _lib.load()

    def make(options):
        return MapperatorinatorHIP(sd, T5_PRESETS[size], vocab_size_in=tok.vocab_size_in, vocab_size_out=tok.vocab_size_out,
                                   src_seq_len=src, tgt_seq_len=tgt, dtype=torch.float32, device="cuda", options=options)

    def stats(reset=0):
        h, m = C.c_long(0), C.c_long(0)
        lib.mh_t5_step_graph_cache_stats(C.byref(h), C.byref(m), reset)
        return h.value, m.value
    cached, percall = make(None), make(dict(decode_graph_cache=0))
    prompt = torch.from_numpy(g["prompt"])
    mk = dict(inputs=audio, decoder_input_ids=prompt, decoder_attention_mask=prompt.ne(0))
    stats(reset=1)
    n_chains = lib.mh_t5_decode_chains_cfg(C.byref(cached.engine.packed.cfg), prompt.shape[0])
    for _ in range(6):      # (a replay needs the caller's buffers at the same addresses: torch's caching allocator settles into
        ids, _ = model_generate(cached, tok, mk, gen_kwargs(tgt))     # a repeating pattern after a call or two)
        assert np.array_equal(ids.numpy(), g["ids"])
        if stats()[0] >= n_chains:
            break
    h, m = stats()
    print("step graphs: hits", h, "captures", m, "chains", n_chains)
    assert m >= n_chains and h >= n_chains, "the repeated call did not find its graphs"
    ids, _ = model_generate(percall, tok, mk, gen_kwargs(tgt))
    assert np.array_equal(ids.numpy(), g["ids"]) and stats() == (h, m)        # the per-call engine never touches the cache
    # sampling: three seeds on the cached engine (graphs shared between them) == the per-call engine on the same seeds
    outs = []
    for eng in (cached, percall):
        stats(reset=1)
        outs.append([model_generate(eng, tok, mk, gen_kwargs(tgt, do_sample=True, top_p=0.9, temperature=1.3, seed=100 + k,
                                                             seed_call_index=0))[0] for k in range(4)])
        if eng is cached:
            h2, m2 = stats()
            assert h2 >= n_chains, (h2, m2)          # at least one of the later seeds replayed the first one's graphs
    for x, y in zip(*outs):
        assert torch.equal(x, y)
    assert not torch.equal(outs[0][0], outs[0][1]), "different seeds must draw different tokens"


def test_a_step_graph_is_never_replayed_for_a_different_description():
    """Every input that is baked into a chain's step graph is part of the graph's cache key: a call `A'` that differs from a cached
    call `A` in ONE such input (top_k, temperature, the prompt mask, the e4m3 cross K/V copy, the e4m3 self-attention shadow, the
    row form of the sampler, the timing hook) gives bit for bit what an engine that captures per call (`decode_graph_cache=0`)
    gives for it, differs from `A`, and leaves `A`'s graph in place: the returning `A` replays it (one hit per chain -- the buffers
    sat at the same addresses, so a key without the varied input WOULD have replayed `A`'s graph for `A'`) with `A`'s result."""
    import ctypes as C

    from mapperatorinator_amd import _lib
    from mapperatorinator_amd.modeling import MapperatorinatorHIP
    from mapperatorinator_amd.server import build_row_sampling, build_sampling
    from mapperatorinator_amd.t5_engine import T5_PRESETS
    g, size, tok, sd, audio, src, tgt = golden_case("t5_tiny")
    lib = _lib.load()

    def make(options):
        return MapperatorinatorHIP(sd, T5_PRESETS[size], vocab_size_in=tok.vocab_size_in, vocab_size_out=tok.vocab_size_out,
                                   src_seq_len=src, tgt_seq_len=tgt, dtype=torch.bfloat16, device="cuda", options=options)

    def stats(reset=0):
        h, m = C.c_long(0), C.c_long(0)
        lib.mh_t5_step_graph_cache_stats(C.byref(h), C.byref(m), reset)
        return h.value, m.value
    cached, percall = make(None), make(dict(decode_graph_cache=0))
    prompt = torch.from_numpy(g["prompt"])          # rows 0 and 2 are left-padded
    B = prompt.shape[0]
    base = gen_kwargs(tgt, do_sample=True, top_p=0.9, temperature=1.3, seed=100, seed_call_index=0)

    def run(model, gk=base, mask=True, rows=None, **kw):
        """-> (ids, logits dump as int32 bit patterns on the CPU); nothing of the call stays allocated on the device"""
        if rows is not None:
            rs = build_row_sampling(tok, rows, tgt)
            sp, eos, kw = rs[0], None, dict(kw, row_sampling=rs)
        else:
            sp, eos = build_sampling(tok, gk, tgt)
        out = model.engine.generate(audio, prompt, prompt.ne(0) if mask else None, eos, sp, dump_logits=True, **kw)
        return out["tokens"], out["logits"].cpu().view(torch.int32)

    def same(x, y):
        return x[0].shape == y[0].shape and torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])
    n_chains = lib.mh_t5_decode_chains_cfg(C.byref(cached.engine.packed.cfg), B)
    # the buffers the variants keep (the shadow cache, the row settings, the stamps) exist before `A` settles, so that they do not
    # take the blocks `A`'s own per-call buffers return to
    ring, L = 8, T5_PRESETS[size].n_dec_layers
    tbuf = torch.zeros((n_chains, ring, L, 2), dtype=torch.int64, device="cuda")
    for m in (cached, percall):
        m.engine._workspace("skv8", lib.mh_t5_self_kv_fp8_bytes(C.byref(m.engine.packed.cfg), B))
        m.engine._workspace("row_sampling", 64 * C.sizeof(_lib.MhRowSampling))
        m.engine._workspace("row_eos_tables", 64 * tok.vocab_size_out)
    stats(reset=1)
    first = run(cached)
    for _ in range(5):      # (as in the test above: the allocator settles after a call or two)
        again = run(cached)
        assert same(again, first)
        if stats()[0] >= n_chains:
            break
    assert stats()[0] >= n_chains, "the repeated call did not find its graphs"

    def check(name, **variant):
        got = run(cached, **variant)
        h0, m0 = stats()
        back = run(cached)
        h1, m1 = stats()
        want = run(percall, **variant)
        assert stats() == (h1, m1)               # (the per-call engine never touches the cache)
        print(name, "ids differ from A:", not torch.equal(got[0], first[0]) if got[0].shape == first[0].shape else True,
              "dump differs:", got[1].shape != first[1].shape or not torch.equal(got[1], first[1]), "hits", h0, "->", h1)
        assert same(got, want), f"{name}: the cached engine and the per-call engine disagree"
        assert not same(got, first), f"{name}: the variant gives A's result -- the comparison has no teeth"
        assert same(back, first), f"{name}: A after the variant is not the first A"
        assert (h1 - h0, m1 - m0) == (n_chains, 0), f"{name}: the returning A did not replay its graphs ({h0, m0} -> {h1, m1})"
    check("top_k", gk=dict(base, top_k=5))
    check("temperature", gk=dict(base, temperature=0.7))
    check("prompt mask", mask=False)
    check("cross_kv_fp8", cross_kv_fp8=True)
    check("self_kv_fp8", self_kv_fp8=True)
    check("row form", rows=[dict(base, top_k=5)] + [base] * (B - 1))
    # the timing hook: its buffer is part of the description -- a call under the hook stamps, the next one without it must not
    tbuf[..., 0] = -1       # (= UINT64_MAX for the kernel's atomicMin)
    _lib.check(lib.mh_t5_decode_timing(tbuf.data_ptr(), ring), "mh_t5_decode_timing")
    try:
        timed = run(cached)
        torch.cuda.synchronize()
    finally:
        _lib.check(lib.mh_t5_decode_timing(None, 0), "mh_t5_decode_timing")
    t = tbuf.cpu()
    assert same(timed, first) and bool(((t[..., 1] != 0) & (t[..., 0] != -1)).any()), "the call under the hook wrote no stamps"
    tbuf.zero_()
    h0, m0 = stats()
    back = run(cached)
    torch.cuda.synchronize()
    assert same(back, first) and stats() == (h0 + n_chains, m0)
    assert not bool(tbuf.any()), "a call without the hook replayed a graph that stamps"


@pytest.mark.parametrize("beams,n_eos", [(2, 0), (2, 1), (3, 40), (2, 700), (5, 300), (8, 2)])
def test_beam_step_kernel_matches_torch_bookkeeping_across_candidate_counts(beams, n_eos):
    """mh_beam_step picks its K = max(2, 1 + #eos) x beams candidates with a radix select + a sort of the K only; the torch-op form
    (torch.topk over beams x V) is the same algorithm one ATen call at a time.  Same ids and same scores for K from 4 to ~1500, with
    EOS sets that end hypotheses at different steps and three ragged windows per call."""
    from mapperatorinator_amd import Tokenizer
    from mapperatorinator_amd.server import build_sampling
    from mapperatorinator_amd.t5_engine import T5_PRESETS
    from mh_testing import DIVERSE_GAINS, random_t5_state_dict, synthetic_audio_varied
    src, tgt = 64, 24
    tok = Tokenizer.benchmark_vocab(src_seq_len=src)
    sd = random_t5_state_dict(T5_PRESETS["tiny"], tok.vocab_size_in, tok.vocab_size_out, seed=3 + beams, lm_head_gain=6.0, gains=DIVERSE_GAINS)
    model = build("tiny", tok, sd, src, tgt, torch.float32)
    eng = model.engine
    audio = synthetic_audio_varied(3, (src - 1) * 128, seed=9).cuda()
    prompt = torch.tensor([[tok.sos_id, 0, 0], [tok.sos_id, 7, 0], [tok.sos_id, 9, 11]], dtype=torch.long)
    mask = prompt.ne(0)
    sp, _ = build_sampling(tok, gen_kwargs(tgt, num_beams=beams), tgt)
    gen = torch.Generator().manual_seed(n_eos)
    eos = sorted(set((torch.randperm(tok.vocab_size_out - 20, generator=gen)[:n_eos] + 20).tolist()))
    outs = [eng.generate_beam(audio, prompt, mask, eos, sp, beams, use_kernel=uk) for uk in (True, False)]
    assert torch.equal(outs[0]["tokens"], outs[1]["tokens"]), (outs[0]["tokens"].tolist(), outs[1]["tokens"].tolist())
    assert outs[0]["tokens"].shape[1] > prompt.shape[1]


def test_incremental_forward_with_past_key_values():
    """SURVEY B2's `forward(past_key_values=..., cache_position=...)` (modeling_mapperatorinator.py:186-228 pass both to the
    transformer; HF's generation loop calls the model this way): prompt in one call with `use_cache=True`, then one id per call with
    the returned cache -- the logits must be those of the teacher-forced full pass (step GEMVs against the prefill GEMMs: 5e-4), a
    plain greedy loop over the cached calls must return `generate`'s ids, and `reorder_cache` (cache_utils.py:16-20) must permute the
    rows."""
    from mapperatorinator_amd.modeling import HIPDecodeCache
    g, size, tok, sd, audio, src, tgt = t5_golden_case("t5_tiny")
    model = build(size, tok, sd, src, tgt, torch.float32)
    prompt = torch.from_numpy(g["prompt"])
    B, P = prompt.shape
    pmask = prompt.ne(0)
    kw = dict(decoder_input_ids=prompt, decoder_attention_mask=pmask, max_length=tgt, do_sample=False, eos_token_id=[])
    ids = model.generate(inputs=audio, **kw).cpu()                      # greedy, no processors, runs to max_length
    assert ids.shape == (B, tgt)
    full_mask = torch.cat([pmask, torch.ones(B, tgt - P, dtype=torch.bool)], 1)
    full = model(frames=audio, decoder_input_ids=ids, decoder_attention_mask=full_mask).logits.cpu()
    out = model(frames=audio, decoder_input_ids=prompt, decoder_attention_mask=pmask, use_cache=True)
    cache = out.past_key_values
    assert isinstance(cache, HIPDecodeCache) and cache.get_seq_length() == P and out.logits.shape == (B, P, tok.vocab_size_out)
    steps, cur = [out.logits.cpu()], prompt.clone()
    for t in range(P, tgt):
        nxt = steps[-1][:, -1].argmax(-1)
        assert torch.equal(nxt, ids[:, t]), t                            # the cached loop IS greedy decoding
        cur = torch.cat([cur, nxt[:, None]], 1)
        o = model(decoder_input_ids=nxt[:, None], decoder_attention_mask=full_mask[:, :t + 1], past_key_values=cache,
                  cache_position=torch.tensor([t]))
        assert o.past_key_values is cache and cache.get_seq_length() == t + 1
        steps.append(o.logits.cpu())
    inc = torch.cat(steps, 1)
    assert inc.shape == full.shape
    real = full_mask[:, :, None].expand_as(full)                         # (a padded position's own logits are not defined)
    assert float((inc - full)[real].abs().max()) < 5e-4
    with pytest.raises(ValueError, match="cache_position"):
        model(decoder_input_ids=ids[:, :1], past_key_values=cache, cache_position=torch.tensor([3]))
    with pytest.raises(ValueError, match="exceed the cache"):
        model(decoder_input_ids=ids[:, :1], past_key_values=cache)
    # reorder: a second cache over the prompt, rows permuted, then the same next id per (moved) row
    perm = torch.tensor([(i + 1) % B for i in range(B)])
    c2 = model(frames=audio, decoder_input_ids=prompt, decoder_attention_mask=pmask, use_cache=True).past_key_values
    c2.reorder_cache(perm)
    o2 = model(decoder_input_ids=ids[perm, P:P + 1], past_key_values=c2)
    assert torch.equal(o2.logits.cpu()[:, 0], steps[1][perm, 0])
