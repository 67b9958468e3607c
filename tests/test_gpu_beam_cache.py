"""-m gpu: beam search over an indexed self-attention cache (`beam_cache="indexed"`: mh_t5_step_indexed + mh_t5_reorder_index) and
the prompt prefilled once per chunk (`beam_prefill=True`: mh_t5_step_prefill).

Contract: the indexed route reads, for every decode row and position, the very cache row the copy route would have copied there, and
keeps every sum in the order of the decode row -- so its logits are BIT-identical to mh_t5_step + mh_t5_reorder_cache under any
sequence of reorders, and every search built on it returns the same ids.  The prefill writes the cache rows mh_t5_generate's prefill
writes (bit for bit); against the token-by-token feed it is held to the project's 5e-4 bound on fp32 step logits."""
import ctypes as C
import functools
import json

import numpy as np
import pytest
import torch

from conftest import GOLDEN, types_first_case

pytestmark = pytest.mark.gpu

TGT, N_POS, FRAMES = 320, 300, 514


def gen_kwargs(tgt, **over):
    kw = dict(precision="fp32", do_sample=False, num_beams=1, top_p=1.0, top_k=0, max_length=tgt, cfg_scale=1.0, timeshift_bias=0,
              types_first=False, temperature=1.0, lookback_time=0, lookahead_time=0, context_type="map", pad_token_id=0)
    kw.update(over)
    return kw


@functools.lru_cache(maxsize=None)
def family(kind, dtype, tgt=TGT):
    """(tokenizer, model) at `test` dims (d_model 128, 2 heads, 2 decoder layers): "t5", "var" (VarWhisper, layer 1 local with a
    32-key window), "hf" (HF Whisper: LayerNorm prologues, decoder positions from the prompt mask)."""
    from mapperatorinator_amd import Tokenizer
    from mapperatorinator_amd.modeling import MapperatorinatorHIP
    from mapperatorinator_amd.t5_engine import T5_PRESETS
    from mapperatorinator_amd.whisper_engine import VARWHISPER_PRESETS
    from mh_testing import DIVERSE_GAINS, random_t5_state_dict, random_varwhisper_state_dict, random_whisper_family_state_dict
    if kind == "t5":
        tok = Tokenizer.benchmark_vocab(src_seq_len=64)
        d = T5_PRESETS["tiny"]
        sd = random_t5_state_dict(d, tok.vocab_size_in, tok.vocab_size_out, seed=5, lm_head_gain=4.0, gains=DIVERSE_GAINS)
        return tok, MapperatorinatorHIP(sd, d, vocab_size_in=tok.vocab_size_in, vocab_size_out=tok.vocab_size_out, src_seq_len=64,
                                        tgt_seq_len=tgt, dtype=dtype, device="cuda")
    tok = Tokenizer.benchmark_vocab(src_seq_len=FRAMES)
    d = VARWHISPER_PRESETS["test"]
    if kind == "var":
        sd = random_varwhisper_state_dict(d.d_model, d.n_heads, d.n_enc_layers, d.n_dec_layers, d.d_ff, tok.vocab_size_in,
                                          tok.vocab_size_out, seed=77, head_gain=5.0, gains={"decoder_embedder": 0.5})
        opts, n_mels = dict(global_attn_every_n_layers=2, local_attention=64), 128
    else:
        sd = random_whisper_family_state_dict("hf", d.d_model, d.n_heads, d.n_enc_layers, d.n_dec_layers, d.d_ff, tok.vocab_size_in,
                                              tok.vocab_size_out, 388, src_positions=FRAMES // 2, tgt_positions=tgt, seed=77,
                                              head_gain=5.0, gains={"decoder_embedder": 0.5})
        opts, n_mels = dict(decoder_positions="mask"), 388
    model = MapperatorinatorHIP(sd, d, vocab_size_in=tok.vocab_size_in, vocab_size_out=tok.vocab_size_out, n_mels=n_mels,
                                src_seq_len=FRAMES, tgt_seq_len=tgt, dtype=dtype, device="cuda", f_min=0 if kind == "hf" else 20,
                                backbone_options=opts)
    cfg = model.engine.packed.cfg
    if kind == "var":
        assert cfg.arch == 1 and cfg.local_every == 2 and 0 < cfg.local_window < N_POS     # a window shorter than the run
    else:
        assert cfg.arch == 2 and cfg.dec_pos_from_mask == 1
    return tok, model


def random_kv(eng, rows, seed):
    """a cross K/V tensor of `rows` chunks in the engine's layout and storage type (the step tests need no encoder)"""
    cfg = eng.packed.cfg
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(cfg.n_dec_layers, 2, rows, cfg.n_heads, cfg.src_len, 64, generator=g) * 0.5).to(eng.device, eng.dtype).contiguous()


def fixed_reorders(n_pos, G, nb, seed, double):
    """src per step, int32 (n_pos, rows): within each chunk a pseudo-random choice of beams, repeats included; the identity on every
    fourth step.  `double` (guidance): both halves carry the first half's indices (`beam_idx.repeat(2)`)."""
    g = torch.Generator().manual_seed(seed)
    pick = torch.randint(0, nb, (n_pos, G, nb), generator=g)
    pick[::4] = torch.arange(nb)
    src = (pick + torch.arange(G).view(1, G, 1) * nb).reshape(n_pos, G * nb)
    R = G * nb
    permuting = int((src != torch.arange(R)).any(dim=1).sum())
    assert 3 * permuting >= n_pos, (permuting, n_pos)                     # otherwise the run shows nothing
    assert int((src.sort(dim=1).values[:, 1:] == src.sort(dim=1).values[:, :-1]).any(dim=1).sum()) > n_pos // 4   # repeats
    if double:
        src = torch.cat([src, src], 1)
    return src.to(torch.int32).contiguous()


def run_steps(eng, kv, kv8, ids, mask, P, srcs, nb, indexed):
    """n_pos steps over all rows, a reorder after every step.  -> logits (n_pos, rows, V) on the CPU"""
    from mapperatorinator_amd import _lib
    lib, p = eng.lib, eng.packed
    n_pos, R = ids.shape
    cfg, w, V = C.byref(p.cfg), C.byref(p.w), p.vocab_out
    eng._enter()
    with eng.on_stream():
        s = eng._s()
        ids_d, srcs_d = ids.to(eng.device, torch.int32).contiguous(), srcs.to(eng.device)
        mask_d = None if mask is None else mask.to(eng.device, torch.uint8).contiguous()
        ws = torch.zeros(int(lib.mh_t5_decode_workspace_bytes(cfg, R)), dtype=torch.uint8, device=eng.device)
        out = torch.empty((n_pos, R, V), dtype=torch.float32, device=eng.device)
        if indexed:
            tabs = [torch.full((int(lib.mh_t5_beam_index_bytes(cfg, R)),), 255, dtype=torch.uint8, device=eng.device) for _ in range(2)]
            _lib.check(lib.mh_t5_beam_index_init(cfg, R, nb, 0, tabs[0].data_ptr(), s), "mh_t5_beam_index_init")
        else:
            scratch = torch.empty(int(lib.mh_t5_reorder_cache_scratch_bytes(cfg, R, n_pos)), dtype=torch.uint8, device=eng.device)
        for pos in range(n_pos):
            common = (R, nb, ids_d[pos].data_ptr(), pos, _lib.ptr(mask_d), P, out[pos].data_ptr(), ws.data_ptr(), ws.numel())
            if indexed:
                rc = lib.mh_t5_step_indexed(cfg, w, kv.data_ptr(), _lib.ptr(kv8), *common, tabs[pos & 1].data_ptr(), s)
                _lib.check(rc, "mh_t5_step_indexed")
                rc = lib.mh_t5_reorder_index(cfg, R, srcs_d[pos].data_ptr(), pos + 1, tabs[pos & 1].data_ptr(), tabs[(pos & 1) ^ 1].data_ptr(), s)
                _lib.check(rc, "mh_t5_reorder_index")
            else:
                if kv8 is None:
                    rc = lib.mh_t5_step(cfg, w, kv.data_ptr(), *common, s)
                else:
                    rc = lib.mh_t5_step_fp8(cfg, w, kv.data_ptr(), kv8.data_ptr(), *common, s)
                _lib.check(rc, "mh_t5_step")
                rc = lib.mh_t5_reorder_cache(cfg, R, srcs_d[pos].data_ptr(), pos + 1, ws.data_ptr(), ws.numel(), scratch.data_ptr(),
                                             scratch.numel(), s)
                _lib.check(rc, "mh_t5_reorder_cache")
    eng._leave()
    eng.synchronize()
    return out.cpu()


def assert_same_logits(a, b, what):
    assert torch.isfinite(a).all(), what
    if not torch.equal(a, b):
        bad = (a != b).flatten(1).any(dim=1).nonzero().flatten()
        raise AssertionError(f"{what}: logits differ from step {int(bad[0])} on ({bad.numel()} of {a.shape[0]} steps), "
                             f"max |d| {(a - b).abs().max().item():.3e}")


def step_case(kind, dtype, nb, guided=False, fp8=False):
    tok, model = family(kind, dtype)
    eng = model.engine
    G, P = 2, 8
    R = G * nb * (2 if guided else 1)
    g = torch.Generator().manual_seed(100 + nb)
    ids = torch.randint(3, tok.vocab_size_out, (N_POS, R), generator=g)
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
    srcs = fixed_reorders(N_POS, G, nb, seed=7 + nb, double=guided)
    copy = run_steps(eng, kv, kv8, ids, mask, P, srcs, nb, indexed=False)
    indexed = run_steps(eng, kv, kv8, ids, mask, P, srcs, nb, indexed=True)
    assert_same_logits(copy, indexed, f"{kind} {dtype} {G} x {nb}{' guided' if guided else ''}{' e4m3 cross' if fp8 else ''}")
    # the reorders mattered: without them (identity tables throughout) the logits are others
    return copy


@pytest.mark.parametrize("nb", [2, 3])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["t5", "var", "hf"])
def test_step_logits_equal_the_copy_route_under_hand_made_reorders(kind, dtype, nb):
    """1. 300 positions (the key loop's 128- and 256-key trips and a ragged tail), 2 chunks x 2 / 3 beams, a reorder after every step."""
    step_case(kind, dtype, nb)


def test_step_logits_equal_the_copy_route_over_the_e4m3_cross_copy():
    """1. ... one case with the e4m3 cross copy on both sides (mh_t5_step_fp8 against mh_t5_step_indexed with the copy)."""
    step_case("var", torch.bfloat16, 2, fp8=True)


def test_the_reorders_change_the_logits():
    """The hand-made reorders are not a no-op for the model: the same ids WITHOUT reorders give other logits from early on (so the
    equalities above compare caches that really were permuted)."""
    tok, model = family("t5", torch.float32)
    eng, nb, G, P = model.engine, 2, 2, 8
    ids = torch.randint(3, tok.vocab_size_out, (40, G * nb), generator=torch.Generator().manual_seed(102))
    kv = random_kv(eng, G, seed=3)
    srcs = fixed_reorders(40, G, nb, seed=9, double=False)
    ident = torch.arange(G * nb, dtype=torch.int32).repeat(40, 1)
    a = run_steps(eng, kv, None, ids, None, P, srcs, nb, indexed=True)
    b = run_steps(eng, kv, None, ids, None, P, ident, nb, indexed=True)
    assert not torch.equal(a, b) and torch.equal(a[0], b[0])


@pytest.mark.parametrize("kind,dtype", [("t5", torch.float32), ("var", torch.bfloat16)], ids=["t5-fp32", "var-bf16"])
def test_guidance_rows_follow_the_first_half(kind, dtype):
    """2. doubled rows, `src` of the second half pointing into the first (`beam_idx.repeat(2)`): equal logits."""
    step_case(kind, dtype, 2, guided=True)


# ---- end to end ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def golden_case():
    """the inputs of tests/golden/t5_tiny_beam.npz (test_fp32_beam_search_matches_reference_golden) on the device"""
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
                                src_seq_len=src, tgt_seq_len=tgt, dtype=torch.float32, device="cuda")
    return g, tok, model, audio, tgt


def golden_inputs(g, audio, guided):
    prompt = torch.from_numpy(g["prompt"])
    mk = dict(inputs=audio, decoder_input_ids=prompt, decoder_attention_mask=prompt.ne(0))
    if guided:
        neg = torch.from_numpy(g["negative"])
        mk.update(negative_prompt=neg, negative_prompt_attention_mask=neg.ne(0))
    return mk


def count_calls(monkeypatch, lib):
    """counts per entry, and the `src` of every index reorder (read back: a test-only synchronisation)"""
    from mapperatorinator_amd import beam as _beam
    calls = dict(mh_t5_step=0, mh_t5_step_fp8=0, mh_t5_reorder_cache=0, mh_t5_step_indexed=0, mh_t5_reorder_index=0, mh_t5_step_prefill=0,
                 mh_t5_reorder_cache_scratch_bytes=0, permuting=0)
    for name in list(calls)[:-1]:
        def counted(*a, _f=getattr(lib, name), _n=name):
            calls[_n] += 1
            return _f(*a)
        monkeypatch.setattr(lib, name, counted)
    real = _beam._IndexedCache.reorder

    def reorder(self, src, n_pos):
        calls["permuting"] += int(not torch.equal(src.cpu(), torch.arange(src.numel(), dtype=src.dtype)))
        return real(self, src, n_pos)
    monkeypatch.setattr(_beam._IndexedCache, "reorder", reorder)
    return calls


@pytest.mark.parametrize("guided", [False, True], ids=["plain", "guided"])
@pytest.mark.parametrize("use_kernel", [True, False], ids=["kernel", "torch"])
@pytest.mark.parametrize("nb", [2, 4])
def test_model_generate_returns_the_default_routes_ids(monkeypatch, nb, use_kernel, guided):
    """3. `model_generate(num_beams, beam_cache="indexed")` against the default route, through the beam kernel and the torch-op
    bookkeeping, with and without guidance; the indexed entries ran, the copy's did not, and the search did reorder."""
    from mapperatorinator_amd import _lib
    from mapperatorinator_amd.server import model_generate
    g, tok, model, audio, tgt = golden_case()
    mk = golden_inputs(g, audio, guided)
    gk = gen_kwargs(tgt, num_beams=nb, beam_use_kernel=use_kernel, temperature=1.2, **(dict(cfg_scale=2.0) if guided else {}))
    want, _ = model_generate(model, tok, mk, gk)
    calls = count_calls(monkeypatch, _lib.load())
    got, _ = model_generate(model, tok, mk, dict(gk, beam_cache="indexed"))
    assert torch.equal(got, want), (got.tolist(), want.tolist())
    n_new = got.shape[1] - mk["decoder_input_ids"].shape[1]
    assert n_new > 0 and calls["mh_t5_step_indexed"] >= n_new and calls["mh_t5_reorder_index"] >= n_new
    assert calls["mh_t5_step"] == calls["mh_t5_step_fp8"] == calls["mh_t5_reorder_cache"] == calls["mh_t5_reorder_cache_scratch_bytes"] == 0
    assert calls["permuting"] >= 1, "the search never reordered: the comparison shows nothing"


@pytest.mark.parametrize("run", ["tb3", "tb2g", "tb2"])
def test_types_first_search_returns_the_goldens_ids(monkeypatch, run):
    """3. ... with the types_first lookback (mh_beam_step_tf: `lookback_prev` stays by row slot whatever the cache does)."""
    from mapperatorinator_amd import _lib
    from mapperatorinator_amd.modeling import MapperatorinatorHIP
    from mapperatorinator_amd.server import model_generate
    from mapperatorinator_amd.t5_engine import T5_PRESETS
    tf, tok, sd, audio, tgt, _ = types_first_case()
    g = np.load(f"{GOLDEN}/t5_tiny_tf_beam.npz")
    model = MapperatorinatorHIP(sd, T5_PRESETS["tiny"], vocab_size_in=tok.vocab_size_in, vocab_size_out=tok.vocab_size_out,
                                src_seq_len=int(tf["src"]), tgt_seq_len=tgt, dtype=torch.float32, device="cuda")
    kw = json.loads(str(g["runs"]))[run]
    mk = golden_inputs(g, audio, kw.get("cfg_scale", 1.0) > 1.0)
    calls = count_calls(monkeypatch, _lib.load())
    for use_kernel in (True, False):
        ids, _ = model_generate(model, tok, mk, gen_kwargs(tgt, beam_use_kernel=use_kernel, beam_cache="indexed", **kw))
        assert np.array_equal(ids.numpy(), g["ids_" + run]), (use_kernel, ids.tolist())
    assert calls["mh_t5_step_indexed"] > 0 and calls["mh_t5_step"] == calls["mh_t5_reorder_cache"] == 0 and calls["permuting"] >= 1


@pytest.mark.parametrize("use_kernel", [True, False], ids=["kernel", "torch"])
def test_beam_sample_in_the_step_kernel_under_a_fixed_seed(monkeypatch, use_kernel):
    """3. ... with `beam_sample_kernel=True`: the draw depends on the seed and the scores alone, so both caches give the same ids."""
    from mapperatorinator_amd import _lib
    from mapperatorinator_amd.server import model_generate
    g, tok, model, audio, tgt = golden_case()
    mk = golden_inputs(g, audio, False)
    gk = gen_kwargs(tgt, num_beams=3, do_sample=True, top_k=40, top_p=0.95, temperature=1.1, seed=1234, seed_call_index=0,
                    beam_sample_kernel=True, beam_use_kernel=use_kernel)      # (seed_call_index: the same seed for every call)
    want, _ = model_generate(model, tok, mk, gk)
    calls = count_calls(monkeypatch, _lib.load())
    got, _ = model_generate(model, tok, mk, dict(gk, beam_cache="indexed"))
    assert torch.equal(got, want), (got.tolist(), want.tolist())
    assert calls["mh_t5_step_indexed"] > 0 and calls["mh_t5_step"] == 0 and calls["permuting"] >= 1


@pytest.mark.parametrize("prefill", [False, True], ids=["indexed", "indexed+prefill"])
@pytest.mark.parametrize("run", ["b2", "b3", "b2p", "b3p", "b2g", "b3g", "b2s", "b3s", "b2sg"])
def test_fp32_reference_goldens(monkeypatch, run, prefill):
    """4. the reference's ids of tests/golden/t5_tiny_beam.npz with `beam_cache="indexed"`, and again with `beam_prefill=True`."""
    from mapperatorinator_amd import _lib
    from mapperatorinator_amd.server import model_generate
    from mh_testing import SeededMultinomial
    g, tok, model, audio, tgt = golden_case()
    kw = json.loads(str(g["runs"]))[run]
    mk = golden_inputs(g, audio, kw.get("cfg_scale", 1.0) > 1.0)
    sampler = SeededMultinomial(json.loads(str(g["sample_seeds"]))[run]) if kw.get("do_sample") else None
    calls = count_calls(monkeypatch, _lib.load())
    ids, _ = model_generate(model, tok, mk, gen_kwargs(tgt, beam_cache="indexed", beam_prefill=prefill, **kw,
                                                       **({"beam_sample_fn": sampler} if sampler else {})))
    want = g["ids_" + run]
    assert ids.shape == want.shape and np.array_equal(ids.numpy(), want), (ids.tolist(), want.tolist())
    assert calls["mh_t5_step"] == calls["mh_t5_reorder_cache"] == 0 and calls["mh_t5_step_indexed"] > 0
    P = mk["decoder_input_ids"].shape[1]
    assert calls["mh_t5_step_prefill"] == (1 if prefill and P > 1 else 0)
    n_search = calls["mh_t5_reorder_index"]
    assert calls["mh_t5_step_indexed"] == n_search + (0 if prefill else P - 1)


# ---- prefill ---------------------------------------------------------------------------------------------------------------------

def prefill_case(kind, dtype, G, nb, P, seed):
    tok, model = family(kind, dtype)
    eng = model.engine
    g = torch.Generator().manual_seed(seed)
    prompt = torch.randint(3, tok.vocab_size_out, (G, P), generator=g)
    mask = torch.ones(G, P, dtype=torch.uint8)
    for r in range(G):                                                     # ragged left padding: row r pads 2 r + 1 columns
        mask[r, :2 * r + 1] = 0
        prompt[r, :2 * r + 1] = 0
    return tok, eng, prompt.to(eng.device, torch.int32).contiguous(), mask.to(eng.device).contiguous(), random_kv(eng, G, seed=seed + 1)


def step_caches(eng, ws, R):
    from mapperatorinator_amd import _lib
    p = eng.packed
    k, v = C.c_void_p(), C.c_void_p()
    _lib.check(eng.lib.mh_t5_decode_self_cache(C.byref(p.cfg), R, ws.data_ptr(), C.byref(k), C.byref(v)), "mh_t5_decode_self_cache")
    shape = (p.cfg.n_dec_layers, R, p.cfg.n_heads, p.tgt_len, 64)
    n = int(np.prod(shape)) * torch.empty(0, dtype=eng.dtype).element_size()
    return [ws[ptr - ws.data_ptr(): ptr - ws.data_ptr() + n].view(eng.dtype).view(shape) for ptr in (k.value, v.value)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["t5", "var", "hf"])
def test_prefill_writes_the_cache_rows_of_mh_t5_generate(kind, dtype):
    """5. mh_t5_step_prefill into rows 0 .. G-1 of a (G x beams)-row workspace against the rows mh_t5_generate's prefill leaves in its
    G-row workspace, for the same prompts under a ragged left-padded mask: bit-equal."""
    from mapperatorinator_amd import _lib
    from mapperatorinator_amd.server import build_sampling
    G, nb, P = 3, 2, 21
    tok, eng, prompt, mask, kv = prefill_case(kind, dtype, G, nb, P, seed=31)
    lib, p, R = eng.lib, eng.packed, G * nb
    sp, _ = build_sampling(tok, gen_kwargs(P + 1), TGT)
    eos_table = torch.zeros(tok.vocab_size_out, dtype=torch.uint8, device=eng.device)
    eng._enter()
    with eng.on_stream():
        eng.decode(kv, prompt, mask, eos_table, sp)                        # prefill of positions 0 .. P-2, then one token step at P-1
        eng.synchronize()
        want = [c[:, :, :, :P - 1].clone() for c in eng.self_kv_caches(G)]
        ws = torch.zeros(int(lib.mh_t5_decode_workspace_bytes(C.byref(p.cfg), R)), dtype=torch.uint8, device=eng.device)
        rc = lib.mh_t5_step_prefill(C.byref(p.cfg), C.byref(p.w), kv.data_ptr(), G, prompt.data_ptr(), mask.data_ptr(), P, P - 1,
                                    ws.data_ptr(), ws.numel(), R, eng._s())
        _lib.check(rc, "mh_t5_step_prefill")
        eng.synchronize()
        got = step_caches(eng, ws, R)
    eng._leave()
    for name, a, b in zip("kv", got, want):
        assert a.shape[1] == R and b.shape[1] == G
        assert b.float().abs().sum() > 0
        assert torch.equal(a[:, :G, :, :P - 1], b), f"{name} cache rows differ"
        assert not a[:, G:].any() and not a[:, :G, :, P - 1:].any()        # nothing else was written


def test_fp32_logits_after_a_prefilled_prompt_agree_with_the_token_by_token_feed():
    """5. fp32, a 40-token prompt, 2 chunks x 2 beams: the step at position 39 after mh_t5_step_prefill(0 .. 38) against the same step
    after 39 single steps, within 5e-4 (the project's bound for the best scores of a step).  Max |d| is printed."""
    from mapperatorinator_amd import _lib
    G, nb, P = 2, 2, 40
    tok, eng, prompt, mask, kv = prefill_case("var", torch.float32, G, nb, P, seed=41)
    lib, p, R, V = eng.lib, eng.packed, G * nb, tok.vocab_size_out
    cfg, w = C.byref(p.cfg), C.byref(p.w)
    ids = prompt.repeat_interleave(nb, 0).t().contiguous()                 # (P, R)
    mask_r = mask.repeat_interleave(nb, 0).contiguous()
    outs = []
    eng._enter()
    with eng.on_stream():
        s = eng._s()
        for prefilled in (False, True):
            ws = torch.zeros(int(lib.mh_t5_decode_workspace_bytes(cfg, R)), dtype=torch.uint8, device=eng.device)
            tab = torch.empty(int(lib.mh_t5_beam_index_bytes(cfg, R)), dtype=torch.uint8, device=eng.device)
            logits = torch.empty((R, V), dtype=torch.float32, device=eng.device)
            first = 0
            if prefilled:
                _lib.check(lib.mh_t5_step_prefill(cfg, w, kv.data_ptr(), G, prompt.data_ptr(), mask.data_ptr(), P, P - 1, ws.data_ptr(),
                                                  ws.numel(), R, s), "mh_t5_step_prefill")
                first = P - 1
            _lib.check(lib.mh_t5_beam_index_init(cfg, R, nb, first, tab.data_ptr(), s), "mh_t5_beam_index_init")
            for pos in range(first, P):
                _lib.check(lib.mh_t5_step_indexed(cfg, w, kv.data_ptr(), None, R, nb, ids[pos].data_ptr(), pos, mask_r.data_ptr(), P,
                                                  logits.data_ptr(), ws.data_ptr(), ws.numel(), tab.data_ptr(), s), "mh_t5_step_indexed")
            eng.synchronize()
            outs.append(logits.cpu())
    eng._leave()
    d = (outs[0] - outs[1]).abs().max().item()
    print(f"fp32 step logits after a prefilled 40-token prompt vs the token-by-token feed: max |d| {d:.3e}")
    assert torch.isfinite(outs[0]).all() and outs[0].abs().max() > 1.0
    assert d < 5e-4


def test_scheduler_equals_the_windows_decoded_one_by_one():
    """6. a three-window song, num_beams = 2, indexed cache + prefill: every window as generate_beam returns it for that window alone."""
    from mapperatorinator_amd.scheduler import SequentialWindowScheduler, SongJob
    from mapperatorinator_amd.server import build_sampling
    from mh_testing import synthetic_audio_varied
    tgt, n = 40, 3
    tok, model = family("var", torch.float32, tgt)
    eng = model.engine
    song = synthetic_audio_varied(n, (FRAMES - 1) * 128, seed=8)
    gk = gen_kwargs(tgt, num_beams=2, beam_cache="indexed", beam_prefill=True)

    def prompt_from(prev):
        carry = [] if prev is None else [t for t in prev.tolist() if t > 2][-3:]
        return torch.tensor([[tok.sos_id] + carry])

    def cut(row, P, eos):
        hit = torch.isin(row[P:], torch.tensor(sorted(eos))).nonzero()
        return row[:P + int(hit[0]) + 1] if hit.numel() else row
    want, prev, prompt_lens = [], None, []
    for w in range(n):
        prompt = prompt_from(prev)
        prompt_lens.append(prompt.shape[1])
        sp, eos = build_sampling(tok, dict(gk, conditional_temperature_per_row=True), tgt)
        out = eng.generate_beam(song[w:w + 1], prompt, None, eos, sp, 2, beam_cache="indexed", beam_prefill=True)
        row = cut(out["tokens"][0], prompt.shape[1], eos)
        prev = row[prompt.shape[1]:]
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
    assert len(want[0]) > 2 and max(prompt_lens) > 1                       # a later window had a prompt to prefill
