"""-m gpu: beam search under LookbackBiasLogitsWarper(types_first=True) on the HIP path -- mh_beam_step_tf (csrc/beam.hip), both of
its kernels, and the torch-op bookkeeping of mapperatorinator_amd/beam.py.

fp32 storage, tiny dims, tgt 48, three ragged rows (oracle/make_golden.py:TF_CASE).  The reference side is
tests/golden/t5_tiny_tf_beam.npz (tools/make_beam_tf_golden.py): ids of the reference's `model_generate` through HF beam search; every
decision of those runs is wider than 1e-3, twice what a processed score may differ by here (5e-4), so the ids are compared bit for
bit.  The warper's state is kept by ROW SLOT (see tests/test_beam_types_first_cpu.py)."""
import json

import numpy as np
import pytest
import torch

from conftest import GOLDEN, types_first_case

pytestmark = pytest.mark.gpu


def gen_kwargs(tgt, **over):
    kw = dict(precision="fp32", do_sample=False, num_beams=1, top_p=1.0, top_k=0, max_length=tgt, cfg_scale=1.0, timeshift_bias=0,
              types_first=False, temperature=1.0, lookback_time=0, lookahead_time=0, context_type="map", pad_token_id=0)
    kw.update(over)
    return kw


@pytest.fixture
def step_path():
    """Sets the library option "beam_step_path" for the test and puts the old value back."""
    from mapperatorinator_amd import _lib
    lib = _lib.load()
    old = lib.mh_get_option(b"beam_step_path")

    def choose(path):
        assert lib.mh_set_option(b"beam_step_path", path) == 0
    yield choose
    assert lib.mh_set_option(b"beam_step_path", old) == 0


_CASE = {}


def tf_model():
    """The TF_CASE model on the device, built once for the module: (golden of t5_tiny_tf, tok, model, audio, tgt)."""
    if not _CASE:
        from mapperatorinator_amd.modeling import MapperatorinatorHIP
        from mapperatorinator_amd.t5_engine import T5_PRESETS
        g, tok, sd, audio, tgt, _ = types_first_case()
        model = MapperatorinatorHIP(sd, T5_PRESETS["tiny"], vocab_size_in=tok.vocab_size_in, vocab_size_out=tok.vocab_size_out,
                                    src_seq_len=int(g["src"]), tgt_seq_len=tgt, dtype=torch.float32, device="cuda")
        _CASE["v"] = (g, tok, model, audio, tgt)
    return _CASE["v"]


def count_kernel_calls(monkeypatch):
    from mapperatorinator_amd import beam as _beam
    calls, orig = [], _beam._beam_search_kernel
    monkeypatch.setattr(_beam, "_beam_search_kernel", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    return calls


@pytest.mark.parametrize("run", ["tb3", "tb2g", "tb2"])
def test_fp32_beams_with_types_first_lookback_match_reference_golden(run, step_path, monkeypatch):
    """3 beams with every processor but guidance, 2 beams under guidance, 2 beams whose ids depend on the warper in 35 positions: the
    reference's ids bit for bit through the LDS kernel, the streaming kernel and the torch-op bookkeeping."""
    from mapperatorinator_amd.server import model_generate
    tf, tok, model, audio, tgt = tf_model()
    g = np.load(f"{GOLDEN}/t5_tiny_tf_beam.npz")
    assert np.array_equal(g["prompt"], tf["prompt"]) and int(g["weight_seed"]) == int(tf["weight_seed"]) and int(g["tgt"]) == tgt
    kw = json.loads(str(g["runs"]))[run]
    prompt, neg = torch.from_numpy(g["prompt"]), torch.from_numpy(g["negative"])
    mk = dict(inputs=audio, decoder_input_ids=prompt, decoder_attention_mask=prompt.ne(0))
    if kw.get("cfg_scale", 1.0) > 1.0:
        mk.update(negative_prompt=neg, negative_prompt_attention_mask=neg.ne(0))
    want = g["ids_" + run]
    calls = count_kernel_calls(monkeypatch)
    for path, use_kernel in ((0, None), (2, True), (0, False)):
        step_path(path)
        ids, stats = model_generate(model, tok, mk, gen_kwargs(tgt, beam_use_kernel=use_kernel, **kw))
        where = f"beam_step_path {path}, use_kernel {use_kernel}"
        assert ids.shape == want.shape and np.array_equal(ids.numpy(), want), (where, np.argwhere(ids.numpy() != want)[:3])
    assert len(calls) == 2                                    # the default route IS the kernel


@pytest.mark.parametrize("beams,n_eos", [(2, 1), (2, 700), (8, 2), (8, 600)])
def test_beam_step_tf_matches_torch_bookkeeping_across_candidate_counts(beams, n_eos, step_path):
    """K = max(2, 1 + #eos) x beams from 4 to 4808 (beyond 4096 candidates only the streaming kernel runs) with EOS sets that end
    hypotheses at different steps: the call's EOS table and the warper's own eos ids (bit 4 of tok_flags) are different sets here.
    Lookback end inside the TIME_SHIFT range, conditional temperatures on.  Same tokens from the kernel and from the torch ops."""
    from mapperatorinator_amd import _lib
    from mapperatorinator_amd.server import build_sampling
    _, tok, model, audio, tgt = tf_model()
    prompt = torch.from_numpy(tf_model()[0]["prompt"])
    sp, _ = build_sampling(tok, gen_kwargs(tgt, num_beams=beams, types_first=True, temperature=1.1, timing_temperature=0.8,
                                           mania_column_temperature=0.8, taiko_hit_temperature=0.5, lookback_time=500), tgt)
    assert sp.lookback_types_first and sp.ts_start < sp.lookback_mask_end < sp.ts_end
    gen = torch.Generator().manual_seed(n_eos)
    eos = sorted(set((torch.randperm(tok.vocab_size_out - 20, generator=gen)[:n_eos] + 20).tolist()))
    K = max(2, 1 + len(eos)) * beams
    step_path(0)
    assert _lib.load().mh_beam_step_path(beams, tok.vocab_size_out, K) == (2 if K > 4096 else 1)
    outs = [model.engine.generate_beam(audio.cuda(), prompt, prompt.ne(0), eos, sp, beams, use_kernel=uk) for uk in (True, False)]
    assert torch.equal(outs[0]["tokens"], outs[1]["tokens"]), (outs[0]["tokens"].tolist(), outs[1]["tokens"].tolist())
    assert outs[0]["tokens"].shape[1] > prompt.shape[1]
    if K <= 4096:                                             # the streaming kernel on a shape the LDS kernel took: same tokens
        step_path(2)
        again = model.engine.generate_beam(audio.cuda(), prompt, prompt.ne(0), eos, sp, beams, use_kernel=True)
        assert torch.equal(again["tokens"], outs[0]["tokens"])


def test_hf_whisper_backbone_with_the_types_first_tokenizer(step_path, monkeypatch):
    """The released V29 combination: 'openai/whisper' wiring (arch 2 decoder kernels), types_first tokenizer, lookback > 0, 2 beams."""
    from mapperatorinator_amd.modeling import MapperatorinatorHIP
    from mapperatorinator_amd.server import FLAG_TIMED, TIMED_EVENT_NAMES, _ev, _has, build_sampling, model_generate
    from mapperatorinator_amd.whisper_engine import VARWHISPER_PRESETS
    from mh_testing import random_whisper_family_state_dict, synthetic_audio_varied
    _, tok, _, _, _ = tf_model()
    d, frames, tgt, n_mels = VARWHISPER_PRESETS["test"], 250, 48, 388           # the dims of the hfw_test golden
    sd = random_whisper_family_state_dict("hf", d.d_model, d.n_heads, d.n_enc_layers, d.n_dec_layers, d.d_ff, tok.vocab_size_in,
                                          tok.vocab_size_out, n_mels, src_positions=frames // 2, tgt_positions=tgt, seed=17, head_gain=5.0,
                                          gains={"decoder_embedder": 0.5})
    for name in TIMED_EVENT_NAMES:                            # (mh_testing.boost_timed_rows, on this family's output head)
        if _has(tok.event_start, name):
            sd["transformer.proj_out.weight"][_ev(tok.event_start, name):_ev(tok.event_end, name)] *= 2.0
    model = MapperatorinatorHIP(sd, d, vocab_size_in=tok.vocab_size_in, vocab_size_out=tok.vocab_size_out, n_mels=n_mels, src_seq_len=frames,
                                tgt_seq_len=tgt, dtype=torch.float32, device="cuda", f_min=0)
    audio = synthetic_audio_varied(3, (frames - 1) * 128, seed=8)
    prompt = torch.tensor([[0, 0, 3], [3, 40, 2068], [0, 3, 9]])
    mk = dict(inputs=audio, decoder_input_ids=prompt, decoder_attention_mask=prompt.ne(0))
    kw = dict(num_beams=2, types_first=True, temperature=0.9, timing_temperature=0.5, mania_column_temperature=0.6,
              taiko_hit_temperature=0.7, lookback_time=500)
    calls = count_kernel_calls(monkeypatch)
    step_path(0)
    ids_k, _ = model_generate(model, tok, mk, gen_kwargs(tgt, **kw))
    ids_t, _ = model_generate(model, tok, mk, gen_kwargs(tgt, beam_use_kernel=False, **kw))
    assert len(calls) == 1 and torch.equal(ids_k, ids_t), (ids_k.tolist(), ids_t.tolist())
    assert ids_k.shape[1] > prompt.shape[1]
    timed = torch.from_numpy(build_sampling(tok, gen_kwargs(tgt, **kw), tgt)[0].host_tok_flags & FLAG_TIMED).bool()
    n_timed = int(timed[ids_k[:, prompt.shape[1]:-1]].sum())
    print("timed events in the best hypotheses:", n_timed)
    assert n_timed > 0, "no timed event emitted: the renormalisation never ran"


def test_prompt_ending_in_an_input_only_id(step_path):
    """An id >= vocab_out as the last prompt column (what the first step's timed-event and conditional-temperature lookups read): it has
    no flags, on the device as on the host.  The types_first tokenizer of the fixtures has no input-only ids, so the model gets 16
    embedding rows behind its vocabulary."""
    from mapperatorinator_amd.modeling import MapperatorinatorHIP
    from mapperatorinator_amd.server import build_sampling
    from mapperatorinator_amd.t5_engine import T5_PRESETS
    from mh_testing import boost_timed_rows, random_t5_state_dict
    _, tok, _, audio, tgt = tf_model()
    hi, extra = tok.vocab_size_out, 16
    sd = random_t5_state_dict(T5_PRESETS["tiny"], tok.vocab_size_in + extra, hi, seed=21, lm_head_gain=6.0)
    boost_timed_rows(sd, tok, 2.0)
    model = MapperatorinatorHIP(sd, T5_PRESETS["tiny"], vocab_size_in=tok.vocab_size_in + extra, vocab_size_out=hi, src_seq_len=251,
                                tgt_seq_len=tgt, dtype=torch.float32, device="cuda")
    prompt = torch.tensor([[0, 3, hi + 7], [3, 40, hi], [0, 3, hi + extra - 1]])
    sp, eos = build_sampling(tok, gen_kwargs(tgt, num_beams=2, types_first=True, temperature=0.9, timing_temperature=0.5,
                                             mania_column_temperature=0.6, taiko_hit_temperature=0.7, lookback_time=500), tgt)
    assert sp.n_cond > 0 and sp.lookback_types_first and len(sp.host_tok_flags) == hi
    outs = []
    for path, uk in ((0, True), (2, True), (0, False)):
        step_path(path)
        outs.append(model.engine.generate_beam(audio.cuda(), prompt, prompt.ne(0), eos, sp, 2, use_kernel=uk)["tokens"])
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), [o.tolist() for o in outs]
    assert outs[0].shape[1] > prompt.shape[1]
