"""-m gpu: option decode_fused_tail -- the three GEMVs that close a decoder layer as one persistent launch (dec_tail_kernel)
against the three launches it replaces.  Each phase runs the stand-alone GEMV's device code with its summation order, so ids
and scores must be BIT-identical between the two settings; mh_t5_generate returns MH_OK only when the hand-off error word of
every chain is zero (a non-zero word becomes MH_ERR_DECODE_TAIL_TIMEOUT), so a returned result is also the "error word is
zero" check.  The second decode of every engine replays the cached step graph on counters that the first one left where a
step ends: the counter-generation check."""
import pytest
import torch

pytestmark = pytest.mark.gpu

NEW = 10      # decoded tokens
SRC = 251


def _t5(dims, dtype, B, seed):
    from mapperatorinator_amd import Tokenizer
    from mapperatorinator_amd.modeling import MapperatorinatorHIP
    from mh_testing import random_t5_state_dict, synthetic_audio
    tok = Tokenizer.benchmark_vocab(src_seq_len=SRC)
    sd = random_t5_state_dict(dims, tok.vocab_size_in, tok.vocab_size_out, seed=seed, lm_head_gain=6.0)
    model = MapperatorinatorHIP(sd, dims, vocab_size_in=tok.vocab_size_in, vocab_size_out=tok.vocab_size_out,
                                src_seq_len=SRC, tgt_seq_len=1 + NEW, dtype=dtype, device="cuda")
    return model, tok, synthetic_audio(B, 32000, seed=seed + 1)


def _whisper(dtype, B, seed):
    from mapperatorinator_amd import Tokenizer
    from mapperatorinator_amd.modeling import MapperatorinatorHIP
    from mapperatorinator_amd.whisper_engine import VARWHISPER_PRESETS
    from mh_testing import random_varwhisper_state_dict, synthetic_audio_varied
    d, frames = VARWHISPER_PRESETS["test"], 250
    tok = Tokenizer.benchmark_vocab(src_seq_len=frames)
    sd = random_varwhisper_state_dict(d.d_model, d.n_heads, d.n_enc_layers, d.n_dec_layers, d.d_ff, tok.vocab_size_in,
                                      tok.vocab_size_out, seed=seed, head_gain=5.0, gains={"decoder_embedder": 0.5})
    model = MapperatorinatorHIP(sd, d, vocab_size_in=tok.vocab_size_in, vocab_size_out=tok.vocab_size_out, n_mels=128,
                                src_seq_len=frames, tgt_seq_len=1 + NEW, dtype=dtype, device="cuda", f_min=20)
    return model, tok, synthetic_audio_varied(B, (frames - 1) * 128, seed=seed + 1)


def _decode(model, tok, audio, fused):
    from mapperatorinator_amd import _lib
    from mapperatorinator_amd.server import build_sampling
    gk = dict(do_sample=False, num_beams=1, max_length=1 + NEW, temperature=1.0, context_type="map", pad_token_id=0)
    sp, _ = build_sampling(tok, gk, 1 + NEW)
    prompt = torch.tensor([[1]] * audio.shape[0])
    model.engine.options["decode_fused_tail"] = fused
    lib = _lib.load()
    lib.mh_t5_step_graph_cache_stats(None, None, 1)
    import ctypes as C
    hits, misses = C.c_long(0), C.c_long(0)
    first = None
    for _ in range(6):      # a replay needs the caller's buffers at the same addresses: torch's caching allocator settles into a
        out = model.engine.generate(audio, prompt, None, [tok.eos_id], sp, dump_logits=True)   # repeating pattern after a call or two
        got = (out["tokens"].cpu().clone(), out["logits"].cpu().clone())
        del out
        if first is None:
            first = got
        assert torch.equal(first[0], got[0]) and torch.equal(first[1], got[1]), "a repeated decode on one engine decoded differently"
        lib.mh_t5_step_graph_cache_stats(C.byref(hits), C.byref(misses), 0)
        if hits.value >= 1:
            break
    assert hits.value >= 1, ("no call replayed a cached step graph", hits.value, misses.value)
    return first


def _check(model, tok, audio, covered=True):
    """covered: the fused kernel has to run for this shape (mh_t5_decode_tail_launches counts its enqueued launches); False: a
    shape the documented fall-back serves with the three launches."""
    from mapperatorinator_amd import _lib
    lib = _lib.load()
    n0 = lib.mh_t5_decode_tail_launches()
    ids0, sc0 = _decode(model, tok, audio, 0)
    n1 = lib.mh_t5_decode_tail_launches()
    assert n1 == n0, "decode_fused_tail = 0 enqueued a fused tail"
    ids1, sc1 = _decode(model, tok, audio, 1)
    n2 = lib.mh_t5_decode_tail_launches()
    assert (n2 > n1) == covered, f"fused tail launches enqueued: {n2 - n1}, expected {'some' if covered else 'none'}"
    assert torch.equal(ids0, ids1), f"token ids differ between decode_fused_tail 0 and 1:\n{ids0}\n{ids1}"
    assert torch.equal(sc0.view(torch.int32), sc1.view(torch.int32)), "per-step scores differ in their bits"
    assert int((ids0[:, 1:] != 0).sum()) > 0


# B = 1: one row, most tiles idle; 3: ragged fragment; 16: full fragment (two chains of 8); 17: two chains of 9 + 8 rows;
# 32: two chains of 16, their tails co-resident.  Waves of (O, wi, wo): tiny and small bf16 (4, 4, 4), small fp32 (4, 4, 8),
# base bf16 (4, 4, 8) -- the headline kernel --, base fp32 (8, 8, 8).  (A chain of more than 16 rows is the single-chain case below.)
@pytest.mark.parametrize("size,dtype,B", [("tiny", torch.bfloat16, 1), ("tiny", torch.float32, 3), ("small", torch.bfloat16, 16),
                                          ("tiny", torch.bfloat16, 17), ("small", torch.float32, 32), ("small", torch.bfloat16, 32),
                                          ("base", torch.bfloat16, 3), ("base", torch.float32, 3)])
def test_fused_tail_is_bit_identical(size, dtype, B):
    from mapperatorinator_amd.t5_engine import T5_PRESETS
    _check(*_t5(T5_PRESETS[size], dtype, B, seed=100 + B))


@pytest.mark.parametrize("dtype,covered", [(torch.float32, True), (torch.bfloat16, False)])
def test_fused_tail_single_chain_of_17_rows(dtype, covered):
    """decode_chains = 1 with 17 rows: two 16-row fragments per GEMV (MF = 2).  fp32 storage runs the fused kernel; bf16 storage is a
    documented fall-back (that kernel would need more than 256 VGPRs): three launches, the same results."""
    from mapperatorinator_amd.t5_engine import T5_PRESETS
    model, tok, audio = _t5(T5_PRESETS["tiny"], dtype, 17, seed=7)
    model.engine.options["decode_chains"] = 1
    _check(model, tok, audio, covered=covered)


def test_fused_tail_ragged_k_split():
    """d_ff = 320 in bf16: 5 k-block pairs over the 4 waves of the wo phase (one wave takes two, three take one); d_ff / 8 = 40
    wi tiles and d_model / 4 = 32 residual tiles on the workgroups' two halves."""
    from mapperatorinator_amd.t5_engine import T5Dims
    dims = T5Dims(d_model=128, d_ff=320, n_heads=2, n_enc_layers=1, n_dec_layers=3)
    _check(*_t5(dims, torch.bfloat16, 5, seed=55))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_fused_tail_whisper_family(dtype):
    """arch 1: biased projections, erf GELU (the LN / BIAS template arguments of the tail kernel)."""
    _check(*_whisper(dtype, 3, seed=77))
