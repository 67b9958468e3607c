"""not gpu: mh_beam_step_sample (beam-sample with the draw inside the beam step kernel) -- the symbol, what it refuses before any
launch, the host routes (`device_draw` is opt-in: without it a beam-sample call goes where it went before), and the rule itself,
restated in numpy (mh_testing/beam_sample.py), against the analytic Plackett-Luce probabilities of sequential sampling without
replacement.

Distribution case: 2 beams x 6 ids, one id masked, K = 4, 16 384 chunks as trials, seed 1234, decode column 5.  With the folding of
the counters in csrc/common.hpp the first draw gives chi-square 4.88 at 10 degrees of freedom (99.9 % quantile 29.59) and the ordered
pair 103.3 at 109 (160.4; no cell's expectation is below 5, the smallest is 7.0); seeds 77 and 2026 gave 15.4 / 99.5 and 14.7 / 114.0.
fp32 and fp64 keys give the same order in all 16 384 chunks, and the masked id is never drawn."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

from conftest import ROOT
from mapperatorinator_amd import _lib
from mh_testing import beam_sample as bsr


@pytest.fixture
def lib():
    return _lib.load()


def descriptor(num_beams=2, V=2080, K=4, do_sample=1, top_k=0, top_p=1.0):
    """Every pointer non-null (never dereferenced: the checks fail on the numbers first)."""
    bs = _lib.MhBeamStep()
    for name, kind in _lib.MhBeamStep._fields_:
        if kind is _lib.VP:
            setattr(bs, name, 64)
    bs.G, bs.num_beams, bs.V, bs.P, bs.max_length, bs.K, bs.cur_len = 1, num_beams, V, 2, 24, K, 2
    bs.sp.temperature, bs.sp.do_sample, bs.sp.top_k, bs.sp.top_p = 1.0, do_sample, top_k, top_p
    return bs


def test_symbol_is_declared_bound_and_exported_at_abi_11(lib):
    hdr = open(os.path.join(ROOT, "include", "mapperhip.h")).read()
    assert re.search(r"\bint\s+mh_beam_step_sample\s*\(\s*const MhBeamStep\*\s*bs,\s*float\*\s*lookback_prev,\s*int min_tokens_to_keep,"
                     r"\s*float\*\s*scores_dump,\s*void\*\s*stream\s*\)", hdr)
    assert re.search(r"#define\s+MH_ABI_VERSION\s+11\b", hdr)
    assert "mh_beam_step_sample" in _lib.SYMBOLS and hasattr(lib, "mh_beam_step_sample")
    assert _lib.ABI_VERSION == 11 and lib.mh_abi_version() == 11
    assert lib.mh_struct_size(9) == -1                                    # no new struct
    assert lib.mh_struct_size(7) == C.sizeof(_lib.MhBeamStep) and lib.mh_struct_size(3) == C.sizeof(_lib.MhSampling)


def refused(lib, bs, keep=2):
    assert lib.mh_beam_step_sample(C.byref(bs), None, keep, None, None) == -1
    return lib.mh_last_error().decode()


def test_sampled_step_names_what_it_refuses_before_any_launch(lib):
    msg = refused(lib, descriptor(do_sample=0))
    assert "mh_beam_step_sample" in msg and "do_sample = 0" in msg, msg
    msg = refused(lib, descriptor(), keep=0)
    assert "min_tokens_to_keep = 0" in msg, msg
    for top_p in (0.0, -0.25, 1.5):
        msg = refused(lib, descriptor(top_p=top_p))
        assert f"top_p = {top_p:g}" in msg and "(0, 1]" in msg, msg
    msg = refused(lib, descriptor(top_k=-3))
    assert "top_k = -3" in msg, msg
    # the limits of mh_beam_step, in its wording
    msg = refused(lib, descriptor(8, 3837, 8193))
    assert "K = 8193" in msg and "8192" in msg, msg
    msg = refused(lib, descriptor(9, 3837, 18))
    assert "9 beams" in msg and "2 .. 8" in msg, msg
    old = lib.mh_get_option(b"beam_step_path")
    try:
        assert lib.mh_set_option(b"beam_step_path", 1) == 0
        msg = refused(lib, descriptor(8, 3837, 16))
        assert "8 x 3837" in msg and "120 KB" in msg and "beam_step_path" in msg, msg
    finally:
        assert lib.mh_set_option(b"beam_step_path", old) == 0
    bs = descriptor()
    bs.sp.lookback_types_first, bs.sp.ts_start, bs.sp.lookback_mask_end = 1, 10, 20     # types_first lookback without its state
    assert "lookback_prev" in refused(lib, bs)


def test_greedy_entries_still_refuse_do_sample(lib):
    bs = descriptor()
    assert lib.mh_beam_step(C.byref(bs), None) == -1 and b"greedy beams only" in lib.mh_last_error()
    assert lib.mh_beam_step_tf(C.byref(bs), None, None) == -1 and b"greedy beams only" in lib.mh_last_error()
    from mapperatorinator_amd.beam import kernel_path_available
    assert not kernel_path_available(types.SimpleNamespace(do_sample=1), 2, 1849, 0)


# ---- host routes ----------------------------------------------------------------------------------------------------------------

class _ReachedDecode(Exception):
    pass


class _StubLib:
    """The first library call of the decode loop ends the run."""

    def mh_t5_decode_workspace_bytes(self, *a):
        raise _ReachedDecode


class _StubEngine:
    def __init__(self, vocab_out=1849, tgt=24):
        self.device, self.dtype, self.lib = torch.device("cpu"), torch.float32, _StubLib()
        self.packed = types.SimpleNamespace(vocab_out=vocab_out, tgt_len=tgt, cfg=C.c_int(0))

    def _s(self):
        return None


def sampled_sp(do_sample=1):
    sp = _lib.MhSampling()
    sp.do_sample, sp.top_p, sp.top_k, sp.temperature, sp.max_length, sp.cfg_scale, sp.seed = do_sample, 0.9, 0, 1.0, 24, 1.0, 7
    return sp


def routes(monkeypatch):
    from mapperatorinator_amd import beam
    seen = []
    monkeypatch.setattr(torch.Tensor, "pin_memory", lambda self, *a, **k: self)         # (no accelerator here)
    orig = beam._beam_search_kernel
    monkeypatch.setattr(beam, "_beam_search_kernel", lambda *a, **k: (seen.append(k.get("sample_keep")), orig(*a, **k))[1])
    return beam, seen


def test_device_draw_is_opt_in_and_excludes_sample_fn(monkeypatch):
    beam, seen = routes(monkeypatch)
    eng, prompt = _StubEngine(), torch.tensor([[1, 7, 9]])
    args = (eng, torch.zeros(1), prompt, None, [3, 4])
    with pytest.raises(ValueError, match="sample_fn"):
        beam.beam_search(*args, sampled_sp(), 2, sample_fn=torch.multinomial, device_draw=True)
    # without the opt-in: the kernel is refused by name, and the default route is the torch-op bookkeeping (never _beam_search_kernel)
    with pytest.raises(NotImplementedError, match="mh_beam_step"):
        beam.beam_search(*args, sampled_sp(), 2, use_kernel=True)
    with pytest.raises(_ReachedDecode):
        beam.beam_search(*args, sampled_sp(), 2)
    assert seen == []
    # with it: the kernel route, min_tokens_to_keep = #eos + 1 (what BeamProcessors is given)
    with pytest.raises(_ReachedDecode):
        beam.beam_search(*args, sampled_sp(), 2, device_draw=True)
    assert seen == [3]
    with pytest.raises(_ReachedDecode):
        beam.beam_search(*args, sampled_sp(), 2, device_draw=True, use_kernel=False)     # the same rule in torch ops
    assert seen == [3]
    with pytest.raises(NotImplementedError, match="mh_beam_step_sample"):
        beam.beam_search(*args, sampled_sp(), 9, device_draw=True, use_kernel=True)
    # greedy beams ignore it: mh_beam_step as before
    with pytest.raises(_ReachedDecode):
        beam.beam_search(*args, sampled_sp(do_sample=0), 2, device_draw=True)
    assert seen == [3, None]


class _RecordingEngine:
    """What server.model_generate needs of an engine, with generate_beam's signature of before this mode: an unexpected keyword
    is a TypeError."""

    def __init__(self):
        self.calls = []

    def generate_beam(self, audio, prompt, mask, eos, sp, num_beams, negative_prompt=None, sample_fn=None, use_kernel=None,
                      cross_kv_fp8=False, **new):
        self.calls.append(new)
        return dict(tokens=torch.zeros((prompt.shape[0], prompt.shape[1] + 1), dtype=torch.int64), n_cols=prompt.shape[1] + 1, logits=None)


def test_model_generate_hands_the_flag_down_only_when_asked():
    from mapperatorinator_amd import Tokenizer
    from mapperatorinator_amd.server import model_generate
    tok = Tokenizer.benchmark_vocab(src_seq_len=64)
    eng = _RecordingEngine()
    model = types.SimpleNamespace(engine=eng, dtype=torch.float32, config=types.SimpleNamespace(max_target_positions=24))
    prompt = torch.tensor([[tok.sos_id, 7, 9]])
    mk = dict(inputs=torch.zeros(1, 16), decoder_input_ids=prompt, decoder_attention_mask=prompt.ne(0))
    kw = dict(precision="fp32", do_sample=True, num_beams=2, top_p=0.9, top_k=0, max_length=24, cfg_scale=1.0, timeshift_bias=0,
              types_first=False, temperature=1.0, lookback_time=0, lookahead_time=0, context_type="map", pad_token_id=0)
    model_generate(model, tok, mk, kw)
    model_generate(model, tok, mk, dict(kw, beam_sample_kernel=True))
    assert eng.calls == [{}, {"device_draw": True}]


# ---- the rule ---------------------------------------------------------------------------------------------------------------------

def test_uniform_is_the_samplers_generator_under_the_stated_folding():
    """The numpy restatement against plain Python-int arithmetic, and the torch-op draw of beam.py (int64 tensors) against both."""
    from mapperatorinator_amd.beam import _device_draw, _rng_mix64, _s64
    M = (1 << 64) - 1

    def mix(seed, row, step):      # rng_mix64 of csrc/common.hpp, spelled out
        z = (seed + 0x9E3779B97F4A7C15 * ((row * 0x100000001 + step + 1) & M)) & M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)
    seed, row, col = 0xDEADBEEFCAFEF00D, 0xFFFFFFFE, 17
    sub = mix(seed, row, col)
    assert int(bsr.rng_mix64(seed, row, col)) == sub
    t = _rng_mix64(torch.tensor(_s64(seed)), torch.tensor(row), torch.tensor(col))
    assert int(t) & M == sub
    u = bsr.beam_uniform(seed, [row, row + 1], col, 50)                    # (row + 1 = 2^32 - 1: the last RNG row)
    assert u.dtype == np.float32 and u.shape == (2, 50) and (u > 0).all() and (u <= 1).all()
    for flat in (0, 1, 49):
        z = mix(sub, 0, flat)
        assert float(u[0, flat]) == float(np.float32((z >> 40) + 0.5) * np.float32(2.0 ** -24))
    # n = 2^24 - 1 rounds to exactly 1.0: the key's clamp is needed
    assert float(np.float32(float(2 ** 24 - 1) + 0.5) * np.float32(2.0 ** -24)) == 1.0 and np.isfinite(bsr.gumbel(np.float32([1.0]))).all()
    gen = torch.Generator().manual_seed(3)
    acc = torch.randn(2, 50, generator=gen) * 2
    acc[0, 7] = acc[1, 30] = float("-inf")
    keys = []
    idx = _device_draw(acc, 6, seed, row, col, keys_out=keys)
    for g in range(2):
        want, want_keys = bsr.draw(acc[g].numpy(), u[g], 6, np.float32)
        assert idx[g].tolist() == want.tolist()
        assert np.allclose(keys[0][g, :7].numpy(), want_keys, rtol=0, atol=1e-5)
        assert bsr.deciding_gap(keys[0][g].numpy(), 6, 2) > 0


def test_generate_and_the_scheduler_hand_the_flag_down_only_when_asked(monkeypatch):
    """`beam_sample_kernel=True` through MapperatorinatorHIP.generate (-> generate_beam(device_draw=True)) and through the scheduler's
    call of beam_search; without it neither passes the keyword at all."""
    from mapperatorinator_amd import Tokenizer, beam as beam_mod
    from mapperatorinator_amd.modeling import MapperatorinatorHIP
    from mapperatorinator_amd.scheduler import SequentialWindowScheduler, SongJob
    from test_host_cpu import _StandInEngine
    eng = _RecordingEngine()
    cfgm = types.SimpleNamespace(max_target_positions=40, pad_token_id=0, vocab_size=64, eos_token_id=2)
    me = types.SimpleNamespace(engine=eng, dtype=torch.float32, config=cfgm, device=torch.device("cpu"), _row_bias=lambda n, kw: None)
    for extra in ({}, dict(beam_sample_kernel=True), dict(beam_sample_kernel=False)):
        MapperatorinatorHIP.generate(me, inputs=torch.zeros(1, 16), decoder_input_ids=torch.tensor([[1]]), num_beams=2, max_length=40,
                                     do_sample=True, top_p=0.9, **extra)
    assert eng.calls == [{}, {"device_draw": True}, {}]
    tok = Tokenizer.benchmark_vocab(src_seq_len=251)
    tgt = 24
    model = types.SimpleNamespace(engine=_StandInEngine(tok.vocab_size_out, eos_every=5), config=types.SimpleNamespace(max_target_positions=tgt))
    seen = []

    def fake_beam_search(engine, kv, prompt, mask, eos, sp, nb, sample_fn=None, kv_fp8=None, **new):
        seen.append((int(sp.do_sample), new))
        G = kv.shape[2]
        return torch.cat([prompt[-G:].long(), torch.full((G, 1), int(sorted(eos)[0]))], 1)
    monkeypatch.setattr(beam_mod, "beam_search", fake_beam_search)

    def job(extra):
        frames = torch.randn(2, 64, generator=torch.Generator().manual_seed(1))
        ask = dict(decoder_input_ids=torch.tensor([[tok.sos_id, 7]]))
        return SongJob(frames=frames, prompt_fn=lambda w: dict(ask), on_result=lambda w, row, st: None,
                       generate_kwargs=dict(max_length=tgt, do_sample=True, top_p=0.9, cfg_scale=1.0, num_beams=2, **extra))
    SequentialWindowScheduler(model, tok, decode_batch=8).run([job({})])
    SequentialWindowScheduler(model, tok, decode_batch=8).run([job(dict(beam_sample_kernel=True))])
    assert seen and all(d == 1 for d, _ in seen)
    n = len(seen) // 2
    assert [new for _, new in seen] == [{}] * n + [{"device_draw": True}] * n


def test_warpers_as_one_cut_value_are_hfs_warpers():
    """The rule of row_cut (whole tie groups, masses by value) removes what HF's element-wise TopK / TopP remove, and what
    BeamProcessors (pinned to HF's warpers by test_host_cpu.py) removes, on rows without a boundary tie."""
    from mapperatorinator_amd.beam import BeamProcessors
    rng = np.random.default_rng(5)
    x = np.log(rng.dirichlet(np.full(97, 0.3), size=4)).astype(np.float32)
    x[1, 10:20] = -np.inf
    for top_k, top_p, keep in ((5, 1.0, 1), (0, 0.8, 1), (20, 0.6, 3), (2, 0.9, 6), (0, 0.05, 9)):
        acc, margin, same = bsr.warped_scores(x, np.zeros(4), top_k, top_p, keep)
        assert same and margin > 1e-4, (top_k, top_p, keep, margin)
        sp = types.SimpleNamespace(do_sample=1, top_k=top_k, top_p=top_p, ts_start=0, ts_end=0, temperature=1.0, n_cond=0,
                                   lookback_mask_end=0, lookback_types_first=0, n_sos=0, sos_ids=[])
        got = BeamProcessors(sp, "cpu", min_tokens_to_keep=keep)(torch.zeros((4, 1), dtype=torch.long), torch.from_numpy(x))
        assert np.array_equal(np.isinf(got.numpy()), np.isinf(acc)), (top_k, top_p, keep)
        assert (np.isfinite(acc).sum(1) >= min(keep, 97)).all()


def test_numpy_rule_draws_with_plackett_luce_probabilities():
    nb, V = bsr.PL_X.shape
    acc = (bsr.PL_X + bsr.PL_RS[:, None]).reshape(-1)
    u = bsr.beam_uniform(bsr.PL_SEED, np.arange(bsr.PL_TRIALS), bsr.PL_COLUMN, nb * V)
    draws = np.empty((bsr.PL_TRIALS, bsr.PL_K), dtype=np.int64)
    same32 = 0
    for c in range(bsr.PL_TRIALS):
        draws[c], _ = bsr.draw(acc, u[c], bsr.PL_K)
        same32 += np.array_equal(draws[c], bsr.draw(acc, u[c], bsr.PL_K, np.float32)[0])
    assert (np.sort(draws, axis=1)[:, 1:] != np.sort(draws, axis=1)[:, :-1]).all()      # without replacement
    (chi1, dof1), (chi2, dof2) = bsr.plackett_luce_chi2(acc, draws)
    print(f"first draw: chi-square {chi1:.2f} at {dof1} dof; ordered pair: {chi2:.2f} at {dof2} dof; fp32 order equal in {same32} chunks")
    assert (dof1, dof2) == (10, 109)
    assert chi1 < bsr.CHI2_999[dof1] and chi2 < bsr.CHI2_999[dof2]
    assert same32 == bsr.PL_TRIALS
