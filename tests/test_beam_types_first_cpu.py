"""not gpu: beam search under LookbackBiasLogitsWarper(types_first=True) -- the library entry mh_beam_step_tf (declared, bound,
exported, its refusals), the torch-op form of the processor replayed against what the reference's processor list did under HF beam
search (tests/golden/t5_tiny_tf_beam.npz, tools/make_beam_tf_golden.py), and the public seam down to `beam_search`.

The replay pins the warper's state BY ROW SLOT: the reference keeps `last_scores` from call to call while HF reorders the beams in
between, so slot r renormalises with the EOS mass of whatever beam sat in slot r one step earlier.  In the 9 recorded steps 8
renormalising rows sit in a slot whose beam changed.  Gathering `BeamProcessors.last_scores` by beam index before every call (tried
by hand: each row takes the state of the previous step's row whose ids it continues) fails the replay at the fifth recorded step:
the probability of the first TIME_SHIFT id, prob_eos_extra, is off by 4.7e-5 where `assert_scores_close` allows 1e-5.  (The recorded
run decodes at temperatures 3 / 4 for that: at temperature ~1 this model's EOS mass is ~1e-8 and both states give the same scores.)"""
import ctypes as C
import json
import os
import re
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, assert_scores_close
from mapperatorinator_amd import _lib


@pytest.fixture
def lib():
    lib = _lib.load()
    old = lib.mh_get_option(b"beam_step_path")
    yield lib
    assert lib.mh_set_option(b"beam_step_path", old) == 0


def tf_golden():
    from mapperatorinator_amd import Tokenizer
    g = np.load(f"{GOLDEN}/t5_tiny_tf_beam.npz")
    tok = Tokenizer.from_json(f"{GOLDEN}/tokenizer_types_first.json")
    assert tok.vocab_size_out == int(g["vocab_out"]) and tok.vocab_size_in == int(g["vocab_in"])
    return g, tok, json.loads(str(g["runs"]))


def gen_kwargs(tgt, **over):
    kw = dict(precision="fp32", do_sample=False, num_beams=1, top_p=1.0, top_k=0, max_length=tgt, cfg_scale=1.0, timeshift_bias=0,
              types_first=False, temperature=1.0, lookback_time=0, lookahead_time=0, context_type="map", pad_token_id=0)
    kw.update(over)
    return kw


def test_beam_step_tf_is_declared_bound_and_exported_at_abi_11(lib):
    hdr = open(os.path.join(ROOT, "include", "mapperhip.h")).read()
    assert re.search(r"\bint\s+mh_beam_step_tf\s*\(\s*const MhBeamStep\*\s*bs,\s*float\*\s*lookback_prev,\s*void\*\s*stream\s*\)", hdr)
    assert re.search(r"#define\s+MH_ABI_VERSION\s+11\b", hdr)
    assert "mh_beam_step_tf" in _lib.SYMBOLS and hasattr(lib, "mh_beam_step_tf")
    assert _lib.ABI_VERSION == 11 and lib.mh_abi_version() == 11
    assert lib.mh_struct_size(9) == -1                                    # no new struct came with it


def descriptor(num_beams, V, K, types_first=True):
    """Every pointer non-null (never dereferenced: the checks below fail first)."""
    bs = _lib.MhBeamStep()
    for name, kind in _lib.MhBeamStep._fields_:
        if kind is _lib.VP:
            setattr(bs, name, 64)
    bs.G, bs.num_beams, bs.V, bs.P, bs.max_length, bs.K, bs.cur_len = 1, num_beams, V, 2, 24, K, 2
    bs.sp.temperature = 1.0
    if types_first:
        bs.sp.lookback_types_first, bs.sp.ts_start, bs.sp.ts_end, bs.sp.lookback_mask_end, bs.sp.tok_flags = 1, 100, 300, 150, 64
    return bs


def test_beam_step_tf_refuses_with_a_message_before_any_launch(lib):
    def refused(bs, prev=64):
        assert lib.mh_beam_step_tf(None if bs is None else C.byref(bs), prev, None) == -1
        return lib.mh_last_error().decode()
    assert "mh_beam_step_tf: null argument" in refused(None)
    bs = descriptor(2, 2080, 4)
    bs.logits = None
    assert "mh_beam_step_tf: null argument" in refused(bs)
    assert "needs lookback_prev" in refused(descriptor(2, 2080, 4), prev=None)
    bs = descriptor(2, 2080, 4)
    bs.sp.tok_flags = None
    assert "needs tok_flags" in refused(bs)
    bs = descriptor(2, 2080, 4)
    bs.sp.lookback_mask_end = 2081
    assert "lookback_mask_end 2081" in refused(bs)
    # every other limit and message is mh_beam_step's
    msg = refused(descriptor(8, 3837, 8193))
    assert "K = 8193" in msg and "8192" in msg, msg
    msg = refused(descriptor(9, 3837, 18))
    assert "9 beams" in msg and "2 .. 8" in msg, msg
    bs = descriptor(2, 2080, 4)
    bs.cur_len = 24
    assert "cur_len 24" in refused(bs)
    bs = descriptor(2, 2080, 4)
    bs.sp.do_sample = 1
    assert "greedy beams only" in refused(bs)
    assert lib.mh_set_option(b"beam_step_path", 1) == 0
    msg = refused(descriptor(8, 3837, 16))
    assert "8 x 3837" in msg and "120 KB" in msg and "beam_step_path" in msg, msg
    # ... and mh_beam_step, which has no state argument, keeps refusing the renormalisation
    assert lib.mh_beam_step(C.byref(descriptor(2, 2080, 4)), None) == -1
    assert b"types_first lookback renormalisation is not built" in lib.mh_last_error()


def test_processors_replay_the_reference_list_with_the_state_by_row_slot():
    from mapperatorinator_amd.beam import BeamProcessors
    from mapperatorinator_amd.server import build_sampling
    g, tok, runs = tf_golden()
    tgt, run = int(g["tgt"]), str(g["record"])
    sp, _ = build_sampling(tok, gen_kwargs(tgt, **runs[run]), tgt)
    assert sp.lookback_types_first and sp.ts_start < sp.lookback_mask_end < sp.ts_end
    procs = BeamProcessors(sp, torch.device("cpu"))
    rec_ids, rec_in, rec_out = torch.from_numpy(g["rec_ids"]).long(), torch.from_numpy(g["rec_in"]), torch.from_numpy(g["rec_out"])
    P = g["prompt"].shape[1]
    assert rec_in.shape[1] == g["prompt"].shape[0] * runs[run]["num_beams"]
    renormalised = moved = 0
    for i in range(rec_in.shape[0]):
        ids = rec_ids[i, :, :P + i]
        assert (ids >= 0).all() and (i + 1 == rec_in.shape[0] or (rec_ids[i, :, P + i] == -1).all())
        got = procs(ids, rec_in[i])
        worst = assert_scores_close(got, rec_out[i], 2e-4, sp.ts_start)
        rows = torch.from_numpy(g["rec_renorm"][i])                      # where the reference's warper changed its input
        assert torch.equal(rows, procs._flag(ids[:, -1], 1) & (i > 0))
        renormalised += int(rows.sum())
        if i:
            moved += int((rows & (ids[:, :-1] != rec_ids[i - 1, :, :P + i - 1]).any(dim=-1)).sum())
        print(f"step {i}: {int(rows.sum())} rows renormalised, worst |dscore| {worst:.2e}")
    assert renormalised > 0 and not g["rec_renorm"][0].any()             # no previous call at the first step: passed through
    assert moved > 0, "the fixture no longer tells by-slot from by-beam state"


class _ReachedDecode(Exception):
    pass


class _StubLib:
    """The first library call of the decode loop ends the run: everything `beam_search` refuses, it refuses before."""

    def mh_t5_decode_workspace_bytes(self, *a):
        raise _ReachedDecode


class _StubEngine:
    def __init__(self, vocab_out, tgt):
        self.device, self.dtype, self.lib = torch.device("cpu"), torch.float32, _StubLib()
        self.packed = types.SimpleNamespace(vocab_out=vocab_out, tgt_len=tgt, cfg=C.c_int(0))
        self.calls = []

    def _s(self):
        return None

    def generate_beam(self, audio, prompt, mask, eos, sp, num_beams, negative_prompt=None, sample_fn=None, use_kernel=None,
                      cross_kv_fp8=False):
        from mapperatorinator_amd.beam import beam_search
        self.calls.append((bool(sp.lookback_types_first), int(num_beams), use_kernel))
        return beam_search(self, torch.zeros(1), prompt, mask, eos, sp, num_beams, sample_fn=sample_fn, use_kernel=use_kernel)


@pytest.mark.parametrize("use_kernel", [None, False])
def test_model_generate_reaches_the_decode_loop_under_beams_and_types_first_lookback(use_kernel, monkeypatch):
    """`model_generate(num_beams=2, types_first=True, lookback_time > 0)` -- every window but the first of a V29 song -- goes through
    `beam_search` into the decode loop of either form; before mh_beam_step_tf both forms raised NotImplementedError on the way."""
    from mapperatorinator_amd.beam import kernel_path_available
    from mapperatorinator_amd.server import build_sampling, model_generate
    g, tok, runs = tf_golden()
    tgt = int(g["tgt"])
    kw = gen_kwargs(tgt, **runs["tb2"])
    sp, eos = build_sampling(tok, kw, tgt)
    assert sp.lookback_types_first and sp.num_beams == 2 and kernel_path_available(sp, 2, tok.vocab_size_out, len(eos))
    monkeypatch.setattr(torch.Tensor, "pin_memory", lambda self, *a, **k: self)         # (no accelerator here)
    engine = _StubEngine(tok.vocab_size_out, tgt)
    model = types.SimpleNamespace(engine=engine, dtype=torch.float32, config=types.SimpleNamespace(max_target_positions=tgt))
    prompt = torch.from_numpy(g["prompt"])
    mk = dict(inputs=torch.zeros(prompt.shape[0], 16), decoder_input_ids=prompt, decoder_attention_mask=prompt.ne(0))
    with pytest.raises(_ReachedDecode):
        model_generate(model, tok, mk, dict(kw, beam_use_kernel=use_kernel))
    assert engine.calls == [(True, 2, use_kernel)]


def test_kernel_path_available_reads_do_sample_first():
    from mapperatorinator_amd.beam import kernel_path_available
    assert not kernel_path_available(types.SimpleNamespace(do_sample=1), 2, 1849, 0)
    assert kernel_path_available(types.SimpleNamespace(do_sample=0, lookback_types_first=1, lookback_mask_end=150, ts_start=100), 2, 1849, 0)
