"""not gpu: the e4m3 cross K/V mode on the host side -- the step-wise entry mh_t5_step_fp8 is declared, bound and exported at
ABI 11; `cross_kv_fp8` reaches the beam path (no NotImplementedError any more) and an fp32-storage model refuses it with a
ValueError before anything is encoded, on the greedy and on the beam path."""
import ctypes as C
import os
import re
import types

import pytest
import torch

from conftest import ROOT
from mapperatorinator_amd import Tokenizer, _lib


def test_step_fp8_is_declared_bound_and_exported_at_abi_11():
    hdr = open(os.path.join(ROOT, "include", "mapperhip.h")).read()
    assert re.search(r"\bint\s+mh_t5_step_fp8\s*\(", hdr), "mh_t5_step_fp8 is not declared in include/mapperhip.h"
    assert re.search(r"#define\s+MH_ABI_VERSION\s+11\b", hdr)
    assert "mh_t5_step_fp8" in _lib.SYMBOLS
    restype, argtypes = _lib.SYMBOLS["mh_t5_step_fp8"]
    step_args = _lib.SYMBOLS["mh_t5_step"][1]
    # mh_t5_step with the packed copy as one more argument, behind cross_kv
    assert restype is C.c_int and list(argtypes) == list(step_args[:3]) + [C.c_void_p] + list(step_args[3:])
    lib = _lib.load()
    assert hasattr(lib, "mh_t5_step_fp8")
    assert _lib.ABI_VERSION == 11 and lib.mh_abi_version() == 11


def test_step_fp8_validates_before_touching_the_device():
    lib = _lib.load()
    bad = _lib.MhT5Config(96, 64, 256, 2, 2, 2, 10, 10, 388, 416, 251, 48, 0, 1e-6)     # d_model no multiple of 128
    assert lib.mh_t5_step_fp8(C.byref(bad), None, None, None, 1, 1, None, 0, None, 0, None, None, 0, None) == -1
    assert b"d_model" in lib.mh_last_error()
    cfg = _lib.MhT5Config(128, 64, 256, 2, 2, 2, 10, 10, 388, 416, 251, 48, 0, 1e-6)    # fine, but every pointer NULL
    assert lib.mh_t5_step_fp8(C.byref(cfg), None, None, None, 1, 1, None, 0, None, 0, None, None, 0, None) == -1
    assert b"mh_t5_step_fp8: null argument" in lib.mh_last_error()
    # fp32 storage (dtype is the 13th field: 0 = fp32) is refused by the library too, with non-NULL pointers that are never followed
    assert cfg.dtype == 0
    w = _lib.MhT5Weights()
    one = C.c_void_p(256)
    assert lib.mh_t5_step_fp8(C.byref(cfg), C.byref(w), one, one, 1, 1, one, 0, None, 0, one, one, 1 << 40, None) == -1
    assert b"bf16 storage" in lib.mh_last_error()


class _RecordingEngine:
    """What server.model_generate needs of an engine: records how generate / generate_beam were called."""

    def __init__(self, dtype):
        self.dtype, self.calls = dtype, []

    def generate(self, audio, prompt, mask, eos, sp, **kw):
        self.calls.append(("generate", kw))
        return dict(tokens=prompt.clone(), n_cols=prompt.shape[1], logits=None)

    def generate_beam(self, audio, prompt, mask, eos, sp, num_beams, **kw):
        self.calls.append(("generate_beam", dict(kw, num_beams=num_beams)))
        return dict(tokens=prompt.clone(), n_cols=prompt.shape[1], logits=None)


def _stub_model(dtype, tgt=40):
    eng = _RecordingEngine(dtype)
    return types.SimpleNamespace(engine=eng, dtype=dtype, config=types.SimpleNamespace(max_target_positions=tgt)), eng


@pytest.mark.parametrize("num_beams", [1, 2])
def test_model_generate_passes_the_flag_on_both_paths(num_beams):
    from mapperatorinator_amd.server import model_generate
    tok = Tokenizer.benchmark_vocab(src_seq_len=251)
    model, eng = _stub_model(torch.bfloat16)
    mk = dict(inputs=torch.zeros(1, 16), decoder_input_ids=torch.tensor([[tok.sos_id]]))
    gk = dict(do_sample=False, num_beams=num_beams, max_length=40, cfg_scale=1.0, cross_kv_fp8=True)
    model_generate(model, tok, mk, gk)                   # (the parent raised NotImplementedError for num_beams > 1)
    (name, kw), = eng.calls
    assert name == ("generate_beam" if num_beams > 1 else "generate") and kw["cross_kv_fp8"] is True
    eng.calls.clear()
    model_generate(model, tok, mk, dict(gk, cross_kv_fp8=False))
    assert eng.calls[0][1]["cross_kv_fp8"] is False


@pytest.mark.parametrize("num_beams", [1, 2])
def test_fp32_model_refuses_the_flag_with_value_error(num_beams):
    from mapperatorinator_amd.server import model_generate
    tok = Tokenizer.benchmark_vocab(src_seq_len=251)
    model, eng = _stub_model(torch.float32)
    mk = dict(inputs=torch.zeros(1, 16), decoder_input_ids=torch.tensor([[tok.sos_id]]))
    gk = dict(do_sample=False, num_beams=num_beams, max_length=40, cfg_scale=1.0, cross_kv_fp8=True)
    with pytest.raises(ValueError, match="bf16 storage"):
        model_generate(model, tok, mk, gk)
    assert eng.calls == []                               # refused before the engine was asked for anything
    model_generate(model, tok, mk, dict(gk, cross_kv_fp8=False))
    assert len(eng.calls) == 1


@pytest.mark.parametrize("num_beams", [1, 2])
def test_engine_entries_refuse_fp32_storage_before_any_device_work(num_beams):
    """T5Engine.generate / generate_beam and the search itself check the storage type first: called here on an object that has
    nothing but a dtype, so anything past the check would raise AttributeError instead."""
    from mapperatorinator_amd import beam
    from mapperatorinator_amd.t5_engine import T5Engine
    eng = types.SimpleNamespace(dtype=torch.float32, device=torch.device("cpu"))
    prompt = torch.tensor([[1]])
    with pytest.raises(ValueError, match="bf16 storage"):
        if num_beams == 1:
            T5Engine.generate(eng, None, prompt, None, [], None, cross_kv_fp8=True)
        else:
            T5Engine.generate_beam(eng, torch.zeros(1, 16), prompt, None, [], types.SimpleNamespace(cfg_scale=1.0), num_beams,
                                   cross_kv_fp8=True)
    with pytest.raises(ValueError, match="bf16 storage"):
        beam._step_kv_fp8(eng, torch.zeros(1, 2, 1, 1, 1, 64), True)
    assert beam._step_kv_fp8(eng, torch.zeros(1, 2, 1, 1, 1, 64), None) is None


def test_modeling_generate_refuses_fp32_and_has_no_beam_refusal():
    """MapperatorinatorHIP.generate: ValueError for fp32 storage on both paths; the word NotImplementedError no longer stands next
    to cross_kv_fp8 anywhere in the host package."""
    from mapperatorinator_amd.modeling import MapperatorinatorHIP
    eng = _RecordingEngine(torch.float32)
    cfgm = types.SimpleNamespace(max_target_positions=40, pad_token_id=0, vocab_size=64, eos_token_id=2)
    me = types.SimpleNamespace(engine=eng, dtype=torch.float32, config=cfgm, device=torch.device("cpu"), _row_bias=lambda n, kw: None)
    for nb in (1, 2):
        with pytest.raises(ValueError, match="bf16 storage"):
            MapperatorinatorHIP.generate(me, inputs=torch.zeros(1, 16), decoder_input_ids=torch.tensor([[1]]), num_beams=nb,
                                         max_length=40, cross_kv_fp8=True)
    assert eng.calls == []
    me.dtype = eng.dtype = torch.bfloat16
    for nb in (1, 2):
        MapperatorinatorHIP.generate(me, inputs=torch.zeros(1, 16), decoder_input_ids=torch.tensor([[1]]), num_beams=nb, max_length=40,
                                     cross_kv_fp8=True)
    assert [(n, kw["cross_kv_fp8"]) for n, kw in eng.calls] == [("generate", True), ("generate_beam", True)]
    for f in ("server.py", "modeling.py", "scheduler.py", "beam.py", "t5_engine.py"):
        src = open(os.path.join(ROOT, "mapperatorinator_amd", f)).read()
        assert not re.search(r"NotImplementedError\([^)]*cross_kv_fp8", src), f


@pytest.mark.parametrize("cfg_scale", [1.0, 2.0])
def test_scheduler_hands_the_flag_to_the_beam_search(monkeypatch, cfg_scale):
    """SequentialWindowScheduler with num_beams = 2 and cross_kv_fp8 on a stand-in engine (the pattern of
    tests/test_host_cpu.py): no NotImplementedError, the search is asked for the e4m3 copy, and the greedy path of the same
    scheduler gets a packed copy from the engine."""
    from mapperatorinator_amd import beam as beam_mod
    from mapperatorinator_amd.scheduler import SequentialWindowScheduler, SongJob
    from test_host_cpu import _StandInEngine
    tok = Tokenizer.benchmark_vocab(src_seq_len=251)
    tgt = 24
    eng = _StandInEngine(tok.vocab_size_out, eos_every=5)
    made = []
    eng.cross_kv_fp8 = lambda kv: made.append(kv.shape[2]) or torch.zeros(4, dtype=torch.uint8)
    model = types.SimpleNamespace(engine=eng, config=types.SimpleNamespace(max_target_positions=tgt))
    seen = []

    def fake_beam_search(engine, kv, prompt, mask, eos, sp, nb, **kw):
        seen.append(dict(rows=prompt.shape[0], kv_rows=kv.shape[2], nb=nb, kv_fp8=kw.get("kv_fp8")))
        G = kv.shape[2]
        return torch.cat([prompt[-G:].long(), torch.full((G, 1), int(sorted(eos)[0]))], 1)
    monkeypatch.setattr(beam_mod, "beam_search", fake_beam_search)
    results = []

    def job(nb):
        frames = torch.randn(2, 64, generator=torch.Generator().manual_seed(nb))
        ask = dict(decoder_input_ids=torch.tensor([[tok.sos_id, 7]]))
        if cfg_scale > 1:
            ask["negative_prompt"] = torch.tensor([[tok.sos_id]])
        return SongJob(frames=frames, prompt_fn=lambda w: dict(ask), on_result=lambda w, row, st: results.append((nb, w, row)),
                       generate_kwargs=dict(max_length=tgt, do_sample=False, cfg_scale=cfg_scale, num_beams=nb, cross_kv_fp8=True))
    SequentialWindowScheduler(model, tok, decode_batch=8).run([job(2), job(1)])
    assert len(seen) == 2 and all(s["kv_fp8"] is True and s["nb"] == 2 and s["kv_rows"] == 1 for s in seen)
    assert made == [1, 1]                                 # the greedy windows: one packed copy per decode call, made by the engine
    assert sorted((nb, w) for nb, w, _ in results) == [(1, 0), (1, 1), (2, 0), (2, 1)]
