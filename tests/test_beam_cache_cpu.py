"""not gpu: beam search over an indexed self-attention cache (`beam_cache="indexed"`, `beam_prefill=True`) on the host side -- the
five entries are declared, bound and exported at ABI 11; each refuses bad arguments with its message before any launch; the two
kwargs reach `beam_search` from `model_generate`, `MapperatorinatorHIP.generate` and the scheduler; the indexed route calls none
of the copy route's entries and asks for no reorder scratch; the bad combinations raise ValueError."""
import ctypes as C
import os
import re
import types

import pytest
import torch

from conftest import ROOT
from mapperatorinator_amd import Tokenizer, _lib

NEW = ("mh_t5_step_indexed", "mh_t5_beam_index_bytes", "mh_t5_beam_index_init", "mh_t5_reorder_index", "mh_t5_step_prefill")


def _cfg(d_model=128, dtype=0, tgt=48):
    """the config of tests/test_cross_kv_fp8_cpu.py: tiny dims, tgt_len 48, fp32 storage unless told otherwise"""
    cfg = _lib.MhT5Config(d_model, 64, 256, 2, 2, 2, 10, 10, 388, 416, 251, tgt, dtype, 1e-6)
    assert cfg.tgt_len == tgt and cfg.dtype == dtype
    return cfg


def test_the_five_entries_are_declared_bound_and_exported_at_abi_11():
    hdr = open(os.path.join(ROOT, "include", "mapperhip.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\bint(64_t)?\s+%s\s*\(" % name, hdr), f"{name} is not declared in include/mapperhip.h"
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert re.search(r"#define\s+MH_ABI_VERSION\s+11\b", hdr)
    assert _lib.ABI_VERSION == 11 and lib.mh_abi_version() == 11
    assert "cache_utils.py:16-20" in hdr[hdr.index("mh_t5_beam_index_bytes") - 3000: hdr.index("mh_t5_beam_index_bytes")]
    # mh_t5_step_fp8's arguments with the table in front of the stream
    step8 = _lib.SYMBOLS["mh_t5_step_fp8"][1]
    assert list(_lib.SYMBOLS["mh_t5_step_indexed"][1]) == list(step8[:-1]) + [C.c_void_p, step8[-1]]
    assert _lib.SYMBOLS["mh_t5_beam_index_bytes"][0] is C.c_int64
    assert lib.mh_t5_beam_index_bytes(C.byref(_cfg()), 6) == 6 * 48
    assert lib.mh_t5_beam_index_bytes(None, 6) == -1 and lib.mh_t5_beam_index_bytes(C.byref(_cfg()), 0) == -1


def test_every_entry_refuses_bad_arguments_before_any_launch():
    """Non-NULL pointers below are the address 256: a launch would fault on it, a refusal never follows it."""
    lib = _lib.load()
    cfg, w, one = _cfg(), _lib.MhT5Weights(), C.c_void_p(256)
    big = 1 << 40

    def refused(rc, msg):
        assert rc == -1, rc
        err = lib.mh_last_error()
        assert msg in err, (msg, err)
    # mh_t5_step_indexed: null table, null anything, position outside the cache, ragged groups, fp32 storage with the e4m3 copy
    step = lambda c, B, grp, pos, kv8, origin, ids=one: lib.mh_t5_step_indexed(C.byref(c), C.byref(w), one, kv8, B, grp, ids, pos, None,
                                                                             1, one, one, big, origin, None)
    refused(step(cfg, 4, 2, 0, None, None), b"mh_t5_step_indexed: null argument")
    refused(step(cfg, 4, 2, 0, None, one, ids=None), b"mh_t5_step_indexed: null argument")
    refused(step(cfg, 4, 2, 48, None, one), b"mh_t5_step_indexed: position 48 outside the cache")
    refused(step(cfg, 4, 2, -1, None, one), b"mh_t5_step_indexed: position -1 outside the cache")
    refused(step(cfg, 4, 3, 0, None, one), b"mh_t5_step_indexed: 4 rows are not whole groups of 3")
    refused(step(cfg, 4, 2, 0, one, one), b"mh_t5_step_indexed: the fp8 cross K/V copy needs bf16 storage")
    refused(step(_cfg(d_model=96), 4, 2, 0, None, one), b"d_model")
    refused(step(_cfg(tgt=2561), 4, 2, 0, None, one), b"mh_t5_step_indexed: the index table covers tgt_len <= 2560")
    # mh_t5_beam_index_init
    init = lambda B, grp, n, origin: lib.mh_t5_beam_index_init(C.byref(cfg), B, grp, n, origin, None)
    refused(init(4, 2, 0, None), b"mh_t5_beam_index_init: null argument")
    refused(init(4, 3, 0, one), b"mh_t5_beam_index_init: 4 rows are not whole groups of 3")
    refused(init(4, 2, 48, one), b"mh_t5_beam_index_init: 48 prefilled positions outside the cache")
    refused(init(4, 2, -1, one), b"mh_t5_beam_index_init: -1 prefilled positions outside the cache")
    refused(init(65, 1, 0, one), b"mh_t5_beam_index_init: batch 65 not in [1, 64]")
    # mh_t5_reorder_index
    two = C.c_void_p(512)
    reorder = lambda B, src, n, a, b: lib.mh_t5_reorder_index(C.byref(cfg), B, src, n, a, b, None)
    refused(reorder(4, None, 1, one, two), b"mh_t5_reorder_index: null argument")
    refused(reorder(4, one, 1, None, two), b"mh_t5_reorder_index: null argument")
    refused(reorder(4, one, 1, one, None), b"mh_t5_reorder_index: null argument")
    refused(reorder(4, one, 1, one, one), b"mh_t5_reorder_index: origin_in and origin_out must be two tables")
    refused(reorder(4, one, 0, one, two), b"mh_t5_reorder_index: 0 positions outside the cache")
    refused(reorder(4, one, 49, one, two), b"mh_t5_reorder_index: 49 positions outside the cache")
    refused(reorder(0, one, 1, one, two), b"mh_t5_reorder_index: batch 0 not in [1, 64]")
    # mh_t5_step_prefill: Bp must be B / kv_group for some whole group size
    pre = lambda Bp, B, P, n, prompt=one, ws=one: lib.mh_t5_step_prefill(C.byref(cfg), C.byref(w), one, Bp, prompt, None, P, n, ws, big,
                                                                        B, None)
    refused(pre(2, 4, 8, 7, prompt=None), b"mh_t5_step_prefill: null argument")
    refused(pre(2, 4, 8, 7, ws=None), b"mh_t5_step_prefill: null argument")
    refused(pre(3, 4, 8, 7), b"mh_t5_step_prefill: 4 rows are not whole groups over 3 prompts")
    refused(pre(0, 4, 8, 7), b"mh_t5_step_prefill: 4 rows are not whole groups over 0 prompts")
    refused(pre(2, 4, 8, 0), b"mh_t5_step_prefill: 0 positions outside the prompt")
    refused(pre(2, 4, 8, 9), b"mh_t5_step_prefill: 9 positions outside the prompt")
    refused(pre(2, 4, 60, 48), b"mh_t5_step_prefill: 48 positions outside the prompt (60 columns) or the cache (tgt_len 48)")
    refused(lib.mh_t5_step_prefill(C.byref(cfg), C.byref(w), one, 2, one, None, 8, 7, one, 16, 4, None),
            b"mh_t5_step_prefill: workspace too small")


# ---- host plumbing over stand-ins -------------------------------------------------------------------------------------------

class _RecordingEngine:
    def __init__(self, dtype):
        self.dtype, self.calls = dtype, []

    def generate(self, audio, prompt, mask, eos, sp, **kw):
        self.calls.append(("generate", kw))
        return dict(tokens=prompt.clone(), n_cols=prompt.shape[1], logits=None)

    def generate_beam(self, audio, prompt, mask, eos, sp, num_beams, **kw):
        self.calls.append(("generate_beam", dict(kw, num_beams=num_beams)))
        return dict(tokens=prompt.clone(), n_cols=prompt.shape[1], logits=None)


def _gk(**over):
    return dict(dict(do_sample=False, num_beams=2, max_length=40, cfg_scale=1.0), **over)


def test_model_generate_hands_the_kwargs_to_generate_beam_and_refuses_bad_ones():
    from mapperatorinator_amd.server import model_generate
    tok = Tokenizer.benchmark_vocab(src_seq_len=251)
    eng = _RecordingEngine(torch.float32)
    model = types.SimpleNamespace(engine=eng, dtype=torch.float32, config=types.SimpleNamespace(max_target_positions=40))
    mk = dict(inputs=torch.zeros(1, 16), decoder_input_ids=torch.tensor([[tok.sos_id]]))
    model_generate(model, tok, mk, _gk(beam_cache="indexed", beam_prefill=True))
    model_generate(model, tok, mk, _gk(beam_cache="indexed"))
    model_generate(model, tok, mk, _gk())
    model_generate(model, tok, mk, _gk(beam_cache="copy"))
    kws = [kw for _, kw in eng.calls]
    assert [n for n, _ in eng.calls] == ["generate_beam"] * 4
    assert (kws[0]["beam_cache"], kws[0]["beam_prefill"]) == ("indexed", True)
    assert (kws[1]["beam_cache"], kws[1]["beam_prefill"]) == ("indexed", False)
    assert "beam_cache" not in kws[2] and "beam_prefill" not in kws[2] and "beam_cache" not in kws[3]   # the default call is unchanged
    eng.calls.clear()
    with pytest.raises(ValueError, match="expected 'copy' or 'indexed'"):
        model_generate(model, tok, mk, _gk(beam_cache="paged"))
    with pytest.raises(ValueError, match="needs cache='indexed'"):
        model_generate(model, tok, mk, _gk(beam_prefill=True))
    with pytest.raises(ValueError, match="needs cache='indexed'"):
        model_generate(model, tok, mk, _gk(beam_cache="copy", beam_prefill=True))
    assert eng.calls == []                               # refused before the engine was asked for anything


def test_modeling_generate_and_generate_beam_pass_the_kwargs_on(monkeypatch):
    from mapperatorinator_amd import beam as beam_mod
    from mapperatorinator_amd.modeling import MapperatorinatorHIP
    from mapperatorinator_amd.t5_engine import T5Engine
    eng = _RecordingEngine(torch.float32)
    cfgm = types.SimpleNamespace(max_target_positions=40, pad_token_id=0, vocab_size=64, eos_token_id=2)
    me = types.SimpleNamespace(engine=eng, dtype=torch.float32, config=cfgm, device=torch.device("cpu"), _row_bias=lambda n, kw: None)
    call = lambda **kw: MapperatorinatorHIP.generate(me, inputs=torch.zeros(1, 16), decoder_input_ids=torch.tensor([[1]]), num_beams=2,
                                                     max_length=40, **kw)
    call(beam_cache="indexed", beam_prefill=True)
    call()
    assert eng.calls[0][1]["beam_cache"] == "indexed" and eng.calls[0][1]["beam_prefill"] is True
    assert "beam_cache" not in eng.calls[1][1]
    with pytest.raises(ValueError, match="expected 'copy' or 'indexed'"):
        call(beam_cache=True)
    with pytest.raises(ValueError, match="needs cache='indexed'"):
        call(beam_prefill=True)
    # T5Engine.generate_beam: refuses before any device work (the object has nothing but a dtype), hands cache / prefill to the search
    bare = types.SimpleNamespace(dtype=torch.float32, device=torch.device("cpu"))
    sp = types.SimpleNamespace(cfg_scale=1.0)
    with pytest.raises(ValueError, match="needs cache='indexed'"):
        T5Engine.generate_beam(bare, torch.zeros(1, 16), torch.tensor([[1]]), None, [], sp, 2, beam_prefill=True)
    with pytest.raises(ValueError, match="expected 'copy' or 'indexed'"):
        T5Engine.generate_beam(bare, torch.zeros(1, 16), torch.tensor([[1]]), None, [], sp, 2, beam_cache="index")
    seen = []
    monkeypatch.setattr(beam_mod, "beam_search", lambda *a, **kw: seen.append(kw) or torch.tensor([[1, 2]]))
    full = types.SimpleNamespace(dtype=torch.float32, device=torch.device("cpu"), _enter=lambda: None, _leave=lambda: None, stream=None,
                                 mel=lambda a: a, encode_mel=lambda m, row_bias=None: m, cross_kv=lambda e: e)
    monkeypatch.setattr(torch.cuda, "stream", lambda s: __import__("contextlib").nullcontext())
    T5Engine.generate_beam(full, torch.zeros(1, 16), torch.tensor([[1]]), None, [], sp, 2, beam_cache="indexed", beam_prefill=True)
    T5Engine.generate_beam(full, torch.zeros(1, 16), torch.tensor([[1]]), None, [], sp, 2)
    assert seen[0]["cache"] == "indexed" and seen[0]["prefill"] is True and "cache" not in seen[1]


@pytest.mark.parametrize("cfg_scale", [1.0, 2.0])
def test_scheduler_hands_the_kwargs_to_the_beam_search(monkeypatch, cfg_scale):
    from mapperatorinator_amd import beam as beam_mod
    from mapperatorinator_amd.scheduler import SequentialWindowScheduler, SongJob
    from test_host_cpu import _StandInEngine
    tok = Tokenizer.benchmark_vocab(src_seq_len=251)
    tgt = 24
    eng = _StandInEngine(tok.vocab_size_out, eos_every=5)
    model = types.SimpleNamespace(engine=eng, config=types.SimpleNamespace(max_target_positions=tgt))
    seen = []

    def fake_beam_search(engine, kv, prompt, mask, eos, sp, nb, **kw):
        seen.append(dict(nb=nb, cache=kw.get("cache"), prefill=kw.get("prefill")))
        G = kv.shape[2]
        return torch.cat([prompt[-G:].long(), torch.full((G, 1), int(sorted(eos)[0]))], 1)
    monkeypatch.setattr(beam_mod, "beam_search", fake_beam_search)

    def job(**extra):
        ask = dict(decoder_input_ids=torch.tensor([[tok.sos_id, 7]]))
        if cfg_scale > 1:
            ask["negative_prompt"] = torch.tensor([[tok.sos_id]])
        return SongJob(frames=torch.randn(2, 64, generator=torch.Generator().manual_seed(1)), prompt_fn=lambda w: dict(ask),
                       on_result=lambda w, row, st: None,
                       generate_kwargs=dict(max_length=tgt, do_sample=False, cfg_scale=cfg_scale, num_beams=2, **extra))
    SequentialWindowScheduler(model, tok, decode_batch=8).run([job(beam_cache="indexed", beam_prefill=True)])
    assert seen and all(s == dict(nb=2, cache="indexed", prefill=True) for s in seen)
    seen.clear()
    SequentialWindowScheduler(model, tok, decode_batch=8).run([job()])
    assert seen and all(s["cache"] is None and s["prefill"] is None for s in seen)         # the default call is unchanged
    with pytest.raises(ValueError, match="needs cache='indexed'"):
        SequentialWindowScheduler(model, tok, decode_batch=8).run([job(beam_prefill=True)])


class _StandInLib:
    """Counts the library calls of a beam search; the step entries write logits that prefer id 5, then EOS."""

    def __init__(self, V, tgt):
        self.calls, self.V, self.tgt, self.logits = [], V, tgt, None

    def __getattr__(self, name):
        if not name.startswith("mh_"):
            raise AttributeError(name)

        def f(*a):
            self.calls.append(name)
            if name in ("mh_t5_decode_workspace_bytes", "mh_t5_reorder_cache_scratch_bytes"):
                return 64
            if name == "mh_t5_beam_index_bytes":
                return int(a[1]) * self.tgt
            if name == "mh_beam_step_path":
                return 0                                   # -> the torch-op bookkeeping, which runs on any device
            if name in ("mh_t5_step", "mh_t5_step_fp8", "mh_t5_step_indexed"):
                self.logits.zero_()
                self.logits[:, 2 if self.calls.count(name) > 3 else 5] = 4.0
            return 0
        return f


@pytest.mark.parametrize("cache,prefill", [("copy", False), ("indexed", False), ("indexed", True)])
def test_the_indexed_route_calls_none_of_the_copy_routes_entries(monkeypatch, cache, prefill):
    """`beam_search` (torch-op bookkeeping, CPU tensors) over a stand-in library: which entries each route calls, and that the
    indexed one allocates no reorder scratch."""
    from mapperatorinator_amd import beam as beam_mod
    V, tgt, P = 16, 12, 3
    lib = _StandInLib(V, tgt)
    monkeypatch.setattr(_lib, "load", lambda: lib)
    monkeypatch.setattr(_lib, "check", lambda rc, what="": None)
    monkeypatch.setattr(torch.cuda, "stream", lambda s: __import__("contextlib").nullcontext())
    real_empty = torch.empty

    def empty(*a, **kw):
        t = real_empty(*a, **kw)
        if kw.get("dtype") is torch.float32 and tuple(t.shape) == (4, V):
            lib.logits = t                                 # the search's logits buffer: the stand-in steps write into it
        return t
    monkeypatch.setattr(torch, "empty", empty)
    cfg = _cfg(tgt=tgt)
    eng = types.SimpleNamespace(device=torch.device("cpu"), lib=lib, dtype=torch.float32, stream=None, _s=lambda: None,
                                _enter=lambda: None, _leave=lambda: None, synchronize=lambda: None,
                                packed=types.SimpleNamespace(cfg=cfg, w=_lib.MhT5Weights(), vocab_out=V, tgt_len=tgt))
    sp = _lib.MhSampling()
    sp.max_length, sp.cfg_scale, sp.temperature, sp.pad_id = tgt, 1.0, 1.0, 0
    kv = torch.zeros(2, 2, 2, 2, 4, 64)
    out = beam_mod.beam_search(eng, kv, torch.tensor([[1, 3, 4], [1, 6, 7]]), None, [2], sp, 2, use_kernel=False, cache=cache,
                               prefill=prefill)
    assert out.shape[0] == 2 and out.shape[1] > P
    names = set(lib.calls)
    if cache == "copy":
        assert {"mh_t5_step", "mh_t5_reorder_cache", "mh_t5_reorder_cache_scratch_bytes"} <= names
        assert not names & set(NEW)
    else:
        assert not names & {"mh_t5_step", "mh_t5_step_fp8", "mh_t5_reorder_cache", "mh_t5_reorder_cache_scratch_bytes"}
        assert {"mh_t5_step_indexed", "mh_t5_reorder_index", "mh_t5_beam_index_bytes", "mh_t5_beam_index_init"} <= names
        assert ("mh_t5_step_prefill" in names) == prefill
        n_steps = lib.calls.count("mh_t5_step_indexed")
        n_search = lib.calls.count("mh_t5_reorder_index")    # one reorder per searched column
        assert n_search >= out.shape[1] - P
        assert n_steps == n_search + (0 if prefill else P - 1)  # the prompt columns cost one call in all, not one step each
    with pytest.raises(ValueError, match="expected 'copy' or 'indexed'"):
        beam_mod.beam_search(eng, kv, torch.tensor([[1, 3, 4]]), None, [2], sp, 2, cache="paged")
    with pytest.raises(ValueError, match="needs cache='indexed'"):
        beam_mod.beam_search(eng, kv, torch.tensor([[1, 3, 4]]), None, [2], sp, 2, prefill=True)
