"""not gpu: the e4m3 self-attention cache under the beam search's index table (`self_kv_fp8` with `beam_cache="indexed"`) on the host
side -- mh_t5_step_indexed_skv8 and mh_t5_self_kv_fp8_fill are declared, bound and exported at ABI 11; each refuses bad arguments
with its message before any launch; the flag reaches `generate_beam` as `beam_self_kv_fp8` from `model_generate`,
`MapperatorinatorHIP.generate` and the scheduler; the copy cache and fp32 storage are refused before the engine is asked for anything;
over a stand-in library the search calls the new step entry, the fill exactly once right after the prefill, and none of the others."""
import ctypes as C
import os
import re
import types

import pytest
import torch

from conftest import ROOT
from mapperatorinator_amd import Tokenizer, _lib

NEW = ("mh_t5_step_indexed_skv8", "mh_t5_self_kv_fp8_fill")
BF16 = 1


def _cfg(d_model=128, dtype=BF16, tgt=48):
    """the config of tests/test_beam_cache_cpu.py: tiny dims, tgt_len 48; bf16 storage unless told otherwise"""
    cfg = _lib.MhT5Config(d_model, 64, 256, 2, 2, 2, 10, 10, 388, 416, 251, tgt, dtype, 1e-6)
    assert cfg.tgt_len == tgt and cfg.dtype == dtype
    return cfg


def test_the_two_entries_are_declared_bound_and_exported_at_abi_11():
    hdr = open(os.path.join(ROOT, "include", "mapperhip.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), f"{name} is not declared in include/mapperhip.h"
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert re.search(r"#define\s+MH_ABI_VERSION\s+11\b", hdr)
    assert _lib.ABI_VERSION == 11 and lib.mh_abi_version() == 11
    # mh_t5_step_indexed's arguments with the shadow in front of the stream
    idx = _lib.SYMBOLS["mh_t5_step_indexed"][1]
    assert list(_lib.SYMBOLS["mh_t5_step_indexed_skv8"][1]) == list(idx[:-1]) + [C.c_void_p, idx[-1]]
    assert _lib.SYMBOLS["mh_t5_step_indexed_skv8"][0] is C.c_int and _lib.SYMBOLS["mh_t5_self_kv_fp8_fill"][0] is C.c_int
    assert list(_lib.SYMBOLS["mh_t5_self_kv_fp8_fill"][1]) == [C.POINTER(_lib.MhT5Config), C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                               C.c_int64, C.c_void_p, C.c_void_p]
    # the two "not built" sentences of the header name the new entry, and the contract is written down
    assert "mh_t5_step_indexed_skv8" in hdr[hdr.index("Not built here"): hdr.index("Not built here") + 700]
    assert "No e4m3 self-cache form" not in hdr
    at = hdr.index("int mh_t5_step_indexed_skv8")
    contract = hdr[at - 4000: at]
    for phrase in ("origin[b][j]", "storage precision", "shadow row b", "mh_t5_step_prefill", "batch-invariant", "still have no shadow form"):
        assert phrase in contract, phrase


def test_both_entries_refuse_bad_arguments_before_any_launch():
    """Non-NULL pointers below are the address 256: a launch would fault on it, a refusal never follows it."""
    lib = _lib.load()
    cfg, w, one = _cfg(), _lib.MhT5Weights(), C.c_void_p(256)
    big = 1 << 40

    def refused(rc, msg):
        assert rc == -1, rc
        err = lib.mh_last_error()
        assert msg in err, (msg, err)

    def step(c=cfg, B=4, grp=2, pos=0, kv8=None, origin=one, shadow=one, ids=one, ws=one, ws_bytes=big):
        return lib.mh_t5_step_indexed_skv8(C.byref(c), C.byref(w), one, kv8, B, grp, ids, pos, None, 1, one, ws, ws_bytes, origin, shadow, None)
    refused(step(shadow=None), b"mh_t5_step_indexed_skv8: null argument")
    refused(step(origin=None), b"mh_t5_step_indexed_skv8: null argument")
    refused(step(ids=None), b"mh_t5_step_indexed_skv8: null argument")
    refused(step(ws=None), b"mh_t5_step_indexed_skv8: null argument")
    refused(step(c=_cfg(dtype=0)), b"mh_t5_step_indexed_skv8: the e4m3 self-attention cache needs bf16 storage")
    refused(step(c=_cfg(dtype=0), kv8=one), b"needs bf16 storage")
    refused(step(c=_cfg(tgt=2561)), b"mh_t5_step_indexed_skv8: the index table covers tgt_len <= 2560")
    refused(step(B=65, grp=1), b"mh_t5_step_indexed_skv8: batch 65 not in [1, 64]")
    refused(step(B=0, grp=1), b"mh_t5_step_indexed_skv8: batch 0 not in [1, 64]")
    refused(step(grp=3), b"mh_t5_step_indexed_skv8: 4 rows are not whole groups of 3")
    refused(step(pos=48), b"mh_t5_step_indexed_skv8: position 48 outside the cache")
    refused(step(pos=-1), b"mh_t5_step_indexed_skv8: position -1 outside the cache")
    refused(step(ws_bytes=16), b"mh_t5_step_indexed_skv8: workspace too small")
    refused(step(c=_cfg(d_model=96)), b"d_model")

    def fill(c=cfg, B=4, n_rows=2, n_pos=7, ws=one, ws_bytes=big, shadow=one):
        return lib.mh_t5_self_kv_fp8_fill(C.byref(c), B, n_rows, n_pos, ws, ws_bytes, shadow, None)
    refused(fill(ws=None), b"mh_t5_self_kv_fp8_fill: null argument")
    refused(fill(shadow=None), b"mh_t5_self_kv_fp8_fill: null argument")
    refused(fill(c=_cfg(dtype=0)), b"mh_t5_self_kv_fp8_fill: the e4m3 self-attention cache needs bf16 storage")
    refused(fill(c=_cfg(tgt=2561)), b"mh_t5_self_kv_fp8_fill: the index table covers tgt_len <= 2560")
    refused(fill(B=65, n_rows=1), b"mh_t5_self_kv_fp8_fill: batch 65 not in [1, 64]")
    refused(fill(B=0, n_rows=1), b"mh_t5_self_kv_fp8_fill: batch 0 not in [1, 64]")
    refused(fill(n_rows=0), b"mh_t5_self_kv_fp8_fill: 0 rows not in [1, 4]")
    refused(fill(n_rows=5), b"mh_t5_self_kv_fp8_fill: 5 rows not in [1, 4]")
    refused(fill(n_rows=3), b"mh_t5_self_kv_fp8_fill: 4 rows are not whole groups over 3 prompts")
    refused(fill(n_pos=0), b"mh_t5_self_kv_fp8_fill: 0 positions outside the cache")
    refused(fill(n_pos=48), b"mh_t5_self_kv_fp8_fill: 48 positions outside the cache (tgt_len 48)")
    refused(fill(ws_bytes=16), b"mh_t5_self_kv_fp8_fill: workspace too small")


def test_the_24_new_instantiations_are_built_without_scratch():
    """dec_self_attn_qkv_kernel<bf16, KC, WH, LN, F8 = true, IDX = true>, KC 1 .. 8 x {T5, Whisper family, + LayerNorm}: read from the
    built library's metadata (tools/check_kernel_resources.py) -- no scratch, no spills, inside the 128 registers of a 16-wave
    workgroup at 4 waves per SIMD, the LDS of the bf16 IDX form; and tools/device_code_diff.py --kernel on one build is clean."""
    import importlib.util
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        mods = {}
        for name in ("check_kernel_resources", "device_code_diff"):
            spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
            mods[name] = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mods[name])
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    ckr, dcd = mods["check_kernel_resources"], mods["device_code_diff"]
    lib = _lib.lib_path()
    rows = [k for elf in ckr.code_objects(lib) for k in ckr.kernels_of(elf) if "dec_self_attn_qkv_kernel" in k[".symbol"]]
    names = ckr.demangle([k[".symbol"].removesuffix(".kd") for k in rows])
    new = {nm.split("(")[0].split("<")[1]: k for nm, k in zip(names, rows) if nm.split("(")[0].endswith("true, true>")}
    want = {f"unsigned short, {kc}, {wh}, {ln}, true, true>" for kc in range(1, 9) for wh, ln in (("false", "false"), ("true", "false"), ("true", "true"))}
    assert set(new) == want, sorted(set(new) ^ want)
    idx_lds = {int(k[".group_segment_fixed_size"]) for nm, k in zip(names, rows) if nm.split("(")[0].endswith("false, true>")}
    for args, k in new.items():
        assert int(k.get(".private_segment_fixed_size", 0)) == 0 and int(k.get(".vgpr_spill_count", 0)) == 0, args
        assert int(k.get(".sgpr_spill_count", 0)) == 0 and int(k[".vgpr_count"]) <= 128, (args, k[".vgpr_count"])
        assert {int(k[".group_segment_fixed_size"])} == idx_lds, (args, k[".group_segment_fixed_size"], idx_lds)
    assert dcd.main(["--kernel", "dec_self_attn_qkv_kernel", lib, lib]) == 0
    assert len(dcd.kernel_texts(lib, "dec_self_attn_qkv_kernel")) == len(rows) == 144


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


def test_the_refusal_passes_beams_over_the_indexed_cache_only():
    from mapperatorinator_amd.t5_engine import require_bf16_for_self_kv_fp8
    require_bf16_for_self_kv_fp8(torch.bfloat16)
    require_bf16_for_self_kv_fp8(torch.bfloat16, 1, "copy")
    require_bf16_for_self_kv_fp8(torch.bfloat16, 4, "indexed")
    for args in ((torch.bfloat16, 2), (torch.bfloat16, 2, "copy")):
        with pytest.raises(ValueError, match="not built for beam search") as e:
            require_bf16_for_self_kv_fp8(*args)
        assert "beam_cache='indexed'" in str(e.value)                   # ... and names the way out
    for nb, cache in ((1, "copy"), (2, "indexed")):
        with pytest.raises(ValueError, match="self_kv_fp8 needs bf16 storage"):
            require_bf16_for_self_kv_fp8(torch.float32, nb, cache)


def test_model_generate_hands_the_flag_to_generate_beam_and_refuses_the_copy_cache_and_fp32():
    from mapperatorinator_amd.server import model_generate
    tok = Tokenizer.benchmark_vocab(src_seq_len=251)
    eng = _RecordingEngine(torch.bfloat16)
    model = types.SimpleNamespace(engine=eng, dtype=torch.bfloat16, config=types.SimpleNamespace(max_target_positions=40))
    mk = dict(inputs=torch.zeros(1, 16), decoder_input_ids=torch.tensor([[tok.sos_id]]))
    model_generate(model, tok, mk, _gk(beam_cache="indexed", self_kv_fp8=True))
    model_generate(model, tok, mk, _gk(beam_cache="indexed", beam_prefill=True, self_kv_fp8=True, cross_kv_fp8=True))
    model_generate(model, tok, mk, _gk(beam_cache="indexed"))
    model_generate(model, tok, mk, _gk())
    model_generate(model, tok, mk, _gk(num_beams=1, self_kv_fp8=True))
    kws = [kw for _, kw in eng.calls]
    assert [n for n, _ in eng.calls] == ["generate_beam"] * 4 + ["generate"]
    assert kws[0]["beam_self_kv_fp8"] is True and kws[0]["beam_cache"] == "indexed" and "self_kv_fp8" not in kws[0]
    assert kws[1]["beam_self_kv_fp8"] is True and kws[1]["beam_prefill"] is True and kws[1]["cross_kv_fp8"] is True
    assert "beam_self_kv_fp8" not in kws[2] and "beam_self_kv_fp8" not in kws[3] and "self_kv_fp8" not in kws[3]   # default calls
    assert kws[4]["self_kv_fp8"] is True and "beam_self_kv_fp8" not in kws[4]                                       # the greedy route
    eng.calls.clear()
    with pytest.raises(ValueError, match="not built for beam search"):
        model_generate(model, tok, mk, _gk(self_kv_fp8=True))
    with pytest.raises(ValueError, match="not built for beam search"):
        model_generate(model, tok, mk, _gk(beam_cache="copy", self_kv_fp8=True))
    model.dtype = eng.dtype = torch.float32
    with pytest.raises(ValueError, match="self_kv_fp8 needs bf16 storage"):
        model_generate(model, tok, mk, _gk(beam_cache="indexed", self_kv_fp8=True))
    assert eng.calls == []                               # refused before the engine was asked for anything


def test_modeling_generate_and_generate_beam_pass_the_flag_on(monkeypatch):
    import inspect
    from mapperatorinator_amd import beam as beam_mod
    from mapperatorinator_amd.modeling import MapperatorinatorHIP
    from mapperatorinator_amd.t5_engine import T5Engine
    eng = _RecordingEngine(torch.bfloat16)
    cfgm = types.SimpleNamespace(max_target_positions=40, pad_token_id=0, vocab_size=64, eos_token_id=2)
    me = types.SimpleNamespace(engine=eng, dtype=torch.bfloat16, config=cfgm, device=torch.device("cpu"), _row_bias=lambda n, kw: None)
    call = lambda **kw: MapperatorinatorHIP.generate(me, inputs=torch.zeros(1, 16), decoder_input_ids=torch.tensor([[1]]), num_beams=2,
                                                     max_length=40, **kw)
    call(beam_cache="indexed", self_kv_fp8=True)
    call(beam_cache="indexed")
    call()
    assert eng.calls[0][1]["beam_self_kv_fp8"] is True and eng.calls[0][1]["beam_cache"] == "indexed"
    assert "beam_self_kv_fp8" not in eng.calls[1][1] and "beam_self_kv_fp8" not in eng.calls[2][1]
    eng.calls.clear()
    with pytest.raises(ValueError, match="not built for beam search"):
        call(self_kv_fp8=True)
    me.dtype = torch.float32
    with pytest.raises(ValueError, match="self_kv_fp8 needs bf16 storage"):
        call(beam_cache="indexed", self_kv_fp8=True)
    assert eng.calls == []
    # T5Engine.generate_beam: the deliberate name, refusals before any device work (the object has nothing but a dtype)
    params = inspect.signature(T5Engine.generate_beam).parameters
    assert "beam_self_kv_fp8" in params and params["beam_self_kv_fp8"].default is False and "self_kv_fp8" not in params
    sp = types.SimpleNamespace(cfg_scale=1.0)
    bare = types.SimpleNamespace(dtype=torch.bfloat16, device=torch.device("cpu"))
    args = (torch.zeros(1, 16), torch.tensor([[1]]), None, [], sp, 2)
    with pytest.raises(ValueError, match="not built for beam search"):
        T5Engine.generate_beam(bare, *args, beam_self_kv_fp8=True)
    bare.dtype = torch.float32
    with pytest.raises(ValueError, match="self_kv_fp8 needs bf16 storage"):
        T5Engine.generate_beam(bare, *args, beam_cache="indexed", beam_self_kv_fp8=True)
    seen = []
    monkeypatch.setattr(beam_mod, "beam_search", lambda *a, **kw: seen.append(kw) or torch.tensor([[1, 2]]))
    full = types.SimpleNamespace(dtype=torch.bfloat16, device=torch.device("cpu"), _enter=lambda: None, _leave=lambda: None, stream=None,
                                 mel=lambda a: a, encode_mel=lambda m, row_bias=None: m, cross_kv=lambda e: e)
    monkeypatch.setattr(torch.cuda, "stream", lambda s: __import__("contextlib").nullcontext())
    T5Engine.generate_beam(full, *args, beam_cache="indexed", beam_prefill=True, beam_self_kv_fp8=True)
    T5Engine.generate_beam(full, *args, beam_cache="indexed")
    T5Engine.generate_beam(full, *args)
    assert seen[0]["self_kv_fp8"] is True and seen[0]["cache"] == "indexed" and seen[0]["prefill"] is True
    assert "self_kv_fp8" not in seen[1] and "self_kv_fp8" not in seen[2]


@pytest.mark.parametrize("cfg_scale", [1.0, 2.0])
def test_scheduler_hands_the_flag_to_the_beam_search_and_refuses_before_encoding(monkeypatch, cfg_scale):
    from mapperatorinator_amd import beam as beam_mod
    from mapperatorinator_amd.scheduler import SequentialWindowScheduler, SongJob
    from test_host_cpu import _StandInEngine
    tok = Tokenizer.benchmark_vocab(src_seq_len=251)
    tgt = 24
    eng = _StandInEngine(tok.vocab_size_out, eos_every=5)
    eng.dtype = torch.bfloat16
    model = types.SimpleNamespace(engine=eng, config=types.SimpleNamespace(max_target_positions=tgt))
    seen = []

    def fake_beam_search(engine, kv, prompt, mask, eos, sp, nb, **kw):
        seen.append(dict(nb=nb, cache=kw.get("cache"), prefill=kw.get("prefill"), self_kv_fp8=kw.get("self_kv_fp8")))
        G = kv.shape[2]
        return torch.cat([prompt[-G:].long(), torch.full((G, 1), int(sorted(eos)[0]))], 1)
    monkeypatch.setattr(beam_mod, "beam_search", fake_beam_search)
    encoded = []
    real_encode = SequentialWindowScheduler.encode_all
    monkeypatch.setattr(SequentialWindowScheduler, "encode_all", lambda self, jobs: encoded.append(1) or real_encode(self, jobs))

    def job(**extra):
        ask = dict(decoder_input_ids=torch.tensor([[tok.sos_id, 7]]))
        if cfg_scale > 1:
            ask["negative_prompt"] = torch.tensor([[tok.sos_id]])
        return SongJob(frames=torch.randn(2, 64, generator=torch.Generator().manual_seed(1)), prompt_fn=lambda w: dict(ask),
                       on_result=lambda w, row, st: None,
                       generate_kwargs=dict(max_length=tgt, do_sample=False, cfg_scale=cfg_scale, num_beams=2, **extra))
    SequentialWindowScheduler(model, tok, decode_batch=8).run([job(beam_cache="indexed", beam_prefill=True, self_kv_fp8=True)])
    assert seen and all(s == dict(nb=2, cache="indexed", prefill=True, self_kv_fp8=True) for s in seen)
    seen.clear()
    SequentialWindowScheduler(model, tok, decode_batch=8).run([job(beam_cache="indexed")])
    SequentialWindowScheduler(model, tok, decode_batch=8).run([job()])
    assert seen and all(s["self_kv_fp8"] is None for s in seen)                            # the default calls carry no new keyword
    n_encoded = len(encoded)
    assert n_encoded == 3
    with pytest.raises(ValueError, match="not built for beam search"):
        SequentialWindowScheduler(model, tok, decode_batch=8).run([job(self_kv_fp8=True)])
    with pytest.raises(ValueError, match="not built for beam search"):
        SequentialWindowScheduler(model, tok, decode_batch=8).run([job(beam_cache="copy", self_kv_fp8=True)])
    eng.dtype = torch.float32
    with pytest.raises(ValueError, match="self_kv_fp8 needs bf16 storage"):
        SequentialWindowScheduler(model, tok, decode_batch=8).run([job(beam_cache="indexed", self_kv_fp8=True)])
    assert len(encoded) == n_encoded                                                         # refused before anything was encoded


class _StandInLib:
    """Records the library calls of a beam search in order; the step entries write logits that prefer id 5, then EOS."""
    STEPS = ("mh_t5_step", "mh_t5_step_fp8", "mh_t5_step_indexed", "mh_t5_step_indexed_skv8")

    def __init__(self, V, tgt):
        self.calls, self.args, self.V, self.tgt, self.logits = [], [], V, tgt, None

    def __getattr__(self, name):
        if not name.startswith("mh_"):
            raise AttributeError(name)

        def f(*a):
            self.calls.append(name)
            self.args.append(a)
            if name in ("mh_t5_decode_workspace_bytes", "mh_t5_reorder_cache_scratch_bytes"):
                return 64
            if name == "mh_t5_beam_index_bytes":
                return int(a[1]) * self.tgt
            if name == "mh_t5_self_kv_fp8_bytes":
                return int(a[1]) * 1000
            if name == "mh_beam_step_path":
                return 0                                   # -> the torch-op bookkeeping, which runs on any device
            if name in self.STEPS:
                self.logits.zero_()
                self.logits[:, 2 if self.calls.count(name) > 3 else 5] = 4.0
            return 0
        return f


def _stand_in_search(monkeypatch, dtype=torch.bfloat16, rows=4, **kw):
    from mapperatorinator_amd import beam as beam_mod
    V, tgt = 16, 12
    lib = _StandInLib(V, tgt)
    monkeypatch.setattr(_lib, "load", lambda: lib)
    monkeypatch.setattr(_lib, "check", lambda rc, what="": None)
    monkeypatch.setattr(torch.cuda, "stream", lambda s: __import__("contextlib").nullcontext())
    real_empty = torch.empty

    def empty(*a, **k):
        t = real_empty(*a, **k)
        if k.get("dtype") is torch.float32 and tuple(t.shape) == (rows, V):
            lib.logits = t                                 # the search's logits buffer: the stand-in steps write into it
        return t
    monkeypatch.setattr(torch, "empty", empty)
    asked = []

    def workspace(kind, nbytes):
        asked.append((kind, int(nbytes)))
        return real_empty(int(nbytes), dtype=torch.uint8)
    eng = types.SimpleNamespace(device=torch.device("cpu"), lib=lib, dtype=dtype, stream=None, _s=lambda: None,
                                _enter=lambda: None, _leave=lambda: None, synchronize=lambda: None, _workspace=workspace,
                                packed=types.SimpleNamespace(cfg=_cfg(tgt=tgt), w=_lib.MhT5Weights(), vocab_out=V, tgt_len=tgt))
    sp = _lib.MhSampling()
    sp.max_length, sp.cfg_scale, sp.temperature, sp.pad_id = tgt, 1.0, 1.0, 0
    kv = torch.zeros(2, 2, 2, 2, 4, 64)
    run = lambda **k2: beam_mod.beam_search(eng, kv, torch.tensor([[1, 3, 4], [1, 6, 7]]), None, [2], sp, 2, use_kernel=False, **dict(kw, **k2))
    return lib, eng, asked, run


@pytest.mark.parametrize("prefill", [False, True], ids=["indexed", "indexed+prefill"])
def test_the_search_calls_the_new_entries_and_none_of_the_others(monkeypatch, prefill):
    """`beam_search` (torch-op bookkeeping, CPU tensors) over a stand-in library with self_kv_fp8=True: every step is
    mh_t5_step_indexed_skv8 over the engine's "skv8" workspace sized for the decoded rows; with a prefill the fill runs exactly once,
    right behind mh_t5_step_prefill, with n_rows = the prompts and the prefill's n_pos."""
    P = 3
    lib, eng, asked, run = _stand_in_search(monkeypatch, cache="indexed", prefill=prefill, self_kv_fp8=True)
    out = run()
    assert out.shape[0] == 2 and out.shape[1] > P
    names = set(lib.calls)
    assert not names & {"mh_t5_step_indexed", "mh_t5_step", "mh_t5_step_fp8", "mh_t5_reorder_cache", "mh_t5_reorder_cache_scratch_bytes"}
    assert {"mh_t5_step_indexed_skv8", "mh_t5_reorder_index", "mh_t5_beam_index_init", "mh_t5_self_kv_fp8_bytes"} <= names
    assert asked == [("skv8", 4 * 1000)]                                     # 2 chunks x 2 beams: the rows the decoder runs
    n_steps, n_search = lib.calls.count("mh_t5_step_indexed_skv8"), lib.calls.count("mh_t5_reorder_index")
    assert n_search >= out.shape[1] - P and n_steps == n_search + (0 if prefill else P - 1)
    assert lib.calls.count("mh_t5_self_kv_fp8_fill") == (1 if prefill else 0)
    assert lib.calls.count("mh_t5_step_prefill") == (1 if prefill else 0)
    if prefill:
        at = lib.calls.index("mh_t5_step_prefill")
        assert lib.calls[at + 1] == "mh_t5_self_kv_fp8_fill" and lib.calls[at + 2] == "mh_t5_beam_index_init"
        fill = lib.args[at + 1]
        assert (fill[1], fill[2], fill[3]) == (4, 2, P - 1)                  # B, n_rows = the prompts, n_pos


def test_the_search_without_the_flag_is_unchanged_and_bad_combinations_raise(monkeypatch):
    lib, eng, asked, run = _stand_in_search(monkeypatch, cache="indexed", prefill=True)
    run()
    assert "mh_t5_step_indexed" in lib.calls and not set(lib.calls) & {"mh_t5_step_indexed_skv8", "mh_t5_self_kv_fp8_fill",
                                                                      "mh_t5_self_kv_fp8_bytes"}
    assert asked == []
    n = len(lib.calls)
    with pytest.raises(ValueError, match="not built for beam search"):
        run(cache="copy", prefill=False, self_kv_fp8=True)
    eng.dtype = torch.float32
    with pytest.raises(ValueError, match="self_kv_fp8 needs bf16 storage"):
        run(self_kv_fp8=True)
    assert len(lib.calls) == n and asked == []                               # refused before the library was asked for anything


def test_guidance_doubles_the_rows_of_the_shadow(monkeypatch):
    lib, eng, asked, run = _stand_in_search(monkeypatch, rows=8, cache="indexed", self_kv_fp8=True)
    from mapperatorinator_amd import beam as beam_mod
    sp = _lib.MhSampling()
    sp.max_length, sp.cfg_scale, sp.temperature, sp.pad_id = 12, 2.0, 1.0, 0
    prompt = torch.tensor([[1, 9, 9], [1, 9, 9], [1, 3, 4], [1, 6, 7]])      # [negative rows | prompt rows]
    beam_mod.beam_search(eng, torch.zeros(2, 2, 2, 2, 4, 64), prompt, None, [2], sp, 2, use_kernel=False, cache="indexed", self_kv_fp8=True)
    assert asked == [("skv8", 8 * 1000)] and "mh_t5_step_indexed_skv8" in lib.calls and "mh_t5_step_indexed" not in lib.calls
