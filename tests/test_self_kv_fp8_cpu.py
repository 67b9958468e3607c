"""not gpu: the e4m3 self-attention K/V cache (`self_kv_fp8`) on the host side -- the new symbols are declared, bound and exported at
ABI 11, null / fp32 arguments are refused by the library with a message, the bytes formula holds, the hosts refuse fp32 storage
and beams before anything is encoded, the flag reaches the engine through every public seam, and the CPU counterpart of the mode
(mh_testing.kv_fp8: a hook on the oracles' `decoder_step`) does what it says.  Last, for every input of
tests/test_gpu_self_kv_fp8.py: the hooked oracle's own share of steps whose top-2 gap is <= 0.25 is at most 10 % -- the share the GPU
gate ("no top-1 mismatch beyond the gap") leaves out."""
import ctypes as C
import os
import re
import types

import pytest
import torch

from conftest import ROOT
from mapperatorinator_amd import Tokenizer, _lib
from mh_testing import kv_fp8

NEW = ("mh_t5_self_kv_fp8_bytes", "mh_t5_generate_skv8", "mh_quantize_kv_rows", "mh_t5_decode_self_cache")


def _cfg(dtype):    # d 128, 2 heads, 2 + 2 layers, src 251, tgt 48
    return _lib.MhT5Config(128, 64, 256, 2, 2, 2, 10, 10, 388, 416, 251, 48, dtype, 1e-6)


def test_new_symbols_are_declared_bound_and_exported_at_abi_11():
    hdr = open(os.path.join(ROOT, "include", "mapperhip.h")).read()
    assert re.search(r"#define\s+MH_ABI_VERSION\s+11\b", hdr)
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\b(int|int64_t)\s+%s\s*\(" % name, hdr), f"{name} is not declared in include/mapperhip.h"
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    # mh_t5_generate's argument list plus the shadow
    assert list(_lib.SYMBOLS["mh_t5_generate_skv8"][1]) == list(_lib.SYMBOLS["mh_t5_generate"][1]) + [C.c_void_p]
    assert _lib.SYMBOLS["mh_t5_self_kv_fp8_bytes"][0] is C.c_int64
    assert _lib.ABI_VERSION == 11 and lib.mh_abi_version() == 11
    # no struct changed layout (load() compares every struct's size with the library's; MhSampling is where a flag would have gone)
    assert C.sizeof(_lib.MhSampling) == lib.mh_struct_size(3)


def test_library_refuses_null_and_fp32_with_a_message():
    lib = _lib.load()
    one, w, sp = C.c_void_p(256), _lib.MhT5Weights(), _lib.MhSampling()
    bf16, f32 = _cfg(_lib.MH_BF16), _cfg(_lib.MH_F32)
    args = (C.byref(w), one, 1, one, None, 1, one, C.byref(sp), one, one, None, None, one, 1 << 40, 16, one)
    assert lib.mh_t5_generate_skv8(C.byref(bf16), *args, None) == -1                 # the shadow is not optional
    assert b"mh_t5_generate_skv8: null argument" in lib.mh_last_error()
    assert lib.mh_t5_generate_skv8(C.byref(f32), *args, one) == -1                   # fp32 storage: nothing is followed
    assert b"bf16 storage" in lib.mh_last_error()
    # an argument error found by the shared body names the entry the caller used (stream NULL: checked before anything is followed)
    assert lib.mh_t5_generate_skv8(C.byref(bf16), *args[:-1], None, one) == -1
    assert b"mh_t5_generate_skv8: needs a non-default stream" in lib.mh_last_error()
    assert lib.mh_t5_generate(C.byref(bf16), *args[:-1], None) == -1
    assert b"mh_t5_generate: needs a non-default stream" in lib.mh_last_error()
    bad = _lib.MhT5Config(96, 64, 256, 2, 2, 2, 10, 10, 388, 416, 251, 48, 1, 1e-6)  # d_model no multiple of 128
    assert lib.mh_t5_generate_skv8(C.byref(bad), *args, one) == -1
    assert b"d_model" in lib.mh_last_error()
    assert lib.mh_t5_self_kv_fp8_bytes(C.byref(f32), 4) == -1
    assert b"bf16 storage" in lib.mh_last_error()
    assert lib.mh_t5_self_kv_fp8_bytes(None, 4) == -1 and lib.mh_t5_self_kv_fp8_bytes(C.byref(bf16), 0) == -1
    assert lib.mh_quantize_kv_rows(None, 4, one, one, None) == -1
    assert b"mh_quantize_kv_rows: null argument" in lib.mh_last_error()
    assert lib.mh_quantize_kv_rows(one, 0, one, one, None) == -1
    assert b"n_rows" in lib.mh_last_error()
    k, v = C.c_void_p(), C.c_void_p()
    assert lib.mh_t5_decode_self_cache(C.byref(bf16), 2, None, C.byref(k), C.byref(v)) == -1
    assert b"mh_t5_decode_self_cache: null argument" in lib.mh_last_error()


@pytest.mark.parametrize("B", [1, 3, 32])
def test_bytes_formula_and_cache_pointers(B):
    lib = _lib.load()
    cfg = _cfg(_lib.MH_BF16)
    rows = cfg.n_dec_layers * 2 * B * cfg.n_heads * cfg.tgt_len
    up = lambda n: (n + 255) // 256 * 256
    assert lib.mh_t5_self_kv_fp8_bytes(C.byref(cfg), B) == up(rows * 64) + up(rows * 4)
    # 0.53 x the bf16 cache (68 bytes per row beside 128)
    assert abs(lib.mh_t5_self_kv_fp8_bytes(C.byref(cfg), B) / (rows * 128) - 0.53) < 0.01
    # the bf16 caches inside a decode workspace: two slabs of [n_dec][B][H][tgt][64] bf16, one behind the other, inside the workspace
    k, v = C.c_void_p(), C.c_void_p()
    base = 1 << 20
    assert lib.mh_t5_decode_self_cache(C.byref(cfg), B, C.c_void_p(base), C.byref(k), C.byref(v)) == 0
    assert base <= k.value and v.value - k.value == rows * 64 and k.value % 256 == 0
    assert v.value + rows * 64 <= base + lib.mh_t5_decode_workspace_bytes(C.byref(cfg), B)


class _RecordingEngine:
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


def test_model_generate_passes_the_flag_and_refuses_fp32_and_beams():
    from mapperatorinator_amd.server import model_generate
    tok = Tokenizer.benchmark_vocab(src_seq_len=251)
    mk = dict(inputs=torch.zeros(1, 16), decoder_input_ids=torch.tensor([[tok.sos_id]]))
    gk = dict(do_sample=False, num_beams=1, max_length=40, cfg_scale=1.0, self_kv_fp8=True)
    model, eng = _stub_model(torch.bfloat16)
    model_generate(model, tok, mk, gk)
    (name, kw), = eng.calls
    assert name == "generate" and kw["self_kv_fp8"] is True and kw["cross_kv_fp8"] is False
    eng.calls.clear()
    model_generate(model, tok, mk, dict(gk, cross_kv_fp8=True))                      # the whole fp8 K/V cache
    assert eng.calls[0][1]["self_kv_fp8"] is True and eng.calls[0][1]["cross_kv_fp8"] is True
    eng.calls.clear()
    model_generate(model, tok, mk, dict(gk, self_kv_fp8=False))
    assert "self_kv_fp8" not in eng.calls[0][1]                                      # the default call is the parent's
    eng.calls.clear()
    with pytest.raises(ValueError, match="not built for beam search"):
        model_generate(model, tok, mk, dict(gk, num_beams=2))
    assert eng.calls == []
    model32, eng32 = _stub_model(torch.float32)
    for nb in (1, 2):
        with pytest.raises(ValueError, match="bf16 storage"):
            model_generate(model32, tok, mk, dict(gk, num_beams=nb))
    assert eng32.calls == []                                                         # refused before the engine was asked for anything


def test_engine_and_model_entries_refuse_before_any_device_work():
    """T5Engine.generate / decode check the storage type first: called on an object that has nothing but a dtype, so anything past the
    check would raise AttributeError instead.  MapperatorinatorHIP.generate: ValueError for fp32 and for beams; forward / score do not
    take the flag."""
    import inspect
    from mapperatorinator_amd.modeling import MapperatorinatorHIP
    from mapperatorinator_amd.t5_engine import T5Engine
    eng = types.SimpleNamespace(dtype=torch.float32, device=torch.device("cpu"))
    prompt = torch.tensor([[1]])
    with pytest.raises(ValueError, match="self_kv_fp8 needs bf16 storage"):
        T5Engine.generate(eng, None, prompt, None, [], None, self_kv_fp8=True)
    with pytest.raises(ValueError, match="self_kv_fp8 needs bf16 storage"):
        T5Engine.decode(eng, None, prompt, None, None, None, self_kv_fp8=True)
    rec = _RecordingEngine(torch.float32)
    cfgm = types.SimpleNamespace(max_target_positions=40, pad_token_id=0, vocab_size=64, eos_token_id=2)
    me = types.SimpleNamespace(engine=rec, dtype=torch.float32, config=cfgm, device=torch.device("cpu"), _row_bias=lambda n, kw: None)
    call = lambda **kw: MapperatorinatorHIP.generate(me, inputs=torch.zeros(1, 16), decoder_input_ids=torch.tensor([[1]]), max_length=40, **kw)
    with pytest.raises(ValueError, match="bf16 storage"):
        call(self_kv_fp8=True)
    me.dtype = rec.dtype = torch.bfloat16
    with pytest.raises(ValueError, match="not built for beam search"):
        call(self_kv_fp8=True, num_beams=2)
    assert rec.calls == []
    call(self_kv_fp8=True)
    call()
    assert rec.calls[0][1]["self_kv_fp8"] is True and "self_kv_fp8" not in rec.calls[1][1]
    for fn in (MapperatorinatorHIP.forward, MapperatorinatorHIP.score, T5Engine.decoder_forward, T5Engine.score, T5Engine.generate_beam):
        assert "self_kv_fp8" not in inspect.signature(fn).parameters


class _SchedulerEngine:
    """What SequentialWindowScheduler needs of an engine, on the CPU: "cross K/V" of one value per window and a decode that appends
    one EOS id to every row; records the encode calls and the `self_kv_fp8` argument of every decode call."""

    def __init__(self, vocab_out, eos_id, dtype):
        import contextlib
        self.device, self.dtype = torch.device("cpu"), dtype
        self.packed = types.SimpleNamespace(vocab_out=vocab_out)
        self.eos_id, self.encoded, self.seen = eos_id, 0, []
        self._ctx = contextlib.nullcontext

    def _enter(self): pass
    def _leave(self): pass
    def synchronize(self): pass
    def on_stream(self): return self._ctx()
    def mel(self, audio): return audio

    def encode_mel(self, mel, row_bias=None):
        self.encoded += 1
        return mel

    def cross_kv(self, enc):
        return enc.abs().sum(-1).view(1, 1, -1, 1, 1, 1).expand(1, 2, -1, 1, 1, 64).contiguous()

    def decode(self, kv, prompt, prompt_mask, eos_table, sampling, forced=None, dump_logits=False, poll_every=16, kv_fp8=None,
               self_kv_fp8=False):
        self.seen.append(self_kv_fp8)
        B, P = prompt.shape
        tokens = torch.full((B, sampling.max_length), int(sampling.pad_id), dtype=torch.int32)
        tokens[:, :P] = prompt
        tokens[:, P] = self.eos_id
        return tokens, torch.tensor([P + 1], dtype=torch.int32), None


def test_scheduler_hands_the_flag_to_decode_and_refuses_fp32_and_beams_before_encoding():
    from mapperatorinator_amd.scheduler import SequentialWindowScheduler, SongJob
    tok = Tokenizer.benchmark_vocab(src_seq_len=251)
    tgt = 24
    eng = _SchedulerEngine(tok.vocab_size_out, tok.eos_id, torch.bfloat16)
    seen = eng.seen
    model = types.SimpleNamespace(engine=eng, config=types.SimpleNamespace(max_target_positions=tgt))

    def job(**gk):
        frames = torch.randn(2, 64, generator=torch.Generator().manual_seed(1))
        return SongJob(frames=frames, prompt_fn=lambda w: dict(decoder_input_ids=torch.tensor([[tok.sos_id, 7]])),
                       on_result=lambda w, row, st: None, generate_kwargs=dict(max_length=tgt, do_sample=False, cfg_scale=1.0, **gk))
    SequentialWindowScheduler(model, tok, decode_batch=8).run([job(num_beams=1, self_kv_fp8=True)])
    assert seen and all(s is True for s in seen)
    seen.clear()
    SequentialWindowScheduler(model, tok, decode_batch=8).run([job(num_beams=1)])
    assert seen and all(s is False for s in seen)                                   # (the default call passes nothing)
    n_encoded = eng.encoded
    assert n_encoded > 0
    with pytest.raises(ValueError, match="not built for beam search"):
        SequentialWindowScheduler(model, tok, decode_batch=8).run([job(num_beams=2, self_kv_fp8=True)])
    eng.dtype = torch.float32
    with pytest.raises(ValueError, match="self_kv_fp8 needs bf16 storage"):
        SequentialWindowScheduler(model, tok, decode_batch=8).run([job(num_beams=1, self_kv_fp8=True)])
    assert eng.encoded == n_encoded                                                  # refused before anything was encoded
    SequentialWindowScheduler(model, tok, decode_batch=8).run([job(num_beams=1)])    # (fp32 without the flag is nobody's business)


def test_row_quantiser_restatement():
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(5, 7, 64, generator=g) * torch.rand(5, 7, 1, generator=g) * 8).to(torch.bfloat16)
    x[1, 2] = 0                                             # an all-zero row: scale 1, bytes 0
    x[3, 3, 5] = 3.0e4                                      # a row whose absmax dwarfs the rest: they become e4m3 subnormals / zeros
    q, s = kv_fp8.quantize_rows(x)
    assert q.dtype == torch.uint8 and q.shape == x.shape and s.shape == x.shape[:-1] and s.dtype == torch.float32
    mx = x.float().abs().amax(-1)
    assert torch.equal(s, torch.where(mx > 0, mx / 448.0, torch.ones_like(mx)))
    assert s[1, 2] == 1 and (q[1, 2] == 0).all()
    val = q.view(torch.float8_e4m3fn).float()
    assert torch.isfinite(val).all() and val.abs().max() == 448       # the absmax element of a row lands on the largest e4m3 value
    assert torch.equal(val.abs().amax(-1)[mx > 0], torch.full_like(mx[mx > 0], 448.0))
    back = kv_fp8.qdq_rows(x)
    # e4m3 keeps 3 mantissa bits: half a step is 2^-4 relative; below the normal range the step is 2^-9 of the scaled value
    assert ((back - x.float()).abs() <= x.float().abs() / 16 + s[..., None] * 2.0 ** -10 + 1e-30).all()
    assert torch.equal(kv_fp8.qdq_rows(back), back)                    # idempotent: a quantised row is its own quantisation


def test_hook_quantises_rows_when_the_contract_says():
    """The hook on a stand-in oracle whose step only writes its row: with prompt_len = 9 the rows 0 .. 7 stay at storage precision
    until the step at position 7 and are quantised together there; from then on every row right after its own step.  prompt_len = 1:
    every row right after its own step."""
    class Base:
        def decoder_step(self, tok, pos, cache, ckv, key_mask):
            for K, V in cache:
                K[:, :, pos] = tok[:, None, None] * torch.linspace(0.1, 1.7, 64)
                V[:, :, pos] = -K[:, :, pos]
            self.seen = [K[:, :, :pos + 1].clone() for K, _ in cache]
            return None
    for P in (9, 1):
        o = kv_fp8.with_self_kv_fp8(Base, P)()
        cache = [(torch.zeros(2, 1, 12, 64), torch.zeros(2, 1, 12, 64)) for _ in range(2)]
        raw = []
        for pos in range(11):
            tok = torch.tensor([1.0 + pos, 2.5 + pos])
            o.decoder_step(tok, pos, cache, None, None)
            raw.append(tok[:, None, None] * torch.linspace(0.1, 1.7, 64))
            want = torch.stack(raw, 2)                                  # (2, 1, pos + 1, 64)
            first_q = 0 if pos >= P - 2 else pos + 1                    # rows below stay raw
            for K, V in cache:
                assert torch.equal(K[:, :, first_q:pos + 1], kv_fp8.qdq_rows(want[:, :, first_q:]))
                assert torch.equal(K[:, :, :first_q], want[:, :, :first_q]) and torch.equal(V[:, :, :pos + 1], -K[:, :, :pos + 1])
            # what the step itself attended: quantised rows below, its own row at storage precision
            n_q = 0 if pos < P - 1 else pos
            assert torch.equal(o.seen[0][:, :, n_q:], want[:, :, n_q:]) and torch.equal(o.seen[0][:, :, :n_q], kv_fp8.qdq_rows(want[:, :, :n_q]))
        assert not torch.equal(kv_fp8.qdq_rows(want), want)


@pytest.mark.parametrize("name", list(kv_fp8.CASES))
def test_oracle_near_tie_share_of_every_gpu_input_is_at_most_10_percent(name):
    """The GPU gate "no top-1 mismatch at any step whose oracle gap exceeds 0.25" leaves out the steps inside the gap; that share is
    asserted here, on the hooked oracle's own free run over the inputs the GPU test uses (mh_testing.kv_fp8.CASES)."""
    r = kv_fp8.oracle_runs(name, plain=False)
    c = r["spec"]
    share = r["n_close"] / r["n_steps"]
    print(f"{name}: {r['n_close']} of {r['n_steps']} steps inside the {kv_fp8.GAP} gap ({100 * share:.1f} %)")
    assert r["n_steps"] == c["rows"] * (c["tgt"] - max(c.get("prompts", (1,)))), "the free run ended early"
    assert share <= 0.10


def test_hooked_oracle_differs_from_the_plain_one():
    r = kv_fp8.oracle_runs("rope-small")
    dmax = max((a - b)[torch.isfinite(a)].abs().max().item() for a, b in zip(r["scores"], r["scores_plain"]))
    print(f"rope-small: the hook moves the oracle's logits by up to {dmax:.3f} on its own ids")
    assert dmax > 1e-3
    assert torch.equal(torch.isfinite(r["scores"][-1]), torch.isfinite(r["scores_plain"][-1]))
