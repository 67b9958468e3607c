"""CPU side of the in-flight decode over the e4m3 K/V caches (`mh_t5_slots_open_kv8`, `T5Engine.open_slots(cross_kv_fp8=, self_kv_fp8=)`,
`SequentialWindowScheduler(inflight=True, inflight_kv_fp8=)`): the symbol, the refusals that need no device, and the scheduler's
switch on the stand-in engine of tests/test_inflight_cpu.py.  The device side is tests/test_gpu_inflight_kv8.py."""
import ctypes as C
import os
import re
import types

import pytest
import torch

from conftest import ROOT
from mapperatorinator_amd import _lib
from mh_testing import row_sampling as rs
from test_inflight_cpu import _Engine, _Slots, _cfg, _songs


def test_symbol_is_declared_bound_and_exported_at_abi_11():
    hdr = open(os.path.join(ROOT, "include", "mapperhip.h")).read()
    lib = _lib.load()
    assert re.search(r"#define\s+MH_ABI_VERSION\s+11\b", hdr) and _lib.ABI_VERSION == 11 == lib.mh_abi_version()
    assert re.search(r"\bmh_t5_slots_open_kv8\s*\(", hdr)
    assert "mh_t5_slots_open_kv8" in _lib.SYMBOLS and hasattr(lib, "mh_t5_slots_open_kv8")
    # the argument list of mh_t5_slots_open; no struct joins the ABI and none changes its size
    assert _lib.SYMBOLS["mh_t5_slots_open_kv8"] == _lib.SYMBOLS["mh_t5_slots_open"]
    assert lib.mh_struct_size(9) == -1 and lib.mh_struct_size(8) == C.sizeof(_lib.MhRowSampling) == 64
    assert lib.mh_struct_size(3) == C.sizeof(_lib.MhSampling)


def test_new_entry_refuses_before_it_touches_the_device():
    """Every refusal of mh_t5_slots_open_kv8 comes with MH_ERR_ARG, a message in its own name and a NULL handle, before any device call
    (this host has no GPU)."""
    lib = _lib.load()
    one, w = C.c_void_p(256), _lib.MhT5Weights()

    def open_(sp, S=2, dtype=_lib.MH_BF16, rows=one, eos=one, n_sets=1, forced=None, skv8=None, kv=one, stream=one, ws_bytes=1 << 40):
        cfg = _cfg(dtype)
        h = C.c_void_p(1)
        rc = lib.mh_t5_slots_open_kv8(C.byref(cfg), C.byref(w), S, C.byref(sp), rows, eos, n_sets, kv, one, None, forced, skv8, one, ws_bytes,
                                      16, stream, C.byref(h))
        assert not h, "a refused open must hand back no session"
        msg = lib.mh_last_error()
        assert rc == -1 and msg.startswith(b"mh_t5_slots_open_kv8: "), (rc, msg)
        return msg

    def sampling(**over):
        sp = _lib.MhSampling()
        sp.max_length, sp.cfg_scale, sp.temperature = 24, 1.0, 1.0
        for k, v in over.items():
            setattr(sp, k, v)
        return sp
    modes = (dict(sp=dict(cross_kv_fp8=256)), dict(skv8=one), dict(sp=dict(cross_kv_fp8=256), skv8=one))
    # fp32 storage with either copy
    assert b"cross_kv_fp8 needs bf16 storage" in open_(sampling(cross_kv_fp8=256), dtype=_lib.MH_F32)
    assert b"the e4m3 self-attention cache needs bf16 storage" in open_(sampling(), dtype=_lib.MH_F32, skv8=one)
    for mode in modes:
        spk, skv8 = mode.get("sp", {}), mode.get("skv8")
        assert b"classifier-free guidance has no slot form" in open_(sampling(cfg_scale=1.5, **spk), skv8=skv8)
        assert b"teacher forcing (forced ids) has no slot form" in open_(sampling(**spk), skv8=skv8, forced=one)
        sp = sampling(n_cond=1, cond_per_row=0, tok_flags=256, **spk)
        sp.cond_temp[0], sp.cond_offset[0] = 0.5, 1
        assert b"need cond_per_row = 1" in open_(sp, skv8=skv8)
        for S in (0, 65, -1):
            assert open_(sampling(**spk), skv8=skv8, S=S) == b"mh_t5_slots_open_kv8: %d slots not in [1, 64]" % S
        # ... and whatever mh_t5_generate_rows refuses, in this entry's name
        assert b"null argument (rows" in open_(sampling(**spk), skv8=skv8, rows=None)
        assert b"needs a non-default stream" in open_(sampling(**spk), skv8=skv8, stream=None)
        assert b"max_length 49 exceeds tgt_len 48" in open_(sampling(max_length=49, **spk), skv8=skv8)
        assert b"workspace too small" in open_(sampling(**spk), skv8=skv8, ws_bytes=1024)
    # no bf16 slot copy: only where the e4m3 one stands in for it (behind that check the next refusal speaks: the workspace)
    assert b"cross_kv_slots may be NULL only where sp->cross_kv_fp8" in open_(sampling(), skv8=one, kv=None)
    assert b"null argument" in open_(sampling(), kv=None)
    assert b"workspace too small" in open_(sampling(cross_kv_fp8=256), kv=None, ws_bytes=1024)
    # with neither copy the entry is mh_t5_slots_open: the same refusals
    assert b"classifier-free guidance has no slot form" in open_(sampling(cfg_scale=1.5))


# ---- the scheduler on the stand-in engine -------------------------------------------------------------------------------------------
class _Kv8Engine(_Engine):
    """an engine whose open_slots takes the two switches; what it was given is recorded"""

    def open_slots(self, S, sp, dump_logits=False, poll_every=16, **switches):
        assert set(switches) <= {"cross_kv_fp8", "self_kv_fp8"}
        self.switches = switches
        self.sessions.append(_Slots(self, S, sp))
        return self.sessions[-1]


def _model(eng):
    return types.SimpleNamespace(engine=eng, config=types.SimpleNamespace(max_target_positions=24))


@pytest.mark.parametrize("value, want", [("cross", dict(cross_kv_fp8=True)), ("self", dict(self_kv_fp8=True)),
                                         ("both", dict(cross_kv_fp8=True, self_kv_fp8=True))])
def test_switch_reaches_open_slots_only_when_set(value, want):
    from mapperatorinator_amd.scheduler import SequentialWindowScheduler
    tok = rs.tokenizer("bench")
    eng, got = _Kv8Engine(tok.vocab_size_out), {}
    stats = SequentialWindowScheduler(_model(eng), tok, decode_batch=2, inflight=True, inflight_kv_fp8=value).run(_songs(tok, [2, 1], got, []))
    assert eng.switches == want and stats["windows"] == 3 == len(got) and len(eng.sessions) == 1
    # at its default the switch is not passed at all: the stand-in with the narrower signature keeps working
    plain, got = _Engine(tok.vocab_size_out), {}
    sched = SequentialWindowScheduler(_model(plain), tok, decode_batch=2, inflight=True)
    assert sched.inflight_kv_fp8 == dict(cross_kv_fp8=False, self_kv_fp8=False)
    assert sched.run(_songs(tok, [2, 1], got, []))["windows"] == 3
    eng = _Kv8Engine(tok.vocab_size_out)
    SequentialWindowScheduler(_model(eng), tok, decode_batch=2, inflight=True, inflight_kv_fp8=None).run(_songs(tok, [1], {}, []))
    assert eng.switches == {}


def test_bad_values_and_fp32_storage_are_refused_before_anything_is_encoded():
    from mapperatorinator_amd.scheduler import SequentialWindowScheduler
    tok = rs.tokenizer("bench")
    eng = _Kv8Engine(tok.vocab_size_out)
    for bad in ("all", "cross,self", True, 1, ""):
        with pytest.raises(ValueError, match="inflight_kv_fp8"):
            SequentialWindowScheduler(_model(eng), tok, decode_batch=2, inflight=True, inflight_kv_fp8=bad)
    for value in ("cross", "self", "both"):
        with pytest.raises(ValueError, match="needs inflight=True"):
            SequentialWindowScheduler(_model(eng), tok, decode_batch=2, inflight_kv_fp8=value)
    eng.dtype = torch.float32
    for value, words in (("cross", "cross_kv_fp8 needs bf16 storage"), ("self", "self_kv_fp8 needs bf16 storage"),
                         ("both", "cross_kv_fp8 needs bf16 storage")):
        with pytest.raises(ValueError, match=words):    # DecodeModes' own texts
            SequentialWindowScheduler(_model(eng), tok, decode_batch=2, inflight=True, inflight_kv_fp8=value).run(_songs(tok, [1], {}, []))
    SequentialWindowScheduler(_model(eng), tok, decode_batch=2, inflight=True)      # (fp32 without the switch: as ever)
    assert eng.encoded == 0 and not eng.sessions


@pytest.mark.parametrize("over, words", [(dict(cross_kv_fp8=True), "e4m3 copy of the cross K/V"), (dict(self_kv_fp8=True), "e4m3 self-attention cache")])
@pytest.mark.parametrize("where", ["job", "window"])
def test_per_job_and_per_window_fp8_kwargs_are_still_refused(over, words, where):
    """... with the session's switch on as well: a window cannot choose the caches.  The message points to the switch."""
    from mapperatorinator_amd.scheduler import SequentialWindowScheduler
    tok = rs.tokenizer("bench")
    eng, got = _Kv8Engine(tok.vocab_size_out), {}
    jobs = _songs(tok, [2, 1], got, [])
    if where == "job":
        jobs[1].generate_kwargs.update(over)
    else:
        ask = jobs[1].prompt_fn
        jobs[1].prompt_fn = lambda w: dict(ask(w), generate_kwargs=dict(ask(w)["generate_kwargs"], **over))
    with pytest.raises(ValueError, match=words + ".*no slot form.*inflight_kv_fp8"):
        SequentialWindowScheduler(_model(eng), tok, decode_batch=2, inflight=True, inflight_kv_fp8="both").run(jobs)
    assert (eng.encoded == 0 or where == "window") and not eng.sessions and not got     # (a job's kwargs: before anything is encoded)


def test_decode_slots_take_the_switches_behind_the_positional_arguments():
    import inspect
    from mapperatorinator_amd.t5_engine import DecodeSlots, T5Engine
    names = list(inspect.signature(T5Engine.open_slots).parameters)
    assert names == ["self", "S", "sampling", "dump_logits", "poll_every", "cross_kv_fp8", "self_kv_fp8"]
    sig = inspect.signature(T5Engine.open_slots)
    assert sig.parameters["cross_kv_fp8"].default is False and sig.parameters["self_kv_fp8"].default is False
    with pytest.raises(ValueError, match="65 slots not in"):
        DecodeSlots(None, 65, None, False, 16, True, True)
    # the storage refusals are DecodeModes' own, before any buffer is made
    fp32 = types.SimpleNamespace(dtype=torch.float32, _slot_session=None)
    with pytest.raises(ValueError, match="cross_kv_fp8 needs bf16 storage"):
        DecodeSlots(fp32, 2, None, False, 16, True, False)
    with pytest.raises(ValueError, match="self_kv_fp8 needs bf16 storage"):
        DecodeSlots(fp32, 2, None, False, 16, False, True)
