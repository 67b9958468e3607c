"""CPU side of the in-flight decode under classifier-free guidance (`mh_t5_slots_open_guided`, `mh_t5_slots_admit_pair`,
`T5Engine.open_guided_slots`, `SequentialWindowScheduler(inflight=True, inflight_guided=True)`): the symbols, the workspace figure, the
refusals that need no device, and the scheduler's switch on a stand-in engine.  The device side is tests/test_gpu_inflight_guided.py."""
import contextlib
import ctypes as C
import os
import re
import types

import pytest
import torch

from conftest import ROOT
from mapperatorinator_amd import _lib
from mh_testing import row_sampling as rs

G = rs.gen_kwargs
GUIDED_SYMBOLS = ("mh_t5_slots_guided_workspace_bytes", "mh_t5_slots_open_guided", "mh_t5_slots_admit_pair")


def _cfg(dtype):    # d 128, 2 heads, 2 + 2 layers, src 251, tgt 48
    return _lib.MhT5Config(128, 64, 256, 2, 2, 2, 10, 10, 388, 416, 251, 48, dtype, 1e-6)


def test_symbols_are_declared_bound_and_exported_at_abi_11():
    hdr = open(os.path.join(ROOT, "include", "mapperhip.h")).read()
    lib = _lib.load()
    assert re.search(r"#define\s+MH_ABI_VERSION\s+11\b", hdr) and _lib.ABI_VERSION == 11 == lib.mh_abi_version()
    for name in GUIDED_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    # the argument lists of the entries they stand beside; no struct joins the ABI and none changes its size
    assert _lib.SYMBOLS["mh_t5_slots_open_guided"] == _lib.SYMBOLS["mh_t5_slots_open_kv8"]
    assert _lib.SYMBOLS["mh_t5_slots_admit_pair"] == _lib.SYMBOLS["mh_t5_slots_admit"]
    assert _lib.SYMBOLS["mh_t5_slots_guided_workspace_bytes"] == _lib.SYMBOLS["mh_t5_slots_workspace_bytes"]
    assert lib.mh_struct_size(9) == -1 and lib.mh_struct_size(8) == C.sizeof(_lib.MhRowSampling) == 64
    assert lib.mh_struct_size(3) == C.sizeof(_lib.MhSampling)


def test_workspace_bytes_cover_two_rows_per_pair_and_refuse_the_pair_count():
    lib = _lib.load()
    cfg = _cfg(_lib.MH_BF16)
    f = lib.mh_t5_slots_guided_workspace_bytes
    assert f(C.byref(cfg), 0) == -1 and f(C.byref(cfg), 33) == -1 and f(None, 4) == -1
    sizes = [f(C.byref(cfg), S) for S in range(1, 33)]
    assert all(a < b for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0
    # the plain session's figure is its decode part (the decode layout of S rows and the slot arrays) and the prompt prefill of one
    # row; that prefill's slabs at this configuration (47 positions: fp32 h, then n, q, attn, ff, the 64-padded V^T and the 256-padded
    # cross V^T of both layers in bf16) are a lower bound of its bytes, so what is left is an upper bound of the decode part
    rows, d, inner, dff, es = 47, 128, 128, 256, 2
    prefill_1 = rows * d * 4 + rows * d * es + 2 * rows * inner * es + rows * dff * es + inner * 64 * es + 2 * inner * 256 * es
    plain = lambda S: lib.mh_t5_slots_workspace_bytes(C.byref(cfg), S)    # noqa: E731
    for S in (1, 3, 17, 32):
        decode_part = plain(S) - prefill_1
        assert decode_part > 0 and f(C.byref(cfg), S) > 2 * decode_part, (S, f(C.byref(cfg), S), decode_part)
        # ... and it holds the decode layout of 2 S rows with the slot arrays of 2 S rows, and a prefill
        assert f(C.byref(cfg), S) >= plain(2 * S)


def _open(lib, sp, S=2, dtype=_lib.MH_BF16, rows=256, eos=256, n_sets=1, forced=None, skv8=None, kv=256, stream=256, ws_bytes=1 << 40):
    one = C.c_void_p(256)
    p = lambda v: None if v is None else C.c_void_p(v) if isinstance(v, int) else v   # noqa: E731
    cfg, w = _cfg(dtype), _lib.MhT5Weights()
    h = C.c_void_p(1)
    rc = lib.mh_t5_slots_open_guided(C.byref(cfg), C.byref(w), S, C.byref(sp), p(rows), p(eos), n_sets, p(kv), one, None, p(forced), p(skv8), one,
                                     ws_bytes, 16, p(stream), C.byref(h))
    assert not h, "a refused open must hand back no session"
    msg = lib.mh_last_error()
    assert rc == -1 and msg.startswith(b"mh_t5_slots_open_guided: "), (rc, msg)
    return msg


def _sampling(**over):
    sp = _lib.MhSampling()
    sp.max_length, sp.cfg_scale, sp.temperature = 24, 2.0, 1.0
    for k, v in over.items():
        setattr(sp, k, v)
    return sp


def test_library_refuses_before_it_touches_the_device():
    """Every refusal of mh_t5_slots_open_guided comes with MH_ERR_ARG, a message in its own name and a NULL handle, before any device
    call (this host has no GPU)."""
    lib = _lib.load()
    modes = (dict(), dict(sp=dict(cross_kv_fp8=256)), dict(skv8=256), dict(sp=dict(cross_kv_fp8=256), skv8=256))
    for mode in modes:
        spk, skv8 = mode.get("sp", {}), mode.get("skv8")
        for scale in (1.0, 0.5, 0.0):
            assert b"needs sp->cfg_scale > 1" in _open(lib, _sampling(cfg_scale=scale, **spk), skv8=skv8)
        assert b"teacher forcing (forced ids) has no slot form" in _open(lib, _sampling(**spk), skv8=skv8, forced=256)
        sp = _sampling(n_cond=1, cond_per_row=0, tok_flags=256, **spk)
        sp.cond_temp[0], sp.cond_offset[0] = 0.5, 1
        assert b"need cond_per_row = 1" in _open(lib, sp, skv8=skv8)
        for S in (0, 33, 64, -1):
            assert _open(lib, _sampling(**spk), skv8=skv8, S=S).startswith(b"mh_t5_slots_open_guided: %d pairs not in [1, 32]" % S)
        # ... and whatever the two existing open entries refuse, in this entry's name
        assert b"null argument (rows" in _open(lib, _sampling(**spk), skv8=skv8, rows=None)
        assert b"n_eos_sets 0 must be >= 1" in _open(lib, _sampling(**spk), skv8=skv8, n_sets=0)
        assert b"needs a non-default stream" in _open(lib, _sampling(**spk), skv8=skv8, stream=None)
        assert b"max_length 49 exceeds tgt_len 48" in _open(lib, _sampling(max_length=49, **spk), skv8=skv8)
        assert b"workspace too small (mh_t5_slots_guided_workspace_bytes)" in _open(lib, _sampling(**spk), skv8=skv8, ws_bytes=1024)
    assert b"cross_kv_fp8 needs bf16 storage" in _open(lib, _sampling(cross_kv_fp8=256), dtype=_lib.MH_F32)
    assert b"the e4m3 self-attention cache needs bf16 storage" in _open(lib, _sampling(), dtype=_lib.MH_F32, skv8=256)
    assert b"cross_kv_slots may be NULL only where sp->cross_kv_fp8" in _open(lib, _sampling(), skv8=256, kv=None)
    assert b"null argument" in _open(lib, _sampling(), kv=None)
    assert b"workspace too small" in _open(lib, _sampling(cross_kv_fp8=256), kv=None, ws_bytes=1024)     # (NULL is fine beside the e4m3 copy)
    # the workspace of a PLAIN session of as many slots is too small for the pairs
    cfg = _cfg(_lib.MH_BF16)
    assert b"workspace too small" in _open(lib, _sampling(), ws_bytes=lib.mh_t5_slots_workspace_bytes(C.byref(cfg), 2))
    one = C.c_void_p(256)
    assert lib.mh_t5_slots_admit_pair(None, 0, one, one, None, 1, None) == -1 and b"mh_t5_slots_admit_pair: null handle" in lib.mh_last_error()


def test_plain_entries_keep_their_refusal_of_guidance():
    lib = _lib.load()
    one, w, cfg = C.c_void_p(256), _lib.MhT5Weights(), _cfg(_lib.MH_BF16)
    for name in ("mh_t5_slots_open", "mh_t5_slots_open_kv8"):
        h = C.c_void_p(1)
        sp = _sampling(cfg_scale=1.5)
        rc = getattr(lib, name)(C.byref(cfg), C.byref(w), 2, C.byref(sp), one, one, 1, one, one, None, None, None, one, 1 << 40, 16, one, C.byref(h))
        assert rc == -1 and not h
        assert lib.mh_last_error() == b"%s: classifier-free guidance has no slot form (a pair spans two rows of one position)" % name.encode()


# ---- the scheduler on a stand-in engine ---------------------------------------------------------------------------------------------
class _Pairs:
    """What `T5Engine.open_guided_slots` returns, on the CPU: a pair admitted with a prompt of P ids is finished after P `run` steps and
    ends on the last id of its own EOS table; everything is recorded."""

    def __init__(self, eng, S, sp, switches):
        self.eng, self.S, self.sp, self.switches = eng, S, sp, switches
        self.live, self.left, self.rows = [False] * S, [0] * S, [None] * S
        self.stats = dict(admissions=0, steps=0, runs=0)
        self.closed = False

    def admit(self, slot, kv_row, prompt, mask, row, eos_table, negative_prompt=None):
        assert not self.live[slot] and not self.closed
        assert negative_prompt is not None, "a guided session admits pairs"
        prompt = prompt.reshape(-1)
        self.live[slot], self.left[slot] = True, int(prompt.shape[0])
        self.rows[slot] = torch.cat([prompt.to(torch.int64), torch.tensor([int(eos_table.nonzero().max())])])
        self.stats["admissions"] += 1
        self.eng.admitted.append(dict(slot=slot, song=float(kv_row.reshape(-1)[0]), P=int(prompt.shape[0]), scale=round(row.cfg_scale, 6),
                                      negative=negative_prompt.reshape(-1).tolist(), run=self.stats["runs"], seed=row.seed))

    def run(self, n_steps):
        self.stats["runs"] += 1
        self.stats["steps"] += n_steps
        for s in range(self.S):
            if self.live[s]:
                self.left[s] -= n_steps
        return [self.live[s] and self.left[s] <= 0 for s in range(self.S)], [0] * self.S

    def take(self, slot):
        assert self.live[slot] and self.left[slot] <= 0
        self.live[slot] = False
        return self.rows[slot]

    def close(self):
        self.closed = True


class _Engine:
    def __init__(self, vocab_out):
        self.device, self.dtype = torch.device("cpu"), torch.bfloat16
        self.packed = types.SimpleNamespace(vocab_out=vocab_out)
        self.admitted, self.sessions, self.plain_sessions, self.encoded = [], [], 0, 0

    def _enter(self): pass
    def _leave(self): pass
    def synchronize(self): pass
    def on_stream(self): return contextlib.nullcontext()
    def mel(self, audio): return audio

    def encode_mel(self, mel, row_bias=None):
        self.encoded += 1
        return mel

    def cross_kv(self, enc):
        return enc.abs().sum(-1).view(1, 1, -1, 1, 1, 1).expand(1, 2, -1, 1, 1, 64).contiguous()

    def decode(self, *a, **k):
        raise AssertionError("inflight must not decode in waves")

    def open_slots(self, S, sp, dump_logits=False, poll_every=16, **switches):
        self.plain_sessions += 1
        raise AssertionError("the guided switch must open a guided session")

    def open_guided_slots(self, S, sp, dump_logits=False, poll_every=16, **switches):
        self.sessions.append(_Pairs(self, S, sp, switches))
        return self.sessions[-1]


def _songs(tok, lengths, got, order, scales=(1.5, 3.0, 2.0), negative=True):
    """song i has lengths[i] windows; window w has a prompt of 1 + (i + w) % 3 ids behind sos, a negative prompt [sos, 90 + i, w] cut to
    the prompt's length, and the scale scales[(i + w) % 3]; its "K/V" value is 16 * (i + 1 + 100 w)"""
    from mapperatorinator_amd.scheduler import SongJob
    jobs = []
    for i, n in enumerate(lengths):
        def prompt_fn(w, i=i, n=n):
            assert w == 0 or (i, w - 1) in got, "window w + 1 was asked for before window w was delivered"
            ids = torch.tensor([[tok.sos_id] + [40 + i] * (1 + (i + w) % 3)])
            ask = dict(decoder_input_ids=ids, generate_kwargs=dict(cfg_scale=scales[(i + w) % 3], lookback_time=300 if w else 0,
                                                                   lookahead_time=400 if w != n - 1 else 0))
            if negative:
                ask["negative_prompt"] = torch.tensor([[tok.sos_id, 90 + i, w]])[:, :ids.shape[1]]
            return ask

        def on_result(w, row, st, i=i):
            got[(i, w)] = row.tolist()
            order.append((i, w))
        frames = torch.full((n, 16), float(i + 1)) + torch.arange(n)[:, None] * 100.0
        jobs.append(SongJob(frames=frames, prompt_fn=prompt_fn, on_result=on_result,
                            generate_kwargs=G(max_length=24, temperature=1.0 + 0.1 * i, seed=9, cfg_scale=2.0)))
    return jobs


def _model(eng):
    return types.SimpleNamespace(engine=eng, config=types.SimpleNamespace(max_target_positions=24))


def test_decode_batch_4_is_two_pairs_and_every_admission_carries_its_negative_prompt_and_scale():
    from mapperatorinator_amd.scheduler import SequentialWindowScheduler
    tok = rs.tokenizer("bench")
    eng, got, order = _Engine(tok.vocab_size_out), {}, []
    lengths = [2, 3, 1]
    sched = SequentialWindowScheduler(_model(eng), tok, decode_batch=4, inflight=True, inflight_guided=True, inflight_steps=1)
    stats = sched.run(_songs(tok, lengths, got, order))
    assert len(eng.sessions) == 1 and eng.plain_sessions == 0
    ses = eng.sessions[0]
    assert ses.S == 2 and ses.closed and ses.switches == {} and ses.sp.cfg_scale > 1.0 and ses.sp.cond_per_row == 1
    assert stats["windows"] == stats["admissions"] == sum(lengths) == len(eng.admitted) == len(got)
    by_song = {a["song"]: a for a in eng.admitted}
    for i, n in enumerate(lengths):
        assert [w for k, w in order if k == i] == list(range(n))     # songs are delivered in order
        for w in range(n):
            a = by_song[16.0 * (i + 1 + 100 * w)]
            P = 2 + (i + w) % 3
            assert a["P"] == P and a["negative"] == [tok.sos_id, 90 + i, w][:P] and a["scale"] == (1.5, 3.0, 2.0)[(i + w) % 3], a
    # the admission policy of the plain session: lowest idle slot first, songs first come first served
    assert [(a["song"], a["slot"], a["run"]) for a in eng.admitted][:3] == [(16.0, 0, 0), (32.0, 1, 0), (48.0, 0, 2)]
    # the e4m3 switches of the session compose
    eng = _Engine(tok.vocab_size_out)
    SequentialWindowScheduler(_model(eng), tok, decode_batch=2, inflight=True, inflight_guided=True, inflight_kv_fp8="both").run(
        _songs(tok, [1], {}, []))
    assert eng.sessions[0].S == 1 and eng.sessions[0].switches == dict(cross_kv_fp8=True, self_kv_fp8=True)


def test_an_unguided_job_is_refused_by_name_before_anything_is_encoded():
    from mapperatorinator_amd.scheduler import SequentialWindowScheduler
    tok = rs.tokenizer("bench")
    for over in (dict(cfg_scale=1.0), None):
        eng, got = _Engine(tok.vocab_size_out), {}
        jobs = _songs(tok, [2, 1], got, [])
        if over is None:
            jobs[1].generate_kwargs.pop("cfg_scale")
        else:
            jobs[1].generate_kwargs.update(over)
        with pytest.raises(ValueError, match=r"inflight_guided: job 1 is not guided"):
            SequentialWindowScheduler(_model(eng), tok, decode_batch=4, inflight=True, inflight_guided=True).run(jobs)
        assert eng.encoded == 0 and not eng.sessions and not got


def test_a_window_without_negative_prompt_is_refused_before_anything_is_encoded():
    from mapperatorinator_amd.scheduler import SequentialWindowScheduler
    tok = rs.tokenizer("bench")
    eng, got = _Engine(tok.vocab_size_out), {}
    jobs = _songs(tok, [2], got, []) + _songs(tok, [1], got, [], negative=False)
    with pytest.raises(ValueError, match=r"inflight_guided: window 0 of job 1 has no negative_prompt"):
        SequentialWindowScheduler(_model(eng), tok, decode_batch=4, inflight=True, inflight_guided=True).run(jobs)
    assert eng.encoded == 0 and not eng.sessions and not got


def test_the_switch_needs_inflight_and_off_it_changes_nothing():
    from mapperatorinator_amd.scheduler import SequentialWindowScheduler
    tok = rs.tokenizer("bench")
    eng = _Engine(tok.vocab_size_out)
    with pytest.raises(ValueError, match="inflight_guided=True.*needs inflight=True"):
        SequentialWindowScheduler(_model(eng), tok, decode_batch=4, inflight_guided=True)
    sched = SequentialWindowScheduler(_model(eng), tok, decode_batch=4, inflight=True)
    assert sched.inflight_guided is False
    # off: guidance under inflight is refused as ever, in the existing words
    with pytest.raises(ValueError, match=r"inflight: job 0 asks for classifier-free guidance \(cfg_scale=2.0\), which has no slot form"):
        sched.run(_songs(tok, [1], {}, []))
    assert eng.encoded == 0 and not eng.sessions and eng.plain_sessions == 0


def test_decode_slots_refuse_the_pair_count_and_an_unguided_setting_on_the_host():
    from mapperatorinator_amd.t5_engine import DecodeSlots
    sp = _sampling()
    for S in (0, 33):
        with pytest.raises(ValueError, match=f"{S} pairs not in"):
            DecodeSlots(None, S, sp, False, 16, guided=True)
    with pytest.raises(ValueError, match="needs sampling.cfg_scale > 1"):
        DecodeSlots(None, 2, _sampling(cfg_scale=1.0), False, 16, guided=True)
