"""CPU side of the in-flight decode (`mh_t5_slots_*`, `T5Engine.open_slots`, `SequentialWindowScheduler(inflight=True)`): symbols,
refusals that need no device, and the scheduler's admission policy, ordering, seed rule and stats on a stand-in engine.  The device
side is tests/test_gpu_inflight.py."""
import ctypes as C
import os
import re
import types

import pytest
import torch

from conftest import ROOT
from mapperatorinator_amd import _lib
from mapperatorinator_amd.server import build_row_sampling, build_sampling
from mh_testing import row_sampling as rs

G = rs.gen_kwargs
SLOT_SYMBOLS = ("mh_t5_slots_workspace_bytes", "mh_t5_slots_open", "mh_t5_slots_admit", "mh_t5_slots_run", "mh_t5_slots_release",
                "mh_t5_slots_close")


def _cfg(dtype):    # d 128, 2 heads, 2 + 2 layers, src 251, tgt 48
    return _lib.MhT5Config(128, 64, 256, 2, 2, 2, 10, 10, 388, 416, 251, 48, dtype, 1e-6)


def test_symbols_are_declared_bound_and_exported_at_abi_11():
    hdr = open(os.path.join(ROOT, "include", "mapperhip.h")).read()
    lib = _lib.load()
    assert re.search(r"#define\s+MH_ABI_VERSION\s+11\b", hdr) and _lib.ABI_VERSION == 11 == lib.mh_abi_version()
    for name in SLOT_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    # the session is an opaque handle: no struct joins the ABI, the existing ones keep their sizes
    assert lib.mh_struct_size(9) == -1 and lib.mh_struct_size(8) == C.sizeof(_lib.MhRowSampling) == 64
    assert lib.mh_struct_size(3) == C.sizeof(_lib.MhSampling)
    assert _lib.SYMBOLS["mh_t5_slots_open"][1][-1] == C.POINTER(C.c_void_p)


def test_workspace_bytes_cover_the_decode_workspace_and_refuse_the_slot_count():
    lib = _lib.load()
    cfg = _cfg(_lib.MH_BF16)
    for S in (1, 3, 17, 64):
        need = lib.mh_t5_slots_workspace_bytes(C.byref(cfg), S)
        # the decode buffers of S rows are in it (that figure also holds a prefill of S rows: only a lower bound of the common part)
        assert need > 0 and need > 2 * 2 * S * 2 * 64 * 48 * 2
    assert lib.mh_t5_slots_workspace_bytes(C.byref(cfg), 1) < lib.mh_t5_slots_workspace_bytes(C.byref(cfg), 2)
    assert lib.mh_t5_slots_workspace_bytes(C.byref(cfg), 0) == -1 and lib.mh_t5_slots_workspace_bytes(C.byref(cfg), 65) == -1
    assert lib.mh_t5_slots_workspace_bytes(None, 4) == -1


def test_library_refuses_before_it_touches_the_device():
    """Every refusal of mh_t5_slots_open comes with MH_ERR_ARG and a message before any device call (this host has no GPU)."""
    lib = _lib.load()
    one, w = C.c_void_p(256), _lib.MhT5Weights()
    cfg = _cfg(_lib.MH_BF16)

    def open_(sp, S=2, rows=one, eos=one, n_sets=1, forced=None, skv8=None, stream=one, ws_bytes=1 << 40):
        h = C.c_void_p(1)
        rc = lib.mh_t5_slots_open(C.byref(cfg), C.byref(w), S, C.byref(sp), rows, eos, n_sets, one, one, None, forced, skv8, one, ws_bytes, 16,
                                  stream, C.byref(h))
        assert not h, "a refused open must hand back no session"
        return rc, lib.mh_last_error()

    def sampling(**over):
        sp = _lib.MhSampling()
        sp.max_length, sp.cfg_scale, sp.temperature = 24, 1.0, 1.0
        for k, v in over.items():
            setattr(sp, k, v)
        return sp
    for S in (0, 65, -1):
        assert open_(sampling(), S=S) == (-1, b"mh_t5_slots_open: %d slots not in [1, 64]" % S)
    rc, msg = open_(sampling(), rows=None)
    assert rc == -1 and b"mh_t5_slots_open: null argument (rows" in msg
    rc, msg = open_(sampling(), n_sets=0)
    assert rc == -1 and b"n_eos_sets 0 must be >= 1" in msg
    rc, msg = open_(sampling(cfg_scale=1.5))
    assert rc == -1 and b"classifier-free guidance has no slot form" in msg
    rc, msg = open_(sampling(), forced=one)
    assert rc == -1 and b"teacher forcing (forced ids) has no slot form" in msg
    rc, msg = open_(sampling(cross_kv_fp8=256))
    assert rc == -1 and b"(cross_kv_fp8) has no slot form" in msg
    rc, msg = open_(sampling(), skv8=one)
    assert rc == -1 and b"e4m3 shadow of the self-attention cache has no slot form" in msg
    sp = sampling(n_cond=1, cond_per_row=0, tok_flags=256)
    sp.cond_temp[0], sp.cond_offset[0] = 0.5, 1
    rc, msg = open_(sp)
    assert rc == -1 and b"need cond_per_row = 1" in msg
    # ... and whatever mh_t5_generate_rows refuses, in this entry's name
    rc, msg = open_(sampling(), stream=None)
    assert rc == -1 and b"mh_t5_slots_open: needs a non-default stream" in msg
    rc, msg = open_(sampling(max_length=49))
    assert rc == -1 and b"mh_t5_slots_open: max_length 49 exceeds tgt_len 48" in msg
    rc, msg = open_(sampling(), ws_bytes=1024)
    assert rc == -1 and b"mh_t5_slots_open: workspace too small" in msg
    # the other entries refuse a missing session
    assert lib.mh_t5_slots_admit(None, 0, one, one, None, 1, None) == -1 and b"mh_t5_slots_admit: null handle" in lib.mh_last_error()
    fin, length = (C.c_uint8 * 2)(), (C.c_int32 * 2)()
    assert lib.mh_t5_slots_run(None, 1, fin, length, None) == -1 and b"mh_t5_slots_run: null handle" in lib.mh_last_error()
    assert lib.mh_t5_slots_release(None, 0) == -1 and lib.mh_t5_slots_close(None) == 0


# ---- the scheduler on a stand-in engine ---------------------------------------------------------------------------------------------
class _Slots:
    """What `T5Engine.open_slots` returns, on the CPU: a window admitted with a prompt of P ids is finished after P `run` steps and
    ends on the LAST id of its own EOS table; everything is recorded."""

    def __init__(self, eng, S, sp):
        self.eng, self.S, self.sp = eng, S, sp
        self.live, self.left, self.rows = [False] * S, [0] * S, [None] * S
        self.stats = dict(admissions=0, steps=0, runs=0)
        self.closed = False

    def admit(self, slot, kv_row, prompt, mask, row, eos_table):
        assert not self.live[slot] and not self.closed
        prompt = prompt.reshape(-1)
        self.live[slot], self.left[slot] = True, int(prompt.shape[0])
        self.rows[slot] = torch.cat([prompt.to(torch.int64), torch.tensor([int(eos_table.nonzero().max())])])
        self.stats["admissions"] += 1
        self.eng.admitted.append(dict(slot=slot, song=float(kv_row.reshape(-1)[0]), P=int(prompt.shape[0]), seed=row.seed, rng_row=row.rng_row,
                                      temperature=round(row.temperature, 6), max_length=row.max_length, run=self.stats["runs"],
                                      lookback=row.lookback_mask_end > 0))

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
        import contextlib
        self.device, self.dtype = torch.device("cpu"), torch.bfloat16
        self.packed = types.SimpleNamespace(vocab_out=vocab_out)
        self.admitted, self.sessions, self.encoded = [], [], 0
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

    def decode(self, *a, **k):
        raise AssertionError("inflight must not decode in waves")

    def open_slots(self, S, sp, dump_logits=False, poll_every=16):
        self.sessions.append(_Slots(self, S, sp))
        return self.sessions[-1]


def _songs(tok, lengths, got, order, **common):
    """song i has lengths[i] windows; window w has a prompt of 1 + (i + w) % 3 ids behind sos, the reference's EOS windows and a
    temperature of its own song; its "K/V" value is 16 * (i + 1 + 100 w)"""
    from mapperatorinator_amd.scheduler import SongJob
    jobs = []
    for i, n in enumerate(lengths):
        def prompt_fn(w, i=i, n=n):
            assert w == 0 or (i, w - 1) in got, "window w + 1 was asked for before window w was delivered"
            return dict(decoder_input_ids=torch.tensor([[tok.sos_id] + [40 + i] * (1 + (i + w) % 3)]),
                        generate_kwargs=dict(lookback_time=300 if w else 0, lookahead_time=400 if w != n - 1 else 0))

        def on_result(w, row, st, i=i):
            got[(i, w)] = row.tolist()
            order.append((i, w))
        frames = torch.full((n, 16), float(i + 1)) + torch.arange(n)[:, None] * 100.0
        jobs.append(SongJob(frames=frames, prompt_fn=prompt_fn, on_result=on_result,
                            generate_kwargs=dict(G(max_length=24, temperature=1.0 + 0.1 * i, seed=9), **common)))
    return jobs


def _run(tok, lengths, S=2, steps=1, **common):
    from mapperatorinator_amd.scheduler import SequentialWindowScheduler
    eng = _Engine(tok.vocab_size_out)
    model = types.SimpleNamespace(engine=eng, config=types.SimpleNamespace(max_target_positions=24))
    got, order = {}, []
    sched = SequentialWindowScheduler(model, tok, decode_batch=S, inflight=True, inflight_steps=steps)
    stats = sched.run(_songs(tok, lengths, got, order, **common))
    return eng, got, order, stats


def test_default_is_waves():
    from mapperatorinator_amd.scheduler import SequentialWindowScheduler
    tok = rs.tokenizer("bench")
    model = types.SimpleNamespace(engine=_Engine(tok.vocab_size_out), config=types.SimpleNamespace(max_target_positions=24))
    assert SequentialWindowScheduler(model, tok).inflight is False


def test_admission_policy_which_window_enters_which_slot_after_which_retirement():
    """2 slots, songs of 2, 3 and 1 windows; the stand-in finishes a window after as many steps as its prompt has ids (2, 3 or 4).
    Lowest idle slot first, songs first come first served, a song's next window queues when its window was delivered."""
    tok = rs.tokenizer("bench")
    eng, got, order, stats = _run(tok, [2, 3, 1])
    adm = [(a["song"], a["slot"], a["run"]) for a in eng.admitted]
    # song value = 16 (i + 1 + 100 w).  run 0: song 0 w 0 (P 2) -> slot 0, song 1 w 0 (P 3) -> slot 1
    # after run 2: slot 0 retires -> song 2 w 0 (P 4: it was ready first), song 0 w 1 queues behind it
    # after run 3: slot 1 retires -> song 0 w 1 (P 3); song 1 w 1 queues
    # after run 6: slots 0 and 1 retire together (song 2 w 0, song 0 w 1) -> song 1 w 1 (P 4) -> slot 0
    # after run 10: song 1 w 2 (P 2) -> slot 0
    assert adm == [(16.0, 0, 0), (32.0, 1, 0), (48.0, 0, 2), (1616.0, 1, 3), (1632.0, 0, 6), (3232.0, 0, 10)], adm
    assert order == [(0, 0), (1, 0), (2, 0), (0, 1), (1, 1), (1, 2)]
    assert len(eng.sessions) == 1 and eng.sessions[0].S == 2 and eng.sessions[0].closed
    assert eng.sessions[0].sp.cond_per_row == 1 and eng.sessions[0].sp.max_length == 24


def test_per_song_order_eos_sets_and_stats():
    tok = rs.tokenizer("bench")
    lengths = [3, 1, 4, 2]
    eng, got, order, stats = _run(tok, lengths, S=3, steps=2)
    for i, n in enumerate(lengths):
        assert [w for k, w in order if k == i] == list(range(n))
    assert len(got) == sum(lengths) == stats["windows"] == stats["admissions"] == len(eng.admitted)
    assert stats["decode_steps"] == eng.sessions[0].stats["steps"] > 0 and stats["generated_tokens"] == sum(lengths)
    assert stats["encode_calls"] == 1 and eng.encoded == 1
    # every window ends on the last id of ITS EOS set (lookahead windows end on a time shift) and carries its own settings
    ts1 = [v for k, v in tok.event_end.items() if k.name == "TIME_SHIFT"][0]
    from mapperatorinator_amd.server import get_eos_token_id
    last_window = max(int(e) for e in get_eos_token_id(tok, lookback_time=300, lookahead_time=0, context_type=None))
    assert got[(0, 0)][-1] == ts1 - 1 and got[(0, 2)][-1] == last_window and got[(1, 0)][-1] == tok.eos_id
    by_song = {a["song"]: a for a in eng.admitted}
    assert by_song[16.0 * (3 + 100 * 1)]["temperature"] == 1.2 and by_song[16.0 * (3 + 100 * 1)]["lookback"]
    assert not by_song[16.0 * 3]["lookback"] and by_song[16.0 * 3]["max_length"] == 24


def test_seed_rule_is_the_default_policys_batch_1_call():
    """Explicit seed: admission n of this scheduler draws from stream (seed, n), RNG row 0 -- what the default policy's n-th batch-1
    call with that seed would draw with."""
    from mapperatorinator_amd.server import fresh_seed
    tok = rs.tokenizer("bench")
    eng, _, _, _ = _run(tok, [2, 2, 1], do_sample=True)
    assert [a["rng_row"] for a in eng.admitted] == [0] * 5
    assert [a["seed"] for a in eng.admitted] == [fresh_seed(9, n) for n in range(5)]
    assert eng.sessions[0].sp.do_sample == 1


@pytest.mark.parametrize("over, words", [(dict(num_beams=2), "beam search"), (dict(cfg_scale=2.0), "guidance"),
                                         (dict(cross_kv_fp8=True), "e4m3 copy of the cross K/V"),
                                         (dict(self_kv_fp8=True), "e4m3 self-attention cache"),
                                         (dict(beam_sample_fn=lambda p, k: None), "injected sampler")])
def test_host_refusals_come_before_anything_is_encoded(over, words):
    tok = rs.tokenizer("bench")
    from mapperatorinator_amd.scheduler import SequentialWindowScheduler
    eng = _Engine(tok.vocab_size_out)
    model = types.SimpleNamespace(engine=eng, config=types.SimpleNamespace(max_target_positions=24))
    got, order = {}, []
    jobs = _songs(tok, [2, 1], got, order)
    jobs[1].generate_kwargs.update(over)
    with pytest.raises(ValueError, match=words):
        SequentialWindowScheduler(model, tok, decode_batch=2, inflight=True).run(jobs)
    assert eng.encoded == 0 and not eng.sessions and not got


def test_jobs_that_differ_in_a_per_call_setting_are_refused_before_anything_is_encoded():
    tok = rs.tokenizer("bench")
    from mapperatorinator_amd.scheduler import SequentialWindowScheduler
    eng = _Engine(tok.vocab_size_out)
    model = types.SimpleNamespace(engine=eng, config=types.SimpleNamespace(max_target_positions=24))
    jobs = _songs(tok, [1, 1], {}, [])
    jobs[1].generate_kwargs.update(do_sample=True)
    with pytest.raises(ValueError, match="per-call setting"):
        SequentialWindowScheduler(model, tok, decode_batch=2, inflight=True).run(jobs)
    assert eng.encoded == 0 and not eng.sessions


def test_open_slots_refuses_the_slot_count_on_the_host():
    from mapperatorinator_amd.t5_engine import DecodeSlots
    with pytest.raises(ValueError, match="65 slots not in"):
        DecodeSlots(None, 65, None, False, 16)
