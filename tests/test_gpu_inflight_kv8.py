"""-m gpu: in-flight decode over the e4m3 K/V caches (`mh_t5_slots_open_kv8`, `T5Engine.open_slots(cross_kv_fp8=, self_kv_fp8=)`,
`SequentialWindowScheduler(inflight=True, inflight_kv_fp8=)`; contract in include/mapperhip.h).

The yardstick is the UNIFORM CALL under the same modes: `T5Engine.decode(row_sampling=..., kv_fp8=mh_t5_quantize_cross_kv of the window's
row, self_kv_fp8=...)` with B = 1, the window's own unpadded prompt and row entry.  Every comparison is bit equality: the dumped scores
after every step, the ids at retirement, the bytes and scales of both copies.  The models are the tiny goldens of
tests/test_gpu_inflight.py in bf16 storage; its helpers are used as they are.  Both session copies are filled with 0xFF bytes (NaN
e4m3, NaN scales) before every session opens, so a byte that no admission and no step of the window itself wrote cannot be read
without the scores showing it."""
import ctypes as C

import pytest
import torch

from conftest import vw_golden_case, wf_golden_case
from test_gpu_inflight import (T5_TGT, _CACHE, _Window, _cross_kv, _gk, _prompt, _row_of, _same_bits, _t5_model, _uniform)

pytestmark = pytest.mark.gpu

MODES = {"cross": dict(cross_kv_fp8=True), "self": dict(self_kv_fp8=True), "both": dict(cross_kv_fp8=True, self_kv_fp8=True)}
BF16 = torch.bfloat16


def _align256(n):
    return (n + 255) // 256 * 256


def _cross8_views(buf, eng, S):
    """the packed e4m3 cross K/V copy of S rows -> (bytes (planes, S, H, L * 64), scales (planes, S, H))"""
    d, p = eng.dims, eng.packed
    planes, n = 2 * d.n_dec_layers, 2 * d.n_dec_layers * S * d.n_heads * p.src_len * 64
    off = _align256(n)
    return (buf[:n].view(planes, S, d.n_heads, p.src_len * 64),
            buf[off:off + planes * S * d.n_heads * 4].view(torch.float32).view(planes, S, d.n_heads))


def _self8_views(buf, eng, S):
    """the e4m3 shadow of S rows -> (bytes (planes, S, H, tgt, 64), scales (planes, S, H, tgt))"""
    d, p = eng.dims, eng.packed
    planes, rows = 2 * d.n_dec_layers, 2 * d.n_dec_layers * S * d.n_heads * p.tgt_len
    off = _align256(rows * 64)
    return (buf[:rows * 64].view(planes, S, d.n_heads, p.tgt_len, 64),
            buf[off:off + rows * 4].view(torch.float32).view(planes, S, d.n_heads, p.tgt_len))


def _uniform8(m, tok, kv, w, tgt, mode, copies=False):
    """THE reference: the window alone, B = 1, under `mode` -> (ids (n,), scores (n, V)[, its copies on the host: cross bytes, cross
    scales, shadow bytes, shadow scales -- None where the mode has no such copy])"""
    from mapperatorinator_amd import _lib
    eng = m.engine
    sw = MODES[mode]
    sp, row, table = _row_of(tok, w, tgt)
    sp.max_length = tgt
    rows = (_lib.MhRowSampling * 1)()
    C.memmove(rows, C.byref(row), C.sizeof(row))
    rows[0].eos_set = 0
    kv_row = kv[:, :, w.kv_row:w.kv_row + 1].contiguous()
    eng._enter()
    with eng.on_stream():
        kv8 = eng.cross_kv_fp8(kv_row) if sw.get("cross_kv_fp8") else None
        tokens, n_out, logits = eng.decode(kv_row, w.prompt[None].to(eng.device, torch.int32),
                                           None if w.mask is None else w.mask[None].to(eng.device).to(torch.uint8), None, sp,
                                           dump_logits=True, kv_fp8=kv8, self_kv_fp8=bool(sw.get("self_kv_fp8")),
                                           row_sampling=(sp, rows, table[None]))
    eng._leave()
    eng.synchronize()
    n = int(n_out.item())
    out = (tokens[0, :n].to(torch.int64).cpu(), logits[:n, 0].cpu())
    if copies:
        c8 = [t[:, 0].cpu() for t in _cross8_views(kv8, eng, 1)] if kv8 is not None else [None, None]
        s8 = [t[:, 0].cpu() for t in _self8_views(eng._ws["skv8"], eng, 1)] if sw.get("self_kv_fp8") else [None, None]
        out += (c8 + s8,)
    return out


def _poison(eng, S):
    """both session copies, as the next session of S slots will find them: every byte 0xFF"""
    p = eng.packed
    eng._workspace("slot_cross_kv8", eng.lib.mh_t5_cross_kv_fp8_bytes(C.byref(p.cfg), S)).fill_(0xFF)
    eng._workspace("slot_skv8", eng.lib.mh_t5_self_kv_fp8_bytes(C.byref(p.cfg), S)).fill_(0xFF)
    torch.cuda.synchronize()


def _check_copies(slots, eng, slot, n, ref_copies, what):
    """slot's rows of the session copies against the B = 1 call's: the cross row and its scales; the shadow at positions 0 .. n - 2, the
    positions a row of n columns was fed at (column n - 1 is its last id: produced, never fed)"""
    torch.cuda.synchronize()
    c_bytes, c_scales, s_bytes, s_scales = ref_copies
    if slots.cross_kv8 is not None:
        b, s = _cross8_views(slots.cross_kv8, eng, slots.S)
        assert torch.equal(b[:, slot].cpu(), c_bytes), f"{what}: the e4m3 cross row differs from mh_t5_quantize_cross_kv(B = 1)"
        assert _same_bits(s[:, slot].cpu(), c_scales), f"{what}: the cross scales differ from mh_t5_quantize_cross_kv(B = 1)"
    if slots.self_kv8 is not None:
        b, s = _self8_views(slots.self_kv8, eng, slots.S)
        assert torch.equal(b[:, slot, :, :n - 1].cpu(), s_bytes[:, :, :n - 1]), f"{what}: shadow bytes below position {n - 1} differ from the B = 1 call's"
        assert _same_bits(s[:, slot, :, :n - 1].cpu().contiguous(), s_scales[:, :, :n - 1].contiguous()), f"{what}: shadow scales differ from the B = 1 call's"


def _run_kv8(m, tok, kv, windows, S, tgt, refs, mode, dump=True, copies=False):
    """The windows, in order, through S slots of a session under `mode` (lowest idle slot first), one step per run.  After every step the
    live rows' newly dumped scores, at retirement the ids (and with `copies` the slot's rows of both copies) are compared with the
    window's uniform call: equal bits.  -> (per slot its occupants, per run the live rows as (window, columns so far))"""
    eng = m.engine
    sp = _row_of(tok, windows[0], tgt)[0]
    sp.max_length = tgt
    _poison(eng, S)
    queue = list(range(len(windows)))
    occupant, seen, history, timeline = [None] * S, [0] * S, [[] for _ in range(S)], []
    with eng.open_slots(S, sp, dump_logits=dump, **MODES[mode]) as slots:
        assert (slots.cross_kv is None) == (slots.cross_kv8 is not None) == ("cross_kv_fp8" in MODES[mode])
        assert (slots.self_kv8 is not None) == ("self_kv_fp8" in MODES[mode])
        while True:
            for slot in range(S):
                if occupant[slot] is None and queue:
                    i = queue.pop(0)
                    w = windows[i]
                    _, row, table = _row_of(tok, w, tgt)
                    slots.admit(slot, kv[:, :, w.kv_row], w.prompt, w.mask, row, table)
                    occupant[slot], seen[slot] = i, w.P
                    history[slot].append(i)
            if all(o is None for o in occupant):
                break
            finished, lengths = slots.run(1)
            timeline.append([(occupant[s], lengths[s]) for s in range(S) if occupant[s] is not None])
            assert len(timeline) < 4 * tgt * len(windows), "the slots make no progress"
            for slot in range(S):
                i = occupant[slot]
                if i is None:
                    continue
                ids, scores = refs[i][0], refs[i][1]
                n = lengths[slot]
                assert 1 <= n <= ids.shape[0], (i, n, ids.shape[0])
                if dump and n > seen[slot]:
                    eng.synchronize()
                    got = slots.logits[seen[slot]:n, slot].cpu()
                    assert _same_bits(got, scores[seen[slot]:n]), \
                        f"{mode}: window {i} in slot {slot}: scores of columns {seen[slot]}..{n - 1} differ from its uniform call"
                    seen[slot] = n
                if finished[slot]:
                    if copies:
                        _check_copies(slots, eng, slot, n, refs[i][2], f"{mode}: window {i} in slot {slot}")
                    row = slots.take(slot)
                    assert torch.equal(row, ids), f"{mode}: window {i} in slot {slot}: ids differ from its uniform call\n{row.tolist()}\n{ids.tolist()}"
                    occupant[slot] = None
                else:
                    assert n < ids.shape[0], f"window {i} in slot {slot} runs on behind its uniform call's end"
    return history, timeline


# ---- 1 / 2 / 8: T5 tiny, 3 slots, 5 windows ----------------------------------------------------------------------------------------
# (prompt length, cap).  Window 1 runs to column 134: past the 128 keys of one iteration of the self-attention's key loop, and live
# while slots 0 and 2 are refilled (windows 3 and 4 enter at steps 13 / 11 with the prefill).  No EOS set: every row runs to its cap.
_WINDOWS = [(1, 14), (3, 135), (9, 20), (3, 12), (1, 10)]


def _case(mode, prefill):
    m, tok, n_samples = _t5_model(BF16, prefill)
    kv = _cross_kv(m, n_samples, 4)
    key = ("kv8case", mode, prefill)
    if key not in _CACHE:
        wins = [_Window(i % 4, _prompt(tok, P, seed=120 + i), _gk(T5_TGT, max_length=cap, temperature=1.0 + 0.05 * (i % 3)))
                for i, (P, cap) in enumerate(_WINDOWS)]
        _CACHE[key] = (wins, [_uniform8(m, tok, kv, w, T5_TGT, mode, copies=True) for w in wins])
    return (m, tok, kv) + _CACHE[key]


@pytest.mark.parametrize("prefill", [True, False], ids=["prefill", "decode_prefill_0"])
@pytest.mark.parametrize("mode", ["cross", "self", "both"])
def test_slot_rows_and_copies_match_the_uniform_call_step_by_step(mode, prefill):
    """Cases 1, 2 and 8 of the feature: scores after every step, ids and both copies at retirement.  Under "cross" the session holds no
    bf16 copy of the slots' cross K/V at all (cross_kv_slots = NULL)."""
    m, tok, kv, wins, refs = _case(mode, prefill)
    if mode != "self":      # the modes must matter: the e4m3 cross K/V moves the scores of the plain call
        if ("kv8plain", prefill) not in _CACHE:
            _CACHE[("kv8plain", prefill)] = _uniform(m, tok, kv, wins[2], T5_TGT)[1]
        assert not _same_bits(_CACHE[("kv8plain", prefill)], refs[2][1]), "the e4m3 cross K/V must change the scores"
    history, timeline = _run_kv8(m, tok, kv, wins, 3, T5_TGT, refs, mode, copies=True)
    assert [len(r[0]) for r in refs] == [cap for _, cap in _WINDOWS]
    assert sorted(len(h) for h in history) == [1, 2, 2] and history[1] == [1], history
    # refills beside window 1 mid-window, and window 1 past position 128
    assert any(any(i == 1 and 10 < n < 120 for i, n in live) and any(i in (3, 4) and n - 1 < 4 for i, n in live) for live in timeline)
    assert any(i == 1 and n - 1 > 128 for live in timeline for i, n in live)


def test_session_with_a_bf16_slot_buffer_as_well_computes_the_same():
    """The entry with BOTH cross copies (cross_kv_slots non-NULL beside sp->cross_kv_fp8: the admission then copies the bf16 row too):
    the token steps stream the e4m3 one, to the bits of the "cross" case, which runs without the bf16 buffer."""
    m, tok, kv, wins, refs = _case("cross", True)
    eng = m.engine
    d, p = eng.dims, eng.packed
    spare = torch.empty((d.n_dec_layers, 2, 3, d.n_heads, p.src_len, 64), dtype=BF16, device=eng.device)
    calls = []

    class Lib:
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if name != "mh_t5_slots_open_kv8":
                return fn

            def open_(*a):
                assert a[7] is None, "open_slots(cross_kv_fp8=True) passes no bf16 slot buffer"
                calls.append(name)
                return fn(*a[:7], spare.data_ptr(), *a[8:])
            return open_
    lib = eng.lib
    eng.lib = Lib()
    try:
        _run_kv8(m, tok, kv, wins, 3, T5_TGT, refs, "cross", copies=True)
    finally:
        eng.lib = lib
    assert calls == ["mh_t5_slots_open_kv8"]
    torch.cuda.synchronize()
    assert torch.equal(spare[:, :, 1].cpu(), kv[:, :, wins[1].kv_row].cpu()), "the bf16 slot row is the window's row as well"


# ---- 2: an admission writes its own row only; an idle slot's rows are never written ---------------------------------------------------
def test_admission_and_steps_leave_the_other_slots_rows_alone():
    m, tok, kv, wins, refs = _case("both", True)
    eng = m.engine
    sp = _row_of(tok, wins[0], T5_TGT)[0]
    sp.max_length = T5_TGT
    _poison(eng, 3)
    with eng.open_slots(3, sp, **MODES["both"]) as slots:
        views = _cross8_views(slots.cross_kv8, eng, 3) + _self8_views(slots.self_kv8, eng, 3)
        for slot, i in ((0, 1), (2, 2)):
            _, row, table = _row_of(tok, wins[i], T5_TGT)
            slots.admit(slot, kv[:, :, wins[i].kv_row], wins[i].prompt, None, row, table)
        for _ in range(6):
            slots.run(1)
        torch.cuda.synchronize()
        # slot 1 was idle through six steps: every byte of its rows is still the 0xFF the session found
        for v in views:
            assert bool((v[:, 1].contiguous().view(torch.uint8) == 0xFF).all()), "a step wrote into an idle slot's row of a copy"
        before = [v.clone() for v in views]
        _, row, table = _row_of(tok, wins[3], T5_TGT)                 # a prompt of 3 ids: the prefill, the shadow's prompt rows
        slots.admit(1, kv[:, :, wins[3].kv_row], wins[3].prompt, None, row, table)
        torch.cuda.synchronize()
        for v, b in zip(views, before):
            for other in (0, 2):
                assert torch.equal(v[:, other].contiguous().view(torch.uint8), b[:, other].contiguous().view(torch.uint8)), \
                    f"the admission into slot 1 changed slot {other}'s row of a copy"
        c_bytes, c_scales, s_bytes, s_scales = refs[3][2]
        assert torch.equal(views[0][:, 1].cpu(), c_bytes) and _same_bits(views[1][:, 1].cpu(), c_scales)
        P = wins[3].P
        assert torch.equal(views[2][:, 1, :, :P - 1].cpu(), s_bytes[:, :, :P - 1]), "positions 0 .. P - 2 of the shadow are the prompt's"
        assert _same_bits(views[3][:, 1, :, :P - 1].cpu().contiguous(), s_scales[:, :, :P - 1].contiguous())
        # ... and nothing else of the slot's shadow row was written
        assert bool((views[2][:, 1, :, P - 1:] == 0xFF).all()) and bool((views[3][:, 1, :, P - 1:].contiguous().view(torch.uint8) == 0xFF).all())


# ---- 3: stale memory -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prefill", [True, False], ids=["prefill", "decode_prefill_0"])
def test_a_short_window_behind_a_long_one_reads_nothing_stale(prefill):
    """Slot 0 holds a window of 40 positions, then one of 5: the 35 rows of both copies behind the new window's end are the old window's
    (and everything else 0xFF); slot 1 runs on beside both."""
    m, tok, n_samples = _t5_model(BF16, prefill)
    kv = _cross_kv(m, n_samples, 4)
    key = ("kv8stale", prefill)
    if key not in _CACHE:
        wins = [_Window(i, _prompt(tok, P, seed=140 + i), _gk(T5_TGT, max_length=cap)) for i, (P, cap) in enumerate([(3, 40), (1, 52), (2, 5)])]
        _CACHE[key] = (wins, [_uniform8(m, tok, kv, w, T5_TGT, "both", copies=True) for w in wins])
    wins, refs = _CACHE[key]
    history, timeline = _run_kv8(m, tok, kv, wins, 2, T5_TGT, refs, "both", copies=True)
    assert history == [[0, 2], [1]] and [len(r[0]) for r in refs] == [40, 52, 5]
    assert any({i for i, _ in live} == {1, 2} for live in timeline)


# ---- 4: two chains -------------------------------------------------------------------------------------------------------------------
def test_17_slots_second_chain_rows_match_their_uniform_calls():
    """S = 17: chains of 9 + 8 rows, 22 windows, refills in both chains.  The slots of chain 1 sit at global rows >= 9 of both copies:
    the chain's row offsets (reads, appends, the admission's row) are the global ones."""
    m, tok, n_samples = _t5_model(BF16)
    eng = m.engine
    assert eng.lib.mh_t5_decode_chains_cfg(C.byref(eng.packed.cfg), 17) == 2
    kv = _cross_kv(m, n_samples, 4)
    if "kv8case17" not in _CACHE:
        caps = {8: 6, 16: 8, 12: 10, 3: 12}
        wins = []
        for i in range(22):
            P = (1, 2, 5, 3)[i % 4]
            cap = P + caps.get(i, 14 + i % 5) if i < 17 else P + 4 + i % 3
            wins.append(_Window(i % 4, _prompt(tok, P, seed=150 + i), _gk(T5_TGT, max_length=cap)))
        _CACHE["kv8case17"] = (wins, [_uniform8(m, tok, kv, w, T5_TGT, "both", copies=True) for w in wins])
    wins, refs = _CACHE["kv8case17"]
    history, timeline = _run_kv8(m, tok, kv, wins, 17, T5_TGT, refs, "both", copies=True)
    refilled = [s for s in range(17) if len(history[s]) > 1]
    assert any(s < 9 for s in refilled) and any(s >= 9 for s in refilled), f"refills in one chain only: {history}"
    chain_of = {i: s // 9 for s in range(17) for i in history[s]}
    assert any(len({chain_of[i] for i, _ in live}) == 2 for live in timeline), "no run with a live slot in both chains"


# ---- 5: the Whisper families -----------------------------------------------------------------------------------------------------------
def _vw_bf16():
    if "kv8vw" not in _CACHE:
        from mapperatorinator_amd.modeling import MapperatorinatorHIP
        g, d, tok, sd, _ = vw_golden_case("vw_test")
        opts = dict(global_attn_every_n_layers=2, local_attention=16, local_rope_theta=1000.0)   # odd layers: 8 keys behind the query
        m = MapperatorinatorHIP(sd, d, vocab_size_in=tok.vocab_size_in, vocab_size_out=tok.vocab_size_out, n_mels=128,
                                src_seq_len=int(g["in_frames"]), tgt_seq_len=int(g["tgt_len"]), dtype=BF16, device="cuda", f_min=20,
                                backbone_options=opts)
        _CACHE["kv8vw"] = (m, tok, int(g["n_samples"]))
    return _CACHE["kv8vw"]


def _hfw_bf16():
    if "kv8hfw" not in _CACHE:
        from mapperatorinator_amd.modeling import MapperatorinatorHIP
        g, kind, d, tok, sd, _, _ = wf_golden_case("hfw_test")
        m = MapperatorinatorHIP(sd, d, vocab_size_in=tok.vocab_size_in, vocab_size_out=tok.vocab_size_out, n_mels=int(g["n_mels"]),
                                src_seq_len=int(g["in_frames"]), tgt_seq_len=int(g["tgt_len"]), dtype=BF16, device="cuda", f_min=0,
                                backbone_options=dict(decoder_positions="mask"))
        assert m.engine.kind == "hf"
        _CACHE["kv8hfw"] = (m, tok, int(g["n_samples"]))
    return _CACHE["kv8hfw"]


def test_vw_slot_past_the_local_window_beside_a_row_below_it():
    """rotary Whisper with local layers in bf16, mode both: the window start j_first and the RoPE rows are the row's own."""
    m, tok, n_samples = _vw_bf16()
    tgt = m.engine.packed.tgt_len
    kv = _cross_kv(m, n_samples, 3)
    wins = [_Window(0, _prompt(tok, 3, seed=1), _gk(tgt, max_length=40)), _Window(1, _prompt(tok, 1, seed=2), _gk(tgt, max_length=9)),
            _Window(2, _prompt(tok, 2, seed=3), _gk(tgt, max_length=12)), _Window(1, _prompt(tok, 12, seed=4), _gk(tgt, max_length=20))]
    refs = [_uniform8(m, tok, kv, w, tgt, "both", copies=True) for w in wins]
    history, timeline = _run_kv8(m, tok, kv, wins, 2, tgt, refs, "both", copies=True)
    assert refs[0][0].shape[0] == 40 and len(history[1]) == 3
    assert any(any(i == 0 and n - 1 > 8 for i, n in live) and any(i != 0 and n - 1 < 8 for i, n in live) for live in timeline)
    assert any(any(i == 0 and n - 1 > 24 for i, n in live) and any(i == 3 for i, n in live) for live in timeline)


def test_hfw_slot_with_a_masked_first_column():
    """HF Whisper (LayerNorm prologue) in bf16, mode both, learned positions from the mask, a masked first column."""
    m, tok, n_samples = _hfw_bf16()
    assert m.engine.packed.cfg.dec_pos_from_mask == 1
    tgt = m.engine.packed.tgt_len
    kv = _cross_kv(m, n_samples, 3)
    one = torch.tensor
    wins = [_Window(0, one([0, 1, 9]), _gk(tgt, max_length=30), mask=one([0, 1, 1])),
            _Window(1, one([1, 40, 700]), _gk(tgt, max_length=12)),
            _Window(2, one([0, 0, 1]), _gk(tgt, max_length=16), mask=one([0, 0, 1])),
            _Window(0, one([1, 9]), _gk(tgt, max_length=20))]
    refs = [_uniform8(m, tok, kv, w, tgt, "both", copies=True) for w in wins]
    _run_kv8(m, tok, kv, wins, 2, tgt, refs, "both", copies=True)


# ---- 6: the scheduler ----------------------------------------------------------------------------------------------------------------
def test_inflight_kv_fp8_scheduler_matches_sequential_loop():
    """Three songs of 2, 3 and 4 dependent windows through `SequentialWindowScheduler(inflight=True, inflight_kv_fp8="both")` with 2
    slots == the reference-shaped loop (one batch-1 `model_generate` per window, in order) run with cross_kv_fp8=True, self_kv_fp8=True."""
    from mapperatorinator_amd.scheduler import SequentialWindowScheduler, SongJob
    from mapperatorinator_amd.server import model_generate
    from mh_testing import synthetic_audio
    m, tok, n_samples = _t5_model(BF16)
    n_windows = [2, 3, 4]
    songs = [synthetic_audio(n, n_samples, seed=40 + k) for k, n in enumerate(n_windows)]

    def kwargs_for(w, n, **modes):
        kw = _gk(48, lookback_time=400 if w != 0 else 0, lookahead_time=3000 if w != n - 1 else 0, temperature=0.9, precision="bf16", **modes)
        kw.pop("conditional_temperature_per_row")
        return kw

    def prompt_from(prev):
        if prev is None:
            return torch.tensor([[tok.sos_id]])
        return torch.tensor([[tok.sos_id] + [t for t in prev.tolist() if t > 2][-3:]])

    want = []
    for k, n in enumerate(n_windows):
        prev, rows = None, []
        for w in range(n):
            prompt = prompt_from(prev)
            ids, _ = model_generate(m, tok, dict(inputs=songs[k][w:w + 1], decoder_input_ids=prompt, decoder_attention_mask=prompt.ne(0)),
                                    kwargs_for(w, n, cross_kv_fp8=True, self_kv_fp8=True))
            prev = ids[0, prompt.shape[1]:]
            rows.append(ids[0])
        want.append(rows)

    got, state, order = [[None] * n for n in n_windows], [None] * 3, []

    def make_job(k, n):
        def prompt_fn(w):
            return dict(decoder_input_ids=prompt_from(state[k]), generate_kwargs=kwargs_for(w, n))

        def on_result(w, row, st):
            p = prompt_from(state[k]).shape[1]
            got[k][w] = row
            state[k] = row[p:]
            order.append((k, w))
        return SongJob(frames=songs[k], prompt_fn=prompt_fn, on_result=on_result)

    _poison(m.engine, 2)
    sched = SequentialWindowScheduler(m, tok, encode_batch=4, decode_batch=2, inflight=True, inflight_steps=4, inflight_kv_fp8="both")
    stats = sched.run([make_job(k, n) for k, n in enumerate(n_windows)])
    assert stats["windows"] == stats["admissions"] == 9 and stats["decode_steps"] > 0
    for k, n in enumerate(n_windows):
        assert [w for kk, w in order if kk == k] == list(range(n)), order
        for w in range(n):
            a, b = got[k][w], want[k][w]
            assert a.shape == b.shape and torch.equal(a, b), (k, w, a.tolist(), b.tolist())


# ---- 7: refusals at the ABI ----------------------------------------------------------------------------------------------------------
def test_new_entry_refuses_and_launches_nothing():
    from mapperatorinator_amd import _lib
    from mapperatorinator_amd.server import build_row_sampling
    S = 2
    hits, misses = C.c_long(), C.c_long()

    def sampling(tok, **over):
        sp = build_row_sampling(tok, [_gk(T5_TGT, **over)], T5_TGT)[0]
        sp.max_length = T5_TGT
        return sp
    for dtype in (BF16, torch.float32):
        m, tok, _ = _t5_model(dtype)
        eng, lib, p = m.engine, m.engine.lib, m.engine.packed
        d = eng.dims
        rows_d = torch.zeros(64 * 64, dtype=torch.uint8, device="cuda")
        eos_d = torch.zeros(64 * p.vocab_out, dtype=torch.uint8, device="cuda")
        kv_d = torch.zeros((d.n_dec_layers, 2, S, d.n_heads, p.src_len, 64), dtype=eng.dtype, device="cuda")
        tokens = torch.zeros((S, T5_TGT), dtype=torch.int32, device="cuda")
        ws = torch.empty(lib.mh_t5_slots_workspace_bytes(C.byref(p.cfg), S), dtype=torch.uint8, device="cuda")
        copy8 = torch.empty(1 << 22, dtype=torch.uint8, device="cuda")        # (stands for either copy: a refused open reads neither)
        torch.cuda.synchronize()
        launches = lib.mh_t5_decode_tail_launches()
        lib.mh_t5_step_graph_cache_stats(C.byref(hits), C.byref(misses), 0)
        before = (hits.value, misses.value)

        def open_(sp, S_=S, forced_=None, skv8=None, kv=kv_d):
            h = C.c_void_p()
            rc = lib.mh_t5_slots_open_kv8(C.byref(p.cfg), C.byref(p.w), S_, C.byref(sp), rows_d.data_ptr(), eos_d.data_ptr(), 64, _lib.ptr(kv),
                                          tokens.data_ptr(), None, _lib.ptr(forced_), _lib.ptr(skv8), ws.data_ptr(), ws.numel(), 16, eng._s(),
                                          C.byref(h))
            assert rc == -1 and not h
            return lib.mh_last_error()
        if dtype == torch.float32:
            sp = sampling(tok)
            sp.cross_kv_fp8 = copy8.data_ptr()
            assert b"mh_t5_slots_open_kv8: cross_kv_fp8 needs bf16 storage" in open_(sp)
            assert b"mh_t5_slots_open_kv8: the e4m3 self-attention cache needs bf16 storage" in open_(sampling(tok), skv8=copy8)
        else:
            sp = sampling(tok)
            sp.cfg_scale, sp.cross_kv_fp8 = 2.0, copy8.data_ptr()
            assert b"guidance has no slot form" in open_(sp, skv8=copy8)
            forced = torch.zeros((S, T5_TGT), dtype=torch.int32, device="cuda")
            assert b"forced ids) has no slot form" in open_(sampling(tok), forced_=forced, skv8=copy8)
            assert b"65 slots not in [1, 64]" in open_(sampling(tok), S_=65, skv8=copy8)
            assert b"cross_kv_slots may be NULL only where sp->cross_kv_fp8" in open_(sampling(tok), skv8=copy8, kv=None)
            assert b"null argument" in open_(sampling(tok), kv=None)
        lib.mh_t5_step_graph_cache_stats(C.byref(hits), C.byref(misses), 0)
        assert (hits.value, misses.value) == before and lib.mh_t5_decode_tail_launches() == launches, "a refused open built or ran a step"
