"""-m gpu: in-flight decode (`mh_t5_slots_*`, `T5Engine.open_slots`, `SequentialWindowScheduler(inflight=True)`; contract in
include/mapperhip.h).

The yardstick throughout is the UNIFORM CALL: `T5Engine.decode(row_sampling=...)` with B = 1, the window's own unpadded prompt and
its own row entry.  Rows are batch-invariant in this engine, so a slot row must reproduce it bit for bit: the dumped scores of every
column it produced, after every step, and its token ids when it retires.  The models are those of the tiny goldens
(tests/golden/t5_tiny.npz, vw_test.npz, hfw_test.npz: seeded weights) at their own sizes; the T5 one gets 160 target positions so
that a row can pass the 128-key iteration of the self-attention's key loop."""
import contextlib
import ctypes as C

import pytest
import torch

from conftest import t5_golden_case, vw_golden_case, wf_golden_case

pytestmark = pytest.mark.gpu

T5_TGT = 160


# ---- models, windows, the uniform call ----------------------------------------------------------------------------------------------
_CACHE = {}


def _t5_model(dtype, prefill=True):
    key = ("t5", dtype, prefill)
    if key not in _CACHE:
        from mapperatorinator_amd.modeling import MapperatorinatorHIP
        from mapperatorinator_amd.t5_engine import T5_PRESETS
        g, size, tok, sd, _, src, _ = t5_golden_case("t5_tiny")
        m = MapperatorinatorHIP(sd, T5_PRESETS[size], vocab_size_in=tok.vocab_size_in, vocab_size_out=tok.vocab_size_out, src_seq_len=src,
                                tgt_seq_len=T5_TGT, dtype=dtype, device="cuda", options=None if prefill else {"decode_prefill": 0})
        _CACHE[key] = (m, tok, int(g["n_samples"]))
    return _CACHE[key]


def _vw_model():
    if "vw" not in _CACHE:
        from mapperatorinator_amd.modeling import MapperatorinatorHIP
        g, d, tok, sd, _ = vw_golden_case("vw_test")
        opts = dict(global_attn_every_n_layers=2, local_attention=16, local_rope_theta=1000.0)   # odd layers: 8 keys behind the query
        m = MapperatorinatorHIP(sd, d, vocab_size_in=tok.vocab_size_in, vocab_size_out=tok.vocab_size_out, n_mels=128,
                                src_seq_len=int(g["in_frames"]), tgt_seq_len=int(g["tgt_len"]), dtype=torch.float32, device="cuda", f_min=20,
                                backbone_options=opts)
        _CACHE["vw"] = (m, tok, int(g["n_samples"]))
    return _CACHE["vw"]


def _hfw_model():
    if "hfw" not in _CACHE:
        from mapperatorinator_amd.modeling import MapperatorinatorHIP
        g, kind, d, tok, sd, _, _ = wf_golden_case("hfw_test")
        m = MapperatorinatorHIP(sd, d, vocab_size_in=tok.vocab_size_in, vocab_size_out=tok.vocab_size_out, n_mels=int(g["n_mels"]),
                                src_seq_len=int(g["in_frames"]), tgt_seq_len=int(g["tgt_len"]), dtype=torch.float32, device="cuda", f_min=0,
                                backbone_options=dict(decoder_positions="mask"))
        assert m.engine.kind == "hf"
        _CACHE["hfw"] = (m, tok, int(g["n_samples"]))
    return _CACHE["hfw"]


def _cross_kv(m, n_samples, n):
    """resident cross K/V of n windows of varied audio, once per model"""
    key = ("kv", id(m), n)
    if key not in _CACHE:
        from mh_testing import synthetic_audio_varied
        eng = m.engine
        audio = synthetic_audio_varied(n, n_samples, seed=6)
        eng._enter()
        with eng.on_stream():
            kv = eng.cross_kv(eng.encode_mel(eng.mel(audio.to(eng.device, torch.float32))))
        eng._leave()
        eng.synchronize()
        _CACHE[key] = kv
    return _CACHE[key]


def _prompt(tok, P, seed):
    """sos, then P - 1 ids that are no time shift and no EOS"""
    from mapperatorinator_amd.server import _ev
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(_ev(tok.event_end, "TIME_SHIFT"), tok.vocab_size_out, (P,), generator=g)
    ids[0] = tok.sos_id
    return ids


def _gk(tgt, **over):
    kw = dict(precision="fp32", do_sample=False, num_beams=1, top_p=1.0, top_k=0, max_length=tgt, cfg_scale=1.0, timeshift_bias=0,
              types_first=False, temperature=1.0, lookback_time=0, lookahead_time=0, context_type="map", pad_token_id=0,
              conditional_temperature_per_row=True)
    kw.update(over)
    return kw


class _Window:
    """One window: its cross K/V row, unpadded prompt (and mask), kwargs, and whether its EOS set is the kwargs' own (`eos`: True),
    empty (False: the row runs to its cap) or a given id list."""

    def __init__(self, kv_row, prompt, gk, mask=None, eos=False):
        self.kv_row, self.prompt, self.gk, self.mask, self.eos = kv_row, prompt, gk, mask, eos
        self.P = int(prompt.shape[0])


def _row_of(tok, w, tgt):
    """-> (per-call settings, row entry, EOS table) of one window, as `server.build_row_sampling` makes them"""
    from mapperatorinator_amd.server import build_row_sampling
    sp, rows, tables = build_row_sampling(tok, [w.gk], tgt)
    table = tables[rows[0].eos_set].clone()
    if w.eos is False:
        table.zero_()
    elif w.eos is not True:
        table[torch.as_tensor(w.eos, dtype=torch.long)] = 1
    return sp, rows[0], table


def _uniform(m, tok, kv, w, tgt):
    """THE reference: the window alone through `T5Engine.decode(row_sampling=)` with B = 1 -> (ids (n,), scores (n, V))"""
    from mapperatorinator_amd import _lib
    eng = m.engine
    sp, row, table = _row_of(tok, w, tgt)
    sp.max_length = tgt                                   # the stride of the session's buffers: the same per-call settings
    rows = (_lib.MhRowSampling * 1)()
    C.memmove(rows, C.byref(row), C.sizeof(row))
    rows[0].eos_set = 0
    eng._enter()
    with eng.on_stream():
        tokens, n_out, logits = eng.decode(kv[:, :, w.kv_row:w.kv_row + 1].contiguous(), w.prompt[None].to(eng.device, torch.int32),
                                           None if w.mask is None else w.mask[None].to(eng.device).to(torch.uint8), None, sp,
                                           dump_logits=True, row_sampling=(sp, rows, table[None]))
    eng._leave()
    eng.synchronize()
    n = int(n_out.item())
    return tokens[0, :n].to(torch.int64).cpu(), logits[:n, 0].cpu()


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _run_inflight(m, tok, kv, windows, S, tgt, refs, dump=True, steps_per_run=1):
    """The windows, in order, through S slots (lowest idle slot first).  After every `run`, every live row's dumped scores so far and,
    at retirement, its ids are compared with its uniform call: equal bits.  -> records: per slot its occupants, and per run the
    positions (fed next) of the live rows as (window, columns so far)."""
    eng = m.engine
    sp = _row_of(tok, windows[0], tgt)[0]
    sp.max_length = tgt
    queue = list(range(len(windows)))
    occupant, history, timeline = [None] * S, [[] for _ in range(S)], []
    with eng.open_slots(S, sp, dump_logits=dump) as slots:
        while True:
            for slot in range(S):
                if occupant[slot] is None and queue:
                    i = queue.pop(0)
                    w = windows[i]
                    _, row, table = _row_of(tok, w, tgt)
                    slots.admit(slot, kv[:, :, w.kv_row], w.prompt, w.mask, row, table)
                    occupant[slot] = i
                    history[slot].append(i)
            if all(o is None for o in occupant):
                break
            finished, lengths = slots.run(steps_per_run)
            timeline.append([(occupant[s], lengths[s]) for s in range(S) if occupant[s] is not None])
            assert len(timeline) < 4 * tgt * len(windows), "the slots make no progress"
            for slot in range(S):
                i = occupant[slot]
                if i is None:
                    continue
                ids, scores = refs[i]
                n, P = lengths[slot], windows[i].P
                assert 1 <= n <= ids.shape[0], (i, n, ids.shape[0])     # (n < P: option decode_prefill = 0 is still feeding the prompt)
                if dump and n > P:
                    eng.synchronize()
                    got = slots.logits[P:n, slot].cpu()
                    assert _same_bits(got, scores[P:n]), f"window {i} in slot {slot}: scores of columns {P}..{n - 1} differ from its uniform call"
                if finished[slot]:
                    row = slots.take(slot)
                    assert torch.equal(row, ids), f"window {i} in slot {slot}: ids differ from its uniform call\n{row.tolist()}\n{ids.tolist()}"
                    occupant[slot] = None
                else:
                    assert n < ids.shape[0], f"window {i} in slot {slot} runs on behind its uniform call's end"
            stats = dict(slots.stats)
    return history, timeline, stats


# ---- 1 / 2: T5 tiny, S = 3, 8 windows ----------------------------------------------------------------------------------------------
# (prompt length, cap): chosen with a host simulation of the admission policy so that, with and without the prompt prefill, a slot is
# used three times with a third occupant shorter than its second (stale keys behind the new row's end) and a window is admitted while
# window 1 is past position 128.  Window 1 has no EOS set and runs to column 140.
_T5_WINDOWS = [(1, 62), (40, 141), (5, 75), (17, 65), (2, 30), (5, 17), (1, 7), (2, 7)]


def _t5_windows(tok, sample):
    over = dict(do_sample=True, top_p=0.9, seed=1234) if sample else {}
    wins = []
    for i, (P, cap) in enumerate(_T5_WINDOWS):
        gk = _gk(T5_TGT, max_length=cap, temperature=1.0 + 0.05 * (i % 3), **over)
        if sample:
            gk["seed_call_index"] = i                      # per-row seeds
        wins.append(_Window(i % 4, _prompt(tok, P, seed=20 + i), gk, eos=(i == 7)))
    return wins


def _t5_case(dtype, prefill, sample):
    m, tok, n_samples = _t5_model(dtype, prefill)
    kv = _cross_kv(m, n_samples, 4)
    key = ("t5case", dtype, prefill, sample)
    if key not in _CACHE:
        wins = _t5_windows(tok, sample)
        # the last window ends by an EOS id: the id its row emits three columns behind its prompt, found with a run without EOS set
        probe = _Window(wins[7].kv_row, wins[7].prompt, wins[7].gk, eos=False)
        ids, _ = _uniform(m, tok, kv, probe, T5_TGT)
        wins[7].eos = [int(ids[wins[7].P + 3])]
        _CACHE[key] = (wins, [_uniform(m, tok, kv, w, T5_TGT) for w in wins])
    return (m, tok, kv) + _CACHE[key]


def _check_t5_timeline(wins, refs, history, timeline):
    assert refs[1][0].shape[0] == 141, "window 1 must run to column 140"
    assert refs[7][0].shape[0] <= wins[7].P + 4, "window 7 must end by its EOS id"
    lengths = {len(r[0]) for r in refs}
    assert len(lengths) >= 6, "the rows must retire at different steps"
    assert any(len(h) >= 3 and refs[h[2]][0].shape[0] < refs[h[1]][0].shape[0] for h in history), \
        f"no slot with a third occupant shorter than its second: {history}"
    # columns so far n -> the position fed next is n - 1: window 1 past position 128 beside a freshly admitted row below position 8
    assert any(any(i == 1 and n - 1 > 128 for i, n in live) and any(i != 1 and n - 1 < 8 for i, n in live) for live in timeline), \
        "no step with window 1 past position 128 beside a row below position 8"


@pytest.mark.parametrize("prefill", [True, False], ids=["prefill", "decode_prefill_0"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_t5_slots_match_the_uniform_call_step_by_step(dtype, prefill):
    """Greedy rows, S = 3, 8 windows with prompts of 1, 2, 5, 17 and 40 ids, one `run(1)` at a time: after each step the live rows'
    dumped scores, at retirement the ids, equal the uniform call's bits.  Under option decode_prefill = 0 the prompts are fed token
    by token (the sampler's "still inside the prompt" branch with the row's own prompt length)."""
    m, tok, kv, wins, refs = _t5_case(dtype, prefill, sample=False)
    history, timeline, stats = _run_inflight(m, tok, kv, wins, 3, T5_TGT, refs)
    _check_t5_timeline(wins, refs, history, timeline)
    assert stats["admissions"] == 8 and stats["steps"] == len(timeline)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_t5_sampled_slots_draw_what_the_uniform_call_draws(dtype):
    """do_sample, top_p = 0.9, a seed per row: the draw is keyed by (seed, RNG row, the row's OWN column)."""
    m, tok, kv, wins, refs = _t5_case(dtype, True, sample=True)
    greedy = _t5_case(dtype, True, sample=False)[4]
    assert any(not torch.equal(a[0], b[0]) for a, b in zip(refs, greedy)), "the sampled case must differ from the greedy one"
    history, timeline, _ = _run_inflight(m, tok, kv, wins, 3, T5_TGT, refs)
    _check_t5_timeline(wins, refs, history, timeline)


# ---- 3: two chains -------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _launch_threads(eng, value):
    """the engine option decode_launch_threads for the block: 1 (the default) = a launcher thread per chain, 0 = one thread feeds all"""
    eng.options["decode_launch_threads"] = value
    try:
        yield
    finally:
        eng.options.clear("decode_launch_threads")


@pytest.mark.parametrize("launch_threads", [1, 0], ids=["launch_threads_1", "launch_threads_0"])
def test_17_slots_are_two_chains_with_refills_in_both(launch_threads):
    """S = 17: chains of 9 + 8 rows.  22 windows; the first retirements are the last row of chain 0 (slot 8) and slots of chain 1.
    With one launcher thread per chain and with one for both: a chain's replay count depends only on its own polls, so the session
    counts the same replays -- one per `run(1)` and chain that holds a live slot."""
    m, tok, n_samples = _t5_model(torch.float32)
    assert m.engine.lib.mh_t5_decode_chains_cfg(C.byref(m.engine.packed.cfg), 17) == 2
    kv = _cross_kv(m, n_samples, 4)
    if "case17" not in _CACHE:
        caps = {8: 6, 16: 8, 12: 10, 3: 12}                               # slot of the first round -> a short cap
        wins = []
        for i in range(22):
            P = (1, 2, 5, 3)[i % 4]
            cap = P + caps.get(i, 14 + i % 5) if i < 17 else P + 4 + i % 3
            wins.append(_Window(i % 4, _prompt(tok, P, seed=50 + i), _gk(T5_TGT, max_length=cap), eos=(i % 2 == 0)))
        _CACHE["case17"] = (wins, [_uniform(m, tok, kv, w, T5_TGT) for w in wins])
    wins, refs = _CACHE["case17"]
    with _launch_threads(m.engine, launch_threads):
        assert m.engine.lib.mh_t5_decode_chains_cfg(C.byref(m.engine.packed.cfg), 17) == 2
        history, timeline, stats = _run_inflight(m, tok, kv, wins, 17, T5_TGT, refs, dump=False)
    refilled = [s for s in range(17) if len(history[s]) > 1]
    assert any(s < 9 for s in refilled) and any(s >= 9 for s in refilled), f"refills in one chain only: {history}"
    assert 8 in refilled or 16 in refilled, f"no refill in a chain's last row: {history}"
    assert stats["admissions"] == 22
    chain_of = {i: s // 9 for s in range(17) for i in history[s]}
    want_steps = sum(len({chain_of[i] for i, _ in live}) for live in timeline)
    assert any(len({chain_of[i] for i, _ in live}) == 2 for live in timeline), "no run with a live slot in both chains"
    assert stats["steps"] == want_steps, (launch_threads, stats, want_steps)
    seen = _CACHE.setdefault("steps17", {})
    seen[launch_threads] = stats["steps"]
    assert len(set(seen.values())) == 1, f"the replay count depends on decode_launch_threads: {seen}"


# ---- 3b: the uniform call over two chains, one launcher thread per chain and one for both -----------------------------------------------
def _two_chain_case(sample):
    """B = 18 through the row-settings entry: rows 0..8 (chain 0) capped near 30 columns, rows 9..17 (chain 1) near 10, no EOS set
    -> (windows, their B = 1 uniform calls)"""
    m, tok, n_samples = _t5_model(torch.float32)
    kv = _cross_kv(m, n_samples, 4)
    key = ("two_chains", sample)
    if key not in _CACHE:
        wins = []
        for i in range(18):
            gk = _gk(T5_TGT, max_length=(28 + i % 5) if i < 9 else (9 + i % 3), temperature=1.0 + 0.05 * (i % 3))
            if sample:
                gk.update(do_sample=True, top_p=0.9, seed=4321, seed_call_index=i)
            wins.append(_Window(i % 4, _prompt(tok, 3, seed=80 + i), gk))
        _CACHE[key] = (wins, [_uniform(m, tok, kv, w, T5_TGT) for w in wins])
    return (m, tok, kv) + _CACHE[key]


@pytest.mark.parametrize("sample", [False, True], ids=["greedy", "sampled"])
def test_uniform_call_two_chains_one_launcher_or_two(sample):
    """`mh_t5_generate_rows`, B = 18 = chains of 9 + 9 rows, poll_every = 4: chain 1 (caps near 10) stops at a poll long before chain 0
    (caps near 30).  Under the engine option decode_launch_threads = 1 (a launcher thread per chain) and = 0 (one thread feeds both,
    burst by burst) the ids and the returned column count are the same bits, and every row's ids are its B = 1 uniform call's."""
    from mapperatorinator_amd import _lib
    m, tok, kv, wins, refs = _two_chain_case(sample)
    eng = m.engine
    B = len(wins)
    assert eng.lib.mh_t5_decode_chains_cfg(C.byref(eng.packed.cfg), B) == 2
    entries = [_row_of(tok, w, T5_TGT) for w in wins]
    sp = entries[0][0]
    sp.max_length = T5_TGT
    rows = (_lib.MhRowSampling * B)()
    for b, (_, row, _) in enumerate(entries):
        C.memmove(C.byref(rows, b * C.sizeof(row)), C.byref(row), C.sizeof(row))
        rows[b].eos_set = b
    tables = torch.stack([e[2] for e in entries])
    prompt = torch.stack([w.prompt for w in wins]).to(eng.device, torch.int32)
    kv_rows = kv[:, :, [w.kv_row for w in wins]].contiguous()
    got = {}
    for launch_threads in (1, 0):
        with _launch_threads(eng, launch_threads):
            assert eng.lib.mh_t5_decode_chains_cfg(C.byref(eng.packed.cfg), B) == 2
            eng._enter()
            with eng.on_stream():
                tokens, n_out, _ = eng.decode(kv_rows, prompt, None, None, sp, poll_every=4, row_sampling=(sp, rows, tables))
            eng._leave()
            eng.synchronize()
        got[launch_threads] = (tokens.cpu(), int(n_out.item()))
    assert got[0][1] == got[1][1], f"returned columns: {got[1][1]} with a launcher per chain, {got[0][1]} with one"
    assert torch.equal(got[0][0], got[1][0]), "the ids depend on decode_launch_threads"
    lengths = [int(ids.shape[0]) for ids, _ in refs]
    assert max(lengths[9:]) + 12 < min(lengths[:9]), lengths           # chain 1 is done at least three polls before chain 0
    if sample:
        greedy = _two_chain_case(False)[4]
        assert any(not torch.equal(a[0], b[0]) for a, b in zip(refs, greedy)), "the sampled case must differ from the greedy one"
    for launch_threads, (tokens, n_cols) in got.items():
        assert n_cols == max(lengths), (launch_threads, n_cols, lengths)
        for b, (ids, _) in enumerate(refs):
            assert torch.equal(tokens[b, :lengths[b]].to(torch.int64), ids), \
                f"decode_launch_threads = {launch_threads}: row {b} differs from its uniform call\n{tokens[b].tolist()}\n{ids.tolist()}"


# ---- 4 / 5: the Whisper families ----------------------------------------------------------------------------------------------------
def test_vw_slot_past_the_local_window_beside_a_row_below_it():
    """rotary Whisper with local layers (8 keys behind the query): a row decoded to column 39 -- its window start moves, its RoPE rows
    are its own -- beside freshly admitted rows still inside the window."""
    m, tok, n_samples = _vw_model()
    tgt = m.engine.packed.tgt_len
    kv = _cross_kv(m, n_samples, 3)
    wins = [_Window(0, _prompt(tok, 3, seed=1), _gk(tgt, max_length=40)), _Window(1, _prompt(tok, 1, seed=2), _gk(tgt, max_length=9)),
            _Window(2, _prompt(tok, 2, seed=3), _gk(tgt, max_length=12)), _Window(1, _prompt(tok, 12, seed=4), _gk(tgt, max_length=20))]
    refs = [_uniform(m, tok, kv, w, tgt) for w in wins]
    history, timeline, _ = _run_inflight(m, tok, kv, wins, 2, tgt, refs)
    assert refs[0][0].shape[0] == 40 and len(history[1]) == 3
    assert any(any(i == 0 and n - 1 > 8 for i, n in live) and any(i != 0 and n - 1 < 8 for i, n in live) for live in timeline)
    assert any(any(i == 0 and n - 1 > 24 for i, n in live) and any(i == 3 for i, n in live) for live in timeline)


def test_hfw_slot_with_a_masked_first_column():
    """HF Whisper: learned positions come from the mask (a masked first column shifts them by one); the slot's mask row and pos_off
    are the row's own."""
    m, tok, n_samples = _hfw_model()
    assert m.engine.packed.cfg.dec_pos_from_mask == 1
    tgt = m.engine.packed.tgt_len
    kv = _cross_kv(m, n_samples, 3)
    one = torch.tensor
    wins = [_Window(0, one([0, 1, 9]), _gk(tgt, max_length=30), mask=one([0, 1, 1])),
            _Window(1, one([1, 40, 700]), _gk(tgt, max_length=12)),
            _Window(2, one([0, 0, 1]), _gk(tgt, max_length=16), mask=one([0, 0, 1])),
            _Window(0, one([1, 9]), _gk(tgt, max_length=20))]
    refs = [_uniform(m, tok, kv, w, tgt) for w in wins]
    unmasked = _uniform(m, tok, kv, _Window(0, one([0, 1, 9]), _gk(tgt, max_length=30)), tgt)
    assert not _same_bits(unmasked[1][3:], refs[0][1][3:]), "the mask must move the positions"
    _run_inflight(m, tok, kv, wins, 2, tgt, refs)


# ---- 6: the scheduler ----------------------------------------------------------------------------------------------------------------
def test_inflight_scheduler_matches_sequential_loop():
    """Three songs of 2, 3 and 5 dependent windows through `SequentialWindowScheduler(inflight=True)` with 2 slots == the
    reference-shaped loop (one batch-1 `model_generate` per window, in order), as test_window_scheduler_matches_sequential_loop checks
    the waves.  Each prompt is built from the previous window's output."""
    from mapperatorinator_amd.scheduler import SequentialWindowScheduler, SongJob
    from mapperatorinator_amd.server import model_generate
    from mh_testing import synthetic_audio
    m, tok, n_samples = _t5_model(torch.float32)
    n_windows = [2, 3, 5]
    songs = [synthetic_audio(n, n_samples, seed=40 + k) for k, n in enumerate(n_windows)]

    def kwargs_for(w, n):
        kw = _gk(48, lookback_time=400 if w != 0 else 0, lookahead_time=3000 if w != n - 1 else 0, temperature=0.9)
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
                                    kwargs_for(w, n))
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
            assert st["generated_tokens"] == int((row[p:] != 0).sum())
        return SongJob(frames=songs[k], prompt_fn=prompt_fn, on_result=on_result)

    sched = SequentialWindowScheduler(m, tok, encode_batch=4, decode_batch=2, inflight=True, inflight_steps=4)
    stats = sched.run([make_job(k, n) for k, n in enumerate(n_windows)])
    assert stats["windows"] == stats["admissions"] == 10 and stats["decode_steps"] > 0
    for k, n in enumerate(n_windows):
        assert [w for kk, w in order if kk == k] == list(range(n)), order
        for w in range(n):
            a, b = got[k][w], want[k][w]
            assert a.shape == b.shape and torch.equal(a, b), (k, w, a.tolist(), b.tolist())


# ---- 7: refusals at the ABI ----------------------------------------------------------------------------------------------------------
def test_library_refuses_what_has_no_slot_form_and_launches_nothing():
    from mapperatorinator_amd import _lib
    from mapperatorinator_amd.server import build_row_sampling
    m, tok, n_samples = _t5_model(torch.float32)
    eng, lib, p = m.engine, m.engine.lib, m.engine.packed
    kv = _cross_kv(m, n_samples, 4)
    d = eng.dims
    S = 2
    rows_d = torch.zeros(64 * 64, dtype=torch.uint8, device="cuda")
    eos_d = torch.zeros(64 * p.vocab_out, dtype=torch.uint8, device="cuda")
    kv_d = torch.zeros((d.n_dec_layers, 2, S, d.n_heads, p.src_len, 64), dtype=eng.dtype, device="cuda")
    tokens = torch.zeros((S, T5_TGT), dtype=torch.int32, device="cuda")
    forced = torch.zeros((S, T5_TGT), dtype=torch.int32, device="cuda")
    ws = torch.empty(lib.mh_t5_slots_workspace_bytes(C.byref(p.cfg), S), dtype=torch.uint8, device="cuda")
    assert lib.mh_t5_slots_workspace_bytes(C.byref(p.cfg), 65) == -1
    torch.cuda.synchronize()
    launches = lib.mh_t5_decode_tail_launches()
    hits, misses = C.c_long(), C.c_long()
    lib.mh_t5_step_graph_cache_stats(C.byref(hits), C.byref(misses), 0)
    before = (hits.value, misses.value)

    def open_(sp, S_=S, forced_=None, skv8=None):
        h = C.c_void_p()
        rc = lib.mh_t5_slots_open(C.byref(p.cfg), C.byref(p.w), S_, C.byref(sp), rows_d.data_ptr(), eos_d.data_ptr(), 64, kv_d.data_ptr(),
                                  tokens.data_ptr(), None, _lib.ptr(forced_), _lib.ptr(skv8), ws.data_ptr(), ws.numel(), 16, eng._s(), C.byref(h))
        return rc, h, lib.mh_last_error()

    def sampling(**over):
        sp = build_row_sampling(tok, [_gk(T5_TGT, **over)], T5_TGT)[0]
        sp.max_length = T5_TGT
        return sp
    ERR_ARG = -1
    sp = sampling()
    sp.cfg_scale = 2.0
    rc, h, msg = open_(sp)
    assert rc == ERR_ARG and not h and b"guidance has no slot form" in msg
    rc, h, msg = open_(sampling(), forced_=forced)
    assert rc == ERR_ARG and not h and b"forced ids) has no slot form" in msg
    sp = sampling()
    sp.cross_kv_fp8 = rows_d.data_ptr()
    rc, h, msg = open_(sp)
    assert rc == ERR_ARG and not h and b"cross_kv_fp8) has no slot form" in msg
    rc, h, msg = open_(sampling(), skv8=rows_d)
    assert rc == ERR_ARG and not h and b"shadow of the self-attention cache has no slot form" in msg
    sp = sampling()
    sp.n_cond, sp.cond_per_row, sp.tok_flags = 1, 0, rows_d.data_ptr()
    sp.cond_temp[0], sp.cond_offset[0] = 0.5, 1
    rc, h, msg = open_(sp)
    assert rc == ERR_ARG and not h and b"cond_per_row = 1" in msg
    rc, h, msg = open_(sampling(), S_=65)
    assert rc == ERR_ARG and not h and b"65 slots not in [1, 64]" in msg
    lib.mh_t5_step_graph_cache_stats(C.byref(hits), C.byref(misses), 0)
    assert (hits.value, misses.value) == before and lib.mh_t5_decode_tail_launches() == launches, "a refused open built or ran a step"
    # admit into a live slot
    w = _Window(0, _prompt(tok, 3, seed=9), _gk(T5_TGT, max_length=12))
    _, row, table = _row_of(tok, w, T5_TGT)
    with eng.open_slots(2, sampling()) as slots:
        slots.admit(0, kv[:, :, 0], w.prompt, None, row, table)
        prompt_d = w.prompt.to("cuda", torch.int32)
        kv_row = kv[:, :, 0:1].contiguous()
        torch.cuda.synchronize()
        assert lib.mh_t5_slots_admit(slots._handle, 0, kv_row.data_ptr(), prompt_d.data_ptr(), None, 3, None) == ERR_ARG
        assert b"slot 0 is live" in lib.mh_last_error()
        assert lib.mh_t5_slots_admit(slots._handle, 2, kv_row.data_ptr(), prompt_d.data_ptr(), None, 3, None) == ERR_ARG
        assert lib.mh_t5_slots_release(slots._handle, 1) == ERR_ARG and b"slot 1 is idle" in lib.mh_last_error()
        with pytest.raises(ValueError):
            slots.admit(0, kv[:, :, 0], w.prompt, None, row, table)
        finished, lengths = slots.run(16)
        assert finished == [True, False] and lengths[1] == 0 and lengths[0] == 12
