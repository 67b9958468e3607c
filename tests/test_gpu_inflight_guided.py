"""-m gpu: in-flight decode under classifier-free guidance -- a slot is a PAIR (`mh_t5_slots_open_guided`, `mh_t5_slots_admit_pair`,
`T5Engine.open_guided_slots`, `SequentialWindowScheduler(inflight=True, inflight_guided=True)`; contract in include/mapperhip.h).

The yardstick throughout is the BATCH-1 GUIDED CALL: `T5Engine.decode(row_sampling=...)` with the 2-row batch [negative | prompt] of the
window alone (`guided_rows`), one cross K/V row and one row entry with the pair's own scale, under the same e4m3 modes.  Every
comparison is bit equality: the dumped scores of every live pair after every `run(1)`, the ids at retirement, and under the e4m3
modes the bytes and scales of the slot's rows of both copies.  The models are those of the tiny goldens (tests/golden/t5_tiny.npz,
vw_test.npz, hfw_test.npz: seeded weights); the T5 one gets 160 target positions so that a row can pass the 128-key iteration of the
self-attention's key loop.  The session's workspace, its token rows and both e4m3 copies are filled with 0xFF bytes before every
session opens: nothing a session reads is left over from an earlier one."""
import ctypes as C

import pytest
import torch

from conftest import t5_golden_case, vw_golden_case, wf_golden_case

pytestmark = pytest.mark.gpu

T5_TGT = 160
BF16 = torch.bfloat16
MODES = {None: {}, "cross": dict(cross_kv_fp8=True), "self": dict(self_kv_fp8=True), "both": dict(cross_kv_fp8=True, self_kv_fp8=True)}
_CACHE = {}


# ---- models, windows, the batch-1 guided call -----------------------------------------------------------------------------------------
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
    kw = dict(precision="fp32", do_sample=False, num_beams=1, top_p=1.0, top_k=0, max_length=tgt, cfg_scale=2.0, timeshift_bias=0,
              types_first=False, temperature=1.0, lookback_time=0, lookahead_time=0, context_type="map", pad_token_id=0,
              conditional_temperature_per_row=True)
    kw.update(over)
    return kw


class _Window:
    """One window: its cross K/V row, unpadded prompt (and mask), negative prompt (n <= P ids), kwargs (cfg_scale = the pair's scale),
    and whether its EOS set is the kwargs' own (`eos`: True), empty (False: the pair runs to its cap) or a given id list."""

    def __init__(self, kv_row, prompt, negative, gk, mask=None, eos=False):
        self.kv_row, self.prompt, self.negative, self.gk, self.mask, self.eos = kv_row, prompt, negative, gk, mask, eos
        self.P = int(prompt.shape[0])
        assert 1 <= negative.shape[0] <= self.P


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


def _align256(n):
    return (n + 255) // 256 * 256


def _cross8_views(buf, eng, S):
    """the packed e4m3 cross K/V copy of S rows -> (bytes (planes, S, H, L * 64), scales (planes, S, H))"""
    d, p = eng.dims, eng.packed
    planes, n = 2 * d.n_dec_layers, 2 * d.n_dec_layers * S * d.n_heads * p.src_len * 64
    off = _align256(n)
    return (buf[:n].view(planes, S, d.n_heads, p.src_len * 64),
            buf[off:off + planes * S * d.n_heads * 4].view(torch.float32).view(planes, S, d.n_heads))


def _self8_views(buf, eng, R):
    """the e4m3 shadow of R rows -> (bytes (planes, R, H, tgt, 64), scales (planes, R, H, tgt))"""
    d, p = eng.dims, eng.packed
    planes, rows = 2 * d.n_dec_layers, 2 * d.n_dec_layers * R * d.n_heads * p.tgt_len
    off = _align256(rows * 64)
    return (buf[:rows * 64].view(planes, R, d.n_heads, p.tgt_len, 64),
            buf[off:off + rows * 4].view(torch.float32).view(planes, R, d.n_heads, p.tgt_len))


def _uniform(m, tok, kv, w, tgt, mode=None, copies=False, guided=True):
    """THE reference: the window alone through `T5Engine.decode(row_sampling=)` as the 2-row guided batch [negative | prompt] over one
    cross K/V row, under `mode` -> (ids of the prompt row (n,), guided scores (n, V)[, its copies on the host: cross bytes and scales
    of the one row, shadow bytes and scales of rows (negative, prompt) -- None where the mode has no such copy]).
    guided = False: the same prompt alone, B = 1, without guidance (what the guided scores must differ from)."""
    from mapperatorinator_amd import _lib
    from mapperatorinator_amd.t5_engine import guided_rows
    eng = m.engine
    sw = MODES[mode]
    if not guided:
        w = _Window(w.kv_row, w.prompt, w.negative, dict(w.gk, cfg_scale=1.0), w.mask, w.eos)
    sp, row, table = _row_of(tok, w, tgt)
    assert (sp.cfg_scale > 1.0) == guided and (not guided or abs(row.cfg_scale - w.gk["cfg_scale"]) < 1e-6)
    sp.max_length = tgt                                   # the stride of the session's buffers: the same per-call settings
    rows = (_lib.MhRowSampling * 1)()
    C.memmove(rows, C.byref(row), C.sizeof(row))
    rows[0].eos_set = 0
    prompt, mask = w.prompt[None], None if w.mask is None else w.mask[None]
    if guided:
        prompt, mask, _ = guided_rows(prompt, mask, w.negative[None])
    kv_row = kv[:, :, w.kv_row:w.kv_row + 1].contiguous()
    eng._enter()
    with eng.on_stream():
        kv8 = eng.cross_kv_fp8(kv_row) if sw.get("cross_kv_fp8") else None
        tokens, n_out, logits = eng.decode(kv_row, prompt.to(eng.device, torch.int32).contiguous(),
                                           None if mask is None else mask.to(eng.device).to(torch.uint8).contiguous(), None, sp,
                                           dump_logits=True, kv_fp8=kv8, self_kv_fp8=bool(sw.get("self_kv_fp8")),
                                           row_sampling=(sp, rows, table[None]))
    eng._leave()
    eng.synchronize()
    n = int(n_out.item())
    out = (tokens[-1, :n].to(torch.int64).cpu(), logits[:n, 0].cpu())
    if guided:
        assert torch.equal(tokens[0, w.P:n], tokens[1, w.P:n]), "both rows of a pair receive the same ids"
    if copies:
        c8 = [t[:, 0].cpu() for t in _cross8_views(kv8, eng, 1)] if kv8 is not None else [None, None]
        s8 = [t.cpu() for t in _self8_views(eng._ws["skv8"], eng, 2)] if sw.get("self_kv_fp8") else [None, None]
        out += (c8 + s8,)
    return out


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _poison(eng, S):
    """what the next guided session of S pairs is given, every byte 0xFF: its workspace (the caches, the mask rows and the slot arrays
    are in it), the token rows and both e4m3 copies"""
    p = eng.packed
    eng._workspace("slots", eng.lib.mh_t5_slots_guided_workspace_bytes(C.byref(p.cfg), S)).fill_(0xFF)
    eng._workspace("slot_tokens", 64 * p.tgt_len * 4).fill_(0xFF)
    if eng.dtype == BF16:
        eng._workspace("slot_cross_kv8", eng.lib.mh_t5_cross_kv_fp8_bytes(C.byref(p.cfg), S)).fill_(0xFF)
        eng._workspace("slot_skv8", eng.lib.mh_t5_self_kv_fp8_bytes(C.byref(p.cfg), 2 * S)).fill_(0xFF)
    torch.cuda.synchronize()


def _check_copies(slots, eng, slot, n, ref_copies, what):
    """the slot's rows of the session copies against the batch-1 guided call's: the cross row and its scales; rows slot (negative) and
    S + slot (prompt) of the shadow at positions 0 .. n - 2, the positions a pair of n columns was fed at"""
    torch.cuda.synchronize()
    c_bytes, c_scales, s_bytes, s_scales = ref_copies
    S = slots.S
    if slots.cross_kv8 is not None:
        b, s = _cross8_views(slots.cross_kv8, eng, S)
        assert torch.equal(b[:, slot].cpu(), c_bytes), f"{what}: the e4m3 cross row differs from the guided call's"
        assert _same_bits(s[:, slot].cpu(), c_scales), f"{what}: the cross scales differ from the guided call's"
    if slots.self_kv8 is not None:
        b, s = _self8_views(slots.self_kv8, eng, 2 * S)
        for j, r in enumerate((slot, S + slot)):
            assert torch.equal(b[:, r, :, :n - 1].cpu(), s_bytes[:, j, :, :n - 1]), \
                f"{what}: shadow bytes of row {r} below position {n - 1} differ from the guided call's row {j}"
            assert _same_bits(s[:, r, :, :n - 1].cpu(), s_scales[:, j, :, :n - 1]), f"{what}: shadow scales of row {r} differ from the guided call's"


def _run_pairs(m, tok, kv, windows, S, tgt, refs, mode=None, copies=False):
    """The windows, in order, through S pair slots (lowest idle slot first), one step per run.  After every `run(1)` the newly dumped
    scores of every live pair, at retirement its ids (and with `copies` its rows of both copies) are compared with the window's batch-1
    guided call: equal bits.  -> (per slot its occupants, per run the live pairs as (window, columns so far), stats)"""
    eng = m.engine
    sp = _row_of(tok, windows[0], tgt)[0]
    sp.max_length = tgt
    _poison(eng, S)
    queue = list(range(len(windows)))
    occupant, seen, history, timeline = [None] * S, [0] * S, [[] for _ in range(S)], []
    with eng.open_guided_slots(S, sp, dump_logits=True, **MODES[mode]) as slots:
        assert slots.guided and slots.tokens.shape == (2 * S, tgt) and slots.logits.shape[1] == S
        while True:
            for slot in range(S):
                if occupant[slot] is None and queue:
                    i = queue.pop(0)
                    w = windows[i]
                    _, row, table = _row_of(tok, w, tgt)
                    slots.admit(slot, kv[:, :, w.kv_row], w.prompt, w.mask, row, table, negative_prompt=w.negative)
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
                    assert lengths[slot] == 0 and not finished[slot]
                    continue
                ids, scores = refs[i][0], refs[i][1]
                n = lengths[slot]
                assert 1 <= n <= ids.shape[0], (i, n, ids.shape[0])     # (n < P: option decode_prefill = 0 is still feeding the prompt)
                if n > seen[slot]:
                    eng.synchronize()
                    got = slots.logits[seen[slot]:n, slot].cpu()
                    assert _same_bits(got, scores[seen[slot]:n]), \
                        f"window {i} in slot {slot}: scores of columns {seen[slot]}..{n - 1} differ from its batch-1 guided call"
                    seen[slot] = n
                if finished[slot]:
                    if copies:
                        _check_copies(slots, eng, slot, n, refs[i][2], f"{mode}: window {i} in slot {slot}")
                    neg_row = slots.tokens[slot, :n].to(torch.int64).cpu()
                    row = slots.take(slot)
                    assert torch.equal(row, ids), f"window {i} in slot {slot}: ids differ from its batch-1 guided call\n{row.tolist()}\n{ids.tolist()}"
                    P, nn = windows[i].P, int(windows[i].negative.shape[0])
                    assert torch.equal(neg_row[P:], ids[P:]) and torch.equal(neg_row[:nn], windows[i].negative.to(torch.int64)) \
                        and torch.equal(neg_row[nn:P], ids[nn:P]), f"window {i}: the negative row is the negative prompt, then the pair's ids"
                    occupant[slot] = None
                else:
                    assert n < ids.shape[0], f"window {i} in slot {slot} runs on behind its batch-1 guided call's end"
        stats = dict(slots.stats)
    return history, timeline, stats


# ---- T5 tiny, 2 pair slots, 5 windows ---------------------------------------------------------------------------------------------------
# (prompt length, negative-prompt length, cap, scale).  Prompts of 1 (no prefill), 2, 9 and 40 ids; window 1 runs to column 135, past
# the 128 keys of one iteration of the self-attention's key loop, and is mid-decode while slot 0 is refilled three times; negative
# prompts shorter than the prompt and as long as it; neighbouring pairs under scales 1.5 and 3.0, different caps and EOS sets (window
# 2: the kwargs' own set; window 4: one id, found with a run without EOS set; the others none: they run to their caps).
_T5_WINDOWS = [(1, 1, 14, 1.5), (40, 7, 136, 3.0), (9, 9, 20, 1.5), (2, 1, 12, 3.0), (9, 4, 30, 1.5)]


def _t5_windows(tok, sample):
    over = dict(do_sample=True, top_p=0.9, seed=1234) if sample else {}
    wins = []
    for i, (P, nn, cap, scale) in enumerate(_T5_WINDOWS):
        gk = _gk(T5_TGT, max_length=cap, cfg_scale=scale, temperature=1.0 + 0.05 * (i % 3), **over)
        if sample:
            gk["seed_call_index"] = i                      # per-row seeds
        negative = _prompt(tok, nn, seed=70 + i)
        wins.append(_Window(i % 4, _prompt(tok, P, seed=20 + i), negative, gk, eos=(i == 2)))
    return wins


def _t5_case(dtype, prefill=True, sample=False, mode=None):
    m, tok, n_samples = _t5_model(dtype, prefill)
    kv = _cross_kv(m, n_samples, 4)
    key = ("t5case", dtype, prefill, sample, mode)
    if key not in _CACHE:
        wins = _t5_windows(tok, sample)
        probe = _Window(wins[4].kv_row, wins[4].prompt, wins[4].negative, wins[4].gk, eos=False)
        ids, _ = _uniform(m, tok, kv, probe, T5_TGT, mode)
        wins[4].eos = [int(ids[wins[4].P + 3])]
        _CACHE[key] = (wins, [_uniform(m, tok, kv, w, T5_TGT, mode, copies=mode is not None) for w in wins])
    return (m, tok, kv) + _CACHE[key]


def _check_t5_timeline(wins, refs, history, timeline):
    assert refs[1][0].shape[0] == 136, "window 1 must run to column 135"
    assert refs[4][0].shape[0] <= wins[4].P + 4, "window 4 must end by its EOS id"
    assert history[1] == [1] and len(history[0]) == 4, f"slot 0 must be reused beside window 1: {history}"
    # columns so far n -> the position fed next is n - 1: window 1 past position 128, and a pair admitted while it is mid-decode
    assert any(i == 1 and n - 1 > 128 for live in timeline for i, n in live)
    assert any(any(i == 1 and 45 < n < 120 for i, n in live) and any(i != 1 and n <= wins[i].P + 1 for i, n in live) for live in timeline), \
        "no pair admitted while its neighbour is mid-decode"


@pytest.mark.parametrize("dtype", [torch.float32, BF16], ids=["fp32", "bf16"])
def test_t5_pairs_match_the_guided_call_step_by_step(dtype):
    m, tok, kv, wins, refs = _t5_case(dtype)
    # the yardstick depends on guidance: the guided scores are not the unguided scores of the same prompt
    plain = _uniform(m, tok, kv, wins[2], T5_TGT, guided=False)
    n = min(plain[1].shape[0], refs[2][1].shape[0])
    assert n > wins[2].P and not _same_bits(plain[1][wins[2].P:n], refs[2][1][wins[2].P:n]), "guidance must change the scores"
    # ... and on the pair's own scale
    other = _uniform(m, tok, kv, _Window(wins[2].kv_row, wins[2].prompt, wins[2].negative, dict(wins[2].gk, cfg_scale=3.0)), T5_TGT)
    assert not _same_bits(other[1][wins[2].P:wins[2].P + 1], refs[2][1][wins[2].P:wins[2].P + 1]), "the scale must change the scores"
    history, timeline, stats = _run_pairs(m, tok, kv, wins, 2, T5_TGT, refs)
    _check_t5_timeline(wins, refs, history, timeline)
    assert stats["admissions"] == 5 and stats["steps"] == len(timeline)      # one chain: one replay per run


def test_t5_sampled_pairs_draw_what_the_guided_call_draws():
    """do_sample, top_p = 0.9, a seed per pair: the draw is keyed by (seed, RNG row, the pair's OWN column)."""
    m, tok, kv, wins, refs = _t5_case(torch.float32, sample=True)
    greedy = _t5_case(torch.float32)[4]
    assert any(not torch.equal(a[0], b[0]) for a, b in zip(refs, greedy)), "the sampled case must differ from the greedy one"
    history, timeline, _ = _run_pairs(m, tok, kv, wins, 2, T5_TGT, refs)
    _check_t5_timeline(wins, refs, history, timeline)


def test_t5_pairs_under_decode_prefill_0_feed_both_prompt_rows_token_by_token():
    """option decode_prefill = 0: nothing is prefilled; the sampler's "still inside the prompt" branch feeds each row of the pair its own
    prompt column (the negative row's differ) and advances both positions."""
    m, tok, kv, wins, refs = _t5_case(torch.float32, prefill=False)
    history, timeline, _ = _run_pairs(m, tok, kv, wins, 2, T5_TGT, refs)
    assert any(n < wins[i].P for live in timeline for i, n in live if wins[i].P > 2), "no step inside a prompt"
    assert refs[1][0].shape[0] == 136


@pytest.mark.parametrize("mode", ["cross", "self", "both"])
def test_e4m3_modes_ids_scores_and_both_copies_match_the_guided_call(mode):
    m, tok, kv, wins, refs = _t5_case(BF16, mode=mode)
    if mode != "self":
        plain = _t5_case(BF16)[4]
        assert not _same_bits(plain[2][1][wins[2].P:wins[2].P + 1], refs[2][1][wins[2].P:wins[2].P + 1]), "the e4m3 cross K/V must change the scores"
    history, timeline, _ = _run_pairs(m, tok, kv, wins, 2, T5_TGT, refs, mode=mode, copies=True)
    _check_t5_timeline(wins, refs, history, timeline)


# ---- the Whisper families -----------------------------------------------------------------------------------------------------------
def test_vw_pairs_rotary_with_local_layers():
    """rotary Whisper with local layers (8 keys behind the query): a pair decoded to column 39 beside freshly admitted pairs still inside
    the window; both rows of a pair rotate by the pair's own position."""
    m, tok, n_samples = _vw_model()
    tgt = m.engine.packed.tgt_len
    kv = _cross_kv(m, n_samples, 3)
    P = _prompt
    wins = [_Window(0, P(tok, 3, 1), P(tok, 2, 11), _gk(tgt, max_length=40, cfg_scale=1.5)),
            _Window(1, P(tok, 1, 2), P(tok, 1, 12), _gk(tgt, max_length=9, cfg_scale=3.0)),
            _Window(2, P(tok, 2, 3), P(tok, 2, 13), _gk(tgt, max_length=12, cfg_scale=1.5)),
            _Window(1, P(tok, 12, 4), P(tok, 5, 14), _gk(tgt, max_length=20, cfg_scale=3.0)),
            _Window(0, P(tok, 9, 5), P(tok, 9, 15), _gk(tgt, max_length=14, cfg_scale=1.5))]
    refs = [_uniform(m, tok, kv, w, tgt) for w in wins]
    history, timeline, _ = _run_pairs(m, tok, kv, wins, 2, tgt, refs)
    assert refs[0][0].shape[0] == 40 and len(history[1]) == 4
    assert any(any(i == 0 and n - 1 > 8 for i, n in live) and any(i != 0 and n - 1 < 8 for i, n in live) for live in timeline)


def test_hfw_pairs_with_a_masked_first_column():
    """HF Whisper: learned positions come from the mask (a masked first column shifts them by one) -- pos_off on BOTH rows of the pair,
    from the one mask they share."""
    m, tok, n_samples = _hfw_model()
    assert m.engine.packed.cfg.dec_pos_from_mask == 1
    tgt = m.engine.packed.tgt_len
    kv = _cross_kv(m, n_samples, 3)
    one = torch.tensor
    wins = [_Window(0, one([0, 1, 9]), one([0, 1]), _gk(tgt, max_length=30, cfg_scale=1.5), mask=one([0, 1, 1])),
            _Window(1, one([1, 40, 700]), one([1, 41, 600]), _gk(tgt, max_length=12, cfg_scale=3.0)),
            _Window(2, one([0, 0, 1]), one([0, 0, 1]), _gk(tgt, max_length=16, cfg_scale=1.5), mask=one([0, 0, 1])),
            _Window(0, one([1, 9]), one([1]), _gk(tgt, max_length=20, cfg_scale=3.0)),
            _Window(1, one([0, 1, 9, 50, 51, 52, 53, 54, 55]), one([0, 1, 8, 60]), _gk(tgt, max_length=18, cfg_scale=1.5),
                    mask=one([0, 1, 1, 1, 1, 1, 1, 1, 1]))]
    refs = [_uniform(m, tok, kv, w, tgt) for w in wins]
    unmasked = _uniform(m, tok, kv, _Window(0, one([0, 1, 9]), one([0, 1]), wins[0].gk), tgt)
    assert not _same_bits(unmasked[1][3:4], refs[0][1][3:4]), "the mask must move the positions"
    _run_pairs(m, tok, kv, wins, 2, tgt, refs)


# ---- state isolation ------------------------------------------------------------------------------------------------------------------
def test_admission_steps_and_release_leave_the_other_pairs_rows_alone():
    m, tok, kv, wins, refs = _t5_case(BF16, mode="both")
    eng = m.engine
    sp = _row_of(tok, wins[0], T5_TGT)[0]
    sp.max_length = T5_TGT
    S = 3
    _poison(eng, S)
    with eng.open_guided_slots(S, sp, **MODES["both"]) as slots:
        c8 = _cross8_views(slots.cross_kv8, eng, S)
        s8 = _self8_views(slots.self_kv8, eng, 2 * S)

        def state(slot):    # everything of the caller's buffers that belongs to the pair in `slot`, as bytes
            torch.cuda.synchronize()
            return [t.contiguous().view(torch.uint8).cpu().clone() for t in
                    (slots.tokens[slot], slots.tokens[S + slot], c8[0][:, slot], c8[1][:, slot], s8[0][:, slot], s8[0][:, S + slot],
                     s8[1][:, slot], s8[1][:, S + slot])]

        def admit(slot, i):
            _, row, table = _row_of(tok, wins[i], T5_TGT)
            slots.admit(slot, kv[:, :, wins[i].kv_row], wins[i].prompt, None, row, table, negative_prompt=wins[i].negative)
        admit(0, 0)
        admit(2, 2)
        for _ in range(6):
            finished, lengths = slots.run(1)
        assert lengths[1] == 0 and lengths[0] > 0 and lengths[2] > 0
        # slot 1 was idle through six steps: every byte of both its rows is still the 0xFF the session found
        assert all(bool((t == 0xFF).all()) for t in state(1)), "a step or a neighbour's admission wrote into an idle pair's rows"
        before = {s: state(s) for s in (0, 2)}
        admit(1, 3)                                        # a prompt of 2 ids: the prefill and the shadow's prompt rows of both rows
        for s in (0, 2):
            assert all(torch.equal(a, b) for a, b in zip(state(s), before[s])), f"the admission into slot 1 changed slot {s}'s rows"
        # ... and of its own shadow rows it wrote the prompt's positions 0 .. P - 2, of both rows, and nothing else
        P = wins[3].P
        for r in (1, S + 1):
            assert not bool((s8[1][:, r, :, :P - 1].contiguous().view(torch.uint8) == 0xFF).all())
            assert bool((s8[0][:, r, :, P - 1:] == 0xFF).all()) and bool((s8[1][:, r, :, P - 1:].contiguous().view(torch.uint8) == 0xFF).all())
        # a released pair's rows are idle: both positions negative again, so no later step writes either row
        while not finished[0]:
            finished, lengths = slots.run(1)
        assert torch.equal(slots.take(0), refs[0][0])
        released = state(0)
        for _ in range(4):
            finished, lengths = slots.run(1)
            assert lengths[0] == 0 and not finished[0]
        assert all(torch.equal(a, b) for a, b in zip(state(0), released)), "a step wrote into a released pair's rows"


# ---- kind mismatch ----------------------------------------------------------------------------------------------------------------------
def test_the_wrong_admission_is_refused_and_the_session_stays_usable():
    m, tok, kv, wins, refs = _t5_case(torch.float32)
    eng, lib = m.engine, m.engine.lib
    sp = _row_of(tok, wins[0], T5_TGT)[0]
    sp.max_length = T5_TGT
    w = wins[3]
    prompt_d = w.prompt.to("cuda", torch.int32)
    kv_row = kv[:, :, w.kv_row:w.kv_row + 1].contiguous()
    _, row, table = _row_of(tok, w, T5_TGT)
    torch.cuda.synchronize()
    _poison(eng, 2)
    with eng.open_guided_slots(2, sp) as slots:
        assert lib.mh_t5_slots_admit(slots._handle, 0, kv_row.data_ptr(), prompt_d.data_ptr(), None, w.P, None) == -1
        msg = lib.mh_last_error()
        assert msg.startswith(b"mh_t5_slots_admit: ") and b"guided" in msg and b"mh_t5_slots_admit_pair" in msg, msg
        with pytest.raises(ValueError, match="negative_prompt is required"):
            slots.admit(0, kv[:, :, w.kv_row], w.prompt, None, row, table)
        slots.admit(0, kv[:, :, w.kv_row], w.prompt, None, row, table, negative_prompt=w.negative)
        finished, lengths = slots.run(T5_TGT)
        assert finished == [True, False] and lengths == [refs[3][0].shape[0], 0]
        assert torch.equal(slots.take(0), refs[3][0])
    # a plain session refuses the pair admission, and guidance as ever
    from mapperatorinator_amd.server import build_row_sampling
    plain = _Window(w.kv_row, w.prompt, w.negative, dict(w.gk, cfg_scale=1.0))
    sp1, row1, table1 = _row_of(tok, plain, T5_TGT)
    sp1.max_length = T5_TGT
    pair_d = torch.stack([w.prompt, w.prompt]).to("cuda", torch.int32)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="classifier-free guidance has no slot form"):
        eng.open_slots(2, build_row_sampling(tok, [w.gk], T5_TGT)[0])
    with eng.open_slots(2, sp1) as slots:
        assert lib.mh_t5_slots_admit_pair(slots._handle, 0, kv_row.data_ptr(), pair_d.data_ptr(), None, w.P, None) == -1
        msg = lib.mh_last_error()
        assert msg.startswith(b"mh_t5_slots_admit_pair: ") and b"not guided" in msg, msg
        with pytest.raises(ValueError, match="negative_prompt on a session without guidance"):
            slots.admit(0, kv[:, :, w.kv_row], w.prompt, None, row1, table1, negative_prompt=w.negative)
        slots.admit(0, kv[:, :, w.kv_row], w.prompt, None, row1, table1)
        finished, lengths = slots.run(T5_TGT)
        assert finished == [True, False] and lengths[0] == w.gk["max_length"]
        slots.take(0)


# ---- the scheduler -----------------------------------------------------------------------------------------------------------------------
def test_guided_inflight_scheduler_matches_the_default_policy():
    """Two guided songs of 2 and 3 dependent windows, every window under a scale of its own, through `SequentialWindowScheduler(inflight=
    True, inflight_guided=True)` with decode_batch = 4 (2 pair slots) == the same jobs through the default policy with decode_batch = 2
    (one guided window per call: no left padding).  Greedy; each prompt is built from the previous window's output."""
    from mapperatorinator_amd.scheduler import SequentialWindowScheduler, SongJob
    from mh_testing import synthetic_audio
    m, tok, n_samples = _t5_model(torch.float32)
    n_windows = [2, 3]
    songs = [synthetic_audio(n, n_samples, seed=40 + k) for k, n in enumerate(n_windows)]

    def kwargs_for(k, w, n):
        kw = _gk(48, lookback_time=400 if w != 0 else 0, lookahead_time=3000 if w != n - 1 else 0, temperature=0.9,
                 cfg_scale=(1.5, 3.0, 2.0)[(k + w) % 3])
        kw.pop("conditional_temperature_per_row")
        return kw

    def prompt_from(prev):
        if prev is None:
            return torch.tensor([[tok.sos_id]])
        return torch.tensor([[tok.sos_id] + [t for t in prev.tolist() if t > 2][-3:]])

    def run(**policy):
        got, state, order = [[None] * n for n in n_windows], [None] * 2, []

        def make_job(k, n):
            def prompt_fn(w):
                prompt = prompt_from(state[k])
                negative = torch.tensor([[tok.sos_id, 500 + k][:prompt.shape[1]]])
                return dict(decoder_input_ids=prompt, negative_prompt=negative, generate_kwargs=kwargs_for(k, w, n))

            def on_result(w, row, st):
                p = prompt_from(state[k]).shape[1]
                got[k][w] = row
                state[k] = row[p:]
                order.append((k, w))
            return SongJob(frames=songs[k], prompt_fn=prompt_fn, on_result=on_result, generate_kwargs=dict(cfg_scale=2.0))
        stats = SequentialWindowScheduler(m, tok, encode_batch=4, **policy).run([make_job(k, n) for k, n in enumerate(n_windows)])
        return got, order, stats

    want, _, _ = run(decode_batch=2)
    got, order, stats = run(decode_batch=4, inflight=True, inflight_guided=True, inflight_steps=4)
    assert stats["windows"] == stats["admissions"] == 5 and stats["decode_steps"] > 0
    for k, n in enumerate(n_windows):
        assert [w for kk, w in order if kk == k] == list(range(n)), order
        for w in range(n):
            a, b = got[k][w], want[k][w]
            assert a.shape == b.shape and torch.equal(a, b), (k, w, a.tolist(), b.tolist())
    assert any(len(r) > 4 for rows in want for r in rows), "the windows must produce ids"
