"""Window scheduler for sequential songs on top of the HIP engine.

The reference generates a song window by window (`Processor.generate_sequential`, osuT5/osuT5/inference/
processor.py:308-368): window i's prompt contains the events that window i-1 produced, so the windows of ONE song are
a chain; each iteration runs mel -> encoder -> decode for a single window (batch 1) and hops through the host between
the stages.  Two things in that loop do not depend on the chain and are taken out of it here:

  * the mel + encoder + cross-K/V of EVERY window depends on the audio only: all windows of all songs are encoded up
    front in MFMA-sized batches and their cross-attention K/V stays resident in HBM (46 MB per 10 s window at
    osuT5-base; a 3-minute song is 0.8 GB -- hundreds of songs fit in 288 GB);
  * different songs are independent: wave w decodes window w of every song that still has one as ONE batch
    (rows grouped by identical generate kwargs -- the lookback / lookahead EOS windows differ on a song's first and
    last window).

Prompt building stays with the caller -- it is the reference's own integer host logic (`get_prompts`,
`prepare_context_sequences`, `add_predicted_tokens_to_context`, processor.py:1022-1052,1226-1268): a `SongJob` supplies
`prompt_fn(window) -> model_kwargs-like dict` and receives every finished window through `on_result`.  Rows are
batch-invariant in the engine, so the tokens are exactly those of the reference-shaped loop (one `model_generate` per
window), which is what tests/test_gpu_t5.py::test_window_scheduler_matches_sequential_loop checks.
"""
from __future__ import annotations

import dataclasses
import time
from typing import Callable, Optional

import torch

from .decode_modes import DecodeModes
from .server import _build_generation_stats, build_row_sampling, build_sampling, row_call_key
from .t5_engine import HostStager, eos_id_table, guided_rows


@dataclasses.dataclass
class SongJob:
    """frames: (n_windows, samples) raw audio windows of one song (what `prepare_frames` yields per window).
    prompt_fn(window_index) -> dict(decoder_input_ids=(1, P) int64, [decoder_attention_mask], [negative_prompt],
        [generate_kwargs=dict]) -- called when the previous window of THIS song has been delivered.
    on_result(window_index, tokens (P + new,) int64 cpu incl. the prompt, stats dict)."""
    frames: torch.Tensor
    prompt_fn: Callable[[int], dict]
    on_result: Callable[[int, torch.Tensor, dict], None]
    generate_kwargs: dict = dataclasses.field(default_factory=dict)
    # models with conditioning embedders: window index -> dict(difficulty=, mapper_idx=, song_position=, beatmap_idx=) of
    # scalars / (2,) for THIS window (the reference sets song_position per window, processor.py:341-345)
    conditioning_fn: Optional[Callable[[int], dict]] = None


def _left_pad(rows, pad_id: int, dtype):
    width = max(r.shape[-1] for r in rows)
    out = torch.full((len(rows), width), pad_id, dtype=dtype)
    for i, r in enumerate(rows):
        out[i, width - r.shape[-1]:] = r.reshape(-1).to(dtype)
    return out


class SequentialWindowScheduler:
    def __init__(self, model, tokenizer, *, encode_batch: int = 32, decode_batch: int = 32, merge_kwargs: bool = False,
                 inflight: bool = False, inflight_steps: int = 16, inflight_kv_fp8: Optional[str] = None,
                 inflight_guided: bool = False):
        if decode_batch > 64 or decode_batch < 1:
            raise ValueError("decode_batch must be in [1, 64] (32 at most when windows run under classifier-free guidance)")
        if inflight_kv_fp8 not in self._INFLIGHT_KV_FP8:
            raise ValueError(f"inflight_kv_fp8={inflight_kv_fp8!r}: expected None, 'cross', 'self' or 'both'")
        if inflight_kv_fp8 is not None and not inflight:
            raise ValueError(f"inflight_kv_fp8={inflight_kv_fp8!r} is a switch of the slot session: it needs inflight=True (a wave takes "
                             "cross_kv_fp8 / self_kv_fp8 from its generate_kwargs)")
        if inflight_guided and not inflight:
            raise ValueError("inflight_guided=True is a switch of the slot session: it needs inflight=True (a wave takes guidance from "
                             "its generate_kwargs)")
        self.model, self.tokenizer = model, tokenizer
        self.engine = model.engine
        self.encode_batch, self.decode_batch = int(encode_batch), int(decode_batch)
        self.stats = dict(windows=0, decode_calls=0, encode_calls=0, generated_tokens=0, elapsed_seconds=0.0)
        self._seed_calls: dict = {}       # explicit seed -> decode calls made with it BY THIS scheduler
        # merge_kwargs (off by default: the reference's grouping): the kwargs groups of a wave that agree in the per-call settings
        # (server.row_call_key) decode as ONE call, every row under its own settings (T5Engine.decode(row_sampling=)); a wave
        # whose first / last windows carry other EOS windows than the rest is then one decode call, not two or three
        self.merge_kwargs = bool(merge_kwargs)
        # inflight (off by default): no waves -- decode_batch SLOTS are kept full (T5Engine.open_slots): a song's window w + 1 is
        # admitted as soon as its window w was delivered, into whatever slot is idle, while the other slots keep stepping;
        # `inflight_steps` token steps run between two looks at the slots.  See `_run_inflight`.
        self.inflight, self.inflight_steps = bool(inflight), max(1, int(inflight_steps))
        # inflight_kv_fp8 (off by default): the e4m3 caches of the slot SESSION (T5Engine.open_slots(cross_kv_fp8=, self_kv_fp8=)): the
        # copies are allocated once for all slots and captured in the chains' step graphs, so they are chosen here, where the session
        # is chosen, and not by a job or a window.  fp32 storage is refused now, before anything is encoded.
        self.inflight_kv_fp8 = dict(zip(("cross_kv_fp8", "self_kv_fp8"), self._INFLIGHT_KV_FP8[inflight_kv_fp8]))
        DecodeModes.of(self.inflight_kv_fp8, getattr(self.engine, "dtype", None))
        # inflight_guided (off by default): the session's slots are classifier-free guidance PAIRS (T5Engine.open_guided_slots):
        # decode_batch // 2 slots, as a guided wave holds half the windows; every job and every window must then be guided (cfg_scale
        # > 1 and a negative_prompt), each window under its own scale.  Off: guidance is refused under inflight as ever.
        self.inflight_guided = bool(inflight_guided)

    # ---- stage 1: everything that depends on the audio only ------------------------------------------------
    @torch.no_grad()
    def encode_all(self, jobs: list[SongJob]):
        """-> per job a tensor [n_dec_layers, 2, n_windows, H, L, 64] of resident cross-attention K/V."""
        eng = self.engine
        flat = torch.cat([j.frames for j in jobs], 0)
        row_bias = self._row_bias(jobs)
        parts = []
        on_gpu = torch.device(eng.device).type == "cuda"     # (CPU stand-in engines of the host tests take the plain path)
        stager = HostStager(eng.device) if on_gpu else None
        eb = self.encode_batch

        def stage(a):
            part = flat[a:a + eb]
            return stager.stage(part, torch.float32) if on_gpu else (part.to(eng.device, torch.float32), None)
        nxt = stage(0)                                        # batch a + 1 crosses PCIe while batch a is encoded
        eng._enter()
        with eng.on_stream():
            for a in range(0, flat.shape[0], eb):
                cur, ev = nxt
                if a + eb < flat.shape[0]:
                    nxt = stage(a + eb)
                if ev is not None:
                    eng.stream.wait_event(ev)
                rb = None if row_bias is None else row_bias[a:a + eb]
                parts.append(eng.cross_kv(eng.encode_mel(eng.mel(cur), row_bias=rb)))
                if on_gpu:
                    cur.record_stream(eng.stream)
                self.stats["encode_calls"] += 1
            kv = torch.cat(parts, 2) if len(parts) > 1 else parts[0]
        eng._leave()
        out, a = [], 0
        for j in jobs:
            out.append(kv[:, :, a:a + j.frames.shape[0]])
            a += j.frames.shape[0]
        return out

    def _row_bias(self, jobs):
        """(total windows, d_model) fp32 for models with conditioning embedders (one row per window, in `frames` order),
        None otherwise."""
        cond = getattr(self.model, "cond", None)
        if cond is None or not cond.active:
            return None
        keys = cond.INPUTS
        rows = {k: [] for k in keys}
        for j in jobs:
            if j.conditioning_fn is None:
                raise ValueError("this model has conditioning embedders: every SongJob needs a conditioning_fn")
            for w in range(j.frames.shape[0]):
                kw = j.conditioning_fn(w)
                for k in keys:
                    rows[k].append(kw.get(k))
        n = len(rows["difficulty"])
        kw = {}
        for k in keys:
            if all(v is None for v in rows[k]):
                continue
            if any(v is None for v in rows[k]):
                raise ValueError(f"conditioning input {k!r} is given for some windows only")
            kw[k] = torch.stack([torch.as_tensor(v, dtype=torch.float32 if k in ("difficulty", "song_position") else torch.long)
                                 for v in rows[k]])
        return cond.encoder_bias(cond.vectors(n, **kw), self.model.dtype)

    # ---- stage 2: waves of dependent windows -----------------------------------------------------------------
    @torch.no_grad()
    def run(self, jobs: list[SongJob]):
        eng, tok = self.engine, self.tokenizer
        for j in jobs:   # a mode where it is not built: refused before anything is encoded
            self._modes(j.generate_kwargs, int(j.generate_kwargs.get("num_beams", 1) or 1))
        if self.inflight:
            return self._run_inflight(jobs)
        start = time.perf_counter()
        kvs = self.encode_all(jobs)
        n_waves = max(j.frames.shape[0] for j in jobs)
        pad_id = int(getattr(tok, "pad_id", 0))
        for w in range(n_waves):
            active = [i for i, j in enumerate(jobs) if w < j.frames.shape[0]]
            asks = {}
            for i in active:
                ask = dict(jobs[i].prompt_fn(w))
                gk = dict(jobs[i].generate_kwargs, **ask.pop("generate_kwargs", {}))
                key = repr(sorted(gk.items(), key=lambda kv_: kv_[0]))
                asks.setdefault(key, []).append((i, ask, gk))
            if self.merge_kwargs:
                self._run_wave_merged(jobs, kvs, w, asks, pad_id)
                continue
            for group in asks.values():
                # guidance doubles the decode batch (negative rows + prompt rows): half as many windows per call
                step = max(1, self.decode_batch // 2) if float(group[0][2].get("cfg_scale", 1.0)) > 1.0 else self.decode_batch
                # beam search decodes (window, beam) rows: num_beams rows per window (processor.py:159; the timing pass uses 2)
                step = max(1, step // max(1, int(group[0][2].get("num_beams", 1) or 1)))
                for a in range(0, len(group), step):
                    self._decode_group(jobs, kvs, w, group[a:a + step], pad_id)
        self.stats["elapsed_seconds"] += time.perf_counter() - start
        return self.stats

    def _run_wave_merged(self, jobs, kvs, w, asks, pad_id):
        """merge_kwargs: the groups of one wave, cut into the calls the default policy would make (so every window keeps the seed
        and the RNG row of its own group's call), then joined per `row_call_key` into calls of up to decode_batch rows.  Groups
        with beams have no row form and decode as they do by default; so does a group whose `max_length` cannot hold the widest
        prompt of the call it would join (a cap counts COLUMNS, the left padding included: the group would fail a call it passes
        among its own prompts)."""
        keys = {k: row_call_key(dict(group[0][2], conditional_temperature_per_row=True)) for k, group in asks.items()}
        width = {}                            # per call key: the widest prompt among the groups that could share a call
        for k, group in asks.items():
            width[keys[k]] = max([width.get(keys[k], 0)] + [ask["decoder_input_ids"].shape[-1] for _, ask, _ in group])
        merged = {}
        for k, group in asks.items():
            gk0 = group[0][2]
            guided = float(gk0.get("cfg_scale", 1.0)) > 1.0
            step = max(1, self.decode_batch // 2) if guided else self.decode_batch
            step = max(1, step // max(1, int(gk0.get("num_beams", 1) or 1)))
            alone = keys[k] is None or (gk0.get("max_length") is not None and int(gk0["max_length"]) <= width[keys[k]])
            for a in range(0, len(group), step):
                if alone:
                    self._decode_group(jobs, kvs, w, group[a:a + step], pad_id)
                    continue
                gk = self._call_kwargs(gk0)   # (one seed call index per call the default policy makes, in its order)
                merged.setdefault(keys[k], []).extend((i, ask, gk, gk0) for i, ask, _ in group[a:a + step])
        for rows in merged.values():
            step = max(1, self.decode_batch // 2) if float(rows[0][2].get("cfg_scale", 1.0)) > 1.0 else self.decode_batch
            for a in range(0, len(rows), step):
                self._decode_group(jobs, kvs, w, rows[a:a + step], pad_id, merged=True)

    # ---- stage 2, in flight: slots instead of waves ----------------------------------------------------------------------------
    _INFLIGHT_KV_FP8 = {None: (False, False), "cross": (True, False), "self": (False, True), "both": (True, True)}
    _INFLIGHT_REFUSED = (("num_beams", lambda gk: int(gk.get("num_beams", 1) or 1) > 1, "beam search"),
                         ("cfg_scale", lambda gk: float(gk.get("cfg_scale", 1.0)) > 1.0, "classifier-free guidance"),
                         ("cross_kv_fp8", lambda gk: bool(gk.get("cross_kv_fp8", False)), "the e4m3 copy of the cross K/V"),
                         ("self_kv_fp8", lambda gk: bool(gk.get("self_kv_fp8", False)), "the e4m3 self-attention cache"),
                         ("beam_sample_fn", lambda gk: gk.get("beam_sample_fn") is not None, "an injected sampler"),
                         ("sample_fn", lambda gk: gk.get("sample_fn") is not None, "an injected sampler"))

    def _check_inflight(self, gk: dict, what: str) -> None:
        for name, on, words in self._INFLIGHT_REFUSED:
            if name == "cfg_scale" and self.inflight_guided:
                if not on(gk):
                    raise ValueError(f"inflight_guided: {what} is not guided (cfg_scale={gk.get('cfg_scale', 1.0)!r}): every slot of the "
                                     "session is a guidance pair, so every job and window needs cfg_scale > 1 and a negative_prompt; "
                                     "run unguided jobs with inflight_guided=False")
                continue
            if on(gk):
                raise ValueError(f"inflight: {what} asks for {words} ({name}={gk.get(name)!r}), which has no slot form: "
                                 "run it with inflight=False"
                                 + (" (the e4m3 caches of a slot session are the scheduler's switch: inflight_kv_fp8)" if name.endswith("_kv_fp8") else ""))

    def _inflight_row(self, probe: list, gk: dict, sp0=None):
        """One window's kwargs -> (per-call settings, its row entry, its EOS table), built TOGETHER with the session's probe list so
        that the conditional rules keep the session's indices; with `sp0` (the session's settings) the window must not need a
        per-call setting the session was not opened with."""
        sp, rows, tables = build_row_sampling(self.tokenizer, probe + [gk], self.model.config.max_target_positions)
        if sp0 is not None:
            same = (sp.n_cond == sp0.n_cond and list(sp.cond_offset) == list(sp0.cond_offset) and sp.do_sample == sp0.do_sample
                    and sp.lookback_types_first == sp0.lookback_types_first and sp.pad_id == sp0.pad_id
                    and (sp.host_tok_flags is None) == (sp0.host_tok_flags is None)
                    and (sp.host_tok_flags is None or bool((sp.host_tok_flags == sp0.host_tok_flags).all())))
            if not same:
                raise ValueError("inflight: a window's generate_kwargs need per-call settings (conditional rules, types_first lookback, "
                                 "do_sample, pad id) that the jobs' own generate_kwargs and first windows did not announce")
        return sp, rows[len(probe)], tables[rows[len(probe)].eos_set]

    @torch.no_grad()
    def _run_inflight(self, jobs: list[SongJob]):
        """`inflight=True`: decode_batch slots kept full.  Window w + 1 of a song is admitted as soon as its window w was delivered
        through `on_result` (per song strictly in order; across songs in no order), into the lowest idle slot, songs first come first
        served; every row decodes under its own kwargs (`build_row_sampling`), as the default policy's batch-1 call for that window
        would: explicit seeds with this scheduler's own call counter, RNG row 0, no left padding (so no redo path).  The per-call
        settings (`row_call_key`) must agree over all jobs; beams, guidance, the fp8 caches as a job's or a window's kwargs (they
        are the session's: `inflight_kv_fp8`) and injected samplers are refused -- both before anything is encoded.
        `inflight_guided=True`: decode_batch // 2 slots, every one a guidance pair (negative-prompt row and prompt row of one window,
        `T5Engine.open_guided_slots`); every job and window must be guided (cfg_scale > 1, a negative_prompt), each window under
        its own scale; a window decodes as the default policy's guided batch-1 call for it would."""
        eng, tok = self.engine, self.tokenizer
        keys = set()
        for n, j in enumerate(jobs):
            self._check_inflight(j.generate_kwargs, f"job {n}")
            keys.add(row_call_key(dict(j.generate_kwargs, conditional_temperature_per_row=True)))
        if len(keys) > 1:
            raise ValueError("inflight: the jobs differ in a per-call setting (server.row_call_key: do_sample, types_first, pad_token_id, "
                             "precision, ...): such jobs need schedulers of their own")
        start = time.perf_counter()

        def ask_of(i, w):
            ask = dict(jobs[i].prompt_fn(w))
            gk = dict(jobs[i].generate_kwargs, **ask.pop("generate_kwargs", {}))
            self._check_inflight(gk, f"window {w} of job {i}")
            if self.inflight_guided and ask.get("negative_prompt") is None:
                raise ValueError(f"inflight_guided: window {w} of job {i} has no negative_prompt (cfg_scale > 1 needs one for every window)")
            return ask, gk
        # (inflight_guided: every song's first window is asked for, and refused without a negative prompt, before anything is encoded)
        first = {i: ask_of(i, 0) for i in range(len(jobs))} if self.inflight_guided else None
        kvs = self.encode_all(jobs)
        pad_id = int(getattr(tok, "pad_id", 0))
        # guidance doubles the decode rows (a slot is a pair): half as many slots, as a guided wave holds half the windows
        S = max(1, self.decode_batch // 2) if self.inflight_guided else self.decode_batch
        self.stats.setdefault("admissions", 0)
        self.stats.setdefault("decode_steps", 0)
        # the session's per-call settings: those of every song's first window (window 0 depends on nothing), and -- types_first --
        # of the same windows with a lookback, which the later windows of a song carry
        if first is None:
            first = {i: ask_of(i, 0) for i in range(len(jobs))}
        probe = []
        for _, gk in first.values():
            # (seed_call_index -1: no window's own kwargs equal a probe entry's, so a window is always a group of its own -- RNG row
            # 0 -- and the probe advances no seed count)
            base = dict(gk, conditional_temperature_per_row=True, seed_call_index=-1)
            base.pop("max_length", None)      # (a cap is the row's own: songs that differ in it alone are one probe entry, so
            for entry in ([base] +            #  an admission builds a handful of rows, not one per song)
                          ([dict(base, lookback_time=max(float(gk.get("lookback_time", 0) or 0), 1000.0))] if gk.get("types_first", False) else [])):
                if entry not in probe:
                    probe.append(entry)
        sp0 = build_row_sampling(tok, probe, self.model.config.max_target_positions)[0]
        sp0.max_length = int(self.model.config.max_target_positions)
        # (a switch at its default is not passed: engines written against the narrower signature keep working)
        slots = (eng.open_guided_slots if self.inflight_guided else eng.open_slots)(S, sp0, **{k: True for k, on in self.inflight_kv_fp8.items() if on})
        occupant = [None] * S                       # slot -> (job, window, ask, admitted at)
        ready = list(range(len(jobs)))              # songs whose next window may enter, first come first served
        next_w = [0] * len(jobs)
        try:
            while True:
                for slot in range(S):
                    if occupant[slot] is not None or not ready:
                        continue
                    i = ready.pop(0)
                    w = next_w[i]
                    ask, gk = first.pop(i) if w == 0 else ask_of(i, w)
                    _, row, eos_table = self._inflight_row(probe, self._call_kwargs(gk), sp0)
                    ids = ask["decoder_input_ids"].reshape(-1)
                    mask = ask.get("decoder_attention_mask")
                    slots.admit(slot, kvs[i][:, :, w], ids, None if mask is None else mask.reshape(-1), row, eos_table,
                                **({"negative_prompt": ask["negative_prompt"].reshape(-1)} if self.inflight_guided else {}))
                    occupant[slot] = (i, w, ask, time.perf_counter())
                    self.stats["admissions"] += 1
                if all(o is None for o in occupant):
                    break
                steps0 = slots.stats["steps"]
                finished, _ = slots.run(self.inflight_steps)
                self.stats["decode_steps"] += slots.stats["steps"] - steps0
                self.stats["decode_calls"] += 1
                for slot in range(S):
                    if occupant[slot] is None or not finished[slot]:
                        continue
                    i, w, ask, t0 = occupant[slot]
                    row = slots.take(slot)
                    occupant[slot] = None
                    st = _build_generation_stats(row[None], dict(decoder_input_ids=ask["decoder_input_ids"].reshape(1, -1)), pad_id,
                                                 time.perf_counter() - t0)
                    self.stats["windows"] += 1
                    self.stats["generated_tokens"] += st["generated_tokens"]
                    jobs[i].on_result(w, row, st)
                    next_w[i] = w + 1
                    if next_w[i] < jobs[i].frames.shape[0]:
                        ready.append(i)
        finally:
            slots.close()
        self.stats["elapsed_seconds"] += time.perf_counter() - start
        return self.stats

    def _modes(self, gk: dict, nb: int) -> DecodeModes:
        """The mode switches of one decode call, the scheduler's own way: the cache route is read under beams only (a greedy window
        ignores it), self_kv_fp8 is refused first and cross_kv_fp8 last, the storage type is the engine's (None for a stand-in without)."""
        return DecodeModes.of(gk, getattr(self.engine, "dtype", None), nb, beam_switches=nb > 1, order=("self", "cache", "cross"))

    def _call_kwargs(self, gk0: dict) -> dict:
        """the kwargs of one decode call of a group"""
        # rows of different songs share this batch where the reference runs one batch-1 call per window: the conditional
        # temperature must look at each row's OWN history (the reference's processor reads row 0 of its batch)
        gk = dict(gk0, conditional_temperature_per_row=True)
        if gk.get("seed") is not None and gk.get("seed_call_index") is None:
            # explicit seed: the n-th decode call of THIS scheduler with that seed draws from stream (seed, n) -- the count is
            # the scheduler's own, so a run reproduces whatever else samples in the process (server.fresh_seed)
            n = self._seed_calls.get(gk["seed"], 0)
            self._seed_calls[gk["seed"]] = n + 1
            gk["seed_call_index"] = n
        return gk

    def _decode_group(self, jobs, kvs, w, group, pad_id, merged: bool = False):
        """merged: every entry of `group` is (job, ask, the kwargs of ITS call, its group's kwargs) (`_run_wave_merged`), the rows
        decode under their own"""
        eng, tok = self.engine, self.tokenizer
        row_sampling = None
        if merged:
            gk = group[0][2]               # (the per-call settings agree over the rows)
            row_sampling = build_row_sampling(tok, [g[2] for g in group], self.model.config.max_target_positions)
            sp, eos = row_sampling[0], []
        else:
            gk = self._call_kwargs(group[0][2])
            sp, eos = build_sampling(tok, gk, self.model.config.max_target_positions)
        cfg = sp.cfg_scale > 1.0
        nb = int(getattr(sp, "num_beams", 1) or 1)
        modes = self._modes(gk, nb)   # (a window's own generate_kwargs may switch a mode on: the same refusals)
        if len(group) * (2 if cfg else 1) * nb > 64:
            raise ValueError(f"{len(group)} windows{' x 2 (guidance)' if cfg else ''}{f' x {nb} beams' if nb > 1 else ''} exceed "
                             f"the engine's 64-row decode batch")
        prompts = _left_pad([g[1]["decoder_input_ids"] for g in group], pad_id, torch.int64)
        masks = None
        if any(g[1].get("decoder_attention_mask") is not None for g in group):
            masks = _left_pad([g[1]["decoder_attention_mask"] if g[1].get("decoder_attention_mask") is not None
                               else torch.ones_like(g[1]["decoder_input_ids"]) for g in group], 0, torch.uint8)
        elif any(g[1]["decoder_input_ids"].shape[-1] != prompts.shape[1] for g in group):
            # ragged prompts: only the left padding added HERE must not be attended -- a pad_id inside a caller's own
            # prompt stays visible, exactly as in the batch-1 call without a mask
            masks = _left_pad([torch.ones_like(g[1]["decoder_input_ids"]) for g in group], 0, torch.uint8)
        p_all, m_all = prompts, masks
        if cfg:      # [negative rows | prompt rows] of the left-padded prompts
            if any(g[1].get("negative_prompt") is None for g in group):
                raise ValueError("cfg_scale > 1 needs a negative_prompt for every window")
            p_all, m_all, _ = guided_rows(prompts, masks, _left_pad([g[1]["negative_prompt"] for g in group], pad_id, torch.int64))
        dev = eng.device
        eos_table = eos_id_table(eos, eng.packed.vocab_out)
        eos_ids = torch.as_tensor(sorted(set(int(e) for e in eos)), dtype=torch.int64)
        t0 = time.perf_counter()
        eng._enter()
        with eng.on_stream():
            kv = torch.stack([kvs[g[0]][:, :, w] for g in group], 2).contiguous()   # rows of this wave, gathered
            # cross_kv_fp8: the token steps stream an e4m3 copy of this wave's cross K / V (under beams the search makes it itself:
            # with guidance it is a copy of the doubled rows)
            kv8 = eng.cross_kv_fp8(kv) if modes.cross_kv_fp8 and nb == 1 else None
            if nb == 1:   # merged: every row under its own settings (mh_t5_generate_rows); eos_table is ignored there
                tokens, n_out, _ = eng.decode(kv, p_all.to(dev, torch.int32).contiguous(),
                                              None if m_all is None else m_all.to(dev).contiguous(), eos_table.to(dev), sp, kv_fp8=kv8,
                                              **modes.decode_kwargs(), **(dict(row_sampling=row_sampling) if merged else {}))
        eng._leave()
        if nb > 1:
            # HF beam search over the step-wise decode entry (beam.py), the windows of this wave as its batch: every window's
            # hypotheses are ranked among themselves only, so a window decodes as in the reference's batch-1 call; rows that
            # end early carry HF's fill (the first EOS id) and are cut at their first EOS-set id below like any other row
            from .beam import beam_search
            result = beam_search(eng, kv, p_all, m_all, eos, sp, nb, sample_fn=gk.get("beam_sample_fn"),
                                 **modes.beam_search_kwargs()).to(torch.int64).cpu()
        else:
            eng.synchronize()
            n_cols = int(n_out.item())
            if cfg:
                tokens = tokens[len(group):]
            result = tokens[:, :n_cols].to(torch.int64).cpu()
        elapsed = time.perf_counter() - t0
        self.stats["decode_calls"] += 1
        P = prompts.shape[1]
        redo = {}
        for r, (i, ask, *_) in enumerate(group):
            own = ask["decoder_input_ids"].shape[-1]
            row = result[r, P - own:]                      # strip the padding this batch added on the left
            # a row that finished early carries pad_id up to the batch's longest row: cut after its first EOS-set id,
            # which is where a batch-1 call for this window would have ended
            body = row[own:]
            cap = sp.max_length
            if merged:                                     # the row's own EOS set and cap
                eos_ids = row_sampling[2][row_sampling[1][r].eos_set].nonzero().reshape(-1)
                cap = row_sampling[1][r].max_length
                if row.shape[0] > cap - (P - own):         # (columns past the row's cap hold pad_id)
                    row, body = row[:cap - (P - own)], row[own:cap - (P - own)]
            hit = torch.isin(body, eos_ids).nonzero()
            if hit.numel():
                row = row[:own + int(hit[0]) + 1]
            elif own < P and row.shape[0] < cap:
                # no EOS and the row stopped at max_length COLUMNS, `P - own` of which were this batch's left padding: the
                # reference's batch-1 call (no padding) would have gone on to max_length tokens.  Rare (windows end by
                # EOS); such rows are decoded again among rows of their own prompt length, i.e. without padding.
                redo.setdefault(own, []).append(group[r])
                continue
            st = _build_generation_stats(row[None], dict(decoder_input_ids=ask["decoder_input_ids"].reshape(1, -1)),
                                         pad_id, elapsed)
            self.stats["windows"] += 1
            self.stats["generated_tokens"] += st["generated_tokens"]
            jobs[i].on_result(w, row, st)
        for sub in redo.values():
            if not merged:
                self._decode_group(jobs, kvs, w, sub, pad_id)
                continue
            # a redo decodes as the default policy's does: the rows of one group and one prompt length by themselves, under the
            # group's kwargs with the next seed call index and the RNG rows of that call
            again = {}
            for i, ask, _, gk0 in sub:
                again.setdefault(repr(sorted(gk0.items(), key=lambda kv_: kv_[0])), []).append((i, ask, gk0))
            for rows in again.values():
                self._decode_group(jobs, kvs, w, rows, pad_id)


# ---- the reference's own sequential loop on the scheduler -------------------------------------------------------------
def processor_generate_kwargs(proc, **window_kwargs) -> dict:
    """The kwargs `Processor.model_generate` (osuT5/osuT5/inference/processor.py:155-170) hands to the module-level
    `model_generate`: the window's own (lookback_time, lookahead_time, context_type) + the processor's sampling knobs."""
    return dict(window_kwargs, precision=proc.precision, do_sample=proc.do_sample, num_beams=proc.num_beams, top_p=proc.top_p,
                top_k=proc.top_k, max_length=proc.tgt_seq_len, cfg_scale=proc.cfg_scale, timeshift_bias=proc.timeshift_bias,
                types_first=proc.types_first, temperature=proc.temperature, timing_temperature=proc.timing_temperature,
                mania_column_temperature=proc.mania_column_temperature, taiko_hit_temperature=proc.taiko_hit_temperature)


def processor_song_job(proc, *, sequences, in_context, out_context, context_index: int, req_special_tokens,
                       model_kwargs: Optional[dict] = None) -> SongJob:
    """ONE pass of the reference's `Processor.generate_sequential` (processor.py:308-368) over output context
    `context_index` of one song, cut at its `self.model_generate(...)` call: everything in front of the call (the window's
    prompts from the contexts as they stand -- `prepare_context_sequences`, `get_prompts`, `pad_prompts` -- the lookback /
    lookahead EOS windows, the per-window song position) is `prompt_fn` / `conditioning_fn`, everything behind it
    (`_record_generation_stats`, `result[0, max_len:]`, `add_predicted_tokens_to_context`) is `on_result`.  `proc` is the
    reference's own `Processor` (duck-typed: its methods and attributes are used as they are -- the host logic stays the
    reference's), so a song decoded through SequentialWindowScheduler leaves `out_context` exactly as the reference loop
    does; many songs (one job each) share the scheduler's waves.  Several output contexts of a song = one scheduler run
    per `context_index`, in order, as the reference's outer loop does."""
    frames_all, frame_times, song_length = sequences
    n = len(frames_all)
    context = out_context[context_index]
    pending = {}
    pad_id = proc.tokenizer.pad_id
    model_kwargs = dict(model_kwargs or {})

    def prompt_fn(w: int) -> dict:
        frame_time = frame_times[w].item()
        trim_lookback = w != 0 and proc.lookback_time > 0
        trim_lookahead = w != n - 1
        cond_prompt, uncond_prompt = proc.get_prompts(
            proc.prepare_context_sequences(in_context, frame_time, False, req_special_tokens),
            proc.prepare_context_sequences(out_context[:context_index + 1], frame_time, True, req_special_tokens))
        [prompt, uncond_prompt], max_len = proc.pad_prompts([cond_prompt, uncond_prompt])
        pending[w] = (frame_time, max_len, trim_lookback, trim_lookahead)
        ask = dict(decoder_input_ids=prompt, decoder_attention_mask=prompt.ne(pad_id),
                   generate_kwargs=processor_generate_kwargs(
                       proc, lookback_time=proc.lookback_time if trim_lookback else 0,
                       lookahead_time=proc.lookahead_time if trim_lookahead else 0, context_type=context["context_type"].value))
        if uncond_prompt is not None:
            ask["negative_prompt"] = uncond_prompt
        return ask

    def on_result(w: int, row: torch.Tensor, stats: dict) -> None:
        frame_time, max_len, trim_lookback, trim_lookahead = pending.pop(w)
        proc._record_generation_stats(stats)
        proc.add_predicted_tokens_to_context(context, row[max_len:].cpu(), frame_time, trim_lookback, trim_lookahead)

    conditioning_fn = None
    if getattr(proc, "do_song_position_embed", False) or any(k in model_kwargs for k in ("difficulty", "mapper_idx", "beatmap_idx")):
        def conditioning_fn(w: int) -> dict:
            kw = {k: (v[0] if isinstance(v, torch.Tensor) and v.dim() > 0 and v.shape[0] == 1 else v)
                  for k, v in model_kwargs.items() if k in ("difficulty", "mapper_idx", "beatmap_idx")}
            if getattr(proc, "do_song_position_embed", False):
                ft = frame_times[w].item()
                kw["song_position"] = torch.tensor([ft / song_length, (ft + proc.miliseconds_per_sequence) / song_length],
                                                   dtype=torch.float32)
            return kw

    frames = torch.stack([proc.prepare_frames(f)[0] for f in frames_all])
    return SongJob(frames=frames, prompt_fn=prompt_fn, on_result=on_result, conditioning_fn=conditioning_fn)
