"""Beam search on the HIP engine (`num_beams > 1`).

The reference hands `num_beams` to HF `generate` (osuT5/osuT5/inference/processor.py:147,159; its timing generator decodes
with two beams, config.py:71) and reorders its static caches per step (`MapperatorinatorCache.reorder_cache`,
inference/cache_utils.py:16-20).  The selection logic is HF's (third-party; the algorithm below restates the published,
vectorised `GenerationMixin._beam_search` -- transformers >= 4.50; line references are to the installed 5.x
`generation/utils.py`): per step

    log_probs = processors(sequences, log_softmax(logits))            (b: processors act on LOG-PROBABILITIES here)
    accumulated = log_probs + running_beam_scores                      -> top K continuations (`_n_candidates`)
    candidates that hit an EOS id / max_length leave the running set   (e), the next `num_beams` others keep running
    finished hypotheses among the TOP num_beams candidates are merged into the finished set by score / length ** penalty   (f)
    the cache rows follow the surviving beams                           (g)
    stop when no running beam can still beat the worst finished one (early_stopping = False heuristic)

The device side is the step-wise entry of the library (`mh_t5_step`: one decoder position for all (chunk, beam) rows, raw
logits out -- `mh_t5_step_fp8` when the search is handed the e4m3 copy of the cross K/V, `kv_fp8`; `mh_t5_reorder_cache`).  Round 6: for greedy beams the WHOLE bookkeeping above is one kernel per token, `mh_beam_step`
(csrc/beam.hip: log_softmax, guidance, processors, top-K over beams x V by a radix select + a sort of the K, EOS split, next-beam
selection, finished-set merge, the early-stopping heuristic; 2 .. 8 beams, K <= 8192, any vocabulary: the scores live in LDS where
they fit 120 KB, else a streaming kernel recomputes them from the logits, same bits) -- `_beam_search_kernel` below; the host reads three flags per chunk and step.  The torch-op
form (`beam_search` with use_kernel=False; ~40 ATen launches per token) stays for beam-SAMPLE as HF draws it (torch.multinomial / an
injected sampler: the default), and as the cross-check of the kernel (tests run both against the reference goldens).  The two forms
differ only in how continuations are ranked: `beam_search` builds one `_BeamDecoder` -- guidance doubling, row counts and refusals,
K, the prompt rows, the buffers, the prompt feed, `step` / `reorder` over the cache route (`_CopiedCache` or `_IndexedCache`, one
surface), the returned slice -- and hands it to `_beam_search_kernel` or `_beam_search_torch_ops`.  The logits processors of
server.py:106-134 are applied here with torch ops (the in-kernel sampler of the greedy / sampling path selects per row and
cannot rank across beams): classifier-free guidance, MonotonicTimeShift, TimeshiftBias, (Conditional)Temperature and the lookback
warper, both branches.  Its types_first branch (logit_processors.py:116-133) keeps `last_scores` from call to call and indexes them by
ROW SLOT: HF reorders the beams between two steps and the warper never sees `beam_idx`, so slot r renormalises with the EOS mass of
whatever beam sat in slot r one step earlier.  Reproduced verbatim by both forms -- `BeamProcessors.last_scores` here, one fp32 per
slot (`lookback_prev`, never gathered by `src`) in mh_beam_step_tf -- and pinned by tests/golden/t5_tiny_tf_beam.npz.

Beam-sample (`do_sample` with beams, round 5; processor.py:147-160 hands both to `generate`): HF appends its top-k / top-p warpers
BEHIND the reference's processor list with `min_tokens_to_keep = #eos + 1` (utils.py `_get_logits_processor`), and
`_get_top_k_continuations` draws the K continuations with `torch.multinomial(softmax(accumulated), K)` -- without replacement, in
draw order (not sorted: "inside the top num_beams" then means "among the first num_beams draws").  The draw uses torch's generator
on the engine's device, like HF on a GPU; `sample_fn(probs, k)` replaces it (parity tests inject the sampler the reference golden
was drawn with).  Opt-in, `device_draw=True`: the draw moves INTO the step kernel (`mh_beam_step_sample`: HF's two warpers as one
cut value per beam row, then Gumbel top-K -- key = accumulated score + -log(-log(u)), u from the library's counter-based generator
keyed by (sp.seed, sp.rng_row0 + chunk, decode column, beam x V + id); the K largest keys, ties by flat index, are K draws without
replacement in draw order: include/mapperhip.h), one kernel per token like greedy beams.  It is another stream of random numbers than
torch.multinomial's, with the same distribution; `use_kernel=False` then draws by the same rule with torch ops (`_device_draw`), the
kernel's cross-check.

Guidance under beams (round 5; the timing pass sets beams, `super_timing_generator.py:28`, and `processor.py:709` halves its batch
for exactly this case) follows what the reference + HF do, quirk included:
  * `prepare_inputs_for_generation` (modeling_mapperatorinator.py:243-254) doubles the (chunk, beam) rows every step: the first
    half carries the negative prompt over the first columns, the second half is the prompt's own rows;
  * HF's `ClassifierFreeGuidanceLogitsProcessor` runs FIRST in the list, on log_softmax(logits) of all 2R rows, and treats the
    first half as the conditional one: guided = second + (first - second) * scale, R rows; the other processors see the prompt rows'
    sequences;
  * `MapperatorinatorCache.reorder_cache` (inference/cache_utils.py:16-20) gathers the doubled cache with `beam_idx.repeat(2)` --
    indices into the FIRST half for both halves: from the first reorder on, the prompt half's self-attention cache holds copies of the
    negative half's rows.  Reproduced verbatim (golden `t5_tiny_beam.npz`, runs `b2g` / `b3g`).

Long targets (opt-in, `cache="indexed"`): step (g) copies the whole cache after every token -- 4 x the cache's bytes up to the current
position.  The indexed route keeps every cache row where its step wrote it and lets attention follow a uint8 (rows, tgt_len) table
instead (`mh_t5_step_indexed`; a reorder is `mh_t5_reorder_index` from one table into the other, `beam_idx.repeat(2)` included):
bit-identical logits, no scratch buffer.  `prefill=True` on top of it sends positions 0 .. P-2 of each chunk's prompt (all beams of a
chunk carry the same one) through the batched prefill of mh_t5_generate once (`mh_t5_step_prefill`) and starts the table with
origin = the chunk's row for those positions.  `self_kv_fp8=True` on top of the indexed route: the steps attend an e4m3 shadow of the
cache (`mh_t5_step_indexed_skv8`) whose rows and scales also stay where their step wrote them and are read through the same table;
after a prefill the prompt rows are quantised in place (`mh_t5_self_kv_fp8_fill`).  The copy route has no such form.

How the generate kwargs of the hosts above (`beam_cache`, `beam_prefill`, `beam_sample_kernel`, the two fp8 switches) become this
module's keywords, and where they are refused: decode_modes.py.
"""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import Optional

import torch

from . import _lib
from .decode_modes import check_cache_mode, require_bf16_for_cross_kv_fp8, require_bf16_for_self_kv_fp8  # noqa: F401


def _gather(t: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    while idx.dim() < t.dim():
        idx = idx.unsqueeze(-1)
    return torch.take_along_dim(t, idx, dim=1)


class BeamProcessors:
    """The reference's processor list (server.py:106-134) on (rows, V) LOG-PROBABILITIES, from an MhSampling struct."""

    def __init__(self, sp, device, min_tokens_to_keep: int = 1):
        self.min_tokens_to_keep = int(min_tokens_to_keep)
        self.sp = sp
        self.sos = torch.tensor([sp.sos_ids[i] for i in range(sp.n_sos)], dtype=torch.long, device=device)
        flags = getattr(sp, "host_tok_flags", None)
        self.flags = None if flags is None else torch.as_tensor(flags, dtype=torch.uint8, device=device)
        self.last_scores = None          # LookbackBiasLogitsWarper types_first: what entered it at the previous call, BY ROW SLOT

    def _flag(self, ids: torch.Tensor, bit: int) -> torch.Tensor:
        """bit `bit` of tok_flags per id; an input-only id (>= vocab_out) has no flags"""
        n = self.flags.shape[0]
        return (ids < n) & ((self.flags[ids.clamp(0, n - 1)] & bit) != 0)

    def __call__(self, ids: torch.Tensor, scores: torch.Tensor) -> torch.Tensor:
        sp = self.sp
        scores = scores.clone()
        R, T = ids.shape
        # MonotonicTimeShiftLogitsProcessor (logit_processors.py:136-183)
        if sp.ts_end > sp.ts_start:
            idx = torch.arange(T, device=ids.device).expand(R, -1)
            is_ts = (ids >= sp.ts_start) & (ids < sp.ts_end)
            is_sos = torch.isin(ids, self.sos)
            last_ts = torch.where(is_ts, idx, -1).max(1).values
            last_sos = torch.where(is_sos, idx, -1).max(1).values
            val = torch.where(last_ts != -1, ids[torch.arange(R, device=ids.device), last_ts.clamp(min=0)] - sp.ts_start, 0)
            apply = (last_ts != -1) & (last_ts > last_sos)
            vocab = torch.arange(sp.ts_start, sp.ts_end, device=ids.device)
            bad = apply[:, None] & (vocab[None, :] < (sp.ts_start + val)[:, None])
            scores[:, sp.ts_start:sp.ts_end] = scores[:, sp.ts_start:sp.ts_end].masked_fill(bad, float("-inf"))
            if sp.timeshift_bias != 0.0:                                     # TimeshiftBias (:36-44)
                scores[:, sp.ts_start:sp.ts_end] += sp.timeshift_bias
        # (Conditional)TemperatureLogitsWarper (:47-82): row 0's history picks the temperature of the whole call
        temp = torch.full((R,), float(sp.temperature), device=ids.device)
        if sp.n_cond > 0:
            if self.flags is None:
                raise ValueError("conditional temperature needs tok_flags")
            rows = ids if sp.cond_per_row else ids[:1].expand(R, -1)
            chosen = torch.zeros(R, dtype=torch.bool, device=ids.device)
            for j in range(sp.n_cond):
                off = int(sp.cond_offset[j])
                if T >= off:
                    hit = self._flag(rows[:, T - off], 2 << j) & ~chosen
                    temp = torch.where(hit, torch.full_like(temp, float(sp.cond_temp[j])), temp)
                    chosen |= hit
        scores = scores / temp[:, None]
        if sp.lookback_mask_end > sp.ts_start and sp.lookback_types_first:    # LookbackBiasLogitsWarper, types_first True (:116-133)
            if self.flags is None:
                raise ValueError("the types_first lookback needs tok_flags")
            entered = scores
            if T != 0 and self.last_scores is not None:
                last_timed = self._flag(ids[:, -1], 1)
                if bool(last_timed.any()):
                    lo, hi = sp.ts_start, sp.lookback_mask_end
                    last_probs = torch.softmax(self.last_scores, dim=-1)           # (row r of the PREVIOUS call, whichever beam it held)
                    probs = torch.softmax(scores, dim=-1)
                    prob_eos = last_probs[:, (self.flags & 16) != 0].sum(dim=-1)
                    prob_event = 1 - prob_eos
                    other = torch.cat((probs[:, :lo], probs[:, hi:]), 1).sum(dim=-1)     # probs[:, other_range], same order
                    s = 1 / (other * prob_event + prob_eos)
                    probs = probs * s.unsqueeze(1)
                    probs[:, lo:hi] = 0
                    probs[:, lo] = torch.clip((s - 1) * prob_eos / prob_event, 0, 1)
                    scores = torch.where(last_timed.unsqueeze(1), torch.log(probs), scores)
            self.last_scores = entered
        elif sp.lookback_mask_end > sp.ts_start:                              # ... types_first False (:111-114)
            scores[:, sp.ts_start:sp.lookback_mask_end] = float("-inf")
        if sp.do_sample:      # HF's own warpers, appended behind the list: TopK then TopP, at least #eos + 1 tokens kept under beams
            keep = self.min_tokens_to_keep
            if sp.top_k > 0:
                kth = torch.topk(scores, min(max(int(sp.top_k), keep), scores.shape[-1]))[0][..., -1, None]
                scores = scores.masked_fill(scores < kth, float("-inf"))
            if sp.top_p < 1.0:
                srt, order = torch.sort(scores, descending=False)
                drop = srt.softmax(dim=-1).cumsum(dim=-1) <= (1 - float(sp.top_p))
                drop[..., -keep:] = False
                scores = scores.masked_fill(drop.scatter(1, order, drop), float("-inf"))
        return scores


def _n_candidates(num_beams: int, vocab_out: int, n_eos: int) -> int:
    """K, the continuations HF ranks per chunk and step (`_get_top_k_continuations`): num_beams of them keep running even when every
    EOS id took a place among them; never more than there are (beam, id) pairs."""
    return min(max(2, 1 + n_eos) * num_beams, num_beams * vocab_out)


_KERNEL_LIMITS = "beams outside 2 .. 8 or K = max(2, 1 + #eos) x beams > 8192"      # (the refusals' words for _n_candidates)


def _min_tokens_to_keep(n_eos: int) -> int:
    """what HF hands its top-k / top-p warpers under beams (utils.py `_get_logits_processor`)"""
    return n_eos + 1 if n_eos else 2


def kernel_path_available(sp, num_beams: int, vocab_out: int, n_eos: int) -> bool:
    """mh_beam_step / mh_beam_step_tf cover greedy beams (no beam-sample: `do_sample` decides before anything else is read), 2 .. 8
    beams, K <= 8192 candidates and any vocabulary: the library says which of its two kernels a shape runs (mh_beam_step_path; 0 =
    refused)."""
    K = _n_candidates(int(num_beams), int(vocab_out), n_eos)
    return (not sp.do_sample) and _lib.load().mh_beam_step_path(int(num_beams), int(vocab_out), K) != 0


_GOLDEN = 0x9E3779B97F4A7C15


def _s64(x: int) -> int:
    """a 64-bit pattern as the int64 that holds it"""
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >> 63 else x


def _lsr(z: torch.Tensor, s: int) -> torch.Tensor:
    """logical shift right of the 64-bit patterns in an int64 tensor"""
    return (z >> s) & ((1 << (64 - s)) - 1)


def _rng_mix64(seed: torch.Tensor, row: torch.Tensor, step: torch.Tensor) -> torch.Tensor:
    """rng_mix64 of csrc/common.hpp on int64 tensors (the 64-bit patterns; int64 products wrap like the device's uint64_t)"""
    z = seed + (row * 0x100000001 + step + 1) * _s64(_GOLDEN)
    z = (z ^ _lsr(z, 30)) * _s64(0xBF58476D1CE4E5B9)
    z = (z ^ _lsr(z, 27)) * _s64(0x94D049BB133111EB)
    return z ^ _lsr(z, 31)


def _device_draw(acc: torch.Tensor, K: int, seed: int, row0: int, cur_len: int, keys_out: Optional[list] = None) -> torch.Tensor:
    """The draw of mh_beam_step_sample in torch ops on acc fp32 (G, num_beams x V): int64 splitmix for u (bit-exact), fp32 keys
    acc + -log(-log(u)), a stable descending sort so that ties fall by flat index.  -> indices (G, K) in draw order.  `keys_out`: a
    list that receives the sorted keys (G, num_beams x V) of the call (tests measure how far apart the deciding keys are)."""
    G, n = acc.shape
    dev = acc.device
    i64 = dict(dtype=torch.int64, device=dev)
    rows = (torch.arange(G, **i64) + int(row0)) & 0xFFFFFFFF
    sub = _rng_mix64(torch.tensor(_s64(int(seed)), **i64), rows, torch.tensor(int(cur_len) & 0xFFFFFFFF, **i64))
    z = _rng_mix64(sub[:, None], torch.zeros((), **i64), torch.arange(n, **i64)[None, :])
    u = (_lsr(z, 40).to(torch.float64) + 0.5).to(torch.float32) * (1.0 / 16777216.0)
    u = torch.clamp(u, max=1.0 - 2.0 ** -24)
    key = acc + -torch.log(-torch.log(u))
    srt, order = torch.sort(key, dim=1, descending=True, stable=True)
    if keys_out is not None:
        keys_out.append(srt)
    return order[:, :K]


def _step_kv_fp8(engine, cross_kv: torch.Tensor, kv_fp8):
    """The packed e4m3 copy the steps stream, or None.  `cross_kv` is the tensor the steps are handed -- under guidance the rows
    already doubled: a copy of the undoubled rows is made again, so that the packed layout stays [data | scales] of ONE tensor."""
    if kv_fp8 is None or kv_fp8 is False:
        return None
    require_bf16_for_cross_kv_fp8(engine.dtype)
    want = int(engine.lib.mh_t5_cross_kv_fp8_bytes(C.byref(engine.packed.cfg), cross_kv.shape[2]))
    if kv_fp8 is True or kv_fp8.numel() != want:
        engine._enter()                                  # (the engine's stream waits for the concatenation above)
        with torch.cuda.stream(engine.stream):
            kv_fp8 = engine.cross_kv_fp8(cross_kv.contiguous())
        engine._leave()
    return kv_fp8


def _self_kv_shadow(engine, rows, self_kv_fp8):
    """The e4m3 shadow of the self-attention cache for the `rows` rows the decoder runs (guidance doubling included), from the
    engine's workspace "skv8" -- the one T5Engine.decode uses; or None."""
    if not self_kv_fp8:
        return None
    n = int(engine.lib.mh_t5_self_kv_fp8_bytes(C.byref(engine.packed.cfg), rows))
    if n <= 0:
        raise ValueError(f"the e4m3 self-attention cache does not cover {rows} rows")
    return engine._workspace("skv8", n)


class _IndexedCache:
    """cache="indexed": the self-attention cache rows stay where the steps wrote them; two uint8 (rows, tgt_len) tables say which
    cache row holds each (row, position) (mh_t5_step_indexed), and a reorder permutes table rows (mh_t5_reorder_index) from one
    table into the other.  `start` with n_pos > 0 (the prompt prefill: n_pos positions of the `groups` prompts, one mh_t5_step_prefill
    call) fills cache rows 0 .. groups-1 and starts the table with them.
    `skv8` (self_kv_fp8): the e4m3 shadow of the self-attention cache for `rows` rows; the steps then go through
    mh_t5_step_indexed_skv8, which reads the shadow through the same table, and a prefill is followed by mh_t5_self_kv_fp8_fill."""

    def __init__(self, lib, p, rows, kv_group, ws, stream, skv8=None):
        self.lib, self.p, self.rows, self.kv_group, self.ws, self.stream, self.skv8 = lib, p, rows, kv_group, ws, stream, skv8
        n = int(lib.mh_t5_beam_index_bytes(C.byref(p.cfg), rows))
        if n <= 0:
            raise ValueError(f"the index table does not cover {rows} rows")
        self.tables = [torch.empty(n, dtype=torch.uint8, device=ws.device) for _ in range(2)]
        self.cur = 0

    def start(self, cross_kv, prompts, masks, n_pos):
        """Before the first token step.  n_pos > 0: positions 0 .. n_pos-1 of every prompt are prefilled -- prompts int32 (groups, P)
        on the device, masks uint8 (groups, P) or None"""
        cfg, ws = C.byref(self.p.cfg), self.ws
        if n_pos:
            G, P = prompts.shape
            rc = self.lib.mh_t5_step_prefill(cfg, C.byref(self.p.w), cross_kv.data_ptr(), G, prompts.data_ptr(), _lib.ptr(masks), P,
                                             int(n_pos), ws.data_ptr(), ws.numel(), self.rows, self.stream)
            _lib.check(rc, "mh_t5_step_prefill")
            if self.skv8 is not None:      # the prompt rows the prefill wrote, quantised where they are
                rc = self.lib.mh_t5_self_kv_fp8_fill(cfg, self.rows, G, int(n_pos), ws.data_ptr(), ws.numel(), self.skv8.data_ptr(),
                                                     self.stream)
                _lib.check(rc, "mh_t5_self_kv_fp8_fill")
        rc = self.lib.mh_t5_beam_index_init(cfg, self.rows, self.kv_group, int(n_pos), self.tables[self.cur].data_ptr(), self.stream)
        _lib.check(rc, "mh_t5_beam_index_init")

    def step(self, cross_kv, kv_fp8, tokens, pos, mask, P, logits):
        ws, table = self.ws, self.tables[self.cur]
        if self.skv8 is not None:
            rc = self.lib.mh_t5_step_indexed_skv8(C.byref(self.p.cfg), C.byref(self.p.w), cross_kv.data_ptr(), _lib.ptr(kv_fp8), self.rows,
                                                  self.kv_group, tokens.data_ptr(), pos, _lib.ptr(mask), P, logits.data_ptr(),
                                                  ws.data_ptr(), ws.numel(), table.data_ptr(), self.skv8.data_ptr(), self.stream)
            _lib.check(rc, "mh_t5_step_indexed_skv8")
            return
        rc = self.lib.mh_t5_step_indexed(C.byref(self.p.cfg), C.byref(self.p.w), cross_kv.data_ptr(), _lib.ptr(kv_fp8), self.rows,
                                         self.kv_group, tokens.data_ptr(), pos, _lib.ptr(mask), P, logits.data_ptr(), ws.data_ptr(),
                                         ws.numel(), table.data_ptr(), self.stream)
        _lib.check(rc, "mh_t5_step_indexed")

    def reorder(self, src, n_pos):
        rc = self.lib.mh_t5_reorder_index(C.byref(self.p.cfg), self.rows, src.data_ptr(), int(n_pos), self.tables[self.cur].data_ptr(),
                                          self.tables[self.cur ^ 1].data_ptr(), self.stream)
        _lib.check(rc, "mh_t5_reorder_index")
        self.cur ^= 1


class _CopiedCache:
    """cache="copy", HF's route: after every token cache row b <- row src[b] over the positions so far (mh_t5_reorder_cache: a gather
    into a scratch buffer and a scatter back).  The steps are mh_t5_step, or mh_t5_step_fp8 over the e4m3 copy of the cross K/V when
    there is one.  No prefill and no e4m3 self cache (`check_cache_mode`, require_bf16_for_self_kv_fp8)."""

    def __init__(self, lib, p, rows, kv_group, ws, stream, max_length):
        self.lib, self.p, self.rows, self.kv_group, self.ws, self.stream = lib, p, rows, kv_group, ws, stream
        n = int(lib.mh_t5_reorder_cache_scratch_bytes(C.byref(p.cfg), rows, max_length))
        self.scratch = torch.empty(n, dtype=torch.uint8, device=ws.device)

    def start(self, cross_kv, prompts, masks, n_pos):
        assert n_pos == 0      # every prompt column is a token step

    def step(self, cross_kv, kv_fp8, tokens, pos, mask, P, logits):
        lib, cfg, w, ws = self.lib, C.byref(self.p.cfg), C.byref(self.p.w), self.ws
        if kv_fp8 is None:
            rc = lib.mh_t5_step(cfg, w, cross_kv.data_ptr(), self.rows, self.kv_group, tokens.data_ptr(), pos, _lib.ptr(mask), P,
                                logits.data_ptr(), ws.data_ptr(), ws.numel(), self.stream)
            _lib.check(rc, "mh_t5_step")
        else:
            rc = lib.mh_t5_step_fp8(cfg, w, cross_kv.data_ptr(), kv_fp8.data_ptr(), self.rows, self.kv_group, tokens.data_ptr(), pos,
                                    _lib.ptr(mask), P, logits.data_ptr(), ws.data_ptr(), ws.numel(), self.stream)
            _lib.check(rc, "mh_t5_step_fp8")

    def reorder(self, src, n_pos):
        rc = self.lib.mh_t5_reorder_cache(C.byref(self.p.cfg), self.rows, src.data_ptr(), int(n_pos), self.ws.data_ptr(), self.ws.numel(),
                                          self.scratch.data_ptr(), self.scratch.numel(), self.stream)
        _lib.check(rc, "mh_t5_reorder_cache")


class _BeamDecoder:
    """The decoder side of a beam search, shared by its two bookkeeping forms, which differ only in how they rank continuations.
    Built once per `beam_search` call: the row counts (G chunks x nb beams = R rows the bookkeeping ranks, RE rows the engine
    decodes: 2 R under guidance, the negative prompt's rows in front), the refusals, K / `fill` / `n_new` / `min_tokens_to_keep`,
    and the prompt rows as the engine is fed them (`ids0e` int32 (RE, P), `mask` uint8 (RE, P) or None).  Inside `running()` there
    are also the buffers -- the cross K/V as the steps read it (doubled under guidance; its e4m3 copy `kv_fp8`), the workspace that
    holds the caches, `logits` fp32 (RE, V), `stream` -- and the cache route (`_CopiedCache` / `_IndexedCache`) behind
    `feed_prompt` / `step` / `reorder`; a call that is refused before it runs allocates none of them."""

    def __init__(self, engine, cross_kv, prompt, prompt_mask, eos_ids, sp, num_beams, kv_fp8, cache, prefill, self_kv_fp8):
        self.engine, self.cross_kv, self.kv_fp8 = engine, cross_kv, kv_fp8
        self.indexed, self.prefill, self.self_kv_fp8 = cache == "indexed", bool(prefill), self_kv_fp8
        dev, p = engine.device, engine.packed
        self.guided = sp.cfg_scale > 1.0
        if self.guided and prompt.shape[0] % 2:
            raise ValueError("guidance: the prompt batch must be [negative rows | prompt rows]")
        self.G, self.P = prompt.shape[0] // (2 if self.guided else 1), prompt.shape[1]
        self.nb = nb = int(num_beams)
        self.R = self.G * nb
        self.RE = 2 * self.R if self.guided else self.R
        if self.RE > 64:
            raise ValueError(f"{self.G} chunks x {nb} beams{' x 2 (guidance)' if self.guided else ''} exceed the engine's 64-row decode batch")
        self.V = p.vocab_out
        self.max_length = int(sp.max_length)
        if not (1 <= self.P < self.max_length <= p.tgt_len):
            raise ValueError("prompt / max_length do not fit the cache")
        self.eos = [int(e) for e in eos_ids]
        self.K = _n_candidates(nb, self.V, len(self.eos))
        self.min_tokens_to_keep = _min_tokens_to_keep(len(self.eos))
        self.fill = int(sp.pad_id) or (self.eos[0] if self.eos else -1)       # HF: `pad_token_id or eos_token_id[0]`
        self.n_new = self.max_length - self.P
        # rows (chunk, beam); under guidance the negative rows come first, as `prompt` / `prompt_mask` carry them
        self.ids0e = prompt.to(dev, torch.int32).repeat_interleave(nb, 0)
        self.mask = None if prompt_mask is None else prompt_mask.to(dev).to(torch.uint8).repeat_interleave(nb, 0).contiguous()

    @contextlib.contextmanager
    def running(self):
        """Makes the buffers and the cache route; inside, the engine's stream is current, behind everything enqueued before."""
        e = self.engine
        lib, p, dev, RE = e.lib, e.packed, e.device, self.RE
        if self.guided:      # [layer][k|v][chunk][H][L][64]: the negative rows read their chunk's K / V
            self.cross_kv = torch.cat([self.cross_kv, self.cross_kv], dim=2)
        self.kv_fp8 = _step_kv_fp8(e, self.cross_kv, self.kv_fp8)
        ws = torch.empty(int(lib.mh_t5_decode_workspace_bytes(C.byref(p.cfg), RE)), dtype=torch.uint8, device=dev)
        self.logits = torch.empty((RE, self.V), dtype=torch.float32, device=dev)
        self.stream = e._s()
        if self.indexed:     # two index tables instead of the copy's scratch buffer
            self.cache = _IndexedCache(lib, p, RE, self.nb, ws, self.stream, skv8=_self_kv_shadow(e, RE, self.self_kv_fp8))
        else:
            self.cache = _CopiedCache(lib, p, RE, self.nb, ws, self.stream, self.max_length)
        e._enter()
        with torch.cuda.stream(e.stream):
            yield
        e._leave()
        e.synchronize()

    def feed_prompt(self):
        """Prompt columns 0 .. P-2 into the caches (column P-1 is the search's first step): with `prefill` in one batched pass, once
        per chunk (all beams of a chunk carry the same prompt: every nb-th row), else token by token."""
        n = self.P - 1 if self.prefill else 0
        prompts = masks = None
        if n:
            prompts = self.ids0e[::self.nb].contiguous()
            masks = None if self.mask is None else self.mask[::self.nb].contiguous()
        self.cache.start(self.cross_kv, prompts, masks, n)
        for pos in range(n, self.P - 1):
            self.step(self.ids0e[:, pos].contiguous(), pos)

    def step(self, tokens: torch.Tensor, pos: int):
        """One decoder position for all RE rows -> `logits`.  tokens (RE,): int32 as they are, int64 converted."""
        if tokens.dtype != torch.int32:
            tokens = tokens.to(torch.int32).contiguous()
        self.cache.step(self.cross_kv, self.kv_fp8, tokens, pos, self.mask, self.P, self.logits)

    def reorder(self, src: torch.Tensor, cur_len: int):
        """The caches follow the beams: row b continues row src[b] (int32 (RE,)) over positions 0 .. cur_len-1."""
        self.cache.reorder(src, cur_len)

    def finish(self, sequences: torch.Tensor, beam_bidx: torch.Tensor) -> torch.Tensor:
        """sequences (G, nb, max_length), beam_bidx (G, nb, n_new; -1 = not generated) of the finished set -> the best hypothesis
        per chunk, int64 (G, P + the longest generated length)"""
        best = sequences[:, 0, :].to(torch.int64)
        n_gen = int(((beam_bidx[:, 0, :] + 1).bool()).sum(dim=1).max())
        return best[:, :self.P + n_gen].clone()


@torch.no_grad()
def _beam_search_kernel(dec: _BeamDecoder, sp, length_penalty, early_stopping, sample_keep: Optional[int] = None) -> torch.Tensor:
    """`beam_search` with the per-token bookkeeping in mh_beam_step: per token mh_t5_step -> mh_beam_step -> mh_t5_reorder_cache and ONE
    D2H copy of 3 G flags (HF's loop condition); the hypotheses live in int32 device arrays that the kernel ping-pongs.  With the
    types_first lookback the step is mh_beam_step_tf over `lookback_prev`, one fp32 per row slot that stays where it is.
    `sample_keep` (beam-sample with the draw in the kernel): the step is mh_beam_step_sample with min_tokens_to_keep = sample_keep."""
    dev, lib = dec.engine.device, dec.engine.lib
    G, nb, R, RE, V, P, max_length, n_new = dec.G, dec.nb, dec.R, dec.RE, dec.V, dec.P, dec.max_length, dec.n_new
    eos_table = torch.zeros(V, dtype=torch.uint8, device=dev)
    good = [e for e in dec.eos if 0 <= e < V]
    if good:
        eos_table[torch.tensor(good, dtype=torch.long, device=dev)] = 1
    types_first = bool(sp.lookback_types_first) and sp.lookback_mask_end > sp.ts_start
    flags_h = getattr(sp, "host_tok_flags", None)
    flags_d = None                                   # (alive until the last step has run: the kernel reads it through bs.sp.tok_flags)
    if flags_h is not None:
        flags_d = torch.as_tensor(flags_h, dtype=torch.uint8).to(dev)
    elif sp.n_cond or types_first:
        raise ValueError("conditional temperature / the types_first lookback need tok_flags (build the sampling struct with "
                         "server.build_sampling)")
    # LookbackBiasLogitsWarper types_first: prob_eos of what entered the processor one step earlier, per row SLOT; < 0 = no call yet
    lookback_prev = torch.full((R,), -1.0, dtype=torch.float32, device=dev) if types_first else None

    def state():
        run = torch.full((G, nb, max_length), dec.fill, dtype=torch.int32, device=dev)
        run[:, :, :P] = dec.ids0e[-R:].view(G, nb, P)
        rs = torch.zeros((G, nb), dtype=torch.float32, device=dev)
        rs[:, 1:] = -1e9
        return dict(run=run, rs=rs, rb=torch.full((G, nb, n_new), -1, dtype=torch.int32, device=dev), seq=run.clone(),
                    bs=torch.full((G, nb), -1e9, dtype=torch.float32, device=dev),
                    bb=torch.full((G, nb, n_new), -1, dtype=torch.int32, device=dev),
                    fin=torch.zeros((G, nb), dtype=torch.uint8, device=dev))
    st = [state(), state()]
    heuristic_open = torch.ones(G, dtype=torch.uint8, device=dev)
    src = torch.zeros(RE, dtype=torch.int32, device=dev)       # the kernel writes both halves under guidance
    feed = torch.zeros(RE, dtype=torch.int32, device=dev)      # ... and the token every row is fed next
    flags = torch.zeros((G, 3), dtype=torch.int32, device=dev)
    flags_host = torch.zeros((G, 3), dtype=torch.int32).pin_memory()
    bs = _lib.MhBeamStep()
    bs.eos_table = eos_table.data_ptr()
    bs.G, bs.num_beams, bs.V, bs.P, bs.max_length, bs.K = G, nb, V, P, max_length, dec.K
    bs.cfg, bs.cfg_scale, bs.length_penalty = int(dec.guided), float(sp.cfg_scale), float(length_penalty)
    bs.early_stopping = 2 if early_stopping == "never" else (1 if early_stopping is True else 0)
    bs.sp = sp                                       # (a copy: the caller's struct keeps its tok_flags)
    if flags_d is not None:
        bs.sp.tok_flags = flags_d.data_ptr()
    bs.heuristic_open, bs.src, bs.last, bs.flags = heuristic_open.data_ptr(), src.data_ptr(), feed.data_ptr(), flags.data_ptr()
    with dec.running():
        bs.logits, stream = dec.logits.data_ptr(), dec.stream
        dec.feed_prompt()
        feed.copy_(dec.ids0e[:, P - 1])                # the last prompt column (under guidance the first half has the negative prompt's)
        cur_len, par = P, 0
        while True:
            dec.step(feed, cur_len - 1)
            a, b = st[par], st[par ^ 1]
            bs.cur_len = cur_len
            bs.run_in, bs.rs_in, bs.rb_in = a["run"].data_ptr(), a["rs"].data_ptr(), a["rb"].data_ptr()
            bs.seq_in, bs.bs_in, bs.bb_in, bs.fin_in = a["seq"].data_ptr(), a["bs"].data_ptr(), a["bb"].data_ptr(), a["fin"].data_ptr()
            bs.run_out, bs.rs_out, bs.rb_out = b["run"].data_ptr(), b["rs"].data_ptr(), b["rb"].data_ptr()
            bs.seq_out, bs.bs_out, bs.bb_out, bs.fin_out = b["seq"].data_ptr(), b["bs"].data_ptr(), b["bb"].data_ptr(), b["fin"].data_ptr()
            if sample_keep is not None:
                _lib.check(lib.mh_beam_step_sample(C.byref(bs), _lib.ptr(lookback_prev), int(sample_keep), None, stream),
                           "mh_beam_step_sample")
            elif types_first:
                _lib.check(lib.mh_beam_step_tf(C.byref(bs), lookback_prev.data_ptr(), stream), "mh_beam_step_tf")
            else:
                _lib.check(lib.mh_beam_step(C.byref(bs), stream), "mh_beam_step")
            par ^= 1
            # (`src` / `feed` were written by the kernel for all RE rows: under guidance `beam_idx.repeat(2)`, cache_utils.py:18, and the
            # beam's token for both halves)
            dec.reorder(src, cur_len)
            cur_len += 1
            flags_host.copy_(flags, non_blocking=True)
            dec.engine.stream.synchronize()
            f = flags_host.numpy()
            go_on = bool(f[:, 0].any()) and not (bool(f[:, 2].all()) and early_stopping is True) and not bool(f[:, 1].all())
            if not go_on:
                break
        out = dec.finish(st[par]["seq"], st[par]["bb"])
    return out


@torch.no_grad()
def beam_search(engine, cross_kv: torch.Tensor, prompt: torch.Tensor, prompt_mask: Optional[torch.Tensor], eos_ids, sp,
                num_beams: int, length_penalty: float = 1.0, early_stopping=False, sample_fn=None,
                use_kernel: Optional[bool] = None, kv_fp8=None, device_draw: bool = False, cache: str = "copy",
                prefill: bool = False, self_kv_fp8: bool = False) -> torch.Tensor:
    """cross_kv: the G chunks' cross K/V (engine.cross_kv); prompt int (G, P) left-padded, prompt_mask (G, P) or None.
    Under guidance (sp.cfg_scale > 1) `prompt` / `prompt_mask` carry 2G rows, [negative-prompt rows | prompt rows] (what
    T5Engine.generate and the scheduler build), and cross_kv still has G rows.
    Returns int64 (G, P + new) on the engine's device: the best hypothesis per chunk, shorter ones filled the way HF does
    (`pad_token_id or eos_token_id[0]`: with pad id 0 that is the FIRST EOS id).
    `use_kernel`: None = mh_beam_step whenever it covers the call (greedy beams, 2 .. 8 of them, K <= 8192: kernel_path_available), False = the torch-op
    bookkeeping below, True = the kernel or an error.
    `kv_fp8`: the packed e4m3 copy of `cross_kv` (engine.cross_kv_fp8(cross_kv)), or True to have it made here: every step streams
    the copy (mh_t5_step_fp8) instead of `cross_kv`.  bf16 storage only.
    `device_draw` (beam-sample only; ignored under greedy beams): the continuations are drawn by the library's rule (Gumbel top-K on
    its counter-based generator, seed sp.seed: module docstring) instead of torch.multinomial -- in the step kernel,
    mh_beam_step_sample (`use_kernel` None / True), or by the same rule in torch ops (`use_kernel` False).  Not with `sample_fn`.
    `cache`: "copy" (the default) reorders the self-attention caches as HF does, row b <- row src[b] after every token
    (mh_t5_reorder_cache).  "indexed" copies nothing: the steps read the cached rows through an index table (mh_t5_step_indexed) and a
    reorder permutes table rows (mh_t5_reorder_index) -- the same logits bit for bit; tgt_len <= 2560.
    `prefill` (with cache="indexed" only): positions 0 .. P-2 of the prompt go through the batched prefill once per chunk
    (mh_t5_step_prefill) instead of one step per column and (chunk, beam) row.  The prefill's MFMA sums are ordered differently from
    the token step's, as in mh_t5_generate: the same cache rows as that entry writes, not bit-identical to the token-by-token feed.
    `self_kv_fp8` (with cache="indexed" and bf16 storage only, else ValueError): the steps attend an e4m3 shadow of the self-attention
    cache, one fp32 scale per cached row, through the same table (mh_t5_step_indexed_skv8); a prefill is followed by
    mh_t5_self_kv_fp8_fill.  The shadow is the engine's workspace "skv8", 0.53 x the bf16 cache on top of it; tgt_len <= 2560, at most
    64 rows.  Not a parity mode: the logits are those of cached K / V rounded to e4m3.  The search itself never sees the cache."""
    check_cache_mode(cache, prefill)
    if self_kv_fp8:
        require_bf16_for_self_kv_fp8(engine.dtype, max(2, int(num_beams)), cache)
    if device_draw and sample_fn is not None:
        raise ValueError("device_draw draws inside the library: it cannot be combined with sample_fn")
    device_draw = bool(device_draw) and bool(sp.do_sample)
    dec = _BeamDecoder(engine, cross_kv, prompt, prompt_mask, eos_ids, sp, num_beams, kv_fp8, cache, prefill, self_kv_fp8)
    if device_draw:
        can_draw = _lib.load().mh_beam_step_path(dec.nb, dec.V, dec.K) != 0
        if use_kernel is True and not can_draw:
            raise NotImplementedError(f"mh_beam_step_sample does not cover this call ({_KERNEL_LIMITS})")
        if can_draw and use_kernel is not False:
            return _beam_search_kernel(dec, sp, length_penalty, early_stopping, sample_keep=dec.min_tokens_to_keep)
    can = kernel_path_available(sp, dec.nb, dec.V, len(dec.eos)) and sample_fn is None
    if use_kernel is True and not can:
        raise NotImplementedError(f"mh_beam_step does not cover this call (beam-sample, an injected sampler, {_KERNEL_LIMITS})")
    if can and use_kernel is not False:
        return _beam_search_kernel(dec, sp, length_penalty, early_stopping)
    return _beam_search_torch_ops(dec, sp, length_penalty, early_stopping, sample_fn, device_draw)


def _beam_search_torch_ops(dec: _BeamDecoder, sp, length_penalty, early_stopping, sample_fn, device_draw: bool) -> torch.Tensor:
    """`beam_search` with HF's bookkeeping restated in torch ops (module docstring, steps b .. g): beam-sample as HF draws it, and the
    cross-check of `_beam_search_kernel`."""
    dev = dec.engine.device
    G, nb, R, V, P, max_length, K, cfg = dec.G, dec.nb, dec.R, dec.V, dec.P, dec.max_length, dec.K, dec.guided
    procs = BeamProcessors(sp, dev, min_tokens_to_keep=dec.min_tokens_to_keep)
    do_sample = bool(sp.do_sample)
    if do_sample and sample_fn is None and not device_draw:
        sample_fn = torch.multinomial
    eos_t = torch.tensor(sorted(set(dec.eos)), dtype=torch.long, device=dev)
    top_mask = torch.zeros(K, dtype=torch.bool, device=dev)
    top_mask[:nb] = True
    running = torch.full((G, nb, max_length), dec.fill, dtype=torch.int64, device=dev)
    running[:, :, :P] = dec.ids0e[-R:].view(G, nb, P)
    sequences = running.clone()
    running_scores = torch.zeros((G, nb), dtype=torch.float32, device=dev)
    running_scores[:, 1:] = -1e9
    beam_scores = torch.full((G, nb), -1e9, dtype=torch.float32, device=dev)
    finished = torch.zeros((G, nb), dtype=torch.bool, device=dev)
    heuristic_open = torch.ones((G, 1), dtype=torch.bool, device=dev)
    running_bidx = torch.full((G, nb, dec.n_new), -1, dtype=torch.int32, device=dev)
    beam_bidx = running_bidx.clone()
    scale = float(sp.cfg_scale)
    with dec.running():
        dec.feed_prompt()
        cur_len = P
        while True:
            flat = running[:, :, :cur_len].reshape(R, cur_len)
            last = flat[:, cur_len - 1]
            if cfg:      # both halves are fed the beam's last token; over the prompt columns the first half has the negative prompt's
                last = torch.cat([last if cur_len > P else dec.ids0e[:R, P - 1], last], 0)
            dec.step(last, cur_len - 1)
            lsm = torch.log_softmax(dec.logits, dim=-1)
            if cfg:      # HF's processor, first in the list: `cond, uncond = scores.split(R); uncond + (cond - uncond) * scale`
                lsm = lsm[R:] + (lsm[:R] - lsm[R:]) * scale
            log_probs = procs(flat, lsm)
            acc = (log_probs.view(G, nb, V) + running_scores[:, :, None]).reshape(G, nb * V)
            if device_draw:   # ... by the rule of mh_beam_step_sample, on acc itself (dead beams order as in the kernel)
                topk_idx = _device_draw(acc, K, int(sp.seed), int(sp.rng_row0), cur_len)
                topk_lp = torch.gather(acc, 1, topk_idx)
            elif do_sample:   # K continuations drawn without replacement, kept in draw order
                topk_idx = sample_fn(torch.softmax(acc, dim=-1), K).to(dev)
                topk_lp = torch.gather(acc, 1, topk_idx)
            else:
                topk_lp, topk_idx = torch.topk(acc, k=K)
            src_beam = topk_idx // V
            topk_bidx = _gather(running_bidx, src_beam)
            topk_seq = _gather(running, src_beam)
            topk_seq[:, :, cur_len] = topk_idx % V
            topk_bidx[:, :, cur_len - P] = (src_beam + torch.arange(G, device=dev).view(-1, 1) * nb).to(torch.int32)
            # d. stopping criteria on the K candidates: EOS id as the new last token, or max_length reached
            hits = torch.isin(topk_seq[:, :, cur_len], eos_t) | (cur_len + 1 >= max_length)
            # e. the running beams of the next step: best num_beams candidates that did not just finish
            run_lp = topk_lp + hits.to(torch.float32) * -1.0e9
            nxt = torch.topk(run_lp, k=nb)[1]
            running, running_scores, running_bidx = _gather(topk_seq, nxt), _gather(run_lp, nxt), _gather(topk_bidx, nxt)
            # f. finished hypotheses: only candidates inside the top num_beams count
            just = hits & top_mask[None, :]
            fin_lp = topk_lp / ((cur_len + 1 - P) ** length_penalty)
            full = torch.all(finished, dim=-1, keepdim=True) & (early_stopping is True)
            fin_lp = fin_lp + full.to(torch.float32) * -1.0e9
            fin_lp = fin_lp + (~heuristic_open).to(torch.float32) * -1.0e9
            fin_lp = fin_lp + (~just) * -1.0e9
            m_seq = torch.cat((sequences, topk_seq), dim=1)
            m_sc = torch.cat((beam_scores, fin_lp), dim=1)
            m_bi = torch.cat((beam_bidx, topk_bidx), dim=1)
            m_fin = torch.cat((finished, just), dim=1)
            sel = torch.topk(m_sc, k=nb)[1]
            sequences, beam_scores, beam_bidx, finished = _gather(m_seq, sel), _gather(m_sc, sel), _gather(m_bi, sel), _gather(m_fin, sel)
            # g. the caches follow the beams that keep running
            src = running_bidx[..., cur_len - P].reshape(R).to(torch.int32).contiguous()
            if cfg:      # `beam_idx.repeat(2)` (cache_utils.py:18): BOTH halves take their rows from the first half
                src = torch.cat([src, src], 0).contiguous()
            dec.reorder(src, cur_len)
            cur_len += 1
            if early_stopping == "never" and length_penalty > 0.0:
                hyp_len = max_length - P
            else:
                hyp_len = cur_len - P
            best_running = running_scores[:, :1] / (hyp_len ** length_penalty)
            worst_fin = torch.where(finished, torch.min(beam_scores, dim=1, keepdim=True)[0], -1.0e9)
            heuristic_open = heuristic_open & torch.any(best_running > worst_fin, dim=-1, keepdim=True)
            go_on = torch.any(heuristic_open) & ~(torch.all(finished) & (early_stopping is True)) & ~torch.all(hits)
            if not bool(go_on):
                break
        out = dec.finish(sequences, beam_bidx)
    return out
