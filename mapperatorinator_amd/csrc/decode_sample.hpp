// The small kernels around a token step: the sampler (HF GenerationMixin._sample's selection with the reference logits processors), the
// init kernels of a call and of an in-flight slot, finalize, and the step-wise embed.  Instantiated in decode_sample.hip and nowhere else
// (the anonymous namespace says so).
#pragma once
#include <type_traits>

#include "decode_device.hpp"
#include "decode_step.hpp"

namespace mh {
namespace {

struct NoRowSetP {};
// ... or those of an in-flight decode (the SLOT instantiation, mh_t5_slots_*): the row settings, and what is the row's own there instead
// of the call's -- pos [S]: the position slot b is fed at this step (negative: the slot is idle), advanced by the row's own workgroup;
// plen [S]: the slot's prompt length.  Both are indexed by the global row.
struct SlotSetP : RowSetP { int32_t* pos; const int32_t* plen; };
struct RowVals {   // one entry as the sampler holds it (scalars: no indexed member, nothing that would live in scratch)
  float temperature, cond_temp0, cond_temp1, cond_temp2, top_p, timeshift_bias, cfg_scale;
  int cond_mask, top_k, lookback_mask_end, max_length, eos_set;
  unsigned rng_row; uint64_t seed;
};

__device__ inline int32_t next_ts_state(const MhSampling& sp, int tok, int32_t cur) {
  // incremental form of MonotonicTimeShiftLogitsProcessor's "last TIME_SHIFT after the last SOS-type
  // token" scan (osuT5/osuT5/inference/logit_processors.py:150-172): the state after `tok`
  if (tok >= sp.ts_start && tok < sp.ts_end) return tok - sp.ts_start;
  for (int i = 0; i < sp.n_sos; ++i)
    if (tok == sp.sos_ids[i]) return -1;
  return cur;
}

// row of decoder.embed_positions for column `col` of global row b (arch 2)
__device__ inline int dec_pos_row(const SampleP& p, int b, int col) {
  const int off = p.pos_off ? p.pos_off[b] : 0;
  return col - off > 0 ? col - off : 0;
}

// input_ids[row][i] as the reference's processors see it: the prompt, then the ids that were FED (the forced ids
// under teacher forcing, the emitted ones otherwise)
__device__ inline int history_id(const SampleP& p, int row, int i) {
  return (p.forced && i >= p.P) ? p.forced[(long)row * p.max_length + i] : p.tokens[(long)row * p.max_length + i];
}

// (the sampler's counter-based RNG, uniform01(seed, row, step), lives in common.hpp: the beam step draws from it too)

// init: consume prompt columns 0..start_pos (processor state machine) and embed the token at start_pos, the first
// position the per-token loop feeds (0 without prefill, P-1 after the batched prompt prefill)
template <typename T>
__global__ __launch_bounds__(256) void dec_init_kernel(SampleP p, int chain_rows, int start_pos) {
  const int lb = blockIdx.x, b = p.b0 + lb;
  if (threadIdx.x == 0) {
    int32_t v = -1;
    for (int i = 0; i <= start_pos; ++i) v = next_ts_state(p.sp, p.tokens[(long)b * p.max_length + i], v);
    p.last_ts_val[b] = v;
    p.finished[b] = 0;
    p.finish_col[b] = p.max_length - 1;
    if (lb == 0) { p.st->pos = start_pos; p.st->n_running = chain_rows; p.st->tail_err = 0; p.st->tail_cnt[0][0] = 0; p.st->tail_cnt[1][0] = 0; p.st->ticket = 0; p.st->rng_row0 = p.sp.rng_row0; p.st->seed = p.sp.seed; }
  }
  __shared__ int s_off;
  if (threadIdx.x == 0) {
    int off = 0;
    if (p.pos_off) {   // transformers 4.57's Whisper decoder_position_ids = cumsum(mask) - 1, clamped at 0: a left-padded row counts from its first real token
      if (p.prompt_mask)
        for (int i = 0; i < p.P; ++i) off += p.prompt_mask[(long)b * p.P + i] == 0;
      p.pos_off[b] = off;
    }
    s_off = off;
  }
  __syncthreads();
  const int tok = p.tokens[(long)b * p.max_length + start_pos];
  const T* e = reinterpret_cast<const T*>(p.dec_embed) + (long)tok * p.d;
  const float* pe = p.dec_pos ? p.dec_pos + (long)(start_pos - s_off > 0 ? start_pos - s_off : 0) * p.d : nullptr;
  for (int i = threadIdx.x; i < p.d; i += 256) p.h[(long)lb * p.d + i] = Elem<T>::to_f32(e[i]) + (pe ? pe[i] : 0.f);
}

// The same for ONE slot of an in-flight decode (mh_t5_slots_admit), row b of the slot buffers: the time-shift state over the prompt
// columns 0 .. start_pos, finished / finish_col, pos_off (the mask row has the stride of `tokens`: ones behind the prompt), the prompt
// length, the embedding of the token at start_pos -- and LAST the position, which is what makes the slot live for the token steps (the
// chain waits for the admission's event before the step that first reads it, so the order inside this kernel is belt and braces).
template <typename T>
__global__ __launch_bounds__(256) void dec_slot_init_kernel(SampleP p, int b, int P, int start_pos, int32_t* slot_pos, int32_t* slot_plen) {
  const int lb = b - p.b0;
  __shared__ int s_off;
  if (threadIdx.x == 0) {
    int32_t v = -1;
    for (int i = 0; i <= start_pos; ++i) v = next_ts_state(p.sp, p.tokens[(long)b * p.max_length + i], v);
    p.last_ts_val[b] = v;
    p.finish_col[b] = p.max_length - 1;
    slot_plen[b] = P;
    int off = 0;
    if (p.pos_off) {
      for (int i = 0; i < P; ++i) off += p.prompt_mask[(long)b * p.max_length + i] == 0;
      p.pos_off[b] = off;
    }
    s_off = off;
  }
  __syncthreads();
  const int tok = p.tokens[(long)b * p.max_length + start_pos];
  const T* e = reinterpret_cast<const T*>(p.dec_embed) + (long)tok * p.d;
  const float* pe = p.dec_pos ? p.dec_pos + (long)(start_pos - s_off > 0 ? start_pos - s_off : 0) * p.d : nullptr;
  for (int i = threadIdx.x; i < p.d; i += 256) p.h[(long)lb * p.d + i] = Elem<T>::to_f32(e[i]) + (pe ? pe[i] : 0.f);
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence();
    p.finished[b] = 0;
    slot_pos[b] = start_pos;
  }
}

// Step bookkeeping without a launch of its own: every workgroup read `pos` when it started, so the one that arrives
// last may advance it; it also recounts the running rows for the host's early-stop poll.  The `finished` flags are
// agent-scope stores drained before the ticket is taken and agent-scope loads here (write-through hand-off, no
// fence); a stale flag could only delay the early stop by a poll, never change a token.
// The recount is ONE round trip of the last workgroup's first wave (lane i reads row i's flag), not chain_rows serial ones.
// SLOT: every row advances its own position (the sampler); the last workgroup only recounts (an idle slot keeps its flag set).
template <bool SLOT>
__device__ __forceinline__ void sample_arrive(const SampleP& p, int pos, int* s_is_last) {
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  if (tid == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int t = __hip_atomic_fetch_add(&p.st->ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *s_is_last = t == (int)gridDim.x - 1;
  }
  __syncthreads();
  if (*s_is_last && wid == 0) {
    int run = 0;
    for (int i0 = 0; i0 < p.chain_rows; i0 += 64) {
      const int i = i0 + lane;
      const bool running = i < p.chain_rows &&
                           __hip_atomic_load(&p.finished[p.b0 + (i < p.chain_rows ? i : 0)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0;
      run += __popcll(__ballot(running));
    }
    if (lane == 0) {
      __hip_atomic_store(&p.st->ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      dec::store_wt(&p.st->n_running, run);
      if (!SLOT) dec::store_wt(&p.st->pos, pos + 1);
    }
  }
}

template <bool SLOT, typename RS> __device__ __forceinline__ int sample_pos(const SampleP& p, const RS& rs, int b) {
  if constexpr (SLOT) return rs.pos[b];
  else return p.st->pos;
}
template <bool SLOT, typename RS> __device__ __forceinline__ int sample_plen(const RS& rs, int b) {
  if constexpr (SLOT) return rs.plen[b];
  else return 0;
}

constexpr int kSampleRegs = 16;   // the register sampling path holds up to 16 ids per thread: vocabularies of <= 4096 ids

// One workgroup per returned row (per CFG pair): processors -> selection -> bookkeeping -> next-token embedding.
// Processor order = server.py:106-134: CFG -> MonotonicTimeShift -> TimeshiftBias -> (Conditional)Temperature ->
// LookbackBias, then HF's own top-k / top-p warpers and the multinomial draw.
// ROWS (mh_t5_generate_rows): temperature, the conditional temperatures and their mask, top-k / top-p, the time-shift bias, the
// lookback end, the length cap, the EOS set, the RNG key and the guidance scale come from rs.rows[returned row] instead of p.sp
// SLOT (mh_t5_slots_*, on top of ROWS): every row is a slot with a window of its own.  The row's own, from rs.pos / rs.plen and the
// buffers indexed by the row: its position and column, its prompt length (the "still inside the prompt" branch under option
// decode_prefill = 0), pos_off (arch 2), the parity of hist_scores, its row of logits_dump [max_length][S][V].  A row that is done (an
// id of its EOS set, or its max_length) writes its finish column, sets its flag and stops: no pad ids afterwards, its position moves no
// further.  An idle slot (negative position) does nothing.  The last-arriving workgroup recounts n_running and advances nothing.  No
// guidance (pair = 0) and cond_per_row = 1: checked on the host.
// PAIR (mh_t5_slots_open_guided, on top of SLOT): every slot is a classifier-free guidance pair, one workgroup per pair (grid = p.pair
// = S): the negative-prompt row s and the prompt row S + s of one window, which share one position, one prompt length and one end.
// The pair's position, length, flag and state are read from the prompt row; the guidance scale is rs.rows[s]'s own.  The emitted id,
// the finished flags, the finish columns and the advanced position go to BOTH rows (the self-attention reads the position by row);
// the next token is embedded for both rows, each with its own pos_off; logits_dump is [max_length][S][V] and the score history is
// per pair.  The last-arriving workgroup recounts over the 2 S flags.
template <typename T, bool ROWS = false, bool SLOT = false, bool PAIR = false>
__global__ __launch_bounds__(256) void dec_sample_kernel(SampleP p, typename std::conditional<SLOT, SlotSetP, typename std::conditional<ROWS, RowSetP, NoRowSetP>::type>::type rs) {
  static_assert(!SLOT || ROWS, "the slot form always reads rs.rows");
  static_assert(!PAIR || SLOT, "the pair form is a slot form");
  __shared__ float sf[8];
  __shared__ int si[8];
  __shared__ float s3[12];
  __shared__ float s_e[256 * kSampleRegs];
  __shared__ int s_is_last;
  __shared__ float s_sum, s_temp;
  __shared__ int s_timed;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const bool cfg = PAIR || p.pair > 0;
  const int nrow = cfg ? 2 : 1;
  const int lneg = blockIdx.x;                 // chain-local row of the negative prompt (CFG only)
  const int lb = cfg ? lneg + p.pair : lneg;   // chain-local returned row (the row whose ids are `input_ids`)
  const int b = p.b0 + lb;                     // its global row
  const int bneg = p.b0 + lneg;
  const int gr = cfg ? lneg : b;               // index among the returned rows
  const int R = cfg ? p.pair : p.B;
  // Requested before anything else, all in ONE round trip: this row's logits (vocabularies of <= 4096 ids sit in registers,
  // thread t holds ids t, t + 256, ...), its finished flag and time-shift state -- none of them depends on the position.
  // (The loop form `for (v = tid; v < V; v += 256) lg[v]` is a chain of V / 256 dependent round trips: the trip count is
  // dynamic, so hipcc neither unrolls it nor hoists the loads.)
  const float* lg = p.logits + (long)lb * p.ldl;
  const float* lgn = p.logits + (long)lneg * p.ldl;
  const bool in_regs = p.V <= 256 * kSampleRegs;
  float raw[kSampleRegs], rawn[kSampleRegs];
  if (in_regs) {
#pragma unroll
    for (int i = 0; i < kSampleRegs; ++i) {
      int v = tid + 256 * i;
      v = v < p.V ? v : p.V - 1;
      raw[i] = lg[v];
      rawn[i] = cfg ? lgn[v] : 0.f;
    }
  }
  // (ROWS: the row's entry, 64 bytes at a workgroup-uniform address, leaves with the same round trip)
  RowVals row{};
  if constexpr (ROWS) {
    const MhRowSampling& r = rs.rows[gr];
    row.temperature = r.temperature; row.cond_temp0 = r.cond_temp[0]; row.cond_temp1 = r.cond_temp[1]; row.cond_temp2 = r.cond_temp[2];
    row.cond_mask = r.cond_mask; row.top_k = r.top_k; row.top_p = r.top_p; row.timeshift_bias = r.timeshift_bias;
    row.lookback_mask_end = r.lookback_mask_end; row.eos_set = r.eos_set; row.rng_row = r.rng_row; row.seed = r.seed;
    row.cfg_scale = r.cfg_scale;
    // the row's own cap, never beyond the stride of `tokens`
    row.max_length = r.max_length < 1 ? 1 : (r.max_length < p.max_length ? r.max_length : p.max_length);
  }
  const bool was_finished = p.finished[b] != 0;
  const int ltv = p.last_ts_val[b];
  const int pos = sample_pos<SLOT>(p, rs, b);   // the position fed this step: the call's, or (SLOT) the row's own
  const int plen = sample_plen<SLOT>(rs, b);
#define MH_PROMPT_LEN (SLOT ? plen : p.P)     // the prompt length: the call's, or (SLOT) the row's own
  const int col = pos + 1;  // column being produced
  const MhSampling& sp = p.sp;
  // a per-row setting where it is used: the row's value, or the very expression the uniform form always had
#define MH_ROWV(f) (ROWS ? row.f : sp.f)
  if constexpr (SLOT) {
    // an idle slot, or a row that is done and waits to be taken: only the step's arrival (workgroup-uniform: one word each)
    if (pos < 0 || was_finished || col >= p.max_length) { sample_arrive<true>(p, pos, &s_is_last); return; }
  } else {
    if (col >= p.max_length) return;
  }
  int nxt[2] = {0, 0};      // the ids the next step is fed (row b, and under guidance its negative-prompt row)

  if (col < MH_PROMPT_LEN) {
    // still inside the prompt: the token is given; only advance the processor state + embedding
    nxt[0] = p.tokens[(long)b * p.max_length + col];
    if (cfg) nxt[1] = p.tokens[(long)bneg * p.max_length + col];
    if (tid == 0) dec::store_wt(&p.last_ts_val[b], next_ts_state(sp, nxt[0], ltv));
    if constexpr (SLOT) { if (tid == 0) dec::store_wt(&rs.pos[b], pos + 1); }
    if constexpr (PAIR) { if (tid == 0) dec::store_wt(&rs.pos[bneg], pos + 1); }
  } else {
    if (tid == 0) {
      // ConditionalTemperatureLogitsWarper: the lookback is ROW 0's history for the whole batch
      // (logit_processors.py:75-80 `input_ids[0, -max_offset:]`), first matching rule wins; cond_per_row: the row's
      // own history (= the reference called with batch 1 per row: sequential songs, shards)
      float temp = MH_ROWV(temperature);
      const int row0 = sp.cond_per_row ? b : (cfg ? p.pair : 0);
      for (int j = 0; j < sp.n_cond; ++j) {
        if constexpr (ROWS) {   // a rule this row does not have (its temperature equals the row's base one) must not match
          if (!((row.cond_mask >> j) & 1)) continue;
        }
        const int off = sp.cond_offset[j];
        if (col >= off && (sp.tok_flags[history_id(p, row0, col - off)] & (2 << j))) { temp = ROWS ? (j == 0 ? row.cond_temp0 : (j == 1 ? row.cond_temp1 : row.cond_temp2)) : sp.cond_temp[j]; break; }
      }
      s_temp = temp;
      // LookbackBiasLogitsWarper types_first: "the scores are for a timeshift event" when the last id is a timed event
      s_timed = (sp.lookback_types_first && col > MH_PROMPT_LEN) ? (sp.tok_flags[history_id(p, b, col - 1)] & 1) : 0;
    }
    __syncthreads();
    const float temp = s_temp;
    const bool lb_range_on = MH_ROWV(lookback_mask_end) > sp.ts_start;
    // CFG -> monotonic -> bias -> temperature
    auto warped_of = [&](int v, float x, float xn) -> float {
      // HF ClassifierFreeGuidanceLogitsProcessor on the reference's row order (first half = negative prompt):
      // uncond + (cond - uncond) * scale with cond = first half, no fused multiply-add
      if (cfg) x = __fadd_rn(x, __fmul_rn(__fsub_rn(xn, x), MH_ROWV(cfg_scale)));
      // MonotonicTimeShiftLogitsProcessor: ids [ts_start, ts_start + value) -> -inf
      if (ltv >= 0 && v >= sp.ts_start && v < sp.ts_start + ltv) x = -INFINITY;
      // TimeshiftBias
      if (MH_ROWV(timeshift_bias) != 0.f && v >= sp.ts_start && v < sp.ts_end) x += MH_ROWV(timeshift_bias);
      // TemperatureLogitsWarper / ConditionalTemperatureLogitsWarper (scores / temperature)
      return x / temp;
    };
    auto warped = [&](int v) -> float { return warped_of(v, lg[v], cfg ? lgn[v] : 0.f); };
    float* dump = p.logits_dump ? p.logits_dump + ((long)col * R + gr) * p.V : nullptr;
    float* fin = p.proc + (long)gr * p.V;
    float best = -INFINITY;
    int besti = 0x7fffffff;
    const bool keep_scores = sp.do_sample != 0;   // only the sampling passes below read the processed scores back
    auto consider = [&](int v, float x) {
      if (keep_scores) fin[v] = x;
      if (dump) dump[v] = x;
      if (x > best) { best = x; besti = v; }   // strided scan keeps the smallest index per thread
    };
    if (sp.lookback_types_first && lb_range_on) {
      // LookbackBiasLogitsWarper, types_first == True (logit_processors.py:116-133).  `last_scores` = what entered
      // this processor at the previous step: two row buffers indexed by the parity of the column.
      float* cur = p.hist_scores + ((long)(col & 1) * R + gr) * p.V;
      const float* last = p.hist_scores + ((long)((col & 1) ^ 1) * R + gr) * p.V;
      const bool renorm = s_timed != 0;
      float mc = -INFINITY, ml = -INFINITY;
      for (int v = tid; v < p.V; v += 256) {
        const float x = warped(v);
        cur[v] = x;
        mc = fmaxf(mc, x);
        if (renorm) ml = fmaxf(ml, last[v]);
      }
      if (!renorm) {
        for (int v = tid; v < p.V; v += 256) consider(v, cur[v]);
      } else {
        mc = block_max(mc, sf);
        ml = block_max(ml, sf);
        float s_cur = 0.f, o_cur = 0.f, s_last = 0.f, e_last = 0.f;
        for (int v = tid; v < p.V; v += 256) {
          const float ec = expf(cur[v] - mc), el = expf(last[v] - ml);
          s_cur += ec;
          if (!(v >= sp.ts_start && v < MH_ROWV(lookback_mask_end))) o_cur += ec;
          s_last += el;
          if (sp.tok_flags[v] & 16) e_last += el;
        }
        s_cur = block_sum(s_cur, sf);
        o_cur = block_sum(o_cur, sf);
        s_last = block_sum(s_last, sf);
        e_last = block_sum(e_last, sf);
        const float prob_eos = e_last / s_last, prob_event = 1.f - prob_eos;
        const float sc = 1.f / ((o_cur / s_cur) * prob_event + prob_eos);
        const float extra = fminf(fmaxf((sc - 1.f) * prob_eos / prob_event, 0.f), 1.f);
        const float log_norm = logf(s_cur) - logf(sc);
        for (int v = tid; v < p.V; v += 256) {
          float x;
          if (v >= sp.ts_start && v < MH_ROWV(lookback_mask_end)) x = (v == sp.ts_start) ? logf(extra) : -INFINITY;
          else x = (cur[v] - mc) - log_norm;   // log(softmax(cur)[v] * sc), kept in the log domain (no underflow)
          consider(v, x);
        }
      }
    } else if (in_regs) {
#pragma unroll
      for (int i = 0; i < kSampleRegs; ++i) {
        const int v = tid + 256 * i;
        if (v < p.V) {
          float x = warped_of(v, raw[i], rawn[i]);
          // LookbackBiasLogitsWarper, types_first == False branch
          if (lb_range_on && v >= sp.ts_start && v < MH_ROWV(lookback_mask_end)) x = -INFINITY;
          consider(v, x);
        }
      }
    } else {
      for (int v = tid; v < p.V; v += 256) {
        float x = warped(v);
        if (lb_range_on && v >= sp.ts_start && v < MH_ROWV(lookback_mask_end)) x = -INFINITY;
        consider(v, x);
      }
    }
    // argmax with first-index tie-break (torch.argmax semantics on ties = first maximal index)
    // (lane exchanges on the VALU, common.hpp; the whole workgroup is here)
#define MH_ARGMAX_LEVEL(O)                                                        \
    {                                                                             \
      const float ob = lane_xor<O>(best);                                         \
      const int oi = lane_xor<O>(besti);                                          \
      if (ob > best || (ob == best && oi < besti)) { best = ob; besti = oi; }     \
    }
    MH_ARGMAX_LEVEL(32) MH_ARGMAX_LEVEL(16) MH_ARGMAX_LEVEL(8) MH_ARGMAX_LEVEL(4) MH_ARGMAX_LEVEL(2) MH_ARGMAX_LEVEL(1)
#undef MH_ARGMAX_LEVEL
    __syncthreads();   // the reductions above may still be reading sf
    if (lane == 0) { sf[wid] = best; si[wid] = besti; }
    __syncthreads();
    if (tid == 0) {
      for (int w2 = 1; w2 < 4; ++w2)
        if (sf[w2] > best || (sf[w2] == best && si[w2] < besti)) { best = sf[w2]; besti = si[w2]; }
      sf[4] = best; si[4] = besti;
    }
    __syncthreads();
    int tok = si[4];
    if (sp.do_sample && p.V <= 256 * kSampleRegs) {
      // softmax sampling with optional top-k / top-p truncation, the processed scores of this row in REGISTERS (thread t
      // holds ids t, t + 256, ...): both thresholds by 4-ary search (three candidate thresholds per block reduction),
      // the draw by a block-wide prefix sum in id order.  The reference's default user settings sample (top_p 0.9,
      // configs/inference/v32.yaml:12-13): the memory-bound bisection + serial scan below cost 350 us per token step.
      const float mx = sf[4];
      __syncthreads();   // sf / s3 are reduction scratch below
      float xr[kSampleRegs];
#pragma unroll
      for (int i = 0; i < kSampleRegs; ++i) {
        const int v = tid + 256 * i;
        xr[i] = v < p.V ? fin[v] - mx : -INFINITY;     // this thread's own stores (consider)
      }
      auto reduce3 = [&](float a, float b, float c, float (&out)[3]) {
        a = wave_sum(a); b = wave_sum(b); c = wave_sum(c);
        __syncthreads();
        if (lane == 0) { s3[wid * 3] = a; s3[wid * 3 + 1] = b; s3[wid * 3 + 2] = c; }
        __syncthreads();
        out[0] = s3[0] + s3[3] + s3[6] + s3[9];
        out[1] = s3[1] + s3[4] + s3[7] + s3[10];
        out[2] = s3[2] + s3[5] + s3[8] + s3[11];
      };
      float thr = -INFINITY;
      if (MH_ROWV(top_k) > 0 && MH_ROWV(top_k) < p.V) {   // largest threshold (to 80 / 4^14) that still keeps >= top_k ids
        float lo = -80.f, hi = 0.f;
        for (int it = 0; it < 14; ++it) {
          const float q = 0.25f * (hi - lo), t1 = lo + q, t2 = lo + 2.f * q, t3 = lo + 3.f * q;
          float c1 = 0.f, c2 = 0.f, c3 = 0.f;
#pragma unroll
          for (int i = 0; i < kSampleRegs; ++i) { c1 += xr[i] >= t1 ? 1.f : 0.f; c2 += xr[i] >= t2 ? 1.f : 0.f; c3 += xr[i] >= t3 ? 1.f : 0.f; }
          float r[3];
          reduce3(c1, c2, c3, r);
          const float k = (float)MH_ROWV(top_k);
          if (r[2] >= k) lo = t3; else if (r[1] >= k) { lo = t2; hi = t3; } else if (r[0] >= k) { lo = t1; hi = t2; } else hi = t1;
        }
        thr = lo;
      }
      float er[kSampleRegs];
      float part = 0.f;
#pragma unroll
      for (int i = 0; i < kSampleRegs; ++i) { er[i] = xr[i] >= thr ? __expf(xr[i]) : 0.f; part += er[i]; }
      const float total = block_sum(part, sf);
      if (MH_ROWV(top_p) < 1.0f) {   // largest probability threshold whose kept mass still reaches top_p
        float lo = 0.f, hi = 1.f;
        const float inv = 1.0f / total;
        for (int it = 0; it < 12; ++it) {
          const float q = 0.25f * (hi - lo), t1 = lo + q, t2 = lo + 2.f * q, t3 = lo + 3.f * q;
          float m1 = 0.f, m2 = 0.f, m3 = 0.f;
#pragma unroll
          for (int i = 0; i < kSampleRegs; ++i) {
            const float pr = er[i] * inv;
            m1 += pr >= t1 ? pr : 0.f; m2 += pr >= t2 ? pr : 0.f; m3 += pr >= t3 ? pr : 0.f;
          }
          float r[3];
          reduce3(m1, m2, m3, r);
          if (r[2] >= MH_ROWV(top_p)) lo = t3; else if (r[1] >= MH_ROWV(top_p)) { lo = t2; hi = t3; } else if (r[0] >= MH_ROWV(top_p)) { lo = t1; hi = t2; } else hi = t1;
        }
#pragma unroll
        for (int i = 0; i < kSampleRegs; ++i) er[i] = (er[i] * inv >= lo) ? er[i] : 0.f;
      }
      // kept weights in id order -> contiguous ownership (thread t: ids [t C, t C + C)) -> inclusive prefix -> first id
      // whose running sum reaches u (else the last kept id), as a sequential scan in id order would pick
#pragma unroll
      for (int i = 0; i < kSampleRegs; ++i) {
        const int v = tid + 256 * i;
        if (v < p.V) s_e[v] = er[i];
      }
      if (tid == 0) { si[5] = 0x7fffffff; si[6] = -1; }
      __syncthreads();
      const int Cn = (p.V + 255) / 256;
      float loc[kSampleRegs];
      float run = 0.f;
#pragma unroll
      for (int i = 0; i < kSampleRegs; ++i) {
        const int v = tid * Cn + i;
        const float e = (i < Cn && v < p.V) ? s_e[v] : 0.f;
        run += e;
        loc[i] = run;
      }
      float incl = run;                       // inclusive scan of the thread totals over the block
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const float up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
      }
      if (lane == 63) sf[wid] = incl;
      __syncthreads();
      float base = incl - run;
      for (int w2 = 0; w2 < wid; ++w2) base += sf[w2];
      const float mass = sf[0] + sf[1] + sf[2] + sf[3];
      const float u = uniform01(ROWS ? row.seed : p.st->seed, ROWS ? row.rng_row : (uint32_t)gr + p.st->rng_row0, (uint32_t)col) * mass;
      int first = 0x7fffffff, last = -1;
      float prev = 0.f;
#pragma unroll
      for (int i = 0; i < kSampleRegs; ++i) {
        const int v = tid * Cn + i;
        const bool kept = i < Cn && v < p.V && loc[i] > prev;     // a kept id carries positive weight
        if (kept) { last = v; if (base + loc[i] >= u && first == 0x7fffffff) first = v; }
        prev = loc[i];
      }
      if (first != 0x7fffffff) atomicMin(&si[5], first);
      if (last >= 0) atomicMax(&si[6], last);
      __syncthreads();
      tok = si[5] != 0x7fffffff ? si[5] : (si[6] >= 0 ? si[6] : tok);
    } else if (sp.do_sample) {
      // (vocabularies beyond 256 * kSampleRegs ids: the same search through memory)
      const float mx = sf[4];
      __syncthreads();   // sf[4] is reused as reduction scratch below
      float thr = -INFINITY;
      if (MH_ROWV(top_k) > 0 && MH_ROWV(top_k) < p.V) {
        float lo = -80.f, hi = 0.f;  // on x - mx
        for (int it = 0; it < 40; ++it) {
          const float mid = 0.5f * (lo + hi);
          int cnt = 0;
          for (int v = tid; v < p.V; v += 256) cnt += (fin[v] - mx >= mid) ? 1 : 0;
          cnt = (int)block_sum((float)cnt, sf);
          if (cnt >= MH_ROWV(top_k)) lo = mid; else hi = mid;
        }
        thr = lo;
      }
      // probabilities of the kept set
      float part = 0.f;
      for (int v = tid; v < p.V; v += 256) {
        const float x = fin[v];
        if (x - mx >= thr) part += __expf(x - mx);
      }
      float total = block_sum(part, sf);
      float pthr = 0.f;
      if (MH_ROWV(top_p) < 1.0f) {
        // keep the smallest set of most-probable ids whose mass reaches top_p
        float lo = 0.f, hi = 1.f;
        for (int it = 0; it < 30; ++it) {
          const float mid = 0.5f * (lo + hi);
          float mass = 0.f;
          for (int v = tid; v < p.V; v += 256) {
            const float x = fin[v];
            if (x - mx >= thr) {
              const float pr = __expf(x - mx) / total;
              if (pr >= mid) mass += pr;
            }
          }
          mass = block_sum(mass, sf);
          if (mass >= MH_ROWV(top_p)) lo = mid; else hi = mid;
        }
        pthr = lo;
        float part2 = 0.f;
        for (int v = tid; v < p.V; v += 256) {
          const float x = fin[v];
          if (x - mx >= thr && __expf(x - mx) / total >= pthr) part2 += __expf(x - mx);
        }
        const float t2 = block_sum(part2, sf);
        if (tid == 0) s_sum = t2;
        __syncthreads();
      } else {
        if (tid == 0) s_sum = total;
        __syncthreads();
      }
      if (tid == 0) {
        const float u = uniform01(ROWS ? row.seed : p.st->seed, ROWS ? row.rng_row : (uint32_t)gr + p.st->rng_row0, (uint32_t)col) * s_sum;
        float cum = 0.f;
        int pick = tok;
        for (int v = 0; v < p.V; ++v) {
          const float x = fin[v];
          if (x - mx >= thr) {
            const float e = __expf(x - mx);
            if (MH_ROWV(top_p) < 1.0f && e / total < pthr) continue;
            cum += e;
            pick = v;
            if (cum >= u) break;
          }
        }
        si[5] = pick;
      }
      __syncthreads();
      tok = si[5];
    }
    // every thread knows the emitted id (the finished flag came with the first round trip), so the embedding row below is
    // requested at once -- beside thread 0's EOS lookup and bookkeeping stores, not behind them
    const bool forced = p.forced != nullptr;
    const int emit = was_finished ? sp.pad_id : tok;      // HF: finished rows receive pad_token_id
    nxt[0] = forced ? p.forced[(long)b * p.max_length + col] : emit;
    if (cfg) nxt[1] = forced ? p.forced[(long)bneg * p.max_length + col] : emit;
    if (tid == 0) {
      const uint8_t* eos = p.eos_table;
      if constexpr (ROWS) {   // the row's set, clamped into the tables the call was given
        const int set = row.eos_set < 0 ? 0 : (row.eos_set < rs.n_eos_sets ? row.eos_set : rs.n_eos_sets - 1);
        eos = rs.eos_tables + (long)set * p.V;
      }
      const bool done = !forced && !was_finished && (eos[emit] || col + 1 >= MH_ROWV(max_length));
      for (int j = 0; j < nrow; ++j) {   // the rows of a CFG pair receive the same id (decoder_input_ids.repeat)
        const int brow = j == 0 ? b : bneg;   // (not `row`: that is the row's settings, which MH_ROWV reads)
        dec::store_wt(p.tokens + (long)brow * p.max_length + col, (int32_t)emit);
        if (done) {
          __hip_atomic_store(&p.finished[brow], (uint8_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // read by the last-arriving workgroup below
          dec::store_wt(p.finish_col + brow, (int32_t)col);
        }
      }
      dec::store_wt(&p.last_ts_val[b], next_ts_state(sp, nxt[0], ltv));
      if constexpr (SLOT) { if (!done) dec::store_wt(&rs.pos[b], pos + 1); }   // (a row that is done stays where it ended)
      if constexpr (PAIR) { if (!done) dec::store_wt(&rs.pos[bneg], pos + 1); }   // (both rows of a pair: equal positions always)
    }
  }
  // embedding of the token that the next step consumes (decoder_embedder, modeling_mapperatorinator.py:205-206)
  for (int j = 0; j < nrow; ++j) {
    const int lrow = j == 0 ? lb : lneg;
    const T* e = reinterpret_cast<const T*>(p.dec_embed) + (long)nxt[j] * p.d;
    const float* pe = p.dec_pos ? p.dec_pos + (long)dec_pos_row(p, j == 0 ? b : bneg, col) * p.d : nullptr;   // (arch 2: + embed_positions[col])
    for (int i = tid * 4; i < p.d; i += 1024) {   // 16-byte write-through pieces (d is a multiple of 4)
      float v4[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) v4[k] = Elem<T>::to_f32(e[i + k]) + (pe ? pe[i + k] : 0.f);
      dec::store_piece_wt<float>(p.h + (long)lrow * p.d + i, v4, 4, 4);
    }
  }
  sample_arrive<SLOT>(p, pos, &s_is_last);
}

#undef MH_ROWV
#undef MH_PROMPT_LEN

__global__ void dec_finalize_kernel(const int32_t* finish_col, int B, int32_t* n_steps_out) {
  if (threadIdx.x == 0) {
    int mx = 0;
    for (int b = 0; b < B; ++b) mx = finish_col[b] > mx ? finish_col[b] : mx;
    *n_steps_out = mx + 1;
  }
}

// ---- step-wise decode (beam search) ----------------------------------------------------------------------------------
// h[b][:] = dec_embed[ids[b]] and the position word of the step
template <typename T>
__global__ __launch_bounds__(256) void step_embed_kernel(const int32_t* ids, const T* emb, int d, float* h, DecState* st, int pos,
                                                        const float* dec_pos, const uint8_t* prompt_mask, int P) {
  // dec_pos (arch 2): + decoder.embed_positions[position]; prompt_mask != NULL here means dec_pos_from_mask: the position is the
  // column minus this row's masked prompt columns
  const int b = blockIdx.x;
  if (b == 0 && threadIdx.x == 0) { st->pos = pos; st->n_running = 0; st->ticket = 0; }
  __shared__ int s_off;
  if (threadIdx.x == 0) {
    int off = 0;
    if (dec_pos && prompt_mask)
      for (int i = 0; i < P; ++i) off += prompt_mask[(long)b * P + i] == 0;
    s_off = off;
  }
  __syncthreads();
  const T* e = emb + (long)ids[b] * d;
  const float* pe = dec_pos ? dec_pos + (long)(pos - s_off > 0 ? pos - s_off : 0) * d : nullptr;
  for (int i = threadIdx.x; i < d; i += 256) h[(long)b * d + i] = Elem<T>::to_f32(e[i]) + (pe ? pe[i] : 0.f);
}

}  // namespace
}  // namespace mh
