// osuT5 on MI355X: the token step of the KV-cached AR decode.  The ONE unit that instantiates the decode kernels
// (decode_kernels.hpp), the sampler / init kernels and the e4m3 K/V quantisers.  It holds every launcher of them,
// enqueue_step() -- one step of one chain, what a step graph captures -- the decode workspace layout and the measurement
// hooks that live inside the step.  The other units reach it through decode_step.hpp: the batched passes are t5_encode.hip,
// the generation loop and the slot session t5_generate.hip, the step-wise entries of beam search t5_stepwise.hip.
//
// Reference semantics reproduced (see include/mapperhip.h for the per-entry citations):
//   HF T5Block / T5Attention / T5LayerFF and the Whisper family's decoder layers, one position at a time;
//   HF GenerationMixin._sample's selection with the reference logits processors (dec_sample_kernel).
#include <stdlib.h>
#include <string.h>

#include <atomic>

#include "decode_kernels.hpp"
#include "decode_step.hpp"

using namespace mh;

// ------------------------------------------------------------------------------------------------
// decode
// ------------------------------------------------------------------------------------------------
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
template <typename T, bool ROWS = false, bool SLOT = false>
__global__ __launch_bounds__(256) void dec_sample_kernel(SampleP p, typename std::conditional<SLOT, SlotSetP, typename std::conditional<ROWS, RowSetP, NoRowSetP>::type>::type rs) {
  static_assert(!SLOT || ROWS, "the slot form always reads rs.rows");
  __shared__ float sf[8];
  __shared__ int si[8];
  __shared__ float s3[12];
  __shared__ float s_e[256 * kSampleRegs];
  __shared__ int s_is_last;
  __shared__ float s_sum, s_temp;
  __shared__ int s_timed;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const bool cfg = p.pair > 0;
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

// real columns per 16-column tile of a decode GEMV: 16 when that still yields >= 192 workgroups, else 8 down to 96
// workgroups, else 4 (every workgroup re-reads ALL activations through L2, the resource the two decode chains fight
// over: at N = 768, 96 workgroups of 8 columns measured 42.9 k tok/s against 42.4 k for 192 of 4 and 42.1 k for 48 of
// 16).  Option decode_gemv_cols overrides; a result never depends on it: every column is an independent dot product.
int gemv_cols(int N) {
  const long o = option(OPT_DECODE_GEMV_COLS);
  if (o == 4 || o == 8 || o == 16) return (int)o;
  if (N / 16 >= 192) return 16;
  if (N / 8 >= 96) return 8;
  return 4;
}

template <typename T, int MF, int PRO, int EPI, bool BIAS = false>
int launch_skinny(dec::SkinnyP p, hipStream_t s) {
  const int kb = 4 * (16 / (int)sizeof(T));
  MH_REQUIRE(p.K % kb == 0 && p.K >= kb, "decode: K=%d must be a positive multiple of %d", p.K, kb);
  const int nkb = p.K / kb;
  MH_REQUIRE(PRO != dec::PRO_PLAIN || nkb % 2 == 0, "decode: K=%d must be a multiple of %d", p.K, 2 * kb);
  // waves per workgroup: a function of K ONLY (batch invariance of the summation order)
  const bool wide = nkb > 4 * dec::kGemvCH;
  MH_REQUIRE(PRO == dec::PRO_PLAIN || nkb <= 8 * dec::kGemvCH, "decode: the norm prologue needs K <= %d", 8 * dec::kGemvCH * kb);
  MH_REQUIRE(PRO != dec::PRO_LAYERNORM || p.ln_b, "decode: LayerNorm prologue without its bias");
  MH_REQUIRE(p.lda == p.K && p.ldw == p.K, "decode: the GEMV operands must be dense (lda = ldw = K)");
  MH_REQUIRE(EPI != dec::SK_RESID || (p.N % 4 == 0 && p.ldh == p.N), "decode: residual GEMV needs a dense [B, N] residual stream, N a multiple of 4");
  int tiles;
  if (EPI == dec::SK_GEGLU) { p.nv = 8; tiles = ceil_div(p.N / 2, 8); }
  else { p.nv = gemv_cols(p.N); tiles = ceil_div(p.N, p.nv); }
  if (wide) {
    if constexpr (PRO != dec::PRO_PLAIN && sizeof(T) == 2) {   // d_model > 1024 in bf16: not a shape of this model family
      set_error("decode: RMSNorm GEMV needs d_model <= 1024 in bf16 storage");
      return MH_ERR_ARG;
    } else {
      hipLaunchKernelGGL((dec::gemv_kernel<T, MF, 8, PRO, EPI, BIAS>), dim3(tiles), dim3(512), 0, s, MH_GEMV_LEAD_ARGS(p), p);
    }
  } else {
    hipLaunchKernelGGL((dec::gemv_kernel<T, MF, 4, PRO, EPI, BIAS>), dim3(tiles), dim3(256), 0, s, MH_GEMV_LEAD_ARGS(p), p);
  }
  return check_launch("gemv_kernel");
}

template <typename T, int PRO, int EPI, bool BIAS = false>
int skinny(const dec::SkinnyP& p, hipStream_t s) {
  MH_REQUIRE(!BIAS || p.bias, "decode: biased GEMV without a bias");
  if (p.B <= 16) return launch_skinny<T, 1, PRO, EPI, BIAS>(p, s);
  if (p.B <= 32) return launch_skinny<T, 2, PRO, EPI, BIAS>(p, s);
  return launch_skinny<T, 4, PRO, EPI, BIAS>(p, s);
}
// residual GEMV with an optional bias (the Whisper family's Wo / fc2)
template <typename T>
int skinny_resid(const dec::SkinnyP& p, hipStream_t s) {
  return p.bias ? skinny<T, dec::PRO_PLAIN, dec::SK_RESID, true>(p, s) : skinny<T, dec::PRO_PLAIN, dec::SK_RESID>(p, s);
}

// ---- the three-GEMV tail of a layer as one launch (option decode_fused_tail; dec::dec_tail_kernel) ---------------------
std::atomic<long> g_tail_launches{0};   // dec_tail_kernel nodes enqueued (captured or launched) by this process: mh_t5_decode_tail_launches
template <typename T> int gemv_waves(int K) { return K / (4 * (16 / (int)sizeof(T))) > 4 * dec::kGemvCH ? 8 : 4; }   // launch_skinny's rule

// The wave combination (O, wi, wo) the fused kernel is instantiated for at these dims: 1 = (4, 4, 4), 2 = (4, 4, 8), 3 = (8, 8, 8)
// (fp32 only), 0 = none.  The ONE table tail_covers() and launch_tail_mf() both read.
template <typename T>
int tail_wave_combo(int inner, int d, int dff) {
  const int a = gemv_waves<T>(inner), b = gemv_waves<T>(d), w = gemv_waves<T>(dff);
  if (a == 4 && b == 4) return w == 4 ? 1 : 2;
  if (sizeof(T) == 4 && a == 8 && b == 8 && w == 8) return 3;
  return 0;
}

// The configurations the fused kernel covers; everything else runs the three launches:
//   chains of <= 16 rows, in fp32 storage <= 32 rows (the bf16 kernel for two row fragments, MF = 2, needs more than 256
//   VGPRs and would spill); a wave combination of the table above -- every T5 / Whisper preset in both storage types; the
//   Whisper family with all of its tail biases present; operand shapes launch_skinny accepts.
template <typename T>
bool tail_covers(const MhT5Config* c, int B, bool wh, const float* b_o, const float* b_fc1, const float* b_fc2) {
  const int kb = 4 * (16 / (int)sizeof(T)), d = c->d_model, inner = c->n_heads * 64, dff = c->d_ff;
  if (B > (sizeof(T) == 2 ? 16 : 32)) return false;
  if (inner % (2 * kb) || dff % (2 * kb) || d % kb || d % 4 || d / kb > 8 * dec::kGemvCH) return false;
  if (wh ? !(b_o && b_fc1 && b_fc2) : (b_o || b_fc1 || b_fc2)) return false;
  return tail_wave_combo<T>(inner, d, dff) != 0;
}

template <typename T, int MF, int PROWI, int EPIWI, bool BIAS>
int launch_tail_mf(const dec::TailP& p, hipStream_t s) {
  const int combo = tail_wave_combo<T>(p.o.K, p.wi.K, p.wo.K);
  if constexpr (sizeof(T) == 2 && MF != 1) {
    set_error("decode: the fused layer tail has no bf16 kernel for chains of more than 16 rows");
    return MH_ERR_ARG;
  } else {
    if (combo == 1) hipLaunchKernelGGL((dec::dec_tail_kernel<T, MF, 4, 4, 4, PROWI, EPIWI, BIAS>), dim3(p.G), dim3(512), 0, s, p);
    else if (combo == 2) hipLaunchKernelGGL((dec::dec_tail_kernel<T, MF, 4, 4, 8, PROWI, EPIWI, BIAS>), dim3(p.G), dim3(512), 0, s, p);
    else if (combo == 3 && sizeof(T) == 4) {
      if constexpr (sizeof(T) == 4) hipLaunchKernelGGL((dec::dec_tail_kernel<T, MF, 8, 8, 8, PROWI, EPIWI, BIAS>), dim3(p.G), dim3(512), 0, s, p);
    } else {
      set_error("decode: no fused layer tail for K = (%d, %d, %d) (tail_covers() should have said so)", p.o.K, p.wi.K, p.wo.K);
      return MH_ERR_ARG;
    }
    g_tail_launches.fetch_add(1, std::memory_order_relaxed);
    return check_launch("dec_tail_kernel");
  }
}

// o / wi / wo: the SkinnyP descriptions of the three launches this one replaces; n_chains: chains that may run side by side
template <typename T, int PROWI, int EPIWI, bool BIAS>
int launch_tail(dec::TailP p, DecState* st, int layer, int n_chains, hipStream_t s) {
  p.o.nv = gemv_cols(p.o.N); p.wo.nv = gemv_cols(p.wo.N);
  p.wi.nv = EPIWI == dec::SK_GEGLU ? 8 : gemv_cols(p.wi.N);
  const int go = 8 / gemv_waves<T>(p.o.K), gi = 8 / gemv_waves<T>(p.wi.K), gw = 8 / gemv_waves<T>(p.wo.K);
  const int to = ceil_div(p.o.N, p.o.nv), tw = ceil_div(p.wo.N, p.wo.nv);
  const int ti = EPIWI == dec::SK_GEGLU ? ceil_div(p.wi.N / 2, 8) : ceil_div(p.wi.N, p.wi.nv);
  int G = std::max(std::max(ceil_div(to, go), ceil_div(ti, gi)), ceil_div(tw, gw));
  const int cap = std::max(1, std::min(128, 256 / std::max(1, n_chains)));   // all chains' tails together: <= 256 workgroups
  p.G = std::min(G, cap);
  p.cnt = &st->tail_cnt[layer & 1][0];
  p.err = &st->tail_err;
  const int khz = mh_wall_clock_khz();
  p.timeout_ticks = 2LL * (khz > 0 ? khz : 100000);   // 2 ms
  if (p.o.B <= 16) return launch_tail_mf<T, 1, PROWI, EPIWI, BIAS>(p, s);
  return launch_tail_mf<T, 2, PROWI, EPIWI, BIAS>(p, s);
}

}  // namespace
DecodeLayout decode_layout(const MhT5Config* c, int B, void* base) {
  const int64_t es = es_of(c->dtype), inner = (int64_t)c->n_heads * 64, V = c->vocab_out;
  const int64_t cache = (int64_t)c->n_dec_layers * B * inner * c->tgt_len * es;
  Arena ar(base, INT64_MAX);
  DecodeLayout ly{};
  ly.bf.h = (float*)ar.take((int64_t)B * c->d_model * 4);
  ly.bf.attn = ar.take(B * inner * es);
  ly.bf.ff = ar.take((int64_t)B * c->d_ff * es);
  ly.bf.logits = (float*)ar.take(B * V * 4);
  ly.bf.self_k = ar.take(cache);
  ly.bf.self_v = ar.take(cache);
  ly.bf.finished = (uint8_t*)ar.take(B);
  ly.bf.finish_col = (int32_t*)ar.take((int64_t)B * 4);
  ly.bf.last_ts = (int32_t*)ar.take((int64_t)B * 4);
  ly.pos_off = (int32_t*)ar.take((int64_t)B * 4);
  ly.bf.st = (DecState*)ar.take((int64_t)align256(sizeof(DecState)) * kMaxChains);
  ly.proc = (float*)ar.take(B * V * 4);                 // processed scores
  ly.hist_scores = (float*)ar.take(B * V * 4 * 2);      // LookbackBias history
  ly.end = ar.off;
  return ly;
}
namespace {

// attention kernels that project their own q (/ k / v): see decode_kernels.hpp.  d_model = 128 KC, KC in 1..8
// (check_decode_shape).
#define MH_SELF_LEAD_ARGS hp.h, hp.ln_w, hp.W, sa.pos, sa.kc, sa.vc, sa.H, hp.d
#define MH_CROSS_LEAD_ARGS hp.h, hp.ln_w, hp.W, ca.k, ca.v, ca.H, ca.L, hp.d, ca.kv_B
// f8 != NULL: the F8 instantiation over this layer's rows of the e4m3 shadow cache (bf16 storage only)
// origin != NULL: the IDX instantiation, cached rows read through the beam search's index table (mh_t5_step_indexed); with f8 as well,
// the F8 + IDX one: the shadow rows and their scales through the same table (mh_t5_step_indexed_skv8)
template <typename T, int KC>
int launch_self_qkv(const dec::SelfAttnP& sa, const dec::HeadProjP& hp, int inner, hipStream_t s, const dec::SelfKv8P* f8,
                    const uint8_t* origin = nullptr, const int32_t* slot_pos = nullptr) {
  MH_REQUIRE(hp.ldh == hp.d && hp.ldw == hp.d && inner == sa.H * 64, "decode: dense residual rows / projection weights expected");
  // dec_self_attn_qkv_kernel<.., F8, IDX> over its cache block, in the model's form (dispatch_attn_form)
  auto qkv = [&](auto f8c, auto idx, const auto& cache) {
    dispatch_attn_form(sa.rope, hp.ln_b, [&](auto wh, auto ln) {
      hipLaunchKernelGGL((dec::dec_self_attn_qkv_kernel<T, KC, decltype(wh)::value, decltype(ln)::value, decltype(f8c)::value, decltype(idx)::value>),
                         dim3(sa.B * sa.H), dim3(1024), 0, s, MH_SELF_LEAD_ARGS, sa, hp, cache);
    });
  };
  if (slot_pos) {   // slot_pos != NULL: the SLOT instantiation, every row at its own position (mh_t5_slots_*); with f8 as well, the
                    // F8 + SLOT one: every row over its own shadow row (mh_t5_slots_open_kv8)
    MH_REQUIRE(!origin, "decode: the slot form of the self-attention has no indexed cache");
    auto slot = [&](auto f8c, const auto& cache) {
      dispatch_attn_form(sa.rope, hp.ln_b, [&](auto wh, auto ln) {
        hipLaunchKernelGGL((dec::dec_slot_self_attn_kernel<T, KC, decltype(wh)::value, decltype(ln)::value, decltype(f8c)::value>),
                           dim3(sa.B * sa.H), dim3(1024), 0, s, MH_SELF_LEAD_ARGS, sa, hp, cache);
      });
    };
    if (!f8) {
      slot(std::false_type{}, dec::SelfSlotP{slot_pos});
    } else if constexpr (sizeof(T) == 2) {
      dec::SelfKv8SlotP sl8{};
      sl8.k8 = f8->k8; sl8.v8 = f8->v8; sl8.ks = f8->ks; sl8.vs = f8->vs; sl8.slot_pos = slot_pos;
      slot(std::true_type{}, sl8);
    } else { set_error("decode: the e4m3 self-attention cache needs bf16 storage"); return MH_ERR_ARG; }
  } else if (origin) {   // with f8 as well: the shadow rows and their scales through the table (mh_t5_step_indexed_skv8)
    MH_REQUIRE(sa.tgt_len <= dec::kSelfIdxMaxTgt, "decode: the indexed self-attention stages at most %d table entries (tgt_len %d)",
               dec::kSelfIdxMaxTgt, sa.tgt_len);
    if (!f8) {
      qkv(std::false_type{}, std::true_type{}, dec::SelfIdxP{origin});
    } else if constexpr (sizeof(T) == 2) {
      dec::SelfKv8IdxP ix8{};
      ix8.k8 = f8->k8; ix8.v8 = f8->v8; ix8.ks = f8->ks; ix8.vs = f8->vs; ix8.origin = origin;
      qkv(std::true_type{}, std::true_type{}, ix8);
    } else { set_error("decode: the e4m3 self-attention cache needs bf16 storage"); return MH_ERR_ARG; }
  } else if (f8) {
    if constexpr (sizeof(T) == 2) qkv(std::true_type{}, std::false_type{}, *f8);
    else { set_error("decode: the e4m3 self-attention cache needs bf16 storage"); return MH_ERR_ARG; }
  } else {
    qkv(std::false_type{}, std::false_type{}, dec::NoSelfKv8P{});
  }
  return check_launch("dec_self_attn_qkv_kernel");
}
template <typename T, int KC>
int launch_cross_q(const dec::CrossAttnP& ca, const dec::HeadProjP& hp, hipStream_t s) {
  MH_REQUIRE(hp.ldh == hp.d && hp.ldw == hp.d, "decode: dense residual rows / projection weights expected");
  // one key in flight per 8-lane group: 64 VGPRs without spills (two 16-wave workgroups per CU); U = 2 measured the
  // same bandwidth.  The Whisper family: biased Wq, scaled scores (over the e4m3 copy the scale folds into the key scale)
  auto cross = [&](auto f8c) {
    dispatch_attn_form(ca.scale != 0.f, hp.ln_b, [&](auto wh, auto ln) {
      hipLaunchKernelGGL((dec::dec_cross_attn_q_kernel<T, KC, 1, decltype(f8c)::value, decltype(wh)::value, decltype(ln)::value>),
                         dim3(ca.B * ca.H), dim3(1024), 0, s, MH_CROSS_LEAD_ARGS, ca, hp);
    });
  };
  if (ca.kscale != nullptr) {   // the e4m3 copy of the cross K/V
    if constexpr (sizeof(T) == 2) cross(std::true_type{});
    else { set_error("decode: the fp8 cross K/V copy needs bf16 storage"); return MH_ERR_ARG; }
  } else {
    cross(std::false_type{});
  }
  return check_launch("dec_cross_attn_q_kernel");
}
template <typename T>
int launch_cross_q_d(const dec::CrossAttnP& ca, const dec::HeadProjP& hp, hipStream_t s) {
  return dispatch_kc(hp.d, [&](auto kc) { return launch_cross_q<T, decltype(kc)::value>(ca, hp, s); });
}

// measurement hook (mh_t5_decode_timing): device buffer that receives per-launch timestamps of the dominant kernel
struct DecodeTiming { unsigned long long* buf = nullptr; int ring = 0; };
DecodeTiming g_timing;

}  // namespace
void step_call_init(StepCall* k, const MhT5Config* c, const MhT5Weights* w) {
  memset(k, 0, sizeof(*k));
  k->c = c; k->w = w; k->timing_buf = g_timing.buf; k->timing_ring = g_timing.ring;
}
namespace {

// The operands of a layer's GEMVs, each described ONCE: the three launches behind the cross-attention and the fused tail (TailP) read
// the same.  resid_gemv: h += A W^T (+ bias), A [Bc, K]: the output projection of either attention (o_gemv), the FFN's wo / fc2 (ffn_out)
dec::SkinnyP resid_gemv(const StepCall& k, const void* A, int K, const void* W, const float* bias) {
  dec::SkinnyP p{};
  p.A = A; p.lda = K; p.W = W; p.ldw = K; p.B = k.Bc; p.N = k.c->d_model; p.K = K; p.h = k.bf.h; p.ldh = k.c->d_model;
  p.bias = k.c->arch >= 1 ? bias : nullptr;
  return p;
}
dec::SkinnyP o_gemv(const StepCall& k, const void* W, const float* bias) { return resid_gemv(k, k.bf.attn, k.c->n_heads * 64, W, bias); }
dec::SkinnyP ffn_out(const StepCall& k, int l) { return resid_gemv(k, k.bf.ff, k.c->d_ff, k.w->dec_wo[l], k.w->dec_fc2_b[l]); }
// ffn_in: ff = act(norm(h) Wi^T): T5 gated GELU (wi_0 / wi_1 interleaved, N = 2 d_ff), the Whisper family's biased fc1 + erf GELU
dec::SkinnyP ffn_in(const StepCall& k, int l) {
  const MhT5Config* c = k.c;
  dec::SkinnyP p{};
  p.A = k.bf.h; p.lda = c->d_model; p.ln_w = k.w->dec_ln3[l]; p.eps = c->eps; p.W = k.w->dec_wi[l]; p.ldw = c->d_model; p.B = k.Bc;
  p.K = c->d_model; p.out = k.bf.ff; p.ldo = c->d_ff; p.N = c->arch >= 1 ? c->d_ff : 2 * c->d_ff;
  if (c->arch >= 1) p.bias = k.w->dec_fc1_b[l];
  if (c->arch == 2) p.ln_b = k.w->dec_ln3_b[l];
  return p;
}
// the projection an attention kernel does for itself: norm(h) W^T (ln_b: the affine LayerNorm of arch 2, else NULL)
dec::HeadProjP head_proj(const MhT5Config* c, const float* h, const float* ln_w, const float* ln_b, const void* W) {
  dec::HeadProjP hp{};
  hp.h = h; hp.ldh = c->d_model; hp.ln_w = ln_w; hp.eps = c->eps; hp.W = W; hp.ldw = c->d_model; hp.d = c->d_model; hp.ln_b = ln_b;
  return hp;
}
// cross-attention of B rows over layer l of a cross_kv of kvB rows (the plain T5 form: the step adds the rest)
dec::CrossAttnP cross_attn(const MhT5Config* c, const void* cross_kv, int kvB, int l, void* out, int B) {
  const long kv_layer = (long)kvB * c->n_heads * c->src_len * 64 * es_of(c->dtype);
  dec::CrossAttnP ca{};
  ca.k = (const char*)cross_kv + (long)(l * 2 + 0) * kv_layer; ca.v = (const char*)cross_kv + (long)(l * 2 + 1) * kv_layer;
  ca.out = out; ca.ldo = c->n_heads * 64; ca.B = B; ca.H = c->n_heads; ca.L = c->src_len;
  return ca;
}

template <typename T>
int enqueue_step(const StepCall& k, hipStream_t s) {
  const MhT5Config* c = k.c;
  const MhT5Weights* w = k.w;
  const DecBuffers& bf = k.bf;
  const int B = k.Bc, Bfull = k.Bfull, kvB = k.kvB, H = c->n_heads, inner = H * 64, tgt = c->tgt_len, es = (int)sizeof(T);
  const int* posp = &bf.st->pos;
  // arch 1 / 2: the Whisper family (VarWhisperDecoderLayer, modeling_varwhisper.py:633-741); arch 2: affine LayerNorm
  // prologues, the identity rotary table the host packs.  Every arch runs the same six dependent kernels per layer.
  const bool wh = c->arch >= 1, hf = c->arch == 2;
  MH_REQUIRE(!wh || w->dec_rope, "decode: the Whisper family needs its rotary table");
  const Kv8Layout self8 = self_kv8_layout(c, Bfull), cross8 = cross_kv8_layout(c, kvB);
  for (int l = 0; l < c->n_dec_layers; ++l) {
    const long cache_off = (long)l * Bfull * H * tgt * 64 * es;
    MH_REQUIRE(!hf || (w->dec_ln1_b[l] && w->dec_ln2_b[l] && w->dec_ln3_b[l]), "decode: arch 2 needs the LayerNorm biases of layer %d", l);
    // self attention (+ q / k / v projection and self-KV append)
    dec::SelfAttnP sa{};
    sa.kc = (char*)bf.self_k + cache_off; sa.vc = (char*)bf.self_v + cache_off; sa.prompt_mask = k.prompt_mask; sa.P = k.P;
    sa.out = bf.attn; sa.ldo = inner; sa.B = B; sa.H = H; sa.tgt_len = tgt; sa.pos = posp;
    if (wh) {   // biased fused Wqkv, RoPE, scaled scores, optional window
      const bool local = is_local_layer(c, l);
      sa.qkv_bias = w->dec_qkv_b[l]; sa.rope = (local && w->dec_rope_local) ? w->dec_rope_local : w->dec_rope;
      sa.scale = c->attn_scale; sa.window = local ? c->local_window : 0;
    } else {    // T5: the shared relative position bias
      sa.bias = w->dec_rel_bias;
    }
    dec::SelfKv8P f8{};
    if (bf.self8) {   // this layer's k | v planes of the shadow: the chain's first row, the strides those of the full batch
      f8.k8 = bf.self8 + self8.data(l, 0); f8.v8 = bf.self8 + self8.data(l, 1);
      f8.ks = bf.self8_scales + self8.scale(l, 0); f8.vs = bf.self8_scales + self8.scale(l, 1);
    }
    const dec::HeadProjP qkv = head_proj(c, bf.h, w->dec_ln1[l], hf ? w->dec_ln1_b[l] : nullptr, w->dec_qkv[l]);
    MH_TRY(dispatch_kc(qkv.d, [&](auto kc) {
      return launch_self_qkv<T, decltype(kc)::value>(sa, qkv, inner, s, bf.self8 ? &f8 : nullptr, k.origin, k.slot_pos ? k.slot_pos + k.smp.b0 : nullptr);
    }));
    MH_TRY(skinny_resid<T>(o_gemv(k, w->dec_o[l], w->dec_o_b[l]), s));
    // cross attention (+ query projection)
    dec::CrossAttnP ca = cross_attn(c, k.cross_kv, kvB, l, bf.attn, B);
    ca.kv_B = k.kv_group > 1 ? -k.kv_group : (kvB < Bfull ? kvB : 0);
    if (wh) { ca.q_bias = w->dec_cq_b[l]; ca.scale = c->attn_scale; }
    if (k.kv8) {
      ca.k = (const char*)k.kv8 + cross8.data(l, 0); ca.v = (const char*)k.kv8 + cross8.data(l, 1);
      ca.kscale = k.kv8_scales + cross8.scale(l, 0); ca.vscale = k.kv8_scales + cross8.scale(l, 1);
    }
    if (k.timing_buf) {   // one region of ring x layers slots per chain (chain index = first row / rows of a full chain)
      ca.tstamp = k.timing_buf + 2L * bf.chain * k.timing_ring * c->n_dec_layers;
      ca.pos = posp; ca.ts_ring = k.timing_ring; ca.ts_layers = c->n_dec_layers; ca.ts_layer = l;
    }
    MH_TRY(launch_cross_q_d<T>(ca, head_proj(c, bf.h, w->dec_ln2[l], hf ? w->dec_ln2_b[l] : nullptr, w->dec_cq[l]), s));
    const dec::SkinnyP co = o_gemv(k, w->dec_co[l], w->dec_co_b[l]), wi = ffn_in(k, l), wo = ffn_out(k, l);
    if (k.with_sampler && option(OPT_DECODE_FUSED_TAIL) != 0 && tail_covers<T>(c, B, wh, co.bias, wi.bias, wo.bias)) {
      // cross O GEMV + residual, norm + wi + activation, wo + residual as ONE launch (the same device code per phase)
      dec::TailP tp{};
      tp.o = co; tp.wi = wi; tp.wo = wo;
      const int n_chains = ceil_div(Bfull, B);
      if (!wh) MH_TRY((launch_tail<T, dec::PRO_RMSNORM, dec::SK_GEGLU, false>(tp, bf.st, l, n_chains, s)));
      else if (hf) MH_TRY((launch_tail<T, dec::PRO_LAYERNORM, dec::SK_GELU_ERF, true>(tp, bf.st, l, n_chains, s)));
      else MH_TRY((launch_tail<T, dec::PRO_RMSNORM, dec::SK_GELU_ERF, true>(tp, bf.st, l, n_chains, s)));
      continue;
    }
    MH_TRY(skinny_resid<T>(co, s));
    if (!wh) MH_TRY((skinny<T, dec::PRO_RMSNORM, dec::SK_GEGLU>(wi, s)));
    else if (hf) MH_TRY((skinny<T, dec::PRO_LAYERNORM, dec::SK_GELU_ERF, true>(wi, s)));
    else MH_TRY((skinny<T, dec::PRO_RMSNORM, dec::SK_GELU_ERF, true>(wi, s)));
    MH_TRY(skinny_resid<T>(wo, s));
  }
  dec::SkinnyP sk{};
  sk.A = bf.h; sk.lda = c->d_model; sk.ln_w = w->dec_final_ln; sk.eps = c->eps; sk.W = w->lm_head; sk.ldw = c->d_model; sk.B = B;
  sk.N = c->vocab_out; sk.K = c->d_model; sk.out = bf.logits; sk.ldo = c->vocab_out;
  if (hf) { sk.ln_b = w->dec_final_ln_b; MH_TRY((skinny<T, dec::PRO_LAYERNORM, dec::SK_LOGITS>(sk, s))); }
  else MH_TRY((skinny<T, dec::PRO_RMSNORM, dec::SK_LOGITS>(sk, s)));
  if (!k.with_sampler) return MH_OK;
  const SampleP& smp = k.smp;
  if (k.slot_pos) {
    MH_REQUIRE(k.has_rows && smp.pair == 0, "decode: the slot form of the sampler reads row settings and has no guidance");
    SlotSetP ss{};
    ss.rows = k.rows.rows; ss.eos_tables = k.rows.eos_tables; ss.n_eos_sets = k.rows.n_eos_sets; ss.pos = k.slot_pos; ss.plen = k.slot_plen;
    hipLaunchKernelGGL((dec_sample_kernel<T, true, true>), dim3(B), dim3(256), 0, s, smp, ss);
  } else if (k.has_rows) hipLaunchKernelGGL((dec_sample_kernel<T, true>), dim3(smp.pair > 0 ? smp.pair : B), dim3(256), 0, s, smp, k.rows);
  else hipLaunchKernelGGL((dec_sample_kernel<T, false>), dim3(smp.pair > 0 ? smp.pair : B), dim3(256), 0, s, smp, NoRowSetP{});
  return check_launch("dec_sample_kernel");
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
// ---- the token step's launches for the host units (contracts in decode_step.hpp) -----------------------------------------
int enqueue_step(const StepCall& k, hipStream_t s) {
  return dispatch_dtype(k.c->dtype, [&](auto t) { return enqueue_step<decltype(t)>(k, s); });
}
int launch_dec_init(int dtype, const SampleP& smp, int chain_rows, int start_pos, hipStream_t s) {
  if (dtype == MH_BF16) hipLaunchKernelGGL(dec_init_kernel<bf16_t>, dim3(chain_rows), dim3(256), 0, s, smp, chain_rows, start_pos);
  else hipLaunchKernelGGL(dec_init_kernel<float>, dim3(chain_rows), dim3(256), 0, s, smp, chain_rows, start_pos);
  return check_launch("dec_init_kernel");
}
int launch_dec_slot_init(int dtype, const SampleP& smp, int slot, int P, int start_pos, int32_t* slot_pos, int32_t* slot_plen, hipStream_t s) {
  if (dtype == MH_BF16) hipLaunchKernelGGL(dec_slot_init_kernel<bf16_t>, dim3(1), dim3(256), 0, s, smp, slot, P, start_pos, slot_pos, slot_plen);
  else hipLaunchKernelGGL(dec_slot_init_kernel<float>, dim3(1), dim3(256), 0, s, smp, slot, P, start_pos, slot_pos, slot_plen);
  return check_launch("dec_slot_init_kernel");
}
int launch_dec_finalize(const int32_t* finish_col, int B, int32_t* n_steps_out, hipStream_t s) {
  hipLaunchKernelGGL(dec_finalize_kernel, dim3(1), dim3(64), 0, s, finish_col, B, n_steps_out);
  return check_launch("dec_finalize_kernel");
}
int launch_step_embed(int dtype, const int32_t* ids, const void* dec_embed, int d, float* h, DecState* st, int pos, const float* dec_pos,
                      const uint8_t* prompt_mask, int P, int B, hipStream_t s) {
  return dispatch_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(step_embed_kernel<T>, dim3(B), dim3(256), 0, s, ids, (const T*)dec_embed, d, h, st, pos, dec_pos, prompt_mask, P);
    return check_launch("step_embed_kernel");
  });
}
}  // namespace mh

// ---- e4m3 copy of the cross-attention K / V -------------------------------------------------------------------------
// one workgroup per (layer, k|v, row, head) slab of L x 64 bf16: absolute maximum, then x / scale -> OCP e4m3
__global__ __launch_bounds__(256) void kv_quant_fp8_kernel(const bf16_t* src, uint8_t* dst, float* scales, int L) {
  __shared__ float red[4];
  const long slab = (long)blockIdx.x * L * 64;
  const uint4* s16 = reinterpret_cast<const uint4*>(src + slab);
  const int n16 = L * 8;   // 16-byte vectors (8 elements) in the slab
  float mx = 0.f;
  for (int i = threadIdx.x; i < n16; i += 256) {
    const uint4 v = s16[i];
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      mx = fmaxf(mx, fabsf(__uint_as_float(w[j] << 16)));
      mx = fmaxf(mx, fabsf(__uint_as_float(w[j] & 0xffff0000u)));
    }
  }
  mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  const float scale = mx > 0.f ? mx / 448.0f : 1.0f;   // 448 = largest finite e4m3 value
  const float inv = 1.0f / scale;
  if (threadIdx.x == 0) scales[blockIdx.x] = scale;
  uint2* d8 = reinterpret_cast<uint2*>(dst + slab);
  for (int i = threadIdx.x; i < n16; i += 256) {
    const uint4 v = s16[i];
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    float f[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) { f[2 * j] = __uint_as_float(w[j] << 16) * inv; f[2 * j + 1] = __uint_as_float(w[j] & 0xffff0000u) * inv; }
    int o0 = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], 0, false);
    o0 = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], o0, true);
    int o1 = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], 0, false);
    o1 = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], o1, true);
    d8[i] = make_uint2((uint32_t)o0, (uint32_t)o1);
  }
}
// The same for ONE row of an S-row copy (mh_t5_slots_admit over a session of mh_t5_slots_open_kv8): workgroup (plane, h) of a window's
// compact cross K/V [n_dec][2][1][H][L][64] -> unit plane * S H + slot H + h of cross_kv8_layout(c, S), bytes and scale alike.  A
// kernel of its own (kv_quant_fp8_kernel keeps its instruction bytes) with the statements of the one above in their order: the bytes
// and scales mh_t5_quantize_cross_kv(B = 1) makes of that row (pinned by tests/test_gpu_inflight_kv8.py).  No other row is written.
__global__ __launch_bounds__(256) void kv_quant_fp8_row_kernel(const bf16_t* src, uint8_t* dst, float* scales, int L, int H, int S, int slot) {
  __shared__ float red[4];
  const long plane = blockIdx.x / H, h = blockIdx.x % H;
  const long unit = (plane * S + slot) * H + h;
  const uint4* s16 = reinterpret_cast<const uint4*>(src + (long)blockIdx.x * L * 64);
  const int n16 = L * 8;
  float mx = 0.f;
  for (int i = threadIdx.x; i < n16; i += 256) {
    const uint4 v = s16[i];
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      mx = fmaxf(mx, fabsf(__uint_as_float(w[j] << 16)));
      mx = fmaxf(mx, fabsf(__uint_as_float(w[j] & 0xffff0000u)));
    }
  }
  mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  const float scale = mx > 0.f ? mx / 448.0f : 1.0f;
  const float inv = 1.0f / scale;
  if (threadIdx.x == 0) scales[unit] = scale;
  uint2* d8 = reinterpret_cast<uint2*>(dst + unit * L * 64);
  for (int i = threadIdx.x; i < n16; i += 256) {
    const uint4 v = s16[i];
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    float f[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) { f[2 * j] = __uint_as_float(w[j] << 16) * inv; f[2 * j + 1] = __uint_as_float(w[j] & 0xffff0000u) * inv; }
    int o0 = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], 0, false);
    o0 = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], o0, true);
    int o1 = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], 0, false);
    o1 = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], o1, true);
    d8[i] = make_uint2((uint32_t)o0, (uint32_t)o1);
  }
}

extern "C" int64_t mh_t5_cross_kv_fp8_bytes(const MhT5Config* c, int B) {
  mh::OptionScope option_scope(c ? c->options : nullptr);
  if (!c || B <= 0) return -1;
  return cross_kv8_layout(c, B).total;
}

extern "C" int mh_t5_quantize_cross_kv(const MhT5Config* c, const void* cross_kv, int B, void* out, void* stream) {
  mh::OptionScope option_scope(c ? c->options : nullptr);
  MH_TRY(check_cfg(c, "mh_t5_quantize_cross_kv"));
  MH_REQUIRE(cross_kv && out && B > 0, "mh_t5_quantize_cross_kv: null argument");
  MH_REQUIRE(c->dtype == MH_BF16, "mh_t5_quantize_cross_kv: needs bf16 storage");
  const Kv8Layout ly = cross_kv8_layout(c, B);
  const int slabs = c->n_dec_layers * 2 * (int)ly.plane_scales;   // one workgroup and one scale per (layer, k|v, row, head)
  hipLaunchKernelGGL(kv_quant_fp8_kernel, dim3(slabs), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)cross_kv,
                     (uint8_t*)out, reinterpret_cast<float*>((char*)out + ly.scales_offset), c->src_len);
  return check_launch("kv_quant_fp8_kernel");
}

// ---- e4m3 shadow of the self-attention cache ----------------------------------------------------------------------------
// One wave per 64-element bf16 row (dec::quant_row64: the token step's append is the same function).  Rows are addressed as
// (plane y, slab, position): plane y = (layer, k|v) reads src_k / src_v at layer * n_slabs * stride rows and writes plane y of q /
// scales; within a plane, row (slab, i) for i < n_pos sits at row slab * stride + i of both.  Plain buffers: one plane, one slab.
// plane_rows: the rows of a whole plane, n_slabs * stride when every slab is visited -- more when only the first n_slabs of a plane
// are (mh_t5_self_kv_fp8_fill: the prompts' rows of a (chunk, beam) batch).
__global__ __launch_bounds__(256) void self_kv_quant_rows_kernel(const bf16_t* src_k, const bf16_t* src_v, uint8_t* q, float* scales,
                                                                long n_slabs, long n_pos, long stride, long plane_rows) {
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);   // (wave-uniform)
  if (r >= n_slabs * n_pos) return;
  const long slab = r / n_pos, i = r - slab * n_pos;
  const long y = blockIdx.y;
  const bf16_t* src = ((y & 1) ? src_v : src_k) + (y >> 1) * plane_rows * 64;
  const long row = slab * stride + i;
  const float x = mh::Elem<bf16_t>::to_f32(src[row * 64 + (threadIdx.x & 63)]);
  mh::dec::quant_row64(x, q + (y * plane_rows + row) * 64, scales + y * plane_rows + row);
}

namespace mh {
int launch_self_kv_quant_rows(const MhT5Config* c, int B, const DecBuffers& bf, uint8_t* self8, int n_rows, int n_pos, hipStream_t s) {
  const long n_slabs = (long)n_rows * c->n_heads, plane_rows = (long)B * c->n_heads * c->tgt_len;
  hipLaunchKernelGGL(self_kv_quant_rows_kernel, dim3((unsigned)((n_slabs * n_pos + 3) / 4), 2 * c->n_dec_layers), dim3(256), 0, s,
                     (const bf16_t*)bf.self_k, (const bf16_t*)bf.self_v, self8,
                     reinterpret_cast<float*>(self8 + self_kv8_layout(c, B).scales_offset), n_slabs, (long)n_pos, (long)c->tgt_len, plane_rows);
  return check_launch("self_kv_quant_rows_kernel");
}
int launch_self_kv_quant_slot(const MhT5Config* c, int S, const DecBuffers& bf, uint8_t* self8, int slot, int n_pos, hipStream_t s) {
  const int H = c->n_heads;
  const long row0 = (long)slot * H * c->tgt_len, plane_rows = (long)S * H * c->tgt_len;
  hipLaunchKernelGGL(self_kv_quant_rows_kernel, dim3((unsigned)(((long)H * n_pos + 3) / 4), 2 * c->n_dec_layers), dim3(256), 0, s,
                     (const bf16_t*)bf.self_k + row0 * 64, (const bf16_t*)bf.self_v + row0 * 64, self8 + row0 * 64,
                     reinterpret_cast<float*>(self8 + self_kv8_layout(c, S).scales_offset) + row0, (long)H, (long)n_pos,
                     (long)c->tgt_len, plane_rows);
  return check_launch("self_kv_quant_rows_kernel");
}
int launch_cross_kv_quant_row(const MhT5Config* c, int S, const void* cross_kv_row, uint8_t* cross8, int slot, hipStream_t s) {
  const int H = c->n_heads;
  hipLaunchKernelGGL(kv_quant_fp8_row_kernel, dim3(c->n_dec_layers * 2 * H), dim3(256), 0, s, (const bf16_t*)cross_kv_row, cross8,
                     reinterpret_cast<float*>(cross8 + cross_kv8_layout(c, S).scales_offset), c->src_len, H, S, slot);
  return check_launch("kv_quant_fp8_row_kernel");
}
}  // namespace mh

extern "C" int mh_quantize_kv_rows(const void* x_bf16, int64_t n_rows, void* q, float* scales, void* stream) {
  MH_REQUIRE(x_bf16 && q && scales, "mh_quantize_kv_rows: null argument");
  MH_REQUIRE(n_rows > 0, "mh_quantize_kv_rows: n_rows %lld must be positive", (long long)n_rows);
  // a launch holds fewer than 2^32 threads: 2^24 rows (2^22 workgroups of four waves) at a time
  constexpr int64_t kChunk = 1LL << 24;
  for (int64_t r0 = 0; r0 < n_rows; r0 += kChunk) {
    const int64_t n = n_rows - r0 < kChunk ? n_rows - r0 : kChunk;
    const bf16_t* x = (const bf16_t*)x_bf16 + r0 * 64;
    hipLaunchKernelGGL(self_kv_quant_rows_kernel, dim3((unsigned)((n + 3) / 4), 1), dim3(256), 0, (hipStream_t)stream, x, x,
                       (uint8_t*)q + r0 * 64, scales + r0, 1L, (long)n, (long)n, (long)n);
    MH_TRY(check_launch("self_kv_quant_rows_kernel"));
  }
  return MH_OK;
}

extern "C" int64_t mh_t5_self_kv_fp8_bytes(const MhT5Config* c, int B) {
  mh::OptionScope option_scope(c ? c->options : nullptr);
  if (!c || B <= 0) return -1;
  if (c->dtype != MH_BF16) { mh::set_error("mh_t5_self_kv_fp8_bytes: the e4m3 self-attention cache needs bf16 storage"); return -1; }
  return self_kv8_layout(c, B).total;
}

// ------------------------------------------------------------------------------------------------
// In-situ timing of the dominant kernel.  `buf` (device, uint64 [n_chains][ring][n_dec_layers][2], pre-filled by the
// caller with (UINT64_MAX, 0) pairs) makes every cross-attention launch of the following mh_t5_generate calls record its
// earliest workgroup start and latest workgroup end in wall-clock ticks (hipDeviceAttributeWallClockRate kHz); slot =
// decode position % ring.  buf = NULL switches it off.  Costs two atomics per workgroup: bench.py uses an EXTRA decode
// pass for it, never the timed region.
extern "C" int mh_t5_decode_timing(void* buf, int ring) {
  MH_REQUIRE((buf == nullptr) == (ring <= 0), "mh_t5_decode_timing: buf and ring go together");
  mh::g_timing.buf = (unsigned long long*)buf;
  mh::g_timing.ring = ring;
  return MH_OK;
}

#ifdef MH_PHASE_STAMPS
// profiling build only: read (and optionally clear) the phase stamps; out = host uint64 [16][16][2]
extern "C" int mh_debug_phase_stamps(unsigned long long* out, int reset) {
  if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(mh::dec::g_stamps), sizeof(mh::dec::g_stamps)) != hipSuccess)
    return mh::check_launch("stamps read");
  if (reset) {
    static unsigned long long zero[16 * 16 * 2] = {};
    if (hipMemcpyToSymbol(HIP_SYMBOL(mh::dec::g_stamps), zero, sizeof(zero)) != hipSuccess) return mh::check_launch("stamps reset");
  }
  return MH_OK;
}
#endif

extern "C" int mh_wall_clock_khz(void) {   // rate of the device wall clock the timing hook records (kHz); 0 if unknown
  int dev = 0, khz = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return khz;
}

// DecState::tail_err -> status: what mh_t5_generate returns (and mh_last_error() says) for the word the decode step leaves
extern "C" int mh_t5_decode_tail_status(int err_word) {
  if (err_word == 0) return MH_OK;
  mh::set_error("decode: a hand-off of the fused layer tail (option decode_fused_tail) waited longer than 2 ms and gave up (error word %d); "
                "the tokens of this call are not valid", err_word);
  return MH_ERR_DECODE_TAIL_TIMEOUT;
}

// dec_tail_kernel launches enqueued so far (a captured graph node counts once, at capture): lets a caller -- the tests -- tell
// that option decode_fused_tail = 1 really took the fused path for its shape instead of the silent three-launch fall-back
extern "C" long mh_t5_decode_tail_launches(void) { return mh::g_tail_launches.load(); }

// ------------------------------------------------------------------------------------------------
// Measurement hook for bench.py's roofline line: the dominant decode kernel (cross-attention over the
// encoder keys) launched `reps` times back to back between two HIP events ON THE GIVEN STREAM, cycling
// through the decoder layers exactly like a decode step does (so every launch streams a different layer's
// K/V: B*H*L*64*2 elements).  ms_out[0] = average milliseconds per launch (split kernel + merge kernel).
extern "C" int mh_t5_cross_attn_probe(const MhT5Config* c, const MhT5Weights* w, const void* cross_kv, int B, int reps,
                                      float* ms_out, void* workspace, int64_t workspace_bytes, void* stream) {
  mh::OptionScope option_scope(c ? c->options : nullptr);
  MH_TRY(check_cfg(c, "mh_t5_cross_attn_probe"));
  MH_TRY(check_decode_shape(c, "mh_t5_cross_attn_probe"));
  MH_REQUIRE(w && cross_kv && ms_out && workspace && B > 0 && B <= 64 && reps > 0, "mh_t5_cross_attn_probe: bad argument");
  MH_REQUIRE(workspace_bytes >= mh_t5_decode_workspace_bytes(c, B), "mh_t5_cross_attn_probe: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const DecodeLayout ly = decode_layout(c, B, workspace);
  float* h = ly.bf.h;
  if (hipMemsetAsync(h, 0, (size_t)B * c->d_model * 4, s) != hipSuccess) return check_launch("probe memset");
  hipEvent_t e0, e1;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return check_launch("event create");
  int rc = MH_OK;
  for (int pass = 0; pass < 2 && rc == MH_OK; ++pass) {   // pass 0 = warm-up
    if (pass == 1) (void)hipEventRecord(e0, s);
    for (int r = 0; r < reps && rc == MH_OK; ++r) {
      const int l = r % c->n_dec_layers;
      const dec::CrossAttnP ca = cross_attn(c, cross_kv, B, l, ly.bf.attn, B);
      const dec::HeadProjP hp = head_proj(c, h, w->dec_ln2[l], nullptr, w->dec_cq[l]);
      rc = dispatch_dtype(c->dtype, [&](auto t) { return launch_cross_q_d<decltype(t)>(ca, hp, s); });
    }
    if (pass == 1) (void)hipEventRecord(e1, s);
  }
  if (rc == MH_OK) {
    float ms = 0.f;
    if (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess)
      rc = check_launch("probe events");
    else
      ms_out[0] = ms / (float)reps;
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  return rc;
}
