// What the host units (t5_step.hip, t5_generate.hip, t5_stepwise.hip, t5_encode.hip) need of the token step: the structs a step is
// described by, the decode workspace layout, and plain host functions that launch the step's kernels.  No kernel is declared here:
// every kernel of the token step is instantiated in ONE unit -- decode_gemv.hip, decode_attn_bf16.hip, decode_attn_f32.hip,
// decode_sample.hip -- and the families meet in enqueue_step (t5_step.hip), which is host code.
#pragma once
#include <string.h>

#include <type_traits>

#include "decode_params.hpp"
#include "t5_host.hpp"

namespace mh {

constexpr int kMaxChains = 8;

struct DecState {       // device-resident control block
  int pos;              // index of the token being fed this step
  int n_running;        // rows not yet finished (written by the sampler)
  int tail_err;         // != 0: a hand-off of dec_tail_kernel gave up (bounded wait); read by the host right after n_running
  int ticket;           // arrival counter of the sampler's workgroups (the last one advances `pos`)
  unsigned rng_row0;    // MhSampling.rng_row0 and .seed of the running call: written by dec_init_kernel and read from here by
  unsigned long long seed;   // the sampler, so that the replayed step graph does not carry them (they change call by call)
  // dec_tail_kernel's hand-off counters, one 128-byte line per layer parity: zeroed by dec_init_kernel, then only ever added to
  alignas(128) unsigned tail_cnt[2][32];
};

struct SampleP {
  const float* logits; int ldl; int V;
  int32_t* tokens; int max_length;    // [B, max_length]
  const int32_t* forced;
  const uint8_t* eos_table;
  uint8_t* finished;                  // [B]
  int32_t* finish_col;                // [B]
  int32_t* last_ts_val;               // [B] value of the last TIME_SHIFT after the last SOS, -1 if none
  float* logits_dump;                 // [max_length][R][V] or null   (R = returned rows: B, or B/2 with CFG)
  float* proc;                        // [R][V] processed scores of this step (read back by the sampling passes)
  float* hist_scores;                 // [2][R][V] scores entering LookbackBias at this / the previous step
  const void* dec_embed; float* h; int d;
  // arch 2 (HF Whisper): decoder.embed_positions fp32 [tgt_len][d] added to the token embedding (NULL otherwise); pos_off [B] =
  // masked prompt columns of each row when MhT5Config.dec_pos_from_mask (written by dec_init_kernel), NULL = cache positions
  const float* dec_pos; int32_t* pos_off; const uint8_t* prompt_mask;
  MhSampling sp;
  DecState* st;
  int B, P;                           // B = rows of the WHOLE batch
  int b0;                             // first global row of this chain; logits / h / ss are chain-local
  int pair;                           // CFG: distance between the negative-prompt row g and its prompt row g + pair
                                      //      (= B/2, single chain); 0 = no guidance
  int chain_rows;                     // rows of this chain (both halves under CFG)
};

// dec_sample_kernel's trailing argument: the row settings of mh_t5_generate_rows (the ROWS instantiations), or nothing
struct RowSetP { const MhRowSampling* rows; const uint8_t* eos_tables; int n_eos_sets; };

struct DecBuffers {
  float* h; void* attn; void* ff; float* logits; int chain;
  void* self_k; void* self_v;  // [n_dec][B][H][tgt][64]
  uint8_t* finished; int32_t* finish_col; int32_t* last_ts; DecState* st;
  // the caller's e4m3 shadow of the self-attention cache (mh_t5_generate_skv8), else NULL: e4m3 [n_dec][2][B][H][tgt][64] and its
  // fp32 scales [n_dec][2][B][H][tgt].  Non-NULL selects the F8 self-attention kernel (and, being part of this struct, is part of
  // the step graph's cache key)
  uint8_t* self8; float* self8_scales;
};

// The decode workspace of B rows (mh_t5_decode_workspace_bytes): the one description of its slabs, read by mh_t5_generate,
// mh_t5_step, mh_t5_cross_attn_probe and mh_t5_reorder_cache.  base == NULL: sizes only (every pointer NULL).
struct DecodeLayout {
  DecBuffers bf;                      // the whole batch; bf.st = the first of kMaxChains states, align256(sizeof(DecState)) apart
  int32_t* pos_off; float* proc; float* hist_scores;
  int64_t end;                        // the batched prompt prefill's region starts here
};
// (t5_step.hip)
DecodeLayout decode_layout(const MhT5Config* c, int B, void* base);

// Everything ONE enqueue of a token step depends on: enqueue_step() reads this and option(), nothing else, and step_graph_key() makes
// a step graph's cache key of exactly this -- a new input of the step is a new field here and so cannot be missing from the key.  Made by
// step_call_init() (zero bytes, padding included), then assigned field by field.  Every pointer is at the chain's first row.
struct StepCall {
  const MhT5Config* c; const MhT5Weights* w;
  const void* cross_kv;                  // kvB rows per (layer, k | v) slab: B/2 under CFG (a pair shares its encoder output, row b
  int Bc, Bfull, kvB;                    // reads K/V row b % kvB); Bc = rows of this chain, Bfull = of the whole batch
  const uint8_t* prompt_mask; int P;
  DecBuffers bf;
  SampleP smp;                           // (all zero without the sampler)
  const void* kv8; const float* kv8_scales;   // the e4m3 copy of cross_kv and its scales (mh_t5_quantize_cross_kv), or NULL
  int with_sampler;                      // 0: the step ends with the logits (mh_t5_step: the host selects)
  int kv_group;                          // > 1: rows are (chunk, beam) pairs and row b reads cross K/V row b / kv_group
  int has_rows; RowSetP rows;            // has_rows: the sampler reads its settings per returned row (mh_t5_generate_rows)
  unsigned long long* timing_buf; int timing_ring;   // the timing hook as it stood when the call was built
  const uint8_t* origin;                 // beam search by index (mh_t5_step_indexed): uint8 [Bfull][tgt_len], else NULL
  int32_t* slot_pos; const int32_t* slot_plen;   // in-flight decode (mh_t5_slots_*): the positions and prompt lengths of all Bfull slots
                                                 // (global row index; the SLOT kernels), else NULL.  Needs has_rows.
};
static_assert(std::is_trivially_copyable<StepCall>::value, "StepCall is keyed by its bytes");
// (t5_step.hip: it reads the timing hook, which lives there)
void step_call_init(StepCall* k, const MhT5Config* c, const MhT5Weights* w);

// The first row of the e4m3 shadow of the self-attention cache, and of its scales, at row b0 of a B-row batch (the b0 offsets of the
// bf16 caches); the same over the packed e4m3 copy of the cross K/V of kvB rows
inline void self8_rows(const MhT5Config* c, int B, int b0, void* self8, DecBuffers* bf) {
  const long row = (long)b0 * c->n_heads * c->tgt_len;
  bf->self8 = (uint8_t*)self8 + row * 64;
  bf->self8_scales = reinterpret_cast<float*>((uint8_t*)self8 + self_kv8_layout(c, B).scales_offset) + row;
}
inline void cross8_rows(const MhT5Config* c, int kvB, int b0, const void* kv8, StepCall* k) {
  k->kv8 = (const char*)kv8 + (long)b0 * c->n_heads * c->src_len * 64;
  k->kv8_scales = reinterpret_cast<const float*>((const char*)kv8 + cross_kv8_layout(c, kvB).scales_offset) + (long)b0 * c->n_heads;
}

// ---- the batched prompt prefill (t5_encode.hip) -----------------------------------------------------------------------------------
struct PrefillBuf {
  float* h; void* n; void* q; void* attn; void* ff; void* vt; void* cross_vt;
  int np_pad, Lpad;
};

// the prefill's slabs of B rows x np_max positions over [base, base + size) -> bytes used; base == NULL: the size only
int64_t prefill_layout(const MhT5Config* c, int B, int np_max, void* base, int64_t size, PrefillBuf* out);
// Batched prompt prefill: positions 0 .. P-2 of every row go through the decoder stack at once (MFMA GEMMs +
// flash attention), filling the self-attention K/V caches exactly as P-1 single-token steps would
// (HF prefill: SURVEY.md appendix A.1).  Position P-1 is left to the per-token loop, which also produces the
// first sampled token.  Left-pad keys are masked, left-pad query rows produce unused garbage, as in HF.
int prefill_prompt(const MhT5Config* c, const MhT5Weights* w, const void* cross_kv, int B, int kvB, const int32_t* prompt,
                   const uint8_t* prompt_mask, int P, int np, void* self_k, void* self_v, const PrefillBuf& pb, hipStream_t s,
                   int cache_rows = 0, int plan_B = 0);

// ---- the token step (t5_step.hip) --------------------------------------------------------------------------------------------------
// One token step of the chain `k` describes: every layer, the LM head and (k.with_sampler) the sampler
int enqueue_step(const StepCall& k, hipStream_t s);

// ---- launches of the token step's kernels ------------------------------------------------------------------------------------------
// Each enqueues on `s` in the storage type `dtype` (MH_F32 / MH_BF16) where the kernel has one, and returns check_launch() under the
// kernel's name.  Each dispatches to the instantiations its unit holds; a combination that has no kernel is MH_ERR_ARG.
// (decode_gemv.hip) gemv_kernel<dtype, rows of p.B, waves of p.K, pro, epi, bias>: PRO_* / SK_* of decode_params.hpp, in the seven
// combinations a step uses -- (PLAIN, RESID, bias or not), (RMSNORM, GEGLU), (RMSNORM | LAYERNORM, GELU_ERF, bias), (RMSNORM |
// LAYERNORM, LOGITS)
int launch_gemv(int dtype, int pro, int epi, bool bias, const dec::SkinnyP& p, hipStream_t s);
// whether dec_tail_kernel covers a chain of B rows of this model (wh: the Whisper family, with its three tail biases), else the three
// launches run; and the launch: o / wi / wo = the SkinnyP descriptions of the three launches it replaces, (prowi, epiwi, bias) = the
// form of the wi GEMV, `st` / `layer` = whose hand-off counters, n_chains = chains that may run side by side
bool tail_covers(const MhT5Config* c, int B, bool wh, const float* b_o, const float* b_fc1, const float* b_fc2);
int launch_tail(int dtype, int prowi, int epiwi, bool bias, const dec::TailP& p, DecState* st, int layer, int n_chains, hipStream_t s);
// (decode_attn_bf16.hip / decode_attn_f32.hip: the attention kernels of one storage type each)
// dec_self_attn_qkv_kernel, or with slot_pos dec_slot_self_attn_kernel, in the form (sa.rope, hp.ln_b) say.  f8 != NULL: over this
// layer's rows of the e4m3 shadow cache (bf16 storage only); origin != NULL: cached rows through the beam search's index table;
// slot_pos != NULL: every row at its own position
int launch_self_attn_bf16(const dec::SelfAttnP& sa, const dec::HeadProjP& hp, int inner, const dec::SelfKv8P* f8, const uint8_t* origin,
                          const int32_t* slot_pos, hipStream_t s);
int launch_self_attn_f32(const dec::SelfAttnP& sa, const dec::HeadProjP& hp, int inner, const dec::SelfKv8P* f8, const uint8_t* origin,
                         const int32_t* slot_pos, hipStream_t s);
inline int launch_self_attn(int dtype, const dec::SelfAttnP& sa, const dec::HeadProjP& hp, int inner, const dec::SelfKv8P* f8,
                            const uint8_t* origin, const int32_t* slot_pos, hipStream_t s) {
  return dtype == MH_BF16 ? launch_self_attn_bf16(sa, hp, inner, f8, origin, slot_pos, s) : launch_self_attn_f32(sa, hp, inner, f8, origin, slot_pos, s);
}
// dec_cross_attn_q_kernel in the form (ca.scale != 0, hp.ln_b) say; ca.kscale != NULL: over the e4m3 copy (bf16 storage only)
int launch_cross_attn_bf16(const dec::CrossAttnP& ca, const dec::HeadProjP& hp, hipStream_t s);
int launch_cross_attn_f32(const dec::CrossAttnP& ca, const dec::HeadProjP& hp, hipStream_t s);
inline int launch_cross_attn(int dtype, const dec::CrossAttnP& ca, const dec::HeadProjP& hp, hipStream_t s) {
  return dtype == MH_BF16 ? launch_cross_attn_bf16(ca, hp, s) : launch_cross_attn_f32(ca, hp, s);
}
// (decode_sample.hip, as everything below) dec_sample_kernel over the logits of k's chain: the uniform form, the per-row form
// (k.has_rows) or the slot form (k.slot_pos)
int launch_sample(int dtype, const StepCall& k, hipStream_t s);
// dec_init_kernel over the chain_rows rows of smp's chain: the processors' state over prompt columns 0 .. start_pos, the chain's
// DecState, the embedding of the token at start_pos
int launch_dec_init(int dtype, const SampleP& smp, int chain_rows, int start_pos, hipStream_t s);
// dec_slot_init_kernel: the same for the ONE slot `slot` (prompt length P) of an in-flight decode; slot_pos[slot] is written last
int launch_dec_slot_init(int dtype, const SampleP& smp, int slot, int P, int start_pos, int32_t* slot_pos, int32_t* slot_plen, hipStream_t s);
// *n_steps_out = 1 + the largest finish column of the B rows
int launch_dec_finalize(const int32_t* finish_col, int B, int32_t* n_steps_out, hipStream_t s);
// step_embed_kernel: h[b] = dec_embed[ids[b]] (+ dec_pos, arch 2) for B rows and the position word of the step (mh_t5_step*)
int launch_step_embed(int dtype, const int32_t* ids, const void* dec_embed, int d, float* h, DecState* st, int pos, const float* dec_pos,
                      const uint8_t* prompt_mask, int P, int B, hipStream_t s);
// positions 0 .. n_pos-1 of cache rows 0 .. n_rows-1 of a B-row batch's bf16 self-attention caches -> the B-row shadow self8, every
// layer, k and v
int launch_self_kv_quant_rows(const MhT5Config* c, int B, const DecBuffers& bf, uint8_t* self8, int n_rows, int n_pos, hipStream_t s);
// ... of the ONE cache row `slot` of an S-row session into the same places of the S-row shadow (mh_t5_slots_admit); no other row is written
int launch_self_kv_quant_slot(const MhT5Config* c, int S, const DecBuffers& bf, uint8_t* self8, int slot, int n_pos, hipStream_t s);
// kv_quant_fp8_row_kernel: a window's compact bf16 cross K/V [n_dec][2][1][H][L][64] -> row `slot` of the S-row e4m3 copy cross8
int launch_cross_kv_quant_row(const MhT5Config* c, int S, const void* cross_kv_row, uint8_t* cross8, int slot, hipStream_t s);

#ifdef MH_PHASE_STAMPS
// profiling build only: acc (host, uint64 [16][16][2]) += the phase stamps of the unit's kernels; reset: cleared afterwards
int gemv_phase_stamps(unsigned long long* acc, int reset);
int attn_bf16_phase_stamps(unsigned long long* acc, int reset);
int attn_f32_phase_stamps(unsigned long long* acc, int reset);
#endif

}  // namespace mh
