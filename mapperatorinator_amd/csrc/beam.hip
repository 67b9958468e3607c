// One beam-search step as ONE kernel (round 6): HF `GenerationMixin._beam_search` (third-party; the vectorised form of transformers
// >= 4.50 as `model_generate` reaches it with num_beams > 1: osuT5/osuT5/inference/processor.py:147,159; server.py:137; the timing
// pass decodes with two beams, super_timing_generator.py:28) between two decoder positions --
//     log_softmax -> [classifier-free guidance] -> the reference's processor list on LOG-PROBABILITIES (server.py:106-134:
//     MonotonicTimeShift, TimeshiftBias, (Conditional)Temperature, LookbackBias) -> + running beam scores -> the K = max(2, 1 + #eos)
//     x num_beams best continuations of the chunk -> EOS / max_length split -> next running beams -> merge of the finished
//     hypotheses -> the "can a running beam still win" heuristic
// -- beside mh_t5_step (the decoder position) and mh_t5_reorder_cache (MapperatorinatorCache.reorder_cache, inference/cache_utils.py:
// 16-20).  mapperatorinator_amd/beam.py ran these as ~40 ATen launches per token until round 5.
// One workgroup per chunk: the K best of its num_beams x V accumulated scores are found in LDS -- a 4-pass radix select of the K-th
// largest value, a deterministic compaction (ties by ascending flat index), then a bitonic sort of the K candidates only (the first
// version sorted all 8192 values: 86 us per token against ~15 us) --, the selection logic runs on that sorted list, the surviving hypotheses are copied from the IN state to the OUT state (ping-pong: every
// workgroup reads what the previous step wrote).  Greedy beams (do_sample = 0) are mh_beam_step / mh_beam_step_tf.
// Beam-SAMPLE is a third template flag, beam_step_kernel<kStream, kTf, kSample> (mh_beam_step_sample; the greedy instantiations keep
// their loops): HF's TopK / TopP warpers become ONE cut value per beam row (beam_row_select: radix selects by count and by softmax
// mass, the masses summed as 64-bit fixed-point integers in LDS, so both kernels and every launch agree bit for bit; a group of equal
// values at the top-p boundary stays or goes whole, where HF may split it by sort order), the accumulated score is beam_warp(), and
// the draw is Gumbel top-K: the radix select, compaction and sort below run on key = score + -log(-log(u)) (beam_key; u from the
// sampler's counter-based generator, folded in common.hpp), after which every candidate's key gives way to its score again.  The K
// candidates are then K draws without replacement IN DRAW ORDER, which is what the selection logic behind the sort assumes of them.
// A -inf score keeps a -inf key: drawn only when the finite ones run out, by flat index.  Without the opt-in (beam.py `device_draw`)
// beam-sample still draws with torch.multinomial / an injected sampler on the host-side path.
// Two kernels, one body (beam_step_kernel<kStream>): the LDS kernel keeps the num_beams x V accumulated scores in LDS (at most 120 KB
// with the K <= 4096 candidates); the STREAMING kernel keeps per-beam softmax / processor state only (BeamRow) and recomputes a score
// from the logits -- read once from HBM, from L2 afterwards -- in every pass that needs one, so any vocabulary and K <= 8192 fit.
// Both evaluate a score with beam_score() and reduce a row in the same thread -> column order: same bits wherever both can run.
#include <math.h>

#include "internal.hpp"

namespace mh {
namespace {

struct BeamKV { float v; int i; };

// descending by value, ties by ascending flat index (deterministic; NaN never occurs: scores are finite or -inf)
__device__ inline bool beam_before(const BeamKV& a, const BeamKV& b) { return a.v > b.v || (a.v == b.v && a.i < b.i); }

constexpr int kBeamThreads = 512;
constexpr int kBeamWaves = kBeamThreads / 64;
constexpr int kBeamMaxK = 8192;      // candidates per chunk the selection logic holds flags for
constexpr int kBeamLdsMaxK = 4096;   // ... of them under the LDS kernel
constexpr int kBeamLdsBytes = 120 * 1024;   // LDS kernel: score array + candidates
constexpr int kBeamMaxBeams = 8;

// order-preserving integer image of a float (-0.0 folded onto +0.0, so equal floats have equal images)
__device__ inline unsigned beam_okey(float x) {
  const unsigned u = __float_as_uint(x + 0.0f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// exclusive prefix sum of one int per thread over the block (wave shuffles + the 8 wave totals); `total` = the block's sum
__device__ inline int beam_excl_scan(int x, int* s_w, int& total) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  int inc = x;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const int y = __shfl_up(inc, o, 64); if (lane >= o) inc += y; }
  __syncthreads();
  if (lane == 63) s_w[wid] = inc;
  __syncthreads();
  int base = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < kBeamWaves; ++w) { const int t = s_w[w]; base += w < wid ? t : 0; total += t; }
  return base + inc - x;
}

// block-wide maximum of a 64-bit key
__device__ inline unsigned long long beam_max_u64(unsigned long long k, unsigned long long* s_w) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)k, o, 64), hi = __shfl_xor((unsigned)(k >> 32), o, 64);
    const unsigned long long y = ((unsigned long long)hi << 32) | lo;
    k = y > k ? y : k;
  }
  __syncthreads();
  if (lane == 0) s_w[wid] = k;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < kBeamWaves; ++w) { const unsigned long long y = s_w[w]; k = y > k ? y : k; }
  return k;
}

// (score, position) -> one key whose maximum is "best score, then earliest position"
__device__ inline unsigned long long beam_rank_key(float sc, int pos) {
  return ((unsigned long long)beam_okey(sc) << 32) | (unsigned)(0x7fffffff - pos);
}

// what one beam's row of accumulated scores depends on besides the logits: log-softmax maximum / log-sum-exp of the prompt row (and of
// the negative row under guidance), MonotonicTimeShift bound, temperature of the step, running score
struct BeamRow { float mp, lse_p, mn, lse_n, temp, rs; int ltv; };

// LookbackBiasLogitsWarper, types_first = True (logit_processors.py:116-133), per beam row of the step: does the row renormalise
// (its last id is a timed event and a previous call exists), the maximum of the scores x that enter the processor, log(sum exp(x -
// mc)) - log(s), and log(prob_eos_extra), the value of the first TIME_SHIFT id.  kTf instantiations only (mh_beam_step_tf).
struct BeamTf { int renorm; float mc, log_norm, log_extra; };

// accumulated score of column v of a beam from its raw logit(s): log_softmax -> guidance -> the processor list -> + running score.
// THE definition for every pass of both kernels (nothing here may contract into an FMA: the guidance combine is spelled out, the
// rest is subtract / add / divide)
// beam_pre is the part in front of LookbackBiasLogitsWarper (what the types_first branch keeps as `last_scores` and renormalises).
__device__ inline float beam_pre(const MhBeamStep& p, const BeamRow& b, float lp, float ln, int v) {
  const MhSampling& sp = p.sp;
  float x = (lp - b.mp) - b.lse_p;
  if (p.cfg) {   // HF ClassifierFreeGuidanceLogitsProcessor, first in the list, on the reference's row order: second + (first - second) * scale
    const float xn = (ln - b.mn) - b.lse_n;
    x = __fadd_rn(x, __fmul_rn(__fsub_rn(xn, x), p.cfg_scale));
  }
  if (b.ltv >= 0 && v >= sp.ts_start && v < sp.ts_start + b.ltv) x = -INFINITY;
  if (sp.timeshift_bias != 0.f && v >= sp.ts_start && v < sp.ts_end) x += sp.timeshift_bias;
  return x / b.temp;
}

// beam_x is the processed score of the column in front of the running score (what HF's top-k / top-p warpers see under beam-sample)
template <bool kTf>
__device__ inline float beam_x(const MhBeamStep& p, const BeamRow& b, const BeamTf& t, float lp, float ln, int v) {
  const MhSampling& sp = p.sp;
  float x = beam_pre(p, b, lp, ln, v);
  if constexpr (kTf) {   // renormalise: log(softmax(x)[v] * s) kept in the log domain; the other rows pass x through, NOT masked
    if (t.renorm) {
      if (v >= sp.ts_start && v < sp.lookback_mask_end) x = v == sp.ts_start ? t.log_extra : -INFINITY;
      else x = (x - t.mc) - t.log_norm;
    }
  } else {
    if (sp.lookback_mask_end > sp.ts_start && v >= sp.ts_start && v < sp.lookback_mask_end) x = -INFINITY;
  }
  return x;
}

template <bool kTf>
__device__ inline float beam_score(const MhBeamStep& p, const BeamRow& b, const BeamTf& t, float lp, float ln, int v) {
  return beam_x<kTf>(p, b, t, lp, ln, v) + b.rs;
}

// ---- beam-sample (kSample instantiations: mh_beam_step_sample) -------------------------------------------------------------------
// HF's TopK / TopP warpers leave every beam row ONE cut value (beam_row_select below): the accumulated score of a column is
// x >= cut ? x + running score : -inf.  THE definition for both kernels, like beam_score.
__device__ inline float beam_warp(float x, float cut, float rs) { return x >= cut ? x + rs : -INFINITY; }

// Gumbel top-K: key = accumulated score + g, g = -log(-log(u)), u = beam_uniform01(sub-seed of (seed, row, column), flat index)
// clamped to 1 - 2^-24 (uniform01 reaches exactly 1.0, where g would be +inf): g lies in [-2.86, 16.64].  A -inf score keeps a -inf
// key.  The K largest keys, best first, ties by ascending flat index, are K draws without replacement in draw order.
// (Every selection pass -- four radix passes, two compaction sweeps -- recomputes the key: one splitmix and two logf per element and
// pass, in both kernels; that is the 0.03 - 0.05 ms a sampled step costs over a greedy one.  Weighed against it: the LDS kernel could
// store the key in `val` once and recompute the score of the K survivors only, as the streaming kernel does.  Not done: the two
// kernels would then no longer share one body per pass, and the pass arithmetic is small beside the step's ~0.5 ms decoder position.)
__device__ inline float beam_key(float acc, uint64_t subseed, int flat) {
  const float u = fminf(beam_uniform01(subseed, (uint32_t)flat), 0x1.fffffep-1f);
  return acc + -logf(-logf(u));
}

__device__ inline float beam_okey_inv(unsigned img) { return __uint_as_float((img & 0x80000000u) ? (img & 0x7fffffffu) : ~img); }

// the types_first state of one beam row from the three reductions over exp(x - mc) -- all columns, the columns outside [ts_start,
// lookback_mask_end), the bit-4 ids (eos + context eos) -- and the slot's state of the previous step.  Returns the slot's next state:
// prob_eos of THIS step's x.  (Rounded operation by operation: the two kernels must agree bit for bit.)
__device__ inline float beam_tf_state(BeamTf& t, bool timed, float prev, float mc, float s_all, float s_other, float s_eos) {
  t.renorm = timed && prev >= 0.f;
  t.mc = mc;
  t.log_norm = t.log_extra = 0.f;
  if (t.renorm) {
    const float prob_eos = prev, prob_event = __fsub_rn(1.f, prob_eos);
    const float sc = __fdiv_rn(1.f, __fadd_rn(__fmul_rn(__fdiv_rn(s_other, s_all), prob_event), prob_eos));
    const float extra = fminf(fmaxf(__fdiv_rn(__fmul_rn(__fsub_rn(sc, 1.f), prob_eos), prob_event), 0.f), 1.f);
    t.log_norm = __fsub_rn(logf(s_all), logf(sc));
    t.log_extra = logf(extra);
  }
  return __fdiv_rn(s_eos, s_all);
}

// bit `bit` of tok_flags for a history id; an input-only id (>= vocab_out) has no flags
__device__ inline bool beam_tok_flag(const MhBeamStep& p, int id, int bit) {
  return id >= 0 && id < p.V && (p.sp.tok_flags[id] & bit) != 0;
}

// where a pass gets the chunk's scores from: the LDS array (kStream = false) or the logits + the beams' BeamRow (kStream = true)
template <bool kStream, bool kTf> struct BeamSrc {
  const MhBeamStep& p;
  const float* val;         // LDS [nb V] (LDS kernel)
  const BeamRow* rows;      // LDS [nb]
  const BeamTf* tf;         // LDS [nb] (kTf)
  const float* lg_pos;      // the chunk's prompt rows of the logits, [nb][V]
  const float* lg_neg;      // ... negative rows (guidance)
  const float* cut;         // LDS [nb] (kSample): the row's cut value
  uint64_t subseed;         // (kSample) beam_rng_subseed(seed, rng_row0 + chunk, cur_len)
};

// what a sweep hands to f: the accumulated score (greedy beams), or under beam-sample the processed score x in front of the warpers,
// the Gumbel key of the warped accumulated score, or that accumulated score itself.  (The LDS array holds x until the cuts are known
// and the accumulated score from then on: BEAM_X sweeps run before, BEAM_KEY / BEAM_ACC sweeps after.)
enum { BEAM_SCORE = 0, BEAM_X = 1, BEAM_KEY = 2, BEAM_ACC = 3 };

// One wave's sweep over columns base0 + lane, + step, ... < end of beam j: f(flat index, score, in range) runs for the WHOLE wave
// (lanes past `end` get in range = false), so f may vote across the wave.  Four columns per lane are loaded before the first is used
// (eight changed the streaming kernel's time by 1 %: it is bound by the 512 threads' arithmetic, not by the loads).
template <int kWhat = BEAM_SCORE, bool kStream, bool kTf, typename F>
__device__ inline void beam_sweep(const BeamSrc<kStream, kTf>& s, int j, int base0, int step, int end, F&& f) {
  const int lane = threadIdx.x & 63, V = s.p.V;
  float cut = 0.f;
  if constexpr (kStream && (kWhat == BEAM_KEY || kWhat == BEAM_ACC)) cut = s.cut[j];
  constexpr int kU = 4;
  BeamRow b;
  BeamTf t{};
  if (kStream) b = s.rows[j];
  if (kStream && kTf) t = s.tf[j];
  for (int vb = base0; vb < end; vb += kU * step) {
    float lp[kU], ln[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int v = vb + u * step + lane;
      lp[u] = ln[u] = 0.f;
      if (v < end) {
        if (kStream) { lp[u] = s.lg_pos[(long)j * V + v]; if (s.p.cfg) ln[u] = s.lg_neg[(long)j * V + v]; }
        else lp[u] = s.val[j * V + v];
      }
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      if (vb + u * step < end) {           // (wave-uniform)
        const int v = vb + u * step + lane;
        const bool ok = v < end;
        if constexpr (kWhat == BEAM_SCORE) {
          const float x = !ok ? 0.f : kStream ? beam_score<kTf>(s.p, b, t, lp[u], ln[u], v) : lp[u];
          f(j * V + v, x, ok);
        } else {
          float x = 0.f;
          if (ok) {
            if constexpr (kStream) {
              x = beam_x<kTf>(s.p, b, t, lp[u], ln[u], v);
              if constexpr (kWhat != BEAM_X) x = beam_warp(x, cut, b.rs);
            } else {
              x = lp[u];
            }
            if constexpr (kWhat == BEAM_KEY) x = beam_key(x, s.subseed, j * V + v);
          }
          f(j * V + v, x, ok);
        }
      }
    }
  }
}

__device__ inline unsigned long long beam_shfl_up_u64(unsigned long long x, int o) {
  const unsigned lo = __shfl_up((unsigned)x, o, 64), hi = __shfl_up((unsigned)(x >> 32), o, 64);
  return ((unsigned long long)hi << 32) | lo;
}
__device__ inline unsigned long long beam_shfl_u64(unsigned long long x, int l) {
  const unsigned lo = __shfl((unsigned)x, l, 64), hi = __shfl((unsigned)(x >> 32), l, 64);
  return ((unsigned long long)hi << 32) | lo;
}

// scratch of beam_row_select, one set per beam row
struct BeamSelect {
  unsigned long long hist[kBeamMaxBeams][256];
  unsigned long long thr[kBeamMaxBeams], below[kBeamMaxBeams];
  unsigned img[kBeamMaxBeams];
  int found[kBeamMaxBeams];
  float row_max[kBeamMaxBeams], floor[kBeamMaxBeams];
};

// Per beam row, all rows at once: the smallest value c of the row's x with W(c) > thr, W(c) = the sum of the integer weights of the
// columns with x <= c -- a radix select from the bottom over the order-preserving image, 8 bits per pass, the 256 bins of row j summed
// up by wave j.  kMass = false: weight 1 per column and thr[j] set by the caller (thr = V - k gives the k-th largest value, ties
// included).  kMass = true: weight = the column's softmax numerator in fixed point, (uint64) (exp(x - row_max[j]) 2^32), 0 for x <
// floor[j] (what TopK removed) -- at most 2^32 each, V < 2^31 of them -- and thr[j] = (uint64) (drop x the row's total), `drop` = 1 -
// top_p in double.  The sums are 64-bit INTEGER adds in LDS: any order gives the same bits, in every launch and in both kernels (a
// float atomicAdd histogram would not).  Out: q.img[j] = image of c, q.found[j] = 0 when no value qualifies (a row without mass).
template <bool kMass, bool kStream, bool kTf>
__device__ inline void beam_row_select(const BeamSrc<kStream, kTf>& s, BeamSelect& q, double drop) {
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, nb = s.p.num_beams, V = s.p.V;
  if (tid < nb) { q.img[tid] = 0u; q.below[tid] = 0ull; q.found[tid] = 1; }
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    const unsigned mask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
    for (int i = tid; i < nb * 256; i += kBeamThreads) q.hist[0][i] = 0ull;
    __syncthreads();
    for (int j = 0; j < nb; ++j) {
      const unsigned prefix = q.img[j];
      const float m = q.row_max[j], fl = q.floor[j];
      beam_sweep<BEAM_X>(s, j, wid * 64, kBeamThreads, V, [&](int, float x, bool ok) {
        const unsigned u = beam_okey(x);
        if (ok && (u & mask) == prefix) {
          unsigned long long w = 1ull;
          if constexpr (kMass) w = (x < fl || x == -INFINITY) ? 0ull : (unsigned long long)(expf(x - m) * 4294967296.f);
          if (w) atomicAdd(&q.hist[j][(u >> shift) & 255], w);
        }
      });
    }
    __syncthreads();
    if (wid < nb) {      // wave j finishes row j: lane l owns bins 4 l .. 4 l + 3, ascending
      const int j = wid;
      unsigned long long h[4], sum = 0ull;
#pragma unroll
      for (int b = 0; b < 4; ++b) { h[b] = q.hist[j][4 * lane + b]; sum += h[b]; }
      unsigned long long inc = sum;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) { const unsigned long long y = beam_shfl_up_u64(inc, o); if (lane >= o) inc += y; }
      unsigned long long thr = q.thr[j];
      if (kMass && pass == 0) thr = (unsigned long long)(drop * (double)beam_shfl_u64(inc, 63));
      unsigned long long acc = q.below[j] + (inc - sum);
      int hit = -1;
      unsigned long long before = 0ull;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        if (hit < 0 && acc + h[b] > thr) { hit = b; before = acc; }
        acc += h[b];
      }
      const unsigned long long votes = __ballot(hit >= 0);
      if (votes == 0ull) { if (lane == 0) q.found[j] = 0; }
      else if (lane == __ffsll((long long)votes) - 1) {
        q.img[j] |= (unsigned)(4 * lane + hit) << shift;
        q.below[j] = before;
      }
      if (kMass && pass == 0 && lane == 0) q.thr[j] = thr;
    }
    __syncthreads();
  }
}

template <bool kStream, bool kTf, bool kSample = false>
__global__ __launch_bounds__(kBeamThreads) void beam_step_kernel(MhBeamStep p, float* lookback_prev, int min_keep, float* scores_dump) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ float red[kBeamThreads / 64];
  __shared__ int s_hist[256];
  __shared__ int s_w[kBeamWaves];
  __shared__ unsigned long long s_w64[kBeamWaves];
  __shared__ unsigned s_prefix;
  __shared__ int s_remaining;
  __shared__ uint8_t s_hit[kBeamMaxK];
  __shared__ int s_sel_run[kBeamMaxBeams], s_sel_fin[kBeamMaxBeams];   // selected candidate / merged-list positions (num_beams <= 8)
  __shared__ float s_run_lp[kBeamMaxBeams], s_fin_sc[kBeamMaxBeams];
  __shared__ BeamRow s_row[kBeamMaxBeams];                          // ltv: value of the last TIME_SHIFT after the last SOS (-1: none)
  __shared__ BeamTf s_tf[kBeamMaxBeams];                            // (kTf)
  __shared__ uint8_t s_timed[kBeamMaxBeams];                        // (kTf) the beam's last id is a timed event
  __shared__ int s_seg_above[kBeamMaxBeams * kBeamWaves], s_seg_ties[kBeamMaxBeams * kBeamWaves];   // compaction: per (beam, wave) slice
  __shared__ BeamSelect s_select;                                   // (kSample) the warpers' per-row selects
  __shared__ float s_cut[kBeamMaxBeams], s_cut_k[kBeamMaxBeams];    // (kSample) the row's cut value; TopK's part of it
  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int nb = p.num_beams, V = p.V, T = p.cur_len, L = p.max_length, R = p.G * nb;
  const MhSampling& sp = p.sp;
  const int n = nb * V;
  int k_pad = 1;
  while (k_pad < p.K) k_pad <<= 1;
  float* val = reinterpret_cast<float*>(smem);                                   // LDS kernel: [n] accumulated scores, flat index j * V + v
  BeamKV* arr = reinterpret_cast<BeamKV*>(smem + (kStream ? 0 : (((size_t)n * 4 + 15) & ~(size_t)15)));   // [k_pad] the K best, sorted
  const float* lg_pos_g = p.logits + (long)(p.cfg ? R + g * nb : g * nb) * V;    // under guidance the prompt rows are the SECOND half
  const float* lg_neg_g = p.logits + (long)g * nb * V;
  const BeamSrc<kStream, kTf> scores{p, val, s_row, s_tf, lg_pos_g, lg_neg_g, s_cut,
                                     kSample ? beam_rng_subseed(sp.seed, sp.rng_row0 + (uint32_t)g, (uint32_t)T) : 0ull};
  constexpr int kSel = kSample ? BEAM_KEY : BEAM_SCORE;             // what the selection below ranks

  // ---- per-beam processor state from the beam's own sequence: MonotonicTimeShiftLogitsProcessor (logit_processors.py:136-183)
  // and the (Conditional)Temperature of the step (:47-82; row 0 of the WHOLE call picks it unless cond_per_row) ------------------
  for (int j = wid; j < nb; j += kBeamThreads / 64) {
    const int32_t* ids = p.run_in + ((long)g * nb + j) * L;
    int last_ts = -1, last_sos = -1;
    for (int i0 = 0; i0 < T; i0 += 64) {
      const int i = i0 + lane;
      const int id = i < T ? ids[i] : -1;
      const bool is_ts = i < T && id >= sp.ts_start && id < sp.ts_end;
      bool is_sos = false;
      for (int q = 0; q < sp.n_sos; ++q) is_sos |= (i < T && id == sp.sos_ids[q]);
      int a = is_ts ? i : -1, b = is_sos ? i : -1;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) { a = max(a, __shfl_xor(a, o, 64)); b = max(b, __shfl_xor(b, o, 64)); }
      last_ts = max(last_ts, a);
      last_sos = max(last_sos, b);
    }
    if (lane == 0) {
      s_row[j].ltv = (sp.ts_end > sp.ts_start && last_ts != -1 && last_ts > last_sos) ? ids[last_ts] - sp.ts_start : -1;
      float temp = sp.temperature;
      const int32_t* hist = sp.cond_per_row ? ids : p.run_in;       // (row 0 of the call = chunk 0, beam 0)
      for (int q = 0; q < sp.n_cond; ++q) {
        const int off = sp.cond_offset[q];
        if (T >= off && beam_tok_flag(p, hist[T - off], 2 << q)) { temp = sp.cond_temp[q]; break; }
      }
      s_row[j].temp = temp;
      s_row[j].rs = p.rs_in[g * nb + j];
      if constexpr (kTf) s_timed[j] = beam_tok_flag(p, ids[T - 1], 1) ? 1 : 0;
    }
  }
  __syncthreads();

  // ---- log_softmax state per beam (both kernels: thread tid reduces columns tid, tid + 512, ... in ascending order, then block_max /
  // block_sum, so a row's maximum and log-sum-exp have the same bits in both) ------------------------------------------------------
  if constexpr (kStream) {
    // all beams in ONE sweep for the maxima and one for the sums: the loads of a column's 2 .. 16 rows are independent
    float mp[kBeamMaxBeams], mn[kBeamMaxBeams], sp_[kBeamMaxBeams], sn_[kBeamMaxBeams];
#pragma unroll
    for (int j = 0; j < kBeamMaxBeams; ++j) { mp[j] = mn[j] = -INFINITY; sp_[j] = sn_[j] = 0.f; }
    for (int v = tid; v < V; v += kBeamThreads) {
#pragma unroll
      for (int j = 0; j < kBeamMaxBeams; ++j)
        if (j < nb) { mp[j] = fmaxf(mp[j], lg_pos_g[(long)j * V + v]); if (p.cfg) mn[j] = fmaxf(mn[j], lg_neg_g[(long)j * V + v]); }
    }
#pragma unroll
    for (int j = 0; j < kBeamMaxBeams; ++j)
      if (j < nb) { mp[j] = block_max(mp[j], red); if (p.cfg) mn[j] = block_max(mn[j], red); }
    for (int v = tid; v < V; v += kBeamThreads) {
#pragma unroll
      for (int j = 0; j < kBeamMaxBeams; ++j)
        if (j < nb) { sp_[j] += expf(lg_pos_g[(long)j * V + v] - mp[j]); if (p.cfg) sn_[j] += expf(lg_neg_g[(long)j * V + v] - mn[j]); }
    }
#pragma unroll
    for (int j = 0; j < kBeamMaxBeams; ++j)
      if (j < nb) {
        sp_[j] = block_sum(sp_[j], red);
        if (p.cfg) sn_[j] = block_sum(sn_[j], red);
        if (tid == 0) { s_row[j].mp = mp[j]; s_row[j].lse_p = logf(sp_[j]); s_row[j].mn = mn[j]; s_row[j].lse_n = p.cfg ? logf(sn_[j]) : 0.f; }
      }
    __syncthreads();
    if constexpr (kTf) {
      // the three reductions of the types_first lookback over x = beam_pre(): per beam, same thread -> column order as the LDS kernel
      for (int j = 0; j < nb; ++j) {
        const BeamRow b = s_row[j];
        float mc = -INFINITY;
        for (int v = tid; v < V; v += kBeamThreads)
          mc = fmaxf(mc, beam_pre(p, b, lg_pos_g[(long)j * V + v], p.cfg ? lg_neg_g[(long)j * V + v] : 0.f, v));
        mc = block_max(mc, red);
        float s_all = 0.f, s_other = 0.f, s_eos = 0.f;
        for (int v = tid; v < V; v += kBeamThreads) {
          const float e = expf(beam_pre(p, b, lg_pos_g[(long)j * V + v], p.cfg ? lg_neg_g[(long)j * V + v] : 0.f, v) - mc);
          s_all += e;
          if (!(v >= sp.ts_start && v < sp.lookback_mask_end)) s_other += e;
          if (sp.tok_flags[v] & 16) s_eos += e;
        }
        s_all = block_sum(s_all, red);
        s_other = block_sum(s_other, red);
        s_eos = block_sum(s_eos, red);
        if (tid == 0) {
          const int slot = g * nb + j;
          lookback_prev[slot] = beam_tf_state(s_tf[j], s_timed[j] != 0, lookback_prev[slot], mc, s_all, s_other, s_eos);
        }
      }
      __syncthreads();
    }
  } else {
    // ---- log_softmax (+ guidance) + processors + running score -> val[] ------------------------------------------------------
    // the prompt rows' logits are staged in LDS once (one round of independent loads); the per-beam maximum / sum then read LDS in
    // the same thread -> column order as before, so the reductions keep their bits
    for (int i = tid; i < n; i += kBeamThreads) val[i] = lg_pos_g[i];
    __syncthreads();
    for (int j = 0; j < nb; ++j) {
      float* lg_pos = val + j * V;
      const float* lg_neg = lg_neg_g + (long)j * V;
      float mp = -INFINITY, mn = -INFINITY;
      for (int v = tid; v < V; v += kBeamThreads) { mp = fmaxf(mp, lg_pos[v]); if (p.cfg) mn = fmaxf(mn, lg_neg[v]); }
      mp = block_max(mp, red);
      if (p.cfg) mn = block_max(mn, red);
      float sp_ = 0.f, sn_ = 0.f;
      for (int v = tid; v < V; v += kBeamThreads) { sp_ += expf(lg_pos[v] - mp); if (p.cfg) sn_ += expf(lg_neg[v] - mn); }
      sp_ = block_sum(sp_, red);
      if (p.cfg) sn_ = block_sum(sn_, red);
      const BeamRow b{mp, logf(sp_), mn, p.cfg ? logf(sn_) : 0.f, s_row[j].temp, s_row[j].rs, s_row[j].ltv};
      BeamTf t{};
      if constexpr (kTf) {   // the types_first lookback's three reductions over x = beam_pre() (the logits stay in LDS for beam_score)
        float mc = -INFINITY;
        for (int v = tid; v < V; v += kBeamThreads) mc = fmaxf(mc, beam_pre(p, b, lg_pos[v], p.cfg ? lg_neg[v] : 0.f, v));
        mc = block_max(mc, red);
        float s_all = 0.f, s_other = 0.f, s_eos = 0.f;
        for (int v = tid; v < V; v += kBeamThreads) {
          const float e = expf(beam_pre(p, b, lg_pos[v], p.cfg ? lg_neg[v] : 0.f, v) - mc);
          s_all += e;
          if (!(v >= sp.ts_start && v < sp.lookback_mask_end)) s_other += e;
          if (sp.tok_flags[v] & 16) s_eos += e;
        }
        s_all = block_sum(s_all, red);
        s_other = block_sum(s_other, red);
        s_eos = block_sum(s_eos, red);
        const int slot = g * nb + j;
        const float next = beam_tf_state(t, s_timed[j] != 0, lookback_prev[slot], mc, s_all, s_other, s_eos);   // (every thread: same inputs)
        __syncthreads();                                  // ... all have read the slot
        if (tid == 0) lookback_prev[slot] = next;
      }
      for (int v = tid; v < V; v += kBeamThreads) {     // (each thread rewrites exactly the columns it read)
        if constexpr (kSample) lg_pos[v] = beam_x<kTf>(p, b, t, lg_pos[v], p.cfg ? lg_neg[v] : 0.f, v);   // (+ running score: below)
        else lg_pos[v] = beam_score<kTf>(p, b, t, lg_pos[v], p.cfg ? lg_neg[v] : 0.f, v);
      }
    }
    __syncthreads();
  }

  // ---- beam-sample: HF's TopKLogitsWarper, then TopPLogitsWarper (min_tokens_to_keep = min_keep), per beam row on x, as ONE cut value
  // per row: cut = max(k'-th largest x, min(smallest x whose mass of values <= it exceeds 1 - top_p, min_keep-th largest x)) --------
  if constexpr (kSample) {
    const int keep = min(min_keep, V);
    const bool top_k_on = sp.top_k > 0, top_p_on = sp.top_p < 1.0f;
    if (tid < nb) { s_cut_k[tid] = -INFINITY; s_cut[tid] = -INFINITY; s_select.thr[tid] = (unsigned long long)(V - min(max(sp.top_k, keep), V)); }
    if (top_k_on) {
      beam_row_select<false>(scores, s_select, 0.0);
      if (tid < nb) { s_cut_k[tid] = beam_okey_inv(s_select.img[tid]); s_cut[tid] = s_cut_k[tid]; }
    }
    if (top_p_on) {
      __syncthreads();
      for (int j = 0; j < nb; ++j) {         // the row's maximum (TopK keeps it)
        float m = -INFINITY;
        beam_sweep<BEAM_X>(scores, j, wid * 64, kBeamThreads, V, [&](int, float x, bool ok) { if (ok) m = fmaxf(m, x); });
        m = block_max(m, red);
        if (tid == 0) { s_select.row_max[j] = m; s_select.floor[j] = s_cut_k[j]; s_select.thr[j] = (unsigned long long)(V - keep); }
      }
      beam_row_select<false>(scores, s_select, 0.0);      // the min_keep-th largest x
      float cut_keep = 0.f;
      if (tid < nb) cut_keep = beam_okey_inv(s_select.img[tid]);
      beam_row_select<true>(scores, s_select, 1.0 - (double)sp.top_p);
      if (tid < nb) {
        const float cut_p = s_select.found[tid] ? beam_okey_inv(s_select.img[tid]) : -INFINITY;
        s_cut[tid] = fmaxf(s_cut_k[tid], fminf(cut_p, cut_keep));
      }
    }
    __syncthreads();
    if constexpr (!kStream) {      // x -> accumulated score, in place
      for (int i = tid; i < n; i += kBeamThreads) { const int j = i / V; val[i] = beam_warp(val[i], s_cut[j], s_row[j].rs); }
      __syncthreads();
    }
    if (scores_dump)
      for (int j = 0; j < nb; ++j)
        beam_sweep<BEAM_ACC>(scores, j, wid * 64, kBeamThreads, V, [&](int i, float x, bool ok) { if (ok) scores_dump[(long)g * n + i] = x; });
  }

  // ---- the K best of the chunk's num_beams x V accumulated scores, best first, ties by ascending flat index ----------------------
  // (1) radix select of the K-th largest value on the order-preserving integer image of the floats, 8 bits per pass
  const int K = p.K;
  if (tid == 0) { s_prefix = 0u; s_remaining = K; }
  __syncthreads();
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    const unsigned mask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
    if (tid < 256) s_hist[tid] = 0;
    __syncthreads();
    const unsigned prefix = s_prefix;
    const int rem = s_remaining;
    for (int j = 0; j < nb; ++j)
      beam_sweep<kSel>(scores, j, wid * 64, kBeamThreads, V, [&](int, float x, bool ok) {
        const unsigned u = beam_okey(x);
        if (ok && (u & mask) == prefix) atomicAdd(&s_hist[(u >> shift) & 255], 1);
      });
    __syncthreads();
    // thread t owns bin 255 - t: the bin where the count from the top first reaches `rem` holds the K-th value
    const int h = tid < 256 ? s_hist[255 - tid] : 0;
    int tot;
    const int before = beam_excl_scan(h, s_w, tot);
    if (tid < 256 && before < rem && before + h >= rem) {      // exactly one thread (the candidates still in play number >= rem)
      s_remaining = rem - before;                               // how many of the elements inside this bin are still wanted
      s_prefix = prefix | ((unsigned)(255 - tid) << shift);
    }
    __syncthreads();
  }
  const unsigned kth = s_prefix;                 // integer image of the K-th largest value; s_remaining of its ties are wanted
  const int want_ties = s_remaining;
  // (2) compaction: everything above the K-th value, then the `want_ties` ties of SMALLEST flat index.  Wave w owns the columns
  //     [w Vw, (w + 1) Vw) of every beam and walks them 64 at a time, so (beam, wave) slices are in flat-index order: the slices'
  //     counts are scanned by one wave, and inside a slice a wave-wide vote ranks the 64 columns of a round.  (Where the values above
  //     the K-th land among themselves does not matter: the sort below orders them by (value, flat index), a total order.)
  const int Vw = (((V + kBeamWaves - 1) / kBeamWaves) + 63) & ~63;
  const int v_lo = min(wid * Vw, V), v_hi = min(v_lo + Vw, V);
  for (int j = 0; j < nb; ++j) {
    int above = 0, ties = 0;
    beam_sweep<kSel>(scores, j, v_lo, 64, v_hi, [&](int, float x, bool ok) {
      const unsigned u = beam_okey(x);
      above += ok && u > kth;
      ties += ok && u == kth;
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { above += __shfl_xor(above, o, 64); ties += __shfl_xor(ties, o, 64); }
    if (lane == 0) { s_seg_above[j * kBeamWaves + wid] = above; s_seg_ties[j * kBeamWaves + wid] = ties; }
  }
  __syncthreads();
  if (wid == 0) {      // exclusive scan over the nb x 8 slices (<= 64: one per lane)
    const bool in = lane < nb * kBeamWaves;
    const int a = in ? s_seg_above[lane] : 0, t = in ? s_seg_ties[lane] : 0;
    int ia = a, it = t;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int ya = __shfl_up(ia, o, 64), yt = __shfl_up(it, o, 64);
      if (lane >= o) { ia += ya; it += yt; }
    }
    if (in) { s_seg_above[lane] = ia - a; s_seg_ties[lane] = it - t; }
  }
  __syncthreads();
  const int n_above = K - want_ties;
  const unsigned long long lanes_below = (1ull << lane) - 1ull;
  for (int j = 0; j < nb; ++j) {
    int wpos = s_seg_above[j * kBeamWaves + wid], trank = s_seg_ties[j * kBeamWaves + wid];
    beam_sweep<kSel>(scores, j, v_lo, 64, v_hi, [&](int i, float x, bool ok) {
      const unsigned u = beam_okey(x);
      const bool is_above = ok && u > kth, is_tie = ok && u == kth;
      const unsigned long long m_above = __ballot(is_above), m_tie = __ballot(is_tie);
      const int pa = wpos + __popcll(m_above & lanes_below), pt = trank + __popcll(m_tie & lanes_below);
      if (is_above && pa < n_above) arr[pa] = BeamKV{x, i};
      if (is_tie && pt < want_ties) arr[n_above + pt] = BeamKV{x, i};
      wpos += __popcll(m_above);
      trank += __popcll(m_tie);
    });
  }
  for (int i = K + tid; i < k_pad; i += kBeamThreads) arr[i] = BeamKV{-INFINITY, 0x7fffffff};
  __syncthreads();
  // (3) bitonic sort of the K candidates
  for (int k = 2; k <= k_pad; k <<= 1) {
    for (int jj = k >> 1; jj > 0; jj >>= 1) {
      for (int t = tid; t < k_pad / 2; t += kBeamThreads) {
        const int i = ((t / jj) * 2 * jj) + (t % jj), ixj = i + jj;
        const bool up = (i & k) == 0;                    // this block sorts "best first"
        const BeamKV a = arr[i], b = arr[ixj];
        if (up ? beam_before(b, a) : beam_before(a, b)) { arr[i] = b; arr[ixj] = a; }
      }
      __syncthreads();
    }
  }
  if constexpr (kSample) {      // the K draws, in draw order: each key gives way to its accumulated score (read back / recomputed, not key - g)
    for (int k = tid; k < K; k += kBeamThreads) {
      const int i = arr[k].i;
      float acc;
      if constexpr (kStream) {
        const int j = i / V, v = i - j * V;
        const BeamRow b = s_row[j];
        BeamTf t{};
        if constexpr (kTf) t = s_tf[j];
        acc = beam_warp(beam_x<kTf>(p, b, t, lg_pos_g[(long)j * V + v], p.cfg ? lg_neg_g[(long)j * V + v] : 0.f, v), s_cut[j], b.rs);
      } else {
        acc = val[i];
      }
      arr[k].v = acc;
    }
    __syncthreads();
  }

  // ---- stopping criteria on the K best candidates (d.) ------------------------------------------------------------------------
  const bool at_max = T + 1 >= L;
  for (int k = tid; k < K; k += kBeamThreads) s_hit[k] = (at_max || p.eos_table[arr[k].i % V]) ? 1 : 0;
  __syncthreads();

  // e. the running beams of the next step: the num_beams best of run_lp = lp + hit * -1e9 (best first, ties by position).  One
  //    block-wide maximum per beam over (score, position) keys -- the serial insertion of the first version cost ~25 ns per candidate
  {
    unsigned long long prev = ~0ull;
    for (int s = 0; s < nb; ++s) {
      unsigned long long best = 0ull;
      for (int k = tid; k < K; k += kBeamThreads) {
        const float rl = arr[k].v + (s_hit[k] ? -1.0e9f : -0.0f);
        const unsigned long long key = beam_rank_key(rl, k);
        if (key < prev && key > best) best = key;
      }
      best = beam_max_u64(best, s_w64);
      prev = best;
      if (tid == 0) {
        const int k = 0x7fffffff - (int)(unsigned)(best & 0xffffffffu);
        s_sel_run[s] = k;
        s_run_lp[s] = arr[k].v + (s_hit[k] ? -1.0e9f : -0.0f);
      }
    }
  }
  // f. finished hypotheses: only candidates inside the top num_beams count; merged with the chunk's finished set by score
  {
    bool all_fin_in = true;
    for (int s = 0; s < nb; ++s) all_fin_in &= p.fin_in[g * nb + s] != 0;
    const bool full = all_fin_in && p.early_stopping == 1;
    const bool open_in = p.heuristic_open[g] != 0;
    const float div = (float)pow((double)(T + 1 - p.P), (double)p.length_penalty);
    auto merged_score = [&](int m) -> float {        // merged list: the nb old slots, then the K candidates
      if (m < nb) return p.bs_in[g * nb + m];
      const int k = m - nb;
      const bool just = s_hit[k] && k < nb;
      float sc = arr[k].v / div;
      sc = sc + (full ? -1.0e9f : -0.0f);
      sc = sc + (!open_in ? -1.0e9f : -0.0f);
      sc = sc + (!just ? -1.0e9f : -0.0f);
      return sc;
    };
    unsigned long long prev = ~0ull;
    for (int s = 0; s < nb; ++s) {
      unsigned long long best = 0ull;
      for (int m = tid; m < nb + K; m += kBeamThreads) {
        const unsigned long long key = beam_rank_key(merged_score(m), m);
        if (key < prev && key > best) best = key;
      }
      best = beam_max_u64(best, s_w64);
      prev = best;
      if (tid == 0) {
        const int m = 0x7fffffff - (int)(unsigned)(best & 0xffffffffu);
        s_sel_fin[s] = m;
        s_fin_sc[s] = merged_score(m);
      }
    }
  }
  __syncthreads();

  // ---- write the OUT state: rows are copied from the IN state (parents' running rows / old finished slots); every element of the
  // four arrays is one independent load -> store -------------------------------------------------------------------------------
  const int n_new = L - p.P;
  for (int e = tid; e < nb * L; e += kBeamThreads) {
    const int s = e / L, i = e - s * L;
    const int flat = arr[s_sel_run[s]].i, parent = flat / V, tok = flat % V;
    const int a = i == T ? tok : p.run_in[((long)g * nb + parent) * L + i];
    const int m = s_sel_fin[s];
    int b;
    if (m < nb) b = p.seq_in[((long)g * nb + m) * L + i];
    else {
      const int flat2 = arr[m - nb].i, par2 = flat2 / V, tok2 = flat2 % V;
      b = i == T ? tok2 : p.run_in[((long)g * nb + par2) * L + i];
    }
    p.run_out[((long)g * nb + s) * L + i] = a;
    p.seq_out[((long)g * nb + s) * L + i] = b;
  }
  for (int e = tid; e < nb * n_new; e += kBeamThreads) {
    const int s = e / n_new, i = e - s * n_new;
    const int parent = arr[s_sel_run[s]].i / V;
    const int a = i == T - p.P ? parent + g * nb : p.rb_in[((long)g * nb + parent) * n_new + i];
    const int m = s_sel_fin[s];
    int b;
    if (m < nb) b = p.bb_in[((long)g * nb + m) * n_new + i];
    else {
      const int par2 = arr[m - nb].i / V;
      b = i == T - p.P ? par2 + g * nb : p.rb_in[((long)g * nb + par2) * n_new + i];
    }
    p.rb_out[((long)g * nb + s) * n_new + i] = a;
    p.bb_out[((long)g * nb + s) * n_new + i] = b;
  }
  if (tid < nb) {
    const int s = tid;
    const int flat = arr[s_sel_run[s]].i, parent = flat / V, tok = flat % V;
    p.rs_out[g * nb + s] = s_run_lp[s];
    p.src[g * nb + s] = parent + g * nb;             // g. the cache rows follow the beams that keep running
    p.last[g * nb + s] = tok;
    if (p.cfg) {   // `beam_idx.repeat(2)` (cache_utils.py:18): BOTH halves gather from the first half, and both are fed the beam's token
      p.src[R + g * nb + s] = parent + g * nb;
      p.last[R + g * nb + s] = tok;
    }
    const int m = s_sel_fin[s];
    p.fin_out[g * nb + s] = m < nb ? p.fin_in[g * nb + m] : ((s_hit[m - nb] && (m - nb) < nb) ? 1 : 0);
    p.bs_out[g * nb + s] = s_fin_sc[s];
  }

  // ---- "can a running beam still beat the worst finished one" (early_stopping = False heuristic) + the flags the host polls ----
  int my_hit = 1;
  for (int k = tid; k < K; k += kBeamThreads) my_hit &= s_hit[k] != 0;
  const bool all_hit = __syncthreads_and(my_hit) != 0;
  if (tid == 0) {
    const int hyp_len = (p.early_stopping == 2 && p.length_penalty > 0.f) ? L - p.P : T + 1 - p.P;
    const float best_running = s_run_lp[0] / (float)pow((double)hyp_len, (double)p.length_penalty);
    float mn = INFINITY;
    bool all_fin = true;
    for (int s = 0; s < nb; ++s) mn = fminf(mn, s_fin_sc[s]);
    bool any = false;
    for (int s = 0; s < nb; ++s) {
      const int m = s_sel_fin[s];
      const bool f = m < nb ? p.fin_in[g * nb + m] != 0 : (s_hit[m - nb] && (m - nb) < nb);
      all_fin &= f;
      any |= best_running > (f ? mn : -1.0e9f);
    }
    const bool open = (p.heuristic_open[g] != 0) && any;
    p.heuristic_open[g] = open ? 1 : 0;
    p.flags[g * 3 + 0] = open; p.flags[g * 3 + 1] = all_hit; p.flags[g * 3 + 2] = all_fin;
  }
}

}  // namespace
}  // namespace mh

using namespace mh;

extern "C" int64_t mh_beam_step_lds_bytes(int num_beams, int V) {      // the score array; mh_beam_step adds the K candidates itself
  if (num_beams < 1 || V < 1) return -1;
  return (((int64_t)num_beams * V * 4 + 15) & ~(int64_t)15);
}

// which kernel a step of this shape runs under the option "beam_step_path" (0 = the LDS kernel wherever it fits, else the streaming
// one; 1 = the LDS kernel or nothing; 2 = the streaming kernel): 0 = refused, 1 = LDS, 2 = streaming
extern "C" int mh_beam_step_path(int num_beams, int V, int K) {
  if (num_beams < 2 || num_beams > kBeamMaxBeams || V < 1 || K < num_beams || K > kBeamMaxK || K > (int64_t)num_beams * V) return 0;
  const long want = option(OPT_BEAM_STEP_PATH);
  if (want == 2) return 2;
  int64_t k_pad = 1;
  while (k_pad < K) k_pad <<= 1;
  const bool fits = K <= kBeamLdsMaxK && mh_beam_step_lds_bytes(num_beams, V) + k_pad * 8 <= kBeamLdsBytes;
  return fits ? 1 : want == 1 ? 0 : 2;
}

// mh_beam_step (lookback_prev = nullptr, `tf` false), mh_beam_step_tf and mh_beam_step_sample: one set of checks, one dispatch rule
static int beam_step_launch(const char* who, const MhBeamStep* bs, float* lookback_prev, bool tf_entry, void* stream,
                            bool sample_entry = false, int min_keep = 0, float* scores_dump = nullptr) {
  MH_REQUIRE(bs && bs->logits && bs->eos_table && bs->run_in && bs->run_out && bs->rs_in && bs->rs_out && bs->rb_in && bs->rb_out &&
             bs->seq_in && bs->seq_out && bs->bs_in && bs->bs_out && bs->bb_in && bs->bb_out && bs->fin_in && bs->fin_out &&
             bs->heuristic_open && bs->src && bs->last && bs->flags, "%s: null argument", who);
  MH_REQUIRE(bs->G >= 1 && bs->V >= 1 && bs->num_beams >= 2 && bs->num_beams <= kBeamMaxBeams, "%s: %d chunks x %d beams (2 .. %d beams)", who, bs->G, bs->num_beams, kBeamMaxBeams);
  MH_REQUIRE(bs->K >= bs->num_beams && bs->K <= kBeamMaxK && bs->K <= (int64_t)bs->num_beams * bs->V, "%s: K = %d candidates not in [num_beams, %d]", who, bs->K, kBeamMaxK);
  MH_REQUIRE(bs->P >= 1 && bs->cur_len >= bs->P && bs->cur_len < bs->max_length, "%s: cur_len %d not in [P, max_length)", who, bs->cur_len);
  if (sample_entry) {
    MH_REQUIRE(bs->sp.do_sample != 0, "%s: do_sample = %d: the sampled step needs do_sample = 1 (greedy beams are mh_beam_step)", who, bs->sp.do_sample);
    MH_REQUIRE(min_keep >= 1, "%s: min_tokens_to_keep = %d (at least 1)", who, min_keep);
    MH_REQUIRE(bs->sp.top_p > 0.f && bs->sp.top_p <= 1.f, "%s: top_p = %g outside (0, 1]", who, (double)bs->sp.top_p);
    MH_REQUIRE(bs->sp.top_k >= 0, "%s: top_k = %d is negative", who, bs->sp.top_k);
  } else {
    MH_REQUIRE(bs->sp.do_sample == 0, "%s: greedy beams only (beam-sample is mh_beam_step_sample)", who);
  }
  const bool tf = bs->sp.lookback_types_first && bs->sp.lookback_mask_end > bs->sp.ts_start;
  MH_REQUIRE(!tf || tf_entry, "%s: the types_first lookback renormalisation is not built for beams", who);
  MH_REQUIRE(!tf || lookback_prev, "%s: the types_first lookback renormalisation needs lookback_prev", who);
  MH_REQUIRE(!tf || bs->sp.tok_flags, "%s: the types_first lookback renormalisation needs tok_flags", who);
  MH_REQUIRE(!tf || bs->sp.lookback_mask_end <= bs->V, "%s: lookback_mask_end %d beyond the vocabulary (%d)", who, bs->sp.lookback_mask_end, bs->V);
  MH_REQUIRE(bs->sp.tok_flags || bs->sp.n_cond == 0, "%s: conditional temperature needs tok_flags", who);
  MH_REQUIRE(bs->sp.temperature > 0.f && bs->sp.n_sos >= 0 && bs->sp.n_sos <= 16 && bs->sp.n_cond >= 0 && bs->sp.n_cond <= 3, "%s: bad sampling parameters", who);
  MH_REQUIRE((int64_t)bs->num_beams * bs->V <= 0x7fffffff, "%s: num_beams x V = %d x %d exceeds the 31-bit flat index", who, bs->num_beams, bs->V);
  const int path = mh_beam_step_path(bs->num_beams, bs->V, bs->K);
  MH_REQUIRE(path != 0, "%s: num_beams x V = %d x %d (+ %d candidates) does not fit the LDS kernel (120 KB of LDS, K <= %d) and beam_step_path = 1 rules the streaming kernel out",
             who, bs->num_beams, bs->V, bs->K, kBeamLdsMaxK);
  int64_t k_pad = 1;
  while (k_pad < bs->K) k_pad <<= 1;
  static PerDeviceOnce attr_set;
  const int arc = attr_set.run([] {
    auto set = [](const void* f, int bytes) { return hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess; };
    return set(reinterpret_cast<const void*>(beam_step_kernel<false, false>), kBeamLdsBytes) &&
                   set(reinterpret_cast<const void*>(beam_step_kernel<true, false>), kBeamMaxK * 8) &&
                   set(reinterpret_cast<const void*>(beam_step_kernel<false, true>), kBeamLdsBytes) &&
                   set(reinterpret_cast<const void*>(beam_step_kernel<true, true>), kBeamMaxK * 8) &&
                   set(reinterpret_cast<const void*>(beam_step_kernel<false, false, true>), kBeamLdsBytes) &&
                   set(reinterpret_cast<const void*>(beam_step_kernel<true, false, true>), kBeamMaxK * 8) &&
                   set(reinterpret_cast<const void*>(beam_step_kernel<false, true, true>), kBeamLdsBytes) &&
                   set(reinterpret_cast<const void*>(beam_step_kernel<true, true, true>), kBeamMaxK * 8)
               ? MH_OK : check_launch("mh_beam_step: LDS attribute");
  });
  if (arc != MH_OK) return arc;
  const size_t lds = path == 1 ? (size_t)(mh_beam_step_lds_bytes(bs->num_beams, bs->V) + k_pad * 8) : (size_t)(k_pad * 8);
  const dim3 grid(bs->G), block(kBeamThreads);
  const hipStream_t st = (hipStream_t)stream;
  if (sample_entry) {
    if (path == 1) {
      if (tf) hipLaunchKernelGGL((beam_step_kernel<false, true, true>), grid, block, lds, st, *bs, lookback_prev, min_keep, scores_dump);
      else hipLaunchKernelGGL((beam_step_kernel<false, false, true>), grid, block, lds, st, *bs, lookback_prev, min_keep, scores_dump);
      return check_launch(tf ? "beam_step_kernel<lds, types_first, sample>" : "beam_step_kernel<lds, sample>");
    }
    if (tf) hipLaunchKernelGGL((beam_step_kernel<true, true, true>), grid, block, lds, st, *bs, lookback_prev, min_keep, scores_dump);
    else hipLaunchKernelGGL((beam_step_kernel<true, false, true>), grid, block, lds, st, *bs, lookback_prev, min_keep, scores_dump);
    return check_launch(tf ? "beam_step_kernel<streaming, types_first, sample>" : "beam_step_kernel<streaming, sample>");
  }
  if (path == 1) {
    if (tf) hipLaunchKernelGGL((beam_step_kernel<false, true>), grid, block, lds, st, *bs, lookback_prev, 0, (float*)nullptr);
    else hipLaunchKernelGGL((beam_step_kernel<false, false>), grid, block, lds, st, *bs, lookback_prev, 0, (float*)nullptr);
    return check_launch(tf ? "beam_step_kernel<lds, types_first>" : "beam_step_kernel<lds>");
  }
  if (tf) hipLaunchKernelGGL((beam_step_kernel<true, true>), grid, block, lds, st, *bs, lookback_prev, 0, (float*)nullptr);
  else hipLaunchKernelGGL((beam_step_kernel<true, false>), grid, block, lds, st, *bs, lookback_prev, 0, (float*)nullptr);
  return check_launch(tf ? "beam_step_kernel<streaming, types_first>" : "beam_step_kernel<streaming>");
}

extern "C" int mh_beam_step(const MhBeamStep* bs, void* stream) { return beam_step_launch("mh_beam_step", bs, nullptr, false, stream); }

extern "C" int mh_beam_step_tf(const MhBeamStep* bs, float* lookback_prev, void* stream) {
  return beam_step_launch("mh_beam_step_tf", bs, lookback_prev, true, stream);
}

extern "C" int mh_beam_step_sample(const MhBeamStep* bs, float* lookback_prev, int min_tokens_to_keep, float* scores_dump, void* stream) {
  return beam_step_launch("mh_beam_step_sample", bs, lookback_prev, true, stream, true, min_tokens_to_keep, scores_dump);
}
