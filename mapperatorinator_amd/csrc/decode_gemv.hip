// The token step's GEMVs: the ONE unit that instantiates gemv_kernel and dec_tail_kernel (decode_gemv.hpp), and their launchers.
// The other units reach them through launch_gemv / tail_covers / launch_tail (decode_step.hpp).
#include <algorithm>
#include <atomic>

#include "decode_gemv.hpp"
#include "decode_step.hpp"

namespace mh {
namespace {

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

// ---- the plain launch functions (contracts in decode_step.hpp): the forms a step uses, and no other ---------------------------------
int launch_gemv(int dtype, int pro, int epi, bool bias, const dec::SkinnyP& p, hipStream_t s) {
  return dispatch_dtype(dtype, [&](auto t) -> int {
    using T = decltype(t);
    if (pro == dec::PRO_PLAIN && epi == dec::SK_RESID) return bias ? skinny<T, dec::PRO_PLAIN, dec::SK_RESID, true>(p, s) : skinny<T, dec::PRO_PLAIN, dec::SK_RESID>(p, s);
    if (pro == dec::PRO_RMSNORM && epi == dec::SK_GEGLU && !bias) return skinny<T, dec::PRO_RMSNORM, dec::SK_GEGLU>(p, s);
    if (pro == dec::PRO_LAYERNORM && epi == dec::SK_GELU_ERF && bias) return skinny<T, dec::PRO_LAYERNORM, dec::SK_GELU_ERF, true>(p, s);
    if (pro == dec::PRO_RMSNORM && epi == dec::SK_GELU_ERF && bias) return skinny<T, dec::PRO_RMSNORM, dec::SK_GELU_ERF, true>(p, s);
    if (pro == dec::PRO_LAYERNORM && epi == dec::SK_LOGITS && !bias) return skinny<T, dec::PRO_LAYERNORM, dec::SK_LOGITS>(p, s);
    if (pro == dec::PRO_RMSNORM && epi == dec::SK_LOGITS && !bias) return skinny<T, dec::PRO_RMSNORM, dec::SK_LOGITS>(p, s);
    set_error("decode: no GEMV kernel with prologue %d, epilogue %d, bias %d", pro, epi, (int)bias);
    return MH_ERR_ARG;
  });
}

bool tail_covers(const MhT5Config* c, int B, bool wh, const float* b_o, const float* b_fc1, const float* b_fc2) {
  return dispatch_dtype(c->dtype, [&](auto t) { return tail_covers<decltype(t)>(c, B, wh, b_o, b_fc1, b_fc2); });
}

int launch_tail(int dtype, int prowi, int epiwi, bool bias, const dec::TailP& p, DecState* st, int layer, int n_chains, hipStream_t s) {
  return dispatch_dtype(dtype, [&](auto t) -> int {
    using T = decltype(t);
    if (prowi == dec::PRO_RMSNORM && epiwi == dec::SK_GEGLU && !bias) return launch_tail<T, dec::PRO_RMSNORM, dec::SK_GEGLU, false>(p, st, layer, n_chains, s);
    if (prowi == dec::PRO_LAYERNORM && epiwi == dec::SK_GELU_ERF && bias) return launch_tail<T, dec::PRO_LAYERNORM, dec::SK_GELU_ERF, true>(p, st, layer, n_chains, s);
    if (prowi == dec::PRO_RMSNORM && epiwi == dec::SK_GELU_ERF && bias) return launch_tail<T, dec::PRO_RMSNORM, dec::SK_GELU_ERF, true>(p, st, layer, n_chains, s);
    set_error("decode: no fused layer tail with wi prologue %d, epilogue %d, bias %d", prowi, epiwi, (int)bias);
    return MH_ERR_ARG;
  });
}

#ifdef MH_PHASE_STAMPS
int gemv_phase_stamps(unsigned long long* acc, int reset) { return dec::take_phase_stamps(acc, reset); }
#endif
}  // namespace mh

// dec_tail_kernel launches enqueued so far (a captured graph node counts once, at capture): lets a caller -- the tests -- tell
// that option decode_fused_tail = 1 really took the fused path for its shape instead of the silent three-launch fall-back
extern "C" long mh_t5_decode_tail_launches(void) { return mh::g_tail_launches.load(); }
