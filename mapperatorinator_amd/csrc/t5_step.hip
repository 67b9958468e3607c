// osuT5 on MI355X: the token step of the KV-cached AR decode, host side.  enqueue_step() -- one step of one chain, what a step graph
// captures -- describes every launch of a step (the operand descriptions below) and hands each to the plain launch function of the
// unit that holds the kernel: decode_attn_bf16.hip / decode_attn_f32.hip, decode_gemv.hip, decode_sample.hip (decode_step.hpp).
// Also here: the decode workspace layout and the measurement hooks that live inside the step.  No kernel is instantiated in this
// unit.  The batched passes are t5_encode.hip, the generation loop and the slot session t5_generate.hip, the step-wise entries of
// beam search t5_stepwise.hip.
//
// Reference semantics reproduced (see include/mapperhip.h for the per-entry citations):
//   HF T5Block / T5Attention / T5LayerFF and the Whisper family's decoder layers, one position at a time.
#include <stdlib.h>
#include <string.h>

#include "decode_step.hpp"

using namespace mh;

namespace mh {
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
// the launch of such a description: residual GEMV with an optional bias (the Whisper family's Wo / fc2)
int resid(int dtype, const dec::SkinnyP& p, hipStream_t s) { return launch_gemv(dtype, dec::PRO_PLAIN, dec::SK_RESID, p.bias != nullptr, p, s); }
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

}  // namespace
int enqueue_step(const StepCall& k, hipStream_t s) {
  const MhT5Config* c = k.c;
  const MhT5Weights* w = k.w;
  const DecBuffers& bf = k.bf;
  const int B = k.Bc, Bfull = k.Bfull, kvB = k.kvB, H = c->n_heads, inner = H * 64, tgt = c->tgt_len, es = es_of(c->dtype), dt = c->dtype;
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
    MH_TRY(launch_self_attn(dt, sa, qkv, inner, bf.self8 ? &f8 : nullptr, k.origin, k.slot_pos ? k.slot_pos + k.smp.b0 : nullptr, s));
    MH_TRY(resid(dt, o_gemv(k, w->dec_o[l], w->dec_o_b[l]), s));
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
    MH_TRY(launch_cross_attn(dt, ca, head_proj(c, bf.h, w->dec_ln2[l], hf ? w->dec_ln2_b[l] : nullptr, w->dec_cq[l]), s));
    const dec::SkinnyP co = o_gemv(k, w->dec_co[l], w->dec_co_b[l]), wi = ffn_in(k, l), wo = ffn_out(k, l);
    // the form of the wi GEMV: T5's gated GELU behind an RMS norm, the Whisper family's biased erf GELU behind its norm
    const int wi_pro = hf ? dec::PRO_LAYERNORM : dec::PRO_RMSNORM, wi_epi = wh ? dec::SK_GELU_ERF : dec::SK_GEGLU;
    if (k.with_sampler && option(OPT_DECODE_FUSED_TAIL) != 0 && tail_covers(c, B, wh, co.bias, wi.bias, wo.bias)) {
      // cross O GEMV + residual, norm + wi + activation, wo + residual as ONE launch (the same device code per phase)
      dec::TailP tp{};
      tp.o = co; tp.wi = wi; tp.wo = wo;
      const int n_chains = ceil_div(Bfull, B);
      MH_TRY(launch_tail(dt, wi_pro, wi_epi, wh, tp, bf.st, l, n_chains, s));
      continue;
    }
    MH_TRY(resid(dt, co, s));
    MH_TRY(launch_gemv(dt, wi_pro, wi_epi, wh, wi, s));
    MH_TRY(resid(dt, wo, s));
  }
  dec::SkinnyP sk{};
  sk.A = bf.h; sk.lda = c->d_model; sk.ln_w = w->dec_final_ln; sk.eps = c->eps; sk.W = w->lm_head; sk.ldw = c->d_model; sk.B = B;
  sk.N = c->vocab_out; sk.K = c->d_model; sk.out = bf.logits; sk.ldo = c->vocab_out;
  if (hf) sk.ln_b = w->dec_final_ln_b;
  MH_TRY(launch_gemv(dt, hf ? dec::PRO_LAYERNORM : dec::PRO_RMSNORM, dec::SK_LOGITS, false, sk, s));
  return k.with_sampler ? launch_sample(dt, k, s) : MH_OK;
}
}  // namespace mh

// ---- byte counts of the e4m3 K/V copies (the quantisers themselves: decode_sample.hip) -----------------------------------------------
extern "C" int64_t mh_t5_cross_kv_fp8_bytes(const MhT5Config* c, int B) {
  mh::OptionScope option_scope(c ? c->options : nullptr);
  if (!c || B <= 0) return -1;
  return cross_kv8_layout(c, B).total;
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
// profiling build only: read (and optionally clear) the phase stamps; out = host uint64 [16][16][2].  Every decode unit keeps the
// table of its own kernels (decode_device.hpp): their sum is the one table
extern "C" int mh_debug_phase_stamps(unsigned long long* out, int reset) {
  if (out) memset(out, 0, sizeof(unsigned long long) * 16 * 16 * 2);
  MH_TRY(mh::gemv_phase_stamps(out, reset));
  MH_TRY(mh::attn_bf16_phase_stamps(out, reset));
  return mh::attn_f32_phase_stamps(out, reset);
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

// (mh_t5_decode_tail_launches: decode_gemv.hip, beside the launcher that counts)

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
      rc = launch_cross_attn(c->dtype, ca, hp, s);
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
