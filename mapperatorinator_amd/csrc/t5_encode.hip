// osuT5 on MI355X: the batched passes -- encoder stack, cross-attention K/V projection, the decoder's prompt prefill and the
// teacher-forced decoder forward / scoring built on it.  All of them are MFMA GEMMs + flash attention over whole sequences; the row
// kernels between them (conversions, rotate-half RoPE) live here.  The token-by-token decode is t5_step.hip and the decode_* units (kernels, one step) under
// t5_generate.hip / t5_stepwise.hip (host loops).
//
// Reference semantics reproduced (see include/mapperhip.h for the per-entry citations):
//   HF T5Stack / T5Block / T5Attention / T5LayerFF (pre-norm residual blocks, shared layer-0 relative
//   bias, no 1/sqrt(d) scaling, gated gelu_new FFN); the Whisper family's encoder / decoder layers.
#include <stdlib.h>
#include <string.h>

#include "decode_step.hpp"
#include "t5_host.hpp"

using namespace mh;

// ------------------------------------------------------------------------------------------------
// encoder
// ------------------------------------------------------------------------------------------------
extern "C" int64_t mh_t5_encode_workspace_bytes(const MhT5Config* c, int B) {
  mh::OptionScope option_scope(c ? c->options : nullptr);
  if (!c || B <= 0) return -1;
  const int64_t rows = (int64_t)B * c->src_len, es = es_of(c->dtype);
  const int inner = c->n_heads * 64, Lpad = round_up(c->src_len, 64);
  int64_t t = 0;
  if (c->arch >= 1)   // front-end scratch + its output (storage type) in front of the layer buffers
    t += align256(mh_whisper_frontend_workspace_bytes(B, c->in_frames, c->arch == 2 ? c->d_model : c->n_mels_pad, c->d_model, c->dtype)) +
         align256(rows * c->d_model * es);
  if (c->arch == 2)   // encoder_embedder output in front of conv1: fp32 accumulator rows + their storage-typed copy
    t += align256((int64_t)B * c->in_frames * c->d_model * 4) + align256((int64_t)B * c->in_frames * c->d_model * es);
  t += align256(rows * c->d_model * 4);                    // h
  t += align256(rows * c->d_model * es);                   // n
  t += align256(rows * 2 * inner * es);                    // qk
  t += align256((int64_t)B * inner * Lpad * es);           // vt
  t += align256(rows * inner * es);                        // attn
  t += align256(rows * c->d_ff * es);                      // ff
  if (c->enc_operand_dtype == MH_MX8)                      // MX-fp8 copy of the current GEMM's A operand (widest: d_ff columns)
    t += mx_operand_bytes(rows, c->d_ff > c->d_model ? c->d_ff : c->d_model);
  return t;
}

namespace mh {
namespace {
// fp32 residual stream <- storage-typed rows (the conv front-end's output)
template <typename T>
__global__ __launch_bounds__(256) void rows_to_f32_kernel(const T* __restrict__ x, float* __restrict__ h, long n) {
  const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i + 3 < n) {
    *reinterpret_cast<float4*>(h + i) = make_float4(Elem<T>::to_f32(x[i]), Elem<T>::to_f32(x[i + 1]), Elem<T>::to_f32(x[i + 2]), Elem<T>::to_f32(x[i + 3]));
  } else {
    for (long j = i; j < n; ++j) h[j] = Elem<T>::to_f32(x[j]);
  }
}
// storage-typed rows <- fp32 rows (arch 2: encoder_embedder's output becomes conv1's operand)
template <typename T>
__global__ __launch_bounds__(256) void f32_to_rows_kernel(const float* __restrict__ h, T* __restrict__ x, long n) {
  const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i + 3 < n) {
    const float4 v = *reinterpret_cast<const float4*>(h + i);
    x[i] = Elem<T>::from_f32(v.x); x[i + 1] = Elem<T>::from_f32(v.y); x[i + 2] = Elem<T>::from_f32(v.z); x[i + 3] = Elem<T>::from_f32(v.w);
  } else {
    for (long j = i; j < n; ++j) x[j] = Elem<T>::from_f32(h[j]);
  }
}
// rotate-half RoPE in place on the q | k block of a QKV GEMM output (apply_rotary_pos_emb,
// osuT5/osuT5/model/custom_transformers/modeling_varwhisper.py:229-258): row r = b * L + position, 2H head slots of 64
// columns; one thread rotates 8 pairs (i, i + 32): two 16-byte (bf16) / four (fp32) accesses each way.
// rope fp32 [L][64] = cos(32) | sin(32).
template <typename T>
__global__ __launch_bounds__(256) void rope_qk_kernel(T* __restrict__ qk, int ld, long rows, int L, int slots, const float* __restrict__ rope) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;       // (row, slot, chunk of 8 pairs)
  const long total = rows * slots * 4;
  if (idx >= total) return;
  const int c = (int)(idx & 3);
  const long rs = idx >> 2;
  const int slot = (int)(rs % slots);
  const long row = rs / slots;
  const int pos = (int)(row % L);
  T* x1 = qk + row * ld + slot * 64 + c * 8;
  T* x2 = x1 + 32;
  const float* cs = rope + (long)pos * 64 + c * 8;
  float a[8], b[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) { a[i] = Elem<T>::to_f32(x1[i]); b[i] = Elem<T>::to_f32(x2[i]); }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float co = cs[i], si = cs[32 + i];
    x1[i] = Elem<T>::from_f32(a[i] * co - b[i] * si);
    x2[i] = Elem<T>::from_f32(b[i] * co + a[i] * si);
  }
}

// rotate-half RoPE in place on the cached keys of positions 0 .. np-1: kc [BH][tgt][64], one thread per (bh, pos, 8 pairs)
template <typename T>
__global__ __launch_bounds__(256) void rope_cache_kernel(T* __restrict__ kc, long BH, int tgt, int np, const float* __restrict__ rope) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= BH * np * 4) return;
  const int c = (int)(idx & 3);
  const long rp = idx >> 2;
  const int pos = (int)(rp % np);
  const long bh = rp / np;
  T* x1 = kc + (bh * tgt + pos) * 64 + c * 8;
  T* x2 = x1 + 32;
  const float* cs = rope + (long)pos * 64 + c * 8;
  float a[8], b[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) { a[i] = Elem<T>::to_f32(x1[i]); b[i] = Elem<T>::to_f32(x2[i]); }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float co = cs[i], si = cs[32 + i];
    x1[i] = Elem<T>::from_f32(a[i] * co - b[i] * si);
    x2[i] = Elem<T>::from_f32(b[i] * co + a[i] * si);
  }
}

// h[b * L + t][:] = row_bias[b][:]  (the conditioning embedders' contribution, constant along a chunk's frames)
__global__ __launch_bounds__(256) void fill_rows_kernel(float* __restrict__ h, const float* __restrict__ row_bias, int L, int d) {
  const long row = blockIdx.x;
  const float4* src = reinterpret_cast<const float4*>(row_bias + (row / L) * d);
  float4* dst = reinterpret_cast<float4*>(h + row * d);
  for (int i = threadIdx.x; i < d / 4; i += 256) dst[i] = src[i];
}
}  // namespace
}  // namespace mh

extern "C" int mh_t5_encode(const MhT5Config* c, const MhT5Weights* w, const void* mel, int B, void* enc_out,
                            float* enc_out_f32, void* workspace, int64_t workspace_bytes, void* stream) {
  mh::OptionScope option_scope(c ? c->options : nullptr);
  return mh_t5_encode_cond(c, w, mel, B, nullptr, enc_out, enc_out_f32, workspace, workspace_bytes, stream);
}

extern "C" int mh_t5_encode_cond(const MhT5Config* c, const MhT5Weights* w, const void* mel, int B, const float* row_bias,
                                 void* enc_out, float* enc_out_f32, void* workspace, int64_t workspace_bytes, void* stream) {
  mh::OptionScope option_scope(c ? c->options : nullptr);
  MH_TRY(check_cfg(c, "mh_t5_encode"));
  MH_REQUIRE(w && mel && enc_out && workspace && B > 0, "mh_t5_encode: null argument");
  MH_REQUIRE(workspace_bytes >= mh_t5_encode_workspace_bytes(c, B), "mh_t5_encode: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int L = c->src_len, d = c->d_model, H = c->n_heads, inner = H * 64, dff = c->d_ff;
  const int rows = B * L, es = es_of(c->dtype), Lpad = round_up(L, 64);
  Arena ar(workspace, workspace_bytes);
  if (c->arch >= 1) {
    // ---- VarWhisperEncoder.forward (modeling_varwhisper.py:779-852) / RoPEWhisperEncoder.forward (modeling_ropewhisper.py:
    // 1167-1278); arch 2: HF WhisperEncoder.forward behind the wrapper's encoder_embedder ---------------------------------
    const bool hf = c->arch == 2;
    MH_REQUIRE(hf || !row_bias, "mh_t5_encode: arch 1 takes its conditioning as conv1 input channels (mh_cond_channels), not as a row bias");
    MH_REQUIRE(w->conv1_w && w->conv1_b && w->conv2_w && w->conv2_b, "mh_t5_encode: arch 1 / 2 need the conv front-end weights");
    MH_REQUIRE(hf || w->enc_rope, "mh_t5_encode: arch 1 needs the rotary table");
    MH_REQUIRE(!hf || (w->enc_embed_w && w->enc_pos && w->enc_final_ln_b), "mh_t5_encode: arch 2 needs encoder_embedder, embed_positions and the LayerNorm biases");
    const int fe_C = hf ? d : c->n_mels_pad;
    const int64_t fe_bytes = mh_whisper_frontend_workspace_bytes(B, c->in_frames, fe_C, d, c->dtype);
    void* fe_ws = ar.take(fe_bytes);
    void* x0 = ar.take((int64_t)rows * d * es);
    const int64_t rows_in = (int64_t)B * c->in_frames;
    float* hin = hf ? (float*)ar.take(rows_in * d * 4) : nullptr;
    void* xin = hf ? ar.take(rows_in * d * es) : nullptr;
    float* h = (float*)ar.take((int64_t)rows * d * 4);
    void* n = ar.take((int64_t)rows * d * es);
    void* qk = ar.take((int64_t)rows * 2 * inner * es);
    void* vt = ar.take((int64_t)B * inner * Lpad * es);
    void* attn = ar.take((int64_t)rows * inner * es);
    void* ff = ar.take((int64_t)rows * dff * es);
    MH_REQUIRE(ar.ok() && ff, "mh_t5_encode: arena overflow");
    const void* fe_in = mel;
    if (hf) {
      // input_features = encoder_embedder([mel | cond]) (modeling_mapperatorinator.py:204-205,211): the T5 path's projection
      // (row_bias = the conditioning columns' contribution incl. the bias), rounded to the storage type = conv1's operand
      MH_REQUIRE(xin != nullptr, "mh_t5_encode: arena overflow");
      MhGemm ge = MhGemm{};
      ge.A = mel; ge.lda = c->n_mels_pad; ge.W = w->enc_embed_w; ge.ldw = c->n_mels_pad; ge.C = hin; ge.ldc = d;
      ge.M = (int)rows_in; ge.N = d; ge.K = c->n_mels_pad; ge.bias = w->enc_embed_b; ge.dtype = c->dtype; ge.epilogue = MH_EPI_STORE_F32;
      if (row_bias) {
        hipLaunchKernelGGL(mh::fill_rows_kernel, dim3((unsigned)rows_in), dim3(256), 0, s, hin, row_bias, c->in_frames, d);
        MH_TRY(check_launch("fill_rows_kernel"));
        ge.bias = nullptr; ge.epilogue = MH_EPI_RESID;
      }
      MH_TRY(gemm(ge, s));
      const long n_in = (long)rows_in * d;
      if (c->dtype == MH_BF16) hipLaunchKernelGGL(mh::f32_to_rows_kernel<bf16_t>, dim3((unsigned)((n_in / 4 + 255) / 256 + 1)), dim3(256), 0, s, hin, (bf16_t*)xin, n_in);
      else hipLaunchKernelGGL(mh::f32_to_rows_kernel<float>, dim3((unsigned)((n_in / 4 + 255) / 256 + 1)), dim3(256), 0, s, hin, (float*)xin, n_in);
      MH_TRY(check_launch("f32_to_rows_kernel"));
      fe_in = xin;
    }
    MH_TRY(mh_whisper_frontend(fe_in, B, c->in_frames, fe_C, w->conv1_w, w->conv1_b, w->conv2_w, w->conv2_b, hf ? w->enc_pos : nullptr, d, x0,
                               fe_ws, fe_bytes, c->dtype, stream));
    const long nel = (long)rows * d;
    if (c->dtype == MH_BF16) hipLaunchKernelGGL(mh::rows_to_f32_kernel<bf16_t>, dim3((unsigned)((nel / 4 + 255) / 256 + 1)), dim3(256), 0, s, (const bf16_t*)x0, h, nel);
    else hipLaunchKernelGGL(mh::rows_to_f32_kernel<float>, dim3((unsigned)((nel / 4 + 255) / 256 + 1)), dim3(256), 0, s, (const float*)x0, h, nel);
    MH_TRY(check_launch("rows_to_f32_kernel"));
    if (hipMemsetAsync(vt, 0, (size_t)B * inner * Lpad * es, s) != hipSuccess) return check_launch("memset vt");
    MhGemm g;
    for (int l = 0; l < c->n_enc_layers; ++l) {
      const bool local = is_local_layer(c, l);
      MH_TRY(pre_norm(c, h, w->enc_ln1[l], w->enc_ln1_b[l], n, rows, c->dtype, s));
      g = MhGemm{};
      g.A = n; g.lda = d; g.W = w->enc_qkv[l]; g.ldw = d; g.C = qk; g.ldc = 2 * inner; g.M = rows; g.N = 3 * inner;
      g.K = d; g.bias = w->enc_qkv_b[l]; g.dtype = c->dtype; g.epilogue = MH_EPI_QKV_VT; g.C2 = vt; g.n_split = 2 * inner;
      g.kv_B = B; g.kv_H = H; g.kv_L = L; g.kv_Lpad = Lpad;
      MH_TRY(gemm(g, s));
      if (!hf) {   // (HF Whisper: absolute positions were added by the front-end, no rotation)
        const float* rope = (local && w->enc_rope_local) ? w->enc_rope_local : w->enc_rope;
        const long work = (long)rows * 2 * H * 4;
        if (c->dtype == MH_BF16) hipLaunchKernelGGL(mh::rope_qk_kernel<bf16_t>, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, s, (bf16_t*)qk, 2 * inner, (long)rows, L, 2 * H, rope);
        else hipLaunchKernelGGL(mh::rope_qk_kernel<float>, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, s, (float*)qk, 2 * inner, (long)rows, L, 2 * H, rope);
        MH_TRY(check_launch("rope_qk_kernel"));
      }
      MH_TRY(attention(qk, 2 * inner, inner, vt, Lpad, nullptr, attn, inner, B, L, H, c->attn_scale, local ? -c->local_window : 0, c->dtype, s));
      g = MhGemm{};
      g.A = attn; g.lda = inner; g.W = w->enc_o[l]; g.ldw = inner; g.C = h; g.ldc = d; g.M = rows; g.N = d; g.K = inner;
      g.bias = w->enc_o_b[l]; g.dtype = c->dtype; g.epilogue = MH_EPI_RESID;
      MH_TRY(gemm(g, s));
      MH_TRY(pre_norm(c, h, w->enc_ln2[l], w->enc_ln2_b[l], n, rows, c->dtype, s));
      MH_REQUIRE(w->enc_fc1_b[l] && w->enc_fc2_b[l], "mh_t5_encode: fc1 / fc2 carry biases in the Whisper family");
      g = MhGemm{};
      g.A = n; g.lda = d; g.W = w->enc_wi[l]; g.ldw = d; g.C = ff; g.ldc = dff; g.M = rows; g.N = dff; g.K = d;
      g.bias = w->enc_fc1_b[l]; g.dtype = c->dtype; g.epilogue = MH_EPI_BIAS_GELU_ERF;
      MH_TRY(gemm(g, s));
      g = MhGemm{};
      g.A = ff; g.lda = dff; g.W = w->enc_wo[l]; g.ldw = dff; g.C = h; g.ldc = d; g.M = rows; g.N = d; g.K = dff;
      g.bias = w->enc_fc2_b[l]; g.dtype = c->dtype; g.epilogue = MH_EPI_RESID;
      MH_TRY(gemm(g, s));
    }
    MH_TRY(pre_norm(c, h, w->enc_final_ln, w->enc_final_ln_b, enc_out, rows, c->dtype, s));
    if (enc_out_f32) MH_TRY(pre_norm(c, h, w->enc_final_ln, w->enc_final_ln_b, enc_out_f32, rows, MH_F32, s));
    return MH_OK;
  }
  float* h = (float*)ar.take((int64_t)rows * d * 4);
  void* n = ar.take((int64_t)rows * d * es);
  void* qk = ar.take((int64_t)rows * 2 * inner * es);
  void* vt = ar.take((int64_t)B * inner * Lpad * es);
  void* attn = ar.take((int64_t)rows * inner * es);
  void* ff = ar.take((int64_t)rows * dff * es);
  const bool mx = enc_mx(c);
  const int kmax = dff > d ? dff : d;
  uint8_t* xq = mx ? (uint8_t*)ar.take((int64_t)rows * kmax) : nullptr;                       // e4m3 bytes of the current A operand
  uint8_t* xs = mx ? (uint8_t*)ar.take((int64_t)rows * mx8_scale_row_bytes(kmax)) : nullptr;  // its E8M0 scales
  MH_REQUIRE(ar.ok() && ff && (!mx || xs), "mh_t5_encode: arena overflow");
  if (mx) {
    MH_REQUIRE(w->dec_ckv_all_mx && w->dec_ckv_all_mxs, "mh_t5_encode: enc_operand_dtype = MH_MX8 needs the MX-fp8 weight copies");
    for (int l = 0; l < c->n_enc_layers; ++l)
      MH_REQUIRE(w->enc_qkv_mx[l] && w->enc_qkv_mxs[l] && w->enc_o_mx[l] && w->enc_o_mxs[l] && w->enc_wi_mx[l] && w->enc_wi_mxs[l] &&
                     w->enc_wo_mx[l] && w->enc_wo_mxs[l], "mh_t5_encode: enc_operand_dtype = MH_MX8 needs the MX-fp8 weight copies (layer %d)", l);
  }
  if (hipMemsetAsync(vt, 0, (size_t)B * inner * Lpad * es, s) != hipSuccess) return check_launch("memset vt");

  MhGemm g;
  // h = encoder_embedder(mel)      (modeling_mapperatorinator.py:195-196)
  g = MhGemm{};
  g.A = mel; g.lda = c->n_mels_pad; g.W = w->enc_embed_w; g.ldw = c->n_mels_pad; g.C = h; g.ldc = d;
  g.M = rows; g.N = d; g.K = c->n_mels_pad; g.bias = w->enc_embed_b; g.dtype = c->dtype; g.epilogue = MH_EPI_STORE_F32;
  if (row_bias) {
    // conditioning: [mel | cond] @ W^T + b = mel @ W[:, :n_mels]^T + (cond @ W[:, n_mels:]^T + b); the bracket is the
    // caller's per-chunk row_bias [B, d] (it already contains b), laid under the mel product
    MH_REQUIRE(d % 4 == 0, "mh_t5_encode_cond: d_model must be a multiple of 4");
    hipLaunchKernelGGL(mh::fill_rows_kernel, dim3(rows), dim3(256), 0, s, h, row_bias, L, d);
    MH_TRY(check_launch("fill_rows_kernel"));
    g.bias = nullptr; g.epilogue = MH_EPI_RESID;
  }
  MH_TRY(gemm(g, s));

  // MX-fp8 operands (enc_operand_dtype = MH_MX8): the A operand of each projection is the e4m3 + E8M0 copy in xq / xs -- written
  // by the RMSNorm itself (the bf16 rounding of the storage mode applied first, so the quantiser sees what the bf16 path multiplies),
  // or by a pass over the bf16 buffer the attention / the gated GELU wrote
  auto operand = [&](MhGemm& gg, const void* a_plain, int K, const void* w_plain, const uint8_t* w_mx, const uint8_t* w_mxs) {
    if (mx) { gg.A = xq; gg.lda = K; gg.a_scale = xs; gg.W = w_mx; gg.ldw = K; gg.w_scale = w_mxs; gg.dtype = MH_MX8; }
    else { gg.A = a_plain; gg.lda = K; gg.W = w_plain; gg.ldw = K; gg.dtype = c->dtype; }
  };
  for (int l = 0; l < c->n_enc_layers; ++l) {
    if (mx) MH_TRY(rmsnorm_mx8(h, d, w->enc_ln1[l], rows, d, c->eps, MH_BF16, xq, d, xs, s));
    else MH_TRY(rmsnorm(h, d, w->enc_ln1[l], n, d, rows, d, c->eps, c->dtype, s));
    g = MhGemm{};
    operand(g, n, d, w->enc_qkv[l], w->enc_qkv_mx[l], w->enc_qkv_mxs[l]);
    g.C = qk; g.ldc = 2 * inner; g.M = rows; g.N = 3 * inner;
    g.K = d; g.epilogue = MH_EPI_QKV_VT; g.C2 = vt; g.n_split = 2 * inner; g.kv_B = B; g.kv_H = H;
    g.kv_L = L; g.kv_Lpad = Lpad;
    MH_TRY(gemm(g, s));
    MH_TRY(attention(qk, 2 * inner, inner, vt, Lpad, w->enc_rel_bias, attn, inner, B, L, H, 1.0f, 0, c->dtype, s));
    if (mx) MH_TRY(quantize_mx8(attn, inner, rows, inner, MH_BF16, xq, inner, xs, s));
    g = MhGemm{};
    operand(g, attn, inner, w->enc_o[l], w->enc_o_mx[l], w->enc_o_mxs[l]);
    g.C = h; g.ldc = d; g.M = rows; g.N = d; g.K = inner; g.epilogue = MH_EPI_RESID;
    MH_TRY(gemm(g, s));
    if (mx) MH_TRY(rmsnorm_mx8(h, d, w->enc_ln2[l], rows, d, c->eps, MH_BF16, xq, d, xs, s));
    else MH_TRY(rmsnorm(h, d, w->enc_ln2[l], n, d, rows, d, c->eps, c->dtype, s));
    g = MhGemm{};
    operand(g, n, d, w->enc_wi[l], w->enc_wi_mx[l], w->enc_wi_mxs[l]);
    g.C = ff; g.ldc = dff; g.M = rows; g.N = 2 * dff; g.K = d; g.epilogue = MH_EPI_GEGLU;
    // MX mode: the gated GELU leaves the GEMM as the MX-fp8 operand of wo (the bytes mh_quantize_mx8 would make of the bf16
    // hidden) -- into the second operand buffer: xq / xs still hold this GEMM's own A operand
    const bool mx_fused = mx && dff % 128 == 0;
    uint8_t* xq2 = reinterpret_cast<uint8_t*>(ff);                 // (the bf16 hidden is not written then: its buffer holds the MX image)
    uint8_t* xs2 = xq2 + (int64_t)rows * dff;
    if (mx_fused) {
      if (dff % 512) MH_REQUIRE(hipMemsetAsync(xs2, 0, (size_t)rows * mx8_scale_row_bytes(dff), s) == hipSuccess, "mh_t5_encode: scale reset failed");
      g.mx_out = xq2; g.mx_out_scales = xs2; g.ldc = dff;
    }
    MH_TRY(gemm(g, s));
    if (mx && !mx_fused) MH_TRY(quantize_mx8(ff, dff, rows, dff, MH_BF16, xq, dff, xs, s));
    g = MhGemm{};
    operand(g, ff, dff, w->enc_wo[l], w->enc_wo_mx[l], w->enc_wo_mxs[l]);
    if (mx_fused) { g.A = xq2; g.a_scale = xs2; }
    g.C = h; g.ldc = d; g.M = rows; g.N = d; g.K = dff; g.epilogue = MH_EPI_RESID;
    MH_TRY(gemm(g, s));
  }
  MH_TRY(rmsnorm(h, d, w->enc_final_ln, enc_out, d, rows, d, c->eps, c->dtype, s));
  if (enc_out_f32) MH_TRY(rmsnorm(h, d, w->enc_final_ln, enc_out_f32, d, rows, d, c->eps, MH_F32, s));
  return MH_OK;
}

extern "C" int64_t mh_t5_cross_kv_workspace_bytes(const MhT5Config* c, int B) {
  mh::OptionScope option_scope(c ? c->options : nullptr);
  if (!c || B <= 0) return -1;
  return c->enc_operand_dtype == MH_MX8 ? mx_operand_bytes((int64_t)B * c->src_len, c->d_model) : 0;
}

extern "C" int mh_t5_cross_kv_ws(const MhT5Config* c, const MhT5Weights* w, const void* enc_out, int B, void* cross_kv, void* workspace,
                                 int64_t workspace_bytes, void* stream) {
  mh::OptionScope option_scope(c ? c->options : nullptr);
  MH_TRY(check_cfg(c, "mh_t5_cross_kv"));
  MH_REQUIRE(w && enc_out && cross_kv && B > 0, "mh_t5_cross_kv: null argument");
  if (!enc_mx(c)) return mh_t5_cross_kv(c, w, enc_out, B, cross_kv, stream);
  MH_REQUIRE(workspace && workspace_bytes >= mh_t5_cross_kv_workspace_bytes(c, B), "mh_t5_cross_kv_ws: workspace too small");
  MH_REQUIRE(w->dec_ckv_all_mx && w->dec_ckv_all_mxs, "mh_t5_cross_kv_ws: enc_operand_dtype = MH_MX8 needs dec_ckv_all_mx / _mxs");
  hipStream_t s = (hipStream_t)stream;
  const int inner = c->n_heads * 64, d = c->d_model, rows = B * c->src_len;
  Arena ar(workspace, workspace_bytes);
  uint8_t* xq = (uint8_t*)ar.take((int64_t)rows * d);
  uint8_t* xs = (uint8_t*)ar.take((int64_t)rows * mx8_scale_row_bytes(d));
  MH_REQUIRE(ar.ok() && xs, "mh_t5_cross_kv_ws: arena overflow");
  MH_TRY(quantize_mx8(enc_out, d, rows, d, MH_BF16, xq, d, xs, s));
  MhGemm g = MhGemm{};
  g.A = xq; g.lda = d; g.a_scale = xs; g.W = w->dec_ckv_all_mx; g.ldw = d; g.w_scale = w->dec_ckv_all_mxs; g.C = cross_kv; g.ldc = 0;
  g.M = rows; g.N = c->n_dec_layers * 2 * inner; g.K = d; g.dtype = MH_MX8;
  g.epilogue = MH_EPI_KV_SCATTER; g.kv_B = B; g.kv_H = c->n_heads; g.kv_L = c->src_len;
  return gemm(g, s);
}

extern "C" int mh_t5_cross_kv(const MhT5Config* c, const MhT5Weights* w, const void* enc_out, int B, void* cross_kv,
                              void* stream) {
  mh::OptionScope option_scope(c ? c->options : nullptr);
  MH_TRY(check_cfg(c, "mh_t5_cross_kv"));
  MH_REQUIRE(w && enc_out && cross_kv && B > 0, "mh_t5_cross_kv: null argument");
  MH_REQUIRE(!enc_mx(c), "mh_t5_cross_kv: enc_operand_dtype = MH_MX8 needs scratch for the quantised encoder output: call mh_t5_cross_kv_ws");
  const int inner = c->n_heads * 64;
  MhGemm g = MhGemm{};
  g.A = enc_out; g.lda = c->d_model; g.W = w->dec_ckv_all; g.ldw = c->d_model; g.C = cross_kv; g.ldc = 0;
  g.M = B * c->src_len; g.N = c->n_dec_layers * 2 * inner; g.K = c->d_model; g.dtype = c->dtype;
  g.bias = c->arch >= 1 ? w->dec_ckv_b_all : nullptr;
  g.epilogue = MH_EPI_KV_SCATTER; g.kv_B = B; g.kv_H = c->n_heads; g.kv_L = c->src_len;
  return gemm(g, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------------
// batched prompt prefill
// ------------------------------------------------------------------------------------------------
namespace mh {
namespace {
// rows r = b*np + i  <-  dec_embed[prompt[b][i]]   (fp32 residual stream of the prompt prefill)
template <typename T>
__global__ __launch_bounds__(256) void prefill_embed_kernel(const int32_t* __restrict__ prompt, int P, int np,
                                                           const T* __restrict__ emb, int d, float* __restrict__ h,
                                                           const float* __restrict__ dec_pos, const uint8_t* __restrict__ pos_mask) {
  // dec_pos (arch 2): + decoder.embed_positions[position of column i]; pos_mask != NULL (dec_pos_from_mask): minus the row's masked columns
  const int r = blockIdx.x, b = r / np, i = r - b * np;
  __shared__ int s_off;
  if (threadIdx.x == 0) {
    int off = 0;
    if (dec_pos && pos_mask)
      for (int k = 0; k < P; ++k) off += pos_mask[(long)b * P + k] == 0;
    s_off = off;
  }
  __syncthreads();
  const T* e = emb + (long)prompt[(long)b * P + i] * d;
  const float* pe = dec_pos ? dec_pos + (long)(i - s_off > 0 ? i - s_off : 0) * d : nullptr;
  for (int k = threadIdx.x; k < d; k += 256) h[(long)r * d + k] = Elem<T>::to_f32(e[k]) + (pe ? pe[k] : 0.f);
}
}  // namespace

int64_t prefill_layout(const MhT5Config* c, int B, int np_max, void* base, int64_t size, PrefillBuf* out) {
  Arena ar(base, size);
  const int64_t es = es_of(c->dtype), rows = (int64_t)B * np_max, inner = c->n_heads * 64;
  PrefillBuf t;
  t.np_pad = round_up(np_max, 64);
  t.Lpad = round_up(c->src_len, 64);
  t.h = (float*)ar.take(rows * c->d_model * 4);
  t.n = ar.take(rows * c->d_model * es);
  t.q = ar.take(rows * inner * es);
  t.attn = ar.take(rows * inner * es);
  t.ff = ar.take(rows * c->d_ff * es);
  t.vt = ar.take((int64_t)B * inner * t.np_pad * es);
  t.cross_vt = ar.take((int64_t)c->n_dec_layers * B * inner * t.Lpad * es);
  if (out) *out = t;
  return ar.off;
}

// Batched prompt prefill: positions 0 .. P-2 of every row go through the decoder stack at once (MFMA GEMMs +
// flash attention), filling the self-attention K/V caches exactly as P-1 single-token steps would
// (HF prefill: SURVEY.md appendix A.1).  Position P-1 is left to the per-token loop, which also produces the
// first sampled token.  Left-pad keys are masked, left-pad query rows produce unused garbage, as in HF.
int prefill_prompt(const MhT5Config* c, const MhT5Weights* w, const void* cross_kv, int B, int kvB, const int32_t* prompt,
                   const uint8_t* prompt_mask, int P, int np, void* self_k, void* self_v, const PrefillBuf& pb, hipStream_t s,
                   int cache_rows, int plan_B) {
  // P = row stride of `prompt` / `prompt_mask`, np <= P = positions that go through the stack
  // cache_rows: rows of the caches self_k / self_v point into (their layer stride); 0 = B.  More than B (mh_t5_step_prefill): the
  // B prompts fill cache rows 0 .. B-1 of every layer
  // plan_B > B: these rows are a row block of the prefill of plan_B rows and every GEMM runs the kernel that one would choose, hence
  // its summation order (mh_t5_slots_admit_pair: one row of a pair at a time computes what the B = 2 prefill computes of it)
  if (cache_rows <= 0) cache_rows = B;
  const int rows = B * np;
  const int plan_M = plan_B > B ? plan_B * np : 0;
  const int d = c->d_model, H = c->n_heads, inner = H * 64, dff = c->d_ff, L = c->src_len, tgt = c->tgt_len;
  const int es = es_of(c->dtype);
  const int np_pad = round_up(np, 64);
  // arch 1 (VarWhisperDecoderLayer, modeling_varwhisper.py:633-741) through the same batched form: biased projections,
  // rotate-half RoPE on q and on the cached keys, scores / 8 without a relative bias, fc1 -> gelu(erf) -> fc2.  A local
  // (windowed) layer takes its own rotary table and the causal attention gets the band |k - q| <= local_window on top -- the
  // keys the token-by-token step attends (decode_params.hpp `window`).
  // arch 2 (HF WhisperDecoderLayer): the same with affine LayerNorms, absolute positions added to the embedding, no rotation
  const bool wh = c->arch >= 1, hf = c->arch == 2;
  if (wh && !hf) MH_REQUIRE(w->dec_rope != nullptr, "prefill: the Whisper family needs its rotary table");
  MH_TRY(check_arch2_weights(c, w, "prefill"));
  const float* dpos = hf ? w->dec_pos : nullptr;
  const uint8_t* pmask = (hf && c->dec_pos_from_mask) ? prompt_mask : nullptr;
  MH_TRY(dispatch_dtype(c->dtype, [&](auto t) {
    hipLaunchKernelGGL(prefill_embed_kernel<decltype(t)>, dim3(rows), dim3(256), 0, s, prompt, P, np, (const decltype(t)*)w->dec_embed, d, pb.h, dpos, pmask);
    return check_launch("prefill_embed_kernel");
  }));
  if (hipMemsetAsync(pb.vt, 0, (size_t)B * inner * np_pad * es, s) != hipSuccess) return check_launch("memset prefill vt");
  if (hipMemsetAsync(pb.cross_vt, 0, (size_t)c->n_dec_layers * kvB * inner * pb.Lpad * es, s) != hipSuccess)
    return check_launch("memset cross vt");
  const long kv_layer = (long)kvB * H * L * 64;   // elements per (layer, k|v) slab of cross_kv (kvB = B/2 under CFG)
  for (int l = 0; l < c->n_dec_layers; ++l)
    MH_TRY(transpose_v((const char*)cross_kv + (long)(l * 2 + 1) * kv_layer * es, (long)H * L * 64, (long)L * 64, L,
                       (char*)pb.cross_vt + (long)l * kvB * inner * pb.Lpad * es, pb.Lpad, kvB, H, c->dtype, s));
  MhGemm g;
  for (int l = 0; l < c->n_dec_layers; ++l) {
    char* kc = (char*)self_k + (long)l * cache_rows * H * tgt * 64 * es;
    char* vc = (char*)self_v + (long)l * cache_rows * H * tgt * 64 * es;
    // self attention over the prompt
    MH_TRY(pre_norm(c, pb.h, w->dec_ln1[l], w->dec_ln1_b[l], pb.n, rows, c->dtype, s));
    g = MhGemm{};
    g.A = pb.n; g.lda = d; g.W = w->dec_qkv[l]; g.ldw = d; g.C = pb.q; g.ldc = inner; g.M = rows; g.N = 3 * inner; g.K = d;
    g.dtype = c->dtype; g.epilogue = MH_EPI_QKV_CACHE; g.n_split = inner; g.C2 = kc; g.C3 = vc; g.C4 = pb.vt; g.kv_B = B;
    g.kv_H = H; g.kv_L = np; g.kv_Lpad = np_pad; g.cache_len = tgt;
    if (wh) g.bias = w->dec_qkv_b[l];
    MH_TRY(gemm(g, s, false, plan_M));
    const bool local = is_local_layer(c, l);
    if (wh && !hf) {   // rotate-half RoPE on q (all prompt positions) and on the keys just cached; position = column of the padded prompt
      const long wq = (long)rows * H * 4, wk = (long)B * H * np * 4;
      const float* rope = (local && w->dec_rope_local) ? w->dec_rope_local : w->dec_rope;
      MH_TRY(dispatch_dtype(c->dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(mh::rope_qk_kernel<T>, dim3((unsigned)((wq + 255) / 256)), dim3(256), 0, s, (T*)pb.q, inner, (long)rows, np, H, rope);
        hipLaunchKernelGGL(mh::rope_cache_kernel<T>, dim3((unsigned)((wk + 255) / 256)), dim3(256), 0, s, (T*)kc, (long)B * H, tgt, np, rope);
        return check_launch("rope (prefill)");
      }));
    }
    AttnArgs a{};
    a.q = pb.q; a.q_rs = (long)inner * es; a.q_bs = (long)np * inner * es;
    a.k = kc; a.k_rs = 64L * es; a.k_hs = (long)tgt * 64 * es; a.k_bs = (long)H * tgt * 64 * es;
    a.vt = pb.vt; a.Lkpad = np_pad; a.vt_hs = 64L * np_pad * es; a.vt_bs = (long)H * 64 * np_pad * es;
    if (!wh) { a.bias = w->dec_rel_bias; a.bias_hs = tgt; a.bias_center = 0; a.bias_sign = -1; a.bias_min = 0; a.bias_max = tgt - 1; }
    a.key_mask = prompt_mask; a.mask_ld = P; a.mask_len = np;
    a.out = pb.attn; a.out_rs = (long)inner * es; a.out_bs = (long)np * inner * es;
    a.Lq = np; a.Lk = np; a.scale = wh ? c->attn_scale : 1.0f; a.band = local ? -c->local_window : 0; a.causal = 1; a.q_pos0 = 0;
    MH_TRY(attention_general(a, B, H, c->dtype, s));
    g = MhGemm{};
    g.A = pb.attn; g.lda = inner; g.W = w->dec_o[l]; g.ldw = inner; g.C = pb.h; g.ldc = d; g.M = rows; g.N = d; g.K = inner;
    g.dtype = c->dtype; g.epilogue = MH_EPI_RESID;
    if (wh) g.bias = w->dec_o_b[l];
    MH_TRY(gemm(g, s, false, plan_M));
    // cross attention of every prompt position over the encoder keys
    MH_TRY(pre_norm(c, pb.h, w->dec_ln2[l], w->dec_ln2_b[l], pb.n, rows, c->dtype, s));
    g = MhGemm{};
    g.A = pb.n; g.lda = d; g.W = w->dec_cq[l]; g.ldw = d; g.C = pb.q; g.ldc = inner; g.M = rows; g.N = inner; g.K = d;
    g.dtype = c->dtype; g.epilogue = MH_EPI_STORE;
    if (wh) g.bias = w->dec_cq_b[l];
    MH_TRY(gemm(g, s, false, plan_M));
    for (int b0 = 0; b0 < B; b0 += kvB) {   // under CFG both halves of the batch attend to the same kvB encoder rows
      a = AttnArgs{};
      a.q = (char*)pb.q + (long)b0 * np * inner * es; a.q_rs = (long)inner * es; a.q_bs = (long)np * inner * es;
      a.k = (const char*)cross_kv + (long)(l * 2 + 0) * kv_layer * es; a.k_rs = 64L * es; a.k_hs = (long)L * 64 * es;
      a.k_bs = (long)H * L * 64 * es;
      a.vt = (char*)pb.cross_vt + (long)l * kvB * inner * pb.Lpad * es; a.Lkpad = pb.Lpad; a.vt_hs = 64L * pb.Lpad * es;
      a.vt_bs = (long)H * 64 * pb.Lpad * es;
      a.out = (char*)pb.attn + (long)b0 * np * inner * es; a.out_rs = (long)inner * es; a.out_bs = (long)np * inner * es;
      a.Lq = np; a.Lk = L; a.scale = wh ? c->attn_scale : 1.0f;
      MH_TRY(attention_general(a, kvB, H, c->dtype, s));
    }
    g = MhGemm{};
    g.A = pb.attn; g.lda = inner; g.W = w->dec_co[l]; g.ldw = inner; g.C = pb.h; g.ldc = d; g.M = rows; g.N = d; g.K = inner;
    g.dtype = c->dtype; g.epilogue = MH_EPI_RESID;
    if (wh) g.bias = w->dec_co_b[l];
    MH_TRY(gemm(g, s, false, plan_M));
    // feed forward
    MH_TRY(pre_norm(c, pb.h, w->dec_ln3[l], w->dec_ln3_b[l], pb.n, rows, c->dtype, s));
    g = MhGemm{};
    g.A = pb.n; g.lda = d; g.W = w->dec_wi[l]; g.ldw = d; g.C = pb.ff; g.ldc = dff; g.M = rows; g.K = d;
    g.dtype = c->dtype;
    if (wh) { g.N = dff; g.epilogue = MH_EPI_BIAS_GELU_ERF; g.bias = w->dec_fc1_b[l]; }     // fc1 -> gelu(erf) (modeling_varwhisper.py:633-741)
    else { g.N = 2 * dff; g.epilogue = MH_EPI_GEGLU; }
    MH_TRY(gemm(g, s, false, plan_M));
    g = MhGemm{};
    g.A = pb.ff; g.lda = dff; g.W = w->dec_wo[l]; g.ldw = dff; g.C = pb.h; g.ldc = d; g.M = rows; g.N = d; g.K = dff;
    g.dtype = c->dtype; g.epilogue = MH_EPI_RESID;
    if (wh) g.bias = w->dec_fc2_b[l];
    MH_TRY(gemm(g, s, false, plan_M));
  }
  return MH_OK;
}
}  // namespace mh

// ------------------------------------------------------------------------------------------------
// Teacher-forced decoder forward over whole sequences: the `Mapperatorinator.forward` seam (B2,
// modeling_mapperatorinator.py:174-228) with `encoder_outputs` given -- every position of `ids` goes through the
// decoder stack at once (the batched prefill path: MFMA GEMMs + flash attention, causal + key mask), then the
// final RMSNorm and lm_head.  logits fp32 [B, T, V].
extern "C" int64_t mh_t5_forward_workspace_bytes(const MhT5Config* c, int B, int T) {
  mh::OptionScope option_scope(c ? c->options : nullptr);
  if (!c || B <= 0 || T <= 0) return -1;
  const int64_t es = es_of(c->dtype);
  return mh::prefill_layout(c, B, T, nullptr, 0, nullptr) +
         2 * mh::align256((int64_t)c->n_dec_layers * B * c->n_heads * 64 * c->tgt_len * es);
}

extern "C" int mh_t5_decoder_forward(const MhT5Config* c, const MhT5Weights* w, const void* cross_kv, int B,
                                     const int32_t* ids, const uint8_t* mask, int T, float* logits, void* workspace,
                                     int64_t workspace_bytes, void* stream) {
  mh::OptionScope option_scope(c ? c->options : nullptr);
  MH_TRY(check_cfg(c, "mh_t5_decoder_forward"));
  MH_REQUIRE(w && cross_kv && ids && logits && workspace, "mh_t5_decoder_forward: null argument");
  MH_REQUIRE(B > 0 && T >= 1 && T <= c->tgt_len, "mh_t5_decoder_forward: T=%d not in [1, tgt_len=%d]", T, c->tgt_len);
  MH_REQUIRE(workspace_bytes >= mh_t5_forward_workspace_bytes(c, B, T), "mh_t5_decoder_forward: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int es = es_of(c->dtype);
  const int64_t cache = align256((int64_t)c->n_dec_layers * B * c->n_heads * 64 * c->tgt_len * es);
  char* self_k = (char*)workspace;
  char* self_v = self_k + cache;
  PrefillBuf pb;
  prefill_layout(c, B, T, self_v + cache, workspace_bytes - 2 * cache, &pb);
  MH_TRY(prefill_prompt(c, w, cross_kv, B, B, ids, mask, T, T, self_k, self_v, pb, s));
  const int rows = B * T, d = c->d_model;
  MH_TRY(pre_norm(c, pb.h, w->dec_final_ln, w->dec_final_ln_b, pb.n, rows, c->dtype, s));
  MhGemm g{};
  g.A = pb.n; g.lda = d; g.W = w->lm_head; g.ldw = d; g.C = logits; g.ldc = c->vocab_out; g.M = rows; g.N = c->vocab_out;
  g.K = d; g.dtype = c->dtype; g.epilogue = MH_EPI_STORE_F32;
  return gemm(g, s);
}

// ------------------------------------------------------------------------------------------------
// Teacher-forced scoring: the decoder stack exactly as mh_t5_decoder_forward runs it, then final norm -> lm_head -> row
// statistics (score.hip) over the SCORED positions only, `score_block_rows` of them at a time through one fp32 logits scratch:
// B*T*V logits never exist.  The scored positions are compacted on the device (row-major (b, t) order, no host round trip); the
// LM-head GEMM of a block is planned as the whole [B*T, V] GEMM of the forward, so a position's logits -- and with them its
// statistics -- are bit for bit those of mh_t5_decoder_forward + mh_score_rows.
namespace mh {
namespace {
struct ScoreBuf { float* logits; float* hc; int32_t* map; int32_t* count; int C, ldv; };
int64_t score_layout(const MhT5Config* c, int B, int T, void* base, int64_t size, ScoreBuf* out) {
  Arena ar(base, size);
  const int64_t rows = (int64_t)B * T;
  long C = option(OPT_SCORE_BLOCK_ROWS);
  C = C < 1 ? 1 : C;
  ScoreBuf t;
  t.C = (int)(C < rows ? C : rows);
  // rows of the scratch start 16-byte aligned.  The forward stores its logits with ldc = V; the bf16 dispatch looks at ldc % 4
  // (`vec_ok`, gemm.hip dispatch_tile) only in a conjunction with N % 4, and N = V in both calls, so the rounding cannot select
  // another kernel than the forward's -- keep it that way (bit-equality with mh_t5_decoder_forward rests on the same kernel)
  t.ldv = round_up(c->vocab_out, 4);
  t.logits = (float*)ar.take((int64_t)t.C * t.ldv * 4);
  t.hc = (float*)ar.take((int64_t)t.C * c->d_model * 4);
  t.map = (int32_t*)ar.take(rows * 4);
  t.count = (int32_t*)ar.take(4);
  if (out) *out = t;
  return ar.off;
}
}  // namespace
}  // namespace mh

extern "C" int64_t mh_t5_score_workspace_bytes(const MhT5Config* c, int B, int T) {
  mh::OptionScope option_scope(c ? c->options : nullptr);
  if (!c || B <= 0 || T <= 0) return -1;
  return mh_t5_forward_workspace_bytes(c, B, T) + mh::score_layout(c, B, T, nullptr, 0, nullptr);
}

extern "C" int mh_t5_score(const MhT5Config* c, const MhT5Weights* w, const void* cross_kv, int B, const int32_t* ids,
                           const uint8_t* mask, int T, const int32_t* targets, int max_scored, float* surprisal, float* entropy,
                           float* relative, float* logprob, int32_t* best_id, void* workspace, int64_t workspace_bytes,
                           void* stream) {
  mh::OptionScope option_scope(c ? c->options : nullptr);
  MH_TRY(check_cfg(c, "mh_t5_score"));
  MH_REQUIRE(w && cross_kv && ids && targets && surprisal && entropy && relative && logprob && best_id && workspace,
             "mh_t5_score: null argument");
  MH_REQUIRE(B > 0, "mh_t5_score: batch %d must be positive", B);
  MH_REQUIRE(T >= 1 && T <= c->tgt_len, "mh_t5_score: T=%d not in [1, tgt_len=%d]", T, c->tgt_len);
  MH_REQUIRE((int64_t)B * T <= INT32_MAX, "mh_t5_score: B*T = %lld positions exceed the int32 index range", (long long)B * T);
  MH_REQUIRE(workspace_bytes >= mh_t5_score_workspace_bytes(c, B, T), "mh_t5_score: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int es = es_of(c->dtype);
  const int64_t fwd = mh_t5_forward_workspace_bytes(c, B, T);
  const int64_t cache = align256((int64_t)c->n_dec_layers * B * c->n_heads * 64 * c->tgt_len * es);
  char* self_k = (char*)workspace;
  char* self_v = self_k + cache;
  PrefillBuf pb;
  prefill_layout(c, B, T, self_v + cache, fwd - 2 * cache, &pb);
  ScoreBuf sb;
  score_layout(c, B, T, (char*)workspace + fwd, workspace_bytes - fwd, &sb);
  MH_TRY(prefill_prompt(c, w, cross_kv, B, B, ids, mask, T, T, self_k, self_v, pb, s));
  const int rows = B * T, d = c->d_model, V = c->vocab_out;
  MH_TRY(score_compact(targets, rows, V, sb.map, sb.count, surprisal, entropy, relative, logprob, best_id, s));
  const int cap = (max_scored >= 0 && max_scored < rows) ? max_scored : rows;   // negative: unknown, every position may be scored
  for (int base = 0; base < cap; base += sb.C) {
    // the block's hidden rows (zeros behind the end of the list) -> final norm (pb.n is free after the stack) -> logits -> statistics
    MH_TRY(score_gather(pb.h, d, sb.map, sb.count, base, cap, sb.hc, sb.C, s));
    MH_TRY(pre_norm(c, sb.hc, w->dec_final_ln, w->dec_final_ln_b, pb.n, sb.C, c->dtype, s));
    MhGemm g{};
    g.A = pb.n; g.lda = d; g.W = w->lm_head; g.ldw = d; g.C = sb.logits; g.ldc = sb.ldv; g.M = sb.C; g.N = V;
    g.K = d; g.dtype = c->dtype; g.epilogue = MH_EPI_STORE_F32;
    MH_TRY(gemm(g, s, false, rows));
    MH_TRY(score_rows(sb.logits, sb.ldv, sb.C, V, targets, sb.map, sb.count, base, cap, surprisal, entropy, relative, logprob,
                      best_id, s));
  }
  return MH_OK;
}
