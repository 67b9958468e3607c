// osuT5 on MI355X: encoder stack, cross-attention K/V projection and the KV-cached AR decode loop.
// Orchestration lives here (C++), so that the per-token loop never returns to Python: every decode
// step is one hipGraph replay; the host only polls a 4-byte "rows still running" word.
//
// Reference semantics reproduced (see include/mapperhip.h for the per-entry citations):
//   HF T5Stack / T5Block / T5Attention / T5LayerFF (pre-norm residual blocks, shared layer-0 relative
//   bias, no 1/sqrt(d) scaling, gated gelu_new FFN), HF GenerationMixin._sample under
//   model_generate (osuT5/osuT5/inference/server.py:83-156) with the reference logits processors.
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "decode_kernels.hpp"

namespace mh {
namespace {

inline int es_of(int dtype) { return dtype == MH_BF16 ? 2 : 4; }

int check_cfg(const MhT5Config* c, const char* who) {
  MH_REQUIRE(c, "%s: null config", who);
  MH_REQUIRE(c->d_kv == 64, "%s: d_kv must be 64 (got %d)", who, c->d_kv);
  MH_REQUIRE(c->n_enc_layers <= MH_MAX_LAYERS && c->n_dec_layers <= MH_MAX_LAYERS, "%s: too many layers", who);
  MH_REQUIRE(c->d_model % 32 == 0 && c->d_ff % 32 == 0, "%s: d_model/d_ff must be multiples of 32", who);
  MH_REQUIRE(c->n_mels_pad % 32 == 0 && c->n_mels_pad >= c->n_mels, "%s: bad n_mels_pad", who);
  MH_REQUIRE(c->dtype == MH_F32 || c->dtype == MH_BF16, "%s: bad dtype", who);
  MH_REQUIRE(c->arch >= 0 && c->arch <= 2, "%s: arch %d is none of 0 (T5), 1 (VarWhisper / RoPEWhisper), 2 (HF Whisper)", who, c->arch);
  MH_REQUIRE(c->dec_pos_from_mask == 0 || c->arch == 2, "%s: dec_pos_from_mask belongs to arch 2 (absolute decoder positions)", who);
  if (c->arch >= 1) {
    MH_REQUIRE(c->d_model == c->n_heads * 64, "%s: the Whisper family needs d_model = 64 heads", who);
    MH_REQUIRE(c->in_frames >= 1 && c->src_len == (c->in_frames - 1) / 2 + 1, "%s: src_len must be the conv-strided in_frames", who);
    MH_REQUIRE(c->attn_scale > 0.f, "%s: attn_scale must be positive", who);
  }
  MH_REQUIRE(c->enc_operand_dtype == 0 || c->enc_operand_dtype == MH_MX8, "%s: enc_operand_dtype must be 0 or MH_MX8", who);
  if (c->enc_operand_dtype == MH_MX8)
    MH_REQUIRE(c->dtype == MH_BF16 && c->arch == 0 && c->d_model % 128 == 0 && c->d_ff % 128 == 0,
               "%s: MX-fp8 encoder operands need bf16 storage, the T5 backbone and d_model / d_ff multiples of 128", who);
  return MH_OK;
}
// the token step's attention kernels project their own q (/ k / v) from the whole residual row: d_model = 128 KC, KC in 1..8
// (mh_t5_generate, mh_t5_step, mh_t5_cross_attn_probe; the encoder, cross K/V and teacher-forced forward take any shape check_cfg does)
int check_decode_shape(const MhT5Config* c, const char* who) {
  MH_REQUIRE(c->d_model % 128 == 0 && c->d_model >= 128 && c->d_model <= 1024,
             "%s: the decode step needs d_model a multiple of 128 in [128, 1024] (got %d)", who, c->d_model);
  return MH_OK;
}
inline bool enc_mx(const MhT5Config* c) { return c->enc_operand_dtype == MH_MX8; }
inline int64_t mx_operand_bytes(int64_t rows, int K) { return align256(rows * K) + align256(rows * mx8_scale_row_bytes(K)); }
// the pre-norm of a block: T5LayerNorm / nn.RMSNorm (arch 0 / 1) or the affine nn.LayerNorm of HF Whisper (arch 2, bias != NULL there)
inline int pre_norm(const MhT5Config* c, const float* x, const float* w, const float* b, void* y, int rows, int out_dtype, hipStream_t s) {
  if (c->arch == 2) {
    MH_REQUIRE(b, "arch 2 needs the LayerNorm biases (MhT5Weights.*_ln*_b)");
    return layernorm(x, c->d_model, w, b, y, c->d_model, rows, c->d_model, c->eps, out_dtype, s);
  }
  return rmsnorm(x, c->d_model, w, y, c->d_model, rows, c->d_model, c->eps, out_dtype, s);
}
inline bool is_local_layer(const MhT5Config* c, int l) { return c->arch == 1 && c->local_every > 1 && c->local_window > 0 && l % c->local_every != 0; }

#define MH_TRY(expr)              \
  do {                            \
    int _rc = (expr);             \
    if (_rc != MH_OK) return _rc; \
  } while (0)

// f(a value of the storage type): one call site for both instantiations of a kernel or launcher (`using T = decltype(t)`)
template <typename F>
auto dispatch_dtype(int dtype, F&& f) { return dtype == MH_BF16 ? f(bf16_t{}) : f(float{}); }
// f(std::integral_constant<int, KC>) for d_model = 128 KC of the attention kernels that project their own q (/ k / v), KC in 1..7;
// any other d_model runs KC = 8 (check_decode_shape guards the range)
template <int KC = 1, typename F>
int dispatch_kc(int d, F&& f) {
  if constexpr (KC == 8) return f(std::integral_constant<int, 8>{});
  else return d == 128 * KC ? f(std::integral_constant<int, KC>{}) : dispatch_kc<KC + 1>(d, f);
}
// THE form table.  A decode attention kernel exists in exactly three forms, (rotary / scaled scores, affine LayerNorm) =
//   (false, false)  T5: bias-free projections behind an RMS norm, relative position bias, unscaled scores
//   (true,  false)  rotary Whisper: biased fused projections, RoPE, scaled scores, optional window
//   (true,  true)   HF Whisper (arch 2): the same behind an affine LayerNorm, identity rotary table
// f(std::bool_constant, std::bool_constant) with one of these three pairs; (false, true) is no model and is never instantiated
template <typename F>
void dispatch_attn_form(bool rope_or_scaled, bool ln_b, F&& f) {
  if (rope_or_scaled && ln_b) f(std::true_type{}, std::true_type{});
  else if (rope_or_scaled) f(std::true_type{}, std::false_type{});
  else f(std::false_type{}, std::false_type{});
}
int check_arch2_weights(const MhT5Config* c, const MhT5Weights* w, const char* who) {
  MH_REQUIRE(c->arch != 2 || (w->dec_pos && w->dec_final_ln_b), "%s: arch 2 needs decoder.embed_positions and the LayerNorm biases", who);
  return MH_OK;
}

// The packed e4m3 copies the token steps stream, laid out HERE and nowhere else: 2 n_dec_layers planes (layer, k | v) of `n` units of
// `unit_bytes` e4m3 bytes, then -- 256-byte aligned -- one fp32 scale per unit, plane by plane
struct Kv8Layout {
  int64_t plane_bytes, plane_scales;   // one plane: its e4m3 bytes, its scales
  int64_t scales_offset, total;        // bytes from the start of the copy to its scales, bytes of the whole copy
  int64_t data(int l, int kv) const { return (int64_t)(l * 2 + kv) * plane_bytes; }     // byte offset of plane (l, kv)
  int64_t scale(int l, int kv) const { return (int64_t)(l * 2 + kv) * plane_scales; }   // index of its first scale
};
inline Kv8Layout kv8_layout(const MhT5Config* c, int64_t n, int64_t unit_bytes) {
  const int64_t planes = 2 * (int64_t)c->n_dec_layers, data = align256(planes * n * unit_bytes);
  return {n * unit_bytes, n, data, data + align256(planes * n * 4)};
}
// cross K/V of kvB rows (mh_t5_quantize_cross_kv): a unit = one (row, head) slab of src_len x 64; the shadow of the self-attention
// cache of B rows (mh_t5_generate_skv8): a unit = one cached row of 64 at (row, head, position)
inline Kv8Layout cross_kv8_layout(const MhT5Config* c, int kvB) { return kv8_layout(c, (int64_t)kvB * c->n_heads, (int64_t)c->src_len * 64); }
inline Kv8Layout self_kv8_layout(const MhT5Config* c, int B) { return kv8_layout(c, (int64_t)B * c->n_heads * c->tgt_len, 64); }

}  // namespace
}  // namespace mh

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
// decode
// ------------------------------------------------------------------------------------------------
namespace mh {
namespace {

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

constexpr int kMaxChains = 8;

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
void step_call_init(StepCall* k, const MhT5Config* c, const MhT5Weights* w) {
  memset(k, 0, sizeof(*k));
  k->c = c; k->w = w; k->timing_buf = g_timing.buf; k->timing_ring = g_timing.ring;
}

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
// cache rows [l][b][h][0 .. n_pos) <- [l][src[b]][h][..]: gather into `tmp`, then copy back (in place would read rows that
// were already overwritten); one workgroup per (k|v, layer, row, head)
template <typename T>
__global__ __launch_bounds__(256) void cache_gather_kernel(const T* kc, const T* vc, T* tmp, const int32_t* src, int B, int H, int tgt,
                                                          int n_pos, long layer_stride) {
  const int h = blockIdx.x % H, b = (blockIdx.x / H) % B, l = (blockIdx.x / H / B) % (int)gridDim.y, kv = blockIdx.z;
  const T* from = (kv ? vc : kc) + (long)blockIdx.y * layer_stride + ((long)src[b] * H + h) * tgt * 64;
  T* to = tmp + ((((long)kv * gridDim.y + blockIdx.y) * B + b) * H + h) * (long)n_pos * 64;
  (void)l;
  const uint4* f4 = reinterpret_cast<const uint4*>(from);
  uint4* t4 = reinterpret_cast<uint4*>(to);
  const int n16 = n_pos * 64 * (int)sizeof(T) / 16;
  for (int i = threadIdx.x; i < n16; i += 256) t4[i] = f4[i];
}
template <typename T>
__global__ __launch_bounds__(256) void cache_scatter_kernel(T* kc, T* vc, const T* tmp, int B, int H, int tgt, int n_pos, long layer_stride) {
  const int h = blockIdx.x % H, b = (blockIdx.x / H) % B, kv = blockIdx.z;
  T* to = (kv ? vc : kc) + (long)blockIdx.y * layer_stride + ((long)b * H + h) * tgt * 64;
  const T* from = tmp + ((((long)kv * gridDim.y + blockIdx.y) * B + b) * H + h) * (long)n_pos * 64;
  const uint4* f4 = reinterpret_cast<const uint4*>(from);
  uint4* t4 = reinterpret_cast<uint4*>(to);
  const int n16 = n_pos * 64 * (int)sizeof(T) / 16;
  for (int i = threadIdx.x; i < n16; i += 256) t4[i] = f4[i];
}

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

struct PrefillBuf {
  float* h; void* n; void* q; void* attn; void* ff; void* vt; void* cross_vt;
  int np_pad, Lpad;
};

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
                   int cache_rows = 0) {
  // P = row stride of `prompt` / `prompt_mask`, np <= P = positions that go through the stack
  // cache_rows: rows of the caches self_k / self_v point into (their layer stride); 0 = B.  More than B (mh_t5_step_prefill): the
  // B prompts fill cache rows 0 .. B-1 of every layer
  if (cache_rows <= 0) cache_rows = B;
  const int rows = B * np;
  const int d = c->d_model, H = c->n_heads, inner = H * 64, dff = c->d_ff, L = c->src_len, tgt = c->tgt_len;
  const int es = es_of(c->dtype);
  const int np_pad = round_up(np, 64);
  // arch 1 (VarWhisperDecoderLayer, modeling_varwhisper.py:633-741) through the same batched form: biased projections,
  // rotate-half RoPE on q and on the cached keys, scores / 8 without a relative bias, fc1 -> gelu(erf) -> fc2.  A local
  // (windowed) layer takes its own rotary table and the causal attention gets the band |k - q| <= local_window on top -- the
  // keys the token-by-token step attends (decode_kernels.hpp `window`).
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
    MH_TRY(gemm(g, s));
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
    MH_TRY(gemm(g, s));
    // cross attention of every prompt position over the encoder keys
    MH_TRY(pre_norm(c, pb.h, w->dec_ln2[l], w->dec_ln2_b[l], pb.n, rows, c->dtype, s));
    g = MhGemm{};
    g.A = pb.n; g.lda = d; g.W = w->dec_cq[l]; g.ldw = d; g.C = pb.q; g.ldc = inner; g.M = rows; g.N = inner; g.K = d;
    g.dtype = c->dtype; g.epilogue = MH_EPI_STORE;
    if (wh) g.bias = w->dec_cq_b[l];
    MH_TRY(gemm(g, s));
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
    MH_TRY(gemm(g, s));
    // feed forward
    MH_TRY(pre_norm(c, pb.h, w->dec_ln3[l], w->dec_ln3_b[l], pb.n, rows, c->dtype, s));
    g = MhGemm{};
    g.A = pb.n; g.lda = d; g.W = w->dec_wi[l]; g.ldw = d; g.C = pb.ff; g.ldc = dff; g.M = rows; g.K = d;
    g.dtype = c->dtype;
    if (wh) { g.N = dff; g.epilogue = MH_EPI_BIAS_GELU_ERF; g.bias = w->dec_fc1_b[l]; }     // fc1 -> gelu(erf) (modeling_varwhisper.py:633-741)
    else { g.N = 2 * dff; g.epilogue = MH_EPI_GEGLU; }
    MH_TRY(gemm(g, s));
    g = MhGemm{};
    g.A = pb.ff; g.lda = dff; g.W = w->dec_wo[l]; g.ldw = dff; g.C = pb.h; g.ldc = d; g.M = rows; g.N = d; g.K = dff;
    g.dtype = c->dtype; g.epilogue = MH_EPI_RESID;
    if (wh) g.bias = w->dec_fc2_b[l];
    MH_TRY(gemm(g, s));
  }
  return MH_OK;
}

// Independent rows => independent "chains": the batch is cut into contiguous blocks of rows and every
// block runs its own captured decode step on its own stream.  A decode step is ~110 dependent, mostly
// tiny kernels (each costs a few microseconds of dispatch + drain whatever its size), so one chain leaves
// the GPU idle most of the time; several chains overlap one another's dispatch gaps and let the
// HBM-bound cross-attention of one chain run under the latency-bound GEMVs of the others.  Results do not
// depend on the chain count (every kernel is batch-invariant by construction).
int pick_chains(int B) {
  int n = B >= 16 ? 2 : 1;   // measured on MI355X (B=32, base): 1 -> 26.7k, 2 -> 28.0k, 4 -> 17.6k tok/s (host graph-launch bound)
  if (option(OPT_DECODE_CHAINS) >= 1) n = (int)option(OPT_DECODE_CHAINS);
  if (n > kMaxChains) n = kMaxChains;
  if (n > B) n = B;
  return n;
}

struct ChainPool {   // extra streams + fork/join events of ONE device, created on first use under that device
  hipStream_t streams[kMaxChains] = {};
  hipEvent_t fork = nullptr, join[kMaxChains] = {};
  bool ready = false;
  int init() {
    if (ready) return MH_OK;
    if (hipEventCreateWithFlags(&fork, hipEventDisableTiming) != hipSuccess) return check_launch("event create");
    for (int i = 0; i < kMaxChains; ++i) {
      if (hipStreamCreateWithFlags(&streams[i], hipStreamNonBlocking) != hipSuccess ||
          hipEventCreateWithFlags(&join[i], hipEventDisableTiming) != hipSuccess)
        return check_launch("chain stream create");
    }
    ready = true;
    return MH_OK;
  }
};
// one pool per device; mh_t5_generate holds the pool's mutex for the whole call, so two engines (or two host
// threads) decoding on the same GPU take turns instead of sharing fork / join events
struct DevicePool { ChainPool pool; std::mutex mu; };
DevicePool* device_pool(int dev) {
  static std::mutex table_mu;
  static std::map<int, DevicePool*> table;
  std::lock_guard<std::mutex> g(table_mu);
  auto it = table.find(dev);
  if (it == table.end()) it = table.emplace(dev, new DevicePool()).first;
  return it->second;
}

}  // namespace
}  // namespace mh

extern "C" int64_t mh_t5_decode_workspace_bytes(const MhT5Config* c, int B) {
  mh::OptionScope option_scope(c ? c->options : nullptr);
  if (!c || B <= 0) return -1;
  return decode_layout(c, B, nullptr).end + prefill_layout(c, B, c->tgt_len - 1, nullptr, 0, nullptr);   // + batched prompt prefill
}

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

// positions 0 .. n_pos-1 of cache rows 0 .. n_rows-1 of a B-row batch's bf16 self-attention caches -> the B-row shadow self8, every
// layer, k and v
static int launch_self_kv_quant_rows(const MhT5Config* c, int B, const DecBuffers& bf, uint8_t* self8, int n_rows, int n_pos, hipStream_t s) {
  const long n_slabs = (long)n_rows * c->n_heads, plane_rows = (long)B * c->n_heads * c->tgt_len;
  hipLaunchKernelGGL(self_kv_quant_rows_kernel, dim3((unsigned)((n_slabs * n_pos + 3) / 4), 2 * c->n_dec_layers), dim3(256), 0, s,
                     (const bf16_t*)bf.self_k, (const bf16_t*)bf.self_v, self8,
                     reinterpret_cast<float*>(self8 + self_kv8_layout(c, B).scales_offset), n_slabs, (long)n_pos, (long)c->tgt_len, plane_rows);
  return check_launch("self_kv_quant_rows_kernel");
}

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

extern "C" int mh_t5_decode_self_cache(const MhT5Config* c, int B, void* workspace, void** k, void** v) {
  mh::OptionScope option_scope(c ? c->options : nullptr);
  MH_TRY(check_cfg(c, "mh_t5_decode_self_cache"));
  MH_REQUIRE(workspace && k && v && B > 0, "mh_t5_decode_self_cache: null argument");
  const mh::DecodeLayout ly = mh::decode_layout(c, B, workspace);
  *k = ly.bf.self_k;
  *v = ly.bf.self_v;
  return MH_OK;
}

namespace mh {
// ------------------------------------------------------------------------------------------------
// Instantiated step graphs kept ACROSS mh_t5_generate calls.  A chain's step graph bakes in nothing but addresses, sizes, the
// sampling struct and the kernel choice (the position and every per-call state live in device memory), so a later call
// whose inputs are byte-for-byte the same description -- the normal case of an engine that decodes window after window out
// of the same workspace with the same prompt length -- replays the graph of the earlier one instead of capturing and
// instantiating ~75 nodes again.  The key comes from ONE place: step_graph_key() over the StepCall that enqueue_step() is given,
// the only thing it reads besides the options -- so whatever a step depends on is in its key (exact compare: a spurious
// difference costs a capture, never a wrong graph).  Small LRU; an entry in use by a concurrent call is never shared
// (hipGraphExec objects are single-flight) nor evicted.  Option decode_graph_cache = 0 switches it off.
struct StepGraphEntry {
  std::vector<unsigned char> key;      // step_graph_key(StepCall)
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  uint64_t stamp = 0;
  bool in_use = false;
};
constexpr size_t kStepGraphCacheMax = 16;
static std::mutex g_step_graph_mu;
static std::vector<StepGraphEntry*> g_step_graphs;
static uint64_t g_step_graph_clock = 0;
static std::atomic<long> g_step_graph_hits{0}, g_step_graph_misses{0};

// The bytes of the StepCall, then what it depends on beyond them: *c without the address of its option set, *w, every option value,
// the device, the storage type.  Scrubbed, here and nowhere else: the addresses of c and w (their contents follow); seed and rng_row0
// (they reach the sampler through DecState, not through the graph); under the row form what that sampler reads per row instead.
static std::vector<unsigned char> step_graph_key(const StepCall& call) {
  std::vector<unsigned char> key;
  auto put = [&key](const void* p, size_t n) { key.insert(key.end(), (const unsigned char*)p, (const unsigned char*)p + n); };
  StepCall k;
  memcpy(&k, &call, sizeof(k));
  k.c = nullptr; k.w = nullptr;
  MhSampling& sp = k.smp.sp;
  sp.seed = 0; sp.rng_row0 = 0;
  if (k.has_rows) {
    k.smp.eos_table = nullptr;
    sp.cfg_scale = sp.cfg_scale > 1.0f ? 2.f : 1.f;   // (guidance on / off is the call's, the scale each pair's own)
    sp.temperature = sp.top_p = sp.timeshift_bias = 0.f;
    sp.top_k = sp.lookback_mask_end = 0;
    for (int j = 0; j < 3; ++j) sp.cond_temp[j] = 0.f;
  }
  MhT5Config cc = *call.c;
  cc.options = nullptr;
  long opts[OPT_COUNT];
  for (int o = 0; o < OPT_COUNT; ++o) opts[o] = option(o);
  int dev_id = 0;
  (void)hipGetDevice(&dev_id);
  const int ids[2] = {dev_id, call.c->dtype == MH_BF16 ? 1 : 0};
  put(&k, sizeof(k)); put(&cc, sizeof(cc)); put(call.w, sizeof(*call.w)); put(opts, sizeof(opts)); put(ids, sizeof(ids));
  return key;
}

static StepGraphEntry* step_graph_acquire(const std::vector<unsigned char>& key) {
  std::lock_guard<std::mutex> lk(g_step_graph_mu);
  for (StepGraphEntry* e : g_step_graphs)
    if (!e->in_use && e->key == key) {
      e->in_use = true;
      e->stamp = ++g_step_graph_clock;
      return e;
    }
  return nullptr;
}

// takes ownership of graph / exec; returns the entry (in use) -- or nullptr when the cache is full of entries in use
static StepGraphEntry* step_graph_insert(std::vector<unsigned char>&& key, hipGraph_t graph, hipGraphExec_t exec) {
  std::lock_guard<std::mutex> lk(g_step_graph_mu);
  while (g_step_graphs.size() >= kStepGraphCacheMax) {
    int victim = -1;
    for (size_t i = 0; i < g_step_graphs.size(); ++i)
      if (!g_step_graphs[i]->in_use && (victim < 0 || g_step_graphs[i]->stamp < g_step_graphs[victim]->stamp)) victim = (int)i;
    if (victim < 0) return nullptr;
    StepGraphEntry* v = g_step_graphs[victim];
    (void)hipGraphExecDestroy(v->exec);
    (void)hipGraphDestroy(v->graph);
    delete v;
    g_step_graphs.erase(g_step_graphs.begin() + victim);
  }
  StepGraphEntry* e = new StepGraphEntry();
  e->key = std::move(key);
  e->graph = graph;
  e->exec = exec;
  e->in_use = true;
  e->stamp = ++g_step_graph_clock;
  g_step_graphs.push_back(e);
  return e;
}

static void step_graph_release(StepGraphEntry* e) {
  std::lock_guard<std::mutex> lk(g_step_graph_mu);
  e->in_use = false;
}

// The device that owns the caller's stream (not whatever happens to be current)
static int stream_device(hipStream_t s, int* dev) {
  if (hipStreamGetDevice(s, dev) != hipSuccess) { (void)hipGetLastError(); if (hipGetDevice(dev) != hipSuccess) return check_launch("hipGetDevice"); }
  return MH_OK;
}
// Streams, events and graphs of a call or a session are created under that device; the current one is restored on every return path
struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int want) { if (hipGetDevice(&prev) == hipSuccess && prev != want) (void)hipSetDevice(want); else prev = -1; }
  ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// A chain of the running call and the owner of its step graph: the cross-call cache (`cached`: handed back when the call ends) or the
// call itself (destroyed with it, after the call's last synchronise)
struct Chain {
  hipStream_t stream = nullptr; DecState* st = nullptr;
  hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr; StepGraphEntry* cached = nullptr;
  Chain() = default;
  Chain(const Chain&) = delete;
  Chain& operator=(const Chain&) = delete;
  ~Chain() {
    if (cached) { step_graph_release(cached); return; }
    if (exec) (void)hipGraphExecDestroy(exec);
    if (graph) (void)hipGraphDestroy(graph);
  }
};

// A chain enters the call on its own stream, behind the caller's work so far (`fork`): dec_init_kernel, then one step of the chain (every
// kernel reads the position from device memory) as a graph for replay: an earlier call's, if its key is this one's, else captured now
static int chain_step_graph(const StepCall& call, const char* who, Chain* ch);
static int start_chain(const StepCall& call, int start_pos, hipEvent_t fork, const char* who, Chain* ch) {
  hipStream_t cs = ch->stream;
  ch->st = call.bf.st;
  if (hipStreamWaitEvent(cs, fork, 0) != hipSuccess) return check_launch("fork wait");
  if (call.c->dtype == MH_BF16) hipLaunchKernelGGL(dec_init_kernel<bf16_t>, dim3(call.Bc), dim3(256), 0, cs, call.smp, call.Bc, start_pos);
  else hipLaunchKernelGGL(dec_init_kernel<float>, dim3(call.Bc), dim3(256), 0, cs, call.smp, call.Bc, start_pos);
  MH_TRY(check_launch("dec_init_kernel"));
  return chain_step_graph(call, who, ch);
}
// One step of the chain as a graph for replay on ch->stream: an earlier call's, if its key is this one's, else captured now
static int chain_step_graph(const StepCall& call, const char* who, Chain* ch) {
  hipStream_t cs = ch->stream;
  std::vector<unsigned char> key;
  if (option(OPT_DECODE_GRAPH_CACHE) != 0) {
    key = step_graph_key(call);
    if ((ch->cached = step_graph_acquire(key))) { ch->exec = ch->cached->exec; g_step_graph_hits.fetch_add(1); return MH_OK; }
    g_step_graph_misses.fetch_add(1);
  }
  if (hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal) != hipSuccess) return check_launch("begin capture");
  const int rce = dispatch_dtype(call.c->dtype, [&](auto t) { return enqueue_step<decltype(t)>(call, cs); });
  const hipError_t ce = hipStreamEndCapture(cs, &ch->graph);
  if (rce != MH_OK) return rce;
  if (ce != hipSuccess || !ch->graph) { set_error("%s: stream capture failed: %s", who, hipGetErrorString(ce)); return MH_ERR_LAUNCH; }
  if (hipGraphInstantiate(&ch->exec, ch->graph, nullptr, nullptr, 0) != hipSuccess) return check_launch("graph instantiate");
  if (!key.empty() && (ch->cached = step_graph_insert(std::move(key), ch->graph, ch->exec))) ch->graph = nullptr;   // the cache owns both now
  return MH_OK;
}

// The host's look at a chain between two bursts of replays: DecState::n_running and ::tail_err in one 8-byte read
static int poll_chain(const Chain& ch, bool* running) {
  int word[2] = {1, 0};
  if (hipMemcpyAsync(word, &ch.st->n_running, 8, hipMemcpyDeviceToHost, ch.stream) != hipSuccess ||
      hipStreamSynchronize(ch.stream) != hipSuccess)
    return MH_ERR_LAUNCH;
  *running = word[0] != 0;
  return word[1] != 0 ? MH_ERR_DECODE_TAIL_TIMEOUT : MH_OK;
}

// The one burst-and-poll loop, of a uniform call and of a slot session alike.  The launcher of chains which[0 .. n) from the calling
// thread: bursts of poll_every replays each, interleaved, then a poll of each (none behind the last burst, none under teacher forcing:
// poll = false).  A chain is left out once its rows are done or it failed (rcs[chain]); replays[chain], if given, counts its
// hipGraphLaunch calls that succeeded.
static void run_chains(const Chain* chains, const int* which, int n, int n_steps, int poll_every, bool poll, int* rcs, int* replays) {
  bool alive[kMaxChains];
  for (int i = 0; i < n; ++i) alive[i] = true;
  for (int step = 0; step < n_steps;) {
    const int burst = n_steps - step < poll_every ? n_steps - step : poll_every;
    for (int r = 0; r < burst; ++r)
      for (int i = 0; i < n; ++i) {
        const int ci = which[i];
        if (!alive[i] || rcs[ci] != MH_OK) continue;
        if (hipGraphLaunch(chains[ci].exec, chains[ci].stream) != hipSuccess) rcs[ci] = MH_ERR_LAUNCH;
        else if (replays) ++replays[ci];
      }
    step += burst;
    bool any = false;
    for (int i = 0; i < n; ++i) {
      const int ci = which[i];
      if (!alive[i] || rcs[ci] != MH_OK) continue;
      if (step < n_steps && poll && (rcs[ci] = poll_chain(chains[ci], &alive[i])) != MH_OK) continue;
      any = any || alive[i];
    }
    if (!any) break;
  }
}
// Replaying a ~110-node graph costs ~0.4 ms of HOST time on ROCm 7.2, so every running chain gets a launcher thread of its own (the
// chains are independent; the first runs on the calling thread); option decode_launch_threads = 0: one launcher for all, their bursts
// interleaved (slower on the host side; the same kernels and arguments).  which: the chains that run -- all of a uniform call, those
// with a live slot of a session.  -> the call's status, the failed chain named by its index
static int launch_chains(const Chain* chains, const int* which, int n, int n_steps, int poll_every, bool poll, const char* who,
                         int* replays = nullptr) {
  int rcs[kMaxChains] = {};
  if (n <= 1 || option(OPT_DECODE_LAUNCH_THREADS) == 0) {
    run_chains(chains, which, n, n_steps, poll_every, poll, rcs, replays);
  } else {
    std::vector<std::thread> th;
    const MhOptionSet* set = current_option_set();   // thread-local in the caller: re-installed in every launcher
    for (int i = 1; i < n; ++i)
      th.emplace_back([&, i, set] { OptionScope sc(set); run_chains(chains, which + i, 1, n_steps, poll_every, poll, rcs, replays); });
    run_chains(chains, which, 1, n_steps, poll_every, poll, rcs, replays);
    for (auto& t : th) t.join();
  }
  int rc = MH_OK;
  for (int i = 0; i < n; ++i) {
    const int ci = which[i];
    if (rcs[ci] == MH_ERR_DECODE_TAIL_TIMEOUT) rc = mh_t5_decode_tail_status(1);
    else if (rcs[ci] != MH_OK) { set_error("%s: graph launch / poll failed on chain %d: %s", who, ci, hipGetErrorString(hipGetLastError())); rc = rcs[ci]; }
  }
  return rc;
}

// What mh_t5_generate, mh_t5_generate_skv8 (self_kv_fp8: the caller's e4m3 shadow of the self-attention cache, else NULL) and
// mh_t5_generate_rows (rowset: the sampler's settings per returned row, else NULL) were given; who: the entry, for error messages
struct GenerateArgs {
  const MhT5Config* c; const MhT5Weights* w; const void* cross_kv; int B; const int32_t* prompt; const uint8_t* prompt_mask; int P;
  const uint8_t* eos_table; const MhSampling* sp; int32_t* tokens; int32_t* n_steps_out; float* logits_dump; const int32_t* forced;
  void* workspace; int64_t workspace_bytes; int poll_every; void* stream; void* self_kv_fp8; const RowSetP* rowset; const char* who;
};

// What every entry that runs the sampled token step checks of its configuration and settings, in this order (ptrs_ok: the entry's own
// pointer arguments are all there; P: the call's prompt length, or NULL where every row brings its own -- mh_t5_slots_admit checks it)
static int check_decode_call(const MhT5Config* c, const MhT5Weights* w, const MhSampling* sp, int B, bool ptrs_ok, void* stream,
                             const int* P, bool rows, const char* who) {
  MH_TRY(check_cfg(c, who));
  MH_TRY(check_decode_shape(c, who));
  MH_REQUIRE(w && sp && ptrs_ok, "%s: null argument", who);
  MH_REQUIRE(stream != nullptr, "%s: needs a non-default stream (hipGraph capture)", who);
  MH_REQUIRE(B > 0 && B <= 64, "%s: batch %d not in [1, 64] (shard larger batches on the host)", who, B);
  MH_REQUIRE(!P || (*P >= 1 && *P < sp->max_length), "%s: prompt length %d must be in [1, max_length)", who, P ? *P : 0);
  MH_REQUIRE(sp->max_length >= 2, "%s: max_length %d must be >= 2", who, sp->max_length);
  MH_REQUIRE(sp->max_length <= c->tgt_len, "%s: max_length %d exceeds tgt_len %d", who, sp->max_length, c->tgt_len);
  MH_REQUIRE(rows || sp->temperature > 0.f, "%s: temperature must be > 0", who);
  MH_REQUIRE(sp->n_sos >= 0 && sp->n_sos <= 16, "%s: too many sos ids", who);
  MH_REQUIRE(!(sp->cfg_scale > 1.0f) || B % 2 == 0, "%s: classifier-free guidance needs an even batch (negative rows, then prompt rows)", who);
  MH_REQUIRE(sp->n_cond >= 0 && sp->n_cond <= 3, "%s: n_cond %d not in [0, 3]", who, sp->n_cond);
  for (int j = 0; j < sp->n_cond; ++j)
    MH_REQUIRE((rows || sp->cond_temp[j] > 0.f) && sp->cond_offset[j] >= 1, "%s: bad conditional temperature rule %d", who, j);
  MH_REQUIRE(sp->tok_flags || (sp->n_cond == 0 && !sp->lookback_types_first),
             "%s: tok_flags is required by the conditional temperature / types_first lookback processors", who);
  MH_REQUIRE(!sp->cross_kv_fp8 || c->dtype == MH_BF16, "%s: cross_kv_fp8 needs bf16 storage", who);
  return MH_OK;
}

// The row settings of mh_t5_generate_rows (one entry per: "returned row") and of mh_t5_slots_open ("slot")
static int check_row_set(const MhRowSampling* rows, const uint8_t* eos_tables, int n_eos_sets, const char* per, const char* who) {
  MH_REQUIRE(rows && eos_tables, "%s: null argument (rows: one MhRowSampling per %s; eos_tables: [n_eos_sets][vocab_out])", who, per);
  MH_REQUIRE(n_eos_sets >= 1, "%s: n_eos_sets %d must be >= 1", who, n_eos_sets);
  return MH_OK;
}

static int check_generate_args(const GenerateArgs& a) {
  const bool ptrs_ok = a.cross_kv && a.prompt && (a.eos_table || a.rowset) && a.tokens && a.n_steps_out && a.workspace;
  MH_TRY(check_decode_call(a.c, a.w, a.sp, a.B, ptrs_ok, a.stream, &a.P, a.rowset != nullptr, a.who));
  MH_REQUIRE(a.workspace_bytes >= mh_t5_decode_workspace_bytes(a.c, a.B), "%s: workspace too small", a.who);
  return check_arch2_weights(a.c, a.w, a.who);
}

// The first row of the e4m3 shadow of the self-attention cache, and of its scales, at row b0 of a B-row batch (the b0 offsets of the
// bf16 caches); the same over the packed e4m3 copy of the cross K/V of kvB rows
static void self8_rows(const MhT5Config* c, int B, int b0, void* self8, DecBuffers* bf) {
  const long row = (long)b0 * c->n_heads * c->tgt_len;
  bf->self8 = (uint8_t*)self8 + row * 64;
  bf->self8_scales = reinterpret_cast<float*>((uint8_t*)self8 + self_kv8_layout(c, B).scales_offset) + row;
}
static void cross8_rows(const MhT5Config* c, int kvB, int b0, const void* kv8, StepCall* k) {
  k->kv8 = (const char*)kv8 + (long)b0 * c->n_heads * c->src_len * 64;
  k->kv8_scales = reinterpret_cast<const float*>((const char*)kv8 + cross_kv8_layout(c, kvB).scales_offset) + (long)b0 * c->n_heads;
}

// Chain ci of the call as a StepCall: rows [ci rows_per, + Bc) of every buffer, of the e4m3 copies and of the sampler's view
// (Bc <= 0: the batch has no such chain).  self8: the shadow of the whole batch, or NULL.
static void chain_call(const GenerateArgs& a, const DecodeLayout& ly, int ci, int rows_per, uint8_t* self8, StepCall* k) {
  const MhT5Config* c = a.c;
  const MhSampling* sp = a.sp;
  const DecBuffers& all = ly.bf;
  const int B = a.B, P = a.P, es = es_of(c->dtype), H = c->n_heads, inner = H * 64, d = c->d_model, V = c->vocab_out;
  const bool cfg = sp->cfg_scale > 1.0f;
  const int b0 = ci * rows_per;
  step_call_init(k, c, a.w);
  k->Bc = (b0 + rows_per <= B) ? rows_per : B - b0;
  k->Bfull = B; k->kvB = cfg ? B / 2 : B; k->P = P; k->with_sampler = 1;
  k->cross_kv = a.cross_kv ? (const char*)a.cross_kv + (long)b0 * H * c->src_len * 64 * es : nullptr;   // (NULL: a kv8 slot session without one)
  k->prompt_mask = a.prompt_mask ? a.prompt_mask + (long)b0 * P : nullptr;
  if (a.rowset) { k->has_rows = 1; k->rows.rows = a.rowset->rows; k->rows.eos_tables = a.rowset->eos_tables; k->rows.n_eos_sets = a.rowset->n_eos_sets; }
  DecBuffers& bf = k->bf;
  bf.chain = ci;
  bf.h = all.h + (long)b0 * d;
  bf.attn = (char*)all.attn + (long)b0 * inner * es;
  bf.ff = (char*)all.ff + (long)b0 * c->d_ff * es;
  bf.logits = all.logits + (long)b0 * V;
  bf.self_k = (char*)all.self_k + (long)b0 * inner * c->tgt_len * es;
  bf.self_v = (char*)all.self_v + (long)b0 * inner * c->tgt_len * es;
  if (self8) self8_rows(c, B, b0, self8, &bf);
  bf.finished = all.finished + b0;
  bf.finish_col = all.finish_col; bf.last_ts = all.last_ts;
  bf.st = (DecState*)((char*)all.st + (long)ci * align256(sizeof(DecState)));
  if (sp->cross_kv_fp8) cross8_rows(c, k->kvB, b0, sp->cross_kv_fp8, k);
  SampleP& smp = k->smp;
  smp.logits = bf.logits; smp.ldl = V; smp.V = V; smp.tokens = a.tokens; smp.max_length = sp->max_length;
  smp.forced = a.forced; smp.eos_table = a.eos_table; smp.finished = all.finished; smp.finish_col = all.finish_col;
  smp.last_ts_val = all.last_ts; smp.logits_dump = a.logits_dump; smp.dec_embed = a.w->dec_embed; smp.h = bf.h;
  smp.d = d; smp.st = bf.st; smp.B = B; smp.P = P; smp.b0 = b0;
  memcpy(&smp.sp, sp, sizeof(*sp));
  smp.proc = ly.proc; smp.hist_scores = ly.hist_scores; smp.pair = cfg ? B / 2 : 0; smp.chain_rows = k->Bc;
  if (c->arch == 2) {
    smp.dec_pos = a.w->dec_pos;
    smp.pos_off = c->dec_pos_from_mask ? ly.pos_off : nullptr;
    smp.prompt_mask = a.prompt_mask;
  }
}
// The batch cut into n_chains blocks of rows_per rows: calls[0 .. used), -> used (a late block may be empty: B = 5 over 4 chains)
static int chain_calls(const GenerateArgs& a, const DecodeLayout& ly, int n_chains, int rows_per, uint8_t* self8, StepCall* calls) {
  int used = 0;
  for (; used < n_chains; ++used) {
    chain_call(a, ly, used, rows_per, self8, &calls[used]);
    if (calls[used].Bc <= 0) break;
  }
  return used;
}

static int generate_impl(const GenerateArgs& a) {
  MH_TRY(check_generate_args(a));
  const MhT5Config* c = a.c;
  const MhSampling* sp = a.sp;
  const int B = a.B, P = a.P;
  hipStream_t s = (hipStream_t)a.stream;
  const bool cfg = sp->cfg_scale > 1.0f;
  const DecodeLayout ly = decode_layout(c, B, a.workspace);
  // a CFG pair spans both halves of the batch and the (batch-wide) conditional temperature reads row 0's history: one chain
  const int n_chains = (cfg || (sp->n_cond > 0 && !sp->cond_per_row)) ? 1 : pick_chains(B);
  const int rows_per = ceil_div(B, n_chains);
  int dev = 0;
  MH_TRY(stream_device(s, &dev));
  DeviceGuard device_guard(dev);
  DevicePool* dp = device_pool(dev);
  std::lock_guard<std::mutex> pool_guard(dp->mu);
  ChainPool& g_pool = dp->pool;
  MH_TRY(g_pool.init());
  Chain chains[kMaxChains];   // (their graphs are released / destroyed on every return path below)
  for (int i = 0; i < kMaxChains; ++i) chains[i].stream = g_pool.streams[i];

  // tokens[:, :P] = prompt; the remainder is produced by the sampler
  if (hipMemcpy2DAsync(a.tokens, (size_t)sp->max_length * 4, a.prompt, (size_t)P * 4, (size_t)P * 4, B,
                       hipMemcpyDeviceToDevice, s) != hipSuccess)
    return check_launch("prompt copy");
  // batched prompt prefill (positions 0..P-2); MH_DECODE_PREFILL=0 feeds the prompt token by token instead
  int start_pos = 0;
  if (P > 1 && option(OPT_DECODE_PREFILL) != 0) {
    PrefillBuf pb;
    prefill_layout(c, B, P - 1, (char*)a.workspace + ly.end, a.workspace_bytes - ly.end, &pb);
    MH_REQUIRE(ly.end + prefill_layout(c, B, P - 1, nullptr, 0, nullptr) <= a.workspace_bytes,
               "%s: workspace too small for the prompt prefill", a.who);
    MH_TRY(prefill_prompt(c, a.w, a.cross_kv, B, cfg ? B / 2 : B, a.prompt, a.prompt_mask, P, P - 1, ly.bf.self_k, ly.bf.self_v, pb, s));
    start_pos = P - 1;
  }
  // the shadow: the prompt positions the batched prefill wrote (they attended each other through the bf16 cache) are quantised in
  // one pass before the first token step; every token step appends its own row
  uint8_t* self8 = (uint8_t*)a.self_kv_fp8;
  if (self8 && start_pos > 0) MH_TRY(launch_self_kv_quant_rows(c, B, ly.bf, self8, B, start_pos, s));
  if (hipEventRecord(g_pool.fork, s) != hipSuccess) return check_launch("fork record");

  StepCall calls[kMaxChains];
  const int used = chain_calls(a, ly, n_chains, rows_per, self8, calls);
  int rc = MH_OK, which[kMaxChains];   // every chain of the call runs
  for (int ci = 0; ci < used && rc == MH_OK; ++ci) {
    which[ci] = ci;
    rc = start_chain(calls[ci], start_pos, g_pool.fork, a.who, &chains[ci]);
  }

  const int total_steps = sp->max_length - 1 - start_pos;   // positions start_pos .. max_length-2 are fed
  if (rc == MH_OK) rc = launch_chains(chains, which, used, total_steps, a.poll_every <= 0 ? 16 : a.poll_every, !a.forced, a.who);
  // join the chains back into the caller's stream
  for (int ci = 0; ci < used; ++ci) {
    (void)hipEventRecord(g_pool.join[ci], chains[ci].stream);
    (void)hipStreamWaitEvent(s, g_pool.join[ci], 0);
  }
  if (rc == MH_OK) {
    hipLaunchKernelGGL(dec_finalize_kernel, dim3(1), dim3(64), 0, s, ly.bf.finish_col, B, a.n_steps_out);
    rc = check_launch("dec_finalize_kernel");
  }
  (void)hipStreamSynchronize(s);   // the graph objects must outlive their launches
  if (rc == MH_OK && option(OPT_DECODE_FUSED_TAIL) != 0) {   // the chains are idle: their last word on the bounded hand-offs
    for (int ci = 0; ci < used && rc == MH_OK; ++ci) {
      int err = 0;
      if (hipMemcpy(&err, &chains[ci].st->tail_err, 4, hipMemcpyDeviceToHost) != hipSuccess) rc = check_launch("tail status");
      else rc = mh_t5_decode_tail_status(err);
    }
  }
  return rc;
}
}  // namespace mh

extern "C" int mh_t5_step_graph_cache_stats(long* hits, long* misses, int reset) {
  if (hits) *hits = mh::g_step_graph_hits.load();
  if (misses) *misses = mh::g_step_graph_misses.load();
  if (reset) { mh::g_step_graph_hits.store(0); mh::g_step_graph_misses.store(0); }
  return MH_OK;
}

extern "C" int mh_t5_generate(const MhT5Config* c, const MhT5Weights* w, const void* cross_kv, int B,
                              const int32_t* prompt, const uint8_t* prompt_mask, int P, const uint8_t* eos_table,
                              const MhSampling* sp, int32_t* tokens, int32_t* n_steps_out, float* logits_dump,
                              const int32_t* forced, void* workspace, int64_t workspace_bytes, int poll_every,
                              void* stream) {
  mh::OptionScope option_scope(c ? c->options : nullptr);
  return generate_impl({c, w, cross_kv, B, prompt, prompt_mask, P, eos_table, sp, tokens, n_steps_out, logits_dump, forced, workspace,
                        workspace_bytes, poll_every, stream, nullptr, nullptr, "mh_t5_generate"});
}

extern "C" int mh_t5_generate_skv8(const MhT5Config* c, const MhT5Weights* w, const void* cross_kv, int B,
                                   const int32_t* prompt, const uint8_t* prompt_mask, int P, const uint8_t* eos_table,
                                   const MhSampling* sp, int32_t* tokens, int32_t* n_steps_out, float* logits_dump,
                                   const int32_t* forced, void* workspace, int64_t workspace_bytes, int poll_every,
                                   void* stream, void* self_kv_fp8) {
  mh::OptionScope option_scope(c ? c->options : nullptr);
  MH_TRY(check_cfg(c, "mh_t5_generate_skv8"));
  MH_REQUIRE(self_kv_fp8, "mh_t5_generate_skv8: null argument (self_kv_fp8: mh_t5_self_kv_fp8_bytes(cfg, B) bytes owned by the caller)");
  MH_REQUIRE(c->dtype == MH_BF16, "mh_t5_generate_skv8: the e4m3 self-attention cache needs bf16 storage");
  return generate_impl({c, w, cross_kv, B, prompt, prompt_mask, P, eos_table, sp, tokens, n_steps_out, logits_dump, forced, workspace,
                        workspace_bytes, poll_every, stream, self_kv_fp8, nullptr, "mh_t5_generate_skv8"});
}

extern "C" int mh_t5_generate_rows(const MhT5Config* c, const MhT5Weights* w, const void* cross_kv, int B,
                                   const int32_t* prompt, const uint8_t* prompt_mask, int P, const uint8_t* eos_table,
                                   const MhSampling* sp, int32_t* tokens, int32_t* n_steps_out, float* logits_dump,
                                   const int32_t* forced, void* workspace, int64_t workspace_bytes, int poll_every,
                                   void* stream, void* self_kv_fp8, const MhRowSampling* rows, const uint8_t* eos_tables,
                                   int n_eos_sets) {
  mh::OptionScope option_scope(c ? c->options : nullptr);
  (void)eos_table;   // ignored: every row names its set of eos_tables
  MH_TRY(check_cfg(c, "mh_t5_generate_rows"));
  MH_TRY(mh::check_row_set(rows, eos_tables, n_eos_sets, "returned row", "mh_t5_generate_rows"));
  MH_REQUIRE(!self_kv_fp8 || c->dtype == MH_BF16, "mh_t5_generate_rows: the e4m3 self-attention cache needs bf16 storage");
  const mh::RowSetP rowset{rows, eos_tables, n_eos_sets};
  return generate_impl({c, w, cross_kv, B, prompt, prompt_mask, P, nullptr, sp, tokens, n_steps_out, logits_dump, forced, workspace,
                        workspace_bytes, poll_every, stream, self_kv_fp8, &rowset, "mh_t5_generate_rows"});
}

// ------------------------------------------------------------------------------------------------
// In-flight decode (mh_t5_slots_*; contract in include/mapperhip.h): S slots, every slot a row with a window of its own that enters
// (admit) and leaves (release) while its neighbours keep stepping.  The chains are those of mh_t5_generate_rows over S rows -- the
// same static row blocks, one DecState and one step graph each (the SLOT kernels: the key holds StepCall::slot_pos) -- on streams
// the session owns; admissions run on a stream of their own.
//
// Why no step can write a cache row, a token or a state word that an admission is filling, and no admission one that a step reads:
//   * an idle slot's position is negative: its self-attention workgroups return before they store, its sampler workgroup only
//     arrives; the GEMVs, the tail and the cross-attention write the slot's rows of h / attn / ff / logits, which nothing reads;
//   * release(slot) makes the position negative ON THE CHAIN'S STREAM, behind the slot's last step, and records freed[slot] there;
//   * admit(slot) waits for freed[slot] on the admission stream before its first write, and the slot's position -- the one word that
//     makes it live -- is the last thing its last kernel writes; then it records admitted[chain];
//   * run() makes the chain's stream wait for admitted[chain] before the first step enqueued after the admission.
// Events only: nothing on the device spins or waits for another launch.
namespace mh {
struct SlotSession {
  const MhT5Config* c = nullptr; const MhT5Weights* w = nullptr;
  int S = 0, n_chains = 0, rows_per = 0, dev = 0, max_length = 0, poll_every = 16;
  DecodeLayout ly{};
  int32_t* pos = nullptr; int32_t* plen = nullptr; uint8_t* mask = nullptr;   // [S], [S], [S][max_length]
  char* prefill_base = nullptr; int64_t prefill_bytes = 0;
  char* cross_kv = nullptr; int32_t* tokens = nullptr;   // cross_kv: the bf16 / fp32 slot copy, NULL where the steps stream cross8 alone
  uint8_t* cross8 = nullptr; uint8_t* self8 = nullptr;   // mh_t5_slots_open_kv8: the caller's S-row e4m3 copies, or NULL
  Chain chains[kMaxChains];
  StepCall calls[kMaxChains];
  hipStream_t admit_stream = nullptr;
  hipEvent_t admitted[kMaxChains] = {}, freed[64] = {}, caller_ev = nullptr;
  bool pending[kMaxChains] = {};    // an admission into the chain since its last step was enqueued
  bool live[64] = {};               // admitted and not released
  int32_t host_pos[64] = {}, host_col[64] = {}; uint8_t host_fin[64] = {};
  ~SlotSession() {
    // joins the chains and the admissions (a graph object must outlive its launches; the Chain members release theirs after this body)
    if (admit_stream) { (void)hipStreamSynchronize(admit_stream); (void)hipStreamDestroy(admit_stream); }
    for (int i = 0; i < kMaxChains; ++i) {
      if (chains[i].stream) { (void)hipStreamSynchronize(chains[i].stream); (void)hipStreamDestroy(chains[i].stream); }
      if (admitted[i]) (void)hipEventDestroy(admitted[i]);
    }
    for (int i = 0; i < 64; ++i) if (freed[i]) (void)hipEventDestroy(freed[i]);
    if (caller_ev) (void)hipEventDestroy(caller_ev);
  }
  int chain_of(int slot) const { return slot / rows_per; }
};
// the slot buffers behind the decode layout of S rows, then the prompt prefill of ONE row (an admission prefills one window)
static int64_t slots_layout(const MhT5Config* c, int S, void* base, SlotSession* ss) {
  const DecodeLayout ly = decode_layout(c, S, base);
  Arena ar(base ? (char*)base + ly.end : nullptr, INT64_MAX);
  int32_t* pos = (int32_t*)ar.take((int64_t)S * 4);
  int32_t* plen = (int32_t*)ar.take((int64_t)S * 4);
  uint8_t* mask = (uint8_t*)ar.take((int64_t)S * c->tgt_len);
  const int64_t pre = prefill_layout(c, 1, c->tgt_len - 1, nullptr, 0, nullptr);
  if (ss) {
    ss->ly = ly; ss->pos = pos; ss->plen = plen; ss->mask = mask;
    ss->prefill_base = (char*)base + ly.end + ar.off; ss->prefill_bytes = pre;
  }
  return ly.end + ar.off + pre;
}
}  // namespace mh

extern "C" int64_t mh_t5_slots_workspace_bytes(const MhT5Config* c, int S) {
  mh::OptionScope option_scope(c ? c->options : nullptr);
  if (!c || S < 1 || S > 64) return -1;
  return mh::slots_layout(c, S, nullptr, nullptr);
}

namespace mh {
// mh_t5_slots_open (kv8 = false: the e4m3 caches are refused) and mh_t5_slots_open_kv8 (kv8 = true: sp->cross_kv_fp8 / self_kv_fp8 are
// the session's S-row copies, filled row by row by the admissions and the token steps)
static int slots_open_impl(const MhT5Config* c, const MhT5Weights* w, int S, const MhSampling* sp, const MhRowSampling* rows,
                           const uint8_t* eos_tables, int n_eos_sets, void* cross_kv_slots, int32_t* tokens, float* logits_dump,
                           const int32_t* forced, void* self_kv_fp8, void* workspace, int64_t workspace_bytes, int poll_every,
                           void* stream, void** handle, bool kv8, const char* who) {
  OptionScope option_scope(c ? c->options : nullptr);
  MH_TRY(check_cfg(c, who));
  MH_REQUIRE(handle, "%s: null argument (handle)", who);
  *handle = nullptr;
  MH_REQUIRE(S >= 1 && S <= 64, "%s: %d slots not in [1, 64]", who, S);
  MH_TRY(check_row_set(rows, eos_tables, n_eos_sets, "slot", who));
  MH_REQUIRE(sp, "%s: null argument (sp)", who);
  MH_REQUIRE(!(sp->cfg_scale > 1.0f), "%s: classifier-free guidance has no slot form (a pair spans two rows of one position)", who);
  MH_REQUIRE(!forced, "%s: teacher forcing (forced ids) has no slot form", who);
  if (!kv8) {
    MH_REQUIRE(!sp->cross_kv_fp8, "%s: the e4m3 copy of the cross K/V (cross_kv_fp8) has no slot form", who);
    MH_REQUIRE(!self_kv_fp8, "%s: the e4m3 shadow of the self-attention cache has no slot form", who);
  } else {
    MH_REQUIRE(!sp->cross_kv_fp8 || c->dtype == MH_BF16, "%s: cross_kv_fp8 needs bf16 storage", who);
    MH_REQUIRE(!self_kv_fp8 || c->dtype == MH_BF16, "%s: the e4m3 self-attention cache needs bf16 storage", who);
    MH_REQUIRE(cross_kv_slots || sp->cross_kv_fp8,
               "%s: null argument (cross_kv_slots may be NULL only where sp->cross_kv_fp8 is the slots' e4m3 copy)", who);
  }
  MH_REQUIRE(sp->n_cond == 0 || sp->cond_per_row, "%s: conditional temperature rules need cond_per_row = 1 (every slot is a window of its own)", who);
  // whatever mh_t5_generate_rows refuses of a configuration and its settings (the prompt length is each admission's)
  MH_TRY(check_decode_call(c, w, sp, S, (cross_kv_slots || (kv8 && sp->cross_kv_fp8)) && tokens && workspace, stream, nullptr, true, who));
  MH_REQUIRE(workspace_bytes >= slots_layout(c, S, nullptr, nullptr), "%s: workspace too small (mh_t5_slots_workspace_bytes)", who);
  MH_TRY(check_arch2_weights(c, w, who));
  hipStream_t s = (hipStream_t)stream;
  int dev = 0;
  MH_TRY(stream_device(s, &dev));
  DeviceGuard device_guard(dev);
  std::unique_ptr<SlotSession> ss(new SlotSession());
  ss->c = c; ss->w = w; ss->S = S; ss->dev = dev; ss->max_length = sp->max_length; ss->poll_every = poll_every <= 0 ? 16 : poll_every;
  ss->cross_kv = (char*)cross_kv_slots; ss->tokens = tokens;
  ss->cross8 = (uint8_t*)sp->cross_kv_fp8; ss->self8 = (uint8_t*)self_kv_fp8;   // (both NULL behind mh_t5_slots_open)
  slots_layout(c, S, workspace, ss.get());
  ss->n_chains = pick_chains(S);
  ss->rows_per = ceil_div(S, ss->n_chains);
  // every slot idle: position -1, flag set (the recount of n_running counts clear flags); the chains' control blocks zero
  if (hipMemsetAsync(ss->pos, 0xff, (size_t)S * 4, s) != hipSuccess || hipMemsetAsync(ss->plen, 0, (size_t)S * 4, s) != hipSuccess ||
      hipMemsetAsync(ss->ly.bf.finished, 1, (size_t)S, s) != hipSuccess ||
      hipMemsetAsync(ss->mask, 1, (size_t)S * sp->max_length, s) != hipSuccess ||
      hipMemsetAsync(ss->ly.bf.st, 0, (size_t)align256(sizeof(DecState)) * kMaxChains, s) != hipSuccess)
    return check_launch("slot state memset");
  if (hipStreamCreateWithFlags(&ss->admit_stream, hipStreamNonBlocking) != hipSuccess) return check_launch("slot stream create");
  for (int b = 0; b < S; ++b) {
    if (hipEventCreateWithFlags(&ss->freed[b], hipEventDisableTiming) != hipSuccess) return check_launch("slot event create");
    if (hipEventRecord(ss->freed[b], s) != hipSuccess) return check_launch("slot event record");
  }
  const RowSetP rowset{rows, eos_tables, n_eos_sets};
  GenerateArgs a{c, w, cross_kv_slots, S, nullptr, ss->mask, sp->max_length, nullptr, sp, tokens, nullptr, logits_dump, nullptr, workspace,
                 workspace_bytes, poll_every, stream, self_kv_fp8, &rowset, who};
  // prompt_mask: the slot mask rows, stride max_length (call.P); the chains' rows of both e4m3 copies (both pointers are in the key
  // of the step graph: a kv8 session and a plain one never share a graph)
  ss->n_chains = chain_calls(a, ss->ly, ss->n_chains, ss->rows_per, ss->self8, ss->calls);
  for (int ci = 0; ci < ss->n_chains; ++ci) {
    StepCall& call = ss->calls[ci];
    call.slot_pos = ss->pos; call.slot_plen = ss->plen;
    Chain& ch = ss->chains[ci];
    if (hipStreamCreateWithFlags(&ch.stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&ss->admitted[ci], hipEventDisableTiming) != hipSuccess)
      return check_launch("slot stream create");
    ch.st = call.bf.st;
    if (hipStreamWaitEvent(ch.stream, ss->freed[0], 0) != hipSuccess) return check_launch("slot stream wait");   // behind the memsets
    MH_TRY(chain_step_graph(call, who, &ch));
  }
  if (hipStreamSynchronize(s) != hipSuccess) return check_launch("slot open");
  *handle = ss.release();
  return MH_OK;
}
}  // namespace mh

extern "C" int mh_t5_slots_open(const MhT5Config* c, const MhT5Weights* w, int S, const MhSampling* sp, const MhRowSampling* rows,
                                const uint8_t* eos_tables, int n_eos_sets, void* cross_kv_slots, int32_t* tokens, float* logits_dump,
                                const int32_t* forced, void* self_kv_fp8, void* workspace, int64_t workspace_bytes, int poll_every,
                                void* stream, void** handle) {
  return mh::slots_open_impl(c, w, S, sp, rows, eos_tables, n_eos_sets, cross_kv_slots, tokens, logits_dump, forced, self_kv_fp8, workspace,
                             workspace_bytes, poll_every, stream, handle, false, "mh_t5_slots_open");
}

extern "C" int mh_t5_slots_open_kv8(const MhT5Config* c, const MhT5Weights* w, int S, const MhSampling* sp, const MhRowSampling* rows,
                                    const uint8_t* eos_tables, int n_eos_sets, void* cross_kv_slots, int32_t* tokens, float* logits_dump,
                                    const int32_t* forced, void* self_kv_fp8, void* workspace, int64_t workspace_bytes, int poll_every,
                                    void* stream, void** handle) {
  // with neither copy this is mh_t5_slots_open (which then refuses a NULL cross_kv_slots as ever)
  const bool kv8 = (sp && sp->cross_kv_fp8) || self_kv_fp8;
  return mh::slots_open_impl(c, w, S, sp, rows, eos_tables, n_eos_sets, cross_kv_slots, tokens, logits_dump, forced, self_kv_fp8, workspace,
                             workspace_bytes, poll_every, stream, handle, kv8, "mh_t5_slots_open_kv8");
}

extern "C" int mh_t5_slots_admit(void* handle, int slot, const void* cross_kv_row, const int32_t* prompt, const uint8_t* prompt_mask, int P,
                                 void* stream) {
  using namespace mh;
  SlotSession* ss = (SlotSession*)handle;
  const char* who = "mh_t5_slots_admit";
  MH_REQUIRE(ss, "%s: null handle", who);
  OptionScope option_scope(ss->c->options);
  MH_REQUIRE(cross_kv_row && prompt, "%s: null argument", who);
  MH_REQUIRE(slot >= 0 && slot < ss->S, "%s: slot %d not in [0, %d)", who, slot, ss->S);
  MH_REQUIRE(!ss->live[slot], "%s: slot %d is live (release it first)", who, slot);
  MH_REQUIRE(P >= 1 && P < ss->max_length, "%s: prompt length %d must be in [1, max_length)", who, P);
  DeviceGuard device_guard(ss->dev);
  const MhT5Config* c = ss->c;
  const int ci = ss->chain_of(slot), es = es_of(c->dtype), H = c->n_heads, inner = H * 64;
  hipStream_t as = ss->admit_stream;
  if (hipStreamWaitEvent(as, ss->freed[slot], 0) != hipSuccess) return check_launch("admit wait");
  if (stream) {   // the caller's stream wrote cross_kv_row / prompt / prompt_mask: the admission reads them behind that work
    if (!ss->caller_ev && hipEventCreateWithFlags(&ss->caller_ev, hipEventDisableTiming) != hipSuccess) return check_launch("admit event create");
    if (hipEventRecord(ss->caller_ev, (hipStream_t)stream) != hipSuccess || hipStreamWaitEvent(as, ss->caller_ev, 0) != hipSuccess)
      return check_launch("admit caller wait");
  }
  // the window's compact cross K/V [n_dec][2][1][H][L][64] -> row `slot` of [n_dec][2][S][H][L][64]
  const size_t row_bytes = (size_t)H * c->src_len * 64 * es;
  if (ss->cross_kv && hipMemcpy2DAsync(ss->cross_kv + (size_t)slot * row_bytes, (size_t)ss->S * row_bytes, cross_kv_row, row_bytes, row_bytes,
                                       (size_t)c->n_dec_layers * 2, hipMemcpyDeviceToDevice, as) != hipSuccess)
    return check_launch("admit cross K/V copy");
  if (ss->cross8) {   // ... and, quantised, -> row `slot` of the S-row e4m3 copy (bytes and scales; no other row is touched)
    hipLaunchKernelGGL(kv_quant_fp8_row_kernel, dim3(c->n_dec_layers * 2 * H), dim3(256), 0, as, (const bf16_t*)cross_kv_row, ss->cross8,
                       reinterpret_cast<float*>(ss->cross8 + cross_kv8_layout(c, ss->S).scales_offset), c->src_len, H, ss->S, slot);
    MH_TRY(check_launch("kv_quant_fp8_row_kernel"));
  }
  int32_t* trow = ss->tokens + (long)slot * ss->max_length;
  uint8_t* mrow = ss->mask + (long)slot * ss->max_length;
  if (hipMemcpyAsync(trow, prompt, (size_t)P * 4, hipMemcpyDeviceToDevice, as) != hipSuccess) return check_launch("admit prompt copy");
  if (hipMemsetAsync(mrow, 1, (size_t)ss->max_length, as) != hipSuccess) return check_launch("admit mask set");
  if (prompt_mask && hipMemcpyAsync(mrow, prompt_mask, (size_t)P, hipMemcpyDeviceToDevice, as) != hipSuccess) return check_launch("admit mask copy");
  int start_pos = 0;
  if (P > 1 && option(OPT_DECODE_PREFILL) != 0) {   // positions 0 .. P-2 into the slot's cache rows: the B = 1 prefill of a uniform call
    PrefillBuf pb;
    prefill_layout(c, 1, P - 1, ss->prefill_base, ss->prefill_bytes, &pb);
    const long cache_row = (long)slot * inner * c->tgt_len * es;
    MH_TRY(prefill_prompt(c, ss->w, cross_kv_row, 1, 1, prompt, prompt_mask, P, P - 1, (char*)ss->ly.bf.self_k + cache_row,
                          (char*)ss->ly.bf.self_v + cache_row, pb, as, ss->S));
    start_pos = P - 1;
    if (ss->self8) {   // the prefilled positions 0 .. P-2 of the slot's cache rows -> the same places of the S-row shadow, every layer,
                       // k and v (the pass a uniform call makes after its prefill); nothing else of the shadow is written
      const long row0 = (long)slot * H * c->tgt_len, plane_rows = (long)ss->S * H * c->tgt_len;
      hipLaunchKernelGGL(self_kv_quant_rows_kernel, dim3((unsigned)(((long)H * start_pos + 3) / 4), 2 * c->n_dec_layers), dim3(256), 0, as,
                         (const bf16_t*)ss->ly.bf.self_k + row0 * 64, (const bf16_t*)ss->ly.bf.self_v + row0 * 64, ss->self8 + row0 * 64,
                         reinterpret_cast<float*>(ss->self8 + self_kv8_layout(c, ss->S).scales_offset) + row0, (long)H, (long)start_pos,
                         (long)c->tgt_len, plane_rows);
      MH_TRY(check_launch("self_kv_quant_rows_kernel"));
    }
  }
  const SampleP& smp = ss->calls[ci].smp;
  if (c->dtype == MH_BF16) hipLaunchKernelGGL(dec_slot_init_kernel<bf16_t>, dim3(1), dim3(256), 0, as, smp, slot, P, start_pos, ss->pos, ss->plen);
  else hipLaunchKernelGGL(dec_slot_init_kernel<float>, dim3(1), dim3(256), 0, as, smp, slot, P, start_pos, ss->pos, ss->plen);
  MH_TRY(check_launch("dec_slot_init_kernel"));
  if (hipEventRecord(ss->admitted[ci], as) != hipSuccess) return check_launch("admit record");
  ss->pending[ci] = true;
  ss->live[slot] = true;
  return MH_OK;
}

extern "C" int mh_t5_slots_run(void* handle, int n_steps, uint8_t* finished_out, int32_t* length_out, int32_t* steps_out) {
  using namespace mh;
  SlotSession* ss = (SlotSession*)handle;
  const char* who = "mh_t5_slots_run";
  MH_REQUIRE(ss, "%s: null handle", who);
  OptionScope option_scope(ss->c->options);
  MH_REQUIRE(n_steps >= 0 && finished_out && length_out, "%s: bad argument", who);
  DeviceGuard device_guard(ss->dev);
  int steps[kMaxChains] = {}, which[kMaxChains], n_run = 0;   // which: the chains with a live slot run
  bool runs[kMaxChains] = {};
  for (int b = 0; b < ss->S; ++b) if (ss->live[b]) runs[ss->chain_of(b)] = true;
  for (int ci = 0; ci < ss->n_chains; ++ci) {
    if (!runs[ci]) continue;
    which[n_run++] = ci;
    // The fused tail's hand-off counters only ever grow inside a call, and a launch takes its base as a multiple of its grid: a
    // session has no dec_init_kernel between its steps, so they start every run at zero (the chain is idle here: the last run
    // ended with its poll) and cannot wrap however long the session lives.  tail_err stays: a timed-out session stays reported.
    if (n_steps > 0 && hipMemsetAsync(ss->chains[ci].st->tail_cnt, 0, sizeof(ss->chains[ci].st->tail_cnt), ss->chains[ci].stream) != hipSuccess)
      return check_launch("tail counter reset");
    if (ss->pending[ci]) {   // the step that first sees the admitted slots live waits for their admissions
      if (hipStreamWaitEvent(ss->chains[ci].stream, ss->admitted[ci], 0) != hipSuccess) return check_launch("admission wait");
      ss->pending[ci] = false;
    }
  }
  int rc = n_steps > 0 ? launch_chains(ss->chains, which, n_run, n_steps, ss->poll_every, true, who, steps) : MH_OK, total = 0;
  for (int ci = 0; ci < ss->n_chains; ++ci) total += steps[ci];
  // one poll per chain: its rows' flags, finish columns and positions, and the bounded hand-offs' last word
  for (int ci = 0; ci < ss->n_chains; ++ci) {
    const int b0 = ci * ss->rows_per, n = ss->calls[ci].Bc;
    hipStream_t cs = ss->chains[ci].stream;
    int word[2] = {0, 0};
    if (hipMemcpyAsync(ss->host_fin + b0, ss->ly.bf.finished + b0, (size_t)n, hipMemcpyDeviceToHost, cs) != hipSuccess ||
        hipMemcpyAsync(ss->host_col + b0, ss->ly.bf.finish_col + b0, (size_t)n * 4, hipMemcpyDeviceToHost, cs) != hipSuccess ||
        hipMemcpyAsync(ss->host_pos + b0, ss->pos + b0, (size_t)n * 4, hipMemcpyDeviceToHost, cs) != hipSuccess ||
        hipMemcpyAsync(word, &ss->chains[ci].st->n_running, 8, hipMemcpyDeviceToHost, cs) != hipSuccess ||
        hipStreamSynchronize(cs) != hipSuccess)
      return check_launch("slot poll");
    if (rc == MH_OK && word[1] != 0) rc = mh_t5_decode_tail_status(word[1]);
  }
  for (int b = 0; b < ss->S; ++b) {
    const bool fin = ss->live[b] && ss->host_fin[b] != 0;
    finished_out[b] = fin ? 1 : 0;
    length_out[b] = !ss->live[b] ? 0 : (fin ? ss->host_col[b] + 1 : ss->host_pos[b] + 1);
  }
  if (steps_out) *steps_out = total;
  return rc;
}

extern "C" int mh_t5_slots_release(void* handle, int slot) {
  using namespace mh;
  SlotSession* ss = (SlotSession*)handle;
  const char* who = "mh_t5_slots_release";
  MH_REQUIRE(ss, "%s: null handle", who);
  MH_REQUIRE(slot >= 0 && slot < ss->S, "%s: slot %d not in [0, %d)", who, slot, ss->S);
  MH_REQUIRE(ss->live[slot], "%s: slot %d is idle", who, slot);
  DeviceGuard device_guard(ss->dev);
  const int ci = ss->chain_of(slot);
  hipStream_t cs = ss->chains[ci].stream;
  if (ss->pending[ci]) {   // released before a step saw it: still behind its own admission
    if (hipStreamWaitEvent(cs, ss->admitted[ci], 0) != hipSuccess) return check_launch("admission wait");
    ss->pending[ci] = false;
  }
  // on the chain's stream, behind the slot's last step: idle again (negative position, flag set), then the event an admission waits for
  if (hipMemsetAsync(ss->pos + slot, 0xff, 4, cs) != hipSuccess || hipMemsetAsync(ss->ly.bf.finished + slot, 1, 1, cs) != hipSuccess ||
      hipEventRecord(ss->freed[slot], cs) != hipSuccess)
    return check_launch("slot release");
  ss->live[slot] = false;
  return MH_OK;
}

extern "C" int mh_t5_slots_close(void* handle) {
  using namespace mh;
  SlotSession* ss = (SlotSession*)handle;
  if (!ss) return MH_OK;
  DeviceGuard device_guard(ss->dev);
  delete ss;   // joins the chains, then releases the graph references (the cross-call cache keeps the graphs it owns)
  return check_launch("slot close");
}

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

extern "C" int mh_t5_decode_chains(int B) { return B > 0 ? mh::pick_chains(B) : 0; }
extern "C" int mh_t5_decode_chains_cfg(const MhT5Config* c, int B) {   // ... under the engine's option set
  mh::OptionScope option_scope(c ? c->options : nullptr);
  return B > 0 ? mh::pick_chains(B) : 0;
}

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


// ------------------------------------------------------------------------------------------------
// Step-wise decode for host-driven search (beam search: HF `GenerationMixin._beam_search` drives the model one position at a
// time and reorders its cache, osuT5/osuT5/inference/cache_utils.py:16-20).  The workspace is the one of mh_t5_generate
// (mh_t5_decode_workspace_bytes) and holds the self-attention K/V caches between calls.
// mh_t5_step (fp8 = false) and mh_t5_step_fp8
static int step_impl(const MhT5Config* c, const MhT5Weights* w, const void* cross_kv, bool fp8, const void* cross_kv_fp8, int B,
                     int kv_group, const int32_t* ids, int pos, const uint8_t* prompt_mask, int P, float* logits, void* workspace,
                     int64_t workspace_bytes, void* stream, const char* who,   // who: the entry the caller used (error messages)
                     bool indexed = false, const uint8_t* origin = nullptr,
                     bool shadow = false, void* self_kv_fp8 = nullptr) {   // shadow: mh_t5_step_indexed_skv8 (the caller's e4m3 self cache)
  MH_TRY(check_cfg(c, who));
  MH_TRY(check_decode_shape(c, who));
  MH_REQUIRE(w && cross_kv && (cross_kv_fp8 || !fp8) && ids && logits && workspace && (origin || !indexed) && (self_kv_fp8 || !shadow),
             "%s: null argument", who);
  MH_REQUIRE(!shadow || c->dtype == MH_BF16, "%s: the e4m3 self-attention cache needs bf16 storage", who);
  MH_REQUIRE(!indexed || c->tgt_len <= dec::kSelfIdxMaxTgt, "%s: the index table covers tgt_len <= %d (got %d)", who,
             dec::kSelfIdxMaxTgt, c->tgt_len);
  MH_REQUIRE(!fp8 || c->dtype == MH_BF16, "%s: the fp8 cross K/V copy needs bf16 storage", who);
  MH_REQUIRE(B > 0 && B <= 64, "%s: batch %d not in [1, 64]", who, B);
  MH_REQUIRE(kv_group >= 1 && B % kv_group == 0, "%s: %d rows are not whole groups of %d", who, B, kv_group);
  MH_REQUIRE(pos >= 0 && pos < c->tgt_len, "%s: position %d outside the cache (tgt_len %d)", who, pos, c->tgt_len);
  MH_REQUIRE(workspace_bytes >= mh_t5_decode_workspace_bytes(c, B), "%s: workspace too small", who);
  MH_TRY(check_arch2_weights(c, w, who));
  hipStream_t s = (hipStream_t)stream;
  StepCall k;
  step_call_init(&k, c, w);
  k.cross_kv = cross_kv; k.Bc = k.Bfull = B; k.kvB = B / kv_group; k.prompt_mask = prompt_mask; k.P = P; k.kv_group = kv_group;
  k.bf = decode_layout(c, B, workspace).bf;
  k.bf.logits = logits;   // (the host selects: the raw logits go straight to the caller)
  k.origin = origin;
  if (shadow) self8_rows(c, B, 0, self_kv_fp8, &k.bf);   // the whole batch is one chain
  if (fp8) cross8_rows(c, k.kvB, 0, cross_kv_fp8, &k);
  const float* dpos = c->arch == 2 ? w->dec_pos : nullptr;
  const uint8_t* pmask = (c->arch == 2 && c->dec_pos_from_mask) ? prompt_mask : nullptr;
  return dispatch_dtype(c->dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(step_embed_kernel<T>, dim3(B), dim3(256), 0, s, ids, (const T*)w->dec_embed, c->d_model, k.bf.h, k.bf.st, pos, dpos, pmask, P);
    MH_TRY(check_launch("step_embed_kernel"));
    return enqueue_step<T>(k, s);
  });
}

extern "C" int mh_t5_step(const MhT5Config* c, const MhT5Weights* w, const void* cross_kv, int B, int kv_group, const int32_t* ids,
                          int pos, const uint8_t* prompt_mask, int P, float* logits, void* workspace, int64_t workspace_bytes,
                          void* stream) {
  mh::OptionScope option_scope(c ? c->options : nullptr);
  return step_impl(c, w, cross_kv, false, nullptr, B, kv_group, ids, pos, prompt_mask, P, logits, workspace, workspace_bytes, stream, "mh_t5_step");
}

// mh_t5_step with the packed e4m3 copy of cross_kv (mh_t5_quantize_cross_kv over its B / kv_group rows) as one more argument: every
// cross-attention of the step streams the copy, its scales indexed by the K/V row a decode row reads.  bf16 storage only.
extern "C" int mh_t5_step_fp8(const MhT5Config* c, const MhT5Weights* w, const void* cross_kv, const void* cross_kv_fp8, int B,
                              int kv_group, const int32_t* ids, int pos, const uint8_t* prompt_mask, int P, float* logits,
                              void* workspace, int64_t workspace_bytes, void* stream) {
  mh::OptionScope option_scope(c ? c->options : nullptr);
  return step_impl(c, w, cross_kv, true, cross_kv_fp8, B, kv_group, ids, pos, prompt_mask, P, logits, workspace, workspace_bytes, stream,
                   "mh_t5_step_fp8");
}

// self-attention cache rows of every layer: row b <- row src[b] for positions 0 .. n_pos-1 (`cache.reorder_cache(beam_idx)`).
// scratch: 2 * n_dec * B * inner * n_pos elements of the storage type (mh_t5_reorder_cache_scratch_bytes).
extern "C" int64_t mh_t5_reorder_cache_scratch_bytes(const MhT5Config* c, int B, int n_pos) {
  mh::OptionScope option_scope(c ? c->options : nullptr);
  if (!c || B <= 0 || n_pos <= 0) return -1;
  return align256(2LL * c->n_dec_layers * B * c->n_heads * 64 * n_pos * es_of(c->dtype));
}
extern "C" int mh_t5_reorder_cache(const MhT5Config* c, int B, const int32_t* src, int n_pos, void* workspace, int64_t workspace_bytes,
                                   void* scratch, int64_t scratch_bytes, void* stream) {
  mh::OptionScope option_scope(c ? c->options : nullptr);
  MH_TRY(check_cfg(c, "mh_t5_reorder_cache"));
  MH_REQUIRE(src && workspace && scratch && B > 0 && B <= 64 && n_pos > 0 && n_pos <= c->tgt_len, "mh_t5_reorder_cache: bad argument");
  MH_REQUIRE(workspace_bytes >= mh_t5_decode_workspace_bytes(c, B) && scratch_bytes >= mh_t5_reorder_cache_scratch_bytes(c, B, n_pos),
             "mh_t5_reorder_cache: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int H = c->n_heads;
  const DecBuffers bf = decode_layout(c, B, workspace).bf;   // (the self-attention caches)
  void* self_k = bf.self_k;
  void* self_v = bf.self_v;
  const long layer_stride = (long)B * H * c->tgt_len * 64;
  const dim3 grid(B * H, c->n_dec_layers, 2);
  return dispatch_dtype(c->dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(cache_gather_kernel<T>, grid, dim3(256), 0, s, (const T*)self_k, (const T*)self_v, (T*)scratch, src, B, H, c->tgt_len, n_pos, layer_stride);
    hipLaunchKernelGGL(cache_scatter_kernel<T>, grid, dim3(256), 0, s, (T*)self_k, (T*)self_v, (const T*)scratch, B, H, c->tgt_len, n_pos, layer_stride);
    return check_launch("cache reorder");
  });
}

// ---- beam search by index: the self-attention cache stays where it was written ---------------------------------------------
// The caches of a (chunk, beam) batch are never copied.  A table origin uint8 [B][tgt_len] says, per decode row b and position j, which
// cache row holds that key / value; the step reads through it (dec_self_attn_qkv_kernel, IDX) and a reorder permutes table rows.  A
// step writes position `pos` of cache row b and nothing else, so every (cache row, position) is written once and an entry never goes
// stale.
namespace mh {
namespace {
__global__ __launch_bounds__(256) void beam_index_init_kernel(uint8_t* origin, int tgt, int kv_group, int n_prefilled) {
  const int b = blockIdx.x;
  for (int j = threadIdx.x; j < tgt; j += 256) origin[(long)b * tgt + j] = (uint8_t)(j < n_prefilled ? b / kv_group : b);
}
// out[b][j] = in[src[b]][j] for j < n_pos, b beyond (src clamped to the batch: a table entry is always a cache row)
__global__ __launch_bounds__(256) void beam_index_reorder_kernel(const uint8_t* in, uint8_t* out, const int32_t* src, int B, int tgt,
                                                                int n_pos) {
  const int b = blockIdx.x;
  int sb = src[b];
  sb = sb < 0 ? 0 : (sb >= B ? B - 1 : sb);
  for (int j = threadIdx.x; j < tgt; j += 256) out[(long)b * tgt + j] = j < n_pos ? in[(long)sb * tgt + j] : (uint8_t)b;
}
}  // namespace
}  // namespace mh

extern "C" int64_t mh_t5_beam_index_bytes(const MhT5Config* c, int B) {
  if (!c || B <= 0 || B > 64 || c->tgt_len <= 0) return -1;
  return (int64_t)B * c->tgt_len;
}

extern "C" int mh_t5_beam_index_init(const MhT5Config* c, int B, int kv_group, int n_prefilled, void* origin, void* stream) {
  mh::OptionScope option_scope(c ? c->options : nullptr);
  MH_TRY(check_cfg(c, "mh_t5_beam_index_init"));
  MH_REQUIRE(origin, "mh_t5_beam_index_init: null argument");
  MH_REQUIRE(B > 0 && B <= 64, "mh_t5_beam_index_init: batch %d not in [1, 64]", B);
  MH_REQUIRE(kv_group >= 1 && B % kv_group == 0, "mh_t5_beam_index_init: %d rows are not whole groups of %d", B, kv_group);
  MH_REQUIRE(n_prefilled >= 0 && n_prefilled < c->tgt_len, "mh_t5_beam_index_init: %d prefilled positions outside the cache (tgt_len %d)",
             n_prefilled, c->tgt_len);
  hipLaunchKernelGGL(mh::beam_index_init_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, (uint8_t*)origin, c->tgt_len, kv_group,
                     n_prefilled);
  return check_launch("beam_index_init_kernel");
}

extern "C" int mh_t5_reorder_index(const MhT5Config* c, int B, const int32_t* src, int n_pos, const void* origin_in, void* origin_out,
                                   void* stream) {
  mh::OptionScope option_scope(c ? c->options : nullptr);
  MH_TRY(check_cfg(c, "mh_t5_reorder_index"));
  MH_REQUIRE(src && origin_in && origin_out, "mh_t5_reorder_index: null argument");
  MH_REQUIRE(origin_in != origin_out, "mh_t5_reorder_index: origin_in and origin_out must be two tables (the caller ping-pongs)");
  MH_REQUIRE(B > 0 && B <= 64, "mh_t5_reorder_index: batch %d not in [1, 64]", B);
  MH_REQUIRE(n_pos > 0 && n_pos <= c->tgt_len, "mh_t5_reorder_index: %d positions outside the cache (tgt_len %d)", n_pos, c->tgt_len);
  hipLaunchKernelGGL(mh::beam_index_reorder_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)origin_in,
                     (uint8_t*)origin_out, src, B, c->tgt_len, n_pos);
  return check_launch("beam_index_reorder_kernel");
}

// mh_t5_step / mh_t5_step_fp8 (cross_kv_fp8 != NULL) reading the cached keys / values through `origin`
extern "C" int mh_t5_step_indexed(const MhT5Config* c, const MhT5Weights* w, const void* cross_kv, const void* cross_kv_fp8, int B,
                                  int kv_group, const int32_t* ids, int pos, const uint8_t* prompt_mask, int P, float* logits,
                                  void* workspace, int64_t workspace_bytes, const void* origin, void* stream) {
  mh::OptionScope option_scope(c ? c->options : nullptr);
  return step_impl(c, w, cross_kv, cross_kv_fp8 != nullptr, cross_kv_fp8, B, kv_group, ids, pos, prompt_mask, P, logits, workspace,
                   workspace_bytes, stream, "mh_t5_step_indexed", true, (const uint8_t*)origin);
}

// mh_t5_step_indexed over the caller's e4m3 shadow of the self-attention cache (mh_t5_self_kv_fp8_bytes(cfg, B) bytes): cached rows
// j < pos are the e4m3 rows of shadow row origin[b][j] with that row's scales; the new row is appended to shadow row b
extern "C" int mh_t5_step_indexed_skv8(const MhT5Config* c, const MhT5Weights* w, const void* cross_kv, const void* cross_kv_fp8, int B,
                                       int kv_group, const int32_t* ids, int pos, const uint8_t* prompt_mask, int P, float* logits,
                                       void* workspace, int64_t workspace_bytes, const void* origin, void* self_kv_fp8, void* stream) {
  mh::OptionScope option_scope(c ? c->options : nullptr);
  return step_impl(c, w, cross_kv, cross_kv_fp8 != nullptr, cross_kv_fp8, B, kv_group, ids, pos, prompt_mask, P, logits, workspace,
                   workspace_bytes, stream, "mh_t5_step_indexed_skv8", true, (const uint8_t*)origin, true, self_kv_fp8);
}

// positions 0 .. n_pos-1 of cache rows 0 .. n_rows-1 (what mh_t5_step_prefill wrote, n_rows = Bp) of the bf16 self-attention caches of
// a B-row step workspace -> the B-row shadow, every layer, k and v; nothing else of the shadow is written
extern "C" int mh_t5_self_kv_fp8_fill(const MhT5Config* c, int B, int n_rows, int n_pos, void* workspace, int64_t workspace_bytes,
                                      void* self_kv_fp8, void* stream) {
  mh::OptionScope option_scope(c ? c->options : nullptr);
  MH_TRY(check_cfg(c, "mh_t5_self_kv_fp8_fill"));
  MH_REQUIRE(workspace && self_kv_fp8, "mh_t5_self_kv_fp8_fill: null argument");
  MH_REQUIRE(c->dtype == MH_BF16, "mh_t5_self_kv_fp8_fill: the e4m3 self-attention cache needs bf16 storage");
  MH_REQUIRE(c->tgt_len <= dec::kSelfIdxMaxTgt, "mh_t5_self_kv_fp8_fill: the index table covers tgt_len <= %d (got %d)",
             dec::kSelfIdxMaxTgt, c->tgt_len);
  MH_REQUIRE(B > 0 && B <= 64, "mh_t5_self_kv_fp8_fill: batch %d not in [1, 64]", B);
  MH_REQUIRE(n_rows >= 1 && n_rows <= B, "mh_t5_self_kv_fp8_fill: %d rows not in [1, %d]", n_rows, B);
  MH_REQUIRE(B % n_rows == 0, "mh_t5_self_kv_fp8_fill: %d rows are not whole groups over %d prompts", B, n_rows);
  MH_REQUIRE(n_pos >= 1 && n_pos < c->tgt_len, "mh_t5_self_kv_fp8_fill: %d positions outside the cache (tgt_len %d)", n_pos, c->tgt_len);
  MH_REQUIRE(workspace_bytes >= mh_t5_decode_workspace_bytes(c, B), "mh_t5_self_kv_fp8_fill: workspace too small");
  return launch_self_kv_quant_rows(c, B, decode_layout(c, B, workspace).bf, (uint8_t*)self_kv_fp8, n_rows, n_pos, (hipStream_t)stream);
}

// positions 0 .. n_pos-1 of Bp prompts through the batched prefill (prefill_prompt: HF's one forward over the prompt) into cache rows
// 0 .. Bp-1 of a B-row step workspace
extern "C" int mh_t5_step_prefill(const MhT5Config* c, const MhT5Weights* w, const void* cross_kv, int Bp, const int32_t* prompt,
                                  const uint8_t* prompt_mask, int P, int n_pos, void* workspace, int64_t workspace_bytes, int B,
                                  void* stream) {
  mh::OptionScope option_scope(c ? c->options : nullptr);
  MH_TRY(check_cfg(c, "mh_t5_step_prefill"));
  MH_TRY(check_decode_shape(c, "mh_t5_step_prefill"));
  MH_REQUIRE(w && cross_kv && prompt && workspace, "mh_t5_step_prefill: null argument");
  MH_REQUIRE(B > 0 && B <= 64, "mh_t5_step_prefill: batch %d not in [1, 64]", B);
  MH_REQUIRE(Bp > 0 && B % Bp == 0, "mh_t5_step_prefill: %d rows are not whole groups over %d prompts", B, Bp);
  MH_REQUIRE(n_pos >= 1 && n_pos <= P && n_pos < c->tgt_len, "mh_t5_step_prefill: %d positions outside the prompt (%d columns) or the cache (tgt_len %d)",
             n_pos, P, c->tgt_len);
  MH_REQUIRE(workspace_bytes >= mh_t5_decode_workspace_bytes(c, B), "mh_t5_step_prefill: workspace too small");
  MH_TRY(check_arch2_weights(c, w, "mh_t5_step_prefill"));
  const DecodeLayout ly = decode_layout(c, B, workspace);
  PrefillBuf pb;
  prefill_layout(c, Bp, n_pos, (char*)workspace + ly.end, workspace_bytes - ly.end, &pb);
  return prefill_prompt(c, w, cross_kv, Bp, Bp, prompt, prompt_mask, P, n_pos, ly.bf.self_k, ly.bf.self_v, pb, (hipStream_t)stream, B);
}
