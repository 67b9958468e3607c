// Host-side helpers shared by the T5 / Whisper-family units (t5_encode.hip, t5_step.hip and the decode_* units, t5_generate.hip, t5_stepwise.hip):
// configuration checks, the storage-type / d_model / attention-form dispatch, the layout of the packed e4m3 K/V copies.
// Inline, host only: no kernel is declared or instantiated here.
#pragma once
#include <type_traits>

#include "internal.hpp"

namespace mh {

inline int es_of(int dtype) { return dtype == MH_BF16 ? 2 : 4; }

inline int check_cfg(const MhT5Config* c, const char* who) {
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
inline int check_decode_shape(const MhT5Config* c, const char* who) {
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
inline int check_arch2_weights(const MhT5Config* c, const MhT5Weights* w, const char* who) {
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

}  // namespace mh
