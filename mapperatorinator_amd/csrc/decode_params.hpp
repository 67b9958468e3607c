// The token step's kernel arguments as the host fills them: the parameter structs and the constants a launch is chosen by.  No device
// code: t5_step.hip describes a step's operands from this header alone; the family headers (decode_gemv.hpp, decode_self_attn.hpp,
// decode_cross_attn.hpp) say what the kernels make of every field.
#pragma once
#include <stdint.h>

namespace mh {
namespace dec {

// ---- decode GEMV (decode_gemv.hpp) --------------------------------------------------------------------------------------------
enum { PRO_PLAIN = 0, PRO_RMSNORM = 1, PRO_LAYERNORM = 2 };   // (LAYERNORM: HF Whisper's affine nn.LayerNorm, library arch 2)
enum { SK_GEGLU = 2, SK_RESID = 3, SK_LOGITS = 4, SK_GELU_ERF = 5 };   // (GELU_ERF: the Whisper family's fc1)

struct SkinnyP {
  const void* A; int lda;      // PRO_PLAIN: T [B, lda];  PRO_RMSNORM: fp32 residual stream [B, lda]
  const float* ln_w; float eps;
  const void* W; int ldw;      // [N, ldw] element type T
  int B, N, K;
  int nv;                      // real columns per 16-column tile: 16, 8 or 4 (GEGLU: 8 gate + 8 linear)
  void* out; int ldo;          // GEGLU / GELU_ERF: T [B, ldo] (GEGLU: N/2 cols); LOGITS: f32 [B, ldo]
  float* h; int ldh;           // RESID: h[b][n] += acc
  void* kc; void* vc;          // (unused: kept so that the kernel-argument layout stays put)
  int H, tgt_len, inner;       // (unused)
  const int* pos;              // (unused)
  const float* bias;           // kernel template BIAS (the Whisper family's biased projections): fp32 [N], else unused
  const float* ln_b;           // PRO_LAYERNORM: the LayerNorm bias fp32 [K] (ln_w = its weight, eps = its epsilon)
};
constexpr int kGemvCH = 8;   // k-blocks per wave whose loads are in flight at once (one pass)

// the three-GEMV tail of a layer as one launch (dec_tail_kernel, decode_gemv.hpp)
struct TailP {
  SkinnyP o, wi, wo;
  unsigned* cnt;            // generation counter of this chain and layer parity
  int* err;                 // DecState::tail_err of the chain
  int G;                    // workgroups of this launch
  long long timeout_ticks;  // wall_clock64() ticks a workgroup may live (2 ms)
};

// ---- self-attention (decode_self_attn.hpp) --------------------------------------------------------------------------------------
constexpr int kSelfIdxMaxTgt = 2560;   // table entries of one row staged in LDS (the released tgt_seq_len)
struct SelfAttnP {
  const void* q; int ldq;         // (unused: kept so that the kernel-argument layout stays put)
  const void* kc; const void* vc; // [B][H][tgt_len][64]
  const float* bias;              // fp32 [H][tgt_len] by distance pos - j
  const uint8_t* prompt_mask; int P;
  void* out; int ldo;             // T [B, inner]
  int B, H, tgt_len;
  const int* pos;
  // the Whisper family (kernel template WH; modeling_varwhisper.py:229-258,381-568): fp32 bias of this layer's fused
  // Wqkv [3 inner] or NULL; rotary table fp32 [tgt_len][64] = cos(32) | sin(32) of every position (built on the host with
  // the reference's formulas, already rounded to the storage type); score scale; window > 0: keys older than
  // pos - window are not attended (local layers under the flash-attention path, :330)
  const float* qkv_bias; const float* rope; float scale; int window;
};
// the self-attention kernel's trailing argument: this layer's shadow rows of the chain's first row (F8 instantiations), or nothing
struct SelfKv8P {
  uint8_t* k8; uint8_t* v8;      // e4m3 [B][H][tgt_len][64]
  float* ks; float* vs;          // fp32 scales [B][H][tgt_len]
};
struct NoSelfKv8P {};
// ... or the index table of a beam search (IDX instantiations, mh_t5_step_indexed): uint8 [B][tgt_len], entry [b][j] = the cache row
// that holds key / value j of decode row b
struct SelfIdxP {
  const uint8_t* origin;
};
// ... or both (F8 with IDX, mh_t5_step_indexed_skv8): the shadow rows and their scales are read through the table as well
struct SelfKv8IdxP : SelfKv8P {
  const uint8_t* origin;
};
// ... or the positions of an in-flight decode (SLOT instantiations, mh_t5_slots_*): int32 [rows of the chain], entry b = the position
// row b is fed at this step, negative = the slot is idle
struct SelfSlotP {
  const int* slot_pos;
};
// ... or both (F8 with SLOT, mh_t5_slots_open_kv8): row b attends shadow row b below its own position and appends there
struct SelfKv8SlotP : SelfKv8P {
  const int* slot_pos;
};

// ---- cross-attention (decode_cross_attn.hpp) ------------------------------------------------------------------------------------
struct CrossAttnP {
  const void* q; int ldq;   // (unused: kept so that the kernel-argument layout stays put)
  const void* k; const void* v;  // this layer's [B][H][L][64]
  void* out; int ldo;       // T [B, inner]
  int B, H, L;
  int kv_B;                 // > 0: row b reads K/V row b % kv_B (CFG pairs share the encoder output);
                            // < 0: row b reads K/V row b / -kv_B (the beams of a chunk share it: rows are (chunk, beam))
  const float* kscale; const float* vscale;   // fp8 rows (kernel template F8): this layer's [kv rows][H] scales, else NULL
  // measurement only (mh_t5_decode_timing): [slots][2] = (earliest workgroup start, latest workgroup end) of THIS
  // launch in wall-clock ticks, slot = *pos * ts_layers + ts_layer for the first ts_ring positions; NULL in production
  unsigned long long* tstamp; const int* pos; int ts_ring, ts_layers, ts_layer;
  // the Whisper family (kernel template WH): fp32 bias of this layer's query projection [inner] or NULL, and the score scale
  const float* q_bias; float scale;
};

// ---- the projection an attention kernel does for itself (HeadProj, decode_device.hpp) --------------------------------------------
struct HeadProjP {
  const float* h; int ldh;            // fp32 residual stream [B, ldh]
  const float* ln_w; float eps;
  const void* W; int ldw;             // [rows, ldw] element type T (cross: Wq [inner][d]; self: Wqkv [3 inner][d])
  int d;
  const float* ln_b;                  // kernel template LN (HF Whisper, library arch 2): affine nn.LayerNorm -- its bias; ln_w = its weight
};

}  // namespace dec
}  // namespace mh
