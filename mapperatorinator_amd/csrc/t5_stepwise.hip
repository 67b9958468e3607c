// Step-wise decode for host-driven search (beam search): one token step per call over the decode workspace (mh_t5_step*), the
// self-attention cache reorder by copy and by index table, the e4m3 shadow fill and the step workspace's prompt prefill.  The step
// itself is t5_step.hip's (decode_step.hpp); the small copy / table kernels of the search live here.
#include <stdlib.h>
#include <string.h>

#include "decode_step.hpp"
#include "t5_host.hpp"

using namespace mh;

namespace mh {
namespace {
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
}  // namespace
}  // namespace mh

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
  MH_TRY(launch_step_embed(c->dtype, ids, w->dec_embed, c->d_model, k.bf.h, k.bf.st, pos, dpos, pmask, P, B, s));
  return enqueue_step(k, s);
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
