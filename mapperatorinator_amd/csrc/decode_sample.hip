// The small kernels around a token step: the ONE unit that instantiates the sampler, the init kernels, finalize and the step-wise
// embed (decode_sample.hpp), and their launchers.  The e4m3 K/V quantisers -- three small kernels that only prepare what the token
// steps stream -- are kept here too, with their launchers and the two C entries that launch them directly.  The other units reach
// all of it through decode_step.hpp.
#include "decode_sample.hpp"

using namespace mh;

namespace mh {
int launch_sample(int dtype, const StepCall& k, hipStream_t s) {
  const SampleP& smp = k.smp;
  const int B = k.Bc;
  return dispatch_dtype(dtype, [&](auto t) -> int {
    using T = decltype(t);
    if (k.slot_pos) {
      MH_REQUIRE(k.has_rows && (smp.pair == 0 || (smp.b0 == 0 && B == 2 * smp.pair)),
                 "decode: the slot form of the sampler reads row settings; its guided form is one chain of whole pairs");
      SlotSetP ss{};
      ss.rows = k.rows.rows; ss.eos_tables = k.rows.eos_tables; ss.n_eos_sets = k.rows.n_eos_sets; ss.pos = k.slot_pos; ss.plen = k.slot_plen;
      if (smp.pair > 0) hipLaunchKernelGGL((dec_sample_kernel<T, true, true, true>), dim3(smp.pair), dim3(256), 0, s, smp, ss);   // one workgroup per pair
      else hipLaunchKernelGGL((dec_sample_kernel<T, true, true>), dim3(B), dim3(256), 0, s, smp, ss);
    } else if (k.has_rows) hipLaunchKernelGGL((dec_sample_kernel<T, true>), dim3(smp.pair > 0 ? smp.pair : B), dim3(256), 0, s, smp, k.rows);
    else hipLaunchKernelGGL((dec_sample_kernel<T, false>), dim3(smp.pair > 0 ? smp.pair : B), dim3(256), 0, s, smp, NoRowSetP{});
    return check_launch("dec_sample_kernel");
  });
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
  return dispatch_dtype(dtype, [&](auto t) -> int {
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
