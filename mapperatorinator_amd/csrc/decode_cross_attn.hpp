// The decode cross-attention with its own query projection -- the HBM-bound kernel of the token step: instantiated in
// decode_attn_bf16.hip / decode_attn_f32.hip (one storage type each) and nowhere else.
#pragma once
#include "decode_device.hpp"

namespace mh {
namespace dec {

// (b, h) of workgroup `blk`; under CFG (B == 2 kv_B) the two rows that share K/V sit in adjacent workgroups
__device__ inline void cross_pair_of_block(const CrossAttnP& p, int blk, int& b, int& h) {
  if (p.kv_B > 0) {
    const int q2 = blk >> 1;
    b = (blk & 1) * p.kv_B + q2 / p.H;
    h = q2 % p.H;
  } else {
    b = blk / p.H;
    h = blk % p.H;
  }
}

// cross-attention of one (b, h) with its own query projection: one 16-wave workgroup, the waves interleave 8-key rows of the
// 1251 encoder keys, partial (max, sum, acc) merged through LDS in wave order -- the reduction order of a row never depends
// on the batch
// F8: K / V are the e4m3 copy (64-byte rows, 8 bytes per lane; the scales multiply the scores and the output)
template <typename T, int KC, int U, bool F8 = false, bool WH = false, bool LN = false>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(8, 8)))   // <= 64 VGPRs: 2 workgroups per CU
void dec_cross_attn_q_kernel(const float* h_, const float* lnw_, const void* W_, const void* k_, const void* v_, int H_, int L_, int d_,
                             int kvB_, CrossAttnP p, HeadProjP hp) {   // leading scalars: preloaded kernel arguments (see gemv_kernel)
  hp.h = h_; hp.ln_w = lnw_; hp.W = W_; hp.ldh = d_; hp.ldw = d_; hp.d = d_;
  p.k = k_; p.v = v_; p.H = H_; p.L = L_; p.kv_B = kvB_;
  constexpr int NW = 16;
  __shared__ float sm[NW][66];
  __shared__ __attribute__((aligned(16))) float xn[1024];
  __shared__ float qs[1][64];
  __shared__ float red16[16];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  int b, h;
  cross_pair_of_block(p, blockIdx.x, b, h);
  MH_STAMP0();
  const int c8 = (lane & 7) * 8, g = lane >> 3;
  const int row0[1] = {h * 64};
  const int kvb = p.kv_B > 0 ? b % p.kv_B : (p.kv_B < 0 ? b / -p.kv_B : b);
  typedef typename std::conditional<F8, fp8_t, T>::type E;
  const E* kb = reinterpret_cast<const E*>(p.k) + ((long)kvb * p.H + h) * p.L * 64;
  const E* vb = reinterpret_cast<const E*>(p.v) + ((long)kvb * p.H + h) * p.L * 64;
  HeadProj<T, KC, 1> proj;
  NormRow<T, LN> nrow;
  // everything the prologue needs is requested at once, from preloaded arguments only: the residual row, the RMSNorm
  // weight and (bf16: fp32 -- the parity path -- would not fit the 64-register budget of two workgroups per CU) this
  // head's 64 x d slice of Wq, which does not depend on the activations; then the remaining kernel arguments
  nrow.issue(hp, b);
  if (sizeof(T) == 2) proj.load(hp, row0);
  // The key stream cannot USE a row before the query exists, but the addresses of every lane group's first K / V row need nothing
  // but kernel arguments.  Three placements of that first request:
  // 1. At kernel entry through LDS-DMA (every wave's first 1-3 key iterations, 32 KB of LDS per iteration, issued as inline asm
  //    behind shadow loads so that no wait of the prologue covers it): 703 / 703 / 729 us per token step for 1 / 2 / 3 iterations
  //    against 679 without.  Not kept.
  // 2. At kernel entry into REGISTERS (32 bytes per lane, beside the prologue's operands): 285.8-286.5 ms per batch against
  //    276.7-277.0 -- the stream's requests queue in front of the weight slice and the residual row the prologue waits for.  Not kept.
  // 3. kEarlyKV, below: into registers AFTER the row is normalised -- the prologue's operands have arrived, nothing of this workgroup
  //    is queued -- and BEFORE the projection's arithmetic, ~0.9 us of VALU and LDS work with no vector-memory request
  //    outstanding, which now covers the round trip that attend_keys used to start behind the projection's barrier.  Kept: the
  //    kernel 14.39 -> 13.64 us at 16 rows, 260.13 -> 256.21 ms per batch (profiles/decode_early_kv.txt).
  // bf16 storage only: the fp32 weight slice is requested after the normalisation and would queue behind the K / V rows.  Not the
  // Whisper family (WH): with 8 (bf16) / 4 (e4m3) more registers live across the projection its bf16 forms at d = 768 and 896 spill
  // and others reach the 64 registers that two workgroups per CU allow; the family keeps the old order.
  constexpr bool kEarlyKV = sizeof(T) == 2 && !WH;
  FirstKeys<E, U> first;
  unsigned long long t_start = 0;
  if (p.tstamp && threadIdx.x == 0) t_start = (unsigned long long)wall_clock64();
  nrow.finish(hp, xn, red16);
  MH_STAMP(KID_CROSS, 0);   // row normalised
  if (sizeof(T) != 2) proj.load(hp, row0);
  if constexpr (kEarlyKV) first.issue(kb, vb, wid * 8 + g, p.L, 8 * NW);
  proj.apply(xn, qs, WH ? p.q_bias : nullptr, row0);
  __syncthreads();
  MH_STAMP(KID_CROSS, 1);   // query projected
  float q[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) q[i] = qs[0][c8 + i];
  const float ks = (F8 ? p.kscale[kvb * p.H + h] : 1.0f) * (WH ? p.scale : 1.0f), vs = F8 ? p.vscale[kvb * p.H + h] : 1.0f;
  Partial st;
  partial_init(st);
  attend_keys<T, U, E, false, false, kEarlyKV>(st, q, kb, vb, wid * 8 + g, p.L, 8 * NW, nullptr, 0, nullptr, 0, ks, 0, nullptr, nullptr,
                                               nullptr, 0, &first);
  MH_STAMP(KID_CROSS, 2);   // keys streamed (this wave)
  partial_merge_groups<T>(st);
  float m, l, a;
  block_merge<T, NW>(st, sm, m, l, a);
  MH_STAMP(KID_CROSS, 3);   // partials merged
  if (threadIdx.x < 64) {
    // (threadIdx.x < 64: the thread index IS the lane.  The e4m3 Whisper instantiations say so: the d = 768 one sits at the 64-register
    // limit and would otherwise keep threadIdx.x & 63 of the prologue alive in scratch for this one use)
    const int lane_st = (F8 && WH) ? (int)threadIdx.x : (int)(threadIdx.x & 63);
    store_head_row_wt<T>(reinterpret_cast<T*>(p.out) + (long)b * p.ldo + h * 64, l > 0.f ? a / l * vs : 0.f, &sm[0][0], lane_st);
  }
  if (p.tstamp && threadIdx.x == 0 && *p.pos < p.ts_ring) {      // the first ts_ring positions of the call, one slot each
    unsigned long long* slot = p.tstamp + 2 * ((long)(*p.pos) * p.ts_layers + p.ts_layer);
    atomicMin(slot, t_start);
    atomicMax(slot + 1, (unsigned long long)wall_clock64());
  }
}

}  // namespace dec
}  // namespace mh
