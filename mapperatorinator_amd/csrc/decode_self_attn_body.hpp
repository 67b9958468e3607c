// The body of the decode self-attention kernels (decode_self_attn.hpp), as TEXT: included inside dec_self_attn_qkv_kernel and inside
// dec_slot_self_attn_kernel, which differ in the constant SLOT alone.  (A shared __device__ function -- inlined, arguments by value or
// by reference -- compiled 112 to 142 of the 144 existing instantiations to other instruction bytes; the text does not.)  In scope where
// it is included: T, KC, WH, LN, F8, IDX, SLOT; the kernel arguments h_, lnw_, W_, pos_, kc_, vc_, H_, d_, p, hp and f8 (the trailing
// argument: the shadow rows, the index table, both, the slot positions, the shadow rows with the slot positions, or nothing).
  static_assert(!F8 || sizeof(T) == 2, "the e4m3 shadow cache is made of bf16 rows");
  static_assert(!SLOT || !IDX, "the slot form has no index table");
  hp.h = h_; hp.ln_w = lnw_; hp.W = W_; hp.ldh = d_; hp.ldw = d_; hp.d = d_;
  p.pos = pos_; p.kc = kc_; p.vc = vc_; p.H = H_;
  const int inner = H_ * 64;
  constexpr int NW = 16;
  __shared__ float sm[NW][66];
  __shared__ __attribute__((aligned(16))) float xn[1024];
  __shared__ float qkv[3][64];
  __shared__ float red16[16];
  MH_STAMP0();
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int b = blockIdx.x / p.H, h = blockIdx.x % p.H;
  const int c8 = (lane & 7) * 8, g = lane >> 3;
  // the first round trip carries everything that does not depend on another load: the residual row + RMSNorm weight, the
  // position, and the two loop-invariant values of the tail (the bias at distance 0 and the prompt mask of the new key:
  // they used to be two serial round trips at the END of the kernel)
  NormRow<T, LN> nrow;
  nrow.issue(hp, b);
  uint8_t* org = nullptr;
  if constexpr (IDX) {
    __shared__ uint8_t org_lds[kSelfIdxMaxTgt];
    org = org_lds;
    // this row's table entries, all tgt_len of them (the position is itself a load: nothing here waits for it), clamped to the
    // batch so that no table content can send a K / V load outside the cache; visible to every wave after the barriers of
    // nrow.finish
    const uint8_t* orow = f8.origin + (long)b * p.tgt_len;
    uint8_t o3[3];
#pragma unroll
    for (int u = 0; u < 3; ++u) {
      const int i = (int)threadIdx.x + u * 1024;
      o3[u] = orow[i < p.tgt_len ? i : 0];
    }
#pragma unroll
    for (int u = 0; u < 3; ++u) {
      const int i = (int)threadIdx.x + u * 1024;
      if (i < p.tgt_len && i < kSelfIdxMaxTgt) org[i] = (int)o3[u] < p.B ? o3[u] : (uint8_t)(p.B - 1);
    }
  }
  int pos;
  if constexpr (SLOT) {
    pos = f8.slot_pos[b];
    // an idle slot (the whole workgroup: the entry is one word): nothing is stored, no barrier was reached.  (An entry past the
    // cache cannot come from the sampler or the admission; it is refused here, so no content of the array can store out of bounds)
    // F8: the append to the shadow is behind this return as well
    if (pos < 0 || pos >= p.tgt_len) return;
  } else {
    pos = *p.pos;
  }
  // (F8, the Whisper family at d = 896: the scale pairs of the key loop on top of the 21 weight vectors spill; one projection at a
  // time, as d = 1024 -- the same sums in the same order)
  constexpr bool kAllAtOnce = sizeof(T) == 2 && KC <= ((F8 && WH) ? 6 : 7);
  HeadProj<T, KC, kAllAtOnce ? 3 : 1, WH> proj;
  const int row03[3] = {h * 64, inner + h * 64, 2 * inner + h * 64};
  const float* bias_row = WH ? nullptr : p.bias + (long)h * p.tgt_len;       // (the Whisper family has no additive bias)
  const uint8_t* mask_row = p.prompt_mask ? p.prompt_mask + (long)b * p.P : nullptr;
  const float bias0 = WH ? 0.f : bias_row[0];
  float rope_c = 1.f, rope_s = 0.f;
  if (WH) {   // cos / sin of this position for rotary pair (threadIdx.x & 31)
    rope_c = p.rope[(long)pos * 64 + (threadIdx.x & 31)];
    rope_s = p.rope[(long)pos * 64 + 32 + (threadIdx.x & 31)];
  }
  const int new_key_mask = (mask_row && pos < p.P) ? (int)mask_row[pos < p.P ? pos : 0] : 1;
  nrow.finish(hp, xn, red16);
  const float* qb = WH ? p.qkv_bias : nullptr;
  if (kAllAtOnce) {
    proj.load3(hp, row03);   // (requested AFTER the normalisation: holding the 18 vectors across it measured 688 vs 677 us per token step)
    proj.apply(xn, qkv, qb, row03);
  } else {   // fp32 storage, or d_model = 1024 in bf16: one projection at a time (register budget of a 1024-thread workgroup)
#pragma unroll
    for (int q3 = 0; q3 < 3; ++q3) {
      const int row0[1] = {q3 * inner + h * 64};
      HeadProj<T, KC, 1, WH> proj1;
      proj1.load(hp, row0);
      proj1.apply(xn, qkv + q3, qb, row0);
    }
  }
  __syncthreads();
  if (WH) {
    // rotate-half RoPE on q and k (apply_rotary_pos_emb, modeling_varwhisper.py:236-258): pair (i, i + 32) of a head ->
    // (x1 cos - x2 sin, x2 cos + x1 sin), T-rounded; threads 0..63 = q, 64..127 = k
    float rot = 0.f;
    const int t = threadIdx.x;
    if (t < 128) {
      const float* x = qkv[t >> 6];
      const int i = t & 31;
      const float x1 = x[i], x2 = x[i + 32];
      rot = (t & 32) ? x2 * rope_c + x1 * rope_s : x1 * rope_c - x2 * rope_s;
    }
    __syncthreads();
    if (t < 128) qkv[t >> 6][t & 63] = Elem<T>::to_f32(Elem<T>::from_f32(rot));
    __syncthreads();
  }
  MH_STAMP(KID_SELF, 0);    // q / k / v projected
  T* kcache = reinterpret_cast<T*>(const_cast<void*>(p.kc)) + ((long)b * p.H + h) * p.tgt_len * 64;
  T* vcache = reinterpret_cast<T*>(const_cast<void*>(p.vc)) + ((long)b * p.H + h) * p.tgt_len * 64;
  store_head_row_from_lds_wt<T>(kcache + (long)pos * 64, qkv[1], (int)threadIdx.x - 64);     // waves 1 / 2: whole 16-byte pieces
  store_head_row_from_lds_wt<T>(vcache + (long)pos * 64, qkv[2], (int)threadIdx.x - 128);
  if constexpr (F8) {   // waves 1 / 2 own the new k / v rows: append them to the shadow (wave-uniform branch)
    const long bh = (long)b * p.H + h;
    if (wid == 1) quant_row64(qkv[1][lane], f8.k8 + (bh * p.tgt_len + pos) * 64, f8.ks + bh * p.tgt_len + pos);
    if (wid == 2) quant_row64(qkv[2][lane], f8.v8 + (bh * p.tgt_len + pos) * 64, f8.vs + bh * p.tgt_len + pos);
  }
  float q[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) q[i] = qkv[0][c8 + i];
  Partial st;
  partial_init(st);
  const float sc = WH ? p.scale : 1.0f;
  int j_first = 0;
  if (WH && p.window > 0 && pos - p.window > 0) j_first = (pos - p.window) & ~(8 * NW - 1);   // whole key iterations below the window are skipped
  if constexpr (F8 && IDX) {   // head h of shadow row 0 (bytes and scales); every key adds the offsets of the row that holds it
    const long row_stride = (long)p.H * p.tgt_len * 64, hh = (long)h * p.tgt_len;
    attend_keys<T, 2, fp8_t, true, true>(st, q, reinterpret_cast<const fp8_t*>(f8.k8) + hh * 64, reinterpret_cast<const fp8_t*>(f8.v8) + hh * 64,
                                         j_first + wid * 8 + g, pos, 8 * NW, bias_row, pos, mask_row, p.P, sc,
                                         (WH && p.window > 0) ? pos - p.window : 0, f8.ks + hh, f8.vs + hh, org, row_stride);
  } else if constexpr (F8) {
    const long bh = (long)b * p.H + h;
    attend_keys<T, 2, fp8_t, true>(st, q, reinterpret_cast<const fp8_t*>(f8.k8) + bh * p.tgt_len * 64,
                                   reinterpret_cast<const fp8_t*>(f8.v8) + bh * p.tgt_len * 64, j_first + wid * 8 + g, pos, 8 * NW,
                                   bias_row, pos, mask_row, p.P, sc, (WH && p.window > 0) ? pos - p.window : 0,
                                   f8.ks + bh * p.tgt_len, f8.vs + bh * p.tgt_len);
  } else if constexpr (IDX) {   // head h of cache row 0; every key adds its own row's offset
    const long row_stride = (long)p.H * p.tgt_len * 64;
    attend_keys<T, 2, T, false, true>(st, q, kcache - (long)b * row_stride, vcache - (long)b * row_stride, j_first + wid * 8 + g, pos,
                                      8 * NW, bias_row, pos, mask_row, p.P, sc, (WH && p.window > 0) ? pos - p.window : 0, nullptr,
                                      nullptr, org, row_stride);
  } else {
    attend_keys<T, 2>(st, q, kcache, vcache, j_first + wid * 8 + g, pos, 8 * NW, bias_row, pos, mask_row, p.P, sc,
                      (WH && p.window > 0) ? pos - p.window : 0);
  }
  MH_STAMP(KID_SELF, 1);    // cached keys attended (this wave)
  partial_merge_groups<T>(st);
  float m, l, a;
  block_merge<T, NW>(st, sm, m, l, a);
  MH_STAMP(KID_SELF, 2);    // partials merged
  if (threadIdx.x < 64) {
    const int d = threadIdx.x;
    float sn = wave_sum(qkv[0][d] * qkv[1][d]) * sc + bias0;
    if (new_key_mask == 0) sn = -INFINITY;
    const float mn = fmaxf(m, sn);
    const float fa = fexp<T>(m - mn), fb = fexp<T>(sn - mn);
    l = l * fa + fb;
    a = a * fa + qkv[2][d] * fb;
    store_head_row_wt<T>(reinterpret_cast<T*>(p.out) + (long)b * p.ldo + h * 64, l > 0.f ? a / l : 0.f, &sm[0][0]);
  }
