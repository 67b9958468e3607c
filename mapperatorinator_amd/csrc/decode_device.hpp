// Device kernels of the KV-cached autoregressive T5 decode step (K5 / K6).
//
// One token step of one layer is SIX dependent kernels per row chain (a chain = up to 16 rows; two chains run side by
// side): [RMSNorm + this head's q / k / v projection + self-KV append + self-attention over the cache] -> [O GEMV +
// residual] -> [RMSNorm + this head's query projection + cross-attention over the 1251 encoder keys: THE HBM-bound
// kernel, B*H*L*64*2 elements per layer per step] -> [O GEMV + residual] -> [RMSNorm + wi GEMV + gated GELU] -> [wo GEMV
// + residual]; then final RMSNorm + lm_head GEMV and the sampler (decode_sample.hpp).  Every kernel reads the current position
// from device memory, so a chain's step is one replayable hipGraph.  Under option decode_fused_tail the last THREE of the six
// are one launch (dec_tail_kernel: the same GEMV code per phase, two bounded in-kernel hand-offs): four nodes per layer.
//
// What shapes these kernels (measured): a dependent kernel costs ~3.3 us before it does anything (launch,
// first-load latency, store flush), so each does its whole job in one or two memory round trips; the CU's load path is
// charged per 128-byte line touched, so operands are loaded as whole lines (weights of the attention kernels' own
// projections; the GEMVs' activations through a wave-private LDS patch) and only where that is impossible as MFMA-
// fragment-shaped pieces; everything handed to the next kernel is stored write-through.
//
// GEMVs ("skinny GEMMs", M = rows of the chain): a workgroup owns one 16-column MFMA tile (4, 8 or 16 real columns),
// its 4 or 8 waves split K, weight fragments go straight from L2 / HBM into registers (read once), the partial
// accumulators are added through LDS in wave order (deterministic, independent of the batch).
//
// This header: what more than one kernel family uses.  The families are decode_gemv.hpp (GEMV, fused tail), decode_self_attn.hpp,
// decode_cross_attn.hpp and decode_sample.hpp (sampler, init, embed, finalize).  decode_gemv.hip and decode_sample.hip instantiate
// the header of their name; the two attention headers are instantiated together, once per storage type (decode_attn_bf16.hip,
// decode_attn_f32.hip).  The kernel arguments the host fills are in decode_params.hpp.
#pragma once
#include <string.h>

#include <type_traits>

#include "decode_params.hpp"
#include "internal.hpp"

namespace mh {
namespace dec {

// ---- phase stamps (profiling build only: `make prof` defines MH_PHASE_STAMPS) --------------------------------------------
// Thread 0 of workgroup 0 adds (shader-clock ticks since its first instruction) to g_stamps[kernel][stamp] at marked
// points; tools/decode_phases.py prints the averages.  The production library contains none of this.
// Every unit that includes this header has a table of its own (static: one per code object) and writes the rows of its own kernels'
// ids only; mh_debug_phase_stamps (t5_step.hip) adds the units' tables up through their *_phase_stamps functions (decode_step.hpp).
// Sums and counts add, so the total is the table one shared array would hold.
#ifdef MH_PHASE_STAMPS
static __device__ unsigned long long g_stamps[16 * 16 * 2];   // [kernel id][stamp][sum of ticks, count]
// acc (host, uint64 [16][16][2]) += this unit's table; reset: the table is cleared afterwards
static inline int take_phase_stamps(unsigned long long* acc, int reset) {
  static unsigned long long buf[16 * 16 * 2];
  if (acc) {
    if (hipMemcpyFromSymbol(buf, HIP_SYMBOL(g_stamps), sizeof(buf)) != hipSuccess) return check_launch("stamps read");
    for (int i = 0; i < 16 * 16 * 2; ++i) acc[i] += buf[i];
  }
  if (reset) {
    memset(buf, 0, sizeof(buf));
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), buf, sizeof(buf)) != hipSuccess) return check_launch("stamps reset");
  }
  return MH_OK;
}
#define MH_STAMP0() unsigned long long mh_t0_ = 0; if (blockIdx.x == 0 && threadIdx.x == 0) mh_t0_ = clock64()
#define MH_STAMP(kid, i)                                                              \
  do {                                                                                \
    if (blockIdx.x == 0 && threadIdx.x == 0) {                                        \
      atomicAdd(&g_stamps[((kid) * 16 + (i)) * 2], (unsigned long long)clock64() - mh_t0_); \
      atomicAdd(&g_stamps[((kid) * 16 + (i)) * 2 + 1], 1ull);                         \
    }                                                                                 \
  } while (0)
#define MH_T0_PARAM , unsigned long long mh_t0_   /* a device function that stamps on behalf of its kernel takes the kernel's t0 */
#define MH_T0_ARG , mh_t0_
#else
#define MH_STAMP0() do {} while (0)
#define MH_STAMP(kid, i) do {} while (0)
#define MH_T0_PARAM
#define MH_T0_ARG
#endif
enum { KID_GEMV = 0 /* + EPI * 2 + (NWV == 8) */, KID_SELF = 10, KID_CROSS = 11, KID_SAMPLE = 12, KID_TAIL = 13 };

// ---- 8-element chunk helpers ----------------------------------------------------------------
// streaming (non-temporal) variants for data that is read once per launch (K/V rows of the decode attention):
// `global_load_dwordx4 ... nt` keeps the 1.5 GB/step K/V stream from evicting the decoder weights (226 MB) out of
// the 256 MB Infinity Cache between token steps.
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2_t;
// The two halves of a streamed chunk: `load` only REQUESTS the 8 elements as they lie in memory (16 bytes per lane for bf16, 8 for
// e4m3), `unpack` widens them where they are used -- a request can then be issued long before its data is needed at the cost of
// the raw registers alone (Raw8 below does the same for the weights).
template <typename T> struct StreamRaw8;
template <> struct StreamRaw8<bf16_t> {
  u32x4_t v;
  __device__ inline void load(const bf16_t* p) { v = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(p)); }
  __device__ inline void unpack(float (&o)[8]) const {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      o[2 * i] = __uint_as_float(v[i] << 16);
      o[2 * i + 1] = __uint_as_float(v[i] & 0xffff0000u);
    }
  }
};
template <> struct StreamRaw8<float> {
  u32x4_t a, b;
  __device__ inline void load(const float* p) {
    a = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(p));
    b = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(p + 4));
  }
  __device__ inline void unpack(float (&o)[8]) const {
#pragma unroll
    for (int i = 0; i < 4; ++i) { o[i] = __uint_as_float(a[i]); o[4 + i] = __uint_as_float(b[i]); }
  }
};
// OCP e4m3 rows (the fp8 copy of the cross-attention K / V): 8 elements = 8 bytes per lane
struct fp8_t { uint8_t v; };
typedef __attribute__((ext_vector_type(2))) float f32x2_t;
template <> struct StreamRaw8<fp8_t> {
  u32x2_t v;
  __device__ inline void load(const fp8_t* p) { v = __builtin_nontemporal_load(reinterpret_cast<const u32x2_t*>(p)); }
  __device__ inline void unpack(float (&o)[8]) const {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const f32x2_t lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)v[i], false);
      const f32x2_t hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)v[i], true);
      o[4 * i] = lo[0]; o[4 * i + 1] = lo[1]; o[4 * i + 2] = hi[0]; o[4 * i + 3] = hi[1];
    }
  }
};
template <typename T> __device__ inline void load8_stream(const T* p, float (&o)[8]) {
  StreamRaw8<T> r;
  r.load(p);
  r.unpack(o);
}
template <typename T> __device__ inline void store8(T* p, const float (&o)[8]);
template <> __device__ inline void store8<bf16_t>(bf16_t* p, const float (&o)[8]) {
  uint32_t w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) w[i] = pack_bf16x2(o[2 * i], o[2 * i + 1]);
  *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
}
template <> __device__ inline void store8<float>(float* p, const float (&o)[8]) {
  *reinterpret_cast<float4*>(p) = make_float4(o[0], o[1], o[2], o[3]);
  *reinterpret_cast<float4*>(p + 4) = make_float4(o[4], o[5], o[6], o[7]);
}

template <typename T> __device__ inline void store4(T* p, float a, float b, float c, float d);
template <> __device__ inline void store4<bf16_t>(bf16_t* p, float a, float b, float c, float d) {
  *reinterpret_cast<uint2*>(p) = make_uint2(pack_bf16x2(a, b), pack_bf16x2(c, d));
}
template <> __device__ inline void store4<float>(float* p, float a, float b, float c, float d) {
  *reinterpret_cast<float4*>(p) = make_float4(a, b, c, d);
}

// Everything a decode kernel hands to the NEXT kernel is stored write-through ("agent scope", `global_store ... sc1`):
// the release at the end of a kernel writes back the dirty lines of every XCD's L2, and with two decode chains on the
// chip each chain's kernel boundaries also pay for the other chain's dirty lines.  With nothing dirty the boundary is
// cheaper: tools/micro/gemv_probe, o-projection 3.53 -> 3.37 us alone, 4.60 -> 4.08 us beside a second chain; the
// K = 2048 projection 6.35 -> 5.54 us (non-temporal stores: no gain).
// hipcc's scheduler sinks loads next to their first use when it believes registers are scarce (`load, s_waitcnt vmcnt(0),
// use, load, ...`: one memory round trip PER LOAD instead of one per kernel -- found in the 8-wave GEMV and, after an
// unrelated edit, in the 4-wave one: tools/isa_mem_signature.py shows it).  The cure is to tell it that registers are
// not scarce (amdgpu_waves_per_eu on the kernels below); __builtin_amdgcn_sched_barrier at this marker was tried and is
// worse: the kernel's private arrays are then promoted to LDS (a dispatch-packet read plus LDS round trips).
#define MH_LOADS_ISSUED() do {} while (0)

// (Naming the not-preloaded kernel arguments in an empty `asm volatile("" :: "s"(arg))` right after the vector loads, so
// that their s_load overlaps the vector round trip, was measured: 677 -> 840 us per token step.  Not kept.)

template <typename U>
__device__ inline void store_wt(U* p, U v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// 16- / 8-byte write-through stores (`__hip_atomic_store` stops at 8 bytes).  A 2- or 4-byte write-through store is one
// fabric write each (MI355X_MICROARCH.md: per byte, dword ~6x and short ~12.5x the dwordx4 time): the decode kernels stage
// what they hand on through LDS and write whole 16-byte pieces of a row.
__device__ inline void store16_wt(void* p, u32x4_t v) { asm volatile("global_store_dwordx4 %0, %1, off sc1" : : "v"(p), "v"(v) : "memory"); }
__device__ inline void store8_wt(void* p, u32x2_t v) { asm volatile("global_store_dwordx2 %0, %1, off sc1" : : "v"(p), "v"(v) : "memory"); }
// n consecutive fp32 values (n = 4 or 8) -> one write-through store of n T elements when the destination is aligned to
// the piece, else element by element
template <typename TO>
__device__ inline void store_piece_wt(TO* dst, const float* v, int n, int nvalid) {
  const bool whole = nvalid == n && (reinterpret_cast<uintptr_t>(dst) & (n * sizeof(TO) - 1)) == 0;
  if (whole && sizeof(TO) == 4 && n == 4) {
    store16_wt(dst, u32x4_t{__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])});
  } else if (whole && sizeof(TO) == 2 && n == 8) {
    store16_wt(dst, u32x4_t{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7])});
  } else if (whole && sizeof(TO) == 2 && n == 4) {
    store8_wt(dst, u32x2_t{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])});
  } else {
    for (int i = 0; i < nvalid; ++i) store_wt(dst + i, Elem<TO>::from_f32(v[i]));
  }
}

// One wave holds the 64 values of a head row (lane = feature): through a wave-private 64-float LDS patch (one wave's LDS
// operations execute in order: no barrier) to 16-byte pieces, written by the first 8 (bf16) / 16 (fp32) lanes.
template <typename T>
__device__ inline void store_head_row_wt(T* dst, float val, float* patch, int lane) {
  constexpr int N = 16 / (int)sizeof(T);
  patch[lane] = val;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  if (lane < 64 / N) {
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = i < N ? patch[lane * N + i] : 0.f;
    store_piece_wt<T>(dst + lane * N, v, N, N);
  }
}
template <typename T>
__device__ inline void store_head_row_wt(T* dst, float val, float* patch) { store_head_row_wt<T>(dst, val, patch, threadIdx.x & 63); }
// the same from 64 floats that already sit in LDS (visible to the calling wave): lanes `lane0 .. lane0 + 64 / N` of the block
template <typename T>
__device__ inline void store_head_row_from_lds_wt(T* dst, const float* src, int t) {   // t = thread index relative to the first storing thread
  constexpr int N = 16 / (int)sizeof(T);
  if (t >= 0 && t < 64 / N) {
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = i < N ? src[t * N + i] : 0.f;
    store_piece_wt<T>(dst + t * N, v, N, N);
  }
}

// ---- single-query attention (online softmax in registers) -----------------------------------------
// lane = (key group g = lane>>3, dim chunk c = lane&7): 8 lanes cover the 64 dims of one key row
// (one 128-byte / 256-byte row per 8 lanes -> every wave load instruction is 8 consecutive rows).
struct Partial {
  float m, l;
  float acc[8];
};
__device__ inline void partial_init(Partial& s) {
  s.m = -1e30f; s.l = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) s.acc[i] = 0.f;
}
template <typename T>
__device__ inline void partial_merge_groups(Partial& s) {  // across the 8 key groups of a wave
  // rescale to the wave-wide maximum first (ONE exponential per lane), then plain shuffle sums: no exponential sits in
  // the 3-level reduction chain
  // (partners 8, 16, 32 on the VALU -- row_ror:8, then the row and half swaps; the whole wave calls this)
  const float mw = across_groups8_max(s.m);
  const float f = fexp<T>(s.m - mw);
  s.l *= f;
#pragma unroll
  for (int i = 0; i < 8; ++i) s.acc[i] *= f;
  s.l = across_groups8_sum(s.l);
#pragma unroll
  for (int i = 0; i < 8; ++i) s.acc[i] = across_groups8_sum(s.acc[i]);
  s.m = mw;
}

// The first iteration of a lane group -- keys j0, j0 + jstride, ..., U of them, K and V -- as its caller requested it AHEAD of the loop:
// raw, as the rows lie in memory (16 bytes per lane and matrix for bf16, 8 for e4m3), unpacked only where attend_keys uses them.  The
// addresses need nothing but kernel arguments, so a kernel can have this round trip under way while it still computes its query.
// `issue` is unconditional: the row index is clamped into [0, max(jend, 1) - 1] like every other load here, and for a group with
// j0 < jend the rows are exactly those the loop's first iteration reads (keys past jend fall back to row j0).  A group with
// j0 >= jend reads some mapped row whose content attend_keys never looks at.
template <typename E, int U, bool IDX = false>
struct FirstKeys {
  StreamRaw8<E> k[U], v[U];
  __device__ inline void issue(const E* kbase, const E* vbase, int j0, int jend, int jstride, const uint8_t* origin = nullptr,
                               long row_stride = 0) {
    const int c8 = (threadIdx.x & 7) * 8;
    const int last = (jend > 1 ? jend : 1) - 1;
    long row[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int jj = j0 + u * jstride;
      int jc = jj < jend ? jj : j0;
      jc = jc < last ? jc : last;
      row[u] = (long)jc * 64 + c8;
      if constexpr (IDX) row[u] += (long)origin[jc] * row_stride;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) k[u].load(kbase + row[u]);
#pragma unroll
    for (int u = 0; u < U; ++u) v[u].load(vbase + row[u]);
  }
};

// SC (the e4m3 self-attention cache): every key row carries its own fp32 scale pair, kscale_row[j] / vscale_row[j], fetched the
// way the bias is (one value per key per 8-lane group, clamped index, unconditional load); the key scale multiplies the score
// before bias and mask, the value scale multiplies the probability before the accumulate
// IDX (beam search over an index table, mh_t5_step_indexed): key / value row j of this head comes from cache row origin[j] -- kbase /
// vbase are then head h of cache row 0, `origin` the decode row's table entries in LDS and `row_stride` the elements between two
// cache rows (H * tgt_len * 64).  An 8-lane group still reads one whole row; only the row's base differs from key to key.
// SC with IDX (mh_t5_step_indexed_skv8): kscale_row / vscale_row are head h of shadow row 0 and key j's pair sits at
// origin[j] * (row_stride / 64) + j -- the scales of the row that holds the key, never those of the decode row.
// EARLY: `first` holds the requests of the first iteration (FirstKeys::issue with the same kbase / vbase / j0 / jend / jstride /
// origin / row_stride); the first iteration takes its rows from there -- if the group has one: the loop header is what discards the
// requests of a group with j0 >= jend -- and every later one loads as ever.  There is ONE loop body: every other load (bias, mask,
// scale pairs, table) and every product, sum, maximum and exponential is where it always was.
template <typename T, int U, typename E = T, bool SC = false, bool IDX = false, bool EARLY = false>
__device__ inline void attend_keys(Partial& st, const float (&q)[8], const E* kbase, const E* vbase, int j0,
                                   int jend, int jstride, const float* bias_row, int pos, const uint8_t* mask_row,
                                   int P, float scale, int jmin = 0,   // keys below jmin are masked (sliding window)
                                   const float* kscale_row = nullptr, const float* vscale_row = nullptr,
                                   const uint8_t* origin = nullptr, long row_stride = 0,
                                   const FirstKeys<E, U, IDX>* first = nullptr) {
  // processes keys j0, j0+jstride, ... < jend for this lane's key group, U at a time
  const int c8 = (threadIdx.x & 7) * 8;
  for (int j = j0; j < jend; j += jstride * U) {
    float s[U];
    float kv[U][8];
    float vv[U][8];
    int org_u[U];   // (IDX) the table value of key u: its scale pair below is addressed from the same LDS read as its K / V
    bool requested = false;   // (EARLY) the rows of this iteration are those of `first`
    if constexpr (EARLY) {
      requested = j == j0;
      if (requested) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if constexpr (IDX) {
            const int jj = j + u * jstride;
            org_u[u] = origin[jj < jend ? jj : j];
          }
          first->k[u].unpack(kv[u]);
          first->v[u].unpack(vv[u]);
        }
      }
    }
    if (requested) {   // (nothing to load; the branches below are the loads as they always were)
    } else if constexpr (IDX) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int jj = j + u * jstride;
        const int jc = jj < jend ? jj : j;
        org_u[u] = origin[jc];
        const long row = (long)org_u[u] * row_stride + (long)jc * 64 + c8;   // the cache row that holds key jc
        load8_stream<E>(kbase + row, kv[u]);
        load8_stream<E>(vbase + row, vv[u]);
      }
    } else {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int jj = j + u * jstride;
        const int jc = jj < jend ? jj : j;
        load8_stream<E>(kbase + (long)jc * 64 + c8, kv[u]);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int jj = j + u * jstride;
        const int jc = jj < jend ? jj : j;
        load8_stream<E>(vbase + (long)jc * 64 + c8, vv[u]);
      }
    }
    // bias / mask values: wave-uniform branch on the pointers, unconditional loads from clamped indices
    float bv[U];
    int mv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) { bv[u] = 0.f; mv[u] = 1; }
    float ksv[U], vsv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int jj = j + u * jstride;
      if constexpr (SC && IDX) {   // requested with the K / V loads above still in flight: no dependent round trip is added
        const long si = (long)org_u[u] * (row_stride >> 6) + (jj < jend ? jj : j);
        ksv[u] = kscale_row[si];
        vsv[u] = vscale_row[si];
      } else {
        ksv[u] = SC ? kscale_row[jj < jend ? jj : j] : 1.f;
        vsv[u] = SC ? vscale_row[jj < jend ? jj : j] : 1.f;
      }
    }
    if (bias_row) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int jj = j + u * jstride;
        bv[u] = bias_row[pos - (jj < jend ? jj : j)];
      }
    }
    if (mask_row) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int jj = j + u * jstride;
        const int jm = jj < P ? jj : P - 1;
        const int mval = mask_row[jm];
        mv[u] = (jj < P) ? mval : 1;
      }
    }
    float cmax = -INFINITY;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int jj = j + u * jstride;
      float d = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) d += q[i] * kv[u][i];
      // (DPP partners 4, 2, 1 stay inside the 8-lane group, and the loop's trip count depends on the group alone: whole groups run)
      if (SC) d = group_sum<8>(d) * ksv[u] * scale + bv[u];
      else d = group_sum<8>(d) * scale + bv[u];
      const bool ok = (jj < jend) && (jj >= jmin) && (mv[u] != 0);
      d = ok ? d : -INFINITY;
      s[u] = d;
      cmax = fmaxf(cmax, d);
    }
    const float mn = fmaxf(st.m, cmax);
    const float fa = fexp<T>(st.m - mn);
    st.l *= fa;
#pragma unroll
    for (int i = 0; i < 8; ++i) st.acc[i] *= fa;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const float pu = fexp<T>(s[u] - mn);
      st.l += pu;
      const float pv = SC ? pu * vsv[u] : pu;
#pragma unroll
      for (int i = 0; i < 8; ++i) st.acc[i] += pv * vv[u][i];
    }
    st.m = mn;
  }
}

// ---- e4m3 shadow of the self-attention cache (mh_t5_generate_skv8) ---------------------------------------------------------
// One cached key / value row (64 elements of one layer, row, head, position) = 64 OCP e4m3 bytes + one fp32 scale:
// scale = absmax / 448 (1 for an all-zero row), element = cvt_e4m3(x * (1 / scale)) -- the reciprocal-multiply form of
// kv_quant_fp8_kernel (decode_sample.hip).  quant_row64 is the ONE statement of it: the token step's append and the bulk pass after the prompt
// prefill both call it, so the two cannot round differently.  A whole wave: lane i holds element i; lanes 0..15 store four bytes each
// and lane 0 the scale, with ordinary vector stores (the next launch reads them).
__device__ inline void quant_row64(float x, uint8_t* q_row, float* scale_slot) {
  const int lane = threadIdx.x & 63;
  const float mx = wave_max(fabsf(x));
  const float scale = mx > 0.f ? mx / 448.0f : 1.0f;   // 448 = largest finite e4m3 value
  const float inv = 1.0f / scale;
  const float y = x * inv;
  const int src = (lane & 15) * 4;
  const float y0 = __shfl(y, src, 64), y1 = __shfl(y, src + 1, 64), y2 = __shfl(y, src + 2, 64), y3 = __shfl(y, src + 3, 64);
  int o = __builtin_amdgcn_cvt_pk_fp8_f32(y0, y1, 0, false);
  o = __builtin_amdgcn_cvt_pk_fp8_f32(y2, y3, o, true);
  if (lane < 16) reinterpret_cast<uint32_t*>(q_row)[lane] = (uint32_t)o;
  if (lane == 0) *scale_slot = scale;
}

// merge the NW waves' partial (m, l, acc[64]) through LDS; threads 0..63 return the merged (m, l, a[d])
template <typename T, int NW = 4>
__device__ inline void block_merge(const Partial& st, float (*sm)[66], float& m, float& l, float& a) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int c8 = (lane & 7) * 8, g = lane >> 3;
  if (g == 0) {
    if (lane == 0) { sm[wid][0] = st.m; sm[wid][1] = st.l; }
#pragma unroll
    for (int i = 0; i < 8; ++i) sm[wid][2 + c8 + i] = st.acc[i];
  }
  __syncthreads();
  m = -1e30f; l = 0.f; a = 0.f;
  if (threadIdx.x < 64) {
    // two passes over the NW partials: the block-wide maximum, then NW INDEPENDENT exponentials (a running merge chains
    // 2 (NW - 1) dependent ones: ~0.7 us at NW = 16); wave order fixed => deterministic
    const int d = threadIdx.x;
    m = sm[0][0];
#pragma unroll
    for (int w = 1; w < NW; ++w) m = fmaxf(m, sm[w][0]);
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      const float f = fexp<T>(sm[w][0] - m);
      l += sm[w][1] * f;
      a += sm[w][2 + d] * f;
    }
  }
}

// ---- attention kernels that project their own query (and the new self-attention key / value) --------------------
// A decode step is ~100 dependent kernels of a few microseconds each, so every kernel removed from the chain is worth
// more than the work it did.  The per-head projections are tiny (64 outputs x d inputs): each attention workgroup
// recomputes RMSNorm(h[b]) and its own 64-row slice of W (the slices of one head are shared by the B workgroups of
// that head through L2), which removes the stand-alone QKV and cross-Q GEMV launches from every layer.
template <typename T> struct Raw8;
template <> struct Raw8<bf16_t> {
  uint4 v;
  __device__ inline void load(const bf16_t* p) { v = *reinterpret_cast<const uint4*>(p); }
  __device__ inline void unpack(float (&o)[8]) const {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) { o[2 * i] = __uint_as_float(w[i] << 16); o[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u); }
  }
};
template <> struct Raw8<float> {
  float4 a, b;
  __device__ inline void load(const float* p) { a = *reinterpret_cast<const float4*>(p); b = *reinterpret_cast<const float4*>(p + 4); }
  __device__ inline void unpack(float (&o)[8]) const {
    o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
  }
};

// xn[k] = T-rounded ln_w[k] * (h[b][k] * rsqrt(mean(h[b]^2) + eps)) for k < d, by a 1024-thread workgroup (d <= 1024).
// The statistics come from the row itself (wave sums -> 16 LDS floats that every thread adds in the same order).
// Two halves: `issue` only REQUESTS the row and the weight (it needs nothing but preloaded kernel arguments), `finish`
// waits for them -- whatever else the kernel can request goes in between.
template <typename T, bool LN = false>
struct NormRow {
  float x, g, bb;
  __device__ inline void issue_weight(const HeadProjP& hp) {      // (independent of the predecessor)
    const int tid = threadIdx.x;
    g = hp.ln_w[tid < hp.d ? tid : hp.d - 1];
    if (LN) bb = hp.ln_b[tid < hp.d ? tid : hp.d - 1];
  }
  __device__ inline void issue_row(const HeadProjP& hp, int b) {   // the residual row the predecessor wrote
    const int tid = threadIdx.x;
    x = hp.h[(long)b * hp.ldh + (tid < hp.d ? tid : hp.d - 1)];
  }
  __device__ inline void issue(const HeadProjP& hp, int b) { issue_row(hp, b); issue_weight(hp); }
  __device__ inline void finish(const HeadProjP& hp, float* xn, float* red16) {
    const int tid = threadIdx.x;
    if (LN) {
      // nn.LayerNorm: mean first, then the centred sum of squares (two block reductions over the same 16 LDS floats)
      const float su = wave_sum(tid < hp.d ? x : 0.f);
      if ((tid & 63) == 0) red16[tid >> 6] = su;
      __syncthreads();
      float tot = 0.f;
#pragma unroll
      for (int w = 0; w < 16; ++w) tot += red16[w];
      x -= tot / (float)hp.d;
      __syncthreads();      // (every thread has read red16 before it is written again)
    }
    const float sq = wave_sum(tid < hp.d ? x * x : 0.f);
    if ((tid & 63) == 0) red16[tid >> 6] = sq;
    __syncthreads();
    float tot = 0.f;
#pragma unroll
    for (int w = 0; w < 16; ++w) tot += red16[w];
    const float rs = rsqrtf(tot / (float)hp.d + hp.eps);
    if (tid < hp.d) xn[tid] = Elem<T>::to_f32(Elem<T>::from_f32(LN ? x * rs * g + bb : g * (x * rs)));
    __syncthreads();
  }
};

// NP projections of 64 outputs each: out[p][o] = T-rounded sum_k xn[k] * W[(row0[p] + o) * ldw + k].
// 1024 threads: 16 consecutive lanes per output, KC 8-element chunks per lane (d = 128 KC), chunk c of lane ks = elements
// [128 c + 8 ks, + 8): the 16 lanes of an output read 256 (bf16) / 512 (fp32) CONTIGUOUS bytes per load instruction, whole
// 128-byte lines (lane-contiguous chunks -- 96-byte strides at d = 768 -- touch 12 lines per output row and instruction;
// the CU's load path is charged per line and lane).  The weight slice does not depend on the activations: `load` is
// called at kernel entry, `apply` after the normalised row is in LDS.
// FENCE: nothing is scheduled across the end of a projection (the shuffle reductions' LDS waits used to keep the projections apart;
// without them hipcc overlaps them and the Whisper-family self-attention instantiations, at the 128-register limit, spill)
template <typename T, int KC, int NP, bool FENCE = false>
struct HeadProj {
  Raw8<T> raw[NP][KC];
  __device__ inline void load(const HeadProjP& hp, const int (&row0)[NP]) {
    const int tid = threadIdx.x, o = tid >> 4, ks = tid & 15;
#pragma unroll
    for (int q = 0; q < NP; ++q) {
      const T* wp = reinterpret_cast<const T*>(hp.W) + (long)(row0[q] + o) * hp.ldw + ks * 8;
#pragma unroll
      for (int c = 0; c < KC; ++c) raw[q][c].load(wp + c * 128);
    }
    MH_LOADS_ISSUED();
  }
  __device__ inline void load3(const HeadProjP& hp, const int (&row0)[3]) {   // (NP == 3 instantiations only)
    const int tid = threadIdx.x, o = tid >> 4, ks = tid & 15;
#pragma unroll
    for (int q = 0; q < (NP < 3 ? NP : 3); ++q) {
      const T* wp = reinterpret_cast<const T*>(hp.W) + (long)(row0[q] + o) * hp.ldw + ks * 8;
#pragma unroll
      for (int c = 0; c < KC; ++c) raw[q][c].load(wp + c * 128);
    }
  }
  // bias (fp32, indexed like the weight rows) or NULL: out = T-rounded (acc + bias[row0 + o]) -- nn.Linear with bias
  __device__ inline void apply(const float* xn, float (*out)[64], const float* bias = nullptr, const int* row0 = nullptr) const {
    const int tid = threadIdx.x, o = tid >> 4, ks = tid & 15;
#pragma unroll
    for (int q = 0; q < NP; ++q) {
      float acc = 0.f;
#pragma unroll
      for (int c = 0; c < KC; ++c) {
        float w[8];
        raw[q][c].unpack(w);
        const float4 x0 = *reinterpret_cast<const float4*>(xn + c * 128 + ks * 8);
        const float4 x1 = *reinterpret_cast<const float4*>(xn + c * 128 + ks * 8 + 4);
        acc += x0.x * w[0] + x0.y * w[1] + x0.z * w[2] + x0.w * w[3] + x1.x * w[4] + x1.y * w[5] + x1.z * w[6] + x1.w * w[7];
      }
      acc = group_sum<16>(acc);
      if (bias) acc += bias[row0[q] + o];
      if (ks == 0) out[q][o] = Elem<T>::to_f32(Elem<T>::from_f32(acc));
      if constexpr (FENCE) __builtin_amdgcn_sched_barrier(0);
    }
  }
};

}  // namespace dec
}  // namespace mh
