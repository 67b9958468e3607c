// Device kernels of the KV-cached autoregressive T5 decode step (K5 / K6).
//
// One token step of one layer is SIX dependent kernels per row chain (a chain = up to 16 rows; two chains run side by
// side): [RMSNorm + this head's q / k / v projection + self-KV append + self-attention over the cache] -> [O GEMV +
// residual] -> [RMSNorm + this head's query projection + cross-attention over the 1251 encoder keys: THE HBM-bound
// kernel, B*H*L*64*2 elements per layer per step] -> [O GEMV + residual] -> [RMSNorm + wi GEMV + gated GELU] -> [wo GEMV
// + residual]; then final RMSNorm + lm_head GEMV and the sampler (t5.hip).  Every kernel reads the current position
// from device memory, so a chain's step is one replayable hipGraph.  Under option decode_fused_tail the last THREE of the six
// are one launch (dec_tail_kernel below: the same GEMV code per phase, two bounded in-kernel hand-offs): four nodes per layer.
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
#pragma once
#include <type_traits>

#include "decode_step.hpp"   // kSelfIdxMaxTgt, which the host entries check too
#include "internal.hpp"

namespace mh {
namespace dec {

// ---- phase stamps (profiling build only: `make prof` defines MH_PHASE_STAMPS) --------------------------------------------
// Thread 0 of workgroup 0 adds (shader-clock ticks since its first instruction) to g_stamps[kernel][stamp] at marked
// points; tools/decode_phases.py prints the averages.  The production library contains none of this.
#ifdef MH_PHASE_STAMPS
__device__ unsigned long long g_stamps[16 * 16 * 2];   // [kernel id][stamp][sum of ticks, count]
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

// ---- decode GEMV ("skinny GEMM": M = batch rows <= 64) ------------------------------------------------------------
// out[b][n] = sum_k A[b][k] * W[n][k] on the 16x16 MFMA atoms.  One workgroup owns ONE 16-column tile of which `nv`
// columns are real (nv = 16, 8 or 4: a 768-column projection becomes 48, 96 or 192 workgroups; the other tile columns
// repeat real ones and are never stored), its NWV waves split K (wave w takes k-blocks w, w + NWV, ...), the partial
// accumulators are added through LDS in wave order (deterministic, independent of the batch).
//   * straight-line code: every load of a pass is issued before the first wait, addresses are clamped instead of
//     predicated, k-blocks beyond K are neutralised by AND-ing the activation fragment with 0 (no branches: a predicated
//     load or a branch around an MFMA made hipcc serialise the loads of the previous version into several round trips);
//   * PRO_RMSNORM: A is the fp32 residual stream; the workgroup holds all of its <= 64 rows x K values in registers at
//     once (single pass), so the RMSNorm statistics come from those registers (lane -> 16-lane shuffle -> LDS over the
//     waves): no statistics buffers, no extra memory round trip, one barrier;
//   * weights are read exactly once per workgroup straight into MFMA fragments (no LDS round trip for data used once).
//   * the activation fragments are "fragment-shaped" loads (16 rows x 64 bytes per wave instruction), which cost the
//     CU's load path about twice what whole lines cost (tools/micro/gemv_probe, mask 128: the same bytes as contiguous
//     1 KB runs take 3.35 -> 2.70 us alone, 4.13 -> 2.92 us beside a second chain).  Staging them through LDS with
//     whole-line loads was built and measured: the extra LDS write / barrier / read costs what the loads save (o-projection
//     3.61 us alone, 4.12 beside a second chain; whole step 37.4 k vs 38.1 k tok/s without it) -- not kept.
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

template <typename T> struct VecOps;
template <> struct VecOps<bf16_t> {
  struct Raw { float4 a, b; };   // 8 consecutive fp32 values (one lane's k-chunk)
  __device__ static inline Raw load_raw(const float* p) {
    Raw r;
    r.a = *reinterpret_cast<const float4*>(p);
    r.b = *reinterpret_cast<const float4*>(p + 4);
    return r;
  }
  // the same 8 values out of a wave-private LDS patch that was written as u32x4_t pieces: read back with the type it was
  // written with (a float4 read of it is a differently-typed access the compiler may move above the write)
  __device__ static inline Raw from_patch(const unsigned char* p) {
    const u32x4_t a = *reinterpret_cast<const u32x4_t*>(p), b = *reinterpret_cast<const u32x4_t*>(p + 16);
    Raw r;
    r.a = make_float4(__uint_as_float(a[0]), __uint_as_float(a[1]), __uint_as_float(a[2]), __uint_as_float(a[3]));
    r.b = make_float4(__uint_as_float(b[0]), __uint_as_float(b[1]), __uint_as_float(b[2]), __uint_as_float(b[3]));
    return r;
  }
  __device__ static inline float sumsq(const Raw& x) {
    return (x.a.x * x.a.x + x.a.y * x.a.y) + (x.a.z * x.a.z + x.a.w * x.a.w) + (x.b.x * x.b.x + x.b.y * x.b.y) +
           (x.b.z * x.b.z + x.b.w * x.b.w);
  }
  __device__ static inline float sum(const Raw& x) { return (x.a.x + x.a.y) + (x.a.z + x.a.w) + (x.b.x + x.b.y) + (x.b.z + x.b.w); }
  __device__ static inline Raw centred(const Raw& x, float mu) {
    Raw r;
    r.a = make_float4(x.a.x - mu, x.a.y - mu, x.a.z - mu, x.a.w - mu);
    r.b = make_float4(x.b.x - mu, x.b.y - mu, x.b.z - mu, x.b.w - mu);
    return r;
  }
  // nn.LayerNorm: (x - mean) * rstd * weight + bias (x arrives centred)
  __device__ static inline uint4 ln_frag(const Raw& x, const Raw& g, const Raw& b, float rs) {
    const uint32_t o0 = pack_bf16x2(x.a.x * rs * g.a.x + b.a.x, x.a.y * rs * g.a.y + b.a.y);
    const uint32_t o1 = pack_bf16x2(x.a.z * rs * g.a.z + b.a.z, x.a.w * rs * g.a.w + b.a.w);
    const uint32_t o2 = pack_bf16x2(x.b.x * rs * g.b.x + b.b.x, x.b.y * rs * g.b.y + b.b.y);
    const uint32_t o3 = pack_bf16x2(x.b.z * rs * g.b.z + b.b.z, x.b.w * rs * g.b.w + b.b.w);
    return make_uint4(o0, o1, o2, o3);
  }
  __device__ static inline uint4 norm_frag(const Raw& x, const Raw& g, float rs) {
    const uint32_t o0 = pack_bf16x2(g.a.x * (x.a.x * rs), g.a.y * (x.a.y * rs));
    const uint32_t o1 = pack_bf16x2(g.a.z * (x.a.z * rs), g.a.w * (x.a.w * rs));
    const uint32_t o2 = pack_bf16x2(g.b.x * (x.b.x * rs), g.b.y * (x.b.y * rs));
    const uint32_t o3 = pack_bf16x2(g.b.z * (x.b.z * rs), g.b.w * (x.b.w * rs));
    return make_uint4(o0, o1, o2, o3);
  }
  __device__ static inline f32x4_t mma(const uint4& a, const uint4& b, f32x4_t c) {
    union U { uint4 u; bf16x8_t f; };
    U ua, ub;
    ua.u = a; ub.u = b;
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(ua.f, ub.f, c, 0, 0, 0);
  }
};
template <> struct VecOps<float> {
  struct Raw { float4 a; };
  __device__ static inline Raw load_raw(const float* p) {
    Raw r;
    r.a = *reinterpret_cast<const float4*>(p);
    return r;
  }
  __device__ static inline Raw from_patch(const unsigned char* p) {   // (never reached: RLINES is bf16 storage only)
    const u32x4_t a = *reinterpret_cast<const u32x4_t*>(p);
    Raw r;
    r.a = make_float4(__uint_as_float(a[0]), __uint_as_float(a[1]), __uint_as_float(a[2]), __uint_as_float(a[3]));
    return r;
  }
  __device__ static inline float sumsq(const Raw& x) { return (x.a.x * x.a.x + x.a.y * x.a.y) + (x.a.z * x.a.z + x.a.w * x.a.w); }
  __device__ static inline float sum(const Raw& x) { return (x.a.x + x.a.y) + (x.a.z + x.a.w); }
  __device__ static inline Raw centred(const Raw& x, float mu) {
    Raw r;
    r.a = make_float4(x.a.x - mu, x.a.y - mu, x.a.z - mu, x.a.w - mu);
    return r;
  }
  __device__ static inline uint4 ln_frag(const Raw& x, const Raw& g, const Raw& b, float rs) {
    return make_uint4(__float_as_uint(x.a.x * rs * g.a.x + b.a.x), __float_as_uint(x.a.y * rs * g.a.y + b.a.y),
                      __float_as_uint(x.a.z * rs * g.a.z + b.a.z), __float_as_uint(x.a.w * rs * g.a.w + b.a.w));
  }
  __device__ static inline uint4 norm_frag(const Raw& x, const Raw& g, float rs) {
    return make_uint4(__float_as_uint(g.a.x * (x.a.x * rs)), __float_as_uint(g.a.y * (x.a.y * rs)),
                      __float_as_uint(g.a.z * (x.a.z * rs)), __float_as_uint(g.a.w * (x.a.w * rs)));
  }
  __device__ static inline f32x4_t mma(const uint4& a, const uint4& b, f32x4_t c) {
    // k permutation: element i of every lane's 4-float vector forms one 16x16x4 product
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.x), __uint_as_float(b.x), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.y), __uint_as_float(b.y), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.z), __uint_as_float(b.z), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.w), __uint_as_float(b.w), c, 0, 0, 0);
    return c;
  }
};

constexpr int kGemvCH = 8;   // k-blocks per wave whose loads are in flight at once (one pass)

// tools/micro/gemv_probe.hip compiles this kernel with parts switched OFF to price them (bit mask: 1 activation loads,
// 2 weight loads, 4 old residual values, 8 cross-wave reduction, 16 stores; 32 / 64: residual stores as agent-scope atomic /
// non-temporal stores); always 0 in the library
#ifndef MH_GEMV_PROBE
#define MH_GEMV_PROBE 0
#endif

// MF 16-row fragments (B <= 16 MF), NWV waves.  NWV depends on K only (never on the batch): a row's summation order,
// hence its rounding and its greedy tokens, must not depend on which other rows share the launch.  The k-block -> wave
// assignment is likewise a function of the prologue only: PRO_PLAIN gives wave w the k-block PAIRS w, w + NWV, ... (two
// consecutive k-blocks = one 128-byte line of a bf16 row) for every MF -- the whole-line path (MF == 1) and the
// fragment-shaped path (MF >= 2: a chain of more than 16 rows, e.g. a guidance batch) add the same products in the same
// order; PRO_RMSNORM gives wave w the single k-blocks w, w + NWV, ...
// Kernel arguments: the operands a workgroup needs to issue its first loads are LEADING SCALAR arguments -- the library is
// built with -amdgpu-kernarg-preload-count=14, so they arrive in SGPRs with the wave launch instead of through an s_load
// from the (cold) kernarg segment: one memory round trip off every dependent kernel (tools/micro/kernarg_preload.hip: a
// GEMV-like dependent kernel 2.49 -> 1.91 us alone, 3.58 -> 2.90 us beside a kernel that streams HBM).  The struct keeps
// the rest; its copies of the leading arguments are never read (lda = ldw = K: checked on the host).
// (12 dwords: the 13th and 14th preload slots do not arrive on this firmware -- the kernel body re-loads them)
#define MH_GEMV_LEAD_PARAMS const void *A_, const void *W_, float *h_, const float *lnw_, int K_, int B_, int N_, int nv_
#define MH_GEMV_LEAD_ARGS(p) (p).A, (p).W, (p).h, (p).ln_w, (p).K, (p).B, (p).N, (p).nv
// LDS of one K-split group (NWV waves): the stand-alone kernel has one, a 512-thread dec_tail_kernel runs its 4-wave phases as
// two groups with one each.  (The staged norm weight / bias are not in here: the groups of a workgroup share them.)
template <typename T, int MF, int NWV, int PRO>
struct GemvLds {
  static constexpr bool NORM = PRO != PRO_PLAIN, LN = PRO == PRO_LAYERNORM;
  static constexpr bool LINES = (MF == 1 && PRO == PRO_PLAIN), RLINES = (MF == 1 && NORM && sizeof(T) == 2);
  static constexpr int PATCH = 16 * 144;            // 16 rows x (128 + 16) bytes: rows 16 bytes apart in the bank row
  __attribute__((aligned(16))) unsigned char Lw[(LINES || RLINES) ? NWV * PATCH : 16];
  f32x4_t red[NWV * MF * 64];
  float ssw[NORM ? NWV : 1][MF * 16];
  float ssw2[LN ? NWV : 1][MF * 16];    // LayerNorm: the centred sums of squares (second reduction)
};

// weight row of tile column l15 of tile `tile` (clamped), and whether this lane fetches it
template <int EPI>
__device__ __forceinline__ void gemv_wrow(const SkinnyP& p, int tile, int l15, int& wrow, int& ocol, bool& wload) {
  if (EPI == SK_GEGLU) {
    // tile t = ff columns [8t, 8t + 8): tile columns 0..7 are their gate rows, 8..15 their linear rows; wi_0 / wi_1 are
    // interleaved in 16-row blocks [gate | linear] (PackedT5.interleave16)
    ocol = tile * 8 + (l15 & 7);
    const int oc = ocol < p.N / 2 ? ocol : p.N / 2 - 1;
    wrow = (oc >> 4) * 32 + (l15 >> 3) * 16 + (oc & 15);
    wload = true;
  } else {
    ocol = tile * p.nv + l15;
    wrow = ocol < p.N ? ocol : p.N - 1;
    wload = l15 < p.nv;
  }
}

// The weight fragments of the FIRST pass of gemv_tile(p, tile, tid, ...), requested ahead of it (dec_tail_kernel: before
// the wait for the previous phase -- they depend on nothing that phase writes).  The same addresses, clamps and exec mask
// as the loads inside gemv_tile.
struct WFrag { uint4 v[kGemvCH]; };   // one pass's weight fragments of a lane (passed by value: they live in registers)
template <typename T, int MF, int NWV, int PRO, int EPI>
__device__ __forceinline__ WFrag gemv_issue_w(const SkinnyP& p, int tile, int tid) {
  WFrag wf;
  constexpr int VEC = Elem<T>::kVec, KB = 4 * VEC, CH = kGemvCH;
  constexpr bool LINES = (MF == 1 && PRO == PRO_PLAIN);
  const int lane = tid & 63, wid = tid >> 6, l15 = lane & 15, lg = lane >> 4;
  int wrow, ocol; bool wload;
  gemv_wrow<EPI>(p, tile, l15, wrow, ocol, wload);
  const T* Wp = reinterpret_cast<const T*>(p.W) + (long)wrow * p.ldw + lg * VEC;
  const int nkb = p.K / KB, npair = nkb >> 1;
#pragma unroll
  for (int c = 0; c < CH; ++c) wf.v[c] = make_uint4(0, 0, 0, 0);
  if (wload) {
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      int kb;
      if (LINES) { const int pw = wid + NWV * (c >> 1); kb = 2 * (pw < npair ? pw : npair - 1) + (c & 1); }
      else { kb = PRO == PRO_PLAIN ? 2 * (wid + NWV * (c >> 1)) + (c & 1) : wid + NWV * c; kb = kb < nkb ? kb : nkb - 1; }
      wf.v[c] = *reinterpret_cast<const uint4*>(Wp + kb * KB);
    }
  }
  return wf;
}

// One 16-column tile of the GEMV by one group of NWV waves: `tile` = tile index (a tile past the last one loads from
// clamped addresses and stores nothing), `tid` = thread index within the group, L = the group's LDS, lnw / lnb = the
// workgroup's staged norm weight / bias.  PRE: the first pass takes its weight fragments from `wpre` (gemv_issue_w)
// instead of loading them.  Every __syncthreads() in here is reached by the whole workgroup: the groups of a workgroup run
// this function in lockstep.  KID < 0: no phase stamps.
template <typename T, int MF, int NWV, int PRO, int EPI, bool BIAS, int KID, bool PRE>
__device__ __forceinline__ void gemv_tile(const SkinnyP& p, const int tile, const int tid, GemvLds<T, MF, NWV, PRO>& L,
                                          float* lnw, float* lnb, const WFrag wpre MH_T0_PARAM) {
  constexpr int VEC = Elem<T>::kVec;   // elements per 16-byte vector (per lane per k-block)
  constexpr int KB = 4 * VEC;          // k elements per k-block (4 lane groups x 16 B)
  constexpr int CH = kGemvCH;
  typedef typename VecOps<T>::Raw Raw;
  // PRO_PLAIN, 16 rows (MF == 1): the activations are loaded as whole 128-byte lines -- 8 rows x 128 bytes per wave
  // instruction; wave w owns the k-block PAIRS w, w + NWV, ... -- and turned into MFMA fragments through a wave-private
  // 2.3 KB LDS patch: no barrier (the LDS operations of one wave execute in order, so the patch is reused line after
  // line), 2 ds_write_b128 + 2 ds_read_b128 per line.  Fragment-shaped global loads (16 rows x 64 bytes per instruction)
  // cost the CU's load path twice as much: tools/micro/gemv_probe, o-projection 3.35 -> 2.80 us alone, 4.13 -> 3.09 us
  // beside a second chain; K = 2048: 4.89 -> 3.66 / 5.54 -> 4.63; whole step 38.2 k -> 39.9 k tok/s.
  // PRO_RMSNORM under bf16 storage (RLINES): the fp32 residual rows are one line per row and k-block; the same patch
  // trick with the k-block -> wave assignment unchanged: RMSNorm + wi + gated GELU 5.80 -> 4.33 us alone, 6.80 -> 5.20 us
  // beside a second chain.  Loading the 16-row WEIGHT tile of that GEMV as lines as well was measured and lost (6.90 /
  // 8.69 us: 16 more LDS operations per wave than the load path saves) -- weights keep fragment-shaped loads.
  constexpr bool LINES = (MF == 1 && PRO == PRO_PLAIN);
  constexpr int CP = CH / 2;                 // k-block pairs per wave and pass
  constexpr int PATCH = GemvLds<T, MF, NWV, PRO>::PATCH;
  constexpr bool NORM = PRO != PRO_PLAIN, LN = PRO == PRO_LAYERNORM;
  constexpr bool RLINES = (MF == 1 && NORM && sizeof(T) == 2);
  unsigned char* const Lw = L.Lw;
  f32x4_t* const red = L.red;
  float (*const ssw)[MF * 16] = L.ssw;
  float (*const ssw2)[MF * 16] = L.ssw2;

  const int lane = tid & 63, wid = tid >> 6;
  const int l15 = lane & 15, lg = lane >> 4;
  const int nv = p.nv;
  // The vector-memory path of a CU moves 64 B per clock and charges every LANE of a load instruction, duplicates
  // included: a tile whose 16 columns repeat nv real ones must not load the repeats (exec-masked W loads below), and
  // the RMSNorm weight is fetched once per workgroup through LDS instead of once per 16-lane row group.
  float4 lnraw = make_float4(0.f, 0.f, 0.f, 0.f), lnbraw = make_float4(0.f, 0.f, 0.f, 0.f);
  if (NORM) {
    const int i4 = tid * 4 < p.K ? tid * 4 : 0;     // K <= 1024 <= 4 * (NWV * 64)
    lnraw = *reinterpret_cast<const float4*>(p.ln_w + i4);
    if (LN) lnbraw = *reinterpret_cast<const float4*>(p.ln_b + i4);
  }
  // weight row of this lane's tile column
  int wrow, ocol;      // ocol: output column of tile column l15 (GEGLU: of the gate / linear PAIR)
  bool wload;          // this lane fetches a weight fragment (tile columns >= nv are never stored: they keep zeros)
  gemv_wrow<EPI>(p, tile, l15, wrow, ocol, wload);
  const T* Wp = reinterpret_cast<const T*>(p.W) + (long)wrow * p.ldw + lg * VEC;
  int arow[MF];
#pragma unroll
  for (int f = 0; f < MF; ++f) arow[f] = (f * 16 + l15) < p.B ? (f * 16 + l15) : p.B - 1;

  constexpr int UPW = (MF * 4 + NWV - 1) / NWV;
  const bool col_ok = (EPI == SK_GEGLU) ? (l15 < 8 && ocol < p.N / 2) : (l15 < nv && ocol < p.N);
  float oldh[UPW];
#pragma unroll
  for (int u = 0; u < UPW; ++u) oldh[u] = 0.f;
  constexpr int PROBE = MH_GEMV_PROBE;
  float bias_v = 0.f;
  if (BIAS) bias_v = p.bias[ocol < p.N ? ocol : p.N - 1];
  // (a macro, not a lambda: a by-reference capture of `oldh` made hipcc keep the array in memory and promote it to LDS --
  // 4 KB per wave, an LDS round trip per value: the residual GEMVs went from 5.4 to 17 us)
#define MH_LOAD_OLDH()                                                                                                        \
  do {                                                                                                                        \
    _Pragma("unroll") for (int u = 0; u < UPW; ++u) {                                                                         \
      const int unit = wid + u * NWV;                                                                                         \
      const int row = (unit >> 2) * 16 + lg * 4 + (unit & 3);                                                                 \
      if (unit < MF * 4) oldh[u] = p.h[(long)(row < p.B ? row : p.B - 1) * p.ldh + (ocol < p.N ? ocol : p.N - 1)];          \
    }                                                                                                                         \
  } while (0)
  if (EPI == SK_RESID && l15 < nv && !(PROBE & 4)) MH_LOAD_OLDH();   // requested before anything is waited for
  f32x4_t acc[MF];
#pragma unroll
  for (int f = 0; f < MF; ++f) acc[f] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  const int nkb = p.K / KB;

  // k-block of slot c of a pass that starts at kb0 (PRO_PLAIN: kb0 counts k-block PAIRS, see the header comment)
  auto kblock = [](int kb0, int c) -> int { return PRO == PRO_PLAIN ? 2 * (kb0 + NWV * (c >> 1)) + (c & 1) : kb0 + NWV * c; };
  int kb0 = wid;
  if constexpr (LINES) {
    const int npair = nkb >> 1;        // K is a multiple of 2 KB elements (checked on the host)
    unsigned char* patch = Lw + wid * PATCH;
    const int r8 = lane >> 3, c16 = (lane & 7) * 16;
    const unsigned char* Ab = reinterpret_cast<const unsigned char*>(p.A) + c16;
    const long rx = (long)(r8 < p.B ? r8 : p.B - 1) * p.lda * (long)sizeof(T);
    const long ry = (long)(8 + r8 < p.B ? 8 + r8 : p.B - 1) * p.lda * (long)sizeof(T);
    for (int pw0 = wid; pw0 < npair + wid; pw0 += NWV * CP) {
      uint4 wv[CH];
      u32x4_t xa[CP], ya[CP];   // (native vectors: as HIP uint4 structs these copies became memcpys that kept the arrays in scratch)
#pragma unroll
      for (int c = 0; c < CH; ++c) wv[c] = make_uint4(0, 0, 0, 0);
      if (PRE && pw0 == wid) {       // requested by the caller (gemv_issue_w)
#pragma unroll
        for (int c = 0; c < CH; ++c) wv[c] = wpre.v[c];
      } else if (wload && !(PROBE & 2)) {   // ONE exec-masked region around all weight loads
#pragma unroll
        for (int c = 0; c < CH; ++c) {
          const int pw = pw0 + NWV * (c >> 1);
          wv[c] = *reinterpret_cast<const uint4*>(Wp + (2 * (pw < npair ? pw : npair - 1) + (c & 1)) * KB);   // clamped address
        }
      }
#pragma unroll
      for (int cp = 0; cp < CP; ++cp) {
        const int pw = pw0 + NWV * cp;
        const long off = (long)(pw < npair ? pw : npair - 1) * 128;
        xa[cp] = *reinterpret_cast<const u32x4_t*>(Ab + rx + off);
        ya[cp] = *reinterpret_cast<const u32x4_t*>(Ab + ry + off);
      }
      MH_LOADS_ISSUED();
      MH_LOADS_ISSUED();
    if constexpr (KID >= 0) MH_STAMP(KID, 0);   // loads issued
#pragma unroll
      for (int cp = 0; cp < CP; ++cp) {
        const uint32_t keep = (pw0 + NWV * cp < npair) ? 0xffffffffu : 0u;   // pairs beyond K contribute zeros
        *reinterpret_cast<u32x4_t*>(patch + r8 * 144 + c16) = xa[cp];
        *reinterpret_cast<u32x4_t*>(patch + (8 + r8) * 144 + c16) = ya[cp];
#pragma unroll
        for (int j = 0; j < 2; ++j) {   // this lane's fragment (row l15, k group lg) of the pair's two k-blocks
          const u32x4_t pa = *reinterpret_cast<const u32x4_t*>(patch + l15 * 144 + (j * 4 + lg) * 16);   // the type the patch was written with
          uint4 a = make_uint4(pa[0], pa[1], pa[2], pa[3]);
          a = make_uint4(a.x & keep, a.y & keep, a.z & keep, a.w & keep);
          acc[0] = VecOps<T>::mma(a, wv[cp * 2 + j], acc[0]);
        }
      }
    }
  } else
  do {   // ONE pass for every RMSNorm shape and for K <= NWV * CH * KB; every wave runs at least one (its barrier)
    uint4 wv[CH];
    uint4 av[PRO == PRO_PLAIN ? CH : 1][PRO == PRO_PLAIN ? MF : 1];
    Raw hraw[NORM ? CH : 1][NORM ? MF : 1];
#pragma unroll
    for (int c = 0; c < CH; ++c) wv[c] = make_uint4(0, 0, 0, 0);
    if (PRE && kb0 == wid) {         // requested by the caller (gemv_issue_w)
#pragma unroll
      for (int c = 0; c < CH; ++c) wv[c] = wpre.v[c];
    } else if (wload && !(PROBE & 2)) {     // ONE exec-masked region around all weight loads (a branch per load would serialise them)
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        const int kb = kblock(kb0, c);
        wv[c] = *reinterpret_cast<const uint4*>(Wp + (kb < nkb ? kb : nkb - 1) * KB);   // clamped address
      }
    }
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int kb = kblock(kb0, c);
      const int kel = (kb < nkb ? kb : nkb - 1) * KB;
      if (PROBE & 1) {
#pragma unroll
        for (int f = 0; f < MF; ++f) {
          if (PRO == PRO_PLAIN) av[c][f] = make_uint4(kel, lane, c, f);
          else hraw[c][f] = VecOps<T>::load_raw(lnw + ((kel + lane) & 1020));
        }
      } else if (PRO == PRO_PLAIN && (PROBE & 128)) {   // timing only: the same bytes as whole 1 KB runs per wave instruction
#pragma unroll
        for (int f = 0; f < MF; ++f)
          av[c][f] = *reinterpret_cast<const uint4*>(reinterpret_cast<const T*>(p.A) + ((long)((c * NWV + wid) % (p.K * 16 / (64 * VEC))) * 64 + lane) * VEC);
      } else if (PRO == PRO_PLAIN) {
#pragma unroll
        for (int f = 0; f < MF; ++f)
          av[c][f] = *reinterpret_cast<const uint4*>(reinterpret_cast<const T*>(p.A) + (long)arow[f] * p.lda + kel + lg * VEC);
      } else if (!RLINES) {
#pragma unroll
        for (int f = 0; f < MF; ++f)
          hraw[c][f] = VecOps<T>::load_raw(reinterpret_cast<const float*>(p.A) + (long)arow[f] * p.lda + kel + lg * VEC);
      }
    }
    u32x4_t xr[RLINES ? CH : 1], yr[RLINES ? CH : 1];
    if (RLINES) {   // one 128-byte line of fp32 per row and k-block: rows 0..7 / 8..15 of the block as two whole-line loads
      const int r8 = lane >> 3;
      const unsigned char* Ab = reinterpret_cast<const unsigned char*>(p.A) + (lane & 7) * 16;
      const long rx = (long)(r8 < p.B ? r8 : p.B - 1) * p.lda * 4, ry = (long)(8 + r8 < p.B ? 8 + r8 : p.B - 1) * p.lda * 4;
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        const int kb = kb0 + NWV * c;
        const long off = (long)(kb < nkb ? kb : nkb - 1) * 128;
        xr[c] = *reinterpret_cast<const u32x4_t*>(Ab + rx + off);
        yr[c] = *reinterpret_cast<const u32x4_t*>(Ab + ry + off);
      }
    }
    MH_LOADS_ISSUED();
    if constexpr (KID >= 0) MH_STAMP(KID, 0);   // loads issued
    if (RLINES) {
      unsigned char* patch = Lw + wid * PATCH;
      const int r8 = lane >> 3, c16 = (lane & 7) * 16;
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        *reinterpret_cast<u32x4_t*>(patch + r8 * 144 + c16) = xr[c];
        *reinterpret_cast<u32x4_t*>(patch + (8 + r8) * 144 + c16) = yr[c];
        hraw[c][0] = VecOps<T>::from_patch(patch + l15 * 144 + lg * 32);
      }
    }
    float rsr[MF];
    if (LN) {
      // nn.LayerNorm statistics from the registers, two passes (mean, then the centred sum of squares -- the arithmetic of
      // F.layer_norm, no E[x^2] - mu^2 cancellation): lane -> the 4 lane groups of the wave -> the NWV waves, twice
#pragma unroll
      for (int f = 0; f < MF; ++f) {
        float q = 0.f;
#pragma unroll
        for (int c = 0; c < CH; ++c) q += (kb0 + NWV * c < nkb) ? VecOps<T>::sum(hraw[c][f]) : 0.f;
        q = xor_add_of_sum<32>(xor_add_of_sum<16>(q));   // the 4 lane groups, VALU row / half swaps (q is an accumulated sum)
        if (lg == 0) ssw[wid][f * 16 + l15] = q;
      }
      if (tid * 4 < p.K) { *reinterpret_cast<float4*>(lnw + tid * 4) = lnraw; *reinterpret_cast<float4*>(lnb + tid * 4) = lnbraw; }
      __syncthreads();
#pragma unroll
      for (int f = 0; f < MF; ++f) {
        float su = 0.f;
#pragma unroll
        for (int w = 0; w < NWV; ++w) su += ssw[w][f * 16 + l15];
        const float mu = su / (float)p.K;
        float q = 0.f;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
          hraw[c][f] = VecOps<T>::centred(hraw[c][f], mu);
          q += (kb0 + NWV * c < nkb) ? VecOps<T>::sumsq(hraw[c][f]) : 0.f;
        }
        q = xor_add_of_sum<32>(xor_add_of_sum<16>(q));   // the 4 lane groups, VALU row / half swaps (q is an accumulated sum)
        if (lg == 0) ssw2[wid][f * 16 + l15] = q;
      }
      __syncthreads();
#pragma unroll
      for (int f = 0; f < MF; ++f) {
        float ss = 0.f;
#pragma unroll
        for (int w = 0; w < NWV; ++w) ss += ssw2[w][f * 16 + l15];
        rsr[f] = rsqrtf(ss / (float)p.K + p.eps);
      }
    } else if (PRO == PRO_RMSNORM) {
      // RMSNorm statistics of the rows from the registers: lane -> the 4 lane groups of the wave -> the NWV waves
#pragma unroll
      for (int f = 0; f < MF; ++f) {
        float q = 0.f;
#pragma unroll
        for (int c = 0; c < CH; ++c) q += (kb0 + NWV * c < nkb) ? VecOps<T>::sumsq(hraw[c][f]) : 0.f;
        q = xor_add_of_sum<32>(xor_add_of_sum<16>(q));   // the 4 lane groups, VALU row / half swaps (q is an accumulated sum)
        if (lg == 0) ssw[wid][f * 16 + l15] = q;
      }
      if (tid * 4 < p.K) *reinterpret_cast<float4*>(lnw + tid * 4) = lnraw;
      __syncthreads();
#pragma unroll
      for (int f = 0; f < MF; ++f) {
        float ss = 0.f;
#pragma unroll
        for (int w = 0; w < NWV; ++w) ss += ssw[w][f * 16 + l15];
        rsr[f] = rsqrtf(ss / (float)p.K + p.eps);
      }
    }
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int kbc = kblock(kb0, c);
      const uint32_t keep = (kbc < nkb) ? 0xffffffffu : 0u;   // k-blocks beyond K contribute zeros
      const int kc_el = ((kbc < nkb) ? kbc : nkb - 1) * KB + lg * VEC;
#pragma unroll
      for (int f = 0; f < MF; ++f) {
        uint4 a;
        if (PRO == PRO_PLAIN) a = av[c][f];
        else if (LN) a = VecOps<T>::ln_frag(hraw[c][f], VecOps<T>::load_raw(lnw + kc_el), VecOps<T>::load_raw(lnb + kc_el), rsr[f]);
        else a = VecOps<T>::norm_frag(hraw[c][f], VecOps<T>::load_raw(lnw + kc_el), rsr[f]);
        a = make_uint4(a.x & keep, a.y & keep, a.z & keep, a.w & keep);
        acc[f] = VecOps<T>::mma(a, wv[c], acc[f]);
      }
    }
    kb0 += NWV * (PRO == PRO_PLAIN ? CP : CH);
  } while (kblock(kb0, 0) < nkb);

  if (!(PROBE & 8)) {
#pragma unroll
    for (int f = 0; f < MF; ++f) red[(wid * MF + f) * 64 + lane] = acc[f];
  }
  if constexpr (KID >= 0) MH_STAMP(KID, 1);     // operands arrived, products done
  if (!(PROBE & 8)) __syncthreads();
  if constexpr (KID >= 0) MH_STAMP(KID, 2);     // all waves done

  const float* redf = reinterpret_cast<const float*>(red);
#pragma unroll
  for (int u = 0; u < UPW; ++u) {
    const int unit = wid + u * NWV;
    if (unit >= MF * 4) break;
    const int ef = unit >> 2, r = unit & 3;
    float v = 0.f;
    if (PROBE & 8) {
      v = acc[0][0] + acc[MF - 1][3];
    } else {
#pragma unroll
      for (int w = 0; w < NWV; ++w) v += redf[((w * MF + ef) * 64 + lane) * 4 + r];    // wave order: deterministic
    }
    const int row = ef * 16 + lg * 4 + r;
    const bool ok = col_ok && row < p.B && (!(PROBE & 16) || p.B < 0);
    if (BIAS) v += bias_v;
    if (EPI == SK_GELU_ERF) {
      if (ok) store_wt(reinterpret_cast<T*>(p.out) + (long)row * p.ldo + ocol, Elem<T>::from_f32(0.5f * v * (1.0f + erff(v * 0.70710678118654752f))));
    } else if (EPI == SK_GEGLU) {
      // the linear half of the pair sits 8 tile columns to the right: row_ror:8 (columns >= 8 get the gate back and are never
      // stored, col_ok; whole waves reach this line -- the `unit` break above is wave-uniform)
      const float lin = lane_xor<8>(v);
      if (ok) store_wt(reinterpret_cast<T*>(p.out) + (long)row * p.ldo + ocol, Elem<T>::from_f32(gelu_tanh(v) * lin));
    } else if (EPI == SK_LOGITS) {
      if (ok) store_wt(reinterpret_cast<float*>(p.out) + (long)row * p.ldo + ocol, v);
    } else if (EPI == SK_RESID) {
      if (ok) store_wt(p.h + (long)row * p.ldh + ocol, oldh[u] + v);
    }
  }
  if constexpr (KID >= 0) MH_STAMP(KID, 3);     // epilogue stores issued
#undef MH_LOAD_OLDH
}

// the stand-alone GEMV: one workgroup = one group = tile blockIdx.x
template <typename T, int MF, int NWV, int PRO, int EPI, bool BIAS = false>
__global__ __launch_bounds__(NWV * 64) __attribute__((amdgpu_waves_per_eu(NWV / 4, 4)))   // registers are free here: never trade a load for one
void gemv_kernel(MH_GEMV_LEAD_PARAMS, SkinnyP p) {
  p.A = A_; p.W = W_; p.h = h_; p.ln_w = lnw_; p.K = K_; p.lda = K_; p.ldw = K_; p.B = B_; p.N = N_; p.nv = nv_;
  if (EPI == SK_RESID) p.ldh = N_;   // the residual stream is dense [B, N] (checked on the host)
  constexpr bool NORM = PRO != PRO_PLAIN, LN = PRO == PRO_LAYERNORM;
  __shared__ GemvLds<T, MF, NWV, PRO> L;
  __shared__ __attribute__((aligned(16))) float lnw[NORM ? 1024 : 4];   // norm weight, staged once per workgroup
  __shared__ __attribute__((aligned(16))) float lnb[LN ? 1024 : 4];     // LayerNorm bias
  MH_STAMP0();
  gemv_tile<T, MF, NWV, PRO, EPI, BIAS, KID_GEMV + EPI * 2 + (NWV == 8 ? 1 : 0), false>(p, blockIdx.x, threadIdx.x, L, lnw, lnb, WFrag{} MH_T0_ARG);
}

// ---- the three-GEMV tail of a layer as ONE launch --------------------------------------------------------------------
// [cross O GEMV + residual] -> [norm + wi GEMV + activation] -> [wo GEMV + residual] by G persistent 512-thread workgroups
// per chain: each phase is gemv_tile() -- the code and the summation order of the three stand-alone launches, bit for bit
// -- over the tiles g, g + G, ... (a 4-wave phase runs as two independent 4-wave groups with a tile and an LDS block each).
// Between two phases every workgroup has to see what ALL workgroups wrote: a hand-off through one counter in the decode
// workspace.  What the form buys: the weight fragments of a workgroup's first tile of the NEXT phase depend on nothing the
// current phase writes, so they are requested before the wait and arrive during it; a later phase then costs the hand-off
// plus ONE round trip (its activations) instead of a kernel start plus two.
//
// Hand-off.  The counter (per chain and layer parity) only ever grows: dec_init_kernel zeroes it, every hand-off adds G.
// When a tail kernel starts, every earlier one of its chain has finished (one stream), so the counter is a multiple of G
// and stays below that value + G until this workgroup itself has arrived: the value a workgroup reads at any time before
// its own first arrival, rounded down to a multiple of G, is the base of this launch for all of them -- nothing is reset inside a step and the
// replayed graph carries no step number.  Arrive: every wave drains its write-through stores (s_waitcnt vmcnt(0)), the
// workgroup meets at a barrier, one thread adds 1 (agent scope).  Wait: that thread polls the counter with agent-scope
// loads, s_sleep between polls, then ONE agent-scope acquire (this CU's L1 may hold lines of h from the phase before),
// its own vmcnt(0), and the workgroup's barrier.
//
// The wait is bounded: 2 ms of wall_clock64() after the workgroup's entry it writes TailP::err (DecState::tail_err) and
// the workgroup returns; a workgroup that finds the word set returns at its first hand-off without waiting, so every later
// tail kernel of the step ends at once, and mh_t5_generate reports MH_ERR_DECODE_TAIL_TIMEOUT.
// (The bound runs from the workgroup's entry, so it bounds the workgroup's life and with it every wait.  Only tail kernels read
// the word, at their first hand-off: the other kernels of the step run on and the call's tokens are invalid until the host reads
// the word at its next poll or at the end of the call.  A workgroup another process's time slice keeps off the chip for more
// than 2 ms is reported as a timeout too.  Acceptable for an option that is off by default)
//
// Residency (what a plain launch needs for the waits to end): G <= 128 per chain and the host divides 256 by the number
// of chains, so all chains' tails together are <= 256 workgroups of 8 waves, <= 36 KB of LDS (31.4 KB for T5; the LayerNorm
// variant's staged bias takes it to 35.9 KB) and, under
// amdgpu_waves_per_eu(2, 4), <= 256 VGPRs: one such workgroup fits every one of the 256 CUs (8 of 32 wave slots, 36 of 160
// KB, 2 of 8 waves per SIMD at 256 VGPRs) whatever else is resident, and every other kernel of the library -- and any
// well-formed kernel of another process -- ends without waiting for anybody, so a tail workgroup that is not yet resident
// becomes resident after finitely many kernel ends.  No cooperative launch: the node replays as a plain kernel node.
struct TailP {
  SkinnyP o, wi, wo;
  unsigned* cnt;            // generation counter of this chain and layer parity
  int* err;                 // DecState::tail_err of the chain
  int G;                    // workgroups of this launch
  long long timeout_ticks;  // wall_clock64() ticks a workgroup may live (2 ms)
};

template <typename T, int MF, int NWV, int PRO, int EPI, bool BIAS>
struct TailPhase {
  typedef GemvLds<T, MF, NWV, PRO> Lds;
  static constexpr int GROUPS = 8 / NWV;      // K-split groups of the 512-thread workgroup
  __device__ static inline int ntiles(const SkinnyP& p) { return EPI == SK_GEGLU ? (p.N / 2 + 7) / 8 : (p.N + p.nv - 1) / p.nv; }
  __device__ static __forceinline__ WFrag issue(const SkinnyP& p, int g) {
    const int grp = threadIdx.x / (NWV * 64), tid = threadIdx.x % (NWV * 64);
    return gemv_issue_w<T, MF, NWV, PRO, EPI>(p, g * GROUPS + grp, tid);
  }
  // tiles g GROUPS + grp, + G GROUPS, ...: the trip count is the same for every thread of the workgroup
  // (the first tile takes the weights requested ahead of the phase.  A later tile -- a phase with more than G GROUPS tiles:
  // none at the headline shape, where O has 96 tiles on 256 half-workgroups, wi 256 on 256, wo 96 on 128 -- loads its own
  // and pays the stand-alone kernel's two round trips inside the phase.)
  __device__ static __forceinline__ void run(const SkinnyP& p, int g, int G, Lds* lds, float* lnw, float* lnb, const WFrag w MH_T0_PARAM) {
    const int grp = threadIdx.x / (NWV * 64), tid = threadIdx.x % (NWV * 64);
    const int nt = ntiles(p);
    int t0 = g * GROUPS;
    if (t0 >= nt) return;
    gemv_tile<T, MF, NWV, PRO, EPI, BIAS, -1, true>(p, t0 + grp, tid, lds[grp], lnw, lnb, w MH_T0_ARG);
    for (t0 += G * GROUPS; t0 < nt; t0 += G * GROUPS) {
      __syncthreads();   // the LDS of the previous tile is read to the end
      gemv_tile<T, MF, NWV, PRO, EPI, BIAS, -1, false>(p, t0 + grp, tid, lds[grp], lnw, lnb, WFrag{} MH_T0_ARG);
    }
  }
};

// arrive at, then wait for, the hand-off that completes at counter value `target`; false: give up (the workgroup returns)
__device__ inline bool tail_handoff(const TailP& p, unsigned base, int nth, int err0, long long t_enter, int* s_ok MH_T0_PARAM) {
  __syncthreads();                   // every wave has drained its stores (the caller)
  if (threadIdx.x == 0) {
    int ok = 1;
    __hip_atomic_fetch_add(p.cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (err0 != 0) {
      ok = 0;
    } else {
      const unsigned target = base + (unsigned)nth * (unsigned)p.G;
      for (bool first = true;; first = false) {
        const unsigned c = __hip_atomic_load(p.cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // (profiling build) the first poll has returned: loads complete in order, so this wave's weight fragments of the next
        // phase, requested before the arrival, are in registers -- what remains of the wait is the hand-off alone
        if (first) MH_STAMP(KID_TAIL, 6 + nth);
        if ((int)(c - target) >= 0) break;
        if ((long long)wall_clock64() - t_enter > p.timeout_ticks) {
          __hip_atomic_store(p.err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          ok = 0;
          break;
        }
        __builtin_amdgcn_s_sleep(2);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    *s_ok = ok;
  }
  __syncthreads();
  return *s_ok != 0;
}

template <typename T, int MF, int NWO, int NWI, int NWW, int PROWI, int EPIWI, bool BIAS>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 4)))   // registers are free here, as in the GEMVs
void dec_tail_kernel(TailP p) {
  typedef TailPhase<T, MF, NWO, PRO_PLAIN, SK_RESID, BIAS> PO;
  typedef TailPhase<T, MF, NWI, PROWI, EPIWI, (BIAS || EPIWI == SK_GELU_ERF)> PI;
  typedef TailPhase<T, MF, NWW, PRO_PLAIN, SK_RESID, BIAS> PW;
  union Lds {
    typename PO::Lds o[PO::GROUPS];
    typename PI::Lds i[PI::GROUPS];
    typename PW::Lds w[PW::GROUPS];
  };
  __shared__ Lds lds;
  __shared__ __attribute__((aligned(16))) float lnw[1024];
  __shared__ __attribute__((aligned(16))) float lnb[PROWI == PRO_LAYERNORM ? 1024 : 4];
  __shared__ int s_ok;
  MH_STAMP0();
  const long long t_enter = (long long)wall_clock64();
  const int g = blockIdx.x;
  WFrag w = PO::issue(p.o, g);
  PO::run(p.o, g, p.G, lds.o, lnw, lnb, w MH_T0_ARG);
  MH_STAMP(KID_TAIL, 0);   // O phase done (stores issued)
  // the base of this launch's hand-offs and the error word: any value read before this workgroup's own arrival will do, so
  // they ride on the drain of the stores instead of costing a round trip at the kernel's start
  unsigned c0 = 0;
  int err0 = 0;
  if (threadIdx.x == 0) {
    c0 = __hip_atomic_load(p.cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    err0 = __hip_atomic_load(p.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's write-through stores have left
  w = PI::issue(p.wi, g);   // weight run-ahead: in flight across the hand-off
  MH_STAMP(KID_TAIL, 1);   // stores drained, wi weights requested
  const unsigned base = c0 - c0 % (unsigned)p.G;
  if (!tail_handoff(p, base, 1, err0, t_enter, &s_ok MH_T0_ARG)) return;
  MH_STAMP(KID_TAIL, 2);   // hand-off 1 over
  PI::run(p.wi, g, p.G, lds.i, lnw, lnb, w MH_T0_ARG);
  MH_STAMP(KID_TAIL, 3);   // wi phase done
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  w = PW::issue(p.wo, g);
  MH_STAMP(KID_TAIL, 4);   // stores drained, wo weights requested
  if (!tail_handoff(p, base, 2, 0, t_enter, &s_ok MH_T0_ARG)) return;
  MH_STAMP(KID_TAIL, 5);   // hand-off 2 over
  PW::run(p.wo, g, p.G, lds.w, lnw, lnb, w MH_T0_ARG);
  MH_STAMP(KID_TAIL, 6);   // wo phase done
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

// ---- e4m3 shadow of the self-attention cache (mh_t5_generate_skv8) ---------------------------------------------------------
// One cached key / value row (64 elements of one layer, row, head, position) = 64 OCP e4m3 bytes + one fp32 scale:
// scale = absmax / 448 (1 for an all-zero row), element = cvt_e4m3(x * (1 / scale)) -- the reciprocal-multiply form of
// kv_quant_fp8_kernel (t5.hip).  quant_row64 is the ONE statement of it: the token step's append and the bulk pass after the prompt
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

// ---- attention kernels that project their own query (and the new self-attention key / value) --------------------
// A decode step is ~100 dependent kernels of a few microseconds each, so every kernel removed from the chain is worth
// more than the work it did.  The per-head projections are tiny (64 outputs x d inputs): each attention workgroup
// recomputes RMSNorm(h[b]) and its own 64-row slice of W (the slices of one head are shared by the B workgroups of
// that head through L2), which removes the stand-alone QKV and cross-Q GEMV launches from every layer.
struct HeadProjP {
  const float* h; int ldh;            // fp32 residual stream [B, ldh]
  const float* ln_w; float eps;
  const void* W; int ldw;             // [rows, ldw] element type T (cross: Wq [inner][d]; self: Wqkv [3 inner][d])
  int d;
  const float* ln_b;                  // kernel template LN (HF Whisper, library arch 2): affine nn.LayerNorm -- its bias; ln_w = its weight
};

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

// self-attention of one (b, h) with its own q / k / v projections: appends the new key / value row to the caches and
// attends over keys 0 .. pos-1 from the cache plus the new key straight from LDS (merged last)
// F8 (bf16 storage only; mh_t5_generate_skv8): keys 0 .. pos-1 come from the e4m3 shadow cache `f8` with their per-row scales (64-byte
// rows, 8 bytes per lane); the new key / value are attended at storage precision from LDS as ever, written to the bf16 cache as ever
// (256 bytes per workgroup: the bf16 cache stays valid for everything that reads it) and appended to the shadow by waves 1 / 2
// IDX (mh_t5_step_indexed: beam search without cache copies): cached key / value j < pos of decode row b is read from cache row
// origin[b][j]; the new row is still written to cache row b at pos.  The row's table entries are requested with the first round trip
// and staged in LDS, so that the key loop has no dependent global load in front of its K / V loads.  Everything else -- bias, masks,
// window, the order of every sum -- is per decode row b as in the plain form: same bits as a cache whose rows were copied.
// F8 with IDX (mh_t5_step_indexed_skv8): cached key / value j < pos is the e4m3 row of shadow row origin[b][j] with THAT row's scale
// pair; the new row goes to bf16 cache row b and, quantised, to shadow row b at pos -- never to an origin row, so the shadow keeps
// the table's invariant (every (row, position) written once, no entry goes stale).
// SLOT (mh_t5_slots_*: in-flight decode, every row a slot with a window of its own): the position of row b is slot_pos[b], the row's
// own, instead of the chain's *pos; a negative entry is an idle slot, whose workgroups return before they store anything -- so no step
// can write a cache row that an admission is filling (the admission makes the entry non-negative last, and the chain waits for the
// admission's event before the step that first sees it).  Everything else is the plain form of that row at that position: bias row,
// RoPE row, j_first, the key-loop split, the new key merged last, the order of every sum -- the bits of a batch-1 call at *pos =
// slot_pos[b].  The prompt mask is [rows][P] with P the stride of the slot's mask buffer (ones behind the row's own prompt).  No IDX.
// F8 with SLOT (mh_t5_slots_open_kv8): the F8 row of the uniform call at the row's own position -- keys < slot_pos[b] from shadow row b
// with their scales, the new key / value at storage precision, appended by waves 1 / 2 to shadow row b at slot_pos[b]; an idle slot
// returns before the append too.  Every key below the position was written by this window's admission or by its own earlier steps,
// so what an earlier window (or nobody) left in the row is never read.
// The flag is on the kernel's BODY; the two kernels below are its entry points.  dec_self_attn_qkv_kernel keeps its six template
// arguments -- its instantiations are a pinned list (tests/test_beam_self_kv_fp8_cpu.py) with pinned instruction bytes
// (tools/device_code_diff.py) -- and the slot form is dec_slot_self_attn_kernel<T, KC, WH, LN[, F8]>.
template <typename T, int KC, bool WH = false, bool LN = false, bool F8 = false, bool IDX = false>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(4, 4)))   // 16 waves = 4 per SIMD: the whole 128-register budget
void dec_self_attn_qkv_kernel(const float* h_, const float* lnw_, const void* W_, const int* pos_,
                                                                 const void* kc_, const void* vc_, int H_, int d_, SelfAttnP p,
                                                                 HeadProjP hp,   // leading scalars: preloaded kernel arguments
                                                                 typename std::conditional<F8, typename std::conditional<IDX, SelfKv8IdxP, SelfKv8P>::type,
                                                                                           typename std::conditional<IDX, SelfIdxP, NoSelfKv8P>::type>::type f8) {
  constexpr bool SLOT = false;
#include "decode_self_attn_body.hpp"
}
// the slot form (SLOT above): the same arguments, the positions of the chain's rows behind them
// (IDX / SLOT are template parameters only so that the body's `if constexpr` branches stay dependent: never given)
template <typename T, int KC, bool WH = false, bool LN = false, bool F8 = false, bool IDX = false, bool SLOT = true>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(4, 4)))
void dec_slot_self_attn_kernel(const float* h_, const float* lnw_, const void* W_, const int* pos_, const void* kc_, const void* vc_,
                               int H_, int d_, SelfAttnP p, HeadProjP hp, typename std::conditional<F8, SelfKv8SlotP, SelfSlotP>::type f8) {
  static_assert(SLOT && !IDX, "the slot form");
#include "decode_self_attn_body.hpp"
}

}  // namespace dec
}  // namespace mh
