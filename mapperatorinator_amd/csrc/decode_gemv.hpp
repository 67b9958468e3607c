// The decode GEMV and the three-GEMV tail of a layer built from it (gemv_tile): instantiated in decode_gemv.hip and nowhere else.
#pragma once
#include "decode_device.hpp"

namespace mh {
namespace dec {

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
// (PRO_* / SK_* and SkinnyP: decode_params.hpp)

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
// (TailP: decode_params.hpp)

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

}  // namespace dec
}  // namespace mh
