// Teacher-forced scoring: a row of fp32 logits -> the statistics MaiMod reads from it (reference
// osuT5/osuT5/inference/processor.py:519-525), without the logits leaving the device:
//   probs     = softmax(logits)
//   entropy   = -sum(probs * log2(probs + 1e-10))
//   surprisal = -log2(probs[target] + 1e-10)
//   relative  = surprisal / entropy where entropy > 0, else 0
//   best_id   = argmax(logits)            (lowest index on ties)
// plus logprob = log_softmax(logits)[target] (natural log, no epsilon).
//
// One workgroup of 256 threads per row.  The row is read from memory ONCE into LDS (V <= 8192; longer rows are re-read, from
// L2) and stays there for the three passes: max / argmax, exponentials and their sum (the exponentials replace the logits in
// LDS), entropy terms.  Every sum has a fixed shape -- thread t adds its elements t, t + 256, ... in ascending order, the 64
// lanes of a wave meet in a xor butterfly, the 4 waves are added in wave order -- and runs in fp64, so a row's result depends
// on nothing but the row: two runs agree bit for bit.  exp / log2 are the accurate fp32 library functions (the quantities are
// compared against the reference's fp32 evaluation to within a few ulps).  32 KB of row stage + 64 bytes of reduction scratch =
// 32832 bytes of static LDS: four workgroups (16 waves) per CU of 160 KB.
#include <limits.h>

#include "internal.hpp"

namespace mh {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kLdsRow = 8192;   // floats of a row kept in LDS

__device__ inline double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ inline double block_sum_f64(double v, double* scratch) {   // scratch: kWaves doubles; all threads get the result
  v = wave_sum_f64(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = 0.0;
#pragma unroll
  for (int i = 0; i < kWaves; ++i) r += scratch[i];
  return r;
}

__device__ inline void write_unscored(long o, float* surprisal, float* entropy, float* relative, float* logprob, int32_t* best_id) {
  surprisal[o] = 0.f; entropy[o] = 0.f; relative[o] = 0.f; logprob[o] = 0.f; best_id[o] = -1;
}

__global__ __launch_bounds__(kThreads) void score_rows_kernel(const float* __restrict__ logits, long row_stride, int V,
                                                              const int32_t* __restrict__ target, const int32_t* __restrict__ map,
                                                              const int32_t* __restrict__ count, int base, int cap,
                                                              float* __restrict__ surprisal, float* __restrict__ entropy,
                                                              float* __restrict__ relative, float* __restrict__ logprob,
                                                              int32_t* __restrict__ best_id) {
  __shared__ float s_row[kLdsRow];
  __shared__ double s_red[kWaves];
  __shared__ float s_max[kWaves];
  __shared__ int s_arg[kWaves];
  const int r = blockIdx.x, tid = threadIdx.x;
  long o = r;
  if (map) {   // compacted rows: entry base + r of the list, if the list is that long (block-uniform)
    const int n = *count < cap ? *count : cap;
    if (base + r >= n) return;
    o = map[base + r];
  }
  const int tgt = target[o];
  if (tgt < 0 || tgt >= V) {   // not scored (a target >= V never indexes the row)
    if (tid == 0) write_unscored(o, surprisal, entropy, relative, logprob, best_id);
    return;
  }
  const float* x = logits + (long)r * row_stride;
  const bool staged = V <= kLdsRow;

  // pass 1: the row into LDS; maximum and its lowest index
  float m = -INFINITY;
  int mi = INT_MAX;
  for (int i = tid; i < V; i += kThreads) {
    const float v = x[i];
    if (staged) s_row[i] = v;
    if (v > m || mi == INT_MAX) { m = v; mi = i; }   // ascending i: a tie keeps the earlier index
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float om = __shfl_xor(m, off, 64);
    const int oi = __shfl_xor(mi, off, 64);
    if (oi != INT_MAX && (mi == INT_MAX || om > m || (om == m && oi < mi))) { m = om; mi = oi; }
  }
  if ((tid & 63) == 0) { s_max[tid >> 6] = m; s_arg[tid >> 6] = mi; }
  __syncthreads();
  m = s_max[0]; mi = s_arg[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) {
    const float om = s_max[w];
    const int oi = s_arg[w];
    if (oi != INT_MAX && (mi == INT_MAX || om > m || (om == m && oi < mi))) { m = om; mi = oi; }
  }

  // pass 2: e = exp(x - max) (kept in LDS in place of x), S = sum e
  double acc = 0.0;
  for (int i = tid; i < V; i += kThreads) {
    const float e = expf((staged ? s_row[i] : x[i]) - m);
    if (staged) s_row[i] = e;
    acc += (double)e;
  }
  const double S = block_sum_f64(acc, s_red);
  const float Sf = (float)S;

  // pass 3: entropy terms p * log2(p + 1e-10), p = e / S in fp32 as the reference's softmax has it
  acc = 0.0;
  for (int i = tid; i < V; i += kThreads) {
    const float e = staged ? s_row[i] : expf(x[i] - m);
    const float p = e / Sf;
    acc += (double)(p * log2f(p + 1e-10f));
  }
  const double ent = block_sum_f64(acc, s_red);

  if (tid == 0) {
    const float xt = x[tgt];
    const float pt = expf(xt - m) / Sf;
    const float sur = -log2f(pt + 1e-10f);
    const float en = -(float)ent;
    surprisal[o] = sur;
    entropy[o] = en;
    relative[o] = en > 0.f ? sur / en : 0.f;
    logprob[o] = (float)((double)(xt - m) - log(S));
    best_id[o] = mi;
  }
}

__global__ __launch_bounds__(256) void score_fill_kernel(int n, float* __restrict__ surprisal, float* __restrict__ entropy,
                                                         float* __restrict__ relative, float* __restrict__ logprob,
                                                         int32_t* __restrict__ best_id) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) write_unscored(i, surprisal, entropy, relative, logprob, best_id);
}

// one workgroup: stable compaction of the scored positions (ballot + popcount inside a wave, wave totals in wave order)
__global__ __launch_bounds__(1024) void score_compact_kernel(const int32_t* __restrict__ target, int n, int V,
                                                             int32_t* __restrict__ map, int32_t* __restrict__ count) {
  __shared__ int s_w[16];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int base = 0;
  for (int c0 = 0; c0 < n; c0 += 1024) {
    const int i = c0 + tid;
    bool f = false;
    if (i < n) { const int t = target[i]; f = t >= 0 && t < V; }
    const unsigned long long bal = __ballot(f);
    if (lane == 0) s_w[w] = __popcll(bal);
    __syncthreads();
    int off = 0, total = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) { const int c = s_w[k]; off += k < w ? c : 0; total += c; }
    if (f) map[base + off + __popcll(bal & ((1ull << lane) - 1ull))] = i;
    base += total;
    __syncthreads();
  }
  if (tid == 0) *count = base;
}

__global__ __launch_bounds__(256) void score_gather_kernel(const float* __restrict__ h, int d, const int32_t* __restrict__ map,
                                                           const int32_t* __restrict__ count, int base, int cap,
                                                           float* __restrict__ dst) {
  const int r = blockIdx.x;
  const int n = *count < cap ? *count : cap;
  float4* out = reinterpret_cast<float4*>(dst + (long)r * d);
  if (base + r < n) {
    const float4* in = reinterpret_cast<const float4*>(h + (long)map[base + r] * d);
    for (int k = threadIdx.x; k < d / 4; k += 256) out[k] = in[k];
  } else {
    for (int k = threadIdx.x; k < d / 4; k += 256) out[k] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

}  // namespace

int score_rows(const float* logits, int64_t row_stride, int R, int V, const int32_t* target, const int32_t* map,
               const int32_t* count, int base, int cap, float* surprisal, float* entropy, float* relative, float* logprob,
               int32_t* best_id, hipStream_t s) {
  hipLaunchKernelGGL(score_rows_kernel, dim3(R), dim3(kThreads), 0, s, logits, (long)row_stride, V, target, map, count, base, cap,
                     surprisal, entropy, relative, logprob, best_id);
  return check_launch("score_rows_kernel");
}

int score_compact(const int32_t* target, int n, int V, int32_t* map, int32_t* count, float* surprisal, float* entropy,
                  float* relative, float* logprob, int32_t* best_id, hipStream_t s) {
  hipLaunchKernelGGL(score_fill_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, s, n, surprisal, entropy, relative, logprob, best_id);
  hipLaunchKernelGGL(score_compact_kernel, dim3(1), dim3(1024), 0, s, target, n, V, map, count);
  return check_launch("score_compact_kernel");
}

int score_gather(const float* h, int d, const int32_t* map, const int32_t* count, int base, int cap, float* dst, int rows,
                 hipStream_t s) {
  hipLaunchKernelGGL(score_gather_kernel, dim3(rows), dim3(256), 0, s, h, d, map, count, base, cap, dst);
  return check_launch("score_gather_kernel");
}

}  // namespace mh

extern "C" int mh_score_rows(const float* logits, int64_t row_stride, int R, int V, const int32_t* target, float* surprisal,
                             float* entropy, float* relative, float* logprob, int32_t* best_id, void* stream) {
  MH_REQUIRE(logits && target && surprisal && entropy && relative && logprob && best_id, "mh_score_rows: null argument");
  MH_REQUIRE(R > 0 && V > 0, "mh_score_rows: bad shape R=%d V=%d", R, V);
  MH_REQUIRE(row_stride >= V, "mh_score_rows: row_stride %lld smaller than V=%d", (long long)row_stride, V);
  return mh::score_rows(logits, row_stride, R, V, target, nullptr, nullptr, 0, 0, surprisal, entropy, relative, logprob, best_id,
                        (hipStream_t)stream);
}
