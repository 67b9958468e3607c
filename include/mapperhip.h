/*
 * libmapperhip -- C ABI of the MI355X-native (gfx950) audio->event hot path of Mapperatorinator.
 *
 * Every entry point below replaces a *Python call site into third-party device code* of the
 * reference (the reference owns no native code); the file:line after each
 * declaration is the reference interface it stands in for (paths relative to the reference root).
 *
 * Conventions (all entry points):
 *   - plain C: raw DEVICE pointers + sizes, no torch / C++ types;
 *   - asynchronous on the given `hipStream_t` (passed as void*), no hidden allocation, no host sync
 *     (the one exception, mh_t5_generate, documents its polling); caller owns every buffer;
 *   - returns MH_OK (0) or a negative MhStatus; the message is available from mh_last_error();
 *     never throws, never aborts;
 *   - `dtype` is MH_F32 or MH_BF16: the storage type of weights and GEMM operands.  Accumulation,
 *     normalisation, softmax, the residual stream and logits are always fp32.
 */
#ifndef MAPPERHIP_H_
#define MAPPERHIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MH_ABI_VERSION 11
#define MH_MAX_LAYERS 32

typedef enum MhStatus {
  MH_OK = 0,
  MH_ERR_ARG = -1,     /* bad argument (shape / alignment / null) */
  MH_ERR_LAUNCH = -2,  /* HIP launch or runtime error */
  MH_ERR_STATE = -3,   /* object used in the wrong state */
  MH_ERR_DECODE_TAIL_TIMEOUT = -4,   /* a bounded in-kernel wait of the decode step's fused layer tail gave up (decode_fused_tail) */
} MhStatus;

/* MH_MX8 (ABI 7): OCP MX-fp8 -- e4m3 elements (one byte each) + one E8M0 scale byte per (row, 32 consecutive k); an OPERAND
 * type of mh_gemm and of the reduced-precision modes built on it (MhT5Config.enc_operand_dtype, MhDiTConfig.operand_dtype),
 * never a storage type of activations that leave a stage.  Layouts: see mh_quantize_mx8. */
typedef enum MhDtype { MH_F32 = 0, MH_BF16 = 1, MH_MX8 = 2 } MhDtype;

/* epilogues of mh_gemm */
typedef enum MhEpilogue {
  MH_EPI_STORE = 0,      /* C[T]   = A W^T (+bias)                                  */
  MH_EPI_STORE_F32 = 1,  /* C[f32] = A W^T (+bias)                                  */
  MH_EPI_RESID = 2,      /* C[f32] += A W^T (+bias)                                 */
  MH_EPI_GEGLU = 3,      /* C[T][M,N/2] = gelu_tanh(acc[:,blk even]) * acc[:,blk odd];
                            W rows interleaved in blocks of 16 (wi_0 blk, wi_1 blk, ...) */
  MH_EPI_BIAS_GELU = 4,  /* C[T]   = gelu_tanh(A W^T + bias)                        */
  MH_EPI_GATE_RESID = 5, /* C[f32][m,n] += gate[m / rows_per_batch, n] * (A W^T + bias)[m,n] */
  MH_EPI_KV_SCATTER = 6, /* C[T] scattered to [(layer,kv)][b][h][key][64]; see mh_t5_cross_kv */
  MH_EPI_QKV_VT = 7,     /* cols < n_split: C[T] = A W^T (+bias) (q|k block, ldc);
                            cols >= n_split (the v block, col' = h*64+dd, row = b*kv_L+key):
                            C2[T][((b*kv_H + h)*64 + dd)*kv_Lpad + key]  (V transposed per head)  */
  MH_EPI_QKV_CACHE = 8,  /* decoder prompt prefill: rows m = b*kv_L + i (prompt position i of chunk b);
                            cols < n_split: C[T] (q, ldc); then the k block -> C2 and the v block -> C3, both
                            [B][H][cache_len][64] at position i; the v block is also written transposed to
                            C4[T][((b*kv_H + h)*64 + dd)*kv_Lpad + i]                                     */
  MH_EPI_BIAS_GELU_ERF = 9, /* C[T] = gelu_erf(A W^T + bias) (+ gate[m % rows_per_batch, n] when gate != NULL:
                               the Whisper position table)                                                 */
} MhEpilogue;

const char* mh_last_error(void);
int mh_abi_version(void);

/* Tuning options (process-wide; per engine through an option set, below): each has a default, an environment override read at first use and this run-time
 * setter.  They choose between kernels that compute the same results (bit-identical unless noted):
 *   "gemm_splitk_tiles"  MH_GEMM_SPLITK_TILES  192  fp32/bf16 GEMMs with fewer 32x32 tiles than this use the 16x16
 *                                                   split-K tile (different fp32 summation order); 0 = never
 *   "decode_chains"      MH_DECODE_CHAINS      0    independent row chains of a decode step (0 = automatic)
 *   "decode_prefill"     MH_DECODE_PREFILL     1    batched prompt prefill (0: token by token)
 *   "decode_gemv_cols"   MH_DECODE_GEMV_COLS   0    valid columns per 16-column tile of the decode GEMVs (0 = automatic)
 *   "gemm_glds"          MH_GEMM_GLDS          3    bf16 GEMM operands by LDS-DMA: 3 = three-stage kernel (256x128 tiles, 128x128
 *                                                   below half a wave of them), 2 = 256x128 only, 1 = two-stage 128x128,
 *                                                   0 = register staging
 *   "decode_launch_threads" MH_DECODE_LAUNCH_THREADS 1  one host launcher thread per decode chain; 0 = one thread feeds all chains
 *                                                   round robin (for profilers whose counter passes do not survive concurrent
 *                                                   launcher threads)
 *   "decode_graph_cache" MH_DECODE_GRAPH_CACHE 1    step graphs kept across mh_t5_generate calls (0: captured per call)
 *   "gemm_tile256sq_min" MH_GEMM_TILE256SQ_MIN 440  bf16 GEMM: the 256x256 tile (two LDS stages, 128x64 wave tiles, staggered wave
 *                                                   groups) from this many tiles on when its rounds of 256 workgroups are >= 88 %
 *                                                   full (0 = never; bit-identical to the 256x128 three-stage kernel)
 *   "gemm_2stage_max_k"  MH_GEMM_2STAGE_MAX_K  512  bf16 GEMM with K <= this: 128x128 tile on two LDS stages, two workgroups per CU
 *                                                   (0 = never; bit-identical)
 *   "beam_step_path"     MH_BEAM_STEP_PATH     0    mh_beam_step: 0 = LDS kernel where it fits, else the streaming kernel; 1 = LDS
 *                                                   kernel or an error; 2 = streaming kernel everywhere (bit-identical)
 *   "decode_fused_tail"  MH_DECODE_FUSED_TAIL  0    decode step: the three GEMVs that close a layer (cross O + residual, norm + wi +
 *                                                   activation, wo + residual) as one persistent launch with two bounded in-kernel
 *                                                   hand-offs (bit-identical; 0 = three launches; uncovered shapes run three anyway)
 * (gemm_tile128_min and dit_split3_min_rows are documented next to their definitions in csrc/api.hip: 11 options in all.
 * Round 5 removed the measured-slower variants decode_overlap, decode_fold_oproj, decode_cu_split, decode_self_rows,
 * mx8_waves = 4, dit_s3_fused_ln, the debugging aid gemm_lds_pad, the variant switches attn_flash2, dit_s3_presplit and
 * mx8_fused_quant (the faster form is the only one left) and turned the thresholds attn_small_max_wgs, gemm_tile256_min,
 * mx8_tile256_min into constants; their measurements stay in profiles/r02_* .. r04_*.  The decode option for stand-alone
 * q / k / v and cross-query projection GEMVs went later (tried / rejected): the decode attention kernels
 * always project their own.)
 * Unknown names return MH_ERR_ARG (set) / -1 (get). */
int mh_set_option(const char* name, long value);
long mh_get_option(const char* name);
/* ABI 8 -- option sets: overrides owned by ONE engine instead of the process.  A set starts empty (every option falls through to
 * the process-wide value above); MhT5Config.options / MhDiTConfig.options point at it (NULL = process-wide values only) and every
 * entry point that takes such a config resolves its options through the set for the duration of the call, the decode chains'
 * launcher threads included.  Two engines in one process can so run different kernel variants side by side.  The set must
 * outlive the calls that name it; setting an option while a call that uses the set is in flight is a data race the caller
 * excludes.  mh_options_get returns the override, else the process-wide value; unknown names: MH_ERR_ARG / -1. */
typedef struct MhOptionSet MhOptionSet;
MhOptionSet* mh_options_create(void);
void mh_options_destroy(MhOptionSet* set);
int mh_options_set(MhOptionSet* set, const char* name, long value);
int mh_options_clear(MhOptionSet* set, const char* name);      /* drop one override (name = NULL: all of them) */
long mh_options_get(const MhOptionSet* set, const char* name);
/* sizeof() of the ABI structs as this library was compiled, so that a binding can verify its own layout:
 * which = 0 MhGemm, 1 MhT5Config, 2 MhT5Weights, 3 MhSampling, 4 MhDiTConfig, 5 MhDiTWeights,
 * 6 MhSliderSet, 7 MhBeamStep, 8 MhRowSampling; -1 otherwise. */
int mh_struct_size(int which);

/* ------------------------------------------------------------------------------------------------
 * K1  mel frontend.  Replaces `nnAudio.features.MelSpectrogram` as constructed and called at
 *     osuT5/osuT5/model/spectrogram.py:50-61 and :63-83 (zero-pad n_fft/2, hann STFT, power
 *     spectrum, Slaney mel filterbank, optional log1p, (B, frames, n_mels) layout).
 * audio   [B, n_samples] fp32.
 * out     [B, n_frames, ld_out] (fp32 if out_dtype==MH_F32 else bf16), n_frames = n_samples/hop + 1;
 *         columns [n_mels, ld_out) are written as zero (K padding for the following GEMM).
 * The sparse filterbank (CSR over mel rows) and the twiddle table are built on the host
 * (mapperatorinator_amd/mel.py) and passed in:
 *   fb_start[n_mels], fb_len[n_mels], fb_off[n_mels] (int32), fb_w[sum(len)] fp32,
 *   window[n_fft] fp32 (periodic hann), twiddle[n_fft] (cos, sin) pairs fp32.
 * log_scale: bit 0 = log1p of the mel energies (spectrogram.py:79-80); bit 1 = reflect instead of zero padding of the
 *   n_fft/2 samples either side (the `torchaudio` parameterisation of the Whisper-family configs:
 *   configs/model/whisper_base_v3.yaml:16-21 -- torch.stft(center=True, pad_mode="reflect"), HTK filterbank without
 *   area normalisation; the filterbank is whatever the host passes in).
 * n_fft must be 1024 (the only size the reference configs use: configs/model/default.yaml:29-37). */
int mh_mel(const float* audio, int B, int n_samples, int n_fft, int hop, int n_mels,
           const float* window, const float* twiddle, const int32_t* fb_start, const int32_t* fb_len,
           const int32_t* fb_off, const float* fb_w, int log_scale, void* out, int ld_out,
           int out_dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Dense layer.  Replaces `nn.Linear` / `torch.matmul` call sites on the hot path
 * (modeling_mapperatorinator.py:195-196; HF T5Attention q/k/v/o, T5DenseGatedActDense;
 *  osu_diffusion/utils/models.py:111-116,145-155).  C = A[M,K] * W[N,K]^T with a fused epilogue.
 * A, W have element type `dtype`; lda/ldw/ldc in elements; K % 8 == 0 (bf16) or % 4 (f32),
 * row starts of A and W 16-byte aligned; lda, ldw >= K (the columns [K, ld) are never read).  bias fp32[N] or NULL.
 * gate fp32 [.., gate_ld]: MH_EPI_GATE_RESID reads gate[m / rows_per_batch], MH_EPI_BIAS_GELU_ERF (gate optional: the position
 * table) adds gate[m % rows_per_batch].
 * C may be ANY pointer aligned to its element (2 bytes bf16, 4 bytes fp32 and the pre-split form), ldc >= the columns written.
 * This is a contract shown on the device, not one of the C++: the register-staged tiles store element by element, but the LDS-DMA,
 * three-stage and MX-fp8 kernels access C in vectors whatever its alignment -- fp32 outputs (STORE_F32, RESID, GATE_RESID, the
 * q | k block of the fp32 QKV_VT) are stored, and the old C loaded, as 16 bytes; bf16 outputs as 8 bytes, or as 16 bytes when C is
 * 16-byte aligned, ldc % 8 == 0 and N % 16 == 0 (pre-split output: 16 bytes when C is 16-byte aligned, ldc % 32 == 0 and
 * N % 32 == 0, else 8) -- and rely on gfx950 serving unaligned global accesses.
 * Only the documented positions are written: rows >= M and columns >= N (>= N / 2 for MH_EPI_GEGLU) of C, the V^T pad columns
 * [kv_L, kv_Lpad) of MH_EPI_QKV_VT / MH_EPI_QKV_CACHE and the cache positions [kv_L, cache_len) of MH_EPI_QKV_CACHE are left
 * untouched (tests/test_gpu_gemm.py runs every kernel and epilogue with sentinels around each output, C also at an 8-byte and at a
 * one-element offset).
 * For MH_EPI_KV_SCATTER: kv_B, kv_H, kv_L describe the scatter (rows m = b*kv_L + key) into [(layer, kv)][b][h][key][64].
 * MH_EPI_QKV_VT: columns < n_split to C; the rest, kv_H heads of v, transposed per head to C2 [b][h][64][kv_Lpad].
 * MH_EPI_QKV_CACHE (N = 3 * kv_H * 64, n_split = kv_H * 64): q to C; k to C2 and v to C3 as [b][h][cache_len][64] at position
 * i = m % kv_L; v also transposed to C4 [b][h][64][kv_Lpad]. */
typedef struct MhGemm {
  const void* A; int lda;
  const void* W; int ldw;
  void* C; int ldc;
  int M, N, K;
  const float* bias;
  const float* gate; int gate_ld; int rows_per_batch;
  int kv_B, kv_H, kv_L;
  void* C2; int n_split; int kv_Lpad;   /* MH_EPI_QKV_VT / MH_EPI_QKV_CACHE */
  void* C3; void* C4; int cache_len;    /* MH_EPI_QKV_CACHE only */
  int dtype; int epilogue;
  /* fp32 only -- adaLN `modulate(LayerNorm(x), shift, scale)` (osu_diffusion/utils/models.py:11-12,145,152) fused
   * around the GEMMs of a DiT block instead of a stand-alone pass over the activations:
   *   stats_out  (MH_EPI_STORE_F32 / MH_EPI_GATE_RESID producers) fp32 [ceil(N/16)][M][2]: per 16-column strip the
   *              sum and sum of squares of every output row, written by the epilogue;
   *   ln_stats   (consumer) the same array for the rows of A (ln_strips strips, K columns): the A operand becomes
   *              (a - mean) * rsqrt(var + ln_eps) * (1 + ln_scale[b][k]) + ln_shift[b][k], b = row / rows_per_batch,
   *              ln_shift / ln_scale fp32 with row stride ln_ld. */
  float* stats_out;
  const float* ln_stats; int ln_strips;
  const float* ln_shift; const float* ln_scale; int ln_ld; float ln_eps;
  /* fp32 only -- "bf16 x 3": W is stored PRE-SPLIT, every 32-float block of a row as [32 x bf16 hi | 32 x bf16 lo]
   * (hi = bf16(w), lo = bf16(w - hi); the same 128 bytes per block, ldw still counted in floats), A stays fp32 and is
   * split on its way into LDS; a w ~= a_hi w_hi + a_hi w_lo + a_lo w_hi on the bf16 matrix cores with fp32 accumulation
   * (relative error ~2^-16 per product instead of exact fp32 products).  K and ldw multiples of 32.
   * Bit flags: 1 = W pre-split (above); | 2 = A is stored pre-split in the same layout by its producer (lda counted in
   * floats, multiple of 32): the three-stage LDS-DMA form, no conversion work inside the GEMM (STORE_F32, QKV_VT,
   * GATE_RESID, BIAS_GELU; N, ldc multiples of 4); | 4 = with 2 and MH_EPI_BIAS_GELU: C is written pre-split as well
   * (it is the next GEMM's A operand; ldc multiple of 32). */
  int w_split3;
  /* ABI 7 -- dtype = MH_MX8 (BASELINE configs[4] "fp8 MFMA"): A [M][lda] and W [N][ldw] hold e4m3 BYTES (lda, ldw counted in
   * elements = bytes, multiples of 16; K a multiple of 128), a_scale / w_scale their E8M0 scales in the row layout of
   * mh_quantize_mx8 (mh_mx8_scale_row_bytes(K) bytes per row).  The product runs on v_mfma_scale_f32_16x16x128_f8f6f4 with
   * fp32 accumulation; outputs are what the epilogue says with T = bf16 (STORE, STORE_F32, RESID, GEGLU, BIAS_GELU,
   * GATE_RESID, KV_SCATTER, QKV_VT; N, ldc multiples of 4). */
  const uint8_t* a_scale; const uint8_t* w_scale;
  /* ABI 9 -- dtype = MH_MX8 with MH_EPI_GEGLU / MH_EPI_BIAS_GELU: when mx_out != NULL the epilogue writes the MX-fp8 image of its
   * bf16 result (the next GEMM's A operand) instead of the bf16 matrix: e4m3 bytes [M][ldc] (ldc = bytes per row) at mx_out and
   * E8M0 scales at mx_out_scales (mh_mx8_scale_row_bytes(width) bytes per row; width = N, or N / 2 for GEGLU, a multiple of 128).
   * Bit for bit what mh_quantize_mx8 makes of the bf16 result; C is not written and may be NULL. */
  uint8_t* mx_out; uint8_t* mx_out_scales;
} MhGemm;
int mh_gemm(const MhGemm* g, void* stream);
/* Test-facing (additive at ABI 11: one symbol and one enum; a library without it is an older 11): the kernel the calling thread's
 * last mh_gemm launch ran, as family * 1024 + tile rows (host-only bookkeeping, no device work; MH_GEMM_NONE before the first
 * launch).  Together with dtype and epilogue, which the caller knows, that names one compiled kernel: e.g. MH_GEMM_TN * 1024 + 16
 * is the 16 x 16 split-K tile, MH_GEMM_GLDS3 * 1024 + 128 the 128-row form of the three-stage kernel (tests/test_gpu_gemm.py). */
typedef enum MhGemmKernel {
  MH_GEMM_NONE = 0,
  MH_GEMM_TN = 1,        /* register-staged tile: 128, 64, 32 or 16 (split-K) rows                   */
  MH_GEMM_TN_S3 = 2,     /* ... its bf16 x 3 form (w_split3 = 1): 64 rows                             */
  MH_GEMM_TN_GLDS = 3,   /* ... its LDS-DMA form (bf16): 128 rows                                     */
  MH_GEMM_GLDS3 = 4,     /* three-stage LDS-DMA kernel (bf16): 256 x 128 or 128 x 128 tile            */
  MH_GEMM_GLDS2S = 5,    /* two-stage short-K kernel (bf16): 128 x 128                                */
  MH_GEMM_GLDS4 = 6,     /* two-stage 256 x 256 kernel (bf16)                                         */
  MH_GEMM_S3G = 7,       /* three-stage bf16 x 3 kernel, A pre-split (w_split3 & 2): 128 rows         */
  MH_GEMM_MX8 = 8,       /* MX-fp8 operands: 128 or 256 rows                                          */
  MH_GEMM_MX8_MXO = 9    /* ... with the MX-fp8 image as output (mx_out)                              */
} MhGemmKernel;
int mh_gemm_last_kernel(void);

/* MX-fp8 quantisation of a row-major matrix (the A / W operands of mh_gemm with dtype = MH_MX8).
 * x [rows][ldx] of in_dtype (MH_F32 / MH_BF16), K % 128 == 0 columns used.  Per (row, block of 32 consecutive k):
 *   amax = max |x|; e = floor(log2(amax)) - 8, raised by one when amax * 2^-e > 448 (the largest finite e4m3 value: nothing is
 *   ever clipped); scale byte = clamp(e + 127, 0, 254) (all-zero block: 0 with zero elements); element = RNE_e4m3(x * 2^-e).
 * q [rows][ldq] bytes (ldq >= K, multiple of 16).  scales [rows][mh_mx8_scale_row_bytes(K)] bytes, LANE-MAJOR in groups of
 * four 128-k steps: byte (kt / 4) * 16 + lg * 4 + (kt % 4) holds the scale of k block kt * 4 + lg (kt = k / 128, lg =
 * (k % 128) / 32) -- the dword a lane of the MFMA fetches for four K steps; unused bytes of the last group are 0. */
int64_t mh_mx8_scale_row_bytes(int K);
int mh_quantize_mx8(const void* x, int ldx, int rows, int K, int in_dtype, uint8_t* q, int ldq, uint8_t* scales, void* stream);
/* RMSNorm (mh_rmsnorm) with the MX-fp8 operand written directly: y = w * x * rsqrt(mean(x^2) + eps) in fp32, rounded to
 * `round_dtype` (MH_BF16: the value a bf16 activation buffer would have held; MH_F32: not rounded), then quantised as above. */
int mh_rmsnorm_mx8(const float* x, int ldx, const float* w, int rows, int d, float eps, int round_dtype, uint8_t* q, int ldq,
                   uint8_t* scales, void* stream);

/* T5 RMSNorm (HF T5LayerNorm; restated at custom_transformers/t5.py:50-62):
 * y[T] = w * x * rsqrt(mean(x^2) + eps), x fp32 [rows, d] (ldx), y [rows, ldy]. */
int mh_rmsnorm(const float* x, int ldx, const float* w, void* y, int ldy, int rows, int d, float eps,
               int out_dtype, void* stream);
/* (ABI 10) nn.LayerNorm with affine parameters -- the pre-norm of stock HF Whisper's blocks ('openai/whisper-*', the V28 / V29
 * backbones; transformers models/whisper/modeling_whisper.py WhisperEncoderLayer / WhisperDecoderLayer): y = (x - mean) *
 * rsqrt(var + eps) * w + b, biased variance of the centred values, fp32 arithmetic; x fp32 [rows, ldx], y [rows, ldy] of
 * `out_dtype`. */
int mh_layernorm(const float* x, int ldx, const float* w, const float* b, void* y, int ldy, int rows, int d, float eps,
                 int out_dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K3  T5 encoder self-attention (HF T5Attention.forward, restated custom_transformers/t5.py:170-250):
 *     softmax(scale * Q K^T + bias[h][k - q + L - 1]) V; T5: scale = 1 (no 1/sqrt(d)), bidirectional.
 * qk   [B*L, ld_qk] element type `dtype`: q of head h at columns [h*64, h*64+64), k at
 *      [k_col0 + h*64, ...);   vt [B][H][64][Lpad] = V transposed per head (MH_EPI_QKV_VT output,
 *      pad columns zero);  bias fp32 [H][2L-1] (host-built bucket lookup by k - q) or NULL;
 * out  [B*L, ld_out] element type `dtype`, head h at columns [h*64, h*64+64).
 * K7  also the DiT attention (osu_diffusion/utils/models.py:145-151): scale = 1/8, bias NULL and
 *     band > 0: query q attends key k iff -(band-1) <= k - q <= band, which is exactly the banded
 *     bool mask built at diffusion_pipeline.py:146-148 (band = seq_len = 128).  band = 0: no mask.
 *     band < 0: the symmetric window |k - q| <= -band (the local layers of the Whisper family). */
int mh_attention(const void* qk, int ld_qk, int k_col0, const void* vt, int Lpad, const float* bias,
                 void* out, int ld_out, int B, int L, int H, float scale, int band, int dtype,
                 void* stream);

/* Test-facing entries of the attention kernels (additive at ABI 11: three symbols and one struct of their own; a library without
 * them is an older 11).  They launch exactly what the models launch and add no kernel.
 *
 * mh_attention_packed: mh_attention with the two options the DiT blocks and the encoders pass internally:
 *   open_from  > 0 with band != 0: positions >= open_from are padding -- key k is visible from query q iff it is in the band OR
 *              k >= open_from OR q >= open_from (the DiT pipeline's pad_sequence); 0 = none;
 *   out_split3 != 0 (fp32 only, ld_out % 32 == 0): every 32 output values are stored as [32 x bf16 hi | 32 x bf16 lo], the
 *              pre-split A operand of MhGemm.w_split3 & 2 (a row still occupies ld_out * 4 bytes).
 *
 * mh_attention_strided: one problem in the strided form the decoder's prompt prefill and its cross-attention use.  All strides in
 * BYTES and multiples of 16; head_dim = 64.  Key `key` is visible from query row `row` (qpos = q_pos0 + row) iff
 *   key < Lk, and (key >= mask_len or key_mask[b * mask_ld + key] != 0; key_mask NULL: no mask), and
 *   (band == 0, or the key is in the band -- band > 0: -(band-1) <= key - qpos <= band; band < 0: |key - qpos| <= -band -- or, with
 *   open_from > 0, key >= open_from or qpos >= open_from), and (causal == 0 or key <= qpos).
 * A visible key's score is scale * q.k + bias[h * bias_hs + bias_center + clamp(bias_sign * (key - qpos), bias_min, bias_max)]
 * (bias NULL: none); a row without a visible key is written as zeros.  vt is V^T [B][H][64][Lkpad] with Lkpad % 64 == 0 and the
 * pad columns zero.  Refused (MH_ERR_ARG): struct_bytes != sizeof(MhAttnProblem); a null q / k / vt / out; q_pos0 < 0; q_pos0 != 0
 * together with band != 0 (the kernels pick their key tiles from the query index: no model combines the two); key_mask with
 * mask_len <= 0 or mask_ld < mask_len; out_split3 with bf16.  A bf16 problem whose out / out_rs / out_bs is not 16-byte aligned
 * runs the 64-query kernel with 2-byte stores instead of the 128-query one. */
typedef struct MhAttnProblem {
  int64_t struct_bytes;                        /* sizeof(MhAttnProblem) of the caller                                      */
  const void* q; int64_t q_rs, q_bs;           /* + b*q_bs + row*q_rs + h*64*sizeof(T)                                     */
  const void* k; int64_t k_rs, k_bs, k_hs;     /* + b*k_bs + h*k_hs + key*k_rs                                             */
  const void* vt; int64_t vt_bs, vt_hs;        /* + b*vt_bs + h*vt_hs + d*Lkpad*sizeof(T)                                  */
  const float* bias; int64_t bias_hs;
  const uint8_t* key_mask;                     /* [B][mask_ld] bytes                                                       */
  void* out; int64_t out_rs, out_bs;           /* + b*out_bs + row*out_rs + h*64*sizeof(T)                                 */
  int Lkpad, bias_center, bias_sign, bias_min, bias_max, mask_ld, mask_len;
  int Lq, Lk;
  float scale;
  int open_from, out_split3, band, causal, q_pos0;
  int B, H, dtype;
} MhAttnProblem;
int mh_attention_packed(const void* qk, int ld_qk, int k_col0, const void* vt, int Lpad, const float* bias,
                        void* out, int ld_out, int B, int L, int H, float scale, int band, int dtype,
                        int open_from, int out_split3, void* stream);
int mh_attention_strided(const MhAttnProblem* p, void* stream);
/* The kernel the calling thread's last attention launch ran (host-only bookkeeping; MH_ATTN_NONE before the first one):
 * MH_ATTN_FLASH2 carries two more bits, MH_ATTN_FLASH2_BIAS and MH_ATTN_FLASH2_SIMPLE, for its four compiled forms. */
typedef enum MhAttnKernel {
  MH_ATTN_NONE = 0,
  MH_ATTN_FLASH_F32 = 1,   /* 64-query flash kernel, fp32                                         */
  MH_ATTN_FLASH_BF16 = 2,  /* 64-query flash kernel, bf16 (outputs that are not 16-byte aligned)  */
  MH_ATTN_SMALL_K2 = 3,    /* key-split fp32 kernel, L <= 128                                     */
  MH_ATTN_SMALL_K4 = 4,    /* key-split fp32 kernel, L <= 256                                     */
  MH_ATTN_FLASH2 = 8,      /* 128-query transposed-S bf16 kernel                                  */
  MH_ATTN_FLASH2_BIAS = 1, MH_ATTN_FLASH2_SIMPLE = 2
} MhAttnKernel;
int mh_attention_last_kernel(void);

/* ------------------------------------------------------------------------------------------------
 * K2  Whisper-style audio front-end (HF WhisperEncoder.forward prologue; reference forks
 *     osuT5/osuT5/model/custom_transformers/modeling_varwhisper.py:779-780,813-816):
 *     y = gelu(conv1d(x, k=3, pad=1)); z = gelu(conv1d(y, k=3, stride=2, pad=1)); out = z (+ pos).
 * x   [B, Lin, C]   time-major activations (element type `dtype`) -- the transpose of HF's input_features
 * w1  [d, Kpad1], w2 [d, Kpad2]: conv weights repacked tap-major, W'[o][k*Cin + c] = W[o][c][k], K padded
 *     with zeros to a multiple of 32;  b1, b2 fp32 [d];  pos fp32 [Lout, d] or NULL (fixed sinusoid table)
 * out [B, Lout, d], Lout = (Lin - 1) / 2 + 1. */
int64_t mh_whisper_frontend_workspace_bytes(int B, int Lin, int C, int d, int dtype);
int mh_whisper_frontend(const void* x, int B, int Lin, int C, const void* w1, const float* b1, const void* w2,
                        const float* b2, const float* pos, int d, void* out, void* workspace,
                        int64_t workspace_bytes, int dtype, void* stream);

/* (ABI 10) The wrapper's conditioning vectors as INPUT CHANNELS of the front-end: with project_encoder_input = false
 * (configs/model/whisper_small_v2.yaml: the V30 / V31 'Tiger14n/ropewhisper-small' releases, cond_size 384) the per-row
 * difficulty / mapper / song-position vectors are repeated over the frames and concatenated to the mel channels
 * (osuT5/osuT5/model/modeling_mapperatorinator.py:183-202), so conv1 sees n_mels + cond_size channels -- a k = 3 convolution with
 * zero padding, where the constant channels do NOT reduce to a row bias (the first and last frame miss one tap).
 * frames [B * L, ld] (element type `dtype`, the K-padded buffer mh_mel wrote); cond fp32 [B, n_cond] (already rounded to the
 * storage type by the caller); writes frames[(b, t)][col0 + j] = cond[b][j]. */
int mh_cond_channels(void* frames, int B, int L, int ld, int col0, const float* cond, int n_cond, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * T5 model object: weights are caller-owned device buffers (packed by the host, see
 * mapperatorinator_amd/t5_engine.py) described by MhT5Weights.  All matrices are [N][Kpad] row major,
 * element type cfg.dtype, K padded with zeros to a multiple of 32.
 */
typedef struct MhT5Config {
  int d_model, d_kv, d_ff, n_heads, n_enc_layers, n_dec_layers;
  int vocab_in, vocab_out;
  int n_mels, n_mels_pad;   /* encoder_embedder K and its padded leading dimension */
  int src_len;              /* L: mel frames per chunk (encoder positions)             */
  int tgt_len;              /* max_target_positions = StaticCache length                */
  int dtype;                /* MhDtype                                                  */
  float eps;                /* RMSNorm epsilon (T5: 1e-6; Whisper family: nn.RMSNorm(eps=None) = finfo(dtype).eps) */
  /* --- ABI 5: the Whisper-family backbone of the released V30-V32 checkpoints ('OliBomby/varwhisper-*',
   * osuT5/osuT5/model/custom_transformers/modeling_varwhisper.py) behind the same entry points ------------------------ */
  int arch;                 /* 0 = T5-v1.1 (relative bias, unscaled scores, gated-GELU FFN); 1 = VarWhisper: conv front-end,
                               pre-norm RMSNorm blocks, fused Wqkv / Wo and fc1 -> gelu(erf) -> fc2 with optional biases,
                               rotate-half RoPE on q / k of the self-attentions, scores * attn_scale, untied head        */
  float attn_scale;         /* arch 1: 1 / sqrt(64)                                                                      */
  int in_frames;            /* arch 1: log-mel frames per chunk entering the front-end (`mel` rows per chunk); src_len is
                               then the number of ENCODER positions = (in_frames - 1) / 2 + 1 (conv2 stride 2), which is
                               what the cross-attention streams.  arch 0: unused (= src_len)                             */
  int local_every;          /* arch 1: global_attn_every_n_layers -- layer l is LOCAL iff l % local_every != 0; <= 1: none */
  int local_window;         /* arch 1: local_attention // 2 keys either side for local layers (the reference applies the
                               window on its flash-attention path only, modeling_varwhisper.py:330)                      */
  /* --- ABI 7: BASELINE configs[4] "fp8 MFMA" ----------------------------------------------------------------------- */
  int enc_operand_dtype;    /* 0 (= the storage type) or MH_MX8: the encoder blocks' four projections and the cross-K/V
                               projection take MX-fp8 operands (weights pre-quantised by the host: MhT5Weights.*_mx;
                               activations quantised where they are produced: RMSNorm output directly, attention output and
                               gated-GELU hidden by a pass over the bf16 buffer).  Needs dtype = MH_BF16, arch 0, d_model /
                               d_ff multiples of 128.  A reduced-precision mode of its own (the reference has none): gates
                               are error bounds against the fp32 reference goldens, never bit-exactness.                 */
  const MhOptionSet* options;   /* ABI 8: this engine's option overrides (mh_options_create), NULL = the process-wide values */
  /* --- ABI 10: arch 2 = stock HF Whisper ('openai/whisper-*': the V28 / V29 releases, configs/model/whisper_{base,small}.yaml;
   * transformers models/whisper/modeling_whisper.py): the wrapper's encoder_embedder (n_mels [+ cond] -> d, as arch 0) in front
   * of the conv front-end (C_in = d), + encoder.embed_positions; pre-norm blocks with AFFINE nn.LayerNorm (eps 1e-5; MhT5Weights
   * *_ln*_b), q / v / out projections with bias and k without (packed as arch 1: fused Wqkv / Wq + Wkv with a zero k-bias),
   * q scaled by 1 / 8, NO rotary embedding, fc1 -> gelu(erf) -> fc2, decoder input = decoder_embedder[id] +
   * decoder.embed_positions[position], final LayerNorm, proj_out.  in_frames / src_len as arch 1.                           */
  int dec_pos_from_mask;    /* arch 2: 0 = the position of column t is t (transformers 5.x: cache positions); 1 = t minus the
                               number of masked (padding) prompt columns of its row, clamped at 0 (transformers 4.57's
                               Whisper `prepare_inputs_for_generation`: decoder_position_ids = cumsum(mask) - 1; needs a
                               left-padded prompt mask)                                                                  */
} MhT5Config;

typedef struct MhT5Weights {
  const void* enc_embed_w;            /* [d, n_mels_pad]           modeling_mapperatorinator.py:123-124 */
  const float* enc_embed_b;           /* [d]                                                           */
  const void* dec_embed;              /* [vocab_in, d]             modeling_mapperatorinator.py:126-128 */
  const float* enc_rel_bias;          /* fp32 [H][2L-1]   bucketed lookup, encoder (bidirectional)      */
  const float* dec_rel_bias;          /* fp32 [H][tgt_len] lookup by distance q-k >= 0 (causal)         */
  /* encoder blocks */
  const float* enc_ln1[MH_MAX_LAYERS];   /* [d]  layer.0.layer_norm                                   */
  const void* enc_qkv[MH_MAX_LAYERS];    /* [3*inner, d]  q|k|v stacked                               */
  const void* enc_o[MH_MAX_LAYERS];      /* [d, inner]                                                */
  const float* enc_ln2[MH_MAX_LAYERS];   /* [d]  layer.1.layer_norm                                   */
  const void* enc_wi[MH_MAX_LAYERS];     /* [2*d_ff, d]  wi_0 / wi_1 interleaved in 16-row blocks     */
  const void* enc_wo[MH_MAX_LAYERS];     /* [d, d_ff]                                                 */
  const float* enc_final_ln;             /* [d]                                                       */
  /* decoder blocks */
  const float* dec_ln1[MH_MAX_LAYERS];
  const void* dec_qkv[MH_MAX_LAYERS];    /* [3*inner, d] self-attention                               */
  const void* dec_o[MH_MAX_LAYERS];
  const float* dec_ln2[MH_MAX_LAYERS];
  const void* dec_cq[MH_MAX_LAYERS];     /* [inner, d]  cross-attention query                         */
  const void* dec_ckv_all;               /* [n_dec*2*inner, d] rows ordered (layer, k|v, head, 64)    */
  const void* dec_co[MH_MAX_LAYERS];     /* [d, inner]                                                */
  const float* dec_ln3[MH_MAX_LAYERS];
  const void* dec_wi[MH_MAX_LAYERS];
  const void* dec_wo[MH_MAX_LAYERS];
  const float* dec_final_ln;
  const void* lm_head;                   /* [vocab_out, d]                                            */
  /* --- ABI 5, arch 1 only (all NULL for T5).  Matrix slots above are reused: *_qkv = fused Wqkv [3 d, d], *_o = Wo,
   * dec_cq = cross Wq, dec_ckv_all = the layers' cross Wkv stacked [n_dec * 2 d, d] (rows k | v per layer, head-major:
   * `kv.view(bs, -1, 2, H, 64)`, :544), dec_co = cross Wo, *_wi = fc1 [d_ff, d] (NOT interleaved), *_wo = fc2 [d, d_ff],
   * dec_embed = the wrapper's decoder_embedder, lm_head = proj_out, enc_ln1 / enc_ln2 = self_attn_layer_norm /
   * final_layer_norm, dec_ln1 / dec_ln2 / dec_ln3 = self_attn_ / cross_attn_ / final_layer_norm. ------------------- */
  const void* conv1_w; const float* conv1_b;      /* front-end, mh_whisper_frontend layout ([d, Kpad] tap-major)      */
  const void* conv2_w; const float* conv2_b;
  const float* enc_qkv_b[MH_MAX_LAYERS]; const float* enc_o_b[MH_MAX_LAYERS];     /* fp32, NULL = attention_bias false */
  const float* enc_fc1_b[MH_MAX_LAYERS]; const float* enc_fc2_b[MH_MAX_LAYERS];
  const float* dec_qkv_b[MH_MAX_LAYERS]; const float* dec_o_b[MH_MAX_LAYERS];
  const float* dec_cq_b[MH_MAX_LAYERS]; const float* dec_ckv_b_all;               /* [n_dec * 2 d]                     */
  const float* dec_co_b[MH_MAX_LAYERS];
  const float* dec_fc1_b[MH_MAX_LAYERS]; const float* dec_fc2_b[MH_MAX_LAYERS];
  /* rotary tables, fp32 [positions][64] = cos(32) | sin(32), built on the host by VarWhisperRotaryEmbedding's formulas
   * (:212-226) and rounded to the storage type there: encoder positions 0 .. src_len-1, decoder 0 .. tgt_len-1;
   * *_local = the same with local_rope_theta for local layers (may alias the global ones)                           */
  const float* enc_rope; const float* enc_rope_local; const float* dec_rope; const float* dec_rope_local;
  /* --- ABI 7, enc_operand_dtype = MH_MX8 only: the MX-fp8 copies (mh_quantize_mx8 layout: e4m3 [N][K] + scales
   * [N][mh_mx8_scale_row_bytes(K)]) of enc_qkv / enc_o / enc_wi (interleaved like enc_wi) / enc_wo / dec_ckv_all --------- */
  const uint8_t* enc_qkv_mx[MH_MAX_LAYERS]; const uint8_t* enc_qkv_mxs[MH_MAX_LAYERS];
  const uint8_t* enc_o_mx[MH_MAX_LAYERS]; const uint8_t* enc_o_mxs[MH_MAX_LAYERS];
  const uint8_t* enc_wi_mx[MH_MAX_LAYERS]; const uint8_t* enc_wi_mxs[MH_MAX_LAYERS];
  const uint8_t* enc_wo_mx[MH_MAX_LAYERS]; const uint8_t* enc_wo_mxs[MH_MAX_LAYERS];
  const uint8_t* dec_ckv_all_mx; const uint8_t* dec_ckv_all_mxs;
  /* --- ABI 10, arch 2 only: LayerNorm biases (fp32 [d]; the *_ln* slots above hold the LayerNorm weights) and the absolute
   * position tables -- encoder.embed_positions fp32 [src_len][d] (the fixed sinusoids, read from the state dict),
   * decoder.embed_positions fp32 [tgt_len][d] (learned) ------------------------------------------------------------------ */
  const float* enc_ln1_b[MH_MAX_LAYERS]; const float* enc_ln2_b[MH_MAX_LAYERS]; const float* enc_final_ln_b;
  const float* dec_ln1_b[MH_MAX_LAYERS]; const float* dec_ln2_b[MH_MAX_LAYERS]; const float* dec_ln3_b[MH_MAX_LAYERS];
  const float* dec_final_ln_b;
  const float* enc_pos; const float* dec_pos;
} MhT5Weights;

/* bytes of scratch needed by mh_t5_encode for a batch of B chunks */
int64_t mh_t5_encode_workspace_bytes(const MhT5Config* cfg, int B);

/* K2/K3/K4  mel -> encoder_embedder -> T5 encoder stack (final RMSNorm included).
 * Replaces OsuTEncoder.forward (modeling_mapperatorinator.py:392-443) + HF T5Stack (encoder).
 * mel    [B*L, n_mels_pad] element type cfg.dtype (output of mh_mel with ld_out = n_mels_pad);
 * enc_out[B*L, d] element type cfg.dtype (final-norm output, the cross-attention K/V GEMM operand);
 * enc_out_f32 optional fp32 copy [B*L, d] (NULL to skip) for parity checks. */
int mh_t5_encode(const MhT5Config* cfg, const MhT5Weights* w, const void* mel, int B, void* enc_out,
                 float* enc_out_f32, void* workspace, int64_t workspace_bytes, void* stream);
/* arch 1 (VarWhisperEncoder.forward, modeling_varwhisper.py:779-852): `mel` is [B * in_frames, n_mels_pad] log-mel
 * frames (mh_mel with the torchaudio parameterisation, log1p) -- the time-major transpose of HF's input_features --
 * and the same call runs conv1 + GELU, conv2 (stride 2) + GELU, the encoder layers (RMSNorm -> Wqkv -> RoPE ->
 * softmax(q k^T / 8) v -> Wo -> + ; RMSNorm -> fc1 -> GELU -> fc2 -> +) and the final RMSNorm; enc_out [B * src_len, d]. */

/* The same with the wrapper's conditioning embedders (difficulty / mapper style / song position / style:
 * modeling_mapperatorinator.py:395-414 -- per-row vectors repeated over the frames and concatenated to the mel frames in
 * front of encoder_embedder).  A vector that is constant along the frames only adds a constant to every frame of its
 * chunk: row_bias [B, d_model] fp32 = cond @ W[:, n_mels:]^T + b (computed by the caller; it REPLACES the bias of
 * encoder_embedder), NULL = mh_t5_encode. */
int mh_t5_encode_cond(const MhT5Config* cfg, const MhT5Weights* w, const void* mel, int B, const float* row_bias,
                      void* enc_out, float* enc_out_f32, void* workspace, int64_t workspace_bytes, void* stream);

/* Cross-attention K/V projection of all decoder layers at once (HF T5Attention with
 * key_value_states, computed once per chunk and kept in the encoder-side StaticCache:
 * osuT5/osuT5/inference/cache_utils.py:32-35).
 * cross_kv out: [n_dec][2][B][H][L][64] element type cfg.dtype. */
/* (ABI 7) the same with scratch for the MX-fp8 copy of enc_out when cfg->enc_operand_dtype = MH_MX8 (mh_t5_cross_kv refuses
 * that mode: it has nowhere to put the copy); workspace >= mh_t5_cross_kv_workspace_bytes(cfg, B) (0 for the plain modes). */
int64_t mh_t5_cross_kv_workspace_bytes(const MhT5Config* cfg, int B);
int mh_t5_cross_kv_ws(const MhT5Config* cfg, const MhT5Weights* w, const void* enc_out, int B, void* cross_kv, void* workspace,
                      int64_t workspace_bytes, void* stream);
int mh_t5_cross_kv(const MhT5Config* cfg, const MhT5Weights* w, const void* enc_out, int B,
                   void* cross_kv, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K5/K6  autoregressive decode.  Replaces HF GenerationMixin.generate/_sample as driven by
 * model_generate (osuT5/osuT5/inference/server.py:83-156) with MapperatorinatorCache
 * (cache_utils.py:7-35) and the reference logits processors
 * (osuT5/osuT5/inference/logit_processors.py:36-44,136-183; server.py:106-134).
 */
typedef struct MhSampling {
  int do_sample;            /* 0: greedy argmax (first maximal index)                          */
  int top_k;                /* >0: keep k best before sampling                                 */
  float top_p;              /* <1: nucleus                                                     */
  float temperature;        /* TemperatureLogitsWarper (server.py:131-132)                     */
  float timeshift_bias;     /* TimeshiftBias (logit_processors.py:36-44), 0 = off              */
  int ts_start, ts_end;     /* TIME_SHIFT id range [start, end)                                */
  int n_sos; int sos_ids[16];   /* sos + context_sos ids (MonotonicTimeShiftLogitsProcessor)   */
  int lookback_mask_end;    /* LookbackBiasLogitsWarper, types_first=False branch: ids in
                               [ts_start, lookback_mask_end) get -inf; <= ts_start disables     */
  int pad_id;
  int max_length;           /* prompt + new tokens cap (MaxLengthCriteria)                      */
  uint64_t seed;            /* Philox seed when do_sample                                       */
  /* --- ABI 2: the remaining processors of server.py:106-134 ----------------------------------- */
  float cfg_scale;          /* > 1: ClassifierFreeGuidanceLogitsProcessor (server.py:107-108).  The batch
                               holds 2G rows: rows [0, G) are fed the NEGATIVE prompt, rows [G, 2G) the
                               prompt (prepare_inputs_for_generation, modeling_mapperatorinator.py:243-254);
                               scores = l[G+g] + (l[g] - l[G+g]) * cfg_scale, exactly what HF's processor
                               computes on that row order; both rows of a pair receive the sampled id;
                               cross_kv then holds G rows (the encoder output is shared by the pair)      */
  int n_cond;               /* ConditionalTemperatureLogitsWarper (logit_processors.py:47-82): up to 3   */
  float cond_temp[3];       /*   (temperature, token set, offset) rules, first match wins; the token set */
  int cond_offset[3];       /*   of rule j is bit (2 << j) of tok_flags; the lookback is ROW 0's history */
  int lookback_types_first; /* LookbackBiasLogitsWarper types_first=True branch (:116-133) over
                               [ts_start, lookback_mask_end): renormalise instead of masking             */
  const uint8_t* tok_flags; /* device uint8 [vocab_out]: bit0 timed-event ids (:104-108), bits 1-3 the
                               conditional-temperature sets, bit4 eos + context-eos ids (:99).  May be
                               NULL when n_cond == 0 and lookback_types_first == 0                       */
  /* --- ABI 3 ------------------------------------------------------------------------------------ */
  int cond_per_row;         /* 0: the reference's batch behaviour -- ConditionalTemperatureLogitsWarper reads
                               `input_ids[0, -max_offset:]`, ROW 0's history, for every row of the batch
                               (logit_processors.py:75-80).  1: every row looks at its OWN history, i.e. what
                               the reference computes when each row is a batch-1 call (generate_sequential,
                               processor.py:308-368): used when rows of different songs / shards share a batch */
  unsigned rng_row0;        /* do_sample: global index of this call's first returned row in the RNG key
                               (seed, row, column), so shards of one job do not replay each other's draws  */
  /* --- ABI 4 ------------------------------------------------------------------------------------ */
  const void* cross_kv_fp8; /* NULL: the token steps stream `cross_kv` (cfg.dtype).  Non-NULL (bf16 storage only): the
                               packed OCP e4m3 copy written by mh_t5_quantize_cross_kv -- the token steps stream THAT
                               (half the HBM bytes of the dominant kernel; BASELINE configs[4]); the prompt prefill
                               still reads `cross_kv`.  Not a parity mode: K / V carry 3 mantissa bits.          */
} MhSampling;

int64_t mh_t5_decode_workspace_bytes(const MhT5Config* cfg, int B);

/* fp8 form of the cross-attention K/V (no reference counterpart; BASELINE configs[4] "fp8 ... KV-cached decode").
 * cross_kv  [n_dec][2][B][H][L][64] bf16 from mh_t5_cross_kv;
 * out       mh_t5_cross_kv_fp8_bytes(cfg, B) bytes: the same layout in OCP e4m3, one byte per element, followed (256-
 *           byte aligned) by fp32 scales [n_dec][2][B][H]: x ~ e4m3 * scale, scale = absmax of the (layer, k|v, row,
 *           head) slab / 448. */
int64_t mh_t5_cross_kv_fp8_bytes(const MhT5Config* cfg, int B);
int mh_t5_quantize_cross_kv(const MhT5Config* cfg, const void* cross_kv, int B, void* out, void* stream);

/* Runs prefill over the (left-padded) prompt and the AR loop until every row has emitted an id of
 * the EOS set or max_length is reached.
 *   prompt      int32 [B, P]    decoder_input_ids (pad_id = left padding)
 *   prompt_mask uint8 [B, P]    decoder_attention_mask (1 = attend), NULL = all ones
 *   eos_table   uint8 [vocab_out] 1 where the id is in get_eos_token_id(...) (server.py:72-80)
 *   cross_kv    from mh_t5_cross_kv
 *   tokens      int32 [B, max_length] out: prompt followed by generated ids, pad_id after EOS
 *   n_steps_out int32 [1] device: number of valid columns of `tokens` (= HF output length)
 *   logits_dump optional fp32 [max_length][B][vocab_out]: processed scores of every step (parity)
 *   forced      optional int32 [B, max_length]: teacher forcing -- when non-NULL the id appended at
 *               column c is forced[b][c] (argmax is still computed and written to `tokens`)
 * The loop is captured into a hipGraph per step shape and replayed; the host polls a device
 * "all finished" flag every `poll_every` steps (one 4-byte D2H on `stream`), otherwise no sync.
 * The token step (mh_t5_generate, mh_t5_step, mh_t5_cross_attn_probe) needs d_model a multiple of 128 in [128, 1024]:
 * other shapes return MH_ERR_ARG. */
int mh_t5_generate(const MhT5Config* cfg, const MhT5Weights* w, const void* cross_kv, int B,
                   const int32_t* prompt, const uint8_t* prompt_mask, int P, const uint8_t* eos_table,
                   const MhSampling* sp, int32_t* tokens, int32_t* n_steps_out, float* logits_dump,
                   const int32_t* forced, void* workspace, int64_t workspace_bytes, int poll_every,
                   void* stream);

/* e4m3 self-attention K/V cache for the token steps ("self_kv_fp8"; additive at ABI 11: symbols only, no struct changes layout; a
 * library without them is an older 11).  The other half of an fp8 K/V cache beside MhSampling.cross_kv_fp8; opt-in, not a parity mode.
 * Contract:
 *   - bf16 storage only (fp32: MH_ERR_ARG; the hosts refuse it before anything is encoded).
 *   - every cached self-attention key row and value row (64 elements of one layer, row, head, position) is held as 64 OCP e4m3 bytes
 *     plus one fp32 scale: scale = absmax / 448 (1 when the row is all zero), element = cvt_e4m3(x * (1 / scale)) -- the reciprocal-
 *     multiply form of mh_t5_quantize_cross_kv.
 *   - a token step at position `pos` attends the e4m3 rows of positions < pos (dequantised by their scales: the key scale multiplies
 *     the score before bias and mask, the value scale the probability), attends its OWN new key / value at storage precision as
 *     mh_t5_generate does, then appends that row in e4m3 with its scale.  The bf16 row is still written to the bf16 cache of the
 *     workspace, which stays valid for everything that reads it.
 *   - the batched prompt prefill is unchanged: positions 0 .. P-2 attend each other through the bf16 cache and are quantised in one
 *     pass before the first token step.  Under option decode_prefill = 0 every prompt position is a token step and behaves as the
 *     previous item says (so a prompt row attends its predecessors in e4m3 there).
 *   - rows stay batch-invariant: a row's logits do not depend on which rows share its call or its chain.
 * mh_t5_self_kv_fp8_bytes: bytes of the caller-owned shadow cache -- e4m3 [n_dec][2][B][H][tgt_len][64] followed, 256-byte aligned,
 *   by fp32 scales [n_dec][2][B][H][tgt_len] (0.53 x the bf16 cache, on top of it); -1 for fp32 storage.
 * mh_t5_generate_skv8: mh_t5_generate's arguments plus the shadow.  Composes with MhSampling.cross_kv_fp8, guidance (the doubled rows
 *   own their cache rows), sampling, forced ids and logits_dump.  The shadow need not be initialised and is rewritten by every call.
 * mh_quantize_kv_rows: the bulk quantiser on plain buffers -- x_bf16 [n_rows][64] bf16 -> q [n_rows][64] e4m3 bytes, scales [n_rows].
 * mh_t5_decode_self_cache: the bf16 self-attention caches [n_dec][B][H][tgt_len][64] inside a decode workspace of B rows.
 * Not built here: mh_t5_step / mh_t5_step_fp8 / mh_t5_reorder_cache (beam search over a copied cache) have no shadow-cache form --
 *   they take no shadow argument and always run over the bf16 cache; the hosts refuse self_kv_fp8 with num_beams > 1 over the copy
 *   cache.  Beam search over the INDEXED cache has one: mh_t5_step_indexed_skv8 and mh_t5_self_kv_fp8_fill, further down beside
 *   mh_t5_step_indexed. */
int64_t mh_t5_self_kv_fp8_bytes(const MhT5Config* cfg, int B);
int mh_t5_generate_skv8(const MhT5Config* cfg, const MhT5Weights* w, const void* cross_kv, int B,
                        const int32_t* prompt, const uint8_t* prompt_mask, int P, const uint8_t* eos_table,
                        const MhSampling* sp, int32_t* tokens, int32_t* n_steps_out, float* logits_dump,
                        const int32_t* forced, void* workspace, int64_t workspace_bytes, int poll_every,
                        void* stream, void* self_kv_fp8);
int mh_quantize_kv_rows(const void* x_bf16, int64_t n_rows, void* q, float* scales, void* stream);
int mh_t5_decode_self_cache(const MhT5Config* cfg, int B, void* workspace, void** k, void** v);

/* Row settings: the greedy / sampled decode with one MhRowSampling per RETURNED row, so that requests with different settings share
 * one call (additive at ABI 11: one struct, one symbol, mh_struct_size(8); MhSampling keeps its layout).  No reference counterpart:
 * the reference decodes one kwargs set per call; every row here computes what it computes in a uniform call (mh_t5_generate /
 * mh_t5_generate_skv8) made with its own settings, bit for bit -- token ids up to the row's end and its rows of logits_dump.
 * Contract:
 *   - per ROW, from rows[r] (r = index among the returned rows: the batch row, or the pair index under guidance):
 *       temperature; cond_temp[3] with cond_mask (bit j set: rule j of sp applies to this row.  A rule the reference drops for this
 *       row because its temperature equals the row's base one (logit_processors.py:62-67) has its bit CLEAR and is skipped -- first
 *       match wins, so it must not match with the base temperature); top_k; top_p; timeshift_bias; lookback_mask_end; max_length (the
 *       row finishes at its own cap and receives pad_id afterwards; `tokens` keeps the stride sp->max_length, the largest cap);
 *       eos_set (row of eos_tables); seed and rng_row (the draw stays uniform01(seed, rng_row, column): rng_row = rng_row0 + the
 *       row's index in the uniform call it is compared with); cfg_scale (the pair's scale under guidance).
 *   - per CALL, from sp as in mh_t5_generate: do_sample, guidance on / off (sp->cfg_scale > 1), ts_start / ts_end, sos_ids, n_cond,
 *     cond_offset, tok_flags (the token set of rule j is bit 2 << j for every row), lookback_types_first, pad_id, cond_per_row,
 *     cross_kv_fp8; max_length is the stride of `tokens` and the cap of the loop.  sp's per-row fields (temperature, cond_temp,
 *     top_k, top_p, timeshift_bias, lookback_mask_end, seed, rng_row0) and the `eos_table` argument are ignored.
 *   - rows       device, B entries (B / 2 under guidance); read by every token step: the CONTENTS may change between calls without
 *                a new step graph, the pointer is part of the graph's cache key (as eos_tables and n_eos_sets are: a caller who
 *                wants one graph for any mix keeps both buffers and passes the count of sets the buffer holds; the key holds
 *                sp->cfg_scale as on / off only, the scale being each pair's own)
 *     eos_tables device uint8 [n_eos_sets][vocab_out]
 *   - the library cannot read `rows` before the launch; the sampler clamps eos_set into [0, n_eos_sets) and max_length into
 *     [1, sp->max_length], so no entry can make it read or write out of bounds.  temperature and cond_temp must be > 0.
 *   - self_kv_fp8 may be NULL (mh_t5_generate) or the shadow of mh_t5_generate_skv8 (bf16 storage only, as there).
 *   - refused with MH_ERR_ARG and a message before any launch: NULL rows / eos_tables, n_eos_sets < 1, what mh_t5_generate(_skv8) refuse.
 * Not built: beams -- mh_t5_step / mh_beam_step have no row form; guided and unguided rows, or greedy and sampled rows, in one call. */
typedef struct MhRowSampling {
  float temperature;
  float cond_temp[3];
  int cond_mask;            /* 3 bits */
  int top_k;
  float top_p;
  float timeshift_bias;
  int lookback_mask_end;
  int max_length;
  int eos_set;
  unsigned rng_row;
  uint64_t seed;
  float cfg_scale;
  int reserved;             /* 0 (the entry is 64 bytes) */
} MhRowSampling;

int mh_t5_generate_rows(const MhT5Config* cfg, const MhT5Weights* w, const void* cross_kv, int B,
                        const int32_t* prompt, const uint8_t* prompt_mask, int P, const uint8_t* eos_table,
                        const MhSampling* sp, int32_t* tokens, int32_t* n_steps_out, float* logits_dump,
                        const int32_t* forced, void* workspace, int64_t workspace_bytes, int poll_every,
                        void* stream, void* self_kv_fp8, const MhRowSampling* rows, const uint8_t* eos_tables, int n_eos_sets);

/* In-flight decode: S slots, every slot a row that decodes a window of its OWN -- its own prompt, position, settings and end -- so
 * that a finished row's place goes to the next window while its neighbours keep stepping (additive at ABI 11: symbols only, the
 * session is an opaque handle, no struct).  No reference counterpart: the reference decodes one window per call.  Opt-in; the other
 * entries run the kernels, graphs and results they always did.
 * What a slot computes: the batch-1 call mh_t5_generate_rows(B = 1, the window's unpadded prompt and mask, rows[slot]) -- token ids
 *   up to the row's end and its rows of logits_dump, bit for bit (rows are batch-invariant).  The slot sits at its own columns
 *   0 .. n: no left padding, RoPE rows / learned positions / the relative bias are those of the row's own position.
 * Kernels: the token step of mh_t5_generate_rows with two kernels in their slot form (csrc/decode_self_attn.hpp, csrc/decode_sample.hpp): the
 *   self-attention reads the position of row b from an int32 [S] array (negative: the slot is idle and its workgroups return before
 *   they store anything), the sampler reads and advances that position, the row's prompt length, pos_off, the parity of its score
 *   history and its row of logits_dump; a row that is done writes its finish column, sets its flag and stops (no pad ids, the
 *   position moves no further).  The GEMVs, the fused tail and the cross-attention are row-independent and run as they are: an idle
 *   slot's rows of their outputs hold anything and are never read; its cross K/V row is still streamed.
 * Chains: mh_t5_decode_chains_cfg(cfg, S) static row blocks (slot s belongs to chain s / ceil(S / chains)), one control block and one
 *   captured step each, kept in the step-graph cache under a key that holds the slot arrays.
 * mh_t5_slots_workspace_bytes: bytes of the session's workspace (the decode workspace of S rows, the slot arrays, the prompt prefill
 *   of one row); -1 for S outside [1, 64].
 * mh_t5_slots_open: the caller owns, for the life of the session, cfg, w, and the device buffers
 *     rows            S MhRowSampling entries, read by every step: rows[slot] is the caller's to fill BEFORE admit(slot) and to
 *                     leave alone while the slot is live
 *     eos_tables      uint8 [n_eos_sets][vocab_out]
 *     cross_kv_slots  [n_dec][2][S][H][L][64] cfg.dtype: row `slot` is filled by admit
 *     tokens          int32 [S][sp->max_length]: row `slot` = the prompt, then the produced ids (nothing behind the row's end)
 *     logits_dump     optional fp32 [sp->max_length][S][vocab_out]
 *     workspace       mh_t5_slots_workspace_bytes(cfg, S) bytes
 *   sp: the per-call settings, read as in mh_t5_generate_rows (max_length = the stride of `tokens`).  `forced` and `self_kv_fp8` exist
 *   to be refused.  Refused with MH_ERR_ARG and a message before any launch: S outside [1, 64], sp->cfg_scale > 1 (guidance), forced
 *   ids, sp->cross_kv_fp8, a shadow cache, sp->n_cond > 0 with cond_per_row == 0, and whatever mh_t5_generate_rows refuses.
 *   `stream`: the work so far on it is what the session starts behind.  *handle: the session.
 * mh_t5_slots_admit: slot must be idle (MH_ERR_ARG otherwise).  On the session's admission stream, behind `stream` (the caller's
 *   work that wrote the arguments; may be NULL) and behind the slot's release: copies the window's compact cross K/V
 *   [n_dec][2][1][H][L][64] into the slot, the prompt (device int32 [P]) into tokens[slot], the mask (device uint8 [P], NULL = ones)
 *   into the slot's mask row; runs the batched prompt prefill with B = 1 into the slot's cache rows (positions 0 .. P-2; nothing under
 *   option decode_prefill = 0, where the prompt is fed token by token); then the one-row init.  Returns without waiting: cross_kv_row,
 *   prompt and prompt_mask must stay valid until the next mh_t5_slots_run returns.  The chain of the slot waits for the admission's
 *   event before the step that first sees the slot live; the other chain steps on.
 * mh_t5_slots_run: every chain with a live slot replays its step up to n_steps times (a poll every poll_every steps; it stops when
 *   no row of the chain is running), then ONE poll per chain returns, for every slot, finished_out[slot] (uint8, host) and
 *   length_out[slot] (int32, host: valid columns of tokens[slot] -- the finish column + 1 of a finished slot, the columns so far of a
 *   running one, 0 for an idle one); *steps_out (optional): graph replays of this call, summed over the chains.  The chains are idle
 *   when it returns.  The bounded hand-offs of the fused tail are reported as by mh_t5_generate (MH_ERR_DECODE_TAIL_TIMEOUT); their
 *   counters restart at zero with every call, so no session length can wrap them.  The early-stop poll happens between bursts of
 *   poll_every steps: a call of n_steps <= poll_every replays all its steps.
 * mh_t5_slots_release: the slot (live: MH_ERR_ARG otherwise; finished or not) becomes idle, on its chain's stream behind its last
 *   step; the caller reads tokens[slot] before it admits the next window there.
 * mh_t5_slots_close: joins the chains and the admissions, releases the graph references, frees the session.
 * Ordering is by events alone (release -> admit -> first step): nothing on the device spins or waits for another launch.  One host
 * thread per session.  Not built: beams, teacher forcing, several rows per admission; guidance pairs and the e4m3 caches are sessions
 * of their own (mh_t5_slots_open_guided, mh_t5_slots_open_kv8 below), not switches of this entry and not of a window. */
int64_t mh_t5_slots_workspace_bytes(const MhT5Config* cfg, int S);
int mh_t5_slots_open(const MhT5Config* cfg, const MhT5Weights* w, int S, const MhSampling* sp, const MhRowSampling* rows,
                     const uint8_t* eos_tables, int n_eos_sets, void* cross_kv_slots, int32_t* tokens, float* logits_dump,
                     const int32_t* forced, void* self_kv_fp8, void* workspace, int64_t workspace_bytes, int poll_every,
                     void* stream, void** handle);
int mh_t5_slots_admit(void* handle, int slot, const void* cross_kv_row, const int32_t* prompt, const uint8_t* prompt_mask, int P,
                      void* stream);
int mh_t5_slots_run(void* handle, int n_steps, uint8_t* finished_out, int32_t* length_out, int32_t* steps_out);
int mh_t5_slots_release(void* handle, int slot);
int mh_t5_slots_close(void* handle);

/* In-flight slots over the e4m3 K/V caches (additive at ABI 11: one symbol; the session stays an opaque handle, no struct changes
 * layout; a library without it is an older 11).  The argument list of mh_t5_slots_open, and the other mh_t5_slots_* entries serve the
 * session as they are.  The caches belong to the SESSION -- allocated once for all S slots, captured in every chain's step graph
 * (both pointers are in its key: a kv8 session and a plain one never share a graph) -- so no window can choose them.
 *   sp->cross_kv_fp8  non-NULL: the caller-owned e4m3 copy of the slots' cross K/V, mh_t5_cross_kv_fp8_bytes(cfg, S) bytes in the
 *                     layout of mh_t5_quantize_cross_kv(B = S).  It need not be initialised: every admission quantises its window's
 *                     compact row into row `slot` (bytes and scales equal mh_t5_quantize_cross_kv(B = 1) of that row; no other row is
 *                     written), and the token steps stream that row.
 *   self_kv_fp8       non-NULL: the caller-owned shadow of the self-attention cache, mh_t5_self_kv_fp8_bytes(cfg, S) bytes in the
 *                     layout of mh_t5_generate_skv8(B = S).  It need not be initialised: an admission quantises positions 0 .. P-2 of
 *                     the slot's prefilled cache rows into the same places (nothing under option decode_prefill = 0), every token
 *                     step appends its own row, and a row attends positions below its own only.
 *   cross_kv_slots    may be NULL where sp->cross_kv_fp8 is given: then the session holds no bf16 copy of the slots' cross K/V at all
 *                     (the admission's B = 1 prefill reads the caller's compact row).
 *   Either copy or both.  With neither, the entry is mh_t5_slots_open.
 * What a slot computes: the batch-1 call mh_t5_generate_rows(B = 1, the window's unpadded prompt and mask, rows[slot]) with the same
 *   modes -- sp->cross_kv_fp8 = mh_t5_quantize_cross_kv(B = 1) of the window's row and / or a shadow of its own -- token ids and rows
 *   of logits_dump, bit for bit; and the slot's rows of both copies hold, below the row's length, the bytes and scales of that call's.
 * Kernels: the self-attention in its F8 slot form (dec_slot_self_attn_kernel<.., F8>: keys below the row's own position from shadow
 *   row `slot` with their scales, its own key / value at storage precision, appended to the shadow by the same workgroup; an idle slot
 *   returns before any store), the cross-attention's e4m3 form as it is (row-independent), one row quantiser per admission.
 * Refused with MH_ERR_ARG and a message before any device call: fp32 storage with either copy, guidance, forced ids, n_cond > 0
 *   without cond_per_row, S outside [1, 64], cross_kv_slots == NULL without sp->cross_kv_fp8, and whatever mh_t5_generate_rows /
 *   mh_t5_generate_skv8 refuse.  mh_t5_slots_admit on such a session, on its admission stream, in this order: the bf16 copy into the
 *   slot (where a bf16 slot buffer exists), the row quantiser, prompt and mask, the B = 1 prefill, the shadow's prompt rows, the
 *   one-row init -- the position stays the last word an admission writes.
 * Memory: the bf16 slot copy is n_dec * 2 * S * H * L * 64 * 2 bytes, the e4m3 one half of that plus 4 bytes per (plane, slot, head);
 *   the shadow adds n_dec * 2 * S * H * tgt_len * 68 bytes beside the bf16 cache, which stays (the prefill and every append write it). */
int mh_t5_slots_open_kv8(const MhT5Config* cfg, const MhT5Weights* w, int S, const MhSampling* sp, const MhRowSampling* rows,
                         const uint8_t* eos_tables, int n_eos_sets, void* cross_kv_slots, int32_t* tokens, float* logits_dump,
                         const int32_t* forced, void* self_kv_fp8, void* workspace, int64_t workspace_bytes, int poll_every,
                         void* stream, void** handle);

/* In-flight slots under classifier-free guidance: a slot is a PAIR (additive at ABI 11: three symbols; the session stays an opaque
 * handle, no struct changes layout; a library without them is an older 11).  Every slot holds the negative-prompt row and the prompt
 * row of one window; the pair is admitted, stepped, finished and released together.  Opt-in: the entries above keep every refusal,
 * guidance included.  mh_t5_slots_run / _release / _close serve the session as they are.
 * What a slot computes: the batch-1 guided call mh_t5_generate_rows(B = 2, the two prompt rows [negative | prompt] -- the negative
 *   prompt over the first columns of a copy of the prompt, both rows under the prompt's mask --, one cross K/V row, one MhRowSampling
 *   entry with the pair's own cfg_scale, the same e4m3 modes): token ids up to the pair's end and the pair's row of logits_dump for
 *   every column it produced, bit for bit; under the e4m3 modes the slot's rows of both copies hold, below the row's length, the bytes
 *   and scales of that call's.
 * Layout: S pairs are 2 S decode rows in the row order of a guided call, slot s = rows s (negative) and S + s (prompt); kvB = S: row
 *   b streams cross K/V row b % S.  One chain, as every guided call runs (a pair spans both halves of the batch).
 * Kernels: the token step of the guided mh_t5_generate_rows with the slot self-attention as it is -- one position entry per decode
 *   row, equal within a pair -- and the sampler in its guided slot form (dec_sample_kernel<.., ROWS, SLOT, PAIR>,
 *   csrc/decode_sample.hpp): one workgroup per pair; it reads the pair's position and prompt length, returns when the pair is idle or
 *   done, guides with rows[slot].cfg_scale as uncond + (cond - uncond) * scale, writes the emitted id, the finished flags, the finish
 *   columns and the advanced position to both rows, embeds the next token for both rows (each with its own position offset, arch 2),
 *   and writes the pair's row of logits_dump; the last-arriving workgroup recounts the running rows over 2 S flags.
 * mh_t5_slots_guided_workspace_bytes: the decode workspace of 2 S rows, the slot arrays, the prompt prefill of one pair; -1 for S
 *   outside [1, 32] (a decode batch holds 64 rows).
 * mh_t5_slots_open_guided: the argument list of mh_t5_slots_open_kv8 with S = pairs and
 *     rows            S entries, one per pair, indexed by the slot (rows[slot].cfg_scale is the pair's scale)
 *     cross_kv_slots  [n_dec][2][S][H][L][64]: one row per pair; may be NULL where sp->cross_kv_fp8 is given
 *     tokens          int32 [2 S][sp->max_length], rows [negative | prompt]
 *     logits_dump     optional fp32 [sp->max_length][S][vocab_out]
 *     sp->cross_kv_fp8 / self_kv_fp8   as in mh_t5_slots_open_kv8: the e4m3 copy of S cross rows, the shadow of 2 S rows; bf16 storage
 *     workspace       mh_t5_slots_guided_workspace_bytes(cfg, S) bytes
 *   Requires sp->cfg_scale > 1: guidance on / off is the session's, the scale each pair's own, as in mh_t5_generate_rows.  Refused with
 *   MH_ERR_ARG and a message in its own name before any device call: sp->cfg_scale <= 1, forced ids, n_cond > 0 without cond_per_row,
 *   S outside [1, 32], and whatever mh_t5_slots_open / mh_t5_slots_open_kv8 refuse.
 * mh_t5_slots_admit_pair: prompt_pair = device int32 [2][P], the negative row first; prompt_mask = device uint8 [P] or NULL, shared
 *   by both rows.  Everything mh_t5_slots_admit does, for both rows: the prompt rows into tokens[slot] and tokens[S + slot], the mask
 *   into both mask rows; the cross K/V row copied and / or quantised ONCE; both rows' cache rows prefilled with positions 0 .. P-2
 *   (one B = 1 prefill per row over the same cross row, each run with the GEMM kernels of the B = 2 prefill so that the cache holds
 *   that call's bits; nothing under option decode_prefill = 0); the shadow's prompt rows quantised for both rows; the one-row init
 *   for both rows -- both positions are the last words written.  mh_t5_slots_admit on a guided session and mh_t5_slots_admit_pair
 *   on an unguided one are MH_ERR_ARG with a message; the session stays usable.
 * mh_t5_slots_run: finished_out / length_out keep S entries, one per pair, read from the prompt row.  mh_t5_slots_release: both rows
 *   of the pair become idle.
 * Not built: guided and unguided slots in one session, more than one chain (pairs cut into per-chain blocks), beams, teacher
 *   forcing, several pairs per admission, skipping an idle slot's cross K/V stream. */
int64_t mh_t5_slots_guided_workspace_bytes(const MhT5Config* cfg, int S);
int mh_t5_slots_open_guided(const MhT5Config* cfg, const MhT5Weights* w, int S, const MhSampling* sp, const MhRowSampling* rows,
                            const uint8_t* eos_tables, int n_eos_sets, void* cross_kv_slots, int32_t* tokens, float* logits_dump,
                            const int32_t* forced, void* self_kv_fp8, void* workspace, int64_t workspace_bytes, int poll_every,
                            void* stream, void** handle);
int mh_t5_slots_admit_pair(void* handle, int slot, const void* cross_kv_row, const int32_t* prompt_pair, const uint8_t* prompt_mask,
                           int P, void* stream);

/* (ABI 10) One beam-search step between two decoder positions as ONE kernel (csrc/beam.hip).  Replaces the per-step body of HF
 * `GenerationMixin._beam_search` (third-party, transformers >= 4.50's vectorised form) as the reference reaches it with
 * `num_beams > 1` (osuT5/osuT5/inference/processor.py:147,159; server.py:137; super_timing_generator.py:28 decodes with two beams):
 * log_softmax of the step's logits (mh_t5_step) -> [HF ClassifierFreeGuidanceLogitsProcessor on the reference's row order, rows
 * [negative | prompt]: modeling_mapperatorinator.py:243-254] -> the reference's processor list on log-probabilities (server.py:
 * 106-134; logit_processors.py:36-44,47-82,111-114,136-183) -> + running beam scores -> the K best continuations of every chunk
 * (sorted, ties by flat index) -> EOS / max_length split -> the next running beams -> merge of the finished hypotheses by score /
 * length ** penalty -> the early_stopping = False heuristic.  Greedy beams only (sp.do_sample = 0; beam-sample is
 * mh_beam_step_sample below).
 * State: G chunks x num_beams rows, int32 sequences [G][nb][max_length] (columns beyond the current length hold the fill value),
 * fp32 scores [G][nb], int32 beam-index trails [G][nb][max_length - P], finished flags [G][nb]; the kernel reads the *_in arrays
 * and writes the *_out arrays (the caller swaps them every step), `heuristic_open` [G] in place.  Outputs for the caller (G nb entries,
 * 2 G nb under guidance: the second half repeats the first, as `beam_idx.repeat(2)` does): `src` [G
 * nb] = the row each new running beam continues (the argument of mh_t5_reorder_cache: MapperatorinatorCache.reorder_cache,
 * inference/cache_utils.py:16-20), `last` [G nb] = the token each running beam is fed next, `flags` [G][3] = (heuristic still
 * open, every candidate hit EOS / max_length, every finished slot filled) from which the host forms HF's loop condition.
 * Limits: num_beams in 2 .. 8, K <= 8192, any V (num_beams V < 2^31), greedy beams, no types_first lookback renormalisation (that
 * is mh_beam_step_tf below, which carries the state it needs).  Two
 * kernels with the same contract and the same bits: where K <= 4096 and 4 num_beams V + 8 K' bytes (K' = K rounded up to a power of
 * two) fit 120 KB of LDS the scores live in LDS; otherwise the streaming kernel keeps the K candidates in LDS only and recomputes a
 * score from the logits in every pass (option "beam_step_path": 0 = that rule, 1 = the LDS kernel or MH_ERR_ARG, 2 = the streaming
 * kernel everywhere). */
typedef struct MhBeamStep {
  const float* logits;          /* [RE][V] fp32: RE = G nb rows, or 2 G nb under guidance ([negative rows | prompt rows]) */
  const uint8_t* eos_table;     /* [V] 1 = an EOS id (get_eos_token_id, server.py:72-80)                                    */
  int G, num_beams, V, P, max_length, K, cur_len;
  int cfg; float cfg_scale;     /* classifier-free guidance (sp.cfg_scale is not read)                                      */
  float length_penalty; int early_stopping;   /* 0 = False, 1 = True, 2 = "never"                                           */
  MhSampling sp;                /* ts_start / ts_end / sos_ids / timeshift_bias / temperature / cond_* / lookback_mask_end / tok_flags */
  const int32_t* run_in; const float* rs_in; const int32_t* rb_in;      /* running beams: sequences, scores, beam-index trail */
  const int32_t* seq_in; const float* bs_in; const int32_t* bb_in; const uint8_t* fin_in;   /* finished set                 */
  int32_t* run_out; float* rs_out; int32_t* rb_out;
  int32_t* seq_out; float* bs_out; int32_t* bb_out; uint8_t* fin_out;
  uint8_t* heuristic_open;      /* [G] in place                                                                              */
  int32_t* src; int32_t* last; int32_t* flags;
} MhBeamStep;
int64_t mh_beam_step_lds_bytes(int num_beams, int V);
int mh_beam_step(const MhBeamStep* bs, void* stream);
/* Which kernel mh_beam_step runs for this shape under the current "beam_step_path": 0 = refused (a limit above), 1 = LDS kernel, 2 =
 * streaming kernel.  Additive at ABI 11 (one symbol, one option; no struct changes layout): a library without it is an older 11. */
int mh_beam_step_path(int num_beams, int V, int K);
/* mh_beam_step with the types_first branch of LookbackBiasLogitsWarper (logit_processors.py:116-133; sp.lookback_types_first = 1 and
 * sp.lookback_mask_end > sp.ts_start, which mh_beam_step refuses).  Per beam row, x = the scores that ENTER the processor (log_softmax
 * -> guidance -> MonotonicTimeShift -> TimeshiftBias -> temperature):
 *   the row renormalises iff its last id is a timed event (bit 0 of tok_flags; an id >= V is not timed) and its slot of
 *   `lookback_prev` is >= 0:  prob_eos = lookback_prev[slot], prob_event = 1 - prob_eos, s = 1 / (softmax(x)[ids outside [ts_start,
 *   lookback_mask_end)].sum() prob_event + prob_eos); ids in [ts_start, lookback_mask_end) get -inf except ts_start, which gets
 *   log(clip((s - 1) prob_eos / prob_event, 0, 1)); every other id gets log(softmax(x) s).  Any other row passes x through -- this
 *   branch does NOT mask;
 *   afterwards lookback_prev[slot] = softmax(x)[bit-4 ids of tok_flags (eos + context eos)].sum(), renormalised or not.
 * `lookback_prev`: device fp32 [G num_beams], one value per row SLOT, updated in place; the caller fills it with a negative value
 * ("no previous call") before the first step and does NOT gather it by `src`: the reference's `last_scores` is indexed by the row
 * slot of the previous step and never sees HF's beam reordering (reproduced verbatim).  A workgroup touches its own chunk's slots only.
 * Everything else -- limits, messages, the two kernels and their dispatch rule ("beam_step_path"), same bits from both -- is
 * mh_beam_step's; with the types_first lookback off the call IS mh_beam_step (lookback_prev may then be NULL).  tok_flags must be
 * set.  Additive at ABI 11 (one symbol; no struct changes layout). */
int mh_beam_step_tf(const MhBeamStep* bs, float* lookback_prev, void* stream);
/* Beam-SAMPLE (HF `_beam_search` with do_sample, which the reference's defaults give whenever num_beams > 1: configs/inference/
 * default.yaml do_sample / top_p, processor.py:147-161): mh_beam_step_tf with the K continuations of a chunk DRAWN inside the kernel.
 * Requires bs->sp.do_sample = 1 and reads sp.top_k, sp.top_p, sp.seed and sp.rng_row0 beside what mh_beam_step reads.  Per beam row,
 * x = the processed score in front of the running score (log_softmax -> guidance -> the processor list, lookback included):
 *   TopK (sp.top_k > 0): k' = min(max(top_k, min_tokens_to_keep), V); ids with x < the k'-th largest x are removed.  Exact; ties at
 *     the threshold stay, as in HF.
 *   TopP (sp.top_p < 1): p = softmax(x) over what TopK left; an id is removed iff the summed p of all ids with value <= its own is
 *     <= 1 - top_p and it is not among the min_tokens_to_keep largest.  HF may split a group of exactly equal values at the boundary
 *     by its sort order; here such a group stays or goes WHOLE.  The sums are deterministic: every numerator is taken in fixed point,
 *     (uint64) (exp(x - max x) 2^32), and added with 64-bit integer adds in LDS, so two launches, and the two kernels, agree bit for
 *     bit; the threshold is (uint64) ((1.0 - (double) top_p) x the row's integer total).
 *   Both leave the row ONE cut value; the accumulated score is acc = x >= cut ? x + running score : -inf (a dead beam's -1e9 running
 *   score enters behind the warpers and cannot collapse its row into ties).
 * The draw is Gumbel top-K: key = acc + g, g = -log(-log(u)) in fp32, u = min(uniform01(m, 0, flat), 1 - 2^-24) with uniform01 the
 * sampler's counter-based generator (splitmix64 finaliser; (n + 0.5) / 2^24 of the top 24 bits), m = the 64-bit word that generator
 * mixes from (sp.seed, row = sp.rng_row0 + chunk, step = bs->cur_len), flat = beam x V + id.  The K largest keys, best first, ties
 * by ascending flat index, ARE the draw, in draw order (the descending order of Gumbel-perturbed scores is distributed as sequential
 * sampling without replacement from softmax(acc); torch.multinomial runs the same race).  Each drawn candidate carries its acc (read
 * back or recomputed, not key - g); "inside the top num_beams" means the first num_beams draws, and the EOS split, next-beam choice,
 * finished-set merge, heuristic and flags are mh_beam_step's.  A -inf score has a -inf key: it is drawn only when the finite ones run
 * out, then in flat-index order (HF leaves this case undefined).  Chunk g of a call draws what a one-chunk call with rng_row0 + g draws.
 * `lookback_prev`: as in mh_beam_step_tf; may be NULL with the types_first lookback off.  `min_tokens_to_keep` >= 1 (HF passes #eos +
 * 1 under beams).  `scores_dump`: NULL or device fp32 [G][num_beams][V], acc of every id (-inf where removed) -- the parity hook.
 * MH_ERR_ARG before any launch, naming the value: do_sample = 0, min_tokens_to_keep < 1, top_p outside (0, 1], top_k < 0, and every
 * limit of mh_beam_step in its wording.  Same two kernels, dispatch rule and bit equality between them as mh_beam_step.  Additive at
 * ABI 11 (one symbol; no struct, no struct-size entry). */
int mh_beam_step_sample(const MhBeamStep* bs, float* lookback_prev, int min_tokens_to_keep, float* scores_dump, void* stream);

/* Step-wise decode for host-driven search.  Replaces the per-position `self(**model_inputs)` of HF
 * `GenerationMixin._beam_search` (num_beams > 1: osuT5/osuT5/inference/processor.py:147,159; server.py:137) and
 * `MapperatorinatorCache.reorder_cache` (osuT5/osuT5/inference/cache_utils.py:16-20).
 *   mh_t5_step: feeds ids[b] (device int32 [B]) at position `pos` to the decoder (self K/V appended at `pos`) and writes the
 *     RAW logits fp32 [B, vocab_out] -- no processors, no selection.  Rows are (chunk, beam) pairs, kv_group beams per
 *     chunk: row b reads cross K/V row b / kv_group (cross_kv holds B / kv_group rows).  prompt_mask uint8 [B, P] as in
 *     mh_t5_generate (NULL = ones).  `workspace` = mh_t5_decode_workspace_bytes(cfg, B) bytes, owned by the caller and kept
 *     between calls: it holds the self-attention caches.
 *   mh_t5_reorder_cache: cache rows b <- src[b] (device int32 [B]) for positions 0 .. n_pos-1 of every layer;
 *     scratch = mh_t5_reorder_cache_scratch_bytes(cfg, B, n_pos) bytes. */
int mh_t5_step(const MhT5Config* cfg, const MhT5Weights* w, const void* cross_kv, int B, int kv_group, const int32_t* ids,
               int pos, const uint8_t* prompt_mask, int P, float* logits, void* workspace, int64_t workspace_bytes,
               void* stream);
/* mh_t5_step over the e4m3 copy of the cross K/V (additive at ABI 11: one symbol, no struct changes layout).  `cross_kv_fp8` = the
 * packed copy mh_t5_quantize_cross_kv made of `cross_kv` (mh_t5_cross_kv_fp8_bytes(cfg, B / kv_group) bytes: it holds the same
 * B / kv_group rows); every cross-attention of the step streams it instead of `cross_kv`, row b with the scales of K/V row
 * b / kv_group.  Every other argument, the workspace and the logits are mh_t5_step's; the two entries may be mixed over one workspace
 * (the self-attention caches do not depend on the copy).  bf16 storage only (fp32: MH_ERR_ARG), every arch.  Not a parity mode: the
 * logits are those of K/V rounded to e4m3 with one fp32 scale per (layer, k|v, row, head). */
int mh_t5_step_fp8(const MhT5Config* cfg, const MhT5Weights* w, const void* cross_kv, const void* cross_kv_fp8, int B, int kv_group,
                   const int32_t* ids, int pos, const uint8_t* prompt_mask, int P, float* logits, void* workspace,
                   int64_t workspace_bytes, void* stream);
int64_t mh_t5_reorder_cache_scratch_bytes(const MhT5Config* cfg, int B, int n_pos);
int mh_t5_reorder_cache(const MhT5Config* cfg, int B, const int32_t* src, int n_pos, void* workspace, int64_t workspace_bytes,
                        void* scratch, int64_t scratch_bytes, void* stream);

/* Beam search without cache copies (additive at ABI 11: five symbols, plain arguments, no struct).  What
 * `MapperatorinatorCache.reorder_cache` (osuT5/osuT5/inference/cache_utils.py:16-20) does by copying whole cache rows is done by
 * index: `origin`, device uint8 [B][tgt_len] (mh_t5_beam_index_bytes(cfg, B) bytes), names per decode row b and position j the cache
 * row that holds that key / value.  A step writes position `pos` of cache row b and nothing else, so every (cache row, position) is
 * written exactly once and an entry never goes stale.  tgt_len <= 2560 (one row's entries are staged in LDS), B <= 64.
 *   mh_t5_step_indexed: mh_t5_step (cross_kv_fp8 NULL) or mh_t5_step_fp8 (cross_kv_fp8 = the packed copy) whose self-attention
 *     reads cached row j < pos of decode row b from cache row origin[b][j] and writes its new row to cache row b.  Bias, masks,
 *     window and the order of every sum are those of row b: with tables kept by mh_t5_reorder_index the logits are bit-identical to
 *     mh_t5_step + mh_t5_reorder_cache.  Entries are clamped to [0, B).  Its e4m3 self-cache form is mh_t5_step_indexed_skv8 (below).
 *   mh_t5_beam_index_init: origin[b][j] = b / kv_group for j < n_prefilled (the prompt rows of mh_t5_step_prefill), b beyond;
 *     n_prefilled = 0 is the identity table.
 *   mh_t5_reorder_index: origin_out[b][j] = origin_in[src[b]][j] for j < n_pos, b beyond -- `reorder_cache(beam_idx)` on the table;
 *     src device int32 [B] may repeat rows and, under guidance, point second-half rows into the first half (`beam_idx.repeat(2)`).
 *     origin_in != origin_out: the caller ping-pongs two tables.  One launch writing B x tgt_len bytes; no scratch.
 *   mh_t5_step_prefill: positions 0 .. n_pos-1 (n_pos <= P, the row stride of prompt int32 [Bp][P] / prompt_mask uint8 [Bp][P] or
 *     NULL) of Bp prompts go through the decoder at once -- HF's batched prefill, the one mh_t5_generate runs -- into cache rows
 *     0 .. Bp-1 of the self-attention caches of a B-row step workspace (mh_t5_decode_workspace_bytes(cfg, B), which includes the
 *     prefill's region).  cross_kv has Bp rows; B must be whole groups over the Bp prompts.  Follow it with
 *     mh_t5_beam_index_init(cfg, B, B / Bp, n_pos, ...) and step from position n_pos.
 * Every entry returns MH_ERR_ARG with a message before any launch for a null pointer, a pos / n_pos / n_prefilled outside the cache,
 * rows that are not whole groups, and fp32 storage together with the e4m3 copy. */
int64_t mh_t5_beam_index_bytes(const MhT5Config* cfg, int B);
int mh_t5_beam_index_init(const MhT5Config* cfg, int B, int kv_group, int n_prefilled, void* origin, void* stream);
int mh_t5_reorder_index(const MhT5Config* cfg, int B, const int32_t* src, int n_pos, const void* origin_in, void* origin_out,
                        void* stream);
int mh_t5_step_indexed(const MhT5Config* cfg, const MhT5Weights* w, const void* cross_kv, const void* cross_kv_fp8, int B,
                       int kv_group, const int32_t* ids, int pos, const uint8_t* prompt_mask, int P, float* logits, void* workspace,
                       int64_t workspace_bytes, const void* origin, void* stream);
int mh_t5_step_prefill(const MhT5Config* cfg, const MhT5Weights* w, const void* cross_kv, int Bp, const int32_t* prompt,
                       const uint8_t* prompt_mask, int P, int n_pos, void* workspace, int64_t workspace_bytes, int B, void* stream);

/* The e4m3 self-attention cache under the index table ("self_kv_fp8" with beam_cache = "indexed"; additive at ABI 11: two symbols,
 * no struct changes layout).  `self_kv_fp8` is the caller-owned shadow of mh_t5_self_kv_fp8_bytes(cfg, B) bytes in the layout written
 * there (e4m3 [n_dec][2][B][H][tgt_len][64], then 256-byte aligned fp32 scales [n_dec][2][B][H][tgt_len]): 0.53 x the bf16 cache, on
 * top of it.  Nothing is ever copied, so the shadow rows and their scales stay where their step wrote them and are read through the
 * same table as the bf16 rows would be.  bf16 storage only, tgt_len <= 2560, B <= 64.
 * Contract:
 *   - mh_t5_step_indexed_skv8: mh_t5_step_indexed's arguments with the shadow between `origin` and `stream` (cross_kv_fp8 NULL or
 *     the packed copy).  The step at `pos` of decode row b attends, for j < pos, the 64 e4m3 bytes of shadow row origin[b][j] (head,
 *     position j) with THAT row's two scales -- the key scale multiplies the score before bias and mask, the value scale the
 *     probability before the accumulate -- attends its own new key / value at storage precision, writes the bf16 row to bf16 cache
 *     row b at `pos` and appends the quantised row and its scale to shadow row b at `pos`, never to an origin row: every (shadow row,
 *     position) is written exactly once and an entry never goes stale.  Bias, prompt mask, window, RoPE and the order of every sum
 *     are those of decode row b.  With the identity table the caches, the shadow and the logits are those of mh_t5_generate_skv8's
 *     token steps.
 *   - mh_t5_self_kv_fp8_fill: after mh_t5_step_prefill (n_rows = Bp, the same n_pos): positions 0 .. n_pos-1 of cache rows
 *     0 .. n_rows-1 of the bf16 self-attention caches inside the B-row step workspace, every layer, k and v, are quantised into the
 *     same places of the B-row shadow by the rule the step's append uses.  Nothing else of the shadow is written.  The prompt
 *     positions attended each other through the bf16 cache, as in mh_t5_generate_skv8.
 *   - rows stay batch-invariant: a row's logits do not depend on which rows share its call (a scale belongs to one cached row).
 *   - mh_t5_step, mh_t5_step_fp8 and mh_t5_reorder_cache still have no shadow form; the shadow need not be initialised.
 * Both return MH_ERR_ARG with a message naming the entry, before any launch, for a null pointer, fp32 storage, tgt_len > 2560, B
 * outside [1, 64], rows that are not whole groups, pos / n_pos outside the cache, n_rows outside [1, B] and a workspace that is too
 * small. */
int mh_t5_step_indexed_skv8(const MhT5Config* cfg, const MhT5Weights* w, const void* cross_kv, const void* cross_kv_fp8, int B,
                            int kv_group, const int32_t* ids, int pos, const uint8_t* prompt_mask, int P, float* logits,
                            void* workspace, int64_t workspace_bytes, const void* origin, void* self_kv_fp8, void* stream);
int mh_t5_self_kv_fp8_fill(const MhT5Config* cfg, int B, int n_rows, int n_pos, void* workspace, int64_t workspace_bytes,
                           void* self_kv_fp8, void* stream);

/* Teacher-forced decoder forward over whole sequences: `Mapperatorinator.forward` with `encoder_outputs` given
 * (seam B2, osuT5/osuT5/model/modeling_mapperatorinator.py:174-228; used by server.py:160-181 `model_forward`).
 *   ids  int32 [B, T] decoder_input_ids, mask uint8 [B, T] decoder_attention_mask (NULL = ones), T <= tgt_len
 *   logits fp32 [B, T, vocab_out]: lm_head(final RMSNorm(decoder(ids)))  -- no processors, no sampling */
int64_t mh_t5_forward_workspace_bytes(const MhT5Config* cfg, int B, int T);
int mh_t5_decoder_forward(const MhT5Config* cfg, const MhT5Weights* w, const void* cross_kv, int B,
                          const int32_t* ids, const uint8_t* mask, int T, float* logits, void* workspace,
                          int64_t workspace_bytes, void* stream);

/* ABI 11: teacher-forced SCORING on the device -- what MaiMod (`Processor.ai_mod`, osuT5/osuT5/inference/processor.py:421-579)
 * computes on the host from the logits `model_forward` (osuT5/osuT5/inference/server.py:159-181) copied to it:
 *     probs = softmax(logits)                                   processor.py:519
 *     entropy   = -sum(probs * log2(probs + 1e-10))             :520      (bits)
 *     surprisal = -log2(probs[target] + 1e-10)                  :521      (bits)
 *     relative  = surprisal / entropy where entropy > 0, else 0 :522
 *     best_id   = argmax(logits), lowest index on ties          :525
 *   and logprob = log_softmax(logits)[target] (natural log, no epsilon).
 * mh_score_rows: logits fp32 [R rows, V columns] with `row_stride` floats between rows (>= V), target int32 [R]; the four
 *   float outputs and best_id are [R].  A row whose target is negative or >= V is NOT SCORED: its floats are 0, its best_id
 *   is -1, its logits are not read.  Sums run in a fixed order: two calls on the same input agree bit for bit.
 * mh_t5_score: the decoder stack of mh_t5_decoder_forward (same ids / mask / cross_kv / T contract), then final norm, lm_head
 *   and the row statistics for the positions whose targets[b, t] is in [0, vocab_out) only -- every other position is written
 *   as not scored.  targets int32 [B, T]; outputs [B, T].  The scored positions are compacted on the device and go through the
 *   lm_head `score_block_rows` (option, MH_SCORE_BLOCK_ROWS, default 1024) at a time: the workspace exceeds the forward's by
 *   block * (vocab_out + d_model) * 4 + O(B T) bytes, B*T*vocab_out logits are never held.  A position's numbers are bit for bit
 *   those of mh_score_rows on mh_t5_decoder_forward's logits, whatever the block size.
 *   max_scored (an argument beyond the reference's call: the lm_head blocks are launched by the host, which cannot see a count
 *   made on the device): an upper bound of the number of scored positions, if the caller knows one (it has the targets on the
 *   host), so that no lm_head block is launched for positions that cannot exist; 0 = none (the outputs are only filled);
 *   negative = unknown, up to B*T.  Scored positions behind the bound (in row-major (b, t) order) would be left as not scored:
 *   pass the exact count or a negative value. */
int mh_score_rows(const float* logits, int64_t row_stride, int R, int V, const int32_t* target, float* surprisal,
                  float* entropy, float* relative, float* logprob, int32_t* best_id, void* stream);
int64_t mh_t5_score_workspace_bytes(const MhT5Config* cfg, int B, int T);
int mh_t5_score(const MhT5Config* cfg, const MhT5Weights* w, const void* cross_kv, int B, const int32_t* ids,
                const uint8_t* mask, int T, const int32_t* targets, int max_scored, float* surprisal, float* entropy,
                float* relative, float* logprob, int32_t* best_id, void* workspace, int64_t workspace_bytes, void* stream);

/* Measurement hook (bench.py `roofline`): launches the dominant decode kernel -- cross-attention over
 * the encoder keys, algorithmic bytes per launch = B*H*src_len*64*2*sizeof(elem) -- `reps` times
 * back to back between two HIP events on `stream`, cycling through the decoder layers as a decode
 * step does: the kernel the decode step really launches (the cross-attention that also projects its own query from
 * the residual row), so `w` is required (NULL: MH_ERR_ARG).
 * ms_out (HOST float[1]) = average milliseconds per launch.  Synchronises `stream`. */
int mh_t5_cross_attn_probe(const MhT5Config* cfg, const MhT5Weights* w, const void* cross_kv, int B, int reps,
                           float* ms_out, void* workspace, int64_t workspace_bytes, void* stream);

/* Measurement hook (bench.py `roofline`, in situ): with `buf` set, every cross-attention launch of the following
 * mh_t5_generate calls records (earliest workgroup start, latest workgroup end) in wall-clock ticks
 * (hipDeviceAttributeWallClockRate, kHz) into buf[chain][pos][layer][2] for decode positions pos < ring (device uint64,
 * pre-filled by the caller with (UINT64_MAX, 0)): the duration of the kernel exactly as the decode step launches it -- rows of one chain per
 * launch, the other chain's kernels running beside it.  Two atomics per workgroup: use an extra decode pass, not a
 * timed one.  buf == NULL (ring 0) switches it off.  mh_t5_decode_chains(B) = row chains mh_t5_generate uses for B. */
int mh_t5_decode_timing(void* buf, int ring);
int mh_t5_decode_chains(int B);
/* The status mh_t5_generate returns for the error word the decode step leaves in its workspace: 0 -> MH_OK, anything else ->
 * MH_ERR_DECODE_TAIL_TIMEOUT with mh_last_error() set (a hand-off of the fused layer tail waited more than 2 ms and gave up). */
int mh_t5_decode_tail_status(int err_word);
/* Fused layer-tail launches enqueued by this process so far (a node of a captured step graph counts once, when it is captured):
 * a shape that option "decode_fused_tail" = 1 does not cover runs the three launches and leaves this count unchanged. */
long mh_t5_decode_tail_launches(void);
int mh_t5_decode_chains_cfg(const MhT5Config* cfg, int B);   /* ABI 8: ... under cfg->options */
/* ABI 8: instantiated step graphs are kept across mh_t5_generate calls (option "decode_graph_cache", default 1: LRU of 16, a
 * call replays an earlier call's graph iff every address, size, sampling field other than seed / rng_row0, option value and the
 * weights struct agree byte for byte).  Counters of graphs replayed from / captured into the cache since the last reset. */
int mh_t5_step_graph_cache_stats(long* hits, long* misses, int reset);
int mh_wall_clock_khz(void);
/* Test aid: the kernels' cross-lane reductions run on the VALU (DPP row exchanges and the gfx950 row / half swaps, csrc/common.hpp)
 * instead of through the LDS crossbar; this applies each of those helpers and the shuffle form it replaced to the same input in one
 * kernel.  in: n_waves * 64 raw 32-bit patterns, one wave per 64; out_new / out_ref: [16][n_waves * 64] -- cases 0 wave sum, 1 wave
 * max, 2-4 sums over groups of 8 / 16 / 64 lanes, 5-7 their maxima, 8 / 9 sum / max over lanes 8, 16, 32 apart (the attention merge),
 * 10-15 the bare exchange with lane ^ 1, 2, 4, 8, 16, 32.  The two outputs must agree bit for bit. */
int mh_debug_lane_reduce(const uint32_t* in, int64_t n_waves, uint32_t* out_new, uint32_t* out_ref, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K7/K8/K9  osu_diffusion DiT + DDPM.  Replaces DiT.forward_with_cfg
 * (osu_diffusion/utils/models.py:281-317) and GaussianDiffusion.p_sample
 * (osu_diffusion/utils/diffusion/gaussian_diffusion.py:273-369, 420-467).  fp32 like the reference (it never
 * casts the DiT: inference.py:637-642) by default; operand_dtype = MH_BF16 is the reduced-precision mode of BASELINE
 * configs[4]: the four projections of every block take bf16 operands (weights stored bf16; LayerNorm-modulate, q / k / v,
 * the attention output and the GELU hidden are rounded to bf16 where they become a GEMM operand), one bf16 MFMA pass
 * with fp32 accumulation; the residual stream, LayerNorm, softmax, the adaLN conditioning, the first and the final
 * layer and the DDPM update stay fp32.  Parity of that mode is an error bound against the fp32 reference golden.
 */
typedef struct MhDiTConfig {
  int hidden, depth, n_heads, context_size, class_size, in_channels; /* in_channels = 2 */
  int freq_dim;      /* FirstLayer frequency_embedding_size = 128                        */
  int t_freq_dim;    /* TimestepEmbedder frequency_embedding_size = 256                  */
  int first_k_pad;   /* padded K of the first layer GEMM (in_channels*freq_dim+context)  */
  int class_pad;     /* padded K of y_embedder[0]                                        */
  int operand_dtype; /* MH_F32 (reference semantics), MH_BF16 (block GEMM operands, see above) or -- ABI 7, BASELINE configs[4]
                        "fp8 MFMA" -- MH_MX8: the four block projections on MX-fp8 operands (LayerNorm-modulate writes the operand
                        directly; attention output and GELU hidden are bf16 as in the MH_BF16 mode and quantised by a pass of their
                        own; attention itself on bf16 operands); hidden %% 128 == 0.  Error-bound gates, as MH_BF16. */
  const MhOptionSet* options;   /* ABI 8: this engine's option overrides, NULL = the process-wide values */
} MhDiTConfig;

typedef struct MhDiTWeights {       /* all fp32, matrices [N][Kpad]                                  */
  const float* pos_freqs;   /* [freq_dim/2]   exp(-ln(1e4) i / (freq_dim/2)), host-built exactly as     */
  const float* t_freqs;     /* [t_freq_dim/2] timestep_embedding does (positional_embedding.py:38-43)   */
  const float* first_w; const float* first_b;        /* context_embedder.mlp[0]  models.py:194-201  */
  const float* t_w0; const float* t_b0; const float* t_w1; const float* t_b1;   /* t_embedder.mlp   */
  const float* y_w0; const float* y_b0; const float* y_w1; const float* y_b1;   /* y_embedder       */
  const float* ada_w[MH_MAX_LAYERS]; const float* ada_b[MH_MAX_LAYERS];   /* [6D, D]               */
  const float* qkv_w[MH_MAX_LAYERS]; const float* qkv_b[MH_MAX_LAYERS];   /* attn.in_proj [3D, D]  */
  const float* out_w[MH_MAX_LAYERS]; const float* out_b[MH_MAX_LAYERS];   /* attn.out_proj         */
  const float* fc1_w[MH_MAX_LAYERS]; const float* fc1_b[MH_MAX_LAYERS];   /* mlp.fc1 [4D, D]       */
  const float* fc2_w[MH_MAX_LAYERS]; const float* fc2_b[MH_MAX_LAYERS];   /* mlp.fc2 [D, 4D]       */
  const float* fin_ada_w; const float* fin_ada_b;    /* final_layer.adaLN_modulation [2D, D]       */
  const float* fin_w; const float* fin_b;            /* final_layer.linear [4, D]                  */
  /* optional pre-split copies (MhGemm.w_split3 layout) of the five big projections; NULL = exact fp32 only.  Used for
   * denoiser batches of at least `dit_split3_min_rows` rows (option, default 2048 = 8 chunks of 128 points). */
  const void* first_w3;
  const void* qkv_w3[MH_MAX_LAYERS]; const void* out_w3[MH_MAX_LAYERS];
  const void* fc1_w3[MH_MAX_LAYERS]; const void* fc2_w3[MH_MAX_LAYERS];
  /* bf16 copies [N][K] of the four block projections; required when operand_dtype = MH_BF16 */
  const void* qkv_wb[MH_MAX_LAYERS]; const void* out_wb[MH_MAX_LAYERS];
  const void* fc1_wb[MH_MAX_LAYERS]; const void* fc2_wb[MH_MAX_LAYERS];
  /* (ABI 7) MX-fp8 copies of the four block projections (mh_quantize_mx8 layout: e4m3 [N][K] | scales [N][mh_mx8_scale_row_bytes(K)]);
   * required when operand_dtype = MH_MX8 */
  const uint8_t* qkv_wm[MH_MAX_LAYERS]; const uint8_t* qkv_wms[MH_MAX_LAYERS];
  const uint8_t* out_wm[MH_MAX_LAYERS]; const uint8_t* out_wms[MH_MAX_LAYERS];
  const uint8_t* fc1_wm[MH_MAX_LAYERS]; const uint8_t* fc1_wms[MH_MAX_LAYERS];
  const uint8_t* fc2_wm[MH_MAX_LAYERS]; const uint8_t* fc2_wms[MH_MAX_LAYERS];
} MhDiTWeights;

int64_t mh_dit_workspace_bytes(const MhDiTConfig* cfg, int N, int T);

/* One denoiser evaluation with classifier-free guidance.
 *   x [N,2,T] fp32 (first half is duplicated internally as forward_with_cfg does, models.py:306-307)
 *   t [N] int32 original-scale timesteps (already mapped by _WrappedModel, respace.py:127-132)
 *   c [N,context,T] fp32;  y [N,class] fp32;  band: |i-j| < band attends (banded bool mask of
 *   diffusion_pipeline.py:146-148), band <= 0 = full attention
 *   open_from: with `pad_sequence` (diffusion_pipeline.py:186-193) the window is padded to max_seq_len and the band mask
 *   is padded with "allowed" -- positions >= open_from attend and are attended by everything (the reference builds a
 *   key_padding_mask for them but DiTBlock.forward never hands it to the attention, models.py:133-150); 0 = no padding
 *   out [N,4,T] fp32: CFG-combined eps (duplicated) ++ variance channels (models.py:312-317). */
int mh_dit_forward_cfg(const MhDiTConfig* cfg, const MhDiTWeights* w, const float* x, const int32_t* t,
                       const float* c, const float* y, float cfg_scale, int band, int open_from, int N, int T,
                       float* out, void* workspace, int64_t workspace_bytes, void* stream);

/* One p_sample update (learned-range variance, epsilon prediction, clip_denoised -> clamp(-2,2)):
 *   coef fp32[7] for this step, extracted on the host from the float64 schedule exactly as
 *   _extract_into_tensor does (gaussian_diffusion.py:951-963):
 *     {posterior_log_variance_clipped, log(beta), sqrt_recip_alphas_cumprod,
 *      sqrt_recipm1_alphas_cumprod, posterior_mean_coef1, posterior_mean_coef2, nonzero_mask}
 *   model_out [N,4,T]; x [N,2,T] in; noise [N,2,T]; inpaint_mask uint8 [N,2,T] (1 = generate) and
 *   inpaint_ref [N,2,T] implement denoised_fn's `torch.where(mask, x, z_part)`
 *   (diffusion_pipeline.py:203-206), both NULL to skip;  x_out [N,2,T]; pred_xstart optional.
 *   Arbitrary host `denoised_fn`s (the slider re-projection of diffusion_pipeline.py:208-220) are
 *   served by two calls: raw_pred=1 writes the unprocessed eps->x0 prediction to pred_xstart and
 *   returns; the caller transforms it and passes it back as x0_override (clamp, posterior mean and
 *   the noise step then proceed from that value). */
int mh_ddpm_step(const float* model_out, const float* x, const float* noise, const float* coef,
                 const uint8_t* inpaint_mask, const float* inpaint_ref, const float* x0_override,
                 int raw_pred, int N, int T, float* x_out, float* pred_xstart, void* stream);

/* Sliders whose END point `denoised_fn` re-projects onto the slider's own path every denoising step (reference
 * diffusion_pipeline.py:208-220; DiffusionSlider :30-35; SliderPath osuT5/osuT5/inference/slider_path.py:26-230 and
 * path_approximator.py).  All arrays live in DEVICE memory; indices are relative to the window (column of x0).
 *   chunk b owns rows b and b + pair_stride of x0 (the CFG pair layout [cond_0..cond_{B-1} | null_0..null_{B-1}] of
 *   mh_dit_forward_cfg: pair_stride = B = n_chunks, N = 2 B), or just row b when pair_stride = 0 (n_chunks = N).
 *   chunk_active[b] != 0: the song of chunk b has sliders at all -- its positions then take the reference's pixel round
 *   trip ((x + 1) / 2 * (512, 384)) / (512, 384) * 2 - 1 and row b is broadcast over its pair, exactly as
 *   `x[:, :, :] = ...` (:220) does, even when no slider of the song lies inside this window.
 *   Sliders chunk_off[b] .. chunk_off[b+1] belong to chunk b; slider s has control points cp_idx[cp_off[s] .. cp_off[s+1]),
 *   curve type[s] (0 Linear, 1 PerfectCurve, 2 Catmull, 3 Bezier), end point end_idx[s] and length[s] (playfield pixels).
 *   The caller leaves out sliders that are not entirely inside the window (:210-212) and guarantees that no end_idx is
 *   another slider's control point or end (true for event streams: a SLIDER_END is its own point).  One Bezier span
 *   (control points between repeated points) holds at most 32 points; a longer one yields NaN positions. */
typedef struct MhSliderSet {
  int32_t n_chunks, pair_stride, n_sliders;
  const uint8_t* chunk_active; /* [n_chunks] */
  const int32_t* chunk_off;    /* [n_chunks + 1] */
  const int32_t* type;         /* [n_sliders] */
  const int32_t* cp_off;       /* [n_sliders + 1] */
  const int32_t* cp_idx;       /* [cp_off[n_sliders]] */
  const int32_t* end_idx;      /* [n_sliders] */
  const double* length;        /* [n_sliders] */
} MhSliderSet;

/* `denoised_fn` of the pipeline on x0 [N,2,T] in place: x0 = where(mask, x0, ref) (mask / ref may be NULL), then the
 * slider end re-projection above.  The path arithmetic follows the reference's numpy dtype flow (float32 Linear /
 * Catmull / circular-arc paths, float64 Bezier subdivision). */
int mh_slider_project(float* x0, const uint8_t* inpaint_mask, const float* inpaint_ref, int N, int T,
                      const MhSliderSet* sliders, void* stream);

/* Whole p_sample_loop on device (gaussian_diffusion.py:469-561): `n_steps` iterations of
 * mh_dit_forward_cfg + mh_ddpm_step captured once into a hipGraph and replayed.
 *   t_map int32 [n_steps] : timestep_map[i] for loop index i (SpacedDiffusion, respace.py:72-86)
 *   coefs fp32 [n_steps][7]; noise fp32 [n_steps][N,2,T], both indexed by loop index i
 *   (the loop runs i = n_steps-1 ... 0).  x_io [N,2,T] is updated in place.
 *   Everything that depends only on (t, y) -- timestep/label embedders and every block's adaLN modulation --
 *   is computed for all steps before the loop; workspace size from mh_ddpm_loop_workspace_bytes.
 *   sliders (NULL = none): the step becomes eps -> x0, mh_slider_project (in-paint + slider ends), posterior + noise --
 *   still inside the one captured graph. */
int64_t mh_ddpm_loop_workspace_bytes(const MhDiTConfig* cfg, int N, int T, int n_steps);
int mh_ddpm_sample_loop(const MhDiTConfig* cfg, const MhDiTWeights* w, float* x_io, const float* c,
                        const float* y, float cfg_scale, int band, int open_from, int N, int T, int n_steps,
                        const int32_t* t_map, const float* coefs, const float* noise,
                        const uint8_t* inpaint_mask, const float* inpaint_ref, const MhSliderSet* sliders,
                        void* workspace, int64_t workspace_bytes, void* stream);

/* One ddim_sample update (GaussianDiffusion.ddim_sample, gaussian_diffusion.py:563-610; epsilon prediction,
 * clip_denoised -> clamp(-2,2)).  Arguments and the raw_pred / x0_override protocol as mh_ddpm_step; the learned-variance
 * channels 2..3 of model_out are not read.
 *   coef fp32[6] for this step: {sqrt_recip_alphas_cumprod, sqrt_recipm1_alphas_cumprod, sqrt(alpha_bar_prev), sigma,
 *   sqrt(1 - alpha_bar_prev - sigma^2), nonzero_mask}, the last four computed on the host with the reference's own fp32
 *   tensor operations (:593-605) from the fp32-extracted alphas_cumprod / alphas_cumprod_prev and eta.
 *   x0 = sqrt_recip * x - sqrt_recipm1 * eps_model (:371-376) | in-paint, clamp | eps = (sqrt_recip * x - x0) / sqrt_recipm1
 *   (:378-382, re-derived from the processed x0) | x_out = x0 * coef[2] + coef[4] * eps + coef[5] * coef[3] * noise. */
int mh_ddim_step(const float* model_out, const float* x, const float* noise, const float* coef,
                 const uint8_t* inpaint_mask, const float* inpaint_ref, const float* x0_override,
                 int raw_pred, int N, int T, float* x_out, float* pred_xstart, void* stream);

/* Whole ddim_sample_loop on device (gaussian_diffusion.py:653-735): mh_ddpm_sample_loop with mh_ddim_step as the update --
 * the same arguments, the same captured graph (denoiser, step, counter; with sliders: eps -> x0, mh_slider_project, the
 * update) replayed n_steps times on the caller's non-default stream, the same workspace (mh_ddpm_loop_workspace_bytes).
 *   coefs fp32 [n_steps][6] as above; noise fp32 [n_steps][N,2,T] is read at every step, eta = 0 included (sigma = 0). */
int mh_ddim_sample_loop(const MhDiTConfig* cfg, const MhDiTWeights* w, float* x_io, const float* c,
                        const float* y, float cfg_scale, int band, int open_from, int N, int T, int n_steps,
                        const int32_t* t_map, const float* coefs, const float* noise,
                        const uint8_t* inpaint_mask, const float* inpaint_ref, const MhSliderSet* sliders,
                        void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MAPPERHIP_H_ */
