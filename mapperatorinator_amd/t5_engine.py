"""Host side of the osuT5 hot path: weight ingestion from the reference `state_dict()` names into
packed device buffers, relative-bias lookup tables, and the mel -> encode -> cross-KV -> AR-decode
driver around libmapperhip (csrc/t5_encode.hip, t5_generate.hip, t5_stepwise.hip over the token step of t5_step.hip and the decode_* units).

Numerics contract ("rounding points") of the two storage modes:
  fp32 : everything fp32; GEMMs on the exact-f32 MFMA atom (bitwise an fmaf chain).
  bf16 : parameters and GEMM operands are bf16 (`model.to(bfloat16)` semantics for the weights,
         reference osuT5/osuT5/utils/model_utils.py:375-376); accumulation, the residual stream,
         RMSNorm, softmax, GELU and logits stay fp32; activations are rounded to bf16 exactly where
         they become a GEMM operand (after each RMSNorm, q/k/v, attention output, gated FFN hidden).
         This keeps MORE precision than the reference's all-bf16 module (which also rounds the
         residual stream); `oracle/t5.py` restates the same contract on the CPU.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
from typing import Optional

import torch

from . import _lib
from .decode_modes import DecodeModes, check_cache_mode, require_bf16_for_cross_kv_fp8, require_bf16_for_self_kv_fp8  # noqa: F401
from .mel import MelSpectrogram


@dataclasses.dataclass
class T5Dims:
    d_model: int
    d_ff: int
    n_heads: int
    n_enc_layers: int
    n_dec_layers: int
    d_kv: int = 64
    n_buckets: int = 32
    max_distance: int = 128
    eps: float = 1e-6

    @property
    def inner(self) -> int:
        return self.n_heads * self.d_kv


# google/t5-v1_1-{small,base,large} (the backbones `get_backbone_model` accepts under "google/t5",
# modeling_mapperatorinator.py:20-24); "tiny" is a test-only size.
T5_PRESETS = {
    "tiny": T5Dims(d_model=128, d_ff=256, n_heads=2, n_enc_layers=2, n_dec_layers=2),
    "small": T5Dims(d_model=512, d_ff=1024, n_heads=6, n_enc_layers=8, n_dec_layers=8),
    "base": T5Dims(d_model=768, d_ff=2048, n_heads=12, n_enc_layers=12, n_dec_layers=12),
    "large": T5Dims(d_model=1024, d_ff=2816, n_heads=16, n_enc_layers=24, n_dec_layers=24),
}


def relative_position_bucket(rel: torch.Tensor, bidirectional: bool, num_buckets: int, max_distance: int):
    """The published T5 bucketing of `rel = key_pos - query_pos` (int64 tensor), evaluated with the
    same fp32 tensor ops as HF `T5Attention._relative_position_bucket` / the restatement at
    osuT5/osuT5/model/custom_transformers/t5.py:88-141, so bucket boundaries agree bit for bit."""
    ret = torch.zeros_like(rel)
    n = num_buckets
    if bidirectional:
        n //= 2
        ret = ret + (rel > 0).to(torch.long) * n
        rp = rel.abs()
    else:
        rp = -torch.min(rel, torch.zeros_like(rel))
    max_exact = n // 2
    is_small = rp < max_exact
    large = max_exact + (torch.log(rp.float() / max_exact) / math.log(max_distance / max_exact)
                         * (n - max_exact)).to(torch.long)
    large = torch.min(large, torch.full_like(large, n - 1))
    return ret + torch.where(is_small, rp, large)


def rel_bias_tables(enc_table: torch.Tensor, dec_table: torch.Tensor, src_len: int, tgt_len: int, dims: T5Dims):
    """enc [H, 2L-1] indexed by (k - q) + L - 1; dec [H, tgt_len] indexed by distance q - k >= 0."""
    rel = torch.arange(-(src_len - 1), src_len, dtype=torch.long)
    eb = relative_position_bucket(rel, True, dims.n_buckets, dims.max_distance)
    enc = enc_table.float()[eb].t().contiguous()           # [H, 2L-1]
    dist = torch.arange(0, tgt_len, dtype=torch.long)
    db = relative_position_bucket(-dist, False, dims.n_buckets, dims.max_distance)
    dec = dec_table.float()[db].t().contiguous()           # [H, tgt_len]
    return enc, dec


def _round_up(a, b):
    return (a + b - 1) // b * b


class PackedT5:
    """Device-resident packed weights + the MhT5Config / MhT5Weights structs that describe them."""

    def __init__(self, sd: dict, dims: T5Dims, vocab_in: int, vocab_out: int, n_mels: int, src_len: int,
                 tgt_len: int, dtype: torch.dtype, device, enc_operand_dtype: Optional[str] = None):
        """`enc_operand_dtype="mx8"` (BASELINE configs[4] "fp8 MFMA"; bf16 storage only): the encoder blocks' projections and
        the cross-K/V projection also get MX-fp8 copies (OCP e4m3 + E8M0 per 32 k, mx8.quantize_mx8 -- the rule the device
        applies to the activations) and MhT5Config.enc_operand_dtype selects the MX GEMMs.  A reduced-precision mode of its
        own, never the default; the decoder is untouched (its GEMVs are latency-bound)."""
        assert dtype in (torch.float32, torch.bfloat16)
        if enc_operand_dtype not in (None, "mx8"):
            raise ValueError(f"enc_operand_dtype must be None or 'mx8', got {enc_operand_dtype!r}")
        if enc_operand_dtype == "mx8" and (dtype != torch.bfloat16 or dims.d_model % 128 or dims.d_ff % 128):
            raise ValueError("MX-fp8 encoder operands need bf16 storage and d_model / d_ff multiples of 128")
        self.enc_operand_dtype = enc_operand_dtype
        self.dims, self.dtype, self.device = dims, dtype, torch.device(device)
        self.vocab_in, self.vocab_out, self.n_mels = vocab_in, vocab_out, n_mels
        self.n_mels_pad = _round_up(n_mels, 32)
        self.src_len, self.tgt_len = src_len, tgt_len
        self._keep = []
        dev = self.device

        def mat(t, kpad=None):  # GEMM operand: storage dtype, K padded with zeros
            t = t.detach().to(torch.float32)
            if kpad is not None and t.shape[1] != kpad:
                t = torch.nn.functional.pad(t, (0, kpad - t.shape[1]))
            t = t.to(dtype).contiguous().to(dev)
            self._keep.append(t)
            return t

        def mxmat(t):  # MX-fp8 copy of a GEMM operand: the weights as the bf16 path holds them, then quantised
            from .mx8 import quantize_mx8
            q, sc = quantize_mx8(t.detach().to(torch.float32).to(dtype).to(torch.float32).to(dev))
            self._keep += [q, sc]
            return q.data_ptr(), sc.data_ptr()

        def vec(t):  # fp32 vector holding the storage-dtype-rounded values
            t = t.detach().to(dtype).to(torch.float32).contiguous().to(dev)
            self._keep.append(t)
            return t

        def interleave16(a, b):  # wi_0 / wi_1 -> alternating 16-row blocks (MH_EPI_GEGLU layout)
            dff, d = a.shape
            assert dff % 16 == 0
            return torch.stack([a.reshape(dff // 16, 16, d), b.reshape(dff // 16, 16, d)], dim=1).reshape(2 * dff, d)

        pe, pd = "transformer.encoder.", "transformer.decoder."
        cfg = _lib.MhT5Config(dims.d_model, dims.d_kv, dims.d_ff, dims.n_heads, dims.n_enc_layers, dims.n_dec_layers,
                              vocab_in, vocab_out, n_mels, self.n_mels_pad, src_len, tgt_len,
                              _lib.MH_BF16 if dtype == torch.bfloat16 else _lib.MH_F32, dims.eps,
                              0, 1.0, src_len, 0, 0,      # arch 0 = T5
                              _lib.MH_MX8 if enc_operand_dtype == "mx8" else 0)
        w = _lib.MhT5Weights()
        # columns beyond n_mels belong to the conditioning vectors: they reach the device as a per-chunk row bias
        # (conditioning.ConditioningEmbedders.row_bias, mh_t5_encode_cond)
        self.cond_cols = int(sd["encoder_embedder.weight"].shape[1]) - n_mels     # > 0: the model carries conditioning embedders
        w.enc_embed_w = mat(sd["encoder_embedder.weight"][:, :n_mels], self.n_mels_pad).data_ptr()
        w.enc_embed_b = vec(sd["encoder_embedder.bias"]).data_ptr()
        w.dec_embed = mat(sd["decoder_embedder.weight"]).data_ptr()
        enc_tab = sd[pe + "block.0.layer.0.SelfAttention.relative_attention_bias.weight"].detach().to(dtype).float().cpu()
        dec_tab = sd[pd + "block.0.layer.0.SelfAttention.relative_attention_bias.weight"].detach().to(dtype).float().cpu()
        eb, db = rel_bias_tables(enc_tab, dec_tab, src_len, tgt_len, dims)
        eb, db = eb.to(dev), db.to(dev)
        self._keep += [eb, db]
        w.enc_rel_bias, w.dec_rel_bias = eb.data_ptr(), db.data_ptr()
        for l in range(dims.n_enc_layers):
            b = f"{pe}block.{l}."
            a = b + "layer.0.SelfAttention."
            w.enc_ln1[l] = vec(sd[b + "layer.0.layer_norm.weight"]).data_ptr()
            w.enc_qkv[l] = mat(torch.cat([sd[a + "q.weight"], sd[a + "k.weight"], sd[a + "v.weight"]], 0)).data_ptr()
            w.enc_o[l] = mat(sd[a + "o.weight"]).data_ptr()
            w.enc_ln2[l] = vec(sd[b + "layer.1.layer_norm.weight"]).data_ptr()
            f = b + "layer.1.DenseReluDense."
            w.enc_wi[l] = mat(interleave16(sd[f + "wi_0.weight"], sd[f + "wi_1.weight"])).data_ptr()
            w.enc_wo[l] = mat(sd[f + "wo.weight"]).data_ptr()
            if enc_operand_dtype == "mx8":
                w.enc_qkv_mx[l], w.enc_qkv_mxs[l] = mxmat(torch.cat([sd[a + "q.weight"], sd[a + "k.weight"], sd[a + "v.weight"]], 0))
                w.enc_o_mx[l], w.enc_o_mxs[l] = mxmat(sd[a + "o.weight"])
                w.enc_wi_mx[l], w.enc_wi_mxs[l] = mxmat(interleave16(sd[f + "wi_0.weight"], sd[f + "wi_1.weight"]))
                w.enc_wo_mx[l], w.enc_wo_mxs[l] = mxmat(sd[f + "wo.weight"])
        w.enc_final_ln = vec(sd[pe + "final_layer_norm.weight"]).data_ptr()
        ckv = []
        for l in range(dims.n_dec_layers):
            b = f"{pd}block.{l}."
            a = b + "layer.0.SelfAttention."
            x = b + "layer.1.EncDecAttention."
            w.dec_ln1[l] = vec(sd[b + "layer.0.layer_norm.weight"]).data_ptr()
            w.dec_qkv[l] = mat(torch.cat([sd[a + "q.weight"], sd[a + "k.weight"], sd[a + "v.weight"]], 0)).data_ptr()
            w.dec_o[l] = mat(sd[a + "o.weight"]).data_ptr()
            w.dec_ln2[l] = vec(sd[b + "layer.1.layer_norm.weight"]).data_ptr()
            w.dec_cq[l] = mat(sd[x + "q.weight"]).data_ptr()
            ckv += [sd[x + "k.weight"], sd[x + "v.weight"]]
            w.dec_co[l] = mat(sd[x + "o.weight"]).data_ptr()
            w.dec_ln3[l] = vec(sd[b + "layer.2.layer_norm.weight"]).data_ptr()
            f = b + "layer.2.DenseReluDense."
            w.dec_wi[l] = mat(interleave16(sd[f + "wi_0.weight"], sd[f + "wi_1.weight"])).data_ptr()
            w.dec_wo[l] = mat(sd[f + "wo.weight"]).data_ptr()
        w.dec_ckv_all = mat(torch.cat(ckv, 0)).data_ptr()
        if enc_operand_dtype == "mx8":
            w.dec_ckv_all_mx, w.dec_ckv_all_mxs = mxmat(torch.cat(ckv, 0))
        w.dec_final_ln = vec(sd[pd + "final_layer_norm.weight"]).data_ptr()
        w.lm_head = mat(sd["transformer.lm_head.weight"]).data_ptr()
        self.cfg, self.w = cfg, w

    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self._keep)


def guided_rows(prompt: torch.Tensor, prompt_mask, negative_prompt: torch.Tensor, forced=None):
    """The doubled batch of classifier-free guidance as the reference's prepare_inputs_for_generation builds it (modeling_mapperatorinator.py:
    243-254): -> (prompt, mask, forced) as [negative rows | prompt rows], the negative prompt over the first columns of a copy of the
    prompt.  The negative rows attend under the PROMPT's mask: in the reference the kwarg `negative_prompt_attention_mask` is
    swallowed by HF `generate()` (a named parameter of its own) before prepare_inputs_for_generation runs."""
    n = negative_prompt.shape[1]
    if n > prompt.shape[1]:
        raise ValueError("negative prompt longer than the prompt")
    neg = prompt.clone()
    neg[:, :n] = negative_prompt.to(prompt.dtype)
    return (torch.cat([neg, prompt], 0), *(None if t is None else torch.cat([t, t], 0) for t in (prompt_mask, forced)))


def eos_id_table(eos_ids, vocab_out: int) -> torch.Tensor:
    """uint8 (vocab_out,) on the host: 1 at every EOS id inside the output vocabulary"""
    table = torch.zeros(vocab_out, dtype=torch.uint8)
    table[torch.as_tensor(sorted({int(e) for e in (eos_ids or ()) if 0 <= int(e) < vocab_out}), dtype=torch.long)] = 1
    return table


def next_token_targets(ids: torch.Tensor, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Targets of next-token scoring: targets[b, t] = ids[b, t + 1]; the last column and every position whose TARGET column
    is masked out (left padding) are -1 = not scored.  int32, on the device of `ids`."""
    ids = ids.to(torch.int32)
    targets = torch.full_like(ids, -1)
    targets[:, :-1] = ids[:, 1:]
    if mask is not None:
        targets[:, :-1] = torch.where(mask[:, 1:].to(ids.device) != 0, targets[:, :-1], torch.full_like(targets[:, :-1], -1))
    return targets


class HostStager:
    """Host -> HBM copies that overlap the kernels of the batch before: the host tensor goes through a pinned buffer and
    a copy stream of its own, the consumer's stream waits on the returned event (nothing overlapped the H2D
    of batch i + 1 with the decode of batch i).  Used by the window scheduler's encode loop and by RequestBatcher."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.stream = torch.cuda.Stream(self.device)
        self._live = []                               # (event, pinned buffer): the buffer outlives its copy

    def stage(self, t: torch.Tensor, dtype=None):
        """-> (device tensor, event or None).  Returns at once; device tensors pass through."""
        if t.device.type == "cuda":
            return (t if dtype is None else t.to(dtype)), None
        self._live = [(e, b) for e, b in self._live if not e.query()]
        pin = torch.empty(t.shape, dtype=dtype or t.dtype, pin_memory=True)
        pin.copy_(t)
        with torch.cuda.stream(self.stream):
            d = pin.to(self.device, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        self._live.append((ev, pin))
        return d, ev


class T5Engine:
    """mel -> encoder -> cross-KV -> KV-cached AR decode on one GPU."""

    def __init__(self, state_dict: dict, dims: T5Dims, vocab_in: int, vocab_out: int, n_mels: int = 388,
                 src_len: int = 1251, tgt_len: int = 512, dtype: torch.dtype = torch.bfloat16, device="cuda",
                 sample_rate: int = 16000, n_fft: int = 1024, hop_length: int = 128, f_min: int = 0,
                 f_max: int = 8000, log_scale: bool = False, enc_operand_dtype: Optional[str] = None,
                 options: Optional[dict] = None):
        """`options`: this engine's own overrides of the library's tuning options ({"decode_chains": 1, ...}; names in
        include/mapperhip.h) -- other engines in the process keep theirs.  `self.options[name] = v` changes one later."""
        if not torch.cuda.is_available():
            raise RuntimeError("T5Engine needs a ROCm GPU; there is no CPU fallback")
        self.lib = _lib.load()
        self.device = torch.device(device)
        self.dims, self.dtype = dims, dtype
        self.packed = PackedT5(state_dict, dims, vocab_in, vocab_out, n_mels, src_len, tgt_len, dtype, self.device,
                               enc_operand_dtype=enc_operand_dtype)
        self.spectrogram = MelSpectrogram("nnAudio", log_scale, sample_rate, n_fft, n_mels, hop_length, f_min,
                                          f_max, "constant").to(self.device)
        self.hop_length, self.src_len, self.tgt_len = hop_length, src_len, tgt_len
        self.stream = torch.cuda.Stream(self.device)
        self._ws = {}
        self._own_options(options)

    def _own_options(self, options: Optional[dict]):
        self.options = _lib.OptionSet(options)

    # `engine.options = OptionSet(...)` (or a dict) REPLACES the set: the packed config must follow, or it would keep the handle
    # of a set that the old object's __del__ has destroyed
    @property
    def options(self) -> "_lib.OptionSet":
        return self._options

    @options.setter
    def options(self, value):
        new = value if isinstance(value, _lib.OptionSet) else _lib.OptionSet(value)
        self.packed.cfg.options = new.handle      # first the config, then drop the old set
        self._options = new

    # ---- buffers ---------------------------------------------------------------------------------
    def _workspace(self, kind: str, nbytes: int) -> torch.Tensor:
        t = self._ws.get(kind)
        if t is None or t.numel() < nbytes:
            t = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
            self._ws[kind] = t
        return t

    def _s(self) -> int:
        return self.stream.cuda_stream

    # ---- stages (all on self.stream; callers bracket with `_enter` / `_leave`) ----------------------
    def _enter(self):
        self.stream.wait_stream(torch.cuda.current_stream(self.device))

    def _leave(self):
        torch.cuda.current_stream(self.device).wait_stream(self.stream)

    def on_stream(self):
        """Context manager: the engine's stream is current (what callers outside this module use around stage calls)."""
        return torch.cuda.stream(self.stream)

    def synchronize(self):
        torch.cuda.current_stream(self.device).synchronize()

    def mel(self, audio: torch.Tensor) -> torch.Tensor:
        """(B, Ns) fp32 -> (B, L, n_mels_pad) storage dtype (K-padded GEMM operand)."""
        p = self.packed
        if audio.shape[1] // self.hop_length + 1 != p.src_len:
            raise ValueError(f"audio of {audio.shape[1]} samples gives {audio.shape[1] // self.hop_length + 1} frames; "
                             f"this engine was built for src_len={p.src_len}")
        return self.spectrogram.forward_padded(audio, p.n_mels_pad, self.dtype)

    def encode_mel(self, mel: torch.Tensor, want_f32: bool = False, row_bias: Optional[torch.Tensor] = None):
        """`row_bias` (B, d_model) fp32: the conditioning embedders' contribution incl. the bias of encoder_embedder
        (conditioning.ConditioningEmbedders.row_bias); None = the plain projection."""
        p = self.packed
        B = mel.shape[0]
        rb = None
        if row_bias is None and getattr(p, "cond_cols", 0) > 0:
            # a conditioned model without its conditioning would neither raise nor reproduce the reference: refuse
            raise ValueError(f"this model's encoder_embedder has {p.cond_cols} conditioning columns: pass row_bias "
                             "(conditioning.ConditioningEmbedders.row_bias; model_generate / MapperatorinatorHIP do)")
        if row_bias is not None:
            rb = row_bias.to(self.device, torch.float32).contiguous()
            if rb.shape != (B, self.dims.d_model):
                raise ValueError(f"row_bias must be ({B}, {self.dims.d_model}), got {tuple(rb.shape)}")
        need = self.lib.mh_t5_encode_workspace_bytes(C.byref(p.cfg), B)
        ws = self._workspace("enc", need)
        enc = torch.empty((B, p.src_len, self.dims.d_model), dtype=self.dtype, device=self.device)
        enc32 = torch.empty((B, p.src_len, self.dims.d_model), dtype=torch.float32, device=self.device) if want_f32 else None
        rc = self.lib.mh_t5_encode_cond(C.byref(p.cfg), C.byref(p.w), mel.data_ptr(), B, _lib.ptr(rb), enc.data_ptr(),
                                        _lib.ptr(enc32), ws.data_ptr(), ws.numel(), self._s())
        _lib.check(rc, "mh_t5_encode_cond")
        return (enc, enc32) if want_f32 else enc

    def cross_kv(self, enc: torch.Tensor) -> torch.Tensor:
        p = self.packed
        B = enc.shape[0]
        kv = torch.empty((self.dims.n_dec_layers, 2, B, self.dims.n_heads, p.src_len, 64), dtype=self.dtype,
                         device=self.device)
        need = self.lib.mh_t5_cross_kv_workspace_bytes(C.byref(p.cfg), B)     # (> 0 only with MX-fp8 operands: the quantised enc)
        ws = self._workspace("ckv", max(int(need), 256))
        rc = self.lib.mh_t5_cross_kv_ws(C.byref(p.cfg), C.byref(p.w), enc.data_ptr(), B, kv.data_ptr(), ws.data_ptr(), ws.numel(), self._s())
        _lib.check(rc, "mh_t5_cross_kv_ws")
        return kv

    def cross_kv_fp8(self, kv: torch.Tensor) -> torch.Tensor:
        """The packed OCP e4m3 copy of `cross_kv(enc)` (one byte per element + one fp32 scale per (layer, k|v, row,
        head)) that the token steps stream when `MhSampling.cross_kv_fp8` points at it (greedy / sampled decode) or when it is
        handed to `mh_t5_step_fp8` (beam search): half the HBM bytes of the dominant decode kernel (BASELINE configs[4]).
        Every backbone (T5 and the Whisper families); bf16 storage only; not a parity mode."""
        require_bf16_for_cross_kv_fp8(self.dtype)
        p = self.packed
        B = kv.shape[2]
        out = torch.empty(self.lib.mh_t5_cross_kv_fp8_bytes(C.byref(p.cfg), B), dtype=torch.uint8, device=self.device)
        rc = self.lib.mh_t5_quantize_cross_kv(C.byref(p.cfg), kv.data_ptr(), B, out.data_ptr(), self._s())
        _lib.check(rc, "mh_t5_quantize_cross_kv")
        return out

    def encode(self, audio: torch.Tensor, want_f32: bool = False, row_bias: Optional[torch.Tensor] = None):
        """audio (B, Ns) on the GPU -> encoder last_hidden_state (final RMSNorm applied)."""
        self._enter()
        with torch.cuda.stream(self.stream):
            out = self.encode_mel(self.mel(audio), want_f32, row_bias)
        self._leave()
        return out

    def decoder_forward(self, cross_kv: torch.Tensor, ids: torch.Tensor, mask: Optional[torch.Tensor] = None):
        """Teacher-forced logits of every position: ids int32 (B, T) on the device -> fp32 (B, T, vocab_out)."""
        p = self.packed
        B, T = ids.shape
        if cross_kv.shape[2] != B:
            raise ValueError(f"cross_kv holds {cross_kv.shape[2]} rows for {B} sequences")
        need = self.lib.mh_t5_forward_workspace_bytes(C.byref(p.cfg), B, T)
        ws = self._workspace("fwd", need)
        logits = torch.empty((B, T, p.vocab_out), dtype=torch.float32, device=self.device)
        rc = self.lib.mh_t5_decoder_forward(C.byref(p.cfg), C.byref(p.w), cross_kv.data_ptr(), B, ids.data_ptr(),
                                            _lib.ptr(mask), T, logits.data_ptr(), ws.data_ptr(), ws.numel(), self._s())
        _lib.check(rc, "mh_t5_decoder_forward")
        return logits

    def score(self, cross_kv: torch.Tensor, ids: torch.Tensor, mask: Optional[torch.Tensor] = None, targets=None):
        """Teacher-forced scoring (mh_t5_score): ids int32 (B, T) on the device -> dict of device tensors `surprisal`, `entropy`,
        `relative`, `logprob` (fp32 (B, T)) and `best_id` (int64 (B, T)); the logits never leave the LM-head block they are
        computed in.  `targets` (B, T): the id each position is scored against, negative = not scored (zeros, best_id -1);
        None = next-token scoring (`next_token_targets`).  A target >= vocab_out is refused here when the targets come from the
        host; targets already on the device are not read back (the kernel leaves such a position unscored)."""
        p = self.packed
        B, T = ids.shape
        if cross_kv.shape[2] != B:
            raise ValueError(f"cross_kv holds {cross_kv.shape[2]} rows for {B} sequences")
        max_scored = -1                                 # unknown: the targets live on the device and are not read back
        if targets is None:
            targets = next_token_targets(ids, mask)
        else:
            targets = torch.as_tensor(targets)
            if tuple(targets.shape) != (B, T):
                raise ValueError(f"targets must be ({B}, {T}), got {tuple(targets.shape)}")
            if targets.device.type == "cpu":            # the host has them: check the range, count the scored positions for free
                if targets.numel() and int(targets.max()) >= p.vocab_out:
                    raise ValueError(f"target id {int(targets.max())} is outside the output vocabulary of {p.vocab_out}")
                max_scored = int((targets >= 0).sum())
        targets = targets.to(self.device, torch.int32).contiguous()
        need = self.lib.mh_t5_score_workspace_bytes(C.byref(p.cfg), B, T)
        ws = self._workspace("score", need)
        f32 = [torch.empty((B, T), dtype=torch.float32, device=self.device) for _ in range(4)]
        best = torch.empty((B, T), dtype=torch.int32, device=self.device)
        rc = self.lib.mh_t5_score(C.byref(p.cfg), C.byref(p.w), cross_kv.data_ptr(), B, ids.data_ptr(), _lib.ptr(mask), T,
                                  targets.data_ptr(), max_scored, f32[0].data_ptr(), f32[1].data_ptr(), f32[2].data_ptr(),
                                  f32[3].data_ptr(), best.data_ptr(), ws.data_ptr(), ws.numel(), self._s())
        _lib.check(rc, "mh_t5_score")
        return dict(surprisal=f32[0], entropy=f32[1], relative=f32[2], logprob=f32[3], best_id=best.to(torch.int64))

    def decode(self, cross_kv: torch.Tensor, prompt: torch.Tensor, prompt_mask: Optional[torch.Tensor],
               eos_table: torch.Tensor, sampling: _lib.MhSampling, forced: Optional[torch.Tensor] = None,
               dump_logits: bool = False, poll_every: int = 16, kv_fp8: Optional[torch.Tensor] = None,
               self_kv_fp8: bool = False, row_sampling=None):
        """prompt int32 (B, P) on device.  Returns (tokens int32 (B, max_length) device, n_cols int, logits|None).
        Under CFG (sampling.cfg_scale > 1) the B rows are [negative-prompt rows | prompt rows], `cross_kv` holds
        B/2 rows and the logits dump has B/2 rows (the guided scores).
        `self_kv_fp8`: the token steps attend an e4m3 shadow of the self-attention cache (`mh_t5_generate_skv8`, contract in
        include/mapperhip.h: one fp32 scale per cached row, the step's own key / value at storage precision, the prompt prefill
        unchanged and quantised in one pass).  The shadow is this engine's, kept like the workspaces.  bf16 storage only.
        `row_sampling`: what `server.build_row_sampling` returned -- `(sp, rows, eos_tables)`, or its `(rows, eos_tables)` -- decodes
        through `mh_t5_generate_rows`: one `MhRowSampling` per returned row and one EOS table per distinct EOS set (the lists of
        per-row and per-call settings: include/mapperhip.h); `sampling` carries the per-call settings and `eos_table` is ignored
        (may be None).  The device copies live in this engine's buffers, so their pointers -- part of the step graph's key -- do not
        move from call to call."""
        if self_kv_fp8:
            require_bf16_for_self_kv_fp8(self.dtype)
        p = self.packed
        B, P = prompt.shape
        cfg = sampling.cfg_scale > 1.0
        row_args = None
        if row_sampling is not None:
            rows, eos_tables = row_sampling[-2], row_sampling[-1]
            n_ret = B // 2 if cfg else B
            if len(rows) != n_ret:
                raise ValueError(f"row_sampling holds {len(rows)} rows for {n_ret} returned rows (batch {B}, cfg={cfg})")
            eos_tables = torch.as_tensor(eos_tables, dtype=torch.uint8).reshape(-1, p.vocab_out).contiguous()
            n_sets = int(eos_tables.shape[0])
            bad = [r for r in range(n_ret) if not 0 <= rows[r].eos_set < n_sets or not P < rows[r].max_length <= sampling.max_length
                   or not rows[r].temperature > 0]
            if bad:
                raise ValueError(f"row_sampling: row {bad[0]} is out of range (eos_set in [0, {n_sets}), prompt length {P} < max_length "
                                 f"<= {sampling.max_length}, temperature > 0)")
            if n_sets > 64:
                raise ValueError(f"row_sampling: {n_sets} EOS sets (a decode batch has 64 rows at most, hence 64 distinct sets)")
            # 64 entries and 64 tables (the largest decode batch), allocated once: neither pointer ever moves, and the library is
            # told the buffer's 64 sets whatever the call uses (its clamp guards the buffer, the check above the call's own range),
            # so neither the pointers nor the count -- all three in the step graph's key -- change with the mix
            rows_d = self._workspace("row_sampling", 64 * C.sizeof(_lib.MhRowSampling))
            eos_d = self._workspace("row_eos_tables", 64 * p.vocab_out)
            host = torch.frombuffer(bytearray(bytes(rows)), dtype=torch.uint8)
            rows_d[:host.numel()].copy_(host)
            eos_d[:eos_tables.numel()].copy_(eos_tables.reshape(-1))
            row_args = (rows_d.data_ptr(), eos_d.data_ptr(), 64)
        if cross_kv.shape[2] != (B // 2 if cfg else B):
            raise ValueError(f"cross_kv holds {cross_kv.shape[2]} rows for a decode batch of {B} (cfg={cfg})")
        flags = getattr(sampling, "host_tok_flags", None)
        if flags is not None:   # keep the device copy alive for the duration of the call
            flags_d = torch.as_tensor(flags, dtype=torch.uint8).to(self.device)
            sampling.tok_flags = flags_d.data_ptr()
        elif sampling.n_cond or sampling.lookback_types_first:
            raise ValueError("sampling needs tok_flags (build it with server.build_sampling)")
        sampling.cross_kv_fp8 = kv_fp8.data_ptr() if kv_fp8 is not None else None
        need = self.lib.mh_t5_decode_workspace_bytes(C.byref(p.cfg), B)
        ws = self._workspace("dec", need)
        maxlen = sampling.max_length
        tokens = torch.full((B, maxlen), int(sampling.pad_id), dtype=torch.int32, device=self.device)
        n_out = torch.zeros(1, dtype=torch.int32, device=self.device)
        logits = (torch.zeros((maxlen, B // 2 if cfg else B, p.vocab_out), dtype=torch.float32, device=self.device)
                  if dump_logits else None)
        args = (C.byref(p.cfg), C.byref(p.w), cross_kv.data_ptr(), B, prompt.data_ptr(),
                _lib.ptr(prompt_mask), P, _lib.ptr(eos_table), C.byref(sampling),
                tokens.data_ptr(), n_out.data_ptr(), _lib.ptr(logits), _lib.ptr(forced),
                ws.data_ptr(), ws.numel(), poll_every, self._s())
        if row_args is not None:
            skv8 = self._workspace("skv8", self.lib.mh_t5_self_kv_fp8_bytes(C.byref(p.cfg), B)) if self_kv_fp8 else None
            _lib.check(self.lib.mh_t5_generate_rows(*args, _lib.ptr(skv8), *row_args), "mh_t5_generate_rows")
        elif self_kv_fp8:
            skv8 = self._workspace("skv8", self.lib.mh_t5_self_kv_fp8_bytes(C.byref(p.cfg), B))
            _lib.check(self.lib.mh_t5_generate_skv8(*args, skv8.data_ptr()), "mh_t5_generate_skv8")
        else:
            _lib.check(self.lib.mh_t5_generate(*args), "mh_t5_generate")
        return tokens, n_out, logits

    def open_slots(self, S: int, sampling: _lib.MhSampling, dump_logits: bool = False, poll_every: int = 16,
                   cross_kv_fp8: bool = False, self_kv_fp8: bool = False) -> "DecodeSlots":
        """In-flight decode (`mh_t5_slots_*`, contract in include/mapperhip.h): S slots, every slot a row that decodes a window of
        its own; a finished row's place goes to the next window while its neighbours keep stepping.  `sampling`: the per-call
        settings (`server.build_row_sampling(...)[0]`; `max_length` = the longest window the session can hold).  Returns a
        `DecodeSlots` with `admit`, `run`, `take` and `close`.  Greedy and sampled rows, per-row settings; no guidance, beams
        or teacher forcing (refused by the library).  One session per engine at a time: its buffers live in this
        engine's workspaces like the row-settings ones, so their pointers -- part of the step graph's key -- do not move.
        `cross_kv_fp8` / `self_kv_fp8`: switches of the SESSION (`mh_t5_slots_open_kv8`; bf16 storage only): the token steps stream
        an S-row e4m3 copy of the slots' cross K/V, which every admission fills for its slot -- the session then holds no bf16 copy
        of it at all -- and / or attend an S-row e4m3 shadow of the self-attention cache.  A slot then computes what the batch-1
        `decode` computes under the same switches, bit for bit.  Guidance: `open_guided_slots`."""
        return DecodeSlots(self, int(S), sampling, dump_logits, poll_every, cross_kv_fp8, self_kv_fp8)

    def open_guided_slots(self, S: int, sampling: _lib.MhSampling, dump_logits: bool = False, poll_every: int = 16,
                          cross_kv_fp8: bool = False, self_kv_fp8: bool = False) -> "DecodeSlots":
        """`open_slots` under classifier-free guidance (`mh_t5_slots_open_guided`): every slot is a PAIR -- the negative-prompt row and
        the prompt row of one window (`guided_rows`), admitted with `admit(..., negative_prompt=)`, stepped, finished and taken
        together; S in [1, 32] pairs over 2 S decode rows on one chain, `sampling.cfg_scale > 1` (the scale is each pair's own: its
        row entry's).  A slot computes what the 2-row guided `decode(row_sampling=)` of the window alone computes, bit for bit, under
        the same `cross_kv_fp8` / `self_kv_fp8` switches.  Every window of the session is guided; `open_slots` refuses guidance as
        ever.  (A method of its own: the argument list of `open_slots` is pinned.)"""
        return DecodeSlots(self, int(S), sampling, dump_logits, poll_every, cross_kv_fp8, self_kv_fp8, guided=True)

    def quantize_kv_rows(self, rows: torch.Tensor):
        """`mh_quantize_kv_rows`: bf16 (..., 64) on the device -> (e4m3 bytes uint8 (..., 64), fp32 scales (...)), the row form of the
        e4m3 self-attention cache (scale = absmax / 448, element = cvt_e4m3(x * (1 / scale)))."""
        rows = rows.contiguous()
        if rows.dtype != torch.bfloat16 or rows.shape[-1] != 64:
            raise ValueError(f"rows must be bf16 (..., 64), got {rows.dtype} {tuple(rows.shape)}")
        q = torch.empty(rows.shape, dtype=torch.uint8, device=rows.device)
        sc = torch.empty(rows.shape[:-1], dtype=torch.float32, device=rows.device)
        _lib.check(self.lib.mh_quantize_kv_rows(rows.data_ptr(), rows.numel() // 64, q.data_ptr(), sc.data_ptr(), self._s()),
                   "mh_quantize_kv_rows")
        return q, sc

    def self_kv_caches(self, B: int, shadow: bool = False):
        """Views of what the last `decode` of B rows left behind (no copy): the bf16 self-attention caches (k, v), each
        (n_dec, B, H, tgt_len, 64), read through `mh_t5_decode_self_cache`; with `shadow` also the e4m3 shadow of a `self_kv_fp8`
        decode: bytes uint8 (n_dec, 2, B, H, tgt_len, 64) and fp32 scales (n_dec, 2, B, H, tgt_len)."""
        p = self.packed
        ws = self._ws["dec"]
        k, v = C.c_void_p(), C.c_void_p()
        _lib.check(self.lib.mh_t5_decode_self_cache(C.byref(p.cfg), B, ws.data_ptr(), C.byref(k), C.byref(v)), "mh_t5_decode_self_cache")
        shape = (self.dims.n_dec_layers, B, self.dims.n_heads, p.tgt_len, 64)
        n = shape[0] * shape[1] * shape[2] * shape[3] * 64 * ws.new_empty(0, dtype=self.dtype).element_size()
        out = [ws[ptr - ws.data_ptr(): ptr - ws.data_ptr() + n].view(self.dtype).view(shape) for ptr in (k.value, v.value)]
        if shadow:
            sh = self._ws["skv8"]
            rows = shape[0] * 2 * B * shape[2] * shape[3]
            off = (rows * 64 + 255) // 256 * 256
            out.append(sh[: rows * 64].view(shape[0], 2, B, shape[2], shape[3], 64))
            out.append(sh[off: off + rows * 4].view(torch.float32).view(shape[0], 2, B, shape[2], shape[3]))
        return tuple(out)

    def generate_beam(self, audio: torch.Tensor, prompt: torch.Tensor, prompt_mask: Optional[torch.Tensor], eos_ids,
                      sampling: _lib.MhSampling, num_beams: int, row_bias: Optional[torch.Tensor] = None,
                      length_penalty: float = 1.0, early_stopping=False, negative_prompt: Optional[torch.Tensor] = None,
                      sample_fn=None, use_kernel: Optional[bool] = None, cross_kv_fp8: bool = False, device_draw: bool = False,
                      beam_cache: str = "copy", beam_prefill: bool = False, beam_self_kv_fp8: bool = False):
        """mel -> encoder -> cross K/V, then HF-style beam search over the step-wise decode entry (beam.py).  Returns
        dict(tokens=int64 CPU (B, n_cols), n_cols, logits=None) like `generate`.  `negative_prompt` with sampling.cfg_scale > 1:
        classifier-free guidance under beams (the doubled batch of modeling_mapperatorinator.py:243-254; beam.py).  With
        `sampling.do_sample` the continuations are drawn (beam-sample): `sample_fn(probs, k)` or torch.multinomial on the device, or
        with `device_draw=True` inside the step kernel (mh_beam_step_sample; seed sampling.seed: beam.py).
        `cross_kv_fp8`: every step streams the e4m3 copy of the cross-attention K / V (see `cross_kv_fp8()`; under guidance the copy
        is made of the doubled rows).
        `beam_cache` "copy" | "indexed", `beam_prefill`, `beam_self_kv_fp8`: beam.py `cache` / `prefill` / `self_kv_fp8` (decode_modes.py)
        -- the self-attention cache followed by an index table instead of copied after every token, the prompt prefilled once per
        chunk, the e4m3 shadow of the cache read through the same table (the last two need the indexed cache)."""
        from .beam import beam_search
        modes = DecodeModes.of(dict(cross_kv_fp8=cross_kv_fp8, self_kv_fp8=beam_self_kv_fp8, beam_cache=beam_cache, beam_prefill=beam_prefill,
                                    beam_sample_kernel=device_draw), self.dtype, int(num_beams), order=("cache", "self", "cross"))
        audio = audio.to(self.device, torch.float32)
        if (negative_prompt is not None) != (sampling.cfg_scale > 1.0):
            raise ValueError("negative_prompt and sampling.cfg_scale > 1 go together")
        if negative_prompt is not None:
            prompt, prompt_mask, _ = guided_rows(prompt, prompt_mask, negative_prompt)
        self._enter()
        with torch.cuda.stream(self.stream):
            kv = self.cross_kv(self.encode_mel(self.mel(audio), row_bias=row_bias))
        self._leave()
        out = beam_search(self, kv, prompt, prompt_mask, eos_ids, sampling, num_beams, length_penalty, early_stopping,
                          sample_fn=sample_fn, use_kernel=use_kernel, **modes.beam_search_kwargs())
        return dict(tokens=out.cpu(), n_cols=int(out.shape[1]), logits=None)

    def generate(self, audio: torch.Tensor, prompt: torch.Tensor, prompt_mask: Optional[torch.Tensor],
                 eos_ids, sampling: _lib.MhSampling, forced: Optional[torch.Tensor] = None,
                 dump_logits: bool = False, poll_every: int = 16, negative_prompt: Optional[torch.Tensor] = None,
                 negative_mask: Optional[torch.Tensor] = None, cross_kv_fp8: bool = False,
                 row_bias: Optional[torch.Tensor] = None, encoder_states: Optional[torch.Tensor] = None,
                 self_kv_fp8: bool = False, row_sampling=None):
        """Full hot path for one batch of chunks.  `row_sampling`: the result of `server.build_row_sampling` -- every row decodes under
        its own settings (see `decode`); `sampling` is its first item and `eos_ids` is ignored.  `encoder_states` (B, src_len, d_model): the encoder's last_hidden_state given by
        the caller (`generate(encoder_outputs=...)` of the reference's signature) -- mel and encoder are skipped, `audio` may be None.  `cross_kv_fp8`: the token steps stream the e4m3 copy of the
        cross-attention K / V (see `cross_kv_fp8()`); `self_kv_fp8`: they attend the e4m3 shadow of the self-attention cache (see `decode`; the two
        compose to a whole fp8 K/V cache).  Inputs may be CPU tensors (copied like
        server.py:86-87 does).  Returns dict(tokens=int64 CPU (B, n_cols), logits=..., n_cols=int).
        With `negative_prompt` (classifier-free guidance) the decode batch is doubled (`guided_rows`); the returned rows are the prompt rows."""
        dev = self.device
        DecodeModes.of(dict(cross_kv_fp8=cross_kv_fp8, self_kv_fp8=self_kv_fp8), self.dtype)
        if encoder_states is None:
            audio = audio.to(dev, torch.float32)
        else:
            encoder_states = encoder_states.to(dev, self.dtype).contiguous()
            if tuple(encoder_states.shape) != (prompt.shape[0], self.packed.src_len, self.dims.d_model):
                raise ValueError(f"encoder_states must be ({prompt.shape[0]}, {self.packed.src_len}, {self.dims.d_model}), got {tuple(encoder_states.shape)}")
        G = prompt.shape[0]
        cfg = negative_prompt is not None
        if cfg != (sampling.cfg_scale > 1.0):
            raise ValueError("negative_prompt and sampling.cfg_scale > 1 go together")
        if cfg:      # (`negative_mask` is accepted for signature parity and deliberately unused: see `guided_rows`)
            prompt, prompt_mask, forced = guided_rows(prompt, prompt_mask, negative_prompt, forced)
        prompt_d = prompt.to(dev, torch.int32).contiguous()
        mask_d = prompt_mask.to(dev).to(torch.uint8).contiguous() if prompt_mask is not None else None
        forced_d = forced.to(dev, torch.int32).contiguous() if forced is not None else None
        eos_table = eos_id_table(eos_ids, self.packed.vocab_out).to(dev)
        self._enter()
        with torch.cuda.stream(self.stream):
            enc = encoder_states if encoder_states is not None else self.encode_mel(self.mel(audio), row_bias=row_bias)
            kv = self.cross_kv(enc)
            kv8 = self.cross_kv_fp8(kv) if cross_kv_fp8 else None
            tokens, n_out, logits = self.decode(kv, prompt_d, mask_d, eos_table, sampling, forced_d, dump_logits,
                                                poll_every, kv_fp8=kv8, self_kv_fp8=self_kv_fp8, row_sampling=row_sampling)
        self._leave()
        torch.cuda.current_stream(dev).synchronize()
        n_cols = int(n_out.item()) if forced is None else sampling.max_length
        if cfg:
            tokens = tokens[G:]
        return dict(tokens=tokens[:, :n_cols].to(torch.int64).cpu(), n_cols=n_cols,
                    logits=None if logits is None else logits[:n_cols])


class DecodeSlots:
    """A session of `T5Engine.open_slots`: S slots over `mh_t5_slots_*` (contract in include/mapperhip.h).

        slots = engine.open_slots(S, sp)
        slots.admit(slot, cross_kv_row, prompt, prompt_mask, row, eos_table)     # an idle slot <- one window
        finished, lengths = slots.run(n_steps)                                   # every chain steps; one poll
        tokens = slots.take(slot)                                                # the row so far, and the slot is idle again
        slots.close()

    A slot computes what `T5Engine.decode(row_sampling=...)` computes for the window alone (B = 1, its unpadded prompt, its own
    row entry), bit for bit.  `stats`: admissions and graph replays so far.
    `guided`: S pairs over R = 2 S decode rows, `tokens` (2 S, max_length) as [negative rows | prompt rows], slot s = rows s and S + s;
    `logits` (max_length, S, vocab_out); `take` returns the prompt row."""

    def __init__(self, engine: "T5Engine", S: int, sampling: _lib.MhSampling, dump_logits: bool, poll_every: int,
                 cross_kv_fp8: bool = False, self_kv_fp8: bool = False, guided: bool = False):
        self.guided = bool(guided)
        if self.guided and not 1 <= S <= 32:
            raise ValueError(f"open_guided_slots: {S} pairs not in [1, 32] (a decode batch holds 64 rows)")
        if self.guided and not sampling.cfg_scale > 1.0:
            raise ValueError("open_guided_slots: needs sampling.cfg_scale > 1 (the scale itself is each pair's own)")
        if not 1 <= S <= 64:
            raise ValueError(f"open_slots: {S} slots not in [1, 64]")
        if getattr(engine, "_slot_session", None) is not None:
            raise RuntimeError("open_slots: this engine has an open slot session (its buffers are the engine's): close it first")
        self.modes = DecodeModes.of(dict(cross_kv_fp8=cross_kv_fp8, self_kv_fp8=self_kv_fp8), engine.dtype)   # (the storage refusals)
        self.engine, self.S, self.sampling = engine, S, sampling
        self.R = R = 2 * S if self.guided else S      # decode rows
        self._handle = C.c_void_p()
        p = engine.packed
        dev, lib = engine.device, engine.lib
        flags = getattr(sampling, "host_tok_flags", None)
        if flags is not None:   # the device copy lives as long as the session
            self._flags_d = torch.as_tensor(flags, dtype=torch.uint8).to(dev)
            sampling.tok_flags = self._flags_d.data_ptr()
        elif sampling.n_cond or sampling.lookback_types_first:
            raise ValueError("sampling needs tok_flags (build it with server.build_row_sampling)")
        self.max_length = maxlen = int(sampling.max_length)
        es = torch.empty(0, dtype=engine.dtype).element_size()
        d = engine.dims
        row_sz = C.sizeof(_lib.MhRowSampling)
        self._rows_d = engine._workspace("slot_rows", 64 * row_sz)
        self._eos_d = engine._workspace("slot_eos_tables", 64 * p.vocab_out)
        self._rows_d.zero_()
        self._eos_d.zero_()
        # the slots' cross K/V: the bf16 / fp32 copy, or -- cross_kv_fp8 -- the e4m3 one alone (no token step would read the other);
        # the e4m3 shadow of the self-attention cache.  Neither e4m3 buffer is initialised: the admissions and the steps fill them
        self.cross_kv = self.cross_kv8 = self.self_kv8 = None
        if self.modes.cross_kv_fp8:
            self.cross_kv8 = engine._workspace("slot_cross_kv8", lib.mh_t5_cross_kv_fp8_bytes(C.byref(p.cfg), S))
        else:
            self.cross_kv = engine._workspace("slot_cross_kv", d.n_dec_layers * 2 * S * d.n_heads * p.src_len * 64 * es)
        if self.modes.self_kv_fp8:
            self.self_kv8 = engine._workspace("slot_skv8", lib.mh_t5_self_kv_fp8_bytes(C.byref(p.cfg), R))
        self.tokens = engine._workspace("slot_tokens", 64 * p.tgt_len * 4)[:R * maxlen * 4].view(torch.int32).view(R, maxlen)
        self.logits = None
        if dump_logits:
            n = maxlen * S * p.vocab_out
            self.logits = engine._workspace("slot_logits", n * 4)[:n * 4].view(torch.float32).view(maxlen, S, p.vocab_out)
            self.logits.zero_()
        ws = engine._workspace("slots", (lib.mh_t5_slots_guided_workspace_bytes if self.guided else lib.mh_t5_slots_workspace_bytes)(C.byref(p.cfg), S))
        self._hold = [None] * S          # what an admission reads, kept until the slot is taken
        self._lengths = [0] * S
        self._finished = [False] * S
        self.live = [False] * S
        self.stats = dict(admissions=0, steps=0, runs=0)
        kv8 = self.cross_kv8 is not None or self.self_kv8 is not None
        entry = "mh_t5_slots_open_kv8" if kv8 else "mh_t5_slots_open"        # the new entry only when a switch is on
        if self.guided:
            entry = "mh_t5_slots_open_guided"
        sampling.cross_kv_fp8 = _lib.ptr(self.cross_kv8)
        engine._enter()
        try:
            _lib.check(getattr(lib, entry)(C.byref(p.cfg), C.byref(p.w), S, C.byref(sampling), self._rows_d.data_ptr(),
                                           self._eos_d.data_ptr(), 64, _lib.ptr(self.cross_kv), self.tokens.data_ptr(),
                                           _lib.ptr(self.logits), None, _lib.ptr(self.self_kv8), ws.data_ptr(), ws.numel(), int(poll_every),
                                           engine._s(), C.byref(self._handle)), entry)
        finally:
            engine._leave()
            sampling.cross_kv_fp8 = None      # (the session has read it: the caller's settings stay those of a plain call)
        engine._slot_session = self

    def admit(self, slot: int, cross_kv_row: torch.Tensor, prompt: torch.Tensor, prompt_mask: Optional[torch.Tensor],
              row: _lib.MhRowSampling, eos_table: torch.Tensor, negative_prompt: Optional[torch.Tensor] = None) -> None:
        """One window into an idle slot: `cross_kv_row` its cross K/V (n_dec, 2, [1,] H, L, 64), `prompt` its own ids (P,) or (1, P)
        without padding, `prompt_mask` or None, `row` its settings (an entry of `server.build_row_sampling(...)[1]`) and
        `eos_table` uint8 (vocab_out,) its EOS set.  Returns at once; the slot's chain picks the window up at its next step.
        `negative_prompt` (n,) or (1, n), n <= P: required on a guided session, refused on a plain one -- the pair is built by
        `guided_rows` (both rows under `prompt_mask`) and admitted as one; `row.cfg_scale` is the pair's scale."""
        eng, p = self.engine, self.engine.packed
        if not 0 <= slot < self.S or self.live[slot]:
            raise ValueError(f"admit: slot {slot} is not an idle slot of this session")
        if self.guided and negative_prompt is None:
            raise ValueError("admit: a guided session admits pairs: negative_prompt is required")
        if not self.guided and negative_prompt is not None:
            raise ValueError("admit: negative_prompt on a session without guidance (open_guided_slots opens a guided one)")
        if self.guided and not row.cfg_scale > 1.0:
            raise ValueError(f"admit: a guided session needs row.cfg_scale > 1, got {row.cfg_scale}")
        prompt = prompt.reshape(-1)
        P = int(prompt.shape[0])
        if self.guided:      # [negative | prompt], (2, P)
            prompt = guided_rows(prompt.reshape(1, -1), None, negative_prompt.reshape(1, -1))[0]
        if not (1 <= P < row.max_length <= self.max_length) or not row.temperature > 0:
            raise ValueError(f"admit: prompt length {P} < row.max_length {row.max_length} <= {self.max_length} and temperature > 0 expected")
        d = eng.dims
        entry = _lib.MhRowSampling.from_buffer_copy(bytes(row))
        entry.eos_set = slot                     # every slot owns a table: the EOS set of the window it holds
        eng._enter()
        try:
            with torch.cuda.stream(eng.stream):
                kv = cross_kv_row.reshape(d.n_dec_layers, 2, 1, d.n_heads, p.src_len, 64).to(eng.device, eng.dtype).contiguous()
                prompt_d = prompt.to(eng.device, torch.int32).contiguous()
                mask_d = None if prompt_mask is None else prompt_mask.reshape(-1).to(eng.device).to(torch.uint8).contiguous()
                sz = C.sizeof(_lib.MhRowSampling)
                self._rows_d[slot * sz:(slot + 1) * sz].copy_(torch.frombuffer(bytearray(bytes(entry)), dtype=torch.uint8))
                self._eos_d[slot * p.vocab_out:(slot + 1) * p.vocab_out].copy_(torch.as_tensor(eos_table, dtype=torch.uint8).reshape(-1))
                self._hold[slot] = (kv, prompt_d, mask_d)
                name = "mh_t5_slots_admit_pair" if self.guided else "mh_t5_slots_admit"
                _lib.check(getattr(eng.lib, name)(self._handle, slot, kv.data_ptr(), prompt_d.data_ptr(), _lib.ptr(mask_d), P, eng._s()), name)
        finally:
            eng._leave()
        self.live[slot], self._finished[slot], self._lengths[slot] = True, False, P
        self.stats["admissions"] += 1

    def run(self, n_steps: int = 16):
        """Up to `n_steps` token steps of every chain that has a live slot -> (finished, lengths): per slot, whether its row is
        done and the valid columns of `tokens[slot]` (0 for an idle slot)."""
        fin = (C.c_uint8 * self.S)()
        length = (C.c_int32 * self.S)()
        steps = C.c_int(0)
        _lib.check(self.engine.lib.mh_t5_slots_run(self._handle, int(n_steps), fin, length, C.byref(steps)), "mh_t5_slots_run")
        self._finished = [bool(f) for f in fin]
        self._lengths = [int(n) for n in length]
        self.stats["steps"] += int(steps.value)
        self.stats["runs"] += 1
        return list(self._finished), list(self._lengths)

    def take(self, slot: int) -> torch.Tensor:
        """The slot's row as of the last `run` -- int64 CPU (length,), the prompt included -- and the slot is idle again."""
        if not 0 <= slot < self.S or not self.live[slot]:
            raise ValueError(f"take: slot {slot} is not a live slot of this session")
        out = self.tokens[self.S + slot if self.guided else slot, :self._lengths[slot]].to(torch.int64).cpu()
        _lib.check(self.engine.lib.mh_t5_slots_release(self._handle, slot), "mh_t5_slots_release")
        self.live[slot], self._hold[slot], self._lengths[slot], self._finished[slot] = False, None, 0, False
        return out

    def close(self) -> None:
        h, self._handle = self._handle, C.c_void_p()
        if h:
            if getattr(self.engine, "_slot_session", None) is self:
                self.engine._slot_session = None
            _lib.check(self.engine.lib.mh_t5_slots_close(h), "mh_t5_slots_close")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
