"""TEST SUPPORT: the decode runs behind tests/golden/attn_early_kv_tiny.npz (tests/test_gpu_attn_early_kv.py).

The decode attention's key loop (`attend_keys`, csrc/decode_device.hpp) can run its first iteration on K / V rows that the kernel
requested before the query existed (`FirstKeys`); every sum keeps its operands and its order, so the scores must not move by a bit.
The fixture holds the processed scores of short teacher-forced decodes as the build BEFORE that change dumped them, and the test
compares a run of the current build bit for bit.  `run_case` is the one statement of every run, shared by the test and by the
recorder below (`MAPPERHIP_LIB=<the library of the build to be recorded> python -m mh_testing.attn_early_kv OUT.npz` on a GPU).

The shapes are the smallest at which a peeled first iteration can go wrong (tiny dims: d_model 128, 2 heads, 2 decoder layers):
  cross-attention   3 rows, a 1-token prompt and 4 forced tokens over encoder lengths 1, 7, 8, 9 (lane groups and whole waves without
                    a key), 127, 128, 129 (one full 128-key workgroup iteration, one key less, one key into the next) and 257 (two
                    iterations plus one), fp32 and bf16 storage; the encoder states are given, so that no audio has to make 1 frame.
                    Plus the e4m3 copy of the cross K / V (`cross_kv_fp8`) at 129 and a Whisper-family model at 129 encoder positions.
  self-attention    a 1-token prompt and 130 forced tokens (positions 0, 1, 127, 128 and 129 are all crossed), 3 rows (one chain) and
                    18 rows (two chains), fp32 and bf16; a left-padded prompt mask of width 9; the e4m3 shadow cache (`self_kv_fp8`);
                    and the indexed step of the beam search (`mh_t5_step_indexed`) under a table that is reordered after every step.
The fixture stays small: per (column, row) the first 16 bytes of the SHA-256 of the row's scores (equal digests = equal bits), and
the raw bits of SAMPLE_IDS evenly spread ids, so that a mismatch can be told apart as one ulp or garbage.
"""
from __future__ import annotations

import numpy as np
import torch

from mh_testing.lane_reduce import DTYPES, SAMPLE_IDS, summarise  # noqa: F401  (one fixture format for both recordings)

CROSS_LENGTHS = (1, 7, 8, 9, 127, 128, 129, 257)
CROSS_ROWS, CROSS_NEW = 3, 4
SELF_NEW, SELF_SRC = 130, 9
MASK_WIDTH, MASK_LENS = 9, (9, 4, 1)
WHISPER_FRAMES = 257            # (257 - 1) // 2 + 1 = 129 encoder positions

CASES = ([f"cross_L{L}_{d}" for L in CROSS_LENGTHS for d in DTYPES] + ["cross_fp8_L129_bf16", "cross_whisper_L129_bf16"] +
         [f"self_rows{r}_{d}" for r in (3, 18) for d in DTYPES] + ["self_mask9_bf16", "self_fp8_bf16", "self_indexed_bf16"])


def _t5(src_len: int, tgt: int, dtype_name: str):
    from mapperatorinator_amd import Tokenizer
    from mapperatorinator_amd.modeling import MapperatorinatorHIP
    from mapperatorinator_amd.t5_engine import T5_PRESETS
    from mh_testing import random_t5_state_dict
    tok = Tokenizer.benchmark_vocab(src_seq_len=251)      # (the vocabulary does not follow the encoder length)
    dims = T5_PRESETS["tiny"]
    sd = random_t5_state_dict(dims, tok.vocab_size_in, tok.vocab_size_out, seed=11, lm_head_gain=6.0)
    model = MapperatorinatorHIP(sd, dims, vocab_size_in=tok.vocab_size_in, vocab_size_out=tok.vocab_size_out,
                                src_seq_len=src_len, tgt_seq_len=tgt, dtype=DTYPES[dtype_name], device="cuda:0")
    return tok, dims, model


def _forced(tok, prompt: torch.Tensor, tgt: int, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    forced = torch.randint(3, tok.vocab_size_out, (prompt.shape[0], tgt), generator=g)
    forced[:, :prompt.shape[1]] = prompt
    return forced


def _decode(tok, model, prompt, mask, tgt, seed, **kw) -> np.ndarray:
    from mapperatorinator_amd.server import build_sampling
    gk = dict(do_sample=False, num_beams=1, max_length=tgt, temperature=1.0, context_type="map", pad_token_id=0)
    sp, _ = build_sampling(tok, gk, tgt)
    out = model.engine.generate(kw.pop("audio", None), prompt, mask, [], sp, forced=_forced(tok, prompt, tgt, seed), dump_logits=True, **kw)
    lg = out["logits"].float().cpu().contiguous().numpy()
    assert lg.shape == (tgt, prompt.shape[0], tok.vocab_size_out), lg.shape
    return lg.view(np.uint32)


def _encoder_states(rows: int, src_len: int, d_model: int, seed: int) -> torch.Tensor:
    return torch.randn(rows, src_len, d_model, generator=torch.Generator().manual_seed(seed))


def _left_padded(tok, lens, width: int):
    g = torch.Generator().manual_seed(13)
    prompt = torch.zeros((len(lens), width), dtype=torch.long)
    for b, n in enumerate(lens):     # pad, sos, then ids above the specials
        prompt[b, width - n] = tok.sos_id
        prompt[b, width - n + 1:] = torch.randint(3, tok.vocab_size_out, (n - 1,), generator=g)
    return prompt, torch.arange(width)[None, :] >= torch.tensor([width - n for n in lens])[:, None]


def _cross(src_len: int, dtype_name: str, fp8: bool = False) -> np.ndarray:
    tgt = 1 + CROSS_NEW
    tok, dims, model = _t5(src_len, tgt, dtype_name)
    prompt = torch.full((CROSS_ROWS, 1), tok.sos_id)
    return _decode(tok, model, prompt, None, tgt, 5, encoder_states=_encoder_states(CROSS_ROWS, src_len, dims.d_model, 40 + src_len),
                   cross_kv_fp8=fp8)


def _cross_whisper() -> np.ndarray:
    from mapperatorinator_amd import Tokenizer
    from mapperatorinator_amd.modeling import MapperatorinatorHIP
    from mapperatorinator_amd.whisper_engine import VARWHISPER_PRESETS
    from mh_testing import random_varwhisper_state_dict, synthetic_audio_varied
    tgt = 1 + CROSS_NEW
    d = VARWHISPER_PRESETS["test"]
    tok = Tokenizer.benchmark_vocab(src_seq_len=WHISPER_FRAMES)
    sd = random_varwhisper_state_dict(d.d_model, d.n_heads, d.n_enc_layers, d.n_dec_layers, d.d_ff, tok.vocab_size_in,
                                      tok.vocab_size_out, seed=77, head_gain=5.0, gains={"decoder_embedder": 0.5})
    model = MapperatorinatorHIP(sd, d, vocab_size_in=tok.vocab_size_in, vocab_size_out=tok.vocab_size_out, n_mels=128,
                                src_seq_len=WHISPER_FRAMES, tgt_seq_len=tgt, dtype=torch.bfloat16, device="cuda:0", f_min=20)
    assert model.engine.packed.src_len == 129
    prompt = torch.full((CROSS_ROWS, 1), tok.sos_id)
    return _decode(tok, model, prompt, None, tgt, 5, audio=synthetic_audio_varied(CROSS_ROWS, (WHISPER_FRAMES - 1) * 128, seed=3))


def _self(rows: int, dtype_name: str, masked: bool = False, fp8: bool = False) -> np.ndarray:
    width = MASK_WIDTH if masked else 1
    tgt = 1 + SELF_NEW                             # 131 columns either way: positions 0 .. 130
    tok, dims, model = _t5(SELF_SRC, tgt, dtype_name)
    if masked:
        prompt, mask = _left_padded(tok, MASK_LENS, width)
    else:
        prompt, mask = torch.full((rows, 1), tok.sos_id), None
    return _decode(tok, model, prompt, mask, tgt, 6, encoder_states=_encoder_states(prompt.shape[0], SELF_SRC, dims.d_model, 50 + rows),
                   self_kv_fp8=fp8)


def _self_indexed() -> np.ndarray:
    """2 chunks x 2 beams through mh_t5_step_indexed, 131 positions; after every step each chunk's beams are re-drawn (repeats
    included, the identity on every fourth step), so that the table the next step reads through is not the identity."""
    from mh_testing import beam_skv8
    n_pos, G, nb = 1 + SELF_NEW, 2, 2
    tok, dims, model = _t5(SELF_SRC, n_pos, "bf16")
    eng = model.engine
    cfg = eng.packed.cfg
    g = torch.Generator().manual_seed(8)
    kv = (torch.randn(cfg.n_dec_layers, 2, G, cfg.n_heads, cfg.src_len, 64, generator=g) * 0.5).to(eng.device, eng.dtype).contiguous()
    ids = torch.randint(3, tok.vocab_size_out, (n_pos, G * nb), generator=g)
    pick = torch.randint(0, nb, (n_pos, G, nb), generator=g)
    pick[::4] = torch.arange(nb)
    srcs = (pick + torch.arange(G).view(1, G, 1) * nb).reshape(n_pos, G * nb).to(torch.int32).contiguous()
    assert 3 * int((srcs != torch.arange(G * nb)).any(dim=1).sum()) >= n_pos
    lg = beam_skv8.run_steps(eng, kv, None, ids, None, 1, nb, srcs, route="table", shadow=False)["logits"]
    lg = lg.float().contiguous().numpy()
    assert lg.shape == (n_pos, G * nb, tok.vocab_size_out), lg.shape
    return lg.view(np.uint32)


def run_case(name: str) -> np.ndarray:
    """-> the dumped scores (columns, rows, vocab_out) of case `name` (one of CASES) as uint32 bit patterns."""
    part = name.split("_")
    if name == "cross_whisper_L129_bf16":
        return _cross_whisper()
    if part[0] == "cross":
        return _cross(int(part[-2][1:]), part[-1], fp8=part[1] == "fp8")
    if name == "self_indexed_bf16":
        return _self_indexed()
    if part[1].startswith("rows"):
        return _self(int(part[1][4:]), part[2])
    return _self(len(MASK_LENS), "bf16", masked=part[1] == "mask9", fp8=part[1] == "fp8")


if __name__ == "__main__":
    import sys
    out = {}
    for case in CASES:
        for name, a in summarise(run_case(case)).items():
            out[f"{case}_{name}"] = a
        print("recorded", case, out[f"{case}_digest"].shape, flush=True)
    np.savez_compressed(sys.argv[1], **out)
    print("recorded", sys.argv[1])
