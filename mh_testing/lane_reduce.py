"""TEST SUPPORT: the decode run behind tests/golden/lane_reduce_tiny.npz (tests/test_gpu_lane_reduce.py).

The decode kernels' cross-lane reductions moved from `__shfl_xor` (LDS crossbar) to DPP / permlane forms with the same partner, level
order and operation; the fixture holds the processed scores of a short teacher-forced decode as the build BEFORE that change dumped
them, and the test compares a run of the current build bit for bit.  `decode_logits` is the one statement of the run, shared by the
test and by the recorder below (`python -m mh_testing.lane_reduce OUT.npz` on a GPU, with the build whose bits are to be recorded).

tiny T5, 251 frames, 3 rows (one chain), a 2-token prompt and 12 forced tokens: the scores of all 14 columns, fp32 and bf16 storage.
The fixture stays small: per (column, row) the first 16 bytes of the SHA-256 of the row's scores (equal digests = equal bits), and
the raw bits of SAMPLE_IDS evenly spread ids, so that a mismatch can be told apart as one ulp or garbage.
"""
from __future__ import annotations

import hashlib

import numpy as np
import torch

ROWS, PROMPT_LEN, NEW_TOKENS, FRAMES = 3, 2, 12, 251
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
SAMPLE_IDS = 8


def summarise(bits: np.ndarray) -> dict:
    """uint32 (columns, rows, V) -> dict(digest uint8 (columns, rows, 16), sample uint32 (columns, rows, SAMPLE_IDS))."""
    cols, rows, V = bits.shape
    bits = np.ascontiguousarray(bits, dtype="<u4")
    digest = np.zeros((cols, rows, 16), dtype=np.uint8)
    for c in range(cols):
        for r in range(rows):
            digest[c, r] = np.frombuffer(hashlib.sha256(bits[c, r].tobytes()).digest()[:16], dtype=np.uint8)
    ids = np.linspace(0, V - 1, SAMPLE_IDS).astype(np.int64)
    return dict(digest=digest, sample=bits[:, :, ids].astype(np.uint32))


def decode_logits(dtype_name: str) -> np.ndarray:
    """-> the dumped scores (columns, rows, vocab_out) of the run as uint32 bit patterns."""
    from mapperatorinator_amd import Tokenizer
    from mapperatorinator_amd.modeling import MapperatorinatorHIP
    from mapperatorinator_amd.server import build_sampling
    from mapperatorinator_amd.t5_engine import T5_PRESETS
    from mh_testing import random_t5_state_dict, synthetic_audio
    tok = Tokenizer.benchmark_vocab(src_seq_len=FRAMES)
    dims = T5_PRESETS["tiny"]
    tgt = PROMPT_LEN + NEW_TOKENS
    sd = random_t5_state_dict(dims, tok.vocab_size_in, tok.vocab_size_out, seed=11, lm_head_gain=6.0)
    model = MapperatorinatorHIP(sd, dims, vocab_size_in=tok.vocab_size_in, vocab_size_out=tok.vocab_size_out,
                                src_seq_len=FRAMES, tgt_seq_len=tgt, dtype=DTYPES[dtype_name], device="cuda:0")
    audio = synthetic_audio(ROWS, 32000, seed=4)
    prompt = torch.tensor([[0, 1], [1, 40], [1, 7]])
    g = torch.Generator().manual_seed(5)
    forced = torch.randint(3, tok.vocab_size_out, (ROWS, tgt), generator=g)
    forced[:, :PROMPT_LEN] = prompt
    gk = dict(do_sample=False, num_beams=1, max_length=tgt, temperature=1.0, context_type="map", pad_token_id=0)
    sp, _ = build_sampling(tok, gk, tgt)
    out = model.engine.generate(audio, prompt, prompt.ne(0), [], sp, forced=forced, dump_logits=True)
    lg = out["logits"].float().cpu().contiguous().numpy()
    assert lg.shape == (tgt, ROWS, tok.vocab_size_out), lg.shape
    return lg.view(np.uint32)


if __name__ == "__main__":
    import sys
    out = {}
    for k in DTYPES:
        for name, a in summarise(decode_logits(k)).items():
            out[f"{k}_{name}"] = a
    np.savez_compressed(sys.argv[1], **out)
    print("recorded", sys.argv[1])
