"""Writes tests/golden/score_t5_small.npz: the reference's teacher-forced pass reduced to MaiMod's per-position statistics.

The unmodified reference is imported through oracle/ref_harness.py (as oracle/make_golden.py does).  Seeded weights and audio
as the other T5 goldens (the t5_small case of oracle/make_golden.py with the LM-head gain below, chosen so that no scored
position is near-deterministic: the assertions at the end); the reference's greedy ids (left-padded prompts included) are fed
back teacher-forced through the reference's own `model_forward` (osuT5/osuT5/inference/server.py:159-181).  Its CPU fp32
logits are reduced by the five lines of `Processor.ai_mod` (osuT5/osuT5/inference/processor.py:519-525) in fp32 on the CPU; only
the (B, T) results are stored, plus the targets, the reference's probability of each target and its top-2 logit gap (the
conditions under which tests/test_gpu_score.py compares).

    python tools/make_score_golden.py        (needs the reference checkout; run from the repository root)
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import make_golden as mg  # noqa: E402
from oracle import ref_harness as rh  # noqa: E402
from oracle import ref_shims  # noqa: E402

DELTA = 5e-4     # the project's logits budget against the oracle (tests/test_gpu_t5.py, forward)
LM_HEAD_GAIN = 2.0


def main(name="t5_small"):
    ref_shims.install()
    from osuT5.osuT5.inference.server import model_forward
    from transformers.modeling_outputs import BaseModelOutput
    c = dict(mg.T5_CASES[name], gain=LM_HEAD_GAIN)
    model, tok, _ = rh.build_reference_t5(c["size"], src_seq_len=c["src"], tgt_seq_len=c["tgt"])
    res = model.load_state_dict(mg.case_weights(c, tok), strict=False)
    assert not res.unexpected_keys, res
    prompt = torch.tensor(c["prompts"])
    audio = mg.case_audio(c, len(c["prompts"]))
    full, _ = rh.reference_generate(model, tok, audio, prompt, rh.default_generate_kwargs(c["tgt"]), prompt.ne(0))
    full = full.to(torch.int64)
    seq = full[:, :-1].contiguous()
    mask = torch.ones_like(seq, dtype=torch.bool)
    mask[:, :prompt.shape[1]] = prompt.ne(0)
    enc = rh.reference_encode(model, audio)
    mk = dict(inputs=audio, encoder_outputs=BaseModelOutput(last_hidden_state=enc), decoder_input_ids=seq,
              decoder_attention_mask=mask)
    logits = model_forward(model, mk, dict(precision="fp32", cfg_scale=1.0))
    assert logits.dtype == torch.float32 and logits.shape == (*seq.shape, tok.vocab_size_out)
    # next-token targets; a position whose own input is left padding is garbage on every implementation: not scored
    targets = torch.where(mask, full[:, 1:], torch.full_like(seq, -1))
    scored = targets >= 0

    # the five lines, in fp32 on the CPU, per row as the reference evaluates them
    probs = logits.softmax(dim=-1)
    entropy = -torch.sum(probs * torch.log2(probs + 1e-10), dim=-1)
    p_target = probs.gather(-1, targets.clamp(min=0)[..., None])[..., 0]
    surprisal = -torch.log2(p_target + 1e-10)
    relative = torch.where(entropy > 0, surprisal / entropy, torch.zeros_like(entropy))
    best = logits.argmax(dim=-1)
    logprob = logits.log_softmax(dim=-1).gather(-1, targets.clamp(min=0)[..., None])[..., 0]
    top2 = logits.topk(2, dim=-1).values
    gap = top2[..., 0] - top2[..., 1]

    n = int(scored.sum())
    low_entropy = int((entropy[scored] <= 0.1).sum())
    small_gap = int((gap[scored] <= 2 * DELTA).sum())
    print(f"{name}: {n} scored positions of {seq.numel()}; entropy <= 0.1 bit: {low_entropy}; top-2 gap <= {2 * DELTA}: {small_gap}; "
          f"p[target] <= 1e-6: {int((p_target[scored] <= 1e-6).sum())}; entropy min / median {float(entropy[scored].min()):.3f} / "
          f"{float(entropy[scored].median()):.3f}")
    assert low_entropy == 0, "choose another seed / lm_head_gain: relative surprisal must be comparable everywhere"
    assert small_gap * 100 < n, "choose another seed / lm_head_gain: too many near-ties for the best_id comparison"
    for a in (surprisal, entropy, relative, logprob):
        a[~scored] = 0
    best[~scored] = -1
    out = os.path.join(mg.OUT, "score_" + name + ".npz")
    np.savez_compressed(out, case=name, delta=DELTA, vocab_in=tok.vocab_size_in, vocab_out=tok.vocab_size_out, n_samples=c["ns"],
                        src_len=c["src"], tgt_len=c["tgt"], weight_seed=c["wseed"], lm_head_gain=c["gain"], audio_seed=c["aseed"],
                        audio_kind=c["audio"], gains=c["gains"] or "", prompt=prompt.numpy(), ids=seq.numpy().astype(np.int32), mask=mask.numpy(),
                        targets=targets.numpy().astype(np.int32), surprisal=surprisal.numpy(), entropy=entropy.numpy(),
                        relative=relative.numpy(), logprob=logprob.numpy(), best_id=best.numpy().astype(np.int32),
                        p_target=p_target.numpy(), top2_gap=gap.numpy())
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
