"""Writes tests/golden/t5_tiny_tf_beam.npz: the reference's beam search under LookbackBiasLogitsWarper(types_first=True).

The unmodified reference is imported through oracle/ref_harness.py (as oracle/make_golden.py does), on the model of
oracle/make_golden.py:TF_CASE (`build_reference_t5("tiny", types_first=True)`, `boost_timed_rows`, the tokenizer of
tests/golden/tokenizer_types_first.json).  Per run of RUNS: the ids its `model_generate` returned through HF beam search.  For the
run RECORD, HF's `LogitsProcessorList.__call__` is wrapped and (input_ids, scores in, scores out) of the first RECORD_STEPS
generated steps are stored too: what `BeamProcessors` is replayed against (tests/test_beam_types_first_cpu.py).  The warper keeps
`last_scores` by ROW SLOT while HF reorders the beams between two steps; the tool counts the recorded row-steps that renormalise in
a slot whose beam changed, i.e. where gathering the state by beam index would give another answer.

Printed per run: how many row-steps renormalised, in how many positions the ids differ from the same beams with the warper switched
off (its `__call__` replaced by the identity for that one run), and the smallest gap that decided anything -- between neighbours
among the first num_beams + 1 candidates, and among the first num_beams + 1 candidates that did not hit a stopping criterion (the
last selected against the first rejected running beam, and the order of the selected ones: the slot order is what the by-slot state
depends on).  The runs are chosen so that it exceeds 1e-3, twice the 5e-4 a processed score may differ by on the GPU: a bit-exact
id comparison then never decides a rounding tie.

    python tools/make_beam_tf_golden.py        (needs the reference checkout; run from the repository root)
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mapperatorinator_amd.t5_engine import T5_PRESETS  # noqa: E402
from mh_testing import boost_timed_rows, random_t5_state_dict, synthetic_audio  # noqa: E402
from oracle import make_golden as mg  # noqa: E402
from oracle import ref_harness as rh  # noqa: E402
from oracle import ref_shims  # noqa: E402

MIN_GAP = 1e-3
RUNS = {
    # 3 beams, everything but guidance
    "tb3": dict(num_beams=3, types_first=True, temperature=1.1, timing_temperature=0.6, mania_column_temperature=0.8,
                taiko_hit_temperature=0.5, lookback_time=800, lookahead_time=400, timeshift_bias=0.2),
    # 2 beams under classifier-free guidance: the `all` run of TF_RUNS with beams
    "tb2g": dict(mg.TF_RUNS["all"], num_beams=2),
    # 2 beams whose ids depend on the warper.  Flat distributions on purpose: the EOS mass of the previous step (the state the warper
    # keeps by row slot) reaches 1e-3 and the lookback range holds a few percent, so that WHICH row's state a slot uses shows in
    # prob_eos_extra (at temperature ~1 this model's EOS mass is ~1e-8 and by-slot and by-beam state give the same scores)
    "tb2": dict(num_beams=2, types_first=True, temperature=3.0, timing_temperature=4.0, mania_column_temperature=0.8,
                taiko_hit_temperature=0.8, lookback_time=1500, timeshift_bias=0.5),
}
RECORD, RECORD_STEPS = "tb2", 9


def run(model, tok, audio, prompt, neg, kw, record=None, warper_off=False):
    """-> ids, stats of the run.  `record`: a list that receives (input_ids, scores in, scores out) per processor-list call."""
    ref_shims.install()
    from osuT5.osuT5.inference import logit_processors as lp
    from transformers import LogitsProcessorList
    from transformers.generation.utils import GenerationMixin
    stats = dict(renorm=0, rows=0, gap=float("inf"), renorm_rows=[])
    nb = kw["num_beams"]
    warper_call, list_call = lp.LookbackBiasLogitsWarper.__call__, LogitsProcessorList.__call__
    next_beams = GenerationMixin._get_running_beams_for_next_iteration

    def warper(self, input_ids, scores):
        out = warper_call(self, input_ids, scores)
        stats["rows"] += scores.shape[0]
        stats["renorm_rows"].append((out != scores).any(dim=-1))
        stats["renorm"] += int(stats["renorm_rows"][-1].sum())
        return scores if warper_off else out

    def plist(self, input_ids, scores, **k):
        x = scores.detach().float().cpu().clone()
        out = list_call(self, input_ids, scores, **k)
        if record is not None:
            record.append((input_ids.detach().cpu().clone(), x, out.detach().float().cpu().clone()))
        return out

    def running(self, topk_log_probs, topk_running_sequences, topk_running_beam_indices, next_token_hits_stopping_criteria, num_beams):
        for lp_row, hit in zip(topk_log_probs, next_token_hits_stopping_criteria):
            for v in (lp_row, lp_row[~hit]):
                v = v[:nb + 1]
                v = v[torch.isfinite(v)]
                if v.numel() > 1:
                    stats["gap"] = min(stats["gap"], float((v[:-1] - v[1:]).min()))
        return next_beams(self, topk_log_probs, topk_running_sequences, topk_running_beam_indices, next_token_hits_stopping_criteria,
                          num_beams)

    lp.LookbackBiasLogitsWarper.__call__, LogitsProcessorList.__call__ = warper, plist
    GenerationMixin._get_running_beams_for_next_iteration = running
    try:
        ids, _ = rh.reference_generate(model, tok, audio, prompt, rh.default_generate_kwargs(mg.TF_CASE["tgt"], **kw), prompt.ne(0),
                                       negative_prompt=neg if kw.get("cfg_scale", 1.0) > 1.0 else None)
    finally:
        lp.LookbackBiasLogitsWarper.__call__, LogitsProcessorList.__call__ = warper_call, list_call
        GenerationMixin._get_running_beams_for_next_iteration = next_beams
    return ids, stats


def main(runs=None, out_name="t5_tiny_tf_beam.npz"):
    runs = runs or RUNS
    c = mg.TF_CASE
    model, tok, _ = rh.build_reference_t5("tiny", src_seq_len=c["src"], tgt_seq_len=c["tgt"], types_first=True)
    with open(os.path.join(mg.OUT, "tokenizer_types_first.json")) as f:
        assert json.load(f) == json.loads(json.dumps(tok.state_dict())), "tests/golden/tokenizer_types_first.json is another tokenizer"
    sd = random_t5_state_dict(T5_PRESETS["tiny"], tok.vocab_size_in, tok.vocab_size_out, seed=c["weight_seed"],
                              lm_head_gain=c["lm_head_gain"])
    boost_timed_rows(sd, tok, c["timed_gain"])
    res = model.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys, res
    audio = synthetic_audio(len(c["prompt"]), c["n_samples"], seed=c["audio_seed"])
    prompt, neg = torch.tensor(c["prompt"]), torch.tensor(c["negative"])
    out = dict(vocab_in=tok.vocab_size_in, vocab_out=tok.vocab_size_out, prompt=prompt.numpy(), negative=neg.numpy(),
               runs=json.dumps(runs), record=RECORD, **{k: v for k, v in c.items() if k not in ("prompt", "negative")})
    for name, kw in runs.items():
        rec = [] if name == RECORD else None
        ids, st = run(model, tok, audio, prompt, neg, kw, record=rec)
        off, _ = run(model, tok, audio, prompt, neg, kw, warper_off=True)
        w = min(ids.shape[1], off.shape[1])
        differ = int((ids[:, :w] != off[:, :w]).sum()) + abs(ids.shape[1] - off.shape[1]) * ids.shape[0]
        print(f"{name}: ids {tuple(ids.shape)}; renormalised row-steps {st['renorm']} / {st['rows']}; ids differing from the beams "
              f"without the warper: {differ}; smallest deciding gap {st['gap']:.3e}")
        assert st["gap"] > MIN_GAP, f"{name}: choose other kwargs, a decision of this run is a rounding tie"
        assert differ > 0 and st["renorm"] > 0, f"{name}: choose other kwargs, the ids do not depend on the warper"
        out["ids_" + name] = ids.numpy()
        if rec is not None:
            rec = rec[:RECORD_STEPS]
            moved = 0
            for (a, _, _), (b, _, _), rows in zip(rec[:-1], rec[1:], st["renorm_rows"][1:]):
                moved += int(((b[:, :-1] != a).any(dim=-1) & rows).sum())
            print(f"{name}: {len(rec)} recorded steps of {rec[0][1].shape[0]} rows; renormalising rows whose slot held another beam one "
                  f"step earlier: {moved}")
            assert moved > 0, "record more steps or another run: by-slot and by-beam state cannot be told apart"
            out["rec_ids"] = np.stack([np.pad(a.numpy(), ((0, 0), (0, rec[-1][0].shape[1] - a.shape[1])), constant_values=-1)
                                       for a, _, _ in rec]).astype(np.int32)
            out["rec_in"] = torch.stack([x for _, x, _ in rec]).numpy()
            out["rec_out"] = torch.stack([x for _, _, x in rec]).numpy()
            out["rec_renorm"] = torch.stack(st["renorm_rows"][:len(rec)]).numpy()
    path = os.path.join(mg.OUT, out_name)
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 1 << 20, "record fewer steps: a committed file stays under 1 MiB"


if __name__ == "__main__":
    main()
