"""gpu: teacher-forced scoring on the device -- the row kernel (mh_score_rows) against the reference's five lines
(osuT5/osuT5/inference/processor.py:519-525), the whole pass (mh_t5_score, `model.score`, `server.model_score`) against the
row kernel on `forward`'s logits, and against the reference's own teacher-forced pass (tests/golden/score_t5_small.npz,
tools/make_score_golden.py).

Measured on one MI355X (printed by the tests, recorded in DESIGN.md):
  row kernel vs float64, worst |error| per scale group (kernel / the reference's fp32 evaluation): see DESIGN.md section 4.4.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from conftest import GOLDEN, t5_golden_case, vw_golden_case, wf_golden_case
from mapperatorinator_amd import _lib

pytestmark = pytest.mark.gpu

FIELDS = ("surprisal", "entropy", "relative", "logprob")
VOCABS = (1, 2, 63, 64, 65, 2080, 3837, 4096, 4097, 8192)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def score_rows(logits, target, V=None):
    """mh_score_rows on device tensors: logits fp32 (R, >= V) with any row stride, target (R,) -> dict of (R,) device tensors"""
    lib = _lib.load()
    R = logits.shape[0]
    V = logits.shape[1] if V is None else V
    assert logits.dtype == torch.float32 and logits.stride(1) == 1
    target = target.to(logits.device, torch.int32).contiguous()
    out = {k: torch.full((R,), float("nan"), dtype=torch.float32, device=logits.device) for k in FIELDS}
    best = torch.full((R,), -7, dtype=torch.int32, device=logits.device)
    rc = lib.mh_score_rows(logits.data_ptr(), logits.stride(0), R, V, target.data_ptr(), out["surprisal"].data_ptr(),
                           out["entropy"].data_ptr(), out["relative"].data_ptr(), out["logprob"].data_ptr(), best.data_ptr(), _stream())
    _lib.check(rc, "mh_score_rows")
    torch.cuda.synchronize()
    out["best_id"] = best
    return out


def five_lines(logits, tokens):
    """processor.py:519-525 as written, in the dtype of `logits` (+ the epsilon-free natural log-probability)"""
    probs = logits.softmax(dim=-1)
    entropy = -torch.sum(probs * torch.log2(probs + 1e-10), dim=-1)
    surprisal = -torch.log2(probs[torch.arange(len(tokens)), tokens] + 1e-10)
    relative = torch.where(entropy > 0, surprisal / entropy, torch.zeros_like(entropy))
    logprob = logits.log_softmax(dim=-1)[torch.arange(len(tokens)), tokens]
    return dict(surprisal=surprisal, entropy=entropy, relative=relative, logprob=logprob, best_id=logits.argmax(dim=-1))


SCALES = ("flat", "unit", "wide", "peaked")


def _rows(V, scale, gen, R=16):
    x = torch.randn(R, V, generator=gen)
    if scale == "flat":
        x = x * 0.01
    elif scale == "wide":
        x = x * 5
    elif scale == "peaked":          # one logit 40 above the rest: p of the others < 1e-10, the epsilon decides their terms
        x[torch.arange(R), torch.randint(0, V, (R,), generator=gen)] += 40.0 + x.max().item() - x.min().item()
    x = x.float()
    top = x.topk(min(2, V), dim=-1).values
    assert V == 1 or bool((top[:, 0] > top[:, 1]).all()), "inputs without ties"
    tgt = torch.randint(0, V, (R,), generator=gen)
    tgt[0] = x[0].argmax()
    tgt[1] = x[1].argmin()
    tgt[2] = -1
    tgt[3] = x[3].argmax()
    return x, tgt


def test_row_kernel_against_the_reference_formulas():
    """The tolerance is the reference's own: per quantity and per scale group, 4 x the worst error of the five lines evaluated
    in fp32 on the CPU (what the reference runs) against their float64 evaluation on the same logits, with a floor of 2 fp32
    ulps of the value.  (Within a scale group the conditioning is the same for every V; taken over all groups at once the
    peaked group's ill-conditioned relative surprisal -- entropy ~1e-12, also in the reference -- would void the check for
    the others.)  `relative` is additionally held to its definition on the kernel's own surprisal and entropy, exactly."""
    gen = torch.Generator().manual_seed(20)
    cases = [(V, s) + _rows(V, s, gen) for V in VOCABS for s in SCALES]
    ref_err = {s: {k: 0.0 for k in FIELDS} for s in SCALES}
    truth, ours = [], []
    for V, s, x, tgt in cases:
        scored = tgt >= 0
        t64 = five_lines(x.double(), tgt.clamp(min=0))
        r32 = five_lines(x, tgt.clamp(min=0))
        assert torch.equal(t64["best_id"], r32["best_id"])
        for k in FIELDS:
            ref_err[s][k] = max(ref_err[s][k], (r32[k].double() - t64[k])[scored].abs().max().item())
        truth.append(t64)
        pad = torch.full((x.shape[0], V + 3), 1e30)          # a row stride that is not V: the padding must never be read
        pad[:, :V] = x
        d = pad.cuda()
        got = score_rows(d, tgt, V)
        again = score_rows(d, tgt, V)
        for k in FIELDS + ("best_id",):
            assert torch.equal(got[k], again[k]), (V, s, k)                       # two runs: bit-identical
        tight = score_rows(x.cuda().contiguous(), tgt)
        for k in FIELDS + ("best_id",):
            assert torch.equal(got[k], tight[k]), (V, s, k)                       # the stride changes nothing
        ours.append({k: v.cpu() for k, v in got.items()})
    our_err = {s: {k: 0.0 for k in FIELDS} for s in SCALES}
    failures = []
    for (V, s, x, tgt), t64, got in zip(cases, truth, ours):
        scored = tgt >= 0
        assert torch.equal(got["best_id"][scored].long(), t64["best_id"][scored]), (V, s)
        assert bool((got["best_id"][~scored] == -1).all())
        for k in FIELDS:
            assert bool((got[k][~scored] == 0).all()), (V, s, k)                  # not scored: zeros
            err = (got[k].double() - t64[k]).abs()[scored]
            ulp = torch.from_numpy(np.spacing(t64[k][scored].abs().float().numpy())).double()
            tol = torch.maximum(torch.full_like(err, 4 * ref_err[s][k]), 2 * ulp)
            our_err[s][k] = max(our_err[s][k], err.max().item())
            if bool((err > tol).any()):
                failures.append((V, s, k, err.max().item(), tol.min().item()))
        want_rel = torch.where(got["entropy"] > 0, got["surprisal"] / got["entropy"], torch.zeros_like(got["entropy"]))
        assert torch.equal(got["relative"], want_rel), (V, s)
    for s in SCALES:
        print(f"row kernel, {s:7s}: worst |err| vs float64  kernel " + "  ".join(f"{k} {our_err[s][k]:.3e}" for k in FIELDS))
        print(f"            {s:7s}:                     reference fp32 " + "  ".join(f"{k} {ref_err[s][k]:.3e}" for k in FIELDS))
    assert not failures, failures


def test_row_kernel_ties_unscored_rows_and_out_of_range_targets():
    V = 5000
    x = torch.randn(6, V)
    x[0, [7, 300, 4097]] = 9.0                       # three equal maxima: the lowest index, as torch.argmax on the CPU
    x[1, [4999, 4096]] = 11.0
    x[2, :] = 0.5                                     # everything ties
    tgt = torch.tensor([7, 0, 1, -1, V, V + 100], dtype=torch.int32)
    got = score_rows(x.cuda(), tgt)
    assert got["best_id"].tolist() == [7, 4096, 0, -1, -1, -1]
    assert x[:3].argmax(-1).tolist() == [7, 4096, 0]
    for k in FIELDS:
        assert got[k][3:].tolist() == [0.0, 0.0, 0.0], k        # negative and >= V targets: not scored, the row is never indexed
    assert abs(got["entropy"][2].item() - math.log2(V)) < 1e-4 and abs(got["surprisal"][2].item() - math.log2(V)) < 1e-4
    # rows longer than the LDS stage (8192 floats) take the re-reading path
    V = 10000
    x = torch.randn(3, V) * 3
    tgt = torch.tensor([5, 9999, 8192], dtype=torch.int32)
    got = score_rows(x.cuda(), tgt)
    t64 = five_lines(x.double(), tgt.long())
    assert got["best_id"].cpu().long().tolist() == t64["best_id"].tolist()
    for k in FIELDS:
        assert torch.allclose(got[k].cpu().double(), t64[k], rtol=2e-6, atol=2e-6), k


# ---- the whole pass ------------------------------------------------------------------------------------------------------

def _t5_model(name, dtype):
    from mapperatorinator_amd.modeling import MapperatorinatorHIP
    from mapperatorinator_amd.t5_engine import T5_PRESETS
    g, size, tok, sd, audio, src, tgt = t5_golden_case(name)
    model = MapperatorinatorHIP(sd, T5_PRESETS[size], vocab_size_in=tok.vocab_size_in, vocab_size_out=tok.vocab_size_out,
                                src_seq_len=src, tgt_seq_len=tgt, dtype=dtype, device="cuda")
    return model, g, audio, {}


def _whisper_model(name, dtype):
    from mapperatorinator_amd.modeling import MapperatorinatorHIP
    if name.startswith("vw"):
        g, d, tok, sd, audio = vw_golden_case(name)
        model = MapperatorinatorHIP(sd, d, vocab_size_in=tok.vocab_size_in, vocab_size_out=tok.vocab_size_out, n_mels=128,
                                    src_seq_len=int(g["in_frames"]), tgt_seq_len=int(g["tgt_len"]), dtype=dtype, device="cuda", f_min=20)
        return model, g, audio, {}
    g, kind, d, tok, sd, audio, cond = wf_golden_case(name)
    model = MapperatorinatorHIP(sd, d, vocab_size_in=tok.vocab_size_in, vocab_size_out=tok.vocab_size_out, n_mels=int(g["n_mels"]),
                                src_seq_len=int(g["in_frames"]), tgt_seq_len=int(g["tgt_len"]), dtype=dtype, device="cuda",
                                f_min=0 if kind == "hf" else 20)
    return model, g, audio, cond or {}


def _inputs(g):
    prompt = torch.from_numpy(g["prompt"]).long()
    seq = torch.from_numpy(g["ids"]).long()[:, :-1].contiguous()
    mask = torch.ones_like(seq, dtype=torch.bool)
    mask[:, :prompt.shape[1]] = prompt.ne(0)
    return seq, mask


def _assert_same(got, want, where, what):
    """bit equality of the five arrays on the positions `where` (B, T) bool"""
    for k in FIELDS + ("best_id",):
        a, b = getattr(got, k) if not isinstance(got, dict) else got[k], want[k]
        a, b = a[where], b[where]
        same = torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b)
        assert same, (what, k, (a.double() - b.double()).abs().max().item())


def _check_whole_pass(model, seq, mask, audio, extra, what):
    """`model.score` == mh_score_rows on `model.forward(...).logits`, bit for bit: a block of the LM-head GEMM is planned as the
    forward's whole GEMM (same kernel, same k order), and a row's result does not depend on which rows share its tile."""
    from mapperatorinator_amd.t5_engine import next_token_targets
    B, T = seq.shape
    use_mask = None if bool(mask.all()) else mask
    logits = model.forward(frames=audio, decoder_input_ids=seq, decoder_attention_mask=use_mask, **extra).logits
    V = logits.shape[-1]
    tg = next_token_targets(seq, use_mask)
    want = score_rows(logits.view(B * T, V), tg.view(-1))
    want = {k: v.view(B, T) for k, v in want.items()}
    want["best_id"] = want["best_id"].long()
    real = mask.cuda()          # left-pad query rows hold unused garbage, but the SAME garbage on both routes: compared bitwise too
    scored = (tg >= 0).cuda()
    got = model.score(frames=audio, decoder_input_ids=seq, decoder_attention_mask=use_mask, **extra)
    assert got.surprisal.shape == (B, T) and got.best_id.dtype == torch.int64 and got.surprisal.is_cuda
    _assert_same(got, want, scored, what)
    for k in FIELDS:
        assert bool((getattr(got, k)[~scored] == 0).all()), (what, k)
    assert bool((got.best_id[~scored] == -1).all()) and bool((got.best_id[real & scored] >= 0).all())
    assert float(got.entropy[real & scored].min()) > 0
    # MaiMod's shape: an explicit span in the middle of every row (host targets: the engine counts them; device targets: it cannot)
    span = torch.zeros(B, T, dtype=torch.bool)
    span[:, T // 3: 2 * T // 3] = True
    span &= mask & (tg >= 0)
    assert int(span.sum()) > 0
    tg_span = torch.where(span, tg.long(), torch.full((B, T), -1))
    for targets in (tg_span, tg_span.cuda()):
        part = model.score(frames=audio, decoder_input_ids=seq, decoder_attention_mask=use_mask, targets=targets, **extra)
        _assert_same(part, want, span.cuda(), what + " span")
        for k in FIELDS:
            assert bool((getattr(part, k)[~span.cuda()] == 0).all()), (what, k)
        assert bool((part.best_id[~span.cuda()] == -1).all())
    # the block size changes nothing (here: many blocks, the last one partial)
    old = _lib.set_option("score_block_rows", 7)
    try:
        small = model.score(frames=audio, decoder_input_ids=seq, decoder_attention_mask=use_mask, **extra)
    finally:
        _lib.set_option("score_block_rows", old)
    _assert_same(small, want, scored, what + " block 7")
    with pytest.raises(ValueError, match="vocabulary"):
        model.score(frames=audio, decoder_input_ids=seq, decoder_attention_mask=use_mask, targets=torch.full((B, T), V), **extra)
    return got, want


@pytest.mark.parametrize("name,dtype", [("t5_tiny", torch.float32), ("t5_small", torch.float32), ("t5_small", torch.bfloat16),
                                        ("vw_test", torch.float32), ("rw_test", torch.float32), ("hfw_test", torch.float32)])
def test_whole_pass_equals_row_kernel_on_forward_logits(name, dtype):
    model, g, audio, extra = (_t5_model if name.startswith("t5") else _whisper_model)(name, dtype)
    seq, mask = _inputs(g)
    _check_whole_pass(model, seq, mask, audio, extra, f"{name} {dtype}")


def test_whole_pass_beyond_4096_output_ids():
    """vocab_out 4100 at tiny dims: the 4096-id boundary (the sampler's own) crossed in a whole pass, not only in the row kernel"""
    from mapperatorinator_amd.modeling import MapperatorinatorHIP
    from mapperatorinator_amd.t5_engine import T5_PRESETS
    from mh_testing import random_t5_state_dict, synthetic_audio
    vin, vout, src, tgt = 4200, 4100, 251, 40
    sd = random_t5_state_dict(T5_PRESETS["tiny"], vin, vout, seed=5, lm_head_gain=4.0)
    model = MapperatorinatorHIP(sd, T5_PRESETS["tiny"], vocab_size_in=vin, vocab_size_out=vout, src_seq_len=src, tgt_seq_len=tgt,
                                dtype=torch.float32, device="cuda")
    gen = torch.Generator().manual_seed(2)
    seq = torch.randint(3, vout, (3, 33), generator=gen)
    seq[:, -4:] = torch.tensor([4096, 4097, 4099, 4095])          # targets on both sides of the boundary
    seq[0, :2] = 0
    mask = seq.ne(0)
    seq[:, 2] = 1
    got, _ = _check_whole_pass(model, seq, mask, synthetic_audio(3, (src - 1) * 128, seed=3), {}, "tiny V=4100")
    high = seq[:, 1:].cuda() >= 4096                       # scored targets behind the boundary: really scored, ids stay in range
    assert int(high.sum()) >= 9 and bool((got.surprisal[:, :-1][high] > 0).all()) and bool((got.best_id[:, :-1][high] >= 0).all())
    assert int(got.best_id.max()) < vout


def _score_golden():
    from mapperatorinator_amd import Tokenizer
    from mapperatorinator_amd.modeling import MapperatorinatorHIP
    from mapperatorinator_amd.t5_engine import T5_PRESETS
    from mh_testing import DIVERSE_GAINS, random_t5_state_dict, synthetic_audio, synthetic_audio_varied
    g = np.load(f"{GOLDEN}/score_t5_small.npz")
    size = str(g["case"]).split("_")[1]
    src, tgt = int(g["src_len"]), int(g["tgt_len"])
    tok = Tokenizer.benchmark_vocab(src_seq_len=src)
    assert tok.vocab_size_out == int(g["vocab_out"]) and tok.vocab_size_in == int(g["vocab_in"])
    sd = random_t5_state_dict(T5_PRESETS[size], tok.vocab_size_in, tok.vocab_size_out, seed=int(g["weight_seed"]),
                              lm_head_gain=float(g["lm_head_gain"]), gains=DIVERSE_GAINS if str(g["gains"]) == "diverse" else None)
    audio = (synthetic_audio_varied if str(g["audio_kind"]) == "varied" else synthetic_audio)(g["prompt"].shape[0], int(g["n_samples"]),
                                                                                             seed=int(g["audio_seed"]))
    model = MapperatorinatorHIP(sd, T5_PRESETS[size], vocab_size_in=tok.vocab_size_in, vocab_size_out=tok.vocab_size_out,
                                src_seq_len=src, tgt_seq_len=tgt, dtype=torch.float32, device="cuda")
    return g, model, audio


def test_score_against_the_reference_golden():
    """The reference's `model_forward` logits reduced by its five lines (fp32, CPU) vs `model.score`.  The budget is the project's
    own for teacher-forced logits, delta = 5e-4 abs (stored in the golden); everything below is derived from it:
      surprisal: target logit and log-sum-exp each move by <= delta      -> |d| <= 2 delta / ln 2 bits, where p[target] > 1e-6
                 (below that the epsilon flattens the reference's value and the first-order bound does not describe it)
      logprob:   the same two terms, no epsilon                          -> |d| <= 2 delta nats
      entropy:   first order sum p |ln p + H| <= 2 H <= 2 ln V            -> |d| <= 2 delta log2 V bits
      relative:  s / e with both moved                                   -> (ds e + s de) / (e (e - de)), where e > 0.1 bit
      best_id:   equal where the reference's top-2 logit gap > 2 delta
    At most 1 % of the scored positions may fall outside the relative / best_id conditions."""
    g, model, audio = _score_golden()
    delta = float(g["delta"])
    V = int(g["vocab_out"])
    seq, mask, tg = torch.from_numpy(g["ids"]).long(), torch.from_numpy(g["mask"]), torch.from_numpy(g["targets"]).long()
    got = model.score(frames=audio, decoder_input_ids=seq, decoder_attention_mask=mask, targets=tg)
    got = {k: getattr(got, k).cpu() for k in FIELDS + ("best_id",)}
    ref = {k: torch.from_numpy(g[k]) for k in FIELDS + ("best_id",)}
    scored = tg >= 0
    n = int(scored.sum())
    assert n > 150
    for k in FIELDS:
        assert bool((got[k][~scored] == 0).all())
    assert bool((got["best_id"][~scored] == -1).all())
    d_s, d_e, d_l = 2 * delta / math.log(2), 2 * delta * math.log2(V), 2 * delta
    err = {k: (got[k].double() - ref[k].double()).abs() for k in FIELDS}
    likely = scored & (torch.from_numpy(g["p_target"]) > 1e-6)
    e_ok = scored & (ref["entropy"] > 0.1)
    gap_ok = scored & (torch.from_numpy(g["top2_gap"]) > 2 * delta)
    e, s = ref["entropy"].double(), ref["surprisal"].double()
    d_r = (d_s * e + s * d_e) / (e * (e - d_e))
    print(f"score vs reference golden ({n} positions): worst |d| surprisal {err['surprisal'][likely].max():.3e} (bound {d_s:.3e}), "
          f"entropy {err['entropy'][scored].max():.3e} (bound {d_e:.3e}), logprob {err['logprob'][likely].max():.3e} (bound {d_l:.3e}), "
          f"relative {err['relative'][e_ok].max():.3e} (bound at that position {d_r[e_ok][err['relative'][e_ok].argmax()]:.3e}); "
          f"outside: p<=1e-6 {n - int(likely.sum())}, entropy<=0.1 {n - int(e_ok.sum())}, gap<=2delta {n - int(gap_ok.sum())}")
    assert (n - int(e_ok.sum())) * 100 <= n and (n - int(gap_ok.sum())) * 100 <= n
    assert bool((err["surprisal"][likely] <= d_s).all())
    assert bool((err["logprob"][likely] <= d_l).all())
    assert bool((err["entropy"][scored] <= d_e).all())
    assert bool((err["relative"][e_ok] <= d_r[e_ok]).all())
    assert torch.equal(got["best_id"][gap_ok], ref["best_id"][gap_ok].long())


def test_server_seams_end_to_end():
    from mapperatorinator_amd import model_forward, model_score
    model, g, audio, _ = _t5_model("t5_small", torch.float32)
    seq, mask = _inputs(g)
    mk = dict(inputs=audio, decoder_input_ids=seq, decoder_attention_mask=mask)
    want = model.score(frames=audio, decoder_input_ids=seq, decoder_attention_mask=mask)
    got = model_score(model, dict(mk), dict(precision="fp32", cfg_scale=1.0))
    for k in FIELDS + ("best_id",):
        assert got[k].device.type == "cpu" and torch.equal(got[k], getattr(want, k).cpu()), k
    tg = torch.full(seq.shape, -1)
    tg[:, 10:20] = seq[:, 11:21]
    part = model_score(model, dict(mk), dict(cfg_scale=1.0), targets=tg)
    assert torch.equal(part["surprisal"][:, 10:20], got["surprisal"][:, 10:20]) and float(part["surprisal"][:, :10].abs().sum()) == 0
    assert bool((part["best_id"][:, 20:] == -1).all())
    logits = model_forward(model, dict(mk), dict(precision="fp32", cfg_scale=1.0))
    assert logits.device.type == "cpu" and logits.dtype == torch.float32
    assert torch.equal(logits, model.forward(frames=audio, decoder_input_ids=seq, decoder_attention_mask=mask).logits.cpu())
    with pytest.raises(ValueError, match="cfg_scale"):
        model_score(model, dict(mk), dict(cfg_scale=2.0))
