"""-m gpu: mh_beam_step_sample -- beam-sample with HF's top-k / top-p warpers and the draw of the K continuations inside the beam
step kernel (csrc/beam.hip, `beam_step_kernel<kStream, kTf, kSample = true>`), both of its kernels, and `beam_search(device_draw=True)`
over it against the same rule in torch ops.

The kernel tests drive the entry through ctypes on synthetic logits and state.  What a step returns of its K draws is what HF's step
keeps of them: the running beams of the next step (the num_beams best non-EOS candidates of the K) and the hypotheses that just
finished (EOS candidates among the FIRST num_beams draws); the entry has no output that lists the K candidates themselves.  The draw
tests therefore restate the whole selection on the fp64 draw and compare every output that depends on it, bit for bit, and the
distribution test reads the first two draws of a chunk as the two hypotheses that finish when every id is an EOS id (an unordered
pair)."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import types_first_case
from mapperatorinator_amd import _lib
from mh_testing import beam_sample as bsr

pytestmark = pytest.mark.gpu

P, N_NEW = 2, 8
L = P + N_NEW
STATE = ("run", "rs", "rb", "seq", "bs", "bb", "fin")


@pytest.fixture
def path_option():
    lib = _lib.load()
    old = lib.mh_get_option(b"beam_step_path")
    yield lambda v: _lib.check(lib.mh_set_option(b"beam_step_path", v), "mh_set_option")
    lib.mh_set_option(b"beam_step_path", old)


def sampling(ts=(0, 0), top_k=0, top_p=1.0, seed=11, temperature=1.0, timeshift_bias=0.0, lookback_mask_end=0, cfg_scale=1.0, row0=0):
    sp = _lib.MhSampling()
    sp.do_sample, sp.top_k, sp.top_p, sp.seed, sp.rng_row0 = 1, top_k, top_p, seed, row0
    sp.temperature, sp.timeshift_bias = temperature, timeshift_bias
    sp.ts_start, sp.ts_end, sp.n_sos, sp.lookback_mask_end = ts[0], ts[1], 1, lookback_mask_end
    sp.sos_ids[0] = 1
    sp.max_length, sp.cfg_scale = L, cfg_scale
    return sp


def make_state(G, nb, fill, cur_len, rs=None, history=None):
    """`state()` of beam._beam_search_kernel at decode column `cur_len`: prompt [SOS, 7], then `history` (G, nb, cur_len - P) ids;
    rs None = the first step (beam 0 alive, the others at -1e9)."""
    run = torch.full((G, nb, L), fill, dtype=torch.int32)
    run[:, :, 0], run[:, :, 1] = 1, 7
    if history is not None:
        run[:, :, P:cur_len] = history
    if rs is None:
        rs = torch.zeros((G, nb))
        rs[:, 1:] = -1e9
    rb = torch.full((G, nb, N_NEW), -1, dtype=torch.int32)
    rb[:, :, :cur_len - P] = (torch.arange(G * nb, dtype=torch.int32).view(G, nb, 1))
    st = dict(run=run, rs=rs.float(), rb=rb, seq=run.clone(), bs=torch.full((G, nb), -1e9), bb=torch.full((G, nb, N_NEW), -1, dtype=torch.int32),
              fin=torch.zeros((G, nb), dtype=torch.uint8))
    return {k: v.contiguous() for k, v in st.items()}


def run_step(path, set_path, sp, logits, state, cur_len, eos, keep, K=None, cfg=False, tok_flags=None, lookback_prev=None, dump=True):
    """One mh_beam_step_sample launch under beam_step_path = `path`; every output as CPU tensors (+ `dump`, `lookback_prev`)."""
    lib = _lib.load()
    set_path(path)
    state = {k: v.cuda() for k, v in state.items()}
    G, nb, _ = state["run"].shape
    RE, V = logits.shape
    assert RE == G * nb * (2 if cfg else 1)
    K = min(max(2, 1 + len(eos)) * nb, nb * V) if K is None else K
    assert lib.mh_beam_step_path(nb, V, K) == (path or 1), (nb, V, K, path)
    eos_table = torch.zeros(V, dtype=torch.uint8, device="cuda")
    if len(eos):
        eos_table[torch.as_tensor(eos, dtype=torch.long, device="cuda")] = 1
    out = {k: torch.zeros_like(v) for k, v in state.items()}
    heuristic_open = torch.ones(G, dtype=torch.uint8, device="cuda")
    src = torch.zeros(RE, dtype=torch.int32, device="cuda")
    last = torch.zeros(RE, dtype=torch.int32, device="cuda")
    flags = torch.zeros((G, 3), dtype=torch.int32, device="cuda")
    lg = logits.cuda().contiguous()
    scores = torch.full((G, nb, V), float("nan"), dtype=torch.float32, device="cuda") if dump else None
    prev = None if lookback_prev is None else lookback_prev.clone().cuda()
    flags_d = None if tok_flags is None else torch.as_tensor(tok_flags, dtype=torch.uint8).cuda()
    bs = _lib.MhBeamStep()
    bs.logits, bs.eos_table = lg.data_ptr(), eos_table.data_ptr()
    bs.G, bs.num_beams, bs.V, bs.P, bs.max_length, bs.K, bs.cur_len = G, nb, V, P, L, K, cur_len
    bs.cfg, bs.cfg_scale, bs.length_penalty, bs.early_stopping = int(cfg), float(sp.cfg_scale), 1.0, 0
    bs.sp = sp
    if flags_d is not None:
        bs.sp.tok_flags = flags_d.data_ptr()
    bs.heuristic_open, bs.src, bs.last, bs.flags = heuristic_open.data_ptr(), src.data_ptr(), last.data_ptr(), flags.data_ptr()
    for k in STATE:
        setattr(bs, k + "_in", state[k].data_ptr())
        setattr(bs, k + "_out", out[k].data_ptr())
    _lib.check(lib.mh_beam_step_sample(C.byref(bs), _lib.ptr(prev), keep, _lib.ptr(scores), torch.cuda.current_stream().cuda_stream),
               "mh_beam_step_sample")
    torch.cuda.synchronize()
    res = {k: out[k].cpu() for k in STATE}
    res.update(src=src.cpu(), last=last.cpu(), flags=flags.cpu(), heuristic_open=heuristic_open.cpu())
    if dump:
        res["dump"] = scores.cpu()
    if prev is not None:
        res["lookback_prev"] = prev.cpu()
    return res


def assert_same_bits(x, y, what):
    for k in x:
        same = torch.equal(x[k].view(torch.int32), y[k].view(torch.int32)) if x[k].dtype == torch.float32 else torch.equal(x[k], y[k])
        assert same, f"{what}: `{k}` differs between the LDS and the streaming kernel"


# ---- 1. the warpers -----------------------------------------------------------------------------------------------------------------

SETTINGS = {   # top_k, top_p, #eos (min_tokens_to_keep = #eos + 1)
    "top_k": (5, 1.0, 1),
    "top_p": (0, 0.8, 1),
    "both": (12, 0.6, 1),
    "keep": (3, 0.9, 5),            # keep = 6 > top_k: TopK keeps 6, TopP never goes below 6
}
WARP_CASES = []
for _nb, _V in ((2, 37), (3, 2080), (8, 3837)):
    for _i, _s in enumerate(SETTINGS):
        WARP_CASES.append((_nb, _V, _s, "first" if _i % 2 == 0 else "later", _s == "both",
                           (_V, _s) in ((2080, "top_p"), (3837, "keep"))))


@pytest.mark.parametrize("nb,V,setting,step,cfg,tf", WARP_CASES, ids=[f"{c[0]}x{c[1]}-{c[2]}-{c[3]}{'-cfg' if c[4] else ''}{'-tf' if c[5] else ''}"
                                                                      for c in WARP_CASES])
def test_scores_after_the_warpers_match_beam_processors(nb, V, setting, step, cfg, tf, path_option):
    """`scores_dump` against BeamProcessors (pinned to HF's warpers by tests/test_host_cpu.py) in fp64 + the running score: the same
    -inf pattern, finite entries of every live row within 5e-4 (the project's processed-score bound).  A dead beam's row (running
    score -1e9, the first step) cannot meet an absolute bound: its score is the fp32 sum x - 1e9, one ulp of which is 64, so x itself
    is rounded away; those rows are held to the rounding of that sum, 2^-23 |score| (+ the 5e-4 of x).  2 x 37 (less than a wave), 3 x 2080 (LDS), 8 x 3837
    (streaming only); top-k only, top-p only, both (under guidance), keep = #eos + 1 > top_k; the first step (dead beams at -1e9) and
    a later one (MonotonicTimeShift engaged on every other beam); the types_first lookback renormalising on two cases.  The numpy
    rule asserts first that no group boundary's mass lies within 1e-4 of 1 - top_p, that the k'-th value is clear of the next one and
    that HF's element-wise warpers remove exactly the same ids (no tie straddles a boundary).  Where both kernels run, the dump and
    every output are bit-equal between them."""
    sp, logits, state, cur_len, eos, keep, flags, prev, want, ok = build_warp_case(nb, V, setting, step, cfg, tf, WARP_SEEDS[(V, setting)])
    assert ok, "the inputs sit on a boundary: pick another seed for this case"
    n_eos, R = len(eos), 2 * nb
    outs = {}
    for path in ((1, 2) if _lib.load().mh_beam_step_path(nb, V, max(2, 1 + n_eos) * nb) == 1 else (2,)):
        outs[path] = run_step(path, path_option, sp, logits, state, cur_len, eos, keep, cfg=cfg, tok_flags=flags, lookback_prev=prev)
        got = outs[path]["dump"].view(R, V).double().numpy()
        assert np.array_equal(np.isinf(got), np.isinf(want)), (path, int((np.isinf(got) != np.isinf(want)).sum()))
        fin = np.isfinite(want)
        err = np.abs(got[fin] - want[fin])
        dead = np.abs(want[fin]) >= 1e8
        print(f"path {path}: {int(fin.sum())} finite of {fin.size} ({int(dead.sum())} on dead rows), worst |dscore| on live rows {err[~dead].max():.2e}")
        assert (err[~dead] <= 5e-4).all()
        assert (err[dead] <= 5e-4 + 2.0 ** -23 * np.abs(want[fin][dead])).all()
        assert (np.isfinite(got).sum(1) >= min(keep, V)).all()
    if len(outs) == 2:
        assert_same_bits(outs[1], outs[2], setting)
    assert (2 in outs) and (V != 3837 or 1 not in outs)


# seeds at which the preconditions of build_warp_case hold (found on the CPU: the builder needs no device)
WARP_SEEDS = {(c[1], c[2]): 1 for c in WARP_CASES}      # (every case holds them at seed 1)


def build_warp_case(nb, V, setting, step, cfg, tf, seed):
    """Inputs of one warper case and their fp64 reference, on the CPU.  -> (sp, logits, state, cur_len, eos, keep, tok_flags,
    lookback_prev, reference scores (R, V) fp64, preconditions hold)."""
    from mapperatorinator_amd.beam import BeamProcessors
    G = 2
    top_k, top_p, n_eos = SETTINGS[setting]
    keep = n_eos + 1
    ts = (16, 30) if V == 37 else (16, 316)
    gen = torch.Generator().manual_seed(seed)
    eos = sorted(set((torch.randperm(V - 3, generator=gen)[:n_eos] + 3).tolist()))
    sp = sampling(ts, top_k, top_p, seed=V, temperature=1.3, timeshift_bias=0.4, cfg_scale=1.5 if cfg else 1.0,
                  lookback_mask_end=ts[0] + 6 if tf else 0)
    R = G * nb
    logits = torch.randn(R * (2 if cfg else 1), V, generator=gen) * 4.0
    cur_len = P if step == "first" else P + 2
    rs = history = None
    if step == "later":
        rs = -torch.rand(G, nb, generator=gen) * 3
        history = torch.randint(ts[1], V, (G, nb, 2), generator=gen, dtype=torch.int32) if V > 37 else torch.full((G, nb, 2), 33, dtype=torch.int32)
        history[:, ::2, 1] = ts[0] + 3                     # a TIME_SHIFT as the last id of every other beam
    flags = prev = None
    if tf:
        sp.lookback_types_first = 1
        flags = np.zeros(V, dtype=np.uint8)
        flags[ts[0]:ts[1]] |= 1                            # timed events
        flags[eos] |= 16
        sp.host_tok_flags = flags
        prev_scores = torch.log_softmax(torch.randn(R, V, generator=gen).double() * 2, -1)
        prev = torch.softmax(prev_scores, -1)[:, torch.from_numpy(flags & 16).bool()].sum(-1).float()
    state = make_state(G, nb, eos[0], cur_len, rs, history)
    # reference: fp64 log_softmax -> guidance -> the processor list with HF's warpers behind it
    ids = state["run"][:, :, :cur_len].reshape(R, cur_len).long()
    lsm = torch.log_softmax(logits.double(), -1)
    if cfg:
        lsm = lsm[R:] + (lsm[:R] - lsm[R:]) * 1.5
    procs = BeamProcessors(sp, "cpu", min_tokens_to_keep=keep)
    sp.do_sample = 0
    plain = BeamProcessors(sp, "cpu")
    if tf:
        procs.last_scores = plain.last_scores = prev_scores
    x = plain(ids, lsm).numpy()                            # what enters the warpers
    sp.do_sample = 1
    want = procs(ids, lsm).numpy() + state["rs"].double().view(R, 1).numpy()
    rule, margin, same = bsr.warped_scores(x, state["rs"].double().view(R).numpy(), top_k, top_p, keep)
    ok = margin > 1e-4 and same and np.array_equal(np.isinf(rule), np.isinf(want))
    if top_k:      # the k'-th value and the keep-th value clear of their neighbours
        srt = np.sort(x, axis=1)
        kk = min(max(top_k, keep), V)
        ok = ok and bool((srt[:, V - kk] - srt[:, V - kk - 1] > 1e-4).all())
    srt = np.sort(x, axis=1)
    ok = ok and bool((srt[:, V - keep] - srt[:, V - keep - 1] > 1e-4).all())
    return sp, logits, state, cur_len, eos, keep, flags, prev, want, ok


# ---- 2. the draw ----------------------------------------------------------------------------------------------------------------------

def restate_step(acc, draws, eos_mask, nb, V, cur_len):
    """HF's step on one chunk's K draws (flat indices in draw order; acc fp32 of every flat index), fresh finished set, fp32 like the
    kernel: -> (rs, last, src within the chunk) of the next running beams, (scores, tokens, flags) of the finished slots."""
    lp = acc[draws].astype(np.float32)
    hit = eos_mask[draws % V] | (cur_len + 1 >= L)
    run_lp = lp + np.where(hit, np.float32(-1e9), np.float32(-0.0))
    order = np.lexsort((np.arange(len(draws)), -run_lp.astype(np.float64)))[:nb]
    just = hit & (np.arange(len(draws)) < nb)
    sc = lp / np.float32(cur_len + 1 - P) + np.where(just, np.float32(-0.0), np.float32(-1e9))
    merged = np.concatenate([np.full(nb, -1e9, dtype=np.float32), sc])
    sel = np.lexsort((np.arange(len(merged)), -merged.astype(np.float64)))[:nb]
    fin_tok = [(-1 if m < nb else int(draws[m - nb] % V)) for m in sel]
    fin_flag = [(0 if m < nb else int(just[m - nb])) for m in sel]
    return (run_lp[order], draws[order] % V, draws[order] // V), (merged[sel], fin_tok, fin_flag)


DRAW_CASES = {"K4": 1, "K1402": 700}      # #eos


@pytest.mark.parametrize("case", list(DRAW_CASES))
def test_the_draw_equals_the_fp64_restatement(case, path_option):
    """512 chunks x 2 beams x V 2080 at a later step (live running scores), every score finite.
    K4: 1 EOS id, top_p 0.95, logits x 4.  A chunk is left out if two adjacent keys among its best K + 1 are closer than 1e-4.
    K1402: 700 EOS ids (K = 701 x 2), warpers off.  All 4160 keys are finite and ranked by the select, the compaction and the sort.
    The EOS ids' logits lie 25 above the others, so their 1400 candidates almost fill the K and the two or three places left go to
    whichever of the 2760 other candidates drew the largest keys: membership in the K alone decides the next running beams (asserted:
    in most chunks they are NOT the two best-scoring non-EOS candidates), and the first two draws finish as hypotheses.  With 1403
    finite keys below 64 in magnitude hardly a chunk has ALL adjacent gaps above 1e-4, so here a chunk is left out only on the gaps
    that decide what the step keeps (mh_testing.beam_sample.deciding_gap: among the first num_beams + 1 keys, and between the K-th
    and the (K + 1)-th); the order of the draws behind the top num_beams is read by nothing.
    The restatement draws in fp64 from the kernel's own `scores_dump` and the bit-exact u, runs HF's selection on its K draws, and
    every output that depends on the draw must be equal: running scores (bits), tokens, parents, finished scores (bits), tokens and
    flags.  1e-4 is about 25 fp32 ulps of a key below 64; at most 2 % of the chunks may be left out.  Both kernels, same bits."""
    n_eos = DRAW_CASES[case]
    G, nb, V, cur_len = 512, 2, 2080, P + 2
    K = (1 + n_eos) * nb if n_eos > 1 else 2 * nb
    keep = n_eos + 1
    gen = torch.Generator().manual_seed(n_eos + 5)
    eos = sorted(set((torch.randperm(V - 3, generator=gen)[:n_eos] + 3).tolist()))
    eos_mask = np.zeros(V, dtype=bool)
    eos_mask[eos] = True
    if case == "K4":
        sp = sampling((16, 316), 0, 0.95, seed=20260 + n_eos, row0=1000)
        logits = torch.randn(G * nb, V, generator=gen) * 4.0
    else:
        sp = sampling((0, 0), 0, 1.0, seed=20260 + n_eos, row0=1000)
        logits = torch.randn(G * nb, V, generator=gen) + 25.0 * torch.from_numpy(eos_mask).float()
    rs = -torch.rand(G, nb, generator=gen) * 3
    history = torch.randint(400, V, (G, nb, 2), generator=gen, dtype=torch.int32)
    state = make_state(G, nb, eos[0], cur_len, rs, history)
    outs = {path: run_step(path, path_option, sp, logits, state, cur_len, eos, keep, K=K) for path in (1, 2)}
    assert_same_bits(outs[1], outs[2], case)
    o = outs[1]
    acc = o["dump"].view(G, nb * V).numpy()
    assert np.isfinite(acc).all() if case == "K1402" else np.isfinite(acc).any(1).all()
    u = bsr.beam_uniform(int(sp.seed), 1000 + np.arange(G), cur_len, nb * V)
    left_out = by_membership = 0
    for g in range(G):
        draws, keys = bsr.draw(acc[g], u[g], K)
        assert np.abs(keys[np.isfinite(keys)]).max() < 64
        if case == "K4":
            with np.errstate(invalid="ignore"):                # (-inf next to -inf)
                gaps = keys[:-1] - keys[1:]
            gaps = gaps[np.isfinite(gaps)]
            gap = gaps.min() if gaps.size else np.inf
        else:
            gap = bsr.deciding_gap(keys, K, nb)
        if gap < 1e-4:
            left_out += 1
            continue
        (w_rs, w_last, w_par), (w_bs, w_tok, w_fin) = restate_step(acc[g], draws, eos_mask, nb, V, cur_len)
        assert np.array_equal(o["rs"][g].numpy().view(np.int32), w_rs.view(np.int32)), (g, o["rs"][g], w_rs)
        assert o["last"][g * nb:(g + 1) * nb].tolist() == w_last.tolist() and o["run"][g, :, cur_len].tolist() == w_last.tolist(), g
        assert (o["src"][g * nb:(g + 1) * nb] - g * nb).tolist() == w_par.tolist(), g
        assert np.array_equal(o["bs"][g].numpy().view(np.int32), w_bs.view(np.int32)), (g, o["bs"][g], w_bs)
        assert o["fin"][g].tolist() == w_fin, g
        assert [int(o["seq"][g, s, cur_len]) for s in range(nb) if w_fin[s]] == [t for t, f in zip(w_tok, w_fin) if f], g
        live = np.where(np.tile(eos_mask, nb), -np.inf, acc[g])
        by_membership += sorted((w_par * V + w_last).tolist()) != sorted(np.argsort(-live, kind="stable")[:nb].tolist())
    print(f"{case}: {left_out} of {G} chunks left out (deciding keys closer than 1e-4); in {by_membership} the running beams are not the best-scoring candidates")
    assert left_out <= 0.02 * G
    if case == "K1402":
        assert by_membership > G // 2 and o["fin"].all()


# ---- 3. the distribution ------------------------------------------------------------------------------------------------------------

CHI2_999_54 = 91.872      # 99.9 % quantile of chi-square at 54 degrees of freedom (55 unordered pairs of 11 live ids)


def test_first_two_draws_follow_plackett_luce(path_option):
    """The CPU test's shape (2 beams x 6 ids, one id masked, K = 4, 16 384 chunks as trials) on the kernel's draws, through both
    kernels.  Every id is an EOS id, so the two hypotheses that finish in a chunk ARE its first two draws, as an unordered pair (a
    step does not return the order inside the top num_beams): the chi-square of the 55 pairs against P(i, j) + P(j, i) of sequential
    sampling without replacement from softmax(scores_dump) must stay below the 99.9 % quantile at 54 degrees of freedom; cells with
    an expectation below 5 are pooled.  The masked id is never drawn.
    This test does NOT see the ORDER of the two draws (the issue's first-draw and ordered-pair statistics): no output of a step
    carries it.  Draw order is checked by the numpy rule on the CPU (tests/test_beam_sample_cpu.py: first draw and ordered pair against
    Plackett-Luce) and, for the kernel, through what depends on it -- the fp64 restatement above and the torch-form cross-check
    below, where "inside the first num_beams draws" decides which hypotheses finish."""
    nb, V = bsr.PL_X.shape
    G, K = bsr.PL_TRIALS, bsr.PL_K
    logits = torch.from_numpy(bsr.PL_X).float().repeat(G, 1)
    rs = torch.from_numpy(bsr.PL_RS).float().repeat(G, 1)
    sp = sampling(seed=bsr.PL_SEED)
    state = make_state(G, nb, 0, bsr.PL_COLUMN, rs, torch.full((G, nb, bsr.PL_COLUMN - P), 2, dtype=torch.int32))
    for path in (1, 2):
        o = run_step(path, path_option, sp, logits, state, bsr.PL_COLUMN, list(range(V)), 1, K=K)
        acc = o["dump"][0].view(-1).double().numpy()
        assert torch.equal(o["dump"], o["dump"][:1].expand_as(o["dump"])) and np.isinf(acc).sum() == 1
        assert o["fin"].all() and o["flags"][:, 1].all()
        parent = o["bb"][:, :, bsr.PL_COLUMN - P].long() - torch.arange(G).view(G, 1) * nb
        flat = (parent * V + o["seq"][:, :, bsr.PL_COLUMN].long()).numpy()
        assert (flat[:, 0] != flat[:, 1]).all() and np.isfinite(acc[flat]).all()
        w = np.where(np.isfinite(acc), np.exp(acc - acc[np.isfinite(acc)].max()), 0.0)
        W = w.sum()
        live = np.nonzero(w > 0)[0]
        obs, exp = [], []
        lo, hi = flat.min(1), flat.max(1)
        for a, i in enumerate(live):
            for j in live[a + 1:]:
                obs.append(int(((lo == i) & (hi == j)).sum()))
                exp.append(G * (w[i] / W * w[j] / (W - w[i]) + w[j] / W * w[i] / (W - w[j])))
        obs, exp = np.array(obs, dtype=np.float64), np.array(exp)
        small = exp < 5
        chi, cells = float((((obs - exp) ** 2) / exp)[~small].sum()), int((~small).sum())
        if small.any():
            chi, cells = chi + float((obs[small].sum() - exp[small].sum()) ** 2 / exp[small].sum()), cells + 1
        print(f"path {path}: chi-square {chi:.2f} over {cells} cells")
        assert cells == 55 and chi < CHI2_999_54
        # ... and the restatement draws the same pairs wherever fp32 keys cannot reorder them
        u = bsr.beam_uniform(bsr.PL_SEED, np.arange(G), bsr.PL_COLUMN, nb * V)
        checked = 0
        for g in range(0, G, 16):
            d, keys = bsr.draw(acc, u[g], K)
            if np.min(keys[:-1] - keys[1:]) >= 1e-4:
                checked += 1
                assert sorted(d[:2].tolist()) == sorted(flat[g].tolist()), g
        assert checked > 900


# ---- 4. bookkeeping, end to end -------------------------------------------------------------------------------------------------

def gen_kwargs(tgt, **over):
    kw = dict(precision="fp32", do_sample=False, num_beams=1, top_p=1.0, top_k=0, max_length=tgt, cfg_scale=1.0, timeshift_bias=0,
              types_first=False, temperature=1.0, lookback_time=0, lookahead_time=0, context_type="map", pad_token_id=0)
    kw.update(over)
    return kw


_CASE = {}


def tiny_model():
    """The model of the types_first fixtures (fp32, tiny dims, three ragged rows), built once for the module."""
    if not _CASE:
        from mapperatorinator_amd.modeling import MapperatorinatorHIP
        from mapperatorinator_amd.t5_engine import T5_PRESETS
        g, tok, sd, audio, tgt, _ = types_first_case()
        model = MapperatorinatorHIP(sd, T5_PRESETS["tiny"], vocab_size_in=tok.vocab_size_in, vocab_size_out=tok.vocab_size_out,
                                    src_seq_len=int(g["src"]), tgt_seq_len=tgt, dtype=torch.float32, device="cuda")
        _CASE["v"] = (g, tok, model, audio, tgt)
    return _CASE["v"]


E2E = {   # beams, #eos, guided, beam_step_path, top_k, top_p, seed
    "b2": (2, 2, False, 0, 0, 0.9, 5),
    "b3": (3, 2, False, 0, 20, 0.95, 6),
    "b2g": (2, 2, True, 0, 0, 0.9, 4),
    "b2_e700": (2, 700, False, 0, 0, 0.9, 4),
    "b3_stream": (3, 2, False, 2, 0, 0.9, 6),
}


@pytest.mark.parametrize("case", list(E2E))
def test_device_draw_kernel_matches_torch_bookkeeping(case, path_option, monkeypatch):
    """`generate_beam(device_draw=True)` through mh_beam_step_sample against the same rule in torch ops (`use_kernel=False`): equal
    tokens for 2 and 3 beams, under guidance, with an EOS set of 700 ids (K = 1402 candidates, hypotheses ending at different steps)
    and with the streaming kernel forced.  The seeds are those at which the torch form's smallest gap between two adjacent keys over
    the whole run (printed) is at least 1e-4, so that one fp32 ulp of a key cannot reorder a draw: among the keys that decide what a
    step keeps (mh_testing.beam_sample.deciding_gap, on the sorted keys `_device_draw` hands out through `keys_out`).  Recorded gaps at these seeds, 45 columns each: b2 3.73e-3, b3 2.02e-3, b2g 1.74e-2, b2_e700
    1.13e-2, b3_stream 1.78e-3 (of seeds 1 .. 8 every one gave equal tokens in every case; b2g at seed 1 has a gap of 3.8e-6)."""
    from mapperatorinator_amd import beam as _beam
    from mapperatorinator_amd.server import build_sampling
    beams, n_eos, guided, path, top_k, top_p, seed = E2E[case]
    g, tok, model, audio, tgt = tiny_model()
    prompt = torch.from_numpy(g["prompt"])
    G = 2 if guided else prompt.shape[0]
    prompt = prompt[:G]
    sp, _ = build_sampling(tok, gen_kwargs(tgt, num_beams=beams, do_sample=True, top_k=top_k, top_p=top_p, temperature=1.1,
                                           cfg_scale=1.5 if guided else 1.0), tgt)
    sp.seed = seed
    gen = torch.Generator().manual_seed(n_eos)
    eos = sorted(set((torch.randperm(tok.vocab_size_out - 20, generator=gen)[:n_eos] + 20).tolist()))
    extra = dict(negative_prompt=torch.roll(prompt, 1, 0)) if guided else {}      # (another row's prompt as the negative one)
    path_option(path)
    keys, orig = [], _beam._device_draw
    monkeypatch.setattr(_beam, "_device_draw", lambda *a, **k: orig(*a, keys_out=keys, **k))
    outs = [model.engine.generate_beam(audio[:G].cuda(), prompt, prompt.ne(0), eos, sp, beams, use_kernel=uk, device_draw=True, **extra)
            for uk in (True, False)]
    K = max(2, 1 + len(eos)) * beams
    gap = min(bsr.deciding_gap(row, K, beams) for step in keys for row in step.cpu().numpy())
    print(f"{case}: seed {seed}: smallest adjacent key gap of the torch form {gap:.3e}; {outs[0]['tokens'].shape[1] - prompt.shape[1]} columns")
    assert gap >= 1e-4, "pick another seed for this case"
    assert torch.equal(outs[0]["tokens"], outs[1]["tokens"]), (outs[0]["tokens"].tolist(), outs[1]["tokens"].tolist())
    assert outs[0]["tokens"].shape[1] > prompt.shape[1]


# ---- 5. repeatability and row independence ------------------------------------------------------------------------------------------

def test_same_seed_same_ids_and_chunks_draw_by_their_rng_row(path_option):
    G, nb, V, cur_len = 3, 2, 2080, P + 1
    gen = torch.Generator().manual_seed(9)
    logits = torch.randn(G * nb, V, generator=gen) * 2.0
    rs = -torch.rand(G, nb, generator=gen)
    history = torch.randint(400, V, (G, nb, 1), generator=gen, dtype=torch.int32)
    eos = [5, 9]
    state = make_state(G, nb, 5, cur_len, rs, history)

    def step(seed, row0=0, chunks=slice(None)):
        st = {k: v[chunks].contiguous() for k, v in state.items()}
        n = st["run"].shape[0]
        lg = logits.view(G, nb, V)[chunks].reshape(n * nb, V)
        return run_step(1, path_option, sampling((16, 316), 0, 0.95, seed=seed, row0=row0), lg, st, cur_len, eos, 3)
    a, b, c = step(41), step(41), step(42)
    assert_same_bits(a, b, "same seed")
    assert not torch.equal(a["last"], c["last"])
    for g in range(G):      # chunk g of the 3-chunk call = the 1-chunk call with rng_row0 = g
        one = step(41, row0=g, chunks=slice(g, g + 1))
        for k in ("run", "rs", "seq", "bs", "fin", "last", "dump"):
            assert torch.equal(one[k], a[k][g * nb:(g + 1) * nb] if k == "last" else a[k][g:g + 1]), (g, k)
        assert torch.equal(one["src"], a["src"][g * nb:(g + 1) * nb] - g * nb)


def test_model_generate_with_beam_sample_kernel(monkeypatch):
    """The public seam: generate kwarg `beam_sample_kernel=True` reaches mh_beam_step_sample; CPU int64 ids of the usual shape, the
    same for the same seed, others for another; `rng_row_offset` moves the draw."""
    from mapperatorinator_amd import beam as _beam
    from mapperatorinator_amd.server import model_generate
    g, tok, model, audio, tgt = tiny_model()
    prompt = torch.from_numpy(g["prompt"])
    mk = dict(inputs=audio, decoder_input_ids=prompt, decoder_attention_mask=prompt.ne(0))
    kw = dict(num_beams=2, do_sample=True, top_p=0.95, temperature=1.2, beam_sample_kernel=True, seed_call_index=0)
    calls, orig = [], _beam._beam_search_kernel
    monkeypatch.setattr(_beam, "_beam_search_kernel", lambda *a, **k: (calls.append(k.get("sample_keep")), orig(*a, **k))[1])
    ids, stats = model_generate(model, tok, mk, gen_kwargs(tgt, seed=3, **kw))
    again, _ = model_generate(model, tok, mk, gen_kwargs(tgt, seed=3, **kw))
    other, _ = model_generate(model, tok, mk, gen_kwargs(tgt, seed=4, **kw))
    moved, _ = model_generate(model, tok, mk, gen_kwargs(tgt, seed=3, rng_row_offset=100, **kw))
    assert len(calls) == 4 and all(c is not None and c >= 2 for c in calls)
    assert ids.dtype == torch.int64 and ids.device.type == "cpu" and ids.shape[0] == prompt.shape[0] and ids.shape[1] > prompt.shape[1]
    assert torch.equal(ids[:, :prompt.shape[1]], prompt) and stats["generated_tokens"] > 0
    assert torch.equal(ids, again)
    assert ids.shape != other.shape or not torch.equal(ids, other)
    assert ids.shape != moved.shape or not torch.equal(ids, moved)
