"""-m gpu: mh_beam_step past the LDS limit.  The streaming kernel (scores recomputed from the logits in every pass) must give the bits
of the LDS kernel wherever both run, choose ties the same way, and carry beam search at the released vocabulary (V >= 3837, up to
K = 5002 candidates) to the ids of the torch-op bookkeeping."""
import ctypes as C

import numpy as np
import pytest
import torch

from mapperatorinator_amd import _lib

pytestmark = pytest.mark.gpu

P, N_NEW = 2, 8
STATE = ("run", "rs", "rb", "seq", "bs", "bb", "fin")


@pytest.fixture
def path_option():
    lib = _lib.load()
    old = lib.mh_get_option(b"beam_step_path")
    yield lambda v: _lib.check(lib.mh_set_option(b"beam_step_path", v), "mh_set_option")
    lib.mh_set_option(b"beam_step_path", old)


def sampling(V, ts_start, ts_end, temperature=1.3, timeshift_bias=0.4, lookback_mask_end=0, cfg_scale=1.0):
    sp = _lib.MhSampling()
    sp.top_p, sp.temperature, sp.timeshift_bias = 1.0, temperature, timeshift_bias
    sp.ts_start, sp.ts_end, sp.n_sos, sp.lookback_mask_end = ts_start, ts_end, 1, lookback_mask_end
    sp.sos_ids[0] = 1
    sp.max_length, sp.cfg_scale = P + N_NEW, cfg_scale
    assert 0 <= ts_start < ts_end <= V
    return sp


def fresh_state(G, nb, fill, equal_scores=False):
    """`state()` of beam._beam_search_kernel: prompt [SOS, 7] in every row."""
    L = P + N_NEW
    run = torch.full((G, nb, L), fill, dtype=torch.int32, device="cuda")
    run[:, :, 0], run[:, :, 1] = 1, 7
    rs = torch.zeros((G, nb), dtype=torch.float32, device="cuda")
    if not equal_scores:
        rs[:, 1:] = -1e9
    return dict(run=run, rs=rs, rb=torch.full((G, nb, N_NEW), -1, dtype=torch.int32, device="cuda"), seq=run.clone(),
                bs=torch.full((G, nb), -1e9, dtype=torch.float32, device="cuda"),
                bb=torch.full((G, nb, N_NEW), -1, dtype=torch.int32, device="cuda"),
                fin=torch.zeros((G, nb), dtype=torch.uint8, device="cuda"))


def run_chain(path, set_path, G, nb, V, eos, sp, logits_per_step, cfg=False, equal_scores=False, engage=True):
    """`len(logits_per_step)` chained mh_beam_step launches under beam_step_path = `path`; returns per step every OUT array and
    src / last / flags / heuristic_open as CPU tensors."""
    lib = _lib.load()
    set_path(path)
    K = min(max(2, 1 + len(eos)) * nb, nb * V)
    assert lib.mh_beam_step_path(nb, V, K) == (path or 1), (nb, V, K, path)
    R = G * nb
    RE = 2 * R if cfg else R
    eos_table = torch.zeros(V, dtype=torch.uint8, device="cuda")
    if eos:
        eos_table[torch.tensor(eos, dtype=torch.long, device="cuda")] = 1
    st = [fresh_state(G, nb, eos[0] if eos else -1, equal_scores) for _ in range(2)]
    heuristic_open = torch.ones(G, dtype=torch.uint8, device="cuda")
    src = torch.zeros(RE, dtype=torch.int32, device="cuda")
    last = torch.zeros(RE, dtype=torch.int32, device="cuda")
    flags = torch.zeros((G, 3), dtype=torch.int32, device="cuda")
    logits = torch.empty((RE, V), dtype=torch.float32, device="cuda")
    bs = _lib.MhBeamStep()
    bs.logits, bs.eos_table = logits.data_ptr(), eos_table.data_ptr()
    bs.G, bs.num_beams, bs.V, bs.P, bs.max_length, bs.K = G, nb, V, P, P + N_NEW, K
    bs.cfg, bs.cfg_scale, bs.length_penalty, bs.early_stopping = int(cfg), float(sp.cfg_scale), 1.0, 0
    bs.sp = sp
    bs.heuristic_open, bs.src, bs.last, bs.flags = heuristic_open.data_ptr(), src.data_ptr(), last.data_ptr(), flags.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    out, par, cur_len = [], 0, P
    for lg in logits_per_step:
        assert lg.shape == (RE, V)
        logits.copy_(lg)
        a, b = st[par], st[par ^ 1]
        bs.cur_len = cur_len
        for k in STATE:
            setattr(bs, k + "_in", a[k].data_ptr())
            setattr(bs, k + "_out", b[k].data_ptr())
        _lib.check(lib.mh_beam_step(C.byref(bs), stream), "mh_beam_step")
        torch.cuda.synchronize()
        snap = {k: b[k].cpu() for k in STATE}
        snap.update(src=src.cpu(), last=last.cpu(), flags=flags.cpu(), heuristic_open=heuristic_open.cpu())
        out.append(snap)
        if engage:      # a TIME_SHIFT as the new last token of every other beam: MonotonicTimeShift masks a different span per beam
            for j in range((cur_len) % 2, nb, 2):
                b["run"][:, j, cur_len] = sp.ts_start + 3 + (j * 5 + cur_len * 11) % 60
        par ^= 1
        cur_len += 1
    return out


def assert_same_bits(a, b, what):
    assert len(a) == len(b)
    for step, (x, y) in enumerate(zip(a, b)):
        for k in x:
            same = torch.equal(x[k].view(torch.int32), y[k].view(torch.int32)) if x[k].dtype == torch.float32 else torch.equal(x[k], y[k])
            assert same, f"{what}: step {step}: `{k}` differs between the LDS and the streaming kernel"


def random_logits(steps, rows, V, seed):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(rows, V, generator=gen) * 6.0 for _ in range(steps)]


CHAINS = {   # G, nb, V, #eos, guidance, lookback
    "g3_b2_v2080": (3, 2, 2080, 0, False, False),
    "g2_b3_v2081_e40": (2, 3, 2081, 40, False, False),
    "g1_b5_v1849_e300": (1, 5, 1849, 300, False, False),
    "g2_b8_v517_e2": (2, 8, 517, 2, False, False),
    "g2_b3_v2080_e40_cfg": (2, 3, 2080, 40, True, False),
    "g2_b2_v2080_lookback": (2, 2, 2080, 0, False, True),
}


@pytest.mark.parametrize("case", list(CHAINS))
def test_streaming_kernel_has_the_bits_of_the_lds_kernel(case, path_option):
    """Six chained steps on seeded logits (x 6), temperature 1.3, a TIME_SHIFT bias, MonotonicTimeShift engaged on every other beam:
    every OUT array and src / last / flags / heuristic_open bitwise equal after every step.  V 2081 / 1849 / 517 leave the 512-wide
    sweep and the 64-wide wave a ragged tail; at V 517 most waves' compaction slices are empty."""
    G, nb, V, n_eos, cfg, lookback = CHAINS[case]
    ts_start, ts_end = 16, 16 + 300
    gen = torch.Generator().manual_seed(n_eos + V)
    eos = sorted(set((torch.randperm(V - 3, generator=gen)[:n_eos] + 3).tolist()))
    sp = sampling(V, ts_start, ts_end, lookback_mask_end=ts_start + 20 if lookback else 0, cfg_scale=1.5 if cfg else 1.0)
    lg = random_logits(6, G * nb * (2 if cfg else 1), V, seed=V + nb)
    outs = [run_chain(path, path_option, G, nb, V, eos, sp, lg, cfg=cfg) for path in (1, 2)]
    assert_same_bits(outs[0], outs[1], case)
    first = outs[0][0]
    assert torch.isfinite(first["rs"]).all() and (first["last"][:G * nb] >= 0).all() and (first["last"] < V).all()
    if lookback:      # LookbackBias: nothing inside the masked span is ever fed on
        assert all(not ((o["last"] >= ts_start) & (o["last"] < ts_start + 20)).any() for o in outs[1])
    assert any((o["src"][:G * nb].view(G, nb) != torch.arange(G * nb, dtype=torch.int32).view(G, nb)).any() for o in outs[1]), \
        "no beam ever changed its parent: the case does not exercise the reorder"


def test_automatic_dispatch_still_launches_the_lds_kernel_where_it_fits(path_option):
    """beam_step_path = 0 at (2 beams, V 2080): the LDS kernel (mh_beam_step_path says 1), with the bits of the forced LDS launch."""
    G, nb, V = 3, 2, 2080
    path_option(0)
    assert _lib.load().mh_beam_step_path(nb, V, 2 * nb) == 1
    sp = sampling(V, 16, 316)
    lg = random_logits(3, G * nb, V, seed=5)
    assert_same_bits(run_chain(0, path_option, G, nb, V, [], sp, lg), run_chain(1, path_option, G, nb, V, [], sp, lg), "automatic")


def test_ties_go_to_the_smallest_flat_index_on_both_paths(path_option):
    """Four equal rows with equal running scores: 5.0 at two EOS columns (8 entries above the K-th value), 3.0 at columns 50 / 900 /
    1500 (12 entries AT the K-th value of K = 12, four of them wanted), 0 elsewhere.  The ties of smallest flat index are
    (beam 0: 50, 900, 1500), (beam 1: 50): none of them an EOS, so they are exactly the next running beams, in that order."""
    G, nb, V = 2, 4, 2080
    eos = [100, 700]
    row = torch.zeros(V)
    row[eos] = 5.0
    row[[50, 900, 1500]] = 3.0
    lg = [row.expand(G * nb, V).contiguous()]
    sp = sampling(V, 2000, 2050, temperature=1.0, timeshift_bias=0.0)
    outs = [run_chain(path, path_option, G, nb, V, eos, sp, lg, equal_scores=True, engage=False) for path in (1, 2)]
    assert_same_bits(outs[0], outs[1], "ties")
    for o in outs:
        o = o[0]
        assert o["last"].view(G, nb).tolist() == [[50, 900, 1500, 50]] * G
        assert o["src"].view(G, nb).tolist() == [[g * nb, g * nb, g * nb, g * nb + 1] for g in range(G)]
        assert o["run"][:, :, P].tolist() == [[50, 900, 1500, 50]] * G
        assert o["fin"].tolist() == [[1] * nb] * G and sorted(o["seq"][0, :, P].tolist()) == [100, 100, 700, 700]
        rs = o["rs"]
        assert torch.equal(rs, rs[:1, :1].expand_as(rs))                  # one value: the ties were ties


# ---- past the old limit, end to end -----------------------------------------------------------------------------------------------

def gen_kwargs(tgt, **over):
    kw = dict(precision="fp32", do_sample=False, num_beams=1, top_p=1.0, top_k=0, max_length=tgt, cfg_scale=1.0,
              timeshift_bias=0, types_first=False, temperature=1.0, lookback_time=0, lookahead_time=0,
              context_type="map", pad_token_id=0)
    kw.update(over)
    return kw


SRC, TGT = 64, 24
_MODELS = {}


def large_vocab_model(seed):
    """Tiny T5 over the benchmark vocabulary with DISTANCE widened to 0 .. 3600: 3859 output ids (odd, past the released 3837)."""
    from mapperatorinator_amd import EventType, Tokenizer
    from mapperatorinator_amd.modeling import MapperatorinatorHIP
    from mapperatorinator_amd.t5_engine import T5_PRESETS
    from mapperatorinator_amd.tokenizer import _TAIL
    from mh_testing import DIVERSE_GAINS, random_t5_state_dict
    if seed not in _MODELS:
        tok = Tokenizer.from_ranges([(EventType.TIME_SHIFT, 0, 50), (EventType.SNAPPING, 0, 16), (EventType.DISTANCE, 0, 3600)] + _TAIL)
        assert tok.vocab_size_out >= 3837 and tok.vocab_size_out % 2 == 1
        sd = random_t5_state_dict(T5_PRESETS["tiny"], tok.vocab_size_in, tok.vocab_size_out, seed=seed, lm_head_gain=6.0, gains=DIVERSE_GAINS)
        model = MapperatorinatorHIP(sd, T5_PRESETS["tiny"], vocab_size_in=tok.vocab_size_in, vocab_size_out=tok.vocab_size_out,
                                    src_seq_len=SRC, tgt_seq_len=TGT, dtype=torch.float32, device="cuda")
        _MODELS.clear()
        _MODELS[seed] = (tok, model)
    return _MODELS[seed]


@pytest.mark.parametrize("beams,n_eos,guided,path", [(8, 2, False, 2), (8, 300, False, 2), (5, 700, False, 1), (2, 2500, False, 2),
                                                     (4, 2, True, 1), (8, 2, True, 2)])
def test_beam_search_past_the_lds_limit_matches_torch_bookkeeping(beams, n_eos, guided, path):
    """The recipe of test_beam_step_kernel_matches_torch_bookkeeping_across_candidate_counts at V = 3859: 8 beams (123 488 B of
    scores; with 300 EOS ids K = 2408), 2 beams with K = 5002 candidates, 8 beams under guidance -- all refused while LDS decided
    alone (`path` 2: the streaming kernel) --, and beside them 5 beams with K = 3505 and 4 guided beams, which the LDS kernel still
    holds at this vocabulary (`path` 1).  Same ids as the torch-op form (torch.topk over beams x V), token for token."""
    from mapperatorinator_amd.server import build_sampling
    from mh_testing import synthetic_audio_varied
    tok, model = large_vocab_model(11)
    eng = model.engine
    V = tok.vocab_size_out
    G = 2 if guided else 3
    assert G * beams * (2 if guided else 1) <= 64
    K = max(2, 1 + n_eos) * beams
    assert _lib.load().mh_beam_step_path(beams, V, K) == path
    audio = synthetic_audio_varied(G, (SRC - 1) * 128, seed=9).cuda()
    prompt = torch.tensor([[tok.sos_id, 0, 0], [tok.sos_id, 7, 0], [tok.sos_id, 9, 11]], dtype=torch.long)[:G]
    mask = prompt.ne(0)
    sp, _ = build_sampling(tok, gen_kwargs(TGT, num_beams=beams, cfg_scale=1.5 if guided else 1.0), TGT)
    extra = dict(negative_prompt=torch.tensor([[tok.sos_id, 5, 0], [tok.sos_id, 3, 13]], dtype=torch.long)) if guided else {}
    gen = torch.Generator().manual_seed(n_eos)
    eos = sorted(set((torch.randperm(V - 20, generator=gen)[:n_eos] + 20).tolist()))
    outs = [eng.generate_beam(audio, prompt, mask, eos, sp, beams, use_kernel=uk, **extra) for uk in (True, False)]
    assert torch.equal(outs[0]["tokens"], outs[1]["tokens"]), (outs[0]["tokens"].tolist(), outs[1]["tokens"].tolist())
    assert outs[0]["tokens"].shape[1] > prompt.shape[1]


def test_model_generate_with_eight_beams_reaches_the_kernel_at_the_large_vocabulary():
    """The public seam: `model_generate(num_beams=8)` at V = 3859 goes through _beam_search_kernel (it fell back to ~40 ATen launches
    per token before) and returns the ids of `beam_use_kernel=False`."""
    from mapperatorinator_amd import beam as _beam
    from mapperatorinator_amd.server import model_generate
    from mh_testing import synthetic_audio_varied
    tok, model = large_vocab_model(11)
    audio = synthetic_audio_varied(2, (SRC - 1) * 128, seed=4)
    prompt = torch.tensor([[tok.sos_id, 0, 0], [tok.sos_id, 9, 11]], dtype=torch.long)
    mk = dict(inputs=audio, decoder_input_ids=prompt, decoder_attention_mask=prompt.ne(0))
    kw = dict(num_beams=8, temperature=0.9, timeshift_bias=0.3, lookahead_time=300)
    calls = []
    orig = _beam._beam_search_kernel
    _beam._beam_search_kernel = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    try:
        ids_k, stats = model_generate(model, tok, mk, gen_kwargs(TGT, **kw))
    finally:
        _beam._beam_search_kernel = orig
    ids_t, _ = model_generate(model, tok, mk, gen_kwargs(TGT, beam_use_kernel=False, **kw))
    assert calls and stats["generated_tokens"] > 0
    assert np.array_equal(ids_k.numpy(), ids_t.numpy()), (ids_k.tolist(), ids_t.tolist())
