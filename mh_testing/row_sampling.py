"""TEST SUPPORT: inputs and runners of tests/test_gpu_row_sampling.py (the row-settings decode, `mh_t5_generate_rows`; contract in
include/mapperhip.h).

The yardstick is the uniform entry: a row decoded in a mixed call must equal, bit for bit, the same row decoded in a uniform call made
of the rows that share its kwargs -- token ids up to the row's end and its rows of the logits dump.  `run_uniform` and `run_rows` decode
over the same resident cross K/V and the same (left-padded) prompt columns, so a row sits at the same positions in both.

Tiny dims (d 128, 2 heads, 2 + 2 layers), 251 frames, tgt 48; seeded weights (lm_head_gain 6, DIVERSE_GAINS: greedy rows depend on
their audio and history)."""
from __future__ import annotations

import torch

from . import DIVERSE_GAINS, boost_timed_rows, random_t5_state_dict, synthetic_audio_varied

FRAMES, TGT = 251, 48
_MODELS, _KV = {}, {}


def tokenizer(kind: str, types_first_json: str = None):
    """`bench`: the benchmark vocabulary of a 251-frame window plus two context types (their EOS ids are what a context EOS set adds);
    `big`: the same with 6000 DISTANCE ids (more than 4096 ids: the sampler's memory path); `tf`: the types_first vocabulary of
    tests/golden (conditional-temperature token sets of all three rules)."""
    from mapperatorinator_amd import Tokenizer
    from mapperatorinator_amd.event import ContextType, EventType
    from mapperatorinator_amd.tokenizer import _TAIL
    if kind == "tf":
        return Tokenizer.from_json(types_first_json)
    max_ts = Tokenizer.benchmark_vocab(src_seq_len=FRAMES).event_range[EventType.TIME_SHIFT].max_value
    return Tokenizer.from_ranges([(EventType.TIME_SHIFT, 0, max_ts), (EventType.SNAPPING, 0, 16),
                                  (EventType.DISTANCE, 0, 6000 if kind == "big" else 640)] + _TAIL,
                                 context_types=[ContextType.MAP, ContextType.GD])


def model(kind: str, dtype, tok, options=None, fresh: bool = False):
    """one model per (vocabulary, storage dtype); `fresh`: an engine of its own (its workspaces are at other addresses)"""
    from mapperatorinator_amd.modeling import MapperatorinatorHIP
    from mapperatorinator_amd.t5_engine import T5_PRESETS
    key = (kind, dtype)
    if fresh or options is not None or key not in _MODELS:
        dims = T5_PRESETS["tiny"]
        sd = random_t5_state_dict(dims, tok.vocab_size_in, tok.vocab_size_out, seed=23, lm_head_gain=6.0, gains=DIVERSE_GAINS)
        if kind == "tf":   # random weights almost never emit a timed event: the types_first processors key on them
            boost_timed_rows(sd, tok, 3.0)
        m = MapperatorinatorHIP(sd, dims, vocab_size_in=tok.vocab_size_in, vocab_size_out=tok.vocab_size_out, src_seq_len=FRAMES,
                                tgt_seq_len=TGT, dtype=dtype, device="cuda", options=options)
        if fresh or options is not None:
            return m
        _MODELS[key] = m
    return _MODELS[key]


def cross_kv(m, kind: str, B: int):
    """resident cross K/V of B rows of varied audio, computed once per (model, B)"""
    key = (id(m), B)
    if key not in _KV:
        eng = m.engine
        audio = synthetic_audio_varied(B, (FRAMES - 1) * 128, seed=6)
        eng._enter()
        with eng.on_stream():
            kv = eng.cross_kv(eng.encode_mel(eng.mel(audio.to(eng.device, torch.float32))))
        eng._leave()
        eng.synchronize()
        _KV[key] = kv
    return _KV[key]


def prompts(tok, widths, seed: int = 3):
    """left-padded prompts (B, max width) int64 and their mask: sos, then ids that are no time shift and no EOS"""
    from mapperatorinator_amd.server import _ev
    g = torch.Generator().manual_seed(seed)
    lo = _ev(tok.event_end, "TIME_SHIFT")
    P = max(widths)
    ids = torch.full((len(widths), P), int(tok.pad_id), dtype=torch.int64)
    mask = torch.zeros((len(widths), P), dtype=torch.uint8)
    for r, w in enumerate(widths):
        ids[r, P - w:] = torch.randint(lo, tok.vocab_size_out, (w,), generator=g)
        ids[r, P - w] = tok.sos_id
        mask[r, P - w:] = 1
    return ids, mask


def gen_kwargs(**over):
    kw = dict(precision="fp32", do_sample=False, num_beams=1, top_p=1.0, top_k=0, max_length=TGT, cfg_scale=1.0, timeshift_bias=0,
              types_first=False, temperature=1.0, lookback_time=0, lookahead_time=0, context_type=None, pad_token_id=0)
    kw.update(over)
    return kw


def _decode(m, kv, prompt, mask, sp, eos_table, neg, row_sampling, modes):
    eng = m.engine
    dev = eng.device
    guided = neg is not None
    p_all = torch.cat([neg, prompt], 0) if guided else prompt
    m_all = None if mask is None else (torch.cat([mask, mask], 0) if guided else mask)
    eng._enter()
    with eng.on_stream():
        kv = kv.contiguous()
        kv8 = eng.cross_kv_fp8(kv) if modes.get("cross_kv_fp8") else None
        tokens, n_out, logits = eng.decode(kv, p_all.to(dev, torch.int32).contiguous(), None if m_all is None else m_all.to(dev).contiguous(),
                                           None if eos_table is None else eos_table.to(dev), sp, None, True, kv_fp8=kv8,
                                           self_kv_fp8=bool(modes.get("self_kv_fp8")), row_sampling=row_sampling)
    eng._leave()
    eng.synchronize()
    if guided:
        tokens = tokens[prompt.shape[0]:]
    return dict(tokens=tokens.cpu().to(torch.int64), n_cols=int(n_out.item()), logits=logits.cpu())


def run_uniform(m, tok, kv, prompt, mask, gk, rows, neg=None, **modes):
    """the uniform entry on `rows` (indices into the mixed call's rows) with the one kwargs dict `gk`"""
    from mapperatorinator_amd.server import build_sampling
    sp, eos = build_sampling(tok, gk, TGT)
    table = torch.zeros(tok.vocab_size_out, dtype=torch.uint8)
    table[torch.as_tensor(sorted(set(int(e) for e in eos)), dtype=torch.long)] = 1
    rows = torch.as_tensor(rows)
    out = _decode(m, kv[:, :, rows], prompt[rows], None if mask is None else mask[rows], sp, table, None if neg is None else neg[rows],
                  None, modes)
    out["eos"], out["cap"] = table, sp.max_length
    return out


def run_rows(m, tok, kv, prompt, mask, gks, neg=None, **modes):
    """the row form: one kwargs dict per returned row"""
    from mapperatorinator_amd.server import build_row_sampling
    rs = build_row_sampling(tok, gks, TGT)
    return _decode(m, kv, prompt, mask, rs[0], None, neg, rs, modes)


def row_end(tokens_row, P: int, eos_table, cap: int) -> int:
    """last column of a row: its first EOS-set id at or behind column P, else its cap's last column"""
    body = tokens_row[P:cap]
    hit = eos_table[body].nonzero()
    return P + int(hit[0]) if hit.numel() else cap - 1


def assert_rows_equal_uniform(mixed, uniform, rows, P: int, pad_id: int = 0):
    """every row of the uniform call `uniform` (made of the mixed call's rows `rows`) against the mixed call: token ids and the dumped
    scores of columns P .. end bit-equal, pad_id behind the end.  Returns the rows' ends."""
    ends = []
    for u, r in enumerate(rows):
        end = row_end(uniform["tokens"][u], P, uniform["eos"], uniform["cap"])
        assert end < uniform["n_cols"] <= uniform["cap"]
        assert torch.equal(mixed["tokens"][r, :end + 1], uniform["tokens"][u, :end + 1]), f"row {r}: ids differ from its uniform call"
        a, b = mixed["logits"][P:end + 1, r], uniform["logits"][P:end + 1, u]
        assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a[~torch.isnan(a)], b[~torch.isnan(b)]), \
            f"row {r}: processed scores differ from its uniform call"
        assert bool((mixed["tokens"][r, end + 1:mixed["n_cols"]] == pad_id).all()), f"row {r}: ids behind its end are not pad_id"
        ends.append(end)
    return ends
