"""not gpu: teacher-forced scoring (mh_score_rows / mh_t5_score, `model_forward` / `model_score`) -- the parts that need no
device: symbols and ABI, argument validation, the workspace bound, the reference's own caller in front of our
`model_forward`, and the next-token target construction."""
import ctypes as C
import os
import re
import types

import pytest
import torch

from conftest import ROOT
from mapperatorinator_amd import _lib
from oracle import ref_shims

NEW = ("mh_score_rows", "mh_t5_score_workspace_bytes", "mh_t5_score")


def test_header_binding_and_library_agree_on_the_scoring_entry_points():
    hdr = open(os.path.join(ROOT, "include", "mapperhip.h")).read()
    declared = set(re.findall(r"\b(mh_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name in NEW:
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert re.search(r"#define MH_ABI_VERSION 11\b", hdr) and _lib.ABI_VERSION == 11 and lib.mh_abi_version() == 11
    import mapperatorinator_amd as pkg
    from mapperatorinator_amd import server
    assert pkg.model_forward is server.model_forward and pkg.model_score is server.model_score
    assert "model_forward" in pkg.__all__ and "model_score" in pkg.__all__


def _base_cfg(tgt_len=2560, vocab_out=3837, dtype=0):
    # osuT5-base dims (d_model 768, d_kv 64, d_ff 2048, 12 heads, 12 + 12 layers), 1251 frames
    return _lib.MhT5Config(d_model=768, d_kv=64, d_ff=2048, n_heads=12, n_enc_layers=12, n_dec_layers=12, vocab_in=4000,
                           vocab_out=vocab_out, n_mels=388, n_mels_pad=416, src_len=1251, tgt_len=tgt_len, dtype=dtype, eps=1e-6)


def test_scoring_argument_validation_without_gpu():
    lib = _lib.load()
    p = 4096            # a non-null "device pointer": validation must return before anything is dereferenced
    assert lib.mh_score_rows(None, 8, 1, 8, p, p, p, p, p, p, None) == -1 and b"null" in lib.mh_last_error()
    assert lib.mh_score_rows(p, 8, 1, 8, p, p, p, None, p, p, None) == -1 and b"null" in lib.mh_last_error()
    assert lib.mh_score_rows(p, 8, 0, 8, p, p, p, p, p, p, None) == -1 and b"R=0" in lib.mh_last_error()
    assert lib.mh_score_rows(p, 8, -3, 8, p, p, p, p, p, p, None) == -1
    assert lib.mh_score_rows(p, 8, 1, 0, p, p, p, p, p, p, None) == -1 and b"V=0" in lib.mh_last_error()
    assert lib.mh_score_rows(p, 7, 1, 8, p, p, p, p, p, p, None) == -1 and b"row_stride" in lib.mh_last_error()
    cfg = _base_cfg(tgt_len=96)
    assert lib.mh_t5_score_workspace_bytes(None, 1, 1) == -1
    assert lib.mh_t5_score_workspace_bytes(C.byref(cfg), 0, 4) == -1 and lib.mh_t5_score_workspace_bytes(C.byref(cfg), 2, 0) == -1

    weights = _lib.MhT5Weights()          # all-null tables: never read before the arguments are accepted

    def score(cfgp, w=C.byref(weights), kv=p, B=2, ids=p, T=8, targets=p, max_scored=0, out=p, ws=p, ws_bytes=1 << 40):
        return lib.mh_t5_score(cfgp, w, kv, B, ids, None, T, targets, max_scored, out, out, out, out, out, ws, ws_bytes, None)

    assert score(None) == -1 and b"null config" in lib.mh_last_error()
    assert score(C.byref(cfg), targets=None) == -1 and b"null argument" in lib.mh_last_error()
    assert score(C.byref(cfg), w=None) == -1 and b"null argument" in lib.mh_last_error()
    assert score(C.byref(cfg), out=None) == -1 and b"null argument" in lib.mh_last_error()
    assert score(C.byref(cfg), T=97) == -1 and b"tgt_len" in lib.mh_last_error()
    assert score(C.byref(cfg), T=0) == -1
    assert score(C.byref(cfg), B=0) == -1 and b"batch" in lib.mh_last_error()
    assert score(C.byref(cfg), ws_bytes=1024) == -1 and b"workspace too small" in lib.mh_last_error()
    bad = _base_cfg(tgt_len=96)
    bad.d_kv = 32
    assert score(C.byref(bad)) == -1 and b"d_kv" in lib.mh_last_error()


@pytest.mark.parametrize("dtype", [0, 1])
def test_score_workspace_does_not_grow_with_the_logits(dtype):
    """mh_t5_score never holds B*T*V logits: beyond the forward's workspace it needs one block of `score_block_rows` logits
    rows and hidden rows plus per-position indices.  The block size is read from the library, not restated here."""
    lib = _lib.load()
    Cb = lib.mh_get_option(b"score_block_rows")
    assert Cb > 0
    cfg = _base_cfg(dtype=dtype)
    V, d, tgt = cfg.vocab_out, cfg.d_model, cfg.tgt_len
    for B, T in ((1, 64), (32, 512), (32, tgt)):
        fwd = lib.mh_t5_forward_workspace_bytes(C.byref(cfg), B, T)
        sc = lib.mh_t5_score_workspace_bytes(C.byref(cfg), B, T)
        assert fwd > 0 and sc > fwd
        extra = sc - fwd
        print(f"B={B} T={T}: forward {fwd} B, score +{extra} B, logits would be {B * T * V * 4} B")
        assert extra < Cb * V * 4 + Cb * d * 4 + 64 * B * T + 4096, (B, T, extra)
    assert extra * 50 < 32 * tgt * V * 4
    # an engine's own block size is honoured (and shrinks the bound with it)
    opts = _lib.OptionSet(dict(score_block_rows=64))
    cfg.options = opts.handle
    small = lib.mh_t5_score_workspace_bytes(C.byref(cfg), 32, 512) - lib.mh_t5_forward_workspace_bytes(C.byref(cfg), 32, 512)
    assert small < 64 * V * 4 + 64 * d * 4 + 64 * 32 * 512 + 4096


def test_next_token_targets():
    from mapperatorinator_amd.t5_engine import next_token_targets
    ids = torch.tensor([[0, 0, 1, 7, 9], [1, 4, 5, 6, 2]])
    t = next_token_targets(ids)
    assert t.dtype == torch.int32 and t.tolist() == [[0, 1, 7, 9, -1], [4, 5, 6, 2, -1]]
    mask = torch.tensor([[0, 0, 1, 1, 1], [1, 1, 1, 1, 1]], dtype=torch.bool)
    t = next_token_targets(ids, mask)
    # the rule looks at the TARGET column only: position 1 (itself padding, its target the first real id) stays, position 0
    # (target column 1 is padding) and the last column are dropped
    assert t.tolist() == [[-1, 1, 7, 9, -1], [4, 5, 6, 2, -1]]
    t = next_token_targets(ids, mask.to(torch.uint8))
    assert t.tolist() == [[-1, 1, 7, 9, -1], [4, 5, 6, 2, -1]]
    assert next_token_targets(ids[:, :1]).tolist() == [[-1], [-1]]


class _RecordingModel:
    """Stands in for MapperatorinatorHIP on the CPU: keeps what `forward` / `score` are handed, answers with recognisable values;
    `prepare_inputs_for_generation` is the product's own."""
    device, dtype = torch.device("cpu"), torch.float32
    V = 11

    def __init__(self):
        from mapperatorinator_amd.modeling import MapperatorinatorHIP
        self._prep = MapperatorinatorHIP.prepare_inputs_for_generation
        self.forward_calls, self.score_calls = [], []

    def prepare_inputs_for_generation(self, *a, **k):
        return self._prep(self, *a, **k)

    def forward(self, **kw):
        self.forward_calls.append(kw)
        ids = kw["decoder_input_ids"]
        logits = ids[..., None].to(torch.float64) + torch.arange(self.V, dtype=torch.float64) / 16     # not fp32: the seam converts
        return types.SimpleNamespace(logits=logits)

    def score(self, **kw):
        self.score_calls.append(kw)
        ids = kw["decoder_input_ids"]
        f = ids.to(torch.float32)
        return types.SimpleNamespace(surprisal=f, entropy=f + 1, relative=f + 2, logprob=-f, best_id=ids.to(torch.int64))


def test_model_forward_and_model_score_seams_on_a_stand_in_model():
    from mapperatorinator_amd import server as our_server
    model = _RecordingModel()
    ids = torch.tensor([[0, 1, 5], [1, 6, 7]])
    mk = dict(inputs=torch.randn(2, 100), decoder_input_ids=ids, decoder_attention_mask=ids.ne(0), negative_prompt=None,
              negative_prompt_attention_mask=None, difficulty=torch.tensor([3.0, 4.0]))
    gk = dict(precision="fp32", cfg_scale=1.0)
    out = our_server.model_forward(model, mk, gk)
    assert gk == {}                                        # popped in place, as the reference does
    assert out.dtype == torch.float32 and out.device.type == "cpu" and out.shape == (2, 3, model.V)
    call = model.forward_calls[0]
    assert "inputs" not in call and torch.equal(call["frames"], mk["inputs"]) and torch.equal(call["difficulty"], mk["difficulty"])
    assert torch.equal(call["decoder_input_ids"], ids) and torch.equal(call["decoder_attention_mask"], ids.ne(0))
    tg = torch.tensor([[-1, 5, -1], [6, 7, -1]])
    sc = our_server.model_score(model, mk, dict(precision="fp32", cfg_scale=1.0), targets=tg)
    assert set(sc) == {"surprisal", "entropy", "relative", "logprob", "best_id"} and sc["best_id"].dtype == torch.int64
    call = model.score_calls[0]
    assert torch.equal(call["targets"], tg) and torch.equal(call["frames"], mk["inputs"]) and "input_ids" not in call
    assert torch.equal(sc["entropy"], ids.float() + 1)
    with pytest.raises(ValueError, match="cfg_scale"):
        our_server.model_forward(model, mk, dict(precision="fp32", cfg_scale=2.0))
    with pytest.raises(ValueError, match="cfg_scale"):
        our_server.model_score(model, mk, dict(cfg_scale=1.5))
    assert len(model.forward_calls) == 1 and len(model.score_calls) == 1


needs_ref = pytest.mark.skipif(not ref_shims.reference_available(), reason="reference checkout not present")


@needs_ref
def test_reference_processor_drives_our_model_forward(monkeypatch):
    """MaiMod's caller against our seam: the reference `Processor._batched_inference(proc.model_forward, ...)`
    (processor.py:469-476, :178-187, :697-746) with its module-level `model_forward` replaced by ours (the INTEGRATION.md swap)
    and a recording stand-in model.  Checks the `inputs -> frames` rename, the left-padded prompts and their masks, conditioning
    kwargs handed through, the CPU fp32 (B, T, V) result -- and that `cfg_scale > 1` raises in the reference's own
    `model_forward` (live call) and in ours."""
    from mapperatorinator_amd import server as our_server
    from oracle import ref_harness as rh
    ref_shims.install()
    from osuT5.osuT5.inference import processor as ref_proc
    from osuT5.osuT5.inference import server as ref_server
    from osuT5.osuT5.tokenizer import Tokenizer as RefTokenizer
    tok = RefTokenizer(rh._train_config("small", 251, 48, 388))

    def make_proc(model, cfg_scale):
        proc = object.__new__(ref_proc.Processor)
        proc.model, proc.tokenizer, proc.precision, proc.cfg_scale = model, tok, "fp32", cfg_scale
        proc.max_batch_size, proc.num_beams, proc.last_generation_stats = 2, 1, None
        return proc

    B = 3
    cond = [torch.tensor([[tok.sos_id]]), torch.tensor([[tok.sos_id, 40, 41]]), torch.tensor([[tok.sos_id, 9]])]
    frames = torch.randn(B, 32000)
    kwargses = [dict(difficulty=torch.tensor([float(k)])) for k in range(B)]

    monkeypatch.setattr(ref_proc, "model_forward", our_server.model_forward)      # the INTEGRATION.md edit
    model = _RecordingModel()
    proc = make_proc(model, 1.0)
    uncond = [torch.tensor([[tok.sos_id]])] * B                        # always built by the caller, used under guidance only
    out = list(proc._batched_inference(proc.model_forward, cond, uncond, frames, kwargses, verbose=False))
    assert len(out) == 2 and len(model.forward_calls) == 2          # max_batch_size 2: rows 0-1, then row 2
    width, rows = 3, 0
    for (result, stats), call in zip(out, model.forward_calls):
        n = call["decoder_input_ids"].shape[0]
        want = torch.cat([torch.nn.functional.pad(c, (width - c.shape[1], 0)) for c in cond[rows:rows + n]])
        assert "inputs" not in call and torch.equal(call["frames"], frames[rows:rows + n])
        assert torch.equal(call["decoder_input_ids"], want) and torch.equal(call["decoder_attention_mask"], want.ne(tok.pad_id))
        assert torch.equal(call["difficulty"], torch.arange(rows, rows + n, dtype=torch.float32))
        assert stats is None and result.dtype == torch.float32 and result.device.type == "cpu" and result.shape == (n, width, model.V)
        assert torch.equal(result[..., 0], want.float())
        rows += n
    assert rows == B

    # guidance: the reference's own function raises (its HF guidance processor is handed already-doubled ids) ...
    monkeypatch.setattr(ref_proc, "model_forward", ref_server.model_forward)
    ref_model = _RecordingModel()
    proc = make_proc(ref_model, 2.0)
    with pytest.raises(ValueError):
        list(proc._batched_inference(proc.model_forward, cond, uncond, frames, kwargses, verbose=False))
    assert len(ref_model.forward_calls) == 1                          # it got as far as the forward, then its processor refused
    # ... and so does ours
    monkeypatch.setattr(ref_proc, "model_forward", our_server.model_forward)
    proc = make_proc(_RecordingModel(), 2.0)
    with pytest.raises(ValueError, match="cfg_scale"):
        list(proc._batched_inference(proc.model_forward, cond, uncond, frames, kwargses, verbose=False))
