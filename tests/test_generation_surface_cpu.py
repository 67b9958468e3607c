"""not gpu: what the generation host path hands to `T5Engine.generate` / `generate_beam` / `decode` and to `beam.beam_search`, for every
combination of the decode mode switches, pinned against a recording.  The grid is the full product of cross_kv_fp8 {off, on} x
self_kv_fp8 {off, on} x (beam_cache, beam_prefill) {absent, copy, indexed, indexed + prefill, copy + prefill, "ring"} x
beam_sample_kernel {off, on} x num_beams {1, 2} x storage {bf16, fp32} x cfg_scale {1.0, 2.0}: 384 cases, through each entry point --
`model_generate`, `model_generate_rows` (one beam only: 192), `MapperatorinatorHIP.generate`, and `SequentialWindowScheduler.run` with
`merge_kwargs` off and on -- over the recording stand-ins of tests/test_self_kv_fp8_cpu.py (extended here to record, not copied).

A case's record is the exception's type and full message, or every call that reached one of the four callees: its name, its keyword
names, the value of every bool / str / None / number keyword, shape and dtype of every tensor keyword, and the values of the prompt, the
mask and the EOS ids (of a table: where it is set).  The scheduler's records also count the encoder calls made before the case ended.
tests/golden/generation_surface.json holds the records (equal ones stored once) and, per entry point, case -> record; its "note" names the
commit whose host path made them.

One deviation from the recording is accepted: `SequentialWindowScheduler.run` refuses a bad `beam_cache` / `beam_prefill` under beams,
and `cross_kv_fp8` on fp32 storage, before it encodes, where the recorded commit refused them at the first decode.  Those cases are
`_refused_late` below (asserted to be exactly the recording's refusals with an encoder call in front); of them type and message are
compared, of every other case the whole record.

To record again (only ever from the commit a change is to be compared WITH, never from the tree under test): copy this file into that
commit's tests/ and run `python tests/test_generation_surface_cpu.py > tests/golden/generation_surface.json` there."""
import ctypes as C
import itertools
import json
import os
import subprocess
import sys
import types

import pytest
import torch

from conftest import GOLDEN, ROOT
from mapperatorinator_amd import Tokenizer

ENTRIES = ("model_generate", "model_generate_rows", "modeling_generate", "scheduler", "scheduler_merged")
CACHES = ((None, None), ("copy", False), ("indexed", False), ("indexed", True), ("copy", True), ("ring", False))
GRID = [dict(cross=c, self_=s, cache=cache, prefill=prefill, draw=d, beams=nb, dtype=dt, cfg=cfg)
        for c, s, (cache, prefill), d, nb, dt, cfg in itertools.product((False, True), (False, True), CACHES, (False, True), (1, 2),
                                                                         ("bfloat16", "float32"), (1.0, 2.0))]
TGT = 24


def case_key(c) -> str:
    cache = "absent" if c["cache"] is None else f"{c['cache']}{'+prefill' if c['prefill'] else ''}"
    return f"cross={int(c['cross'])} self={int(c['self_'])} cache={cache} draw={int(c['draw'])} beams={c['beams']} {c['dtype']} cfg={c['cfg']}"


def cases_of(entry):
    return [c for c in GRID if c["beams"] == 1] if entry == "model_generate_rows" else GRID


def _switches(c) -> dict:
    d = dict(cross_kv_fp8=c["cross"], self_kv_fp8=c["self_"], beam_sample_kernel=c["draw"])
    return d if c["cache"] is None else dict(d, beam_cache=c["cache"], beam_prefill=c["prefill"])


def _describe(v):
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    if isinstance(v, torch.Tensor):
        return dict(shape=list(v.shape), dtype=str(v.dtype))
    if isinstance(v, (tuple, list)):
        return [_describe(x) for x in v]
    if isinstance(v, C.Array):
        return f"{type(v)._type_.__name__}[{len(v)}]"
    return type(v).__name__


def _values(t):
    return None if t is None else dict(_describe(t), values=t.tolist())


def _call(callee, prompt, mask, eos, sp, kw) -> dict:
    if isinstance(eos, torch.Tensor):                      # decode's table: its width and where it is set
        eos = dict(_describe(eos), set=eos.nonzero().reshape(-1).tolist())
    elif eos is not None:
        eos = [int(e) for e in eos]
    return dict(callee=callee, prompt=_values(prompt), mask=_values(mask), eos=eos,
                sampling=dict(cfg_scale=float(sp.cfg_scale), max_length=int(sp.max_length), num_beams=getattr(sp, "num_beams", None)),
                kw={k: _describe(v) for k, v in sorted(kw.items())})


def _engines():
    """The stand-ins of tests/test_self_kv_fp8_cpu.py, recording every call in full."""
    from test_self_kv_fp8_cpu import _RecordingEngine, _SchedulerEngine
    from mapperatorinator_amd.t5_engine import require_bf16_for_cross_kv_fp8

    class Engine(_RecordingEngine):
        def generate(self, audio, prompt, mask, eos, sp, **kw):
            self.trace.append(_call("generate", prompt, mask, eos, sp, kw))
            return super().generate(audio, prompt, mask, eos, sp, **kw)

        def generate_beam(self, audio, prompt, mask, eos, sp, num_beams, **kw):
            self.trace.append(_call("generate_beam", prompt, mask, eos, sp, dict(kw, num_beams=num_beams)))
            return super().generate_beam(audio, prompt, mask, eos, sp, num_beams, **kw)

    class WaveEngine(_SchedulerEngine):
        def cross_kv_fp8(self, kv):
            require_bf16_for_cross_kv_fp8(self.dtype)     # (as T5Engine.cross_kv_fp8 begins)
            return torch.zeros(4, dtype=torch.uint8)

        def decode(self, kv, prompt, prompt_mask, eos_table, sampling, **kw):
            self.trace.append(_call("decode", prompt, prompt_mask, eos_table, sampling, kw))
            kw.pop("row_sampling", None)
            return super().decode(kv, prompt, prompt_mask, eos_table, sampling, **kw)
    return Engine, WaveEngine


class ClassifierFreeGuidanceLogitsProcessor:              # (recognised by its class name: server.sampling_from_processors)
    def __init__(self, scale):
        self.guidance_scale = scale


def run_case(entry, c, tok, mp) -> dict:
    from mapperatorinator_amd import beam as beam_mod
    from mapperatorinator_amd.modeling import MapperatorinatorHIP
    from mapperatorinator_amd.scheduler import SequentialWindowScheduler, SongJob
    from mapperatorinator_amd.server import model_generate, model_generate_rows
    Engine, WaveEngine = _engines()
    dtype, guided, nb = getattr(torch, c["dtype"]), c["cfg"] > 1.0, c["beams"]
    prompt = torch.tensor([[tok.sos_id, 7, 9], [0, tok.sos_id, 7]])
    neg = torch.tensor([[tok.sos_id, 5], [0, tok.sos_id]])
    mk = dict(inputs=torch.zeros(2, 16), decoder_input_ids=prompt, decoder_attention_mask=prompt.ne(0))
    if guided:
        mk["negative_prompt"] = neg
    gk = dict(do_sample=False, num_beams=nb, max_length=TGT, cfg_scale=c["cfg"], **_switches(c))
    trace, out = [], {}
    try:
        if entry in ("model_generate", "model_generate_rows"):
            eng = Engine(dtype)
            eng.trace = trace
            model = types.SimpleNamespace(engine=eng, dtype=dtype, config=types.SimpleNamespace(max_target_positions=TGT))
            if entry == "model_generate":
                model_generate(model, tok, mk, gk)
            else:
                model_generate_rows(model, tok, mk, [gk, dict(gk, lookahead_time=30)])
        elif entry == "modeling_generate":
            eng = Engine(dtype)
            eng.trace = trace
            cfgm = types.SimpleNamespace(max_target_positions=TGT, pad_token_id=0, vocab_size=tok.vocab_size_out, eos_token_id=tok.eos_id)
            me = types.SimpleNamespace(engine=eng, dtype=dtype, config=cfgm, device=torch.device("cpu"), _row_bias=lambda n, kw: None)
            procs = [ClassifierFreeGuidanceLogitsProcessor(c["cfg"])] if guided else []
            call = {k: v for k, v in mk.items() if k != "inputs"}
            MapperatorinatorHIP.generate(me, inputs=mk["inputs"], logits_processor=procs, num_beams=nb, max_length=TGT, **call, **_switches(c))
        else:
            eng = WaveEngine(tok.vocab_size_out, tok.eos_id, dtype)
            eng.trace = trace
            model = types.SimpleNamespace(engine=eng, config=types.SimpleNamespace(max_target_positions=TGT))

            def search(engine, kv, prompt, mask, eos, sp, num_beams, **kw):
                # the refusals the real search begins with (beam.py: beam_search, _step_kv_fp8), then the record
                beam_mod.check_cache_mode(kw.get("cache", "copy"), kw.get("prefill", False))
                if kw.get("self_kv_fp8"):
                    beam_mod.require_bf16_for_self_kv_fp8(engine.dtype, max(2, int(num_beams)), kw.get("cache", "copy"))
                if kw.get("kv_fp8") is not None and kw.get("kv_fp8") is not False:
                    beam_mod.require_bf16_for_cross_kv_fp8(engine.dtype)
                trace.append(_call("beam_search", prompt, mask, eos, sp, dict(kw, num_beams=num_beams)))
                G = kv.shape[2]
                return torch.cat([prompt[-G:].long(), torch.full((G, 1), int(sorted(eos)[0]))], 1)
            mp.setattr(beam_mod, "beam_search", search)

            def job(k):          # songs 0 and 1 share their kwargs (ragged prompts: one call, left-padded and masked), song 2 has its own EOS window
                own = prompt[k % 2][prompt[k % 2] != 0][None]
                ask = dict(decoder_input_ids=own, generate_kwargs=dict(lookahead_time=30 if k == 2 else 0))
                if guided:
                    ask["negative_prompt"] = neg[k % 2][neg[k % 2] != 0][None]
                return SongJob(frames=torch.full((1, 16), 1.0 + k), prompt_fn=lambda w: dict(ask), on_result=lambda w, row, st: None,
                               generate_kwargs=gk)
            try:
                SequentialWindowScheduler(model, tok, decode_batch=8, merge_kwargs=entry == "scheduler_merged").run([job(k) for k in range(3)])
            finally:
                out["encoded"] = eng.encoded
    except Exception as e:                                 # noqa: BLE001  (whatever the entry point raised is the record)
        out["raises"] = [type(e).__name__, str(e)]
    return dict(out, calls=trace)


def _refused_late(entry, c) -> bool:
    """Scheduler cases the recorded commit refused at the first decode call (one encoder call made), which `run` now refuses up front:
    a bad cache mode under beams, or cross_kv_fp8 on fp32 storage -- unless the self_kv_fp8 refusal, made up front then as now, came first."""
    if not entry.startswith("scheduler"):
        return False
    up_front = c["self_"] and (c["dtype"] == "float32" or (c["beams"] > 1 and c["cache"] != "indexed"))
    bad_cache = c["beams"] > 1 and (c["cache"] == "ring" or (bool(c["prefill"]) and c["cache"] != "indexed"))
    return not up_front and (bad_cache or (c["cross"] and c["dtype"] == "float32"))


@pytest.fixture(scope="module")
def recording():
    return json.load(open(os.path.join(GOLDEN, "generation_surface.json")))


@pytest.mark.parametrize("entry", ENTRIES)
def test_every_mode_combination_reaches_the_callees_as_recorded(monkeypatch, recording, entry):
    tok = Tokenizer.benchmark_vocab(src_seq_len=251)
    cases, records = recording["entries"][entry], recording["records"]
    grid = cases_of(entry)
    assert sorted(cases) == sorted(case_key(c) for c in grid) and len(grid) == (192 if entry == "model_generate_rows" else 384)
    late = {k for k, i in cases.items() if "raises" in records[i] and records[i].get("encoded", 0) > 0}
    assert late == {case_key(c) for c in grid if _refused_late(entry, c)}
    wrong, n_calls = [], 0
    for c in grid:
        key = case_key(c)
        want, got = records[cases[key]], json.loads(json.dumps(run_case(entry, c, tok, monkeypatch)))
        n_calls += len(want["calls"])
        if key in late:
            want, got = want["raises"], got.get("raises")
        if got != want:
            wrong.append(f"{key}:\n  got  {got}\n  want {want}")
    assert n_calls > 100                                   # (the recording holds calls, not only refusals)
    assert not wrong, f"{len(wrong)} of {len(grid)} cases differ from the recording; the first:\n" + "\n".join(wrong[:3])


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    commit = subprocess.run(["git", "-C", ROOT, "log", "-1", "--format=%h %s"], capture_output=True, text=True).stdout.strip()
    dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain", "--", "mapperatorinator_amd"], capture_output=True, text=True).stdout
    assert not dirty.strip(), "record from a clean checkout of the commit to compare with:\n" + dirty
    tok = Tokenizer.benchmark_vocab(src_seq_len=251)
    records, index, entries = [], {}, {}
    for entry in ENTRIES:
        entries[entry] = {}
        for c in cases_of(entry):
            with pytest.MonkeyPatch.context() as mp:
                rec = json.dumps(run_case(entry, c, tok, mp), sort_keys=True)
            if rec not in index:
                index[rec] = len(records)
                records.append(json.loads(rec))
            entries[entry][case_key(c)] = index[rec]
    note = (f"What the four generation entry points handed to generate / generate_beam / decode / beam_search at commit {commit}: "
            "recorded by tests/test_generation_surface_cpu.py run as a script in a clean checkout of that commit.")
    print(json.dumps(dict(note=note, records=records, entries=entries), indent=None, separators=(",", ":")))
