"""not gpu: what `beam_search` asks of the library, call by call, pinned against a recording.  The torch-op form runs on CPU tensors
over the recording stand-in library of tests/test_beam_self_kv_fp8_cpu.py (2 chunks x 2 beams, V = 16, tgt_len = 12, P = 3; four
prompt rows under guidance) on both cache routes, with the prompt prefill, with the e4m3 self cache, each with and without
guidance.  tests/golden/beam_call_traces.json holds the eight recordings; its "note" names the commit whose beam.py made them.

A recording is the ordered list of [entry, arguments]: integers as they are, NULL as null, a struct handed by reference as "&Type",
and every buffer as "p<n>", n = the ordinal of its first appearance among the run's arguments -- which pins the buffers' identities
(the logits buffer, the workspace, the ping-pong of the two index tables) without pinning addresses.  Every tensor whose pointer is
taken during a run is kept alive until the run ends, so no address comes back for another buffer.  Behind the arguments stand the
int32 values the call was handed through its `tokens` / `src` / prompt argument: the tokens every row was fed and the rows every
reorder gathered.

To record again (only ever from the commit a change is to be compared WITH, never from the tree under test): copy this file into that
commit's tests/ and run `python tests/test_beam_call_trace_cpu.py > tests/golden/beam_call_traces.json` there."""
import json
import os
import subprocess
import sys

import pytest
import torch

from conftest import GOLDEN, ROOT
from mapperatorinator_amd import _lib

MODES = {"copy": dict(cache="copy"), "indexed": dict(cache="indexed"), "indexed+prefill": dict(cache="indexed", prefill=True),
         "indexed+prefill+self_kv_fp8": dict(cache="indexed", prefill=True, self_kv_fp8=True)}
SCALES = (1.0, 2.0)
# entry -> which of its arguments carries int32 values the search computed (tokens / src / the prompts of the prefill)
VALUES = {"mh_t5_step": 5, "mh_t5_step_fp8": 6, "mh_t5_step_indexed": 6, "mh_t5_step_indexed_skv8": 6, "mh_t5_reorder_cache": 2,
          "mh_t5_reorder_index": 2, "mh_t5_step_prefill": 4}


def record(monkeypatch, mode, cfg_scale):
    from test_beam_self_kv_fp8_cpu import _stand_in_search
    from mapperatorinator_amd import beam as beam_mod
    guided = cfg_scale > 1.0
    lib, eng, asked, _ = _stand_in_search(monkeypatch, rows=8 if guided else 4)
    held = {}                                              # address -> the tensors that gave it, alive until the run ends
    values = []                                            # per call: the int32 values behind its VALUES argument, read AT the call

    class Snapshots(type(lib)):
        def __getattr__(self, name):
            f = super().__getattr__(name)

            def g(*a):
                values.append(held[a[VALUES[name]]][-1].flatten().tolist() if name in VALUES else None)
                return f(*a)
            return g
    lib.__class__ = Snapshots
    real_ptr = torch.Tensor.data_ptr

    def data_ptr(self):
        at = real_ptr(self)
        held.setdefault(at, []).append(self)
        return at
    monkeypatch.setattr(torch.Tensor, "data_ptr", data_ptr)
    sp = _lib.MhSampling()
    sp.max_length, sp.cfg_scale, sp.temperature, sp.pad_id = 12, cfg_scale, 1.0, 0
    rows = [[1, 3, 4], [1, 6, 7]]
    prompt = torch.tensor(([[1, 9, 9], [1, 9, 8]] if guided else []) + rows)          # [negative rows | prompt rows]
    out = beam_mod.beam_search(eng, torch.zeros(2, 2, 2, 2, 4, 64), prompt, None, [2], sp, 2, use_kernel=False, **MODES[mode])
    assert out.shape[0] == 2 and out.shape[1] > 3
    ordinal, trace = {}, []
    for name, args, vals in zip(lib.calls, lib.args, values):
        line = []
        for a in args:
            if a is None or (isinstance(a, int) and a not in held):
                line.append(a)
            elif isinstance(a, int):
                line.append("p%d" % ordinal.setdefault(a, len(ordinal)))
            else:
                line.append("&" + type(a._obj).__name__)  # ctypes.byref(struct)
        trace.append([name, line] if vals is None else [name, line, vals])
    return dict(calls=trace, workspaces=[list(x) for x in asked], ids=out.tolist())


@pytest.mark.parametrize("cfg_scale", SCALES)
@pytest.mark.parametrize("mode", list(MODES))
def test_the_search_asks_the_library_for_what_the_recording_holds(monkeypatch, mode, cfg_scale):
    want = json.load(open(os.path.join(GOLDEN, "beam_call_traces.json")))["traces"][f"{mode} cfg_scale={cfg_scale}"]
    got = record(monkeypatch, mode, cfg_scale)
    assert len(want["calls"]) > 10
    for i, (g, w) in enumerate(zip(got["calls"], want["calls"])):
        assert g == w, f"call {i}: {g} where the recording has {w}"
    assert len(got["calls"]) == len(want["calls"])
    assert got["workspaces"] == want["workspaces"] and got["ids"] == want["ids"]


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    commit = subprocess.run(["git", "-C", ROOT, "log", "-1", "--format=%h %s"], capture_output=True, text=True).stdout.strip()
    dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain", "--", "mapperatorinator_amd"], capture_output=True, text=True).stdout
    assert not dirty.strip(), "record from a clean checkout of the commit to compare with:\n" + dirty
    traces = {}
    for mode in MODES:
        for scale in SCALES:
            with pytest.MonkeyPatch.context() as mp:
                traces[f"{mode} cfg_scale={scale}"] = record(mp, mode, scale)
    note = (f"What beam_search(use_kernel=False) asked of the recording stand-in library at commit {commit}: "
            "recorded by tests/test_beam_call_trace_cpu.py run as a script in a clean checkout of that commit.")
    print(json.dumps(dict(note=note, traces=traces), indent=None, separators=(",", ":")))
