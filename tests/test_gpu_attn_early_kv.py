"""-m gpu: the decode attention's first key iteration on K / V rows requested ahead of the query (csrc/decode_device.hpp: `FirstKeys`,
`attend_keys<..., EARLY>`, `dec_cross_attn_q_kernel`) gives the bits of the build that requested them inside the key loop.

Short teacher-forced decodes of tiny models dump the scores of every column; they equal, bit for bit, what the PARENT build dumped:
tests/golden/attn_early_kv_tiny.npz holds a SHA-256 prefix of every (column, row)'s scores and the raw bits of a few ids.  The
recording was made on an MI355X from a library built from the commit before this change (`make` in a clean checkout of it), never
from the tree under test: `MAPPERHIP_LIB=<that library> python -m mh_testing.attn_early_kv tests/golden/attn_early_kv_tiny.npz`
(mh_testing/attn_early_kv.py is the run and the recorder; its docstring gives the shapes and why those).

Cross-attention: encoder lengths 1, 7, 8, 9, 127, 128, 129, 257 in fp32 and bf16 (bf16 T5 forms issue early, fp32 ones keep the old
order), one `cross_kv_fp8` case and one Whisper-family case (which keeps the old order: unchanged either way).  Self-attention (its
kernel keeps the old order, but runs the restructured `attend_keys`): positions 0 .. 130 with 3 and 18 rows, a left-padded prompt mask of
width 9, the e4m3 shadow cache and the indexed step under a reordered table."""
import numpy as np
import pytest

from conftest import GOLDEN
from mh_testing.attn_early_kv import CASES, run_case, summarise

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", CASES)
def test_decode_scores_equal_the_recording_of_the_parent_build(case):
    g = np.load(f"{GOLDEN}/attn_early_kv_tiny.npz")
    want_digest, want_sample = g[f"{case}_digest"], g[f"{case}_sample"]
    n_prompt = 9 if "mask9" in case else 1
    first = 0 if "indexed" in case else n_prompt          # (the indexed step is driven from position 0: every column holds scores)
    assert np.any(want_sample[first:] != 0), "the recording holds no scores"
    got = summarise(run_case(case))
    assert got["digest"].shape == want_digest.shape and got["sample"].shape == want_sample.shape
    bad = np.argwhere((got["digest"] != want_digest).any(-1))
    print(f"{case}: the scores of {len(bad)} of {want_digest.shape[0] * want_digest.shape[1]} (column, row) pairs differ from the recording")
    if len(bad):
        c, r = bad[0]
        print("first differing (column, row):", (int(c), int(r)), "sampled ids, bits now / recorded:",
              [f"{a:#010x}/{b:#010x}" for a, b in zip(got["sample"][c, r], want_sample[c, r])])
    assert len(bad) == 0, f"(column, row) pairs whose scores differ in some bit: {bad[:6].tolist()}"
    assert np.array_equal(got["sample"], want_sample)
