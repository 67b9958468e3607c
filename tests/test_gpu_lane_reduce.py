"""-m gpu: the cross-lane reductions of the kernels on the VALU (csrc/common.hpp: DPP row exchanges, gfx950 row / half swaps) give
the bits of the `__shfl_xor` forms they replaced.

1. `mh_debug_lane_reduce` applies every new helper and its shuffle reference to the same input in one kernel: sums and maxima over
   the wave, over groups of 8 / 16 / 64 lanes and over the attention merge's partners 8 / 16 / 32, plus the bare exchanges.  256
   waves of 64 lanes; the inputs are raw bit patterns (random finite values, denormals, +-0, +-inf); equal as uint32 in every lane.
2. A short teacher-forced decode of the tiny T5 (3 rows = one chain, 12 new tokens, fp32 and bf16 storage) dumps the scores of every
   column; they equal, bit for bit, what the build before the change dumped: tests/golden/lane_reduce_tiny.npz holds a SHA-256
   prefix of every (column, row)'s scores and the raw bits of a few ids (mh_testing/lane_reduce.py is the run and the recorder)."""
import numpy as np
import pytest
import torch

from conftest import GOLDEN
from mapperatorinator_amd import _lib

pytestmark = pytest.mark.gpu

N_WAVES = 256
CASES = ["wave_sum", "wave_max", "group_sum<8>", "group_sum<16>", "group_sum<64>", "group_max<8>", "group_max<16>", "group_max<64>",
         "merge sum 8/16/32", "merge max 8/16/32", "xor 1", "xor 2", "xor 4", "xor 8", "xor 16", "xor 32"]


def _inputs():
    """uint32 (N_WAVES * 64): by wave -- random finite patterns of every exponent; moderate values (sums stay finite); denormals; a
    mix with +-0 and +-inf sprinkled in (inf - inf gives the default NaN on both sides; no NaN goes in)."""
    rng = np.random.default_rng(20)
    n = N_WAVES * 64
    u = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    u = np.where((u & 0x7f800000) == 0x7f800000, u & np.uint32(0xbfffffff), u)          # exponent 255 -> finite
    wave = np.arange(n) // 64
    mod = rng.standard_normal(n).astype(np.float32).view(np.uint32)
    den = (u & np.uint32(0x807fffff))                                                     # exponent 0: denormals and +-0
    kind = wave % 4
    x = np.where(kind == 1, mod, u)
    x = np.where(kind == 2, den, x)
    special = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x00000001, 0x80000001], dtype=np.uint32)
    pick = rng.integers(0, len(special), n)
    x = np.where((kind == 3) & (rng.random(n) < 0.25), special[pick], np.where(kind == 3, mod, x))
    # a few waves of one special value only, and single specials among moderate values
    x[63 * 64:64 * 64] = 0x80000000
    x[127 * 64:128 * 64] = 0x7f800000
    x[191 * 64 + 17] = 0xff800000
    return x.astype(np.uint32)


def test_helpers_equal_shuffle_forms_bit_for_bit():
    lib = _lib.load()
    x = _inputs()
    n = x.size
    xin = torch.from_numpy(x.view(np.int32)).cuda()
    new = torch.full((len(CASES), n), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    ref = torch.full((len(CASES), n), 0x3c3c3c3c, dtype=torch.int32, device="cuda")
    _lib.check(lib.mh_debug_lane_reduce(xin.data_ptr(), N_WAVES, new.data_ptr(), ref.data_ptr(), None), "mh_debug_lane_reduce")
    torch.cuda.synchronize()
    new, ref = new.cpu().numpy().view(np.uint32), ref.cpu().numpy().view(np.uint32)
    # the reference side is what the test thinks it is: the bare exchanges against numpy, the wave maximum of the moderate waves too
    lanes = np.arange(n)
    for c, o in enumerate((1, 2, 4, 8, 16, 32)):
        assert np.array_equal(ref[10 + c], x[lanes ^ o]), f"reference exchange xor {o}"
    mod_waves = np.nonzero(np.arange(N_WAVES) % 4 == 1)[0]
    want_max = x.view(np.float32).reshape(N_WAVES, 64)[mod_waves].max(axis=1)
    assert np.array_equal(ref[1].view(np.float32).reshape(N_WAVES, 64)[mod_waves], np.repeat(want_max[:, None], 64, 1))
    for c, name in enumerate(CASES):
        bad = np.nonzero(new[c] != ref[c])[0]
        print(f"{name}: {bad.size} of {n} lanes differ")
        assert bad.size == 0, (f"{name}: lane {bad[0] % 64} of wave {bad[0] // 64}: {new[c][bad[0]]:#010x} vs the shuffle form's "
                               f"{ref[c][bad[0]]:#010x} ({bad.size} lanes differ)")


@pytest.mark.parametrize("dtype_name", ["f32", "bf16"])
def test_decode_scores_equal_the_recording_of_the_shuffle_build(dtype_name):
    from mh_testing.lane_reduce import NEW_TOKENS, PROMPT_LEN, ROWS, decode_logits, summarise
    g = np.load(f"{GOLDEN}/lane_reduce_tiny.npz")
    want_digest, want_sample = g[f"{dtype_name}_digest"], g[f"{dtype_name}_sample"]
    assert want_digest.shape == (PROMPT_LEN + NEW_TOKENS, ROWS, 16)
    assert np.any(want_sample[PROMPT_LEN:] != 0), "the recording holds no scores"
    got = summarise(decode_logits(dtype_name))
    assert got["digest"].shape == want_digest.shape and got["sample"].shape == want_sample.shape
    bad = np.argwhere((got["digest"] != want_digest).any(-1))
    print(f"{dtype_name}: the scores of {len(bad)} of {want_digest.shape[0] * ROWS} (column, row) pairs differ from the recording")
    if len(bad):
        c, r = bad[0]
        print("first differing (column, row):", (int(c), int(r)), "sampled ids, bits now / recorded:",
              [f"{a:#010x}/{b:#010x}" for a, b in zip(got["sample"][c, r], want_sample[c, r])])
    assert len(bad) == 0, f"(column, row) pairs whose scores differ in some bit: {bad[:6].tolist()}"
    assert np.array_equal(got["sample"], want_sample)
