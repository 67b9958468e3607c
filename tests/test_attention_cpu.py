"""not gpu: the host side of the attention kernel tests (mh_testing/attention.py) -- the three test-facing entries are declared,
bound and refuse bad arguments; the mask predicate equals a literal double loop; the fp64 reference equals torch's own attention and
the oracle's decoder bias; and, for EVERY case tests/test_gpu_attention.py runs, the tolerance 4 * floor is finite and every mutant of
the case (the same problem with one fault) is at least 10 tolerances away from the reference in at least 4 output rows, so that a
kernel with that fault cannot pass."""
import ctypes as C
import itertools
import os

import pytest
import torch

from conftest import ROOT
from mapperatorinator_amd import _lib
from mh_testing import attention as A


# ---- binding -------------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mapperhip.h")).read()
    lib = _lib.load()
    for name in ("mh_attention_strided", "mh_attention_packed", "mh_attention_last_kernel"):
        assert name + "(" in hdr and name in _lib.SYMBOLS and hasattr(lib, name)
    assert "typedef struct MhAttnProblem" in hdr and "band < 0" in hdr and "band <= 0: no mask" not in hdr
    assert lib.mh_abi_version() == 11 and lib.mh_struct_size(9) == -1          # additive: no new entry of the size table
    assert C.sizeof(_lib.MhAttnProblem) == 8 + 16 * 8 + 18 * 4
    assert (_lib.ATTN_FLASH_F32, _lib.ATTN_FLASH_BF16, _lib.ATTN_SMALL_K2, _lib.ATTN_SMALL_K4, _lib.ATTN_FLASH2) == \
        (A.K_FLASH_F32, A.K_FLASH_BF16, A.K_SMALL_K2, A.K_SMALL_K4, A.K_FLASH2)
    for tok in ("MH_ATTN_FLASH_F32 = 1", "MH_ATTN_FLASH_BF16 = 2", "MH_ATTN_SMALL_K2 = 3", "MH_ATTN_SMALL_K4 = 4", "MH_ATTN_FLASH2 = 8",
                "MH_ATTN_FLASH2_BIAS = 1", "MH_ATTN_FLASH2_SIMPLE = 2"):
        assert tok in hdr
    assert len(A.ALL_KERNELS) == 8
    assert lib.mh_attention_last_kernel() in {0} | A.ALL_KERNELS               # host-only: callable without a device


def test_entries_refuse_bad_arguments_without_gpu():
    lib = _lib.load()
    assert lib.mh_attention_strided(None, None) == -1 and b"null problem" in lib.mh_last_error()
    p = _lib.MhAttnProblem()
    for wrong in (0, C.sizeof(p) - 8, C.sizeof(p) + 8):
        p.struct_bytes = wrong
        assert lib.mh_attention_strided(C.byref(p), None) == -1 and b"struct_bytes" in lib.mh_last_error()
    p.struct_bytes = C.sizeof(p)
    p.B, p.H, p.Lq, p.Lk, p.Lkpad, p.scale = 1, 1, 8, 8, 64, 1.0
    assert lib.mh_attention_strided(C.byref(p), None) == -1 and b"null operand" in lib.mh_last_error()
    p.dtype = 2
    assert lib.mh_attention_strided(C.byref(p), None) == -1 and b"dtype" in lib.mh_last_error()
    p.dtype, p.q_pos0, p.band = 0, 3, 4      # a band at q_pos0 != 0: the kernels would pick the wrong key tiles
    assert lib.mh_attention_strided(C.byref(p), None) == -1 and b"q_pos0" in lib.mh_last_error()
    p.band, p.q_pos0 = 0, -1
    assert lib.mh_attention_strided(C.byref(p), None) == -1 and b"q_pos0" in lib.mh_last_error()
    p.q_pos0, p.dtype, p.out_split3 = 0, 1, 1
    assert lib.mh_attention_strided(C.byref(p), None) == -1 and b"out_split3" in lib.mh_last_error()
    args = (None, 256, 128, None, 64, None, None, 128, 1, 8, 2, 1.0, 0, 0)
    assert lib.mh_attention_packed(*args, 0, 0, None) == -1 and b"null operand" in lib.mh_last_error()
    assert lib.mh_attention_packed(*args[:-1], 1, 0, 1, None) == -1 and b"out_split3" in lib.mh_last_error()
    assert lib.mh_attention_packed(*args[:-1], 5, 0, 0, None) == -1 and b"dtype" in lib.mh_last_error()
    assert lib.mh_attention(*args, None) == -1 and b"null operand" in lib.mh_last_error()


# ---- the reference itself ---------------------------------------------------------------------------------------------------------
def _visible_loop(B, Lq, Lk, band, open_from, causal, q_pos0, key_mask, mask_len):
    out = torch.zeros(B, Lq, Lk, dtype=torch.bool)
    for b in range(B):
        for q in range(Lq):
            for key in range(Lk):
                qpos = q_pos0 + q
                ok = key >= mask_len or key_mask is None or bool(key_mask[b][key])
                if band != 0:
                    rel = key - qpos
                    in_band = (-(band - 1) <= rel <= band) if band > 0 else (abs(rel) <= -band)
                    ok = ok and (in_band or (open_from > 0 and (key >= open_from or qpos >= open_from)))
                if causal:
                    ok = ok and key <= qpos
                out[b, q, key] = ok
    return out


FORMS = [dict(Lq=Lq, Lk=Lk, band=band, open_from=of, causal=causal, q_pos0=q_pos0, masked=masked)
         for (Lq, Lk, q_pos0) in ((23, 23, 0), (9, 40, 31), (40, 17, 0))
         for band, of in ((0, 0), (5, 0), (-5, 0), (5, 14), (-5, 14), (1, 0), (-1, 30))
         for causal in (False, True) for masked in (False, True)]


def test_visible_equals_the_literal_double_loop():
    g = torch.Generator().manual_seed(1)
    for f in FORMS:
        B, Lk = 3, f["Lk"]
        km, ml = None, 0
        if f["masked"]:
            km = (torch.rand(B, Lk + 3, generator=g) < 0.6).to(torch.uint8)
            km[0, :7] = 0
            ml = Lk - 4                      # keys >= mask_len always attend, whatever the mask holds there
            km[:, ml:] = 0
        want = _visible_loop(B, f["Lq"], Lk, f["band"], f["open_from"], f["causal"], f["q_pos0"], km, ml)
        got = A.visible(B, f["Lq"], Lk, f["band"], f["open_from"], f["causal"], f["q_pos0"], km, ml)
        assert torch.equal(got, want), f


@pytest.mark.parametrize("bias", [None, "enc", "dec"])
def test_reference_equals_torch_sdpa_in_fp64(bias):
    g = torch.Generator().manual_seed(2)
    for f in FORMS[::3]:
        B, H, Lq, Lk = 2, 3, f["Lq"], f["Lk"]
        if bias == "enc" and Lq != Lk:
            continue
        q, k, v = (torch.randn(B, H, n, 64, generator=g, dtype=torch.float64) for n in (Lq, Lk, Lk))
        km = (torch.rand(B, Lk, generator=g) < 0.7).to(torch.uint8) if f["masked"] else None
        vis = A.visible(B, Lq, Lk, f["band"], f["open_from"], f["causal"], f["q_pos0"], km, Lk if f["masked"] else 0)
        form = None if bias is None else (A.enc_bias_form(Lk) if bias == "enc" else A.dec_bias_form(Lk + 40))
        table = None if bias is None else torch.randn(H, form.hs, generator=g, dtype=torch.float64)
        got = A.reference(q, k, v, 0.3, vis, table, form, f["q_pos0"])
        add = torch.zeros(B, H, Lq, Lk, dtype=torch.float64)
        if bias is not None:     # an independent restatement of bias[h][center + clamp(sign * (key - qpos), min, max)]
            for qi, key in itertools.product(range(Lq), range(Lk)):
                add[:, :, qi, key] = table[:, form.center + min(max(form.sign * (key - f["q_pos0"] - qi), form.lo), form.hi)]
        alive = vis.any(-1)
        add = add.masked_fill(~vis[:, None], float("-inf")).masked_fill(~alive[:, None, :, None], 0.0)
        want = torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=add, scale=0.3)
        sel = alive[:, None, :, None].expand_as(got)
        assert alive.any() and (got[sel] - want[sel]).abs().max().item() < 1e-12, f
        assert (got[~sel] == 0).all()
        for dt, bound in (("f32", 1e-4), ("bf16", 5e-2)):      # the emulation is the same function (loose: only that it is not another one)
            assert (A.emulated(q, k, v, 0.3, vis, table, form, f["q_pos0"], dt) - got).abs().max().item() < bound


def test_decoder_bias_form_equals_the_oracle():
    from mapperatorinator_amd.t5_engine import T5_PRESETS, rel_bias_tables
    from oracle.t5 import T5Oracle
    dims, H, tgt = T5_PRESETS["tiny"], T5_PRESETS["tiny"].n_heads, 48
    g = torch.Generator().manual_seed(3)
    tab = torch.randn(dims.n_buckets, H, generator=g)
    name = "transformer.%s.block.0.layer.0.SelfAttention.relative_attention_bias.weight"
    o = T5Oracle({name % "encoder": tab, name % "decoder": tab}, dims.d_model, dims.d_ff, H, 1, 1, n_buckets=dims.n_buckets,
                 max_distance=dims.max_distance)
    enc, dec = rel_bias_tables(tab, tab, 33, tgt, dims)
    for q_pos0, Lq, Lk in ((0, 40, 40), (29, 11, 40), (0, 48, 48)):
        want = o.dec_bias(torch.arange(q_pos0, q_pos0 + Lq), Lk)[0]
        got = A.bias_term(dec, A.dec_bias_form(tgt), Lq, Lk, q_pos0)
        assert torch.equal(got, want)       # every pair: the clamp at 0 is the oracle's bucket of a key in the future
    assert torch.equal(A.bias_term(enc, A.enc_bias_form(33), 33, 33), o.enc_bias(33)[0])


def test_layouts_round_trip():
    g = torch.Generator().manual_seed(4)
    x, y = torch.randn(2, 3, 5, 64, generator=g), torch.randn(2, 3, 5, 64, generator=g)
    assert torch.equal(A.heads_of(A.rows_of(x), 2, 3), x)
    qk = A.pack_qk(x, y)
    assert qk.shape == (10, 384) and torch.equal(A.heads_of(qk[:, :192], 2, 3), x) and torch.equal(A.heads_of(qk[:, 192:], 2, 3), y)
    kc = A.cache_layout(x, 9)
    assert kc.shape == (2, 3, 9, 64) and torch.equal(kc[:, :, :5], x) and (kc[:, :, 5:] == 7.0).all()
    vt = A.vt_layout(x, 64)
    assert vt.shape == (2, 3, 64, 64) and torch.equal(vt[..., :5].transpose(-1, -2), x) and (vt[..., 5:] == 0).all()
    w = torch.randn(4, 64, generator=g)
    hi = w.to(torch.bfloat16)
    lo = (w - hi.float()).to(torch.bfloat16)
    packed = torch.stack([hi.reshape(4, 2, 32), lo.reshape(4, 2, 32)], 2).reshape(4, 128).view(torch.float32)
    assert torch.equal(A.split3_unpack(packed), hi.float() + lo.float())
    assert (A.split3_unpack(packed) - w).abs().max().item() <= 2.0 ** -16 * w.abs().max().item()


# ---- every case of the GPU table -------------------------------------------------------------------------------------------------
def test_gpu_table_covers_the_forms():
    runs = A.GPU_RUNS
    assert {r.kernel for r in runs} == A.ALL_KERNELS
    assert all(r.case.B * r.case.H <= 12 or r.case.name.startswith("big") for r in runs)
    big = [r.case for r in runs if r.case.name.startswith("big")]
    assert big and all(c.B * c.H * ((c.Lq + 15) // 16) > 1024 and c.Lq <= 256 for c in big)
    assert len({r.id for r in runs}) == len(runs)
    m = A.mutants(next(c for c in A.GPU_CASES if c.name == "t5pre"))
    assert {"causal_strict", "causal_dropped", "q_pos0_plus1", "mask_dropped", "mask_shift_right", "mask_shift_left", "mask_len_minus1",
            "last_key_invisible", "key_past_Lk", "bias_sign_flipped", "bias_clamp_min_plus1", "bias_next_head", "skip_t_lo",
            "skip_t_hi"} <= set(m)
    m = A.mutants(next(c for c in A.GPU_CASES if c.name == "dit_o200"))
    assert {"band_wider", "band_narrower", "band_other_convention", "open_from_plus1", "open_from_minus1", "open_keys_ignored",
            "open_queries_ignored", "q_pos0_plus1", "last_key_invisible", "key_past_Lk", "skip_t_lo", "skip_t_hi", "skip_t_open"} <= set(m)
    m = A.mutants(next(c for c in A.GPU_CASES if c.name == "enc200"))
    assert {"bias_sign_flipped", "bias_clamp_min_plus1", "bias_clamp_max_minus1", "bias_next_head", "q_pos0_plus1",
            "last_key_invisible", "key_past_Lk", "skip_t_lo", "skip_t_hi"} <= set(m)
    assert {"band_wider", "band_narrower", "band_other_convention"} <= set(A.mutants(next(c for c in A.GPU_CASES if c.name == "whpre_b-8")))


@pytest.mark.parametrize("case", A.GPU_CASES, ids=lambda c: c.name)
def test_every_mutant_is_ten_tolerances_away(case):
    P = A.prepared(case)
    assert P["mutants"], "a case without a mutant proves nothing about its tolerance"
    for dt in sorted({r.dtype for r in A.GPU_RUNS if r.case == case}):
        floor, tol = P["floor"][dt], P["tol"][dt]
        assert tol == 4 * floor and 0 <= tol < float("inf")
        # one key: softmax is 1 and the output is V itself in every arithmetic -- the only case whose floor is exactly 0
        assert tol > 0 or case.Lk == 1
        assert tol < (6.5e-2 if dt == "bf16" else 3e-5), (dt, tol)     # the bound stays near the project's 3e-2 / 1e-5
        for name, mref in P["mutants"].items():
            n = A.rows_off(mref, P["ref"], 10 * tol)
            assert n >= 4, f"{case.name} {dt}: mutant {name} is 10 tol = {10 * tol:.3g} away in only {n} rows"


def test_fully_masked_rows_exist_in_the_prefill_cases_and_are_zero():
    for c in A.GPU_CASES:
        P = A.prepared(c)
        dead = P["dead_rows"]                                   # [B, Lq]
        if c.pads is not None:
            assert int(dead.sum()) >= 5 + 70 + 149 and not dead.all()
            assert dead[3, :149].all() and not dead[3, 149]
        else:
            assert not dead.any()
        assert (P["ref"].permute(0, 2, 1, 3)[dead] == 0).all()
        assert torch.isfinite(P["ref"]).all()
