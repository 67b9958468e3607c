"""not gpu: the host side of the GEMM kernel tests (mh_testing/gemm.py) -- mh_gemm_last_kernel is declared, bound, exported and callable
without a device; mh_gemm refuses bad geometry before it touches a device; the fp64 reference equals torch's own linear / gelu and a
literal loop per scatter layout; and, for EVERY run tests/test_gpu_gemm.py launches, the floor is finite, the reference passes its own
assertion, the emulation passes it with the factor 1 (instead of 4), and every mutant of the launch (the same launch with one fault) is
at least 10 tolerances away from the reference in at least 4 elements of some output buffer, so that a kernel with that fault cannot
pass.  No launch is without the mutants listed for its epilogue."""
import ctypes as C
import os

import pytest
import torch

from conftest import ROOT
from mapperatorinator_amd import _lib
from mh_testing import gemm as G


# ---- binding -------------------------------------------------------------------------------------------------------------------------
def test_last_kernel_query_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mapperhip.h")).read()
    lib = _lib.load()
    assert "int mh_gemm_last_kernel(void);" in hdr and "mh_gemm_last_kernel" in _lib.SYMBOLS and hasattr(lib, "mh_gemm_last_kernel")
    assert "typedef enum MhGemmKernel" in hdr and "family * 1024 + tile rows" in hdr
    assert lib.mh_abi_version() == 11 and lib.mh_struct_size(9) == -1          # additive: no new entry of the size table
    fams = ("NONE", "TN", "TN_S3", "TN_GLDS", "GLDS3", "GLDS2S", "GLDS4", "S3G", "MX8", "MX8_MXO")
    for i, name in enumerate(fams):
        assert "MH_GEMM_%s = %d" % (name, i) in hdr
        assert getattr(_lib, "GEMM_" + name) == i == getattr(G, "FAM_" + name)
    assert (_lib.EPI_STORE, _lib.EPI_STORE_F32, _lib.EPI_RESID, _lib.EPI_GEGLU, _lib.EPI_BIAS_GELU, _lib.EPI_GATE_RESID, _lib.EPI_KV_SCATTER,
            _lib.EPI_QKV_VT, _lib.EPI_QKV_CACHE, _lib.EPI_BIAS_GELU_ERF) == G.ALL_EPIS
    import threading
    seen = []
    t = threading.Thread(target=lambda: seen.append(lib.mh_gemm_last_kernel()))     # host-only: callable without a device
    t.start()
    t.join()
    assert seen == [G.FAM_NONE]                                                 # thread-local: a thread that launched nothing yet
    kid = lib.mh_gemm_last_kernel()
    assert kid == G.FAM_NONE or (G.FAM_TN <= kid // 1024 <= G.FAM_MX8_MXO and kid % 1024 in (16, 32, 64, 128, 256))


def _descriptor(**kw):
    g = _lib.MhGemm()
    g.A, g.W, g.C = 0x10000, 0x20000, 0x30000          # never dereferenced: every launch below is refused on the host
    g.M, g.N, g.K, g.lda, g.ldw, g.ldc = 64, 64, 64, 64, 64, 64
    g.dtype, g.epilogue = _lib.MH_F32, _lib.EPI_STORE
    for k, v in kw.items():
        setattr(g, k, v)
    return g


REFUSED = [
    (dict(lda=56), b"leading dimension smaller than K"),
    (dict(ldw=32), b"leading dimension smaller than K"),
    (dict(epilogue=_lib.EPI_GEGLU, N=48), b"GEGLU needs N % 32 == 0"),
    (dict(epilogue=_lib.EPI_KV_SCATTER, kv_B=2, kv_H=1, kv_L=31), b"bad KV scatter geometry"),           # M != kv_B * kv_L
    (dict(epilogue=_lib.EPI_KV_SCATTER, kv_B=2, kv_H=3, kv_L=32), b"bad KV scatter geometry"),           # N % (kv_H * 64)
    (dict(epilogue=_lib.EPI_QKV_VT, N=192, C2=0x40000, kv_H=1, kv_L=32, kv_Lpad=31, n_split=128), b"bad QKV_VT geometry"),
    (dict(epilogue=_lib.EPI_QKV_VT, N=192, C2=0x40000, kv_H=1, kv_L=32, kv_Lpad=64, n_split=96), b"bad QKV_VT geometry"),
    (dict(epilogue=_lib.EPI_QKV_VT, N=192, kv_H=1, kv_L=32, kv_Lpad=64, n_split=128), b"bad QKV_VT geometry"),                # no C2
    (dict(epilogue=_lib.EPI_QKV_CACHE, N=192, C2=0x40000, C3=0x50000, C4=0x60000, kv_H=1, kv_L=32, kv_Lpad=64, n_split=64, cache_len=31),
     b"bad QKV_CACHE geometry"),
    (dict(epilogue=_lib.EPI_QKV_CACHE, N=192, C2=0x40000, C3=0x50000, kv_H=1, kv_L=32, kv_Lpad=64, n_split=64, cache_len=40),
     b"bad QKV_CACHE geometry"),                                                                                               # no C4
    (dict(epilogue=_lib.EPI_QKV_CACHE, N=192, C2=0x40000, C3=0x50000, C4=0x60000, kv_H=1, kv_L=48, kv_Lpad=64, n_split=64, cache_len=64),
     b"bad QKV_CACHE geometry"),                                                                                               # M % kv_L
    (dict(epilogue=_lib.EPI_STORE_F32, w_split3=2), b"w_split3 & 2 (A pre-split) needs w_split3 & 1"),
    (dict(epilogue=_lib.EPI_STORE_F32, w_split3=1, ln_stats=0x70000, ln_shift=0x80000, ln_scale=0x90000, ln_strips=4, rows_per_batch=8,
          ln_ld=64), b"not available with w_split3"),
]


@pytest.mark.parametrize("fields,text", REFUSED, ids=[t.decode()[:24].replace(" ", "_") + str(i) for i, (_, t) in enumerate(REFUSED)])
def test_gemm_refuses_bad_geometry_without_a_device(fields, text):
    lib = _lib.load()
    assert lib.mh_gemm(C.byref(_descriptor(**fields)), None) == -1
    assert text in lib.mh_last_error(), lib.mh_last_error()


# ---- the reference itself ---------------------------------------------------------------------------------------------------------
TINY = {dt: G.Run(G.FAM_TN, 16, dt, 19, 20, 24, (), tuple(e for e in G.ALL_EPIS if e != G.GEGLU)) for dt in (G.BF16, G.F32)}
TINY_GEGLU = G.Run(G.FAM_TN, 64, G.F32, 21, 96, 24, (), (G.GEGLU,))


def _window(r, epi, bufs, name="C"):
    g = G.geometry(r, epi)
    return bufs[name][0][:g.M, :g.n_out]


@pytest.mark.parametrize("dt", [G.BF16, G.F32])
def test_reference_equals_torch_linear_and_gelu_in_fp64(dt):
    F = torch.nn.functional
    r = TINY[dt]
    P = G.prepared(r)
    X = P.X
    A, W = X["A"][:r.M].double(), X["W"][:r.N].double()
    if dt == G.BF16:
        assert torch.equal(X["A"], X["A"].to(torch.bfloat16).float()) and torch.equal(X["W"], X["W"].to(torch.bfloat16).float())
    lin = F.linear(A, W, X["bias_plain"][:r.N].double())
    act = F.linear(A, W, X["bias"][:r.N].double())
    old = X["old"][:r.M, :r.N].double()
    g = G.geometry(r, G.GATE_RESID)
    gate = X["gate"][:, :r.N].double()
    rows = torch.arange(r.M)

    def ref(epi, **kw):
        return _window(r, epi, G.evaluate(r, epi, X, P.P, **kw))

    assert (ref(G.STORE) - lin).abs().max() < 1e-13 and (ref(G.STORE_F32) - lin).abs().max() < 1e-13
    assert (ref(G.RESID) - (old + lin)).abs().max() < 1e-13
    assert (ref(G.GATE_RESID) - (old + gate[rows // g.rpb] * lin)).abs().max() < 1e-13
    assert (ref(G.BIAS_GELU) - F.gelu(act, approximate="tanh")).abs().max() < 1e-13
    assert (ref(G.BIAS_GELU_ERF, with_pos=False) - F.gelu(act)).abs().max() < 1e-13
    assert (ref(G.BIAS_GELU_ERF) - (F.gelu(act) + gate[rows % g.rpb])).abs().max() < 1e-13
    # the two GELU forms differ by more than 10 % on the steered columns, which hold pre-activations in [-4, -3]
    st = X["steered"][:r.N]
    assert st.sum() >= 3 and (act[:, st] < -3).all() and (act[:, st] > -4).all()
    a, b = F.gelu(act, approximate="tanh")[:, st], F.gelu(act)[:, st]
    assert ((a - b).abs() > 0.1 * b.abs()).all()
    # the emulation is the same function (loose: only that it is not another one)
    for epi in r.epis:
        emu, want = G.evaluate(r, epi, X, P.P32, emulate=True), G.evaluate(r, epi, X, P.P)
        for name in want:
            assert (emu[name][0] - want[name][0]).abs().max() < 1e-4 and torch.equal(emu[name][1], want[name][1])


def test_reference_geglu_equals_torch():
    F = torch.nn.functional
    r = TINY_GEGLU
    P = G.prepared(r)
    A, W = P.X["A"][:r.M].double(), P.X["W"][:r.N].double()
    Wb = W.reshape(r.N // 32, 2, 16, r.K)                          # 16-row blocks alternate wi_0 / wi_1
    wi0, wi1 = Wb[:, 0].reshape(-1, r.K), Wb[:, 1].reshape(-1, r.K)
    want = F.gelu(F.linear(A, wi0), approximate="tanh") * F.linear(A, wi1)
    got = _window(r, G.GEGLU, G.evaluate(r, G.GEGLU, P.X, P.P))
    assert got.shape == (r.M, r.N // 2) and (got - want).abs().max() < 1e-13


def test_scatter_layouts_equal_a_literal_loop():
    r = TINY[G.F32]
    P = G.prepared(r)
    S = G.SENTINEL
    for epi in (G.KV_SCATTER, G.QKV_VT, G.QKV_CACHE):
        g = G.geometry(r, epi)
        assert g.M == g.B * g.L and g.B == 2 and g.H >= 2
        v = P.P[:g.M, :g.N] + P.X["bias_plain"][:g.N].double()
        sizes = G.buffer_sizes(r, epi)
        want = {k: torch.full(s, S, dtype=torch.float64) for k, s in sizes.items()}
        for m in range(g.M):
            b, i = divmod(m, g.L)
            for n in range(g.N):
                x = v[m, n]
                if epi == G.KV_SCATTER:                      # [(layer, kv)][b][h][key][64]
                    lk, h, dd = n // (g.H * 64), (n // 64) % g.H, n % 64
                    want["C"][:-G.GUARD_ROWS].view(g.LK, g.B, g.H, g.L, 64)[lk, b, h, i, dd] = x
                elif n < g.n_split:                          # the q | k block (QKV_VT), q (QKV_CACHE)
                    want["C"][m, n] = x
                elif epi == G.QKV_VT:                        # V^T [b][h][64][kv_Lpad]
                    h, dd = divmod(n - g.n_split, 64)
                    want["C2"][(b * g.H + h) * 64 + dd, i] = x
                else:                                        # k, v -> [b][h][cache_len][64] at position i; v also transposed
                    kv, c = divmod(n - g.n_split, g.H * 64)
                    h, dd = divmod(c, 64)
                    want["C2" if kv == 0 else "C3"][(b * g.H + h) * g.cache_len + i, dd] = x
                    if kv == 1:
                        want["C4"][(b * g.H + h) * 64 + dd, i] = x
        got = G.evaluate(r, epi, P.X, P.P)
        assert set(got) == set(want)
        for k in want:
            assert torch.equal(got[k][0], want[k]), (G.EPI_NAMES[epi], k)
            assert torch.equal(got[k][1], want[k] != S)
        # what must stay untouched exists in this case: V^T pad columns, cache positions >= kv_L, guard rows
        if epi != G.KV_SCATTER:
            assert g.Lpad > g.L and g.Lpad % 64 == 0
        if epi == G.QKV_CACHE:
            assert g.cache_len > g.L


def test_split3_layout_round_trip():
    g = torch.Generator().manual_seed(4)
    w = torch.randn(5, 64, generator=g)
    hi = w.to(torch.bfloat16).float()
    lo = (w - hi).to(torch.bfloat16).float()
    packed = G.split3_pack(hi, lo, 96)
    assert packed.shape == (5, 192) and packed.dtype == torch.bfloat16
    un = G.split3_unpack(packed.view(torch.float32))
    assert torch.equal(un[:, :64], hi + lo) and (un[:, 64:] == 2 * G.PAD_VALUE * (9984 / 1e4)).all()


# ---- the GPU table ----------------------------------------------------------------------------------------------------------------
def test_gpu_table_reaches_every_built_kernel_with_every_epilogue():
    runs = G.GPU_RUNS
    assert len({r.id for r in runs}) == len(runs)
    reached = {(r.dtype, r.kernel, e) for r in runs for e in r.epis}
    assert reached == G.built_kernels(), sorted(G.built_kernels() ^ reached)
    by_family = {}
    for r in runs:
        by_family.setdefault((r.dtype, r.kernel), []).append(r)
    for key, rs in by_family.items():
        assert {"pad", "ldc4", "off8", "off1"} <= {r.var for r in rs}, key
        for r in rs:
            assert r.lda * r.es >= r.K * r.es + 16 and r.ldw * r.es >= r.K * r.es + 32
    # K below the pipeline depth of the three-stage kernels: one and two K steps
    for fam in (G.FAM_GLDS3, G.FAM_GLDS4, G.FAM_GLDS2S):
        assert {64, 128} <= {r.K for r in runs if r.family == fam}, fam
    for fam in (G.FAM_GLDS3, G.FAM_GLDS4, G.FAM_GLDS2S, G.FAM_S3G):   # both forms of the vector stores: N % 16 == 0 and == 8
        assert {0, 8} <= {r.N % 16 for r in runs if r.family == fam and r.var == "pad"}, fam
    # the wide pre-split BIAS_GELU store of gemm_s3g_kernel (N % 32 == 0, ldc % 32 == 0, C 16-byte aligned) and its narrow form
    wide = [r for r in runs if r.family == G.FAM_S3G and r.var == "pad" and r.N % 32 == 0 and G.geometry(r, G.BIAS_GELU).ldc % 32 == 0]
    assert wide and any(r.N % 32 for r in runs if r.family == G.FAM_S3G)
    for r in wide:
        assert {"split_hi_lo_exchanged", "wide_halves_exchanged", "wide_blocks_exchanged"} <= set(G.epilogue_mutants(r, G.BIAS_GELU))
    assert max(r.M * r.N * r.K for r in runs) <= 2100 * 2052 * 320
    assert any(-(-r.M // 128) * -(-r.N // 128) > 256 for r in runs if r.family == G.FAM_S3G)     # more tiles than the persistent grid


@pytest.mark.parametrize("run", G.GPU_RUNS, ids=lambda r: r.id)
def test_every_mutant_is_ten_tolerances_away(run):
    P = G.prepared(run)
    for epi in run.epis:
        for with_pos in ((True, False) if epi == G.BIAS_GELU_ERF else (True,)):
            what = "%s %s%s" % (run.id, G.EPI_NAMES[epi], "" if with_pos else " (no gate)")
            spec = P.launch(epi, with_pos)
            ref = {k: s["ref"] for k, s in spec.items()}
            emu = {k: v[0] for k, v in G.evaluate(run, epi, P.X, P.P32, emulate=True, with_pos=with_pos).items()}
            for k, s in spec.items():
                assert 0 < s["floor"] < float("inf") and torch.isfinite(s["ref"]).all(), (what, k, s["floor"])
                assert s["floor"] < (2e-5 if run.K <= 128 else 1e-4), (what, k, s["floor"])       # the inputs keep the floor near 1e-6
            assert G.passes(ref, ref, spec) and G.passes(emu, ref, spec, factor=0.25), what
            names = set()
            for name, mref in P.mutants(epi, with_pos):
                names.add(name)
                n = G.elements_off(mref, spec, 10.0)
                assert n >= 4, f"{what}: mutant {name} is 10 tol away in only {n} elements"
                assert not G.passes(ref, mref, spec), (what, name)
            need = set(G.REQUIRED_MUTANTS[epi]) | ({"split_hi_lo_exchanged"} if "C_hi" in spec else set())
            if epi == G.BIAS_GELU_ERF and not with_pos:
                need -= {"div_mod_exchanged", "rpb_plus1", "rpb_minus1", "gate_ld_is_N", "gate_dropped"}
            assert need <= names, (what, sorted(need - names))
            if -(-run.K // run.step) >= 2:
                assert "stale_stage" in names, what
