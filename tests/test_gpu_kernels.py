"""-m gpu: kernel-level parity of libmapperhip (through the C ABI) against plain torch fp32 references
of the same op, and K1 (mel) against the CPU oracle."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from mh_testing.attention import split3_unpack

pytestmark = pytest.mark.gpu


def _lib():
    from mapperatorinator_amd import _lib
    return _lib, _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bf16r(x):
    return x.to(torch.bfloat16).float()


def split3_pack(W):
    """[N, K] fp32 -> the MhGemm.w_split3 layout: every 32-float block as [32 x bf16 hi | 32 x bf16 lo]"""
    n, k = W.shape
    hi = W.to(torch.bfloat16)
    lo = (W - hi.float()).to(torch.bfloat16)
    return torch.stack([hi.reshape(n, k // 32, 32), lo.reshape(n, k // 32, 32)], dim=2).reshape(n, 2 * k).contiguous()


VT_SENTINEL = -768.0      # exact in bf16 and fp32: what the V^T buffer of MH_EPI_QKV_VT holds before the launch


def run_gemm(A, W, epi, dtype, bias=None, C0=None, gate=None, rows_per_batch=0, kv=None, n_split=0, Lpad=0, out_cols=None,
             split3=False):
    L, lib = _lib()
    dev = "cuda"
    td = torch.bfloat16 if dtype == L.MH_BF16 else torch.float32
    M, K = A.shape
    N = W.shape[0]
    Ad, Wd = A.to(dev, td).contiguous(), (split3_pack(W).to(dev) if split3 else W.to(dev, td).contiguous())
    if split3 and int(split3) & 2:          # A pre-split by its producer (the three-stage gemm_s3g_kernel)
        Ad = split3_pack(A).to(dev)
    g = L.MhGemm()
    g.w_split3 = int(split3) if split3 else 0
    g.A, g.lda, g.W, g.ldw = Ad.data_ptr(), K, Wd.data_ptr(), K
    g.M, g.N, g.K, g.dtype, g.epilogue = M, N, K, dtype, epi
    keep = [Ad, Wd]
    if bias is not None:
        b = bias.to(dev, torch.float32).contiguous(); keep.append(b); g.bias = b.data_ptr()
    if epi in (L.EPI_STORE, L.EPI_BIAS_GELU):
        out = torch.zeros((M, N), dtype=td, device=dev); g.C, g.ldc = out.data_ptr(), N
    elif epi == L.EPI_STORE_F32:
        out = torch.zeros((M, N), dtype=torch.float32, device=dev); g.C, g.ldc = out.data_ptr(), N
    elif epi in (L.EPI_RESID, L.EPI_GATE_RESID):
        out = C0.to(dev, torch.float32).contiguous().clone(); g.C, g.ldc = out.data_ptr(), N
        if gate is not None:
            gt = gate.to(dev, torch.float32).contiguous(); keep.append(gt)
            g.gate, g.gate_ld, g.rows_per_batch = gt.data_ptr(), gt.shape[1], rows_per_batch
    elif epi == L.EPI_GEGLU:
        out = torch.zeros((M, N // 2), dtype=td, device=dev); g.C, g.ldc = out.data_ptr(), N // 2
    elif epi == L.EPI_KV_SCATTER:
        B_, H_, L_ = kv
        out = torch.zeros((N // (H_ * 64), B_, H_, L_, 64), dtype=td, device=dev)
        g.C, g.kv_B, g.kv_H, g.kv_L = out.data_ptr(), B_, H_, L_
    elif epi == L.EPI_QKV_VT:
        B_, H_, L_ = kv
        out = torch.zeros((M, n_split), dtype=td, device=dev)
        vt = torch.full((B_, H_, 64, Lpad), VT_SENTINEL, dtype=td, device=dev); keep.append(vt)   # pad columns must be left untouched
        g.C, g.ldc, g.C2, g.n_split, g.kv_B, g.kv_H, g.kv_L, g.kv_Lpad = out.data_ptr(), n_split, vt.data_ptr(), n_split, B_, H_, L_, Lpad
    L.check(lib.mh_gemm(C.byref(g), _stream()), "mh_gemm")
    torch.cuda.synchronize()
    if epi == L.EPI_QKV_VT:
        return out.float().cpu(), vt.float().cpu()
    return out.float().cpu()


def gelu_tanh(x):
    return torch.nn.functional.gelu(x, approximate="tanh")


@pytest.mark.parametrize("dtype_name", ["f32", "bf16"])
@pytest.mark.parametrize("shape", [(300, 200, 96), (1251, 768, 416), (33, 1849, 128), (2600, 1100, 64)])
def test_gemm_store_and_transpose_detecting(dtype_name, shape):
    L, _ = _lib()
    dtype = L.MH_F32 if dtype_name == "f32" else L.MH_BF16
    M, N, K = shape
    g = torch.Generator().manual_seed(M * 7 + N)
    A = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) * torch.linspace(0.5, 2.0, N)[:, None]   # asymmetric
    bias = torch.randn(N, generator=g)
    if dtype == L.MH_BF16:
        A, W = _bf16r(A), _bf16r(W)
    ref = A.double() @ W.double().t() + bias.double()
    out = run_gemm(A, W, L.EPI_STORE_F32, dtype, bias=bias)
    tol = 2e-5 * math.sqrt(K) * 4 + 1e-4
    err = (out.double() - ref).abs().max().item()
    assert err < tol * max(1.0, ref.abs().max().item() / 10), (err, tol)
    out_t = run_gemm(A, W, L.EPI_STORE, dtype, bias=bias)
    rel = 8e-3 if dtype == L.MH_BF16 else 1e-5
    assert ((out_t.double() - ref).abs() <= rel * ref.abs() + 1e-3).all()


@pytest.mark.parametrize("shape", [(1251, 768, 416), (2600, 1100, 768), (700, 520, 2048)])
def test_gemm_lds_dma_tile_equals_register_staged_tile(shape):
    """The 128 x 128 bf16 tile fills its LDS stages by LDS-DMA (`global_load_lds`, option gemm_glds, the default) or by
    register staging: the same products in the same order, so every epilogue's output must be BIT-equal between the two
    and right against fp64.  Shapes with M / N / K tails (K = 416: half a K tile of zeros from the DMA's zero source)."""
    import mapperatorinator_amd._lib as ML
    L, _ = _lib()
    M, N, K = shape
    g = torch.Generator().manual_seed(M + N + K)
    A, W = _bf16r(torch.randn(M, K, generator=g)), _bf16r(torch.randn(N, K, generator=g) * torch.linspace(0.5, 2.0, N)[:, None])
    bias = torch.randn(N, generator=g)
    C0 = torch.randn(M, N, generator=g)
    N2 = N // 32 * 32
    old_min = ML.set_option("gemm_tile128_min", 1)
    outs = {}
    try:
        for glds in (1, 0):
            old = ML.set_option("gemm_glds", glds)
            try:
                outs[glds] = (run_gemm(A, W, L.EPI_STORE_F32, L.MH_BF16, bias=bias), run_gemm(A, W, L.EPI_RESID, L.MH_BF16, C0=C0),
                              run_gemm(A, W[:N2], L.EPI_GEGLU, L.MH_BF16), run_gemm(A, W, L.EPI_STORE, L.MH_BF16))
            finally:
                ML.set_option("gemm_glds", old)
    finally:
        ML.set_option("gemm_tile128_min", old_min)
    for a, b in zip(outs[1], outs[0]):
        assert torch.equal(a, b)
    ref = A.double() @ W.double().t() + bias.double()
    assert (outs[1][0].double() - ref).abs().max().item() < 2e-5 * math.sqrt(K) * 4 + 1e-4


def test_gemm_large_lds_kernel_on_a_second_device():
    """The opt-in to more than 64 KB of dynamic LDS is an attribute of a kernel ON ONE DEVICE: gemm_prepare() keeps its "done"
    per device.  A bf16 GEMM that takes the three-stage 128 x 128 LDS-DMA kernel (96 KB) runs on device 0, then on device 1 of
    the same process, and both are right against fp64 (the bound of test_gemm_store_and_transpose_detecting)."""
    if torch.cuda.device_count() < 2:
        pytest.skip("one visible device")
    import mapperatorinator_amd._lib as ML
    L, _ = _lib()
    M, N, K = 2600, 1100, 768
    g = torch.Generator().manual_seed(5)
    A, W = _bf16r(torch.randn(M, K, generator=g)), _bf16r(torch.randn(N, K, generator=g))
    bias = torch.randn(N, generator=g)
    ref = A.double() @ W.double().t() + bias.double()
    old_min = ML.set_option("gemm_tile128_min", 1)
    try:
        for dev in (0, 1):
            with torch.cuda.device(dev):
                out = run_gemm(A, W, L.EPI_STORE_F32, L.MH_BF16, bias=bias)
            err = (out.double() - ref).abs().max().item()
            print(f"device {dev}: max |err| {err:.3e}")
            assert err < (2e-5 * math.sqrt(K) * 4 + 1e-4) * max(1.0, ref.abs().max().item() / 10), (dev, err)
    finally:
        ML.set_option("gemm_tile128_min", old_min)


def test_gemm_bf16x3_refuses_the_fused_layernorm_prologue():
    """LayerNorm + modulate fused into the bf16 x 3 GEMM's A load (an option of the batched DiT until round 5, measured slower
    than the stand-alone pass) once returned non-repeatable rows and did so again after an unrelated edit; the cause was never
    isolated.  The combination is refused by mh_gemm -- loudly -- instead of shipped."""
    L, lib = _lib()
    M, N, K = 256, 128, 64
    A = torch.zeros(M, K, device="cuda"); W = torch.zeros(N, 2 * K, device="cuda"); out = torch.zeros(M, N, device="cuda")
    st = torch.zeros(K // 16, M, 2, device="cuda"); mod = torch.zeros(2, K, device="cuda")
    gm = L.MhGemm()
    gm.A, gm.lda, gm.W, gm.ldw, gm.C, gm.ldc = A.data_ptr(), K, W.data_ptr(), K, out.data_ptr(), N
    gm.M, gm.N, gm.K, gm.dtype, gm.epilogue, gm.w_split3 = M, N, K, L.MH_F32, L.EPI_STORE_F32, 1
    gm.ln_stats, gm.ln_strips, gm.ln_shift, gm.ln_scale, gm.ln_ld, gm.ln_eps, gm.rows_per_batch = (
        st.data_ptr(), K // 16, mod.data_ptr(), mod.data_ptr(), K, 0.0, 128)
    assert lib.mh_gemm(C.byref(gm), _stream()) != 0
    assert b"w_split3" in lib.mh_last_error()


def test_gemm_fused_layernorm_prologue_is_bit_repeatable():
    """the LayerNorm + modulate prologue of the fp32 GEMM (MhGemm.ln_stats: statistics written by the producer's
    epilogue, reduced into LDS, applied on the A load) still ships for the non-split3 path (dit.hip `fuse_ln && !g.w_split3`: 2-7
    chunk batches).  Its bf16 x 3 sibling once returned non-repeatable rows and is refused; THIS form is held to: six runs of the
    same launch bit-identical (grid of 1152 workgroups), and with an identity modulation equal to the plain GEMM on F.layer_norm'd
    rows to fp32 rounding -- for a well-conditioned and for a large-mean input."""
    L, lib = _lib()
    g = torch.Generator().manual_seed(21)
    M, D, N2, rpb = 4096, 384, 1152, 128
    for shift_mean in (0.0, 40.0):
        A0 = torch.randn(M, 96, generator=g)
        W0 = torch.randn(D, 96, generator=g) * 0.3
        b0 = torch.randn(D, generator=g) * 0.1 + shift_mean
        W1 = torch.randn(N2, D, generator=g) * D ** -0.5
        A0d, W0d, b0d, W1d = A0.cuda(), W0.cuda(), b0.cuda(), W1.cuda()
        xs = torch.zeros(M, D, device="cuda")
        stats = torch.zeros(D // 16, M, 2, device="cuda")
        gp = L.MhGemm()
        gp.A, gp.lda, gp.W, gp.ldw, gp.C, gp.ldc = A0d.data_ptr(), 96, W0d.data_ptr(), 96, xs.data_ptr(), D
        gp.M, gp.N, gp.K, gp.bias, gp.dtype, gp.epilogue, gp.stats_out = M, D, 96, b0d.data_ptr(), L.MH_F32, L.EPI_STORE_F32, stats.data_ptr()
        L.check(lib.mh_gemm(C.byref(gp), _stream()), "producer")
        nb = M // rpb
        shift = torch.randn(nb, D, generator=g).cuda() * 0.1
        scale = torch.randn(nb, D, generator=g).cuda() * 0.1
        outs = []
        for ident in (False, True):
            sh = torch.zeros_like(shift) if ident else shift
            sc = torch.zeros_like(scale) if ident else scale
            for rep in range(6 if not ident else 1):
                out = torch.full((M, N2), float("nan"), device="cuda")
                gc = L.MhGemm()
                gc.A, gc.lda, gc.W, gc.ldw, gc.C, gc.ldc = xs.data_ptr(), D, W1d.data_ptr(), D, out.data_ptr(), N2
                gc.M, gc.N, gc.K, gc.dtype, gc.epilogue = M, N2, D, L.MH_F32, L.EPI_STORE_F32
                gc.ln_stats, gc.ln_strips, gc.ln_shift, gc.ln_scale, gc.ln_ld, gc.ln_eps, gc.rows_per_batch = (
                    stats.data_ptr(), D // 16, sh.data_ptr(), sc.data_ptr(), D, 1e-6, rpb)
                L.check(lib.mh_gemm(C.byref(gc), _stream()), "consumer")
                torch.cuda.synchronize()
                outs.append(out.cpu())
        for rep in range(1, 6):
            assert torch.equal(outs[rep], outs[0]), f"fused LayerNorm prologue: run {rep} differs from run 0 (mean shift {shift_mean})"
        xs_h = xs.cpu().double()
        ln = torch.nn.functional.layer_norm(xs_h, (D,), eps=1e-6)
        ref_mod = (ln * (1 + scale.cpu().double().repeat_interleave(rpb, 0)) + shift.cpu().double().repeat_interleave(rpb, 0)) @ W1.double().t()
        ref_id = ln @ W1.double().t()
        e_mod, e_id = (outs[0].double() - ref_mod).abs().max().item(), (outs[6].double() - ref_id).abs().max().item()
        print(f"fused LN prologue, row mean ~{shift_mean}: 6 runs identical; max err vs fp64 modulated {e_mod:.2e}, identity {e_id:.2e}")
        # (the strip statistics are sums / sums of squares: at |mu| = 40 sigma ~ 1 the variance carries ~1e-4 relative error)
        tol = 5e-4 if shift_mean == 0.0 else 2e-2
        assert e_mod < tol and e_id < tol


def test_gemm_bf16x3_split_path():
    """MhGemm.w_split3 (fp32 GEMM as three bf16 MFMAs on pre-split weights, activations split on the way into LDS):
    ~2^-16 relative error per product -- two orders of magnitude tighter than bf16, one looser than exact fp32 -- on
    every epilogue the DiT uses, incl. ragged M / N and the K tail of a 64-wide tile."""
    L, _ = _lib()
    g = torch.Generator().manual_seed(8)
    M, N, K = 333, 200, 416                      # M, N not tile multiples; K = 13 blocks of 32
    A = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) * torch.linspace(0.5, 2.0, N)[:, None]
    bias = torch.randn(N, generator=g)
    ref = A.double() @ W.double().t() + bias.double()
    exact = run_gemm(A, W, L.EPI_STORE_F32, L.MH_F32, bias=bias)
    split = run_gemm(A, W, L.EPI_STORE_F32, L.MH_F32, bias=bias, split3=True)
    scale = (A.abs().double() @ W.abs().double().t()).max().item()
    e_exact, e_split = (exact.double() - ref).abs().max().item() / scale, (split.double() - ref).abs().max().item() / scale
    print(f"relative to sum|a||w|: exact fp32 {e_exact:.2e}, bf16x3 {e_split:.2e}")
    assert e_split < 3e-5 and e_split > 0 and e_exact < 2e-6
    out = run_gemm(A, W, L.EPI_BIAS_GELU, L.MH_F32, bias=bias, split3=True)
    assert torch.allclose(out, gelu_tanh(ref.float()), atol=2e-3, rtol=1e-4)
    C0 = torch.randn(M, N, generator=g)
    gate = torch.randn(3, N, generator=g)
    out = run_gemm(A, W, L.EPI_GATE_RESID, L.MH_F32, bias=bias, C0=C0, gate=gate, rows_per_batch=111, split3=True)
    assert torch.allclose(out, C0 + gate.repeat_interleave(111, dim=0) * ref.float(), atol=3e-3, rtol=1e-4)


def test_gemm_bf16x3_presplit_three_stage_path():
    """MhGemm.w_split3 = 3 / 7: both operands pre-split, the three-stage LDS-DMA kernel (gemm_s3g_kernel).  Same products
    and the same summation order per 32-k block as the 64 x 64 split kernel, so the two agree to fp32 rounding; ragged M
    (clamped rows), small and large grids, the pre-split BIAS_GELU output."""
    L, _ = _lib()
    g = torch.Generator().manual_seed(18)
    for M, N, K in ((700, 384, 416), (2300, 1536, 384), (4100, 1152, 768)):
        A = torch.randn(M, K, generator=g)
        W = torch.randn(N, K, generator=g) * torch.linspace(0.5, 2.0, N)[:, None]
        bias = torch.randn(N, generator=g)
        ref = A.double() @ W.double().t() + bias.double()
        scale = (A.abs().double() @ W.abs().double().t()).max().item()
        old = run_gemm(A, W, L.EPI_STORE_F32, L.MH_F32, bias=bias, split3=1)
        new = run_gemm(A, W, L.EPI_STORE_F32, L.MH_F32, bias=bias, split3=3)
        e_new, d_on = (new.double() - ref).abs().max().item() / scale, (new - old).abs().max().item() / scale
        print(f"M={M} N={N} K={K}: pre-split path vs fp64 {e_new:.2e}, vs the 64x64 split kernel {d_on:.2e} (of sum|a||w|)")
        assert e_new < 3e-5 and d_on < 2e-7
        C0 = torch.randn(M, N, generator=g)
        gate = torch.randn(-(-M // 100), N, generator=g)
        out = run_gemm(A, W, L.EPI_GATE_RESID, L.MH_F32, bias=bias, C0=C0, gate=gate, rows_per_batch=100, split3=3)
        assert torch.allclose(out, C0 + gate.repeat_interleave(100, dim=0)[:M] * ref.float(), atol=3e-3, rtol=1e-4)
        out = run_gemm(A, W, L.EPI_BIAS_GELU, L.MH_F32, bias=bias, split3=7)          # fp32-sized buffer holding [hi | lo] blocks
        got = split3_unpack(out)
        want = gelu_tanh(ref.float())
        assert torch.allclose(got, want, atol=2e-3, rtol=1e-4)
        assert (got - want).abs().max().item() < 2e-3 and (got - _bf16r(want)).abs().max().item() > 0      # hi + lo, not bf16


@pytest.mark.parametrize("dtype_name", ["f32", "bf16"])
def test_gemm_epilogues(dtype_name):
    L, _ = _lib()
    dtype = L.MH_F32 if dtype_name == "f32" else L.MH_BF16
    g = torch.Generator().manual_seed(5)
    M, N, K = 260, 192, 160
    A, W = torch.randn(M, K, generator=g) * 0.5, torch.randn(N, K, generator=g) * 0.2
    if dtype == L.MH_BF16:
        A, W = _bf16r(A), _bf16r(W)
    bias = torch.randn(N, generator=g) * 0.1
    acc = (A.double() @ W.double().t()).float()
    rel = 1e-2 if dtype == L.MH_BF16 else 2e-5
    # RESID
    C0 = torch.randn(M, N, generator=g)
    out = run_gemm(A, W, L.EPI_RESID, dtype, C0=C0)
    assert torch.allclose(out, C0 + acc, atol=1e-3, rtol=1e-4)
    # BIAS_GELU
    out = run_gemm(A, W, L.EPI_BIAS_GELU, dtype, bias=bias)
    assert torch.allclose(out, gelu_tanh(acc + bias), atol=2e-3, rtol=rel)
    # GATE_RESID (rows_per_batch = 130 -> 2 batches)
    gate = torch.randn(2, 3 * N, generator=g)
    # gate passed as the [:, N:] view of a [2, 3N] modulation matrix: ld = 2N after .contiguous(), first N used
    gexp = gate[:, N:2 * N].repeat_interleave(130, dim=0)
    out2 = run_gemm(A, W, L.EPI_GATE_RESID, dtype, bias=bias, C0=C0, gate=gate[:, N:], rows_per_batch=130)
    assert torch.allclose(out2, C0 + gexp * (acc + bias), atol=2e-3, rtol=1e-4)
    # GEGLU: interleave wi0 / wi1 in 16-row blocks
    dff = N // 2
    wi0, wi1 = W[:dff], W[dff:]
    Wi = torch.stack([wi0.reshape(dff // 16, 16, K), wi1.reshape(dff // 16, 16, K)], 1).reshape(2 * dff, K)
    out = run_gemm(A, Wi, L.EPI_GEGLU, dtype)
    exp = gelu_tanh((A.double() @ wi0.double().t()).float()) * (A.double() @ wi1.double().t()).float()
    assert torch.allclose(out, exp, atol=3e-3, rtol=rel), (out - exp).abs().max()


@pytest.mark.parametrize("dtype_name", ["f32", "bf16"])
def test_gemm_kv_scatter_and_qkv_vt(dtype_name):
    L, _ = _lib()
    dtype = L.MH_F32 if dtype_name == "f32" else L.MH_BF16
    g = torch.Generator().manual_seed(6)
    B_, H_, L_, K = 2, 3, 70, 64
    M = B_ * L_
    A = torch.randn(M, K, generator=g)
    nl = 2
    W = torch.randn(nl * 2 * H_ * 64, K, generator=g) * 0.2
    if dtype == L.MH_BF16:
        A, W = _bf16r(A), _bf16r(W)
    out = run_gemm(A, W, L.EPI_KV_SCATTER, dtype, kv=(B_, H_, L_))
    full = (A.double() @ W.double().t()).float()               # [M, nl*2*H*64]
    exp = full.view(B_, L_, nl * 2, H_, 64).permute(2, 0, 3, 1, 4)   # [(l,kv), B, H, L, 64]
    tol = 2e-2 if dtype == L.MH_BF16 else 1e-4
    assert torch.allclose(out, exp, atol=tol, rtol=1e-2 if dtype == L.MH_BF16 else 1e-5)
    # QKV_VT
    Wq = torch.randn(3 * H_ * 64, K, generator=g) * 0.2
    if dtype == L.MH_BF16:
        Wq = _bf16r(Wq)
    qk, vt = run_gemm(A, Wq, L.EPI_QKV_VT, dtype, kv=(B_, H_, L_), n_split=2 * H_ * 64, Lpad=128)
    full = (A.double() @ Wq.double().t()).float()
    assert torch.allclose(qk, full[:, :2 * H_ * 64], atol=tol, rtol=1e-2)
    v = full[:, 2 * H_ * 64:].view(B_, L_, H_, 64).permute(0, 2, 3, 1)   # [B,H,64,L]
    assert torch.allclose(vt[..., :L_], v, atol=tol, rtol=1e-2)
    assert (vt[..., L_:] == VT_SENTINEL).all()              # the pad columns [kv_L, kv_Lpad) were not written


@pytest.mark.parametrize("dtype_name", ["f32", "bf16"])
def test_rmsnorm(dtype_name):
    L, lib = _lib()
    dt = L.MH_F32 if dtype_name == "f32" else L.MH_BF16
    g = torch.Generator().manual_seed(1)
    x = torch.randn(37, 768, generator=g) * 3
    w = 1 + 0.1 * torch.randn(768, generator=g)
    xd, wd = x.cuda(), w.cuda()
    y = torch.empty((37, 768), dtype=torch.bfloat16 if dt == L.MH_BF16 else torch.float32, device="cuda")
    L.check(lib.mh_rmsnorm(xd.data_ptr(), 768, wd.data_ptr(), y.data_ptr(), 768, 37, 768, 1e-6, dt, _stream()))
    ref = w * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-6))
    tol = 2e-2 if dt == L.MH_BF16 else 2e-6
    assert torch.allclose(y.float().cpu(), ref, atol=tol, rtol=8e-3 if dt == L.MH_BF16 else 1e-5)


@pytest.mark.parametrize("dtype_name", ["f32", "bf16"])
def test_layernorm_affine(dtype_name):
    """mh_layernorm (the pre-norm of HF Whisper's blocks, library arch 2) vs torch F.layer_norm in fp64, rows with a mean far above
    their spread included (|mu| >> sigma: the two-pass arithmetic must hold)."""
    L, lib = _lib()
    dt = L.MH_F32 if dtype_name == "f32" else L.MH_BF16
    g = torch.Generator().manual_seed(2)
    x = torch.randn(41, 768, generator=g) * 3
    x[5] = x[5] * 0.01 + 300.0
    x[6] = x[6] * 1e-3 - 1000.0
    w, b = 1 + 0.1 * torch.randn(768, generator=g), 0.1 * torch.randn(768, generator=g)
    xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
    y = torch.empty((41, 768), dtype=torch.bfloat16 if dt == L.MH_BF16 else torch.float32, device="cuda")
    L.check(lib.mh_layernorm(xd.data_ptr(), 768, wd.data_ptr(), bd.data_ptr(), y.data_ptr(), 768, 41, 768, 1e-5, dt, _stream()))
    ref = torch.nn.functional.layer_norm(x.double(), (768,), w.double(), b.double(), 1e-5).float()
    err = (y.float().cpu() - ref).abs()
    # rows 5 / 6: sigma = 0.03 / 3e-3 at |mu| = 300 / 1000.  The fp32 MEAN of 768 such values is good to a few ulp of the sum
    # (2.3e5 -> 0.016 / 768 = 2e-5), i.e. 1e-3 / 2e-2 of sigma: that is the floor of any fp32 two-pass LayerNorm (measured 3.5e-4 /
    # 6e-3 here); a single-pass E[x^2] - mu^2 form would lose ALL digits on these rows
    tol = 2e-2 if dt == L.MH_BF16 else 2e-5
    assert err[:5].max().item() < tol and err[7:].max().item() < tol and err[5].max().item() < max(tol, 2e-3) and err[6].max().item() < 5e-2, \
        (err[:5].max(), err[5].max(), err[6].max())


def ref_attention(q, k, v, bias=None, scale=1.0, band=0):
    """q,k,v [B,H,L,64] fp64 reference of mh_attention."""
    s = torch.matmul(q.double(), k.double().transpose(-1, -2)) * scale
    Ln = q.shape[2]
    if bias is not None:
        rel = torch.arange(Ln)[None, :] - torch.arange(Ln)[:, None]
        s = s + bias.double()[:, rel + Ln - 1][None]
    if band > 0:
        rel = torch.arange(Ln)[None, :] - torch.arange(Ln)[:, None]
        ok = (rel >= -(band - 1)) & (rel <= band)
        s = s.masked_fill(~ok, float("-inf"))
    return torch.matmul(torch.softmax(s, -1), v.double()).float()


@pytest.mark.parametrize("dtype_name", ["f32", "bf16"])
@pytest.mark.parametrize("case", [dict(B=2, H=3, L=251, bias=True, scale=1.0, band=0),
                                  dict(B=1, H=2, L=1251, bias=True, scale=1.0, band=0),
                                  dict(B=2, H=2, L=400, bias=False, scale=0.125, band=128),
                                  dict(B=2, H=1, L=96, bias=False, scale=0.125, band=128),
                                  # short fp32 sequences without bias take the key-split kernel (attn_small_f32_kernel)
                                  dict(B=2, H=2, L=96, bias=False, scale=0.125, band=0),
                                  dict(B=2, H=2, L=128, bias=False, scale=0.125, band=0),
                                  dict(B=1, H=3, L=160, bias=False, scale=0.125, band=32),
                                  dict(B=2, H=2, L=250, bias=False, scale=0.125, band=128)])
def test_attention(dtype_name, case):
    L, lib = _lib()
    dt = L.MH_F32 if dtype_name == "f32" else L.MH_BF16
    td = torch.bfloat16 if dt == L.MH_BF16 else torch.float32
    B_, H_, Ln = case["B"], case["H"], case["L"]
    g = torch.Generator().manual_seed(Ln)
    q = torch.randn(B_, H_, Ln, 64, generator=g) * 0.6
    k = torch.randn(B_, H_, Ln, 64, generator=g) * 0.6
    v = torch.randn(B_, H_, Ln, 64, generator=g)
    if dt == L.MH_BF16:
        q, k, v = _bf16r(q), _bf16r(k), _bf16r(v)
    bias = (torch.randn(H_, 2 * Ln - 1, generator=g) * 0.5) if case["bias"] else None
    inner = H_ * 64
    qk = torch.cat([q.permute(0, 2, 1, 3).reshape(B_ * Ln, inner), k.permute(0, 2, 1, 3).reshape(B_ * Ln, inner)], 1)
    Lpad = (Ln + 63) // 64 * 64
    vt = torch.zeros(B_, H_, 64, Lpad)
    vt[..., :Ln] = v.transpose(-1, -2)
    qk_d, vt_d = qk.to("cuda", td).contiguous(), vt.to("cuda", td).contiguous()
    out = torch.zeros(B_ * Ln, inner, dtype=td, device="cuda")
    bias_d = bias.cuda().contiguous() if bias is not None else None
    L.check(lib.mh_attention(qk_d.data_ptr(), 2 * inner, inner, vt_d.data_ptr(), Lpad, L.ptr(bias_d), out.data_ptr(),
                             inner, B_, Ln, H_, case["scale"], case["band"], dt, _stream()), "mh_attention")
    torch.cuda.synchronize()
    ref = ref_attention(q, k, v, bias, case["scale"], case["band"]).permute(0, 2, 1, 3).reshape(B_ * Ln, inner)
    err = (out.float().cpu() - ref).abs().max().item()
    assert err < (3e-2 if dt == L.MH_BF16 else 2e-5), err


@pytest.mark.parametrize("B,ns", [(1, 16000), (3, 160000), (2, 32000 + 77)])
def test_mel_vs_oracle(B, ns):
    from mapperatorinator_amd.mel import MelSpectrogram
    from mh_testing import synthetic_audio
    from oracle import mel as omel
    a = synthetic_audio(B, ns, seed=9)
    m = MelSpectrogram().cuda()
    got = m(a.cuda()).cpu()
    want = omel.mel_spectrogram(a)
    assert got.shape == want.shape == (B, ns // 128 + 1, 388)
    f64 = torch.from_numpy(omel.mel_spectrogram_f64(a.numpy())).float()
    scale = want.abs().max().item()
    e_or = (got - want).abs().max().item() / scale
    e_f64 = (got - f64).abs().max().item() / scale
    o_f64 = (want - f64).abs().max().item() / scale
    print(f"mel rel-to-max err: hip-vs-oracle {e_or:.2e}, hip-vs-f64 {e_f64:.2e}, oracle-vs-f64 {o_f64:.2e}")
    # tolerance: 1e-4 of the spectrum peak (fp32 DFT-by-conv vs fp32 FFT differ by accumulated rounding)
    assert e_or < 1e-4 and e_f64 < 1e-4
    # elementwise relative where the value is not tiny
    big = want > 1e-3 * scale
    assert ((got - want).abs()[big] / want[big]).max().item() < 2e-3
    # zero filterbank rows stay exactly zero; padded K columns are zero
    zero_rows = (want.abs().sum((0, 1)) == 0)
    assert (got[..., zero_rows] == 0).all()
    pad = m.forward_padded(a.cuda(), 416, torch.bfloat16)
    assert pad.shape[-1] == 416 and (pad[..., 388:] == 0).all()
    assert torch.allclose(pad[..., :388].float().cpu(), want, rtol=1e-2, atol=1e-4 * scale)


@pytest.mark.parametrize("ns", [16000, 160000, 12345])
def test_mel_torchaudio_parameterisation_vs_oracle(ns):
    """The Whisper-family front-end settings (configs/model/whisper_base_v3.yaml:16-21: torchaudio, log-mel, 128 HTK mels
    from 20 Hz, reflect padding) against the torch.stft restatement of that branch (oracle/mel.py; parity unpinned:
    torchaudio itself is not installed).  The edge frames are the ones reflect padding changes."""
    from mapperatorinator_amd.mel import MelSpectrogram
    from mh_testing import synthetic_audio
    from oracle import mel as omel
    a = synthetic_audio(2, ns, seed=4)
    m = MelSpectrogram(implementation="torchaudio", log_scale=True, n_mels=128, f_min=20, pad_mode="reflect").cuda()
    got = m(a.cuda()).cpu()
    want = omel.mel_spectrogram_torchaudio(a, n_mels=128, f_min=20.0, pad_mode="reflect", log_scale=True)
    assert got.shape == want.shape == (2, ns // 128 + 1, 128)
    err = (got - want).abs()
    print(f"torchaudio-style log-mel: max |d| {err.max().item():.2e} (values up to {want.max().item():.2f}), "
          f"first / last frame {err[:, 0].max().item():.2e} / {err[:, -1].max().item():.2e}")
    assert err.max().item() < 2e-3                     # log1p domain
    lin = MelSpectrogram(implementation="torchaudio", log_scale=False, n_mels=128, f_min=20, pad_mode="constant").cuda()(a.cuda()).cpu()
    wl = omel.mel_spectrogram_torchaudio(a, n_mels=128, f_min=20.0, pad_mode="constant", log_scale=False)
    assert (lin - wl).abs().max().item() < 1e-4 * wl.abs().max().item()
    assert (got[:, 0] - torch.log1p(lin[:, 0])).abs().max().item() > 1e-3      # reflect padding really differs from zeros at the edge


def test_mel_silence_and_tone():
    from mapperatorinator_amd.mel import MelSpectrogram
    m = MelSpectrogram().cuda()
    z = torch.zeros(1, 16000, device="cuda")
    assert (m(z) == 0).all()
    n = torch.arange(16000, dtype=torch.float64)
    k0 = 100
    tone = torch.cos(2 * math.pi * k0 * n / 1024).float()[None]
    mel = m(tone.cuda()).cpu()[0, 40]          # a frame fully inside the signal
    # total energy = sum_k P[k] * colsum(W) -> compare against the f64 formulation
    from oracle import mel as omel
    ref = torch.from_numpy(omel.mel_spectrogram_f64(tone.numpy()))[0, 40].float()
    assert torch.allclose(mel, ref, rtol=1e-3, atol=1e-3 * ref.max().item())


def _whisper_case():
    g = np.load(f"{__import__('conftest').GOLDEN}/whisper_frontend.npz")
    rng = np.random.default_rng(int(g["seed"]))
    d, c, Ln = int(g["d"]), int(g["c_in"]), int(g["L"])

    def rnd(shape, std):
        return torch.from_numpy((rng.standard_normal(shape) * std).astype(np.float32))
    w1, b1 = rnd((d, c, 3), 0.08), rnd((d,), 0.05)
    w2, b2 = rnd((d, d, 3), 0.06), rnd((d,), 0.05)
    x = rnd((2, c, Ln), 1.0)
    return g, x, w1, b1, w2, b2, torch.from_numpy(g["pos"])


@pytest.mark.parametrize("dtype_name", ["f32", "bf16"])
def test_whisper_frontend(dtype_name):
    """K2 vs the HF WhisperEncoder golden (fp32: 2e-5 abs) and vs the bf16-contract oracle (bf16: 3e-2 abs)."""
    from mapperatorinator_amd.whisper_frontend import WhisperFrontendHIP
    from oracle.whisper_frontend import whisper_frontend
    g, x, w1, b1, w2, b2, pos = _whisper_case()
    dt = torch.float32 if dtype_name == "f32" else torch.bfloat16
    fe = WhisperFrontendHIP(w1, b1, w2, b2, pos, dtype=dt)
    got = fe(x.cuda()).float().cpu()
    assert got.shape == (2, 75, 128)
    if dt == torch.float32:
        err = (got - torch.from_numpy(g["out"])).abs().max().item()
        print("whisper front-end fp32 max abs err vs HF golden", err)
        assert err < 2e-5
    else:
        want = whisper_frontend(x, w1, b1, w2, b2, pos, rounding="bf16")
        err = (got - want).abs().max().item()
        print("whisper front-end bf16 max abs err vs bf16 oracle", err)
        assert err < 3e-2
    # no position table: the reference's VarWhisperEncoder conv stack (golden `out_var`, made by the imported fork)
    fe2 = WhisperFrontendHIP(w1, b1, w2, b2, None, dtype=dt)
    got_var = fe2(x.cuda()).float().cpu()
    err_var = (got_var - torch.from_numpy(g["out_var"])).abs().max().item()
    print("whisper front-end", dtype_name, "max abs err vs the reference VarWhisperEncoder golden", err_var)
    assert err_var < (2e-5 if dt == torch.float32 else 3e-2)
    # odd length, batch 3
    x2 = torch.randn(3, 96, 77, generator=torch.Generator().manual_seed(1))
    got2 = fe2(x2.cuda()).float().cpu()
    want2 = whisper_frontend(x2, w1, b1, w2, b2, None, rounding=None if dt == torch.float32 else "bf16")
    assert got2.shape == want2.shape == (3, 39, 128)
    assert (got2 - want2).abs().max().item() < (2e-5 if dt == torch.float32 else 3e-2)


@pytest.mark.parametrize("case", ["STORE", "STORE_F32", "RESID_k768", "RESID_k2048", "GEGLU", "BIAS_GELU", "QKV_VT", "KV_SCATTER", "ragged"])
def test_gemm_256sq_tile_is_bit_identical_to_the_three_stage_kernel(case):
    """gemm_glds4_kernel (256 x 256 tile, 128 x 64 wave tiles, AGPR accumulators, asm MFMAs; the encoder's GEMMs at 32 chunks)
    accumulates the same products in the same order as gemm_glds3_kernel and shares its epilogues: every output bit must agree,
    for every epilogue the T5 path uses and for ragged M / N / short K.  (It caught hipcc scheduling an accumulator read in
    between the final asm MFMAs: the GEGLU epilogue then saw acc[0][0] one K step old.)"""
    L, _ = _lib()
    M = 5 * 1251 if case in ("QKV_VT", "KV_SCATTER") else (4099 if case == "ragged" else 6000)
    g = torch.Generator().manual_seed(len(case))
    A768 = torch.randn(M, 768, generator=g)
    w = lambda n, k, sc=0.05: torch.randn(n, k, generator=g) * sc
    if case == "STORE":
        fn = lambda W=w(2304, 768, 1.0): run_gemm(A768, W, L.EPI_STORE, L.MH_BF16)
    elif case == "STORE_F32":
        fn = lambda W=w(768, 768, 1.0): run_gemm(A768, W, L.EPI_STORE_F32, L.MH_BF16)
    elif case == "RESID_k768":
        fn = lambda W=w(768, 768), C0=torch.randn(M, 768, generator=g): run_gemm(A768, W, L.EPI_RESID, L.MH_BF16, C0=C0)
    elif case == "RESID_k2048":
        fn = lambda A=torch.randn(M, 2048, generator=g), W=w(768, 2048), C0=torch.randn(M, 768, generator=g): run_gemm(A, W, L.EPI_RESID, L.MH_BF16, C0=C0)
    elif case == "GEGLU":
        fn = lambda W=w(4096, 768): run_gemm(A768, W, L.EPI_GEGLU, L.MH_BF16)
    elif case == "BIAS_GELU":
        fn = lambda W=w(3072, 768), b=torch.randn(3072, generator=g): run_gemm(A768, W, L.EPI_BIAS_GELU, L.MH_BF16, bias=b)
    elif case == "QKV_VT":
        fn = lambda W=w(2304, 768): run_gemm(A768, W, L.EPI_QKV_VT, L.MH_BF16, kv=(5, 12, 1251), n_split=1536, Lpad=1280)
    elif case == "KV_SCATTER":
        fn = lambda W=w(2 * 2 * 768, 768): run_gemm(A768, W, L.EPI_KV_SCATTER, L.MH_BF16, kv=(5, 12, 1251))
    else:
        fn = lambda A=torch.randn(M, 192, generator=g), W=w(1284, 192, 1.0): run_gemm(A, W, L.EPI_STORE, L.MH_BF16)
    outs = []
    old = L.set_option("gemm_tile256sq_min", 0)
    try:
        for thr in (0, 1):
            L.set_option("gemm_tile256sq_min", thr)
            outs.append(fn())
    finally:
        L.set_option("gemm_tile256sq_min", old)
    a, b = outs
    if isinstance(a, tuple):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    else:
        assert torch.equal(a, b), (a - b).abs().max().item()


@pytest.mark.parametrize("case", ["STORE", "GATE_RESID", "BIAS_GELU", "RESID_ragged", "QKV_VT"])
def test_gemm_two_stage_tile_is_bit_identical_to_the_three_stage_kernel(case):
    """gemm_glds2s_kernel (128 x 128 tile, two LDS stages = 64 KB: two workgroups per CU; the batched DiT's short-K projections)
    against the three-stage kernels: same products, same order, same epilogues -- every output bit."""
    L, _ = _lib()
    g = torch.Generator().manual_seed(3 + len(case))
    M = 8192
    if case == "STORE":
        fn = lambda A=torch.randn(M, 384, generator=g), W=torch.randn(1152, 384, generator=g): run_gemm(A, W, L.EPI_STORE, L.MH_BF16)
    elif case == "GATE_RESID":
        fn = lambda A=torch.randn(M, 1536, generator=g), W=torch.randn(384, 1536, generator=g) * 0.05, C0=torch.randn(M, 384, generator=g), G=torch.randn(64, 384, generator=g): run_gemm(
            A, W, L.EPI_GATE_RESID, L.MH_BF16, C0=C0, gate=G, rows_per_batch=128)
    elif case == "BIAS_GELU":
        fn = lambda A=torch.randn(M, 384, generator=g), W=torch.randn(1536, 384, generator=g) * 0.05, b=torch.randn(1536, generator=g): run_gemm(
            A, W, L.EPI_BIAS_GELU, L.MH_BF16, bias=b)
    elif case == "RESID_ragged":
        fn = lambda A=torch.randn(4099, 192, generator=g), W=torch.randn(1284, 192, generator=g), C0=torch.randn(4099, 1284, generator=g): run_gemm(
            A, W, L.EPI_RESID, L.MH_BF16, C0=C0)
    else:
        fn = lambda A=torch.randn(64 * 128, 384, generator=g), W=torch.randn(1152, 384, generator=g) * 0.05: run_gemm(
            A, W, L.EPI_QKV_VT, L.MH_BF16, kv=(64, 6, 128), n_split=768, Lpad=128)
    outs = []
    old = L.set_option("gemm_2stage_max_k", 0)
    try:
        for mk in (0, 4096):
            L.set_option("gemm_2stage_max_k", mk)
            outs.append(fn())
    finally:
        L.set_option("gemm_2stage_max_k", old)
    a, b = outs
    assert all(torch.equal(x, y) for x, y in zip(a, b)) if isinstance(a, tuple) else torch.equal(a, b)



@pytest.mark.parametrize("tile256", [0, 1])
def test_lds_dma_kernels_wide_epilogues_vs_fp64(tile256):
    """Round 6: the bf16 epilogues of gemm_glds3_kernel / gemm_glds4_kernel store 16 bytes per lane (two 16-column blocks exchanged
    across lane rows with v_permlane16_swap) and evaluate the gated-GELU through one exponential.  Against fp64 references at shapes
    that take those kernels (M = 4099 ragged rows): STORE, BIAS_GELU, GEGLU, KV_SCATTER, QKV_VT (q | k block wide, V^T scatter
    narrow), and a STORE whose N is not a multiple of 16 (the 8-byte fallback inside the same kernel) -- every element within one
    bf16 rounding of the exact value."""
    L, _ = _lib()
    g = torch.Generator().manual_seed(77 + tile256)
    B_, H_, L_ = 3, 12, 1367            # M = 4101 rows: ragged last tile
    M, K = B_ * L_, 768
    A = _bf16r(torch.randn(M, K, generator=g) * 0.5)
    w = lambda n: _bf16r(torch.randn(n, K, generator=g) * 0.05)

    def close(out, exp, what):
        err = (out.double() - exp.double()).abs()
        tol = exp.double().abs() * 2.0 ** -8 + 2e-3          # one bf16 rounding of the value (+ the fp32 accumulation noise of K = 768)
        assert bool((err <= tol).all()), (what, float(err.max()), int((err > tol).sum()))

    old = L.set_option("gemm_tile256sq_min", tile256)
    try:
        W = w(2304)
        bias = torch.randn(2304, generator=g) * 0.1
        full = A.double() @ W.double().t()
        close(run_gemm(A, W, L.EPI_STORE, L.MH_BF16, bias=bias), full + bias.double(), "STORE")
        close(run_gemm(A, W, L.EPI_BIAS_GELU, L.MH_BF16, bias=bias), gelu_tanh((full + bias.double()).float()), "BIAS_GELU")
        Wn = W[:2296]                      # N % 16 == 8: the narrow stores of the same kernel
        close(run_gemm(A, Wn, L.EPI_STORE, L.MH_BF16), full[:, :2296], "STORE narrow")
        dff = 2048
        wi0, wi1 = w(dff), w(dff)
        Wi = torch.stack([wi0.reshape(dff // 16, 16, K), wi1.reshape(dff // 16, 16, K)], 1).reshape(2 * dff, K)
        exp = gelu_tanh((A.double() @ wi0.double().t()).float()).double() * (A.double() @ wi1.double().t())
        close(run_gemm(A, Wi, L.EPI_GEGLU, L.MH_BF16), exp, "GEGLU")
        Wkv = w(2 * 2 * H_ * 64)
        out = run_gemm(A, Wkv, L.EPI_KV_SCATTER, L.MH_BF16, kv=(B_, H_, L_))
        exp = (A.double() @ Wkv.double().t()).view(B_, L_, 4, H_, 64).permute(2, 0, 3, 1, 4)
        close(out, exp, "KV_SCATTER")
        Wq = w(3 * H_ * 64)
        qk, vt = run_gemm(A, Wq, L.EPI_QKV_VT, L.MH_BF16, kv=(B_, H_, L_), n_split=2 * H_ * 64, Lpad=1408)
        fq = A.double() @ Wq.double().t()
        close(qk, fq[:, :2 * H_ * 64], "QKV_VT q|k")
        close(vt[..., :L_], fq[:, 2 * H_ * 64:].view(B_, L_, H_, 64).permute(0, 2, 3, 1), "QKV_VT v^T")
    finally:
        L.set_option("gemm_tile256sq_min", old)
