"""Host side of the GEMM kernel tests (tests/test_gemm_cpu.py, tests/test_gpu_gemm.py): no GPU, no library call.

For one launch of mh_gemm -- a Run (family, dtype, shape, leading dimensions) and one epilogue -- `evaluate` returns every output buffer
in its documented PHYSICAL layout (guard rows, pad columns, V^T pads and unused cache positions included, holding SENTINEL), together
with the mask of the positions the launch writes:

  reference   fp64 from the operands as stored (bf16 cases round A and W to bf16 first; w_split3 operands are hi + lo);
  emulated    the same function in the kernels' DECLARED arithmetic: exact products of the stored operands summed in fp32 (for w_split3
              the three products hi.hi + hi.lo + lo.hi), the epilogue in fp32, returned before the output cast.  Its distance from the
              reference is the error floor of the launch: it comes from the reference alone, never from a device result;
  mutants     the same launch with ONE fault (a dropped K tail, a stale stage, a shifted bias, `/` for `%`, a wrong stride ...), in fp64.

Two terms of the kernels are not exact fp32 evaluations of the epilogue.  `gelu_erf_fast` (bf16 LDS-DMA kernels, BIAS_GELU_ERF) carries the
declared 1.5e-7 of the Abramowitz-Stegun erf, which `emulated` adds.  `gelu_tanh_fast` (the same kernels and gemm_s3g_kernel, BIAS_GELU and
GEGLU) is ~1e-6 RELATIVE through raw v_exp_f32 / v_rcp_f32: not a term of `emulated`, because relative to the value it is 500 x below the
rounding of a bf16 output and 8 x below the 2^-17 of the pre-split one, both of which the tolerance carries as u_out |reference|.

Tolerance, per element: tol = 4 * (floor + u_out * |reference|), floor = max |emulated - reference| over the buffer, u_out the unit
roundoff of the output type (2^-9 bf16, 2^-24 fp32, 2^-17 for the hi + lo pre-split output).  tests/test_gemm_cpu.py proves that every
mutant of every run is at least 10 tol away in at least 4 elements; tests/test_gpu_gemm.py asserts the device output within tol.

Inputs are seeded and LOUD at the edges (x8 on the last 16-byte K group, the last K step, the first and last row and column), the
storage padding of A and W holds 1e4, and a share of the GELU pre-activations sits in [-3.9, -3.1] where the tanh and erf forms differ
by more than 10 %."""
from __future__ import annotations

import math
import zlib
from dataclasses import dataclass
from functools import lru_cache
from typing import Dict, Optional, Tuple

import torch

from .attention import split3_unpack  # noqa: F401  (the pre-split output form: re-exported for the tests)

BF16, F32 = "bf16", "f32"
# MhGemm.epilogue (include/mapperhip.h)
(STORE, STORE_F32, RESID, GEGLU, BIAS_GELU, GATE_RESID, KV_SCATTER, QKV_VT, QKV_CACHE, BIAS_GELU_ERF) = range(10)
EPI_NAMES = ("STORE", "STORE_F32", "RESID", "GEGLU", "BIAS_GELU", "GATE_RESID", "KV_SCATTER", "QKV_VT", "QKV_CACHE", "BIAS_GELU_ERF")
ALL_EPIS = tuple(range(10))
S3_EPIS = (STORE_F32, QKV_VT, GATE_RESID, BIAS_GELU)          # Bf16x3Epis of csrc/gemm.hip
# MhGemmKernel families (include/mapperhip.h): mh_gemm_last_kernel() = family * 1024 + tile rows
(FAM_NONE, FAM_TN, FAM_TN_S3, FAM_TN_GLDS, FAM_GLDS3, FAM_GLDS2S, FAM_GLDS4, FAM_S3G, FAM_MX8, FAM_MX8_MXO) = range(10)
FAM_NAMES = ("none", "TN", "TN_S3", "TN_GLDS", "GLDS3", "GLDS2S", "GLDS4", "S3G", "MX8", "MX8_MXO")


def kernel_id(family, bm):
    return family * 1024 + bm


def kernel_name(kid):
    return "%s<%d rows>" % (FAM_NAMES[kid // 1024] if 0 <= kid // 1024 < len(FAM_NAMES) else "?", kid % 1024)


GUARD_ROWS = 4
SENTINEL = -768.0          # exact in bf16 and fp32
PAD_VALUE = 1.0e4          # storage padding of A and W: a read past K shows
ERF_AS_ERROR = 1.5e-7      # declared |error| of the Abramowitz-Stegun erf of gelu_erf_fast (csrc/common.hpp)
U_OUT = {"bf16": 2.0 ** -9, "f32": 2.0 ** -24, "split": 2.0 ** -17}
FAST_ERF_FAMILIES = (FAM_GLDS3, FAM_GLDS2S, FAM_GLDS4)       # g3_epilogue: gelu_erf_fast; gemm_tn_kernel keeps erff


def _bf16r(x):
    return x.to(torch.bfloat16).to(x.dtype)


def _ceil(a, b):
    return -(-a // b) * b


# ---- runs -------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Run:
    family: int
    bm: int                      # tile rows the dispatcher must choose
    dtype: str
    M: int
    N: int
    K: int
    options: Tuple[Tuple[str, int], ...]
    epis: Tuple[int, ...]
    split3: int = 0              # MhGemm.w_split3 (BIAS_GELU of the A-pre-split form adds | 4)
    var: str = "pad"             # "pad": ldc = N + 8; "ldc4": ldc = N + 4; "off8" / "off1": C starts 8 bytes / one element into its buffer
    note: str = ""

    @property
    def kernel(self):
        return kernel_id(self.family, self.bm)

    @property
    def id(self):
        return "%s%d-%s-%dx%dx%d-%s%s" % (FAM_NAMES[self.family], self.bm, self.dtype, self.M, self.N, self.K, self.var, self.note)

    @property
    def es(self):
        return 2 if self.dtype == BF16 else 4

    @property
    def step(self):
        """K step of the kernel in elements (RowBytes of csrc/gemm.hip; one 32-value block for the bf16 x 3 forms)"""
        rb = 1024 if self.bm == 16 else 512 if self.bm == 32 else 128
        return rb // self.es

    @property
    def lda(self):
        return self.K + (32 if self.split3 & 2 else 16 // self.es)         # + 16 bytes (w_split3 & 2: lda % 32 == 0)

    @property
    def ldw(self):
        return self.K + (32 if self.split3 else 32 // self.es)             # + 32 bytes (w_split3: ldw % 32 == 0)

    def c_offset_bytes(self, element_bytes):
        """where C starts in its allocation (a 16-byte aligned one): 8 bytes in, or at the weakest alignment of its element type"""
        return 8 if self.var == "off8" else element_bytes if self.var == "off1" else 0


@dataclass(frozen=True)
class Geo:
    """the problem one epilogue of a run is given: its own M / N where the epilogue's geometry asks for it"""
    M: int
    N: int
    ldc: int
    n_out: int                   # columns of C written per row
    rpb: int = 0
    gate_rows: int = 0
    gate_ld: int = 0
    B: int = 0
    H: int = 0
    L: int = 0
    Lpad: int = 0
    LK: int = 0                  # (layer, kv) count of KV_SCATTER
    n_split: int = 0
    cache_len: int = 0
    split_out: bool = False      # C is written pre-split (w_split3 & 4)


def geometry(r: Run, epi: int) -> Geo:
    M, N = r.M, r.N
    extra = 4 if r.var == "ldc4" else 8
    if epi in (KV_SCATTER, QKV_VT, QKV_CACHE):
        L = (M + 1) // 2                      # two batch entries; kv_L is no tile multiple
        M = 2 * L
        Lpad = _ceil(L, 64) + (64 if L % 64 == 0 else 0)
        if epi == KV_SCATTER:
            N = max(_ceil(N, 128), 256)       # H = 2 heads, N / 128 >= 2 (layer, kv) blocks
            return Geo(M, N, 0, N, B=2, H=2, L=L, LK=N // 128)
        if epi == QKV_VT:
            N = _ceil(max(N, 160), 32)        # q | k columns, then H = 2 heads of v
            return Geo(M, N, N - 128 + extra, N - 128, B=2, H=2, L=L, Lpad=Lpad, n_split=N - 128)
        N = max(_ceil(N, 192), 384)           # q | k | v of H = N / 192 >= 2 heads
        H = N // 192
        return Geo(M, N, H * 64 + extra, H * 64, B=2, H=H, L=L, Lpad=Lpad, n_split=H * 64, cache_len=L + 5)
    if epi == GEGLU:
        N = _ceil(N, 32)
        return Geo(M, N, N // 2 + extra, N // 2)
    rpb = 7 if M < 74 else 37 if M < 600 else 111
    gate_rows = max((M - 1) // (rpb - 1) + 1, rpb + 2)
    if epi == BIAS_GELU and (r.split3 & 2):
        return Geo(M, N, _ceil(N, 32) + 32, N, split_out=True)
    if epi in (GATE_RESID, BIAS_GELU_ERF):
        return Geo(M, N, N + extra, N, rpb=rpb, gate_rows=gate_rows, gate_ld=N + 4)
    return Geo(M, N, N + extra, N)


def out_kind(r: Run, epi: int, g: Geo) -> str:
    if g.split_out:
        return "split"
    if epi in (STORE_F32, RESID, GATE_RESID) or r.dtype == F32:
        return "f32"
    return "bf16"


def launch_split3(r: Run, epi: int) -> int:
    return r.split3 | (4 if (r.split3 & 2) and epi == BIAS_GELU else 0)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def _extent(r: Run):
    gs = [geometry(r, e) for e in r.epis]
    return max(g.M for g in gs), max(g.N for g in gs), gs


def steered(n_cols):
    """columns whose GELU pre-activation is steered into [-3.9, -3.1]"""
    c = torch.arange(n_cols)
    return (c % 5 == 2) & (c > 0)


def make_inputs(r: Run):
    Mx, Nx, gs = _extent(r)
    K = r.K
    g = torch.Generator().manual_seed(zlib.crc32(r.id.encode()))
    A = torch.randn(Mx, K, generator=g, dtype=torch.float64)
    W = torch.randn(Nx, K, generator=g, dtype=torch.float64) * torch.linspace(0.6, 1.4, Nx, dtype=torch.float64)[:, None]
    vec = 16 // r.es
    loud_k = torch.zeros(K, dtype=torch.bool)
    loud_k[K - vec:] = True                                  # the last 16-byte group
    nk = -(-K // r.step)
    if nk >= 2:
        loud_k[(nk - 1) * r.step:] = True                    # the last K step
    A[:, loud_k] *= 8
    W[:, loud_k] *= 8
    rows = {0} | {q.M - 1 for q in gs}
    cols = {0} | {q.N - 1 for q in gs}
    A[sorted(rows)] *= 8
    W[sorted(cols)] *= 8
    st = steered(Nx)
    st[sorted(cols)] = False                                 # (the loud last columns stay loud)
    W[st] /= 64                                              # small products on the steered columns
    # one scale for both operands so that the largest |product| is 4 (0.5 for the bf16 x 3 forms, whose products carry 2^-17): the
    # summation error (the floor) stays near 1e-6, below a tenth of what separates the two GELU forms on the steered columns
    s = math.sqrt((0.5 if r.split3 else 4.0) / float((A @ W.t()).abs().max()))
    A, W = (A * s).float(), (W * s).float()
    if r.dtype == BF16:
        A, W = _bf16r(A), _bf16r(W)
    X = {"A": A, "W": W, "steered": st}
    if r.split3:
        X["W_hi"] = W.to(torch.bfloat16).float()
        X["W_lo"] = (W - X["W_hi"]).to(torch.bfloat16).float()
        X["A_hi"] = A.to(torch.bfloat16).float()
        X["A_lo"] = (A - X["A_hi"]).to(torch.bfloat16).float()
    bias = 0.25 * torch.randn(Nx, generator=g) + 0.05 * torch.arange(Nx).remainder(7).float()
    bias[st] = -3.5 + 0.8 * (torch.rand(int(st.sum()), generator=g) - 0.5)
    X["bias"] = bias
    X["bias_plain"] = 0.25 * torch.randn(Nx, generator=g) + 0.05 * torch.arange(Nx).remainder(7).float()   # epilogues without a GELU
    gr = max(q.gate_rows for q in gs)
    gl = max(q.gate_ld for q in gs)
    if gr:
        X["gate"] = 0.3 * torch.randn(gr, gl, generator=g)                # differs in every row and column, pad columns too
        small = torch.zeros(gl, dtype=torch.bool)
        small[:min(gl, Nx)] = st[:gl]
        X["gate"][:, small] *= 1e-3                                       # (steered columns: the position row must not hide the GELU form in bf16)
    X["old"] = torch.randn(Mx, Nx, generator=g)
    return X


def stored(r: Run, X, dt):
    """(A, W) as the kernel reads them, in `dt`: w_split3 operands are hi + lo of their stored halves"""
    A = (X["A_hi"].to(dt) + X["A_lo"].to(dt)) if r.split3 & 2 else X["A"].to(dt)
    W = (X["W_hi"].to(dt) + X["W_lo"].to(dt)) if r.split3 else X["W"].to(dt)
    return A, W


def padded(x, ld):
    out = torch.full((x.shape[0], ld), PAD_VALUE, dtype=x.dtype)
    out[:, :x.shape[1]] = x
    return out


def split3_pack(hi, lo, ld):
    """[n, K] halves -> the w_split3 layout with storage padding: [n, 2 * ld] bf16 (every 32 values as [32 hi | 32 lo])"""
    n, k = hi.shape
    ph, pl = padded(hi, ld), padded(lo, ld)
    return torch.stack([ph.reshape(n, ld // 32, 32), pl.reshape(n, ld // 32, 32)], 2).reshape(n, 2 * ld).to(torch.bfloat16)


# ---- products ---------------------------------------------------------------------------------------------------------------------
def product_ref(r: Run, X):
    A, W = stored(r, X, torch.float64)
    return A @ W.t()


def product_emulated(r: Run, X):
    """exact products of the stored operands, summed in fp32"""
    if r.split3:
        ah, al = X["A_hi"], X["A_lo"]
        return (al @ X["W_hi"].t() + ah @ X["W_lo"].t()) + ah @ X["W_hi"].t()       # small terms first; lo.lo is dropped
    return X["A"] @ X["W"].t()


PRODUCT_MUTANTS = ("k_group_dropped", "k_step_dropped", "stale_stage", "lda_is_K", "ldw_is_K")


def product_mutants(r: Run, X, P):
    A, W = stored(r, X, torch.float64)
    K, vec, step = r.K, 16 // r.es, r.step
    nk = -(-K // step)
    out = {}
    t = slice(K - vec, K)
    out["k_group_dropped"] = P - A[:, t] @ W[:, t].t()
    t = slice((nk - 1) * step, K)
    out["k_step_dropped"] = P - A[:, t] @ W[:, t].t()
    if nk >= 2:
        s1 = slice(step, min(2 * step, K))
        n1 = s1.stop - s1.start
        out["stale_stage"] = P + (A[:, :n1] - A[:, s1]) @ W[:, s1].t()
    Ap = padded(A, r.lda).reshape(-1)[:A.shape[0] * K].reshape(A.shape[0], K)
    out["lda_is_K"] = Ap @ W.t()
    Wp = padded(W, r.ldw).reshape(-1)[:W.shape[0] * K].reshape(W.shape[0], K)
    out["ldw_is_K"] = A @ Wp.t()
    return out


# ---- epilogues --------------------------------------------------------------------------------------------------------------------
def _gelu_tanh(x):
    return 0.5 * x * (1.0 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x * x * x)))


def _gelu_erf(x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.70710678118654752))


def _swap_cols(v, mut):
    """the wide-store faults on the columns of v"""
    if mut == "wide_blocks_exchanged":
        n = v.shape[1] // 32 * 32
        if n:
            v = torch.cat([v[:, :n].reshape(v.shape[0], -1, 2, 16).flip(2).reshape(v.shape[0], n), v[:, n:]], 1)
    elif mut == "wide_halves_exchanged":
        n = v.shape[1] // 16 * 16
        if n:
            v = torch.cat([v[:, :n].reshape(v.shape[0], -1, 2, 8).flip(2).reshape(v.shape[0], n), v[:, n:]], 1)
    return v


def _rows_buffer(v, M, ldc):
    """C as [M + GUARD_ROWS, ldc]: the values in the M x n window, SENTINEL everywhere else"""
    buf = torch.full((M + GUARD_ROWS, ldc), SENTINEL, dtype=torch.float64)
    wr = torch.zeros((M + GUARD_ROWS, ldc), dtype=torch.bool)
    buf[:M, :v.shape[1]] = v.double()
    wr[:M, :v.shape[1]] = True
    return buf, wr


def buffer_sizes(r: Run, epi: int):
    """name -> (rows, cols) of every output buffer of the launch, guards included (cols = the row stride)"""
    g = geometry(r, epi)
    if epi == KV_SCATTER:
        return {"C": (g.LK * g.B * g.H * g.L + GUARD_ROWS, 64)}
    out = {"C": (g.M + GUARD_ROWS, g.ldc)}
    if epi in (QKV_VT, QKV_CACHE):
        out["C4" if epi == QKV_CACHE else "C2"] = (g.B * g.H * 64 + GUARD_ROWS, g.Lpad)
    if epi == QKV_CACHE:
        out["C2"] = out["C3"] = (g.B * g.H * g.cache_len + GUARD_ROWS, 64)
    return out


def initial_c(r: Run, epi: int, X):
    """what C holds before the launch: the old C in the M x N window for RESID / GATE_RESID, SENTINEL elsewhere"""
    g = geometry(r, epi)
    rows, cols = buffer_sizes(r, epi)["C"]
    buf = torch.full((rows, cols), SENTINEL, dtype=torch.float32)
    if epi in (RESID, GATE_RESID):
        buf[:g.M, :g.N] = X["old"][:g.M, :g.N]
    return buf


def has_gate(epi, with_pos=True):
    return epi == GATE_RESID or (epi == BIAS_GELU_ERF and with_pos)


def evaluate(r: Run, epi: int, X, P, mut: Optional[str] = None, emulate: bool = False, with_pos: bool = True):
    """every output buffer of the launch -> {name: (values fp64 [rows, cols], written mask)}; P = the product over the run's extent
    (fp64: reference / mutants; fp32 with emulate: the declared arithmetic)"""
    g = geometry(r, epi)
    dt = torch.float32 if emulate else torch.float64
    M, N = g.M, g.N
    v = P[:M, :N].to(dt).clone()
    if mut == "last_row_from_neighbour":
        v[M - 1] = v[M - 2]
    if mut == "last_col_from_neighbour":
        v[:, N - 1] = v[:, N - 2]
    gelu = epi in (BIAS_GELU, BIAS_GELU_ERF, GEGLU)
    if epi != GEGLU:
        b = (X["bias"] if gelu else X["bias_plain"])[:N].to(dt)
        if mut == "bias_shift1":
            b = torch.cat([b[1:], b[-1:]])
        elif mut == "bias_shift4":
            b = torch.cat([b[4:], b[-4:]])
        elif mut == "bias_clamped_last_group":
            b = torch.cat([b[:N - 4], b[N - 4:N - 3].expand(4)])
        if mut != "bias_dropped":
            v = v + b

    def gate_of(rpb_index):
        gt, ld = X["gate"][:, :g.gate_ld].to(dt), g.gate_ld
        if mut == "gate_ld_is_N":                      # the rows of the [gate_rows, gate_ld] storage read with stride N
            flat = X["gate"][:g.gate_rows, :g.gate_ld].contiguous().reshape(-1).to(dt)
            idx = (rpb_index[:, None] * N + torch.arange(N)[None]).clamp(max=flat.numel() - 1)
            return flat[idx]
        return gt[rpb_index.clamp(max=gt.shape[0] - 1), :N]

    rows = torch.arange(M)
    if has_gate(epi, with_pos):
        rpb = g.rpb + (1 if mut == "rpb_plus1" else -1 if mut == "rpb_minus1" else 0)
        by_div = (epi == GATE_RESID) != (mut == "div_mod_exchanged")
        gsel = gate_of(rows // rpb if by_div else rows % rpb)
    if epi in (STORE, STORE_F32):
        pass
    elif epi == RESID:
        v = v if mut == "old_c_dropped" else X["old"][:M, :N].to(dt) + v
    elif epi == GATE_RESID:
        gq = torch.ones_like(v) if mut == "gate_dropped" else gsel
        v = X["old"][:M, :N].to(dt) + gq * v
    elif epi in (BIAS_GELU, BIAS_GELU_ERF):
        erf = (epi == BIAS_GELU_ERF) != (mut == "tanh_erf_exchanged")
        x = v
        if mut != "gelu_dropped":
            v = _gelu_erf(x) if erf else _gelu_tanh(x)
            if emulate and erf and r.family in FAST_ERF_FAMILIES:
                v = v + 0.5 * x.abs() * ERF_AS_ERROR           # gelu_erf_fast: the declared error of the Abramowitz-Stegun erf
        if epi == BIAS_GELU_ERF and with_pos and mut != "gate_dropped":
            v = v + gsel
    elif epi == GEGLU:
        blk = v.reshape(M, N // 32, 2, 16)
        a, l = blk[:, :, 0], blk[:, :, 1]
        if mut == "geglu_blocks_paired_02_13":
            n4 = N // 64 * 64
            q = v[:, :n4].reshape(M, -1, 4, 16)
            a = torch.cat([torch.stack([q[:, :, 0], q[:, :, 1]], 2).reshape(M, -1, 16), a[:, n4 // 32:]], 1)
            l = torch.cat([torch.stack([q[:, :, 2], q[:, :, 3]], 2).reshape(M, -1, 16), l[:, n4 // 32:]], 1)
        if mut == "geglu_halves_exchanged":
            a, l = l, a
        v = (_gelu_tanh(a * l) if mut == "geglu_gelu_on_product" else _gelu_tanh(a) * l).reshape(M, N // 2)
    if mut in ("wide_blocks_exchanged", "wide_halves_exchanged"):
        if epi == QKV_VT:
            v = torch.cat([_swap_cols(v[:, :g.n_split], mut), v[:, g.n_split:]], 1)
        elif epi != QKV_CACHE:
            v = _swap_cols(v, mut)
    if epi not in (KV_SCATTER, QKV_VT, QKV_CACHE):
        out = {"C": _rows_buffer(v, M, g.ldc)}
        if g.split_out:
            # the hi half on its own (the sum hi + lo does not see the two halves exchanged): bf16(value), judged as a bf16 output
            hi = v.double() - _bf16r(v.double()) if mut == "split_hi_lo_exchanged" else v
            out["C_hi"] = _rows_buffer(hi, M, g.ldc)
        return out

    plan = _scatter_plan(r, epi, mut if mut in LAYOUT_MUTANTS else None)
    flat = v.reshape(-1).double()
    out = {}
    for name, (shape, dst, src, wr) in plan.items():
        buf = torch.full((shape[0] * shape[1],), SENTINEL, dtype=torch.float64)
        buf[dst] = flat[src]
        out[name] = (buf.reshape(shape), wr)
    return out


LAYOUT_MUTANTS = ("kvL_plus1", "kvL_minus1", "h_lk_exchanged", "n_split_plus32", "n_split_minus32", "vt_stride_is_kvL", "vt_b_h_exchanged",
                  "k_v_exchanged", "cache_len_is_kvL", "c4_write_missing")


@lru_cache(maxsize=16)
def _scatter_plan(r: Run, epi: int, mut: Optional[str]):
    """destination of element (row, col) in every buffer of a scatter epilogue -> {name: (shape, flat destinations, flat sources, written)};
    destinations outside the buffer are dropped"""
    g = geometry(r, epi)
    M, N = g.M, g.N
    sizes = buffer_sizes(r, epi)
    row = torch.arange(M)[:, None].expand(M, N)
    col = torch.arange(N)[None, :].expand(M, N)
    Ldiv = g.L + (1 if mut == "kvL_plus1" else -1 if mut == "kvL_minus1" else 0)
    b = row // Ldiv
    key = row - b * Ldiv
    src_all = torch.arange(M * N)
    plan = {}

    def put(name, dst, ok=None):
        shape = sizes[name]
        size = shape[0] * shape[1]
        dst = dst.reshape(-1)
        keep = (dst >= 0) & (dst < size)
        if ok is not None:
            keep = keep & ok.reshape(-1)
        wr = torch.zeros(size, dtype=torch.bool)
        wr[dst[keep]] = True
        plan[name] = (shape, dst[keep], src_all[keep], wr.reshape(shape))

    if epi == KV_SCATTER:
        c6, dd = col >> 6, col & 63
        if mut == "h_lk_exchanged":
            lk, h = c6 % g.LK, c6 // g.LK
        else:
            h, lk = c6 % g.H, c6 // g.H
        put("C", (((lk * g.B + b) * g.H + h) * g.L + key) * 64 + dd)
        return plan
    ns = g.n_split + (32 if mut == "n_split_plus32" else -32 if mut == "n_split_minus32" else 0)
    left = col < ns
    put("C", row * g.ldc + col, left & (col < g.ldc))
    c2 = col - ns
    stride = g.L if mut == "vt_stride_is_kvL" else g.Lpad

    def vt_dst(c):
        if mut == "vt_b_h_exchanged":
            return (((c >> 6) * g.B + b) * 64 + (c & 63)) * stride + key
        return (b * g.H * 64 + c) * stride + key

    if epi == QKV_VT:
        put("C2", vt_dst(c2), ~left)
        return plan
    inner = g.H * 64
    kv = c2 // inner
    c = c2 - kv * inner
    clen = g.L if mut == "cache_len_is_kvL" else g.cache_len
    dst = ((b * g.H + (c >> 6)) * clen + key) * 64 + (c & 63)
    is_k, is_v = ~left & (kv == 0), ~left & (kv == 1)
    if mut == "k_v_exchanged":
        is_k, is_v = is_v, is_k
    put("C2", dst, is_k)
    put("C3", dst, is_v)
    put("C4", vt_dst(c), is_v & (mut != "c4_write_missing"))
    return plan


def epilogue_mutants(r: Run, epi: int, with_pos: bool = True):
    """names of the faults of the epilogue itself that apply to this launch"""
    g = geometry(r, epi)
    m = ["last_row_from_neighbour", "last_col_from_neighbour"]
    if epi != GEGLU:
        m += ["bias_dropped", "bias_shift1", "bias_shift4", "bias_clamped_last_group"]
    if has_gate(epi, with_pos):
        m += ["div_mod_exchanged", "rpb_plus1", "rpb_minus1", "gate_ld_is_N", "gate_dropped"]
    if epi == RESID:
        m += ["old_c_dropped"]
    if epi in (BIAS_GELU, BIAS_GELU_ERF):
        m += ["tanh_erf_exchanged", "gelu_dropped"]
    if epi == GEGLU:
        m += ["geglu_halves_exchanged", "geglu_gelu_on_product"] + (["geglu_blocks_paired_02_13"] if g.N >= 64 else [])
    if g.split_out:         # the wide pre-split store of gemm_s3g_kernel: 32-column groups, hi and lo halves 64 bytes apart
        m += ["split_hi_lo_exchanged"] + (["wide_halves_exchanged", "wide_blocks_exchanged"] if g.n_out % 32 == 0 else [])
    if r.dtype == BF16 and epi in (STORE, BIAS_GELU, BIAS_GELU_ERF, GEGLU, KV_SCATTER, QKV_VT) and g.n_out % 16 == 0:
        m += ["wide_halves_exchanged"] + (["wide_blocks_exchanged"] if g.n_out >= 32 else [])
    if epi == KV_SCATTER:
        m += ["h_lk_exchanged", "kvL_plus1", "kvL_minus1"]
    if epi in (QKV_VT, QKV_CACHE):
        m += ["n_split_plus32", "n_split_minus32", "vt_stride_is_kvL", "vt_b_h_exchanged"]
    if epi == QKV_CACHE:
        m += ["k_v_exchanged", "cache_len_is_kvL", "c4_write_missing"]
    return m


# the mutants every launch of an epilogue must have (tests/test_gemm_cpu.py checks the condition)
REQUIRED_MUTANTS = {e: {"k_group_dropped", "k_step_dropped", "last_row_from_neighbour", "last_col_from_neighbour", "lda_is_K", "ldw_is_K"}
                    for e in ALL_EPIS}
for _e in ALL_EPIS:
    if _e != GEGLU:
        REQUIRED_MUTANTS[_e] |= {"bias_dropped", "bias_shift1", "bias_shift4", "bias_clamped_last_group"}
for _e in (GATE_RESID, BIAS_GELU_ERF):
    REQUIRED_MUTANTS[_e] |= {"div_mod_exchanged", "rpb_plus1", "rpb_minus1", "gate_ld_is_N", "gate_dropped"}
REQUIRED_MUTANTS[RESID] |= {"old_c_dropped"}
for _e in (BIAS_GELU, BIAS_GELU_ERF):
    REQUIRED_MUTANTS[_e] |= {"tanh_erf_exchanged", "gelu_dropped"}
REQUIRED_MUTANTS[GEGLU] |= {"geglu_halves_exchanged", "geglu_blocks_paired_02_13", "geglu_gelu_on_product"}
REQUIRED_MUTANTS[KV_SCATTER] |= {"h_lk_exchanged", "kvL_plus1", "kvL_minus1"}
for _e in (QKV_VT, QKV_CACHE):
    REQUIRED_MUTANTS[_e] |= {"n_split_plus32", "n_split_minus32", "vt_stride_is_kvL", "vt_b_h_exchanged"}
REQUIRED_MUTANTS[QKV_CACHE] |= {"k_v_exchanged", "cache_len_is_kvL", "c4_write_missing"}


# ---- one run, prepared ------------------------------------------------------------------------------------------------------------
class Prepared:
    """inputs, products and product-level mutants of a run (computed once, shared by its epilogues and left unchanged)"""

    def __init__(self, r: Run):
        self.run = r
        self.X = make_inputs(r)
        self.P = product_ref(r, self.X)
        self.P32 = product_emulated(r, self.X)
        self.Pm = product_mutants(r, self.X, self.P)

    def launch(self, epi, with_pos=True):
        """-> dict(ref, wr, floor, tol, kind) per buffer name, and mutants(): name -> {buffer: values}"""
        r, X = self.run, self.X
        ref = evaluate(r, epi, X, self.P, with_pos=with_pos)
        emu = evaluate(r, epi, X, self.P32, emulate=True, with_pos=with_pos)
        out = {}
        for name, (val, wr) in ref.items():
            kind = "bf16" if name == "C_hi" else out_kind(r, epi, geometry(r, epi))
            floor = float((emu[name][0] - val)[wr].abs().max())
            out[name] = dict(ref=val, wr=wr, floor=floor, kind=kind, tol=tolerance(val, floor, kind))
        return out

    def mutants(self, epi, with_pos=True):
        r, X = self.run, self.X
        for name, Pm in self.Pm.items():
            yield name, {k: v[0] for k, v in evaluate(r, epi, X, Pm, with_pos=with_pos).items()}
        for name in epilogue_mutants(r, epi, with_pos):
            yield name, {k: v[0] for k, v in evaluate(r, epi, X, self.P, mut=name, with_pos=with_pos).items()}


def tolerance(reference, floor, kind):
    return 4.0 * (floor + U_OUT[kind] * reference.abs())


def passes(got: Dict[str, torch.Tensor], want: Dict[str, torch.Tensor], spec, factor=1.0):
    """THE error assertion: in every buffer, at every position the launch writes, |got - want| < factor * 4 (floor + u_out |want|)"""
    for name, s in spec.items():
        wr = s["wr"]
        err = (got[name] - want[name]).abs()[wr]
        if not bool((err < factor * tolerance(want[name], s["floor"], s["kind"])[wr]).all()):
            return False
    return True


def elements_off(mref, spec, by=10.0):
    """the largest count, over the buffers, of elements where a mutant is at least `by` tolerances away from the reference"""
    n = 0
    for name, s in spec.items():
        d = (mref[name] - s["ref"]).abs()
        n = max(n, int((d >= by * s["tol"]).sum()))
    return n


@lru_cache(maxsize=2)
def prepared(r: Run) -> Prepared:
    return Prepared(r)


# ---- the GPU table ----------------------------------------------------------------------------------------------------------------
HUGE = 1 << 30


def _k(nbytes, dtype):
    return nbytes // (2 if dtype == BF16 else 4)


def gpu_runs():
    """(family, dtype, shape, options, kernel that must be reported): the smallest shapes that reach each member of tile_kernels<T, EPI>
    under dispatch_tile() (csrc/gemm.hip).  Per family: every shape with padded leading dimensions (lda = K + 16 bytes, ldw = K + 32
    bytes, gate_ld = N + 4, ldc = N + 8), and its first shape again with ldc = N + 4, with C offset by 8 bytes and with C offset by one
    element (2 bytes bf16, 4 bytes fp32 and pre-split): the last three must take the narrow stores and still be right."""
    runs = []
    no_geglu = tuple(e for e in ALL_EPIS if e != GEGLU)

    def family(fam, bm, dtype, shapes, options, epis, split3=0):
        for i, (M, N, K) in enumerate(shapes):
            for var in (("pad", "ldc4", "off8", "off1") if i == 0 else ("pad",)):
                runs.append(Run(fam, bm, dtype, M, N, K, tuple(sorted(options.items())), epis, split3, var))

    for dt in (BF16, F32):
        # 16 x 16 split-K tile: fewer than 192 64 x 64 tiles and fewer than gemm_splitk_tiles 32 x 32 tiles.  K step = 1024 bytes
        family(FAM_TN, 16, dt, [(19, 20, _k(16, dt)), (37, 52, _k(1024 + 16, dt)), (50, 36, _k(2048 + 16, dt))],
               {"gemm_tile128_min": 192, "gemm_splitk_tiles": 192}, no_geglu)
        # 32 x 32 tile (K step 512 bytes)
        family(FAM_TN, 32, dt, [(37, 52, _k(512 + 16, dt)), (70, 44, _k(16, dt))], {"gemm_tile128_min": 192, "gemm_splitk_tiles": 0}, no_geglu)
        # 64 x 64 tile: >= 192 of them (14 x 15), or GEGLU at any size
        family(FAM_TN, 64, dt, [(837, 900, _k(144, dt))], {"gemm_tile128_min": HUGE}, ALL_EPIS)
        family(FAM_TN, 64, dt, [(70, 96, _k(144, dt))], {"gemm_tile128_min": HUGE}, (GEGLU,))
    # 128 x 128 register-staged tile (fp32: 8 x gemm_tile128_min tiles)
    family(FAM_TN, 128, BF16, [(130, 140, 72)], {"gemm_tile128_min": 1, "gemm_glds": 0}, ALL_EPIS)
    family(FAM_TN, 128, F32, [(300, 260, 36)], {"gemm_tile128_min": 1, "gemm_glds": 0}, ALL_EPIS)
    # ... its LDS-DMA form; also where the three-stage kernels fall back to (K % 64 != 0)
    family(FAM_TN_GLDS, 128, BF16, [(130, 140, 72), (130, 140, 96), (130, 140, 128)], {"gemm_tile128_min": 1, "gemm_glds": 1}, ALL_EPIS)
    runs.append(Run(FAM_TN_GLDS, 128, BF16, 130, 140, 72, tuple(sorted({"gemm_tile128_min": 1, "gemm_glds": 3, "gemm_2stage_max_k": 512}.items())),
                    (STORE, BIAS_GELU_ERF), note="-fallback"))
    g3 = {"gemm_tile128_min": 1, "gemm_glds": 3, "gemm_tile256sq_min": 0}
    family(FAM_GLDS2S, 128, BF16, [(130, 132, 64), (300, 264, 192), (130, 144, 128)], dict(g3, gemm_2stage_max_k=512), ALL_EPIS)
    # 96 <= 256 x 128 tiles < 128 (2 x 48: the fewest elements that count 96 tiles with more than one tile row): the 128-row form with
    # gemm_glds = 3, the 256-row form with gemm_glds = 2
    s3 = [(260, 6024, 64), (260, 6024, 128), (260, 6024, 192), (260, 6024, 320), (260, 6032, 128)]
    family(FAM_GLDS3, 128, BF16, s3, dict(g3, gemm_2stage_max_k=0), ALL_EPIS)
    family(FAM_GLDS3, 256, BF16, s3, dict(g3, gemm_2stage_max_k=0, gemm_glds=2), ALL_EPIS)
    # >= 128 256 x 128 tiles (2 x 64)
    family(FAM_GLDS4, 256, BF16, [(260, 8072, 64), (260, 8072, 128), (260, 8072, 320), (260, 8080, 128)],
           dict(g3, gemm_2stage_max_k=0, gemm_tile256sq_min=1), ALL_EPIS)
    family(FAM_TN_S3, 64, F32, [(70, 68, 32), (333, 200, 416)], {}, S3_EPIS, split3=1)
    family(FAM_S3G, 128, F32, [(130, 132, 32), (300, 264, 96), (130, 16388, 64), (130, 160, 32)], {}, S3_EPIS, split3=3)
    return runs


GPU_RUNS = gpu_runs()


def built_kernels():
    """(dtype, kernel id, epilogue) of every member of tile_kernels<bf16_t, .> and tile_kernels<float, .>"""
    out = set()
    for dt in (BF16, F32):
        for e in ALL_EPIS:
            for bm in (128, 64) + ((32, 16) if e != GEGLU else ()):
                out.add((dt, kernel_id(FAM_TN, bm), e))
            if dt == BF16:
                out |= {(dt, kernel_id(FAM_TN_GLDS, 128), e), (dt, kernel_id(FAM_GLDS3, 256), e), (dt, kernel_id(FAM_GLDS3, 128), e),
                        (dt, kernel_id(FAM_GLDS4, 256), e), (dt, kernel_id(FAM_GLDS2S, 128), e)}
            elif e in S3_EPIS:
                out |= {(dt, kernel_id(FAM_TN_S3, 64), e), (dt, kernel_id(FAM_S3G, 128), e)}
    return out
