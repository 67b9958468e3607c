"""-m gpu: every member of tile_kernels<bf16_t, EPI> and tile_kernels<float, EPI> (csrc/gemm.hip), through every epilogue built for it,
against the fp64 reference of mh_testing/gemm.py.

One case per (kernel family, dtype, shape, leading-dimension form); the epilogues loop inside it.  Per launch: every output buffer
carries GUARD_ROWS extra rows and padded rows and starts as SENTINEL (the old C in the M x N window for RESID / GATE_RESID); after the
launch everything the launch does not write -- guard rows, columns >= N, V^T pad columns, cache positions >= kv_L, the bytes in front
of an offset C -- is bit-unchanged; mh_gemm_last_kernel() reports the kernel the table names; the output is finite and
|out - reference| < tol = 4 (floor + u_out |reference|) elementwise (floor: the distance of the kernels' DECLARED arithmetic from the
reference, computed on the host from the reference alone); and every single-fault mutant of the launch, evaluated in fp64 on the host,
fails that same assertion against the same device output (tests/test_gemm_cpu.py shows each is >= 10 tol away in >= 4 elements).

Measured on an MI355X over the 840 launches below: largest |out - reference| / tol per kernel (the test prints them as GEMM_MAX), for
the bf16 kernels first over the epilogues that write bf16, then over those that write fp32 (STORE_F32, RESID, GATE_RESID)
  gemm_tn_kernel 16 x 16 split-K     bf16 0.497 / 0.294    fp32 0.362
  gemm_tn_kernel 32 x 32             bf16 0.497 / 0.144    fp32 0.358
  gemm_tn_kernel 64 x 64             bf16 0.498 / 0.168    fp32 0.276
  gemm_tn_kernel 128 x 128           bf16 0.498 / 0.134    fp32 0.277
  ... its LDS-DMA form               bf16 0.498 / 0.193
  gemm_glds2s_kernel                 bf16 0.498 / 0.149
  gemm_glds3_kernel<EPI, 2>          bf16 0.498 / 0.172
  gemm_glds3_kernel<EPI, 4>          bf16 0.498 / 0.171
  gemm_glds4_kernel                  bf16 0.498 / 0.174
  gemm_tn_kernel bf16 x 3 (64 x 64)                        fp32 0.252
  gemm_s3g_kernel<EPI, 2>                                  fp32 0.255; pre-split BIAS_GELU 0.498 (the hi half judged as a bf16 value), wide
                                                           (N = 160, ldc = 192, C aligned) and narrow form alike
The bf16 outputs sit at half the bound: their error is the rounding to bf16, up to 2^-8 |value| just above a power of two against
u_out = 2^-9.  Floors are 2e-7 .. 9e-7 (bf16, fp32) and 2e-6 .. 4e-6 (bf16 x 3).  No term had to be added to `emulated` beyond the
declared error of the Abramowitz-Stegun erf, no kernel failed a case, every mutant failed against every device output, and C at an
8-byte and at a one-element offset is served by every kernel (the header's alignment statement)."""
import ctypes as C

import pytest
import torch

from mh_testing import gemm as G

pytestmark = pytest.mark.gpu

SEEN = {}                  # (dtype, kernel id, epilogue) -> largest |out - reference| / tol over the launches of this process
TD = {"bf16": torch.bfloat16, "f32": torch.float32, "split": torch.bfloat16}
_OPERANDS = {}             # the last run's operands on the device


def _lib():
    from mapperatorinator_amd import _lib
    return _lib, _lib.load()


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def operands(r: G.Run, X):
    """A and W of the run in their padded storage (the pad columns hold PAD_VALUE), on the device"""
    if _OPERANDS.get("run") != r:
        _OPERANDS.clear()
        td = torch.bfloat16 if r.dtype == G.BF16 else torch.float32
        if r.split3 & 2:
            A = G.split3_pack(X["A_hi"], X["A_lo"], r.lda)
        else:
            A = G.padded(X["A"], r.lda).to(td)
        W = G.split3_pack(X["W_hi"], X["W_lo"], r.ldw) if r.split3 else G.padded(X["W"], r.ldw).to(td)
        _OPERANDS.update(run=r, A=A.cuda(), W=W.cuda())
    return _OPERANDS["A"], _OPERANDS["W"]


def launch(r: G.Run, epi: int, with_pos: bool, X, spec):
    """one mh_gemm launch -> ({buffer: values fp64 [rows, cols]}, kernel id); asserts that nothing outside the written mask changed"""
    L, lib = _lib()
    g = G.geometry(r, epi)
    kind = G.out_kind(r, epi, g)
    A, W = operands(r, X)
    d = L.MhGemm()
    d.A, d.lda, d.W, d.ldw = A.data_ptr(), r.lda, W.data_ptr(), r.ldw
    d.M, d.N, d.K, d.ldc = g.M, g.N, r.K, g.ldc
    d.dtype, d.epilogue, d.w_split3 = (L.MH_BF16 if r.dtype == G.BF16 else L.MH_F32), epi, G.launch_split3(r, epi)
    keep = []
    if epi != G.GEGLU:
        b = X["bias"] if epi in (G.BIAS_GELU, G.BIAS_GELU_ERF) else X["bias_plain"]
        bias = torch.cat([b[:g.N], torch.full((8,), G.PAD_VALUE)]).cuda()          # a read past N shows
        keep.append(bias)
        d.bias = bias.data_ptr()
    if G.has_gate(epi, with_pos):
        gate = X["gate"][:g.gate_rows, :g.gate_ld].contiguous().cuda()
        keep.append(gate)
        d.gate, d.gate_ld, d.rows_per_batch = gate.data_ptr(), g.gate_ld, g.rpb
    d.kv_B, d.kv_H, d.kv_L, d.kv_Lpad, d.n_split, d.cache_len = g.B, g.H, g.L, g.Lpad, g.n_split, g.cache_len
    # output buffers: SENTINEL (the old C in its window), C possibly 8 bytes into its allocation
    sizes = G.buffer_sizes(r, epi)
    init, dev, off = {}, {}, {}
    for name, (rows, cols) in sizes.items():
        if name == "C":
            first = G.initial_c(r, epi, X)
            if kind == "split":
                first = torch.full((rows, 2 * cols), G.SENTINEL, dtype=torch.bfloat16)
            else:
                first = first.to(TD[kind])
            off[name] = r.c_offset_bytes(4 if kind == "split" else first.element_size()) // first.element_size()
        else:
            first = torch.full((rows, cols), G.SENTINEL, dtype=TD[kind])
            off[name] = 0
        flat = torch.cat([torch.full((off[name],), G.SENTINEL, dtype=first.dtype), first.reshape(-1)])
        init[name], dev[name] = flat, flat.cuda()
        setattr(d, name, dev[name].data_ptr() + off[name] * first.element_size())
    assert d.C % 16 == {"pad": 0, "ldc4": 0, "off8": 8, "off1": 2 if kind == "bf16" else 4}[r.var]
    L.check(lib.mh_gemm(C.byref(d), torch.cuda.current_stream().cuda_stream), "%s %s" % (r.id, G.EPI_NAMES[epi]))
    kid = lib.mh_gemm_last_kernel()
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:      # a device fault: nothing more is started on this GPU by this session
        pytest.exit(f"{r.id} {G.EPI_NAMES[epi]}: {e}", returncode=3)
    got = {}
    for name, (rows, cols) in sizes.items():
        raw, was = dev[name].cpu(), init[name]
        wr = spec[name]["wr"]
        if name == "C" and kind == "split":        # [32 x bf16 hi | 32 x bf16 lo] per 32 values: both halves of a written position
            wr_raw = wr.reshape(rows, cols // 32, 1, 32).expand(rows, cols // 32, 2, 32).reshape(-1)
        else:
            wr_raw = wr.reshape(-1)
        o = off[name]
        assert torch.equal(_bits(raw[:o]), _bits(was[:o])), f"{name}: the bytes in front of the offset buffer were written"
        same = _bits(raw[o:]) == _bits(was[o:])
        assert bool(same[~wr_raw].all()), f"{r.id} {G.EPI_NAMES[epi]}: {name} was written outside its documented positions " \
                                          f"(guard rows, pad columns, cache positions >= kv_L): {int((~same[~wr_raw]).sum())} elements"
        body = raw[o:]
        if name == "C" and kind == "split":
            got[name] = G.split3_unpack(body.reshape(rows, 2 * cols).view(torch.float32)).double()
            got["C_hi"] = body.reshape(rows, cols // 32, 2, 32)[:, :, 0].reshape(rows, cols).double()     # the hi halves alone
        else:
            got[name] = body.reshape(rows, cols).double()
    return got, kid


def check_launch(r: G.Run, epi: int, with_pos: bool = True):
    P = G.prepared(r)
    what = "%s %s%s" % (r.id, G.EPI_NAMES[epi], "" if with_pos else "-nogate")
    spec = P.launch(epi, with_pos)
    got, kid = launch(r, epi, with_pos, P.X, spec)
    assert kid == r.kernel, f"{what}: ran {G.kernel_name(kid)}, the table names {G.kernel_name(r.kernel)}"
    ref = {k: s["ref"] for k, s in spec.items()}
    err = ratio = 0.0
    for k, s in spec.items():
        e = (got[k] - s["ref"]).abs()[s["wr"]]
        err, ratio = max(err, float(e.max())), max(ratio, float((e / s["tol"][s["wr"]]).max()))
        assert torch.isfinite(got[k][s["wr"]]).all(), what
    print(f"GEMM_ERR {what} {G.kernel_name(kid)} err {err:.3e} err/tol {ratio:.3f} floor {max(s['floor'] for s in spec.values()):.3e}")
    key = (r.dtype, kid, epi)
    SEEN[key] = max(SEEN.get(key, 0.0), ratio)
    assert G.passes(got, ref, spec), f"{what}: max |out - reference| = {err:.3e} is {ratio:.2f} x tol = 4 (floor + u_out |reference|)"
    # the tolerance is not vacuous: a kernel computing one of the mutants would have failed the assertion above
    missed = [name for name, mref in P.mutants(epi, with_pos) if G.passes(got, mref, spec)]
    assert not missed, f"{what}: these mutants pass the error assertion against the device output: {missed}"


def check(r: G.Run, epis=None):
    L, _ = _lib()
    old = []
    try:
        for name, value in r.options:
            old.append((name, L.set_option(name, value)))
        for epi in (epis or r.epis):
            check_launch(r, epi)
            if epi == G.BIAS_GELU_ERF:
                check_launch(r, epi, with_pos=False)
    finally:
        for name, value in reversed(old):
            L.set_option(name, value)


RAN = set()                # the table's runs that test_gemm_family went through in this process


@pytest.mark.parametrize("run", G.GPU_RUNS, ids=lambda r: r.id)
def test_gemm_family(run):
    RAN.add(run.id)
    check(run)


def test_zz_every_built_kernel_ran_every_epilogue():
    """Every member of tile_kernels<bf16_t, EPI> and tile_kernels<float, EPI> was reported by mh_gemm_last_kernel() for every epilogue
    built for it: asserted from the ids the table's runs produced when all of them ran; under a selection (-k) one representative launch
    each is made first for those the selection left out."""
    if RAN == {r.id for r in G.GPU_RUNS}:      # the whole table ran: the ids it produced must cover everything, nothing is filled in
        assert set(SEEN) == G.built_kernels(), sorted(G.built_kernels() ^ set(SEEN))
    for dt, kid, epi in sorted(G.built_kernels() - set(SEEN)):
        check(next(r for r in G.GPU_RUNS if (r.dtype, r.kernel) == (dt, kid) and epi in r.epis), (epi,))
    assert set(SEEN) == G.built_kernels(), sorted(G.built_kernels() ^ set(SEEN))
    worst = {}
    for (dt, kid, epi), ratio in SEEN.items():
        worst[(dt, kid)] = max(worst.get((dt, kid), (0.0, 0)), (ratio, epi))
    for (dt, kid), (ratio, epi) in sorted(worst.items()):
        print(f"GEMM_MAX {G.kernel_name(kid)} {dt}: max err / tol {ratio:.3f} ({G.EPI_NAMES[epi]})")
