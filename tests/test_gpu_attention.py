"""-m gpu: every attention kernel instantiation, through every mask form the models use, against the fp64 reference of
mh_testing/attention.py.

Per run: max |out - reference| < tol = 4 * floor (floor = the distance of the kernels' DECLARED arithmetic from the reference, computed
on the host from the reference alone; tests/test_attention_cpu.py shows that every single-fault mutant of the case is >= 10 tol away
in >= 4 rows); fully masked rows exactly zero; sentinel columns and guard rows of the output bit-unchanged; the kernel that ran is the
one the table names; and every mutant, evaluated in fp64 on the host, fails the same assertion against the same device output.

Measured on an MI355X over the 156 launches below: max |out - reference| (largest ratio to the asserted bound: tol, or
tol + 2^-16 |reference| for out_split3)
  flash_attn_kernel<float>            5.9e-6 plain, 3.0e-5 through out_split3   (0.39)
  attn_small_f32_kernel<2>            3.0e-6 plain, 2.0e-5 through out_split3   (0.45)
  attn_small_f32_kernel<4>            5.4e-6 plain, 3.0e-5 through out_split3   (0.54)
  flash_attn_kernel<bf16_t>           1.46e-2                                   (0.25)
  flash2_bf16_kernel<2,false,false>   1.46e-2                                   (0.25)
  flash2_bf16_kernel<2,true,false>    7.97e-3                                   (0.25)
  flash2_bf16_kernel<2,false,true>    1.31e-2                                   (0.25)
  flash2_bf16_kernel<2,true,true>     8.32e-3                                   (0.25)
The bf16 kernels sit on the floor itself (floors up to 1.5e-2 in bf16, up to 5.5e-6 in fp32): their error is the rounding of the output to
bf16, which the emulation shares.  No term had to be added to `emulated`, and no kernel failed a case."""
import ctypes as C

import pytest
import torch

from mh_testing import attention as A

pytestmark = pytest.mark.gpu

GUARD_ROWS = 4
SENTINEL = -768.0          # exact in bf16 and fp32
SEEN = {}                  # kernel id -> {dtype: [max err, max err / tol]} over the runs of this process


def _lib():
    from mapperatorinator_amd import _lib
    return _lib, _lib.load()


def _kernel_name(kid):
    names = {A.K_FLASH_F32: "flash_attn_kernel<float>", A.K_FLASH_BF16: "flash_attn_kernel<bf16_t>", A.K_SMALL_K2: "attn_small_f32_kernel<2>",
             A.K_SMALL_K4: "attn_small_f32_kernel<4>"}
    if kid & A.K_FLASH2:
        return "flash2_bf16_kernel<2,%s,%s>" % ("true" if kid & 1 else "false", "true" if kid & 2 else "false")
    return names.get(kid, str(kid))


def launch(r: A.Run):
    """run one row of the table on the device -> (output rows [B*Lq + guard, ld_out] on the host, kernel id)"""
    L, lib = _lib()
    c, P = r.case, A.prepared(r.case)
    inp = P["inputs"]
    bf = r.dtype == A.BF16
    td, es, dt = (torch.bfloat16, 2, L.MH_BF16) if bf else (torch.float32, 4, L.MH_F32)
    inner = c.H * 64
    ld_out = inner + r.ld_extra
    Lkpad = (c.Lk + 63) // 64 * 64
    dev = "cuda"
    vt = A.vt_layout(inp["v"], Lkpad).to(dev, td)
    assert (vt[..., c.Lk:] == 0).all()                                    # the header's contract on the pad columns
    out = torch.full((c.B * c.Lq + GUARD_ROWS, ld_out), SENTINEL, dtype=td, device=dev)
    bias = inp["bias"].to(dev).contiguous() if inp["bias"] is not None else None
    stream = torch.cuda.current_stream().cuda_stream
    keep = [vt, out, bias]
    if r.entry in ("packed", "public"):
        assert c.Lq == c.Lk and c.pads is None and not c.causal and c.q_pos0 == 0 and c.bias in (None, "enc")
        qk = A.pack_qk(inp["q"], inp["k"]).to(dev, td)
        args = (qk.data_ptr(), 2 * inner, inner, vt.data_ptr(), Lkpad, L.ptr(bias), out.data_ptr(), ld_out, c.B, c.Lq, c.H, c.scale,
                c.band, dt)
        if r.entry == "public":
            assert c.open_from == 0 and not r.out_split3
            rc = lib.mh_attention(*args, stream)
        else:
            rc = lib.mh_attention_packed(*args, c.open_from, r.out_split3, stream)
    else:
        p = L.MhAttnProblem()
        p.struct_bytes = C.sizeof(p)
        if r.kcache:
            q = A.rows_of(inp["q"]).to(dev, td)
            kc = A.cache_layout(inp["k"], c.tgt).to(dev, td)
            keep += [q, kc]
            p.q, p.q_rs, p.q_bs = q.data_ptr(), inner * es, c.Lq * inner * es
            p.k, p.k_rs, p.k_hs, p.k_bs = kc.data_ptr(), 64 * es, c.tgt * 64 * es, c.H * c.tgt * 64 * es
        else:
            assert c.Lq == c.Lk
            qk = A.pack_qk(inp["q"], inp["k"]).to(dev, td)
            keep.append(qk)
            p.q, p.q_rs, p.q_bs = qk.data_ptr(), 2 * inner * es, c.Lq * 2 * inner * es
            p.k, p.k_rs, p.k_hs, p.k_bs = qk.data_ptr() + inner * es, 2 * inner * es, 64 * es, c.Lk * 2 * inner * es
        p.vt, p.vt_hs, p.vt_bs, p.Lkpad = vt.data_ptr(), 64 * Lkpad * es, c.H * 64 * Lkpad * es, Lkpad
        if bias is not None:
            f = c.bias_form
            p.bias, p.bias_hs, p.bias_center, p.bias_sign, p.bias_min, p.bias_max = bias.data_ptr(), f.hs, f.center, f.sign, f.lo, f.hi
        if c.pads is not None:
            km = c.key_mask().to(dev)
            keep.append(km)
            p.key_mask, p.mask_ld, p.mask_len = km.data_ptr(), km.shape[1], c.mask_len
        p.out, p.out_rs, p.out_bs = out.data_ptr(), ld_out * es, c.Lq * ld_out * es
        p.Lq, p.Lk, p.scale, p.open_from, p.out_split3 = c.Lq, c.Lk, c.scale, c.open_from, r.out_split3
        p.band, p.causal, p.q_pos0, p.B, p.H, p.dtype = c.band, int(c.causal), c.q_pos0, c.B, c.H, dt
        rc = lib.mh_attention_strided(C.byref(p), stream)
    L.check(rc, r.id)
    kid = lib.mh_attention_last_kernel()
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:      # a device fault: nothing more is started on this GPU by this session
        pytest.exit(f"{r.id}: {e}", returncode=3)
    return out.cpu(), kid


def check(r: A.Run):
    c, P = r.case, A.prepared(r.case)
    raw, kid = launch(r)
    assert kid == r.kernel, f"{r.id}: ran {_kernel_name(kid)}, the table names {_kernel_name(r.kernel)}"
    n, inner = c.B * c.Lq, c.H * 64
    # canaries: the columns past `inner` of every row and the guard rows after the last one, bit for bit
    bits = raw.view(torch.int16 if raw.dtype == torch.bfloat16 else torch.int32)
    want = torch.full((1,), SENTINEL, dtype=raw.dtype).view(bits.dtype).item()
    assert (bits[n:] == want).all(), "guard rows after the output were written"
    assert (bits[:n, inner:] == want).all(), "columns >= inner were written"
    got = A.split3_unpack(raw[:n, :inner]) if r.out_split3 else raw[:n, :inner].float()
    got = A.heads_of(got, c.B, c.H).double()
    ref, tol = P["ref"], P["tol"][r.dtype]

    def bound(reference):      # out_split3 stores hi + lo: two bf16 halves carry 16 significant bits
        return tol + 2.0 ** -16 * reference.abs() if r.out_split3 else torch.full_like(reference, tol)

    def passes(reference):
        """the error assertion of this run against `reference`"""
        err = (got - reference).abs()
        return bool((err < bound(reference)).all()) or (tol == 0 and bool(err.max() == 0))   # (one key: floor = tol = 0, the output is V exactly)

    err = float((got - ref).abs().max())
    e = SEEN.setdefault(kid, {}).setdefault(r.dtype, [0.0, 0.0])
    e[0], e[1] = max(e[0], err), max(e[1], float(((got - ref).abs() / bound(ref)).max()) if tol > 0 else 0.0)
    print(f"ATTN_ERR {r.id} {_kernel_name(kid)} err {err:.3e} tol {tol:.3e} floor {P['floor'][r.dtype]:.3e}")
    assert torch.isfinite(got).all()
    assert passes(ref), f"{r.id}: max |out - reference| = {err:.3e}, tol = 4 * floor = {tol:.3e}"
    dead = P["dead_rows"]
    assert (got.permute(0, 2, 1, 3)[dead] == 0).all(), "a fully masked row is not exactly zero"
    # the tolerance is not vacuous: a kernel computing one of the mutants would have failed the assertion above
    caught = [name for name, mref in P["mutants"].items() if not passes(mref)]
    assert caught, f"{r.id}: no mutant fails the error assertion against this output"
    assert len(caught) == len(P["mutants"]), sorted(set(P["mutants"]) - set(caught))


@pytest.mark.parametrize("run", A.GPU_RUNS, ids=lambda r: r.id)
def test_attention_forms(run):
    check(run)


def test_zz_every_instantiation_ran():
    """All eight instantiations were launched (by the runs above; one representative run each for those a selection left out)."""
    for kid in sorted(A.ALL_KERNELS - set(SEEN)):
        check(next(r for r in A.GPU_RUNS if r.kernel == kid))
    assert set(SEEN) == A.ALL_KERNELS, sorted(_kernel_name(k) for k in A.ALL_KERNELS ^ set(SEEN))
    for kid in sorted(SEEN):
        for dt, (err, ratio) in sorted(SEEN[kid].items()):
            print(f"ATTN_MAX {_kernel_name(kid)} {dt}: max err {err:.3e}, max err / bound {ratio:.3f}")
