"""TEST SUPPORT for tests/test_gpu_beam_self_kv_fp8.py: the step-wise decode entries driven by hand over caller-owned buffers -- the
indexed step with and without the e4m3 shadow of the self-attention cache (mh_t5_step_indexed_skv8 / mh_t5_step_indexed), the
prefill and the shadow's fill, and the two ways a beam search's reorder can be applied: to the index table (mh_t5_reorder_index), or,
as a copy route would, to the caches themselves (mh_t5_reorder_cache for the bf16 rows, torch ops for the shadow's bytes and scales)."""
from __future__ import annotations

import ctypes as C

import torch

MARKER = 0xA5


def self_caches(eng, ws: torch.Tensor, R: int):
    """views (k, v), each (n_dec, R, H, tgt_len, 64) of the storage type, of the self-attention caches inside the step workspace `ws`"""
    from mapperatorinator_amd import _lib
    p = eng.packed
    k, v = C.c_void_p(), C.c_void_p()
    _lib.check(eng.lib.mh_t5_decode_self_cache(C.byref(p.cfg), R, ws.data_ptr(), C.byref(k), C.byref(v)), "mh_t5_decode_self_cache")
    shape = (p.cfg.n_dec_layers, R, p.cfg.n_heads, p.tgt_len, 64)
    n = shape[0] * shape[1] * shape[2] * shape[3] * 64 * torch.empty(0, dtype=eng.dtype).element_size()
    return [ws[ptr - ws.data_ptr(): ptr - ws.data_ptr() + n].view(eng.dtype).view(shape) for ptr in (k.value, v.value)]


def shadow_views(eng, sh: torch.Tensor, R: int):
    """views of a caller-owned shadow of R rows (mh_t5_self_kv_fp8_bytes; layout in include/mapperhip.h): e4m3 bytes uint8
    (n_dec, 2, R, H, tgt_len, 64), fp32 scales (n_dec, 2, R, H, tgt_len), and the bool mask of the bytes that belong to neither"""
    cfg = eng.packed.cfg
    shape = (cfg.n_dec_layers, 2, R, cfg.n_heads, eng.packed.tgt_len)
    rows = shape[0] * shape[1] * shape[2] * shape[3] * shape[4]
    off = (rows * 64 + 255) // 256 * 256
    assert sh.numel() >= off + rows * 4
    slack = torch.ones(sh.numel(), dtype=torch.bool, device=sh.device)
    slack[: rows * 64] = False
    slack[off: off + rows * 4] = False
    return sh[: rows * 64].view(*shape, 64), sh[off: off + rows * 4].view(torch.float32).view(shape), slack


def new_shadow(eng, R: int, fill: int = MARKER) -> torch.Tensor:
    n = int(eng.lib.mh_t5_self_kv_fp8_bytes(C.byref(eng.packed.cfg), R))
    assert n > 0
    return torch.full((n,), fill, dtype=torch.uint8, device=eng.device)


def run_steps(eng, kv, kv8, ids, mask, P, nb, srcs=None, route="table", shadow=True, prefill=None, keep=False):
    """Steps over all R rows for positions first .. n_pos-1, ids (n_pos, R) by absolute position, a reorder after every step when
    `srcs` (n_pos, R) is given.
      route "table":   the reorder goes to the index table (mh_t5_reorder_index), the caches stay where they are;
      route "permute": the table stays the identity (as initialised) and the test itself copies what a copy route would copy after
                       every step: the bf16 cache rows (mh_t5_reorder_cache), the shadow's bytes and its scales (torch ops).
      shadow:  mh_t5_step_indexed_skv8 over a shadow of this call's own (pre-filled with MARKER), else mh_t5_step_indexed.
      prefill: (prompts int32 (G, P), masks uint8 (G, P) or None, n) on the device: mh_t5_step_prefill of positions 0 .. n-1, then
               (shadow) mh_t5_self_kv_fp8_fill, the table initialised for them; first = n.
    -> dict(logits (n_pos - first, R, V) on the CPU[, ws, sh: the buffers, with `keep`])"""
    from mapperatorinator_amd import _lib
    lib, p = eng.lib, eng.packed
    n_pos, R = ids.shape
    cfg, w, V = C.byref(p.cfg), C.byref(p.w), p.vocab_out
    first = 0
    eng._enter()
    with eng.on_stream():
        s = eng._s()
        ids_d = ids.to(eng.device, torch.int32).contiguous()
        srcs_d = None if srcs is None else srcs.to(eng.device, torch.int32).contiguous()
        mask_d = None if mask is None else mask.to(eng.device, torch.uint8).contiguous()
        ws = torch.zeros(int(lib.mh_t5_decode_workspace_bytes(cfg, R)), dtype=torch.uint8, device=eng.device)
        sh = new_shadow(eng, R) if shadow else None
        tabs = [torch.full((int(lib.mh_t5_beam_index_bytes(cfg, R)),), 255, dtype=torch.uint8, device=eng.device) for _ in range(2)]
        if prefill is not None:
            prompts, pmasks, first = prefill
            _lib.check(lib.mh_t5_step_prefill(cfg, w, kv.data_ptr(), prompts.shape[0], prompts.data_ptr(), _lib.ptr(pmasks), prompts.shape[1],
                                              first, ws.data_ptr(), ws.numel(), R, s), "mh_t5_step_prefill")
            if shadow:
                _lib.check(lib.mh_t5_self_kv_fp8_fill(cfg, R, prompts.shape[0], first, ws.data_ptr(), ws.numel(), sh.data_ptr(), s),
                           "mh_t5_self_kv_fp8_fill")
        _lib.check(lib.mh_t5_beam_index_init(cfg, R, nb, first, tabs[0].data_ptr(), s), "mh_t5_beam_index_init")
        out = torch.empty((n_pos - first, R, V), dtype=torch.float32, device=eng.device)
        cur = 0
        if srcs is not None and route == "permute":
            scratch = torch.empty(int(lib.mh_t5_reorder_cache_scratch_bytes(cfg, R, n_pos)), dtype=torch.uint8, device=eng.device)
            q8, sc, _ = shadow_views(eng, sh, R)
        for pos in range(first, n_pos):
            common = (R, nb, ids_d[pos].data_ptr(), pos, _lib.ptr(mask_d), P, out[pos - first].data_ptr(), ws.data_ptr(), ws.numel())
            if shadow:
                rc = lib.mh_t5_step_indexed_skv8(cfg, w, kv.data_ptr(), _lib.ptr(kv8), *common, tabs[cur].data_ptr(), sh.data_ptr(), s)
                _lib.check(rc, "mh_t5_step_indexed_skv8")
            else:
                _lib.check(lib.mh_t5_step_indexed(cfg, w, kv.data_ptr(), _lib.ptr(kv8), *common, tabs[cur].data_ptr(), s), "mh_t5_step_indexed")
            if srcs is None:
                continue
            n = pos + 1
            if route == "table":
                rc = lib.mh_t5_reorder_index(cfg, R, srcs_d[pos].data_ptr(), n, tabs[cur].data_ptr(), tabs[cur ^ 1].data_ptr(), s)
                _lib.check(rc, "mh_t5_reorder_index")
                cur ^= 1
            else:
                rc = lib.mh_t5_reorder_cache(cfg, R, srcs_d[pos].data_ptr(), n, ws.data_ptr(), ws.numel(), scratch.data_ptr(),
                                             scratch.numel(), s)
                _lib.check(rc, "mh_t5_reorder_cache")
                src = srcs_d[pos].long()
                q8[:, :, :, :, :n] = q8.index_select(2, src)[:, :, :, :, :n]       # row b <- row src[b], positions < n
                sc[:, :, :, :, :n] = sc.index_select(2, src)[:, :, :, :, :n]
    eng._leave()
    eng.synchronize()
    res = dict(logits=out.cpu())
    if keep:
        res.update(ws=ws, sh=sh)
    return res


def oracle_gate(name, lg8, lg16, want, plain, gap_limit, excess):
    """The logit gate of tests/test_gpu_self_kv_fp8.py on RAW step logits: lg8 (mode on) against `want`, the hooked oracle's processed
    scores, on the entries finite there (under the neutral kwargs the processors only mask, so a finite processed score is the raw
    logit); floor = lg16 (mode off, the same ids) against `plain`, the plain oracle's.  Prints, then asserts.  -> (floor, excess, flips)"""
    assert lg8.shape == want.shape == lg16.shape == plain.shape, (lg8.shape, want.shape, lg16.shape, plain.shape)
    fin, finp = torch.isfinite(want), torch.isfinite(plain)
    assert torch.isfinite(lg8).all() and torch.isfinite(lg16).all() and fin.any()
    worst8 = (lg8[fin] - want[fin]).abs().max().item()
    floor = (lg16[finp] - plain[finp]).abs().max().item()
    top2 = want.topk(2, dim=-1).values
    gap = top2[..., 0] - top2[..., 1]
    miss = lg8.masked_fill(~fin, float("-inf")).argmax(-1) != want.argmax(-1)
    n_bad, n_tie = int((miss & (gap > gap_limit)).sum()), int((miss & (gap <= gap_limit)).sum())
    moved = (lg8 - lg16).abs().max().item()
    print(f"{name}: {gap.numel()} steps ({int((gap <= gap_limit).sum())} inside the {gap_limit} gap), {n_tie} near-tie flips, {n_bad} real "
          f"mismatches; worst |dlogit| {worst8:.3f} vs the hooked oracle, floor (mh_t5_step_indexed vs the plain oracle on the same ids) "
          f"{floor:.3f}, excess {worst8 - floor:+.3f} (allowed {excess}); the mode moves the logits by up to {moved:.3f}")
    assert moved > 0, "the mode is not on: the logits equal the mode-off run's"
    assert n_bad == 0
    assert worst8 < floor + excess
    return floor, worst8 - floor, n_tie
