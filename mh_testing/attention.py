"""Host side of the attention kernel tests (tests/test_attention_cpu.py, tests/test_gpu_attention.py): the documented mask predicate,
an fp64 reference, the same function in the kernels' declared arithmetic (its distance from the reference is the error floor the
tolerances are built on), the buffer layouts of the three entries, seeded inputs with LOUD keys on every edge, and MUTANTS -- the
same problem with one fault each -- that show on the CPU that the tolerance of a case would catch an off-by-one.  No GPU needed.

Shapes: q [B, H, Lq, 64], k / v [B, H, Lk, 64], masks [B, Lq, Lk], outputs [B, H, Lq, 64]."""
from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass, replace
from typing import Optional, Tuple

import torch

TILE = 64


# ---- the documented predicate ----------------------------------------------------------------------------------------------------
def _in_band(rel, band, swap=False):
    """band > 0: -(band - 1) <= rel <= band; band < 0: |rel| <= -band.  `swap`: the other convention at the same width (a mutant)."""
    w = abs(band)
    asym = (band > 0) != swap
    return ((rel >= -(w - 1)) & (rel <= w)) if asym else (rel.abs() <= w)


def visible(B, Lq, Lk, band=0, open_from=0, causal=False, q_pos0=0, key_mask=None, mask_len=0, *, _swap_band=False,
            _strict_causal=False, _open_keys=True, _open_queries=True):
    """bool [B, Lq, Lk]: key `key` is visible from query row q (qpos = q_pos0 + q) iff  key < Lk  and  (key >= mask_len or
    key_mask[b][key] != 0)  and  (band == 0 or key in the band or, with open_from > 0, key >= open_from or qpos >= open_from)  and
    (not causal or key <= qpos).  The underscore arguments exist for mutants() only."""
    key = torch.arange(Lk)[None, :]
    qpos = q_pos0 + torch.arange(Lq)[:, None]
    ok = torch.ones(Lq, Lk, dtype=torch.bool)
    if band != 0:
        b = _in_band(key - qpos, band, _swap_band)
        if open_from > 0:
            if _open_keys:
                b = b | (key >= open_from)
            if _open_queries:
                b = b | (qpos >= open_from)
        ok = ok & b
    if causal:
        ok = ok & ((key < qpos) if _strict_causal else (key <= qpos))
    ok = ok[None].expand(B, Lq, Lk).clone()
    if key_mask is not None:
        km = torch.as_tensor(key_mask)[:, :Lk] != 0
        m = torch.ones(B, Lk, dtype=torch.bool)
        n = min(mask_len, Lk)
        m[:, :n] = km[:, :n]
        ok = ok & m[:, None, :]
    return ok


# ---- bias, reference, emulation -------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class BiasForm:
    """bias[h][center + clamp(sign * (key - qpos), lo, hi)] over a table [H][hs]"""
    hs: int
    center: int
    sign: int
    lo: int
    hi: int


def enc_bias_form(L):      # the encoders: table [H][2L - 1] indexed by key - query
    return BiasForm(2 * L - 1, L - 1, 1, -(L - 1), L - 1)


def dec_bias_form(tgt):    # the T5 decoder: table [H][tgt] indexed by the distance query - key >= 0
    return BiasForm(tgt, 0, -1, 0, tgt - 1)


def bias_index(form: BiasForm, Lq, Lk, q_pos0=0):
    key = torch.arange(Lk)[None, :]
    qpos = q_pos0 + torch.arange(Lq)[:, None]
    return form.center + (form.sign * (key - qpos)).clamp(form.lo, form.hi)


def bias_term(table, form: BiasForm, Lq, Lk, q_pos0=0, head_shift=0):
    """[H, Lq, Lk] in the table's dtype"""
    H = table.shape[0]
    t = table[(torch.arange(H) + head_shift) % H]
    return t[:, bias_index(form, Lq, Lk, q_pos0)]


def _attend(q, k, v, scale, vis, bias, dt, round_p=None, round_out=None):
    s = torch.matmul(q.to(dt), k.to(dt).transpose(-1, -2)) * torch.tensor(scale, dtype=dt)
    if bias is not None:
        s = s + bias.to(dt)[None]
    s = s.masked_fill(~vis[:, None], float("-inf"))
    alive = vis.any(-1)[:, None, :, None]                           # rows with a visible key
    m = s.max(-1, keepdim=True).values
    p = torch.exp(s - torch.where(alive, m, torch.zeros_like(m)))   # a fully masked row: exp(-inf) = 0, never NaN
    l = p.sum(-1, keepdim=True)
    if round_p is not None:
        p = round_p(p)
    o = torch.matmul(p, v.to(dt)) / torch.where(alive, l, torch.ones_like(l))
    o = torch.where(alive, o, torch.zeros_like(o))                  # a fully masked row gives zeros, as both kernels state
    return round_out(o) if round_out is not None else o


def reference(q, k, v, scale, vis, bias_table=None, bias_form=None, q_pos0=0, head_shift=0):
    """fp64 [B, H, Lq, 64]"""
    bias = None
    if bias_table is not None:
        bias = bias_term(bias_table.double(), bias_form, q.shape[2], k.shape[2], q_pos0, head_shift)
    return _attend(q, k, v, scale, vis, bias, torch.float64)


def _bf16r(x):
    return x.to(torch.bfloat16).to(x.dtype)


def emulated(q, k, v, scale, vis, bias_table=None, bias_form=None, q_pos0=0, dtype="f32"):
    """The reference in the kernels' declared arithmetic, returned as fp64.  f32: scores and softmax in fp32.  bf16: additionally
    the (unnormalised) probabilities rounded to bf16 before P V -- the row sum is taken of the unrounded ones, as both bf16 kernels
    do -- and the output rounded to bf16."""
    bias = None
    if bias_table is not None:
        bias = bias_term(bias_table.float(), bias_form, q.shape[2], k.shape[2], q_pos0)
    if dtype == "f32":
        return _attend(q, k, v, scale, vis, bias, torch.float32).double()
    return _attend(q, k, v, scale, vis, bias, torch.float32, round_p=_bf16r, round_out=_bf16r).double()


# ---- layouts -----------------------------------------------------------------------------------------------------------------------
def pack_qk(q, k):
    """[B, H, L, 64] x 2 -> the packed [B*L, 2*inner] q | k buffer of mh_attention (k_col0 = inner)"""
    B, H, L, _ = q.shape
    f = lambda x: x.permute(0, 2, 1, 3).reshape(B * L, H * 64)
    return torch.cat([f(q), f(k)], 1).contiguous()


def rows_of(x):
    """[B, H, L, 64] -> [B*L, inner] (the q rows of the strided entry; the layout of a plain output)"""
    B, H, L, _ = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * L, H * 64).contiguous()


def heads_of(rows, B, H):
    """inverse of rows_of: [B*L, >= inner] -> [B, H, L, 64] (columns beyond inner are dropped)"""
    L = rows.shape[0] // B
    return rows[:, :H * 64].reshape(B, L, H, 64).permute(0, 2, 1, 3).contiguous()


def cache_layout(k, cache_len, fill=7.0):
    """[B, H, Lk, 64] -> the decoder's cache layout [B][H][cache_len][64], cache_len > Lk; rows >= Lk hold `fill` (a key that must never
    be read as visible: it would outshout every real one)"""
    B, H, Lk, _ = k.shape
    assert cache_len > Lk
    out = torch.full((B, H, cache_len, 64), fill, dtype=k.dtype)
    out[:, :, :Lk] = k
    return out


def vt_layout(v, Lkpad):
    """[B, H, Lk, 64] -> V^T [B][H][64][Lkpad] with zero pad columns (the header's contract)"""
    B, H, Lk, _ = v.shape
    assert Lkpad % 64 == 0 and Lkpad >= Lk
    out = torch.zeros(B, H, 64, Lkpad, dtype=v.dtype)
    out[..., :Lk] = v.transpose(-1, -2)
    return out


def split3_unpack(P):
    """rows of [32 x bf16 hi | 32 x bf16 lo] blocks (MhGemm.w_split3 / out_split3), viewed from an fp32-sized buffer -> fp32 hi + lo"""
    n = P.shape[0]
    b = P.contiguous().view(torch.bfloat16).reshape(n, -1, 2, 32).float()
    return (b[:, :, 0] + b[:, :, 1]).reshape(n, -1)


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    """One attention PROBLEM (what is computed); Run below adds how it is launched."""
    name: str
    B: int
    H: int
    Lq: int
    Lk: int
    scale: float
    band: int = 0
    open_from: int = 0
    causal: bool = False
    q_pos0: int = 0
    pads: Optional[Tuple[int, ...]] = None    # left pads per batch row -> key mask, mask_len = Lk; a 0 is planted at mask_len - 1 of rows 0, 1
    bias: Optional[str] = None                # "enc" | "dec"
    tgt: int = 0                              # decoder table length = cache_len of the cache layout
    small: bool = False                       # also plant the key-split kernel's wave seams (multiples of 32)

    @property
    def bias_form(self):
        return None if self.bias is None else (enc_bias_form(self.Lk) if self.bias == "enc" else dec_bias_form(self.tgt))

    @property
    def mask_len(self):
        return self.Lk if self.pads is not None else 0

    def key_mask(self):
        if self.pads is None:
            return None
        m = torch.ones(self.B, self.Lk, dtype=torch.uint8)
        for b, p in enumerate(self.pads):
            m[b, :p] = 0
        m[:2, self.Lk - 1] = 0     # the hole a `mask_len - 1` fault would fill
        return m

    def vis_args(self):
        return dict(B=self.B, Lq=self.Lq, Lk=self.Lk, band=self.band, open_from=self.open_from, causal=self.causal,
                    q_pos0=self.q_pos0, key_mask=self.key_mask(), mask_len=self.mask_len)


def _edge_keys(c: Case):
    """keys that sit on an edge for every query that sees them"""
    e = {c.Lk - 1}
    step = 32 if c.small else TILE           # 64-key tiles; the key-split kernel's wave seams KBW * 16 * w are multiples of 32
    for m in range(0, c.Lk + step, step):
        e |= {m - 1, m}
    if c.band != 0 and 0 < c.open_from < c.Lk:
        e |= {c.open_from - 1, c.open_from}
    return sorted(k for k in e if 0 <= k < c.Lk)


def _aimed_pairs(c: Case):
    """(query row, key) pairs whose edge belongs to ONE query: the band ends and the causal diagonal of every 8th query, the last key
    under a causal mask, the two pairs that reach the ends of the encoder's bias table, a far key for the first and the last pad
    query, and -- where there are too few queries for chance to help -- keys 0 and Lk - 1 for query 0."""
    w = abs(c.band)
    lo, hi = (-(w - 1), w) if c.band > 0 else (-w, w)
    pairs, strong = [], None
    for q in range(5 if c.Lq > 5 else 0, c.Lq, 8):
        qpos = c.q_pos0 + q
        if c.band != 0:
            pairs += [(q, qpos + lo - 1), (q, qpos + lo), (q, qpos + hi), (q, qpos + hi + 1)]
        if c.causal:
            pairs += [(q, qpos), (q, qpos + 1)]
    if c.causal and 0 <= c.Lk - 1 - c.q_pos0 < c.Lq:
        strong = (c.Lk - 1 - c.q_pos0, c.Lk - 1)     # its only query: lifted 3 ABOVE the row (a copy of it with V = 0 must show)
    if c.bias == "enc":
        pairs += [(c.Lq - 1, 0), (0, c.Lk - 1)]
    if c.band != 0 and 0 < c.open_from < c.Lk:
        for q in {c.open_from - c.q_pos0, c.Lq - 1}:
            pairs.append((q, 0 if q - w > 0 else c.Lk - 1))
    if c.Lq < 16:
        pairs += [(0, 0), (0, c.Lk - 1)]
    out = {(q, k): 0.0 for q, k in pairs if 0 <= q < c.Lq and 0 <= k < c.Lk and c.Lk >= 2}
    if strong is not None and c.Lk >= 2:
        out[strong] = 3.0
    return sorted((q, k, lift) for (q, k), lift in out.items())


def make_inputs(c: Case):
    """Seeded by the case's name; q, k, v rounded to bf16 for both dtypes (both see the same problem, and the products of the bf16
    kernels are exact).  Score standard deviation ~3: sigma(q) = sigma(k) = sqrt(3 / (8 * scale)); bias table 0.5 N(0, 1) with the two
    entries at each end set to +-2 (a clamp that is off by one shows); V ~ N(0, 1).  Louder keys are planted on the edges:
      - the rows of _edge_keys and the first unmasked key of each left-padded batch row are multiplied by 3;
      - for each pair of _aimed_pairs the key gets a component along its query that lifts that one logit to the largest other logit
        of the query's row: the key then holds a third to a half of the row, whichever side of the edge it belongs to."""
    g = torch.Generator().manual_seed(zlib.crc32(c.name.encode()))
    sigma = (3.0 / (8.0 * c.scale)) ** 0.5
    q = torch.randn(c.B, c.H, c.Lq, 64, generator=g) * sigma
    k = torch.randn(c.B, c.H, c.Lk, 64, generator=g) * sigma
    v = torch.randn(c.B, c.H, c.Lk, 64, generator=g)
    bias = None
    if c.bias is not None:
        bias = torch.randn(c.H, c.bias_form.hs, generator=g) * 0.5
        if c.bias_form.hs >= 4:
            bias[:, 0], bias[:, 1], bias[:, -2], bias[:, -1] = 2.0, -2.0, -2.0, 2.0
    q = _bf16r(q)
    k[:, :, _edge_keys(c)] *= 3.0
    for b, p in enumerate(c.pads or ()):
        if p < c.Lk and p not in _edge_keys(c):
            k[b, :, p] *= 3.0
    pairs = _aimed_pairs(c)
    if pairs:
        vis = visible(**c.vis_args())
        s = torch.matmul(q.double(), k.double().transpose(-1, -2)) * c.scale
        bt = bias_term(bias.double(), c.bias_form, c.Lq, c.Lk, c.q_pos0) if bias is not None else torch.zeros(c.H, c.Lq, c.Lk, dtype=torch.float64)
        s = (s + bt[None]).masked_fill(~vis[:, None], float("-inf"))
        for qi, key, above in pairs:
            row = s[:, :, qi].clone()
            row[:, :, key] = float("-inf")
            target = row.max(-1).values                                        # [B, H]: the largest OTHER visible logit of the row
            qv = q[:, :, qi].double()
            have = (qv * k[:, :, key].double()).sum(-1) * c.scale + bt[None, :, qi, key]
            lift = torch.where(torch.isfinite(target), target + above - have, torch.zeros_like(have))
            k[:, :, key] += (lift / (c.scale * (qv * qv).sum(-1)))[..., None].float() * q[:, :, qi]
    return dict(q=q, k=_bf16r(k), v=_bf16r(v), bias=bias)


def evaluate(c: Case, inp, mut=None):
    """fp64 reference of the case, or of one of its mutants (a dict of overrides from mutants())"""
    mut = dict(mut or {})
    va = c.vis_args()
    va.update(mut.pop("vis", {}))
    vis = visible(**va)
    if "hide" in mut:
        vis = vis & ~mut.pop("hide")
    form = c.bias_form
    if form is not None and "form" in mut:
        form = replace(form, **mut.pop("form"))
    k, v = inp["k"], inp["v"]
    q_pos0 = va["q_pos0"]
    head_shift = mut.pop("head_shift", 0)
    extra = mut.pop("extra_key", False)
    assert not mut, mut
    if not extra:
        return reference(inp["q"], k, v, c.scale, vis, inp["bias"], form, q_pos0, head_shift)
    # one clamped copy of key Lk - 1 with V = 0: what reading one key past Lk does
    k = torch.cat([k, k[:, :, -1:]], 2)
    v = torch.cat([v, torch.zeros_like(v[:, :, -1:])], 2)
    vis = torch.cat([vis, vis[:, :, -1:]], 2)
    bias = None
    if inp["bias"] is not None:
        bias = bias_term(inp["bias"].double(), form, c.Lq, c.Lk, q_pos0, head_shift)
        bias = torch.cat([bias, bias[..., -1:]], -1)
    return _attend(inp["q"], k, v, c.scale, vis, bias, torch.float64)


def _tile_hides(c: Case):
    """name -> bool [B, Lq, Lk]: one whole 64-key tile dropped from every 64-query block, at the first tile of the block's range
    (t_lo), at the last tile of its band / causal range (t_hi), at the first tile of the open pad columns (t_open)"""
    geo = visible(1, c.Lq, c.Lk, c.band, 0, c.causal, c.q_pos0)[0]       # band and causal only: what the tile ranges are built from
    has_open = c.band != 0 and 0 < c.open_from < c.Lk
    out = {n: torch.zeros(c.B, c.Lq, c.Lk, dtype=torch.bool) for n in ("skip_t_lo", "skip_t_hi", "skip_t_open")}
    for q0 in range(0, c.Lq, TILE):
        q1 = min(q0 + TILE, c.Lq)
        keys = geo[q0:q1].any(0).nonzero().flatten()
        if len(keys) == 0:
            continue
        t_lo, t_hi, t_open = int(keys[0]) // TILE, int(keys[-1]) // TILE, None
        if has_open:
            if c.q_pos0 + q1 - 1 >= c.open_from:
                t_lo, t_hi = 0, (c.Lk - 1) // TILE
            else:
                t_open = c.open_from // TILE
        for n, t in (("skip_t_lo", t_lo), ("skip_t_hi", t_hi), ("skip_t_open", t_open)):
            if t is not None:
                out[n][:, q0:q1, t * TILE:(t + 1) * TILE] = True
    if not has_open:
        del out["skip_t_open"]
    return out


def mutants(c: Case):
    """name -> overrides for evaluate(): the same case with ONE fault, applicable ones only (a fault that cannot change the function
    on this case's domain -- a clamp end no visible pair reaches, a bias on a single key -- is left out)."""
    m = {}
    w = abs(c.band)
    sgn = 1 if c.band > 0 else -1
    if c.band != 0:
        m["band_wider"] = dict(vis=dict(band=sgn * (w + 1)))
        m["band_narrower"] = dict(vis=dict(band=sgn * (w - 1)))
        m["band_other_convention"] = dict(vis=dict(_swap_band=True))
        if 0 < c.open_from < c.Lk:
            m["open_from_plus1"] = dict(vis=dict(open_from=c.open_from + 1))
            m["open_from_minus1"] = dict(vis=dict(open_from=c.open_from - 1))
            m["open_keys_ignored"] = dict(vis=dict(_open_keys=False))
            m["open_queries_ignored"] = dict(vis=dict(_open_queries=False))
    if c.causal:
        m["causal_strict"] = dict(vis=dict(_strict_causal=True))
        m["causal_dropped"] = dict(vis=dict(causal=False))
    if c.causal or c.band != 0 or (c.bias is not None and c.Lk >= 2):
        m["q_pos0_plus1"] = dict(vis=dict(q_pos0=c.q_pos0 + 1))
    if c.pads is not None:
        km = c.key_mask()
        m["mask_dropped"] = dict(vis=dict(key_mask=None, mask_len=0))
        m["mask_shift_right"] = dict(vis=dict(key_mask=torch.cat([km[:, :1], km[:, :-1]], 1)))
        m["mask_shift_left"] = dict(vis=dict(key_mask=torch.cat([km[:, 1:], km[:, -1:]], 1)))
        m["mask_len_minus1"] = dict(vis=dict(mask_len=c.mask_len - 1))
    m["last_key_invisible"] = dict(hide=(torch.arange(c.Lk) == c.Lk - 1)[None, None].expand(c.B, c.Lq, c.Lk))
    m["key_past_Lk"] = dict(extra_key=True)
    if c.bias is not None and c.Lk >= 2:
        f = c.bias_form
        vis = visible(**c.vis_args()).any(0)
        idx = f.sign * (torch.arange(c.Lk)[None, :] - (c.q_pos0 + torch.arange(c.Lq)[:, None]))
        m["bias_sign_flipped"] = dict(form=dict(sign=-f.sign))
        if bool(((idx <= f.lo) & vis).any()):
            m["bias_clamp_min_plus1"] = dict(form=dict(lo=f.lo + 1))
        if bool(((idx >= f.hi) & vis).any()):
            m["bias_clamp_max_minus1"] = dict(form=dict(hi=f.hi - 1))
        if c.H >= 2:
            m["bias_next_head"] = dict(head_shift=1)
    for n, h in _tile_hides(c).items():
        m[n] = dict(hide=h)
    return {n: mu for n, mu in m.items() if _changes_the_function(c, mu)}


def _changes_the_function(c: Case, mu):
    """does the fault change the visible set, or the bias entry of a visible pair, on this case's own domain?"""
    if mu.get("extra_key") or mu.get("head_shift"):
        return True
    va = c.vis_args()
    base = visible(**va)
    va.update(mu.get("vis", {}))
    vis = visible(**va) & ~mu.get("hide", torch.zeros_like(base))
    if not torch.equal(vis, base):
        return True
    if c.bias is None:
        return False
    form = replace(c.bias_form, **mu.get("form", {}))
    return bool(((bias_index(form, c.Lq, c.Lk, va["q_pos0"]) != bias_index(c.bias_form, c.Lq, c.Lk, c.q_pos0)) & base.any(0)).any())


@functools.lru_cache(maxsize=None)
def prepared(c: Case):
    """Everything the tests need of a case, computed once and shared: inputs, visibility, fp64 reference, the per-dtype floor
    (max |emulated - reference|: from the reference alone) and tol = 4 * floor, and the fp64 output of every mutant."""
    inp = make_inputs(c)
    vis = visible(**c.vis_args())
    ref = evaluate(c, inp)
    out = dict(inputs=inp, visible=vis, ref=ref, dead_rows=~vis.any(-1), floor={}, tol={})
    for dt in ("f32", "bf16"):
        emu = emulated(inp["q"], inp["k"], inp["v"], c.scale, vis, inp["bias"], c.bias_form, c.q_pos0, dt)
        out["floor"][dt] = float((emu - ref).abs().max())
        out["tol"][dt] = 4.0 * out["floor"][dt]
    out["mutants"] = {n: evaluate(c, inp, mu) for n, mu in mutants(c).items()}
    return out


def rows_off(a, b, by):
    """number of output rows (one query of one head) in which a and b differ by at least `by` somewhere"""
    d = (a - b).abs().amax(-1)
    return int(((d >= by) & (d > 0)).sum())


# ---- the GPU table -------------------------------------------------------------------------------------------------------------------
F32, BF16 = "f32", "bf16"
K_FLASH_F32, K_FLASH_BF16, K_SMALL_K2, K_SMALL_K4, K_FLASH2 = 1, 2, 3, 4, 8      # MhAttnKernel (include/mapperhip.h)


def k_flash2(bias, simple):
    return K_FLASH2 | (1 if bias else 0) | (2 if simple else 0)


ALL_KERNELS = {K_FLASH_F32, K_FLASH_BF16, K_SMALL_K2, K_SMALL_K4, k_flash2(0, 0), k_flash2(0, 1), k_flash2(1, 0), k_flash2(1, 1)}


@dataclass(frozen=True)
class Run:
    case: Case
    entry: str            # "strided" (mh_attention_strided) | "packed" (mh_attention_packed) | "public" (mh_attention)
    dtype: str
    kernel: int           # what mh_attention_last_kernel() must report
    kcache: bool = False  # strided: K in the cache layout [B][H][tgt][64] (else the packed q | k buffer; needs Lq == Lk)
    out_split3: int = 0
    ld_extra: int = 0     # ld_out = inner + ld_extra

    @property
    def id(self):
        return "-".join([self.case.name, self.entry, self.dtype] + (["split3"] if self.out_split3 else []) +
                        ([f"ld+{self.ld_extra}"] if self.ld_extra else []))


def _lkpad(L):
    return (L + 63) // 64 * 64


def gpu_runs():
    R = []

    def both(c, entry, k_bf16, kcache=False, unaligned=False):
        R.append(Run(c, entry, F32, K_FLASH_F32, kcache))
        R.append(Run(c, entry, BF16, k_bf16, kcache))
        if unaligned:
            R.append(Run(c, entry, BF16, K_FLASH_BF16, kcache, ld_extra=4))

    # encoder: bias [H][2L-1], sign +1, scale 1
    for L in (200, 1, 63, 64, 65, 129):
        c = Case(f"enc{L}", 2, 3 if L == 200 else 2, L, L, 1.0, bias="enc")
        both(c, "strided", k_flash2(1, 1), unaligned=L == 200)
        both(c, "public", k_flash2(1, 1), unaligned=L == 200)
    # T5 prompt prefill: causal, key mask (left pads), decoder bias, K in the cache layout
    pads = (0, 5, 70, 149)
    both(Case("t5pre", 4, 3, 150, 150, 1.0, causal=True, pads=pads, bias="dec", tgt=160), "strided", k_flash2(1, 0), True, True)
    # Whisper prompt prefill: no bias, band 0 / -8, scale 1/8
    for band in (0, -8):
        both(Case(f"whpre_b{band}", 4, 3, 150, 150, 0.125, band=band, causal=True, pads=pads, tgt=160), "strided", k_flash2(0, 0),
             True, True)
    # cross-attention over the cache layout, no mask
    for Lq in (1, 70, 129):
        B, H = (3, 4) if Lq == 1 else (2, 2)
        both(Case(f"cross{Lq}", B, H, Lq, 1251, 1.0, tgt=1251 + 5), "strided", k_flash2(0, 1), True)
    # chunked causal: q_pos0 = Lk - Lq, with and without the T5 bias
    both(Case("chunk", 2, 2, 40, 150, 1.0, causal=True, q_pos0=110, tgt=160), "strided", k_flash2(0, 0), True)
    both(Case("chunk_bias", 2, 2, 40, 150, 1.0, causal=True, q_pos0=110, bias="dec", tgt=160), "strided", k_flash2(1, 0), True)
    # DiT band with pad_sequence columns
    for of in (0, 192, 200, 299, 300):
        c = Case(f"dit_o{of}", 2, 2, 300, 300, 0.125, band=64, open_from=of)
        R.append(Run(c, "strided", F32, K_FLASH_F32))
        R.append(Run(c, "packed", BF16, k_flash2(0, 0)))
        R.append(Run(c, "packed", BF16, K_FLASH_BF16, ld_extra=4))
    # the key-split kernel (fp32), and the flash kernel above its workgroup limit with the same options
    for band in (0, 32, -8):
        for of in (0, 80):
            for L in (15, 17, 96, 128, 129, 250, 256):
                c = Case(f"small{L}_b{band}_o{of}", 2, 2, L, L, 0.125, band=band, open_from=of, small=True)
                for s3 in (0, 1):
                    R.append(Run(c, "packed", F32, K_SMALL_K2 if L <= 128 else K_SMALL_K4, out_split3=s3))
            c = Case(f"big250_b{band}_o{of}", 9, 8, 250, 250, 0.125, band=band, open_from=of, small=True)
            for s3 in (0, 1):
                R.append(Run(c, "packed", F32, K_FLASH_F32, out_split3=s3))
    return R


GPU_RUNS = gpu_runs()
GPU_CASES = list(dict.fromkeys(r.case for r in GPU_RUNS))
