"""Restatement of mh_beam_step_sample (include/mapperhip.h, csrc/beam.hip) for tests: the library's counter-based uniform in exact
integer arithmetic (numpy uint64 wraps like the device's uint64_t), and the rule -- HF's TopK / TopP warpers as one cut value per beam
row, Gumbel keys, draw order -- in numpy fp64 (or fp32, to see what rounding does to an order)."""
from __future__ import annotations

import numpy as np

_U = np.uint64
GOLDEN = _U(0x9E3779B97F4A7C15)
U_MAX = np.float32(1.0 - 2.0 ** -24)             # uniform01 reaches exactly 1.0: the key clamps it


def rng_mix64(seed, row, step) -> np.ndarray:
    """rng_mix64 of csrc/common.hpp: uint64 words from (seed uint64, row uint32, step uint32); arguments broadcast."""
    seed, row, step = (np.asarray(a, dtype=_U) for a in (seed, row, step))
    with np.errstate(over="ignore"):
        z = seed + GOLDEN * ((row & _U(0xFFFFFFFF)) * _U(0x100000001) + (step & _U(0xFFFFFFFF)) + _U(1))
        z = (z ^ (z >> _U(30))) * _U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _U(27))) * _U(0x94D049BB133111EB)
        return z ^ (z >> _U(31))


def uniform01(seed, row, step) -> np.ndarray:
    """uniform01 of csrc/common.hpp, bit for bit: ((z >> 40) + 0.5 in double) rounded to fp32, times 2^-24."""
    n = (rng_mix64(seed, row, step) >> _U(40)).astype(np.float64)
    return (n + 0.5).astype(np.float32) * np.float32(1.0 / 16777216.0)


def beam_uniform(seed: int, row, column: int, n_flat: int) -> np.ndarray:
    """u of every flat index beam * V + id of the chunks with RNG rows `row` (rng_row0 + chunk) at decode column `column`:
    fp32 (len(row), n_flat).  The folding: (seed, row, column) -> a 64-bit sub-seed; the flat index is the step of row 0 under it."""
    sub = rng_mix64(seed, np.atleast_1d(np.asarray(row, dtype=_U)), column)
    return uniform01(sub[:, None], 0, np.arange(n_flat, dtype=_U)[None, :])


def gumbel(u: np.ndarray, dtype=np.float64) -> np.ndarray:
    u = np.minimum(u.astype(np.float32), U_MAX).astype(dtype)
    return -np.log(-np.log(u))


def hf_warp_mask(x: np.ndarray, top_k: int, top_p: float, keep: int) -> np.ndarray:
    """HF TopKLogitsWarper then TopPLogitsWarper on one row, element by element (stable ascending sort): True = removed."""
    V = x.size
    removed = np.zeros(V, dtype=bool)
    if top_k > 0:
        kk = min(max(int(top_k), keep), V)
        removed |= x < np.sort(x)[V - kk]
    if top_p < 1.0:
        y = np.where(removed, -np.inf, x)
        order = np.argsort(y, kind="stable")
        e = np.exp(y[order] - y.max())
        drop = np.cumsum(e / e.sum()) <= 1.0 - float(np.float32(top_p))
        drop[V - min(keep, V):] = False
        removed[order] |= drop
    return removed


def row_cut(x: np.ndarray, top_k: int, top_p: float, keep: int):
    """The library's rule on one row of processed scores x (fp64): -> (cut value, distance of the nearest group boundary's mass
    from 1 - top_p).  An id stays iff x >= cut; groups of equal values stay or go whole."""
    V = x.size
    keep = min(int(keep), V)
    srt = np.sort(x)
    cut_k = srt[V - min(max(int(top_k), keep), V)] if top_k > 0 else -np.inf
    if not top_p < 1.0:
        return cut_k, np.inf
    live = (x >= cut_k) & np.isfinite(x)
    vals, inv = np.unique(x[live], return_inverse=True)                   # ascending
    e = np.exp(x[live] - vals[-1])
    mass = np.cumsum(np.bincount(inv, weights=e / e.sum()))               # M(v): mass of the ids with value <= v
    drop = 1.0 - float(np.float32(top_p))
    above = np.nonzero(mass > drop)[0]
    cut_p = vals[above[0]] if above.size else -np.inf
    return max(cut_k, min(cut_p, srt[V - keep])), float(np.abs(mass - drop).min())


def warped_scores(x: np.ndarray, rs: np.ndarray, top_k: int, top_p: float, keep: int):
    """x (rows, V) processed scores, rs (rows,) running scores -> (acc (rows, V) with -inf where removed, smallest boundary margin,
    whether HF's element-wise warpers remove exactly the same ids)."""
    acc = np.full(x.shape, -np.inf)
    margin, same = np.inf, True
    for r in range(x.shape[0]):
        cut, m = row_cut(x[r].astype(np.float64), top_k, top_p, keep)
        stay = x[r] >= cut
        acc[r, stay] = x[r, stay].astype(np.float64) + float(rs[r])
        margin = min(margin, m)
        same &= bool(np.array_equal(~stay, hf_warp_mask(x[r].astype(np.float64), top_k, top_p, keep)))
    return acc, margin, same


def draw(acc_flat: np.ndarray, u_flat: np.ndarray, K: int, dtype=np.float64):
    """One chunk: acc of the flat indices, their u -> (the K drawn flat indices in draw order, the best K + 1 keys): descending key,
    ties by ascending flat index."""
    key = acc_flat.astype(dtype) + gumbel(u_flat, dtype)
    order = np.lexsort((np.arange(key.size), -key))
    return order[:K], key[order[:K + 1]]


def deciding_gap(keys: np.ndarray, K: int, nb: int) -> float:
    """keys: one chunk's keys, best first (at least K + 1 of them where there are more than K).  The smallest gap between two
    adjacent keys that decides what a step keeps of the draw: among the first nb + 1 (the order inside the top num_beams) and
    between the K-th and the (K + 1)-th (membership in the K; the order of the draws behind the top num_beams is never read).
    Pairs whose lower key is -inf or a dead beam's (-1e9 to within an fp32 ulp of 64: exact ties in any form, broken by flat index)
    are left out."""
    pairs = [(i, i + 1) for i in range(nb)] + ([(K - 1, K)] if K < len(keys) else [])
    gaps = [float(keys[a]) - float(keys[b]) for a, b in pairs if b < len(keys) and keys[b] > -1.0e8]
    return min(gaps) if gaps else float("inf")


CHI2_999 = {10: 29.588, 109: 160.372}            # 99.9 % quantiles of chi-square for the cell counts the tests below reach


def plackett_luce_chi2(acc_flat: np.ndarray, draws: np.ndarray):
    """draws (trials, >= 2) flat indices in draw order against sequential sampling without replacement from softmax(acc_flat):
    -> ((chi-square, degrees of freedom) of the first draw, the same of the ordered pair (first, second)).  Cells with an
    expectation below 5 are pooled into one; an id with -inf score must never be drawn (asserted)."""
    n = draws.shape[0]
    w = np.where(np.isfinite(acc_flat), np.exp(acc_flat - acc_flat[np.isfinite(acc_flat)].max()), 0.0)
    W = w.sum()
    live = np.nonzero(w > 0)[0]
    assert np.isin(draws[:, :2], live).all(), "a removed id was drawn"
    first = np.bincount(draws[:, 0], minlength=w.size)
    pair = np.zeros((w.size, w.size))
    np.add.at(pair, (draws[:, 0], draws[:, 1]), 1)

    def stat(obs, exp):
        small = exp < 5
        chi, cells = float((((obs - exp) ** 2) / exp)[~small].sum()), int((~small).sum())
        if small.any():
            chi, cells = chi + float((obs[small].sum() - exp[small].sum()) ** 2 / exp[small].sum()), cells + 1
        return chi, cells - 1
    e1 = n * w[live] / W
    ij = [(i, j) for i in live for j in live if i != j]
    e2 = np.array([n * w[i] / W * w[j] / (W - w[i]) for i, j in ij])
    o2 = np.array([pair[i, j] for i, j in ij])
    return stat(first[live].astype(np.float64), e1), stat(o2, e2)


# the distribution case of the tests: 2 beams x 6 ids, one id masked, K = 4, 16 384 chunks as trials (processed scores, running scores)
PL_X = np.array([[-1.2, -0.3, -2.5, -0.9, -1.7, -3.0], [-0.8, -2.2, -1.1, -np.inf, -1.9, -0.6]])
PL_RS = np.array([-0.4, -1.1])
PL_SEED, PL_COLUMN, PL_TRIALS, PL_K = 1234, 5, 16384, 4
