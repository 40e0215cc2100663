"""Consensus (minimum-Bayes-risk) choice among candidate captions: the CPU statement of the rule (numpy, no GPU).

``conette_consensus`` (include/conette_hip.h, csrc/dec_consensus.h) computes exactly this rule on the device; ``select_fp32``
follows its arithmetic step by step, so the device results are compared bit for bit.

Per clip: N candidates (1 <= N <= ``MAX_CANDS``) as rows of ``preds`` (N, L) int32, 1 <= L <= ``MAX_PRED``, ids anywhere in
0 .. 2**31 - 1; optionally ``lens`` (N,) with 0 <= len <= L as ``sample`` reports them (<eos> included), and ``weights`` (N,).

* content of a candidate: with ``lens``, ``row[:len]`` without its last token if that token is ``eos_id``; without, the tokens in
  front of the first ``eos_id`` or ``pad_id`` of the row (the whole row if neither occurs).  A content may be empty.
* pair utility u(i, j), symmetric, in [0, 1], u(i, i) = 1:
    ``"ngram"`` with ``max_order`` n_max in 1 .. 4: for every order n = 1 .. n_max, t_i = max(|c_i| - n + 1, 0); an order with
    t_i + t_j = 0 does not count; otherwise m_n = the clipped match, the sum over distinct n-grams g of min(count_i(g), count_j(g)),
    and F_n = 2 m_n / (t_i + t_j); u = the mean of F_n over the orders that count, 1 when none counts (both contents empty).
    ``"edit"``: u = 1 - lev(c_i, c_j) / max(|c_i|, |c_j|), lev the Levenshtein distance over tokens at unit costs; 1 when both
    contents are empty.
* evidence weights: finite and > 0, normalised to sum 1 in float64 and handed over as fp32; ``None``: every weight fp32(1 / N).
* choice: E_i = sum_j w_j u(i, j) over all j, i included; ``best`` = the first index of the maximum; ``margin`` = E_best minus the
  largest E at any other index: +inf when N = 1, 0 when a duplicate ties.

The device arithmetic is part of the rule: counts and distances are exact integers; F_n is ONE correctly rounded fp32 division of
the two converted integers 2 m_n and t_i + t_j; the F_n are added in ascending n, each addition rounded, and the sum is divided
once by the number of counted orders; ``"edit"`` is one division and one subtraction from 1; E_i starts at 0 and takes, for
j = 0 .. N - 1 in order, the separately rounded product w_j u(i, j) (no fused multiply-add).  The fp32 rule stays within
73 * 2**-24 < 2**-17 of the float64 one on E: at most 8 roundings of values <= 1 per u, 64 products and 63 additions of 2**-24 each.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

MAX_CANDS = 64      # CONETTE_MAX_CANDS
MAX_PRED = 64       # CN_MAX_PRED
MAX_ORDER = 4
UTILITY = {"ngram": 0, "edit": 1}     # CONETTE_UTILITY_*


def check_arguments(preds, lens=None, weights=None, utility: str = "ngram", max_order: int = 4) -> Tuple[np.ndarray, int]:
    """(the weights normalised to sum 1, float64, of ``preds``' leading shape; the utility's code); ValueError for what
    conette_consensus refuses.  ``preds`` (..., N, L); ``lens`` / ``weights`` (..., N) or None (``weights`` None: equal weights)."""
    shape = tuple(np.shape(preds))
    if len(shape) < 2:
        raise ValueError(f"preds of shape {shape}: expected (..., n_cands, row_len)")
    n, l = shape[-2], shape[-1]
    if not 1 <= n <= MAX_CANDS:
        raise ValueError(f"n_cands={n} unsupported (1..{MAX_CANDS})")
    if not 1 <= l <= MAX_PRED:
        raise ValueError(f"row_len={l} unsupported (1..{MAX_PRED})")
    if utility not in UTILITY:
        raise ValueError(f"utility={utility!r} unknown (expected one of {tuple(UTILITY)})")
    if int(max_order) != max_order or not 1 <= int(max_order) <= MAX_ORDER:
        raise ValueError(f"max_order={max_order} unsupported (1..{MAX_ORDER})")
    if lens is not None:
        ln = np.asarray(lens)
        if tuple(ln.shape) != shape[:-1]:
            raise ValueError(f"lens of shape {tuple(ln.shape)} for preds of shape {shape}")
        if ln.size and (ln.min() < 0 or ln.max() > l):
            raise ValueError(f"lens must lie in 0..row_len={l} (found {int(ln.min())}..{int(ln.max())})")
    if weights is None:
        w = np.ones(shape[:-1], dtype=np.float64)
    else:
        w = np.asarray(weights, dtype=np.float64)
        if tuple(w.shape) != shape[:-1]:
            raise ValueError(f"weights of shape {tuple(w.shape)} for preds of shape {shape}")
        if not (np.isfinite(w).all() and (w > 0).all()):
            raise ValueError("weights must be finite and > 0")
    return w / w.sum(axis=-1, keepdims=True), UTILITY[utility]


def content(row: Sequence[int], length: Optional[int] = None, eos_id: int = 2, pad_id: int = 0) -> List[int]:
    """The tokens of a candidate that count."""
    row = [int(t) for t in row]
    if length is not None:
        c = row[:int(length)]
        return c[:-1] if c and c[-1] == eos_id else c
    for k, t in enumerate(row):
        if t == eos_id or t == pad_id:
            return row[:k]
    return row


def contents(preds, lens=None, eos_id: int = 2, pad_id: int = 0) -> List[List[int]]:
    preds = np.asarray(preds)
    return [content(preds[i], None if lens is None else int(np.asarray(lens)[i]), eos_id, pad_id) for i in range(preds.shape[0])]


def ngram_match(ci: Sequence[int], cj: Sequence[int], n: int) -> Tuple[int, int]:
    """(the clipped match m_n, t_i + t_j) of order n."""
    ti, tj = max(len(ci) - n + 1, 0), max(len(cj) - n + 1, 0)
    cnt: Dict[tuple, int] = {}
    for a in range(tj):
        g = tuple(cj[a:a + n])
        cnt[g] = cnt.get(g, 0) + 1
    m = 0
    for a in range(ti):
        g = tuple(ci[a:a + n])
        if cnt.get(g, 0) > 0:
            cnt[g] -= 1
            m += 1
    return m, ti + tj


def levenshtein(ci: Sequence[int], cj: Sequence[int]) -> int:
    prev = list(range(len(cj) + 1))
    for a, x in enumerate(ci, 1):
        cur = [a]
        for b, y in enumerate(cj, 1):
            cur.append(min(prev[b] + 1, cur[b - 1] + 1, prev[b - 1] + (x != y)))
        prev = cur
    return prev[-1]


def utility(ci: Sequence[int], cj: Sequence[int], kind: str = "ngram", max_order: int = 4) -> float:
    """u(i, j) in float64 from two contents."""
    if kind == "edit":
        big = max(len(ci), len(cj))
        return 1.0 if big == 0 else 1.0 - levenshtein(ci, cj) / big
    if kind != "ngram":
        raise ValueError(f"utility={kind!r} unknown (expected one of {tuple(UTILITY)})")
    total, counted = 0.0, 0
    for n in range(1, int(max_order) + 1):
        m, t = ngram_match(ci, cj, n)
        if t > 0:
            total += 2.0 * m / t
            counted += 1
    return 1.0 if counted == 0 else total / counted


# The integers of the rule for ALL pairs of a clip's contents at once (numpy over the pairs): what ``select`` and ``select_fp32`` run
# on.  They give the numbers ``ngram_match`` and ``levenshtein`` give pair by pair, which the tests hold them to.
def ngram_matches(cs: Sequence[Sequence[int]], max_order: int = 4) -> Tuple[np.ndarray, np.ndarray]:
    """(m_n (n_max, N, N), t_i + t_j (n_max, N, N))"""
    n = len(cs)
    ln = np.asarray([len(c) for c in cs], dtype=np.int64)
    match = np.zeros((int(max_order), n, n), dtype=np.int64)
    total = np.zeros((int(max_order), n, n), dtype=np.int64)
    for o in range(1, int(max_order) + 1):
        t = np.maximum(ln - o + 1, 0)
        total[o - 1] = t[:, None] + t[None, :]
        ids: Dict[tuple, int] = {}
        grams = [[ids.setdefault(tuple(c[a:a + o]), len(ids)) for a in range(int(t[i]))] for i, c in enumerate(cs)]
        counts = np.zeros((n, max(len(ids), 1)), dtype=np.int64)
        for i, g in enumerate(grams):
            np.add.at(counts[i], g, 1)
        for i in range(n):
            match[o - 1, i] = np.minimum(counts[i][None, :], counts).sum(axis=1)
    return match, total


def levenshtein_all(cs: Sequence[Sequence[int]]) -> Tuple[np.ndarray, np.ndarray]:
    """(lev (N, N), max(|c_i|, |c_j|) (N, N)): row a of every pair's table from row a - 1; the insertion chain inside a row is a
    running minimum"""
    n = len(cs)
    ln = np.asarray([len(c) for c in cs], dtype=np.int64)
    width = max(int(ln.max()), 1)
    tok = np.full((n, width), -1, dtype=np.int64)
    for i, c in enumerate(cs):
        tok[i, :len(c)] = c
    cols = np.arange(width + 1, dtype=np.int64)
    prev = np.broadcast_to(cols, (n, n, width + 1)).copy()       # row 0: the column index
    for a in range(width):
        differ = (tok[:, a][:, None, None] != tok[None, :, :]).astype(np.int64)      # (N, N, width): c_i[a] against c_j[b - 1]
        step = np.empty_like(prev)
        step[:, :, 0] = a + 1
        step[:, :, 1:] = np.minimum(prev[:, :, 1:] + 1, prev[:, :, :-1] + differ)
        cur = np.minimum.accumulate(step - cols, axis=2) + cols
        prev = np.where((a < ln)[:, None, None], cur, prev)      # (pairs whose c_i has ended keep their last row)
    lev = np.take_along_axis(prev, np.broadcast_to(ln[None, :, None], (n, n, 1)), axis=2)[:, :, 0]
    return lev, np.maximum(ln[:, None], ln[None, :])


def _pairwise(cs: Sequence[Sequence[int]], kind: str, max_order: int, dtype) -> np.ndarray:
    """u (N, N) in ``dtype`` arithmetic, every operation rounded on its own in the order the rule fixes"""
    f = dtype
    with np.errstate(invalid="ignore", divide="ignore"):
        if kind == "edit":
            lev, big = levenshtein_all(cs)
            return np.where(big == 0, f(1.0), f(1.0) - lev.astype(f) / big.astype(f)).astype(f)
        match, both = ngram_matches(cs, max_order)
        n = len(cs)
        total, counted = np.zeros((n, n), dtype=f), np.zeros((n, n), dtype=np.int64)
        for o in range(int(max_order)):
            counts = both[o] > 0
            fo = ((2 * match[o]).astype(f) / both[o].astype(f)).astype(f)
            total = np.where(counts, (total + fo).astype(f), total)
            counted += counts
        return np.where(counted == 0, f(1.0), total / counted.astype(f)).astype(f)


def _choose(e: np.ndarray) -> Tuple[int, float]:
    best = int(np.argmax(e))        # (the first maximum)
    others = np.delete(e, best)
    return best, (float("inf") if others.size == 0 else e[best] - others.max())


def expected(pairwise, weights) -> np.ndarray:
    """E (N,) float64 from u (N, N) and normalised weights (N,), added in the order j = 0 .. N - 1."""
    u, w = np.asarray(pairwise, dtype=np.float64), np.asarray(weights, dtype=np.float64)
    e = np.zeros(u.shape[0], dtype=np.float64)
    for j in range(u.shape[1]):
        e += w[j] * u[:, j]
    return e


def device_weights(n: int, weights, as_given: bool = False) -> np.ndarray:
    """What the device reads: fp32 of the float64-normalised weights (None: fp32(1) / fp32(N)); ``as_given``: the weights are
    those fp32 values already and are used as they are."""
    if weights is None:
        return np.full(n, np.float32(1.0) / np.float32(n), dtype=np.float32)
    if as_given:
        return np.asarray(weights, dtype=np.float32)
    w = np.asarray(weights, dtype=np.float64)
    return (w / w.sum()).astype(np.float32)


def select(preds, lens=None, weights=None, utility: str = "ngram", max_order: int = 4, eos_id: int = 2,
           pad_id: int = 0, as_given: bool = False) -> Dict[str, object]:
    """The rule in float64 for one clip: {"pairwise" (N, N), "expected" (N,), "best", "margin"}.  The weights are the fp32 values
    the device sees (``device_weights``), taken to float64."""
    check_arguments(preds, lens, weights, utility, max_order)
    cs = contents(preds, lens, eos_id, pad_id)
    n = len(cs)
    u = _pairwise(cs, utility, max_order, np.float64)
    e = expected(u, device_weights(n, weights, as_given).astype(np.float64))
    best, margin = _choose(e)
    return {"pairwise": u, "expected": e, "best": best, "margin": float(margin)}


def select_fp32(preds, lens=None, weights=None, utility: str = "ngram", max_order: int = 4, eos_id: int = 2,
                pad_id: int = 0, as_given: bool = False) -> Dict[str, object]:
    """The rule with the device's arithmetic (numpy.float32, every operation rounded on its own) for one clip: the same keys,
    fp32 arrays, ``margin`` a numpy.float32."""
    check_arguments(preds, lens, weights, utility, max_order)
    cs = contents(preds, lens, eos_id, pad_id)
    n = len(cs)
    u = _pairwise(cs, utility, max_order, np.float32)
    w = device_weights(n, weights, as_given)
    e = np.zeros(n, dtype=np.float32)
    for j in range(n):
        e = (e + (w[j] * u[:, j]).astype(np.float32)).astype(np.float32)
    best, margin = _choose(e)
    return {"pairwise": u, "expected": e, "best": best, "margin": np.float32(margin)}


def select_batch(preds, lens=None, weights=None, fp32: bool = False, **kw) -> Dict[str, np.ndarray]:
    """``select`` (``select_fp32`` with ``fp32``) over a batch (B, N, L): stacked arrays."""
    preds = np.asarray(preds)
    fn = select_fp32 if fp32 else select
    rs = [fn(preds[b], None if lens is None else np.asarray(lens)[b], None if weights is None else np.asarray(weights)[b], **kw)
          for b in range(preds.shape[0])]
    dt = np.float32 if fp32 else np.float64
    return {"pairwise": np.stack([r["pairwise"] for r in rs]), "expected": np.stack([r["expected"] for r in rs]),
            "best": np.asarray([r["best"] for r in rs], dtype=np.int32), "margin": np.asarray([r["margin"] for r in rs], dtype=dt)}
