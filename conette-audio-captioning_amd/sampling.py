"""Sampling semantics: the CPU restatement of one sampling decision and of a whole sampled caption (float64 numpy, no GPU).

``conette_sample`` (include/conette_hip.h, csrc/dec_sample.h) computes exactly this rule in fp32 on the device; the tests replay
its decisions through the functions below.  One decision takes a row's logits ``z`` (V), the row's prefix (the task token at
position 0 included), ``step`` and a uniform ``u`` in [0, 1):

1. masks, as the searches apply them: ``z[eos] = -inf`` while ``step < min_pred``; ``z[v] = -inf`` for every ``v`` with
   ``forbid[v]`` set that already occurs in the prefix;
2. the reported log-probability is ``log_softmax(z_masked)[token]``: temperature 1, unfiltered -- what the beam search sums;
3. ``y = z_masked / temperature``;
4. top-k: ``v`` is kept iff fewer than ``top_k`` tokens have a strictly larger ``y`` (``top_k`` 0 or >= V: off);
5. top-p: with ``q = softmax(y over the top-k set)``, ``v`` is kept iff the total ``q`` of the tokens with strictly larger ``y`` is
   ``< top_p`` (``top_p`` 1: off).  Both rules are tie-inclusive and always keep the arg-max; a token of probability zero
   (``y = -inf``) is never kept;
6. draw: ``q`` renormalised over the kept set, walked in ascending token id: the first token whose running sum exceeds ``u``, or
   the largest kept id when rounding leaves the total ``<= u``.

A row finishes when it draws ``<eos>`` or at step ``max_pred - 1`` (the drawn token stays); later positions hold ``pad_id`` and add
no log-probability.  A row without a finite logit takes ``<eos>``, its log-probability becomes NaN, and it finishes.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

MAX_SAMPLES_PER_CALL = 16   # CN_MAX_BEAM: rows per clip of one conette_sample call


def masked_logits(z, prefix: Sequence[int], step: int, min_pred: int, eos_id: int, forbid=None) -> np.ndarray:
    """Rule 1: the float64 logits with the EOS floor and the forbid-repeat mask applied (a copy)."""
    z = np.array(z, dtype=np.float64).reshape(-1)
    if step < min_pred:
        z[eos_id] = -np.inf
    if forbid is not None:
        fb = np.asarray(forbid).astype(bool).reshape(-1)
        for t in prefix:
            if fb[int(t)]:
                z[int(t)] = -np.inf
    return z


def log_softmax(z: np.ndarray) -> np.ndarray:
    m = np.max(z)
    if not np.isfinite(m):
        return np.full_like(z, np.nan)
    return (z - m) - np.log(np.sum(np.exp(z - m)))


def _mass_above(y: np.ndarray, q: np.ndarray) -> np.ndarray:
    """for every v: the total q of the tokens with strictly larger y"""
    order = np.argsort(-y, kind="stable")
    ys, cs = y[order], np.cumsum(q[order])
    first = np.searchsorted(-ys, -ys, side="left")          # start of each tie group
    above_sorted = np.where(first > 0, cs[np.maximum(first - 1, 0)], 0.0)
    out = np.empty_like(above_sorted)
    out[order] = above_sorted
    return out


def keep_mask(y, top_k: int = 0, top_p: float = 1.0) -> np.ndarray:
    """Rules 4 and 5 on the tempered logits ``y``: (V,) bool."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    v = y.shape[0]
    keep = y > -np.inf
    if not keep.any():
        return keep
    if 0 < int(top_k) < v:
        larger = _mass_above(y, np.ones(v))                  # number of strictly larger tokens
        keep &= larger < int(top_k)
    if top_p < 1.0:
        m = np.max(y[keep])
        q = np.where(keep, np.exp(y - m), 0.0)
        q = q / q.sum()
        keep &= _mass_above(np.where(keep, y, -np.inf), q) < top_p
    return keep


def keep_masks(y, top_k: int = 0, top_p: float = 1.0) -> np.ndarray:
    """``keep_mask`` for N rows at once: (N, V) tempered logits -> (N, V) bool.  Rows without a finite entry keep nothing."""
    y = np.asarray(y, dtype=np.float64)
    n, v = y.shape
    keep = y > -np.inf
    if 0 < int(top_k) < v:
        kth = -np.partition(-y, int(top_k) - 1, axis=1)[:, int(top_k) - 1:int(top_k)]    # the k-th largest value, with multiplicity
        keep &= y >= kth
    if top_p < 1.0:
        yk = np.where(keep, y, -np.inf)
        m = yk.max(axis=1, keepdims=True)
        m = np.where(np.isfinite(m), m, 0.0)
        q = np.exp(yk - m)
        q = q / np.maximum(q.sum(axis=1, keepdims=True), np.finfo(np.float64).tiny)
        order = np.argsort(-yk, axis=1, kind="stable")
        ys, qs = np.take_along_axis(yk, order, axis=1), np.take_along_axis(q, order, axis=1)
        ex = np.zeros_like(qs)
        ex[:, 1:] = np.cumsum(qs, axis=1)[:, :-1]                        # mass in front of each sorted position
        start = np.ones((n, v), dtype=bool)
        start[:, 1:] = ys[:, 1:] != ys[:, :-1]                           # first of its tie group: `ex` there is the strictly larger mass
        above_sorted = np.maximum.accumulate(np.where(start, ex, -np.inf), axis=1)
        above = np.empty_like(above_sorted)
        np.put_along_axis(above, order, above_sorted, axis=1)
        keep &= above < top_p
    return keep


def kept_probs(z_masked, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0) -> np.ndarray:
    """Rules 3-6 up to the draw: the renormalised probabilities over the kept set (0 elsewhere); all 0 without a finite logit."""
    z = np.asarray(z_masked, dtype=np.float64).reshape(-1)
    y = z / float(temperature)
    keep = keep_mask(y, top_k, top_p)
    if not keep.any():
        return np.zeros_like(y)
    q = np.where(keep, np.exp(y - np.max(y[keep])), 0.0)
    return q / q.sum()


def draw(q: np.ndarray, keep: np.ndarray, u: float) -> int:
    """Rule 6: walk the kept set in ascending id."""
    ids = np.nonzero(keep)[0]
    c = np.cumsum(q[ids])
    hit = np.nonzero(c > float(u))[0]
    return int(ids[hit[0]] if hit.size else ids[-1])


def decide(z, prefix: Sequence[int], step: int, u: float, *, min_pred: int = 0, eos_id: int = 2, forbid=None,
           temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0) -> Tuple[int, float]:
    """One decision: (token, reported log-probability)."""
    zm = masked_logits(z, prefix, step, min_pred, eos_id, forbid)
    if not np.isfinite(zm).any():
        return int(eos_id), float("nan")
    y = zm / float(temperature)
    keep = keep_mask(y, top_k, top_p)
    q = kept_probs(zm, temperature, top_k, top_p)
    tok = draw(q, keep, u)
    return tok, float(log_softmax(zm)[tok])


def sample_rows(logits_fn: Callable[[int, List[int], int], np.ndarray], bos_ids: Sequence[int], uniforms, *, max_pred: int,
                min_pred: int = 0, eos_id: int = 2, pad_id: int = 0, forbid=None, temperature: float = 1.0, top_k: int = 0,
                top_p: float = 1.0) -> Dict[str, np.ndarray]:
    """Whole captions of R rows: ``logits_fn(row, prefix, step)`` stands in for the decoder, ``uniforms`` is (max_pred, R),
    step-major as conette_sample takes it.  Returns preds (R, max_pred), tok_lprobs, sum_lprobs, lens and sizes (2)."""
    uniforms = np.asarray(uniforms)
    rows = len(bos_ids)
    preds = np.full((rows, max_pred), pad_id, dtype=np.int64)
    tok_lp = np.zeros((rows, max_pred), dtype=np.float64)
    lens = np.zeros(rows, dtype=np.int64)
    for r in range(rows):
        prefix = [int(bos_ids[r])]
        for step in range(max_pred):
            tok, lp = decide(logits_fn(r, list(prefix), step), prefix, step, float(uniforms[step, r]), min_pred=min_pred,
                             eos_id=eos_id, forbid=forbid, temperature=temperature, top_k=top_k, top_p=top_p)
            preds[r, step], tok_lp[r, step] = tok, lp
            prefix.append(tok)
            if tok == eos_id or step == max_pred - 1:
                lens[r] = step + 1
                break
    longest = int(lens.max()) if rows else 0
    return {"preds": preds, "tok_lprobs": tok_lp, "sum_lprobs": tok_lp.sum(axis=1), "lens": lens,
            "sizes": np.array([longest, longest], dtype=np.int64)}


def plan_sample_chunks(n_samples: int, limit: int = MAX_SAMPLES_PER_CALL) -> List[Tuple[int, int]]:
    """(first sample, count) of the conette_sample calls that draw ``n_samples`` captions per clip: full calls of ``limit`` samples,
    then the remainder.  Sample j of the result is sample ``j - first`` of its call and reads column block ``first .. first + count``
    of the caller's (max_pred, batch, n_samples) uniforms."""
    n, limit = int(n_samples), int(limit)
    if n < 1 or limit < 1:
        raise ValueError(f"n_samples={n_samples} must be >= 1")
    return [(i, min(limit, n - i)) for i in range(0, n, limit)]
