"""Ensemble beam search semantics: the CPU restatement of one top-k call and of a whole search (float64 numpy, no GPU).

``conette_decode_ensemble`` (include/conette_hip.h, csrc/dec_ensemble.h) computes exactly this rule in fp32 on the device; the tests
replay its calls through ``decide`` and compare whole searches with ``ensemble_search``.

Members m = 0 .. M - 1, 1 <= M <= 4: each a decoder with its own task (BOS) token per clip, its own audio memory and a weight
``w_m``, finite and positive; the host normalises the weights to sum 1 in float64 (``check_arguments``) and hands them over as
fp32.  Shared: the frame lengths, the forbid mask, the beam W (1 .. 16), ``min_pred``, ``max_pred``, the vocabulary and the eos /
pad ids -- and ONE hypothesis tree: every member decodes the same prefixes, only position 0 differs, where member m sees its own
task token.  One call (a clip at a step, ``k`` live rows, at step 0 its first row only):

* per candidate row p and member m, ``lp_m(p, .)`` = log_softmax of member m's logits masked as the plain search masks them (EOS
  floor while ``step < min_pred``, forbid-repeat over the row's prefix with member m's own task token at position 0);
* combination: M = 1: ``c = lp_0``; ``"logprob"``: ``c(p, v) = sum_m w_m * lp_m(p, v)`` (a product of experts: -inf where any
  member is -inf); ``"prob"``: ``c(p, v) = log sum_m w_m * exp(lp_m(p, v))`` (a mixture: -inf only where every member is -inf,
  taken around the largest ``lp_m`` so that it does not underflow where some ``lp_m`` is finite);
* score ``sum[p] + c(p, v)`` (step 0: ``c``); the picks are the top ``k`` scores over the ``k * V`` candidates, ties to the lowest flat
  index ``p * V + v``; with fewer finite candidates than picks the remaining picks are -inf candidates in flat-index order;
* bookkeeping as the plain search's: a pick of ``<eos>``, or any pick at step ``max_pred - 1``, goes to the output slot of its row
  position with score / (step + 1) and leaves; the others continue, in pick order.  The reported scores are the combined ones.
"""
from __future__ import annotations

import math
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from .group_search import finalize
from .sampling import log_softmax, masked_logits

MAX_MEMBERS = 4     # CN_MAX_MEMBERS
MAX_BEAM = 16       # CN_MAX_BEAM
COMBINE = {"logprob": 0, "prob": 1}     # CONETTE_COMBINE_*


def check_arguments(n_members: int, weights: Optional[Sequence[float]], combine: str, beam: int) -> Tuple[np.ndarray, int]:
    """(the weights normalised to sum 1, float64 (M,); the rule's code); ValueError for what conette_decode_ensemble refuses.
    ``weights`` None: equal weights."""
    m = int(n_members)
    if m != n_members or m < 1 or m > MAX_MEMBERS:
        raise ValueError(f"n_members={n_members} unsupported (1..{MAX_MEMBERS})")
    if combine not in COMBINE:
        raise ValueError(f"combine={combine!r} unknown (expected one of {tuple(COMBINE)})")
    if int(beam) != beam or not 1 <= int(beam) <= MAX_BEAM:
        raise ValueError(f"beam={beam} unsupported (1..{MAX_BEAM})")
    w = np.ones(m, dtype=np.float64) if weights is None else np.asarray([float(x) for x in weights], dtype=np.float64)
    if w.shape != (m,):
        raise ValueError(f"weights: {w.size} given for {m} members")
    if not (np.isfinite(w).all() and (w > 0).all()):
        raise ValueError(f"weights={w.tolist()} must be finite and > 0")
    return w / w.sum(), COMBINE[combine]


def member_log_probs(logits, prefixes: Sequence[Sequence[int]], bos: Sequence[int], step: int, min_pred: int, eos_id: int = 2,
                     forbid=None) -> np.ndarray:
    """lp (M, n, V): ``logits`` (M, n, V) raw; ``prefixes`` the shared prefixes of the n rows; ``bos`` (M,) each member's token at
    position 0."""
    z = np.asarray(logits, dtype=np.float64)
    lp = np.empty_like(z)
    for m in range(z.shape[0]):
        for p in range(z.shape[1]):
            prefix = [int(bos[m])] + [int(t) for t in prefixes[p][1: step + 1]]
            lp[m, p] = log_softmax(masked_logits(z[m, p], prefix, step, min_pred, eos_id, forbid))
    return lp


def combine_log_probs(lp: np.ndarray, weights: Sequence[float], combine: str) -> np.ndarray:
    """c (n, V) from lp (M, n, V): the direct float64 formula of the rule."""
    lp = np.asarray(lp, dtype=np.float64)
    w = np.asarray(weights, dtype=np.float64).reshape(-1, 1, 1)
    if lp.shape[0] == 1:
        return lp[0].copy()
    with np.errstate(invalid="ignore", divide="ignore"):
        if combine == "logprob":
            return (w * lp).sum(axis=0)
        top = lp.max(axis=0)
        safe = np.where(np.isfinite(top), top, 0.0)
        return np.where(np.isfinite(top), safe + np.log((w * np.exp(lp - safe)).sum(axis=0)), -np.inf)


def decide(logits, prefixes: Sequence[Sequence[int]], bos: Sequence[int], sums: Sequence[float], weights: Sequence[float], combine: str,
           k: int, step: int, min_pred: int, eos_id: int = 2, forbid=None) -> Dict[str, object]:
    """One call.  ``logits`` (M, n, V): every member's raw logits of the clip's candidate rows (n = 1 at step 0, else n = k);
    ``prefixes`` / ``sums``: the rows' shared prefixes and running sums; ``bos`` (M,): the members' tokens at position 0;
    ``weights`` (M,) normalised.  Returns parents, tokens and the carried ``sums`` in pick order, and the effective ``margin``: the
    smallest of the last pick's score minus the first rejected score and the gaps between consecutive picks (NaN where a pick
    is not finite)."""
    z = np.asarray(logits, dtype=np.float64)
    m_n, n, v = z.shape
    assert n == (1 if step == 0 else k) and len(prefixes) >= n and len(bos) == m_n == len(weights)
    c = combine_log_probs(member_log_probs(z, prefixes, bos, step, min_pred, eos_id, forbid), weights, combine)
    score = (c if step == 0 else np.asarray(sums[:n], dtype=np.float64)[:, None] + c).reshape(-1)
    order = np.argsort(-score, kind="stable")[: k + 1]          # stable: ties go to the lowest flat index
    picks = order[:k]
    vals = score[picks]
    with np.errstate(invalid="ignore"):
        gaps = [float(vals[j] - vals[j + 1]) for j in range(k - 1)]
        if order.shape[0] > k:
            gaps.append(float(vals[k - 1] - score[order[k]]))
    margin = float("nan") if any(math.isnan(g) for g in gaps) else (min(gaps) if gaps else float("inf"))
    return {"parents": (picks // v).tolist(), "tokens": (picks % v).tolist(), "sums": vals.tolist(), "margin": margin}


def ensemble_search(logits_fns: Sequence[Callable[[List[Tuple[int, List[int]]], int], np.ndarray]], bos_ids: Sequence[Sequence[int]],
                    weights: Optional[Sequence[float]], combine: str, beam: int, min_pred: int, max_pred: int, vocab_size: int,
                    eos_id: int = 2, pad_id: int = 0, forbid=None) -> Dict[str, object]:
    """The whole search.  ``logits_fns[m](rows, step)`` stands in for member m's decoder: ``rows`` is the list of (clip, prefix) of
    every candidate row, clips ascending, rows in their order -- the prefix with member m's own task token first; it returns their
    (N, V) logits of position ``step``.  ``bos_ids`` (M, B).  Returns mult_preds (B, W, max_pred), mult_lprobs, lens, best_preds,
    best_lprobs, sizes, ``weights`` (normalised) and ``calls``: one dict per (step, clip) that took picks -- step, clip, k, parents,
    tokens, sums, margin."""
    m_n = len(logits_fns)
    w, _ = check_arguments(m_n, weights, combine, beam)
    bos = np.asarray(bos_ids, dtype=np.int64).reshape(m_n, -1)
    b_n = bos.shape[1]
    live = [[{"prefix": [int(bos[0, b])], "sum": 0.0, "slot": j} for j in range(beam)] for b in range(b_n)]
    out_preds = np.full((b_n, beam, max_pred), pad_id, dtype=np.int64)
    out_avg = np.zeros((b_n, beam), dtype=np.float64)
    out_len = np.zeros((b_n, beam), dtype=np.int64)
    calls: List[dict] = []
    for step in range(max_pred):
        cand = [(b, r["prefix"]) for b in range(b_n) for r in (live[b][:1] if step == 0 else live[b])]
        if not cand:
            break
        logits = np.stack([np.asarray(fn([(b, [int(bos[m, b])] + p[1:]) for b, p in cand], step), dtype=np.float64)
                           for m, fn in enumerate(logits_fns)])
        at = 0
        for b in range(b_n):
            rows = live[b]
            k = len(rows)
            if k == 0:
                continue
            n = 1 if step == 0 else k
            d = decide(logits[:, at:at + n], [r["prefix"] for r in rows], bos[:, b].tolist(), [r["sum"] for r in rows], w, combine, k, step,
                       min_pred, eos_id, forbid)
            at += n
            calls.append({"step": step, "clip": b, "k": k, **d})
            nxt = []
            for c in range(k):
                parent, token, s = d["parents"][c], d["tokens"][c], d["sums"][c]
                seq = rows[parent]["prefix"] + [token]
                if token == eos_id or step == max_pred - 1:
                    sl = rows[c]["slot"]
                    out_preds[b, sl, : step + 1] = seq[1:]
                    out_avg[b, sl] = s / (step + 1)
                    out_len[b, sl] = step + 1
                else:
                    nxt.append({"prefix": seq, "sum": s, "slot": rows[c]["slot"]})
            live[b] = nxt
        assert at == logits.shape[1]
    best_preds, best_lprobs, sizes = finalize(out_preds, out_avg, out_len, eos_id)
    return {"mult_preds": out_preds, "mult_lprobs": out_avg, "lens": out_len, "best_preds": best_preds, "best_lprobs": best_lprobs,
            "sizes": sizes, "weights": w, "calls": calls}
