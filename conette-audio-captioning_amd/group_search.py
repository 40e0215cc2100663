"""Diverse beam search semantics: the CPU restatement of one group's top-k call and of a whole search (float64 numpy, no GPU).

``conette_decode_groups`` (include/conette_hip.h, csrc/dec_group.h) computes exactly this rule in fp32 on the device; the tests
replay its calls through ``decide_group`` and compare whole searches with ``group_search``.

Parameters: ``n_groups`` G >= 1, ``group_beam`` W >= 1, G * W <= 16, ``diversity_penalty`` lambda finite and >= 0.  Clip b owns
rows ``b * G * W ..``; group g owns rows ``g * W .. g * W + W - 1`` of the clip, its ``k_g`` live rows (W at the start) compacted
to the front of its own range.  One step ``i`` of a clip goes through g = 0 .. G - 1 in this order:

* a group with ``k_g == 0`` takes no picks and adds nothing to the counts;
* candidates: the group's live rows (step 0: its first row only); logits masked as the plain searches mask them (EOS floor while
  ``i < min_pred``, forbid-repeat over the row's own prefix, position 0 included); ``lp = log_softmax`` of the masked row;
* model score ``m(p, v) = sum_lp[p] + lp[p][v]`` (step 0: ``lp``);
* ``c[v]`` = the number of picks made at this step by groups 0 .. g - 1 of this clip whose token is v (every pick counts,
  finishing ones included);
* key ``s(p, v) = m`` if ``c[v] == 0``, else ``m - lambda * c[v]``;
* picks: the top ``k_g`` keys over the group's ``k_g * V`` candidates, ties to the lowest flat index ``p * V + v``;
* a pick carries its model score ``m``, never its key;
* bookkeeping per group as the plain search's: a pick of ``<eos>``, or any pick at step ``max_pred - 1``, goes to output slot
  ``g * W + slot`` with score ``m / (i + 1)`` and leaves; the others continue, in pick order, with a smaller ``k_g``.

At the end ``mult_preds`` / ``mult_lprobs`` are (B, G * W, .) in slot order, group-major, and ``best_*`` is the first maximum of
the averaged score over all G * W slots.  With G = 1 this is the plain beam search at beam W for any lambda; group 0 is that
search for any G and lambda; with lambda = 0 every group is.
"""
from __future__ import annotations

import math
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from .sampling import log_softmax, masked_logits

MAX_ROWS_PER_CLIP = 16   # CN_MAX_BEAM: n_groups * group_beam of one conette_decode_groups call


def check_arguments(n_groups: int, group_beam: int, diversity_penalty: float) -> Tuple[int, int]:
    """(G, W) as ints; ValueError for what conette_decode_groups refuses."""
    g, w = int(n_groups), int(group_beam)
    if g != n_groups or w != group_beam or g < 1 or w < 1 or g * w > MAX_ROWS_PER_CLIP:
        raise ValueError(f"n_groups={n_groups} x group_beam={group_beam} unsupported (both >= 1, product <= {MAX_ROWS_PER_CLIP})")
    lam = float(diversity_penalty)
    if not (math.isfinite(lam) and lam >= 0.0):
        raise ValueError(f"diversity_penalty={diversity_penalty} must be finite and >= 0")
    return g, w


def decide_group(logits, prefixes: Sequence[Sequence[int]], sums: Sequence[float], counts, k: int, step: int,
                 diversity_penalty: float, min_pred: int, eos_id: int = 2, forbid=None) -> Dict[str, object]:
    """One group's call.  ``logits`` (n, V): the raw logits of the group's candidate rows (n = 1 at step 0, else n = k);
    ``prefixes`` / ``sums``: their prefixes (the task token first) and running sums; ``counts`` (V,): picks of this step by the
    earlier groups of the clip, per token.  Returns parents (row within the group), tokens, the carried model scores ``sums``,
    the selection ``keys`` (all in pick order), and the effective ``margin``: the smallest of the last pick's key minus the
    first rejected key and the gaps between consecutive picks' keys."""
    z = np.asarray(logits, dtype=np.float64)
    n, v = z.shape
    assert n == (1 if step == 0 else k) and len(prefixes) >= n
    c = np.asarray(counts, dtype=np.float64).reshape(-1)
    m = np.empty((n, v), dtype=np.float64)
    for p in range(n):
        lp = log_softmax(masked_logits(z[p], prefixes[p][: step + 1], step, min_pred, eos_id, forbid))
        m[p] = lp if step == 0 else float(sums[p]) + lp
    key = np.where(c[None, :] == 0, m, m - float(diversity_penalty) * c[None, :]).reshape(-1)
    order = np.argsort(-key, kind="stable")[: k + 1]          # stable: ties go to the lowest flat index
    picks = order[:k]
    keys = key[picks]
    gaps = [float(keys[j] - keys[j + 1]) for j in range(k - 1)]
    if order.shape[0] > k:
        gaps.append(float(keys[k - 1] - key[order[k]]))
    return {"parents": (picks // v).tolist(), "tokens": (picks % v).tolist(), "sums": m.reshape(-1)[picks].tolist(),
            "keys": keys.tolist(), "margin": min(gaps) if gaps else float("inf")}


def unpenalised_picks(logits, prefixes, sums, k: int, step: int, min_pred: int, eos_id: int = 2, forbid=None) -> List[Tuple[int, int]]:
    """The (parent, token) pairs the same call picks without a penalty: what a penalised call is compared with."""
    v = np.asarray(logits).shape[1]
    d = decide_group(logits, prefixes, sums, np.zeros(v), k, step, 0.0, min_pred, eos_id, forbid)
    return list(zip(d["parents"], d["tokens"]))


def finalize(out_preds: np.ndarray, out_avg: np.ndarray, out_len: np.ndarray, eos_id: int = 2):
    """best_preds (B, max_pred), best_lprobs (B,), sizes [pred_size, best_maxlen] from the filled slots, as the plain search ends:
    the first maximum of the averaged score; pred_size = the longest hypothesis; best_maxlen = the longest best caption."""
    b, _, maxp = out_preds.shape
    best = np.argmax(out_avg, axis=1)                        # first maximum
    best_preds = out_preds[np.arange(b), best]
    ps = int(out_len.max())
    m = 0
    for i in range(b):
        e = np.nonzero(best_preds[i] == eos_id)[0]
        m = max(m, int(e[0]) if e.size and int(e[0]) < ps else ps)
    return best_preds, out_avg[np.arange(b), best], [ps, min(m + 1, ps)]


def group_search(logits_fn: Callable[[List[Tuple[int, List[int]]], int], np.ndarray], bos_ids: Sequence[int], n_groups: int,
                 group_beam: int, diversity_penalty: float, min_pred: int, max_pred: int, vocab_size: int, eos_id: int = 2,
                 pad_id: int = 0, forbid=None) -> Dict[str, object]:
    """The whole search.  ``logits_fn(rows, step)`` stands in for the decoder: ``rows`` is the list of (clip, prefix) of every
    live row, clips ascending, groups ascending inside a clip, rows in their order inside a group; it returns their (N, V) logits
    of position ``step``.  Returns mult_preds (B, G * W, max_pred), mult_lprobs, lens, best_preds, best_lprobs, sizes, and
    ``calls``: one dict per (step, clip, group) that took picks -- step, clip, group, k, parents (within the group), tokens,
    sums (carried), keys, margin, counts (token -> count before the call), plain (the picks of the same call without a penalty)."""
    g_n, w_n = check_arguments(n_groups, group_beam, diversity_penalty)
    b_n, gw = len(bos_ids), g_n * w_n
    # live rows of (clip, group): dicts of prefix, sum, slot -- W identical rows at the start
    live = [[[{"prefix": [int(bos_ids[b])], "sum": 0.0, "slot": g * w_n + j} for j in range(w_n)] for g in range(g_n)]
            for b in range(b_n)]
    out_preds = np.full((b_n, gw, max_pred), pad_id, dtype=np.int64)
    out_avg = np.zeros((b_n, gw), dtype=np.float64)
    out_len = np.zeros((b_n, gw), dtype=np.int64)
    calls: List[dict] = []
    for step in range(max_pred):
        rows = [(b, r["prefix"]) for b in range(b_n) for g in range(g_n) for r in live[b][g]]
        if not rows:
            break
        logits = np.asarray(logits_fn(rows, step), dtype=np.float64)
        at = 0
        for b in range(b_n):
            counts = np.zeros(vocab_size, dtype=np.int64)
            for g in range(g_n):
                grp = live[b][g]
                k = len(grp)
                if k == 0:
                    continue
                z = logits[at:at + k]
                at += k
                n = 1 if step == 0 else k
                prefixes, sums = [r["prefix"] for r in grp], [r["sum"] for r in grp]
                d = decide_group(z[:n], prefixes, sums, counts, k, step, diversity_penalty, min_pred, eos_id, forbid)
                plain = unpenalised_picks(z[:n], prefixes, sums, k, step, min_pred, eos_id, forbid)
                calls.append({"step": step, "clip": b, "group": g, "k": k, "counts": {int(t): int(counts[t]) for t in np.nonzero(counts)[0]},
                              "plain": plain, **d})
                nxt = []
                for c in range(k):
                    parent, token, m = d["parents"][c], d["tokens"][c], d["sums"][c]
                    counts[token] += 1
                    seq = grp[parent]["prefix"] + [token]
                    if token == eos_id or step == max_pred - 1:
                        sl = grp[c]["slot"]
                        out_preds[b, sl, : step + 1] = seq[1:]
                        out_avg[b, sl] = m / (step + 1)
                        out_len[b, sl] = step + 1
                    else:
                        nxt.append({"prefix": seq, "sum": m, "slot": grp[c]["slot"]})
                live[b][g] = nxt
        assert at == logits.shape[0]
    best_preds, best_lprobs, sizes = finalize(out_preds, out_avg, out_len, eos_id)
    return {"mult_preds": out_preds, "mult_lprobs": out_avg, "lens": out_len, "best_preds": best_preds, "best_lprobs": best_lprobs,
            "sizes": sizes, "calls": calls}
