"""Constrained beam search semantics: the CPU restatement of one call and of a whole search (float64 numpy, no GPU).

``conette_decode_constrained`` (include/conette_hip.h, csrc/dec_constrain.h) computes exactly this rule in fp32 on the device; the
tests replay its calls through ``decide`` and compare whole searches with ``constrained_search``.

Parameters: beam W in 1 .. 16; per clip a prefix of ``plen`` tokens (0 <= plen <= max_pred - 1; in [0, V), neither ``<eos>`` nor
pad); a ban mask over the vocabulary or None; ``no_repeat_ngram`` n in 0 (off) .. 64.  A row's sequence at step ``i`` is s_0 (the
task token), s_1 .. s_i; a candidate's token becomes s_{i+1}.

Masks on the raw logits ``z`` of a candidate row at step ``i`` (``constraint_mask``):

* M1: the plain searches' masks -- the EOS floor while ``i < min_pred``, forbid-repeat over s_0 .. s_i;
* M2: ``z[v] = -inf`` where the ban mask is set;
* M3 (n >= 1): for every j with 0 <= j <= i - n + 1 for which s_j .. s_{j+n-2} equals s_{i-n+2} .. s_i (n - 1 tokens; n = 1: always),
  ``z[s_{j+n-1}] = -inf``.  Position 0 takes part;
* ``lp = log_softmax`` of the masked row; model score ``m(p, v) = sum_lp[p] + lp[p][v]`` (step 0: ``lp``).

Calls of clip b at step i (``decide``):

* forced (i < plen): the only candidate is (row 0, t = prefix[i]).  m finite: row 0 goes on with t and carries m, the clip keeps its
  W live rows.  m not finite: all W slots of the clip become void and the clip leaves the search;
* fan-out (i == plen): candidates are the V tokens of row 0, k = W picks (plen 0: the plain search's step 0);
* later steps: the plain search's step over the k live rows;
* picks: the top k FINITE m, ties to the lowest flat index ``p * V + v``; with f < k finite candidates there are f picks and the
  slots of row positions f .. k - 1 become void;
* a void slot has score -inf, length 0 and pad throughout; ``best_*`` is the first maximum of the averaged score;
* bookkeeping as the plain search's: a pick of ``<eos>``, or any pick at step ``max_pred - 1``, goes to the slot of its row position
  with score ``m / (i + 1)`` (prefix tokens count in the sum and in the length) and leaves; the others continue in pick order.

With no constraint this is ``group_search.group_search`` with one group.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from .group_search import finalize
from .sampling import log_softmax, masked_logits

MAX_BEAM = 16     # CN_MAX_BEAM
MAX_NGRAM = 64    # CN_MAX_NGRAM
MAX_PRED = 64     # CN_MAX_PRED


def check_arguments(beam: int, no_repeat_ngram: int, max_pred: int, prefix_width: int = 0) -> Tuple[int, int]:
    """(W, n) as ints; ValueError for what conette_decode_constrained refuses."""
    w, n, p = int(beam), int(no_repeat_ngram), int(prefix_width)
    if w != beam or w < 1 or w > MAX_BEAM:
        raise ValueError(f"beam={beam} unsupported (1..{MAX_BEAM})")
    if n != no_repeat_ngram or n < 0 or n > MAX_NGRAM:
        raise ValueError(f"no_repeat_ngram={no_repeat_ngram} outside 0 .. {MAX_NGRAM}")
    if int(max_pred) < 1 or int(max_pred) > MAX_PRED:
        raise ValueError(f"max_pred={max_pred} unsupported (1..{MAX_PRED})")
    if p < 0 or p > int(max_pred) - 1:
        raise ValueError(f"prefix of {p} tokens is not shorter than max_pred={max_pred}")
    return w, n


def ngram_banned(seq: Sequence[int], n: int) -> List[int]:
    """M3: the tokens that would complete an n-gram the sequence (s_0 .. s_i) already holds."""
    n, i = int(n), len(seq) - 1
    if n < 1:
        return []
    tail = list(seq[i - n + 2: i + 1]) if n > 1 else []
    return [int(seq[j + n - 1]) for j in range(0, i - n + 2) if list(seq[j: j + n - 1]) == tail]


def has_repeated_ngram(seq: Sequence[int], n: int) -> bool:
    """True if some n-gram occurs twice in ``seq`` (n >= 1)."""
    grams = [tuple(seq[j: j + n]) for j in range(len(seq) - n + 1)]
    return len(set(grams)) != len(grams)


def check_prefix(prefix: Sequence[int], task_token: int, *, vocab_size: int, max_pred: int, eos_id: int, pad_id: int,
                 bos_id: Optional[int] = None, ban=None, forbid=None, no_repeat_ngram: int = 0) -> List[int]:
    """One clip's prefix as a list of ints; ValueError for a prefix the search could only void: a token outside the vocabulary,
    ``<eos>`` / pad / ``<bos>``, a banned token, a second occurrence of a forbid-masked token (the task token counts), an n-gram
    of its own twice, or a length that is not below ``max_pred``."""
    toks = [int(t) for t in prefix]
    if len(toks) > int(max_pred) - 1:
        raise ValueError(f"prefix of {len(toks)} tokens is not shorter than max_pred={max_pred}")
    special = {int(eos_id): "<eos>", int(pad_id): "<pad>"}
    if bos_id is not None:
        special[int(bos_id)] = "<bos>"
    banned = None if ban is None else np.asarray(ban).astype(bool).reshape(-1)
    fb = None if forbid is None else np.asarray(forbid).astype(bool).reshape(-1)
    seq = [int(task_token)]
    for i, t in enumerate(toks):
        if not 0 <= t < int(vocab_size):
            raise ValueError(f"prefix token {t} at position {i} is outside the vocabulary (0..{int(vocab_size) - 1})")
        if t in special:
            raise ValueError(f"prefix token {t} at position {i} is {special[t]}")
        if banned is not None and banned[t]:
            raise ValueError(f"prefix token {t} at position {i} is banned")
        if fb is not None and fb[t] and t in seq:
            raise ValueError(f"prefix token {t} at position {i} repeats a token the forbid mask allows once")
        seq.append(t)
    n = int(no_repeat_ngram)
    if n >= 1 and has_repeated_ngram(seq, n):
        raise ValueError(f"prefix repeats one of its own {n}-grams (no_repeat_ngram={n})")
    return toks


def constraint_mask(z, seq: Sequence[int], step: int, min_pred: int, eos_id: int, forbid=None, ban=None,
                    no_repeat_ngram: int = 0) -> np.ndarray:
    """M1, M2 and M3 on the float64 logits of a row whose sequence is ``seq`` (s_0 .. s_step); a copy."""
    assert len(seq) == step + 1
    z = masked_logits(z, seq, step, min_pred, eos_id, forbid)
    if ban is not None:
        z[np.asarray(ban).astype(bool).reshape(-1)] = -np.inf
    for t in ngram_banned(seq, no_repeat_ngram):
        z[t] = -np.inf
    return z


def decide(logits, prefixes: Sequence[Sequence[int]], sums: Sequence[float], k: int, step: int, min_pred: int, eos_id: int = 2,
           forbid=None, ban=None, no_repeat_ngram: int = 0, forced_token: Optional[int] = None) -> Dict[str, object]:
    """One call.  ``logits`` (n, V): the raw logits of the candidate rows (n = 1 in a forced or fan-out call, else n = k);
    ``prefixes`` / ``sums``: their sequences and running sums.  ``forced_token`` None: a free call -- returns parents, tokens and
    carried ``sums`` of the f <= k picks in pick order and the effective ``margin`` (the smallest gap between consecutive picks
    and between the last pick and the best finite candidate left; inf where there is none).  Else the forced call: one pick
    (0, token), or none when its score is not finite (``void``)."""
    z = np.asarray(logits, dtype=np.float64)
    n, v = z.shape
    m = np.empty((n, v), dtype=np.float64)
    for p in range(n):
        lp = log_softmax(constraint_mask(z[p], prefixes[p][: step + 1], step, min_pred, eos_id, forbid, ban, no_repeat_ngram))
        m[p] = lp if step == 0 else float(sums[p]) + lp
    if forced_token is not None:
        t = int(forced_token)
        ok = n >= 1 and 0 <= t < v and t != eos_id and bool(np.isfinite(m[0, t]))
        return {"parents": [0] if ok else [], "tokens": [t] if ok else [], "sums": [float(m[0, t])] if ok else [],
                "margin": float("inf"), "void": not ok, "forced": True}
    flat = m.reshape(-1)
    finite = np.nonzero(np.isfinite(flat))[0]
    order = finite[np.argsort(-flat[finite], kind="stable")][: k + 1]        # stable: ties go to the lowest flat index
    picks = order[:k]
    vals = flat[picks]
    gaps = [float(vals[j] - vals[j + 1]) for j in range(len(picks) - 1)]
    if order.shape[0] > k:
        gaps.append(float(vals[k - 1] - flat[order[k]]))
    return {"parents": (picks // v).tolist(), "tokens": (picks % v).tolist(), "sums": vals.tolist(),
            "margin": min(gaps) if gaps else float("inf"), "void": False, "forced": False}


def constrained_search(logits_fn: Callable[[List[Tuple[int, List[int]]], int], np.ndarray], bos_ids: Sequence[int], beam: int,
                       min_pred: int, max_pred: int, vocab_size: int, eos_id: int = 2, pad_id: int = 0, forbid=None,
                       prefixes: Optional[Sequence[Sequence[int]]] = None, ban=None, no_repeat_ngram: int = 0) -> Dict[str, object]:
    """The whole search.  ``logits_fn(rows, step)`` stands in for the decoder: ``rows`` is the list of (clip, sequence) of every
    candidate row, clips ascending (a clip that is still forced or fans out has one row); it returns their (N, V) logits of
    position ``step``.  ``prefixes``: one token list per clip (ragged) or None.  Returns mult_preds (B, W, max_pred), mult_lprobs,
    lens, best_preds, best_lprobs, sizes, and ``calls``: one dict per (step, clip) that was called -- step, clip, k, ``decide``'s
    fields, and for a free call ``plain``, the (parent, token) picks of the same state without M2 and M3."""
    b_n = len(bos_ids)
    pre = [[] for _ in range(b_n)] if prefixes is None else [[int(t) for t in p] for p in prefixes]
    w_n, n_g = check_arguments(beam, no_repeat_ngram, max_pred, max([len(p) for p in pre] + [0]))
    # a clip: its candidate rows (dicts of prefix, sum, slot) and the picks its next free call takes
    clips = [{"rows": [{"prefix": [int(bos_ids[b])], "sum": 0.0, "slot": 0}], "k": w_n, "slots": list(range(w_n))} for b in range(b_n)]
    out_preds = np.full((b_n, w_n, max_pred), pad_id, dtype=np.int64)
    out_avg = np.zeros((b_n, w_n), dtype=np.float64)
    out_len = np.zeros((b_n, w_n), dtype=np.int64)
    calls: List[dict] = []
    for step in range(max_pred):
        rows = [(b, r["prefix"]) for b in range(b_n) for r in clips[b]["rows"]]
        if not rows:
            break
        logits = np.asarray(logits_fn(rows, step), dtype=np.float64)
        at = 0
        for b in range(b_n):
            cl = clips[b]
            n = len(cl["rows"])
            if n == 0:
                continue
            z = logits[at:at + n]
            at += n
            k, slots = cl["k"], cl["slots"]
            seqs, sums = [r["prefix"] for r in cl["rows"]], [r["sum"] for r in cl["rows"]]
            if step < len(pre[b]):
                d = decide(z, seqs, sums, k, step, min_pred, eos_id, forbid, ban, n_g, forced_token=pre[b][step])
                calls.append({"step": step, "clip": b, "k": k, **d})
                if d["void"]:
                    out_avg[b, :] = -np.inf
                    cl["rows"], cl["k"] = [], 0
                else:
                    cl["rows"] = [{"prefix": seqs[0] + [d["tokens"][0]], "sum": d["sums"][0], "slot": 0}]
                continue
            d = decide(z, seqs, sums, k, step, min_pred, eos_id, forbid, ban, n_g)
            plain = decide(z, seqs, sums, k, step, min_pred, eos_id, forbid)
            calls.append({"step": step, "clip": b, "k": k, "plain": list(zip(plain["parents"], plain["tokens"])), **d})
            nxt, nslots = [], []
            for c, (parent, token, m) in enumerate(zip(d["parents"], d["tokens"], d["sums"])):
                seq = seqs[parent] + [token]
                if token == eos_id or step == max_pred - 1:
                    out_preds[b, slots[c], : step + 1] = seq[1:]
                    out_avg[b, slots[c]] = m / (step + 1)
                    out_len[b, slots[c]] = step + 1
                else:
                    nxt.append({"prefix": seq, "sum": m, "slot": slots[c]})
                    nslots.append(slots[c])
            for c in range(len(d["tokens"]), k):       # fewer finite candidates than picks: void slots
                out_avg[b, slots[c]] = -np.inf
            cl["rows"], cl["k"], cl["slots"] = nxt, len(nxt), nslots
        assert at == logits.shape[0]
    best_preds, best_lprobs, sizes = finalize(out_preds, out_avg, out_len, eos_id)
    return {"mult_preds": out_preds, "mult_lprobs": out_avg, "lens": out_len, "best_preds": best_preds, "best_lprobs": best_lprobs,
            "sizes": sizes, "calls": calls}


def min_margin(res: Dict[str, object]) -> float:
    return min(call["margin"] for call in res["calls"])
