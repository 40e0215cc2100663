"""Keyword-guided beam search semantics: the CPU restatement of one call and of a whole search (float64 numpy, no GPU).

``conette_decode_required`` (include/conette_hip.h, csrc/dec_require.h) computes exactly this rule in fp32 on the device; the
tests replay its calls through ``decide`` and compare whole searches with ``required_search``.

It is ``constrained_search.py``'s search -- the same prefix, ban mask, n-gram rule, forced / fan-out / later calls, void slots and
bookkeeping -- with per-clip requirements on top (dynamic beam allocation: hypotheses are banked by the requirements they have met,
the beam's slots are dealt to the banks in turn, and a caption cannot end early).

Requirements of clip b: G groups, 0 <= G <= 8, each a non-empty set of tokens ("dog" or "dogs"); at most R = 32 tokens per clip
over all groups; no token in two groups; a required token is never ``<eos>``, pad, ``<bos>``, the clip's task token or a banned
token.  Group g of a row is MET when one of its tokens occurs among s_1 .. s_i (prefix tokens count); ``unmet(p)`` is the number of
unmet groups of row p and ``c(p) = G - unmet(p)``.

Masks, after M1 to M3 of the constrained search, on every call of a row, forced calls included (``requirement_mask``):

* M4: while ``unmet(p) > 0``, ``z[eos] = -inf``;
* M5: if ``unmet(p) >= max_pred - i``, ``z[v] = -inf`` for every v that is not a token of one of the row's unmet groups (only just
  enough positions are left: the candidate's token becomes s_{i+1});
* ``lp = log_softmax`` of the masked row; the model score ``m(p, v)`` is the constrained search's.

Banks: candidate (p, v) is in bank ``c(p) + 1`` if v belongs to an unmet group of row p, else in bank ``c(p)``.

Picks of a free call with k slots (``decide``): per bank the candidates are ordered by descending finite m, ties to the lowest flat
index ``p * V + v``; the slots are dealt round-robin from the highest non-empty bank to the lowest, again and again, skipping
exhausted banks, until k picks or until no finite candidate is left.  With fewer finite candidates than k the slots of the
remaining row positions become void.  Pick order is deal order.  Forced calls are the constrained search's, under M4 / M5.

``check_requirements`` refuses a clip whose unmet count after its prefix exceeds ``max_pred - plen``; then M5 never fires against a
prefix token, and with M4 every hypothesis that is not void holds a token of every group.  Under that check an M5 row itself never
runs dry (the n-gram rule and the forbid mask only take tokens the row's sequence holds, and a token of an unmet group is not among
them), but M5 can leave a call fewer finite candidates than slots -- a fan-out with fewer unmet-group tokens than W: void slots.

The effective margin of a call: the smallest gap, over banks, between consecutive picks of one bank and between a bank's last pick
and the best finite candidate left in that bank (inf where there is none).  Which bank a candidate is in, and how many picks a
bank gets, is decided by integers alone.  With no requirement this is ``constrained_search.constrained_search``.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import constrained_search as CS
from .group_search import finalize
from .sampling import log_softmax

MAX_GROUPS = 8        # RQ_MAX_GROUPS
MAX_REQ_TOKENS = 32   # RQ_MAX_TOKENS

Groups = List[List[int]]


def check_arguments(beam: int, no_repeat_ngram: int, max_pred: int, prefix_width: int = 0, req_width: int = 0) -> Tuple[int, int]:
    """(W, n) as ints; ValueError for what conette_decode_required refuses."""
    w, n = CS.check_arguments(beam, no_repeat_ngram, max_pred, prefix_width)
    if int(req_width) < 0 or int(req_width) > MAX_REQ_TOKENS:
        raise ValueError(f"req_width={req_width} outside 0 .. {MAX_REQ_TOKENS}")
    return w, n


def check_requirements(groups: Sequence[Sequence[int]], task_token: int, *, vocab_size: int, max_pred: int, eos_id: int, pad_id: int,
                       bos_id: Optional[int] = None, ban=None, prefix: Sequence[int] = (), words=None) -> Groups:
    """One clip's requirements as a list of token lists (duplicates inside a group dropped); ValueError for what the search could
    not honour: more than 8 groups, an empty group, more than 32 tokens, a token outside the vocabulary, in two groups, ``<eos>`` /
    pad / ``<bos>`` / the task token, a banned token, or more groups left unmet by the prefix than positions left after it.
    ``words``: optional {token: word} for the messages."""
    name = (lambda t: f"{t} ({words[t]!r})") if words else (lambda t: str(t))
    out: Groups = [list(dict.fromkeys(int(t) for t in g)) for g in groups]
    if len(out) > MAX_GROUPS:
        raise ValueError(f"{len(out)} requirement groups (at most {MAX_GROUPS})")
    special = {int(eos_id): "<eos>", int(pad_id): "<pad>", int(task_token): "the clip's task token"}
    if bos_id is not None:
        special.setdefault(int(bos_id), "<bos>")
    banned = None if ban is None else np.asarray(ban).astype(bool).reshape(-1)
    owner: Dict[int, int] = {}
    for g, toks in enumerate(out):
        if not toks:
            raise ValueError(f"requirement group {g} is empty")
        for t in toks:
            if not 0 <= t < int(vocab_size):
                raise ValueError(f"required token {name(t)} of group {g} is outside the vocabulary (0..{int(vocab_size) - 1})")
            if t in special:
                raise ValueError(f"required token {name(t)} of group {g} is {special[t]}")
            if banned is not None and banned[t]:
                raise ValueError(f"required token {name(t)} of group {g} is banned")
            if t in owner:
                raise ValueError(f"required token {name(t)} is in groups {owner[t]} and {g}")
            owner[t] = g
    if len(owner) > MAX_REQ_TOKENS:
        raise ValueError(f"{len(owner)} required tokens (at most {MAX_REQ_TOKENS} per clip)")
    pre = [int(t) for t in prefix]
    unmet = sum(1 for m in met_groups([int(task_token)] + pre, out) if not m)
    if unmet > int(max_pred) - len(pre):
        left = [name(toks[0]) for toks, m in zip(out, met_groups([int(task_token)] + pre, out)) if not m]
        raise ValueError(f"{unmet} required groups (first tokens {', '.join(left)}) do not fit into the {int(max_pred) - len(pre)} "
                         f"positions max_pred={max_pred} leaves after a prefix of {len(pre)} tokens")
    return out


def met_groups(seq: Sequence[int], groups: Sequence[Sequence[int]]) -> List[bool]:
    """Per group: does one of its tokens occur among s_1 .. s_i of ``seq`` = s_0 .. s_i?"""
    seen = set(int(t) for t in seq[1:])
    return [any(int(t) in seen for t in g) for g in groups]


def unmet_tokens(seq: Sequence[int], groups: Sequence[Sequence[int]]) -> List[int]:
    """The tokens of the row's unmet groups."""
    return [int(t) for g, m in zip(groups, met_groups(seq, groups)) if not m for t in g]


def requirement_mask(z, seq: Sequence[int], step: int, max_pred: int, eos_id: int, groups: Sequence[Sequence[int]]) -> np.ndarray:
    """M4 and M5 on the float64 logits of a row whose sequence is ``seq`` (s_0 .. s_step); a copy."""
    assert len(seq) == step + 1
    z = np.array(z, dtype=np.float64).reshape(-1)
    open_tokens = unmet_tokens(seq, groups)
    unmet = sum(1 for m in met_groups(seq, groups) if not m)
    if unmet > 0:
        z[eos_id] = -np.inf
    if unmet > 0 and unmet >= int(max_pred) - step:
        keep = np.zeros(z.shape[0], dtype=bool)
        keep[[t for t in open_tokens if 0 <= t < z.shape[0]]] = True
        z[~keep] = -np.inf
    return z


def masked_row(z, seq: Sequence[int], step: int, min_pred: int, max_pred: int, eos_id: int, forbid=None, ban=None,
               no_repeat_ngram: int = 0, groups: Sequence[Sequence[int]] = ()) -> np.ndarray:
    """M1 to M5 on one row's float64 logits; a copy."""
    return requirement_mask(CS.constraint_mask(z, seq, step, min_pred, eos_id, forbid, ban, no_repeat_ngram), seq, step, max_pred,
                            eos_id, groups)


def decide(logits, prefixes: Sequence[Sequence[int]], sums: Sequence[float], k: int, step: int, min_pred: int, max_pred: int,
           eos_id: int = 2, forbid=None, ban=None, no_repeat_ngram: int = 0, groups: Sequence[Sequence[int]] = (),
           forced_token: Optional[int] = None) -> Dict[str, object]:
    """One call of a clip whose requirements are ``groups``.  Arguments as ``constrained_search.decide``.  A free call returns
    parents, tokens and carried ``sums`` of the f <= k picks in deal order, their ``banks``, and the effective ``margin``; a forced
    call one pick (0, token) or none (``void``).  ``m5_rows``: the candidate rows M5 applied to."""
    z = np.asarray(logits, dtype=np.float64)
    n, v = z.shape
    m = np.empty((n, v), dtype=np.float64)
    bank = np.empty((n, v), dtype=np.int64)
    m5_rows = 0
    for p in range(n):
        seq = list(prefixes[p][: step + 1])
        unmet = sum(1 for g in met_groups(seq, groups) if not g)
        m5_rows += int(0 < unmet and unmet >= int(max_pred) - step)
        lp = log_softmax(masked_row(z[p], seq, step, min_pred, max_pred, eos_id, forbid, ban, no_repeat_ngram, groups))
        m[p] = lp if step == 0 else float(sums[p]) + lp
        bank[p] = sum(1 for g in met_groups(seq, groups) if g)
        open_tokens = [t for t in unmet_tokens(seq, groups) if 0 <= t < v]
        bank[p, open_tokens] += 1
    if forced_token is not None:
        t = int(forced_token)
        ok = n >= 1 and 0 <= t < v and t != eos_id and bool(np.isfinite(m[0, t]))
        return {"parents": [0] if ok else [], "tokens": [t] if ok else [], "sums": [float(m[0, t])] if ok else [],
                "banks": [int(bank[0, t])] if ok else [], "margin": float("inf"), "void": not ok, "forced": True, "m5_rows": m5_rows}
    flat, fbank = m.reshape(-1), bank.reshape(-1)
    finite = np.nonzero(np.isfinite(flat))[0]
    orders = {}
    for j in sorted(set(fbank[finite].tolist()), reverse=True):
        idx = finite[fbank[finite] == j]
        orders[j] = idx[np.argsort(-flat[idx], kind="stable")]        # stable: ties go to the lowest flat index
    picks: List[int] = []
    taken = {j: 0 for j in orders}
    r = 0
    while len(picks) < k and any(r < len(o) for o in orders.values()):
        for j in orders:                                                # highest bank first
            if r < len(orders[j]) and len(picks) < k:
                picks.append(int(orders[j][r]))
                taken[j] += 1
        r += 1
    gaps = []
    for j, o in orders.items():
        vals = flat[o[: taken[j] + 1]]
        if taken[j] > 0:
            gaps += [float(vals[i] - vals[i + 1]) for i in range(len(vals) - 1)]
    pk = np.asarray(picks, dtype=np.int64)
    return {"parents": (pk // v).tolist(), "tokens": (pk % v).tolist(), "sums": flat[pk].tolist(), "banks": fbank[pk].tolist(),
            "margin": min(gaps) if gaps else float("inf"), "void": False, "forced": False, "m5_rows": m5_rows}


def required_search(logits_fn: Callable[[List[Tuple[int, List[int]]], int], np.ndarray], bos_ids: Sequence[int], beam: int,
                    min_pred: int, max_pred: int, vocab_size: int, eos_id: int = 2, pad_id: int = 0, forbid=None,
                    prefixes: Optional[Sequence[Sequence[int]]] = None, ban=None, no_repeat_ngram: int = 0,
                    required: Optional[Sequence[Sequence[Sequence[int]]]] = None) -> Dict[str, object]:
    """The whole search; arguments and result as ``constrained_search.constrained_search`` plus ``required``: per clip its list of
    groups (None: none anywhere).  ``calls``: one dict per (step, clip) that was called -- step, clip, k, ``decide``'s fields, and
    for a free call ``plain``, the (parent, token) picks of the same state without requirements."""
    b_n = len(bos_ids)
    pre = [[] for _ in range(b_n)] if prefixes is None else [[int(t) for t in p] for p in prefixes]
    req: List[Groups] = [[] for _ in range(b_n)] if required is None else [[[int(t) for t in g] for g in r] for r in required]
    w_n, n_g = check_arguments(beam, no_repeat_ngram, max_pred, max([len(p) for p in pre] + [0]),
                               max([sum(len(g) for g in r) for r in req] + [0]))
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
                d = decide(z, seqs, sums, k, step, min_pred, max_pred, eos_id, forbid, ban, n_g, req[b], forced_token=pre[b][step])
                calls.append({"step": step, "clip": b, "k": k, **d})
                if d["void"]:
                    out_avg[b, :] = -np.inf
                    cl["rows"], cl["k"] = [], 0
                else:
                    cl["rows"] = [{"prefix": seqs[0] + [d["tokens"][0]], "sum": d["sums"][0], "slot": 0}]
                continue
            d = decide(z, seqs, sums, k, step, min_pred, max_pred, eos_id, forbid, ban, n_g, req[b])
            plain = CS.decide(z, seqs, sums, k, step, min_pred, eos_id, forbid, ban, n_g)
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


def pack_tables(required: Sequence[Sequence[Sequence[int]]], width: Optional[int] = None, order=None) -> Tuple[np.ndarray, np.ndarray]:
    """The (B, width) int32 tables ``conette_decode_required`` takes: (req_tokens, req_groups), unused entries (0, -1).
    ``order``: optional per clip a list of the ``width`` table positions its entries go to (tests: shuffled order, gaps)."""
    flat = [[(int(t), g) for g, toks in enumerate(r) for t in toks] for r in required]
    need = max([len(f) for f in flat] + [0])
    width = need if width is None else int(width)
    if width < need:
        raise ValueError(f"req_width={width} is below the {need} required tokens of a clip")
    toks = np.zeros((len(flat), width), dtype=np.int32)
    grps = np.full((len(flat), width), -1, dtype=np.int32)
    for b, f in enumerate(flat):
        pos = list(range(len(f))) if order is None else list(order[b])[: len(f)]
        for (t, g), e in zip(f, pos):
            toks[b, e], grps[b, e] = t, g
    return toks, grps


def min_margin(res: Dict[str, object]) -> float:
    return min(call["margin"] for call in res["calls"])
