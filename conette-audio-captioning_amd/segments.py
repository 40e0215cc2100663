"""Caption timeline: the window grid over a long recording and the rule that merges per-window captions into segments (numpy, no GPU).

``conette_decode_spans`` searches spans of recordings that were encoded once; ``conette_segments`` (include/conette_hip.h,
csrc/dec_segments.h) computes exactly the merge rule below on the device and is compared with ``merge_batch`` bit for bit.  All
quantities are in encoder frames (``alignment.FRAME_SEC`` seconds each); seconds round half up to frames, as in ``tagging``.

Window grid over a recording of n >= 1 valid frames, window Tw >= 1, hop >= 1: W = 1 if n <= Tw, else ceil((n - Tw) / hop) + 1;
window k starts at min(k * hop, max(n - Tw, 0)) and has min(Tw, n) frames.  Every frame is covered, every window of a recording has
the same length, and the last window is aligned to the recording's end.

Merge rule for one recording with windows 0 .. W - 1 in time order (best caption ids (W, L), average log-probs (W,), spans (W, 2) as
(start, len)):

* adjacency a_k = u(k, k + 1), k = 0 .. W - 2, with ``consensus``'s pair utility ("ngram" with max_order 1 .. 4, or "edit") on the
  contents in front of the first ``eos_id`` or ``pad_id``, in its fp32 operation order: an fp32 array defined bit for bit.
* window k + 1 joins the run of window k iff a_k >= threshold (compared in fp32); a run that has reached ``max_run`` windows closes
  anyway (``max_run`` 0: no cap).
* a segment reports its windows (first, end) with end exclusive; ``rep``, the window of the run with the largest log-prob (the first
  on ties; a NaN never wins; the first window if all are NaN); ``agree``, the smallest a_k inside the run (its bits), fp32(1) for a
  run of one window; and its frames (frame_start, frame_end): the first segment starts at start_0, the last ends at
  start_{W-1} + len_{W-1}, and between a segment that ends with window k and the next one the boundary is
  (start_{k+1} + start_k + len_k + 1) // 2 -- the middle of the overlap (or gap) of the two windows, rounded half up.
* ``count`` is the true number of segments; the first ``max_segments`` (1 .. 256) are stored in time order, unused slots hold
  (-1, -1), -1, 0.0 and (-1, -1).
"""
from __future__ import annotations

import math
from typing import Dict, Sequence, Tuple

import numpy as np

from . import consensus
from .alignment import FRAME_SEC

MAX_PRED = 64           # row length of the caption table (CN_MAX_PRED)
MAX_WINDOWS = 4096      # CONETTE_SEG_MAX_WINDOWS
MAX_SEGMENTS = 256      # CONETTE_SEG_MAX_SEGMENTS
UTILITY = consensus.UTILITY


# ---- seconds -> frames, rounded half up
def _frames(seconds, lowest: int) -> int:
    s = float(seconds)
    if not math.isfinite(s) or s < 0:
        raise ValueError(f"a duration of {seconds} seconds (expected a finite number >= 0)")
    return max(lowest, int(math.floor(s / FRAME_SEC + 0.5)))


def window_frames(window_s) -> int:
    """frames of a window of ``window_s`` seconds: max(1, floor(window_s / FRAME_SEC + 0.5))"""
    return _frames(window_s, 1)


def hop_frames(hop_s) -> int:
    """frames of a hop of ``hop_s`` seconds: max(1, floor(hop_s / FRAME_SEC + 0.5))"""
    return _frames(hop_s, 1)


def run_windows(max_run_s, window: int, hop: int) -> int:
    """the longest run in windows for a longest segment of ``max_run_s`` seconds: 0 (no cap) for 0 seconds, else the largest m >= 1
    with window + (m - 1) * hop <= frames(max_run_s), 1 when even one window is longer."""
    f = _frames(max_run_s, 0)
    if f == 0:
        return 0
    return max(1, (f - int(window)) // int(hop) + 1)


def seconds_to_span(onset_s, offset_s) -> Tuple[int, int]:
    """(start, len) in frames of the span [onset_s, offset_s) in seconds: both ends rounded half up, at least one frame."""
    a, b = _frames(onset_s, 0), _frames(offset_s, 0)
    if b < a:
        raise ValueError(f"span ({onset_s}, {offset_s}): offset before onset")
    return a, max(b - a, 1)


# ---- window grid
def n_windows(n: int, window: int, hop: int) -> int:
    n, window, hop = int(n), int(window), int(hop)
    if n < 1 or window < 1 or hop < 1:
        raise ValueError(f"grid of n={n} frames, window={window}, hop={hop}: all three must be at least 1")
    return 1 if n <= window else -(-(n - window) // hop) + 1


def grid(n: int, window: int, hop: int) -> np.ndarray:
    """(W, 2) int32 (start, len) of the windows over a recording of n valid frames"""
    w = n_windows(n, window, hop)
    last = max(int(n) - int(window), 0)
    out = np.empty((w, 2), dtype=np.int32)
    out[:, 0] = np.minimum(np.arange(w, dtype=np.int64) * int(hop), last)
    out[:, 1] = min(int(window), int(n))
    return out


def span_table(frame_lens: Sequence[int], window: int, hop: int) -> Tuple[np.ndarray, np.ndarray]:
    """((S, 3) int32 (recording, start, len), recording-major in time order; (N,) int32 windows per recording)"""
    rows, counts = [], []
    for r, n in enumerate(np.asarray(frame_lens).reshape(-1).tolist()):
        g = grid(n, window, hop)
        rows.append(np.concatenate([np.full((g.shape[0], 1), r, dtype=np.int32), g], axis=1))
        counts.append(g.shape[0])
    table = np.concatenate(rows, axis=0) if rows else np.zeros((0, 3), dtype=np.int32)
    return np.ascontiguousarray(table, dtype=np.int32), np.asarray(counts, dtype=np.int32)


def check_spans(table, n_rec: int, frame_lens: Sequence[int], t_span: int) -> np.ndarray:
    """The table as (S, 3) int32; ValueError naming the row for a span that does not lie inside its recording or exceeds ``t_span``."""
    t = np.asarray(table)
    if t.ndim != 2 or t.shape[1] != 3 or t.shape[0] < 1:
        raise ValueError(f"spans of shape {tuple(t.shape)}: expected (n_spans >= 1, 3) rows of (recording, start, len)")
    if not np.issubdtype(t.dtype, np.integer):
        raise ValueError(f"spans of dtype {t.dtype}: expected integers")
    lens = np.asarray(frame_lens).reshape(-1)
    if lens.shape[0] != int(n_rec):
        raise ValueError(f"frame_lens of {lens.shape[0]} entries for {n_rec} recordings")
    if int(t_span) < 1:
        raise ValueError(f"t_span={t_span} < 1")
    for s, (rec, start, ln) in enumerate(t.tolist()):
        if not 0 <= rec < int(n_rec):
            raise ValueError(f"spans[{s}]: recording {rec} outside 0 .. {int(n_rec) - 1}")
        if start < 0:
            raise ValueError(f"spans[{s}]: start {start} < 0")
        if ln < 1:
            raise ValueError(f"spans[{s}]: len {ln} < 1")
        if start + ln > int(lens[rec]):
            raise ValueError(f"spans[{s}]: start {start} + len {ln} exceeds the {int(lens[rec])} valid frames of recording {rec}")
        if ln > int(t_span):
            raise ValueError(f"spans[{s}]: len {ln} exceeds t_span={int(t_span)}")
    return np.ascontiguousarray(t, dtype=np.int32)


# ---- merge rule
def check_arguments(row_len: int = 1, w_max: int = 1, utility: str = "ngram", max_order: int = 4, threshold: float = 0.5,
                    max_run: int = 0, max_segments: int = 64) -> int:
    """The utility's code; ValueError naming the argument for what conette_segments refuses."""
    if not 1 <= int(row_len) <= MAX_PRED:
        raise ValueError(f"row_len={row_len} unsupported (1..{MAX_PRED})")
    if not 1 <= int(w_max) <= MAX_WINDOWS:
        raise ValueError(f"w_max={w_max} unsupported (1..{MAX_WINDOWS})")
    if utility not in UTILITY:
        raise ValueError(f"utility={utility!r} unknown (expected one of {tuple(UTILITY)})")
    if isinstance(max_order, bool) or int(max_order) != max_order or not 1 <= int(max_order) <= consensus.MAX_ORDER:
        raise ValueError(f"max_order={max_order} unsupported (1..{consensus.MAX_ORDER})")
    if not math.isfinite(float(threshold)):
        raise ValueError(f"threshold={threshold} must be finite")
    if isinstance(max_run, bool) or int(max_run) != max_run or int(max_run) < 0:
        raise ValueError(f"max_run={max_run} unsupported (0: no cap, or at least 1)")
    if isinstance(max_segments, bool) or int(max_segments) != max_segments or not 1 <= int(max_segments) <= MAX_SEGMENTS:
        raise ValueError(f"max_segments={max_segments} unsupported (1..{MAX_SEGMENTS})")
    return UTILITY[utility]


def adjacency(preds, utility: str = "ngram", max_order: int = 4, eos_id: int = 2, pad_id: int = 0, dtype=np.float32) -> np.ndarray:
    """a (W - 1,) in ``dtype`` arithmetic: ``consensus``'s pair utility of every two neighbouring rows of ``preds`` (W, L)"""
    cs = consensus.contents(np.asarray(preds), None, eos_id, pad_id)
    out = np.zeros(max(len(cs) - 1, 0), dtype=dtype)
    for k in range(len(cs) - 1):
        out[k] = consensus._pairwise([cs[k], cs[k + 1]], utility, max_order, dtype)[0, 1]
    return out


def runs(adj: np.ndarray, w: int, threshold, max_run: int = 0):
    """[(first, end)] of the runs over windows 0 .. w - 1 given the adjacency (compared as it is: fp32 against fp32(threshold))"""
    out, first = [], 0
    thr = adj.dtype.type(threshold) if w > 1 else threshold
    for k in range(w - 1):
        joins = bool(adj[k] >= thr) and not (max_run > 0 and k + 1 - first >= max_run)
        if not joins:
            out.append((first, k + 1))
            first = k + 1
    if w > 0:
        out.append((first, w))
    return out


def representative(lprobs: np.ndarray, first: int, end: int) -> int:
    best, bv = first, lprobs[first]
    for k in range(first + 1, end):
        v = lprobs[k]
        if v > bv or (np.isnan(bv) and not np.isnan(v)):
            best, bv = k, v
    return best


def merge(preds, lprobs, spans, utility: str = "ngram", max_order: int = 4, threshold: float = 0.5, max_run: int = 0,
          max_segments: int = 64, eos_id: int = 2, pad_id: int = 0) -> Dict[str, object]:
    """The rule for one recording: {"adjacency" (W - 1,) fp32, "seg_windows" (max_segments, 2) int32, "seg_frames"
    (max_segments, 2) int32, "seg_rep" (max_segments,) int32, "seg_agree" (max_segments,) fp32, "count"}."""
    preds = np.asarray(preds)
    if preds.ndim != 2:
        raise ValueError(f"preds of shape {tuple(preds.shape)}: expected (windows, row_len)")
    w = preds.shape[0]
    check_arguments(preds.shape[1], max(w, 1), utility, max_order, threshold, max_run, max_segments)
    lprobs = np.asarray(lprobs, dtype=np.float32).reshape(-1)
    spans = np.asarray(spans, dtype=np.int64).reshape(-1, 2)
    if lprobs.shape[0] != w or spans.shape[0] != w:
        raise ValueError(f"{w} windows with {lprobs.shape[0]} lprobs and {spans.shape[0]} spans")
    adj = adjacency(preds, utility, max_order, eos_id, pad_id, np.float32)
    ms = int(max_segments)
    seg_w = np.full((ms, 2), -1, dtype=np.int32)
    seg_f = np.full((ms, 2), -1, dtype=np.int32)
    seg_rep = np.full(ms, -1, dtype=np.int32)
    seg_agree = np.zeros(ms, dtype=np.float32)
    rs = runs(adj, w, np.float32(threshold), int(max_run))
    for i, (first, end) in enumerate(rs[:ms]):
        seg_w[i] = (first, end)
        f0 = spans[0, 0] if first == 0 else (spans[first, 0] + spans[first - 1, 0] + spans[first - 1, 1] + 1) // 2
        f1 = spans[w - 1, 0] + spans[w - 1, 1] if end == w else (spans[end, 0] + spans[end - 1, 0] + spans[end - 1, 1] + 1) // 2
        seg_f[i] = (f0, f1)
        seg_rep[i] = representative(lprobs, first, end)
        seg_agree[i] = np.float32(1.0) if end - first == 1 else adj[first:end - 1].min()
    return {"adjacency": adj, "seg_windows": seg_w, "seg_frames": seg_f, "seg_rep": seg_rep, "seg_agree": seg_agree, "count": len(rs)}


def merge_batch(preds, n_windows, lprobs, spans, **kw) -> Dict[str, np.ndarray]:
    """``merge`` over recordings: ``preds`` (N, Wmax, L), ``n_windows`` (N,) in 0 .. Wmax, ``lprobs`` (N, Wmax), ``spans``
    (N, Wmax, 2).  Windows at or beyond ``n_windows[r]`` are never read.  "adjacency" is (N, Wmax - 1) with exact zeros beyond
    ``n_windows[r] - 2``; "counts" (N,) int32."""
    preds = np.asarray(preds)
    if preds.ndim != 3:
        raise ValueError(f"preds of shape {tuple(preds.shape)}: expected (recordings, windows, row_len)")
    n, wmax = preds.shape[0], preds.shape[1]
    nw = np.asarray(n_windows).reshape(-1)
    lprobs, spans = np.asarray(lprobs), np.asarray(spans)
    if nw.shape[0] != n or tuple(lprobs.shape) != (n, wmax) or tuple(spans.shape) != (n, wmax, 2):
        raise ValueError(f"preds {tuple(preds.shape)} with n_windows {tuple(nw.shape)}, lprobs {tuple(lprobs.shape)}, spans {tuple(spans.shape)}")
    if nw.size and (nw.min() < 0 or nw.max() > wmax):
        raise ValueError(f"n_windows must lie in 0..{wmax} (found {int(nw.min())}..{int(nw.max())})")
    check_arguments(preds.shape[2], max(wmax, 1), kw.get("utility", "ngram"), kw.get("max_order", 4), kw.get("threshold", 0.5),
                    kw.get("max_run", 0), kw.get("max_segments", 64))
    adj = np.zeros((n, max(wmax - 1, 0)), dtype=np.float32)
    rs = []
    for r in range(n):
        w = int(nw[r])
        one = merge(preds[r, :w], lprobs[r, :w], spans[r, :w], **kw)
        adj[r, :max(w - 1, 0)] = one["adjacency"]
        rs.append(one)
    return {"adjacency": adj, "seg_windows": np.stack([o["seg_windows"] for o in rs]), "seg_frames": np.stack([o["seg_frames"] for o in rs]),
            "seg_rep": np.stack([o["seg_rep"] for o in rs]), "seg_agree": np.stack([o["seg_agree"] for o in rs]),
            "counts": np.asarray([o["count"] for o in rs], dtype=np.int32)}
