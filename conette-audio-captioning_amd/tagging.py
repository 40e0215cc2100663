"""The tag timeline's rule, in numpy: WHEN each AudioSet tag is heard in a clip.  No GPU and no library; the statement that
csrc/enc_tags.h (conette_tag_frames / conette_tag_events, include/conette_hip.h) is held to.

Frame rule (``frame_probs``, float64).  The clip head pools the encoder's frame embeddings over the whole clip -- max over time plus
mean over time, LayerNorm, head_audioset, sigmoid.  Pooled over a window of ``w`` frames around frame ``t`` instead, the same head
gives a probability per 0.32 s frame: with lo = (w - 1) // 2, hi = w // 2 and n = frame_lens[b], for t < n
    a = max(0, t - lo), e = min(n, t + hi + 1)
    v[c] = max_{a <= u < e} fe[b, u, c] + (sum_{a <= u < e} fe[b, u, c]) / (e - a)
    z    = LayerNorm_768(v, eps 1e-6) * norm_w + norm_b
    p[b, t, :] = sigmoid(head_w z + head_b)
and p[b, t, :] = 0 for t >= n.  The window never reads a frame at or beyond n: the padded frames of a batch are the encoder's output
for zero-padded audio, not zeros.  A window that covers the clip (w >= 2 n - 1) gives the clip head's ``clipwise_output`` at every t.

Event rule (``events``) for one (clip, tag) sequence p[0 .. T) of fp32 values, compared in fp32 -- so it is exact:
 1. a RUN is a maximal interval of consecutive frames t < n with p[t] >= off that holds at least one frame with p[t] >= on
    (hysteresis; off = on is plain thresholding; a NaN is below every threshold);
 2. in time order, a run that starts at most ``max_gap`` frames after the (exclusive) end of the event before it joins that event;
 3. after merging, an event shorter than ``min_frames`` (end - start) is dropped;
 4. an event reports (start, end), peak -- the largest p inside it, its bits copied -- and peak_frame, the lowest index of that peak;
 5. count is the true number of events; the first ``max_events`` in time order are stored, unused slots hold (-1, -1), 0.0 and -1.
"""
import math

import numpy as np

from .alignment import FRAME_SEC

MAX_WINDOW = 255       # CONETTE_TAG_MAX_WINDOW
MAX_EVENTS = 64        # CONETTE_TAG_MAX_EVENTS
LN_EPS = 1e-6


# ---- seconds -> frames: all round half up on the 0.32 s grid -------------------------------------------------------------------------
def _frames(seconds, lowest):
    s = float(seconds)
    if not math.isfinite(s) or s < 0:
        raise ValueError(f"a duration of {seconds} seconds (expected a finite number >= 0)")
    return max(lowest, int(math.floor(s / FRAME_SEC + 0.5)))


def window_frames(window_s) -> int:
    """frames of a pooling window of ``window_s`` seconds: max(1, floor(window_s / FRAME_SEC + 0.5))"""
    return _frames(window_s, 1)


def min_frames(min_duration_s) -> int:
    """the shortest event kept, in frames: max(1, floor(min_duration_s / FRAME_SEC + 0.5))"""
    return _frames(min_duration_s, 1)


def gap_frames(max_gap_s) -> int:
    """the longest gap bridged, in frames: max(0, floor(max_gap_s / FRAME_SEC + 0.5))"""
    return _frames(max_gap_s, 0)


def check_arguments(window=1, on=0.5, off=None, min_frames=1, max_gap=0, max_events=1) -> None:
    """ValueError naming the argument for settings the kernels refuse (off None: off = on)."""
    if isinstance(window, bool) or int(window) != window or not 1 <= int(window) <= MAX_WINDOW:
        raise ValueError(f"Invalid argument window={window}. (expected 1..{MAX_WINDOW} frames)")
    on32 = np.float32(on)
    if not np.isfinite(on32) or not 0 < on32 <= 1:
        raise ValueError(f"Invalid argument on={on}. (expected a finite threshold with 0 < off <= on <= 1)")
    if off is not None:
        off32 = np.float32(off)
        if not np.isfinite(off32) or not 0 < off32 <= on32:
            raise ValueError(f"Invalid argument off={off}. (expected a finite threshold with 0 < off <= on <= 1, on={on})")
    if int(min_frames) != min_frames or min_frames < 1:
        raise ValueError(f"Invalid argument min_frames={min_frames}. (expected at least 1)")
    if int(max_gap) != max_gap or max_gap < 0:
        raise ValueError(f"Invalid argument max_gap={max_gap}. (expected at least 0)")
    if isinstance(max_events, bool) or int(max_events) != max_events or not 1 <= int(max_events) <= MAX_EVENTS:
        raise ValueError(f"Invalid argument max_events={max_events}. (expected 1..{MAX_EVENTS})")


# ---- the frame rule ------------------------------------------------------------------------------------------------------------------
def frame_probs(frame_embs, frame_lens, norm_w, norm_b, head_w, head_b, window) -> np.ndarray:
    """(B, T, n_tags) float64 from ``frame_embs`` (B, T, 768), ``frame_lens`` (B,) in 0 .. T, the clip head's LayerNorm
    (``norm_w``, ``norm_b``: (768,)) and linear layer (``head_w`` (n_tags, 768), ``head_b`` (n_tags,)), and a window in frames."""
    check_arguments(window=window)
    fe = np.asarray(frame_embs, dtype=np.float64)
    lens = np.asarray(frame_lens).astype(np.int64)
    nw, nb = np.asarray(norm_w, dtype=np.float64), np.asarray(norm_b, dtype=np.float64)
    hw, hb = np.asarray(head_w, dtype=np.float64), np.asarray(head_b, dtype=np.float64)
    bsize, t_audio, _ = fe.shape
    if lens.shape != (bsize,) or (lens < 0).any() or (lens > t_audio).any():
        raise ValueError(f"Invalid argument frame_lens={lens.tolist()}. (expected {bsize} lengths in 0..{t_audio})")
    w = int(window)
    lo, hi = (w - 1) // 2, w // 2
    out = np.zeros((bsize, t_audio, hw.shape[0]), dtype=np.float64)
    for b in range(bsize):
        n = int(lens[b])
        if n == 0:
            continue
        v = np.empty((n, fe.shape[2]), dtype=np.float64)
        for t in range(n):
            a, e = max(0, t - lo), min(n, t + hi + 1)
            v[t] = fe[b, a:e].max(axis=0) + fe[b, a:e].sum(axis=0) / (e - a)
        mean = v.mean(axis=1, keepdims=True)
        var = ((v - mean) ** 2).mean(axis=1, keepdims=True)
        z = (v - mean) / np.sqrt(var + LN_EPS) * nw + nb
        for t in range(n):      # (row by row: a row's value does not depend on how many rows there are)
            out[b, t] = 1.0 / (1.0 + np.exp(-(hw @ z[t] + hb)))
    return out


# ---- the event rule ------------------------------------------------------------------------------------------------------------------
def _empty_tables(shape, max_events):
    return {"spans": np.full(shape + (max_events, 2), -1, dtype=np.int32), "peaks": np.zeros(shape + (max_events,), dtype=np.float32),
            "peak_frames": np.full(shape + (max_events,), -1, dtype=np.int32)}


def events(p, n, on, off, min_frames=1, max_gap=0, max_events=MAX_EVENTS) -> dict:
    """The events of ONE sequence ``p`` (T,) fp32 of which the first ``n`` frames count, as the module's docstring states them:
    {"spans": (max_events, 2) int32, "peaks": (max_events,) fp32, "peak_frames": (max_events,) int32, "count": int}."""
    check_arguments(on=on, off=off, min_frames=min_frames, max_gap=max_gap, max_events=max_events)
    p = np.asarray(p)
    if p.dtype != np.float32 or p.ndim != 1:
        raise ValueError(f"Invalid argument p of dtype {p.dtype} and shape {p.shape}. (expected one fp32 sequence)")
    n = min(max(int(n), 0), p.shape[0])
    on32, off32 = np.float32(on), np.float32(off)
    # 1. runs
    runs, t = [], 0
    while t < n:
        if not p[t] >= off32:       # (a NaN compares false)
            t += 1
            continue
        start = t
        while t < n and p[t] >= off32:
            t += 1
        if any(p[u] >= on32 for u in range(start, t)):
            runs.append((start, t))
    # 2. merging
    merged = []
    for start, end in runs:
        if merged and start - merged[-1][1] <= max_gap:
            merged[-1] = (merged[-1][0], end)
        else:
            merged.append((start, end))
    # 3. - 5.
    kept = [(s, e) for s, e in merged if e - s >= min_frames]
    out = _empty_tables((), int(max_events))
    for k, (s, e) in enumerate(kept[:max_events]):
        best = s                    # (p[s] >= off: not a NaN, and a NaN further on is never larger)
        for u in range(s + 1, e):
            if p[u] > p[best]:
                best = u
        out["spans"][k] = (s, e)
        out["peaks"][k] = p[best]
        out["peak_frames"][k] = best
    out["count"] = len(kept)
    return out


def events_batch(frame_probs, frame_lens, on, off, min_frames=1, max_gap=0, max_events=MAX_EVENTS) -> dict:
    """``events`` on every (clip, tag) sequence of ``frame_probs`` (B, T, n_tags) fp32 at once -- one walk over the frames with the
    state the kernel keeps (the current run, the pending merged event, the peak), vectorised over the sequences:
    {"spans": (B, n_tags, max_events, 2), "peaks", "peak_frames": (B, n_tags, max_events), "counts": (B, n_tags) int32}."""
    check_arguments(on=on, off=off, min_frames=min_frames, max_gap=max_gap, max_events=max_events)
    p = np.asarray(frame_probs)
    if p.dtype != np.float32 or p.ndim != 3:
        raise ValueError(f"Invalid argument frame_probs of dtype {p.dtype} and shape {p.shape}. (expected (B, T, n_tags) fp32)")
    bsize, t_audio, n_tags = p.shape
    n = np.clip(np.asarray(frame_lens).astype(np.int64).reshape(bsize, 1), 0, t_audio)
    on32, off32 = np.float32(on), np.float32(off)
    shape = (bsize, n_tags)
    out = _empty_tables(shape, int(max_events))
    count = np.zeros(shape, dtype=np.int32)
    in_run, hit = np.zeros(shape, dtype=bool), np.zeros(shape, dtype=bool)
    r_start, r_pf = np.zeros(shape, dtype=np.int32), np.zeros(shape, dtype=np.int32)
    r_peak = np.zeros(shape, dtype=np.float32)
    pend = np.zeros(shape, dtype=bool)
    e_start, e_end, e_pf = (np.zeros(shape, dtype=np.int32) for _ in range(3))
    e_peak = np.zeros(shape, dtype=np.float32)

    def emit(which):
        nonlocal count
        keep = which & (e_end - e_start >= min_frames)
        store = keep & (count < max_events)
        bi, ci = np.nonzero(store)
        k = count[bi, ci]
        out["spans"][bi, ci, k, 0], out["spans"][bi, ci, k, 1] = e_start[bi, ci], e_end[bi, ci]
        out["peaks"][bi, ci, k], out["peak_frames"][bi, ci, k] = e_peak[bi, ci], e_pf[bi, ci]
        count = count + keep.astype(np.int32)

    with np.errstate(invalid="ignore"):
        for t in range(t_audio + 1):
            x = p[:, t, :] if t < t_audio else np.zeros(shape, dtype=np.float32)
            above = (t < n) & (x >= off32)
            opening = above & ~in_run
            r_start = np.where(opening, t, r_start)
            hit = np.where(opening, False, hit) | (above & (x >= on32))
            better = above & (opening | (x > r_peak))
            r_peak, r_pf = np.where(better, x, r_peak), np.where(better, t, r_pf)
            closing = in_run & ~above & hit         # a run ended at t (exclusive)
            join = closing & pend & (r_start - e_end <= max_gap)
            fresh = closing & ~join
            emit(fresh & pend)
            up = join & (r_peak > e_peak)
            e_peak, e_pf = np.where(up | fresh, r_peak, e_peak), np.where(up | fresh, r_pf, e_pf)
            e_start, e_end = np.where(fresh, r_start, e_start), np.where(closing, t, e_end)
            pend = pend | closing
            in_run = above
    emit(pend)
    out["counts"] = count
    return out
