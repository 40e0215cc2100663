"""Host side of word-to-audio alignment (``conette_align``, include/conette_hip.h): what to read off an attention map
``attn`` (..., T) -- per caption position a distribution over the clip's encoder frames -- as frames and as seconds.

One encoder frame is 32 STFT hops (the stem's stride 4, then three downsample layers of stride 2) of 320 samples at 32 kHz:
0.32 s.  Rows that are all zero (pad positions) have no peak, mean or span: -1 where the result is an index, NaN where it is a
float.

Pure tensor logic: no GPU, no library (tests/test_cpu_alignment.py)."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch
from torch import Tensor

FRAME_SEC = 32 * 320 / 32000   # seconds per encoder frame


def frame_times(n: int) -> Tensor:
    """(n,) float64: the nominal centres of frames 0 .. n - 1 in seconds, (i + 0.5) * FRAME_SEC."""
    return (torch.arange(int(n), dtype=torch.float64) + 0.5) * FRAME_SEC


def _masked(attn: Tensor, frame_lens: Optional[Tensor]) -> Tensor:
    a = torch.as_tensor(attn).double()
    if frame_lens is not None:   # (the library writes zeros behind a clip's length already; this holds for any map)
        lens = torch.as_tensor(frame_lens).to(a.device).reshape(-1, *([1] * (a.ndim - 1)))
        a = a * (torch.arange(a.shape[-1], device=a.device) < lens)
    return a


def summarize(attn: Tensor, frame_lens: Optional[Tensor] = None) -> Dict[str, Tensor]:
    """``attn`` (..., T), ``frame_lens`` (attn.shape[0],) valid frames per clip or None -> {"peak_frame": (...) int64, the arg-max
    (the lowest index among equal maxima; -1 for an all-zero row), "mean_frame": (...) float64, sum_i i * a_i / sum_i a_i (NaN for
    an all-zero row), "spread": (...) float64, the standard deviation of the frame index under a, in frames (NaN likewise)}."""
    a = _masked(attn, frame_lens)
    t = a.shape[-1]
    idx = torch.arange(t, device=a.device)
    total = a.sum(dim=-1)
    empty = total <= 0
    top = a.amax(dim=-1, keepdim=True)
    peak = torch.where(a == top, idx, t).amin(dim=-1)
    safe = torch.where(empty, torch.ones_like(total), total)
    mean = (a * idx).sum(dim=-1) / safe
    var = (a * (idx - mean[..., None]) ** 2).sum(dim=-1) / safe
    nan = torch.full_like(total, float("nan"))
    return {"peak_frame": torch.where(empty, torch.full_like(peak, -1), peak),
            "mean_frame": torch.where(empty, nan, mean), "spread": torch.where(empty, nan, var.clamp(min=0).sqrt())}


def span(attn: Tensor, mass: float = 0.5, frame_lens: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """(start, end) (...) int64 of the shortest run of consecutive frames start .. end - 1 that holds at least ``mass`` (0 < mass
    <= 1) of the row's total weight; among runs of that length the earliest.  (-1, -1) for an all-zero row."""
    if not 0.0 < float(mass) <= 1.0:
        raise ValueError(f"span: mass={mass} outside (0, 1]")
    a = _masked(attn, frame_lens)
    lead, t = a.shape[:-1], a.shape[-1]
    a = a.reshape(-1, t)
    c = torch.cat([torch.zeros_like(a[:, :1]), a.cumsum(dim=-1)], dim=-1)             # (N, T + 1) prefix sums, non-decreasing
    total = c[:, -1:]
    # a run from `start` holds the mass once the prefix sum reaches c[start] + mass * total: its first such index is the run's end
    end = torch.searchsorted(c, c[:, :-1] + float(mass) * total, side="left")         # (N, T); T + 1 = never reached
    start = torch.arange(t, device=a.device)[None]
    length = torch.where(end <= t, end - start, t + 1)
    key = (length * (t + 1) + start).amin(dim=-1)                                     # shortest first, then earliest
    s, n = key % (t + 1), key // (t + 1)
    empty = (total[:, 0] <= 0) | (n > t)
    s, e = torch.where(empty, -1, s), torch.where(empty, -1, s + n)
    return s.reshape(lead), e.reshape(lead)


def to_seconds(frames: Tensor) -> Tensor:
    """Frame positions (a boundary: ``span``'s start / end; or a fractional index: ``mean_frame``) as float64 seconds from the clip's
    start, index * FRAME_SEC; negative (absent) and NaN positions become NaN."""
    f = torch.as_tensor(frames).double()
    return torch.where(f < 0, torch.full_like(f, float("nan")), f * FRAME_SEC)


def times(attn: Tensor, frame_lens: Optional[Tensor] = None, mass: float = 0.5) -> Dict[str, Tensor]:
    """``summarize`` and ``span`` in seconds: {"peak_time": the centre of the peak frame, "mean_time": the centre of mass (a frame's
    weight sits at its centre), "span_time": (..., 2) start and end of the span}; NaN for all-zero rows."""
    s = summarize(attn, frame_lens)
    lo, hi = span(attn, mass, frame_lens)
    peak = s["peak_frame"].double()
    return {"peak_time": to_seconds(torch.where(peak < 0, peak, peak + 0.5)),
            "mean_time": to_seconds(s["mean_frame"] + 0.5), "span_time": torch.stack([to_seconds(lo), to_seconds(hi)], dim=-1)}
