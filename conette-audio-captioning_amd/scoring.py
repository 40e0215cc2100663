"""Host side of caption scoring (``conette_score``, include/conette_hip.h): what the reference does around its forcing
logits in ``CoNeTTEPLM.validation_step`` / ``test_step`` (pl_modules/conette.py:233-336) -- split the captions into decoder
inputs and targets, replace ``<bos>`` by the task token, turn summed log-probabilities into ``CrossEntropyLossMean`` losses
(nn/loss/ce_mean.py:30-34) -- plus the clip x caption tiling of a retrieval matrix and the chunking of one large call.

Pure tensor logic: no GPU, no library (tests/test_cpu_scoring.py)."""
from __future__ import annotations

from typing import Callable, List, Optional, Tuple

import torch
from torch import Tensor

BOS_NOT_REPLACED = "BOS was not replaced in input captions for decode_method='forcing'."   # pl_modules/conette.py:404-407
SCORE_WORKSPACE_BOUND = 1 << 30   # bytes: Engine.score splits a call whose workspace would be larger (about 80 k rows in bf16)


def _as_int_captions(captions) -> Tensor:
    captions = torch.as_tensor(captions)
    if captions.is_floating_point() or captions.dtype == torch.bool or captions.ndim < 2:
        raise ValueError("captions must be an integer tensor of shape (..., caps_size) with at least two dimensions.")
    return captions


def split_captions(captions, pad_id: int) -> Tuple[Tensor, Tensor]:
    """(caps_in, targets) = (captions[..., :-1], captions[..., 1:]) as contiguous int32 (pl_modules/conette.py:241-242): position
    t of ``caps_in`` predicts ``targets[..., t]``; ``pad_id`` targets are not scored."""
    captions = _as_int_captions(captions)
    if captions.shape[-1] < 2:
        raise ValueError(f"captions of {captions.shape[-1]} token(s) have no target (first token + at least one more expected).")
    del pad_id   # (the split does not depend on it: pads stay pads on both sides)
    return captions[..., :-1].to(torch.int32).contiguous(), captions[..., 1:].to(torch.int32).contiguous()


def replace_bos(captions, bos_id: int, task_ids: Optional[Tensor]) -> Tensor:
    """Column 0 equal to ``<bos>`` becomes the caption's task token (pl_modules/conette.py:268-270); any other column-0 value
    (a task token already in place) is kept.  ``task_ids``: broadcastable to ``captions.shape[:-1]`` (one per clip for
    (B, n_caps, L) captions: shape (B, 1) or (B,) -- a (B,) tensor is read as one id per clip), or None = no task given, in
    which case a ``<bos>`` raises the reference's message."""
    captions = _as_int_captions(captions)
    first = captions[..., 0]
    is_bos = first.eq(int(bos_id))
    if task_ids is None:
        if bool(is_bos.any()):
            raise ValueError(BOS_NOT_REPLACED)
        return captions.clone()
    task_ids = torch.as_tensor(task_ids).to(captions.dtype).to(captions.device)
    if task_ids.ndim == 1 and first.ndim == 2 and task_ids.shape[0] == first.shape[0]:
        task_ids = task_ids[:, None]
    out = captions.clone()
    out[..., 0] = torch.where(is_bos, task_ids.expand_as(first), first)
    return out


def pairwise_captions(captions, n_audio: int) -> Tensor:
    """(M, L) captions -> (n_audio, M, L): every caption against every clip (the rows of a retrieval score matrix)."""
    captions = _as_int_captions(captions)
    if captions.ndim != 2:
        raise ValueError(f"pairwise scoring takes captions of shape (n_caps, caps_size), found {tuple(captions.shape)}.")
    return captions[None].expand(int(n_audio), *captions.shape).contiguous()


def losses_from(sum_lprobs: Tensor, n_tokens: Tensor) -> Tensor:
    """The reference's per-caption loss, CrossEntropyLossMean(ignore_index=pad_id, dim=1) of the forcing logits
    (nn/loss/ce_mean.py:30-34): -sum of the non-pad targets' log-probabilities / their number."""
    n_tokens = torch.as_tensor(n_tokens)
    if bool((n_tokens <= 0).any()):
        raise ValueError("a caption without any non-pad target has no loss (n_tokens == 0).")
    return -torch.as_tensor(sum_lprobs) / n_tokens.to(torch.float32)


def plan_chunks(n_audio: int, caps_per_audio: int, need: Callable[[int, int], int], bound: int) -> List[Tuple[int, int, int, int]]:
    """[(clip0, n_clips, cap0, n_caps)] covering n_audio x caps_per_audio so that ``need(n_clips, n_caps)`` (workspace bytes,
    monotone in both) stays within ``bound``: whole clips per call while one clip with all its captions fits, else one clip per
    call and its captions in slices.  One call when everything fits."""
    def largest(lo_ok: int, hi: int, fits: Callable[[int], bool]) -> int:   # largest k in [lo_ok, hi] with fits(k); fits(lo_ok) holds
        lo = lo_ok
        while lo < hi:
            mid = (lo + hi + 1) // 2
            if fits(mid):
                lo = mid
            else:
                hi = mid - 1
        return lo

    if need(1, 1) > bound:
        raise ValueError(f"scoring one caption needs {need(1, 1)} workspace bytes, above the bound of {bound}.")
    if need(1, caps_per_audio) <= bound:
        step = largest(1, n_audio, lambda k: need(k, caps_per_audio) <= bound)
        return [(i, min(step, n_audio - i), 0, caps_per_audio) for i in range(0, n_audio, step)]
    step = largest(1, caps_per_audio, lambda k: need(1, k) <= bound)
    return [(i, 1, j, min(step, caps_per_audio - j)) for i in range(n_audio) for j in range(0, caps_per_audio, step)]
