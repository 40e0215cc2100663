"""``CoNeTTEEnsemble``: several CoNeTTEModel checkpoints captioning as one -- every member's decoder scores the candidates of ONE
beam search on the device (conette_decode_ensemble, include/conette_hip.h; the rule: ensemble_search.py)."""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence, Union

import torch
from torch import Tensor

from . import ensemble_search


class CoNeTTEEnsemble:
    """``CoNeTTEEnsemble(models, weights=None, combine="logprob")(x, sr=..., task=...)``: ``forward``'s arguments and keys.

    ``models``: 1 .. 4 CoNeTTEModel on one device, of one decoder precision, whose tokenizers hold the same vocabulary (else
    ValueError); the same model may appear more than once (with ``task`` one per member: a task ensemble).  Each distinct model
    encodes the audio once; the members then decode one hypothesis tree in lockstep and the top-k runs on the combined scores
    (``combine="logprob"``: sum_m w_m log p_m, a product of experts; ``"prob"``: log sum_m w_m p_m, a mixture; ``weights`` are
    normalised to sum 1).  Beam size, caption lengths, the forbid mask, the tags and the tokenizer are the first model's.  No
    exact re-run: precision "certified*" and the mixed precisions decode on their base decoder context, and an overflow of a
    16-bit encoder raises as in ``CoNeTTEModel.caption_diverse``."""

    def __init__(self, models: Sequence[Any], weights: Optional[Sequence[float]] = None, combine: str = "logprob") -> None:
        self.models = list(models)
        self.weights, _ = ensemble_search.check_arguments(len(self.models), weights, combine, 1)
        self.combine = combine
        first = self.models[0]
        vocab = self._vocabulary(first.tokenizer)
        for i, m in enumerate(self.models[1:], 1):
            if self._vocabulary(m.tokenizer) != vocab:
                raise ValueError(f"models[{i}]: its tokenizer does not hold the vocabulary of models[0] (an ensemble shares one vocabulary)")
            if torch.device(m.device) != torch.device(first.device):
                raise ValueError(f"models[{i}] is on {m.device}, models[0] on {first.device} (an ensemble runs on one device)")
            if m.engine.precision_dec != first.engine.precision_dec:
                raise ValueError(f"models[{i}] decodes in another precision than models[0] (an ensemble shares one decoder precision)")

    @staticmethod
    def _vocabulary(tok) -> List[str]:
        return [tok.id_to_token(i) for i in range(tok.get_vocab_size())]

    def _member_tasks(self, task: Union[str, Sequence[str], None]) -> List[Optional[str]]:
        if task is None or isinstance(task, str):
            return [task] * len(self.models)
        task = list(task)
        if len(task) != len(self.models):
            raise ValueError(f"Invalid number of tasks. (found {len(task)} tasks but {len(self.models)} members: one task, or one per member)")
        return task

    @torch.no_grad()
    def forward(self, x, sr=None, x_shapes=None, preprocess: bool = True, threshold: Union[float, Tensor] = 0.3,
                task: Union[str, Sequence[str], None] = None, beam_size: Optional[int] = None, min_pred_size: Optional[int] = None,
                max_pred_size: Optional[int] = None, forbid_rep_mode: Optional[str] = None) -> Dict[str, Any]:
        first = self.models[0]
        cfg = first.config
        beam = cfg.beam_size if beam_size is None else int(beam_size)
        ensemble_search.check_arguments(len(self.models), self.weights, self.combine, beam)
        member_tasks = self._member_tasks(task)
        with torch.cuda.device(first.device):
            encoded: Dict[int, tuple] = {}
            for m in self.models:       # each distinct model encodes once
                if id(m) not in encoded:
                    keep: dict = {}
                    audio, audio_shape = m._frame_embeddings(x, sr, x_shapes, preprocess, keep)
                    m._refuse_encoder_overflow(preprocess)
                    encoded[id(m)] = (audio, torch.as_tensor(audio_shape), keep.get("clip_probs"))
            audio0, shape0, clip_probs = encoded[id(first)]
            bsize = len(audio0)
            members, names = [], []
            for m, t, w in zip(self.models, member_tasks, self.weights):
                tasks, dataset_lst, source_lst = m._split_tasks(t, bsize)
                names.append(tasks[0])
                members.append((m.engine, encoded[id(m)][0], m.batch_to_task_token_ids(dataset_lst, source_lst), float(w)))
            min_pred = cfg.min_pred_size if min_pred_size is None else int(min_pred_size)
            max_pred = cfg.max_pred_size if max_pred_size is None else int(max_pred_size)
            res = first.engine.decode_ensemble(members, shape0[:, 1].to(torch.int32), first.get_forbid_rep_mask(forbid_rep_mode), beam,
                                               min_pred, max_pred, combine=self.combine)
            return first._search_outputs(res, ["+".join(names)] * bsize, clip_probs, threshold)

    __call__ = forward
