"""CoNeTTEModel -- drop-in for the reference's inference API on MI355X.

Mirrors ``conette.huggingface.model.CoNeTTEModel`` (reference huggingface/model.py:38-289) and
the inference methods of ``CoNeTTEPLM`` (pl_modules/conette.py:352-525): same constructor
arguments, ``from_pretrained(name_or_dir, config=...)``, ``model(x, sr, x_shapes, preprocess,
threshold, task, beam_size, min_pred_size, max_pred_size, forbid_rep_mode)`` and the same
output dict.  All dense work runs in libconette_hip.so through ``engine.Engine``.
"""
from __future__ import annotations

import csv
import json
import logging
import math
import os
import os.path as osp
from pathlib import Path
from typing import Any, Dict, Iterable, List, Optional, Union

import torch
from torch import Size, Tensor

from .config import CoNeTTEConfig
from .engine import Engine, PREC_BF16, PREC_F16
from .preprocessor import CoNeTTEPreprocessor
from .tokenizer import AACTokenizer, ENGLISH_STOPWORDS, unpickle_extra_state

pylog = logging.getLogger(__name__)

FORBID_MODES = ("none", "all", "content_words")
# What `CoNeTTEModel.from_pretrained(dir)(x)` runs when the caller names no precision (round 6): a 16-bit base pipeline (fp16
# encoder + exact decoder: engine.CERT_DEFAULT_BASE) with the device-side id certificate -- clips whose search margins do not
# certify their token ids are re-run through the exact context from the waveform, so the ids are the reference's (fp32) ids.
# "bf16" is the benchmark's throughput mode (BASELINE configs[1-3]).
DEFAULT_PRECISION = "certified"


def load_audioset_idx_to_name(offline: bool = False, cache_path: Union[str, Path, None] = None) -> Dict[int, str]:
    """transforms/audioset_mapping.py:102-107: index -> display_name from class_labels_indices.csv."""
    if cache_path is None:  # reference default: ~/.cache/audioset_mapping (audioset_mapping.py:16-24)
        cache_path = os.environ.get("CONETTE_AUDIOSET_CACHE")
    cache = Path(cache_path) if cache_path is not None else Path.home().joinpath(".cache", "audioset_mapping")
    fpath = cache.joinpath("class_labels_indices.csv")
    if not osp.isfile(fpath):
        if offline:
            raise FileNotFoundError(
                f"Cannot find or download audioset mapping file in '{fpath}' with mode offline={offline}.")
        from torch.hub import download_url_to_file
        os.makedirs(cache, exist_ok=True)
        download_url_to_file("http://storage.googleapis.com/us_audioset/youtube_corpus/v1/csv/class_labels_indices.csv",
                             str(fpath), progress=False)
    with open(fpath, "r") as file:
        data = list(csv.DictReader(file, skipinitialspace=True, strict=True))
    return {int(d["index"]): d["display_name"] for d in data}


def probs_to_names(probs: Tensor, threshold: Union[float, Tensor], idx_to_name: Dict[int, str]) -> List[List[str]]:
    mask = (probs >= threshold).cpu()
    return [[idx_to_name[int(j)] for j in torch.where(row)[0].tolist()] for row in mask]


def _requirement_groups(tok, spec) -> List[List[int]]:
    """One clip's requirement groups from a spec: a string (split on whitespace, each word its own group) or a list whose items
    are a word, an id, or a list of alternatives.  An unknown alternative is dropped while its group keeps a known one; a group
    left empty is a ValueError that names its words."""
    if isinstance(spec, str):
        items = spec.split()
    elif isinstance(spec, (list, tuple)):
        items = list(spec)
    else:
        raise ValueError(f"a requirement spec is a string or a list of words, ids or lists of alternatives, not {type(spec).__name__}")
    groups = []
    for item in items:
        alts = list(item) if isinstance(item, (list, tuple)) else [item]
        ids: List[int] = []
        for a in alts:
            if isinstance(a, str):
                found = tok.words_to_ids(a, skip_unknown=True)
                if len(a.split()) != 1:
                    raise ValueError(f"required word {a!r}: a requirement is one word (phrases are not supported)")
                ids += found
            elif isinstance(a, bool) or not isinstance(a, int):
                raise ValueError(f"a required alternative is a word or an id, not {a!r}")
            else:
                ids.append(int(a))
        if not ids:
            raise ValueError("required word " + " | ".join(repr(a) for a in alts) + " is not in the vocabulary")
        groups.append(list(dict.fromkeys(ids)))
    return groups


def required_groups(tok, required, required_per_clip, bsize: int) -> List[List[List[int]]]:
    """Per clip the requirement groups of ``CoNeTTEModel.caption_constrained``'s ``required`` (one spec for all clips) or
    ``required_per_clip`` (a list of ``bsize`` specs, None = none for that clip); ``tok`` needs ``words_to_ids`` only."""
    if required is not None and required_per_clip is not None:
        raise ValueError("required and required_per_clip exclude each other")
    if required_per_clip is not None:
        if isinstance(required_per_clip, str) or len(required_per_clip) != bsize:
            raise ValueError(f"required_per_clip must be a list of {bsize} specs, one per clip")
        return [[] if s is None else _requirement_groups(tok, s) for s in required_per_clip]
    one = [] if required is None else _requirement_groups(tok, required)
    return [[list(g) for g in one] for _ in range(bsize)]


def _read_state_dict(path: str) -> Dict[str, Tensor]:
    st = osp.join(path, "model.safetensors")
    if osp.isfile(st):
        from safetensors.torch import load_file
        return load_file(st)
    for name in ("pytorch_model.bin", "model.pt", "model.bin"):
        fp = osp.join(path, name)
        if osp.isfile(fp):
            return torch.load(fp, map_location="cpu", weights_only=True)
    raise FileNotFoundError(f"No weights file (model.safetensors / pytorch_model.bin) in '{path}'.")


class CoNeTTEModel:
    """CoNeTTE for inference; weights live packed on the GPU inside the HIP context."""

    config_class = CoNeTTEConfig

    def __init__(self, config: CoNeTTEConfig, device: Union[str, torch.device, None] = "cuda_if_available",
                 inference: bool = True, offline: bool = False, model_override: Any = None, *,
                 state_dict: Optional[Dict[str, Tensor]] = None, precision: str = DEFAULT_PRECISION,
                 audioset_idx_to_name: Optional[Dict[int, str]] = None,
                 stopwords: Optional[Iterable[str]] = None) -> None:
        if model_override is not None:
            raise NotImplementedError("model_override (Lightning checkpoints) is not supported by the MI355X path.")
        if not inference:
            raise NotImplementedError("The MI355X path is inference-only (reference training stack is out of scope).")
        if state_dict is None:
            raise ValueError("CoNeTTEModel needs weights: use CoNeTTEModel.from_pretrained(dir) or pass state_dict=.")
        if device in ("cuda_if_available", None, "auto"):
            device = "cuda"
        self.config = config
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("conette_amd runs on a ROCm GPU only; there is no CPU fallback.")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.precision = precision
        self._stopwords = list(ENGLISH_STOPWORDS if stopwords is None else stopwords)
        self.audioset_idx_to_name = (load_audioset_idx_to_name(offline=offline) if audioset_idx_to_name is None
                                     else dict(audioset_idx_to_name))
        self.training = False
        self.last_recomputed: Optional[Tensor] = None
        self._build(dict(state_dict))

    def _build(self, state_dict: Dict[str, Tensor]) -> None:
        """module construction + load_state_dict of the reference (model.py:41-107,126-163): tokenizer from the pickled extra
        state, task tokens, forbid mask, then the packed weights inside the HIP contexts on ``self.device``."""
        config = self.config
        # non-tensor state: pickled dict in `_extra_state_` (model.py:126-139)
        tok_state = None
        if "_extra_state_" in state_dict:
            extra = unpickle_extra_state(state_dict.pop("_extra_state_"))
            tok_state = extra.get("model.tokenizers.0._extra_state")
        if tok_state is None:
            tok_state = state_dict.pop("model.tokenizers.0._extra_state", None)   # an already-unpacked state dict
        if tok_state is None:
            tok_state = config.tokenizer_state
        if tok_state is None:
            raise RuntimeError("Cannot build the model from state_dict. (tokenizer is not fit)")
        self.tokenizer = AACTokenizer.from_txt_state(tok_state)
        self._tok_state = tok_state
        # task tokens (conette.py:103-129); present in a trained tokenizer, appended otherwise
        self.task_name_to_token_id: Dict[str, int] = {}
        if config.task_mode in ("ds", "ds_src"):
            for name in config.task_names:
                token = f"<bos_{name}>"
                self.task_name_to_token_id[name] = (self.tokenizer.token_to_id(token) if self.tokenizer.has(token)
                                                    else self.tokenizer.add_special_token(token))
        elif config.task_mode != "none":
            raise ValueError(f"Invalid argument {config.task_mode=}.")
        vocab = self.tokenizer.get_vocab_size()
        cls_rows = int(state_dict["model.decoder.classifier.weight"].shape[0])
        if cls_rows != vocab:
            raise RuntimeError(f"vocab size mismatch: tokenizer {vocab} vs classifier {cls_rows}")
        if "model.task_id_to_token_id" in state_dict:
            self.task_id_to_token_id = state_dict["model.task_id_to_token_id"].to(torch.long).cpu()
        else:
            self.task_id_to_token_id = torch.as_tensor([self.task_name_to_token_id[n] for n in config.task_names])
        frm = state_dict.get("model.forbid_rep_mask")
        self.forbid_rep_mask: Optional[Tensor] = None if frm is None else frm.to(torch.bool).to(self.device)
        # the HIP path implements the published architecture only: fail loudly instead of silently running GELU / lin768
        if config.acti_name != "gelu" or config.proj_name != "lin768":
            raise ValueError(f"Unsupported config for the MI355X path: acti_name={config.acti_name!r}, "
                             f"proj_name={config.proj_name!r} (expected 'gelu' and 'lin768').")
        with torch.cuda.device(self.device):
            self.engine = Engine(state_dict, precision=self.precision, d_model=config.d_model, nhead=config.nhead,
                                 n_layers=config.num_decoder_layers, d_ff=config.dim_feedforward,
                                 pad_id=self.tokenizer.pad_token_id, bos_id=self.tokenizer.bos_token_id,
                                 eos_id=self.tokenizer.eos_token_id, device=self.device)
        self.preprocessor = CoNeTTEPreprocessor(self.engine, verbose=config.verbose)
        # the tensors the contexts were packed from, kept by reference (host memory the caller already holds) so that
        # state_dict() / save_pretrained() round-trip the reference layout (model.py:163-183)
        self._weights: Dict[str, Tensor] = {k: v for k, v in state_dict.items() if isinstance(v, Tensor)}

    # ---- construction -----------------------------------------------------------------------
    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path: str, *args, config: Optional[CoNeTTEConfig] = None,
                        **kwargs) -> "CoNeTTEModel":
        path = str(pretrained_model_name_or_path)
        if not osp.isdir(path):
            from huggingface_hub import snapshot_download  # needs network; raises offline
            path = snapshot_download(path)
        if config is None:
            config = CoNeTTEConfig.from_pretrained(path)
        return cls(config, *args, state_dict=_read_state_dict(path), **kwargs)

    # ---- PreTrainedModel surface (model.py:38,126-183): the checkpoint round trip -------------------------------------------
    def state_dict(self) -> Dict[str, Tensor]:
        """model.py:163-183: every tensor of the checkpoint the contexts were packed from (reference key names) + the non-tensor
        states -- the fitted tokenizer -- pickled into the uint8 tensor ``_extra_state_``; tensors contiguous."""
        import pickle
        out = {k: v.contiguous() for k, v in self._weights.items()}
        non_tensor = {"model.tokenizers.0._extra_state": self._tok_state}
        out["_extra_state_"] = torch.frombuffer(bytearray(pickle.dumps(non_tensor)), dtype=torch.uint8)
        return out

    def load_state_dict(self, state_dict: Dict[str, Tensor], strict: bool = True) -> "CoNeTTEModel":
        """Re-packs the HIP contexts from another checkpoint of the same layout (the pre-hook of model.py:126-161 unpickles
        ``_extra_state_`` and re-fits the tokenizer first: same here).  ``strict``: missing tensors are an error either way --
        ``conette_create`` names the first one it cannot find."""
        old = getattr(self, "engine", None)
        self._build(dict(state_dict))
        del old
        return self

    def save_pretrained(self, save_directory: str, safe_serialization: bool = True, **kwargs) -> None:
        """``config.json`` + ``model.safetensors`` (or ``pytorch_model.bin``) readable by ``from_pretrained`` here AND by the
        reference's ``CoNeTTEModel.from_pretrained`` (transformers' PreTrainedModel layout; key names are the reference's)."""
        os.makedirs(save_directory, exist_ok=True)
        self.config.save_pretrained(save_directory)
        sd = {k: v.detach().cpu() for k, v in self.state_dict().items()}
        if safe_serialization:
            from safetensors.torch import save_file
            # (safetensors refuses aliased storage: `.contiguous().clone()` for tensors that share memory)
            save_file({k: v.clone() for k, v in sd.items()}, osp.join(save_directory, "model.safetensors"), metadata={"format": "pt"})
        else:
            torch.save(sd, osp.join(save_directory, "pytorch_model.bin"))

    def to(self, device: Union[str, torch.device, None] = None, *args, **kwargs) -> "CoNeTTEModel":
        """nn.Module.to for devices: the device the contexts live on is a no-op, another ROCm GPU re-packs the weights there,
        a CPU is refused (the path has no CPU fallback); dtype arguments are ignored -- ``precision`` is chosen at construction."""
        if device is None or isinstance(device, torch.dtype):
            return self
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("conette_amd runs on a ROCm GPU only; there is no CPU fallback.")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if dev != self.device:
            self.device = dev
            self._build(self.state_dict())
        return self

    def cuda(self, device: Union[int, torch.device, None] = None) -> "CoNeTTEModel":
        return self.to("cuda" if device is None else (f"cuda:{device}" if isinstance(device, int) else device))

    def cpu(self) -> "CoNeTTEModel":
        return self.to("cpu")

    # ---- reference properties / methods (model.py:109-124) -------------------------------------
    @property
    def default_task(self) -> str:
        return next(iter(self.config.task_names))

    @property
    def tasks(self) -> List[str]:
        return list(self.config.task_names)

    def train_and_enable_grad(self, mode: bool = True) -> "CoNeTTEModel":
        if mode:
            raise NotImplementedError("The MI355X path is inference-only.")
        return self

    def eval_and_disable_grad(self, mode: bool = True) -> "CoNeTTEModel":
        return self.train_and_enable_grad(not mode)

    def eval(self) -> "CoNeTTEModel":
        return self

    # ---- helpers ---------------------------------------------------------------------------------
    def get_forbid_rep_mask(self, mode: Optional[str]) -> Optional[Tensor]:
        """pl_modules/common.py:222-299; None -> the checkpoint's persisted mask (conette.py:427-433)."""
        if mode is None:
            return self.forbid_rep_mask
        vocab = self.tokenizer.get_vocab_size()
        if mode == "none":
            return None
        if mode == "all":
            return torch.ones((vocab,), dtype=torch.bool, device=self.device)
        if mode == "content_words":
            mask = torch.ones((vocab,), dtype=torch.bool)
            for word in set(self._stopwords):
                if self.tokenizer.has(word):
                    mask[self.tokenizer.token_to_id(word)] = False
            return mask.to(self.device)
        raise ValueError(f"Invalid argument forbid_rep_mode={mode!r}. (expected one of {FORBID_MODES})")

    def batch_to_task_token_ids(self, datasets: List[str], sources: List[Optional[str]]) -> Tensor:
        """conette.py:486-525."""
        bsize = len(datasets)
        mode = self.config.task_mode
        if mode == "none":
            return torch.full((bsize,), self.tokenizer.bos_token_id, dtype=torch.long)
        task_to_idx = {name: i for i, name in enumerate(self.config.task_names)}
        if mode == "ds":
            idx = [task_to_idx[ds] for ds in datasets]
        elif mode == "ds_src":
            names = [ds if src is None else f"{ds}_{src}".lower() for ds, src in zip(datasets, sources)]
            idx = [task_to_idx[n] for n in names]
        else:
            raise ValueError(f"Invalid task mode {mode} for batch_to_task_token_ids.")
        return self.task_id_to_token_id[torch.as_tensor(idx, dtype=torch.long)]

    def _split_tasks(self, task: Union[str, List[str], None], bsize: int):
        """(tasks, datasets, sources) of a batch, with forward's errors (model.py:215-238)."""
        if task is None:
            tasks = [self.default_task] * bsize
        elif isinstance(task, str):
            tasks = [task] * bsize
        elif len(task) != bsize:
            raise ValueError(f"Invalid number of tasks with input. (found {len(task)} tasks but {bsize} elements)")
        else:
            tasks = task
        del task
        for task in tasks:
            if task not in self.config.task_names:
                raise ValueError(f"Invalid argument {tasks=}. (task {task} is not in {self.config.task_names})")
        dataset_lst = [self.default_task] * bsize
        source_lst: List[Optional[str]] = [None] * bsize
        for i, task in enumerate(tasks):
            parts = task.split("_")
            dataset_lst[i] = parts[0]
            if len(parts) >= 2:
                source_lst[i] = "_".join(parts[1:])
        return tasks, dataset_lst, source_lst

    def _encoder_overflowed(self, preprocess: bool) -> bool:
        """Did the encode that just ran overflow?  Raises unless the precision can re-run the batch exactly."""
        if not (preprocess and self.engine.precision in (PREC_BF16, PREC_F16)):
            return False
        # the fp16 residual stream of the 16-bit encoders holds |x| <= 65504; beyond it the embeddings are garbage
        # (include/conette_hip.h: conette_encode_nonfinite).  The certified precision re-runs the whole batch through
        # the exact context (fp32 stream) then; the others fail loudly.
        bad = self.engine.encode_nonfinite()
        if bad and not self.engine.certified:
            raise RuntimeError(
                f"precision={self.engine.precision_name!r}: the encoder's fp16 residual stream overflowed ({bad} "
                "positions with non-finite LayerNorm statistics); use precision='certified', 'exact' or 'fp32' for "
                "this checkpoint")
        return bad > 0

    # ---- forward (model.py:185-261) -----------------------------------------------------------------
    @torch.no_grad()
    def forward(self, x: Union[Tensor, str, Iterable[str], Iterable[Tensor]],
                sr: Union[None, int, Iterable[int]] = None, x_shapes: Union[Tensor, None, List[Size]] = None,
                preprocess: bool = True, threshold: Union[float, Tensor] = 0.3,
                task: Union[str, List[str], None] = None, beam_size: Optional[int] = None,
                min_pred_size: Optional[int] = None, max_pred_size: Optional[int] = None,
                forbid_rep_mode: Optional[str] = None) -> Dict[str, Any]:
        with torch.cuda.device(self.device):
            if preprocess:
                batch = self.preprocessor(x, sr, x_shapes)
                clip_probs = batch.pop("clip_probs")
                tags = True   # (names from the probabilities below, once the certified precision has patched re-run clips)
            else:
                assert isinstance(x, Tensor) and isinstance(x_shapes, Tensor)
                batch = {"audio": x.to(self.device), "audio_shape": x_shapes.to(self.device)}
                clip_probs, tags = None, None
            wave = batch.pop("_wave", None)

            bsize = len(batch["audio"])
            tasks, dataset_lst, source_lst = self._split_tasks(task, bsize)

            overflow = self._encoder_overflowed(preprocess)
            outs = self._generate(batch["audio"], batch["audio_shape"], dataset_lst, source_lst,
                                  beam_size=beam_size, min_pred_size=min_pred_size, max_pred_size=max_pred_size,
                                  forbid_rep_mode=forbid_rep_mode, wave=wave, recompute_all=overflow)
            outs["tasks"] = tasks
            patch = outs.pop("_clip_probs_patch", None)
            if clip_probs is not None and tags is not None:
                if patch is not None:    # certified: clips the exact context re-encoded carry its tag probabilities too
                    clip_probs.index_copy_(0, patch[0], patch[1])
                outs["tags_probs"] = clip_probs
                outs["tags"] = probs_to_names(clip_probs, threshold, self.audioset_idx_to_name)
            return outs

    def __call__(self, x, sr=None, x_shapes=None, preprocess: bool = True, threshold=0.3, task=None, beam_size=None,
                 min_pred_size=None, max_pred_size=None, forbid_rep_mode=None) -> Dict[str, Any]:
        return self.forward(x=x, sr=sr, x_shapes=x_shapes, preprocess=preprocess, threshold=threshold, task=task,
                            beam_size=beam_size, min_pred_size=min_pred_size, max_pred_size=max_pred_size,
                            forbid_rep_mode=forbid_rep_mode)

    @torch.no_grad()
    def sample(self, x, num_samples: int = 1, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0,
               seed: Optional[int] = None, generator: Optional[torch.Generator] = None, sr=None, x_shapes=None,
               preprocess: bool = True, task: Union[str, List[str], None] = None, min_pred_size: Optional[int] = None,
               max_pred_size: Optional[int] = None, forbid_rep_mode: Optional[str] = None,
               _consensus: Optional[Dict[str, Any]] = None) -> Dict[str, Any]:
        """``num_samples`` captions per clip DRAWN from the model's distribution (temperature, top-k and nucleus sampling on the
        device: conette_sample; the rule: sampling.py) instead of searched for.  ``x``, ``task`` and the size / mask arguments as
        in ``forward``, whose keys it returns: "mult_preds" (B, n, pred_size), "mult_cands", "mult_lprobs" (B, n) -- the mean
        log-probability per token, sum / length, as the beam search reports it --, "preds" / "cands" / "lprobs": per clip the
        sample with the highest mean log-probability; plus "sum_lprobs" (B, n), "lens" (B, n) and "tasks" (and the tags, when it
        ran the preprocessor).  The log-probabilities are the model's own (temperature 1, unfiltered), whatever the sampling
        settings.  ``seed`` (or a device ``generator``) makes the draw reproducible; precision "certified" samples through its
        16-bit base context, like ``teacher_forcing`` and ``score_captions``.  With waveforms in, an overflow of the 16-bit
        encoders' fp16 residual stream raises as in ``forward`` (every precision here: there is no exact re-run of a draw)."""
        n = int(num_samples)
        if n < 1:
            raise ValueError(f"Invalid argument num_samples={num_samples}. (expected at least 1)")
        with torch.cuda.device(self.device):
            if preprocess:
                batch = self.preprocessor(x, sr, x_shapes)
                clip_probs = batch.pop("clip_probs")
            elif isinstance(x, dict):
                batch, clip_probs = {"audio": x["audio"], "audio_shape": torch.as_tensor(x["audio_shape"])}, None
            else:
                assert isinstance(x, Tensor) and isinstance(x_shapes, Tensor)
                batch, clip_probs = {"audio": x.to(self.device), "audio_shape": x_shapes.to(self.device)}, None
            audio, audio_shape = batch["audio"], batch["audio_shape"]
            if audio.ndim == 4:
                audio = audio.squeeze(dim=1)
            bsize = len(audio)
            tasks, dataset_lst, source_lst = self._split_tasks(task, bsize)
            if preprocess and self.engine.precision in (PREC_BF16, PREC_F16):
                bad = self.engine.encode_nonfinite()       # (include/conette_hip.h: conette_encode_nonfinite)
                if bad:
                    raise RuntimeError(
                        f"precision={self.engine.precision_name!r}: the encoder's fp16 residual stream overflowed ({bad} "
                        "positions with non-finite LayerNorm statistics); sample with precision='exact' or 'fp32' for this checkpoint")
            cfg = self.config
            min_pred = cfg.min_pred_size if min_pred_size is None else int(min_pred_size)
            max_pred = cfg.max_pred_size if max_pred_size is None else int(max_pred_size)
            if seed is not None:
                generator = torch.Generator(device=self.device).manual_seed(int(seed))
            res = self.engine.sample(audio, audio_shape[:, 1].to(torch.int32), self.batch_to_task_token_ids(dataset_lst, source_lst),
                                     self.get_forbid_rep_mask(forbid_rep_mode), n, min_pred, max_pred, temperature=temperature,
                                     top_k=top_k, top_p=top_p, generator=generator)
            pick = None if _consensus is None else self._consensus_pick(res["preds"], res["lens"], res["sum_lprobs"], **_consensus)
            lens = res["lens"]
            mult_lprobs = res["sum_lprobs"] / lens.to(torch.float32)
            # (the first maximum, like beam.py:214-217 -- or the consensus pick)
            best = mult_lprobs.argmax(dim=1) if pick is None else pick["best"].to(torch.long)
            rows = torch.arange(bsize, device=best.device)
            sizes = torch.stack([res["sizes"][0], lens[rows, best].max()])
            if pick is None:
                pred_size, best_maxlen = (int(v) for v in sizes.tolist())  # the one host sync
            else:       # (the chosen indices come over with the sizes)
                pred_size, best_maxlen, *index = (int(v) for v in torch.cat([sizes.to(torch.long), best]).tolist())
            mult_preds = res["preds"][:, :, :pred_size].to(torch.long).contiguous()
            preds = mult_preds[rows, best][:, :best_maxlen].contiguous()
            mult_cands = self.tokenizer.decode_rec(mult_preds)
            outs = {
                "cands": self.tokenizer.decode_rec(preds) if pick is None else [mult_cands[i][j] for i, j in enumerate(index)],
                "preds": preds, "lprobs": mult_lprobs[rows, best],
                "mult_cands": mult_cands, "mult_preds": mult_preds, "mult_lprobs": mult_lprobs,
                "sum_lprobs": res["sum_lprobs"], "lens": lens, "tasks": tasks,
            }
            if clip_probs is not None:
                outs["tags_probs"] = clip_probs
                outs["tags"] = probs_to_names(clip_probs, 0.3, self.audioset_idx_to_name)
            if pick is not None:
                outs.update(self._consensus_keys(pick))
            return outs

    # ---- consensus (minimum-Bayes-risk) choice among candidates: conette_consensus; the rule: consensus.py ---------------------
    def _consensus_pick(self, mult_preds: Tensor, lens: Optional[Tensor], sum_lprobs: Optional[Tensor], utility: str = "ngram",
                        max_order: int = 4, evidence: str = "uniform", evidence_scale: float = 1.0,
                        mult_lprobs: Optional[Tensor] = None) -> Dict[str, Tensor]:
        """Engine.consensus on a table of candidates, with the evidence weights computed on the device; no host sync."""
        if evidence not in ("uniform", "model"):
            raise ValueError(f"Invalid argument evidence={evidence!r}. (expected 'uniform' or 'model')")
        if not math.isfinite(float(evidence_scale)):
            raise ValueError(f"Invalid argument evidence_scale={evidence_scale}. (expected a finite number)")
        weights = None
        if evidence == "model":
            if sum_lprobs is None:      # a search reports sum / length: the length is the tokens up to and including <eos>
                ids = mult_preds
                width = ids.shape[-1]
                pos = torch.arange(width, device=ids.device).expand_as(ids)
                length = torch.where(ids == self.engine.eos_id, pos + 1, width).amin(dim=-1)
                total = mult_lprobs.to(torch.float64) * length.to(torch.float64)
                total = torch.where(torch.isfinite(mult_lprobs), total, mult_lprobs.to(torch.float64))   # (a void slot: -inf, weight 0)
            else:
                total = sum_lprobs.to(torch.float64)
            weights = torch.softmax(float(evidence_scale) * total, dim=1)
        return self.engine.consensus(mult_preds, lens, weights, utility=utility, max_order=max_order)

    @staticmethod
    def _consensus_keys(pick: Dict[str, Tensor]) -> Dict[str, Tensor]:
        keys = {"consensus": pick["expected"], "consensus_index": pick["best"].to(torch.long), "consensus_margin": pick["margin"]}
        if "weights" in pick:
            keys["consensus_weights"] = pick["weights"]
        return keys

    @torch.no_grad()
    def select_consensus(self, outputs: Dict[str, Any], utility: str = "ngram", max_order: int = 4, evidence: str = "uniform",
                         evidence_scale: float = 1.0) -> Dict[str, Any]:
        """ONE caption per clip out of the candidates a call returned: the consensus (minimum-Bayes-risk) choice, the candidate
        that agrees most with all the others (conette_consensus on the device; the rule: consensus.py).  ``outputs`` is the dict
        of ``forward`` / ``sample`` / ``caption_diverse`` / ``caption_constrained`` / ``caption_ensemble``: its "mult_preds" are
        the candidates, cut by "lens" where present (``sample``) and at the first <eos> or pad otherwise.  ``utility`` "ngram"
        (mean n-gram F-score over the orders 1 .. ``max_order`` <= 4) or "edit" (1 - token edit distance / longer length);
        ``evidence`` "uniform" weights the candidates equally, "model" by softmax_j(``evidence_scale`` * sum of the caption's
        token log-probabilities) ("sum_lprobs" where present, else "mult_lprobs" times the caption's length), computed on the
        device; a void slot of a steered search (score -inf) weighs nothing.  Returns the same dict with "cands" / "preds" /
        "lprobs" replaced by the pick, plus "consensus" (B, N) -- every candidate's expected utility --, "consensus_index" (B,),
        "consensus_margin" (B,) and, under "model", "consensus_weights" (B, N).  At most 64 candidates of at most 64 tokens.
        Reads the B chosen indices back to pick the strings: its one host sync."""
        if "mult_preds" not in outputs:
            raise ValueError("select_consensus: outputs hold no 'mult_preds' (expected the dict of forward / sample / caption_*)")
        with torch.cuda.device(self.device):
            mult_preds = outputs["mult_preds"]
            lens = outputs.get("lens")
            pick = self._consensus_pick(mult_preds, lens, outputs.get("sum_lprobs"), utility=utility, max_order=max_order,
                                        evidence=evidence, evidence_scale=evidence_scale, mult_lprobs=outputs["mult_lprobs"])
            best = pick["best"].to(torch.long)
            bsize, _, width = mult_preds.shape
            rows = torch.arange(bsize, device=best.device)
            chosen = mult_preds[rows, best]
            if lens is not None:
                length = lens[rows, best].to(torch.long)
            else:
                pos = torch.arange(width, device=best.device).expand_as(chosen)
                length = torch.where(chosen == self.engine.eos_id, pos + 1, width).amin(dim=-1)
            best_maxlen, *index = (int(v) for v in torch.cat([length.max().reshape(1), best]).tolist())   # the one host sync
            outs = dict(outputs)
            outs["preds"] = chosen[:, :best_maxlen].to(torch.long).contiguous()
            outs["cands"] = [outputs["mult_cands"][i][j] for i, j in enumerate(index)]
            outs["lprobs"] = outputs["mult_lprobs"][rows, best]
            outs.update(self._consensus_keys(pick))
            return outs

    @torch.no_grad()
    def caption_consensus(self, x, num_samples: int = 16, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0,
                          seed: Optional[int] = None, generator: Optional[torch.Generator] = None, sr=None, x_shapes=None,
                          preprocess: bool = True, task: Union[str, List[str], None] = None, min_pred_size: Optional[int] = None,
                          max_pred_size: Optional[int] = None, forbid_rep_mode: Optional[str] = None, utility: str = "ngram",
                          max_order: int = 4, evidence: str = "uniform", evidence_scale: float = 1.0) -> Dict[str, Any]:
        """Sample-and-rerank: ``sample(x, num_samples, ...)`` followed by ``select_consensus`` on its draws, with the choice made
        on the device in between -- the chosen indices come to the host with the sizes, in ``sample``'s one host sync.  Returns
        exactly ``select_consensus(sample(...))``: "cands" / "preds" / "lprobs" are the consensus caption of each clip, the
        "mult_*" keys all the draws.  ``num_samples`` <= 64."""
        from . import consensus
        if not 1 <= int(num_samples) <= consensus.MAX_CANDS:       # (before anything is drawn)
            raise ValueError(f"Invalid argument num_samples={num_samples}: n_cands unsupported (1..{consensus.MAX_CANDS})")
        return self.sample(x, num_samples=num_samples, temperature=temperature, top_k=top_k, top_p=top_p, seed=seed,
                           generator=generator, sr=sr, x_shapes=x_shapes, preprocess=preprocess, task=task,
                           min_pred_size=min_pred_size, max_pred_size=max_pred_size, forbid_rep_mode=forbid_rep_mode,
                           _consensus=dict(utility=utility, max_order=max_order, evidence=evidence, evidence_scale=evidence_scale))

    @torch.no_grad()
    def caption_diverse(self, x, num_groups: int = 3, group_beam_size: int = 1, diversity_penalty: float = 0.5, sr=None,
                        x_shapes=None, preprocess: bool = True, task: Union[str, List[str], None] = None,
                        min_pred_size: Optional[int] = None, max_pred_size: Optional[int] = None,
                        forbid_rep_mode: Optional[str] = None, threshold: Union[float, Tensor] = 0.3) -> Dict[str, Any]:
        """``num_groups * group_beam_size`` deterministic, likely and DIFFERENT captions per clip: diverse beam search on the
        device (conette_decode_groups; the rule: group_search.py) -- the search runs in ``num_groups`` groups of
        ``group_beam_size`` beams, a group's candidates paying ``diversity_penalty`` for each time their token was already
        picked at this step by an earlier group.  ``x``, ``task`` and the size / mask arguments as in ``forward``, whose keys it
        returns: "mult_preds" (B, G * W, pred_size), "mult_cands" and "mult_lprobs" (B, G * W) hold the hypotheses group-major
        (group g at positions g * W .. g * W + W - 1), "preds" / "cands" / "lprobs" the one with the highest mean log-probability;
        the scores are the model's, never the penalised keys.  ``num_groups=1`` is ``forward`` at ``beam_size=group_beam_size``.
        Precision "certified*" and the mixed precisions run this search on the base pipeline's decoder context, with no exact
        re-run: no certificate is defined for it.  With waveforms in, an overflow of the 16-bit encoders' fp16 residual stream
        raises as in ``sample``."""
        from . import group_search
        g, w = group_search.check_arguments(num_groups, group_beam_size, diversity_penalty)
        with torch.cuda.device(self.device):
            keep: dict = {}
            audio, audio_shape = self._frame_embeddings(x, sr, x_shapes, preprocess, keep)
            audio_shape = torch.as_tensor(audio_shape)
            clip_probs = keep.get("clip_probs")
            bsize = len(audio)
            tasks, dataset_lst, source_lst = self._split_tasks(task, bsize)
            self._refuse_encoder_overflow(preprocess)
            cfg = self.config
            min_pred = cfg.min_pred_size if min_pred_size is None else int(min_pred_size)
            max_pred = cfg.max_pred_size if max_pred_size is None else int(max_pred_size)
            res = self.engine.decode_groups(audio, audio_shape[:, 1].to(torch.int32), self.batch_to_task_token_ids(dataset_lst, source_lst),
                                            self.get_forbid_rep_mask(forbid_rep_mode), g, w, float(diversity_penalty), min_pred, max_pred)
            return self._search_outputs(res, tasks, clip_probs, threshold)

    def _refuse_encoder_overflow(self, preprocess: bool) -> None:
        """After an encode of a search that has no exact re-run: an overflow of the 16-bit encoders' fp16 residual stream raises."""
        if preprocess and self.engine.precision in (PREC_BF16, PREC_F16):
            bad = self.engine.encode_nonfinite()       # (include/conette_hip.h: conette_encode_nonfinite)
            if bad:
                raise RuntimeError(
                    f"precision={self.engine.precision_name!r}: the encoder's fp16 residual stream overflowed ({bad} "
                    "positions with non-finite LayerNorm statistics); use precision='exact' or 'fp32' for this checkpoint")

    def _search_outputs(self, res: Dict[str, Tensor], tasks: List[str], clip_probs, threshold) -> Dict[str, Any]:
        """``forward``'s keys from a search's device outputs (best_* / mult_* / sizes)."""
        pred_size, best_maxlen = (int(v) for v in res["sizes"].tolist())            # the one host sync
        mult_preds = res["mult_preds"][:, :, :pred_size].to(torch.long).contiguous()
        preds = res["best_preds"][:, :best_maxlen].to(torch.long).contiguous()
        outs = {
            "cands": self.tokenizer.decode_rec(preds), "preds": preds, "lprobs": res["best_lprobs"],
            "mult_cands": self.tokenizer.decode_rec(mult_preds), "mult_preds": mult_preds, "mult_lprobs": res["mult_lprobs"],
            "tasks": tasks,
        }
        if clip_probs is not None:
            outs["tags_probs"] = clip_probs
            outs["tags"] = probs_to_names(clip_probs, threshold, self.audioset_idx_to_name)
        return outs

    @torch.no_grad()
    def caption_ensemble(self, x, tasks: Union[str, List[str]], weights: Optional[List[float]] = None, combine: str = "logprob",
                         beam_size: Optional[int] = None, sr=None, x_shapes=None, preprocess: bool = True,
                         min_pred_size: Optional[int] = None, max_pred_size: Optional[int] = None,
                         forbid_rep_mode: Optional[str] = None, threshold: Union[float, Tensor] = 0.3) -> Dict[str, Any]:
        """ONE caption per clip that several task tokens agree on: a task ensemble on the device (conette_decode_ensemble; the
        rule: ensemble_search.py).  One encode; one member per entry of ``tasks`` (1 .. 4 task names, each applied to every clip),
        all members decoding one hypothesis tree, the top-k running on the combined scores -- ``combine="logprob"``: the
        ``weights``-weighted mean of the members' log-probabilities (a product of experts), ``"prob"``: the log of the weighted mean
        of their probabilities (a mixture); ``weights`` are normalised to sum 1 (None: equal).  ``x`` and the size / mask arguments
        as in ``forward``, whose keys it returns; "tasks" holds the members' tasks joined by "+" for every clip, the scores are
        the combined ones.  With one task this is ``forward`` under that task.  Precision "certified*" and the mixed precisions run
        this search on the base pipeline's decoder context, with no exact re-run: no certificate is defined for it.  With
        waveforms in, an overflow of the 16-bit encoders' fp16 residual stream raises as in ``caption_diverse``."""
        from . import ensemble_search
        names = [tasks] if isinstance(tasks, str) else list(tasks)
        cfg = self.config
        beam = cfg.beam_size if beam_size is None else int(beam_size)
        w, _ = ensemble_search.check_arguments(len(names), weights, combine, beam)
        with torch.cuda.device(self.device):
            keep: dict = {}
            audio, audio_shape = self._frame_embeddings(x, sr, x_shapes, preprocess, keep)
            audio_shape = torch.as_tensor(audio_shape)
            bsize = len(audio)
            self._refuse_encoder_overflow(preprocess)
            members = []
            for name, wt in zip(names, w):
                _, dataset_lst, source_lst = self._split_tasks(name, bsize)
                members.append((self.engine, audio, self.batch_to_task_token_ids(dataset_lst, source_lst), float(wt)))
            min_pred = cfg.min_pred_size if min_pred_size is None else int(min_pred_size)
            max_pred = cfg.max_pred_size if max_pred_size is None else int(max_pred_size)
            res = self.engine.decode_ensemble(members, audio_shape[:, 1].to(torch.int32), self.get_forbid_rep_mask(forbid_rep_mode), beam,
                                              min_pred, max_pred, combine=combine)
            return self._search_outputs(res, ["+".join(names)] * bsize, keep.get("clip_probs"), threshold)

    def required_groups(self, required, required_per_clip, bsize: int) -> List[List[List[int]]]:
        """per clip the requirement groups (token lists) of ``caption_constrained``'s ``required`` / ``required_per_clip``"""
        return required_groups(self.tokenizer, required, required_per_clip, bsize)

    def _prefix_rows(self, prefix, bsize: int) -> List[List[int]]:
        """one token list per clip from ``caption_constrained``'s ``prefix``: None, one string, one string per clip, or padded ids"""
        if prefix is None:
            return [[] for _ in range(bsize)]
        if isinstance(prefix, str):
            return [self.tokenizer.words_to_ids(prefix)] * bsize
        if isinstance(prefix, (list, tuple)) and all(isinstance(p, str) for p in prefix):
            if len(prefix) != bsize:
                raise ValueError(f"prefix holds {len(prefix)} strings for {bsize} clips")
            return [self.tokenizer.words_to_ids(p) for p in prefix]
        ids = torch.as_tensor(prefix)
        if ids.ndim != 2 or ids.shape[0] != bsize or ids.is_floating_point():
            raise ValueError("prefix must be a string, one string per clip, or an integer tensor of shape (bsize, P) padded with pad_id")
        pad = self.tokenizer.pad_token_id
        rows = []
        for r in ids.tolist():
            n = len(r)
            while n > 0 and r[n - 1] == pad:
                n -= 1
            rows.append([int(t) for t in r[:n]])
        return rows

    @torch.no_grad()
    def caption_constrained(self, x, prefix=None, banned=None, no_repeat_ngram_size: int = 0, beam_size: Optional[int] = None, sr=None,
                            x_shapes=None, preprocess: bool = True, task: Union[str, List[str], None] = None,
                            min_pred_size: Optional[int] = None, max_pred_size: Optional[int] = None,
                            forbid_rep_mode: Optional[str] = None, threshold: Union[float, Tensor] = 0.3, *, required=None,
                            required_per_clip=None) -> Dict[str, Any]:
        """The beam search of ``forward``, steered on the device (conette_decode_constrained; the rule: constrained_search.py):
        every caption begins with ``prefix`` -- one string for all clips, one string per clip, or ids (B, P) right-padded with
        pad_id --, never holds a token of ``banned`` (words or ids) and repeats no ``no_repeat_ngram_size``-gram (0: off; the task
        token takes part).  Strings go through ``AACTokenizer.words_to_ids``: whitespace-separated vocabulary entries, not the
        reference's spaCy tokenisation.  A prefix word outside the vocabulary raises a ValueError that names it; a banned word
        outside the vocabulary is ignored.  ValueError also for a prefix that contains <eos> / <pad> / <bos> or a banned token,
        repeats a token the forbid mask allows once or an n-gram of its own, or is not shorter than ``max_pred_size``, and for a
        ban of <eos>.  Returns ``forward``'s keys; scores are the model's mean log-probabilities, prefix tokens included; a
        hypothesis slot the constraints left empty has ``mult_lprobs`` -inf and an empty caption.  Precision "certified*" and
        the mixed precisions run this search on the base pipeline's decoder context, with no exact re-run: no certificate is
        defined for it.  With waveforms in, an overflow of the 16-bit encoders' fp16 residual stream raises as in ``sample``.

        ``required`` (for all clips) or ``required_per_clip`` (a list of one spec per clip; the two exclude each other): words
        every caption must hold (conette_decode_required; the rule: required_search.py).  A spec is a string -- split on
        whitespace, each word its own requirement -- or a list whose items are a word, an id, or a list of alternatives ("dog" or
        "dogs"); at most 8 requirements and 32 tokens per clip.  An unknown alternative is dropped while its group keeps a known
        one; a group left empty is a ValueError that names the word, as is a required word that is banned, special, in two groups,
        or more requirements than ``max_pred_size`` leaves room for after the prefix.  Every caption that is returned non-empty
        then holds a word of every group, and none ends before it does.  With both None the call is what it was."""
        from . import constrained_search
        if required is not None and required_per_clip is not None:
            raise ValueError("required and required_per_clip exclude each other")
        with torch.cuda.device(self.device):
            keep: dict = {}
            audio, audio_shape = self._frame_embeddings(x, sr, x_shapes, preprocess, keep)
            audio_shape = torch.as_tensor(audio_shape)
            clip_probs = keep.get("clip_probs")
            bsize = len(audio)
            tasks, dataset_lst, source_lst = self._split_tasks(task, bsize)
            self._refuse_encoder_overflow(preprocess)
            cfg, tok = self.config, self.tokenizer
            beam = cfg.beam_size if beam_size is None else int(beam_size)
            min_pred = cfg.min_pred_size if min_pred_size is None else int(min_pred_size)
            max_pred = cfg.max_pred_size if max_pred_size is None else int(max_pred_size)
            vocab = self.engine.vocab_size
            ban = None
            if banned is not None:
                items = [banned] if isinstance(banned, (str, int)) else (banned.tolist() if isinstance(banned, Tensor) else list(banned))
                ids = [t for it in items for t in (tok.words_to_ids(it, skip_unknown=True) if isinstance(it, str) else [int(it)])]
                if any(not 0 <= t < vocab for t in ids):
                    raise ValueError(f"banned ids must lie in 0 .. {vocab - 1}")
                if tok.eos_token_id in ids:
                    raise ValueError("<eos> cannot be banned: no caption could end")
                if ids:
                    ban = torch.zeros(vocab, dtype=torch.bool)
                    ban[torch.as_tensor(ids)] = True
            rows = self._prefix_rows(prefix, bsize)
            width = max(len(r) for r in rows)
            w, n = constrained_search.check_arguments(beam, no_repeat_ngram_size, max_pred, width)
            forbid = self.get_forbid_rep_mask(forbid_rep_mode)
            bos = self.batch_to_task_token_ids(dataset_lst, source_lst)
            fb_host = None if forbid is None else forbid.cpu().numpy()
            for r, t in zip(rows, bos.tolist()):
                constrained_search.check_prefix(r, int(t), vocab_size=vocab, max_pred=max_pred, eos_id=tok.eos_token_id,
                                                pad_id=tok.pad_token_id, bos_id=tok.bos_token_id,
                                                ban=None if ban is None else ban.numpy(), forbid=fb_host, no_repeat_ngram=n)
            table = lens = None
            if width > 0:
                table = torch.full((bsize, width), tok.pad_token_id, dtype=torch.int32)
                for i, r in enumerate(rows):
                    table[i, :len(r)] = torch.as_tensor(r, dtype=torch.int32)
                lens = torch.as_tensor([len(r) for r in rows], dtype=torch.int32)
            if required is None and required_per_clip is None:
                res = self.engine.decode_constrained(audio, audio_shape[:, 1].to(torch.int32), bos, forbid, w, min_pred, max_pred,
                                                     prefix=table, prefix_lens=lens, ban_mask=ban, no_repeat_ngram=n, check=False)
            else:
                from . import required_search
                groups = required_groups(tok, required, required_per_clip, bsize)
                names = {t: tok.id_to_token(t) for r in groups for g in r for t in g if 0 <= t < min(vocab, tok.get_vocab_size())}
                groups = [required_search.check_requirements(g, int(t), vocab_size=vocab, max_pred=max_pred, eos_id=tok.eos_token_id,
                                                             pad_id=tok.pad_token_id, bos_id=tok.bos_token_id,
                                                             ban=None if ban is None else ban.numpy(), prefix=r, words=names)
                          for g, r, t in zip(groups, rows, bos.tolist())]
                rt, rg = required_search.pack_tables(groups)
                required_search.check_arguments(w, n, max_pred, width, rt.shape[1])
                res = self.engine.decode_required(audio, audio_shape[:, 1].to(torch.int32), bos, forbid, w, min_pred, max_pred,
                                                  prefix=table, prefix_lens=lens, ban_mask=ban, no_repeat_ngram=n,
                                                  req_tokens=torch.from_numpy(rt), req_groups=torch.from_numpy(rg), check=False)
            return self._search_outputs(res, tasks, clip_probs, threshold)

    def teacher_forcing(self, x, caps_in: Tensor, sr=None, x_shapes=None, preprocess: bool = True) -> Tensor:
        """CoNeTTEPLM.decode_audio(encode_audio(...), "forcing", caps_in=caps_in) (pl_modules/conette.py:392-417,
        nn/decoding/forcing.py:12-71): logits (B, vocab, cap_len) of given input captions in one causal pass.

        ``caps_in`` (B, cap_len): token ids, column 0 = the task token that replaced <bos>
        (``batch_to_task_token_ids``), right-padded with pad_id.  ``x`` as in ``forward`` (waveforms, or the
        preprocessor's output dict / (B, T, 768) embeddings with ``preprocess=False``)."""
        caps_in = torch.as_tensor(caps_in)
        if caps_in.ndim != 2 or caps_in.is_floating_point():
            raise ValueError("caps_in must be an integer tensor of shape (bsize, caps_size).")
        if bool(caps_in[:, 0].eq(self.tokenizer.bos_token_id).any()):
            raise ValueError("BOS was not replaced in input captions for decode_method='forcing'.")
        if preprocess:
            batch = self.preprocessor(x, sr, x_shapes)
            audio, audio_shape = batch["audio"], batch["audio_shape"]
        elif isinstance(x, dict):
            audio, audio_shape = x["audio"], x["audio_shape"]
        else:
            audio = x
            audio_shape = x_shapes if x_shapes is not None else torch.as_tensor([list(a.shape) for a in x])
        if audio.ndim == 4:
            audio = audio.squeeze(dim=1)
        if caps_in.shape[0] != audio.shape[0]:
            raise ValueError(f"Invalid number of captions {caps_in.shape[0]} for {audio.shape[0]} audio clips.")
        lens = torch.as_tensor(audio_shape)[:, 1].to(torch.int32)
        logits = self.engine.forcing(audio, lens, caps_in)  # (B, cap_len, V)
        return logits.permute(0, 2, 1)

    # ---- what score_captions and align_captions share: the clips' frame embeddings and the captions as rows of the engine ----
    @staticmethod
    def _check_captions(captions, pairwise: bool = False) -> Tensor:
        captions = torch.as_tensor(captions)
        if captions.is_floating_point() or captions.ndim not in ((2,) if pairwise else (2, 3)):
            raise ValueError("captions must be an integer tensor of shape (bsize, caps_size) or (bsize, n_caps, caps_size)"
                             " -- (n_caps, caps_size) with pairwise=True.")
        return captions

    def _frame_embeddings(self, x, sr, x_shapes, preprocess: bool, keep: Optional[dict] = None):
        """(audio (B, T, 768), audio_shape (B, 2)) of ``x`` as ``teacher_forcing`` takes it; ``keep`` receives the preprocessor's
        other outputs."""
        if preprocess:
            batch = self.preprocessor(x, sr, x_shapes)
            audio, audio_shape = batch["audio"], batch["audio_shape"]
            if keep is not None:
                keep.update({k: v for k, v in batch.items() if k not in ("audio", "audio_shape")})
        elif isinstance(x, dict):
            audio, audio_shape = x["audio"], x["audio_shape"]
        else:
            audio = x
            audio_shape = x_shapes if x_shapes is not None else torch.as_tensor([list(a.shape) for a in x])
        if audio.ndim == 4:
            audio = audio.squeeze(dim=1)
        return audio, audio_shape

    def _caption_rows(self, captions: Tensor, bsize: int, task, pairwise: bool = False):
        """(caps_in, targets (bsize * n_caps, size - 1) int32, n_caps, size) of full captions, <bos> replaced by the task token"""
        from . import scoring
        caps3 = scoring.pairwise_captions(captions, bsize) if pairwise else (captions[:, None] if captions.ndim == 2 else captions)
        if caps3.shape[0] != bsize:
            raise ValueError(f"Invalid number of captions {caps3.shape[0]} for {bsize} audio clips.")
        task_ids = None
        if task is not None:
            tasks = [task] * bsize if isinstance(task, str) else list(task)
            if len(tasks) != bsize:
                raise ValueError(f"Invalid number of tasks with input. (found {len(tasks)} tasks but {bsize} elements)")
            for name in tasks:
                if name not in self.config.task_names:
                    raise ValueError(f"Invalid argument {tasks=}. (task {name} is not in {self.config.task_names})")
            parts = [name.split("_") for name in tasks]
            task_ids = self.batch_to_task_token_ids([q[0] for q in parts], ["_".join(q[1:]) if len(q) >= 2 else None for q in parts])
        caps3 = scoring.replace_bos(caps3.cpu(), self.tokenizer.bos_token_id, task_ids)
        n_caps, size = int(caps3.shape[1]), int(caps3.shape[2])
        caps_in, targets = scoring.split_captions(caps3.reshape(bsize * n_caps, size), self.tokenizer.pad_token_id)
        return caps_in, targets, n_caps, size

    def score_captions(self, x, captions: Tensor, sr=None, x_shapes=None, preprocess: bool = True,
                       task: Union[str, List[str], None] = None, pairwise: bool = False) -> Dict[str, Tensor]:
        """How likely given captions are for given clips -- the quantity CoNeTTEPLM.validation_step / test_step report
        (pl_modules/conette.py:233-336: forcing logits of every reference caption -> CrossEntropyLossMean(ignore_index=pad_id,
        dim=1), nn/loss/ce_mean.py:30-34), computed without materialising logits (conette_score).

        ``x`` as in ``teacher_forcing``.  ``captions``: integer ids (B, L) or (B, n_caps, L) -- FULL captions: first token,
        words, <eos>, pad_id; with ``pairwise=True`` (M, L), every caption scored against every clip (n_caps = M: a B x M
        retrieval matrix; projection and cross-attention keys / values run once per clip).  ``task`` as in ``forward``: a
        first token equal to <bos> is replaced by the clip's task token; without a task a <bos> raises the reference's error.
        Returns {"lprobs": (B, n_caps, L - 1) per-token log-probabilities (0 at pads), "sum_lprobs" / "n_tokens": (B, n_caps),
        "losses": (B, n_caps) the reference's ``losses``, "loss": their mean}.  Precision "certified" scores through its
        16-bit base context, like ``teacher_forcing``."""
        from . import scoring
        captions = self._check_captions(captions, pairwise)
        with torch.cuda.device(self.device):
            audio, audio_shape = self._frame_embeddings(x, sr, x_shapes, preprocess)
            bsize = int(audio.shape[0])
            caps_in, targets, n_caps, size = self._caption_rows(captions, bsize, task, pairwise)
            lens = torch.as_tensor(audio_shape)[:, 1].to(torch.int32)
            res = self.engine.score(audio, lens, caps_in, targets, caps_per_audio=n_caps)
            sums, cnt = res["sum_lprobs"].reshape(bsize, n_caps), res["n_tokens"].reshape(bsize, n_caps)
            losses = scoring.losses_from(sums, cnt)
            return {"lprobs": res["tok_lprobs"].reshape(bsize, n_caps, size - 1), "sum_lprobs": sums, "n_tokens": cnt,
                    "losses": losses, "loss": losses.mean()}

    @torch.no_grad()
    def align_captions(self, x, captions: Optional[Tensor] = None, sr=None, x_shapes=None, preprocess: bool = True,
                       task: Union[str, List[str], None] = None, layers=None, per_layer: bool = False, mass: float = 0.5,
                       **search_kwargs) -> Dict[str, Any]:
        """WHERE in the clip each word of a caption is heard: the decoder's cross-attention over the encoder's 0.32 s frames,
        mean over heads and over ``layers`` (decoder layer indices; None = all), from the one causal pass that scores the
        caption (conette_align; alignment.py reads the maps).

        ``x``, ``captions`` ((B, L) or (B, n_caps, L) FULL captions) and ``task`` as in ``score_captions``.  With
        ``captions=None`` the clips are captioned first -- ``forward``'s search on the same encoder output, ``search_kwargs`` =
        its beam_size / min_pred_size / max_pred_size / forbid_rep_mode -- and each clip's best caption is aligned (task token +
        prediction through <eos>; n_caps = 1); "cands" / "preds" are returned too.
        Returns {"attn": (B, n_caps, L - 1, T) -- row t is the position that PREDICTS token t + 1, so it is labelled with it:
        "tokens" (B, n_caps, L - 1) (= the targets), "lprobs": ``score_captions``'s, "peak_time" /
        "mean_time" (B, n_caps, L - 1) and "span_time" (B, n_caps, L - 1, 2) in seconds from the clip's start (the centre of the
        strongest frame, the centre of mass, the shortest window holding ``mass`` of the weight; NaN where the token is pad_id),
        "frame_sec",
        "sum_lprobs", "n_tokens" [, "attn_layers": (n_layers, B, n_caps, L - 1, T) with ``per_layer``]}.  Precision "certified"
        aligns through its 16-bit base context, like ``score_captions``."""
        from . import alignment
        if captions is not None:
            if search_kwargs:
                raise TypeError(f"align_captions: {sorted(search_kwargs)} belong to the search, which given captions do not run")
            captions = self._check_captions(captions)
        with torch.cuda.device(self.device):
            extra: Dict[str, Any] = {}
            audio, audio_shape = self._frame_embeddings(x, sr, x_shapes, preprocess, keep=extra)
            audio_shape = torch.as_tensor(audio_shape)
            bsize = int(audio.shape[0])
            outs: Dict[str, Any] = {}
            if captions is None:
                tasks, dataset_lst, source_lst = self._split_tasks(task, bsize)
                gen = self._generate(audio, audio_shape.to(audio.device), dataset_lst, source_lst, wave=extra.get("_wave"),
                                     recompute_all=self._encoder_overflowed(preprocess), **search_kwargs)
                gen.pop("_clip_probs_patch", None)
                outs.update(cands=gen["cands"], preds=gen["preds"], tasks=tasks)
                preds = gen["preds"].cpu()
                ended = (preds == self.tokenizer.eos_token_id).long().cumsum(dim=1) - (preds == self.tokenizer.eos_token_id).long()
                preds = torch.where(ended > 0, torch.full_like(preds, self.tokenizer.pad_token_id), preds)   # nothing after <eos>
                first = self.batch_to_task_token_ids(dataset_lst, source_lst).cpu().to(preds.dtype)
                captions, task = torch.cat([first[:, None], preds], dim=1), None
            caps_in, targets, n_caps, size = self._caption_rows(captions, bsize, task)
            lens = audio_shape[:, 1].to(torch.int32)
            res = self.engine.align(audio, lens, caps_in, targets, caps_per_audio=n_caps, layers=layers, per_layer=per_layer)
            t = int(audio.shape[1])
            attn = res["attn"].reshape(bsize, n_caps, size - 1, t)
            tokens = targets.reshape(bsize, n_caps, size - 1).to(attn.device)
            labelled = attn * tokens.ne(self.tokenizer.pad_token_id)[..., None]   # (a row that predicts a pad has no word to place)
            outs.update(attn=attn, tokens=tokens,
                        lprobs=res["tok_lprobs"].reshape(bsize, n_caps, size - 1),
                        sum_lprobs=res["sum_lprobs"].reshape(bsize, n_caps), n_tokens=res["n_tokens"].reshape(bsize, n_caps),
                        frame_sec=alignment.FRAME_SEC, **alignment.times(labelled, lens.to(attn.device), mass))
            if per_layer:
                outs["attn_layers"] = res["attn_layers"].reshape(-1, bsize, n_caps, size - 1, t)
            return outs

    def _tag_indices(self, tags) -> Optional[set]:
        """the indices a ``tags=`` filter of names or indices keeps (None: all)"""
        if tags is None:
            return None
        by_name = {name: idx for idx, name in self.audioset_idx_to_name.items()}
        wanted = set()
        for tag in ([tags] if isinstance(tags, (str, int)) else tags):
            if isinstance(tag, str):
                if tag not in by_name:
                    raise ValueError(f"Invalid argument tags: unknown AudioSet tag name {tag!r}.")
                wanted.add(int(by_name[tag]))
            elif isinstance(tag, bool) or int(tag) != tag or not 0 <= int(tag) < 527:
                raise ValueError(f"Invalid argument tags: unknown AudioSet tag index {tag!r}. (expected 0..526 or a name)")
            else:
                wanted.add(int(tag))
        return wanted

    @torch.no_grad()
    def tag_timeline(self, x, window_s: float = 2.24, threshold: float = 0.3, off_threshold: Optional[float] = None,
                     min_duration_s: float = 0.0, max_gap_s: float = 0.0, max_events: int = 16, tags=None, sr=None, x_shapes=None,
                     preprocess: bool = True) -> Dict[str, Any]:
        """WHEN each AudioSet tag is heard in a clip -- sound event detection with the model as shipped, the tag-side counterpart
        of ``align_captions``: the clip head (max + mean over time, LayerNorm, head_audioset, sigmoid) pooled over a window of
        ``window_s`` seconds around every 0.32 s frame of the encoder instead of over the whole clip (conette_tag_frames), and the
        frames of every tag gathered into events on the device (conette_tag_events; both rules: tagging.py).

        ``x`` as in ``score_captions``.  A frame opens an event of a tag where its probability reaches ``threshold``; the event
        extends over the neighbouring frames that stay at or above ``off_threshold`` (None: = ``threshold``, plain thresholding);
        events of one tag at most ``max_gap_s`` apart are merged, then those shorter than ``min_duration_s`` are dropped (seconds,
        rounded half up to frames).  Returns {"frame_probs": (B, T, 527) on the device, rows beyond a clip's frames zero,
        "frame_lens": (B,), "frame_sec", "event_counts": (B, 527) -- the true numbers --, "events_truncated": (B,) bool, true where
        a tag has more than the ``max_events`` (1 .. 64) events kept, "events": per clip a list of {"tag", "index", "onset",
        "offset", "peak", "peak_time"} (seconds from the clip's start; "peak_time" is the centre of the strongest frame) sorted by
        (onset, index) [, "tags_probs", "tags": ``forward``'s, when the call ran the preprocessor]}.  ``tags`` (names or indices)
        filters the "events" list only: the device computes all 527.  The event tables come to the host in one transfer.
        Precision "certified" runs on its 16-bit base context, like ``score_captions``."""
        import numpy as np
        from . import alignment, tagging
        window, shortest, gap = tagging.window_frames(window_s), tagging.min_frames(min_duration_s), tagging.gap_frames(max_gap_s)
        off = threshold if off_threshold is None else off_threshold
        tagging.check_arguments(window=window, on=threshold, off=off, min_frames=shortest, max_gap=gap, max_events=max_events)
        wanted = self._tag_indices(tags)
        with torch.cuda.device(self.device):
            keep: Dict[str, Any] = {}
            audio, audio_shape = self._frame_embeddings(x, sr, x_shapes, preprocess, keep)
            self._refuse_encoder_overflow(preprocess)
            lens = torch.as_tensor(audio_shape)[:, 1].to(torch.int32)
            probs = self.engine.tag_frames(audio, lens, window)
            ev = self.engine.tag_events(probs, lens, threshold, off, shortest, gap, max_events)
            bsize, m = int(probs.shape[0]), int(max_events)
            n_tags = int(probs.shape[2])
            # one transfer: per (clip, tag) its count, then the spans, the peaks' bits and the peak frames of its slots
            table = torch.cat([ev["counts"].reshape(bsize, n_tags, 1), ev["spans"].reshape(bsize, n_tags, 2 * m),
                               ev["peaks"].view(torch.int32), ev["peak_frames"]], dim=2).cpu().numpy()
            counts = table[:, :, 0]
            spans = table[:, :, 1:1 + 2 * m].reshape(bsize, n_tags, m, 2)
            peaks = np.ascontiguousarray(table[:, :, 1 + 2 * m:1 + 3 * m]).view(np.float32)
            peak_frames = table[:, :, 1 + 3 * m:]
            events: List[List[Dict[str, Any]]] = []
            for b in range(bsize):
                found = []
                for c, k in zip(*np.nonzero(spans[b, :, :, 0] >= 0)):
                    if wanted is not None and int(c) not in wanted:
                        continue
                    found.append({"tag": self.audioset_idx_to_name.get(int(c), str(int(c))), "index": int(c),
                                  "onset": int(spans[b, c, k, 0]) * alignment.FRAME_SEC, "offset": int(spans[b, c, k, 1]) * alignment.FRAME_SEC,
                                  "peak": float(peaks[b, c, k]), "peak_time": (int(peak_frames[b, c, k]) + 0.5) * alignment.FRAME_SEC})
                found.sort(key=lambda e: (e["onset"], e["index"]))
                events.append(found)
            outs = {"frame_probs": probs, "frame_lens": lens, "frame_sec": alignment.FRAME_SEC, "event_counts": ev["counts"],
                    "events_truncated": torch.from_numpy((counts > m).any(axis=1)), "events": events}
            clip_probs = keep.get("clip_probs")
            if clip_probs is not None:
                outs["tags_probs"] = clip_probs
                outs["tags"] = probs_to_names(clip_probs, threshold, self.audioset_idx_to_name)
            return outs

    # ---- caption timeline: captions of spans of recordings encoded once (conette_decode_spans) and their merge into segments
    # (conette_segments); the grid and the rule: segments.py
    def _span_search(self, audio, lens_h, table, tasks, dataset_lst, source_lst, beam_size, min_pred_size, max_pred_size, forbid_rep_mode):
        """One decode_spans over ``table`` (S, 3); (device outputs, pred_size, best_maxlen)"""
        cfg = self.config
        beam = cfg.beam_size if beam_size is None else int(beam_size)
        min_pred = cfg.min_pred_size if min_pred_size is None else int(min_pred_size)
        max_pred = cfg.max_pred_size if max_pred_size is None else int(max_pred_size)
        bos = self.batch_to_task_token_ids(dataset_lst, source_lst)[torch.from_numpy(table[:, 0].astype("int64"))]
        res = self.engine.decode_spans(audio, torch.from_numpy(lens_h), table, bos, self.get_forbid_rep_mask(forbid_rep_mode), beam,
                                       min_pred, max_pred)
        pred_size, best_maxlen = (int(v) for v in res["sizes"].tolist())
        return res, pred_size, best_maxlen

    @staticmethod
    def _span_list(spans) -> List[List[tuple]]:
        """``caption_spans``' argument as frames: per recording a list of (start, len); ValueError for what no recording can hold"""
        from . import segments
        if spans is None or isinstance(spans, (str, bytes)) or len(spans) == 0:
            raise ValueError("Invalid argument spans: expected, per recording, a list of (onset_s, offset_s) in seconds.")
        out = []
        for r, rows in enumerate(spans):
            rows = list(rows)
            if not rows:
                raise ValueError(f"Invalid argument spans: recording {r} has no span.")
            conv = []
            for k, row in enumerate(rows):
                if len(row) != 2:
                    raise ValueError(f"Invalid argument spans: spans[{r}][{k}]={row!r} is not an (onset_s, offset_s) pair.")
                try:
                    conv.append(segments.seconds_to_span(row[0], row[1]))
                except ValueError as e:
                    raise ValueError(f"Invalid argument spans: spans[{r}][{k}]: {e}") from None
            out.append(conv)
        return out

    @torch.no_grad()
    def caption_spans(self, x, spans, task: Union[str, List[str], None] = None, beam_size: Optional[int] = None,
                      min_pred_size: Optional[int] = None, max_pred_size: Optional[int] = None, forbid_rep_mode: Optional[str] = None,
                      sr=None, x_shapes=None, preprocess: bool = True) -> Dict[str, Any]:
        """Captions of given spans of (long) recordings: one encode, then ONE beam search whose clips are the spans
        (conette_decode_spans): the projection and the cross-attention keys / values run once per recording frame, however many
        spans hold it.  ``x`` as in ``score_captions``; ``spans`` holds, per recording, a list of (onset_s, offset_s) in seconds
        from the recording's start -- for instance the events of ``tag_timeline`` -- rounded half up to 0.32 s frames, at least one
        frame each; an offset beyond the recording's end is cut there, an onset at or beyond it raises.  ``task`` (one per
        recording) and the search arguments as in ``forward``.  Returns ``forward``'s keys per recording as lists over its spans --
        "cands", "mult_cands": lists of strings; "preds" (n_r, best_maxlen), "lprobs" (n_r,), "mult_preds" (n_r, beam, pred_size),
        "mult_lprobs" (n_r, beam): tensors per recording --, "tasks", and "span_frames": per recording an (n_r, 2) tensor of
        (start, len) in frames.  A span's caption sees the encoder's context beyond the span (its receptive field covers several
        seconds): it is not the caption of the cut waveform.  Precision "certified" runs on its 16-bit base context, with no exact
        re-run, like ``score_captions``; an overflow of the 16-bit encoders raises as in ``tag_timeline``."""
        import numpy as np
        frames = CoNeTTEModel._span_list(spans)
        with torch.cuda.device(self.device):
            audio, audio_shape = self._frame_embeddings(x, sr, x_shapes, preprocess)
            self._refuse_encoder_overflow(preprocess)
            bsize = int(audio.shape[0])
            if len(frames) != bsize:
                raise ValueError(f"Invalid argument spans: {len(frames)} lists of spans for {bsize} recordings.")
            tasks, dataset_lst, source_lst = self._split_tasks(task, bsize)
            lens_h = torch.as_tensor(audio_shape)[:, 1].to(torch.int32).cpu().numpy()
            rows = []
            for r, conv in enumerate(frames):
                for k, (start, ln) in enumerate(conv):
                    if start >= int(lens_h[r]):
                        raise ValueError(f"Invalid argument spans: spans[{r}][{k}] starts at frame {start}, at or beyond the "
                                         f"{int(lens_h[r])} frames of recording {r}.")
                    rows.append((r, start, min(ln, int(lens_h[r]) - start)))
            table = np.asarray(rows, dtype=np.int32)
            res, pred_size, best_maxlen = self._span_search(audio, lens_h, table, tasks, dataset_lst, source_lst, beam_size,
                                                            min_pred_size, max_pred_size, forbid_rep_mode)
            preds = res["best_preds"][:, :best_maxlen].to(torch.long).contiguous()
            mult_preds = res["mult_preds"][:, :, :pred_size].to(torch.long).contiguous()
            cands, mult_cands = self.tokenizer.decode_rec(preds), self.tokenizer.decode_rec(mult_preds)
            bounds = np.concatenate([[0], np.cumsum([len(c) for c in frames])]).tolist()
            cut = lambda v: [v[bounds[r]:bounds[r + 1]] for r in range(bsize)]
            return {"cands": cut(cands), "preds": cut(preds), "lprobs": cut(res["best_lprobs"]), "mult_cands": cut(mult_cands),
                    "mult_preds": cut(mult_preds), "mult_lprobs": cut(res["mult_lprobs"]), "tasks": tasks,
                    "span_frames": cut(torch.from_numpy(table[:, 1:].copy()))}

    @torch.no_grad()
    def caption_segments(self, x, window_s: float = 10.0, hop_s: float = 5.0, merge_threshold: Optional[float] = 0.5,
                         utility: str = "ngram", max_order: int = 4, max_run_s: float = 0.0, max_segments: int = 64,
                         task: Union[str, List[str], None] = None, beam_size: Optional[int] = None,
                         min_pred_size: Optional[int] = None, max_pred_size: Optional[int] = None,
                         forbid_rep_mode: Optional[str] = None, threshold: Union[float, Tensor] = 0.3, sr=None, x_shapes=None,
                         preprocess: bool = True) -> Dict[str, Any]:
        """Captions over time -- WHAT is heard WHEN in a long recording, the caption-side counterpart of ``tag_timeline``.  The
        recording is encoded once; windows of ``window_s`` seconds every ``hop_s`` seconds over each recording's own frames (the
        last window aligned to its end; the grid: segments.py) are captioned by one beam search over all recordings' windows
        (conette_decode_spans), and neighbouring windows whose captions agree are merged into segments on the device
        (conette_segments): window k + 1 joins the run of window k iff the ``utility`` ("ngram" with ``max_order`` 1 .. 4, or "edit":
        ``select_consensus``'s pair utilities) of their two captions is at least ``merge_threshold``; a run never grows beyond
        ``max_run_s`` seconds (0: no cap).  ``merge_threshold=None``: one segment per window.  A segment carries the caption of its
        most likely window; two neighbouring segments meet in the middle of the overlap of the windows on either side.

        ``x`` as in ``score_captions``; ``task`` and the search arguments as in ``forward``.  Returns {"segments": per recording a
        list, in time order, of {"onset", "offset" (seconds from the recording's start), "caption", "pred" (ids), "lprob",
        "agreement" (the smallest utility between neighbouring windows of the segment, 1 for a single window), "windows":
        (first, end)}; "window_cands", "window_preds", "window_lprobs", "window_times": per recording the windows' captions, ids
        (n_r, best_maxlen), scores (n_r,) and (onset, offset) seconds; "adjacency": (N, Wmax - 1) the utilities of neighbouring
        windows (zeros beyond a recording's windows); "segment_counts": (N,) the true numbers; "segments_truncated": (N,) bool, true
        where a recording has more than the ``max_segments`` (1 .. 256) segments kept; "frame_sec" [, "tags_probs", "tags":
        ``forward``'s, with ``threshold``, when the call ran the preprocessor]}.  The tables come to the host in one transfer.

        The defaults -- 10 s windows, 5 s hop, threshold 0.5 -- are UNTUNED: no trained checkpoint was available to choose them on.
        A window's caption sees the encoder's context beyond the window (its receptive field covers several seconds), so it is not
        the caption of the cut waveform.  A recording the encoder refuses raises the library's error: nothing is chunked silently.
        Precision "certified" runs on its 16-bit base context, with no exact re-run, like ``score_captions``; an overflow of the
        16-bit encoders raises as in ``tag_timeline``."""
        import numpy as np
        from . import alignment, segments
        window, hop = segments.window_frames(window_s), segments.hop_frames(hop_s)
        max_run = 1 if merge_threshold is None else segments.run_windows(max_run_s, window, hop)
        thr = 0.0 if merge_threshold is None else float(merge_threshold)
        segments.check_arguments(1, 1, utility, max_order, thr, max_run, max_segments)
        sec = alignment.FRAME_SEC
        with torch.cuda.device(self.device):
            keep: Dict[str, Any] = {}
            audio, audio_shape = self._frame_embeddings(x, sr, x_shapes, preprocess, keep)
            self._refuse_encoder_overflow(preprocess)
            bsize = int(audio.shape[0])
            tasks, dataset_lst, source_lst = self._split_tasks(task, bsize)
            lens_h = torch.as_tensor(audio_shape)[:, 1].to(torch.int32).cpu().numpy()
            if lens_h.min() < 1:
                raise ValueError("caption_segments: a recording without a frame")
            table, n_win = segments.span_table(lens_h, window, hop)
            wmax = int(n_win.max())
            segments.check_arguments(1, wmax, utility, max_order, thr, max_run, max_segments)   # (the window count)
            res, pred_size, best_maxlen = self._span_search(audio, lens_h, table, tasks, dataset_lst, source_lst, beam_size,
                                                            min_pred_size, max_pred_size, forbid_rep_mode)
            # the windows as (N, Wmax) tables: window k of recording r is row bounds[r] + k of the search
            bounds = np.concatenate([[0], np.cumsum(n_win)]).astype(np.int64)
            slot = np.concatenate([np.arange(w, dtype=np.int64) + r * wmax for r, w in enumerate(n_win.tolist())])
            slot_d = torch.from_numpy(slot).to(self.device)
            max_pred = int(res["best_preds"].shape[1])
            ids = torch.full((bsize * wmax, max_pred), self.tokenizer.pad_token_id, dtype=torch.int32, device=self.device)
            ids.index_copy_(0, slot_d, res["best_preds"])
            lp = torch.zeros((bsize * wmax,), dtype=torch.float32, device=self.device)
            lp.index_copy_(0, slot_d, res["best_lprobs"])
            sp = torch.zeros((bsize * wmax, 2), dtype=torch.int32)
            sp[torch.from_numpy(slot)] = torch.from_numpy(table[:, 1:].copy())
            m = int(max_segments)
            seg = self.engine.segments(ids.view(bsize, wmax, max_pred), torch.from_numpy(n_win), lp.view(bsize, wmax),
                                       sp.view(bsize, wmax, 2), utility=utility, max_order=max_order, threshold=thr, max_run=max_run,
                                       max_segments=m)
            # one transfer: per recording its count, the segments' windows, frames, representatives and agreement bits, the adjacency bits
            # and the windows' score bits
            tab = torch.cat([seg["counts"].reshape(bsize, 1), seg["seg_windows"].reshape(bsize, 2 * m), seg["seg_frames"].reshape(bsize, 2 * m),
                             seg["seg_rep"], seg["seg_agree"].view(torch.int32), seg["adjacency"].view(torch.int32),
                             lp.view(bsize, wmax).view(torch.int32)], dim=1).cpu().numpy()
            counts = tab[:, 0]
            seg_w = tab[:, 1:1 + 2 * m].reshape(bsize, m, 2)
            seg_f = tab[:, 1 + 2 * m:1 + 4 * m].reshape(bsize, m, 2)
            seg_rep = tab[:, 1 + 4 * m:1 + 5 * m]
            seg_agree = np.ascontiguousarray(tab[:, 1 + 5 * m:1 + 6 * m]).view(np.float32)
            adjacency = np.ascontiguousarray(tab[:, 1 + 6 * m:wmax + 6 * m]).view(np.float32)
            lprobs_h = torch.from_numpy(np.ascontiguousarray(tab[:, wmax + 6 * m:]).view(np.float32).reshape(-1)[slot].copy())
            preds = res["best_preds"][:, :best_maxlen].to(torch.long).contiguous()
            cands = self.tokenizer.decode_rec(preds)
            cut = lambda v: [v[int(bounds[r]):int(bounds[r + 1])] for r in range(bsize)]
            w_cands, w_preds, w_lprobs = cut(cands), cut(preds), cut(lprobs_h)
            found: List[List[Dict[str, Any]]] = []
            for r in range(bsize):
                rows = []
                for k in range(min(int(counts[r]), m)):
                    rep = int(seg_rep[r, k])
                    rows.append({"onset": int(seg_f[r, k, 0]) * sec, "offset": int(seg_f[r, k, 1]) * sec, "caption": w_cands[r][rep],
                                 "pred": w_preds[r][rep], "lprob": float(w_lprobs[r][rep]), "agreement": float(seg_agree[r, k]),
                                 "windows": (int(seg_w[r, k, 0]), int(seg_w[r, k, 1]))})
                found.append(rows)
            times = [[(int(a) * sec, (int(a) + int(b)) * sec) for a, b in table[int(bounds[r]):int(bounds[r + 1]), 1:]] for r in range(bsize)]
            outs = {"segments": found, "window_cands": w_cands, "window_preds": w_preds, "window_lprobs": w_lprobs, "window_times": times,
                    "window_frames": cut(torch.from_numpy(table[:, 1:].copy())), "adjacency": torch.from_numpy(adjacency.copy()),
                    "segment_counts": torch.from_numpy(counts.copy()), "segments_truncated": torch.from_numpy(counts > m),
                    "frame_sec": sec, "tasks": tasks}
            clip_probs = keep.get("clip_probs")
            if clip_probs is not None:
                outs["tags_probs"] = clip_probs
                outs["tags"] = probs_to_names(clip_probs, threshold, self.audioset_idx_to_name)
            return outs

    def greedy_search(self, x, sr=None, x_shapes=None, preprocess: bool = True, bos_id: Optional[int] = None,
                      min_pred_size: Optional[int] = None, max_pred_size: Optional[int] = None,
                      forbid_rep_mode: Optional[str] = None) -> Tensor:
        """nn/decoding/greedy.py:17-131 (the decoder of BaselinePLM, baseline.py:339-401): the arg-max chain, returned
        as the masked logits of every step, (B, vocab, pred_size).  ``bos_id`` defaults to the plain <bos> token
        (BaselinePLM has no task token); pass a task token id for CoNeTTE-style prompting."""
        if preprocess:
            batch = self.preprocessor(x, sr, x_shapes)
            audio, audio_shape = batch["audio"], batch["audio_shape"]
        elif isinstance(x, dict):
            audio, audio_shape = x["audio"], x["audio_shape"]
        else:
            audio = x
            audio_shape = x_shapes if x_shapes is not None else torch.as_tensor([list(a.shape) for a in x])
        if audio.ndim == 4:
            audio = audio.squeeze(dim=1)
        cfg = self.config
        min_pred = cfg.min_pred_size if min_pred_size is None else int(min_pred_size)
        max_pred = cfg.max_pred_size if max_pred_size is None else int(max_pred_size)
        bos = torch.full((audio.shape[0],), self.tokenizer.bos_token_id if bos_id is None else int(bos_id), dtype=torch.int32)
        lens = torch.as_tensor(audio_shape)[:, 1].to(torch.int32)
        res = self.engine.greedy(audio, lens, bos, self.get_forbid_rep_mask(forbid_rep_mode), min_pred, max_pred)
        return res["logits"].permute(0, 2, 1)

    def decode_audio(self, encoder_outs: Dict[str, Tensor], decode_method: str, **kwargs) -> Any:
        """The decode_audio surface shared by CoNeTTEPLM (pl_modules/conette.py:386-450) and BaselinePLM
        (pl_modules/baseline.py:339-401): ``encoder_outs`` = the preprocessor's output ({"audio": (B, T, 768),
        "audio_shape": (B, 2)}; the projection of conette.py:457 / baseline.py:409 runs inside the engine),
        ``decode_method`` in ("forcing", "greedy", "generate", "sample").

        * "forcing": ``caps_in`` required -> logits (B, vocab, cap_len)
        * "greedy": kwargs bos_id (default <bos>: BaselinePLM has no task token), min_pred_size, max_pred_size,
          forbid_rep_mode -> logits (B, vocab, pred_size)
        * "generate": kwargs bos_id (int or (B,) tensor; REQUIRED for CoNeTTE-style task prompting, default <bos>),
          beam_size, min_pred_size, max_pred_size, forbid_rep_mode -> (preds, lprobs, mult_preds, mult_lprobs)
        * "sample": the keyword arguments of ``sample`` (num_samples, temperature, top_k, top_p, seed, task ...) -> its dict"""
        if decode_method == "forcing":
            if "caps_in" not in kwargs:
                raise ValueError(f"Please provide a 'caps_in' keyword argument with {decode_method=}. "
                                 f"(found {tuple(kwargs.keys())})")
            return self.teacher_forcing(encoder_outs, kwargs["caps_in"], preprocess=False)
        if decode_method == "greedy":
            return self.greedy_search(encoder_outs, preprocess=False, bos_id=kwargs.get("bos_id"),
                                      min_pred_size=kwargs.get("min_pred_size"), max_pred_size=kwargs.get("max_pred_size"),
                                      forbid_rep_mode=kwargs.get("forbid_rep_mode"))
        if decode_method == "sample":   # kwargs of CoNeTTEModel.sample -> its dict
            return self.sample(encoder_outs, preprocess=False, **kwargs)
        if decode_method == "generate":
            audio, audio_shape = encoder_outs["audio"], torch.as_tensor(encoder_outs["audio_shape"])
            if audio.ndim == 4:
                audio = audio.squeeze(dim=1)
            cfg = self.config
            bos = kwargs.get("bos_id")
            if bos is None:
                bos = self.tokenizer.bos_token_id
            bos = torch.as_tensor(bos, dtype=torch.int32).reshape(-1)
            if bos.numel() == 1:
                bos = bos.expand(audio.shape[0])
            beam = cfg.beam_size if kwargs.get("beam_size") is None else int(kwargs["beam_size"])
            min_pred = cfg.min_pred_size if kwargs.get("min_pred_size") is None else int(kwargs["min_pred_size"])
            max_pred = cfg.max_pred_size if kwargs.get("max_pred_size") is None else int(kwargs["max_pred_size"])
            if self.engine.certified:
                res = self.engine.generate_certified(None, audio, audio_shape[:, 1].to(torch.int32), bos.contiguous(),
                                                     self.get_forbid_rep_mask(kwargs.get("forbid_rep_mode")), beam, min_pred,
                                                     max_pred)
            else:
                res = self.engine.decode(audio, audio_shape[:, 1].to(torch.int32), bos.contiguous(),
                                         self.get_forbid_rep_mask(kwargs.get("forbid_rep_mode")), beam, min_pred, max_pred)
            pred_size, best_maxlen = (int(v) for v in res["sizes"].tolist())
            return (res["best_preds"][:, :best_maxlen].to(torch.long).contiguous(), res["best_lprobs"],
                    res["mult_preds"][:, :, :pred_size].to(torch.long).contiguous(), res["mult_lprobs"])
        raise ValueError(f"Unknown argument {decode_method=}. (expected one of ('forcing', 'greedy', 'generate', 'sample'))")

    def _generate(self, audio: Tensor, audio_shape: Tensor, datasets: List[str], sources: List[Optional[str]], *,
                  beam_size=None, min_pred_size=None, max_pred_size=None, forbid_rep_mode=None,
                  wave: Optional[Tensor] = None, recompute_all: bool = False) -> Dict[str, Any]:
        """CoNeTTEPLM.forward("generate") = encode_audio + decode_audio + decode_text (conette.py:352-450)."""
        if audio.ndim == 4:  # FrameIdentEncoder (nn/encoders/ident.py:19-21)
            audio = audio.squeeze(dim=1)
        cfg = self.config
        beam = cfg.beam_size if beam_size is None else int(beam_size)
        min_pred = cfg.min_pred_size if min_pred_size is None else int(min_pred_size)
        max_pred = cfg.max_pred_size if max_pred_size is None else int(max_pred_size)
        assert beam > 0 and min_pred >= 0
        lens = audio_shape[:, 1].to(torch.int32)
        bos = self.batch_to_task_token_ids(datasets, sources)
        if self.engine.certified:   # base-precision search + margins; uncertified clips re-run through the exact context
            res = self.engine.generate_certified(wave, audio, lens, bos, self.get_forbid_rep_mask(forbid_rep_mode), beam,
                                                 min_pred, max_pred, tol=(float("inf"), 0.0, 0.0) if recompute_all else None)
        else:
            res = self.engine.decode(audio, lens, bos, self.get_forbid_rep_mask(forbid_rep_mode), beam, min_pred, max_pred)
        self.last_recomputed = res.get("recomputed")   # certified: (B,) bool, the clips the exact context re-ran
        pred_size, best_maxlen = (int(v) for v in res["sizes"].tolist())  # the one host sync of the path
        preds = res["best_preds"][:, :best_maxlen].to(torch.long).contiguous()
        mult_preds = res["mult_preds"][:, :, :pred_size].to(torch.long).contiguous()
        out = {
            "cands": self.tokenizer.decode_rec(preds), "preds": preds, "lprobs": res["best_lprobs"],
            "mult_cands": self.tokenizer.decode_rec(mult_preds), "mult_preds": mult_preds,
            "mult_lprobs": res["mult_lprobs"],
        }
        if "recomputed_clip_probs" in res:
            out["_clip_probs_patch"] = (res["recomputed_idx"], res["recomputed_clip_probs"])   # (popped by forward)
        return out
