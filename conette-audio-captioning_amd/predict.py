"""``conette-predict`` for the MI355X path: same flags and CSV format as the reference CLI
(reference src/conette/predict.py:27-232).

    python -m conette_amd.predict --audio a.wav b.wav --task clotho --model_name DIR_OR_HUB_NAME \
        [--csv_export out.csv] [--precision certified|certified:BASE|bf16|bf16+f16dec|f16|mixed|mixed16|exact|fp32]
        [--sample N --temperature T --top_k K --top_p P --seed S [--consensus ngram|edit --consensus_order K]] [--align]
        [--tag_timeline --tag_window SECONDS --tag_threshold P --tag_off_threshold P --tag_min_duration SECONDS --tag_max_gap SECONDS]
        [--segments --segment_window SECONDS --segment_hop SECONDS --segment_merge X]
        [--beam_groups G --group_beam W --diversity_penalty L]
        [--prefix "a dog" --ban_words WORD ... --no_repeat_ngram N]

``--model_path`` (a Lightning training log directory with hydra/config.yaml + checkpoints/best.ckpt, predict.py:123-178) is
accepted when the audio encoder's weights come with it: the reference builds its HF wrapper around the Lightning module and leaves
the ConvNeXt of the preprocessor at its RANDOM initialisation there (huggingface/preprocessor.py:23-33: ``pretrained=False``,
nothing in such a directory is loaded into it), so its captions from that path are noise; this CLI wants ``preprocessor.encoder.*``
tensors -- inside best.ckpt's state dict, in ``checkpoints/encoder.ckpt`` or through ``--encoder_ckpt`` -- and refuses otherwise.
Audio files are PCM WAV (see preprocessor.load_audio).
"""
from __future__ import annotations

import csv
import json
import logging
import os.path as osp
import sys
from argparse import ArgumentParser, Namespace
from typing import List, Optional

pylog = logging.getLogger("conette_amd.predict")


def _opt_str(x: str) -> Optional[str]:
    return None if x.lower() in ("none", "null", "") else x


def _opt_int(x: str) -> Optional[int]:
    return None if x.lower() in ("none", "null", "") else int(x)


def get_predict_args(argv: Optional[List[str]] = None) -> Namespace:
    parser = ArgumentParser(description="CoNeTTE audio captioning on MI355X.")
    parser.add_argument("--audio", type=str, help="Path to an audio file.", default=(), required=True, nargs="+")
    parser.add_argument("--task", type=_opt_str, help="CoNeTTE task embedding input.", default=None, nargs="+")
    parser.add_argument("--model_name", type=_opt_str, help="Model name on huggingface or local HF directory.",
                        default="Labbeti/conette")
    parser.add_argument("--model_path", type=_opt_str, default=None,
                        help="Path to a trained model directory (hydra/config.yaml + checkpoints/best.ckpt of a CoNeTTEPLM run). The "
                             "reference leaves the ConvNeXt audio encoder at its random initialisation on this path; here the "
                             "encoder weights (preprocessor.encoder.* tensors) must be in best.ckpt, in checkpoints/encoder.ckpt "
                             "or given by --encoder_ckpt.")
    parser.add_argument("--encoder_ckpt", type=_opt_str, default=None,
                        help="With --model_path: a state dict of the ConvNeXt audio encoder (keys preprocessor.encoder.*, encoder.* or bare).")
    parser.add_argument("--device", type=str, help="Torch device used to run the model.", default="cuda_if_available")
    parser.add_argument("--token", type=_opt_str, help="Optional access token.", default=None)
    parser.add_argument("--seed", type=_opt_int, help="Random seed value (the search is deterministic; --sample draws with it).", default=1234)
    parser.add_argument("--sample", type=int, default=0,
                        help="N > 0: draw N captions per file from the model's distribution instead of searching (one row per draw).")
    parser.add_argument("--temperature", type=float, help="With --sample: softmax temperature.", default=1.0)
    parser.add_argument("--top_k", type=int, help="With --sample: keep the k most likely tokens (0: off).", default=0)
    parser.add_argument("--top_p", type=float, help="With --sample: nucleus mass (1: off).", default=1.0)
    parser.add_argument("--consensus", type=str, choices=("ngram", "edit"), default=None,
                        help="With --sample: one row per file, the draw that agrees most with all the others (minimum Bayes risk; "
                             "CoNeTTEModel.caption_consensus) by n-gram overlap or by token edit distance, instead of one row per draw.")
    parser.add_argument("--consensus_order", type=int, default=None,
                        help="With --consensus ngram: the longest n-gram counted, 1 .. 4 (default 4).")
    parser.add_argument("--align", action="store_true",
                        help="One row per word of each file's caption -- audio, task, word, start, end (seconds) -- instead of one per file: "
                             "where in the clip the decoder listens while it predicts the word (CoNeTTEModel.align_captions).")
    parser.add_argument("--align_mass", type=float, default=0.5,
                        help="With --align: start .. end is the shortest window holding this share of the word's attention.")
    parser.add_argument("--tag_timeline", action="store_true",
                        help="Besides the caption, WHEN each AudioSet tag is heard in the file (CoNeTTEModel.tag_timeline): its events "
                             "are printed, and exported as one JSON column 'tag_events'.")
    parser.add_argument("--tag_window", type=float, default=None,
                        help="With --tag_timeline: seconds of audio pooled around every 0.32 s frame (default 2.24).")
    parser.add_argument("--tag_threshold", type=float, default=None,
                        help="With --tag_timeline: the probability that opens an event (default 0.3).")
    parser.add_argument("--tag_off_threshold", type=float, default=None,
                        help="With --tag_timeline: an open event lasts while the probability stays at or above this (default: --tag_threshold).")
    parser.add_argument("--tag_min_duration", type=float, default=None,
                        help="With --tag_timeline: events shorter than this many seconds are dropped (default 0).")
    parser.add_argument("--tag_max_gap", type=float, default=None,
                        help="With --tag_timeline: events of one tag at most this many seconds apart are merged (default 0).")
    parser.add_argument("--segments", action="store_true",
                        help="Captions over time for long recordings (CoNeTTEModel.caption_segments): one row per segment with its onset "
                             "and offset in seconds.  The defaults of the three flags below are untuned.")
    parser.add_argument("--segment_window", type=float, default=None, help="With --segments: seconds per captioned window (default 10).")
    parser.add_argument("--segment_hop", type=float, default=None, help="With --segments: seconds between window starts (default 5).")
    parser.add_argument("--segment_merge", type=float, default=None,
                        help="With --segments: neighbouring windows whose captions agree at least this much (n-gram F-score, 0 .. 1) "
                             "form one segment (default 0.5).")
    parser.add_argument("--beam_groups", type=int, default=0,
                        help="G > 0: diverse beam search in G groups (CoNeTTEModel.caption_diverse): G x --group_beam different captions "
                             "per file, one row each, group-major.")
    parser.add_argument("--group_beam", type=int, help="With --beam_groups: beams per group.", default=1)
    parser.add_argument("--diversity_penalty", type=float, default=0.5,
                        help="With --beam_groups: what a candidate pays for each earlier group that picked its token at this step.")
    parser.add_argument("--prefix", type=_opt_str, default=None,
                        help="Every caption begins with these words (CoNeTTEModel.caption_constrained): whitespace-separated "
                             "vocabulary entries.")
    parser.add_argument("--ban_words", type=str, nargs="+", default=None,
                        help="Words no caption may hold; words outside the vocabulary are ignored.")
    parser.add_argument("--no_repeat_ngram", type=int, default=0, help="N > 0: no caption repeats an N-gram.")
    parser.add_argument("--require_words", type=str, nargs="+", default=None,
                        help="Words every caption must hold (CoNeTTEModel.caption_constrained(required=...)); 'bark|barks' asks for "
                             "one of the alternatives.")
    parser.add_argument("--ensemble_models", type=str, nargs="+", default=None,
                        help="2 .. 4 local HF directories: their models caption as one ensemble (one search, combined scores); "
                             "in place of --model_name / --model_path.")
    parser.add_argument("--ensemble_tasks", type=str, nargs="+", default=None,
                        help="Task ensemble: one caption that these tasks agree on (with --ensemble_models: one task per model).")
    parser.add_argument("--ensemble_weights", type=float, nargs="+", default=None,
                        help="With --ensemble_models / --ensemble_tasks: one positive weight per member (normalised; default equal).")
    parser.add_argument("--ensemble_combine", type=str, choices=("logprob", "prob"), default="logprob",
                        help="With --ensemble_models / --ensemble_tasks: logprob (product of experts) or prob (mixture).")
    parser.add_argument("--csv_export", type=_opt_str, help="Path to CSV output file.", default=None)
    parser.add_argument("--verbose", type=int, help="Verbose level.", default=1)
    parser.add_argument("--precision", type=str, default=None,
                        help="certified (default: fp16 pipeline + id certificate, uncertified clips re-run exactly), certified:<base>, "
                             "bf16, bf16+f16dec, f16, mixed, mixed16, exact, fp32")
    args = parser.parse_args(argv)
    if args.consensus is None and args.consensus_order is not None:
        raise ValueError("--consensus_order goes with --consensus")
    if args.consensus is not None:
        if args.sample <= 0:
            raise ValueError("--consensus chooses among the draws of --sample N; it does not go without --sample")
        if args.consensus_order is None:
            args.consensus_order = 4
        import numpy as np
        from . import consensus
        consensus.check_arguments(np.zeros((1, args.sample, 1), dtype=np.int32), None, None, args.consensus, args.consensus_order)
    tag_flags = ("tag_window", "tag_threshold", "tag_off_threshold", "tag_min_duration", "tag_max_gap")
    if not args.tag_timeline and any(getattr(args, k) is not None for k in tag_flags):
        raise ValueError("--tag_window / --tag_threshold / --tag_off_threshold / --tag_min_duration / --tag_max_gap go with --tag_timeline")
    if args.tag_timeline:
        if args.ensemble_models is not None:
            raise ValueError("--tag_timeline reads one model's tag head; it does not go with --ensemble_models")
        for k, v in zip(tag_flags, (2.24, 0.3, None, 0.0, 0.0)):
            if getattr(args, k) is None:
                setattr(args, k, v)
        from . import tagging
        tagging.check_arguments(window=tagging.window_frames(args.tag_window), on=args.tag_threshold, off=args.tag_off_threshold,
                                min_frames=tagging.min_frames(args.tag_min_duration), max_gap=tagging.gap_frames(args.tag_max_gap))
    seg_flags = ("segment_window", "segment_hop", "segment_merge")
    if not args.segments and any(getattr(args, k) is not None for k in seg_flags):
        raise ValueError("--segment_window / --segment_hop / --segment_merge go with --segments")
    if args.segments:
        steered = args.prefix is not None or args.ban_words is not None or args.no_repeat_ngram > 0 or args.require_words is not None
        for flag, on in (("--sample", args.sample > 0), ("--beam_groups", args.beam_groups > 0), ("--align", args.align),
                         ("--prefix / --ban_words / --no_repeat_ngram / --require_words", steered),
                         ("--ensemble_models / --ensemble_tasks", args.ensemble_models is not None or args.ensemble_tasks is not None)):
            if on:
                raise ValueError(f"--segments runs the plain beam search over windows of a recording; it does not go with {flag}")
        for k, v in zip(seg_flags, (10.0, 5.0, 0.5)):
            if getattr(args, k) is None:
                setattr(args, k, v)
        from . import segments
        segments.window_frames(args.segment_window), segments.hop_frames(args.segment_hop)
        segments.check_arguments(threshold=args.segment_merge)
    if args.beam_groups > 0 and args.sample > 0:
        raise ValueError("--beam_groups searches for different captions; it does not go with --sample")
    if args.beam_groups > 0 and args.align:
        raise ValueError("--align places the words of the searched caption; it does not go with --beam_groups")
    if args.prefix is not None or args.ban_words is not None or args.no_repeat_ngram > 0 or args.require_words is not None:
        for flag, on in (("--sample", args.sample > 0), ("--beam_groups", args.beam_groups > 0), ("--align", args.align)):
            if on:
                raise ValueError(f"--prefix / --ban_words / --no_repeat_ngram / --require_words steer the beam search; they do not go with {flag}")
    ensemble = args.ensemble_models is not None or args.ensemble_tasks is not None
    if not ensemble and args.ensemble_weights is not None:
        raise ValueError("--ensemble_weights goes with --ensemble_models or --ensemble_tasks")
    if ensemble:
        steered = args.prefix is not None or args.ban_words is not None or args.no_repeat_ngram > 0 or args.require_words is not None
        for flag, on in (("--sample", args.sample > 0), ("--beam_groups", args.beam_groups > 0), ("--align", args.align),
                         ("--prefix / --ban_words / --no_repeat_ngram / --require_words", steered), ("--task", args.task is not None)):
            if on:
                raise ValueError(f"--ensemble_models / --ensemble_tasks run the plain beam search on combined scores; they do not go with {flag}")
        if args.ensemble_models is not None:
            if args.model_path is not None or args.model_name != parser.get_default("model_name"):
                raise ValueError("--ensemble_models names the models; it does not go with --model_name / --model_path")
            if not 2 <= len(args.ensemble_models) <= 4:
                raise ValueError(f"--ensemble_models: {len(args.ensemble_models)} directories (expected 2 .. 4; one model: --model_name)")
        n = len(args.ensemble_models) if args.ensemble_models is not None else len(args.ensemble_tasks)
        if args.ensemble_models is not None and args.ensemble_tasks is not None and len(args.ensemble_tasks) not in (1, n):
            raise ValueError(f"--ensemble_tasks: {len(args.ensemble_tasks)} tasks for {n} --ensemble_models (expected one, or one per model)")
        if args.ensemble_weights is not None and len(args.ensemble_weights) != n:
            raise ValueError(f"--ensemble_weights: {len(args.ensemble_weights)} weights for {n} members")
        from . import ensemble_search
        ensemble_search.check_arguments(n, args.ensemble_weights, args.ensemble_combine, 1)
    return args


def format_results(fpaths: List[str], tasks: List[str], cands: List[str]) -> List[dict]:
    """Row format of predict.py:214-218."""
    return [{"audio": osp.basename(f), "task": t, "candidate": c} for f, t, c in zip(fpaths, tasks, cands)]


def format_alignment(fpaths: List[str], tasks: List[str], tokenizer, outs: dict) -> List[dict]:
    """Rows of ``--align``: the words of each file's aligned caption (n_caps = 1) in order, special tokens left out, with the
    span of ``align_captions`` in seconds."""
    special = (tokenizer.pad_token_id, tokenizer.bos_token_id, tokenizer.eos_token_id)
    tokens, spans = outs["tokens"][:, 0].tolist(), outs["span_time"][:, 0].tolist()
    return [{"audio": osp.basename(f), "task": t, "word": tokenizer.id_to_token(tok), "start": f"{lo:.2f}", "end": f"{hi:.2f}"}
            for f, t, row, sp in zip(fpaths, tasks, tokens, spans) for tok, (lo, hi) in zip(row, sp) if tok not in special]


def format_segments(fpaths: List[str], outs: dict) -> List[dict]:
    """Rows of ``--segments``: one per segment of each file, in time order."""
    return [{"audio": osp.basename(f), "onset": f"{s['onset']:.2f}", "offset": f"{s['offset']:.2f}", "caption": s["caption"],
             "lprob": f"{s['lprob']:.4f}"} for f, segs in zip(fpaths, outs["segments"]) for s in segs]


def add_tag_events(model, args: Namespace, fpaths: List[str], results: List[dict]) -> None:
    """``--tag_timeline``: every row of ``results`` gets its file's events as the JSON column "tag_events"; they are printed once per file."""
    outs = model.tag_timeline(fpaths, window_s=args.tag_window, threshold=args.tag_threshold, off_threshold=args.tag_off_threshold,
                              min_duration_s=args.tag_min_duration, max_gap_s=args.tag_max_gap)
    by_file = {}
    for f, events, cut in zip(fpaths, outs["events"], outs["events_truncated"].tolist()):
        rows = [{"tag": e["tag"], "onset": round(e["onset"], 2), "offset": round(e["offset"], 2), "peak": round(e["peak"], 3)} for e in events]
        by_file[osp.basename(f)] = json.dumps(rows)
        listed = "\n".join(f" - {r['tag']} [{r['onset']:.2f}-{r['offset']:.2f}] peak {r['peak']:.2f}" for r in rows) or " - (none)"
        pylog.info(f"File '{osp.basename(f)}' tag events{' (more than the 16 kept per tag)' if cut else ''}:\n{listed}")
    for r in results:
        r["tag_events"] = by_file[r["audio"]]


def write_csv(path: str, results: List[dict]) -> None:
    with open(path, "w") as file:
        writer = csv.DictWriter(file, fieldnames=list(results[0]) if results else ["audio", "task", "candidate"])
        writer.writeheader()
        writer.writerows(results)


def _check_model_path(model_path: str) -> None:
    """predict.py:123-141 (same three messages)."""
    cfg_fpath = osp.join(model_path, "hydra", "config.yaml")
    ckpt_fpath = osp.join(model_path, "checkpoints", "best.ckpt")
    if not osp.isdir(model_path):
        raise FileNotFoundError(f"Cannot find model_path directory. ({model_path} is not a directory)")
    if not osp.isfile(cfg_fpath):
        raise FileNotFoundError(f"Cannot find config file in model_path directory. ({cfg_fpath} is not a file)")
    if not osp.isfile(ckpt_fpath):
        raise FileNotFoundError(f"Cannot find checkpoint file in model_path directory. ({ckpt_fpath} is not a file)")


ENCODER_PREFIX = "preprocessor.encoder."


def model_path_state_dict(model_path: str, encoder_ckpt: Optional[str] = None):
    """(CoNeTTEConfig, HF-layout state dict) of a training log directory (predict.py:144-178): the Lightning module's tensors
    under ``model.`` (the attribute the HF wrapper holds it by, huggingface/model.py:86-98) + the audio encoder's under
    ``preprocessor.encoder.``."""
    import torch
    import yaml

    from . import CoNeTTEConfig

    _check_model_path(model_path)
    with open(osp.join(model_path, "hydra", "config.yaml"), "r") as file:
        raw_cfg = yaml.safe_load(file) or {}
    pl_cfg = dict(raw_cfg.get("pl", {}) or {})
    target = pl_cfg.pop("_target_", "unknown")
    if "CoNeTTEPLM" not in target:
        if "BaselinePLM" in target:
            raise NotImplementedError("model_path holds a BaselinePLM run: load it with conette_amd.BaselinePLM.from_checkpoint("
                                      "'<model_path>/checkpoints/best.ckpt') (no task tokens, precomputed frame embeddings).")
        raise NotImplementedError(f"Unsupported pretrained model type '{target}'.")
    ckpt = torch.load(osp.join(model_path, "checkpoints", "best.ckpt"), map_location="cpu", weights_only=False)
    plm_sd = ckpt["state_dict"]
    sd = {}
    for k, v in plm_sd.items():
        sd[k if k.startswith(ENCODER_PREFIX) else "model." + k] = v
    enc_file = encoder_ckpt or osp.join(model_path, "checkpoints", "encoder.ckpt")
    if not any(k.startswith(ENCODER_PREFIX) for k in sd) and osp.isfile(enc_file):
        enc = torch.load(enc_file, map_location="cpu", weights_only=False)
        enc = enc.get("state_dict", enc.get("model", enc)) if isinstance(enc, dict) else enc
        for k, v in enc.items():
            for pre in (ENCODER_PREFIX, "encoder."):
                if k.startswith(pre):
                    k = k[len(pre):]
                    break
            sd[ENCODER_PREFIX + k] = v
    if not any(k.startswith(ENCODER_PREFIX) for k in sd):
        raise ValueError(
            f"--model_path {model_path}: no audio-encoder weights.  The reference wraps the Lightning checkpoint in its HF model and "
            "leaves the ConvNeXt of the preprocessor at its random initialisation on this path (predict.py:144-178, "
            "huggingface/preprocessor.py:23-33); this CLI needs preprocessor.encoder.* tensors in checkpoints/best.ckpt, "
            "a checkpoints/encoder.ckpt, or --encoder_ckpt FILE.")
    import inspect
    known = set(inspect.signature(CoNeTTEConfig.__init__).parameters) - {"self", "kwargs"}
    config = CoNeTTEConfig(**{k: v for k, v in pl_cfg.items() if k in known})
    return config, sd


def main_predict(argv: Optional[List[str]] = None) -> List[dict]:
    args = get_predict_args(argv)
    logging.basicConfig(level=logging.INFO if args.verbose >= 1 else logging.WARNING, format="%(message)s")
    from . import CoNeTTEConfig
    from .model import DEFAULT_PRECISION, CoNeTTEModel

    precision = DEFAULT_PRECISION if args.precision is None else args.precision
    if args.ensemble_models is not None:     # several checkpoints, one search (ensemble.py)
        from .ensemble import CoNeTTEEnsemble
        models = [CoNeTTEModel.from_pretrained(d, config=CoNeTTEConfig.from_pretrained(d), device=args.device, precision=precision).eval_and_disable_grad()
                  for d in args.ensemble_models]
        ens = CoNeTTEEnsemble(models, weights=args.ensemble_weights, combine=args.ensemble_combine)
        tasks = args.ensemble_tasks[0] if args.ensemble_tasks is not None and len(args.ensemble_tasks) == 1 else args.ensemble_tasks
        fpaths = list(args.audio)
        outs = ens(fpaths, task=tasks)
        results = format_results(fpaths, outs["tasks"], outs["cands"])
        for r in results:
            pylog.info(f"File '{r['audio']}' with task '{r['task']}':\n - '{r['candidate']}'")
        if args.csv_export is not None:
            write_csv(args.csv_export, results)
        return results
    if args.model_path is not None:     # (the reference gives model_path the precedence too: predict.py:196-201)
        config, sd = model_path_state_dict(args.model_path, args.encoder_ckpt)
        model = CoNeTTEModel(config, device=args.device, state_dict=sd, precision=precision)
    elif args.model_name is not None:
        config = CoNeTTEConfig.from_pretrained(args.model_name)
        model = CoNeTTEModel.from_pretrained(args.model_name, config=config, device=args.device, precision=precision)
    else:
        raise ValueError(f"Invalid arguments {args.model_name=} and {args.model_path=}. (expected at one str value)")
    model.eval_and_disable_grad()
    fpaths = list(args.audio)
    tasks = args.task
    if tasks is not None and len(tasks) == 1:
        tasks = tasks[0]
    if args.align and args.sample > 0:
        raise ValueError("--align places the words of the searched caption; it does not go with --sample")
    if args.align:        # one row per word of the best caption
        outs = model.align_captions(fpaths, task=tasks, mass=args.align_mass)
        results = format_alignment(fpaths, outs["tasks"], model.tokenizer, outs)
        for f, t, c in zip(fpaths, outs["tasks"], outs["cands"]):
            words = " ".join(f"{r['word']}[{r['start']}-{r['end']}]" for r in results if r["audio"] == osp.basename(f))
            pylog.info(f"File '{osp.basename(f)}' with task '{t}':\n - '{c}'\n - {words}")
        if args.tag_timeline:
            add_tag_events(model, args, fpaths, results)
        if args.csv_export is not None:
            write_csv(args.csv_export, results)
        return results
    if args.segments:     # one row per segment of each file
        outs = model.caption_segments(fpaths, window_s=args.segment_window, hop_s=args.segment_hop, merge_threshold=args.segment_merge, task=tasks)
        results = format_segments(fpaths, outs)
        for f, cut in zip(fpaths, outs["segments_truncated"].tolist()):
            listed = "\n".join(f" - [{r['onset']}-{r['offset']}] '{r['caption']}'" for r in results if r["audio"] == osp.basename(f))
            pylog.info(f"File '{osp.basename(f)}' segments{' (more than the 64 kept)' if cut else ''}:\n{listed}")
        if args.tag_timeline:
            add_tag_events(model, args, fpaths, results)
        if args.csv_export is not None:
            write_csv(args.csv_export, results)
        return results
    if args.ensemble_tasks is not None:   # one caption per file that the tasks agree on
        outs = model.caption_ensemble(fpaths, tasks=args.ensemble_tasks, weights=args.ensemble_weights, combine=args.ensemble_combine)
        results = format_results(fpaths, outs["tasks"], outs["cands"])
    elif args.beam_groups > 0:   # G x W captions per file, group-major
        outs = model.caption_diverse(fpaths, num_groups=args.beam_groups, group_beam_size=args.group_beam,
                                     diversity_penalty=args.diversity_penalty, task=tasks)
        n = args.beam_groups * args.group_beam
        results = format_results([f for f in fpaths for _ in range(n)], [t for t in outs["tasks"] for _ in range(n)],
                                 [c for cands in outs["mult_cands"] for c in cands])
    elif args.prefix is not None or args.ban_words is not None or args.no_repeat_ngram > 0 or args.require_words is not None:
        required = None if args.require_words is None else [w.split("|") for w in args.require_words]
        outs = model.caption_constrained(fpaths, prefix=args.prefix, banned=args.ban_words, no_repeat_ngram_size=args.no_repeat_ngram,
                                         task=tasks, required=required)
        results = format_results(fpaths, outs["tasks"], outs["cands"])
    elif args.sample > 0 and args.consensus is not None:   # N draws per file, one row: the consensus among them
        outs = model.caption_consensus(fpaths, num_samples=args.sample, temperature=args.temperature, top_k=args.top_k, top_p=args.top_p,
                                       seed=args.seed, task=tasks, utility=args.consensus, max_order=args.consensus_order)
        results = format_results(fpaths, outs["tasks"], outs["cands"])
    elif args.sample > 0:   # N draws per file, in the order drawn
        outs = model.sample(fpaths, num_samples=args.sample, temperature=args.temperature, top_k=args.top_k, top_p=args.top_p,
                            seed=args.seed, task=tasks)
        results = format_results([f for f in fpaths for _ in range(args.sample)], [t for t in outs["tasks"] for _ in range(args.sample)],
                                 [c for cands in outs["mult_cands"] for c in cands])
    else:
        outs = model(fpaths, task=tasks)
        results = format_results(fpaths, outs["tasks"], outs["cands"])
    for r in results:
        pylog.info(f"File '{r['audio']}' with task '{r['task']}':\n - '{r['candidate']}'")
    if args.tag_timeline:
        add_tag_events(model, args, fpaths, results)
    if args.csv_export is not None:
        write_csv(args.csv_export, results)
    return results


if __name__ == "__main__":
    main_predict(sys.argv[1:])
