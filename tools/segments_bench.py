"""Caption timeline of one long recording, shared encoding against cut waveforms, on the synthetic checkpoint.

One 600 s synthetic recording (1875 frames unless the encoder refuses the length: then the library's error is printed with the
largest length of --seconds that it accepted), windows of 10 s every 5 s:
  shared : Engine.encode once, then Engine.decode_spans over all windows, then Engine.segments -- timed separately
  cut    : the same windows cut from the waveform and sent through model(x) in batches of --batch
milliseconds, median of --iters after --warmup; both paths in one process on one device.

    python tools/segments_bench.py [--seconds 600,300,120,60,30] [--iters 5] [--warmup 2] [--batch 32] [--precision bf16] [--out profiles/segments_bench.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, iters, warmup):
    out = None
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", default="600,300,120,60,30")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import conette_amd  # noqa: F401
    from conette_amd import CoNeTTEConfig, segments, synth
    from conette_amd.model import CoNeTTEModel
    from oracle import cpu_ref as O

    sd = O.to_torch(synth.synth_state_dict())
    sd["_extra_state_"] = torch.from_numpy(synth.extra_state_tensor())
    model = CoNeTTEModel(CoNeTTEConfig(**synth.synth_config_dict()), device="cuda:0", state_dict=sd, precision=args.precision,
                         audioset_idx_to_name={i: f"tag{i}" for i in range(527)})
    eng = model.engine
    props = torch.cuda.get_device_properties(0)
    lines = [f"device: {props.name}, {props.multi_processor_count} CUs; torch {torch.__version__}; precision {args.precision}; "
             f"median of {args.iters} after {args.warmup} warm-up; beam {model.config.beam_size}, max_pred {model.config.max_pred_size}"]
    window, hop = segments.window_frames(10.0), segments.hop_frames(5.0)
    for seconds in (int(v) for v in args.seconds.split(",")):
        n = seconds * 32000
        wave = torch.from_numpy(synth.synth_waveforms(1, n, 600)).cuda()
        try:
            t_enc, (fe, _) = timed(lambda: eng.encode(wave), args.iters, args.warmup)
        except RuntimeError as e:
            lines.append(f"{seconds} s: the encoder refuses this length: {e}")
            continue
        frames = int(eng.lib.conette_num_audio_frames(n))
        lens = np.asarray([frames], dtype=np.int32)
        table, counts = segments.span_table(lens, window, hop)
        s_n = int(table.shape[0])
        bos = model.batch_to_task_token_ids([model.default_task] * s_n, [None] * s_n)
        forbid = model.get_forbid_rep_mask(None)
        cfg = model.config
        t_dec, res = timed(lambda: eng.decode_spans(fe, torch.from_numpy(lens), table, bos, forbid, cfg.beam_size, cfg.min_pred_size,
                                                    cfg.max_pred_size, clone=False), args.iters, args.warmup)
        ids = res["best_preds"].view(1, s_n, -1)
        spans = torch.from_numpy(table[:, 1:].copy()).view(1, s_n, 2)
        t_seg, seg = timed(lambda: eng.segments(ids, torch.from_numpy(counts), res["best_lprobs"].view(1, s_n), spans), args.iters, args.warmup)
        cuts = [wave[:, int(a) * 10240:min((int(a) + int(b)) * 10240, n)].contiguous() for a, b in table[:, 1:]]

        def cut_path():
            out = []
            for i in range(0, len(cuts), args.batch):
                out.append(model(cuts[i:i + args.batch], sr=32000))
            return out
        t_cut, _ = timed(cut_path, args.iters, args.warmup)
        lines.append(f"{seconds} s: {frames} frames, {s_n} windows of {window} frames every {hop}, {int(seg['counts'][0])} segments | "
                     f"shared: encode {t_enc:.2f} ms + decode_spans {t_dec:.2f} ms + segments {t_seg:.3f} ms = {t_enc + t_dec + t_seg:.2f} ms | "
                     f"cut waveforms through model(x), batches of {args.batch}: {t_cut:.2f} ms")
        break       # (the first length the encoder takes)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
