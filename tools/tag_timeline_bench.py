"""Tag timeline, the device entries against what a caller had to write without them, on random frame embeddings (the default synthetic
checkpoint's clip head).

For (B clips, T frames, window w) in {(64, 31, 7): the benchmark's 10 s batch, (64, 94, 31): 30 s clips under a 10 s window,
(1, 1875, 7): one 10-minute recording}:
  device : Engine.tag_frames + Engine.tag_events on device tensors -- conette_tag_frames, conette_tag_events; no host sync
  torch  : unfold + amax / mean over the window (padded with -inf / 0 at the clip's ends), layer_norm, linear, sigmoid in PyTorch fp32
           on the GPU, then a copy of the (B, T, 527) probabilities to the host and tagging.events_batch there
milliseconds per call: medians of --iters windows of 20 back-to-back calls after --warmup windows; GPU work by HIP events, the host part of the torch path by wall clock around a
synchronised copy.  Both paths see the same inputs; their probabilities are compared, and the events of the device path are compared
with the rule on the device's own probabilities.

    python tools/tag_timeline_bench.py [--iters 30] [--warmup 5] [--host_iters 3] [--precisions bf16 fp32] [--out profiles/tag_timeline_notes.md]
"""
import argparse
import datetime
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((64, 31, 7, "the benchmark's 10 s batch"), (64, 94, 31, "30 s clips, 10 s window"), (1, 1875, 7, "one 10-minute recording"))
SETTING = (0.3, 0.3, 1, 0, 16)          # CoNeTTEModel.tag_timeline's defaults: (on, off, min_frames, max_gap, max_events)


def torch_frames(fe, w, norm_w, norm_b, head_w, head_b):
    """the frame rule for clips of full length, composed from PyTorch operators"""
    lo, hi = (w - 1) // 2, w // 2
    x = fe.transpose(1, 2)                                               # (B, 768, T)
    mx = F.pad(x, (lo, hi), value=float("-inf")).unfold(2, w, 1).amax(dim=3)
    sm = F.pad(x, (lo, hi)).unfold(2, w, 1).sum(dim=3)
    cnt = F.pad(torch.ones_like(x[:1, :1]), (lo, hi)).unfold(2, w, 1).sum(dim=3)
    v = (mx + sm / cnt).transpose(1, 2)
    z = F.layer_norm(v, (v.shape[2],), norm_w, norm_b, 1e-6)
    return torch.sigmoid(F.linear(z, head_w, head_b))


REPS = 20       # calls between two events: one call is tens of microseconds, less than what an event pair resolves


def timed(fn, iters, warmup):
    """median milliseconds per call over ``iters`` windows of REPS back-to-back calls, and the last result"""
    ms, out = [], None
    for it in range(warmup + iters):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(REPS):
            out = fn()
        z.record()
        z.synchronize()
        if it >= warmup:
            ms.append(a.elapsed_time(z) / REPS)
    return float(np.median(ms)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host_iters", type=int, default=3)
    ap.add_argument("--precisions", nargs="+", default=["bf16", "fp32"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import conette_amd  # noqa: F401
    from conette_amd import synth, tagging
    from conette_amd.engine import Engine
    from oracle import cpu_ref as O

    weights = O.to_torch(synth.synth_state_dict())
    pre = "preprocessor.encoder."
    head = [weights[pre + k].cuda().float() for k in ("norm.weight", "norm.bias", "head_audioset.weight", "head_audioset.bias")]
    props = torch.cuda.get_device_properties(0)
    lines = ["# Tag timeline: the device entries against the PyTorch composition", "",
             f"{props.name}, {props.multi_processor_count} CUs; torch {torch.__version__}; {datetime.date.today().isoformat()}; milliseconds per call, medians of "
             f"{args.iters} windows of {REPS} back-to-back calls after {args.warmup} warm-up windows, GPU work by HIP events; the host part of the torch path (copy of the probabilities + "
             f"tagging.events_batch) by wall clock, median of {args.host_iters}.  Settings: on = off = {SETTING[0]}, max_events = {SETTING[4]}; "
             "clips of full length; random frame embeddings, the synthetic checkpoint's clip head.", "",
             "| B x T, window | precision | tag_frames ms | tag_events ms | device total ms | torch frames ms (fp32) | host events ms | torch total ms "
             "| torch / device | largest probability difference |", "|---|---|---|---|---|---|---|---|---|---|"]
    rng = np.random.Generator(np.random.PCG64(5))
    engines = {p: Engine(weights, precision=p) for p in args.precisions}
    for b, t, w, what in SHAPES:
        fe = torch.from_numpy((rng.standard_normal((b, t, 768)) + 0.5 * rng.standard_normal(768)).astype(np.float32)).cuda()
        lens = torch.full((b,), t, dtype=torch.int32, device="cuda")
        torch_ms, ref = timed(lambda: torch_frames(fe, w, *head), args.iters, args.warmup)
        host_ms = []
        for _ in range(args.host_iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host = tagging.events_batch(ref.cpu().numpy(), lens.cpu().numpy(), *SETTING)
            host_ms.append((time.perf_counter() - t0) * 1e3)
        h = float(np.median(host_ms))
        for prec, eng in engines.items():
            frames_ms, probs = timed(lambda: eng.tag_frames(fe, lens, w), args.iters, args.warmup)
            events_ms, ev = timed(lambda: eng.tag_events(probs, lens, *SETTING), args.iters, args.warmup)
            both_ms, _ = timed(lambda: eng.tag_events(eng.tag_frames(fe, lens, w), lens, *SETTING), args.iters, args.warmup)
            diff = float((probs - ref).abs().max())
            assert diff < (1e-3 if prec in ("fp32", "exact") else 0.03), (b, t, w, prec, diff)
            own = tagging.events_batch(probs.cpu().numpy(), lens.cpu().numpy(), *SETTING)
            assert all(np.array_equal(ev[k].cpu().numpy().view(np.int32), own[k].view(np.int32)) for k in own), (b, t, w, prec)
            lines.append(f"| {b} x {t}, {w} ({what}) | {prec} | {frames_ms:.3f} | {events_ms:.3f} | {both_ms:.3f} | {torch_ms:.3f} | {h:.1f} | "
                         f"{torch_ms + h:.1f} | {(torch_ms + h) / both_ms:.0f} | {diff:.1e} |")
            print(lines[-1], flush=True)
        print(f"({b} x {t}: {int(host['counts'].sum())} events on the host path)", flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
