"""Consensus choice, device against host, on random candidate tables (no checkpoint beyond a decoder-only synthetic Engine).

For (B clips, N candidates, L tokens) in {(256, 16, 20), (256, 64, 22)} and the utilities "ngram" (order 4) and "edit":
  device : Engine.consensus(preds, lens) on device tensors -- conette_consensus, one launch, no host sync
  host   : preds / lens copied to the host + consensus.select per clip (numpy, float64): what a caller had to do without the entry
milliseconds (device: median of --iters after --warmup by HIP events; host: median of --host_iters wall-clock runs, the copy included).
The picks of both paths are compared wherever the float64 margin exceeds 2**-16.

    python tools/consensus_bench.py [--iters 50] [--warmup 5] [--host_iters 1] [--out profiles/consensus_notes.md]
"""
import argparse
import datetime
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((256, 16, 20), (256, 64, 22))
SETTINGS = (("ngram", 4), ("edit", 4))
VOCAB = 400         # words the random captions draw from: short captions share unigrams and some bigrams, as samples of one clip do


def table(rng, b, n, l):
    """random captions around one per-clip "theme" (a draw shares most words with it), <eos> = 2, pads = 0"""
    preds = np.zeros((b, n, l), dtype=np.int32)
    lens = np.zeros((b, n), dtype=np.int32)
    for i in range(b):
        theme = 4 + rng.integers(0, VOCAB, l)
        for j in range(n):
            k = int(rng.integers(l // 2, l))
            row = np.where(rng.random(k) < 0.7, theme[:k], 4 + rng.integers(0, VOCAB, k))
            preds[i, j, :k], preds[i, j, k], lens[i, j] = row, 2, k + 1
    return preds, lens


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host_iters", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import conette_amd  # noqa: F401
    from conette_amd import consensus, synth
    from conette_amd.engine import Engine
    from oracle import cpu_ref as O

    w = {k: v for k, v in O.to_torch(synth.synth_state_dict()).items() if k.startswith("model.")}
    eng = Engine(w, precision="bf16")
    props = torch.cuda.get_device_properties(0)
    lines = ["# Consensus choice: device against host", "",
             f"{props.name}, {props.multi_processor_count} CUs; torch {torch.__version__}; {datetime.date.today().isoformat()}; device: median of "
             f"{args.iters} after {args.warmup} warm-up (HIP events); host: median of {args.host_iters} (copy to host + consensus.select per clip)", "",
             "| B x N x L | utility | device ms | us per clip | host ms | host / device |", "|---|---|---|---|---|---|"]
    rng = np.random.Generator(np.random.PCG64(99))
    for b, n, l in SHAPES:
        preds_h, lens_h = table(rng, b, n, l)
        preds, lens = torch.from_numpy(preds_h).cuda(), torch.from_numpy(lens_h).cuda()
        for kind, order in SETTINGS:
            dev_ms = []
            for it in range(args.warmup + args.iters):
                a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                out = eng.consensus(preds, lens, utility=kind, max_order=order)
                z.record()
                z.synchronize()
                if it >= args.warmup:
                    dev_ms.append(a.elapsed_time(z))
            host_ms = []
            for _ in range(args.host_iters):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ref = consensus.select_batch(preds.cpu().numpy(), lens.cpu().numpy(), utility=kind, max_order=order)
                host_ms.append((time.perf_counter() - t0) * 1e3)
            sure = ref["margin"] > 2.0 ** -16
            assert np.array_equal(out["best"].cpu().numpy()[sure], ref["best"][sure]), (b, n, l, kind)
            d, h = float(np.median(dev_ms)), float(np.median(host_ms))
            lines.append(f"| {b} x {n} x {l} | {kind} | {d:.3f} | {d * 1e3 / b:.2f} | {h:.0f} | {h / d:.0f} |")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
