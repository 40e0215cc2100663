"""Diverse beam search beside the plain search of equal width, on the synthetic checkpoint's decoder (decoder-only contexts).

B = 64 clips, T = 31 frames, max_pred = 20; min_pred = 20 too, so that every row searches through all 20 steps in both searches and the
times compare step kernels, not caption lengths.  For (G, W) in (3, 1), (3, 3), (8, 1), (4, 4):
  groups : Engine.decode_groups(G, W, diversity_penalty 0.5)   -- conette_decode_groups, one search-step launch per decode step
  plain  : Engine.decode(beam = G * W)                          -- conette_decode, the same rows per clip
Both in one process on one device, alternating, median of --iters after --warmup, milliseconds per whole search (prepare, 20 steps,
finalize), two ways: `eager` (the library's own decode graph cache switched off: ~10^3 launches from the host per search) and `graph`
(each call captured once into a torch.cuda.CUDAGraph and replayed: device time without launch overhead).  The difference
groups - plain per step is what the G - 1 extra serial merges (and, on the generic kernel, the extra arg-max bookkeeping) cost.

    python tools/time_group_search.py [--iters 20] [--warmup 3] [--precisions bf16] [--out profiles/group_search_times.md]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((3, 1), (3, 3), (8, 1), (4, 4))
B, T_AUDIO, MAX_PRED = 64, 31, 20


def median_ms(fns, iters, warmup):
    """the callables alternating; per callable the median time of `iters` runs after `warmup`"""
    times = [[] for _ in fns]
    for it in range(warmup + iters):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if it >= warmup:
                times[i].append(a.elapsed_time(b))
    return [float(np.median(t)) for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--precisions", default="bf16")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import conette_amd  # noqa: F401
    from conette_amd import synth
    from conette_amd.engine import Engine
    from oracle import cpu_ref as O

    w = {k: v for k, v in O.to_torch(synth.synth_state_dict()).items() if k.startswith("model.")}
    v = int(w["model.decoder.classifier.weight"].shape[0])
    props = torch.cuda.get_device_properties(0)
    lines = [f"device: {props.name}, {props.multi_processor_count} CUs; torch {torch.__version__}; V = {v}, B = {B}, T = {T_AUDIO}, "
             f"max_pred = min_pred = {MAX_PRED}; median of {args.iters} after {args.warmup} warm-up, paths alternating; ms per whole search",
             "",
             "| precision | G | W | rows/clip | step kernel | groups eager | plain eager | groups graph | plain graph | graph diff / step (us) | graph ratio |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    rng = np.random.Generator(np.random.PCG64(4243))
    fe = torch.from_numpy(((rng.random((B, T_AUDIO, 768)) * 2 - 1) * 1.1).astype(np.float32)).cuda()
    lens = torch.full((B,), T_AUDIO, dtype=torch.int32, device="cuda")
    bos = w["model.task_id_to_token_id"][torch.arange(B) % 7].int().cuda()
    forbid = w["model.forbid_rep_mask"].to(torch.uint8).cuda()
    for prec in args.precisions.split(","):
        eng = Engine(w, precision=prec)
        eng.set_decode_graph(False)
        for g, wd in SHAPES:
            groups = lambda: eng.decode_groups(fe, lens, bos, forbid, g, wd, 0.5, MAX_PRED, MAX_PRED)
            plain = lambda: eng.decode(fe, lens, bos, forbid, g * wd, MAX_PRED, MAX_PRED)
            eager = median_ms([groups, plain], args.iters, args.warmup)
            graphs = []
            for fn in (groups, plain):
                fn()
                torch.cuda.synchronize()
                cg = torch.cuda.CUDAGraph()
                with torch.cuda.graph(cg):
                    held = fn()
                graphs.append((cg, held))
            replay = median_ms([gr.replay for gr, _ in graphs], args.iters, args.warmup)
            kernel = "register" if (v <= 8192 and g * wd <= 8) else "generic"
            lines.append(f"| {prec} | {g} | {wd} | {g * wd} | {kernel} | {eager[0]:.3f} | {eager[1]:.3f} | {replay[0]:.3f} | {replay[1]:.3f} | "
                         f"{(replay[0] - replay[1]) * 1000.0 / MAX_PRED:+.1f} | {replay[0] / replay[1]:.3f} |")
            del graphs
        del eng
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
