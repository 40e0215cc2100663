"""Constrained beam search beside the plain search of equal beam, on the synthetic checkpoint's decoder (decoder-only contexts).

B = 64 clips, T = 31 frames, max_pred = 20; min_pred = 20 too, so that every row searches through all 20 steps in every search and
the times compare step kernels, not caption lengths.  For W in 1, 3, 8 (register kernel) and 9 (generic kernel):
  plain   : Engine.decode(beam = W)                                            -- conette_decode
  idle    : Engine.decode_constrained(beam = W), nothing active                -- the same picks through the constrained step
  ban     : ... with a ban mask of 64 words                                    -- M2 at every step
  ngram   : ... with no_repeat_ngram = 3                                       -- M3 at every step
  masks   : ... with both
  prefix  : ... with a prefix of 4 word tokens per clip                        -- 4 forced calls, then the fan-out
All in one process on one device, alternating, median of --iters after --warmup, milliseconds per whole search (prepare, 20 steps,
finalize), two ways: `eager` (the library's own decode graph cache switched off) and `graph` (each call captured once into a
torch.cuda.CUDAGraph and replayed: device time without launch overhead).

    python tools/time_constrained_search.py [--iters 20] [--warmup 3] [--precisions bf16,exact] [--out profiles/constrained_search_times.md]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BEAMS = (1, 3, 8, 9)
B, T_AUDIO, MAX_PRED, PREFIX_LEN, N_BANNED = 64, 31, 20, 4, 64


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
    ap.add_argument("--precisions", default="bf16,exact")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import conette_amd  # noqa: F401
    from conette_amd import synth
    from conette_amd.engine import Engine
    from oracle import cpu_ref as O

    w = {k: v for k, v in O.to_torch(synth.synth_state_dict()).items() if k.startswith("model.")}
    v = int(w["model.decoder.classifier.weight"].shape[0])
    props = torch.cuda.get_device_properties(0)
    names = ("plain", "idle", "ban", "ngram", "masks", "prefix")
    lines = [f"device: {props.name}, {props.multi_processor_count} CUs; torch {torch.__version__}; V = {v}, B = {B}, T = {T_AUDIO}, "
             f"max_pred = min_pred = {MAX_PRED}; median of {args.iters} after {args.warmup} warm-up, paths alternating; ms per whole search",
             "",
             "| precision | W | step kernel | " + " | ".join(f"{n} eager" for n in names) + " | " + " | ".join(f"{n} graph" for n in names) +
             " | per step (us), graph: idle - plain | ban - idle | ngram - idle | masks - idle |",
             "|" + "---|" * (3 + 2 * len(names) + 4)]
    rng = np.random.Generator(np.random.PCG64(4243))
    fe = torch.from_numpy(((rng.random((B, T_AUDIO, 768)) * 2 - 1) * 1.1).astype(np.float32)).cuda()
    lens = torch.full((B,), T_AUDIO, dtype=torch.int32, device="cuda")
    bos = w["model.task_id_to_token_id"][torch.arange(B) % 7].int().cuda()
    forbid = w["model.forbid_rep_mask"].to(torch.uint8).cuda()
    words = torch.from_numpy(rng.permutation(np.arange(4, v - 7))).int()          # ids of words: behind the specials, before the task tokens
    ban = torch.zeros(v, dtype=torch.uint8)
    ban[words[:N_BANNED].long()] = 1
    ban = ban.cuda()
    prefix = torch.stack([words[N_BANNED + PREFIX_LEN * i: N_BANNED + PREFIX_LEN * (i + 1)] for i in range(B)]).cuda()
    plens = torch.full((B,), PREFIX_LEN, dtype=torch.int32, device="cuda")
    for prec in args.precisions.split(","):
        eng = Engine(w, precision=prec)
        eng.set_decode_graph(False)
        for beam in BEAMS:
            con = lambda **kw: eng.decode_constrained(fe, lens, bos, forbid, beam, MAX_PRED, MAX_PRED, check=False, **kw)
            fns = [lambda: eng.decode(fe, lens, bos, forbid, beam, MAX_PRED, MAX_PRED), lambda: con(),
                   lambda: con(ban_mask=ban), lambda: con(no_repeat_ngram=3), lambda: con(ban_mask=ban, no_repeat_ngram=3),
                   lambda: con(prefix=prefix, prefix_lens=plens)]
            eager = median_ms(fns, args.iters, args.warmup)
            graphs = []
            for fn in fns:
                fn()
                torch.cuda.synchronize()
                cg = torch.cuda.CUDAGraph()
                with torch.cuda.graph(cg):
                    held = fn()
                graphs.append((cg, held))
            replay = median_ms([gr.replay for gr, _ in graphs], args.iters, args.warmup)
            kernel = "register" if (v <= 8192 and beam <= 8) else "generic"
            lines.append(f"| {prec} | {beam} | {kernel} | " + " | ".join(f"{x:.3f}" for x in eager + replay) +
                         " | " + " | ".join(f"{(replay[i] - replay[j]) * 1000.0 / MAX_PRED:+.1f}" for i, j in ((1, 0), (2, 1), (3, 1), (4, 1))) + " |")
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
