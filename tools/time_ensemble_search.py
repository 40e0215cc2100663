"""Ensemble beam search beside M plain searches of the same beam, on the synthetic checkpoint's decoder (decoder-only contexts).

B = 64 clips, T = 31 frames, max_pred = 20; min_pred = 20 too, so that every row searches through all 20 steps in every search and
the times compare kernels, not caption lengths.  For M in 1 .. 4 and beam in 1, 3, 8 (members: the synthetic decoder at seeds
0 .. M - 1, each with its own frame embeddings, rule "logprob"; --combine prob for the mixture):
  ensemble : Engine.decode_ensemble(M members)          -- conette_decode_ensemble: M forwards + one search-step launch per step
  plain    : Engine.decode(beam) on each of the M engines, one after another -- M x (forward + search step) per step
Both in one process on one device at one build, alternating, median of --iters after --warmup, milliseconds per whole search, each
call captured once into a torch.cuda.CUDAGraph and replayed (device time without launch overhead).  Beside them the step kernel's
own time: the "search" class of the library's profiler (event pairs around the step launch, eager), microseconds per step, of the
ensemble step and of ONE plain search's step.
The expectation under test: one ensemble costs about M plain forwards plus one step launch -- `ensemble / plain` at or a little
below 1 --, and the M = 1 ensemble costs what the plain search costs.

    python tools/time_ensemble_search.py [--iters 20] [--warmup 3] [--precisions bf16,exact] [--combine logprob] [--out FILE.md]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MEMBERS = (1, 2, 3, 4)
BEAMS = (1, 3, 8)
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


def step_us(eng, fn, reps=3):
    """microseconds per search-step launch of `fn` (the profiler's "search" class on `eng`'s decoder context)"""
    eng.profile_enable(("search",))
    try:
        fn()
        torch.cuda.synchronize()
        eng.profile_read()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        ms, n = eng.profile_read().get("search", (0.0, 0))
    finally:
        eng.profile_enable(())
    return 1000.0 * ms / max(n, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--precisions", default="bf16,exact")
    ap.add_argument("--combine", default="logprob")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import conette_amd  # noqa: F401
    from conette_amd import synth
    from conette_amd.engine import Engine
    from oracle import cpu_ref as O

    ws = [{k: v for k, v in O.to_torch(synth.synth_state_dict(seed=s)).items() if k.startswith("model.")} for s in range(max(MEMBERS))]
    v = int(ws[0]["model.decoder.classifier.weight"].shape[0])
    props = torch.cuda.get_device_properties(0)
    lines = [f"device: {props.name}, {props.multi_processor_count} CUs; torch {torch.__version__}; V = {v}, B = {B}, T = {T_AUDIO}, "
             f"max_pred = min_pred = {MAX_PRED}, combine = {args.combine}; median of {args.iters} after {args.warmup} warm-up, paths alternating, "
             "graph replay; ms per whole search, us per step launch",
             "",
             "| precision | M | beam | step kernel | ensemble (ms) | M plain searches (ms) | ensemble / plain | one plain search (ms) | "
             "ensemble step (us) | plain step (us) |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    rng = np.random.Generator(np.random.PCG64(4243))
    fes = [torch.from_numpy(((rng.random((B, T_AUDIO, 768)) * 2 - 1) * 1.1).astype(np.float32)).cuda() for _ in ws]
    lens = torch.full((B,), T_AUDIO, dtype=torch.int32, device="cuda")
    bos = ws[0]["model.task_id_to_token_id"][torch.arange(B) % 7].int().cuda()
    forbid = ws[0]["model.forbid_rep_mask"].to(torch.uint8).cuda()
    for prec in args.precisions.split(","):
        engs = [Engine(w, precision=prec) for w in ws]
        for e in engs:
            e.set_decode_graph(False)
        for beam in BEAMS:
            one = lambda: engs[0].decode(fes[0], lens, bos, forbid, beam, MAX_PRED, MAX_PRED)
            plain_step = step_us(engs[0], one)
            for m in MEMBERS:
                members = [(engs[i], fes[i], bos, 1.0) for i in range(m)]
                ens = lambda: engs[0].decode_ensemble(members, lens, forbid, beam, MAX_PRED, MAX_PRED, combine=args.combine)
                plain = lambda: [engs[i].decode(fes[i], lens, bos, forbid, beam, MAX_PRED, MAX_PRED) for i in range(m)]
                graphs = []
                for fn in (ens, plain, one):
                    fn()
                    torch.cuda.synchronize()
                    cg = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(cg):
                        held = fn()
                    graphs.append((cg, held))
                replay = median_ms([gr.replay for gr, _ in graphs], args.iters, args.warmup)
                ens_step = step_us(engs[0], ens)
                vpt = (v + 1023) // 1024
                kernel = "register" if (v <= 8192 and (beam <= 4 or (beam <= 8 and vpt <= 6))) else "generic"
                lines.append(f"| {prec} | {m} | {beam} | {kernel} | {replay[0]:.3f} | {replay[1]:.3f} | {replay[0] / replay[1]:.3f} | {replay[2]:.3f} | "
                             f"{ens_step:.1f} | {plain_step:.1f} |")
                del graphs
        del engs
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
