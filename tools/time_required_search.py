"""Keyword-guided beam search beside the constrained search, on the benchmark's synthetic checkpoint (decoder-only contexts).

B = 64 clips, T = 31 frames, beam 3, max_pred = 20, min_pred as the checkpoint's config has it, forbid mask on, no prefix, no ban
mask, no n-gram rule.  In ONE process on one device, HIP events around each call, the median of --iters calls after --warmup:
  constrained : Engine.decode_constrained                                   -- this tree's build
  width 0     : Engine.decode_required, no table                            -- runs the constrained step kernel
  G = 2       : Engine.decode_required, 2 one-word groups per clip          -- the register kernel of dec_require.h
  G = 8       : Engine.decode_required, 8 groups of 1 to 3 words per clip
  parent      : Engine.decode_constrained of the library at --parent_lib (a build of the parent commit), --repeats medians: their
                spread is the yardstick for the differences above
The required words of a clip are drawn from the words the unrequired search of that clip does not use.

With --min_pred 20 no row ends before step 20 in any of the searches: the times then compare step kernels, not caption lengths.

    python tools/time_required_search.py [--parent_lib PATH] [--iters 50] [--warmup 5] [--repeats 5] [--precisions bf16,exact]
                                         [--min_pred N] [--out FILE]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, T_AUDIO, BEAM, MAX_PRED = 64, 31, 3, 20


def median_ms(fn, iters, warmup):
    times = []
    for it in range(warmup + iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if it >= warmup:
            times.append(a.elapsed_time(b))
    return float(np.median(times))


def parent_engine(path, weights, prec):
    """an Engine on another build of the library: entry points that build lacks are left unbound"""
    from conette_amd import engine

    class _Unbound:
        restype = argtypes = None

    class _Tolerant(C.CDLL):
        def __getattr__(self, name):
            try:
                return super().__getattr__(name)
            except AttributeError:
                if name.startswith("conette_"):
                    return _Unbound()
                raise
    saved = engine._lib, engine.LIB_PATH, C.CDLL
    engine._lib, engine.LIB_PATH, C.CDLL = None, path, _Tolerant
    try:
        return engine.Engine(weights, precision=prec)
    finally:
        engine._lib, engine.LIB_PATH, C.CDLL = saved


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent_lib", default=None)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--precisions", default="bf16,exact")
    ap.add_argument("--min_pred", type=int, default=None, help="default: the checkpoint's; max_pred makes every row run every step")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import conette_amd  # noqa: F401
    from conette_amd import required_search as RS
    from conette_amd import synth
    from conette_amd.engine import Engine
    from oracle import cpu_ref as O

    w = {k: v for k, v in O.to_torch(synth.synth_state_dict()).items() if k.startswith("model.")}
    v = int(w["model.decoder.classifier.weight"].shape[0])
    min_pred = int(synth.synth_config_dict()["min_pred_size"]) if args.min_pred is None else args.min_pred
    props = torch.cuda.get_device_properties(0)
    lines = [f"device: {props.name}, {props.multi_processor_count} CUs; torch {torch.__version__}; V = {v}, B = {B}, T = {T_AUDIO}, beam {BEAM}, "
             f"max_pred = {MAX_PRED}, min_pred = {min_pred}; median of {args.iters} calls after {args.warmup}; ms per whole search", "",
             "| precision | constrained | width 0 | G = 2 | G = 8 | parent's constrained: medians | parent: min .. max (spread) | "
             "width 0 - parent median | G = 2 / constrained | G = 8 / constrained |", "|" + "---|" * 10]
    rng = np.random.Generator(np.random.PCG64(4243))
    fe = torch.from_numpy(((rng.random((B, T_AUDIO, 768)) * 2 - 1) * 1.1).astype(np.float32)).cuda()
    lens = torch.full((B,), T_AUDIO, dtype=torch.int32, device="cuda")
    bos = w["model.task_id_to_token_id"][torch.arange(B) % 7].int().cuda()
    forbid = w["model.forbid_rep_mask"].to(torch.uint8).cuda()
    for prec in args.precisions.split(","):
        eng = Engine(w, precision=prec)
        con = lambda e=eng: e.decode_constrained(fe, lens, bos, forbid, BEAM, min_pred, MAX_PRED, check=False)
        used = con()["mult_preds"].cpu()
        tables = {}
        for g_n in (2, 8):
            req = []
            for b in range(B):
                free = [t for t in rng.permutation(np.arange(4, v - 7)).tolist() if t not in set(used[b].reshape(-1).tolist())]
                req.append([[free.pop() for _ in range(1 if g_n == 2 else 1 + g % 3)] for g in range(g_n)])
            rt, rg = RS.pack_tables(req)
            tables[g_n] = (torch.from_numpy(rt).cuda(), torch.from_numpy(rg).cuda())
        reqd = lambda t: eng.decode_required(fe, lens, bos, forbid, BEAM, min_pred, MAX_PRED, req_tokens=t[0], req_groups=t[1], check=False)
        t_con = median_ms(con, args.iters, args.warmup)
        t_w0 = median_ms(lambda: eng.decode_required(fe, lens, bos, forbid, BEAM, min_pred, MAX_PRED, check=False), args.iters, args.warmup)
        t_g2 = median_ms(lambda: reqd(tables[2]), args.iters, args.warmup)
        t_g8 = median_ms(lambda: reqd(tables[8]), args.iters, args.warmup)
        parent = []
        if args.parent_lib:
            old = parent_engine(os.path.abspath(args.parent_lib), w, prec)
            parent = [median_ms(lambda: con(old), args.iters, args.warmup) for _ in range(args.repeats)]
            del old
        pm = float(np.median(parent)) if parent else float("nan")
        spread = (max(parent) - min(parent)) if parent else float("nan")
        lines.append(f"| {prec} | {t_con:.3f} | {t_w0:.3f} | {t_g2:.3f} | {t_g8:.3f} | " + (" ".join(f"{x:.3f}" for x in parent) or "-") +
                     f" | {min(parent) if parent else float('nan'):.3f} .. {max(parent) if parent else float('nan'):.3f} ({spread:.3f}) | "
                     f"{t_w0 - pm:+.3f} | {t_g2 / t_con:.4f} | {t_g8 / t_con:.4f} |")
        del eng
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
