"""Caption scoring, fused against today's way, on the synthetic checkpoint (decoder-only contexts).

For every precision and (N clips, M captions per clip, L positions) in {(64, 1, 22), (64, 5, 22), (64, 64, 22)}:
  fused : Engine.score(frame_embs, ..., caps_per_audio=M) -- conette_score, automatic vocabulary split
  today : Engine.forcing on M-times repeated embeddings + torch.log_softmax + gather + masked sum
milliseconds (median of --iters after --warmup, both paths alternating in one process on one device) and
torch.cuda.max_memory_allocated of each, plus the number of vocabulary slabs the fused kernel ran with ('x k': Engine.score split the
call into k calls to keep its workspace under 1 GiB).

    python tools/score_bench.py [--iters 20] [--warmup 3] [--precisions bf16,f16,exact,fp32] [--out profiles/score_bench.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((64, 1, 22), (64, 5, 22), (64, 64, 22))
T_AUDIO = 32            # frames of a 10 s clip
SC_BM, SC_BN, SC_MAX_AUTO_SLABS = 64, 128, 21          # csrc/dec_score.h


def auto_slabs(r, v, n_cu):
    return max(1, min((2 * n_cu) // -(-r // SC_BM), SC_MAX_AUTO_SLABS, -(-v // SC_BN)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--precisions", default="bf16,f16,exact,fp32")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import conette_amd  # noqa: F401
    from conette_amd import scoring, synth
    from conette_amd.engine import Engine
    from oracle import cpu_ref as O

    w = {k: v for k, v in O.to_torch(synth.synth_state_dict()).items() if k.startswith("model.")}
    v = int(w["model.decoder.classifier.weight"].shape[0])
    props = torch.cuda.get_device_properties(0)
    lines = [f"device: {props.name}, {props.multi_processor_count} CUs; torch {torch.__version__}; V = {v}, T = {T_AUDIO}, "
             f"median of {args.iters} after {args.warmup} warm-up, paths alternating",
             f"{'precision':9} {'N x M x L':>12} {'rows':>6} {'S':>6} {'fused ms':>9} {'today ms':>9} {'ratio':>6} {'fused MB':>9} {'today MB':>9}"]
    rng = np.random.Generator(np.random.PCG64(4242))
    for prec in args.precisions.split(","):
        eng = Engine(w, precision=prec)
        for n, m, cap_len in SHAPES:
            fe = torch.from_numpy(((rng.random((n, T_AUDIO, 768)) * 2 - 1) * 1.1).astype(np.float32)).cuda()
            lens = torch.full((n,), T_AUDIO, dtype=torch.int32, device="cuda")
            caps = np.zeros((n * m, cap_len + 1), dtype=np.int64)
            for i in range(n * m):
                k = 1 + int(rng.integers(cap_len // 2, cap_len))
                caps[i, 0] = int(w["model.task_id_to_token_id"][i % 7])
                caps[i, 1:k] = 4 + rng.integers(0, v - 11, k - 1)
                caps[i, k] = 2
            caps_in = torch.from_numpy(caps[:, :-1].copy()).int().cuda()
            tg = torch.from_numpy(caps[:, 1:].copy()).int().cuda()
            idx = tg.long()[..., None]

            def fused():
                return eng.score(fe, lens, caps_in, tg, caps_per_audio=m, want_tokens=False)["sum_lprobs"]

            def today():
                fe_rep, lens_rep = fe.repeat_interleave(m, dim=0), lens.repeat_interleave(m)
                lp = torch.log_softmax(eng.forcing(fe_rep, lens_rep, caps_in), dim=-1).gather(2, idx)[..., 0]
                return torch.where(tg != 0, lp, torch.zeros_like(lp)).sum(dim=1)

            res = {}
            for name, fn in (("fused", fused), ("today", today)):
                eng._ws.clear()
                torch.cuda.empty_cache()
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                out = fn()
                torch.cuda.synchronize()
                res[name + "_mb"] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
                res[name + "_out"] = out.cpu()
            assert torch.allclose(res["fused_out"], res["today_out"], rtol=0, atol=cap_len * (1e-3 if prec in ("bf16", "f16") else 1e-4))
            ms = {"fused": [], "today": []}
            for it in range(args.warmup + args.iters):
                for name, fn in (("fused", fused), ("today", today)):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    fn()
                    b.record()
                    b.synchronize()
                    if it >= args.warmup:
                        ms[name].append(a.elapsed_time(b))
            f_ms, t_ms = float(np.median(ms["fused"])), float(np.median(ms["today"]))
            r = n * m * cap_len
            need = lambda nc, mc: int(eng.lib.conette_score_workspace_bytes(eng._ctx_dec, nc, T_AUDIO, mc, cap_len))
            plan = scoring.plan_chunks(n, m, need, scoring.SCORE_WORKSPACE_BOUND)   # (Engine.score's own split of the call)
            s = "/".join(str(x) for x in sorted({auto_slabs(nc * mc * cap_len, v, props.multi_processor_count) for _, nc, _, mc in plan}))
            s += "" if len(plan) == 1 else f" x{len(plan)}"
            lines.append(f"{prec:9} {f'{n} x {m} x {cap_len}':>12} {r:6d} {s!s:>6} {f_ms:9.3f} {t_ms:9.3f} {t_ms / f_ms:6.2f} "
                         f"{res['fused_mb']:9.1f} {res['today_mb']:9.1f}")
            print(lines[-1], flush=True)
        del eng
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
