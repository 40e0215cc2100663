"""The sampling step beside the search step, for one kernel trace.

Runs, on the default synthetic decoder (V = 5631, decoder-only bf16 context) at R = 192 rows and 20 steps:
  search : Engine.decode, 24 clips x beam 8                -> cn_search_step3_kernel<8, 8>
  sample : Engine.sample, 12 clips x 16 samples, for (top_k, top_p) in (0, 1), (40, 1), (0, 0.9), (40, 0.9) at T = 1
           -> cn_sample_step_kernel<6>
min_pred = max_pred = 20, so every row takes every step.  Meant to run under a kernel trace; the per-kernel mean durations
of the two step kernels are the figures DESIGN.md quotes (the trace's statistics give one mean over the four sampling settings;
--only picks one setting for a run of its own):

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- python tools/sample_step_trace.py [--only 40,0.9]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T_AUDIO, STEPS, REPEAT = 32, 20, 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None, help="top_k,top_p of the one sampling setting to run")
    args = ap.parse_args()
    import conette_amd  # noqa: F401
    from conette_amd import synth
    from conette_amd.engine import Engine
    from oracle import cpu_ref as O

    w = {k: v for k, v in O.to_torch(synth.synth_state_dict()).items() if k.startswith("model.")}
    eng = Engine(w, precision="bf16")
    eng.set_decode_graph(False)
    rng = np.random.Generator(np.random.PCG64(99))
    forbid = w["model.forbid_rep_mask"].bool()

    def inputs(b):
        fe = torch.from_numpy(((rng.random((b, T_AUDIO, 768)) * 2 - 1) * 1.1).astype(np.float32)).cuda()
        return fe, torch.full((b,), T_AUDIO, dtype=torch.int32), w["model.task_id_to_token_id"][torch.arange(b) % 7]

    settings = [(0, 1.0), (40, 1.0), (0, 0.9), (40, 0.9)]
    if args.only:
        k, p = args.only.split(",")
        settings = [(int(k), float(p))]
    fe, lens, bos = inputs(24)
    for _ in range(REPEAT):
        eng.decode(fe, lens, bos, forbid, 8, STEPS, STEPS)
    fe, lens, bos = inputs(12)
    gen = torch.Generator(device="cuda").manual_seed(0)
    for k, p in settings:
        for _ in range(REPEAT):
            out = eng.sample(fe, lens, bos, forbid, 16, STEPS, STEPS, temperature=1.0, top_k=k, top_p=p, generator=gen)
    torch.cuda.synchronize()
    print("rows", 192, "steps", STEPS, "sampling settings", settings, "last sizes", out["sizes"].tolist())


if __name__ == "__main__":
    main()
