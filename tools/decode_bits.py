#!/usr/bin/env python
"""Every output of the decoder entry points on the deterministic cases of tests/decoder_geometry.py, as bit patterns:

    python tools/decode_bits.py OUT.npz             # run on a GPU, from the tree whose library is to be recorded
    python tools/decode_bits.py --compare A.npz B.npz

Per geometry, at bf16 and exact: every search through ``decode`` (trace, margins and step-0 logits on), ``greedy`` on the beam-1
searches, ``sample`` on the first search (3 samples, seeded CPU uniforms, unfiltered and with temperature 0.7 / top-k 5 / top-p 0.9,
token log-probs and step logits on; V > 8192 reaches the generic variant), ``forcing`` in its three modes, ``score`` and ``align``
on the forcing case.  Floats are stored as their int32 bit patterns, so two builds that compute the same thing give bytewise equal
files; --compare lists every array that differs and exits non-zero if any does."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PRECISIONS = ("bf16", "exact")
MODES = ("step_fused", "step_unfused", "onepass")


def compare(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    bad = sorted(set(a.files) ^ set(b.files))
    n_bytes = 0
    for k in sorted(set(a.files) & set(b.files)):
        x, y = a[k], b[k]
        n_bytes += x.nbytes
        if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
            bad.append(k)
    print(f"{len(a.files)} / {len(b.files)} arrays, {n_bytes} bytes compared, {len(bad)} differ")
    for k in bad:
        print("  differs:", k)
    return 1 if bad else 0


def record(out_path):
    import torch
    from conette_amd.engine import Engine
    from tests import decoder_geometry as D

    arrays = {}

    def put(key, t):
        if t is None:
            return
        t = t.detach().cpu().contiguous()
        assert key not in arrays, key
        arrays[key] = (t.view(torch.int32) if t.dtype == torch.float32 else t).numpy()

    def put_all(prefix, out):
        for k, v in out.items():
            put(f"{prefix}/{k}", v)

    side = torch.cuda.Stream()
    for g in D.GEOMETRIES:
        for prec in PRECISIONS:
            eng = Engine(D.weights(g), precision=prec, n_layers=g.n_layers, d_ff=g.d_ff)
            for i, s in enumerate(g.searches):
                fe, shape, bos, forbid = D.search_inputs(g, s)
                lens = shape[:, 1].int()
                tag = f"{g.name}/{prec}/{s.name}"
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    out = eng.decode(fe.cuda(), lens, bos, forbid, s.beam, s.min_pred, s.max_pred, want_step0_logits=True,
                                     want_trace=True, want_margins=True)
                torch.cuda.synchronize()
                put_all(tag + "/decode", out)
                if s.beam == 1:
                    put_all(tag + "/greedy", eng.greedy(fe.cuda(), lens, bos, forbid, s.min_pred, s.max_pred))
                if i == 0:
                    gen = torch.Generator().manual_seed(1234 + s.seed)
                    uni = torch.rand((s.max_pred, s.b, 3), dtype=torch.float32, generator=gen)
                    for name, kw in (("plain", {}), ("filtered", dict(temperature=0.7, top_k=5, top_p=0.9))):
                        sm = eng.sample(fe.cuda(), lens, bos, forbid, 3, s.min_pred, s.max_pred, uniforms=uni, want_tokens=True,
                                        want_logits=True, **kw)
                        # a finished row takes no further decision: its later step logits are never written
                        after = torch.arange(s.max_pred, device=sm["lens"].device)[None, None, :] >= sm["lens"][:, :, None]
                        sm["step_logits"].masked_fill_(after[..., None], 0.0)
                        put_all(f"{tag}/sample_{name}", sm)
            f = g.forcing
            fe, shape, caps = D.forcing_inputs(g, f)
            lens = shape[:, 1].int()
            tag = f"{g.name}/{prec}/{f.name}"
            for mode in MODES:
                eng.set_decode_fusion(mode == "step_fused")
                eng.set_forcing_stepwise(mode != "onepass")
                try:
                    put(f"{tag}/forcing_{mode}", eng.forcing(fe.cuda(), lens, caps))
                finally:
                    eng.set_decode_fusion(True)
                    eng.set_forcing_stepwise(False)
            targets = torch.cat([caps[:, 1:], caps[:, :1]], dim=1)   # next token; the last position predicts the task token
            put_all(tag + "/score", eng.score(fe.cuda(), lens, caps, targets))
            put_all(tag + "/align", eng.align(fe.cuda(), lens, caps, targets, per_layer=True))
            torch.cuda.synchronize()
            del eng
            print(f"{g.name}/{prec}: {len(arrays)} arrays so far", flush=True)
        D.drop_weights(g)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    np.savez(out_path, **arrays)
    print(f"wrote {out_path}: {len(arrays)} arrays, {sum(a.nbytes for a in arrays.values())} bytes")


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    record(sys.argv[1])
