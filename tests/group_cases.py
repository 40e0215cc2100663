"""The cases of the diverse beam search tests (conette_decode_groups, csrc/dec_group.h) and their runs through the CPU restatement
(conette_amd/group_search.py) on the oracle's logits (oracle/cpu_ref.py).

tests/test_cpu_group_search.py holds every case to the input conditions the GPU tests rely on; tests/test_gpu_group_search.py
runs them.  Geometries, weights and frames are those of tests/decoder_geometry.py.

The table.  Register kernel (G * W <= 8 and V <= 8192): (G, W) = (1,3) (2,1) (3,1) (2,2) at NR 4 and (3,2) (2,4) (4,2) (8,1) at
NR 8; generic kernel: (3,3) (5,3) (2,8) (16,1) (1,16), and every (G, W) of v8193_ff4096_l2.  Batches of 1, 3 and 5 clips (rows
mod 4 in {0, 1, 2, 3} over the table), memory lengths 1, 7, 8 and 25 with ragged frame lengths, lambda in {0, 0.5, 2}; max_pred =
64 with min_pred = 60, min_pred = max_pred, min_pred = 0, with and without the forbid mask.

Seeds: per case the first of 0, 1, 2 ... at which the restatement's search on the oracle's logits has every call's effective
margin at or above decoder_geometry.MIN_MARGIN and, with lambda > 0 and more than one group, at least one call whose penalised
picks differ from its unpenalised top-k (the CPU test recomputes both)."""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Tuple

from tests import decoder_geometry as D

EOS, PAD = 2, 0
# (B, t_audio, frame_lens)
SHAPES = ((1, 25, (25,)), (3, 8, (8, 7, 1)), (5, 7, (7, 3, 5, 1, 6)))
LAMBDAS = (0.5, 2.0, 0.0)
REGISTER_GW = ((1, 3), (2, 1), (3, 1), (2, 2), (3, 2), (2, 4), (4, 2), (8, 1))
GENERIC_GW = ((3, 3), (5, 3), (2, 8), (16, 1), (1, 16))
GEOS = ("v31_ff32_l2", "v2049_ff256_l6", "v4097_ff1792_l1", "v8192_ff2304_l6", "v8193_ff4096_l2")


class Case(NamedTuple):
    geo: str
    name: str
    g: int
    w: int
    lam: float
    b: int
    ta: int
    frame_lens: Tuple[int, ...]
    min_pred: int
    max_pred: int
    forbid: bool
    seed: int

    @property
    def rows(self) -> int:
        return self.b * self.g * self.w

    def __repr__(self):
        return (f"{self.geo}/{self.name}(G={self.g}, W={self.w}, lambda={self.lam}, B={self.b}, min={self.min_pred}, max={self.max_pred}, "
                f"forbid={self.forbid}, seed={self.seed})")


# per geometry: (G, W) -> (index of SHAPES, index of LAMBDAS, min_pred, max_pred, forbid, seed)
_TABLE: Dict[str, Tuple[Tuple, ...]] = {
    "v31_ff32_l2": tuple(((gw, i % 3, i % 3, (3, 0)[i % 2], 10, i % 4 != 1, 0) for i, gw in enumerate(REGISTER_GW + GENERIC_GW))),
    "v2049_ff256_l6": tuple(((gw, (i + 1) % 3, (i + 2) % 3, (3, 0)[(i // 2) % 2], 10, i % 4 != 2, 0)
                             for i, gw in enumerate(REGISTER_GW + GENERIC_GW))) + (((2, 2), 1, 0, 60, 64, True, 0),),
    "v4097_ff1792_l1": (((2, 2), 2, 0, 3, 10, True, 0), ((3, 2), 1, 1, 3, 10, True, 0), ((3, 3), 0, 0, 0, 10, False, 0),
                        ((2, 1), 1, 1, 9, 9, True, 0)),
    "v8192_ff2304_l6": (((3, 1), 1, 0, 3, 8, True, 0), ((2, 4), 2, 1, 3, 8, True, 0), ((8, 1), 0, 0, 0, 8, False, 0),
                        ((5, 3), 1, 1, 3, 6, True, 0)),
    "v8193_ff4096_l2": (((1, 3), 1, 0, 3, 10, True, 0), ((2, 1), 2, 1, 0, 10, False, 0), ((2, 2), 0, 0, 3, 10, True, 0),
                        ((4, 2), 1, 1, 3, 10, True, 0), ((2, 8), 1, 0, 3, 8, True, 0), ((16, 1), 0, 1, 3, 8, True, 0),
                        ((1, 16), 1, 2, 3, 8, False, 0), ((3, 3), 2, 2, 3, 8, True, 0)),
}
# seeds that replace the 0 of the table: the first seed at which the case meets the margin condition (smallest margins found:
# 0.0033 / 0.0025 / 0.0101 / 0.0090 / 0.0051 / 0.0026) and, in the last two entries, at which the penalty changes a pick at all
# (at seed 0 those searches are decided by gaps larger than the penalty)
SEEDS: Dict[Tuple[str, str], int] = {
    ("v2049_ff256_l6", "g2w8_l0.5_p0-10"): 9, ("v2049_ff256_l6", "g1w16_l0.0_p3-10"): 5, ("v2049_ff256_l6", "g2w2_l0.5_p60-64"): 1,
    ("v8192_ff2304_l6", "g3w1_l0.5_p3-8"): 1, ("v8192_ff2304_l6", "g2w4_l2.0_p3-8"): 6, ("v8193_ff4096_l2", "g1w16_l0.0_p3-8"): 2,
    ("v8193_ff4096_l2", "g2w1_l2.0_p0-10"): 1, ("v31_ff32_l2", "g2w2_l0.5_p0-10"): 3,
}


def _name(gw, lam, min_pred, max_pred) -> str:
    return f"g{gw[0]}w{gw[1]}_l{lam}_p{min_pred}-{max_pred}"


def cases(geo: str) -> List[Case]:
    out = []
    for gw, si, li, min_pred, max_pred, forbid, seed in _TABLE[geo]:
        b, ta, lens = SHAPES[si]
        name = _name(gw, LAMBDAS[li], min_pred, max_pred)
        out.append(Case(geo, name, gw[0], gw[1], LAMBDAS[li], b, ta, lens, min_pred, max_pred, forbid, SEEDS.get((geo, name), seed)))
    assert len({c.name for c in out}) == len(out)
    return out


def all_cases() -> List[Case]:
    return [c for geo in GEOS for c in cases(geo)]


def inputs(c: Case):
    """(frame_embs (B, Ta, 768), audio_shape (B, 2), bos (B,) int64, forbid (V,) bool or None): clip i is prompted with task (seed + i) % 7."""
    import torch
    w = D.weights(D.geometry(c.geo))
    fe, shape = D.frames(c.b, c.ta, c.frame_lens, 500 + c.seed)
    bos = w["model.task_id_to_token_id"][torch.as_tensor([(c.seed + i) % 7 for i in range(c.b)])]
    return fe, shape, bos, (w["model.forbid_rep_mask"].bool() if c.forbid else None)


def oracle_logits_fn(geo: str, fe, shape, rowwise: bool = False):
    """``logits_fn`` of group_search.group_search on oracle.cpu_ref: every live row's whole prefix re-decoded, as the oracle's own
    search does.  ``rowwise``: one decoder pass per distinct (clip, prefix), remembered -- the logits of a row then do not depend on
    which rows are decoded beside it (the fp32 products of another row count sum in another order), so searches that must take
    the same decisions see the same bits."""
    import numpy as np
    import torch
    from oracle import cpu_ref as O
    g = D.geometry(geo)
    w = D.weights(g)
    with torch.no_grad():
        mem, mask = O.encode_audio(w, fe, shape)

    def decode(clips, prefixes):
        clips = torch.as_tensor(clips)
        caps = torch.as_tensor(prefixes, dtype=torch.long).t().contiguous()
        with torch.no_grad():
            return O.decoder_forward(w, mem[clips].permute(2, 0, 1).contiguous(), mask[clips], caps, 8, g.n_layers)[-1].double().numpy()
    seen: Dict[tuple, object] = {}

    def fn(rows, step):
        if not rowwise:
            return decode([b for b, _ in rows], [p for _, p in rows])
        for b, p in rows:
            if (b, tuple(p)) not in seen:
                seen[(b, tuple(p))] = decode([b], [p])[0]
        return np.stack([seen[(b, tuple(p))] for b, p in rows])
    return fn


_RUNS: Dict[Case, dict] = {}


def oracle_run(c: Case, **override) -> dict:
    """The restatement's search of the case on the oracle's logits (cached; ``override`` replaces g / w / lam, uncached)."""
    from conette_amd import group_search as GS
    if not override and c in _RUNS:
        return _RUNS[c]
    fe, shape, bos, forbid = inputs(c)
    geo = D.geometry(c.geo)
    res = GS.group_search(oracle_logits_fn(c.geo, fe, shape), bos.tolist(), override.get("g", c.g), override.get("w", c.w),
                          override.get("lam", c.lam), c.min_pred, c.max_pred, geo.v, EOS, PAD,
                          None if forbid is None else forbid.numpy())
    if not override:
        _RUNS[c] = res
    return res


def min_margin(res: dict) -> float:
    return min(call["margin"] for call in res["calls"])
