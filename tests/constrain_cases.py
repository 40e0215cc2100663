"""The cases of the constrained beam search tests (conette_decode_constrained, csrc/dec_constrain.h) and their runs through the CPU
restatement (conette_amd/constrained_search.py) on the oracle's logits (oracle/cpu_ref.py).

tests/test_cpu_constrained_search.py holds every case to the input conditions the GPU tests rely on;
tests/test_gpu_constrained_search.py runs them.  Geometries, weights and frames are those of tests/decoder_geometry.py, batches and
memory lengths those of tests/group_cases.py (1, 3 and 5 clips, ragged frame lengths).

The table.  Beams 1, 3, 4 (register kernel, NR 4), 5, 8 (NR 8), 9, 16 (generic kernel), every one of them at v8193_ff4096_l2
(generic at any beam).  Prefix lengths are ragged inside a batch -- (L,), (0, 1, L), (2, 0, L, 1, 3), each capped at
max_pred - 1 -- with L = max_pred - 1 in a third of the table (the fan-out is then the last step: all its picks finish) and one
case of max_pred 64 with L = 62.  A prefix is distinct word tokens drawn from the case's seed: it repeats no token, so neither the
forbid mask nor the n-gram rule voids it.  n in {0, 2, 3}, ban mask off or on, forbid mask on or off, min_pred in {0, 3, max_pred}.
The ban mask of a case is every token the same search without ban mask and n-gram rule picks at a clip's first free step (<eos>
and the prefix tokens left out).

Seeds: per case the first of 0, 1, 2 ... at which the restatement's search on the oracle's logits has every free call's effective
margin at or above decoder_geometry.MIN_MARGIN and, where n > 0 or a ban is on, at least one call whose picks differ from the
unconstrained picks of the same state (the CPU test recomputes both)."""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional, Tuple

from tests import decoder_geometry as D
from tests import group_cases as GC

EOS, PAD = GC.EOS, GC.PAD
SHAPES = GC.SHAPES
GEOS = GC.GEOS
REGISTER_W = (1, 3, 4, 5, 8)
GENERIC_W = (9, 16)
ALL_W = REGISTER_W + GENERIC_W
NGRAMS = (2, 3, 0)


class Case(NamedTuple):
    geo: str
    name: str
    w: int
    b: int
    ta: int
    frame_lens: Tuple[int, ...]
    plens: Tuple[int, ...]
    n: int
    ban: bool
    forbid: bool
    min_pred: int
    max_pred: int
    seed: int

    def __repr__(self):
        return (f"{self.geo}/{self.name}(W={self.w}, B={self.b}, plens={self.plens}, n={self.n}, ban={self.ban}, forbid={self.forbid}, "
                f"min={self.min_pred}, max={self.max_pred}, seed={self.seed})")


def _row(i: int, w: int, max_pred: int = 10):
    """(W, index of SHAPES, L, n, ban, forbid, min_pred, max_pred) of the i-th row of a geometry's table.  The n-gram rule alone
    (no ban) goes with the forbid mask off: where every word may occur once, no n-gram can occur twice."""
    n = NGRAMS[i % 3]
    ban = i % 2 == 1 or n == 0
    if i % 7 == 6:
        n, ban = 0, True
    forbid = ban and i % 4 != 3
    min_pred = (3, 0, max_pred)[(i // 2) % 3]
    long = max_pred - 1 if i % 3 == 1 else 2 + i % 3
    return (w, i % 3, long, n, ban, forbid, min_pred, max_pred)


_TABLE: Dict[str, Tuple[Tuple, ...]] = {
    # (beam 16 at 31 tokens: a ban mask of 16 of the 20 words would leave the search the tied logits of the special tokens)
    "v31_ff32_l2": tuple(_row(i, w) for i, w in enumerate(ALL_W[:-1])) + ((16, 0, 2, 2, False, False, 3, 10),),
    "v2049_ff256_l6": tuple(_row(i + 1, w, 12 if w == 4 else 10) for i, w in enumerate(ALL_W)) + ((3, 1, 62, 2, False, False, 64, 64),),
    "v4097_ff1792_l1": tuple(_row(i + 2, w) for i, w in enumerate((3, 5, 9))),
    # (beam 1 over 8 steps repeats no bigram at any seed tried: its n-gram rule runs beside a ban mask)
    "v8192_ff2304_l6": ((1, 0, 2, 2, True, False, 3, 8),) + tuple(_row(i + 1, w, 8) for i, w in enumerate((4, 8, 16))),
    "v8193_ff4096_l2": tuple(_row(i + 3, w, 8) for i, w in enumerate(ALL_W)),
}
# seeds that replace the 0 of the table: the first seed at which the case meets both conditions of the docstring
SEEDS: Dict[Tuple[str, str], int] = {
    ("v31_ff32_l2", "w9_L4_n0_ban1_fb1_p10-10"): 5, ("v2049_ff256_l6", "w16_L9_n3_ban1_fb0_p3-10"): 2,
    ("v2049_ff256_l6", "w3_L62_n2_ban0_fb0_p64-64"): 3, ("v4097_ff1792_l1", "w9_L9_n3_ban0_fb0_p10-10"): 2,
    ("v8192_ff2304_l6", "w16_L2_n2_ban1_fb0_p0-8"): 1, ("v8193_ff4096_l2", "w3_L7_n3_ban0_fb0_p8-8"): 1,
}


def _plens(b: int, long: int, max_pred: int) -> Tuple[int, ...]:
    raw = {1: (long,), 3: (0, 1, long), 5: (2, 0, long, 1, 3)}[b]
    return tuple(min(p, max_pred - 1) for p in raw)


def cases(geo: str) -> List[Case]:
    out = []
    for w, si, long, n, ban, forbid, min_pred, max_pred in _TABLE[geo]:
        b, ta, lens = SHAPES[si]
        name = f"w{w}_L{long}_n{n}_ban{int(ban)}_fb{int(forbid)}_p{min_pred}-{max_pred}"
        out.append(Case(geo, name, w, b, ta, lens, _plens(b, long, max_pred), n, ban, forbid, min_pred, max_pred,
                        SEEDS.get((geo, name), 0)))
    assert len({c.name for c in out}) == len(out)
    return out


def all_cases() -> List[Case]:
    return [c for geo in GEOS for c in cases(geo)]


def prefixes(c: Case) -> List[List[int]]:
    """Clip i's prefix: plens[i] distinct word tokens (ids at or above the specials and the task tokens), from the case's seed."""
    import torch
    v = D.geometry(c.geo).v
    gen = torch.Generator().manual_seed(7000 + c.seed)
    out = []
    for p in c.plens:
        perm = torch.randperm(v - D.N_SPECIALS_AND_TASKS, generator=gen)[:p] + D.N_SPECIALS_AND_TASKS
        out.append([int(t) for t in perm])
    return out


def inputs(c: Case):
    """(frame_embs (B, Ta, 768), audio_shape (B, 2), bos (B,) int64, forbid (V,) bool or None, prefix (B, P) int64 padded with
    PAD, prefix_lens (B,) int64)"""
    import torch
    fe, shape, bos, forbid = GC.inputs(GC.Case(c.geo, c.name, 1, c.w, 0.0, c.b, c.ta, c.frame_lens, c.min_pred, c.max_pred, c.forbid, c.seed))
    pre = prefixes(c)
    width = max(c.plens)
    table = torch.full((c.b, width), PAD, dtype=torch.long)
    for i, p in enumerate(pre):
        table[i, :len(p)] = torch.as_tensor(p, dtype=torch.long)
    return fe, shape, bos, forbid, table, torch.as_tensor(c.plens, dtype=torch.long)


_FNS: Dict[Case, object] = {}
_RUNS: Dict[Tuple[Case, bool], dict] = {}
_BANS: Dict[Case, object] = {}


def _logits_fn(c: Case):
    """one remembered oracle pass per distinct (clip, sequence): the constrained and the unconstrained run of a case see equal bits"""
    if c not in _FNS:
        fe, shape = inputs(c)[:2]
        _FNS[c] = GC.oracle_logits_fn(c.geo, fe, shape, rowwise=True)
    return _FNS[c]


def oracle_run(c: Case, constrained: bool = True) -> dict:
    """The restatement's search of the case on the oracle's logits (cached).  ``constrained`` False: the same search, prefixes
    included, without the ban mask and the n-gram rule."""
    from conette_amd import constrained_search as CS
    key = (c, constrained)
    if key not in _RUNS:
        _, _, bos, forbid = inputs(c)[:4]
        fb = None if forbid is None else forbid.numpy()
        ban = ban_mask(c) if constrained else None
        _RUNS[key] = CS.constrained_search(_logits_fn(c), bos.tolist(), c.w, c.min_pred, c.max_pred, D.geometry(c.geo).v, EOS, PAD, fb,
                                           prefixes(c), None if ban is None else ban.numpy(), c.n if constrained else 0)
    return _RUNS[key]


def ban_mask(c: Case):
    """(V,) bool or None: the tokens the unconstrained search picks at each clip's first free step, <eos> and prefix tokens left out"""
    import torch
    if not c.ban:
        return None
    if c not in _BANS:
        res = oracle_run(c, constrained=False)
        keep_out = {EOS} | {t for p in prefixes(c) for t in p}
        mask = torch.zeros(D.geometry(c.geo).v, dtype=torch.bool)
        for call in res["calls"]:
            if not call["forced"] and call["step"] == c.plens[call["clip"]]:
                for t in call["tokens"]:
                    if t not in keep_out:
                        mask[t] = True
        _BANS[c] = mask
    return _BANS[c]


def drop_runs(c: Optional[Case] = None) -> None:
    for d in (_FNS, _BANS):
        if c is None:
            d.clear()
        else:
            d.pop(c, None)
    for k in [k for k in _RUNS if c is None or k[0] == c]:
        _RUNS.pop(k)


def facts(c: Case) -> Tuple[float, int, int]:
    """(smallest effective margin of the free calls, free calls whose picks differ from the unconstrained picks of their state, calls)"""
    res = oracle_run(c)
    free = [k for k in res["calls"] if not k["forced"]]
    differs = sum(1 for k in free if list(zip(k["parents"], k["tokens"])) != k["plain"])
    return min(k["margin"] for k in free), differs, len(res["calls"])


def meets_conditions(c: Case) -> bool:
    margin, differs, _ = facts(c)
    return margin >= D.MIN_MARGIN and (differs >= 1 or not (c.n > 0 or c.ban))
