"""The cases of the keyword-guided beam search tests (conette_decode_required, csrc/dec_require.h) and their runs through the CPU
restatement (conette_amd/required_search.py) on the oracle's logits (oracle/cpu_ref.py).

tests/test_cpu_required_search.py holds every case to the input conditions the GPU tests rely on;
tests/test_gpu_required_search.py runs them.  Geometries, weights and frames are those of tests/decoder_geometry.py, batches and
memory lengths those of tests/group_cases.py (1, 3 and 5 clips, ragged frame lengths), prefixes those of tests/constrain_cases.py.

The table.  Beams 1, 3, 4, 5, 8 (register kernel), 9, 16 (generic kernel) and beams 3, 4, 9 at v8193_ff4096_l2 (generic at any
beam); beams 1, 8, 16 at v8192_ff2304_l6, the register kernel's last vocabulary.  Requirements per clip: G in {0, 1, 2, 3, 8},
ragged inside a batch, a clip with G = 0 beside clips with requirements; groups of 1 to 3 alternatives (4 in the case that fills
all 32 table entries); the table entries of a clip lie in shuffled order with -1 gaps.  max_pred 4 to 10, one case at 64.
Modes: ``m5`` -- G so close to max_pred that M5 fires; ``fan`` -- G = max_pred - plen, M5 from the fan-out on; ``short`` -- the
same with three one-token groups at beam 4: the fan-out has three finite candidates for four slots (an M5 row itself cannot run
dry under the argument check: the n-gram rule and the forbid mask only take tokens the row's sequence holds, and a token of an
unmet group is not among them; the shortage M5 can cause is that of a call, here beside the n-gram rule); ``premet`` -- clip 0's
prefix holds a token of its first group; ``allmet`` -- clip 0's prefix holds a token of every one of its groups; ``full32`` -- 8 groups of 4.
With the forbid mask on, a case's required tokens lie inside it (each then occurs once).  Ban mask off or on (a fixed quarter of the words, prefix
tokens left out), n in {0, 2, 3}, min_pred in {0, 3, max_pred}.

Seeds: per case the first of 0, 1, 2 ... at which the restatement's search on the oracle's logits has every free call's effective
margin at or above decoder_geometry.MIN_MARGIN and at least one call whose picks differ from the picks of the same state without
requirements (the CPU test recomputes both)."""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional, Tuple

from tests import constrain_cases as CC
from tests import decoder_geometry as D
from tests import group_cases as GC

EOS, PAD = GC.EOS, GC.PAD
SHAPES = GC.SHAPES
GEOS = GC.GEOS


class Case(NamedTuple):
    geo: str
    name: str
    w: int
    b: int
    ta: int
    frame_lens: Tuple[int, ...]
    plens: Tuple[int, ...]
    gs: Tuple[int, ...]
    n: int
    ban: bool
    forbid: bool
    min_pred: int
    max_pred: int
    mode: str
    seed: int

    def __repr__(self):
        return (f"{self.geo}/{self.name}(W={self.w}, B={self.b}, plens={self.plens}, G={self.gs}, n={self.n}, ban={self.ban}, "
                f"forbid={self.forbid}, min={self.min_pred}, max={self.max_pred}, mode={self.mode!r}, seed={self.seed})")

    @property
    def base(self) -> CC.Case:
        """the constrained search's case with the same inputs"""
        return CC.Case(self.geo, self.name, self.w, self.b, self.ta, self.frame_lens, self.plens, self.n, self.ban, self.forbid,
                       self.min_pred, self.max_pred, self.seed)


# per geometry: (W, index of SHAPES, plens, G per clip, n, ban, forbid, min_pred, max_pred, mode)
_TABLE: Dict[str, Tuple[Tuple, ...]] = {
    "v31_ff32_l2": ((1, 1, (0, 1, 2), (0, 1, 2), 0, False, True, 3, 6, ""),
                    (3, 0, (0,), (3,), 0, False, False, 0, 4, "m5"),
                    (4, 2, (2, 0, 3, 1, 0), (1, 0, 2, 1, 3), 2, False, False, 0, 7, "premet"),
                    (5, 1, (0, 1, 0), (2, 0, 1), 0, True, True, 6, 6, ""),
                    (8, 1, (2, 0, 1), (2, 1, 0), 3, False, False, 3, 8, "allmet"),
                    (9, 1, (0, 0, 1), (2, 3, 0), 0, False, True, 0, 5, "m5")),
    "v2049_ff256_l6": ((4, 1, (0, 2, 1), (8, 0, 3), 0, True, True, 3, 10, "full32"),
                       (16, 0, (0,), (2,), 2, False, False, 3, 6, ""),
                       (3, 0, (60,), (2,), 0, False, False, 64, 64, "m5")),
    "v4097_ff1792_l1": ((5, 2, (0, 1, 0, 2, 0), (1, 2, 0, 3, 1), 0, False, True, 3, 6, "m5"),
                        (9, 0, (1,), (3,), 0, False, False, 0, 4, "fan")),
    "v8192_ff2304_l6": ((1, 1, (0, 0, 1), (2, 0, 1), 2, True, False, 3, 8, ""),
                        (8, 1, (0, 1, 2), (3, 1, 0), 0, False, True, 0, 5, "m5"),
                        (16, 0, (0,), (1,), 0, False, True, 3, 6, "")),
    "v8193_ff4096_l2": ((3, 1, (0, 1, 0), (2, 0, 8), 0, False, True, 3, 9, "m5"),
                        (4, 0, (1,), (3,), 2, False, False, 0, 4, "short"),
                        (9, 2, (0, 2, 0, 1, 0), (1, 2, 0, 3, 2), 3, True, True, 3, 7, "")),
}
M5_MODES = ("m5", "fan", "short")
# seeds that replace the 0 of the table: the first seed at which the case meets both conditions of the docstring
SEEDS: Dict[Tuple[str, str], int] = {
    ("v31_ff32_l2", "w8_b3_G2_n3_ban0_fb0_p3-8_allmet"): 1, ("v4097_ff1792_l1", "w5_b5_G3_n0_ban0_fb1_p3-6_m5"): 2,
}


def cases(geo: str) -> List[Case]:
    out = []
    for w, si, plens, gs, n, ban, forbid, min_pred, max_pred, mode in _TABLE[geo]:
        b, ta, lens = SHAPES[si]
        assert len(plens) == b and len(gs) == b
        name = f"w{w}_b{b}_G{max(gs)}_n{n}_ban{int(ban)}_fb{int(forbid)}_p{min_pred}-{max_pred}{'_' + mode if mode else ''}"
        out.append(Case(geo, name, w, b, ta, lens, plens, gs, n, ban, forbid, min_pred, max_pred, mode, SEEDS.get((geo, name), 0)))
    assert len({c.name for c in out}) == len(out)
    return out


def all_cases() -> List[Case]:
    return [c for geo in GEOS for c in cases(geo)]


def prefixes(c: Case) -> List[List[int]]:
    return CC.prefixes(c.base)


def ban_mask(c: Case):
    """(V,) bool or None: a fixed quarter of the word tokens, the case's prefix tokens left out"""
    import torch
    if not c.ban:
        return None
    v = D.geometry(c.geo).v
    ids = torch.arange(v)
    mask = (ids >= D.N_SPECIALS_AND_TASKS) & ((ids * 7 + c.seed) % 4 == 0)
    for p in prefixes(c):
        for t in p:
            mask[t] = False
    return mask


def requirements(c: Case) -> List[List[List[int]]]:
    """Clip i's gs[i] groups: distinct word tokens (the task tokens are the vocabulary's last seven) that are neither banned nor
    in the clip's prefix, from the case's seed; the modes ``premet`` / ``allmet`` then put prefix tokens into the groups."""
    import torch
    v = D.geometry(c.geo).v
    gen = torch.Generator().manual_seed(9000 + c.seed)
    ban, pre = ban_mask(c), prefixes(c)
    small = v - D.N_SPECIALS_AND_TASKS < 64
    out = []
    for i, g_n in enumerate(c.gs):
        perm = (torch.randperm(v - D.N_SPECIALS_AND_TASKS, generator=gen) + 4).tolist()      # the words: behind the four specials
        pool = [t for t in perm if t not in pre[i] and (ban is None or not bool(ban[t]))]
        groups = []
        for g in range(g_n):
            size = 4 if c.mode == "full32" and g_n == 8 else 1 if c.mode == "short" else (1, 2)[(i + g) % 2] if small else (1, 2, 3)[(i + g) % 3]
            groups.append([pool.pop() for _ in range(size)])
        if c.mode == "premet" and i == 0 and g_n > 0:
            groups[0][0] = pre[0][0]
        if c.mode == "allmet" and i == 0:
            assert 0 < g_n <= len(pre[i])
            for g in range(g_n):
                groups[g][0] = pre[i][g]
        out.append(groups)
    return out


def tables(c: Case):
    """(req_tokens, req_groups) (B, width) int32 tensors: the clips' entries in shuffled order, two -1 gaps where 32 leave room"""
    import torch
    from conette_amd import required_search as RS
    req = requirements(c)
    need = max(sum(len(g) for g in r) for r in req)
    width = min(need + 2, RS.MAX_REQ_TOKENS)
    gen = torch.Generator().manual_seed(9500 + c.seed)
    order = [torch.randperm(width, generator=gen).tolist() for _ in req]
    rt, rg = RS.pack_tables(req, width, order)
    return torch.from_numpy(rt), torch.from_numpy(rg)


def inputs(c: Case):
    """constrain_cases.inputs: (frame_embs, audio_shape, bos, forbid or None, prefix table, prefix_lens).  The geometries' forbid
    mask holds the special tokens alone: a case with the mask on adds its required tokens, each of which may then occur once."""
    fe, shape, bos, forbid, table, lens = CC.inputs(c.base)
    if forbid is not None:
        forbid = forbid.clone()
        for r in requirements(c):
            for g in r:
                forbid[g] = True
    return fe, shape, bos, forbid, table, lens


_FNS: Dict[Case, object] = {}
_RUNS: Dict[Tuple[Case, bool], dict] = {}


def _logits_fn(c: Case):
    if c not in _FNS:
        fe, shape = inputs(c)[:2]
        _FNS[c] = GC.oracle_logits_fn(c.geo, fe, shape, rowwise=True)
    return _FNS[c]


def oracle_run(c: Case, required: bool = True) -> dict:
    """The restatement's search of the case on the oracle's logits (cached).  ``required`` False: the constrained search of the
    same inputs."""
    from conette_amd import required_search as RS
    key = (c, required)
    if key not in _RUNS:
        _, _, bos, forbid = inputs(c)[:4]
        fb = None if forbid is None else forbid.numpy()
        ban = ban_mask(c)
        _RUNS[key] = RS.required_search(_logits_fn(c), bos.tolist(), c.w, c.min_pred, c.max_pred, D.geometry(c.geo).v, EOS, PAD, fb,
                                        prefixes(c), None if ban is None else ban.numpy(), c.n, requirements(c) if required else None)
    return _RUNS[key]


def drop_runs(c: Optional[Case] = None) -> None:
    if c is None:
        _FNS.clear()
        _RUNS.clear()
    else:
        _FNS.pop(c, None)
        for k in [k for k in _RUNS if k[0] == c]:
            _RUNS.pop(k)
    CC.drop_runs()


def facts(c: Case) -> Dict[str, float]:
    """margin: smallest effective margin of the free calls; differs: free calls whose picks differ from the picks of their state
    without requirements; m5: calls with a row under M5; void: void slots; calls"""
    res = oracle_run(c)
    free = [k for k in res["calls"] if not k["forced"]]
    import numpy as np
    return {"margin": min(k["margin"] for k in free),
            "differs": sum(1 for k in free if list(zip(k["parents"], k["tokens"])) != k["plain"]),
            "m5": sum(1 for k in res["calls"] if k["m5_rows"] > 0),
            "m5_fan": sum(1 for k in free if k["m5_rows"] > 0 and k["step"] == c.plens[k["clip"]]),
            "void": int(np.isneginf(res["mult_lprobs"]).sum()), "calls": len(res["calls"])}


def meets_conditions(c: Case) -> bool:
    f = facts(c)
    return f["margin"] >= D.MIN_MARGIN and f["differs"] >= 1
