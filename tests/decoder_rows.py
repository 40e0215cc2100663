"""The GEMM dispatch of the decoder above 4096 and 8192 rows, mirrored from the sources, and the table of one-pass and step-path
cases that crosses both thresholds.

tests/test_cpu_decoder_rows.py holds the rules here to the C++ text (a retuned threshold fails there until this table is
revisited) and asserts what ``coverage()`` reaches; tests/test_gpu_decoder_rows.py runs the cases against the CPU oracles.

Sources mirrored (paths under conette-audio-captioning_amd/csrc):
  * gemm2.h ``cn_gemm2`` (16-bit), ``cn_gemm2_sp`` (exact); gemm.h ``cn_gemm`` (fp32): 64-row tiles below 4096 rows, 128-row
    tiles from 4096, and for the 16-bit operands from 8192 rows with N % 256 == 0 and no split-K the 256 x 256, 224 x 256 or
    three-deep 224 x 192 tiles, by the device's compute-unit count.
  * decoder.hip ``dec_prepare``, ``dec_sublayer_layer``, ``dec_step_forward``, ``forcing_prefill_impl``: the products each
    of them hands to that dispatch, with their (N, K, epilogue, splits).

Geometries, weights, frames and captions are those of tests/decoder_geometry.py; nothing synthetic is added here.
No torch at import time."""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Tuple

from tests import decoder_geometry as D

BIG_ROWS = 4096                  # gemm2.h / gemm.h: M >= 4096 in all three dispatchers
WIDE_ROWS = 8192                 # gemm2.h cn_gemm2: N % 256 == 0 && M >= 8192 && splits == 1
CVT_GRID_CAP = 4096              # decoder.hip dec_prepare: blocks of cn_cvt_kernel, 1024 elements each per trip
CVT_BLOCK_ELEMS = 1024
CN_FEAT = 768
D_MODEL = D.D_MODEL
DEFAULT_CUS = 256                # gemm2.h cn_g2_cus(): the count assumed when the device does not tell


def _cdiv(a: int, b: int) -> int:
    return -(-a // b)


def gemm_tile(prec: str, m: int, n: int, k: int, splits: int = 1, n_cu: int = DEFAULT_CUS) -> Tuple[int, int, int, int]:
    """(BM, BN, BK, NST) of the launch cn_gemm2 (bf16 / f16), cn_gemm2_sp (exact) or cn_gemm (fp32) makes for an M x N x K product."""
    assert k % 32 == 0 and m > 0 and n > 0 and splits >= 1
    n96 = n % 96 == 0 and n % 128 != 0
    if prec in D.H16:
        k64 = k % 64 == 0
        assert splits == 1 or (k // splits) % 64 == 0
        if m >= BIG_ROWS:
            if not k64:
                return (128, 128, 32, 2)
            if n96:
                return (128, 96, 64, 2)
            if n % 256 == 0 and m >= WIDE_ROWS and splits == 1:
                nt = n // 256
                r256, r224 = _cdiv(_cdiv(m, 256) * nt, n_cu), _cdiv(_cdiv(m, 224) * nt, n_cu)
                if r256 == 1 and n % 192 == 0 and _cdiv(m, 224) * (n // 192) <= n_cu:
                    return (224, 192, 64, 3)
                if r256 > 1 and r224 * 224 < r256 * 256:
                    return (224, 256, 64, 2)
                return (256, 256, 64, 2)
            return (128, 128, 64, 2)
        return (64, 64, 64 if k64 else 32, 2)
    if prec == "exact":          # (K elements of 4 bytes: BK = 64 bf16-sized columns = 32 elements)
        assert (k // splits) % 32 == 0
        if m >= BIG_ROWS:
            return (128, 96 if n96 else 128, 64, 2)
        return (64, 64, 64, 2)
    assert prec == "fp32" and splits == 1
    return (128 if m >= BIG_ROWS else 64, 96 if n96 else 128, 32, 2)


def cvt_trips(frames: int) -> int:
    """Trips of cn_cvt_kernel's grid-stride loop over the frames of dec_prepare (1 until the grid cap binds)."""
    return _cdiv(_cdiv(frames * CN_FEAT, CVT_BLOCK_ELEMS), CVT_GRID_CAP)


# ---- the call sites ---------------------------------------------------------------------------------------------------------------
class Product(NamedTuple):
    site: str                    # "<function>/<product>"
    m: int
    n: int
    k: int
    epi: str                     # epilogue class; T = the operand type of the precision
    splits: int
    ldo: int                     # leading dimension of the output (an odd one sends the epilogue's commit down its scalar branch)


def prepare_products(g: D.Geometry, frames: int) -> List[Product]:
    """dec_prepare over ``frames`` = B * Ta (or n_rec * t_rec) rows."""
    kv_ld = g.n_layers * 2 * D_MODEL
    return [Product("dec_prepare/proj", frames, D_MODEL, CN_FEAT, "BiasAct<T,RELU>", 1, D_MODEL),
            Product("dec_prepare/cross_kv", frames, kv_ld, D_MODEL, "BiasAct<T,NONE>", 1, kv_ld)]


def sublayer_products(g: D.Geometry, prec: str, rows: int, ffn2_split: bool) -> List[Product]:
    """dec_sublayer_layer (the same for every layer)."""
    d, dff = D_MODEL, g.d_ff
    out = [Product("dec_sublayer_layer/qkv", rows, 3 * d, d, "BiasAct<f32,NONE>", 1, 3 * d),
           Product("dec_sublayer_layer/sa_out", rows, d, d, "Resid", 1, d),
           Product("dec_sublayer_layer/ca_q", rows, d, d, "BiasAct<f32,NONE>", 1, d),
           Product("dec_sublayer_layer/ca_out", rows, d, d, "Resid", 1, d),
           Product("dec_sublayer_layer/ffn1", rows, dff, d, "BiasAct<T,GELU>", 1, dff)]
    if ffn2_split and prec in D.H16:
        out.append(Product("dec_sublayer_layer/ffn2", rows, d, dff, "Slab", D.FF2_SPLITS if dff % (D.FF2_SPLITS * 64) == 0 else 1, d))
    elif ffn2_split and prec == "exact":
        out.append(Product("dec_sublayer_layer/ffn2", rows, d, dff, "Slab", D.FF2_SPLITS if dff % (D.FF2_SPLITS * 32) == 0 else 1, d))
    else:
        out.append(Product("dec_sublayer_layer/ffn2", rows, d, dff, "Resid", 1, d))
    return out


def step_products(g: D.Geometry, prec: str, rows: int, fusion: bool) -> List[Product]:
    """dec_step_forward at R = B x beam rows: the GEMMs of one step (the block and fused-FFN kernels are no cn_mm products)."""
    d, dff = D_MODEL, g.d_ff
    ldv = (g.v + 7) // 8 * 8
    regime = D.ffn_regime(prec, dff, fusion)
    cls = Product("dec_step_forward/classifier", rows, g.v, d, "BiasAct<f32,NONE>", 1, ldv)
    if regime.startswith("fused/"):
        return [cls]
    if regime.startswith("block+gemm2/"):
        splits = int(regime.split("/")[1])
        return [Product("dec_step_forward/ffn1", rows, dff, d, "BiasAct<T,GELU_FAST>", 1, dff),
                Product("dec_step_forward/ffn2", rows, d, dff, "Slab", splits, d), cls]
    return sublayer_products(g, prec, rows, ffn2_split=prec != "fp32") + [cls]


def forcing_products(g: D.Geometry, prec: str, frames: int, rows: int, classifier: bool = True) -> List[Product]:
    """forcing_prefill_impl: dec_prepare, the sub-layer loop with FFN2 as one GEMM, the classifier written with ldo = V
    (conette_score and conette_align without targets run no classifier GEMM)."""
    out = prepare_products(g, frames) + sublayer_products(g, prec, rows, ffn2_split=False)
    if classifier:
        out.append(Product("forcing_prefill_impl/classifier", rows, g.v, D_MODEL, "BiasAct<f32,NONE>", 1, g.v))
    return out


# ---- the case table ---------------------------------------------------------------------------------------------------------------
def _ragged(b: int, top: int, step: int) -> Tuple[int, ...]:
    """b lengths in 1..top: full at every third clip and at the last two (the last row tile holds real rows), ragged between."""
    return tuple(top if (i % 3 == 0 or i >= b - 2) else 1 + (i * step) % top for i in range(b))


def _forcing(name: str, b: int, ta: int, cap_len: int, seed: int) -> D.Forcing:
    return D.Forcing(name, b, ta, _ragged(b, ta, 5), cap_len, _ragged(b, cap_len, 11), seed)


# One-pass cases, R = B x cap_len.  Ta = 17 keeps dec_prepare's B x Ta far below 4096 in the first two (1088 / 1411 frames);
# Ta = 64 takes it to 8192 / 8256 in the last two: the caption rows and the frame rows cross their thresholds separately.
ONEPASS_SHAPES = (
    ("r4096", 64, 17, 64),       # first 128-row launch, no row tail
    ("r4150", 83, 17, 50),       # row tail of 54
    ("r8192", 128, 64, 64),      # first launch of the 256-row regime
    ("r8256", 129, 64, 64),      # tails of 64 / 192 rows for 256- / 224-row tiles
)
ONEPASS_GEOMETRIES = ("v31_ff32_l2", "v2048_ff96_l1", "v2049_ff256_l6", "v4097_ff1792_l1", "v6145_ff2080_l2")


# 8288 = 37 x 224 rows and frames: the 224-row tiles without a row tail (QKV on 224 x 192, the classifier at N = 2048 on 224 x 256)
ONEPASS_EXTRA = {"v2048_ff96_l1": (("r8288", 148, 56, 56),)}


def onepass_cases(gname: str) -> Tuple[D.Forcing, ...]:
    gi = ONEPASS_GEOMETRIES.index(gname)
    shapes = ONEPASS_SHAPES + ONEPASS_EXTRA.get(gname, ())
    return tuple(_forcing(name, b, ta, cap, 100 + 10 * gi + i) for i, (name, b, ta, cap) in enumerate(shapes))


def onepass_case(gname: str, cname: str) -> D.Forcing:
    return next(f for f in onepass_cases(gname) if f.name == cname)


class Tiled(NamedTuple):
    """``copies`` copies of a search of decoder_geometry.GEOMETRIES in one batch.  Copy c holds the search's clips in the order
    rotated by c (position j holds clip (j + c) % b); the frames behind each clip's length are re-seeded per copy.  ``ta`` >=
    the search's pads the frame axis (more padding frames at PAD_FRAME_SCALE)."""
    gname: str
    sname: str
    copies: int
    ta: int

    @property
    def name(self) -> str:
        return "%s/%s/x%d/ta%d" % (self.gname, self.sname, self.copies, self.ta)

    @property
    def geometry(self) -> D.Geometry:
        return D.geometry(self.gname)

    @property
    def search(self) -> D.Search:
        return next(s for s in self.geometry.searches if s.name == self.sname)

    @property
    def b(self) -> int:
        return self.copies * self.search.b

    @property
    def rows(self) -> int:
        return self.b * self.search.beam

    @property
    def frames(self) -> int:
        return self.b * self.ta


def _T(gname, sname, copies, ta=None):
    s = next(s for s in D.geometry(gname).searches if s.name == sname)
    return Tiled(gname, sname, copies, s.ta if ta is None else ta)


# Step-path cases: R = B x beam just above 4096 and, for the two searches with max_pred 12 and at most two layers (the KV cache
# grows with R x max_pred x layers), above 8192.  No entry point refused a size; none is shrunk.
TILED = (
    _T("v31_ff32_l2", "beam8_r64", 65),              # R = 4160, row tail of 64; 8840 frames
    _T("v31_ff32_l2", "beam8_r64", 129),             # R = 8256; 17 544 frames
    _T("v2049_ff256_l6", "beam4_r2mod4", 342),       # R = 4104, row tail of 8; 16 416 frames at kv_ld = 3072
    _T("v6145_ff2080_l2", "beam4_r36", 114),         # R = 4104; 9234 frames
    _T("v8192_ff2304_l6", "beam8_r24", 171),         # R = 4104; 4617 frames
    _T("v2048_ff96_l1", "beam5_r35", 118),           # R = 4130; 7434 frames
    _T("v2048_ff96_l1", "beam5_r35", 236),           # R = 8260; 14 868 frames
    # the one search here with d_ff % 512 == 0: with fusion off the 16-bit FFN2 is split over 8 slabs (the others reach 4, or 8
    # in the exact precision only)
    _T("v4096_ff1024_l2", "beam8_r8", 513),          # R = 4104; 4617 frames
    # d_ff = 2304 at 8208 rows: FFN1 (nine 256-wide column tiles) is the one product that takes 224 x 256 tiles through the GELU
    # epilogues; max_pred = 6 keeps the six layers' KV cache at 0.6 GB
    _T("v8192_ff2304_l6", "beam8_r24", 342),         # R = 8208; 9234 frames
)
# dec_prepare alone above 8192 frames, the search itself far below 4096 rows: few copies, the frame axis padded
PREPARE_ONLY = (
    _T("v2049_ff256_l6", "beam4_r2mod4", 43, 64),    # R = 516, 129 x 64 = 8256 frames: tails of 64 / 192 rows
)
# Greedy searches over distinct clips, (geometry, clips, Ta, max_pred, seed).  The third is the one way to 256 x 256 tiles through
# the fast GELU of the FFN1 behind the block kernel: d_ff = 4096 is sixteen column tiles, which 224-row tiles serve in three
# rounds against two -- at exactly 8192 rows; one row more and both take three, and 224 x 256 wins.
GREEDY = (("v31_ff32_l2", 4160, 9, 4, 31), ("v2048_ff96_l1", 4100, 9, 4, 32), ("v8193_ff4096_l2", 8192, 3, 2, 33))


def tiled_index(t: Tiled):
    """(copies, b) int array: where clip i of the untiled search sits in copy c of the tiled batch."""
    import numpy as np
    b = t.search.b
    c, i = np.meshgrid(np.arange(t.copies), np.arange(b), indexing="ij")
    return c * b + (i - c) % b


def tiled_inputs(t: Tiled):
    """(frame_embs (B, ta, 768), audio_shape (B, 2), bos_ids (B,), forbid (V,)) of a tiled search."""
    import numpy as np
    import torch
    g, s = t.geometry, t.search
    fe0, shape0, bos0, forbid = D.search_inputs(g, s)
    idx = tiled_index(t)
    src = np.empty(t.b, dtype=np.int64)
    for c in range(t.copies):
        src[idx[c]] = np.arange(s.b)
    fe = torch.zeros((t.b, t.ta, CN_FEAT), dtype=torch.float32)
    fe[:, :s.ta] = fe0[src]
    rng = np.random.Generator(np.random.PCG64(99000 + s.seed))
    # (the values of decoder_geometry.frames behind a clip's length, drawn anew for every slot of the tiled batch)
    pad = torch.from_numpy((rng.random((t.b, t.ta, CN_FEAT), dtype=np.float32) * 2.0 - 1.0) * np.float32(0.65 * 3 ** 0.5 * D.PAD_FRAME_SCALE))
    lens = shape0[src, 1]
    behind = torch.arange(t.ta)[None, :] >= lens[:, None]
    fe[behind] = pad[behind]
    return fe, shape0[src].clone(), bos0[src].clone(), forbid


# ---- what a set of cases reaches --------------------------------------------------------------------------------------------------
class Reach(NamedTuple):
    site: str
    prec: str                    # "h16", "exact" or "fp32": the dispatcher
    tile: Tuple[int, int, int, int]
    epi: str
    splits: int
    k: int
    row_tail: bool               # M % BM != 0
    col_tail: bool               # N % BN != 0
    odd_ldo: bool                # the output's leading dimension is odd


def _reach(products, prec, n_cu):
    disp = "h16" if prec in D.H16 else prec
    out = set()
    for p in products:
        tile = gemm_tile(prec, p.m, p.n, p.k, p.splits, n_cu)
        out.add(Reach(p.site, disp, tile, p.epi, p.splits, p.k, p.m % tile[0] != 0, p.n % tile[1] != 0, p.ldo % 2 == 1))
    return out


def case_reach(kind: str, gname: str, case, prec: str, n_cu: int = DEFAULT_CUS, fusion: bool = True) -> set:
    """kind "onepass" (a Forcing), "score" (the same without the classifier GEMM), "step" (a Tiled: dec_prepare + one step),
    "greedy" ((geometry, clips, Ta, max_pred, seed))."""
    g = D.geometry(gname)
    if kind in ("onepass", "score"):
        return _reach(forcing_products(g, prec, case.b * case.ta, case.b * case.cap_len, kind == "onepass"), prec, n_cu)
    if kind == "step":
        return _reach(prepare_products(g, case.frames) + step_products(g, prec, case.rows, fusion), prec, n_cu)
    assert kind == "greedy"
    return _reach(prepare_products(g, case[1] * case[2]) + step_products(g, prec, case[1], fusion), prec, n_cu)


def coverage(n_cu: int = DEFAULT_CUS, onepass=ONEPASS_GEOMETRIES, tiled=TILED + PREPARE_ONLY, greedy=GREEDY) -> set:
    """Every Reach of the case table as tests/test_gpu_decoder_rows.py runs it: the one-pass cases, the tiled searches with decode
    fusion on and off, the greedy searches, in the four precisions."""
    cov = set()
    for prec in D.PRECISIONS:
        for gname in onepass:
            for f in onepass_cases(gname):
                cov |= case_reach("onepass", gname, f, prec, n_cu)
        for fusion in (True, False):
            for t in tiled:
                cov |= case_reach("step", t.gname, t, prec, n_cu, fusion)
        for c in greedy:                                        # (the greedy searches run with the default setting only)
            cov |= case_reach("greedy", c[0], c, prec, n_cu, True)
    return cov


def describe(reach: set) -> List[str]:
    return ["%-32s %-5s %3d x %3d x %2d, %d stages  %-20s splits %d  K %4d%s%s%s" % (
        r.site, r.prec, r.tile[0], r.tile[1], r.tile[2], r.tile[3], r.epi, r.splits, r.k, "  row tail" if r.row_tail else "",
        "  column tail" if r.col_tail else "", "  odd ldo" if r.odd_ldo else "") for r in sorted(reach)]


# ---- the comparison rule of the one-pass logits -----------------------------------------------------------------------------------
def onepass_regions(rows: int, v: int, row_tiles) -> Dict[str, tuple]:
    """Named (row slice, column slice) regions on which the rule is applied again: for every row-tile height BM the case's
    products take, the rows of the last (partial, where rows % BM != 0) row tile and of the first; the classifier's tail columns
    (those beyond the last full 128; the last 128 where there is no tail)."""
    reg = {}
    for bm in sorted(set(row_tiles)):
        reg["last row tile of %d" % bm] = (slice((rows - 1) // bm * bm, rows), slice(None))
        reg["first row tile of %d" % bm] = (slice(0, min(bm, rows)), slice(None))
    c0 = v // 128 * 128
    reg["classifier tail columns"] = (slice(None), slice(c0 if c0 < v else max(v - 128, 0), v))
    return reg


def forcing_violations(prec: str, got, ref, ref32, valid, k: float, regions: Dict[str, tuple]):
    """The rule of tests/test_gpu_decoder_edges.py::test_forcing_logits_match_the_precisions_oracle on (R, V) arrays, over every
    non-pad row (``valid`` (R,) bool) and again on each region alone.  ``ref`` is the precision's own oracle (``ref32`` itself for
    fp32 / exact), ``k`` the precision's entry of that module's ROUNDING.  Returns (figures, violations): figures maps region ->
    (max, mean, dist); violations is a list of strings, empty when the rule holds everywhere."""
    import numpy as np
    assert got.shape == ref.shape == ref32.shape and valid.shape == (got.shape[0],)
    figures, bad = {}, []
    full = {"all": (slice(None), slice(None))}
    full.update(regions)
    dist = float(np.abs(ref[valid] - ref32[valid]).max())       # one distance, of the whole case, for every region
    for name, (rs, cs) in full.items():
        ok = valid[rs]
        g, r = got[rs, cs][ok], ref[rs, cs][ok]
        if g.size == 0:
            bad.append("%s: no valid position" % name)
            continue
        if not np.isfinite(g).all():
            bad.append("%s: not finite" % name)
            continue
        err = np.abs(g - r)
        e_max, e_mean = float(err.max()), float(err.mean())
        figures[name] = (e_max, e_mean, dist)
        if prec in ("fp32", "exact"):
            if not (err <= 2e-3 + 1e-3 * np.abs(r)).all():
                bad.append("%s: rtol 1e-3 / atol 2e-3 missed, max %.6f" % (name, e_max))
            continue
        if not e_max < dist:
            bad.append("%s: max %.5f not below the operand oracle's distance to fp32 %.5f" % (name, e_max, dist))
        if not (err <= 0.15 * min(1.0, 2 * k) + 3e-3 * k * np.abs(r)).all():
            bad.append("%s: rtol %.2g / atol %.3g missed, max %.5f" % (name, 3e-3 * k, 0.15 * min(1.0, 2 * k), e_max))
        if not e_mean < 0.03 * min(1.0, 2 * k):
            bad.append("%s: mean %.5f not below %.4f" % (name, e_mean, 0.03 * min(1.0, 2 * k)))
    return figures, bad


def onepass_oracle(g: D.Geometry, f: D.Forcing, kind: str, inputs=None):
    """(R, V) float32 logits of a one-pass case: kind "fp32" (oracle/cpu_ref.py) or "bf16" / "f16" (oracle/bf16_ref.py).
    ``inputs``: (frame_embs, audio_shape, caps_in) in place of the case's own (captions folded onto fewer clips)."""
    import numpy as np
    from oracle import bf16_ref as Bf
    from oracle import cpu_ref as O
    fe, shape, caps = D.forcing_inputs(g, f) if inputs is None else inputs
    if kind == "fp32":
        ref = O.teacher_forcing(D.weights(g), fe, shape, caps, n_layers=g.n_layers)
    else:
        with Bf.operands(kind):
            ref = Bf.teacher_forcing_bf16(D.weights(g), fe, shape, caps, n_layers=g.n_layers)
    return np.ascontiguousarray(ref.permute(0, 2, 1).reshape(caps.shape[0] * caps.shape[1], g.v).numpy())


# ---- the step path ----------------------------------------------------------------------------------------------------------------
def malformed(preds, lprobs, v: int, eos: int = 2, pad: int = 0) -> List[str]:
    """What is wrong with captions (..., L) int and their scores (...): ids outside [0, V), a pad in front of a token, a token
    behind <eos>, a score that is not a finite log-probability.  Empty when every caption is well-formed."""
    import numpy as np
    p, lp = np.asarray(preds).reshape(-1, np.asarray(preds).shape[-1]), np.asarray(lprobs).reshape(-1)
    bad = []
    if not ((p >= 0) & (p < v)).all():
        bad.append("id outside [0, V)")
    is_pad = p == pad
    if (is_pad[:, :-1] & ~is_pad[:, 1:]).any():
        bad.append("a pad in front of a token")
    if (p[:, 0] == pad).any():
        bad.append("an empty caption")
    after = (np.cumsum(p == eos, axis=1) - (p == eos)) > 0          # positions behind the first <eos>
    if (after & ~is_pad).any():
        bad.append("a token behind <eos>")
    if not (np.isfinite(lp).all() and (lp <= 0).all()):
        bad.append("a score that is no finite log-probability")
    return bad


def greedy_inputs(case):
    """(frame_embs, audio_shape, bos (B,), forbid (V,)) of a GREEDY entry: distinct seeded clips, ragged lengths, task (seed + i) % 7."""
    import torch
    gname, b, ta, _, seed = case
    g = D.geometry(gname)
    w = D.weights(g)
    fe, shape = D.frames(b, ta, _ragged(b, ta, 5), seed)
    tasks = torch.as_tensor([(seed + i) % 7 for i in range(b)])
    return fe, shape, w["model.task_id_to_token_id"][tasks], w["model.forbid_rep_mask"].bool()
