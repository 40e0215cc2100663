"""CPU: the launch rules that tests/decoder_geometry.py mirrors equal the ones in the kernel sources, its table of decoder
geometries reaches every search-step instantiation, FFN regime, row tail and memory-length tail, and every search of the table is
decided by margins that no rounding of the exact precisions can flip (so the GPU comparison may skip no call).  A retuned
threshold fails here until the table (and the cases that reach its edges) is revisited."""
import os
import re

import pytest

from tests import decoder_geometry as D

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "conette-audio-captioning_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _ints(pattern, text):
    found = {int(v) for v in re.findall(pattern, text)}
    assert found, pattern
    return found


def _one(pattern, text):
    found = _ints(pattern, text)
    assert len(found) == 1, (pattern, found)
    return found.pop()


def test_search_dispatch_matches_the_sources():
    dec, srch = _src("decoder.hip"), _src("dec_search.h")
    assert _one(r"#define S3_T (\d+)", srch) == D.S3_T
    assert _one(r"#define S3_VPT (\d+)", srch) == D.S3_VPT
    assert _one(r"#define CN_MAX_BEAM (\d+)", srch) == D.CN_MAX_BEAM
    assert _one(r"#define CN_MAX_PRED (\d+)", srch) == D.CN_MAX_PRED
    assert _one(r"if \(V <= S3_T \* S3_VPT && beam <= (\d+)\) \{", dec) == D.S3_MAX_BEAM
    body = dec[dec.index("const int vpt = cn_cdiv(V, S3_T);"):dec.index("#undef S3_LAUNCH")]
    assert re.sub(r"\s+", " ", body).strip() == (
        "const int vpt = cn_cdiv(V, S3_T); if (beam <= 4) { if (vpt <= 2) S3_LAUNCH(4, 2); else if (vpt <= 4) S3_LAUNCH(4, 4); "
        "else if (vpt <= 6) S3_LAUNCH(4, 6); else S3_LAUNCH(4, 8); } else { if (vpt <= 4) S3_LAUNCH(8, 4); else S3_LAUNCH(8, 8); }")
    assert {(int(a), int(b)) for a, b in re.findall(r"S3_LAUNCH\((\d+), (\d+)\);", body)} == set(D.S3_KERNELS)
    assert "beam < 1 || beam > CN_MAX_BEAM || max_pred < 1 || max_pred > CN_MAX_PRED || min_pred < 0" in dec
    # the rule at the ends of every instantiation's range
    for nr, beams in ((4, (1, 4)), (8, (5, 8))):
        for beam in beams:
            want = {2: (1, 2048), 4: (2049, 4096), 6: (4097, 6144), 8: (6145, 8192)} if nr == 4 else {4: (1, 4096), 8: (4097, 8192)}
            for vpt, (lo, hi) in want.items():
                assert D.search_kernel(max(lo, 4), beam) == D.search_kernel(hi, beam) == ("s3", nr, vpt)
    assert D.search_kernel(8193, 1) == D.search_kernel(31, 9) == D.search_kernel(8192, 16) == ("generic",)


def test_ffn_dispatch_matches_the_sources():
    dec, api = _src("decoder.hip"), _src("api.hip")
    assert _one(r"#define FF2_SPLITS (\d+)", dec) == D.FF2_SPLITS
    assert _one(r"static int ff2_splits_default\(\) \{ return (\d+); \}", dec) == D.ff2_splits_default()
    # which geometries get the packed stream of the fused FFN kernel (16-bit and exact: two sites)
    assert re.findall(r"dff % (\d+) == 0 && dff <= (\d+)\)", api) == [(str(D.FFN_SLAB), str(D.FUSED_FFN_MAX))] * 2
    assert "cfg->d_ff % 32 != 0 || cfg->vocab_size < 4" in api
    assert "cfg->n_layers < 1 || cfg->n_layers > CN_MAX_LAYERS || cfg->d_model != 256 || cfg->nhead != 8" in api
    # the fused path and its slab count
    assert dec.count("ctx->layers[0].ffn_w != nullptr && dff / 256 <= FF2_SPLITS") == 2
    assert "const bool block_path = kBlockT && !ctx->dec_unfused && ctx->layers[0].blk_w != nullptr &&" in dec
    assert "if (ffn_fused) splits = dff / 256;" in dec
    assert "if (splits < 1 || splits > FF2_SPLITS || splits > 8 || dff % (splits * 64) != 0) splits = 1;" in dec
    assert "dim3(dff / 256, cn_cdiv(R, DF_ROWS))" in dec
    # split-K of the per-sub-layer FFN2: 16-bit and exact
    assert "const int splits = (dff % (FF2_SPLITS * 64) == 0) ? FF2_SPLITS : 1;" in dec
    assert "const int splits = (dff % (FF2_SPLITS * 32) == 0) ? FF2_SPLITS : 1;" in dec
    # the slabs reach the next layer's block prologue and the final LayerNorm
    assert "pro.slabs = w.slabs, pro.nslab = splits, pro.b2_prev = pw.ff2_b" in dec
    assert "w.slabs, splits, slab, lw.ff2_b, w.x," in dec
    assert _one(r"w\.slabs = \(float\*\)take\(\(size_t\)FF2_SPLITS \* R \* d \* (\d+)\);", dec) == 4
    # the arena of the exact precision is sized from d_ff and the layer count
    assert "(size_t)cfg->n_layers * ((size_t)12 * 131072 + (size_t)(cfg->d_ff / 256 + 1) * 4 * 131072 + 4096)" in api
    g2 = _src("gemm2.h")
    assert "const bool k64 = (K % 64 == 0);" in g2
    assert "if (!k64) return cn_launch_gemm2_t<64, 64, 32, 2," in g2 and "return cn_launch_gemm2_t<64, 64, 64, 2, Epi, 2, 2, OPK>" in g2
    assert "if (!k64) return cn_launch_gemm2_t<128, 128, 32, 2," in g2
    assert D.k_tile(96) == D.k_tile(2080) == 32 and D.k_tile(256) == D.k_tile(4096) == 64
    # the rules at the values of the table
    want = {32: ("block+gemm2/1", "sublayer_h16/1", "sublayer_sp/1"), 96: ("block+gemm2/1", "sublayer_h16/1", "sublayer_sp/1"),
            256: ("fused/1", "sublayer_h16/1", "fused/1"), 1024: ("fused/4", "sublayer_h16/8", "fused/4"),
            1792: ("fused/7", "sublayer_h16/1", "fused/7"), 2048: ("fused/8", "sublayer_h16/8", "fused/8"),
            2080: ("block+gemm2/1", "sublayer_h16/1", "sublayer_sp/1"), 2304: ("block+gemm2/4", "sublayer_h16/1", "sublayer_sp/8"),
            4096: ("block+gemm2/4", "sublayer_h16/8", "sublayer_sp/8")}
    for d_ff, (h16, h16_unfused, exact) in want.items():
        for p in D.H16:
            assert D.ffn_regime(p, d_ff) == h16 and D.ffn_regime(p, d_ff, fusion=False) == h16_unfused, (p, d_ff)
        assert D.ffn_regime("exact", d_ff) == exact, d_ff
        assert D.ffn_regime("exact", d_ff, fusion=False) == "sublayer_sp/%d" % (8 if d_ff % 256 == 0 else 1), d_ff
        assert D.ffn_regime("fp32", d_ff) == D.ffn_regime("fp32", d_ff, fusion=False) == "fp32"


def test_row_and_key_tiles_match_the_sources():
    blk, ffn, ctx, dec, rows = _src("dec_block.h"), _src("dec_ffn.h"), _src("ctx.h"), _src("decoder.hip"), _src("dec_rows.h")
    for name in ("DB_ROWS", "DB_ROWS_SP", "DB_WIDE_ROWS", "DB_WIDE_ROWS_SP", "DB_WIDE_R", "DB_NB_SELF", "DB_DEPTH_SELF", "DB_NB_CROSS",
                 "DB_DEPTH_CROSS"):
        assert _one(r"#define %s (\d+)\b" % name, blk) == getattr(D, name), name
    assert _one(r"#define DF_ROWS (\d+)", ffn) == D.DF_ROWS
    assert _one(r"#define CN_MAX_LAYERS (\d+)", ctx) == D.CN_MAX_LAYERS
    assert _ints(r"constexpr int NB = (\d+);", rows) == {D.ATTN_NB}
    assert "if (kWide != DbOp<T>::ROWS && R >= DB_WIDE_R)" in dec
    assert "constexpr int kWide = CnIsH16<T>::value ? DB_WIDE_ROWS : DB_WIDE_ROWS_SP;" in dec
    for p in D.PRECISIONS:
        assert D.block_rows(p, D.DB_WIDE_R - 1) == 4 and D.block_rows(p, D.DB_WIDE_R) == 8


def test_vocabulary_of_the_synthetic_checkpoint():
    from conette_amd import synth
    assert len(synth.SPECIAL_TOKENS) + len(synth.TASK_NAMES) == D.N_SPECIALS_AND_TASKS
    assert D.vocab(20) == 31 and D.vocab(8182) == 8193


def test_table_reaches_every_regime():
    cov = D.coverage()
    names = [g.name for g in D.GEOMETRIES] + [(g.name, s.name) for g in D.GEOMETRIES for s in g.searches]
    assert len(set(names)) == len(names)
    assert set(D.CLEAN_CLIPS) == {(g.name, s.name) for g in D.GEOMETRIES for s in g.searches}
    # search kernels: every s3 instantiation at both ends of its V range, at a beam in 1..4 and one in 5..8 where that matters
    assert cov["search"] == {("s3", nr, vpt) for nr, vpt in D.S3_KERNELS} | {("generic",)}
    vb = cov["search_v_beam"]
    for v in (2048, 2049, 4096, 4097, 6144, 6145, 8192):
        lo = {k for (vv, beam, k) in vb if vv == v and beam <= 4}
        hi = {k for (vv, beam, k) in vb if vv == v and 5 <= beam <= 8}
        assert lo == {D.search_kernel(v, 1)} and hi == {D.search_kernel(v, 8)}, (v, lo, hi)
    for v, (lo_hi) in ((2048, ((4, 2), (8, 4))), (2049, ((4, 4), (8, 4))), (4096, ((4, 4), (8, 4))), (4097, ((4, 6), (8, 8))),
                       (6144, ((4, 6), (8, 8))), (6145, ((4, 8), (8, 8))), (8192, ((4, 8), (8, 8)))):
        assert D.search_kernel(v, 4) == ("s3",) + lo_hi[0] and D.search_kernel(v, 5) == ("s3",) + lo_hi[1]
    assert {k for (v, beam, k) in vb if v == 31 and beam <= 4} == {("s3", 4, 2)}
    assert {k for (v, beam, k) in vb if v == 31 and 5 <= beam <= 8} == {("s3", 8, 4)}
    assert any(v == 8193 and beam <= 8 for (v, beam, k) in vb)                      # generic because of V alone
    assert any(beam == 9 and v <= 8192 for (v, beam, k) in vb)                      # generic because of the beam alone: its boundary
    assert (31, D.CN_MAX_BEAM, ("generic",)) in vb
    assert {1, 4, 5, 8, 9, D.CN_MAX_BEAM} <= cov["beam"]
    # FFN widths and regimes
    assert cov["d_ff"] == {32, 96, 256, 1024, 1792, 2048, 2080, 2304, 4096}
    assert cov["k_tile"] == {32, 64}
    for p in D.H16:
        assert {r for (pp, r) in cov["ffn"] if pp == p} == {"fused/1", "fused/4", "fused/7", "fused/8", "block+gemm2/1", "block+gemm2/4",
                                                              "sublayer_h16/1", "sublayer_h16/8"}
    assert {r for (pp, r) in cov["ffn"] if pp == "exact"} == {"fused/1", "fused/4", "fused/7", "fused/8", "sublayer_sp/1", "sublayer_sp/8"}
    assert {r for (pp, r) in cov["ffn"] if pp == "fp32"} == {"fp32"}
    # every value the rule can take at all (d_ff = 32 .. 4096 in steps of 32) is reached, bar the fused slab counts 2, 3, 5, 6
    for p in D.PRECISIONS:
        every = {D.ffn_regime(p, d_ff, fu) for d_ff in range(32, 4097, 32) for fu in (True, False)}
        assert every - {r for (pp, r) in cov["ffn"] if pp == p} <= {"fused/2", "fused/3", "fused/5", "fused/6"}, p
    over = [g for g in D.GEOMETRIES if g.d_ff > D.FUSED_FFN_MAX]
    assert any(g.d_ff % 256 == 0 for g in over) and any(g.d_ff % 256 != 0 for g in over)
    assert cov["layers"] == {1, 2, 6, D.CN_MAX_LAYERS}
    assert {g.name for g in D.GEOMETRIES if g.n_layers > 6 or g.d_ff >= 4096} == set(D.MEASURED_BOUND_GEOMETRIES)
    # rows R = B x beam: every residue of the 4-row blocks, one row, and both sides of the 32-row FFN tiles' edges
    assert cov["rows_mod4"] == {0, 1, 2, 3}
    assert {1, 32, 33, 35, 63, 64, 65} <= cov["rows"]
    assert all(D.block_rows(p, r) == 4 for p in D.PRECISIONS for r in cov["rows"])
    # memory lengths against the 8-key batches kept two in flight
    assert {1, 7, 8, 9, 16, 17, 25} <= cov["mem_len"]
    assert {1, D.DB_NB_CROSS - 1, D.DB_NB_CROSS, D.DB_NB_CROSS + 1, D.DB_NB_CROSS * D.DB_DEPTH_CROSS,
            D.DB_NB_CROSS * D.DB_DEPTH_CROSS + 1, 3 * D.DB_NB_CROSS + 1} <= cov["mem_len"]
    searches = [s for g in D.GEOMETRIES for s in g.searches]
    assert any(max(s.frame_lens) < s.ta for s in searches) and any(max(s.frame_lens) == s.ta for s in searches)
    # search parameters
    assert sum(s.max_pred == D.CN_MAX_PRED for s in searches) == 1
    assert any(s.min_pred == 0 for s in searches) and any(s.min_pred > 3 for s in searches)
    assert any(s.min_pred >= s.max_pred for s in searches)                          # nothing finishes before the last step
    forc = [g.forcing for g in D.GEOMETRIES]
    assert any(f.cap_len == D.CN_MAX_PRED and any(1 < n < f.cap_len for n in f.n_valid) for f in forc)
    assert any(f.cap_len == 1 for f in forc)
    # sizes
    for g in D.GEOMETRIES:
        for s in g.searches:
            assert 1 <= s.b <= 9 and s.ta <= 32 and (s.max_pred <= 20 or s.max_pred == D.CN_MAX_PRED), (g.name, s.name)
            assert len(s.frame_lens) == s.b and all(1 <= n <= s.ta for n in s.frame_lens)
        assert g.forcing.b <= 9 and g.forcing.ta <= 32


_TRACES = {}


def _oracle(g, s):
    import torch
    if (g.name, s.name) not in _TRACES:
        torch.set_num_threads(min(8, os.cpu_count() or 1))
        _TRACES[(g.name, s.name)] = D.oracle_search(g, s)["calls"]
    return _TRACES[(g.name, s.name)]


@pytest.mark.parametrize("gname", [g.name for g in D.GEOMETRIES])
def test_every_search_is_decided_by_clear_margins(gname):
    """A condition on the INPUTS: the smallest effective margin of every search is at least MIN_MARGIN (four times the 5e-4 tie
    tolerance the exact precisions are held to elsewhere), so the GPU comparison needs no near-tie allowance; and every search
    has clips whose every call clears 0.25 x R16[f16], which the f16 precision must therefore decode like the oracle."""
    g = D.geometry(gname)
    for s in g.searches:
        calls = _oracle(g, s)
        eff = [D.effective_margin(c) for c in calls]
        clean = D.clean_clips(calls, s.b)
        print(f"{g.name}/{s.name}: {len(calls)} calls, smallest effective margin {min(eff):.5f}, clean clips {clean}")
        assert min(eff) >= D.MIN_MARGIN, (g.name, s.name, min(eff))
        assert len(clean) == D.CLEAN_CLIPS[(g.name, s.name)] >= 1, (g.name, s.name, clean)
        assert {c[1] for c in calls} == set(range(s.b))
    D.drop_weights(g)


def test_searches_shrink_and_run_to_the_end():
    """The finishing patterns the table promises: a search whose hypotheses end at several different steps until one row is left,
    one in which nothing ends before the last step, and the CN_MAX_PRED search really reaches step 63."""
    def ks(g, s):
        per = {}
        for step, clip, par, *_ in _oracle(g, s):
            per.setdefault(clip, []).append((step, len(par)))
        return per
    shrink = never = False
    for g in D.GEOMETRIES:
        for s in g.searches:
            per = ks(g, s)
            shrink |= any(v[-1][1] == 1 and len({k for _, k in v}) >= 3 for v in per.values() if s.beam >= 3)
            if s.min_pred >= s.max_pred:
                assert all(k == s.beam for v in per.values() for _, k in v) and all(v[-1][0] == s.max_pred - 1 for v in per.values())
                never = True
            if s.max_pred == D.CN_MAX_PRED:
                assert max(v[-1][0] for v in per.values()) == D.CN_MAX_PRED - 1
    assert shrink and never
    D.drop_weights()
