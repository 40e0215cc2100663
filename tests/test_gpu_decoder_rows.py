"""GPU: the decoder's GEMMs at 4096 and 8192 rows -- the 128-row tiles, the 128 x 96 and BK = 32 variants, split-K slabs on
128-row tiles, and from 8192 rows the 256 x 256, 224 x 256 and three-deep 224 x 192 tiles -- on the cases of tests/decoder_rows.py,
against the CPU oracles (oracle/cpu_ref.py; oracle/bf16_ref.py for the 16-bit operand precisions).
tests/test_cpu_decoder_rows.py holds the mirrored dispatch to the sources and proves what the table reaches at 256 compute units.

  a. one-pass forcing logits, every case x four precisions, by the rule of test_gpu_decoder_edges.py on every non-pad position and
     again on the first row tile, the last row tile and the classifier's tail columns alone
  b. Engine.score and Engine.align at 8256 rows
  c. the step path at R >= 4096 and >= 8192: tiled searches against the untiled oracle search, copy by copy, fusion on and off
  d. Engine.greedy's masked step logits over thousands of distinct clips
  e. dec_prepare alone above 8192 frames: a padded search of few rows, and Engine.decode_spans over long recordings

Every test prints the tile each call site took at the device's compute-unit count and names the tiles of the 256-unit list that a
device of another size does not reach.  Engines and weights live per geometry and are dropped when the tests move on."""
import gc
import os

import numpy as np
import pytest
import torch

from tests import decoder_geometry as D
from tests import decoder_rows as R
from tests.test_gpu_decoder_edges import ROUNDING

pytestmark = pytest.mark.gpu

EXACT = ("fp32", "exact")
R16 = D.R16


class _Geo:
    """One decoder geometry: its engines (lazily, per precision) and the oracle runs of the case at hand."""

    def __init__(self, g):
        self.g = g
        self.engines, self.cache, self.case = {}, {}, None
        self.side = torch.cuda.Stream()
        torch.set_num_threads(min(16, os.cpu_count() or 1))

    def engine(self, prec):
        if prec not in self.engines:
            from conette_amd.engine import Engine
            self.engines[prec] = Engine(D.weights(self.g), precision=prec, n_layers=self.g.n_layers, d_ff=self.g.d_ff)
        return self.engines[prec]

    def of_case(self, case, key, make):
        """results computed once per case and shared by the precisions (never modified); one case's are kept at a time"""
        if self.case != case:
            self.cache.clear()
            self.case = case
        if key not in self.cache:
            self.cache[key] = make()
        return self.cache[key]


_GEO = []


def _geo(gname):
    if _GEO and _GEO[0].g.name != gname:
        _drop()
    if not _GEO:
        _GEO.append(_Geo(D.geometry(gname)))
    return _GEO[0]


def _drop():
    for h in _GEO:
        h.engines.clear()
        h.cache.clear()
        D.drop_weights(h.g)
    _GEO.clear()
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _drop()


def _n_cu():
    return int(torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count)


def _report(kind, gname, case, prec, fusion=True):
    """prints the tile of every call site at this device's compute-unit count; returns that reach"""
    n_cu = _n_cu()
    here = R.case_reach(kind, gname, case, prec, n_cu, fusion)
    print(f"tiles at {n_cu} compute units, {kind} {gname} {getattr(case, 'name', case)} {prec} fusion {fusion}:")
    print("\n".join("  " + line for line in R.describe(here)))
    if n_cu != R.DEFAULT_CUS:
        missed = {r.tile for r in R.case_reach(kind, gname, case, prec, R.DEFAULT_CUS, fusion)} - {r.tile for r in here}
        if missed:
            print(f"  NOT REACHED on this device (reached at {R.DEFAULT_CUS} compute units): {sorted(missed)}")
    return here


# ---- a. one-pass forcing logits -------------------------------------------------------------------------------------------------
ONEPASS = [(gname, f.name, prec) for gname in R.ONEPASS_GEOMETRIES for f in R.onepass_cases(gname) for prec in D.PRECISIONS]


def _onepass(h, f):
    fe, shape, caps = h.of_case(("onepass", f.name), "inputs", lambda: D.forcing_inputs(h.g, f))
    return fe, shape, caps, (caps.numpy() != 0).reshape(-1)


def _oracle(h, f, kind):
    return h.of_case(("onepass", f.name), ("oracle", kind), lambda: R.onepass_oracle(h.g, f, kind))


@pytest.mark.parametrize("gname,cname,prec", ONEPASS)
def test_onepass_logits_match_the_precisions_oracle(gname, cname, prec):
    """Engine.forcing (one pass) at 4096 .. 8288 rows.  fp32 / exact against oracle/cpu_ref.py: rtol 1e-3, atol 2e-3.  bf16 / f16
    against oracle/bf16_ref.py at the same operand type: rtol 3e-3 k, atol 0.15 min(1, 2k), mean < 0.03 min(1, 2k), and closer to
    that oracle than it is to the fp32 one -- on every non-pad position, and again on the rows of the first and of the last row
    tile (of every tile height the case's products take) and on the classifier's tail columns, so that an error confined to a
    tail cannot hide in the mean of 8256 rows."""
    h = _geo(gname)
    g, f = h.g, R.onepass_case(gname, cname)
    here = _report("onepass", gname, f, prec)
    fe, shape, caps, valid = _onepass(h, f)
    rows = f.b * f.cap_len
    ref32 = _oracle(h, f, "fp32")
    ref = ref32 if prec in EXACT else _oracle(h, f, prec)
    got = h.engine(prec).forcing(fe.cuda(), shape[:, 1].int(), caps).reshape(rows, g.v).cpu().numpy()
    regions = R.onepass_regions(rows, g.v, {r.tile[0] for r in here if not r.site.startswith("dec_prepare")})
    figures, bad = R.forcing_violations(prec, got, ref, ref32, valid, ROUNDING.get(prec, 0.0), regions)
    for name, (e_max, e_mean, dist) in figures.items():
        print(f"onepass {(gname, cname, prec)} {name}: max {e_max:.5f} mean {e_mean:.6f}; operand oracle to fp32 oracle {dist:.5f}")
    assert bad == [], (gname, cname, prec, bad)


# ---- b. score and align at 8256 rows --------------------------------------------------------------------------------------------
SCORED = [(gname, prec) for gname in ("v2049_ff256_l6", "v2048_ff96_l1") for prec in D.PRECISIONS]


class _Bound:
    """what tests/test_gpu_score.py::logit_bound reads of its fixture"""

    def __init__(self, g):
        self.g = g


FOLD = 43                                                                  # 129 captions = 3 clips x 43


@pytest.mark.parametrize("cpa", (1, FOLD))
@pytest.mark.parametrize("gname,prec", SCORED)
def test_score_at_8256_rows(gname, prec, cpa):
    """Engine.score on the 129 x 64 case -- one caption per clip, and the same 129 captions folded onto the first 3 clips
    (caps_per_audio = 43) -- against float64 log-softmax + gather of the precision's oracle logits (for the folded call: the
    oracle run on the three clips' frames repeated per caption), within the bound tests/test_gpu_score.py derives from the forcing
    test's logit bound."""
    from tests.test_gpu_score import logit_bound, make_targets, ref_from_logits
    h = _geo(gname)
    g, f = h.g, R.onepass_case(gname, "r8256")
    _report("score", gname, f, prec)
    fe, shape, caps, _ = _onepass(h, f)
    targets = h.of_case(("onepass", f.name), "targets", lambda: make_targets(caps, g.v, f.seed))
    kind = "fp32" if prec in EXACT else prec
    if cpa == 1:
        logits = lambda: _oracle(h, f, kind)
    else:
        assert f.b == 3 * cpa
        fe, shape = fe[:3], shape[:3]
        logits = lambda: R.onepass_oracle(g, f, kind, (fe.repeat_interleave(cpa, dim=0), shape.repeat_interleave(cpa, dim=0), caps))
    ref_lp, zt, zmax = h.of_case(("onepass", f.name), ("score ref", kind, cpa), lambda: ref_from_logits(
        torch.from_numpy(logits()).reshape(f.b, f.cap_len, g.v).permute(0, 2, 1), targets))
    out = h.engine(prec).score(fe.cuda(), shape[:, 1].int(), caps, targets, caps_per_audio=cpa)
    torch.cuda.synchronize()
    tok, sums, cnt = out["tok_lprobs"].cpu(), out["sum_lprobs"].cpu(), out["n_tokens"].cpu()
    scored = targets != 0
    n = scored.sum(dim=1)
    assert cnt.tolist() == n.tolist() and int(n.sum()) > 0
    assert torch.isfinite(tok).all() and torch.isfinite(sums).all()
    bound = (logit_bound(_Bound(g), prec, zt.abs()) + logit_bound(_Bound(g), prec, zmax)) * scored
    err = (tok.double() - ref_lp).abs()
    has = n > 0
    mean_err = (sums.double() - ref_lp.sum(dim=1)).abs()[has] / n[has]
    print(f"score {(gname, f.name, prec, cpa)}: max |d lp| {float(err.max()):.3e} (bound there {float(bound.flatten()[err.argmax()]):.3e}) "
          f"max |d sum / n| {float(mean_err.max()):.3e}; last 64 rows max {float(err[-1].max()):.3e}")
    assert bool((err <= bound).all()), (gname, prec, float(err.max()))
    assert bool((mean_err <= (bound.sum(dim=1)[has] / n[has])).all()), (gname, prec, float(mean_err.max()))
    # (<=, not <: at V = 2048 the float64 oracle itself holds three targets of these 8256 rows at -7e-11, which is 0 in fp32)
    assert bool((tok[scored] <= 0).all())


@pytest.mark.parametrize("gname,prec", SCORED)
def test_align_at_8256_rows(gname, prec):
    """Engine.align's per-layer maps on the 129 x 64 case against the restatement of tests/test_cpu_alignment.py, by the rule of
    tests/test_gpu_align.py part 1: fp32 / exact within 2e-3; bf16 / f16 closer to the operand restatement than that is to the
    fp32 one, in the maximum and in the mean; both within twice ALIGN_MEASURED."""
    from tests.test_cpu_alignment import reference_maps
    from tests.test_gpu_align import ALIGN_MEASURED
    h = _geo(gname)
    g, f = h.g, R.onepass_case(gname, "r8256")
    _report("score", gname, f, prec)
    fe, shape, caps, _ = _onepass(h, f)

    def reference(kind):
        return h.of_case(("onepass", f.name), ("align ref", kind), lambda: torch.stack(reference_maps(g, kind, (fe, shape, caps))[1]).double())

    out = h.engine(prec).align(fe.cuda(), shape[:, 1].int(), caps, per_layer=True)
    torch.cuda.synchronize()
    got = out["attn_layers"].cpu().double()                                  # (NL, B, L, Ta)
    frames = torch.arange(f.ta)[None, None, :] < shape[:, 1][:, None, None]
    valid = (frames & (caps != 0)[:, :, None])[None].expand_as(got)
    assert bool(torch.isfinite(got).all()) and not bool(got[~valid].any())
    ref = reference("fp32" if prec in EXACT else prec)
    err = (got - ref).abs()[valid]
    e_max, e_mean = float(err.max()), float(err.mean())
    if prec in EXACT:
        cap_max, cap_mean = 2e-3, 2e-3
    else:
        dist = (ref - reference("fp32")).abs()[valid]
        cap_max, cap_mean = float(dist.max()), float(dist.mean())
    tail = float((got - ref).abs()[:, -1][valid[:, -1]].max())
    print(f"align {(gname, f.name, prec)}: max |d a| {e_max:.3e} mean {e_mean:.3e} (ceilings {cap_max:.3e} / {cap_mean:.3e}); last clip max {tail:.3e}")
    cap_max, cap_mean = min(cap_max, 2 * ALIGN_MEASURED[prec][0]), min(cap_mean, 2 * ALIGN_MEASURED[prec][1])
    assert e_max <= cap_max and e_mean <= cap_mean, (gname, prec, e_max, cap_max, e_mean, cap_mean)


# ---- c. / e. the step path ------------------------------------------------------------------------------------------------------
def _decode(h, prec, t, fusion):
    fe, shape, bos, forbid = h.of_case(("tiled", t.name), "inputs", lambda: R.tiled_inputs(t))
    s = t.search
    eng = h.engine(prec)
    eng.set_decode_fusion(fusion)
    try:
        # on a side stream, as tests/test_gpu_decoder_edges.py decodes (the legacy default stream cannot be captured)
        h.side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(h.side):
            out = eng.decode(fe.cuda(), shape[:, 1].int(), bos, forbid, s.beam, s.min_pred, s.max_pred, want_trace=True)
        torch.cuda.synchronize()
    finally:
        eng.set_decode_fusion(True)
    return {k: v.cpu() for k, v in out.items()}


def _check_tiled(h, prec, t, out, tag):
    """Copy by copy against the oracle's run of the untiled search.  fp32 / exact: the rule of
    test_gpu_decoder_edges.py::test_search_matches_the_oracle.  bf16 / f16: every copy of every clean clip equals the oracle end
    to end (the clean-clip rule of test_sequential_search_16bit); the other clips' captions are well-formed."""
    g, s = h.g, t.search
    ref = h.of_case(("tiled", t.name), "oracle", lambda: D.oracle_search(g, s))
    idx = R.tiled_index(t)                                                    # (copies, b): slot of clip i in copy c
    sel, val = out["trace_sel"].numpy()[:, idx], out["trace_val"].numpy()[:, idx]   # (steps, copies, b, beam[, 2])
    ps_ref, bm_ref = ref["mult_preds"].shape[2], ref["best_preds"].shape[1]
    ps, bm = (int(x) for x in out["sizes"].tolist())
    mult, best = out["mult_preds"].numpy()[idx], out["best_preds"].numpy()[idx]
    mult_lp, best_lp = out["mult_lprobs"].numpy()[idx], out["best_lprobs"].numpy()[idx]
    assert np.isfinite(mult_lp).all() and np.isfinite(best_lp).all(), tag
    if prec in EXACT:
        clips, sum_atol, lp_atol = list(range(s.b)), 2e-4, 1e-4
        assert [ps, bm] == [ps_ref, bm_ref], tag
    else:
        tol = 0.25 * R16[prec]
        clips, sum_atol, lp_atol = D.clean_clips(ref["calls"], s.b, tol), 0.2 * R16[prec], 0.05 * R16[prec]
        if prec == "f16":
            assert len(clips) == D.CLEAN_CLIPS[(g.name, s.name)] >= 1, tag
        assert 1 <= ps <= s.max_pred and 1 <= bm <= s.max_pred, (tag, ps, bm)          # (a diverged clip's captions may be shorter or longer)
        assert R.malformed(mult[..., :ps], mult_lp, g.v) == [] and R.malformed(best[..., :bm], best_lp, g.v) == [], tag
        assert not mult[..., ps:].any() and not best[..., bm:].any(), tag
    # every call of a clip in ``clips`` must be the oracle's in every copy; a copy of another clip (16-bit only) is followed call by
    # call, as test_sequential_search_16bit follows it, until a call below the tolerance falls the other way
    diverged = np.zeros((t.copies, s.b), dtype=bool)
    n_calls = n_eligible = 0
    for call in ref["calls"]:
        step, clip, par, tok, sums, margin = call
        k = len(par)
        want = np.stack([np.asarray(par), np.asarray(tok)], axis=1)
        same = (sel[step, :, clip, :k] == want[None]).all(axis=(1, 2))
        if clip not in clips and D.effective_margin(call) <= 0.25 * R16[prec]:
            diverged[:, clip] |= ~same
            continue
        n_eligible += 1
        live = ~diverged[:, clip]
        wrong = np.nonzero(live & ~same)[0]
        assert wrong.size == 0, (tag, "step", step, "clip", clip, "copies", wrong[:8].tolist(), sel[step, wrong[0], clip, :k].tolist(), par, tok)
        np.testing.assert_allclose(val[step, live, clip, :k], np.broadcast_to(np.asarray(sums, dtype=np.float32), (int(live.sum()), k)),
                                   rtol=0, atol=sum_atol * (step + 1), err_msg=str((tag, step, clip)))
        n_calls += int(live.any())
    assert not diverged[:, clips].any(), tag
    for clip in clips:
        assert (mult[:, clip, :, :ps_ref] == ref["mult_preds"][clip].numpy()[None]).all() and not mult[:, clip, :, ps_ref:].any(), (tag, clip)
        assert (best[:, clip, :bm_ref] == ref["best_preds"][clip].numpy()[None]).all() and not best[:, clip, bm_ref:].any(), (tag, clip)
        np.testing.assert_allclose(mult_lp[:, clip], np.broadcast_to(ref["mult_lprobs"][clip].numpy(), mult_lp[:, clip].shape), rtol=0, atol=lp_atol)
        np.testing.assert_allclose(best_lp[:, clip], np.broadcast_to(ref["best_lprobs"][clip].numpy(), best_lp[:, clip].shape), rtol=0, atol=lp_atol)
    print(f"tiled search {tag}: {len(clips)} of {s.b} clips x {t.copies} copies end to end, {n_calls} of {len(ref['calls'])} calls checked, "
          f"{int(diverged.sum())} of {t.b} slots left the oracle's path at a call below the tolerance")
    # (fewer than eligible: a call none of whose copies is still on the oracle's path; the exact precisions never leave it)
    assert n_calls == len(ref["calls"]) if prec in EXACT else n_calls <= n_eligible, tag


STEP = [(i, prec, fusion) for i in range(len(R.TILED)) for prec in D.PRECISIONS for fusion in (True, False)]


@pytest.mark.parametrize("i,prec,fusion", STEP, ids=[f"{R.TILED[i].name}-{p}-{'fused' if fu else 'unfused'}" for i, p, fu in STEP])
def test_tiled_search_matches_the_oracle(i, prec, fusion):
    """Every search of decoder_rows.TILED: R = B x beam above 4096 (two above 8192), decode fusion on and off.  With fusion off the
    FFN2 of the 16-bit and exact precisions runs as split-K slabs on 128-row tiles."""
    t = R.TILED[i]
    h = _geo(t.gname)
    _report("step", t.gname, t, prec, fusion)
    tag = (t.name, prec, D.ffn_regime(prec, h.g.d_ff, fusion), D.search_kernel(h.g.v, t.search.beam))
    _check_tiled(h, prec, t, _decode(h, prec, t, fusion), tag)


PREP = [(i, prec) for i in range(len(R.PREPARE_ONLY)) for prec in D.PRECISIONS]


@pytest.mark.parametrize("i,prec", PREP, ids=[f"{R.PREPARE_ONLY[i].name}-{p}" for i, p in PREP])
def test_prepare_above_8192_frames_search_below_4096_rows(i, prec):
    """dec_prepare alone in the wide regime: B x Ta >= 8192 frames (the frame axis padded with frames at PAD_FRAME_SCALE) while the
    search itself stays on the 64-row tiles."""
    t = R.PREPARE_ONLY[i]
    h = _geo(t.gname)
    here = _report("step", t.gname, t, prec)
    assert all(r.tile[0] == 64 for r in here if not r.site.startswith("dec_prepare")) and all(r.tile[0] >= 128 for r in here if r.site.startswith("dec_prepare"))
    _check_tiled(h, prec, t, _decode(h, prec, t, True), (t.name, prec))


# ---- d. greedy logits -----------------------------------------------------------------------------------------------------------
GREEDY = [(i, prec) for i in range(len(R.GREEDY)) for prec in D.PRECISIONS]


@pytest.mark.parametrize("i,prec", GREEDY, ids=[f"{R.GREEDY[i][0]}-x{R.GREEDY[i][1]}-{p}" for i, p in GREEDY])
def test_greedy_logits_of_thousands_of_clips(i, prec):
    """Engine.greedy's masked logits of every step against oracle.cpu_ref.greedy_search, with the tolerances tests/test_gpu_parity.py
    holds the greedy fixtures to: fp32 / exact every row (finite pattern, rtol 1e-3 / atol 2e-3, the arg-max chain); bf16 / f16 the
    rows whose prefix equals the oracle's (finite pattern, atol 0.8 x R16) -- step 0 is such a row for every clip."""
    case = R.GREEDY[i]
    gname, b, ta, max_pred, seed = case
    h = _geo(gname)
    g = h.g
    _report("greedy", gname, case, prec)
    fe, shape, bos, forbid = h.of_case(("greedy", i), "inputs", lambda: R.greedy_inputs(case))

    def oracle():
        from oracle import cpu_ref as O
        with torch.no_grad():
            mem, mask = O.encode_audio(D.weights(g), fe, shape)
            return O.greedy_search(D.weights(g), mem, mask, bos, vocab_size=g.v, min_pred_size=1, max_pred_size=max_pred,
                                   forbid_rep_mask=forbid, n_layers=g.n_layers)

    want = h.of_case(("greedy", i), "oracle", oracle)                      # (B, V, steps)
    out = h.engine(prec).greedy(fe.cuda(), shape[:, 1].int(), bos, forbid, 1, max_pred)
    got = out["logits"].permute(0, 2, 1).cpu()
    steps = min(got.shape[2], want.shape[2])
    if prec in EXACT:
        assert tuple(got.shape) == tuple(want.shape)
        fin = torch.isfinite(want)
        assert torch.equal(torch.isfinite(got), fin)
        np.testing.assert_allclose(got[fin].numpy(), want[fin].numpy(), rtol=1e-3, atol=2e-3)
        assert torch.equal(got.argmax(dim=1), want.argmax(dim=1))
        assert torch.equal(out["preds"].cpu().long(), got.argmax(dim=1))
        return
    alive, n_cmp = torch.ones(b, dtype=torch.bool), 0
    for st in range(steps):
        rows = torch.nonzero(alive)[:, 0]
        gs, ws = got[rows, :, st], want[rows, :, st]
        fin = torch.isfinite(ws)
        assert torch.equal(torch.isfinite(gs), fin), (gname, prec, st)
        e = float((gs[fin] - ws[fin]).abs().max()) if bool(fin.any()) else 0.0
        print(f"greedy {(gname, b, prec)} step {st}: {rows.numel()} rows on the oracle's prefix, max |d logit| {e:.5f}")
        assert e <= 0.8 * R16[prec], (gname, prec, st, e)
        n_cmp += rows.numel()
        alive[rows] = gs.argmax(dim=1) == ws.argmax(dim=1)
    assert n_cmp >= b


# ---- e. decode_spans over long recordings ---------------------------------------------------------------------------------------
SPAN_RECORDINGS, SPAN_T_REC = 2, 4200                                      # 8400 frames: dec_prepare_spans in the wide regime


@pytest.mark.parametrize("prec", D.PRECISIONS)
def test_decode_spans_over_8400_frames(prec):
    """Engine.decode_spans over 2 recordings of 4200 frames: the clips of the search beam4_r2mod4 of tests/span_cases.py's geometry,
    each planted twice at seeded offsets in seeded noise, the span table pointing at them.  Every span's captions against that
    search's oracle as in (c): all of them in fp32 / exact, the clean clips' in bf16 / f16, the others well-formed."""
    from tests import span_cases as K
    h = _geo(K.GEOMETRY)
    g = h.g
    s = next(s for s in g.searches if s.name == "beam4_r2mod4")
    print(f"tiles at {_n_cu()} compute units, dec_prepare over {SPAN_RECORDINGS * SPAN_T_REC} frames, {prec}:")
    print("\n".join("  " + line for line in R.describe(R._reach(R.prepare_products(g, SPAN_RECORDINGS * SPAN_T_REC), prec, _n_cu()))))

    def inputs():
        fe0, shape0, bos0, forbid = D.search_inputs(g, s)
        rng = np.random.Generator(np.random.PCG64(66000 + s.seed))
        rec = torch.from_numpy(((rng.random((SPAN_RECORDINGS, SPAN_T_REC, 768), dtype=np.float32) * 2.0 - 1.0) * np.float32(0.65 * 3 ** 0.5)))
        table, clip_of = [], []
        slots = rng.permutation(SPAN_T_REC // 32 - 1)[:2 * s.b]             # 32-frame slots: no two plants overlap (Ta = 16)
        for j in range(2 * s.b):
            clip, r = j % s.b, j % SPAN_RECORDINGS
            n, start = s.frame_lens[clip], int(slots[j]) * 32 + int(rng.integers(0, 16))
            if j == 2 * s.b - 1:
                start = SPAN_T_REC - n                                      # the last frames of the last recording: the GEMMs' last rows
            rec[r, start:start + n] = fe0[clip, :n]
            table.append((r, start, n))
            clip_of.append(clip)
        return rec, np.asarray(table, dtype=np.int32), clip_of, bos0[clip_of], forbid

    rec, table, clip_of, bos, forbid = h.of_case("spans", "inputs", inputs)
    ref = h.of_case("spans", "oracle", lambda: D.oracle_search(g, s))
    lens = torch.full((SPAN_RECORDINGS,), SPAN_T_REC, dtype=torch.int32)
    out = h.engine(prec).decode_spans(rec.cuda(), lens, table, bos, forbid, s.beam, s.min_pred, s.max_pred)
    torch.cuda.synchronize()
    out = {k: v.cpu() for k, v in out.items()}
    ps_ref, bm_ref = ref["mult_preds"].shape[2], ref["best_preds"].shape[1]
    ps, bm = (int(x) for x in out["sizes"].tolist())
    mult, best, mult_lp, best_lp = out["mult_preds"].numpy(), out["best_preds"].numpy(), out["mult_lprobs"].numpy(), out["best_lprobs"].numpy()
    if prec in EXACT:
        clips, lp_atol = list(range(s.b)), 1e-4
        assert [ps, bm] == [ps_ref, bm_ref]
    else:
        clips, lp_atol = D.clean_clips(ref["calls"], s.b, 0.25 * R16[prec]), 0.05 * R16[prec]
        assert 1 <= ps <= s.max_pred and 1 <= bm <= s.max_pred
        assert R.malformed(mult[..., :ps], mult_lp, g.v) == [] and R.malformed(best[..., :bm], best_lp, g.v) == []
    assert len(clips) >= 1 or prec == "bf16"                                  # (no clip of this search clears 0.25 in every call)
    for j, clip in enumerate(clip_of):
        if clip not in clips:
            continue
        assert (mult[j, :, :ps_ref] == ref["mult_preds"][clip].numpy()).all() and not mult[j, :, ps_ref:].any(), (prec, j, clip)
        assert (best[j, :bm_ref] == ref["best_preds"][clip].numpy()).all() and not best[j, bm_ref:].any(), (prec, j, clip)
        np.testing.assert_allclose(mult_lp[j], ref["mult_lprobs"][clip].numpy(), rtol=0, atol=lp_atol, err_msg=str((prec, j, clip)))
        np.testing.assert_allclose(best_lp[j], ref["best_lprobs"][clip].numpy(), rtol=0, atol=lp_atol, err_msg=str((prec, j, clip)))
