"""GPU: conette_score / Engine.score -- log-likelihoods of given captions without logits (csrc/dec_score.h).

Part 1, per decoder geometry of tests/decoder_geometry.py (its forcing case: V = 31 .. 8193 on both sides of every 128-column
tile edge, cap_len 1 .. 64, pad layouts down to one valid token, 1 .. 12 layers) and per precision:
  * against float64 log_softmax + gather of the precision's own oracle (the one the forcing tests use), within the bound
    DERIVED from that test's logit bound: lp = z_t - lse(z) and |d lse| <= max_v |d z_v|, so the logit bound applies once at
    z_t and once at the position's largest |z|;
  * against the same arithmetic on the library's own forcing logits (CONSISTENCY: accumulation order and the fp32
    log-sum-exp are all that differ);
  * pad and out-of-range targets, tok_lprobs = NULL, forced vocabulary splits, stale workspaces, the workspace bound.
Part 2, on the default synthetic decoder (V = 5631, decoder-only contexts): clip -> captions fan-out, chunking, graph capture,
C ABI errors, and the fused path against today's way (forcing on repeated embeddings + log_softmax + gather) at 20 480 rows.

Targets: caps_in shifted left with a trailing pad; in addition every third position of a valid (non-pad) input -- counted over
the whole batch, the first one included, so that the cap_len = 1 case scores a token too -- gets a seeded random id in
[1, V): low-probability tokens and the position after the last valid token are scored as well."""
import ctypes as C
import gc
import os

import numpy as np
import pytest
import torch

from tests import decoder_geometry as D
from tests.test_gpu_decoder_edges import FORCING_MEASURED, ROUNDING

pytestmark = pytest.mark.gpu

EXACT = ("fp32", "exact")
SC_BM, SC_BN, SC_MAX_AUTO_SLABS = 64, 128, 21          # csrc/dec_score.h
# Largest |tok_lprobs - (float64 log_softmax + gather of Engine.forcing's logits)| over all nine geometries x four precisions:
# the same operands and rounding, only the accumulation order and the fp32 log-sum-exp differ.  The ceiling is 3e-3 (worst-case
# fp32 accumulation over K = 256 at these logit magnitudes): anything larger is a bug, not a tolerance.  NOT YET MEASURED on an
# MI355X (no GPU run was possible when this file was written): the tests hold a build to the ceiling and print the figure; once
# measured, CONSISTENCY_MEASURED takes the value and the bound becomes 4 x it.
CONSISTENCY_MEASURED = None
CONSISTENCY = 3e-3 if CONSISTENCY_MEASURED is None else 4 * CONSISTENCY_MEASURED
assert CONSISTENCY <= 3e-3


def auto_slabs(r, v, n_cu=256):
    """cn_score_slabs (csrc/dec_score.h) at the automatic setting"""
    return max(1, min((2 * n_cu) // -(-r // SC_BM), SC_MAX_AUTO_SLABS, -(-v // SC_BN)))


def make_targets(caps, v, seed):
    """(B, L) int64 targets of (B, L) caps_in, see the module docstring"""
    caps = caps.numpy()
    tg = np.zeros_like(caps)
    tg[:, :-1] = caps[:, 1:]
    rng = np.random.Generator(np.random.PCG64(99000 + seed))
    pos = np.argwhere(caps != 0)
    for k in range(0, len(pos), 3):
        tg[pos[k][0], pos[k][1]] = int(rng.integers(1, v))
    return torch.from_numpy(tg)


def ref_from_logits(logits_bvl, targets):
    """float64 (lp (B, L) with 0 at pad targets, z_t (B, L), max_v |z| (B, L)) from (B, V, L) logits"""
    z = torch.as_tensor(logits_bvl).double().permute(0, 2, 1)                      # (B, L, V)
    idx = targets.long().clamp(min=0)[..., None]
    lp = torch.log_softmax(z, dim=-1).gather(2, idx)[..., 0]
    zt = z.gather(2, idx)[..., 0]
    keep = targets != 0
    return torch.where(keep, lp, torch.zeros_like(lp)), zt, z.abs().amax(dim=-1)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _cpu(out):
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu()) for k, v in out.items()}


def _assert_bit_equal(a, b, what):
    for k in a:
        if a[k] is None:
            assert b[k] is None, (what, k)
        else:
            assert torch.equal(_bits(a[k]), _bits(b[k])), (what, k)


class _Geo:
    def __init__(self, g):
        self.g, self.f = g, g.forcing
        self.engines, self.cache = {}, {}
        torch.set_num_threads(min(16, os.cpu_count() or 1))
        self.fe, self.shape, self.caps = D.forcing_inputs(g, g.forcing)
        self.lens = self.shape[:, 1].int()
        self.targets = make_targets(self.caps, g.v, g.forcing.seed)

    def engine(self, prec):
        if prec not in self.engines:
            from conette_amd.engine import Engine
            self.engines[prec] = Engine(D.weights(self.g), precision=prec, n_layers=self.g.n_layers, d_ff=self.g.d_ff)
        return self.engines[prec]

    def oracle_logits(self, kind):
        """(B, V, cap_len) logits of the forcing case: "fp32" (oracle/cpu_ref.py) or "bf16" / "f16" (oracle/bf16_ref.py)"""
        if kind not in self.cache:
            from oracle import bf16_ref as Bf
            from oracle import cpu_ref as O
            if kind == "fp32":
                ref = O.teacher_forcing(D.weights(self.g), self.fe, self.shape, self.caps, n_layers=self.g.n_layers)
            else:
                with Bf.operands(kind):
                    ref = Bf.teacher_forcing_bf16(D.weights(self.g), self.fe, self.shape, self.caps, n_layers=self.g.n_layers)
            self.cache[kind] = ref
        return self.cache[kind]

    def score(self, prec, targets=None, **kw):
        tg = self.targets if targets is None else targets
        return _cpu(self.engine(prec).score(self.fe.cuda(), self.lens, self.caps, tg, **kw))


@pytest.fixture(scope="module", params=[g.name for g in D.GEOMETRIES])
def geo(request):
    h = _Geo(D.geometry(request.param))
    yield h
    h.engines.clear()
    h.cache.clear()
    D.drop_weights(h.g)
    gc.collect()
    torch.cuda.empty_cache()


def logit_bound(geo, prec, z_abs):
    """The forcing test's bound on one logit of magnitude ``z_abs`` (test_forcing_logits_match_the_precisions_oracle): fp32 /
    exact rtol 1e-3, atol 2e-3; 16-bit rtol 3e-3 k, atol 0.15 min(1, 2 k), or -- at the geometries that test holds to measured
    values -- min(2 x FORCING_MEASURED, distance of the operand oracle to the fp32 oracle)."""
    if prec in EXACT:
        return 2e-3 + 1e-3 * z_abs
    g = geo.g
    if g.name in D.MEASURED_BOUND_GEOMETRIES:
        valid = (geo.caps != 0)[:, None, :]
        dist = float(((geo.oracle_logits(prec) - geo.oracle_logits("fp32")).abs() * valid).max())
        return torch.full_like(z_abs, min(2 * FORCING_MEASURED[(g.name, prec)][0], dist))
    k = ROUNDING[prec]
    return 0.15 * min(1.0, 2 * k) + 3e-3 * k * z_abs


# ---- part 1: every geometry ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", D.PRECISIONS)
def test_score_matches_the_precisions_oracle(prec, geo):
    g, f = geo.g, geo.f
    ref_lp, zt, zmax = ref_from_logits(geo.oracle_logits("fp32" if prec in EXACT else prec), geo.targets)
    out = geo.score(prec)
    scored = geo.targets != 0
    n = scored.sum(dim=1)
    assert out["n_tokens"].tolist() == n.tolist() and int(n.sum()) > 0, (g.name, prec)
    bound = (logit_bound(geo, prec, zt.abs()) + logit_bound(geo, prec, zmax)) * scored
    err = (out["tok_lprobs"].double() - ref_lp).abs()
    assert torch.isfinite(out["tok_lprobs"]).all() and torch.isfinite(out["sum_lprobs"]).all()
    has = n > 0
    mean_err = ((out["sum_lprobs"].double() - ref_lp.sum(dim=1)).abs()[has] / n[has])
    mean_bound = (bound.sum(dim=1)[has] / n[has])
    print(f"score {(g.name, f.name, prec)}: rows {f.b * f.cap_len} S {auto_slabs(f.b * f.cap_len, g.v)} max |d lp| {float(err.max()):.3e} "
          f"(bound there {float(bound.flatten()[err.argmax()]):.3e}) max |d sum / n| {float(mean_err.max()):.3e}")
    assert bool((err <= bound).all()), (g.name, prec, float(err.max()))
    assert bool((mean_err <= mean_bound).all()), (g.name, prec, float(mean_err.max()))
    assert bool((out["tok_lprobs"][scored] < 0).all())


@pytest.mark.parametrize("prec", D.PRECISIONS)
def test_score_is_consistent_with_the_librarys_logits(prec, geo):
    eng = geo.engine(prec)
    logits = eng.forcing(geo.fe.cuda(), geo.lens, geo.caps).permute(0, 2, 1).cpu()
    ref_lp, _, _ = ref_from_logits(logits, geo.targets)
    out = geo.score(prec)
    err = float((out["tok_lprobs"].double() - ref_lp).abs().max())
    print(f"score consistency {(geo.g.name, prec)}: max |d lp| {err:.3e} (bound {CONSISTENCY:.1e})")
    assert err <= CONSISTENCY, (geo.g.name, prec, err)


@pytest.mark.parametrize("prec", D.PRECISIONS)
def test_pad_invalid_targets_and_no_token_output(prec, geo):
    g = geo.g
    out = geo.score(prec)
    pad = geo.targets == 0
    assert torch.equal(_bits(out["tok_lprobs"][pad]), torch.zeros(int(pad.sum()), dtype=torch.int32)), "exactly +0.0 at pad targets"
    assert out["n_tokens"].tolist() == (~pad).sum(dim=1).tolist()
    np.testing.assert_allclose(out["sum_lprobs"].numpy(), out["tok_lprobs"].sum(dim=1).numpy(), rtol=1e-5, atol=0)
    nosum = geo.score(prec, want_tokens=False)
    assert nosum["tok_lprobs"] is None
    assert torch.equal(_bits(nosum["sum_lprobs"]), _bits(out["sum_lprobs"])) and torch.equal(nosum["n_tokens"], out["n_tokens"])
    # a target >= V (one that a clamped column of the last tile could "match" were it not masked by index) and one < 0
    rows = [int(i) for i in torch.nonzero((~pad).any(dim=1)).flatten()]
    bad_vals = {rows[0]: g.v + ((-g.v) % SC_BN) // 2, rows[-1]: -3} if len(rows) > 1 else {rows[0]: g.v}
    tg = geo.targets.clone()
    where = {}
    for r, val in bad_vals.items():
        t = int(torch.nonzero(~pad[r]).flatten()[0])
        tg[r, t] = val
        where[r] = t
    bad = geo.score(prec, targets=tg)
    for r, t in where.items():
        assert torch.isnan(bad["tok_lprobs"][r, t]) and torch.isnan(bad["sum_lprobs"][r]), (g.name, prec, r, t)
        assert int(bad["n_tokens"][r]) == int(out["n_tokens"][r])          # still a non-pad target
        keep = torch.ones(tg.shape[1], dtype=torch.bool)
        keep[t] = False
        assert torch.equal(_bits(bad["tok_lprobs"][r, keep]), _bits(out["tok_lprobs"][r, keep]))
    others = [r for r in range(tg.shape[0]) if r not in where]
    for k in ("tok_lprobs", "sum_lprobs", "n_tokens"):
        assert torch.equal(_bits(bad[k][others]), _bits(out[k][others])), (g.name, prec, k)


@pytest.mark.parametrize("prec", D.PRECISIONS)
def test_vocabulary_split(prec, geo):
    """Forced slab counts 1, 2 and 1000 (clamped to the N-tiles) agree within the consistency bound; the automatic choice is
    bit-identical from call to call.  The table holds cases below one row-tile (most) and of three (cap_len 64 x 3 clips); every
    geometry but V = 31 (one N-tile: every setting is one slab) has at least 16 N-tiles."""
    g = geo.g
    eng = geo.engine(prec)
    auto = geo.score(prec)
    _assert_bit_equal(auto, geo.score(prec), (g.name, prec, "auto twice"))
    got = {}
    try:
        for s in (1, 2, 1000):
            eng.set_score_vsplit(s)
            got[s] = geo.score(prec)
            _assert_bit_equal(got[s], geo.score(prec), (g.name, prec, "forced twice", s))
    finally:
        eng.set_score_vsplit(0)
    _assert_bit_equal(auto, geo.score(prec), (g.name, prec, "auto after reset"))
    for s in (2, 1000):
        d = float((got[s]["tok_lprobs"].double() - got[1]["tok_lprobs"].double()).abs().max())
        assert d <= CONSISTENCY, (g.name, prec, s, d)
        assert got[s]["n_tokens"].tolist() == got[1]["n_tokens"].tolist()
    assert float((auto["tok_lprobs"].double() - got[1]["tok_lprobs"].double()).abs().max()) <= CONSISTENCY


def _raw_score(eng, fe, lens, caps, tg, n, t, cpa, cap_len, tok, sums, cnt, ws, ws_bytes=None):
    p = lambda x: C.c_void_p(0 if x is None else x.data_ptr())
    return eng.lib.conette_score(eng._ctx_dec, p(fe), p(lens), p(caps), p(tg), n, t, cpa, cap_len, p(tok), p(sums), p(cnt), p(ws),
                                 (0 if ws is None else ws.numel()) if ws_bytes is None else ws_bytes,
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("prec", ("bf16", "exact"))
def test_workspace_holds_no_logits_and_stale_memory_is_not_read(prec, geo):
    g, f = geo.g, geo.f
    eng = geo.engine(prec)
    r = f.b * f.cap_len
    need = int(eng.lib.conette_score_workspace_bytes(eng._ctx_dec, f.b, f.ta, 1, f.cap_len))
    assert need > 0
    if g.v >= 2048:
        forcing = int(eng.lib.conette_forcing_workspace_bytes(eng._ctx_dec, f.b, f.ta, f.cap_len))
        assert need <= forcing + 256 * r + 65536, (g.name, need, forcing)
        assert need < forcing, "the forcing workspace holds an (R, V) logits buffer, the scoring one must not"
    fe, lens = geo.fe.cuda(), geo.lens.cuda()
    caps, tg = geo.caps.int().cuda(), geo.targets.int().cuda()
    runs = []
    for byte in (None, 0xFF, 0):
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        tok = torch.empty((f.b, f.cap_len), dtype=torch.float32, device="cuda")
        sums = torch.empty((f.b,), dtype=torch.float32, device="cuda")
        cnt = torch.empty((f.b,), dtype=torch.int32, device="cuda")
        if byte is not None:
            for x in (ws, tok, sums, cnt):
                x.view(torch.uint8).fill_(byte)
        assert _raw_score(eng, fe, lens, caps, tg, f.b, f.ta, 1, f.cap_len, tok, sums, cnt, ws) == 0, eng.lib.conette_last_error()
        runs.append(_cpu({"tok_lprobs": tok, "sum_lprobs": sums, "n_tokens": cnt}))
    _assert_bit_equal(runs[0], runs[1], (g.name, prec, "0xFF"))
    _assert_bit_equal(runs[0], runs[2], (g.name, prec, "zeros"))
    _assert_bit_equal(runs[0], geo.score(prec), (g.name, prec, "Engine.score"))


# ---- part 2: the default synthetic decoder (V = 5631, 6 layers), decoder-only contexts ---------------------------------------------
class _Synth:
    def __init__(self, weights):
        self.w = {k: v for k, v in weights.items() if k.startswith("model.")}
        self.v = int(self.w["model.decoder.classifier.weight"].shape[0])
        self.engines = {}

    def engine(self, prec):
        if prec not in self.engines:
            from conette_amd.engine import Engine
            self.engines[prec] = Engine(self.w, precision=prec)
        return self.engines[prec]

    def captions(self, p, cap_len, seed):
        """(caps_in, targets) (P, cap_len) int64: task token, 1 .. cap_len - 1 words, pads; targets = next token, <eos> after the last"""
        rng = np.random.Generator(np.random.PCG64(55000 + seed))
        caps = np.zeros((p, cap_len + 1), dtype=np.int64)
        for i in range(p):
            n = 1 + int(rng.integers(1, cap_len))                 # tokens before <eos>, task token included: 2 .. cap_len
            caps[i, 0] = int(self.w["model.task_id_to_token_id"][i % 7])
            caps[i, 1:n] = 4 + rng.integers(0, self.v - 11, n - 1)
            caps[i, n] = 2
        return torch.from_numpy(caps[:, :-1].copy()), torch.from_numpy(caps[:, 1:].copy())


@pytest.fixture(scope="module")
def synth(synth_weights):
    h = _Synth(synth_weights)
    yield h
    h.engines.clear()
    gc.collect()
    torch.cuda.empty_cache()


FANOUT_ATOL = {"fp32": 1e-5, "exact": 1e-5, "bf16": 1e-3, "f16": 1e-3}    # test_teacher_forcing_matches_reference_fixture's row independence


@pytest.mark.parametrize("prec", D.PRECISIONS)
def test_fan_out_chunks_and_clip_independence(prec, synth):
    """3 clips (9, 4, 1 frames) x 4 captions x 10 positions: equal to caps_per_audio = 1 on embeddings repeated 4 x, each clip
    alone equal to the clip in the batch, and the call split into 3 chunks of clips / 6 slices of captions equal to the
    unsplit call -- bit for bit where a chunk runs the same number of vocabulary slabs."""
    eng = synth.engine(prec)
    n, cpa, cap_len = 3, 4, 10
    fe, shape = D.frames(n, 9, (9, 4, 1), 5)
    lens = shape[:, 1].int()
    caps, tg = synth.captions(n * cpa, cap_len, 1)
    fe_d = fe.cuda()
    full = _cpu(eng.score(fe_d, lens, caps, tg, caps_per_audio=cpa))
    assert full["n_tokens"].tolist() == (tg != 0).sum(dim=1).tolist() and bool((full["n_tokens"] > 0).all())
    atol = FANOUT_ATOL[prec]
    rep = _cpu(eng.score(fe_d.repeat_interleave(cpa, dim=0), lens.repeat_interleave(cpa), caps, tg))
    for k in ("tok_lprobs", "sum_lprobs"):
        np.testing.assert_allclose(full[k].numpy(), rep[k].numpy(), rtol=0, atol=atol * (1 if k == "tok_lprobs" else cap_len), err_msg=f"{prec} {k}")
    np.testing.assert_allclose((full["sum_lprobs"] / full["n_tokens"]).numpy(), (rep["sum_lprobs"] / rep["n_tokens"]).numpy(), rtol=0, atol=atol)
    assert full["n_tokens"].tolist() == rep["n_tokens"].tolist()
    for i in range(n):
        rows = slice(i * cpa, (i + 1) * cpa)
        one = _cpu(eng.score(fe_d[i:i + 1], lens[i:i + 1], caps[rows], tg[rows], caps_per_audio=cpa))
        np.testing.assert_allclose(one["tok_lprobs"].numpy(), full["tok_lprobs"][rows].numpy(), rtol=0, atol=atol, err_msg=f"{prec} clip {i}")
        assert one["n_tokens"].tolist() == full["n_tokens"][rows].tolist()
    need = lambda a, b: int(eng.lib.conette_score_workspace_bytes(eng._ctx_dec, a, 9, b, cap_len))
    from conette_amd import scoring
    for bound, n_chunks, rows_per_chunk in ((need(1, cpa), 3, cpa * cap_len), (need(1, 2), 6, 2 * cap_len)):
        assert len(scoring.plan_chunks(n, cpa, need, bound)) == n_chunks
        eng.score_workspace_bound = bound
        try:
            part = _cpu(eng.score(fe_d, lens, caps, tg, caps_per_audio=cpa))
        finally:
            del eng.score_workspace_bound
        if auto_slabs(rows_per_chunk, synth.v) == auto_slabs(n * cpa * cap_len, synth.v):
            _assert_bit_equal(full, part, (prec, n_chunks))
        else:
            assert float((part["tok_lprobs"].double() - full["tok_lprobs"].double()).abs().max()) <= CONSISTENCY, (prec, n_chunks)
            assert part["n_tokens"].tolist() == full["n_tokens"].tolist()


@pytest.mark.parametrize("prec", ("bf16", "exact"))
def test_eager_capture_and_replay_agree(prec, synth):
    eng = synth.engine(prec)
    n, cpa, cap_len = 2, 3, 12
    fe, shape = D.frames(n, 8, (8, 5), 6)
    caps, tg = synth.captions(n * cpa, cap_len, 2)
    fe_d, lens_d, caps_d, tg_d = fe.cuda(), shape[:, 1].int().cuda(), caps.int().cuda(), tg.int().cuda()
    eager = _cpu(eng.score(fe_d, lens_d, caps_d, tg_d, caps_per_audio=cpa))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = eng.score(fe_d, lens_d, caps_d, tg_d, caps_per_audio=cpa)
    for name in ("first replay", "second replay"):
        for x in held.values():
            x.view(torch.uint8).fill_(0xFF)
        graph.replay()
        _assert_bit_equal(eager, _cpu(held), (prec, name))
    del graph, held


def test_c_abi_errors(synth):
    eng = synth.engine("bf16")
    n, t, cpa, cap_len = 2, 8, 2, 6
    fe, shape = D.frames(n, t, (8, 3), 7)
    caps, tg = synth.captions(n * cpa, cap_len, 3)
    fe_d, lens_d, caps_d, tg_d = fe.cuda(), shape[:, 1].int().cuda(), caps.int().cuda(), tg.int().cuda()
    need = int(eng.lib.conette_score_workspace_bytes(eng._ctx_dec, n, t, cpa, cap_len))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    tok = torch.empty((n * cpa, cap_len), dtype=torch.float32, device="cuda")
    sums = torch.empty((n * cpa,), dtype=torch.float32, device="cuda")
    cnt = torch.empty((n * cpa,), dtype=torch.int32, device="cuda")
    good = dict(fe=fe_d, lens=lens_d, caps=caps_d, tg=tg_d, n=n, t=t, cpa=cpa, cap_len=cap_len, tok=tok, sums=sums, cnt=cnt, ws=ws)
    bad_calls = [{k: None} for k in ("fe", "lens", "caps", "tg", "sums", "cnt", "ws")]
    bad_calls += [{"cap_len": 0}, {"cap_len": D.CN_MAX_PRED + 1}, {"cpa": 0}, {"cpa": -1}, {"n": 0}, {"ws_bytes": need - 1}]
    for change in bad_calls:
        st = _raw_score(eng, **{**good, **change})
        msg = eng.lib.conette_last_error().decode()
        assert st != 0 and "score" in msg, (change, st, msg)
    for args in ((0, t, cpa, cap_len), (n, t, 0, cap_len), (n, t, cpa, 0)):
        assert eng.lib.conette_score_workspace_bytes(eng._ctx_dec, *args) == 0
    assert _raw_score(eng, **good) == 0, eng.lib.conette_last_error()
    assert _raw_score(eng, **{**good, "tok": None}) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(sums).all()) and cnt.tolist() == (tg != 0).sum(dim=1).tolist()
    with pytest.raises(ValueError, match="caps_in ids"):      # Engine.score holds the ids to the vocabulary before the call
        eng.score(fe_d, lens_d, torch.full_like(caps, synth.v), tg, caps_per_audio=cpa)


def test_faster_than_forcing_plus_log_softmax(synth):
    """16 clips x 64 captions x 20 positions in bf16 (20 480 rows; their logits alone would be 461 MB): Engine.score against
    Engine.forcing on 64-times repeated embeddings + log_softmax + gather, medians of 5 after warm-up."""
    eng = synth.engine("bf16")
    n, m, cap_len, t = 16, 64, 20, 32
    fe, shape = D.frames(n, t, tuple(32 - (i % 5) for i in range(n)), 8)
    caps, tg = synth.captions(n * m, cap_len, 4)
    fe_d, lens_d, caps_d, tg_d = fe.cuda(), shape[:, 1].int().cuda(), caps.int().cuda(), tg.int().cuda()
    fe_rep, lens_rep = fe_d.repeat_interleave(m, dim=0), lens_d.repeat_interleave(m)
    idx = tg_d.long()[..., None]

    def fused():
        return eng.score(fe_d, lens_d, caps_d, tg_d, caps_per_audio=m)["sum_lprobs"]

    def today():
        lp = torch.log_softmax(eng.forcing(fe_rep, lens_rep, caps_d), dim=-1).gather(2, idx)[..., 0]
        return torch.where(tg_d != 0, lp, torch.zeros_like(lp)).sum(dim=1)

    def median_ms(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return sorted(ms)[2]

    np.testing.assert_allclose(fused().cpu().numpy(), today().cpu().numpy(), rtol=0, atol=cap_len * 1e-3)
    t_old, t_new = median_ms(today), median_ms(fused)
    print(f"score {n} x {m} x {cap_len} bf16: fused {t_new:.3f} ms, forcing + log_softmax + gather {t_old:.3f} ms, ratio {t_old / t_new:.2f}")
    assert t_new < t_old
