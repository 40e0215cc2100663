"""GPU: conette_sample / Engine.sample -- temperature, top-k and nucleus sampling on the step path (csrc/dec_sample.h).

Decoder-only engines on the weights of tests/decoder_geometry.py, bf16 (fused block path) and fp32 (one launch per sub-layer):
  v31_ff32_l2 (15 of the 16 waves hold no candidate), v2049_ff256_l6, v4097_ff1792_l1 (5 logits per thread),
  v8192_ff2304_l6 (the register limit), v8193_ff4096_l2 (the generic variant).
Per geometry the nine (T, k, p) settings {1, 4} x {0, 40} x {1, 0.9} + (0.5, 0, 0.3) are spread over the row shapes
(B, n) in {(1, 1), (3, 3), (5, 13), (2, 16)} with ragged frame lengths taken from the table's searches (1 included), min_pred
0 / 3, with and without the forbid mask, 12 steps; two more cases, (3, 3) and (5, 13) at min_pred = 0 without the mask; v4097 adds min_pred = max_pred = 9 and v2049 max_pred = 64 with min_pred = 60.

1. REPLAY.  Every decision a row took is recomputed in float64 (conette_amd/sampling.py) from the library's own step logits:
   masks, temperature, both keep rules, the running sum in ascending id.  A token is ACCEPTED iff its float64 interval of the
   running sum comes within DELTA of u, with the kept set of top_p - DELTA or of top_p + DELTA; the GPU token must always be
   accepted; a decision is SETTLED when one token is.  At most 5 % of all decisions of the table may be unsettled.
   DELTA, from the kernel's arithmetic.  A term of the running sum is e = __expf((z - max) / T).  Only terms with e >= DELTA
   matter to first order (a = |z - max| / T <= ln(1 / DELTA) < 11.2); for them
     * the subtraction and the division each round once: |d a| <= 2 * 2^-24 * 11.2 = 1.34e-6, the same relative error of e;
     * __expf(a) = exp2(a * log2 e): the product rounds once, |d| <= 2^-24 * 16.1 * ln 2 = 6.7e-7 relative, v_exp_f32 adds one
       ulp, 1.2e-7: 2.13e-6 per term in all;
     * the sum is a tree of fixed shape: <= 8 terms per thread, 6 wave levels, 16 wave partials, then <= 16 wave bases and
       <= 8 slab bases on the way to a token's running sum: <= 54 additions of non-negative terms, 54 * 2^-24 = 3.2e-6 relative.
   Numerator (running sum) and denominator (total) each carry <= 5.4e-6 relative, their ratio <= 1.08e-5, u * total rounds
   once more (6e-8): 1.09e-5 absolute on a scale of 1.  The same 1.08e-5 (times top_p <= 1) bounds the error of comparing an
   upper mass with top_p * total, hence top_p -/+ DELTA.  Top-k is a count, exact.  DELTA = 1.2e-5 (<= 3e-5).
   Unsettled share of this exact table on the CPU oracle's fp32 logits (oracle/cpu_ref.py stepped through the same cases,
   decisions by sampling.decide): 71 of 11 276 decisions = 0.63 % at DELTA = 1.2e-5; 58 of the 71 are the planted edge uniforms
   of the five one-row T = 4 cases (u = 0 and u = 1 - 2^-24 sit within DELTA of several tokens of small mass by construction),
   the rest come from the other T = 4 cases.  The test prints the share of the run.
2. LOG-PROBS.  |tok_lprobs - float64 log_softmax(masked z)[token]| <= 2^-21 max(1, max_v |z_v|); sum_lprobs is the fp32 sum of
   tok_lprobs in step order, bit for bit; lens, pads and out_sizes follow from preds.
3. LIMITS.  n = 1, top_k = 1 (and top_p = 1e-6) on the table's beam1_* searches: preds equal Engine.decode(beam 1) and
   Engine.greedy, in fp32 the oracle's ids too.  min_pred = 0 without a forbid mask, rows (1, 1), (3, 3) and (5, 13): the sampled
   captions' log-probs recomputed from every row's own caption reproduce tok_lprobs within test_gpu_score.CONSISTENCY -- by
   Engine.score in fp32, by the step-path forcing logits in bf16 (see test_score_reproduces_the_sampled_log_probs).
4. INDEPENDENCE AND DETERMINISM.  A clip alone = the clip in its batch, every geometry and both precisions (bit-equal where the
   step path is row-local bit for bit, up to the first unsettled decision elsewhere: test_clip_alone_equals_clip_in_batch);
   two calls, a 0xFF workspace, eager / capture / replay are bit-equal.
5. C ABI errors name the argument."""
import ctypes as C
import gc
import os

import numpy as np
import pytest
import torch

from conette_amd import sampling as S
from tests import decoder_geometry as D
from tests.test_gpu_score import CONSISTENCY

pytestmark = pytest.mark.gpu

DELTA = 1.2e-5
assert DELTA <= 3e-5
PRECS = ("bf16", "fp32")
GEOS = ("v31_ff32_l2", "v2049_ff256_l6", "v4097_ff1792_l1", "v8192_ff2304_l6", "v8193_ff4096_l2")
SETTINGS = ((1.0, 0, 1.0), (1.0, 0, 0.9), (1.0, 40, 1.0), (1.0, 40, 0.9), (4.0, 0, 1.0), (4.0, 0, 0.9), (4.0, 40, 1.0),
            (4.0, 40, 0.9), (0.5, 0, 0.3))
# (B, n) -> (t_audio, frame_lens): beam1_r1, beam11_r33_generic, beam13_r65, beam4_never_finishes of the table
SHAPES = (((1, 1), 25, (25,)), ((3, 3), 8, (8, 7, 1)), ((5, 13), 7, (7, 3, 5, 1, 6)), ((2, 16), 7, (7, 6)))
U_TOP = 1.0 - 2.0 ** -24


class Case:
    def __init__(self, i, setting, shape, min_pred, max_pred, forbid, plant):
        self.i, (self.temp, self.k, self.p) = i, setting
        (self.b, self.n), self.ta, self.frame_lens = shape
        self.min_pred, self.max_pred, self.forbid, self.plant = min_pred, max_pred, forbid, plant

    def __repr__(self):
        return (f"case{self.i}(T={self.temp}, k={self.k}, p={self.p}, B={self.b}, n={self.n}, min={self.min_pred}, max={self.max_pred}, "
                f"forbid={self.forbid})")


def cases(gname):
    out = [Case(i, st, SHAPES[i % 4], (0, 3)[(i // 4 + i) % 2], 12, i % 4 != 0, i % 3 == 1) for i, st in enumerate(SETTINGS)]
    # several clips x several samples, min_pred = 0, no forbid mask: the cases whose logits the scorer / forcing recompute from
    # every row's own prefix (a row that read another row's KV history would be seen there)
    out.append(Case(10, SETTINGS[0], SHAPES[1], 0, 12, False, False))
    out.append(Case(11, SETTINGS[7], SHAPES[2], 0, 12, False, False))
    if gname == "v4097_ff1792_l1":
        out.append(Case(9, SETTINGS[5], SHAPES[1], 9, 9, True, False))
    if gname == "v2049_ff256_l6":
        out.append(Case(9, SETTINGS[3], SHAPES[1], 60, 64, True, True))
    return out


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _assert_bit_equal(a, b, what, keys=None):
    for k in (keys or a):
        assert torch.equal(_bits(a[k]), _bits(b[k])), (what, k)


class _Geo:
    def __init__(self, g):
        self.g, self.engines, self.cache = g, {}, {}
        torch.set_num_threads(min(16, os.cpu_count() or 1))

    def engine(self, prec):
        if prec not in self.engines:
            from conette_amd.engine import Engine
            self.engines[prec] = Engine(D.weights(self.g), precision=prec, n_layers=self.g.n_layers, d_ff=self.g.d_ff)
        return self.engines[prec]

    def inputs(self, c):
        w = D.weights(self.g)
        fe, shape = D.frames(c.b, c.ta, c.frame_lens, 40 + c.i)
        bos = w["model.task_id_to_token_id"][torch.as_tensor([(c.i + j) % 7 for j in range(c.b)])]
        forbid = w["model.forbid_rep_mask"].bool() if c.forbid else None
        gen = torch.Generator().manual_seed(1234 + c.i)
        u = torch.rand((c.max_pred, c.b, c.n), generator=gen, dtype=torch.float32)
        if c.plant:
            u[0::2, 0, 0] = 0.0
            u[1::2, -1, -1] = U_TOP
            u[1::2, 0, 0] = U_TOP
        return fe, shape[:, 1].int(), bos, forbid, u

    def sample(self, prec, c, **kw):
        key = (prec, c.i)
        if kw or key not in self.cache:
            fe, lens, bos, forbid, u = self.inputs(c)
            out = self.engine(prec).sample(fe.cuda(), lens, bos, forbid, c.n, c.min_pred, c.max_pred, c.temp, c.k, c.p,
                                           uniforms=u.cuda(), want_tokens=True, want_logits=True, **kw)
            torch.cuda.synchronize()
            out = {k: v.cpu() for k, v in out.items()}
            if kw:
                return out
            self.cache[key] = out
        return self.cache[key]


@pytest.fixture(scope="module", params=GEOS)
def geo(request):
    h = _Geo(D.geometry(request.param))
    yield h
    h.engines.clear()
    h.cache.clear()
    D.drop_weights(h.g)
    gc.collect()
    torch.cuda.empty_cache()


def decisions(geo, c, out):
    """The decisions the rows took, from the library's own step logits: (zm (N, V) float64 masked logits, tok (N,), u (N,),
    lp (N,) fp32 as reported)."""
    _, _, bos, forbid, u = geo.inputs(c)
    eos = 2
    preds, lens = out["preds"].reshape(c.b * c.n, c.max_pred).numpy(), out["lens"].reshape(-1).numpy()
    logits = out["step_logits"].reshape(c.b * c.n, c.max_pred, -1)
    lps = out["tok_lprobs"].reshape(c.b * c.n, c.max_pred).numpy()
    uu = u.reshape(c.max_pred, c.b * c.n).numpy()
    fb = None if forbid is None else forbid.numpy()
    zs, toks, us, lp = [], [], [], []
    for r in range(c.b * c.n):
        prefix = [int(bos[r // c.n])]
        for s in range(int(lens[r])):
            zs.append(S.masked_logits(logits[r, s].numpy(), prefix, s, c.min_pred, eos, fb))
            toks.append(int(preds[r, s]))
            us.append(float(uu[s, r]))
            lp.append(lps[r, s])
            prefix.append(int(preds[r, s]))
    return np.stack(zs), np.array(toks), np.array(us, dtype=np.float64), np.array(lp, dtype=np.float32)


def acceptance(zm, u, temp, k, p):
    """(N, V) bool: the tokens whose float64 interval of the running sum comes within DELTA of u, for the kept set of
    top_p - DELTA or of top_p + DELTA."""
    acc = np.zeros(zm.shape, dtype=bool)
    for pp in ((1.0,) if p >= 1.0 else (p - DELTA, min(p + DELTA, 1.0))):
        keep = S.keep_masks(zm / temp, k, pp)
        y = np.where(keep, zm / temp, -np.inf)
        q = np.exp(y - y.max(axis=1, keepdims=True))
        q /= q.sum(axis=1, keepdims=True)
        hi = np.cumsum(q, axis=1)
        lo = hi - q
        last = zm.shape[1] - 1 - np.argmax(keep[:, ::-1], axis=1)
        hi[np.arange(len(hi)), last] = 1.0                      # the largest kept id takes whatever rounding leaves
        acc |= keep & (lo - DELTA <= u[:, None]) & (u[:, None] <= hi + DELTA)
    return acc


_SHARE = {}


def replay(geo, prec, c):
    key = (geo.g.name, prec, c.i)
    if key not in _SHARE:
        out = geo.sample(prec, c)
        zm, tok, u, _ = decisions(geo, c, out)
        acc = acceptance(zm, u, c.temp, c.k, c.p)
        ok = acc[np.arange(len(tok)), tok]
        settled = acc.sum(axis=1) == 1
        _SHARE[key] = (len(tok), int((~settled).sum()), int((~ok).sum()))
        bad = np.nonzero(~ok)[0]
        assert bad.size == 0, (key, c, "decision", int(bad[0]), "token", int(tok[bad[0]]), "accepted", np.nonzero(acc[bad[0]])[0].tolist(),
                               "u", float(u[bad[0]]), f"{bad.size} of {len(tok)}")
    return _SHARE[key]


# ---- 1. replay ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_every_decision_replays_in_float64(prec, geo):
    total = unsettled = 0
    for c in cases(geo.g.name):
        n, un, _ = replay(geo, prec, c)
        total, unsettled = total + n, unsettled + un
        print(f"sample replay {(geo.g.name, prec)} {c}: {n} decisions, {un} unsettled")
    print(f"sample replay {(geo.g.name, prec)}: unsettled share {unsettled / total:.4%} of {total}")
    assert total > 0


def test_unsettled_share_of_the_table():
    """Over every (geometry, precision, case) of the table: at most 5 % of the decisions are unsettled.  Replays already made by
    the tests above are reused; whatever a selection of tests left out is replayed here, so the share is always the whole table's."""
    for name in GEOS:
        h = None
        for prec in PRECS:
            for c in cases(name):
                if (name, prec, c.i) not in _SHARE:
                    h = h or _Geo(D.geometry(name))
                    replay(h, prec, c)
        if h is not None:
            h.engines.clear()
            D.drop_weights(h.g)
            gc.collect()
            torch.cuda.empty_cache()
    keys = [(name, prec, c.i) for name in GEOS for prec in PRECS for c in cases(name)]
    total = sum(_SHARE[k][0] for k in keys)
    unsettled = sum(_SHARE[k][1] for k in keys)
    print(f"sample replay, whole table: {unsettled} of {total} decisions unsettled ({unsettled / total:.4%}) at DELTA = {DELTA}")
    assert unsettled <= 0.05 * total, (unsettled, total)


# ---- 2. log-probs and bookkeeping ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_log_probs_lens_pads_and_sizes(prec, geo):
    worst = 0.0
    for c in cases(geo.g.name):
        out = geo.sample(prec, c)
        tag = (geo.g.name, prec, c)
        zm, tok, _, lp = decisions(geo, c, out)
        m = zm.max(axis=1, keepdims=True)
        ref = (zm - m) - np.log(np.exp(zm - m).sum(axis=1, keepdims=True))
        ref = ref[np.arange(len(tok)), tok]
        zabs = np.where(np.isfinite(zm), np.abs(zm), 0.0).max(axis=1)
        bound = 2.0 ** -21 * np.maximum(1.0, zabs)
        err = np.abs(lp.astype(np.float64) - ref)
        worst = max(worst, float((err / bound).max()))
        assert bool((err <= bound).all()), (tag, float(err.max()), float(bound[err.argmax()]))
        preds = out["preds"].reshape(-1, c.max_pred).numpy()
        lens = out["lens"].reshape(-1).numpy()
        tl = out["tok_lprobs"].reshape(-1, c.max_pred).numpy()
        sums = out["sum_lprobs"].reshape(-1).numpy()
        assert preds.min() >= 0 and preds.max() < geo.g.v, tag
        for r in range(preds.shape[0]):
            eos_at = np.nonzero(preds[r] == 2)[0]
            want_len = int(eos_at[0]) + 1 if eos_at.size else c.max_pred
            assert int(lens[r]) == want_len, (tag, r)
            assert (preds[r, want_len:] == 0).all() and (tl[r, want_len:].view(np.int32) == 0).all(), (tag, r)
            assert want_len > c.min_pred or want_len == c.max_pred, (tag, r, "the EOS floor")
            s = np.float32(tl[r, 0])
            for j in range(1, want_len):
                s = np.float32(s + tl[r, j])
            assert np.float32(sums[r]).view(np.int32) == s.view(np.int32), (tag, r)
            assert (tl[r, :want_len] <= 0).all() and np.isfinite(tl[r, :want_len]).all(), (tag, r)
        assert out["sizes"].tolist() == [int(lens.max())] * 2, tag
        if c.forbid:
            fb = D.weights(geo.g)["model.forbid_rep_mask"].bool().numpy()
            _, _, bos, _, _ = geo.inputs(c)
            for r in range(preds.shape[0]):
                seq = [int(bos[r // c.n])] + preds[r, :lens[r]].tolist()
                rep = [t for j, t in enumerate(seq) if fb[t] and t in seq[:j]]
                assert not rep, (tag, r, rep)
    print(f"sample log-probs {(geo.g.name, prec)}: worst |d lp| / bound {worst:.3f}")


# ---- 3. limits that meet existing paths ------------------------------------------------------------------------------------------------
BEAM1 = [(g.name, s.name) for g in D.GEOMETRIES for s in g.searches if s.name.startswith("beam1_")]


@pytest.mark.parametrize("gname,sname", BEAM1)
def test_top1_equals_the_greedy_paths(gname, sname):
    from conette_amd.engine import Engine
    g = D.geometry(gname)
    s = next(x for x in g.searches if x.name == sname)
    fe, shape, bos, forbid = D.search_inputs(g, s)
    lens = shape[:, 1].int()
    try:
        for prec in PRECS:
            eng = Engine(D.weights(g), precision=prec, n_layers=g.n_layers, d_ff=g.d_ff)
            dec = eng.decode(fe.cuda(), lens, bos, forbid, 1, s.min_pred, s.max_pred)
            gr = eng.greedy(fe.cuda(), lens, bos, forbid, s.min_pred, s.max_pred)
            u = torch.rand((s.max_pred, s.b, 1), generator=torch.Generator().manual_seed(7))
            ids = {}
            for name, kw in (("top_k=1", dict(top_k=1)), ("top_p=1e-6", dict(top_p=1e-6)), ("top_k=1, T=4", dict(top_k=1, temperature=4.0))):
                out = eng.sample(fe.cuda(), lens, bos, forbid, 1, s.min_pred, s.max_pred, uniforms=u.cuda(), **kw)
                ids[name] = out["preds"][:, 0].cpu()
                ps = int(out["sizes"][0])
                tag = (gname, sname, prec, name)
                assert ps == int(dec["sizes"][0]), tag
                assert torch.equal(ids[name][:, :ps], dec["best_preds"][:, :ps].cpu()) and bool((ids[name][:, ps:] == 0).all()), tag
                assert torch.equal(ids[name][:, :gr["preds"].shape[1]], gr["preds"].cpu()), tag
            if prec == "fp32":
                ref = D.oracle_search(g, s)["best_preds"]
                assert ids["top_k=1"][:, :ref.shape[1]].tolist() == ref.tolist(), (gname, sname)
            del eng
    finally:
        D.drop_weights(g)
        gc.collect()
        torch.cuda.empty_cache()


def _sampled_captions(geo, c, out):
    """(caps_in (R, max_pred) with the task token first and pad_id behind the end, preds (R, max_pred), rows (R,) bool: rows without
    pad_id inside the caption -- the scorer and the forcing pass read pad_id as padding, such a row cannot be given to them)"""
    _, _, bos, _, _ = geo.inputs(c)
    preds = out["preds"].reshape(-1, c.max_pred).long()
    lens = out["lens"].reshape(-1)
    caps = torch.cat([bos.repeat_interleave(c.n)[:, None].long(), preds[:, :-1]], dim=1)
    caps = torch.where(torch.arange(c.max_pred)[None] < lens[:, None], caps, torch.zeros_like(caps))
    rows = torch.as_tensor([bool((preds[r, :int(n_)] != 0).all()) for r, n_ in enumerate(lens)])
    return caps, preds, rows


@pytest.mark.parametrize("prec", PRECS)
def test_score_reproduces_the_sampled_log_probs(prec, geo):
    """min_pred = 0, no forbid mask; one-row cases and (3, 3) / (5, 13) rows with distinct prefixes.  The recomputation starts from
    every row's own caption, so it also holds the per-row KV history (anc[r][s] = r % n_samples) to account.
    fp32: Engine.score on the sampled captions, within test_gpu_score.CONSISTENCY.
    bf16: Engine.score runs the ONE-PASS forcing layers, whose 16-bit intermediates are rounded at other places than the step
    path's (measured: up to 1.1e-2 between the two at v8192, against the 3e-3 of CONSISTENCY, which is a bound for equal operands);
    the comparison with equal operands is the library's forcing logits through the KV-cached STEP kernels
    (CONETTE_OPT_FORCING_STEPWISE) on the sampled captions, float64 log_softmax + gather -- held to the same CONSISTENCY."""
    eng = geo.engine(prec)
    compared = multi = 0
    for c in cases(geo.g.name):
        if c.min_pred != 0 or c.forbid:
            continue
        out = geo.sample(prec, c)
        fe, lens, _, _, _ = geo.inputs(c)
        caps, preds, rows = _sampled_captions(geo, c, out)
        want = out["tok_lprobs"].reshape(-1, c.max_pred).double()
        if prec == "fp32":
            sc = eng.score(fe.cuda(), lens, caps, preds, caps_per_audio=c.n)
            got = sc["tok_lprobs"].cpu().double()
            assert sc["n_tokens"].cpu()[rows].tolist() == out["lens"].reshape(-1)[rows].tolist()
        else:
            eng.set_forcing_stepwise(True)
            try:
                logits = eng.forcing(fe.repeat_interleave(c.n, dim=0).cuda(), lens.repeat_interleave(c.n), caps).cpu().double()
            finally:
                eng.set_forcing_stepwise(False)
            got = torch.log_softmax(logits, dim=-1).gather(2, preds[..., None])[..., 0]
        sel = rows[:, None] & (preds != 0)
        if not bool(sel.any()):
            continue
        err = (got - want).abs()[sel]
        print(f"sample vs {'score' if prec == 'fp32' else 'stepwise forcing'} {(geo.g.name, prec)} {c}: {int(sel.sum())} tokens of "
              f"{int(rows.sum())} rows, max |d lp| {float(err.max()):.3e} (bound {CONSISTENCY:.1e})")
        assert float(err.max()) <= CONSISTENCY, (geo.g.name, prec, c, float(err.max()))
        compared += int(rows.sum())
        if c.n > 1:
            distinct = len({tuple(r) for r in preds[rows].tolist()})
            multi += distinct > c.b        # some samples of a clip differ: the check sees the rows' own histories
    assert compared > 0 and multi >= 1, (compared, multi)


# ---- 4. independence and determinism ---------------------------------------------------------------------------------------------------
def _det_case():
    return Case(20, (4.0, 40, 0.9), ((5, 3), 7, (7, 3, 5, 1, 6)), 3, 12, True, True)


@pytest.mark.parametrize("prec", PRECS)
def test_clip_alone_equals_clip_in_batch(prec, geo):
    """Clip i of a (5, 3) call, re-run alone with its slice of the uniforms.  bf16 where the fused FFN kernel runs: equal ids and
    bit-equal log-probs (the step path is row-local bit for bit there: test_gpu_decoder_edges.test_clip_alone_equals_clip_in_batch).
    Elsewhere the GEMMs of another row count sum in another order (2e-5 on a score, the same test): a row's ids are equal up to
    its first decision that is unsettled in the batch run's own replay, where the lone run must still take an accepted token;
    log-probs of the equal part within 2e-5."""
    c = _det_case()
    eng = geo.engine(prec)
    fe, lens, bos, forbid, u = geo.inputs(c)
    full = geo.sample(prec, c)
    bitwise = prec == "bf16" and D.ffn_regime("bf16", geo.g.d_ff).startswith("fused")
    zm, _, uu, _ = decisions(geo, c, full)
    acc = acceptance(zm, uu, c.temp, c.k, c.p)
    first = np.concatenate([[0], np.cumsum(full["lens"].reshape(-1).numpy())])      # decisions() walks rows, then steps
    for i in range(c.b):
        one = eng.sample(fe[i:i + 1].cuda(), lens[i:i + 1], bos[i:i + 1], forbid, c.n, c.min_pred, c.max_pred, c.temp, c.k, c.p,
                         uniforms=u[:, i:i + 1].contiguous().cuda(), want_tokens=True)
        one = {k: v.cpu() for k, v in one.items()}
        tag = (geo.g.name, prec, i)
        if bitwise:
            assert torch.equal(one["preds"][0], full["preds"][i]) and torch.equal(one["lens"][0], full["lens"][i]), tag
            assert torch.equal(_bits(one["tok_lprobs"][0]), _bits(full["tok_lprobs"][i])), tag
            assert torch.equal(_bits(one["sum_lprobs"][0]), _bits(full["sum_lprobs"][i])), tag
            continue
        for j in range(c.n):
            a, b = one["preds"][0, j].tolist(), full["preds"][i, j].tolist()
            n_full = int(full["lens"][i, j])
            same = next((s_ for s_ in range(n_full) if a[s_] != b[s_]), n_full)
            if same < n_full:      # the rows part at an unsettled decision of the batch run, and the lone run took an accepted token
                d = int(first[i * c.n + j]) + same
                assert acc[d].sum() > 1 and acc[d, a[same]], (tag, j, same, a[same], b[same], np.nonzero(acc[d])[0].tolist())
            else:
                assert a == b and int(one["lens"][0, j]) == n_full, (tag, j)
            np.testing.assert_allclose(one["tok_lprobs"][0, j, :same].numpy(), full["tok_lprobs"][i, j, :same].numpy(), rtol=0, atol=2e-5,
                                       err_msg=str((tag, j)))


@pytest.mark.parametrize("prec", PRECS)
def test_identical_calls_stale_workspace_and_graph_replay_are_bit_equal(prec, geo):
    c = _det_case()
    eng = geo.engine(prec)
    fe, lens, bos, forbid, u = geo.inputs(c)
    fe_d, lens_d, bos_d, u_d = fe.cuda(), lens.cuda(), bos.int().cuda(), u.cuda()
    fb_d = forbid.to(torch.uint8).cuda()
    call = lambda: eng.sample(fe_d, lens_d, bos_d, fb_d, c.n, c.min_pred, c.max_pred, c.temp, c.k, c.p, uniforms=u_d, want_tokens=True)
    cpu = lambda o: (torch.cuda.synchronize(), {k: v.cpu() for k, v in o.items()})[1]
    first = cpu(call())
    _assert_bit_equal(first, cpu(call()), (geo.g.name, prec, "second call"))
    for ws in eng._ws.values():
        ws.fill_(0xFF)
    _assert_bit_equal(first, cpu(call()), (geo.g.name, prec, "0xFF workspace"))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = call()
    for x in held.values():
        x.view(torch.uint8).fill_(0xFF)
    graph.replay()
    _assert_bit_equal(first, cpu(held), (geo.g.name, prec, "capture + replay"))
    del graph, held


# ---- 5. C ABI errors -------------------------------------------------------------------------------------------------------------------
def test_c_abi_errors():
    from conette_amd.engine import Engine
    g = D.geometry("v31_ff32_l2")
    eng = Engine(D.weights(g), precision="bf16", n_layers=g.n_layers, d_ff=g.d_ff)
    b, t, n, maxp = 2, 7, 3, 6
    fe, shape = D.frames(b, t, (7, 2), 3)
    dev = dict(device="cuda")
    fe_d, lens_d = fe.cuda(), shape[:, 1].int().cuda()
    bos = D.weights(g)["model.task_id_to_token_id"][:b].int().cuda()
    u = torch.rand((maxp, b * n), **dev)
    preds = torch.empty((b, n, maxp), dtype=torch.int32, **dev)
    sums = torch.empty((b, n), dtype=torch.float32, **dev)
    lens_o = torch.empty((b, n), dtype=torch.int32, **dev)
    sizes = torch.empty((2,), dtype=torch.int32, **dev)
    need = int(eng.lib.conette_sample_workspace_bytes(eng._ctx_dec, b, t, n, maxp))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, **dev)
    good = dict(fe=fe_d, lens=lens_d, bos=bos, u=u, b=b, t=t, n=n, min_pred=0, maxp=maxp, temp=1.0, k=0, p=1.0, preds=preds, sums=sums,
                lens_o=lens_o, sizes=sizes, ws=ws, ws_bytes=need)

    def raw(a):
        p = lambda x: C.c_void_p(0 if x is None else x.data_ptr())
        return eng.lib.conette_sample(eng._ctx_dec, p(a["fe"]), p(a["lens"]), p(a["bos"]), p(None), p(a["u"]), a["b"], a["t"], a["n"],
                                      a["min_pred"], a["maxp"], a["temp"], a["k"], a["p"], p(a["preds"]), p(a["sums"]), p(a["lens_o"]),
                                      p(a["sizes"]), p(None), p(None), p(a["ws"]), a["ws_bytes"],
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream))

    bad = [({"n": 0}, "n_samples"), ({"n": 17}, "n_samples"), ({"temp": 0.0}, "temperature"), ({"temp": float("nan")}, "temperature"),
           ({"temp": float("inf")}, "temperature"), ({"p": 0.0}, "top_p"), ({"p": 1.5}, "top_p"), ({"k": -1}, "top_k"),
           ({"ws_bytes": need - 1}, "workspace"), ({"maxp": 65}, "max_pred"), ({"u": None}, "sample"), ({"preds": None}, "sample")]
    for change, word in bad:
        st = raw({**good, **change})
        msg = eng.lib.conette_last_error().decode()
        assert st != 0 and "sample" in msg and word in msg, (change, st, msg)
    for args in ((0, t, n, maxp), (b, t, 0, maxp), (b, t, n, 0)):
        assert eng.lib.conette_sample_workspace_bytes(eng._ctx_dec, *args) == 0
    assert raw(good) == 0, eng.lib.conette_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(sums).all()) and int(lens_o.min()) >= 1 and int(sizes[0]) == int(lens_o.max())
    with pytest.raises(ValueError, match="uniforms"):
        eng.sample(fe_d, lens_d, bos, None, n, 0, maxp, uniforms=torch.rand((maxp, b, n + 1), **dev))
    D.drop_weights(g)
