"""GPU: conette_decode_groups / Engine.decode_groups -- diverse beam search in beam groups with a Hamming penalty (csrc/dec_group.h).

Decoder-only engines on the weights of tests/decoder_geometry.py in fp32, exact, bf16 and f16; the cases are the table of
tests/group_cases.py (its docstring lists what they cover; tests/test_cpu_group_search.py holds them to their input conditions).

1. REPLAY.  Every call of every case is recomputed in float64 (group_search.decide_group) from the library's own step logits and
   trace: masks, log-softmax, the running sums the device carried, the counts of the earlier groups' picks.  Where the call's
   float64 effective margin exceeds DELTA (tests/test_gpu_sample.py: fp32 log-softmax against float64, 1.2e-5) the picks --
   parents, tokens, order -- are identical; the carried sums are within 2e-4 * (step + 1) of their float64 accumulation; every
   output slot, length, out_sizes and best_* is recomputed from the trace.  Calls at or below DELTA are counted: none in fp32 and
   exact (the CPU-checked 2e-3 margin of the oracle's run guarantees it), at most 1 % in bf16 and f16.
2. END TO END against the restatement on the oracle's logits, fp32 and exact: picks identical, scores within 1e-4, captions and
   sizes identical.
3. IDENTITIES with conette_decode, bit for bit, all four precisions: one group equals conette_decode(beam = W) in all outputs;
   group 0 equals it for every G and lambda; with lambda = 0 every group does.
4. HAMMING.  W = 1, lambda = 1e4: the tokens the live groups of a clip pick at one step are pairwise distinct.
5. SCORES ARE THE MODEL'S.  min_pred = 0, no forbid mask: the log-likelihood of every returned hypothesis, recomputed from the
   hypothesis itself, reproduces mult_lprobs x length (see test_scores_are_the_models).
6. STATE INDEPENDENCE.  A clip alone equals the clip in its batch; a 0xFF-filled workspace, a repeated call and capture + replay
   are bit-equal.
7. C ABI errors name the argument, launch nothing and leave the outputs untouched."""
import ctypes as C
import gc
import os

import numpy as np
import pytest
import torch

from conette_amd import group_search as GS
from tests import decoder_geometry as D
from tests import group_cases as GC
from tests.test_gpu_sample import DELTA
from tests.test_gpu_score import CONSISTENCY

pytestmark = pytest.mark.gpu

PRECS = D.PRECISIONS
EXACT = ("fp32", "exact")
KEYS = ("best_preds", "best_lprobs", "mult_preds", "mult_lprobs", "sizes")


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _cpu(o):
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in o.items()}


class _Geo:
    def __init__(self, g):
        self.g, self.engines, self.cache = g, {}, {}
        torch.set_num_threads(min(16, os.cpu_count() or 1))

    def engine(self, prec):
        if prec not in self.engines:
            from conette_amd.engine import Engine
            self.engines[prec] = Engine(D.weights(self.g), precision=prec, n_layers=self.g.n_layers, d_ff=self.g.d_ff)
        return self.engines[prec]

    def run(self, prec, c, g=None, w=None, lam=None, trace=True):
        key = (prec, c.name, g, w, lam)
        if key not in self.cache:
            fe, shape, bos, forbid = GC.inputs(c)
            out = self.engine(prec).decode_groups(fe.cuda(), shape[:, 1].int(), bos, forbid, c.g if g is None else g, c.w if w is None else w,
                                                  c.lam if lam is None else lam, c.min_pred, c.max_pred, want_trace=trace,
                                                  want_logits=trace and g is None and w is None and lam is None)
            self.cache[key] = _cpu(out)
        return self.cache[key]

    def plain(self, prec, c):
        """conette_decode at beam W on the case's inputs"""
        key = (prec, c.name, "plain")
        if key not in self.cache:
            fe, shape, bos, forbid = GC.inputs(c)
            self.cache[key] = _cpu(self.engine(prec).decode(fe.cuda(), shape[:, 1].int(), bos, forbid, c.w, c.min_pred, c.max_pred,
                                                            want_trace=True))
        return self.cache[key]


@pytest.fixture(scope="module", params=GC.GEOS)
def geo(request):
    h = _Geo(D.geometry(request.param))
    yield h
    h.engines.clear()
    h.cache.clear()
    GC._RUNS.clear()
    D.drop_weights(h.g)
    gc.collect()
    torch.cuda.empty_cache()


# ---- 1. replay -------------------------------------------------------------------------------------------------------------------------
def replay(c, out, v):
    """Walks the device's trace; returns (calls, calls at or below DELTA, calls below DELTA whose picks differ)."""
    _, _, bos, forbid = GC.inputs(c)
    fb = None if forbid is None else forbid.numpy()
    gw = c.g * c.w
    sel, val = out["trace_sel"].numpy(), out["trace_val"].numpy()
    logits = out["step_logits"].numpy()
    live = [[[{"prefix": [int(bos[b])], "sum": 0.0, "sum64": 0.0, "slot": g * c.w + j} for j in range(c.w)] for g in range(c.g)]
            for b in range(c.b)]
    out_preds = np.zeros((c.b, gw, c.max_pred), dtype=np.int64)
    out_avg = np.zeros((c.b, gw), dtype=np.float32)
    out_len = np.zeros((c.b, gw), dtype=np.int64)
    n_calls = n_close = n_close_differ = 0
    for step in range(c.max_pred):
        for b in range(c.b):
            counts = np.zeros(v, dtype=np.int64)
            for g in range(c.g):
                grp = live[b][g]
                k = len(grp)
                got = sel[step, b, g * c.w:(g + 1) * c.w]
                tag = (c, "step", step, "clip", b, "group", g)
                assert (got[k:] == -1).all(), tag
                if k == 0:
                    continue
                n = 1 if step == 0 else k
                z = logits[step, b * gw + g * c.w: b * gw + g * c.w + n]
                d = GS.decide_group(z, [r["prefix"] for r in grp], [r["sum"] for r in grp], counts, k, step, c.lam, c.min_pred, GC.EOS, fb)
                got_par, got_tok = (got[:k, 0] - g * c.w).tolist(), got[:k, 1].tolist()
                assert all(0 <= p < n for p in got_par) and all(0 <= t < v for t in got_tok), tag
                n_calls += 1
                if d["margin"] > DELTA:
                    assert (d["parents"], d["tokens"]) == (got_par, got_tok), (tag, d, got.tolist())
                else:
                    n_close += 1
                    n_close_differ += (d["parents"], d["tokens"]) != (got_par, got_tok)
                nxt = []
                for j in range(k):      # the state goes on with the device's picks
                    parent, token, m = got_par[j], got_tok[j], float(val[step, b, g * c.w + j])
                    zm = GS.masked_logits(z[parent], grp[parent]["prefix"], step, c.min_pred, GC.EOS, fb)
                    m64 = grp[parent]["sum64"] + float(GS.log_softmax(zm)[token])
                    assert abs(m - m64) <= 2e-4 * (step + 1), (tag, j, m, m64)
                    counts[token] += 1
                    seq = grp[parent]["prefix"] + [token]
                    if token == GC.EOS or step == c.max_pred - 1:
                        sl = grp[j]["slot"]
                        out_preds[b, sl, :step + 1] = seq[1:]
                        out_avg[b, sl] = np.float32(m) / np.float32(step + 1)
                        out_len[b, sl] = step + 1
                    else:
                        nxt.append({"prefix": seq, "sum": m, "sum64": m64, "slot": grp[j]["slot"]})
                live[b][g] = nxt
    assert all(len(grp) == 0 for clip in live for grp in clip), c
    assert (out_len > 0).all(), c
    assert out["mult_preds"].tolist() == out_preds.tolist(), c
    assert np.array_equal(out["mult_lprobs"].numpy().view(np.int32), out_avg.view(np.int32)), c
    best_preds, best_lp, sizes = GS.finalize(out_preds, out_avg, out_len, GC.EOS)
    assert out["sizes"].tolist() == sizes, (c, out["sizes"].tolist(), sizes)
    assert out["best_preds"].tolist() == best_preds.tolist(), c
    assert np.array_equal(out["best_lprobs"].numpy().view(np.int32), best_lp.view(np.int32)), c
    return n_calls, n_close, n_close_differ


@pytest.mark.parametrize("prec", PRECS)
def test_every_call_replays_in_float64(prec, geo):
    total = close = differ = 0
    for c in GC.cases(geo.g.name):
        n, nc, nd = replay(c, geo.run(prec, c), geo.g.v)
        total, close, differ = total + n, close + nc, differ + nd
        print(f"group replay {prec} {c}: {n} calls, {nc} at or below DELTA = {DELTA} ({nd} of them picked otherwise)")
    print(f"group replay {(geo.g.name, prec)}: {close} of {total} calls at or below DELTA ({close / total:.4%})")
    assert total > 0
    if prec in EXACT:
        assert close == 0, (geo.g.name, prec, close, total)
    else:
        assert close <= 0.01 * total, (geo.g.name, prec, close, total)


# ---- 2. end to end against the restatement on the oracle's logits -----------------------------------------------------------------
@pytest.mark.parametrize("prec", EXACT)
def test_end_to_end_equals_the_restatement(prec, geo):
    for c in GC.cases(geo.g.name):
        out, ref = geo.run(prec, c), GC.oracle_run(c)
        sel, val = out["trace_sel"].numpy(), out["trace_val"].numpy()
        seen = np.zeros(sel.shape[:3], dtype=bool)
        worst = 0.0
        for call in ref["calls"]:
            s, b, g, k = call["step"], call["clip"], call["group"], call["k"]
            at = slice(g * c.w, g * c.w + k)
            assert (sel[s, b, at, 0] - g * c.w).tolist() == call["parents"] and sel[s, b, at, 1].tolist() == call["tokens"], (c, prec, s, b, g)
            worst = max(worst, float(np.abs(val[s, b, at] - np.array(call["sums"])).max()))
            seen[s, b, at] = True
        assert (sel[~seen] == -1).all(), (c, prec)
        assert out["mult_preds"].tolist() == ref["mult_preds"].tolist() and out["best_preds"].tolist() == ref["best_preds"].tolist(), (c, prec)
        assert out["sizes"].tolist() == ref["sizes"], (c, prec)
        worst = max(worst, float(np.abs(out["mult_lprobs"].numpy() - ref["mult_lprobs"]).max()),
                    float(np.abs(out["best_lprobs"].numpy() - ref["best_lprobs"]).max()))
        print(f"group end to end {prec} {c}: {len(ref['calls'])} calls, max |d score| {worst:.3e}")
        assert worst <= 1e-4, (c, prec, worst)


# ---- 3. identities with the pinned search -----------------------------------------------------------------------------------------------
def _group_slice(out, c, grp, w):
    """what group `grp` of a grouped run holds, laid out as a plain search at beam w: parents count from the group's first row"""
    sl = slice(grp * w, (grp + 1) * w)
    sel = out["trace_sel"][:, :, sl].clone()
    sel[..., 0] = torch.where(sel[..., 0] >= 0, sel[..., 0] - grp * w, sel[..., 0])
    return {"mult_preds": out["mult_preds"][:, sl], "mult_lprobs": out["mult_lprobs"][:, sl], "trace_sel": sel,
            "trace_val": out["trace_val"][:, :, sl]}


def _assert_group_is_plain(got, plain, what):
    for k in ("mult_preds", "mult_lprobs", "trace_sel", "trace_val"):
        assert torch.equal(_bits(got[k]), _bits(plain[k])), (what, k)


@pytest.mark.parametrize("prec", PRECS)
def test_one_group_equals_conette_decode(prec, geo):
    for c in GC.cases(geo.g.name):
        plain = geo.plain(prec, c)
        for lam in (0.0, 2.0):
            one = geo.run(prec, c, g=1, lam=lam)
            for k in KEYS + ("trace_sel", "trace_val"):
                assert torch.equal(_bits(one[k]), _bits(plain[k])), (c, prec, lam, k)


@pytest.mark.parametrize("prec", PRECS)
def test_group_zero_and_unpenalised_groups_equal_conette_decode(prec, geo):
    for c in GC.cases(geo.g.name):
        if c.g == 1:
            continue
        plain = geo.plain(prec, c)
        _assert_group_is_plain(_group_slice(geo.run(prec, c), c, 0, c.w), plain, (c, prec, "group 0"))
        other = geo.run(prec, c, lam=0.5 if c.lam == 0 else 0.0)       # the case's own lambda is 0 for a third of the table
        zero, pen = (geo.run(prec, c), other) if c.lam == 0 else (other, geo.run(prec, c))
        _assert_group_is_plain(_group_slice(pen, c, 0, c.w), plain, (c, prec, "group 0, lambda > 0"))
        for grp in range(c.g):
            _assert_group_is_plain(_group_slice(zero, c, grp, c.w), plain, (c, prec, "lambda = 0, group", grp))


# ---- 4. the Hamming property -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ("fp32", "bf16"))
def test_huge_penalty_makes_the_groups_pick_distinct_tokens(prec, geo):
    done = 0
    for c in GC.cases(geo.g.name):
        if c.w != 1 or c.g == 1:
            continue
        assert geo.g.v > c.g
        sel = geo.run(prec, c, lam=1e4)["trace_sel"].numpy()
        several = 0
        for s in range(c.max_pred):
            for b in range(c.b):
                toks = [int(t) for t in sel[s, b, :, 1] if t >= 0]
                assert len(set(toks)) == len(toks), (c, prec, s, b, toks)
                several += len(toks) > 1
        assert several > 0, c
        done += 1
    assert done > 0


# ---- 5. scores are the model's ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_scores_are_the_models(prec, geo):
    """min_pred = 0, no forbid mask (the search's log-softmax is then the unmasked one).  Every returned hypothesis is scored from
    its own tokens: in fp32 and exact by Engine.score, in bf16 and f16 by the forcing logits of the KV-cached step kernels
    (CONETTE_OPT_FORCING_STEPWISE) through float64 log_softmax + gather -- the comparison with equal operands, as
    tests/test_gpu_sample.py::test_score_reproduces_the_sampled_log_probs makes it.  That test holds every TOKEN's log-prob to
    test_gpu_score.CONSISTENCY; the search returns only the mean over a hypothesis' tokens, which is held to the same bound:
    |mult_lprobs - sum / length| <= CONSISTENCY.  A penalised key in place of a model score would miss it by lambda / length."""
    eng = geo.engine(prec)
    compared = 0
    for c in GC.cases(geo.g.name):
        if c.min_pred != 0 or c.forbid:
            continue
        out = geo.run(prec, c)
        fe, shape, bos, _ = GC.inputs(c)
        lens = shape[:, 1].int()
        gw = c.g * c.w
        preds = out["mult_preds"].reshape(-1, c.max_pred).long()
        n_tok = torch.as_tensor([int((r == GC.EOS).nonzero()[0]) + 1 if bool((r == GC.EOS).any()) else c.max_pred for r in preds])
        caps = torch.cat([bos.repeat_interleave(gw)[:, None].long(), preds[:, :-1]], dim=1)
        caps = torch.where(torch.arange(c.max_pred)[None] < n_tok[:, None], caps, torch.zeros_like(caps))
        rows = torch.as_tensor([bool((preds[r, :int(n)] != GC.PAD).all()) for r, n in enumerate(n_tok)])   # pad_id inside: not scorable
        if prec in EXACT:
            sc = eng.score(fe.cuda(), lens, caps, preds, caps_per_audio=gw)
            sums = sc["sum_lprobs"].cpu().double()
            assert sc["n_tokens"].cpu()[rows].tolist() == n_tok[rows].tolist(), (c, prec)
        else:
            eng.set_forcing_stepwise(True)
            try:
                logits = eng.forcing(fe.repeat_interleave(gw, dim=0).cuda(), lens.repeat_interleave(gw), caps).cpu().double()
            finally:
                eng.set_forcing_stepwise(False)
            lp = torch.log_softmax(logits, dim=-1).gather(2, preds[..., None])[..., 0]
            sums = torch.where(torch.arange(c.max_pred)[None] < n_tok[:, None], lp, torch.zeros_like(lp)).sum(dim=1)
        err = (out["mult_lprobs"].reshape(-1).double() - sums / n_tok.double()).abs()[rows]
        print(f"group scores {prec} {c}: {int(rows.sum())} hypotheses, max |mean lp - rescored| {float(err.max()):.3e} (bound {CONSISTENCY:.1e})")
        assert float(err.max()) <= CONSISTENCY, (c, prec, float(err.max()))
        compared += int(rows.sum())
    assert compared > 0


# ---- 6. state independence ---------------------------------------------------------------------------------------------------------------
def _det_case(geo):
    return next(c for c in GC.cases(geo.g.name) if c.b > 1 and c.g > 1 and c.lam > 0)


@pytest.mark.parametrize("prec", PRECS)
def test_clip_alone_equals_clip_in_batch(prec, geo):
    c = _det_case(geo)
    eng = geo.engine(prec)
    fe, shape, bos, forbid = GC.inputs(c)
    lens = shape[:, 1].int()
    full = geo.run(prec, c)
    for i in range(c.b):
        one = _cpu(eng.decode_groups(fe[i:i + 1].cuda(), lens[i:i + 1], bos[i:i + 1], forbid, c.g, c.w, c.lam, c.min_pred, c.max_pred,
                                     want_trace=True))
        for k in ("best_preds", "best_lprobs", "mult_preds", "mult_lprobs"):
            assert torch.equal(_bits(one[k][0]), _bits(full[k][i])), (c, prec, i, k)
        assert torch.equal(one["trace_sel"][:, 0], full["trace_sel"][:, i]), (c, prec, i)
        assert torch.equal(_bits(one["trace_val"][:, 0]), _bits(full["trace_val"][:, i])), (c, prec, i)


@pytest.mark.parametrize("prec", PRECS)
def test_identical_calls_stale_workspace_and_graph_replay_are_bit_equal(prec, geo):
    c = _det_case(geo)
    eng = geo.engine(prec)
    fe, shape, bos, forbid = GC.inputs(c)
    fe_d, lens_d, bos_d = fe.cuda(), shape[:, 1].int().cuda(), bos.int().cuda()
    fb_d = None if forbid is None else forbid.to(torch.uint8).cuda()
    call = lambda: eng.decode_groups(fe_d, lens_d, bos_d, fb_d, c.g, c.w, c.lam, c.min_pred, c.max_pred, want_trace=True)
    first = _cpu(call())
    for k in first:
        assert torch.equal(_bits(first[k]), _bits(geo.run(prec, c)[k])), (c, prec, "the cached run", k)
    for ws in eng._ws.values():
        ws.zero_()
    second = _cpu(call())
    for ws in eng._ws.values():
        ws.fill_(0xFF)
    third = _cpu(call())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = call()
    for x in held.values():
        x.view(torch.uint8).fill_(0xFF)
    graph.replay()
    replayed = _cpu(held)
    for what, o in (("zeroed workspace", second), ("0xFF workspace", third), ("capture + replay", replayed)):
        for k in first:
            assert torch.equal(_bits(first[k]), _bits(o[k])), (c, prec, what, k)
    del graph, held


# ---- 7. C ABI errors -----------------------------------------------------------------------------------------------------------------------
def test_c_abi_errors():
    from conette_amd.engine import Engine
    g = D.geometry("v31_ff32_l2")
    eng = Engine(D.weights(g), precision="bf16", n_layers=g.n_layers, d_ff=g.d_ff)
    b, t, n_g, w, maxp = 2, 7, 3, 2, 6
    fe, shape = D.frames(b, t, (7, 2), 3)
    dev = dict(device="cuda")
    fe_d, lens_d = fe.cuda(), shape[:, 1].int().cuda()
    bos = D.weights(g)["model.task_id_to_token_id"][:b].int().cuda()
    mk = lambda: dict(best_preds=torch.full((b, maxp), -7, dtype=torch.int32, **dev), best_lp=torch.full((b,), -7.0, **dev),
                      mult_preds=torch.full((b, n_g * w, maxp), -7, dtype=torch.int32, **dev), mult_lp=torch.full((b, n_g * w), -7.0, **dev),
                      sizes=torch.full((2,), -7, dtype=torch.int32, **dev))
    o = mk()
    need = int(eng.lib.conette_decode_groups_workspace_bytes(eng._ctx_dec, b, t, n_g, w, maxp))
    assert need > int(eng.lib.conette_decode_workspace_bytes(eng._ctx_dec, b, t, n_g * w, maxp)) > 0
    ws = torch.empty(need, dtype=torch.uint8, **dev)
    good = dict(fe=fe_d, lens=lens_d, bos=bos, b=b, t=t, g=n_g, w=w, lam=0.5, min_pred=0, maxp=maxp, ws=ws, ws_bytes=need, **o)

    def raw(a):
        p = lambda x: C.c_void_p(0 if x is None else x.data_ptr())
        return eng.lib.conette_decode_groups(eng._ctx_dec, p(a["fe"]), p(a["lens"]), p(a["bos"]), p(None), a["b"], a["t"], a["g"], a["w"],
                                             a["lam"], a["min_pred"], a["maxp"], p(a["best_preds"]), p(a["best_lp"]), p(a["mult_preds"]),
                                             p(a["mult_lp"]), p(a["sizes"]), p(None), p(None), p(None), p(a["ws"]), a["ws_bytes"],
                                             C.c_void_p(torch.cuda.current_stream().cuda_stream))

    bad = [({"g": 17, "w": 1}, "n_groups"), ({"g": 3, "w": 6}, "n_groups"), ({"g": 0}, "n_groups"), ({"w": 0}, "group_beam"),
           ({"g": 65536, "w": 65536}, "n_groups"), ({"lam": -0.5}, "diversity_penalty"), ({"lam": float("nan")}, "diversity_penalty"),
           ({"lam": float("inf")}, "diversity_penalty"), ({"ws_bytes": need - 1}, "workspace"), ({"maxp": 65}, "max_pred"),
           ({"min_pred": -1}, "min_pred"), ({"fe": None}, "decode_groups"), ({"mult_preds": None}, "decode_groups")]
    for change, word in bad:
        st = raw({**good, **change})
        msg = eng.lib.conette_last_error().decode()
        assert st != 0 and "decode_groups" in msg and word in msg, (change, st, msg)
    torch.cuda.synchronize()
    for k, x in o.items():      # nothing was launched: the outputs are untouched
        assert bool((x == -7).all()), k
    for args in ((0, t, n_g, w, maxp), (b, t, 0, w, maxp), (b, t, 3, 6, maxp), (b, t, n_g, w, 0)):
        assert eng.lib.conette_decode_groups_workspace_bytes(eng._ctx_dec, *args) == 0
    assert raw(good) == 0, eng.lib.conette_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(o["mult_lp"]).all()) and int(o["sizes"][0]) >= 1
    with pytest.raises(ValueError, match="n_groups"):
        eng.decode_groups(fe_d, lens_d, bos, None, 5, 4, 0.5, 0, maxp)
    with pytest.raises(ValueError, match="diversity_penalty"):
        eng.decode_groups(fe_d, lens_d, bos, None, 3, 2, -1.0, 0, maxp)
    D.drop_weights(g)
