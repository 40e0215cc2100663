"""GPU: conette_decode_ensemble / Engine.decode_ensemble -- one beam search scored by several checkpoints or tasks (csrc/dec_ensemble.h).

Decoder-only engines on the weights of tests/ensemble_cases.py (the geometries of tests/decoder_geometry.py at synth seeds 0 .. 3)
in fp32, exact, bf16 and f16; the cases are the table of tests/ensemble_cases.py (its docstring lists what they cover;
tests/test_cpu_ensemble_search.py holds them to their input conditions).

1. REPLAY.  Every call of every case is recomputed in float64 (ensemble_search.decide) from the library's own step logits of every
   member and its trace.  Where the call's float64 effective margin exceeds THRESHOLD(M, rule) = DELTA (tests/test_gpu_sample.py:
   fp32 log-softmax against float64) + 2 x DELTA_ENS[M][rule] (tests/ensemble_cases.py: the fp32 combination against float64) the
   picks -- parents, tokens, order -- are identical; the carried sums are within 2e-4 * (step + 1) of their float64 accumulation;
   every output slot, length, out_sizes and best_* is recomputed from the trace.  Calls at or below the threshold are counted:
   none in fp32 and exact (the CPU-checked 2e-3 margin of the oracle's run guarantees it), at most 1 % in bf16 and f16.
2. END TO END against the restatement on the oracle's logits, fp32 and exact: picks, captions and sizes identical; carried sums
   and returned scores within 1e-4 (the diverse search's bound) -- in the one case of 64 steps, whose sums reach magnitudes where
   one fp32 rounding exceeds that, a carried sum within 1e-4 + 2 ulp(|sum|).
3. IDENTITIES with conette_decode, bit for bit, all four precisions, all outputs: one member under either rule; 2 and 4 copies of
   one member (same context, same task tokens, separate workspaces) at equal weights under "logprob".
4. SWAPPING the two members of an M = 2 ensemble (fp32 and exact, where every call's margin is known to exceed the threshold):
   the same picks; returned scores within the threshold, carried sums within 2.5 ulp(|sum|) x (step + 1) -- the two orders of
   one two-term sum differ by a rounding per step.
5. STATE INDEPENDENCE.  A clip alone equals the clip in its batch; a 0xFF-filled workspace, a repeated call, the library's own
   capture + replay and a capture by the caller are bit-equal.
6. C ABI errors name the argument, launch nothing and leave the outputs untouched."""
import ctypes as C
import gc
import os

import numpy as np
import pytest
import torch

from conette_amd import ensemble_search as ES
from conette_amd import group_search as GS
from tests import decoder_geometry as D
from tests import ensemble_cases as EC
from tests.test_gpu_sample import DELTA

pytestmark = pytest.mark.gpu

PRECS = D.PRECISIONS
EXACT = ("fp32", "exact")
KEYS = ("best_preds", "best_lprobs", "mult_preds", "mult_lprobs", "sizes")


def threshold(m: int, rule: str) -> float:
    return DELTA + 2.0 * EC.DELTA_ENS[m][rule]


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _cpu(o):
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in o.items()}


class _Geo:
    def __init__(self, g):
        self.g, self.engines, self.cache = g, {}, {}
        torch.set_num_threads(min(16, os.cpu_count() or 1))

    def engine(self, prec, wseed=0):
        if (prec, wseed) not in self.engines:
            from conette_amd.engine import Engine
            self.engines[(prec, wseed)] = Engine(EC.member_weights(self.g.name, wseed), precision=prec, n_layers=self.g.n_layers,
                                                 d_ff=self.g.d_ff)
        return self.engines[(prec, wseed)]

    def members(self, prec, c, order=None, clips=None):
        mem, shape, forbid = EC.inputs(c)
        w = c.weights if c.weights is not None else (1.0,) * c.m
        sl = slice(None) if clips is None else clips
        out = [(self.engine(prec, ws), fe[sl].cuda(), bos[sl], w[i]) for i, (ws, fe, bos) in enumerate(mem)]
        if order is not None:
            out = [out[i] for i in order]
        return out, shape[sl, 1].int(), forbid

    def run(self, prec, c, order=None, trace=True, logits=None):
        key = (prec, c.name, order)
        if key not in self.cache:
            mem, lens, forbid = self.members(prec, c, order)
            out = mem[0][0].decode_ensemble(mem, lens, forbid, c.beam, c.min_pred, c.max_pred, combine=c.rule, want_trace=trace,
                                            want_logits=(order is None) if logits is None else logits, want_margins=True)
            self.cache[key] = _cpu(out)
        return self.cache[key]

    def plain(self, prec, c):
        """conette_decode of member 0 alone on the case's inputs"""
        key = (prec, c.name, "plain")
        if key not in self.cache:
            mem, lens, forbid = self.members(prec, c)
            eng, fe, bos, _ = mem[0]
            self.cache[key] = _cpu(eng.decode(fe, lens, bos, forbid, c.beam, c.min_pred, c.max_pred, want_trace=True, want_margins=True))
        return self.cache[key]

    def copies(self, prec, c, n, rule):
        """n copies of member 0 at equal weights"""
        key = (prec, c.name, "copies", n, rule)
        if key not in self.cache:
            mem, lens, forbid = self.members(prec, c)
            eng, fe, bos, _ = mem[0]
            out = eng.decode_ensemble([(eng, fe, bos, 1.0)] * n, lens, forbid, c.beam, c.min_pred, c.max_pred, combine=rule, want_trace=True,
                                      want_margins=True)
            self.cache[key] = _cpu(out)
        return self.cache[key]


@pytest.fixture(scope="module", params=EC.GEOS)
def geo(request):
    h = _Geo(D.geometry(request.param))
    yield h
    h.engines.clear()
    h.cache.clear()
    EC._RUNS.clear()
    EC.drop_member_weights(h.g.name)
    D.drop_weights(h.g)
    gc.collect()
    torch.cuda.empty_cache()


def _weights32(c):
    """the weights as the device received them: normalised in float64, rounded to fp32"""
    w, _ = ES.check_arguments(c.m, c.weights, c.rule, c.beam)
    return w.astype(np.float32).astype(np.float64)


# ---- 1. replay -------------------------------------------------------------------------------------------------------------------------
def replay(c, out, v):
    """Walks the device's trace; returns (calls, calls at or below the threshold, those of them whose picks differ)."""
    mem, _, forbid = EC.inputs(c)
    fb = None if forbid is None else forbid.numpy()
    bos = np.stack([b.numpy() for _, _, b in mem])
    w = _weights32(c)
    thr = threshold(c.m, c.rule)
    sel, val = out["trace_sel"].numpy(), out["trace_val"].numpy()
    logits = out["step_logits"].numpy()          # (max_pred, M, B * beam, V)
    live = [[{"prefix": [int(bos[0, b])], "sum": 0.0, "sum64": 0.0, "slot": j} for j in range(c.beam)] for b in range(c.b)]
    out_preds = np.zeros((c.b, c.beam, c.max_pred), dtype=np.int64)
    out_avg = np.zeros((c.b, c.beam), dtype=np.float32)
    out_len = np.zeros((c.b, c.beam), dtype=np.int64)
    n_calls = n_close = n_close_differ = 0
    for step in range(c.max_pred):
        for b in range(c.b):
            rows = live[b]
            k = len(rows)
            got = sel[step, b]
            tag = (c, "step", step, "clip", b)
            assert (got[k:] == -1).all(), tag
            if k == 0:
                continue
            n = 1 if step == 0 else k
            z = logits[step, :, b * c.beam: b * c.beam + n]
            prefixes = [r["prefix"] for r in rows]
            d = ES.decide(z, prefixes, bos[:, b], [r["sum"] for r in rows], w, c.rule, k, step, c.min_pred, EC.EOS, fb)
            got_par, got_tok = got[:k, 0].tolist(), got[:k, 1].tolist()
            assert all(0 <= p < n for p in got_par) and all(0 <= t < v for t in got_tok), tag
            n_calls += 1
            if d["margin"] > thr:
                assert (d["parents"], d["tokens"]) == (got_par, got_tok), (tag, d, got.tolist())
            else:
                n_close += 1
                n_close_differ += (d["parents"], d["tokens"]) != (got_par, got_tok)
            comb = ES.combine_log_probs(ES.member_log_probs(z, prefixes, bos[:, b], step, c.min_pred, EC.EOS, fb), w, c.rule)
            nxt = []
            for j in range(k):      # the state goes on with the device's picks
                parent, token, m = got_par[j], got_tok[j], float(val[step, b, j])
                m64 = rows[parent]["sum64"] + float(comb[parent, token])
                assert abs(m - m64) <= 2e-4 * (step + 1), (tag, j, m, m64)
                seq = rows[parent]["prefix"] + [token]
                if token == EC.EOS or step == c.max_pred - 1:
                    sl = rows[j]["slot"]
                    out_preds[b, sl, :step + 1] = seq[1:]
                    out_avg[b, sl] = np.float32(m) / np.float32(step + 1)
                    out_len[b, sl] = step + 1
                else:
                    nxt.append({"prefix": seq, "sum": m, "sum64": m64, "slot": rows[j]["slot"]})
            live[b] = nxt
    assert all(len(rows) == 0 for rows in live), c
    assert (out_len > 0).all(), c
    assert out["mult_preds"].tolist() == out_preds.tolist(), c
    assert np.array_equal(out["mult_lprobs"].numpy().view(np.int32), out_avg.view(np.int32)), c
    best_preds, best_lp, sizes = GS.finalize(out_preds, out_avg, out_len, EC.EOS)
    assert out["sizes"].tolist() == sizes, (c, out["sizes"].tolist(), sizes)
    assert out["best_preds"].tolist() == best_preds.tolist(), c
    assert np.array_equal(out["best_lprobs"].numpy().view(np.int32), best_lp.view(np.int32)), c
    return n_calls, n_close, n_close_differ


@pytest.mark.parametrize("prec", PRECS)
def test_every_call_replays_in_float64(prec, geo):
    total = close = differ = 0
    for c in EC.cases(geo.g.name):
        n, nc, nd = replay(c, geo.run(prec, c), geo.g.v)
        total, close, differ = total + n, close + nc, differ + nd
        print(f"ensemble replay {prec} {c}: {n} calls, {nc} at or below {threshold(c.m, c.rule):.2e} ({nd} of them picked otherwise)")
    print(f"ensemble replay {(geo.g.name, prec)}: {close} of {total} calls at or below the threshold ({close / total:.4%})")
    assert total > 0
    if prec in EXACT:
        assert close == 0, (geo.g.name, prec, close, total)
    else:
        assert close <= 0.01 * total, (geo.g.name, prec, close, total)


# ---- 2. end to end against the restatement on the oracle's logits -----------------------------------------------------------------
@pytest.mark.parametrize("prec", EXACT)
def test_end_to_end_equals_the_restatement(prec, geo):
    for c in EC.cases(geo.g.name):
        out, ref = geo.run(prec, c), EC.oracle_run(c)
        sel, val = out["trace_sel"].numpy(), out["trace_val"].numpy()
        seen = np.zeros(sel.shape[:3], dtype=bool)
        # One bound, the diverse search's 1e-4, on the carried sums (the score of the rule, sum[p] + c(p, v)) and on the returned
        # averaged scores together, in every case of up to 10 steps.  The one long case (max_pred = 64) carries sums of a magnitude
        # at which 1e-4 is below one fp32 rounding (near -1300 an ulp is 1.2e-4): there a carried sum is allowed 1e-4 + 2 ulp(|sum|).
        worst = worst_long = 0.0
        for call in ref["calls"]:
            s, b, k = call["step"], call["clip"], call["k"]
            assert sel[s, b, :k, 0].tolist() == call["parents"] and sel[s, b, :k, 1].tolist() == call["tokens"], (c, prec, s, b)
            want = np.array(call["sums"])
            err = np.abs(val[s, b, :k] - want)
            if c.max_pred <= 10:
                worst = max(worst, float(err.max()))
            else:
                worst_long = max(worst_long, float((err / (1e-4 + 2.0 * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64))).max()))
            seen[s, b, :k] = True
        assert (sel[~seen] == -1).all(), (c, prec)
        assert out["mult_preds"].tolist() == ref["mult_preds"].tolist() and out["best_preds"].tolist() == ref["best_preds"].tolist(), (c, prec)
        assert out["sizes"].tolist() == ref["sizes"], (c, prec)
        worst = max(worst, float(np.abs(out["mult_lprobs"].numpy() - ref["mult_lprobs"]).max()),
                    float(np.abs(out["best_lprobs"].numpy() - ref["best_lprobs"]).max()))
        print(f"ensemble end to end {prec} {c}: {len(ref['calls'])} calls, max |d score| {worst:.3e}"
              + (f", carried sums of the long case at {worst_long:.3f} of 1e-4 + 2 ulp" if c.max_pred > 10 else ""))
        assert worst <= 1e-4, (c, prec, worst)
        assert worst_long <= 1.0, (c, prec, worst_long)


# ---- 3. identities with conette_decode -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_one_member_and_copies_of_one_member_equal_conette_decode(prec, geo):
    for c in EC.cases(geo.g.name):
        plain = geo.plain(prec, c)
        for what, got in (("one member, logprob", geo.copies(prec, c, 1, "logprob")), ("one member, prob", geo.copies(prec, c, 1, "prob")),
                          ("two copies", geo.copies(prec, c, 2, "logprob")), ("four copies", geo.copies(prec, c, 4, "logprob"))):
            for k in KEYS + ("trace_sel", "trace_val", "margins"):
                assert torch.equal(_bits(got[k]), _bits(plain[k])), (c, prec, what, k)


# ---- 4. swapping the members -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", EXACT)
def test_swapping_two_members_keeps_the_picks(prec, geo):
    """fp32 and exact only: there the device's logits are the oracle's to 1e-4 and the CPU-checked margins (>= 2e-3) put every call
    above the threshold, so equal picks are owed; in bf16 and f16 a call of the device's own logits may lie at or below the
    threshold (the replay test counts them), where either order's pick is legitimate."""
    done = 0
    for c in EC.cases(geo.g.name):
        if c.m != 2:
            continue
        a, b = geo.run(prec, c), geo.run(prec, c, order=(1, 0))
        thr = threshold(2, c.rule)
        assert torch.equal(a["trace_sel"], b["trace_sel"]), (c, prec)
        for k in ("best_preds", "mult_preds", "sizes"):
            assert torch.equal(a[k], b[k]), (c, prec, k)
        for k in ("best_lprobs", "mult_lprobs"):
            assert float((a[k] - b[k]).abs().max()) <= thr, (c, prec, k)
        # The carried sums: the two orders of the two-term combination differ by at most 1.5 ulp(c), and each run rounds
        # base + c once, half an ulp of the sum each; per step the two runs therefore part by at most 2.5 ulp(|sum|), (step + 1)
        # times that since step 0.  (A flat bound cannot hold: the roundings accumulate, and at step 64 one ulp is above it.)
        va, vb = a["trace_val"].double(), b["trace_val"].double()
        ulp = torch.from_numpy(np.spacing(np.maximum(va.abs().numpy(), vb.abs().numpy()).astype(np.float32)).astype(np.float64))
        steps = torch.arange(1, c.max_pred + 1, dtype=torch.float64)[:, None, None]
        assert bool(((va - vb).abs() <= 2.5 * ulp * steps).all()), (c, prec, float(((va - vb).abs() / (2.5 * ulp * steps)).max()))
        done += 1
    assert done > 0


# ---- 5. state independence ---------------------------------------------------------------------------------------------------------------
def _det_case(geo):
    return next(c for c in EC.cases(geo.g.name) if c.b > 1 and c.m > 1)


@pytest.mark.parametrize("prec", PRECS)
def test_clip_alone_equals_clip_in_batch(prec, geo):
    c = _det_case(geo)
    full = geo.run(prec, c)
    for i in range(c.b):
        mem, lens, forbid = geo.members(prec, c, clips=slice(i, i + 1))
        one = _cpu(mem[0][0].decode_ensemble(mem, lens, forbid, c.beam, c.min_pred, c.max_pred, combine=c.rule, want_trace=True))
        for k in ("best_preds", "best_lprobs", "mult_preds", "mult_lprobs"):
            assert torch.equal(_bits(one[k][0]), _bits(full[k][i])), (c, prec, i, k)
        assert torch.equal(one["trace_sel"][:, 0], full["trace_sel"][:, i]), (c, prec, i)
        assert torch.equal(_bits(one["trace_val"][:, 0]), _bits(full["trace_val"][:, i])), (c, prec, i)


@pytest.mark.parametrize("prec", PRECS)
def test_identical_calls_stale_workspace_and_graph_replay_are_bit_equal(prec, geo):
    c = _det_case(geo)
    mem, lens, forbid = geo.members(prec, c)
    # every input on the device: a capture must hold no copy from host memory that is gone when the graph is replayed
    mem = [(e, fe, bos.int().cuda(), w) for e, fe, bos, w in mem]
    lens = lens.cuda()
    forbid = None if forbid is None else forbid.to(torch.uint8).cuda()
    eng = mem[0][0]
    call = lambda: eng.decode_ensemble(mem, lens, forbid, c.beam, c.min_pred, c.max_pred, combine=c.rule, want_trace=True)
    ref = geo.run(prec, c)
    # the library captures its graph on a stream of its caller's, never on the default stream -- where an attempt (a second call on
    # the same buffers, which the cached runs of this module make) switches the context's graph cache off: switched on again here
    eng.set_decode_graph(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        first = _cpu(call())          # first sighting of these buffers: eager
        for ws in eng._ws.values():
            ws.zero_()
        second = _cpu(call())         # second sighting: the library captures its graph
        for ws in eng._ws.values():
            ws.fill_(0xFF)
        third = _cpu(call())          # replayed from the graph cache of member 0's context
    torch.cuda.current_stream().wait_stream(side)
    for k in first:
        assert torch.equal(_bits(first[k]), _bits(ref[k])), (c, prec, "the cached run", k)
    assert eng.decode_graph_nodes() > 0, (c, prec)
    for what, o in (("zeroed workspace", second), ("0xFF workspace + library replay", third)):
        for k in first:
            assert torch.equal(_bits(first[k]), _bits(o[k])), (c, prec, what, k)
    print(f"ensemble state {prec} {c}: repeated calls and the library's replay ({eng.decode_graph_nodes()} nodes) are bit-equal", flush=True)
    graph = torch.cuda.CUDAGraph()      # (on a capturing stream the library launches into the caller's graph)
    with torch.cuda.graph(graph):
        held = eng.decode_ensemble(mem, lens, forbid, c.beam, c.min_pred, c.max_pred, combine=c.rule, want_trace=True, clone=False)
    for x in held.values():
        x.view(torch.uint8).fill_(0xFF)
    graph.replay()
    replayed = _cpu(held)
    print(f"ensemble state {prec} {c}: the caller's capture replayed", flush=True)
    for k in first:
        assert torch.equal(_bits(first[k]), _bits(replayed[k])), (c, prec, "caller's capture + replay", k)
    del graph, held


# ---- 6. C ABI errors -----------------------------------------------------------------------------------------------------------------------
def test_c_abi_errors():
    from conette_amd.engine import ConetteMemberC, Engine
    g = D.geometry("v31_ff32_l2")
    other = D.geometry("v2049_ff256_l6")
    eng = Engine(D.weights(g), precision="bf16", n_layers=g.n_layers, d_ff=g.d_ff)
    eng32 = Engine(D.weights(g), precision="fp32", n_layers=g.n_layers, d_ff=g.d_ff)
    engv = Engine(D.weights(other), precision="bf16", n_layers=other.n_layers, d_ff=other.d_ff)
    b, t, beam, maxp = 2, 7, 3, 6
    fe, shape = D.frames(b, t, (7, 2), 3)
    dev = dict(device="cuda")
    fe_d, lens_d = fe.cuda(), shape[:, 1].int().cuda()
    bos = D.weights(g)["model.task_id_to_token_id"][:b].int().cuda()
    o = dict(best_preds=torch.full((b, maxp), -7, dtype=torch.int32, **dev), best_lp=torch.full((b,), -7.0, **dev),
             mult_preds=torch.full((b, beam, maxp), -7, dtype=torch.int32, **dev), mult_lp=torch.full((b, beam), -7.0, **dev),
             sizes=torch.full((2,), -7, dtype=torch.int32, **dev))
    need = int(eng.lib.conette_decode_ensemble_workspace_bytes(eng._ctx_dec, b, t, beam, maxp))
    assert need > int(eng.lib.conette_decode_workspace_bytes(eng._ctx_dec, b, t, beam, maxp)) > 0
    ws = [torch.empty(max(need, int(engv.lib.conette_decode_ensemble_workspace_bytes(engv._ctx_dec, b, t, beam, maxp))) + 256, dtype=torch.uint8, **dev)
          for _ in range(5)]
    for args in ((0, t, beam, maxp), (b, 0, beam, maxp), (b, t, 0, maxp), (b, t, 17, maxp), (b, t, beam, 0)):
        assert eng.lib.conette_decode_ensemble_workspace_bytes(eng._ctx_dec, *args) == 0

    def member(e=eng, fe_=fe_d, bos_=bos, w=0.5, ws_=ws[0], nbytes=None):
        return dict(ctx=e._ctx_dec if e is not None else None, fe=fe_, bos=bos_, w=w, ws=ws_, nbytes=ws_.numel() if nbytes is None and ws_ is not None else (nbytes or 0))

    def raw(members, combine=0, **kw):
        a = dict(lens=lens_d, b=b, t=t, beam=beam, min_pred=0, maxp=maxp, **o)
        a.update(kw)
        p = lambda x: C.c_void_p(0 if x is None else x.data_ptr())
        recs = (ConetteMemberC * max(1, len(members)))()
        for i, m in enumerate(members):
            recs[i] = ConetteMemberC(m["ctx"], 0 if m["fe"] is None else m["fe"].data_ptr(), 0 if m["bos"] is None else m["bos"].data_ptr(),
                                     m["w"], 0 if m["ws"] is None else m["ws"].data_ptr(), m["nbytes"])
        return eng.lib.conette_decode_ensemble(recs, len(members), combine, p(a["lens"]), p(None), a["b"], a["t"], a["beam"], a["min_pred"],
                                               a["maxp"], p(a["best_preds"]), p(a["best_lp"]), p(a["mult_preds"]), p(a["mult_lp"]),
                                               p(a["sizes"]), p(None), p(None), p(None), p(None),
                                               C.c_void_p(torch.cuda.current_stream().cuda_stream))

    two = [member(), member(ws_=ws[1])]
    bad = [(dict(members=[]), "n_members"), (dict(members=[member(ws_=ws[i]) for i in range(5)]), "n_members"),
           (dict(members=two, combine=2), "combine"),
           (dict(members=[member(), member(e=None, ws_=ws[1])]), "members[1].ctx"), (dict(members=[member(fe_=None), two[1]]), "members[0].frame_embs"),
           (dict(members=[member(), member(bos_=None, ws_=ws[1])]), "members[1].bos_ids"), (dict(members=[member(), member(ws_=None)]), "members[1].workspace"),
           (dict(members=[member(), member(e=engv, ws_=ws[1])]), "vocab_size"), (dict(members=[member(), member(e=eng32, ws_=ws[1])]), "precision"),
           (dict(members=[member(), member(w=0.0, ws_=ws[1])]), "members[1].weight"), (dict(members=[member(w=-0.5), two[1]]), "members[0].weight"),
           (dict(members=[member(), member(w=float("nan"), ws_=ws[1])]), "members[1].weight"),
           (dict(members=[member(), member(w=float("inf"), ws_=ws[1])]), "members[1].weight"),
           (dict(members=[member(), member(ws_=ws[1], nbytes=need - 1)]), "workspace"), (dict(members=[member(), member()]), "members[1].workspace overlaps members[0]"),
           (dict(members=[member(), member(ws_=ws[1]), member(ws_=ws[1][64:], nbytes=ws[1].numel() - 64)]), "members[2].workspace overlaps members[1]"),
           (dict(members=two, maxp=65), "max_pred"),
           (dict(members=two, beam=17), "beam"), (dict(members=two, min_pred=-1), "min_pred"), (dict(members=two, lens=None), "bad argument"),
           (dict(members=two, mult_preds=None), "bad argument")]
    for change, word in bad:
        st = raw(**change)
        msg = eng.lib.conette_last_error().decode()
        assert st != 0 and "decode_ensemble" in msg and word in msg, (word, st, msg)
    torch.cuda.synchronize()
    for k, x in o.items():      # nothing was launched: the outputs are untouched
        assert bool((x == -7).all()), k
    assert raw(two) == 0, eng.lib.conette_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(o["mult_lp"]).all()) and int(o["sizes"][0]) >= 1
    with pytest.raises(ValueError, match="n_members"):
        eng.decode_ensemble([], lens_d, None, beam, 0, maxp)
    with pytest.raises(ValueError, match="weights"):
        eng.decode_ensemble([(eng, fe_d, bos, 1.0), (eng, fe_d, bos, -1.0)], lens_d, None, beam, 0, maxp)
    with pytest.raises(ValueError, match="combine"):
        eng.decode_ensemble([(eng, fe_d, bos, 1.0)], lens_d, None, beam, 0, maxp, combine="mean")
    with pytest.raises(ValueError, match="vocabulary"):
        eng.decode_ensemble([(eng, fe_d, bos, 1.0), (engv, fe_d, bos, 1.0)], lens_d, None, beam, 0, maxp)
    with pytest.raises(ValueError, match="precision"):
        eng.decode_ensemble([(eng, fe_d, bos, 1.0), (eng32, fe_d, bos, 1.0)], lens_d, None, beam, 0, maxp)
    D.drop_weights(g)
    D.drop_weights(other)
