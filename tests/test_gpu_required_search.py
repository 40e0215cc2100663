"""GPU: conette_decode_required / Engine.decode_required -- the constrained beam search with words every caption must hold
(csrc/dec_require.h).

Decoder-only engines on the weights of tests/decoder_geometry.py in fp32, exact, bf16 and f16; the cases are the table of
tests/require_cases.py (its docstring lists what they cover; tests/test_cpu_required_search.py holds them to their input
conditions).

1. REPLAY.  Every call of every case is recomputed in float64 (required_search.decide) from the library's own step logits and
   trace.  The number of picks and each pick's bank are exact always (integers decide them); where the call's float64 effective
   margin exceeds DELTA (tests/test_gpu_sample.py, 1.2e-5) the picks -- parents, tokens, order -- are identical; the carried sums
   are within 2e-4 * (step + 1) of their float64 accumulation; every slot, length, out_sizes and best_* is recomputed from the
   trace.  Calls at or below DELTA are counted: none in fp32 and exact, at most 1 % in bf16 and f16.
2. END TO END against the restatement on the oracle's logits, fp32 and exact: picks identical, scores within 1e-4.
3. IDENTITIES, bit for bit, all four precisions, every output and the trace: req_width == 0 == conette_decode_constrained;
   requirements every clip's prefix already meets == conette_decode_constrained with that prefix (the groups are the first
   min(plen, min_pred) prefix tokens: met before the EOS floor ends, so that M4 masks nothing the floor does not); the G = 0 clips
   of a ragged batch == the constrained search's clips.
4. PROPERTY, every precision: every non-void hypothesis holds a token of every group of its clip and ends in <eos> or at max_pred;
   no <eos> before the last group is met.
5. SHORTAGE.  A ban mask that leaves <eos>, two words and one required word at beam 4, through the C ABI into canary-padded
   outputs: the void slots are the restatement's.
6. STATE INDEPENDENCE: a clip alone equals the clip in its batch; a zeroed workspace, a 0xFF workspace, a repeated call and
   capture + replay are bit-equal.
7. C ABI errors name the argument, launch nothing and leave the outputs untouched."""
import ctypes as C
import gc
import os

import numpy as np
import pytest
import torch

from conette_amd import group_search as GS
from conette_amd import required_search as RS
from tests import decoder_geometry as D
from tests import require_cases as RC
from tests.test_gpu_sample import DELTA

pytestmark = pytest.mark.gpu

PRECS = D.PRECISIONS
EXACT = ("fp32", "exact")
KEYS = ("best_preds", "best_lprobs", "mult_preds", "mult_lprobs", "sizes")
TRACE = ("trace_sel", "trace_val")
_DEFAULT = object()


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _cpu(o):
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in o.items()}


def _np(x):
    return None if x is None else x.numpy()


class _Geo:
    def __init__(self, g):
        self.g, self.engines, self.cache = g, {}, {}
        torch.set_num_threads(min(16, os.cpu_count() or 1))

    def engine(self, prec):
        if prec not in self.engines:
            from conette_amd.engine import Engine
            self.engines[prec] = Engine(D.weights(self.g), precision=prec, n_layers=self.g.n_layers, d_ff=self.g.d_ff)
        return self.engines[prec]

    def _args(self, c):
        fe, shape, bos, fb, table, lens = RC.inputs(c)
        prefix, plens = (table, lens) if table.shape[1] > 0 else (None, None)
        return fe.cuda(), shape[:, 1].int(), bos, fb, prefix, plens

    def run(self, prec, c, tag=None, tables=_DEFAULT):
        """decode_required on the case (tag None), or with other requirement tables (tag: the cache key of the variant)"""
        key = (prec, c.name, tag)
        if key not in self.cache:
            fe, lens, bos, fb, prefix, plens = self._args(c)
            rt, rg = RC.tables(c) if tables is _DEFAULT else tables
            out = self.engine(prec).decode_required(fe, lens, bos, fb, c.w, c.min_pred, c.max_pred, prefix=prefix, prefix_lens=plens,
                                                    ban_mask=RC.ban_mask(c), no_repeat_ngram=c.n, req_tokens=rt, req_groups=rg,
                                                    want_trace=True, want_logits=tag is None, check=False)
            self.cache[key] = _cpu(out)
        return self.cache[key]

    def constrained(self, prec, c):
        """conette_decode_constrained on the case's inputs"""
        key = (prec, c.name, "constrained")
        if key not in self.cache:
            fe, lens, bos, fb, prefix, plens = self._args(c)
            self.cache[key] = _cpu(self.engine(prec).decode_constrained(fe, lens, bos, fb, c.w, c.min_pred, c.max_pred, prefix=prefix,
                                                                        prefix_lens=plens, ban_mask=RC.ban_mask(c), no_repeat_ngram=c.n,
                                                                        want_trace=True, check=False))
        return self.cache[key]


@pytest.fixture(scope="module", params=RC.GEOS)
def geo(request):
    h = _Geo(D.geometry(request.param))
    yield h
    h.engines.clear()
    h.cache.clear()
    RC.drop_runs()
    D.drop_weights(h.g)
    gc.collect()
    torch.cuda.empty_cache()


# ---- 1. replay -------------------------------------------------------------------------------------------------------------------------
def replay(out, bos, w, v, min_pred, max_pred, prefixes, required, forbid=None, ban=None, n=0, what=""):
    """Walks the device's trace; returns (free calls, free calls at or below DELTA, of those the ones whose picks differ, void slots)."""
    sel, val, logits = out["trace_sel"].numpy(), out["trace_val"].numpy(), out["step_logits"].numpy()
    b_n = len(bos)
    clips = [{"rows": [{"prefix": [int(bos[b])], "sum": 0.0, "sum64": 0.0}], "k": w, "slots": list(range(w))} for b in range(b_n)]
    out_preds = np.zeros((b_n, w, max_pred), dtype=np.int64)
    out_avg = np.zeros((b_n, w), dtype=np.float32)
    out_len = np.zeros((b_n, w), dtype=np.int64)
    n_calls = n_close = n_close_differ = 0
    for step in range(max_pred):
        for b in range(b_n):
            cl, groups = clips[b], required[b]
            rows, k, slots = cl["rows"], cl["k"], cl["slots"]
            got = sel[step, b]
            tag = (what, "step", step, "clip", b)
            if not rows:
                assert (got == -1).all(), tag
                continue
            seqs, sums = [r["prefix"] for r in rows], [r["sum"] for r in rows]
            z = logits[step, b * w: b * w + len(rows)]
            lp64 = lambda p, t: float(RS.log_softmax(RS.masked_row(z[p], seqs[p], step, min_pred, max_pred, RC.EOS, forbid, ban, n, groups))[t])
            if step < len(prefixes[b]):
                t = prefixes[b][step]
                d = RS.decide(z, seqs, sums, k, step, min_pred, max_pred, RC.EOS, forbid, ban, n, groups, forced_token=t)
                if d["void"]:
                    assert (got == -1).all(), tag
                    out_avg[b, :] = -np.inf
                    cl["rows"], cl["k"] = [], 0
                    continue
                assert got[0].tolist() == [0, t] and (got[1:] == -1).all(), (tag, got.tolist())
                m, m64 = float(val[step, b, 0]), rows[0]["sum64"] + lp64(0, t)
                assert abs(m - m64) <= 2e-4 * (step + 1), (tag, m, m64)
                cl["rows"] = [{"prefix": seqs[0] + [t], "sum": m, "sum64": m64}]
                continue
            d = RS.decide(z, seqs, sums, k, step, min_pred, max_pred, RC.EOS, forbid, ban, n, groups)
            f = len(d["tokens"])
            assert (got[f:] == -1).all() and (got[:f] >= 0).all(), (tag, f, got.tolist())
            got_par, got_tok = got[:f, 0].tolist(), got[:f, 1].tolist()
            assert all(0 <= p < len(rows) for p in got_par) and all(0 <= t < v for t in got_tok), tag
            got_banks = [sum(RS.met_groups(seqs[p], groups)) + int(t in RS.unmet_tokens(seqs[p], groups)) for p, t in zip(got_par, got_tok)]
            assert got_banks == d["banks"], (tag, got_banks, d["banks"])
            assert len(set(zip(got_par, got_tok))) == f, (tag, got.tolist())
            n_calls += 1
            if d["margin"] > DELTA:
                assert (d["parents"], d["tokens"]) == (got_par, got_tok), (tag, d, got.tolist())
            else:
                n_close += 1
                n_close_differ += (d["parents"], d["tokens"]) != (got_par, got_tok)
            nxt, nslots = [], []
            for j in range(f):      # the state goes on with the device's picks
                parent, token, m = got_par[j], got_tok[j], float(val[step, b, j])
                m64 = rows[parent]["sum64"] + lp64(parent, token)
                assert abs(m - m64) <= 2e-4 * (step + 1), (tag, j, m, m64)
                seq = seqs[parent] + [token]
                if token == RC.EOS or step == max_pred - 1:
                    out_preds[b, slots[j], :step + 1] = seq[1:]
                    out_avg[b, slots[j]] = np.float32(m) / np.float32(step + 1)
                    out_len[b, slots[j]] = step + 1
                else:
                    nxt.append({"prefix": seq, "sum": m, "sum64": m64})
                    nslots.append(slots[j])
            for j in range(f, k):
                out_avg[b, slots[j]] = -np.inf
            cl["rows"], cl["k"], cl["slots"] = nxt, len(nxt), nslots
    assert all(not cl["rows"] for cl in clips), what
    assert out["mult_preds"].tolist() == out_preds.tolist(), what
    assert np.array_equal(out["mult_lprobs"].numpy().view(np.int32), out_avg.view(np.int32)), what
    best_preds, best_lp, sizes = GS.finalize(out_preds, out_avg, out_len, RC.EOS)
    assert out["sizes"].tolist() == sizes, (what, out["sizes"].tolist(), sizes)
    assert out["best_preds"].tolist() == best_preds.tolist(), what
    assert np.array_equal(out["best_lprobs"].numpy().view(np.int32), best_lp.view(np.int32)), what
    return n_calls, n_close, n_close_differ, int((out_len == 0).sum())


@pytest.mark.parametrize("prec", PRECS)
def test_every_call_replays_in_float64(prec, geo):
    total = close = differ = 0
    for c in RC.cases(geo.g.name):
        _, _, bos, forbid = RC.inputs(c)[:4]
        n, nc, nd, void = replay(geo.run(prec, c), bos.tolist(), c.w, geo.g.v, c.min_pred, c.max_pred, RC.prefixes(c), RC.requirements(c),
                                 _np(forbid), _np(RC.ban_mask(c)), c.n, (c, prec))
        total, close, differ = total + n, close + nc, differ + nd
        print(f"required replay {prec} {c}: {n} free calls, {nc} at or below DELTA = {DELTA} ({nd} of them picked otherwise), {void} void slots")
    print(f"required replay {(geo.g.name, prec)}: {close} of {total} calls at or below DELTA ({close / total:.4%})")
    assert total > 0
    if prec in EXACT:
        assert close == 0, (geo.g.name, prec, close, total)
    else:
        assert close <= 0.01 * total, (geo.g.name, prec, close, total)


# ---- 2. end to end against the restatement on the oracle's logits -----------------------------------------------------------------
@pytest.mark.parametrize("prec", EXACT)
def test_end_to_end_equals_the_restatement(prec, geo):
    for c in RC.cases(geo.g.name):
        out, ref = geo.run(prec, c), RC.oracle_run(c)
        sel = out["trace_sel"].numpy()
        seen = np.zeros(sel.shape[:3], dtype=bool)
        for call in ref["calls"]:
            s, b, f = call["step"], call["clip"], len(call["tokens"])
            assert sel[s, b, :f, 0].tolist() == call["parents"] and sel[s, b, :f, 1].tolist() == call["tokens"], (c, prec, s, b)
            seen[s, b, :f] = True
        assert (sel[~seen] == -1).all(), (c, prec)
        assert out["mult_preds"].tolist() == ref["mult_preds"].tolist() and out["best_preds"].tolist() == ref["best_preds"].tolist(), (c, prec)
        assert out["sizes"].tolist() == ref["sizes"], (c, prec)
        got, want = out["mult_lprobs"].numpy().astype(np.float64), ref["mult_lprobs"]
        assert np.array_equal(np.isfinite(got), np.isfinite(want)), (c, prec)
        fin = np.isfinite(want)
        worst = max(float(np.abs(got[fin] - want[fin]).max()), float(np.abs(out["best_lprobs"].numpy() - ref["best_lprobs"]).max()))
        print(f"required end to end {prec} {c}: {len(ref['calls'])} calls, max |d score| {worst:.3e}")
        assert worst <= 1e-4, (c, prec, worst)


# ---- 3. identities with the constrained search ----------------------------------------------------------------------------------------------
def _empty(b):
    return torch.zeros((b, 0), dtype=torch.int32), torch.zeros((b, 0), dtype=torch.int32)


@pytest.mark.parametrize("prec", PRECS)
def test_width_zero_equals_the_constrained_search(prec, geo):
    for c in RC.cases(geo.g.name):
        con, free = geo.constrained(prec, c), geo.run(prec, c, "width 0", tables=_empty(c.b))
        for k in KEYS + TRACE:
            assert torch.equal(_bits(free[k]), _bits(con[k])), (c, prec, k)


@pytest.mark.parametrize("prec", PRECS)
def test_requirements_the_prefix_meets_equal_the_constrained_search(prec, geo):
    done = 0
    for c in RC.cases(geo.g.name):
        pre = RC.prefixes(c)
        groups = [[[t] for t in p[: min(len(p), c.min_pred, RS.MAX_GROUPS)]] for p in pre]
        if not any(groups):
            continue
        rt, rg = RS.pack_tables(groups)
        con = geo.constrained(prec, c)
        met = geo.run(prec, c, "met by the prefix", tables=(torch.from_numpy(rt), torch.from_numpy(rg)))
        for k in KEYS + TRACE:
            assert torch.equal(_bits(met[k]), _bits(con[k])), (c, prec, k)
        done += 1
    assert done > 0


@pytest.mark.parametrize("prec", PRECS)
def test_clips_without_requirements_equal_the_constrained_searchs_clips(prec, geo):
    done = 0
    for c in RC.cases(geo.g.name):
        if 0 not in c.gs:
            continue
        con, req = geo.constrained(prec, c), geo.run(prec, c)
        for i, g_n in enumerate(c.gs):
            if g_n:
                continue
            for k in ("best_preds", "best_lprobs", "mult_preds", "mult_lprobs"):
                assert torch.equal(_bits(req[k][i]), _bits(con[k][i])), (c, prec, i, k)
            for k in TRACE:
                assert torch.equal(_bits(req[k][:, i]), _bits(con[k][:, i])), (c, prec, i, k)
            done += 1
    assert done > 0


# ---- 4. property ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_hypotheses_hold_every_required_group(prec, geo):
    seen = 0
    for c in RC.cases(geo.g.name):
        out, req, bos = geo.run(prec, c), RC.requirements(c), RC.inputs(c)[2].tolist()
        for b in range(c.b):
            for s in range(c.w):
                r = out["mult_preds"][b, s].tolist()
                if not bool(torch.isfinite(out["mult_lprobs"][b, s])):
                    assert all(t == RC.PAD for t in r), (c, prec, b, s)
                    continue
                toks = r[: r.index(RC.EOS) + 1] if RC.EOS in r else r
                assert toks[-1] == RC.EOS or len(toks) == c.max_pred, (c, prec, b, s, toks)
                assert all(RS.met_groups([bos[b]] + toks, req[b])), (c, prec, b, s, toks, req[b])
                if RC.EOS in toks:      # no <eos> before the last group is met
                    assert all(RS.met_groups([bos[b]] + toks[: toks.index(RC.EOS)], req[b])), (c, prec, b, s, toks)
                seen += 1
    assert seen > 0


# ---- 5. candidate shortage, through the C ABI into canary-padded outputs ------------------------------------------------------------------
CANARY = -7


class _Raw:
    """conette_decode_required called directly; every output lies between two canary blocks of 64 elements"""

    def __init__(self, eng, b, t, w, maxp, v, logits=True):
        self.eng, self.dims = eng, (b, t, w, maxp)
        shapes = {"best_preds": ((b, maxp), torch.int32), "best_lp": ((b,), torch.float32), "mult_preds": ((b, w, maxp), torch.int32),
                  "mult_lp": ((b, w), torch.float32), "sizes": ((2,), torch.int32), "trace_sel": ((maxp, b, w, 2), torch.int32),
                  "trace_val": ((maxp, b, w), torch.float32)}
        if logits:
            shapes["step_logits"] = ((maxp, b * w, v), torch.float32)
        self.whole, self.o = {}, {}
        for k, (shape, dt) in shapes.items():
            n = int(np.prod(shape))
            self.whole[k] = torch.full((n + 128,), CANARY, dtype=dt, device="cuda")
            self.o[k] = self.whole[k][64:64 + n].view(shape)
        self.need = int(eng.lib.conette_decode_required_workspace_bytes(eng._ctx_dec, b, t, w, maxp))
        self.ws = torch.empty(self.need, dtype=torch.uint8, device="cuda")

    def call(self, fe, lens, bos, forbid=None, prefix=None, plens=None, pw=0, ban=None, n=0, rt=None, rg=None, rw=0, min_pred=0, change=None):
        b, t, w, maxp = self.dims
        a = dict(fe=fe, lens=lens, bos=bos, forbid=forbid, prefix=prefix, plens=plens, pw=pw, ban=ban, n=n, rt=rt, rg=rg, rw=rw, b=b, t=t,
                 w=w, min_pred=min_pred, maxp=maxp, ws=self.ws, ws_bytes=self.need, **self.o)
        a.update(change or {})
        p = lambda x: C.c_void_p(0 if x is None else x.data_ptr())
        return self.eng.lib.conette_decode_required(
            self.eng._ctx_dec, p(a["fe"]), p(a["lens"]), p(a["bos"]), p(a["forbid"]), p(a["prefix"]), p(a["plens"]), a["pw"], p(a["ban"]),
            a["n"], p(a["rt"]), p(a["rg"]), a["rw"], a["b"], a["t"], a["w"], a["min_pred"], a["maxp"], p(a["best_preds"]), p(a["best_lp"]),
            p(a["mult_preds"]), p(a["mult_lp"]), p(a["sizes"]), p(a["trace_sel"]), p(a["trace_val"]), p(a.get("step_logits")), p(a["ws"]),
            a["ws_bytes"], C.c_void_p(torch.cuda.current_stream().cuda_stream))

    def canaries_intact(self):
        torch.cuda.synchronize()
        return all(bool((x[:64] == CANARY).all()) and bool((x[-64:] == CANARY).all()) for x in self.whole.values())

    def outputs(self):
        torch.cuda.synchronize()
        names = {"best_lp": "best_lprobs", "mult_lp": "mult_lprobs"}
        return {names.get(k, k): v.cpu().clone() for k, v in self.o.items()}


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("gname", ("v31_ff32_l2", "v2049_ff256_l6", "v8193_ff4096_l2"))
def test_candidate_shortage_gives_the_restatements_void_slots(prec, gname):
    from conette_amd.engine import Engine
    g = D.geometry(gname)
    try:
        eng = Engine(D.weights(g), precision=prec, n_layers=g.n_layers, d_ff=g.d_ff)
        b, t, w, maxp = 3, 8, 4, 6
        fe, shape = D.frames(b, t, (8, 7, 1), 11)
        fe_d, lens_d = fe.cuda(), shape[:, 1].int().cuda()
        bos = D.weights(g)["model.task_id_to_token_id"][:b].int()
        words, req_word = (D.N_SPECIALS_AND_TASKS + 1, g.v - 1), D.N_SPECIALS_AND_TASKS + 3
        ban = torch.ones(g.v, dtype=torch.uint8)
        ban[[RC.EOS, *words, req_word]] = 0
        required = [[[req_word]], [], [[req_word]]]          # the clip in the middle has no requirement
        rt, rg = RS.pack_tables(required, 3, [[2, 0, 1]] * b)
        raw = _Raw(eng, b, t, w, maxp, g.v)
        assert raw.call(fe_d, lens_d, bos.cuda(), ban=ban.cuda(), rt=torch.from_numpy(rt).cuda(), rg=torch.from_numpy(rg).cuda(), rw=3) == 0, \
            eng.lib.conette_last_error()
        assert raw.canaries_intact()
        out = raw.outputs()
        _, _, _, void = replay(out, bos.tolist(), w, g.v, 0, maxp, [[]] * b, required, None, ban.bool().numpy(), 0, (gname, prec, "shortage"))
        # step 0 offers three candidates (<eos> is masked while the word is missing) or four: a void slot per clip with a requirement
        assert void >= 2 and int((~torch.isfinite(out["mult_lprobs"])).sum()) == void
        assert bool(torch.isfinite(out["best_lprobs"]).all())
        for i in (0, 2):
            for s in range(w):
                if bool(torch.isfinite(out["mult_lprobs"][i, s])):
                    assert req_word in out["mult_preds"][i, s].tolist(), (gname, prec, i, s)
    finally:
        D.drop_weights(g)


# ---- 6. state independence ---------------------------------------------------------------------------------------------------------------
def _det_case(geo):
    return next(c for c in RC.cases(geo.g.name) if c.b > 1 and max(c.gs) > 0)


@pytest.mark.parametrize("prec", PRECS)
def test_clip_alone_equals_clip_in_batch(prec, geo):
    c = _det_case(geo)
    eng = geo.engine(prec)
    fe, shape, bos, forbid, table, plens = RC.inputs(c)
    lens = shape[:, 1].int()
    rt, rg = RC.tables(c)
    full = geo.run(prec, c)
    for i in range(c.b):
        one = _cpu(eng.decode_required(fe[i:i + 1].cuda(), lens[i:i + 1], bos[i:i + 1], forbid, c.w, c.min_pred, c.max_pred,
                                       prefix=table[i:i + 1], prefix_lens=plens[i:i + 1], ban_mask=RC.ban_mask(c), no_repeat_ngram=c.n,
                                       req_tokens=rt[i:i + 1], req_groups=rg[i:i + 1], want_trace=True))
        for k in ("best_preds", "best_lprobs", "mult_preds", "mult_lprobs"):
            assert torch.equal(_bits(one[k][0]), _bits(full[k][i])), (c, prec, i, k)
        assert torch.equal(one["trace_sel"][:, 0], full["trace_sel"][:, i]), (c, prec, i)
        assert torch.equal(_bits(one["trace_val"][:, 0]), _bits(full["trace_val"][:, i])), (c, prec, i)


@pytest.mark.parametrize("prec", PRECS)
def test_identical_calls_stale_workspace_and_graph_replay_are_bit_equal(prec, geo):
    c = _det_case(geo)
    eng = geo.engine(prec)
    fe, shape, bos, forbid, table, plens = RC.inputs(c)
    fe_d, lens_d, bos_d = fe.cuda(), shape[:, 1].int().cuda(), bos.int().cuda()
    fb_d = None if forbid is None else forbid.to(torch.uint8).cuda()
    ban = RC.ban_mask(c)
    ban_d = None if ban is None else ban.to(torch.uint8).cuda()
    pre_d, plens_d = table.int().cuda(), plens.int().cuda()
    rt_d, rg_d = (x.cuda() for x in RC.tables(c))
    call = lambda: eng.decode_required(fe_d, lens_d, bos_d, fb_d, c.w, c.min_pred, c.max_pred, prefix=pre_d, prefix_lens=plens_d,
                                       ban_mask=ban_d, no_repeat_ngram=c.n, req_tokens=rt_d, req_groups=rg_d, want_trace=True, check=False)
    first = _cpu(call())
    for k in first:
        assert torch.equal(_bits(first[k]), _bits(geo.run(prec, c)[k])), (c, prec, "the cached run", k)
    for ws in eng._ws.values():
        ws.zero_()
    second = _cpu(call())
    for ws in eng._ws.values():
        ws.fill_(0xFF)
    third = _cpu(call())
    fourth = _cpu(call())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = call()
    for x in held.values():
        x.view(torch.uint8).fill_(0xFF)
    graph.replay()
    replayed = _cpu(held)
    for what, o in (("zeroed workspace", second), ("0xFF workspace", third), ("repeated call", fourth), ("capture + replay", replayed)):
        for k in first:
            assert torch.equal(_bits(first[k]), _bits(o[k])), (c, prec, what, k)
    del graph, held


# ---- 7. C ABI errors -----------------------------------------------------------------------------------------------------------------------
def test_c_abi_errors():
    from conette_amd.engine import Engine
    g = D.geometry("v31_ff32_l2")
    eng = Engine(D.weights(g), precision="bf16", n_layers=g.n_layers, d_ff=g.d_ff)
    b, t, w, maxp = 2, 7, 3, 6
    fe, shape = D.frames(b, t, (7, 2), 3)
    fe_d, lens_d = fe.cuda(), shape[:, 1].int().cuda()
    bos = D.weights(g)["model.task_id_to_token_id"][:b].int().cuda()
    raw = _Raw(eng, b, t, w, maxp, g.v, logits=False)
    assert raw.need == int(eng.lib.conette_decode_workspace_bytes(eng._ctx_dec, b, t, w, maxp)) > 0
    prefix = torch.full((b, 2), 12, dtype=torch.int32, device="cuda")
    plens = torch.ones(b, dtype=torch.int32, device="cuda")
    rt = torch.full((b, 2), 14, dtype=torch.int32, device="cuda")
    rt[:, 1] = 15
    rg = torch.as_tensor([[0, 1], [0, -1]], dtype=torch.int32, device="cuda")
    wide = torch.zeros((b, 33), dtype=torch.int32, device="cuda")
    g8, gm2 = rg.clone(), rg.clone()
    g8[1, 0], gm2[0, 1] = 8, -2
    bad = [({"w": 0}, "beam"), ({"w": 17}, "beam"), ({"n": -1}, "no_repeat_ngram"), ({"n": 65}, "no_repeat_ngram"),
           ({"pw": -1}, "prefix_width"), ({"pw": maxp, "prefix": prefix, "plens": plens}, "prefix_width"),
           ({"pw": 2, "prefix": None, "plens": plens}, "prefix"), ({"pw": 2, "prefix": prefix, "plens": None}, "prefix_lens"),
           ({"ws_bytes": raw.need - 1}, "workspace"), ({"maxp": 65}, "max_pred"), ({"min_pred": -1}, "min_pred"),
           ({"fe": None}, "decode_required"), ({"mult_preds": None}, "decode_required"),
           ({"rw": 33, "rt": wide, "rg": wide}, "req_width"), ({"rw": -1}, "req_width"),
           ({"rw": 2, "rt": None, "rg": rg}, "req_tokens"), ({"rw": 2, "rt": rt, "rg": None}, "req_groups"),
           ({"rw": 2, "rt": rt, "rg": g8}, "req_groups[1][0]=8"), ({"rw": 2, "rt": rt, "rg": gm2}, "req_groups[0][1]=-2")]
    for change, word in bad:
        st = raw.call(fe_d, lens_d, bos, change=change)
        msg = eng.lib.conette_last_error().decode()
        assert st != 0 and "decode_required" in msg and word in msg, (change, st, msg)
    torch.cuda.synchronize()
    for k, x in raw.whole.items():      # nothing was launched: the outputs are untouched
        assert bool((x == CANARY).all()), k
    for args in ((0, t, w, maxp), (b, t, 0, maxp), (b, t, 17, maxp), (b, t, w, 0)):
        assert eng.lib.conette_decode_required_workspace_bytes(eng._ctx_dec, *args) == 0
    assert raw.call(fe_d, lens_d, bos, prefix=prefix, plens=plens, pw=2, n=2, rt=rt, rg=rg, rw=2) == 0, eng.lib.conette_last_error()
    assert raw.canaries_intact()
    out = raw.outputs()
    assert bool(torch.isfinite(out["mult_lprobs"]).all()) and int(out["sizes"][0]) >= 1
    assert bool((out["mult_preds"][:, :, 0] == 12).all())
    assert all(14 in r for r in out["mult_preds"].reshape(-1, maxp).tolist()) and all(15 in r for r in out["mult_preds"][0].tolist())
    with pytest.raises(ValueError, match="beam"):
        eng.decode_required(fe_d, lens_d, bos, None, 17, 0, maxp)
    with pytest.raises(ValueError, match="req_width"):
        eng.decode_required(fe_d, lens_d, bos, None, 3, 0, maxp, req_tokens=wide, req_groups=wide)
    with pytest.raises(ValueError, match="req_groups"):
        eng.decode_required(fe_d, lens_d, bos, None, 3, 0, maxp, req_tokens=rt, req_groups=g8)
    with pytest.raises(ValueError, match="together"):
        eng.decode_required(fe_d, lens_d, bos, None, 3, 0, maxp, req_tokens=rt)
    with pytest.raises(ValueError, match="<eos>"):
        eng.decode_required(fe_d, lens_d, bos, None, 3, 0, maxp, req_tokens=torch.full((b, 1), RC.EOS), req_groups=torch.zeros((b, 1)))
    with pytest.raises(ValueError, match="do not fit"):
        eng.decode_required(fe_d, lens_d, bos, None, 3, 0, 2, req_tokens=torch.as_tensor([[14, 15, 16]] * b), req_groups=torch.as_tensor([[0, 1, 2]] * b))
    D.drop_weights(g)
