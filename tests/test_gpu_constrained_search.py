"""GPU: conette_decode_constrained / Engine.decode_constrained -- beam search with a forced prefix, a ban mask and an n-gram ban
(csrc/dec_constrain.h).

Decoder-only engines on the weights of tests/decoder_geometry.py in fp32, exact, bf16 and f16; the cases are the table of
tests/constrain_cases.py (its docstring lists what they cover; tests/test_cpu_constrained_search.py holds them to their input
conditions).

1. REPLAY.  Every call of every case is recomputed in float64 (constrained_search.decide) from the library's own step logits and
   trace.  Forced calls: token and parent exact.  Free calls: the number of picks is exact (which candidates are finite is decided
   by the masks alone), and where the call's float64 effective margin exceeds DELTA (tests/test_gpu_sample.py, 1.2e-5) the picks --
   parents, tokens, order -- are identical; the carried sums are within 2e-4 * (step + 1) of their float64 accumulation; every
   slot, length, out_sizes and best_* is recomputed from the trace.  Calls at or below DELTA are counted: none in fp32 and exact
   (the CPU-checked 2e-3 margin of the oracle's run guarantees it), at most 1 % in bf16 and f16.
2. END TO END against the restatement on the oracle's logits, fp32 and exact: picks identical, scores (mult_lprobs, best_lprobs)
   within 1e-4, carried sums within the replay's 2e-4 * (step + 1) (a random prefix makes them large: down to -500 over 62 tokens).
3. IDENTITIES, bit for bit, all four precisions: no constraints == conette_decode in every output and in the trace; the clips with
   an empty prefix of a ragged batch == conette_decode's clips; beam 1 with the prefix taken from conette_decode's own beam-1
   caption == that caption and score; n = 1 == conette_decode with an all-ones forbid mask; an all-zero ban mask and n = 64 ==
   the unconstrained call.
4. PROPERTIES, every precision: every hypothesis starts with its prefix, holds no banned token, and (with the task token in front)
   no n-gram twice.
5. SHORTAGE.  A ban mask that leaves <eos> and two words at beam 4 and min_pred 0 gives the void slots the restatement gives; a
   forced banned token voids its clip; both through the C ABI into canary-padded outputs.
6. SCORES ARE THE MODEL'S: masks off, prefixes on, |mult_lprobs - rescored mean| <= test_gpu_score.CONSISTENCY.
7. STATE INDEPENDENCE: a clip alone equals the clip in its batch; a 0xFF-filled workspace, a repeated call and capture + replay
   are bit-equal.
8. C ABI errors name the argument, launch nothing and leave the outputs untouched."""
import ctypes as C
import gc
import os

import numpy as np
import pytest
import torch

from conette_amd import constrained_search as CS
from conette_amd import group_search as GS
from tests import constrain_cases as CC
from tests import decoder_geometry as D
from tests.test_gpu_sample import DELTA
from tests.test_gpu_score import CONSISTENCY

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


class _Geo:
    def __init__(self, g):
        self.g, self.engines, self.cache = g, {}, {}
        torch.set_num_threads(min(16, os.cpu_count() or 1))

    def engine(self, prec):
        if prec not in self.engines:
            from conette_amd.engine import Engine
            self.engines[prec] = Engine(D.weights(self.g), precision=prec, n_layers=self.g.n_layers, d_ff=self.g.d_ff)
        return self.engines[prec]

    def run(self, prec, c, tag=None, w=None, prefix=_DEFAULT, plens=None, ban=_DEFAULT, n=None, forbid=_DEFAULT, logits=False):
        """the case as the table has it (tag None), or with the given arguments replaced (tag: the cache key of the variant)"""
        key = (prec, c.name, tag)
        if key not in self.cache:
            fe, shape, bos, fb, table, lens = CC.inputs(c)
            if prefix is _DEFAULT:
                prefix, plens = (table, lens) if table.shape[1] > 0 else (None, None)
            out = self.engine(prec).decode_constrained(
                fe.cuda(), shape[:, 1].int(), bos, fb if forbid is _DEFAULT else forbid, c.w if w is None else w, c.min_pred, c.max_pred,
                prefix=prefix, prefix_lens=plens, ban_mask=CC.ban_mask(c) if ban is _DEFAULT else ban,
                no_repeat_ngram=c.n if n is None else n, want_trace=True, want_logits=logits or tag is None, check=False)
            self.cache[key] = _cpu(out)
        return self.cache[key]

    def plain(self, prec, c, w=None, forbid=_DEFAULT):
        """conette_decode on the case's inputs"""
        key = (prec, c.name, "plain", w, forbid is _DEFAULT)
        if key not in self.cache:
            fe, shape, bos, fb = CC.inputs(c)[:4]
            self.cache[key] = _cpu(self.engine(prec).decode(fe.cuda(), shape[:, 1].int(), bos, fb if forbid is _DEFAULT else forbid,
                                                            c.w if w is None else w, c.min_pred, c.max_pred, want_trace=True))
        return self.cache[key]


@pytest.fixture(scope="module", params=CC.GEOS)
def geo(request):
    h = _Geo(D.geometry(request.param))
    yield h
    h.engines.clear()
    h.cache.clear()
    CC.drop_runs()
    D.drop_weights(h.g)
    gc.collect()
    torch.cuda.empty_cache()


# ---- 1. replay -------------------------------------------------------------------------------------------------------------------------
def replay(out, bos, w, v, min_pred, max_pred, prefixes, forbid=None, ban=None, n=0, what=""):
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
            cl = clips[b]
            rows, k, slots = cl["rows"], cl["k"], cl["slots"]
            got = sel[step, b]
            tag = (what, "step", step, "clip", b)
            if not rows:
                assert (got == -1).all(), tag
                continue
            seqs, sums = [r["prefix"] for r in rows], [r["sum"] for r in rows]
            z = logits[step, b * w: b * w + len(rows)]
            if step < len(prefixes[b]):
                t = prefixes[b][step]
                d = CS.decide(z, seqs, sums, k, step, min_pred, CC.EOS, forbid, ban, n, forced_token=t)
                if d["void"]:
                    assert (got == -1).all(), tag
                    out_avg[b, :] = -np.inf
                    cl["rows"], cl["k"] = [], 0
                    continue
                assert got[0].tolist() == [0, t] and (got[1:] == -1).all(), (tag, got.tolist())
                m = float(val[step, b, 0])
                m64 = rows[0]["sum64"] + float(CS.log_softmax(CS.constraint_mask(z[0], seqs[0], step, min_pred, CC.EOS, forbid, ban, n))[t])
                assert abs(m - m64) <= 2e-4 * (step + 1), (tag, m, m64)
                cl["rows"] = [{"prefix": seqs[0] + [t], "sum": m, "sum64": m64}]
                continue
            d = CS.decide(z, seqs, sums, k, step, min_pred, CC.EOS, forbid, ban, n)
            f = len(d["tokens"])
            assert (got[f:] == -1).all() and (got[:f] >= 0).all(), (tag, f, got.tolist())
            got_par, got_tok = got[:f, 0].tolist(), got[:f, 1].tolist()
            assert all(0 <= p < len(rows) for p in got_par) and all(0 <= t < v for t in got_tok), tag
            n_calls += 1
            if d["margin"] > DELTA:
                assert (d["parents"], d["tokens"]) == (got_par, got_tok), (tag, d, got.tolist())
            else:
                n_close += 1
                n_close_differ += (d["parents"], d["tokens"]) != (got_par, got_tok)
            nxt, nslots = [], []
            for j in range(f):      # the state goes on with the device's picks
                parent, token, m = got_par[j], got_tok[j], float(val[step, b, j])
                zm = CS.constraint_mask(z[parent], seqs[parent], step, min_pred, CC.EOS, forbid, ban, n)
                m64 = rows[parent]["sum64"] + float(CS.log_softmax(zm)[token])
                assert abs(m - m64) <= 2e-4 * (step + 1), (tag, j, m, m64)
                seq = seqs[parent] + [token]
                if token == CC.EOS or step == max_pred - 1:
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
    best_preds, best_lp, sizes = GS.finalize(out_preds, out_avg, out_len, CC.EOS)
    assert out["sizes"].tolist() == sizes, (what, out["sizes"].tolist(), sizes)
    assert out["best_preds"].tolist() == best_preds.tolist(), what
    assert np.array_equal(out["best_lprobs"].numpy().view(np.int32), best_lp.view(np.int32)), what
    return n_calls, n_close, n_close_differ, int((out_len == 0).sum())


def _np(x):
    return None if x is None else x.numpy()


@pytest.mark.parametrize("prec", PRECS)
def test_every_call_replays_in_float64(prec, geo):
    total = close = differ = 0
    for c in CC.cases(geo.g.name):
        _, _, bos, forbid = CC.inputs(c)[:4]
        n, nc, nd, void = replay(geo.run(prec, c), bos.tolist(), c.w, geo.g.v, c.min_pred, c.max_pred, CC.prefixes(c), _np(forbid),
                                 _np(CC.ban_mask(c)), c.n, (c, prec))
        total, close, differ = total + n, close + nc, differ + nd
        print(f"constrained replay {prec} {c}: {n} free calls, {nc} at or below DELTA = {DELTA} ({nd} of them picked otherwise), {void} void slots")
    print(f"constrained replay {(geo.g.name, prec)}: {close} of {total} calls at or below DELTA ({close / total:.4%})")
    assert total > 0
    if prec in EXACT:
        assert close == 0, (geo.g.name, prec, close, total)
    else:
        assert close <= 0.01 * total, (geo.g.name, prec, close, total)


# ---- 2. end to end against the restatement on the oracle's logits -----------------------------------------------------------------
@pytest.mark.parametrize("prec", EXACT)
def test_end_to_end_equals_the_restatement(prec, geo):
    for c in CC.cases(geo.g.name):
        out, ref = geo.run(prec, c), CC.oracle_run(c)
        sel, val = out["trace_sel"].numpy(), out["trace_val"].numpy()
        seen = np.zeros(sel.shape[:3], dtype=bool)
        worst_sum = 0.0      # carried sums, in units of the replay's bound 2e-4 * (step + 1)
        for call in ref["calls"]:
            s, b, f = call["step"], call["clip"], len(call["tokens"])
            assert sel[s, b, :f, 0].tolist() == call["parents"] and sel[s, b, :f, 1].tolist() == call["tokens"], (c, prec, s, b)
            if f:
                worst_sum = max(worst_sum, float(np.abs(val[s, b, :f] - np.array(call["sums"])).max()) / (2e-4 * (s + 1)))
            seen[s, b, :f] = True
        assert (sel[~seen] == -1).all(), (c, prec)
        assert out["mult_preds"].tolist() == ref["mult_preds"].tolist() and out["best_preds"].tolist() == ref["best_preds"].tolist(), (c, prec)
        assert out["sizes"].tolist() == ref["sizes"], (c, prec)
        got, want = out["mult_lprobs"].numpy().astype(np.float64), ref["mult_lprobs"]
        assert np.array_equal(np.isfinite(got), np.isfinite(want)), (c, prec)
        fin = np.isfinite(want)
        worst = max(float(np.abs(got[fin] - want[fin]).max()), float(np.abs(out["best_lprobs"].numpy() - ref["best_lprobs"]).max()))
        print(f"constrained end to end {prec} {c}: {len(ref['calls'])} calls, max |d score| {worst:.3e}, "
              f"max |d carried sum| {worst_sum:.3f} of 2e-4 * (step + 1)")
        assert worst <= 1e-4, (c, prec, worst)
        assert worst_sum <= 1.0, (c, prec, worst_sum)


# ---- 3. identities with the pinned search -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_no_constraints_equals_conette_decode(prec, geo):
    for c in CC.cases(geo.g.name):
        plain = geo.plain(prec, c)
        free = geo.run(prec, c, "free", prefix=None, ban=None, n=0)
        for k in KEYS + TRACE:
            assert torch.equal(_bits(free[k]), _bits(plain[k])), (c, prec, k)
        if c.max_pred <= 20:     # an all-zero ban mask and an n no sequence reaches: the unconstrained call
            idle = geo.run(prec, c, "idle", prefix=None, ban=torch.zeros(geo.g.v, dtype=torch.bool), n=64)
            for k in KEYS + TRACE:
                assert torch.equal(_bits(idle[k]), _bits(plain[k])), (c, prec, "idle", k)


@pytest.mark.parametrize("prec", PRECS)
def test_clips_without_a_prefix_equal_conette_decodes_clips(prec, geo):
    done = 0
    for c in CC.cases(geo.g.name):
        if 0 not in c.plens or max(c.plens) == 0:
            continue
        plain, pre = geo.plain(prec, c), geo.run(prec, c, "prefix only", ban=None, n=0)
        for i, p in enumerate(c.plens):
            if p:
                continue
            for k in ("best_preds", "best_lprobs", "mult_preds", "mult_lprobs"):
                assert torch.equal(_bits(pre[k][i]), _bits(plain[k][i])), (c, prec, i, k)
            for k in TRACE:
                assert torch.equal(_bits(pre[k][:, i]), _bits(plain[k][:, i])), (c, prec, i, k)
            done += 1
    assert done > 0


@pytest.mark.parametrize("prec", PRECS)
def test_beam_one_forced_along_its_own_caption_reproduces_it(prec, geo):
    for c in CC.cases(geo.g.name)[:4]:
        plain = geo.plain(prec, c, w=1)
        caps = plain["mult_preds"][:, 0].long()
        lens = torch.as_tensor([min(int((r == CC.EOS).nonzero()[0]) if bool((r == CC.EOS).any()) else c.max_pred, c.max_pred - 1) for r in caps])
        lens = torch.minimum(lens, torch.arange(c.b) * 3 + 1) if c.b > 1 else lens        # ragged: 1, 4, 7 .. tokens, and the whole caption
        width = int(lens.max())
        if width == 0:
            continue
        forced = geo.run(prec, c, "own caption", w=1, prefix=caps[:, :width].contiguous(), plens=lens, ban=None, n=0)
        for k in KEYS + TRACE:
            assert torch.equal(_bits(forced[k]), _bits(plain[k])), (c, prec, k)


@pytest.mark.parametrize("prec", PRECS)
def test_unigram_ban_equals_an_all_ones_forbid_mask(prec, geo):
    for c in CC.cases(geo.g.name):
        ones = torch.ones(geo.g.v, dtype=torch.bool)
        plain = geo.plain(prec, c, forbid=ones)
        uni = geo.run(prec, c, "n = 1", prefix=None, ban=None, n=1)
        for k in KEYS + TRACE:
            assert torch.equal(_bits(uni[k]), _bits(plain[k])), (c, prec, k)


# ---- 4. properties ---------------------------------------------------------------------------------------------------------------------
def _hypotheses(out, c):
    """(clip, slot, tokens up to and including <eos>) of every slot that is not void"""
    for b in range(c.b):
        for s in range(out["mult_preds"].shape[1]):
            if not bool(torch.isfinite(out["mult_lprobs"][b, s])):
                assert bool((out["mult_preds"][b, s] == CC.PAD).all()), (c, b, s)
                continue
            r = out["mult_preds"][b, s].tolist()
            yield b, s, r[: r.index(CC.EOS) + 1] if CC.EOS in r else r


@pytest.mark.parametrize("prec", PRECS)
def test_hypotheses_keep_the_constraints(prec, geo):
    seen = 0
    for c in CC.cases(geo.g.name):
        out, pre, ban = geo.run(prec, c), CC.prefixes(c), CC.ban_mask(c)
        bos = CC.inputs(c)[2].tolist()
        for b, s, toks in _hypotheses(out, c):
            assert toks[: len(pre[b])] == pre[b], (c, prec, b, s, toks)
            if ban is not None:
                assert not bool(ban[torch.as_tensor(toks)].any()), (c, prec, b, s, toks)
            if c.n > 0:
                assert not CS.has_repeated_ngram([int(bos[b])] + toks, c.n), (c, prec, b, s, toks)
            seen += 1
    assert seen > 0


# ---- 5. candidate shortage, through the C ABI into canary-padded outputs ------------------------------------------------------------------
CANARY = -7


class _Raw:
    """conette_decode_constrained called directly; every output lies between two canary blocks of 64 elements"""

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
        self.need = int(eng.lib.conette_decode_constrained_workspace_bytes(eng._ctx_dec, b, t, w, maxp))
        self.ws = torch.empty(self.need, dtype=torch.uint8, device="cuda")

    def call(self, fe, lens, bos, forbid=None, prefix=None, plens=None, pw=0, ban=None, n=0, min_pred=0, **change):
        b, t, w, maxp = self.dims
        a = dict(fe=fe, lens=lens, bos=bos, forbid=forbid, prefix=prefix, plens=plens, pw=pw, ban=ban, n=n, b=b, t=t, w=w, min_pred=min_pred,
                 maxp=maxp, ws=self.ws, ws_bytes=self.need, **self.o)
        a.update(change.pop("change", {}))
        assert not change, change
        p = lambda x: C.c_void_p(0 if x is None else x.data_ptr())
        return self.eng.lib.conette_decode_constrained(
            self.eng._ctx_dec, p(a["fe"]), p(a["lens"]), p(a["bos"]), p(a["forbid"]), p(a["prefix"]), p(a["plens"]), a["pw"], p(a["ban"]),
            a["n"], a["b"], a["t"], a["w"], a["min_pred"], a["maxp"], p(a["best_preds"]), p(a["best_lp"]), p(a["mult_preds"]), p(a["mult_lp"]),
            p(a["sizes"]), p(a["trace_sel"]), p(a["trace_val"]), p(a.get("step_logits")), p(a["ws"]), a["ws_bytes"],
            C.c_void_p(torch.cuda.current_stream().cuda_stream))

    def canaries_intact(self):
        torch.cuda.synchronize()
        return all(bool((x[:64] == CANARY).all()) and bool((x[-64:] == CANARY).all()) for x in self.whole.values())

    def outputs(self):
        torch.cuda.synchronize()
        names = {"best_lp": "best_lprobs", "mult_lp": "mult_lprobs"}
        return {names.get(k, k): v.cpu().clone() for k, v in self.o.items()}


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("gname,w", (("v31_ff32_l2", 4), ("v2049_ff256_l6", 4), ("v8193_ff4096_l2", 4), ("v31_ff32_l2", 9)))
def test_candidate_shortage_and_forced_banned_token_void_slots(prec, gname, w):
    from conette_amd.engine import Engine
    g = D.geometry(gname)
    try:
        eng = Engine(D.weights(g), precision=prec, n_layers=g.n_layers, d_ff=g.d_ff)
        b, t, maxp = 3, 8, 6
        fe, shape = D.frames(b, t, (8, 7, 1), 11)
        fe_d, lens_d = fe.cuda(), shape[:, 1].int().cuda()
        bos = D.weights(g)["model.task_id_to_token_id"][:b].int()
        words = (D.N_SPECIALS_AND_TASKS + 1, g.v - 1)
        ban = torch.ones(g.v, dtype=torch.uint8)
        ban[[CC.EOS, *words]] = 0
        raw = _Raw(eng, b, t, w, maxp, g.v)
        # (a) three finite candidates per row: step 0 takes 3 picks of w, later steps what two or fewer live rows offer
        assert raw.call(fe_d, lens_d, bos.cuda(), ban=ban.cuda()) == 0, eng.lib.conette_last_error()
        assert raw.canaries_intact()
        out = raw.outputs()
        _, _, _, void = replay(out, bos.tolist(), w, g.v, 0, maxp, [[]] * b, None, ban.bool().numpy(), 0, (gname, prec, "shortage"))
        assert void >= b * (w - 3) and int((~torch.isfinite(out["mult_lprobs"])).sum()) == void
        assert bool(torch.isfinite(out["best_lprobs"]).all())
        # (b) clip 1 is forced onto a banned token at its second step: the clip is void, its neighbours search on
        ban2 = torch.zeros(g.v, dtype=torch.uint8)
        ban2[words[1]] = 1
        prefix = torch.as_tensor([[words[0], 0], [words[0], words[1]], [0, 0]], dtype=torch.int32)
        plens = torch.as_tensor([1, 2, 0], dtype=torch.int32)
        raw2 = _Raw(eng, b, t, w, maxp, g.v)
        assert raw2.call(fe_d, lens_d, bos.cuda(), prefix=prefix.cuda(), plens=plens.cuda(), pw=2, ban=ban2.cuda(), n=2) == 0
        assert raw2.canaries_intact()
        out = raw2.outputs()
        replay(out, bos.tolist(), w, g.v, 0, maxp, [[words[0]], [words[0], words[1]], []], None, ban2.bool().numpy(), 2, (gname, prec, "forced ban"))
        assert bool((out["mult_lprobs"][1] == -float("inf")).all()) and bool((out["mult_preds"][1] == CC.PAD).all())
        assert float(out["best_lprobs"][1]) == -float("inf") and bool((out["best_preds"][1] == CC.PAD).all())
        assert bool((out["trace_sel"][1:, 1] == -1).all()) and out["trace_sel"][0, 1, 0].tolist() == [0, words[0]]
        assert bool(torch.isfinite(out["mult_lprobs"][[0, 2]]).all())
    finally:
        D.drop_weights(g)


# ---- 6. scores are the model's ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_scores_are_the_models(prec, geo):
    """Masks off (min_pred = 0, no forbid mask, no ban, n = 0), prefixes on: every returned hypothesis is scored from its own
    tokens as tests/test_gpu_group_search.py::test_scores_are_the_models scores them -- Engine.score in fp32 and exact, the forcing
    logits of the KV-cached step kernels in bf16 and f16 -- and |mult_lprobs - sum / length| <= CONSISTENCY: the prefix tokens count
    in the sum and in the length."""
    eng = geo.engine(prec)
    compared = 0
    for c in CC.cases(geo.g.name):
        if c.min_pred != 0 or c.forbid:
            continue
        out = geo.run(prec, c, "masks off", ban=None, n=0)
        fe, shape, bos = CC.inputs(c)[:3]
        lens = shape[:, 1].int()
        preds = out["mult_preds"].reshape(-1, c.max_pred).long()
        assert bool(torch.isfinite(out["mult_lprobs"]).all()), c
        n_tok = torch.as_tensor([int((r == CC.EOS).nonzero()[0]) + 1 if bool((r == CC.EOS).any()) else c.max_pred for r in preds])
        caps = torch.cat([bos.repeat_interleave(c.w)[:, None].long(), preds[:, :-1]], dim=1)
        caps = torch.where(torch.arange(c.max_pred)[None] < n_tok[:, None], caps, torch.zeros_like(caps))
        rows = torch.as_tensor([bool((preds[r, :int(n)] != CC.PAD).all()) for r, n in enumerate(n_tok)])   # pad_id inside: not scorable
        if prec in EXACT:
            sc = eng.score(fe.cuda(), lens, caps, preds, caps_per_audio=c.w)
            sums = sc["sum_lprobs"].cpu().double()
            assert sc["n_tokens"].cpu()[rows].tolist() == n_tok[rows].tolist(), (c, prec)
        else:
            eng.set_forcing_stepwise(True)
            try:
                logits = eng.forcing(fe.repeat_interleave(c.w, dim=0).cuda(), lens.repeat_interleave(c.w), caps).cpu().double()
            finally:
                eng.set_forcing_stepwise(False)
            lp = torch.log_softmax(logits, dim=-1).gather(2, preds[..., None])[..., 0]
            sums = torch.where(torch.arange(c.max_pred)[None] < n_tok[:, None], lp, torch.zeros_like(lp)).sum(dim=1)
        err = (out["mult_lprobs"].reshape(-1).double() - sums / n_tok.double()).abs()[rows]
        print(f"constrained scores {prec} {c}: {int(rows.sum())} hypotheses, max |mean lp - rescored| {float(err.max()):.3e} (bound {CONSISTENCY:.1e})")
        assert float(err.max()) <= CONSISTENCY, (c, prec, float(err.max()))
        compared += int(rows.sum())
    assert compared > 0


# ---- 7. state independence ---------------------------------------------------------------------------------------------------------------
def _det_case(geo):
    return next(c for c in CC.cases(geo.g.name) if c.b > 1 and (c.n > 0 or c.ban))


@pytest.mark.parametrize("prec", PRECS)
def test_clip_alone_equals_clip_in_batch(prec, geo):
    c = _det_case(geo)
    eng = geo.engine(prec)
    fe, shape, bos, forbid, table, plens = CC.inputs(c)
    lens = shape[:, 1].int()
    full = geo.run(prec, c)
    for i in range(c.b):
        one = _cpu(eng.decode_constrained(fe[i:i + 1].cuda(), lens[i:i + 1], bos[i:i + 1], forbid, c.w, c.min_pred, c.max_pred,
                                          prefix=table[i:i + 1], prefix_lens=plens[i:i + 1], ban_mask=CC.ban_mask(c), no_repeat_ngram=c.n,
                                          want_trace=True))
        for k in ("best_preds", "best_lprobs", "mult_preds", "mult_lprobs"):
            assert torch.equal(_bits(one[k][0]), _bits(full[k][i])), (c, prec, i, k)
        assert torch.equal(one["trace_sel"][:, 0], full["trace_sel"][:, i]), (c, prec, i)
        assert torch.equal(_bits(one["trace_val"][:, 0]), _bits(full["trace_val"][:, i])), (c, prec, i)


@pytest.mark.parametrize("prec", PRECS)
def test_identical_calls_stale_workspace_and_graph_replay_are_bit_equal(prec, geo):
    c = _det_case(geo)
    eng = geo.engine(prec)
    fe, shape, bos, forbid, table, plens = CC.inputs(c)
    fe_d, lens_d, bos_d = fe.cuda(), shape[:, 1].int().cuda(), bos.int().cuda()
    fb_d = None if forbid is None else forbid.to(torch.uint8).cuda()
    ban = CC.ban_mask(c)
    ban_d = None if ban is None else ban.to(torch.uint8).cuda()
    pre_d, plens_d = table.int().cuda(), plens.int().cuda()
    call = lambda: eng.decode_constrained(fe_d, lens_d, bos_d, fb_d, c.w, c.min_pred, c.max_pred, prefix=pre_d, prefix_lens=plens_d,
                                          ban_mask=ban_d, no_repeat_ngram=c.n, want_trace=True, check=False)
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


# ---- 8. C ABI errors -----------------------------------------------------------------------------------------------------------------------
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
    bad = [({"w": 0}, "beam"), ({"w": 17}, "beam"), ({"n": -1}, "no_repeat_ngram"), ({"n": 65}, "no_repeat_ngram"),
           ({"pw": -1}, "prefix_width"), ({"pw": maxp, "prefix": prefix, "plens": plens}, "prefix_width"),
           ({"pw": 2, "prefix": None, "plens": plens}, "prefix"), ({"pw": 2, "prefix": prefix, "plens": None}, "prefix_lens"),
           ({"ws_bytes": raw.need - 1}, "workspace"), ({"maxp": 65}, "max_pred"), ({"min_pred": -1}, "min_pred"),
           ({"fe": None}, "decode_constrained"), ({"mult_preds": None}, "decode_constrained")]
    for change, word in bad:
        st = raw.call(fe_d, lens_d, bos, change=change)
        msg = eng.lib.conette_last_error().decode()
        assert st != 0 and "decode_constrained" in msg and word in msg, (change, st, msg)
    torch.cuda.synchronize()
    for k, x in raw.whole.items():      # nothing was launched: the outputs are untouched
        assert bool((x == CANARY).all()), k
    for args in ((0, t, w, maxp), (b, t, 0, maxp), (b, t, 17, maxp), (b, t, w, 0)):
        assert eng.lib.conette_decode_constrained_workspace_bytes(eng._ctx_dec, *args) == 0
    assert raw.call(fe_d, lens_d, bos, prefix=prefix, plens=plens, pw=2, n=2) == 0, eng.lib.conette_last_error()
    assert raw.canaries_intact()
    out = raw.outputs()
    assert bool(torch.isfinite(out["mult_lprobs"]).all()) and int(out["sizes"][0]) >= 1
    assert bool((out["mult_preds"][:, :, 0] == 12).all())
    with pytest.raises(ValueError, match="beam"):
        eng.decode_constrained(fe_d, lens_d, bos, None, 17, 0, maxp)
    with pytest.raises(ValueError, match="no_repeat_ngram"):
        eng.decode_constrained(fe_d, lens_d, bos, None, 3, 0, maxp, no_repeat_ngram=65)
    with pytest.raises(ValueError, match="max_pred"):
        eng.decode_constrained(fe_d, lens_d, bos, None, 3, 0, maxp, prefix=torch.full((b, maxp), 12))
    with pytest.raises(ValueError, match="<eos>"):
        eng.decode_constrained(fe_d, lens_d, bos, None, 3, 0, maxp, prefix=torch.full((b, 2), CC.EOS))
    D.drop_weights(g)
