"""CPU: the diverse beam search rule of conette_amd/group_search.py -- the restatement conette_decode_groups is held to
(tests/test_gpu_group_search.py) -- and the input conditions of the GPU cases (tests/group_cases.py).

1. With one group the restatement reproduces decoder_geometry.oracle_search (oracle.cpu_ref.generate, which is verified against
   the reference) on the table's searches of v31_ff32_l2 and v2049_ff256_l6: parents and tokens identical, sums within 1e-5.
2. Identities of the rule: with lambda = 0 every group equals the one-group search, with lambda > 0 group 0 does.
3. Conditions on the GPU cases: every call's effective margin >= MIN_MARGIN; every lambda > 0 case has a call whose penalised
   picks differ from its unpenalised top-k; some case has a group with k_g == 0 while another group of the clip searches on;
   some case has hypotheses finishing at several steps inside one group; the table covers what it says it covers.
4. The built library exports both symbols and the header declares them; argument validation of the host helper."""
import os
import re

import numpy as np
import pytest
import torch

from conette_amd import group_search as GS
from tests import decoder_geometry as D
from tests import group_cases as GC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch.set_num_threads(min(16, os.cpu_count() or 1))


# ---- 1. the restatement against the oracle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gname", ("v31_ff32_l2", "v2049_ff256_l6"))
def test_one_group_reproduces_the_oracle_search(gname):
    g = D.geometry(gname)
    try:
        for s in g.searches:
            ref = D.oracle_search(g, s)
            fe, shape, bos, forbid = D.search_inputs(g, s)
            for lam in (0.0, 0.7):     # with one group the penalty has nothing to count
                res = GS.group_search(GC.oracle_logits_fn(gname, fe, shape), bos.tolist(), 1, s.beam, lam, s.min_pred, s.max_pred, g.v,
                                      GC.EOS, GC.PAD, forbid.numpy())
                calls = {(c["step"], c["clip"]): c for c in res["calls"]}
                assert len(calls) == len(ref["calls"]), (gname, s.name)
                for step, clip, par, tok, sums, margin in ref["calls"]:
                    c = calls[(step, clip)]
                    assert c["parents"] == par and c["tokens"] == tok, (gname, s.name, step, clip)
                    np.testing.assert_allclose(c["sums"], sums, rtol=0, atol=1e-5)
                    np.testing.assert_allclose(c["keys"], c["sums"], rtol=0, atol=0)
                    assert abs(c["margin"] - D.effective_margin((step, clip, par, tok, sums, margin))) <= 2e-5
                ps = ref["mult_preds"].shape[2]
                assert res["mult_preds"][:, :, :ps].tolist() == ref["mult_preds"].tolist(), (gname, s.name)
                assert bool((res["mult_preds"][:, :, ps:] == GC.PAD).all()) and res["sizes"][0] == ps
                np.testing.assert_allclose(res["mult_lprobs"], ref["mult_lprobs"].numpy(), rtol=0, atol=1e-5)
                bl = ref["best_preds"].shape[1]
                assert res["best_preds"][:, :bl].tolist() == ref["best_preds"].tolist() and res["sizes"][1] == bl
                np.testing.assert_allclose(res["best_lprobs"], ref["best_lprobs"].numpy(), rtol=0, atol=1e-5)
    finally:
        D.drop_weights(g)


# ---- 2. identities of the rule ---------------------------------------------------------------------------------------------------------
def _group_calls(res, group):
    return [(c["step"], c["clip"], c["parents"], c["tokens"], c["sums"]) for c in res["calls"] if c["group"] == group]


@pytest.mark.parametrize("gname", ("v31_ff32_l2", "v2049_ff256_l6"))
def test_group_identities(gname):
    """On logits that depend on a row's clip and prefix alone (one oracle pass per distinct row), exactly."""
    geo = D.geometry(gname)
    try:
        for c in GC.cases(gname):
            if c.g == 1 or (c.g, c.w) in ((16, 1), (2, 8), (5, 3)):
                continue
            fe, shape, bos, forbid = GC.inputs(c)
            fn = GC.oracle_logits_fn(gname, fe, shape, rowwise=True)
            run = lambda g, lam: GS.group_search(fn, bos.tolist(), g, c.w, lam, c.min_pred, c.max_pred, geo.v, GC.EOS, GC.PAD,
                                                 None if forbid is None else forbid.numpy())
            one = run(1, c.lam)
            want = _group_calls(one, 0)
            zero = run(c.g, 0.0)
            for grp in range(c.g):
                assert _group_calls(zero, grp) == want, (c, grp)
                sl = slice(grp * c.w, (grp + 1) * c.w)
                assert zero["mult_preds"][:, sl].tolist() == one["mult_preds"].tolist(), (c, grp)
                assert zero["mult_lprobs"][:, sl].tolist() == one["mult_lprobs"].tolist(), (c, grp)
            pen = run(c.g, c.lam if c.lam > 0 else 1.5)
            assert _group_calls(pen, 0) == want, c
            assert pen["mult_preds"][:, :c.w].tolist() == one["mult_preds"].tolist(), c
            assert pen["mult_lprobs"][:, :c.w].tolist() == one["mult_lprobs"].tolist(), c
    finally:
        D.drop_weights()


def test_decide_group_by_hand():
    """Three tokens + <eos>, two rows: counts shift the keys, the picks carry the model scores, ties go to the lowest flat index."""
    z = np.log(np.array([[0.1, 0.2, 0.3, 0.4], [0.25, 0.25, 0.25, 0.25]]))
    d = GS.decide_group(z[:1], [[5]], [0.0], np.zeros(4), 2, 0, 1.0, 0, eos_id=2)
    assert d["parents"] == [0, 0] and d["tokens"] == [3, 2]
    np.testing.assert_allclose(d["sums"], np.log([0.4, 0.3]), atol=1e-12)
    np.testing.assert_allclose(d["margin"], min(np.log(0.4 / 0.3), np.log(0.3 / 0.2)), atol=1e-12)
    d = GS.decide_group(z[:1], [[5]], [0.0], np.array([0, 0, 0, 1]), 2, 0, 1.0, 0, eos_id=2)     # token 3 was picked once: -1
    assert d["tokens"] == [2, 1]
    d = GS.decide_group(z[:1], [[5]], [0.0], np.array([0, 0, 0, 1]), 2, 0, 0.1, 0, eos_id=2)     # a small penalty keeps it first
    assert d["tokens"] == [3, 2]
    np.testing.assert_allclose(d["sums"][0], np.log(0.4), atol=1e-12)                            # the model score, not the key
    np.testing.assert_allclose(d["keys"][0], np.log(0.4) - 0.1, atol=1e-12)
    d = GS.decide_group(z, [[5, 1], [5, 3]], [-1.0, -1.0], np.zeros(4), 2, 1, 0.0, 0, eos_id=2)
    assert (d["parents"], d["tokens"]) == ([0, 0], [3, 2])
    d = GS.decide_group(np.zeros((3, 4)), [[5, 1], [5, 3], [5, 0]], [-1.0, -1.0, -1.0], np.zeros(4), 3, 1, 0.0, 0, eos_id=2)
    assert (d["parents"], d["tokens"]) == ([0, 0, 0], [0, 1, 2]) and d["margin"] == 0.0                     # all tied: lowest flat index
    d = GS.decide_group(np.zeros((1, 4)), [[1]], [0.0], np.zeros(4), 1, 0, 0.0, 3, eos_id=2, forbid=np.array([0, 1, 0, 0]))
    assert d["tokens"] == [0]                                                                                # EOS floor + forbid of token 1
    d = GS.decide_group(np.array([[0.0, 1.0, 5.0, 0.5]]), [[1]], [0.0], np.zeros(4), 1, 0, 0.0, 3, eos_id=2, forbid=np.array([0, 1, 0, 0]))
    assert d["tokens"] == [3]


# ---- 3. the input conditions of the GPU cases --------------------------------------------------------------------------------------------
_FACTS = {}


def _facts(c):
    if c not in _FACTS:
        res = GC.oracle_run(c)
        differs = sum(1 for k in res["calls"] if list(zip(k["parents"], k["tokens"])) != k["plain"])
        live = {}
        for k in res["calls"]:
            live.setdefault((k["step"], k["clip"]), set()).add(k["group"])
        partial = sum(1 for gs in live.values() if len(gs) < c.g)
        lens = res["lens"].reshape(c.b, c.g, c.w)
        several = sum(1 for b in range(c.b) for g in range(c.g) if len(set(lens[b, g].tolist())) > 1)
        _FACTS[c] = (GC.min_margin(res), differs, partial, several, len(res["calls"]))
        GC._RUNS.pop(c, None)
    return _FACTS[c]


@pytest.mark.parametrize("gname", GC.GEOS)
def test_cases_meet_the_margin_and_exercise_the_penalty(gname):
    try:
        for c in GC.cases(gname):
            margin, differs, _, _, n = _facts(c)
            print(f"group case {c}: {n} calls, smallest effective margin {margin:.4f}, {differs} calls the penalty changes")
            assert margin >= D.MIN_MARGIN, (c, margin)
            if c.lam > 0 and c.g > 1:
                assert differs >= 1, c
            else:
                assert differs == 0, c
    finally:
        D.drop_weights()


def test_table_coverage():
    cs = GC.all_cases()
    try:
        assert {(c.g, c.w) for c in cs if c.geo != "v8193_ff4096_l2" and c.g * c.w <= 8} == set(GC.REGISTER_GW)
        assert {(c.g, c.w) for c in cs if c.g * c.w > 8} == set(GC.GENERIC_GW)
        for gname in GC.GEOS:
            v = D.geometry(gname).v
            kernels = {"register" if (v <= D.S3_T * D.S3_VPT and c.g * c.w <= 8) else "generic" for c in GC.cases(gname)}
            assert kernels == ({"generic"} if gname == "v8193_ff4096_l2" else {"register", "generic"}), gname
            assert all(v > c.g for c in GC.cases(gname))
        assert {c.b for c in cs} == {1, 3, 5} and {c.rows % 4 for c in cs} == {0, 1, 2, 3}
        assert {1, 7, 8, 25} <= {n for c in cs for n in c.frame_lens}
        assert {c.lam for c in cs} == {0.0, 0.5, 2.0}
        assert any(c.max_pred == 64 and c.min_pred == 60 for c in cs) and any(c.min_pred == c.max_pred for c in cs)
        assert any(c.min_pred == 0 for c in cs) and any(c.forbid for c in cs) and any(not c.forbid for c in cs)
        facts = [_facts(c) for c in cs]
        assert any(f[2] > 0 for f in facts), "no case has a finished group beside a searching one"
        assert any(f[3] > 0 for f, c in zip(facts, cs) if c.w > 1), "no group finishes its hypotheses at several steps"
    finally:
        D.drop_weights()


# ---- 4. the library, the header, the host helper ---------------------------------------------------------------------------------------
def test_library_exports_and_header_declares_the_entry_points():
    import __graft_entry__ as ge
    ge.build()
    from conette_amd import engine
    lib = engine.load_library()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "conette_hip.h")).read(), flags=re.S)
    for name in ("conette_decode_groups_workspace_bytes", "conette_decode_groups"):
        assert hasattr(lib, name) and name in engine.EXPORTS and re.search(r"\b" + name + r"\s*\(", hdr), name
    assert "#define CONETTE_ABI_VERSION 3" in open(os.path.join(ROOT, "include", "conette_hip.h")).read()
    assert lib.conette_abi_version() == 3


def test_argument_validation():
    assert GS.check_arguments(3, 1, 0.5) == (3, 1) and GS.check_arguments(16, 1, 0.0) == (16, 1) and GS.check_arguments(4, 4, 2) == (4, 4)
    for g, w in ((17, 1), (1, 17), (3, 6), (0, 3), (3, 0), (-1, 2), (2.5, 2)):
        with pytest.raises(ValueError, match="n_groups"):
            GS.check_arguments(g, w, 0.5)
    for lam in (-0.1, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="diversity_penalty"):
            GS.check_arguments(3, 1, lam)
    with pytest.raises(ValueError, match="n_groups"):
        GS.group_search(lambda rows, step: np.zeros((len(rows), 8)), [5], 9, 2, 0.5, 0, 4, 8)


def test_cli_flags_are_exclusive():
    from conette_amd import predict
    a = predict.get_predict_args(["--audio", "a.wav", "--beam_groups", "3", "--group_beam", "2", "--diversity_penalty", "1.5"])
    assert (a.beam_groups, a.group_beam, a.diversity_penalty) == (3, 2, 1.5)
    a = predict.get_predict_args(["--audio", "a.wav"])
    assert (a.beam_groups, a.group_beam, a.diversity_penalty) == (0, 1, 0.5)
    with pytest.raises(ValueError, match="--sample"):
        predict.get_predict_args(["--audio", "a.wav", "--beam_groups", "3", "--sample", "2"])
    with pytest.raises(ValueError, match="--align"):
        predict.get_predict_args(["--audio", "a.wav", "--beam_groups", "3", "--align"])
