"""CPU: the constrained beam search rule of conette_amd/constrained_search.py -- the restatement conette_decode_constrained is held
to (tests/test_gpu_constrained_search.py) -- and the input conditions of the GPU cases (tests/constrain_cases.py).

1. Conditions on the GPU cases: every free call's effective margin >= MIN_MARGIN; every case with n > 0 or a ban mask has a call
   whose picks differ from the unconstrained picks of the same state; the seed is the first that meets both; the table covers what
   it says it covers.
2. Identities of the rule: no constraints == group_search with one group; n = 1 == a forbid mask of all ones.
3. The candidate-shortage rule and void slots, by hand.
4. check_prefix errors, AACTokenizer.words_to_ids.
5. The built library exports both symbols, the header declares them, the ABI version stays 3; argument validation."""
import os
import re

import numpy as np
import pytest
import torch

from conette_amd import constrained_search as CS
from conette_amd import group_search as GS
from tests import constrain_cases as CC
from tests import decoder_geometry as D
from tests import group_cases as GC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch.set_num_threads(min(16, os.cpu_count() or 1))


# ---- 1. the input conditions of the GPU cases --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gname", CC.GEOS)
def test_cases_meet_the_margin_and_exercise_the_constraints(gname):
    try:
        for c in CC.cases(gname):
            for seed in range(c.seed):       # the seed is the FIRST that meets both conditions
                assert not CC.meets_conditions(c._replace(seed=seed)), (c, seed)
                CC.drop_runs()
            margin, differs, n = CC.facts(c)
            print(f"constrained case {c}: {n} calls, smallest effective margin {margin:.4f}, {differs} calls the constraints change")
            assert margin >= D.MIN_MARGIN, (c, margin)
            assert differs >= 1 if (c.n > 0 or c.ban) else differs == 0, c
            res = CC.oracle_run(c)
            forced = [k for k in res["calls"] if k["forced"]]
            assert len(forced) == sum(c.plens) and not any(k["void"] for k in forced), c
            pre = CC.prefixes(c)
            for b in range(c.b):
                for s in range(c.w):
                    if np.isfinite(res["mult_lprobs"][b, s]):
                        assert res["mult_preds"][b, s, :len(pre[b])].tolist() == pre[b], (c, b, s)
            CC.drop_runs()
    finally:
        CC.drop_runs()
        D.drop_weights()


def test_table_coverage():
    cs = CC.all_cases()
    reg = lambda c: D.geometry(c.geo).v <= D.S3_T * D.S3_VPT and c.w <= 8
    assert {c.w for c in cs if reg(c)} == set(CC.REGISTER_W)
    assert {c.w for c in cs if c.w > 8} == set(CC.GENERIC_W)
    assert {c.w for c in CC.cases("v8193_ff4096_l2")} == set(CC.ALL_W)
    assert {c.b for c in cs} == {1, 3, 5}
    assert {c.n for c in cs} == {0, 2, 3} and {c.ban for c in cs} == {False, True} and {c.forbid for c in cs} == {False, True}
    assert {0, 3} <= {c.min_pred for c in cs} and any(c.min_pred == c.max_pred for c in cs)
    assert {0, 1} <= {p for c in cs for p in c.plens} and any(max(c.plens) == c.max_pred - 1 for c in cs)
    assert any(len(set(c.plens)) > 1 for c in cs)
    assert [c.max_pred for c in cs if c.max_pred > 12] == [64] and any(c.max_pred == 64 and 62 in c.plens for c in cs)


# ---- 2. identities of the rule ---------------------------------------------------------------------------------------------------------
def _calls(res):
    return [(k["step"], k["clip"], k["parents"], k["tokens"], k["sums"]) for k in res["calls"]]


@pytest.mark.parametrize("gname", ("v31_ff32_l2", "v2049_ff256_l6"))
def test_rule_identities(gname):
    """On logits that depend on a row's clip and sequence alone (one oracle pass per distinct row), exactly."""
    geo = D.geometry(gname)
    try:
        for c in CC.cases(gname):
            if c.w > 8 or c.max_pred > 12:
                continue
            fe, shape, bos, forbid = CC.inputs(c)[:4]
            fb = None if forbid is None else forbid.numpy()
            fn = GC.oracle_logits_fn(gname, fe, shape, rowwise=True)
            # a fan-out passes one row where the grouped search passes W identical ones
            gfn = lambda rows, step: fn(rows, step)
            free = CS.constrained_search(fn, bos.tolist(), c.w, c.min_pred, c.max_pred, geo.v, CC.EOS, CC.PAD, fb)
            one = GS.group_search(gfn, bos.tolist(), 1, c.w, 0.0, c.min_pred, c.max_pred, geo.v, CC.EOS, CC.PAD, fb)
            assert _calls(free) == _calls(one), c
            for k in ("mult_preds", "mult_lprobs", "lens", "best_preds", "best_lprobs"):
                assert free[k].tolist() == one[k].tolist(), (c, k)
            assert free["sizes"] == one["sizes"], c
            assert all(k["plain"] == list(zip(k["parents"], k["tokens"])) for k in free["calls"]), c
            idle = CS.constrained_search(fn, bos.tolist(), c.w, c.min_pred, c.max_pred, geo.v, CC.EOS, CC.PAD, fb,
                                         ban=np.zeros(geo.v, dtype=bool), no_repeat_ngram=64)
            assert _calls(idle) == _calls(free), c
            uni = CS.constrained_search(fn, bos.tolist(), c.w, c.min_pred, c.max_pred, geo.v, CC.EOS, CC.PAD, fb, no_repeat_ngram=1)
            ones = CS.constrained_search(fn, bos.tolist(), c.w, c.min_pred, c.max_pred, geo.v, CC.EOS, CC.PAD, np.ones(geo.v, dtype=bool))
            assert _calls(uni) == _calls(ones), c
            assert uni["mult_preds"].tolist() == ones["mult_preds"].tolist() and uni["mult_lprobs"].tolist() == ones["mult_lprobs"].tolist(), c
    finally:
        D.drop_weights()


def test_ngram_rule_by_hand():
    assert CS.ngram_banned([5, 1, 2, 1], 2) == [2]                   # the bigram (1, 2) exists: after 1, never 2 again
    assert CS.ngram_banned([5, 1, 2, 1], 3) == []
    assert CS.ngram_banned([5, 1, 2, 3, 1, 2], 3) == [3]
    assert CS.ngram_banned([5, 5, 5], 2) == [5, 5]                   # position 0 takes part
    assert sorted(CS.ngram_banned([5, 1, 2], 1)) == [1, 2, 5]        # n = 1: every token of the sequence
    assert CS.ngram_banned([5, 1, 2], 0) == [] and CS.ngram_banned([5], 2) == [] and CS.ngram_banned([5, 1], 64) == []
    assert CS.has_repeated_ngram([5, 1, 2, 1, 2], 2) and not CS.has_repeated_ngram([5, 1, 2, 1, 3], 2)
    z = CS.constraint_mask(np.zeros(6), [5, 1, 2, 1], 3, 5, 0, forbid=np.array([0, 0, 0, 0, 0, 1]), ban=np.array([0, 0, 0, 1, 0, 0]),
                           no_repeat_ngram=2)
    assert np.isneginf(z).tolist() == [True, False, True, True, False, True]     # EOS floor (id 0), M3 (2), M2 (3), forbid-repeat (5)


# ---- 3. candidate shortage and void slots -----------------------------------------------------------------------------------------------
def test_decide_takes_only_finite_candidates():
    z = np.log(np.array([[0.1, 0.2, 0.3, 0.4]]))
    d = CS.decide(z, [[5]], [0.0], 3, 0, 0, eos_id=2, ban=np.array([1, 1, 0, 0]))
    assert (d["parents"], d["tokens"]) == ([0, 0], [3, 2]) and not d["void"]          # two finite candidates for three picks
    np.testing.assert_allclose(d["sums"], np.log([0.4 / 0.7, 0.3 / 0.7]), atol=1e-12)
    np.testing.assert_allclose(d["margin"], np.log(0.4 / 0.3), atol=1e-12)           # no candidate is left: only the picks' gap
    d = CS.decide(z, [[5]], [0.0], 2, 0, 0, eos_id=2, ban=np.ones(4))
    assert d["tokens"] == [] and d["margin"] == float("inf")                          # nothing finite: no pick, NaN scores never picked
    d = CS.decide(np.zeros((2, 4)), [[5, 1], [5, 3]], [-1.0, -1.0], 2, 1, 0, eos_id=2)
    assert (d["parents"], d["tokens"]) == ([0, 0], [0, 1]) and d["margin"] == 0.0     # ties: lowest flat index
    f = CS.decide(z, [[5]], [0.0], 3, 0, 0, eos_id=2, forced_token=1)
    assert (f["parents"], f["tokens"], f["void"]) == ([0], [1], False)
    np.testing.assert_allclose(f["sums"], [np.log(0.2)], atol=1e-12)
    for bad in (dict(forced_token=1, ban=np.array([0, 1, 0, 0])), dict(forced_token=2), dict(forced_token=4), dict(forced_token=-1)):
        f = CS.decide(z, [[5]], [0.0], 3, 0, 0, eos_id=2, **bad)
        assert f["void"] and f["tokens"] == []


def test_void_slots_of_a_whole_search():
    """Four tokens, <eos> = 2; token 0 banned: every row offers three candidates to a beam of 4."""
    logits = np.log(np.array([0.1, 0.4, 0.2, 0.3]))
    fn = lambda rows, step: np.stack([logits for _ in rows])
    res = CS.constrained_search(fn, [3, 3], 4, 0, 3, 4, 2, 0, ban=np.array([1, 0, 0, 0]), prefixes=[[], [0]])
    first = res["calls"][0]
    assert (first["step"], first["clip"], first["tokens"]) == (0, 0, [1, 3, 2])       # three picks; <eos> lands in slot 2, slot 3 is void
    assert res["lens"][0].tolist() == [3, 3, 1, 0] and np.isneginf(res["mult_lprobs"][0, 3]) and np.isfinite(res["mult_lprobs"][0, :3]).all()
    assert res["mult_preds"][0, 3].tolist() == [0, 0, 0] and res["mult_preds"][0, 2].tolist() == [2, 0, 0]
    # clip 1 is forced onto the banned token: all four slots void, best_* of a void clip
    assert res["calls"][1]["void"] and np.isneginf(res["mult_lprobs"][1]).all() and res["lens"][1].tolist() == [0, 0, 0, 0]
    assert res["best_preds"][1].tolist() == [0, 0, 0] and np.isneginf(res["best_lprobs"][1])
    assert [k["clip"] for k in res["calls"]].count(1) == 1
    assert res["sizes"][0] == 3


def test_prefix_search_is_the_restricted_search():
    """The scores of a prefixed search count the prefix tokens in the sum and in the length."""
    logits = np.log(np.array([0.1, 0.4, 0.2, 0.3]))
    fn = lambda rows, step: np.stack([logits for _ in rows])
    res = CS.constrained_search(fn, [3], 1, 0, 4, 4, 2, 0, prefixes=[[3, 0]])
    assert res["mult_preds"][0, 0].tolist() == [3, 0, 1, 1] and res["lens"][0, 0] == 4
    np.testing.assert_allclose(res["mult_lprobs"][0, 0], np.log(0.3 * 0.1 * 0.4 * 0.4) / 4, atol=1e-12)
    assert [k["forced"] for k in res["calls"]] == [True, True, False, False]


# ---- 4. the host checks ------------------------------------------------------------------------------------------------------------------
def test_check_prefix():
    kw = dict(vocab_size=20, max_pred=6, eos_id=2, pad_id=0, bos_id=1)
    assert CS.check_prefix([11, 12, 13], 5, **kw) == [11, 12, 13] and CS.check_prefix([], 5, **kw) == []
    assert CS.check_prefix([11, 12, 11], 5, no_repeat_ngram=2, **kw) == [11, 12, 11]
    for bad, word in (([11, 2], "<eos>"), ([0], "<pad>"), ([1, 11], "<bos>"), ([20], "vocabulary"), ([-1], "vocabulary"),
                      ([11] * 6, "max_pred")):
        with pytest.raises(ValueError, match=word):
            CS.check_prefix(bad, 5, **kw)
    with pytest.raises(ValueError, match="banned"):
        CS.check_prefix([11, 12], 5, ban=np.eye(20)[12], **kw)
    with pytest.raises(ValueError, match="forbid"):
        CS.check_prefix([11, 12, 11], 5, forbid=np.eye(20)[11], **kw)
    with pytest.raises(ValueError, match="forbid"):
        CS.check_prefix([11, 5], 5, forbid=np.eye(20)[5], **kw)               # the task token counts
    assert CS.check_prefix([11, 12, 11], 5, forbid=np.eye(20)[12], **kw)
    with pytest.raises(ValueError, match="2-gram"):
        CS.check_prefix([11, 12, 11, 12], 5, no_repeat_ngram=2, **kw)
    with pytest.raises(ValueError, match="1-gram"):
        CS.check_prefix([11, 12, 11], 5, no_repeat_ngram=1, **kw)


def test_words_to_ids():
    from conette_amd.tokenizer import AACTokenizer
    tok = AACTokenizer()
    for i, word in enumerate(["<pad>", "<bos>", "<eos>", "<unk>", "a", "dog", "barks", "loudly"]):
        tok._itos[i], tok._stoi[word], tok._vocab[word] = word, i, 1
    assert tok.words_to_ids("a dog  barks") == [4, 5, 6] and tok.words_to_ids("") == [] and tok.words_to_ids(" \n") == []
    assert tok.words_to_ids("A Dog") == [4, 5]                      # the tokenizer lower-cases
    tok._hparams["lowercase"] = False
    with pytest.raises(ValueError, match="Dog"):
        tok.words_to_ids("a Dog")
    with pytest.raises(ValueError, match="cat"):
        tok.words_to_ids("a cat barks")
    assert tok.words_to_ids("a cat barks", skip_unknown=True) == [4, 6]
    assert "spaCy" in AACTokenizer.words_to_ids.__doc__


# ---- 5. the library, the header, the host helper ---------------------------------------------------------------------------------------
def test_library_exports_and_header_declares_the_entry_points():
    import __graft_entry__ as ge
    ge.build()
    from conette_amd import engine
    lib = engine.load_library()
    text = open(os.path.join(ROOT, "include", "conette_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("conette_decode_constrained_workspace_bytes", "conette_decode_constrained"):
        assert hasattr(lib, name) and name in engine.EXPORTS and re.search(r"\b" + name + r"\s*\(", hdr), name
    assert "#define CONETTE_ABI_VERSION 3" in text
    assert lib.conette_abi_version() == 3
    for word in ("forced", "fan-out", "void slot", "M3"):
        assert word in text, word


def test_argument_validation():
    assert CS.check_arguments(1, 0, 20) == (1, 0) and CS.check_arguments(16, 64, 64, 63) == (16, 64)
    for w in (0, 17, -1, 2.5):
        with pytest.raises(ValueError, match="beam"):
            CS.check_arguments(w, 0, 20)
    for n in (-1, 65, 1.5):
        with pytest.raises(ValueError, match="no_repeat_ngram"):
            CS.check_arguments(3, n, 20)
    for p in (20, 21, -1):
        with pytest.raises(ValueError, match="max_pred"):
            CS.check_arguments(3, 0, 20, p)
    with pytest.raises(ValueError, match="max_pred"):
        CS.check_arguments(3, 0, 65)
    with pytest.raises(ValueError, match="beam"):
        CS.constrained_search(lambda rows, step: np.zeros((len(rows), 8)), [5], 17, 0, 4, 8)


def test_cli_flags():
    from conette_amd import predict
    a = predict.get_predict_args(["--audio", "a.wav", "--prefix", "a dog", "--ban_words", "barks", "loudly", "--no_repeat_ngram", "3"])
    assert (a.prefix, a.ban_words, a.no_repeat_ngram) == ("a dog", ["barks", "loudly"], 3)
    a = predict.get_predict_args(["--audio", "a.wav"])
    assert (a.prefix, a.ban_words, a.no_repeat_ngram) == (None, None, 0)
    with pytest.raises(ValueError, match="--sample"):
        predict.get_predict_args(["--audio", "a.wav", "--prefix", "a dog", "--sample", "2"])
    with pytest.raises(ValueError, match="--beam_groups"):
        predict.get_predict_args(["--audio", "a.wav", "--no_repeat_ngram", "2", "--beam_groups", "3"])
