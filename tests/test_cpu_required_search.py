"""CPU: the keyword-guided beam search rule of conette_amd/required_search.py -- the restatement conette_decode_required is held to
(tests/test_gpu_required_search.py) -- and the input conditions of the GPU cases (tests/require_cases.py).

1. Conditions on the GPU cases: every free call's effective margin >= MIN_MARGIN; every case has a call whose picks differ from the
   picks of the same state without requirements; the seed is the first that meets both; the M5 and shortage cases exercise M5 and
   shortage; every hypothesis of the restatement holds a token of every group; the table covers what it says it covers.
2. The rule on synthetic logits: banks, deal order, ties, shortage, M4 / M5, the guarantee; no requirement == constrained_search.
3. check_requirements / check_arguments errors, pack_tables, spec parsing of the model layer against a toy tokenizer, the CLI flag.
4. The built library exports both symbols, the header declares them, the ABI version stays 3."""
import os
import re

import numpy as np
import pytest
import torch

from conette_amd import constrained_search as CS
from conette_amd import required_search as RS
from tests import decoder_geometry as D
from tests import require_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch.set_num_threads(min(16, os.cpu_count() or 1))


# ---- 1. the input conditions of the GPU cases --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gname", RC.GEOS)
def test_cases_meet_the_margin_and_exercise_the_requirements(gname):
    try:
        for c in RC.cases(gname):
            for seed in range(c.seed):       # the seed is the FIRST that meets both conditions
                assert not RC.meets_conditions(c._replace(seed=seed)), (c, seed)
                RC.drop_runs()
            f = RC.facts(c)
            print(f"required case {c}: {f['calls']} calls, smallest effective margin {f['margin']:.4f}, {f['differs']} calls the "
                  f"requirements change, {f['m5']} calls under M5, {f['void']} void slots")
            assert f["margin"] >= D.MIN_MARGIN, (c, f)
            assert f["differs"] >= 1, (c, f)
            if c.mode in RC.M5_MODES:
                assert f["m5"] >= 1, (c, f)
            if c.mode in ("fan", "short"):
                assert f["m5_fan"] >= 1, (c, f)
            if c.mode == "short":
                assert f["void"] >= 1, (c, f)
            res, req, pre, bos = RC.oracle_run(c), RC.requirements(c), RC.prefixes(c), RC.inputs(c)[2].tolist()
            seen = 0
            for b in range(c.b):
                RS.check_requirements(req[b], bos[b], vocab_size=D.geometry(gname).v, max_pred=c.max_pred, eos_id=RC.EOS, pad_id=RC.PAD,
                                      ban=None if RC.ban_mask(c) is None else RC.ban_mask(c).numpy(), prefix=pre[b])
                for s in range(c.w):
                    if not np.isfinite(res["mult_lprobs"][b, s]):
                        continue
                    toks = res["mult_preds"][b, s, : res["lens"][b, s]].tolist()
                    assert all(RS.met_groups([bos[b]] + toks, req[b])), (c, b, s, toks)
                    assert toks[-1] == RC.EOS or len(toks) == c.max_pred, (c, b, s, toks)
                    seen += 1
            assert seen > 0, c
            if c.mode == "premet":
                assert pre[0][0] in req[0][0]
            if c.mode == "allmet":
                assert all(RS.met_groups([bos[0]] + pre[0], req[0])) and len(req[0]) > 0
            RC.drop_runs()
    finally:
        RC.drop_runs()
        D.drop_weights()


def test_table_coverage():
    cs = RC.all_cases()
    reg = lambda c: D.geometry(c.geo).v <= D.S3_T * D.S3_VPT and c.w <= 8
    assert {c.w for c in cs if reg(c)} == {1, 3, 4, 5, 8} and {c.w for c in cs if c.w > 8} == {9, 16}
    assert {c.w for c in RC.cases("v8193_ff4096_l2")} == {3, 4, 9} and {c.w for c in RC.cases("v8192_ff2304_l6")} == {1, 8, 16}
    assert {c.geo for c in cs} == set(RC.GEOS) and {c.b for c in cs} == {1, 3, 5}
    assert {g for c in cs for g in c.gs} == {0, 1, 2, 3, 8}
    assert any(0 in c.gs and max(c.gs) > 0 for c in cs) and any(len(set(c.gs)) > 2 for c in cs)
    assert {c.n for c in cs} == {0, 2, 3} and {c.ban for c in cs} == {False, True} and {c.forbid for c in cs} == {False, True}
    assert {0, 3} <= {c.min_pred for c in cs} and any(c.min_pred == c.max_pred for c in cs)
    assert all(4 <= c.max_pred <= 10 for c in cs if c.max_pred != 64) and [c.max_pred for c in cs].count(64) == 1
    assert 3 * sum(c.mode in RC.M5_MODES for c in cs) >= len(cs)
    assert any(c.mode in ("fan", "short") and any(g == c.max_pred - p for g, p in zip(c.gs, c.plens)) for c in cs)
    assert {"short", "premet", "allmet", "full32"} <= {c.mode for c in cs}
    sizes = set()
    for c in cs:
        req = RC.requirements(c)
        rt, rg = RC.tables(c)
        sizes |= {len(g) for r in req for g in r}
        assert rt.shape == rg.shape and rt.shape[1] <= RS.MAX_REQ_TOKENS
        for b, r in enumerate(req):      # the table holds the clip's groups, whatever the order of its entries
            got = {g: sorted(rt[b][rg[b] == g].tolist()) for g in range(len(r))}
            assert got == {g: sorted(toks) for g, toks in enumerate(r)} and int((rg[b] >= len(r)).sum()) == 0, (c, b)
        if c.mode == "full32":
            assert rt.shape[1] == 32 and int((rg[0] >= 0).sum()) == 32
        else:
            assert bool((rg == -1).any()), c                     # gaps
        if c.forbid:
            fb = RC.inputs(c)[3]
            sizes.add(("forbid", bool(fb[torch.as_tensor([t for r in req for g in r for t in g])].any())))
    assert {1, 2, 3} <= sizes and ("forbid", True) in sizes
    D.drop_weights()


# ---- 2. the rule on synthetic logits -------------------------------------------------------------------------------------------------------
def _z(*rows):
    return np.log(np.array(rows, dtype=np.float64))


def test_banks_and_deal_order_by_hand():
    """V = 6, <eos> = 2, task token 1; groups {3} and {4, 5}.  Row 0 has met nothing, row 1 has met group 0."""
    groups = [[3], [4, 5]]
    z = _z([0.30, 0.05, 0.05, 0.10, 0.20, 0.30], [0.25, 0.05, 0.30, 0.20, 0.15, 0.05])
    d = RS.decide(z, [[1, 0], [1, 3]], [-1.0, -1.5], 4, 1, 0, 10, eos_id=2, groups=groups)
    # banks: row 0 (c = 0): tokens 3, 4, 5 -> bank 1, others bank 0 (<eos> masked by M4); row 1 (c = 1): 4, 5 -> bank 2, others bank 1
    # bank 2: (1, 4) (1, 5); bank 1: row 0's 5, 4, 3 and row 1's 0, 3, 1 by score; bank 0: (0, 0), (0, 1)
    assert d["banks"] == [2, 1, 0, 2] and d["parents"] == [1, 0, 0, 1] and d["tokens"] == [4, 5, 0, 5]
    lp0 = np.log(np.array([0.30, 0.05, 0, 0.10, 0.20, 0.30]) / 0.95)
    lp1 = np.log(np.array([0.25, 0.05, 0, 0.20, 0.15, 0.05]) / 0.70)
    np.testing.assert_allclose(d["sums"], [-1.5 + lp1[4], -1.0 + lp0[5], -1.0 + lp0[0], -1.5 + lp1[5]], atol=1e-12)
    # margin: bank 2 has no candidate left after its two picks; bank 1: pick vs (1, 0); bank 0: pick vs (0, 1)
    gaps = [lp1[4] - lp1[5], (-1.0 + lp0[5]) - max(-1.0 + lp0[4], -1.5 + lp1[0]), lp0[0] - lp0[1]]
    np.testing.assert_allclose(d["margin"], min(gaps), atol=1e-12)
    assert d["m5_rows"] == 0
    # beam 1 takes the highest bank; beam 2 one of each of the two highest
    assert RS.decide(z, [[1, 0], [1, 3]], [-1.0, -1.5], 1, 1, 0, 10, eos_id=2, groups=groups)["banks"] == [2]
    assert RS.decide(z, [[1, 0], [1, 3]], [-1.0, -1.5], 2, 1, 0, 10, eos_id=2, groups=groups)["banks"] == [2, 1]
    # an exhausted bank is skipped: 7 slots over 2 + 6 + 2 candidates -> 2, 1, 0, 2, 1, 0, 1
    assert RS.decide(z, [[1, 0], [1, 3]], [-1.0, -1.5], 7, 1, 0, 10, eos_id=2, groups=groups)["banks"] == [2, 1, 0, 2, 1, 0, 1]
    # ties inside a bank go to the lowest flat index
    t = RS.decide(np.zeros((2, 6)), [[1, 0], [1, 0]], [-1.0, -1.0], 4, 1, 0, 10, eos_id=2, groups=groups)
    assert (t["banks"], t["parents"], t["tokens"]) == ([1, 0, 1, 0], [0, 0, 0, 0], [3, 0, 4, 1]) and t["margin"] == 0.0


def test_m4_m5_and_shortage_by_hand():
    groups = [[3], [4, 5]]
    z = _z([0.30, 0.05, 0.05, 0.10, 0.20, 0.30])
    m = RS.requirement_mask(z[0], [1], 0, 10, 2, groups)
    assert np.isneginf(m).tolist() == [False, False, True, False, False, False]                  # M4
    m = RS.requirement_mask(z[0], [1], 0, 2, 2, groups)
    assert np.isneginf(m).tolist() == [True, True, True, False, False, False]                    # M5: 2 unmet >= 2 - 0
    m = RS.requirement_mask(z[0], [1, 3], 1, 2, 2, groups)
    assert np.isneginf(m).tolist() == [True, True, True, True, False, False]                     # only the open group's tokens
    m = RS.requirement_mask(z[0], [1, 3, 4], 2, 3, 2, groups)
    assert not np.isneginf(m).any()                                                             # all met: nothing
    assert not np.isneginf(RS.requirement_mask(z[0], [3, 1], 1, 2, 2, [[3]])).all()              # position 0 does not count
    assert np.isneginf(RS.requirement_mask(z[0], [3, 1], 1, 2, 2, [[3]])).tolist() == [True, True, True, False, True, True]
    # M5 at the fan-out: three candidates for four slots, and one void slot in the whole search
    d = RS.decide(z, [[1]], [0.0], 4, 0, 0, 2, eos_id=2, groups=groups)
    assert (d["tokens"], d["banks"], d["m5_rows"]) == ([5, 4, 3], [1, 1, 1], 1)
    fn = lambda rows, step: np.stack([z[0] for _ in rows])
    res = RS.required_search(fn, [1], 4, 0, 2, 6, 2, 0, required=[groups])
    assert np.isneginf(res["mult_lprobs"][0]).sum() == 1 and res["lens"][0].tolist() == [2, 2, 2, 0]
    assert sorted(res["mult_preds"][0, :3].tolist()) == [[3, 5], [4, 3], [5, 3]]       # (3, 4) is the fourth of three picks
    # a forced call under M5: a prefix token outside the open groups voids the clip
    f = RS.decide(z, [[1]], [0.0], 4, 0, 0, 2, eos_id=2, groups=groups, forced_token=0)
    assert f["void"] and RS.decide(z, [[1]], [0.0], 4, 0, 0, 2, eos_id=2, groups=groups, forced_token=4)["tokens"] == [4]


@pytest.mark.parametrize("beam", (1, 2, 3, 5, 8, 16))
def test_guarantee_on_random_logits(beam):
    """Every hypothesis that is not void holds a token of every group and ends in <eos> or at max_pred; no <eos> before the last
    group is met; with no requirement the calls are constrained_search's."""
    rng = np.random.default_rng(beam)
    v, seen = 40, 0
    for g_n in range(0, 6):
        ids = rng.permutation(np.arange(4, v))
        groups = [[int(t) for t in ids[3 * g: 3 * g + 1 + g % 3]] for g in range(g_n)]
        table = rng.normal(size=(64, v)) * 2.0
        fn = lambda rows, step: np.stack([table[(sum(p) * 7 + step) % 64] for _, p in rows])
        max_pred = 6 + g_n % 2
        ban = np.zeros(v, dtype=bool)
        ban[ids[-5:]] = True
        res = RS.required_search(fn, [3, 3], beam, 0, max_pred, v, 2, 0, None, [[], [int(ids[20])]], ban, 2, [groups, groups[: g_n // 2]])
        for b, gr in enumerate((groups, groups[: g_n // 2])):
            for s in range(beam):
                if not np.isfinite(res["mult_lprobs"][b, s]):
                    continue
                toks = res["mult_preds"][b, s, : res["lens"][b, s]].tolist()
                assert all(RS.met_groups([3] + toks, gr)), (g_n, b, s, toks)
                assert toks[-1] == 2 or len(toks) == max_pred
                if 2 in toks:
                    assert all(RS.met_groups([3] + toks[: toks.index(2)], gr)), (g_n, b, s, toks)
                seen += 1
        if g_n == 0:
            plain = CS.constrained_search(fn, [3, 3], beam, 0, max_pred, v, 2, 0, None, [[], [int(ids[20])]], ban, 2)
            assert [(k["step"], k["clip"], k["parents"], k["tokens"], k["sums"], k["margin"]) for k in res["calls"]] == \
                   [(k["step"], k["clip"], k["parents"], k["tokens"], k["sums"], k["margin"]) for k in plain["calls"]]
            for k in ("mult_preds", "mult_lprobs", "lens", "best_preds", "best_lprobs"):
                assert res[k].tolist() == plain[k].tolist(), k
            assert all(set(k["banks"]) <= {0} for k in res["calls"])
            assert all(k["plain"] == list(zip(k["parents"], k["tokens"])) for k in res["calls"] if not k["forced"])
    assert seen > 0


# ---- 3. the host checks ------------------------------------------------------------------------------------------------------------------
def test_check_requirements():
    kw = dict(vocab_size=60, max_pred=6, eos_id=2, pad_id=0, bos_id=1)
    assert RS.check_requirements([[11], [12, 13, 12]], 5, **kw) == [[11], [12, 13]] and RS.check_requirements([], 5, **kw) == []
    for bad, word in (([[11, 2]], "<eos>"), ([[0]], "<pad>"), ([[1]], "<bos>"), ([[5]], "task token"), ([[60]], "vocabulary"),
                      ([[-1]], "vocabulary"), ([[11], []], "empty"), ([[11], [12, 11]], "groups 0 and 1"),
                      ([[10 + g] for g in range(9)], "9 requirement groups"), ([list(range(10, 27)), list(range(27, 43))], "33 required tokens")):
        with pytest.raises(ValueError, match=word):
            RS.check_requirements(bad, 5, **kw)
    with pytest.raises(ValueError, match=r"12.*banned"):
        RS.check_requirements([[11], [12]], 5, ban=np.eye(60)[12], **kw)
    with pytest.raises(ValueError, match=r"'dog'"):
        RS.check_requirements([[12]], 5, ban=np.eye(60)[12], words={12: "dog"}, **kw)
    # the prefix: met groups do not count, the others must fit behind it
    assert RS.check_requirements([[11], [12], [13]], 5, prefix=[20, 21, 22], **kw)
    with pytest.raises(ValueError, match="3 required groups"):
        RS.check_requirements([[11], [12], [13]], 5, prefix=[20, 21, 22, 23], **kw)
    assert RS.check_requirements([[11], [12], [13]], 5, prefix=[20, 11, 22, 23], **kw)
    assert RS.check_requirements([[10 + g] for g in range(6)], 5, **kw)
    with pytest.raises(ValueError, match="7 required groups"):
        RS.check_requirements([[10 + g] for g in range(7)], 5, **kw)


def test_argument_validation_and_tables():
    assert RS.check_arguments(1, 0, 20) == (1, 0) and RS.check_arguments(16, 64, 64, 63, 32) == (16, 64)
    for bad, word in (((0, 0, 20), "beam"), ((17, 0, 20), "beam"), ((3, 65, 20), "no_repeat_ngram"), ((3, 0, 65), "max_pred"),
                      ((3, 0, 20, 20), "max_pred"), ((3, 0, 20, 0, 33), "req_width"), ((3, 0, 20, 0, -1), "req_width")):
        with pytest.raises(ValueError, match=word):
            RS.check_arguments(*bad)
    rt, rg = RS.pack_tables([[[11], [12, 13]], [], [[14]]])
    assert rt.tolist() == [[11, 12, 13], [0, 0, 0], [14, 0, 0]] and rg.tolist() == [[0, 1, 1], [-1, -1, -1], [0, -1, -1]]
    assert rt.dtype == np.int32 and rg.dtype == np.int32
    rt, rg = RS.pack_tables([[[11], [12, 13]]], 5, [[4, 0, 2, 1, 3]])
    assert rt.tolist() == [[12, 0, 13, 0, 11]] and rg.tolist() == [[1, -1, 1, -1, 0]]
    assert RS.pack_tables([[], []])[0].shape == (2, 0)
    with pytest.raises(ValueError, match="req_width"):
        RS.pack_tables([[[11, 12]]], 1)
    with pytest.raises(ValueError, match="req_width"):
        RS.required_search(lambda rows, step: np.zeros((len(rows), 50)), [5], 2, 0, 4, 50, required=[[list(range(10, 43))]])


class _ToyTokenizer:
    words = ["<pad>", "<bos>", "<eos>", "<unk>", "a", "dog", "dogs", "bark", "barks", "loudly"]

    def words_to_ids(self, text, skip_unknown=False):
        ids = []
        for piece in text.lower().split():
            if piece in self.words:
                ids.append(self.words.index(piece))
            elif not skip_unknown:
                raise ValueError(f"{piece!r} is not in the vocabulary")
        return ids


def test_spec_parsing():
    from conette_amd.model import required_groups
    tok = _ToyTokenizer()
    assert required_groups(tok, "dog  barks", None, 2) == [[[5], [8]], [[5], [8]]]
    assert required_groups(tok, None, None, 2) == [[], []]
    assert required_groups(tok, ["dog", 9, ["bark", "barks", "woof"]], None, 1) == [[[5], [9], [7, 8]]]
    assert required_groups(tok, None, ["dog", None, [["dogs", "dog", "dog"]]], 3) == [[[5]], [], [[6, 5]]]
    assert required_groups(tok, "", None, 1) == [[]] and required_groups(tok, [], None, 1) == [[]]
    with pytest.raises(ValueError, match="'cat'"):
        required_groups(tok, "dog cat", None, 1)
    with pytest.raises(ValueError, match="'cat'.*'cats'"):
        required_groups(tok, [["cat", "cats"]], None, 1)
    with pytest.raises(ValueError, match="exclude"):
        required_groups(tok, "dog", ["dog"], 1)
    with pytest.raises(ValueError, match="one per clip"):
        required_groups(tok, None, ["dog"], 2)
    with pytest.raises(ValueError, match="one per clip"):
        required_groups(tok, None, "dog", 3)
    with pytest.raises(ValueError, match="phrases"):
        required_groups(tok, ["a dog"], None, 1)
    with pytest.raises(ValueError, match="word or an id"):
        required_groups(tok, [1.5], None, 1)
    with pytest.raises(ValueError, match="spec"):
        required_groups(tok, 5, None, 1)


def test_cli_flag():
    from conette_amd import predict
    a = predict.get_predict_args(["--audio", "a.wav", "--require_words", "dog", "bark|barks"])
    assert a.require_words == ["dog", "bark|barks"]
    assert predict.get_predict_args(["--audio", "a.wav"]).require_words is None
    with pytest.raises(ValueError, match="--sample"):
        predict.get_predict_args(["--audio", "a.wav", "--require_words", "dog", "--sample", "2"])
    with pytest.raises(ValueError, match="--beam_groups"):
        predict.get_predict_args(["--audio", "a.wav", "--require_words", "dog", "--beam_groups", "3"])


# ---- 4. the library and the header -------------------------------------------------------------------------------------------------------
def test_library_exports_and_header_declares_the_entry_points():
    import __graft_entry__ as ge
    ge.build()
    from conette_amd import engine
    lib = engine.load_library()
    text = open(os.path.join(ROOT, "include", "conette_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("conette_decode_required_workspace_bytes", "conette_decode_required"):
        assert hasattr(lib, name) and name in engine.EXPORTS and re.search(r"\b" + name + r"\s*\(", hdr), name
    assert "#define CONETTE_ABI_VERSION 3" in text
    assert lib.conette_abi_version() == 3
    for word in ("req_tokens", "req_groups", "req_width", "M4", "M5", "round-robin", "bank"):
        assert word in text, word
