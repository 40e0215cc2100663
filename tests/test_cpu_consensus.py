"""CPU: the consensus rule (conette_amd/consensus.py) -- against an independent restatement, hand values, its properties, its fp32
emulation against float64, the arguments it refuses; the header, the export list, the built library and the CLI flags."""
import collections
import ctypes
import os
import re

import numpy as np
import pytest

from conette_amd import consensus as C
from tests import consensus_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- an independent restatement: collections.Counter for the n-grams, the textbook full-matrix Levenshtein ------------------------
def ref_content(row, length, eos=K.EOS, pad=K.PAD):
    row = [int(t) for t in row]
    if length is None:
        stops = [k for k, t in enumerate(row) if t in (eos, pad)]
        return row[:stops[0]] if stops else row
    c = row[:length]
    return c[:-1] if c[-1:] == [eos] else c


def ref_lev(a, b):
    d = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
    for i in range(len(a) + 1):
        d[i][0] = i
    for j in range(len(b) + 1):
        d[0][j] = j
    for i in range(1, len(a) + 1):
        for j in range(1, len(b) + 1):
            d[i][j] = min(d[i - 1][j] + 1, d[i][j - 1] + 1, d[i - 1][j - 1] + (0 if a[i - 1] == b[j - 1] else 1))
    return d[len(a)][len(b)]


def ref_utility(a, b, kind, order):
    if kind == "edit":
        return 1.0 if not a and not b else 1.0 - ref_lev(a, b) / max(len(a), len(b))
    fs = []
    for n in range(1, order + 1):
        ga = collections.Counter(tuple(a[k:k + n]) for k in range(len(a) - n + 1))
        gb = collections.Counter(tuple(b[k:k + n]) for k in range(len(b) - n + 1))
        t = sum(ga.values()) + sum(gb.values())
        if t:
            fs.append(2.0 * sum((ga & gb).values()) / t)
    return sum(fs) / len(fs) if fs else 1.0


@pytest.fixture(scope="module")
def clips():
    """every clip of the table once per distinct content list: (name, contents)"""
    seen, out = set(), []
    for name, preds, lens, _ in K.cases():
        for b in range(preds.shape[0]):
            cs = [ref_content(preds[b, i], None if lens is None else int(lens[b, i])) for i in range(preds.shape[1])]
            assert cs == C.contents(preds[b], None if lens is None else lens[b], K.EOS, K.PAD), (name, b)
            key = tuple(tuple(c) for c in cs)
            if key not in seen:
                seen.add(key)
                out.append((f"{name}[{b}]", cs))
    return out


def test_lens_and_pads_give_the_same_contents():
    by = {name: (p, l) for name, p, l, _ in K.cases()}
    for name, (p, l) in by.items():
        if l is not None:
            q, none = by[name.replace("_lens_", "_pads_")]
            assert none is None and q is p
            for b in range(p.shape[0]):
                assert C.contents(p[b], l[b], K.EOS, K.PAD) == C.contents(p[b], None, K.EOS, K.PAD)


def test_table_holds_the_planted_cases():
    shapes = {tuple(p.shape) for _, p, _, _ in K.cases()}
    assert shapes == set(K.SHAPES) and len(K.cases()) == len(K.SHAPES) * 2 * 4
    big = [p for name, p, _, _ in K.cases() if "_big_" in name]
    ids = set(int(t) for p in big for t in p.ravel())
    assert 2 ** 31 - 1 in ids and {(1 << 16) + 5, (1 << 17) + 5} <= ids and min(ids - {K.EOS, K.PAD}) >= 65536
    for name, p, l, _ in K.cases():
        b, n, width = p.shape
        if l is None:
            continue
        cs = [C.contents(p[k], l[k], K.EOS, K.PAD) for k in range(b)]
        if n >= 6:
            assert cs[0][0] == cs[0][1] and cs[0][n - 1] == cs[0][n // 2], name               # duplicates, adjacent and far apart
            assert sum(1 for x, y in zip(cs[0][0], cs[0][2]) if x != y) <= 1 and len(cs[0][0]) == len(cs[0][2])   # one token apart
            assert len(cs[0][3]) == width and int(l[0, 3]) == width                          # full length, no <eos>
            assert cs[0][4] == [] and cs[0][n - 2] == [] and int(l[0, 4]) == 1                # only <eos>
        if b >= 2:
            assert all(c == cs[b - 1][0] for c in cs[b - 1]) and cs[b - 1][0], name           # all identical
        if b >= 3:
            assert all(c == [] for c in cs[b - 2]), name                                     # all empty
        assert len({int(v) for v in l.ravel()}) > 1 or n * b == 1, name                       # ragged


def test_utility_equals_the_restatement_on_the_whole_table(clips):
    for name, cs in clips:
        for kind, order in K.SETTINGS:
            for i in range(len(cs)):
                for j in range(i, len(cs)):
                    got, want = C.utility(cs[i], cs[j], kind, order), ref_utility(cs[i], cs[j], kind, order)
                    assert got == pytest.approx(want, rel=0, abs=1e-15), (name, kind, order, i, j)
                    assert 0.0 <= got <= 1.0
                    if i == j:
                        assert got == 1.0


def test_all_pairs_path_equals_the_pairwise_functions(clips):
    """select / select_fp32 run on numpy-over-pairs integers: the same m_n, t_i + t_j and distances as the functions above"""
    for name, cs in clips:
        match, both = C.ngram_matches(cs, 4)
        lev, longer = C.levenshtein_all(cs)
        for i in range(len(cs)):
            for j in range(len(cs)):
                for n in range(1, 5):
                    assert (int(match[n - 1, i, j]), int(both[n - 1, i, j])) == C.ngram_match(cs[i], cs[j], n), (name, i, j, n)
                if i <= j:
                    assert int(lev[i, j]) == int(lev[j, i]) == ref_lev(cs[i], cs[j]), (name, i, j)
                assert int(longer[i, j]) == max(len(cs[i]), len(cs[j]))


def test_select_is_utility_expected_and_first_maximum():
    for name, preds, lens, weights in K.cases():
        if preds.shape[1] > 17:
            continue
        for kind, order in K.SETTINGS:
            for b in range(preds.shape[0]):
                r = C.select(preds[b], None if lens is None else lens[b], None if weights is None else weights[b], kind, order, K.EOS, K.PAD)
                cs = C.contents(preds[b], None if lens is None else lens[b], K.EOS, K.PAD)
                n = len(cs)
                u = np.array([[C.utility(cs[i], cs[j], kind, order) for j in range(n)] for i in range(n)])
                assert np.array_equal(r["pairwise"], u) and np.array_equal(u, u.T), (name, kind, b)
                w = (np.full(n, np.float32(1) / np.float32(n)) if weights is None else
                     (weights[b] / weights[b].sum()).astype(np.float32)).astype(np.float64)
                assert np.array_equal(r["expected"], C.expected(u, w))
                np.testing.assert_allclose(r["expected"], u @ w, rtol=0, atol=1e-14)
                e = r["expected"]
                assert r["best"] == int(np.flatnonzero(e == e.max())[0])
                assert r["margin"] == (np.inf if n == 1 else e[r["best"]] - np.delete(e, r["best"]).max())


def test_hand_values():
    f = C.utility
    assert f([5, 6, 7], [5, 6, 8], "ngram", 2) == pytest.approx(7 / 12, abs=1e-15)
    assert f([5, 6, 7], [5, 6, 8], "edit") == pytest.approx(2 / 3, abs=1e-15)
    assert C.ngram_match([5, 5, 5], [5, 9], 1) == (1, 5) and f([5, 5, 5], [5, 9], "ngram", 1) == pytest.approx(2 / 5, abs=1e-15)
    assert f([5], [5, 6, 7], "ngram", 4) == pytest.approx(1 / 6, abs=1e-15)
    for kind in ("ngram", "edit"):
        assert f([], [5], kind) == 0.0 and f([5], [], kind) == 0.0 and f([], [], kind) == 1.0


def test_properties():
    rng = np.random.default_rng(5)
    for _ in range(200):
        a = [int(t) for t in rng.integers(4, 9, size=rng.integers(0, 9))]
        b = [int(t) for t in rng.integers(4, 9, size=rng.integers(0, 9))]
        for kind, order in K.SETTINGS:
            assert C.utility(a, b, kind, order) == C.utility(b, a, kind, order)
            assert C.utility(a, a, kind, order) == 1.0
    for fn in (C.select, C.select_fp32):
        one = fn(np.array([[7, 8, 2, 0]]), utility="edit")
        assert one["best"] == 0 and one["margin"] == np.inf and one["expected"].tolist() == [1.0]
        # candidates 1 and 3 are the same caption and tie: the lower index wins, the margin is 0
        r = fn(np.array([[9, 9, 9, 2], [4, 5, 6, 2], [9, 2, 0, 0], [4, 5, 6, 2]]))
        assert r["best"] == 1 and r["margin"] == 0 and r["expected"][1] == r["expected"][3]


def test_fp32_rule_against_float64_on_the_table():
    worst = 0.0
    for name, preds, lens, weights in K.cases():
        for kind, order in K.SETTINGS:
            kw = dict(utility=kind, max_order=order, eos_id=K.EOS, pad_id=K.PAD)
            a = C.select_batch(preds, lens, weights, **kw)
            f = C.select_batch(preds, lens, weights, fp32=True, **kw)
            assert f["expected"].dtype == np.float32 and f["pairwise"].dtype == np.float32 and f["margin"].dtype == np.float32
            dev = float(np.abs(f["expected"].astype(np.float64) - a["expected"]).max())
            worst = max(worst, dev)
            assert dev <= 2.0 ** -17, (name, kind, order, dev)
            sure = a["margin"] > 2.0 ** -16
            assert np.array_equal(f["best"][sure], a["best"][sure]), (name, kind, order)
    print(f"fp32 rule against float64: worst deviation of E {worst:.3g} (bound {2.0 ** -17:.3g})")


def test_check_arguments_refuses():
    ok = np.zeros((2, 3, 5), dtype=np.int32)
    w, code = C.check_arguments(ok, np.full((2, 3), 5), [[1, 2, 1], [3, 3, 3]], "edit", 1)
    assert code == C.UTILITY["edit"] == 1 and C.UTILITY["ngram"] == 0 and np.allclose(w.sum(axis=1), 1) and w[0, 1] == 0.5
    bad = [
        (dict(preds=np.zeros((2, 0, 5))), "n_cands"), (dict(preds=np.zeros((2, 65, 5))), "n_cands"),
        (dict(preds=np.zeros((2, 3, 0))), "row_len"), (dict(preds=np.zeros((2, 3, 65))), "row_len"),
        (dict(max_order=0), "max_order"), (dict(max_order=5), "max_order"), (dict(utility="bleu"), "utility"),
        (dict(weights=[[1, 0, 1], [1, 1, 1]]), "weights"), (dict(weights=[[1, -1, 1], [1, 1, 1]]), "weights"),
        (dict(weights=[[1, float("nan"), 1], [1, 1, 1]]), "weights"), (dict(weights=[[1, float("inf"), 1], [1, 1, 1]]), "weights"),
        (dict(weights=[1, 1, 1]), "weights"), (dict(weights=np.ones((2, 4))), "weights"),
        (dict(lens=np.full((2, 3), 6)), "lens"), (dict(lens=np.full((2, 3), -1)), "lens"), (dict(lens=np.zeros((2, 2))), "lens"),
    ]
    for change, word in bad:
        kw = dict(preds=ok, lens=None, weights=None, utility="ngram", max_order=4)
        kw.update(change)
        with pytest.raises(ValueError, match=word):
            C.check_arguments(**kw)
    assert C.MAX_CANDS == 64 and C.MAX_PRED == 64


def test_header_exports_and_library():
    hdr = open(os.path.join(ROOT, "include", "conette_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+conette_consensus\s*\(", code)
    for name, value in (("CONETTE_UTILITY_NGRAM", 0), ("CONETTE_UTILITY_EDIT", 1), ("CONETTE_MAX_CANDS", C.MAX_CANDS)):
        assert re.search(rf"#define\s+{name}\s+{value}\b", code), name
    assert re.search(r"#define\s+CONETTE_ABI_VERSION\s+3\b", code)
    from conette_amd import engine
    assert "conette_consensus" in engine.EXPORTS
    import __graft_entry__ as ge
    ge.build()
    lib = engine.load_library()
    assert hasattr(lib, "conette_consensus") and lib.conette_abi_version() == 3
    assert isinstance(ctypes.CDLL(engine.LIB_PATH).conette_consensus, ctypes._CFuncPtr)


def test_cli_flags():
    from conette_amd.predict import get_predict_args
    a = get_predict_args(["--audio", "a.wav", "--sample", "8", "--consensus", "edit"])
    assert a.consensus == "edit" and a.consensus_order == 4 and a.sample == 8
    a = get_predict_args(["--audio", "a.wav", "--sample", "8", "--consensus", "ngram", "--consensus_order", "2"])
    assert a.consensus == "ngram" and a.consensus_order == 2
    assert get_predict_args(["--audio", "a.wav", "--sample", "8"]).consensus is None
    with pytest.raises(ValueError, match="--sample"):
        get_predict_args(["--audio", "a.wav", "--consensus", "ngram"])
    with pytest.raises(ValueError, match="--consensus"):
        get_predict_args(["--audio", "a.wav", "--consensus_order", "2"])
    with pytest.raises(ValueError, match="max_order"):
        get_predict_args(["--audio", "a.wav", "--sample", "4", "--consensus", "ngram", "--consensus_order", "5"])
    with pytest.raises(ValueError, match="n_cands"):
        get_predict_args(["--audio", "a.wav", "--sample", "65", "--consensus", "ngram"])
    with pytest.raises(SystemExit):
        get_predict_args(["--audio", "a.wav", "--sample", "4", "--consensus", "bleu"])
