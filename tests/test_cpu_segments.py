"""CPU: conette_amd/segments.py -- the window grid and the merge rule of the caption timeline -- against brute force and float64; the
header, the export list, the built library, the CLI flags and the argument checks of CoNeTTEModel.caption_segments / caption_spans
that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest

from conette_amd import consensus as C
from conette_amd import segments as S
from conette_amd.alignment import FRAME_SEC
from tests import span_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int32) if x.dtype == np.float32 else x


# ---- grid ----------------------------------------------------------------------------------------------------------------------------
def brute_windows(n, tw, hop):
    """windows by walking: hop forward until one reaches the end"""
    if n <= tw:
        return [(0, n)]
    out, start = [], 0
    while True:
        if start + tw >= n:
            out.append((n - tw, tw))
            return out
        out.append((start, tw))
        start += hop


def test_grid_covers_every_frame_inside_the_recording():
    n_grids = 0
    for n in range(1, 71):
        for tw in range(1, 13):
            for hop in range(1, 13):
                g = S.grid(n, tw, hop)
                want = brute_windows(n, tw, hop)
                assert g.dtype == np.int32 and g.tolist() == [list(w) for w in want], (n, tw, hop)
                assert S.n_windows(n, tw, hop) == len(want) == g.shape[0]
                assert (g[:, 0] >= 0).all() and (g[:, 0] + g[:, 1] <= n).all() and len(set(g[:, 1].tolist())) == 1
                assert g[0, 0] == 0 and g[-1, 0] + g[-1, 1] == n and (np.diff(g[:, 0]) >= 0).all()
                if hop <= tw:       # (a hop beyond the window leaves frames out by the caller's choice)
                    covered = np.zeros(n, dtype=bool)
                    for a, ln in g.tolist():
                        covered[a:a + ln] = True
                    assert covered.all(), (n, tw, hop)
                n_grids += 1
    assert n_grids == 70 * 12 * 12
    for bad in ((0, 3, 1), (5, 0, 1), (5, 3, 0)):
        with pytest.raises(ValueError, match="at least 1"):
            S.grid(*bad)


def test_span_table_is_recording_major_in_time_order():
    table, counts = S.span_table([40, 33, 17, 1], 8, 4)
    assert table.dtype == np.int32 and counts.tolist() == [9, 8, 4, 1] and table.shape == (22, 3)
    assert table[:, 0].tolist() == [0] * 9 + [1] * 8 + [2] * 4 + [3]
    for r, n in enumerate((40, 33, 17, 1)):
        assert table[table[:, 0] == r][:, 1:].tolist() == S.grid(n, 8, 4).tolist()
    assert S.check_spans(table, 4, [40, 33, 17, 1], 8) is not None


def test_seconds_round_half_up():
    assert S.window_frames(10.0) == 31 and S.hop_frames(5.0) == 16 and S.window_frames(0.0) == 1
    assert S.window_frames(2.56) == 8 and S.hop_frames(1.28) == 4 and S.window_frames(1.5 * FRAME_SEC) == 2
    assert S.run_windows(0.0, 31, 16) == 0 and S.run_windows(10.0, 31, 16) == 1 and S.run_windows(15.2, 31, 16) == 2
    assert S.run_windows(1.0, 31, 16) == 1
    assert S.seconds_to_span(0.0, 0.0) == (0, 1) and S.seconds_to_span(0.32, 2.88) == (1, 8)
    for bad in (float("nan"), -1.0, float("inf")):
        with pytest.raises(ValueError, match="seconds"):
            S.window_frames(bad)
    with pytest.raises(ValueError, match="offset before onset"):
        S.seconds_to_span(2.0, 1.0)


def test_check_spans_refuses_each_bad_row_by_name():
    lens = [40, 33, 17]
    good = [(0, 0, 8), (2, 9, 8), (1, 25, 8)]
    assert S.check_spans(good, 3, lens, 8).tolist() == [list(r) for r in good]
    for row, word in (((3, 0, 8), "recording 3"), ((-1, 0, 8), "recording -1"), ((0, -1, 8), "start -1"), ((0, 0, 0), "len 0"),
                      ((2, 10, 8), "17 valid frames"), ((0, 33, 8), "40 valid frames"), ((0, 0, 9), "t_span=8")):
        with pytest.raises(ValueError, match=rf"spans\[1\].*{word}"):
            S.check_spans([good[0], row, good[2]], 3, lens, 8)
    for table, word in ((np.zeros((0, 3), dtype=np.int32), "shape"), (np.zeros((2, 2), dtype=np.int32), "shape"),
                        (np.zeros((2, 3), dtype=np.float32), "dtype")):
        with pytest.raises(ValueError, match=word):
            S.check_spans(table, 3, lens, 8)
    with pytest.raises(ValueError, match="frame_lens"):
        S.check_spans(good, 2, lens, 8)
    with pytest.raises(ValueError, match="t_span"):
        S.check_spans(good, 3, lens, 0)


# ---- merge ---------------------------------------------------------------------------------------------------------------------------
def brute_merge(preds, lprobs, spans, kind, order, threshold, max_run):
    """the rule in float64, restated with lists: [(first, end, rep, agree, frame_start, frame_end)] and the adjacency"""
    cs = [C.content(row, None, K.EOS, K.PAD) for row in preds]
    w = len(cs)
    adj = [C.utility(cs[k], cs[k + 1], kind, order) for k in range(w - 1)]
    groups = [[0]]
    for k in range(1, w):
        if adj[k - 1] >= threshold and not (max_run and len(groups[-1]) >= max_run):
            groups[-1].append(k)
        else:
            groups.append([k])
    out = []
    for g in groups:
        finite = [k for k in g if not np.isnan(lprobs[k])]
        rep = g[0] if not finite else min(finite, key=lambda k: (-float(lprobs[k]), k))
        agree = min([adj[k] for k in g[:-1]], default=1.0)
        f0 = int(spans[0][0]) if g[0] == 0 else (int(spans[g[0]][0]) + int(spans[g[0] - 1][0]) + int(spans[g[0] - 1][1]) + 1) // 2
        f1 = int(spans[-1][0]) + int(spans[-1][1]) if g[-1] == w - 1 else \
            (int(spans[g[-1] + 1][0]) + int(spans[g[-1]][0]) + int(spans[g[-1]][1]) + 1) // 2
        out.append((g[0], g[-1] + 1, rep, agree, f0, f1))
    return out, adj


def test_merge_against_float64_brute_force():
    """wherever no adjacency lies within 2**-17 (consensus.py's fp32-to-float64 bound) of the threshold -- the tables and
    BRUTE_THRESHOLDS are built so that none does: nothing is left out"""
    n_checked, worst = 0, 0.0
    for name, preds, lprobs, spans in K.caption_tables():
        for kind, order in K.UTILITIES:
            for thr in K.BRUTE_THRESHOLDS:
                for max_run in K.MAX_RUNS:
                    want, adj64 = brute_merge(preds, lprobs, spans, kind, order, thr, max_run)
                    assert all(abs(a - thr) > 2.0 ** -17 for a in adj64), (name, kind, order, thr)
                    got = S.merge(preds, lprobs, spans, utility=kind, max_order=order, threshold=thr, max_run=max_run, max_segments=64,
                                  eos_id=K.EOS, pad_id=K.PAD)
                    assert got["adjacency"].dtype == np.float32 and got["count"] == len(want), (name, kind, thr, max_run)
                    if adj64:
                        worst = max(worst, float(np.abs(got["adjacency"].astype(np.float64) - np.asarray(adj64)).max()))
                    for i, (first, end, rep, agree, f0, f1) in enumerate(want):
                        assert got["seg_windows"][i].tolist() == [first, end] and got["seg_frames"][i].tolist() == [f0, f1]
                        assert got["seg_rep"][i] == rep, (name, i)
                        assert abs(float(got["seg_agree"][i]) - agree) <= 2.0 ** -17
                    assert (got["seg_windows"][len(want):] == -1).all() and (got["seg_rep"][len(want):] == -1).all()
                    n_checked += 1
    assert n_checked == len(K.caption_tables()) * len(K.UTILITIES) * len(K.BRUTE_THRESHOLDS) * len(K.MAX_RUNS)
    assert worst <= 2.0 ** -17


def test_adjacency_is_the_consensus_pair_utility_bit_for_bit():
    for name, preds, _, _ in K.caption_tables():
        for kind, order in K.UTILITIES:
            adj = S.adjacency(preds, kind, order, K.EOS, K.PAD)
            pair = C.select_fp32(preds, utility=kind, max_order=order, eos_id=K.EOS, pad_id=K.PAD)["pairwise"]
            want = np.asarray([pair[k, k + 1] for k in range(preds.shape[0] - 1)], dtype=np.float32)
            assert adj.dtype == np.float32 and np.array_equal(bits(adj), bits(want)), (name, kind, order)


def test_merge_batch_agrees_with_merge_on_every_setting():
    preds, n_windows, lprobs, spans = K.merge_batch_input()
    assert len(K.SETTINGS) == 3 * 3 * 3 * 2
    for (kind, order), thr, max_run, max_seg in K.SETTINGS:
        kw = dict(utility=kind, max_order=order, threshold=thr, max_run=max_run, max_segments=max_seg, eos_id=K.EOS, pad_id=K.PAD)
        got = S.merge_batch(preds, n_windows, lprobs, spans, **kw)
        assert got["adjacency"].shape == (len(n_windows), K.W_MAX - 1) and got["counts"].dtype == np.int32
        for r, (name, p, lp, sp) in enumerate(K.caption_tables()):
            one = S.merge(p, lp, sp, **kw)
            w = p.shape[0]
            assert np.array_equal(bits(got["adjacency"][r, :w - 1]), bits(one["adjacency"])) and not got["adjacency"][r, max(w - 1, 0):].any()
            assert got["counts"][r] == one["count"]
            for key in ("seg_windows", "seg_frames", "seg_rep", "seg_agree"):
                assert got[key][r].shape[0] == max_seg and np.array_equal(bits(got[key][r]), bits(one[key])), (name, key, kw)


def test_segments_tile_the_recording_and_follow_the_settings():
    for name, preds, lprobs, spans in K.caption_tables():
        w = preds.shape[0]
        for (kind, order), thr, max_run, _ in K.SETTINGS:
            m = S.merge(preds, lprobs, spans, utility=kind, max_order=order, threshold=thr, max_run=max_run, max_segments=64)
            n = m["count"]
            sw, sf = m["seg_windows"][:n], m["seg_frames"][:n]
            assert sw[0, 0] == 0 and sw[-1, 1] == w and (sw[1:, 0] == sw[:-1, 1]).all() and (sw[:, 1] > sw[:, 0]).all()
            assert sf[0, 0] == spans[0, 0] and sf[-1, 1] == spans[-1, 0] + spans[-1, 1]
            assert (sf[1:, 0] == sf[:-1, 1]).all() and (sf[:, 1] >= sf[:, 0]).all(), (name, sf)     # no gap, no overlap, monotone
            assert ((m["seg_rep"][:n] >= sw[:, 0]) & (m["seg_rep"][:n] < sw[:, 1])).all()
            if max_run:
                assert (sw[:, 1] - sw[:, 0] <= max_run).all()
            if max_run == 1:
                assert n == w and (m["seg_agree"][:n] == 1).all()
            if thr == 0.0 and max_run == 0:
                assert n == 1
            one = S.merge(preds, lprobs, spans, utility=kind, max_order=order, threshold=thr, max_run=max_run, max_segments=1)
            assert one["count"] == n and np.array_equal(one["seg_windows"][0], sw[0]) and np.array_equal(one["seg_frames"][0], sf[0])


def test_hand_values():
    by = {name: (p, lp, sp) for name, p, lp, sp in K.caption_tables()}
    m = S.merge(*by["aabba"], threshold=0.5)
    assert m["count"] == 3 and m["seg_windows"][:3].tolist() == [[0, 2], [2, 4], [4, 5]]
    assert m["adjacency"].tolist() == [1.0, 0.0, 1.0, 0.0]
    # windows (4 k, 8): window 1 ends at 12, window 2 starts at 8 -> they meet at (8 + 4 + 8 + 1) // 2 = 10
    assert m["seg_frames"][:3].tolist() == [[0, 10], [10, 18], [18, 24]] and m["seg_agree"][:3].tolist() == [1.0, 1.0, 1.0]
    m = S.merge(*by["gap_between_windows"], threshold=0.5)
    assert m["seg_frames"][:2].tolist() == [[0, 6], [6, 25]]        # (7 + 0 + 4 + 1) // 2 = 6: inside the gap
    m = S.merge(*by["lprob_ties"], threshold=0.5)
    assert m["count"] == 1 and m["seg_rep"][0] == 4                 # the first of the two largest
    m = S.merge(*by["lprob_nans"], threshold=0.5)
    assert m["seg_windows"][:3].tolist() == [[0, 3], [3, 5], [5, 6]] and m["seg_rep"][:3].tolist() == [1, 3, 5]
    m = S.merge(*by["near_pairs"], utility="ngram", max_order=1, threshold=0.7)
    assert m["adjacency"][0] == np.float32(0.75) and m["seg_windows"][:3].tolist() == [[0, 3], [3, 4], [4, 5]]
    assert m["seg_agree"][0] == np.float32(0.75)
    m = S.merge(*by["empty_contents"], threshold=1.0)
    assert m["adjacency"].tolist() == [1.0, 0.0, 0.0, 1.0]          # two empty contents agree; a row that starts with pad is empty
    m = S.merge(*by["one_window"])
    assert m["count"] == 1 and m["adjacency"].shape == (0,) and m["seg_frames"][0].tolist() == [0, 5] and m["seg_agree"][0] == 1


def test_check_arguments_refuses():
    assert S.check_arguments(8, 12, "edit", 1, 0.5, 0, 64) == 1 and S.check_arguments() == 0
    for kw, word in ((dict(row_len=0), "row_len"), (dict(row_len=65), "row_len"), (dict(w_max=0), "w_max"), (dict(w_max=4097), "w_max"),
                     (dict(utility="bleu"), "utility"), (dict(max_order=0), "max_order"), (dict(max_order=5), "max_order"),
                     (dict(threshold=float("nan")), "threshold"), (dict(threshold=float("inf")), "threshold"),
                     (dict(max_run=-1), "max_run"), (dict(max_run=1.5), "max_run"), (dict(max_segments=0), "max_segments"),
                     (dict(max_segments=257), "max_segments")):
        with pytest.raises(ValueError, match=word):
            S.check_arguments(**kw)
    preds, n_windows, lprobs, spans = K.merge_batch_input()
    with pytest.raises(ValueError, match="n_windows"):
        S.merge_batch(preds, n_windows + 1, lprobs, spans)
    with pytest.raises(ValueError, match="lprobs"):
        S.merge_batch(preds, n_windows, lprobs[:, :-1], spans)
    assert S.MAX_WINDOWS == 4096 and S.MAX_SEGMENTS == 256 and S.MAX_PRED == 64


# ---- library and host ------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("conette_decode_spans_workspace_bytes", "conette_decode_spans", "conette_segments")


def test_header_exports_and_library():
    hdr = open(os.path.join(ROOT, "include", "conette_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bsize_t\s+conette_decode_spans_workspace_bytes\s*\(", code)
    assert re.search(r"\bint\s+conette_decode_spans\s*\(", code) and re.search(r"\bint\s+conette_segments\s*\(", code)
    for name, value in (("CONETTE_SEG_MAX_WINDOWS", S.MAX_WINDOWS), ("CONETTE_SEG_MAX_SEGMENTS", S.MAX_SEGMENTS)):
        assert re.search(rf"#define\s+{name}\s+{value}\b", code), name
    assert re.search(r"#define\s+CONETTE_ABI_VERSION\s+3\b", code)
    from conette_amd import engine
    assert all(name in engine.EXPORTS for name in NEW_SYMBOLS)
    import __graft_entry__ as ge
    ge.build()
    lib = engine.load_library()
    assert lib.conette_abi_version() == 3
    raw = ctypes.CDLL(engine.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and isinstance(getattr(raw, name), ctypes._CFuncPtr), name
    assert lib.conette_decode_spans_workspace_bytes.restype is ctypes.c_size_t
    assert len(lib.conette_decode_spans.argtypes) == 20 and len(lib.conette_segments.argtypes) == 23


def test_model_argument_checks_need_no_device():
    from conette_amd.model import CoNeTTEModel
    nobody = object()       # every one of these raises before the model or the device is touched
    x = np.zeros((1, 32000), dtype=np.float32)
    for kw, word in ((dict(window_s=-1.0), "seconds"), (dict(hop_s=float("nan")), "seconds"), (dict(utility="bleu"), "utility"),
                     (dict(max_order=5), "max_order"), (dict(merge_threshold=float("inf")), "threshold"), (dict(max_segments=0), "max_segments"),
                     (dict(max_segments=257), "max_segments"), (dict(max_run_s=-2.0), "seconds")):
        with pytest.raises(ValueError, match=word):
            CoNeTTEModel.caption_segments(nobody, x, **kw)
    for spans, word in ((None, "spans"), ([], "spans"), ([[]], "recording 0 has no span"), ([[(0.0, 1.0)], [(1.0,)]], r"spans\[1\]\[0\]"),
                        ([[(2.0, 1.0)]], "offset before onset"), ([[(0.0, 1.0), (float("nan"), 1.0)]], r"spans\[0\]\[1\]")):
        with pytest.raises(ValueError, match=word):
            CoNeTTEModel.caption_spans(nobody, x, spans)
    assert CoNeTTEModel._span_list([[(0.0, 2.56), (0.32, 0.32)], [(1.0, 1.5)]]) == [[(0, 8), (1, 1)], [(3, 2)]]


def test_cli_flags():
    from conette_amd.predict import format_segments, get_predict_args
    a = get_predict_args(["--audio", "a.wav", "--segments"])
    assert a.segments and (a.segment_window, a.segment_hop, a.segment_merge) == (10.0, 5.0, 0.5)
    a = get_predict_args(["--audio", "a.wav", "--segments", "--segment_window", "4", "--segment_hop", "2", "--segment_merge", "0.25"])
    assert (a.segment_window, a.segment_hop, a.segment_merge) == (4.0, 2.0, 0.25)
    assert not get_predict_args(["--audio", "a.wav"]).segments
    with pytest.raises(ValueError, match="--segments"):
        get_predict_args(["--audio", "a.wav", "--segment_hop", "2"])
    with pytest.raises(ValueError, match="--sample"):
        get_predict_args(["--audio", "a.wav", "--segments", "--sample", "4"])
    with pytest.raises(ValueError, match="seconds"):
        get_predict_args(["--audio", "a.wav", "--segments", "--segment_window", "-1"])
    rows = format_segments(["/x/a.wav"], {"segments": [[{"onset": 0.0, "offset": 3.2, "caption": "rain", "lprob": -0.5}]]})
    assert rows == [{"audio": "a.wav", "onset": "0.00", "offset": "3.20", "caption": "rain", "lprob": "-0.5000"}]
    assert list(rows[0]) == ["audio", "onset", "offset", "caption", "lprob"]
