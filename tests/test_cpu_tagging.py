"""CPU: the tag timeline's rule (conette_amd/tagging.py) -- the frame rule against the recorded clip head of every golden fixture and
its window clipping; the seconds-to-frames conversions and the argument checks; the event rule against expected tables written out
here, its statements on random sequences, and its two forms against each other; the header, the export list, the built library and
the CLI flags."""
import ctypes
import os
import re

import numpy as np
import pytest

from conette_amd import tagging as R
from tests import golden_util as G
from tests import tag_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def head(synth_weights_np):
    return K.head(synth_weights_np)


# ---- the frame rule ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", G.SCENARIOS)
def test_window_over_the_clip_is_the_recorded_clip_head(name, head):
    """window 2 T - 1 and lengths T: every row is the reference's clipwise_output (rtol 1e-4, atol 1e-5: the line
    test_oracle_golden.py holds tags_probs to; measured 2.9e-7)"""
    g = G.load(name)
    fe = g["frame_embs"]
    b, t, _ = fe.shape
    p = R.frame_probs(fe, [t] * b, *head, 2 * t - 1)
    assert p.shape == (b, t, K.N_TAGS) and p.dtype == np.float64
    print(name, "largest difference", float(np.abs(p - g["tags_probs"][:, None, :]).max()))
    np.testing.assert_allclose(p, np.broadcast_to(g["tags_probs"][:, None, :], p.shape), rtol=1e-4, atol=1e-5)


def test_window_never_reads_beyond_the_length(head):
    for name, fe, lens, windows in K.frame_cases():
        poisoned = fe.copy()
        for b, n in enumerate(lens):
            poisoned[b, n:] = np.nan
        for w in windows:
            p = R.frame_probs(fe, lens, *head, w)
            assert np.array_equal(p, R.frame_probs(poisoned, lens, *head, w)), (name, w)
            for b, n in enumerate(lens):
                assert not p[b, n:].any() and np.isfinite(p[b, :n]).all() and (p[b, :n] > 0).all(), (name, w, b)
                if n > 0:       # the clip cut to T = n, alone
                    assert np.array_equal(p[b:b + 1, :n], R.frame_probs(fe[b:b + 1, :n], [n], *head, w)), (name, w, b)


def test_window_extent(head):
    """w = 1 uses frame t alone; an even w reaches one frame further to the right than to the left"""
    _, fe, _, _ = next(c for c in K.frame_cases() if c[0] == "gauss_T9_B3")
    fe, t = fe[:1], 5
    for w, (lo, hi) in ((1, (0, 0)), (2, (0, 1)), (3, (1, 1)), (4, (1, 2)), (7, (3, 3))):
        base = R.frame_probs(fe, [9], *head, w)[0, t]
        for u in range(9):
            moved = fe.copy()
            moved[0, u] += 1.0
            changed = not np.array_equal(R.frame_probs(moved, [9], *head, w)[0, t], base)
            assert changed == (t - lo <= u <= t + hi), (w, u)
    alone = R.frame_probs(fe[:, t:t + 1], [1], *head, 1)[0, 0]
    assert np.array_equal(R.frame_probs(fe, [9], *head, 1)[0, t], alone)
    # a hand computation of one row
    nw, nb, hw, hb = (np.asarray(a, dtype=np.float64) for a in head)
    x = fe[0, 4:8].astype(np.float64)       # w = 4 at t = 5: frames 4 .. 7
    v = x.max(axis=0) + x.mean(axis=0)
    z = (v - v.mean()) / np.sqrt(v.var() + 1e-6) * nw + nb
    np.testing.assert_allclose(R.frame_probs(fe, [9], *head, 4)[0, t], 1 / (1 + np.exp(-(hw @ z + hb))), rtol=1e-12, atol=0)


def test_frame_rule_refusals(head):
    fe = np.zeros((2, 3, K.FEAT), dtype=np.float32)
    for lens in ([3], [3, 4], [-1, 2]):
        with pytest.raises(ValueError, match="frame_lens"):
            R.frame_probs(fe, lens, *head, 3)
    for w in (0, 256, -1, 2.5):
        with pytest.raises(ValueError, match="window"):
            R.frame_probs(fe, [3, 3], *head, w)


# ---- conversions and checks ----------------------------------------------------------------------------------------------------------
def test_conversions_round_half_up():
    from conette_amd.alignment import FRAME_SEC
    assert FRAME_SEC == 0.32 and R.MAX_WINDOW == 255 and R.MAX_EVENTS == 64
    assert R.window_frames(2.24) == 7                                    # the public default
    # k + 1/2 frames, stated in binary fractions of a frame so that the quotient is exact: 0.32 * 2**-1 etc. are not, so go up and down
    for k in range(0, 6):
        half = (k + 0.5) * FRAME_SEC
        up, down = half * (1 + 1e-9) + 1e-12, half * (1 - 1e-9) - 1e-12
        assert R.window_frames(up) == k + 1 and R.window_frames(down) == max(1, k), k
        assert R.min_frames(up) == k + 1 and R.min_frames(down) == max(1, k), k
        assert R.gap_frames(up) == k + 1 and R.gap_frames(down) == k, k
    assert R.window_frames(0.0) == 1 and R.min_frames(0.0) == 1 and R.gap_frames(0.0) == 0
    assert R.gap_frames(0.16) == int(np.floor(0.16 / FRAME_SEC + 0.5)) == 1      # exactly half a frame goes up
    assert R.window_frames(0.48) == 2 and R.min_frames(0.8) == 3                 # 1.5 and 2.5 frames
    assert R.window_frames(10.0) == 31 and R.window_frames(81.6) == 255
    for bad in (-0.1, float("nan"), float("inf")):
        for f in (R.window_frames, R.min_frames, R.gap_frames):
            with pytest.raises(ValueError, match="seconds"):
                f(bad)


def test_check_arguments_names_the_argument():
    R.check_arguments(window=1, on=1.0, off=1e-6, min_frames=1, max_gap=0, max_events=1)
    R.check_arguments(window=255, on=0.5, off=0.5, min_frames=100, max_gap=100, max_events=64)
    R.check_arguments(on=0.3)                                             # off None: = on
    bad = [("window", 0), ("window", 256), ("window", 1.5), ("window", True), ("on", 0.0), ("on", 1.0001), ("on", float("nan")),
           ("on", float("inf")), ("on", -0.5), ("off", 0.0), ("off", 0.6), ("off", float("nan")), ("off", -float("inf")),
           ("min_frames", 0), ("min_frames", 1.5), ("max_gap", -1), ("max_gap", 0.5), ("max_events", 0), ("max_events", 65),
           ("max_events", 2.5)]
    for word, value in bad:
        with pytest.raises(ValueError, match=rf"argument {word}="):
            R.check_arguments(**{"on": 0.5, word: value})


# ---- the event rule ------------------------------------------------------------------------------------------------------------------
# per sequence of tag_cases.EVENT_CASES, per setting in its order: ([(start, end, peak_frame) of the stored events], count)
EXPECTED = {
    "lone_frame_at_on": [([(1, 2, 1)], 1), ([(1, 2, 1)], 1), ([], 0)],
    "one_ulp_below_on": [([], 0), ([], 0), ([(1, 2, 1)], 1)],
    "plateau_never_on": [([], 0), ([(1, 4, 1)], 1)],
    "plateau_on_in_last_frame": [([(1, 4, 3)], 1), ([(3, 4, 3)], 1), ([], 0)],
    "gaps_of_2_and_3": [([(0, 5, 0), (8, 9, 8)], 2), ([(0, 9, 0)], 1), ([(0, 2, 0), (4, 5, 4), (8, 9, 8)], 3),
                        ([(0, 2, 0), (4, 5, 4), (8, 9, 8)], 3)],
    "short_until_merged": [([(0, 3, 0)], 1), ([], 0), ([(0, 3, 0), (6, 7, 6)], 2)],
    "run_cut_by_n": [([(1, 3, 1)], 1), ([], 0)],
    "runs_at_0_and_at_n_minus_1": [([(0, 1, 0), (3, 4, 3)], 2), ([(0, 4, 0)], 1)],
    "n_is_0": [([], 0), ([], 0)],
    "alternating": [([(0, 1, 0)], 5), ([(0, 1, 0), (2, 3, 2), (4, 5, 4), (6, 7, 6)], 5),
                    ([(0, 1, 0), (2, 3, 2), (4, 5, 4), (6, 7, 6), (8, 9, 8)], 5), ([(0, 9, 0)], 1)],
    "nan_inside_a_run": [([(0, 1, 0), (2, 3, 2)], 2), ([(0, 3, 2)], 1)],
    "equal_peaks": [([(0, 5, 1)], 1), ([(1, 4, 1)], 1)],
    "dip_between_off_and_on": [([(0, 3, 2)], 1), ([(0, 1, 0), (2, 3, 2)], 2), ([(0, 3, 2)], 1)],
}


def bits(x):
    return np.ascontiguousarray(x).view(np.int32)


def test_handcrafted_sequences():
    assert set(EXPECTED) == {name for name, _, _, _ in K.EVENT_CASES}
    for name, p, n, settings in K.EVENT_CASES:
        assert len(settings) == len(EXPECTED[name]), name
        for s, (stored, count) in zip(settings, EXPECTED[name]):
            got = R.events(p, n, *s)
            m = s[4]
            assert got["count"] == count and len(stored) == min(count, m), (name, s)
            assert got["spans"].shape == (m, 2) and got["peaks"].shape == (m,) and got["peak_frames"].shape == (m,)
            assert got["spans"].dtype == np.int32 and got["peaks"].dtype == np.float32 and got["peak_frames"].dtype == np.int32
            k = len(stored)
            assert [tuple(r) for r in got["spans"][:k].tolist()] == [(a, e) for a, e, _ in stored], (name, s, got["spans"])
            assert got["peak_frames"][:k].tolist() == [f for _, _, f in stored], (name, s)
            assert np.array_equal(bits(got["peaks"][:k]), bits(p[[f for _, _, f in stored]])) if k else True, (name, s)
            assert (got["spans"][k:] == -1).all() and (bits(got["peaks"][k:]) == 0).all() and (got["peak_frames"][k:] == -1).all()


def test_tiling_reaches_every_lane_with_every_sequence():
    p, which = K.tiled_events_input()
    assert p.shape == (3, K.T_EVENTS, K.N_TAGS) and p.dtype == np.float32
    lane = (np.arange(3)[:, None] * K.N_TAGS + np.arange(K.N_TAGS)[None, :]) % 64
    assert len(set(zip(lane.ravel().tolist(), which.ravel().tolist()))) == 64 * len(K.EVENT_CASES)
    for b, c in ((0, 0), (1, 5), (2, 526)):
        i = which[b, c]
        s = K.EVENT_CASES[i][1]
        assert np.array_equal(bits(p[b, :len(s), c]), bits(s)) and (p[b, len(s):, c] == K.L).all()


def random_sequences(rng, count):
    for _ in range(count):
        t = int(rng.integers(1, 40))
        p = rng.choice(np.asarray([0.05, 0.2, 0.35, 0.5, 0.65, 0.8, 0.95], dtype=np.float32), size=t)
        p = (p + rng.choice(np.asarray([0, 0, 1e-3], dtype=np.float32), size=t)).astype(np.float32)
        p[rng.random(t) < 0.04] = np.nan
        on = np.float32(rng.choice([0.5, 0.65, 0.95]))
        off = np.float32(min(on, rng.choice([0.2, 0.35, 0.5, 0.95])))
        yield p, int(rng.integers(0, t + 1)), (on, off, int(rng.integers(1, 5)), int(rng.integers(0, 4)), int(rng.choice([1, 2, 4, 64])))


def test_statements_of_the_rule_on_random_sequences():
    rng = np.random.Generator(np.random.PCG64(7))
    n_events = 0
    for p, n, s in random_sequences(rng, 1500):
        on, off, shortest, gap, m = s
        got = R.events(p, n, *s)
        k = min(got["count"], m)
        assert got["count"] >= k and (got["spans"][k:] == -1).all()
        full = R.events(p, n, on, off, shortest, gap, 64)         # (no sequence of < 40 frames holds more than 64 events)
        assert full["count"] == got["count"] and np.array_equal(full["spans"][:k], got["spans"][:k])
        spans = full["spans"][:full["count"]].tolist()
        for j, (a, e) in enumerate(spans):
            n_events += 1
            assert 0 <= a < e <= n and e - a >= shortest
            if j > 0:
                assert a - spans[j - 1][1] > gap           # disjoint, ascending, further apart than the gaps merged
            inside = p[a:e]
            assert (inside >= on).any() and inside[0] >= off and inside[-1] >= off
            assert (a == 0 or not p[a - 1] >= off) and (e == n or not p[e] >= off)       # maximal
            # no frame below off except inside a merged gap: every stretch below off is at most `gap` long and strictly inside
            low = [u for u in range(a, e) if not p[u] >= off]
            for u in low:
                left = max(v for v in range(a, u) if p[v] >= off)
                right = min(v for v in range(u, e) if p[v] >= off)
                assert right - (left + 1) <= gap
            f = int(full["peak_frames"][j])
            assert a <= f < e and bits(full["peaks"][j:j + 1])[0] == bits(p[f:f + 1])[0]
            assert p[f] == np.nanmax(inside) and not (inside[:f - a] == p[f]).any()
        # and nothing that qualifies is missing: a frame >= on lies in an event unless its merged event was too short
        if shortest == 1:
            for u in range(n):
                if p[u] >= on:
                    assert any(a <= u < e for a, e in spans)
    assert n_events > 1000       # (the properties were not checked on nothing)


def test_batch_form_equals_the_sequence_form():
    rng = np.random.Generator(np.random.PCG64(8))
    for trial in range(40):
        b, t, c = int(rng.integers(1, 4)), int(rng.integers(1, 30)), int(rng.integers(1, 9))
        p = rng.random((b, t, c)).astype(np.float32)
        p[rng.random(p.shape) < 0.05] = np.nan
        lens = rng.integers(0, t + 1, b)
        on = np.float32(rng.choice([0.5, 0.7, 0.9]))
        s = (on, np.float32(min(on, rng.choice([0.3, 0.45, 0.9]))), int(rng.integers(1, 4)), int(rng.integers(0, 4)), int(rng.choice([1, 2, 64])))
        whole = R.events_batch(p, lens, *s)
        assert whole["counts"].dtype == np.int32 and whole["counts"].shape == (b, c)
        for i in range(b):
            for j in range(c):
                one = R.events(np.ascontiguousarray(p[i, :, j]), lens[i], *s)
                assert one["count"] == whole["counts"][i, j]
                for key in ("spans", "peak_frames"):
                    assert np.array_equal(one[key], whole[key][i, j]), (trial, key)
                assert np.array_equal(bits(one["peaks"]), bits(whole["peaks"][i, j]))
    # the tiled table of the GPU test, at every length and setting it uses
    p, which = K.tiled_events_input()
    for n in K.EVENT_LENGTHS:
        for s in K.EVENT_SETTINGS[::3]:
            whole = R.events_batch(p, [n] * 3, *s)
            for i in range(len(K.EVENT_CASES)):
                one = R.events(K.padded(i), n, *s)
                b, c = np.argwhere(which == i)[0]
                assert one["count"] == whole["counts"][b, c] and np.array_equal(one["spans"], whole["spans"][b, c])


def test_event_rule_refusals():
    p = np.zeros(4, dtype=np.float32)
    with pytest.raises(ValueError, match="fp32"):
        R.events(p.astype(np.float64), 4, 0.5, 0.5)
    with pytest.raises(ValueError, match="fp32"):
        R.events_batch(np.zeros((1, 4, 2)), [4], 0.5, 0.5)
    with pytest.raises(ValueError, match="max_events"):
        R.events(p, 4, 0.5, 0.5, max_events=65)
    with pytest.raises(ValueError, match="off"):
        R.events_batch(np.zeros((1, 4, 2), dtype=np.float32), [4], 0.5, 0.6)


# ---- wiring --------------------------------------------------------------------------------------------------------------------------
NEW = ("conette_tag_frames_workspace_bytes", "conette_tag_frames", "conette_tag_events")


def test_header_exports_and_library():
    from conette_amd import engine
    text = open(os.path.join(ROOT, "include", "conette_hip.h")).read()
    for name in NEW:
        assert re.search(rf"^(size_t|int) {name}\(", text, re.M), name
        assert name in engine.EXPORTS
    assert re.search(r"#define CONETTE_TAG_MAX_WINDOW 255\b", text) and re.search(r"#define CONETTE_TAG_MAX_EVENTS 64\b", text)
    assert re.search(r"#define CONETTE_ABI_VERSION 3\b", text)
    path = os.path.join(ROOT, "conette-audio-captioning_amd", "libconette_hip.so")
    if not os.path.exists(path):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(path)
    for name in NEW:
        assert hasattr(lib, name), name
    lib.conette_abi_version.restype = ctypes.c_int
    assert lib.conette_abi_version() == 3


def test_predict_flags():
    from conette_amd import predict as P
    a = P.get_predict_args(["--audio", "a.wav", "--tag_timeline"])
    assert a.tag_timeline and (a.tag_window, a.tag_threshold, a.tag_off_threshold, a.tag_min_duration, a.tag_max_gap) == (2.24, 0.3, None, 0.0, 0.0)
    a = P.get_predict_args(["--audio", "a.wav", "--tag_timeline", "--tag_window", "1.0", "--tag_threshold", "0.5", "--tag_off_threshold", "0.2",
                            "--tag_min_duration", "0.64", "--tag_max_gap", "0.32", "--align"])
    assert (a.tag_window, a.tag_threshold, a.tag_off_threshold, a.tag_min_duration, a.tag_max_gap) == (1.0, 0.5, 0.2, 0.64, 0.32)
    assert not P.get_predict_args(["--audio", "a.wav"]).tag_timeline
    for extra, word in ((["--tag_window", "1"], "--tag_timeline"), (["--tag_timeline", "--tag_threshold", "1.5"], "on="),
                        (["--tag_timeline", "--tag_off_threshold", "0.9"], "off="), (["--tag_timeline", "--tag_window", "100"], "window="),
                        (["--tag_timeline", "--tag_max_gap", "-1"], "seconds")):
        with pytest.raises(ValueError, match=word):
            P.get_predict_args(["--audio", "a.wav"] + extra)
