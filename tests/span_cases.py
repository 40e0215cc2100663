"""The tables the caption-timeline tests share (conette_amd/segments.py, csrc/dec_spans.h, csrc/dec_segments.h).

Span tables ``(name, set, spans (S, 3), t_span)`` over two recording sets of seeded frame embeddings at the encoder's scale (no
encoder needed): ``one9`` -- N = 1, t_rec = 9 -- and ``three40`` -- N = 3, t_rec = 40 with valid lengths 40, 33 and 17.  Span lengths
1, 7, 8, 9, 16, 17, 31, 33 are the 8-frame batches of the block kernel's cross-attention and their tails; each length sits at start 0,
at an odd frame and at ``len_r - len`` (ending on the recording's last valid frame) of every recording that holds it.  The rows of
different recordings are interleaved, two rows are identical, and every set comes with ``t_span`` equal to its longest span and larger.
``SEARCHES`` are the (beam, min_pred) pairs at max_pred 8: beams 1, 3 and 10 (the register-resident and the generic search step),
min_pred 0 and 3.

Caption tables ``(name, preds (W, L), lprobs (W,), spans (W, 2))`` for the merge rule: handcrafted captions over a small alphabet
(ids 4 .. 12; <eos> = 2, pad = 0), L = 8; ``merge_batch_input`` stacks them, ragged, to (N, Wmax, L).  ``SETTINGS`` is the product of
utilities x thresholds 0, 0.5, 1 x max_run 0, 1, 2 x max_segments 1, 64."""
import functools
import itertools

import numpy as np

FEAT = 768
EOS, PAD = 2, 0
GEOMETRY = "v2049_ff256_l6"      # tests/decoder_geometry.py: six layers, the fused block + FFN kernels in the 16-bit and exact precisions
MAX_PRED = 8
SEARCHES = ((1, 0), (3, 3), (10, 0), (10, 3), (3, 0))        # (beam, min_pred)
SPAN_LENGTHS = (1, 7, 8, 9, 16, 17, 31, 33)
SETS = {"one9": (9, (9,)), "three40": (40, (40, 33, 17))}    # name -> (t_rec, valid lengths)


@functools.lru_cache(maxsize=None)
def recordings(name):
    """(frame_embs (N, t_rec, 768) fp32, lens (N,) int32): uniform frames of std 0.65; frames behind a recording's length are eight
    times larger (tests/decoder_geometry.py: they must be ignored)"""
    t_rec, lens = SETS[name]
    rng = np.random.Generator(np.random.PCG64(91000 + t_rec))
    fe = ((rng.random((len(lens), t_rec, FEAT)) * 2.0 - 1.0) * (0.65 * 3 ** 0.5)).astype(np.float32)
    for r, n in enumerate(lens):
        fe[r, n:] *= 8.0
    fe.setflags(write=False)
    return fe, np.asarray(lens, dtype=np.int32)


def _rows(lens):
    """every (recording, start, len): start 0, an odd frame, and the one that ends on the last valid frame"""
    rows = []
    for ln in SPAN_LENGTHS:
        for r, n in enumerate(lens):
            if ln > n:
                continue
            odd = 3 if 3 + ln <= n else 1
            for start in sorted({0, odd, n - ln}):
                if start + ln <= n:
                    rows.append((r, start, ln))
    return rows


@functools.lru_cache(maxsize=None)
def span_tables():
    out = []
    for name, (t_rec, lens) in SETS.items():
        rows = _rows(lens)                      # length-major: the recordings interleave
        rows.insert(len(rows) // 2, rows[1])    # two identical rows, apart from each other
        table = np.asarray(rows, dtype=np.int32)
        assert len({tuple(r) for r in rows}) == len(rows) - 1
        longest = int(table[:, 2].max())
        for t_span in (longest, longest + 7):
            out.append((f"{name}_t{t_span}", name, table, t_span))
    return tuple(out)


def span_cases():
    """(table name, set, spans, t_span, beam, min_pred): every table at two searches, every search at some table"""
    tabs = span_tables()
    picks = {0: (0, 1), 1: (2, 4), 2: (1, 3), 3: (2, 4)}
    return tuple((n, s, t, ts, *SEARCHES[i]) for k, (n, s, t, ts) in enumerate(tabs) for i in picks[k])


def gather(fe, table, t_span):
    """the (S, t_span, 768) clips a table names, zeros behind a span's length, and their lengths"""
    out = np.zeros((table.shape[0], t_span, FEAT), dtype=np.float32)
    for s, (r, start, ln) in enumerate(table.tolist()):
        out[s, :ln] = fe[r, start:start + ln]
    return out, np.ascontiguousarray(table[:, 2], dtype=np.int32)


# ---- caption tables for the merge rule -----------------------------------------------------------------------------------------------
L = 8
NAN = float("nan")


def cap(*words, eos=True):
    row = list(words) + ([EOS] if eos else [])
    assert len(row) <= L
    return row + [PAD] * (L - len(row))


A = cap(4, 5, 6, 7)
B = cap(8, 9, 10, 11, 12)
A2 = cap(4, 5, 6, 9)            # three of A's four words
EMPTY = cap()
FULL = cap(4, 5, 6, 7, 8, 9, 10, 11, eos=False)     # no <eos>: the whole row counts


def windows(w, window=8, hop=4):
    """(start, len) of w windows of a regular grid"""
    return [(k * hop, window) for k in range(w)]


def _table(name, rows, lprobs=None, spans=None):
    w = len(rows)
    lp = np.asarray([-0.5 - 0.125 * ((3 * k) % 5) for k in range(w)] if lprobs is None else lprobs, dtype=np.float32)
    sp = np.asarray(windows(w) if spans is None else spans, dtype=np.int32).reshape(w, 2)
    return name, np.asarray(rows, dtype=np.int32).reshape(w, L), lp, sp


def _random_rows(w, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    rows, prev = [], None
    for _ in range(w):
        if prev is not None and rng.random() < 0.5:     # a neighbour that shares most words
            words = list(prev)
            words[int(rng.integers(len(words)))] = int(rng.integers(4, 13))
        else:
            words = [int(v) for v in rng.integers(4, 13, size=int(rng.integers(1, 8)))]
        prev = words
        rows.append(cap(*words))
    return rows


@functools.lru_cache(maxsize=None)
def caption_tables():
    return (
        _table("all_equal", [A] * 5),
        _table("all_different", [cap(4, 5), cap(6, 7), cap(8, 9), cap(10, 11), cap(12, 4, 12)]),
        _table("aabba", [A, A, B, B, A]),
        _table("near_pairs", [A, A2, A2, B, A]),
        _table("empty_contents", [EMPTY, EMPTY, A, EMPTY, cap(PAD, 4, eos=False)]),
        _table("no_eos", [FULL, FULL, cap(4, 5, 6, 7, 8, 9, 10), FULL]),
        _table("one_window", [A], spans=[(0, 5)]),
        _table("two_windows", [A, B], spans=[(0, 9), (3, 9)]),
        _table("gap_between_windows", [A, B, B], spans=[(0, 4), (7, 4), (20, 5)]),        # hop > window: boundaries inside the gaps
        _table("lprob_ties", [A] * 6, lprobs=[-1.0, -0.5, -0.5, -2.0, -0.25, -0.25]),
        _table("lprob_nans", [A, A, A, B, B, A2], lprobs=[NAN, -0.75, NAN, NAN, NAN, -0.5]),
        _table("random_12", _random_rows(12, 5)),
        _table("random_12b", _random_rows(12, 6), spans=[(3 * k, 7) for k in range(11)] + [(31, 7)]),
    )


W_MAX = 12
UTILITIES = (("ngram", 4), ("ngram", 1), ("edit", 4))
THRESHOLDS = (0.0, 0.5, 1.0)
MAX_RUNS = (0, 1, 2)
MAX_SEGMENTS = (1, 64)
SETTINGS = tuple(itertools.product(UTILITIES, THRESHOLDS, MAX_RUNS, MAX_SEGMENTS))
# thresholds of the float64 comparison: at least 2**-17 (consensus.py's fp32-to-float64 bound) away from every adjacency of the tables
BRUTE_THRESHOLDS = (0.3, 0.45, 0.9)


def merge_batch_input():
    """(preds (N, W_MAX, L), n_windows (N,), lprobs (N, W_MAX), spans (N, W_MAX, 2)): the tables stacked, ragged; what lies behind a
    table's windows is another caption, a NaN score and a span far away -- never to be read"""
    tabs = caption_tables()
    n = len(tabs)
    preds = np.tile(np.asarray(B, dtype=np.int32), (n, W_MAX, 1))
    lprobs = np.full((n, W_MAX), np.nan, dtype=np.float32)
    spans = np.full((n, W_MAX, 2), 10 ** 6, dtype=np.int32)
    n_windows = np.zeros(n, dtype=np.int32)
    for r, (_, p, lp, sp) in enumerate(tabs):
        w = p.shape[0]
        preds[r, :w], lprobs[r, :w], spans[r, :w], n_windows[r] = p, lp, sp, w
    assert n_windows.max() == W_MAX and n_windows.min() == 1
    return preds, n_windows, lprobs, spans
