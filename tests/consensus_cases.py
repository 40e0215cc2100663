"""The case table of the consensus tests (CPU and GPU): seeded, pure numpy.

Per shape (B, N, L) two alphabets: "small", 8 words (n-grams repeat inside and across candidates, so clipping matters), and "big",
ids of 65 536 and above -- two of them differ only above bit 16, two only in bit 0 at the top of the range, and 2**31 - 1 is one.
Lengths are ragged.  Planted, where the shape has room: exact duplicates, adjacent and far apart; candidates one token apart;
rows that are only <eos> (empty content), several per clip; rows of full length L without <eos>; a clip whose candidates are all
identical (margin 0, best 0: the last clip of a batch of >= 2); a clip whose candidates are all empty (the one before it, batches
of >= 3).  Each table runs with ``lens`` and without (pads after <eos>), with uniform and with given weights, for "ngram" at orders
1, 2 and 4 and for "edit"."""
import numpy as np

EOS, PAD = 2, 0
SHAPES = ((1, 1, 1), (3, 2, 5), (5, 3, 12), (2, 16, 20), (4, 13, 22), (7, 17, 31), (3, 33, 63), (2, 64, 64), (2, 64, 3), (3, 5, 64))
SMALL = np.arange(4, 12, dtype=np.int64)
BIG = np.array([65536, 65537, 65536 + 7, (1 << 16) + 5, (1 << 17) + 5, (1 << 30) + 5, 2 ** 31 - 2, 2 ** 31 - 1], dtype=np.int64)
ALPHABETS = {"small": SMALL, "big": BIG}
SETTINGS = (("ngram", 1), ("ngram", 2), ("ngram", 4), ("edit", 4))


def _row(content, l):
    """(row, len): the content, <eos> if there is room for it, pads behind"""
    row = np.full(l, PAD, dtype=np.int32)
    k = len(content)
    row[:k] = content
    if k < l:
        row[k] = EOS
        return row, k + 1
    return row, k


def table(shape, alphabet, seed=0):
    """{"preds": (B, N, L) int32, "lens": (B, N) int32, "weights": (B, N) float64, positive, not normalised}"""
    b, n, l = shape
    rng = np.random.default_rng([seed, b, n, l, len(alphabet), int(alphabet[0])])
    preds = np.zeros((b, n, l), dtype=np.int32)
    lens = np.zeros((b, n), dtype=np.int32)
    for bi in range(b):
        cs = []
        for _ in range(n):
            k = int(rng.integers(0, l + 1)) if rng.random() < 0.7 else int(rng.integers(max(l - 2, 0), l + 1))
            cs.append([int(t) for t in rng.choice(alphabet, size=k)])
        if n >= 4:
            near = list(cs[0])
            if near:
                at = int(rng.integers(0, len(near)))
                near[at] = int(alphabet[(int(np.where(alphabet == near[at])[0][0]) + 1) % len(alphabet)])
            cs[2] = near                                          # one token apart
            cs[3] = [int(t) for t in rng.choice(alphabet, size=l)]    # full length, no <eos>
        if n >= 6:
            cs[4], cs[n - 2] = [], []                             # only <eos>, twice
        if n >= 2:
            cs[1] = list(cs[0])                                   # an adjacent duplicate
            cs[n - 1] = list(cs[n // 2])                          # a far one
        if b >= 2 and bi == b - 1:
            cs = [list(cs[0] or [int(alphabet[0])][:l])] * n      # every candidate the same
        if b >= 3 and bi == b - 2:
            cs = [[] for _ in range(n)]                           # every candidate empty
        for i, c in enumerate(cs):
            preds[bi, i], lens[bi, i] = _row(c, l)
    weights = rng.uniform(0.05, 4.0, size=(b, n))
    return {"preds": preds, "lens": lens, "weights": weights}


_CACHE = {}


def cases():
    """every (name, preds, lens or None, weights or None) of the table; built once"""
    if not _CACHE:
        for shape in SHAPES:
            for aname, alphabet in ALPHABETS.items():
                t = table(shape, alphabet)
                for with_lens in (True, False):
                    for with_w in (False, True):
                        name = "B%dN%dL%d_%s_%s_%s" % (*shape, aname, "lens" if with_lens else "pads", "w" if with_w else "u")
                        _CACHE[name] = (t["preds"], t["lens"] if with_lens else None, t["weights"] if with_w else None)
    return [(k, *v) for k, v in _CACHE.items()]
