"""CPU: the load addresses of the one-body depthwise kernel (cn_dwconv_ln_kernel, fp16 stream, stages 0 / 1), mirrored in Python.

The kernel reads element  b H W C + hh W C + col C + c  of x (B, H, W, C) for every halo row hh = h0 - 3 + r whose bit is set in
``rows`` and for the ten columns of its three column groups.  For every tile and every thread kind of the shapes below this file
checks that
  * every element read lies inside clip b, so inside [0, B H W C);
  * a row is read exactly when it lies in the map (no row above clip 0, none below the last clip, none of a neighbouring clip);
  * a column group that is not dropped by the pack reads exactly the halo columns w0 - 3 + q, and a dropped group covers exactly
    the columns outside the map (so dropping it is the zero padding);
  * the launcher sends every other width to the clamped body.
The expressions mirrored here are held to the source text, so an edit of the kernel's index arithmetic fails this file until the
mirror is revisited.
"""
import os
import re

import pytest

from tests import encoder_geometry as E

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "conette-audio-captioning_amd", "csrc", "encoder.hip")

# (C, S, TH, W) of the two launches (encoder.hip dwconv_dispatch, 16-bit precisions)
STAGES = ((96, 2, E.CN_DW96_TH, 56), (192, 1, E.CN_DW192_TH, 28))
# stage-0 heights of tests/test_gpu_dwconv_edge_paths.py and the small heights no clip can reach, + the benchmark's 10 s clips
H0S = (1, 2, 3, 4, 8, 9, 11, 12, 13, 15, 24, 25, 27)


def _shapes():
    out = []
    for h0 in H0S:
        for st, (c, s, th, w) in enumerate(STAGES):
            h = h0 >> st
            if h >= 1:
                out.append((2, h, w, c, s, th))
    _, hs, _ = E.geometry(E.TEN_S)
    for st, (c, s, th, w) in enumerate(STAGES):
        out.append((E.BENCH_BATCH, hs[st], w, c, s, th))
    return out


def one_body(w, c, s):
    """launch_dwconv: the widths that run the one-body kernel"""
    return c <= 192 and w % (4 * s) == 0 and w >= 12


def row_mask(h, th, h0):
    """the kernel's ``rows``"""
    return ((1 << min(th + 6, h + 3 - h0)) - 1) & ~((1 << max(0, 3 - h0)) - 1)


def thread_columns(w, w0):
    """(column read, dropped by the pack) for q = 0 .. 9: the kernel's oL / oM / oR and selL / selR"""
    left, right = w0 == 0, w0 + 7 > w
    o_l = 0 if left else w0 - 3
    o_m = w0
    o_r = w0 + 1 if right else w0 + 4
    cols = [o_l + q for q in range(3)] + [o_m + q for q in range(4)] + [o_r + q for q in range(3)]
    drop = [left] * 3 + [False] * 4 + [right] * 3
    return cols, drop


def test_the_mirror_is_the_source():
    src = open(SRC).read()
    for text in (
        "const bool left = (w0 == 0), right = (w0 + 7 > W);",
        "oL = 2u * (unsigned)((left ? 0 : w0 - 3) * C + c), oM = 2u * (unsigned)(w0 * C + c);",
        "oR = 2u * (unsigned)((right ? w0 + 1 : w0 + 4) * C + c);",
        "selL = left ? SEL_ZERO : SEL_PAIR, selR = right ? SEL_ZERO : SEL_PAIR;",
        "const unsigned rows = ((1u << min(TH + 6, H + 3 - h0)) - 1u) & ~((1u << max(0, 3 - h0)) - 1u);",
        "const bool rows_in = (h0 >= 3) && (h0 + TH + 3 <= H);",
        "q < 3 ? xr + (size_t)oL + q * C * 2 : q < 7 ? xr + (size_t)oM + (q - 3) * C * 2 : xr + (size_t)oR + (q - 7) * C * 2",
        "const char* xr = xc + (size_t)hh * W * C * 2;",
        "const char* xc = (const char*)(x + (size_t)b * H * W * C);",
        "if (W % (4 * S) == 0 && W >= 12) return launch_dwconv_as<T, XT, C, S, TH, false>(x, B, H, W, bw, y, s);",
        "const int h0 = th * TH, w0 = tw * (4 * S) + sidx * 4;",
    ):
        assert text in src, text
    assert re.search(r"if \(!CHECK \|\| \(\(rows >> r\) & 1u\)\)", src)


@pytest.mark.parametrize("shape", _shapes(), ids=lambda s: "B%d_H%d_W%d_C%d" % s[:4])
def test_every_load_lies_in_its_clip(shape):
    b_n, h, w, c_n, s, th = shape
    assert one_body(w, c_n, s)
    tiles_h, tiles_w = -(-h // th), -(-w // (4 * s))
    size = b_n * h * w * c_n
    lo, hi = size, -1
    kinds = set()
    for t_h in range(tiles_h):
        h0 = t_h * th
        mask = row_mask(h, th, h0)
        rows_in = h0 >= 3 and h0 + th + 3 <= h
        rows = [r for r in range(th + 6) if rows_in or (mask >> r) & 1]
        # a row is read exactly when it lies in the map
        assert rows == [r for r in range(th + 6) if 0 <= h0 - 3 + r < h], (shape, h0)
        for t_w in range(tiles_w):
            for sidx in range(s):
                w0 = t_w * 4 * s + sidx * 4
                cols, drop = thread_columns(w, w0)
                kinds.add((drop[0], drop[9]))
                assert not (drop[0] and drop[9])
                for q in range(10):
                    true_col = w0 - 3 + q
                    assert 0 <= cols[q] < w, (shape, w0, q)
                    if drop[q]:
                        assert not 0 <= true_col < w, (shape, w0, q)      # dropped = outside: the zero padding
                    else:
                        assert cols[q] == true_col, (shape, w0, q)        # kept = the halo column itself
                for b in (0, b_n - 1):
                    for r in (rows[0], rows[-1]):
                        for c in (0, c_n - 1):
                            offs = [(b * h + h0 - 3 + r) * w * c_n + col * c_n + c for col in cols]
                            assert b * h * w * c_n <= min(offs) and max(offs) < (b + 1) * h * w * c_n, (shape, b, h0, w0, r)
                            lo, hi = min(lo, min(offs)), max(hi, max(offs))
    assert kinds == {(False, False), (True, False), (False, True)}
    assert 0 <= lo and hi < size
    assert lo == 0 and hi == size - 1    # the first and the last element of x are read, nothing beyond


def test_other_widths_run_the_clamped_body():
    for c, s, _, _ in STAGES:
        for w in range(1, 12):
            assert not one_body(w, c, s), (c, w)           # narrower than the halo: both sides outside for one thread
        assert not one_body(4 * s * 3 + 4 * s // 2 + 1, c, s)   # not whole tiles across the width
    assert not one_body(56, 384, 1) and not one_body(28, 768, 1)   # the deep stages' tiled fallback keeps the clamped body
    assert one_body(56, 96, 2) and one_body(28, 192, 1)


def test_no_clip_is_shorter_than_eight_rows():
    """encode rejects clips below 7680 samples, so the stage-0 map has at least 8 rows and the stage-1 map at least 4: the
    heights 1-4 (stage 0) and 1-3 (stage 1) are covered by the arithmetic above and cannot be run on a device."""
    assert "need >= 7680 samples" in open(SRC).read()
    _, hs, _ = E.geometry(7680)
    assert hs[0] == 8 and hs[1] == 4
