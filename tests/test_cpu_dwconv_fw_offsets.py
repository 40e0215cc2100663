"""CPU: the load addresses of the full-width depthwise kernel (cn_dwconv_ln_fw_kernel / cn_fw_conv, fp16 stream, stages 2 / 3),
mirrored in Python.

A thread (channel c, output columns OW0 .. OW0 + NOW - 1) reads the input columns Q0 .. Q1 - 1 of every halo row
hh = h0 - 3 + r whose bit is set in ``rows``, as  scalar row base (clip + hh WW C 2 bytes) + per-thread 32-bit byte offset of the
column group + immediate.  For both kernels (C = 384 in two half-width threads, C = 768), every tile of every height H2 = 2 .. 24 /
H3 = 1 .. 12 and batches of 1 to 3 this file checks that
  * every element a thread loads lies inside clip b of the stream, the first rows of clip 0 and the last rows of clip B - 1 included;
  * the row bit mask equals the range test row by row, and ``rows_in`` holds exactly when the mask is full;
  * every immediate is within 0 .. 4095 and every per-thread offset plus immediate is below 2^32;
  * the column groups reproduce the columns Q0 .. Q1 - 1 in order, all of them inside the map.
The expressions mirrored here are held to the source text, so an edit of the kernel's index arithmetic fails this file until the
mirror is revisited.
"""
import os

import pytest

from tests import encoder_geometry as E

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "conette-audio-captioning_amd", "csrc", "encoder.hip")

# (C, WW, TH, ((OW0, NOW) of each thread kind), heights): encoder.hip launch_dwconv_fw<.., 384, 14, CN_FW_TH, CN_FW_SPLIT = 2> and <.., 768, 7, 4>
KERNELS = (
    (384, 14, E.CN_FW_TH, ((0, 7), (7, 7)), range(2, 25)),
    (768, 7, E.FW768_TH, ((0, 7),), range(1, 13)),
)
BATCHES = (1, 2, 3)
IMM_MAX = 4095           # the 13-bit signed immediate of a global load, non-negative half


def columns(ww, ow0, now):
    """cn_fw_conv's Q0, Q1: the input columns the outputs OW0 .. OW0 + NOW - 1 can see inside the map"""
    q0 = 0 if ow0 - 3 < 0 else ow0 - 3
    q1 = ww if ow0 + now + 3 > ww else ow0 + now + 3
    return q0, q1


def groups(c_n, nq):
    """GRP, NG: columns per group (the last one's immediate still fits) and groups"""
    grp = IMM_MAX // (2 * c_n) + 1
    return grp, -(-nq // grp)


def group_offsets(c_n, q0, grp, ng, c):
    """og[g]: byte offset of a group's first column from column 0 of a row"""
    return [2 * ((q0 + g * grp) * c_n + c) for g in range(ng)]


def row_mask(h, th, h0):
    """the kernel's ``rows``"""
    return ((1 << min(th + 6, h + 3 - h0)) - 1) & ~((1 << max(0, 3 - h0)) - 1)


def test_the_mirror_is_the_source():
    src = open(SRC).read()
    for text in (
        "constexpr int Q0 = OW0 - 3 < 0 ? 0 : OW0 - 3, Q1 = OW0 + NOW + 3 > WW ? WW : OW0 + NOW + 3, NQ = Q1 - Q0;",
        "constexpr int GRP = 4095 / (2 * C) + 1, NG = (NQ + GRP - 1) / GRP;",
        "og[g] = 2u * (unsigned)((Q0 + g * GRP) * C + c);",
        "const char* xcb = (const char*)xc;",
        "const char* xr = xcb + (size_t)hh * WW * C * 2;",
        "v[q] = *(const unsigned short*)(xr + (size_t)og[q / GRP] + (q % GRP) * C * 2);",
        "const int hh = h0 - 3 + r;",
        "if (!CHECK || ((rows >> r) & 1u)) {",
        "const bool rows_in = (h0 >= 3) && (h0 + TH + 3 <= H);",
        "const unsigned rows = ((1u << min(TH + 6, H + 3 - h0)) - 1u) & ~((1u << max(0, 3 - h0)) - 1u);",
        "if (rows_in) conv(std::false_type{});",
        "const XT* xb0 = x + (size_t)b * H * WW * C;",
        "const int h0 = th * TH;",
        "cn_fw_conv<C, WW, TH, 0, WW, XT>(xb0, H, h0,",
        "cn_fw_conv<C, WW, TH, 0, WW / 2, XT>(xb0, H, h0,",
        "cn_fw_conv<C, WW, TH, WW / 2, WW / 2, XT>(xb0, H, h0,",
        "return launch_dwconv_fw<T, XT, 384, 14, CN_FW_TH, CN_FW_SPLIT>(x, B, H, bw, y, s);",
        "return launch_dwconv_fw<T, XT, 768, 7, 4>(x, B, H, bw, y, s);",
    ):
        assert text in src, text
    assert "#define CN_FW_SPLIT 2" in src and f"#define CN_FW_TH {E.CN_FW_TH} " in src


def test_the_column_groups_are_the_issue_s():
    """six + four columns at C = 384 (both halves: columns 0-9 and 4-13 of 14), 3 + 3 + 1 at C = 768 (columns 0-6 of 7)"""
    seen = []
    for c_n, ww, _, kinds, _ in KERNELS:
        for ow0, now in kinds:
            q0, q1 = columns(ww, ow0, now)
            grp, ng = groups(c_n, q1 - q0)
            seen.append((c_n, q0, q1, [min(grp, q1 - q0 - g * grp) for g in range(ng)]))
    assert seen == [(384, 0, 10, [6, 4]), (384, 4, 14, [6, 4]), (768, 0, 7, [3, 3, 1])]


@pytest.mark.parametrize("kernel", KERNELS, ids=lambda k: f"C{k[0]}")
def test_every_load_lies_in_its_clip(kernel):
    c_n, ww, th, kinds, heights = kernel
    full = (1 << (th + 6)) - 1
    n_rows_in = 0
    for h in heights:
        for b_n in BATCHES:
            size = b_n * h * ww * c_n
            lo, hi = size, -1
            for t_h in range(-(-h // th)):
                h0 = t_h * th
                mask = row_mask(h, th, h0)
                rows_in = h0 >= 3 and h0 + th + 3 <= h
                # the bit mask is the range test, row by row; the copy without row tests runs exactly where every row passes it
                for r in range(th + 6):
                    assert bool((mask >> r) & 1) == (0 <= h0 - 3 + r <= h - 1), (h, h0, r)
                assert rows_in == (mask == full), (h, h0)
                n_rows_in += rows_in
                rows = [r for r in range(th + 6) if rows_in or (mask >> r) & 1]
                assert rows and all(0 <= h0 - 3 + r < h for r in rows)
                for ow0, now in kinds:
                    q0, q1 = columns(ww, ow0, now)
                    nq = q1 - q0
                    assert 0 <= q0 and q1 <= ww                   # no column of either kernel lies outside the map
                    grp, ng = groups(c_n, nq)
                    for c in (0, 1, c_n - 1):
                        og = group_offsets(c_n, q0, grp, ng, c)
                        for b in range(b_n):
                            clip = b * h * ww * c_n * 2            # bytes: the block-uniform clip base (xb0)
                            for r in rows:
                                row = clip + (h0 - 3 + r) * ww * c_n * 2
                                elems = []
                                for q in range(nq):
                                    imm = (q % grp) * c_n * 2
                                    assert 0 <= imm <= IMM_MAX, (c_n, q, imm)
                                    assert og[q // grp] + imm < 2 ** 32
                                    addr = row + og[q // grp] + imm
                                    assert addr % 2 == 0
                                    elems.append(addr // 2)
                                # the groups reproduce columns Q0 .. Q1 - 1 of row hh, channel c, in order
                                assert elems == [((b * h + h0 - 3 + r) * ww + q0 + q) * c_n + c for q in range(nq)], (h, b, h0, r, ow0, c)
                                assert b * h * ww * c_n <= min(elems) and max(elems) < (b + 1) * h * ww * c_n, (h, b, h0, r, ow0, c)
                                lo, hi = min(lo, min(elems)), max(hi, max(elems))
            assert lo == 0 and hi == size - 1, (h, b_n)   # the first and the last element of x are read, nothing beyond
    assert n_rows_in > 0


def test_the_ten_second_map_runs_mostly_without_row_tests():
    """at 10 s, 14 of 16 tile rows of stage 2 and 6 of 8 of stage 3 hold all their halo rows"""
    _, hs, _ = E.geometry(E.TEN_S)
    for st, th, want in ((2, E.CN_FW_TH, (14, 16)), (3, E.FW768_TH, (6, 8))):
        h = hs[st]
        tiles = -(-h // th)
        inside = sum(1 for t in range(tiles) if t * th >= 3 and t * th + th + 3 <= h)
        assert (inside, tiles) == want, (st, h)
