"""CPU: the host logic of caption scoring (conette_amd/scoring.py) and the reference arithmetic the GPU score tests rely on:
the reference's per-caption loss -- CrossEntropyLossMean(ignore_index=pad_id, dim=1) over forcing logits
(pl_modules/conette.py:233-256, nn/loss/ce_mean.py:30-34) -- restated with torch on logits the reference wrote itself
(tests/golden/forcing/forcing_ragged.npz) and on the oracle's."""
import os

import numpy as np
import pytest
import torch

from conette_amd import scoring
from tests import golden_util as G

PAD, BOS, EOS = 0, 1, 2


def reference_losses(logits_bvl: torch.Tensor, targets: torch.Tensor, pad_id: int = PAD) -> torch.Tensor:
    """CrossEntropyLossMean(ignore_index=pad_id, dim=1): cross_entropy(reduction="none") of (B, V, L) logits, summed over the
    caption and divided by the number of non-pad targets (ce_mean.py:30-34)."""
    ce = torch.nn.functional.cross_entropy(logits_bvl.double(), targets.long(), reduction="none", ignore_index=pad_id)   # (B, L)
    mask = targets != pad_id
    return (ce * mask).sum(dim=1) / mask.sum(dim=1)


def test_split_captions_2d_and_3d():
    caps = torch.tensor([[7, 5, 6, EOS, PAD], [8, 9, EOS, PAD, PAD]])
    ci, tg = scoring.split_captions(caps, PAD)
    assert ci.dtype == torch.int32 and tg.dtype == torch.int32 and ci.is_contiguous() and tg.is_contiguous()
    assert ci.tolist() == [[7, 5, 6, EOS], [8, 9, EOS, PAD]] and tg.tolist() == [[5, 6, EOS, PAD], [9, EOS, PAD, PAD]]
    caps3 = torch.stack([caps, caps.flip(0)])                  # (2, 2, 5)
    ci3, tg3 = scoring.split_captions(caps3, PAD)
    assert tuple(ci3.shape) == (2, 2, 4) and ci3.is_contiguous() and tg3.is_contiguous()
    assert torch.equal(ci3[1, 0], ci[1]) and torch.equal(tg3[1, 1], tg[0])
    with pytest.raises(ValueError, match="integer tensor"):
        scoring.split_captions(caps.float(), PAD)
    with pytest.raises(ValueError, match="no target"):
        scoring.split_captions(caps[:, :1], PAD)


def test_replace_bos():
    caps = torch.tensor([[BOS, 5, EOS], [11, 6, EOS], [BOS, 7, EOS]])
    out = scoring.replace_bos(caps, BOS, torch.tensor([20, 21, 22]))
    assert out.tolist() == [[20, 5, EOS], [11, 6, EOS], [22, 7, EOS]]       # a task token already in place is kept
    assert caps[0, 0] == BOS                                                # the input is not modified
    assert scoring.replace_bos(caps, BOS, torch.tensor(30)).tolist() == [[30, 5, EOS], [11, 6, EOS], [30, 7, EOS]]
    # (B, n_caps, L): one task id per clip
    caps3 = torch.stack([caps, caps])                                       # (2, 3, 3)
    out3 = scoring.replace_bos(caps3, BOS, torch.tensor([40, 41]))
    assert out3[0, :, 0].tolist() == [40, 11, 40] and out3[1, :, 0].tolist() == [41, 11, 41]
    assert torch.equal(out3[..., 1:], caps3[..., 1:])
    # no task: a task token everywhere passes, a <bos> raises the reference's text
    ok = torch.tensor([[11, 5, EOS], [12, 6, EOS]])
    assert torch.equal(scoring.replace_bos(ok, BOS, None), ok)
    with pytest.raises(ValueError) as e:
        scoring.replace_bos(caps, BOS, None)
    assert str(e.value) == "BOS was not replaced in input captions for decode_method='forcing'."
    # only column 0 counts
    assert scoring.replace_bos(torch.tensor([[11, BOS, EOS]]), BOS, None).tolist() == [[11, BOS, EOS]]


def test_losses_from_and_the_zero_token_caption():
    sums = torch.tensor([[-6.0, -1.5], [-8.0, 0.0]])
    cnt = torch.tensor([[3, 1], [4, 2]], dtype=torch.int32)
    assert scoring.losses_from(sums, cnt).tolist() == [[2.0, 1.5], [2.0, -0.0]]
    with pytest.raises(ValueError, match="n_tokens == 0"):
        scoring.losses_from(sums, torch.tensor([[3, 1], [0, 2]], dtype=torch.int32))


def test_pairwise_tiling():
    caps = torch.tensor([[11, 5, EOS, PAD], [12, 6, 7, EOS], [BOS, 8, EOS, PAD]])    # M = 3
    t = scoring.pairwise_captions(caps, 2)                                          # B = 2
    assert tuple(t.shape) == (2, 3, 4) and t.is_contiguous()
    for b in range(2):
        assert torch.equal(t[b], caps)
    # row p of the flattened (B * M, L) layout belongs to clip p // M and is caption p % M: conette_score's contract
    flat = t.reshape(6, 4)
    for p in range(6):
        assert torch.equal(flat[p], caps[p % 3])
    # the clip's task token goes to every <bos> of its row of the matrix
    r = scoring.replace_bos(t, BOS, torch.tensor([20, 21]))
    assert r[:, :, 0].tolist() == [[11, 12, 20], [11, 12, 21]]
    with pytest.raises(ValueError, match="pairwise"):
        scoring.pairwise_captions(t, 2)


def test_plan_chunks():
    need = lambda n, m: 1000 + 100 * n + 10 * n * m                 # monotone in both
    assert scoring.plan_chunks(5, 4, need, 10 ** 9) == [(0, 5, 0, 4)]
    plan = scoring.plan_chunks(5, 4, need, need(2, 4))              # two clips per call
    assert plan == [(0, 2, 0, 4), (2, 2, 0, 4), (4, 1, 0, 4)]
    plan = scoring.plan_chunks(2, 7, need, need(1, 3))              # one clip does not fit: slices of its captions
    assert plan == [(0, 1, 0, 3), (0, 1, 3, 3), (0, 1, 6, 1), (1, 1, 0, 3), (1, 1, 3, 3), (1, 1, 6, 1)]
    for n, m, bound in ((5, 4, need(2, 4)), (2, 7, need(1, 3)), (9, 1, need(4, 1))):
        covered = sorted((i, j) for i0, nc, j0, mc in scoring.plan_chunks(n, m, need, bound)
                         for i in range(i0, i0 + nc) for j in range(j0, j0 + mc))
        assert covered == [(i, j) for i in range(n) for j in range(m)]
        assert all(need(nc, mc) <= bound for _, nc, _, mc in scoring.plan_chunks(n, m, need, bound))
    with pytest.raises(ValueError, match="above the bound"):
        scoring.plan_chunks(2, 2, need, need(1, 1) - 1)


def test_reference_losses_on_the_references_own_logits(synth_weights):
    """The reference arithmetic of the GPU score tests, pinned on the CPU: losses from the logits the reference wrote
    (forcing_ragged.npz) equal the same from the oracle's logits to 1e-4, and -sum / n of float64 log_softmax + gather (what
    the GPU tests compare the kernel with) is the same number.  caps_in = fixture caps_in[:, :-1], targets = caps_in[:, 1:],
    logits columns 0..8 (the pass is causal: dropping the last input column changes no earlier position)."""
    from oracle import cpu_ref as O
    g = np.load(os.path.join(G.GOLDEN, "forcing", "forcing_ragged.npz"))
    caps = torch.from_numpy(g["caps_in"])
    caps_in, targets = scoring.split_captions(caps, PAD)
    assert (targets != PAD).sum(dim=1).tolist() == [9, 5, 3]         # valid lengths 10, 6, 4: every row has a target
    losses_ref = reference_losses(torch.from_numpy(g["logits"])[:, :, :9], targets)
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    logits = O.teacher_forcing(synth_weights, torch.from_numpy(g["frame_embs"]), torch.from_numpy(g["audio_shape"]), caps_in.long())
    assert tuple(logits.shape) == (3, g["logits"].shape[1], 9)
    losses_oracle = reference_losses(logits, targets)
    np.testing.assert_allclose(losses_oracle.numpy(), losses_ref.numpy(), rtol=0, atol=1e-4)
    # the same through log_softmax + gather + scoring.losses_from (the form the kernel's outputs take)
    lp = torch.log_softmax(logits.double().permute(0, 2, 1), dim=-1).gather(2, targets.long()[..., None])[..., 0]
    lp = torch.where(targets != PAD, lp, torch.zeros_like(lp))
    got = scoring.losses_from(lp.sum(dim=1), (targets != PAD).sum(dim=1))
    np.testing.assert_allclose(got.numpy(), losses_oracle.numpy(), rtol=0, atol=1e-9)
    assert torch.isfinite(losses_ref).all() and float(losses_ref.min()) > 0
