"""GPU: the Python surface of caption scoring -- CoNeTTEModel.score_captions and BaselinePLM.score_captions -- against the
reference's own forcing logits (tests/golden/forcing/forcing_ragged.npz -> CrossEntropyLossMean, restated in
tests/test_cpu_scoring.py), and the shape / task / pairwise contracts."""
import json
import os

import numpy as np
import pytest
import torch

from conette_amd import scoring, synth
from tests import golden_util as G
from tests.test_cpu_scoring import reference_losses

pytestmark = pytest.mark.gpu
TAGS = {i: f"tag{i}" for i in range(527)}


@pytest.fixture(scope="module")
def model_fp32(tmp_path_factory):
    from conette_amd import CoNeTTEConfig, CoNeTTEModel
    model_dir = synth.write_pretrained_dir(str(tmp_path_factory.mktemp("conette_synth_score")))
    config = CoNeTTEConfig.from_pretrained(model_dir)
    return CoNeTTEModel.from_pretrained(model_dir, config=config, precision="fp32", offline=True, audioset_idx_to_name=TAGS,
                                        stopwords=synth.synth_stopwords())


@pytest.fixture(scope="module")
def ragged():
    g = np.load(os.path.join(G.GOLDEN, "forcing", "forcing_ragged.npz"))
    pre = {"audio": torch.from_numpy(g["frame_embs"]), "audio_shape": torch.from_numpy(g["audio_shape"])}
    caps = torch.from_numpy(g["caps_in"])                      # (3, 10): task token, words, pads -- used as FULL captions here
    return g, pre, caps


def loss_bound(logits_bvl, targets, rtol, atol):
    """The bound on a caption's loss that follows from a logit bound (rtol, atol): per token, once at the target's logit and once
    at the position's largest |logit| (lp = z_t - lse(z), |d lse| <= max |d z|); the loss is the mean over the scored tokens."""
    z = logits_bvl.double().permute(0, 2, 1)
    zt = z.gather(2, targets.long()[..., None])[..., 0].abs()
    per_tok = (atol + rtol * zt) + (atol + rtol * z.abs().amax(dim=-1))
    keep = targets != 0
    return (per_tok * keep).sum(dim=1) / keep.sum(dim=1)


def test_losses_match_the_references_forcing_logits(model_fp32, ragged):
    g, pre, caps = ragged
    _, targets = scoring.split_captions(caps, 0)
    ref_logits = torch.from_numpy(g["logits"])[:, :, :9]
    losses_ref = reference_losses(ref_logits, targets)
    out = model_fp32.score_captions(pre, caps, preprocess=False)
    assert tuple(out["lprobs"].shape) == (3, 1, 9) and tuple(out["losses"].shape) == (3, 1) and out["loss"].ndim == 0
    assert out["n_tokens"].cpu().tolist() == [[9], [5], [3]]
    err = (out["losses"][:, 0].cpu().double() - losses_ref).abs()
    bound = loss_bound(ref_logits, targets, 1e-3, 2e-3)       # the fixture test's bound on embeddings input
    print(f"score_captions fp32 vs the reference's losses {losses_ref.tolist()}: max err {float(err.max()):.3e}, bound {bound.tolist()}")
    assert bool((err <= bound).all()), (err.tolist(), bound.tolist())
    assert float(out["loss"]) == float(out["losses"].mean())
    np.testing.assert_allclose(out["losses"].cpu().numpy(), (-out["sum_lprobs"] / out["n_tokens"]).cpu().numpy(), rtol=1e-6)
    assert bool((out["lprobs"].cpu()[:, 0][targets == 0] == 0).all())


def test_shapes_tasks_and_the_bos_check(model_fp32, ragged):
    g, pre, caps = ragged
    one = model_fp32.score_captions(pre, caps, preprocess=False)
    other = caps.clone()
    other[:, 1] = caps[:, 2]                                   # another word at position 1: another caption
    both = model_fp32.score_captions(pre, torch.stack([caps, other], dim=1), preprocess=False)
    assert tuple(both["losses"].shape) == (3, 2) and tuple(both["sum_lprobs"].shape) == (3, 2) and tuple(both["n_tokens"].shape) == (3, 2)
    assert tuple(both["lprobs"].shape) == (3, 2, 9)
    np.testing.assert_allclose(both["losses"][:, 0].cpu().numpy(), one["losses"][:, 0].cpu().numpy(), rtol=0, atol=1e-5)
    assert not torch.allclose(both["losses"][:, 1], both["losses"][:, 0])
    # waveform input: <bos> in column 0 + task= scores like the task token in place
    n = [int(v) for v in g["lengths"]]
    wav = synth.synth_waveforms(len(n), max(n), int(g["seed0"]), lengths=n)
    x = [torch.from_numpy(wav[i, : n[i]].copy())[None, :] for i in range(len(n))]
    tasks = json.loads(str(g["tasks"]))
    with_bos = caps.clone()
    with_bos[:, 0] = model_fp32.tokenizer.bos_token_id
    a = model_fp32.score_captions(x, with_bos, sr=32000, task=tasks)
    b = model_fp32.score_captions(x, caps, sr=32000)
    assert torch.equal(a["lprobs"], b["lprobs"]) and torch.equal(a["losses"], b["losses"])
    _, targets = scoring.split_captions(caps, 0)
    ref_logits = torch.from_numpy(g["logits"])[:, :, :9]
    err = (a["losses"][:, 0].cpu().double() - reference_losses(ref_logits, targets)).abs()
    assert bool((err <= loss_bound(ref_logits, targets, 2e-3, 5e-3)).all()), err.tolist()   # the waveform bound of test_model_teacher_forcing_api
    with pytest.raises(ValueError) as e:
        model_fp32.score_captions(pre, with_bos, preprocess=False)
    assert str(e.value) == "BOS was not replaced in input captions for decode_method='forcing'."
    with pytest.raises(ValueError, match="Invalid number of captions"):
        model_fp32.score_captions(pre, caps[:2], preprocess=False)
    with pytest.raises(ValueError, match="n_tokens == 0"):      # a caption of a first token and pads has no loss
        model_fp32.score_captions(pre, torch.tensor([[5624, 0, 0]] * 3), preprocess=False)


def test_pairwise_matrix(model_fp32, ragged):
    """M = 5 captions over B = 3 clips: row by row equal to five calls of one caption per clip; and among the captions the model
    itself generated for the three clips (beam 1), each clip's own has the lowest loss of its row -- a condition on the inputs
    that the CPU oracle confirms for this fixture (every row of the oracle's 3 x 3 loss matrix has its minimum on the diagonal)."""
    g, pre, caps = ragged
    extra = caps[:2].clone()
    extra[:, 1:3] = caps[:2, 1:3].flip(1)
    caps5 = torch.cat([caps, extra])
    mat = model_fp32.score_captions(pre, caps5, preprocess=False, pairwise=True)
    assert tuple(mat["losses"].shape) == (3, 5) and tuple(mat["lprobs"].shape) == (3, 5, 9)
    for j in range(5):
        col = model_fp32.score_captions(pre, caps5[j][None].expand(3, -1), preprocess=False)
        np.testing.assert_allclose(mat["losses"][:, j].cpu().numpy(), col["losses"][:, 0].cpu().numpy(), rtol=0, atol=1e-5)
        np.testing.assert_allclose(mat["lprobs"][:, j].cpu().numpy(), col["lprobs"][:, 0].cpu().numpy(), rtol=0, atol=1e-5)
    gen = model_fp32(pre["audio"], x_shapes=pre["audio_shape"], preprocess=False, beam_size=1)
    preds = gen["preds"].cpu()
    own = torch.zeros((3, preds.shape[1] + 2), dtype=torch.long)
    own[:, 0] = model_fp32.batch_to_task_token_ids([model_fp32.default_task] * 3, [None] * 3)
    own[:, 1:-1] = preds
    for i in range(3):                                          # nothing after the first <eos>
        e = torch.nonzero(own[i] == model_fp32.tokenizer.eos_token_id).flatten()
        if len(e):
            own[i, int(e[0]) + 1:] = 0
    m3 = model_fp32.score_captions(pre, own, preprocess=False, pairwise=True)["losses"].cpu()
    print(f"pairwise losses of the model's own captions:\n{m3}")
    assert m3.argmin(dim=1).tolist() == [0, 1, 2]


def test_baseline_plm_score_captions_equals_engine_score():
    from conette_amd.baseline import BaselinePLM
    sd = synth.synth_baseline_state_dict()
    sd = {k: (torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v) for k, v in sd.items()}
    g = np.load(os.path.join(G.GOLDEN, "baseline", "baseline_b4.npz"))
    fe, shape = torch.from_numpy(G.load(str(g["src"]))["frame_embs"]), torch.from_numpy(g["audio_shape"])
    caps = torch.from_numpy(g["caps_in"])                      # (4, 20): <bos>, words, pads -- no task token in this family
    plm = BaselinePLM(sd, beam_size=3, max_pred_size=20, precision="bf16")
    out = plm.score_captions({"audio": fe[:, None], "audio_shape": shape}, caps)
    caps_in, targets = scoring.split_captions(caps, plm.pad_id)
    raw = plm.engine.score(fe, shape[:, 1].int(), caps_in, targets)
    assert tuple(out["losses"].shape) == (4, 1) and tuple(out["lprobs"].shape) == (4, 1, 19)
    assert torch.equal(out["lprobs"][:, 0], raw["tok_lprobs"]) and torch.equal(out["sum_lprobs"][:, 0], raw["sum_lprobs"])
    assert torch.equal(out["n_tokens"][:, 0], raw["n_tokens"]) and bool((raw["n_tokens"] > 0).all())
    assert torch.equal(out["losses"], scoring.losses_from(out["sum_lprobs"], out["n_tokens"]))
    two = plm.score_captions({"audio": fe, "audio_shape": shape}, torch.stack([caps, caps.roll(1, 0)], dim=1))
    assert tuple(two["losses"].shape) == (4, 2) and torch.equal(two["losses"][:, 0], out["losses"][:, 0])
