"""GPU: the Python surface of the diverse beam search -- CoNeTTEModel.caption_diverse and ``conette-predict --beam_groups`` -- on
the default synthetic checkpoint with waveforms in: two clips of 1 s and 2.5 s, precision fp32, bf16 and certified (which runs
this search on its base pipeline's decoder context, with no exact re-run).

The waveform seed (0) is the first of 0, 1, 2 ... at which the CPU restatement (conette_amd/group_search.py on oracle/cpu_ref.py's
frame embeddings and decoder; G = 3, W = 1, lambda = 2) returns three different captions for each clip with every call's
effective margin above 0.04; with lambda = 0 it returns the same caption three times.  The fp32 case recomputes that here."""
import os
import wave

import numpy as np
import pytest
import torch

from conette_amd import group_search as GS
from conette_amd import synth

pytestmark = pytest.mark.gpu
TAGS = {i: f"tag{i}" for i in range(527)}
PRECS = ("fp32", "bf16", "certified")
WAVE_SEED = 0
LENGTHS = [32000, 80000]


@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    return synth.write_pretrained_dir(str(tmp_path_factory.mktemp("conette_synth_groups")))


@pytest.fixture(scope="module", params=PRECS)
def model(request, model_dir):
    from conette_amd import CoNeTTEConfig, CoNeTTEModel
    config = CoNeTTEConfig.from_pretrained(model_dir)
    return CoNeTTEModel.from_pretrained(model_dir, config=config, precision=request.param, offline=True, audioset_idx_to_name=TAGS,
                                        stopwords=synth.synth_stopwords())


@pytest.fixture(scope="module")
def waves():
    w = torch.from_numpy(synth.synth_waveforms(2, max(LENGTHS), WAVE_SEED, lengths=LENGTHS))
    return [w[i:i + 1, :n].contiguous() for i, n in enumerate(LENGTHS)]


def _strip(rows):
    """token rows without their trailing pad_id"""
    out = []
    for r in rows:
        r = list(r)
        while r and r[-1] == 0:
            r.pop()
        out.append(r)
    return out


def test_keys_and_shapes(model, waves):
    g, w = 3, 2
    out = model.caption_diverse(waves, num_groups=g, group_beam_size=w, diversity_penalty=0.5, sr=32000, task=["clotho", "audiocaps"])
    ref = model(waves, sr=32000, task=["clotho", "audiocaps"], beam_size=2)
    assert set(ref) == set(out)
    b, ps = len(waves), out["mult_preds"].shape[2]
    assert out["mult_preds"].shape == (b, g * w, ps) and out["mult_preds"].dtype == torch.long
    assert out["mult_lprobs"].shape == (b, g * w) and out["lprobs"].shape == (b,)
    assert len(out["mult_cands"]) == b and all(len(c) == g * w and all(isinstance(s, str) for s in c) for c in out["mult_cands"])
    assert out["tasks"] == ["clotho", "audiocaps"] and len(out["tags"]) == b and out["tags_probs"].shape == ref["tags_probs"].shape
    best = out["mult_lprobs"].argmax(dim=1).cpu()            # the first maximum over all G * W slots
    assert torch.equal(out["lprobs"].cpu(), out["mult_lprobs"].cpu()[torch.arange(b), best])
    assert out["cands"] == [out["mult_cands"][i][int(best[i])] for i in range(b)]
    assert _strip(out["preds"].tolist()) == _strip(out["mult_preds"].cpu()[torch.arange(b), best].tolist())
    with pytest.raises(ValueError, match="n_groups"):
        model.caption_diverse(waves, num_groups=5, group_beam_size=4, sr=32000)
    with pytest.raises(ValueError, match="diversity_penalty"):
        model.caption_diverse(waves, diversity_penalty=-1.0, sr=32000)
    with pytest.raises(ValueError, match="is not in"):
        model.caption_diverse(waves, sr=32000, task="nope")


@pytest.mark.parametrize("w", (1, 3))
def test_one_group_is_forward_and_group_zero_is_that_search(model, waves, w):
    ref = model(waves, sr=32000, task="clotho", beam_size=w)
    # certified: a clip its certificate sent through the exact context was searched there, and caption_diverse has no re-run: such
    # clips (at beam 3 on this checkpoint: both) are compared with the base pipeline's own search below
    rec = getattr(model, "last_recomputed", None)
    same = [i for i in range(len(waves)) if rec is None or not bool(rec[i])]
    assert len(same) == len(waves) or model.engine.certified
    one = model.caption_diverse(waves, num_groups=1, group_beam_size=w, diversity_penalty=0.7, sr=32000, task="clotho")
    three = model.caption_diverse(waves, num_groups=3, group_beam_size=w, diversity_penalty=0.7, sr=32000, task="clotho")
    for i in same:
        assert one["cands"][i] == ref["cands"][i] and one["mult_cands"][i] == ref["mult_cands"][i], i
        assert _strip(one["preds"][i:i + 1].tolist()) == _strip(ref["preds"][i:i + 1].tolist()), i
        assert _strip(one["mult_preds"][i].tolist()) == _strip(ref["mult_preds"][i].tolist()), i
        assert torch.equal(one["lprobs"][i].view(torch.int32), ref["lprobs"][i].view(torch.int32)), i
        assert torch.equal(one["mult_lprobs"][i].view(torch.int32), ref["mult_lprobs"][i].view(torch.int32)), i
        assert three["mult_cands"][i][:w] == ref["mult_cands"][i], i
    if len(same) == len(waves):
        for k in ("preds", "mult_preds"):
            assert torch.equal(one[k], ref[k]), k
    # every clip, every precision: the search of the pipeline's decoder context on the preprocessor's embeddings, bit for bit
    batch = model.preprocessor(waves, 32000, None)
    cfg = model.config
    base = model.engine.decode(batch["audio"], batch["audio_shape"][:, 1].to(torch.int32),
                               model.batch_to_task_token_ids(["clotho"] * len(waves), [None] * len(waves)), model.get_forbid_rep_mask(None),
                               w, cfg.min_pred_size, cfg.max_pred_size)
    ps, bl = (int(v) for v in base["sizes"].tolist())
    assert torch.equal(one["mult_preds"], base["mult_preds"][:, :, :ps].long()) and torch.equal(one["preds"], base["best_preds"][:, :bl].long())
    assert torch.equal(one["mult_lprobs"].view(torch.int32), base["mult_lprobs"].view(torch.int32))
    assert torch.equal(one["lprobs"].view(torch.int32), base["best_lprobs"].view(torch.int32))
    assert _strip(three["mult_preds"][:, :w].reshape(-1, three["mult_preds"].shape[2]).tolist()) == \
        _strip(base["mult_preds"].reshape(-1, base["mult_preds"].shape[2]).tolist())


def test_penalty_makes_the_groups_captions_differ(model, waves):
    pen = model.caption_diverse(waves, num_groups=3, group_beam_size=1, diversity_penalty=2.0, sr=32000)
    for i, cands in enumerate(pen["mult_cands"]):
        assert len(set(cands)) > 1, (i, cands)
    if model.engine.precision_name == "fp32":     # the CPU restatement says the same, caption for caption
        from oracle import cpu_ref as O
        torch.set_num_threads(min(16, os.cpu_count() or 1))
        sd, cfg = O.to_torch(synth.synth_state_dict()), synth.synth_config_dict()
        with torch.no_grad():
            batch = O.preprocessor_forward(sd, waves, 32000, None, None)
            mem, mask = O.encode_audio(sd, batch["audio"], batch["audio_shape"])

        def logits_fn(rows, step):
            clips = torch.as_tensor([b for b, _ in rows])
            caps = torch.as_tensor([p for _, p in rows]).t().contiguous()
            with torch.no_grad():
                return O.decoder_forward(sd, mem[clips].permute(2, 0, 1).contiguous(), mask[clips], caps, cfg["nhead"],
                                         cfg["num_decoder_layers"])[-1].double().numpy()
        bos = sd["model.task_id_to_token_id"][torch.zeros(len(waves), dtype=torch.long)].tolist()
        res = GS.group_search(logits_fn, bos, 3, 1, 2.0, cfg["min_pred_size"], cfg["max_pred_size"],
                              sd["model.decoder.classifier.weight"].shape[0], 2, 0, sd["model.forbid_rep_mask"].numpy())
        assert min(c["margin"] for c in res["calls"]) > 0.04
        for b in range(len(waves)):
            assert len({tuple(r) for r in res["mult_preds"][b].tolist()}) == 3, b
        ps = pen["mult_preds"].shape[2]
        assert pen["mult_preds"].cpu().tolist() == res["mult_preds"][:, :, :ps].tolist()
        np.testing.assert_allclose(pen["mult_lprobs"].cpu().numpy(), res["mult_lprobs"], rtol=0, atol=2e-4)
    none = model.caption_diverse(waves, num_groups=3, group_beam_size=1, diversity_penalty=0.0, sr=32000)
    for cands in none["mult_cands"]:
        assert len(set(cands)) == 1, cands


def test_predict_cli(model_dir, tmp_path):
    import csv
    from conette_amd.predict import get_predict_args, main_predict
    paths = []
    for i in range(2):
        wav = synth.synth_waveforms(1, 40000 + 8000 * i, 77 + i)[0]
        pcm = np.clip(np.round(wav * 32768.0), -32768, 32767).astype("<i2")
        p = str(tmp_path / f"clip{i}.wav")
        with wave.open(p, "wb") as w:
            w.setnchannels(1), w.setsampwidth(2), w.setframerate(32000)
            w.writeframes(pcm.tobytes())
        paths.append(p)
    a = get_predict_args(["--audio", *paths, "--beam_groups", "2", "--group_beam", "2", "--diversity_penalty", "1.0"])
    assert (a.beam_groups, a.group_beam, a.diversity_penalty) == (2, 2, 1.0)
    with pytest.raises(ValueError, match="does not go with --sample"):
        main_predict(["--audio", *paths, "--model_name", model_dir, "--beam_groups", "2", "--sample", "3"])
    with pytest.raises(ValueError, match="does not go with --beam_groups"):
        main_predict(["--audio", *paths, "--model_name", model_dir, "--beam_groups", "2", "--align"])
    cache = tmp_path / "audioset_mapping"
    cache.mkdir()
    with open(cache / "class_labels_indices.csv", "w") as f:
        f.write("index,mid,display_name\n" + "".join(f"{i},/m/{i},tag{i}\n" for i in range(527)))
    os.environ["CONETTE_AUDIOSET_CACHE"] = str(cache)
    try:
        out_csv = str(tmp_path / "out.csv")
        res = main_predict(["--audio", *paths, "--task", "audiocaps", "--model_name", model_dir, "--precision", "bf16", "--csv_export", out_csv,
                            "--verbose", "0", "--beam_groups", "2", "--group_beam", "2", "--diversity_penalty", "1.0"])
    finally:
        os.environ.pop("CONETTE_AUDIOSET_CACHE", None)
    assert [r["audio"] for r in res] == ["clip0.wav"] * 4 + ["clip1.wav"] * 4 and all(r["task"] == "audiocaps" for r in res)
    rows = list(csv.DictReader(open(out_csv)))
    assert len(rows) == 8 and [r["candidate"] for r in rows] == [r["candidate"] for r in res]
