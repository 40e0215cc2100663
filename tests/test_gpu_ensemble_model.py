"""GPU: the Python surface of the ensemble beam search -- CoNeTTEModel.caption_ensemble, conette_amd.CoNeTTEEnsemble and
``conette-predict --ensemble_models / --ensemble_tasks`` -- on synthetic pretrained directories (the default checkpoint at synth
seeds 0 and 1, one vocabulary) with waveforms in: two clips of 1 s and 2.5 s, precision fp32, bf16 and certified (which runs this
search on its base pipeline's decoder context, with no exact re-run).

What the search computes is held to its rule by tests/test_gpu_ensemble_search.py; here the model level is held to
Engine.decode_ensemble on the same embeddings, bit for bit, and to ``forward``'s keys and shapes."""
import os
import wave

import numpy as np
import pytest
import torch

from conette_amd import synth

pytestmark = pytest.mark.gpu
TAGS = {i: f"tag{i}" for i in range(527)}
PRECS = ("fp32", "bf16", "certified")
LENGTHS = [32000, 80000]


@pytest.fixture(scope="module")
def model_dirs(tmp_path_factory):
    return [synth.write_pretrained_dir(str(tmp_path_factory.mktemp(f"conette_synth_ens{s}")), seed=s) for s in (0, 1)]


@pytest.fixture(scope="module", params=PRECS)
def models(request, model_dirs):
    from conette_amd import CoNeTTEConfig, CoNeTTEModel
    return [CoNeTTEModel.from_pretrained(d, config=CoNeTTEConfig.from_pretrained(d), precision=request.param, offline=True,
                                         audioset_idx_to_name=TAGS, stopwords=synth.synth_stopwords()) for d in model_dirs]


@pytest.fixture(scope="module")
def waves():
    w = torch.from_numpy(synth.synth_waveforms(2, max(LENGTHS), 0, lengths=LENGTHS))
    return [w[i:i + 1, :n].contiguous() for i, n in enumerate(LENGTHS)]


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _engine_run(members_of, models, waves, tasks, weights, combine, beam):
    """Engine.decode_ensemble on the preprocessors' embeddings; ``members_of``: the index into ``models`` of every member"""
    first = models[0]
    batches = {i: models[i].preprocessor(waves, 32000, None) for i in set(members_of)}
    b = len(waves)
    members = []
    for i, t, w in zip(members_of, tasks, weights):
        m = models[i]
        members.append((m.engine, batches[i]["audio"], m.batch_to_task_token_ids([t] * b, [None] * b), w))
    cfg = first.config
    return first.engine.decode_ensemble(members, batches[members_of[0]]["audio_shape"][:, 1].to(torch.int32), first.get_forbid_rep_mask(None),
                                        beam, cfg.min_pred_size, cfg.max_pred_size, combine=combine)


def _assert_is(out, base):
    ps, bl = (int(v) for v in base["sizes"].tolist())
    assert torch.equal(out["mult_preds"], base["mult_preds"][:, :, :ps].long()) and torch.equal(out["preds"], base["best_preds"][:, :bl].long())
    assert torch.equal(_bits(out["mult_lprobs"]), _bits(base["mult_lprobs"])) and torch.equal(_bits(out["lprobs"]), _bits(base["best_lprobs"]))


def test_caption_ensemble_keys_shapes_and_the_engines_search(models, waves):
    model = models[0]
    beam = 3
    out = model.caption_ensemble(waves, tasks=["clotho", "audiocaps", "macs"], weights=(2, 5, 3), combine="prob", beam_size=beam, sr=32000)
    ref = model(waves, sr=32000, task="clotho", beam_size=beam)
    assert set(ref) == set(out)
    b, ps = len(waves), out["mult_preds"].shape[2]
    assert out["mult_preds"].shape == (b, beam, ps) and out["mult_preds"].dtype == torch.long and out["preds"].dtype == torch.long
    assert out["mult_lprobs"].shape == (b, beam) and out["lprobs"].shape == (b,)
    assert len(out["mult_cands"]) == b and all(len(c) == beam and all(isinstance(s, str) for s in c) for c in out["mult_cands"])
    assert out["tasks"] == ["clotho+audiocaps+macs"] * b and len(out["tags"]) == b and out["tags_probs"].shape == ref["tags_probs"].shape
    best = out["mult_lprobs"].argmax(dim=1).cpu()
    assert torch.equal(out["lprobs"].cpu(), out["mult_lprobs"].cpu()[torch.arange(b), best])
    assert out["cands"] == [out["mult_cands"][i][int(best[i])] for i in range(b)]
    _assert_is(out, _engine_run([0, 0, 0], models, waves, ["clotho", "audiocaps", "macs"], (0.2, 0.5, 0.3), "prob", beam))
    # one task: the plain search of the pipeline's decoder context under that task, bit for bit
    one = model.caption_ensemble(waves, tasks="audiocaps", beam_size=beam, sr=32000)
    batch = model.preprocessor(waves, 32000, None)
    cfg = model.config
    base = model.engine.decode(batch["audio"], batch["audio_shape"][:, 1].to(torch.int32), model.batch_to_task_token_ids(["audiocaps"] * b, [None] * b),
                               model.get_forbid_rep_mask(None), beam, cfg.min_pred_size, cfg.max_pred_size)
    _assert_is(one, base)
    assert one["tasks"] == ["audiocaps"] * b
    with pytest.raises(ValueError, match="n_members"):
        model.caption_ensemble(waves, tasks=["clotho"] * 5, sr=32000)
    with pytest.raises(ValueError, match="weights"):
        model.caption_ensemble(waves, tasks=["clotho", "audiocaps"], weights=(1.0, -1.0), sr=32000)
    with pytest.raises(ValueError, match="combine"):
        model.caption_ensemble(waves, tasks=["clotho", "audiocaps"], combine="mean", sr=32000)
    with pytest.raises(ValueError, match="is not in"):
        model.caption_ensemble(waves, tasks=["clotho", "nope"], sr=32000)


def test_ensemble_of_models_is_the_engines_search(models, waves):
    from conette_amd import CoNeTTEEnsemble
    beam = 2
    ens = CoNeTTEEnsemble(models, weights=(1.0, 3.0), combine="logprob")
    out = ens(waves, sr=32000, task="clotho", beam_size=beam)
    ref = models[0](waves, sr=32000, task="clotho", beam_size=beam)
    assert set(ref) == set(out) and out["tasks"] == ["clotho+clotho"] * len(waves)
    assert out["mult_preds"].shape[:2] == (len(waves), beam) and out["tags_probs"].shape == ref["tags_probs"].shape
    _assert_is(out, _engine_run([0, 1], models, waves, ["clotho", "clotho"], (0.25, 0.75), "logprob", beam))
    per_member = ens(waves, sr=32000, task=["audiocaps", "clotho"], beam_size=beam)
    assert per_member["tasks"] == ["audiocaps+clotho"] * len(waves)
    _assert_is(per_member, _engine_run([0, 1], models, waves, ["audiocaps", "clotho"], (0.25, 0.75), "logprob", beam))
    # the same model twice, a task per member: caption_ensemble's search
    twice = CoNeTTEEnsemble([models[1], models[1]], combine="prob")(waves, sr=32000, task=["clotho", "audiocaps"], beam_size=beam)
    same = models[1].caption_ensemble(waves, tasks=["clotho", "audiocaps"], combine="prob", beam_size=beam, sr=32000)
    for k in ("preds", "mult_preds", "lprobs", "mult_lprobs"):
        assert torch.equal(_bits(twice[k]), _bits(same[k])), k
    assert twice["cands"] == same["cands"]
    with pytest.raises(ValueError, match="tasks"):
        ens(waves, sr=32000, task=["clotho", "audiocaps", "clotho"])
    with pytest.raises(ValueError, match="n_members"):
        CoNeTTEEnsemble([])
    with pytest.raises(ValueError, match="weights"):
        CoNeTTEEnsemble(models, weights=(1.0,))


def test_tokenizer_mismatch_is_refused(models, tmp_path_factory):
    from conette_amd import CoNeTTEConfig, CoNeTTEEnsemble, CoNeTTEModel
    d = synth.write_pretrained_dir(str(tmp_path_factory.mktemp("conette_synth_ens_small")), n_words=50)
    other = CoNeTTEModel.from_pretrained(d, config=CoNeTTEConfig.from_pretrained(d), precision="fp32", offline=True, audioset_idx_to_name=TAGS,
                                         stopwords=synth.synth_stopwords())
    with pytest.raises(ValueError, match="vocabulary"):
        CoNeTTEEnsemble([models[0], other])


def test_predict_cli(model_dirs, tmp_path):
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
    a = get_predict_args(["--audio", *paths, "--ensemble_models", *model_dirs, "--ensemble_weights", "1", "3", "--ensemble_combine", "prob"])
    assert (a.ensemble_models, a.ensemble_weights, a.ensemble_combine, a.ensemble_tasks) == (model_dirs, [1.0, 3.0], "prob", None)
    a = get_predict_args(["--audio", *paths])
    assert (a.ensemble_models, a.ensemble_tasks, a.ensemble_weights, a.ensemble_combine) == (None, None, None, "logprob")
    for extra, word in ((["--ensemble_tasks", "clotho", "audiocaps", "--sample", "2"], "--sample"),
                        (["--ensemble_tasks", "clotho", "audiocaps", "--beam_groups", "2"], "--beam_groups"),
                        (["--ensemble_tasks", "clotho", "audiocaps", "--align"], "--align"),
                        (["--ensemble_tasks", "clotho", "audiocaps", "--prefix", "w5"], "--prefix"),
                        (["--ensemble_tasks", "clotho", "audiocaps", "--task", "clotho"], "--task"),
                        (["--ensemble_weights", "1", "2"], "--ensemble_weights"),
                        (["--ensemble_tasks", "clotho", "audiocaps", "--ensemble_weights", "1"], "--ensemble_weights"),
                        (["--ensemble_tasks", "clotho", "audiocaps", "--ensemble_weights", "1", "-1"], "weights"),
                        (["--ensemble_models", *model_dirs, "--ensemble_tasks", "a", "b", "c"], "--ensemble_tasks"),
                        (["--ensemble_tasks", "a", "b", "c", "d", "e"], "n_members"),
                        (["--ensemble_models", *model_dirs, "--model_path", "x"], "--model_name / --model_path"),
                        (["--ensemble_models", *model_dirs, "--model_name", model_dirs[0]], "--model_name / --model_path"),
                        (["--ensemble_models", model_dirs[0]], "expected 2 .. 4")):
        with pytest.raises(ValueError, match=word):
            get_predict_args(["--audio", *paths, *extra])
    cache = tmp_path / "audioset_mapping"
    cache.mkdir()
    with open(cache / "class_labels_indices.csv", "w") as f:
        f.write("index,mid,display_name\n" + "".join(f"{i},/m/{i},tag{i}\n" for i in range(527)))
    os.environ["CONETTE_AUDIOSET_CACHE"] = str(cache)
    try:
        out_csv = str(tmp_path / "out.csv")
        res = main_predict(["--audio", *paths, "--model_name", model_dirs[0], "--precision", "bf16", "--csv_export", out_csv, "--verbose", "0",
                            "--ensemble_tasks", "clotho", "audiocaps", "--ensemble_weights", "1", "3", "--ensemble_combine", "prob"])
        both = main_predict(["--audio", *paths, "--precision", "bf16", "--verbose", "0", "--ensemble_models", *model_dirs,
                             "--ensemble_tasks", "audiocaps"])
    finally:
        os.environ.pop("CONETTE_AUDIOSET_CACHE", None)
    assert [r["audio"] for r in res] == ["clip0.wav", "clip1.wav"] and all(r["task"] == "clotho+audiocaps" for r in res)
    assert all(isinstance(r["candidate"], str) and r["candidate"] for r in res)
    rows = list(csv.DictReader(open(out_csv)))
    assert len(rows) == 2 and [r["candidate"] for r in rows] == [r["candidate"] for r in res]
    assert [r["audio"] for r in both] == ["clip0.wav", "clip1.wav"] and all(r["task"] == "audiocaps+audiocaps" for r in both)
