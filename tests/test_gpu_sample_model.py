"""GPU: the Python surface of sampling -- CoNeTTEModel.sample, decode_audio(..., "sample") and ``conette-predict --sample`` -- on
the default synthetic checkpoint with waveforms in, precision bf16 and certified (which samples through its 16-bit base context)."""
import os
import wave

import numpy as np
import pytest
import torch

from conette_amd import sampling, synth

pytestmark = pytest.mark.gpu
TAGS = {i: f"tag{i}" for i in range(527)}
PRECS = ("bf16", "certified")


@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    return synth.write_pretrained_dir(str(tmp_path_factory.mktemp("conette_synth_sample")))


@pytest.fixture(scope="module", params=PRECS)
def model(request, model_dir):
    from conette_amd import CoNeTTEConfig, CoNeTTEModel
    config = CoNeTTEConfig.from_pretrained(model_dir)
    return CoNeTTEModel.from_pretrained(model_dir, config=config, precision=request.param, offline=True, audioset_idx_to_name=TAGS,
                                        stopwords=synth.synth_stopwords())


@pytest.fixture(scope="module")
def waves():
    lengths = [64000, 40000, 9000]      # a list of mono clips of different lengths: a batch of 3
    w = torch.from_numpy(synth.synth_waveforms(3, 64000, 21, lengths=lengths))
    return [w[i:i + 1, :n].contiguous() for i, n in enumerate(lengths)]     # (channels, time) each


def test_keys_shapes_best_sample_and_tasks(model, waves):
    n = 4
    out = model.sample(waves, num_samples=n, temperature=2.0, top_k=50, top_p=0.95, seed=3, sr=32000, task=["clotho", "audiocaps", "clotho"])
    ref = model(waves, sr=32000, task=["clotho", "audiocaps", "clotho"], beam_size=2)
    assert set(ref) <= set(out) and {"sum_lprobs", "lens", "tasks"} <= set(out)
    b = len(waves)
    ps = out["mult_preds"].shape[2]
    lens = out["lens"].cpu()
    assert out["mult_preds"].shape == (b, n, ps) and out["mult_preds"].dtype == torch.long and ps == int(lens.max())
    assert out["mult_lprobs"].shape == (b, n) and out["sum_lprobs"].shape == (b, n) and lens.shape == (b, n)
    assert len(out["mult_cands"]) == b and all(len(c) == n and all(isinstance(s, str) for s in c) for c in out["mult_cands"])
    assert out["tasks"] == ["clotho", "audiocaps", "clotho"] and len(out["tags"]) == b
    mean = out["sum_lprobs"].cpu() / lens.float()
    assert torch.equal(out["mult_lprobs"].cpu(), mean)
    best = mean.argmax(dim=1)
    rows = torch.arange(b)
    assert torch.equal(out["lprobs"].cpu(), mean[rows, best])
    bm = int(lens[rows, best].max())
    assert torch.equal(out["preds"].cpu(), out["mult_preds"].cpu()[rows, best][:, :bm])
    assert out["cands"] == [out["mult_cands"][i][int(best[i])] for i in range(b)]
    assert int(lens.min()) > model.config.min_pred_size or int(lens.min()) == model.config.max_pred_size
    with pytest.raises(ValueError, match="Invalid number of tasks"):
        model.sample(waves, sr=32000, task=["clotho"])
    with pytest.raises(ValueError, match="is not in"):
        model.sample(waves, sr=32000, task="nope")
    with pytest.raises(ValueError, match="num_samples"):
        model.sample(waves, num_samples=0, sr=32000)


def test_seed_reproduces_and_seeds_differ(model, waves):
    a = model.sample(waves, num_samples=5, temperature=4.0, seed=11, sr=32000)
    b = model.sample(waves, num_samples=5, temperature=4.0, seed=11, sr=32000)
    c = model.sample(waves, num_samples=5, temperature=4.0, seed=12, sr=32000)
    assert torch.equal(a["mult_preds"], b["mult_preds"]) and a["mult_cands"] == b["mult_cands"]
    assert torch.equal(a["sum_lprobs"].view(torch.int32), b["sum_lprobs"].view(torch.int32))
    assert a["mult_preds"].shape != c["mult_preds"].shape or not torch.equal(a["mult_preds"], c["mult_preds"])


def test_twenty_samples_are_the_planned_chunks(model, waves):
    """num_samples = 20 = one call of 16 + one of 4 on the column blocks of the same uniforms."""
    eng = model.engine
    cfg = model.config
    batch = model.preprocessor(waves, 32000, None)
    audio, lens = batch["audio"], batch["audio_shape"][:, 1].to(torch.int32)
    bos = model.batch_to_task_token_ids([model.default_task] * 3, [None] * 3)
    fb = model.get_forbid_rep_mask(None)
    n = 20
    u = torch.rand((cfg.max_pred_size, 3, n), device=model.device, generator=torch.Generator(device=model.device).manual_seed(5))
    args = (cfg.min_pred_size, cfg.max_pred_size)
    whole = eng.sample(audio, lens, bos, fb, n, *args, temperature=2.0, top_k=100, uniforms=u, want_tokens=True)
    plan = sampling.plan_sample_chunks(n)
    assert plan == [(0, 16), (16, 4)]
    parts = [eng.sample(audio, lens, bos, fb, cnt, *args, temperature=2.0, top_k=100, uniforms=u[:, :, first:first + cnt].contiguous(),
                        want_tokens=True) for first, cnt in plan]
    for k in ("preds", "sum_lprobs", "lens", "tok_lprobs"):
        cat = torch.cat([p[k] for p in parts], dim=1)
        assert torch.equal(whole[k].view(torch.int32) if whole[k].dtype == torch.float32 else whole[k],
                           cat.view(torch.int32) if cat.dtype == torch.float32 else cat), k
    assert whole["preds"].shape == (3, n, cfg.max_pred_size)
    assert int(whole["sizes"][0]) == int(whole["lens"].max())
    # the model-level call with the same generator state draws the same uniforms
    out = model.sample(waves, num_samples=n, temperature=2.0, top_k=100, sr=32000,
                       generator=torch.Generator(device=model.device).manual_seed(5))
    ps = out["mult_preds"].shape[2]
    assert torch.equal(out["mult_preds"], whole["preds"][:, :, :ps].long())


def test_top1_sample_is_the_greedy_caption(model, waves):
    out = model.sample(waves, num_samples=2, top_k=1, seed=1, sr=32000, task="clotho")
    ref = model(waves, sr=32000, task="clotho", beam_size=1)
    # certified: a clip its certificate sent through the exact context was searched at another precision than the 16-bit base
    # context that samples; the others took the base context's own arg-max chain
    rec = getattr(model, "last_recomputed", None)
    same = [i for i in range(3) if rec is None or not bool(rec[i])]
    assert same, "every clip was re-run exactly"
    for i in same:
        assert out["mult_cands"][i][0] == ref["cands"][i] and out["mult_cands"][i][1] == ref["cands"][i], i
        assert out["cands"][i] == ref["cands"][i]
    via = model.decode_audio({"audio": model.preprocessor(waves, 32000, None)["audio"],
                              "audio_shape": model.preprocessor(waves, 32000, None)["audio_shape"]}, "sample", num_samples=2, top_k=1,
                             task="clotho")
    assert via["mult_cands"] == out["mult_cands"]


def test_predict_cli_writes_n_candidates_per_file(model_dir, tmp_path):
    import csv
    from conette_amd.predict import main_predict
    paths = []
    for i in range(2):
        wav = synth.synth_waveforms(1, 40000 + 8000 * i, 77 + i)[0]
        pcm = np.clip(np.round(wav * 32768.0), -32768, 32767).astype("<i2")
        p = str(tmp_path / f"clip{i}.wav")
        with wave.open(p, "wb") as w:
            w.setnchannels(1), w.setsampwidth(2), w.setframerate(32000)
            w.writeframes(pcm.tobytes())
        paths.append(p)
    cache = tmp_path / "audioset_mapping"
    cache.mkdir()
    with open(cache / "class_labels_indices.csv", "w") as f:
        f.write("index,mid,display_name\n" + "".join(f"{i},/m/{i},tag{i}\n" for i in range(527)))
    os.environ["CONETTE_AUDIOSET_CACHE"] = str(cache)
    try:
        out_csv = str(tmp_path / "out.csv")
        argv = ["--audio", *paths, "--task", "audiocaps", "--model_name", model_dir, "--precision", "bf16", "--csv_export", out_csv,
                "--verbose", "0", "--sample", "3", "--seed", "1", "--temperature", "2.0"]
        res = main_predict(argv)
        again = main_predict(argv)
    finally:
        os.environ.pop("CONETTE_AUDIOSET_CACHE", None)
    assert [r["audio"] for r in res] == ["clip0.wav"] * 3 + ["clip1.wav"] * 3 and all(r["task"] == "audiocaps" for r in res)
    assert res == again, "--seed reproduces"
    rows = list(csv.DictReader(open(out_csv)))
    assert len(rows) == 6 and [r["candidate"] for r in rows] == [r["candidate"] for r in res]
