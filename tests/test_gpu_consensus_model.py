"""GPU: the Python surface of the consensus choice -- CoNeTTEModel.select_consensus / caption_consensus and ``conette-predict --sample N
--consensus`` -- on the default synthetic checkpoint with waveforms in (precision bf16); the host rule is consensus.select_fp32."""
import os
import wave

import numpy as np
import pytest
import torch

from conette_amd import consensus as R
from conette_amd import synth

pytestmark = pytest.mark.gpu
TAGS = {i: f"tag{i}" for i in range(527)}
SAMPLING = dict(temperature=2.0, top_k=50, sr=32000)


@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    return synth.write_pretrained_dir(str(tmp_path_factory.mktemp("conette_synth_consensus")))


@pytest.fixture(scope="module")
def model(model_dir):
    from conette_amd import CoNeTTEConfig, CoNeTTEModel
    config = CoNeTTEConfig.from_pretrained(model_dir)
    return CoNeTTEModel.from_pretrained(model_dir, config=config, precision="bf16", offline=True, audioset_idx_to_name=TAGS,
                                        stopwords=synth.synth_stopwords())


@pytest.fixture(scope="module")
def waves():
    lengths = [64000, 40000, 9000]
    w = torch.from_numpy(synth.synth_waveforms(3, 64000, 21, lengths=lengths))
    return [w[i:i + 1, :n].contiguous() for i, n in enumerate(lengths)]


def host_rule(out, weights=None, **kw):
    """select_fp32 on a returned table (its lens where it has them); ``weights``: the fp32 values the device read"""
    preds = out["mult_preds"].cpu().numpy().astype(np.int32)
    lens = out["lens"].cpu().numpy() if "lens" in out else None
    return R.select_batch(preds, lens, weights, fp32=True, as_given=weights is not None, **kw)


def same_tensors(a, b):
    if isinstance(a, torch.Tensor):
        return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                                        b.view(torch.int32) if b.dtype == torch.float32 else b)
    return a == b


def check_pick(out, base, want):
    b = out["mult_preds"].shape[0]
    index = out["consensus_index"].cpu()
    assert index.dtype == torch.long and index.tolist() == want["best"].tolist()
    assert np.array_equal(out["consensus"].cpu().numpy().view(np.int32), want["expected"].view(np.int32))
    assert np.array_equal(out["consensus_margin"].cpu().numpy().view(np.int32), want["margin"].view(np.int32))
    assert out["cands"] == [out["mult_cands"][i][int(index[i])] for i in range(b)]
    rows = torch.arange(b)
    chosen = out["mult_preds"].cpu()[rows, index]
    assert torch.equal(out["preds"].cpu(), chosen[:, :out["preds"].shape[1]]) and out["preds"].dtype == torch.long
    assert not bool(((chosen[:, out["preds"].shape[1]:] != 0) & (chosen[:, out["preds"].shape[1]:] != 2)).any())
    assert torch.equal(out["lprobs"].cpu(), out["mult_lprobs"].cpu()[rows, index])
    for k in base:      # everything else is the call's own
        if k not in ("cands", "preds", "lprobs"):
            assert same_tensors(out[k], base[k]), k


@pytest.mark.parametrize("utility,order", [("ngram", 4), ("ngram", 1), ("edit", 4)])
def test_caption_consensus_is_sample_then_select(model, waves, utility, order):
    n = 12
    kw = dict(utility=utility, max_order=order)
    out = model.caption_consensus(waves, num_samples=n, seed=5, task=["clotho", "audiocaps", "clotho"], **SAMPLING, **kw)
    base = model.sample(waves, num_samples=n, seed=5, task=["clotho", "audiocaps", "clotho"], **SAMPLING)
    two = model.select_consensus(base, **kw)
    assert set(out) == set(two) == set(base) | {"consensus", "consensus_index", "consensus_margin"}
    for k in out:
        assert same_tensors(out[k], two[k]), k
    assert out["consensus"].shape == (3, n) and out["mult_preds"].shape[:2] == (3, n)
    check_pick(out, base, host_rule(out, utility=utility, max_order=order))


def test_one_sample_is_the_sample(model, waves):
    out = model.caption_consensus(waves, num_samples=1, seed=9, **SAMPLING)
    base = model.sample(waves, num_samples=1, seed=9, **SAMPLING)
    assert out["cands"] == base["cands"] and torch.equal(out["preds"], base["preds"]) and torch.equal(out["lprobs"], base["lprobs"])
    assert out["consensus_index"].tolist() == [0, 0, 0] and bool(torch.isinf(out["consensus_margin"]).all())
    assert out["consensus"].tolist() == [[1.0]] * 3


def test_select_on_searches_without_lens(model, waves):
    for base in (model(waves, sr=32000, beam_size=3), model.caption_diverse(waves, num_groups=3, group_beam_size=2, sr=32000)):
        assert "lens" not in base and "sum_lprobs" not in base
        for utility, order in (("ngram", 2), ("edit", 4)):
            out = model.select_consensus(base, utility=utility, max_order=order)
            check_pick(out, base, host_rule(base, utility=utility, max_order=order))


@pytest.mark.parametrize("scale", [1.0, 0.25])
def test_model_evidence(model, waves, scale):
    base = model.sample(waves, num_samples=16, seed=2, **SAMPLING)
    out = model.select_consensus(base, evidence="model", evidence_scale=scale)
    w = out["consensus_weights"].cpu().numpy()
    z = scale * base["sum_lprobs"].cpu().numpy().astype(np.float64)
    want = np.exp(z - z.max(axis=1, keepdims=True))
    want /= want.sum(axis=1, keepdims=True)
    # fp32 rounding of the normalised weights (half an ulp, 2**-24 relative) over the device's float64 exp / sum (<= 1e-14)
    assert w.dtype == np.float32 and np.all(np.abs(w - want) <= 2.0 ** -24 * want + 1e-14)
    check_pick(out, {k: v for k, v in base.items()}, host_rule(base, weights=w))
    # a search reports sum / length: the evidence is mult_lprobs * (tokens up to and including <eos>)
    beam = model(waves, sr=32000, beam_size=3)
    got = model.select_consensus(beam, evidence="model", evidence_scale=scale)
    ids = beam["mult_preds"].cpu().numpy()
    length = np.array([[(list(r).index(2) + 1) if 2 in r else len(r) for r in clip] for clip in ids], dtype=np.float64)
    z = scale * beam["mult_lprobs"].cpu().numpy().astype(np.float64) * length
    want = np.exp(z - z.max(axis=1, keepdims=True))
    want /= want.sum(axis=1, keepdims=True)
    w = got["consensus_weights"].cpu().numpy()
    assert np.all(np.abs(w - want) <= 2.0 ** -24 * want + 1e-14)
    check_pick(got, beam, host_rule(beam, weights=w))


def test_arguments(model, waves):
    base = model.sample(waves, num_samples=2, seed=1, **SAMPLING)
    for kw, word in ((dict(utility="bleu"), "utility"), (dict(max_order=0), "max_order"), (dict(evidence="votes"), "evidence"),
                     (dict(evidence="model", evidence_scale=float("nan")), "evidence_scale")):
        with pytest.raises(ValueError, match=word):
            model.select_consensus(base, **kw)
    with pytest.raises(ValueError, match="mult_preds"):
        model.select_consensus({"cands": ["a"]})
    with pytest.raises(ValueError, match="n_cands"):
        model.caption_consensus(waves, num_samples=65, seed=1, **SAMPLING)


def test_predict_cli_writes_the_consensus_caption(model_dir, tmp_path):
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
        common = ["--audio", *paths, "--task", "audiocaps", "--model_name", model_dir, "--precision", "bf16", "--verbose", "0",
                  "--sample", "6", "--seed", "1", "--temperature", "2.0"]
        draws = main_predict(common)
        res = main_predict(common + ["--consensus", "ngram", "--consensus_order", "2", "--csv_export", out_csv])
    finally:
        os.environ.pop("CONETTE_AUDIOSET_CACHE", None)
    assert [r["audio"] for r in res] == ["clip0.wav", "clip1.wav"] and all(r["task"] == "audiocaps" for r in res)
    for i, r in enumerate(res):     # one of the file's six draws
        assert r["candidate"] in [d["candidate"] for d in draws[6 * i:6 * i + 6]]
    rows = list(csv.DictReader(open(out_csv)))
    assert len(rows) == 2 and [r["candidate"] for r in rows] == [r["candidate"] for r in res]
