"""GPU: the Python surface of the keyword-guided beam search -- CoNeTTEModel.caption_constrained(required=... /
required_per_clip=...) and ``conette-predict --require_words`` -- on the default synthetic checkpoint with waveforms in: two clips
of 1 s and 2.5 s, precision fp32, bf16 and certified (which runs this search on its base pipeline's decoder context)."""
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
KW = dict(sr=32000, task=["clotho", "audiocaps"], beam_size=3)


@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    return synth.write_pretrained_dir(str(tmp_path_factory.mktemp("conette_synth_required")))


@pytest.fixture(scope="module", params=PRECS)
def model(request, model_dir):
    from conette_amd import CoNeTTEConfig, CoNeTTEModel
    config = CoNeTTEConfig.from_pretrained(model_dir)
    return CoNeTTEModel.from_pretrained(model_dir, config=config, precision=request.param, offline=True, audioset_idx_to_name=TAGS,
                                        stopwords=synth.synth_stopwords())


@pytest.fixture(scope="module")
def waves():
    w = torch.from_numpy(synth.synth_waveforms(2, max(LENGTHS), 0, lengths=LENGTHS))
    return [w[i:i + 1, :n].contiguous() for i, n in enumerate(LENGTHS)]


def _absent_words(model, ref, n):
    """n vocabulary words (ids from 40 up) that no hypothesis of ``ref`` holds"""
    used = set(ref["mult_preds"].reshape(-1).tolist())
    ids = [i for i in range(40, 200) if i not in used][:n]
    assert len(ids) == n
    return ids, [model.tokenizer.id_to_token(i) for i in ids]


def _holds(cands, groups):
    return all(any(w in c.split() for w in g) for c in cands if c for g in groups)


def test_required_words_are_in_every_caption(model, waves):
    ref = model.caption_constrained(waves, **KW)
    again = model.caption_constrained(waves, required=None, required_per_clip=None, **KW)      # None: what the call was
    assert set(again) == set(ref) and again["mult_cands"] == ref["mult_cands"] and torch.equal(again["mult_preds"], ref["mult_preds"])
    assert torch.equal(again["mult_lprobs"].view(torch.int32), ref["mult_lprobs"].view(torch.int32))
    assert torch.equal(again["lprobs"].view(torch.int32), ref["lprobs"].view(torch.int32))
    ids, words = _absent_words(model, ref, 4)
    out = model.caption_constrained(waves, required=f"{words[0]}  {words[1]}", **KW)
    assert set(out) == set(ref) and out["mult_preds"].shape[:2] == (2, 3) and out["tasks"] == ["clotho", "audiocaps"]
    flat = [c for cands in out["mult_cands"] for c in cands]
    assert sum(1 for c in flat if c) > 0 and _holds(flat, [[words[0]], [words[1]]]) and _holds(out["cands"], [[words[0]], [words[1]]])
    assert all(c for c in out["cands"])
    for r, lp in zip(out["mult_preds"].reshape(-1, out["mult_preds"].shape[2]).tolist(), out["mult_lprobs"].reshape(-1).tolist()):
        if np.isfinite(lp):
            assert ids[0] in r and ids[1] in r, r
    # a list spec: a word, an id, alternatives of which one is unknown; equal to the string spec where they say the same
    same = model.caption_constrained(waves, required=[words[0], ids[1]], **KW)
    assert torch.equal(same["mult_preds"], out["mult_preds"]) and same["mult_cands"] == out["mult_cands"]
    alt = model.caption_constrained(waves, required=[[words[2], "no-such-word", words[3]]], **KW)
    assert _holds([c for cands in alt["mult_cands"] for c in cands], [[words[2], words[3]]]) and all(c for c in alt["cands"])
    # with a prefix, a ban and the n-gram rule
    both = model.caption_constrained(waves, prefix=words[2], banned=[words[3]], no_repeat_ngram_size=2, required=[words[0]], **KW)
    assert all(c.startswith(words[2]) and words[0] in c.split() and words[3] not in c.split() for c in both["cands"])


def test_required_per_clip(model, waves):
    ref = model.caption_constrained(waves, **KW)
    ids, words = _absent_words(model, ref, 2)
    out = model.caption_constrained(waves, required_per_clip=[words[0], None], **KW)
    assert _holds(out["mult_cands"][0], [[words[0]]]) and all(c for c in out["cands"])
    # the clip without a requirement is searched as before
    assert torch.equal(out["mult_lprobs"][1].view(torch.int32), ref["mult_lprobs"][1].view(torch.int32))
    n = min(out["mult_preds"].shape[2], ref["mult_preds"].shape[2])
    assert torch.equal(out["mult_preds"][1, :, :n], ref["mult_preds"][1, :, :n]) and out["mult_cands"][1] == ref["mult_cands"][1]
    two = model.caption_constrained(waves, required_per_clip=[[words[0]], [[words[1], words[0]]]], **KW)
    assert _holds(two["mult_cands"][0], [[words[0]]]) and _holds(two["mult_cands"][1], [[words[0], words[1]]])


def test_value_errors(model, waves):
    tok = model.tokenizer
    kw = dict(sr=32000, task="clotho")
    w = lambda i: tok.id_to_token(i)
    with pytest.raises(ValueError, match="no-such-word"):
        model.caption_constrained(waves, required="no-such-word", **kw)
    with pytest.raises(ValueError, match="exclude"):
        model.caption_constrained(waves, required=w(40), required_per_clip=[w(40), w(41)], **kw)
    with pytest.raises(ValueError, match="one per clip"):
        model.caption_constrained(waves, required_per_clip=[w(40)], **kw)
    with pytest.raises(ValueError, match=tok.eos_token):
        model.caption_constrained(waves, required=[tok.eos_token_id], **kw)
    with pytest.raises(ValueError, match=f"{w(41)}.*banned"):
        model.caption_constrained(waves, required=w(41), banned=[w(41)], **kw)
    with pytest.raises(ValueError, match=f"{w(41)}.*groups 0 and 1"):
        model.caption_constrained(waves, required=[[w(40), w(41)], w(41)], **kw)
    with pytest.raises(ValueError, match="9 requirement groups"):
        model.caption_constrained(waves, required=" ".join(w(40 + i) for i in range(9)), **kw)
    with pytest.raises(ValueError, match="do not fit"):
        model.caption_constrained(waves, required=" ".join(w(40 + i) for i in range(4)), max_pred_size=3, **kw)
    with pytest.raises(ValueError, match="do not fit"):
        model.caption_constrained(waves, prefix=w(50) + " " + w(51), required=" ".join(w(40 + i) for i in range(3)), max_pred_size=4, **kw)
    with pytest.raises(ValueError, match="task token"):
        model.caption_constrained(waves, required=[int(model.batch_to_task_token_ids(["clotho"], [None])[0])], **kw)


def test_predict_cli(model_dir, tmp_path):
    import csv
    from conette_amd import CoNeTTEConfig, CoNeTTEModel
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
    with pytest.raises(ValueError, match="do not go with --sample"):
        main_predict(["--audio", *paths, "--model_name", model_dir, "--require_words", "w40", "--sample", "3"])
    cache = tmp_path / "audioset_mapping"
    cache.mkdir()
    with open(cache / "class_labels_indices.csv", "w") as f:
        f.write("index,mid,display_name\n" + "".join(f"{i},/m/{i},tag{i}\n" for i in range(527)))
    os.environ["CONETTE_AUDIOSET_CACHE"] = str(cache)
    try:
        config = CoNeTTEConfig.from_pretrained(model_dir)
        tok = CoNeTTEModel.from_pretrained(model_dir, config=config, precision="bf16", offline=True, audioset_idx_to_name=TAGS,
                                           stopwords=synth.synth_stopwords()).tokenizer
        words = [tok.id_to_token(i) for i in (140, 141, 142)]
        out_csv = str(tmp_path / "out.csv")
        res = main_predict(["--audio", *paths, "--task", "audiocaps", "--model_name", model_dir, "--precision", "bf16", "--csv_export", out_csv,
                            "--verbose", "0", "--require_words", words[0], f"{words[1]}|nope|{words[2]}"])
    finally:
        os.environ.pop("CONETTE_AUDIOSET_CACHE", None)
    assert [r["audio"] for r in res] == ["clip0.wav", "clip1.wav"] and all(r["task"] == "audiocaps" for r in res)
    for r in res:
        got = r["candidate"].split()
        assert words[0] in got and (words[1] in got or words[2] in got), r
    rows = list(csv.DictReader(open(out_csv)))
    assert len(rows) == 2 and [r["candidate"] for r in rows] == [r["candidate"] for r in res]
