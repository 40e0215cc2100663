"""GPU: the Python surface of the constrained beam search -- CoNeTTEModel.caption_constrained and ``conette-predict --prefix /
--ban_words / --no_repeat_ngram`` -- on the default synthetic checkpoint with waveforms in: two clips of 1 s and 2.5 s, precision
fp32, bf16 and certified (which runs this search on its base pipeline's decoder context, with no exact re-run)."""
import os
import wave

import numpy as np
import pytest
import torch

from conette_amd import constrained_search as CS
from conette_amd import synth

pytestmark = pytest.mark.gpu
TAGS = {i: f"tag{i}" for i in range(527)}
PRECS = ("fp32", "bf16", "certified")
LENGTHS = [32000, 80000]
PREFIX_IDS = (40, 41)


@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    return synth.write_pretrained_dir(str(tmp_path_factory.mktemp("conette_synth_constrained")))


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


def _rows(mult_preds, mult_lprobs, eos=2):
    """(clip, slot, tokens up to and including <eos>) of every hypothesis that is not void"""
    for b in range(mult_preds.shape[0]):
        for s in range(mult_preds.shape[1]):
            if bool(torch.isfinite(mult_lprobs[b, s])):
                r = mult_preds[b, s].tolist()
                yield b, s, r[: r.index(eos) + 1] if eos in r else r


def test_keys_shapes_and_prefixes(model, waves):
    tok = model.tokenizer
    words = " ".join(tok.id_to_token(i) for i in PREFIX_IDS)
    ref = model(waves, sr=32000, task=["clotho", "audiocaps"], beam_size=3)
    out = model.caption_constrained(waves, prefix=words, sr=32000, task=["clotho", "audiocaps"], beam_size=3)
    assert set(ref) == set(out)
    b, ps = len(waves), out["mult_preds"].shape[2]
    assert out["mult_preds"].shape == (b, 3, ps) and out["mult_preds"].dtype == torch.long and out["preds"].dtype == torch.long
    assert out["mult_lprobs"].shape == (b, 3) and out["lprobs"].shape == (b,) and out["tasks"] == ["clotho", "audiocaps"]
    assert len(out["mult_cands"]) == b and all(len(c) == 3 and all(isinstance(s, str) for s in c) for c in out["mult_cands"])
    assert len(out["tags"]) == b and out["tags_probs"].shape == ref["tags_probs"].shape
    seen = 0
    for _, _, toks in _rows(out["mult_preds"].cpu(), out["mult_lprobs"].cpu()):
        assert tuple(toks[:2]) == PREFIX_IDS, toks
        seen += 1
    assert seen == b * 3 and all(c.startswith(words) for c in out["cands"])
    best = out["mult_lprobs"].argmax(dim=1).cpu()
    assert torch.equal(out["lprobs"].cpu(), out["mult_lprobs"].cpu()[torch.arange(b), best])
    # ids, one string per clip and one string for all clips are one search
    ids = torch.as_tensor([list(PREFIX_IDS) + [tok.pad_token_id]] * b)
    for other in (model.caption_constrained(waves, prefix=ids, sr=32000, task=["clotho", "audiocaps"], beam_size=3),
                  model.caption_constrained(waves, prefix=[words] * b, sr=32000, task=["clotho", "audiocaps"], beam_size=3)):
        assert torch.equal(other["mult_preds"], out["mult_preds"]) and other["mult_cands"] == out["mult_cands"]
        assert torch.equal(other["mult_lprobs"].view(torch.int32), out["mult_lprobs"].view(torch.int32))
    # ragged: the clip without a prefix is searched as the base pipeline's decoder context searches it
    rag = model.caption_constrained(waves, prefix=[words, ""], sr=32000, task="clotho", beam_size=3)
    batch = model.preprocessor(waves, 32000, None)
    cfg = model.config
    base = model.engine.decode(batch["audio"], batch["audio_shape"][:, 1].to(torch.int32),
                               model.batch_to_task_token_ids(["clotho"] * b, [None] * b), model.get_forbid_rep_mask(None), 3,
                               cfg.min_pred_size, cfg.max_pred_size)
    assert torch.equal(rag["mult_lprobs"][1].view(torch.int32), base["mult_lprobs"][1].view(torch.int32))
    n = min(rag["mult_preds"].shape[2], base["mult_preds"].shape[2])
    assert torch.equal(rag["mult_preds"][1, :, :n], base["mult_preds"][1, :, :n].long())


def test_banned_words_are_absent_and_no_ngram_repeats(model, waves):
    tok = model.tokenizer
    ref = model.caption_constrained(waves, sr=32000, task="clotho", beam_size=3)
    first = sorted({c.split()[0] for c in ref["cands"]})
    out = model.caption_constrained(waves, banned=first + ["no-such-word"], sr=32000, task="clotho", beam_size=3)
    ban_ids = {tok.token_to_id(w) for w in first}
    for _, _, toks in _rows(out["mult_preds"].cpu(), out["mult_lprobs"].cpu()):
        assert not ban_ids & set(toks), toks
    assert all(not set(first) & set(c.split()) for cands in out["mult_cands"] for c in cands)
    assert out["cands"] != ref["cands"]
    by_id = model.caption_constrained(waves, banned=torch.as_tensor(sorted(ban_ids)), sr=32000, task="clotho", beam_size=3)
    assert torch.equal(by_id["mult_preds"], out["mult_preds"])
    bos = model.batch_to_task_token_ids(["clotho"] * len(waves), [None] * len(waves)).tolist()
    for n in (1, 2):
        rep = model.caption_constrained(waves, no_repeat_ngram_size=n, sr=32000, task="clotho", beam_size=3, forbid_rep_mode="none",
                                        min_pred_size=12, max_pred_size=14)
        seen = 0
        for b, _, toks in _rows(rep["mult_preds"].cpu(), rep["mult_lprobs"].cpu()):
            assert not CS.has_repeated_ngram([int(bos[b])] + toks, n), (n, toks)
            seen += 1
        assert seen > 0


def test_value_errors(model, waves):
    tok = model.tokenizer
    w = lambda *ids: " ".join(tok.id_to_token(i) for i in ids)
    kw = dict(sr=32000, task="clotho")
    with pytest.raises(ValueError, match="no-such-word"):
        model.caption_constrained(waves, prefix="no-such-word", **kw)
    for bad in (tok.eos_token, tok.pad_token, tok.bos_token):
        with pytest.raises(ValueError, match=bad):
            model.caption_constrained(waves, prefix=w(40) + " " + bad, **kw)
    with pytest.raises(ValueError, match="banned"):
        model.caption_constrained(waves, prefix=w(40, 41), banned=[w(41)], **kw)
    with pytest.raises(ValueError, match="2-gram"):
        model.caption_constrained(waves, prefix=w(40, 41, 40, 41), no_repeat_ngram_size=2, forbid_rep_mode="none", **kw)
    content = int(torch.nonzero(model.get_forbid_rep_mask("content_words").cpu())[10])      # (behind the four special tokens: a word)
    with pytest.raises(ValueError, match="forbid"):
        model.caption_constrained(waves, prefix=w(content, 40, content), forbid_rep_mode="content_words", **kw)
    with pytest.raises(ValueError, match="max_pred"):
        model.caption_constrained(waves, prefix=w(40, 41, 42), max_pred_size=3, **kw)
    with pytest.raises(ValueError, match="<eos>"):
        model.caption_constrained(waves, banned=[tok.eos_token], **kw)
    with pytest.raises(ValueError, match="beam"):
        model.caption_constrained(waves, beam_size=17, **kw)
    with pytest.raises(ValueError, match="no_repeat_ngram"):
        model.caption_constrained(waves, no_repeat_ngram_size=65, **kw)
    with pytest.raises(ValueError, match="strings for"):
        model.caption_constrained(waves, prefix=[w(40)] * 3, **kw)


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
        main_predict(["--audio", *paths, "--model_name", model_dir, "--prefix", "w40", "--sample", "3"])
    cache = tmp_path / "audioset_mapping"
    cache.mkdir()
    with open(cache / "class_labels_indices.csv", "w") as f:
        f.write("index,mid,display_name\n" + "".join(f"{i},/m/{i},tag{i}\n" for i in range(527)))
    os.environ["CONETTE_AUDIOSET_CACHE"] = str(cache)
    try:
        config = CoNeTTEConfig.from_pretrained(model_dir)
        tok = CoNeTTEModel.from_pretrained(model_dir, config=config, precision="bf16", offline=True, audioset_idx_to_name=TAGS,
                                           stopwords=synth.synth_stopwords()).tokenizer
        words = [tok.id_to_token(i) for i in (40, 41, 42)]
        out_csv = str(tmp_path / "out.csv")
        res = main_predict(["--audio", *paths, "--task", "audiocaps", "--model_name", model_dir, "--precision", "bf16", "--csv_export", out_csv,
                            "--verbose", "0", "--prefix", " ".join(words[:2]), "--ban_words", words[2], "nope", "--no_repeat_ngram", "2"])
    finally:
        os.environ.pop("CONETTE_AUDIOSET_CACHE", None)
    assert [r["audio"] for r in res] == ["clip0.wav", "clip1.wav"] and all(r["task"] == "audiocaps" for r in res)
    assert all(r["candidate"].startswith(" ".join(words[:2])) and words[2] not in r["candidate"].split() for r in res)
    rows = list(csv.DictReader(open(out_csv)))
    assert len(rows) == 2 and [r["candidate"] for r in rows] == [r["candidate"] for r in res]
