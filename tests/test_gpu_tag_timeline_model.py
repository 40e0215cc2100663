"""GPU: the Python surface of the tag timeline -- CoNeTTEModel.tag_timeline on the default synthetic checkpoint with two waveforms of
1 s and 4 s in (T = 12, lengths 3 and 12); the host rule is tagging.events on the returned frame_probs."""
import json
import os
import wave

import numpy as np
import pytest
import torch

from conette_amd import synth
from conette_amd import tagging as R
from conette_amd.alignment import FRAME_SEC

pytestmark = pytest.mark.gpu
TAGS = {i: f"tag{i}" for i in range(527)}


@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    return synth.write_pretrained_dir(str(tmp_path_factory.mktemp("conette_synth_tags")))


def load(model_dir, precision):
    from conette_amd import CoNeTTEConfig, CoNeTTEModel
    config = CoNeTTEConfig.from_pretrained(model_dir)
    return CoNeTTEModel.from_pretrained(model_dir, config=config, precision=precision, offline=True, audioset_idx_to_name=TAGS,
                                        stopwords=synth.synth_stopwords())


@pytest.fixture(scope="module")
def model(model_dir):
    return load(model_dir, "bf16")


@pytest.fixture(scope="module")
def waves():
    lengths = [32000, 128000]
    w = torch.from_numpy(synth.synth_waveforms(2, 128000, 33, lengths=lengths))
    return [w[i:i + 1, :n].contiguous() for i, n in enumerate(lengths)]


def frame_embs(model, waves):
    audio = model.preprocessor(waves, 32000, None)["audio"]
    return audio.squeeze(dim=1) if audio.ndim == 4 else audio


def expected_events(out, on, off, shortest, gap, m, wanted=None):
    """the event lists the rule gives for the returned frame_probs"""
    p, lens = out["frame_probs"].cpu().numpy(), out["frame_lens"].cpu().numpy()
    clips, counts = [], np.zeros(p.shape[::2], dtype=np.int64)
    for b in range(p.shape[0]):
        found = []
        for c in range(p.shape[2]):
            e = R.events(np.ascontiguousarray(p[b, :, c]), lens[b], on, off, shortest, gap, m)
            counts[b, c] = e["count"]
            if wanted is not None and c not in wanted:
                continue
            for k in range(min(e["count"], m)):
                found.append({"tag": TAGS[c], "index": c, "onset": int(e["spans"][k, 0]) * 0.32, "offset": int(e["spans"][k, 1]) * 0.32,
                              "peak": float(e["peaks"][k]), "peak_time": (int(e["peak_frames"][k]) + 0.5) * 0.32})
        found.sort(key=lambda ev: (ev["onset"], ev["index"]))
        clips.append(found)
    return clips, counts


def test_keys_shapes_and_events(model, waves):
    out = model.tag_timeline(waves, sr=32000)
    assert set(out) == {"frame_probs", "frame_lens", "frame_sec", "event_counts", "events_truncated", "events", "tags_probs", "tags"}
    assert out["frame_probs"].is_cuda and out["frame_probs"].dtype == torch.float32 and tuple(out["frame_probs"].shape) == (2, 12, 527)
    assert out["frame_lens"].tolist() == [3, 12] and out["frame_sec"] == FRAME_SEC == 0.32
    assert tuple(out["event_counts"].shape) == (2, 527) and tuple(out["events_truncated"].shape) == (2,)
    assert out["events_truncated"].dtype == torch.bool and tuple(out["tags_probs"].shape) == (2, 527) and len(out["tags"]) == 2
    assert not bool(out["frame_probs"][0, 3:].any())
    # the defaults: a 7-frame window, on = off = 0.3, no merging, nothing dropped, 16 slots
    want, counts = expected_events(out, 0.3, 0.3, 1, 0, 16)
    assert out["events"] == want and sum(len(c) for c in want) > 100
    assert np.array_equal(out["event_counts"].cpu().numpy(), counts)
    assert out["events_truncated"].tolist() == (counts > 16).any(axis=1).tolist()
    for clip, n in zip(out["events"], (3, 12)):
        assert set(clip[0]) == {"tag", "index", "onset", "offset", "peak", "peak_time"}
        assert all(0 <= e["onset"] < e["peak_time"] < e["offset"] <= n * 0.32 + 1e-9 and e["peak"] >= np.float32(0.3) for e in clip)
    frames = model.engine.tag_frames(frame_embs(model, waves), out["frame_lens"], 7)
    assert torch.equal(frames, out["frame_probs"])


def test_converted_arguments(model, waves):
    """seconds become frames, rounded half up: a 1 s window is 3 frames, 0.64 s at least 2, a 0.32 s gap 1"""
    out = model.tag_timeline(waves, sr=32000, window_s=1.0, threshold=0.5, off_threshold=0.35, min_duration_s=0.64, max_gap_s=0.32, max_events=4)
    frames = model.engine.tag_frames(frame_embs(model, waves), out["frame_lens"], 3)
    assert torch.equal(frames, out["frame_probs"])
    want, counts = expected_events(out, 0.5, 0.35, 2, 1, 4)
    assert out["events"] == want and len(want[1]) > 10 and np.array_equal(out["event_counts"].cpu().numpy(), counts)
    assert all(e["offset"] - e["onset"] >= 0.64 - 1e-9 for clip in out["events"] for e in clip)


def test_tags_filter_the_list_and_nothing_else(model, waves):
    base = model.tag_timeline(waves, sr=32000)
    busiest = [e["index"] for e in base["events"][1]][:3]
    picked = model.tag_timeline(waves, sr=32000, tags=[TAGS[busiest[0]], busiest[1]])
    keep = {busiest[0], busiest[1]}
    assert picked["events"] == [[e for e in clip if e["index"] in keep] for clip in base["events"]] and picked["events"][1]
    for k in ("frame_probs", "event_counts", "events_truncated", "tags_probs"):
        assert torch.equal(picked[k], base[k]), k
    assert model.tag_timeline(waves, sr=32000, tags=TAGS[busiest[2]])["events"][1][0]["index"] == busiest[2]
    with pytest.raises(ValueError, match="no_such_tag"):
        model.tag_timeline(waves, sr=32000, tags=["no_such_tag"])
    with pytest.raises(ValueError, match="527"):
        model.tag_timeline(waves, sr=32000, tags=[527])
    for kw, word in ((dict(window_s=100.0), "window"), (dict(threshold=0.0), "on"), (dict(off_threshold=0.5), "off"),
                     (dict(max_events=65), "max_events"), (dict(max_gap_s=-1.0), "seconds")):
        with pytest.raises(ValueError, match=word):
            model.tag_timeline(waves, sr=32000, **kw)


def test_truncation(model, waves):
    one = model.tag_timeline(waves, sr=32000, window_s=0.32, threshold=0.5, max_events=1)
    many = model.tag_timeline(waves, sr=32000, window_s=0.32, threshold=0.5, max_events=64)
    assert torch.equal(one["event_counts"], many["event_counts"]) and int(one["event_counts"].max()) > 1
    assert one["events_truncated"].tolist() == (one["event_counts"] > 1).any(dim=1).tolist() and one["events_truncated"].tolist()[1]
    assert many["events_truncated"].tolist() == [False, False]
    assert sum(len(c) for c in one["events"]) == int(one["event_counts"].clamp(max=1).sum())
    assert sum(len(c) for c in many["events"]) == int(many["event_counts"].sum())


def test_frame_embeddings_in(model, waves):
    base = model.tag_timeline(waves, sr=32000)
    batch = model.preprocessor(waves, 32000, None)
    out = model.tag_timeline(batch, preprocess=False)
    assert "tags_probs" not in out and "tags" not in out
    assert torch.equal(out["frame_probs"], base["frame_probs"]) and out["events"] == base["events"]
    out = model.tag_timeline(batch["audio"], x_shapes=batch["audio_shape"], preprocess=False)
    assert torch.equal(out["frame_probs"], base["frame_probs"])


def test_certified_precision_runs(model_dir, waves):
    m = load(model_dir, "certified")
    assert m.engine.certified
    out = m.tag_timeline(waves, sr=32000, max_gap_s=0.32)
    want, counts = expected_events(out, 0.3, 0.3, 1, 1, 16)
    assert out["events"] == want and np.array_equal(out["event_counts"].cpu().numpy(), counts)
    assert tuple(out["frame_probs"].shape) == (2, 12, 527) and "tags" in out


def test_forward_is_untouched(model, waves):
    before = model(waves, sr=32000, task="clotho")
    model.tag_timeline(waves, sr=32000, max_events=3)
    after = model(waves, sr=32000, task="clotho")
    for k in ("preds", "lprobs", "tags_probs"):
        assert torch.equal(before[k], after[k]), k
    assert before["cands"] == after["cands"]


def test_predict_cli(model_dir, tmp_path):
    """conette-predict --tag_timeline: the caption rows gain the file's events as one JSON column"""
    import csv
    from conette_amd.predict import main_predict
    paths = []
    for i in range(2):
        wav = synth.synth_waveforms(1, 40000 + 48000 * i, 77 + i)[0]
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
        common = ["--audio", *paths, "--task", "audiocaps", "--model_name", model_dir, "--precision", "bf16", "--verbose", "0"]
        plain = main_predict(common)
        res = main_predict(common + ["--tag_timeline", "--tag_window", "1.0", "--tag_threshold", "0.5", "--tag_off_threshold", "0.35",
                                     "--tag_max_gap", "0.32", "--csv_export", out_csv])
        m = load(model_dir, "bf16")
        want = m.tag_timeline(paths, window_s=1.0, threshold=0.5, off_threshold=0.35, max_gap_s=0.32)
    finally:
        os.environ.pop("CONETTE_AUDIOSET_CACHE", None)
    assert [r["candidate"] for r in res] == [r["candidate"] for r in plain] and [r["audio"] for r in res] == ["clip0.wav", "clip1.wav"]
    rows = list(csv.DictReader(open(out_csv)))
    assert len(rows) == 2 and list(rows[0]) == ["audio", "task", "candidate", "tag_events"]
    for row, r, events in zip(rows, res, want["events"]):
        listed = json.loads(row["tag_events"])
        assert row["tag_events"] == r["tag_events"] and len(listed) == len(events) > 10
        for got, e in zip(listed, events):
            assert got == {"tag": e["tag"], "onset": round(e["onset"], 2), "offset": round(e["offset"], 2), "peak": round(e["peak"], 3)}
