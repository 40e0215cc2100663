"""GPU: the Python surface of the caption timeline -- CoNeTTEModel.caption_segments / caption_spans and ``conette-predict --segments`` --
on the default synthetic checkpoint with two recordings of 13 s and 8 s (40 and 25 encoder frames), windows of 2.56 s every 1.28 s
(8 frames every 4).  The host rules are segments.span_table / merge_batch; the search is held to Engine.decode on the gathered
windows and, in precision fp32, to the CPU oracle's beam search on the sliced projected memory."""
import os
import wave

import numpy as np
import pytest
import torch

from conette_amd import segments as S
from conette_amd import synth
from conette_amd.alignment import FRAME_SEC

pytestmark = pytest.mark.gpu
TAGS = {i: f"tag{i}" for i in range(527)}
LENGTHS = (13 * 32000, 8 * 32000)
WINDOW = dict(window_s=2.56, hop_s=1.28)
TASKS = ["clotho", "audiocaps"]
ORACLE_SEED = 37                 # seeded frames for the oracle comparison: see oracle_case()
ORACLE_FRAMES = (40, 25)


@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    return synth.write_pretrained_dir(str(tmp_path_factory.mktemp("conette_synth_segments")))


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
    w = torch.from_numpy(synth.synth_waveforms(2, max(LENGTHS), 31, lengths=list(LENGTHS)))
    return [w[i:i + 1, :n].contiguous() for i, n in enumerate(LENGTHS)]


@pytest.fixture(scope="module")
def encoded(model, waves):
    """(frame_embs (2, T, 768) on the device, audio_shape (2, 2)): one encode that every test below reads"""
    with torch.no_grad(), torch.cuda.device(model.device):
        audio, shape = model._frame_embeddings(waves, 32000, None, True)
    shape = torch.as_tensor(shape).cpu()
    assert shape[:, 1].tolist() == [40, 25]
    return audio.clone(), shape


@pytest.fixture(scope="module")
def timeline(model, encoded):
    fe, shape = encoded
    return model.caption_segments(fe, x_shapes=shape, preprocess=False, task=TASKS, beam_size=2, **WINDOW)


def fbits(t):
    return torch.as_tensor(t).contiguous().view(torch.int32)


def test_windows_equal_decode_on_gathered_windows(model, encoded, timeline):
    fe, shape = encoded
    lens = shape[:, 1].numpy()
    table, counts = S.span_table(lens, 8, 4)
    assert counts.tolist() == [9, 6] and [len(c) for c in timeline["window_cands"]] == [9, 6]
    clips = torch.zeros((table.shape[0], 8, 768), device=fe.device)
    for s, (r, start, ln) in enumerate(table.tolist()):
        clips[s, :ln] = fe[r, start:start + ln]
    _, dataset_lst, source_lst = model._split_tasks(TASKS, 2)
    bos = model.batch_to_task_token_ids(dataset_lst, source_lst)[torch.from_numpy(table[:, 0].astype(np.int64))]
    cfg = model.config
    ref = model.engine.decode(clips, torch.from_numpy(np.ascontiguousarray(table[:, 2])), bos, model.get_forbid_rep_mask(None), 2,
                              cfg.min_pred_size, cfg.max_pred_size)
    pred_size, best_maxlen = ref["sizes"].tolist()
    got = torch.cat(timeline["window_preds"]).cpu()
    assert got.dtype == torch.long and torch.equal(got, ref["best_preds"][:, :best_maxlen].long().cpu())
    assert torch.equal(fbits(torch.cat(timeline["window_lprobs"])), fbits(ref["best_lprobs"].cpu()))
    flat = [c for cands in timeline["window_cands"] for c in cands]
    assert flat == model.tokenizer.decode_rec(got) and all(isinstance(c, str) for c in flat)
    assert torch.equal(torch.cat(timeline["window_frames"]), torch.from_numpy(table[:, 1:]))
    times = [t for rec in timeline["window_times"] for t in rec]
    assert times == [(int(a) * FRAME_SEC, (int(a) + int(b)) * FRAME_SEC) for a, b in table[:, 1:]]
    assert timeline["frame_sec"] == FRAME_SEC and timeline["tasks"] == TASKS


def rule_on(out, **kw):
    """segments.merge_batch on a call's own window outputs"""
    n = len(out["window_preds"])
    wmax = max(p.shape[0] for p in out["window_preds"])
    l = out["window_preds"][0].shape[1]
    preds = np.zeros((n, wmax, l), dtype=np.int32)
    lprobs = np.zeros((n, wmax), dtype=np.float32)
    spans = np.zeros((n, wmax, 2), dtype=np.int32)
    nw = np.zeros(n, dtype=np.int32)
    for r in range(n):
        w = out["window_preds"][r].shape[0]
        preds[r, :w], lprobs[r, :w], spans[r, :w], nw[r] = out["window_preds"][r].cpu().numpy(), out["window_lprobs"][r].cpu().numpy(), \
            out["window_frames"][r].numpy(), w
    return S.merge_batch(preds, nw, lprobs, spans, **kw), nw


def check_segments(out, want, nw, max_segments=64):
    assert out["segment_counts"].tolist() == want["counts"].tolist()
    assert out["segments_truncated"].tolist() == (want["counts"] > max_segments).tolist()
    assert np.array_equal(out["adjacency"].numpy().view(np.int32), want["adjacency"].view(np.int32))
    for r, segs in enumerate(out["segments"]):
        assert len(segs) == min(int(want["counts"][r]), max_segments)
        for k, s in enumerate(segs):
            rep = int(want["seg_rep"][r, k])
            assert s["windows"] == tuple(want["seg_windows"][r, k].tolist())
            assert (s["onset"], s["offset"]) == tuple(int(f) * FRAME_SEC for f in want["seg_frames"][r, k])
            assert s["caption"] == out["window_cands"][r][rep] and torch.equal(s["pred"], out["window_preds"][r][rep])
            assert np.float32(s["lprob"]) == out["window_lprobs"][r][rep].numpy() and np.float32(s["agreement"]) == want["seg_agree"][r, k]
        assert segs[0]["onset"] == 0.0 and (want["counts"][r] > max_segments or segs[-1]["windows"][1] == nw[r])
        assert all(a["offset"] == b["onset"] and a["windows"][1] == b["windows"][0] for a, b in zip(segs, segs[1:]))


def test_segments_equal_the_rule_on_the_windows(model, encoded, timeline):
    want, nw = rule_on(timeline, threshold=0.5)
    check_segments(timeline, want, nw)
    assert timeline["segments"][0][-1]["offset"] == 40 * FRAME_SEC and timeline["segments"][1][-1]["offset"] == 25 * FRAME_SEC
    fe, shape = encoded
    for kw, rule_kw in ((dict(utility="edit", merge_threshold=0.3), dict(utility="edit", threshold=0.3)),
                        (dict(max_order=1, merge_threshold=0.25, max_run_s=4.0), dict(max_order=1, threshold=0.25, max_run=2)),
                        (dict(merge_threshold=0.0, max_segments=1, max_run_s=2.56), dict(threshold=0.0, max_segments=1, max_run=1))):
        out = model.caption_segments(fe, x_shapes=shape, preprocess=False, task=TASKS, beam_size=2, **WINDOW, **kw)
        assert all(torch.equal(a, b) for a, b in zip(out["window_preds"], timeline["window_preds"]))
        want, nw = rule_on(out, **rule_kw)
        check_segments(out, want, nw, rule_kw.get("max_segments", 64))
    assert out["segments_truncated"].tolist() == [True, True] and out["segment_counts"].tolist() == [9, 6]


def test_threshold_extremes(model, encoded, timeline):
    fe, shape = encoded
    every = model.caption_segments(fe, x_shapes=shape, preprocess=False, task=TASKS, beam_size=2, merge_threshold=None, **WINDOW)
    assert [[s["windows"] for s in segs] for segs in every["segments"]] == [[(k, k + 1) for k in range(9)], [(k, k + 1) for k in range(6)]]
    assert [[s["caption"] for s in segs] for segs in every["segments"]] == timeline["window_cands"]
    assert all(s["agreement"] == 1.0 for segs in every["segments"] for s in segs)
    whole = model.caption_segments(fe, x_shapes=shape, preprocess=False, task=TASKS, beam_size=2, merge_threshold=0.0, max_run_s=0.0, **WINDOW)
    assert [[s["windows"] for s in segs] for segs in whole["segments"]] == [[(0, 9)], [(0, 6)]]
    assert [(segs[0]["onset"], segs[0]["offset"]) for segs in whole["segments"]] == [(0.0, 40 * FRAME_SEC), (0.0, 25 * FRAME_SEC)]
    for r, segs in enumerate(whole["segments"]):
        assert segs[0]["lprob"] == float(timeline["window_lprobs"][r].max())


def test_caption_spans_on_the_grid_and_with_waveforms(model, encoded, timeline, waves):
    fe, shape = encoded
    seconds = [[(a, b) for a, b in rec] for rec in timeline["window_times"]]
    out = model.caption_spans(fe, seconds, task=TASKS, beam_size=2, x_shapes=shape, preprocess=False)
    assert out["cands"] == timeline["window_cands"] and out["tasks"] == TASKS
    for r in range(2):
        assert torch.equal(out["preds"][r], timeline["window_preds"][r]) and torch.equal(out["span_frames"][r], timeline["window_frames"][r])
        assert torch.equal(fbits(out["lprobs"][r].cpu()), fbits(timeline["window_lprobs"][r]))
        assert out["mult_preds"][r].shape[:2] == (len(seconds[r]), 2) and len(out["mult_cands"][r]) == len(seconds[r])
    # an offset beyond the recording's end is cut there; an onset beyond it raises
    cut = model.caption_spans(fe, [[(10.24, 99.0)], [(0.0, 1.0)]], task=TASKS, beam_size=2, x_shapes=shape, preprocess=False)
    assert cut["span_frames"][0].tolist() == [[32, 8]] and cut["cands"][0] == [timeline["window_cands"][0][8]]
    with pytest.raises(ValueError, match=r"spans\[1\]\[0\]"):
        model.caption_spans(fe, [[(0.0, 1.0)], [(8.0, 9.0)]], x_shapes=shape, preprocess=False)
    with pytest.raises(ValueError, match="2 recordings"):
        model.caption_spans(fe, [[(0.0, 1.0)]], x_shapes=shape, preprocess=False)
    # waveforms in: the preprocessor's tags come along
    full = model.caption_segments(waves, sr=32000, task=TASKS, beam_size=2, **WINDOW)
    assert set(full) == set(timeline) | {"tags", "tags_probs"} and full["tags_probs"].shape == (2, 527)
    assert [len(c) for c in full["window_cands"]] == [9, 6] and full["segment_counts"].tolist() == [len(s) for s in full["segments"]]


# ---- the CPU oracle -----------------------------------------------------------------------------------------------------------------
def oracle_case(seed=ORACLE_SEED):
    """(frame_embs (2, 40, 768), audio_shape, table, oracle results, smallest margin of any top-k call): seeded frames at the
    encoder's scale, windows of 8 frames every 4, the oracle's beam search (beam 2) on the windows cut from the projected memory.
    ORACLE_SEED is the first of the seeds 0 .. 39 at which every decision of the oracle's own search clears 1e-2 -- ten times the
    near-tie line of the fp32 model tests (1e-3) --, found by running this function on the CPU."""
    from oracle import cpu_ref as O
    rng = np.random.Generator(np.random.PCG64(93000 + seed))
    fe = ((rng.random((2, max(ORACLE_FRAMES), 768)) * 2.0 - 1.0) * (0.65 * 3 ** 0.5)).astype(np.float32)
    shape = torch.tensor([[768, n] for n in ORACLE_FRAMES], dtype=torch.int64)
    table, _ = S.span_table(ORACLE_FRAMES, 8, 4)
    w = O.to_torch(synth.synth_state_dict())
    cfg = synth.synth_config_dict()
    task_idx = torch.as_tensor([cfg["task_names"].index(t) for t in TASKS])[torch.from_numpy(table[:, 0].astype(np.int64))]
    with torch.no_grad():
        mem, _ = O.encode_audio(w, torch.from_numpy(fe), shape)                  # (2, 256, 40)
        cut = torch.stack([mem[r, :, a:a + n] for r, a, n in table.tolist()])   # every window has 8 frames here
        mask = torch.zeros((cut.shape[0], 8), dtype=torch.bool)
        trace: list = []
        ref = O.generate(w, cut, mask, w["model.task_id_to_token_id"][task_idx], vocab_size=w["model.decoder.classifier.weight"].shape[0],
                         beam_size=2, min_pred_size=cfg["min_pred_size"], max_pred_size=cfg["max_pred_size"],
                         forbid_rep_mask=w["model.forbid_rep_mask"], trace=trace)
    # a call's margin to the first rejected candidate, and the gaps between its picks (their order assigns the slots of mult_preds)
    gaps = [d["margin"] for step in trace for d in step]
    gaps += [d["sum_lprob"][i] - d["sum_lprob"][i + 1] for step in trace for d in step for i in range(len(d["parent"]) - 1)]
    return torch.from_numpy(fe), shape, table, ref, float(min(gaps))


def test_caption_spans_fp32_equals_the_cpu_oracle(model_dir):
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    fe, shape, table, ref, margin = oracle_case()
    assert (table[:, 2] == 8).all() and table.shape[0] == 15
    assert margin > 1e-3, margin        # (no case is skipped: the seed was picked for it)
    model32 = load(model_dir, "fp32")
    seconds = [[(int(a) * FRAME_SEC, (int(a) + int(n)) * FRAME_SEC) for r, a, n in table.tolist() if r == rec] for rec in range(2)]
    out = model32.caption_spans(fe, seconds, task=TASKS, beam_size=2, x_shapes=shape, preprocess=False)
    assert torch.cat(out["preds"]).cpu().tolist() == ref[0].tolist()
    assert torch.cat(out["mult_preds"]).cpu().tolist() == ref[2].tolist()
    np.testing.assert_allclose(torch.cat(out["lprobs"]).cpu().numpy(), ref[1].numpy(), atol=1e-3)


def test_predict_cli_writes_segment_rows(model_dir, tmp_path):
    import csv
    from conette_amd.predict import main_predict
    paths = []
    for i, n in enumerate((5 * 32000, 3 * 32000)):
        wav = synth.synth_waveforms(1, n, 57 + i)[0]
        pcm = np.clip(np.round(wav * 32768.0), -32768, 32767).astype("<i2")
        p = str(tmp_path / f"rec{i}.wav")
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
        res = main_predict(["--audio", *paths, "--task", "clotho", "--model_name", model_dir, "--precision", "bf16", "--verbose", "0",
                            "--segments", "--segment_window", "2.56", "--segment_hop", "1.28", "--segment_merge", "0.5", "--csv_export", out_csv])
    finally:
        os.environ.pop("CONETTE_AUDIOSET_CACHE", None)
    assert {r["audio"] for r in res} == {"rec0.wav", "rec1.wav"} and all(list(r) == ["audio", "onset", "offset", "caption", "lprob"] for r in res)
    for name, frames in (("rec0.wav", 15), ("rec1.wav", 9)):
        rows = [r for r in res if r["audio"] == name]
        assert rows[0]["onset"] == "0.00" and rows[-1]["offset"] == f"{frames * FRAME_SEC:.2f}"
        assert all(a["offset"] == b["onset"] for a, b in zip(rows, rows[1:])) and all(r["caption"] for r in rows)
    assert [dict(r) for r in csv.DictReader(open(out_csv))] == res
