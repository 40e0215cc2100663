"""CPU: the host side of word-to-audio alignment (conette_amd/alignment.py) on hand-made maps, the exported symbols, and the
reference of tests/test_gpu_align.py: ``forcing_with_attention_fp32`` / ``_operands``, a restatement of the one-pass decoder that
also returns every layer's head-mean cross-attention.  It is tied to the pinned oracles through its logits --
oracle.cpu_ref.teacher_forcing (to 1e-6) in its fp32 form, oracle.bf16_ref.teacher_forcing_bf16 (exactly) in its operand form --
on the forcing cases of tests/decoder_geometry.py."""
import math
import os

import pytest
import torch
from torch.nn import functional as F

from tests import decoder_geometry as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mha_with_weights(x_q, x_kv, w_in, b_in, w_out, b_out, nhead, key_padding_mask):
    """oracle.cpu_ref._mha (no attn_mask), statement for statement, returning the soft-max (R, nhead, tq, tk) as well"""
    tq, r, e = x_q.shape
    tk = x_kv.shape[0]
    dh = e // nhead
    q = F.linear(x_q, w_in[:e], b_in[:e])
    k = F.linear(x_kv, w_in[e: 2 * e], b_in[e: 2 * e])
    v = F.linear(x_kv, w_in[2 * e:], b_in[2 * e:])
    q = q.reshape(tq, r * nhead, dh).transpose(0, 1)
    k = k.reshape(tk, r * nhead, dh).transpose(0, 1)
    v = v.reshape(tk, r * nhead, dh).transpose(0, 1)
    q = q * math.sqrt(1.0 / float(dh))
    scores = torch.bmm(q, k.transpose(1, 2))
    kpm = torch.zeros(key_padding_mask.shape, dtype=scores.dtype).masked_fill(key_padding_mask, -math.inf)
    scores = (scores.view(r, nhead, tq, tk) + kpm[:, None, None, :]).view(r * nhead, tq, tk)
    attn = torch.softmax(scores, dim=-1)
    out = torch.bmm(attn, v).transpose(0, 1).reshape(tq, r, e)
    return F.linear(out, w_out, b_out), attn.view(r, nhead, tq, tk)


@torch.no_grad()
def forcing_with_attention_fp32(w, audio, audio_shape, caps_in, *, n_layers, pad_id=0, nhead=8):
    """oracle.cpu_ref.teacher_forcing (encode_audio + decoder_forward) with every layer's cross-attention weights kept:
    (logits (B, V, t), [per layer: (B, t, Ta) mean over heads; 0 in rows of pad inputs])."""
    from oracle import cpu_ref as O
    P = "model.decoder."
    memory_bdt, mask = O.encode_audio(w, audio, audio_shape)
    memory, caps, caps_pad = memory_bdt.permute(2, 0, 1), caps_in.permute(1, 0), caps_in.eq(pad_id)
    d, t = w[P + "emb_layer.weight"].shape[1], caps.shape[0]
    x = F.embedding(caps, w[P + "emb_layer.weight"]) * math.sqrt(d) + w[P + "pos_encoding.pos_embedding"][:t]
    sq_mask = O.tp.generate_square_subsequent_mask(t)
    maps = []
    for l in range(n_layers):
        p = P + f"layers.{l}."
        ln = lambda y, i: F.layer_norm(y, (d,), w[p + f"norm{i}.weight"], w[p + f"norm{i}.bias"], 1e-5)
        x = ln(x + O._mha(x, x, w[p + "self_attn.in_proj_weight"], w[p + "self_attn.in_proj_bias"], w[p + "self_attn.out_proj.weight"],
                          w[p + "self_attn.out_proj.bias"], nhead, sq_mask, caps_pad), 1)
        ca, pr = _mha_with_weights(x, memory, w[p + "multihead_attn.in_proj_weight"], w[p + "multihead_attn.in_proj_bias"],
                                   w[p + "multihead_attn.out_proj.weight"], w[p + "multihead_attn.out_proj.bias"], nhead, mask)
        maps.append(pr.mean(dim=1) * caps_in.ne(pad_id)[..., None])
        x = ln(x + ca, 2)
        x = ln(x + F.linear(F.gelu(F.linear(x, w[p + "linear1.weight"], w[p + "linear1.bias"])), w[p + "linear2.weight"],
                            w[p + "linear2.bias"]), 3)
    return F.linear(x, w[P + "classifier.weight"], w[P + "classifier.bias"]).permute(1, 2, 0), maps


@torch.no_grad()
def forcing_with_attention_operands(w, audio, audio_shape, caps_in, *, n_layers, pad_id=0, nhead=8):
    """oracle.bf16_ref.teacher_forcing_bf16, statement for statement (call it inside ``bf16_ref.operands(kind)``), with every
    layer's cross-attention weights kept: the same pair as ``forcing_with_attention_fp32``."""
    from oracle.bf16_ref import bf16 as rnd
    P = "model.decoder."
    d = w[P + "emb_layer.weight"].shape[1]
    b, t = caps_in.shape
    scale = 1.0 / ((d // nhead) ** 0.5)
    mem = rnd(F.relu(F.linear(rnd(audio), rnd(w["model.projection.2.weight"]), w["model.projection.2.bias"])))
    ta = mem.shape[1]
    lens = audio_shape[:, 1].clamp(1, ta)
    mem_mask = (torch.arange(ta)[None, :] >= lens[:, None])[:, None, :].expand(b, t, ta)
    self_mask = torch.triu(torch.ones(t, t, dtype=torch.bool), diagonal=1)[None].expand(b, t, t) | caps_in.eq(pad_id)[:, None, :]

    def attend(q, k, v, mask):
        heads = lambda x: x.view(b, x.shape[1], nhead, d // nhead).transpose(1, 2)
        p = torch.softmax(torch.matmul(heads(q), heads(k).transpose(2, 3)).masked_fill(mask[:, None], float("-inf")), dim=-1)
        return torch.matmul(p, heads(v)).transpose(1, 2).reshape(b, q.shape[1], d), p

    x = F.embedding(caps_in, w[P + "emb_layer.weight"]) * (d ** 0.5) + w[P + "pos_encoding.pos_embedding"][:t, 0][None]
    maps = []
    for l in range(n_layers):
        p = P + f"layers.{l}."
        ln = lambda y, i: F.layer_norm(y, (d,), w[p + f"norm{i}.weight"], w[p + f"norm{i}.bias"], 1e-5)
        qkv = F.linear(rnd(x), rnd(w[p + "self_attn.in_proj_weight"]), w[p + "self_attn.in_proj_bias"])
        a, _ = attend(qkv[..., :d] * scale, rnd(qkv[..., d:2 * d]), rnd(qkv[..., 2 * d:]), self_mask)
        x = ln(x + F.linear(rnd(a), rnd(w[p + "self_attn.out_proj.weight"]), w[p + "self_attn.out_proj.bias"]), 1)
        wi, bi = w[p + "multihead_attn.in_proj_weight"], w[p + "multihead_attn.in_proj_bias"]
        q2 = F.linear(rnd(x), rnd(wi[:d]), bi[:d]) * scale
        k2, v2 = rnd(F.linear(mem, rnd(wi[d:2 * d]), bi[d:2 * d])), rnd(F.linear(mem, rnd(wi[2 * d:]), bi[2 * d:]))
        c, pr = attend(q2, k2, v2, mem_mask)
        maps.append(pr.mean(dim=1) * caps_in.ne(pad_id)[..., None])
        x = ln(x + F.linear(rnd(c), rnd(w[p + "multihead_attn.out_proj.weight"]), w[p + "multihead_attn.out_proj.bias"]), 2)
        h = rnd(F.gelu(F.linear(rnd(x), rnd(w[p + "linear1.weight"]), w[p + "linear1.bias"])))
        x = ln(x + F.linear(h, rnd(w[p + "linear2.weight"]), w[p + "linear2.bias"]), 3)
    logits = F.linear(rnd(x), rnd(w[P + "classifier.weight"]), w[P + "classifier.bias"])
    return logits.permute(0, 2, 1), maps


def reference_maps(g, kind, inputs=None):
    """The restatement on a geometry's forcing case (or on ``inputs`` = (fe, shape, caps)): "fp32", or "bf16" / "f16" operands."""
    from oracle import bf16_ref as Bf
    fe, shape, caps = inputs or D.forcing_inputs(g, g.forcing)
    if kind == "fp32":
        return forcing_with_attention_fp32(D.weights(g), fe, shape, caps, n_layers=g.n_layers)
    with Bf.operands(kind):
        return forcing_with_attention_operands(D.weights(g), fe, shape, caps, n_layers=g.n_layers)


# ---- the restatement against the pinned oracles --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [g.name for g in D.GEOMETRIES])
def test_restatement_logits_match_the_oracles(name):
    from oracle import bf16_ref as Bf
    from oracle import cpu_ref as O
    g = D.geometry(name)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    fe, shape, caps = D.forcing_inputs(g, g.forcing)
    try:
        logits, maps = reference_maps(g, "fp32")
        ref = O.teacher_forcing(D.weights(g), fe, shape, caps, n_layers=g.n_layers)
        err = float((logits - ref).abs().max())
        print(f"restatement {name}: max |d logit| against cpu_ref {err:.3e}")
        assert err <= 1e-6, (name, err)
        for kind in D.H16:
            got, maps16 = reference_maps(g, kind)
            with Bf.operands(kind):
                ref16 = Bf.teacher_forcing_bf16(D.weights(g), fe, shape, caps, n_layers=g.n_layers)
            assert torch.equal(got, ref16), (name, kind)
        # the maps are distributions over the clip's frames, zero behind its length and in pad rows
        f = g.forcing
        assert len(maps) == g.n_layers
        for m in maps + maps16:
            assert tuple(m.shape) == (f.b, f.cap_len, f.ta)
            for i, n in enumerate(f.frame_lens):
                assert float(m[i, :, n:].abs().max()) == 0.0 if n < f.ta else True
                assert float(m[i, f.n_valid[i]:].abs().max()) == 0.0 if f.n_valid[i] < f.cap_len else True
                torch.testing.assert_close(m[i, :f.n_valid[i]].sum(dim=-1), torch.ones(f.n_valid[i]), rtol=0, atol=1e-5)
    finally:
        D.drop_weights(g)


# ---- alignment.py on hand-made maps --------------------------------------------------------------------------------------------
def test_frame_clock():
    from conette_amd import alignment as A
    assert A.FRAME_SEC == 0.32
    assert A.frame_times(3).tolist() == [0.5 * 0.32, 1.5 * 0.32, 2.5 * 0.32]
    assert A.frame_times(0).numel() == 0


def test_one_hot_row():
    from conette_amd import alignment as A
    a = torch.zeros(1, 1, 6)
    a[0, 0, 4] = 1.0
    s = A.summarize(a, torch.tensor([6]))
    assert s["peak_frame"].tolist() == [[4]] and s["mean_frame"].tolist() == [[4.0]] and s["spread"].tolist() == [[0.0]]
    for mass in (0.5, 1.0, 1e-3):
        lo, hi = A.span(a, mass)
        assert (lo.tolist(), hi.tolist()) == ([[4]], [[5]]), mass
    t = A.times(a)
    assert t["peak_time"].tolist() == [[4.5 * A.FRAME_SEC]] and t["mean_time"].tolist() == [[4.5 * A.FRAME_SEC]]
    assert t["span_time"].tolist() == [[[4 * A.FRAME_SEC, 5 * A.FRAME_SEC]]]


def test_two_peaks_with_a_tie():
    from conette_amd import alignment as A
    a = torch.tensor([[0.0, 0.5, 0.0, 0.0, 0.5, 0.0]])
    s = A.summarize(a)
    assert s["peak_frame"].tolist() == [1], "the lowest index among equal maxima"
    assert s["mean_frame"].tolist() == [2.5] and s["spread"].tolist() == [1.5]
    assert tuple(x.tolist() for x in A.span(a, 0.5)) == ([1], [2]), "the earliest of the two one-frame windows"
    assert tuple(x.tolist() for x in A.span(a, 0.51)) == ([1], [5])
    assert tuple(x.tolist() for x in A.span(a, 1.0)) == ([1], [5])
    b = torch.tensor([[0.125, 0.375, 0.375, 0.125]])     # windows [0, 2) and [1, 3) both hold a half; [1, 3) alone holds 0.75
    assert tuple(x.tolist() for x in A.span(b, 0.5)) == ([0], [2])
    assert tuple(x.tolist() for x in A.span(b, 0.75)) == ([1], [3])
    assert tuple(x.tolist() for x in A.span(b, 1.0)) == ([0], [4])


def test_row_ending_at_frame_lens():
    from conette_amd import alignment as A
    a = torch.tensor([[[0.0, 0.125, 0.125, 0.75, 0.0, 0.0]], [[0.125, 0.125, 0.0625, 0.0625, 0.125, 0.5]]])      # (2 clips, 1 row, 6 frames)
    lens = torch.tensor([4, 6])
    s = A.summarize(a, lens)
    assert s["peak_frame"].tolist() == [[3], [5]]
    assert s["mean_frame"][0, 0].item() == 2.625 and s["mean_frame"][1, 0].item() == 3.4375
    lo, hi = A.span(a, 0.5, lens)
    assert (lo.tolist(), hi.tolist()) == ([[3], [5]], [[4], [6]])
    lo, hi = A.span(a, 1.0, lens)
    assert (lo.tolist(), hi.tolist()) == ([[1], [0]], [[4], [6]])
    # weight behind a clip's length does not count: it is masked, and the rest is read as it stands
    dirty = a.clone()
    dirty[0, 0, 5] = 9.0
    assert A.summarize(dirty, lens)["peak_frame"].tolist() == [[3], [5]]
    assert A.summarize(dirty)["peak_frame"].tolist() == [[5], [5]]
    assert float(A.times(a, lens)["peak_time"].max()) < 6 * A.FRAME_SEC


def test_pad_rows():
    from conette_amd import alignment as A
    a = torch.zeros(2, 3, 5)
    a[0, 0, 2] = 1.0
    a[1, 1] = torch.tensor([0.25, 0.25, 0.25, 0.25, 0.0])
    s = A.summarize(a, torch.tensor([5, 4]))
    assert s["peak_frame"].tolist() == [[2, -1, -1], [-1, 0, -1]]
    pad = s["peak_frame"] < 0
    assert bool(torch.isnan(s["mean_frame"][pad]).all()) and bool(torch.isnan(s["spread"][pad]).all())
    assert bool(torch.isfinite(s["mean_frame"][~pad]).all())
    lo, hi = A.span(a, 0.5)
    assert lo.tolist() == [[2, -1, -1], [-1, 0, -1]] and hi.tolist() == [[3, -1, -1], [-1, 2, -1]]
    t = A.times(a)
    for k in ("peak_time", "mean_time"):
        assert bool(torch.isnan(t[k][pad]).all()) and bool(torch.isfinite(t[k][~pad]).all()), k
    assert bool(torch.isnan(t["span_time"][pad]).all()) and tuple(t["span_time"].shape) == (2, 3, 2)
    with pytest.raises(ValueError, match="mass"):
        A.span(a, 0.0)
    with pytest.raises(ValueError, match="mass"):
        A.span(a, 1.5)


def test_full_mass_is_the_support():
    from conette_amd import alignment as A
    g = torch.Generator().manual_seed(3)
    a = torch.rand(7, 33, generator=g).float()
    a[:, :3] = 0
    a[:, 29:] = 0
    a[2, 3] = 0                                        # a support that starts later
    a = a / a.sum(dim=-1, keepdim=True)
    lo, hi = A.span(a, 1.0)
    assert lo.tolist() == [3, 3, 4, 3, 3, 3, 3] and hi.tolist() == [29] * 7
    half_lo, half_hi = A.span(a, 0.5)
    for i in range(7):                                # brute force: the shortest, then the earliest window
        best = min(((e - s, s) for s in range(33) for e in range(s + 1, 34) if float(a[i, s:e].double().sum()) >= 0.5 * float(a[i].double().sum()) - 1e-12))
        assert (int(half_hi[i] - half_lo[i]), int(half_lo[i])) == best, i


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_align_is_declared_and_exported():
    import re
    from conette_amd import engine
    assert {"conette_align", "conette_align_workspace_bytes"} <= set(engine.EXPORTS)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "conette_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(conette_[a-z0-9_]+)\s*\(", hdr))
    assert {"conette_align", "conette_align_workspace_bytes"} <= declared
    assert "#define CONETTE_ABI_VERSION 3" in open(os.path.join(ROOT, "include", "conette_hip.h")).read()
    lib = engine.load_library()
    assert hasattr(lib, "conette_align") and hasattr(lib, "conette_align_workspace_bytes")
    assert lib.conette_abi_version() == 3
    assert lib.conette_align_workspace_bytes(None, 1, 1, 1, 1, 0) == 0


def test_predict_rows_of_an_alignment():
    from types import SimpleNamespace
    from conette_amd.predict import format_alignment
    tok = SimpleNamespace(pad_token_id=0, bos_token_id=1, eos_token_id=2, id_to_token=lambda i: f"w{i}")
    nan = float("nan")
    outs = {"tokens": torch.tensor([[[7, 9, 2, 0]], [[5, 2, 0, 0]]]),
            "span_time": torch.tensor([[[[0.0, 0.32], [0.64, 1.6], [0.0, 0.32], [nan, nan]]], [[[0.32, 0.64], [0.0, 0.32], [nan, nan], [nan, nan]]]])}
    rows = format_alignment(["/x/a.wav", "b.wav"], ["clotho", "audiocaps"], tok, outs)
    assert rows == [{"audio": "a.wav", "task": "clotho", "word": "w7", "start": "0.00", "end": "0.32"},
                    {"audio": "a.wav", "task": "clotho", "word": "w9", "start": "0.64", "end": "1.60"},
                    {"audio": "b.wav", "task": "audiocaps", "word": "w5", "start": "0.32", "end": "0.64"}]
