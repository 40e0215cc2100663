"""GPU: the kernels that the benchmark runs (bf16 mode) pinned against the bf16-operand oracle (oracle/bf16_ref.py) on
FULL tensors, block by block, plus the configurations VERDICT r01 listed as untested.

Tolerances: every ConvNeXt block / downsample output rtol 3e-3 + atol 2e-3 of an O(1) activation against the oracle
evaluated on the GPU's own input of that block (so errors do not accumulate across blocks); teacher-forcing logits
(|logit| up to ~40) atol 0.03 + rtol 3e-3 against the oracle's bf16-operand decoder.  The only arithmetic the oracle does not
share with the kernels is the accumulation order and the GELU polynomial (<= 2.5e-5 absolute), which move a few
hidden values per million to the neighbouring bf16.

The same tests run for CONETTE_PREC_F16 (the same kernels instantiated for IEEE fp16 operands) against the same oracle with
its rounding points switched to fp16 (``bf16_ref.operands("f16")``), with every bound that is made of operand rounding
scaled by 1/8 (11 significant bits against 8).  What does NOT scale is the MEAN error against the oracle: it is made of
values that round to the neighbouring operand because the kernels sum in another order than the oracle (fp32 noise d): such
a flip happens with probability d / ulp and moves the value by one ulp, so its expected size is d whatever the operand type
(measured per decoder layer: mean 3e-4..6e-4 in bf16, 5e-4..8e-4 in fp16; max 0.065 against 0.0098).  Mean bounds are
therefore shared; worst-element bounds are scaled (by 1/4 where six chained layers amplify a flip)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import golden_util as G
from tests.block_oracle import FP32_BOUND, ROUNDING, _assert_close, _nchw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["bf16", "f16"])
def eng_bf16(request, synth_weights):
    """The 16-bit engine under test (the name is historical: bf16 and f16 both come through here)."""
    from conette_amd.engine import Engine
    e = Engine(synth_weights, precision=request.param)
    e.test_prec = request.param
    return e


def _wave(g):
    from conette_amd import synth
    n = [int(v) for v in g["lengths"]]
    return torch.from_numpy(synth.synth_waveforms(len(n), max(n), int(g["seed0"]), lengths=n))


@pytest.mark.parametrize("name", ["b8_10s_beam3_all", "b3_mixed_beam3_none"])
def test_every_block_against_bf16_operand_oracle(name, eng_bf16, synth_weights):
    from oracle import bf16_ref as Bf
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    g = G.load(name)
    prec = eng_bf16.test_prec
    k = ROUNDING[prec]
    fe, clip, taps = eng_bf16.encode(_wave(g).cuda(), taps="blocks")
    torch.cuda.synchronize()
    worst = {}
    blk = 0
    for st, depth in enumerate((3, 3, 9, 3)):
        if st > 0:  # downsample_layers[st] from the previous stage's output (LN + patch GEMM, 16-bit operands)
            with torch.no_grad(), Bf.operands(prec):
                ref = Bf.downsample_bf16(synth_weights, st, _nchw(taps[f"stage{st - 1}"]), folded=st <= 2)
            got = _nchw(taps[f"down{st}"])
            _assert_close(got, ref, f"{name}/down{st}", k)
        for b in range(depth):
            src = taps["stem"] if blk == 0 else (taps[f"down{st}"] if b == 0 else taps[f"block{blk - 1}"])
            with torch.no_grad(), Bf.operands(prec):
                ref = Bf.convnext_block_bf16(synth_weights, Bf.block_prefix(blk), _nchw(src), folded=st < 3)
            got = _nchw(taps[f"block{blk}"])
            err = (got - ref).abs()
            worst[blk] = (float(err.max()), float(err.mean()))
            _assert_close(got, ref, f"{name}/block{blk} (stage {st})", k)
            blk += 1
    assert torch.equal(taps["block17"], taps["stage3"]) and torch.equal(taps["block0"], taps["stage0_block0"])
    print("max / mean |err| per block:", {k: (round(a, 5), round(b, 7)) for k, (a, b) in worst.items()})


def test_every_block_against_the_unmodified_fp32_oracle(eng_bf16, synth_weights):
    """the operand oracle (bf16_ref.py) is edited together with the kernels whenever a rounding point moves, so a
    kernel-plus-oracle co-edit could hide a regression.  This assertion does not move with the kernels: every ConvNeXt block's
    output against oracle/cpu_ref.py's plain fp32 block (convnext.py:61-74) on the GPU's own input of that block, with explicit
    ABSOLUTE bounds on the worst element and on the mean (activations are O(1))."""
    from oracle import bf16_ref as Bf
    from oracle import cpu_ref as O
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    g = G.load("b3_mixed_beam3_none")
    prec = eng_bf16.test_prec
    fe, clip, taps = eng_bf16.encode(_wave(g).cuda(), taps="blocks")
    torch.cuda.synchronize()
    worst_max = worst_mean = 0.0
    blk = 0
    for st, depth in enumerate((3, 3, 9, 3)):
        for b in range(depth):
            src = taps["stem"] if blk == 0 else (taps[f"down{st}"] if b == 0 else taps[f"block{blk - 1}"])
            with torch.no_grad():
                ref = O.convnext_block(synth_weights, Bf.block_prefix(blk), _nchw(src))
            err = (_nchw(taps[f"block{blk}"]) - ref).abs()
            worst_max, worst_mean = max(worst_max, float(err.max())), max(worst_mean, float(err.mean()))
            assert float(err.max()) < FP32_BOUND[prec][0] and float(err.mean()) < FP32_BOUND[prec][1], (prec, blk, float(err.max()), float(err.mean()))
            blk += 1
    print(f"{prec}: worst block against the fp32 oracle: max {worst_max:.5f} mean {worst_mean:.6f}")


@pytest.mark.parametrize("copies", [32, 8, 5, 13])
def test_encoder_at_256_clips(copies, eng_bf16):
    """BASELINE config 3's encoder half: 32 copies of the b8_10s fixture batch (B = 256) -- every copy must reproduce
    copy 0 bit for bit in every tap (persistent kernels walk many tiles per wave, tiles straddle clip boundaries at
    stages 1-3), and copy 0 must match the reference fixture like the B = 8 run does.  8 copies (B = 64) is the benchmark's
    shape: its stage-3 products run in other GEMM tiles (224 x 256 and the three-deep 224 x 192 ring) than B = 256
    (224 x 256 throughout) and B = 8 (64 x 64) -- all must agree bit for bit (same k order per output element).  5 and 13
    copies (B = 40, 104) put ragged last tiles and the other branches of the tile-height rule under the same check."""
    g = G.load("b8_10s_beam3_all")
    w8 = _wave(g)
    wave = w8.repeat(copies, 1).cuda()
    fe, clip, taps = eng_bf16.encode(wave, taps=True)
    fe8, clip8, taps8 = eng_bf16.encode(w8.cuda(), taps=True)
    torch.cuda.synchronize()
    for k in ["stem", "stage0_block0", "stage0", "down1", "stage1_block0", "stage1", "down2", "stage2_block0", "stage2",
              "down3", "stage3_block0", "stage3"]:
        t = taps[k]
        v = t.view(copies, 8, *t.shape[1:])
        assert torch.equal(v, v[0:1].expand_as(v)), k
        assert torch.equal(v[0], taps8[k]), k
        if "sub_" + k in g.files:
            got = G.sub(taps8[k].permute(0, 3, 1, 2).contiguous())
            np.testing.assert_allclose(got, g["sub_" + k], rtol=0, atol=0.1 * ROUNDING[eng_bf16.test_prec], err_msg=k)
    assert torch.equal(fe.view(copies, 8, *fe.shape[1:]), fe8[None].expand(copies, *fe8.shape))
    assert torch.equal(clip.view(copies, 8, -1), clip8[None].expand(copies, *clip8.shape))
    np.testing.assert_allclose(fe8.cpu().numpy(), g["frame_embs"], atol=0.06 * ROUNDING[eng_bf16.test_prec])


@pytest.mark.parametrize("mode", ["step_fused", "step_unfused", "onepass"])
def test_teacher_forcing_against_bf16_operand_oracle(mode, eng_bf16, synth_weights):
    """cn_dec_block_kernel + cn_dec_ffn_kernel (step_fused), the one-launch-per-sub-layer step kernels (step_unfused) and the
    one-pass kernels (onepass) against the bf16-operand decoder oracle on the full (B, V, cap_len) logits of the ragged
    forcing fixture's inputs."""
    fused = mode == "step_fused"
    from oracle import bf16_ref as Bf
    g = np.load(os.path.join(G.GOLDEN, "forcing", "forcing_ragged.npz"))
    fe = torch.from_numpy(g["frame_embs"])
    shp = torch.from_numpy(g["audio_shape"])
    caps = torch.from_numpy(g["caps_in"]).long()
    k = ROUNDING[eng_bf16.test_prec]
    with Bf.operands(eng_bf16.test_prec):
        ref = Bf.teacher_forcing_bf16(synth_weights, fe, shp, caps).numpy()
    eng_bf16.set_decode_fusion(fused)
    eng_bf16.set_forcing_stepwise(mode != "onepass")
    try:
        got = eng_bf16.forcing(fe.cuda(), shp[:, 1].int(), caps).permute(0, 2, 1).cpu().numpy()
    finally:
        eng_bf16.set_decode_fusion(True)
        eng_bf16.set_forcing_stepwise(False)
    valid = (g["caps_in"] != 0)[:, None, :]                      # padded query positions carry no information
    err = np.abs(got - ref) * valid
    print("\nforcing", eng_bf16.test_prec, mode, "max", err.max(), "mean", err.mean(), "oracle vs fp32 reference", np.abs((ref - g["logits"]) * valid).max())
    np.testing.assert_allclose(got * valid, ref * valid, rtol=3e-3 * k, atol=0.15 * min(1.0, 2 * k))
    assert err.mean() < 0.03 * min(1.0, 2 * k)
    # and the oracle itself sits at bf16 (fp16) distance from the reference's fp32 logits
    assert np.abs((ref - g["logits"]) * valid).max() < 0.6 * k


@pytest.mark.parametrize("prec", ["bf16", "f16"])
@pytest.mark.parametrize("layer", range(6))
def test_decoder_layer_against_bf16_operand_oracle(layer, prec, synth_weights):
    """One decoder layer at a time (a 1-layer decoder built from layer `layer`'s weights): logits of the fused block / FFN
    kernels against the bf16-operand oracle.  Across 6 chained layers a value that rounds to the neighbouring bf16 in one
    layer is amplified by the next ones (the test above bounds that at 0.15 of a ~40-wide logit range); a single layer
    must agree to 2e-3 on average and to 0.1 in the worst element (one LayerNorm output that rounds to the neighbouring
    bf16 in front of the classifier moves a logit by 2^-8 |x_i| |Wc_vi|, up to ~0.06 with this checkpoint)."""
    from conette_amd.engine import Engine
    from oracle import bf16_ref as Bf
    sd = {}
    for k, v in synth_weights.items():
        if k.startswith("model.decoder.layers."):
            l = int(k.split(".")[3])
            if l == layer:
                sd["model.decoder.layers.0." + k.split(".", 4)[4]] = v
        else:
            sd[k] = v
    eng = Engine(sd, precision=prec, n_layers=1)
    k = ROUNDING[prec]
    g = np.load(os.path.join(G.GOLDEN, "forcing", "forcing_ragged.npz"))
    fe = torch.from_numpy(g["frame_embs"])
    shp = torch.from_numpy(g["audio_shape"])
    caps = torch.from_numpy(g["caps_in"]).long()
    with Bf.operands(prec):
        ref = Bf.teacher_forcing_bf16(sd, fe, shp, caps, n_layers=1).numpy()
    valid = (g["caps_in"] != 0)[:, None, :]
    for mode in ("step_fused", "step_unfused", "onepass"):
        eng.set_decode_fusion(mode == "step_fused")
        eng.set_forcing_stepwise(mode != "onepass")
        got = eng.forcing(fe.cuda(), shp[:, 1].int(), caps).permute(0, 2, 1).cpu().numpy()
        err = np.abs(got - ref) * valid
        print(f"\nlayer {layer} {prec} {mode}: max {err.max():.4f} mean {err.mean():.5f}")
        np.testing.assert_allclose(got * valid, ref * valid, rtol=3e-3 * k, atol=0.1 * k)
        assert err.mean() < 2e-3, err.mean()


def test_config1_single_5s_wav_greedy_clotho(tmp_path, synth_weights, synth_cfg):
    """BASELINE config 1 (the reference's CPU plumbing case, here on the GPU -- the product has no CPU path): one 5 s
    16-bit mono WAV -> CoNeTTEModel.from_pretrained(dir)(path, task="clotho", beam_size=1) vs the oracle on the same file."""
    import wave as wave_mod
    from conette_amd import CoNeTTEModel, synth
    from oracle import cpu_ref as O
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    d = synth.write_pretrained_dir(str(tmp_path / "ckpt"))
    wav = synth.synth_waveforms(1, 160000, 515)[0]
    pcm = np.clip(np.round(wav * 32768.0), -32768, 32767).astype("<i2")
    p = str(tmp_path / "five_seconds.wav")
    with wave_mod.open(p, "wb") as w:
        w.setnchannels(1), w.setsampwidth(2), w.setframerate(32000)
        w.writeframes(pcm.tobytes())
    tags = {i: f"tag{i}" for i in range(527)}
    with torch.no_grad():
        ref = O.model_forward(synth_weights, synth_cfg, p, task="clotho", beam_size=1)
    m32 = CoNeTTEModel.from_pretrained(d, precision="fp32", offline=True, audioset_idx_to_name=tags)
    out = m32(p, task="clotho", beam_size=1)
    assert out["preds"].cpu().tolist() == ref["preds"].tolist()
    assert out["cands"] == ref["cands"] and isinstance(out["cands"][0], str)
    np.testing.assert_allclose(out["lprobs"].cpu().numpy(), ref["lprobs"].numpy(), atol=2e-4)
    np.testing.assert_allclose(out["tags_probs"].cpu().numpy(), ref["tags_probs"].numpy(), rtol=1e-3, atol=1e-4)
    m16 = CoNeTTEModel.from_pretrained(d, precision="bf16", offline=True, audioset_idx_to_name=tags)
    o16 = m16(p, task="clotho", beam_size=1)
    assert abs(float(o16["lprobs"][0]) - float(ref["lprobs"][0])) < 0.15 and len(o16["cands"]) == 1


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_forbid_rep_mode_content_words(prec, tmp_path, synth_weights, synth_cfg, monkeypatch):
    """forbid_rep_mode="content_words" (pl_modules/common.py:239-276): the mask is rebuilt from the stop-word list at call
    time.  A stop-word set different from the one baked into the checkpoint's persisted mask, same set for the oracle."""
    from conette_amd import CoNeTTEModel, synth
    from oracle import cpu_ref as O
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    stop = [f"w{i}" for i in list(range(4, 40)) + list(range(300, 340))]
    monkeypatch.setattr(O, "SYNTH_STOPWORDS", stop)
    d = synth.write_pretrained_dir(str(tmp_path / "ckpt"))
    m = CoNeTTEModel.from_pretrained(d, precision=prec, offline=True, stopwords=stop,
                                     audioset_idx_to_name={i: f"tag{i}" for i in range(527)})
    wav = torch.from_numpy(synth.synth_waveforms(3, 96000, 4242, lengths=[96000, 64000, 80000]))
    x = [wav[i : i + 1, :n] for i, n in enumerate((96000, 64000, 80000))]
    with torch.no_grad():
        ref = O.model_forward(synth_weights, synth_cfg, x, sr=32000, task="clotho", forbid_rep_mode="content_words")
        ref_default = O.model_forward(synth_weights, synth_cfg, x, sr=32000, task="clotho")
    out = m(x, sr=32000, task="clotho", forbid_rep_mode="content_words")
    mask = m.get_forbid_rep_mask("content_words").cpu()
    assert int((~mask).sum()) == len(stop)
    if prec == "fp32":
        assert out["preds"].cpu().tolist() == ref["preds"].tolist()
        assert out["mult_preds"].cpu().tolist() == ref["mult_preds"].tolist()
        np.testing.assert_allclose(out["lprobs"].cpu().numpy(), ref["lprobs"].numpy(), atol=2e-4)
        assert ref["mult_preds"].tolist() != ref_default["mult_preds"].tolist()   # the mode changes the search
    else:
        assert np.all(np.abs(out["lprobs"].cpu().numpy() - ref["lprobs"].numpy()) < 0.3)
    # a repeated non-stop-word never appears in any hypothesis
    allowed = {i for i in range(4, 40)} | {i for i in range(300, 340)} | {0, 2}
    for hyp in out["mult_preds"].cpu().reshape(-1, out["mult_preds"].shape[-1]).tolist():
        seen = set()
        for t in hyp:
            assert t in allowed or t not in seen, hyp
            seen.add(t)


def test_f16_conversions_saturate_instead_of_overflowing(synth_weights):
    """CONETTE_PREC_F16: a hidden activation beyond the fp16 range (65504) must come out as 65504, not as inf -> NaN.  Block 4's
    pwconv1 weights and bias scaled until GELU outputs pass 1e5 (the fp32 mode's taps prove they do): the fp16 engine's frame
    embeddings stay finite and stay close to the bf16 engine's, whose operands have the fp32 range."""
    from conette_amd.engine import Engine
    from conette_amd import synth
    sd = dict(synth_weights)
    p = "preprocessor.encoder.stages.1.1."
    sd[p + "pwconv1.weight"] = synth_weights[p + "pwconv1.weight"] * 3.0e4
    sd[p + "pwconv1.bias"] = synth_weights[p + "pwconv1.bias"] * 3.0e4
    sd[p + "pwconv2.weight"] = synth_weights[p + "pwconv2.weight"] / 3.0e4   # (keeps the block's update O(1))
    wave = torch.from_numpy(synth.synth_waveforms(2, 64000, 77)).cuda()
    fe16, _ = Engine(sd, precision="f16").encode(wave)
    feb, _ = Engine(sd, precision="bf16").encode(wave)
    fe32, _ = Engine(sd, precision="fp32").encode(wave)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(fe16).all()) and bool(torch.isfinite(feb).all())
    # (measured: 2 % for fp16 -- clamped hidden values and the 3e-5-sized W2 operands, which are fp16 subnormals -- against 0.4 % for bf16)
    rel = float((fe16 - fe32).pow(2).mean().sqrt() / fe32.pow(2).mean().sqrt())
    relb = float((feb - fe32).pow(2).mean().sqrt() / fe32.pow(2).mean().sqrt())
    print("rel rms vs fp32: f16", rel, "bf16", relb)
    assert rel < 0.5 and relb < 0.05
