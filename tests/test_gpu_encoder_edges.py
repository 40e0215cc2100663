"""GPU: the encoder's kernels at every tile tail, clip seam and launch grid of the case table in tests/encoder_geometry.py.

(a) Every block / downsample (and the stem) of every case against the oracles, on the GPU's own input of that layer:
    * bf16 / f16: the operand oracle (oracle/bf16_ref.py) with the rule of tests/block_oracle.py on the whole tensor AND on each
      tail region alone (there its 1e-5 share rounded up to whole values) (the 3 halo rows at both ends of every clip, the last partial depthwise tile, the last 32-position tile of
      the fused MLP), and the unmodified fp32 oracle with FP32_BOUND.
    * fp32 / exact: oracle/cpu_ref.py's fp32 block, every element within 5e-5 + 5e-5 |ref| and the mean error below 1e-6.  The
      bound is derived, not measured: operands of 22 bits (fp16 hi / lo pairs) are 2^-22 relative, with an absolute floor of
      2^-25 where lo is an fp16 subnormal (common.h); the accumulation is fp32 over K <= 3072 with O(1) activations: ~1e-5.
      Measured worst over all cases (MI355X): fp32 max 1.14e-5 / mean 5.3e-7, exact max 9.5e-6 / mean 6.6e-7, both at down3 of
      the large cases (a whole LayerNorm + K = 1536 GEMM, not a residual update; blocks stay below 8e-6 / 4.5e-7).
    The large cases check only stages 2-3 (blocks 6-17, down2, down3): the small cases cover stages 0-1.
(b) Batch invariance with distinct clips: every tap, frame_embs row and clip_probs row of clip i equals, bit for bit, the same
    clip's output from a sub-batch at the same padded length (1 clip for the small cases, chunks of 8 for the large ones).
(c) Launch-grid invariance: set_encode_reserved_cus(r) for r in (0, 24, n_cu // 2) changes no bit of any tap; the bf16 oracle
    check of the benchmark's batch runs at r = 24, the benchmark's setting.
(d) Stale memory: an encode's results and its overflow watch do not depend on what its workspace and outputs held before
    (all bytes 0xFF -- NaN in fp32, fp16 and bf16 -- against all bytes 0x00)."""
import math
import os

import pytest
import torch
from torch.nn import functional as F

from tests import encoder_geometry as E
from tests.block_oracle import FP32_BOUND, ROUNDING, _assert_close, _nchw

pytestmark = pytest.mark.gpu

SMALL_IDS = [c.name for c in E.small_cases()]
LARGE_IDS = ["L128", "L256", "Lbench"]
PRECS = ["bf16", "f16", "fp32", "exact"]
F32_ATOL, F32_RTOL, F32_MEAN = 5e-5, 5e-5, 1e-6
# FP32_BOUND was measured on block outputs, a residual plus a small update.  A downsample's output is a whole LayerNorm + patch GEMM
# on 16-bit operands: measured against the fp32 oracle at every case here, bf16 max 0.0128 / mean 1.92e-3 (f16 stays inside
# FP32_BOUND); this bound leaves a factor ~2.
DOWN_FP32_BOUND = {"bf16": (0.025, 3.8e-3), "f16": FP32_BOUND["f16"]}


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _case(cid):
    if cid.startswith("L"):
        tag = cid[1:]
        return next(c for c in E.large_cases(_n_cu()) if c.name.startswith(f"L{tag}_"))
    return next(c for c in E.small_cases() if c.name == cid)


_WAVES = {}


def _wave(c):
    from conette_amd import synth
    if c.name not in _WAVES:
        _WAVES.clear()
        _WAVES[c.name] = torch.from_numpy(synth.synth_waveforms(c.b, c.n_samples, c.seed0, lengths=list(c.lengths))).cuda()
    return _WAVES[c.name]


@pytest.fixture(scope="module")
def engines(synth_weights):
    from conette_amd.engine import Engine
    made = {}

    def get(prec):
        if prec not in made:
            made[prec] = Engine(synth_weights, precision=prec)
        return made[prec]
    yield get
    made.clear()


def _stem_fp32(w, logmel):
    d = "preprocessor.encoder.downsample_layers.0."
    from oracle import cpu_ref as O
    x = F.conv2d(logmel[:, None], w[d + "0.weight"], w[d + "0.bias"], stride=(4, 4), padding=(4, 0))
    return O._ln_cf(x, w[d + "1.weight"], w[d + "1.bias"])


def _down_fp32(w, i, x):
    from oracle import cpu_ref as O
    d = f"preprocessor.encoder.downsample_layers.{i}."
    return F.conv2d(O._ln_cf(x, w[d + "0.weight"], w[d + "0.bias"]), w[d + "1.weight"], w[d + "1.bias"], stride=2)


def _tail_mask(prec, st, b, h, w, kind):
    """(B, H, W) bool: the tail regions of a layer at stage st (kind "block": halo rows of every clip, the last partial
    depthwise tile, the last fused-MLP tile; "down" / "stem": the last 32 positions)."""
    m = torch.zeros(b, h, w, dtype=torch.bool)
    if kind == "block":
        m[:, :E.HALO] = True
        m[:, max(0, h - E.HALO):] = True
        rows = E.dw_tail_rows(E.STREAM[prec], st, h)
        if len(rows):
            m[:, rows.start:rows.stop] = True
    if kind != "block" or st in E.FUSED_MLP_STAGES[prec]:
        tail = E.mlp_tail_positions(b * h * w)
        m.view(-1)[tail.start:tail.stop] = True
    return m


def _assert_close_counted(got, ref, what, k):
    """_assert_close's rule on a tail region, or on a tensor too small for its 1e-5 share to admit one value (a one-clip stage-2
    block): the share is rounded UP to whole values -- a value that rounds to the neighbouring operand is as likely in a tail as
    anywhere else (measured: at most 2 in a tail region of 177 408 values, f16) -- with the same 4x and mean bounds."""
    err = (got - ref).abs()
    bound = k * (2e-3 + 3e-3 * ref.abs()) + 2.0 ** -10 * ref.abs()
    n_out = int((err > bound).sum())
    assert n_out <= math.ceil(1e-5 * err.numel()), (what, n_out, float(err.max()))
    assert bool((err <= 4 * bound).all()), (what, float(err.max()))
    assert float(err.mean()) < k * 1.5e-4 + (2e-5 if k < 1 else 0.0), (what, float(err.mean()))


def _check16(got, ref, ref32, what, prec, mask, bound32):
    k = ROUNDING[prec]
    (_assert_close if got.numel() >= 1e5 else _assert_close_counted)(got, ref, what, k)
    sel = lambda t: t.permute(0, 2, 3, 1)[mask]
    _assert_close_counted(sel(got), sel(ref), what + " [tails]", k)
    err32 = (got - ref32).abs()
    assert float(err32.max()) < bound32[prec][0] and float(err32.mean()) < bound32[prec][1], \
        (what, "fp32 oracle", float(err32.max()), float(err32.mean()))
    err = (got - ref).abs()
    return float(err.max()), float(err.mean())


def _check32(got, ref, what, mask):
    err = (got - ref).abs()
    bad = err > F32_ATOL + F32_RTOL * ref.abs()
    assert not bool(bad.any()), (what, int(bad.sum()), float(err.max()))
    assert float(err.mean()) <= F32_MEAN, (what, float(err.mean()))
    tail = err.permute(0, 2, 3, 1)[mask]
    assert float(tail.mean()) <= F32_MEAN, (what + " [tails]", float(tail.mean()))
    return float(err.max()), float(err.mean())


def _against_oracles(eng, prec, c, w, reserved=0):
    """Part (a) for one engine and case; returns {layer: (max, mean)} against the operand oracle (16-bit) / fp32 oracle."""
    from oracle import bf16_ref as Bf
    from oracle import cpu_ref as O
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    eng.set_encode_reserved_cus(reserved)
    try:
        fe, clip, taps = eng.encode(_wave(c), taps="blocks")
        torch.cuda.synchronize()
    finally:
        eng.set_encode_reserved_cus(0)
    _, hs, ws = E.geometry(c.n_samples)
    first = 2 if c.large else 0
    sixteen = prec in ("bf16", "f16")
    worst = {}

    def check(name, st, kind, got, ref32, ref16_fn):
        mask = _tail_mask(prec, st, c.b, hs[st], ws[st], kind)
        what = f"{c.name}/{prec}/{name}"
        if sixteen:
            with Bf.operands(prec):
                ref = ref16_fn()
            worst[name] = _check16(got, ref, ref32, what, prec, mask, DOWN_FP32_BOUND if kind == "down" else FP32_BOUND)
        else:
            worst[name] = _check32(got, ref32, what, mask)

    with torch.no_grad():
        if first == 0:
            got = _nchw(taps["stem"])
            ref32 = _stem_fp32(w, taps["logmel"].cpu())
            check("stem", 0, "stem", got, ref32, lambda: Bf.res16(ref32))
        blk = 0
        for st, depth in enumerate(E.DEPTHS):
            if st >= first and st > 0:
                src = _nchw(taps[f"stage{st - 1}"])
                ref32 = _down_fp32(w, st, src)
                check(f"down{st}", st, "down", _nchw(taps[f"down{st}"]), ref32,
                      lambda: Bf.downsample_bf16(w, st, src, folded=st <= 2))
            for b in range(depth):
                if st >= first:
                    src = _nchw(taps["stem"] if blk == 0 else (taps[f"down{st}"] if b == 0 else taps[f"block{blk - 1}"]))
                    prefix = Bf.block_prefix(blk)
                    ref32 = O.convnext_block(w, prefix, src)
                    check(f"block{blk}", st, "block", _nchw(taps[f"block{blk}"]), ref32,
                          lambda: Bf.convnext_block_bf16(w, prefix, src, folded=st < 3))
                blk += 1
    return worst


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("cid", SMALL_IDS + LARGE_IDS)
def test_every_layer_against_the_oracles(cid, prec, engines, synth_weights):
    c = _case(cid)
    # the benchmark's batch in bf16 runs at the benchmark's launch grid (24 CUs left to the decode stream)
    reserved = E.BENCH_RESERVED_CUS if (cid == "Lbench" and prec == "bf16") else 0
    worst = _against_oracles(engines(prec), prec, c, synth_weights, reserved)
    top = max(worst.items(), key=lambda kv: kv[1][0])
    print(f"\n{c.name} {prec} (r = {reserved}): worst max {top[1][0]:.3g} at {top[0]}, worst mean "
          f"{max(v[1] for v in worst.values()):.3g} | " + " ".join(f"{k}:{v[0]:.2g}/{v[1]:.2g}" for k, v in worst.items()))


def _encode_all(eng, wave, exact=False):
    fe, clip, taps = eng.encode(wave, taps="blocks", exact=exact)
    return fe, clip, taps


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("cid", ["s15040x5", "s36800x5", "s62400x5", "s71360x5"] + LARGE_IDS)
def test_batch_invariance_with_distinct_clips(cid, prec, engines):
    """Clip i of a batch of distinct clips equals, bit for bit, the same clip encoded in a sub-batch at the same padded length:
    a tile that reads rows of another clip, or a k order that depends on the batch, shows here (copies of one batch cannot
    show a wrong-clip read whose offset is a multiple of the copy).  Small cases: one clip at a time; large: chunks of 8."""
    c = _case(cid)
    eng = engines(prec)
    wave = _wave(c)
    fe, clip, taps = _encode_all(eng, wave)
    chunk = 8 if c.large else 1
    for i0 in range(0, c.b, chunk):
        i1 = min(c.b, i0 + chunk)
        fe_s, clip_s, taps_s = _encode_all(eng, wave[i0:i1].contiguous())
        torch.cuda.synchronize()
        for k, t in taps_s.items():
            assert torch.equal(taps[k][i0:i1], t), (c.name, prec, k, i0)
        assert torch.equal(fe[i0:i1], fe_s), (c.name, prec, "frame_embs", i0)
        assert torch.equal(clip[i0:i1], clip_s), (c.name, prec, "clip_probs", i0)


@pytest.mark.parametrize("prec", ["bf16", "f16", "exact"])
@pytest.mark.parametrize("cid", ["s26560x5", "Lbench"])
def test_launch_grid_invariance(cid, prec, engines):
    """set_encode_reserved_cus shrinks the grid of every persistent encoder kernel (fused MLPs, mlp_sp, fused downsample), so each
    block walks more tiles and rounds: no bit of any tap may move."""
    c = _case(cid)
    eng = engines(prec)
    wave = _wave(c)
    ref = None
    try:
        for r in (0, E.BENCH_RESERVED_CUS, _n_cu() // 2):
            eng.set_encode_reserved_cus(r)
            fe, clip, taps = _encode_all(eng, wave)
            torch.cuda.synchronize()
            if ref is None:
                ref = (fe, clip, taps)
                continue
            for k, t in taps.items():
                assert torch.equal(ref[2][k], t), (c.name, prec, r, k)
            assert torch.equal(ref[0], fe) and torch.equal(ref[1], clip), (c.name, prec, r)
    finally:
        eng.set_encode_reserved_cus(0)


@pytest.mark.parametrize("prec", ["bf16", "f16", "fp32", "exact", "certified:exact-context"])
@pytest.mark.parametrize("cid", ["s15040x5", "L128"])
def test_stale_workspace_and_outputs(cid, prec, synth_weights):
    """encode only: enc_ws (encoder.hip) holds floating-point activations alone, so a stale value can flow into arithmetic but
    never into an address.  The fused MLP reads rows past the last position by design, and after an fp16-stream overflow inf /
    NaN stays in the cached workspace: neither may reach a result or the overflow watch."""
    from conette_amd.engine import FEAT, N_TAGS, Engine
    c = _case(cid)
    exact = prec.startswith("certified")
    eng = Engine(synth_weights, precision="certified" if exact else prec)
    wave = _wave(c)
    _, hs, _ = E.geometry(c.n_samples)
    fill = {"v": 0}
    orig = eng._workspace

    def poisoned(key, nbytes):
        ws = orig(key, nbytes)
        ws.fill_(fill["v"])
        return ws

    eng._workspace = poisoned
    runs = []
    try:
        eng.encode_nonfinite()   # (process-wide counter: start from zero)
        for v in (0xFF, 0x00):
            fill["v"] = v
            fe = torch.empty((c.b, hs[3], FEAT), dtype=torch.float32, device="cuda")
            clip = torch.empty((c.b, N_TAGS), dtype=torch.float32, device="cuda")
            fe.view(torch.uint8).fill_(v)
            clip.view(torch.uint8).fill_(v)
            out = eng.encode(wave, taps="blocks", out=(fe, clip), exact=exact)
            torch.cuda.synchronize()
            assert out[0] is fe and out[1] is clip
            assert eng.encode_nonfinite() == 0, (c.name, prec, hex(v))
            for k, t in [("frame_embs", fe), ("clip_probs", clip)] + list(out[2].items()):
                assert bool(torch.isfinite(t).all()), (c.name, prec, hex(v), k)
            runs.append(out)
    finally:
        eng._workspace = orig
    a, b = runs
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (c.name, prec)
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), (c.name, prec, k)
