"""GPU: conette_tag_frames / conette_tag_events and Engine.tag_frames / tag_events (csrc/enc_tags.h; the rule: conette_amd/tagging.py).

1. FRAMES AGAINST THE RULE.  Every case and window of tests/tag_cases.py in the four precisions against the float64 rule, on the
   lines test_gpu_parity.py holds clip_probs to: rtol 1e-3, atol 1e-4 for fp32 / exact; atol 0.03 x R16 for bf16 / f16.
2. ANCHOR.  With a window over the whole clip every row is that encode's clip_probs, on the same lines.
3. BIT FOR BIT AGAINST ITSELF.  A clip alone = the clip in a batch; rows below the length do not see what lies beyond it; two calls,
   another stream; 0xFF-filled outputs are fully overwritten and rows beyond the length are exact zeros.
4. EVENTS, EXACT.  Every handcrafted sequence under every setting and length, tiled over 527 tags and 3 clips; the device's own
   frame_probs; n_tags 1, 63, 64, 65, 527.  No tolerance.
5. C ABI refusals name the argument and launch nothing."""
import ctypes as C

import numpy as np
import pytest
import torch

from conette_amd import tagging as R
from tests import tag_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
PRECISIONS = ("fp32", "exact", "bf16", "f16")
R16 = {"bf16": 1.0, "f16": 0.125}


@pytest.fixture(scope="module")
def lib():
    from conette_amd import engine
    return engine.load_library()


@pytest.fixture(scope="module")
def engines(synth_weights):
    from conette_amd.engine import Engine
    return {p: Engine(synth_weights, precision=p) for p in PRECISIONS}


@pytest.fixture(scope="module")
def reference(synth_weights_np):
    """the float64 rule over the whole table, computed once: {(case, window): (B, T, 527)}"""
    head = K.head(synth_weights_np)
    return {(name, w): R.frame_probs(fe, lens, *head, w) for name, fe, lens, windows in K.frame_cases() for w in windows}


def dev(a, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dt is None else t.to(dt)


def poison(shape, dt):
    return torch.full(shape, -1, dtype=torch.int32, device=DEV).view(dt)


def ptr(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def raw_frames(lib, eng, fe, lens, window, stream=None):
    """one raw conette_tag_frames call on a 0xFF-filled output and workspace; the (B, T, 527) result as numpy"""
    b, t, _ = fe.shape
    x, ln = dev(fe, torch.float32), dev(lens, torch.int32)
    out = poison((b, t, K.N_TAGS), torch.float32)
    need = int(lib.conette_tag_frames_workspace_bytes(eng._ctx, b, t))
    ws = torch.full((max(need, 1),), 255, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    s = torch.cuda.current_stream() if stream is None else stream
    st = lib.conette_tag_frames(eng._ctx, ptr(x), ptr(ln), b, t, int(window), ptr(out), ptr(ws), ws.numel(), C.c_void_p(s.cuda_stream))
    assert st == 0, lib.conette_last_error().decode()
    s.synchronize()
    return out.cpu().numpy()


def raw_events(lib, p, lens, setting, stream=None):
    """one raw conette_tag_events call on 0xFF-filled outputs; numpy results"""
    on, off, shortest, gap, m = setting
    b, t, c = p.shape
    x, ln = dev(p, torch.float32), dev(lens, torch.int32)
    out = {"spans": poison((b, c, m, 2), torch.int32), "peaks": poison((b, c, m), torch.float32),
           "peak_frames": poison((b, c, m), torch.int32), "counts": poison((b, c), torch.int32)}
    torch.cuda.synchronize()
    s = torch.cuda.current_stream() if stream is None else stream
    st = lib.conette_tag_events(ptr(x), ptr(ln), b, t, c, float(on), float(off), shortest, gap, m, ptr(out["spans"]), ptr(out["peaks"]),
                                ptr(out["peak_frames"]), ptr(out["counts"]), C.c_void_p(s.cuda_stream))
    assert st == 0, lib.conette_last_error().decode()
    s.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def bits(x):
    return np.ascontiguousarray(x).view(np.int32) if x.dtype == np.float32 else x


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def same_events(got, want):
    return all(same(got[k], want[k]) for k in ("spans", "peaks", "peak_frames", "counts"))


# ---- 1. frames against the rule -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECISIONS)
def test_frames_against_the_rule(prec, engines, reference):
    eng = engines[prec]
    rtol, atol = (1e-3, 1e-4) if prec not in R16 else (0.0, 0.03 * R16[prec])
    worst, n_calls = 0.0, 0
    for name, fe, lens, windows in K.frame_cases():
        x, ln = dev(fe), dev(lens)
        for w in windows:
            out = eng.tag_frames(x, ln, w)
            assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == fe.shape[:2] + (K.N_TAGS,)
            got, want = out.cpu().numpy().astype(np.float64), reference[name, w]
            for b, n in enumerate(lens):
                assert not got[b, n:].any(), (name, w, b)            # exact zeros, not sigmoid(bias)
            err = float(np.abs(got - want).max())
            worst, n_calls = max(worst, err), n_calls + 1
            print(prec, name, "window", w, "largest error", err)
            np.testing.assert_allclose(got, want, rtol=rtol, atol=atol, err_msg=f"{prec} {name} window {w}")
    print(prec, "largest error over", n_calls, "calls:", worst)
    assert n_calls == sum(len(c[3]) for c in K.frame_cases()) >= 40


# ---- 2. the anchor on the device ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECISIONS)
def test_window_over_the_clip_is_clip_probs(prec, engines):
    from conette_amd import synth
    eng = engines[prec]
    wave = torch.from_numpy(synth.synth_waveforms(3, 320000, 77)).to(DEV)
    fe, clip = eng.encode(wave)
    b, t = int(fe.shape[0]), int(fe.shape[1])
    assert (b, t) == (3, 31)
    out = eng.tag_frames(fe, torch.full((b,), t, dtype=torch.int32), 2 * t - 1)
    got, want = out.cpu().numpy(), np.broadcast_to(clip.cpu().numpy()[:, None, :], (b, t, K.N_TAGS))
    print(prec, "rows bit-equal to clip_probs:", bool(np.array_equal(bits(got), bits(np.ascontiguousarray(want)))),
          "largest difference", float(np.abs(got.astype(np.float64) - want).max()))
    rtol, atol = (1e-3, 1e-4) if prec not in R16 else (0.0, 0.03 * R16[prec])
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol)


# ---- 3. bit for bit against itself ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECISIONS)
def test_frames_bit_for_bit(prec, lib, engines):
    eng = engines[prec]
    side = torch.cuda.Stream()
    for name, windows in (("b4_odd_beam5_minpred0", (3, 4, 77)), ("gauss_T9_B3", (1, 7, 255)), ("gauss_T2_B3", (2,))):
        _, fe, lens, _ = next(c for c in K.frame_cases() if c[0] == name)
        for w in windows:
            whole = raw_frames(lib, eng, fe, lens, w)
            assert not (bits(whole) == -1).any(), (name, w)                  # every element written
            for b, n in enumerate(lens):
                assert (bits(whole[b, n:]) == 0).all() and (whole[b, :n] > 0).all() and np.isfinite(whole[b, :n]).all(), (name, w, b)
            assert same(whole, raw_frames(lib, eng, fe, lens, w)), (name, w)
            assert same(whole, raw_frames(lib, eng, fe, lens, w, stream=side)), (name, w)
            assert same(whole, eng.tag_frames(dev(fe), dev(lens), w).cpu().numpy()), (name, w)
            for fill in (1e30, np.nan):
                beyond = fe.copy()
                for b, n in enumerate(lens):
                    beyond[b, n:] = fill
                assert same(whole, raw_frames(lib, eng, beyond, lens, w)), (name, w, fill)
            for b, n in enumerate(lens):
                alone = raw_frames(lib, eng, fe[b:b + 1], lens[b:b + 1], w)
                assert same(alone, whole[b:b + 1]), (name, w, b)
                if n > 0:
                    cut = raw_frames(lib, eng, fe[b:b + 1, :n], lens[b:b + 1], w)
                    assert same(cut, whole[b:b + 1, :n]), (name, w, b)


# ---- 4. events, exact -----------------------------------------------------------------------------------------------------------------
def test_events_on_every_handcrafted_sequence(lib):
    p, which = K.tiled_events_input()
    assert p.shape[0] == 3 and p.shape[2] == K.N_TAGS
    n_calls = 0
    for n in K.EVENT_LENGTHS:
        for s in K.EVENT_SETTINGS:
            per_case = [R.events(K.padded(i), n, *s) for i in range(len(K.EVENT_CASES))]
            want = {k: np.stack([per_case[i][k] for i in which.ravel()]).reshape(which.shape + per_case[0][k].shape)
                    for k in ("spans", "peaks", "peak_frames")}
            want["counts"] = np.asarray([per_case[i]["count"] for i in which.ravel()], dtype=np.int32).reshape(which.shape)
            got = raw_events(lib, p, [n] * 3, s)
            assert got["peaks"].dtype == np.float32 and same_events(got, want), (n, s)
            n_calls += 1
    assert n_calls == len(K.EVENT_LENGTHS) * len(K.EVENT_SETTINGS)
    # every sequence at its own length under its own settings is among them
    for _, _, n, settings in K.EVENT_CASES:
        assert n in K.EVENT_LENGTHS and all(s in K.EVENT_SETTINGS for s in settings)


DEVICE_SETTINGS = ((0.3, 0.3, 1, 0, 16), (0.5, 0.3, 2, 1, 4), (0.3, 0.2, 1, 2, 1), (0.7, 0.7, 1, 0, 64))


def test_events_on_the_devices_own_frame_probs(lib, engines):
    eng = engines["fp32"]
    side = torch.cuda.Stream()
    busy = 0
    for name, w in (("b4_odd_beam5_minpred0", 3), ("gauss_T9_B3", 1), ("b1_30s_beam3", 7), ("gauss_T1_B1", 1)):
        _, fe, lens, _ = next(c for c in K.frame_cases() if c[0] == name)
        probs = eng.tag_frames(dev(fe), dev(lens), w)
        p = probs.cpu().numpy()
        for s in DEVICE_SETTINGS:
            want = R.events_batch(p, lens, *s)
            got = raw_events(lib, p, lens, s)
            assert same_events(got, want), (name, s)
            busy += int(want["counts"].sum())
            out = eng.tag_events(probs, dev(lens), *s)
            assert all(v.is_cuda for v in out.values()) and same_events({k: v.cpu().numpy() for k, v in out.items()}, want), (name, s)
            assert same_events(raw_events(lib, p, lens, s, stream=side), want), (name, s)
        b, c = 0, int(np.argmax(p[0].max(axis=0)))          # one sequence through the sequence form of the rule
        one = R.events(np.ascontiguousarray(p[b, :, c]), lens[b], *DEVICE_SETTINGS[1])
        got = raw_events(lib, p, lens, DEVICE_SETTINGS[1])
        assert same(got["spans"][b, c], one["spans"]) and same(got["peaks"][b, c], one["peaks"]) and got["counts"][b, c] == one["count"]
    assert busy > 1000        # (the synthetic head does give events to find)


@pytest.mark.parametrize("n_tags", (1, 63, 64, 65, 527))
def test_events_at_any_number_of_tags(lib, n_tags):
    p, _ = K.tiled_events_input()
    p = np.ascontiguousarray(p[:, :, :n_tags])
    for lens, s in (([10, 4, 0], (K.ON, K.OFF, 1, 1, 4)), ([7, 10, 3], (K.ON, K.ON, 1, 0, 1)), ([9, 5, 10], (K.ON, K.ON, 2, 2, 64))):
        assert same_events(raw_events(lib, p, lens, s), R.events_batch(p, lens, *s)), (n_tags, lens, s)


def test_off_none_is_plain_thresholding(engines):
    p, _ = K.tiled_events_input()
    eng = engines["bf16"]
    lens = dev(np.asarray([10, 10, 10], dtype=np.int32))
    a = eng.tag_events(dev(p), lens, 0.5)
    b = eng.tag_events(dev(p), lens, 0.5, 0.5, 1, 0, 16)
    assert all(torch.equal(a[k], b[k]) for k in a) and tuple(a["spans"].shape) == (3, K.N_TAGS, 16, 2)
    for kw, word in ((dict(on=1.5), "on"), (dict(on=0.5, off=0.6), "off"), (dict(on=0.5, max_events=65), "max_events"),
                     (dict(on=0.5, max_gap=-1), "max_gap")):
        with pytest.raises(ValueError, match=word):
            eng.tag_events(dev(p), lens, **kw)
    with pytest.raises(ValueError, match="window"):
        eng.tag_frames(torch.zeros((1, 2, 768), device=DEV), torch.ones(1, dtype=torch.int32), 256)
    with pytest.raises(ValueError, match="frame_lens"):
        eng.tag_frames(torch.zeros((2, 2, 768), device=DEV), torch.ones(1, dtype=torch.int32), 3)


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------
def test_c_abi_errors(lib, engines, synth_weights):
    from conette_amd.engine import Engine
    eng = engines["bf16"]
    b, t, m = 2, 5, 4
    fe = torch.zeros((b, t, 768), dtype=torch.float32, device=DEV)
    lens = torch.full((b,), t, dtype=torch.int32, device=DEV)
    probs = poison((b, t, K.N_TAGS), torch.float32)
    need = int(lib.conette_tag_frames_workspace_bytes(eng._ctx, b, t))
    assert need >= b * t * 768 * 2
    ws = torch.full((need,), 255, dtype=torch.uint8, device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = dict(ctx=eng._ctx.value, frame_embs=fe.data_ptr(), frame_lens=lens.data_ptr(), batch=b, t_audio=t, window=3,
                frame_probs=probs.data_ptr(), workspace=ws.data_ptr(), workspace_bytes=need)
    pointers = ("ctx", "frame_embs", "frame_lens", "frame_probs", "workspace")

    def frames(a):
        return lib.conette_tag_frames(*[C.c_void_p(v) if k in pointers else v for k, v in a.items()], stream)

    decoder_only = Engine({k: v for k, v in synth_weights.items() if k.startswith("model.")}, precision="bf16")
    bad = [("ctx", 0, "ctx"), ("frame_embs", 0, "frame_embs"), ("frame_lens", 0, "frame_lens"), ("frame_probs", 0, "frame_probs"),
           ("workspace", 0, "workspace"), ("batch", -1, "batch"), ("t_audio", -1, "t_audio"), ("window", 0, "window"),
           ("window", 256, "window"), ("window", -3, "window"), ("workspace_bytes", need - 1, "workspace"),
           ("ctx", decoder_only._ctx.value, "decoder-only")]
    for key, value, word in bad:
        st = frames({**good, key: value})
        msg = lib.conette_last_error().decode()
        assert st != 0 and "tag_frames" in msg and word in msg, (key, value, st, msg)
        assert (st == 4) == (key == "workspace_bytes"), (key, st)         # CN_ERR_WORKSPACE for the short workspace alone
    torch.cuda.synchronize()
    assert bool((probs.view(torch.int32) == -1).all()) and bool((ws == 255).all())       # nothing was launched
    assert frames(good) == 0, lib.conette_last_error()
    torch.cuda.synchronize()
    assert not bool((probs.view(torch.int32) == -1).any())

    p = torch.rand((b, t, K.N_TAGS), dtype=torch.float32, device=DEV)
    out = [poison((b, K.N_TAGS, m, 2), torch.int32), poison((b, K.N_TAGS, m), torch.float32), poison((b, K.N_TAGS, m), torch.int32),
           poison((b, K.N_TAGS), torch.int32)]
    good = dict(frame_probs=p.data_ptr(), frame_lens=lens.data_ptr(), batch=b, t_audio=t, n_tags=K.N_TAGS, on_threshold=0.5,
                off_threshold=0.3, min_frames=1, max_gap=0, max_events=m, spans=out[0].data_ptr(), peaks=out[1].data_ptr(),
                peak_frames=out[2].data_ptr(), counts=out[3].data_ptr())
    pointers = ("frame_probs", "frame_lens", "spans", "peaks", "peak_frames", "counts")

    def events(a):
        return lib.conette_tag_events(*[C.c_void_p(v) if k in pointers else v for k, v in a.items()], stream)

    nan, inf = float("nan"), float("inf")
    bad = [(k, 0) for k in pointers] + [("batch", -1), ("t_audio", -1), ("n_tags", -1), ("on_threshold", 0.0), ("on_threshold", 1.5),
                                        ("on_threshold", nan), ("on_threshold", inf), ("on_threshold", -0.5), ("off_threshold", 0.0),
                                        ("off_threshold", 0.6), ("off_threshold", nan), ("off_threshold", -inf), ("min_frames", -1),
                                        ("max_gap", -1), ("max_events", 0), ("max_events", 65)]
    for key, value in bad:
        st = events({**good, key: value})
        msg = lib.conette_last_error().decode()
        assert st == 1 and "tag_events" in msg and key in msg, (key, value, st, msg)
    torch.cuda.synchronize()
    for o in out:
        assert bool((o.view(torch.int32) == -1).all())
    assert events(good) == 0, lib.conette_last_error()
    torch.cuda.synchronize()
    for o in out:
        assert not bool((o.view(torch.int32) == -1).all())
