"""GPU: the audio front end (cn_logmel_kernel, csrc/frontend.hip) and the sinc resampler (csrc/api.hip) against float64, at every
frame class of the case table in tests/frontend_geometry.py and on seven checkpoints (stock, three that select the raw power
spectrum of bins 0-223 / 224-447 / 448-512, three with ragged mel bands of at most 49 / 50 / 513 rows -- the last with an
asymmetric window and the mel matrix in global memory).

(a) Accuracy: every case x every engine against ref64 with the power-domain interval rule at C_GPU = 4 C_fft, every element.
(b) Spectrum reassembly: the select engines' outputs side by side are the dB power spectrum of all 513 bins; the bins above 448
    and bin 512 on the 15.5 kHz / 15.99 kHz tones and on the impulse (w[n0]^2 at every bin).
(c) Bit invariances: batch against single clip, the one-float-offset view against the aligned run, stale output memory, the
    encoder's logmel tap, and the grid-stride trip against two smaller batches.
(d) A NaN or +inf sample makes every mel bin of every frame that holds it NaN and moves no bit of any other frame.
(e) L = 512 is refused, L = 513 runs.
(f) The resampler at 12 rates and every length edge against float64 accumulation over the fp32-built torchaudio table.

The C the kernel itself needed (MI355X, for information; the bound does not come from it) is in profiles/frontend_edges_notes.md."""
import numpy as np
import pytest
import torch

from tests import frontend_geometry as G

pytestmark = pytest.mark.gpu

ENGINES = list(G.CHECKPOINTS)


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def engines(synth_weights_np):
    from conette_amd.engine import Engine
    from oracle import cpu_ref
    made = {}

    def get(name):
        if name not in made:
            sd = G.checkpoint(name, synth_weights_np)
            made[name] = (Engine(cpu_ref.to_torch(sd), precision="fp32"), G.front_tensors(sd))
        return made[name]
    yield get
    made.clear()


_WAVES, _SPECTRA = {}, {}


def _wave(c):
    if c.name not in _WAVES:
        _WAVES.clear()
        _SPECTRA.clear()
        _WAVES[c.name] = G.make_wave(c)
    return _WAVES[c.name]


def _spectrum(c, window):
    """(z, X) of the case in float64 for a window; computed once per case and window."""
    wave = _wave(c)
    key = (c.name, window.tobytes())
    if key not in _SPECTRA:
        z, X, _, _ = G.ref64(wave, window, np.zeros((G.N_BINS, 1)))
        _SPECTRA[key] = (z, X)
    return _SPECTRA[key]


def _device_view(wave_np, offset):
    """The batch on the device: offset 1 is a contiguous view one float into a larger buffer (its rows are 4 mod 8 bytes)."""
    b, n = wave_np.shape
    buf = torch.empty(b * n + 2, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 8 == 0
    view = buf[offset:offset + b * n].view(b, n)
    view.copy_(torch.from_numpy(wave_np))
    assert view.is_contiguous() and view.data_ptr() % 8 == 4 * offset
    return view


def _run(eng, wave_np, offset=0):
    out = eng.frontend_logmel(_device_view(wave_np, offset))
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ---- (a) -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ENGINES)
@pytest.mark.parametrize("cid", G.CASE_NAMES)
def test_every_case_against_float64(cid, name, engines):
    c = G.case(cid, _n_cu())
    eng, (window, melw, bn) = engines(name)
    got = _run(eng, _wave(c), c.offset)
    assert got.shape == (c.b, G.n_frames(c.n_samples), G.N_MELS)
    z, X = _spectrum(c, window)
    ref = G.make_ref(z, X, melw, bn)
    need = G.required_C(got, ref)
    print(f"\n{c.name} ({c.b} x {c.n_samples}, {c.kind}, offset {c.offset}) on {name}: needs C = {need:.2f} of {G.C_GPU}")
    bad = G.violations(got, ref, G.C_GPU)
    assert not bad.any(), (c.name, name, int(bad.sum()), need, np.argwhere(bad)[:5].tolist())
    dead = np.abs(melw).sum(0) == 0
    assert int(dead.sum()) == (G.N_MELS - 65 if name == "select2" else 0)
    if dead.any():
        # all-zero columns read the clamp's floor, -100 dB (times the fp32 identity scale: within 2 ulp of 100)
        assert np.abs(got[..., dead].astype(np.float64) + 100.0).max() <= 2.0 * 2.0 ** -17


# ---- (b) -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["hi_tones", "hi_15500", "imp_17", "t16_edge"])
def test_select_engines_reassemble_the_spectrum(cid, engines):
    c = G.case(cid, _n_cu())
    wave = _wave(c)
    parts = [_run(engines(f"select{j}")[0], wave, c.offset) for j in range(3)]
    spec = np.concatenate(parts, axis=-1)[..., :G.N_BINS]
    _, (window, _, bn) = engines("select0")
    z, X = _spectrum(c, window)
    ref = G.spectrum_ref(z, X, bn)
    bad = G.violations(spec, ref, G.C_GPU)
    assert not bad[..., 449:].any(), (cid, "bins above 448", np.argwhere(bad[..., 449:])[:5].tolist())
    assert not bad[..., 512].any() and not bad.any(), (cid, int(bad.sum()))
    src = G.frame_sources(c.n_samples)
    if c.kind in ("t15500", "t15990"):
        # the peak of every frame that lies inside a full-length clip sits where the tone is: bin 496, or 511 / 512 (15.99 kHz is
        # bin 511.7; at the Nyquist bin the tone and its image add by phase), the same bin as in float64
        peaks = {"t15500": (496,), "t15990": (511, 512)}[c.kind]
        inside = [f for f in range(src.shape[0]) if G.frame_class(c.n_samples, f) == "inside"]
        for i in range(c.b):
            if c.lengths[i] == c.n_samples:
                peak = spec[i, inside].argmax(-1)
                assert np.isin(peak, peaks).all() and np.array_equal(peak, ref.M[i, inside].argmax(-1)), (cid, i)
                assert (spec[i, inside].max(-1) > spec[i, inside, 440] + 40.0).all()     # 40 dB above the stock matrix's last bins
    if c.kind == "impulse":
        # a frame that holds the impulse once, at window position n0, has the power w[n0]^2 at EVERY bin; by the rule
        # (||z|| = |X[k]| = w[n0]) that is 10 log10((1 + C eps)^2 + 8 eps) dB plus the rounding of log10f at |dB| <= 32
        at = min(G.IMPULSE_AT, c.n_samples - 1)
        bound = 10.0 * np.log10((1.0 + G.C_GPU * G.EPS) ** 2 + 8.0 * G.EPS) + 6.0 * 2.0 ** -19
        seen = 0
        for f in range(src.shape[0]):
            pos = np.nonzero(src[f] == at)[0]
            if len(pos) == 1 and window[pos[0]] > 0.03:
                want = 20.0 * np.log10(float(window[pos[0]]))
                assert np.abs(spec[0, f].astype(np.float64) - want).max() <= bound, (cid, f, int(pos[0]))
                seen += 1
        assert seen >= 3


# ---- (c) -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["stock", "ragged50"])
@pytest.mark.parametrize("cid", ["t15_odd", "edge_m1", "four_kinds", "four_off1", "big_p17"])
def test_clip_of_a_batch_equals_the_clip_alone(cid, name, engines):
    c = G.case(cid, _n_cu())
    eng = engines(name)[0]
    wave = _wave(c)
    full = _run(eng, wave, c.offset)
    picks = range(c.b) if c.b <= 4 else (0, 1, c.b // 2, c.b - 2, c.b - 1)
    for i in picks:
        assert np.array_equal(full[i], _run(eng, wave[i:i + 1], c.offset)[0]), (cid, name, i)


@pytest.mark.parametrize("name", ["stock", "select2", "ragged513"])
@pytest.mark.parametrize("cid", ["edge_off1", "four_off1", "t16_edge", "big_p17"])
def test_offset_view_equals_the_aligned_run(cid, name, engines):
    """An even-L batch whose base is 4 mod 8 bytes takes the scalar loads with reflect arithmetic for every frame; the aligned run
    takes the 8-byte loads for the frames inside the clip.  Same products, same order: no bit may differ."""
    c = G.case(cid, _n_cu())
    assert c.n_samples % 2 == 0
    eng = engines(name)[0]
    wave = _wave(c)
    assert np.array_equal(_run(eng, wave, 0), _run(eng, wave, 1)), (cid, name)


@pytest.mark.parametrize("name", ["stock", "select2", "ragged50"])
@pytest.mark.parametrize("cid", ["t15_odd", "t17", "big_p1"])
def test_stale_output_memory(cid, name, engines):
    from conette_amd.engine import _check, _ptr, _stream
    c = G.case(cid, _n_cu())
    eng = engines(name)[0]
    dev = _device_view(_wave(c), c.offset)
    runs = []
    for fill in (0xFF, 0x00):
        out = torch.empty((c.b, G.n_frames(c.n_samples), G.N_MELS), dtype=torch.float32, device="cuda")
        out.view(torch.uint8).fill_(fill)
        _check(eng.lib.conette_frontend_logmel(eng._ctx, _ptr(dev), c.b, c.n_samples, _ptr(out), _stream()), "frontend_logmel")
        torch.cuda.synchronize()
        runs.append(out.cpu())
    assert not bool(torch.isnan(runs[0]).any()) and torch.equal(runs[0], runs[1]), (cid, name)


@pytest.mark.parametrize("n", [8001, 9600])
def test_encoder_tap_equals_frontend_logmel(n, engines):
    eng = engines("stock")[0]
    c = G.Case("tap", 3, n, (n, n // 3, n - 7), "noise", 0, 777)
    dev = _device_view(G.make_wave(c), 0)
    taps = eng.encode(dev, taps=True)[2]
    alone = eng.frontend_logmel(dev)
    torch.cuda.synchronize()
    assert torch.equal(taps["logmel"], alone)


@pytest.mark.parametrize("name", ["stock", "select1", "ragged513"])
def test_second_trip_equals_two_smaller_batches(name, engines):
    """n_cu * 16 + 17 frames: every block's first trip and two blocks' second trip (the last one partial) against the same clips
    run as two batches that fit in one trip each."""
    n_cu = _n_cu()
    c = G.case("big_p17", n_cu)
    assert G.launch(c.total, n_cu)[1] == 2 and c.total % G.FE_NW == 1
    eng = engines(name)[0]
    wave = _wave(c)
    full = _run(eng, wave)
    h = c.b // 2 + 1
    assert all(G.launch(k * G.n_frames(c.n_samples), n_cu)[1] == 1 for k in (h, c.b - h))
    two = np.concatenate([_run(eng, wave[:h]), _run(eng, wave[h:])], axis=0)
    assert np.array_equal(full, two)


# ---- (d) -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["stock", "ragged513"])
@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("at", [100, 3001, 6399])
def test_non_finite_sample(at, bad, name, engines):
    """Every mel bin of every frame whose window (after reflection) holds the sample is NaN; every other frame, of either clip, is
    bit-equal to the run with that sample set to 0.  (at = 100 is reflected into frame 0 twice, 6399 is the last sample.)"""
    eng = engines(name)[0]
    c = G.Case("nonfinite", 2, 6400, (6400, 6400), "noise", 0, 4100)
    clean = G.make_wave(c)
    clean[1, at] = 0.0
    dirty = clean.copy()
    dirty[1, at] = bad
    ref = _run(eng, clean)
    got = _run(eng, dirty)
    holds = (G.frame_sources(c.n_samples) == at).any(-1)
    assert 2 <= int(holds.sum()) <= 4
    assert np.array_equal(got[0], ref[0])
    assert np.isnan(got[1, holds]).all(), (name, at, bad, int(np.isnan(got[1, holds]).sum()), got[1, holds].size)
    assert np.array_equal(got[1, ~holds], ref[1, ~holds])
    assert np.isfinite(ref).all()


# ---- (e) -----------------------------------------------------------------------------------------------------------------------------
def test_shortest_clip(engines):
    eng = engines("stock")[0]
    x = torch.zeros((2, 512), dtype=torch.float32, device="cuda")
    with pytest.raises(RuntimeError, match="must exceed 512"):
        eng.frontend_logmel(x)
    out = eng.frontend_logmel(torch.zeros((2, 513), dtype=torch.float32, device="cuda"))
    torch.cuda.synchronize()
    assert out.shape == (2, 2, G.N_MELS) and bool(torch.isfinite(out).all())


# ---- (f) -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", G.RATES)
def test_resampler_against_float64(rate, engines):
    """tol_i = 2^-21 ||x_win,i||_2 + 8 2^-24 sum_t |k_t x_t| against float64 accumulation over the table torchaudio 0.13.1 builds
    in fp32.  Outputs only: at 52 800 Hz the library's table is one tap wider on both sides, where the window is zero."""
    eng = engines("stock")[0]
    tab, width = G.torch_table32(rate)
    worst = 0.0
    for li, n_in in enumerate(G.resample_lengths(rate)):
        for si, kind in enumerate(G.RES_SIGNALS):
            x = G.resample_signal(kind, n_in, 100 * li + si)
            got = eng.resample(torch.from_numpy(x).cuda(), rate, G.RES_TARGET)
            torch.cuda.synchronize()
            got = got.cpu().numpy().astype(np.float64)
            ref, tol = G.resample_apply(x, tab, width, rate)
            assert got.shape == ref.shape == (3, G.resample_len(n_in, rate))
            err = np.abs(got - ref)
            worst = max(worst, float((err / np.where(tol > 0, tol, 1.0)).max()))
            assert (err <= tol).all(), (rate, n_in, kind, float((err / np.where(tol > 0, tol, 1.0)).max()))
    print(f"\n{rate} Hz: the kernel uses {worst:.3f} of the rule")
