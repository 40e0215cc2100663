"""The audio front end's launch rules, mirrored from the sources, a float64 reference of it, altered checkpoints that expose every
FFT bin and every band-loop regime, the table of cases that reaches every frame class of cn_logmel_kernel, and the comparison
rule the CPU and GPU tests share.  The same for the sinc resampler (smaller part, at the end).

tests/test_cpu_frontend_geometry.py holds the constants here to the text of csrc/frontend.hip and csrc/api.hip (a retuned FE_NW
fails there until this table is revisited), proves the coverage of ``cases(n_cu)`` by counting frames, and measures the rule's
constant on references; tests/test_gpu_frontend_edges.py runs the cases on the device.

The rule (power-domain interval).  An fp32 FFT of a windowed frame z errs per bin by a multiple of ||z||_2, not of the bin's own
value.  With eps = 2^-24 and delta = C eps ||z_f||_2,

    tol[f, m] = sum_k |melW[k, m]| (2 |X[f, k]| delta + delta^2) + 8 eps M[f, m]

and the device value must lie in [g(M - tol), g(M + tol)], g(M) = sc 10 log10(max(M, 1e-10)) + sh in float64, each end widened
by rounding slack: 4 ulp32(|dB|) |sc| for log10f, 2 ulp32(|out|) and 2 ulp32(|sh|) for the affine.  No element is left out.

The constant.  C_GPU = 4 C_FFT, where C_FFT is the smallest C at which an fp32 torch.fft.rfft pipeline passes against ref64 over
the whole table and all seven checkpoints (measured on the CPU, never on the kernel); the factor 4 is for the kernel's other
factorisation (radix 8 x 8 x 8 on a half-length complex transform, and an untangle stage that adds one more twiddle product and
subtracts near-equal values near k = 0 and k = 512).  Measured values (the CPU test prints and re-checks them; see
profiles/frontend_edges_notes.md):

    C_fft   = 23.33  (DC 0.5 + 1e-3 tone, L = 639, on select2; per checkpoint 7.3 .. 23.3)     -> C_FFT_MEASURED = 23.4
    C_GPU   = 93.6
    C_dense = 100.6  (oracle/cpu_ref.logmel_bn0, the fp32 dense DFT; 15.99 kHz tones on select2)
    mutations, on the gentlest input where each acts at first order:
        window shifted by one sample 1.35e5, stage twiddle 2.71e4, untangle twiddle 2.19e4, X[512] = Re Z0 + Im Z0 2.32e7,
        reflect with edge repeat 1.58e6, band one bin late 1.45e7, p0 off by one hop for b > 0 2.87e7
    at second order only (factor 10 not met, see the notes): window shift on the DC case 388, untangle twiddle on the
        bin-centred tone 381
    the kernel itself (MI355X, for information): stock 19.7, select0 20.4, select1 27.8, select2 24.0, ragged49 12.7,
        ragged50 11.8, ragged513 7.7
"""
from __future__ import annotations

import math
from typing import Callable, Dict, List, NamedTuple, Optional, Set, Tuple

import numpy as np

# ---- constants mirrored from csrc/frontend.hip and csrc/ctx.h ------------------------------------------------------------------
FE_NW = 16                       # frontend.hip: #define FE_NW 16 (waves = frames in flight per block)
FE_PITCH = 72                    # frontend.hip: #define FE_PITCH 72
N_FFT = 1024                     # CN_N_FFT
HOP = 320                        # CN_HOP
N_BINS = 513                     # CN_N_BINS
N_MELS = 224                     # CN_N_MELS
FE_LDS_TOTAL = 160 * 1024
FE_STATIC_BYTES = (512 + 513) * 8 + 1024 * 4 + FE_NW * 8 * FE_PITCH * 8 + FE_NW * 520 * 4
FE_FILL_BYTES = (FE_LDS_TOTAL - FE_STATIC_BYTES - 256) // 256 * 256
MEL_LDS_MAX_ROWS = FE_FILL_BYTES // (N_MELS * 4)     # widest band whose compact mel matrix stays in LDS (49)
RESAMPLE_BLOCK = 256             # api.hip: cn_resample_kernel launches dim3(256)
SAMPLE_RATE = 32000
EPS = 2.0 ** -24
MAX_SAMPLES = 5_000_000          # no case may hold more

P = "preprocessor.encoder."
K_REAL = P + "spectrogram_extractor.stft.conv_real.weight"
K_IMAG = P + "spectrogram_extractor.stft.conv_imag.weight"
K_MEL = P + "logmel_extractor.melW"
K_BN = tuple(P + "bn0." + s for s in ("weight", "bias", "running_mean", "running_var"))

# The rule's constant.  C_FFT_MEASURED is what tests/test_cpu_frontend_geometry.py measured (it fails if a fresh measurement
# exceeds it by a tenth, or falls below half of it: the table changed, measure again); the kernel's bound is four times that.
C_FFT_MEASURED = 23.4
C_GPU = 4.0 * C_FFT_MEASURED


# ---- launch rules of cn_frontend / cn_logmel_kernel ----------------------------------------------------------------------------
def n_frames(n_samples: int) -> int:
    return n_samples // HOP + 1


def launch(total: int, n_cu: int) -> Tuple[int, int]:
    """(grid, trips): one block per compute unit at most, each walking base = blockIdx * FE_NW + k * grid * FE_NW."""
    grid = min(-(-total // FE_NW), n_cu)
    return grid, -(-total // (grid * FE_NW))


def mel_in_lds(mel_rows: int) -> bool:
    return mel_rows * N_MELS * 4 <= FE_FILL_BYTES


def bands(melw: np.ndarray) -> np.ndarray:
    """(224, 2) [lo, hi) of the non-zero rows of every column (api.hip: an all-zero column is [0, 0))."""
    out = np.zeros((N_MELS, 2), dtype=np.int64)
    for m in range(N_MELS):
        nz = np.nonzero(melw[:, m])[0]
        if len(nz):
            out[m] = (nz[0], nz[-1] + 1)
    return out


def mel_rows_of(melw: np.ndarray) -> int:
    b = bands(melw)
    return max(1, int((b[:, 1] - b[:, 0]).max()))


def group_trips(melw: np.ndarray) -> np.ndarray:
    """(224,) trip count of every mel bin's band loop: the widest band of its group of 64 lanes."""
    b = bands(melw)
    w = b[:, 1] - b[:, 0]
    rows = mel_rows_of(melw)
    return np.array([min(int(w[m // 64 * 64:m // 64 * 64 + 64].max()), rows) for m in range(N_MELS)])


def frame_sources(n_samples: int) -> np.ndarray:
    """(F, 1024) sample index every window position of every frame reads (reflect, no edge repeat)."""
    q = (np.arange(n_frames(n_samples)) * HOP - N_FFT // 2)[:, None] + np.arange(N_FFT)[None, :]
    q = np.where(q < 0, -q, q)
    return np.where(q >= n_samples, 2 * n_samples - 2 - q, q)


def frame_class(n_samples: int, f: int) -> str:
    p0 = f * HOP - N_FFT // 2
    return "left" if p0 < 0 else ("right" if p0 + N_FFT > n_samples else "inside")


def pair_path(n_samples: int, offset: int, f: int) -> bool:
    """The frame takes the 8-byte loads: even L, 8-byte aligned base, the whole window inside the clip."""
    return n_samples % 2 == 0 and offset % 2 == 0 and frame_class(n_samples, f) == "inside"


# ---- float64 reference ------------------------------------------------------------------------------------------------------------
def ref64(wave, window, melw, bn=None):
    """wave (B, L), window (1024,), melW (513, 224), all taken as float64.  Returns (z, X, P, M): the windowed frames
    (B, F, 1024), their spectrum (B, F, 513) complex, the power spectrum and the mel power (B, F, 224).  ``bn`` is unused here
    (the affine is ``bn_affine64`` + ``g64``); it is accepted so that a call site can pass the checkpoint's four tensors along."""
    wave = np.asarray(wave, dtype=np.float64)
    pad = np.pad(wave, ((0, 0), (N_FFT // 2, N_FFT // 2)), mode="reflect")
    nf = n_frames(wave.shape[1])
    idx = (np.arange(nf) * HOP)[:, None] + np.arange(N_FFT)[None, :]
    z = pad[:, idx] * np.asarray(window, dtype=np.float64)
    X = np.fft.rfft(z, axis=-1)
    Pw = X.real ** 2 + X.imag ** 2
    return z, X, Pw, Pw @ np.asarray(melw, dtype=np.float64)


def bn_affine64(bn) -> Tuple[np.ndarray, np.ndarray]:
    """Eval-mode BatchNorm over the mel axis as out = sc x + sh, float64 (eps 1e-5)."""
    w, b, mean, var = (np.asarray(t, dtype=np.float64) for t in bn)
    sc = w / np.sqrt(var + 1e-5)
    return sc, b - mean * sc


def g64(M, sc, sh):
    return sc * (10.0 * np.log10(np.maximum(M, 1e-10))) + sh


def _ulp32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def _slack(M, sc, sh):
    db = 10.0 * np.log10(np.maximum(M, 1e-10))
    return 4.0 * _ulp32(db) * np.abs(sc) + 2.0 * _ulp32(sc * db + sh) + 2.0 * _ulp32(np.broadcast_to(sh, db.shape))


class Ref(NamedTuple):
    M: np.ndarray                # (B, F, 224) float64
    a: np.ndarray                # tol = a C + b C^2 + c
    b: np.ndarray
    c: np.ndarray
    sc: np.ndarray
    sh: np.ndarray


def make_ref(z, X, melw, bn) -> Ref:
    w = np.abs(np.asarray(melw, dtype=np.float64))
    nz = EPS * np.sqrt((z * z).sum(-1))[..., None]               # delta / C per frame
    Pw = X.real ** 2 + X.imag ** 2
    M = Pw @ np.asarray(melw, dtype=np.float64)
    sc, sh = bn_affine64(bn)
    assert (sc > 0).all(), "the interval rule is written for a positive bn0 scale"
    return Ref(M, 2.0 * nz * (np.abs(X) @ w), nz * nz * w.sum(0), 8.0 * EPS * M, sc, sh)


def spectrum_ref(z, X, bn) -> Ref:
    """The rule for the three ``select`` engines' outputs put side by side: melW is the 513 x 513 identity."""
    nz = EPS * np.sqrt((z * z).sum(-1))[..., None]
    Pw = X.real ** 2 + X.imag ** 2
    sc, sh = bn_affine64(bn)
    one = np.ones(N_BINS)
    return Ref(Pw, 2.0 * nz * np.abs(X), nz * nz * one, 8.0 * EPS * Pw, sc[0] * one, sh[0] * one)


def interval(ref: Ref, C: float) -> Tuple[np.ndarray, np.ndarray]:
    tol = ref.a * C + ref.b * C * C + ref.c
    lo_m, hi_m = ref.M - tol, ref.M + tol
    return g64(lo_m, ref.sc, ref.sh) - _slack(lo_m, ref.sc, ref.sh), g64(hi_m, ref.sc, ref.sh) + _slack(hi_m, ref.sc, ref.sh)


def violations(got, ref: Ref, C: float) -> np.ndarray:
    """Boolean mask of the elements outside the rule (a NaN is outside)."""
    lo, hi = interval(ref, C)
    got = np.asarray(got, dtype=np.float64)
    return ~((got >= lo) & (got <= hi))


def required_C(got, ref: Ref) -> float:
    """The smallest C at which ``got`` passes: closed form per element with the slack taken at ``got``, then stepped up until the
    rule itself (slack at the interval's ends) passes.  inf if no C can pass (a value below the clamp's floor, a NaN, or a
    deviation on an all-zero column)."""
    got = np.asarray(got, dtype=np.float64)
    if not np.isfinite(got).all():
        return math.inf
    floor = g64(np.zeros_like(ref.M), ref.sc, ref.sh)
    db = (got - ref.sh) / ref.sc
    s = 4.0 * _ulp32(db) * np.abs(ref.sc) + 2.0 * _ulp32(got) + 2.0 * _ulp32(np.broadcast_to(ref.sh, got.shape))
    if (got + s < floor).any():
        return math.inf
    inv = lambda y: 10.0 ** (((y - ref.sh) / ref.sc) / 10.0)
    m_up = np.where(got - s <= floor, -np.inf, inv(got - s))      # need M + tol >= m_up
    m_dn = inv(got + s)                                           # need M - tol <= m_dn
    d = np.maximum(np.maximum(m_up - ref.M, ref.M - m_dn), 0.0) - ref.c
    d = np.maximum(d, 0.0)
    disc = np.sqrt(ref.a * ref.a + 4.0 * ref.b * d)
    with np.errstate(invalid="ignore", divide="ignore"):
        need = np.where(d > 0, 2.0 * d / (ref.a + disc), 0.0)
    if not np.isfinite(need).all():
        return math.inf
    C = float(need.max())
    for _ in range(60):
        if not violations(got, ref, C).any():
            return C
        C = C * 1.02 + 1e-3
    raise AssertionError("required_C did not converge")


# ---- altered checkpoints ----------------------------------------------------------------------------------------------------------
def _identity_bn(sd: Dict[str, np.ndarray]) -> None:
    sd[K_BN[0]] = np.ones(N_MELS, dtype=np.float32)
    sd[K_BN[1]] = np.zeros(N_MELS, dtype=np.float32)
    sd[K_BN[2]] = np.zeros(N_MELS, dtype=np.float32)
    sd[K_BN[3]] = np.full(N_MELS, 1.0 - 1e-5, dtype=np.float32)


def select(j: int) -> Callable[[Dict[str, np.ndarray]], Dict[str, np.ndarray]]:
    """melW[:, m] = unit vector of bin 224 j + m (columns past bin 512 stay all-zero), bn0 the identity: the output is the dB
    power spectrum of bins 224 j .. 224 j + 223."""
    def alter(sd):
        out = dict(sd)
        w = np.zeros((N_BINS, N_MELS), dtype=np.float32)
        for m in range(N_MELS):
            if N_MELS * j + m < N_BINS:
                w[N_MELS * j + m, m] = 1.0
        out[K_MEL] = w
        _identity_bn(out)
        return out
    return alter


def ragged_melw(maxw: int, seed: int = 4242) -> np.ndarray:
    g = np.random.Generator(np.random.PCG64(seed + maxw))
    w = np.zeros((N_BINS, N_MELS), dtype=np.float32)
    for m in range(N_MELS):
        lo = m * N_BINS // N_MELS
        width = int(g.integers(1, maxw + 1))
        if m % 64 == 0:
            width = maxw         # the group's widest band (untruncated at m = 0; at 49 / 50 in every group)
        if m % 64 == 1:
            width = 1
        hi = min(lo + width, N_BINS)
        col = g.uniform(0.05, 1.0, hi - lo)
        gaps = g.random(hi - lo) < 0.1
        gaps[0] = gaps[-1] = False   # the band's ends stay non-zero: they are what api.hip locates
        col[gaps] = 0.0
        w[lo:hi, m] = col.astype(np.float32)
    return w


def asym_window(seed: int = 777) -> np.ndarray:
    """A positive, non-smooth, asymmetric window in [0.2, 1] (float64)."""
    g = np.random.Generator(np.random.PCG64(seed))
    return g.uniform(0.2, 1.0, N_FFT)


def dft_tensors(window64: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    n = np.arange(N_FFT, dtype=np.int64)
    k = np.arange(N_BINS, dtype=np.int64)
    ang = -2.0 * np.pi * ((k[:, None] * n[None, :]) % N_FFT).astype(np.float64) / N_FFT
    return ((np.cos(ang) * window64).astype(np.float32)[:, None, :], (np.sin(ang) * window64).astype(np.float32)[:, None, :])


def ragged(maxw: int) -> Callable[[Dict[str, np.ndarray]], Dict[str, np.ndarray]]:
    def alter(sd):
        out = dict(sd)
        out[K_MEL] = ragged_melw(maxw)
        _identity_bn(out)
        if maxw == N_BINS:
            out[K_REAL], out[K_IMAG] = dft_tensors(asym_window())
        return out
    return alter


CHECKPOINTS: Dict[str, Optional[Callable]] = {
    "stock": None, "select0": select(0), "select1": select(1), "select2": select(2),
    "ragged49": ragged(49), "ragged50": ragged(50), "ragged513": ragged(513),
}


def checkpoint(name: str, sd: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    alter = CHECKPOINTS[name]
    return dict(sd) if alter is None else alter(sd)


def front_tensors(sd) -> Tuple[np.ndarray, np.ndarray, tuple]:
    """(window, melW, bn) of a state dict, as the device takes them: the window is row 0 of conv_real in fp32."""
    t = lambda k: np.asarray(sd[k], dtype=np.float32)
    return t(K_REAL)[0, 0, :], t(K_MEL), tuple(t(k) for k in K_BN)


# ---- signals ------------------------------------------------------------------------------------------------------------------------
KINDS = ("noise", "tone_c", "tone_off", "dc_tone", "impulse", "tiny", "int16", "t15500", "t15990", "synth")
IMPULSE_AT = 700


def _clip(kind: str, n: int, g, i: int) -> np.ndarray:
    t = np.arange(n, dtype=np.float64)
    ph = g.uniform(0, 2 * np.pi)
    tone = lambda hz, a: a * np.sin(2.0 * np.pi * hz / SAMPLE_RATE * t + ph)
    if kind == "noise":
        return 0.1 * g.standard_normal(n)
    if kind == "tone_c":
        return tone(100 * SAMPLE_RATE / N_FFT, 0.5)          # bin 100 exactly
    if kind == "tone_off":
        return tone(100.37 * SAMPLE_RATE / N_FFT, 0.5)
    if kind == "dc_tone":
        return 0.5 + tone(5000.0, 1e-3)
    if kind == "impulse":
        x = np.zeros(n)
        x[min(IMPULSE_AT + 37 * i, n - 1)] = 1.0
        return x
    if kind == "tiny":
        return tone(1000.0, 1e-6)
    if kind == "int16":
        return 3e4 * g.standard_normal(n)
    if kind == "t15500":
        return tone(15500.0, 0.5)
    if kind == "t15990":
        return tone(15990.0, 0.5)
    raise KeyError(kind)


class Case(NamedTuple):
    name: str
    b: int
    n_samples: int
    lengths: Tuple[int, ...]     # true length of every clip (zero beyond)
    kind: str
    offset: int                  # 0, or 1: the batch is a contiguous view one float into a larger buffer
    seed: int

    @property
    def total(self) -> int:
        return self.b * n_frames(self.n_samples)


def make_wave(c: Case) -> np.ndarray:
    """(B, L) float32, built in float64 and rounded."""
    if c.kind == "synth":
        from conette_amd import synth
        return synth.synth_waveforms(c.b, c.n_samples, c.seed, lengths=list(c.lengths))
    out = np.zeros((c.b, c.n_samples), dtype=np.float64)
    for i in range(c.b):
        g = np.random.Generator(np.random.PCG64(c.seed + i))
        out[i, :c.lengths[i]] = _clip(c.kind, c.n_samples, g, i)[:c.lengths[i]]
    return out.astype(np.float32)


def _lens(b: int, n: int, ragged_: bool) -> Tuple[int, ...]:
    if not ragged_:
        return (n,) * b
    return tuple(n if i % 3 == 0 else (n // 3 if i % 3 == 1 else n * 5 // 8) for i in range(b))


def _factor(total: int) -> Tuple[int, int]:
    """(B, F) with B F == total, short clips first (21 frames = 6400 samples where total allows)."""
    for f in [21] + list(range(20, 2, -1)) + list(range(22, 65)):
        if total % f == 0:
            return total // f, f
    return 1, total


BOUNDARY_L = 6 * HOP + N_FFT // 2    # 2432: frame 6 ends exactly at L (p0 + 1024 == L), F = 8


def cases(n_cu: int) -> List[Case]:
    out: List[Case] = []

    def add(name, b, n, kind, offset=0, ragged_=False):
        c = Case(name, b, n, _lens(b, n, ragged_), kind, offset, 31000 + 64 * len(out))
        assert c.b * c.n_samples <= MAX_SAMPLES and n > N_FFT // 2, c
        out.append(c)

    add("t2_L513", 1, 513, "noise")                              # the smallest legal length: 2 frames, both reflected twice
    add("t15_odd", 3, 1281, "tone_off")                          # 15 frames; odd L, B >= 2: rows 1, 2 misaligned
    add("t16_edge", 2, BOUNDARY_L, "noise")                      # 16 frames; f = 6 is the last frame of the 8-byte path
    add("t17", 1, 16 * HOP + 7, "tone_c")                        # 17 frames
    add("L639", 1, 639, "dc_tone")
    add("L640", 1, 640, "impulse")
    add("L641", 2, 641, "tiny")
    add("edge_m2", 2, BOUNDARY_L - 2, "int16")                   # even, two samples of frame 6 reflected
    add("edge_m1", 2, BOUNDARY_L - 1, "t15500")                  # odd
    add("edge_off1", 2, BOUNDARY_L, "t15990", offset=1)          # even L through the one-float offset: no 8-byte loads
    add("four_kinds", 3, 6400, "synth", ragged_=True)            # left / right reflect, inside, inside zero padding; seams
    add("four_off1", 3, 6400, "noise", offset=1, ragged_=True)
    add("imp_17", 1, 16 * HOP, "impulse")
    add("hi_tones", 4, 6400, "t15990", ragged_=True)
    add("hi_15500", 3, 3200, "t15500")
    add("dc", 3, 4001, "dc_tone")
    add("tiny", 3, 3200, "tiny", ragged_=True)
    add("int16", 3, 3333, "int16", ragged_=True)
    add("tone_c", 3, 5000, "tone_c")
    full = n_cu * FE_NW
    for tag, total, kind, off in (("m1", full - 1, "noise", 0), ("full", full, "tone_off", 0), ("p1", full + 1, "synth", 0),
                                  ("p17", full + 17, "noise", 0)):
        b, f = _factor(total)
        n = (f - 1) * HOP + (HOP // 2 if tag != "p17" else 0)
        n += n % 2                                               # even (p17's twin below needs the offset view)
        add(f"big_{tag}", b, n, kind, off, ragged_=b >= 3)
    return out


def case(name: str, n_cu: int) -> Case:
    return next(c for c in cases(n_cu) if c.name == name)


CASE_NAMES = [c.name for c in cases(256)]


def coverage(case_list: List[Case], n_cu: int) -> Set[Tuple[str, object]]:
    """What a table of cases reaches, counted with the mirrored rules above."""
    hit: Set[Tuple[str, object]] = set()
    for c in case_list:
        nf = n_frames(c.n_samples)
        grid, trips = launch(c.total, n_cu)
        hit.add(("total", c.total))
        hit.add(("L", c.n_samples))
        hit.add(("kind", c.kind))
        if trips >= 2:
            hit.add(("second_trip", c.total % FE_NW != 0))       # True: its last block is partial
        classes = set()
        for i in range(c.b):
            for f in range(nf):
                k = frame_class(c.n_samples, f)
                p0 = f * HOP - N_FFT // 2
                if k == "inside" and p0 >= c.lengths[i]:
                    k = "padding"
                classes.add(k)
                if k in ("inside", "padding"):
                    hit.add(("pair", pair_path(c.n_samples, c.offset, f)))
                if p0 + N_FFT == c.n_samples:
                    hit.add(("window_ends_at_L", (c.n_samples % 2, c.offset)))
                if k == "right" and c.n_samples % 2 == 0 and p0 + N_FFT == c.n_samples + 2:
                    hit.add(("two_reflected", c.offset))
        if classes >= {"left", "right", "inside", "padding"}:
            hit.add(("four_kinds", c.offset))
        if c.n_samples % 2 == 1 and c.b >= 2:
            hit.add(("odd_rows", True))
        if c.n_samples % 2 == 0 and c.offset == 1:
            hit.add(("even_offset", True))
        if c.b >= 3 and nf % FE_NW != 0 and any((base // nf) != (min(base + FE_NW, c.total) - 1) // nf
                                                for base in range(0, c.total, FE_NW)):
            hit.add(("seam_in_block", True))
    return hit


def required_coverage(n_cu: int) -> Set[Tuple[str, object]]:
    full = n_cu * FE_NW
    want: Set[Tuple[str, object]] = {("total", t) for t in (2, 15, 16, 17, full - 1, full, full + 1, full + 17)}
    want |= {("L", n) for n in (513, 639, 640, 641, BOUNDARY_L, BOUNDARY_L - 1, BOUNDARY_L - 2)}
    want |= {("kind", k) for k in KINDS}
    want |= {("second_trip", True), ("pair", True), ("pair", False), ("window_ends_at_L", (0, 0)), ("window_ends_at_L", (0, 1)),
             ("two_reflected", 0), ("four_kinds", 0), ("four_kinds", 1), ("odd_rows", True), ("even_offset", True),
             ("seam_in_block", True)}
    return want


# ---- an explicit half-length FFT + untangle in float64, for the seeded mutations -------------------------------------------------
def tables64() -> Tuple[np.ndarray, np.ndarray]:
    return np.exp(-2j * np.pi * np.arange(512) / 512.0), np.exp(-2j * np.pi * np.arange(513) / 1024.0)


def fft_untangle64(zr: np.ndarray, tw512: np.ndarray, tw1024: np.ndarray, nyquist_plus: bool = False) -> np.ndarray:
    """Spectrum (…, 513) of real frames (…, 1024) the way the kernel factors it: z[n] = x[2n] + i x[2n+1], a 512-point transform
    as radix 8 x 8 x 8 with the twiddles tw512[b c] and tw512[8 b' c'], then X[k] = E + tw1024[k] O and X[512] = Re Z0 - Im Z0."""
    lead = zr.shape[:-1]
    z = (zr[..., 0::2] + 1j * zr[..., 1::2]).reshape(-1, 8, 64)                      # [a][b], n = 64 a + b
    D = np.exp(-2j * np.pi * np.outer(np.arange(8), np.arange(8)) / 8.0)
    y = np.einsum("ca,nab->ncb", D, z) * tw512[np.outer(np.arange(8), np.arange(64))]      # [c][b] * W^(b c)
    y = y.reshape(-1, 8, 8, 8)                                                        # [c][a'][b'], b = 8 a' + b'
    y = np.einsum("da,ncab->ncdb", D, y) * tw512[8 * np.outer(np.arange(8), np.arange(8))]   # [c][c'][b'] * W^(8 b' c')
    Z = np.einsum("eb,ncdb->nedc", D, y).reshape(-1, 512)                             # k = c + 8 c' + 64 d'
    k = np.arange(512)
    A, B = Z, np.conj(Z[:, (512 - k) % 512])
    X = np.empty((Z.shape[0], N_BINS), dtype=np.complex128)
    X[:, :512] = 0.5 * (A + B) + tw1024[:512] * (-0.5j) * (A - B)
    X[:, 512] = Z[:, 0].real + Z[:, 0].imag if nyquist_plus else Z[:, 0].real - Z[:, 0].imag
    return X.reshape(lead + (N_BINS,))


def frames64(wave: np.ndarray, edge_repeat: bool = False, hop_off: bool = False) -> np.ndarray:
    """(B, F, 1024) unwindowed frames in float64 by index arithmetic (the kernel's way, not numpy's pad)."""
    wave = np.asarray(wave, dtype=np.float64)
    b, n = wave.shape
    out = np.empty((b, n_frames(n), N_FFT))
    for i in range(b):
        q = (np.arange(n_frames(n)) * HOP - N_FFT // 2 + (HOP if (hop_off and i > 0) else 0))[:, None] + np.arange(N_FFT)[None, :]
        q = np.where(q < 0, -q - (1 if edge_repeat else 0), q)
        q = np.where(q >= n, 2 * n - 2 - q + (1 if edge_repeat else 0), q)
        out[i] = wave[i, np.clip(q, 0, n - 1)]
    return out


MUTATIONS = ("window_shift", "stage_twiddle", "untangle_twiddle", "nyquist_plus", "edge_repeat", "band_late", "hop_off")


def mutated64(name: str, wave, window, melw) -> np.ndarray:
    """Mel power (B, F, 224) of the float64 pipeline with one seeded mistake."""
    window = np.asarray(window, dtype=np.float64)
    melw = np.asarray(melw, dtype=np.float64)
    t512, t1024 = tables64()
    if name == "window_shift":
        window = np.roll(window, 1)
    if name == "stage_twiddle":
        t512 = t512.copy()
        t512[37] = t512[38]
    if name == "untangle_twiddle":
        t1024 = t1024.copy()
        t1024[101] = t1024[102]
    if name == "band_late":
        melw = melw.copy()
        lo = bands(melw)[:, 0]
        melw[lo, np.arange(N_MELS)] = 0.0
    z = frames64(wave, edge_repeat=name == "edge_repeat", hop_off=name == "hop_off") * window
    X = fft_untangle64(z, t512, t1024, nyquist_plus=name == "nyquist_plus")
    return (X.real ** 2 + X.imag ** 2) @ melw


# ---- fp32 stand-ins measured on the CPU --------------------------------------------------------------------------------------------
def fft32_pipeline(wave32: np.ndarray, window32, melw32, bn32) -> np.ndarray:
    """The front end with torch's fp32 rfft: fp32 throughout, the affine with fp32 coefficients."""
    import torch
    src = frame_sources(wave32.shape[1])
    z = torch.from_numpy(wave32[:, src] * np.asarray(window32, dtype=np.float32))
    X = torch.fft.rfft(z, dim=-1)
    Pw = X.real * X.real + X.imag * X.imag
    M = Pw @ torch.from_numpy(np.asarray(melw32, dtype=np.float32))
    w, b, mean, var = (torch.from_numpy(np.asarray(t, dtype=np.float32)) for t in bn32)
    sc = w / torch.sqrt(var + 1e-5)
    sh = b - mean * sc
    return (10.0 * torch.log10(torch.clamp(M, min=1e-10)) * sc + sh).numpy()


# ---- resampler -------------------------------------------------------------------------------------------------------------------
RATES = (8000, 11025, 12000, 16000, 22050, 24000, 44100, 48000, 88200, 96000, 192000, 52800)
RES_TARGET = 32000


def resample_ratio(orig: int, new: int = RES_TARGET) -> Tuple[int, int]:
    g = math.gcd(orig, new)
    return orig // g, new // g


def resample_len(n_in: int, orig: int, new: int = RES_TARGET) -> int:
    """conette_resample_len in exact integers: ceil(n len / o)."""
    o, n = resample_ratio(orig, new)
    return -(-n * n_in // o)


def host_table32(orig: int, new: int = RES_TARGET) -> Tuple[np.ndarray, int]:
    """numpy-fp32 emulation of the table conette_resample builds on the host (api.hip): (n, K) float32 and its width."""
    f = np.float32
    o, n = resample_ratio(orig, new)
    lpw = f(6.0)
    base = f(min(o, n)) * f(0.99)
    width = int(math.ceil(float(np.float64(lpw) * o / np.float64(base))))
    K = 2 * width + o
    scale = base / f(o)
    idx = (np.arange(K, dtype=np.int64) - width).astype(f) / f(o)
    tt = (-np.arange(n, dtype=np.int64)).astype(f)[:, None] / f(n) + idx[None, :]
    tt = tt * base
    tt = np.minimum(np.maximum(tt, -lpw), lpw)
    cw = np.cos(tt * f(math.pi) / lpw / f(2.0))
    window = cw * cw
    tt = tt * f(math.pi)
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.where(tt == 0, f(1.0), np.sin(tt) / tt)
    tab = sinc * window * scale
    assert tab.dtype == np.float32
    return tab, width


def torch_table32(orig: int, new: int = RES_TARGET) -> Tuple[np.ndarray, int]:
    import torch
    from oracle.thirdparty import sinc_resample_kernel
    k, width = sinc_resample_kernel(orig, new, dtype=torch.float32)
    return k[:, 0, :].numpy(), int(width)


def _windows(x: np.ndarray, o: int, width: int, K: int, n_blocks: int) -> np.ndarray:
    pad = np.zeros((x.shape[0], (n_blocks - 1) * o + K + 1))
    m = min(x.shape[1], pad.shape[1] - width)
    pad[:, width:width + m] = x[:, :m]
    idx = (np.arange(n_blocks) * o)[:, None] + np.arange(K)[None, :]
    return pad[:, idx]                                            # (rows, n_blocks, K): samples start = m o - width ..


def resample_apply(x, table, width: int, orig: int, new: int = RES_TARGET, start_off: int = 0):
    """Float64 accumulation of a (n, K) table over x (rows, n_in): (out, tol), both (rows, n_out).
    tol_i = 2^-21 ||x_win,i||_2 + 8 2^-24 sum_t |k_t x_t|."""
    x = np.asarray(x, dtype=np.float64)
    table = np.asarray(table, dtype=np.float64)
    o, n = resample_ratio(orig, new)
    n_out = resample_len(x.shape[1], orig, new)
    n_blocks = -(-n_out // n)
    win = _windows(x, o, width - start_off, table.shape[1], n_blocks)
    out = win @ table.T                                           # (rows, n_blocks, n)
    tol = 2.0 ** -21 * np.sqrt((win * win).sum(-1))[..., None] + 8.0 * EPS * (np.abs(win) @ np.abs(table).T)
    return out.reshape(x.shape[0], -1)[:, :n_out], tol.reshape(x.shape[0], -1)[:, :n_out]


def resample_lengths(orig: int) -> List[int]:
    o, n = resample_ratio(orig)
    width = torch_width(orig)
    lens = {1, width - 1, width, o, o + 1, 3 * o - 1}
    # n_out one more than a multiple of n, and of the block (an up-sampling ratio steps over some residues: 8 kHz gives 4 len)
    lens.add(next((l for l in range(3 * o, 3 * o + 4000) if n > 1 and resample_len(l, orig) % n == 1), 3 * o))
    lens.add(next((l for l in range(max(600, 2 * o), max(600, 2 * o) + 400 * o)
                   if resample_len(l, orig) % RESAMPLE_BLOCK == 1), 3 * o))
    return sorted(l for l in lens if l >= 1)


def torch_width(orig: int) -> int:
    o, n = resample_ratio(orig)
    return math.ceil(6 * o / (min(o, n) * 0.99))


RES_SIGNALS = ("noise", "tone", "imp_first", "imp_last")


def resample_signal(kind: str, n_in: int, seed: int) -> np.ndarray:
    """(3, n_in) float32: three rows of distinct data."""
    g = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(n_in, dtype=np.float64)
    x = np.zeros((3, n_in))
    for r in range(3):
        if kind == "noise":
            x[r] = g.standard_normal(n_in)
        elif kind == "tone":
            x[r] = 1e-3 * np.sin(2.0 * np.pi * (0.01 + 0.013 * r) * t + g.uniform(0, 6.28))
        elif kind == "imp_first":
            x[r, 0] = 1.0 + r
        else:
            x[r, n_in - 1] = 1.0 + r
    return x.astype(np.float32)
