"""The tables the tag-timeline tests share (conette_amd/tagging.py, csrc/enc_tags.h).

Frame cases ``(name, fe (B, T, 768) fp32, lens (B,), windows)``: frame embeddings of three golden fixtures -- one with lengths forced
to [39, 13, 1, 0] -- and seeded Gaussian ones (rms 1 plus a per-channel offset) at T = 1, 2, 8, 9; B T = 1, 3, 6, 8, 27, 94 and 156
rows cover the row tails of the head GEMM.  Windows come from {1, 2, 3, 4, 7, 2 T - 1, 255}; of the first five those beyond 2 T are
left out (they pool what 2 T - 1 pools).

Event cases ``(name, p (T,) fp32, n, settings)``, settings = (on, off, min_frames, max_gap, max_events): handcrafted sequences for
every clause of the event rule; the expected tables are written out in tests/test_cpu_tagging.py."""
import functools

import numpy as np

from tests import golden_util as G

FEAT, N_TAGS = 768, 527
NORM_W, NORM_B = "preprocessor.encoder.norm.weight", "preprocessor.encoder.norm.bias"
HEAD_W, HEAD_B = "preprocessor.encoder.head_audioset.weight", "preprocessor.encoder.head_audioset.bias"

FIXTURES = (("b2_1s_beam3", None), ("b4_odd_beam5_minpred0", [39, 13, 1, 0]), ("b1_30s_beam3", None))
GAUSSIAN = ((1, 1, [1]), (2, 3, [2, 1, 2]), (8, 1, [8]), (9, 3, [9, 8, 4]))      # (T, B, lens)


def windows_for(t):
    return sorted({w for w in (1, 2, 3, 4, 7) if w <= 2 * t} | {2 * t - 1, 255})


@functools.lru_cache(maxsize=None)
def frame_cases():
    out = []
    for name, forced in FIXTURES:
        g = G.load(name)
        fe = np.ascontiguousarray(g["frame_embs"], dtype=np.float32)
        lens = np.asarray(g["audio_shape"][:, 1] if forced is None else forced, dtype=np.int32)
        assert fe.shape[0] == len(lens) and fe.shape[2] == FEAT and lens.max() <= fe.shape[1]
        out.append((name, fe, lens, windows_for(fe.shape[1])))
    for t, b, lens in GAUSSIAN:
        rng = np.random.Generator(np.random.PCG64(1000 + 10 * t + b))
        fe = (rng.standard_normal((b, t, FEAT)) + 0.5 * rng.standard_normal(FEAT)).astype(np.float32)
        out.append((f"gauss_T{t}_B{b}", fe, np.asarray(lens, dtype=np.int32), windows_for(t)))
    return tuple(out)


def head(weights):
    """(norm_w, norm_b, head_w, head_b) as numpy arrays from a state dict of numpy arrays or tensors"""
    return tuple(np.asarray(weights[k]) for k in (NORM_W, NORM_B, HEAD_W, HEAD_B))


# ---- event sequences -----------------------------------------------------------------------------------------------------------------
f32 = np.float32
ON, OFF = f32(0.5), f32(0.3)
BELOW = np.nextafter(ON, f32(0))        # one ulp below ON
H, M, L = f32(0.9), f32(0.4), f32(0.1)  # above ON; between OFF and ON; below OFF
NAN = f32("nan")


def seq(*values):
    return np.asarray(values, dtype=np.float32)


EVENT_CASES = (
    ("lone_frame_at_on", seq(L, ON, L), 3, ((ON, ON, 1, 0, 4), (ON, OFF, 1, 0, 4), (ON, ON, 2, 0, 4))),
    ("one_ulp_below_on", seq(L, BELOW, L), 3, ((ON, ON, 1, 0, 4), (ON, OFF, 1, 0, 4), (BELOW, BELOW, 1, 0, 4))),
    ("plateau_never_on", seq(L, M, M, M, L), 5, ((ON, OFF, 1, 0, 4), (M, OFF, 1, 0, 4))),
    ("plateau_on_in_last_frame", seq(L, M, M, H, L), 5, ((ON, OFF, 1, 0, 4), (ON, ON, 1, 0, 4), (ON, OFF, 4, 0, 4))),
    # runs [0, 2), [4, 5), [8, 9): gaps of 2 and of 3 frames
    ("gaps_of_2_and_3", seq(H, H, L, L, H, L, L, L, H), 9, ((ON, ON, 1, 2, 4), (ON, ON, 1, 3, 4), (ON, ON, 1, 1, 4), (ON, ON, 1, 0, 4))),
    ("short_until_merged", seq(H, L, H, L, L, L, H), 7, ((ON, ON, 3, 1, 4), (ON, ON, 3, 0, 4), (ON, ON, 1, 1, 4))),
    ("run_cut_by_n", seq(L, H, H, H, H), 3, ((ON, ON, 1, 0, 4), (ON, ON, 3, 0, 4))),
    ("runs_at_0_and_at_n_minus_1", seq(H, L, L, H, H), 4, ((ON, ON, 1, 0, 4), (ON, ON, 1, 2, 4))),
    ("n_is_0", seq(H, H, H), 0, ((ON, ON, 1, 0, 4), (ON, OFF, 1, 3, 1))),
    ("alternating", seq(H, L, H, L, H, L, H, L, H, L), 10, ((ON, ON, 1, 0, 1), (ON, ON, 1, 0, 4), (ON, ON, 1, 0, 64), (ON, ON, 1, 1, 1))),
    ("nan_inside_a_run", seq(f32(0.8), NAN, H, L), 4, ((ON, ON, 1, 0, 4), (ON, OFF, 1, 1, 4))),
    ("equal_peaks", seq(M, H, f32(0.6), H, M), 5, ((ON, OFF, 1, 0, 4), (ON, ON, 1, 0, 4))),
    ("dip_between_off_and_on", seq(f32(0.6), M, H), 3, ((ON, OFF, 1, 0, 4), (ON, ON, 1, 0, 4), (ON, ON, 1, 1, 4))),
)


T_EVENTS = max(len(s) for _, s, _, _ in EVENT_CASES)
EVENT_LENGTHS = sorted({n for _, _, n, _ in EVENT_CASES})            # every sequence's own n
EVENT_SETTINGS = sorted({s for _, _, _, settings in EVENT_CASES for s in settings}, key=lambda s: tuple(float(v) for v in s))


def padded(i):
    """sequence i at the common length T_EVENTS, continued with frames below every threshold"""
    s = EVENT_CASES[i][1]
    return np.concatenate([s, np.full(T_EVENTS - len(s), L, dtype=np.float32)])


def tiled_events_input(batch=3, n_tags=N_TAGS):
    """(p (batch, T_EVENTS, n_tags) fp32, which (batch, n_tags)): the sequences tiled over the tags, each clip's pattern shifted by
    eight more tags -- thread b n_tags + c takes sequence (c + 8 b) mod 13, so with 527 tags and three clips every lane of a wave
    meets every sequence (tests/test_cpu_tagging.py counts them)."""
    which = (np.arange(n_tags)[None, :] + 8 * np.arange(batch)[:, None]) % len(EVENT_CASES)
    table = np.stack([padded(i) for i in range(len(EVENT_CASES))])      # (cases, T)
    return np.ascontiguousarray(table[which].transpose(0, 2, 1)), which
