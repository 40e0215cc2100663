"""ctypes binding of libconette_hip.so (include/conette_hip.h).

PyTorch is plumbing here: it owns device memory and the stream; every dense stage of the hot
path runs in the hand-written HIP library.  There is NO CPU / eager fallback: if the library
is missing or a call fails, this module raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Any, Dict, Optional, Tuple

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libconette_hip.so")

PREC_F32 = 0
PREC_BF16 = 1
PREC_F16X2 = 2   # "exact": fp16 hi/lo operand pairs, three MFMAs per product (include/conette_hip.h)
# (3 was the experimental fp8 precision of ABI 2: withdrawn in round 6 -- e4m3 operands cost the frame embeddings 4 % whatever
#  the scaling, block-scaled MX included: profiles/r06_notes.md section 3)
PREC_F16 = 4     # the bf16 mode's kernels with IEEE fp16 operands: 8x less operand rounding error at the same speed
N_MELS = 224
FEAT = 768
N_TAGS = 527

EXPORTS = (
    "conette_last_error", "conette_abi_version", "conette_create", "conette_destroy", "conette_num_frames",
    "conette_num_audio_frames", "conette_encode_workspace_bytes", "conette_decode_workspace_bytes",
    "conette_frontend_logmel", "conette_encode", "conette_decode", "conette_resample", "conette_resample_len",
    "conette_set_option", "conette_profile_enable", "conette_profile_read", "conette_stream_create_masked",
    "conette_stream_destroy", "conette_forcing_workspace_bytes", "conette_forcing",
    "conette_greedy_workspace_bytes", "conette_greedy", "conette_decode_graph_nodes", "conette_encode_nonfinite",
    "conette_score_workspace_bytes", "conette_score", "conette_sample_workspace_bytes", "conette_sample",
    "conette_align_workspace_bytes", "conette_align", "conette_decode_groups_workspace_bytes", "conette_decode_groups",
    "conette_decode_constrained_workspace_bytes", "conette_decode_constrained",
    "conette_decode_required_workspace_bytes", "conette_decode_required",
    "conette_decode_ensemble_workspace_bytes", "conette_decode_ensemble", "conette_consensus",
    "conette_tag_frames_workspace_bytes", "conette_tag_frames", "conette_tag_events",
    "conette_decode_spans_workspace_bytes", "conette_decode_spans", "conette_segments",
)
# ---- precision "certified": when is a 16-bit search's decision as good as an exact one's? ------------------------------------
# Per base precision and kind of search, (a, b, c): the top-k call of step i is certified when its margin is at least
# a + b * (i + 1), the final best-beam choice when its margin is at least c.  Calibration (tools/calibrate_margins.py: 512 + 4096
# clips x 2 synthetic checkpoints x greedy / beam 3 against the exact precision with per-call traces, ~10^6 decisions per base
# precision; profiles/r06_margin_calibration*.txt): when a 16-bit search leaves the exact search's trajectory, the margin it saw at
# that call was at most
#     mixed16 0.0156 (greedy) / 0.0218 (beam 3),  f16 0.0312 / 0.0371,  bf16+f16dec 0.097 / 0.184,  bf16 0.193 / 0.290
# -- flat over the 20 steps (the running sums' error is common to the candidates of a parent and cancels in a gap; hence b = 0),
# larger between rows of different parents (beam > 1) than inside one row (greedy); final choice on the averaged scores: at most
# 0.0007 / 0.0014 / 0.013 / 0.019.  The tail is heavy: the 4096-clip maxima are about twice the 512-clip ones (the first
# tolerances, 1.7 x the 512-clip maxima, let ONE greedy clip of a 4096-clip soak through: profiles/r06_certified_soak_first.txt).
# The tolerances below are 2 x the maxima of all 4608 clips per checkpoint.  The certificate is therefore exact in its logic and
# STATISTICAL in its tolerance: tools/certified_soak.py (profiles/r06_certified_soak.txt) counts what gets through on fresh clips;
# what the tolerances cost is the share of clips whose closest decision is nearer than that: `recompute_fraction` of the bench line.
# Other beam sizes (profiles/r06_margin_calibration_beams.txt, base mixed16, 2 048 clips per checkpoint): beams 2 and 5 stay inside the
# beam-3 maxima (0.021 / 0.022; final choice 0.0024), beam 8 reached 0.0385 -- more rows, more chances of a large deviation -- hence a
# third class, "wide" (beam >= 6), at 2 x that; for the other bases the wide tolerances are the beam-3 ones scaled by the same 1.77 and
# were then held to their own runs at beams 2 / 5 / 8 (profiles/r06_margin_calibration_beams_other.txt: f16 reached 0.0405 at beam 2 -- its
# beam tolerance is 2 x that --, bf16 0.024 on the final choice).
# A certificate at beam >= 5 flags 93-100 % of the clips of either synthetic checkpoint anyway.
CERT_TOL = {
    "mixed16": {"greedy": (0.032, 0.0, 0.0), "beam": (0.045, 0.0, 0.005), "wide": (0.08, 0.0, 0.005)},
    "f16": {"greedy": (0.063, 0.0, 0.0), "beam": (0.082, 0.0, 0.008), "wide": (0.13, 0.0, 0.008)},
    "bf16+f16dec": {"greedy": (0.20, 0.0, 0.0), "beam": (0.37, 0.0, 0.026), "wide": (0.65, 0.0, 0.05)},
    "bf16": {"greedy": (0.39, 0.0, 0.0), "beam": (0.58, 0.0, 0.05), "wide": (1.0, 0.0, 0.08)},
}


def cert_kind(beam: int) -> str:
    """the tolerance class of a search: greedy (beam 1), beam (2-5), wide (>= 6)"""
    return "greedy" if int(beam) == 1 else ("beam" if int(beam) <= 5 else "wide")


# The default base: fp16 encoder + EXACT decoder.  Measured against the f16 base in one call (profiles/r06_c_certified_*.json): the exact
# decoder costs every step 0.35 ms, its tighter tolerance spares more exact-ENCODER re-runs than that -- greedy 9.6 k against 8.8 k
# clips/s on the peaked checkpoint (8 % against 16 % of the clips re-run), 6.1 k against 5.1 k on the default one; beam 3 4.8 k against 4.1 k.
CERT_DEFAULT_BASE = "mixed16"
OPT_DECODE_GRAPH = 1
OPT_DECODE_FUSION = 2
OPT_ENCODE_RESERVED_CUS = 3
OPT_FORCING_STEPWISE = 4
OPT_SCORE_VSPLIT = 5
MAX_DECODE_GRAPHS = 64   # CONETTE_MAX_DECODE_GRAPHS: decode hipGraphs (= persistent buffer sets) kept per context
PROF_CLASSES = ("frontend", "stem", "dwconv_ln", "pw1_gemm", "pw2_gemm", "downsample", "heads", "dec_prepare",
                "dec_gemm", "dec_attn", "dec_misc", "search")


class ConetteConfigC(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("precision", "vocab_size", "d_model", "nhead", "n_layers", "d_ff", "pad_id",
                                         "bos_id", "eos_id")] + [("reserved", C.c_int32 * 7)]


class EncodeTapsC(C.Structure):
    _fields_ = [("struct_bytes", C.c_size_t), ("logmel", C.c_void_p), ("stem", C.c_void_p), ("stage_block0", C.c_void_p * 4),
                ("stage", C.c_void_p * 4), ("down", C.c_void_p * 4), ("block", C.c_void_p * 18)]


class ConetteMemberC(C.Structure):
    """conette_member (include/conette_hip.h): one member of a conette_decode_ensemble call"""
    _fields_ = [("ctx", C.c_void_p), ("frame_embs", C.c_void_p), ("bos_ids", C.c_void_p), ("weight", C.c_float),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t)]


_lib = None


def load_library() -> C.CDLL:
    """dlopen the in-tree library; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(the MI355X path has no CPU fallback)")
    lib = C.CDLL(LIB_PATH)
    lib.conette_last_error.restype = C.c_char_p
    lib.conette_abi_version.restype = C.c_int
    lib.conette_create.restype = C.c_int
    lib.conette_create.argtypes = [C.POINTER(ConetteConfigC), C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_void_p),
                                   C.POINTER(C.c_int64), C.POINTER(C.c_void_p)]
    lib.conette_destroy.restype = None
    lib.conette_destroy.argtypes = [C.c_void_p]
    lib.conette_num_frames.restype = C.c_int32
    lib.conette_num_frames.argtypes = [C.c_int32]
    lib.conette_num_audio_frames.restype = C.c_int32
    lib.conette_num_audio_frames.argtypes = [C.c_int32]
    lib.conette_encode_workspace_bytes.restype = C.c_size_t
    lib.conette_encode_workspace_bytes.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    lib.conette_decode_workspace_bytes.restype = C.c_size_t
    lib.conette_decode_workspace_bytes.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    lib.conette_frontend_logmel.restype = C.c_int
    lib.conette_frontend_logmel.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    lib.conette_encode.restype = C.c_int
    lib.conette_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                   C.POINTER(EncodeTapsC), C.c_void_p, C.c_size_t, C.c_void_p]
    lib.conette_decode.restype = C.c_int
    lib.conette_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                   C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                   C.c_void_p]
    lib.conette_encode_nonfinite.restype = C.c_int
    lib.conette_encode_nonfinite.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]
    lib.conette_forcing_workspace_bytes.restype = C.c_size_t
    lib.conette_forcing_workspace_bytes.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
    lib.conette_forcing.restype = C.c_int
    lib.conette_forcing.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                    C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.conette_score_workspace_bytes.restype = C.c_size_t
    lib.conette_score_workspace_bytes.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    lib.conette_score.restype = C.c_int
    lib.conette_score.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                  C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.conette_align_workspace_bytes.restype = C.c_size_t
    lib.conette_align_workspace_bytes.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    lib.conette_align.restype = C.c_int
    lib.conette_align.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                  C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_size_t, C.c_void_p]
    lib.conette_sample_workspace_bytes.restype = C.c_size_t
    lib.conette_sample_workspace_bytes.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    lib.conette_sample.restype = C.c_int
    lib.conette_sample.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                   C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_float, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.conette_decode_groups_workspace_bytes.restype = C.c_size_t
    lib.conette_decode_groups_workspace_bytes.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    lib.conette_decode_groups.restype = C.c_int
    lib.conette_decode_groups.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                          C.c_int32, C.c_float, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.conette_decode_constrained_workspace_bytes.restype = C.c_size_t
    lib.conette_decode_constrained_workspace_bytes.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    lib.conette_decode_constrained.restype = C.c_int
    lib.conette_decode_constrained.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                               C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.conette_decode_required_workspace_bytes.restype = C.c_size_t
    lib.conette_decode_required_workspace_bytes.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    lib.conette_decode_required.restype = C.c_int
    lib.conette_decode_required.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                            C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.conette_decode_ensemble_workspace_bytes.restype = C.c_size_t
    lib.conette_decode_ensemble_workspace_bytes.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    lib.conette_decode_ensemble.restype = C.c_int
    lib.conette_decode_ensemble.argtypes = [C.POINTER(ConetteMemberC), C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                            C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.conette_greedy_workspace_bytes.restype = C.c_size_t
    lib.conette_greedy_workspace_bytes.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
    lib.conette_greedy.restype = C.c_int
    lib.conette_greedy.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                   C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                   C.c_void_p]
    lib.conette_set_option.restype = C.c_int
    lib.conette_set_option.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    lib.conette_decode_graph_nodes.restype = C.c_int32
    lib.conette_decode_graph_nodes.argtypes = [C.c_void_p]
    lib.conette_profile_enable.restype = C.c_int
    lib.conette_profile_enable.argtypes = [C.c_void_p, C.c_uint32]
    lib.conette_profile_read.restype = C.c_int
    lib.conette_profile_read.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int32)]
    lib.conette_stream_create_masked.restype = C.c_int
    lib.conette_stream_create_masked.argtypes = [C.POINTER(C.c_uint32), C.c_int32, C.POINTER(C.c_void_p)]
    lib.conette_stream_destroy.restype = C.c_int
    lib.conette_stream_destroy.argtypes = [C.c_void_p]
    lib.conette_resample.restype = C.c_int
    lib.conette_resample.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    lib.conette_resample_len.restype = C.c_int32
    lib.conette_resample_len.argtypes = [C.c_int32, C.c_int32, C.c_int32]
    lib.conette_consensus.restype = C.c_int
    lib.conette_consensus.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                      C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.conette_tag_frames_workspace_bytes.restype = C.c_size_t
    lib.conette_tag_frames_workspace_bytes.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    lib.conette_tag_frames.restype = C.c_int
    lib.conette_tag_frames.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                       C.c_size_t, C.c_void_p]
    lib.conette_tag_events.restype = C.c_int
    lib.conette_tag_events.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_int32,
                                       C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.conette_decode_spans_workspace_bytes.restype = C.c_size_t
    lib.conette_decode_spans_workspace_bytes.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    lib.conette_decode_spans.restype = C.c_int
    lib.conette_decode_spans.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                         C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.conette_segments.restype = C.c_int
    lib.conette_segments.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                     C.c_int32, C.c_float, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    if lib.conette_abi_version() != 3:
        raise RuntimeError("libconette_hip.so ABI version mismatch")
    _lib = lib
    return lib


def _check(status: int, what: str) -> None:
    if status != 0:
        raise RuntimeError(f"{what} failed ({status}): {load_library().conette_last_error().decode()}")


def _stream() -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t: Optional[torch.Tensor]) -> C.c_void_p:
    return C.c_void_p(0 if t is None else t.data_ptr())


def encoder_geometry(n_samples: int) -> Tuple[int, list, list]:
    """(F, H[4], W[4]) -- SURVEY.md A.6."""
    f = n_samples // 320 + 1
    h = [(f + 8 - 4) // 4 + 1]
    w = [56]
    for _ in range(3):
        h.append(h[-1] // 2)
        w.append(w[-1] // 2)
    return f, h, w


def make_partitioned_streams(device: torch.device, decode_share: int = 8, n_cus: int = 256):
    """(encode_stream, decode_stream): the decode stream owns every ``decode_share``-th CU-mask bit
    (1/decode_share of the chip), the encode stream the complement.  Returns torch ExternalStreams."""
    lib = load_library()
    words = (n_cus + 31) // 32
    dec = [0] * words
    for i in range(0, n_cus, decode_share):
        dec[i // 32] |= 1 << (i % 32)
    enc = [(~w) & 0xFFFFFFFF for w in dec]
    out = []
    with torch.cuda.device(device):
        for mask in (enc, dec):
            h = C.c_void_p()
            _check(lib.conette_stream_create_masked((C.c_uint32 * words)(*mask), words, C.byref(h)),
                   "conette_stream_create_masked")
            out.append(torch.cuda.ExternalStream(h.value, device=device))
    return out[0], out[1]


def make_masked_stream(device: torch.device, n_share: int, n_cus: int = 256, offset: int = 0):
    """A stream whose kernels run on ``n_share`` of the ``n_cus`` compute units only: mask bits ``offset .. offset + n_share - 1``.
    On MI355X bit i of the mask is compute unit i // 8 of XCD i % 8 (measured: tools/lab/cumask_probe.hip), so a contiguous run
    of bits takes the same n_share / 8 compute units on every XCD; an XCD whose bits are all clear is left UNRESTRICTED by the
    driver (a mask of every 8th bit therefore restricts nothing).  A decode chain confined this way never holds a compute unit
    one of the encoder's persistent kernels is waiting for, while the encoder's own stream stays unrestricted."""
    lib = load_library()
    words = (n_cus + 31) // 32
    mask = [0] * words
    for j in range(n_share):
        i = (offset + j) % n_cus
        mask[i // 32] |= 1 << (i % 32)
    with torch.cuda.device(device):
        h = C.c_void_p()
        _check(lib.conette_stream_create_masked((C.c_uint32 * words)(*mask), words, C.byref(h)), "conette_stream_create_masked")
        return torch.cuda.ExternalStream(h.value, device=device)


def uncertified_mask(margins: torch.Tensor, best_lprobs: torch.Tensor, tol: Tuple[float, float, float], order: bool = True) -> torch.Tensor:
    """(B,) bool, True = the 16-bit search of this clip is NOT certified to have taken an exact search's decisions: some top-k call of
    step i has a margin below ``a + b * (i + 1)``, or the final best-beam choice one below ``c``, or a score / margin is not finite
    (NaN: fewer finite candidates than picks, or an fp16 residual-stream overflow).  ``margins`` (B, 2, max_pred + 1) as conette_decode
    writes them (include/conette_hip.h): plane 0 membership (+ the final choice in its last column), plane 1 pick order; ``order`` also
    holds the ORDER plane to the tolerance: with it the slot tables (mult_preds / mult_lprobs, in order) are certified, without it
    best_preds / best_lprobs and mult_preds as a SET of hypotheses.  ``tol`` = (a, b, c).  Pure tensor logic (CPU-testable)."""
    a, b, c = tol
    max_pred = margins.shape[2] - 1
    need = a + b * torch.arange(1, max_pred + 1, device=margins.device, dtype=torch.float32)
    ok = (margins[:, 0, :max_pred] >= need).all(dim=1) & (margins[:, 0, max_pred] >= c) & torch.isfinite(best_lprobs)
    if order:
        ok = ok & (margins[:, 1, :max_pred] >= need).all(dim=1)
    return ~ok


def caption_sizes(best_preds: torch.Tensor, mult_preds: torch.Tensor, eos_id: int) -> torch.Tensor:
    """[pred_size, best_maxlen] (beam.py:192-194,207-211,222-225) recomputed from full-width ids -- after rows of two searches have
    been merged.  A hypothesis ends at its first <eos>, or at max_pred when it never emitted one.  Pure tensor logic (CPU-testable)."""
    max_pred = mult_preds.shape[-1]
    pos = torch.arange(max_pred, device=mult_preds.device)

    def first_eos(x):   # index of the first <eos>, max_pred where absent
        return torch.where(x == eos_id, pos, max_pred).amin(dim=-1)

    ps = torch.clamp(first_eos(mult_preds) + 1, max=max_pred).amax()
    e = first_eos(best_preds)
    ml = torch.minimum(torch.where(e < ps, e, ps).amax() + 1, ps)
    return torch.stack([ps, ml]).to(torch.int32)


class Engine:
    """Opaque context (packed weights) + caller-owned workspaces for one device."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], *, precision: str = "bf16", d_model: int = 256,
                 nhead: int = 8, n_layers: int = 6, d_ff: int = 2048, pad_id: int = 0, bos_id: int = 1,
                 eos_id: int = 2, device: Optional[torch.device] = None) -> None:
        if not torch.cuda.is_available():
            raise RuntimeError("conette_amd.Engine needs a ROCm GPU (no CPU fallback)")
        self.lib = load_library()
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        table = {"fp32": PREC_F32, "f32": PREC_F32, "bf16": PREC_BF16, "exact": PREC_F16X2, "f16x2": PREC_F16X2,
                 "f16": PREC_F16, "fp16": PREC_F16}
        # "certified" (round 6): a 16-bit base precision for every clip + the device-side margins of its search (conette_decode's
        # `margins`); clips whose margins do not certify their ids are re-run through an exact context.  "certified" alone picks
        # CERT_DEFAULT_BASE; "certified:<base>" names it; "certified-best[:<base>]" relaxes the slot order (below).
        head = precision.split(":", 1)[0]
        self.certified = head in ("certified", "certified-best")
        # "certified": ids, candidates AND their slot order (mult_preds) are the exact search's; "certified-best": the returned
        # caption (best_preds / best_lprobs) and the SET of beam hypotheses are -- the pick-order margins are not held to the
        # tolerance, so two hypotheses of near-equal score may swap slots; far fewer clips need the exact re-run under beam search
        self.cert_order = head != "certified-best"
        base = precision
        if self.certified:
            base = precision.split(":", 1)[1] if ":" in precision else CERT_DEFAULT_BASE
            if base not in CERT_TOL:
                raise ValueError(f"certified: unknown base precision {base!r} (expected one of {tuple(CERT_TOL)})")
        self.base_precision = base
        if base == "mixed":     # bf16 encoder + exact (fp16 hi/lo pairs) decoder
            self.precision, self.precision_dec = PREC_BF16, PREC_F16X2
        elif base == "mixed16":  # fp16 encoder + exact decoder
            self.precision, self.precision_dec = PREC_F16, PREC_F16X2
        elif base == "bf16+f16dec":  # bf16 encoder (the throughput mode's) + fp16 decoder: the decoder's operands flip the most captions
            self.precision, self.precision_dec = PREC_BF16, PREC_F16
        else:
            if base not in table:
                raise ValueError(f"unknown precision {precision!r}" + (" (the experimental fp8 precision was withdrawn in round 6: "
                                 "profiles/r06_notes.md section 3)" if base == "fp8" else f" (expected one of {sorted(table)}, mixed, mixed16, "
                                 "bf16+f16dec, certified[:base])"))
            self.precision = self.precision_dec = table[base]
        self.precision_name = precision if (self.certified or base in ("mixed", "mixed16", "bf16+f16dec")) else {
            PREC_BF16: "bf16", PREC_F32: "fp32", PREC_F16X2: "exact", PREC_F16: "f16"}[self.precision]
        self.eos_id, self.pad_id = int(eos_id), int(pad_id)
        vocab = int(state_dict["model.decoder.classifier.weight"].shape[0])
        self.vocab_size = vocab
        self.d_model, self.nhead, self.n_layers, self.d_ff = d_model, nhead, n_layers, d_ff
        keep, names, ptrs, numel = [], [], [], []
        with torch.cuda.device(self.device):
            for k, v in state_dict.items():
                if not isinstance(v, torch.Tensor) or k == "_extra_state_":
                    continue
                if v.dtype == torch.bool:
                    v = v.to(torch.uint8)
                elif v.is_floating_point():
                    v = v.to(torch.float32)
                v = v.to(self.device).contiguous()
                keep.append(v)
                names.append(k.encode())
                ptrs.append(v.data_ptr())
                numel.append(v.numel())
            n = len(names)

            def create(prec: int) -> C.c_void_p:
                cfg = ConetteConfigC(prec, vocab, d_model, nhead, n_layers, d_ff, pad_id, bos_id, eos_id)
                handle = C.c_void_p()
                torch.cuda.synchronize(self.device)
                st = self.lib.conette_create(C.byref(cfg), n, (C.c_char_p * n)(*names), (C.c_void_p * n)(*ptrs),
                                             (C.c_int64 * n)(*numel), C.byref(handle))
                _check(st, "conette_create")
                torch.cuda.synchronize(self.device)
                return handle

            self._ctx = create(self.precision)
            # "mixed": frame_embs (B, T, 768) fp32 is the interface between the two halves of the path, so the encoder and the
            # decoder may run at different precisions -- here the bf16 encoder (the throughput mode's) feeds an exact decoder
            self._ctx_dec = create(self.precision_dec) if self.precision_dec != self.precision else self._ctx
            # "certified": the exact context that re-runs the clips the margins do not certify (encoder + decoder; shared with
            # the base's decoder when that is exact already)
            self._ctx_x = None
            if self.certified:
                self._ctx_x = self._ctx_dec if self.precision_dec == PREC_F16X2 else create(PREC_F16X2)
        self.cert_stats = {"clips": 0, "recomputed": 0}
        self._ws: Dict[str, torch.Tensor] = {}
        self._dec_bufs: Dict[Any, Dict[str, Any]] = {}
        del keep

    def __del__(self) -> None:
        seen = []
        for c in (getattr(self, "_ctx", None), getattr(self, "_ctx_dec", None), getattr(self, "_ctx_x", None)):
            if c and all(c is not d for d in seen):
                seen.append(c)
                try:
                    self.lib.conette_destroy(c)
                except Exception:
                    pass
        self._ctx = self._ctx_dec = self._ctx_x = None

    def _workspace(self, key: str, nbytes: int) -> torch.Tensor:
        ws = self._ws.get(key)
        if ws is None or ws.numel() < nbytes:
            ws = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
            self._ws[key] = ws
        return ws

    # ---- a2 --------------------------------------------------------------------------------
    def frontend_logmel(self, wave: torch.Tensor) -> torch.Tensor:
        wave = wave.to(self.device, torch.float32).contiguous()
        b, l = wave.shape
        out = torch.empty((b, self.lib.conette_num_frames(l), N_MELS), dtype=torch.float32, device=self.device)
        _check(self.lib.conette_frontend_logmel(self._ctx, _ptr(wave), b, l, _ptr(out), _stream()), "frontend_logmel")
        return out

    # ---- a2-a7 -----------------------------------------------------------------------------
    def encode(self, wave: torch.Tensor, taps=False, out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
               slot: int = 0, exact: bool = False):
        """wave (B, L) fp32 on device -> frame_embs (B, T, 768), clip_probs (B, 527) [, taps dict].
        ``taps="blocks"`` additionally returns the output of every ConvNeXt block ("block0" .. "block17").
        ``slot`` selects the scratch workspace: encodes running concurrently on different streams need different slots.
        ``exact`` (certified engines only): run on the exact context that re-computes uncertified clips."""
        ctx = self._ctx
        if exact:
            if self._ctx_x is None:
                raise RuntimeError("encode(exact=True) needs a certified engine")
            ctx = self._ctx_x
        wave = wave.to(self.device, torch.float32).contiguous()
        b, l = wave.shape
        f, hs, ws_ = encoder_geometry(l)
        t = hs[3]
        if out is None:
            frame_embs = torch.empty((b, t, FEAT), dtype=torch.float32, device=self.device)
            clip = torch.empty((b, N_TAGS), dtype=torch.float32, device=self.device)
        else:
            frame_embs, clip = out
        need = self.lib.conette_encode_workspace_bytes(ctx, b, l)
        wsb = self._workspace(("xenc" if exact else "enc") + ("" if slot == 0 else str(slot)), need)
        tap_struct, tap_out = None, None
        if taps:
            dims = (96, 192, 384, 768)
            e = lambda *s: torch.empty(s, dtype=torch.float32, device=self.device)
            tap_out = {"logmel": e(b, f, N_MELS), "stem": e(b, hs[0], ws_[0], 96)}
            for i in range(4):
                tap_out[f"stage{i}_block0"] = e(b, hs[i], ws_[i], dims[i])
                tap_out[f"stage{i}"] = e(b, hs[i], ws_[i], dims[i])
                if i > 0:
                    tap_out[f"down{i}"] = e(b, hs[i], ws_[i], dims[i])
            tap_struct = EncodeTapsC()
            tap_struct.struct_bytes = C.sizeof(EncodeTapsC)
            tap_struct.logmel = tap_out["logmel"].data_ptr()
            tap_struct.stem = tap_out["stem"].data_ptr()
            for i in range(4):
                tap_struct.stage_block0[i] = tap_out[f"stage{i}_block0"].data_ptr()
                tap_struct.stage[i] = tap_out[f"stage{i}"].data_ptr()
                tap_struct.down[i] = tap_out[f"down{i}"].data_ptr() if i > 0 else 0
            if taps == "blocks":
                blk = 0
                for i, depth in enumerate((3, 3, 9, 3)):
                    for _ in range(depth):
                        tap_out[f"block{blk}"] = e(b, hs[i], ws_[i], dims[i])
                        tap_struct.block[blk] = tap_out[f"block{blk}"].data_ptr()
                        blk += 1
        st = self.lib.conette_encode(ctx, _ptr(wave), b, l, _ptr(frame_embs), _ptr(clip),
                                     C.byref(tap_struct) if tap_struct is not None else None, _ptr(wsb),
                                     wsb.numel(), _stream())
        _check(st, "conette_encode")
        if taps:
            return frame_embs, clip, tap_out
        return frame_embs, clip

    # ---- a9-a14 ----------------------------------------------------------------------------
    def _decode_buffers(self, b: int, t: int, beam: int, max_pred: int, s0: bool, trace: bool,
                        slot: int = 0, margins: bool = False, exact: bool = False,
                        spans: Optional[Tuple[int, int]] = None) -> Dict[str, Any]:
        """Persistent I/O buffers per shape (and pipeline slot): identical pointers let the library
        replay its hipGraph.  ``spans`` = (n_rec, t_rec): the buffers of decode_spans -- b spans of t frames, "fe" holds the
        recordings and "spans" the table."""
        key = (b, t, beam, max_pred, s0, trace, slot, margins, exact) + (() if spans is None else ("spans",) + tuple(spans))
        buf = self._dec_bufs.pop(key, None)
        if buf is not None:
            self._dec_bufs[key] = buf           # least recently used first: a hit moves to the back
        if buf is None:
            dev = self.device
            ldv = (self.vocab_size + 7) // 8 * 8
            e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
            buf = {
                "fe": e((b, t, FEAT) if spans is None else (spans[0], spans[1], FEAT), torch.float32),
                "lens": e((b,), torch.int32), "spans": None if spans is None else e((b, 3), torch.int32), "bos": e((b,), torch.int32),
                "forbid": e((self.vocab_size,), torch.uint8),
                "best_preds": e((b, max_pred), torch.int32), "best_lprobs": e((b,), torch.float32),
                "mult_preds": e((b, beam, max_pred), torch.int32), "mult_lprobs": e((b, beam), torch.float32),
                "sizes": e((2,), torch.int32),
                "step0": e((b * beam, ldv), torch.float32) if s0 else None,
                "trace_sel": e((max_pred, b, beam, 2), torch.int32) if trace else None,
                "trace_val": e((max_pred, b, beam), torch.float32) if trace else None,
                "margins": e((b, 2, max_pred + 1), torch.float32) if margins else None,
            }
            if len(self._dec_bufs) >= MAX_DECODE_GRAPHS:
                # the evicted buffers may still be written by a decode running on another stream: drain before they are freed
                torch.cuda.synchronize(self.device)
                self._dec_bufs.pop(next(iter(self._dec_bufs)))
            self._dec_bufs[key] = buf
        return buf

    def decode(self, frame_embs: torch.Tensor, frame_lens: torch.Tensor, bos_ids: torch.Tensor,
               forbid_mask: Optional[torch.Tensor], beam: int, min_pred: int, max_pred: int,
               want_step0_logits: bool = False, want_trace: bool = False, clone: bool = True,
               slot: int = 0, want_margins: bool = False, exact: bool = False) -> Dict[str, torch.Tensor]:
        """Beam search over pre-computed frame embeddings.  Outputs are full width; trim with
        ``sizes`` = [pred_size, best_maxlen].  ``clone=False`` returns the persistent buffers of
        pipeline ``slot`` (two slots let the decode of batch i overlap the encode of batch i+1).
        ``want_margins``: also ``margins`` (B, 2, max_pred + 1), the per-decision margins of the search -- plane 0 membership (+ the
        final choice in its last column), plane 1 pick order (include/conette_hip.h).
        ``exact`` (certified engines only): run on the exact context."""
        ctx = self._ctx_dec
        if exact:
            if self._ctx_x is None:
                raise RuntimeError("decode(exact=True) needs a certified engine")
            ctx = self._ctx_x
        b, t, _ = frame_embs.shape
        buf = self._decode_buffers(b, t, int(beam), int(max_pred), want_step0_logits, want_trace, slot, want_margins, exact)
        if frame_embs.data_ptr() != buf["fe"].data_ptr():
            buf["fe"].copy_(frame_embs, non_blocking=True)
        buf["lens"].copy_(frame_lens.to(torch.int32), non_blocking=True)
        buf["bos"].copy_(bos_ids.to(torch.int32), non_blocking=True)
        forbid_ptr = None
        if forbid_mask is not None:
            if forbid_mask.numel() != self.vocab_size:
                raise ValueError("forbid_mask must have vocab_size entries")
            buf["forbid"].copy_(forbid_mask.to(torch.uint8), non_blocking=True)
            forbid_ptr = buf["forbid"]
        need = self.lib.conette_decode_workspace_bytes(ctx, b, t, beam, max_pred)
        # per slot: decodes of different slots may run on different streams
        wsb = self._workspace(("xdec" if exact else "dec") + ("" if slot == 0 else str(slot)), need)
        st = self.lib.conette_decode(ctx, _ptr(buf["fe"]), _ptr(buf["lens"]), _ptr(buf["bos"]), _ptr(forbid_ptr),
                                     b, t, beam, min_pred, max_pred, _ptr(buf["best_preds"]), _ptr(buf["best_lprobs"]),
                                     _ptr(buf["mult_preds"]), _ptr(buf["mult_lprobs"]), _ptr(buf["sizes"]),
                                     _ptr(buf["step0"]), _ptr(buf["trace_sel"]), _ptr(buf["trace_val"]), _ptr(buf["margins"]),
                                     _ptr(wsb), wsb.numel(), _stream())
        _check(st, "conette_decode")
        cp = (lambda x: x.clone()) if clone else (lambda x: x)
        out = {k: cp(buf[k]) for k in ("best_preds", "best_lprobs", "mult_preds", "mult_lprobs", "sizes")}
        if want_step0_logits:
            out["step0_logits"] = cp(buf["step0"])[:, : self.vocab_size]
        if want_trace:
            out["trace_sel"] = cp(buf["trace_sel"])
            out["trace_val"] = cp(buf["trace_val"])
        if want_margins:
            out["margins"] = cp(buf["margins"])
        return out

    # ---- the id certificate (round 6) ------------------------------------------------------------------------------------
    def uncertified(self, margins: torch.Tensor, best_lprobs: torch.Tensor, tol: Optional[Tuple[float, float, float]] = None,
                    beam: int = 2, order: Optional[bool] = None) -> torch.Tensor:
        """``uncertified_mask`` with the engine's defaults: ``tol`` = ``CERT_TOL[base precision][cert_kind(beam)]`` (measured:
        tools/calibrate_margins.py, profiles/r06_margin_calibration*.txt), ``order`` = the engine's policy (True for "certified",
        False for "certified-best")."""
        tol = CERT_TOL[self.base_precision][cert_kind(beam)] if tol is None else tol
        return uncertified_mask(margins, best_lprobs, tol, self.cert_order if order is None else order)

    def caption_sizes(self, best_preds: torch.Tensor, mult_preds: torch.Tensor) -> torch.Tensor:
        return caption_sizes(best_preds, mult_preds, self.eos_id)

    def generate_certified(self, wave: Optional[torch.Tensor], frame_embs: torch.Tensor, frame_lens: torch.Tensor,
                           bos_ids: torch.Tensor, forbid_mask: Optional[torch.Tensor], beam: int, min_pred: int,
                           max_pred: int, tol: Optional[Tuple[float, float, float]] = None) -> Dict[str, torch.Tensor]:
        """The certified search: the base precision's search of every clip with margins; the clips it does not certify are
        compacted into one batch and re-run through the exact context -- from the waveform (``wave`` (B, L), the padded batch
        the embeddings came from: exact encoder + exact decoder) or, when ``wave`` is None (the caller gave embeddings:
        ``preprocess=False``, BaselinePLM), from the same embeddings (exact decoder) -- and scattered back.  One host
        round trip per BATCH (the number of such clips sizes the second launch), none per search step.
        Returns decode()'s dict + ``recomputed`` (B,) bool."""
        if not self.certified:
            raise RuntimeError("generate_certified needs Engine(precision='certified[:base]')")
        res = self.decode(frame_embs, frame_lens, bos_ids, forbid_mask, beam, min_pred, max_pred, want_margins=True)
        flag = self.uncertified(res["margins"], res["best_lprobs"], tol, beam)
        if wave is None and self.precision_dec == PREC_F16X2:
            flag = torch.zeros_like(flag)   # given embeddings + an exact decoder already: nothing a re-run could change
        idx = torch.nonzero(flag).flatten()
        n = int(idx.numel())            # (the host round trip)
        b = int(frame_embs.shape[0])
        self.cert_stats["clips"] += b
        self.cert_stats["recomputed"] += n
        res["recomputed"] = flag
        if n == 0:
            return res
        lens_d = frame_lens.to(self.device)
        bos_d = bos_ids.to(self.device)
        if wave is not None:
            fe_x, clip_x = self.encode(wave.index_select(0, idx), exact=True)
            res["recomputed_idx"], res["recomputed_clip_probs"] = idx, clip_x    # (the exact encoder's tag probabilities of those clips)
        else:
            fe_x = frame_embs.to(self.device).index_select(0, idx)
        rx = self.decode(fe_x, lens_d.index_select(0, idx), bos_d.index_select(0, idx), forbid_mask, beam, min_pred, max_pred,
                         exact=True)
        for k in ("best_preds", "best_lprobs", "mult_preds", "mult_lprobs"):
            res[k].index_copy_(0, idx, rx[k])
        res["sizes"] = self.caption_sizes(res["best_preds"], res["mult_preds"])
        return res

    def encode_nonfinite(self) -> int:
        """Positions whose LayerNorm statistics were not finite in the encodes of this process since the last call (the fp16
        residual stream of the 16-bit precisions overflowed: include/conette_hip.h); waits for the current stream."""
        n = C.c_int32(0)
        _check(self.lib.conette_encode_nonfinite(self._ctx, _stream(), C.byref(n)), "conette_encode_nonfinite")
        return int(n.value)

    def forcing(self, frame_embs: torch.Tensor, frame_lens: torch.Tensor, caps_in: torch.Tensor) -> torch.Tensor:
        """Teacher forcing (forcing.py:12-71): frame_embs (B, T, 768), caps_in (B, cap_len) ids right-padded with
        pad_id -> logits (B, cap_len, vocab) fp32."""
        b, t, _ = frame_embs.shape
        cap_len = int(caps_in.shape[1])
        fe = frame_embs.to(self.device, torch.float32).contiguous()
        lens = frame_lens.to(self.device, torch.int32).contiguous()
        caps = caps_in.to(self.device, torch.int32).contiguous()
        out = torch.empty((b, cap_len, self.vocab_size), dtype=torch.float32, device=self.device)
        need = self.lib.conette_forcing_workspace_bytes(self._ctx_dec, b, t, cap_len)
        wsb = self._workspace("dec", need)
        st = self.lib.conette_forcing(self._ctx_dec, _ptr(fe), _ptr(lens), _ptr(caps), b, t, cap_len, _ptr(out), _ptr(wsb),
                                      wsb.numel(), _stream())
        _check(st, "conette_forcing")
        return out

    def score(self, frame_embs: torch.Tensor, frame_lens: torch.Tensor, caps_in: torch.Tensor, targets: torch.Tensor,
              caps_per_audio: int = 1, want_tokens: bool = True) -> Dict[str, Optional[torch.Tensor]]:
        """Log-likelihoods of given captions (conette_score, include/conette_hip.h): frame_embs (N, T, 768), caps_in / targets
        (N * caps_per_audio, cap_len) ids (scoring.split_captions; caption p belongs to clip p // caps_per_audio) ->
        {"tok_lprobs": (P, cap_len) fp32 or None, "sum_lprobs": (P,) fp32, "n_tokens": (P,) int32}.  No logits are written.
        ``caps_in`` is held to [0, vocab) before the call (the embedding lookup trusts it; skipped while the stream is being
        captured, where nothing may be read back).  A call whose workspace would exceed ``score_workspace_bound`` bytes
        (default scoring.SCORE_WORKSPACE_BOUND, 1 GiB) runs as several calls over clips -- or, when one clip's captions alone
        exceed it, over slices of its captions -- with equal results."""
        from . import scoring
        n, t, _ = frame_embs.shape
        cpa, cap_len = int(caps_per_audio), int(caps_in.shape[1])
        if cpa < 1 or caps_in.ndim != 2 or tuple(caps_in.shape) != tuple(targets.shape) or caps_in.shape[0] != n * cpa:
            raise ValueError(f"score: caps_in {tuple(caps_in.shape)} / targets {tuple(targets.shape)} do not hold "
                             f"{n} x {cpa} captions of one length")
        if not torch.cuda.is_current_stream_capturing() and caps_in.numel() > 0:
            lo, hi = int(caps_in.min()), int(caps_in.max())
            if lo < 0 or hi >= self.vocab_size:
                raise ValueError(f"score: caps_in ids must lie in [0, {self.vocab_size}), found [{lo}, {hi}]")
        fe = frame_embs.to(self.device, torch.float32).contiguous()
        lens = frame_lens.to(self.device, torch.int32).contiguous()
        caps = caps_in.to(self.device, torch.int32).contiguous()
        tgt = targets.to(self.device, torch.int32).contiguous()
        p = n * cpa
        tok = torch.empty((p, cap_len), dtype=torch.float32, device=self.device) if want_tokens else None
        sums = torch.empty((p,), dtype=torch.float32, device=self.device)
        cnt = torch.empty((p,), dtype=torch.int32, device=self.device)
        ctx = self._ctx_dec
        # (0 = more rows than one call takes: never fits)
        need = lambda nc, mc: int(self.lib.conette_score_workspace_bytes(ctx, nc, t, mc, cap_len)) or (1 << 62)
        bound = int(getattr(self, "score_workspace_bound", scoring.SCORE_WORKSPACE_BOUND))
        for i0, nc, j0, mc in scoring.plan_chunks(n, cpa, need, bound):
            if mc == cpa:     # whole clips: their captions are one contiguous run of rows
                rows = slice(i0 * cpa, (i0 + nc) * cpa)
            else:             # a slice of one clip's captions
                rows = slice(i0 * cpa + j0, i0 * cpa + j0 + mc)
            wsb = self._workspace("score", need(nc, mc))
            st = self.lib.conette_score(ctx, _ptr(fe[i0:i0 + nc]), _ptr(lens[i0:i0 + nc]), _ptr(caps[rows]), _ptr(tgt[rows]), nc, t, mc,
                                        cap_len, _ptr(None if tok is None else tok[rows]), _ptr(sums[rows]), _ptr(cnt[rows]),
                                        _ptr(wsb), wsb.numel(), _stream())
            _check(st, "conette_score")
        return {"tok_lprobs": tok, "sum_lprobs": sums, "n_tokens": cnt}

    def align(self, frame_embs: torch.Tensor, frame_lens: torch.Tensor, caps_in: torch.Tensor,
              targets: Optional[torch.Tensor] = None, caps_per_audio: int = 1, layers=None,
              per_layer: bool = False) -> Dict[str, Optional[torch.Tensor]]:
        """Where in the clip each caption position listens (conette_align, include/conette_hip.h): the head-mean cross-attention of
        the one-pass decoder, averaged over ``layers`` (decoder layer indices; None = all).  Inputs as in ``score``; ``targets``
        is optional -- without it the classifier does not run and the three score entries are None.  Returns {"attn": (P, cap_len,
        T) fp32 -- row t belongs to the position that predicts targets[:, t]; exactly 0 behind the clip's length and in rows of
        pad inputs --, "attn_layers": (n_layers, P, cap_len, T) when ``per_layer`` else None, "tok_lprobs", "sum_lprobs",
        "n_tokens": ``score``'s, bit for bit}.  The id check and the chunking by ``score_workspace_bound`` are ``score``'s."""
        from . import scoring
        n, t, _ = frame_embs.shape
        cpa, cap_len = int(caps_per_audio), int(caps_in.shape[1])
        if cpa < 1 or caps_in.ndim != 2 or caps_in.shape[0] != n * cpa or (targets is not None and tuple(caps_in.shape) != tuple(targets.shape)):
            raise ValueError(f"align: caps_in {tuple(caps_in.shape)}" + ("" if targets is None else f" / targets {tuple(targets.shape)}") +
                             f" do not hold {n} x {cpa} captions of one length")
        mask = 0
        for l in (() if layers is None else layers):
            if not 0 <= int(l) < self.n_layers:
                raise ValueError(f"align: layer {l} outside [0, {self.n_layers})")
            mask |= 1 << int(l)
        if layers is not None and mask == 0:
            raise ValueError("align: no layer selected")
        if not torch.cuda.is_current_stream_capturing() and caps_in.numel() > 0:
            lo, hi = int(caps_in.min()), int(caps_in.max())
            if lo < 0 or hi >= self.vocab_size:
                raise ValueError(f"align: caps_in ids must lie in [0, {self.vocab_size}), found [{lo}, {hi}]")
        fe = frame_embs.to(self.device, torch.float32).contiguous()
        lens = frame_lens.to(self.device, torch.int32).contiguous()
        caps = caps_in.to(self.device, torch.int32).contiguous()
        tgt = None if targets is None else targets.to(self.device, torch.int32).contiguous()
        p = n * cpa
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device=self.device)
        attn = e((p, cap_len, t), torch.float32)
        planes = e((self.n_layers, p, cap_len, t), torch.float32) if per_layer else None
        tok = e((p, cap_len), torch.float32) if tgt is not None else None
        sums = e((p,), torch.float32) if tgt is not None else None
        cnt = e((p,), torch.int32) if tgt is not None else None
        ctx = self._ctx_dec
        need = lambda nc, mc: int(self.lib.conette_align_workspace_bytes(ctx, nc, t, mc, cap_len, int(tgt is not None))) or (1 << 62)
        bound = int(getattr(self, "score_workspace_bound", scoring.SCORE_WORKSPACE_BOUND))
        sl = lambda x, rows: None if x is None else x[rows]
        for i0, nc, j0, mc in scoring.plan_chunks(n, cpa, need, bound):
            rows = slice(i0 * cpa, (i0 + nc) * cpa) if mc == cpa else slice(i0 * cpa + j0, i0 * cpa + j0 + mc)
            whole = rows.stop - rows.start == p
            part = planes if (planes is None or whole) else e((self.n_layers, rows.stop - rows.start, cap_len, t), torch.float32)
            wsb = self._workspace("score", need(nc, mc))
            st = self.lib.conette_align(ctx, _ptr(fe[i0:i0 + nc]), _ptr(lens[i0:i0 + nc]), _ptr(caps[rows]), _ptr(sl(tgt, rows)), nc, t,
                                        mc, cap_len, mask, _ptr(attn[rows]), _ptr(part), _ptr(sl(tok, rows)), _ptr(sl(sums, rows)),
                                        _ptr(sl(cnt, rows)), _ptr(wsb), wsb.numel(), _stream())
            _check(st, "conette_align")
            if part is not planes:   # (a chunk's planes are (n_layers, its rows, ...): copied into place)
                planes[:, rows].copy_(part)
        return {"attn": attn, "attn_layers": planes, "tok_lprobs": tok, "sum_lprobs": sums, "n_tokens": cnt}

    def set_score_vsplit(self, slabs: int) -> None:
        """Vocabulary slabs of conette_score's fused kernel: 0 = chosen from the row count (default), k >= 1 = k (clamped)."""
        _check(self.lib.conette_set_option(self._ctx_dec, OPT_SCORE_VSPLIT, int(slabs)), "set_option")

    def greedy(self, frame_embs: torch.Tensor, frame_lens: torch.Tensor, bos_ids: torch.Tensor,
               forbid_mask: Optional[torch.Tensor], min_pred: int, max_pred: int) -> Dict[str, torch.Tensor]:
        """greedy_search (greedy.py:17-131): {"logits": (B, pred_size, vocab) masked step logits, "preds": (B, pred_size)}."""
        b, t, _ = frame_embs.shape
        fe = frame_embs.to(self.device, torch.float32).contiguous()
        lens = frame_lens.to(self.device, torch.int32).contiguous()
        bos = bos_ids.to(self.device, torch.int32).contiguous()
        fm = None if forbid_mask is None else forbid_mask.to(self.device, torch.uint8).contiguous()
        logits = torch.empty((b, max_pred, self.vocab_size), dtype=torch.float32, device=self.device)
        preds = torch.empty((b, max_pred), dtype=torch.int32, device=self.device)
        sizes = torch.zeros((2,), dtype=torch.int32, device=self.device)
        need = self.lib.conette_greedy_workspace_bytes(self._ctx_dec, b, t, max_pred)
        wsb = self._workspace("dec", need)
        st = self.lib.conette_greedy(self._ctx_dec, _ptr(fe), _ptr(lens), _ptr(bos), _ptr(fm), b, t, int(min_pred), int(max_pred),
                                     _ptr(logits), _ptr(preds), _ptr(sizes), _ptr(wsb), wsb.numel(), _stream())
        _check(st, "conette_greedy")
        ps = int(sizes[0].item())
        return {"logits": logits[:, :ps].contiguous(), "preds": preds[:, :ps].contiguous()}

    def sample(self, frame_embs: torch.Tensor, frame_lens: torch.Tensor, bos_ids: torch.Tensor,
               forbid_mask: Optional[torch.Tensor], n_samples: int, min_pred: int, max_pred: int, temperature: float = 1.0,
               top_k: int = 0, top_p: float = 1.0, uniforms: Optional[torch.Tensor] = None,
               generator: Optional[torch.Generator] = None, want_tokens: bool = False,
               want_logits: bool = False) -> Dict[str, torch.Tensor]:
        """``n_samples`` captions per clip drawn from the model's distribution (conette_sample, include/conette_hip.h; the rule:
        sampling.py): {"preds": (B, n, max_pred) int32 with pad_id after the end, "sum_lprobs": (B, n), "lens": (B, n) int32,
        "sizes": (2,) int32 [, "tok_lprobs": (B, n, max_pred)] [, "step_logits": (B, n, max_pred, vocab), the raw logits each
        decision saw]}.  ``uniforms`` (max_pred, B, n) fp32 in [0, 1) are drawn with ``torch.rand(..., generator=generator)`` on
        the device when none are passed; more than 16 samples per clip run as several calls (sampling.plan_sample_chunks), sample
        j reading column j of the uniforms."""
        from . import sampling
        b, t, _ = frame_embs.shape
        n, max_pred = int(n_samples), int(max_pred)
        plan = sampling.plan_sample_chunks(n)
        if uniforms is None:
            uniforms = torch.rand((max_pred, b, n), dtype=torch.float32, device=self.device, generator=generator)
        if tuple(uniforms.shape) != (max_pred, b, n):
            raise ValueError(f"sample: uniforms {tuple(uniforms.shape)} are not (max_pred, batch, n_samples) = {(max_pred, b, n)}")
        uni = uniforms.to(self.device, torch.float32)
        fe = frame_embs.to(self.device, torch.float32).contiguous()
        lens_in = frame_lens.to(self.device, torch.int32).contiguous()
        bos = bos_ids.to(self.device, torch.int32).contiguous()
        fm = None
        if forbid_mask is not None:
            if forbid_mask.numel() != self.vocab_size:
                raise ValueError("forbid_mask must have vocab_size entries")
            fm = forbid_mask.to(self.device, torch.uint8).contiguous()
        ctx = self._ctx_dec
        parts = []
        for first, cnt in plan:
            e = lambda shape, dt: torch.empty(shape, dtype=dt, device=self.device)
            o = {"preds": e((b, cnt, max_pred), torch.int32), "sum_lprobs": e((b, cnt), torch.float32),
                 "lens": e((b, cnt), torch.int32), "sizes": e((2,), torch.int32),
                 "tok_lprobs": e((b, cnt, max_pred), torch.float32) if want_tokens else None,
                 "step_logits": e((b, cnt, max_pred, self.vocab_size), torch.float32) if want_logits else None}
            u = uni[:, :, first:first + cnt].contiguous()
            need = self.lib.conette_sample_workspace_bytes(ctx, b, t, cnt, max_pred)
            wsb = self._workspace("dec", need)
            st = self.lib.conette_sample(ctx, _ptr(fe), _ptr(lens_in), _ptr(bos), _ptr(fm), _ptr(u), b, t, cnt, int(min_pred),
                                         max_pred, float(temperature), int(top_k), float(top_p), _ptr(o["preds"]),
                                         _ptr(o["sum_lprobs"]), _ptr(o["lens"]), _ptr(o["sizes"]), _ptr(o["tok_lprobs"]),
                                         _ptr(o["step_logits"]), _ptr(wsb), wsb.numel(), _stream())
            _check(st, "conette_sample")
            parts.append(o)
        if len(parts) == 1:
            return {k: v for k, v in parts[0].items() if v is not None}
        out = {k: torch.cat([p[k] for p in parts], dim=1) for k in ("preds", "sum_lprobs", "lens", "tok_lprobs", "step_logits")
               if parts[0][k] is not None}
        out["sizes"] = torch.stack([p["sizes"] for p in parts]).amax(dim=0)
        return out

    def decode_groups(self, frame_embs: torch.Tensor, frame_lens: torch.Tensor, bos_ids: torch.Tensor,
                      forbid_mask: Optional[torch.Tensor], n_groups: int, group_beam: int, diversity_penalty: float, min_pred: int,
                      max_pred: int, want_trace: bool = False, want_logits: bool = False) -> Dict[str, torch.Tensor]:
        """Diverse beam search (conette_decode_groups, include/conette_hip.h; the rule: group_search.py): ``n_groups`` groups of
        ``group_beam`` beams per clip, a group's candidates paying ``diversity_penalty`` for each time their token was already
        picked at this step by an earlier group.  Returns ``decode``'s outputs at beam G * W -- "best_preds", "best_lprobs",
        "mult_preds" (B, G * W, max_pred) and "mult_lprobs" (B, G * W) in slot order, group-major, "sizes" -- [, "trace_sel"
        (max_pred, B, G * W, 2), "trace_val" (max_pred, B, G * W)] [, "step_logits" (max_pred, B * G * W, vocab), the raw logits
        each step decided on].  Scores are the model's averaged log-probabilities, never the penalised keys."""
        from . import group_search
        g, w = group_search.check_arguments(n_groups, group_beam, diversity_penalty)
        b, t, _ = frame_embs.shape
        max_pred, r = int(max_pred), b * g * w
        fe = frame_embs.to(self.device, torch.float32).contiguous()
        lens_in = frame_lens.to(self.device, torch.int32).contiguous()
        bos = bos_ids.to(self.device, torch.int32).contiguous()
        fm = None
        if forbid_mask is not None:
            if forbid_mask.numel() != self.vocab_size:
                raise ValueError("forbid_mask must have vocab_size entries")
            fm = forbid_mask.to(self.device, torch.uint8).contiguous()
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device=self.device)
        o = {"best_preds": e((b, max_pred), torch.int32), "best_lprobs": e((b,), torch.float32),
             "mult_preds": e((b, g * w, max_pred), torch.int32), "mult_lprobs": e((b, g * w), torch.float32),
             "sizes": e((2,), torch.int32),
             "trace_sel": e((max_pred, b, g * w, 2), torch.int32) if want_trace else None,
             "trace_val": e((max_pred, b, g * w), torch.float32) if want_trace else None,
             "step_logits": e((max_pred, r, self.vocab_size), torch.float32) if want_logits else None}
        ctx = self._ctx_dec
        need = self.lib.conette_decode_groups_workspace_bytes(ctx, b, t, g, w, max_pred)
        wsb = self._workspace("dec", need)
        st = self.lib.conette_decode_groups(ctx, _ptr(fe), _ptr(lens_in), _ptr(bos), _ptr(fm), b, t, g, w, float(diversity_penalty),
                                            int(min_pred), max_pred, _ptr(o["best_preds"]), _ptr(o["best_lprobs"]),
                                            _ptr(o["mult_preds"]), _ptr(o["mult_lprobs"]), _ptr(o["sizes"]), _ptr(o["trace_sel"]),
                                            _ptr(o["trace_val"]), _ptr(o["step_logits"]), _ptr(wsb), wsb.numel(), _stream())
        _check(st, "conette_decode_groups")
        return {k: v for k, v in o.items() if v is not None}

    def decode_ensemble(self, members, frame_lens: torch.Tensor, forbid_mask: Optional[torch.Tensor], beam: int, min_pred: int,
                        max_pred: int, combine: str = "logprob", want_trace: bool = False, want_logits: bool = False,
                        want_margins: bool = False, clone: bool = True) -> Dict[str, torch.Tensor]:
        """Ensemble beam search (conette_decode_ensemble, include/conette_hip.h; the rule: ensemble_search.py).  ``members``: a list
        of (engine, frame_embs (B, T, 768), bos_ids (B,), weight) -- the same engine may appear more than once (one checkpoint under
        several task tokens); the weights are normalised to sum 1 here.  The members decode one hypothesis tree in lockstep and the
        top-k runs on the combined scores (``combine`` "logprob": sum_m w_m lp_m; "prob": log sum_m w_m exp lp_m).  Returns
        ``decode``'s dict [, "trace_sel", "trace_val"] [, "margins"] [, "step_logits" (max_pred, M, B * beam, vocab): every member's
        raw logits as each step read them].  The I/O buffers and the members' workspaces are this engine's and persist per shape, so
        the library replays its hipGraph; ``clone=False`` returns those buffers."""
        from . import ensemble_search
        members = list(members)
        w64, rule = ensemble_search.check_arguments(len(members), [m[3] for m in members], combine, beam)
        m_n, beam, max_pred = len(members), int(beam), int(max_pred)
        b, t, _ = members[0][1].shape
        for eng, fe, bos, _ in members:
            if tuple(fe.shape) != (b, t, FEAT) or bos.numel() != b:
                raise ValueError("members: every frame_embs must be (B, T, 768) of one shape, every bos_ids (B,)")
            if eng.vocab_size != self.vocab_size or eng.eos_id != self.eos_id or eng.pad_id != self.pad_id:
                raise ValueError("members: the engines must share the vocabulary size and the eos / pad ids")
            if eng.precision_dec != members[0][0].precision_dec:
                raise ValueError("members: the engines' decoders must share one precision")
            if eng.device != self.device:
                raise ValueError(f"members: an engine on {eng.device} in an ensemble run on {self.device} (one device per ensemble)")
        key = ("ens", m_n, b, t, beam, max_pred, want_trace, want_logits, want_margins)
        buf = self._dec_bufs.pop(key, None)
        if buf is None:
            dev = self.device
            ldv = (self.vocab_size + 7) // 8 * 8
            e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
            buf = {"fe": [e((b, t, FEAT), torch.float32) for _ in range(m_n)], "bos": [e((b,), torch.int32) for _ in range(m_n)],
                   "lens": e((b,), torch.int32), "forbid": e((self.vocab_size,), torch.uint8),
                   "best_preds": e((b, max_pred), torch.int32), "best_lprobs": e((b,), torch.float32),
                   "mult_preds": e((b, beam, max_pred), torch.int32), "mult_lprobs": e((b, beam), torch.float32),
                   "sizes": e((2,), torch.int32),
                   "trace_sel": e((max_pred, b, beam, 2), torch.int32) if want_trace else None,
                   "trace_val": e((max_pred, b, beam), torch.float32) if want_trace else None,
                   "margins": e((b, 2, max_pred + 1), torch.float32) if want_margins else None,
                   "step_logits": e((max_pred, m_n, b * beam, ldv), torch.float32) if want_logits else None}
            if len(self._dec_bufs) >= MAX_DECODE_GRAPHS:
                torch.cuda.synchronize(self.device)     # (as _decode_buffers: the evicted buffers may still be in use)
                self._dec_bufs.pop(next(iter(self._dec_bufs)))
        self._dec_bufs[key] = buf
        recs = (ConetteMemberC * m_n)()
        for i, (eng, fe, bos, _) in enumerate(members):
            if fe.data_ptr() != buf["fe"][i].data_ptr():
                buf["fe"][i].copy_(fe, non_blocking=True)
            buf["bos"][i].copy_(bos.to(torch.int32), non_blocking=True)
            ctx = eng._ctx_dec
            need = self.lib.conette_decode_ensemble_workspace_bytes(ctx, b, t, beam, max_pred)
            wsb = self._workspace(f"ens{i}", need)
            recs[i] = ConetteMemberC(ctx, buf["fe"][i].data_ptr(), buf["bos"][i].data_ptr(), float(w64[i]), wsb.data_ptr(),
                                     wsb.numel())
        buf["lens"].copy_(frame_lens.to(torch.int32), non_blocking=True)
        forbid_ptr = None
        if forbid_mask is not None:
            if forbid_mask.numel() != self.vocab_size:
                raise ValueError("forbid_mask must have vocab_size entries")
            buf["forbid"].copy_(forbid_mask.to(torch.uint8), non_blocking=True)
            forbid_ptr = buf["forbid"]
        st = self.lib.conette_decode_ensemble(recs, m_n, rule, _ptr(buf["lens"]), _ptr(forbid_ptr), b, t, beam, int(min_pred), max_pred,
                                              _ptr(buf["best_preds"]), _ptr(buf["best_lprobs"]), _ptr(buf["mult_preds"]),
                                              _ptr(buf["mult_lprobs"]), _ptr(buf["sizes"]), _ptr(buf["trace_sel"]), _ptr(buf["trace_val"]),
                                              _ptr(buf["margins"]), _ptr(buf["step_logits"]), _stream())
        _check(st, "conette_decode_ensemble")
        cp = (lambda x: x.clone()) if clone else (lambda x: x)
        out = {k: cp(buf[k]) for k in ("best_preds", "best_lprobs", "mult_preds", "mult_lprobs", "sizes")}
        for k in ("trace_sel", "trace_val", "margins"):
            if buf[k] is not None:
                out[k] = cp(buf[k])
        if want_logits:
            out["step_logits"] = cp(buf["step_logits"])[..., : self.vocab_size]
        return out

    def decode_constrained(self, frame_embs: torch.Tensor, frame_lens: torch.Tensor, bos_ids: torch.Tensor,
                           forbid_mask: Optional[torch.Tensor], beam: int, min_pred: int, max_pred: int,
                           prefix: Optional[torch.Tensor] = None, prefix_lens: Optional[torch.Tensor] = None,
                           ban_mask: Optional[torch.Tensor] = None, no_repeat_ngram: int = 0, want_trace: bool = False,
                           want_logits: bool = False, exact: bool = False, check: bool = True) -> Dict[str, torch.Tensor]:
        """Constrained beam search (conette_decode_constrained, include/conette_hip.h; the rule: constrained_search.py): the beam
        search at ``beam`` whose captions begin with ``prefix`` (B, P) int [``prefix_lens`` (B,); None: every row is P long], never
        hold a token of ``ban_mask`` (vocab) and repeat no ``no_repeat_ngram``-gram.  Returns ``decode``'s outputs -- a void slot
        has ``mult_lprobs`` -inf and pad throughout -- [, "trace_sel" (max_pred, B, beam, 2), "trace_val" (max_pred, B, beam)]
        [, "step_logits" (max_pred, B * beam, vocab), the raw logits each step decided on].  ``check``: the prefix tokens are
        checked on the host (in the vocabulary, neither <eos> nor pad; a device prefix is copied back for it); ``exact``
        (certified engines only): run on the exact context."""
        return self._decode_steered("decode_constrained", frame_embs, frame_lens, bos_ids, forbid_mask, beam, min_pred, max_pred, prefix,
                                    prefix_lens, ban_mask, no_repeat_ngram, None, None, want_trace, want_logits, exact, check)

    def decode_required(self, frame_embs: torch.Tensor, frame_lens: torch.Tensor, bos_ids: torch.Tensor,
                        forbid_mask: Optional[torch.Tensor], beam: int, min_pred: int, max_pred: int,
                        prefix: Optional[torch.Tensor] = None, prefix_lens: Optional[torch.Tensor] = None,
                        ban_mask: Optional[torch.Tensor] = None, no_repeat_ngram: int = 0, req_tokens: Optional[torch.Tensor] = None,
                        req_groups: Optional[torch.Tensor] = None, want_trace: bool = False, want_logits: bool = False,
                        exact: bool = False, check: bool = True) -> Dict[str, torch.Tensor]:
        """Keyword-guided beam search (conette_decode_required, include/conette_hip.h; the rule: required_search.py):
        ``decode_constrained`` whose every caption holds a token of each of a clip's requirement groups.  ``req_tokens`` /
        ``req_groups`` (B, width <= 32) int: the clip's required tokens and the group 0 .. 7 of each, -1 = unused entry
        (``required_search.pack_tables``); both None: no requirement.  Outputs and switches as ``decode_constrained``; ``check``
        also holds the tables to ``required_search.check_requirements`` on the host."""
        if (req_tokens is None) != (req_groups is None):
            raise ValueError("req_tokens and req_groups must be given together")
        if req_tokens is None:
            req_tokens = req_groups = torch.zeros((frame_embs.shape[0], 0), dtype=torch.int32)
        return self._decode_steered("decode_required", frame_embs, frame_lens, bos_ids, forbid_mask, beam, min_pred, max_pred, prefix,
                                    prefix_lens, ban_mask, no_repeat_ngram, req_tokens, req_groups, want_trace, want_logits, exact, check)

    def _decode_steered(self, entry, frame_embs, frame_lens, bos_ids, forbid_mask, beam, min_pred, max_pred, prefix, prefix_lens,
                        ban_mask, no_repeat_ngram, req_tokens, req_groups, want_trace, want_logits, exact, check):
        """decode_constrained (``req_tokens`` None) and decode_required: one preparation, the entry ``conette_<entry>``"""
        from . import constrained_search, required_search
        b, t, _ = frame_embs.shape
        max_pred = int(max_pred)
        pw = 0 if prefix is None else int(prefix.shape[1])
        if prefix is not None and (prefix.dim() != 2 or prefix.shape[0] != b):
            raise ValueError(f"prefix must be (batch, P), got {tuple(prefix.shape)}")
        rw = 0
        if req_tokens is not None:
            if req_tokens.dim() != 2 or req_tokens.shape[0] != b or tuple(req_groups.shape) != tuple(req_tokens.shape):
                raise ValueError(f"req_tokens and req_groups must both be (batch, width), got {tuple(req_tokens.shape)} and "
                                 f"{tuple(req_groups.shape)}")
            rw = int(req_tokens.shape[1])
            w, n = required_search.check_arguments(beam, no_repeat_ngram, max_pred, pw, rw)
        else:
            w, n = constrained_search.check_arguments(beam, no_repeat_ngram, max_pred, pw)
        ctx = self._ctx_dec
        if exact:
            if self._ctx_x is None:
                raise RuntimeError(f"{entry}(exact=True) needs a certified engine")
            ctx = self._ctx_x
        pre = plens = None
        if pw > 0:
            if prefix_lens is None:
                prefix_lens = torch.full((b,), pw, dtype=torch.int32)
            if prefix_lens.numel() != b:
                raise ValueError("prefix_lens must have one entry per clip")
            if check:
                ph, lh = prefix.cpu().long(), prefix_lens.cpu().long()
                if bool(((lh < 0) | (lh > pw)).any()):
                    raise ValueError(f"prefix_lens must lie in 0 .. {pw}")
                live = ph[torch.arange(pw)[None] < lh[:, None]]
                if bool(((live < 0) | (live >= self.vocab_size) | (live == self.eos_id) | (live == self.pad_id)).any()):
                    raise ValueError("prefix tokens must lie in the vocabulary and be neither <eos> nor pad")
            pre = prefix.to(self.device, torch.int32).contiguous()
            plens = prefix_lens.to(self.device, torch.int32).contiguous()
        fe = frame_embs.to(self.device, torch.float32).contiguous()
        lens_in = frame_lens.to(self.device, torch.int32).contiguous()
        bos = bos_ids.to(self.device, torch.int32).contiguous()
        masks = []
        for name, m in (("forbid_mask", forbid_mask), ("ban_mask", ban_mask)):
            if m is not None and m.numel() != self.vocab_size:
                raise ValueError(f"{name} must have vocab_size entries")
            masks.append(None if m is None else m.to(self.device, torch.uint8).contiguous())
        fm, bm = masks
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device=self.device)
        o = {"best_preds": e((b, max_pred), torch.int32), "best_lprobs": e((b,), torch.float32),
             "mult_preds": e((b, w, max_pred), torch.int32), "mult_lprobs": e((b, w), torch.float32),
             "sizes": e((2,), torch.int32),
             "trace_sel": e((max_pred, b, w, 2), torch.int32) if want_trace else None,
             "trace_val": e((max_pred, b, w), torch.float32) if want_trace else None,
             "step_logits": e((max_pred, b * w, self.vocab_size), torch.float32) if want_logits else None}
        outs = (_ptr(o["best_preds"]), _ptr(o["best_lprobs"]), _ptr(o["mult_preds"]), _ptr(o["mult_lprobs"]), _ptr(o["sizes"]),
                _ptr(o["trace_sel"]), _ptr(o["trace_val"]), _ptr(o["step_logits"]))
        if req_tokens is None:
            need = self.lib.conette_decode_constrained_workspace_bytes(ctx, b, t, w, max_pred)
            wsb = self._workspace("xdec" if exact else "dec", need)
            st = self.lib.conette_decode_constrained(ctx, _ptr(fe), _ptr(lens_in), _ptr(bos), _ptr(fm), _ptr(pre), _ptr(plens), pw, _ptr(bm),
                                                     n, b, t, w, int(min_pred), max_pred, *outs, _ptr(wsb), wsb.numel(), _stream())
        else:
            rt = rg = None
            if rw > 0:
                if check:
                    self._check_req_tables(req_tokens, req_groups, bos_ids, prefix, prefix_lens, ban_mask, max_pred)
                rt = req_tokens.to(self.device, torch.int32).contiguous()
                rg = req_groups.to(self.device, torch.int32).contiguous()
            need = self.lib.conette_decode_required_workspace_bytes(ctx, b, t, w, max_pred)
            wsb = self._workspace("xdec" if exact else "dec", need)
            st = self.lib.conette_decode_required(ctx, _ptr(fe), _ptr(lens_in), _ptr(bos), _ptr(fm), _ptr(pre), _ptr(plens), pw, _ptr(bm),
                                                  n, _ptr(rt), _ptr(rg), rw, b, t, w, int(min_pred), max_pred, *outs, _ptr(wsb),
                                                  wsb.numel(), _stream())
        _check(st, "conette_" + entry)
        return {k: v for k, v in o.items() if v is not None}

    def _check_req_tables(self, req_tokens, req_groups, bos_ids, prefix, prefix_lens, ban_mask, max_pred) -> None:
        """the host check of decode_required: every clip's table against required_search.check_requirements"""
        from . import required_search
        th, gh, bos = req_tokens.cpu().long(), req_groups.cpu().long(), bos_ids.cpu().long()
        if bool(((gh < -1) | (gh >= required_search.MAX_GROUPS)).any()):
            raise ValueError(f"req_groups must lie in -1 .. {required_search.MAX_GROUPS - 1}")
        ban = None if ban_mask is None else ban_mask.cpu().bool().numpy()
        for i in range(th.shape[0]):
            used = sorted(set(gh[i][gh[i] >= 0].tolist()))
            groups = [[int(x) for x in th[i][gh[i] == g].tolist()] for g in used]
            pre = []
            if prefix is not None:
                n_pre = int(prefix.shape[1]) if prefix_lens is None else int(prefix_lens.reshape(-1)[i])
                pre = [int(x) for x in prefix[i, :n_pre].cpu().tolist()]
            required_search.check_requirements(groups, int(bos[i]), vocab_size=self.vocab_size, max_pred=max_pred, eos_id=self.eos_id,
                                               pad_id=self.pad_id, ban=ban, prefix=pre)

    def decode_input_buffer(self, b: int, t: int, beam: int, max_pred: int, slot: int = 0, margins: bool = False,
                            exact: bool = False) -> torch.Tensor:
        """The persistent (B, T, 768) input of decode() (of the call with the same ``want_margins`` / ``exact``): encode
        straight into it to skip a copy."""
        return self._decode_buffers(b, t, int(beam), int(max_pred), False, False, slot, margins, exact)["fe"]

    # ---- options / profiling ------------------------------------------------------------------
    def set_decode_graph(self, enabled: bool) -> None:
        _check(self.lib.conette_set_option(self._ctx_dec, OPT_DECODE_GRAPH, int(bool(enabled))), "set_option")

    def set_decode_fusion(self, enabled: bool) -> None:
        """bf16: fused decoder-layer kernels (default) or one launch per sub-layer (cross-check path)."""
        _check(self.lib.conette_set_option(self._ctx_dec, OPT_DECODE_FUSION, int(bool(enabled))), "set_option")

    def set_forcing_stepwise(self, enabled: bool) -> None:
        """Teacher forcing through the KV-cached step kernels (cross-check) instead of the one-pass kernels (default)."""
        _check(self.lib.conette_set_option(self._ctx_dec, OPT_FORCING_STEPWISE, int(bool(enabled))), "set_option")

    def set_encode_reserved_cus(self, n: int) -> None:
        """Compute units the encoder's persistent kernels leave free for a decode running on another stream."""
        _check(self.lib.conette_set_option(self._ctx, OPT_ENCODE_RESERVED_CUS, int(n)), "set_option")

    def decode_graph_nodes(self) -> int:
        """Kernel / copy nodes of the most recently captured decode hipGraph (0 before the first capture)."""
        return int(self.lib.conette_decode_graph_nodes(self._ctx_dec))

    _DEC_CLASSES = ("dec_prepare", "dec_gemm", "dec_attn", "dec_misc", "search")

    def profile_enable(self, classes=()) -> None:
        """Event pairs around the launches of these kernel classes.  In the two-context precisions (mixed, mixed16,
        bf16+f16dec) the encoder classes go to the encoder context and the decoder classes to the decoder context (which also
        makes its decode run eagerly instead of replaying a hipGraph, as in the one-context case)."""
        mask_enc = mask_dec = 0
        for c in classes:
            bit = 1 << PROF_CLASSES.index(c)
            if c in self._DEC_CLASSES:
                mask_dec |= bit
            else:
                mask_enc |= bit
        if self._ctx_dec is self._ctx:
            _check(self.lib.conette_profile_enable(self._ctx, mask_enc | mask_dec), "profile_enable")
        else:
            _check(self.lib.conette_profile_enable(self._ctx, mask_enc), "profile_enable")
            _check(self.lib.conette_profile_enable(self._ctx_dec, mask_dec), "profile_enable")

    def profile_read(self) -> Dict[str, Any]:
        n = len(PROF_CLASSES)
        ms = (C.c_float * n)()
        cnt = (C.c_int32 * n)()
        _check(self.lib.conette_profile_read(self._ctx, ms, cnt), "profile_read")   # (accumulates into ms / cnt)
        if self._ctx_dec is not self._ctx:
            _check(self.lib.conette_profile_read(self._ctx_dec, ms, cnt), "profile_read")
        return {PROF_CLASSES[i]: (float(ms[i]), int(cnt[i])) for i in range(n) if cnt[i] > 0}

    def consensus(self, preds: torch.Tensor, lens: Optional[torch.Tensor] = None, weights: Optional[torch.Tensor] = None,
                  utility: str = "ngram", max_order: int = 4, pairwise: bool = False) -> Dict[str, torch.Tensor]:
        """The consensus (minimum-Bayes-risk) choice among the candidates of every clip (conette_consensus, include/conette_hip.h;
        the rule: consensus.py): {"expected": (B, N) fp32, the weighted mean utility of each candidate against all of them,
        "best": (B,) int32, "margin": (B,) fp32 [, "pairwise": (B, N, N) fp32] [, "weights": (B, N) fp32, the normalised weights
        as the kernel read them, when ``weights`` are given]}.  ``preds`` (B, N, L) int32 or int64 (converted on
        the device), ``lens`` (B, N) as ``sample`` reports them or None (contents end at the first <eos> / pad), ``weights`` (B, N)
        finite and > 0 (normalised here, on the device) or None (equal).  Device tensors in, device tensors out, no host sync:
        what only the values could show -- a length outside 0 .. L (clamped), a weight that is not positive -- is the caller's
        contract (consensus.check_arguments states it)."""
        from . import consensus as rule
        if preds.ndim != 3:
            raise ValueError(f"consensus: preds of shape {tuple(preds.shape)} (expected (batch, n_cands, row_len))")
        b, n, l = (int(v) for v in preds.shape)
        rule.check_arguments(preds, None, None, utility, max_order)     # (shapes and settings: nothing here reads device memory)
        for name, t in (("lens", lens), ("weights", weights)):
            if t is not None and tuple(t.shape) != (b, n):
                raise ValueError(f"consensus: {name} of shape {tuple(t.shape)} for preds of shape {(b, n, l)}")
        ids = preds.to(self.device, torch.int32).contiguous()
        ln = None if lens is None else lens.to(self.device, torch.int32).contiguous()
        w = None
        if weights is not None:
            w64 = weights.to(self.device, torch.float64)
            w = (w64 / w64.sum(dim=1, keepdim=True)).to(torch.float32).contiguous()
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device=self.device)
        out = {"expected": e((b, n), torch.float32), "best": e((b,), torch.int32), "margin": e((b,), torch.float32)}
        if pairwise:
            out["pairwise"] = e((b, n, n), torch.float32)
        if w is not None:
            out["weights"] = w
        st = self.lib.conette_consensus(_ptr(ids), _ptr(ln), _ptr(w), b, n, l, rule.UTILITY[utility], int(max_order), self.eos_id,
                                        self.pad_id, _ptr(out["expected"]), _ptr(out["best"]), _ptr(out["margin"]),
                                        _ptr(out.get("pairwise")), _stream())
        _check(st, "conette_consensus")
        return out

    # ---- tag timeline: conette_tag_frames / conette_tag_events; the rule: tagging.py ------------------------------------------------
    def tag_frames(self, frame_embs: torch.Tensor, frame_lens: torch.Tensor, window: int) -> torch.Tensor:
        """Per-frame AudioSet tag probabilities (conette_tag_frames, include/conette_hip.h): the clip head pooled over ``window``
        frames around every frame.  frame_embs (B, T, 768), frame_lens (B,) -> (B, T, 527) fp32 on the device, rows at or beyond a
        clip's length exact zeros.  Runs on the encoder's context (a certified engine: its 16-bit base); no host sync."""
        from . import tagging
        if frame_embs.ndim != 3 or frame_embs.shape[2] != FEAT:
            raise ValueError(f"tag_frames: frame_embs of shape {tuple(frame_embs.shape)} (expected (batch, t_audio, {FEAT}))")
        b, t = int(frame_embs.shape[0]), int(frame_embs.shape[1])
        if tuple(frame_lens.shape) != (b,):
            raise ValueError(f"tag_frames: frame_lens of shape {tuple(frame_lens.shape)} for frame_embs of shape {tuple(frame_embs.shape)}")
        tagging.check_arguments(window=window)
        fe = frame_embs.to(self.device, torch.float32).contiguous()
        lens = frame_lens.to(self.device, torch.int32).contiguous()
        probs = torch.empty((b, t, N_TAGS), dtype=torch.float32, device=self.device)
        if probs.numel() == 0:
            return probs
        wsb = self._workspace("tags", max(1, int(self.lib.conette_tag_frames_workspace_bytes(self._ctx, b, t))))
        st = self.lib.conette_tag_frames(self._ctx, _ptr(fe), _ptr(lens), b, t, int(window), _ptr(probs), _ptr(wsb), wsb.numel(), _stream())
        _check(st, "conette_tag_frames")
        return probs

    def tag_events(self, frame_probs: torch.Tensor, frame_lens: torch.Tensor, on: float, off: Optional[float] = None,
                   min_frames: int = 1, max_gap: int = 0, max_events: int = 16) -> Dict[str, torch.Tensor]:
        """The events of every (clip, tag) sequence of ``frame_probs`` (B, T, n_tags) fp32 (conette_tag_events; the rule:
        tagging.events): {"spans": (B, n_tags, max_events, 2) int32, "peaks": (B, n_tags, max_events) fp32, "peak_frames":
        (B, n_tags, max_events) int32, "counts": (B, n_tags) int32} on the device; no host sync.  ``off`` None: off = on."""
        from . import tagging
        if frame_probs.ndim != 3:
            raise ValueError(f"tag_events: frame_probs of shape {tuple(frame_probs.shape)} (expected (batch, t_audio, n_tags))")
        b, t, c = (int(v) for v in frame_probs.shape)
        if tuple(frame_lens.shape) != (b,):
            raise ValueError(f"tag_events: frame_lens of shape {tuple(frame_lens.shape)} for frame_probs of shape {(b, t, c)}")
        off = on if off is None else off
        tagging.check_arguments(on=on, off=off, min_frames=min_frames, max_gap=max_gap, max_events=max_events)
        p = frame_probs.to(self.device, torch.float32).contiguous()
        lens = frame_lens.to(self.device, torch.int32).contiguous()
        m = int(max_events)
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device=self.device)
        out = {"spans": e((b, c, m, 2), torch.int32), "peaks": e((b, c, m), torch.float32), "peak_frames": e((b, c, m), torch.int32),
               "counts": e((b, c), torch.int32)}
        st = self.lib.conette_tag_events(_ptr(p), _ptr(lens), b, t, c, float(on), float(off), int(min_frames), int(max_gap), m,
                                         _ptr(out["spans"]), _ptr(out["peaks"]), _ptr(out["peak_frames"]), _ptr(out["counts"]), _stream())
        _check(st, "conette_tag_events")
        return out

    # ---- caption timeline: conette_decode_spans / conette_segments; the grid and the rule: segments.py --------------------------------
    def decode_spans(self, frame_embs: torch.Tensor, frame_lens: torch.Tensor, spans, bos_ids: torch.Tensor,
                     forbid_mask: Optional[torch.Tensor], beam: int, min_pred: int, max_pred: int, t_span: Optional[int] = None,
                     clone: bool = True) -> Dict[str, torch.Tensor]:
        """Beam search over spans of recordings that were encoded once (conette_decode_spans, include/conette_hip.h).
        frame_embs (N, t_rec, 768), frame_lens (N,) valid frames, ``spans`` (S, 3) rows of (recording, start, len) in frames -- held
        to ``segments.check_spans`` here, on the host, so ``frame_lens`` and ``spans`` are read back if they live on the device --,
        bos_ids (S,).  ``t_span`` (default: the longest len) is the width of the span axis.  Returns ``decode``'s dict over the S
        spans plus "spans", the table as the device read it.  The I/O buffers are persistent per shape, so that the library replays
        its hipGraph: a later call with another table of the same shape only rewrites the table's contents.  A certified engine
        searches on its 16-bit base context."""
        import numpy as np
        from . import segments as rule
        if frame_embs.ndim != 3 or frame_embs.shape[2] != FEAT:
            raise ValueError(f"decode_spans: frame_embs of shape {tuple(frame_embs.shape)} (expected (n_rec, t_rec, {FEAT}))")
        n, t_rec = int(frame_embs.shape[0]), int(frame_embs.shape[1])
        lens_h = torch.as_tensor(frame_lens).detach().cpu().reshape(-1).numpy()
        if lens_h.shape[0] != n:
            raise ValueError(f"decode_spans: frame_lens of {lens_h.shape[0]} entries for {n} recordings")
        if lens_h.size and (lens_h.min() < 0 or lens_h.max() > t_rec):
            raise ValueError(f"decode_spans: frame_lens must lie in 0..t_rec={t_rec}")
        table_h = spans.detach().cpu().numpy() if isinstance(spans, torch.Tensor) else np.asarray(spans)
        if t_span is None:
            t_span = int(table_h[:, 2].max()) if table_h.ndim == 2 and table_h.shape[0] > 0 and table_h.shape[1] == 3 else 0
        table_h = rule.check_spans(table_h, n, lens_h, int(t_span))
        s_n, t_span = int(table_h.shape[0]), int(t_span)
        if tuple(bos_ids.shape) != (s_n,):
            raise ValueError(f"decode_spans: bos_ids of shape {tuple(bos_ids.shape)} for {s_n} spans")
        ctx = self._ctx_dec
        beam, max_pred = int(beam), int(max_pred)
        buf = self._decode_buffers(s_n, t_span, beam, max_pred, False, False, spans=(n, t_rec))
        if frame_embs.data_ptr() != buf["fe"].data_ptr():
            buf["fe"].copy_(frame_embs, non_blocking=True)
        buf["spans"].copy_(torch.from_numpy(table_h), non_blocking=False)
        buf["bos"].copy_(bos_ids.to(torch.int32), non_blocking=True)
        forbid_ptr = None
        if forbid_mask is not None:
            if forbid_mask.numel() != self.vocab_size:
                raise ValueError("forbid_mask must have vocab_size entries")
            buf["forbid"].copy_(forbid_mask.to(torch.uint8), non_blocking=True)
            forbid_ptr = buf["forbid"]
        need = int(self.lib.conette_decode_spans_workspace_bytes(ctx, n, t_rec, s_n, t_span, beam, max_pred))
        wsb = self._workspace("dec_spans", max(need, 1))
        st = self.lib.conette_decode_spans(ctx, _ptr(buf["fe"]), _ptr(buf["spans"]), _ptr(buf["bos"]), _ptr(forbid_ptr), n, t_rec, s_n,
                                           t_span, beam, int(min_pred), max_pred, _ptr(buf["best_preds"]), _ptr(buf["best_lprobs"]),
                                           _ptr(buf["mult_preds"]), _ptr(buf["mult_lprobs"]), _ptr(buf["sizes"]), _ptr(wsb),
                                           wsb.numel() if need else 0, _stream())
        _check(st, "conette_decode_spans")
        cp = (lambda x: x.clone()) if clone else (lambda x: x)
        return {k: cp(buf[k]) for k in ("best_preds", "best_lprobs", "mult_preds", "mult_lprobs", "sizes", "spans")}

    def segments(self, preds: torch.Tensor, n_windows: torch.Tensor, lprobs: torch.Tensor, win_spans: torch.Tensor,
                 utility: str = "ngram", max_order: int = 4, threshold: float = 0.5, max_run: int = 0, max_segments: int = 64,
                 adjacency: bool = True) -> Dict[str, torch.Tensor]:
        """The merge rule over recordings (conette_segments; the rule: segments.merge_batch): ``preds`` (N, Wmax, L) the windows'
        best captions, ``n_windows`` (N,), ``lprobs`` (N, Wmax), ``win_spans`` (N, Wmax, 2) (start, len) in frames ->
        {"seg_windows", "seg_frames": (N, max_segments, 2) int32, "seg_rep": (N, max_segments) int32, "seg_agree":
        (N, max_segments) fp32, "counts": (N,) int32 [, "adjacency": (N, Wmax - 1) fp32]} on the device; no host sync."""
        from . import segments as rule
        if preds.ndim != 3:
            raise ValueError(f"segments: preds of shape {tuple(preds.shape)} (expected (n_rec, w_max, row_len))")
        n, wmax, l = (int(v) for v in preds.shape)
        if n < 1:
            raise ValueError("segments: no recording")
        code = rule.check_arguments(l, wmax, utility, max_order, threshold, max_run, max_segments)
        for name, t, shape in (("n_windows", n_windows, (n,)), ("lprobs", lprobs, (n, wmax)), ("win_spans", win_spans, (n, wmax, 2))):
            if tuple(t.shape) != shape:
                raise ValueError(f"segments: {name} of shape {tuple(t.shape)} for preds of shape {(n, wmax, l)} (expected {shape})")
        ids = preds.to(self.device, torch.int32).contiguous()
        nw = n_windows.to(self.device, torch.int32).contiguous()
        lp = lprobs.to(self.device, torch.float32).contiguous()
        sp = win_spans.to(self.device, torch.int32).contiguous()
        m = int(max_segments)
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device=self.device)
        out = {"seg_windows": e((n, m, 2), torch.int32), "seg_frames": e((n, m, 2), torch.int32), "seg_rep": e((n, m), torch.int32),
               "seg_agree": e((n, m), torch.float32), "counts": e((n,), torch.int32)}
        wsb = None
        if adjacency:
            out["adjacency"] = e((n, wmax - 1), torch.float32)
        elif wmax > 1:
            wsb = self._workspace("segments", n * (wmax - 1) * 4)
        st = self.lib.conette_segments(_ptr(ids), _ptr(nw), _ptr(sp), _ptr(lp), n, wmax, l, code, int(max_order), float(threshold),
                                       int(max_run), m, self.eos_id, self.pad_id, _ptr(out.get("adjacency")), _ptr(out["seg_windows"]),
                                       _ptr(out["seg_frames"]), _ptr(out["seg_rep"]), _ptr(out["seg_agree"]), _ptr(out["counts"]),
                                       _ptr(wsb), 0 if wsb is None else wsb.numel(), _stream())
        _check(st, "conette_segments")
        return out

    # ---- a1 --------------------------------------------------------------------------------
    def resample(self, x: torch.Tensor, orig_sr: int, new_sr: int) -> torch.Tensor:
        """(..., n) fp32 -> (..., ceil(n * new / orig)); torchaudio sinc_interpolation defaults."""
        if orig_sr == new_sr:
            return x
        shape = x.shape
        x2 = x.to(self.device, torch.float32).reshape(-1, shape[-1]).contiguous()
        n_out = self.lib.conette_resample_len(shape[-1], int(orig_sr), int(new_sr))
        out = torch.empty((x2.shape[0], n_out), dtype=torch.float32, device=self.device)
        _check(self.lib.conette_resample(_ptr(x2), x2.shape[0], shape[-1], int(orig_sr), int(new_sr), _ptr(out),
                                         _stream()), "conette_resample")
        return out.reshape(*shape[:-1], n_out)
