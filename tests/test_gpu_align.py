"""GPU: conette_align / Engine.align / align_captions -- the cross-attention maps of given captions (csrc/dec_align.h).

Part 1, per forcing case of tests/decoder_geometry.py (cap_len 1 .. 64, pad layouts down to one valid token, frame_lens 1 .. Ta,
1 / 2 / 6 / 12 layers) plus one case that reaches the kernel's frame tiling (Ta = AL_TILE + 3, one clip's length straddling the
tile edge, the other's below it), and per precision.  Every call here goes through the C ABI with output buffers pre-filled
with NaN; the frames behind a clip's length carry decoder_geometry.PAD_FRAME_SCALE.
  * no tolerance: zeros behind frame_lens and in pad rows, the scores equal to conette_score's, targets = NULL, layer selection,
    stale workspaces, Engine.align;
  * derived: rows sum to 1, the all-layers map against the mean of the planes;
  * measured: against the restatement of tests/test_cpu_alignment.py (pinned to the oracles there).
Part 2, on the default synthetic decoder (decoder-only contexts): graph capture, chunking, fan-out, C ABI errors.
Part 3: CoNeTTEModel.align_captions and BaselinePLM.align_captions."""
import ctypes as C
import gc
import os

import numpy as np
import pytest
import torch

from tests import decoder_geometry as D
from tests.test_cpu_alignment import reference_maps
from tests.test_gpu_score import _Synth, auto_slabs, make_targets

pytestmark = pytest.mark.gpu

EXACT = ("fp32", "exact")
AL_TILE = 256                                       # csrc/dec_align.h: frames whose scores a wave keeps in LDS
TILE_CASE = D.Forcing("tile_edge", 2, AL_TILE + 3, (AL_TILE + 2, 200), 3, (3, 2), 21)
TILE_GEOMETRY = "v2048_ff96_l1"                     # the 1-layer geometry
CASES = [g.name for g in D.GEOMETRIES] + ["tile_edge"]

# Accuracy against the restatement, precision -> (max |d a|, mean |d a|) over the valid entries of every layer's plane: fp32 /
# exact against its fp32 form, bf16 / f16 against its operand form at that type; compared per case, the table holds the largest
# figure any of the ten cases gave (one MI355X run; the per-case figures: profiles/align_notes.md).  The bound of a case is
# 2 x the table (the margin of FORCING_MEASURED: box-to-box and accumulation-order variation), capped by ceilings that hold
# whatever was measured: fp32 / exact max |d a| <= 2e-3 (soft-max is 1-Lipschitz in the sup norm of the scores per element, and
# these precisions' logits are held to atol 2e-3 through the same layers); bf16 / f16 closer to their operand restatement than
# that restatement is to the fp32 one on the same case, in the maximum and in the mean.  The test prints every figure.
ALIGN_MEASURED = {"fp32": (7.153e-07, 8.350e-08), "exact": (1.103e-06, 1.277e-07), "bf16": (1.418e-03, 1.166e-04),
                  "f16": (1.841e-04, 2.306e-05)}
SUM_TOL = 1e-4                                      # Ta <= 70: (Ta / 8 + Ta) roundings of 2^-22 < 3e-5, times 3
MEAN_TOL = 4 * 2.0 ** -23                           # the all-layers map against the ascending mean of the stored planes


def sum_tol(ta):
    """pass 2's __expf against the running sum of pass 1: (Ta / 8 + Ta) roundings of 2^-22, times 3; 1e-4 up to Ta = 70"""
    return SUM_TOL if ta <= 70 else 3 * (ta / 8 + ta) * 2.0 ** -22


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _ptr(x):
    return C.c_void_p(0 if x is None else x.data_ptr())


def raw_align(eng, fe, lens, caps, tg, n, t, cpa, cap_len, mask, attn, planes, tok, sums, cnt, ws, ws_bytes=None):
    return eng.lib.conette_align(eng._ctx_dec, _ptr(fe), _ptr(lens), _ptr(caps), _ptr(tg), n, t, cpa, cap_len, mask, _ptr(attn),
                                 _ptr(planes), _ptr(tok), _ptr(sums), _ptr(cnt), _ptr(ws),
                                 (0 if ws is None else ws.numel()) if ws_bytes is None else ws_bytes,
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))


def nan_align(eng, fe, lens, caps, tg, cpa=1, mask=0, per_layer=True, ws_byte=None):
    """conette_align into NaN-filled buffers -> dict of CPU tensors (attn (P, L, T), attn_layers (NL, P, L, T) or None, scores)"""
    n, t = int(fe.shape[0]), int(fe.shape[1])
    p, cap_len = int(caps.shape[0]), int(caps.shape[1])
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device="cuda")
    out = {"attn": nan(p, cap_len, t), "attn_layers": nan(eng.n_layers, p, cap_len, t) if per_layer else None,
           "tok_lprobs": None if tg is None else nan(p, cap_len), "sum_lprobs": None if tg is None else nan(p),
           "n_tokens": None if tg is None else torch.full((p,), -7, dtype=torch.int32, device="cuda")}
    need = int(eng.lib.conette_align_workspace_bytes(eng._ctx_dec, n, t, cpa, cap_len, int(tg is not None)))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    if ws_byte is not None:
        ws.fill_(ws_byte)
    st = raw_align(eng, fe, lens, caps, tg, n, t, cpa, cap_len, mask, out["attn"], out["attn_layers"], out["tok_lprobs"],
                   out["sum_lprobs"], out["n_tokens"], ws)
    assert st == 0, eng.lib.conette_last_error()
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu()) for k, v in out.items()}


def _assert_bit_equal(a, b, what, keys=None):
    for k in keys or a:
        if a[k] is None:
            assert b[k] is None, (what, k)
        else:
            assert torch.equal(_bits(a[k]), _bits(b[k])), (what, k)


class _Case:
    def __init__(self, name):
        self.name = name
        self.g = D.geometry(TILE_GEOMETRY if name == "tile_edge" else name)
        self.f = TILE_CASE if name == "tile_edge" else self.g.forcing
        self.engines, self.cache, self.refs = {}, {}, {}
        torch.set_num_threads(min(16, os.cpu_count() or 1))
        self.fe, self.shape, self.caps = D.forcing_inputs(self.g, self.f)
        self.lens = self.shape[:, 1].int()
        self.targets = make_targets(self.caps, self.g.v, self.f.seed)
        self.dev = None

    def engine(self, prec):
        if prec not in self.engines:
            from conette_amd.engine import Engine
            self.engines[prec] = Engine(D.weights(self.g), precision=prec, n_layers=self.g.n_layers, d_ff=self.g.d_ff)
        return self.engines[prec]

    def inputs(self):
        if self.dev is None:
            self.dev = (self.fe.cuda(), self.lens.cuda(), self.caps.int().cuda(), self.targets.int().cuda())
        return self.dev

    def align(self, prec, mask=0, targets=True, per_layer=True):
        key = (prec, mask, targets, per_layer)
        if key not in self.cache:
            fe, lens, caps, tg = self.inputs()
            self.cache[key] = nan_align(self.engine(prec), fe, lens, caps, tg if targets else None, mask=mask, per_layer=per_layer)
        return self.cache[key]

    def reference(self, kind):
        """[per layer (B, L, Ta)] of the restatement: "fp32", "bf16" or "f16" """
        if kind not in self.refs:
            self.refs[kind] = torch.stack(reference_maps(self.g, kind, (self.fe, self.shape, self.caps))[1])
        return self.refs[kind]

    def valid(self):
        """(B, L, Ta) bool: a non-pad row and a frame inside the clip"""
        frames = torch.arange(self.f.ta)[None, None, :] < self.lens[:, None, None]
        return frames & (self.caps != 0)[:, :, None]


@pytest.fixture(scope="module", params=CASES)
def case(request):
    h = _Case(request.param)
    yield h
    h.engines.clear()
    h.cache.clear()
    h.refs.clear()
    h.dev = None
    D.drop_weights(h.g)
    gc.collect()
    torch.cuda.empty_cache()


# ---- part 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", D.PRECISIONS)
def test_zeros_row_sums_and_the_layer_mean(prec, case):
    g, f = case.g, case.f
    out = case.align(prec)
    valid = case.valid()
    rows = (case.caps != 0)
    assert int(rows.sum()) > 0 and int((~valid).sum()) > 0, "the case has valid rows and entries that must be zero"
    for name, a in [("attn", out["attn"])] + [(f"layer {l}", out["attn_layers"][l]) for l in range(g.n_layers)]:
        assert bool(torch.isfinite(a).all()), (case.name, prec, name, "NaN left in the buffer")
        assert torch.equal(_bits(a[~valid]), torch.zeros(int((~valid).sum()), dtype=torch.int32)), (case.name, prec, name, "exactly +0.0")
        assert bool((a >= 0).all())
        err = float((a.double().sum(dim=-1)[rows] - 1.0).abs().max())
        assert err <= sum_tol(f.ta), (case.name, prec, name, err)
    planes = out["attn_layers"]
    mean = planes[0].clone()
    for l in range(1, g.n_layers):
        mean = mean + planes[l]
    mean = mean * torch.tensor(1.0 / g.n_layers, dtype=torch.float32)
    d = float((out["attn"] - mean).abs().max())
    print(f"align {(case.name, prec)}: rows {f.b * f.cap_len} Ta {f.ta} |attn - mean of planes| {d:.3e}")
    assert d <= MEAN_TOL, (case.name, prec, d)


@pytest.mark.parametrize("prec", D.PRECISIONS)
def test_scores_equal_conette_score_and_targets_are_optional(prec, case):
    eng = case.engine(prec)
    out = case.align(prec)
    score = eng.score(case.fe.cuda(), case.lens, case.caps, case.targets)
    torch.cuda.synchronize()
    for k in ("tok_lprobs", "sum_lprobs", "n_tokens"):
        assert torch.equal(_bits(out[k]), _bits(score[k].cpu())), (case.name, prec, k)
    bare = case.align(prec, targets=False)
    assert bare["tok_lprobs"] is None and bare["sum_lprobs"] is None and bare["n_tokens"] is None
    _assert_bit_equal(out, bare, (case.name, prec, "targets = NULL"), keys=("attn", "attn_layers"))
    # the workspace: the lean one, with the score partials only when scores are asked for
    f = case.f
    lean = int(eng.lib.conette_align_workspace_bytes(eng._ctx_dec, f.b, f.ta, 1, f.cap_len, 0))
    full = int(eng.lib.conette_align_workspace_bytes(eng._ctx_dec, f.b, f.ta, 1, f.cap_len, 1))
    assert 0 < lean < full == int(eng.lib.conette_score_workspace_bytes(eng._ctx_dec, f.b, f.ta, 1, f.cap_len))


@pytest.mark.parametrize("prec", D.PRECISIONS)
def test_layer_selection(prec, case):
    g = case.g
    out = case.align(prec)
    all_ones = case.align(prec, mask=(1 << g.n_layers) - 1)
    _assert_bit_equal(out, all_ones, (case.name, prec, "mask 0 = all layers"))
    for l in range(g.n_layers):
        one = case.align(prec, mask=1 << l, targets=False)
        assert torch.equal(_bits(one["attn"]), _bits(out["attn_layers"][l])), (case.name, prec, l)
        assert torch.equal(_bits(one["attn_layers"]), _bits(out["attn_layers"])), (case.name, prec, l, "the planes do not depend on the mask")
    if g.n_layers >= 3:   # a subset that starts and ends inside: layers 1 and n - 1, no planes asked for
        sub = case.align(prec, mask=(1 << 1) | (1 << (g.n_layers - 1)), targets=False, per_layer=False)
        mean = (out["attn_layers"][1] + out["attn_layers"][g.n_layers - 1]) * torch.tensor(0.5)
        assert sub["attn_layers"] is None and float((sub["attn"] - mean).abs().max()) <= MEAN_TOL


@pytest.mark.parametrize("prec", ("bf16", "exact"))
def test_stale_workspace_and_engine_align(prec, case):
    eng = case.engine(prec)
    out = case.align(prec)
    fe, lens, caps, tg = case.inputs()
    for byte in (0xFF, 0):
        again = nan_align(eng, fe, lens, caps, tg, ws_byte=byte)
        _assert_bit_equal(out, again, (case.name, prec, byte))
    got = eng.align(case.fe.cuda(), case.lens, case.caps, case.targets, per_layer=True)
    torch.cuda.synchronize()
    _assert_bit_equal(out, {k: (None if v is None else v.cpu()) for k, v in got.items()}, (case.name, prec, "Engine.align"))
    some = eng.align(case.fe.cuda(), case.lens, case.caps, layers=[0])
    assert some["attn_layers"] is None and some["tok_lprobs"] is None
    assert torch.equal(_bits(some["attn"].cpu()), _bits(out["attn_layers"][0]))


@pytest.mark.parametrize("prec", D.PRECISIONS)
def test_maps_match_the_restatement(prec, case):
    got = case.align(prec)["attn_layers"].double()                      # (NL, B, L, Ta)
    valid = case.valid()[None].expand_as(got)
    ref = case.reference("fp32" if prec in EXACT else prec).double()
    err = (got - ref).abs()[valid]
    e_max, e_mean = float(err.max()), float(err.mean())
    if prec in EXACT:
        cap_max, cap_mean = 2e-3, 2e-3
    else:
        dist = (ref - case.reference("fp32").double()).abs()[valid]
        cap_max, cap_mean = float(dist.max()), float(dist.mean())
    print(f"align accuracy {(case.name, prec)}: max |d a| {e_max:.3e} mean {e_mean:.3e} (ceilings {cap_max:.3e} / {cap_mean:.3e})")
    if ALIGN_MEASURED is not None:
        m_max, m_mean = ALIGN_MEASURED[prec]
        cap_max, cap_mean = min(cap_max, 2 * m_max), min(cap_mean, 2 * m_mean)
    assert e_max <= cap_max and e_mean <= cap_mean, (case.name, prec, e_max, cap_max, e_mean, cap_mean)
    # the layer-mean map is the mean of what was just compared
    mean_err = float((case.align(prec)["attn"].double() - ref.mean(dim=0)).abs()[case.valid()].max())
    assert mean_err <= cap_max + MEAN_TOL, (case.name, prec, mean_err)


# ---- part 2: the default synthetic decoder (V = 5631, 6 layers), decoder-only contexts ----------------------------------------
@pytest.fixture(scope="module")
def synth(synth_weights):
    h = _Synth(synth_weights)
    yield h
    h.engines.clear()
    gc.collect()
    torch.cuda.empty_cache()


def _cpu(out):
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu()) for k, v in out.items()}


@pytest.mark.parametrize("prec", ("bf16", "exact"))
def test_eager_capture_and_replay_agree(prec, synth):
    eng = synth.engine(prec)
    n, cpa, cap_len = 2, 3, 12
    fe, shape = D.frames(n, 8, (8, 5), 6)
    caps, tg = synth.captions(n * cpa, cap_len, 2)
    fe_d, lens_d, caps_d, tg_d = fe.cuda(), shape[:, 1].int().cuda(), caps.int().cuda(), tg.int().cuda()
    eager = _cpu(eng.align(fe_d, lens_d, caps_d, tg_d, caps_per_audio=cpa, per_layer=True))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = eng.align(fe_d, lens_d, caps_d, tg_d, caps_per_audio=cpa, per_layer=True)
    for name in ("first replay", "second replay"):
        for x in held.values():
            x.view(torch.uint8).fill_(0xFF)
        graph.replay()
        _assert_bit_equal(eager, _cpu(held), (prec, name))
    del graph, held


@pytest.mark.parametrize("prec", D.PRECISIONS)
def test_chunks_and_fan_out_are_bit_identical(prec, synth):
    """3 clips (9, 4, 1 frames) x 3 captions x 10 positions: split into 3 chunks of clips / into slices of one caption, the maps
    are those of the unsplit call; and a (clip, caption) pair aligned alone (caps_per_audio = 1) has the maps it has among the
    clip's three."""
    from conette_amd import scoring
    eng = synth.engine(prec)
    n, cpa, cap_len, t = 3, 3, 10, 9
    fe, shape = D.frames(n, t, (9, 4, 1), 5)
    lens = shape[:, 1].int()
    caps, tg = synth.captions(n * cpa, cap_len, 1)
    fe_d = fe.cuda()
    full = _cpu(eng.align(fe_d, lens, caps, tg, caps_per_audio=cpa, per_layer=True))
    assert bool(torch.isfinite(full["attn"]).all()) and float((full["attn"].sum(dim=-1)[caps != 0] - 1).abs().max()) <= SUM_TOL
    need = lambda a, b: int(eng.lib.conette_align_workspace_bytes(eng._ctx_dec, a, t, b, cap_len, 1))
    for bound, n_chunks, rows_per_chunk in ((need(1, cpa), 3, cpa * cap_len), (need(1, 1), 9, cap_len)):
        assert len(scoring.plan_chunks(n, cpa, need, bound)) == n_chunks
        eng.score_workspace_bound = bound
        try:
            part = _cpu(eng.align(fe_d, lens, caps, tg, caps_per_audio=cpa, per_layer=True))
        finally:
            del eng.score_workspace_bound
        same_slabs = auto_slabs(rows_per_chunk, synth.v) == auto_slabs(n * cpa * cap_len, synth.v)
        _assert_bit_equal(full, part, (prec, n_chunks), keys=None if same_slabs else ("attn", "attn_layers", "n_tokens"))
    for clip, j in ((0, 1), (2, 2)):
        p = clip * cpa + j
        one = _cpu(eng.align(fe_d[clip:clip + 1], lens[clip:clip + 1], caps[p:p + 1], per_layer=True))
        assert torch.equal(_bits(one["attn"][0]), _bits(full["attn"][p])), (prec, clip, j)
        assert torch.equal(_bits(one["attn_layers"][:, 0]), _bits(full["attn_layers"][:, p])), (prec, clip, j)


def test_c_abi_errors(synth):
    eng = synth.engine("bf16")            # (a decoder-only context: it must work)
    n, t, cpa, cap_len = 2, 8, 2, 6
    fe, shape = D.frames(n, t, (8, 3), 7)
    caps, tg = synth.captions(n * cpa, cap_len, 3)
    fe_d, lens_d, caps_d, tg_d = fe.cuda(), shape[:, 1].int().cuda(), caps.int().cuda(), tg.int().cuda()
    need = int(eng.lib.conette_align_workspace_bytes(eng._ctx_dec, n, t, cpa, cap_len, 1))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    p = n * cpa
    attn = torch.empty((p, cap_len, t), dtype=torch.float32, device="cuda")
    planes = torch.empty((eng.n_layers, p, cap_len, t), dtype=torch.float32, device="cuda")
    tok = torch.empty((p, cap_len), dtype=torch.float32, device="cuda")
    sums = torch.empty((p,), dtype=torch.float32, device="cuda")
    cnt = torch.empty((p,), dtype=torch.int32, device="cuda")
    good = dict(fe=fe_d, lens=lens_d, caps=caps_d, tg=tg_d, n=n, t=t, cpa=cpa, cap_len=cap_len, mask=0, attn=attn, planes=planes,
                tok=tok, sums=sums, cnt=cnt, ws=ws)
    bad_calls = [{k: None} for k in ("fe", "lens", "caps", "attn", "sums", "cnt", "ws")]
    bad_calls += [{"tg": None}, {"tg": None, "tok": None, "sums": None}, {"tg": None, "tok": None, "cnt": None}]   # scores without targets
    bad_calls += [{"cap_len": 0}, {"cap_len": D.CN_MAX_PRED + 1}, {"cpa": 0}, {"cpa": -1}, {"n": 0}, {"t": 0}, {"ws_bytes": need - 1}]
    bad_calls += [{"mask": 1 << eng.n_layers}, {"mask": 1 | (1 << 31)}]
    for change in bad_calls:
        st = raw_align(eng, **{**good, **change})
        msg = eng.lib.conette_last_error().decode()
        assert st != 0 and "align" in msg, (change, st, msg)
    for args in ((0, t, cpa, cap_len, 1), (n, 0, cpa, cap_len, 0), (n, t, 0, cap_len, 1), (n, t, cpa, 0, 0)):
        assert eng.lib.conette_align_workspace_bytes(eng._ctx_dec, *args) == 0
    assert raw_align(eng, **good) == 0, eng.lib.conette_last_error()
    assert raw_align(eng, **{**good, "tok": None, "planes": None}) == 0
    assert raw_align(eng, **{**good, "tg": None, "tok": None, "sums": None, "cnt": None, "mask": 1 << (eng.n_layers - 1)}) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(attn).all()) and cnt.tolist() == (tg != 0).sum(dim=1).tolist()
    with pytest.raises(ValueError, match="caps_in ids"):
        eng.align(fe_d, lens_d, torch.full_like(caps, synth.v), tg, caps_per_audio=cpa)
    with pytest.raises(ValueError, match="layer"):
        eng.align(fe_d, lens_d, caps, tg, caps_per_audio=cpa, layers=[eng.n_layers])


# ---- part 3: the Python surface -----------------------------------------------------------------------------------------------
TAGS = {i: f"tag{i}" for i in range(527)}


@pytest.fixture(scope="module", params=("bf16", "fp32"))
def model(request, tmp_path_factory):
    from conette_amd import CoNeTTEConfig, CoNeTTEModel, synth as S
    model_dir = S.write_pretrained_dir(str(tmp_path_factory.mktemp("conette_synth_align")))
    config = CoNeTTEConfig.from_pretrained(model_dir)
    return CoNeTTEModel.from_pretrained(model_dir, config=config, precision=request.param, offline=True, audioset_idx_to_name=TAGS,
                                        stopwords=S.synth_stopwords())


def test_align_captions(model):
    from conette_amd import alignment as A
    from conette_amd import synth as S
    n = [48000, 29000]                                            # 1.5 s and 0.9 s at 32 kHz
    wav = S.synth_waveforms(2, max(n), 31, lengths=n)
    x = [torch.from_numpy(wav[i, : n[i]].copy())[None, :] for i in range(2)]
    frames = int(model.preprocessor(x, 32000, None)["audio"].shape[1])
    gen = model(x, sr=32000)
    out = model.align_captions(x, sr=32000, per_layer=True)
    assert out["cands"] == gen["cands"] and torch.equal(out["preds"], gen["preds"])
    b, n_caps, rows, t = out["attn"].shape
    assert (b, n_caps, t) == (2, 1, frames) and rows == gen["preds"].shape[1] and out["frame_sec"] == A.FRAME_SEC
    assert tuple(out["attn_layers"].shape) == (model.engine.n_layers, 2, 1, rows, t)
    assert torch.equal(out["tokens"][:, 0].cpu().long(), torch.where(gen["preds"].cpu() > 0, gen["preds"].cpu(), 0))
    scored = out["tokens"].cpu() != 0                            # rows labelled with a token
    assert bool(scored[:, :, 0].all())
    task_tok = model.batch_to_task_token_ids([model.default_task] * 2, [None] * 2).cpu().long()
    caps = torch.cat([task_tok[:, None], out["tokens"][:, 0].cpu().long()], dim=1)
    fed = (caps[:, :-1] != 0)[:, None]                           # rows with an input token: a row fed <eos> predicts a pad
    sums = out["attn"].cpu().sum(dim=-1)
    assert float((sums[fed] - 1).abs().max()) <= SUM_TOL and bool((sums[~fed] == 0).all()) and bool(fed[scored].all())
    for i in range(2):
        dur = n[i] / 32000
        peak = out["peak_time"][i][scored[i]]
        assert bool((peak >= 0).all()) and float(peak.max()) < dur + A.FRAME_SEC, (i, peak.tolist(), dur)
        span = out["span_time"][i][scored[i]]
        assert bool((span[:, 0] >= 0).all()) and bool((span[:, 0] < span[:, 1]).all()) and float(span.max()) < dur + A.FRAME_SEC
    assert bool(torch.isnan(out["peak_time"][~scored]).all()) and bool(torch.isnan(out["span_time"][~scored]).all())
    # explicit captions: the log-probabilities are score_captions's, bit for bit, and the search's own caption gives the same maps
    again = model.align_captions(x, caps, sr=32000)
    score = model.score_captions(x, caps, sr=32000)
    assert torch.equal(_bits(again["lprobs"]), _bits(score["lprobs"])) and torch.equal(_bits(again["sum_lprobs"]), _bits(score["sum_lprobs"]))
    assert torch.equal(again["n_tokens"], score["n_tokens"])
    assert torch.equal(_bits(again["attn"]), _bits(out["attn"])) and torch.equal(_bits(again["lprobs"]), _bits(out["lprobs"]))
    with_bos = caps.clone()
    with_bos[:, 0] = model.tokenizer.bos_token_id
    third = model.align_captions(x, with_bos[:, None], sr=32000, task=model.default_task, layers=[0])
    assert torch.equal(_bits(third["attn"]), _bits(out["attn_layers"][0])) and "attn_layers" not in third
    with pytest.raises(TypeError, match="search"):
        model.align_captions(x, caps, sr=32000, beam_size=2)


def test_predict_cli_align_writes_one_row_per_word(tmp_path):
    import csv
    import wave
    from conette_amd import synth as S
    from conette_amd.predict import main_predict
    model_dir = S.write_pretrained_dir(str(tmp_path / "model"))
    paths, secs = [], []
    for i in range(2):
        wav = S.synth_waveforms(1, 40000 + 8000 * i, 77 + i)[0]
        pcm = np.clip(np.round(wav * 32768.0), -32768, 32767).astype("<i2")
        p = str(tmp_path / f"clip{i}.wav")
        with wave.open(p, "wb") as w:
            w.setnchannels(1), w.setsampwidth(2), w.setframerate(32000)
            w.writeframes(pcm.tobytes())
        paths.append(p)
        secs.append((40000 + 8000 * i) / 32000)
    cache = tmp_path / "audioset_mapping"
    cache.mkdir()
    with open(cache / "class_labels_indices.csv", "w") as f:
        f.write("index,mid,display_name\n" + "".join(f"{i},/m/{i},tag{i}\n" for i in range(527)))
    os.environ["CONETTE_AUDIOSET_CACHE"] = str(cache)
    try:
        out_csv = str(tmp_path / "out.csv")
        common = ["--audio", *paths, "--task", "audiocaps", "--model_name", model_dir, "--precision", "fp32", "--verbose", "0"]
        plain = main_predict(common)
        res = main_predict(common + ["--align", "--csv_export", out_csv])
        with pytest.raises(ValueError, match="--sample"):
            main_predict(common + ["--align", "--sample", "2"])
    finally:
        os.environ.pop("CONETTE_AUDIOSET_CACHE", None)
    from conette_amd import alignment as A
    for i, p in enumerate(plain):
        rows = [r for r in res if r["audio"] == p["audio"]]
        assert " ".join(r["word"] for r in rows) == p["candidate"] and all(r["task"] == "audiocaps" for r in rows), (i, rows, p)
        assert all(0 <= float(r["start"]) < float(r["end"]) < secs[i] + A.FRAME_SEC for r in rows), (i, rows)
    got = list(csv.DictReader(open(out_csv)))
    assert list(got[0]) == ["audio", "task", "word", "start", "end"] and got == res


def test_baseline_plm_align_captions_equals_engine_align():
    from conette_amd import scoring, synth as S
    from conette_amd.baseline import BaselinePLM
    from tests import golden_util as G
    sd = S.synth_baseline_state_dict()
    sd = {k: (torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v) for k, v in sd.items()}
    g = np.load(os.path.join(G.GOLDEN, "baseline", "baseline_b4.npz"))
    fe, shape = torch.from_numpy(G.load(str(g["src"]))["frame_embs"]), torch.from_numpy(g["audio_shape"])
    caps = torch.from_numpy(g["caps_in"])                      # (4, 20): <bos>, words, pads -- no task token in this family
    plm = BaselinePLM(sd, beam_size=3, max_pred_size=20, precision="bf16")
    out = plm.align_captions({"audio": fe[:, None], "audio_shape": shape}, caps, per_layer=True)
    caps_in, targets = scoring.split_captions(caps, plm.pad_id)
    raw = plm.engine.align(fe, shape[:, 1].int(), caps_in, targets, per_layer=True)
    t = int(fe.shape[1])
    assert tuple(out["attn"].shape) == (4, 1, 19, t) and tuple(out["attn_layers"].shape) == (plm.engine.n_layers, 4, 1, 19, t)
    assert torch.equal(_bits(out["attn"][:, 0]), _bits(raw["attn"])) and torch.equal(_bits(out["attn_layers"][:, :, 0]), _bits(raw["attn_layers"]))
    assert torch.equal(_bits(out["lprobs"][:, 0]), _bits(raw["tok_lprobs"])) and torch.equal(out["tokens"][:, 0].cpu(), targets)
    assert torch.equal(_bits(out["lprobs"]), _bits(plm.score_captions({"audio": fe, "audio_shape": shape}, caps)["lprobs"]))
    peak = out["peak_time"][:, 0]
    lens = shape[:, 1]
    has = targets != plm.pad_id
    assert bool((peak.cpu()[has] < (lens[:, None].expand(-1, 19)[has] * out["frame_sec"])).all()) and bool(torch.isnan(peak.cpu()[~has]).all())
