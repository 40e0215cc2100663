"""GPU: conette_segments / Engine.segments -- the merge rule of the caption timeline (csrc/dec_segments.h) -- on the handcrafted
caption tables of tests/span_cases.py.

1. BIT FOR BIT against segments.merge_batch on every setting (utilities x thresholds x max_run x max_segments): the rule fixes every
   rounding and the counts are integers, so there is no tolerance; ``adjacency`` is also held to the neighbouring entries of
   consensus.select_fp32's pairwise table.  The comparison runs on outputs pre-filled with 0xFF bytes.
2. The same bits on a second stream, without ``adjacency`` (the pair utilities in the workspace) and for a recording alone.
3. conette_consensus on one of its own cases: unchanged by the routines it now shares with the adjacency kernel.
4. C ABI errors name the argument and launch nothing."""
import ctypes as C

import numpy as np
import pytest
import torch

from conette_amd import consensus as R
from conette_amd import segments as S
from tests import span_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
OUT_KEYS = ("adjacency", "seg_windows", "seg_frames", "seg_rep", "seg_agree", "counts")


@pytest.fixture(scope="module")
def lib():
    from conette_amd import engine
    return engine.load_library()


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int32) if x.dtype == np.float32 else x


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def run(lib, preds, n_windows, lprobs, spans, kind, order, thr, max_run, max_seg, adjacency=True, stream=None, workspace=True):
    """one raw call on 0xFF-filled outputs; numpy results"""
    n, wmax, l = preds.shape
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(DEV)
    p, nw, lp, sp = dev(preds, np.int32), dev(n_windows, np.int32), dev(lprobs, np.float32), dev(spans, np.int32)
    poison = lambda shape, dt: torch.full(shape, -1, dtype=torch.int32, device=DEV).view(dt)
    out = {"adjacency": poison((n, wmax - 1), torch.float32) if adjacency else None, "seg_windows": poison((n, max_seg, 2), torch.int32),
           "seg_frames": poison((n, max_seg, 2), torch.int32), "seg_rep": poison((n, max_seg), torch.int32),
           "seg_agree": poison((n, max_seg), torch.float32), "counts": poison((n,), torch.int32)}
    ws = torch.empty(max(n * (wmax - 1) * 4, 1), dtype=torch.uint8, device=DEV) if (workspace and not adjacency) else None
    ptr = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream.cuda_stream
    st = lib.conette_segments(ptr(p), ptr(nw), ptr(sp), ptr(lp), n, wmax, l, R.UTILITY[kind], order, float(thr), max_run, max_seg, K.EOS, K.PAD,
                              *[ptr(out[k]) for k in OUT_KEYS], ptr(ws), 0 if ws is None else ws.numel(), C.c_void_p(s))
    assert st == 0, lib.conette_last_error().decode()
    (torch.cuda.current_stream() if stream is None else stream).synchronize()
    return {k: v.cpu().numpy() for k, v in out.items() if v is not None}


def rule(preds, n_windows, lprobs, spans, kind, order, thr, max_run, max_seg):
    return S.merge_batch(preds, n_windows, lprobs, spans, utility=kind, max_order=order, threshold=thr, max_run=max_run, max_segments=max_seg,
                         eos_id=K.EOS, pad_id=K.PAD)


def test_bit_for_bit_on_every_table_and_setting(lib):
    preds, n_windows, lprobs, spans = K.merge_batch_input()
    n_settings = 0
    for (kind, order), thr, max_run, max_seg in K.SETTINGS:
        got = run(lib, preds, n_windows, lprobs, spans, kind, order, thr, max_run, max_seg)
        want = rule(preds, n_windows, lprobs, spans, kind, order, thr, max_run, max_seg)
        for key in OUT_KEYS:
            assert same(got[key], want[key]), (kind, order, thr, max_run, max_seg, key, got[key], want[key])
        n_settings += 1
    assert n_settings == 54
    # the adjacency is the neighbouring entries of the consensus rule's pairwise table
    for kind, order in K.UTILITIES:
        got = run(lib, preds, n_windows, lprobs, spans, kind, order, 0.5, 0, 64)["adjacency"]
        for r, (name, p, _, _) in enumerate(K.caption_tables()):
            pair = R.select_fp32(p, utility=kind, max_order=order, eos_id=K.EOS, pad_id=K.PAD)["pairwise"]
            w = p.shape[0]
            want = np.asarray([pair[k, k + 1] for k in range(w - 1)], dtype=np.float32)
            assert same(got[r, :w - 1], want) and not bits(got[r, w - 1:]).any(), (name, kind, order)


def test_other_streams_no_adjacency_and_a_recording_alone(lib):
    preds, n_windows, lprobs, spans = K.merge_batch_input()
    side = torch.cuda.Stream()
    for (kind, order), thr, max_run, max_seg in (K.SETTINGS[0], K.SETTINGS[9], K.SETTINGS[29], K.SETTINGS[53]):
        args = (preds, n_windows, lprobs, spans, kind, order, thr, max_run, max_seg)
        a = run(lib, *args)
        b = run(lib, *args, stream=side)
        c = run(lib, *args, adjacency=False)
        assert "adjacency" not in c
        for other in (b, c):
            assert all(same(a[k], other[k]) for k in other)
        for r in (0, 6, len(n_windows) - 1):
            one = run(lib, preds[r:r + 1], n_windows[r:r + 1], lprobs[r:r + 1], spans[r:r + 1], kind, order, thr, max_run, max_seg)
            assert all(same(one[k], a[k][r:r + 1]) for k in one), (r, kind)
    # a table of one window per recording: no pair, no adjacency column, no workspace
    one = run(lib, preds[:, :1], np.ones_like(n_windows), lprobs[:, :1], spans[:, :1], "ngram", 4, 0.5, 0, 4, adjacency=False, workspace=False)
    assert (one["counts"] == 1).all() and (one["seg_windows"][:, 0] == [0, 1]).all() and (one["seg_agree"][:, 0] == 1).all()
    # n_windows = 0 and beyond w_max (clamped)
    odd = run(lib, preds[:2], np.asarray([0, 99], dtype=np.int32), np.zeros((2, K.W_MAX), np.float32), spans[:2] * 0, "edit", 4, 0.5, 0, 4)
    assert odd["counts"][0] == 0 and (odd["seg_rep"][0] == -1).all() and not odd["adjacency"][0].any() and odd["counts"][1] >= 1


def test_engine_segments():
    from conette_amd.engine import Engine
    from tests import decoder_geometry as D
    g = D.geometry("v31_ff32_l2")
    eng = Engine(D.weights(g), precision="bf16", n_layers=g.n_layers, d_ff=g.d_ff)
    preds, n_windows, lprobs, spans = K.merge_batch_input()
    t = lambda a: torch.from_numpy(a)
    for dt in (torch.int32, torch.int64):
        out = eng.segments(t(preds).to(DEV, dt), t(n_windows), t(lprobs).to(DEV), t(spans), utility="edit", threshold=0.5, max_run=2, max_segments=8)
        want = rule(preds, n_windows, lprobs, spans, "edit", 4, 0.5, 2, 8)
        assert set(out) == set(OUT_KEYS) and all(v.is_cuda for v in out.values())
        for key in OUT_KEYS:
            assert same(out[key].cpu().numpy(), want[key]), key
    slim = eng.segments(t(preds), t(n_windows), t(lprobs), t(spans), adjacency=False)
    assert "adjacency" not in slim and same(slim["counts"].cpu().numpy(), rule(preds, n_windows, lprobs, spans, "ngram", 4, 0.5, 0, 64)["counts"])
    for kw, word in ((dict(utility="bleu"), "utility"), (dict(max_order=0), "max_order"), (dict(threshold=float("nan")), "threshold"),
                     (dict(max_run=-1), "max_run"), (dict(max_segments=257), "max_segments")):
        with pytest.raises(ValueError, match=word):
            eng.segments(t(preds), t(n_windows), t(lprobs), t(spans), **kw)
    with pytest.raises(ValueError, match="lprobs"):
        eng.segments(t(preds), t(n_windows), t(lprobs[:, :3]), t(spans))
    D.drop_weights(g)


def test_consensus_keeps_its_bits(lib):
    """conette_consensus on cases of its own table: its phases are now calls of the routines dec_segments.h shares"""
    from tests import consensus_cases as KC
    from tests.test_gpu_consensus import fp32_weights
    from tests.test_gpu_consensus import run as consensus_run
    for name in ("B4N13L22_small_lens_w", "B7N17L31_small_pads_u"):
        _, preds, lens, weights = next(c for c in KC.cases() if c[0] == name)
        for kind, order in (("ngram", 4), ("edit", 4)):
            got = consensus_run(lib, preds, lens, fp32_weights(weights), kind, order)
            want = R.select_batch(preds, lens, weights, fp32=True, utility=kind, max_order=order, eos_id=KC.EOS, pad_id=KC.PAD)
            for key in ("pairwise", "expected", "margin", "best"):
                assert same(got[key], want[key]), (name, kind, key)


def test_c_abi_errors(lib):
    n, wmax, l, m = 2, 3, 5, 4
    preds = torch.zeros((n, wmax, l), dtype=torch.int32, device=DEV)
    nw = torch.full((n,), wmax, dtype=torch.int32, device=DEV)
    sp = torch.zeros((n, wmax, 2), dtype=torch.int32, device=DEV)
    lp = torch.zeros((n, wmax), dtype=torch.float32, device=DEV)
    poison = lambda shape, dt: torch.full(shape, -1, dtype=torch.int32, device=DEV).view(dt)
    outs = {"adjacency": poison((n, wmax - 1), torch.float32), "seg_windows": poison((n, m, 2), torch.int32),
            "seg_frames": poison((n, m, 2), torch.int32), "seg_rep": poison((n, m), torch.int32), "seg_agree": poison((n, m), torch.float32),
            "counts": poison((n,), torch.int32)}
    good = dict(preds=preds.data_ptr(), n_windows=nw.data_ptr(), win_spans=sp.data_ptr(), lprobs=lp.data_ptr(), n_rec=n, w_max=wmax, row_len=l,
                utility=0, max_order=4, threshold=0.5, max_run=0, max_segments=m, eos_id=2, pad_id=0,
                **{k: v.data_ptr() for k, v in outs.items()}, workspace=0, workspace_bytes=0)
    ptrs = ("preds", "n_windows", "win_spans", "lprobs", "workspace") + OUT_KEYS

    def raw(a):
        args = [C.c_void_p(v) if k in ptrs else v for k, v in a.items()]
        return lib.conette_segments(*args, C.c_void_p(torch.cuda.current_stream().cuda_stream))

    bad = [("preds", 0), ("n_windows", 0), ("win_spans", 0), ("lprobs", 0), ("seg_windows", 0), ("seg_frames", 0), ("seg_rep", 0),
           ("seg_agree", 0), ("counts", 0), ("n_rec", 0), ("w_max", 0), ("w_max", 4097), ("row_len", 0), ("row_len", 65), ("utility", 2),
           ("max_order", 0), ("max_order", 5), ("threshold", float("nan")), ("threshold", float("inf")), ("max_run", -1),
           ("max_segments", 0), ("max_segments", 257)]
    for word, value in bad:
        st = raw({**good, word: value})
        msg = lib.conette_last_error().decode()
        assert st != 0 and "segments" in msg and word in msg, (word, value, st, msg)
    st = raw({**good, "adjacency": 0})       # no adjacency and no workspace
    assert st != 0 and "workspace" in lib.conette_last_error().decode()
    torch.cuda.synchronize()
    for t in outs.values():      # nothing was launched
        assert bool((t.view(torch.int32) == -1).all())
    assert raw(good) == 0, lib.conette_last_error()
    torch.cuda.synchronize()
    assert outs["counts"].tolist() == [1, 1] and outs["seg_windows"][:, 0].tolist() == [[0, 3], [0, 3]] and bool((outs["adjacency"] == 1).all())
