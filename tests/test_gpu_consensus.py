"""GPU: conette_consensus / Engine.consensus -- the consensus (minimum-Bayes-risk) choice among candidates (csrc/dec_consensus.h).

1. BIT FOR BIT.  On the whole table of tests/consensus_cases.py -- ten shapes up to 2 clips of 64 x 64, two alphabets (ids up to
   2**31 - 1), with lens and with pads, uniform and given weights, "ngram" at orders 1, 2, 4 and "edit" -- ``expected``,
   ``pairwise`` and ``margin`` are the bits of consensus.select_fp32 and ``best`` is equal: the rule fixes every rounding and the
   counts are integers, so there is no tolerance.
2. DETERMINISM AND STREAMS.  Outputs pre-filled with 0xFF bytes are fully overwritten (the comparison of 1. runs on such buffers);
   two calls, a call on another stream, a clip alone and int64 ids give the same bits.
3. C ABI errors name the argument and launch nothing."""
import ctypes as C

import numpy as np
import pytest
import torch

from conette_amd import consensus as R
from tests import consensus_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def lib():
    from conette_amd import engine
    return engine.load_library()


@pytest.fixture(scope="module")
def eng():
    from conette_amd.engine import Engine
    from tests import decoder_geometry as D
    g = D.geometry("v31_ff32_l2")
    e = Engine(D.weights(g), precision="bf16", n_layers=g.n_layers, d_ff=g.d_ff)
    assert (e.eos_id, e.pad_id) == (K.EOS, K.PAD)
    yield e
    D.drop_weights(g)


def fp32_weights(weights):
    """what the host hands over: per clip normalised in float64, then fp32"""
    return None if weights is None else np.stack([R.device_weights(len(w), w) for w in weights])


def run(lib, preds, lens, w32, kind, order, pairwise=True, stream=None, eos=K.EOS, pad=K.PAD):
    """one raw call on 0xFF-filled outputs; numpy results"""
    b, n, l = preds.shape
    p = torch.from_numpy(np.ascontiguousarray(preds, dtype=np.int32)).to(DEV)
    ln = None if lens is None else torch.from_numpy(np.ascontiguousarray(lens, dtype=np.int32)).to(DEV)
    w = None if w32 is None else torch.from_numpy(np.ascontiguousarray(w32, dtype=np.float32)).to(DEV)
    poison = lambda shape, dt: torch.full(shape, -1, dtype=torch.int32, device=DEV).view(dt)
    out = {"expected": poison((b, n), torch.float32), "best": poison((b,), torch.int32), "margin": poison((b,), torch.float32),
           "pairwise": poison((b, n, n), torch.float32) if pairwise else None}
    ptr = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream.cuda_stream
    st = lib.conette_consensus(ptr(p), ptr(ln), ptr(w), b, n, l, R.UTILITY[kind], order, eos, pad, ptr(out["expected"]), ptr(out["best"]),
                               ptr(out["margin"]), ptr(out["pairwise"]), C.c_void_p(s))
    assert st == 0, lib.conette_last_error().decode()
    (torch.cuda.current_stream() if stream is None else stream).synchronize()
    return {k: v.cpu().numpy() for k, v in out.items() if v is not None}


def bits(x):
    return np.ascontiguousarray(x).view(np.int32) if x.dtype == np.float32 else x


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def reference():
    """select_fp32 over the table, computed once: {(name, kind, order): batch results}"""
    ref = {}
    for name, preds, lens, weights in K.cases():
        for kind, order in K.SETTINGS:
            ref[name, kind, order] = R.select_batch(preds, lens, weights, fp32=True, utility=kind, max_order=order, eos_id=K.EOS, pad_id=K.PAD)
    return ref


def test_bit_for_bit_on_the_whole_table(lib, reference):
    n_cases = 0
    for name, preds, lens, weights in K.cases():
        for kind, order in K.SETTINGS:
            got, want = run(lib, preds, lens, fp32_weights(weights), kind, order), reference[name, kind, order]
            for key in ("pairwise", "expected", "margin"):
                assert got[key].dtype == np.float32 and same(got[key], want[key]), (name, kind, order, key, got[key], want[key])
            assert np.array_equal(got["best"], want["best"]), (name, kind, order)
            n_cases += 1
    assert n_cases == len(K.SHAPES) * 2 * 4 * len(K.SETTINGS)


def test_given_fp32_weights_are_used_as_given(lib):
    """the library normalises nothing: weights that do not sum to 1 give the sums the rule gives for exactly those numbers"""
    name, preds, lens, weights = next(c for c in K.cases() if c[0] == "B4N13L22_small_lens_w")
    w32 = (weights / 3.0).astype(np.float32)
    got = run(lib, preds, lens, w32, "ngram", 4)
    want = R.select_batch(preds, lens, w32, fp32=True, as_given=True, utility="ngram", max_order=4, eos_id=K.EOS, pad_id=K.PAD)
    assert all(same(got[k], want[k]) for k in got)


PICKED = ("B2N64L64_big_lens_w", "B7N17L31_small_pads_u", "B5N3L12_big_pads_w", "B1N1L1_small_lens_u")


@pytest.mark.parametrize("name", PICKED)
def test_deterministic_on_any_stream_and_without_pairwise(lib, name):
    _, preds, lens, weights = next(c for c in K.cases() if c[0] == name)
    w32 = fp32_weights(weights)
    side = torch.cuda.Stream()
    for kind, order in (("ngram", 4), ("edit", 4)):
        a = run(lib, preds, lens, w32, kind, order)
        assert not any((bits(v) == -1).all() for v in a.values()) and np.isfinite(a["expected"]).all() and np.isfinite(a["pairwise"]).all()
        b = run(lib, preds, lens, w32, kind, order)
        c = run(lib, preds, lens, w32, kind, order, stream=side)
        d = run(lib, preds, lens, w32, kind, order, pairwise=False)
        assert "pairwise" not in d
        for other in (b, c, d):
            assert all(same(a[k], other[k]) for k in other), (name, kind)


@pytest.mark.parametrize("name", PICKED[:3])
def test_clip_alone_equals_clip_in_batch(lib, name):
    _, preds, lens, weights = next(c for c in K.cases() if c[0] == name)
    w32 = fp32_weights(weights)
    for kind, order in (("ngram", 2), ("edit", 4)):
        whole = run(lib, preds, lens, w32, kind, order)
        for b in range(preds.shape[0]):
            one = run(lib, preds[b:b + 1], None if lens is None else lens[b:b + 1], None if w32 is None else w32[b:b + 1], kind, order)
            assert all(same(one[k], whole[k][b:b + 1]) for k in one), (name, kind, b)


def test_other_eos_and_pad_ids(lib):
    """the ids are arguments: with eos 9 / pad 8 the rows of the small alphabet end where those words stand"""
    _, preds, _, _ = next(c for c in K.cases() if c[0] == "B4N13L22_small_pads_u")
    got = run(lib, preds, None, None, "ngram", 4, eos=9, pad=8)
    want = R.select_batch(preds, None, None, fp32=True, utility="ngram", max_order=4, eos_id=9, pad_id=8)
    assert all(same(got[k], want[k]) for k in got)


def test_engine_consensus(eng, lib, reference):
    for name in ("B2N16L20_small_lens_w", "B3N33L63_big_pads_u", "B4N13L22_big_lens_u", "B3N2L5_small_pads_w"):
        _, preds, lens, weights = next(c for c in K.cases() if c[0] == name)
        dev = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dt)
        for kind, order in (("ngram", 4), ("ngram", 1), ("edit", 4)):
            want = reference[name, kind, order]
            for dt in (torch.int32, torch.int64):
                out = eng.consensus(dev(preds, dt), dev(lens, torch.int64), dev(weights, torch.float64), utility=kind, max_order=order,
                                    pairwise=True)
                assert set(out) == {"expected", "best", "margin", "pairwise"} | ({"weights"} if weights is not None else set())
                assert out["best"].dtype == torch.int32 and out["expected"].is_cuda
                if weights is not None:     # the device's float64 normalisation gives the host's fp32 weights
                    assert same(out["weights"].cpu().numpy(), fp32_weights(weights)), name
                for key in ("pairwise", "expected", "margin", "best"):
                    assert same(out[key].cpu().numpy(), want[key]), (name, kind, order, dt, key)
            slim = eng.consensus(dev(preds, torch.int32), dev(lens, torch.int32), dev(weights, torch.float64), utility=kind, max_order=order)
            assert "pairwise" not in slim and np.array_equal(slim["best"].cpu().numpy(), want["best"])
    ok = torch.zeros((2, 3, 5), dtype=torch.int32, device=DEV)
    for kw, word in ((dict(utility="bleu"), "utility"), (dict(max_order=5), "max_order"), (dict(max_order=0), "max_order"),
                     (dict(lens=torch.zeros((2, 4), device=DEV)), "lens"), (dict(weights=torch.ones((3, 3), device=DEV)), "weights")):
        with pytest.raises(ValueError, match=word):
            eng.consensus(ok, **kw)
    for shape, word in (((2, 65, 5), "n_cands"), ((2, 3, 65), "row_len"), ((3, 5), "preds")):
        with pytest.raises(ValueError, match=word):
            eng.consensus(torch.zeros(shape, dtype=torch.int32, device=DEV))


def test_c_abi_errors(lib):
    b, n, l = 2, 3, 5
    preds = torch.zeros((b, n, l), dtype=torch.int32, device=DEV)
    poison = lambda shape, dt: torch.full(shape, -1, dtype=torch.int32, device=DEV).view(dt)
    e, best, m, pw = poison((b, n), torch.float32), poison((b,), torch.int32), poison((b,), torch.float32), poison((b, n, n), torch.float32)
    good = dict(preds=preds.data_ptr(), lens=0, weights=0, batch=b, n_cands=n, row_len=l, utility=0, max_order=4, eos_id=2, pad_id=0,
                expected=e.data_ptr(), best=best.data_ptr(), margin=m.data_ptr(), pairwise=pw.data_ptr())
    ptrs = ("preds", "lens", "weights", "expected", "best", "margin", "pairwise")

    def raw(a):
        args = [C.c_void_p(v) if k in ptrs else v for k, v in a.items()]
        return lib.conette_consensus(*args, C.c_void_p(torch.cuda.current_stream().cuda_stream))

    bad = [("preds", 0), ("expected", 0), ("best", 0), ("margin", 0), ("batch", 0), ("batch", -1), ("n_cands", 0), ("n_cands", 65),
           ("row_len", 0), ("row_len", 65), ("utility", 2), ("utility", -1), ("max_order", 0), ("max_order", 5)]
    for word, value in bad:
        st = raw({**good, word: value})
        msg = lib.conette_last_error().decode()
        assert st != 0 and "consensus" in msg and word in msg, (word, value, st, msg)
    torch.cuda.synchronize()
    for t in (e, best, m, pw):      # nothing was launched
        assert bool((t.view(torch.int32) == -1).all())
    assert raw(good) == 0, lib.conette_last_error()
    torch.cuda.synchronize()
    assert best.tolist() == [0, 0] and m.tolist() == [0.0, 0.0] and bool((pw == 1).all()) and bool((e == 1).all())
