"""GPU: conette_decode_spans / Engine.decode_spans -- conette_decode's beam search over spans of recordings that were encoded once
(csrc/dec_spans.h) -- on the tables of tests/span_cases.py, in the four precisions.

1. EQUAL TO conette_decode ON GATHERED FRAMES, bit for bit: for every table all five outputs equal Engine.decode on the torch-gathered
   (S, t_span, 768) clips with the spans' lengths.  Both GEMMs of the preparation stay below 4096 rows here, where cn_gemm2 and
   cn_gemm2_sp dispatch one 64 x 64 tile and a row's sum does not depend on its neighbours.  (Above 4096 and 8192 rows, where the
   tiles change: tests/test_gpu_decoder_rows.py::test_decode_spans_over_8400_frames, against the CPU oracle.)
2. AGAINST ITSELF, bit for bit: a span alone equals the same span in a table, duplicated spans give duplicated rows, a permuted table
   gives permuted rows, NaNs behind a recording's length and outside every span change nothing, and outputs filled with 0xFF bytes
   are fully overwritten.
3. GRAPH REPLAY: three calls on the same buffers with the table's contents changed between them -- eager, captured, replayed --
   each equal to a fresh reference; the same with the graph cache switched off.
4. REFUSALS name the argument and launch nothing."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import decoder_geometry as D
from tests import span_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEYS = ("best_preds", "best_lprobs", "mult_preds", "mult_lprobs", "sizes")
GEO = D.geometry(K.GEOMETRY)


@pytest.fixture(scope="module", params=D.PRECISIONS)
def eng(request):
    from conette_amd.engine import Engine
    e = Engine(D.weights(GEO), precision=request.param, n_layers=GEO.n_layers, d_ff=GEO.d_ff)
    assert (e.eos_id, e.pad_id) == (K.EOS, K.PAD)
    return e


def search_inputs(table, seed=0):
    """(bos (S,) int64, forbid (V,) bool): span s is prompted with the task of its recording"""
    w = D.weights(GEO)
    tasks = torch.as_tensor([(seed + int(r)) % 7 for r in table[:, 0]])
    return w["model.task_id_to_token_id"][tasks], w["model.forbid_rep_mask"].bool()


def bits(t):
    t = t.cpu()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b, rows=None):
    for k in KEYS:
        x, y = bits(a[k]), bits(b[k])
        if rows is not None and k != "sizes":
            x = x[rows]
        if x.shape != y.shape or not torch.equal(x, y):
            return False
    return True


def spans_call(eng, set_name, table, t_span, beam, min_pred, fe=None):
    rec, lens = K.recordings(set_name)
    bos, forbid = search_inputs(table)
    fe = torch.from_numpy(rec) if fe is None else fe
    return eng.decode_spans(fe.to(DEV), torch.from_numpy(lens), table, bos, forbid, beam, min_pred, K.MAX_PRED, t_span=t_span)


def reference(eng, set_name, table, t_span, beam, min_pred):
    """Engine.decode on the gathered clips"""
    rec, _ = K.recordings(set_name)
    clips, lens = K.gather(rec, table, t_span)
    bos, forbid = search_inputs(table)
    return eng.decode(torch.from_numpy(clips).to(DEV), torch.from_numpy(lens), bos, forbid, beam, min_pred, K.MAX_PRED)


@pytest.mark.parametrize("case", K.span_cases(), ids=lambda c: f"{c[0]}_beam{c[4]}_min{c[5]}")
def test_equals_decode_on_gathered_frames(eng, case):
    name, set_name, table, t_span, beam, min_pred = case
    got = spans_call(eng, set_name, table, t_span, beam, min_pred)
    want = reference(eng, set_name, table, t_span, beam, min_pred)
    assert torch.equal(got["spans"].cpu(), torch.from_numpy(table))
    for k in KEYS:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        assert torch.equal(bits(got[k]), bits(want[k])), (name, beam, min_pred, k, got[k], want[k])
    # the duplicated row of the table (tests/span_cases.py: row 1 again in the middle)
    twin = (table.shape[0] - 1) // 2
    assert np.array_equal(table[twin], table[1])
    for k in KEYS[:4]:
        assert torch.equal(bits(got[k])[twin], bits(got[k])[1]), k


def test_alone_permuted_and_poisoned(eng):
    name, set_name, table, t_span = K.span_tables()[2]
    assert set_name == "three40"
    beam, min_pred = 3, 3
    sub = np.ascontiguousarray(table[[2, 17, 30, 41, 5, 17]])      # spans of all three recordings, one of them twice
    whole = spans_call(eng, set_name, sub, t_span, beam, min_pred)
    assert all(torch.equal(bits(whole[k])[1], bits(whole[k])[5]) for k in KEYS[:4])
    # a permuted table gives permuted rows (the sizes are maxima over the table: unchanged)
    perm = np.asarray([4, 0, 5, 3, 1, 2])
    moved = spans_call(eng, set_name, np.ascontiguousarray(sub[perm]), t_span, beam, min_pred)
    assert same(whole, moved, rows=torch.from_numpy(perm))
    # a span alone: the same row, up to the sizes (the widths the whole table needs)
    for s in (0, 3):
        one = spans_call(eng, set_name, sub[s:s + 1], t_span, beam, min_pred)
        for k in KEYS[:4]:
            assert torch.equal(bits(one[k])[0], bits(whole[k])[s]), (s, k)
    # frames behind a recording's length and frames outside every span do not matter
    rec, lens = K.recordings(set_name)
    used = np.zeros(rec.shape[:2], dtype=bool)
    for r, start, ln in sub.tolist():
        used[r, start:start + ln] = True
    assert (~used).sum() > 20 and all((~used[r, :n]).any() for r, n in enumerate(lens))
    poisoned = rec.copy()
    poisoned[~used] = np.nan
    again = spans_call(eng, set_name, sub, t_span, beam, min_pred, fe=torch.from_numpy(poisoned))
    assert same(whole, again)


def test_outputs_are_fully_overwritten(eng):
    name, set_name, table, t_span = K.span_tables()[1]
    sub = np.ascontiguousarray(table[::3])
    first = spans_call(eng, set_name, sub, t_span, 3, 0)
    rec, lens = K.recordings(set_name)
    bos, forbid = search_inputs(sub)
    bufs = eng.decode_spans(torch.from_numpy(rec).to(DEV), torch.from_numpy(lens), sub, bos, forbid, 3, 0, K.MAX_PRED, t_span=t_span,
                            clone=False)
    for k in KEYS:
        bufs[k].view(torch.uint8).fill_(0xFF)
    torch.cuda.synchronize()
    second = spans_call(eng, set_name, sub, t_span, 3, 0)
    assert same(first, second)


@pytest.mark.parametrize("graph", [True, False])
def test_graph_replay_follows_the_table(eng, graph):
    name, set_name, table, t_span = K.span_tables()[3]
    beam, min_pred = 3, 3
    n = 7
    tables = [np.ascontiguousarray(table[i::5][:n]) for i in (0, 1, 2)] + [np.ascontiguousarray(table[0::5][:n])]
    assert all(t.shape == (n, 3) for t in tables) and not np.array_equal(tables[0], tables[1])
    side = torch.cuda.Stream()       # (the legacy default stream cannot be captured)
    side.wait_stream(torch.cuda.current_stream())
    eng.set_decode_graph(graph)
    try:
        # same shape, same persistent buffers: eager, captured, replayed, replayed -- only the table's contents change
        with torch.cuda.stream(side):
            got = [spans_call(eng, set_name, t, t_span, beam, min_pred) for t in tables]
        side.synchronize()
        if graph:
            assert eng.decode_graph_nodes() > 0
    finally:
        eng.set_decode_graph(True)
    for t, g in zip(tables, got):
        assert same(g, reference(eng, set_name, t, t_span, beam, min_pred)), t
    assert same(got[0], got[3])


def test_refusals_name_the_argument_and_launch_nothing(eng):
    lib, ctx = eng.lib, eng._ctx_dec
    n, t_rec, s_n, t_span, beam, max_pred = 1, 9, 2, 9, 3, K.MAX_PRED
    rec, _ = K.recordings("one9")
    fe = torch.from_numpy(rec).to(DEV)
    spans = torch.tensor([[0, 0, 9], [0, 1, 7]], dtype=torch.int32, device=DEV)
    bos = torch.full((s_n,), 1, dtype=torch.int32, device=DEV)
    poison = lambda shape, dt: torch.full(shape, -1, dtype=torch.int32, device=DEV).view(dt)
    outs = [poison((s_n, max_pred), torch.int32), poison((s_n,), torch.float32), poison((s_n, beam, max_pred), torch.int32),
            poison((s_n, beam), torch.float32), poison((2,), torch.int32)]
    need = lib.conette_decode_spans_workspace_bytes(ctx, n, t_rec, s_n, t_span, beam, max_pred)
    assert need > lib.conette_decode_workspace_bytes(ctx, s_n, t_span, beam, max_pred) > 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def raw(t_span=t_span, beam=beam, ws_bytes=need, spans_ptr=ptr(spans), max_pred=max_pred):
        return lib.conette_decode_spans(ctx, ptr(fe), spans_ptr, ptr(bos), C.c_void_p(0), n, t_rec, s_n, t_span, beam, 0, max_pred,
                                        *[ptr(o) for o in outs], ptr(ws), ws_bytes, C.c_void_p(torch.cuda.current_stream().cuda_stream))

    for kw, word in ((dict(ws_bytes=need - 1), "workspace"), (dict(t_span=0), "t_span"), (dict(t_span=-3), "t_span"), (dict(beam=17), "beam"),
                     (dict(beam=0), "beam"), (dict(spans_ptr=C.c_void_p(0)), "spans"), (dict(max_pred=65), "max_pred")):
        st = raw(**kw)
        msg = lib.conette_last_error().decode()
        assert st != 0 and "decode_spans" in msg and word in msg, (kw, st, msg)
    assert lib.conette_decode_spans_workspace_bytes(ctx, n, t_rec, s_n, 0, beam, max_pred) == 0
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o.view(torch.int32) == -1).all())
    assert raw() == 0, lib.conette_last_error()
    torch.cuda.synchronize()
    assert not any(bool((o.view(torch.int32) == -1).all()) for o in outs[:4])
