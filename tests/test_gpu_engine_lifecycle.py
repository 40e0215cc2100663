"""GPU: the decode graph cache (csrc/decoder.hip dec_graph_run), the persistent I/O buffer sets (Engine._decode_buffers) and the
grow-only workspaces (Engine._workspace) over an engine's whole life: the call sequences of tests/lifecycle_cases.py
(tests/test_cpu_engine_lifecycle.py proves on the model what each of them crosses).

The reference of EVERY call is the same call on a second engine of the same weights whose graph cache is switched off
(set_decode_graph(False): the eager path, which the state under test never touches), under the same fusion setting.  Every output
of the call is compared bit for bit (floats as int32); there is no tolerance.  Once per sequence the first call is also anchored
to the CPU oracle: an fp32 engine equals decoder_geometry.oracle_search of it by the rule of
test_gpu_decoder_edges.py::test_search_matches_the_oracle.

Besides the outputs, integer facts only: decode_graph_nodes() > 0 wherever the model says the key was captured or replays, the
buffer table never exceeds MAX_DECODE_GRAPHS and holds exactly the model's keys, a buffer set or a workspace is allocated again
exactly where the model says so.

  a. one key replayed on fresh data      b. several C keys on one buffer set      c. eviction of both tables
  d. options changed in mid-life         e. workspace regrowth, shared workspaces  f. teardown and rebuild (plain and ensemble)
  g. plain decode under the caller's capture at the first, second and third sighting of its key"""
import gc
import os

import numpy as np
import pytest
import torch

from tests import decoder_geometry as D
from tests import ensemble_cases as EC
from tests import lifecycle_cases as L

pytestmark = pytest.mark.gpu

SEQ = L.sequences()


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _assert_bit_equal(got, ref, what):
    assert set(got) == set(ref), (what, sorted(got), sorted(ref))
    for k in ref:
        assert got[k].shape == ref[k].shape and torch.equal(_bits(got[k]), _bits(ref[k])), (what, k)


def _engine(g, prec, wseed=0):
    from conette_amd.engine import Engine
    return Engine(EC.member_weights(g.name, wseed), precision=prec, n_layers=g.n_layers, d_ff=g.d_ff)


def _run(eng, g, c, side):
    """one call of the sequence on a side stream (the legacy default stream cannot be captured), every output on the host"""
    fe, lens, bos, forbid = L.inputs(g, c)
    fe = fe.cuda()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        if c.entry == "decode":
            out = eng.decode(fe, lens, bos, forbid, c.beam, c.min_pred, c.max_pred, want_trace=True, slot=c.slot)
        elif c.entry == "greedy":
            out = eng.greedy(fe, lens, bos, forbid, c.min_pred, c.max_pred)
        elif c.entry == "forcing":
            out = {"logits": eng.forcing(fe, lens, L.captions(g, c)[0])}
        elif c.entry == "score":
            out = eng.score(fe, lens, *L.captions(g, c))
        elif c.entry == "groups":
            out = eng.decode_groups(fe, lens, bos, forbid, 2, c.beam // 2, 0.5, c.min_pred, c.max_pred, want_trace=True)
        elif c.entry == "sample":
            rng = np.random.Generator(np.random.PCG64(97000 + c.seed))
            u = torch.from_numpy(rng.random((c.max_pred, c.b, c.beam)).astype(np.float32)).cuda()
            out = eng.sample(fe, lens, bos, forbid, c.beam, c.min_pred, c.max_pred, uniforms=u, want_tokens=True)
        else:
            assert c.entry == "constrained", c.entry
            out = eng.decode_constrained(fe, lens, bos, forbid, c.beam, c.min_pred, c.max_pred, no_repeat_ngram=2, want_trace=True)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items() if v is not None}


class _Life:
    """The eager reference engines, one per (geometry, precision, checkpoint seed), and their results: computed once per (fusion
    setting, call), shared by the tests, never modified."""

    def __init__(self):
        self.refs, self.results = {}, {}
        self.side = torch.cuda.Stream()
        torch.set_num_threads(min(16, os.cpu_count() or 1))

    def ref_engine(self, g, prec, wseed=0):
        key = (g.name, prec, wseed)
        if key not in self.refs:
            self.refs[key] = _engine(g, prec, wseed)
            self.refs[key].set_decode_graph(False)
        return self.refs[key]

    def reference(self, g, prec, c, fusion=True, wseed=0):
        key = (g.name, prec, wseed, fusion, c)
        if key not in self.results:
            ref = self.ref_engine(g, prec, wseed)
            ref.set_decode_fusion(fusion)
            try:
                self.results[key] = _run(ref, g, c, self.side)
            finally:
                ref.set_decode_fusion(True)
        return self.results[key]


@pytest.fixture(scope="module")
def life():
    h = _Life()
    yield h
    h.refs.clear()
    h.results.clear()
    D.drop_weights()
    EC.drop_member_weights()
    gc.collect()
    torch.cuda.empty_cache()


def _walk_sequence(life, seq, prec, eng=None, wseed=0, each=None):
    """Every step of the sequence on ``eng`` (a fresh engine when none is given): each call equals its reference, the Python tables
    move as the model says, and the graph cache has captured wherever the model says so.  ``each(event, engine)`` after every step."""
    from conette_amd.engine import MAX_DECODE_GRAPHS
    g = D.geometry(seq.geo)
    eng = _engine(g, prec, wseed) if eng is None else eng
    model = L.Model()
    fusion = True
    for i, step in enumerate(seq.steps):
        tag = (seq.name, prec, i, step)
        if isinstance(step, L.Opt):
            model.step(step)
            if step.name == "fusion":
                eng.set_decode_fusion(step.value)
                fusion = step.value
            elif step.name == "graph":
                eng.set_decode_graph(step.value)
            else:
                eng.profile_enable(("search",) if step.value else ())
                if not step.value:
                    eng.profile_read()
            continue
        had_buffers = L.py_key(step) in eng._dec_bufs
        ws_before = eng._ws.get(L.ws_key(step))
        got = _run(eng, g, step, life.side)
        ev = model.step(step)
        _assert_bit_equal(got, life.reference(g, prec, step, fusion, wseed), tag + (ev.mode,))
        assert (eng._ws[L.ws_key(step)] is not ws_before) == ev.regrew, tag
        if step.entry == "decode":
            assert had_buffers == (not ev.new_buffers), tag
            assert len(eng._dec_bufs) <= MAX_DECODE_GRAPHS and list(eng._dec_bufs) == list(model.bufs), tag
            if ev.mode in ("capture", "replay"):
                assert eng.decode_graph_nodes() > 0, tag
        if each is not None:
            each(ev, eng)
    return eng, model


# ---- the anchor: the first call of every sequence against the CPU oracle, fp32 ------------------------------------------------
@pytest.mark.parametrize("name", sorted(SEQ))
def test_first_call_matches_the_oracle(name, life):
    seq = SEQ[name]
    g, c = D.geometry(seq.geo), seq.steps[0]
    assert c.entry == "decode" and c.forbid == 0
    s = c.search()
    if ("oracle", g.name, c) not in life.results:      # (sequences that open with the same call share its oracle run)
        life.results[("oracle", g.name, c)] = D.oracle_search(g, s)
    ref = life.results[("oracle", g.name, c)]
    key = ("fp32 engine", g.name)
    if key not in life.refs:
        life.refs[key] = _engine(g, "fp32")
    out = _run(life.refs[key], g, c, life.side)
    tag = (name, g.name, s)
    sel, val = out["trace_sel"].numpy(), out["trace_val"].numpy()
    for step, clip, par, tok, sums, margin in ref["calls"]:
        k = len(par)
        assert sel[step, clip, :k, 0].tolist() == par and sel[step, clip, :k, 1].tolist() == tok, (tag, step, clip)
        np.testing.assert_allclose(val[step, clip, :k], sums, rtol=0, atol=2e-4 * (step + 1), err_msg=str((tag, step, clip)))
    ps, bm = (int(x) for x in out["sizes"].tolist())
    assert [ps, bm] == [ref["mult_preds"].shape[2], ref["best_preds"].shape[1]], tag
    assert out["mult_preds"][:, :, :ps].tolist() == ref["mult_preds"].tolist(), tag
    assert out["best_preds"][:, :bm].tolist() == ref["best_preds"].tolist(), tag
    np.testing.assert_allclose(out["mult_lprobs"].numpy(), ref["mult_lprobs"].numpy(), rtol=0, atol=1e-4, err_msg=str(tag))
    np.testing.assert_allclose(out["best_lprobs"].numpy(), ref["best_lprobs"].numpy(), rtol=0, atol=1e-4, err_msg=str(tag))


# ---- a .. e: the sequences ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", L.PRECISIONS)
def test_replay_on_fresh_data(prec, life):
    """a. One key, six calls, every input rewritten (frames, ragged lengths, task tokens, the mask's contents): the replays of calls
    three to six read the rewritten buffers."""
    eng, model = _walk_sequence(life, SEQ["replay"], prec)
    assert [e.mode for e in model.events] == ["eager", "capture"] + ["replay"] * 4
    assert len(eng._dec_bufs) == 1 and eng.decode_graph_nodes() > 0


@pytest.mark.parametrize("prec", L.PRECISIONS)
def test_one_buffer_set_several_keys(prec, life):
    """b. Two min_pred values x mask given / null at one shape and slot: one Python buffer set, four graph keys, three rounds."""
    eng, model = _walk_sequence(life, SEQ["keys"], prec)
    assert len(eng._dec_bufs) == 1 and len(model.graphs) == 4
    assert [e.mode for e in model.events] == ["eager"] * 4 + ["capture"] * 4 + ["replay"] * 4


@pytest.mark.parametrize("prec", L.PRECISIONS)
def test_eviction_of_graphs_and_buffers(prec, life):
    """c. More keys than either table holds, each seen three times; the dropped keys and the one kept by a touch again."""
    from conette_amd.engine import MAX_DECODE_GRAPHS
    eng, model = _walk_sequence(life, SEQ["walk"], prec)
    assert len(eng._dec_bufs) == MAX_DECODE_GRAPHS == len(model.graphs)
    assert model.events[-1].mode == "replay" and eng.decode_graph_nodes() > 0


@pytest.mark.parametrize("prec", L.PRECISIONS)
def test_options_in_mid_life(prec, life):
    """d. set_decode_fusion between the sightings of a key and under a replaying key, set_decode_graph off and on around a replaying
    key, a profiled context (which bypasses the cache): every result equals the reference under the same fusion setting."""
    _walk_sequence(life, SEQ["options"], prec)


@pytest.mark.parametrize("prec", L.PRECISIONS)
def test_workspace_regrowth_and_shared_workspaces(prec, life):
    """e. A replaying key, a larger decode that reallocates the workspace under its graph, the other entry points on that workspace
    (greedy, forcing, decode_groups, sample, decode_constrained take "dec"; score its own), the small key again."""
    seen = {}

    def each(ev, eng):
        seen.setdefault(ev.step.entry, set()).add(L.ws_key(ev.step))
        assert set(eng._ws) <= {"dec", "score"}, sorted(eng._ws)

    eng, model = _walk_sequence(life, SEQ["regrowth"], prec, each=each)
    assert seen == {e: {k} for e, k in L.WS_KEYS.items()}
    assert sum(e.regrew for e in model.events if e.step.entry == "decode") == 2      # the first call and the larger decode
    assert eng.decode_graph_nodes() > 0


# ---- f. teardown and rebuild -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", L.PRECISIONS)
def test_teardown_and_rebuild(prec, life):
    """An engine driven to replay, deleted and collected; an engine of another checkpoint in its place equals its OWN reference (a
    graph, buffer or context of the dead engine that survived would give the other checkpoint's captions)."""
    seq = SEQ["teardown"]
    eng, _ = _walk_sequence(life, seq, prec, wseed=0)
    assert eng.decode_graph_nodes() > 0
    del eng
    gc.collect()
    eng, _ = _walk_sequence(life, seq, prec, wseed=1)
    assert eng.decode_graph_nodes() > 0


def _ensemble(engines, g, c, side):
    """the two-member ensemble search of the call: member m on its own frames (seed + 100 m), equal weights"""
    _, lens, bos, forbid = L.inputs(g, c)
    fes = [D.frames(c.b, c.ta, c.frame_lens, c.seed + 100 * m)[0].cuda() for m in range(len(engines))]
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = engines[0].decode_ensemble([(e, fe, bos, 1.0) for e, fe in zip(engines, fes)], lens, forbid, c.beam, c.min_pred, c.max_pred,
                                         want_trace=True)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


@pytest.mark.parametrize("prec", L.PRECISIONS)
def test_ensemble_member_teardown_and_rebuild(prec, life):
    """A two-member ensemble driven to replay (the graph lives in member 0's context and holds member 1's context and workspace);
    member 1's engine deleted and rebuilt from other weights: the search equals the eager reference of the new pair."""
    seq = SEQ["teardown"]
    g = D.geometry(seq.geo)
    first = _engine(g, prec, 0)
    for wseed in (1, 2):
        second = _engine(g, prec, wseed)
        refs = [life.ref_engine(g, prec, 0), life.ref_engine(g, prec, wseed)]
        for i, c in enumerate(seq.steps):
            got = _ensemble([first, second], g, c, life.side)
            _assert_bit_equal(got, _ensemble(refs, g, c, life.side), (seq.name, prec, "ensemble", wseed, i))
        assert first.decode_graph_nodes() > 0, (prec, wseed)
        del second
        gc.collect()


# ---- g. plain decode under the caller's capture -------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", L.PRECISIONS)
def test_callers_capture_of_plain_decode(prec, life):
    """Three engines reach torch.cuda.graph at the first, second and third sighting of one key.  On a capturing stream the library
    launches into the caller's graph and leaves its own cache alone: the caller's graph, replayed twice after the input buffers
    were rewritten, equals the eager reference of the new data, and three later calls of a new key outside the capture still end
    in a graph of the library's own."""
    seq = SEQ["capture"]
    g = D.geometry(seq.geo)
    key_calls, new_calls = seq.steps[:L.CAPTURE_NEW_KEY], seq.steps[L.CAPTURE_NEW_KEY:]
    c0 = key_calls[0]
    assert all(L.py_key(c) == L.py_key(c0) and c.min_pred == c0.min_pred and c.forbid >= 0 for c in key_calls)
    # the references first: they also run every kernel of these calls once outside any capture (the library's one-time
    # per-kernel setup is not part of what is captured below)
    refs = {c: life.reference(g, prec, c) for c in seq.steps}
    for sighting in (1, 2, 3):
        tag = (prec, "sighting", sighting)
        eng = _engine(g, prec)
        for k in range(sighting - 1):
            _assert_bit_equal(_run(eng, g, key_calls[k], life.side), refs[key_calls[k]], tag + ("warm-up", k))
        # nothing may be allocated while capturing: the buffer set of decode(want_trace=True) (decode_input_buffer names the one
        # without the trace) and, where no call came before, the workspace by hand
        buf = eng._decode_buffers(c0.b, c0.ta, c0.beam, c0.max_pred, False, True, c0.slot, False, False)
        eng._workspace("dec", eng.lib.conette_decode_workspace_bytes(eng._ctx_dec, c0.b, c0.ta, c0.beam, c0.max_pred))
        lens_d = torch.empty((c0.b,), dtype=torch.int32, device="cuda")
        bos_d = torch.empty((c0.b,), dtype=torch.int32, device="cuda")
        forbid_d = torch.empty((g.v,), dtype=torch.uint8, device="cuda")

        def load(c):
            fe, lens, bos, forbid = L.inputs(g, c)
            buf["fe"].copy_(fe.cuda())
            lens_d.copy_(lens.cuda())
            bos_d.copy_(bos.int().cuda())
            forbid_d.copy_(forbid.to(torch.uint8).cuda())

        load(key_calls[sighting - 1])
        torch.cuda.synchronize()
        n_bufs, ws = len(eng._dec_bufs), eng._ws["dec"]
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            held = eng.decode(buf["fe"], lens_d, bos_d, forbid_d, c0.beam, c0.min_pred, c0.max_pred, want_trace=True, clone=False,
                              slot=c0.slot)
        assert len(eng._dec_bufs) == n_bufs and eng._ws["dec"] is ws, tag
        for c in key_calls[1:]:
            load(c)
            for x in held.values():
                x.view(torch.uint8).fill_(0xFF)
            graph.replay()
            torch.cuda.synchronize()
            _assert_bit_equal({k: v.cpu() for k, v in held.items()}, refs[c], tag + ("caller's replay", c.seed))
        del graph, held
        for c in new_calls:
            _assert_bit_equal(_run(eng, g, c, life.side), refs[c], tag + ("new key", c.seed))
        assert eng.decode_graph_nodes() > 0, tag
        del eng
        gc.collect()
