"""CPU: the rules that tests/lifecycle_cases.py mirrors equal the ones in the sources, and its call sequences, run through its model
of the graph table (csrc/decoder.hip dec_graph_run), the buffer table (Engine._decode_buffers) and the workspaces
(Engine._workspace), cross what tests/test_gpu_engine_lifecycle.py relies on: evictions of both tables, a revisit of a dropped
key, a key kept by a touch, several graph keys on one buffer set, a workspace regrowth between two replays of one key, every
option change between the sightings it is meant to separate.  The first decode of every sequence is decided by margins that no
rounding of the fp32 engine can flip, and the "keys" sequence's results really depend on what tells its graph keys apart."""
import inspect
import os
import re

import pytest

from tests import decoder_geometry as D
from tests import lifecycle_cases as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "conette-audio-captioning_amd")
SEQ = L.sequences()


def _read(*parts):
    with open(os.path.join(PKG, *parts)) as f:
        return f.read()


def _decodes(events):
    return [e for e in events if isinstance(e.step, L.Call) and e.step.entry == "decode"]


# ---- the mirrored rules ----------------------------------------------------------------------------------------------------
def test_table_sizes_match_the_sources():
    dec, eng = _read("csrc", "decoder.hip"), _read("engine.py")
    c = {int(v) for v in re.findall(r"#define CN_MAX_DEC_GRAPHS (\d+)\b", dec)}
    py = {int(v) for v in re.findall(r"^MAX_DECODE_GRAPHS = (\d+)\b", eng, flags=re.M)}
    assert c == py == {L.MAX_GRAPHS}, (c, py)
    assert "DecGraph g[CN_MAX_DEC_GRAPHS] = {};" in dec and "if (cache->n == CN_MAX_DEC_GRAPHS) {" in dec
    assert eng.count("if len(self._dec_bufs) >= MAX_DECODE_GRAPHS:") == 2        # decode and decode_ensemble


def test_graph_table_rules_match_the_sources():
    dec = _read("csrc", "decoder.hip")
    run = dec[dec.index("static int dec_graph_run("):dec.index('extern "C" int conette_decode(')]
    # the key is the bytes of the record; a hit moves to the back; a miss at a full table drops the front
    assert "bool operator==(const DecArgs& o) const { return memcmp(this, &o, sizeof(DecArgs)) == 0; }" in dec
    assert "cache->g[cache->n - 1] = hit;" in run and "evicted = cache->g[0];" in run
    # eager at the first sighting, captured at the second, replayed from then on
    assert "fresh->seen = 1;" in run and "if (e->seen == 1) {" in run and "todo = CAPTURE;" in run
    assert run.index("if (e->exec) {") < run.index("if (e->seen == 1) {") < run.index("fresh->seen = 1;")
    # a profiled context bypasses the table; a disabled one runs eagerly without touching it
    assert "if (!cache || (ctx->prof_mask & dec_classes) != 0) return run();" in run
    assert re.search(r"if \(!cache->enabled\) \{\s*todo = EAGER;", run)
    # the fusion option empties the table, the graph option only flips the flag
    opt = dec[dec.index('extern "C" int conette_set_option('):dec.index("if (option == CONETTE_OPT_FORCING_STEPWISE)")]
    fusion = opt[opt.index("if (option == CONETTE_OPT_DECODE_FUSION)"):]
    assert "dec_graph_release(c->g[i]);" in fusion and "c->n = 0;" in fusion
    graph = opt[:opt.index("if (option == CONETTE_OPT_DECODE_FUSION)")]
    assert "c->enabled = value ? 1 : 0;" in graph and "c->n = 0" not in graph


def test_decode_asks_whether_the_stream_is_capturing():
    """conette_decode, like conette_decode_ensemble, launches into its caller's capture and leaves the graph table alone: the test
    comes before the call of dec_graph_run in both."""
    dec = _read("csrc", "decoder.hip")
    plain = dec[dec.index('extern "C" int conette_decode('):dec.index("// ---- ensemble beam search")]
    ens = dec[dec.index('extern "C" int conette_decode_ensemble('):dec.index('extern "C" int32_t conette_decode_graph_nodes(')]
    for body, call in ((plain, "return dec_graph_run(ctx, a, s, run);"), (ens, "return dec_graph_run(a.ens_ctx[0], a, s, run);")):
        ask = body.index("CN_HIP(hipStreamIsCapturing(s, &cap));")
        leave = body.index("if (cap != hipStreamCaptureStatusNone) return run();")
        assert ask < leave < body.index(call)
        assert body.count("dec_graph_run(") == 1


def test_python_tables_match_the_sources():
    eng = _read("engine.py")
    assert "key = (b, t, beam, max_pred, s0, trace, slot, margins, exact)" in eng
    body = eng[eng.index("def _decode_buffers("):eng.index("def decode(")]
    assert "buf = self._dec_bufs.pop(key, None)" in body and re.search(r"self\._dec_bufs\[key\] = buf +# least recently used first", body)
    assert "self._dec_bufs.pop(next(iter(self._dec_bufs)))" in body
    assert "buf = self._decode_buffers(b, t, int(beam), int(max_pred), want_step0_logits, want_trace, slot, want_margins, exact)" in eng
    c = L.dec(L.PAIR, 0, slot=3)
    assert L.py_key(c) == (2, 5, 3, 6, False, True, 3, False, False)
    # the workspace every entry point takes
    assert 'wsb = self._workspace(("xdec" if exact else "dec") + ("" if slot == 0 else str(slot)), need)' in eng
    assert L.ws_key(c) == "dec3" and L.ws_key(c._replace(slot=0)) == "dec"
    entry = {"greedy": "greedy", "forcing": "forcing", "sample": "sample", "groups": "decode_groups", "score": "score"}
    for name, method in entry.items():
        src = eng[eng.index("    def %s(self" % method):]
        src = src[:src.index("\n    def ", 10)]
        assert re.findall(r'self\._workspace\("(\w+)"', src) == [L.WS_KEYS[name]], name
    steered = eng[eng.index("    def _decode_steered(self"):eng.index("    def _check_req_tables(self")]
    assert steered.count('wsb = self._workspace("xdec" if exact else "dec", need)') == 2
    assert L.WS_KEYS["constrained"] == L.WS_KEYS["decode"] == "dec"
    # grow-only
    ws = eng[eng.index("    def _workspace(self"):eng.index("    # ---- a2")]
    assert "if ws is None or ws.numel() < nbytes:" in ws and "self._ws[key] = ws" in ws


def test_no_torch_at_import():
    src = inspect.getsource(L)
    assert not re.search(r"^(import|from) (torch|numpy)", src, flags=re.M)


# ---- the model itself, at a table of four entries ---------------------------------------------------------------------------
def test_model_orders_and_sightings():
    m = L.Model(capacity=4)
    k = lambda slot: L.dec(L.WALK, 0, slot=slot)
    assert [m.step(k(0)).mode for _ in range(4)] == ["eager", "capture", "replay", "replay"]
    for slot in (1, 2, 3):
        assert m.step(k(slot)).c_evicted is None
    assert [key[0][6] for key in m.graphs] == [0, 1, 2, 3] == [key[6] for key in m.bufs]
    assert m.step(k(0)).mode == "replay"                                           # the touch: slot 0 moves to the back
    ev = m.step(k(4))
    assert ev.mode == "eager" and ev.c_evicted[0][6] == 1 and ev.py_evicted[6] == 1 and ev.new_buffers
    assert [key[6] for key in m.bufs] == [2, 3, 0, 4]
    ev = m.step(k(1))                                                              # dropped: new buffers, a new key
    assert ev.mode == "eager" and ev.new_buffers and ev.c_evicted[0][6] == 2
    # options
    m.step(L.Opt("graph", False))
    assert m.step(k(0)).mode == "off" and m.step(L.Opt("graph", True)).mode == "option" and m.step(k(0)).mode == "replay"
    m.step(L.Opt("profile", True))
    assert m.step(k(0)).mode == "bypass"
    m.step(L.Opt("profile", False))
    m.step(L.Opt("fusion", False))
    assert len(m.graphs) == 0 and len(m.bufs) == 4 and m.step(k(0)).mode == "eager"
    # the workspace: grow-only, per key, ordered only where one shape holds the other
    assert not m.step(L.dec(L.WALK, 1, slot=0)).regrew and m.step(L.dec(L.MAIN, 1, slot=0)).regrew
    assert not m.step(L.dec(L.WALK, 2, slot=0)).regrew
    with pytest.raises(AssertionError):
        m.step(L.dec((4, 2, 3, 4), 0, slot=0))


# ---- what the sequences cross ---------------------------------------------------------------------------------------------------
def test_shapes_stay_tiny():
    assert set(SEQ) == set(L.FIRST_SEED)
    for seq in SEQ.values():
        assert seq.geo == (L.GEO_WALK if seq.name == "walk" else L.GEO_MAIN)
        first = seq.steps[0]
        assert isinstance(first, L.Call) and first.entry == "decode" and first.forbid == 0 and first.seed == L.FIRST_SEED[seq.name]
        for c in seq.steps:
            if isinstance(c, L.Call):
                assert 1 <= c.b <= 3 and 2 <= c.beam <= 4 and 3 <= c.ta <= 9 and 4 <= c.max_pred <= 8, (seq.name, c)
                assert len(c.frame_lens) == c.b and all(1 <= n <= c.ta for n in c.frame_lens) and c.min_pred <= c.max_pred


def test_replay_sequence():
    ev = L.simulate(SEQ["replay"])
    assert [e.mode for e in ev] == ["eager", "capture", "replay", "replay", "replay", "replay"]
    assert len({e.c_key for e in ev}) == 1
    calls = [e.step for e in ev]
    assert all(c.forbid >= 0 for c in calls) and len({c.forbid for c in calls}) == 6 and len({c.seed for c in calls}) == 6
    assert len({c.frame_lens for c in calls}) >= 3 and all(len(set(c.frame_lens)) > 1 for c in calls)


def test_keys_sequence():
    ev = L.simulate(SEQ["keys"])
    assert len({L.py_key(e.step) for e in ev}) == 1 and sum(e.new_buffers for e in ev) == 1
    keys = {e.c_key for e in ev}
    assert len(keys) == 4 and {(k[2], k[5]) for k in keys} == {(f, m) for f in (True, False) for m in L.KEYS_MIN_PRED}
    assert [e.mode for e in ev] == ["eager"] * 4 + ["capture"] * 4 + ["replay"] * 4
    # neighbours in the sequence differ in min_pred alone or in the mask alone: a key comparison that dropped either would hand
    # one call the other's graph
    first = [e.step for e in ev[:4]]
    assert first[0]._replace(min_pred=first[1].min_pred) == first[1] and first[0]._replace(forbid=-1) == first[2]


def test_walk_sequence():
    ev = L.simulate(SEQ["walk"])
    assert len({L.py_key(e.step) for e in ev}) == L.WALK_KEYS > L.MAX_GRAPHS
    slot = lambda key: key[0][6]
    first = next(i for i, e in enumerate(ev) if e.c_evicted is not None)
    assert ev[first].py_evicted is not None and first == 3 * L.MAX_GRAPHS + 1
    # every key before the overflow was seen three times: eager, capture, replay
    assert [e.mode for e in ev[:first - 1]] == ["eager", "capture", "replay"] * L.MAX_GRAPHS
    # the touch just before the overflow keeps slot 0: the front of both tables, yet slot 1 is what the overflow drops
    assert ev[first - 1].step.slot == 0 and ev[first - 1].mode == "replay"
    assert slot(ev[first].c_evicted) == 1 == ev[first].py_evicted[6]
    c_gone = [slot(e.c_evicted) for e in ev if e.c_evicted is not None]
    py_gone = [e.py_evicted[6] for e in ev if e.py_evicted is not None]
    assert c_gone == py_gone == [1, 2, 3, 4]
    # the dropped keys again: new buffers, and eager / capture / replay once more
    for s in (1, 2):
        again = [e for e in ev[first:] if e.step.slot == s]
        assert [e.mode for e in again] == ["eager", "capture", "replay"] and again[0].new_buffers
        assert again[0].c_key != next(e.c_key for e in ev if e.step.slot == s)
    # the kept key at the very end: the same buffers, a replay
    assert ev[-1].step.slot == 0 and ev[-1].mode == "replay" and not ev[-1].new_buffers and ev[-1].c_key == ev[0].c_key
    assert len({e.step.seed for e in ev}) == len(ev)


def test_options_sequence():
    seq = SEQ["options"]
    ev = L.simulate(seq)
    modes = [e.mode if e.mode != "option" else "%s=%d" % (e.step.name, e.step.value) for e in ev]
    assert modes == ["eager", "fusion=0", "eager", "capture", "fusion=1", "eager", "capture", "replay", "fusion=0",
                     "eager", "capture", "replay", "fusion=1", "eager", "capture", "replay",
                     "graph=0", "off", "graph=1", "replay", "profile=1", "bypass", "profile=0", "replay"]
    assert len({e.c_key for e in _decodes(ev)}) == 1


def test_regrowth_sequence():
    ev = L.simulate(SEQ["regrowth"])
    dec = _decodes(ev)
    small = [e for e in dec if L.py_key(e.step) == L.py_key(dec[0].step)]
    assert [e.mode for e in small] == ["eager", "capture", "replay", "eager", "capture", "replay"]
    grow = [i for i, e in enumerate(ev) if e.regrew and i > 0 and e.step.entry == "decode"]
    assert len(grow) == 1 and ev.index(small[2]) < grow[0] < ev.index(small[5])      # between two replays of one key
    assert small[2].c_key[:4] == small[5].c_key[:4] and small[2].c_key[4] != small[5].c_key[4]
    assert not any(e.new_buffers for e in small[1:])
    # the other entry points run on the regrown workspace, behind a decode that is larger in every dimension
    others = [e for e in ev if e.step.entry != "decode"]
    assert {e.step.entry for e in others} == set(L.WS_KEYS) - {"decode"}
    big = ev[grow[0]].step
    for e in others:
        assert ev.index(e) > grow[0]
        c = e.step
        assert c.b <= big.b and c.ta <= big.ta and c.beam <= big.beam and c.max_pred <= big.max_pred


def test_capture_and_teardown_sequences():
    cap = SEQ["capture"].steps
    key, new = cap[:L.CAPTURE_NEW_KEY], cap[L.CAPTURE_NEW_KEY:]
    assert len(key) == 3 and len(new) == 3
    assert len({L.py_key(c) for c in key}) == 1 and len({(c.min_pred, c.forbid >= 0) for c in key}) == 1 and key[0].forbid >= 0
    assert len({L.py_key(c) for c in new}) == 1 and L.py_key(new[0]) != L.py_key(key[0])
    assert len({c.seed for c in cap}) == 6
    assert [e.mode for e in L.simulate(SEQ["teardown"])] == ["eager", "capture", "replay"]


# ---- conditions on the inputs -------------------------------------------------------------------------------------------------
def _oracle(g, c, min_pred=None, forbid=True):
    import torch
    from oracle import cpu_ref as O
    s = c.search() if min_pred is None else c.search()._replace(min_pred=min_pred)
    w = D.weights(g)
    fe, shape, bos, mask = D.search_inputs(g, s)
    with torch.no_grad():
        mem, m = O.encode_audio(w, fe, shape)
        trace = []
        out = O.generate(w, mem, m, bos, vocab_size=g.v, beam_size=s.beam, min_pred_size=s.min_pred, max_pred_size=s.max_pred,
                         forbid_rep_mask=mask if forbid else None, n_layers=g.n_layers, trace=trace)
    calls = [(step, x["clip"], x["parent"], x["token"], x["sum_lprob"], x["margin"]) for step, st in enumerate(trace) for x in st]
    return min(D.effective_margin(x) for x in calls), out[2], out[3]


def test_first_calls_are_decided_by_clear_margins():
    """The anchor of the GPU file holds an fp32 engine to the oracle on the first call of every sequence without any near-tie
    allowance: every effective margin of that search is at least decoder_geometry.MIN_MARGIN."""
    import torch
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    seen = {}
    for seq in SEQ.values():
        c = seq.steps[0]
        if c not in seen:
            seen[c] = _oracle(D.geometry(seq.geo), c)[0]
            print(f"{seq.name}: smallest effective margin {seen[c]:.5f}")
        assert seen[c] >= D.MIN_MARGIN, (seq.name, seen[c])


def test_keys_results_depend_on_what_separates_the_keys():
    """Every round of the "keys" sequence: the oracle's captions or scores differ between any two of its four variants (two
    min_pred values x mask given / absent), so a call that ran another variant's graph cannot equal its reference."""
    import torch
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    g = D.geometry(L.GEO_MAIN)
    assert tuple(sorted({c.seed for c in SEQ["keys"].steps})) == L.KEYS_SEEDS
    for seed in L.KEYS_SEEDS:
        c = L.dec(L.PAIR, seed, min_pred=L.KEYS_MIN_PRED[0])
        outs = [_oracle(g, c, mp, fb)[1:] for mp in L.KEYS_MIN_PRED for fb in (True, False)]
        for i in range(4):
            for j in range(i + 1, 4):
                same = outs[i][0].shape == outs[j][0].shape and torch.equal(outs[i][0], outs[j][0]) and torch.equal(outs[i][1], outs[j][1])
                assert not same, (seed, i, j)
    D.drop_weights(g)
    D.drop_weights()
