"""The host-side state that decides which decode launches run and on which memory, mirrored from the sources as a pure-Python
model, and the call sequences that walk it over an engine's whole life.

tests/test_cpu_engine_lifecycle.py pins the mirrored rules to the sources, runs every sequence through the model and asserts what
it crosses; tests/test_gpu_engine_lifecycle.py runs the sequences on an engine and compares every call, bit for bit, with the same
call on a second engine whose graph cache is switched off.

Sources mirrored:
  * csrc/decoder.hip ``dec_graph_run``: per context a table of at most CN_MAX_DEC_GRAPHS entries keyed by the bytes of the
    ``DecArgs`` record (every pointer, the shape, min_pred), least recently used first.  A hit moves to the back; a miss at a full
    table drops the front.  A key runs eagerly at its first sighting, is captured at the second and replays from then on.  A
    context that is profiled bypasses the table, one whose graphs are switched off runs eagerly without touching it,
    CONETTE_OPT_DECODE_FUSION empties it, and a call on a stream its caller captures launches into that capture and leaves the
    table alone.
  * conette_amd/engine.py ``Engine._decode_buffers``: at most MAX_DECODE_GRAPHS persistent I/O buffer sets keyed by (b, t, beam,
    max_pred, step-0 logits, trace, slot, margins, exact); a hit is popped and re-inserted, a miss at a full table drops the front.
  * ``Engine._workspace``: grow-only, one tensor per key; ``decode`` takes "dec" at slot 0 and "dec<slot>" elsewhere, ``greedy``,
    ``forcing``, ``sample``, ``decode_groups`` and ``decode_constrained`` take "dec", ``score`` takes "score".

What the model cannot know: addresses.  A buffer set or a workspace that is allocated again counts as a new pointer (a new
generation), so a key the model calls new may in truth meet a stale entry of equal bytes -- whose graph then holds exactly the
pointers of the call and is as good as a fresh one.  The byte size of a workspace is the library's; the model only orders two
decodes of which one is at least as large in every dimension, and a plan may not put two decodes of incomparable shapes on one
workspace key.  Entry points other than ``decode`` are taken not to grow "dec": the plans run them behind a decode that is larger
in every dimension, and the GPU test holds the pointer to that.

No torch at import time."""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict, List, NamedTuple, Optional, Tuple, Union

from tests import decoder_geometry as D

MAX_GRAPHS = 64                  # decoder.hip: #define CN_MAX_DEC_GRAPHS 64; engine.py: MAX_DECODE_GRAPHS = 64
WS_KEYS = {"decode": "dec", "greedy": "dec", "forcing": "dec", "sample": "dec", "groups": "dec", "constrained": "dec",
           "score": "score"}     # engine.py: the first argument of self._workspace(...) in each entry point
GEO_WALK = "v31_ff32_l2"         # the eviction walk: the cheapest launches
GEO_MAIN = "v2049_ff256_l6"      # elsewhere: the fused FFN stream, six layers
PRECISIONS = ("bf16", "exact")


class Call(NamedTuple):
    entry: str                   # a key of WS_KEYS
    b: int
    beam: int                    # decode: the beam; groups: 2 groups of beam // 2; sample: samples per clip; others: unused
    ta: int
    frame_lens: Tuple[int, ...]
    min_pred: int
    max_pred: int                # forcing / score: the caption length
    forbid: int                  # -1: no mask; 0: the checkpoint's mask; k > 0: that mask with seeded entries flipped
    slot: int
    seed: int

    def search(self) -> D.Search:
        """the decode as a case of tests/decoder_geometry.py (the checkpoint's mask, i.e. forbid == 0)"""
        return D.Search("lifecycle_%d" % self.seed, self.b, self.beam, self.ta, self.frame_lens, self.min_pred, self.max_pred, self.seed)


class Opt(NamedTuple):
    name: str                    # "fusion": set_decode_fusion; "graph": set_decode_graph; "profile": profile_enable(("search",)) / (())
    value: bool


Step = Union[Call, Opt]


class Sequence(NamedTuple):
    name: str
    geo: str
    steps: Tuple[Step, ...]


# ---- the model ------------------------------------------------------------------------------------------------------------------
def py_key(c: Call) -> Tuple:
    """engine.py _decode_buffers: key = (b, t, beam, max_pred, s0, trace, slot, margins, exact), as the tests call decode
    (want_trace=True, nothing else)"""
    return (c.b, c.ta, c.beam, c.max_pred, False, True, c.slot, False, False)


def ws_key(c: Call) -> str:
    """engine.py decode: ("xdec" if exact else "dec") + ("" if slot == 0 else str(slot))"""
    return WS_KEYS[c.entry] + ("" if c.entry != "decode" or c.slot == 0 else str(c.slot))


def _dims(c: Call) -> Tuple[int, int, int, int]:
    return (c.b, c.ta, c.beam, c.max_pred)


class Event(NamedTuple):
    step: Step
    mode: str                    # "eager" | "capture" | "replay" | "bypass" (profiled) | "off" (graphs switched off) | "other" | "option"
    c_key: Optional[Tuple]
    c_evicted: Optional[Tuple]   # the C key dropped from the front of the graph table
    py_evicted: Optional[Tuple]  # the Python key dropped from the front of the buffer table
    regrew: bool                 # the call's workspace was allocated again
    new_buffers: bool


class Model:
    def __init__(self, capacity: int = MAX_GRAPHS) -> None:
        self.capacity = capacity
        self.graphs: "OrderedDict[Tuple, str]" = OrderedDict()     # C key -> "seen" | "graph", least recently used first
        self.bufs: "OrderedDict[Tuple, int]" = OrderedDict()       # Python key -> generation of its buffer set
        self.ws: Dict[str, Tuple[int, Tuple[int, int, int, int]]] = {}   # workspace key -> (generation, largest decode so far)
        self.generation = 0
        self.enabled, self.profiled, self.fusion = True, False, True
        self.events: List[Event] = []

    def _buffers(self, c: Call) -> Tuple[int, Optional[Tuple], bool]:
        key = py_key(c)
        gen = self.bufs.pop(key, None)
        if gen is not None:
            self.bufs[key] = gen                 # a hit moves to the back
            return gen, None, False
        evicted = None
        if len(self.bufs) >= self.capacity:
            evicted = next(iter(self.bufs))
            self.bufs.pop(evicted)
        self.generation += 1
        self.bufs[key] = self.generation
        return self.generation, evicted, True

    def _workspace(self, c: Call) -> Tuple[int, bool]:
        key = ws_key(c)
        have = self.ws.get(key)
        if c.entry != "decode":                  # (taken not to grow the workspace: the module docstring)
            if have is None:
                self.generation += 1
                self.ws[key] = (self.generation, (0, 0, 0, 0))
                return self.generation, True
            return have[0], False
        dims = _dims(c)
        if have is not None:
            le = all(a <= b for a, b in zip(dims, have[1]))
            ge = all(a >= b for a, b in zip(dims, have[1]))
            assert le or ge, ("incomparable decode shapes on one workspace", key, dims, have[1])
            if le:
                return have[0], False
        self.generation += 1
        self.ws[key] = (self.generation, dims)
        return self.generation, True

    def step(self, s: Step) -> Event:
        if isinstance(s, Opt):
            if s.name == "fusion":
                self.fusion = s.value
                self.graphs.clear()              # cached graphs hold the other launch sequence
            elif s.name == "graph":
                self.enabled = s.value
            else:
                assert s.name == "profile"
                self.profiled = s.value
            ev = Event(s, "option", None, None, None, False, False)
            self.events.append(ev)
            return ev
        if s.entry != "decode":
            _, regrew = self._workspace(s)
            ev = Event(s, "other", None, None, None, regrew, False)
            self.events.append(ev)
            return ev
        buf_gen, py_evicted, new_buffers = self._buffers(s)
        ws_gen, regrew = self._workspace(s)
        key = (py_key(s), buf_gen, s.forbid >= 0, ws_key(s), ws_gen, s.min_pred)
        c_evicted = None
        if self.profiled:
            mode = "bypass"
        elif not self.enabled:
            mode = "off"
        elif key in self.graphs:
            state = self.graphs.pop(key)
            mode = "replay" if state == "graph" else "capture"
            self.graphs[key] = "graph"
        else:
            if len(self.graphs) == self.capacity:
                c_evicted = next(iter(self.graphs))
                self.graphs.pop(c_evicted)
            self.graphs[key] = "seen"
            mode = "eager"
        ev = Event(s, mode, key, c_evicted, py_evicted, regrew, new_buffers)
        self.events.append(ev)
        return ev


def simulate(seq: Sequence, capacity: int = MAX_GRAPHS) -> List[Event]:
    m = Model(capacity)
    return [m.step(s) for s in seq.steps]


# ---- the sequences ----------------------------------------------------------------------------------------------------------------
# (b, beam, ta, max_pred): B 1 .. 3, beam 2 .. 4, Ta 3 .. 9, max_pred 4 .. 8
MAIN = (3, 4, 9, 8)
PAIR = (2, 3, 5, 6)
SMALL = (1, 2, 3, 4)
WALK = (2, 2, 3, 4)

# The seed of every sequence's first decode: the first of 0, 1, 2 ... at which the oracle's search of that call has every effective
# margin at or above decoder_geometry.MIN_MARGIN (the fp32 engine is held to the oracle on it by the rule of
# test_gpu_decoder_edges.py::test_search_matches_the_oracle); for "keys" the three seeds (one per round) at which, besides, the
# oracle's result changes with min_pred and with the mask (tests/test_cpu_engine_lifecycle.py recomputes all of it).
FIRST_SEED = {"replay": 1, "keys": 0, "walk": 0, "options": 1, "regrowth": 0, "teardown": 0, "capture": 0}
KEYS_SEEDS = (0, 1, 2)
KEYS_MIN_PRED = (2, 5)


def _lens(b: int, ta: int, seed: int) -> Tuple[int, ...]:
    """ragged memory lengths: clip 0 is full, the others 1 .. ta by the seed"""
    return tuple(ta if i == 0 else 1 + (seed * 5 + i * 3) % ta for i in range(b))


def dec(shape, seed: int, min_pred: int = 3, forbid: int = 0, slot: int = 0) -> Call:
    b, beam, ta, max_pred = shape
    return Call("decode", b, beam, ta, _lens(b, ta, seed), min(min_pred, max_pred), max_pred, forbid, slot, seed)


def other(entry: str, shape, seed: int) -> Call:
    b, beam, ta, max_pred = shape
    return Call(entry, b, beam, ta, _lens(b, ta, seed), 2, max_pred, 0, 0, seed)


def _replay() -> Sequence:
    """a. one key, six calls, every input rewritten between them, the mask present throughout"""
    s0 = FIRST_SEED["replay"]
    return Sequence("replay", GEO_MAIN, tuple(dec(MAIN, s0 if i == 0 else 100 + i, forbid=i) for i in range(6)))


def _keys() -> Sequence:
    """b. four C keys (two min_pred values x mask given / null) on one Python buffer set, three rounds"""
    steps = []
    for seed in KEYS_SEEDS:
        for forbid in (0, -1):
            for mp in KEYS_MIN_PRED:
                steps.append(dec(PAIR, seed, min_pred=mp, forbid=forbid))
    return Sequence("keys", GEO_MAIN, tuple(steps))


WALK_KEYS = MAX_GRAPHS + 2       # slots 0 .. 65


def _walk() -> Sequence:
    """c. more keys than either table holds: slots 0 .. 63 three times each, a touch of slot 0 (the front of both tables), slots 64
    and 65 (which drop slots 1 and 2), then slots 1 and 2 again (dropped: new buffers, new graphs) and slot 0 (resident: a replay)"""
    s0 = FIRST_SEED["walk"]
    seed = lambda slot, k: s0 if (slot, k) == (0, 0) else 200 + 7 * slot + k
    steps = [dec(WALK, seed(slot, k), min_pred=2, slot=slot) for slot in range(MAX_GRAPHS) for k in range(3)]
    steps.append(dec(WALK, seed(0, 3), min_pred=2, slot=0))
    steps += [dec(WALK, seed(slot, k), min_pred=2, slot=slot) for slot in (MAX_GRAPHS, MAX_GRAPHS + 1) for k in range(3)]
    steps += [dec(WALK, seed(slot, 3 + k), min_pred=2, slot=slot) for slot in (1, 2) for k in range(3)]
    steps.append(dec(WALK, seed(0, 4), min_pred=2, slot=0))
    return Sequence("walk", GEO_WALK, tuple(steps))


def _options() -> Sequence:
    """d. options changed in mid-life of one key"""
    s0 = FIRST_SEED["options"]
    n = iter(range(300, 400))
    k = lambda first=False: dec(MAIN, s0 if first else next(n))
    return Sequence("options", GEO_MAIN, (
        k(True), Opt("fusion", False),                   # between the eager and the capture sighting
        k(), k(), Opt("fusion", True),                   # between the capture and the replay
        k(), k(), k(), Opt("fusion", False),             # under a replaying key
        k(), k(), k(), Opt("fusion", True),
        k(), k(), k(),
        Opt("graph", False), k(), Opt("graph", True), k(),
        Opt("profile", True), k(), Opt("profile", False), k()))


def _regrowth() -> Sequence:
    """e. a small key replays on slot 0; a larger decode reallocates the workspace they share; the other entry points that take
    the same workspace run on it; the small key again"""
    s0 = FIRST_SEED["regrowth"]
    return Sequence("regrowth", GEO_MAIN, (
        dec(SMALL, s0), dec(SMALL, 401), dec(SMALL, 402),
        dec(MAIN, 403),
        other("greedy", SMALL, 404), other("forcing", SMALL, 405), other("score", SMALL, 406), other("groups", (1, 4, 3, 4), 407),
        other("sample", SMALL, 408), other("constrained", SMALL, 409),
        dec(SMALL, 410), dec(SMALL, 411), dec(SMALL, 412)))


def _teardown() -> Sequence:
    """f. three calls of one key: what an engine is driven through before it is deleted, and what its successor is held to"""
    s0 = FIRST_SEED["teardown"]
    return Sequence("teardown", GEO_MAIN, (dec(PAIR, s0), dec(PAIR, 501), dec(PAIR, 502)))


CAPTURE_NEW_KEY = 3              # the steps from here on are the new key decoded outside the capture


def _capture() -> Sequence:
    """g. one key for the caller's capture (the warm-up calls and the captured one take steps 0 .. 2's data in turn, the two replays
    of the caller's graph steps 1 and 2's), then three calls of a new key"""
    s0 = FIRST_SEED["capture"]
    return Sequence("capture", GEO_MAIN, (dec(PAIR, s0, forbid=0), dec(PAIR, 601, forbid=1), dec(PAIR, 602, forbid=2),
                                          dec(SMALL, 603), dec(SMALL, 604), dec(SMALL, 605)))


def sequences() -> Dict[str, Sequence]:
    return {s.name: s for s in (_replay(), _keys(), _walk(), _options(), _regrowth(), _teardown(), _capture())}


# ---- inputs (torch imported on use) -------------------------------------------------------------------------------------------------
def forbid_mask(g: D.Geometry, c: Call):
    """None, the checkpoint's mask, or that mask with a seeded quarter of the word ids flipped ((V,) bool)"""
    if c.forbid < 0:
        return None
    import numpy as np
    import torch
    m = D.weights(g)["model.forbid_rep_mask"].bool().clone()
    if c.forbid > 0:
        rng = np.random.Generator(np.random.PCG64(99000 + 31 * c.forbid + c.seed))
        idx = torch.from_numpy(4 + (rng.random(max(1, g.n_words // 4)) * g.n_words).astype(np.int64))
        m[idx] = ~m[idx]
    return m


def inputs(g: D.Geometry, c: Call):
    """(frame_embs (B, Ta, 768), frame_lens (B,) int32, bos (B,) int64, forbid (V,) bool or None): decoder_geometry.search_inputs
    with this call's mask"""
    fe, shape, bos, _ = D.search_inputs(g, c.search())
    return fe, shape[:, 1].int(), bos, forbid_mask(g, c)


def captions(g: D.Geometry, c: Call):
    """(caps_in, targets) (B, max_pred) int64 of a forcing / score call: the task token, seeded words, <eos> as the last target"""
    import numpy as np
    import torch
    rng = np.random.Generator(np.random.PCG64(98000 + c.seed))
    _, _, bos, _ = D.search_inputs(g, c.search())
    words = torch.from_numpy(4 + (rng.random((c.b, c.max_pred)) * g.n_words).astype(np.int64))
    caps = torch.cat([bos[:, None], words[:, :-1]], dim=1)
    targets = words.clone()
    targets[:, -1] = 2
    return caps, targets
