"""CPU: the sampling rule of conette_amd/sampling.py -- the restatement conette_sample is held to (tests/test_gpu_sample.py).

  * keep rule against the `transformers` warper chain (temperature -> top-k -> top-p) on seeded tie-free logits;
  * the tie-inclusive rule on planted ties, against the definition spelled out as loops;
  * edge uniforms, masks and finished rows on a scripted toy, the chunking plan of Engine.sample."""
import numpy as np
import pytest
import torch

from conette_amd import sampling as S


def _logits(v, seed):
    rng = np.random.Generator(np.random.PCG64(31000 + seed))
    z = (rng.standard_normal(v) * 3.0).astype(np.float32)
    assert len(np.unique(z)) == v, "tie-free"
    return z


@pytest.mark.parametrize("v", (31, 2049))
def test_keep_rule_equals_the_transformers_warper_chain(v):
    from transformers import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    checked = 0
    for seed in range(3):
        z = _logits(v, seed)
        for temp in (0.5, 1.0, 4.0):
            y = z.astype(np.float64) / temp
            for k in (0, 1, 2, 40, v - 1, v, v + 5):
                for p in (1.0, 0.9, 0.3, 1e-6):
                    scores = torch.from_numpy(z.astype(np.float64))[None]
                    if temp != 1.0:
                        scores = TemperatureLogitsWarper(temp)(None, scores)
                    if k > 0:
                        scores = TopKLogitsWarper(top_k=k)(None, scores)
                    if p < 1.0:
                        scores = TopPLogitsWarper(top_p=p)(None, scores)
                    want = torch.isfinite(scores[0]).numpy()
                    got = S.keep_mask(y, k, p)
                    assert np.array_equal(got, want), (v, seed, temp, k, p, int(got.sum()), int(want.sum()))
                    assert got[np.argmax(y)]
                    assert np.array_equal(S.keep_masks(y[None], k, p)[0], got)
                    checked += 1
    assert checked == 3 * 3 * 7 * 4


def _keep_by_definition(y, k, p):
    v = len(y)
    keep = np.isfinite(y)
    if 0 < k < v:
        keep &= np.array([np.sum(y > y[i]) < k for i in range(v)])
    if p < 1.0:
        q = np.where(keep, np.exp(y - y[keep].max()), 0.0)
        q /= q.sum()
        keep &= np.array([np.sum(q[keep & (y > y[i])]) < p for i in range(v)])
    return keep


def test_tie_rule_is_inclusive():
    # ties at the top-k edge: the third and fourth largest are equal -> k = 3 keeps four tokens, k = 2 two
    y = np.array([0.5, 3.0, 2.0, 1.0, 1.0, -1.0, 1.0, -np.inf])
    assert S.keep_mask(y, 2, 1.0).tolist() == [False, True, True, False, False, False, False, False]
    assert S.keep_mask(y, 3, 1.0).tolist() == [False, True, True, True, True, False, True, False]
    assert S.keep_mask(y, 7, 1.0).tolist() == [True] * 7 + [False], "a token of probability zero is never kept"
    # ties at the top-p edge: two equal maxima hold 2 x 0.4 -> with p = 0.3 both are kept (no strictly larger mass), nothing else
    y = np.log(np.array([0.4, 0.1, 0.4, 0.06, 0.04]))
    assert S.keep_mask(y, 0, 0.3).tolist() == [True, False, True, False, False]
    assert S.keep_mask(y, 0, 0.85).tolist() == [True, True, True, False, False]          # 0.8 < 0.85: the 0.1 token stays
    assert S.keep_mask(y, 0, 0.95).tolist() == [True, True, True, True, False]           # 0.9 < 0.95, 0.96 is not
    # top-p renormalises over the top-k set: k = 3 leaves {0.4, 0.4, 0.1} / 0.9 -> mass above the 0.1 token is 0.889
    assert S.keep_mask(y, 3, 0.88).tolist() == [True, False, True, False, False]
    assert S.keep_mask(y, 3, 0.89).tolist() == [True, True, True, False, False]
    rng = np.random.Generator(np.random.PCG64(5))
    for trial in range(40):
        v = int(rng.integers(2, 40))
        y = np.round(rng.standard_normal(v) * 2.0) / 2.0            # a grid: many ties
        if trial % 3 == 0:
            y[rng.integers(0, v)] = -np.inf
        for k in (0, 1, 2, 5, v):
            for p in (1.0, 0.9, 0.5, 0.1):
                want = _keep_by_definition(y, k, p)
                assert np.array_equal(S.keep_mask(y, k, p), want), (trial, k, p)
                assert np.array_equal(S.keep_masks(np.stack([y, y[::-1]]), k, p)[0], want), (trial, k, p)
                assert want[np.argmax(y)]


def test_edge_uniforms():
    z = _logits(31, 7)
    for k, p in ((0, 1.0), (5, 1.0), (0, 0.6), (7, 0.8)):
        keep = S.keep_mask(z.astype(np.float64), k, p)
        ids = np.nonzero(keep)[0]
        tok, lp = S.decide(z, [9], 4, 0.0, top_k=k, top_p=p)
        assert tok == ids[0], "u = 0: the lowest kept id"
        assert np.isclose(lp, S.log_softmax(z.astype(np.float64))[tok])
        tok, _ = S.decide(z, [9], 4, 1.0 - 2.0 ** -24, top_k=k, top_p=p)
        assert keep[tok]
        q = S.kept_probs(z.astype(np.float64), 1.0, k, p)
        assert S.draw(q, keep, 1.0) == ids[-1], "rounding left the total <= u: the largest kept id"
        c = np.cumsum(q)
        for u in (0.25, 0.5, 0.75):
            tok, _ = S.decide(z, [9], 4, u, top_k=k, top_p=p)
            assert keep[tok] and c[tok] > u and c[tok] - q[tok] <= u


def test_masks_and_finished_rows_on_a_scripted_toy():
    """V = 7, pad 0, bos 1, eos 2; top_k = 1 makes every draw the arg-max of the masked logits whatever u is."""
    eos, pad, v = 2, 0, 7
    forbid = np.zeros(v, dtype=bool)
    forbid[[4, 6]] = True
    NEG = -np.inf
    script = {
        # row 0 (prompt 6, a forbidden token): eos floored at step 0 -> 4; 4 repeats -> masked, 6 is in the prefix at position 0 -> 5; eos
        0: [[0, 0, 9, 1, 8, 2, 3], [0, 0, 1, 2, 9, 7, 8], [0, 0, 9, 1, 1, 1, 1]],
        # row 1: 3, then eos at step 1 (min_pred = 1 no longer floors it); step 2 is never asked for
        1: [[0, 0, 1, 9, 2, 1, 1], [0, 0, 9, 8, 1, 1, 1], None],
        # row 2: never draws eos: ends at max_pred - 1 with the drawn token kept; 3 is not forbidden and may repeat
        2: [[0, 0, 1, 9, 1, 1, 1], [0, 0, 1, 9, 1, 1, 1], [0, 0, 1, 9, 8, 1, 1]],
        # row 3: no finite logit at step 1 -> eos, NaN, finished
        3: [[0, 0, 1, 1, 1, 9, 1], [NEG] * 7, None],
    }
    asked = []

    def logits_fn(r, prefix, step):
        asked.append((r, step))
        assert len(prefix) == step + 1
        return np.array(script[r][step], dtype=np.float64)

    u = np.full((3, 4), 0.37)
    out = S.sample_rows(logits_fn, [6, 1, 1, 1], u, max_pred=3, min_pred=1, eos_id=eos, pad_id=pad, forbid=forbid, top_k=1)
    assert out["preds"].tolist() == [[4, 5, 2], [3, 2, pad], [3, 3, 3], [5, 2, pad]]
    assert out["lens"].tolist() == [3, 2, 3, 2] and out["sizes"].tolist() == [3, 3]
    assert (1, 2) not in asked and (3, 2) not in asked, "a finished row takes no further decision"
    lp = out["tok_lprobs"]
    assert lp[1, 2] == 0.0 and np.isnan(lp[3, 1]) and np.isnan(out["sum_lprobs"][3])
    # reported log-probs: log_softmax of the MASKED logits, temperature 1, unfiltered
    z = np.array(script[0][1], dtype=np.float64)
    z[[4, 6]] = NEG
    assert np.isclose(lp[0, 1], S.log_softmax(z)[5])
    z = np.array(script[0][0], dtype=np.float64)
    z[[eos, 6]] = NEG                     # the EOS floor, and the prompt itself is a forbidden token in the prefix
    assert np.isclose(lp[0, 0], S.log_softmax(z)[4])
    assert np.isclose(out["sum_lprobs"][0], lp[0].sum())
    # temperature and filters do not change the reported quantity
    t1, l1 = S.decide(script[2][2], [1, 3, 3], 2, 0.0, min_pred=1, eos_id=eos, forbid=forbid, temperature=4.0, top_k=1)
    assert (t1, l1) == (3, lp[2, 2])


def test_chunking_plan():
    assert S.plan_sample_chunks(1) == [(0, 1)]
    assert S.plan_sample_chunks(16) == [(0, 16)]
    assert S.plan_sample_chunks(17) == [(0, 16), (16, 1)]
    assert S.plan_sample_chunks(40) == [(0, 16), (16, 16), (32, 8)]
    for n in (1, 16, 17, 40):
        plan = S.plan_sample_chunks(n)
        assert sum(c for _, c in plan) == n and all(1 <= c <= S.MAX_SAMPLES_PER_CALL for _, c in plan)
        assert [f for f, _ in plan] == list(np.cumsum([0] + [c for _, c in plan[:-1]]))
    with pytest.raises(ValueError):
        S.plan_sample_chunks(0)
