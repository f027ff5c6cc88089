"""CPU: the definition of beam search (dimx.beam, numpy float64) -- one step in its three modes, the tie-break, the -inf start,
the loop against a brute-force optimum on a toy model, and the margins."""
import itertools

import numpy as np

import dimx  # noqa: F401
from dimx import beam, scoring


def _logits(seed, W, V=512, scale=1.0):
    return (np.random.default_rng(seed).standard_normal((W, V)) * scale).astype(np.float32)


def test_width_one_is_the_argmax():
    lg = _logits(0, 1)
    parent, tok, cum = beam.beam_step(lg, np.array([-1.5]))
    assert parent.tolist() == [0] and tok.tolist() == [int(lg[0].argmax())]
    lp = scoring.token_logprob(lg[None], tok[None])[0, 0]
    assert abs(cum[0] - (-1.5 + lp)) < 1e-13


def test_live_step_keeps_the_w_largest_in_order():
    W = 4
    lg, cum = _logits(1, W, scale=3.0), np.array([-2.0, -2.5, -1.0, -7.0])
    parent, tok, new = beam.beam_step(lg, cum)
    sc = cum[:, None] + beam.log_softmax(lg)
    want = np.sort(sc.reshape(-1))[::-1][:W]
    assert np.array_equal(new, want) and (np.diff(new) <= 0).all()
    assert np.array_equal(sc[parent, tok], new)
    assert parent.dtype == np.int32 and tok.dtype == np.int32


def test_ties_go_to_the_smaller_flat_index():
    lg = np.zeros((2, 4), dtype=np.float32)          # every candidate of both beams ties
    parent, tok, new = beam.beam_step(lg, np.zeros(2))
    assert parent.tolist() == [0, 0] and tok.tolist() == [0, 1]
    lg[1, 3] = lg[0, 2] = 1.0                        # two tied maxima: beam 0's comes first
    parent, tok, _ = beam.beam_step(lg, np.zeros(2))
    assert list(zip(parent.tolist(), tok.tolist())) == [(0, 2), (1, 3)]


def test_minus_inf_start_expands_beam_zero_only():
    W = 5
    lg = _logits(2, W)
    parent, tok, new = beam.beam_step(lg, beam.start_scores(W))
    assert parent.tolist() == [0] * W
    assert tok.tolist() == np.argsort(-lg[0].astype(np.float64), kind="stable")[:W].tolist()
    assert np.isfinite(new).all()


def test_forced_and_frozen_modes():
    W = 4
    lg, cum = _logits(3, W), np.array([-1.0, -2.0, -np.inf, -3.0])
    parent, tok, new = beam.beam_step(lg, cum, beam.FORCED, 77)
    assert parent.tolist() == list(range(W)) and tok.tolist() == [77] * W and np.array_equal(new, cum)
    parent, tok, new = beam.beam_step(lg, cum, beam.FROZEN)
    assert parent.tolist() == list(range(W)) and tok.tolist() == lg.argmax(1).tolist() and np.array_equal(new, cum)
    assert [beam.column_mode(c, 2, 5) for c in range(7)] == [beam.FORCED] * 2 + [beam.LIVE] * 3 + [beam.FROZEN] * 2


class _Toy:
    """logits as a function of the whole prefix (a table drawn once), rows reordered by the parents the search hands over"""
    V, N = 4, 4

    def __init__(self, seed):
        rng = np.random.default_rng(seed)
        self.table = {p: rng.standard_normal(self.V).astype(np.float32) * 2
                      for k in range(self.N) for p in itertools.product(range(self.V), repeat=k + 1)}

    def step_fn(self):
        state = {"prefix": None}

        def fn(c, inputs, parent):
            prev = [()] * len(inputs) if parent is None else [state["prefix"][p] for p in parent]
            state["prefix"] = [p + (int(t),) for p, t in zip(prev, inputs)]
            return np.stack([self.table[p] for p in state["prefix"]])
        return fn

    def score(self, start, seq):
        total, prefix = 0.0, (start,)
        for t in seq:
            total += beam.log_softmax(self.table[prefix])[t]
            prefix += (t,)
        return total


def test_beam_search_finds_the_brute_force_optimum_when_nothing_is_pruned():
    toy, start = _Toy(4), 1
    every = {seq: toy.score(start, seq) for seq in itertools.product(range(toy.V), repeat=toy.N)}
    best_seq = max(every, key=every.get)
    tokens, scores, backptr = beam.beam_search(toy.step_fn(), start, toy.N, 256)
    assert tuple(tokens[0]) == best_seq and abs(scores[0] - every[best_seq]) < 1e-12
    assert (np.diff(scores) <= 0).all()
    assert sorted(map(tuple, tokens.tolist())) == sorted(every)          # all 256 sequences, each once
    for w in (0, 17, 255):
        assert abs(scores[w] - every[tuple(tokens[w])]) < 1e-12
    for W in (1, 2, 8):
        t, s, _ = beam.beam_search(toy.step_fn(), start, toy.N, W)
        assert s[0] <= every[best_seq] + 1e-12 and abs(s[0] - every[tuple(t[0])]) < 1e-12


def test_back_pointers_and_the_column_range():
    toy, start, W = _Toy(5), 2, 3
    rows = []
    inner = toy.step_fn()

    def fn(c, inputs, parent):
        rows.append((np.array(inputs), parent))
        return inner(c, inputs, parent)
    prompt = [start, 3, 0]
    tokens, scores, backptr = beam.beam_search(fn, start, toy.N, W, first=1, last=3, prompt=prompt)
    assert (tokens[:, 0] == 3).all()
    # backptr[w, c] is the row that ran step c: the token hypothesis w consumed at step c + 1 sat in that row's successor
    for w in range(W):
        for c in range(1, toy.N):
            assert rows[c][0][backptr[w, c]] == tokens[w, c - 1]
    # only the live columns 1, 2 were scored
    for w in range(W):
        want = sum(beam.log_softmax(toy.table[(start,) + tuple(tokens[w, :c])])[tokens[w, c]] for c in (1, 2))
        assert abs(scores[w] - want) < 1e-12


def test_margins_agree_with_a_direct_computation():
    W = 4
    lg, cum = _logits(6, W, scale=3.0), np.array([-2.0, -2.5, -1.0, -7.0])
    sc = np.sort((cum[:, None] + beam.log_softmax(lg)).reshape(-1))[::-1]
    keep, order = beam.margins(lg, cum)
    assert keep == sc[W - 1] - sc[W] and order == min(sc[i] - sc[i + 1] for i in range(W - 1))
    assert beam.margins(lg[:1], cum[:1])[1] == np.inf
    keep, order = beam.margins(lg, beam.start_scores(W))      # beam 0 alone: its 4th against its 5th logit
    row = np.sort(beam.log_softmax(lg[0]))[::-1]
    assert keep == row[3] - row[4] and order == min(row[i] - row[i + 1] for i in range(3))
    assert beam.margins(np.zeros((2, 4), np.float32), np.zeros(2)) == (0.0, 0.0)
