"""CPU: the definition of the sequence log-likelihood (dimx.scoring) against scipy's log_softmax, its range / skip / pick rules,
the scored columns of both decoder geometries, the C-ABI surface of the two operators, and the refusals of
evaluate_test_epoch(select=...) that need no GPU."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stub_model  # noqa: E402

import dimx  # noqa: E402,F401
from dimx import lib, prng, scoring  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, S, N = 5, 10, 39
R = B * S
LAST = [39, 33, 7, 1, 0]
FIRST = [0, 5, 6, 0, 0]


def _case(scale):
    logits = (prng.normal(21, "score.logits", (R, N, 512)) * scale).astype(np.float32)
    tokens = prng.integers(21, "score.tok", (R, N), 0, 512)
    return logits, tokens


@pytest.fixture(scope="module", params=[1, 3])
def case(request):
    from scipy.special import log_softmax
    logits, tokens = _case(request.param)
    ref = np.take_along_axis(log_softmax(logits.astype(np.float64), axis=2), tokens[..., None].astype(np.int64), axis=2)[..., 0]
    return request.param, logits, tokens, ref


def test_token_logprob_is_log_softmax_at_the_token(case):
    _, logits, tokens, ref = case
    lp = scoring.token_logprob(logits, tokens)
    assert lp.dtype == np.float64 and lp.shape == (R, N)
    assert np.abs(lp - ref).max() < 1e-12


def test_sequence_scores_sum_the_scored_columns(case):
    scale, logits, tokens, ref = case
    sc = scoring.sequence_scores(logits, tokens, FIRST, LAST, rows_per_clip=S)
    assert isinstance(sc, scoring.SeqScores) and sc.score.dtype == np.float64 and sc.count.dtype == np.int32
    for r in range(R):
        c0, c1 = FIRST[r // S], LAST[r // S]
        assert sc.count[r] == max(c1 - c0, 0)
        assert abs(sc.score[r] - ref[r, c0:c1].sum()) < 1e-11
    # an empty range gives (0.0, 0)
    assert (sc.score[4 * S:] == 0.0).all() and (sc.count[4 * S:] == 0).all()
    # the case's own premise (the GPU test leaves no clip out of the selection because of it): the top two scores of every
    # non-empty clip are well apart
    top = np.sort(sc.score.reshape(B, S)[:4], axis=1)
    assert (top[:, -1] - top[:, -2]).min() >= (0.45 if scale == 1 else 1.38)


def test_range_and_skip_rules():
    logits, tokens = _case(1)
    lp = scoring.token_logprob(logits, tokens)
    # first >= last
    sc = scoring.sequence_scores(logits, tokens, [7] * B, [7, 6, 0, -3, 7], rows_per_clip=S)
    assert (sc.score == 0.0).all() and (sc.count == 0).all()
    # -100 and 512 are skipped and not counted; 0 and 511 are tokens
    tok = tokens.copy()
    tok[0, 3], tok[0, 4], tok[1, 0], tok[1, 38] = -100, 512, 0, 511
    lp2 = scoring.token_logprob(logits, tok)
    assert lp2[0, 3] == 0.0 and lp2[0, 4] == 0.0 and lp2[1, 0] != 0.0 and lp2[1, 38] != 0.0
    sc = scoring.sequence_scores(logits, tok)
    assert sc.count[0] == N - 2 and sc.count[1] == N
    assert abs(sc.score[0] - (lp[0].sum() - lp[0, 3] - lp[0, 4])) < 1e-11
    # clamping: first below 0 and last beyond n are the row's ends; None is (0, n)
    a = scoring.sequence_scores(logits, tokens, [-5] * R, [N + 9] * R)
    b = scoring.sequence_scores(logits, tokens)
    assert np.array_equal(a.score, b.score) and (a.count == N).all() and np.array_equal(a.count, b.count)
    assert np.abs(b.score - lp.sum(1)).max() < 1e-11
    # per-row ranges with rows_per_clip = 1
    c = scoring.sequence_scores(logits[:3], tokens[:3], [0, 38, 2], [1, 39, 4])
    assert list(c.count) == [1, 1, 2]
    assert abs(c.score[0] - lp[0, 0]) < 1e-13 and abs(c.score[1] - lp[1, 38]) < 1e-13 and abs(c.score[2] - lp[2, 2:4].sum()) < 1e-12
    with pytest.raises(AssertionError):
        scoring.sequence_scores(logits[:7], tokens[:7], rows_per_clip=2)


def test_pick_first_maximum_nan_as_minus_inf():
    nan, inf = float("nan"), float("inf")
    score = np.array([[-3.0, -1.0, -1.0, -2.0],
                      [nan, -5.0, nan, -4.0],
                      [nan, nan, nan, nan],
                      [-inf, -inf, -inf, -inf],
                      [nan, -inf, -7.0, nan],
                      [0.0, 0.0, 0.0, 0.0]])
    win, ok = scoring.pick(score)
    assert win.dtype == np.int32 and list(win) == [1, 3, 0, 0, 2, 0]
    assert list(ok) == [True, True, False, False, True, True]


def test_scored_columns_of_both_geometries():
    lens = np.array([40, 33, 7, 1, 0])
    # SLMFT: n = T - 1 columns, column c is position c + 1: the len - 1 columns evaluate_test_epoch keeps
    first, last = scoring.scored_columns(40, 39, lens)
    assert list(first) == [0] * 5 and list(last) == [39, 32, 6, 0, -1]
    # the legacy decoder generates n = T tokens
    first, last = scoring.scored_columns(40, 40, lens)
    assert list(first) == [0] * 5 and list(last) == [40, 33, 7, 1, 0]
    # a prompt's forced tokens are not scored
    first, last = scoring.scored_columns(40, 39, lens, np.array([16, 9, 7, 1, 1]))
    assert list(first) == [15, 8, 6, 0, 0] and list(last) == [39, 32, 6, 0, -1]
    # lists and tensors alike
    first, last = scoring.scored_columns(40, 39, [40, 33], [16, 9])
    assert list(first) == [15, 8] and list(last) == [39, 32]
    ft, lt = scoring.scored_columns(40, 39, torch.tensor([40, 33], dtype=torch.int32), torch.tensor([16, 9], dtype=torch.int32))
    assert ft.tolist() == [15, 8] and lt.tolist() == [39, 32] and lt.dtype == torch.int32
    # counts of a clip: len - plen, clamped at 0
    sc = scoring.sequence_scores(np.zeros((3, 39, 512), np.float32), np.zeros((3, 39), np.int64),
                                 *scoring.scored_columns(40, 39, [40, 33, 7], [16, 9, 7]))
    assert list(sc.count) == [24, 24, 0]


def test_perplexity():
    sc = scoring.SeqScores(np.array([-2.0, -4.0, 0.0]), np.array([1, 2, 0], dtype=np.int32))
    assert abs(scoring.perplexity(sc) - np.exp(2.0)) < 1e-12
    uniform = scoring.sequence_scores(np.zeros((2, 5, 512), np.float32), np.zeros((2, 5), np.int64))
    assert abs(scoring.perplexity(uniform) - 512.0) < 1e-9
    assert np.isnan(scoring.perplexity(scoring.SeqScores(np.zeros(2), np.zeros(2, dtype=np.int32))))


def test_operators_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "dimx.h")).read()
    l = lib.load()
    for name in ("dimx_op_seq_logprob", "dimx_op_score_select"):
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in lib.SIGNATURES and hasattr(l, name)
    assert len(lib.SIGNATURES["dimx_op_seq_logprob"][1]) == 14 and len(lib.SIGNATURES["dimx_op_score_select"][1]) == 18
    # refused before anything touches a device: null operands, and R not a multiple of rows_per_clip
    assert l.dimx_op_seq_logprob(None, 512 * N, 512, None, N, None, None, 1, R, N, None, None, None, None) == -1
    assert l.dimx_op_score_select(None, None, 0, 0, 0, None, None, 0, B, S, N, 56, N, None, None, None, None, None) == -1


def test_likelihood_selection_refuses_a_cpu_device_and_unknown_values():
    from dimx import x_engine_pt
    with pytest.raises(lib.DimxError):
        x_engine_pt.evaluate_test_epoch(stub_model.StubSLMFT(), stub_model.protocol_batches(), torch.device("cpu"), beam_size=5,
                                        select="likelihood")
    with pytest.raises(ValueError):
        x_engine_pt.evaluate_test_epoch(stub_model.StubSLMFT(), stub_model.protocol_batches(), torch.device("cpu"), beam_size=5,
                                        select="nonsense")


def test_gpu_only_operators_refuse_cpu_tensors():
    from dimx import engine
    with pytest.raises(lib.DimxError):
        engine.op_seq_logprob(torch.zeros(2, 3, 512), torch.zeros(2, 3, dtype=torch.int32))
    with pytest.raises(lib.DimxError):
        engine.op_score_select(torch.zeros(2, 3, dtype=torch.float64), torch.zeros(2, 3, 4, 56), [4, 4])
