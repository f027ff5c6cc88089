"""Sequence log-likelihoods: the definition (numpy float64, no GPU needed) of what dimx_op_seq_logprob / dimx_op_score_select
compute (csrc/seq_score.hip, include/dimx.h).

The score of a token sequence is sum_c log softmax(logits[c])[token[c]] over the scored columns: the model's own verdict on a
sampled sequence, the standard reranking score of an autoregressive sampler, and with the number of scored tokens a perplexity.
Within a clip all tries share their scored columns, so the sum and the per-token mean rank them alike: there is one criterion.
"""
import math
from collections import namedtuple

import numpy as np

VOCAB = 512
SeqScores = namedtuple("SeqScores", "score count")


def token_logprob(logits, tokens):
    """logits [R, n, 512], tokens [R, n] -> float64 [R, n]: logits[r, c, tok] - logsumexp(logits[r, c, :]) on float64 copies of the
    values, 0.0 where the token is outside [0, 512) (the -100 padding of forward_vq is skipped, as ce_argmax_kernel skips it)."""
    x = np.asarray(logits, dtype=np.float64)
    tok = np.asarray(tokens).astype(np.int64)
    assert x.ndim == 3 and x.shape[2] == VOCAB and tok.shape == x.shape[:2], (x.shape, tok.shape)
    m = x.max(axis=2)
    lse = m + np.log(np.exp(x - m[..., None]).sum(axis=2))
    valid = (tok >= 0) & (tok < VOCAB)
    picked = np.take_along_axis(x, np.where(valid, tok, 0)[..., None], axis=2)[..., 0]
    return np.where(valid, picked - lse, 0.0)


def _per_clip(v, n_clips, default):
    if v is None:
        return np.full(n_clips, default, dtype=np.int64)
    v = np.asarray(v).astype(np.int64).reshape(-1)
    assert v.shape[0] == n_clips, "%d entries for %d clips" % (v.shape[0], n_clips)
    return v


def sequence_scores(logits, tokens, first=None, last=None, rows_per_clip=1):
    """-> SeqScores(score float64 [R], count int32 [R]).  Row r belongs to clip r // rows_per_clip and sums the columns
    clamp(first[clip], 0, n) <= c < clamp(last[clip], 0, n) whose token is in range; count is how many were summed.  None is 0 for
    ``first`` and n for ``last``; an empty range gives (0.0, 0)."""
    tok = np.asarray(tokens).astype(np.int64)
    R, n = tok.shape
    assert rows_per_clip >= 1 and R % rows_per_clip == 0, "R=%d is not a multiple of rows_per_clip=%d" % (R, rows_per_clip)
    clips = R // rows_per_clip
    c0 = np.repeat(np.clip(_per_clip(first, clips, 0), 0, n), rows_per_clip)
    c1 = np.repeat(np.clip(_per_clip(last, clips, n), 0, n), rows_per_clip)
    cols = np.arange(n)[None, :]
    use = (cols >= c0[:, None]) & (cols < c1[:, None]) & (tok >= 0) & (tok < VOCAB)
    lp = token_logprob(logits, np.where(use, tok, -1))
    return SeqScores(lp.sum(axis=1), use.sum(axis=1).astype(np.int32))


def pick(score):
    """score [B, S] -> (win int32 [B], ok bool [B]): the first maximum of the row with NaN counting as -inf; ok is False when no
    try of the clip has a finite score."""
    s = np.asarray(score, dtype=np.float64)
    assert s.ndim == 2
    win = np.where(np.isnan(s), -np.inf, s).argmax(axis=1).astype(np.int32)
    return win, np.isfinite(s).any(axis=1)


def scored_columns(T, n, lens, plen=None):
    """Which columns of a generation count -> (first, last), the one place that says so.  ``n`` columns were generated for clips of
    ``T`` frames and column c is position c + 1: last = lens - (T - n), that is len - 1 for SLMFT's n = T - 1 and len
    for the legacy decoder's n = T -- the columns evaluate_test_epoch keeps (``y_preds[j][:src_len[j] - 1]``).  first = plen - 1 (0
    without a prompt): a prompt's forced tokens were not sampled and are not scored.  ``lens`` / ``plen``: numpy arrays, torch
    tensors (the arithmetic stays on their device) or sequences."""
    if isinstance(lens, (list, tuple)):
        lens = np.asarray(lens, dtype=np.int64)
    if isinstance(plen, (list, tuple)):
        plen = np.asarray(plen, dtype=np.int64)
    last = lens - (int(T) - int(n))
    first = last * 0 if plen is None else plen - 1
    return first, last


def perplexity(scores):
    """exp(-sum score / sum count) of a SeqScores (numpy arrays or tensors); NaN when nothing was scored."""
    s, c = float(scores.score.sum()), float(scores.count.sum())
    return math.exp(-s / c) if c > 0 else float("nan")
