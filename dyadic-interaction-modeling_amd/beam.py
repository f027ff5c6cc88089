"""Beam search: the definition (numpy float64, no GPU needed) of what dimx_generate_beam / dimx_op_beam_step compute
(csrc/beam.hip, include/dimx.h).

W hypotheses per clip are extended one column per step.  A candidate (w, v) scores cum[w] + log softmax(logits[w])[v] on float64
copies of the raw f32 logits -- the per-token term of dimx.scoring, no temperature and no filter -- and the W largest survive in
descending order, ties to the smaller flat index w * V + v.  A search starts from cum = (0, -inf, ...), so the first live step
expands hypothesis 0 alone.  Columns inside a prompt are *forced*, columns at or past the clip's last scored column are *frozen*
(every hypothesis follows its own arg-max); neither changes a score.  Which columns those are is said once, by
dimx.scoring.scored_columns.  There is no end token and no length penalty: all hypotheses of a clip have one length.
"""
import numpy as np

LIVE, FORCED, FROZEN = 0, 1, 2


def log_softmax(logits):
    """logits [..., V] -> float64 logits - logsumexp(logits) over the last axis (the definition of dimx.scoring.token_logprob)"""
    x = np.asarray(logits, dtype=np.float64)
    m = x.max(axis=-1, keepdims=True)
    return x - (m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True)))


def _ranked(logits, cum):
    """every candidate of a live step, best first -> (flat indices, scores), ties to the smaller flat index"""
    sc = (np.asarray(cum, dtype=np.float64)[:, None] + log_softmax(logits)).reshape(-1)
    order = np.lexsort((np.arange(sc.size), -sc))
    return order, sc[order]


def beam_step(logits, cum, mode=LIVE, forced_tok=0):
    """logits [W, V] f32, cum [W] f64 -> (parent [W] int32, token [W] int32, cum' [W] f64) for one clip and one column."""
    logits = np.asarray(logits)
    cum = np.asarray(cum, dtype=np.float64)
    W, V = logits.shape
    assert cum.shape == (W,)
    ident = np.arange(W, dtype=np.int32)
    if mode == FORCED:
        return ident, np.full(W, forced_tok, dtype=np.int32), cum.copy()
    if mode == FROZEN:
        return ident, logits.argmax(axis=1).astype(np.int32), cum.copy()
    assert mode == LIVE, mode
    order, sc = _ranked(logits, cum)
    keep = order[:W]
    return (keep // V).astype(np.int32), (keep % V).astype(np.int32), sc[:W].copy()


def margins(logits, cum):
    """The two gaps that decide a live step -> (keep, order): score of the W-th minus the (W+1)-th candidate (inf when there is
    none), and the smallest gap between adjacent kept candidates (inf for W = 1).  A step whose gaps are below the error of an
    evaluation may legitimately come out differently there -- what sampling.undecidable is to the sampler."""
    W = np.asarray(logits).shape[0]
    _, sc = _ranked(logits, cum)
    with np.errstate(invalid="ignore"):
        keep = sc[W - 1] - sc[W] if sc.size > W else np.inf
        gaps = sc[:W - 1] - sc[1:W]
    keep = np.inf if np.isnan(keep) else keep   # -inf against -inf: the cut falls among candidates that cannot survive anyway
    gaps = gaps[~np.isnan(gaps)]
    return float(keep), float(gaps.min()) if gaps.size else np.inf


def start_scores(W):
    cum = np.full(W, -np.inf)
    cum[0] = 0.0
    return cum


def column_mode(c, first, last):
    """the mode of column c of a clip whose scored columns are first <= c < last (dimx.scoring.scored_columns)"""
    return FORCED if c < first else (FROZEN if c >= last else LIVE)


def beam_search(step_logits_fn, start, n, W, first=0, last=None, prompt=None):
    """One clip.  ``step_logits_fn(c, inputs [W] int, parent [W] int or None) -> logits [W, V]`` runs step c: ``inputs`` are the
    tokens the W rows consume, ``parent`` the permutation the previous selection applied to the rows (None at the first step) --
    a stateful model reorders its caches by it.  ``start``: the first input token; ``prompt`` [>= first + 1]: the forced columns
    c < first take prompt[c + 1].  Returns (tokens [W, n], scores [W], backptr [W, n]): whole hypotheses, best first;
    backptr[w, c] is the row that ran step c on hypothesis w's path."""
    last = n if last is None else last
    tokens = np.zeros((W, n), dtype=np.int32)
    backptr = np.zeros((W, n), dtype=np.int32)
    cum = start_scores(W)
    inputs, parent = np.full(W, start, dtype=np.int64), None
    for c in range(n):
        logits = step_logits_fn(c, inputs, parent)
        mode = column_mode(c, first, last)
        parent, tok, cum = beam_step(logits, cum, mode, int(prompt[c + 1]) if mode == FORCED else 0)
        tokens, backptr = tokens[parent], backptr[parent]
        tokens[:, c], backptr[:, c] = tok, parent
        inputs = tok.astype(np.int64)
    return tokens, cum, backptr
