"""Consensus (minimum-Bayes-risk, medoid) best-of-N selection: the definition (numpy float64, no GPU needed) of what
dimx_op_consensus_select computes (csrc/consensus.hip, include/dimx.h).

Of the S tries of a clip the one with the smallest total distance to the other S - 1 is kept: the candidate the others agree with
most.  No ground truth enters, and unlike the likelihood pick (dimx.scoring) the rule has no preference for the modal, low-motion
sequence.  The distance is the protocol's own metric, the Frechet distance of the coefficients (dimx.metrics.clip_fd), or the mean
squared difference.
"""
import numpy as np

KINDS = {"fd": 0, "l2": 1}


def kind_index(distance):
    """"fd" / "l2" -> the ``kind`` of dimx_op_consensus_select; anything else raises ValueError"""
    if distance not in KINDS:
        raise ValueError("consensus distance %r: one of 'fd', 'l2'" % (distance,))
    return KINDS[distance]


def _window(tries, n, cols):
    x = np.asarray(tries)
    assert x.ndim == 3, "tries [S, L, W] expected, got %s" % (x.shape,)
    c0 = int(cols[0])
    c1 = x.shape[2] if cols[1] is None else int(cols[1])
    n = min(max(int(n), 0), x.shape[1])
    return x[:, :n, c0:c1], n


def _pairwise(tries, n, cols, dist):
    x, n = _window(tries, n, cols)
    S = x.shape[0]
    D = np.zeros((S, S), dtype=np.float64)
    for i in range(S):
        for j in range(i + 1, S):
            D[i, j] = D[j, i] = dist(x[i], x[j]) if n >= 2 else np.nan
    return D


def pairwise_fd(tries, n, cols=(0, None)):
    """tries [S, L, W], the first ``n`` frames and the columns cols = (c0, c1) (None = the row's end) -> D float64 [S, S]:
    D[i, j] for i < j is dimx.metrics.clip_fd(tries[i], tries[j]), the try with the lower index as the first operand; D[j, i] is
    that same value (scipy's own d(i, j) and d(j, i) differ in the last digits: mirroring is part of the definition) and
    D[i, i] = 0.  Nothing is clamped at 0, as in the reference's calculate_frechet_distance.  With fewer than 2 valid frames there
    is no covariance: every distance off the diagonal is NaN."""
    from .metrics import clip_fd
    return _pairwise(tries, n, cols, lambda a, b: float(np.real(clip_fd(a, b))))


def pairwise_l2(tries, n, cols=(0, None)):
    """The same matrix with D[i, j] = the mean over the valid frames and the window's columns of (x_i - x_j)^2 in float64."""
    return _pairwise(tries, n, cols, lambda a, b: float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


def pairwise(tries, n, cols=(0, None), distance="fd"):
    kind_index(distance)
    return (pairwise_fd if distance == "fd" else pairwise_l2)(tries, n, cols)


def risks(D):
    """D [..., S, S] -> risk [..., S]: risk[i] = sum over j != i of D[i, j], added in ascending j starting from zero."""
    D = np.asarray(D, dtype=np.float64)
    S = D.shape[-1]
    assert D.ndim >= 2 and D.shape[-2] == S, D.shape
    risk = np.zeros(D.shape[:-1], dtype=np.float64)
    for j in range(S):
        risk += np.where(np.arange(S) == j, 0.0, D[..., j])
    return risk


def pick(risk):
    """risk [B, S] (or [S]) -> (win int32, ok bool): the first minimum of the row with NaN counting as +inf; ok is False when no
    risk of the clip is finite.  S = 1 has risk 0: try 0 wins with ok True."""
    r = np.asarray(risk, dtype=np.float64)
    win = np.where(np.isnan(r), np.inf, r).argmin(axis=-1).astype(np.int32)
    return win, np.isfinite(r).any(axis=-1)


def margins(risk):
    """risk [B, S] (or [S]) -> the relative gap between the two smallest risks of each row, (second - first) / |first|: a clip whose
    margin is below the error of an evaluation of the distances may legitimately get another winner there -- what
    sampling.undecidable is to the sampler and beam.margins to the beam.  inf for S = 1; NaN risks count as +inf (a row with fewer
    than two finite risks gives inf, or NaN when none is finite)."""
    r = np.asarray(risk, dtype=np.float64)
    r = np.where(np.isnan(r), np.inf, r)
    if r.shape[-1] < 2:
        return np.full(r.shape[:-1], np.inf)
    two = np.partition(r, 1, axis=-1)[..., :2]
    with np.errstate(invalid="ignore", divide="ignore"):
        return (two[..., 1] - two[..., 0]) / np.abs(two[..., 0])


def select(tries, n, cols=(0, None), distance="fd"):
    """One clip from end to end -> (D [S, S], risk [S], win, ok)."""
    D = pairwise(tries, n, cols, distance)
    risk = risks(D)
    win, ok = pick(risk)
    return D, risk, int(win), bool(ok)
