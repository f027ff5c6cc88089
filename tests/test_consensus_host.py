"""Host: the definition of consensus (minimum-Bayes-risk) selection, dimx/consensus.py, and what of dimx_op_consensus_select can be
checked without a GPU (the exported symbols, the workspace size, the refusals of the Python layer)."""
import functools

import numpy as np
import pytest
import torch


@functools.lru_cache(maxsize=None)
def _tries():
    """one clip: 5 tries of 40 frames x 12 columns around a common signal"""
    g = torch.Generator().manual_seed(21)
    base = torch.randn(40, 12, generator=g)
    x = (0.6 * base[None] + 0.5 * torch.randn(5, 40, 12, generator=g)).numpy()
    x.setflags(write=False)
    return x


def test_pairwise_fd_is_the_double_loop_over_clip_fd():
    from dimx import consensus, metrics
    x = _tries()
    n, (c0, c1) = 33, (2, 11)
    D = consensus.pairwise_fd(x, n, (c0, c1))
    S = x.shape[0]
    for i in range(S):
        for j in range(S):
            lo, hi = min(i, j), max(i, j)
            want = 0.0 if i == j else metrics.clip_fd(x[lo, :n, c0:c1], x[hi, :n, c0:c1])
            assert D[i, j] == want, (i, j)
    assert np.isfinite(D).all() and (D[~np.eye(S, dtype=bool)] > 0).all()


@pytest.mark.parametrize("distance", ["fd", "l2"])
def test_symmetry_zero_diagonal_and_permutation(distance):
    from dimx import consensus
    x = _tries()
    D = consensus.pairwise(x, 40, (0, None), distance)
    assert np.array_equal(D, D.T) and not np.diagonal(D).any()
    risk = consensus.risks(D)
    assert np.array_equal(risk, np.array([sum(D[i, j] for j in range(5) if j != i) for i in range(5)]))
    perm = np.array([3, 0, 4, 1, 2])
    rp = consensus.risks(consensus.pairwise(x[perm], 40, (0, None), distance))
    # the same pairs in another operand and summation order: scipy's d(i, j) and d(j, i) differ by about 1e-14 relative
    assert np.allclose(rp, risk[perm], rtol=1e-9, atol=0.0)
    assert int(consensus.pick(rp)[0]) == int(np.where(perm == consensus.pick(risk)[0])[0][0])


def test_l2_is_the_mean_squared_difference():
    from dimx import consensus
    x = _tries()
    D = consensus.pairwise_l2(x, 17, (3, 9))
    a, b = x[1, :17, 3:9].astype(np.float64), x[4, :17, 3:9].astype(np.float64)
    assert D[1, 4] == D[4, 1] == np.mean((a - b) ** 2)


@pytest.mark.parametrize("distance", ["fd", "l2"])
def test_single_try_and_short_clips(distance):
    from dimx import consensus
    x = _tries()
    D, risk, win, ok = consensus.select(x[:1], 40, (0, None), distance)
    assert D.shape == (1, 1) and D[0, 0] == 0.0 and risk.tolist() == [0.0] and win == 0 and ok
    assert consensus.margins(risk) == np.inf
    for n in (0, 1):
        D, risk, win, ok = consensus.select(x, n, (0, None), distance)
        assert np.isnan(D[~np.eye(5, dtype=bool)]).all() and not np.diagonal(D).any()
        assert np.isnan(risk).all() and win == 0 and not ok


def test_pick_takes_the_first_minimum_and_nan_counts_as_inf():
    from dimx import consensus
    nan, inf = float("nan"), float("inf")
    risk = np.array([[3.0, 1.0, 1.0, 2.0], [nan, 5.0, nan, 4.0], [nan, nan, nan, nan], [inf, nan, inf, inf]])
    win, ok = consensus.pick(risk)
    assert win.tolist() == [1, 3, 0, 0] and ok.tolist() == [True, True, False, False]
    m = consensus.margins(np.array([[4.0, 2.0, 3.0], [1.0, 1.0, 7.0]]))
    assert m.tolist() == [0.5, 0.0]


@pytest.mark.parametrize("distance", ["fd", "l2"])
def test_three_identical_tries_and_an_outlier(distance):
    from dimx import consensus
    x = _tries()
    y = np.stack([x[0], x[0], x[0], x[3]])
    D, risk, win, ok = consensus.select(y, 40, (0, None), distance)
    assert risk[0] == risk[1] == risk[2] and risk[3] > risk[0]
    assert win == 0 and ok


def test_the_library_exports_what_the_header_declares():
    import ctypes
    import os
    import re
    from dimx import lib as L
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "dimx.h")) as fh:
        declared = set(re.findall(r"\b(dimx_op_consensus_select\w*)\s*\(", fh.read()))
    assert declared == {"dimx_op_consensus_select", "dimx_op_consensus_select_ws_bytes"}
    assert declared <= set(L.SIGNATURES)
    L.load()
    so = ctypes.CDLL(L.LIB_PATH)          # a handle of its own: no attribute that load() may have set
    for name in declared:
        assert hasattr(so, name), name


def test_workspace_size_is_positive_and_monotone_in_the_tries():
    from dimx import lib as L
    ws = L.load().dimx_op_consensus_select_ws_bytes
    for kind in (0, 1):
        sizes = [int(ws(4, S, 56, kind)) for S in (1, 2, 3, 5, 10, 33)]
        assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:])), (kind, sizes)
    assert int(ws(4, 10, 56, 0)) > int(ws(4, 10, 56, 1))
    for args in ((0, 4, 56, 0), (4, 0, 56, 0), (4, 4, 0, 0), (4, 4, 65, 0), (4, 4, 56, 2), (4, 4, 56, -1), (1, 70000, 56, 1)):
        assert int(ws(*args)) == 0, args


def test_cpu_tensors_are_refused():
    from dimx import lib as L
    from dimx.engine import op_consensus_select
    from dimx.metrics import consensus_distances_hip
    x = torch.from_numpy(_tries().copy())[None]
    with pytest.raises(L.DimxError):
        op_consensus_select(x, [40])
    with pytest.raises(L.DimxError):
        consensus_distances_hip(x, [40], distance="l2")
    with pytest.raises(ValueError):
        op_consensus_select(x, [40], distance="cosine")


def test_the_protocol_rejects_unknown_selectors():
    from dimx import lib as L
    from dimx import x_engine_pt
    for kw in (dict(select="medoid"), dict(select="consensus", consensus_distance="cosine"), dict(consensus_distance="l1")):
        with pytest.raises(ValueError):
            x_engine_pt.evaluate_test_epoch(None, [], "cpu", **kw)
    with pytest.raises(L.DimxError):      # a known selector on a CPU device: GPU only, in the other selectors' error style
        x_engine_pt.evaluate_test_epoch(None, [], "cpu", beam_size=5, select="consensus")
    with pytest.raises(ValueError):       # not a batched sample count
        x_engine_pt.evaluate_test_epoch(None, [], "cuda:0", beam_size=3, select="consensus")
