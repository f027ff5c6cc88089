"""CPU: the host restatement of the SID metric's KMeans (dimx.mymetrics.kmeans_draws / kmeans_fit_f64 / sid_f64, the definition of
dimx_op_kmeans_fit and dimx_op_sid_assign) against scikit-learn on float64 copies of the same values and against the numbers the
reference printed (tests/golden/metrics_256.npz).  Inputs: the golden.m256.* generator of tests/test_host_io.py, rounded to f32 and
widened to f64 -- the values the operator sees.

Bounds.  Labels: 0 mismatches and equal iteration counts (scikit-learn alone meets that on these inputs).  Centres: 1e-11 * max|X|
-- with identical labels a centre is a mean of the same at most N values, the project's bound for float64 sums.  SID: 1e-11 relative.
The printed values: rtol 1e-6, atol 1e-9, the bound tests/test_host_io.py holds the restatement to."""
import functools
import os

import numpy as np
import pytest
import torch

import dimx  # noqa: F401
from dimx import lib, mymetrics, prng

SEED = 20260928
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def _clips(nclips):
    """per-clip lists (gt, pred) of [n, 56] float64 arrays holding f32 values; computed once, never modified"""
    lens = [int(v) for v in np.load(os.path.join(GOLDEN, "metrics_256.npz"))["lens"]][:nclips]
    gts = [prng.normal(SEED, "golden.m256.gt%d" % i, (n, 56)).astype(np.float64) for i, n in enumerate(lens)]
    prs = [0.6 * a + 0.5 * prng.normal(SEED, "golden.m256.pr%d" % i, a.shape) for i, a in enumerate(gts)]
    rnd = lambda l: [a.astype(np.float32).astype(np.float64) for a in l]
    gts, prs = rnd(gts), rnd(prs)
    for a in gts + prs:
        a.setflags(write=False)
    return gts, prs


@pytest.mark.parametrize("type", ["pose", "exp"])
@pytest.mark.parametrize("nclips,n_frames", [(6, 846), (24, 3615)])
def test_fit_and_assign_match_scikit_learn_on_float64(nclips, n_frames, type):
    pytest.importorskip("sklearn")
    from sklearn.cluster import KMeans, kmeans_plusplus
    gts, prs = _clips(nclips)
    k, c0, F = mymetrics.SID_GROUPS[type]
    X = np.ascontiguousarray(np.concatenate(gts)[:, c0:c0 + F])
    Y = np.ascontiguousarray(np.concatenate(prs)[:, c0:c0 + F])
    assert X.shape == (n_frames, F) and X.dtype == np.float64
    draws = mymetrics.kmeans_draws(n_frames, k)
    assert draws[0] == int(kmeans_plusplus(X, n_clusters=k, random_state=0)[1][0])     # scikit-learn's first centre
    centers, n_iter, status = mymetrics.kmeans_fit_f64(X, k, draws)
    km = KMeans(n_clusters=k, random_state=0, n_init="auto").fit(X)
    assert status == 0 and n_iter == km.n_iter_, (n_iter, km.n_iter_)
    for name, Z in (("gt", X), ("pred", Y)):
        bad = int((mymetrics.kmeans_assign_f64(Z, centers) != km.predict(Z)).sum())
        print("%s %d clips, %s: %d label mismatches of %d" % (type, nclips, name, bad, len(Z)))
        assert bad == 0
    cerr = float(np.abs(centers - km.cluster_centers_).max())
    print("%s %d clips: n_iter %d, centres max abs err %.3e (bound %.3e)" % (type, nclips, n_iter, cerr, 1e-11 * np.abs(X).max()))
    assert cerr <= 1e-11 * np.abs(X).max()
    got = mymetrics.sid_f64(gts, prs, type)
    want = (mymetrics.calcuate_sid(gts, prs, type), mymetrics.calcuate_sid(gts, gts, type))
    for g, w in zip(got, want):
        assert abs(g - w) <= 1e-11 * abs(w), (got, want)


def test_all_256_clips_give_the_sid_values_the_reference_printed():
    g = np.load(os.path.join(GOLDEN, "metrics_256.npz"))
    exp = {str(k): [v for v in row if not np.isnan(v)] for k, row in zip(g["labels"], g["values"])}
    gts, prs = _clips(256)
    G, P = np.concatenate(gts), np.concatenate(prs)
    for t in ("pose", "exp"):
        got = mymetrics.sid_f64(G, P, t)
        print("sid_%s: " % t, *got, " printed:", *exp["sid_" + t])
        assert np.allclose(got, exp["sid_" + t], rtol=1e-6, atol=1e-9), (t, got, exp["sid_" + t])


@pytest.mark.parametrize("k,trials", [(20, 4), (40, 5)])
def test_kmeans_draws_are_scikit_learns_in_its_order(k, trials):
    n = 846
    first, U = mymetrics.kmeans_draws(n, k)
    assert U.shape == (k - 1, trials) and U.dtype == np.float64
    rs = np.random.RandomState(0)
    w = np.ones(n, dtype=np.float64)
    assert first == rs.choice(n, p=w / w.sum())                     # _kmeans_plusplus: the first centre
    for c in range(k - 1):
        assert np.array_equal(U[c], rs.uniform(size=2 + int(np.log(k))))   # one draw of n_local_trials per further centre
    assert mymetrics.kmeans_draws(n, k) [0] == first and np.array_equal(mymetrics.kmeans_draws(n, k)[1], U)


def test_an_empty_cluster_is_reported_not_papered_over():
    rows = prng.normal(3, "sid.eight", (8, 6)).astype(np.float32).astype(np.float64)
    X = np.tile(rows, (8, 1))                                       # 64 frames, 8 distinct: at least 12 of 20 centres stay empty
    centers, n_iter, status = mymetrics.kmeans_fit_f64(X, 20, mymetrics.kmeans_draws(64, 20))
    assert status != 0 and status == n_iter
    with pytest.raises(ValueError, match="empty"):
        mymetrics.sid_f64(np.tile(X, (1, 10))[:, :56], np.tile(X, (1, 10))[:, :56], "pose")
    with pytest.raises(ValueError):
        mymetrics.kmeans_fit_f64(X[:10], 20, mymetrics.kmeans_draws(64, 20))


def test_the_operators_are_exported_size_their_workspace_and_have_no_cpu_fallback():
    l = lib.load()
    for name in ("dimx_op_kmeans_fit", "dimx_op_kmeans_fit_ws_bytes", "dimx_op_sid_assign"):
        assert hasattr(l, name) and name in lib.SIGNATURES
    need = int(l.dimx_op_kmeans_fit_ws_bytes(40855, 40, 50))
    assert need >= 40855 * 50 * 8 + 3 * 40855 * 8                   # the centred copy, closest, scan, labels
    assert l.dimx_op_kmeans_fit_ws_bytes(0, 40, 50) == 0
    assert l.dimx_op_kmeans_fit_ws_bytes(100, 0, 50) == 0
    assert l.dimx_op_kmeans_fit_ws_bytes(100, 40, 65) == 0          # F beyond the LDS plan
    assert l.dimx_op_kmeans_fit_ws_bytes(100, 41, 50) == 0          # K * F beyond the LDS plan
    from dimx import engine, metrics
    y = torch.zeros(64, 56)
    with pytest.raises(lib.DimxError):
        engine.op_kmeans_fit(y, 20, cols=(0, 6))
    with pytest.raises(lib.DimxError):
        engine.op_sid_assign(y, torch.zeros(20, 6, dtype=torch.float64), cols=(0, 6))
    with pytest.raises(lib.DimxError):
        metrics.sid_hip(y, y, "pose")
    assert metrics.ListenerMetrics().sid is False and metrics.ListenerMetrics(sid=True).sid is True
