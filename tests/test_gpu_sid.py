"""GPU: the SID diversity metric in the HIP library (dimx_op_kmeans_fit / dimx_op_sid_assign, csrc/kmeans_sid.hip, dimx.metrics.sid_hip
and ListenerMetrics(sid=True)) against its host definition (dimx.mymetrics.kmeans_fit_f64 / kmeans_assign_f64 / sid_entropy, which
tests/test_sid_host.py holds to scikit-learn) on the same f32 values.

Bounds.  Labels: 0 mismatches, equal iteration counts.  Centres: 1e-11 * max|X| (identical labels: a centre is a mean of the same at
most N float64 values; the project's bound for float64 sums).  SID: 1e-11 relative.  The epoch against the numbers the reference
printed (tests/golden/metrics_256.npz): rtol 1e-6, atol 1e-9, the bound the host restatement is held to.  Observed errors are printed."""
import functools
import io
import os
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEED = 20260928
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = [(6, "pose"), (6, "exp"), (24, "pose"), (24, "exp")]


def _dev():
    return torch.device("cuda:0")


def _lens():
    return [int(v) for v in np.load(os.path.join(GOLDEN, "metrics_256.npz"))["lens"]]


@functools.lru_cache(maxsize=None)
def _clip(i):
    """(gt, pred, x) of clip i, f32; computed once, never modified"""
    from dimx import prng
    n = _lens()[i]
    gt = prng.normal(SEED, "golden.m256.gt%d" % i, (n, 56)).astype(np.float64)
    pr = 0.6 * gt + 0.5 * prng.normal(SEED, "golden.m256.pr%d" % i, gt.shape)
    xs = prng.normal(SEED, "golden.m256.x%d" % i, (n, 56)).astype(np.float64)
    out = tuple(a.astype(np.float32) for a in (gt, pr, xs))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _frames(nclips):
    """the concatenated valid frames (gt, pred) [N, 56] f32 of the first nclips clips"""
    G = np.concatenate([_clip(i)[0] for i in range(nclips)])
    P = np.concatenate([_clip(i)[1] for i in range(nclips)])
    G.setflags(write=False)
    P.setflags(write=False)
    return G, P


@functools.lru_cache(maxsize=None)
def _host(nclips, type):
    """the host definition on float64 copies: (centers, n_iter, labels gt, labels pred, sid pred, sid gt)"""
    from dimx import mymetrics as mm
    k, c0, F = mm.SID_GROUPS[type]
    G, P = _frames(nclips)
    X, Y = G[:, c0:c0 + F].astype(np.float64), P[:, c0:c0 + F].astype(np.float64)
    centers, n_iter, status = mm.kmeans_fit_f64(X, k, mm.kmeans_draws(len(X), k))
    assert status == 0
    lg, lp = mm.kmeans_assign_f64(X, centers), mm.kmeans_assign_f64(Y, centers)
    return centers, n_iter, lg, lp, mm.sid_entropy(lp, k), mm.sid_entropy(lg, k)


def _device_run(G, P, type):
    """fit on G, assign P and G -> (centers, n_iter, (hist, sid, labels) of P, the same of G), all on the host"""
    from dimx import mymetrics as mm
    from dimx.engine import op_kmeans_fit, op_sid_assign
    k, c0, F = mm.SID_GROUPS[type]
    centers, n_iter = op_kmeans_fit(G, k, cols=(c0, c0 + F))
    outs = [tuple(t.cpu() for t in op_sid_assign(Z, centers, cols=(c0, c0 + F), want_labels=True)) for Z in (P, G)]
    return centers.cpu(), n_iter, outs[0], outs[1]


@functools.lru_cache(maxsize=None)
def _device(nclips, type):
    G, P = _frames(nclips)
    return _device_run(torch.from_numpy(G.copy()).to(_dev()), torch.from_numpy(P.copy()).to(_dev()), type)


# ------------------------------------------------------------------------------------------------ 1. parity with the host definition
@pytest.mark.parametrize("nclips,type", CASES)
def test_fit_and_assign_match_the_host_definition(nclips, type):
    from dimx import mymetrics as mm
    k, c0, F = mm.SID_GROUPS[type]
    h_cen, h_iter, h_lg, h_lp, h_sp, h_sg = _host(nclips, type)
    centers, n_iter, (hist_p, sid_p, lab_p), (hist_g, sid_g, lab_g) = _device(nclips, type)
    xmax = float(np.abs(_frames(nclips)[0][:, c0:c0 + F]).max())
    bad_g, bad_p = int((lab_g.numpy() != h_lg).sum()), int((lab_p.numpy() != h_lp).sum())
    cerr = float(np.abs(centers.numpy() - h_cen).max())
    e_p, e_g = abs(float(sid_p) - h_sp) / abs(h_sp), abs(float(sid_g) - h_sg) / abs(h_sg)
    print("%s, %d clips (N = %d): n_iter %d (host %d), label mismatches gt %d pred %d, centres max abs err %.3e (bound %.3e), "
          "SID rel err pred %.3e gt %.3e" % (type, nclips, len(h_lg), n_iter, h_iter, bad_g, bad_p, cerr, 1e-11 * xmax, e_p, e_g))
    assert n_iter == h_iter
    assert bad_g == 0 and bad_p == 0
    assert cerr <= 1e-11 * xmax
    assert e_p <= 1e-11 and e_g <= 1e-11
    assert np.array_equal(hist_p.numpy(), np.bincount(h_lp, minlength=k)) and np.array_equal(hist_g.numpy(), np.bincount(h_lg, minlength=k))
    assert hist_p.dtype == torch.int64 and int(hist_p.sum()) == len(h_lp)


# ------------------------------------------------------------------------------------------------ 2. views, determinism
def _same(a, b):
    ca, ia, pa, ga = a
    cb, ib, pb, gb = b
    return (ia == ib and torch.equal(ca, cb) and all(torch.equal(u, v) for u, v in zip(pa, pb))
            and all(torch.equal(u, v) for u, v in zip(ga, gb)))


def test_strided_views_inside_nan_give_the_bits_of_the_contiguous_call():
    G, P = _frames(6)
    N = len(G)
    views = []
    for Z in (G, P):
        buf = torch.full((N + 3, 64), float("nan"))
        buf[:N, 6:56] = torch.from_numpy(Z[:, 6:56].copy())       # columns 0:6 and 56:64 and the rows beyond N stay NaN
        views.append(buf.to(_dev())[:N, :56])
    assert views[0].stride(0) == 64 and not views[0].is_contiguous()
    got = _device_run(views[0], views[1], "exp")
    assert not torch.isnan(got[0]).any() and got[2][1] == got[2][1]
    assert _same(got, _device(6, "exp"))


def test_two_calls_are_bit_identical():
    G, P = _frames(24)
    for type in ("pose", "exp"):
        again = _device_run(torch.from_numpy(G.copy()).to(_dev()), torch.from_numpy(P.copy()).to(_dev()), type)
        assert _same(again, _device(24, type)), type


# ------------------------------------------------------------------------------------------------ 3. the epoch
def _parse(text):
    got = {}
    for line in text.strip().splitlines():
        k, v = line.split(":")
        got[k.strip()] = [float(t) for t in v.split()]
    return got


def test_epoch_through_the_accumulator_matches_the_numbers_the_reference_printed():
    """the 256 ragged clips as four padded batches of 64 with NaN in the padding"""
    from dimx import metrics
    g = np.load(os.path.join(GOLDEN, "metrics_256.npz"))
    lens = _lens()
    acc, plain = metrics.ListenerMetrics(sid=True), metrics.ListenerMetrics()
    for lo in range(0, 256, 64):
        ln = lens[lo:lo + 64]
        yt, yp, x = (torch.full((64, max(ln), 56), float("nan")) for _ in range(3))
        for j, n in enumerate(ln):
            yt[j, :n], yp[j, :n], x[j, :n] = (torch.from_numpy(a.copy()) for a in _clip(lo + j))
        yt, yp, x = yt.to(_dev()), yp.to(_dev()), x.to(_dev())
        acc.update(yt, yp, x, ln)
        plain.update(yt, yp, x, ln)
    buf = io.StringIO()
    with redirect_stdout(buf):
        m = acc.print()
    got = _parse(buf.getvalue())
    assert list(got) == [str(k) for k in g["labels"]]             # every line of print_metrics / print_metrics_full, in order
    exp = {str(k): [v for v in row if not np.isnan(v)] for k, row in zip(g["labels"], g["values"])}
    for t in ("sid_pose", "sid_exp"):
        err = np.max(np.abs(np.asarray(m[t]) - np.asarray(exp[t])) / np.abs(np.asarray(exp[t])))
        print("%-9s %.12g %.12g  printed %.12g %.12g  rel err %.3e" % (t, m[t][0], m[t][1], exp[t][0], exp[t][1], err))
        assert np.allclose(m[t], exp[t], rtol=1e-6, atol=1e-9), (t, m[t], exp[t])
        assert np.allclose(got[t], exp[t], rtol=1e-6, atol=1e-9)
    # bit-identical to one sid_hip call on the concatenation
    G, P = _frames(256)
    Gd, Pd = torch.from_numpy(G.copy()).to(_dev()), torch.from_numpy(P.copy()).to(_dev())
    for t in ("pose", "exp"):
        assert metrics.sid_hip(Gd, Pd, t) == tuple(m["sid_" + t]), t
    # the 16 entries of an accumulator without sid are unchanged
    base = plain.result()
    assert len(base) == 16 and set(m) == set(base) | {"sid_pose", "sid_exp"}
    for k, v in base.items():
        assert m[k] == v, k


def test_device_tensor_lens_give_the_same_frames():
    from dimx import metrics
    lens = _lens()[:4]
    yt, yp, x = (torch.full((4, max(lens), 56), float("nan")) for _ in range(3))
    for j, n in enumerate(lens):
        yt[j, :n], yp[j, :n], x[j, :n] = (torch.from_numpy(a.copy()) for a in _clip(j))
    yt, yp, x = yt.to(_dev()), yp.to(_dev()), x.to(_dev())
    a = metrics.ListenerMetrics(sid=True).update(yt, yp, x, lens)
    b = metrics.ListenerMetrics(sid=True).update(yt, yp, x, torch.tensor(lens, device=_dev()))
    assert torch.equal(a._frames[0][0], b._frames[0][0]) and torch.equal(a._frames[1][0], b._frames[1][0])
    assert a._frames[0][0].shape == (sum(lens), 56) and not torch.isnan(a._frames[0][0]).any()
    assert a.result()["sid_pose"] == b.result()["sid_pose"]


# ------------------------------------------------------------------------------------------------ 4. errors
def test_errors_are_raised_not_computed():
    from dimx import metrics, prng
    from dimx.engine import op_kmeans_fit, op_sid_assign
    from dimx.lib import DimxError
    G = torch.from_numpy(_frames(6)[0].copy())
    Gd = G.to(_dev())
    with pytest.raises(DimxError, match="frames for"):
        op_kmeans_fit(Gd[:10], 20, cols=(0, 6))                    # N < K
    with pytest.raises(DimxError, match="leave the row"):
        op_kmeans_fit(Gd, 20, cols=(52, 58))                      # a window outside the row
    cen = torch.zeros(20, 6, dtype=torch.float64, device=_dev())
    with pytest.raises(DimxError, match="leave the row"):
        op_sid_assign(Gd, cen, cols=(52, 58))
    with pytest.raises(DimxError, match="LDS plan"):
        op_kmeans_fit(Gd, 400, cols=(0, 6))                       # K * F beyond the LDS plan
    with pytest.raises(DimxError, match="GPU only"):
        op_kmeans_fit(G, 20, cols=(0, 6))
    with pytest.raises(DimxError, match="GPU only"):
        op_sid_assign(G, cen.cpu(), cols=(0, 6))
    with pytest.raises(DimxError, match="GPU only"):
        metrics.sid_hip(G, G, "pose")
    # eight distinct rows repeated to 64 frames, K = 20: at least 12 centres stay empty -- an error status, not a fault
    rows = prng.normal(3, "sid.eight", (8, 56)).astype(np.float32)
    X = torch.from_numpy(np.tile(rows, (8, 1))).to(_dev())
    with pytest.raises(DimxError, match=r"without a frame at Lloyd iteration \d+.*calcuate_sid"):
        op_kmeans_fit(X, 20, cols=(0, 6))
    with pytest.raises(DimxError, match=r"without a frame at Lloyd iteration \d+.*calcuate_sid"):
        metrics.sid_hip(X, X, "pose")
    centers, info = op_kmeans_fit(X, 20, cols=(0, 6), check=False)
    n_iter, status = info.tolist()
    assert status != 0 and status == n_iter
