"""GPU: the listener evaluation metrics in the HIP library (dimx_op_listener_metrics, csrc/listener_metrics.hip, and its accumulator
dimx.metrics.ListenerMetrics) against the host restatement of the reference (dimx.mymetrics.compute_metrics / compute_metrics_full,
dimx.metrics.clip_fd: numpy / scipy float64) on the valid frames of each clip.

Bounds.  Distances: 1e-6 relative on full-rank clips (lens >= F + 1), the bound tests/test_gpu_fd_select.py holds fd_select to; on
rank-deficient clips 10 x the error of frechet_distances_torch (CPU, float64) against clip_fd on the same clip, floor 1e-6.  Moments,
squared error, STS sums and edge rows: 1e-11 relative against numpy float64 on the same f32 values, the bound
tests/test_gpu_mesh_metrics.py uses for float64 sums.  Epoch labels against the numbers the reference itself printed
(tests/golden/metrics_256.npz): rtol 1e-6, atol 1e-9, the bound the host restatement is held to.  The observed errors are printed."""
import ctypes
import functools
import io
import os
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stub_model  # noqa: E402

pytestmark = pytest.mark.gpu

SEED, B1, L1, LENS1 = 21, 7, 130, [130, 113, 120, 101, 100, 60, 20]
GROUPS = ((0, 6), (6, 56))


def _dev():
    return torch.device("cuda:0")


def _windows():
    from dimx.engine import LISTENER_WINDOWS
    return LISTENER_WINDOWS


@functools.lru_cache(maxsize=None)
def _inputs():
    g = torch.Generator().manual_seed(SEED)
    yt = torch.randn(B1, L1, 56, generator=g)
    yp = 0.6 * yt + 0.5 * torch.randn(B1, L1, 56, generator=g)
    x = torch.randn(B1, L1, 56, generator=g)
    return yt, yp, x, list(LENS1)


def _operands(yt, yp, x, n, win):
    xc0, xF, yc0, yF = win
    return (torch.cat([x[:n, xc0:xc0 + xF], yt[:n, yc0:yc0 + yF]], -1), torch.cat([x[:n, xc0:xc0 + xF], yp[:n, yc0:yc0 + yF]], -1))


@functools.lru_cache(maxsize=None)
def _reference_fd():
    """clip_fd per (clip, window) on the concatenated columns, and the torch path's error against it on the rank-deficient clips;
    computed once, never modified"""
    from dimx import metrics
    yt, yp, x, lens = _inputs()
    ref = np.empty((B1, len(_windows())))
    terr = np.zeros_like(ref)
    for b, n in enumerate(lens):
        for w, (_, win) in enumerate(_windows()):
            a, c = _operands(yt[b], yp[b], x[b], n, win)
            ref[b, w] = metrics.clip_fd(a.numpy(), c.numpy())
            if n < a.shape[1] + 1:
                t = float(metrics.frechet_distances_torch(a[None], c[None, None], [n])[0, 0])
                terr[b, w] = abs(t - ref[b, w]) / abs(ref[b, w])
    ref.setflags(write=False)
    terr.setflags(write=False)
    return ref, terr


def _moments_numpy(yt, yp, x, n):
    """one row of the operator's second output in numpy float64 (include/dimx.h)"""
    g, p, xs = (t[:n, :56].double().numpy() for t in (yt, yp, x))
    row = np.zeros(133)
    row[0] = n
    for gi, (c0, c1) in enumerate(GROUPS):
        o = 1 + 10 * gi
        G, P, X = g[:, c0:c1], p[:, c0:c1], xs[:, c0:c1]
        row[o] = np.sum((G - P) ** 2)
        for k, v in ((1, G), (3, P), (5, X)):
            row[o + k] = np.mean(v)
            row[o + k + 1] = np.sum((v - np.mean(v)) ** 2)
        row[o + 7] = np.sum((G - np.mean(G)) * (X - np.mean(X)))
        row[o + 8] = np.sum((P - np.mean(P)) * (X - np.mean(X)))
        row[o + 9] = np.sum((np.diff(G, axis=0) - np.diff(P, axis=0)) ** 2)
    row[21:77] = g[0] - p[0]
    row[77:133] = g[-1] - p[-1]
    return row


def _run(yt, yp, x, lens):
    from dimx.engine import op_listener_metrics
    fd, mom = op_listener_metrics(yt, yp, x, lens)
    return fd.cpu(), mom.cpu()


@functools.lru_cache(maxsize=None)
def _clean():
    from dimx.engine import listener_metrics_sweeps
    yt, yp, x, lens = _inputs()
    out = _run(yt.to(_dev()), yp.to(_dev()), x.to(_dev()), lens)
    sw = listener_metrics_sweeps(_dev(), B1, len(_windows()), 112)
    return out + (sw[0].cpu(), sw[1].cpu())


# ------------------------------------------------------------------------------------------------ 1. per-clip parity
def test_distances_match_the_reference_arithmetic_per_clip_and_window():
    ref, terr = _reference_fd()
    fd = _clean()[0].numpy()
    failures = []
    for w, (name, win) in enumerate(_windows()):
        F = win[1] + win[3]
        for b, n in enumerate(LENS1):
            err = abs(fd[b, w] - ref[b, w]) / abs(ref[b, w])
            if n >= F + 1:
                bound = 1e-6
                print("%-9s F=%3d clip %d (n=%3d, full rank): kernel rel err %.3e" % (name, F, b, n, err))
            else:
                bound = max(10.0 * terr[b, w], 1e-6)
                print("%-9s F=%3d clip %d (n=%3d, rank-deficient): kernel rel err %.3e, torch path %.3e, bound %.3e"
                      % (name, F, b, n, err, terr[b, w], bound))
            if not err <= bound:
                failures.append((name, b, err, bound))
    assert not failures, failures


def test_moments_squared_error_sts_and_edges_match_numpy_float64():
    yt, yp, x, lens = _inputs()
    mom = _clean()[1].numpy()
    assert mom.shape == (B1, 133)
    worst = 0.0
    for b, n in enumerate(lens):
        ref = _moments_numpy(yt[b], yp[b], x[b], n)
        err = np.abs(mom[b] - ref) / np.where(ref != 0, np.abs(ref), 1.0)
        print("clip %d (n=%3d): moments max rel err %.3e (entry %d)" % (b, n, err.max(), int(err.argmax())))
        worst = max(worst, float(err.max()))
        assert (err <= 1e-11).all(), (b, int(err.argmax()), float(err.max()))
    print("worst %.3e" % worst)


def test_sweep_counts_stay_below_the_bound():
    _, _, sw_t, sw_c = _clean()
    print("sweeps: target %d..%d, candidate %d..%d" % (int(sw_t.min()), int(sw_t.max()), int(sw_c.min()), int(sw_c.max())))
    assert tuple(sw_t.shape) == (len(_windows()), B1) and tuple(sw_c.shape) == (len(_windows()), B1)
    assert int(sw_t.min()) >= 1 and int(sw_c.min()) >= 1
    assert int(sw_t.max()) < 30 and int(sw_c.max()) < 30


# the boundaries of the shared templates (csrc/frechet.hpp), every clip full rank (lens >= 113): F = 64 the last of the eight-row
# Jacobi; 65 the first of the fourteen-row one, odd; 57 odd; 1 no pair at all; 112 the operator's maximum
SEED2, B2, L2, LENS2 = 22, 2, 130, [130, 114]
EDGE_WINDOWS = ((0, 8, 0, 56), (0, 9, 0, 56), (0, 1, 0, 56), (0, 0, 0, 1), (0, 56, 0, 56))


def test_template_boundaries_match_the_reference_arithmetic():
    from dimx import metrics
    from dimx.engine import listener_metrics_sweeps, op_listener_metrics
    g = torch.Generator().manual_seed(SEED2)
    yt = torch.randn(B2, L2, 56, generator=g)
    yp = 0.6 * yt + 0.5 * torch.randn(B2, L2, 56, generator=g)
    x = torch.randn(B2, L2, 56, generator=g)
    fd = op_listener_metrics(yt.to(_dev()), yp.to(_dev()), x.to(_dev()), LENS2, windows=EDGE_WINDOWS)[0].cpu().numpy()
    sw_t, sw_c = (t.cpu() for t in listener_metrics_sweeps(_dev(), B2, len(EDGE_WINDOWS), 112))
    failures = []
    for w, win in enumerate(EDGE_WINDOWS):
        F = win[1] + win[3]
        for b, n in enumerate(LENS2):
            assert n >= F + 1                                  # full rank: the 1e-6 bound applies
            ref = metrics.clip_fd(*(t.numpy() for t in _operands(yt[b], yp[b], x[b], n, win)))
            assert np.isfinite(ref) and ref > 0                # the bound is not met vacuously
            err = abs(fd[b, w] - ref) / abs(ref)
            print("window %s F=%3d clip %d (n=%3d): kernel rel err %.3e, sweeps %d / %d" % (win, F, b, n, err, int(sw_t[w, b]),
                                                                                            int(sw_c[w, b])))
            if not err <= 1e-6:
                failures.append((win, b, err))
    assert not failures, failures
    assert int(sw_t.min()) >= 1 and int(sw_c.min()) >= 1
    assert int(sw_t.max()) < 30 and int(sw_c.max()) < 30


# ------------------------------------------------------------------------------------------------ 2. epoch parity
def _parse(text):
    got = {}
    for line in text.strip().splitlines():
        k, v = line.split(":")
        got[k.strip()] = [float(t) for t in v.split()]
    return got


def test_epoch_matches_the_numbers_the_reference_printed(golden_dir):
    """the 256 ragged clips of tests/test_host_io.py rounded to f32, as four padded batches of 64: the Chan merge and the STS step
    across clips and across batch boundaries"""
    from dimx import metrics, prng
    g = np.load(os.path.join(golden_dir, "metrics_256.npz"))
    lens = [int(v) for v in g["lens"]]
    seed = 20260928
    acc = metrics.ListenerMetrics()
    for lo in range(0, 256, 64):
        ln = lens[lo:lo + 64]
        Lm = max(ln)
        yt, yp, x = (torch.zeros(64, Lm, 56) for _ in range(3))
        for j, n in enumerate(ln):
            i = lo + j
            gt = prng.normal(seed, "golden.m256.gt%d" % i, (n, 56)).astype(np.float64)
            pr = 0.6 * gt + 0.5 * prng.normal(seed, "golden.m256.pr%d" % i, gt.shape)
            xs = prng.normal(seed, "golden.m256.x%d" % i, (n, 56)).astype(np.float64)
            yt[j, :n], yp[j, :n], x[j, :n] = (torch.from_numpy(a.astype(np.float32)) for a in (gt, pr, xs))
        acc.update(yt.to(_dev()), yp.to(_dev()), x.to(_dev()), ln)
    buf = io.StringIO()
    with redirect_stdout(buf):
        acc.print()
    got = _parse(buf.getvalue())
    labels = [str(k) for k in g["labels"] if not str(k).startswith("sid")]
    assert list(got) == labels                                 # the same labels in the same order, SID left out
    exp = {str(k): [v for v in row if not np.isnan(v)] for k, row in zip(g["labels"], g["values"])}
    bad = []
    for k in labels:
        err = np.max(np.abs(np.asarray(got[k]) - np.asarray(exp[k])) / np.abs(np.asarray(exp[k])))
        print("%-10s rel err %.3e" % (k, err))
        if not np.allclose(got[k], exp[k], rtol=1e-6, atol=1e-9):
            bad.append((k, got[k], exp[k]))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ 3. accumulator invariance
def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.abs(b)))


def test_one_batch_of_eight_equals_two_batches_of_four():
    from dimx import metrics
    g = torch.Generator().manual_seed(5)
    lens = [70, 64, 58, 61, 66, 59, 70, 63]
    yt = torch.randn(8, 70, 56, generator=g)
    yp = 0.6 * yt + 0.5 * torch.randn(8, 70, 56, generator=g)
    x = torch.randn(8, 70, 56, generator=g)
    yt, yp, x = yt.to(_dev()), yp.to(_dev()), x.to(_dev())
    one = metrics.ListenerMetrics().update(yt, yp, x, lens).result()
    acc = metrics.ListenerMetrics()
    acc.update(yt[:4], yp[:4], x[:4], lens[:4]).update(yt[4:], yp[4:], x[4:], lens[4:])
    two = acc.result()
    assert set(one) == set(two)
    for k in one:
        print("%-10s %.3e" % (k, _rel(two[k], one[k])))
        assert _rel(two[k], one[k]) <= 1e-12, (k, one[k], two[k])


def test_sts_runs_over_the_concatenation_of_the_clips():
    from dimx import metrics
    g = torch.Generator().manual_seed(6)
    lens = [40, 33]
    yt = torch.randn(2, 40, 56, generator=g)
    yp = 0.6 * yt + 0.5 * torch.randn(2, 40, 56, generator=g)
    yt[1] += 25.0                                              # the step from clip 0 to clip 1 dominates the sum
    x = torch.randn(2, 40, 56, generator=g)
    r = metrics.ListenerMetrics().update(yt.to(_dev()), yp.to(_dev()), x.to(_dev()), lens).result()
    split = metrics.ListenerMetrics()
    for j in range(2):                                         # the same two clips as two updates: the carry across batches
        split.update(yt[j:j + 1].to(_dev()), yp[j:j + 1].to(_dev()), x[j:j + 1].to(_dev()), lens[j:j + 1])
    rs = split.result()
    cg = np.concatenate([yt[j, :n].double().numpy() for j, n in enumerate(lens)])
    cp = np.concatenate([yp[j, :n].double().numpy() for j, n in enumerate(lens)])
    for name, (c0, c1) in zip(("sts_pose", "sts_exp"), GROUPS):
        whole = metrics.sts(cg[:, c0:c1], cp[:, c0:c1])
        parts = np.sqrt(sum(metrics.sts(yt[j, :n, c0:c1].double().numpy(), yp[j, :n, c0:c1].double().numpy()) ** 2
                            for j, n in enumerate(lens)))
        print("%s: accumulator %.12g, concatenation %.12g, per-clip sum %.12g" % (name, r[name], whole, parts))
        assert abs(whole - parts) / whole > 0.1               # the case tells the two apart
        assert _rel(r[name], whole) <= 1e-11 and _rel(rs[name], whole) <= 1e-11


def test_accumulator_refuses_to_average_the_nan_of_a_clip_without_a_covariance():
    from dimx import metrics
    yt, yp, x, _ = _inputs()
    acc = metrics.ListenerMetrics().update(yt[:2].to(_dev()), yp[:2].to(_dev()), x[:2].to(_dev()), [50, 1])
    with pytest.raises(ValueError):
        acc.result()


# ------------------------------------------------------------------------------------------------ 4. memory discipline
def test_padding_is_never_read():
    yt, yp, x, lens = (t.clone() if torch.is_tensor(t) else t for t in _inputs())
    for j, n in enumerate(lens):
        yt[j, n:] = float("nan")
        yp[j, n:] = float("nan")
        x[j, n:] = float("nan")
    fd, mom = _run(yt.to(_dev()), yp.to(_dev()), x.to(_dev()), lens)
    assert torch.equal(fd, _clean()[0]) and torch.equal(mom, _clean()[1])


def test_strided_views_give_the_contiguous_result():
    yt, yp, x, lens = _inputs()
    big = torch.full((B1, L1 + 1, 56), float("nan"))          # tgt[:, 1:]
    big[:, 1:] = yt
    wide = torch.full((B1, L1, 61), float("nan"))              # a wider row
    wide[:, :, :56] = yp
    long = torch.full((B1, L1 + 5, 56), float("nan"))          # a longer frame axis
    long[:, :L1] = x
    a, b, c = big.to(_dev())[:, 1:], wide.to(_dev())[:, :, :56], long.to(_dev())
    assert not a.is_contiguous() and not b.is_contiguous()
    fd, mom = _run(a, b, c, lens)
    assert torch.equal(fd, _clean()[0]) and torch.equal(mom, _clean()[1])


def test_two_calls_are_bit_identical():
    yt, yp, x, lens = _inputs()
    fd, mom = _run(yt.to(_dev()), yp.to(_dev()), x.to(_dev()), lens)
    assert torch.equal(fd, _clean()[0]) and torch.equal(mom, _clean()[1])


def test_a_clip_without_two_frames_gives_nan_and_leaves_the_others_alone():
    yt, yp, x, lens = _inputs()
    lens = list(lens)
    lens[1], lens[4] = 1, 0
    fd, mom = _run(yt.to(_dev()), yp.to(_dev()), x.to(_dev()), lens)
    assert torch.isnan(fd[1]).all() and torch.isnan(fd[4]).all()
    assert float(mom[1, 0]) == 1.0 and not mom[4].any()
    assert torch.equal(mom[1, 21:77], mom[1, 77:133])
    for j in (0, 2, 3, 5, 6):
        assert torch.equal(fd[j], _clean()[0][j]) and torch.equal(mom[j], _clean()[1][j])


# ------------------------------------------------------------------------------------------------ 5. raw ctypes
def test_argument_checks_return_an_error_and_enqueue_nothing():
    from dimx import lib as L
    lib = L.load()
    yt, yp, x, lens = _inputs()
    wide = torch.zeros(B1, L1, 60)
    wide[:, :, :56] = x
    d_t, d_p, d_x = yt.to(_dev()), yp.to(_dev()), wide.to(_dev())
    d_l = torch.tensor(lens, dtype=torch.int32, device=_dev())
    wins = [w for _, w in _windows()]
    need = int(lib.dimx_op_listener_metrics_ws_bytes(B1, 6, 112))
    assert need > 0
    ws = torch.zeros(need + 8, dtype=torch.uint8, device=_dev())
    fd = torch.full((B1, 6), -7.0, dtype=torch.float64, device=_dev())
    mom = torch.full((B1, 133), -7.0, dtype=torch.float64, device=_dev())

    def call(windows, ws_off=0, ws_bytes=need):
        flat = [v for w in windows for v in w]
        arr = (ctypes.c_int32 * len(flat))(*flat)
        return lib.dimx_op_listener_metrics(L.ptr(d_t), d_t.stride(0), d_t.stride(1), L.ptr(d_p), d_p.stride(0), d_p.stride(1),
                                            L.ptr(d_x), d_x.stride(0), d_x.stride(1), L.ptr(d_l), B1, L1, 56, 60, arr, len(windows),
                                            L.ptr(fd), L.ptr(mom), ctypes.c_void_p(ws.data_ptr() + ws_off), ws_bytes,
                                            L.stream_ptr(_dev()))

    assert call(wins[:5] + [(0, 57, 0, 56)]) != 0              # F = 113
    assert call(wins[:5] + [(0, 0, 10, 50)]) != 0              # columns [10, 60) leave the row of 56
    assert call(wins[:5] + [(5, 56, 0, 56)]) != 0              # columns [5, 61) leave x's row of 60
    assert call(wins, ws_bytes=need - 1) != 0                  # one byte short
    assert call(wins, ws_off=4) != 0                           # misaligned
    torch.cuda.synchronize()
    assert (fd == -7.0).all() and (mom == -7.0).all() and not ws.any()
    assert call(wins) == 0                                     # the same buffers with valid arguments: the call itself works
    torch.cuda.synchronize()
    assert torch.equal(fd.cpu(), _clean()[0]) and torch.equal(mom.cpu(), _clean()[1])


# ------------------------------------------------------------------------------------------------ 6. protocol
class _DeviceStub(stub_model.StubSLMFT):
    """the CPU stub behind device tensors: its arithmetic stays on the host, the samples go to the GPU"""

    def forward(self, v_speaker, v_listener, v_audio, mask, mode="train", n_samples=1, **kw):
        dev = v_listener.device
        a, b, pred = super().forward(v_speaker.cpu(), v_listener.cpu(), v_audio.cpu(), mask.cpu(), mode=mode, n_samples=n_samples, **kw)
        return a, b, pred.to(dev)


def test_protocol_accumulates_what_the_host_metrics_give_for_the_returned_lists():
    """The operator sees f32 tensors (the stub's float64 batches are rounded where fd_select rounds them), so the host reference runs
    on the returned lists rounded to f32 and widened to float64: the same values."""
    from dimx import metrics, mymetrics, x_engine_pt
    acc = metrics.ListenerMetrics()
    with_m = x_engine_pt.evaluate_test_epoch(_DeviceStub(), stub_model.protocol_batches(), _dev(), beam_size=10, fd_backend="hip",
                                             metrics=acc)
    plain = x_engine_pt.evaluate_test_epoch(_DeviceStub(), stub_model.protocol_batches(), _dev(), beam_size=10, fd_backend="hip")
    for a, b in zip(with_m[:3], plain[:3]):
        assert len(a) == len(b) and all(np.array_equal(u, v) for u, v in zip(a, b))
    assert list(with_m[3]) == list(plain[3])
    got = acc.result()
    gl, pl, xl = ([np.asarray(a, dtype=np.float32).astype(np.float64) for a in lst] for lst in with_m[:3])
    ref = mymetrics.compute_metrics(gl, pl, xl, with_sid=False)
    ref.update(mymetrics.compute_metrics_full(gl, pl, xl))
    assert set(got) == set(ref)
    names = dict(_windows())
    for k in ref:
        assert type(got[k]) is type(ref[k]), k
        err = _rel(got[k], ref[k])
        if k in names:                                          # a mean of distances: the bounds of the per-clip case
            F = names[k][1] + names[k][3]
            bound = 1e-6
            if any(a.shape[0] < F + 1 for a in gl):
                t = np.mean([float(metrics.frechet_distances_torch(*_fd_pair(g_, p_, x_, names[k]), [g_.shape[0]])[0, 0])
                             for g_, p_, x_ in zip(gl, pl, xl)])
                bound = max(10.0 * abs(t - ref[k]) / abs(ref[k]), 1e-6)
        else:
            bound = 1e-11
        print("%-10s rel err %.3e (bound %.1e)" % (k, err, bound))
        assert err <= bound, (k, got[k], ref[k])


def _fd_pair(g, p, x, win):
    a, c = _operands(torch.from_numpy(g), torch.from_numpy(p), torch.from_numpy(x), g.shape[0], win)
    return a[None], c[None, None]
