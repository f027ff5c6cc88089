"""GPU: best-of-S selection by Frechet distance in the HIP library (dimx_op_fd_select, csrc/fd_select.hip) against the reference's
numpy / scipy float64 arithmetic (dimx.metrics.clip_fd, pinned by tests/golden/host_protocol.npz) on the valid frames of each clip.

Bounds: 1e-6 relative on full-rank clips (lens >= F + 1), the bound tests/test_host_protocol_golden.py holds the torch path to.  On
rank-deficient clips (case C) 10 x the error of frechet_distances_torch (CPU, float64) against clip_fd on the same clip, floor 1e-6:
eigenvalues that are exactly zero come out of different solvers as different residues, and the square root amplifies them.  Both
errors are printed."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stub_model  # noqa: E402

pytestmark = pytest.mark.gpu

#        seed  B  S   L    lens                    windows
CASES = {
    "A": (3, 5, 4, 90, [90, 77, 64, 90, 58], [(0, 56)]),
    "B": (11, 4, 3, 70, [70, 57, 64, 61], [(0, 56), (0, 6), (6, 50)]),
    "C": (12, 3, 10, 40, [40, 20, 2], [(0, 56)]),
    "D": (13, 2, 10, 330, [330, 299], [(0, 56)]),
    # the boundaries of the shared templates (csrc/frechet.hpp), rows of 64 columns, every clip full rank: F = 64 the operator's
    # maximum (every pair lane live, full register tile); 7 odd (the bye pair) in the one-row-per-lane Jacobi, c0 > 0; 8 the last F
    # of that Jacobi; 9 the first of the eight-row one, odd; 1 no pair at all
    "E": (14, 2, 2, 80, [80, 66], [(0, 64), (3, 10), (0, 8), (0, 9), (5, 6)]),
}
WIDTH = {"E": 64}
CASE_WINDOWS = [(k, w) for k, v in CASES.items() if k != "E" for w in v[5]]
EDGE_WINDOWS = CASES["E"][5]


@functools.lru_cache(maxsize=None)
def _inputs(name):
    seed, B, S, L, lens, _ = CASES[name]
    g = torch.Generator().manual_seed(seed)
    W = WIDTH.get(name, 56)
    yt = torch.randn(B, L, W, generator=g)
    yp = 0.6 * yt[:, None] + 0.5 * torch.randn(B, S, L, W, generator=g)
    return yt, yp, list(lens)


@functools.lru_cache(maxsize=None)
def _reference(name, window):
    """clip_fd per (clip, try) on the valid frames and the window's columns; computed once per case, never modified"""
    from dimx import metrics
    yt, yp, lens = _inputs(name)
    c0, c1 = window
    ref = np.empty((yp.shape[0], yp.shape[1]))
    for j in range(yp.shape[0]):
        for s in range(yp.shape[1]):
            ref[j, s] = metrics.clip_fd(yt[j, :lens[j], c0:c1].numpy(), yp[j, s, :lens[j], c0:c1].numpy())
    ref.setflags(write=False)
    return ref


def _dev():
    return torch.device("cuda:0")


def _run(yt, yp, lens, window=(0, 56)):
    from dimx.engine import op_fd_select
    fd, win, ok, best = op_fd_select(yt, yp, lens, cols=window)
    return fd.cpu(), win.cpu(), ok.cpu(), best.cpu()


@functools.lru_cache(maxsize=None)
def _clean_b():
    yt, yp, lens = _inputs("B")
    return _run(yt.to(_dev()), yp.to(_dev()), lens)


def _check_distances_winner_and_gather(name, window):
    from dimx import metrics
    yt, yp, lens = _inputs(name)
    ref = _reference(name, window)
    fd, win, ok, best = _run(yt.to(_dev()), yp.to(_dev()), lens, window)
    c0, c1 = window
    F = c1 - c0
    B, S = ref.shape
    fd = fd.numpy()
    failures = []
    for j in range(B):
        err = np.abs(fd[j] - ref[j]) / np.abs(ref[j])
        if lens[j] >= F + 1:
            bound = 1e-6
            print("case %s window %s clip %d (n=%d, full rank): kernel max rel err %.3e" % (name, window, j, lens[j], err.max()))
        else:
            t = metrics.frechet_distances_torch(yt[j:j + 1, :, c0:c1], yp[j:j + 1, :, :, c0:c1], [lens[j]])[0].numpy()
            terr = float((np.abs(t - ref[j]) / np.abs(ref[j])).max())
            bound = max(10.0 * terr, 1e-6)
            print("case %s window %s clip %d (n=%d, rank-deficient): kernel max rel err %.3e, torch path %.3e, bound %.3e" % (
                name, window, j, lens[j], err.max(), terr, bound))
        if not (err <= bound).all():
            failures.append((j, err.max(), bound))
    assert not failures, failures
    assert win.tolist() == ref.argmin(1).tolist()
    assert ok.tolist() == [1] * B
    for j in range(B):
        assert torch.equal(best[j, :lens[j]], yp[j, int(win[j]), :lens[j]])      # the full row, also for the sliced windows
        assert not best[j, lens[j]:].any()


@pytest.mark.parametrize("name,window", CASE_WINDOWS, ids=["%s-%d-%d" % (k, w[0], w[1]) for k, w in CASE_WINDOWS])
def test_distances_winner_and_gather_match_the_reference_arithmetic(name, window):
    _check_distances_winner_and_gather(name, window)


@pytest.mark.parametrize("window", EDGE_WINDOWS, ids=["E-%d-%d" % w for w in EDGE_WINDOWS])
def test_template_boundaries_match_the_reference_arithmetic(window):
    from dimx.engine import fd_select_sweeps
    _, B, S, _, lens, _ = CASES["E"]
    F = window[1] - window[0]
    assert min(lens) >= F + 1                                  # full rank: the 1e-6 bound applies to every clip
    ref = _reference("E", window)
    assert np.isfinite(ref).all() and (ref > 0).all()          # the bound is not met vacuously
    _check_distances_winner_and_gather("E", window)
    sw_t, sw_c = (t.cpu() for t in fd_select_sweeps(_dev(), B, S, F))
    print("window %s F=%d sweeps: target %d..%d, candidate %d..%d" % (window, F, int(sw_t.min()), int(sw_t.max()), int(sw_c.min()),
                                                                     int(sw_c.max())))
    assert tuple(sw_t.shape) == (B,) and tuple(sw_c.shape) == (B, S)
    assert int(sw_t.min()) >= 1 and int(sw_c.min()) >= 1
    assert int(sw_t.max()) < 30 and int(sw_c.max()) < 30


def test_padding_is_never_read():
    yt, yp, lens = _inputs("B")
    yt, yp = yt.clone(), yp.clone()
    for j, n in enumerate(lens):
        yt[j, n:] = float("nan")
        yp[j, :, n:] = float("nan")
    fd, win, ok, best = _run(yt.to(_dev()), yp.to(_dev()), lens)
    cfd, cwin, cok, cbest = _clean_b()
    assert torch.equal(fd, cfd) and torch.equal(win, cwin) and torch.equal(best, cbest) and torch.equal(ok, cok)


def test_strided_views_give_the_contiguous_result():
    yt, yp, lens = _inputs("B")
    B, S, L, W = yp.shape
    big = torch.full((B, L + 1, W), float("nan"))
    big[:, 1:] = yt
    wide = torch.full((B, S, L + 5, W), float("nan"))
    wide[:, :, :L] = yp
    y_true = big.to(_dev())[:, 1:]
    y_pred = wide.to(_dev())[:, :, :L]
    assert not y_true.is_contiguous() and not y_pred.is_contiguous()
    fd, win, ok, best = _run(y_true, y_pred, lens)
    cfd, cwin, cok, cbest = _clean_b()
    assert torch.equal(fd, cfd) and torch.equal(win, cwin) and torch.equal(best, cbest) and torch.equal(ok, cok)


def test_ties_and_reproducibility():
    yt, yp, lens = _inputs("B")
    yp = yp.clone()
    yp[:, 2] = yp[:, 0]
    d_t, d_p = yt.to(_dev()), yp.to(_dev())
    fd, win, ok, best = _run(d_t, d_p, lens)
    assert torch.equal(fd[:, 2], fd[:, 0])
    for j in range(fd.shape[0]):
        if float(fd[j, 0]) == float(fd[j].min()):
            assert int(win[j]) == 0
    fd2 = _run(d_t, d_p, lens)[0]
    assert torch.equal(fd, fd2)


def test_degenerate_clip_is_flagged_and_leaves_the_others_alone():
    yt, yp, lens = _inputs("B")
    lens = [70, 1, 64, 61]
    fd, win, ok, best = _run(yt.to(_dev()), yp.to(_dev()), lens)
    cfd, cwin, cok, cbest = _clean_b()
    assert ok.tolist() == [1, 0, 1, 1]
    assert not torch.isfinite(fd[1]).any()
    assert not best[1].any()
    for j in (0, 2, 3):
        assert torch.equal(fd[j], cfd[j]) and int(win[j]) == int(cwin[j]) and torch.equal(best[j], cbest[j])


class _DeviceStub(stub_model.StubSLMFT):
    """the CPU stub behind device tensors: its arithmetic stays on the host (bit for bit the fixture's), the samples go to the GPU"""

    def forward(self, v_speaker, v_listener, v_audio, mask, mode="train", n_samples=1, **kw):
        dev = v_listener.device
        a, b, pred = super().forward(v_speaker.cpu(), v_listener.cpu(), v_audio.cpu(), mask.cpu(), mode=mode, n_samples=n_samples, **kw)
        return a, b, pred.to(dev)


def test_protocol_selects_what_the_reference_selects(golden_dir):
    from dimx import x_engine_pt
    gold = np.load(os.path.join(golden_dir, "host_protocol.npz"))
    yt, yp, xs, ids = x_engine_pt.evaluate_test_epoch(_DeviceStub(), stub_model.protocol_batches(), _dev(), beam_size=10,
                                                      fd_backend="hip")
    assert list(ids) == list(gold["test_ids"])
    assert [a.shape[0] for a in yp] == list(gold["test_pred_lens"])
    assert np.array_equal(np.concatenate([np.asarray(a) for a in yp], 0), gold["test_pred"])
    assert x_engine_pt.last_eval_report["fd_backend"] == "hip"


def test_argument_checks_return_an_error_and_enqueue_nothing():
    from dimx import lib as L
    lib = L.load()
    yt, yp, lens = _inputs("B")
    B, S, Ln, W = yp.shape
    d_t, d_p = yt.to(_dev()), yp.to(_dev())
    d_l = torch.tensor(lens, dtype=torch.int32, device=_dev())
    need = int(lib.dimx_op_fd_select_ws_bytes(B, S, 56))
    assert need > 0 and lib.dimx_op_fd_select_ws_bytes(B, S, 0) == 0 and lib.dimx_op_fd_select_ws_bytes(B, S, 65) == 0
    ws = torch.zeros(need, dtype=torch.uint8, device=_dev())
    fd = torch.full((B, S), -7.0, dtype=torch.float64, device=_dev())
    win = torch.full((B,), -7, dtype=torch.int32, device=_dev())
    ok = torch.full((B,), 7, dtype=torch.uint8, device=_dev())
    best = torch.full((B, Ln, W), -7.0, device=_dev())

    def call(c0, F, ws_bytes):
        return lib.dimx_op_fd_select(L.ptr(d_t), d_t.stride(0), d_t.stride(1), L.ptr(d_p), d_p.stride(0), d_p.stride(1), d_p.stride(2),
                                     L.ptr(d_l), B, S, Ln, W, c0, F, L.ptr(fd), L.ptr(win), L.ptr(ok), L.ptr(best),
                                     ctypes.c_void_p(ws.data_ptr()), ws_bytes, L.stream_ptr(_dev()))

    for c0, F, ws_bytes in ((0, 0, need), (0, 65, need), (1, 56, need), (50, 7, need), (0, 56, need - 1)):
        assert call(c0, F, ws_bytes) != 0, (c0, F, ws_bytes)
    torch.cuda.synchronize()
    assert (fd == -7.0).all() and (win == -7).all() and (ok == 7).all() and (best == -7.0).all() and not ws.any()
    assert call(0, 56, need) == 0                      # the same buffers with valid arguments: the call itself works
    torch.cuda.synchronize()
    assert torch.equal(fd.cpu(), _clean_b()[0])
