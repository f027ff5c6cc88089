"""GPU: consensus (minimum-Bayes-risk) best-of-S selection in the HIP library (dimx_op_consensus_select, csrc/consensus.hip) against
its definition (dimx.consensus: numpy float64 around dimx.metrics.clip_fd) on the inputs of tests/test_gpu_fd_select.py, tries only.

Bounds against the definition: 1e-6 relative for "fd" (the bound tests/test_gpu_fd_select.py holds the same arithmetic to on
full-rank clips; every clip here is full rank), 1e-11 relative for "l2" (the project's bound for float64 moments).  The winner is
compared on every clip whose two smallest risks differ by more than 1e-4 relative, 100 x the distance bound, and no clip of the
cases A, B and D is closer than that (asserted; the definition's smallest margins are 6.1e-4 for fd, case D clip 0, and 1.0e-3 for
l2, case A clip 0).  The worst errors are printed."""
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
    "B": (11, 4, 3, 70, [70, 57, 64, 61], [(0, 6), (6, 56)]),
    "D": (13, 2, 10, 330, [330, 299], [(0, 56)]),
    # the boundaries of the shared templates (csrc/frechet.hpp), rows of 64 columns: tests/test_gpu_fd_select.py, case E
    "E": (14, 2, 2, 80, [80, 66], [(0, 64), (3, 10), (0, 8), (0, 9), (5, 6)]),
}
WIDTH = {"E": 64}
CASE_WINDOWS = [(k, w) for k in "ABD" for w in CASES[k][5]]
EDGE_WINDOWS = CASES["E"][5]
BOUND = {"fd": 1e-6, "l2": 1e-11}
MARGIN = 1e-4
ERR_ARG = -1


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """the generator of tests/test_gpu_fd_select.py; only the tries are used"""
    seed, B, S, L, lens, _ = CASES[name]
    g = torch.Generator().manual_seed(seed)
    W = WIDTH.get(name, 56)
    yt = torch.randn(B, L, W, generator=g)
    yp = 0.6 * yt[:, None] + 0.5 * torch.randn(B, S, L, W, generator=g)
    return yp, list(lens)


@functools.lru_cache(maxsize=None)
def _reference(name, window, distance):
    """the definition per clip -> (D [B, S, S], risk [B, S]); computed once per (case, window, distance), never modified"""
    from dimx import consensus
    yp, lens = _inputs(name)
    D = np.stack([consensus.pairwise(yp[j].numpy(), lens[j], window, distance) for j in range(yp.shape[0])])
    risk = consensus.risks(D)
    D.setflags(write=False)
    risk.setflags(write=False)
    return D, risk


def _dev():
    return torch.device("cuda:0")


def _run(yp, lens, window=(0, 56), distance="fd", tokens=None):
    from dimx.engine import op_consensus_select
    out = op_consensus_select(yp, lens, cols=window, distance=distance, tokens=tokens, want_dist=True)
    return tuple(t.cpu() for t in out)      # (risk, win, ok, best[, best_tokens], dist)


@functools.lru_cache(maxsize=None)
def _clean_b(distance):
    yp, lens = _inputs("B")
    return _run(yp.to(_dev()), lens, distance=distance)


def _same(a, b):
    return all(torch.equal(p.view(torch.int64) if p.dtype == torch.float64 else p, q.view(torch.int64) if q.dtype == torch.float64 else q)
               for p, q in zip(a, b))


def _host_risks(dist):
    """the ascending-j sum from zero of the kernel's own distances, on the host"""
    d = dist.numpy()
    S = d.shape[-1]
    risk = np.zeros(d.shape[:-1])
    for j in range(S):
        risk += np.where(np.arange(S) == j, 0.0, d[..., j])
    return risk


def _check(name, window, distance, need_margin):
    from dimx import consensus
    yp, lens = _inputs(name)
    ref_d, ref_risk = _reference(name, window, distance)
    risk, win, ok, best, dist = _run(yp.to(_dev()), lens, window, distance)
    B, S = ref_risk.shape
    d = dist.numpy()
    off = ~np.eye(S, dtype=bool)
    assert np.isfinite(ref_d).all() and (ref_d[:, off] > 0).all()              # the bound is not met vacuously
    err = np.abs(d[:, off] - ref_d[:, off]) / np.abs(ref_d[:, off])
    print("case %s window %s %s: worst relative error of a distance %.3e (bound %.0e)" % (name, window, distance, err.max(), BOUND[distance]))
    assert (err <= BOUND[distance]).all()
    assert np.array_equal(d, d.transpose(0, 2, 1)) and not d[:, ~off].any()    # exactly symmetric, zero diagonal
    assert np.array_equal(risk.numpy().view(np.int64), _host_risks(dist).view(np.int64))
    margins = consensus.margins(ref_risk)
    want, _ = consensus.pick(ref_risk)
    print("case %s window %s %s: margins of the definition %s" % (name, window, distance, ["%.2e" % m for m in margins]))
    if need_margin:
        assert (margins > MARGIN).all(), "a clip of case %s is closer than the winner check allows: %s" % (name, margins)
    for j in range(B):
        if margins[j] > MARGIN:
            assert int(win[j]) == int(want[j]), "clip %d" % j
    own, _ = consensus.pick(risk.numpy())
    assert win.tolist() == own.tolist() and ok.tolist() == [1] * B
    for j in range(B):
        assert torch.equal(best[j, :lens[j]], yp[j, int(win[j]), :lens[j]])    # the full row, also for the sliced windows
        assert not best[j, lens[j]:].any()
    return win


@pytest.mark.parametrize("distance", ["fd", "l2"])
@pytest.mark.parametrize("name,window", CASE_WINDOWS, ids=["%s-%d-%d" % (k, w[0], w[1]) for k, w in CASE_WINDOWS])
def test_distances_risks_winner_and_gather_match_the_definition(name, window, distance):
    _check(name, window, distance, need_margin=True)


@pytest.mark.parametrize("distance", ["fd", "l2"])
@pytest.mark.parametrize("window", EDGE_WINDOWS, ids=["E-%d-%d" % w for w in EDGE_WINDOWS])
def test_template_boundaries(window, distance):
    from dimx.engine import consensus_select_sweeps
    _, B, S, _, lens, _ = CASES["E"]
    F = window[1] - window[0]
    assert min(lens) >= F + 1                                  # full rank: the bound applies to every clip
    win = _check("E", window, distance, need_margin=False)
    assert win.tolist() == [0] * B                             # two tries: the two risks are the same bits, the first one wins
    if distance == "fd":
        sw_f, sw_p = (t.cpu() for t in consensus_select_sweeps(_dev(), B, S, F))
        print("window %s F=%d sweeps: factor %d..%d, pair %d..%d" % (window, F, int(sw_f.min()), int(sw_f.max()), int(sw_p.min()),
                                                                     int(sw_p.max())))
        assert tuple(sw_f.shape) == (B, S) and tuple(sw_p.shape) == (B, S * (S - 1) // 2)
        assert int(sw_f.min()) >= 1 and int(sw_p.min()) >= 1
        assert int(sw_f.max()) < 30 and int(sw_p.max()) < 30


def test_sweep_counts_of_the_largest_case():
    from dimx.engine import consensus_select_sweeps
    _, B, S, _, lens, _ = CASES["D"]
    yp, lens = _inputs("D")
    _run(yp.to(_dev()), lens)
    sw_f, sw_p = (t.cpu() for t in consensus_select_sweeps(_dev(), B, S, 56))
    print("case D sweeps: factor %d..%d, pair %d..%d" % (int(sw_f.min()), int(sw_f.max()), int(sw_p.min()), int(sw_p.max())))
    assert tuple(sw_p.shape) == (B, 45)
    assert int(sw_f.min()) >= 1 and int(sw_p.min()) >= 1 and int(sw_f.max()) < 30 and int(sw_p.max()) < 30


@pytest.mark.parametrize("distance", ["fd", "l2"])
def test_three_identical_tries_and_an_outlier(distance):
    yp, lens = _inputs("A")
    yp = yp.clone()
    yp[:, 1] = yp[:, 0]
    yp[:, 2] = yp[:, 0]
    risk, win, ok, best, dist = _run(yp.to(_dev()), lens, distance=distance)
    r = risk.view(torch.int64)
    assert torch.equal(r[:, 0], r[:, 1]) and torch.equal(r[:, 0], r[:, 2])
    assert bool((risk[:, 3] > risk[:, 0]).all())
    assert win.tolist() == [0] * len(lens) and ok.tolist() == [1] * len(lens)
    d = dist.view(torch.int64)
    assert torch.equal(d[:, 0, 3], d[:, 1, 3]) and torch.equal(d[:, 0, 3], d[:, 2, 3])
    assert torch.equal(d[:, 0, 1], d[:, 0, 2]) and torch.equal(d[:, 0, 1], d[:, 1, 2])
    if distance == "l2":
        assert not dist[:, 0, 1].any()


@pytest.mark.parametrize("distance", ["fd", "l2"])
def test_repeats_strided_views_and_padding(distance):
    yp, lens = _inputs("B")
    B, S, L, W = yp.shape
    clean = _clean_b(distance)
    assert _same(_run(yp.to(_dev()), lens, distance=distance), clean)
    shifted = torch.full((B, S, L + 1, W), float("nan"))
    shifted[:, :, 1:] = yp
    view = shifted.to(_dev())[:, :, 1:]
    assert not view.is_contiguous()
    assert _same(_run(view, lens, distance=distance), clean)
    wide = torch.full((B, S, L, W + 9), float("nan"))
    wide[..., :W] = yp
    view = wide.to(_dev())[..., :W]
    assert not view.is_contiguous() and view.stride(-1) == 1
    assert _same(_run(view, lens, distance=distance), clean)
    nanpad = yp.clone()
    for j, n in enumerate(lens):
        nanpad[j, :, n:] = float("nan")
    assert _same(_run(nanpad.to(_dev()), lens, distance=distance), clean)


@pytest.mark.parametrize("distance", ["fd", "l2"])
def test_a_clip_of_one_frame_is_flagged_and_leaves_the_others_alone(distance):
    yp, _ = _inputs("B")
    lens = [70, 1, 64, 61]
    risk, win, ok, best, dist = _run(yp.to(_dev()), lens, distance=distance)
    c_risk, c_win, c_ok, c_best, c_dist = _clean_b(distance)
    S = yp.shape[1]
    off = ~torch.eye(S, dtype=torch.bool)
    assert ok.tolist() == [1, 0, 1, 1] and int(win[1]) == 0
    assert torch.isnan(dist[1][off]).all() and not dist[1][~off].any() and torch.isnan(risk[1]).all()
    assert not best[1].any()
    for j in (0, 2, 3):
        assert _same((risk[j], dist[j], best[j]), (c_risk[j], c_dist[j], c_best[j])) and int(win[j]) == int(c_win[j])


def test_a_rank_deficient_clip_picks_the_first_minimum_of_its_own_risks():
    from dimx import consensus
    yp, _ = _inputs("A")
    lens = [90, 20, 64, 90, 58]                                # n = 20 < F + 1 = 57
    risk, win, ok, best, dist = _run(yp.to(_dev()), lens)
    assert torch.isfinite(risk).all() and torch.isfinite(dist).all()
    own, own_ok = consensus.pick(risk.numpy())
    assert win.tolist() == own.tolist() and ok.tolist() == [1] * 5
    assert torch.equal(best[1, :20], yp[1, int(win[1]), :20]) and not best[1, 20:].any()


@pytest.mark.parametrize("distance", ["fd", "l2"])
def test_a_single_try(distance):
    yp, lens = _inputs("B")
    risk, win, ok, best, dist = _run(yp[:, :1].to(_dev()), lens, distance=distance)
    assert not risk.any() and not dist.any() and win.tolist() == [0] * 4 and ok.tolist() == [1] * 4
    for j, n in enumerate(lens):
        assert torch.equal(best[j, :n], yp[j, 0, :n]) and not best[j, n:].any()


def test_tokens_are_gathered_with_the_winner():
    yp, _ = _inputs("B")
    lens = [70, 1, 64, 61]
    B, S = yp.shape[:2]
    tok = torch.arange(B * S * 13, dtype=torch.int32).reshape(B * S, 13)
    wide = torch.full((B * S, 20), -5, dtype=torch.int32)
    wide[:, :13] = tok
    for t in (tok.to(_dev()), wide.to(_dev())[:, :13], tok.long().to(_dev())):
        risk, win, ok, best, best_tok, dist = _run(yp.to(_dev()), lens, tokens=t)
        assert ok.tolist() == [1, 0, 1, 1]
        for j in range(B):
            want = tok[j * S + int(win[j])] if ok[j] else torch.full((13,), -100, dtype=torch.int32)
            assert torch.equal(best_tok[j], want)
    from dimx.engine import op_consensus_select
    out = op_consensus_select(yp.to(_dev()), lens, want_best=False)
    assert len(out) == 4 and out[3] is None and torch.equal(out[1].cpu(), win)


def test_the_metrics_wrapper_returns_the_distances():
    from dimx.metrics import consensus_distances_hip
    yp, lens = _inputs("B")
    for distance in ("fd", "l2"):
        d = consensus_distances_hip(yp.to(_dev()), lens, distance=distance).cpu()
        assert torch.equal(d.view(torch.int64), _clean_b(distance)[-1].view(torch.int64))


def test_bad_arguments_return_an_error_and_leave_the_outputs_untouched():
    from dimx import lib as L
    lib = L.load()
    yp, lens = _inputs("B")
    B, S, Ln, W = yp.shape
    d_p = yp.to(_dev())
    d_l = torch.tensor(lens, dtype=torch.int32, device=_dev())
    need = int(lib.dimx_op_consensus_select_ws_bytes(B, S, 56, 0))
    ws = torch.zeros(need + 8, dtype=torch.uint8, device=_dev())
    dist = torch.full((B, S, S), -7.0, dtype=torch.float64, device=_dev())
    risk = torch.full((B, S), -7.0, dtype=torch.float64, device=_dev())
    win = torch.full((B,), -7, dtype=torch.int32, device=_dev())
    ok = torch.full((B,), 7, dtype=torch.uint8, device=_dev())
    best = torch.full((B, Ln, W), -7.0, device=_dev())
    btok = torch.full((B, 4), -7, dtype=torch.int32, device=_dev())

    def call(c0=0, F=56, kind=0, ws_bytes=need, ws_off=0, risk_p=L.ptr(risk), lens_p=L.ptr(d_l), n_tok=0, btok_p=None, S_=S):
        return lib.dimx_op_consensus_select(L.ptr(d_p), d_p.stride(0), d_p.stride(1), d_p.stride(2), lens_p, B, S_, Ln, W, c0, F, kind,
                                            L.ptr(dist), risk_p, L.ptr(win), L.ptr(ok), L.ptr(best), None, 0, n_tok, btok_p,
                                            ctypes.c_void_p(ws.data_ptr() + ws_off), ws_bytes, L.stream_ptr(_dev()))

    bad = (dict(F=0), dict(F=65), dict(c0=1), dict(c0=50, F=7), dict(c0=-1, F=6), dict(kind=2), dict(kind=-1), dict(ws_bytes=need - 1),
           dict(ws_off=4), dict(risk_p=None), dict(lens_p=None), dict(S_=0), dict(n_tok=4, btok_p=L.ptr(btok)))
    for kw in bad:
        assert call(**kw) == ERR_ARG, kw
    torch.cuda.synchronize()
    assert (dist == -7.0).all() and (risk == -7.0).all() and (win == -7).all() and (ok == 7).all() and (best == -7.0).all()
    assert (btok == -7).all() and not ws.any()
    assert call() == 0                                 # the same buffers with valid arguments: the call itself works
    torch.cuda.synchronize()
    assert torch.equal(dist.cpu().view(torch.int64), _clean_b("fd")[-1].view(torch.int64))


# ---- the protocol
class _DeviceStub(stub_model.StubSLMFT):
    """the CPU stub behind device tensors; a beam search is stood in for by ``num_return`` fixed tries (the same at every call, as a
    beam's n-best list is)"""

    def forward(self, v_speaker, v_listener, v_audio, mask, mode="train", n_samples=1, beam_width=None, num_return=None, **kw):
        dev = v_listener.device
        if beam_width is not None:
            pred = torch.stack([self._sample(100 + s, v_speaker.cpu(), v_listener.cpu()) for s in range(int(num_return))], 1)
            return torch.zeros(()), {}, pred.to(dev)
        a, b, pred = super().forward(v_speaker.cpu(), v_listener.cpu(), v_audio.cpu(), mask.cpu(), mode=mode, n_samples=n_samples)
        return a, b, pred.to(dev)


@pytest.mark.parametrize("distance", ["fd", "l2"])
@pytest.mark.parametrize("decode", ["sample", "beam"])
def test_protocol_keeps_the_try_the_operator_picks(decode, distance):
    from dimx import x_engine_pt
    from dimx.engine import op_consensus_select
    loader = stub_model.protocol_batches()[1:]                 # one batch of 3 clips
    kw = dict(beam_size=5) if decode == "sample" else dict(decode="beam", beam_width=4)
    S = 5 if decode == "sample" else 4
    y_true, y_pred, x, ids = x_engine_pt.evaluate_test_epoch(_DeviceStub(), loader, _dev(), select="consensus",
                                                             consensus_distance=distance, **kw)
    assert len(y_true) == len(y_pred) == len(x) == len(ids) == 3
    assert x_engine_pt.last_eval_report["fd_backend"] is None
    src_s_v, src_s_a, tgt, mask, src_len, _ = x_engine_pt._prepare(loader[0], _dev())
    tries_kw = dict(n_samples=5) if decode == "sample" else dict(beam_width=4, num_return=4)
    tries = _DeviceStub()(src_s_v, tgt, src_s_a, mask, mode="val", **tries_kw)[2]       # a fresh stub: the same tries again
    assert tuple(tries.shape) == (3, S, tgt.shape[1] - 1, 56)
    lens = [n - 1 for n in src_len]
    risk, win, ok, best = op_consensus_select(tries, lens, distance=distance)
    assert ok.tolist() == [1, 1, 1]
    for j, n in enumerate(lens):
        assert y_pred[j].shape == (n, 56)
        assert np.array_equal(y_pred[j], tries[j, int(win[j]), :n].cpu().numpy()), "clip %d" % j
        assert np.array_equal(y_true[j], tgt[j, 1:n + 1].cpu().numpy())
    if distance == "fd":                                       # the default distance is "fd"
        again = x_engine_pt.evaluate_test_epoch(_DeviceStub(), loader, _dev(), select="consensus", **kw)[1]
        assert all(np.array_equal(p, q) for p, q in zip(y_pred, again))
    print("protocol %s %s: winners %s" % (decode, distance, win.tolist()))


def test_protocol_feeds_the_metrics_accumulator_with_the_winners():
    from dimx import x_engine_pt
    from dimx.metrics import ListenerMetrics
    loader = stub_model.protocol_batches()[1:]
    acc = ListenerMetrics()
    _, y_pred, _, _ = x_engine_pt.evaluate_test_epoch(_DeviceStub(), loader, _dev(), beam_size=5, select="consensus", metrics=acc)
    src_s_v, _, tgt, _, src_len, _ = x_engine_pt._prepare(loader[0], _dev())
    lens = [n - 1 for n in src_len]
    best = torch.zeros(3, tgt.shape[1] - 1, 56)
    for j, n in enumerate(lens):
        best[j, :n] = torch.from_numpy(y_pred[j])
    want = ListenerMetrics().update(tgt[:, 1:], best.to(_dev()), src_s_v, lens).result()
    assert acc.result() == want                                # the same kernel on the same rows: the same bits
