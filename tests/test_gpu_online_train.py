"""GPU: online fine-tuning (dimx_set_train_lookahead, dimx_op_train_attention_win) -- the six training attention kernels under the
window of dimx/online.py against float64 autograd over Attend, their exact properties (offline limit, unseen keys, the one-key
floor, no leak, determinism), and the HIP training step under the window against CPU autograd over dimx.train.slmft_loss
(checked on the host by tests/test_online_train_host.py), against the forced online generation it trains for, across the graph
key and both launch paths."""
import ctypes

import numpy as np
import pytest
import torch

from test_gpu_prompt import STEP_TOL
from test_gpu_train_hip import _inputs, _trainer

pytestmark = pytest.mark.gpu

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
ERR_ARG = -1
SCALE = 0.125
MFMA_TOL = ((0, 2e-5), (2, 2e-5), (1, 1e-2))      # tests/test_gpu_train_hip.py: relative norm error; 4 x that in the max norm


def _window(Lq, Lk, L, dev):
    """[Lq, Lk] bool: query i keeps key j < visible(i, L, Lk) (dimx.online.visible_mask for any Lq)"""
    from dimx.online import visible
    vis = torch.from_numpy(np.asarray(visible(np.arange(Lq), L, Lk))).to(dev)
    return torch.arange(Lk, device=dev)[None, :] < vis[:, None]


def _attend_window_reference(q, k, v, d_o, scale, L, kmask, H):
    """x-transformers' Attend in float64 with autograd, the online window and-ed into the keep mask (L None: no window)"""
    B, Lq, _ = q.shape
    Lk = k.shape[1]
    with torch.enable_grad():
        q, k, v = (t.double().detach().requires_grad_(True) for t in (q, k, v))
        sp = lambda t, n: t.view(B, n, H, 64).transpose(1, 2)
        dots = torch.matmul(sp(q, Lq), sp(k, Lk).transpose(-1, -2)) * scale
        keep = torch.ones(B, 1, Lq, Lk, dtype=torch.bool, device=q.device)
        if L is not None:
            keep = keep & _window(Lq, Lk, L, q.device)
        if kmask is not None:
            keep = keep & kmask.bool()[:, None, None, :]
        dots = dots.masked_fill(~keep, -torch.finfo(torch.float32).max)
        o = torch.matmul(dots.softmax(-1), sp(v, Lk)).transpose(1, 2).reshape(B, Lq, H * 64)
        o.backward(d_o.double())
    return o.detach(), q.grad, k.grad, v.grad


def _operands(B, H, Lq, Lk, ragged, dev, tag="wa"):
    from dimx import prng
    g = lambda name, n: torch.from_numpy(prng.normal(41, "%s.%s" % (tag, name), (B, n, H * 64))).to(dev)
    kmask = None
    if ragged:                                       # the last quarter of the last clip dropped, key 0 kept
        kmask = torch.ones(B, Lk, dtype=torch.bool, device=dev)
        kmask[-1, Lk - Lk // 4:] = False
    return g("q", Lq), g("k", Lk), g("v", Lk), g("do", Lq), kmask


BIG = (2, 2, 299, 300)
PARITY = ([((2, 3, 70, 71), L, True) for L in (0, -3, 5)] +
          [(BIG, L, False) for L in (-65, -64, -63, 61, 62, 63, 126, 127, 0, -305, 305, INT32_MIN, INT32_MAX)] +
          [((1, 2, 129, 130), L, False) for L in (0, -1, -2)] +
          [((3, 2, 33, 129), L, True) for L in (0, 40)] +
          [((2, 1, 128, 64), L, False) for L in (0, -3)])
WORST = {}


@pytest.mark.parametrize("shape,L,ragged", PARITY)
def test_windowed_training_attention_matches_attend_and_its_adjoint(shape, L, ragged):
    """forward, dQ, dK, dV of all six kernels against float64 autograd, at the bounds tests/test_gpu_train_hip.py holds the same
    kernels to (a mask does not change the arithmetic).  One case needs a word: when every query sees key 0 only (L <= -Lq)
    dQ and dK are zero in exact arithmetic -- dS = P (dO.v0 - delta) with delta = dO.O = dO.v0 -- so an error relative to the
    reference's norm means nothing there.  Their error is then measured against the terms that cancel, scale (dO_i.v0) k_0 for
    dQ and the root sum of squares over i of scale (dO_i.v0) q_i for dK: the size of what each kernel subtracts.
    Measured on one MI355X, worst relative error over all cases: mfma 0 7.3e-7, mfma 2 7.7e-7 (bound 2e-5), mfma 1 6.7e-3 (bound 1e-2)."""
    from dimx import engine as E
    B, H, Lq, Lk = shape
    dev = torch.device("cuda:0")
    q, k, v, d_o, kmask = _operands(B, H, Lq, Lk, ragged, dev)
    ro, rq, rk, rv = _attend_window_reference(q, k, v, d_o, SCALE, L, kmask, H)
    one_key = bool((_window(Lq, Lk, L, dev).sum(1) == 1).all())
    assert one_key == (L <= -Lq)
    den = {n: (r.norm(), r.abs().max()) for n, r in (("o", ro), ("dq", rq), ("dk", rk), ("dv", rv))}
    if one_key:
        sp = lambda t, n: t.double().view(B, n, H, 64).transpose(1, 2)                     # [B,H,L,64]
        dp = (sp(d_o, Lq) * sp(v, Lk)[:, :, :1]).sum(-1, keepdim=True) * SCALE             # scale (dO_i . v0)  [B,H,Lq,1]
        tq, tk = dp * sp(k, Lk)[:, :, :1], dp * sp(q, Lq)
        den["dq"] = (tq.norm(), tq.abs().max())
        den["dk"] = (tk.norm(), tk.abs().max())
    for mfma, tol in MFMA_TOL:
        o, lse, dq, dk, dv = E.op_train_attention(q, k, v, SCALE, d_o=d_o, kmask=kmask, mfma=mfma, lookahead=L)
        for name, got, ref in (("o", o, ro), ("dq", dq, rq), ("dk", dk, rk), ("dv", dv, rv)):
            err = ((got.double() - ref).norm() / den[name][0]).item()
            worst = ((got.double() - ref).abs().max() / den[name][1]).item()
            print("windowed train attention %s L=%d mfma=%d %s: relative error %.2e (max-norm %.2e)" % (shape, L, mfma, name, err, worst))
            WORST[mfma] = max(WORST.get(mfma, 0.0), err)
            assert torch.isfinite(got).all()
            assert err < tol and worst < 4 * tol, (name, mfma, err, worst)
    print("worst relative error so far per mfma: %s" % {m: "%.2e" % e for m, e in sorted(WORST.items())})


@pytest.fixture(scope="module")
def big():
    dev = torch.device("cuda:0")
    return _operands(*BIG, False, dev)


def _run(ops, mfma, L, k=None, v=None, kmask=None):
    from dimx import engine as E
    q, k0, v0, d_o, _ = ops
    return E.op_train_attention(q, k0 if k is None else k, v0 if v is None else v, SCALE, d_o=d_o, kmask=kmask, mfma=mfma, lookahead=L)


@pytest.mark.parametrize("mfma", [0, 2, 1])
def test_a_window_past_the_last_key_is_the_window_off_bit_for_bit(big, mfma):
    Lk = BIG[3]
    off = _run(big, mfma, None)
    for L in (Lk + 5, INT32_MAX, Lk - 2):
        on = _run(big, mfma, L)
        for name, a, b in zip(("o", "lse", "dq", "dk", "dv"), on, off):
            assert torch.equal(a, b), (name, L)
    again = _run(big, mfma, 0)
    assert not torch.equal(again[0], off[0])
    for a, b in zip(again, _run(big, mfma, 0)):          # a repeated call returns identical bits
        assert torch.equal(a, b)


@pytest.mark.parametrize("mfma", [0, 2, 1])
@pytest.mark.parametrize("shape,L", [(BIG, -65), (BIG, -3), (BIG, 0), ((3, 2, 33, 129), 0), ((3, 2, 33, 129), 40), ((2, 1, 128, 64), -3)])
def test_keys_no_query_sees_get_exactly_zero_gradient(shape, L, mfma):
    from dimx import engine as E
    B, H, Lq, Lk = shape
    q, k, v, d_o, kmask = _operands(B, H, Lq, Lk, shape[2] == 33, torch.device("cuda:0"))
    o, lse, dq, dk, dv = E.op_train_attention(q, k, v, SCALE, d_o=d_o, kmask=kmask, mfma=mfma, lookahead=L)
    last = min(max(Lq + L, 0), Lk - 1)                  # the last key of the last query
    assert torch.count_nonzero(dk[:, last + 1:]) == 0 and torch.count_nonzero(dv[:, last + 1:]) == 0
    assert torch.count_nonzero(dv[0, last]) > 0 and torch.count_nonzero(dk[0, 0]) > 0
    if kmask is not None:                               # keys the mask drops get none either
        assert torch.count_nonzero(dk[-1, Lk - Lk // 4:]) == 0 and torch.count_nonzero(dv[-1, Lk - Lk // 4:]) == 0


@pytest.mark.parametrize("mfma", [0, 2, 1])
@pytest.mark.parametrize("L", [-305, INT32_MIN])
def test_below_the_floor_every_query_sees_key_0_alone(mfma, L):
    """L < -Lq: a one-key softmax.  o[i] is v[0] per head, dK (and dQ) is zero everywhere, key 0 included (dS = P (dO.v0 - dO.o) =
    0), and only dV[0] is not zero -- asserted bit for bit.  The property is exact in exact arithmetic; so that no rounding of the
    kernels' own arithmetic can hide or fake it, v and dO lie on a coarse dyadic grid (multiples of 1/4 in [-2, 2], exact in
    bf16), where every product and every partial sum of dO.v0 is exact in f32 in any order.  q and k are
    ordinary normal draws.  The block and the wave that own key 0 walk every query tile for this to hold (5 tiles here)."""
    from dimx import engine as E
    from dimx import prng
    B, H, Lq, Lk = BIG
    dev = torch.device("cuda:0")
    q, k, _, _, _ = _operands(B, H, Lq, Lk, False, dev)
    grid = lambda name, n: (torch.from_numpy(prng.integers(43, name, (B, n, H * 64), 0, 17)).float() - 8.0).div(4.0).to(dev)
    v, d_o = grid("wa.vg", Lk), grid("wa.dog", Lq)
    o, lse, dq, dk, dv = E.op_train_attention(q, k, v, SCALE, d_o=d_o, mfma=mfma, lookahead=L)
    assert torch.equal(o, v[:, :1].expand(B, Lq, H * 64))
    assert torch.count_nonzero(dk) == 0 and torch.count_nonzero(dq) == 0
    assert torch.count_nonzero(dv[:, 1:]) == 0 and torch.count_nonzero(dv[:, 0]) > 0
    assert (dv[:, 0] - d_o.sum(1)).abs().max() <= 1e-2 * d_o.sum(1).abs().max()


@pytest.mark.parametrize("mfma", [0, 2, 1])
@pytest.mark.parametrize("c", [64, 65])
def test_rows_behind_the_window_do_not_reach_the_output_or_dq(big, mfma, c):
    from dimx import prng
    from dimx.online import visible
    B, H, Lq, Lk = BIG
    dev = torch.device("cuda:0")
    q, k, v, d_o, _ = big
    k2, v2 = k.clone(), v.clone()
    k2[:, c:] = torch.from_numpy(prng.normal(47, "wa.k2", (B, Lk - c, H * 64))).to(dev) * 3.0
    v2[:, c:] = torch.from_numpy(prng.normal(47, "wa.v2", (B, Lk - c, H * 64))).to(dev) * 3.0
    for L in (0, -3, 5, -63):
        a = _run(big, mfma, L)
        b = _run(big, mfma, L, k=k2, v=v2)
        rows = torch.from_numpy(np.asarray(visible(np.arange(Lq), L, Lk)) <= c).to(dev)
        n = int(rows.sum())
        assert n == c - 1 - L
        assert torch.equal(a[0][:, rows], b[0][:, rows]) and torch.equal(a[2][:, rows], b[2][:, rows]), (L, c)
        assert torch.equal(a[1][:, :, rows], b[1][:, :, rows])                     # the row LSE
        assert not torch.equal(a[0][:, n], b[0][:, n]) and not torch.equal(a[2][:, n], b[2][:, n])   # the next row sees key c


def test_the_window_and_causal_together_are_refused():
    from dimx import lib as Lb
    dev = torch.device("cuda:0")
    q, k, v, d_o, _ = _operands(1, 1, 8, 9, False, dev)
    o, lse = torch.full_like(q, -7.0), torch.empty(1, 1, 8, device=dev)
    lib = Lb.load()
    rc = lib.dimx_op_train_attention_win(2, Lb.ptr(q), Lb.ptr(k), Lb.ptr(v), None, None, None, 1, 1, 8, 9, 1, SCALE, 1, 0, Lb.ptr(o), Lb.ptr(lse),
                                         None, None, None, None, Lb.stream_ptr(dev))
    torch.cuda.synchronize()
    assert rc == ERR_ARG and bool((o == -7.0).all())


# ---------------------------------------------------------------------------------------------------------------- the step
def _kv():
    from oracle import ref_cpu
    return ref_cpu.ar_kv_mask(2, 48, 0.15, torch.Generator().manual_seed(3))


def _autograd(model, v_s, v_a, z, mask, kv, L):
    """CPU autograd over dimx.train.slmft_loss(lookahead=L) on the model's own parameters -> (loss, logits, {name: grad})"""
    from dimx import train
    P = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    for t in P.values():
        if t.dtype.is_floating_point:
            t.requires_grad_(True)
    with torch.enable_grad():
        loss, logits = train.slmft_loss(P, model.s2s, v_s, v_a, mask, z, kv, lookahead=L)
        loss.backward()
    return loss.detach(), logits.detach(), {k: t.grad for k, t in P.items() if t.dtype.is_floating_point}


def _check_step(L):
    """loss, logits on the valid rows and every per-tensor gradient of the f32 HIP step under look-ahead L (None: window off)
    against the checker, at the bounds of test_hip_gradients_match_autograd_over_the_oracle_f32"""
    from dimx import lib
    v_s, v_l, v_a, z, mask = _inputs()
    kv = _kv()
    model, tr = _trainer(lib.MODE_PARITY_F32, lookahead=L)
    assert tr.lookahead == L
    c_loss, c_logits, c_grads = _autograd(model, v_s, v_a, z, mask, kv, L)
    loss, logits = tr.forward_backward(v_s.cuda(), v_l.cuda(), v_a.cuda(), mask.cuda(), kv_mask=kv.cuda(), z_l=z.cuda(), return_logits=True)
    assert abs(loss.item() - c_loss.item()) < 1e-5 * max(1.0, abs(c_loss.item()))
    lerr = (logits.cpu() - c_logits)[mask[:, 1:]].abs().max().item()
    assert lerr < 1e-4
    names = {n for n, _, _ in tr.layout}
    worst, worst_name, checked = 0.0, None, 0
    for name, g_c in c_grads.items():
        if name.startswith(("speaker_vq.", "listener_vq.")):
            continue
        if g_c is None:
            assert name not in names, name
            continue
        assert name in names, name
        err = (tr.grad(name).cpu() - g_c).abs().max().item() / max(g_c.abs().max().item(), 1e-8)
        if err > worst:
            worst, worst_name = err, name
        assert err <= 1e-3, "%s: relative gradient error %.2e" % (name, err)
        checked += 1
    assert checked == len(tr.layout) and checked > 100
    print("step L=%s: loss %.6f (checker %.6f), logits differ by %.2e, %d tensors, worst relative gradient error %.2e (%s)"
          % (L, loss.item(), c_loss.item(), lerr, checked, worst, worst_name))
    return loss.item()


@pytest.fixture(scope="module")
def offline_loss():
    """the checker is sound before it is trusted with the window: lookahead=None against the window-off step, same bounds"""
    return _check_step(None)


@pytest.mark.parametrize("L", [0, -3, 5])
def test_windowed_step_matches_autograd_over_the_checker_f32(offline_loss, L):
    loss = _check_step(L)
    assert abs(loss - offline_loss) > 1e-4              # the window changes the loss by more than the bound could hide


@pytest.mark.parametrize("mode_name", ["f32", "bf16"])
def test_a_window_of_the_whole_clip_is_the_offline_step_bit_for_bit(mode_name):
    from dimx import lib
    mode = lib.MODE_PARITY_F32 if mode_name == "f32" else lib.MODE_PERF_BF16
    v_s, v_l, v_a, z, mask = _inputs()
    kv = _kv()
    args = (v_s.cuda(), v_l.cuda(), v_a.cuda(), mask.cuda())
    _, tr0 = _trainer(mode)
    _, tr1 = _trainer(mode, lookahead=48)
    l0, g0 = tr0.forward_backward(*args, kv_mask=kv.cuda(), z_l=z.cuda(), return_logits=True)
    l1, g1 = tr1.forward_backward(*args, kv_mask=kv.cuda(), z_l=z.cuda(), return_logits=True)
    assert torch.equal(l0, l1) and torch.equal(g0, g1) and torch.equal(tr0.grads, tr1.grads)
    tr1.set_lookahead(46)                                # T - 2: still everything
    l2 = tr1.forward_backward(*args, kv_mask=kv.cuda(), z_l=z.cuda())
    assert torch.equal(l0, l2) and torch.equal(tr0.grads, tr1.grads)


@pytest.mark.parametrize("mode_name", ["f32", "bf16"])
@pytest.mark.parametrize("L", [0, -3])
def test_the_step_does_not_see_a_perturbed_future(mode_name, L):
    from dimx import lib
    from dimx.online import visible
    mode = lib.MODE_PARITY_F32 if mode_name == "f32" else lib.MODE_PERF_BF16
    T, CUT = 48, 20
    v_s, v_l, v_a, z, mask = _inputs()
    v_s2, v_a2 = v_s.clone(), v_a.clone()
    v_s2[:, CUT:] += 1.0
    v_a2[:, CUT:] -= 0.5
    _, tr = _trainer(mode, lookahead=L)
    _, a = tr.forward_backward(v_s.cuda(), v_l.cuda(), v_a.cuda(), mask.cuda(), kv_mask=False, z_l=z.cuda(), return_logits=True)
    _, b = tr.forward_backward(v_s2.cuda(), v_l.cuda(), v_a2.cuda(), mask.cuda(), kv_mask=False, z_l=z.cuda(), return_logits=True)
    rows = torch.from_numpy(np.asarray(visible(np.arange(T - 1), L, T)) <= CUT).cuda()
    assert int(rows.sum()) == CUT - 1 - L
    assert torch.equal(a[:, rows], b[:, rows])
    assert not torch.equal(a[0, T - 2], b[0, T - 2]) and not torch.equal(a[1, T - 2], b[1, T - 2])
    tr.set_lookahead(None)                               # the offline step looks at the perturbed frames from row 0 on
    _, c = tr.forward_backward(v_s.cuda(), v_l.cuda(), v_a.cuda(), mask.cuda(), kv_mask=False, z_l=z.cuda(), return_logits=True)
    _, d = tr.forward_backward(v_s2.cuda(), v_l.cuda(), v_a2.cuda(), mask.cuda(), kv_mask=False, z_l=z.cuda(), return_logits=True)
    assert not torch.equal(c[0, 0], d[0, 0])


def test_bf16_windowed_step_agrees_with_the_f32_one():
    from dimx import lib
    v_s, v_l, v_a, z, mask = _inputs(B=4, T=40, seed=5)
    args = (v_s.cuda(), v_l.cuda(), v_a.cuda(), mask.cuda())
    _, tb = _trainer(lib.MODE_PERF_BF16, lookahead=0)
    _, tf = _trainer(lib.MODE_PARITY_F32, lookahead=0)
    lb = tb.forward_backward(*args, kv_mask=False, z_l=z.cuda()).item()
    lf = tf.forward_backward(*args, kv_mask=False, z_l=z.cuda()).item()
    rel = ((tb.grads - tf.grads).norm() / tf.grads.norm()).item()
    print("bf16 windowed training step (L = 0): loss %.5f vs f32 %.5f, relative gradient difference %.3f" % (lb, lf, rel))
    assert abs(lb - lf) < 2e-2 and rel < 0.05


def test_the_window_keys_the_captured_step():
    from dimx import lib
    v_s, v_l, v_a, z, mask = _inputs()
    args = (v_s.cuda(), v_l.cuda(), v_a.cuda(), mask.cuda())
    kw = dict(kv_mask=False, z_l=z.cuda())
    _, tr = _trainer(lib.MODE_PARITY_F32)
    l_off = tr.forward_backward(*args, **kw)
    g_off = tr.grads.clone()
    tr.forward_backward(*args, **kw)                     # same persistent buffers: captured and launched
    assert tr.graph_stats()[:2] == (1, 1) and torch.equal(tr.grads, g_off)
    tr.set_lookahead(0)
    l_on = tr.forward_backward(*args, **kw)
    g_on = tr.grads.clone()
    assert tr.graph_stats()[:2] == (1, 2), "the window-off graph was replayed under the window"
    _, fresh = _trainer(lib.MODE_PARITY_F32, lookahead=0)
    l_f = fresh.forward_backward(*args, **kw)
    assert torch.equal(l_on, l_f) and torch.equal(g_on, fresh.grads) and not torch.equal(g_on, g_off)
    tr.forward_backward(*args, **kw)                     # the window-on step is captured under its own key
    assert tr.graph_stats()[:2] == (2, 2) and torch.equal(tr.grads, g_on)
    tr.set_lookahead(-3)
    tr.forward_backward(*args, **kw)
    assert tr.graph_stats()[:2] == (2, 3) and not torch.equal(tr.grads, g_on)
    tr.set_lookahead(None)
    for _ in range(2):
        l = tr.forward_backward(*args, **kw)
        assert torch.equal(l, l_off) and torch.equal(tr.grads, g_off)


def test_both_launch_paths_give_the_same_windowed_gradients(monkeypatch):
    from dimx import lib
    v_s, v_l, v_a, z, mask = _inputs(B=2, T=48, seed=37)
    args = (v_s.cuda(), v_l.cuda(), v_a.cuda(), mask.cuda())
    ref = None
    for graph in ("0", "1"):
        for side in ("0", "1"):
            monkeypatch.setenv("DIMX_TRAIN_GRAPH", graph)
            monkeypatch.setenv("DIMX_TRAIN_SIDE", side)
            _, tr = _trainer(lib.MODE_PERF_BF16, lookahead=0)
            for it in range(2):
                l = tr.forward_backward(*args, kv_mask=False, z_l=z.cuda()).item()
                if ref is None:
                    ref = (l, tr.grads.clone())
                assert l == ref[0] and torch.equal(tr.grads, ref[1]), (graph, side, it)
            assert tr.graph_stats()[:2] == ((1, 1) if graph == "1" else (0, 2))
    _, off = _trainer(lib.MODE_PERF_BF16)
    off.forward_backward(*args, kv_mask=False, z_l=z.cuda())
    assert not torch.equal(off.grads, ref[1])


@pytest.mark.parametrize("L", [0, -3])
def test_the_step_trains_what_the_online_generation_runs(L):
    """the step's logits_out against the logits a fully forced online generation dumps (the route of SLMFT.score(lookahead=L)):
    the same tokens, no mask_prob draw, the valid rows; the bound is the project's for forced steps against a teacher-forced
    checker (STEP_TOL of tests/test_gpu_online.py)."""
    from dimx import lib
    T = 48
    v_s, v_l, v_a, z, mask = _inputs()
    model, tr = _trainer(lib.MODE_PARITY_F32, lookahead=L)
    dev = [t.cuda() for t in (v_s, v_l, v_a, mask)]
    _, logits = tr.forward_backward(*dev, kv_mask=False, z_l=z.cuda(), return_logits=True)
    with torch.no_grad(), model.engine_pinned():
        eng = model.engine(dev[0].device)
        m8 = model._mask8(dev[3])
        model._build_context(eng, None, dev[0], dev[2], m8, True)
        _, gen = eng.generate(None, m8, T, 0.0, 52, None, 0, return_logits=True, prompt=z.cuda()[:, :T - 1], prefill=1, no_prefill=True,
                              lookahead=L)
        model._build_context(eng, None, dev[0], dev[2], m8, False)
        off, _, _ = eng.decode_tf(z.cuda(), m8, None)
    assert eng.cross_lookahead() is None                 # generation's setting and the trainer's do not touch each other
    valid = mask[:, 1:]
    err = (logits - gen.view_as(logits)).cpu()[valid].abs().max().item()
    gap = (logits - off.view_as(logits)).cpu()[valid].abs().max().item()
    print("L=%d: step logits against the forced online generation: %.2e (against the offline teacher-forced pass: %.2f)" % (L, err, gap))
    assert err < STEP_TOL
    assert gap > 10 * STEP_TOL


def test_training_under_the_window_reduces_the_loss():
    from dimx import lib
    v_s, v_l, v_a, z, mask = _inputs(B=4, T=40, seed=5)
    args = (v_s.cuda(), v_l.cuda(), v_a.cuda(), mask.cuda())
    _, tr = _trainer(lib.MODE_PARITY_F32, lr=3e-4, lookahead=0)
    l0 = tr.train_step(*args, kv_mask=False, z_l=z.cuda()).item()
    for _ in range(5):
        l1 = tr.train_step(*args, kv_mask=False, z_l=z.cuda()).item()
    print("six windowed training steps (L = 0, lr 3e-4): loss %.4f -> %.4f" % (l0, l1))
    assert l1 < l0


def test_refusals_and_handle_state():
    from dimx import engine, lib as Lb
    from dimx import train_hip
    from dimx.seq2seq_pretrain import SLM

    def read(e):
        on, la = ctypes.c_int(-9), ctypes.c_int(-9)
        Lb.check(e.lib.dimx_train_lookahead(e.h, ctypes.byref(on), ctypes.byref(la)), "dimx_train_lookahead")
        return on.value, la.value

    for variant in ("slm", "legacy"):
        other = engine.Engine("cuda:0", Lb.MODE_PARITY_F32, variant=variant)
        rc = other.lib.dimx_set_train_lookahead(other.h, 1, 0)
        assert rc == ERR_ARG and b"variant" in other.lib.dimx_last_error()
        assert other.lib.dimx_set_train_lookahead(other.h, 0, 0) == ERR_ARG
        assert read(other) == (0, 0)
        other.close()
    e = engine.Engine("cuda:0", Lb.MODE_PARITY_F32)
    assert read(e) == (0, 0) and e.cross_lookahead() is None
    for L in (0, -3, 5, INT32_MIN, INT32_MAX):
        Lb.check(e.lib.dimx_set_train_lookahead(e.h, 1, L), "dimx_set_train_lookahead")
        assert read(e) == (1, L)
        assert e.cross_lookahead() is None               # the generation's window is untouched
    e.set_cross_lookahead(7)
    assert read(e) == (1, INT32_MAX) and e.cross_lookahead() == 7
    Lb.check(e.lib.dimx_set_train_lookahead(e.h, 0, 11), "dimx_set_train_lookahead")
    assert read(e) == (0, 0) and e.cross_lookahead() == 7   # on = 0 resets the look-ahead
    e.set_cross_lookahead(None)
    assert read(e) == (0, 0)
    Lb.check(e.lib.dimx_train_lookahead(e.h, None, None), "dimx_train_lookahead")
    e.close()
    with pytest.raises(Lb.DimxError):                    # the other steps do not take the setting
        train_hip.SlmHipTrainer(SLM().cuda()).set_lookahead(0)
