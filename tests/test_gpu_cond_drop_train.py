"""GPU: condition dropout in the HIP training step (dimx_set_train_cond_keep; the definition is dimx/guidance.py) -- off and
all-ones against the plain step bit for bit, a mixed keep vector against CPU autograd over dimx.train.slmft_loss(cond_keep=)
(checked on the host by tests/test_guidance_host.py), exact zero gradients behind a dropped context, a dropped clip against the
teacher-forced decoder under a zero context, graph replay across draws, and the four launch paths.  3 clips x 71 frames."""
import ctypes

import numpy as np
import pytest
import torch

from test_gpu_prompt import LOGIT_TOL
from test_gpu_train_hip import _inputs, _trainer

pytestmark = pytest.mark.gpu

B, T = 3, 71
KEEP = (1, 0, 1)
CTX_SIDE = ("encoder_s.", "encoder_joint.", "norm_s.", "patch_embed_s", "patch_embed_dec_s")


def _mode(name):
    from dimx import lib
    return lib.MODE_PARITY_F32 if name == "f32" else lib.MODE_PERF_BF16


def _args():
    v_s, v_l, v_a, z, mask = _inputs(B=B, T=T)
    return (v_s.cuda(), v_l.cuda(), v_a.cuda(), mask.cuda()), dict(kv_mask=False, z_l=z.cuda()), (v_s, v_a, z, mask)


def _run(tr, args, kw, keep=None):
    loss, logits = tr.forward_backward(*args, return_logits=True, cond_keep=keep, **kw)
    return loss.clone(), logits, tr.grads.clone()


@pytest.mark.parametrize("mode_name", ["f32", "bf16"])
def test_off_and_all_ones_are_the_plain_step_bit_for_bit(mode_name):
    args, kw, _ = _args()
    _, plain = _trainer(_mode(mode_name))
    l0, g0, d0 = _run(plain, args, kw)
    _, tr = _trainer(_mode(mode_name))
    keep_dev = ctypes.c_void_p(1)
    tr.lib.dimx_train_cond_keep(tr.eng.h, ctypes.byref(keep_dev))
    assert keep_dev.value is None                                        # off from the start
    l1, g1, d1 = _run(tr, args, kw, keep=np.ones(B, dtype=bool))
    tr.lib.dimx_train_cond_keep(tr.eng.h, ctypes.byref(keep_dev))
    assert keep_dev.value == tr._keep.data_ptr()
    assert torch.equal(l0, l1) and torch.equal(g0, g1) and torch.equal(d0, d1)
    l2, g2, d2 = _run(tr, args, kw)                                      # the setter off again
    tr.lib.dimx_train_cond_keep(tr.eng.h, ctypes.byref(keep_dev))
    assert keep_dev.value is None
    assert torch.equal(l0, l2) and torch.equal(g0, g2) and torch.equal(d0, d2)
    l3, _, d3 = _run(tr, args, kw, keep=KEEP)
    assert not torch.equal(l0, l3) and not torch.equal(d0, d3)


def test_mixed_keep_vector_matches_autograd_over_the_checker_f32():
    """loss, logits on the valid rows and every per-tensor gradient at the bounds tests/test_gpu_online_train.py holds the windowed
    step to (1e-5 relative, 1e-4, 1e-3 relative to the tensor's largest gradient)"""
    from dimx import train
    args, kw, (v_s, v_a, z, mask) = _args()
    model, tr = _trainer(_mode("f32"))
    P = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    for t in P.values():
        if t.dtype.is_floating_point:
            t.requires_grad_(True)
    with torch.enable_grad():
        c_loss, c_logits = train.slmft_loss(P, model.s2s, v_s, v_a, mask, z, None, cond_keep=np.array(KEEP, dtype=bool))
        c_loss.backward()
    c_loss, c_logits = c_loss.detach(), c_logits.detach()
    loss, logits, _ = _run(tr, args, kw, keep=KEEP)
    assert abs(loss.item() - c_loss.item()) < 1e-5 * max(1.0, abs(c_loss.item()))
    lerr = (logits.cpu() - c_logits)[mask[:, 1:]].abs().max().item()
    assert lerr < 1e-4
    names = {n for n, _, _ in tr.layout}
    worst, worst_name, checked = 0.0, None, 0
    for name, t in P.items():
        if not t.dtype.is_floating_point or name.startswith(("speaker_vq.", "listener_vq.")):
            continue
        if t.grad is None:
            assert name not in names, name
            continue
        assert name in names, name
        err = (tr.grad(name).cpu() - t.grad).abs().max().item() / max(t.grad.abs().max().item(), 1e-8)
        if err > worst:
            worst, worst_name = err, name
        assert err <= 1e-3, "%s: relative gradient error %.2e" % (name, err)
        checked += 1
    assert checked == len(tr.layout) and checked > 100
    print("step keep=%s: loss %.6f (checker %.6f), logits differ by %.2e, %d tensors, worst relative gradient error %.2e (%s)"
          % (KEEP, loss.item(), c_loss.item(), lerr, checked, worst, worst_name))


@pytest.mark.parametrize("mode_name", ["f32", "bf16"])
def test_all_dropped_sends_exactly_nothing_into_the_context(mode_name):
    args, kw, _ = _args()
    _, tr = _trainer(_mode(mode_name))
    _run(tr, args, kw, keep=np.zeros(B, dtype=bool))
    n = 0
    for name, _, _ in tr.layout:
        if name.startswith(CTX_SIDE):
            assert torch.count_nonzero(tr.grad(name)) == 0, name
            n += 1
    assert n > 20
    assert torch.count_nonzero(tr.grad("decoder_joint.net.to_logits.weight")) > 0
    _run(tr, args, kw, keep=KEEP)
    assert torch.count_nonzero(tr.grad("patch_embed_dec_s")) > 0 and torch.count_nonzero(tr.grad("encoder_s.project_in.weight")) > 0


def test_a_dropped_clip_is_the_decoder_under_a_zero_context():
    args, kw, (v_s, v_a, z, mask) = _args()
    model, tr = _trainer(_mode("f32"))
    _, logits, _ = _run(tr, args, kw, keep=KEEP)
    eng = tr.eng
    m8 = mask.to(torch.uint8).cuda()
    # zero rows after the concat [x + patch_embed_dec_s | audio]: x = -patch_embed_dec_s, audio = 0
    x_null = (-model.state_dict()["patch_embed_dec_s"]).reshape(1, 1, -1).expand(B, T, -1).contiguous().cuda()
    eng.set_context(x_null, torch.zeros_like(v_a).cuda(), which_patch=0, for_generate=False)
    tf_null = eng.decode_tf(z.cuda(), m8)[0]
    eng.encode_ctx(v_s.cuda(), v_a.cuda(), m8, False)
    tf_cond = eng.decode_tf(z.cuda(), m8)[0]
    valid = mask[:, 1:].cuda()
    e_drop = (logits[1] - tf_null[1])[valid[1]].abs().max().item()
    e_keep = max((logits[b] - tf_cond[b])[valid[b]].abs().max().item() for b in (0, 2))
    print("dropped clip against decode_tf under a zero context: %.2e; kept clips against decode_tf under their context: %.2e; the two "
          "contexts differ by %.2f" % (e_drop, e_keep, (tf_null[1] - tf_cond[1])[valid[1]].abs().max().item()))
    assert e_drop < LOGIT_TOL and e_keep < LOGIT_TOL
    assert (tf_null[1] - tf_cond[1])[valid[1]].abs().max().item() > 0.1


def test_a_new_draw_replays_the_captured_step():
    args, kw, _ = _args()
    _, tr = _trainer(_mode("f32"))
    _, _, g_a = _run(tr, args, kw, keep=KEEP)
    _, _, g_a2 = _run(tr, args, kw, keep=KEEP)           # same persistent buffers: captured and launched
    assert tr.graph_stats()[:2] == (1, 1) and torch.equal(g_a, g_a2)
    l_b, d_b, g_b = _run(tr, args, kw, keep=(0, 1, 1))   # new contents in the same vector: a replay
    assert tr.graph_stats()[:2] == (2, 1), "a new draw must not cost a capture"
    assert not torch.equal(g_a, g_b)
    _, fresh = _trainer(_mode("f32"))
    l_f, d_f, g_f = _run(fresh, args, kw, keep=(0, 1, 1))
    assert torch.equal(l_b, l_f) and torch.equal(d_b, d_f) and torch.equal(g_b, g_f)
    _run(tr, args, kw)                                   # off: another pointer, never the captured step
    assert tr.graph_stats()[:2] == (2, 2)


def test_the_trainer_draws_its_own_keep_vector():
    from dimx import guidance
    args, kw, _ = _args()
    _, tr = _trainer(_mode("f32"), cond_drop=0.5, seed=7)
    want = guidance.cond_keep(7, 0, B, 0.5)
    _, d0, g0 = _run(tr, args, kw)
    assert np.array_equal(tr._keep[:B].cpu().numpy().astype(bool), want)
    _, fresh = _trainer(_mode("f32"))
    _, d1, g1 = _run(fresh, args, kw, keep=want)
    assert torch.equal(d0, d1) and torch.equal(g0, g1)


def test_all_launch_paths_give_the_same_bits(monkeypatch):
    args, kw, _ = _args()
    ref = None
    for graph in ("0", "1"):
        for side in ("0", "1"):
            monkeypatch.setenv("DIMX_TRAIN_GRAPH", graph)
            monkeypatch.setenv("DIMX_TRAIN_SIDE", side)
            _, tr = _trainer(_mode("bf16"))
            for it in range(2):
                l, d, g = _run(tr, args, kw, keep=KEEP)
                if ref is None:
                    ref = (l, d.clone(), g)
                assert torch.equal(l, ref[0]) and torch.equal(d, ref[1]) and torch.equal(g, ref[2]), (graph, side, it)
            assert tr.graph_stats()[:2] == ((1, 1) if graph == "1" else (0, 2))


def test_bf16_step_agrees_with_the_f32_one():
    """the bound tests/test_gpu_online_train.py holds the bf16 windowed step to"""
    args, kw, _ = _args()
    _, tb = _trainer(_mode("bf16"))
    _, tf = _trainer(_mode("f32"))
    lb, _, gb = _run(tb, args, kw, keep=KEEP)
    lf, _, gf = _run(tf, args, kw, keep=KEEP)
    rel = ((gb - gf).norm() / gf.norm()).item()
    print("bf16 step with keep=%s: loss %.5f vs f32 %.5f, relative gradient difference %.3f" % (KEEP, lb.item(), lf.item(), rel))
    assert abs(lb.item() - lf.item()) < 2e-2 and rel < 0.05


def test_a_null_handle_and_other_trainers_are_refused():
    from dimx import lib
    _, tr = _trainer(_mode("f32"))
    assert tr.lib.dimx_set_train_cond_keep(None, None) == -1
    with pytest.raises(lib.DimxError):
        from dimx import train_hip
        class Other(train_hip.HipTrainer):
            pass
        Other(tr.model, cond_drop=0.1)
