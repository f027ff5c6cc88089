"""GPU: the VQ-VAE's own training step (stage 1, reference loop code/train_vq.py:173-196) on the HIP kernels
(dimx.train_hip.VqHipTrainer -> csrc/train.hip vq_run, vqenc_* / vqdec_*, csrc/train_vq.hip):
  * f32, no dropout: against one step of the reference (tests/golden/vq_train_B2_T27.npz), against PyTorch autograd over
    dimx.train.vq_loss at three shapes, codes equal to dimx_vq_encode's, bit-identical reruns;
  * dropout 0.1: against vq_loss given the mirrored keep masks (dimx.prng.dropout_keep);
  * training: the loss falls, 2 steps equal vq_loss + torch.optim.AdamW, bf16 agrees;
  * hand-off: the checkpoint loads through SLMFT(vq_listener_ckpt=...) and encodes as the trainer did; examples/train_vq.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20260928


def _cfg():
    from dimx.config import load_cfg_from_cfg_file
    return load_cfg_from_cfg_file(os.path.join(ROOT, "dyadic-interaction-modeling_amd", "config.yaml"))


def _model(mode=None):
    from dimx import lib
    from dimx.models import VQAutoEncoder
    return VQAutoEncoder(_cfg(), numeric_mode=lib.MODE_PARITY_F32 if mode is None else mode).cuda()


def _x(B, T, tag="vqtr.x", seed=3):
    from dimx import prng
    return torch.from_numpy(prng.normal(seed, tag, (B, T, 56))).cuda()


def _autograd(model, x, masks=None, idx=None):
    from dimx import train as TR
    with torch.enable_grad():
        P = {k: v.detach().clone().requires_grad_(not k.endswith(".pe")) for k, v in model.state_dict().items()}
        out = TR.vq_loss(P, x, masks=masks, idx=idx)
        out[0].backward()
    return out, {k: v.grad for k, v in P.items() if not k.endswith(".pe")}


def _worst(tr, grads):
    worst = 0.0
    for name, g_a in grads.items():
        g_h = tr.grad(tr.prefix + name)
        rel = (g_h - g_a).abs().max().item() / max(g_a.abs().max().item(), 1e-12)
        worst = max(worst, rel)
    return worst


def test_vq_step_matches_the_reference_fixture(golden_dir):
    from dimx import prng
    from dimx.train_hip import VqHipTrainer
    g = np.load(os.path.join(golden_dir, "vq_train_B2_T27.npz"))
    model = _model()
    tr = VqHipTrainer(model, dropout=0.0)
    assert len(tr.layout) == 148 and sum(n for _, _, n in tr.layout) == 23258496
    x = torch.from_numpy(prng.normal(SEED, "vq_train.x", (2, 27, 56))).cuda()
    d, pred, idx = tr.forward_backward(x)
    assert np.array_equal(idx.cpu().numpy(), g["idx"])
    for key, k2 in (("loss", "loss"), ("rec_loss", "rec_loss"), ("quant_loss", "quant_loss"), ("perplexity", "perplexity")):
        want = float(g[k2])
        assert abs(d[key].item() - want) <= 1e-5 * abs(want), (key, d[key].item(), want)
    assert (pred.cpu() - torch.from_numpy(g["pred"])).abs().max().item() <= 1e-4 * float(np.abs(g["pred"]).max())
    for i, name in enumerate(str(n) for n in g["names"]):
        gh = tr.grad("listener_vq." + name).double().reshape(-1).cpu()
        gmax = float(np.abs(g["grad_samples"][i]).max())
        assert abs(float(gh.norm()) - g["grad_norm"][i]) <= 1e-4 * max(g["grad_norm"][i], gmax), name
        pos = torch.from_numpy(prng.integers(SEED, "vq_train.sample." + name, (128,), 0, gh.numel()))
        assert np.abs(gh[pos].numpy() - g["grad_samples"][i]).max() <= 1e-4 * max(float(gh.abs().max()), 1e-30), name
    book = tr.grad("listener_vq.quantize.embedding.weight").double().cpu().numpy()
    assert np.abs(book[g["book_rows"]] - g["book_grad_rows"]).max() <= 1e-4 * np.abs(book).max()


@pytest.mark.parametrize("B,T", [(1, 5), (4, 300), (1, 1024)])
def test_vq_step_gradients_match_autograd(B, T):
    from dimx.train_hip import VqHipTrainer
    model = _model()
    tr = VqHipTrainer(model, dropout=0.0)
    x = _x(B, T)
    d, pred, idx = tr.forward_backward(x)
    (loss, rec, quant, ppl, a_pred, a_idx), grads = _autograd(model, x, idx=idx)
    own = _autograd(model, x)[0][5]
    assert (own.cpu() == idx.long().cpu()).float().mean().item() >= 0.99     # the checker's own argmin, up to near ties
    for key, ref in (("loss", loss), ("rec_loss", rec), ("quant_loss", quant), ("perplexity", ppl)):
        assert abs(d[key].item() - ref.item()) <= 1e-4 * abs(ref.item()), (key, d[key].item(), ref.item())
    assert (pred - a_pred.detach()).abs().max().item() <= 1e-3 * a_pred.abs().max().item()
    worst = _worst(tr, grads)
    print("VQ-VAE HIP step B=%d T=%d: worst relative gradient error vs autograd %.2e over %d tensors" % (B, T, worst, len(grads)))
    assert worst <= 1e-3


def test_vq_step_codes_equal_the_inference_encoder_and_reruns_are_bit_identical():
    from dimx.train_hip import VqHipTrainer
    model = _model()
    tr = VqHipTrainer(model, dropout=0.0)
    x = _x(4, 300, tag="vqtr.codes")
    d1, p1, i1 = tr.forward_backward(x)
    g1 = tr.grads.clone()
    with torch.no_grad():
        ref = model.engine(x.device).vq_encode(1, x, pe_mode=1).reshape(-1)
    assert torch.equal(i1.cpu(), ref.to(torch.int32).cpu())
    d2, p2, i2 = tr.forward_backward(x)
    assert torch.equal(g1, tr.grads) and torch.equal(p1, p2) and torch.equal(i1, i2)
    assert all(torch.equal(d1[k], d2[k]) for k in d1)


def test_vq_step_with_dropout_matches_autograd_over_the_mirrored_masks():
    from dimx import prng
    from dimx.train_hip import VqHipTrainer
    B, T, p = 4, 300, 0.1
    model = _model()
    tr = VqHipTrainer(model, dropout=p, seed=77)
    x = _x(B, T, tag="vqtr.drop")
    d, pred, idx = tr.forward_backward(x, step=5)
    masks = tuple(torch.from_numpy(prng.dropout_scale_mask(77, 5, s, (B, T, 384), p)).cuda() for s in (0, 1))
    (loss, *_), grads = _autograd(model, x, masks=masks, idx=idx)
    assert abs(d["loss"].item() - loss.item()) <= 1e-4 * abs(loss.item())
    worst = _worst(tr, grads)
    print("VQ-VAE HIP step with dropout %.1f: worst relative gradient error %.2e" % (p, worst))
    assert worst <= 1e-3
    g5 = tr.grads.clone()
    tr.forward_backward(x, step=6)
    assert not torch.equal(g5, tr.grads)


def test_vq_training_lowers_the_loss_and_matches_torch_adamw():
    from dimx import train as TR
    from dimx.train_hip import VqHipTrainer
    x = _x(2, 64, tag="vqtr.fit")
    model = _model()
    P = {k: v.detach().clone().requires_grad_(not k.endswith(".pe")) for k, v in model.state_dict().items()}
    tr = VqHipTrainer(model, lr=1e-4, dropout=0.0)
    losses = []
    for _ in range(5):
        tr.train_step(x)
        losses.append(tr.last["loss"].item())
    assert losses[-1] < losses[0], losses
    # two steps of the autograd checker + torch.optim.AdamW from the same start
    model2 = _model()
    tr2 = VqHipTrainer(model2, lr=1e-4, dropout=0.0)
    opt = torch.optim.AdamW([v for k, v in P.items() if not k.endswith(".pe")], lr=1e-4)
    for _ in range(2):
        d, _, idx = tr2.forward_backward(x)
        tr2.step()
        opt.zero_grad()
        with torch.enable_grad():
            TR.vq_loss(P, x, idx=idx)[0].backward()
        opt.step()
    diff = torch.cat([(tr2.view(tr2.params, tr2.prefix + k) - v.detach()).abs().reshape(-1) for k, v in P.items() if not k.endswith(".pe")])
    over = int((diff > 1e-5).sum())
    print("VQ-VAE: 2 AdamW steps, |HIP - torch| weight difference max %.2e, %d of %d elements above 1e-5"
          % (diff.max().item(), over, diff.numel()))
    # AdamW's first steps move every element by ~lr sign(g): where |g| is at the rounding level of the two gradient
    # computations its sign may differ, so a handful of elements may differ by up to 2 lr; all others agree within 1e-5
    assert over <= diff.numel() * 1e-5 and diff.max().item() <= 4 * 1e-4


def test_vq_step_bf16_agrees_with_f32_and_trains():
    from dimx import lib
    from dimx.train_hip import VqHipTrainer
    x = _x(4, 120, tag="vqtr.bf16")
    tf = VqHipTrainer(_model(), dropout=0.0)
    df, _, _ = tf.forward_backward(x)
    tb = VqHipTrainer(_model(lib.MODE_PERF_BF16), dropout=0.0)
    db, _, _ = tb.forward_backward(x)
    for k in ("loss", "rec_loss", "quant_loss"):
        assert abs(db[k].item() - df[k].item()) <= 0.02 * abs(df[k].item()), (k, db[k].item(), df[k].item())
    first = None
    for _ in range(5):
        tb.train_step(x)
        first = tb.last["loss"].item() if first is None else first
    assert tb.last["loss"].item() < first


def test_vq_checkpoint_hands_off_to_slmft(tmp_path):
    from dimx.seq2seq_pretrain import SLMFT
    from dimx.train_hip import VqHipTrainer
    x = _x(2, 48, tag="vqtr.handoff")
    model = _model()
    tr = VqHipTrainer(model, dropout=0.1)
    for _ in range(2):
        tr.train_step(x)
    _, _, idx = tr.forward_backward(x, dropout=0.0)
    tr.sync_to_model()
    path = tmp_path / "model.pth.tar"
    torch.save({"state_dict": model.state_dict()}, str(path))
    slm = SLMFT(vq_listener_ckpt=str(path)).cuda()
    for k, v in model.state_dict().items():
        assert torch.equal(slm.listener_vq.state_dict()[k].cpu(), v.cpu()), k
    _, got = slm.listener_vq.get_quant(x)
    assert torch.equal(got.reshape(-1).cpu(), idx.long().cpu())


def test_train_vq_driver_writes_a_loadable_checkpoint(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "examples", "train_vq.py"), "--epochs", "2", "--clips", "12", "--max-len", "48",
           "save_path", str(tmp_path), "batch_size", "4"]
    r = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    ck = tmp_path / "model" / "model.pth.tar"
    assert ck.exists(), r.stdout
    sd = torch.load(str(ck), map_location="cpu")["state_dict"]
    assert "quantize.embedding.weight" in sd and "encoder.vertice_mapping.0.weight" in sd
    assert "VAL Epoch: 2" in r.stdout
