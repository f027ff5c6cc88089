"""Generate tests/golden/vq_train_B2_T27.npz: one training step of the REFERENCE VQ-VAE (stage 1, code/train_vq.py:173-196)
at B=2, T=27 -- VQAutoEncoder.forward, calc_vq_loss (quant_loss_weight 1.0) and loss.backward() -- with the reference module
in eval() (only the PositionalEncoding dropout changes: InstanceNorm has no running statistics).  Weights and input are
regenerated from dimx.prng on both sides (seed below), so only the results are stored:
  * loss, rec_loss, quant_loss, perplexity, idx [B*T], pred [B,T,56];
  * per parameter (state-dict order, the pe buffers excluded): the gradient's L2 norm and sum, and 128 entries at flat
    positions regenerated from dimx.prng (stream "vq_train.sample.<name>");
  * the codebook gradient's rows that the step touched (the distinct idx values).

Run:  python tests/golden/make_golden_vq_train.py
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import numpy as np
import torch

import dimx  # noqa: E402,F401
from dimx import prng  # noqa: E402

SEED = 20260928
B, T = 2, 27
OUT = os.path.join(HERE, "vq_train_B%d_T%d.npz" % (B, T))


def sample_positions(name, numel, k=128):
    return prng.integers(SEED, "vq_train.sample." + name, (k,), 0, numel)


def input_clip():
    return prng.normal(SEED, "vq_train.x", (B, T, 56))


def main():
    import make_golden
    cwd = os.getcwd()
    _, models, _ = make_golden.load_reference()
    os.chdir(os.path.join(make_golden.REF))
    try:
        from metrics.loss import calc_vq_loss
    finally:
        os.chdir(cwd)
    m = models["listener_vq."].eval()
    for p in m.parameters():
        p.requires_grad_(True)
        p.grad = None
    x = torch.from_numpy(input_clip())
    with torch.enable_grad():
        pred, quant_loss, info = m(x)
        loss, (rec, quant) = calc_vq_loss(pred, x, quant_loss, quant_loss_weight=1.0)
        loss.backward()
    names, norms, sums, samples = [], [], [], []
    for name, p in m.named_parameters():
        g = p.grad
        assert g is not None, name
        g = g.detach().double().reshape(-1)
        names.append(name)
        norms.append(float(g.norm()))
        sums.append(float(g.sum()))
        samples.append(g[torch.from_numpy(sample_positions(name, g.numel()))].numpy())
    idx = info[2].reshape(-1).numpy().astype(np.int32)
    rows = np.unique(idx)
    book_grad = m.quantize.embedding.weight.grad.detach().numpy()[rows]
    np.savez_compressed(
        OUT, loss=np.float64(loss.item()), rec_loss=np.float64(rec.item()), quant_loss=np.float64(quant.item()),
        perplexity=np.float64(info[0].item()), idx=idx, pred=pred.detach().numpy().astype(np.float32),
        names=np.array(names), grad_norm=np.array(norms), grad_sum=np.array(sums),
        grad_samples=np.stack(samples).astype(np.float64), book_rows=rows.astype(np.int32),
        book_grad_rows=book_grad.astype(np.float64))
    print("wrote %s (%d bytes, %d tensors, %d codes used)" % (OUT, os.path.getsize(OUT), len(names), len(rows)))


if __name__ == "__main__":
    main()
