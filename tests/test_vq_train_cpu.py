"""CPU: the VQ-VAE training step's checker and contract (stage 1, reference code/train_vq.py:173-196).
  * dimx.train.vq_loss (encoder, straight-through quantiser, decoder, calc_vq_loss; PyTorch autograd) against one step of the
    reference VQAutoEncoder in eval() (tests/golden/vq_train_B2_T27.npz, make_golden_vq_train.py): codes, loss terms, every
    gradient tensor's norm and sampled entries;
  * the counter-based dropout keep-mask (dimx.prng.dropout_keep) that the HIP step and the checker share;
  * VqHipTrainer refuses a CPU module; the new C-ABI names are declared."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20260928


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "vq_train_B2_T27.npz"))


def _sd():
    import dimx  # noqa: F401
    from dimx import weights
    return weights.synth_state_dict(weights.vq_spec(prefix="listener_vq."), SEED, strip_prefix="listener_vq.")


def _positions(name, numel):
    from dimx import prng
    return prng.integers(SEED, "vq_train.sample." + name, (128,), 0, numel)


def test_vq_loss_matches_the_reference_step(golden):
    from dimx import prng
    from dimx import train as TR
    x = torch.from_numpy(prng.normal(SEED, "vq_train.x", (2, 27, 56)))
    with torch.enable_grad():
        P = {k: v.clone().requires_grad_(not k.endswith(".pe")) for k, v in _sd().items()}
        loss, rec, quant, ppl, pred, idx = TR.vq_loss(P, x)
        loss.backward()
    assert np.array_equal(idx.numpy(), golden["idx"])
    for got, key in ((loss, "loss"), (rec, "rec_loss"), (quant, "quant_loss"), (ppl, "perplexity")):
        want = float(golden[key])
        got = float(got.detach())
        assert abs(got - want) <= 1e-5 * abs(want), (key, got, want)
    assert np.abs(pred.detach().numpy() - golden["pred"]).max() <= 1e-4 * np.abs(golden["pred"]).max()
    names = [str(n) for n in golden["names"]]
    assert len(names) == 148 and set(names) == {k for k in P if not k.endswith(".pe")}
    for i, name in enumerate(names):
        g = P[name].grad.detach().double().reshape(-1)
        gmax = float(g.abs().max())
        assert gmax > 0, name
        assert abs(float(g.norm()) - golden["grad_norm"][i]) <= 1e-4 * max(golden["grad_norm"][i], gmax), name
        samp = g[torch.from_numpy(_positions(name, g.numel()))].numpy()
        assert np.abs(samp - golden["grad_samples"][i]).max() <= 1e-4 * gmax, name
    book = P["quantize.embedding.weight"].grad.detach().double().numpy()
    rows = golden["book_rows"]
    assert np.abs(book[rows] - golden["book_grad_rows"]).max() <= 1e-4 * np.abs(book).max()
    untouched = np.setdiff1d(np.arange(512), rows)
    assert not book[untouched].any()          # no other term reaches the codebook


def test_dropout_mask_is_deterministic_and_keyed():
    from dimx import prng
    shape = (2, 27, 384)
    a = prng.dropout_keep(7, 3, prng.DROPOUT_SITE_ENCODER, shape, 0.1)
    assert np.array_equal(a, prng.dropout_keep(7, 3, prng.DROPOUT_SITE_ENCODER, shape, 0.1))
    assert not np.array_equal(a, prng.dropout_keep(7, 4, prng.DROPOUT_SITE_ENCODER, shape, 0.1))
    assert not np.array_equal(a, prng.dropout_keep(7, 3, prng.DROPOUT_SITE_DECODER, shape, 0.1))
    assert not np.array_equal(a, prng.dropout_keep(8, 3, prng.DROPOUT_SITE_ENCODER, shape, 0.1))
    # any element regenerates alone: a clip's mask does not depend on the batch / clip length around it
    b = prng.dropout_keep(7, 3, prng.DROPOUT_SITE_ENCODER, (3, 40, 384), 0.1)
    assert np.array_equal(a, b[:2, :27])
    assert prng.dropout_keep(7, 3, 0, shape, 0.0).all()
    m = prng.dropout_scale_mask(7, 3, 0, shape, 0.1)
    assert set(np.unique(m).tolist()) == {0.0, float(np.float32(1) / np.float32(0.9))}


def test_dropout_mask_keeps_the_expected_fraction():
    from dimx import prng
    keep = prng.dropout_keep(20260928, 0, prng.DROPOUT_SITE_DECODER, (10, 1000, 100), 0.1)
    assert keep.size == 10 ** 6
    assert abs(keep.mean() - 0.9) <= 0.005


def test_vq_loss_dropout_masks_change_the_step():
    from dimx import prng
    from dimx import train as TR
    x = torch.from_numpy(prng.normal(SEED, "vq_train.x", (1, 9, 56)))
    P = _sd()
    shape = (1, 9, 384)
    masks = tuple(torch.from_numpy(prng.dropout_scale_mask(1, 0, s, shape, 0.1)) for s in (0, 1))
    ones = tuple(torch.ones(shape) for _ in range(2))
    base = TR.vq_loss(P, x)[0]
    assert torch.equal(TR.vq_loss(P, x, masks=ones)[0], base)
    assert not torch.equal(TR.vq_loss(P, x, masks=masks)[0], base)


def test_vq_trainer_refuses_a_cpu_module():
    from dimx import lib
    from dimx.config import load_cfg_from_cfg_file
    from dimx.models import VQAutoEncoder
    from dimx.train_hip import VqHipTrainer
    cfg = load_cfg_from_cfg_file(os.path.join(ROOT, "dyadic-interaction-modeling_amd", "config.yaml"))
    with pytest.raises(lib.DimxError):
        VqHipTrainer(VQAutoEncoder(cfg))


def test_vq_training_abi_is_declared():
    from dimx import lib
    hdr = open(os.path.join(ROOT, "include", "dimx.h")).read()
    for name in ("dimx_train_vq_num_params", "dimx_train_vq_total", "dimx_train_vq_param_info", "dimx_train_vq_workspace_bytes",
                 "dimx_train_vq_forward_backward"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in lib.SIGNATURES, name
