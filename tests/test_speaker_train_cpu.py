"""CPU: the host side of the DIM-Speaker fine-tuning step (reference train_epoch_biwi, code/x_engine_pt.py:62-132, over
SpeakerSLMFT.forward(mode='train'), code/seq2seq_pretrain.py:708-757): the C-ABI surface, which tensors the PyTorch-autograd
checker ``dimx.train.speaker_loss`` differentiates, its ``tokens=`` injection, the summation order of the embedding adjoint,
and the loop on the checker.  The HIP step itself is tests/test_gpu_train_speaker.py."""
import importlib.util
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dimx_train_spk_num_params", "dimx_train_spk_total", "dimx_train_spk_param_info", "dimx_train_spk_workspace_bytes",
               "dimx_train_spk_forward_backward")


def synthetic_biwi_loader(*a, **k):
    spec = importlib.util.spec_from_file_location("dimx_examples_test_biwi", os.path.join(ROOT, "examples", "test_biwi.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.synthetic_biwi_loader(*a, **k)


@pytest.fixture(scope="module")
def model():
    import dimx  # noqa: F401
    from dimx.seq2seq_pretrain import SpeakerSLMFT
    return SpeakerSLMFT(mesh_dim=120, mouth_map=[3, 3, 11, 39])


def _case(B, T, seed=5):
    from dimx import prng
    xe = torch.from_numpy(prng.normal(seed, "spk.cpu.e", (B, T, 56)))
    xa = torch.from_numpy(prng.normal(seed, "spk.cpu.a", (B, T, 768)))
    return xe, xa, torch.ones(B, T, dtype=torch.bool)


def _loss(model, xe, xa, mask, ids, tokens=None):
    from dimx import train as T
    from dimx import x_engine_pt
    P = dict(model.state_dict(keep_vars=True))
    with torch.no_grad():
        z = x_engine_pt._speaker_codes(model, P, xe, mask)
    return T.speaker_loss(P, model.s2s, model.vq_dims, xe, xa, mask, z, P["speaker_vq.decoder.decoder_pos_embedding.pe"],
                          speaker_ids=ids, tokens=tokens)


def test_library_exports_the_speaker_training_entry_points():
    import ctypes
    import dimx  # noqa: F401
    from dimx import lib as L
    so = ctypes.CDLL(L.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "dimx.h")).read()
    for name in NEW_SYMBOLS:
        assert name in L.SIGNATURES, name
        assert hasattr(so, name), name
        assert name + "(" in header, name
    assert len(L.SIGNATURES["dimx_train_spk_forward_backward"][1]) == 19


def test_speaker_trainable_parameters_are_what_the_loss_differentiates(model):
    from dimx import train as T
    names = [n for n, _ in T.speaker_trainable_parameters(model)]
    assert names == [n for n, _ in model.dimx_trainable_parameters()]
    every = [n for n, _ in model.named_parameters()]
    expect = [n for n in every if n.startswith("decoder_joint.") or n.startswith("speaker_vq.decoder.")
              or n in ("patch_embed_dec_l", "speaker_embed.weight")]
    assert names == expect and "patch_embed_dec_l" in names and "speaker_embed.weight" in names
    assert not any(n.startswith(("listener_vq.", "speaker_vq.encoder.", "speaker_vq.quantize.", "vertice_map", "encoder_", "norm"))
                   for n in names)
    for p in model.parameters():
        p.requires_grad_(True)
        p.grad = None
    xe, xa, mask = _case(2, 6)
    with torch.enable_grad():
        total, o = _loss(model, xe, xa, mask, torch.tensor([2, 7]))
        total.backward()
    trained = set(names)
    for n, p in model.named_parameters():
        if n in trained:
            assert p.grad is not None and float(p.grad.abs().max()) > 0.0, n
        else:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, n
    g = dict(model.named_parameters())["speaker_embed.weight"].grad
    used = torch.zeros(g.shape[0], dtype=torch.bool)
    used[[2, 7]] = True
    assert float(g[~used].abs().max()) == 0.0 and bool((g[used].abs().amax(dim=1) > 0).all())
    for p in model.parameters():
        p.grad = None


def test_speaker_loss_with_its_own_argmax_as_tokens_is_the_same_value(model):
    xe, xa, mask = _case(2, 6)
    with torch.no_grad():
        a, oa = _loss(model, xe, xa, mask, torch.tensor([0, 14]))
        b, ob = _loss(model, xe, xa, mask, torch.tensor([0, 14]), tokens=oa["tokens"])
        c, oc = _loss(model, xe, xa, mask, torch.tensor([0, 14]), tokens=(oa["tokens"] + 1) % 512)
    assert torch.equal(oa["tokens"], oa["logits"].argmax(-1))
    assert float(a) == float(b) and torch.equal(oa["pred"], ob["pred"])
    assert float(oc["l_ce"]) == float(oa["l_ce"]) and float(oc["l_emoca"]) != float(oa["l_emoca"])


@pytest.mark.parametrize("ids,T", [([2, 2, 7], 24), ([2, 2, 7], 5), (None, 9)])
def test_embedding_adjoint_in_the_kernel_order_equals_float64_autograd(ids, T):
    import dimx  # noqa: F401
    from dimx import prng
    from dimx import train as Tr
    B, C, rows = 3, 384, 15
    dctx = torch.from_numpy(prng.normal(3, "spk.cpu.dctx", (B, T, C))).double()
    embed = torch.zeros(rows, C, dtype=torch.float64, requires_grad=True)
    patch = torch.zeros(C, dtype=torch.float64, requires_grad=True)
    with torch.enable_grad():
        x = patch.expand(B, T, C)
        if ids is not None:
            x = x + embed[torch.tensor(ids)][:, None, :]
        (x * dctx).sum().backward()
    d_patch, d_embed = Tr.speaker_context_adjoint(dctx, ids, rows)
    assert torch.allclose(d_patch, patch.grad, rtol=1e-12, atol=1e-12)
    if ids is None:
        assert embed.grad is None and float(d_embed.abs().max()) == 0.0
        return
    assert torch.allclose(d_embed, embed.grad, rtol=1e-12, atol=1e-12)
    assert torch.allclose(d_embed[2], dctx[0].sum(0) + dctx[1].sum(0), rtol=1e-12, atol=1e-12)   # the duplicated id adds both clips
    assert float(d_embed[[r for r in range(rows) if r not in (2, 7)]].abs().max()) == 0.0
    # f32, as the kernel runs it: the fixed order stays within rounding of the float64 sum
    p32, e32 = Tr.speaker_context_adjoint(dctx.float(), ids, rows)
    assert (e32.double() - embed.grad).abs().max() < 1e-5 * embed.grad.abs().max()


def test_train_epoch_biwi_on_the_autograd_checker_trains_what_it_should(model):
    """runs on the CPU: the checker's listener codes come from the torch restatement of the frozen encoder there"""
    from dimx import train as T
    from dimx import x_engine_pt
    loader = synthetic_biwi_loader(2, 8, 120)
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    opt = torch.optim.AdamW([p for _, p in T.speaker_trainable_parameters(model)], lr=1e-3)
    logs = []
    loss = x_engine_pt.train_epoch_biwi(model, loader, opt, torch.device("cpu"), clip=1.0, print_freq=1, log=logs.append,
                                        backward="autograd")
    assert loss == loss and len(logs) == 2
    assert logs[0].startswith("Epoch 0 Batch 0:\tLoss ") and all(k in logs[0] for k in ("CE_s", "CE_l", "Cont_s", "Cont_l", "NCE", "C_acc"))
    after = model.state_dict()
    trained = {n for n, _ in T.speaker_trainable_parameters(model)}
    for k in before:
        changed = not torch.equal(before[k], after[k])
        if k not in trained:
            assert not changed, k
        elif k.startswith(("speaker_vq.decoder.decoder_transformer", "decoder_joint.net.attn_layers")):
            assert changed, k
    with pytest.raises(ValueError):
        x_engine_pt.train_epoch_biwi(model, loader, opt, torch.device("cpu"), backward="torch")
    model.load_state_dict(before)
    for p in model.parameters():
        p.grad = None
