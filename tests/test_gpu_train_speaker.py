"""GPU: the DIM-Speaker fine-tuning step on the HIP kernels (dimx.train_hip.SpeakerHipTrainer -> csrc/train.hip: spk_run,
csrc/train_spk.hip) against PyTorch autograd over ``dimx.train.speaker_loss`` on the same inputs -- reference loop
train_epoch_biwi (code/x_engine_pt.py:62-132), model code/seq2seq_pretrain.py:708-757.  f32 parity mode unless stated: both
losses <= 1e-4 relative, every trained tensor's gradient <= 1e-3 relative to its largest entry (the tolerances of
tests/test_gpu_train_slm.py).  mesh_dim = 120 (40 vertices) wherever the mouth metric is involved: nothing here depends on V."""
import importlib.util
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOUTH = [3, 3, 11, 39]
# (B, T, lens, ids): padding + a duplicated id | no ids | the shortest legal clip (one target per row), first and last table rows
CASES = [(3, 24, [24, 17, 9], [2, 2, 7]), (1, 12, [12], None), (2, 2, [2, 2], [14, 0])]
# the seed of the inputs: with it the checker's own top-two logit margin is above 3e-3 on every row of the three cases (checked
# on the CPU restatement), so the 1e-4 near-tie allowance below is a condition that never has to be used here
SEED = 6


def synthetic_biwi_loader(*a, **k):
    spec = importlib.util.spec_from_file_location("dimx_examples_test_biwi", os.path.join(ROOT, "examples", "test_biwi.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.synthetic_biwi_loader(*a, **k)


def _case(B, T, lens, ids, seed=SEED, V=120):
    from dimx import prng
    tag = "spk.%d.%d" % (B, T)
    xe = torch.from_numpy(prng.normal(seed, tag + ".e", (B, T, 56)))
    xa = torch.from_numpy(prng.normal(seed, tag + ".a", (B, T, 768)))
    xt = torch.from_numpy(prng.normal(seed, tag + ".t", (B, V))) * 0.1
    xv = xt[:, None, :] + 0.01 * torch.from_numpy(prng.normal(seed, tag + ".v", (B, T, V)))
    mask = torch.zeros(B, T, dtype=torch.bool)
    for j, n in enumerate(lens):
        mask[j, :n] = True
    return xv, xe, xa, mask, xt, (None if ids is None else torch.tensor(ids))


def _model(mode, mouth_map=MOUTH):
    from dimx import train as T
    from dimx.seq2seq_pretrain import SpeakerSLMFT
    m = SpeakerSLMFT(mesh_dim=120, mouth_map=mouth_map, numeric_mode=mode).cuda()
    T.set_speaker_trainable(m)
    m.train()
    return m


@pytest.fixture(scope="module")
def f32_model():
    """one f32 model for every test that leaves the module's parameters alone"""
    from dimx import lib
    return _model(lib.MODE_PARITY_F32)


def _gpu(case):
    dev = torch.device("cuda:0")
    return tuple(None if t is None else t.to(dev) for t in case)


def _checker(model, xe, xa, mask, z, ids, tokens):
    from dimx import train as Tr
    for p in model.parameters():
        p.grad = None
    P = dict(model.state_dict(keep_vars=True))
    with torch.enable_grad():
        total, o = Tr.speaker_loss(P, model.s2s, model.vq_dims, xe, xa, mask, z, P["speaker_vq.decoder.decoder_pos_embedding.pe"],
                                   speaker_ids=ids, tokens=tokens)
        total.backward()
    return total.detach(), o


@pytest.mark.parametrize("B,T,lens,ids", CASES)
def test_speaker_hip_gradients_match_autograd(f32_model, B, T, lens, ids):
    from dimx import train as Tr
    from dimx.train_hip import SpeakerHipTrainer
    model = f32_model
    xv, xe, xa, mask, xt, sid = _gpu(_case(B, T, lens, ids))
    with torch.no_grad():
        _, z = model.forward_vq(None, xe, mask)
    tr = SpeakerHipTrainer(model, mouth_map=None)
    total, d = tr.forward_backward(None, xe, xa, mask, None, speaker_ids=sid, z=z, return_logits=True)
    idx, logits = tr.last_out["idx"].view(B, T - 1).long(), tr.last_out["logits"]
    assert torch.equal(idx, torch.argmax(logits, dim=-1))          # first index on ties, like torch
    a_total, o = _checker(model, xe, xa, mask, z, sid, idx)
    # the checker's own arg-max may differ from the step's only at a near tie of ITS logits, and on at most 2 % of the rows
    top2 = o["logits"].detach().topk(2, dim=-1).values
    margin = top2[..., 0] - top2[..., 1]
    differ = o["logits"].detach().argmax(-1) != idx
    print("case B=%d T=%d: rows whose arg-max differs from the checker's %d of %d, smallest checker margin %.3e" % (
        B, T, int(differ.sum()), differ.numel(), float(margin.min())))
    assert bool((margin[differ] < 1e-4).all()) and int(differ.sum()) <= 0.02 * differ.numel()
    l_ce, l_emoca = float(d["l_ce_l"]), float(d["l_cont_l"])
    a_ce, a_emoca = float(o["l_ce"].detach()), float(o["l_emoca"].detach())
    print("  l_ce %.6f vs %.6f, l_emoca %.6f vs %.6f" % (l_ce, a_ce, l_emoca, a_emoca))
    assert abs(l_ce - a_ce) < 1e-4 * abs(a_ce)
    assert abs(l_emoca - a_emoca) < 1e-4 * abs(a_emoca)
    assert abs(float(total) - float(a_total)) < 1e-4 * abs(float(a_total))
    assert d["l_cont_s"] == 0 and d["l_ce_s"] == 0 and d["nce"] == 0 and d["c_acc"] == 0
    named = dict(model.named_parameters())
    trained = {n for n, _ in Tr.speaker_trainable_parameters(model)}
    assert {n for n, _, _ in tr.layout} == trained
    worst, worst_name, zero_worst = 0.0, "", 0.0
    for name in sorted(trained):
        g_h = tr.grad(name)
        g_a = named[name].grad
        if name == "speaker_embed.weight" and ids is None:
            assert g_a is None and float(g_h.abs().max()) == 0.0
            continue
        assert g_a is not None, name
        if float(g_a.abs().max()) == 0.0:
            # a gradient that is exactly zero in autograd has no largest entry to be relative to: with a single key (T = 2) the
            # self-attention's softmax is the constant 1, so d to_q = d to_k = 0 analytically; autograd's softmax adjoint
            # p (g - sum p g) returns the exact zero, a flash-style adjoint p (dP - delta) leaves the rounding of two separately
            # summed dot products.  The absolute bound is the one tests/test_gpu_train_slm.py uses for such tensors.
            zero_worst = max(zero_worst, float(g_h.abs().max()))
            assert float(g_h.abs().max()) < 1e-7, (name, float(g_h.abs().max()))
            continue
        rel = (g_h - g_a).abs().max().item() / max(g_a.abs().max().item(), 1e-8)
        if rel > worst:
            worst, worst_name = rel, name
        assert rel < 1e-3, (name, rel)
    print("  worst relative gradient error vs autograd %.2e (%s) over %d tensors; largest entry where autograd is exactly zero %.2e" % (
        worst, worst_name, len(trained), zero_worst))
    g_e = tr.grad("speaker_embed.weight")
    if ids is not None:
        absent = [r for r in range(g_e.shape[0]) if r not in ids]
        assert float(g_e[absent].abs().max()) == 0.0                  # exactly zero, not small
        assert all(float(g_e[r].abs().max()) > 0.0 for r in set(ids))
    assert float(tr.grad("patch_embed_dec_l").abs().max()) > 0.0
    g1 = tr.grads.clone()                                              # a second call gives the same bits
    tr.forward_backward(None, xe, xa, mask, None, speaker_ids=sid, z=z)
    assert torch.equal(g1, tr.grads)


def test_speaker_step_outputs_decode_and_mse(f32_model):
    """the context / arg-max / MSE kernels through the step's own outputs: pred_out is the engine's decode of idx_out, and
    loss_out[2] is the mean squared error of pred_out against the EMOCA stream read one frame ahead"""
    from dimx.train_hip import SpeakerHipTrainer
    model = f32_model
    B, T, lens, ids = CASES[0]
    xv, xe, xa, mask, xt, sid = _gpu(_case(B, T, lens, ids))
    tr = SpeakerHipTrainer(model, mouth_map=None)
    total, d = tr.forward_backward(None, xe, xa, mask, None, speaker_ids=sid)
    idx, pred = tr.last_out["idx"].view(B, T - 1).long(), tr.last_out["pred"]
    with torch.no_grad():
        ref = model.engine(xe.device).vq_decode(0, idx, 0)
    err = (pred - ref).abs().max().item()
    want = F.mse_loss(pred, xe[:, 1:, :]).item()
    print("pred_out vs vq_decode(idx_out): %.2e; l_emoca %.7f vs mse_loss %.7f" % (err, float(d["l_cont_l"]), want))
    assert err < 1e-5
    assert abs(float(d["l_cont_l"]) - want) < 1e-6 * want
    inv = 1.0 / (B * (T - 1) * 56)
    assert abs(float(tr._loss[3]) - inv) < 1e-6 * inv                 # an f32 holds it to 6e-8 relative
    from dimx import lib as L
    with pytest.raises(L.DimxError):                                   # an id outside the table is refused on the host
        tr.forward_backward(None, xe, xa, mask, None, speaker_ids=torch.tensor([2, 15, 7]))
    with pytest.raises(L.DimxError):
        tr.forward_backward(None, xe, xa, mask, None, speaker_ids=torch.tensor([-1, 2, 7]))


def test_speaker_hip_training_reduces_the_loss_and_trains_the_right_tensors():
    from dimx import lib
    from dimx.train_hip import SpeakerHipTrainer
    model = _model(lib.MODE_PARITY_F32, mouth_map=None)
    B, T, ids = 2, 32, [2, 7]
    xv, xe, xa, mask, xt, sid = _gpu(_case(B, T, [T, T], ids))
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    tr = SpeakerHipTrainer(model, lr=1e-4)
    l0, _ = tr.train_step(None, xe, xa, mask, None, speaker_ids=sid)
    for _ in range(4):
        l1, _ = tr.train_step(None, xe, xa, mask, None, speaker_ids=sid)
    print("DIM-Speaker step, five steps at lr 1e-4: total %.5f -> %.5f" % (l0.item(), l1.item()))
    assert l1.item() < l0.item(), (l0.item(), l1.item())
    last_total, last_d = tr.forward_backward(None, xe, xa, mask, None, speaker_ids=sid)
    tr.sync_to_model()
    after = model.state_dict()
    for k in before:
        changed = not torch.equal(before[k], after[k])
        if k.startswith(("listener_vq.", "speaker_vq.encoder.", "speaker_vq.quantize.", "vertice_map_reverse", "encoder_", "norm")) or k == "W":
            assert not changed, k
        elif k.startswith(("decoder_joint.net.attn_layers.", "speaker_vq.decoder.")) and not k.endswith(".pe"):
            assert changed, k
    assert not torch.equal(before["patch_embed_dec_l"], after["patch_embed_dec_l"])
    e0, e1 = before["speaker_embed.weight"], after["speaker_embed.weight"]
    assert all(not torch.equal(e0[r], e1[r]) for r in range(e0.shape[0]))
    absent = [r for r in range(e0.shape[0]) if r not in ids]
    decay = (1.0 - 1e-4 * 1e-2) ** 5                                   # zero gradient: AdamW's decoupled weight decay alone
    # five f32 products p (1 - lr wd), each rounded to half an ulp of its result: 5 x 2^-24 relative, doubled for the f32 rounding
    # of the factor itself
    bound = 5 * 2.0 ** -23 * e0.abs().max().item()
    err = (e1[absent] - e0[absent] * decay).abs().max().item()
    print("  unreferenced embedding rows vs weight decay alone: %.2e (bound %.2e; the decay itself moves them by %.2e)" % (
        err, bound, (e0[absent] * (1 - decay)).abs().max().item()))
    assert err < bound
    assert (e1[ids] - e0[ids] * decay).abs().max().item() > 1e-5
    with torch.no_grad():
        _, d_m, _ = model(None, xe, xa, mask, None, mode="train", speaker_ids=sid)
    print("  l_ce after sync: module %.6f, trainer %.6f" % (float(d_m["l_ce_l"]), float(last_d["l_ce_l"])))
    assert abs(float(d_m["l_ce_l"]) - float(last_d["l_ce_l"])) < 1e-4 * max(1.0, abs(float(last_d["l_ce_l"])))


def test_speaker_clip_and_adamw_match_torch(f32_model):
    from dimx.train_hip import SpeakerHipTrainer
    B, T, lens, ids = CASES[0]
    xv, xe, xa, mask, xt, sid = _gpu(_case(B, T, lens, ids))
    tr = SpeakerHipTrainer(f32_model, lr=1e-5, clip=1.0, mouth_map=None)
    tr.forward_backward(None, xe, xa, mask, None, speaker_ids=sid)
    tr.grads.mul_(3.0 / tr.grads.double().norm().item())              # a norm of 3: the clip has to act
    g, p0 = tr.grads.clone(), tr.params.clone()
    norm = tr.step()
    want = g.double().norm().item()
    print("clip: reported norm %.7f, torch %.7f" % (float(norm), want))
    assert want > 1.0 and abs(float(norm) - want) < 1e-5 * want
    p = torch.nn.Parameter(p0.clone())
    p.grad = g.clone()
    opt = torch.optim.AdamW([p], lr=1e-5)
    torch.nn.utils.clip_grad_norm_([p], 1.0)
    opt.step()
    err = (tr.params - p.detach()).abs().max().item()
    print("  update vs torch.optim.AdamW after clip_grad_norm_: %.2e" % err)
    assert err < 1e-6 and not torch.equal(tr.params, p0)


def test_speaker_bf16_step_agrees_with_f32(f32_model):
    """bf16 operands: the losses within 2 %, the gradient of everything in front of the arg-max within 8 % in norm (the bound of
    the SLM step's test).  The C-ABI takes no tokens, so a bf16 arg-max that flips a code cannot be aligned with the f32 step's:
    the VQ decoder's gradient is left out of the norm comparison."""
    from dimx import lib
    from dimx.train_hip import SpeakerHipTrainer
    B, T, lens, ids = CASES[0]
    xv, xe, xa, mask, xt, sid = _gpu(_case(B, T, lens, ids))
    with torch.no_grad():
        _, z = f32_model.forward_vq(None, xe, mask)
    ga = SpeakerHipTrainer(f32_model, mouth_map=None)
    gb = SpeakerHipTrainer(_model(lib.MODE_PERF_BF16, mouth_map=None))
    la, da = ga.forward_backward(None, xe, xa, mask, None, speaker_ids=sid, z=z)
    lb, db = gb.forward_backward(None, xe, xa, mask, None, speaker_ids=sid, z=z)
    dev = xe.device
    pre = torch.cat([torch.arange(off, off + numel) for name, off, numel in ga.layout if "_vq." not in name]).to(dev)
    rel = ((gb.grads[pre] - ga.grads[pre]).norm() / ga.grads[pre].norm()).item()
    flips = int((ga.last_out["idx"] != gb.last_out["idx"]).sum())
    print("DIM-Speaker bf16 step: l_ce %.5f vs f32 %.5f, l_emoca %.5f vs %.5f, %d flipped codes, relative gradient difference %.3f" % (
        float(db["l_ce_l"]), float(da["l_ce_l"]), float(db["l_cont_l"]), float(da["l_cont_l"]), flips, rel))
    assert abs(float(db["l_ce_l"]) - float(da["l_ce_l"])) < 0.02 * abs(float(da["l_ce_l"]))
    assert abs(float(db["l_cont_l"]) - float(da["l_cont_l"])) < 0.02 * abs(float(da["l_cont_l"]))
    assert rel < 0.08


def test_speaker_mouth_metric_is_the_modules(f32_model, monkeypatch):
    from dimx.train_hip import SpeakerHipTrainer
    model = f32_model
    B, T, lens, ids = CASES[0]
    xv, xe, xa, mask, xt, sid = _gpu(_case(B, T, lens, ids))
    tr = SpeakerHipTrainer(model)
    assert tr.mouth_map == MOUTH
    total, d = tr.forward_backward(xv, xe, xa, mask, xt, speaker_ids=sid)
    with torch.no_grad():
        m_total, m_d, _ = model(xv, xe, xa, mask, xt, mode="train", speaker_ids=sid)
    print("mouth term: trainer %.7f, module %.7f" % (float(d["l_cont_s"]), float(m_d["l_cont_s"])))
    assert float(m_d["l_cont_s"]) > 0.0 and abs(float(d["l_cont_s"]) - float(m_d["l_cont_s"])) < 1e-5
    assert abs(float(total) - float(m_total)) < 1e-4 * abs(float(m_total))     # the mouth term adds nothing to the total
    eng = model.engine(xe.device)

    def boom(*a, **k):
        raise AssertionError("the mesh head was launched without a mouth map")
    monkeypatch.setattr(eng, "mesh_head", boom)
    tr0 = SpeakerHipTrainer(model, mouth_map=None)
    total0, d0 = tr0.forward_backward(xv, xe, xa, mask, xt, speaker_ids=sid)
    assert d0["l_cont_s"] == 0 and float(total0) == float(total)


def test_train_epoch_biwi_runs_on_the_hip_step():
    from dimx import lib, x_engine_pt
    from dimx import train as Tr
    from dimx.seq2seq_pretrain import EmocaConverter
    from dimx.train_hip import SpeakerHipTrainer
    dev = torch.device("cuda:0")
    loader = synthetic_biwi_loader(2, 16, 120)
    m = _model(lib.MODE_PARITY_F32)
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    tr = SpeakerHipTrainer(m, lr=1e-4)
    logs = []
    loss = x_engine_pt.train_epoch_biwi(m, loader, tr, dev, clip=1.0, print_freq=1, log=logs.append)
    assert loss == loss and tr.step_count == 2 and tr.clip == 1.0 and len(logs) == 2
    assert logs[1].startswith("Epoch 0 Batch 1:\tLoss ")
    assert [w.split(" ")[0] for w in logs[1].split("\t")[1:]] == ["Loss", "CE_s", "CE_l", "Cont_s", "Cont_l", "NCE", "C_acc"]
    after = m.state_dict()
    assert not torch.equal(before["decoder_joint.net.to_logits.weight"], after["decoder_joint.net.to_logits.weight"])
    assert torch.equal(before["vertice_map_reverse.0.weight"], after["vertice_map_reverse.0.weight"])
    # the reference's own call: a torch AdamW over the trained tensors, a SpeakerHipTrainer stands in for it
    opt = torch.optim.AdamW([p for _, p in Tr.speaker_trainable_parameters(m)], lr=1e-5)
    x_engine_pt.train_epoch_biwi(m, loader, opt, dev, clip=1.0, log=logs.append)
    assert isinstance(m._dimx_hip_trainer[1], SpeakerHipTrainer) and m._dimx_hip_trainer[1].step_count == 2
    assert float(opt.state[dict(m.named_parameters())["speaker_embed.weight"]]["step"]) == 2.0
    # a model of this package without a HIP fine-tuning step: backward='auto' raises instead of changing backend
    conv = EmocaConverter(mesh_dim=120).cuda()
    opt_c = torch.optim.AdamW(conv.dimx_trainable_parameters(), lr=1e-5)
    with pytest.raises(lib.DimxError):
        x_engine_pt.train_epoch_biwi(conv, loader, opt_c, dev, clip=1.0, log=logs.append)
