"""GPU: the DIM-Speaker converter's training step on the HIP kernels (dimx.train_hip.ConverterHipTrainer -> csrc/train.hip
conv_run, csrc/lstm.hip with its save switch, csrc/train_lstm.hip) against the float64 CPU yardstick of tests/converter_ref.py
(stock torch.nn.LSTM / F.linear / autograd).  Every case runs on the default path and with flags bit 0 (everything on the
no-communication path) unless stated.  Tolerances: gradients 1e-4 * max|ref| per tensor (tests/test_gpu_train_vq.py:73-75),
losses 1e-5 relative; the yardstick's own f32-vs-f64 noise must lie 10x below the gradient tolerance
(tests/test_gpu_speaker.py:60).

Every test runs under a time limit of its own (the process is ended with a traceback if a test exceeds it)."""
import faulthandler
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4
MESH = 150
MOUTH = [0, 3, 7, 7, 21, 49]          # vertex 7 twice
FAULTS = []                           # fault counts seen by the tests of this file, checked by the last one
TEST_SECONDS = 900


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(TEST_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _rel(got, ref):
    return (got.detach().double().cpu() - ref.double()).abs().max().item() / max(ref.abs().max().item(), 1e-300)


def _check_layer(m, x, dy, tag, names=("dx", "dw_ih", "dw_hh", "db")):
    """dimx_op_lstm_layer_bwd on both paths against float64 autograd; returns the float64 reference"""
    import converter_ref
    from dimx import engine as E
    ref64 = converter_ref.layer_grads(m, x, dy, torch.float64)
    ref32 = converter_ref.layer_grads(m, x, dy, torch.float32)
    flat = lambda r: {"dx": [r[1]], "dw_ih": list(r[2]), "dw_hh": list(r[3]), "db": list(r[4])}
    f64, f32 = flat(ref64), flat(ref32)
    noise = max(_rel(a, b) for k in names for a, b in zip(f32[k], f64[k]))
    w_ih, w_hh, b_ih, b_hh = converter_ref.pairs(m.state_dict())
    for safe in (False, True):
        dx, dw_ih, dw_hh, db, faults = E.op_lstm_layer_bwd(x.cuda(), w_ih, w_hh, b_ih, b_hh, dy.cuda(), safe=safe, return_faults=True)
        FAULTS.append(faults)
        got = {"dx": [dx], "dw_ih": list(dw_ih), "dw_hh": list(dw_hh), "db": list(db)}
        errs = {k: max(_rel(a, b) for a, b in zip(got[k], f64[k])) for k in names}
        print("%s %s path: %s (tolerance %.0e, torch f32 vs f64 %.1e)"
              % (tag, "safe" if safe else "default", " ".join("%s %.2e" % kv for kv in errs.items()), TOL, noise))
        for k, e in errs.items():
            assert e <= TOL, "%s: %s differs from float64 autograd by %g of its maximum" % (tag, k, e)
    assert noise * 10 <= TOL, "torch's own f32 noise %g is not 10x below the tolerance" % noise
    return ref64


@pytest.mark.parametrize("T", [1, 2, 27, 300])
@pytest.mark.parametrize("B", [1, 3, 17])
@pytest.mark.parametrize("In", [56, 768])
def test_layer_adjoint_matches_float64_autograd(In, B, T):
    import converter_ref
    m = converter_ref.lstm_module(In, seed=1000 + In + 31 * B + T)
    g = torch.Generator().manual_seed(B * 1000 + T)
    x = torch.randn(B, T, In, generator=g)
    dy = torch.randn(B, T, 768, generator=g)
    _check_layer(m, x, dy, "lstm adjoint In=%d B=%d T=%d" % (In, B, T))


def _recurrent_share(m, x, y64):
    """max|y - y(W_hh = 0)| of the float64 reference: how much of the layer's output the recurrence carries"""
    import converter_ref
    m0 = converter_ref.lstm_module(m.input_size)
    m0.load_state_dict({k: torch.zeros_like(v) if k.startswith("weight_hh") else v for k, v in m.state_dict().items()})
    return (y64 - converter_ref.layer_grads(m0, x, torch.zeros(x.shape[0], x.shape[1], 768), torch.float64)[0]).abs().max().item()


# B = 4, 8, 16: whole 4-clip blocks; 5, 9: a one-clip tail block.  B = 130: the training forward's save rows of the group
# kernel's second launch (clips 128, 129), and 33 adjoint blocks per direction, the last with 2 clips
BOUNDARY_CASES = [(B, T, 56) for B in (4, 5, 8, 9, 16) for T in (2, 7)] + [(130, 3, 56), (130, 2, 768)]


@pytest.mark.parametrize("B,T,In", BOUNDARY_CASES)
def test_layer_adjoint_at_block_and_launch_boundaries(B, T, In):
    """independent random clips and dy: dx is per clip, so a save row or a dgates row taken from another clip shows there.  On the
    reference alone: the recurrence carries at least 100x the forward tolerance of 1e-4 (tests/test_gpu_lstm.py); that torch's
    f32 noise lies 10x below the gradient tolerance is asserted by _check_layer."""
    import converter_ref
    m = converter_ref.lstm_module(In, seed=2000 + In + 31 * B + T)
    g = torch.Generator().manual_seed(B * 1000 + T + 7)
    x = torch.randn(B, T, In, generator=g)
    dy = torch.randn(B, T, 768, generator=g)
    ref64 = _check_layer(m, x, dy, "lstm adjoint boundaries In=%d B=%d T=%d" % (In, B, T))
    share = _recurrent_share(m, x, ref64[0])
    print("recurrent share of the forward: %.2e" % share)
    assert share >= 100 * 1e-4, "the case does not exercise the recurrence (share %g)" % share


def _recurrence_case(B, direction):
    import converter_ref
    T, In = 27, 56
    m = converter_ref.lstm_module(In, seed=77, hh_scale=4.0)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, T, In, generator=g)
    dy = torch.zeros(B, T, 768)
    if direction == "forward":
        dy[:, T - 1, :384] = torch.randn(B, 384, generator=g)
        far = 0
    else:
        dy[:, 0, 384:] = torch.randn(B, 384, generator=g)
        far = T - 1
    dx = converter_ref.layer_grads(m, x, dy, torch.float64)[1]
    ratio = dx[:, far].abs().max().item() / dx.abs().max().item()
    print("far-end share of max|dx|: %.3f" % ratio)
    assert ratio >= 0.1, "the case does not exercise the recurrence (far-end ratio %g)" % ratio
    _check_layer(m, x, dy, "recurrence case B=%d (%s)" % (B, direction), names=("dx", "dw_hh"))


@pytest.mark.parametrize("direction", ["forward", "reverse"])
def test_layer_adjoint_carries_a_gradient_through_the_recurrence(direction):
    """At the synthetic weight scale a gradient injected at one end has faded below the tolerance after 27 steps, so the case
    above cannot see a wrong W_hh^T term.  weight_hh x 4, T = 27, dy non-zero only at the last frame of the direction's walk:
    the far end of dx then holds a large share of the maximum (precondition, asserted on the reference), and dx / dW_hh are held
    to the same tolerance."""
    _recurrence_case(3, direction)


@pytest.mark.parametrize("direction", ["forward", "reverse"])
def test_layer_adjoint_carries_a_gradient_through_the_recurrence_at_16_clips(direction):
    """the same case at B = 16: four whole adjoint blocks per direction, and a training forward whose eight groups hold 2 clips
    each for 27 steps"""
    _recurrence_case(16, direction)


def _model(mesh=MESH, mode=None):
    from dimx import lib
    from dimx.seq2seq_pretrain import EmocaConverter
    return EmocaConverter(mesh_dim=mesh, numeric_mode=lib.MODE_PARITY_F32 if mode is None else mode).cuda()


def _batch(B, T, mesh=MESH, seed=4):
    from dimx import prng
    templ = torch.from_numpy(prng.normal(seed, "conv.t", (B, mesh))) * 0.1
    xv = templ[:, None] + 0.05 * torch.from_numpy(prng.normal(seed, "conv.v", (B, T, mesh)))
    xe = torch.from_numpy(prng.normal(seed, "conv.e", (B, T, 56)))
    return xv.cuda(), templ.cuda(), xe.cuda()


def _check_step(tr, d, ref_losses, ref_grads, tag):
    for key, want in zip(("loss", "mse", "mouth"), ref_losses):
        got, want = d[key].item(), want.item()
        print("%s %s: %.9g vs %.9g" % (tag, key, got, want))
        assert abs(got - want) <= 1e-5 * abs(want), (key, got, want)
    assert len(ref_grads) == 20 and len(tr.layout) == 20
    worst = 0.0
    for name, g_ref in ref_grads.items():
        e = _rel(tr.grad(name), g_ref)
        worst = max(worst, e)
        assert e <= TOL, "%s: gradient of %s differs by %g of its maximum" % (tag, name, e)
    print("%s: worst gradient error %.2e of max|ref| over 20 tensors" % (tag, worst))


@pytest.mark.parametrize("with_mouth", [True, False])
@pytest.mark.parametrize("with_template", [True, False])
@pytest.mark.parametrize("B", [1, 3])
def test_step_matches_float64_autograd(B, with_template, with_mouth):
    import converter_ref
    from dimx.train_hip import ConverterHipTrainer
    T = 40
    model = _model()
    tr = ConverterHipTrainer(model)
    xv, templ, xe = _batch(B, T)
    templ = templ if with_template else None
    mouth = MOUTH if with_mouth else None
    motion = tr.motion(xe)
    (rl, rg, rmesh) = converter_ref.converter_step(model.state_dict(), motion, templ, xv, mouth)
    for flags in (0, 1):
        d, mesh = tr.forward_backward(xv, templ, xe, mouth_map=mouth, flags=flags)
        _check_step(tr, d, rl, rg, "converter step B=%d templ=%d mouth=%d flags=%d" % (B, with_template, with_mouth, flags))
        assert _rel(mesh, rmesh) <= TOL
        # the inference head on the same path, bit for bit
        want = tr.eng.mesh_head(motion, templ, safe=bool(flags))
        assert torch.equal(mesh, want), "mesh_out differs from dimx_mesh_head on the same path"
        # grads == NULL: forward and loss only, the same loss
        g0 = tr.grads.clone()
        d2, mesh2 = tr.evaluate(xv, templ, xe, mouth_map=mouth, flags=flags)
        assert all(torch.equal(d[k], d2[k]) for k in d) and torch.equal(mesh, mesh2) and torch.equal(g0, tr.grads)
    FAULTS.append(tr.eng.lstm_faults())


def test_split_batch_head_and_step_match_float64_autograd():
    """B = 130, T = 3: the group kernel takes the batch in two launches (128 + 2 clips), with and without the save rows, and the
    adjoint in 33 blocks per direction.  dimx_mesh_head on both paths, then one training step per path: losses, all 20 gradients,
    and mesh_out bit-equal to the inference head on the same path.  On the reference alone: its f32 arithmetic lies 10x below the
    tolerance on the mesh and on every gradient, and the recurrence carries 100x the tolerance of the mesh."""
    import converter_ref
    from dimx import prng
    from dimx.train_hip import ConverterHipTrainer
    B, T = 130, 3
    model = _model()
    tr = ConverterHipTrainer(model)
    xv, templ, _ = _batch(B, T)
    # a template a tenth of _batch's: at full size it is 0.4 of a mesh whose head output is 0.06, the bound 1e-4 * max|ref| would
    # be set by the template and the recurrence would carry only 0.9e-2 of it at T = 3
    xv, templ = xv - 0.9 * templ[:, None], 0.1 * templ
    motion = torch.from_numpy(prng.normal(4, "conv.split.motion", (B, T, 56))).float().cuda()
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items() if k.startswith("vertice_map_reverse")}
    rl, rg, rmesh = converter_ref.converter_step(sd, motion, templ, xv, MOUTH)
    _, rg32, rmesh32 = converter_ref.converter_step(sd, motion, templ, xv, MOUTH, dtype=torch.float32)
    noise = max([_rel(rmesh32, rmesh)] + [_rel(rg32[k], rg[k]) for k in rg])
    sd0 = {k: torch.zeros_like(v) if "weight_hh" in k else v for k, v in sd.items()}
    share = _rel(converter_ref.converter_step(sd0, motion, templ, xv, MOUTH)[2], rmesh)
    print("split batch reference: torch f32 vs f64 %.1e of max|ref|, recurrent share of the mesh %.2e of max|mesh|" % (noise, share))
    assert noise * 10 <= TOL, "torch's own f32 noise %g is not 10x below the tolerance" % noise
    assert share >= 100 * TOL, "the case does not exercise the recurrence (share %g)" % share
    for flags in (0, 1):
        path = "safe" if flags else "default"
        head = tr.eng.mesh_head(motion, templ, safe=bool(flags)).clone()
        err_clip = (head.double().cpu() - rmesh).abs().amax(dim=(1, 2)) / rmesh.abs().max().item()
        worst = int(err_clip.argmax())
        print("mesh_head B=%d T=%d %s path: %.2e of max|ref| (worst clip %d, launch %d of the group kernel)"
              % (B, T, path, err_clip.max().item(), worst, worst // 128))
        assert err_clip.max().item() <= TOL, "clips above the tolerance: %s" % [(b, "%.1e" % e) for b, e in enumerate(err_clip.tolist())
                                                                                 if e > TOL]
        d, mesh = tr.forward_backward(xv, templ, None, mouth_map=MOUTH, flags=flags, motion=motion)
        _check_step(tr, d, rl, rg, "converter step B=%d T=%d flags=%d" % (B, T, flags))
        assert torch.equal(mesh, head), "mesh_out differs from dimx_mesh_head on the same path"
    FAULTS.append(tr.eng.lstm_faults())


def test_full_size_step_matches_float64_autograd():
    """V = 70110 (no multiple of 4), B = 1, T = 60, once: norms and sampled entries per tensor, as the VQ test does"""
    import converter_ref
    from dimx import prng
    from dimx.train_hip import ConverterHipTrainer
    V, B, T = 70110, 1, 60
    model = _model(V)
    tr = ConverterHipTrainer(model)
    xv, templ, xe = _batch(B, T, mesh=V)
    mouth = [int(i) for i in prng.integers(3, "conv.mouth", (500,), 0, V // 3)] + [11, 11]
    motion = tr.motion(xe)
    d, mesh = tr.forward_backward(xv, templ, xe, mouth_map=mouth)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items() if k.startswith("vertice_map_reverse")}
    rl, rg, rmesh = converter_ref.converter_step(sd, motion, templ, xv, mouth)
    for key, want in zip(("loss", "mse", "mouth"), rl):
        assert abs(d[key].item() - want.item()) <= 1e-5 * abs(want.item()), (key, d[key].item(), want.item())
    assert _rel(mesh, rmesh) <= TOL
    assert torch.equal(mesh, tr.eng.mesh_head(motion, templ))
    for name, g_ref in rg.items():
        gh = tr.grad(name).double().reshape(-1).cpu()
        gr = g_ref.reshape(-1)
        gmax = gr.abs().max().item()
        assert abs(gh.norm().item() - gr.norm().item()) <= TOL * max(gr.norm().item(), gmax), name
        pos = torch.from_numpy(prng.integers(3, "conv.sample." + name, (128,), 0, gh.numel()))
        assert (gh[pos] - gr[pos]).abs().max().item() <= TOL * gmax, name
    FAULTS.append(tr.eng.lstm_faults())


def test_reruns_are_bit_identical():
    from dimx.train_hip import ConverterHipTrainer
    model = _model()
    tr = ConverterHipTrainer(model)
    xv, templ, xe = _batch(3, 64, seed=8)
    for flags in (0, 1):
        d1, m1 = tr.forward_backward(xv, templ, xe, mouth_map=MOUTH, flags=flags)
        g1 = tr.grads.clone()
        d2, m2 = tr.forward_backward(xv, templ, xe, mouth_map=MOUTH, flags=flags)
        assert torch.equal(g1, tr.grads) and torch.equal(m1, m2) and all(torch.equal(d1[k], d2[k]) for k in d1)
        assert g1.abs().max().item() > 0
    FAULTS.append(tr.eng.lstm_faults())


def test_two_steps_match_torch_adamw_and_leave_the_other_tensors_alone():
    from dimx import train as TR
    from dimx.train_hip import ConverterHipTrainer
    model = _model()
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    tr = ConverterHipTrainer(model, lr=1e-4)
    names = [n for n, _, _ in tr.layout]
    assert sorted(names) == sorted(n for n, _ in model.named_parameters() if n.startswith("vertice_map_reverse_lstm.") or
                                   n.startswith("vertice_map_reverse."))
    assert sorted(id(p) for p in model.dimx_trainable_parameters()) == sorted(id(dict(model.named_parameters())[n]) for n in names)
    xv, templ, xe = _batch(2, 48, seed=9)
    motion = tr.motion(xe)
    P = {k: v.detach().clone().requires_grad_(k in names) for k, v in before.items()}
    opt = torch.optim.AdamW([P[k] for k in names], lr=1e-4)
    for _ in range(2):
        tr.train_step(xv, templ, xe, mouth_map=MOUTH)
        opt.zero_grad()
        with torch.enable_grad():
            TR.converter_loss(P, xv, templ, xe, MOUTH, motion=motion)[0].backward()
        opt.step()
    diff = torch.cat([(tr.view(tr.params, k) - P[k].detach()).abs().reshape(-1) for k in names])
    over = int((diff > 1e-5).sum())
    print("converter: 2 AdamW steps, |HIP - torch| weight difference max %.2e, %d of %d elements above 1e-5"
          % (diff.max().item(), over, diff.numel()))
    # the bounds of tests/test_gpu_train_vq.py's two-step comparison
    assert over <= diff.numel() * 1e-5 and diff.max().item() <= 4 * 1e-4
    tr.sync_to_model()
    after = model.state_dict()
    moved = 0
    for k, v in before.items():
        if k in names:
            moved += int(not torch.equal(after[k], v))
        else:
            assert torch.equal(after[k], v), "%s is outside the arena and must come back bit-identical" % k
    assert moved == 20
    FAULTS.append(tr.eng.lstm_faults())


def test_bf16_mode_agrees_with_f32_and_trains():
    from dimx import lib
    from dimx.train_hip import ConverterHipTrainer
    xv, templ, xe = _batch(2, 120, seed=10)
    tf = ConverterHipTrainer(_model())
    df, _ = tf.forward_backward(xv, templ, xe, mouth_map=MOUTH)
    tb = ConverterHipTrainer(_model(mode=lib.MODE_PERF_BF16), lr=1e-4)
    db, _ = tb.forward_backward(xv, templ, xe, mouth_map=MOUTH)
    for k in ("loss", "mse", "mouth"):
        print("bf16 %s %.6g, f32 %.6g" % (k, db[k].item(), df[k].item()))
        assert abs(db[k].item() - df[k].item()) <= 0.02 * abs(df[k].item()), (k, db[k].item(), df[k].item())
    first = None
    for _ in range(5):
        tb.train_step(xv, templ, xe, mouth_map=MOUTH)
        first = tb.last["loss"].item() if first is None else first
    assert tb.last["loss"].item() < first, (first, tb.last["loss"].item())
    FAULTS.append(tf.eng.lstm_faults() + tb.eng.lstm_faults())


def test_checkpoint_hands_off_to_speaker_slmft(tmp_path):
    from dimx import prng
    from dimx.seq2seq_pretrain import SpeakerSLMFT
    from dimx.train_hip import ConverterHipTrainer
    model = _model()
    tr = ConverterHipTrainer(model, lr=1e-4)
    xv, templ, xe = _batch(2, 32, seed=12)
    for _ in range(2):
        tr.train_step(xv, templ, xe, mouth_map=MOUTH)
    tr.sync_to_model()
    path = tmp_path / "best_converter.pt"
    torch.save(model.state_dict(), str(path))
    slm = SpeakerSLMFT(mesh_dim=MESH, converter_ckpt=str(path)).cuda()
    for n, _, _ in tr.layout:
        assert torch.equal(slm.state_dict()[n], model.state_dict()[n]), n
    tokens = torch.from_numpy(prng.integers(3, "conv.tok", (2, 32), 0, 512)).cuda()
    with torch.no_grad():
        mesh, emoca = slm.forward_vq_decoder(tokens, type="emoca", mode="val", template=templ)
    _, own = tr.evaluate(xv, templ, None, mouth_map=MOUTH, motion=emoca)
    scale = max(1.0, mesh.abs().max().item())
    err = (mesh - own).abs().max().item()
    print("hand-off: |SpeakerSLMFT mesh - trainer mesh| %.2e (tolerance %.2e)" % (err, 1e-4 * scale))
    assert err < 1e-4 * scale
    FAULTS.append(tr.eng.lstm_faults() + slm.engine("cuda:0").lstm_faults())


def test_train_converter_driver_writes_the_checkpoint(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "examples", "train_converter.py"), "--synthetic", "--epochs", "2", "--mesh-dim", str(MESH),
           "--clips", "3", "--frames", "24"]
    r = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "training for 2 epochs" in r.stdout and "Epoch 1 val loss:" in r.stdout and "Epoch: [1][2/3]" in r.stdout
    ck = tmp_path / "best_converter.pt"
    assert ck.exists(), r.stdout
    sd = torch.load(str(ck), map_location="cpu")
    assert "vertice_map_reverse_lstm.weight_hh_l1_reverse" in sd and "speaker_vq.quantize.embedding.weight" in sd


def test_zz_no_lstm_fault_was_counted():
    """last in the file: no bounded wait of a group kernel timed out anywhere above (nor in one more step of its own)"""
    from dimx.train_hip import ConverterHipTrainer
    tr = ConverterHipTrainer(_model())
    xv, templ, xe = _batch(1, 300, seed=13)
    tr.train_step(xv, templ, xe, mouth_map=MOUTH)
    FAULTS.append(tr.eng.lstm_faults())
    assert sum(FAULTS) == 0, FAULTS
