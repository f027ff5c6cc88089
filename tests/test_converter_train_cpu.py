"""CPU: the host side of the DIM-Speaker converter training step (reference code/train_converter.py:17-96): the autograd
checker's loss against the reference's literal expression, the mouth-vertex weight vector, the exported C-ABI symbols and the
driver's epoch loop over a stub trainer.  The GPU step itself is tests/test_gpu_train_converter.py."""
import ctypes
import importlib.util
import os
import types

import pytest
import torch

import dimx  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESH = 150
MOUTH = [0, 3, 7, 7, 21, 49]          # vertex 7 twice: fancy indexing counts it twice


def _sd(mesh=MESH, seed=5):
    from dimx import weights
    spec = weights.vq_spec(prefix="speaker_vq.") + weights.emoca_converter_spec(mesh)
    return weights.synth_state_dict(spec, seed)


def _batch(B, T, mesh=MESH, seed=4):
    from dimx import prng
    templ = torch.from_numpy(prng.normal(seed, "conv.t", (B, mesh))) * 0.1
    xv = templ[:, None] + 0.05 * torch.from_numpy(prng.normal(seed, "conv.v", (B, T, mesh)))
    xe = torch.from_numpy(prng.normal(seed, "conv.e", (B, T, 56)))
    return xv, templ, xe


def test_converter_loss_is_the_reference_expression_at_batch_one():
    import converter_ref
    from dimx import train as TR
    sd = _sd()
    xv, templ, xe = _batch(1, 9)
    loss, mse, mouth, mesh = TR.converter_loss(sd, xv, templ, xe, MOUTH)
    assert tuple(mesh.shape) == (1, 9, MESH)
    want = converter_ref.literal_loss(mesh, xv, MOUTH)
    assert abs(float(loss) - float(want)) <= 1e-6 * abs(float(want)), (float(loss), float(want))
    assert abs(float(loss) - float(mse) - 5 * float(mouth)) <= 1e-6 * abs(float(loss))
    # the duplicate matters: the map without it gives another mouth term
    other = converter_ref.literal_loss(mesh, xv, sorted(set(MOUTH)))
    assert abs(float(other) - float(want)) > 1e-4 * abs(float(want))
    # the head alone, on a given motion, equals the stock-module yardstick
    motion = torch.randn(1, 9, 56, generator=torch.Generator().manual_seed(1))
    l2, _, _, mesh2 = TR.converter_loss(sd, xv, templ, None, MOUTH, motion=motion)
    (rl, _, _), _, rmesh = converter_ref.converter_step(sd, motion, templ, xv, MOUTH, dtype=torch.float32)
    assert (mesh2 - rmesh).abs().max().item() <= 1e-6 * max(1.0, rmesh.abs().max().item())
    assert abs(float(l2) - float(rl)) <= 1e-6 * abs(float(rl))


def test_converter_loss_gradients_reach_exactly_the_twenty_head_tensors():
    from dimx import train as TR
    sd = _sd()
    xv, templ, xe = _batch(2, 6)
    P = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in sd.items()}
    with torch.enable_grad():
        TR.converter_loss(P, xv, templ, xe, MOUTH)[0].backward()
    got = sorted(k for k, v in P.items() if v.grad is not None)
    want = sorted(k for k in sd if k.startswith("vertice_map_reverse_lstm.") or k.startswith("vertice_map_reverse."))
    assert got == want and len(got) == 20


def test_vertex_weight_vector_holds_the_multiplicities():
    from dimx import train as TR
    from dimx.train_hip import ConverterHipTrainer
    w = TR.mouth_vertex_weights(MOUTH, MESH // 3)
    assert w.dtype == torch.float32 and tuple(w.shape) == (MESH // 3,)
    assert w[7] == 2 and w[0] == 1 and w[3] == 1 and w[21] == 1 and w[49] == 1 and float(w.sum()) == len(MOUTH)
    # the trainer builds its device vector with the same function (no GPU needed for that part)
    stub = types.SimpleNamespace(_vw={}, model=types.SimpleNamespace(mesh_dim=MESH), device=torch.device("cpu"))
    vw, n = ConverterHipTrainer.vertex_weights(stub, MOUTH)
    assert n == len(MOUTH) and torch.equal(vw, w)
    # sum_v m_v |d_v|^2 / (3 N_m) is the fancy-indexed mean
    d = torch.randn(4, MESH // 3, 3, generator=torch.Generator().manual_seed(0))
    lit = (d[:, MOUTH, :] ** 2).mean()
    assert abs(float((w[None, :, None] * d ** 2).sum() / (4 * 3 * len(MOUTH))) - float(lit)) <= 1e-6 * float(lit)
    with pytest.raises(AssertionError):
        TR.mouth_vertex_weights([MESH // 3], MESH // 3)


def test_library_exports_the_converter_training_symbols():
    from dimx import lib
    hdr = open(os.path.join(ROOT, "include", "dimx.h")).read()
    names = ["dimx_train_conv_num_params", "dimx_train_conv_total", "dimx_train_conv_param_info", "dimx_train_conv_workspace_bytes",
             "dimx_train_conv_forward_backward", "dimx_op_lstm_layer_bwd"]
    l = lib.load()
    for name in names:
        assert (name + "(") in hdr, name
        assert name in lib.SIGNATURES, name
        assert hasattr(l, name), name
    assert isinstance(l, ctypes.CDLL)
    # a null handle is refused, not dereferenced
    assert l.dimx_train_conv_num_params(None) < 0
    assert l.dimx_train_conv_workspace_bytes(None, 1, 10) == 0


def _driver():
    spec = importlib.util.spec_from_file_location("train_converter_example", os.path.join(ROOT, "examples", "train_converter.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)          # must import without running (main() guard)
    return mod


class _StubTrainer:
    """train_step / evaluate of ConverterHipTrainer with scripted losses"""

    def __init__(self, train_losses, val_losses):
        self.train_losses, self.val_losses = list(train_losses), list(val_losses)
        self.clip = None
        self.clips_seen, self.synced, self.calls = [], 0, []

    def train_step(self, xv, xt, xe, mouth_map=None, flags=0):
        self.clips_seen.append(self.clip)
        self.calls.append(("train", tuple(xv.shape), mouth_map, flags))
        return torch.tensor(self.train_losses.pop(0)), None

    def evaluate(self, xv, xt, xe, mouth_map=None, flags=0):
        self.calls.append(("eval", tuple(xv.shape), mouth_map, flags))
        return {"loss": torch.tensor(self.val_losses.pop(0))}, None

    def sync_to_model(self):
        self.synced += 1


def test_driver_loop_prints_the_reference_lines_and_keeps_the_best_checkpoint(tmp_path, capsys):
    drv = _driver()
    loader = [_batch(1, 4, seed=s) + (["F2_e%02d.npy" % s],) for s in (1, 2, 3)]
    model = torch.nn.Linear(2, 2)
    out = tmp_path / "best_converter.pt"
    # epoch 0: val 0.5 (saved), epoch 1: val 0.75 (not saved), epoch 2: val 0.25 (saved)
    st = _StubTrainer([1.0, 2.0, 3.0] + [0.5, 0.5, 0.5] + [0.25, 0.25, 0.25], [0.5] * 3 + [0.75] * 3 + [0.25] * 3)
    saves = []
    real_save = torch.save
    torch.save = lambda obj, path: (saves.append(path), real_save(obj, path))[1]
    try:
        best = drv.fit(st, model, loader, loader, torch.device("cpu"), 3, str(out), mouth_map=MOUTH)
    finally:
        torch.save = real_save
    lines = capsys.readouterr().out.splitlines()
    assert lines == ["training for 3 epochs",
                     "Epoch: [0][2/3]\tLoss 2.0000\t", "Epoch 0 val loss: 0.5",
                     "Epoch: [1][2/3]\tLoss 0.5000\t", "Epoch 1 val loss: 0.75",
                     "Epoch: [2][2/3]\tLoss 0.2500\t", "Epoch 2 val loss: 0.25"]
    assert best == 0.25 and len(saves) == 2 and st.synced == 2 and out.exists()
    assert set(torch.load(str(out))) == {"weight", "bias"}
    assert st.clips_seen == [0.0] * 9, "the drop-in default applies no clipping"
    assert all(c[2] == MOUTH and c[3] == 0 for c in st.calls)
    # the validation pass sees the loader it is given, batch by batch
    assert [c[0] for c in st.calls[:6]] == ["train"] * 3 + ["eval"] * 3


def test_driver_defaults_and_mouth_map_file(tmp_path):
    drv = _driver()
    f = tmp_path / "lve.txt"
    f.write_text("3, 7, 7, 11")
    assert drv.read_mouth_map(str(f)) == [3, 7, 7, 11]
    import inspect
    assert inspect.signature(drv.train_epoch).parameters["clip"].default == 0.0
    assert inspect.signature(drv.fit).parameters["clip"].default == 0.0
    with pytest.raises(SystemExit):
        drv.main([])          # no BIWI data: only --synthetic runs
