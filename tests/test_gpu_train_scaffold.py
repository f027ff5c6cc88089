"""GPU: what the six HIP training steps share in csrc/train.hip -- the per-handle plan registry (plan_of / train_forget) and the
sizing pass every entry point runs before its first launch (check_workspace).  The steps' arithmetic is checked by their own
files (tests/test_gpu_train_*.py); here: the plans of one handle do not alias, the DIM-Speaker plan follows a reloaded speaker
embedding, a destroyed handle leaves no plan behind, and dimx_train_*_workspace_bytes is exactly what a live step takes."""
import ctypes
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

MESH = 120      # the mesh width of tests/test_gpu_train_speaker.py: nothing here depends on V
SENTINEL = 12345.0


@pytest.fixture(scope="module")
def speaker_sd():
    """the state dict of a DIM-Speaker module at the tests' mesh width, its speaker embedding cut to 3 rows"""
    import dimx  # noqa: F401
    from dimx.seq2seq_pretrain import SpeakerSLMFT
    sd = {k: v.detach().clone() for k, v in SpeakerSLMFT(mesh_dim=MESH)._engine_state_dict().items()}
    sd["speaker_embed.weight"] = sd["speaker_embed.weight"][:3].clone()
    return sd


def _engine(sd, monkeypatch=None, vq_layers=None):
    """a speaker handle (variant 2 with the mesh head) holding ``sd``; vq_layers: with that many VQ-VAE transformer layers"""
    from dimx import lib as L
    from dimx.engine import Engine
    if vq_layers is not None:
        dims = L.speaker_dims(MESH)
        dims.vq_layers = vq_layers
        monkeypatch.setattr(L, "speaker_dims", lambda mesh_dim: dims)
        sd = {k: v for k, v in sd.items()
              if not (re.search(r"_transformer\.net\.(\d+)\.", k) and int(re.search(r"_transformer\.net\.(\d+)\.", k).group(1)) >= 2 * vq_layers)}
    eng = Engine("cuda:0", L.MODE_PARITY_F32, variant="speaker", mesh_dim=MESH)
    eng.load_state_dict(sd)
    assert eng.missing_weights() == 0
    return eng


def _layout(eng, family, *slot):
    """(total, [(name, offset, numel)]) through dimx_<family>_num_params / _param_info / _total"""
    from dimx import lib as L
    lib = eng.lib
    n = getattr(lib, "dimx_%s_num_params" % family)(eng.h, *slot)
    if n <= 0:
        L.check(n, "dimx_%s_num_params" % family)
    out = []
    for i in range(n):
        name, off, numel = ctypes.c_char_p(), ctypes.c_int64(), ctypes.c_int64()
        L.check(getattr(lib, "dimx_%s_param_info" % family)(eng.h, *slot, i, ctypes.byref(name), ctypes.byref(off), ctypes.byref(numel)),
                "dimx_%s_param_info" % family)
        out.append((name.value.decode(), int(off.value), int(numel.value)))
    return int(getattr(lib, "dimx_%s_total" % family)(eng.h, *slot)), out


QUERIES = [("train_vq", 0), ("train_vq", 1), ("train_conv",), ("train_spk",)]


def test_plans_of_one_handle_do_not_alias(speaker_sd):
    a, b = _engine(speaker_sd), _engine(speaker_sd)
    forward = [_layout(a, *q) for q in QUERIES]
    backward = [_layout(b, *q) for q in reversed(QUERIES)][::-1]
    assert forward == backward
    for i in range(4):
        for j in range(i + 1, 4):
            assert forward[i] != forward[j], (QUERIES[i], QUERIES[j])
    # asked again, every kind still answers with its own plan
    assert [_layout(a, *q) for q in QUERIES] == forward
    prefixes = ("speaker_vq.", "listener_vq.", "vertice_map_reverse", None)
    for (total, lay), pre in zip(forward, prefixes):
        assert total >= sum(n for _, _, n in lay) and lay[0][1] == 0
        if pre is not None:
            assert all(name.startswith(pre) for name, _, _ in lay), pre
    assert len(forward[2][1]) == 20 and forward[3][1][-1][0] == "speaker_embed.weight"
    a.close()
    b.close()


def test_speaker_plan_follows_a_reloaded_embedding(speaker_sd):
    eng = _engine(speaker_sd)
    dim = speaker_sd["speaker_embed.weight"].shape[1]
    total3, lay3 = _layout(eng, "train_spk")
    assert lay3[-1] == ("speaker_embed.weight", lay3[-1][1], 3 * dim)
    conv = _layout(eng, "train_conv")
    eng.load_state_dict({"speaker_embed.weight": torch.zeros(5, dim)}, new_checkpoint=False)
    total5, lay5 = _layout(eng, "train_spk")
    pad4 = lambda n: (n + 3) // 4 * 4           # every tensor starts on a 4-float boundary of the arena
    assert total5 - total3 == pad4(5 * dim) - pad4(3 * dim)
    assert lay5[-1] == ("speaker_embed.weight", lay3[-1][1], 5 * dim) and lay5[:-1] == lay3[:-1]
    assert _layout(eng, "train_conv") == conv    # the other plans of the handle stay
    eng.close()


def test_no_plan_outlives_its_handle(speaker_sd, monkeypatch):
    from dimx import lib as L
    layers = L.speaker_dims(MESH).vq_layers
    assert layers >= 2
    eng = _engine(speaker_sd)
    n_spk, n_vq = len(_layout(eng, "train_spk")[1]), len(_layout(eng, "train_vq", 0)[1])
    eng.close()
    # a new handle with one VQ-VAE layer less (whether or not the allocator hands the old address back): 11 tensors per block
    eng2 = _engine(speaker_sd, monkeypatch, vq_layers=layers - 1)
    assert len(_layout(eng2, "train_spk")[1]) == n_spk - 11          # speaker_vq.decoder only
    assert len(_layout(eng2, "train_vq", 0)[1]) == n_vq - 22         # encoder and decoder
    eng2.close()


# ---------------------------------------------------------------------------------------------------------------- sizing
def _f(seed, tag, *shape):
    from dimx import prng
    return torch.from_numpy(prng.normal(seed, "scaffold." + tag, shape)).cuda()


def _main(mode):
    from dimx.seq2seq_pretrain import SLMFT
    from dimx.train_hip import HipTrainer
    tr = HipTrainer(SLMFT(numeric_mode=mode).cuda())

    def call(B, T):
        mask = torch.ones(B, T, dtype=torch.bool, device="cuda")
        tr.forward_backward(_f(1, "vs", B, T, 56), _f(1, "vl", B, T, 56), _f(1, "va", B, T, 768), mask,
                            kv_mask=torch.ones(B, T - 1, dtype=torch.bool, device="cuda"), z_l=torch.zeros(B, T, dtype=torch.long, device="cuda"))
    return tr, call, "dimx_train_forward_backward", ()


def _legacy(mode):
    from dimx import seq2seq
    from dimx import train as Tr
    from dimx.train_hip import LegacyHipTrainer
    m = seq2seq.ListenerGenerator(numeric_mode=mode).cuda()
    Tr.set_legacy_trainable(m)
    tr = LegacyHipTrainer(m.train())

    def call(B, T):
        mask = torch.ones(B, T, dtype=torch.bool, device="cuda")
        tr.forward_backward(_f(2, "vs", B, T, 824), _f(2, "vl", B, T, 56), mask, listener_ids=torch.tensor([3] * B, device="cuda"))
    return tr, call, "dimx_train_legacy_forward_backward", (13,)          # pred_out


def _slm(mode):
    from dimx import train as Tr
    from dimx.seq2seq_pretrain import SLM
    from dimx.train_hip import SlmHipTrainer
    m = SLM(numeric_mode=mode).cuda()
    Tr.set_slm_trainable(m)
    tr = SlmHipTrainer(m.train())

    def call(B, T):
        mask = torch.ones(B, T, dtype=torch.bool, device="cuda")
        none = torch.zeros(B, T, dtype=torch.bool, device="cuda")
        tr.forward_backward(_f(3, "vs", B, T, 56), _f(3, "vl", B, T, 56), _f(3, "va", B, T, 768), mask, mask_speaker=none, mask_listener=none)
    return tr, call, "dimx_train_slm_forward_backward", ()


def _vq(mode):
    import os
    from dimx.config import load_cfg_from_cfg_file
    from dimx.models import VQAutoEncoder
    from dimx.train_hip import VqHipTrainer
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = load_cfg_from_cfg_file(os.path.join(root, "dyadic-interaction-modeling_amd", "config.yaml"))
    tr = VqHipTrainer(VQAutoEncoder(cfg, numeric_mode=mode).cuda(), dropout=0.0)
    return tr, (lambda B, T: tr.forward_backward(_f(4, "x", B, T, 56))), "dimx_train_vq_forward_backward", (13, 14)    # pred_out, idx_out


def _conv(mode):
    from dimx.seq2seq_pretrain import EmocaConverter
    from dimx.train_hip import ConverterHipTrainer
    tr = ConverterHipTrainer(EmocaConverter(mesh_dim=MESH, numeric_mode=mode).cuda())

    def call(B, T):
        tr.forward_backward(_f(5, "v", B, T, MESH), _f(5, "t", B, MESH), None, mouth_map=[3, 3, 11, 39], motion=_f(5, "m", B, T, 56))
    return tr, call, "dimx_train_conv_forward_backward", (12,)            # mesh_out


def _spk(mode):
    from dimx import train as Tr
    from dimx.seq2seq_pretrain import SpeakerSLMFT
    from dimx.train_hip import SpeakerHipTrainer
    m = SpeakerSLMFT(mesh_dim=MESH, numeric_mode=mode).cuda()
    Tr.set_speaker_trainable(m)
    tr = SpeakerHipTrainer(m.train(), mouth_map=None)

    def call(B, T):
        mask = torch.ones(B, T, dtype=torch.bool, device="cuda")
        tr.forward_backward(None, _f(6, "e", B, T, 56), _f(6, "a", B, T, 768), mask, None)
    return tr, call, "dimx_train_spk_forward_backward", (14, 15)          # idx_out, pred_out


@pytest.mark.parametrize("step,shapes", [(_main, [(1, 2)]), (_legacy, [(1, 2)]), (_slm, [(1, 2)]), (_vq, [(1, 1), (1, 2)]),
                                         (_conv, [(1, 1), (1, 2)]), (_spk, [(1, 2)])], ids=["main", "legacy", "slm", "vq", "conv", "spk"])
def test_workspace_bytes_is_what_a_live_step_takes(step, shapes, monkeypatch):
    """The trainer hands its step exactly dimx_train_*_workspace_bytes.  That figure is sized for the call that allocates the
    most: every optional input there, every optional output left to the workspace, weight gradients on the side stream.  Such
    a call must run in it, and must be refused (DIMX_ERR_WORKSPACE, -5) with 256 bytes less -- by the sizing pass, before
    anything is launched: the gradient arena still holds the sentinel afterwards."""
    from dimx import lib as L
    monkeypatch.setenv("DIMX_TRAIN_SIDE", "1")      # the DIM-Listener steps: what their workspace_bytes is sized with
    monkeypatch.setenv("DIMX_TRAIN_GRAPH", "0")
    tr, call, fn_name, outputs_to_workspace = step(L.MODE_PARITY_F32)
    real = getattr(tr.lib, fn_name)
    shrink = [0]

    def entry(*args):
        args = list(args)
        for i in outputs_to_workspace:
            args[i] = None
        args[-2] -= shrink[0]                       # ws_bytes (the stream is last)
        return real(*args)
    monkeypatch.setattr(tr.lib, fn_name, entry)
    for B, T in shapes:
        for less in (0, 256):
            shrink[0] = less
            tr._ws, tr._ws_bytes = None, 0          # a workspace of exactly this shape's size
            tr.grads.fill_(SENTINEL)
            if less == 0:
                call(B, T)
                torch.cuda.synchronize()
                assert not bool((tr.grads == SENTINEL).all())
                continue
            with pytest.raises(L.DimxError, match=r"failed \(-5\): train\w*: workspace \d+ < required \d+ \(dimx_train\w*_workspace_bytes\)"):
                call(B, T)
            torch.cuda.synchronize()
            assert bool((tr.grads == SENTINEL).all()), "a kernel ran before the workspace was refused"
