"""DIM-Speaker surface without a GPU: the state-dict spec of SpeakerSLMFT (reference code/seq2seq_pretrain.py:540-635,
:784-824), the module's construction on the CPU and the two new exports of the built library."""
import ctypes
import os

import torch

MESH = 363     # 121 vertices: a small stand-in for the reference's 70110


def test_lstm_entries_equal_torch_lstm_state_dict():
    import dimx  # noqa: F401
    from dimx import weights
    ref = torch.nn.LSTM(56, 384, 2, batch_first=True, bidirectional=True).state_dict()
    pre = "vertice_map_reverse_lstm."
    got = {n[len(pre):]: tuple(s) for n, s, _, _ in weights.speaker_slmft_spec(MESH) if n.startswith(pre)}
    assert set(got) == set(ref)
    for k, v in ref.items():
        assert got[k] == tuple(v.shape), k


def test_spec_contains_slm_spec_and_the_converter():
    import dimx  # noqa: F401
    from dimx import weights
    spec = {n: tuple(s) for n, s, _, _ in weights.speaker_slmft_spec()}
    for n, s, _, _ in weights.slm_spec():
        assert spec[n] == tuple(s), n
    assert spec["vertice_map_reverse.2.weight"] == (70110, 768) and spec["vertice_map_reverse2.2.weight"] == (70110, 768)
    assert spec["vertice_mapping.0.weight"] == (56, 70110) and spec["squasher.0.0.weight"] == (56, 56, 5)
    assert spec["vertice_map_reverse.0.weight"] == (768, 768) and spec["vertice_map_reverse.2.bias"] == (70110,)
    assert spec["W"] == (2,) and spec["speaker_embed.weight"] == (15, 384)
    assert spec["vertice_map_reverse_lstm_2.weight_ih_l1_reverse"] == (1536, 768)


def test_speaker_slmft_constructs_on_cpu_and_round_trips():
    import dimx  # noqa: F401
    from dimx import weights
    from dimx.seq2seq_pretrain import SpeakerSLMFT
    m = SpeakerSLMFT(mesh_dim=MESH)
    sd = m.state_dict()
    spec = weights.speaker_slmft_spec(MESH)
    assert set(sd) == {n for n, _, _, _ in spec}
    for n, s, _, _ in spec:
        assert tuple(sd[n].shape) == tuple(s), n
    other = SpeakerSLMFT(mesh_dim=MESH, synthetic_seed=5)
    assert not torch.equal(other.state_dict()["vertice_map_reverse_lstm.weight_hh_l0"], sd["vertice_map_reverse_lstm.weight_hh_l0"])
    res = other.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in other.state_dict().items():
        assert torch.equal(v, sd[k]), k
    # the LSTM tensors follow torch's own initialisation range +-1/sqrt(hidden); never-applied tensors are zeros
    w = sd["vertice_map_reverse_lstm.weight_ih_l0"]
    assert w.abs().max() <= 384 ** -0.5 and w.abs().max() > 0.9 * 384 ** -0.5
    assert not sd["vertice_map_reverse2.2.weight"].any() and sd["vertice_map_reverse.2.weight"].any()


def test_emoca_converter_state_dict_and_errors():
    import pytest
    import dimx  # noqa: F401
    from dimx import weights
    from dimx.seq2seq_pretrain import EmocaConverter, SpeakerSLMFT
    c = EmocaConverter(mesh_dim=MESH)
    want = {n for n, _, _, _ in weights.vq_spec(prefix="speaker_vq.") + weights.emoca_converter_spec(MESH)}
    assert set(c.state_dict()) == want
    m = SpeakerSLMFT(mesh_dim=MESH)
    with pytest.raises(ValueError):
        m(torch.zeros(1, 4, MESH), None, torch.zeros(1, 4, 768), torch.ones(1, 4, dtype=torch.bool), torch.zeros(1, MESH))
    with pytest.raises(NotImplementedError):
        m.forward_vq_decoder(torch.zeros(1, 3, dtype=torch.long), type="mesh", mode="val")


def test_library_exports_the_speaker_entry_points():
    import dimx  # noqa: F401
    from dimx import lib as L
    assert os.path.exists(L.LIB_PATH), "libdimx_hip.so is not built"
    so = ctypes.CDLL(L.LIB_PATH)
    for name in ("dimx_op_lstm_layer", "dimx_mesh_head", "dimx_lstm_faults"):
        assert hasattr(so, name), name
        assert name in L.SIGNATURES, name
    assert [f[0] for f in L.Dims._fields_][-1] == "mesh_dim"
