"""Host side of the BIWI evaluation protocol (reference code/x_engine_pt.py:279-338) around a stub model with scripted
predictions: best candidate per clip, the strict '<' tie rule, the T - 2 stored frames, the speaker-id table and the calls."""
import numpy as np
import torch

B, T, V = 3, 9, 12
IDS = ["F3_e01.npy", "M6_e40.npy", "F2_e07.npy"]


class StubSpeaker(torch.nn.Module):
    """k-th call returns xe[:, 1:] + offsets[k][b]: the distance of clip b in call k is sqrt(56) * |offsets[k][b]|."""

    def __init__(self, offsets):
        super().__init__()
        self.offsets = offsets
        self.calls = []

    def forward(self, v_speaker, v_speaker_emoca, v_audio, mask, template, mode="train", speaker_ids=None):
        k = len(self.calls)
        self.calls.append({"mode": mode, "speaker_ids": speaker_ids.clone(), "mask": mask.clone(),
                           "shapes": (tuple(v_speaker.shape), tuple(v_speaker_emoca.shape), tuple(v_audio.shape), tuple(template.shape))})
        off = torch.tensor(self.offsets[k], dtype=torch.float32)[:, None, None]
        return torch.zeros(()), {}, v_speaker_emoca[:, 1:] + off


def _batch(seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, T, 768, generator=g), torch.randn(B, T, V, generator=g), torch.randn(B, V, generator=g),
            torch.round(torch.randn(B, T, 56, generator=g) * 64) / 64, list(IDS))   # multiples of 1/64: offsets below add exactly


def test_biwi_protocol_selection_and_shapes():
    import dimx  # noqa: F401
    from dimx.x_engine_pt import evaluate_test_epoch_biwi
    # clip 0: best is call 2; clip 1: calls 1 and 3 tie (same magnitude, opposite sign) -> the FIRST stays (strict <);
    # clip 2: call 0 is already the best
    offsets = [[0.5, 0.5, 0.125], [0.375, 0.25, 0.25], [0.125, 0.375, 0.375], [0.25, -0.25, 0.5]]
    model = StubSpeaker(offsets)
    batch = _batch()
    y_true, y_pred, x_all, ids = evaluate_test_epoch_biwi(model, [batch], torch.device("cpu"), beam_size=4)
    xe = batch[3]
    assert x_all == [] and ids == IDS
    assert len(model.calls) == 4 and all(c["mode"] == "train" for c in model.calls)
    assert len(y_true) == B and len(y_pred) == B
    for j, best_off in enumerate([0.125, 0.25, 0.125]):
        assert y_true[j].shape == (T - 2, 56) and y_pred[j].shape == (T - 2, 56)
        assert np.array_equal(y_true[j], xe[j, 2:].numpy())
        assert np.array_equal(y_pred[j], (xe[j, 2:] + torch.tensor(best_off)).numpy()), j   # clip 1: +0.25 (call 1), not -0.25
    c = model.calls[0]
    assert c["speaker_ids"].tolist() == [1, 13, 0] and c["speaker_ids"].dtype == torch.long
    assert c["mask"].dtype == torch.bool and c["mask"].shape == (B, T) and bool(c["mask"].all())
    assert c["shapes"] == ((B, T, V), (B, T, 56), (B, T, 768), (B, V))


def test_biwi_protocol_several_batches_and_speaker_table():
    import dimx  # noqa: F401
    from dimx.x_engine_pt import BIWI_SPEAKER_IDS, evaluate_test_epoch_biwi
    assert len(BIWI_SPEAKER_IDS) == 14 and sorted(BIWI_SPEAKER_IDS.values()) == list(range(14))
    assert BIWI_SPEAKER_IDS["F2"] == 0 and BIWI_SPEAKER_IDS["M3"] == 3 and BIWI_SPEAKER_IDS["F1"] == 6 and BIWI_SPEAKER_IDS["M6"] == 13
    model = StubSpeaker([[0.0] * B] * 6)
    y_true, y_pred, _, ids = evaluate_test_epoch_biwi(model, [_batch(1), _batch(2)], torch.device("cpu"), beam_size=3)
    assert len(model.calls) == 6 and len(y_true) == 2 * B and ids == IDS + IDS
    for a, b in zip(y_true, y_pred):
        assert np.array_equal(a, b)
