"""CPU: the HIP selection backend (dimx_op_fd_select) has no CPU fallback, and the set of backends is closed."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stub_model  # noqa: E402


def test_hip_backend_on_a_cpu_device_raises():
    from dimx import lib, x_engine_pt
    with pytest.raises(lib.DimxError):
        x_engine_pt.evaluate_test_epoch(stub_model.StubSLMFT(), stub_model.protocol_batches(), torch.device("cpu"), beam_size=10,
                                        fd_backend="hip")


def test_unknown_backend_still_fails_the_assertion():
    from dimx import x_engine_pt
    with pytest.raises(AssertionError):
        x_engine_pt.evaluate_test_epoch(stub_model.StubSLMFT(), stub_model.protocol_batches(), torch.device("cpu"), beam_size=10,
                                        fd_backend="nonsense")


def test_frechet_distances_hip_on_cpu_tensors_raises():
    from dimx import lib, metrics
    yt = torch.zeros(2, 8, 56)
    yp = torch.zeros(2, 3, 8, 56)
    with pytest.raises(lib.DimxError):
        metrics.frechet_distances_hip(yt, yp, [8, 8])
