"""CPU: the listener metrics operator (dimx_op_listener_metrics) is exported, sizes its workspace, and has no CPU fallback."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stub_model  # noqa: E402


def test_library_exports_the_operator_and_its_workspace_query():
    from dimx import lib
    l = lib.load()
    for name in ("dimx_op_listener_metrics", "dimx_op_listener_metrics_ws_bytes"):
        assert name in lib.SIGNATURES and hasattr(l, name)


def test_workspace_bytes():
    from dimx import lib
    l = lib.load()
    need = int(l.dimx_op_listener_metrics_ws_bytes(4, 6, 112))
    assert need >= 4 * 6 * 112 * 112 * 8 and need % 8 == 0
    assert l.dimx_op_listener_metrics_ws_bytes(0, 6, 112) == 0
    assert l.dimx_op_listener_metrics_ws_bytes(4, 9, 112) == 0
    assert l.dimx_op_listener_metrics_ws_bytes(4, 0, 112) == 0
    assert l.dimx_op_listener_metrics_ws_bytes(4, 6, 113) == 0
    assert l.dimx_op_listener_metrics_ws_bytes(4, 6, 0) == 0


def test_the_six_windows_of_the_python_layer():
    from dimx.engine import LISTENER_WINDOWS
    assert dict(LISTENER_WINDOWS) == {"fid_pose": (0, 0, 0, 6), "fid_exp": (0, 0, 6, 50), "pfid_pose": (0, 6, 0, 6),
                                      "pfid_exp": (6, 50, 6, 50), "fid": (0, 0, 0, 56), "pfid": (0, 56, 0, 56)}


def test_op_listener_metrics_on_cpu_tensors_raises():
    from dimx import engine, lib
    y = torch.zeros(2, 8, 56)
    with pytest.raises(lib.DimxError):
        engine.op_listener_metrics(y, y, y, [8, 8])


def test_accumulator_update_on_cpu_tensors_raises_and_result_needs_an_update():
    from dimx import lib, metrics
    y = torch.zeros(2, 8, 56)
    acc = metrics.ListenerMetrics()
    with pytest.raises(lib.DimxError):
        acc.update(y, y, y, [8, 8])
    with pytest.raises(ValueError):
        acc.result()


def test_protocol_with_metrics_needs_the_hip_backend_and_a_gpu():
    from dimx import lib, metrics, x_engine_pt
    for backend in ("reference", "device"):
        with pytest.raises(ValueError):
            x_engine_pt.evaluate_test_epoch(stub_model.StubSLMFT(), stub_model.protocol_batches(), torch.device("cpu"), beam_size=10,
                                            fd_backend=backend, metrics=metrics.ListenerMetrics())
    with pytest.raises(lib.DimxError):
        x_engine_pt.evaluate_test_epoch(stub_model.StubSLMFT(), stub_model.protocol_batches(), torch.device("cpu"), beam_size=10,
                                        fd_backend="hip", metrics=metrics.ListenerMetrics())


def test_hip_metrics_example_driver_compiles():
    import py_compile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(root, "examples", "eval_s2s_pretrain_hip.py")
    py_compile.compile(path, doraise=True)      # what tests/test_host_io.py does for the reference's driver
