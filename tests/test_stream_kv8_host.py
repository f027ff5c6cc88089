"""CPU: FP8 K/V for streaming sessions (dimx_stream_set_kv8) -- the row locality of the definition (dimx/kv8.py append
against quantize under every chunking of the session suite), the C-ABI's new symbols, and the margins of the inputs
tests/test_gpu_stream_kv8.py compares free-running tokens on."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from dimx import kv8, lib
from test_gpu_prompt import _case, _noise
from test_kv8_host import MARGIN, MAX_LEFT_OUT
from test_stream_host import CHUNKINGS

torch.set_grad_enabled(False)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAM_KV8_CASE = (3, 40, 48)      # clips, frames, Tmax: the session suite's shapes, every clip of full length
STREAM_KV8_SEED = 12               # chosen here, on the CPU: with it the margins below hold (printed by the test)
LOOKAHEADS = [0, -3, 2, 40]
TABLE0_QUANT = (1, 2, 3)           # an unprompted session's first layer reads the token table: its self rows stay plain


def _u32(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _rows():
    """[2, 3, 40, 64]: rows of magnitudes 2**-8 .. 2**7, an all-zero row, a row holding +-3e4, a row below the zero threshold"""
    g = np.random.default_rng(31)
    x = g.standard_normal((2, 3, 40, 64)).astype(np.float32) * np.exp2(g.integers(-8, 8, (2, 3, 40, 1))).astype(np.float32)
    x[0, 1, 16] = 0.0
    x[1, 2, 0] = 0.0
    x[1, 0, 17, ::2] = 3e4
    x[1, 0, 17, 1::2] = -3e4
    x[0, 2, 39] *= np.float32(2.0 ** -80)
    return x


@pytest.mark.parametrize("chunking", CHUNKINGS, ids=lambda c: "x".join(map(str, c[:3])) + "_%d" % len(c))
def test_append_under_any_chunking_is_quantize_of_the_whole(chunking):
    x = _rows()
    Tp = 48
    want_c, want_s = kv8.quantize(x)
    assert want_s[0, 1, 16] == 0 and not want_c[0, 1, 16].any() and want_s[0, 2, 39] == 0
    assert want_s[1, 0, 17] == np.float32(3e4) / np.float32(448.0) and set(want_c[1, 0, 17].tolist()) == {0x7E, 0xFE}
    codes = np.full((2, 3, Tp, 64), 0xFF, dtype=np.uint8)
    scales = np.full((2, 3, Tp), np.nan, dtype=np.float32)
    n = 0
    for c in chunking:
        before = (codes, scales)
        codes, scales = kv8.append(codes, scales, x[:, :, n:n + c], n)
        assert codes is not before[0] and scales is not before[1]
        n += c
        assert (codes[:, :, n:] == 0xFF).all() and np.isnan(scales[:, :, n:]).all()       # nothing past the rows appended
    assert n == 40
    assert kv8.same_codes(codes[:, :, :40], want_c).all()
    assert np.array_equal(_u32(scales[:, :, :40]), _u32(want_s))
    with pytest.raises(AssertionError):
        kv8.append(codes, scales, x[:, :, :9], 40)


NEW = {"dimx_stream_set_kv8": 5, "dimx_stream_kv8": 5, "dimx_stream_cross_kv": 4, "dimx_op_kv8_append": 12}


def test_symbols_are_declared_exported_and_refuse_bad_arguments_without_a_gpu():
    hdr = open(os.path.join(ROOT, "include", "dimx.h")).read()
    l = lib.load()
    for name, nargs in NEW.items():
        m = re.search(r"\b(?:int|size_t) %s\(([^;]*)\);" % name, hdr)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(lib.SIGNATURES[name][1]), name
        assert hasattr(l, name)
    assert l.dimx_stream_set_kv8(None, None, 0, None, 0) == -1 and l.dimx_stream_kv8(None, None, None, None, None) == -1
    assert l.dimx_stream_cross_kv(None, 0, None, None) == -1
    null2 = (ctypes.c_void_p * 2)()
    assert l.dimx_op_kv8_append(lib.F32, None, None, None, 1, 1, 1, 8, 8, 0, 1, None) == -1 and b"null" in l.dimx_last_error()
    assert l.dimx_op_kv8_append(lib.F32, null2, null2, null2, 1, 1, 1, 8, 8, 0, 1, None) == -1 and b"null" in l.dimx_last_error()
    for depth in (0, 9):
        assert l.dimx_op_kv8_append(lib.F32, null2, null2, null2, depth, 1, 1, 8, 8, 0, 1, None) == -1 and b"depth" in l.dimx_last_error()


@pytest.fixture(scope="module")
def case(full_sd):
    import kv8_ref
    import prompt_ref
    B, T, _ = STREAM_KV8_CASE
    v_s, v_a, z, mask = _case(B, T, [T] * B, seed=STREAM_KV8_SEED)
    ctx = prompt_ref.case_context(full_sd, v_s, v_a, mask)
    kv = kv8_ref.cross_kv(full_sd, ctx)
    return {"z": z, "mask": mask, "ctx": ctx, "kv": kv, "kv8": kv8_ref.through_kv8(kv), "noise": _noise(B, T), "T": T}


@pytest.mark.parametrize("noisy", [False, True])
@pytest.mark.parametrize("L", LOOKAHEADS)
def test_fixture_margins_cover_the_free_running_gpu_test(full_sd, case, L, noisy):
    """the cap on the pairs left out is a condition on the inputs: it is checked here, where the reference alone decides it"""
    import kv8_ref
    import online_ref
    import self_kv8_ref
    c = case
    n = c["T"] - 1
    nz = c["noise"] if noisy else None
    runs = {"cross": kv8_ref.kv8_generate(full_sd, c["z"][:, :1], None, n, c["ctx"], c["mask"], L, c["kv8"], nz),
            "self": self_kv8_ref.self_kv8_generate(full_sd, c["z"][:, :1], None, n, c["ctx"], c["mask"], L,
                                                   self_kv8_ref.SelfRows(quant_layers=TABLE0_QUANT), nz, cross_kv=c["kv"]),
            "both": self_kv8_ref.self_kv8_generate(full_sd, c["z"][:, :1], None, n, c["ctx"], c["mask"], L,
                                                   self_kv8_ref.SelfRows(quant_layers=TABLE0_QUANT), nz, cross_kv=c["kv8"])}
    for what, (tok, lg, margins) in runs.items():
        _, left_out = online_ref.compared_steps(margins, MARGIN)
        print("L=%d noisy=%d %s: smallest margin %.3e, pairs left out %.4f" % (L, noisy, what, margins.min().item(), left_out))
        assert left_out <= MAX_LEFT_OUT, what
