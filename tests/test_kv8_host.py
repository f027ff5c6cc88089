"""CPU: the definition of FP8 cross K/V (dimx/kv8.py) against torch's CPU float8_e4m3fn cast, its attention against a float64 softmax,
the C-ABI's new symbols, and the margins of the generation case tests/test_gpu_kv8.py compares tokens on."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from dimx import kv8, lib
from test_gpu_prompt import LOGIT_TOL, _case, _noise

torch.set_grad_enabled(False)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 2 * LOGIT_TOL        # the suite's near-tie bound (tests/test_online_host.py, tests/test_gpu_online.py)
MAX_LEFT_OUT = 0.10           # the share of (clip, step) pairs the free-running GPU test may leave out
KV8_CASE = (3, 40, (40, 33, 17))
KV8_SEED = 9                  # chosen here, on the CPU: with it the margins below hold (printed by the test)
FINITE = [c for c in range(256) if c & 0x7F != 0x7F]


def _torch_codes(y):
    return torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def _unit_rows(vals):
    """rows [n, 64] with amax = 448 exactly (scale = 1): element 0 is 448, the values fill the rest, 63 per row"""
    vals = np.asarray(vals, dtype=np.float32)
    n = (len(vals) + 62) // 63
    body = np.zeros(n * 63, dtype=np.float32)
    body[:len(vals)] = vals
    return np.concatenate([np.full((n, 1), 448.0, dtype=np.float32), body.reshape(n, 63)], axis=1)


def test_decode_table_is_torchs():
    t = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float().numpy()
    assert np.array_equal(t[FINITE], kv8.DECODE[FINITE])
    assert np.isnan(kv8.DECODE[0x7F]) and np.isnan(kv8.DECODE[0xFF])
    assert kv8.DECODE[0x7E] == 448.0 and kv8.DECODE[0x01] == 2.0 ** -9 and kv8.DECODE[0x08] == 2.0 ** -6


def test_every_code_point_round_trips():
    vals = kv8.DECODE[FINITE]
    rows = _unit_rows(vals)
    codes, scale = kv8.quantize(rows)
    assert np.array_equal(scale, np.ones(len(rows), dtype=np.float32))
    got = codes[:, 1:].reshape(-1)[:len(vals)]
    assert kv8.same_codes(got, np.array(FINITE, dtype=np.uint8)).all()
    assert np.array_equal(got[vals != 0], np.array(FINITE, dtype=np.uint8)[vals != 0])
    assert np.array_equal(kv8.dequantize(codes, scale), rows)
    assert kv8.same_codes(codes, _torch_codes(rows)).all()


def tie_values():
    """every midpoint between neighbouring code points (both signs), values just beside them, the subnormal range, 2**-10 (ties to
    zero) and values below it, +-448"""
    pos = kv8.DECODE[:0x7F].astype(np.float64)
    mid = ((pos[:-1] + pos[1:]) / 2).astype(np.float32)           # exact in float32
    assert np.array_equal(mid.astype(np.float64), (pos[:-1] + pos[1:]) / 2)
    eps = np.float32(2.0 ** -24)
    tail = [2.0 ** -10, -2.0 ** -10, 2.0 ** -10 * 1.0001, 2.0 ** -11, 2.0 ** -20, -2.0 ** -30, 3 * 2.0 ** -10, 5 * 2.0 ** -10, 2.0 ** -9, 2.0 ** -6,
            448.0, -448.0, 447.9, 432.0, 1e-38, 0.0, -0.0]
    return np.concatenate([mid, -mid, mid * (1 + eps * 2), mid * (1 - eps), tail]).astype(np.float32), mid


def test_midpoints_tie_to_even_and_subnormals_round_like_torch():
    vals, mid = tie_values()
    rows = _unit_rows(vals)
    codes, scale = kv8.quantize(rows)
    assert (scale == 1).all()
    want = _torch_codes(rows)
    assert kv8.same_codes(codes, want).all(), np.argwhere(~kv8.same_codes(codes, want))
    got = codes[:, 1:].reshape(-1)[:len(vals)]
    n = len(mid)
    lower = np.arange(0x7E, dtype=np.uint8)
    even = np.where(lower % 2 == 0, lower, lower + 1)            # the midpoint of codes c, c + 1 goes to the even one
    assert np.array_equal(got[:n], even) and np.array_equal(got[n:2 * n][1:], even[1:] | 0x80)
    assert got[2 * n + 2 * n] & 0x7F == 0 and got[2 * n + 2 * n + 1] & 0x7F == 0       # +-2**-10 ties to zero
    assert got[4 * n + 2] == 1 and got[4 * n + 3] == 0 and got[4 * n + 4] == 0   # just above 2**-10 -> 2**-9; below -> 0


def test_zero_rows_and_the_scale_arithmetic():
    g = np.random.default_rng(3)
    rows = g.standard_normal((6, 64)).astype(np.float32)
    rows[1] = 0.0
    rows[2] = 0.0
    rows[2, 5] = 2.0 ** -70
    rows[3] *= 2.0 ** -58
    codes, scale = kv8.quantize(rows)
    assert scale[1] == 0 and scale[2] == 0 and not codes[1].any() and not codes[2].any()
    assert np.array_equal(kv8.dequantize(codes[1:3], scale[1:3]), np.zeros((2, 64), np.float32))
    amax = np.abs(rows).max(-1)
    for r in (0, 3, 4, 5):
        assert scale[r] == np.float32(amax[r]) / np.float32(448.0) and scale[r].dtype == np.float32
        y = np.clip((rows[r] / scale[r]).astype(np.float32), -448, 448)
        assert kv8.same_codes(codes[r], _torch_codes(y)).all()
        assert (codes[r] & 0x7F).max() == 0x7E                      # the row's largest element maps to +-448
    err = np.abs(kv8.dequantize(codes, scale) - rows).max(-1)
    assert (err[[0, 4, 5]] <= amax[[0, 4, 5]] / 16 + 1e-12).all()   # half a step of the top binade: 16 / 448 of amax... at most amax / 16


def test_rows_scaled_by_powers_of_two_get_their_own_scale():
    g = np.random.default_rng(5)
    base = g.standard_normal(64).astype(np.float32)
    ks = np.arange(-6, 7)
    rows = np.stack([base * np.float32(2.0 ** k) for k in ks])
    codes, scale = kv8.quantize(rows)
    assert np.array_equal(scale, scale[6] * (2.0 ** ks).astype(np.float32)) and len(set(scale.tolist())) == 13
    assert all(np.array_equal(codes[i], codes[6]) for i in range(13))
    assert np.array_equal(kv8.dequantize(codes, scale), kv8.dequantize(codes[6], scale[6])[None] * (2.0 ** ks)[:, None].astype(np.float32))


def test_attention_is_a_float64_softmax_over_the_dequantised_rows():
    g = np.random.default_rng(7)
    B, H, Tp, n = 4, 2, 24, 19
    q = g.standard_normal((B, H, 64)).astype(np.float32)
    kc, ks = kv8.quantize(g.standard_normal((B, H, Tp, 64)).astype(np.float32) * 2.0 ** g.integers(-3, 4, (B, H, Tp, 1)))
    vc, vs = kv8.quantize(g.standard_normal((B, H, Tp, 64)).astype(np.float32))
    mask = (g.random((B, Tp)) > 0.4).astype(np.uint8)
    mask[1] = 0              # every key masked: the mean of V over the n keys
    mask[2, :n] = 0
    mask[2, n - 1] = 1
    k = torch.from_numpy(kv8.dequantize(kc, ks)).double()[:, :, :n]
    v = torch.from_numpy(kv8.dequantize(vc, vs)).double()[:, :, :n]
    for m in (None, mask):
        s = torch.einsum("bhd,bhjd->bhj", torch.from_numpy(q).double(), k) * 0.125
        if m is not None:
            s = s.masked_fill(torch.from_numpy(m)[:, None, :n] == 0, -torch.finfo(torch.float32).max)
        ref = torch.einsum("bhj,bhjd->bhd", s.softmax(-1), v).numpy()
        out = kv8.attention(q, kc, ks, vc, vs, m, n)
        assert out.dtype == np.float64 and np.abs(out - ref).max() < 1e-12
    out = kv8.attention(q, kc, ks, vc, vs, mask, n)
    assert np.abs(out[1] - v[1].mean(1).numpy()).max() < 1e-12
    assert np.abs(out[2] - v[2][:, n - 1].numpy()).max() < 1e-12


def test_buffer_layout_is_the_headers():
    lay, total = kv8.buffer_layout(4, 3, 12, 40)
    cb, sb = (3 * 12 * 40 * 64 + 255) // 256 * 256, (3 * 12 * 40 * 4 + 255) // 256 * 256
    assert total == 4 * 2 * (cb + sb)
    assert lay[0] == {"kcodes": 0, "vcodes": cb, "kscale": 2 * cb, "vscale": 2 * cb + sb}
    assert lay[1]["kcodes"] == 2 * (cb + sb) and all(v % 256 == 0 for o in lay for v in o.values())


NEW = {"dimx_cross_kv8_bytes": 3, "dimx_set_cross_kv8": 3, "dimx_cross_kv8": 3, "dimx_op_kv8_quantize": 9, "dimx_op_decode_attn_kv8": 25}


def test_symbols_are_declared_exported_and_refuse_bad_arguments_without_a_gpu():
    hdr = open(os.path.join(ROOT, "include", "dimx.h")).read()
    l = lib.load()
    for name, nargs in NEW.items():
        m = re.search(r"\b(?:int|size_t) %s\(([^;]*)\);" % name, hdr)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(lib.SIGNATURES[name][1]), name
        assert hasattr(l, name)
    assert lib.SIGNATURES["dimx_cross_kv8_bytes"][0] is ctypes.c_size_t
    assert l.dimx_cross_kv8_bytes(None, 3, 40) == 0
    assert l.dimx_set_cross_kv8(None, None, 0) == -1 and l.dimx_cross_kv8(None, None, None) == -1
    assert l.dimx_op_kv8_quantize(lib.F32, None, 1, 1, 8, 8, None, None, None) == -1
    assert b"null" in l.dimx_last_error()
    assert l.dimx_op_decode_attn_kv8(lib.F32, None, 64, 1, 1, 0, None, None, None, None, None, 64, 1, 1, 8, None, 8, None, 0, 1, 0.125, 0, 0, 0,
                                     None) == -1
    # more than one row per clip and a windowed call without a step counter are refused before the operands are looked at
    assert l.dimx_op_decode_attn_kv8(lib.F32, None, 64, 1, 1, 0, None, None, None, None, None, 64, 1, 1, 8, None, 8, None, 0, 2, 0.125, 0, 0, 0,
                                     None) == -1 and b"row per clip" in l.dimx_last_error()
    assert l.dimx_op_decode_attn_kv8(lib.F32, None, 64, 1, 1, 0, None, None, None, None, None, 64, 1, 1, 8, None, 8, None, 0, 1, 0.125, 0, 0, 1,
                                     None) == -1 and b"step counter" in l.dimx_last_error()


def test_module_layers_refuse_what_kv8_does_not_take():
    import stub_model
    from dimx import x_engine_pt
    for kw in ({"decode": "beam", "beam_width": 2}, {"select": "likelihood"}):
        with pytest.raises(ValueError):
            x_engine_pt.evaluate_test_epoch(stub_model.StubSLMFT(), stub_model.protocol_batches(), torch.device("cpu"), beam_size=2, kv8=True, **kw)


@pytest.fixture(scope="module")
def case(full_sd):
    import kv8_ref
    import prompt_ref
    B, T, lens = KV8_CASE
    v_s, v_a, z, mask = _case(B, T, list(lens), seed=KV8_SEED)
    ctx = prompt_ref.case_context(full_sd, v_s, v_a, mask)
    kv = kv8_ref.cross_kv(full_sd, ctx)
    return {"z": z, "mask": mask, "ctx": ctx, "kv": kv, "kv8": kv8_ref.through_kv8(kv), "noise": _noise(B, T), "T": T}


def test_checker_with_the_plain_rows_is_the_online_checker(full_sd, case):
    import kv8_ref
    import online_ref
    c = case
    a = kv8_ref.kv8_generate(full_sd, c["z"][:, :1], None, 6, c["ctx"], c["mask"], 0, c["kv"])
    b = online_ref.online_generate(full_sd, c["z"][:, :1], None, 6, c["ctx"], c["mask"], 0)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("noisy", [False, True])
def test_fixture_margins_cover_the_free_running_gpu_test(full_sd, case, noisy):
    import kv8_ref
    import online_ref
    c = case
    tok, lg, margins = kv8_ref.kv8_generate(full_sd, c["z"][:, :1], None, c["T"] - 1, c["ctx"], c["mask"], None, c["kv8"],
                                            c["noise"] if noisy else None)
    ptok, plg, _ = kv8_ref.kv8_generate(full_sd, c["z"][:, :1], None, c["T"] - 1, c["ctx"], c["mask"], None, c["kv"],
                                        c["noise"] if noisy else None)
    _, left_out = online_ref.compared_steps(margins, MARGIN)
    print("noisy=%d: smallest margin %.3e, pairs below MARGIN's first hit left out %.4f; kv8 against plain rows: first-step logits "
          "differ by %.3e, %.0f %% of the tokens equal" % (noisy, margins.min().item(), left_out, (lg[:, 0] - plg[:, 0]).abs().max().item(),
                                                            100 * (tok == ptok).float().mean().item()))
    assert left_out <= MAX_LEFT_OUT
