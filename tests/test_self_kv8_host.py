"""CPU: the definition of the self-attention step over FP8 self K/V caches (dimx/kv8.py self_step) against a direct float64
restatement, the C-ABI's new symbols, the module layers' refusals, the checker of tests/self_kv8_ref.py against online_ref with
quantisation switched off, and the margins of the free-running case tests/test_gpu_self_kv8.py compares tokens on."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from dimx import kv8, lib
from test_gpu_prompt import _case
from test_kv8_host import KV8_CASE, MARGIN, MAX_LEFT_OUT

torch.set_grad_enabled(False)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SELF_SEED = 9                 # the free-running GPU case's inputs; chosen here, on the CPU: with it the margins below hold
# samples per clip of that case.  The library generates 1, 2, 4, 5, 8 or 10 samples per clip (dimx_generate refuses every other
# count, 3 included, with or without FP8 caches): 4 is the smallest count it takes that is not below the 3 the case was specified with.
SELF_SAMPLES = 4
# what the device quantises on that case: the first layer reads its K / V from the token table (no prompt), the others from codes
FREE_QUANT_LAYERS = (1, 2, 3)


def sample_noise(B, T, S):
    from dimx import prng
    return torch.from_numpy(prng.exponential(13, "self_kv8.noise", (T - 1, B * S, 512)))


@pytest.mark.parametrize("n", [0, 1, 18])
def test_self_step_is_a_float64_softmax_over_the_dequantised_rows_its_own_included(n):
    g = np.random.default_rng(11 + n)
    R, H, Tp = 4, 2, 24
    q, k_new, v_new = (g.standard_normal((R, H, 64)).astype(np.float32) for _ in range(3))
    k_new *= (2.0 ** g.integers(-3, 4, (R, H, 1))).astype(np.float32)
    kc, ks = kv8.quantize(g.standard_normal((R, H, Tp, 64)).astype(np.float32))
    vc, vs = kv8.quantize(g.standard_normal((R, H, Tp, 64)).astype(np.float32))
    kc[:, :, n:], vc[:, :, n:], ks[:, :, n:], vs[:, :, n:] = 0x7F, 0x7F, np.nan, np.nan     # rows at and past n are not read
    before = [a.copy() for a in (kc, ks, vc, vs)]
    out = kv8.self_step(q, k_new, v_new, kc, ks, vc, vs, n, 0.125)
    # the restatement: rows 0 .. n - 1 as they were, row n = the new rows through the quantiser, one float64 softmax over n + 1 keys
    qk, qks = kv8.quantize(k_new)
    qv, qvs = kv8.quantize(v_new)
    k = np.concatenate([kv8.dequantize(before[0][:, :, :n], before[1][:, :, :n]), kv8.dequantize(qk, qks)[:, :, None]], 2).astype(np.float64)
    v = np.concatenate([kv8.dequantize(before[2][:, :, :n], before[3][:, :, :n]), kv8.dequantize(qv, qvs)[:, :, None]], 2).astype(np.float64)
    s = torch.einsum("bhd,bhjd->bhj", torch.from_numpy(q).double(), torch.from_numpy(k)) * 0.125
    ref = torch.einsum("bhj,bhjd->bhd", s.softmax(-1), torch.from_numpy(v)).numpy()
    assert out.dtype == np.float64 and out.shape == (R, H, 64) and np.abs(out - ref).max() < 1e-12
    # row n holds the quantised new rows, every other row is untouched
    assert np.array_equal(kc[:, :, n], qk) and np.array_equal(vc[:, :, n], qv)
    assert np.array_equal(ks[:, :, n].view(np.int32), qks.view(np.int32)) and np.array_equal(vs[:, :, n].view(np.int32), qvs.view(np.int32))
    for a, b in zip((kc, ks, vc, vs), before):
        keep = np.arange(Tp) != n
        assert np.ascontiguousarray(a[:, :, keep]).tobytes() == np.ascontiguousarray(b[:, :, keep]).tobytes()
    # the own key is the dequantised one, not k_new itself: the plain own key gives another answer
    if n > 0:
        k[:, :, n] = k_new
        s2 = torch.einsum("bhd,bhjd->bhj", torch.from_numpy(q).double(), torch.from_numpy(k)) * 0.125
        assert np.abs(torch.einsum("bhj,bhjd->bhd", s2.softmax(-1), torch.from_numpy(v)).numpy() - out).max() > 1e-6
    else:
        assert np.abs(out - kv8.dequantize(qv, qvs)).max() < 1e-12      # one key: the output is its value


NEW = {"dimx_self_kv8_bytes": 3, "dimx_set_self_kv8": 3, "dimx_self_kv8": 3, "dimx_op_decode_attn_self_kv8": 19}


def test_symbols_are_declared_exported_and_refuse_bad_arguments_without_a_gpu():
    hdr = open(os.path.join(ROOT, "include", "dimx.h")).read()
    l = lib.load()
    for name, nargs in NEW.items():
        m = re.search(r"\b(?:int|size_t) %s\(([^;]*)\);" % name, hdr)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(lib.SIGNATURES[name][1]), name
        assert hasattr(l, name)
    assert lib.SIGNATURES["dimx_self_kv8_bytes"][0] is ctypes.c_size_t
    assert l.dimx_self_kv8_bytes(None, 9, 40) == 0
    assert l.dimx_set_self_kv8(None, None, 0) == -1 and l.dimx_self_kv8(None, None, None) == -1

    def op(qkv=None, ld=192, nslab=1, n=3, Tmax=8, dt=lib.F32):
        return l.dimx_op_decode_attn_self_kv8(dt, qkv, ld, nslab, 0, None, None, None, None, None, 64, 1, 1, Tmax, None, n, 0.125, 0, None)
    assert op() == -1 and b"null" in l.dimx_last_error()
    assert op(qkv=4096, ld=128) == -1 and b"q | k | v" in l.dimx_last_error()      # refused before the operands are looked at
    assert op(qkv=4096) == -1 and b"null" in l.dimx_last_error()


def test_module_layers_refuse_what_self_kv8_does_not_take():
    import stub_model
    from dimx import x_engine_pt
    from dimx.seq2seq_pretrain import SLMFT
    for kw in ({"decode": "beam", "beam_width": 2}, {"guidance": 1.5}):
        with pytest.raises(ValueError):
            x_engine_pt.evaluate_test_epoch(stub_model.StubSLMFT(), stub_model.protocol_batches(), torch.device("cpu"), beam_size=2, self_kv8=True, **kw)
    # the batched best-of-N pass takes it with every sample count
    out = x_engine_pt.evaluate_test_epoch(stub_model.StubSLMFT(), stub_model.protocol_batches(), torch.device("cpu"), beam_size=2, self_kv8=True)
    assert len(out) == 4
    model = SLMFT().eval()
    B, T = 2, 8
    args = (torch.zeros(B, T, 56), torch.zeros(B, T, 56), torch.zeros(B, T, 768), torch.ones(B, T, dtype=torch.bool))
    for kw in ({"mode": "train"}, {"mode": "val", "beam_width": 2}, {"mode": "val", "guidance": 1.5}):
        with pytest.raises(ValueError, match="self_kv8"):
            model(*args, self_kv8=True, **kw)
        with pytest.raises(ValueError, match="self_kv8"):
            model.forward_decoder(None, torch.zeros(B, T, dtype=torch.long), args[2], args[3], kw["mode"], v_speaker=args[0], self_kv8=True,
                                  beam_width=kw.get("beam_width", 0), guidance=kw.get("guidance"), n_samples=kw.get("beam_width", 1))


@pytest.fixture(scope="module")
def case(full_sd):
    import prompt_ref
    B, T, lens = KV8_CASE
    v_s, v_a, z, mask = _case(B, T, list(lens), seed=SELF_SEED)
    return {"z": z, "mask": mask, "ctx": prompt_ref.case_context(full_sd, v_s, v_a, mask), "noise": sample_noise(B, T, SELF_SAMPLES), "T": T}


@pytest.mark.parametrize("lookahead", [None, 0])
def test_checker_without_quantisation_is_the_online_checker(full_sd, case, lookahead):
    import online_ref
    import self_kv8_ref
    c = case
    a = self_kv8_ref.self_kv8_generate(full_sd, c["z"][:, :3], [3, 1, 2], 6, c["ctx"], c["mask"], lookahead, self_kv8_ref.SelfRows())
    b = online_ref.online_generate(full_sd, c["z"][:, :3], [3, 1, 2], 6, c["ctx"], c["mask"], lookahead)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("noisy", [False, True])
def test_fixture_margins_cover_the_free_running_gpu_test(full_sd, case, noisy):
    import self_kv8_ref
    c, S = case, SELF_SAMPLES
    run = lambda quant: self_kv8_ref.self_kv8_generate(full_sd, c["z"][:, :1], None, c["T"] - 1, c["ctx"], c["mask"], None,
                                                       self_kv8_ref.SelfRows(quant_layers=quant), c["noise"] if noisy else None, samples=S)
    tok, lg, margins = run(FREE_QUANT_LAYERS)
    ptok, plg, _ = run(())
    left_out = (margins < MARGIN).float().mean().item()
    print("noisy=%d, %d samples: smallest margin %.3e, (row, step) pairs below MARGIN %.4f; quantised against plain self rows: first-step "
          "logits differ by %.3e, %.0f %% of the tokens equal" % (noisy, S, margins.min().item(), left_out, (lg[:, 0] - plg[:, 0]).abs().max().item(),
                                                                  100 * (tok == ptok).float().mean().item()))
    assert tuple(tok.shape) == (KV8_CASE[0] * S, c["T"] - 1)
    assert left_out <= MAX_LEFT_OUT
    assert (lg[:, 0] - plg[:, 0]).abs().max().item() > 0      # the quantised rows were read
