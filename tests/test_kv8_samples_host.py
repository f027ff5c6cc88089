"""CPU: the definition of the multi-query cross attention over FP8 codes (dimx/kv8.py attention_rows, round_bf16, pv_abs) against a
direct float64 restatement, the C-ABI's new symbols, the module layers' refusals, and the margins of the free-running best-of-4
case tests/test_gpu_kv8_samples.py compares tokens on."""
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
SAMPLES_SEED = 9              # the free-running GPU case's inputs; chosen here, on the CPU: with it the margins below hold
SAMPLES = 4                   # samples per clip of that case


def sample_noise(B, T, S):
    from dimx import prng
    return torch.from_numpy(prng.exponential(14, "kv8_samples.noise", (T - 1, B * S, 512)))


def _operands(g, B, H, Tp, n):
    kc, ks = kv8.quantize(g.standard_normal((B, H, Tp, 64)).astype(np.float32))
    vc, vs = kv8.quantize(g.standard_normal((B, H, Tp, 64)).astype(np.float32))
    kc[:, :, n:], vc[:, :, n:], ks[:, :, n:], vs[:, :, n:] = 0x7F, 0x7F, np.nan, np.nan     # rows at and past n are not read
    return kc, ks, vc, vs


@pytest.mark.parametrize("masked", [False, True])
def test_attention_rows_is_a_float64_softmax_per_row_over_the_rows_clip(masked):
    g = np.random.default_rng(31 + masked)
    B, H, Tp, n, S = 2, 3, 24, 19, 5
    kc, ks, vc, vs = _operands(g, B, H, Tp, n)
    q = g.standard_normal((B * S, H, 64)).astype(np.float32)
    mask = None
    if masked:
        mask = (g.random((B, Tp)) > 0.4).astype(np.uint8)
        mask[1, :] = 0            # clip 1: every key masked -> the mean of V over the keys
        mask[:, n:] = 7
    out = kv8.attention_rows(q, kc, ks, vc, vs, mask, n, S, 0.125)
    A = kv8.pv_abs(q, kc, ks, vc, vs, mask, n, S, 0.125)
    assert out.dtype == np.float64 and out.shape == A.shape == (B * S, H, 64)
    for r in range(B * S):
        b = r // S
        k = (kv8.decode(kc[b, :, :n]) * ks[b, :, :n, None]).astype(np.float64)     # the dequantised row is the float32 product
        v = (kv8.decode(vc[b, :, :n]) * vs[b, :, :n, None]).astype(np.float64)
        s = torch.einsum("hd,hjd->hj", torch.from_numpy(q[r]).double(), torch.from_numpy(k)) * 0.125
        if masked:
            s = s.masked_fill(torch.from_numpy(mask[b, :n] == 0)[None, :], kv8.NEG)
        p = s.softmax(-1)
        ref = torch.einsum("hj,hjd->hd", p, torch.from_numpy(v)).numpy()
        assert np.abs(out[r] - ref).max() < 1e-12, r
        assert np.abs(A[r] - torch.einsum("hj,hjd->hd", p, torch.from_numpy(np.abs(v))).numpy()).max() < 1e-12, r
        assert (np.abs(out[r]) <= A[r] + 1e-15).all()
    if masked:
        mean_v = (kv8.decode(vc[1, :, :n]) * vs[1, :, :n, None]).astype(np.float64).mean(1)
        assert np.abs(out[S:] - mean_v[None]).max() < 1e-12
    # row b*S+s depends on clip b's operands alone: other codes for clip 1 leave clip 0's rows bit for bit, and change clip 1's
    kc2, ks2, vc2, vs2 = (a.copy() for a in (kc, ks, vc, vs))
    kc2[1, :, :n], ks2[1, :, :n], vc2[1, :, :n], vs2[1, :, :n] = kc[0, :, :n], ks[0, :, :n], vc[0, :, :n], vs[0, :, :n]
    mask2 = None if mask is None else np.concatenate([mask[:1], np.ones_like(mask[:1])])
    out2 = kv8.attention_rows(q, kc2, ks2, vc2, vs2, mask2, n, S, 0.125)
    assert np.array_equal(out2[:S], out[:S]) and (np.abs(out2[S:] - out[S:]).max(-1) > 1e-3).all()
    # ... and it is not the per-clip form with the rows dealt out the other way (row s*B+b)
    wrong = kv8.attention(q, np.tile(kc, (S, 1, 1, 1)), np.tile(ks, (S, 1, 1)), np.tile(vc, (S, 1, 1, 1)), np.tile(vs, (S, 1, 1)),
                          None if mask is None else np.tile(mask, (S, 1)), n, 0.125)
    assert np.abs(wrong - out).max() > 1e-3


def test_round_bf16_is_torchs_round_to_nearest_even():
    g = np.random.default_rng(5)
    x = np.concatenate([g.standard_normal(4096).astype(np.float32) * np.float32(2.0) ** g.integers(-20, 20, 4096).astype(np.float32),
                        np.array([0.0, -0.0, 1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -(1.0 + 2.0 ** -8)], dtype=np.float32)])
    want = torch.from_numpy(x).to(torch.bfloat16).float().numpy()
    got = kv8.round_bf16(x)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert kv8.round_bf16(x[:4096].reshape(-1, 8)).shape == (512, 8)
    assert kv8.round_bf16(np.float32(1.0 + 2.0 ** -8)) == 1.0 and kv8.round_bf16(np.float32(1.0 + 3 * 2.0 ** -8)) == np.float32(1.0 + 2.0 ** -6)


NEW = {"dimx_op_decode_attn_kv8_multi": 26, "dimx_set_cross_kv8_samples": 2, "dimx_cross_kv8_samples": 2}


def test_symbols_are_declared_exported_and_refuse_bad_arguments_without_a_gpu():
    hdr = open(os.path.join(ROOT, "include", "dimx.h")).read()
    l = lib.load()
    for name, nargs in NEW.items():
        m = re.search(r"\bint %s\(([^;]*)\);" % name, hdr)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(lib.SIGNATURES[name][1]), name
        assert hasattr(l, name)
    assert l.dimx_set_cross_kv8_samples(None, 1) == -1 and l.dimx_cross_kv8_samples(None, None) == -1

    def op(q=None, rpc=4, n=3, Tmax=8, win=0, exact=0):
        return l.dimx_op_decode_attn_kv8_multi(lib.F32, q, 64, 1, 1, 0, None, None, None, None, None, 64, 1, 1, Tmax, None, n, None, 0, rpc, 0.125, 0, 0,
                                               win, exact, None)
    assert op() == -1 and b"null" in l.dimx_last_error()
    assert op(q=4096) == -1 and b"null" in l.dimx_last_error()
    assert op(win=1) == -1 and b"step counter" in l.dimx_last_error()
    # the one-query operator keeps its refusal
    assert l.dimx_op_decode_attn_kv8(lib.F32, 4096, 64, 1, 1, 0, 4096, 4096, 4096, 4096, 4096, 64, 1, 1, 8, None, 3, None, 0, 2, 0.125, 0, 0, 0, None) == -1
    assert b"row per clip" in l.dimx_last_error()


def test_module_layers_take_kv8_samples_and_refuse_beam_search_and_guidance():
    import stub_model
    from dimx import x_engine_pt
    from dimx.seq2seq_pretrain import SLMFT
    ev = lambda **kw: x_engine_pt.evaluate_test_epoch(stub_model.StubSLMFT(), stub_model.protocol_batches(), torch.device("cpu"), beam_size=2,
                                                      kv8_samples=True, **kw)
    for kw in ({"decode": "beam", "beam_width": 2}, {"guidance": 1.5}):
        with pytest.raises(ValueError, match="kv8_samples"):
            ev(**kw)
    # the batched best-of-N pass stays, with every select (the two that need no ground truth select on the GPU: past the argument
    # checks, a CPU device is what they refuse) and with self_kv8 on top
    assert len(ev()) == 4 and len(ev(self_kv8=True)) == 4
    for select in ("likelihood", "consensus"):
        with pytest.raises(lib.DimxError, match="ROCm GPU"):
            ev(select=select)
    # kv8 alone stays one sample per clip with select='fd'
    with pytest.raises(ValueError):
        x_engine_pt.evaluate_test_epoch(stub_model.StubSLMFT(), stub_model.protocol_batches(), torch.device("cpu"), beam_size=2, kv8=True,
                                        select="likelihood")
    model = SLMFT().eval()
    B, T = 2, 8
    args = (torch.zeros(B, T, 56), torch.zeros(B, T, 56), torch.zeros(B, T, 768), torch.ones(B, T, dtype=torch.bool))
    for kw in ({"mode": "train"}, {"mode": "val", "beam_width": 2}, {"mode": "val", "guidance": 1.5}):
        with pytest.raises(ValueError, match="kv8_samples"):
            model(*args, kv8_samples=True, **kw)
        with pytest.raises(ValueError, match="kv8_samples"):
            model.forward_decoder(None, torch.zeros(B, T, dtype=torch.long), args[2], args[3], kw["mode"], v_speaker=args[0], kv8_samples=True,
                                  beam_width=kw.get("beam_width", 0), guidance=kw.get("guidance"), n_samples=kw.get("beam_width", 1))


@pytest.fixture(scope="module")
def case(full_sd):
    import kv8_ref
    import prompt_ref
    B, T, lens = KV8_CASE
    v_s, v_a, z, mask = _case(B, T, list(lens), seed=SAMPLES_SEED)
    ctx = prompt_ref.case_context(full_sd, v_s, v_a, mask)
    cross = kv8_ref.cross_kv(full_sd, ctx)
    return {"z": z, "mask": mask, "ctx": ctx, "cross": cross, "cross8": kv8_ref.through_kv8(cross), "noise": sample_noise(B, T, SAMPLES), "T": T}


@pytest.mark.parametrize("noisy", [False, True])
def test_fixture_margins_cover_the_free_running_gpu_test(full_sd, case, noisy):
    """the checker alone, SAMPLES samples per clip over the checker's own cross K / V through the quantiser"""
    import self_kv8_ref
    c, S = case, SAMPLES
    run = lambda kv: self_kv8_ref.self_kv8_generate(full_sd, c["z"][:, :1], None, c["T"] - 1, c["ctx"], c["mask"], None, self_kv8_ref.SelfRows(),
                                                    c["noise"] if noisy else None, cross_kv=kv, samples=S)
    tok, lg, margins = run(c["cross8"])
    ptok, plg, _ = run(c["cross"])
    left_out = (margins < MARGIN).float().mean().item()
    print("noisy=%d, %d samples: smallest margin %.3e, (row, step) pairs below MARGIN %.4f; quantised against plain cross rows: first-step "
          "logits differ by %.3e, %.0f %% of the tokens equal" % (noisy, S, margins.min().item(), left_out, (lg[:, 0] - plg[:, 0]).abs().max().item(),
                                                                  100 * (tok == ptok).float().mean().item()))
    assert tuple(tok.shape) == (KV8_CASE[0] * S, c["T"] - 1)
    assert left_out <= MAX_LEFT_OUT
    assert (lg[:, 0] - plg[:, 0]).abs().max().item() > 0      # the quantised rows were read
    if noisy:
        assert not torch.equal(tok[0], tok[1])                # the samples of a clip are different sequences
