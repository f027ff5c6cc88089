"""GPU: the first decoder layer's q/k/v from a table over the 512 token ids (csrc/generate.hip qkv0_table_build) against the
projection GEMM per token that it replaces (DIMX_NO_QKV0_TABLE=1).  The SLMFT decoder has no positional embedding, so layer 0's
input is LayerNorm(token_emb[tok]); the table is built with the decode step's own kernels at the step's row count, hence
"equal" below is torch.equal on the tokens AND on the per-step logits, greedy and sampled with injected noise, in both modes."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def _case(B, T, lens, seed=3):
    from dimx import prng
    v_s = torch.from_numpy(prng.normal(seed, "s2s.vs", (B, T, 56)))
    v_a = torch.from_numpy(prng.normal(seed, "s2s.va", (B, T, 768)))
    z = torch.from_numpy(prng.integers(seed, "s2s.z", (B, T), 0, 512))
    mask = torch.zeros(B, T, dtype=torch.bool)
    for j, n in enumerate(lens):
        mask[j, :n] = True
    z = torch.where(mask, z, torch.full_like(z, -100))
    return v_s, v_a, z, mask


def _engine(mode, table, variant="slmft"):
    """the switch is read when the handle is created"""
    from dimx import engine
    if not table:
        os.environ["DIMX_NO_QKV0_TABLE"] = "1"
    try:
        return engine.Engine("cuda:0", mode, variant)
    finally:
        os.environ.pop("DIMX_NO_QKV0_TABLE", None)


def _run(sd, mode, table, v_s, v_a, start, mask, T, S=1, noise_seed=5):
    """greedy and sampled generation of one engine: (tokens, logits) of each, the build count, the chain faults"""
    e = _engine(mode, table)
    e.load_state_dict(sd)
    m8 = mask.to(torch.uint8).cuda()
    B = start.shape[0]
    noise = torch.empty(T - 1, B * S, 512).exponential_(generator=torch.Generator().manual_seed(noise_seed)).cuda()
    out = []
    for temp, nz in ((0.0, None), (1.0, noise)):
        e.encode_ctx(v_s.cuda(), v_a.cuda(), m8, True, n_samples=S)
        tok, lg = e.generate(start.cuda(), m8, T, temp, 52, nz, return_logits=True, n_samples=S)
        out.append((tok.cpu(), lg.cpu()))
    builds, faults = e.qkv0_table_builds(), e.chain_faults()
    e.close()
    return out, builds, faults


def _compare(sd, mode, B, T, lens, S=1, seed=3, start_fix=None, builds=1):
    v_s, v_a, z, mask = _case(B, T, lens, seed=seed)
    start = z[:, 0].clone()
    if start_fix is not None:
        start_fix(start)
    on, b_on, f_on = _run(sd, mode, True, v_s, v_a, start, mask, T, S)
    off, b_off, f_off = _run(sd, mode, False, v_s, v_a, start, mask, T, S)
    assert b_on == builds and b_off == 0, "table builds: %d with the table, %d without" % (b_on, b_off)
    assert f_on == 0 and f_off == 0
    for (t1, l1), (t0, l0), what in zip(on, off, ("greedy", "sampled")):
        assert t1.shape == (B * S, T - 1)
        assert torch.equal(t1, t0), "%s tokens differ in %d places" % (what, (t1 != t0).sum())
        assert torch.equal(l1, l0), "%s logits differ by %g" % (what, (l1 - l0).abs().max())
    return on


def test_bf16_chain_path_ragged_and_clamped_start(full_sd):
    """B = 6: the chain kernels without the layer kernel; one clip starts from -100, which both paths clamp to id 0"""
    from dimx import lib

    def fix(start):
        start[4] = -100

    _compare(full_sd, lib.MODE_PERF_BF16, 6, 40, [40, 33, 7, 40, 21, 12], start_fix=fix)


def test_bf16_layer_kernel_path_three_build_rounds(full_sd):
    """B = 200: the layer kernel with a partly empty last group; the table is built in three rounds, the last one padded"""
    from dimx import lib
    B, T = 200, 48
    _compare(full_sd, lib.MODE_PERF_BF16, B, T, [T - (i * 7) % 20 for i in range(B)], seed=31)


def test_f32_parity_mode(full_sd):
    from dimx import lib
    _compare(full_sd, lib.MODE_PARITY_F32, 4, 24, [24, 24, 17, 5], seed=9)


@pytest.mark.parametrize("mode_name", ["MODE_PERF_BF16", "MODE_PARITY_F32"])
def test_several_samples_per_clip(full_sd, mode_name):
    from dimx import lib
    on = _compare(full_sd, getattr(lib, mode_name), 3, 16, [16, 11, 4], S=5, seed=23)
    assert not torch.equal(on[1][0][0], on[1][0][1])   # samples of a clip see different noise


def test_more_rows_than_tokens(full_sd):
    """520 rows per projection launch: one build round of 520 rows, ids past 511 repeat 511"""
    from dimx import lib
    _compare(full_sd, lib.MODE_PERF_BF16, 52, 8, [8 - i % 3 for i in range(52)], S=10, seed=14)


def test_cache_and_invalidation(full_sd):
    """one build per (rows, weights); new weights rebuild, and the rebuilt table is the one a fresh engine builds"""
    from dimx import lib, weights
    T = 20
    e = _engine(lib.MODE_PERF_BF16, True)
    e.load_state_dict(full_sd)

    def gen(eng, B, seed):
        v_s, v_a, z, mask = _case(B, T, [T - i for i in range(B)], seed=seed)
        m8 = mask.to(torch.uint8).cuda()
        eng.encode_ctx(v_s.cuda(), v_a.cuda(), m8, True)
        return eng.generate(z[:, 0].cuda(), m8, T, 0.0).cpu()

    assert e.qkv0_table_builds() == 0
    a = gen(e, 5, 3)
    assert e.qkv0_table_builds() == 1
    assert torch.equal(gen(e, 5, 3), a) and e.qkv0_table_builds() == 1
    gen(e, 5, 4)
    assert e.qkv0_table_builds() == 1            # other inputs, same rows: the table stays
    gen(e, 7, 3)
    assert e.qkv0_table_builds() == 2            # another row count: another split plan may apply
    other = weights.synth_state_dict(weights.slmft_spec(), 77)
    e.load_state_dict(other)
    b = gen(e, 7, 3)
    assert e.qkv0_table_builds() == 3
    fresh = _engine(lib.MODE_PERF_BF16, True)
    fresh.load_state_dict(other)
    assert torch.equal(gen(fresh, 7, 3), b) and fresh.qkv0_table_builds() == 1
    fresh.load_state_dict(full_sd)
    assert not torch.equal(gen(fresh, 7, 3), b) and fresh.qkv0_table_builds() == 2   # the weights do matter to the tokens
    e.close()
    fresh.close()


def test_legacy_decoder_keeps_the_projection():
    """ListenerGenerator's decoder input is emb + pos[t]: no table, whatever the switch says"""
    from dimx import lib, prng, weights
    sd = weights.synth_state_dict(weights.listener_generator_spec(), 20260928)
    B, T = 2, 12
    v_s = torch.from_numpy(prng.normal(5, "legacy.vs", (B, T, 824)))
    mask = torch.ones(B, T, dtype=torch.bool)
    mask[1, 9:] = False
    m8 = mask.to(torch.uint8).cuda()
    start = torch.from_numpy(prng.integers(5, "qkv0.legacy.start", (B,), 0, 512))
    noise = torch.from_numpy(prng.exponential(12, "legacy.noise", (T, B, 512))).cuda()
    outs = []
    for table in (True, False):
        e = _engine(lib.MODE_PARITY_F32, table, "legacy")
        e.load_state_dict(sd)
        for temp, nz in ((0.0, None), (1.0, noise)):
            e.encode_ctx(v_s.cuda(), None, m8, True)
            tok, lg = e.generate(start.cuda(), m8, T, temp, 52, nz, return_logits=True)
            outs.append((tok.cpu(), lg.cpu()))
        assert e.qkv0_table_builds() == 0
        e.close()
    for (t1, l1), (t0, l0) in zip(outs[:2], outs[2:]):
        assert torch.equal(t1, t0) and torch.equal(l1, l0)
