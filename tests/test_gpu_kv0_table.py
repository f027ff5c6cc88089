"""GPU: the first decoder layer's self attention reading K/V from the table over the 512 token ids (csrc/decode_attn_body.hpp,
TAB) against the per-clip cache it replaces (DIMX_NO_KV0_TABLE=1).  The SLMFT decoder has no positional embedding, so the cached
K/V of a position are columns of the q/k/v table row of that position's input token; the table form reads those rows through a
per-row token history, in the cache form's key order and arithmetic.  "Equal" below is therefore torch.equal on the tokens AND on
the per-step logits, greedy and sampled with injected noise, in both modes; kv0_table_generations() tells which form ran."""
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
        os.environ["DIMX_NO_KV0_TABLE"] = "1"
    try:
        return engine.Engine("cuda:0", mode, variant)
    finally:
        os.environ.pop("DIMX_NO_KV0_TABLE", None)


def _run(sd, mode, table, v_s, v_a, start, mask, T, S=1, noise_seed=5):
    """greedy and sampled generation of one engine: (tokens, logits) of each, the table-form generations, the chain faults"""
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
    gens, faults = e.kv0_table_generations(), e.chain_faults()
    e.close()
    return out, gens, faults


def _compare(sd, mode, B, T, lens, S=1, seed=3, start_fix=None):
    v_s, v_a, z, mask = _case(B, T, lens, seed=seed)
    start = z[:, 0].clone()
    if start_fix is not None:
        start_fix(start)
    on, g_on, f_on = _run(sd, mode, True, v_s, v_a, start, mask, T, S)
    off, g_off, f_off = _run(sd, mode, False, v_s, v_a, start, mask, T, S)
    assert g_on == 2 and g_off == 0, "table-form generations: %d with the switch on, %d with it off" % (g_on, g_off)
    assert f_on == 0 and f_off == 0
    for (t1, l1), (t0, l0), what in zip(on, off, ("greedy", "sampled")):
        assert t1.shape == (B * S, T - 1)
        assert torch.equal(t1, t0), "%s tokens differ in %d places" % (what, (t1 != t0).sum())
        assert torch.equal(l1, l0), "%s logits differ by %g" % (what, (l1 - l0).abs().max())
    return on


def test_bf16_chain_path_ragged_and_clamped_start(full_sd):
    """B = 6: decode_attn_kernel with four waves per (clip, head) beside the chain kernels; one clip starts from -100, which
    the history records as the clamped id 0"""
    from dimx import lib

    def fix(start):
        start[4] = -100

    _compare(full_sd, lib.MODE_PERF_BF16, 6, 40, [40, 33, 7, 40, 21, 12], start_fix=fix)


def test_bf16_layer_kernel_path_partly_empty_group(full_sd):
    """B = 200: the layer kernel's first-layer instantiation, the last XCD group partly empty"""
    from dimx import lib
    B, T = 200, 48
    _compare(full_sd, lib.MODE_PERF_BF16, B, T, [T - (i * 7) % 20 for i in range(B)], seed=31)


def test_bf16_layer_kernel_path_shortest_history(full_sd):
    """B = 130, T = 12: the layer kernel from step 0 (no cached key) to key counts short of one 32-key batch"""
    from dimx import lib
    B, T = 130, 12
    _compare(full_sd, lib.MODE_PERF_BF16, B, T, [T - i % 5 for i in range(B)], seed=17)


def test_f32_parity_mode_reads_the_table_and_matches_the_oracle(full_sd):
    """the f32 mode reads the K/V columns of the q/k/v table itself; its greedy tokens are the CPU oracle's"""
    from dimx import lib
    from oracle import ref_cpu
    B, T, lens = 4, 24, [24, 24, 17, 5]
    on = _compare(full_sd, lib.MODE_PARITY_F32, B, T, lens, seed=9)
    v_s, v_a, z, mask = _case(B, T, lens, seed=9)
    x_s = ref_cpu.slmft_forward_encoder(full_sd, v_s, mask)
    ctx = ref_cpu.slmft_context(full_sd, x_s, v_a)
    ref_tok = ref_cpu.ar_generate(full_sd, z[:, 0], T - 1, ctx, mask, None)
    assert torch.equal(on[0][0].long(), ref_tok.long())


@pytest.mark.parametrize("mode_name", ["MODE_PERF_BF16", "MODE_PARITY_F32"])
def test_several_samples_per_clip(full_sd, mode_name):
    """rows are samples: each has a history of its own"""
    from dimx import lib
    on = _compare(full_sd, getattr(lib, mode_name), 3, 16, [16, 11, 4], S=5, seed=23)
    assert not torch.equal(on[1][0][0], on[1][0][1])   # samples of a clip see different noise


def test_several_key_batches_and_repeated_ids(full_sd):
    """T = 80 at B = 6: up to 79 keys = several 32-key batches per wave (and per wave of a four-way split), histories in which
    token ids repeat"""
    from dimx import lib
    B, T = 6, 80
    on = _compare(full_sd, lib.MODE_PERF_BF16, B, T, [80, 80, 71, 64, 33, 80], seed=41)
    rows = torch.cat([on[0][0], on[1][0]])
    assert any(len(set(r.tolist())) < r.numel() for r in rows), "no history of this case repeats a token id"


def _gate_engines(full_sd, mode, variant="slmft", sd=None):
    es = []
    for table in (True, False):
        e = _engine(mode, table, variant)
        e.load_state_dict(full_sd if sd is None else sd)
        es.append(e)
    return es


def test_a_prefilled_prompt_keeps_the_cache(full_sd):
    from dimx import lib
    B, T, P = 3, 20, 4
    v_s, v_a, z, mask = _case(B, T, [20, 15, 9], seed=13)
    m8 = mask.to(torch.uint8).cuda()
    outs = []
    for e in _gate_engines(full_sd, lib.MODE_PERF_BF16):
        e.encode_ctx(v_s.cuda(), v_a.cuda(), m8, True, prompt_frames=P)
        tok, lg = e.generate(None, m8, T, 0.0, return_logits=True, prompt=z[:, :P].cuda(), prefill=P)
        assert e.kv0_table_generations() == 0 and e.chain_faults() == 0
        outs.append((tok.cpu(), lg.cpu()))
        e.close()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_beam_search_keeps_the_cache(full_sd):
    from dimx import lib
    B, T, W = 3, 14, 2
    v_s, v_a, z, mask = _case(B, T, [14, 10, 6], seed=19)
    m8 = mask.to(torch.uint8).cuda()
    outs = []
    for e in _gate_engines(full_sd, lib.MODE_PERF_BF16):
        e.encode_ctx(v_s.cuda(), v_a.cuda(), m8, True, n_samples=W)
        tok, score, lg = e.generate_beam(z[:, 0].cuda(), m8, T, W, return_logits=True)
        assert e.kv0_table_generations() == 0 and e.chain_faults() == 0
        outs.append((tok.cpu(), score.cpu(), lg.cpu()))
        e.close()
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_legacy_decoder_never_takes_the_table_form():
    """ListenerGenerator's decoder input is emb + pos[t]: its first layer's K/V depend on the position"""
    from dimx import lib, prng, weights
    sd = weights.synth_state_dict(weights.listener_generator_spec(), 20260928)
    B, T = 2, 12
    v_s = torch.from_numpy(prng.normal(5, "legacy.vs", (B, T, 824)))
    mask = torch.ones(B, T, dtype=torch.bool)
    mask[1, 9:] = False
    m8 = mask.to(torch.uint8).cuda()
    start = torch.from_numpy(prng.integers(5, "kv0.legacy.start", (B,), 0, 512))
    outs = []
    for e in _gate_engines(None, lib.MODE_PARITY_F32, "legacy", sd):
        e.encode_ctx(v_s.cuda(), None, m8, True)
        tok, lg = e.generate(start.cuda(), m8, T, 0.0, return_logits=True)
        assert e.kv0_table_generations() == 0
        outs.append((tok.cpu(), lg.cpu()))
        e.close()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_the_image_follows_the_tables_epoch(full_sd):
    """after load_state_dict with other weights the next generation reads a rebuilt image: it equals a fresh engine's"""
    from dimx import lib, weights
    T = 20
    e = _engine(lib.MODE_PERF_BF16, True)
    e.load_state_dict(full_sd)

    def gen(eng, B, seed):
        v_s, v_a, z, mask = _case(B, T, [T - i for i in range(B)], seed=seed)
        m8 = mask.to(torch.uint8).cuda()
        eng.encode_ctx(v_s.cuda(), v_a.cuda(), m8, True)
        return eng.generate(z[:, 0].cuda(), m8, T, 0.0).cpu()

    a = gen(e, 7, 3)
    other = weights.synth_state_dict(weights.slmft_spec(), 77)
    e.load_state_dict(other)
    b = gen(e, 7, 3)
    assert e.kv0_table_generations() == 2 and e.qkv0_table_builds() == 2
    fresh = _engine(lib.MODE_PERF_BF16, True)
    fresh.load_state_dict(other)
    assert torch.equal(gen(fresh, 7, 3), b) and fresh.kv0_table_generations() == 1
    cache = _engine(lib.MODE_PERF_BF16, False)
    cache.load_state_dict(other)
    assert torch.equal(gen(cache, 7, 3), b) and cache.kv0_table_generations() == 0
    assert not torch.equal(a, b)   # the weights do matter to the tokens
    e.close()
    fresh.close()
    cache.close()
