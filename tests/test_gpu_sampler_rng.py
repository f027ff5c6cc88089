"""GPU: what a seeded sampler call draws.  Every route that consumes the on-device noise generator (csrc/sample_pick.hpp,
sample_survivor) is held to its host definition dimx.prng.sampler_noise (include/dimx.h, at dimx_set_shard): the sampler launches
alone (dimx_op_sample, _filtered, _guided), the step launches on a parameter block (dimx_op_sample_step, dimx_op_layer_chain_head),
and Engine.generate -- plain, best-of-N, prompted, sharded, in clip groups, guided, the bf16 head-in-layer route -- and a streaming
session, each step against that step's own returned logits.

The rule is tests/test_gpu_sampler_filters.py's: the wanted token is dimx.sampling.sample_ref(l, q, T, kind) with
q = sampler_noise(...) of that call, a row is left out only when dimx.sampling.undecidable(l, kind, MARGIN, noise=q, ...) marks it,
and every case asserts excluded <= EXCLUDE_CAP * rows and mismatches == 0 and prints both counts.  The definition does not restate
the kernel's float32 log1pf / expf / division: two float64 scores at least MARGIN apart are not reordered by those roundings."""
import os
import struct

import numpy as np
import pytest
import torch

from test_gpu_sampler_filters import (B, EXCLUDE_CAP, FILTERS, MARGIN, P0, PLEN, PMAX, T, _check_steps, _Gen, _logits, _report)
from test_sampler_rng_host import SEED, chi2_q999, multinomial_case, multinomial_statistic

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

SEEDS = (1, 2 ** 63 + 12345)
STEPS = (0, 3, 2 ** 33 + 5)          # the last one needs the 64-bit counter
TOP_K = ("top_k", {"k": 52})


def _count(l, q, tok, kind, kw, temperature=1.0):
    """(excluded, mismatches on decidable rows, rows) of one launch: logits l [R,512], definition noise q, device tokens tok"""
    from dimx import sampling
    bad = sampling.undecidable(l, kind, MARGIN, noise=q, temperature=temperature, **kw)
    want = sampling.sample_ref(l, q, temperature, kind, **kw)
    tok = np.asarray(tok, dtype=np.int64)
    return int(bad.sum()), int((tok[~bad] != want[~bad]).sum()), len(tok)


def _settle(what, counts):
    """report and assert the sum of _count results of one case"""
    excluded, mismatches, rows = (sum(c[i] for c in counts) for i in range(3))
    _report(what, excluded, rows, mismatches)
    assert rows > 0 and excluded <= EXCLUDE_CAP * rows
    assert mismatches == 0
    return rows


def _gen_noise(seed, steps, rows, rows_total=None, row_offset=0):
    """[steps, rows, 512] float64: the definition's noise of a generation's steps 0 .. steps - 1"""
    from dimx import prng
    return np.stack([prng.sampler_noise(seed, t, rows, rows_total, row_offset) for t in range(steps)])


def _check_gen(what, tok, lg, noise, kind, kw, temperature=1.0, free=None):
    """_check_steps for any shape: tok [R,n], lg [R,n,512] (numpy), noise [n,R,512]; free [R,n] marks the sampled columns"""
    counts = []
    for t in range(tok.shape[1]):
        sel = np.ones(tok.shape[0], dtype=bool) if free is None else free[:, t]
        if sel.any():
            counts.append(_count(lg[sel, t], noise[t][sel], tok[sel, t], kind, kw, temperature))
    return _settle(what, counts)


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("scale", [1, 3, 6])
@pytest.mark.parametrize("R", [1, 256, 1030])      # one row / one wave per block / four waves per block with a ragged last block
def test_op_sample_draws_the_definition(R, scale):
    from dimx import engine, prng
    l = _logits(R, scale)
    lg = torch.from_numpy(l).cuda()
    counts, drawn = [], set()
    for seed in SEEDS:
        for step in STEPS:
            q = prng.sampler_noise(seed, step, R)
            for temperature in (1.0, 0.7):
                tok = engine.op_sample(lg, 52, temperature, None, seed, step).cpu().numpy()
                counts.append(_count(l, q, tok, *TOP_K, temperature=temperature))
                drawn.add(tok.tobytes())
    _settle("op_sample R=%d scale=%d top-k 52, 2 seeds x 3 steps x 2 temperatures" % (R, scale), counts)
    if R >= 256 and scale < 6:
        assert len(drawn) == 12, "every (seed, step, temperature) draws other tokens"


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("kind,kw", FILTERS)
def test_op_sample_filtered_draws_the_definition(kind, kw):
    """scale 1: more than 128 survivors under top_p 0.9 (the per-element loop); 3: the compacted path; 6: single survivors"""
    from dimx import engine, prng, sampling
    R, seed, step = 1030, 9001, 3
    q = prng.sampler_noise(seed, step, R)
    for scale in (1, 3, 6):
        l = _logits(R, scale)
        lg = torch.from_numpy(l).cuda()
        counts = []
        for temperature in (1.0, 0.7):
            tok = engine.op_sample(lg, noise=None, seed=seed, step=step, temperature=temperature, filter_logits_fn=kind, filter_kwargs=kw)
            counts.append(_count(l, q, tok.cpu().numpy(), kind, kw, temperature))
        _settle("op_sample_filtered R=%d scale=%d %s %s T=1.0, 0.7" % (R, scale, kind, kw), counts)
        if (kind, kw) == ("top_p", {"thres": 0.9}) and scale == 1:
            assert sampling.keep_mask(l, kind, **kw).sum(1).max() > 128


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("R,scale", [(256, 1), (1030, 3)])
def test_seeded_call_equals_the_call_given_the_definition_as_a_tensor(R, scale):
    """ties the generator to the injected-noise path the goldens (sampler_multinomial.npz) pin"""
    from dimx import engine, prng, sampling
    l = _logits(R, scale)
    lg = torch.from_numpy(l).cuda()
    for kind, kw in [TOP_K, ("top_p", {"thres": 0.9})]:
        excluded = differ = 0
        for seed, step in ((9001, 3), (SEEDS[1], STEPS[2])):
            q = prng.sampler_noise(seed, step, R)
            a = engine.op_sample(lg, noise=None, seed=seed, step=step, filter_logits_fn=kind, filter_kwargs=kw).cpu().numpy()
            b = engine.op_sample(lg, noise=torch.from_numpy(q.astype(np.float32)).cuda(), filter_logits_fn=kind, filter_kwargs=kw).cpu().numpy()
            bad = sampling.undecidable(l, kind, MARGIN, noise=q, **kw)
            excluded += int(bad.sum())
            differ += int((a[~bad] != b[~bad]).sum())
        _report("seeded against injected sampler_noise R=%d scale=%d %s" % (R, scale, kind), excluded, 2 * R, differ)
        assert excluded <= EXCLUDE_CAP * 2 * R
        assert differ == 0


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("lscale", [1, 3])
def test_op_sample_guided_draws_the_definition(lscale):
    """the mixed logits are tests/guidance_ref.py's (dimx.guidance.combine, float64); one noise row per clip: row b of an R-row
    generation, the same token for both branches"""
    import guidance_ref
    from dimx import engine, guidance, prng, sampling
    from test_gpu_guidance import _rows
    R, seed = 256, 9001
    c, u = _rows(R, lscale, "c"), _rows(R, lscale, "u")
    cg, ug = torch.from_numpy(c).cuda(), torch.from_numpy(u).cuda()
    counts = []
    for scale in (1.0, 1.5, 3.0):
        g = guidance.combine(c, u, scale)
        for step in (0, 3):
            q = prng.sampler_noise(seed, step, R)
            tok = engine.op_sample_guided(cg, ug, scale, noise=None, seed=seed, step=step, return_guided=False).cpu().numpy()
            assert np.array_equal(tok[:R], tok[R:])
            bad = sampling.undecidable(g, "top_k", MARGIN, noise=q, k=52)
            want = np.asarray(guidance_ref.sample_guided(g, q, 1.0, *TOP_K))
            counts.append((int(bad.sum()), int((tok[:R][~bad] != want[~bad]).sum()), R))
    _settle("op_sample_guided R=%d logits x%d, scales 1, 1.5, 3 x steps 0, 3" % (R, lscale), counts)


# ---------------------------------------------------------------------------------------------------------------- 5
def _block(step, temperature, seed, offset, total, epoch, first=0):
    """the 16-word parameter block: 0 step, 2 temperature, 4-5 seed, 6 / 7 the generator window, 9 epoch, 14 first-step flag"""
    p = [0] * 16
    p[0], p[2], p[6], p[7], p[9], p[14] = step, struct.unpack("i", struct.pack("f", temperature))[0], offset, total, epoch, first
    p[4], p[5] = struct.unpack("ii", struct.pack("Q", seed))
    return torch.tensor(p, dtype=torch.int32, device="cuda:0")


@pytest.mark.parametrize("Bh", [129, 256])
def test_step_launches_draw_the_definition_inside_a_window(Bh):
    """dimx_op_sample_step and the head of the first layer's launch (the shapes of test_gpu_sample_head.py: one clip in the fifth
    group / every CU has one), no noise tensor, the seed in words 4-5, the window (300, 1000) in words 6 / 7: row r of step t draws
    global row 300 + r of 1000"""
    import layer_ref as LR
    from dimx import engine as E
    from dimx import prng
    dev, Th, NK, OFF, TOT = "cuda:0", 48, 40, 300, 1000
    inp = LR.make_inputs(Bh, Th, Th, NK, seed=Bh, device=dev)
    rows = inp["R"]
    qkv0 = torch.from_numpy(prng.normal(31, "sampler.rng.head.qkv0", (512, 3 * LR.INNER))).to(dev)
    tab = qkv0[:, LR.INNER:].to(torch.bfloat16).contiguous()
    emb = torch.from_numpy(prng.normal(31, "sampler.rng.head.emb", (512, LR.C))).to(dev)
    l = prng.normal(31, "sampler.rng.head.logits.%d" % Bh, (rows, 512)) * np.float32(3)
    logits = torch.from_numpy(l).to(dev)
    hist0 = torch.from_numpy(prng.integers(31, "sampler.rng.head.hist.%d" % Bh, (rows, Th), 0, 512).astype(np.int32)).to(dev)
    counts = {"sample_step": [], "layer_chain_head": []}
    for step, temperature, seed in ((4, 1.0, SEEDS[0]), (39, 0.7, SEEDS[1])):
        q = prng.sampler_noise(seed, step, Bh, rows_total=TOT, row_offset=OFF)
        tok_s = torch.full((rows, Th - 1), -7, dtype=torch.int32, device=dev)
        tok_h = tok_s.clone()
        x_s, x_h = inp["x0"].clone(), inp["x0"].clone()
        qkv = torch.full((rows, 3 * LR.INNER), float("nan"), device=dev)
        p_s, p_h = _block(step, temperature, seed, OFF, TOT, -1), _block(step, temperature, seed, OFF, TOT, -1)
        E.op_sample_step(logits, Bh, 52, None, Bh, tok_s, emb, x_s, qkv0, qkv, hist0.clone(), p_s)
        flags = E.op_layer_chain_head(qkv0, logits, 52, None, Bh, tok_h, emb, p_h, hist0.clone(), tab, inp["ck"], inp["cv"], NK, inp["mask"],
                                      inp["w_so"], inp["w_cq"], inp["colsum"], inp["w_co"], x_h, Bh, scale=LR.SCALE, tab_voff=LR.INNER)[4]
        assert flags == 0 and p_s[0].item() == step + 1 and p_h[0].item() == step + 1
        for name, tok in (("sample_step", tok_s), ("layer_chain_head", tok_h)):
            tok = tok.cpu().numpy()
            assert (np.delete(tok[:Bh], step, axis=1) == -7).all() and (tok[Bh:] == -7).all(), "only the step's column of the B rows"
            counts[name].append(_count(l[:Bh], q, tok[:Bh, step], *TOP_K, temperature=temperature))
    for name in counts:
        _settle("op_%s B=%d window (%d, %d), steps 4 and 39" % (name, Bh, OFF, TOT), counts[name])


# ---------------------------------------------------------------------------------------------------------------- 6 - 9
class _Seeded:
    """what _check_steps reads of its inputs object, with the definition's noise in the place of the injected tensor"""

    def __init__(self, gen, S, seed, rows_total=None, row_offset=0):
        self.z = gen.z
        self.noise = {S: torch.from_numpy(_gen_noise(seed, T - 1, B * S, rows_total, row_offset))}


def _run(eng, g, S, prompted, seed, **kw):
    """_Gen.run without a noise tensor"""
    eng.encode_ctx(g.v_s, g.v_a, g.m8, True, n_samples=S, prompt_frames=P0 if prompted else 1)
    if prompted:
        kw.update(prompt=g.z[:, :PMAX].to(torch.int32).cuda().contiguous(), prompt_len=torch.tensor(PLEN, dtype=torch.int32).cuda(), prefill=P0)
    tok, lg = eng.generate(None if prompted else g.z[:, 0].cuda(), g.m8, T, 1.0, 52, None, seed=seed, return_logits=True, n_samples=S, **kw)
    return tok.cpu().numpy().astype(np.int64), lg.cpu().numpy()


@pytest.fixture(scope="module")
def gen():
    return _Gen()


def _f32_engine(sd):
    from dimx import engine, lib
    e = engine.Engine("cuda:0", lib.MODE_PARITY_F32)
    e.load_state_dict(sd)
    return e


@pytest.fixture(scope="module")
def eng(full_sd):
    return _f32_engine(full_sd)


GEN_FILTERS = [TOP_K, ("top_p", {"thres": 0.9})]


@pytest.mark.parametrize("kind,kw", GEN_FILTERS)
@pytest.mark.parametrize("S,prompted", [(1, False), (2, False), (1, True), (2, True)])
def test_generation_draws_the_definition_at_every_step(eng, gen, S, prompted, kind, kw):
    """sample s of clip b is row b S + s of B S; a prompted call draws at step t what dimx_generate draws at step t (the forced
    columns consume nothing)"""
    seed = SEEDS[S - 1]
    tok, lg = _run(eng, gen, S, prompted, seed, filter_logits_fn=kind, filter_kwargs=kw)
    rows = _check_steps("generate(seed) S=%d prompted=%d %s %s" % (S, prompted, kind, kw), _Seeded(gen, S, seed), tok, lg, S, kind, kw,
                        prompted=prompted)
    assert rows == (B * S * (T - 1) if not prompted else S * sum(T - p for p in PLEN))


def test_a_shard_draws_its_rows_of_the_whole_batch(eng, gen):
    """set_shard(5, 11) with two samples per clip: the definition at row offset 5 * 2 of 11 * 2 rows"""
    S, seed = 2, 4242
    eng.set_shard(5, 11)
    try:
        tok, lg = _run(eng, gen, S, False, seed)
    finally:
        eng.set_shard(0, 0)
    _check_steps("generate(seed) S=2 on shard (5, 11)", _Seeded(gen, S, seed, rows_total=11 * S, row_offset=5 * S), tok, lg, S, *TOP_K)
    plain, plain_lg = _run(eng, gen, S, False, seed)
    assert not np.array_equal(plain, tok), "the window does move the draw"
    _check_steps("generate(seed) S=2 after set_shard(0, 0)", _Seeded(gen, S, seed), plain, plain_lg, S, *TOP_K)


def _clips(Bc, Tc, seed):
    from dimx import prng
    v_s = torch.from_numpy(prng.normal(seed, "s2s.vs", (Bc, Tc, 56))).cuda()
    v_a = torch.from_numpy(prng.normal(seed, "s2s.va", (Bc, Tc, 768))).cuda()
    start = torch.from_numpy(prng.integers(seed, "s2s.z", (Bc, Tc), 0, 512))[:, 0].to(torch.int32).cuda()
    return v_s, v_a, start


def test_clip_groups_keep_the_rows_numbers(full_sd):
    """B = 5 in two clip groups (rows 0-1 and 2-4, each on its own stream): row0 enters the counter"""
    Bc, Tc, seed = 5, 12, 77
    v_s, v_a, start = _clips(Bc, Tc, 6)
    m8 = torch.zeros(Bc, Tc, dtype=torch.uint8)
    for j, n in enumerate((12, 10, 12, 5, 9)):
        m8[j, :n] = 1
    m8 = m8.cuda()
    os.environ["DIMX_GEN_GROUPS"] = "2"
    try:
        e = _f32_engine(full_sd)
    finally:
        os.environ.pop("DIMX_GEN_GROUPS", None)
    e.encode_ctx(v_s, v_a, m8, True)
    tok, lg = e.generate(start, m8, Tc, 1.0, 52, None, seed=seed, return_logits=True)
    e.close()
    tok, lg = tok.cpu().numpy(), lg.cpu().numpy()
    noise = _gen_noise(seed, Tc - 1, Bc)
    _check_gen("generate(seed) B=5 in 2 clip groups", tok, lg, noise, *TOP_K)
    # a second group that numbered its rows from 0 would give rows 2 .. 4 the noise of rows 0 .. 2: that is another draw here
    from dimx import sampling
    shifted = np.stack([sampling.sample_ref(lg[2:, t], noise[t][:3], 1.0, *TOP_K[:1], **TOP_K[1]) for t in range(Tc - 1)], axis=1)
    assert not np.array_equal(shifted, tok[2:])


def test_guided_generation_draws_one_row_per_clip(full_sd, gen):
    """generate(guidance=): the returned logits are the guided ones, row b draws row b of a B-row generation"""
    e = _f32_engine(full_sd)
    for scale, seed in ((1.5, SEEDS[0]), (3.0, SEEDS[1])):
        e.encode_ctx(gen.v_s, gen.v_a, gen.m8, True, guided=True)
        tok, lg = e.generate(gen.z[:, 0].cuda(), gen.m8, T, 1.0, 52, None, seed=seed, return_logits=True, guidance=scale)
        _check_gen("generate(guidance=%.1f, seed)" % scale, tok.cpu().numpy(), lg.cpu().numpy(), _gen_noise(seed, T - 1, B), *TOP_K)
    e.close()


@pytest.mark.parametrize("lookahead", [0, 2])
def test_a_streaming_session_draws_what_generate_draws(eng, gen, lookahead):
    """Engine.stream(seed=): step t of a session draws step t of a B-row generation, whatever Tmax and the pushes' sizes; the
    whole-clip generate(lookahead=, seed=) is checked the same way"""
    seed, Tmax = 31337, T + 4
    noise = _gen_noise(seed, T - 1, B)
    n = 0
    with eng.stream(B, Tmax, gen.z[:, 0].to(torch.int32).cuda(), lookahead=lookahead, seed=seed) as s:
        for ch in (5, 1, T - 6):
            s.push(gen.v_s[:, n:n + ch], gen.v_a[:, n:n + ch], return_logits=True)
            n += ch
        s.end(return_logits=True)
        assert s.steps == T - 1
        tok, lg = s.tokens.cpu().numpy(), s._lg[:, :s.steps].cpu().numpy()
    _check_gen("stream(lookahead=%d, seed)" % lookahead, tok, lg, noise, *TOP_K)
    full = torch.ones(B, T, dtype=torch.uint8).cuda()
    eng.encode_ctx(gen.v_s, gen.v_a, full, True)
    wtok, wlg = eng.generate(gen.z[:, 0].cuda(), full, T, 1.0, 52, None, seed=seed, return_logits=True, lookahead=lookahead)
    _check_gen("generate(lookahead=%d, seed)" % lookahead, wtok.cpu().numpy(), wlg.cpu().numpy(), noise, *TOP_K)


# ---------------------------------------------------------------------------------------------------------------- 10
def test_bf16_head_in_layer_route_draws_the_definition(full_sd):
    """B = 140, T = 14 on the bf16 engine: the sampling head inside the first layer's launch.  Against the call's own logits, so
    the mode's rounding does not enter."""
    from dimx import engine, lib
    from test_gpu_sample_head import _case
    Bc, Tc, seed, temperature = 140, 14, 1234, 0.9
    v_s, v_a, z, mask = _case(Bc, Tc, [Tc - i % 4 for i in range(Bc)], seed=29)
    m8 = mask.to(torch.uint8).cuda()
    e = engine.Engine("cuda:0", lib.MODE_PERF_BF16, "slmft")
    e.load_state_dict(full_sd)
    e.encode_ctx(v_s.cuda(), v_a.cuda(), m8, True)
    tok, lg = e.generate(z[:, 0].cuda(), m8, Tc, temperature, 52, None, seed=seed, return_logits=True)
    heads, faults = e.sample_head_generations(), e.chain_faults()
    e.close()
    assert heads == 1 and faults == 0, "the head route ran (%d generations, %d chain faults)" % (heads, faults)
    _check_gen("generate(seed) bf16 B=140 T=14, head in the layer launch, T=0.9", tok.cpu().numpy(), lg.cpu().numpy(),
               _gen_noise(seed, Tc - 1, Bc), *TOP_K, temperature=temperature)


# ---------------------------------------------------------------------------------------------------------------- 11
def test_device_frequencies_are_the_definitions():
    """the multinomial case of tests/test_sampler_rng_host.py at R = 4099 rows of one tiled logit row: the device's tokens are the
    definition's on decidable rows, so the definition's statistics are the device's.  The chi-square of the device's own counts is
    printed and held to the same quantile."""
    from dimx import engine, sampling
    R = 4099
    l, q, p = multinomial_case(R)
    tok = engine.op_sample(torch.from_numpy(l).cuda(), 52, 1.0, None, SEED, 0).cpu().numpy()
    _settle("op_sample R=%d rows of one logit row, seed %d" % (R, SEED), [_count(l, q, tok, *TOP_K)])
    stat, cells = multinomial_statistic(tok, p)
    ref, _ = multinomial_statistic(sampling.sample_ref(l, q, 1.0, "top_k", k=52), p)
    print("device counts: chi-square %.2f over %d cells (the definition's %.2f, bound %.1f)" % (stat, cells, ref, chi2_q999(cells - 1)))
    assert stat < chi2_q999(cells - 1)
