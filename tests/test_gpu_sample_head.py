"""GPU: the sampler as the first stage of the first decoder layer's launch (csrc/chain.hip, xcd_layer_kernel HEAD; the shared
arithmetic is csrc/sample_pick.hpp) against the sampler launch it replaces (DIMX_NO_SAMPLE_HEAD=1).  The head runs sample_kernel's
top-k route with the same lane <-> element map, reductions and noise addressing, and the self attention reads the same f32
q/k/v table row the sampler used to copy, so "equal" below is torch.equal on the tokens AND on the per-step logits, greedy and
sampled; sample_head_generations() tells which route ran.  bf16 throughout: the f32 mode has no layer kernel."""
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


def _engine(head, sd):
    """the switch is read when the handle is created"""
    from dimx import engine, lib
    if not head:
        os.environ["DIMX_NO_SAMPLE_HEAD"] = "1"
    try:
        e = engine.Engine("cuda:0", lib.MODE_PERF_BF16, "slmft")
    finally:
        os.environ.pop("DIMX_NO_SAMPLE_HEAD", None)
    e.load_state_dict(sd)
    return e


def _both(sd, fn):
    """fn(engine) -> tuple of tensors, on the head route's engine and on the sampler launch's: (results, head generations, table-form
    generations) of each"""
    res = []
    for head in (True, False):
        e = _engine(head, sd)
        out = fn(e)
        assert e.chain_faults() == 0
        res.append(([t.cpu() for t in out], e.sample_head_generations(), e.kv0_table_generations()))
        e.close()
    return res


def _assert_equal(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and torch.equal(x, y), "output %d differs in %d places" % (i, (x != y).sum())


def _greedy_and_sampled(B, T, lens, seed, start_fix=None, temps=(0.0, 1.0)):
    v_s, v_a, z, mask = _case(B, T, lens, seed=seed)
    start = z[:, 0].clone()
    if start_fix is not None:
        start_fix(start)
    noise = torch.empty(T - 1, B, 512).exponential_(generator=torch.Generator().manual_seed(5)).cuda()

    def fn(e):
        m8 = mask.to(torch.uint8).cuda()
        out = []
        for temp in temps:
            e.encode_ctx(v_s.cuda(), v_a.cuda(), m8, True)
            tok, lg = e.generate(start.cuda(), m8, T, temp, 52, noise if temp > 0 else None, return_logits=True)
            assert tok.shape == (B, T - 1)
            out += [tok, lg]
        return out

    return fn


def _head_case(sd, B, T, lens, seed, **kw):
    (on, h_on, k_on), (off, h_off, k_off) = _both(sd, _greedy_and_sampled(B, T, lens, seed, **kw))
    assert h_on == 2 and h_off == 0, "head generations: %d with the switch on, %d with it off" % (h_on, h_off)
    assert k_on == 2 and k_off == 2   # the table form of the first layer runs on both routes
    _assert_equal(on, off)
    return on


def test_shortest_history_one_clip_in_the_fifth_group(full_sd):
    """B = 130, T = 12, ragged: the fifth XCD group holds two clips; the head runs from the first skipped step up to key counts
    short of one key batch"""
    B, T = 130, 12
    _head_case(full_sd, B, T, [T - i % 5 for i in range(B)], seed=17)


def test_partly_empty_group_and_clamped_start(full_sd):
    """B = 200, T = 48: a partly empty last group; one start id is -100, its history entry the clamped id 0"""
    B, T = 200, 48

    def fix(start):
        start[77] = -100

    _head_case(full_sd, B, T, [T - (i * 7) % 20 for i in range(B)], seed=31, start_fix=fix)


def test_every_cu_has_a_clip(full_sd):
    """B = 256, T = 20: temperature 0 and 1; the sampled tokens are not the greedy ones (the noise matters)"""
    B, T = 256, 20
    on = _head_case(full_sd, B, T, [T - i % 3 for i in range(B)], seed=7)
    assert not torch.equal(on[0], on[2])


def test_seeded_generation_on_the_device_generator(full_sd):
    """no noise tensor: the counter-based generator, keyed by (step, row, code), inside the head"""
    B, T = 140, 14
    v_s, v_a, z, mask = _case(B, T, [T - i % 4 for i in range(B)], seed=29)

    def fn(e):
        m8 = mask.to(torch.uint8).cuda()
        e.encode_ctx(v_s.cuda(), v_a.cuda(), m8, True)
        tok, lg = e.generate(z[:, 0].cuda(), m8, T, 0.9, 52, None, seed=1234, return_logits=True)
        e.encode_ctx(v_s.cuda(), v_a.cuda(), m8, True)
        greedy = e.generate(z[:, 0].cuda(), m8, T, 0.0)
        return tok, lg, greedy

    (on, h_on, _), (off, h_off, _) = _both(full_sd, fn)
    assert h_on == 2 and h_off == 0
    _assert_equal(on, off)
    assert not torch.equal(on[0], on[2])


def test_two_calls_replay_one_graph(full_sd):
    """seed and temperature live in the parameter block, and so does the first-step flag: a second call with other values replays
    the captured steps, the head runs in both, the table counter moves as before"""
    B, T = 136, 16
    v_s, v_a, z, mask = _case(B, T, [T - i % 6 for i in range(B)], seed=11)

    def fn(e):
        m8 = mask.to(torch.uint8).cuda()
        out = []
        for temp, seed in ((1.0, 77), (0.7, 78), (1.0, 77)):
            e.encode_ctx(v_s.cuda(), v_a.cuda(), m8, True)
            tok, lg = e.generate(z[:, 0].cuda(), m8, T, temp, 52, None, seed=seed, return_logits=True)
            out += [tok, lg]
        assert e.qkv0_table_builds() == 1
        return out

    (on, h_on, k_on), (off, h_off, k_off) = _both(full_sd, fn)
    assert h_on == 3 and h_off == 0 and k_on == 3 and k_off == 3
    _assert_equal(on, off)
    assert torch.equal(on[0], on[4]) and not torch.equal(on[0], on[2])   # the same seed again: the same tokens


# ---- the gate: each of these runs the sampler launch (counter unchanged) and equals the switched-off engine's output

def _gate_case(sd, fn):
    (on, h_on, _), (off, h_off, _) = _both(sd, fn)
    assert h_on == 0 and h_off == 0
    _assert_equal(on, off)


def _gate_inputs(B, T, seed):
    v_s, v_a, z, mask = _case(B, T, [T - i % 5 for i in range(B)], seed=seed)
    return v_s.cuda(), v_a.cuda(), z, mask.to(torch.uint8).cuda()


def test_gate_top_p_filter(full_sd):
    B, T = 132, 10
    v_s, v_a, z, m8 = _gate_inputs(B, T, 43)

    def fn(e):
        e.set_sampler_filter(1, 0.8)
        e.encode_ctx(v_s, v_a, m8, True)
        return e.generate(z[:, 0].cuda(), m8, T, 1.0, 52, None, seed=9, return_logits=True)

    _gate_case(full_sd, fn)


def test_gate_several_samples_per_clip(full_sd):
    B, T, S = 30, 10, 5
    v_s, v_a, z, m8 = _gate_inputs(B, T, 47)

    def fn(e):
        e.encode_ctx(v_s, v_a, m8, True, n_samples=S)
        return e.generate(z[:, 0].cuda(), m8, T, 1.0, 52, None, seed=9, return_logits=True, n_samples=S)

    _gate_case(full_sd, fn)


def test_gate_prompt(full_sd):
    B, T, P = 132, 12, 4
    v_s, v_a, z, m8 = _gate_inputs(B, T, 53)

    def fn(e):
        e.encode_ctx(v_s, v_a, m8, True, prompt_frames=P)
        a = e.generate(None, m8, T, 0.0, return_logits=True, prompt=z[:, :P].cuda(), prefill=P)
        e.encode_ctx(v_s, v_a, m8, True, prompt_frames=P)
        b = e.generate(None, m8, T, 0.0, return_logits=True, prompt=z[:, :P].cuda(), no_prefill=True)
        return a + b

    _gate_case(full_sd, fn)


def test_gate_beam_search(full_sd):
    B, T, W = 3, 12, 2
    v_s, v_a, z, m8 = _gate_inputs(B, T, 59)

    def fn(e):
        e.encode_ctx(v_s, v_a, m8, True, n_samples=W)
        return e.generate_beam(z[:, 0].cuda(), m8, T, W, return_logits=True)

    _gate_case(full_sd, fn)


def test_gate_guidance(full_sd):
    B, T = 66, 10
    v_s, v_a, z, m8 = _gate_inputs(B, T, 61)

    def fn(e):
        e.encode_ctx(v_s, v_a, m8, True, guided=True)
        return e.generate(z[:, 0].cuda(), m8, T, 1.0, 52, None, seed=9, return_logits=True, guidance=1.5)

    _gate_case(full_sd, fn)


def test_gate_small_batch(full_sd):
    """B = 6: no layer kernel (a (clip, head) pair is split over several waves), so no head"""
    B, T = 6, 16
    v_s, v_a, z, m8 = _gate_inputs(B, T, 67)

    def fn(e):
        e.encode_ctx(v_s, v_a, m8, True)
        return e.generate(z[:, 0].cuda(), m8, T, 1.0, 52, None, seed=9, return_logits=True)

    _gate_case(full_sd, fn)


def test_gate_logits_bias(full_sd):
    """a checkpoint with to_logits.bias: the logits are not the final chain launch's single slab"""
    from dimx import prng
    B, T = 132, 10
    v_s, v_a, z, m8 = _gate_inputs(B, T, 71)
    sd = dict(full_sd)
    sd["decoder_joint.net.to_logits.bias"] = torch.from_numpy(prng.normal(5, "head.b", (512,))) * 0.5

    def fn(e):
        e.encode_ctx(v_s, v_a, m8, True)
        return e.generate(z[:, 0].cuda(), m8, T, 1.0, 52, None, seed=9, return_logits=True)

    _gate_case(sd, fn)


def test_new_weights_between_two_generations(full_sd):
    """load_state_dict between two generations rebuilds the table the head reads q/k/v rows of: the second generation equals a
    fresh engine's, on both routes"""
    from dimx import weights
    B, T = 130, 12
    v_s, v_a, z, m8 = _gate_inputs(B, T, 73)
    other = weights.synth_state_dict(weights.slmft_spec(), 77)

    def gen(e):
        e.encode_ctx(v_s, v_a, m8, True)
        return e.generate(z[:, 0].cuda(), m8, T, 1.0, 52, None, seed=21, return_logits=True)

    def fn(e):
        a = gen(e)
        e.load_state_dict(other)
        b = gen(e)
        assert e.qkv0_table_builds() == 2
        return a + b

    (on, h_on, _), (off, h_off, _) = _both(full_sd, fn)
    assert h_on == 2 and h_off == 0
    _assert_equal(on, off)
    assert not torch.equal(on[0], on[2])   # the weights do matter to the tokens
    fresh = _engine(True, other)
    tok, lg = gen(fresh)
    assert torch.equal(tok.cpu(), on[2]) and torch.equal(lg.cpu(), on[3]) and fresh.sample_head_generations() == 1
    fresh.close()


def test_forced_placement_fault_is_noticed_and_repaired(full_sd):
    """the chain kernels' placement hook (dimx_debug_chain_fault) on the head route: the call itself counts the fault and
    regenerates the batch on the one-kernel-per-op step with the plain sampler -- the tokens of a handle without chain kernels"""
    from dimx import engine, lib
    B, T = 130, 10
    v_s, v_a, z, m8 = _gate_inputs(B, T, 79)
    os.environ["DIMX_NO_CHAIN"] = "1"
    try:
        ref_eng = engine.Engine("cuda:0", lib.MODE_PERF_BF16, "slmft")
    finally:
        os.environ.pop("DIMX_NO_CHAIN", None)
    ref_eng.load_state_dict(full_sd)
    ref_eng.encode_ctx(v_s, v_a, m8, True)
    ref = ref_eng.generate(z[:, 0].cuda(), m8, T, 1.0, 52, None, seed=33).cpu()
    assert ref_eng.sample_head_generations() == 0
    ref_eng.close()
    e = _engine(True, full_sd)
    e.debug_chain_fault(1)
    e.encode_ctx(v_s, v_a, m8, True)
    tok = e.generate(z[:, 0].cuda(), m8, T, 1.0, 52, None, seed=33).cpu()
    assert e.chain_faults() == 1, "the faulted call itself must notice"
    assert e.sample_head_generations() == 1   # the faulted run took the head, its regeneration did not
    assert torch.equal(tok, ref), "the faulted batch must be regenerated without the chain kernels"
    e.close()


# ---- the launch alone (dimx_op_layer_chain_head) against sample_kernel followed by the first layer's launch on the same buffers

def _params(step, temp, epoch, first, rows_total):
    import struct
    p = [0] * 16
    p[0], p[2], p[7], p[9], p[14] = step, struct.unpack("i", struct.pack("f", temp))[0], rows_total, epoch, first
    return torch.tensor(p, dtype=torch.int32, device="cuda:0")


@pytest.mark.parametrize("B", [129, 256])
def test_the_launch_alone_has_the_bits_of_sampler_then_layer_launch(B):
    """B = 129: one clip in the fifth group; B = 256: every CU has one.  0 cached keys is the first step of a call (the head is
    skipped, the token is the history's), 5 and 40 are later steps, greedy and sampled with injected noise.  Token column, history,
    x, y, the partial statistics, qc, o and the step / epoch words must have the bits the two launches leave."""
    import layer_ref as R
    from dimx import engine as E
    dev, T, NK = "cuda:0", 48, 40
    inp = R.make_inputs(B, T, T, NK, seed=B, device=dev)
    rows = inp["R"]
    g = torch.Generator().manual_seed(100 + B)
    qkv0 = torch.randn(512, 3 * R.INNER, generator=g).to(dev)
    tab = qkv0[:, R.INNER:].to(torch.bfloat16).contiguous()   # K at 0, V at 768: the image the cache append would hold
    emb = torch.randn(512, R.C, generator=g).to(dev)
    logits = (torch.randn(rows, 512, generator=g) * 3).to(dev)
    noise = torch.empty(T, B, 512).exponential_(generator=g).to(dev)
    hist0 = torch.randint(0, 512, (rows, T), generator=g, dtype=torch.int32).to(dev)
    cache = torch.zeros(1, R.H, T, R.D, dtype=torch.bfloat16, device=dev)   # never touched by the table form

    def bits(t):
        return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)

    def layer(qkv, x, hist, step):
        return E.op_layer_chain(qkv, cache, cache, inp["ck"], inp["cv"], NK, inp["mask"], inp["w_so"], inp["w_cq"], inp["colsum"],
                                inp["w_co"], x, step, B=B, scale=R.SCALE, tab=tab, hist=hist, tab_koff=0, tab_voff=R.INNER, tab_rows=512)

    for keys, temp in ((0, 1.0), (5, 1.0), (40, 0.0), (40, 1.0)):
        first = keys == 0
        step = 0 if first else keys - 1
        tok_h = torch.full((rows, T - 1), -7, dtype=torch.int32, device=dev)
        tok_r = tok_h.clone()
        hist_h, hist_r = hist0.clone(), hist0.clone()
        x_h, x_r = inp["x0"].clone(), inp["x0"].clone()
        p_h = _params(step, temp, 0 if first else -1, 1 if first else 0, B)
        p_r = _params(step, temp, 0 if first else -1, 0, B)
        nz = noise if temp > 0 else None
        got = E.op_layer_chain_head(qkv0, logits, 52, nz, B, tok_h, emb, p_h, hist_h, tab, inp["ck"], inp["cv"], NK, inp["mask"],
                                    inp["w_so"], inp["w_cq"], inp["colsum"], inp["w_co"], x_h, B, scale=R.SCALE, tab_voff=R.INNER)
        if first:
            qkv = qkv0[hist_r[:, 0].long()].unsqueeze(0).contiguous()
        else:
            qkv = torch.full((1, rows, 3 * R.INNER), float("nan"), device=dev)
            E.op_sample_step(logits, B, 52, nz, B, tok_r, emb, x_r, qkv0, qkv[0], hist_r, p_r)
        want = layer(qkv, x_r, hist_r, p_r[0:1])
        assert got[4] == 0 and want[4] == 0
        assert torch.equal(tok_h, tok_r) and torch.equal(hist_h, hist_r), (keys, temp)
        assert first or (tok_h[:B, step] >= 0).all()
        assert torch.equal(bits(x_h), bits(x_r)), (keys, temp, "x")
        for name, a, b in zip(("y", "o", "qc"), got, want):
            assert torch.equal(bits(a[:B]), bits(b[:B])), (keys, temp, name)
        assert torch.equal(bits(got[3]), bits(want[3])), (keys, temp, "stats")
        assert p_h.tolist() == p_r.tolist(), (keys, temp, p_h.tolist(), p_r.tolist())
        assert p_h[0].item() == keys and p_h[8].item() == 0 and p_h[9].item() == 0 and p_h[14].item() == 0
