"""GPU: prompted generation (dimx_generate_prompted) -- the prefill of the decode K/V cache from given codes, the forced
decode steps of ragged prompts, and the host layers above them -- against the prompted CPU oracle of tests/prompt_ref.py
and against the library's own free generation."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
LOGIT_TOL = 1e-4     # tests/test_gpu_s2s.py: teacher-forced logits against the oracle (the prefill's first decode step)
STEP_TOL = 2e-3      # tests/test_gpu_s2s.py: per-step logits of a generation against the oracle
SHORT = (3, 40, (40, 33, 7))
LONG = (2, 150, (150, 101))   # Pmax = P0 = 131: a prefill that crosses a 128-row tile with a ragged tail
ERR_ARG, ERR_WORKSPACE = -1, -5


def _case(B, T, lens, seed=9):
    from dimx import prng
    v_s = torch.from_numpy(prng.normal(seed, "s2s.vs", (B, T, 56)))
    v_a = torch.from_numpy(prng.normal(seed, "s2s.va", (B, T, 768)))
    z = torch.from_numpy(prng.integers(seed, "s2s.z", (B, T), 0, 512))
    mask = torch.zeros(B, T, dtype=torch.bool)
    for j, n in enumerate(lens):
        mask[j, :n] = True
    z = torch.where(mask, z, torch.full_like(z, -100))
    return v_s, v_a, z, mask


def _noise(B, T):
    from dimx import prng
    return torch.from_numpy(prng.exponential(11, "s2s.noise", (T - 1, B, 512)))


class _Case:
    """inputs of one shape + the oracle's context, computed once and left unchanged"""

    def __init__(self, sd, B, T, lens):
        import prompt_ref
        self.B, self.T, self.lens = B, T, lens
        self.v_s, self.v_a, self.z, self.mask = _case(B, T, list(lens))
        self.noise = _noise(B, T)
        self.ctx = prompt_ref.case_context(sd, self.v_s, self.v_a, self.mask)
        self.m8 = self.mask.to(torch.uint8).cuda()
        self.sd = sd
        self._ref = {}

    def oracle(self, Pmax, plen, noisy):
        import prompt_ref
        key = (Pmax, None if plen is None else tuple(plen), noisy)
        if key not in self._ref:
            self._ref[key] = prompt_ref.prompted_generate(self.sd, self.z[:, :Pmax], plen, self.T - 1, self.ctx, self.mask,
                                                          self.noise if noisy else None)
        return self._ref[key]

    def context(self, eng, prompt_frames=1, n_samples=1):
        eng.encode_ctx(self.v_s.cuda(), self.v_a.cuda(), self.m8, True, n_samples=n_samples, prompt_frames=prompt_frames)

    def run(self, eng, noisy, **kw):
        tok, lg = eng.generate(self.z[:, 0].cuda(), self.m8, self.T, 1.0 if noisy else 0.0, 52, self.noise.cuda() if noisy else None,
                               return_logits=True, **kw)
        return tok.cpu().long(), lg.cpu()


@pytest.fixture(scope="module")
def eng(full_sd):
    from dimx import engine, lib
    e = engine.Engine("cuda:0", lib.MODE_PARITY_F32)
    e.load_state_dict(full_sd)
    return e


@pytest.fixture(scope="module")
def eng_bf16(full_sd):
    from dimx import engine, lib
    e = engine.Engine("cuda:0", lib.MODE_PERF_BF16)
    e.load_state_dict(full_sd)
    return e


@pytest.fixture(scope="module")
def short(full_sd):
    return _Case(full_sd, *SHORT)


@pytest.fixture(scope="module")
def long_(full_sd):
    return _Case(full_sd, *LONG)


def _plen_t(plen):
    return None if plen is None else torch.tensor(plen, dtype=torch.int32).cuda()


# ---- 1
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("seeded", [False, True])
def test_one_token_prompt_is_dimx_generate(eng, eng_bf16, short, mode, seeded):
    e = eng if mode == "f32" else eng_bf16
    c = short
    kw = dict(temperature=1.0, seed=12345) if seeded else dict(temperature=0.0)
    start = c.z[:, 0].cuda()
    c.context(e)
    tok, lg = e.generate(start, c.m8, c.T, return_logits=True, **kw)
    c.context(e)
    ptok, plg = e.generate(None, c.m8, c.T, return_logits=True, prompt=start[:, None], **kw)
    assert torch.equal(tok, ptok) and torch.equal(lg, plg)


# ---- 2
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("seeded", [False, True])
def test_forced_steps_are_the_decode_steps(eng, eng_bf16, short, mode, seeded):
    """a prompt made of the first [17, 9, 4] tokens of a free generation, all of it through forced decode steps: the same
    kernels run the same steps, so tokens and logits are those of the free generation bit for bit"""
    e = eng if mode == "f32" else eng_bf16
    c = short
    kw = dict(temperature=1.0, seed=12345) if seeded else dict(temperature=1.0, noise=c.noise.cuda())
    start = c.z[:, 0].cuda()
    c.context(e)
    tok, lg = e.generate(start, c.m8, c.T, return_logits=True, **kw)
    prompt = torch.cat([start[:, None].to(torch.int32), tok[:, :16]], 1).contiguous()
    c.context(e)
    ptok, plg = e.generate(None, c.m8, c.T, return_logits=True, prompt=prompt, prompt_len=_plen_t([17, 9, 4]), no_prefill=True, **kw)
    assert torch.equal(tok, ptok)
    assert torch.equal(lg, plg)


# ---- 3 and 4
# (2, 2, None) and (3, 3, None): the shortest prefills, one and two positions
SHORT_CFG = [(17, 17, None), (17, 4, (17, 9, 4)), (2, 2, None), (39, 39, None), (3, 3, None)]


def _check_prefill(e, c, Pmax, P0, plen, noisy):
    ref_tok, ref_lg = c.oracle(Pmax, plen, noisy)
    prompt = c.z[:, :Pmax].to(torch.int32).cuda().contiguous()
    c.context(e, prompt_frames=P0)
    free_tok, _ = c.run(e, noisy)
    c.context(e, prompt_frames=P0)
    tok, lg = c.run(e, noisy, prompt=prompt, prompt_len=_plen_t(plen), prefill=P0)
    c.context(e, prompt_frames=P0)
    ftok, flg = c.run(e, noisy, prompt=prompt, prompt_len=_plen_t(plen), no_prefill=True)
    n0 = P0 - 1
    e_first = (lg[:, n0] - ref_lg[:, n0]).abs().max().item()
    e_steps = (lg[:, n0:] - ref_lg[:, n0:]).abs().max().item()
    e_forced = (lg[:, n0:] - flg[:, n0:]).abs().max().item()
    eff = [Pmax] * c.B if plen is None else [min(max(p, P0), Pmax) for p in plen]
    gen = torch.zeros_like(tok, dtype=torch.bool)
    for b, p in enumerate(eff):
        gen[b, p - 1:] = True
    differ = (tok != free_tok)[gen].float().mean().item()
    print("prefill B=%d T=%d Pmax=%d P0=%d plen=%s noisy=%d: |logits - oracle| first step %.2e, all steps %.2e; "
          "|prefill - forced steps| %.2e; generated tokens that differ from the free generation %.3f (%d)"
          % (c.B, c.T, Pmax, P0, plen, noisy, e_first, e_steps, e_forced, differ, int(gen.sum())))
    # 3: against the oracle
    assert torch.equal(tok, ref_tok), "%d tokens differ from the oracle" % int((tok != ref_tok).sum())
    assert e_steps < STEP_TOL
    assert e_first < LOGIT_TOL
    assert n0 == 0 or float(lg[:, :n0].abs().max()) == 0.0
    assert differ > 0.5, "the prompt is ignored?"
    # 4: against the forced decode steps
    assert torch.equal(tok, ftok)
    assert e_forced < STEP_TOL


@pytest.mark.parametrize("noisy", [False, True])
@pytest.mark.parametrize("Pmax,P0,plen", SHORT_CFG)
def test_prefill_matches_oracle_and_forced_steps(eng, short, Pmax, P0, plen, noisy):
    _check_prefill(eng, short, Pmax, P0, plen, noisy)


@pytest.mark.parametrize("noisy", [False, True])
def test_prefill_across_a_row_tile_matches_oracle_and_forced_steps(eng, long_, noisy):
    _check_prefill(eng, long_, 131, 131, None, noisy)


# ---- 5
def test_bf16_prefill_error_is_the_decode_steps_error(eng_bf16, short, long_):
    """bf16: both paths round K/V to bf16 and differ only in summation order and in which kernel formed the rows, so the
    prefill's error against the f32 oracle at the first decode step may be at most twice the forced-step path's own error
    (+ 1e-3), and greedy first generated tokens agree (>= 90 %).
    Measured on MI355X (max |logits - f32 oracle| at the first decode step, prefill / forced steps): T = 40, P0 = 17:
    6.607e-3 / 6.827e-3; T = 150, P0 = 131: 6.793e-3 / 5.446e-3; T = 40, P0 = 2: 7.917e-3 / 6.039e-3; all 8 first generated
    tokens equal."""
    e = eng_bf16
    first_a, first_b = [], []
    for c, P in ((short, 17), (long_, 131), (short, 2)):   # 2: the shortest prefill, one position
        _, ref_lg = c.oracle(P, None, False)
        prompt = c.z[:, :P].to(torch.int32).cuda().contiguous()
        c.context(e, prompt_frames=P)
        tok, lg = c.run(e, False, prompt=prompt, prefill=P)
        c.context(e, prompt_frames=P)
        ftok, flg = c.run(e, False, prompt=prompt, no_prefill=True)
        e_prefill = (lg[:, P - 1] - ref_lg[:, P - 1]).abs().max().item()
        e_steps = (flg[:, P - 1] - ref_lg[:, P - 1]).abs().max().item()
        print("bf16 T=%d P0=%d: first decode step max |logits - f32 oracle|: prefill %.3e, forced steps %.3e" % (c.T, P, e_prefill, e_steps))
        assert e_prefill <= 2 * e_steps + 1e-3
        first_a.append(tok[:, P - 1])
        first_b.append(ftok[:, P - 1])
    agree = (torch.cat(first_a) == torch.cat(first_b)).float().mean().item()
    print("bf16: first generated tokens of the two paths that agree: %.2f" % agree)
    assert agree >= 0.9


def test_bf16_layer_chain_path_with_a_prompt(eng_bf16, full_sd):
    """bf16, more than 128 clips: the decode step's attention half runs as the XCD-local layer kernel, whose counters' epoch is
    the number of steps done in the call -- not the step index, which starts at P0 - 1 after a prefill.  No chain fault may
    be reported, the forced steps reproduce the free generation bit for bit, and the prefill path continues it alike."""
    e = eng_bf16
    B, T, P = 130, 12, 5
    c = _Case(full_sd, B, T, tuple([T] * 100 + [7] * 30))
    faults = e.lib.dimx_chain_faults(e.h)
    c.context(e, prompt_frames=P)
    tok = e.generate(c.z[:, 0].cuda(), c.m8, T, 0.0).cpu()
    prompt = torch.cat([c.z[:, :1].to(torch.int32), tok[:, :P - 1]], 1).cuda().contiguous()
    c.context(e, prompt_frames=P)
    ftok = e.generate(None, c.m8, T, 0.0, prompt=prompt, no_prefill=True).cpu()
    c.context(e, prompt_frames=P)
    ptok = e.generate(None, c.m8, T, 0.0, prompt=prompt, prefill=P).cpu()
    assert e.lib.dimx_chain_faults(e.h) == faults
    assert torch.equal(ftok, tok)
    assert torch.equal(ptok[:, :P - 1], tok[:, :P - 1])
    agree = (ptok[:, P - 1] == tok[:, P - 1]).float().mean().item()
    print("bf16 B=%d: first generated tokens after a prefill that equal the free generation's: %.3f" % (B, agree))
    assert agree >= 0.9   # the bar of test 5 (and of tests/test_gpu_s2s.py for a kernel swap in the bf16 mode)


# ---- 6
def test_samples_share_the_prefill(eng, full_sd):
    B, T, S, P = 2, 40, 5, 9
    c = _Case(full_sd, B, T, (40, 33))
    prompt = c.z[:, :P].to(torch.int32).cuda().contiguous()
    c.context(eng, prompt_frames=P, n_samples=S)
    tok = eng.generate(None, c.m8, T, 1.0, 52, None, 7, n_samples=S, prompt=prompt, prefill=P).cpu()
    assert tok.shape == (B * S, T - 1)
    for r in range(B * S):
        assert torch.equal(tok[r, :P - 1], prompt[r // S, 1:].cpu())
    try:
        for b in range(B):
            for s in range(S):
                eng.set_shard(b * S + s, B * S)   # the global row of sample s of clip b
                eng.encode_ctx(c.v_s[b:b + 1].cuda(), c.v_a[b:b + 1].cuda(), c.m8[b:b + 1].contiguous(), True, prompt_frames=P)
                one = eng.generate(None, c.m8[b:b + 1].contiguous(), T, 1.0, 52, None, 7, prompt=prompt[b:b + 1].contiguous(), prefill=P).cpu()
                assert torch.equal(one[0], tok[b * S + s]), "clip %d sample %d" % (b, s)
    finally:
        eng.set_shard(0, 0)


# ---- 7
def test_groups_graphs_and_another_prefix_give_the_same_tokens(full_sd):
    """The handle exposes no capture counter, so this shows what a caller can see: another P0 on the same handle, and replays
    of both, give the same tokens with and without graphs.  That P0 is not in GraphKey is a statement about the code (P0 only
    sets the device counter's start and the number of graph launches), not something this test observes."""
    from dimx import engine, lib
    B, T, P = 4, 30, 11
    c = _Case(full_sd, B, T, (30, 30, 21, 12))
    prompt = c.z[:, :P].to(torch.int32).cuda().contiguous()
    full_len = torch.full((B,), P, dtype=torch.int32).cuda()
    outs = []
    try:
        for no_graph, groups in (("0", "1"), ("1", "1"), ("0", "2"), ("1", "2")):
            os.environ["DIMX_NO_GRAPH"] = no_graph
            os.environ["DIMX_GEN_GROUPS"] = groups
            e = engine.Engine("cuda:0", lib.MODE_PARITY_F32)
            e.load_state_dict(full_sd)
            c.context(e, prompt_frames=P)
            a = e.generate(None, c.m8, T, 1.0, 52, c.noise.cuda(), prompt=prompt, prefill=P).cpu()
            # another P0 on the same handle (the rest of the prompt is forced), then replays of both
            c.context(e, prompt_frames=P)
            b = e.generate(None, c.m8, T, 1.0, 52, c.noise.cuda(), prompt=prompt, prompt_len=full_len, prefill=5).cpu()
            c.context(e, prompt_frames=P)
            a2 = e.generate(None, c.m8, T, 1.0, 52, c.noise.cuda(), prompt=prompt, prefill=P).cpu()
            c.context(e, prompt_frames=P)
            b2 = e.generate(None, c.m8, T, 1.0, 52, c.noise.cuda(), prompt=prompt, prompt_len=full_len, prefill=5).cpu()
            e.close()
            assert torch.equal(a, b) and torch.equal(a, a2) and torch.equal(a, b2), "no_graph=%s groups=%s" % (no_graph, groups)
            outs.append(a)
    finally:
        os.environ.pop("DIMX_NO_GRAPH", None)
        os.environ.pop("DIMX_GEN_GROUPS", None)
    for o in outs[1:]:
        assert torch.equal(o, outs[0])


def test_bf16_prefill_with_samples_and_with_clip_groups(full_sd):
    """bf16: the prefill in front of the multi-sample decode path (S = 5: the clip's cache rows are broadcast, cross attention
    on the matrix-core kernel) and in front of two clip groups.  Prompt columns repeat the prompt in every row; the first
    generated tokens (greedy) equal those of the forced-step path in at least 90 % of the rows, the bar of test 5."""
    from dimx import engine, lib
    B, T, S, P = 4, 30, 5, 11
    c = _Case(full_sd, B, T, (30, 30, 21, 12))
    prompt = c.z[:, :P].to(torch.int32).cuda().contiguous()
    want = prompt[:, 1:].clamp(min=0).cpu()
    try:
        for groups, s in (("1", S), ("2", 1)):
            os.environ["DIMX_GEN_GROUPS"] = groups
            e = engine.Engine("cuda:0", lib.MODE_PERF_BF16)
            e.load_state_dict(full_sd)
            c.context(e, prompt_frames=P, n_samples=s)
            tok = e.generate(None, c.m8, T, 0.0, n_samples=s, prompt=prompt, prefill=P).cpu()
            c.context(e, prompt_frames=P, n_samples=s)
            ftok = e.generate(None, c.m8, T, 0.0, n_samples=s, prompt=prompt, no_prefill=True).cpu()
            e.close()
            for r in range(B * s):
                assert torch.equal(tok[r, :P - 1], want[r // s]) and torch.equal(ftok[r, :P - 1], want[r // s])
            agree = (tok[:, P - 1] == ftok[:, P - 1]).float().mean().item()
            print("bf16 groups=%s S=%d: first generated tokens, prefill == forced steps: %.2f" % (groups, s, agree))
            assert agree >= 0.9
    finally:
        os.environ.pop("DIMX_GEN_GROUPS", None)


# ---- 8
def _clips(B, T, lens, seed=5):
    from dimx import prng
    v_s = torch.from_numpy(prng.normal(seed, "m.vs", (B, T, 56)))
    v_l = torch.from_numpy(prng.normal(seed, "m.vl", (B, T, 56)))
    v_a = torch.from_numpy(prng.normal(seed, "m.va", (B, T, 768)))
    mask = torch.zeros(B, T, dtype=torch.bool)
    for j, n in enumerate(lens):
        mask[j, :n] = True
    return v_s, v_l, v_a, mask


@pytest.fixture(scope="module")
def model():
    from dimx.seq2seq_pretrain import SLMFT
    return SLMFT().eval()


def test_prompt_frames_through_the_model(model):
    B, T, lens, P = 3, 40, [40, 33, 7], 17
    v_s, v_l, v_a, mask = [t.cuda() for t in _clips(B, T, lens)]
    _, z_l = model.forward_vq(v_s, v_l, mask, with_speaker=False)
    tot, d, pred, tok = model(v_s, v_l, v_a, mask, mode="val", greedy=True, prompt_frames=P, lengths=lens, return_tokens=True)
    assert tok.shape == (B, T - 1) and pred.shape == (B, T - 1, 56)
    for b, n in enumerate(lens):
        plen = min(n, P)
        assert torch.equal(tok[b, :plen - 1], z_l[b, 1:plen])
    assert torch.equal(pred, model.forward_vq_decoder(tok, "val"))
    # without host lengths the common prefix costs one .item(); the result is the same
    tok2 = model(v_s, v_l, v_a, mask, mode="val", greedy=True, prompt_frames=P, return_tokens=True)[3]
    assert torch.equal(tok, tok2)
    free = model(v_s, v_l, v_a, mask, mode="val", greedy=True, return_tokens=True)[3]
    assert not torch.equal(free[0, P - 1:], tok[0, P - 1:])


@pytest.mark.parametrize("fd_backend", ["reference", "device", "hip"])
def test_evaluate_test_epoch_with_prompt_frames(model, fd_backend):
    import numpy as np
    from dimx import x_engine_pt
    torch.manual_seed(1234)     # the sampling seeds are drawn from torch's generator
    T = 32
    loader, all_lens = [], []
    for i, lens in enumerate(([32, 20, 11], [32, 25])):
        v_s, v_l, v_a, mask = _clips(len(lens), T, lens, seed=30 + i)
        src = torch.cat([v_s, v_a], -1) * mask[..., None]
        loader.append((src, v_l * mask[..., None], lens, None, ["clip%d_%d" % (i, j) for j in range(len(lens))]))
        all_lens += lens
    y_true, y_pred, x, ids = x_engine_pt.evaluate_test_epoch(model, loader, torch.device("cuda:0"), beam_size=2, prompt_frames=17,
                                                             fd_backend=fd_backend)
    assert len(y_true) == len(x) == len(ids) == 5
    assert [a.shape for a in y_pred] == [(n - 1, 56) for n in all_lens] and all(np.isfinite(a).all() for a in y_pred)


# ---- 9
def test_bad_arguments_return_their_error_without_a_launch(eng, short):
    from dimx import engine, lib as L
    c = short
    B, T = c.B, c.T
    c.context(eng)
    prompt = c.z.to(torch.int32).cuda().contiguous()
    tokens = torch.full((B, T - 1), -7, dtype=torch.int32).cuda()
    ws, wsb = eng.workspace(B, T)

    def call(e, Pmax, P0, ws_bytes, ws_ptr=None):
        return e.lib.dimx_generate_prompted(e.h, L.ptr(prompt), T, None, Pmax, P0, L.ptr(c.m8), B, T, 1, 0.0, 52, None, 0, L.ptr(tokens),
                                            None, 0, ws_ptr if ws_ptr is not None else ws, ws_bytes, eng._s())

    assert call(eng, T, 1, wsb) == ERR_ARG          # Pmax = T
    assert call(eng, 17, 18, wsb) == ERR_ARG        # P0 > Pmax
    slm = engine.Engine("cuda:0", L.MODE_PARITY_F32, variant="slm")
    rc = call(slm, 17, 17, wsb)
    assert rc == ERR_ARG and b"variant" in slm.lib.dimx_last_error()
    slm.close()
    small = eng.lib.dimx_workspace_bytes_samples(eng.h, B, T, 1)
    big = eng.lib.dimx_workspace_bytes_prompt(eng.h, B, T, 1, 17)
    assert eng.lib.dimx_workspace_bytes_prompt(eng.h, B, T, 1, 1) == small and big >= small
    torch.cuda.synchronize()
    assert bool((tokens == -7).all()), "a refused call launched something"
    if big == small:
        pytest.skip("the prompt workspace at P0 = 17 is no larger than dimx_workspace_bytes_samples at B = %d, T = %d" % (B, T))
    assert call(eng, 17, 17, small) == ERR_WORKSPACE
    torch.cuda.synchronize()
    assert bool((tokens == -7).all()), "a refused call launched something"
