"""GPU: online generation (dimx_set_cross_lookahead) -- the windowed cross form of the one-query attention kernels against the
plain form, the generation against the CPU checker of tests/online_ref.py, its offline limit, causality in the speaker, graph
replay across settings, samples, ragged prompts, the layer-kernel shape, SLMFT.score and the host layers."""
import os

import numpy as np
import pytest
import torch

from test_gpu_prompt import LOGIT_TOL, SHORT, STEP_TOL, _case, _clips, _noise

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
MIN_MARGIN = 2 * LOGIT_TOL   # a checker decision closer than this may fall the other way on the device (tests/test_online_host.py)
MAX_LEFT_OUT = 0.02
ERR_ARG = -1
SCALE = 0.125


# ---------------------------------------------------------------- 1: the kernel
def _vis(t, L, n):
    from dimx.online import visible
    return visible(t, L, n)


# (step, lookahead): the issue's grid, then steps that put vis = step + 2 one below, at and one above a key batch (16 keys in f32,
# 32 in bf16; with 2 / 4 waves per pair the batches of 16 alternate between the waves, so 16 and 32 are both wave boundaries)
WIN_GRID = [(t, L) for t in (0, 1, 6, 35, 38) for L in (0, -3, 4, 100, -100)] + [(t, 0) for t in (13, 14, 15, 29, 30, 31)]


@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_windowed_cross_form_is_the_plain_form_over_the_visible_keys(dtype, S):
    from dimx import engine as E
    dev = torch.device("cuda:0")
    B, H, Tmax, n = 2, 12, 40, 37
    dt = torch.bfloat16 if dtype == "bf16" else torch.float32
    g = torch.Generator().manual_seed(77 + S)
    q = torch.randn(2, B * S, H * 64, generator=g).to(dev)            # two f32 split-K slabs, as generate's projection writes them
    kc = torch.randn(B, H, Tmax, 64, generator=g).to(dt)
    vc = torch.randn(B, H, Tmax, 64, generator=g).to(dt)
    km = torch.ones(B, Tmax, dtype=torch.uint8)
    km[0, [0, 3, 4, 17, 30, 31, 36]] = 0
    km[1, 20:] = 0
    km[1, 5] = 0
    km = km.to(dev)
    kcd, vcd = kc.to(dev), vc.to(dev)
    seen = set()
    for nsplit in ((1, 2, 4) if S == 1 else (0,)):
        for t, L in WIN_GRID:
            vis = _vis(t, L, n)
            seen.add(vis)
            step = torch.tensor([t], dtype=torch.int32, device=dev)
            plain = E.op_decode_attn_ex(q, kcd, vcd, SCALE, n_keys=vis, kmask=km, kmask_ld=Tmax, rows_per_clip=S, nsplit=nsplit, q_f32=True)
            # rows at or past vis may not be read: NaN there; the masked rows below vis keep their values
            kp, vp = kc.clone(), vc.clone()
            kp[:, :, vis:] = float("nan")
            vp[:, :, vis:] = float("nan")
            win = E.op_decode_attn_ex(q, kp.to(dev), vp.to(dev), SCALE, n_keys=n, step=step, kmask=km, kmask_ld=Tmax, rows_per_clip=S,
                                      nsplit=nsplit, q_f32=True, lookahead=L)
            assert bool(torch.isfinite(win.float()).all()), (t, L, nsplit)
            assert torch.equal(win, plain), "step %d lookahead %d nsplit %d: vis %d" % (t, L, nsplit, vis)
    assert {1, 2, 15, 16, 17, 31, 32, 33, 37} <= seen


def test_windowed_form_needs_a_step_counter():
    from dimx import engine as E
    from dimx import lib as L
    dev = torch.device("cuda:0")
    kc = torch.zeros(2, 12, 40, 64, device=dev)
    q = torch.zeros(2, 12 * 64, device=dev)
    with pytest.raises(L.DimxError):
        E.op_decode_attn_ex(q, kc, kc, SCALE, n_keys=37, lookahead=0)


# ---------------------------------------------------------------- the generation
class _Short:
    """the SHORT inputs of tests/test_gpu_prompt.py, the oracle's encoder output and context, and the checker's runs, computed once"""

    def __init__(self, sd):
        import prompt_ref
        from oracle import ref_cpu
        self.sd = sd
        self.B, self.T, self.lens = SHORT
        self.v_s, self.v_a, self.z, self.mask = _case(self.B, self.T, list(self.lens))
        self.noise = _noise(self.B, self.T)
        self.x_s = ref_cpu.slmft_forward_encoder(sd, self.v_s, self.mask)
        self.ctx = prompt_ref.case_context(sd, self.v_s, self.v_a, self.mask)
        self.m8 = self.mask.to(torch.uint8).cuda()
        self._ref = {}

    def checker(self, L, noisy, Pmax=1, plen=None):
        import online_ref
        key = (L, noisy, Pmax, None if plen is None else tuple(plen))
        if key not in self._ref:
            self._ref[key] = online_ref.online_generate(self.sd, self.z[:, :Pmax], plen, self.T - 1, self.ctx, self.mask, L,
                                                        self.noise if noisy else None)
        return self._ref[key]

    def context(self, eng, **kw):
        eng.encode_ctx(self.v_s.cuda(), self.v_a.cuda(), self.m8, True, **kw)

    def run(self, eng, noisy, lookahead, **kw):
        self.context(eng)
        tok, lg = eng.generate(self.z[:, 0].cuda(), self.m8, self.T, 1.0 if noisy else 0.0, 52, self.noise.cuda() if noisy else None,
                               return_logits=True, lookahead=lookahead, **kw)
        return tok.cpu().long(), lg.cpu()


def _engine(sd, mode="f32"):
    from dimx import engine, lib
    e = engine.Engine("cuda:0", lib.MODE_PARITY_F32 if mode == "f32" else lib.MODE_PERF_BF16)
    e.load_state_dict(sd)
    return e


@pytest.fixture(scope="module")
def eng(full_sd):
    return _engine(full_sd)


@pytest.fixture(scope="module")
def eng_bf16(full_sd):
    return _engine(full_sd, "bf16")


@pytest.fixture(scope="module")
def short(full_sd):
    return _Short(full_sd)


def _against_checker(what, tok, lg, ref, tokens=True):
    """logits within STEP_TOL and tokens equal on every (row, step) before the row's first near-tie of the checker; the near-tie
    step's own logits still belong to the common history and are compared too"""
    import online_ref
    ref_tok, ref_lg, margins = ref
    keep, left_out = online_ref.compared_steps(margins, MIN_MARGIN)
    keep_lg = keep.clone()
    keep_lg[:, 1:] |= keep[:, :-1]
    keep_lg[:, 0] = True
    err = (lg - ref_lg).abs().amax(-1)
    wrong = int(((tok != ref_tok) & keep).sum())
    print("%s: max |logits - checker| %.2e over the compared steps (%.2e over all), %d compared tokens differ, smallest margin %.2e, "
          "pairs left out %.4f" % (what, err[keep_lg].max().item(), err.max().item(), wrong, margins.min().item(), left_out))
    assert left_out <= MAX_LEFT_OUT
    assert err[keep_lg].max().item() < STEP_TOL
    if tokens:
        assert wrong == 0
    return left_out


# ---- 2
@pytest.mark.parametrize("noisy", [False, True])
@pytest.mark.parametrize("L", [SHORT[1], 0, -3])
def test_generation_matches_the_checker(eng, short, L, noisy):
    tok, lg = short.run(eng, noisy, L)
    left_out = _against_checker("L=%d noisy=%d" % (L, noisy), tok, lg, short.checker(L, noisy))
    assert left_out == 0.0     # tests/test_online_host.py: none of these cases has a near-tie


def test_generation_with_a_lookahead_buffer_matches_the_checker_logits(eng, short):
    tok, lg = short.run(eng, True, 4)
    _against_checker("L=4 noisy=1", tok, lg, short.checker(4, True), tokens=False)


# ---- 3
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("noisy", [False, True])
def test_full_lookahead_is_the_window_off(eng, eng_bf16, short, mode, noisy):
    e = eng if mode == "f32" else eng_bf16
    off_tok, off_lg = short.run(e, noisy, None)
    assert e.cross_lookahead() is None
    tok, lg = short.run(e, noisy, short.T)
    assert e.cross_lookahead() is None      # generate(lookahead=) restores the setting
    assert torch.equal(tok, off_tok) and torch.equal(lg, off_lg)
    tok2, lg2 = short.run(e, noisy, short.T - 2)
    assert torch.equal(tok2, off_tok) and torch.equal(lg2, off_lg)
    tok0, _ = short.run(e, noisy, 0)
    assert (tok0 != off_tok).float().mean().item() > 0.5


# ---- 4
def _run_on_context(eng, c, x_s, v_a, lookahead):
    eng.set_context(x_s.cuda(), v_a.cuda(), which_patch=0, for_generate=True)
    tok, lg = eng.generate(c.z[:, 0].cuda(), c.m8, c.T, 0.0, return_logits=True, lookahead=lookahead)
    return tok.cpu(), lg.cpu()


@pytest.mark.parametrize("L", [0, -3])
def test_steps_do_not_see_a_perturbed_future(eng, short, L):
    c = short
    P = 20
    x_s2, v_a2 = c.x_s.clone(), c.v_a.clone()
    x_s2[:, P:] += 0.5
    v_a2[:, P:] -= 0.5
    tok, lg = _run_on_context(eng, c, c.x_s, c.v_a, L)
    tok2, lg2 = _run_on_context(eng, c, x_s2, v_a2, L)
    last = P - 2 - L      # the last step with vis(t) = t + 2 + L <= P
    assert torch.equal(lg[:, :last + 1], lg2[:, :last + 1]) and torch.equal(tok[:, :last + 1], tok2[:, :last + 1])
    assert not torch.equal(lg[0, last + 1], lg2[0, last + 1]) and not torch.equal(lg[1, last + 1], lg2[1, last + 1])


def test_offline_generation_sees_the_future_from_its_first_step(eng, short):
    c = short
    x_s2, v_a2 = c.x_s.clone(), c.v_a.clone()
    x_s2[:, 20:] += 0.5
    v_a2[:, 20:] -= 0.5
    _, lg = _run_on_context(eng, c, c.x_s, c.v_a, None)
    _, lg2 = _run_on_context(eng, c, x_s2, v_a2, None)
    assert not torch.equal(lg[0, 0], lg2[0, 0]) and not torch.equal(lg[1, 0], lg2[1, 0])
    _, on = _run_on_context(eng, c, c.x_s, c.v_a, 0)
    _, on2 = _run_on_context(eng, c, x_s2, v_a2, 0)
    assert torch.equal(on[:, 0], on2[:, 0])


# ---- 5
def test_graph_replay_never_reuses_another_setting(full_sd, short):
    c = short
    fresh = {}
    for L in (0, 5, None):
        e = _engine(full_sd)
        if L is not None:
            e.set_cross_lookahead(L)
            assert e.cross_lookahead() == L
        fresh[L] = c.run(e, True, None)       # the handle's own setting
        e.close()
    assert not torch.equal(fresh[0][0], fresh[5][0]) and not torch.equal(fresh[0][0], fresh[None][0])
    e = _engine(full_sd)
    try:
        for L in (0, 5, None, 0):
            e.set_cross_lookahead(L)
            tok, lg = c.run(e, True, None)
            assert torch.equal(tok, fresh[L][0]) and torch.equal(lg, fresh[L][1]), "setting %s after another one" % (L,)
    finally:
        e.close()


# ---- 5b: the same rule across everything that selects the step's route (csrc/generate.hip resolve_route, GraphKey)
def _route_calls(B, T, lens):
    v_s, v_a, z, mask = _case(B, T, list(lens))
    v_s, v_a, m8 = v_s.cuda(), v_a.cuda(), mask.to(torch.uint8).cuda()
    start = z[:, 0].cuda()
    prompt = z[:, :5].to(torch.int32).cuda().contiguous()
    plen = torch.tensor([5, 4, 3], dtype=torch.int32).cuda()

    def plain(e, **kw):
        e.encode_ctx(v_s, v_a, m8, True)
        return e.generate(start, m8, T, 1.0, 52, None, seed=2024, return_logits=True, **kw)

    def samples(e):
        e.encode_ctx(v_s, v_a, m8, True, n_samples=4)
        return e.generate(start, m8, T, 1.0, 52, None, seed=2024, return_logits=True, n_samples=4)

    def prompted(e):
        e.encode_ctx(v_s, v_a, m8, True, prompt_frames=3)
        return e.generate(None, m8, T, 1.0, 52, None, seed=2024, return_logits=True, prompt=prompt, prompt_len=plen, prefill=3)

    def beam(e):
        e.encode_ctx(v_s, v_a, m8, True, n_samples=4)
        return e.generate_beam(start, m8, T, 4, return_logits=True, return_backptr=True)

    def window_on(e):
        e.set_cross_lookahead(1)
        return plain(e)

    def window_off(e):
        e.set_cross_lookahead(None)
        return plain(e)

    def top_p(e):
        return plain(e, filter_logits_fn="top_p", filter_kwargs={"thres": 0.8})

    return [("seeded", plain), ("n_samples 4", samples), ("prompted", prompted), ("beam", beam), ("window on", window_on),
            ("window off", window_off), ("top_p", top_p), ("top_k again", plain), ("seeded again", plain)]


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_graph_replay_never_belongs_to_another_route(full_sd, mode):
    calls = _route_calls(3, 12, (12, 9, 5))
    fresh = {}
    for _, fn in calls:
        if fn not in fresh:
            e = _engine(full_sd, mode)
            fresh[fn] = [t.cpu() for t in fn(e)]
            e.close()
    e = _engine(full_sd, mode)
    try:
        got = [[t.cpu() for t in fn(e)] for _, fn in calls]
    finally:
        e.close()
    for (name, fn), out in zip(calls, got):
        assert len(out) == len(fresh[fn])
        for i, (a, b) in enumerate(zip(out, fresh[fn])):
            assert torch.equal(a, b), "%s after the calls before it: output %d differs from a fresh engine's" % (name, i)
    for a, b in zip(got[-1], got[0]):
        assert torch.equal(a, b)
    assert not torch.equal(got[0][0], got[4][0]) or not torch.equal(got[0][1], got[4][1])   # the window changes the result


# ---- 6
def test_samples_match_the_checker_row_by_row(eng, full_sd):
    import online_ref
    import prompt_ref
    from dimx import prng
    B, T, S, L = 2, 40, 5, 0
    v_s, v_a, z, mask = _case(B, T, [40, 33])
    noise = torch.from_numpy(prng.exponential(11, "s2s.noise", (T - 1, B * S, 512)))
    ctx = prompt_ref.case_context(full_sd, v_s, v_a, mask)
    ref = online_ref.online_generate(full_sd, z[:, :1].repeat_interleave(S, 0), None, T - 1, ctx.repeat_interleave(S, 0),
                                     mask.repeat_interleave(S, 0), L, noise)
    m8 = mask.to(torch.uint8).cuda()
    eng.encode_ctx(v_s.cuda(), v_a.cuda(), m8, True, n_samples=S)
    tok, lg = eng.generate(z[:, 0].cuda(), m8, T, 1.0, 52, noise.cuda(), return_logits=True, n_samples=S, lookahead=L)
    assert tok.shape == (B * S, T - 1)
    _against_checker("S=%d L=%d" % (S, L), tok.cpu().long(), lg.cpu(), ref)
    assert len({tuple(r.tolist()) for r in tok.cpu()}) > B     # the samples of a clip are different sequences


# ---- 7
@pytest.mark.parametrize("noisy", [False, True])
def test_ragged_prompt_runs_through_forced_steps(eng, short, noisy):
    c = short
    Pmax, P0, plen, L = 17, 4, (17, 9, 4), 0
    prompt = c.z[:, :Pmax].to(torch.int32).cuda().contiguous()
    plen_t = torch.tensor(plen, dtype=torch.int32).cuda()
    c.context(eng, prompt_frames=P0)
    tok, lg = eng.generate(None, c.m8, c.T, 1.0 if noisy else 0.0, 52, c.noise.cuda() if noisy else None, return_logits=True,
                           prompt=prompt, prompt_len=plen_t, prefill=P0, lookahead=L)
    c.context(eng, prompt_frames=P0)
    ftok, flg = eng.generate(None, c.m8, c.T, 1.0 if noisy else 0.0, 52, c.noise.cuda() if noisy else None, return_logits=True,
                             prompt=prompt, prompt_len=plen_t, no_prefill=True, lookahead=L)
    assert torch.equal(tok, ftok) and torch.equal(lg, flg)
    for b, p in enumerate(plen):
        assert torch.equal(tok[b, :p - 1].cpu(), prompt[b, 1:p].cpu())
    _against_checker("ragged prompt noisy=%d" % noisy, tok.cpu().long(), lg.cpu(), c.checker(L, noisy, Pmax, plen))


# ---- 8
def test_bf16_layer_kernel_shape_takes_the_per_op_launches(full_sd):
    """130 clips in bf16: with the window off the attention half of a layer is the decoder-layer kernel.  The window takes the
    launches a handle without that kernel takes, so with every row visible it reproduces that handle bit for bit."""
    from dimx import engine, lib
    B, T = 130, 12
    v_s, v_a, z, mask = _case(B, T, [T] * 100 + [7] * 30)
    m8 = mask.to(torch.uint8).cuda()

    def run(e, lookahead):
        e.encode_ctx(v_s.cuda(), v_a.cuda(), m8, True)
        tok, lg = e.generate(z[:, 0].cuda(), m8, T, 0.0, return_logits=True, lookahead=lookahead)
        return tok.cpu(), lg.cpu()

    os.environ["DIMX_NO_LAYER_CHAIN"] = "1"
    try:
        plain = _engine(full_sd, "bf16")
    finally:
        os.environ.pop("DIMX_NO_LAYER_CHAIN", None)
    ref_tok, ref_lg = run(plain, None)
    assert plain.lib.dimx_chain_faults(plain.h) == 0
    plain.close()
    e = _engine(full_sd, "bf16")
    tok, lg = run(e, T)
    faults = e.lib.dimx_chain_faults(e.h)
    e.close()
    assert faults == 0
    assert torch.equal(tok, ref_tok) and torch.equal(lg, ref_lg)


# ---- 9, 10
@pytest.fixture(scope="module")
def model():
    from dimx.seq2seq_pretrain import SLMFT
    return SLMFT().eval()


def test_score_under_online_visibility(model):
    import online_ref
    import prompt_ref
    from dimx import scoring
    B, T, lens = 3, 40, [40, 33, 7]
    v_s, v_l, v_a, mask = _clips(B, T, lens)
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    dev = [t.cuda() for t in (v_s, v_l, v_a, mask)]
    _, z_l = model.forward_vq(dev[0], dev[1], dev[3], with_speaker=False)
    z = z_l.cpu().long()
    ctx = prompt_ref.case_context(sd, v_s, v_a, mask)
    _, ref_lg, _ = online_ref.online_generate(sd, z[:, :T - 1], None, T - 1, ctx, mask, 0)
    first, last = scoring.scored_columns(T, T - 1, lens)
    ref = scoring.sequence_scores(ref_lg.numpy(), z[:, 1:].numpy(), first, last)
    on = model.score(*dev, lookahead=0)
    full = model.score(*dev, lookahead=T)
    off = model.score(*dev)
    count = on.count.cpu().numpy()
    assert np.array_equal(count, ref.count) and np.array_equal(count, [n - 1 for n in lens])
    assert np.array_equal(full.count.cpu().numpy(), off.count.cpu().numpy())
    d_on = np.abs(on.score.cpu().numpy() - ref.score) / count
    d_full = np.abs(full.score.cpu().numpy() - off.score.cpu().numpy()) / count
    print("score(lookahead=0) against the checker: per-token log-probability differs by %s; score(lookahead=T) against score(): %s; "
          "perplexity offline %.2f, lookahead 0 %.2f" % (d_on, d_full, scoring.perplexity(off), scoring.perplexity(on)))
    # a log-softmax moves by at most twice the largest logit error
    assert d_on.max() <= 2 * STEP_TOL and d_full.max() <= 2 * STEP_TOL
    # withholding the future changes the likelihood by more than the bound above could hide
    assert (np.abs(on.score.cpu().numpy() - off.score.cpu().numpy()) / count).max() > 2 * STEP_TOL


def test_forward_with_a_lookahead(model):
    B, T, lens = 3, 40, [40, 33, 7]
    v_s, v_l, v_a, mask = [t.cuda() for t in _clips(B, T, lens)]
    tot, d, pred, tok = model(v_s, v_l, v_a, mask, mode="val", greedy=True, return_tokens=True)
    tot0, d0, pred0, tok0 = model(v_s, v_l, v_a, mask, mode="val", greedy=True, lookahead=0, return_tokens=True)
    assert tok0.shape == tok.shape == (B, T - 1) and pred0.shape == pred.shape == (B, T - 1, 56)
    assert not torch.equal(tok0, tok) and bool(torch.isfinite(pred0).all())
    assert torch.equal(pred0, model.forward_vq_decoder(tok0, "val"))
    full = model(v_s, v_l, v_a, mask, mode="val", greedy=True, lookahead=T, return_tokens=True)[3]
    assert torch.equal(full, tok)
    assert model.engine(v_s.device).cross_lookahead() is None
    with pytest.raises(ValueError):
        model(v_s, v_l, v_a, mask, mode="train", lookahead=0)
    with pytest.raises(ValueError):
        model(v_s, v_l, v_a, mask, mode="val", lookahead=0, beam_width=2)


def test_evaluate_test_epoch_with_a_lookahead(model):
    from dimx import x_engine_pt
    T = 32
    loader, all_lens = [], []
    for i, lens in enumerate(([32, 20, 11], [32, 25])):
        v_s, v_l, v_a, mask = _clips(len(lens), T, lens, seed=30 + i)
        src = torch.cat([v_s, v_a], -1) * mask[..., None]
        loader.append((src, v_l * mask[..., None], lens, None, ["clip%d_%d" % (i, j) for j in range(len(lens))]))
        all_lens += lens
    out = {}
    for L in (None, 0):
        torch.manual_seed(1234)     # the sampling seeds are drawn from torch's generator
        out[L] = x_engine_pt.evaluate_test_epoch(model, loader, torch.device("cuda:0"), beam_size=2, lookahead=L)
    for y_true, y_pred, x, ids in out.values():
        assert len(y_true) == len(x) == len(ids) == 5
        assert [a.shape for a in y_pred] == [(n - 1, 56) for n in all_lens] and all(np.isfinite(a).all() for a in y_pred)
    assert any(not np.array_equal(a, b) for a, b in zip(out[None][1], out[0][1]))
    with pytest.raises(ValueError):
        x_engine_pt.evaluate_test_epoch(model, loader, torch.device("cuda:0"), decode="beam", beam_width=2, lookahead=0)


# ---- 11
def test_bad_arguments_return_their_error_without_a_launch(eng, short):
    from dimx import engine, lib as L
    c = short
    B, T, W = c.B, c.T, 2
    c.context(eng, n_samples=W)
    start = c.z[:, :1].to(torch.int32).cuda().contiguous()
    tokens = torch.full((B * W, T - 1), -7, dtype=torch.int32).cuda()
    scores = torch.full((B * W,), -7.0, dtype=torch.float64).cuda()
    state = torch.empty(2 * B * W, dtype=torch.float64).cuda()
    ws, wsb = eng.workspace(B, T, W)
    eng.set_cross_lookahead(0)
    try:
        rc = eng.lib.dimx_generate_beam(eng.h, L.ptr(start), 1, None, 1, 1, L.ptr(c.m8), None, B, T, W, L.ptr(tokens), L.ptr(scores), None, None,
                                        L.ptr(state), state.numel() * 8, 0, ws, wsb, eng._s())
        assert rc == ERR_ARG and b"window" in eng.lib.dimx_last_error()
    finally:
        eng.set_cross_lookahead(None)
    torch.cuda.synchronize()
    assert bool((tokens == -7).all()) and bool((scores == -7.0).all()), "a refused call launched something"
    for variant in ("slm", "legacy"):
        other = engine.Engine("cuda:0", L.MODE_PARITY_F32, variant=variant)
        rc = other.lib.dimx_set_cross_lookahead(other.h, 1, 0)
        assert rc == ERR_ARG and b"variant" in other.lib.dimx_last_error()
        with pytest.raises(L.DimxError):
            other.set_cross_lookahead(0)
        assert other.cross_lookahead() is None
        other.close()
