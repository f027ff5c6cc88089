"""GPU: classifier-free guidance -- the guided sampler kernel (dimx_op_sample_guided) against dimx.guidance and against the plain
sampler on its own guided rows, and the guided generation (dimx_generate_guided) against the CPU checker tests/guidance_ref.py,
against teacher-forced passes under the real and the null context, and against itself (workspace contents, scale 1, graph replay,
the window, prompts, scores, bf16).  Synthetic SLMFT weights."""
import numpy as np
import pytest
import torch

from test_gpu_prompt import STEP_TOL, _case
from test_gpu_sampler_filters import EXCLUDE_CAP, FILTERS, MARGIN

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
ERR_ARG, ERR_STATE, ERR_WORKSPACE = -1, -4, -5
SCALE = 0.125
SCALES = [0.0, 1.0, 1.5, 3.0]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- the operator
def _rows(R, lscale, what):
    from dimx import prng
    return prng.normal(21, "guidance.op.%s.%d.%d" % (what, R, lscale), (R, 512)) * np.float32(lscale)


def _op_noise(R):
    from dimx import prng
    return prng.exponential(22, "guidance.op.noise.%d" % R, (R, 512))


def _slabs(x, nslab):
    """nslab f32 slabs whose in-order f32 sum is returned with them (the kernel adds slab 0, 1, 2, ... in this order)"""
    from dimx import prng
    if nslab == 1:
        return x[None].copy(), x
    parts = [prng.normal(23, "guidance.op.slab.%d.%d" % (x.shape[0], i), x.shape) for i in range(nslab - 1)]
    first = x - np.sum(parts, axis=0, dtype=np.float32)
    slabs = np.stack([first] + parts).astype(np.float32)
    tot = slabs[0].copy()
    for s in slabs[1:]:
        tot = tot + s
    return slabs, tot


@pytest.mark.parametrize("nslab", [1, 3])
@pytest.mark.parametrize("lscale", [1, 3])
@pytest.mark.parametrize("R", [5, 256, 1030])      # one wave per block (odd, full) / four waves per block with a ragged last block
def test_guided_rows_against_the_definition(R, lscale, nslab):
    from dimx import engine, guidance
    cs, c = _slabs(_rows(R, lscale, "c"), nslab)
    us, u = _slabs(_rows(R, lscale, "u"), nslab)
    cg, ug = (torch.from_numpy(cs).cuda(), torch.from_numpy(us).cuda()) if nslab > 1 else (torch.from_numpy(c).cuda(), torch.from_numpy(u).cuda())
    for scale in SCALES:
        tok, g = engine.op_sample_guided(cg, ug, scale, temperature=0.0)
        g = g.cpu().numpy()
        want, bound = guidance.combine(c, u, scale), guidance.combine_bound(c, u, scale)
        err = np.abs(g.astype(np.float64) - want)
        print("R=%d logits x%d nslab=%d scale=%.1f: max |guided - combine| / bound = %.3f" % (R, lscale, nslab, scale, (err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all()
        if scale == 1.0:
            assert np.array_equal(_bits(g), _bits(c))                 # the conditional row's bits
        tok = tok.cpu().numpy()
        assert np.array_equal(tok[:R], g.argmax(1)) and np.array_equal(tok[R:], tok[:R])


@pytest.mark.parametrize("lscale", [1, 3])
@pytest.mark.parametrize("R", [5, 256, 1030])
def test_token_is_the_plain_sampler_on_the_guided_rows(R, lscale):
    """the same device body: exact equality, whatever the filter; the unconditional half gets the same token"""
    from dimx import engine
    cg, ug = torch.from_numpy(_rows(R, lscale, "c")).cuda(), torch.from_numpy(_rows(R, lscale, "u")).cuda()
    qg = torch.from_numpy(_op_noise(R)).cuda()
    moved = 0
    for scale in SCALES:
        for kind, kw in [("top_k", {"k": 52})] + FILTERS:
            for temperature in (1.0, 0.7):
                tok, g = engine.op_sample_guided(cg, ug, scale, temperature=temperature, noise=qg, filter_logits_fn=kind, filter_kwargs=kw)
                want = engine.op_sample(g, temperature=temperature, noise=qg, filter_logits_fn=kind, filter_kwargs=kw)
                assert torch.equal(tok[:R], want) and torch.equal(tok[R:], want), (scale, kind, kw, temperature)
                again, g2 = engine.op_sample_guided(cg, ug, scale, temperature=temperature, noise=qg, filter_logits_fn=kind, filter_kwargs=kw)
                assert torch.equal(again, tok) and torch.equal(g2, g)          # repeats are bit-identical
        # the counter-based generator: row r of an R-row launch, salted by the step
        a, g = engine.op_sample_guided(cg, ug, scale, noise=None, seed=9001, step=3)
        assert torch.equal(a[:R], engine.op_sample(g, noise=None, seed=9001, step=3))
        if R >= 256:
            assert not torch.equal(a, engine.op_sample_guided(cg, ug, scale, noise=None, seed=9001, step=4)[0])
        plain = engine.op_sample(cg, temperature=1.0, noise=qg)
        moved += int(scale != 1.0 and not torch.equal(engine.op_sample_guided(cg, ug, scale, noise=qg)[0][:R], plain))
    if R >= 256:
        assert moved == 3          # every scale but 1 samples other tokens than the conditional rows would


def test_invalid_scale_and_slabs_are_refused_before_the_launch():
    from dimx import lib
    L = lib.load()
    cg, ug = torch.from_numpy(_rows(5, 1, "c")).cuda(), torch.from_numpy(_rows(5, 1, "u")).cuda()
    out = torch.full((10,), -7, dtype=torch.int32).cuda()
    g = torch.full((5, 512), -7.0).cuda()

    def call(scale=1.5, nslab=1, stride=5 * 512, kind=0, a=0.0):
        return L.dimx_op_sample_guided(lib.ptr(cg), lib.ptr(ug), 5, nslab, stride, scale, kind, 52, a, 0.0, 1.0, None, 5, 0, lib.ptr(out), lib.ptr(g),
                                       lib.stream_ptr(cg.device))
    for bad in (float("nan"), float("inf"), float("-inf")):
        assert call(scale=bad) == ERR_ARG
    assert call(nslab=0) == ERR_ARG and call(nslab=9) == ERR_ARG and call(nslab=2, stride=5 * 512 - 1) == ERR_ARG
    assert call(kind=1, a=float("nan")) == ERR_ARG and call(kind=4) == ERR_ARG
    torch.cuda.synchronize()
    assert (out == -7).all() and (g == -7.0).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert (out >= 0).all()


# ---------------------------------------------------------------------------------------------------------------- the generation
B, T, LENS = 3, 40, (40, 33, 17)            # an odd B: the row-slice offsets of the unconditional half are unaligned
WIDE = (130, 12)                            # 2B = 260 rows: the halves split inside a GEMM row tile
PMAX, PLEN = 5, (5, 3, 4)


class _Gen:
    """inputs of one shape and the oracle's context, built once and left unchanged"""

    def __init__(self, sd, B, T, lens):
        import prompt_ref
        from dimx import prng
        self.sd, self.B, self.T = sd, B, T
        self.v_s, self.v_a, self.z, self.mask = _case(B, T, list(lens))
        self.noise = torch.from_numpy(prng.exponential(11, "guidance.gen.noise.%d" % B, (T - 1, B, 512)))
        self.ctx = prompt_ref.case_context(sd, self.v_s, self.v_a, self.mask)
        self.m8 = self.mask.to(torch.uint8).cuda()

    def context(self, eng, v_s=None, v_a=None):
        eng.encode_ctx((self.v_s if v_s is None else v_s).cuda(), (self.v_a if v_a is None else v_a).cuda(), self.m8, True, guided=True)

    def run(self, eng, scale, noisy, v_s=None, v_a=None, **kw):
        """-> tokens [B,n] int64, guided logits [B,n,512], branch logits [2,B,n,512] (numpy)"""
        self.context(eng, v_s, v_a)
        tok, lg, br = eng.generate(self.z[:, 0].cuda(), self.m8, self.T, 1.0 if noisy else 0.0, 52, self.noise.cuda() if noisy else None,
                                   return_logits=True, guidance=scale, return_branches=True, **kw)
        return tok.cpu().numpy().astype(np.int64), lg.cpu().numpy(), br.cpu().numpy()

    def checker(self, tok, scale, noisy, **kw):
        import guidance_ref
        return guidance_ref.guided_generate(self.sd, kw.pop("prompt", self.z[:, :1]), kw.pop("plen", None), self.T - 1, self.ctx, self.mask, scale,
                                            noise=self.noise if noisy else None, temperature=1.0 if noisy else 0.0, force=tok, **kw)


def _engine(sd, mode="f32"):
    from dimx import engine, lib
    e = engine.Engine("cuda:0", lib.MODE_PARITY_F32 if mode == "f32" else lib.MODE_PERF_BF16)
    e.load_state_dict(sd)
    return e


@pytest.fixture(scope="module")
def eng(full_sd):
    return _engine(full_sd)


@pytest.fixture(scope="module")
def gen(full_sd):
    return _Gen(full_sd, B, T, LENS)


def _structure(what, g, tok, lg, br, scale, noisy, kind="top_k", kw=None, free=None):
    """what holds in either numeric mode: the guided dump is combine(branch dumps) within the kernel's bound, and every free step's
    token is the definition's on that step's own guided logits"""
    from dimx import guidance, sampling
    kw = {"k": 52} if kw is None else kw
    want, bound = guidance.combine(br[0], br[1], scale), guidance.combine_bound(br[0], br[1], scale)
    assert (np.abs(lg.astype(np.float64) - want) <= bound).all()
    if scale == 1.0:
        assert np.array_equal(_bits(lg), _bits(br[0]))
    R, n = tok.shape
    free = np.ones((R, n), dtype=bool) if free is None else free
    excluded = mismatches = rows = 0
    for t in range(n):
        sel = free[:, t]
        if not sel.any():
            continue
        l = lg[sel, t]
        if noisy:
            q = g.noise[t].numpy()[sel]
            bad = sampling.undecidable(l, kind, MARGIN, noise=q, temperature=1.0, **kw)
            ref = sampling.sample_ref(l, q, 1.0, kind, **kw)
        else:
            bad = np.zeros(len(l), dtype=bool)            # the arg-max of the step's own float32 row: nothing to round
            ref = l.argmax(1)
        rows += int(sel.sum())
        excluded += int(bad.sum())
        mismatches += int((tok[sel, t][~bad] != ref[~bad]).sum())
    print("%-56s excluded %3d / %4d steps (%.2f %%), mismatches on decidable steps: %d" % (what, excluded, rows, 100.0 * excluded / rows, mismatches))
    assert excluded <= EXCLUDE_CAP * rows
    assert mismatches == 0


def _against_checker(what, g, tok, lg, br, scale, noisy, **kw):
    """the branch dumps against the checker FORCED ALONG THE DEVICE'S TOKENS: a near tie costs one pair, not the rest of the clip"""
    ref = g.checker(tok, scale, noisy, **kw)
    ec = np.abs(br[0] - ref["cond"].numpy()).max()
    eu = np.abs(br[1] - ref["uncond"].numpy()).max()
    eg = np.abs(lg - ref["guided"]).max()
    print("%-56s max |cond - checker| %.2e, |uncond - checker| %.2e, |guided - checker| %.2e; branches differ by %.2f"
          % (what, ec, eu, eg, np.abs(br[0] - br[1]).max()))
    assert ec < STEP_TOL and eu < STEP_TOL
    assert np.abs(br[0] - br[1]).max() > 0.1
    return ref


# Share of (clip, step) pairs the definition alone leaves out at MARGIN, computed on the CPU with the checker's own free-running
# guided logits before the seeds were fixed: 0 of 117 pairs in each of the top-k cases below (scales 0 / 1.5 / 3, greedy and noisy,
# the window, the ragged prompt), 1 of 117 (0.85 %) under top_p 0.9, 0 of 1430 for the wide case -- far below EXCLUDE_CAP.
@pytest.mark.parametrize("noisy", [False, True])
@pytest.mark.parametrize("scale", [1.5, 0.0])
def test_generation_matches_the_checker(eng, gen, scale, noisy):
    tok, lg, br = gen.run(eng, scale, noisy)
    assert tok.shape == (B, T - 1) and lg.shape == (B, T - 1, 512) and br.shape == (2, B, T - 1, 512)
    what = "guided scale=%.1f noisy=%d" % (scale, noisy)
    _against_checker(what, gen, tok, lg, br, scale, noisy)
    _structure(what, gen, tok, lg, br, scale, noisy)


def test_both_halves_saw_the_same_tokens_and_the_second_no_context(eng, gen):
    tok, lg, br = gen.run(eng, 3.0, True)
    z = torch.cat([gen.z[:, :1], torch.from_numpy(tok)], dim=1).cuda()
    eng.encode_ctx(gen.v_s.cuda(), gen.v_a.cuda(), gen.m8, False)
    tf_c = eng.decode_tf(z, gen.m8)[0].cpu().numpy()
    # zero rows after the concat [x + patch_embed_dec_s | audio]: x = -patch_embed_dec_s, audio = 0
    x_null = (-gen.sd["patch_embed_dec_s"]).reshape(1, 1, -1).expand(B, T, -1).contiguous().cuda()
    eng.set_context(x_null, torch.zeros_like(gen.v_a).cuda(), which_patch=0, for_generate=False)
    tf_u = eng.decode_tf(z, gen.m8)[0].cpu().numpy()
    ec, eu = np.abs(tf_c - br[0]).max(), np.abs(tf_u - br[1]).max()
    print("teacher-forced along the run's tokens: max |cond dump - real context| %.2e, |uncond dump - zero context| %.2e" % (ec, eu))
    assert ec < STEP_TOL and eu < STEP_TOL
    assert np.abs(tf_c - br[1]).max() > 0.1


def test_unconditional_half_does_not_depend_on_the_speaker(eng, gen):
    """along a fully forced prompt (the tokens do depend on the speaker through the guided row) the unconditional dump keeps its bits
    when speaker frames and audio are replaced"""
    from dimx import prng
    prompt = gen.z[:, :T - 1].to(torch.int32).cuda().contiguous()
    tok, lg, br = gen.run(eng, 1.5, True, prompt=prompt)
    v_s2 = torch.from_numpy(prng.normal(31, "guidance.other.vs", (B, T, 56)))
    v_a2 = torch.from_numpy(prng.normal(31, "guidance.other.va", (B, T, 768)))
    tok2, lg2, br2 = gen.run(eng, 1.5, True, v_s=v_s2, v_a=v_a2, prompt=prompt)
    assert np.array_equal(tok[:, :T - 3], gen.z[:, 1:T - 2].clamp(min=0).numpy()) and np.array_equal(tok2[:, :T - 3], tok[:, :T - 3])
    assert np.array_equal(_bits(br[1]), _bits(br2[1]))
    assert np.abs(br[0] - br2[0]).max() > 0.1 and not np.array_equal(lg, lg2)


def test_workspace_contents_do_not_matter(full_sd, gen):
    e = _engine(full_sd)
    try:
        need = e.lib.dimx_workspace_bytes_guided(e.h, B, T)
        assert need > e.lib.dimx_workspace_bytes(e.h, B, T) and need == e.lib.dimx_workspace_bytes_samples(e.h, B, T, 2)
        e.workspace(B, T, guided=True)
        out = []
        for fill in (0xFF, 0x00):
            e._ws.fill_(fill)
            out.append(gen.run(e, 1.5, True))
        (tok_f, lg_f, br_f), (tok_0, lg_0, br_0) = out
        assert np.array_equal(tok_f, tok_0) and np.array_equal(_bits(lg_f), _bits(lg_0)) and np.array_equal(_bits(br_f), _bits(br_0))
        assert np.isfinite(out[0][1]).all() and np.isfinite(out[0][2]).all()
    finally:
        e.close()


def test_scale_one_is_the_conditional_row_and_a_new_scale_replays_the_graph(full_sd, eng, gen):
    tok1, lg1, br1 = gen.run(eng, 1.0, True)
    assert np.array_equal(_bits(lg1), _bits(br1[0]))
    tok3, lg3, br3 = gen.run(eng, 3.0, True)               # same shapes and buffers as the call before: the step graphs are replayed
    assert not np.array_equal(tok1, tok3)
    assert np.array_equal(_bits(br1[:, :, 0]), _bits(br3[:, :, 0]))       # the first step does not depend on the scale ...
    assert not np.array_equal(lg1[:, 0], lg3[:, 0])                       # ... its guided row does
    _structure("replay: scale 3 after scale 1", gen, tok3, lg3, br3, 3.0, True)
    fresh = _engine(full_sd)
    try:
        ftok, flg, fbr = gen.run(fresh, 3.0, True)
    finally:
        fresh.close()
    assert np.array_equal(tok3, ftok) and np.array_equal(_bits(lg3), _bits(flg)) and np.array_equal(_bits(br3), _bits(fbr))
    # a plain generation on the same handle afterwards is what a fresh handle generates
    plain = _plain(eng, gen)
    fresh = _engine(full_sd)
    try:
        want = _plain(fresh, gen)
    finally:
        fresh.close()
    assert torch.equal(plain[0], want[0]) and torch.equal(plain[1], want[1])


def _plain(e, g):
    e.encode_ctx(g.v_s.cuda(), g.v_a.cuda(), g.m8, True)
    return e.generate(g.z[:, 0].cuda(), g.m8, g.T, 1.0, 52, g.noise.cuda(), return_logits=True)


def test_generation_under_the_window(eng, gen):
    tok, lg, br = gen.run(eng, 1.5, True, lookahead=0)
    assert eng.cross_lookahead() is None
    _against_checker("guided scale=1.5 lookahead=0", gen, tok, lg, br, 1.5, True, lookahead=0)
    _structure("guided scale=1.5 lookahead=0", gen, tok, lg, br, 1.5, True)
    off = gen.run(eng, 1.5, True)
    assert not np.array_equal(br[0], off[2][0])
    assert np.array_equal(_bits(br[1][:, 0]), _bits(off[2][1][:, 0]))      # the window is the conditional half's alone


def test_generation_with_a_ragged_forced_prompt(eng, gen):
    prompt = gen.z[:, :PMAX].to(torch.int32).cuda().contiguous()
    plen = torch.tensor(PLEN, dtype=torch.int32).cuda()
    tok, lg, br = gen.run(eng, 1.5, True, prompt=prompt, prompt_len=plen)
    free = np.ones((B, T - 1), dtype=bool)
    for b, p in enumerate(PLEN):
        free[b, :p - 1] = False
        assert np.array_equal(tok[b, :p - 1], gen.z[b, 1:p].numpy())
    _against_checker("guided scale=1.5 ragged prompt", gen, tok, lg, br, 1.5, True, prompt=gen.z[:, :PMAX], plen=PLEN)
    _structure("guided scale=1.5 ragged prompt", gen, tok, lg, br, 1.5, True, free=free)


def test_generation_with_a_sampler_filter(eng, gen):
    tok, lg, br = gen.run(eng, 1.5, True, filter_logits_fn="top_p", filter_kwargs={"thres": 0.9})
    _structure("guided scale=1.5 top_p 0.9", gen, tok, lg, br, 1.5, True, kind="top_p", kw={"thres": 0.9})
    tok2, lg2, br2 = gen.run(eng, 1.5, True)
    _structure("guided scale=1.5 after the filtered call (top-k 52)", gen, tok2, lg2, br2, 1.5, True)


def test_scores_are_taken_under_the_guided_logits(eng, gen):
    from dimx import engine
    from dimx.scoring import scored_columns
    gen.context(eng)
    tok, lg, sc = eng.generate(gen.z[:, 0].cuda(), gen.m8, T, 1.0, 52, gen.noise.cuda(), return_logits=True, return_scores=True, guidance=1.5)
    first, last = scored_columns(T, T - 1, gen.m8.sum(1, dtype=torch.int32), None)
    want = engine.op_seq_logprob(lg, tok, first, last)
    assert torch.equal(sc.score, want.score) and torch.equal(sc.count, want.count)
    assert sc.count.cpu().tolist() == [n - 1 for n in LENS]


def test_wide_batch_splits_inside_a_row_tile(eng, full_sd):
    Bw, Tw = WIDE
    g = _Gen(full_sd, Bw, Tw, (Tw,) * Bw)
    tok, lg, br = g.run(eng, 1.5, True)
    _against_checker("guided scale=1.5 B=%d T=%d" % WIDE, g, tok, lg, br, 1.5, True)
    _structure("guided scale=1.5 B=%d T=%d" % WIDE, g, tok, lg, br, 1.5, True)


def test_bf16_mode_is_self_consistent(full_sd, eng, gen):
    """structure only: the combine bound, token against own logits, the scale-1 identity; the distance to f32 is reported"""
    e = _engine(full_sd, "bf16")
    try:
        for scale in (1.5, 1.0):
            tok, lg, br = gen.run(e, scale, True)
            _structure("bf16 guided scale=%.1f" % scale, gen, tok, lg, br, scale, True)
        prompt = gen.z[:, :T - 1].to(torch.int32).cuda().contiguous()
        _, _, b16 = gen.run(e, 1.5, True, prompt=prompt)
        _, _, b32 = gen.run(eng, 1.5, True, prompt=prompt)
        print("bf16 against f32 along a forced prompt: max |cond| difference %.3e, |uncond| %.3e (reported, not bounded)"
              % (np.abs(b16[0] - b32[0]).max(), np.abs(b16[1] - b32[1]).max()))
    finally:
        e.close()


def test_what_guidance_does_not_take_is_refused(eng, gen):
    from dimx import lib
    gen.context(eng)
    start = gen.z[:, :1].to(torch.int32).cuda().contiguous()
    tok = torch.full((B, T - 1), -7, dtype=torch.int32).cuda()
    ws, wsb = eng.workspace(B, T, guided=True)

    def call(scale=1.5, Pmax=1, wsb=wsb):
        return eng.lib.dimx_generate_guided(eng.h, lib.ptr(start), 1, None, Pmax, lib.ptr(gen.m8), B, T, scale, 1.0, 52, None, 5, lib.ptr(tok), None, None,
                                            ws, wsb, lib.stream_ptr(tok.device))
    for bad in (float("nan"), float("inf")):
        assert call(scale=bad) == ERR_ARG
    assert call(Pmax=2) == ERR_ARG                                   # ld_prompt < Pmax
    assert call(wsb=eng.lib.dimx_workspace_bytes(eng.h, B, T)) == ERR_WORKSPACE
    torch.cuda.synchronize()
    assert (tok == -7).all()
    with pytest.raises(lib.DimxError):
        eng.generate(gen.z[:, 0].cuda(), gen.m8, T, guidance=1.5, n_samples=2)
    with pytest.raises(ValueError):
        eng.generate(gen.z[:, 0].cuda(), gen.m8, T, return_branches=True)
    sess = eng.stream(B, T, gen.z[:, 0].cuda())
    try:
        assert call() == ERR_STATE
    finally:
        sess.close()
    gen.context(eng)
    assert call() == 0
    torch.cuda.synchronize()
    assert (tok >= 0).all()


# ---------------------------------------------------------------------------------------------------------------- the host layers
@pytest.fixture(scope="module")
def model(full_sd):
    from dimx import lib
    from dimx.seq2seq_pretrain import SLMFT
    m = SLMFT(numeric_mode=lib.MODE_PARITY_F32).eval()
    m.load_state_dict({k: v.clone() for k, v in full_sd.items()}, strict=False)
    return m.cuda()


def _listener(g):
    from dimx import prng
    return torch.from_numpy(prng.normal(9, "guidance.vl", (g.B, g.T, 56)))


def test_module_forward_takes_the_guided_route(model, gen):
    v_s, v_l, v_a, mask = gen.v_s.cuda(), _listener(gen).cuda(), gen.v_a.cuda(), gen.mask.cuda()
    noise = gen.noise.cuda()
    out = {}
    for s in (None, 1.0, 3.0):
        _, _, pred, tok = model(v_s, v_l, v_a, mask, mode="val", noise=noise, return_tokens=True, guidance=s)
        assert tuple(pred.shape) == (B, T - 1, 56) and tuple(tok.shape) == (B, T - 1)
        out[s] = tok.cpu()
    assert not torch.equal(out[3.0], out[1.0])
    # what the engine generates from the module's own codes
    _, z_l = model.forward_vq(v_s, v_l, mask, with_speaker=False)
    eng = model.engine(v_s.device)
    eng.encode_ctx(v_s, v_a, gen.m8, True, guided=True)
    tok = eng.generate(z_l[:, 0], gen.m8, T, 1.0, 52, noise, guidance=3.0)
    assert torch.equal(tok.cpu().long(), out[3.0])
    _, _, _, tok5, sc = model(v_s, v_l, v_a, mask, mode="val", noise=noise, return_tokens=True, return_scores=True, guidance=3.0,
                              prompt_frames=5)
    assert torch.equal(tok5[:, :4].cpu(), z_l[:, 1:5].cpu().long())        # every clip here is longer than the prompt
    assert sc.count.cpu().tolist() == [max(n - 5, 0) for n in LENS]
    for bad in (dict(n_samples=2), dict(beam_width=2, num_return=1), dict(mode="train")):
        with pytest.raises(ValueError):
            model(v_s, v_l, v_a, mask, **dict(dict(mode="val", guidance=1.5), **bad))


def test_null_context_score_and_pmi(model, gen):
    from dimx import guidance, prng
    v_s, v_l, v_a, mask = gen.v_s.cuda(), _listener(gen).cuda(), gen.v_a.cuda(), gen.mask.cuda()
    _, z_l = model.forward_vq(v_s, v_l, mask, with_speaker=False)
    cond = model.score(v_s, v_l, v_a, mask, z_l=z_l)
    null = model.score(v_s, v_l, v_a, mask, z_l=z_l, context="null")
    v_s2 = torch.from_numpy(prng.normal(31, "guidance.other.vs", (B, T, 56))).cuda()
    v_a2 = torch.from_numpy(prng.normal(31, "guidance.other.va", (B, T, 768))).cuda()
    null2 = model.score(v_s2, v_l, v_a2, mask, z_l=z_l, context="null")
    assert torch.equal(null.score, null2.score) and torch.equal(null.count, cond.count)
    assert not torch.equal(null.score, cond.score)
    got = model.pmi(v_s, v_l, v_a, mask, z_l=z_l)
    want = (cond.score.cpu().numpy() - null.score.cpu().numpy()) / cond.count.cpu().numpy()
    assert got.shape == (B,) and np.array_equal(got, want) and np.array_equal(got, guidance.pmi(cond, null))
    with pytest.raises(ValueError):
        model.score(v_s, v_l, v_a, mask, context="null", lookahead=0)
    # the null-context score is the unconditional branch's: a fully forced guided generation dumps the same logits within STEP_TOL
    eng = model.engine(v_s.device)
    eng.encode_ctx(v_s, v_a, gen.m8, True, guided=True)
    _, br = eng.generate(None, gen.m8, T, 0.0, 52, None, prompt=z_l[:, :T - 1].to(torch.int32).contiguous(), guidance=1.5, return_branches=True)
    from dimx import engine
    from dimx.scoring import scored_columns
    first, last = scored_columns(T, T - 1, gen.m8.sum(1, dtype=torch.int32))
    dumped = engine.op_seq_logprob(br[1], z_l[:, 1:], first, last)
    err = (dumped.score - null.score).abs().max().item()
    print("null-context score: decode_tf against the guided step's unconditional dump: max |difference| %.2e over %d tokens" % (err, int(null.count.sum())))
    assert err < 2 * STEP_TOL * int(null.count.max())       # a log-probability moves by at most twice the largest logit difference
