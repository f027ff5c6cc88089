"""GPU: beam search (dimx_generate_beam, dimx_op_beam_step, dimx_op_beam_reorder; csrc/beam.hip) against its float64 definition
dimx.beam, against the library's own greedy and teacher-forced passes, against the CPU oracle loop of tests/beam_ref.py, and the host
layers above it.

BOUND is the project's bound for its float64 operators (1e-11 per token, tests/test_gpu_seq_score.py); STEP_TOL / LOGIT_TOL are those
of tests/test_gpu_s2s.py.  TAU: see test_against_the_cpu_oracle."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
BOUND = 1e-11
LOGIT_TOL, STEP_TOL = 1e-4, 2e-3
SHORT = (3, 40, (40, 33, 7))     # tests/test_gpu_prompt.py
PROMPT = dict(Pmax=17, plen=(17, 9, 4), prefill=4)
WIDTHS = (1, 2, 4, 5, 8, 10)
ERR_ARG = -1
# Oracle comparison: decisions whose oracle margin is below TAU may legitimately differ.  Measured on MI355X: the largest
# |running score (HIP) - running score (oracle)| over the agreed steps is 3.4e-6 (W = 2) / 5.5e-6 (W = 4); TAU = 10 x that, rounded up.
TAU = 6e-5


def _dev():
    return torch.device("cuda:0")


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


class _Case:
    """the SHORT clips: host inputs and their device copies, computed once and left unchanged"""

    def __init__(self):
        self.B, self.T, self.lens = SHORT
        self.v_s, self.v_a, self.z, self.mask = _case(self.B, self.T, list(self.lens))
        self.m8 = self.mask.to(torch.uint8).to(_dev())
        self.prompt = self.z[:, :PROMPT["Pmax"]].to(torch.int32).to(_dev()).contiguous()
        self.plen = torch.tensor(PROMPT["plen"], dtype=torch.int32).to(_dev())

    def context(self, eng, n_samples=1, prompt_frames=1, for_generate=True, repeat=1):
        rep = (lambda t: t.repeat_interleave(repeat, 0)) if repeat > 1 else (lambda t: t)
        eng.encode_ctx(rep(self.v_s).to(_dev()), rep(self.v_a).to(_dev()), rep(self.m8).contiguous(), for_generate, n_samples=n_samples,
                       prompt_frames=prompt_frames)

    def beam(self, eng, W, prompted=False, **kw):
        if prompted:
            self.context(eng, W, PROMPT["prefill"])
            return eng.generate_beam(None, self.m8, self.T, W, prompt=self.prompt, prompt_len=self.plen, prefill=PROMPT["prefill"], **kw)
        self.context(eng, W)
        return eng.generate_beam(self.z[:, 0].to(_dev()), self.m8, self.T, W, **kw)

    def columns(self, prompted):
        """(first, last, first decode step) of the SHORT clips"""
        from dimx import scoring
        first, last = scoring.scored_columns(self.T, self.T - 1, list(self.lens), list(PROMPT["plen"]) if prompted else None)
        return np.asarray(first), np.asarray(last), PROMPT["prefill"] - 1 if prompted else 0


@pytest.fixture(scope="module")
def engines(full_sd):
    from dimx import engine, lib
    out = {}
    for name, mode in (("f32", lib.MODE_PARITY_F32), ("bf16", lib.MODE_PERF_BF16)):
        out[name] = engine.Engine("cuda:0", mode)
        out[name].load_state_dict(full_sd)
    return out


@pytest.fixture(scope="module")
def clips():
    return _Case()


def _close(a, b):
    """|a - b| within BOUND x max(1, |b|); infinities must agree exactly"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    fin = np.isfinite(b)
    return np.array_equal(a[~fin], b[~fin]) and bool((np.abs(a[fin] - b[fin]) <= BOUND * np.maximum(1.0, np.abs(b[fin]))).all())


# ---- 1
@pytest.mark.parametrize("scale", [1, 3])
@pytest.mark.parametrize("W", WIDTHS)
def test_op_beam_step_matches_the_definition(W, scale):
    """Measured on MI355X: worst |cum' - definition| 8.9e-16 over the twelve cases; smallest margin of the inputs 1.3e-2."""
    from dimx import beam, prng
    from dimx.engine import op_beam_step
    logits = (prng.normal(31, "beam.logits", (3 * W, 512)) * scale).astype(np.float32)
    cum = -np.abs(prng.normal(31, "beam.cum", (3, W))) * 5
    if W > 1:
        cum[0, W - 1] = cum[1, 0] = cum[2, W // 2] = -np.inf
    mode, forced = [beam.LIVE, beam.FORCED, beam.FROZEN], [0, 77, 0]
    keep, order = beam.margins(logits[:W], cum[0])
    print("W=%d scale %d: margins of the live clip %.3e (keep) %.3e (order)" % (W, scale, keep, order))
    assert min(keep, order) > 1e-9, "a condition on the inputs"
    ref = [beam.beam_step(logits[b * W:(b + 1) * W], cum[b], mode[b], forced[b]) for b in range(3)]
    lg, cm = torch.from_numpy(logits).to(_dev()), torch.from_numpy(cum.reshape(-1)).to(_dev())
    parent, token, new = op_beam_step(lg, cm, mode, forced, beam_width=W)
    assert np.array_equal(parent.cpu().numpy(), np.concatenate([r[0] for r in ref]))
    assert np.array_equal(token.cpu().numpy(), np.concatenate([r[1] for r in ref]))
    want = np.concatenate([r[2] for r in ref])
    got = new.cpu().numpy()
    fin = np.isfinite(want)
    print("worst |cum' - definition| %.3e" % (np.abs(got[fin] - want[fin]).max() if fin.any() else 0.0))
    assert _close(got, want)
    again = op_beam_step(lg, cm, mode, forced, beam_width=W)
    assert torch.equal(again[0], parent) and torch.equal(again[1], token) and torch.equal(again[2].view(torch.int64), new.view(torch.int64))


def test_op_beam_step_first_live_step_and_arguments():
    from dimx import beam, prng
    from dimx.engine import op_beam_step
    from dimx import lib as L
    W = 5
    logits = prng.normal(32, "beam.logits", (W, 512)).astype(np.float32)
    parent, token, new = op_beam_step(torch.from_numpy(logits).to(_dev()), torch.from_numpy(beam.start_scores(W)).to(_dev()), [beam.LIVE],
                                      beam_width=W)
    ref = beam.beam_step(logits, beam.start_scores(W))
    assert parent.cpu().tolist() == [0] * W and np.array_equal(token.cpu().numpy(), ref[1]) and _close(new.cpu().numpy(), ref[2])
    with pytest.raises(L.DimxError):
        op_beam_step(torch.zeros(6, 512, device=_dev()), torch.zeros(6, dtype=torch.float64, device=_dev()), [0, 0], beam_width=3)
    with pytest.raises(L.DimxError):
        op_beam_step(torch.zeros(4, 512), torch.zeros(4, dtype=torch.float64), [0], beam_width=4)


# ---- 2
def _parents(W, kind):
    ident = list(range(W))
    if kind == "swap":
        p = [w ^ 1 if (w ^ 1) < W else w for w in ident]
    elif kind == "cycle":
        p = [(w + 1) % W for w in ident]
    else:
        p = [min(2, W - 1)] * W
    return ident + p       # clip 0 keeps the identity, clip 1 is permuted


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("W", WIDTHS[1:])
def test_op_beam_reorder(W, dtype):
    from dimx.engine import op_beam_reorder
    R, H, T = 2 * W, 2, 9
    gen = torch.Generator().manual_seed(5)
    src = torch.randn(R, H, T, 64, generator=gen).to(dtype).to(_dev())
    for kind in ("identity", "swap", "cycle", "equal"):
        parent = list(range(W)) * 2 if kind == "identity" else _parents(W, kind)      # parents count within the clip
        rows = torch.tensor([r // W * W + parent[r] for r in range(R)], device=_dev())
        for c in (0, 4, 8):
            cache = src.clone()
            cache[:, :, c + 1:] = 7.0         # the sentinel past position c
            want = cache.clone()
            want[:, :, :c + 1] = cache[rows][:, :, :c + 1]
            out = op_beam_reorder(cache, parent, c, W)
            assert out.data_ptr() == cache.data_ptr()
            assert torch.equal(out.view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                               want.view(torch.int16 if dtype == torch.bfloat16 else torch.int32)), (kind, c)
            assert bool((out[:, :, c + 1:] == 7.0).all()) and torch.equal(out[:W, :, :c + 1], src[:W, :, :c + 1])


def test_op_beam_reorder_arguments():
    from dimx import lib as L
    from dimx.engine import op_beam_reorder
    cache = torch.zeros(4, 2, 9, 64, device=_dev())
    for bad in (dict(c=9, beam_width=2), dict(c=-1, beam_width=2), dict(c=0, beam_width=3)):
        with pytest.raises(L.DimxError):
            op_beam_reorder(cache, [0, 1, 0, 1], **bad)
    with pytest.raises(L.DimxError):
        op_beam_reorder(torch.zeros(4, 2, 9, 64), [0, 1, 0, 1], 0, 2)
    out_of_range = op_beam_reorder(torch.ones(4, 2, 9, 64, device=_dev()), [0, 1, 5, -2], 8, 2)      # such a clip is left alone
    assert bool((out_of_range == 1).all())


# ---- 3
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("prompted", [False, True], ids=["free", "prompted"])
def test_width_one_is_greedy(engines, clips, mode, prompted):
    e, c = engines[mode], clips
    if prompted:
        c.context(e, 1, PROMPT["prefill"])
        tok, lg = e.generate(None, c.m8, c.T, 0.0, return_logits=True, prompt=c.prompt, prompt_len=c.plen, prefill=PROMPT["prefill"])
    else:
        c.context(e)
        tok, lg = e.generate(c.z[:, 0].to(_dev()), c.m8, c.T, 0.0, return_logits=True)
    btok, score, blg, bp = c.beam(e, 1, prompted, return_logits=True, return_backptr=True)
    assert torch.equal(btok, tok) and torch.equal(blg.view(torch.int32), lg.view(torch.int32))
    first, last, step0 = c.columns(prompted)
    assert bool((bp[:, step0:] == 0).all()) and bool((bp[:, :step0] == -1).all())
    from dimx.engine import op_seq_logprob
    sc = op_seq_logprob(lg, tok, first.tolist(), last.tolist())
    assert _close(score.cpu().numpy(), sc.score.cpu().numpy())


# ---- 4
def _replay(c, W, prompted, lg, prompt):
    """the definition fed with the dumped logits column by column -> per clip (parents [n, W], tokens [n, W], cum [n, W])"""
    from dimx import beam
    first, last, step0 = c.columns(prompted)
    n = lg.shape[1]
    out = []
    for b in range(c.B):
        cum = beam.start_scores(W)
        par, tok, cums = np.zeros((n, W), np.int32), np.zeros((n, W), np.int32), np.zeros((n, W))
        for col in range(step0, n):
            mode = beam.column_mode(col, first[b], last[b])
            new = beam.beam_step(lg[b * W:(b + 1) * W, col], cum, mode, max(int(prompt[b, col + 1]), 0) if mode == beam.FORCED else 0)
            if mode != beam.LIVE:
                assert np.array_equal(new[2], cum)
            par[col], tok[col], cum = new
            cums[col] = cum
        out.append((par, tok, cums))
    return out


def _check_replay(c, W, prompted, tok, score, lg, bp, prompt):
    first, last, step0 = c.columns(prompted)
    steps = _replay(c, W, prompted, lg, prompt)
    n = tok.shape[1]
    for b in range(c.B):
        par, stok, cums = steps[b]
        for w in range(W):
            r, slot = b * W + w, w
            for col in range(n - 1, step0 - 1, -1):     # backtracking: slot is the hypothesis's row after step col
                assert tok[r, col] == stok[col, slot] and bp[r, col] == par[col, slot], (b, w, col)
                slot = par[col, slot]
            assert (tok[r, :step0] == np.maximum(prompt[b, 1:step0 + 1], 0)).all() and (bp[r, :step0] == -1).all()
        assert _close(score[b * W:(b + 1) * W], cums[n - 1])
        assert (np.diff(score[b * W:(b + 1) * W]) <= 0).all()
        if last[b] < n:      # the frozen columns changed nothing: the score is the one after the last live column
            assert _close(score[b * W:(b + 1) * W], cums[max(last[b] - 1, step0)])
    return steps


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("prompted", [False, True], ids=["free", "prompted"])
@pytest.mark.parametrize("W", [2, 4, 10])
def test_replay_of_the_dumped_logits(engines, clips, W, prompted, mode):
    e, c = engines[mode], clips
    tok, score, lg, bp = (t.cpu().numpy() for t in c.beam(e, W, prompted, return_logits=True, return_backptr=True))
    _check_replay(c, W, prompted, tok, score, lg, bp, c.prompt.cpu().numpy())
    if prompted:
        assert (lg[:, :PROMPT["prefill"] - 1] == 0).all()


# ---- 5
@pytest.mark.parametrize("W", [4, 10])
def test_the_cache_was_reordered(engines, clips, W):
    """Every returned hypothesis teacher-forced (no key mask): the logits the search saw along the hypothesis's own ancestry are those
    of the hypothesis as a whole -- a wrong cache row moves them by order 1.  Measured on MI355X: worst |logit difference| 3.3e-6
    (W = 4) / 4.3e-6 (W = 10) against STEP_TOL = 2e-3; worst |score difference| 1.1e-5 / 9.2e-6 on 39 counted tokens."""
    from dimx import scoring
    from dimx.engine import op_seq_logprob
    e, c = engines["f32"], clips
    tok, score, lg, bp = c.beam(e, W, return_logits=True, return_backptr=True)
    R, n = tok.shape
    z = torch.cat([c.z[:, :1].repeat_interleave(W, 0).to(_dev()), tok.long()], 1)
    c.context(e, for_generate=False, repeat=W)
    tf, _, _ = e.decode_tf(z, c.m8.repeat_interleave(W, 0).contiguous(), None)
    rows = (torch.arange(R, device=_dev()) // W * W)[:, None] + bp.long()
    seen = lg[rows, torch.arange(n, device=_dev())[None, :]]
    d = (seen - tf).abs().amax(-1)
    print("W=%d: worst |dump along the ancestry - teacher forced| %.3e" % (W, float(d.max())))
    assert float(d.max()) <= STEP_TOL
    first, last = scoring.scored_columns(c.T, n, list(c.lens))
    sc = op_seq_logprob(tf, tok, first, last, rows_per_clip=W)
    ds = (sc.score - score).abs().cpu().numpy()
    count = sc.count.cpu().numpy()
    print("W=%d: worst |score - teacher-forced score| %.3e (counts up to %d)" % (W, ds.max(), count.max()))
    assert (ds <= 2 * (STEP_TOL + LOGIT_TOL) * count).all()


# ---- 6
@pytest.fixture(scope="module")
def oracle_ctx(full_sd, clips):
    import prompt_ref
    return prompt_ref.case_context(full_sd, clips.v_s, clips.v_a, clips.mask)


@pytest.mark.parametrize("W", [2, 4])
def test_against_the_cpu_oracle(engines, clips, full_sd, oracle_ctx, W):
    """Parents and tokens equal the oracle loop's at every live decision whose oracle margin exceeds TAU; after a decision below TAU
    the rest of the clip is not compared -- on this case no clip is cut short.  Measured on MI355X: largest |running score (HIP) -
    running score (oracle)| over the agreed steps 3.4e-6 (W = 2), 5.5e-6 (W = 4); worst |logits - oracle| 1.9e-6 / 1.6e-6; smallest
    oracle margins (keep / order) 1.7e-3 / 3.2e-3 (W = 2), 1.8e-3 / 7.2e-4 (W = 4)."""
    import beam_ref
    e, c = engines["f32"], clips
    n = c.T - 1
    ref = beam_ref.beam_generate(full_sd, c.z[:, :1], None, list(c.lens), n, c.T, W, oracle_ctx, c.mask)
    tok, score, lg, bp = (t.cpu().numpy() for t in c.beam(e, W, return_logits=True, return_backptr=True))
    steps = _check_replay(c, W, False, tok, score, lg, bp, c.prompt.cpu().numpy())
    worst, smallest = 0.0, np.inf
    for b in range(c.B):
        par, stok, cums = steps[b]
        for col in range(n):
            margin = ref["margins"][col, b].min()
            smallest = min(smallest, margin)
            assert margin > TAU, "clip %d is cut short at column %d: oracle margin %.3e" % (b, col, margin)
            assert np.array_equal(par[col], ref["parent"][col, b]) and np.array_equal(stok[col], ref["token"][col, b]), (b, col)
            fin = np.isfinite(ref["cum"][col, b])
            worst = max(worst, float(np.abs(cums[col][fin] - ref["cum"][col, b][fin]).max()))
    print("W=%d: largest |running score - oracle| %.3e, smallest oracle margin %.3e, TAU %.1e" % (W, worst, smallest, TAU))
    assert TAU <= 7e-4 and TAU >= 10 * worst
    assert np.array_equal(tok, ref["tokens"]) and np.array_equal(bp, ref["backptr"])
    d = np.abs(lg - ref["logits"].numpy()).max()
    print("W=%d: worst |logits - oracle| %.3e" % (W, d))
    assert d <= STEP_TOL


# ---- 7
def test_two_runs_are_bit_identical(engines, clips):
    for mode in ("f32", "bf16"):
        a = clips.beam(engines[mode], 5, True, return_logits=True, return_backptr=True)
        b = clips.beam(engines[mode], 5, True, return_logits=True, return_backptr=True)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int64), b[1].view(torch.int64))
        assert torch.equal(a[2].view(torch.int32), b[2].view(torch.int32)) and torch.equal(a[3], b[3])


def test_bad_arguments_and_unchanged_workspace_sizes(engines, clips):
    from dimx import engine, lib as L
    e, c = engines["f32"], clips
    B, T, W = c.B, c.T, 4
    sizes = lambda: ([e.lib.dimx_workspace_bytes(e.h, b, t) for b, t in ((B, T), (8, 64))] +
                     [e.lib.dimx_workspace_bytes_samples(e.h, B, T, s) for s in (1, 4, 10)] +
                     [e.lib.dimx_workspace_bytes_prompt(e.h, B, T, s, p) for s, p in ((1, 1), (4, 4), (10, 17))])
    before = sizes()
    c.context(e, W)
    start = c.z[:, :1].to(torch.int32).to(_dev()).contiguous()
    tokens = torch.full((B * W, T - 1), -7, dtype=torch.int32, device=_dev())
    scores = torch.zeros(B * W, dtype=torch.float64, device=_dev())
    state = torch.zeros(2 * B * W, dtype=torch.float64, device=_dev())
    ws, wsb = e.workspace(B, T, W)

    def call(eng, width, state_bytes):
        return eng.lib.dimx_generate_beam(eng.h, L.ptr(start), 1, None, 1, 1, L.ptr(c.m8), None, B, T, width, L.ptr(tokens), L.ptr(scores),
                                          None, None, L.ptr(state), state_bytes, 0, ws, wsb, e._s())

    for width in (0, 3, 6, 16):
        assert call(e, width, state.numel() * 8) == ERR_ARG and b"beam_width" in e.lib.dimx_last_error()
    assert call(e, W, 16 * B * W - 8) == ERR_ARG and b"beam state" in e.lib.dimx_last_error()
    slm = engine.Engine("cuda:0", L.MODE_PARITY_F32, variant="slm")
    assert call(slm, W, state.numel() * 8) == ERR_ARG and b"variant" in slm.lib.dimx_last_error()
    slm.close()
    torch.cuda.synchronize()
    assert bool((tokens == -7).all()), "a refused call launched something"
    assert call(e, W, state.numel() * 8) == 0
    torch.cuda.synchronize()
    assert bool((tokens >= 0).all())
    assert sizes() == before


# ---- 8
@pytest.fixture(scope="module")
def model():
    from dimx.seq2seq_pretrain import SLMFT
    return SLMFT().eval()


def _model_inputs(c):
    from dimx import prng
    v_l = torch.from_numpy(prng.normal(9, "s2s.vl", (c.B, c.T, 56)))
    return c.v_s.to(_dev()), v_l.to(_dev()), c.v_a.to(_dev()), c.mask.to(_dev())


def test_beam_through_the_model(model, clips):
    c, W = clips, 4
    args = _model_inputs(c)
    out = model(*args, mode="val", beam_width=W, num_return=W, return_tokens=True, return_scores=True)
    assert len(out) == 5 and out[2].shape == (c.B, W, c.T - 1, 56) and out[3].shape == (c.B, W, c.T - 1)
    assert out[4].score.shape == (c.B, W) and out[4].count.cpu().tolist() == [[n - 1] * W for n in c.lens]
    assert bool((out[4].score[:, :-1] >= out[4].score[:, 1:]).all())
    one = model(*args, mode="val", beam_width=W, return_tokens=True, return_scores=True)
    assert one[2].shape == (c.B, c.T - 1, 56) and torch.equal(one[3], out[3][:, 0]) and torch.equal(one[4].score, out[4].score[:, 0])
    assert torch.equal(one[2], model.forward_vq_decoder(out[3][:, 0].contiguous(), "val"))
    assert torch.equal(model(*args, mode="val", beam_width=W)[2], one[2])
    greedy = model(*args, mode="val", greedy=True, return_tokens=True)
    assert torch.equal(model(*args, mode="val", beam_width=1, return_tokens=True)[3], greedy[3])
    with pytest.raises(ValueError):
        model(*args, mode="val", beam_width=W, num_return=2)
    with pytest.raises(ValueError):
        model(*args, mode="train", beam_width=W)


def _loader():
    from dimx import prng
    T = SHORT[1]
    out = []
    for i, lens in enumerate((SHORT[2], (40, 21, 12))):
        Bn = len(lens)
        v_s = torch.from_numpy(prng.normal(40 + i, "m.vs", (Bn, T, 56)))
        v_l = torch.from_numpy(prng.normal(40 + i, "m.vl", (Bn, T, 56)))
        v_a = torch.from_numpy(prng.normal(40 + i, "m.va", (Bn, T, 768)))
        mask = torch.zeros(Bn, T, dtype=torch.bool)
        for j, n in enumerate(lens):
            mask[j, :n] = True
        src = torch.cat([v_s, v_a], -1) * mask[..., None]
        out.append((src, v_l * mask[..., None], list(lens), None, ["clip%d_%d" % (i, j) for j in range(Bn)]))
    return out


@pytest.mark.parametrize("select", ["likelihood", "fd"])
def test_protocol_with_beam_decoding(model, select):
    from dimx import x_engine_pt
    loader = _loader()
    kw = dict(select=select) if select == "likelihood" else dict(select=select, fd_backend="hip")
    y_true, y_pred, x, ids = x_engine_pt.evaluate_test_epoch(model, loader, _dev(), decode="beam", beam_width=4, **kw)
    again = x_engine_pt.evaluate_test_epoch(model, loader, _dev(), decode="beam", beam_width=4, **kw)[1]
    assert len(y_true) == len(y_pred) == len(x) == len(ids) == 6
    k = 0
    for batch in loader:
        src_s_v, src_s_a, tgt, mask, src_len, _ = x_engine_pt._prepare(batch, _dev())
        pred = model(src_s_v, tgt, src_s_a, mask, mode="val", beam_width=4, num_return=4)[2].cpu().numpy()
        for j in range(len(src_len)):
            n = src_len[j] - 1
            assert y_pred[k].shape == (n, 56) and np.array_equal(y_pred[k], again[k])      # no seed: the protocol is deterministic
            if select == "likelihood":
                assert np.array_equal(y_pred[k], pred[j, 0, :n])      # the search's best hypothesis is the likelihood winner
            else:
                assert any(np.array_equal(y_pred[k], pred[j, s, :n]) for s in range(4))
            k += 1
    with pytest.raises(ValueError):
        x_engine_pt.evaluate_test_epoch(model, loader, _dev(), decode="beam", beam_width=3)
    with pytest.raises(ValueError):
        x_engine_pt.evaluate_test_epoch(model, loader, _dev(), decode="greedy")
