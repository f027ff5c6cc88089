"""GPU: sequence log-likelihoods (dimx_op_seq_logprob) and the best-of-S pick by them (dimx_op_score_select), csrc/seq_score.hip,
against their float64 definition dimx.scoring, and the layers above them: Engine.generate(return_scores=True), SLMFT.score and
evaluate_test_epoch(select="likelihood").

BOUND is the project's bound for its float64 operators: 1e-11 per token and 1e-11 x max(1, count) per row sum; the magnitudes here
are at most 25.  Worst differences observed on MI355X are recorded in the docstrings of the tests that measure them."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
BOUND = 1e-11
B, S, N = 5, 10, 39
R = B * S
LAST = [39, 33, 7, 1, 0]
FIRST = [0, 5, 6, 0, 0]
SHORT = (3, 40, (40, 33, 7))     # tests/test_gpu_prompt.py
LOGIT_TOL, STEP_TOL = 1e-4, 2e-3    # tests/test_gpu_s2s.py, tests/test_gpu_prompt.py
ERR_ARG = -1


def _dev():
    return torch.device("cuda:0")


class _Seeded:
    """the seeded case of one scale: host arrays, device tensors and the definition's values, computed once"""

    def __init__(self, scale):
        from dimx import prng, scoring
        self.logits = (prng.normal(21, "score.logits", (R, N, 512)) * scale).astype(np.float32)
        self.tokens = prng.integers(21, "score.tok", (R, N), 0, 512).astype(np.int32)
        self.lg = torch.from_numpy(self.logits).to(_dev())
        self.tok = torch.from_numpy(self.tokens).to(_dev())
        self.ref = scoring.sequence_scores(self.logits, self.tokens, FIRST, LAST, rows_per_clip=S)


@pytest.fixture(scope="module", params=[1, 3], ids=["scale1", "scale3"])
def case(request):
    return _Seeded(request.param)


def _check(sc, tok_lp, logits, tokens, first, last, rpc, what):
    """operator outputs against dimx.scoring on the same host values: counts equal, per-token and per-row differences within BOUND"""
    from dimx import scoring
    ref = scoring.sequence_scores(logits, tokens, first, last, rows_per_clip=rpc)
    n = tokens.shape[1]
    clips = tokens.shape[0] // rpc
    c0 = np.repeat(np.clip(np.zeros(clips, int) if first is None else np.asarray(first), 0, n), rpc)[:, None]
    c1 = np.repeat(np.clip(np.full(clips, n) if last is None else np.asarray(last), 0, n), rpc)[:, None]
    cols = np.arange(n)[None, :]
    ref_tok = np.where((cols >= c0) & (cols < c1), scoring.token_logprob(logits, tokens), 0.0)
    count = sc.count.cpu().numpy()
    assert sc.score.dtype == torch.float64 and sc.count.dtype == torch.int32
    assert np.array_equal(count, ref.count)
    d_row = np.abs(sc.score.cpu().numpy() - ref.score)
    d_tok = np.abs(tok_lp.cpu().numpy() - ref_tok).max() if tok_lp is not None else 0.0
    worst_row = (d_row / np.maximum(1, count)).max()
    print("%s: worst |per-token - definition| %.3e, worst |row sum - definition| %.3e (%.3e per max(1, count))"
          % (what, d_tok, d_row.max(), worst_row))
    assert d_tok <= BOUND
    assert (d_row <= BOUND * np.maximum(1, count)).all()


# ---- 1
def test_operator_matches_the_definition(case):
    """Measured on MI355X (scale 1 / scale 3): worst per-token difference 1.8e-15 / 3.6e-15, worst row-sum difference 1.1e-13 /
    1.7e-13 (2.9e-15 / 4.4e-15 per counted token), against BOUND = 1e-11; n = 1: 8.9e-16 / 1.8e-15."""
    from dimx.engine import op_seq_logprob
    sc, tl = op_seq_logprob(case.lg, case.tok, FIRST, LAST, rows_per_clip=S, want_tokens=True)
    _check(sc, tl, case.logits, case.tokens, FIRST, LAST, S, "clips of %d rows" % S)
    assert float(sc.score[4 * S:].abs().max()) == 0.0 and int(sc.count[4 * S:].max()) == 0      # the empty range
    # rows_per_clip = 1 with per-row ranges, as tensors on the device
    first = [r % 7 for r in range(R)]
    last = [N - 8 * (r % 5) for r in range(R)]
    sc, tl = op_seq_logprob(case.lg, case.tok, torch.tensor(first).to(_dev()), torch.tensor(last).to(_dev()), want_tokens=True)
    _check(sc, tl, case.logits, case.tokens, first, last, 1, "per-row ranges")
    # no ranges at all
    sc, tl = op_seq_logprob(case.lg, case.tok, want_tokens=True)
    _check(sc, tl, case.logits, case.tokens, None, None, 1, "whole rows")
    # n = 1
    sc, tl = op_seq_logprob(case.lg[:, :1], case.tok[:, :1], want_tokens=True)
    _check(sc, tl, case.logits[:, :1], case.tokens[:, :1], None, None, 1, "n = 1")
    # a few tokens outside the vocabulary: skipped, not counted
    tokens = case.tokens.copy()
    tokens[0, 3], tokens[0, 4], tokens[7, 0], tokens[7, 38] = -100, 512, -1, 1 << 20
    sc, tl = op_seq_logprob(case.lg, torch.from_numpy(tokens).to(_dev()), FIRST, LAST, rows_per_clip=S, want_tokens=True)
    _check(sc, tl, case.logits, tokens, FIRST, LAST, S, "with skipped tokens")
    assert int(sc.count[0]) == N - 2 and int(sc.count[7]) == N - 2
    assert float(tl[0, 3]) == 0.0 and float(tl[0, 4]) == 0.0


def test_count_of_a_skipped_token_at_the_range_start(case):
    from dimx.engine import op_seq_logprob
    tokens = case.tok.clone()
    tokens[12, 5] = -100      # row 12 is clip 1: columns [5, 33)
    sc = op_seq_logprob(case.lg, tokens, FIRST, LAST, rows_per_clip=S)
    assert int(sc.count[12]) == LAST[1] - FIRST[1] - 1 and int(sc.count[13]) == LAST[1] - FIRST[1]


# ---- 2
def test_determinism_and_strided_views(case):
    from dimx.engine import op_seq_logprob
    a, ta = op_seq_logprob(case.lg, case.tok, FIRST, LAST, rows_per_clip=S, want_tokens=True)
    b, tb = op_seq_logprob(case.lg, case.tok, FIRST, LAST, rows_per_clip=S, want_tokens=True)
    assert torch.equal(a.score, b.score) and torch.equal(a.count, b.count) and torch.equal(ta, tb)
    # slices of longer buffers: row strides (n + 3) * 512 and n + 3; the padding columns hold NaN (token 0: a column that were read
    # would be scored), and so does every column of the view outside its clip's range
    lbuf = torch.full((R, N + 3, 512), float("nan"), dtype=torch.float32, device=_dev())
    tbuf = torch.zeros(R, N + 3, dtype=torch.int32, device=_dev())
    lbuf[:, :N] = case.lg
    tbuf[:, :N] = case.tok
    for r in range(R):
        lbuf[r, :FIRST[r // S]] = float("nan")
        lbuf[r, LAST[r // S]:] = float("nan")
    lv, tv = lbuf[:, :N], tbuf[:, :N]
    assert lv.stride() == ((N + 3) * 512, 512, 1) and tv.stride() == (N + 3, 1)
    c, tc = op_seq_logprob(lv, tv, FIRST, LAST, rows_per_clip=S, want_tokens=True)
    assert torch.equal(a.score, c.score) and torch.equal(a.count, c.count) and torch.equal(ta, tc)
    assert bool(torch.isfinite(c.score).all())


# ---- 3
def _select_inputs():
    from dimx import prng
    return torch.from_numpy(prng.normal(21, "score.pred", (B, S, N, 56))).to(_dev())


def test_selection(case):
    from dimx import scoring
    from dimx.engine import op_score_select, op_seq_logprob
    sc = op_seq_logprob(case.lg, case.tok, FIRST, LAST, rows_per_clip=S)
    y_pred = _select_inputs()
    win, ok, best, btok = op_score_select(sc.score, y_pred, LAST, tokens=case.tok)
    ref_win, ref_ok = scoring.pick(case.ref.score.reshape(B, S))
    assert win.dtype == torch.int32 and ok.dtype == torch.uint8
    assert win.cpu().tolist() == ref_win.tolist()        # all five clips: the top two scores are >= 0.45 apart (test_seq_score_host)
    assert ok.cpu().tolist() == [1] * B and ref_ok.all()
    for j in range(B):
        w = int(ref_win[j])
        assert torch.equal(best[j, :LAST[j]], y_pred[j, w, :LAST[j]])
        assert float(best[j, LAST[j]:].abs().max() if LAST[j] < N else 0.0) == 0.0
        assert torch.equal(btok[j], case.tok[j * S + w])
    # a strided y_pred view gives identical results
    buf = torch.full((B, S, N + 1, 56), float("nan"), dtype=torch.float32, device=_dev())
    buf[:, :, 1:] = y_pred
    win2, ok2, best2 = op_score_select(sc.score, buf[:, :, 1:], torch.tensor(LAST, dtype=torch.int32).to(_dev()))
    assert torch.equal(win, win2) and torch.equal(ok, ok2) and torch.equal(best, best2)
    # a clip without a finite score: ok = 0, zero rows; ten copies of one row: the first wins
    score = sc.score.reshape(B, S).clone()
    score[2] = float("nan")
    score[1] = score[1, 3].item()
    score[0, 0] = float("nan")
    win3, ok3, best3, btok3 = op_score_select(score, y_pred, LAST, tokens=case.tok)
    ref_win3, ref_ok3 = scoring.pick(score.cpu().numpy())
    assert win3.cpu().tolist() == ref_win3.tolist() and ok3.cpu().bool().tolist() == ref_ok3.tolist()
    assert int(win3[1]) == 0 and int(ok3[2]) == 0 and int(ok3[0]) == 1
    assert float(best3[2].abs().max()) == 0.0 and bool((btok3[2] == -100).all())
    assert torch.equal(best3[1, :LAST[1]], y_pred[1, 0, :LAST[1]])


def test_bad_arguments_enqueue_nothing(case):
    from dimx import lib as L
    lib = L.load()
    score = torch.full((R,), -7.0, dtype=torch.float64, device=_dev())
    count = torch.full((R,), -7, dtype=torch.int32, device=_dev())
    tl = torch.full((R, N), -7.0, dtype=torch.float64, device=_dev())

    def call(rpc=S, rows=R, n=N, step=512, logits=case.lg):
        return lib.dimx_op_seq_logprob(L.ptr(logits), N * 512, step, L.ptr(case.tok), N, None, None, rpc, rows, n, L.ptr(tl), L.ptr(score),
                                       L.ptr(count), L.stream_ptr(_dev()))

    assert call(rpc=7) == ERR_ARG          # R = 50 is not a multiple of 7
    assert b"multiple" in lib.dimx_last_error()
    assert call(rpc=0) == ERR_ARG and call(n=0) == ERR_ARG and call(rows=-1) == ERR_ARG and call(step=511) == ERR_ARG
    assert call(logits=None) == ERR_ARG
    assert call(rows=0) == 0               # a no-op
    win = torch.full((B,), -7, dtype=torch.int32, device=_dev())
    ok = torch.full((B,), 9, dtype=torch.uint8, device=_dev())
    sel = lambda b, s: lib.dimx_op_score_select(L.ptr(score), None, 0, 0, 0, None, None, 0, b, s, 0, 0, 0, L.ptr(win), L.ptr(ok), None, None,
                                                L.stream_ptr(_dev()))
    assert sel(0, S) == ERR_ARG and sel(B, 0) == ERR_ARG
    torch.cuda.synchronize()
    assert bool((score == -7).all()) and bool((count == -7).all()) and bool((tl == -7).all()), "a refused call launched something"
    assert bool((win == -7).all()) and bool((ok == 9).all()), "a refused call launched something"


# ---- 4
class _Clips:
    """the SHORT inputs of tests/test_gpu_prompt.py (its prng streams)"""

    def __init__(self):
        from dimx import prng
        self.B, self.T, self.lens = SHORT[0], SHORT[1], list(SHORT[2])
        B_, T = self.B, self.T
        self.v_s = torch.from_numpy(prng.normal(9, "s2s.vs", (B_, T, 56))).to(_dev())
        self.v_a = torch.from_numpy(prng.normal(9, "s2s.va", (B_, T, 768))).to(_dev())
        self.v_l = torch.from_numpy(prng.normal(9, "score.vl", (B_, T, 56))).to(_dev())
        z = torch.from_numpy(prng.integers(9, "s2s.z", (B_, T), 0, 512))
        self.mask = torch.zeros(B_, T, dtype=torch.bool)
        for j, n in enumerate(self.lens):
            self.mask[j, :n] = True
        self.z = torch.where(self.mask, z, torch.full_like(z, -100)).to(_dev())
        self.mask = self.mask.to(_dev())
        self.m8 = self.mask.to(torch.uint8).contiguous()

    def context(self, eng, for_generate=True, **kw):
        eng.encode_ctx(self.v_s, self.v_a, self.m8, for_generate, **kw)


@pytest.fixture(scope="module")
def clips():
    return _Clips()


@pytest.fixture(scope="module")
def engines(full_sd):
    from dimx import engine, lib
    out = {}
    for name, mode in (("f32", lib.MODE_PARITY_F32), ("bf16", lib.MODE_PERF_BF16)):
        out[name] = engine.Engine("cuda:0", mode)
        out[name].load_state_dict(full_sd)
    return out


PROMPT = dict(Pmax=16, prompt_len=(16, 9, 7), prefill=7)


def _generate(e, c, n_samples, prompted, **kw):
    """one seeded generation of the SHORT clips -> what Engine.generate returns"""
    if prompted:
        c.context(e, n_samples=n_samples, prompt_frames=PROMPT["prefill"])
        return e.generate(None, c.m8, c.T, 1.0, seed=12345, n_samples=n_samples, prompt=c.z[:, :PROMPT["Pmax"]].to(torch.int32).contiguous(),
                          prompt_len=torch.tensor(PROMPT["prompt_len"], dtype=torch.int32).to(_dev()), prefill=PROMPT["prefill"], **kw)
    c.context(e, n_samples=n_samples)
    return e.generate(c.z[:, 0], c.m8, c.T, 1.0, seed=12345, n_samples=n_samples, **kw)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("n_samples,prompted", [(1, False), (5, False), (1, True), (5, True)])
def test_generation_scores(engines, clips, mode, n_samples, prompted):
    """Measured on MI355X: worst |score - definition| 5.7e-14 on a row (1.8e-15 per counted token) over the eight cases."""
    from dimx import scoring
    from dimx.engine import op_seq_logprob
    e, c = engines[mode], clips
    tok0, lg0 = _generate(e, c, n_samples, prompted, return_logits=True)
    tok, lg, sc = _generate(e, c, n_samples, prompted, return_logits=True, return_scores=True)
    assert torch.equal(tok, tok0) and torch.equal(lg, lg0)
    tok2, sc2 = _generate(e, c, n_samples, prompted, return_scores=True)      # the dump is requested internally
    assert torch.equal(tok2, tok) and torch.equal(sc2.score, sc.score) and torch.equal(sc2.count, sc.count)
    assert sc.score.shape == (c.B * n_samples,) and sc.count.shape == (c.B * n_samples,)
    plen = [min(max(p, PROMPT["prefill"]), PROMPT["Pmax"]) for p in PROMPT["prompt_len"]] if prompted else None
    first, last = scoring.scored_columns(c.T, c.T - 1, c.lens, plen)
    mine = op_seq_logprob(lg, tok, first, last, rows_per_clip=n_samples)
    assert torch.equal(mine.score, sc.score) and torch.equal(mine.count, sc.count)
    want = [max(n - p, 0) for n, p in zip(c.lens, plen)] if prompted else [n - 1 for n in c.lens]
    assert sc.count.cpu().tolist() == [k for k in want for _ in range(n_samples)]
    _check(sc, None, lg.cpu().numpy(), tok.cpu().numpy(), first, last, n_samples, "generate %s S=%d prompted=%d" % (mode, n_samples, prompted))


# ---- 5
@pytest.fixture(scope="module")
def model():
    from dimx.seq2seq_pretrain import SLMFT
    return SLMFT().eval()


def test_teacher_forced_score(model, clips):
    """Measured on MI355X: worst |score - definition| 2.8e-14 (8.9e-16 per counted token); worst |per-token + row_loss| 8.7e-07
    against 1e-4 (row_loss is formed in f32)."""
    from dimx import scoring
    from dimx.engine import op_seq_logprob
    c = clips
    sc = model.score(c.v_s, c.v_l, c.v_a, c.mask)
    assert sc.score.shape == (c.B,) and sc.count.cpu().tolist() == [n - 1 for n in c.lens]
    _, z_l = model.forward_vq(c.v_s, c.v_l, c.mask, with_speaker=False)
    eng = model.engine(_dev())
    c.context(eng, for_generate=False)
    logits, row_loss, _ = eng.decode_tf(z_l, c.m8, None)
    first, last = scoring.scored_columns(c.T, c.T - 1, c.lens)
    _check(sc, None, logits.cpu().numpy(), z_l[:, 1:].cpu().numpy(), first, last, 1, "SLMFT.score")
    _, tl = op_seq_logprob(logits, z_l[:, 1:], first, last, want_tokens=True)
    d = (tl + row_loss.double()).abs().max().item()
    print("SLMFT.score: worst |per-token log-likelihood + row_loss| %.3e" % d)
    assert d <= 1e-4
    assert abs(scoring.perplexity(sc) - float(torch.exp(-sc.score.sum() / sc.count.sum()))) < 1e-9


def test_generation_score_agrees_with_teacher_forcing(model, engines, clips):
    """The f32 generation's own score against the teacher-forced score of the tokens it sampled (start token prepended, no key
    mask): within count x 4.2e-3 = 2 (STEP_TOL + LOGIT_TOL) per token, log-softmax being 2-Lipschitz in the sup norm of the logits.
    Measured on MI355X: |score difference| 9.1e-06, 4.9e-06, 2.7e-06 for counts 39, 32, 6 (4.4e-07 per token at worst)."""
    e, c = engines["f32"], clips
    tok, sc = _generate(e, c, 1, False, return_scores=True)
    z = torch.cat([c.z[:, :1], tok.long()], 1)
    tf = model.score(c.v_s, c.v_l, c.v_a, c.mask, z_l=z)
    assert torch.equal(tf.count, sc.count)
    d = (tf.score - sc.score).abs().cpu().numpy()
    count = sc.count.cpu().numpy()
    print("generation vs teacher forcing: |score difference| %s for counts %s (%.3e per token at worst)"
          % (d.tolist(), count.tolist(), (d / np.maximum(1, count)).max()))
    assert (d <= count * 2 * (STEP_TOL + LOGIT_TOL)).all()


def test_return_scores_through_the_model(model, clips):
    c = clips
    out = model(c.v_s, c.v_l, c.v_a, c.mask, mode="val", seed=77, n_samples=5, return_tokens=True, return_scores=True)
    assert len(out) == 5 and out[2].shape == (c.B, 5, c.T - 1, 56) and out[3].shape == (c.B, 5, c.T - 1)
    assert out[4].score.shape == (c.B, 5) and out[4].count.shape == (c.B, 5)
    one = model(c.v_s, c.v_l, c.v_a, c.mask, mode="val", seed=77, return_scores=True)
    assert len(one) == 4 and one[3].score.shape == (c.B,)
    with pytest.raises(ValueError):
        model(c.v_s, c.v_l, c.v_a, c.mask, mode="train", return_scores=True)


# ---- 6
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


def test_protocol_selects_by_likelihood(model):
    from dimx import x_engine_pt
    loader = _loader()
    y_true, y_pred, x, ids = x_engine_pt.evaluate_test_epoch(model, loader, _dev(), beam_size=5, select="likelihood", seed=4321)
    assert len(y_true) == len(y_pred) == len(x) == len(ids) == 6
    k = 0
    for batch in loader:
        src_s_v, src_s_a, tgt, mask, src_len, _ = x_engine_pt._prepare(batch, _dev())
        _, _, pred, sc = model(src_s_v, tgt, src_s_a, mask, mode="val", n_samples=5, seed=4321, return_scores=True)
        win = np.argmax(sc.score.cpu().numpy(), axis=1)
        for j, n in enumerate(src_len):
            want = pred[j, int(win[j]), :n - 1].cpu().numpy()
            assert y_pred[k].shape == (n - 1, 56) and np.array_equal(y_pred[k], want), "clip %d" % k
            assert np.array_equal(y_true[k], tgt[j, 1:n].cpu().numpy())
            k += 1
    assert x_engine_pt.last_eval_report["fd_backend"] is None


def test_protocol_default_selection_is_unchanged(model):
    from dimx import x_engine_pt
    loader = _loader()
    a = x_engine_pt.evaluate_test_epoch(model, loader, _dev(), beam_size=5, fd_backend="hip", seed=4321)
    b = x_engine_pt.evaluate_test_epoch(model, loader, _dev(), beam_size=5, fd_backend="hip", select="fd", seed=4321)
    assert x_engine_pt.last_eval_report["fd_backend"] == "hip"
    for la, lb in zip(a[:3], b[:3]):
        assert len(la) == len(lb) == 6
        for p, q in zip(la, lb):
            assert (p is None and q is None) or np.array_equal(p, q)
    assert list(a[3]) == list(b[3])
    with pytest.raises(ValueError):
        x_engine_pt.evaluate_test_epoch(model, loader, _dev(), beam_size=3, select="likelihood")
