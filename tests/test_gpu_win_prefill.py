"""GPU: the windowed prefill -- the many-query windowed cross attention (dimx_op_cross_attn_win, csrc/win_attn.hip)
against float64, against itself under other launch shapes and against poisoned memory; the teacher-forced pass under the window
(dimx_decode_tf_win) against the online CPU checker, the forced-step generation and the offline pass; the windowed prompt
prefill of dimx_generate_prompted; sessions begun from a prompt (dimx_stream_begin_prompted); and the host layers."""
import ctypes

import numpy as np
import pytest
import torch

from test_gpu_decode_step import tolerance
from test_gpu_online import MAX_LEFT_OUT, MIN_MARGIN, _against_checker
from test_gpu_prompt import LOGIT_TOL, LONG, SHORT, STEP_TOL, _case, _clips, _noise
from test_win_prefill_host import PROMPT_CFG, PROMPT_LOOKAHEADS, SESSION_LOOKAHEADS, WIN_SEED, session_cases

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
ERR_ARG, ERR_STATE = -1, -4
SCALE = 0.125
SENTINEL = 777.0


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


# ---------------------------------------------------------------- 1 - 3: the kernel
AB, AH, ATP, AQ = 3, 2, 48, 40


class _Attn:
    """q rows for 40 positions and 48 K / V rows per (clip, head), computed once and left unchanged"""

    def __init__(self):
        from dimx import prng
        self.q = torch.from_numpy(prng.normal(5, "win.q", (AB, AQ, AH * 64))).float().cuda()
        self.k32 = torch.from_numpy(prng.normal(5, "win.k", (AB, AH, ATP, 64))).float().cuda()
        self.v32 = torch.from_numpy(prng.normal(5, "win.v", (AB, AH, ATP, 64))).float().cuda()

    def kv(self, dtype):
        return self.k32.to(dtype).contiguous(), self.v32.to(dtype).contiguous()

    @staticmethod
    def keep(n_keys):
        """ragged keep-masks: the clips keep their first (n_keys, n_keys - 7 or 1, 1) keys"""
        lens = (n_keys, max(n_keys - 7, 1), 1)
        km = torch.zeros(AB, ATP, dtype=torch.uint8)
        for b, n in enumerate(lens):
            km[b, :n] = 1
        return km.cuda()

    def ref(self, dtype, t0, Lq, L, n_keys, km):
        """float64 softmax over the cache-rounded K / V under dimx.online's bound and the keep-mask -> [B, Lq, H*64]"""
        from dimx.online import visible
        k, v = self.kv(dtype)
        q = self.q[:, t0:t0 + Lq].view(AB, Lq, AH, 64)
        s = torch.einsum("bihd,bhjd->bhij", q.double(), k[:, :, :n_keys].double()) * SCALE
        vis = torch.from_numpy(np.asarray(visible(np.arange(t0, t0 + Lq), L, n_keys)).reshape(-1)).cuda()
        m = (torch.arange(n_keys, device="cuda")[None, :] < vis[:, None])[None] & km[:, None, :n_keys].bool()     # [B, Lq, n_keys]
        s = s.masked_fill(~m[:, None], float("-inf"))
        o = torch.einsum("bhij,bhjd->bihd", s.softmax(-1), v[:, :, :n_keys].double())
        return o.reshape(AB, Lq, AH * 64).cpu()


@pytest.fixture(scope="module")
def attn():
    return _Attn()


def _win(attn, dtype, t0, Lq, L, n_keys, km, k=None, v=None, q=None):
    from dimx import engine as E
    kk, vv = attn.kv(dtype)
    q = attn.q[:, t0:t0 + Lq].contiguous() if q is None else q
    return E.op_cross_attn_win(q, kk if k is None else k, vv if v is None else v, L, SCALE, t0=t0, n_keys=n_keys, kmask=km)


@pytest.mark.parametrize("n_keys", [2, 17, 40])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_operator_against_float64(attn, dtype, n_keys):
    from dimx import engine as E
    bf = dtype == torch.bfloat16
    k, v = attn.kv(dtype)
    km = attn.keep(n_keys)
    worst, G = 0.0, 4
    for Lq in (1, 15, 16, 17, 33):
        for t0 in (0, 5):
            for L in (0, -3, 2, 40, -100):
                ref = attn.ref(dtype, t0, Lq, L, n_keys, km)
                what = "n_keys=%d Lq=%d t0=%d L=%d %s" % (n_keys, Lq, t0, L, "bf16" if bf else "f32")
                big = torch.full((AB * Lq + 2 * G, AH * 64), SENTINEL, dtype=dtype, device="cuda")
                out = big[G:G + AB * Lq].view(AB, Lq, AH * 64)
                E.op_cross_attn_win(attn.q[:, t0:t0 + Lq].contiguous(), k, v, L, SCALE, t0=t0, n_keys=n_keys, kmask=km, out=out)
                assert bool((big[:G] == SENTINEL).all()) and bool((big[G + AB * Lq:] == SENTINEL).all()), what
                assert torch.isfinite(out).all(), what
                err = (out.double().cpu() - ref).abs()
                tol = tolerance(ref, bf)
                assert (err <= tol).all(), "%s: max err %.3g (tol %.3g there)" % (what, err.max().item(), tol.flatten()[err.argmax()].item())
                worst = max(worst, err.max().item())
    print("windowed cross attention %s n_keys=%d: largest |out - float64| %.3g" % ("bf16" if bf else "f32", n_keys, worst))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_a_row_with_no_kept_key_is_zero(attn, dtype):
    km = attn.keep(17)
    km[1] = 0
    out = _win(attn, dtype, 0, 17, 0, 17, km)
    assert bool((out[1] == 0).all()) and bool((out[0] != 0).any()) and torch.isfinite(out).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("L", [0, -3, 2])
def test_a_row_is_a_function_of_its_own_inputs(attn, dtype, L):
    n_keys, Lq = 40, 33
    km = attn.keep(n_keys)
    whole = _win(attn, dtype, 0, Lq, L, n_keys, km)
    alone = torch.cat([_win(attn, dtype, i, 1, L, n_keys, km) for i in range(Lq)], 1)
    assert torch.equal(whole, alone), "a row alone (Lq = 1, t0 = i) differs from the row inside the launch of 33"
    for c in (5, 16):
        parts = torch.cat([_win(attn, dtype, i, min(c, Lq - i), L, n_keys, km) for i in range(0, Lq, c)], 1)
        assert torch.equal(whole, parts), "launches of %d rows" % c


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_no_read_past_the_bound(attn, dtype):
    from dimx.online import visible
    k, v = attn.kv(dtype)
    for n_keys in (17, 40):
        km = attn.keep(n_keys)
        for Lq, t0, L in ((15, 0, 0), (17, 5, -3), (33, 0, 2), (16, 5, 2), (1, 0, -100)):
            bound = visible(t0 + Lq - 1, L, n_keys)        # of the launch's last query
            clean = _win(attn, dtype, t0, Lq, L, n_keys, km)
            kp, vp = k.clone(), v.clone()
            kp[:, :, bound:], vp[:, :, bound:] = float("nan"), float("nan")       # past the bound, the padding past n_keys included
            # q rows past Lq (and before the first row) poisoned: the launch reads its own B * Lq rows only
            G = 3
            qbig = torch.full((AB * Lq + 2 * G, AH * 64), float("nan"), device="cuda")
            qbig[G:G + AB * Lq] = attn.q[:, t0:t0 + Lq].reshape(AB * Lq, AH * 64)
            out = _win(attn, dtype, t0, Lq, L, n_keys, km, kp, vp, qbig[G:G + AB * Lq].view(AB, Lq, AH * 64))
            what = "n_keys=%d Lq=%d t0=%d L=%d bound=%d" % (n_keys, Lq, t0, L, bound)
            assert torch.isfinite(out).all(), what
            assert torch.equal(out, clean), what
            # the masked rows' values never reach the output either: NaN in every row a clip's mask drops
            km_rows = km[:, None, :, None].bool().expand(AB, AH, ATP, 64)
            kq = torch.where(km_rows, kp, torch.full_like(kp, float("nan")))
            vq = torch.where(km_rows, vp, torch.full_like(vp, float("nan")))
            assert torch.equal(_win(attn, dtype, t0, Lq, L, n_keys, km, kq, vq), clean), what + " (masked rows)"


def test_operator_refuses_bad_shapes_without_a_launch(attn):
    from dimx import engine as E, lib as L
    k, v = attn.kv(torch.float32)
    q = attn.q[:, :4].contiguous()
    out = torch.full((AB, 4, AH * 64), SENTINEL, device="cuda")
    lib = L.load()

    def call(qp=None, ld=AH * 64, Tp=ATP, o_ld=AH * 64, Lq=4, t0=0, n_keys=40, kmask=None, kmask_ld=0, kc=None):
        return lib.dimx_op_cross_attn_win(L.F32, L.ptr(q) if qp is None else qp, ld, L.ptr(k) if kc is None else kc, L.ptr(v), Tp, L.ptr(out),
                                          o_ld, AB, AH, Lq, t0, n_keys, 0, kmask, kmask_ld, SCALE, L.stream_ptr(q.device))

    assert call(n_keys=ATP + 1) == ERR_ARG and call(n_keys=0) == ERR_ARG and call(n_keys=2049, Tp=4096) == ERR_ARG      # > kMaxKeys
    assert call(Lq=0) == ERR_ARG and call(t0=-1) == ERR_ARG and call(ld=AH * 64 - 4) == ERR_ARG and call(o_ld=AH * 64 + 4) == ERR_ARG
    assert call(qp=ctypes.c_void_p(q.data_ptr() + 4)) == ERR_ARG and call(kc=ctypes.c_void_p(0)) == ERR_ARG
    assert call(kmask=L.ptr(attn.keep(40)), kmask_ld=39) == ERR_ARG
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()), "a refused call launched something"
    for la in (2 ** 31 - 1, -2 ** 31):     # any int is a look-ahead: the bound is formed in 64 bits
        o = E.op_cross_attn_win(q, k, v, la, SCALE, n_keys=40)
        want = E.op_cross_attn_win(q, k, v, 40 if la > 0 else -100, SCALE, n_keys=40)
        assert torch.equal(o, want)


# ---------------------------------------------------------------- 4, 5: decode_tf_win
class _Short:
    """the SHORT inputs, the oracle's context and the checker's runs, computed once and left unchanged"""

    def __init__(self, sd):
        import prompt_ref
        self.sd = sd
        self.B, self.T, self.lens = SHORT
        self.v_s, self.v_a, self.z, self.mask = _case(self.B, self.T, list(self.lens), seed=WIN_SEED)
        self.noise = _noise(self.B, self.T)
        self.ctx = prompt_ref.case_context(sd, self.v_s, self.v_a, self.mask)
        self.m8 = self.mask.to(torch.uint8).cuda()
        self.zd = self.z.to(torch.int32).cuda().contiguous()
        self.inside = torch.arange(self.T - 1)[None, :] < (torch.tensor(self.lens)[:, None] - 1)     # columns inside each clip's length
        self._ref = {}

    def checker(self, L, noisy=False, Pmax=1, plen=None):
        import online_ref
        key = (L, noisy, Pmax, None if plen is None else tuple(plen))
        if key not in self._ref:
            self._ref[key] = online_ref.online_generate(self.sd, self.z[:, :Pmax], plen, self.T - 1, self.ctx, self.mask, L,
                                                        self.noise if noisy else None)
        return self._ref[key]

    def forced(self, L):
        """every token forced: the teacher-forced logits under the window, step by step"""
        return self.checker(L, False, self.T - 1, None)[1]

    def context(self, eng, for_generate=True, v_s=None, v_a=None, **kw):
        eng.encode_ctx((self.v_s if v_s is None else v_s).cuda(), (self.v_a if v_a is None else v_a).cuda(), self.m8, for_generate, **kw)

    def tf_win(self, eng, L, **kw):
        self.context(eng, **kw)
        return eng.decode_tf(self.zd, self.m8, None, lookahead=L)

    def forced_steps(self, eng, L):
        self.context(eng)
        _, lg = eng.generate(None, self.m8, self.T, 0.0, return_logits=True, prompt=self.zd[:, :self.T - 1].contiguous(), prefill=1,
                             no_prefill=True, lookahead=L)
        return lg


@pytest.fixture(scope="module")
def short(full_sd):
    return _Short(full_sd)


@pytest.mark.parametrize("L", [0, -3, 2, 6, 40])
def test_decode_tf_win(eng, short, L):
    c = short
    logits, row_loss, amax = c.tf_win(eng, L)
    lg = logits.cpu()
    assert lg.shape == (c.B, c.T - 1, 512) and torch.isfinite(lg).all()
    e_ref = (lg - c.forced(L)).abs().amax(-1)
    e_steps = (lg - c.forced_steps(eng, L).cpu()).abs().max().item()
    print("decode_tf_win L=%d: max |logits - checker| %.2e inside the clips (%.2e over all columns); |logits - forced steps| %.2e"
          % (L, e_ref[c.inside].max().item(), e_ref.max().item(), e_steps))
    assert e_ref[c.inside].max().item() < LOGIT_TOL
    assert e_steps < STEP_TOL
    if L == 40:     # the window-off limit: the offline pass on the same clip (other kernels, no bit claim)
        c.context(eng, for_generate=False)
        off = eng.decode_tf(c.zd, c.m8, None)[0].cpu()
        e_off = (lg - off).abs().amax(-1)
        print("decode_tf_win L=40 against dimx_decode_tf: %.2e inside the clips (%.2e over all columns)" % (e_off[c.inside].max().item(), e_off.max().item()))
        assert e_off[c.inside].max().item() < LOGIT_TOL
    # row_loss and argmax_tok are those of the logits
    tgt = c.z[:, 1:]
    ce = torch.nn.functional.cross_entropy(lg.double().reshape(-1, 512), tgt.clamp(min=0).reshape(-1), reduction="none").view(c.B, c.T - 1)
    ce = torch.where(tgt >= 0, ce, torch.zeros_like(ce))
    assert (row_loss.cpu().double() - ce).abs().max().item() < 1e-4      # f32 log-sum-exp of 512 unit-scale logits against float64
    assert torch.equal(amax.cpu().long(), lg.argmax(-1))


def test_decode_tf_win_state_and_arguments(eng, short):
    from dimx import lib as L
    c = short
    logits = torch.full((c.B, c.T - 1, 512), SENTINEL, device="cuda")
    ws, wsb = eng.workspace(c.B, c.T)

    def call(z=c.zd, m=c.m8):
        return eng.lib.dimx_decode_tf_win(eng.h, L.ptr(z), L.ptr(m), c.B, c.T, 0, L.ptr(logits), None, None, ws, wsb, eng._s())

    c.context(eng, for_generate=False)
    assert call() == ERR_STATE and b"for_generate=1" in eng.lib.dimx_last_error()
    c.context(eng)
    assert call(z=None) == ERR_ARG
    torch.cuda.synchronize()
    assert bool((logits == SENTINEL).all()), "a refused call launched something"
    with pytest.raises(L.DimxError):
        eng.decode_tf(c.zd, c.m8, c.m8[:, :c.T - 1].contiguous(), lookahead=0)     # no random key mask under the window
    assert call() == 0
    # the look-ahead is the call's argument: the handle's setting is neither read nor changed
    a = eng.decode_tf(c.zd, c.m8, None, lookahead=0)[0]
    eng.set_cross_lookahead(5)
    try:
        b = eng.decode_tf(c.zd, c.m8, None, lookahead=0)[0]
        assert eng.cross_lookahead() == 5
    finally:
        eng.set_cross_lookahead(None)
    assert torch.equal(a, b)


def test_bf16_decode_tf_win_error_is_the_decode_steps_error(eng_bf16, short):
    """bf16: the one-pass logits and the forced-step logits round K / V alike and differ in the kernels that formed the rows; the
    bound is the one tests/test_gpu_prompt.py::test_bf16_prefill_error_is_the_decode_steps_error uses for the offline prefill --
    the error against the f32 checker at most twice the forced-step path's own error + 1e-3 (columns inside the clips)."""
    c = short
    for L in (0, 6):
        lg = c.tf_win(eng_bf16, L)[0].cpu()
        flg = c.forced_steps(eng_bf16, L).cpu()
        ref = c.forced(L)
        e_pass = (lg - ref).abs().amax(-1)[c.inside].max().item()
        e_steps = (flg - ref).abs().amax(-1)[c.inside].max().item()
        d = (lg - flg).abs().amax(-1)[c.inside].max().item()
        print("bf16 decode_tf_win L=%d: max |logits - f32 checker| one pass %.3e, forced steps %.3e; largest |one pass - forced steps| %.3e"
              % (L, e_pass, e_steps, d))
        assert torch.isfinite(lg).all()
        assert e_pass <= 2 * e_steps + 1e-3


@pytest.mark.parametrize("L", [0, -3, 2])
def test_decode_tf_win_does_not_see_perturbed_frames(eng, short, L):
    from dimx.online import visible
    c, f = short, 17
    v_s2, v_a2 = c.v_s.clone(), c.v_a.clone()
    v_s2[:, f:] += 0.5
    v_a2[:, f:] -= 0.5
    a = c.tf_win(eng, L)[0].cpu()
    b = c.tf_win(eng, L, v_s=v_s2, v_a=v_a2)[0].cpu()
    rows = torch.from_numpy(np.asarray(visible(np.arange(c.T - 1), L, c.T)) <= f)
    assert int(rows.sum()) == f - 1 - L
    assert torch.equal(a[:, rows], b[:, rows])
    first = int(rows.sum())
    assert not torch.equal(a[0, first], b[0, first]) and not torch.equal(a[1, first], b[1, first])


# ---------------------------------------------------------------- 6: the windowed prompt prefill
def _from_column(n0, tok, lg, ref):
    return tok[:, n0:], lg[:, n0:], tuple(t[:, n0:] for t in ref)


def _prompted(eng, c, Pmax, P0, plen, noisy, L, window, **kw):
    prompt = c.z[:, :Pmax].to(torch.int32).cuda().contiguous()
    plen_t = None if plen is None else torch.tensor(plen, dtype=torch.int32).cuda()
    c.context(eng, prompt_frames=P0, **kw)
    tok, lg = eng.generate(None, c.m8, c.T, 1.0 if noisy else 0.0, 52, c.noise.cuda() if noisy else None, return_logits=True, prompt=prompt,
                           prompt_len=plen_t, prefill=("window", P0) if window else P0, lookahead=L)
    return tok.cpu().long(), lg.cpu()


@pytest.mark.parametrize("noisy", [False, True])
@pytest.mark.parametrize("L", PROMPT_LOOKAHEADS)
@pytest.mark.parametrize("Pmax,P0,plen", PROMPT_CFG)
def test_windowed_prompt_prefill(eng, short, Pmax, P0, plen, L, noisy):
    c = short
    n0 = P0 - 1
    tok, lg = _prompted(eng, c, Pmax, P0, plen, noisy, L, True)
    ftok, flg = _prompted(eng, c, Pmax, P0, plen, noisy, L, False)       # the same call without the flag: forced steps
    ref = c.checker(L, noisy, Pmax, plen)
    what = "windowed prefill Pmax=%d P0=%d plen=%s L=%d noisy=%d" % (Pmax, P0, plen, L, noisy)
    assert n0 == 0 or float(lg[:, :n0].abs().max()) == 0.0          # the prefill forms no logits
    eff = [Pmax] * c.B if plen is None else [min(max(p, P0), Pmax) for p in plen]
    for b, p in enumerate(eff):
        assert torch.equal(tok[b, :p - 1], c.z[b, 1:p].clamp(min=0)), what
    _against_checker(what, *_from_column(n0, tok, lg, ref))
    _against_checker(what + " against forced steps", *_from_column(n0, tok, lg, (ftok, flg, ref[2])))


def test_windowed_prefill_without_the_window_is_the_plain_prefill(eng, short):
    c = short
    a = _prompted(eng, c, 17, 17, None, True, None, True)
    b = _prompted(eng, c, 17, 17, None, True, None, False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_windowed_prefill_across_a_row_tile(eng, full_sd):
    import online_ref
    import prompt_ref
    B, T, lens = LONG
    P, L = 131, 0
    v_s, v_a, z, mask = _case(B, T, list(lens))
    m8 = mask.to(torch.uint8).cuda()
    prompt = z[:, :P].to(torch.int32).cuda().contiguous()
    ref = online_ref.online_generate(full_sd, z[:, :P], None, T - 1, prompt_ref.case_context(full_sd, v_s, v_a, mask), mask, L)
    eng.encode_ctx(v_s.cuda(), v_a.cuda(), m8, True, prompt_frames=P)
    tok, lg = eng.generate(None, m8, T, 0.0, return_logits=True, prompt=prompt, prefill=("window", P), lookahead=L)
    _against_checker("windowed prefill T=150 P0=131", *_from_column(P - 1, tok.cpu().long(), lg.cpu(), ref))


def test_samples_share_the_windowed_prefill(eng, full_sd):
    B, T, S, P, L = 2, 40, 5, 9, 0
    v_s, v_a, z, mask = _case(B, T, [40, 33])
    m8 = mask.to(torch.uint8).cuda()
    prompt = z[:, :P].to(torch.int32).cuda().contiguous()
    eng.encode_ctx(v_s.cuda(), v_a.cuda(), m8, True, n_samples=S, prompt_frames=P)
    tok = eng.generate(None, m8, T, 1.0, 52, None, 7, n_samples=S, prompt=prompt, prefill=("window", P), lookahead=L).cpu()
    assert tok.shape == (B * S, T - 1)
    for r in range(B * S):
        assert torch.equal(tok[r, :P - 1], prompt[r // S, 1:].cpu())
    try:
        for b in range(B):
            for s in (0, 2, 4):      # three separate calls per clip
                eng.set_shard(b * S + s, B * S)
                eng.encode_ctx(v_s[b:b + 1].cuda(), v_a[b:b + 1].cuda(), m8[b:b + 1].contiguous(), True, prompt_frames=P)
                one = eng.generate(None, m8[b:b + 1].contiguous(), T, 1.0, 52, None, 7, prompt=prompt[b:b + 1].contiguous(),
                                   prefill=("window", P), lookahead=L).cpu()
                assert torch.equal(one[0], tok[b * S + s]), "clip %d sample %d" % (b, s)
    finally:
        eng.set_shard(0, 0)
    assert len({tuple(r.tolist()) for r in tok}) > B


# ---------------------------------------------------------------- 7: a session from a prompt
SB, ST, STMAX = 3, 40, 48


class _Clip:
    """the 40-frame clip, its context, the checker's prompted runs and the whole-clip windowed-prefill runs: computed once"""

    def __init__(self, sd):
        import prompt_ref
        self.sd = sd
        self.v_s, self.v_a, self.z, self.mask = _case(SB, ST, [ST] * SB, seed=WIN_SEED)
        self.ctx = prompt_ref.case_context(sd, self.v_s, self.v_a, self.mask)
        self.m8 = self.mask.to(torch.uint8).cuda()
        self.vs_d, self.va_d = self.v_s.cuda(), self.v_a.cuda()
        self.zd = self.z.to(torch.int32).cuda().contiguous()
        self._ref, self._whole = {}, {}

    def checker(self, L, P):
        import online_ref
        if (L, P) not in self._ref:
            self._ref[(L, P)] = online_ref.online_generate(self.sd, self.z[:, :P], None, ST - 1, self.ctx, self.mask, L)
        return self._ref[(L, P)]

    def whole(self, eng, L, P):
        if (L, P) not in self._whole:
            eng.encode_ctx(self.vs_d, self.va_d, self.m8, True, prompt_frames=P)
            tok, lg = eng.generate(None, self.m8, ST, 0.0, return_logits=True, prompt=self.zd[:, :P].contiguous(),
                                   prefill=("window", P) if P > 1 else None, lookahead=L)
            self._whole[(L, P)] = (tok.cpu().long(), lg.cpu())
        return self._whole[(L, P)]


@pytest.fixture(scope="module")
def clip(full_sd):
    return _Clip(full_sd)


def _run_session(eng, c, L, F, P, chunking, session=None):
    """begin from P codes and F frames, push the rest by `chunking`, end; checks the schedule -> tokens [B, 39], logits"""
    from dimx import stream
    kw = dict(prompt=c.zd[:, :P].contiguous(), v_speaker=c.vs_d[:, :F].contiguous(), v_audio=c.va_d[:, :F].contiguous())
    s = session
    if s is None:
        s = eng.stream(SB, STMAX, None, lookahead=L, temperature=0.0, **kw)
    else:
        s.begin(None, 0.0, 52, None, 0, **kw)
    try:
        assert s.state() == (F, P - 1, True) and s.steps == P - 1 and s.frames == F and s.tokens.shape == (SB, P - 1)
        assert torch.equal(s.tokens.cpu(), c.zd[:, 1:P].cpu())
        sched = stream.schedule(chunking, L, F=F, P=P)
        n = F
        for ch, (frames, lo, hi) in zip(chunking, sched):
            out = s.push(c.vs_d[:, n:n + ch], c.va_d[:, n:n + ch], return_logits=True)
            n += ch
            assert n == frames and s.state() == (n, hi, True) and out[0].shape == (SB, hi - lo), (chunking, n)
        tail = s.end(return_logits=True)
        assert tail[0].shape == (SB, sched[-1][2] - sched[-1][1]) and s.steps == ST - 1 and s.state() == (0, 0, False)
        lg = s._lg[:, :s.steps].cpu()
        assert P == 1 or float(lg[:, :P - 1].abs().max()) == 0.0
        return s.tokens.cpu().long(), lg
    finally:
        s.close()


@pytest.mark.parametrize("case", [0, 1, 2])
@pytest.mark.parametrize("L", SESSION_LOOKAHEADS)
def test_session_from_a_prompt(eng, clip, L, case):
    from dimx import stream
    F, P = session_cases(L)[case]
    assert stream.prompt_fits(P, L, F, STMAX)
    n = ST - F
    w_tok, w_lg = clip.whole(eng, L, P)
    ref = clip.checker(L, P)
    for chunking in ([1] * n, stream.chunks(n, [17, 1, ST]), [n]):
        tok, lg = _run_session(eng, clip, L, F, P, chunking)
        what = "session from a prompt L=%d F=%d P=%d chunks %s.. (%d)" % (L, F, P, chunking[:3], len(chunking))
        assert tok.shape == (SB, ST - 1)
        _against_checker(what, *_from_column(P - 1, tok, lg, ref))
        _against_checker(what + " against generate(prefill='window')", *_from_column(P - 1, tok, lg, (w_tok, w_lg, ref[2])))


@pytest.mark.parametrize("L", [0, 2])
def test_one_code_prompt_is_begin_and_a_push(eng, clip, L):
    F, rest = 17, [1, 16, 6]
    with eng.stream(SB, STMAX, clip.zd[:, 0].contiguous(), lookahead=L, temperature=0.0) as s:
        n = 0
        for ch in [F] + rest:
            s.push(clip.vs_d[:, n:n + ch], clip.va_d[:, n:n + ch], return_logits=True)
            n += ch
        s.end(return_logits=True)
        tok, lg = s.tokens.clone(), s._lg[:, :s.steps].clone()
    ptok, plg = _run_session(eng, clip, L, F, 1, rest)
    assert torch.equal(tok.cpu().long(), ptok) and torch.equal(lg.cpu(), plg)


def test_prompted_session_does_not_depend_on_the_workspace_contents(eng, clip):
    L, F, P, chunking = 2, 17, 15, [7, 16]
    s = eng.stream(SB, STMAX, clip.zd[:, 0].contiguous(), lookahead=L, temperature=0.0)
    s.close()
    _run_session(eng, clip, L, F, P, chunking, s)      # the first prompted begin sizes the workspace
    runs = []
    for fill in (0x00, 0xFF):
        s._ws.fill_(fill)
        runs.append(_run_session(eng, clip, L, F, P, chunking, s))
    for tok, lg in runs[1:]:
        assert torch.isfinite(lg).all() and torch.equal(tok, runs[0][0]) and torch.equal(lg, runs[0][1])


def test_prompted_begin_state_machine_and_refusals(eng, clip):
    from dimx import lib as L
    lib, h, c = eng.lib, eng.h, clip
    eng.encode_ctx(c.vs_d, c.va_d, c.m8, True)
    before = eng.generate(c.zd[:, 0].contiguous(), c.m8, ST, 0.0, return_logits=True)
    s = eng.stream(SB, STMAX, c.zd[:, 0].contiguous(), lookahead=2, temperature=0.0)
    s.close()
    need = lib.dimx_stream_workspace_bytes_prompt(h, SB, STMAX)
    assert need >= lib.dimx_stream_workspace_bytes(h, SB, STMAX) > 0
    assert lib.dimx_stream_workspace_bytes_prompt(h, SB, 2049) == 0 and lib.dimx_stream_workspace_bytes_prompt(h, SB, 1) == 0
    wsbuf = torch.empty(need + 256, dtype=torch.uint8, device="cuda")
    ws = ctypes.c_void_p((wsbuf.data_ptr() + 255) // 256 * 256)
    vs, va = c.vs_d[:, :17].contiguous(), c.va_d[:, :17].contiguous()
    prompt = c.zd[:, :17].contiguous()

    def begin(P=15, F=17, Tmax=STMAX, lookahead=2, p=prompt, v=vs, a=va, ld=17, wsb=need):
        return lib.dimx_stream_begin_prompted(h, L.ptr(p), ld, P, L.ptr(v), L.ptr(a), F, SB, Tmax, lookahead, 0.0, 52, None, 0, ws, wsb, eng._s())

    assert begin(P=16) == ERR_ARG            # P + max(L, 0) > F
    assert begin(P=0) == ERR_ARG and begin(P=-3) == ERR_ARG
    assert begin(F=17, Tmax=16) == ERR_ARG   # F > Tmax
    assert begin(p=None) == ERR_ARG and begin(v=None) == ERR_ARG and begin(a=None) == ERR_ARG
    assert begin(ld=14) == ERR_ARG
    assert begin(wsb=4096) == -5
    assert s.state() == (0, 0, False)
    with pytest.raises(ValueError):
        s.begin(None, 0.0, prompt=prompt[:, :16].contiguous(), v_speaker=vs, v_audio=va)
    assert begin() == 0 and s.state() == (17, 14, True)
    assert begin() == ERR_STATE and s.state() == (17, 14, True)          # open: state first
    assert lib.dimx_stream_abort(h) == 0 and s.state() == (0, 0, False)
    torch.cuda.synchronize()
    eng.encode_ctx(c.vs_d, c.va_d, c.m8, True)
    after = eng.generate(c.zd[:, 0].contiguous(), c.m8, ST, 0.0, return_logits=True)
    assert torch.equal(after[0], before[0]) and torch.equal(after[1], before[1])


# ---------------------------------------------------------------- 8: the host layers
@pytest.fixture(scope="module")
def model():
    from dimx.seq2seq_pretrain import SLMFT
    return SLMFT().eval()


def test_score_in_one_pass(model):
    B, T, lens = 3, 40, [40, 33, 7]
    dev = [t.cuda() for t in _clips(B, T, lens)]
    for L in (0, -3, 6):
        steps = model.score(*dev, lookahead=L)
        one = model.score(*dev, lookahead=L, one_pass=True)
        count = steps.count.cpu().numpy()
        assert np.array_equal(one.count.cpu().numpy(), count)
        d = np.abs(one.score.cpu().numpy() - steps.score.cpu().numpy()) / count
        print("score(lookahead=%d): one pass against forced steps, per-token log-probability differs by %s" % (L, d))
        assert d.max() <= 2 * STEP_TOL      # a log-softmax moves by at most twice the largest logit error (test_gpu_online.py)
    assert model.engine(dev[0].device).cross_lookahead() is None


def test_forward_and_test_epoch_with_a_windowed_prefill(model):
    from dimx import x_engine_pt
    B, T, lens, P = 3, 40, [40, 33, 7], 17
    v_s, v_l, v_a, mask = [t.cuda() for t in _clips(B, T, lens)]
    _, z_l = model.forward_vq(v_s, v_l, mask, with_speaker=False)
    out = {}
    for wp in (False, True):
        out[wp] = model(v_s, v_l, v_a, mask, mode="val", greedy=True, prompt_frames=P, lengths=lens, lookahead=0, window_prefill=wp,
                        return_tokens=True)[3]
        for b, n in enumerate(lens):
            assert torch.equal(out[wp][b, :min(n, P) - 1], z_l[b, 1:min(n, P)])
    agree = (out[True] == out[False]).long().cummin(1).values.sum(1)
    print("forward(window_prefill=True): steps before a row's first token that differs from the forced-step form: %s of %d" % (agree.tolist(), T - 1))
    assert int(agree.min()) >= P - 1
    loader = []
    for i, ln in enumerate(([32, 20, 11], [32, 25])):
        a, b, cc, m = _clips(len(ln), 32, ln, seed=30 + i)
        loader.append((torch.cat([a, cc], -1) * m[..., None], b * m[..., None], ln, None, ["clip%d_%d" % (i, j) for j in range(len(ln))]))
    torch.manual_seed(1234)
    y_true, y_pred, x, ids = x_engine_pt.evaluate_test_epoch(model, loader, torch.device("cuda:0"), beam_size=2, prompt_frames=9, lookahead=0,
                                                             window_prefill=True)
    assert len(ids) == 5 and all(np.isfinite(a).all() for a in y_pred)


def test_evaluate_finetune_epoch_with_a_lookahead(model):
    from dimx import x_engine_pt
    T, L = 32, 0
    loader, batches = [], []
    for i, lens in enumerate(([32, 20, 11], [32, 25])):
        v_s, v_l, v_a, mask = _clips(len(lens), T, lens, seed=30 + i)
        src = torch.cat([v_s, v_a], -1) * mask[..., None]
        loader.append((src, v_l * mask[..., None], lens, None, ["clip%d_%d" % (i, j) for j in range(len(lens))]))
        batches.append(lens)
    dev = torch.device("cuda:0")
    off = x_engine_pt.evaluate_finetune_epoch(model, loader, dev)
    assert len(off) == 4      # lookahead=None: the offline epoch's four lists
    y_true, y_pred, x, ids, loss = x_engine_pt.evaluate_finetune_epoch(model, loader, dev, lookahead=L)
    assert [a.shape for a in y_pred] == [(n - 1, 56) for lens in batches for n in lens] and len(ids) == 5
    # the loss: decode_tf_win's row_loss, summed over the valid targets of a batch / their number, averaged over the batches
    eng = model.engine(dev)
    want = []
    for batch in loader:
        src_s_v, src_s_a, tgt, mask, src_len, _ = x_engine_pt._prepare(batch, dev)
        _, z_l = model.forward_vq(src_s_v, tgt, mask.bool(), with_speaker=False)
        m8 = mask.bool().to(torch.uint8).contiguous()
        eng.encode_ctx(src_s_v, src_s_a, m8, True)
        _, row_loss, _ = eng.decode_tf(z_l, m8, None, lookahead=L)
        want.append((row_loss.sum() / (z_l[:, 1:] != -100).sum()).item())
    assert abs(loss - float(np.mean(want))) <= 1e-6 * max(1.0, abs(loss))
    assert np.isfinite(loss) and loss > 0
