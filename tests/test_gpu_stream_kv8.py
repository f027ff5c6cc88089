"""GPU: FP8 K/V for streaming sessions (dimx_stream_set_kv8) -- the incremental quantiser (dimx_op_kv8_append,
csrc/decode_attn_kv8.hip kv8_append_kernel) against dimx_op_kv8_quantize bit for bit, the session's buffer against the quantiser on
the session's own plain rows under every chunking, its tokens and logits against the CPU checkers (tests/kv8_ref.py,
tests/self_kv8_ref.py) run on the buffers' own dequantised rows, the frontier, the restart, the opt-in and the refusals."""
import ctypes

import pytest
import torch

from test_gpu_prompt import STEP_TOL, _case, _noise
from test_kv8_host import MARGIN, MAX_LEFT_OUT
from test_stream_host import CHUNKINGS
from test_stream_kv8_host import LOOKAHEADS, STREAM_KV8_CASE, STREAM_KV8_SEED

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
B, T, TMAX = STREAM_KV8_CASE
TP = (TMAX + 7) // 8 * 8
CHECKED = [[1] * 40, [17, 1, 22], [40]]
MODES = {"cross": (True, False), "self": (False, True), "both": (True, True)}
ERR_ARG, ERR_STATE, ERR_WORKSPACE = -1, -4, -5


def _cid(c):
    return "x".join(map(str, c[:3])) + "_%d" % len(c)


def _raw(t):
    return t.contiguous().view(torch.uint8)


# ---------------------------------------------------------------- 1: the operator
OB, OH = 3, 12
N0S, CS = (0, 1, 15, 16, 17, 31), (1, 2, 5, 16, 17)


def _op_caches(depth, dtype):
    """2 * depth caches [3, 12, 48, 64] of row magnitudes 2**-3 .. 2**3 with a zero row, and the whole-cache quantiser's planes"""
    from dimx import engine as E
    g = torch.Generator().manual_seed(100 + depth)
    caches = []
    for i in range(2 * depth):
        x = torch.randn(OB, OH, TP, 64, generator=g) * torch.exp2(torch.randint(-3, 4, (OB, OH, TP, 1), generator=g).float())
        x[1, 2, 16] = 0.0
        caches.append(x.to(dtype).cuda())
    return caches, [E.op_kv8_quantize(x) for x in caches]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("depth", [1, 4])
def test_append_is_the_quantiser_on_its_rows_and_touches_nothing_else(depth, dtype):
    from dimx import engine as E
    caches, ref = _op_caches(depth, dtype)
    assert all(int((c & 0x7F).amax()) == 0x7E and bool((s[1, 2, 16] == 0)) for c, s in ref)
    for n0 in N0S:
        for c in CS:
            what = "depth=%d n0=%d c=%d" % (depth, n0, c)
            rows = slice(n0, n0 + c)
            runs = []
            for _ in range(2):
                poisoned = []
                for x in caches:       # rows outside the range are NaN: they change nothing
                    p = torch.full_like(x, float("nan"))
                    p[:, :, rows] = x[:, :, rows]
                    poisoned.append(p)
                codes = [torch.full((OB, OH, TP, 64), 0xAB, dtype=torch.uint8, device="cuda") for _ in caches]
                scales = [torch.full((OB, OH, TP), -7.0, device="cuda") for _ in caches]
                E.op_kv8_append(poisoned, codes, scales, n0, c)
                runs.append((codes, scales))
            keep = torch.ones(TP, dtype=torch.bool)
            keep[rows] = False
            for i, (cd, sc) in enumerate(zip(*runs[0])):
                assert torch.equal(cd[:, :, rows], ref[i][0][:, :, rows]), "%s: codes of cache %d differ from the quantiser's" % (what, i)
                assert torch.equal(_raw(sc[:, :, rows]), _raw(ref[i][1][:, :, rows])), "%s: scales of cache %d differ from the quantiser's" % (what, i)
                assert bool((cd[:, :, keep] == 0xAB).all()) and bool((sc[:, :, keep] == -7.0).all()), "%s: a row outside the range was written" % what
                assert torch.equal(cd, runs[1][0][i]) and torch.equal(_raw(sc), _raw(runs[1][1][i])), "%s: a repeat differs" % what


def test_append_refuses_misuse_before_the_launch():
    """planes of 2056 rows per (clip, head): every refused argument list would stay inside them"""
    from dimx import lib as L
    l = L.load()
    Bq, Hq, Tq = 2, 3, 2056
    cache = torch.zeros(2, Bq * Hq * Tq * 64, device="cuda")
    codes = torch.full((2, Bq * Hq * Tq * 64), 0xAB, dtype=torch.uint8, device="cuda")
    scales = torch.full((2, Bq * Hq * Tq + 4), -7.0, device="cuda")
    arr = lambda ps: (ctypes.c_void_p * len(ps))(*ps)
    good = dict(dt=L.F32, ca=[cache[0].data_ptr(), cache[1].data_ptr()], co=[codes[0].data_ptr(), codes[1].data_ptr()],
                sc=[scales[0].data_ptr(), scales[1].data_ptr()], depth=1, Tc=2048, Tp=2048, n0=5, c=3)

    def call(**kw):
        a = dict(good, **kw)
        return l.dimx_op_kv8_append(a["dt"], arr(a["ca"]) if a["ca"] else None, arr(a["co"]) if a["co"] else None,
                                    arr(a["sc"]) if a["sc"] else None, a["depth"], Bq, Hq, a["Tc"], a["Tp"], a["n0"], a["c"], L.stream_ptr(cache.device))

    def alt(key, i, val):
        ps = list(good[key])
        ps[i] = val
        return {key: ps}
    bad = [dict(dt=7), dict(depth=0), dict(depth=9), dict(c=0), dict(c=-1), dict(n0=-1), dict(n0=2046, c=3), dict(Tc=7, n0=5, c=3), dict(Tp=2056),
           dict(ca=None), dict(co=None), dict(sc=None), alt("ca", 1, None), alt("co", 0, None), alt("sc", 1, None),
           alt("ca", 0, cache[0].data_ptr() + 8), alt("co", 1, codes[1].data_ptr() + 8), alt("sc", 0, scales[0].data_ptr() + 2)]
    for kw in bad:
        assert call(**kw) == ERR_ARG, kw
    torch.cuda.synchronize()
    assert bool((codes == 0xAB).all()) and bool((scales == -7.0).all()), "a refused call launched something"
    assert call() == 0
    torch.cuda.synchronize()
    cd = codes[:, :Bq * Hq * 2048 * 64].view(2, Bq * Hq, 2048, 64)
    sc = scales[:, :Bq * Hq * 2048].view(2, Bq * Hq, 2048)
    assert bool((sc[:, :, 5:8] == 0).all()) and not bool(cd[:, :, 5:8].any())       # the caches hold zero rows
    assert bool((cd[:, :, :5] == 0xAB).all()) and bool((cd[:, :, 8:] == 0xAB).all()) and bool((codes[:, Bq * Hq * 2048 * 64:] == 0xAB).all())
    assert bool((sc[:, :, :5] == -7.0).all()) and bool((sc[:, :, 8:] == -7.0).all())


# ---------------------------------------------------------------- the session
class _Clip:
    """the 40-frame clips under the seed tests/test_stream_kv8_host.py chose, built once and left unchanged"""

    def __init__(self, sd):
        self.sd = sd
        self.v_s, self.v_a, self.z, self.mask = _case(B, T, [T] * B, seed=STREAM_KV8_SEED)
        self.noise48, self.noise40 = _noise(B, TMAX), _noise(B, T)
        self.m8 = self.mask.to(torch.uint8).cuda()
        self.start = self.z[:, 0].to(torch.int32).cuda()
        self.vs_d, self.va_d = self.v_s.cuda(), self.v_a.cuda()
        self.shape_only = torch.empty(B, T, 1)     # the checkers get every cross row handed: they ask the context for its shape
        self._plain = {}


class _Run:
    """one session fed the clip: tokens, logits, the plain cross rows and the FP8 buffers it left, all on the host"""

    def __init__(self, eng, c, L, noisy, chunking, kv8, self_kv8, fill=0xFF, fill_ws=None, vs=None, va=None, prompt=None, F=0):
        vs = c.vs_d if vs is None else vs
        va = c.va_d if va is None else va
        s = eng.stream(B, TMAX, c.start, lookahead=L, temperature=1.0 if noisy else 0.0, top_k=52, noise=c.noise48.cuda() if noisy else None,
                       kv8=kv8, self_kv8=self_kv8)
        s.close()
        t0 = eng.lib.dimx_kv0_table_generations(eng.h)
        for buf in (s._kv8, s._skv8):
            if buf is not None:
                buf.fill_(fill)
        if fill_ws is not None:
            s._ws.fill_(fill_ws)
        assert eng.stream_kv8() == (None, None)
        if prompt is None:
            s.begin(c.start, 1.0 if noisy else 0.0, 52, c.noise48.cuda() if noisy else None, 0)
        else:
            s.begin(None, 1.0 if noisy else 0.0, 52, c.noise48.cuda() if noisy else None, 0, prompt=prompt, v_speaker=vs[:, :F].contiguous(),
                    v_audio=va[:, :F].contiguous())
        want = (None if s._kv8 is None else (s._kv8.data_ptr(), s._kv8.numel()), None if s._skv8 is None else (s._skv8.data_ptr(), s._skv8.numel()))
        assert eng.stream_kv8() == want
        n = F
        for ch in chunking:
            s.push(vs[:, n:n + ch], va[:, n:n + ch], return_logits=True)
            n += ch
        s.end(return_logits=True)
        assert n == T and s.steps == T - 1 and eng.stream_kv8() == (None, None)      # the session cleared the handle's setting
        self.table0 = eng.lib.dimx_kv0_table_generations(eng.h) > t0
        self.session = s
        self.tok, self.lg = s.tokens.cpu().long(), s._lg[:, :s.steps].cpu()
        self.plain_dev = s.cross_kv_layers()
        self.plain = [(k[:, :, :T].float().cpu(), v[:, :, :T].float().cpu()) for k, v in self.plain_dev]
        self.cross8 = [tuple(t.cpu().clone() for t in lay) for lay in s.cross_kv8_layers()] if kv8 else None
        self.self8 = [tuple(t.cpu().clone() for t in lay) for lay in s.self_kv8_layers()] if self_kv8 else None

    def cross_rows(self):
        import kv8_ref
        return kv8_ref.dequantized(self.cross8, T) if self.cross8 else self.plain

    def self_rows(self, n=T - 1):
        import self_kv8_ref
        if not self.self8:
            return None
        rows = self_kv8_ref.dequantized(self.self8, n)
        return [None] + rows[1:] if self.table0 else rows


def _check(c, run, L, noisy, Pmax=1, what=""):
    """the checker on the rows the session left, replayed along the session's tokens: (its choices, logits, margins)"""
    import online_ref
    import self_kv8_ref
    hook = self_kv8_ref.SelfRows(given=run.self_rows())
    ref_tok, ref_lg, margins = self_kv8_ref.self_kv8_generate(c.sd, c.z[:, :Pmax], None, T - 1, c.shape_only, c.mask, L, hook,
                                                              c.noise40 if noisy else None, cross_kv=run.cross_rows(), follow=run.tok)
    keep, left_out = online_ref.compared_steps(margins, MARGIN)
    keep_lg = keep.clone()
    keep_lg[:, 1:] |= keep[:, :-1]
    keep_lg[:, 0] = True
    keep[:, :Pmax - 1] = keep_lg[:, :Pmax - 1] = False         # a prompt's columns: nothing was decided, no logits were formed
    err = (run.lg - ref_lg).abs().amax(-1)
    wrong = int(((run.tok != ref_tok) & keep).sum())
    print("%s: %d compared tokens differ, max |logits - checker| %.3e over the compared steps, smallest margin %.3e, pairs left out %.4f"
          % (what, wrong, err[keep_lg].max().item(), margins.min().item(), left_out))
    assert left_out <= MAX_LEFT_OUT
    assert wrong == 0
    assert err[keep_lg].max().item() < STEP_TOL
    return ref_lg, hook


def _engine(sd, mode="f32"):
    from dimx import engine, lib
    e = engine.Engine("cuda:0", lib.MODE_PARITY_F32 if mode == "f32" else lib.MODE_PERF_BF16)
    e.load_state_dict(sd)
    return e


@pytest.fixture(scope="module")
def eng(full_sd):
    return _engine(full_sd)


@pytest.fixture(scope="module")
def clip(full_sd):
    return _Clip(full_sd)


def _plain_session(eng, c, L, noisy, chunking):
    key = (L, noisy, tuple(chunking))
    if key not in c._plain:
        r = _Run(eng, c, L, noisy, chunking, False, False)
        c._plain[key] = (r.tok, r.lg)
    return c._plain[key]


# ---- 2
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_buffer_holds_the_quantiser_of_the_sessions_own_rows_under_every_chunking(full_sd, eng, clip, mode):
    from dimx import engine as E
    e = eng if mode == "f32" else _engine(full_sd, "bf16")
    for chunking in CHUNKINGS:
        run = _Run(e, clip, 0, False, chunking, True, False)
        assert len(run.cross8) == 4
        for l, ((k, v), (kc, vc, ks, vs)) in enumerate(zip(run.plain_dev, run.cross8)):
            assert tuple(kc.shape) == (B, 12, TP, 64) and tuple(ks.shape) == (B, 12, TP) and tuple(k.shape) == (B, 12, TP, 64)
            for cache, codes, scales in ((k, kc, ks), (v, vc, vs)):
                want_c, want_s = E.op_kv8_quantize(cache, T)
                what = "%s %s layer %d" % (mode, _cid(chunking), l)
                assert torch.equal(codes[:, :, :T], want_c[:, :, :T].cpu()), what
                assert torch.equal(_raw(scales[:, :, :T]), _raw(want_s[:, :, :T].cpu())), what
                assert bool((scales[:, :, :T] > 0).all()) and int((codes[:, :, :T] & 0x7F).amax(-1).min()) == 0x7E, what
                assert bool((codes[:, :, T:] == 0xFF).all()) and bool((_raw(scales[:, :, T:]) == 0xFF).all()), what + ": a row past T was written"
    if e is not eng:
        e.close()


# ---- 3
@pytest.mark.parametrize("noisy", [False, True])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("L", LOOKAHEADS)
def test_session_matches_the_checker_on_the_buffers_rows(eng, clip, L, mode, noisy):
    kv8, self_kv8 = MODES[mode]
    for chunking in CHECKED:
        run = _Run(eng, clip, L, noisy, chunking, kv8, self_kv8)
        ref_lg, _ = _check(clip, run, L, noisy, what="session L=%d %s noisy=%d %s" % (L, mode, noisy, _cid(chunking)))
        # a plain session along the same inputs is further from the checker than that: the codes are what was read
        ptok, plg = _plain_session(eng, clip, L, noisy, chunking)
        common = torch.cat([torch.ones(B, 1), (ptok == run.tok).float().cumprod(1)[:, :-1]], 1).bool()
        d = (plg - ref_lg).abs().amax(-1)
        print("    the plain session: max |logits - checker| %.3e (%.3e over the common history)" % (d.max().item(), d[common].max().item()))
        assert d.max().item() > STEP_TOL


# ---- 4
def test_buffer_and_workspace_contents_and_repeats_do_not_matter(eng, clip):
    chunking = [7] * 5 + [5]
    runs = [_Run(eng, clip, 2, True, chunking, True, True, fill=f, fill_ws=f) for f in (0x00, 0xFF)]
    a, b = runs
    assert torch.equal(a.tok, b.tok) and torch.equal(a.lg, b.lg) and bool(torch.isfinite(a.lg).all())
    s = a.session       # repeated sessions in the same buffers
    for _ in range(2):
        s.begin(clip.start, 1.0, 52, clip.noise48.cuda(), 0)
        n = 0
        for ch in chunking:
            s.push(clip.vs_d[:, n:n + ch], clip.va_d[:, n:n + ch], return_logits=True)
            n += ch
        s.end(return_logits=True)
        assert torch.equal(s.tokens.cpu().long(), a.tok) and torch.equal(s._lg[:, :s.steps].cpu(), a.lg)
        for lay, want in zip(s.cross_kv8_layers(), a.cross8):
            assert all(torch.equal(_raw(x[:, :, :T].cpu()), _raw(w[:, :, :T])) for x, w in zip(lay, want))
        for lay, want in zip(s.self_kv8_layers()[1:], a.self8[1:]):
            assert all(torch.equal(_raw(x[:, :, :T - 1].cpu()), _raw(w[:, :, :T - 1])) for x, w in zip(lay, want))


@pytest.mark.parametrize("chunking", [[1] * 40, [17, 1, 22]], ids=_cid)
@pytest.mark.parametrize("L", [0, -3])
def test_tokens_do_not_depend_on_frames_not_yet_pushed(eng, clip, L, chunking):
    from dimx import stream
    k = 17
    vs2, va2 = clip.vs_d.clone(), clip.va_d.clone()
    vs2[:, k:] += 0.5
    va2[:, k:] -= 0.5
    a = _Run(eng, clip, L, False, chunking, True, True)
    b = _Run(eng, clip, L, False, chunking, True, True, vs=vs2, va=va2)
    before = stream.steps_due(k, L)      # the steps that had run when frames 0 .. k-1 were all there was
    assert before > 0
    assert torch.equal(a.tok[:, :before], b.tok[:, :before]) and torch.equal(a.lg[:, :before], b.lg[:, :before])
    assert not torch.equal(a.lg[:, before:], b.lg[:, before:])
    for x, y in zip(a.cross8, b.cross8):       # the rows below frame k are the same bits, the later ones are not
        assert all(torch.equal(_raw(p[:, :, :k]), _raw(q[:, :, :k])) and not torch.equal(_raw(p[:, :, k:T]), _raw(q[:, :, k:T])) for p, q in zip(x, y))


# ---- 5
def test_restart_from_a_prompt_with_both_buffers(eng, clip):
    """F = 20 frames and P = 19 codes: the prefilled self rows 0 .. 17 are the quantiser's over what a plain teacher-forced pass
    projects, and the steps from 18 on match the checker seeded with the buffer's rows"""
    import numpy as np
    import self_kv8_ref
    from test_gpu_self_kv8 import _row_bound
    F, P, L = 20, 19, 0
    prompt = clip.z[:, :P].to(torch.int32).cuda().contiguous()
    run = _Run(eng, clip, L, False, [7, 13], True, True, prompt=prompt, F=F)
    assert not run.table0 and torch.equal(run.tok[:, :P - 1], clip.z[:, 1:P]) and not bool(run.lg[:, :P - 1].any())
    _check(clip, run, L, False, Pmax=P, what="restarted session, F=%d P=%d" % (F, P))
    plain = self_kv8_ref.SelfRows()
    self_kv8_ref.self_kv8_generate(clip.sd, clip.z[:, :P], None, P - 1, clip.shape_only, clip.mask, L, plain, cross_kv=run.plain)
    for (kc, vc, ks, vs), (k_new, v_new) in zip(run.self8, plain.new_rows()):
        for codes, scales, mine in ((kc, ks, k_new), (vc, vs, v_new)):
            d, m, bound = _row_bound(codes, scales, mine, P - 1)
            assert (np.abs(d - m) <= bound).all()
            assert bool((scales[:, :, :T - 1] > 0).all()) and bool((_raw(scales[:, :, T - 1:]) == 0xFF).all())


# ---- 6
def test_opt_in(full_sd, eng, clip):
    chunking = [17, 1, 22]
    eng.encode_ctx(clip.vs_d, clip.va_d, clip.m8, True)
    before = eng.generate(clip.start, clip.m8, T, 1.0, 52, clip.noise40.cuda(), return_logits=True)
    fp8 = _Run(eng, clip, 2, True, chunking, True, True)
    eng.encode_ctx(clip.vs_d, clip.va_d, clip.m8, True)
    after = eng.generate(clip.start, clip.m8, T, 1.0, 52, clip.noise40.cuda(), return_logits=True)
    assert torch.equal(after[0], before[0]) and torch.equal(after[1], before[1])        # an offline generate after an FP8 session
    fresh = _engine(full_sd)
    try:
        want = _Run(fresh, clip, 2, True, chunking, False, False)      # a handle that never had the setting
    finally:
        fresh.close()
    need = eng.cross_kv8_bytes(B, TMAX)
    bufs = [torch.full((need,), 0xAB, dtype=torch.uint8, device="cuda") for _ in range(2)]
    eng.stream_set_kv8(*bufs)
    assert eng.stream_kv8() == ((bufs[0].data_ptr(), need), (bufs[1].data_ptr(), need))
    eng.stream_set_kv8(None, None)
    got = _Run(eng, clip, 2, True, chunking, False, False)
    assert torch.equal(got.tok, want.tok) and torch.equal(got.lg, want.lg)
    assert not torch.equal(fp8.lg, want.lg)
    # the offline settings do not reach a session
    eng.set_cross_kv8(bufs[0])
    eng.set_self_kv8(bufs[1])
    try:
        got = _Run(eng, clip, 2, True, chunking, False, False)
    finally:
        eng.set_cross_kv8(None)
        eng.set_self_kv8(None)
    assert torch.equal(got.tok, want.tok) and torch.equal(got.lg, want.lg)
    torch.cuda.synchronize()
    assert all(bool((b == 0xAB).all()) for b in bufs)


# ---- 7
def test_refusals_launch_nothing(eng, clip):
    from dimx import engine
    from dimx import lib as L
    lib, h = eng.lib, eng.h
    need = eng.cross_kv8_bytes(B, TMAX)
    assert need == eng.self_kv8_bytes(B, TMAX) > 0
    buf = torch.full((need + 256,), 0xAB, dtype=torch.uint8, device="cuda")
    s = eng.stream(B, TMAX, clip.start)
    try:
        assert lib.dimx_stream_set_kv8(h, L.ptr(buf), need, None, 0) == ERR_STATE       # set while open
        assert lib.dimx_stream_set_kv8(h, None, 0, None, 0) == ERR_STATE
    finally:
        s.close()
    assert eng.stream_kv8() == (None, None)
    mis = ctypes.c_void_p(buf.data_ptr() + 16)
    assert lib.dimx_stream_set_kv8(h, mis, need, None, 0) == ERR_ARG and lib.dimx_stream_set_kv8(h, None, 0, mis, need) == ERR_ARG
    assert eng.stream_kv8() == (None, None)
    for variant in ("slm", "legacy"):
        other = engine.Engine("cuda:0", L.MODE_PARITY_F32, variant=variant)
        assert other.lib.dimx_stream_set_kv8(other.h, L.ptr(buf), need, None, 0) == ERR_ARG and b"variant" in other.lib.dimx_last_error()
        other.close()
    # one byte short: the begin answers, nothing opens
    ws, wsb = s._ws_ptr()
    tokens = torch.full((B, TMAX - 1), -7, dtype=torch.int32, device="cuda")
    for cross, self_ in (((L.ptr(buf), need - 1), (None, 0)), ((None, 0), (L.ptr(buf), need - 1)), ((L.ptr(buf), need), (L.ptr(buf), need - 1))):
        assert lib.dimx_stream_set_kv8(h, cross[0], cross[1], self_[0], self_[1]) == 0
        assert lib.dimx_stream_begin(h, L.ptr(clip.start), B, TMAX, 0, 0.0, 52, None, 0, ws, wsb, eng._s()) == ERR_WORKSPACE
        assert b"dimx_" in lib.dimx_last_error() and s.state() == (0, 0, False)
        n_new = ctypes.c_int(5)
        assert lib.dimx_stream_push(h, L.ptr(clip.vs_d[:, :4].contiguous()), L.ptr(clip.va_d[:, :4].contiguous()), 4, L.ptr(tokens), TMAX - 1, None,
                                    None, ctypes.byref(n_new), eng._s()) == ERR_STATE
    assert lib.dimx_stream_set_kv8(h, None, 0, None, 0) == 0
    torch.cuda.synchronize()
    assert bool((buf == 0xAB).all()) and bool((tokens == -7).all()), "a refused call launched something"


# ---- 8
def test_module_session_is_the_engine_session():
    from dimx.seq2seq_pretrain import SLMFT
    from test_gpu_prompt import _clips
    model = SLMFT().eval()
    v_s, v_l, v_a, mask = [t.cuda() for t in _clips(B, T, [T] * B)]
    _, z_l = model.forward_vq(v_s, v_l, mask, with_speaker=False)
    toks = []
    for opener in (model.stream, model.engine(v_s.device).stream):
        kw = dict(greedy=True) if opener == model.stream else dict(temperature=0.0)
        with opener(B, TMAX, z_l[:, 0], lookahead=2, kv8=True, self_kv8=True, **kw) as s:
            assert s._kv8 is not None and s._skv8 is not None
            n = 0
            for ch in (7, 16, 17):
                s.push(v_s[:, n:n + ch], v_a[:, n:n + ch])
                n += ch
            s.end()
            toks.append(s.tokens.clone())
    assert toks[0].shape == (B, T - 1) and torch.equal(toks[0], toks[1])
    with model.stream(B, TMAX, z_l[:, 0], lookahead=2, greedy=True) as s:
        s.push(v_s, v_a)
        s.end()
        print("SLMFT.stream(kv8=True, self_kv8=True): %.0f %% of the greedy tokens equal the plain session's"
              % (100 * (s.tokens == toks[0]).float().mean().item()))


# ---- 9
@pytest.mark.parametrize("L", [0, 2])
def test_report_against_the_offline_generation(eng, clip, L):
    """a report, no assertion: the incremental and the batch encoder agree to about 1e-6, not to the bit, so a code may land on the
    other side of a rounding boundary"""
    for noisy in (False, True):
        eng.encode_ctx(clip.vs_d, clip.va_d, clip.m8, True)
        tok, lg = eng.generate(clip.start, clip.m8, T, 1.0 if noisy else 0.0, 52, clip.noise40.cuda() if noisy else None, return_logits=True,
                               lookahead=L, kv8=True, self_kv8=True)
        tok, lg = tok.cpu().long(), lg.cpu()
        off8 = [tuple(t[:, :, :T].cpu() for t in lay) for lay in eng.cross_kv8_layers(B, T)]
        for chunking in ([17, 1, 22], [1] * 40):
            run = _Run(eng, clip, L, noisy, chunking, True, True)
            codes = sum(int((a[:, :, :T] != b).sum()) for x, y in zip(run.cross8, off8) for a, b in zip(x[:2], y[:2]))
            scales = sum(int((_raw(a[:, :, :T]) != _raw(b)).view(-1, 4).any(1).sum()) for x, y in zip(run.cross8, off8) for a, b in zip(x[2:], y[2:]))
            common = torch.cat([torch.ones(B, 1), (tok == run.tok).float().cumprod(1)[:, :-1]], 1).bool()
            d = (lg - run.lg).abs().amax(-1)
            print("f32 session (cross + self FP8) L=%d noisy=%d %s against generate(kv8, self_kv8): %d of %d tokens differ; largest logit difference "
                  "%.3e over the common history (%.3e over all steps); %d cross codes and %d cross scales of %d rows differ"
                  % (L, noisy, _cid(chunking), int((tok != run.tok).sum()), tok.numel(), d[common].max().item(), d.max().item(), codes, scales,
                     4 * 2 * B * 12 * T))
