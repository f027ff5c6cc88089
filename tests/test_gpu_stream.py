"""GPU: streaming sessions (dimx_stream_*, csrc/stream.hip) and their attention kernel (dimx_op_append_attn, csrc/stream_attn.hip):
the kernel against float64 and against itself under other chunkings, the session's encoder rows against the oracle, its tokens and
logits against the online CPU checker (tests/online_ref.py) and against the whole-clip Engine.generate(lookahead=L), its schedule,
its causality, its indifference to the workspace's contents, the chunked VQ decode, and the state machine."""
import ctypes

import pytest
import torch

from test_gpu_decode_step import tolerance
from test_gpu_online import ERR_ARG, _against_checker
from test_gpu_prompt import STEP_TOL, _case, _noise

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
B, T, TMAX = 3, 40, 48
CHUNKINGS = [[1] * 40, [7] * 5 + [5], [16, 16, 8], [17, 1, 22], [40]]
CHECKED = [[1] * 40, [17, 1, 22], [40]]
LOOKAHEADS = [0, -3, 2, 6, 40]
ERR_STATE, ERR_WORKSPACE = -4, -5
SCALE = 0.125


def _cid(c):
    return "x".join(map(str, c[:3])) + "_%d" % len(c)


# ---------------------------------------------------------------- 1, 2: the kernel
AB, AH, ATMAX = 2, 12, 56


class _Attn:
    """56 rows of q / k / v per (clip, head), computed once and left unchanged"""

    def __init__(self):
        from dimx import prng
        shape = (AB, ATMAX, 3 * AH * 64)
        self.qkv = torch.from_numpy(prng.normal(3, "stream.qkv", shape)).float().cuda()

    def rows(self, lo, hi):
        return self.qkv[:, lo:hi].contiguous()

    def kv(self, dtype):
        """K, V [B, H, Tmax, 64] as the cache holds them"""
        k = self.qkv[..., AH * 64:2 * AH * 64].view(AB, ATMAX, AH, 64).permute(0, 2, 1, 3)
        v = self.qkv[..., 2 * AH * 64:].view(AB, ATMAX, AH, 64).permute(0, 2, 1, 3)
        return k.to(dtype).contiguous(), v.to(dtype).contiguous()

    def ref(self, dtype, lo, hi):
        """float64: rows lo .. hi-1, each over the cache-rounded keys 0 .. its own position -> [B, hi-lo, H*64]"""
        k, v = self.kv(dtype)
        q = self.qkv[:, lo:hi, :AH * 64].view(AB, hi - lo, AH, 64)
        s = torch.einsum("bihd,bhjd->bhij", q.double(), k[:, :, :hi].double()) * SCALE
        j = torch.arange(hi, device=s.device)[None, :]
        i = torch.arange(lo, hi, device=s.device)[:, None]
        s = s.masked_fill(j > i, float("-inf"))
        o = torch.einsum("bhij,bhjd->bihd", s.softmax(-1), v[:, :, :hi].double())
        return o.reshape(AB, hi - lo, AH * 64).cpu()


@pytest.fixture(scope="module")
def attn():
    return _Attn()


SENTINEL = 777.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_append_attention_against_float64(attn, dtype):
    from dimx import engine as E
    bf = dtype == torch.bfloat16
    k, v = attn.kv(dtype)
    worst = 0.0
    for n0 in (0, 1, 15, 16, 17, 31, 32, 33):
        for c in (1, 2, 5, 16):
            ref = attn.ref(dtype, n0, n0 + c)
            outs = []
            for fill in (SENTINEL, float("nan")):
                kc = torch.full((AB, AH, ATMAX, 64), SENTINEL, dtype=dtype, device="cuda")
                vc = torch.full((AB, AH, ATMAX, 64), SENTINEL, dtype=dtype, device="cuda")
                kc[:, :, :n0], vc[:, :, :n0] = k[:, :, :n0], v[:, :, :n0]
                kc[:, :, n0 + c:], vc[:, :, n0 + c:] = fill, fill
                out = E.op_append_attn(attn.rows(n0, n0 + c), kc, vc, n0, SCALE)
                what = "n0=%d c=%d %s fill=%s" % (n0, c, "bf16" if bf else "f32", fill)
                assert torch.isfinite(out).all(), what
                err = (out.double().cpu() - ref).abs()
                tol = tolerance(ref, bf)
                assert (err <= tol).all(), "%s: max err %.3g (tol %.3g there)" % (what, err.max().item(), tol.flatten()[err.argmax()].item())
                worst = max(worst, err.max().item())
                # the new rows are the rounded inputs, every other row is what it was
                for cache, want in ((kc, k), (vc, v)):
                    assert torch.equal(cache[:, :, :n0 + c], want[:, :, :n0 + c]), what
                    rest = cache[:, :, n0 + c:]
                    assert bool(torch.isnan(rest).all()) if fill != fill else bool((rest == SENTINEL).all()), what
                outs.append(out)
            assert torch.equal(outs[0], outs[1]), "n0=%d c=%d: rows past the frontier reached the output" % (n0, c)
    print("append attention %s: largest |out - float64| %.3g" % ("bf16" if bf else "f32", worst))


def _append_all(attn, dtype, chunking):
    from dimx import engine as E
    kc = torch.full((AB, AH, ATMAX, 64), SENTINEL, dtype=dtype, device="cuda")
    vc = torch.full((AB, AH, ATMAX, 64), SENTINEL, dtype=dtype, device="cuda")
    outs, n = [], 0
    for c in chunking:
        outs.append(E.op_append_attn(attn.rows(n, n + c), kc, vc, n, SCALE))
        n += c
    return torch.cat(outs, 1), kc, vc


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_a_row_is_a_function_of_its_own_inputs(attn, dtype):
    one, kc1, vc1 = _append_all(attn, dtype, [1] * 40)
    for chunking in [[7] * 5 + [5], [16, 16, 8], [16, 2, 16, 5, 1], [4, 4, 16, 16]]:
        out, kc, vc = _append_all(attn, dtype, chunking)
        assert torch.equal(out, one), chunking
        assert torch.equal(kc, kc1) and torch.equal(vc, vc1), chunking


def test_append_attention_refuses_bad_shapes_without_a_launch(attn):
    from dimx import engine as E, lib as L
    kc = torch.full((AB, AH, ATMAX, 64), SENTINEL, device="cuda")
    for rows, n0 in ((attn.rows(0, 17), 0), (attn.rows(0, 4), ATMAX - 3), (attn.rows(0, 4), -1)):
        with pytest.raises(L.DimxError):
            E.op_append_attn(rows, kc, kc, n0, SCALE)
    torch.cuda.synchronize()
    assert bool((kc == SENTINEL).all())


# ---------------------------------------------------------------- the session
class _Clip:
    """the 40-frame clip, its oracle encoder rows and context, the checker's runs and the whole-clip runs: computed once"""

    def __init__(self, sd):
        import prompt_ref
        from oracle import ref_cpu
        self.sd = sd
        self.v_s, self.v_a, self.z, self.mask = _case(B, T, [T] * B)
        self.noise48 = _noise(B, TMAX)
        self.noise40 = _noise(B, T)
        assert torch.equal(self.noise48[:T - 1], self.noise40)
        self.x_s = ref_cpu.slmft_forward_encoder(sd, self.v_s, self.mask)
        self.ctx = prompt_ref.case_context(sd, self.v_s, self.v_a, self.mask)
        self.m8 = self.mask.to(torch.uint8).cuda()
        self.start = self.z[:, 0].to(torch.int32).cuda()
        self.vs_d, self.va_d = self.v_s.cuda(), self.v_a.cuda()
        self._ref, self._whole = {}, {}

    def checker(self, L, noisy):
        import online_ref
        if (L, noisy) not in self._ref:
            self._ref[(L, noisy)] = online_ref.online_generate(self.sd, self.z[:, :1], None, T - 1, self.ctx, self.mask, L,
                                                               self.noise40 if noisy else None)
        return self._ref[(L, noisy)]

    def whole(self, eng, key, L, noisy):
        if (key, L, noisy) not in self._whole:
            eng.encode_ctx(self.vs_d, self.va_d, self.m8, True)
            tok, lg = eng.generate(self.start, self.m8, T, 1.0 if noisy else 0.0, 52, self.noise40.cuda() if noisy else None,
                                   return_logits=True, lookahead=L)
            self._whole[(key, L, noisy)] = (tok.cpu().long(), lg.cpu())
        return self._whole[(key, L, noisy)]


def _open(eng, c, L, noisy):
    return eng.stream(B, TMAX, c.start, lookahead=L, temperature=1.0 if noisy else 0.0, top_k=52,
                      noise=c.noise48.cuda() if noisy else None)


def _feed(s, c, chunking, vs=None, va=None, want_x_s=False):
    """push the clip by `chunking`, end; checks the schedule on the way -> tokens [B, 39], logits, per-push new-token counts[, x_s]"""
    from dimx import stream
    vs = c.vs_d if vs is None else vs
    va = c.va_d if va is None else va
    n, done, xs, counts = 0, 0, [], []
    for ch in chunking:
        out = s.push(vs[:, n:n + ch], va[:, n:n + ch], return_logits=True, return_x_s=want_x_s)
        n += ch
        due = stream.steps_due(n, s.lookahead)
        counts.append(out[0].shape[1])
        assert s.steps == due and s.frames == n and s.state() == (n, due, True)          # 6: the schedule
        assert out[0].shape == (B, due - done) and out[1].shape == (B, due - done, 512)
        done = due
        if want_x_s:
            xs.append(out[2])
    tail = s.end(return_logits=True)
    counts.append(tail[0].shape[1])
    assert sum(counts) == s.steps == n - 1 and not s.is_open and s.state() == (0, 0, False)
    tok, lg = s.tokens.cpu().long(), s._lg[:, :s.steps].cpu()
    return (tok, lg, counts) + ((torch.cat(xs, 1).cpu(),) if want_x_s else ())


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


# ---- 3
def test_encoder_rows_match_the_oracle_under_every_chunking(eng, clip):
    rows = []
    for chunking in CHUNKINGS:
        with _open(eng, clip, 0, False) as s:
            x_s = _feed(s, clip, chunking, want_x_s=True)[3]
        err = (x_s - clip.x_s).abs().max().item()
        rows.append(x_s)
        print("chunking %s: max |x_s - oracle| %.3g" % (_cid(chunking), err))
        assert x_s.shape == clip.x_s.shape and err < 1e-4, chunking
    between = max((a - rows[0]).abs().max().item() for a in rows[1:])
    print("largest difference between two chunkings' encoder rows: %.3g" % between)
    assert between < 2e-4      # two sets of rows that are each within 1e-4 of the oracle


# ---- 4, 6
@pytest.mark.parametrize("chunking", CHECKED, ids=_cid)
@pytest.mark.parametrize("noisy", [False, True])
@pytest.mark.parametrize("L", LOOKAHEADS)
def test_session_matches_the_checker(eng, clip, L, noisy, chunking):
    from dimx import stream
    with _open(eng, clip, L, noisy) as s:
        tok, lg, counts = _feed(s, clip, chunking)
    sched = stream.schedule(chunking, L)
    assert counts == [hi - lo for _, lo, hi in sched] and sum(counts) == T - 1
    assert tok.shape == (B, T - 1)
    left_out = _against_checker("session L=%d noisy=%d %s" % (L, noisy, _cid(chunking)), tok, lg, clip.checker(L, noisy))
    assert left_out == 0.0     # none of these cases has a checker margin below MIN_MARGIN


# ---- 5
@pytest.mark.parametrize("noisy", [False, True])
@pytest.mark.parametrize("L", LOOKAHEADS)
def test_session_matches_the_whole_clip_call(eng, clip, L, noisy):
    w_tok, w_lg = clip.whole(eng, "f32", L, noisy)
    for chunking in ([17, 1, 22], [7] * 5 + [5]):
        with _open(eng, clip, L, noisy) as s:
            tok, lg, _ = _feed(s, clip, chunking)
        _against_checker("session against generate(lookahead=%d) noisy=%d %s" % (L, noisy, _cid(chunking)), tok, lg,
                         (w_tok, w_lg, clip.checker(L, noisy)[2]))


def test_bf16_session_against_the_whole_clip_call(full_sd, clip):
    e = _engine(full_sd, "bf16")
    worst = 0.0
    for L in (0, 6):
        w_tok, w_lg = clip.whole(e, "bf16", L, True)
        with _open(e, clip, L, True) as s:
            tok, lg, _ = _feed(s, clip, [17, 1, 22])
        assert torch.isfinite(lg).all() and tok.shape == w_tok.shape
        same = (tok == w_tok).long().cummin(1).values.sum(1)      # steps before a row's first differing token
        d = max((lg[r, :int(n) + 1] - w_lg[r, :int(n) + 1]).abs().max().item() for r, n in enumerate(same.clamp(max=T - 2)))
        print("bf16 L=%d: largest |logits - generate()| over the common history %.3g, common steps per row %s" % (L, d, same.tolist()))
        worst = max(worst, d)
    print("bf16 session against the whole-clip call: largest logit difference %.3g (a report, no token claim)" % worst)
    e.close()


# ---- 7
@pytest.mark.parametrize("chunking", [[1] * 40, [17, 1, 22]], ids=_cid)
@pytest.mark.parametrize("L", [0, -3])
def test_tokens_do_not_depend_on_frames_not_yet_pushed(eng, clip, L, chunking):
    from dimx import stream
    k = 17
    vs2, va2 = clip.vs_d.clone(), clip.va_d.clone()
    vs2[:, k:] += 0.5
    va2[:, k:] -= 0.5
    with _open(eng, clip, L, False) as s:
        tok, lg, _ = _feed(s, clip, chunking)
    with _open(eng, clip, L, False) as s:
        tok2, lg2, _ = _feed(s, clip, chunking, vs2, va2)
    before = stream.steps_due(k, L)      # the steps that had run when frames 0 .. k-1 were all there was
    assert before > 0
    assert torch.equal(tok[:, :before], tok2[:, :before]) and torch.equal(lg[:, :before], lg2[:, :before])
    assert not torch.equal(lg[:, before:], lg2[:, before:])


# ---- 8, 9
def test_workspace_contents_and_repeats_do_not_matter(eng, clip):
    chunking = [7] * 5 + [5]
    runs = []
    s = _open(eng, clip, 2, True)
    s.close()
    for fill in (0x00, 0xFF, None, None):
        if fill is not None:
            s._ws.fill_(fill)
        s.begin(clip.start, 1.0, 52, clip.noise48.cuda(), 0)     # a begin after an end (or an abort) starts clean
        runs.append(_feed(s, clip, chunking, want_x_s=True))
    for tok, lg, _, x_s in runs:
        assert torch.isfinite(lg).all() and torch.isfinite(x_s).all()
        assert torch.equal(tok, runs[0][0]) and torch.equal(lg, runs[0][1]) and torch.equal(x_s, runs[0][3])
    with _open(eng, clip, 2, True) as other:       # another session object, another workspace
        tok, lg, _, x_s = _feed(other, clip, chunking, want_x_s=True)
    assert torch.equal(tok, runs[0][0]) and torch.equal(lg, runs[0][1]) and torch.equal(x_s, runs[0][3])


# ---- 10
def test_motion_is_the_vq_decode_of_the_slice(eng, clip):
    with _open(eng, clip, 0, False) as s:
        n = 0
        for ch in (16, 5, 1):
            new = s.push(clip.vs_d[:, n:n + ch], clip.va_d[:, n:n + ch])
            n += ch
            hi, k = s.steps, new.shape[1]
            for W in (None, 8):
                lo = 0 if W is None else min(max(hi - W, 0), hi - k)
                want = eng.vq_decode(1, s.tokens[:, lo:hi].contiguous())[:, hi - lo - k:]
                got = s.motion(W)
                assert got.shape == (B, k, 56) and torch.equal(got, want), (n, W)
        windowed, whole = s.motion(8, all_rows=True), s.motion(None, all_rows=True)
        assert windowed.shape == (B, 8, 56) and not torch.equal(windowed, whole[:, -8:])     # another function of the tokens
        s.push(clip.vs_d[:, n:], clip.va_d[:, n:])
        tail = s.end()
        assert tail.shape == (B, 0) and s.motion(None).shape == (B, 0, 56)
        assert torch.equal(s.motion(None, all_rows=True), eng.vq_decode(1, s.tokens.contiguous()))
    with _open(eng, clip, 40, False) as s:      # nothing is due before the end: its tokens are the whole sequence
        assert s.push(clip.vs_d, clip.va_d).shape == (B, 0) and s.motion().shape == (B, 0, 56)
        tok = s.end()
        assert tok.shape == (B, T - 1) and torch.equal(s.motion(None), eng.vq_decode(1, tok.contiguous()))


def test_model_session_is_forward_val_with_a_lookahead():
    from dimx.seq2seq_pretrain import SLMFT
    from test_gpu_prompt import _clips
    model = SLMFT().eval()
    v_s, v_l, v_a, mask = [t.cuda() for t in _clips(B, T, [T] * B)]
    for L in (0, 6):
        _, _, pred, tok = model(v_s, v_l, v_a, mask, mode="val", greedy=True, lookahead=L, return_tokens=True)
        _, z_l = model.forward_vq(v_s, v_l, mask, with_speaker=False)
        with model.stream(B, TMAX, z_l[:, 0], lookahead=L, greedy=True) as s:
            n = 0
            for ch in (7, 16, 17):
                s.push(v_s[:, n:n + ch], v_a[:, n:n + ch])
                n += ch
            s.end()
            agree = (s.tokens.long() == tok).long().cummin(1).values.sum(1)
            print("model session L=%d: steps before a row's first token that differs from forward(): %s of %d" % (L, agree.tolist(), T - 1))
            assert s.tokens.shape == tok.shape
            if bool((agree == T - 1).all()):
                assert torch.equal(s.motion(None, all_rows=True), model.forward_vq_decoder(tok, "val"))
            assert torch.equal(s.motion(None, all_rows=True), model.forward_vq_decoder(s.tokens.long(), "val"))


# ---- 11
def test_state_machine_and_refusals(eng, clip):
    from dimx import engine, lib as L
    lib, h = eng.lib, eng.h
    # an offline generation before any session
    eng.encode_ctx(clip.vs_d, clip.va_d, clip.m8, True)
    before = eng.generate(clip.start, clip.m8, T, 1.0, 52, clip.noise40.cuda(), return_logits=True)
    tokens = torch.full((B, TMAX - 1), -7, dtype=torch.int32, device="cuda")
    n_new = ctypes.c_int(5)

    def push(vs, va, c):
        return lib.dimx_stream_push(h, L.ptr(vs), L.ptr(va), c, L.ptr(tokens), TMAX - 1, None, None, ctypes.byref(n_new), eng._s())

    vs16, va16 = clip.vs_d[:, :16].contiguous(), clip.va_d[:, :16].contiguous()
    # before begin
    assert push(vs16, va16, 16) == ERR_STATE and n_new.value == 0
    assert lib.dimx_stream_end(h, L.ptr(tokens), TMAX - 1, None, ctypes.byref(n_new), eng._s()) == ERR_STATE
    assert lib.dimx_stream_abort(h) == 0
    # shapes begin refuses
    assert lib.dimx_stream_workspace_bytes(h, B, 2049) == 0 and lib.dimx_stream_workspace_bytes(h, B, 1) == 0
    with pytest.raises(L.DimxError):
        eng.stream(B, 2049, clip.start)
    s = _open(eng, clip, 0, False)
    ws, wsb = s._ws_ptr()
    assert lib.dimx_stream_begin(h, L.ptr(clip.start), B, 2049, 0, 0.0, 52, None, 0, ws, wsb, eng._s()) == ERR_STATE   # open: state first
    s.close()
    assert lib.dimx_stream_begin(h, L.ptr(clip.start), B, 2049, 0, 0.0, 52, None, 0, ws, wsb, eng._s()) == ERR_ARG
    assert lib.dimx_stream_begin(h, L.ptr(clip.start), B, TMAX, 0, 0.0, 52, None, 0, ws, 4096, eng._s()) == ERR_WORKSPACE
    assert lib.dimx_stream_begin(h, None, B, TMAX, 0, 0.0, 52, None, 0, ws, wsb, eng._s()) == ERR_ARG
    assert s.state() == (0, 0, False)
    for variant in ("slm", "legacy"):
        other = engine.Engine("cuda:0", L.MODE_PARITY_F32, variant=variant)
        assert other.lib.dimx_stream_workspace_bytes(other.h, B, TMAX) == 0
        rc = other.lib.dimx_stream_begin(other.h, L.ptr(clip.start), B, TMAX, 0, 0.0, 52, None, 0, ws, wsb, other._s())
        assert rc == ERR_ARG and b"variant" in other.lib.dimx_last_error()
        assert other.lib.dimx_stream_push(other.h, L.ptr(vs16), L.ptr(va16), 16, L.ptr(tokens), TMAX - 1, None, None, ctypes.byref(n_new),
                                          other._s()) == ERR_STATE
        other.close()
    # an open session
    s.begin(clip.start, 0.0, 52, None, 0)
    with pytest.raises(L.DimxError):
        eng.stream(B, TMAX, clip.start)                       # one session per handle
    with pytest.raises(L.DimxError):
        s.begin(clip.start)
    assert push(vs16, va16, 0) == ERR_ARG and push(vs16, va16, -1) == ERR_ARG
    assert push(None, va16, 16) == ERR_ARG
    assert lib.dimx_stream_end(h, L.ptr(tokens), TMAX - 1, None, ctypes.byref(n_new), eng._s()) == ERR_ARG     # fewer than 2 frames
    assert s.state() == (0, 0, True)
    # the stages that rebuild the context or generate are blocked ...
    for call in (lambda: eng.encode_ctx(clip.vs_d, clip.va_d, clip.m8, True),
                 lambda: eng.set_context(clip.x_s.cuda(), clip.va_d, which_patch=0, for_generate=True),
                 lambda: eng.generate(clip.start, clip.m8, T, 0.0),
                 lambda: eng.generate(None, clip.m8, T, 0.0, prompt=clip.z[:, :3].cuda()),
                 lambda: eng.generate_beam(clip.start, clip.m8, T, 2),
                 lambda: eng.decode_tf(clip.z.cuda(), clip.m8),
                 lambda: eng.set_cross_lookahead(0)):
        with pytest.raises(L.DimxError) as ei:
            call()
        assert "(%d)" % ERR_STATE in str(ei.value) and "session" in str(ei.value)
    # ... the VQ stages and the unit ops are not
    assert torch.isfinite(eng.vq_decode(1, clip.z[:, :8].cuda())).all()
    kc = torch.zeros(AB, AH, ATMAX, 64, device="cuda")
    assert torch.isfinite(engine.op_append_attn(torch.ones(AB, 2, 3 * AH * 64, device="cuda"), kc, kc.clone(), 0, SCALE)).all()
    torch.cuda.synchronize()
    assert bool((tokens == -7).all()), "a refused call launched something"
    # past Tmax
    s.push(clip.vs_d, clip.va_d)
    assert s.state() == (T, T - 1, True)
    assert push(vs16, va16, 16) == ERR_ARG and b"Tmax" in lib.dimx_last_error() and s.state() == (T, T - 1, True)
    s.end()
    assert push(vs16, va16, 16) == ERR_STATE                  # after end
    torch.cuda.synchronize()
    assert bool((tokens == -7).all())
    # the blocked stages work again, and an offline generation is what it was
    eng.encode_ctx(clip.vs_d, clip.va_d, clip.m8, True)
    after = eng.generate(clip.start, clip.m8, T, 1.0, 52, clip.noise40.cuda(), return_logits=True)
    assert torch.equal(after[0], before[0]) and torch.equal(after[1], before[1])
    assert eng.cross_lookahead() is None
    s.begin(clip.start, 0.0, 52, None, 0)
    s.close()                                                  # abort
    eng.encode_ctx(clip.vs_d, clip.va_d, clip.m8, True)
    again = eng.generate(clip.start, clip.m8, T, 1.0, 52, clip.noise40.cuda(), return_logits=True)
    assert torch.equal(again[0], before[0]) and torch.equal(again[1], before[1])
