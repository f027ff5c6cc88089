"""GPU: FP8 cross K/V for best-of-N generation (dimx_set_cross_kv8_samples; the definition is dimx/kv8.py attention_rows) -- the
multi-query cross attention over codes on the matrix cores (csrc/decode_attn_kv8.hip, decode_attn_mq_kv8_kernel) in its exact and
matrix-core forms against the definition, its windowed form, slice invariance and misuse, and the best-of-4 generation against the CPU
checker of tests/self_kv8_ref.py run on the device buffer's own dequantised rows."""
import functools
import zlib

import numpy as np
import pytest
import torch

from test_gpu_decode_step import masks, q_operand, tolerance
from test_gpu_prompt import STEP_TOL, _case
from test_kv8_host import KV8_CASE, MARGIN, MAX_LEFT_OUT
from test_kv8_samples_host import SAMPLES, SAMPLES_SEED, sample_noise

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
SCALE = 0.125
ERR_ARG = -1
B_OP, H_OP, TMAX_OP = 5, 3, 136      # five clips: masks() yields its five mask kinds; 15 pairs: the last block has an idle wave
N_KEYS = (1, 7, 16, 17, 63, 64, 65, 128, 129, 136)
ROWS = (2, 4, 5, 8, 10)
O_PAD, GUARD = 8, 2                  # extra columns of out and guard rows behind row B * S, all holding the sentinel
SENTINEL = -7.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t.contiguous().view(torch.int16)


@functools.lru_cache(maxsize=None)
def _codes(n):
    """codes / scales of unit-normal K / V rows over Tmax + 1 rows (rows at and past n are valid data: the shifted references read
    row n, also at n = Tmax) and the poisoned copies [.., Tmax, ..] the kernel gets; shared by every S, q form and output type"""
    from dimx import kv8
    g = torch.Generator().manual_seed(zlib.crc32(("kv8 samples codes %d" % n).encode()))
    kc, ks = kv8.quantize(torch.randn(B_OP, H_OP, TMAX_OP + 1, 64, generator=g).numpy())
    vc, vs = kv8.quantize(torch.randn(B_OP, H_OP, TMAX_OP + 1, 64, generator=g).numpy())
    pk, pks, pv, pvs = (torch.from_numpy(a[:, :, :TMAX_OP].copy()) for a in (kc, ks, vc, vs))
    pk[:, :, n:] = 0x7F
    pv[:, :, n:] = 0x7F
    pks[:, :, n:] = float("nan")
    pvs[:, :, n:] = float("nan")
    m = masks(B_OP, n, n + 7, g)
    return (kc, ks, vc, vs), (pk, pks, pv, pvs), m


@functools.lru_cache(maxsize=None)
def _op_case(S, qform, n, masked, rounded):
    """q, the float64 reference (at round_bf16(q) when ``rounded``), the absolute mass and the wrong alternatives; computed once"""
    from dimx import kv8
    B, H = B_OP, H_OP
    (kc, ks, vc, vs), _, m = _codes(n)
    g = torch.Generator().manual_seed(zlib.crc32(("kv8 samples q %d %s %d %d" % (S, qform, n, masked)).encode()))
    q, qeff, _ = q_operand(B * S, H, "cache" if qform == "bf16" else qform, torch.bfloat16 if qform == "bf16" else torch.float32, g)
    qe = kv8.round_bf16(qeff.numpy()) if rounded else qeff.numpy()
    mm = m[:, :n].numpy() if masked else None
    att = lambda q_, kc_, ks_, vc_, vs_, mask_, n_: torch.from_numpy(
        kv8.attention_rows(q_, kc_, ks_, vc_, vs_, mask_, n_, S, SCALE)).reshape(B * S, H * 64)
    ref = att(qe, kc, ks, vc, vs, mm, n)
    mass = torch.from_numpy(kv8.pv_abs(qe, kc, ks, vc, vs, mm, n, S, SCALE)).reshape(B * S, H * 64)
    nxt = lambda a: np.roll(a, -1, axis=0)       # clip b gets clip b + 1's
    perm = np.arange(B * S).reshape(B, S)[:, ::-1].reshape(-1)     # the sample rows of a clip in reverse order
    alts = [("keys shifted by one", att(qe, kc[:, :, 1:], ks[:, :, 1:], vc[:, :, 1:], vs[:, :, 1:], mm, n)),
            ("V scales shifted by one row", att(qe, kc, ks, vc, vs[:, :, 1:], mm, n)),
            ("clip b's rows over clip b + 1's codes", att(qe, nxt(kc), nxt(ks), nxt(vc), nxt(vs), mm, n))]
    if n > 1:    # with one key the softmax is 1 whatever the query and the K scale: these three ARE the right answer at n = 1
        alts.append(("sample rows permuted within a clip", ref[perm]))
        alts.append(("one key dropped", att(qe, kc, ks, vc, vs, mm[:, :n - 1] if masked else None, n - 1)))
        alts.append(("K scales shifted by one row", att(qe, kc, ks[:, :, 1:], vc, vs, mm, n)))
    mean_v = torch.from_numpy(kv8.dequantize(vc, vs)[:, :, :n].astype(np.float64).mean(2)).reshape(B, H * 64)
    return {"q": q, "mask": m, "ref": ref, "mass": mass, "alts": alts, "mean_v": mean_v}


def _out(dev, S, bf):
    return torch.full((B_OP * S + GUARD, H_OP * 64 + O_PAD), SENTINEL, dtype=torch.bfloat16 if bf else torch.float32, device=dev)


def _check(out, S, ref, bound, alts, what):
    rows, cols = B_OP * S, H_OP * 64
    assert bool((out[rows:] == SENTINEL).all()) and bool((out[:, cols:] == SENTINEL).all()), "%s: a sentinel was overwritten" % what
    got = out[:rows, :cols].double().cpu()
    assert torch.isfinite(got).all(), what
    err = (got - ref).abs()
    over = err > bound
    assert not over.any(), "%s: %d elements outside the bound, worst %.3g (bound %.3g there)" % (
        what, int(over.sum()), (err - bound).max().item(), bound.flatten()[(err - bound).argmax()].item())
    for name, alt in alts:
        assert ((alt - ref).abs() > bound).any(), "%s: the bound cannot tell %s from the right answer" % (what, name)
    return (err / bound).max().item(), got


@pytest.mark.parametrize("out", ["f32", "bf16"])
@pytest.mark.parametrize("form,qform", [("exact", "slab1"), ("exact", "slab3"), ("mfma", "slab1"), ("mfma", "slab3"), ("mfma", "bf16")])
def test_multi_query_attention_over_codes_against_the_definition(dev, form, qform, out):
    """exact form: within tolerance(ref, bf16_out) of kv8.attention_rows.  Matrix-core form: the reference is taken at round_bf16(q)
    and the bound is 2**-8 * pv_abs + tolerance(ref, bf16_out) -- the P operand's unit roundoff times the absolute mass, plus the
    step kernels' f32 / output-ulp term (derived, not measured)."""
    from dimx import engine as E
    bf, exact = out == "bf16", form == "exact"
    worst = 0.0
    for n in N_KEYS:
        _, poisoned, _ = _codes(n)
        clean, _, _ = _codes(n)
        pk = tuple(t.to(dev) for t in poisoned)
        ck = tuple(torch.from_numpy(a[:, :, :TMAX_OP].copy()).to(dev) for a in clean)
        for S in ROWS:
            for masked in (False, True):
                c = _op_case(S, qform, n, masked, not exact)
                what = "%s %s S=%d n=%d masked=%d" % (form, qform, S, n, masked)
                q = c["q"].to(dev)
                m = c["mask"].to(dev) if masked else None
                o = E.op_decode_attn_kv8_multi(q, *pk, SCALE, n, S, kmask=m, exact=exact, out=_out(dev, S, bf))
                bound = tolerance(c["ref"], bf) + (0 if exact else 2.0 ** -8 * c["mass"])
                rel, got = _check(o, S, c["ref"], bound, c["alts"], what)
                worst = max(worst, rel)
                # codes 0x7F and NaN scales past n_keys were never read: the clean operands give the same bits, and so does a repeat
                for ops in (ck, pk):
                    again = E.op_decode_attn_kv8_multi(q, *ops, SCALE, n, S, kmask=m, exact=exact, out=_out(dev, S, bf))
                    assert torch.equal(_bits(again), _bits(o)), "%s: rows past n_keys were read, or a repeat differs" % what
                if masked:   # the all-masked clip's rows are the mean of the dequantised V over the n keys
                    mv = c["mean_v"][3]
                    assert ((got[3 * S:4 * S] - mv[None]).abs() <= bound[3 * S:4 * S]).all(), what
    print("kv8 multi-query %s %s out %s: worst |err| / bound %.3f" % (form, qform, out, worst))


@pytest.mark.parametrize("form", ["exact", "mfma"])
@pytest.mark.parametrize("out", ["f32", "bf16"])
def test_windowed_form_is_the_plain_form_at_the_bound(dev, out, form):
    from dimx import engine as E
    from dimx.online import visible
    bf, exact, n, S = out == "bf16", form == "exact", 136, 5
    (kc, ks, vc, vs), _, _ = _codes(n)
    kc, ks, vc, vs = (torch.from_numpy(a[:, :, :TMAX_OP].copy()) for a in (kc, ks, vc, vs))
    c = _op_case(S, "slab3", n, True, False)
    m = torch.ones(B_OP, n + 7, dtype=torch.uint8)
    m[0, [0, 3, 14, 15, 16, 31, 32, 33, 62, 63, 64, 100]] = 0
    m[1, 40:] = 0
    m[2, :] = 0
    q, md = c["q"].to(dev), m.to(dev)
    seen = set()
    for L in (0, -3, 5):
        for t in [-1 - L, 13 - L, 14 - L, 15 - L, 29 - L, 30 - L, 31 - L, 61 - L, 62 - L, 63 - L, 500]:
            vis = visible(t, L, n)
            seen.add(vis)
            step = torch.tensor([t], dtype=torch.int32, device=dev)
            pk, pks, pv, pvs = kc.clone(), ks.clone(), vc.clone(), vs.clone()
            pk[:, :, vis:] = 0x7F
            pv[:, :, vis:] = 0x7F
            pks[:, :, vis:] = float("nan")
            pvs[:, :, vis:] = float("nan")
            plain = E.op_decode_attn_kv8_multi(q, kc.to(dev), ks.to(dev), vc.to(dev), vs.to(dev), SCALE, vis, S, kmask=md, exact=exact, out_bf16=bf)
            win = E.op_decode_attn_kv8_multi(q, pk.to(dev), pks.to(dev), pv.to(dev), pvs.to(dev), SCALE, n, S, kmask=md, exact=exact, out_bf16=bf,
                                             step=step, lookahead=L)
            assert bool(torch.isfinite(win.float()).all()), (t, L)
            assert torch.equal(_bits(win), _bits(plain)), "step %d lookahead %d: vis %d" % (t, L, vis)
    assert seen == {1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 136}


@pytest.mark.parametrize("form", ["exact", "mfma"])
def test_slice_of_clips_reproduces_the_whole_batch(dev, form):
    """one wave per (clip, head) whatever the batch: the rows of a 2-clip slice have the bits of the 5-clip batch"""
    from dimx import engine as E
    n, S, exact = 129, 4, form == "exact"
    (kc, ks, vc, vs), _, m = _codes(n)
    kc, ks, vc, vs = (torch.from_numpy(a[:, :, :TMAX_OP].copy()).to(dev) for a in (kc, ks, vc, vs))
    q = _op_case(S, "slab3", n, True, False)["q"].to(dev)
    m = m.to(dev)
    whole = E.op_decode_attn_kv8_multi(q, kc, ks, vc, vs, SCALE, n, S, kmask=m, exact=exact)
    for lo, hi in ((0, 2), (3, 5)):
        part = E.op_decode_attn_kv8_multi(q[:, lo * S:hi * S].contiguous(), kc[lo:hi].contiguous(), ks[lo:hi].contiguous(), vc[lo:hi].contiguous(),
                                          vs[lo:hi].contiguous(), SCALE, n, S, kmask=m[lo:hi].contiguous(), exact=exact)
        assert torch.equal(_bits(part), _bits(whole[lo * S:hi * S])), "clips %d..%d" % (lo, hi - 1)


def test_operator_rejects_misuse_before_the_launch(dev):
    from dimx import lib as L
    l = L.load()
    B, H, Tmax, S = 2, 3, 2056, 4
    kc = torch.zeros(B, H, Tmax, 64, dtype=torch.uint8, device=dev)
    ks = torch.ones(B * H * Tmax + 4, device=dev)
    q = torch.zeros(B * S * H * 64 + 8, device=dev)
    out = torch.full((B * S * H * 64 + 8,), SENTINEL, device=dev)
    km = torch.ones(B, Tmax, dtype=torch.uint8, device=dev)
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    good = dict(q=q.data_ptr(), q_ld=H * 64, nslab=1, kc=kc.data_ptr(), ks=ks.data_ptr(), vc=kc.data_ptr(), vs=ks.data_ptr(), out=out.data_ptr(),
                o_ld=H * 64, Tmax=Tmax, step=None, n=100, km=km.data_ptr(), kld=Tmax, rpc=S, la=0, win=0, q_f32=1, dt=L.F32, exact=0)

    def call(**kw):
        a = dict(good, **kw)
        return l.dimx_op_decode_attn_kv8_multi(a["dt"], a["q"], a["q_ld"], a["q_f32"], a["nslab"], B * S * a["q_ld"], a["kc"], a["ks"], a["vc"], a["vs"],
                                               a["out"], a["o_ld"], B, H, a["Tmax"], a["step"], a["n"], a["km"], a["kld"], a["rpc"], SCALE, 0, a["la"],
                                               a["win"], a["exact"], L.stream_ptr(dev))
    bad = [dict(q=None), dict(kc=None), dict(ks=None), dict(vc=None), dict(vs=None), dict(out=None),
           dict(q=q.data_ptr() + 4), dict(kc=kc.data_ptr() + 8), dict(vc=kc.data_ptr() + 4), dict(out=out.data_ptr() + 4), dict(ks=ks.data_ptr() + 2),
           dict(vs=ks.data_ptr() + 1), dict(q_ld=H * 64 + 2), dict(o_ld=H * 64 + 2), dict(o_ld=H * 64 + 4, dt=L.BF16), dict(q_ld=H * 64 + 4, q_f32=0),
           dict(n=0), dict(n=-1), dict(n=Tmax + 1), dict(n=2049), dict(n=100, Tmax=99), dict(kld=99),
           dict(win=1), dict(rpc=0), dict(rpc=1), dict(rpc=3), dict(rpc=6), dict(rpc=16), dict(nslab=0), dict(nslab=9), dict(nslab=2, q_f32=0), dict(dt=7)]
    for exact in (0, 1):
        for kw in bad:
            assert call(exact=exact, **kw) == ERR_ARG, kw
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()), "a refused call launched something"
    for exact in (0, 1):
        out.fill_(SENTINEL)
        assert call(exact=exact) == 0 and call(exact=exact, win=1, step=step.data_ptr(), la=3) == 0 and call(exact=exact, n=2048) == 0
        torch.cuda.synchronize()
        assert bool((out[:B * S * H * 64] != SENTINEL).all()) and bool((out[B * S * H * 64:] == SENTINEL).all())


# ---------------------------------------------------------------- the generation
class _Gen:
    """the inputs of KV8_CASE under the seed tests/test_kv8_samples_host.py chose, built once and left unchanged"""

    def __init__(self, sd):
        import prompt_ref
        self.sd = sd
        self.B, self.T, self.lens = KV8_CASE
        self.n = self.T - 1
        self.S = SAMPLES
        self.v_s, self.v_a, self.z, self.mask = _case(self.B, self.T, list(self.lens), seed=SAMPLES_SEED)
        self.noise = sample_noise(self.B, self.T, SAMPLES)
        self.m8 = self.mask.to(torch.uint8).cuda()
        self.z0 = self.z.clamp(min=0)
        self.ctx = prompt_ref.case_context(sd, self.v_s, self.v_a, self.mask)

    def context(self, eng, **kw):
        eng.encode_ctx(self.v_s.cuda(), self.v_a.cuda(), self.m8, True, n_samples=self.S, **kw)

    def cross_rows(self, eng):
        import kv8_ref
        return kv8_ref.dequantized(eng.cross_kv8_layers(self.B, self.T), self.T)

    def self_rows(self, eng, table0=False):
        import self_kv8_ref
        rows = self_kv8_ref.dequantized(eng.self_kv8_layers(self.B * self.S, self.T), self.n)
        return [None] + rows[1:] if table0 else rows

    def check(self, cross, Pmax, lookahead=None, noise=None, follow=None, self_rows=None):
        import self_kv8_ref
        return self_kv8_ref.self_kv8_generate(self.sd, self.z0[:, :Pmax], None, self.n, self.ctx, self.mask, lookahead,
                                              self_kv8_ref.SelfRows(given=self_rows), noise, cross_kv=cross, follow=follow, samples=self.S)

    def forced(self, eng, L=None, **kw):
        """the whole clip as a forced prompt (no token can diverge), S rows per clip"""
        prompt = self.z0[:, :self.n].to(torch.int32).cuda().contiguous()
        self.context(eng)
        tok, lg = eng.generate(None, self.m8, self.T, 0.0, 52, None, return_logits=True, n_samples=self.S, prompt=prompt, no_prefill=True,
                               lookahead=L, **kw)
        return tok.cpu().long(), lg.cpu()

    def free(self, eng, noisy, **kw):
        self.context(eng)
        tok, lg = eng.generate(self.z0[:, 0].cuda(), self.m8, self.T, 1.0 if noisy else 0.0, 52, self.noise.cuda() if noisy else None,
                               return_logits=True, n_samples=self.S, **kw)
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
def gen(full_sd):
    return _Gen(full_sd)


@pytest.mark.parametrize("L", [None, 0])
def test_teacher_forced_logits_match_the_checker_on_the_buffers_rows(eng, gen, L):
    """f32 engine (the exact form): every step's logits of every sample row against the checker on the buffer's dequantised K/V"""
    tok, lg = gen.forced(eng, L, kv8_samples=True)
    assert not eng.cross_kv8_samples() and eng.cross_kv8() is None        # generate(kv8_samples=True) cleared both settings
    ref_lg = gen.check(gen.cross_rows(eng), gen.n, L)[1]
    assert tuple(lg.shape) == (gen.B * gen.S, gen.n, 512)
    assert torch.equal(tok[:, :gen.n - 1], gen.z0[:, 1:gen.n].repeat_interleave(gen.S, 0))
    err = (lg - ref_lg).abs().amax(-1)
    for s in range(gen.S):
        print("teacher-forced kv8_samples, lookahead %s, sample %d: max |logits - checker| %.3e (STEP_TOL %.0e)" % (L, s, err[s::gen.S].max().item(), STEP_TOL))
        assert err[s::gen.S].max().item() < STEP_TOL
    # the plain best-of-4 along the same tokens is further away than that: the codes are what was read
    _, plain = gen.forced(eng, L)
    assert (plain - ref_lg).abs().max().item() > STEP_TOL


@pytest.mark.parametrize("noisy", [False, True])
def test_free_running_tokens_match_the_checker(eng, gen, noisy):
    tok, lg = gen.free(eng, noisy, kv8_samples=True)
    assert tuple(tok.shape) == (gen.B * gen.S, gen.n)
    ref_tok, ref_lg, margins = gen.check(gen.cross_rows(eng), 1, None, gen.noise if noisy else None, follow=tok)
    keep = margins >= MARGIN
    left_out = 1.0 - keep.float().mean().item()
    err = (lg - ref_lg).abs().amax(-1)
    wrong = int(((tok != ref_tok) & keep).sum())
    print("free-running kv8_samples noisy=%d: %d compared tokens differ, max |logits - checker| %.3e, smallest margin %.3e, pairs left out %.4f"
          % (noisy, wrong, err.max().item(), margins.min().item(), left_out))
    assert left_out <= MAX_LEFT_OUT
    assert wrong == 0
    assert err.max().item() < STEP_TOL
    if noisy:
        assert not torch.equal(tok[0], tok[1])


def test_with_self_kv8_on_top(eng, gen):
    t0 = eng.lib.dimx_kv0_table_generations(eng.h)
    tok, lg = gen.free(eng, True, kv8_samples=True, self_kv8=True)
    table0 = eng.lib.dimx_kv0_table_generations(eng.h) > t0
    assert eng.self_kv8() is None and eng.cross_kv8() is None and not eng.cross_kv8_samples()
    cross = gen.cross_rows(eng)
    ref_tok, ref_lg, margins = gen.check(cross, 1, None, gen.noise, follow=tok, self_rows=gen.self_rows(eng, table0))
    err = (lg - ref_lg).abs().amax(-1)
    wrong = int(((tok != ref_tok) & (margins >= MARGIN)).sum())
    print("kv8_samples + self_kv8: %d compared tokens differ, max |logits - checker| %.3e" % (wrong, err.max().item()))
    assert wrong == 0 and err.max().item() < STEP_TOL
    only_cross = gen.check(cross, 1, None, gen.noise, follow=tok)[1]
    assert (lg - only_cross).abs().max().item() > STEP_TOL      # the self codes were read as well


def test_prefilled_prompt_and_lookahead_zero(eng, gen):
    P0 = 20
    prompt = gen.z0[:, :P0].to(torch.int32).cuda().contiguous()
    gen.context(eng, prompt_frames=P0)
    tok, lg = eng.generate(None, gen.m8, gen.T, 0.0, 52, None, return_logits=True, n_samples=gen.S, prompt=prompt, kv8_samples=True)
    tok, lg = tok.cpu().long(), lg.cpu()
    # the prefill reads the unquantised caches: the self rows of the positions 0 .. P0 - 2 are those of a plain teacher-forced pass
    # (the checker over its own projected cross K / V), the steps from P0 - 1 on read the codes
    import self_kv8_ref
    plain = self_kv8_ref.SelfRows()
    self_kv8_ref.self_kv8_generate(gen.sd, gen.z0[:, :P0], None, P0 - 1, gen.ctx, gen.mask, None, plain, samples=gen.S)
    pre = plain.new_rows()

    class PrefilledRows(self_kv8_ref.SelfRows):
        def rows(self, i, t, k_new, v_new):
            if t < P0 - 1:
                k_new, v_new = pre[i][0][:, :, t:t + 1], pre[i][1][:, :, t:t + 1]
            return super().rows(i, t, k_new, v_new)

    ref_tok, ref_lg, margins = self_kv8_ref.self_kv8_generate(gen.sd, gen.z0[:, :P0], None, gen.n, gen.ctx, gen.mask, None, PrefilledRows(),
                                                              cross_kv=gen.cross_rows(eng), follow=tok, samples=gen.S)
    err = (lg[:, P0 - 1:] - ref_lg[:, P0 - 1:]).abs().amax(-1)
    print("prefilled kv8_samples, P0 = %d: max |logits - checker| %.3e from step %d on" % (P0, err.max().item(), P0 - 1))
    assert err.max().item() < STEP_TOL
    assert not bool(lg[:, :P0 - 1].any())
    assert int(((tok != ref_tok) & (margins >= MARGIN))[:, P0 - 1:].sum()) == 0
    # online, lookahead 0, free-running
    tok, lg = gen.free(eng, True, kv8_samples=True, lookahead=0)
    ref_tok, ref_lg, margins = gen.check(gen.cross_rows(eng), 1, 0, gen.noise, follow=tok)
    err = (lg - ref_lg).abs().amax(-1)
    print("kv8_samples, lookahead 0: max |logits - checker| %.3e" % err.max().item())
    assert err.max().item() < STEP_TOL and int(((tok != ref_tok) & (margins >= MARGIN)).sum()) == 0


def test_off_is_what_it_was_and_replays_equal_a_fresh_handle(full_sd, eng, gen):
    from dimx import lib as L
    before = gen.free(eng, True)
    # with kv8_samples off, n_samples = 4 under a cross buffer is still refused
    gen.context(eng)
    with pytest.raises(L.DimxError, match=r"\(-1\)"):
        eng.generate(gen.z0[:, 0].cuda(), gen.m8, gen.T, 0.0, n_samples=gen.S, kv8=True)
    assert eng.cross_kv8() is None and not eng.cross_kv8_samples()
    # beam search and guidance stay refused with it on
    buf = torch.zeros(eng.cross_kv8_bytes(gen.B, gen.T), dtype=torch.uint8, device="cuda:0")
    eng.set_cross_kv8(buf)
    eng.set_cross_kv8_samples(True)
    assert eng.cross_kv8_samples()
    try:
        with pytest.raises(L.DimxError, match=r"\(-1\)"):
            eng.generate_beam(gen.z0[:, 0].cuda(), gen.m8, gen.T, 2)
    finally:
        eng.set_cross_kv8_samples(False)
        eng.set_cross_kv8(None)
    first = gen.free(eng, True, kv8_samples=True)
    again = gen.free(eng, True, kv8_samples=True)           # the same buffer: the captured graph is replayed
    fresh = _engine(full_sd)
    try:
        f = gen.free(fresh, True, kv8_samples=True)
    finally:
        fresh.close()
    for tok, lg in (again, f):
        assert torch.equal(tok, first[0]) and torch.equal(_bits(lg), _bits(first[1]))
    assert not torch.equal(first[1], before[1])
    after = gen.free(eng, True)
    assert torch.equal(after[0], before[0]) and torch.equal(_bits(after[1]), _bits(before[1]))


BF16_ROUTE_FACTOR = 2.0      # the kv8_samples route may lie twice as far from its S = 1 calls as the plain multi-query route from its own


def test_bf16_engine_matrix_core_route_against_one_query_calls(full_sd, gen):
    """bf16 engine (the matrix-core form), forced along fixed tokens through a full-length prompt: the logits of the S = 4 kv8_samples
    call against four S = 1 kv8=True calls on the same codes (every sample row of a forced clip equals the S = 1 row).  The bound is
    measured on this very case: twice the distance of the plain bf16 best-of-4 route (attention_tr multi-query) from the plain S = 1
    bf16 call, because the two multi-query routes round q and P in different places.  Measured on an MI355X (max |logit difference| over all
    rows and steps): the plain multi-query route lies 7.019e-03 from its S = 1 call, the kv8_samples route 6.285e-03 from the S = 1
    kv8 call; the allowance is 1.404e-02."""
    e = _engine(full_sd, "bf16")
    try:
        P = gen.n
        prompt = gen.z0[:, :P].to(torch.int32).cuda().contiguous()

        def one(**kw):
            e.encode_ctx(gen.v_s.cuda(), gen.v_a.cuda(), gen.m8, True)
            return e.generate(None, gen.m8, gen.T, 0.0, 52, None, return_logits=True, prompt=prompt, no_prefill=True, **kw)[1].cpu()

        plain1, kv1 = one(), one(kv8=True)
        _, plain4 = gen.forced(e)
        _, kv4 = gen.forced(e, kv8_samples=True)
        rep = lambda x: x.repeat_interleave(gen.S, 0)
        d_plain = (plain4 - rep(plain1)).abs().max().item()
        d_kv8 = (kv4 - rep(kv1)).abs().max().item()
        print("bf16 forced best-of-%d: plain multi-query route vs S=1 %.3e; kv8_samples vs S=1 kv8 %.3e (allowed: %.1f x the former)"
              % (gen.S, d_plain, d_kv8, BF16_ROUTE_FACTOR))
        assert bool(torch.isfinite(kv4).all())
        assert d_kv8 <= BF16_ROUTE_FACTOR * d_plain
        assert not torch.equal(kv4, plain4)             # the codes were read
    finally:
        e.close()


def test_module_forward_takes_the_route(full_sd, gen):
    from dimx.seq2seq_pretrain import SLMFT
    from dimx import prng
    model = SLMFT().eval()
    B, T, S = gen.B, gen.T, gen.S
    v_l = torch.from_numpy(prng.normal(SAMPLES_SEED, "kv8_samples.vl", (B, T, 56)))
    args = [t.cuda() for t in (gen.v_s, v_l, gen.v_a, gen.mask)]
    tok = model(*args, mode="val", greedy=True, return_tokens=True, n_samples=S)[3]
    tot, d, pred, tok8 = model(*args, mode="val", greedy=True, return_tokens=True, n_samples=S, kv8_samples=True)
    assert tok8.shape == tok.shape == (B, S, T - 1) and pred.shape == (B, S, T - 1, 56) and bool(torch.isfinite(pred).all())
    eng = model.engine(args[0].device)
    assert not eng.cross_kv8_samples() and eng.cross_kv8() is None and eng.cross_kv8_buffer() is not None
    assert torch.equal(model(*args, mode="val", greedy=True, return_tokens=True, n_samples=S)[3], tok)
    print("SLMFT.forward(kv8_samples=True, n_samples=%d): %.0f %% of the greedy tokens equal the plain call's" % (S, 100 * (tok8 == tok).float().mean().item()))
