"""GPU: FP8 cross-attention K/V (dimx_set_cross_kv8; the definition is dimx/kv8.py) -- the quantiser against the definition bit for
bit, the one-query cross attention over codes (csrc/decode_attn_kv8.hip) against kv8.attention at the step kernels' tolerance, its
windowed form, shard invariance and misuse, and the generation against the CPU checker of tests/kv8_ref.py run on the device
buffer's own dequantised rows."""
import functools
import os
import zlib

import numpy as np
import pytest
import torch

from test_gpu_decode_step import check, masks, q_operand, tolerance   # the step kernels' bound on unit-scale data, as test_gpu_stream.py
from test_gpu_prompt import STEP_TOL, _case, _noise
from test_kv8_host import KV8_CASE, KV8_SEED, MARGIN, MAX_LEFT_OUT, _unit_rows, tie_values

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
SCALE = 0.125
ERR_ARG, ERR_WORKSPACE = -1, -5
N_KEYS = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 200)
B_OP, H_OP, TMAX_OP = 5, 3, 208      # 15 (clip, head) pairs: the last block has inactive waves for every wave count


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t.contiguous().view(torch.int16)


# ---------------------------------------------------------------- the quantiser
def _quant_cache(dt):
    """[3, 3, 80, 64]: unit rows scaled by 2**k, k in -6 .. 6 by row, then the tie / subnormal rows of the host test, a zero row and an
    amax = 2**-70 row; everything rounded to the cache type first (the definition applies to what the cache holds)"""
    from dimx import kv8
    g = np.random.default_rng(17)
    x = g.standard_normal((3, 3, 80, 64)).astype(np.float32) * (2.0 ** (np.arange(80) % 13 - 6)).astype(np.float32)[None, None, :, None]
    ties = _unit_rows(tie_values()[0])
    flat = x.reshape(-1, 64)
    for i in range(9):                       # the tie rows appear below every T: at rows 0 .. of every (clip, head)
        flat[i * 80:i * 80 + 1] = ties[i % len(ties)]
    flat[2 * 80 + 5: 2 * 80 + 5 + len(ties)] = ties
    flat[3 * 80 + 7] = 0.0
    flat[3 * 80 + 8] = 0.0
    flat[3 * 80 + 8, 3] = 2.0 ** -70
    t = torch.from_numpy(x).to(dt)
    return t, kv8.quantize(t.float().numpy())


@pytest.mark.parametrize("T", [1, 17, 80])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_quantiser_is_the_definition(dev, dtype, T):
    from dimx import engine as E
    from dimx import kv8
    dt = torch.bfloat16 if dtype == "bf16" else torch.float32
    cache, (rc, rs) = _quant_cache(dt)
    poisoned = cache.clone()
    poisoned[:, :, T:] = float("nan")        # rows at or past T are not read ...
    codes = torch.full((3, 3, 80, 64), 0xAB, dtype=torch.uint8, device=dev)
    scales = torch.full((3, 3, 80), -7.0, dtype=torch.float32, device=dev)
    E.op_kv8_quantize(poisoned.to(dev), T, codes, scales)
    c, s = codes.cpu().numpy(), scales.cpu().numpy()
    assert (c[:, :, T:] == 0xAB).all() and (s[:, :, T:] == -7.0).all()       # ... and not written
    assert np.array_equal(s[:, :, :T].view(np.int32), rs[:, :, :T].view(np.int32)), "scales differ from the definition"
    same = kv8.same_codes(c[:, :, :T], rc[:, :, :T])
    assert same.all(), "%d codes differ from the definition, first at %s" % ((~same).sum(), np.argwhere(~same)[0])
    if T > 8:    # the zero row and the amax = 2**-70 row of (clip 1, head 0)
        assert (s[1, 0, 7:9] == 0).all() and not c[1, 0, 7:9].any()
    # repeats, and a cache that was a strided view before it became contiguous, give the same bits
    c2, s2 = E.op_kv8_quantize(poisoned.to(dev), T, torch.full_like(codes, 0xAB), torch.full_like(scales, -7.0))
    wide = torch.zeros(3, 3, 160, 64, dtype=dt)
    wide[:, :, ::2] = poisoned
    c3, s3 = E.op_kv8_quantize(wide.to(dev)[:, :, ::2].contiguous(), T, torch.full_like(codes, 0xAB), torch.full_like(scales, -7.0))
    for cc, ss in ((c2, s2), (c3, s3)):
        assert torch.equal(cc, codes) and torch.equal(_bits(ss), _bits(scales))


def test_quantiser_rejects_misuse_before_the_launch(dev):
    from dimx import lib as L
    cache = torch.zeros(1, 1, 8, 64, device=dev)
    codes = torch.full((1, 1, 8, 64 + 16), 0xAB, dtype=torch.uint8, device=dev)
    scales = torch.full((1, 1, 8), -7.0, device=dev)
    l = L.load()
    p = lambda t, off=0: t.data_ptr() + off
    for args in ((p(cache), 8, 0, p(codes), p(scales)), (p(cache), 8, 9, p(codes), p(scales)), (None, 8, 8, p(codes), p(scales)),
                 (p(cache), 8, 8, None, p(scales)), (p(cache), 8, 8, p(codes), None), (p(cache), 8, 8, p(codes, 4), p(scales)),
                 (p(cache, 4), 8, 8, p(codes), p(scales)), (p(cache), 8, 8, p(codes), p(scales, 2))):
        rc = l.dimx_op_kv8_quantize(L.F32, args[0], 1, 1, args[1], args[2], args[3], args[4], L.stream_ptr(dev))
        assert rc == ERR_ARG, args
    assert l.dimx_op_kv8_quantize(7, p(cache), 1, 1, 8, 8, p(codes), p(scales), L.stream_ptr(dev)) == ERR_ARG
    torch.cuda.synchronize()
    assert bool((codes == 0xAB).all()) and bool((scales == -7.0).all()), "a refused call launched something"


# ---------------------------------------------------------------- the operator
@functools.lru_cache(maxsize=None)
def _op_case(qform, n, masked):
    """One case's operands and float64 references, computed once and shared by every wave count and output type: codes / scales of
    unit-normal K / V rows over the whole Tmax (rows at and past n are valid data: the shifted references read row n), the poisoned
    copies the kernel gets, q, the mask, kv8.attention and its wrong alternatives."""
    from dimx import kv8
    g = torch.Generator().manual_seed(zlib.crc32(("kv8 %s %d %d" % (qform, n, masked)).encode()))
    B, H, Tmax = B_OP, H_OP, TMAX_OP
    kc, ks = kv8.quantize(torch.randn(B, H, Tmax, 64, generator=g).numpy())
    vc, vs = kv8.quantize(torch.randn(B, H, Tmax, 64, generator=g).numpy())
    q, qeff, _ = q_operand(B, H, qform, torch.float32, g)
    m = masks(B, n, n + 7, g) if masked else None
    mm = m[:, :n].numpy() if masked else None
    att = lambda kc_, ks_, vc_, vs_, mask_, n_: torch.from_numpy(
        kv8.attention(qeff.numpy(), kc_, ks_, vc_, vs_, mask_, n_, SCALE)).reshape(B, H * 64)
    ref = att(kc, ks, vc, vs, mm, n)
    alts = [("keys shifted by one", att(kc[:, :, 1:], ks[:, :, 1:], vc[:, :, 1:], vs[:, :, 1:], mm, n)),
            ("V scales shifted by one row", att(kc, ks, vc, vs[:, :, 1:], mm, n))]
    if n > 1:
        alts.append(("one key dropped", att(kc, ks, vc, vs, mm[:, :n - 1] if masked else None, n - 1)))
        alts.append(("K scales shifted by one row", att(kc, ks[:, :, 1:], vc, vs, mm, n)))
    pk, pks, pv, pvs = (torch.from_numpy(a.copy()) for a in (kc, ks, vc, vs))
    pk[:, :, n:] = 0x7F
    pv[:, :, n:] = 0x7F
    pks[:, :, n:] = float("nan")
    pvs[:, :, n:] = float("nan")
    mean_v = torch.from_numpy(kv8.dequantize(vc, vs)[:, :, :n].astype(np.float64).mean(2)).reshape(B, H * 64)
    return {"clean": tuple(torch.from_numpy(a) for a in (kc, ks, vc, vs)), "poisoned": (pk, pks, pv, pvs), "q": q, "mask": m,
            "ref": ref, "alts": alts, "mean_v": mean_v}


@pytest.mark.parametrize("out", ["f32", "bf16"])
@pytest.mark.parametrize("qform", ["slab1", "slab3"])
@pytest.mark.parametrize("nsplit", [0, 1, 2, 4])
def test_cross_attention_over_codes_against_the_definition(dev, nsplit, qform, out):
    from dimx import engine as E
    bf = out == "bf16"
    worst = 0.0
    for n in N_KEYS:
        for masked in (False, True):
            c = _op_case(qform, n, masked)
            kc, ks, vc, vs = (t.to(dev) for t in c["poisoned"])
            m = c["mask"].to(dev) if masked else None
            got = E.op_decode_attn_kv8(c["q"].to(dev), kc, ks, vc, vs, SCALE, n, kmask=m, nsplit=nsplit, out_bf16=bf)
            worst = max(worst, check(got.float(), c["ref"], bf, c["alts"], "n=%d masked=%d" % (n, masked)))
            # codes 0x7F and NaN scales past n_keys were never read: the clean operands give the same bits
            kc2, ks2, vc2, vs2 = (t.to(dev) for t in c["clean"])
            again = E.op_decode_attn_kv8(c["q"].to(dev), kc2, ks2, vc2, vs2, SCALE, n, kmask=m, nsplit=nsplit, out_bf16=bf)
            assert torch.equal(_bits(again), _bits(got)), "n=%d masked=%d: rows past n_keys were read" % (n, masked)
            if masked:   # the all-masked clip is the mean of the dequantised V over the n keys
                mv = c["mean_v"][3]
                assert (got[3].double().cpu() - mv).abs().max().item() <= tolerance(mv, bf).max().item()
    print("kv8 cross %s %s nsplit=%d: worst |err| %.3g" % (out, qform, nsplit, worst))


@pytest.mark.parametrize("out", ["f32", "bf16"])
def test_windowed_form_is_the_plain_form_at_the_bound(dev, out):
    from dimx import engine as E
    from dimx.online import visible
    bf = out == "bf16"
    n = 200
    c = _op_case("slab3", n, True)
    kc, ks, vc, vs = c["clean"]
    m = torch.ones(B_OP, n + 7, dtype=torch.uint8)
    m[0, [0, 3, 14, 15, 16, 62, 63, 64, 100]] = 0
    m[1, 40:] = 0
    m[2, :] = 0
    q, md = c["q"].to(dev), m.to(dev)
    seen = set()
    for L in (0, -3, 5):
        for t in [13 - L, 14 - L, 15 - L, 61 - L, 62 - L, 63 - L]:
            vis = visible(t, L, n)
            seen.add(vis)
            step = torch.tensor([t], dtype=torch.int32, device=dev)
            pk, pks, pv, pvs = kc.clone(), ks.clone(), vc.clone(), vs.clone()
            pk[:, :, vis:] = 0x7F
            pv[:, :, vis:] = 0x7F
            pks[:, :, vis:] = float("nan")
            pvs[:, :, vis:] = float("nan")
            for nsplit in (1, 2, 4, 0):
                plain = E.op_decode_attn_kv8(q, kc.to(dev), ks.to(dev), vc.to(dev), vs.to(dev), SCALE, vis, kmask=md, nsplit=nsplit, out_bf16=bf)
                win = E.op_decode_attn_kv8(q, pk.to(dev), pks.to(dev), pv.to(dev), pvs.to(dev), SCALE, n, kmask=md, nsplit=nsplit, out_bf16=bf,
                                           step=step, lookahead=L)
                assert bool(torch.isfinite(win.float()).all()), (t, L, nsplit)
                assert torch.equal(_bits(win), _bits(plain)), "step %d lookahead %d nsplit %d: vis %d" % (t, L, nsplit, vis)
    assert seen == {15, 16, 17, 63, 64, 65}


@pytest.mark.parametrize("Tmax", [208, 1024])
def test_f32_shard_reproduces_the_whole_batch(dev, Tmax):
    """out in f32 (the parity mode's handle): the automatic wave count depends on Tmax only, so the rows of a 2-clip shard have the
    bits of the 5-clip batch"""
    from dimx import engine as E
    from dimx import kv8
    g = torch.Generator().manual_seed(5 + Tmax)
    B, H, n = 5, 3, Tmax - 8
    kc, ks = (torch.from_numpy(a).to(dev) for a in kv8.quantize(torch.randn(B, H, Tmax, 64, generator=g).numpy()))
    vc, vs = (torch.from_numpy(a).to(dev) for a in kv8.quantize(torch.randn(B, H, Tmax, 64, generator=g).numpy()))
    q = torch.randn(2, B, H * 64, generator=g).to(dev)
    m = (torch.rand(B, n, generator=g) > 0.3).to(torch.uint8).to(dev)
    whole = E.op_decode_attn_kv8(q, kc, ks, vc, vs, SCALE, n, kmask=m)
    again = E.op_decode_attn_kv8(q, kc, ks, vc, vs, SCALE, n, kmask=m)
    assert torch.equal(_bits(whole), _bits(again))
    for lo, hi in ((0, 2), (3, 5)):
        part = E.op_decode_attn_kv8(q[:, lo:hi].contiguous(), kc[lo:hi].contiguous(), ks[lo:hi].contiguous(), vc[lo:hi].contiguous(),
                                    vs[lo:hi].contiguous(), SCALE, n, kmask=m[lo:hi].contiguous())
        assert torch.equal(_bits(part), _bits(whole[lo:hi])), "clips %d..%d at Tmax %d" % (lo, hi - 1, Tmax)


def test_operator_rejects_misuse_before_the_launch(dev):
    from dimx import lib as L
    l = L.load()
    B, H, Tmax = 2, 3, 2056
    kc = torch.zeros(B, H, Tmax, 64, dtype=torch.uint8, device=dev)
    ks = torch.ones(B * H * Tmax + 4, device=dev)
    q = torch.zeros(B * H * 64 + 8, device=dev)
    out = torch.full((B * H * 64 + 8,), -7.0, device=dev)
    km = torch.ones(B, Tmax, dtype=torch.uint8, device=dev)
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    good = dict(q=q.data_ptr(), q_ld=H * 64, nslab=1, kc=kc.data_ptr(), ks=ks.data_ptr(), vc=kc.data_ptr(), vs=ks.data_ptr(), out=out.data_ptr(),
                o_ld=H * 64, Tmax=Tmax, step=None, n=100, km=km.data_ptr(), kld=Tmax, rpc=1, la=0, win=0, q_f32=1, dt=L.F32)

    def call(**kw):
        a = dict(good, **kw)
        return l.dimx_op_decode_attn_kv8(a["dt"], a["q"], a["q_ld"], a["q_f32"], a["nslab"], B * a["q_ld"], a["kc"], a["ks"], a["vc"], a["vs"], a["out"],
                                         a["o_ld"], B, H, a["Tmax"], a["step"], a["n"], a["km"], a["kld"], a["rpc"], SCALE, 0, a["la"], a["win"],
                                         L.stream_ptr(dev))
    bad = [dict(q=None), dict(kc=None), dict(ks=None), dict(vc=None), dict(vs=None), dict(out=None),
           dict(q=q.data_ptr() + 4), dict(kc=kc.data_ptr() + 8), dict(vc=kc.data_ptr() + 4), dict(out=out.data_ptr() + 4), dict(ks=ks.data_ptr() + 2),
           dict(vs=ks.data_ptr() + 1), dict(q_ld=H * 64 + 2), dict(o_ld=H * 64 + 2), dict(o_ld=H * 64 + 4, dt=L.BF16),
           dict(n=0), dict(n=-1), dict(n=Tmax + 1), dict(n=2049), dict(n=100, Tmax=99), dict(kld=99),
           dict(win=1), dict(rpc=2), dict(q_f32=0), dict(nslab=0), dict(nslab=9), dict(dt=7)]
    for kw in bad:
        assert call(**kw) == ERR_ARG, kw
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()), "a refused call launched something"
    assert call() == 0 and call(win=1, step=step.data_ptr(), la=3) == 0 and call(n=2048) == 0   # the operands themselves are fine
    torch.cuda.synchronize()
    assert bool((out[:B * H * 64] != -7.0).all())


# ---------------------------------------------------------------- the generation
class _Gen:
    """the inputs of KV8_CASE (the seeds tests/test_kv8_host.py chose), built once and left unchanged"""

    def __init__(self, sd):
        self.sd = sd
        self.B, self.T, self.lens = KV8_CASE
        self.v_s, self.v_a, self.z, self.mask = _case(self.B, self.T, list(self.lens), seed=KV8_SEED)
        self.noise = _noise(self.B, self.T)
        self.m8 = self.mask.to(torch.uint8).cuda()
        self.z0 = self.z.clamp(min=0)
        self.shape_only = torch.zeros(self.B, self.T, 1)    # kv8_ref asks the context for its shape alone
        self._ref = {}

    def context(self, eng, **kw):
        eng.encode_ctx(self.v_s.cuda(), self.v_a.cuda(), self.m8, True, **kw)

    def run(self, eng, noisy, kv8=True, **kw):
        self.context(eng)
        tok, lg = eng.generate(self.z0[:, 0].cuda(), self.m8, self.T, 1.0 if noisy else 0.0, 52, self.noise.cuda() if noisy else None,
                               return_logits=True, kv8=kv8, **kw)
        return tok.cpu().long(), lg.cpu()

    def buffer_rows(self, eng):
        import kv8_ref
        return kv8_ref.dequantized(eng.cross_kv8_layers(self.B, self.T), self.T)

    def checker(self, kv, key, Pmax, lookahead, noisy):
        """kv8_ref on the given dequantised rows; cached under ``key`` (one per distinct set of rows)"""
        import kv8_ref
        k = (key, Pmax, lookahead, noisy)
        if k not in self._ref:
            self._ref[k] = kv8_ref.kv8_generate(self.sd, self.z0[:, :Pmax], None, self.T - 1, self.shape_only, self.mask, lookahead, kv,
                                                self.noise if noisy else None)
        return self._ref[k]


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


@pytest.fixture(scope="module")
def rows(eng, gen):
    """the dequantised rows of the buffer a kv8 generation of the case leaves behind (they depend on the context alone)"""
    gen.run(eng, False)
    return gen.buffer_rows(eng)


def test_buffer_holds_a_fixed_point_of_the_quantiser(eng, gen, rows):
    """re-quantising the dequantised buffer returns the buffer's codes: they are e4m3fn codes under per-row scales, written by the
    quantiser for every layer, K and V, rows 0 .. T - 1"""
    from dimx import engine as E
    from dimx import kv8
    layers = eng.cross_kv8_layers(gen.B, gen.T)
    assert len(layers) == 4 and eng.cross_kv8() is None          # generate(kv8=True) cleared the setting
    for (kc, vc, ks, vs), (k, v) in zip(layers, rows):
        assert tuple(kc.shape) == (gen.B, 12, 40, 64) and tuple(ks.shape) == (gen.B, 12, 40)
        for codes, scales, deq in ((kc, ks, k), (vc, vs, v)):
            c2, s2 = E.op_kv8_quantize(deq.cuda().contiguous(), gen.T)
            assert kv8.same_codes(c2.cpu().numpy(), codes.cpu().numpy()).all()
            assert bool(((s2 - scales).abs() <= scales * 2.0 ** -22).all())
            valid = gen.mask[:, None, :].expand(-1, 12, -1)             # padded frames hold whatever the encoder left there
            assert bool((scales.cpu()[valid] > 0).all())
            assert int((codes.cpu() & 0x7F).amax(-1)[valid].min()) == 0x7E     # a row's largest element sits at +-448


@pytest.mark.parametrize("L", [None, 0])
def test_teacher_forced_logits_match_the_checker_on_the_buffers_rows(eng, gen, rows, L):
    """the whole clip as a forced prompt (no token can diverge): every step's logits against kv8_ref on the buffer's dequantised K/V"""
    P = gen.T - 1
    prompt = gen.z0[:, :P].to(torch.int32).cuda().contiguous()
    gen.context(eng)
    tok, lg = eng.generate(None, gen.m8, gen.T, 0.0, 52, None, return_logits=True, prompt=prompt, no_prefill=True, kv8=True, lookahead=L)
    ref_tok, ref_lg, _ = gen.checker(rows, "buffer", P, L, False)
    assert torch.equal(tok.cpu().long()[:, :P - 1], gen.z0[:, 1:P])
    err = (lg.cpu() - ref_lg).abs().amax(-1)
    print("teacher-forced kv8, lookahead %s: max |logits - checker| %.3e (STEP_TOL %.0e)" % (L, err.max().item(), STEP_TOL))
    assert err.max().item() < STEP_TOL
    # the plain generation along the same tokens is further away than that: the codes are what was read
    gen.context(eng)
    _, plain = eng.generate(None, gen.m8, gen.T, 0.0, 52, None, return_logits=True, prompt=prompt, no_prefill=True, lookahead=L)
    assert (plain.cpu() - ref_lg).abs().max().item() > STEP_TOL


def test_guided_conditional_dump_matches_the_checker(eng, gen, rows):
    P = gen.T - 1
    prompt = gen.z0[:, :P].to(torch.int32).cuda().contiguous()
    gen.context(eng, guided=True)
    tok, br = eng.generate(None, gen.m8, gen.T, 0.0, 52, None, prompt=prompt, guidance=1.5, return_branches=True, kv8=True)
    _, ref_lg, _ = gen.checker(rows, "buffer", P, None, False)
    err = (br[0].cpu() - ref_lg).abs().max().item()
    print("guided kv8, conditional dump: max |logits - checker| %.3e" % err)
    assert err < STEP_TOL
    gen.context(eng, guided=True)
    _, br0 = eng.generate(None, gen.m8, gen.T, 0.0, 52, None, prompt=prompt, guidance=1.5, return_branches=True)
    assert torch.equal(br[1], br0[1])        # the unconditional half reads no cross K/V in either form
    assert not torch.equal(br[0], br0[0])


@pytest.mark.parametrize("noisy", [False, True])
def test_free_running_tokens_match_the_checker(eng, gen, rows, noisy):
    import online_ref
    tok, lg = gen.run(eng, noisy)
    ref_tok, ref_lg, margins = gen.checker(rows, "buffer", 1, None, noisy)
    keep, left_out = online_ref.compared_steps(margins, MARGIN)
    keep_lg = keep.clone()
    keep_lg[:, 1:] |= keep[:, :-1]
    keep_lg[:, 0] = True
    err = (lg - ref_lg).abs().amax(-1)
    wrong = int(((tok != ref_tok) & keep).sum())
    print("free-running kv8 noisy=%d: %d compared tokens differ, max |logits - checker| %.3e over the compared steps, smallest margin %.3e, "
          "pairs left out %.4f" % (noisy, wrong, err[keep_lg].max().item(), margins.min().item(), left_out))
    assert left_out <= MAX_LEFT_OUT
    assert wrong == 0
    assert err[keep_lg].max().item() < STEP_TOL


def test_buffer_contents_do_not_matter_and_replays_equal_a_fresh_handle(full_sd, eng, gen):
    """a 0xFF-filled buffer gives the bits of a zeroed one; a second call in the same buffer replays the graph and equals a fresh
    handle's run; after kv8 is cleared a plain generation has the bits it had before"""
    from dimx import kv8
    before = gen.run(eng, True, kv8=False)
    need = eng.cross_kv8_bytes(gen.B, gen.T)
    assert need == kv8.buffer_layout(4, gen.B, 12, 40)[1]
    buf = torch.zeros(need, dtype=torch.uint8, device="cuda:0")
    outs = []
    for fill in (0, 0xFF, 0xFF):
        buf.fill_(fill)
        eng.set_cross_kv8(buf)
        assert eng.cross_kv8() == (buf.data_ptr(), need)
        try:
            outs.append(gen.run(eng, True, kv8=False))      # the handle's own setting
        finally:
            eng.set_cross_kv8(None)
    for tok, lg in outs[1:]:
        assert torch.equal(tok, outs[0][0]) and torch.equal(lg, outs[0][1])
    fresh = _engine(full_sd)
    try:
        ftok, flg = gen.run(fresh, True)
    finally:
        fresh.close()
    assert torch.equal(ftok, outs[0][0]) and torch.equal(flg, outs[0][1])
    assert not torch.equal(outs[0][1], before[1])
    after = gen.run(eng, True, kv8=False)
    assert eng.cross_kv8() is None
    assert torch.equal(after[0], before[0]) and torch.equal(after[1], before[1])


def test_zero_context_gives_zero_codes_and_the_plain_bits(eng, gen):
    B, T = gen.B, gen.T
    x_null = (-gen.sd["patch_embed_dec_s"]).reshape(1, 1, -1).expand(B, T, -1).contiguous().cuda()

    def run(kv8):
        eng.set_context(x_null, torch.zeros_like(gen.v_a).cuda(), which_patch=0, for_generate=True)
        tok, lg = eng.generate(gen.z0[:, 0].cuda(), gen.m8, T, 1.0, 52, gen.noise.cuda(), return_logits=True, kv8=kv8)
        return tok.cpu(), lg.cpu()

    tok8, lg8 = run(True)
    for kc, vc, ks, vs in eng.cross_kv8_layers(B, T):
        assert not bool(kc.any()) and not bool(vc.any()) and bool((ks == 0).all()) and bool((vs == 0).all())
    tok, lg = run(False)
    assert torch.equal(tok8, tok) and torch.equal(_bits(lg8), _bits(lg))


def test_what_kv8_does_not_take_is_refused(eng, gen):
    from dimx import lib as L
    B, T = gen.B, gen.T
    need = eng.cross_kv8_bytes(B, T)
    buf = torch.zeros(need, dtype=torch.uint8, device="cuda:0")
    assert eng.cross_kv8_bytes(B, 1) == 0 and eng.cross_kv8_bytes(0, T) == 0
    gen.context(eng, n_samples=2)
    with pytest.raises(L.DimxError, match=r"\(-1\)"):
        eng.generate(gen.z0[:, 0].cuda(), gen.m8, T, 0.0, n_samples=2, kv8=True)
    assert eng.cross_kv8() is None
    eng.set_cross_kv8(buf)
    try:
        with pytest.raises(L.DimxError, match=r"\(-1\)"):
            eng.generate_beam(gen.z0[:, 0].cuda(), gen.m8, T, 2)
        eng.set_cross_kv8(buf[:need - 256])
        gen.context(eng)
        with pytest.raises(L.DimxError, match=r"\(-5\)"):
            eng.generate(gen.z0[:, 0].cuda(), gen.m8, T, 0.0)
        with pytest.raises(L.DimxError, match=r"\(-1\)"):
            eng.set_cross_kv8(buf[16:])          # not 256-byte aligned
    finally:
        eng.set_cross_kv8(None)
    for variant in ("slm", "legacy"):
        from dimx import engine
        other = engine.Engine("cuda:0", L.MODE_PARITY_F32, variant=variant)
        assert other.cross_kv8_bytes(B, T) == 0
        with pytest.raises(L.DimxError, match=r"\(-1\)"):
            other.set_cross_kv8(buf)
        other.close()


def test_module_forward_takes_the_kv8_route(full_sd, gen):
    from dimx.seq2seq_pretrain import SLMFT
    from dimx import prng
    model = SLMFT().eval()
    B, T = gen.B, gen.T
    v_l = torch.from_numpy(prng.normal(KV8_SEED, "kv8.vl", (B, T, 56)))
    args = [t.cuda() for t in (gen.v_s, v_l, gen.v_a, gen.mask)]
    tok = model(*args, mode="val", greedy=True, return_tokens=True)[3]
    tot, d, pred, tok8 = model(*args, mode="val", greedy=True, return_tokens=True, kv8=True)
    assert tok8.shape == tok.shape == (B, T - 1) and pred.shape == (B, T - 1, 56) and bool(torch.isfinite(pred).all())
    eng = model.engine(args[0].device)
    assert eng.cross_kv8() is None and eng.cross_kv8_buffer() is not None
    assert torch.equal(model(*args, mode="val", greedy=True, return_tokens=True)[3], tok)
    print("SLMFT.forward(kv8=True): %.0f %% of the greedy tokens equal the plain call's" % (100 * (tok8 == tok).float().mean().item()))
    for kw in ({"mode": "train"}, {"mode": "val", "n_samples": 2}, {"mode": "val", "beam_width": 2}):
        with pytest.raises(ValueError):
            model(*args, kv8=True, **kw)


def test_chain_route_completes_and_agrees_with_the_per_op_route(full_sd):
    """130 clips in bf16: the step is the chain route without the decoder-layer kernel.  Its greedy tokens equal the per-op route's
    (DIMX_NO_CHAIN=1) on every pair before a clip's first decision closer than CHAIN_MARGIN: the two routes round bf16 in different
    places (the chain's deferred LayerNorm), a bf16 activation carries 2**-9 relative rounding noise, and a logit here is a dot product
    of 384 such terms of unit scale -- 0.05 is a few standard deviations of that noise.  The f32 run's logits are reported only."""
    import online_ref
    CHAIN_MARGIN = 0.05
    B, T = 130, 12
    v_s, v_a, z, mask = _case(B, T, [T] * 100 + [7] * 30)
    m8 = mask.to(torch.uint8).cuda()

    def run(mode, no_chain):
        if no_chain:
            os.environ["DIMX_NO_CHAIN"] = "1"
        try:
            e = _engine(full_sd, mode)
        finally:
            os.environ.pop("DIMX_NO_CHAIN", None)
        e.encode_ctx(v_s.cuda(), v_a.cuda(), m8, True)
        tok, lg = e.generate(z[:, 0].clamp(min=0).cuda(), m8, T, 0.0, return_logits=True, kv8=True)
        faults = e.lib.dimx_chain_faults(e.h)
        e.close()
        return tok.cpu().long(), lg.cpu(), faults

    tok, lg, faults = run("bf16", False)
    ref_tok, ref_lg, _ = run("bf16", True)
    f32_tok, f32_lg, _ = run("f32", False)
    assert faults == 0 and bool(torch.isfinite(lg).all())
    top = torch.topk(ref_lg, 2, dim=-1).values
    keep, left_out = online_ref.compared_steps(top[..., 0] - top[..., 1], CHAIN_MARGIN)
    wrong = int(((tok != ref_tok) & keep).sum())
    same = (tok == f32_tok).float().cumprod(1)      # steps before the first token that differs from the f32 run's
    d32 = ((lg - f32_lg).abs().amax(-1) * torch.cat([torch.ones(B, 1), same[:, :-1]], 1)).max().item()
    print("kv8 chain route vs per-op route, bf16, 130 x 12: %d compared tokens differ, pairs left out %.4f; first-step logits differ by %.3e; "
          "bf16 vs f32 kv8 logits along the common history: %.3e (reported, not bounded)"
          % (wrong, left_out, (lg[:, 0] - ref_lg[:, 0]).abs().max().item(), d32))
    assert wrong == 0
    assert left_out < 1.0
