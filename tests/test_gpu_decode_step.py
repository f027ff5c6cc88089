"""GPU: the decode step's kernels against float64, at the shapes, key counts and variants dimx_generate launches.

One-query attention (csrc/decode_attn.hip, csrc/decode_attn_body.hpp) through dimx_op_decode_attn_ex: the cross form with f32
split-K q slabs, a strided key mask and every wave count; the self form with its cache append; the multi-sample form; the parity
mode's shard invariance; the table form of the first layer's self attention (dimx_op_decode_attn_tab).  The reference has the
model's mask semantics: a masked score is -finfo.max, so a row with every key masked is the plain mean of V over the n keys.
Then the residual + pre-norm of every decoder layer (dimx_op_add_slabs_layernorm).

Every attention case also checks its own tolerance: it must be smaller than what dropping one key or shifting the keys by one does
to the float64 reference, so a tolerance loose enough to pass an off-by-one fails the test itself."""
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

SCALE = 0.125
KEY_COUNTS = (1, 2, 15, 16, 17, 31, 32, 33, 63, 65, 299, 300, 1500, 2048)
F32_TOL = 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def ref_attn(q, k, v, mask=None):
    """q [B, S, H, 64], k / v [B, H, n, 64], mask [B, n] (0 = masked) -> [B, S, H, 64] float64"""
    s = torch.einsum("bshd,bhjd->bshj", q.double(), k.double()) * SCALE
    if mask is not None:
        s = s.masked_fill(mask[:, None, None, :] == 0, -torch.finfo(torch.float32).max)
    return torch.einsum("bshj,bhjd->bshd", s.softmax(-1), v.double())


def tolerance(ref, bf16):
    """f32: 1e-5 absolute on unit-scale data; bf16: one ulp of the bf16 output plus the f32 accumulation"""
    if not bf16:
        return torch.full_like(ref, F32_TOL)
    ulp = torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -100))) - 7)
    return ulp + F32_TOL


def check(out, ref, bf16, alts, what):
    """out against ref elementwise; every alternative reference (one key dropped, keys shifted) must be outside the tolerance"""
    out = out.double().cpu()
    tol = tolerance(ref, bf16)
    assert torch.isfinite(out).all(), what
    err = (out - ref).abs()
    assert (err <= tol).all(), "%s: max err %.3g (tol %.3g at the worst element)" % (what, err.max().item(), tol.flatten()[err.argmax()].item())
    for name, alt in alts:
        assert ((alt - ref).abs() > tol).any(), "%s: the tolerance cannot tell %s from the right answer" % (what, name)
    return err.max().item()


def masks(B, n, ld, g):
    """clip 0 random, 1 only key 0 kept, 2 only the last key kept, 3 every key masked, 4.. random (ragged lengths)"""
    m = (torch.rand(B, ld, generator=g) > 0.4).to(torch.uint8)
    m[1:4] = 0
    m[1, 0] = 1
    m[2, n - 1] = 1
    for b in range(4, B):
        m[b, n - b:] = 0
        m[b, 0] = 1
    m[:, n:] = 7   # past n_keys: never read
    return m


def cache_pair(B, H, Tmax, n, dt, g):
    """K / V caches whose rows at and past n are NaN, and the clean data of n + 1 rows behind them (for the shifted reference)"""
    data_k = torch.randn(B, H, n + 1, 64, generator=g).to(dt)
    data_v = torch.randn(B, H, n + 1, 64, generator=g).to(dt)
    kc = torch.full((B, H, Tmax, 64), float("nan"), dtype=dt)
    vc = kc.clone()
    kc[:, :, :n] = data_k[:, :, :n]
    vc[:, :, :n] = data_v[:, :, :n]
    return kc, vc, data_k, data_v


def q_operand(R, H, qform, dt, g):
    """(q as the kernel gets it, q as the kernel computes with it [R, H, 64] f32)"""
    ld = H * 64 + 64
    if qform == "cache":
        q = torch.randn(R, ld, generator=g).to(dt)
        return q, q[:, :H * 64].float().view(R, H, 64), False
    ns = int(qform[4:])
    slabs = torch.randn(ns, R, ld, generator=g) / ns ** 0.5
    q = slabs[0].clone()
    for s in range(1, ns):
        q += slabs[s]           # slab order, float32: what the kernel sums
    return slabs, q[:, :H * 64].view(R, H, 64), True


@pytest.mark.parametrize("nsplit", [0, 1, 2, 4])
@pytest.mark.parametrize("qform", ["cache", "slab1", "slab3", "slab8"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_cross_attention_against_float64(dev, dtype, qform, nsplit):
    from dimx import engine as E
    bf = dtype == "bf16"
    dt = torch.bfloat16 if bf else torch.float32
    B, H = 5, 3                 # 15 (clip, head) pairs: the last block has inactive pairs for every wave count
    g = _gen(zlib.crc32(("%s %s %d" % (dtype, qform, nsplit)).encode()))
    worst = 0.0
    for n in KEY_COUNTS:
        Tmax = min(n + 5, 2048)   # Tmax > n_keys, and Tmax = n_keys = 2048
        kc, vc, dk, dv = cache_pair(B, H, Tmax, n, dt, g)
        q, qeff, q_f32 = q_operand(B, H, qform, dt, g)
        qe = qeff.view(B, 1, H, 64)
        kcd, vcd = kc.to(dev), vc.to(dev)
        for ld in (None, n, n + 7):   # no mask; the product's kmask_ld = n_keys; a wider mask row
            m = masks(B, n, ld, g) if ld else None
            mm = m[:, :n] if ld else None
            ref = ref_attn(qe, dk[:, :, :n], dv[:, :, :n], mm).view(B, H * 64)
            alts = [("keys shifted by one", ref_attn(qe, dk[:, :, 1:], dv[:, :, 1:], mm).view(B, H * 64))]
            if n > 1:
                alts.append(("one key dropped", ref_attn(qe, dk[:, :, :n - 1], dv[:, :, :n - 1],
                                                         mm[:, :n - 1] if ld else None).view(B, H * 64)))
            out = E.op_decode_attn_ex(q.to(dev), kcd, vcd, SCALE, n_keys=n, kmask=m.to(dev) if ld else None,
                                      kmask_ld=ld, nsplit=nsplit, q_f32=q_f32)
            worst = max(worst, check(out.float(), ref, bf, alts, "n=%d Tmax=%d ld=%s" % (n, Tmax, ld)))
            if ld:   # the all-masked clip is the plain mean of V over the n keys
                mean_v = dv[:, :, :n].double().mean(2).reshape(B, H * 64)[3]
                assert (out[3].double().cpu() - mean_v).abs().max().item() <= tolerance(mean_v, bf).max().item()
    print("cross %s %s nsplit=%d: worst |err| %.3g" % (dtype, qform, nsplit, worst))


@pytest.mark.parametrize("nslab", [0, 1, 4])   # 0: q / k / v in the cache type
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_self_attention_appends_one_row_and_attends_over_step_plus_one_keys(dev, dtype, nslab):
    from dimx import engine as E
    bf = dtype == "bf16"
    dt = torch.bfloat16 if bf else torch.float32
    B, H, Tmax = 5, 3, 320
    hd = H * 64
    g = _gen(17 + nslab + 3 * bf)
    sentinel = torch.tensor(float("nan"), dtype=dt)
    for step in (0, 1, 15, 31, 32, 63, 299, Tmax - 1):
        for nsplit in (0, 1, 2, 4):
            data_k = torch.randn(B, H, Tmax + 1, 64, generator=g).to(dt)
            data_v = torch.randn(B, H, Tmax + 1, 64, generator=g).to(dt)
            kc = torch.full((B, H, Tmax, 64), float("nan"), dtype=dt)
            vc = kc.clone()
            kc[:, :, :step], vc[:, :, :step] = data_k[:, :, :step], data_v[:, :, :step]
            kc[:, :, step + 1:] = sentinel
            vc[:, :, step + 1:] = sentinel
            if nslab == 0:
                qkv = torch.randn(B, 3 * hd, generator=g).to(dt)
                eff = qkv.float()
            else:
                qkv = torch.randn(nslab, B, 3 * hd, generator=g) / nslab ** 0.5
                eff = qkv[0].clone()
                for s in range(1, nslab):
                    eff += qkv[s]
            qe, kn, vn = (eff[:, i * hd:(i + 1) * hd].reshape(B, H, 1, 64) for i in range(3))
            kcd, vcd = kc.to(dev), vc.to(dev)
            step_d = torch.tensor([step], dtype=torch.int32, device=dev)
            out = E.op_decode_attn_ex(qkv.to(dev), kcd, vcd, SCALE, step=step_d, nsplit=nsplit, q_f32=nslab > 0)
            # the cache: row `step` is the new k / v (f32 slab sum, or its bf16 round-to-nearest-even); every other row bit-unchanged
            kco, vco = kcd.cpu(), vcd.cpu()
            assert torch.equal(kco[:, :, step], kn[:, :, 0].to(dt)) and torch.equal(vco[:, :, step], vn[:, :, 0].to(dt)), step
            for new, old in ((kco, kc), (vco, vc)):
                rows = torch.ones(Tmax, dtype=torch.bool)
                rows[step] = False
                iv = torch.int16 if bf else torch.int32
                assert torch.equal(new[:, :, rows].view(iv), old[:, :, rows].view(iv)), step
            # the output: cached keys in the cache type, this step's key and value at f32 (what the kernel computes with)
            k_all = torch.cat([kc[:, :, :step].double(), kn.double()], 2)
            v_all = torch.cat([vc[:, :, :step].double(), vn.double()], 2)
            q4 = qe.view(B, 1, H, 64)
            ref = ref_attn(q4, k_all, v_all).view(B, hd)
            alts = []
            if step > 0:   # step 0: the one key is this step's own
                alts.append(("keys shifted by one", ref_attn(q4, torch.cat([data_k[:, :, 1:step + 1].double(), kn.double()], 2),
                                                             torch.cat([data_v[:, :, 1:step + 1].double(), vn.double()], 2)).view(B, hd)))
                alts.append(("one key dropped", ref_attn(q4, k_all[:, :, 1:], v_all[:, :, 1:]).view(B, hd)))
            check(out.float(), ref, bf, alts, "step=%d nsplit=%d" % (step, nsplit))


# ---------------------------------------------------------------- the table form of the first layer's self attention

def _table(B, H, Tmax, dt, g):
    """A [512 + 8, ld] table in the layout generate's self_args sets (bf16: K | V, f32: q | K | V), its 8 spare rows NaN; a token
    history [B, Tmax + 1] with repeated ids; the K / V rows it addresses as [B, H, Tmax + 1, 64]"""
    hd = H * 64
    ld, koff, voff = (2 * hd, 0, hd) if dt == torch.bfloat16 else (3 * hd, hd, 2 * hd)
    tab = torch.randn(520, ld, generator=g).to(dt)
    tab[512:] = float("nan")
    hist = torch.randint(0, 512, (B, Tmax + 1), generator=g, dtype=torch.int32)
    hist[:, 9] = hist[:, 5]      # repeats, clear of positions 0 / 1: at step 1 "keys shifted by one" must differ from the right keys
    hist[:, 17] = hist[:, 3]
    rows = tab[hist.long()]
    data_k, data_v = (rows[..., off:off + hd].reshape(B, Tmax + 1, H, 64).permute(0, 2, 1, 3).contiguous() for off in (koff, voff))
    return tab, koff, voff, hist, data_k, data_v


def _table_case(dev, tab_d, koff, voff, hist, data_k, data_v, Tmax, step, nsplit, g):
    """one launch of the table form at `step`: caches untouched, the bits of the cache form on gathered caches, float64"""
    from dimx import engine as E
    dt = data_k.dtype
    bf = dt == torch.bfloat16
    B, H = data_k.shape[:2]
    hd = H * 64
    qkv = torch.randn(2, B, 3 * hd, generator=g) / 2 ** 0.5
    eff = qkv[0] + qkv[1]
    qe, kn, vn = (eff[:, i * hd:(i + 1) * hd].reshape(B, H, 1, 64) for i in range(3))
    h = hist[:, :Tmax].clone()
    h[:, step:] = (512 + torch.arange(Tmax - step) % 8).to(torch.int32)    # stale ids past the table: clamped, loaded, not used
    nan_c = torch.full((B, H, Tmax, 64), float("nan"), dtype=dt)
    kcd, vcd = nan_c.to(dev), nan_c.to(dev)
    step_d = torch.tensor([step], dtype=torch.int32, device=dev)
    out = E.op_decode_attn_ex(qkv.to(dev), kcd, vcd, SCALE, step=step_d, nsplit=nsplit, q_f32=True, tab=tab_d, hist=h.to(dev),
                              tab_koff=koff, tab_voff=voff, tab_rows=512)
    iv = torch.int16 if bf else torch.int32
    assert torch.equal(kcd.cpu().view(iv), nan_c.view(iv)) and torch.equal(vcd.cpu().view(iv), nan_c.view(iv)), "the table form appends nothing"
    kc, vc = nan_c.clone(), nan_c.clone()
    kc[:, :, :step], vc[:, :, :step] = data_k[:, :, :step], data_v[:, :, :step]
    cache_form = E.op_decode_attn_ex(qkv.to(dev), kc.to(dev), vc.to(dev), SCALE, step=step_d, nsplit=nsplit, q_f32=True)
    assert torch.equal(out.view(iv), cache_form.view(iv)), "table form != cache form on gathered caches (step=%d nsplit=%d)" % (step, nsplit)
    q4 = qe.view(B, 1, H, 64)
    k_all = torch.cat([data_k[:, :, :step].double(), kn.double()], 2)
    v_all = torch.cat([data_v[:, :, :step].double(), vn.double()], 2)
    ref = ref_attn(q4, k_all, v_all).view(B, hd)
    alts = []
    if step > 0:
        alts.append(("keys shifted by one", ref_attn(q4, torch.cat([data_k[:, :, 1:step + 1].double(), kn.double()], 2),
                                                     torch.cat([data_v[:, :, 1:step + 1].double(), vn.double()], 2)).view(B, hd)))
        alts.append(("one key dropped", ref_attn(q4, k_all[:, :, 1:], v_all[:, :, 1:]).view(B, hd)))
    return check(out.float(), ref, bf, alts, "table form step=%d nsplit=%d" % (step, nsplit))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_table_form_self_attention(dev, dtype):
    """decode_attn_body<.., TAB> through dimx_op_decode_attn_tab, every wave count of both types: B * H = 15 pairs run 4 waves per
    pair on their own (bf16), Tmax = 320 runs 1 (f32)"""
    dt = torch.bfloat16 if dtype == "bf16" else torch.float32
    B, H, Tmax = 5, 3, 320
    g = _gen(4000 + (dtype == "bf16"))
    tab, koff, voff, hist, data_k, data_v = _table(B, H, Tmax, dt, g)
    tab_d = tab.to(dev)
    worst = 0.0
    for step in (0, 1, 15, 31, 32, 63, 299, Tmax - 1):
        for nsplit in (0, 1, 2, 4):
            worst = max(worst, _table_case(dev, tab_d, koff, voff, hist, data_k, data_v, Tmax, step, nsplit, g))
    print("table form %s: worst |err| %.3g" % (dtype, worst))


@pytest.mark.parametrize("Tmax", [512, 1024])
def test_table_form_f32_takes_its_wave_count_from_the_cache_length(dev, Tmax):
    """nsplit = 0 in f32: 2 waves per pair from Tmax = 512, 4 from 1024 (launch_decode_attn) -- the table instantiations of both"""
    B, H = 5, 3
    g = _gen(Tmax + 1)
    tab, koff, voff, hist, data_k, data_v = _table(B, H, Tmax, torch.float32, g)
    _table_case(dev, tab.to(dev), koff, voff, hist, data_k, data_v, Tmax, Tmax - 1, 0, g)


def test_table_form_rejects_misuse_before_the_launch(dev):
    from dimx import engine as E
    from dimx import lib as L
    B, H, Tmax = 2, 3, 40
    hd = H * 64
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    hist = torch.zeros(B, Tmax, dtype=torch.int32, device=dev)
    for dt, ld, koff, voff, bad in ((torch.float32, 3 * hd, hd, 2 * hd, 2), (torch.bfloat16, 2 * hd, 0, hd, 4)):
        kc = torch.zeros(B, H, Tmax, 64, dtype=dt, device=dev)
        tab = torch.zeros(16, ld, dtype=dt, device=dev)
        q = torch.zeros(B, 3 * hd, device=dev)
        ok = dict(step=step, q_f32=True, tab=tab, hist=hist, tab_koff=koff, tab_voff=voff)
        E.op_decode_attn_ex(q, kc, kc.clone(), SCALE, **ok)
        for kw in (dict(ok, hist=hist[:, :Tmax - 1].contiguous()),            # a history row shorter than Tmax
                   dict(ok, tab_koff=koff + bad), dict(ok, tab_voff=voff - bad),  # offsets off the 16-byte chunk
                   dict(ok, tab_voff=ld - hd + 16)):                           # V past the end of the table row
            with pytest.raises(L.DimxError):
                E.op_decode_attn_ex(q, kc, kc.clone(), SCALE, **kw)
        with pytest.raises(L.DimxError):                                       # q in the cache type: the table form takes f32 slabs only
            E.op_decode_attn_ex(q.to(dt) if dt == torch.bfloat16 else q, kc, kc.clone(), SCALE, **dict(ok, q_f32=False))


@pytest.mark.parametrize("S", [2, 4, 5, 8, 10])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_multi_sample_cross_attention(dev, dtype, S):
    from dimx import engine as E
    bf = dtype == "bf16"
    dt = torch.bfloat16 if bf else torch.float32
    B, H = 6, 3
    g = _gen(31 + S + 100 * bf)
    for n in (1, 17, 77, 300):
        Tmax = n + 3
        kc, vc, dk, dv = cache_pair(B, H, Tmax, n, dt, g)
        m = masks(B, n, n, g)
        m[5] = 0                # a clip whose context is empty
        for qform in ("slab1", "cache"):
            q, qeff, q_f32 = q_operand(B * S, H, qform, dt, g)
            qe = qeff.view(B, S, H, 64)
            out = E.op_decode_attn_ex(q.to(dev), kc.to(dev), vc.to(dev), SCALE, n_keys=n, kmask=m.to(dev), rows_per_clip=S,
                                      q_f32=q_f32)
            ref = ref_attn(qe, dk[:, :, :n], dv[:, :, :n], m).reshape(B * S, H * 64)
            alts = [("keys shifted by one", ref_attn(qe, dk[:, :, 1:], dv[:, :, 1:], m).reshape(B * S, H * 64))]
            if n > 1:
                alts.append(("one key dropped", ref_attn(qe, dk[:, :, :n - 1], dv[:, :, :n - 1], m[:, :n - 1]).reshape(B * S, H * 64)))
            check(out.float(), ref, bf, alts, "S=%d n=%d %s" % (S, n, qform))
    # a count the LDS score buffer cannot hold is refused before the launch
    from dimx import lib as L
    kc = torch.zeros(2, H, 1500, 64, dtype=dt, device=dev)
    q = torch.zeros(2 * 10, H * 64, dtype=torch.float32, device=dev)
    if S == 10:
        with pytest.raises(L.DimxError, match="LDS"):
            E.op_decode_attn_ex(q, kc, kc, SCALE, n_keys=1500, rows_per_clip=10)


@pytest.mark.parametrize("Tmax", [300, 512, 1024])   # one per wave-count regime of the f32 mode (1, 2, 4 waves)
def test_parity_mode_shard_reproduces_the_whole_batch(dev, Tmax):
    """In f32 the wave count depends on Tmax only: a shard of clips gives the whole batch's rows bit for bit"""
    from dimx import engine as E
    B, H, n = 23, 12, Tmax - 3
    g = _gen(Tmax)
    kc, vc, _, _ = cache_pair(B, H, Tmax, n, torch.float32, g)
    m = masks(B, n, n, g)
    q, _, _ = q_operand(B, H, "slab3", torch.float32, g)
    whole = E.op_decode_attn_ex(q.to(dev), kc.to(dev), vc.to(dev), SCALE, n_keys=n, kmask=m.to(dev)).cpu()
    for lo, hi in ((0, 1), (3, 11), (17, 23)):
        part = E.op_decode_attn_ex(q[:, lo:hi].contiguous().to(dev), kc[lo:hi].contiguous().to(dev), vc[lo:hi].contiguous().to(dev),
                                   SCALE, n_keys=n, kmask=m[lo:hi].contiguous().to(dev)).cpu()
        assert torch.equal(part, whole[lo:hi]), (Tmax, lo, hi)


def test_decode_attn_ex_rejects_misuse_before_the_launch(dev):
    from dimx import engine as E
    from dimx import lib as L
    kc = torch.zeros(2, 3, 40, 64, device=dev)
    q = torch.zeros(2, 3 * 64, device=dev)
    for kw in (dict(n_keys=0), dict(n_keys=41), dict(n_keys=10, kmask=torch.ones(2, 10, dtype=torch.uint8, device=dev), kmask_ld=9),
               dict(step=torch.zeros(1, dtype=torch.int32, device=dev))):   # self form: q rows narrower than q | k | v
        with pytest.raises(L.DimxError):
            E.op_decode_attn_ex(q, kc, kc, SCALE, **kw)



@pytest.mark.parametrize("Lq", [1, 10, 130])
@pytest.mark.parametrize("Lk", [40, 64, 77, 300])
def test_matrix_core_attention_fully_masked_row_is_the_mean_of_v(dev, Lq, Lk):
    """The bf16 multi-sample step runs the prefill kernel (attention_tr.hip) with Lq = S queries per clip over the context K / V.
    A clip whose mask keeps no key gets the mean of V over its Lk keys, as the decode kernels and the reference's -FLT_MAX fill
    do -- not the mean over the 64 slots of each tile (slots past Lk repeat row Lk - 1).  The other clips: float64 within the
    kernel's bf16 rounding of P and of the output (test_gpu_kernels' bound)."""
    from dimx import engine as E
    B, H, D = 4, 3, 64
    g = _gen(Lq * 1000 + Lk)
    q, k, v = (torch.randn(B, L_, H, D, generator=g).bfloat16().float() for L_ in (Lq, Lk, Lk))
    m = torch.ones(B, Lk, dtype=torch.uint8)
    m[0] = (torch.rand(Lk, generator=g) > 0.3).to(torch.uint8)
    m[0, 0] = 1
    m[1] = 0                   # empty context
    m[2, :Lk - 1] = 0          # only the last key
    out = E.op_attention(q.to(dev), k.to(dev), v.to(dev), SCALE, False, None, m.to(dev), bf16=True, row_v=True).double().cpu()
    assert torch.isfinite(out).all()
    mean_v = v[1].double().mean(0)                                    # [H, D]
    assert ((out[1] - mean_v).abs() <= tolerance(mean_v, True)).all(), (out[1] - mean_v).abs().max().item()
    s = torch.einsum("bihd,bjhd->bhij", q.double(), k.double()) * SCALE
    s = s.masked_fill(m[:, None, None, :] == 0, -torch.finfo(torch.float32).max)
    ref = torch.einsum("bhij,bjhd->bihd", s.softmax(-1), v.double())
    assert (out - ref).abs().max().item() < 2.5e-2
    # clip 1 would be far from its mean over the tile slots
    slots = -(-Lk // 64) * 64
    slot_mean = (v[1].double().sum(0) + (slots - Lk) * v[1, Lk - 1].double()) / slots
    if slots > Lk:
        assert ((slot_mean - mean_v).abs() > tolerance(mean_v, True)).any()


def test_all_masked_context_through_generate(full_sd):
    """bf16 mode, best-of-N: a clip whose context mask is all zero.  Its step-0 logits are finite and agree to bf16 level on the
    three paths of the cross attention: the matrix-core multi-sample kernel, the VALU multi-query kernel (DIMX_NO_MULTI_TR=1) and
    the one-row-per-clip kernel (S = 1).  Every sample of a clip has the same step-0 input, so its step-0 logits are the clip's."""
    import os
    from dimx import engine, lib, prng
    B, T, S = 3, 72, 4
    v_s = torch.from_numpy(prng.normal(41, "s2s.vs", (B, T, 56)))
    v_a = torch.from_numpy(prng.normal(41, "s2s.va", (B, T, 768)))
    z = torch.from_numpy(prng.integers(41, "s2s.z", (B, T), 0, 512))
    mask = torch.zeros(B, T, dtype=torch.bool)
    mask[0, :72] = True
    mask[2, :33] = True            # clip 1: empty context
    m8 = mask.to(torch.uint8).cuda()
    out = {}
    for name, n_samples, env in (("tr", S, None), ("valu", S, "1"), ("one", 1, None)):
        if env is None:
            os.environ.pop("DIMX_NO_MULTI_TR", None)
        else:
            os.environ["DIMX_NO_MULTI_TR"] = env
        try:
            e = engine.Engine("cuda:0", lib.MODE_PERF_BF16)       # the switch is read when the handle is created
        finally:
            os.environ.pop("DIMX_NO_MULTI_TR", None)
        e.load_state_dict(full_sd)
        e.encode_ctx(v_s.cuda(), v_a.cuda(), m8, True, n_samples=n_samples)
        _, lg = e.generate(z[:, 0].cuda(), m8, T, 1.0, return_logits=True, n_samples=n_samples)
        out[name] = lg[:, 0].cpu().view(B, n_samples, -1)
        e.close()
    for name, lg in out.items():
        assert torch.isfinite(lg).all(), name
    one = out["one"][:, 0]
    for name in ("tr", "valu"):
        for s_ in range(S):
            d = (out[name][:, s_] - one).abs().max(1).values
            print("all-masked context, %s vs S = 1: step-0 logits differ by %s" % (name, [round(x, 4) for x in d.tolist()]))
            assert d.max().item() < 3e-2, (name, s_, d.tolist())


# ---------------------------------------------------------------- residual + pre-norm of the decode step

@pytest.mark.parametrize("out_bf16", [False, True])
@pytest.mark.parametrize("C", [384, 512, 768, 1152])
def test_add_slabs_layernorm(dev, C, out_bf16):
    from dimx import lib as L
    lib = L.load()
    g = _gen(C + out_bf16)
    gamma = torch.rand(C, generator=g) + 0.5
    worst = 0.0
    for M in (1, 37, 256, 1025, 2051):          # > 1024 rows: four rows (waves) per block
        for nslab in (0, 1, 3, 4, 5, 8):
            x = torch.randn(M, C, generator=g)
            x[M // 2] = 100.0 + torch.randn(C, generator=g)     # a row whose mean is 100 times its spread
            slabs = torch.randn(max(nslab, 1), M, C, generator=g) * 0.3
            want_x = x.clone()
            for s in range(nslab):
                want_x += slabs[s]               # slab order, float32
            xd, sd_, gd = x.to(dev), slabs.to(dev), gamma.to(dev)
            y = torch.empty(M, C, dtype=torch.bfloat16 if out_bf16 else torch.float32, device=dev)
            L.check(lib.dimx_op_add_slabs_layernorm(L.BF16 if out_bf16 else L.F32, L.ptr(xd), L.ptr(sd_) if nslab else None, nslab,
                                                    M * C, L.ptr(y), L.ptr(gd), M, C, L.stream_ptr(dev)), "dimx_op_add_slabs_layernorm")
            xo = xd.cpu()
            assert torch.equal(xo.view(torch.int32), want_x.view(torch.int32)), (M, nslab)
            xn = want_x.double()
            mu, sd = xn.mean(1, keepdim=True), xn.var(1, unbiased=False, keepdim=True).sqrt()
            ref = (xn - mu) / (sd ** 2 + 1e-5).sqrt() * gamma.double()
            # f32: 1e-5 on unit rows; the row mean's f32 rounding enters as |mean| / spread (1e-6 per unit: 1.1e-4 for the hard row)
            tol = (1e-5 + 1e-6 * mu.abs() / sd).expand_as(ref)
            if out_bf16:
                tol = tol + tolerance(ref, True) - F32_TOL
            err = (y.double().cpu() - ref).abs()
            assert (err <= tol).all(), (M, nslab, err.max().item())
            worst = max(worst, (err / tol).max().item())
    print("add_slabs_layernorm C=%d bf16=%s: worst err / tol %.3g" % (C, out_bf16, worst))

