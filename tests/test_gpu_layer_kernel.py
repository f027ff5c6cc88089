"""GPU: the decoder-layer kernel (csrc/chain.hip xcd_layer_kernel, through dimx_op_layer_chain / dimx_op_layer_chain_tab) against
the four launches it replaces, bit for bit, and against float64 stage by stage (tests/layer_ref.py).

H = 12, D = 64, C = 1152, scale 0.125 are the only values the operator takes.  Inputs are unit-scale: weights / sqrt(K), the
residual stream randn * 1.5 + 0.7, cache rows at and past the live count NaN, three sentinel rows past B in every buffer.

The float64 checks start each stage from the kernel's own observable output of the stage before (qc, the final o; x1 is
reconstructed as x - o . Wco^T), so a bf16 rounding tie upstream is not charged to the next stage.  The first self-attention
output is not observable at all, and neither is y1 = bf16(x1): where the float64 value is within the attention tolerance's f32
term of a rounding midpoint the reference takes the neighbour the observed x (qc) asks for (layer_ref.admissible_bf16),
everywhere else the nearest bf16.  Every
tolerance must reject every wrong answer of layer_ref (a key dropped, keys shifted, the mask ignored, a k-tile missing, a CU's
column slice shifted, statistics without the centring term): asserted next to each bound."""
import functools

import pytest
import torch

import layer_ref as R
from test_gpu_decode_step import tolerance

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

T, TP, NKEYS = 72, 80, 72
SENT = 777.0
DEV = "cuda:0"


@functools.lru_cache(maxsize=2)
def inputs(B):
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return R.make_inputs(B, T, TP, NKEYS, seed=B, device=DEV)


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def run_layer(inp, qkv, step, x0=None, sk=None, sv=None, B=None, **kw):
    """one launch on fresh output buffers filled with a sentinel; sk / sv: caches to append to (default: copies live up to step)"""
    from dimx import engine as E
    rows, bf = inp["R"], torch.bfloat16
    x = (inp["x0"] if x0 is None else x0).clone()
    sk = R.live_cache(inp["sk"], step) if sk is None else sk
    sv = R.live_cache(inp["sv"], step) if sv is None else sv
    o = torch.full((rows, R.INNER), SENT, dtype=bf, device=DEV)
    qc = torch.full((rows, R.INNER), SENT, device=DEV)
    y = torch.full((rows, R.C), SENT, dtype=bf, device=DEV)
    step_d = torch.tensor([step], dtype=torch.int32, device=DEV)
    y, o, qc, stats, flags = E.op_layer_chain(qkv, sk, sv, inp["ck"], inp["cv"], inp["n_keys"], inp["mask"], inp["w_so"], inp["w_cq"],
                                              inp["colsum"], inp["w_co"], x, step_d, B=inp["B"] if B is None else B, scale=R.SCALE,
                                              o=o, qc=qc, y=y, **kw)
    return dict(x=x, y=y, o=o, qc=qc, stats=stats, sk=sk, sv=sv, flags=flags)


def four_launches(inp, qkv, step):
    """self attention | {out-projection + residual, cross-q} | cross attention | {out-projection + residual} on copies"""
    from dimx import engine as E
    B = inp["B"]
    x = inp["x0"].clone()
    sk, sv = R.live_cache(inp["sk"], step), R.live_cache(inp["sv"], step)
    step_d = torch.tensor([step], dtype=torch.int32, device=DEV)
    o1 = E.op_decode_attn_ex(qkv[:, :B].contiguous(), sk[:B], sv[:B], R.SCALE, step=step_d, q_f32=True)
    _, _, qc = E.op_chain_ln(x[:B], o1, inp["w_so"], inp["w_cq"], inp["colsum"])
    o2 = E.op_decode_attn_ex(qc, inp["ck"][:B], inp["cv"][:B], R.SCALE, n_keys=inp["n_keys"], kmask=inp["mask"][:B], q_f32=True)
    y, stats, _ = E.op_chain_ln(x[:B], o2, inp["w_co"])
    return dict(x=x, y=y, o=o2, qc=qc, stats=stats, sk=sk, sv=sv)


def assert_same_as_four_launches(inp, qkv, step, out):
    B = inp["B"]
    want = four_launches(inp, qkv, step)
    assert out["flags"] == 0
    for name in ("x", "y", "qc", "o"):
        assert same_bits(out[name][:B], want[name][:B]), "%s differs from the four launches (B=%d step=%d)" % (name, B, step)
    for name in ("stats", "sk", "sv"):
        assert same_bits(out[name], want[name]), "%s differs from the four launches (B=%d step=%d)" % (name, B, step)


def within(got, ref, tol, alts, what):
    """|got - ref| <= tol elementwise, and every wrong answer is outside tol somewhere; returns the worst err / tol"""
    got = got.double()
    assert torch.isfinite(got).all(), what
    err = (got - ref).abs()
    tol = tol if torch.is_tensor(tol) else torch.full_like(ref, tol)
    print("%s: worst err %.3g (tol %.3g there)" % (what, err.max().item(), tol.flatten()[err.argmax()].item()))
    assert (err <= tol).all(), "%s: max err %.3g (tol %.3g at the worst element)" % (what, err.max().item(), tol.flatten()[err.argmax()].item())
    for name, alt in alts:
        assert ((alt - ref).abs() > tol).any(), "%s: the tolerance cannot tell '%s' from the right answer" % (what, name)
    return err.max().item()


def assert_matches_float64(inp, qkv, step, out, rows=None, what=""):
    """Case (b) for the clips `rows` (default all).  Returns the worst errors {x, qc, o, mean, var (relative), moved}."""
    B, rows_all = inp["B"], inp["R"]
    rows = torch.arange(B, device=DEV) if rows is None else rows.to(DEV)
    assert out["flags"] == 0, what
    r = R.reference(inp, qkv, step, rows=rows, obs=out)
    fig = {"moved": r["moved"]}
    # the caches: row `step` is bf16(f32 slab sum) bit for bit, every other row (and every row of the sentinel clips) untouched
    for name, col in (("sk", 1), ("sv", 2)):
        want = r["qkv"][:, col * R.INNER:(col + 1) * R.INNER].reshape(-1, R.H, R.D).to(torch.bfloat16)
        assert same_bits(out[name][rows, :, step], want), "%s %s: appended row" % (what, name)
        rest = out[name].clone()
        rest[:B, :, step] = float("nan")
        assert same_bits(rest, R.live_cache(inp[name], step)), "%s %s: another row changed" % (what, name)
    # the residual stream, through both projections
    fig["x"] = within(out["x"][rows], r["x2"], R.X_TOL, r["alts"]["x"], what + " x")
    assert same_bits(out["y"][:B], out["x"][:B].bfloat16()), what + " y is not bf16(x)"
    # cross-q on the kernel's own operands
    fig["qc"] = within(out["qc"][rows], r["qc"], R.QC_TOL, r["alts"]["qc"], what + " qc")
    # cross attention from the kernel's own qc
    fig["o"] = within(out["o"][rows].float(), r["o2_exact"], tolerance(r["o2_exact"], True), r["alts"]["o"], what + " o")
    for i in (rows == 3).nonzero().flatten().tolist():    # every key masked: the plain mean of V over the n keys
        mean_v = inp["cv"][3, :, :inp["n_keys"]].double().mean(1).reshape(-1)
        assert ((out["o"][3].double() - mean_v).abs() <= tolerance(mean_v, True)).all(), what
    # the partial statistics of x, recombined as the consumer does
    st = out["stats"].permute(0, 2, 1, 3).reshape(256, R.CUS, 2)
    mean, var = R.merge_stats(st[rows])
    fig["mean"] = (mean - r["mean2"]).abs().max().item()
    fig["var"] = ((var - r["var2"]) / r["var2"]).abs().max().item()
    print("%s stats: mean err %.3g, relative variance err %.3g, %d bf16 operands moved" % (what, fig["mean"], fig["var"], fig["moved"]))
    assert fig["mean"] <= R.MEAN_TOL and fig["var"] <= R.VAR_RTOL, (what, fig)
    for name, alt in r["alts"]["stats"]:
        assert R.stats_separated(r["mean2"], r["var2"], alt), "%s: the statistics bounds cannot tell '%s' from the right answer" % (what, name)
    assert (st[B:] == 0).all(), what + ": statistics of rows past B"
    # sentinel rows
    assert (out["x"][B:] == 12345.0).all() and rows_all > B, what
    for name in ("y", "o", "qc"):
        assert (out[name][B:] == SENT).all(), "%s: %s rows past B" % (what, name)
    return fig


@pytest.mark.parametrize("B", [129, 130, 160, 200, 256])
def test_layer_kernel_has_the_bits_of_the_four_launches(B):
    """(a) DESIGN and the kernel's header promise "the same arithmetic in the same order": x, y, stats, qc, o and both self caches.
    B: one row in the last live group, two rows, full groups, a partly filled last group, full."""
    inp = inputs(B)
    for step, nslab in ((0, 1), (33, 2), (71, 4)):
        qkv = R.slabs(inp, nslab)
        assert_same_as_four_launches(inp, qkv, step, run_layer(inp, qkv, step))


@pytest.mark.parametrize("B", [129, 200, 256])
def test_layer_kernel_against_float64_stage_by_stage(B):
    """(b) T = 72, Tp = 80 > n_keys = 72, every step around the 32-key batch, 1 / 2 / 4 slabs, ragged / first-only / last-only /
    all-masked context masks.  Bounds: layer_ref X_TOL, QC_TOL, MEAN_TOL, VAR_RTOL and test_gpu_decode_step.tolerance().
    Worst errors measured over these cases (MI355X): x 4.8e-6 (bound 2e-4), qc 2.4e-6 (2e-3), o 7.8e-3 where one bf16 ulp is
    1.56e-2, recombined mean 2.4e-8 (2e-5), variance 3.3e-8 relative (1e-5); at most 23 of a case's bf16 operands sat on a tie."""
    inp = inputs(B)
    worst = {}
    for step in (0, 1, 31, 32, 33, 71):
        for nslab in (1, 2, 4):
            qkv = R.slabs(inp, nslab)
            fig = assert_matches_float64(inp, qkv, step, run_layer(inp, qkv, step), what="B=%d step=%d nslab=%d" % (B, step, nslab))
            worst = {k: max(v, worst.get(k, 0)) for k, v in fig.items()}
    print("layer kernel B=%d worst: %s" % (B, worst))


def test_consecutive_calls_on_one_scratch():
    """(c) call_index 0, 1, 2 on one scratch (steps 5, 6, 7, different x): the arrival counters and claim stamps carry over, and
    every call has the bits of the same launch on a fresh scratch.  (A fresh scratch is at epoch 0: its call_index is 0.)"""
    inp = inputs(200)
    qkv = R.slabs(inp, 2)
    scratch = torch.zeros(1024, dtype=torch.int32, device=DEV)
    sk, sv = R.live_cache(inp["sk"], 5), R.live_cache(inp["sv"], 5)
    for i in range(3):
        x0 = inp["x0"] + 0.25 * i
        sk0, sv0 = sk.clone(), sv.clone()
        a = run_layer(inp, qkv * (1 + 0.5 * i), 5 + i, x0=x0, sk=sk, sv=sv, scratch=scratch, call_index=i)
        b = run_layer(inp, qkv * (1 + 0.5 * i), 5 + i, x0=x0, sk=sk0, sv=sv0)
        assert a["flags"] == 0 and b["flags"] == 0, i
        for name in ("x", "y", "o", "qc", "stats", "sk", "sv"):
            assert same_bits(a[name], b[name]), (i, name)
        assert not torch.isnan(sk[:200, :, 5 + i].float()).any()


def test_layer_kernel_at_its_lds_limit():
    """(d) layer_plan (csrc/chain.hip): the stage area is max(end1, end2, end3) with, for Wso / Wco (N = 1152, K = 768: 36 columns
    per CU padded to 40 rows, 12 k-tiles, 2 column blocks) A = 12 * 32 * 128 = 49152, W = 12 * 40 * 128 + 4096 = 65536, reduction
    scratch 8 * 2 * 4096 = 65536, and for Wcq (N = 768, K = 1152: 24 columns, 18 k-tiles, 1 block) A = 73728, W = 18 * 24 * 128 + 4096
    = 59392: end1 = 49152 + 65536 = 114688, end2 = max(73728, 65536) + 59392 = 133120, end3 = 65536 + 49152 = 114688.  The launch
    fits while ceil1024(12 * 4 * sc_stride) + 133120 <= 160 * 1024 - 512 = 163328, i.e. the score bytes <= 30208; sc_stride =
    ceil16(max(T, n_keys)) = 608 gives 29184 -> 29696 (fits), 624 gives 29952 -> 30720 (does not).  So 608 keys fit, 609 do not."""
    from dimx import lib as L
    n = 608
    inp = R.make_inputs(129, n, n, n, seed=n, device=DEV)
    qkv = R.slabs(inp, 2)
    out = run_layer(inp, qkv, n - 1)
    assert_same_as_four_launches(inp, qkv, n - 1, out)
    assert_matches_float64(inp, qkv, n - 1, out, rows=torch.tensor([0, 31, 32, 127, 128]), what="T=%d" % n)


def test_layer_kernel_refuses_what_it_cannot_run():
    """(d) one key past the LDS limit (T = 609), B = 128 (the attention would split a pair over two waves) and B = 257: an error
    before any launch, x keeps its bits"""
    from dimx import engine as E
    from dimx import lib as L
    step_d = torch.tensor([5], dtype=torch.int32, device=DEV)
    long_k = torch.zeros(inputs(129)["R"], R.H, 609, R.D, dtype=torch.bfloat16, device=DEV)
    for inp, sk, B in ((inputs(129), long_k, 129), (inputs(129), None, 128), (inputs(256), None, 257)):
        assert inp["R"] >= B
        x = inp["x0"].clone()
        sk, sv = (long_k, long_k) if sk is not None else (R.live_cache(inp["sk"], 5), R.live_cache(inp["sv"], 5))
        with pytest.raises(L.DimxError):
            E.op_layer_chain(R.slabs(inp, 1), sk, sv, inp["ck"], inp["cv"], NKEYS, inp["mask"], inp["w_so"], inp["w_cq"], inp["colsum"],
                             inp["w_co"], x, step_d, B=B)
        assert same_bits(x, inp["x0"]), B


def test_precision_guard_flag():
    """(e) seven rows whose mean is 300 at a spread of ~1.8: bf16(x) is too coarse for the deferred LayerNorm, flag bit 2"""
    inp = inputs(200)
    qkv = R.slabs(inp, 2)
    x0 = inp["x0"].clone()
    x0[:7] += 300.0
    assert run_layer(inp, qkv, 9, x0=x0)["flags"] == 4
    assert run_layer(inp, qkv, 9)["flags"] == 0


@pytest.mark.parametrize("B", [130, 200])
def test_table_form_has_the_bits_of_the_cache_form(B):
    """(f) dimx_op_layer_chain_tab: K / V of position j from row hist[b, j] of a [512 + 8, 2 * 768] bf16 table (K at 0, V at 768,
    tab_rows = 512, the 8 spare rows NaN).  History entries at and past the step hold stale ids 512..519: clamped to row 511, loaded,
    not used -- and inside the allocation even if the clamp were missing, where their NaN would reach the output."""
    inp = inputs(B)
    g = torch.Generator().manual_seed(B)
    tab = torch.randn(520, 2 * R.INNER, generator=g).bfloat16()
    tab[512:] = float("nan")
    tab = tab.to(DEV)
    hist = torch.randint(0, 512, (inp["R"], T), generator=g, dtype=torch.int32)
    hist[:, 1] = hist[:, 0]                 # a repeated id next to itself, and others by chance (72 draws of 512 per row, 200 rows)
    hist[:, 40] = hist[:, 7]
    hist = hist.to(DEV)
    kv = tab[hist.long()].view(inp["R"], T, 2, R.H, R.D)
    sk_g, sv_g = (kv[:, :, i].permute(0, 2, 1, 3).contiguous() for i in range(2))
    nan_k = torch.full_like(inp["sk"], float("nan"))
    for step in (0, 1, 33, T - 1):
        qkv = R.slabs(inp, 2)
        h = hist.clone()
        h[:, step:] = (512 + torch.arange(T - step, device=DEV) % 8).to(torch.int32)
        sk, sv = nan_k.clone(), nan_k.clone()
        a = run_layer(inp, qkv, step, sk=sk, sv=sv, tab=tab, hist=h, tab_koff=0, tab_voff=R.INNER, tab_rows=512)
        b = run_layer(inp, qkv, step, sk=R.live_cache(sk_g, step), sv=R.live_cache(sv_g, step))
        assert a["flags"] == 0 and b["flags"] == 0
        for name in ("x", "y", "o", "qc", "stats"):
            assert same_bits(a[name], b[name]), (step, name)
        assert same_bits(sk, nan_k) and same_bits(sv, nan_k), "the table form appends nothing"
