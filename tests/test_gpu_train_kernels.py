"""GPU: the training kernels whose launch plan depends on the row count alone (csrc/train.hip, train_kernels.hip), each against
float64 at the smallest row counts that cross its thresholds -- through the entry points that run the step's own helpers
(dimx_op_train_layernorm_bwd / _colsum / _prep / _cross_entropy), dimx_train_adamw, and dimx_op_gemm with C == residual.

The yardstick.  Where no rigorous bound exists the bound is 8 x the error of the SAME formula evaluated in float32 by torch on
the CPU against float64 on the same inputs; the factor covers the different summation order (wave reductions, the 4-wave and
600-row finishes).  "Error" is always max |got - ref| over the tensor divided by max |ref| of the tensor, for the kernel and for
the yardstick alike.  The yardstick is never taken below 2^-24 (half a float32 ulp of the tensor's largest element): a float32
result cannot be closer to float64 than its own rounding, and on a tensor of a few elements (M = 1, the scalar loss) the CPU
evaluation is sometimes exact by luck, which would turn the bound into bit-equality with float64.

Measured on an MI355X (kernel error / yardstick, worst over the cases of each test; the bound is 8):
  LayerNorm adjoint   dx 1.04 (1.5e-7 vs 1.4e-7, M = 600), d gamma 1.62 (M = 5), d beta 2.09 (2.7e-7 vs 1.3e-7, M = 2400),
                      d gamma of a single row 2.76 (1.6e-7 against the 2^-24 floor)
  cross entropy       loss 1.67 (9.9e-8 against the 2^-24 floor; the float32 CPU loss is below the floor at every R but 5),
                      d logits 0.39 (2.3e-7 vs 5.9e-7, R = 4136)
  operand copy, f32   worst error / (8 x yardstick): mode 1 0.125, 2 0.156, 3 0.167, 4 0.125, 5 0.221 (yardsticks 6e-8 .. 1.5e-7)
  operand copy, bf16  1.000 in every mode: the half bf16 ulp of the rounding itself, the float32 part is as above
  column sums         error / rigorous bound <= 0.004
  AdamW               parameter error <= 7.5e-7 after two steps at n = 2 097 155 (bound 4e-6), norm equal to 7 digits
  in-place GEMM       3.9e-6 (f32, tolerance 4.9e-5), 1.6e-6 / 2.7e-6 (bf16 at M = 2051 / 4099, tolerance 2e-3), bits equal
"""
import ctypes
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

DEV = "cuda:0"
FACTOR = 8.0
FLOOR = 2.0 ** -24
ERR_ARG = -1


def _normal(name, shape, seed=71):
    from dimx import prng
    return torch.from_numpy(prng.normal(seed, name, shape))


def _ints(name, shape, lo, hi, seed=71):
    from dimx import prng
    return torch.from_numpy(prng.integers(seed, name, shape, lo, hi))


def _rel(got, ref):
    """max |got - ref| / max |ref| in float64 (ref on any device)"""
    ref = ref.to(got.device)
    return ((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


def _check(what, got, ref64, ref32):
    """got (device f32) against ref64 within FACTOR x the float32-CPU evaluation's own error; prints both"""
    assert torch.isfinite(got).all(), "%s: unwritten or non-finite elements" % what
    yard = max(_rel(ref32, ref64), FLOOR)
    err = _rel(got, ref64)
    print("%s: kernel %.3e, float32 CPU %.3e (ratio %.2f)" % (what, err, yard, err / yard))
    assert err <= FACTOR * yard, "%s: error %.3e > %g x %.3e" % (what, err, FACTOR, yard)
    return err / yard


# ------------------------------------------------------------------------------------------------ LayerNorm adjoint
LN_SHAPES = [(M, 384) for M in (1, 3, 4, 5, 600, 2400, 2401, 4803)] + [(M, C) for C in (512, 768, 1152) for M in (5, 2401)]


def _ln_rows(M):
    """rows per block of ln_adjoint / tr_layernorm_bwd_fused: roundup4(ceil(M / 600))"""
    return (-(-M // 600) + 3) // 4 * 4


def _ln_formula(x, gamma, dy, dx0=None):
    mean = x.mean(1, keepdim=True)
    xc = x - mean
    rstd = ((xc * xc).mean(1, keepdim=True) + 1e-5).rsqrt()
    xh = xc * rstd
    g = dy * gamma
    dx = (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True)) * rstd
    if dx0 is not None:
        dx = dx0 + dx
    return dx, (dy * xh).sum(0), dy.sum(0), xh


@functools.lru_cache(maxsize=None)
def _ln_inputs(M, C):
    x = _normal("ln.x.%d.%d" % (M, C), (M, C)) + 3.0          # row mean 3: the statistics cancel
    gamma = 1.0 + 0.25 * _normal("ln.g.%d" % C, (C,))
    dy = _normal("ln.dy.%d.%d" % (M, C), (M, C))
    dx0 = _normal("ln.dx0.%d.%d" % (M, C), (M, C))
    return x, gamma, dy, dx0


@pytest.mark.parametrize("M,C", LN_SHAPES)
def test_layernorm_adjoint_values_against_float64(M, C):
    """ln_adjoint -> tr_layernorm_bwd_fused + tr_multi_finish.  Rows per block roundup4(ceil(M / 600)): 4 up to M = 2400 (every
    wave owns at most one row of its block; M = 600: 150 partial rows), 8 at M = 2401 (a wave loops over two rows; 301 blocks,
    the last holds one row), 12 at M = 4803 (401 blocks, the last holds 3 rows); M = 1, 3, 4, 5: blocks with idle waves and a
    second block of one row.  dx per element and d gamma / d beta per column against the float64 formula, accumulate 0 and 1,
    with and without d beta; x has row mean 3."""
    from dimx import engine as E
    x, gamma, dy, dx0 = _ln_inputs(M, C)
    dev = lambda t: t.to(DEV)
    for accumulate in (0, 1):
        r64 = _ln_formula(x.double(), gamma.double(), dy.double(), dx0.double() if accumulate else None)
        r32 = _ln_formula(x, gamma, dy, dx0 if accumulate else None)
        for with_beta in (True, False):
            dx, dg, db = E.op_train_layernorm_bwd(dev(x), dev(gamma), dev(dy), dx=dev(dx0).clone() if accumulate else None,
                                                  with_beta=with_beta)
            tag = "ln adjoint M=%d C=%d acc=%d beta=%d" % (M, C, accumulate, with_beta)
            _check(tag + " dx", dx, r64[0], r32[0])
            _check(tag + " dgamma", dg, r64[1], r32[1])
            if with_beta:
                _check(tag + " dbeta", db, r64[2], r32[2])
            else:
                assert db is None


@pytest.mark.parametrize("M,C", LN_SHAPES)
def test_layernorm_adjoint_counts_every_row_once(M, C):
    """Row coverage of the same row loop, exact: dy integer-valued in [-8, 8] makes the d beta column sums exact in float32 in any
    order, so they must EQUAL the integer sums -- a dropped or doubled row (the wave's row loop at 8 / 12 rows per block, the
    ragged last block, the 600-partial-row multi_finish) fails at any M."""
    from dimx import engine as E
    x, gamma, _, _ = _ln_inputs(M, C)
    dy = _ints("ln.idy.%d.%d" % (M, C), (M, C), -8, 9)
    dx, dg, db = E.op_train_layernorm_bwd(x.to(DEV), gamma.to(DEV), dy.float().to(DEV))
    assert torch.equal(db.cpu(), dy.sum(0).float())
    assert torch.isfinite(dx).all() and torch.isfinite(dg).all()


@pytest.mark.parametrize("M,C", LN_SHAPES)
def test_layernorm_adjoint_dgamma_takes_each_row_from_its_own_block(M, C):
    """d gamma with dy zero except one row r must be dy_r o xhat_r: r = 0, rows - 1, rows (the first row of the second block), M - 1
    and the first row of the last block, rows = the per-block count."""
    from dimx import engine as E
    x, gamma, dy, _ = _ln_inputs(M, C)
    rows = _ln_rows(M)
    picks = sorted({r for r in (0, rows - 1, rows, M - 1, (M - 1) // rows * rows) if 0 <= r < M})
    xh64, xh32 = _ln_formula(x.double(), gamma.double(), dy.double())[3], _ln_formula(x, gamma, dy)[3]
    xd, gd = x.to(DEV), gamma.to(DEV)
    for r in picks:
        one = torch.zeros(M, C)
        one[r] = dy[r]
        _, dg, db = E.op_train_layernorm_bwd(xd, gd, one.to(DEV))
        _check("ln adjoint M=%d C=%d one-hot row %d dgamma" % (M, C, r), dg, dy[r].double() * xh64[r], dy[r] * xh32[r])
        assert torch.equal(db.cpu(), dy[r])


# ------------------------------------------------------------------------------------------------ column sums
@pytest.mark.parametrize("C", [56, 72, 4608])
@pytest.mark.parametrize("M", [1, 255, 256, 257, 4803])
def test_column_sums_across_the_slab_threshold(M, C):
    """bias_adjoint -> tr_colsum_partial + tr_multi_finish: 1 slab below 256 rows (M = 1, 255), 32 slabs from 256 up (M = 256: 8 rows
    per slab, 257: 9 rows, slab 28 short and slabs 29-31 empty, 4803: 151 rows, last slab 122).  C = 72: a second column block with 8 live lanes;
    C = 56: one partial block.  Integer dy: exact.  Random dy against float64 within (M + 4) 2^-24 sum_m |dy| per column --
    rigorous for any summation order (M - 1 additions + the finishes, each relative 2^-24).  (tr_colsums, the two-launch form with
    the same slab rule, has no caller left; ln_colsums_kernel, which both launch, runs here.)"""
    from dimx import engine as E
    idy = _ints("cs.idy.%d.%d" % (M, C), (M, C), -8, 9)
    assert torch.equal(E.op_train_colsum(idy.float().to(DEV)).cpu(), idy.sum(0).float())
    dy = _normal("cs.dy.%d.%d" % (M, C), (M, C))
    got = E.op_train_colsum(dy.to(DEV)).cpu()
    ref = dy.double().sum(0)
    bound = (M + 4) * 2.0 ** -24 * dy.double().abs().sum(0)
    excess = ((got.double() - ref).abs() / bound).max().item()
    print("colsum M=%d C=%d: worst error / rigorous bound %.3f" % (M, C, excess))
    assert torch.isfinite(got).all() and excess <= 1.0


# ------------------------------------------------------------------------------------------------ operand copy
PREP_ROWS, PREP_COLS = (1, 31, 32, 33, 94, 4803), (56, 384, 1152, 4608)
PREP_SHAPES = sorted({(r, c) for r in PREP_ROWS for c in (56, 1152)} | {(r, c) for r in (94, 4803) for c in PREP_COLS})
_C0, _C1 = 0.7978845608028654, 0.044715


def _prep_formula(mode, x, z, gamma, beta):
    """what tr_prep_fused casts, in the dtype of its arguments (modes as in include/dimx.h)"""
    if mode == 0:
        return x
    if mode == 1:
        return 0.5 * x * (1.0 + torch.erf(x * 0.7071067811865476))
    if mode == 2:
        mean = x.mean(1, keepdim=True)
        xc = x - mean
        return xc * ((xc * xc).mean(1, keepdim=True) + 1e-5).rsqrt() * gamma + beta
    if mode == 3:
        return x * (0.5 * (1.0 + torch.erf(z * 0.7071067811865476)) + z * 0.3989422804014327 * torch.exp(-0.5 * z * z))
    if mode == 4:
        return 0.5 * x * (1.0 + torch.tanh(_C0 * (x + _C1 * x * x * x)))
    th = torch.tanh(_C0 * (z + _C1 * z * z * z))
    return x * (0.5 * (1.0 + th) + 0.5 * z * (1.0 - th * th) * _C0 * (1.0 + 3.0 * _C1 * z * z))


@functools.lru_cache(maxsize=1)
def _prep_case(rows, cols):
    """inputs and, per mode, (float64 reference on the device, absolute yardstick) -- computed once per shape, shared by both
    operand types"""
    x = _normal("prep.x.%d.%d" % (rows, cols), (rows, cols)) + 0.5
    z = x.flip(0).flip(1).contiguous() * 1.25 - 0.3            # the pre-activation of modes 3 / 5: another arrangement of the stream
    gamma = 1.0 + 0.25 * _normal("prep.g.%d" % cols, (cols,))
    beta = 0.5 * _normal("prep.b.%d" % cols, (cols,))
    refs = {}
    for mode in range(1, 6):
        r64 = _prep_formula(mode, x.double(), z.double(), gamma.double(), beta.double())
        r32 = _prep_formula(mode, x, z, gamma, beta)
        scale = r64.abs().max().item()
        yard = max(((r32.double() - r64).abs().max() / scale).item(), FLOOR)
        refs[mode] = (r64.to(DEV), yard, scale)
    return x.to(DEV), z.to(DEV), gamma.to(DEV), beta.to(DEV), refs


def _bf16_half_ulp(ref):
    """half a bf16 ulp (8 significant bits) of |ref|, 0 at 0"""
    _, e = torch.frexp(ref.abs())
    return torch.where(ref == 0, torch.zeros_like(ref), torch.ldexp(torch.full_like(ref, 0.5), e - 8))


def _assert_padding_is_plus_zero(what, o, t, rows, cols):
    """every padding element of o [rows,Kp] (columns cols..Kp) and t [cols,Mp] (columns rows..Mp) is +0 bit for bit: they enter the
    GEMM contraction"""
    bits = torch.int16 if o.dtype == torch.bfloat16 else torch.int32
    assert not o[:, cols:].contiguous().view(bits).any(), "%s: padding columns of o" % what
    assert not t[:, rows:].contiguous().view(bits).any(), "%s: padding rows of the transposed copy" % what


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("rows,cols", PREP_SHAPES)
def test_operand_copy_modes_against_float64_and_exact_zero_padding(rows, cols, bf16):
    """tr_prep_fused as fwd_operands / lin_bwd call it, Kp / Mp padded to the operand type's k-tile (64 bf16, 32 f32), grid.x =
    Mp / 32.  rows 1, 31, 32, 33: one row block, ragged and full, and a second one of one row; rows 94 in bf16: Mp = 128, the fourth
    row block lies wholly past the data; rows 4803: 151 (f32) / 152 (bf16) row blocks.  cols 56: Kp = 64 > cols; column chunk from
    Kp (Mp / 32) / 512: 64 at 94 x 4608 and below, 256 at 4803 x 1152 (f32: Kp (Mp / 32) / 512 = 340) with a 128-wide last chunk,
    128 for the LayerNorm mode at few rows.  Mode 0: bit-equal to the source / its round-to-nearest-even bf16.  Modes 1, 3, 4, 5
    (erf / tanh GELU, their derivatives times dy) and 2 (LayerNorm gamma + beta): float64, 8 x the float32-CPU error (+ half a
    bf16 ulp of the reference).  Padding exact +0 in every mode."""
    from dimx import engine as E
    x, z, gamma, beta, refs = _prep_case(rows, cols)
    cast = (lambda v: v.bfloat16()) if bf16 else (lambda v: v)
    o, t, _ = E.op_train_prep(x, 0, bf16)
    assert torch.equal(o[:, :cols], cast(x)) and torch.equal(t[:, :rows], cast(x).t())
    _assert_padding_is_plus_zero("mode 0", o, t, rows, cols)
    for mode in range(1, 6):
        o, t, _ = E.op_train_prep(x, mode, bf16, src2=z if mode in (3, 5) else None, gamma=gamma if mode == 2 else None,
                                  beta=beta if mode == 2 else None)
        what = "prep %dx%d %s mode %d" % (rows, cols, "bf16" if bf16 else "f32", mode)
        _assert_padding_is_plus_zero(what, o, t, rows, cols)
        r64, yard, scale = refs[mode]
        tol = FACTOR * yard * scale + (_bf16_half_ulp(r64) if bf16 else 0.0)
        for name, got in (("o", o[:, :cols]), ("t", t[:, :rows].t())):
            assert torch.isfinite(got).all(), what
            diff = (got.double() - r64).abs()
            worst = (diff / tol).max().item() if bf16 else (diff.max() / (FACTOR * yard * scale)).item()
            print("%s %s: worst error / bound %.3f (float32 CPU yardstick %.3e)" % (what, name, worst, yard))
            assert worst <= 1.0, (what, name, worst)
        assert torch.equal(o[:, :cols], t[:, :rows].t())          # both copies hold the same cast values


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("rows,cols", PREP_SHAPES)
def test_operand_copy_partial_column_sums_hold_their_32_rows_only(rows, cols, bf16):
    """colpart as lin_bwd takes the bias gradient from the copy's pass: n_part == ceil(rows / 32) rows (one fewer than grid.x when
    the operand type pads a whole row block: rows 94 / 33 / 1 in bf16), partial row i the exact sum of rows 32 i .. 32 i + 31 of
    an integer-valued source, hence the partial rows sum to the column sums."""
    from dimx import engine as E
    src = _ints("prep.int.%d.%d" % (rows, cols), (rows, cols), -8, 9).float()
    o, t, part = E.op_train_prep(src.to(DEV), 0, bf16, colpart=True)
    n_part = -(-rows // 32)
    assert part.shape == (n_part, cols)
    want = torch.stack([src[32 * i:32 * i + 32].sum(0) for i in range(n_part)])
    assert torch.equal(part.cpu(), want) and torch.equal(part.sum(0).cpu(), src.sum(0))
    assert torch.equal(o[:, :cols].float().cpu(), src)
    _assert_padding_is_plus_zero("colpart", o, t, rows, cols)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("mode", range(6))
def test_operand_copy_of_a_strided_source(mode, bf16):
    """lds > cols: the q third of a fused q / k / v buffer [94, 3 x 384] (and a pre-activation that lies the same way) gives the
    bits of the same call on a contiguous copy; the k / v columns beside it are NaN and must not be read."""
    from dimx import engine as E
    rows, cols = 94, 384
    x, z, gamma, beta, _ = _prep_case(rows, cols)
    wide = lambda v: torch.cat([v, torch.full((rows, 2 * cols), float("nan"), device=DEV)], 1)[:, :cols]
    kw = dict(src2=z if mode in (3, 5) else None, gamma=gamma if mode == 2 else None, beta=beta if mode == 2 else None, colpart=True)
    o0, t0, p0 = E.op_train_prep(x, mode, bf16, **kw)
    xs = wide(x)
    assert xs.stride(0) == 3 * cols and not xs.is_contiguous()
    if kw["src2"] is not None:
        kw["src2"] = wide(z)
    o1, t1, p1 = E.op_train_prep(xs, mode, bf16, **kw)
    assert torch.isfinite(o1.float()).all() and torch.equal(o0, o1) and torch.equal(t0, t1) and torch.equal(p0, p1)


# ------------------------------------------------------------------------------------------------ cross entropy
def _ce_formula(logits, targets):
    valid = (targets >= 0) & (targets < 512)
    count = max(int(valid.sum()), 1)
    lse = torch.logsumexp(logits, 1)
    tgt = targets.clamp(0, 511)
    row = torch.where(valid, lse - logits.gather(1, tgt[:, None])[:, 0], torch.zeros_like(lse))
    p = torch.exp(logits - lse[:, None])
    p = p - torch.nn.functional.one_hot(tgt, 512).to(p.dtype)
    d = torch.where(valid[:, None], p / count, torch.zeros_like(p))
    return row.sum() / count, 1.0 / count, d


@pytest.mark.parametrize("R", [1, 3, 4, 5, 257, 4136])
def test_cross_entropy_against_float64(R):
    """tr_cross_entropy: ce_fwd_bwd_kernel has one wave per row, four rows per block (R = 1, 3, 4, 5: a ragged block, a full one, a
    second block of one row); the single-block ce_count_kernel / sum_scale_kernel loop over all rows from R > 256 (257: one
    thread takes two rows; 4136 = the decoder rows of the B = 88 step).  Targets: valid codes mixed with -100."""
    from dimx import engine as E
    logits = 3.0 * _normal("ce.logits.%d" % R, (R, 512))
    targets = _ints("ce.t.%d" % R, (R,), 0, 512)
    ignore = _ints("ce.ignore.%d" % R, (R,), 0, 4) == 0
    ignore[0] = False
    targets = torch.where(ignore, torch.full_like(targets, -100), targets)
    loss, inv, d = E.op_train_cross_entropy(logits.to(DEV), targets.to(DEV))
    l64, i64, d64 = _ce_formula(logits.double(), targets)
    l32, _, d32 = _ce_formula(logits, targets)
    _check("cross entropy R=%d loss" % R, loss.reshape(1), l64.reshape(1), l32.reshape(1))
    _check("cross entropy R=%d dlogits" % R, d, d64, d32)
    assert abs(inv.item() - i64) <= 2.0 ** -24 * i64
    assert not d[ignore.to(DEV)].any(), "rows with an ignored target have exactly zero d logits"


def test_cross_entropy_with_every_target_ignored_is_zero():
    """no valid target: the count is clamped to 1 (the kernel's documented clamp), loss 0 and d logits 0 exactly"""
    from dimx import engine as E
    R = 5
    logits = 3.0 * _normal("ce.logits.allignored", (R, 512))
    loss, inv, d = E.op_train_cross_entropy(logits.to(DEV), torch.full((R,), -100, dtype=torch.int64, device=DEV))
    assert loss.item() == 0.0 and inv.item() == 1.0 and not d.any() and torch.isfinite(d).all()


# ------------------------------------------------------------------------------------------------ AdamW and the norm
ADAM = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=1e-2)


def _adamw64(p, g, m, v, step, max_norm):
    """clip_grad_norm_(max_norm) + torch.optim.AdamW restated in float64"""
    norm = g.pow(2).sum().sqrt().item()
    if max_norm > 0:
        g = g * min(1.0, max_norm / (norm + 1e-6))
    p = p * (1.0 - ADAM["lr"] * ADAM["wd"])
    m = ADAM["b1"] * m + (1.0 - ADAM["b1"]) * g
    v = ADAM["b2"] * v + (1.0 - ADAM["b2"]) * g * g
    bc1, bc2 = 1.0 - ADAM["b1"] ** step, 1.0 - ADAM["b2"] ** step
    p = p - ADAM["lr"] / bc1 * m / (v.sqrt() / math.sqrt(bc2) + ADAM["eps"])
    return p, m, v, norm


def _adamw_call(p, g, m, v, step, max_norm, scratch):
    from dimx import lib as L
    raw = lambda t: ctypes.c_void_p(t.data_ptr())
    return L.load().dimx_train_adamw(raw(p), raw(g), raw(m), raw(v), p.numel(), ADAM["lr"], ADAM["b1"], ADAM["b2"], ADAM["eps"], ADAM["wd"],
                                     step, float(max_norm), raw(scratch), L.stream_ptr(p.device))


@pytest.mark.parametrize("max_norm", [1.0, 0.0])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 1023, 1025, 2097155])
def test_adamw_and_the_gradient_norm_against_float64(n, max_norm):
    """sumsq_partial_kernel / adamw_kernel: n = 1, 2, 3 only the scalar tail (n % 4 != 0), 4 one float4, 5 both, 1023 / 1025 the
    remainder loop, 2 097 155 = 4 x 524 288 + 3 > 1.57 M: the 4-way unrolled loop (512 blocks x 256 threads x 4 float4 in flight),
    the remainder loop and the scalar tail.  Two steps (the second with moments in use) against clip_grad_norm_ + AdamW in float64:
    norm 1e-5 relative, parameters 2e-6 / 4e-6 at lr 1e-3 (the bounds of test_gpu_train_hip.py)."""
    from dimx import lib as L
    p0 = _normal("adam.p.%d" % n, (n,))
    grads = [_normal("adam.g%d.%d" % (i, n), (n,)) * (0.02 if i else 3.0) for i in range(2)]     # norm above and (for small n) below 1
    p, m, v = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    p64, m64, v64 = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    scratch = torch.full((1026,), float("nan"), device=DEV)
    for step, tol in ((1, 2e-6), (2, 4e-6)):
        g = grads[step - 1]
        L.check(_adamw_call(p, g.to(DEV), m, v, step, max_norm, scratch), "dimx_train_adamw")
        p64, m64, v64, norm64 = _adamw64(p64, g.double(), m64, v64, step, max_norm)
        norm, coef = scratch[1024].item(), scratch[1025].item()
        err = (p.cpu().double() - p64).abs().max().item()
        print("adamw n=%d max_norm=%g step %d: norm %.7g (float64 %.7g), clip %.6g, max parameter error %.2e" % (n, max_norm, step, norm, norm64, coef, err))
        assert abs(norm - norm64) <= 1e-5 * norm64
        assert coef == 1.0 if max_norm == 0 else abs(coef - min(1.0, max_norm / (norm64 + 1e-6))) <= 1e-5
        assert err <= tol
        # the moments of every element, tails included (1e-4: the kernel's 1 - beta2 is float32 arithmetic, 1.3e-5 from 0.001)
        assert (m.cpu().double() - m64).abs().max().item() <= 1e-4 * m64.abs().max().item()
        assert (v.cpu().double() - v64).abs().max().item() <= 1e-4 * v64.abs().max().item()


@pytest.mark.parametrize("which", ["params", "exp_avg", "exp_avg_sq"])
def test_adamw_refuses_a_misaligned_arena_before_any_launch(which):
    """adamw_kernel reads params, grads, exp_avg and exp_avg_sq as float4: a view offset by one float is DIMX_ERR_ARG, the arenas and
    the scratch (which the norm kernels would have written first) are unchanged."""
    n = 1025
    arenas = {k: _normal("adam.mis.%s" % k, (n + 4,)).to(DEV) for k in ("params", "grads", "exp_avg", "exp_avg_sq")}
    arenas["exp_avg_sq"].abs_()
    before = {k: t.clone() for k, t in arenas.items()}
    scratch = torch.full((1026,), float("nan"), device=DEV)
    views = {k: t[1:1 + n] if k == which else t[:n] for k, t in arenas.items()}
    assert views[which].data_ptr() % 16 == 4
    rc = _adamw_call(views["params"], views["grads"], views["exp_avg"], views["exp_avg_sq"], 1, 1.0, scratch)
    torch.cuda.synchronize()
    assert rc == ERR_ARG
    assert all(torch.equal(arenas[k], before[k]) for k in arenas) and torch.isnan(scratch).all()


# ------------------------------------------------------------------------------------------------ in-place residual GEMM
@pytest.mark.parametrize("M,N,K,bf16", [(2051, 1152, 384, False), (2051, 1152, 384, True), (4099, 2304, 1152, True)],
                         ids=["f32-2051", "bf16-2051", "bf16-4099-gemm256"])
def test_gemm_accumulates_onto_its_own_output_through_the_large_row_epilogues(M, N, K, bf16):
    """launch_gemm as the training step hands it a residual that IS the output (gemm_f32(..., accumulate_dx ? dx : nullptr), the
    residual stream): from M >= 2048 the output leaves through the staged epilogue (M = 2051: a ragged last row tile), from
    M >= 4096 bf16 takes gemm256 (M = 4099).  engine.op_gemm always allocates a fresh output, so dimx_op_gemm is called directly
    with C == residual: float64 on the rounded operands at test_gemm's tolerances, and the bits of the same call with a separate
    output buffer."""
    from dimx import lib as L
    lib = L.load()
    dt = torch.bfloat16 if bf16 else torch.float32
    a = _normal("ipg.a.%d.%d" % (M, K), (M, K)).to(DEV).to(dt)
    w = (_normal("ipg.w.%d.%d" % (N, K), (N, K)) / math.sqrt(K)).to(DEV).to(dt)
    res = _normal("ipg.r.%d.%d" % (M, N), (M, N)).to(DEV)
    code = L.BF16 if bf16 else L.F32

    def gemm(out, residual):
        L.check(lib.dimx_op_gemm(code, L.F32, L.ptr(a), K, L.ptr(w), K, L.ptr(out), N, M, N, K, None, 0, L.ptr(residual), N, 0, None, 0,
                                 L.stream_ptr(a.device)), "dimx_op_gemm")
    separate = torch.full((M, N), float("nan"), device=DEV)
    gemm(separate, res)
    inplace = res.clone()
    gemm(inplace, inplace)
    ref = a.double() @ w.double().t() + res.double()
    err = (inplace.double() - ref).abs().max().item()
    tol = 2e-3 if bf16 else 2e-5 * max(1.0, math.sqrt(K) / 8)
    print("in-place gemm M=%d N=%d K=%d %s: max error %.3e (tolerance %.1e)" % (M, N, K, "bf16" if bf16 else "f32", err, tol))
    assert torch.isfinite(inplace).all() and err < tol
    assert torch.equal(inplace, separate)
