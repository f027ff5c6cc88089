"""GPU: the GEMM epilogues' output maps (csrc/gemm.hip epilogue_tile / stage_copy_out, csrc/gemm256.hip store_chunk) through
dimx_op_gemm_map, one map at a time, against tests/gemm_map_ref.py.

Every case, the same way:
  * all destinations are views into ONE allocation prefilled with the sentinel 16384.0 (exact in bf16 and f32), a guard zone of at
    least one clip (sb elements) in front of and behind every segment;
  * the route dimx_op_gemm_route reports (kernel, staged epilogue, packed V^T stores) is asserted before the launch, so that a
    later threshold change cannot turn a "staged" case into a second "direct" one unnoticed;
  * outside the map's image (guards, padding rows t in [T, Tp), columns N .. ldc) every element still holds the sentinel bit for
    bit, inside it none does;
  * without a row add the image equals, bit for bit, the plain-destination dimx_op_gemm result of the same operands / bias /
    activation / residual / forced cfg re-laid by the reference scatter (only the store address differs); with a row add of
    scale 1 into an f32 destination it equals (act(acc + bias) + row) + residual evaluated in torch f32 in the kernel's order, the
    act(acc + bias) term coming from a plain run without residual; other scales and bf16 destinations are judged by tolerance;
  * always: the float64 evaluation of the same operation on the kernel's own operands within test_gemm's tolerances
    (f32 2e-5 * max(1, sqrt(K) / 8); bf16 operands, f32 destination 2e-3; bf16 destination 0.05), and two runs bit-identical.
"""
import ctypes
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import gemm_map_ref as R

pytestmark = pytest.mark.gpu

torch.set_grad_enabled(False)

SENT = 16384.0
ACTS = {0: lambda x: x, 1: lambda x: F.leaky_relu(x, 0.2),
        2: lambda x: x * 0.5 * (1 + torch.tanh(math.sqrt(2 / math.pi) * (x + 0.044715 * x ** 3))),
        3: lambda x: F.gelu(x)}
# (id, bf16 operands, bf16 destination)
DTYPES = [("f32", False, False), ("bf16_f32", True, False), ("bf16_bf16", True, True)]
# (id, cfg, force the register-staged kernel, kernel id of the route word)
DIRECT_KERNELS = [("cfg3", 3, False, 3), ("cfg34", 34, False, 34), ("cfg1", 1, False, 1), ("simple", 0, True, 1064)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def _tol(bf16, out_bf16, K):
    return 0.05 if out_bf16 else (2e-3 if bf16 else 2e-5 * max(1.0, math.sqrt(K) / 8))


def _bits(x):
    return x.view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32)


@functools.lru_cache(maxsize=3)
def _operands(M, N, K, bf16):
    """inputs randn, weights randn / sqrt(K), bias / residual randn (the operands the kernel sees: bf16-rounded where bf16) and the
    float64 product of exactly those operands -- computed once per shape, shared by the cases of that shape, never modified"""
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(7 * M + 3 * N + K + (1 if bf16 else 0))
    a = torch.randn(M, K, device=dev, generator=g)
    w = torch.randn(N, K, device=dev, generator=g) / math.sqrt(K)
    bias = torch.randn(N, device=dev, generator=g)
    res = torch.randn(M, N, device=dev, generator=g)
    if bf16:
        a, w = a.bfloat16(), w.bfloat16()
    acc64 = a.double() @ w.double().t()
    return a, w, bias, res, acc64


def _table(dev, rows, N, seed):
    """row-add table randn [rows, N + 8]: a row stride that is not N"""
    g = torch.Generator(device=dev).manual_seed(1000 + seed)
    return torch.randn(rows, N + 8, device=dev, generator=g)


class Layout:
    """the destinations of an OutMap inside one allocation: [guard] dest 0 [guard] [guard] dest 1 [guard] ..., every destination
    starting on a multiple of 64 elements (the 16-byte alignment the model's buffers have)"""

    def __init__(self, mp, dtype, dev):
        self.mp, self.dtype, self.dev = mp, dtype, dev
        self.starts, pos = [], 0
        for size, seg in zip(mp.sizes, mp.segs):
            guard = -(-max(seg[0], 64) // 64) * 64      # at least one clip's sb
            pos += guard
            self.starts.append(pos)
            pos += -(-size // 64) * 64 + guard
        self.total = pos

    def alloc(self, dtype=None, fill=SENT):
        return torch.full((self.total,), fill, dtype=dtype or self.dtype, device=self.dev)

    def views(self, buf):
        return [buf[s + o:] for s, o in zip(self.starts, self.mp.base)]

    def segs(self, buf):
        return [(v,) + tuple(seg) for v, seg in zip(self.views(buf), self.mp.segs)]

    def place(self, values, dtype=None, fill=SENT):
        """values [M, N] laid out by the reference scatter in a fresh allocation -> (allocation, image of the map)"""
        buf = self.alloc(dtype, fill)
        imgs = R.scatter(values, self.mp.rowT, self.mp.segs, self.mp.seg_width, self.views(buf))
        image = torch.zeros(self.total, dtype=torch.bool, device=self.dev)
        for s, o, im in zip(self.starts, self.mp.base, imgs):
            assert not (image[s + o:] & im).any(), "two segments share an element"
            image[s + o:] |= im
        return buf, image


def _check(dev, mp, M, N, K, bf16, out_bf16, route, cfg=0, simple=False, act=0, use_bias=True, use_res=False, rowadd=None, tag="",
           plain_cfg=None):
    """one case; rowadd = (mode, off, div, scale) or None; route = (kernel, staged, packed or None = not asked); plain_cfg: the cfg
    of the plain run when the automatic choice of the mapped call has to be forced on it"""
    from dimx import engine as E
    a, w, bias, res, acc64 = _operands(M, N, K, bf16)
    bias_t, res_t = (bias if use_bias else None), (res if use_res else None)
    odt = torch.bfloat16 if out_bf16 else torch.float32
    lay = Layout(mp, odt, dev)
    kw = dict(rowT=mp.rowT, bias=bias_t, act=act, residual=res_t, bf16=bf16, cfg=cfg, force_simple=simple)
    plain_kw = dict(bf16=bf16, force_simple=simple, cfg=cfg if plain_cfg is None else plain_cfg)
    ref64 = ACTS[act](acc64 + bias.double() if use_bias else acc64)
    exact = None
    if rowadd is None:
        exact = E.op_gemm(a, w, bias_t, act, res_t, out_bf16=out_bf16, **plain_kw)
    else:
        mode, off, div, scale = rowadd
        rows = R.rowadd_rows(mode, off, div, mp.rowT, M).to(dev)
        # as tall as a div = 1 call would read (the model's positional tables are taller than what one call indexes)
        table = _table(dev, int(R.rowadd_rows(mode, off, 1, mp.rowT, M).max()) + 1, N, mode * 97 + off + div)
        kw.update(rowadd=table, rowadd_mode=mode, rowadd_scale=scale, rowadd_off=off, rowadd_div=div)
        ref64 = ref64 + table[rows, :N].double() * float(torch.tensor(scale, dtype=torch.float32))
        if scale == 1.0 and not out_bf16:   # the kernel's order in f32: (act(acc + bias) + row) + residual
            exact = E.op_gemm(a, w, bias_t, act, None, out_bf16=False, **plain_kw) + table[rows, :N]
            if use_res:
                exact = exact + res
    if use_res:
        ref64 = ref64 + res.double()
    # the expectation comes first: the scatter also proves that the map stays inside the allocation before anything is launched
    ref_buf, image = lay.place(ref64, torch.float64, 0.0)
    exp_buf = lay.place(exact)[0] if exact is not None else None
    buf1, buf2 = lay.alloc(), lay.alloc()
    got = E.op_gemm_route(a, w, lay.segs(buf1), **kw)
    assert got[:2] == tuple(route[:2]) and (route[2] is None or got[2] == route[2]), "%s: route %s, expected %s" % (tag, got, route)
    E.op_gemm_map(a, w, lay.segs(buf1), **kw)
    E.op_gemm_map(a, w, lay.segs(buf2), **kw)
    torch.cuda.synchronize()
    stray = _bits(buf1)[~image] != _bits(torch.full((1,), SENT, dtype=odt, device=dev))
    assert not stray.any(), "%s: %d elements outside the map's image were written" % (tag, int(stray.sum()))
    assert (buf1[image] != SENT).all(), "%s: elements of the image were not written" % tag
    err = float((buf1.double() - ref_buf)[image].abs().max())
    tol = _tol(bf16, out_bf16, K)
    nbad = -1 if exp_buf is None else int((_bits(buf1)[image] != _bits(exp_buf)[image]).sum())
    print("%s route=%s err64=%.3g tol=%.3g bit-mismatches=%d" % (tag, got, err, tol, nbad))
    if exp_buf is not None:
        assert nbad == 0, "%s: %d elements differ in bits from the plain run re-laid by the map" % (tag, nbad)
    assert err < tol, "%s: |out - float64| = %g (tolerance %g)" % (tag, err, tol)
    assert torch.equal(buf1, buf2), "%s: two runs differ" % tag


# ---------------------------------------------------------------------------------------------- A. direct generic epilogue
def _a1():
    return R.qkv_map(3, 27, 3, 48, 32, False), 81, 432, 128, dict(act=3)


def _a2():
    return R.qkv_map(2, 299, 2, 96, 304, False), 598, 576, 192, dict(use_bias=False)


def _a3():
    return R.qkv_map(7, 5, 2, 64, 8, True), 35, 384, 128, dict(act=1, use_res=True)


def _a4(M):
    return lambda: (R.decode_row_map(M, 2, 64, 16, 5), M, 384, 192, dict())


DIRECT_CASES = [("A1_qkv_vt_seg144", _a1), ("A2_qkv_vt_d96", _a2), ("A3_qkv_rowv_T5", _a3), ("A4_decode_rows_37", _a4(37)),
                ("A4_decode_rows_200", _a4(200))]


@pytest.mark.parametrize("dt", DTYPES, ids=[d[0] for d in DTYPES])
@pytest.mark.parametrize("kern", DIRECT_KERNELS, ids=[k[0] for k in DIRECT_KERNELS])
@pytest.mark.parametrize("case", DIRECT_CASES, ids=[c[0] for c in DIRECT_CASES])
def test_direct_epilogue_maps(dev, case, kern, dt):
    """A1-A4: segments that do not align with the 32 / 64-column tiles, 96-wide heads, up to six clip boundaries inside one 32-row
    slice, and the rowT == 1 fast path (interior tiles and ragged tail; cache rows other than 5 keep the sentinel)"""
    mp, M, N, K, kw = case[1]()
    _check(dev, mp, M, N, K, dt[1], dt[2], (kern[3], False, False), cfg=kern[1], simple=kern[2], tag="%s/%s/%s" % (case[0], kern[0], dt[0]), **kw)


def _rowadd_configs(N):
    """A5: (mode, off, div, scale)"""
    return [(1, 0, 1, N ** -0.5), (1, 0, 1, 1.0), (2, 1792, 1, 1.0), (2, 3, 4, 1.0), (3, 2, 1, 1.0)]


@pytest.mark.parametrize("dt", DTYPES, ids=[d[0] for d in DTYPES])
@pytest.mark.parametrize("kern", DIRECT_KERNELS, ids=[k[0] for k in DIRECT_KERNELS])
@pytest.mark.parametrize("M", [81, 130])
def test_direct_epilogue_row_adds(dev, M, kern, dt):
    """A5: the three row-add modes with off / div / scale on a plain destination (rowT = 27; M = 130 ends in a partial clip), each
    with LeakyReLU and erf-GELU, with and without residual"""
    N, K = 200, 128
    mp = R.plain_map(M, N, N + 8, rowT=27)
    for ra in _rowadd_configs(N):
        for act in (1, 3):
            for use_res in (False, True):
                _check(dev, mp, M, N, K, dt[1], dt[2], (kern[3], False, None), cfg=kern[1], simple=kern[2], act=act, use_res=use_res,
                       rowadd=ra, tag="A5/M%d/%s/%s/mode%d.off%d.div%d.scale%.3g/act%d/res%d" % ((M, kern[0], dt[0]) + ra + (act, int(use_res))))


def _headmajor(dev, bf16, B, T, Tp, N, K, nlayers, kernel, tag):
    """dimx_op_gemm_headmajor: nlayers x (K | V) head-major [B, H, Tp, 64] caches in one buffer; rows T .. Tp-1 and the guards keep
    the sentinel, the rest equals the plain run bit for bit"""
    from dimx import engine as E
    from dimx import lib as L
    lib = L.load()
    M, nseg = B * T, 2 * nlayers
    H = N // nseg // 64
    a, w, _, _, acc64 = _operands(M, N, K, bf16)
    odt = torch.bfloat16 if bf16 else torch.float32
    mp = R.cache_map(B, T, H, Tp, nseg)
    size, guard = mp.sizes[0], mp.segs[0][0]
    total = 2 * guard + nseg * size

    def place(values, dtype, fill):
        buf = torch.full((total,), fill, dtype=dtype, device=dev)
        imgs = R.scatter(values, mp.rowT, mp.segs, mp.seg_width, [buf[guard + i * size:] for i in range(nseg)])
        image = torch.zeros(total, dtype=torch.bool, device=dev)
        for i, im in enumerate(imgs):
            image[guard + i * size:] |= im
        return buf, image

    plain = E.op_gemm(a, w, bf16=bf16, out_bf16=bf16)
    ref_buf, image = place(acc64, torch.float64, 0.0)
    exp_buf = place(plain, odt, SENT)[0]
    assert int(image.sum()) == M * N
    bufs = [torch.full((total,), SENT, dtype=odt, device=dev) for _ in range(2)]
    # the entry point takes the 256 x 256 kernel when the plain probe of the same shape is eligible, else launch_gemm with the
    # two-segment map (one layer only)
    probe = Layout(R.plain_map(M, N, N), odt, dev)
    assert E.op_gemm_route(a, w, probe.segs(probe.alloc()), bf16=bf16)[0] == kernel, tag
    if nlayers == 1:
        segs = [(bufs[0][guard + i * size:],) + tuple(mp.segs[i]) for i in range(2)]
        assert E.op_gemm_route(a, w, segs, rowT=T, bf16=bf16) == (kernel, False, False), tag
    for buf in bufs:
        out = buf[guard:]
        L.check(lib.dimx_op_gemm_headmajor(L.BF16 if bf16 else L.F32, L.ptr(a), K, L.ptr(w), K, ctypes.c_void_p(out.data_ptr()), M, N, K,
                                           T, Tp, nlayers, L.stream_ptr(dev)), "dimx_op_gemm_headmajor")
    torch.cuda.synchronize()
    sent = _bits(torch.full((1,), SENT, dtype=odt, device=dev))
    assert not (_bits(bufs[0])[~image] != sent).any(), "%s: padding rows or guards were written" % tag
    assert (bufs[0][image] != SENT).all(), tag
    caches = bufs[0][guard:guard + nseg * size].view(nseg, B, H, Tp, 64)
    assert (caches[:, :, :, T:] == SENT).all(), "%s: rows T .. Tp-1 of a cache were written" % tag
    err = float((bufs[0].double() - ref_buf)[image].abs().max())
    nbad = int((_bits(bufs[0])[image] != _bits(exp_buf)[image]).sum())
    print("%s err64=%.3g bit-mismatches=%d" % (tag, err, nbad))
    assert nbad == 0, "%s: %d elements differ in bits from the plain run" % (tag, nbad)
    assert err < _tol(bf16, bf16, K), tag
    assert torch.equal(bufs[0], bufs[1]), tag


@pytest.mark.parametrize("B,T,Tp,N", [(3, 27, 32, 128), (2, 299, 304, 1536)])
def test_headmajor_f32_small(dev, B, T, Tp, N):
    """A6: the non-256 route of dimx_op_gemm_headmajor (f32, one layer)"""
    _headmajor(dev, False, B, T, Tp, N, 192, 1, 34, "A6/N%d" % N)


# ---------------------------------------------------------------------------------------------- B. staged epilogue (cfg 14, M >= 2048)
def _qkv(B, T, Tp, H=2, D=64):
    return R.qkv_map(B, T, H, D, Tp, False), B * T, 3 * H * D, 128


STAGED_CASES = [
    # id, builder -> (map, M, N, K), route (kernel, staged, packed), extra
    ("B1_T300_packed", lambda: _qkv(7, 300, 304), (14, True, True), dict(act=1)),
    ("B2_T299_unpacked", lambda: _qkv(7, 299, 304), (14, True, False), dict(act=1)),
    ("B3_Tp301_unpacked", lambda: _qkv(7, 300, 301), (14, True, False), dict()),
    ("B4a_rowT32", lambda: _qkv(65, 32, 32), (14, True, True), dict(act=3)),
    ("B4b_rowT33", lambda: _qkv(63, 33, 36), (14, True, False), dict(act=3)),
    ("B4c_rowT31_direct", lambda: _qkv(67, 31, 32), (14, False, False), dict(act=3)),
    ("B5_rowT1_mode2_div10", lambda: (R.plain_map(2050, 384, 392), 2050, 384, 128), (14, True, None),
     dict(act=2, use_res=True, rowadd=(2, 3, 10, 1.0))),
    ("B6_seg144_direct", lambda: _qkv(7, 300, 304, 3, 48), (14, False, False), dict(act=1)),
    ("B7_mode1", lambda: (R.plain_map(2100, 384, 392, rowT=300), 2100, 384, 128), (14, True, None),
     dict(act=1, use_res=True, rowadd=(1, 0, 1, 1.0))),
    ("B7_mode1_scaled", lambda: (R.plain_map(2100, 384, 392, rowT=300), 2100, 384, 128), (14, True, None),
     dict(act=3, rowadd=(1, 0, 1, 384 ** -0.5))),
    ("B7_mode2_div2", lambda: (R.plain_map(2100, 384, 392, rowT=300), 2100, 384, 128), (14, True, None),
     dict(act=3, use_res=True, rowadd=(2, 5, 2, 1.0))),
    ("B7_mode3", lambda: (R.plain_map(2100, 384, 392, rowT=300), 2100, 384, 128), (14, True, None),
     dict(use_res=True, rowadd=(3, 2, 1, 1.0))),
]


@pytest.mark.parametrize("dt", DTYPES, ids=[d[0] for d in DTYPES])
@pytest.mark.parametrize("case", STAGED_CASES, ids=[c[0] for c in STAGED_CASES])
def test_staged_epilogue_maps(dev, case, dt):
    """B1-B7: stage_copy_out's three branches (row-major pieces, packed and unpacked transposed), its admission limits rowT = 32 / 33
    (31: direct), the fall-back to the direct epilogue for a segment width that is no multiple of 32, and the row adds on
    row-contiguous pieces (rowadd_div > 1 included)"""
    (mp, M, N, K), route, kw = case[1](), case[2], case[3]
    _check(dev, mp, M, N, K, dt[1], dt[2], route, cfg=14, tag="%s/%s" % (case[0], dt[0]), **kw)


@pytest.mark.parametrize("dt,B", [(DTYPES[0], 25), (DTYPES[1], 14), (DTYPES[2], 14)], ids=["B8a_f32", "B8b_bf16_f32", "B8b_bf16_bf16"])
def test_staged_epilogue_by_automatic_choice(dev, dt, B):
    """B8: cfg 0 -- the encoder's positional GEMM (mode 1) at N 1152, K 384: f32 at 25 clips and bf16 at 14 clips (297 128 x 128
    tiles, 85 256 x 256 tiles: not the 256-tile kernel's) both take cfg 14 and the staged epilogue by themselves"""
    T, N, K = 300, 1152, 384
    mp = R.plain_map(B * T, N, N, rowT=T)
    for scale in (1.0, N ** -0.5):
        _check(dev, mp, B * T, N, K, dt[1], dt[2], (14, True, None), cfg=0, act=1, rowadd=(1, 0, 1, scale), tag="B8/%s/scale%.3g" % (dt[0], scale))


# ---------------------------------------------------------------------------------------------- C. the 256 x 256 kernel (bf16 operands)
@pytest.mark.parametrize("T", [299, 300])
def test_gemm256_three_row_major_segments(dev, T):
    """C1: the prefill q/k/v form (row-major V), bf16 destination; T = 299 is M = 5083, exactly the 100 tiles the kernel asks for"""
    B, H, D, K = 17, 8, 48, 384
    _check(dev, R.qkv_map(B, T, H, D, T, True), B * T, 3 * H * D, K, True, True, (256, False, False), act=0, tag="C1/T%d" % T)


@pytest.mark.parametrize("out_bf16", [True, False], ids=["bf16_dest", "f32_dest_residual"])
@pytest.mark.parametrize("rowT,M", [(32, 5120), (1, 5121)])
def test_gemm256_row_adds(dev, rowT, M, out_bf16):
    """C2: row-add modes 1, 2 (div 4) and 3 in the 256-tile epilogue: the unpack-add-repack branch of a bf16 destination, and an f32
    destination with residual (scale 1: bit-exact against the f32 order; scaled: tolerance)"""
    N, K = 1152, 384
    mp = R.plain_map(M, N, N, rowT=rowT)
    for ra in [(1, 0, 1, 1.0), (1, 0, 1, N ** -0.5), (2, 3, 4, 1.0), (2, 3, 4, N ** -0.5), (3, 2, 1, 1.0)]:
        _check(dev, mp, M, N, K, True, out_bf16, (256, False, None), act=3, use_res=not out_bf16, rowadd=ra,
               tag="C2/rowT%d/%s/mode%d.off%d.div%d.scale%.3g" % ((rowT, "bf16" if out_bf16 else "f32") + ra))


@pytest.mark.parametrize("nlayers", [1, 4])
def test_gemm256_head_major_caches_T299(dev, nlayers):
    """C3: head-major caches at T % 4 != 0 (T 299, Tp 304), one layer and the fused four"""
    _headmajor(dev, True, 14, 299, 304, nlayers * 1536, 384, nlayers, 256, "C3/nlayers%d" % nlayers)


@pytest.mark.parametrize("out_bf16", [True, False], ids=["bf16_dest", "f32_dest"])
@pytest.mark.parametrize("head_major", [True, False], ids=["head_major_cfg14", "row_major_gemm256"])
def test_gemm256_head_width_36(dev, head_major, out_bf16):
    """C4: 36-column heads at a shape the 256-tile kernel otherwise takes (M 5100, 100+ tiles).  Its epilogue splits (head, column)
    once per lane and reaches the other columns of the lane's piece -- 8 bf16 columns, an f32 destination's second pass 32 columns
    further -- by pointer addition.  Row-major heads lie back to back (sh == D): the address is linear in the column and the
    kernel is right.  Head-major [B, 16, Tp, 36] caches are not: bf16 columns 32..39 went to frames t and t + 1 of head 0, f32
    columns 32..63 to head 0's next frames instead of head 1 (found by this test), so gemm256_eligible now sends such heads
    (D % 8 != 0 for bf16, D % 64 != 0 for f32) to cfg 14, staged"""
    B, T, Tp, H, D, K = 17, 300, 304, 16, 36, 384
    tag = "C4/%s/%s" % ("head_major" if head_major else "row_major", "bf16" if out_bf16 else "f32")
    if head_major:
        seg = (H * Tp * D, Tp * D, D, 1, D)
        mp = R.OutMap(T, H * D, [seg, seg], [B * H * Tp * D] * 2, [0, 0])
        _check(dev, mp, B * T, 2 * H * D, K, True, out_bf16, (14, True, None), tag=tag, plain_cfg=14)
    else:
        _check(dev, R.qkv_map(B, T, H, D, T, True), B * T, 3 * H * D, K, True, out_bf16, (256, False, False), tag=tag)


# ---------------------------------------------------------------------------------------------- D. refusals
def test_cfg72_refuses_a_map_and_writes_nothing(dev):
    """the 64 x 72 decode kernel stores to plain rows only: a mapped or row-add call that forces it is an error, not a launch"""
    from dimx import engine as E
    from dimx import lib as L
    M, N, K = 64, 144, 128
    a, w, bias, _, _ = _operands(M, N, K, True)
    two = R.OutMap(1, 72, [(72, 0, 72, 1, 72)] * 2, [M * 72] * 2, [0, 0])
    for mp, kw in ((two, dict()), (R.plain_map(M, N, N), dict(rowadd=_table(dev, 1, N, 0), rowadd_mode=3))):
        for odt in (torch.float32, torch.bfloat16):
            lay = Layout(mp, odt, dev)
            buf = lay.alloc()
            with pytest.raises(L.DimxError):
                E.op_gemm_map(a, w, lay.segs(buf), bias=bias, bf16=True, cfg=72, **kw)
            with pytest.raises(L.DimxError):
                E.op_gemm_route(a, w, lay.segs(buf), bias=bias, bf16=True, cfg=72, **kw)
            torch.cuda.synchronize()
            assert torch.equal(buf, lay.alloc())
    plain = Layout(R.plain_map(M, N, N), torch.float32, dev)   # the same call without a row add is the kernel's own case
    assert E.op_gemm_route(a, w, plain.segs(plain.alloc()), bias=bias, bf16=True, cfg=72) == (72, False, False)
