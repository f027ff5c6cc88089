"""FP8 cross-attention K/V for generation: the definition (numpy, no GPU).

The cross K/V cache of a generation is written once per clip and read by every decode step.  ``quantize`` states how a cache row
[64] becomes 64 OCP ``e4m3fn`` codes and one float32 scale -- one scale per (clip, head, key) -- and ``attention`` what the decode
step's one-query cross attention computes over such codes.  csrc/decode_attn_kv8.hip follows this file bit for bit (codes, scales)
or within the step kernels' tolerance (attention); tests/test_kv8_host.py pins the rounding against torch's CPU ``float8_e4m3fn``
cast.  ``self_step`` is the same for the self-attention caches (dimx_set_self_kv8): the caches that grow by one row per decode step,
whose new row is quantised by the step itself.  ``attention_rows`` is ``attention`` for best-of-N generation (dimx_set_cross_kv8_samples):
several query rows per clip over that clip's codes; ``round_bf16`` and ``pv_abs`` state what its matrix-core form rounds and how far
that can move an output element.  ``append`` is ``quantize`` for the rows a streaming session's push adds (dimx_stream_set_kv8).
``reorder`` is what a beam step does to the self caches' codes and scales (dimx_set_beam_kv8): a permutation by parent hypothesis.

    amax = max |x| over the row (float32)
    scale = float32(amax) / float32(448)              one IEEE float32 division; amax < 2**-60: a zero row, scale 0, codes 0
    y     = clamp(float32(x) / scale, -448, 448)      IEEE float32 division
    code  = e4m3fn(y), round to nearest even, subnormals included (spacing 2**-9 below 2**-6)

Codes 0x00 and 0x80 are interchangeable wherever a value rounds to zero.  Non-finite inputs are outside the contract.  The format
is OCP e4m3fn (bias 7, no infinities, 0x7F / 0xFF NaN, largest finite 448) -- what gfx950 converts in hardware -- not MI300's fnuz.
"""
import numpy as np

FP8_MAX = np.float32(448.0)
ZERO_ROW = np.float32(2.0 ** -60)
NEG = -float(np.finfo(np.float32).max)   # a masked key's score (the model's mask value)


def _decode_table():
    t = np.zeros(256, dtype=np.float32)
    for c in range(256):
        e, m = (c >> 3) & 15, c & 7
        if e == 15 and m == 7:
            v = np.nan
        elif e == 0:
            v = m * 2.0 ** -9
        else:
            v = (1.0 + m / 8.0) * 2.0 ** (e - 7)
        t[c] = -v if c & 0x80 else v
    return t


DECODE = _decode_table()
_POS = DECODE[:0x7F].copy()   # the 127 non-negative finite values, ascending: index = code


def decode(codes):
    """uint8 codes -> float32 values (0x7F / 0xFF: NaN)"""
    return DECODE[np.asarray(codes, dtype=np.uint8)]


def encode(y):
    """float32 values in [-448, 448] -> e4m3fn codes, round to nearest even (negative values that round to zero give 0x80)"""
    y = np.asarray(y, dtype=np.float32)
    a = np.abs(y).astype(np.float64)
    assert np.all(a <= 448.0), "encode: values outside +-448 (or not finite)"
    _, ex = np.frexp(a)                          # a = f * 2**ex, f in [0.5, 1)
    e = np.maximum(ex - 1, -6)                   # the binade, subnormals share the first normal binade's spacing
    sp = np.exp2((e - 3).astype(np.float64))
    r = np.rint(a / sp) * sp                     # power-of-two scaling is exact; rint rounds half to even
    code = np.searchsorted(_POS.astype(np.float64), r).astype(np.uint8)
    assert np.array_equal(_POS[code].astype(np.float64), r)
    return np.where(np.signbit(y), code | np.uint8(0x80), code).astype(np.uint8)


def quantize(rows):
    """rows [..., 64] float -> (codes uint8 [..., 64], scale float32 [...])"""
    x = np.asarray(rows).astype(np.float32)
    assert x.shape[-1] == 64, "quantize: rows of 64 elements"
    amax = np.max(np.abs(x), axis=-1).astype(np.float32)
    zero = amax < ZERO_ROW
    scale = np.where(zero, np.float32(0), amax / FP8_MAX).astype(np.float32)
    div = np.where(zero, np.float32(1), scale).astype(np.float32)
    y = (x / div[..., None]).astype(np.float32)
    y = np.clip(y, -FP8_MAX, FP8_MAX)
    codes = encode(y)
    codes = np.where(zero[..., None], np.uint8(0), codes).astype(np.uint8)
    return codes, scale


def append(kcodes, kscale, rows, n0):
    """The incremental quantiser (a streaming session under dimx_stream_set_kv8; kv8_append_kernel): ``quantize(rows)`` placed at
    positions [n0, n0 + c) of the second-to-last axis of the codes and the last axis of the scales.

    kcodes [..., Tp, 64] uint8, kscale [..., Tp] float32, rows [..., c, 64].  Returns the two arrays (copies; the arguments are
    left as they are) with every other position unchanged.

    Row locality: ``quantize`` gives every row its own scale, so the codes and the scale of cache row j are a function of row j
    alone.  Quantising the c rows a push appends therefore writes the bits that quantising the finished cache would write at those
    positions, whatever the chunking; and because the decode step under the window reads rows below its bound only, and those rows
    never change after they are written, a session's buffer equals the offline buffer on equal rows."""
    rows = np.asarray(rows)
    c = rows.shape[-2]
    kcodes, kscale = np.array(kcodes, dtype=np.uint8), np.array(kscale, dtype=np.float32)
    assert n0 >= 0 and n0 + c <= kcodes.shape[-2] == kscale.shape[-1], "append: rows [n0, n0 + c) inside the planes"
    codes, scale = quantize(rows)
    kcodes[..., n0:n0 + c, :] = codes
    kscale[..., n0:n0 + c] = scale
    return kcodes, kscale


def dequantize(codes, scale):
    """float32(decode(code)) * scale -> float32 [..., 64]"""
    return (decode(codes) * np.asarray(scale, dtype=np.float32)[..., None]).astype(np.float32)


def same_codes(a, b):
    """codes equal except 0x00 / 0x80"""
    a, b = np.asarray(a, dtype=np.uint8), np.asarray(b, dtype=np.uint8)
    return (a == b) | (((a | b) & 0x7F) == 0)


def attention(q, kcodes, kscale, vcodes, vscale, mask, n, scale=0.125):
    """The one-query cross attention over the dequantised rows, in float64, with dimx_op_decode_attn_ex's conventions.

    q [B, H, 64]; kcodes / vcodes [B, H, Tp, 64] uint8; kscale / vscale [B, H, Tp] float32; mask [B, >= n] (0 = masked) or None;
    keys 0 .. n - 1.  Scores are scale * q.k, a masked key scores -FLT_MAX, so a row with every key masked is the mean of V over
    the n keys.  -> [B, H, 64] float64."""
    q = np.asarray(q, dtype=np.float64)
    k = dequantize(np.asarray(kcodes)[:, :, :n], np.asarray(kscale)[:, :, :n]).astype(np.float64)
    v = dequantize(np.asarray(vcodes)[:, :, :n], np.asarray(vscale)[:, :, :n]).astype(np.float64)
    s = np.einsum("bhd,bhjd->bhj", q, k) * float(scale)
    if mask is not None:
        dead = np.asarray(mask)[:, None, :n] == 0
        s = np.where(dead, NEG, s)
    s = s - s.max(-1, keepdims=True)
    p = np.exp(s)
    p = p / p.sum(-1, keepdims=True)
    return np.einsum("bhj,bhjd->bhd", p, v)


def _rows_softmax(q, kcodes, kscale, vcodes, vscale, mask, n, S, scale):
    """attention's softmax for S rows per clip: p [B, S, H, n] float64 (rows sum to 1) and the dequantised V [B, H, n, 64] float64"""
    B = np.asarray(kcodes).shape[0]
    q = np.asarray(q, dtype=np.float64)
    assert q.shape[0] == B * S, "q holds rows_per_clip rows per clip"
    q = q.reshape((B, S) + q.shape[1:])
    k = dequantize(np.asarray(kcodes)[:, :, :n], np.asarray(kscale)[:, :, :n]).astype(np.float64)
    v = dequantize(np.asarray(vcodes)[:, :, :n], np.asarray(vscale)[:, :, :n]).astype(np.float64)
    s = np.einsum("bshd,bhjd->bshj", q, k) * float(scale)
    if mask is not None:
        s = np.where(np.asarray(mask)[:, None, None, :n] == 0, NEG, s)
    p = np.exp(s - s.max(-1, keepdims=True))
    return p / p.sum(-1, keepdims=True), v


def attention_rows(q, kcodes, kscale, vcodes, vscale, mask, n, rows_per_clip, scale=0.125):
    """The multi-query form (best-of-N generation; decode_attn_mq_kv8_kernel): ``attention`` per row, with the row's clip's codes.

    q [B * S, H, 64] with S = rows_per_clip: rows b*S .. b*S+S-1 share clip b's codes, scales and mask row.  -> [B * S, H, 64]
    float64.  The exact form of the kernel computes this within the step kernels' f32 tolerance; the matrix-core form computes it
    at ``round_bf16(q)`` with p * vscale rounded to bf16 (``pv_abs`` bounds what that rounding moves)."""
    p, v = _rows_softmax(q, kcodes, kscale, vcodes, vscale, mask, n, int(rows_per_clip), scale)
    return np.einsum("bshj,bhjd->bshd", p, v).reshape((-1,) + v.shape[1:2] + (64,))


def round_bf16(x):
    """float32 values rounded to bfloat16 (round to nearest even), as float32: what the matrix-core form makes of q"""
    u = np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def pv_abs(q, kcodes, kscale, vcodes, vscale, mask, n, rows_per_clip, scale=0.125):
    """A = sum_j p_j |v_j| / sum_j p_j of ``attention_rows``' softmax, float64 [B * S, H, 64]: the absolute mass of an output
    element.  Rounding every p_j * vscale_j to bf16 (unit roundoff 2**-8) moves the element by at most 2**-8 * A."""
    p, v = _rows_softmax(q, kcodes, kscale, vcodes, vscale, mask, n, int(rows_per_clip), scale)
    return np.einsum("bshj,bhjd->bshd", p, np.abs(v)).reshape((-1,) + v.shape[1:2] + (64,))


def self_step(q, k_new, v_new, kcodes, kscale, vcodes, vscale, n, scale=0.125):
    """One decode step's self attention over FP8 self caches (dimx_set_self_kv8; decode_attn_self_kv8_kernel), in place.

    q, k_new, v_new [R, H, 64]: the float32 sum of the projection's split-K slabs in slab order, in both numeric modes -- never
    rounded to the cache type.  kcodes / vcodes [R, H, Tp, 64] uint8 and kscale / vscale [R, H, Tp] float32 hold the rows 0 .. n - 1.
    The new rows go through ``quantize`` and are stored at position n; the result is the float64 softmax attention (scores
    scale * q.k, no key mask: the self form has none) over the dequantised rows 0 .. n, all n + 1 of them.

    The step's own key and value are the DEQUANTISED ones: the own key carries the same quantisation error as every other key.
    The output of step t is therefore a function of the buffer's rows <= t alone, and a teacher-forced replay over a finished
    buffer reproduces every step.  Rows past n are neither read nor written.  -> [R, H, 64] float64."""
    kc, ksc = quantize(np.asarray(k_new, dtype=np.float32))
    vc, vsc = quantize(np.asarray(v_new, dtype=np.float32))
    kcodes[:, :, n], kscale[:, :, n] = kc, ksc
    vcodes[:, :, n], vscale[:, :, n] = vc, vsc
    return attention(q, kcodes, kscale, vcodes, vscale, None, n + 1, scale)


def reorder(codes, scale, parent, c, W):
    """Beam search over FP8 self caches (dimx_set_beam_kv8; beam_reorder_kv8_kernel): what a beam step's reorder does to one code
    plane and its scale plane.

    codes [R, H, Tp, 64] uint8, scale [R, H, Tp] float32, parent [R] (the step's parent beams, counted within the clip), rows
    clip * W + w the W hypotheses of a clip.  Row clip * W + w takes the positions 0 .. c of row clip * W + parent[w], codes and scale
    together; positions > c are unchanged; a clip is untouched if its parents are the identity or if any of them lies outside
    [0, W).  Returns the two arrays (copies; the arguments are left as they are).

    It is a pure permutation of (codes, scale) pairs, so ``dequantize(reorder(x)) == reorder(dequantize(x))`` bit for bit: after the
    step a hypothesis's buffer rows ARE its ancestor's, and ``self_step`` on them is what ``self_step`` on the ancestor's buffer
    is.  That is the whole reason beam search over FP8 caches needs no definition beyond dimx.beam (the search) plus ``self_step``
    (the attention): nothing is re-quantised, no scale is recomputed, and no value is ever formed from the moved bits."""
    codes, scale = np.array(codes, dtype=np.uint8, order="C"), np.array(scale, dtype=np.float32, order="C")
    parent = np.asarray(parent).astype(np.int64).reshape(-1)
    R, W, c = codes.shape[0], int(W), int(c)
    assert W >= 1 and R % W == 0 and parent.shape[0] == R and scale.shape == codes.shape[:3], "reorder: R rows of W per clip"
    assert 0 <= c < codes.shape[2], "reorder: c inside the planes"
    src_c, src_s = codes.copy(), scale.view(np.uint32).copy()   # the scales as bits: a NaN payload moves unchanged
    out_s = scale.view(np.uint32)
    for clip in range(R // W):
        p = parent[clip * W:(clip + 1) * W]
        if np.array_equal(p, np.arange(W)) or (p < 0).any() or (p >= W).any():
            continue
        for w in range(W):
            codes[clip * W + w, :, :c + 1] = src_c[clip * W + p[w], :, :c + 1]
            out_s[clip * W + w, :, :c + 1] = src_s[clip * W + p[w], :, :c + 1]
    return codes, scale


def buffer_layout(depth, B, H, Tp):
    """The caller's buffer of dimx_set_cross_kv8 (include/dimx.h): per layer K codes, V codes, K scales, V scales, each 256-byte
    aligned, layers in order.  dimx_set_self_kv8's buffer is the same with the row count R = B * n_samples in place of B.
    -> (list of per-layer dicts of byte offsets, total bytes)"""
    al = lambda x: (x + 255) // 256 * 256
    cb, sb = al(B * H * Tp * 64), al(B * H * Tp * 4)
    off, lay = 0, []
    for _ in range(depth):
        lay.append({"kcodes": off, "vcodes": off + cb, "kscale": off + 2 * cb, "vscale": off + 2 * cb + sb})
        off += 2 * cb + 2 * sb
    return lay, off


def drift(logits_kv8, logits_plain, tokens_kv8=None, tokens_plain=None):
    """The report's arithmetic (tools/bench_kv8.py): the logit difference of a teacher-forced pair of runs and the share of equal
    tokens of a free-running pair.  logits [..., V]; tokens integer arrays of one shape."""
    a, b = np.asarray(logits_kv8, dtype=np.float64), np.asarray(logits_plain, dtype=np.float64)
    d = np.abs(a - b)
    out = {"logit_max_abs": float(d.max()), "logit_mean_abs": float(d.mean()),
           "logit_rel_to_spread": float(d.max() / max(float(b.std()), 1e-30)),
           "argmax_equal": float((a.argmax(-1) == b.argmax(-1)).mean())}
    if tokens_kv8 is not None:
        out["tokens_equal"] = float((np.asarray(tokens_kv8) == np.asarray(tokens_plain)).mean())
    return out
