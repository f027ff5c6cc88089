"""Plain reference of the GEMM epilogue's output map (GemmArgs.rowT / seg[] / rowadd_* in csrc/common.hpp), written from the
definition and importing nothing from the library:

    row m = b * rowT + t; the N columns are len(segs) equal segments of seg_width columns; element (m, n) of segment s,
    nn = n - s * seg_width, lands at element  b*sb + t*st + (nn // D)*sh + (nn % D)*sd  of the segment's destination.

A segment is the tuple (sb, sh, st, sd, D).  The builders below describe the maps the library's projections use; each returns an
OutMap whose ``base[i]`` is the element of destination i the segment pointer refers to and whose ``sizes[i]`` is the number of
elements of that destination (so that a test can lay the destinations out in one allocation, guards around them).
"""
import collections

import torch

OutMap = collections.namedtuple("OutMap", "rowT seg_width segs sizes base")


def scatter(values, rowT, segs, seg_width, dest_buffers):
    """Place values[M, N] through the map into dest_buffers (one flat tensor per segment, element 0 = the segment pointer), in place.
    Returns the boolean image of the map: one flat bool tensor per destination, True where an element is written.  Raises when
    the map leaves a destination or sends two elements to the same place."""
    M, N = values.shape
    assert N == seg_width * len(segs) == seg_width * len(dest_buffers)
    dev = values.device
    m = torch.arange(M, device=dev, dtype=torch.int64)
    b, t = m // rowT, m % rowT
    images = []
    for s, ((sb, sh, st, sd, D), dst) in enumerate(zip(segs, dest_buffers)):
        assert dst.dim() == 1 and dst.is_contiguous() and seg_width % D == 0
        nn = torch.arange(seg_width, device=dev, dtype=torch.int64)
        idx = ((b * sb + t * st)[:, None] + ((nn // D) * sh + (nn % D) * sd)[None, :]).reshape(-1)
        assert int(idx.min()) >= 0 and int(idx.max()) < dst.numel(), "segment %d leaves its destination" % s
        img = torch.zeros(dst.numel(), dtype=torch.bool, device=dev)
        img[idx] = True
        assert int(img.sum()) == idx.numel(), "segment %d writes an element twice" % s
        dst[idx] = values[:, s * seg_width:(s + 1) * seg_width].reshape(-1).to(dst.dtype)
        images.append(img)
    return images


def rowadd_rows(mode, off, div, rowT, M):
    """Table row added to output row m (mode 1: t, 2: b // div + off, 3: off); int64 [M]."""
    m = torch.arange(M, dtype=torch.int64)
    if mode == 1:
        return m % rowT
    if mode == 2:
        return (m // rowT) // div + off
    assert mode == 3
    return torch.full((M,), off, dtype=torch.int64)


def plain_map(M, N, ldc, rowT=1):
    """C [M, ldc] row-major, columns N .. ldc-1 untouched (gemm_set_plain_out)."""
    return OutMap(rowT, N, [(ldc * rowT, 0, ldc, 1, N)], [M * ldc], [0])


def qkv_map(B, T, H, D, Tp, rowv):
    """Fused q/k/v projection: q and k [B, T, H*D] row-major; v the same (rowv) or transposed [B, H, D, Tp] (time contiguous)."""
    segw = H * D
    row = (T * segw, D, segw, 1, D)
    if rowv:
        return OutMap(T, segw, [row, row, row], [B * T * segw] * 3, [0, 0, 0])
    vt = (H * D * Tp, D * Tp, 1, Tp, D)
    return OutMap(T, segw, [row, row, vt], [B * T * segw, B * T * segw, B * H * D * Tp], [0, 0, 0])


def cache_map(B, T, H, Tp, nseg):
    """Cross-attention K | V (| K | V ...) projection: every segment a head-major [B, H, Tp, 64] cache, rows T .. Tp-1 untouched."""
    seg = (H * Tp * 64, Tp * 64, 64, 1, 64)
    return OutMap(T, H * 64, [seg] * nseg, [B * H * Tp * 64] * nseg, [0] * nseg)


def decode_row_map(B, H, D, Tp, pos):
    """One decode step (one row per clip): q to plain rows [B, H*D], k and v to row `pos` of [B, H, Tp, D] caches."""
    segw = H * D
    q = (segw, D, segw, 1, D)
    kv = (H * Tp * D, Tp * D, D, 1, D)
    return OutMap(1, segw, [q, kv, kv], [B * segw, B * H * Tp * D, B * H * Tp * D], [0, pos * D, pos * D])
