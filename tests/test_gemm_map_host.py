"""CPU: the yardstick of tests/test_gpu_gemm_map.py (tests/gemm_map_ref.py) against the definition of the output map -- a naive
triple loop --, and its builders against torch's own view / permute of the same layouts."""
import pytest
import torch

import gemm_map_ref as R

SENT = 16384.0


def _naive(values, rowT, segs, seg_width, sizes):
    M, N = values.shape
    outs = [[SENT] * n for n in sizes]
    hit = [[False] * n for n in sizes]
    for m in range(M):
        b, t = divmod(m, rowT)
        for n in range(N):
            s, nn = divmod(n, seg_width)
            sb, sh, st, sd, D = segs[s]
            at = b * sb + t * st + (nn // D) * sh + (nn % D) * sd
            assert not hit[s][at]
            outs[s][at] = float(values[m, n])
            hit[s][at] = True
    return [torch.tensor(o) for o in outs], [torch.tensor(h) for h in hit]


def _run(values, mp):
    """scatter through an OutMap into fresh sentinel-filled destinations (segment pointer = destination + base)"""
    dests = [torch.full((n,), SENT) for n in mp.sizes]
    imgs = R.scatter(values, mp.rowT, mp.segs, mp.seg_width, [d[o:] for d, o in zip(dests, mp.base)])
    full = []
    for d, o, im in zip(dests, mp.base, imgs):
        f = torch.zeros(d.numel(), dtype=torch.bool)
        f[o:] = im
        full.append(f)
    return dests, full


MAPS = [("qkv_vt", lambda: R.qkv_map(2, 5, 2, 4, 8, False), 10), ("qkv_rowv", lambda: R.qkv_map(3, 3, 1, 8, 4, True), 9),
        ("cache", lambda: R.cache_map(2, 3, 1, 4, 2), 6), ("decode", lambda: R.decode_row_map(5, 2, 4, 6, 3), 5),
        ("plain", lambda: R.plain_map(7, 12, 16, rowT=3), 7)]


@pytest.mark.parametrize("name,build,M", MAPS, ids=[m[0] for m in MAPS])
def test_scatter_equals_the_triple_loop(name, build, M):
    mp = build()
    N = mp.seg_width * len(mp.segs)
    values = torch.arange(M * N, dtype=torch.float32).reshape(M, N) + 1.0
    dests, imgs = _run(values, mp)
    # the naive loop works on the segment pointers' frame: shift by base
    ref, hit = _naive(values, mp.rowT, mp.segs, mp.seg_width, [n - o for n, o in zip(mp.sizes, mp.base)])
    for d, im, o, r, h in zip(dests, imgs, mp.base, ref, hit):
        assert torch.equal(d[o:], r) and torch.equal(im[o:], h)
        assert not im[:o].any() and bool((d[:o] == SENT).all())
        assert bool((d[~im] == SENT).all()) and bool((d[im] != SENT).all())
    assert sum(int(im.sum()) for im in imgs) == M * N      # every element lands somewhere, once


@pytest.mark.parametrize("name,build,M", MAPS, ids=[m[0] for m in MAPS])
def test_segment_images_are_disjoint_in_one_allocation(name, build, M):
    """laid out back to back in ONE buffer (as the GPU tests allocate them) no two segments touch the same element"""
    mp = build()
    N = mp.seg_width * len(mp.segs)
    starts = [sum(mp.sizes[:i]) for i in range(len(mp.sizes))]
    buf = torch.full((sum(mp.sizes),), SENT)
    imgs = R.scatter(torch.ones(M, N), mp.rowT, mp.segs, mp.seg_width, [buf[s + o:] for s, o in zip(starts, mp.base)])
    count = torch.zeros(buf.numel(), dtype=torch.int32)
    for s, o, im in zip(starts, mp.base, imgs):
        count[s + o:] += im.int()
    assert int(count.max()) == 1 and int(count.sum()) == M * N


@pytest.mark.parametrize("B,T,H,D,Tp", [(2, 5, 2, 4, 8), (3, 7, 3, 2, 7)])
def test_qkv_builder_is_view_and_permute(B, T, H, D, Tp):
    x = torch.randn(B * T, 3 * H * D, generator=torch.Generator().manual_seed(B + T))
    x5 = x.view(B, T, 3, H, D)
    (q, k, vt), imgs = _run(x, R.qkv_map(B, T, H, D, Tp, False))
    assert torch.equal(q.view(B, T, H, D), x5[:, :, 0]) and torch.equal(k.view(B, T, H, D), x5[:, :, 1])
    vt = vt.view(B, H, D, Tp)
    assert torch.equal(vt[..., :T], x5[:, :, 2].permute(0, 2, 3, 1))
    assert bool((vt[..., T:] == SENT).all()) and not imgs[2].view(B, H, D, Tp)[..., T:].any()
    (q2, k2, v2), _ = _run(x, R.qkv_map(B, T, H, D, Tp, True))
    assert torch.equal(q2, q) and torch.equal(k2, k) and torch.equal(v2.view(B, T, H, D), x5[:, :, 2])


def test_cache_and_decode_builders_are_view_and_permute():
    B, T, H, Tp, nseg = 2, 3, 2, 5, 4
    x = torch.randn(B * T, nseg * H * 64, generator=torch.Generator().manual_seed(1))
    dests, imgs = _run(x, R.cache_map(B, T, H, Tp, nseg))
    ref = x.view(B, T, nseg, H, 64).permute(2, 0, 3, 1, 4)
    for i in range(nseg):
        c = dests[i].view(B, H, Tp, 64)
        assert torch.equal(c[:, :, :T], ref[i]) and bool((c[:, :, T:] == SENT).all())
    Bd, D, pos = 5, 4, 3
    y = torch.randn(Bd, 3 * H * D, generator=torch.Generator().manual_seed(2))
    (q, k, v), _ = _run(y, R.decode_row_map(Bd, H, D, Tp, pos))
    y4 = y.view(Bd, 3, H, D)
    assert torch.equal(q.view(Bd, H, D), y4[:, 0])
    for c, j in ((k, 1), (v, 2)):
        c = c.view(Bd, H, Tp, D)
        assert torch.equal(c[:, :, pos], y4[:, j])
        keep = torch.ones(Tp, dtype=torch.bool)
        keep[pos] = False
        assert bool((c[:, :, keep] == SENT).all())


def test_rowadd_rows():
    assert R.rowadd_rows(1, 9, 9, 3, 7).tolist() == [0, 1, 2, 0, 1, 2, 0]
    assert R.rowadd_rows(2, 5, 1, 3, 7).tolist() == [5, 5, 5, 6, 6, 6, 7]
    assert R.rowadd_rows(2, 3, 2, 1, 5).tolist() == [3, 3, 4, 4, 5]
    assert R.rowadd_rows(3, 2, 7, 3, 4).tolist() == [2, 2, 2, 2]


def test_scatter_refuses_a_map_that_overlaps_or_leaves():
    v = torch.ones(4, 4)
    with pytest.raises(AssertionError):
        R.scatter(v, 2, [(4, 0, 4, 1, 4)], 4, [torch.zeros(64)])      # clips 4 apart, rows 4 apart: clip 1 row 0 == clip 0 row 1
    with pytest.raises(AssertionError):
        R.scatter(v, 1, [(4, 0, 4, 1, 4)], 4, [torch.zeros(15)])
