"""GPU: the prefill attention kernels (csrc/attention_tr.hip through the row-major-v and the strided entry, csrc/attention.hip in
bf16 and f32) against tests/attn_probe.py: the count and the locator probe say exactly which keys every query saw, random data
against float64 at the tolerances of test_gpu_kernels.py, launches in which every persistent block takes several items, the
head-major cache layout with key words packed ahead, and rows without a visible key.  tests/test_attn_probe_host.py shows on the
CPU that the probes fail for every visibility defect at these shapes."""
import functools

import pytest
import torch

import attn_probe as P

pytestmark = pytest.mark.gpu

torch.set_grad_enabled(False)

BF, F32 = torch.bfloat16, torch.float32
# kernel, head width: attention_tr has 48- and 64-wide heads, attention.hip also the 96-wide ones of the legacy speaker VQ-VAE
KERNELS = [("tr_rowv", 48), ("tr_rowv", 64), ("bf16", 48), ("bf16", 64), ("bf16", 96), ("f32", 48), ("f32", 64), ("f32", 96)]
KERNEL_IDS = ["%s-%d" % k for k in KERNELS]
# random data against float64: (max, mean) as test_attention / test_row_major_v_attention_matches_f64_and_the_transposed_v_kernel
RANDOM_TOL = {"tr_rowv": (2.5e-2, 2e-3), "tr_packed": (2.5e-2, 2e-3), "tr_headmajor": (2.5e-2, 2e-3), "bf16": (2e-2, None), "f32": (2e-5, None)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def _dtype(kernel):
    return F32 if kernel == "f32" else BF


def _run(kernel, dev, q, k, v, scale, causal, lens, kmask, **kw):
    from dimx import engine
    lens_t = torch.tensor(lens, dtype=torch.int32, device=dev) if lens is not None else None
    km = kmask.to(dev) if kmask is not None else None
    args = (q.to(dev), k.to(dev), v.to(dev), scale, causal, lens_t, km)
    if kernel == "tr_rowv":
        out = engine.op_attention(*args, bf16=True, row_v=True)
    elif kernel in ("tr_packed", "tr_headmajor"):
        out = engine.op_attention(*args, layout=kernel[3:], **kw)
    else:
        out = engine.op_attention(*args, bf16=kernel == "bf16")
    if isinstance(out, tuple):
        return out[0].float().cpu(), out[1].float().cpu()
    return out.float().cpu()


@functools.lru_cache(maxsize=None)
def _case_data(name, D, dtype):
    """the masks, the three probes' inputs and references and (for a third of the cases) random data of a case, computed once"""
    case = P.CASES[P.CASE_IDS.index(name)]
    _, Lq, Lk, causal, _, _, with_random = case
    B, lens, kmask, kp = P.case_masks(case)
    H, scale = P.HEADS[D]
    d = {"B": B, "lens": lens, "kmask": kmask, "kp": kp, "H": H, "scale": scale, "Lq": Lq, "Lk": Lk, "causal": causal}
    d["count"] = P.count_inputs(B, Lq, Lk, H, D, P.SEED)
    for choice in ("last", "hidden"):
        q, k, v, _, hidden = P.locator_inputs(kp, H, D, scale, P.SEED + Lk, choice)
        d[choice] = (q, k, v, hidden, P.reference(q, k, v, scale, kp, dtype, lens))
    if with_random:
        g = torch.Generator().manual_seed(Lq * 31 + D)
        q, k, v = (torch.randn(B, n, H, D, generator=g) for n in (Lq, Lk, Lk))
        d["random"] = (q, k, v, P.reference(q, k, v, scale, kp, dtype, lens))
    return d


def _check_random(kernel, out, ref, kp, lens):
    valid, empty = P.row_classes(kp, lens)
    rows = valid & ~empty[:, None]
    err = (out.double() - ref).abs()[rows]
    tol_max, tol_mean = RANDOM_TOL[kernel]
    print("%s random data: max err %.3g mean %.3g" % (kernel, err.max().item(), err.mean().item()))
    assert torch.isfinite(out).all()
    assert err.max().item() < tol_max
    if tol_mean is not None:
        assert err.mean().item() < tol_mean


def _run_all_entries(kernel, dev, *args):
    """attention_tr also through the strided entry in the packed layout, where q / k / v are followed by NaN rows (rows at or past
    Lq / Lk are clamped to the last row, never read), the key words packed inside the launch and ahead of it: the same bits"""
    out = _run(kernel, dev, *args)
    if kernel == "tr_rowv":
        for pre in (False, True):
            assert torch.equal(_run("tr_packed", dev, *args, prepacked=pre), out), pre
    return out


def _check_case(kernel, dev, d, dtype):
    """the count probe, both locator probes and, where the case has it, random data"""
    args = (d["scale"], d["causal"], d["lens"], d["kmask"])
    q, k, v = d["count"]
    assert P.count_failures(_run_all_entries(kernel, dev, q, k, v, *args), d["kp"], v, d["lens"], dtype) == []
    for choice in ("last", "hidden"):
        q, k, v, hidden, ref = d[choice]
        out = _run_all_entries(kernel, dev, q, k, v, *args)
        assert P.locator_failures(out, ref, d["kp"], d["lens"], d["Lk"], hidden) == [], choice
    if "random" in d:
        q, k, v, ref = d["random"]
        _check_random(kernel, _run_all_entries(kernel, dev, q, k, v, *args), ref, d["kp"], d["lens"])


@pytest.mark.parametrize("kernel,D", KERNELS, ids=KERNEL_IDS)
@pytest.mark.parametrize("name", P.CASE_IDS)
def test_every_query_sees_exactly_its_keys(dev, name, kernel, D):
    """Every case of attn_probe.CASES on every kernel (attention_tr through both of its entries): the visible-key counts and the
    located key are exact, an empty clip's rows are zero, its neighbours unaffected, nothing past the last row is read.  D = 96 in
    f32 holds the 2e-5 of the narrower heads on random data (measured 9e-7)."""
    dtype = _dtype(kernel)
    _check_case(kernel, dev, _case_data(name, D, dtype), dtype)


@pytest.mark.parametrize("Lq", [1, 10, 33])
def test_head_major_caches_with_a_wide_output_and_prepacked_key_words(dev, Lq):
    """The layout of the best-of-N cross attention and the prompt prefill: K / V [B, H, Tp, 64] with T = 130 of Tp = 136 rows (the
    rest NaN), Lq != Lk, a key mask with a row stride of its own, an output wider than H * D.  Both probes exact, nothing written
    outside the Lq x H*D block, the same bits with the key words packed ahead of the launch."""
    from dimx import engine
    D, T, Tp = 64, 130, 136
    H, scale = P.HEADS[D]
    B = 3
    kmask = P.build_mask(B, T, ("random", ("hide", 0, 71), ("hide", 64, 128)), P.SEED + Lq)
    kp = P.keep(Lq, T, False, None, kmask, B)
    kw = dict(tp=Tp, ld_o=H * D + 64, kmask_ld=T + 14, return_buffer=True)
    q, k, v = P.count_inputs(B, Lq, T, H, D, P.SEED)
    outs = {}
    for pre in (False, True):
        out, buf = _run("tr_headmajor", dev, q, k, v, scale, False, None, kmask, prepacked=pre, **kw)
        assert P.count_failures(out, kp, v, None, BF) == []
        assert (buf[:, :Lq, H * D:] == engine.ATTN_CANARY).all() and (buf[:, Lq:] == engine.ATTN_CANARY).all()
        outs[pre] = buf
    assert torch.equal(outs[False], outs[True])
    for choice in ("last", "hidden"):
        q, k, v, _, hidden = P.locator_inputs(kp, H, D, scale, P.SEED + T, choice)
        ref = P.reference(q, k, v, scale, kp, BF)
        bufs = []
        for pre in (False, True):
            out, buf = _run("tr_headmajor", dev, q, k, v, scale, False, None, kmask, prepacked=pre, **kw)
            assert P.locator_failures(out, ref, kp, None, T, hidden) == [], choice
            assert (buf[:, :Lq, H * D:] == engine.ATTN_CANARY).all() and (buf[:, Lq:] == engine.ATTN_CANARY).all()
            bufs.append(buf)
        assert torch.equal(bufs[0], bufs[1])
    g = torch.Generator().manual_seed(Lq)
    q, k, v = (torch.randn(B, n, H, D, generator=g) for n in (Lq, T, T))
    out, _ = _run("tr_headmajor", dev, q, k, v, scale, False, None, kmask, prepacked=True, **kw)
    _check_random("tr_headmajor", out, P.reference(q, k, v, scale, kp, BF), kp, None)
    assert torch.equal(out, _run("tr_rowv", dev, q, k, v, scale, False, None, kmask))


@pytest.mark.parametrize("L,D,causal", [(130, 64, False), (130, 64, True), (129, 48, False)])
def test_persistent_blocks_taking_three_items_each(dev, L, D, causal):
    """attention_tr runs 3 blocks per CU; with more than 6 * CUs items every block takes three or more, so the K / V ring, the Q rows
    of the next item, the counted waits, the next item's key word and clip length and the item rotation all cross item boundaries
    (L = 130: three tiles per item, the ring slot's parity flips from item to item).  Clip lengths cycle through 0, 1, 64, 65, L
    under a random mask.  Counts exact and random data within tolerance over all clips; chosen clips bit-equal to a launch of that
    clip alone, because an item's arithmetic does not depend on the block that runs it."""
    H, scale = P.HEADS[D]
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    nqb = (L + 127) // 128
    B = 6 * n_cu // (H * nqb) + 1
    assert B * H * nqb > 6 * n_cu
    cycle = [L, 0, L, 1, 64, 65, L]
    lens = [cycle[b % len(cycle)] for b in range(B)]
    lens[-1] = L
    kmask = P.random_mask(B, L, P.SEED + L)
    kp = P.keep(L, L, causal, lens, kmask)
    args = (scale, causal)
    q, k, v = P.count_inputs(B, L, L, H, D, P.SEED)
    assert P.count_failures(_run("tr_rowv", dev, q, k, v, *args, lens, kmask), kp, v, lens, BF) == []
    g = torch.Generator().manual_seed(L * 17 + D)
    q, k, v = (torch.randn(B, L, H, D, generator=g) for _ in range(3))
    out = _run("tr_rowv", dev, q, k, v, *args, lens, kmask)
    _check_random("tr_rowv", out, P.reference(q, k, v, scale, kp, BF, lens), kp, lens)
    # the first and the last clip, both neighbours of an empty clip, and more: a clip's H pairs fall on every residue mod 8
    chosen = sorted({0, 2, B - 1, 3, 4, 5, 6, 7, 8, B // 2, B - 2})
    assert lens[1] == 0 and len(chosen) >= 8
    for b in chosen:
        alone = _run("tr_rowv", dev, q[b:b + 1], k[b:b + 1], v[b:b + 1], *args, lens[b:b + 1], kmask[b:b + 1])
        assert torch.equal(alone[0], out[b]), b


@pytest.mark.parametrize("kernel,D", KERNELS + [("tr_packed", 48), ("tr_packed", 64)], ids=KERNEL_IDS + ["tr_packed-48", "tr_packed-64"])
def test_rows_without_a_visible_key(dev, kernel, D):
    """A context mask that hides every key of a clip reaches the cross attention of every decoder stack (nothing rejects it:
    test_all_masked_context_through_generate), so the non-causal value is pinned: the mean of V over all Lk keys, here exactly, by
    the count probe and on random data.  Causal rows whose keys 0 .. i are all masked (no caller produces them: AutoregressiveWrapper
    keeps token 0, the padding masks keep a prefix) only have to be finite.  Either way the other clips' bits do not change."""
    dtype = _dtype(kernel)
    H, scale = P.HEADS[D]
    B, Lq, Lk = 3, 33, 129
    for causal in (False, True):
        L = Lk if causal else Lq
        kmask = P.random_mask(B, Lk, P.SEED)
        other = kmask.clone()
        other[1] = 1
        if causal:
            kmask[1, :5] = 0                   # rows 0 .. 4 of clip 1 see nothing
        else:
            kmask[1] = 0
        kp = P.keep(L, Lk, causal, None, kmask, B)
        q, k, v = P.count_inputs(B, L, Lk, H, D, P.SEED)
        out = _run(kernel, dev, q, k, v, scale, causal, None, kmask)
        assert P.count_failures(out, kp, v, None, dtype, full_rows_exact=not causal) == []
        g = torch.Generator().manual_seed(7 + D)
        q, k, v = (torch.randn(B, n, H, D, generator=g) for n in (L, Lk, Lk))
        out = _run(kernel, dev, q, k, v, scale, causal, None, kmask)
        ref = P.reference(q, k, v, scale, kp, dtype)
        _check_random(kernel, out, ref, kp if causal else torch.ones_like(kp), None)    # non-causal: clip 1's rows too
        base = _run(kernel, dev, q, k, v, scale, causal, None, other)
        assert torch.equal(out[0], base[0]) and torch.equal(out[2], base[2])
