"""GPU: the retrieval baselines in the HIP library (dimx_op_pool_desc / dimx_op_nn_search / dimx_op_nn_gather, csrc/retrieval.hip)
through dimx.engine and the C-ABI, against their definition (dimx.retrieval, numpy float64).

Bounds against the definition: max descriptors are bit-equal; mean descriptors and norms 1e-11 relative (the project's bound for
float64 moments, tests/test_gpu_consensus.py); every similarity 1e-11 absolute (|sim| <= 1).  The k-best lists are compared on every
query whose smallest gap among its top K + 1 similarities (dimx.retrieval.margins) exceeds 1e-9, 100 x the bound, and no query of
the cases below is closer than that (asserted; the smallest margin of each case is printed).  Exact ties are constructed and checked
by bit equality."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import stub_model  # noqa: E402,F401  (puts dimx on the path as the other protocol tests do)

pytestmark = pytest.mark.gpu

T = 39
SIZES = [(1, 1), (2, 5), (37, 5), (1025, 17)]           # (N, Q): one library chunk (256) and one query tile (16) crossed by one
FEATS = [(768, "max"), (56, "mean"), (9, "mean")]
KS = (1, 3, 10, 16)
CASES = [(n, q, d, kind) for n, q in SIZES for d, kind in FEATS]
CASE_IDS = ["N%d-Q%d-D%d-%s" % c for c in CASES]
BOUND, MARGIN = 1e-11, 1e-9
ERR_ARG, ERR_WORKSPACE = -1, -5


def _dev():
    return torch.device("cuda:0")


def _bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


@functools.lru_cache(maxsize=None)
def _clips(seed, n, d):
    """a seeded ragged batch: x [n, T, d] f32, lens in 1..T (clip 0 has one frame when there is more than one clip)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, T, d, generator=g)
    lens = torch.randint(1, T + 1, (n,), generator=g).tolist()
    if n > 1:
        lens[0], lens[1] = 1, T
    return x, lens


@functools.lru_cache(maxsize=None)
def _reference(n, q, d, kind):
    """the definition: library / query descriptors, norms and the similarity matrix; computed once per case, never modified"""
    from dimx import retrieval
    x, xl = _clips(100 + n, n, d)
    qx, ql = _clips(200 + q, q, d)
    Xd, Xn = retrieval.pool_batch(x.numpy(), xl, kind)
    Qd, Qn = retrieval.pool_batch(qx.numpy(), ql, kind)
    sim = retrieval.similarities(Qd, Xd)
    for a in (Xd, Xn, Qd, Qn, sim):
        a.setflags(write=False)
    return Xd, Xn, Qd, Qn, sim


@functools.lru_cache(maxsize=None)
def _device(n, q, d, kind):
    """the operators' descriptors of the same clips, left on the GPU"""
    from dimx.engine import op_pool_desc
    x, xl = _clips(100 + n, n, d)
    qx, ql = _clips(200 + q, q, d)
    return op_pool_desc(x.to(_dev()), xl, kind) + op_pool_desc(qx.to(_dev()), ql, kind)


def _search(qd, qn, xd, xn, k, want_sim=True):
    from dimx.engine import op_nn_search
    return tuple(t.cpu() for t in op_nn_search(qd, qn, xd, xn, k, want_sim=want_sim))


@pytest.mark.parametrize("n,q,d,kind", CASES, ids=CASE_IDS)
def test_pooling_matches_the_definition(n, q, d, kind):
    Xd, Xn, Qd, Qn, _ = _reference(n, q, d, kind)
    xd, xn, qd, qn = (t.cpu().numpy() for t in _device(n, q, d, kind))
    for got, want, gn, wn in ((xd, Xd, xn, Xn), (qd, Qd, qn, Qn)):
        assert got.dtype == np.float64 and got.shape == want.shape and gn.shape == wn.shape
        if kind == "max":
            assert np.array_equal(got.view(np.int64), want.view(np.int64))
        else:
            err = np.abs(got - want) / np.abs(want)
            print("mean descriptors: worst relative error %.3e (bound %.0e)" % (err.max(), BOUND))
            assert (want != 0).all() and (err <= BOUND).all()
        assert (wn > 0).all() and (np.abs(gn - wn) <= BOUND * wn).all()


@pytest.mark.parametrize("n,q,d,kind", CASES, ids=CASE_IDS)
def test_similarities_and_k_best_lists_match_the_definition(n, q, d, kind):
    from dimx import retrieval
    _, _, _, _, ref_sim = _reference(n, q, d, kind)
    xd, xn, qd, qn = _device(n, q, d, kind)
    assert np.isfinite(ref_sim).all()
    for k in KS:
        idx, sim, found, sim_all = _search(qd, qn, xd, xn, k)
        assert tuple(idx.shape) == (q, k) and tuple(sim.shape) == (q, k) and tuple(found.shape) == (q,) and tuple(sim_all.shape) == (q, n)
        err = np.abs(sim_all.numpy() - ref_sim).max()
        margins = retrieval.margins(ref_sim, k)
        print("K=%d: worst error of a similarity %.3e (bound %.0e), smallest margin of the definition %.3e" % (k, err, BOUND, margins.min()))
        assert err <= BOUND
        assert (margins > MARGIN).all(), "a query is closer than the list check allows: %s" % (margins,)
        want_idx, _, want_found = retrieval.top_k(ref_sim, k)
        assert np.array_equal(idx.numpy(), want_idx) and np.array_equal(found.numpy(), want_found)
        assert found.tolist() == [min(k, n)] * q
        # the returned similarities are the matrix entries they name, bit for bit; unfilled slots are -1 / NaN
        own_idx, own_sim, _ = retrieval.top_k(sim_all.numpy(), k)
        assert np.array_equal(idx.numpy(), own_idx) and np.array_equal(sim.numpy().view(np.int64)[own_idx >= 0],
                                                                       own_sim.view(np.int64)[own_idx >= 0])
        assert np.isnan(sim.numpy()[own_idx < 0]).all()
        # without the matrix the lists are the same bits
        plain = _search(qd, qn, xd, xn, k, want_sim=False)
        assert len(plain) == 3 and _same(plain[0], idx) and _same(plain[1][idx >= 0], sim[idx >= 0]) and _same(plain[2], found)


def test_duplicates_across_a_chunk_boundary_tie_bit_for_bit():
    xd, xn, qd, qn = (t.clone() for t in _device(1025, 17, 768, "max"))
    xd[1024], xn[1024] = xd[3], xn[3]
    xd[300], xn[300] = xd[3], xn[3]
    qd[16], qn[16] = xd[3], xn[3]                         # query 16 is that entry: the three copies lead its list
    idx, sim, found, sim_all = _search(qd, qn, xd, xn, 10)
    s = sim_all.view(torch.int64)
    assert torch.equal(s[:, 3], s[:, 1024]) and torch.equal(s[:, 3], s[:, 300])
    assert idx[16, :3].tolist() == [3, 300, 1024]
    assert torch.equal(sim[16, :3].view(torch.int64), s[16, [3, 300, 1024]])
    for j in range(17):                                   # wherever the copies are listed, they are adjacent and in index order
        row = idx[j].tolist()
        if 3 in row and row.index(3) + 2 < 10:
            assert row[row.index(3):row.index(3) + 3] == [3, 300, 1024]
        assert 1024 not in row or 3 in row


def test_a_slice_of_the_library_and_repeated_calls_give_the_same_bits():
    xd, xn, qd, qn = _device(1025, 17, 768, "max")
    full = _search(qd, qn, xd, xn, 3)
    again = _search(qd, qn, xd, xn, 3)
    assert all(_same(a, b) for a, b in zip(full, again))
    part = _search(qd, qn, xd[5:30], xn[5:30], 3)
    assert _same(part[3], full[3][:, 5:30])
    part = _search(qd[3:4], qn[3:4], xd[250:270], xn[250:270], 16)      # another tile slot, across the chunk boundary at 256
    assert _same(part[3], full[3][3:4, 250:270])
    xd9, xn9, qd9, qn9 = _device(37, 5, 9, "mean")
    full9 = _search(qd9, qn9, xd9, xn9, 3)
    assert _same(_search(qd9[1:], qn9[1:], xd9[5:30], xn9[5:30], 3)[3], full9[3][1:, 5:30])
    pool_a = _device.__wrapped__(37, 5, 56, "mean")
    assert all(_same(a, b) for a, b in zip(pool_a, _device(37, 5, 56, "mean")))


def test_zero_norms_opposites_and_short_libraries():
    from dimx import retrieval
    g = torch.Generator().manual_seed(9)
    D = 16
    xd = torch.randn(9, D, generator=g, dtype=torch.float64)
    q = torch.sign(torch.randn(D, generator=g, dtype=torch.float64))        # +-1: the norm is 4 and the similarities below are exact
    xd[4] = 0.0                                           # a zero-norm entry: NaN, never chosen
    xd[7] = -q                                            # exactly opposite: similarity -1, not eligible
    xd[2] = xd[6] = 3.0 * q
    qd = torch.stack([q, torch.zeros(D, dtype=torch.float64)])              # and a zero query
    xn, qn = xd.pow(2).sum(1).sqrt(), qd.pow(2).sum(1).sqrt()
    idx, sim, found, sim_all = _search(qd.to(_dev()), qn.to(_dev()), xd.to(_dev()), xn.to(_dev()), 16)      # N < K
    ref = retrieval.similarities(qd.numpy(), xd.numpy())
    assert torch.isnan(sim_all[0, 4]) and float(sim_all[0, 7]) == -1.0 and float(sim_all[0, 2]) == 1.0 == float(sim_all[0, 6])
    ok = ~np.isnan(ref)
    assert np.array_equal(np.isnan(sim_all.numpy()), ~ok) and np.abs(sim_all.numpy()[ok] - ref[ok]).max() <= BOUND
    want_idx, want_sim, want_found = retrieval.top_k(ref, 16)
    assert found.tolist() == [7, 0] == want_found.tolist()
    assert np.array_equal(idx.numpy(), want_idx)
    assert idx[0, :2].tolist() == [2, 6] and idx[0, 7:].tolist() == [-1] * 9 and idx[1].tolist() == [-1] * 16
    assert torch.isnan(sim[0, 7:]).all() and torch.isnan(sim[1]).all() and torch.isnan(sim_all[1]).all()
    assert retrieval.reference_index(idx[:, :1].numpy()).tolist() == [[2], [0]]
    # nothing but an opposite and a zero entry: nothing found
    two = torch.stack([-q, torch.zeros(D, dtype=torch.float64)])
    idx, sim, found = _search(qd[:1].to(_dev()), qn[:1].to(_dev()), two.to(_dev()), two.pow(2).sum(1).sqrt().to(_dev()), 3, want_sim=False)
    assert found.tolist() == [0] and idx.tolist() == [[-1, -1, -1]] and torch.isnan(sim).all()


def test_guard_values_behind_the_valid_frames_and_behind_the_library_change_nothing():
    from dimx.engine import op_pool_desc
    for d, kind in FEATS:
        x, lens = _clips(137, 37, d)
        clean = _device(37, 5, d, kind)
        g = x.clone()
        for j, n in enumerate(lens):
            g[j, n:] = float("nan") if j % 2 else 1e30
        big = torch.full((40, T + 2, d + 3), float("nan"))
        big[:37, :T, :d] = g
        view = big.to(_dev())[:37, :T, :d]                # clip, frame and column strides of a larger buffer
        assert not view.is_contiguous() and view.stride(2) == 1
        got = op_pool_desc(view, lens, kind)
        assert _same(got[0], clean[0]) and _same(got[1], clean[1])
    xd, xn, qd, qn = _device(37, 5, 56, "mean")
    over_d = torch.full((64, 56), float("nan"), dtype=torch.float64, device=_dev())
    over_n = torch.full((64,), float("nan"), dtype=torch.float64, device=_dev())
    over_d[:37], over_n[:37] = xd, xn
    a, b = _search(qd, qn, over_d[:37], over_n[:37], 16), _search(qd, qn, xd, xn, 16)
    assert all(_same(p, r) for p, r in zip(a, b)) and not torch.isnan(a[1]).any()


@functools.lru_cache(maxsize=None)
def _gather_inputs():
    g = torch.Generator().manual_seed(21)
    N, Lmax, W, Q, K = 11, 23, 56, 6, 3
    lib = torch.randn(N, Lmax, W, generator=g)
    lib_lens = torch.randint(1, Lmax + 1, (N,), generator=g).tolist()
    lib_lens[2], lib_lens[5] = 0, Lmax
    idx = torch.randint(0, N, (Q, K), generator=g, dtype=torch.int32)
    idx[0, 1], idx[3, 2], idx[4, 0], idx[1, 0], idx[2, 1] = -1, -1, 2, 5, 5
    q_lens = [Lmax, 1, 17, 9, 23, 0]
    return lib, lib_lens, idx, q_lens


def test_gather_matches_the_definition_on_views_and_ignores_guards():
    from dimx import retrieval
    from dimx.engine import op_nn_gather
    lib, lib_lens, idx, q_lens = _gather_inputs()
    N, Lmax, W = lib.shape
    for L_out in (None, 12, 30):
        want, want_len = retrieval.gather(lib.numpy(), lib_lens, idx.numpy(), q_lens, L=L_out)
        out, out_len = (t.cpu() for t in op_nn_gather(lib.to(_dev()), lib_lens, idx.to(_dev()), q_lens, L=L_out))
        assert out.dtype == torch.float32 and out_len.dtype == torch.int32
        assert np.array_equal(out_len.numpy(), want_len) and np.array_equal(out.numpy().view(np.int32), want.view(np.int32))
        assert not out[0, 1].any() and int(out_len[0, 1]) == 0 and not out[4, 0].any() and not out[5].any()
    clean = tuple(t.cpu() for t in op_nn_gather(lib.to(_dev()), lib_lens, idx.to(_dev()), q_lens))
    guarded = lib.clone()
    for j, n in enumerate(lib_lens):
        guarded[j, n:] = float("nan")
    big = torch.full((N + 4, Lmax + 2, W + 8), float("nan"))                # entries behind N, frames behind Lmax, columns behind 56
    big[:N, :Lmax, :W] = guarded
    view = big.to(_dev())[:N, :Lmax, :W]
    assert not view.is_contiguous() and view.stride(2) == 1
    shifted = torch.full((N, Lmax + 1, W), float("nan"))
    shifted[:, 1:] = guarded
    for v in (guarded.to(_dev()), view, shifted.to(_dev())[:, 1:]):
        got = tuple(t.cpu() for t in op_nn_gather(v, lib_lens, idx.to(_dev()), q_lens))
        assert _same(got[0], clean[0]) and _same(got[1], clean[1])
    got = op_nn_gather(lib.to(_dev()), torch.tensor(lib_lens, device=_dev()), idx.long().to(_dev()), torch.tensor(q_lens, device=_dev()))
    assert _same(got[0].cpu(), clean[0]) and _same(got[1].cpu(), clean[1])


def test_cpu_tensors_raise():
    from dimx import lib as L
    from dimx.engine import op_nn_gather, op_nn_search, op_pool_desc
    lib, lib_lens, idx, q_lens = _gather_inputs()
    with pytest.raises(L.DimxError):
        op_pool_desc(lib, lib_lens, "max")
    with pytest.raises(L.DimxError):
        op_nn_gather(lib, lib_lens, idx, q_lens)
    d = torch.zeros(3, 4, dtype=torch.float64)
    with pytest.raises(L.DimxError):
        op_nn_search(d, d[:, 0], d, d[:, 0], 1)
    with pytest.raises(ValueError):
        op_pool_desc(lib.to(_dev()), lib_lens, "median")


def test_bad_arguments_return_an_error_and_leave_the_outputs_untouched():
    from dimx import lib as L
    lib = L.load()
    xd, xn, qd, qn = _device(37, 5, 56, "mean")
    Q, N, D = 5, 37, 56
    need = int(lib.dimx_op_nn_search_ws_bytes(Q, N, D, 16))
    assert need > 0 and int(lib.dimx_op_nn_search_ws_bytes(Q, N, D, 0)) == 0 and int(lib.dimx_op_nn_search_ws_bytes(Q, N, D, 17)) == 0
    ws = torch.zeros(need + 8, dtype=torch.uint8, device=_dev())
    idx = torch.full((Q, 17), -7, dtype=torch.int32, device=_dev())
    sim = torch.full((Q, 17), -7.0, dtype=torch.float64, device=_dev())
    found = torch.full((Q,), -7, dtype=torch.int32, device=_dev())

    def call(K=16, N_=N, D_=D, ld=D, ws_bytes=need, ws_off=0, idx_p=L.ptr(idx)):
        return lib.dimx_op_nn_search(L.ptr(qd), ld, L.ptr(qn), L.ptr(xd), D, L.ptr(xn), Q, N_, D_, K, idx_p, L.ptr(sim), L.ptr(found), None,
                                     ctypes.c_void_p(ws.data_ptr() + ws_off), ws_bytes, L.stream_ptr(_dev()))

    for kw in (dict(K=0), dict(K=17), dict(K=-1), dict(N_=0), dict(D_=0), dict(D_=961), dict(ld=-56), dict(ws_off=4), dict(idx_p=None)):
        assert call(**kw) == ERR_ARG, kw
    assert call(ws_bytes=need - 1) == ERR_WORKSPACE and call(ws_bytes=0) == ERR_WORKSPACE
    lib_seq, lib_lens, g_idx, q_lens = _gather_inputs()
    d_lib, d_idx = lib_seq.to(_dev()), g_idx.to(_dev())
    d_ll, d_ql = torch.tensor(lib_lens, dtype=torch.int32, device=_dev()), torch.tensor(q_lens, dtype=torch.int32, device=_dev())
    out = torch.full((6, 3, 23, 56), -7.0, device=_dev())
    out_len = torch.full((6, 3), -7, dtype=torch.int32, device=_dev())

    def gather(K=3, cs=d_lib.stride(0), fs=d_lib.stride(1), L_=23):
        return lib.dimx_op_nn_gather(L.ptr(d_idx), L.ptr(d_lib), cs, fs, L.ptr(d_ll), L.ptr(d_ql), 6, K, 11, 23, L_, 56, L.ptr(out),
                                     L.ptr(out_len), L.stream_ptr(_dev()))

    for kw in (dict(K=0), dict(K=17), dict(cs=-1), dict(fs=-56), dict(L_=0)):
        assert gather(**kw) == ERR_ARG, kw
    x = lib_seq.to(_dev())
    desc = torch.full((11, 56), -7.0, dtype=torch.float64, device=_dev())
    norm = torch.full((11,), -7.0, dtype=torch.float64, device=_dev())

    def pool(kind=0, cs=x.stride(0), D_=56, N_=11):
        return lib.dimx_op_pool_desc(L.ptr(x), cs, x.stride(1), L.ptr(d_ll), N_, 23, D_, kind, L.ptr(desc), L.ptr(norm), L.stream_ptr(_dev()))

    for kw in (dict(kind=2), dict(kind=-1), dict(cs=-1), dict(D_=0), dict(N_=0)):
        assert pool(**kw) == ERR_ARG, kw
    torch.cuda.synchronize()
    assert (idx == -7).all() and (sim == -7.0).all() and (found == -7).all() and not ws.any()
    assert (out == -7.0).all() and (out_len == -7).all() and (desc == -7.0).all() and (norm == -7.0).all()
    assert call() == 0 and gather() == 0 and pool() == 0      # the same buffers with valid arguments: the calls themselves work
    torch.cuda.synchronize()
    want = _search(qd, qn, xd, xn, 16, want_sim=False)
    assert torch.equal(idx.cpu().reshape(-1)[:Q * 16].reshape(Q, 16), want[0]) and torch.equal(found.cpu(), want[2])     # dense [Q, 16]


# ---- the protocol: batches in the loader's format, B = 4, T = 40
def _batches(seed, n_batches, lens_of):
    from dimx import prng
    out = []
    for i in range(n_batches):
        lens = lens_of(i)
        B, Tm = len(lens), 40
        src = torch.from_numpy(prng.normal(seed + i, "retr.src", (B, Tm, 824)))
        tgt = torch.from_numpy(prng.normal(seed + i, "retr.tgt", (B, Tm, 56)))
        for j, n in enumerate(lens):
            src[j, n:] = 0
            tgt[j, n:] = 0
        out.append((src, tgt, list(lens), None, ["clip_%d_%d_%d" % (seed, i, j) for j in range(B)]))
    return out


def _train():
    return _batches(500, 3, lambda i: [40, 33 - i, 27 + i, 21 + 2 * i])


def _test():
    return _batches(600, 2, lambda i: [40, 36 - 3 * i, 25, 29 + i])


@functools.lru_cache(maxsize=None)
def _protocol_reference(kind, k):
    """the definition on the loader's clips -> per test clip (idx [k], list [k, L, 56], length); asserts the picks are decidable"""
    from dimx import retrieval
    pooling = retrieval.FEATURES[kind]
    cols = slice(56, 824) if kind == "audio" else slice(0, 56)
    feats = [(b[0][j, :, cols].numpy(), b[2][j]) for b in _train() for j in range(len(b[2]))]
    lib_seq = np.stack([b[1][j, 1:].numpy() for b in _train() for j in range(len(b[2]))])
    lib_lens = [b[2][j] - 1 for b in _train() for j in range(len(b[2]))]
    Xd = np.stack([retrieval.pool(x, n, pooling) for x, n in feats])
    out = []
    for b in _test():
        Qd = np.stack([retrieval.pool(b[0][j, :, cols].numpy(), b[2][j], pooling) for j in range(len(b[2]))])
        sim = retrieval.similarities(Qd, Xd)
        assert (retrieval.margins(sim, k) > MARGIN).all()
        idx, _, found = retrieval.top_k(sim, k)
        assert found.tolist() == [k] * len(b[2])
        q_lens = [n - 1 for n in b[2]]
        seqs, seq_len = retrieval.gather(lib_seq, lib_lens, idx, q_lens, L=39)
        out.extend((idx[j], seqs[j], int(seq_len[j].min()), b[1][j, 1:].numpy()) for j in range(len(b[2])))
    return out


def _library(kind):
    from dimx import x_engine_pt
    from dimx.retrieval import RetrievalLibrary
    return x_engine_pt.fill_retrieval_library(RetrievalLibrary(kind), _train(), _dev())


@pytest.mark.parametrize("kind", ["audio", "motion"])
def test_library_add_and_query_equal_the_definitions_picks(kind):
    from dimx import x_engine_pt
    lib = _library(kind)
    assert len(lib) == 12
    ref = _protocol_reference(kind, 3)
    at = 0
    for batch in _test():
        src_s_v, src_s_a, tgt, _, src_len, _ = x_engine_pt._prepare(batch, _dev())
        feats = src_s_a if kind == "audio" else src_s_v
        idx, sim, found, y_pred, out_len = lib.query(feats, src_len, k=3, out_lens=[n - 1 for n in src_len], L=39)
        assert all(t.is_cuda for t in (idx, sim, found, y_pred, out_len)) and tuple(y_pred.shape) == (4, 3, 39, 56)
        for j in range(4):
            want_idx, want_list, want_n, _ = ref[at + j]
            assert idx[j].tolist() == want_idx.tolist() and int(found[j]) == 3
            assert np.array_equal(y_pred[j].cpu().numpy(), want_list) and int(out_len[j].min()) == want_n
        at += 4
    ridx, ry, rlen = lib.query_random(4, [39, 20, 5, 1], seed=3, first=5)
    from dimx.retrieval import random_indices
    assert ridx.cpu().tolist() == random_indices(4, 12, 3, first=5).tolist() and tuple(ry.shape) == (4, 1, 39, 56)
    assert bool((rlen.cpu()[:, 0] <= torch.tensor([39, 20, 5, 1])).all())


@pytest.mark.parametrize("kind", ["audio", "motion"])
def test_baseline_epoch_returns_the_training_listener_the_definition_names(kind):
    from dimx import x_engine_pt
    from dimx.metrics import ListenerMetrics
    ref = _protocol_reference(kind, 1)
    acc = ListenerMetrics()
    y_true, y_pred, x, ids = x_engine_pt.evaluate_baseline_epoch(_library(kind), _test(), _dev(), k=1, metrics=acc)
    assert len(y_true) == len(y_pred) == len(x) == len(ids) == 8 and ids[5] == "clip_600_1_1"
    for j, (want_idx, want_list, want_n, gt) in enumerate(ref):
        assert y_pred[j].shape == (want_n, 56) and np.array_equal(y_pred[j], want_list[0, :want_n]), "clip %d" % j
        assert np.array_equal(y_true[j], gt[:want_n]) and x[j].shape == (want_n, 56)
    m = acc.result()
    assert np.isfinite(m["fid"]) and np.isfinite(m["mse"])
    # strict_len keeps the clips whose retrieved clip has their own length only
    train_lens = [n - 1 for b in _train() for n in b[2]]
    test_lens = [n - 1 for b in _test() for n in b[2]]
    same = [j for j, r in enumerate(ref) if train_lens[int(r[0][0])] == test_lens[j]]
    kept = x_engine_pt.evaluate_baseline_epoch(_library(kind), _test(), _dev(), k=1, strict_len=True)
    assert len(kept[0]) == len(same) and kept[3] == [ids[j] for j in same]
    # the Random baseline: host-drawn picks, reproducible
    r1 = x_engine_pt.evaluate_baseline_epoch(_library(kind), _test(), _dev(), random_seed=11, random_first=5)
    r2 = x_engine_pt.evaluate_baseline_epoch(_library(kind), _test(), _dev(), random_seed=11, random_first=5)
    assert len(r1[1]) == 8 and all(np.array_equal(a, b) for a, b in zip(r1[1], r2[1]))


def test_baseline_epoch_with_a_k_best_list_equals_the_selector_on_the_definitions_list():
    from dimx import x_engine_pt
    from dimx.engine import op_consensus_select, op_fd_select
    ref = _protocol_reference("audio", 4)
    lib = _library("audio")
    lists = torch.from_numpy(np.stack([r[1] for r in ref])).to(_dev())
    lens = [r[2] for r in ref]
    gt = torch.from_numpy(np.stack([r[3] for r in ref])).to(_dev())
    _, y_pred, _, _ = x_engine_pt.evaluate_baseline_epoch(lib, _test(), _dev(), k=4, select="consensus")
    _, win, ok, best = op_consensus_select(lists, lens)
    assert ok.tolist() == [1] * 8
    for j, n in enumerate(lens):
        assert np.array_equal(y_pred[j], best[j, :n].cpu().numpy()), "clip %d" % j
    _, y_pred, _, _ = x_engine_pt.evaluate_baseline_epoch(lib, _test(), _dev(), k=4, select="fd")
    _, _, ok, best = op_fd_select(gt, lists, lens)
    assert ok.tolist() == [1] * 8
    for j, n in enumerate(lens):
        assert np.array_equal(y_pred[j], best[j, :n].cpu().numpy()), "clip %d" % j
    print("k-best consensus winners %s" % (win.tolist(),))


def test_baseline_epoch_refuses_what_it_cannot_do():
    from dimx import lib as L
    from dimx import x_engine_pt
    from dimx.retrieval import RetrievalLibrary
    lib = RetrievalLibrary("audio")
    with pytest.raises(ValueError):
        x_engine_pt.evaluate_baseline_epoch(lib, _test(), _dev(), k=4, select="likelihood")
    with pytest.raises(ValueError):
        x_engine_pt.evaluate_baseline_epoch(lib, _test(), _dev(), k=4)
    with pytest.raises(ValueError):
        x_engine_pt.evaluate_baseline_epoch(lib, _test(), _dev(), k=1, select="best")
    with pytest.raises(L.DimxError):
        x_engine_pt.evaluate_baseline_epoch(lib, _test(), "cpu")
