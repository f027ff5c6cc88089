"""CPU: the definition of the retrieval baselines (dimx.retrieval: pooling, cosine similarity, k-best search, gather, random picks)
against a literal restatement of the reference's loop (code/baselines.py:39-46: one pair at a time, strict ``>`` from -1) written
here, and its documented edge cases."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dimx  # noqa: E402,F401
from dimx import retrieval  # noqa: E402


def _clips(seed, N, T, D, lo=1):
    g = np.random.default_rng(seed)
    x = g.standard_normal((N, T, D)).astype(np.float32)
    lens = g.integers(lo, T + 1, size=N)
    return x, lens


def _literal_pool(x, n, kind):
    v = np.array(x[:n])
    return v.max(axis=0) if kind == "max" else v.mean(axis=0)


def _literal_nn(cur_vector, X):
    """the reference's loop, one pair at a time"""
    best_index, best_sim = 0, -1
    with np.errstate(invalid="ignore", divide="ignore"):
        for j in range(len(X)):
            cur_sim = np.dot(cur_vector, X[j]) / (np.linalg.norm(cur_vector) * np.linalg.norm(X[j]))
            if cur_sim > best_sim:
                best_sim = cur_sim
                best_index = j
    return best_index, best_sim


def _literal_topk(q, X, k):
    """k passes of the reference's loop, each over the entries not yet taken"""
    taken, sims = [], []
    with np.errstate(invalid="ignore", divide="ignore"):
        for _ in range(k):
            best_index, best_sim = -1, -1
            for j in range(len(X)):
                if j in taken:
                    continue
                cur_sim = np.dot(q, X[j]) / (np.linalg.norm(q) * np.linalg.norm(X[j]))
                if cur_sim > best_sim:
                    best_sim, best_index = cur_sim, j
            if best_index < 0:
                break
            taken.append(best_index)
            sims.append(best_sim)
    return taken, sims


@pytest.mark.parametrize("kind,D", [("max", 768), ("mean", 56), ("mean", 9)])
def test_pool_matches_the_literal_descriptor_on_ragged_clips(kind, D):
    x, lens = _clips(1, 7, 39, D)
    lens[0], lens[1] = 1, 39
    for i in range(len(lens)):
        got = retrieval.pool(x[i], lens[i], kind)
        want = _literal_pool(x[i], lens[i], kind)
        assert got.dtype == np.float64 and got.shape == (D,)
        if kind == "max":
            assert np.array_equal(got, want.astype(np.float64))           # exact
        else:
            assert np.allclose(got, want, rtol=0, atol=1e-6)              # the literal mean is float32
            assert np.allclose(got, x[i, :lens[i]].astype(np.float64).mean(axis=0), rtol=1e-13, atol=0)
    assert np.array_equal(retrieval.pool(x[0], 1, kind), x[0, 0].astype(np.float64))      # n = 1: the frame itself
    assert not retrieval.pool(x[0], 0, kind).any()                                         # n = 0: a zero descriptor
    assert np.array_equal(retrieval.pool(x[0], 99, kind), retrieval.pool(x[0], 39, kind))  # clamped to the tensor
    desc, norm = retrieval.pool_batch(x, lens, kind)
    assert desc.shape == (7, D) and np.allclose(norm, np.linalg.norm(desc, axis=1), rtol=1e-14)
    with pytest.raises(ValueError):
        retrieval.pool(x[0], 3, "median")


@pytest.mark.parametrize("kind,D,N", [("max", 768, 37), ("mean", 56, 37), ("mean", 9, 120)])
def test_search_matches_the_literal_loop(kind, D, N):
    x, lens = _clips(2, N, 20, D)
    qx, qlens = _clips(3, 6, 20, D)
    Xd, _ = retrieval.pool_batch(x, lens, kind)
    Qd, _ = retrieval.pool_batch(qx, qlens, kind)
    sim = retrieval.similarities(Qd, Xd)
    idx, s, found = retrieval.search(Qd, Xd, 1)
    assert idx.dtype == np.int32 and idx.shape == (6, 1) and found.tolist() == [1] * 6
    for q in range(6):
        j, best = _literal_nn(Qd[q], Xd)
        assert int(idx[q, 0]) == j and abs(s[q, 0] - best) < 1e-14
        assert np.allclose(sim[q], retrieval.cosine(Qd[q], Xd), rtol=0, atol=0)
    for k in (3, 10, 16):
        idx, s, found = retrieval.search(Qd, Xd, k)
        assert found.tolist() == [k] * 6
        for q in range(6):
            taken, sims = _literal_topk(Qd[q], Xd, k)
            assert idx[q].tolist() == taken and np.allclose(s[q], sims, rtol=0, atol=1e-14)
            assert np.array_equal(s[q], sim[q, idx[q]])
    m = retrieval.margins(sim, 3)
    assert m.shape == (6,) and (m > 0).all()
    top = -np.sort(-sim, axis=1)[:, :4]
    assert np.allclose(m, (top[:, :-1] - top[:, 1:]).min(axis=1), rtol=0, atol=0)


def test_duplicates_zero_descriptors_opposites_and_short_libraries():
    g = np.random.default_rng(5)
    Xd = g.standard_normal((9, 16))
    q = np.sign(g.standard_normal(16))                   # 16 entries of +-1: the norm is 4 and the similarities below are exact
    Xd[6] = Xd[2]                                        # a duplicate: the smaller index wins, the similarities are the same bits
    Xd[4] = 0.0                                          # a zero descriptor: NaN, never chosen
    Xd[7] = -q                                           # exactly opposite: similarity -1, not eligible
    Xd[2] = Xd[6] = 3.0 * q                              # and the duplicate pair is the best match
    sim = retrieval.similarities(q[None], Xd)
    assert np.isnan(sim[0, 4]) and sim[0, 7] == -1.0 and sim[0, 2] == sim[0, 6]
    idx, s, found = retrieval.search(q[None], Xd, 16)    # N < k: unfilled slots
    assert found.tolist() == [7]
    assert idx[0, :2].tolist() == [2, 6] and s[0, 0] == s[0, 1]
    assert 4 not in idx[0].tolist() and 7 not in idx[0].tolist()
    assert idx[0, 7:].tolist() == [-1] * 9 and np.isnan(s[0, 7:]).all() and not np.isnan(s[0, :7]).any()
    assert (np.diff(s[0, :7]) <= 0).all()
    assert _literal_nn(q, Xd)[0] == 2
    # a zero query: nothing is eligible, the reference keeps index 0
    idx, s, found = retrieval.search(np.zeros((1, 16)), Xd, 1)
    assert found.tolist() == [0] and idx.tolist() == [[-1]] and np.isnan(s).all()
    assert retrieval.reference_index(idx).tolist() == [[0]] and _literal_nn(np.zeros(16), Xd)[0] == 0
    assert retrieval.reference_index(np.array([[3, -1]])).tolist() == [[3, 0]]
    # only an opposite entry and a zero entry: nothing found either
    idx, _, found = retrieval.search(q[None], np.stack([-q, np.zeros(16)]), 3)
    assert found.tolist() == [0] and idx.tolist() == [[-1, -1, -1]]
    assert retrieval.margins(sim, 3).shape == (1,) and retrieval.margins(np.array([[np.nan, 0.5]]), 1)[0] == np.inf
    for bad in (0, 17):
        with pytest.raises(ValueError):
            retrieval.search(q[None], Xd, bad)


def test_gather_lengths_and_zero_rows():
    g = np.random.default_rng(6)
    lib = g.standard_normal((5, 11, 4)).astype(np.float32)
    lib_lens = [11, 3, 0, 7, 20]                         # 20: clamped to the tensor
    idx = np.array([[0, 1], [3, -1], [4, 2]], dtype=np.int32)
    q_lens = [5, 9, 11]
    out, out_len = retrieval.gather(lib, lib_lens, idx, q_lens)
    assert out.shape == (3, 2, 11, 4) and out.dtype == np.float32 and out_len.dtype == np.int32
    assert out_len.tolist() == [[5, 3], [7, 0], [11, 0]]
    for q in range(3):
        for s in range(2):
            n = out_len[q, s]
            assert np.array_equal(out[q, s, :n], lib[idx[q, s], :n]) and not out[q, s, n:].any()
    out8, len8 = retrieval.gather(lib, lib_lens, idx, q_lens, L=8)
    assert out8.shape == (3, 2, 8, 4) and len8.tolist() == [[5, 3], [7, 0], [8, 0]]
    assert np.array_equal(out8, out[:, :, :8] * (np.arange(8)[None, None, :, None] < len8[..., None, None]))


def test_random_indices_are_reproducible_and_respect_first():
    a = retrieval.random_indices(200, 50, seed=4)
    assert a.shape == (200, 1) and a.dtype == np.int32 and a.min() >= 0 and a.max() < 50
    assert np.array_equal(a, retrieval.random_indices(200, 50, seed=4))
    assert not np.array_equal(a, retrieval.random_indices(200, 50, seed=5))
    assert len(np.unique(a)) > 5
    b = retrieval.random_indices(200, 50, seed=4, first=5)
    assert b.max() < 5 and set(np.unique(b)) == {0, 1, 2, 3, 4}
    assert retrieval.random_indices(10, 3, seed=1, first=5).max() < 3
    with pytest.raises(ValueError):
        retrieval.random_indices(4, 0, seed=1)


def test_library_kinds():
    assert retrieval.RetrievalLibrary("audio").pooling == "max" and retrieval.RetrievalLibrary("motion").pooling == "mean"
    with pytest.raises(ValueError):
        retrieval.RetrievalLibrary("video")
    with pytest.raises(ValueError):
        retrieval.RetrievalLibrary("audio").buffers()
