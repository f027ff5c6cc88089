"""Retrieval baselines (reference code/baselines.py:30-103: "NN audio", "NN motion", "Random"): the definition (numpy float64, no
GPU needed) of what dimx_op_pool_desc / dimx_op_nn_search / dimx_op_nn_gather compute (csrc/retrieval.hip, include/dimx.h), and
RetrievalLibrary, the device-side library built on those operators.

A clip is described by one vector: the per-dimension maximum over time of its audio features [T, 768] (NN audio) or the mean over
time of the speaker motion [T, 56] (NN motion).  A test clip's prediction is the listener sequence of the training clip whose
descriptor has the largest cosine similarity to its own; the reference starts from ``best_sim = -1, best_index = 0`` and replaces on
a strict ``>``, so the first maximum wins and a similarity of -1 or NaN (a zero descriptor: 0 / 0) is never chosen.  The k best
training clips of a test clip form an n-best list that the selectors of dimx.x_engine_pt rank as they rank generated tries.
"""
import numpy as np

KINDS = {"max": 0, "mean": 1}
FEATURES = {"audio": "max", "motion": "mean"}     # RetrievalLibrary(kind) -> pooling
MAX_K = 16


def kind_index(kind):
    """"max" / "mean" -> the ``kind`` of dimx_op_pool_desc; anything else raises ValueError"""
    if kind not in KINDS:
        raise ValueError("pooling kind %r: one of 'max', 'mean'" % (kind,))
    return KINDS[kind]


def pool(x, n, kind):
    """x [T, D] float32, the first ``n`` frames (clamped to 0..T) -> descriptor [D] float64.  "max": the maximum of the f32 values,
    widened (exact).  "mean": the float64 sum in frame order from zero, divided by n.  n == 0 gives a zero descriptor."""
    kind_index(kind)
    x = np.asarray(x, dtype=np.float32)
    assert x.ndim == 2, "x [T, D] expected, got %s" % (x.shape,)
    n = min(max(int(n), 0), x.shape[0])
    if n == 0:
        return np.zeros(x.shape[1], dtype=np.float64)
    if kind == "max":
        return x[:n].max(axis=0).astype(np.float64)
    acc = np.zeros(x.shape[1], dtype=np.float64)
    for t in range(n):
        acc += x[t].astype(np.float64)
    return acc / float(n)


def pool_batch(x, lens, kind):
    """x [N, T, D], lens [N] -> (desc [N, D] f64, norm [N] f64): pool per clip and the Euclidean norm of each descriptor"""
    desc = np.stack([pool(x[i], lens[i], kind) for i in range(len(lens))]) if len(lens) else np.zeros((0, np.shape(x)[-1]))
    return desc, np.sqrt((desc * desc).sum(axis=1))


def cosine(q, X, q_norm=None, X_norm=None):
    """q [D], X [N, D] float64 -> sim [N] = dot(q, x) / (|q| |x|) in float64.  A zero norm gives NaN, as the reference's 0 / 0."""
    q = np.asarray(q, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64).reshape(-1, q.shape[0])
    qn = np.sqrt((q * q).sum()) if q_norm is None else float(q_norm)
    Xn = np.sqrt((X * X).sum(axis=1)) if X_norm is None else np.asarray(X_norm, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (X @ q) / (qn * Xn)


def similarities(Qd, Xd):
    """Qd [Q, D], Xd [N, D] -> sim [Q, N] float64 (cosine per query)"""
    Qd, Xd = np.asarray(Qd, dtype=np.float64), np.asarray(Xd, dtype=np.float64)
    return np.stack([cosine(q, Xd) for q in Qd]) if len(Qd) else np.zeros((0, len(Xd)))


def top_k(sim, k):
    """sim [Q, N] -> (idx int32 [Q, k], sim f64 [Q, k], found int32 [Q]): per query the k best library entries under the total order
    (similarity descending, index ascending); an entry is eligible only if its similarity is not NaN and is > -1 (the reference's
    strict ``>`` from ``best_sim = -1``).  Unfilled slots hold -1 / NaN."""
    sim = np.asarray(sim, dtype=np.float64)
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError("k=%d outside 1..%d" % (k, MAX_K))
    Q, N = sim.shape
    idx = np.full((Q, k), -1, dtype=np.int32)
    out = np.full((Q, k), np.nan, dtype=np.float64)
    found = np.zeros(Q, dtype=np.int32)
    for q in range(Q):
        ok = np.flatnonzero(~np.isnan(sim[q]) & (sim[q] > -1.0))
        order = ok[np.lexsort((ok, -sim[q, ok]))][:k]
        found[q] = len(order)
        idx[q, :len(order)] = order
        out[q, :len(order)] = sim[q, order]
    return idx, out, found


def search(Qd, Xd, k):
    """Qd [Q, D], Xd [N, D] float64 descriptors -> (idx [Q, k], sim [Q, k], found [Q]) as top_k leaves them.  k = 1 with found == 0
    is the case where the reference keeps index 0: ``idx`` reports -1 and reference_index maps it."""
    return top_k(similarities(Qd, Xd), k)


def reference_index(idx):
    """the reference's ``best_index``: a query for which no entry was eligible keeps its initial index 0"""
    idx = np.asarray(idx)
    return np.where(idx < 0, 0, idx).astype(np.int32)


def gather(lib_seq, lib_lens, idx, q_lens, L=None):
    """lib_seq [N, Lmax, W] f32, lib_lens [N], idx [Q, k] (-1 = no entry), q_lens [Q] -> (out [Q, k, L, W] f32, out_len [Q, k] int32):
    out_len[q, s] = min(q_lens[q], lib_lens[idx[q, s]]) (each clamped to its tensor, and to L), the rows at and beyond it zero; an
    idx of -1 gives zeros and length 0.  L defaults to Lmax."""
    lib_seq = np.asarray(lib_seq, dtype=np.float32)
    idx = np.asarray(idx)
    N, Lmax, W = lib_seq.shape
    L = Lmax if L is None else int(L)
    Q, k = idx.shape
    out = np.zeros((Q, k, L, W), dtype=np.float32)
    out_len = np.zeros((Q, k), dtype=np.int32)
    for q in range(Q):
        for s in range(k):
            i = int(idx[q, s])
            if 0 <= i < N:
                n = min(max(int(q_lens[q]), 0), min(max(int(lib_lens[i]), 0), Lmax), L)
                out[q, s, :n] = lib_seq[i, :n]
                out_len[q, s] = n
    return out, out_len


def random_indices(Q, N, seed, first=None):
    """The Random baseline's picks, drawn on the host (they do not depend on the data): Q indices uniform in [0, N), or in
    [0, min(first, N)) -- ``first=5`` reproduces the checked-in script's leftover ``np.random.randint(0, 5)``.  int32 [Q, 1]."""
    hi = int(N) if first is None else min(int(first), int(N))
    if hi < 1:
        raise ValueError("random_indices: nothing to draw from (N=%d, first=%r)" % (N, first))
    return np.random.default_rng(int(seed)).integers(0, hi, size=(int(Q), 1)).astype(np.int32)


def margins(sim_matrix, k):
    """sim [Q, N] -> per query the smallest gap between neighbours among its top k + 1 eligible similarities: a query whose margin
    is below the error of an evaluation of the similarities may legitimately get another list there.  inf with fewer than two
    eligible entries."""
    sim = np.asarray(sim_matrix, dtype=np.float64)
    out = np.full(sim.shape[0], np.inf)
    for q in range(sim.shape[0]):
        s = sim[q][~np.isnan(sim[q]) & (sim[q] > -1.0)]
        top = np.sort(s)[::-1][:int(k) + 1]
        if len(top) >= 2:
            out[q] = float(np.min(top[:-1] - top[1:]))
    return out


class RetrievalLibrary:
    """The training clips of a retrieval baseline on one GPU: ``add`` pools a batch (dimx.engine.op_pool_desc) and appends
    descriptors, norms, listener sequences and lengths to device buffers; ``query`` pools the test batch, searches
    (op_nn_search) and gathers the k nearest clips' listener sequences (op_nn_gather).  Nothing is synchronised or copied to the
    host.  kind "audio" = per-dimension maximum over time, "motion" = mean over time (reference code/baselines.py:39, 67)."""

    def __init__(self, kind="audio"):
        if kind not in FEATURES:
            raise ValueError("RetrievalLibrary kind %r: one of 'audio', 'motion'" % (kind,))
        self.kind, self.pooling = kind, FEATURES[kind]
        self._parts = []        # per add: (desc, norm, listener [n, L, W], lens)
        self._cat = None

    def __len__(self):
        return sum(int(p[0].shape[0]) for p in self._parts)

    def add(self, features, listener, lens, listener_lens=None):
        """features [B, T, D] f32 and listener [B, L, W] f32 on one GPU, lens[b] = valid frames of clip b's features;
        listener_lens (default lens) = valid frames of its listener sequence."""
        import torch
        from .engine import _lens_i32, op_pool_desc
        desc, norm = op_pool_desc(features, lens, self.pooling)
        B = int(features.shape[0])
        ll = _lens_i32(lens if listener_lens is None else listener_lens, features.device, B, "RetrievalLibrary.add")
        if not (torch.is_tensor(listener) and listener.is_cuda and listener.dim() == 3 and listener.shape[0] == B):
            raise ValueError("RetrievalLibrary.add: listener [B, L, W] on the features' GPU expected")
        self._parts.append((desc, norm, listener.float(), ll))
        self._cat = None
        return self

    def buffers(self):
        """-> (desc [N, D] f64, norm [N] f64, listener [N, Lmax, W] f32 zero-padded, lens [N] int32), concatenated once per change"""
        import torch
        if not self._parts:
            raise ValueError("RetrievalLibrary: empty library")
        if self._cat is None:
            Lmax = max(int(p[2].shape[1]) for p in self._parts)
            seqs = [p[2] if p[2].shape[1] == Lmax else torch.nn.functional.pad(p[2], (0, 0, 0, Lmax - p[2].shape[1])) for p in self._parts]
            self._cat = (torch.cat([p[0] for p in self._parts]), torch.cat([p[1] for p in self._parts]), torch.cat(seqs),
                         torch.cat([p[3] for p in self._parts]))
        return self._cat

    def query(self, features, lens, k=1, out_lens=None, L=None):
        """features [Q, T, D], lens [Q] -> (idx [Q, k] int32, sim [Q, k] f64, found [Q] int32, y_pred [Q, k, L, W] f32, out_len [Q, k]
        int32); out_lens (default lens) are the lengths the gathered sequences are cut to."""
        from .engine import op_nn_gather, op_nn_search, op_pool_desc
        desc, norm, seq, ll = self.buffers()
        qd, qn = op_pool_desc(features, lens, self.pooling)
        idx, sim, found = op_nn_search(qd, qn, desc, norm, k)
        y_pred, out_len = op_nn_gather(seq, ll, idx, lens if out_lens is None else out_lens, L=L)
        return idx, sim, found, y_pred, out_len

    def query_random(self, Q, lens, seed, first=None, L=None):
        """The Random baseline: -> (idx [Q, 1], y_pred [Q, 1, L, W], out_len [Q, 1]) for host-drawn indices (random_indices)"""
        import torch
        from .engine import op_nn_gather
        _, _, seq, ll = self.buffers()
        idx = torch.from_numpy(random_indices(Q, len(self), seed, first)).to(seq.device, non_blocking=True)
        y_pred, out_len = op_nn_gather(seq, ll, idx, lens, L=L)
        return idx, y_pred, out_len
