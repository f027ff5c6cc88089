"""Host-side metrics of the evaluation step (numpy/scipy, float64), restating
reference code/metrics/eval_utils.py:6-91.  They consume the per-clip arrays the engine returns after the
(all-gathered) generation; they are not on the GPU path (excluded from clips/s).  ``frechet_distances_hip`` is the exception: the
best-of-N selection's distances from the HIP library."""
import numpy as np
from scipy import linalg


def calculate_activation_statistics(activations):
    """eval_utils.py:6-10: mean over frames and unbiased covariance (np.cov, rowvar=False)."""
    return np.mean(activations, axis=0), np.cov(activations, rowvar=False)


def calculate_frechet_distance(mu1, sigma1, mu2, sigma2, eps=1e-6):
    """eval_utils.py:12-46."""
    mu1, mu2 = np.atleast_1d(mu1), np.atleast_1d(mu2)
    sigma1, sigma2 = np.atleast_2d(sigma1), np.atleast_2d(sigma2)
    assert mu1.shape == mu2.shape and sigma1.shape == sigma2.shape
    diff = mu1 - mu2
    covmean, _ = linalg.sqrtm(sigma1.dot(sigma2), disp=False)
    if not np.isfinite(covmean).all():
        offset = np.eye(sigma1.shape[0]) * eps
        covmean = linalg.sqrtm((sigma1 + offset).dot(sigma2 + offset))
    if np.iscomplexobj(covmean):
        if not np.allclose(np.diagonal(covmean).imag, 0, atol=1e-3):
            raise ValueError("Imaginary component {}".format(np.max(np.abs(covmean.imag))))
        covmean = covmean.real
    return diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2 * np.trace(covmean)


def clip_fd(gt, pred):
    m1, s1 = calculate_activation_statistics(gt)
    m2, s2 = calculate_activation_statistics(pred)
    return calculate_frechet_distance(m1, s1, m2, s2)


def frechet_distances_torch(y_true, y_pred, lens):
    """The same Frechet distance for a whole batch at once, in torch float64 on whatever device the tensors live on (the GPU in
    ``evaluate_test_epoch(fd_backend="device")``): y_true [B, L, F], y_pred [B, S, L, F], lens[j] = valid frames of clip j ->
    fd [B, S].  Mean and unbiased covariance over the valid frames as eval_utils.py:6-10; the trace of the matrix square root
    as sum sqrt(eig(A^T S2 A)) with S1 = A A^T (A = V sqrt(L) from eigh) -- the eigenvalues of S1 S2 without a non-symmetric
    Schur form.  Mathematically the reference's quantity; NOT its arithmetic: scipy's sqrtm differs in the last digits and has
    failure modes on rank-deficient covariances (clips shorter than F + 1 frames: complex results, the eps retry, the
    "Imaginary component" ValueError) that this form does not have.  The host path above stays the default."""
    import torch
    B, S, L, F = y_pred.shape
    dev = y_pred.device
    n = torch.as_tensor(lens, dtype=torch.float64, device=dev)
    m = (torch.arange(L, device=dev)[None, :] < n[:, None]).to(torch.float64)           # [B, L]

    def stats(x, mm, nn):                      # x [..., L, F] float64, mm [..., L], nn [...]
        mu = (x * mm[..., None]).sum(-2) / nn[..., None]
        c = (x - mu[..., None, :]) * mm[..., None]
        return mu, c.transpose(-1, -2) @ c / (nn[..., None, None] - 1.0)

    mu1, s1 = stats(y_true.to(torch.float64), m, n)                                      # [B, F], [B, F, F]
    mu2, s2 = stats(y_pred.to(torch.float64), m[:, None].expand(B, S, L), n[:, None].expand(B, S))
    lam, V = torch.linalg.eigh(s1)
    A = V * lam.clamp(min=0).sqrt()[..., None, :]                                        # S1 = A A^T
    M = A.transpose(-1, -2)[:, None] @ s2 @ A[:, None]                                   # [B, S, F, F] symmetric PSD
    M = 0.5 * (M + M.transpose(-1, -2))
    tr_sqrt = torch.linalg.eigvalsh(M).clamp(min=0).sqrt().sum(-1)
    diff = mu1[:, None] - mu2
    tr = lambda t: torch.diagonal(t, dim1=-2, dim2=-1).sum(-1)
    return (diff * diff).sum(-1) + tr(s1)[:, None] + tr(s2) - 2.0 * tr_sqrt


def frechet_distances_hip(y_true, y_pred, lens, cols=(0, None)):
    """The same distances from the project's own kernel (dimx_op_fd_select, csrc/fd_select.hip; float64 throughout, Jacobi
    eigenvalues in LDS, padded frames never read): y_true [B, L, W], y_pred [B, S, L, W] on a GPU, lens[j] = valid frames of
    clip j, cols = (c0, c1) the columns that enter the distance -> fd [B, S] float64 on that GPU.  CPU tensors raise
    lib.DimxError: there is no CPU fallback (frechet_distances_torch and clip_fd above are the host forms)."""
    from .engine import op_fd_select
    return op_fd_select(y_true, y_pred, lens, cols=cols, want_best=False)[0]


def consensus_distances_hip(y_pred, lens, cols=(0, None), distance="fd"):
    """The pairwise distances among the tries of each clip from the project's own kernel (dimx_op_consensus_select,
    csrc/consensus.hip; the definition is dimx.consensus.pairwise_fd / pairwise_l2): y_pred [B, S, L, W] on a GPU -> dist
    [B, S, S] float64 on that GPU, symmetric with a zero diagonal.  CPU tensors raise lib.DimxError."""
    from .engine import op_consensus_select
    return op_consensus_select(y_pred, lens, cols=cols, distance=distance, want_best=False, want_dist=True)[-1]


def sid_device(gt_frames, pred_frames, type="exp"):
    """One fit and two assigns on the GPU, nothing read back: -> f64 [4] on the frames' device = {sid_pred, sid_gt, n_iter, status}
    (status: 0, or the Lloyd iteration at which a cluster was left empty -- the two SID values mean nothing then)."""
    import torch
    from .engine import op_kmeans_fit, op_sid_assign
    from .mymetrics import SID_GROUPS
    k, c0, F = SID_GROUPS[type]
    centers, info = op_kmeans_fit(gt_frames, k, cols=(c0, c0 + F), check=False)
    sid_p = op_sid_assign(pred_frames, centers, cols=(c0, c0 + F))[1]
    sid_g = op_sid_assign(gt_frames, centers, cols=(c0, c0 + F))[1]
    return torch.cat([sid_p, sid_g, info.to(torch.float64)])


def sid_hip(gt_frames, pred_frames, type="exp"):
    """calcuate_sid(gt, pred, type) and calcuate_sid(gt, gt, type) from ONE fit in the HIP library (csrc/kmeans_sid.hip; float64 on
    the f32 values, the definition is mymetrics.sid_f64): gt_frames [N, 56], pred_frames [M, 56] f32 on one GPU, the concatenated
    valid frames of the epoch in clip order (the first centre is an index into that order) -> (sid_pred, sid_gt).  One readback.
    scikit-learn computes in the dtype it is given and the reference hands it float32: this is scikit-learn's value on float64
    copies of the same numbers.  A cluster left empty raises lib.DimxError; CPU tensors raise it too."""
    from .engine import kmeans_empty_cluster_error
    sid_p, sid_g, n_iter, status = sid_device(gt_frames, pred_frames, type).tolist()
    if status:
        raise kmeans_empty_cluster_error(status, "sid_hip(%s)" % type)
    return sid_p, sid_g


def calculate_variance(activations):
    """eval_utils.py:48-49."""
    return np.sum(np.var(activations, axis=0))


def sts(x, y, timestep=0.1):
    """eval_utils.py:85-91, vectorised (same value as the reference's double loop)."""
    dx = np.diff(np.asarray(x, dtype=np.float64), axis=0)
    dy = np.diff(np.asarray(y, dtype=np.float64), axis=0)
    return np.sqrt(np.sum((dx - dy) ** 2) / timestep)


def summarize(y_trues, y_preds):
    """FD / MSE / variance / STS averaged over clips on pose[0:6] and exp[6:56]
    (the quantities reference code/mymetrics.py:7-88 prints that need no clustering)."""
    out = {}
    for name, sl in (("pose", slice(0, 6)), ("exp", slice(6, 56))):
        fds, mses, vars_, stss = [], [], [], []
        for gt, pr in zip(y_trues, y_preds):
            g, p = gt[:, sl], pr[:, sl]
            fds.append(clip_fd(g, p))
            mses.append(np.mean((g - p) ** 2))
            vars_.append(calculate_variance(p))
            stss.append(sts(g, p))
        out[name] = {"fd": float(np.mean(fds)), "mse": float(np.mean(mses)), "var": float(np.mean(vars_)),
                     "sts": float(np.mean(stss))}
    return out


class BiwiMeshMetrics:
    """Device-side accumulator of the DIM-Speaker mesh metrics (reference print_biwi_metrics, code/mymetrics.py:122-182) over the
    batches of an evaluation epoch: ``update`` runs dimx_op_mesh_metrics (csrc/mesh_metrics.hip, float64) on the meshes where they
    lie and adds into float64 state on that GPU -- no mesh crosses to the host and nothing is synchronised; ``result`` does the one
    readback.  CPU tensors raise lib.DimxError (mymetrics.compute_biwi_metrics is the host form)."""

    def __init__(self, mouth_map, upper_map):
        self.mouth_map = [int(i) for i in mouth_map]
        self.upper_map = [int(i) for i in upper_map]
        self._maps = {}        # (device, row width) -> the two MeshMaps
        self._state = None     # f64 [5]: sum of frame maxima, frames, sum of (sigma_gt - sigma_pred), clips, status

    def update(self, y_true, y_pred, lens, template):
        """y_true [B, Lt, 3*Nv], y_pred [B, Lp, 3*Nv] on one GPU, lens[b] valid frames (host sequence), template [B, 3*Nv] or None."""
        import torch
        from .engine import mesh_map, op_mesh_metrics
        n_vert, key = int(y_pred.shape[-1]) // 3, (str(getattr(y_pred, "device", None)), int(y_pred.shape[-1]))
        if getattr(y_pred, "is_cuda", False) and key not in self._maps:      # validated and uploaded once per (device, mesh)
            self._maps[key] = (mesh_map(self.mouth_map, n_vert, y_pred.device, "mouth_map"),
                               mesh_map(self.upper_map, n_vert, y_pred.device, "upper_map"))
        mouth, upper = self._maps.get(key, (self.mouth_map, self.upper_map))
        clip, _, status = op_mesh_metrics(y_true, y_pred, lens, template, mouth, upper, return_status=True)
        add = torch.cat([clip[:, 0].sum(0, keepdim=True), clip[:, 1].sum(0, keepdim=True), (clip[:, 2] - clip[:, 3]).sum(0, keepdim=True),
                         torch.full((1,), float(clip.shape[0]), dtype=torch.float64, device=clip.device), status.to(torch.float64)])
        if self._state is None:
            self._state = add
        else:
            if self._state.device != add.device:
                raise ValueError("BiwiMeshMetrics: updates from %s and %s" % (self._state.device, add.device))
            self._state = torch.cat([self._state[:4] + add[:4], torch.maximum(self._state[4:], add[4:])])
        return self

    def result(self):
        """-> (lve, fdd) as Python floats: frames weigh equally in lve, clips in fdd."""
        if self._state is None:
            raise ValueError("BiwiMeshMetrics.result() before any update()")
        s_max, frames, s_diff, clips, status = self._state.tolist()
        if status != 0:
            raise RuntimeError("BiwiMeshMetrics: a map index outside the mesh reached the kernel and was skipped")
        return s_max / frames, s_diff / clips


class ListenerMetrics:
    """Device-side accumulator of the listener metrics (reference print_metrics / print_metrics_full, code/mymetrics.py:7-120) over
    the batches of an evaluation epoch: ``update`` runs dimx_op_listener_metrics (csrc/listener_metrics.hip, float64) on the
    tensors where they lie and merges its per-clip rows into float64 state on that GPU -- nothing crosses to the host and nothing
    is synchronised; ``result`` does the one readback.  Clips count in update order: the reference's ``sts`` runs over the
    concatenation of all clips, so the step from a clip's last frame to the next clip's first frame is part of it, across batches
    too.  SID stays on the host (``print``) unless the accumulator is built with ``sid=True``: ``update`` then also appends the valid
    frames of y_true and y_pred (56 columns, f32) to buffers on the GPU, in update order (the first KMeans centre is an index into
    that concatenation), and ``result`` runs the fits and assignments there (sid_device, csrc/kmeans_sid.hip) inside its one
    readback.  The gather is built from ``lens``: a host sequence costs no synchronisation, a device tensor is read back once per
    update (the number of valid frames sizes the buffer).  CPU tensors raise lib.DimxError (mymetrics.compute_metrics is the host form).
    Every clip of every batch counts as a clip, as every list entry does in the reference: a clip with fewer than 2 valid frames has
    no covariance, its distances are NaN (the reference's np.cov gives NaN there too) and ``result`` raises ValueError rather than
    return distance means that one such clip has turned into NaN; an empty clip also adds nothing to the MSE means' numerators
    while it counts in their denominator.  Pass only clips with at least 2 valid frames."""

    GROUPS = (("pose", 6), ("exp", 50))

    def __init__(self, sid=False):
        from .engine import LISTENER_WINDOWS
        self.windows = LISTENER_WINDOWS
        self._s = None
        self.sid = bool(sid)
        self._frames = ([], [])    # sid: per update the valid frames [n, 56] f32 of y_true / y_pred
        self._sid_cache = None     # (updates seen, f64 [8] on the GPU)

    def _append_frames(self, y_true, y_pred, lens):
        """the valid frames of the batch in clip order, gathered on the GPU by an index built from lens"""
        import torch
        dev = y_pred.device
        lens_h = [int(n) for n in (lens.tolist() if torch.is_tensor(lens) else lens)]
        Ln = int(min(y_true.shape[1], y_pred.shape[1]))
        lens_h = [min(max(n, 0), Ln) for n in lens_h]
        b_idx = torch.from_numpy(np.repeat(np.arange(len(lens_h), dtype=np.int64), lens_h)).to(dev)
        t_idx = torch.from_numpy(np.concatenate([np.arange(n, dtype=np.int64) for n in lens_h] or [np.zeros(0, np.int64)])).to(dev)
        for buf, y in zip(self._frames, (y_true, y_pred)):
            buf.append(y[b_idx, t_idx, :56].float())

    @staticmethod
    def _merge(na, a, nb, b):
        """Chan's merge of (mean gt, m2 gt, mean pred, m2 pred, mean x, m2 x, c(gt,x), c(pred,x)) over na and nb elements"""
        import torch
        n = na + nb
        f = na * nb / n.clamp(min=1.0)
        w = nb / n.clamp(min=1.0)
        dg, dp, dx = b[0] - a[0], b[2] - a[2], b[4] - a[4]
        return torch.stack([a[0] + dg * w, a[1] + b[1] + dg * dg * f, a[2] + dp * w, a[3] + b[3] + dp * dp * f,
                            a[4] + dx * w, a[5] + b[5] + dx * dx * f, a[6] + b[6] + dg * dx * f, a[7] + b[7] + dp * dx * f])

    def update(self, y_true, y_pred, x, lens):
        """y_true, y_pred [B, L, 56], x [B, L', >=56] on one GPU, lens[b] = valid frames of clip b (a sequence or a tensor)."""
        import torch
        from .engine import op_listener_metrics
        fd, mom = op_listener_metrics(y_true, y_pred, x, lens, windows=tuple(w for _, w in self.windows))
        if self.sid:
            self._append_frames(y_true, y_pred, lens)
        dev, B = mom.device, mom.shape[0]
        n = mom[:, 0]                                              # [B] valid frames
        s = {"clips": (self._s["clips"] if self._s else 0) + B, "fd": fd.sum(0)}
        d_first, d_last = mom[:, 21:77], mom[:, 77:133]
        # the step from the previous non-empty clip's last row of d = gt - pred to this clip's first (empty clips are transparent)
        rows = torch.cat([self._s["last"][None] if self._s else torch.zeros(1, 56, dtype=torch.float64, device=dev), d_last])
        valid = torch.cat([self._s["has_last"][None] if self._s else torch.zeros(1, dtype=torch.bool, device=dev), n > 0])
        idx = torch.where(valid, torch.arange(B + 1, device=dev), torch.full((B + 1,), -1, device=dev)).cummax(0)[0]
        prev = idx[:-1]                                            # per clip: index into rows of the last non-empty clip before it
        step = (d_first - rows[prev.clamp(min=0)]) ** 2
        step = torch.where(((prev >= 0) & (n > 0))[:, None], step, torch.zeros_like(step))
        s["last"], s["has_last"] = rows[idx[-1].clamp(min=0)], idx[-1] >= 0
        nn = n.clamp(min=1.0)
        mse, sts_, stat, cnt = [], [], [], []
        for g, (name, cols) in enumerate(self.GROUPS):
            o = 1 + 10 * g
            lo = 0 if g == 0 else 6
            mse.append((mom[:, o] / (nn * cols)).sum())
            sts_.append(mom[:, o + 9].sum() + step[:, lo:lo + cols].sum())
            ne = n * cols                                          # elements per clip
            tot = ne.sum()
            t1 = tot.clamp(min=1.0)
            mg, mp, mx = [(ne * mom[:, o + k]).sum() / t1 for k in (1, 3, 5)]
            dg, dp, dx = mom[:, o + 1] - mg, mom[:, o + 3] - mp, mom[:, o + 5] - mx
            stat.append(torch.stack([mg, mom[:, o + 2].sum() + (ne * dg * dg).sum(), mp, mom[:, o + 4].sum() + (ne * dp * dp).sum(),
                                     mx, mom[:, o + 6].sum() + (ne * dx * dx).sum(), mom[:, o + 7].sum() + (ne * dg * dx).sum(),
                                     mom[:, o + 8].sum() + (ne * dp * dx).sum()]))
            cnt.append(tot)
        mse.append(((mom[:, 1] + mom[:, 11]) / (nn * 56)).sum())
        s["mse"], s["sts"], s["cnt"] = torch.stack(mse), torch.stack(sts_), torch.stack(cnt)
        if self._s is None:
            s["stat"] = stat
        else:
            if self._s["fd"].device != dev:
                raise ValueError("ListenerMetrics: updates from %s and %s" % (self._s["fd"].device, dev))
            for k in ("fd", "mse", "sts"):
                s[k] = self._s[k] + s[k]
            s["stat"] = [self._merge(self._s["cnt"][g], self._s["stat"][g], s["cnt"][g], stat[g]) for g in range(2)]
            s["cnt"] = self._s["cnt"] + s["cnt"]
        self._s = s
        return self

    def result(self):
        """-> the dict of mymetrics.compute_metrics(with_sid=False) merged with mymetrics.compute_metrics_full: floats, and
        (gt, pred) pairs for the var_* entries.  The one readback."""
        import torch
        if self._s is None:
            raise ValueError("ListenerMetrics.result() before any update()")
        s = self._s
        parts = [s["fd"], s["mse"], s["sts"], s["cnt"], s["stat"][0], s["stat"][1]]
        if self.sid:
            if self._sid_cache is None or self._sid_cache[0] != len(self._frames[0]):
                gt, pr = (torch.cat(buf) for buf in self._frames)
                self._sid_cache = (len(self._frames[0]), torch.cat([sid_device(gt, pr, t) for t in ("pose", "exp")]))
            parts.append(self._sid_cache[1])
        flat = torch.cat(parts).tolist()
        nw = len(self.windows)
        clips = float(s["clips"])
        fd, mse, sts_, cnt = flat[:nw], flat[nw:nw + 3], flat[nw + 3:nw + 5], flat[nw + 5:nw + 7]
        st = [flat[nw + 7:nw + 15], flat[nw + 15:nw + 23]]
        if any(v != v for v in fd):
            raise ValueError("ListenerMetrics: a clip with fewer than 2 valid frames was passed to update(): its Frechet distances "
                             "are NaN and so is every distance mean of the epoch")
        out = {name: v / clips for (name, _), v in zip(self.windows, fd)}
        out["mse_pose"], out["mse_exp"], out["mse"] = mse[0] / clips, mse[1] / clips, mse[2] / clips
        for g, (name, _) in enumerate(self.GROUPS):
            mg, m2g, mp, m2p, mx, m2x, cgx, cpx = st[g]
            out["var_" + name] = (m2g / cnt[g], m2p / cnt[g])
            out["rpcc_" + name] = float(abs(cgx / np.sqrt(m2g * m2x) - cpx / np.sqrt(m2p * m2x)))
            out["sts_" + name] = float(np.sqrt(sts_[g] / 0.1))
        # all 56 columns: Chan's merge of the two groups
        n, f = cnt[0] + cnt[1], cnt[0] * cnt[1] / (cnt[0] + cnt[1])
        out["var"] = tuple((st[0][k] + st[1][k] + (st[1][k - 1] - st[0][k - 1]) ** 2 * f) / n for k in (1, 3))
        if self.sid:
            from .engine import kmeans_empty_cluster_error
            for i, t in enumerate(("pose", "exp")):
                sid_p, sid_g, _, status = flat[nw + 23 + 4 * i:nw + 27 + 4 * i]
                if status:
                    raise kmeans_empty_cluster_error(status, "ListenerMetrics(sid=True), sid_%s" % t)
                out["sid_" + t] = (sid_p, sid_g)
        return out

    def print(self, y_true=None, y_pred=None):
        """The lines of print_metrics and then print_metrics_full, in their order and format.  The two SID lines come from the GPU
        when the accumulator was built with ``sid=True``; otherwise they need the per-clip lists (host KMeans,
        mymetrics.calcuate_sid) and are left out without them.  Returns the dict of ``result``."""
        from .mymetrics import calcuate_sid
        m = self.result()
        for k in ("fid_pose", "fid_exp", "pfid_pose", "pfid_exp", "mse_pose", "mse_exp"):
            print(k + ": ", m[k])
        if self.sid:
            for t in ("pose", "exp"):
                print("sid_%s: " % t, *m["sid_" + t])
        elif y_true is not None and y_pred is not None:
            for t in ("pose", "exp"):
                m["sid_" + t] = (calcuate_sid(y_true, y_pred, t), calcuate_sid(y_true, y_true, t))
                print("sid_%s: " % t, *m["sid_" + t])
        print("var_pose: ", *m["var_pose"])
        print("var_exp: ", *m["var_exp"])
        print("rpcc pose: ", m["rpcc_pose"])
        print("rpcc exp: ", m["rpcc_exp"])
        print("sts pose: ", m["sts_pose"])
        print("sts exp: ", m["sts_exp"])
        print("fid: ", m["fid"])
        print("pfid: ", m["pfid"])
        print("mse: ", m["mse"])
        print("var: ", *m["var"])
        return m
