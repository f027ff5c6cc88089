"""``print_metrics`` / ``print_metrics_full`` with the output format and values of reference
``code/mymetrics.py:7-130`` (what ``test_s2s_pretrain.py:68-69`` calls after ``evaluate_test_epoch``).

Inputs are the per-clip lists the evaluation engine returns: ``y_true[i]``, ``y_pred[i]`` ``[len_i-1, 56]`` and the
speaker motion ``x[i]`` ``[len_i-1, >=56]`` (numpy).  Host-side numpy/scipy/sklearn, float64 like the reference;
the per-clip double loop of the reference's ``sts`` is vectorised (same value).  Both functions also RETURN what
they print (the reference returns only ``(fid_pose, fid_exp)`` from ``print_metrics``; that pair stays the return
value, the full dict is available through ``compute_metrics``).

``print_biwi_metrics`` (reference ``code/mymetrics.py:122-182``, what ``test_biwi.py`` and ``finetune_s2s_pretrain.py`` import) is
restated at the end: Lip Vertex Error and upper-Face Dynamics Deviation of vertex clips, in the inputs' own dtype.
"""
import os
import pickle

import numpy as np

from .metrics import calculate_activation_statistics, calculate_frechet_distance, sts


def calcuate_sid(gt, pred, type="exp"):
    """reference code/metrics/eval_utils.py:51-83 (name kept, typo included): entropy of the histogram of the
    predictions over a KMeans codebook (k = 40 exp / 20 pose, random_state 0) fitted on the ground truth."""
    from sklearn.cluster import KMeans
    k = 40 if type == "exp" else 20
    sl = slice(6, None) if type == "exp" else slice(0, 6)
    merge_gt = np.concatenate(gt, axis=0)[:, sl]
    km = KMeans(n_clusters=k, random_state=0, n_init="auto").fit(merge_gt)
    lab = km.predict(np.concatenate(pred, axis=0)[:, sl])
    hist = np.bincount(lab, minlength=k).astype(np.float64)
    hist = hist / hist.sum()
    return float(-np.sum(hist * np.log2(hist + 1e-6)))


def _fd(a, b):
    mu1, s1 = calculate_activation_statistics(a)
    mu2, s2 = calculate_activation_statistics(b)
    return calculate_frechet_distance(mu1, s1, mu2, s2)


def compute_metrics(y_true, y_pred, x, with_sid=True):
    gt, pred = y_true, y_pred
    pose, exp = slice(0, 6), slice(6, None)
    out = {}
    out["fid_pose"] = float(np.mean([_fd(g[:, pose], p[:, pose]) for g, p in zip(gt, pred)]))
    out["fid_exp"] = float(np.mean([_fd(g[:, exp], p[:, exp]) for g, p in zip(gt, pred)]))
    out["pfid_pose"] = float(np.mean([_fd(np.concatenate([xi[:, 0:6], g[:, pose]], -1),
                                          np.concatenate([xi[:, 0:6], p[:, pose]], -1)) for g, p, xi in zip(gt, pred, x)]))
    out["pfid_exp"] = float(np.mean([_fd(np.concatenate([xi[:, 6:], g[:, exp]], -1),
                                         np.concatenate([xi[:, 6:], p[:, exp]], -1)) for g, p, xi in zip(gt, pred, x)]))
    out["mse_pose"] = float(np.mean([np.mean((g[:, pose] - p[:, pose]) ** 2) for g, p in zip(gt, pred)]))
    out["mse_exp"] = float(np.mean([np.mean((g[:, exp] - p[:, exp]) ** 2) for g, p in zip(gt, pred)]))
    if with_sid:
        out["sid_pose"] = (calcuate_sid(gt, pred, "pose"), calcuate_sid(gt, gt, "pose"))
        out["sid_exp"] = (calcuate_sid(gt, pred, "exp"), calcuate_sid(gt, gt, "exp"))
    g = np.concatenate(gt, axis=0).reshape(-1, 56)
    p = np.concatenate(pred, axis=0).reshape(-1, 56)
    out["var_pose"] = (float(np.var(g[:, pose].reshape(-1))), float(np.var(p[:, pose].reshape(-1))))
    out["var_exp"] = (float(np.var(g[:, exp].reshape(-1))), float(np.var(p[:, exp].reshape(-1))))
    xs = np.concatenate(x, axis=0)[:, 0:56]

    def pcc(a, b):
        return np.corrcoef(a.reshape(-1), b.reshape(-1))[0, 1]
    out["rpcc_pose"] = float(abs(pcc(g[:, pose], xs[:, pose]) - pcc(p[:, pose], xs[:, pose])))
    out["rpcc_exp"] = float(abs(pcc(g[:, exp], xs[:, exp]) - pcc(p[:, exp], xs[:, exp])))
    out["sts_pose"] = float(sts(g[:, pose], p[:, pose]))
    out["sts_exp"] = float(sts(g[:, exp], p[:, exp]))
    return out


def print_metrics(y_true, y_pred, x):
    m = compute_metrics(y_true, y_pred, x)
    print("fid_pose: ", m["fid_pose"])
    print("fid_exp: ", m["fid_exp"])
    print("pfid_pose: ", m["pfid_pose"])
    print("pfid_exp: ", m["pfid_exp"])
    print("mse_pose: ", m["mse_pose"])
    print("mse_exp: ", m["mse_exp"])
    print("sid_pose: ", *m["sid_pose"])
    print("sid_exp: ", *m["sid_exp"])
    print("var_pose: ", *m["var_pose"])
    print("var_exp: ", *m["var_exp"])
    print("rpcc pose: ", m["rpcc_pose"])
    print("rpcc exp: ", m["rpcc_exp"])
    print("sts pose: ", m["sts_pose"])
    print("sts exp: ", m["sts_exp"])
    return m["fid_pose"], m["fid_exp"]


def compute_metrics_full(y_true, y_pred, x):
    gt, pred = y_true, y_pred
    out = {"fid": float(np.mean([_fd(g, p) for g, p in zip(gt, pred)])),
           "pfid": float(np.mean([_fd(np.concatenate([xi, g], -1), np.concatenate([xi, p], -1))
                                  for g, p, xi in zip(gt, pred, x)])),
           "mse": float(np.mean([np.mean((g - p) ** 2) for g, p in zip(gt, pred)]))}
    g = np.concatenate(gt, axis=0).reshape(-1, 56)
    p = np.concatenate(pred, axis=0).reshape(-1, 56)
    out["var"] = (float(np.var(g.reshape(-1))), float(np.var(p.reshape(-1))))
    return out


def print_metrics_full(y_true, y_pred, x):
    m = compute_metrics_full(y_true, y_pred, x)
    print("fid: ", m["fid"])
    print("pfid: ", m["pfid"])
    print("mse: ", m["mse"])
    print("var: ", *m["var"])
    return m


# ---------------------------------------------------------------- BIWI mesh metrics (reference code/mymetrics.py:122-182)
BIWI_TEMPLATES_PATH = "../data/BIWI_data/templates.pkl"
BIWI_REGION_PATH = "../data/CodeTalker/BIWI/regions/"


def read_region_map(path):
    """``lve.txt`` / ``fdd.txt``: vertex indices separated by ``", "`` (reference :128-134)."""
    with open(path) as f:
        return [int(i) for i in f.read().split(", ")]


def read_biwi_templates(path):
    """``templates.pkl``: {subject: [Nv, 3] array}, a Python-2 pickle read with ``encoding='latin1'`` (reference :125-126)."""
    with open(path, "rb") as fin:
        return pickle.load(fin, encoding="latin1")


def _clip_template(templates, i, file_names):
    if templates is None:
        return None
    if isinstance(templates, dict):
        return np.asarray(templates[file_names[i].split("_")[0]])
    return np.asarray(templates[i])


def compute_biwi_metrics(y_true, y_pred, file_names, templates, mouth_map, upper_map):
    """The values ``print_biwi_metrics`` prints, vectorised, in the dtype numpy gives the inputs (float32 clips stay float32, as in
    the reference; nothing is upcast).  ``y_true[i]`` ``[Tg_i, 3*Nv]`` (or ``[Tg_i, Nv, 3]``), ``y_pred[i]`` with at least ``Tg_i``
    frames, of which the first ``Tg_i`` count; ``templates`` a dict keyed on the subject ``file_names[i].split("_")[0]`` (the
    reference's), a per-clip sequence, or None (zero template); the maps are vertex indices, duplicates counting as numpy fancy
    indexing counts them.  Nv comes from the data (the reference hard-codes 23370).

        lve = mean over all frames of all clips of max_m |gt - pred|^2
        fdd = mean over clips of sigma_gt - sigma_pred,  sigma_x = mean_u std_t |x - template|^2   (population std)

    Returns a dict: ``lve``, ``fdd``, ``fdd_scale`` = mean over clips of (sigma_gt + sigma_pred) (what an error of fdd is relative
    to: fdd itself is a difference and may be near 0), and the per-clip arrays ``frame_max`` (list of [Tg_i]), ``frames``,
    ``sigma_gt``, ``sigma_pred``."""
    mouth = np.asarray(mouth_map, dtype=np.int64).reshape(-1)
    upper = np.asarray(upper_map, dtype=np.int64).reshape(-1)
    frame_max, frames, sig_gt, sig_pred, diffs = [], [], [], [], []
    for i in range(len(y_true)):
        gt = np.asarray(y_true[i])
        gt = gt.reshape(gt.shape[0], -1, 3)
        nv = gt.shape[1]
        pred = np.asarray(y_pred[i])
        pred = pred.reshape(pred.shape[0], -1, 3)
        if pred.shape[0] < gt.shape[0] or pred.shape[1] != nv:
            raise ValueError("clip %d: prediction %s against ground truth %s (at least as many frames and the same vertices are needed)"
                             % (i, pred.shape, gt.shape))
        for name, mp in (("mouth_map", mouth), ("upper_map", upper)):
            if mp.size and (mp.min() < 0 or mp.max() >= nv):
                raise ValueError("%s holds an index outside [0, %d)" % (name, nv))
        pred = pred[:gt.shape[0]]
        t = _clip_template(templates, i, file_names)
        sig = []
        for x in (gt, pred):
            xu = x[:, upper, :]
            motion = xu if t is None else xu - t.reshape(1, nv, 3)[:, upper, :]
            s = np.sum(np.square(motion), axis=2)                    # [T, n_upper]
            sig.append(np.mean(np.std(s, axis=0)) if upper.size else s.dtype.type(0))
        sig_gt.append(sig[0])
        sig_pred.append(sig[1])
        diffs.append(sig[0] - sig[1])
        d = np.sum(np.square(gt[:, mouth, :] - pred[:, mouth, :]), axis=2)   # [T, n_mouth]
        frame_max.append(np.max(d, axis=1) if mouth.size else np.zeros(gt.shape[0], d.dtype))
        frames.append(gt.shape[0])
    lve = np.mean(np.concatenate(frame_max))
    fdd = sum(diffs) / len(diffs)
    scale = sum(a + b for a, b in zip(sig_gt, sig_pred)) / len(diffs)
    return {"lve": lve, "fdd": fdd, "fdd_scale": scale, "frame_max": frame_max, "frames": np.asarray(frames),
            "sigma_gt": np.asarray(sig_gt), "sigma_pred": np.asarray(sig_pred)}


def print_biwi_metrics(y_true, y_pred, file_names, templates=None, mouth_map=None, upper_map=None,
                       templates_path=BIWI_TEMPLATES_PATH, region_path=BIWI_REGION_PATH):
    """reference :122-182: prints ``Lip Vertex Error`` and ``FDD`` and returns ``(lve, fdd)``.  ``templates`` / ``mouth_map`` /
    ``upper_map`` left None are read from the reference's files (``templates.pkl``, ``lve.txt``, ``fdd.txt``)."""
    if templates is None:
        templates = read_biwi_templates(templates_path)
    if mouth_map is None:
        mouth_map = read_region_map(os.path.join(region_path, "lve.txt"))
    if upper_map is None:
        upper_map = read_region_map(os.path.join(region_path, "fdd.txt"))
    m = compute_biwi_metrics(y_true, y_pred, file_names, templates, mouth_map, upper_map)
    print('Lip Vertex Error: {:.4e}'.format(m["lve"]))
    print('FDD: {:.4e}'.format(m["fdd"]))
    return m["lve"], m["fdd"]


# ---------------------------------------------------------------- SID without scikit-learn (reference code/metrics/eval_utils.py:51-83)
# The definition of the HIP operator (csrc/kmeans_sid.hip): KMeans(k, random_state=0, n_init='auto') as scikit-learn's lloyd path
# computes it on float64 inputs, restated in numpy.  calcuate_sid above stays the reference's own call.
SID_GROUPS = {"pose": (20, 0, 6), "exp": (40, 6, 50)}     # type -> (k, first column, columns)


def kmeans_draws(n, k, seed=0):
    """The random numbers KMeans(random_state=seed, n_init='auto', init='k-means++') consumes for n samples and k clusters, in its
    order; none depends on the data: one ``choice(n, p=uniform)`` (the first centre), then per further centre one
    ``uniform(size=2 + int(ln k))``.  -> (first_index, U [(k - 1), trials] float64)."""
    rs = np.random.RandomState(seed)
    trials = 2 + int(np.log(k))
    first = int(rs.choice(n, p=np.full(n, 1.0) / float(n)))
    u = np.empty((max(k - 1, 0), trials), dtype=np.float64)
    for c in range(k - 1):
        u[c] = rs.uniform(size=trials)
    return first, u


def _sq_dist_rows(c, X):
    """[len(c), N] squared distances, summed over the columns directly (no |x|^2 - 2 x.c + |c|^2 cancellation)."""
    return np.stack([np.sum((X - row) ** 2, axis=1) for row in c])


def kmeans_assign_f64(X, centers):
    """Nearest centre per row of X, the first index on ties; scikit-learn's lloyd form argmin_k (|c_k|^2 - 2 x.c_k)."""
    X, centers = np.asarray(X, dtype=np.float64), np.asarray(centers, dtype=np.float64)
    return np.argmin(np.sum(centers * centers, axis=1)[None, :] - 2.0 * (X @ centers.T), axis=1)


def kmeans_fit_f64(X, k, draws, tol=1e-4, max_iter=300):
    """scikit-learn's KMeans fit (init='k-means++', one initialisation, algorithm='lloyd') in float64 with the random numbers of
    ``kmeans_draws`` -> (centers [k, F], n_iter, status).  status 0, or the (1-based) iteration at which a cluster was left without
    points: scikit-learn relocates such a centre, this restatement and the operator stop there and say so."""
    X = np.asarray(X, dtype=np.float64)
    n, F = X.shape
    first, U = draws
    if n < k:
        raise ValueError("kmeans_fit_f64: %d samples for %d clusters" % (n, k))
    tol_abs = tol * float(np.mean(np.var(X, axis=0)))
    mean = X.mean(axis=0)
    X = X - mean
    centers = np.empty((k, F), dtype=np.float64)
    centers[0] = X[first]
    closest = _sq_dist_rows(centers[:1], X)[0]
    for c in range(1, k):
        pot = float(np.sum(closest))
        ids = np.searchsorted(np.cumsum(closest), U[c - 1] * pot)
        np.clip(ids, None, n - 1, out=ids)
        cand = np.minimum(closest[None, :], _sq_dist_rows(X[ids], X))
        best = int(np.argmin(cand.sum(axis=1)))
        centers[c], closest = X[ids[best]], cand[best]
    labels_old = np.full(n, -1, dtype=np.int64)
    n_iter, status = 0, 0
    for it in range(max_iter):
        labels = kmeans_assign_f64(X, centers)
        counts = np.bincount(labels, minlength=k)
        sums = np.stack([np.bincount(labels, weights=X[:, c], minlength=k) for c in range(F)], axis=1)
        n_iter = it + 1
        if (counts == 0).any():
            status = n_iter
            break
        new = sums * (1.0 / counts)[:, None]
        shift = np.sqrt(np.sum((new - centers) ** 2, axis=1))
        centers = new
        if np.array_equal(labels, labels_old) or float(np.sum(shift ** 2)) <= tol_abs:
            break
        labels_old = labels
    return centers + mean, n_iter, status


def sid_entropy(labels, k):
    hist = np.bincount(labels, minlength=k).astype(np.float64)
    hist = hist / hist.sum()
    return float(-np.sum(hist * np.log2(hist + 1e-6)))


def sid_f64(gt_frames, pred_frames, type="exp"):
    """calcuate_sid(gt, pred, type) and calcuate_sid(gt, gt, type) from ONE fit, float64 on the values given: gt_frames / pred_frames
    are the concatenated frames [N, 56] / [M, 56] (or per-clip lists) -> (sid_pred, sid_gt).  An empty cluster raises ValueError."""
    k, c0, F = SID_GROUPS[type]
    cat = lambda a: np.concatenate(a, axis=0) if isinstance(a, (list, tuple)) else np.asarray(a)
    g = cat(gt_frames)[:, c0:c0 + F].astype(np.float64)
    p = cat(pred_frames)[:, c0:c0 + F].astype(np.float64)
    centers, n_iter, status = kmeans_fit_f64(g, k, kmeans_draws(g.shape[0], k))
    if status:
        raise ValueError("sid_f64: a cluster was left empty at iteration %d (scikit-learn would relocate it: mymetrics.calcuate_sid)" % status)
    return sid_entropy(kmeans_assign_f64(p, centers), k), sid_entropy(kmeans_assign_f64(g, centers), k)
