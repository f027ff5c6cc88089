"""Sampler filters of generation: top-k, nucleus (top-p), min-p and top-a.  Host definition, numpy float64, no GPU.

This module is the contract the HIP sampler (``sample_kernel`` in csrc/elementwise.hip) is tested against.  It restates the
``filter_logits_fn`` set of x-transformers' ``AutoregressiveWrapper.generate(..., temperature, filter_logits_fn,
filter_kwargs)`` (reference code/seq2seq_pretrain.py:450,656).

All filters act on the RAW logits of a row, ``l[0..511]``; temperature is applied afterwards, as in
``AutoregressiveWrapper.generate``.  With ``p = softmax(l)`` over all entries and ``p_max`` its maximum, token ``i`` is kept iff

    top_k   (k, or frac_num_tokens with k = ceil(frac * 512))   l_i >= the k-th largest logit (ties at the threshold kept;
                                                                k <= 0 or k >= 512 keeps everything)
    top_p   (thres = 0.9)                                       G(i) = sum of p_j over {j : l_j > l_i} <= thres
    min_p   (min_p = 0.1)                                       p_i >= min_p * p_max
    top_a   (min_p_pow = 2.0, min_p_ratio = 0.02)               p_i >= p_max ** min_p_pow * min_p_ratio

``G(i)`` is the mass ranked strictly above ``i``, so the arg-max is always kept.  ``thres >= 1`` and ``min_p = 0`` mean "filter
off": every token is kept (a rule, so that a rounded sum of 1.0000001 cannot drop the tail).  A top_a limit above ``p_max``
(possible only with ``min_p_pow < 1`` and ``min_p_ratio > 1``) would keep nothing; the arg-max (and its ties) is kept then.

The token is ``argmax_i over the kept set of softmax(l_kept / temperature)_i / q_i`` with ``q`` the Exp(1) noise of the step,
indexed by the token id (never renumbered over the kept set); the lower index wins a tie.

Ties.  The top_p rule is x-transformers' ``top_p`` (sort descending, cumsum(softmax), ``cum > thres`` shifted right by one) on
every row without tied logits.  With ties torch's result depends on the order its sort leaves them in; this rule keeps or drops
equal logits together.  The top-k kernel has always taken the same liberty.

What this is not.  The x-transformers half of this project's oracle is restated from knowledge of v1.30.16 and cannot be checked
on a machine without the wheel (VERDICT.md "Missing 1").  The four filter bodies above join that list: nothing
here claims parity with the wheel.

``top_k``, ``top_p``, ``top_a`` and ``min_p`` below are callable on a torch tensor and return the ``-inf``-filled logits, so code
written against x-transformers keeps working on the host; each is also accepted, as the object or as its name string, wherever
this project takes ``filter_logits_fn``.
"""
import math

import numpy as np

VOCAB = 512
KINDS = {"top_k": 0, "top_p": 1, "min_p": 2, "top_a": 3}   # include/dimx.h DIMX_FILTER_*
DEFAULTS = {
    "top_k": {"frac_num_tokens": 0.1, "k": None},
    "top_p": {"thres": 0.9},
    "min_p": {"min_p": 0.1},
    "top_a": {"min_p_pow": 2.0, "min_p_ratio": 0.02},
}


def kind_name(kind):
    """'top_p' for the name, the Filter object, DIMX_FILTER_TOP_P or a function called top_p; None stays None."""
    if kind is None:
        return None
    if isinstance(kind, Filter):
        return kind.name
    if isinstance(kind, str):
        name = kind
    elif isinstance(kind, (int, np.integer)):
        name = {v: k for k, v in KINDS.items()}.get(int(kind))
    else:
        name = getattr(kind, "__name__", None)
    if name not in KINDS:
        raise ValueError("unknown sampler filter %r (one of %s)" % (kind, ", ".join(sorted(KINDS))))
    return name


def _params(name, kwargs):
    kw = dict(DEFAULTS[name])
    for k, v in (kwargs or {}).items():
        if k not in kw:
            raise TypeError("%s() got an unexpected filter argument %r" % (name, k))
        kw[k] = v
    return kw


def resolve(filter_logits_fn=None, filter_kwargs=None, top_k=52):
    """(kind, k, a, b) as the C-ABI takes them (dimx_set_sampler_filter).  No filter: kind 0 with the caller's ``top_k``."""
    name = kind_name(filter_logits_fn)
    if name is None:
        if filter_kwargs:
            name = "top_k"
        else:
            return 0, int(top_k), 0.0, 0.0
    kw = _params(name, filter_kwargs)
    if name == "top_k":
        if filter_kwargs and (filter_kwargs.get("k") is not None or "frac_num_tokens" in filter_kwargs):
            k = kw["k"] if kw["k"] is not None else math.ceil(float(kw["frac_num_tokens"]) * VOCAB)
        else:
            k = top_k
        return 0, int(k), 0.0, 0.0
    if name == "top_p":
        return 1, 0, float(kw["thres"]), 0.0
    if name == "min_p":
        return 2, 0, float(kw["min_p"]), 0.0
    return 3, 0, float(kw["min_p_pow"]), float(kw["min_p_ratio"])


def _rows(logits):
    l = np.asarray(logits, dtype=np.float64)
    if l.ndim == 1:
        l = l[None]
    if l.ndim != 2:
        raise ValueError("logits must be [R, V]")
    return l


def _softmax(l):
    e = np.exp(l - l.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def mass_above(logits):
    """G[r, i] = sum of softmax(l[r])_j over {j : l[r, j] > l[r, i]} (float64; equal logits share one value)."""
    l = _rows(logits)
    p = _softmax(l)
    order = np.argsort(-l, axis=-1, kind="stable")
    ls = np.take_along_axis(l, order, -1)
    ps = np.take_along_axis(p, order, -1)
    excl = np.cumsum(ps, axis=-1) - ps
    idx = np.broadcast_to(np.arange(l.shape[1]), l.shape)
    first = np.ones_like(l, dtype=bool)
    first[:, 1:] = ls[:, 1:] != ls[:, :-1]
    start = np.maximum.accumulate(np.where(first, idx, 0), axis=-1)   # first member of each run of equal logits
    gs = np.take_along_axis(excl, start, -1)
    g = np.empty_like(gs)
    np.put_along_axis(g, order, gs, -1)
    return g


def _limit(l, name, kw):
    """(p, lim): min_p / top_a keep p >= lim (lim [R, 1])."""
    p = _softmax(l)
    pmax = p.max(axis=-1, keepdims=True)
    if name == "min_p":
        return p, float(kw["min_p"]) * pmax
    return p, pmax ** float(kw["min_p_pow"]) * float(kw["min_p_ratio"])


def keep_mask(logits, kind, **kwargs):
    """bool [R, V]: the kept set of every row under filter ``kind`` (name, object or DIMX_FILTER_* number)."""
    name = kind_name(kind)
    kw = _params(name, kwargs)
    l = _rows(logits)
    V = l.shape[1]
    if name == "top_k":
        k = kw["k"] if kw["k"] is not None else math.ceil(float(kw["frac_num_tokens"]) * V)
        k = int(k)
        if k <= 0 or k >= V:
            return np.ones(l.shape, dtype=bool)
        kth = -np.partition(-l, k - 1, axis=-1)[:, k - 1:k]
        return l >= kth
    if name == "top_p":
        if float(kw["thres"]) >= 1.0:
            return np.ones(l.shape, dtype=bool)
        return mass_above(l) <= float(kw["thres"])
    if name == "min_p" and float(kw["min_p"]) == 0.0:
        return np.ones(l.shape, dtype=bool)
    p, lim = _limit(l, name, kw)
    return (p >= lim) | (l == l.max(axis=-1, keepdims=True))


def _scores(logits, noise, temperature, mask):
    l = np.where(mask, _rows(logits), -np.inf) / float(temperature)
    return _softmax(l) / np.asarray(noise, dtype=np.float64).reshape(l.shape)


def sample_ref(logits, noise, temperature, kind, **kwargs):
    """int64 [R]: one sampling step.  ``noise`` [R, V] Exp(1) (None, or temperature <= 0: the greedy arg-max)."""
    l = _rows(logits)
    if noise is None or temperature <= 0:
        return l.argmax(axis=-1).astype(np.int64)
    return _scores(l, noise, temperature, keep_mask(l, kind, **kwargs)).argmax(axis=-1).astype(np.int64)


def undecidable(logits, kind, margin, noise=None, temperature=1.0, **kwargs):
    """bool [R]: rows that a float32 evaluation may legitimately decide the other way.

    Kept set: top_p rows with |G(i) - thres| < margin for some i; min_p / top_a rows where some p_i lies within ``margin``
    (relative) of the limit.  Top-k compares integers images of the logits and has no such rows.  With ``noise`` the token
    is judged too: rows whose best and second-best score p_i / q_i differ by less than ``margin`` relative."""
    name = kind_name(kind)
    kw = _params(name, kwargs)
    l = _rows(logits)
    bad = np.zeros(l.shape[0], dtype=bool)
    if name == "top_p" and float(kw["thres"]) < 1.0:
        bad |= (np.abs(mass_above(l) - float(kw["thres"])) < margin).any(axis=-1)
    elif name in ("min_p", "top_a") and not (name == "min_p" and float(kw["min_p"]) == 0.0):
        p, lim = _limit(l, name, kw)
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.abs(p - lim) / lim
        bad |= (np.nan_to_num(rel, nan=np.inf) < margin).any(axis=-1)
    if noise is not None and temperature > 0:
        sc = _scores(l, noise, temperature, keep_mask(l, name, **kwargs))
        top2 = -np.partition(-sc, 1, axis=-1)[:, :2]
        bad |= (top2[:, 0] - top2[:, 1]) < margin * top2[:, 0]
    return bad


class Filter:
    """One of the four filters: callable on a torch tensor [..., V] like the x-transformers function of the same name
    (returns the logits with ``-inf`` outside the kept set), and accepted as ``filter_logits_fn`` by this project."""

    def __init__(self, name):
        self.name = self.__name__ = name
        self.kind = KINDS[name]

    def __call__(self, logits, **kwargs):
        import torch
        flat = logits.detach().reshape(-1, logits.shape[-1]).to("cpu", torch.float64).numpy()
        mask = torch.from_numpy(keep_mask(flat, self.name, **kwargs)).reshape(logits.shape).to(logits.device)
        return logits.masked_fill(~mask, float("-inf"))

    def __repr__(self):
        return "dimx.sampling.%s" % self.name


top_k = Filter("top_k")
top_p = Filter("top_p")
min_p = Filter("min_p")
top_a = Filter("top_a")


def add_filter_arguments(ap):
    """the sampler options of the example drivers: --filter {top_k,top_p,min_p,top_a} and its parameters"""
    ap.add_argument("--filter", choices=sorted(KINDS), default=None,
                    help="sampler filter of the generation (default: the reference's top_k with k = 52)")
    ap.add_argument("--filter-k", type=int, default=None, help="top_k: k (default ceil(0.1 * 512) = 52)")
    ap.add_argument("--filter-thres", type=float, default=None, help="top_p: thres (default 0.9)")
    ap.add_argument("--min-p", type=float, default=None, help="min_p: min_p (default 0.1)")
    ap.add_argument("--top-a-pow", type=float, default=None, help="top_a: min_p_pow (default 2.0)")
    ap.add_argument("--top-a-ratio", type=float, default=None, help="top_a: min_p_ratio (default 0.02)")


def filter_from_args(args):
    """{} or {'filter_logits_fn': name, 'filter_kwargs': {...}} for evaluate_test_epoch / forward, from add_filter_arguments"""
    given = {"top_k": {"k": args.filter_k}, "top_p": {"thres": args.filter_thres}, "min_p": {"min_p": args.min_p},
             "top_a": {"min_p_pow": args.top_a_pow, "min_p_ratio": args.top_a_ratio}}
    name = args.filter
    for other, kw in given.items():
        if other != name and any(v is not None for v in kw.values()):
            if name is None and other == "top_k":
                name = "top_k"      # --filter-k alone: the default filter with another k
            else:
                raise SystemExit("a parameter of %s was given, but --filter is %s" % (other, name))
    if name is None:
        return {}
    return {"filter_logits_fn": name, "filter_kwargs": {k: v for k, v in given[name].items() if v is not None}}
