"""dimx.sampling: the float64 host definition of the sampler filters (top-k, top-p, min-p, top-a).  No GPU."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dimx  # noqa: F401
from dimx import prng, sampling
from oracle import ref_cpu

NEG_INF = float("-inf")


# ---- the four x-transformers bodies, restated in torch float64 (sort / cumsum / pad / scatter) ----------------------
def xt_top_k(logits, frac_num_tokens=0.1, k=None):
    k = min(k if k is not None else math.ceil(frac_num_tokens * logits.shape[-1]), logits.shape[-1])
    val, ind = torch.topk(logits, k)
    return torch.full_like(logits, NEG_INF).scatter_(1, ind, val)


def xt_top_p(logits, thres=0.9):
    sorted_logits, sorted_indices = torch.sort(logits, descending=True)
    cum_probs = torch.cumsum(F.softmax(sorted_logits, dim=-1), dim=-1)
    remove = F.pad(cum_probs > thres, (1, -1), value=False)
    sorted_logits[remove] = NEG_INF
    return sorted_logits.scatter(1, sorted_indices, sorted_logits)


def xt_min_p(logits, min_p=0.1):
    probs = logits.softmax(dim=-1)
    limit = min_p * probs.amax(dim=-1, keepdim=True)
    return torch.where(probs < limit, NEG_INF, logits)


def xt_top_a(logits, min_p_pow=2.0, min_p_ratio=0.02):
    probs = logits.softmax(dim=-1)
    limit = torch.pow(probs.amax(dim=-1, keepdim=True), min_p_pow) * min_p_ratio
    return torch.where(probs < limit, NEG_INF, logits)


XT = {"top_k": xt_top_k, "top_p": xt_top_p, "min_p": xt_min_p, "top_a": xt_top_a}
CASES = [("top_k", {"k": 52}), ("top_k", {"frac_num_tokens": 0.1}), ("top_k", {"k": 1}), ("top_k", {"frac_num_tokens": 0.5}),
         ("top_p", {"thres": 0.9}), ("top_p", {"thres": 0.5}), ("top_p", {"thres": 0.05}), ("top_p", {}),
         ("min_p", {"min_p": 0.1}), ("min_p", {"min_p": 0.02}), ("min_p", {"min_p": 0.9}), ("min_p", {}),
         ("top_a", {}), ("top_a", {"min_p_pow": 2.0, "min_p_ratio": 0.02}), ("top_a", {"min_p_pow": 1.5, "min_p_ratio": 0.2})]


def _logits(scale, rows=64, seed=11):
    # the generator's 24-bit uniforms repeat now and then: the comparison with torch needs untied rows, so those are taken
    pool = prng.normal(seed, "sampling.host.logits.%d" % scale, (2 * rows, 512)).astype(np.float64) * scale
    l = pool[[len(np.unique(r)) == 512 for r in pool]][:rows]
    assert l.shape == (rows, 512)
    return np.ascontiguousarray(l)


@pytest.mark.parametrize("scale", [1, 3, 6])
@pytest.mark.parametrize("kind,kw", CASES)
def test_keep_mask_against_torch(kind, kw, scale):
    l = _logits(scale)
    want = torch.isfinite(XT[kind](torch.from_numpy(l.copy()), **kw)).numpy()
    got = sampling.keep_mask(l, kind, **kw)
    assert got.shape == (64, 512) and got.dtype == np.bool_
    # float64 against float64: a row may differ only where a probability sits within rounding of the limit
    edge = sampling.undecidable(l, kind, 1e-12, **kw)
    assert edge.sum() <= 1
    assert np.array_equal(got[~edge], want[~edge])
    assert got.any(axis=1).all()
    assert got[np.arange(64), l.argmax(1)].all(), "the arg-max is always kept"


def test_top_k_52_is_the_oracles_filter():
    for scale in (1, 3, 6):
        l = _logits(scale)
        want = torch.isfinite(ref_cpu.top_k_filter(torch.from_numpy(l), 52)).numpy()
        assert np.array_equal(sampling.keep_mask(l, "top_k", k=52), want)
        assert np.array_equal(sampling.keep_mask(l, "top_k"), want)          # frac_num_tokens 0.1 -> ceil(51.2) = 52
        assert sampling.keep_mask(l, "top_k", k=52).sum(1).tolist() == [52] * 64


@pytest.mark.parametrize("kind,kw", [("top_k", {"k": 52}), ("top_p", {"thres": 0.9}), ("top_p", {"thres": 0.0}),
                                     ("min_p", {"min_p": 0.1}), ("min_p", {"min_p": 1.0}), ("top_a", {})])
def test_all_equal_row_keeps_everything(kind, kw):
    for value in (0.0, -3.25, 7.0):
        assert sampling.keep_mask(np.full((2, 512), value), kind, **kw).all()


def test_two_equal_maxima_survive_top_p_zero():
    l = _logits(3, rows=4)
    l[:, 17] = l[:, 400] = l.max(axis=1) + 1.0
    keep = sampling.keep_mask(l, "top_p", thres=0.0)
    assert keep[:, 17].all() and keep[:, 400].all() and keep.sum(1).tolist() == [2] * 4
    # untied: thres = 0 is greedy
    l = _logits(3, rows=4)
    keep = sampling.keep_mask(l, "top_p", thres=0.0)
    assert keep.sum(1).tolist() == [1] * 4 and keep[np.arange(4), l.argmax(1)].all()


def test_off_values_keep_every_token():
    for scale in (1, 6, 40):     # scale 40: the tail's probabilities underflow, the rule still keeps them
        l = _logits(1) * scale
        assert sampling.keep_mask(l, "top_p", thres=1.0).all()
        assert sampling.keep_mask(l, "top_p", thres=1.5).all()
        assert sampling.keep_mask(l, "min_p", min_p=0.0).all()
        assert sampling.keep_mask(l, "top_k", k=0).all() and sampling.keep_mask(l, "top_k", k=512).all()
        assert not sampling.undecidable(l, "top_p", 1e-5, thres=1.0).any()
        assert not sampling.undecidable(l, "min_p", 1e-5, min_p=0.0).any()
    assert not sampling.keep_mask(_logits(6), "top_p", thres=0.999999).all()


def test_sample_ref_top_k_is_the_oracles_sampler(golden_dir):
    g = np.load(os.path.join(golden_dir, "sampler_multinomial.npz"))
    ids = sampling.sample_ref(g["logits"], g["noise"], 1.0, "top_k", k=52)
    assert ids.dtype == np.int64
    assert np.array_equal(ids, g["ids"].astype(np.int64))
    want = ref_cpu.sample_tokens(torch.from_numpy(g["logits"]), torch.from_numpy(g["noise"])).numpy()
    assert np.array_equal(ids, want)
    for temperature in (0.7, 1.3):
        want = ref_cpu.sample_tokens(torch.from_numpy(g["logits"]).double(), torch.from_numpy(g["noise"]).double(), temperature).numpy()
        assert np.array_equal(sampling.sample_ref(g["logits"], g["noise"], temperature, "top_k"), want)
    assert np.array_equal(sampling.sample_ref(g["logits"], None, 1.0, "top_p"), g["logits"].argmax(1))
    assert np.array_equal(sampling.sample_ref(g["logits"], g["noise"], 0.0, "min_p"), g["logits"].argmax(1))


@pytest.mark.parametrize("kind,kw", [("top_p", {"thres": 0.9}), ("min_p", {"min_p": 0.1}), ("top_a", {})])
def test_sample_ref_draws_inside_the_kept_set_with_unrenumbered_noise(kind, kw):
    l = _logits(3)
    q = prng.exponential(5, "sampling.host.noise", (64, 512)).astype(np.float64)
    keep = sampling.keep_mask(l, kind, **kw)
    tok = sampling.sample_ref(l, q, 0.7, kind, **kw)
    assert keep[np.arange(64), tok].all()
    p = torch.from_numpy(np.where(keep, l, NEG_INF) / 0.7).softmax(-1).numpy()
    assert np.array_equal(tok, (p / q).argmax(1))
    # a tie goes to the lower index
    l2 = np.zeros((1, 512)); q2 = np.ones((1, 512))
    assert sampling.sample_ref(l2, q2, 1.0, kind, **kw).tolist() == [0]


def test_undecidable_marks_knife_edges():
    l = _logits(1, rows=8)
    g = sampling.mass_above(l)
    thres = float(g[3, 100])                      # a row whose G(i) hits the threshold exactly
    u = sampling.undecidable(l, "top_p", 1e-5, thres=thres)
    assert u[3]
    assert not sampling.undecidable(l, "top_k", 1e-5, k=52).any()
    p = torch.from_numpy(l).softmax(-1).numpy()
    ratio = float(p[5, 200] / p[5].max())
    assert sampling.undecidable(l, "min_p", 1e-5, min_p=ratio)[5]
    # the token: two equal best scores
    q = np.ones((8, 512))
    l2 = l.copy(); l2[:, 7] = l2[:, 9] = l2.max(1) + 2.0
    assert sampling.undecidable(l2, "top_k", 1e-5, noise=q, temperature=1.0, k=52).all()
    assert not sampling.undecidable(l, "top_k", 1e-5, noise=q, temperature=1.0, k=52).all()


def test_names_objects_and_numbers_are_accepted():
    l = _logits(3, rows=4)
    for name, obj in (("top_k", sampling.top_k), ("top_p", sampling.top_p), ("min_p", sampling.min_p), ("top_a", sampling.top_a)):
        assert obj.name == name and obj.__name__ == name and sampling.kind_name(obj) == name
        want = sampling.keep_mask(l, name)
        assert np.array_equal(sampling.keep_mask(l, obj), want)
        assert np.array_equal(sampling.keep_mask(l, sampling.KINDS[name]), want)
        def wheel_fn(logits, **kw):      # any function of that name, e.g. the wheel's own, names the kind
            raise AssertionError("never called")
        wheel_fn.__name__ = name
        assert np.array_equal(sampling.keep_mask(l, wheel_fn), want)
    with pytest.raises(ValueError):
        sampling.keep_mask(l, "top_z")
    with pytest.raises(TypeError):
        sampling.keep_mask(l, "top_p", min_p=0.1)


@pytest.mark.parametrize("kind,kw", [("top_k", {}), ("top_k", {"k": 5}), ("top_p", {}), ("top_p", {"thres": 0.4}), ("min_p", {}),
                                     ("top_a", {}), ("top_a", {"min_p_pow": 1.0, "min_p_ratio": 0.3})])
def test_objects_fill_minus_inf_outside_their_mask(kind, kw):
    l = _logits(3, rows=6).astype(np.float32)
    t = torch.from_numpy(l)
    out = getattr(sampling, kind)(t, **kw)
    assert out.dtype == torch.float32 and out.shape == t.shape
    mask = sampling.keep_mask(l, kind, **kw)
    assert np.array_equal(torch.isfinite(out).numpy(), mask)
    assert np.array_equal(out.numpy()[mask], l[mask])
    assert torch.equal(t, torch.from_numpy(l)), "the input is left alone"
    # leading dimensions as AutoregressiveWrapper passes them
    out3 = getattr(sampling, kind)(t.view(2, 3, 512), **kw)
    assert torch.equal(out3.view(6, 512), out)


def test_resolve_maps_to_the_c_abi():
    assert sampling.resolve() == (0, 52, 0.0, 0.0)
    assert sampling.resolve(None, None, 30) == (0, 30, 0.0, 0.0)
    assert sampling.resolve("top_k") == (0, 52, 0.0, 0.0)
    assert sampling.resolve(sampling.top_k, {"k": 7}) == (0, 7, 0.0, 0.0)
    assert sampling.resolve(None, {"frac_num_tokens": 0.25}) == (0, 128, 0.0, 0.0)
    assert sampling.resolve("top_p") == (1, 0, 0.9, 0.0)
    assert sampling.resolve(sampling.top_p, {"thres": 0.5}) == (1, 0, 0.5, 0.0)
    assert sampling.resolve("min_p", {"min_p": 0.02}) == (2, 0, 0.02, 0.0)
    assert sampling.resolve(sampling.top_a) == (3, 0, 2.0, 0.02)
    assert sampling.KINDS == {"top_k": 0, "top_p": 1, "min_p": 2, "top_a": 3}


def test_the_c_header_declares_the_same_kinds():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "dimx.h")) as fh:
        text = fh.read()
    for name, kind in sampling.KINDS.items():
        assert "DIMX_FILTER_%s = %d" % (name.upper(), kind) in text
    from dimx import lib
    assert "dimx_set_sampler_filter" in lib.SIGNATURES and "dimx_op_sample_filtered" in lib.SIGNATURES
