"""GPU: the sampler filters top-p / min-p / top-a of sample_kernel (csrc/elementwise.hip) against the float64 definition
dimx.sampling -- the kernel alone (dimx_op_sample_filtered: kept set and token), and through dimx_generate /
dimx_generate_prompted (every step's token against that step's own returned logits)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

# Margins (conditions, not measurements).  A float32 evaluation of a cumulative mass cannot be held to a float64 rule at a
# knife edge, so a row is UNDECIDABLE, and left out of the exact comparison, when
#   top_p:          |G(i) - thres| < MARGIN for some i (G = probability mass ranked strictly above i),
#   min_p / top_a:  some p_i lies within MARGIN (relative) of the limit,
#   the token:      the best and the second-best score p_i / q_i (float64) differ by less than MARGIN relative.
# MARGIN = 1e-5 is about 7 times the 1.4e-6 maximum deviation between a float32 and a float64 cumulative softmax (numpy,
# 256 rows x 512, normal logits at scales 1, 3 and 6).  A case may leave out at most EXCLUDE_CAP of its rows and asserts it:
# a kernel that is wrong on many rows then fails instead of hiding behind the exclusion.  The float64 definition alone
# excludes 0 - 4.7 % of 256 rows with numpy's generator (worst: top_p 0.9 at scale 1), min_p <= 0.4 %; the dimx.prng streams
# below exclude at most 1.95 % (top_p 0.9, scale 1, R = 256) -- computed on the CPU before the seeds were fixed.
MARGIN = 1e-5
EXCLUDE_CAP = 0.10

ERR_ARG = -1
FILTERS = [("top_p", {"thres": 0.5}), ("top_p", {"thres": 0.9}), ("min_p", {"min_p": 0.1}), ("min_p", {"min_p": 0.02}),
           ("top_a", {"min_p_pow": 2.0, "min_p_ratio": 0.02})]


def _logits(R, scale, seed=3):
    from dimx import prng
    return prng.normal(seed, "sampler.filters.logits.%d.%d" % (R, scale), (R, 512)) * np.float32(scale)


def _noise(R, seed=4):
    from dimx import prng
    return prng.exponential(seed, "sampler.filters.noise.%d" % R, (R, 512))


def _report(what, excluded, rows, mismatches):
    print("%-64s excluded %4d / %4d rows (%.2f %%), mismatches on decidable rows: %d"
          % (what, excluded, rows, 100.0 * excluded / rows, mismatches))


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("scale", [1, 3, 6])
@pytest.mark.parametrize("R", [256, 1030])      # one wave per block / four waves per block with a ragged last block
def test_kept_set_and_token_against_the_definition(R, scale):
    from dimx import engine, sampling
    l = _logits(R, scale)
    q = _noise(R)
    lg, qg = torch.from_numpy(l).cuda(), torch.from_numpy(q).cuda()
    survivors = set()
    for kind, kw in FILTERS:
        want_keep = sampling.keep_mask(l, kind, **kw)
        edge = sampling.undecidable(l, kind, MARGIN, **kw)
        survivors.update(want_keep.sum(1).tolist())
        for temperature in (1.0, 0.7):
            bad = edge | sampling.undecidable(l, kind, MARGIN, noise=q, temperature=temperature, **kw)
            tok, keep = engine.op_sample(lg, temperature=temperature, noise=qg, filter_logits_fn=kind, filter_kwargs=kw,
                                         return_keep=True)
            tok, keep = tok.cpu().numpy().astype(np.int64), keep.cpu().numpy()
            want_tok = sampling.sample_ref(l, q, temperature, kind, **kw)
            ok = ~bad
            miss = int((keep[ok] != want_keep[ok]).any(axis=1).sum() + (tok[ok] != want_tok[ok]).sum())
            _report("op R=%d scale=%d %s %s T=%.1f" % (R, scale, kind, kw, temperature), int(bad.sum()), R, miss)
            assert bad.mean() <= EXCLUDE_CAP
            assert np.array_equal(keep[ok], want_keep[ok])
            assert np.array_equal(tok[ok], want_tok[ok])
            # what the kernel kept it also sampled from, decidable or not
            assert keep[np.arange(R), tok].all()
    # the shapes are chosen for the paths: > 128 survivors (the per-element loop) at scale 1, the compact path at scale 3,
    # single survivors at scale 6
    if scale == 1:
        assert max(survivors) > 128
    if scale == 3:
        assert min(survivors) <= 128
    if scale == 6:
        assert min(survivors) == 1


# ---------------------------------------------------------------------------------------------------------------- 2
def test_ties_keep_or_drop_together():
    from dimx import engine
    for value in (0.0, -3.25):
        flat = torch.full((2, 512), value).cuda()
        for kind, kw in FILTERS + [("top_p", {"thres": 0.0}), ("min_p", {"min_p": 1.0}), ("top_k", {"k": 52})]:
            _, keep = engine.op_sample(flat, noise=torch.from_numpy(_noise(2)).cuda(), filter_logits_fn=kind, filter_kwargs=kw,
                                       return_keep=True)
            assert keep.all(), (kind, kw)
    l = _logits(4, 3)
    l[:, 17] = l[:, 400] = l.max(axis=1) + 1.0
    tok, keep = engine.op_sample(torch.from_numpy(l).cuda(), noise=torch.from_numpy(_noise(4)).cuda(), filter_logits_fn="top_p",
                                 filter_kwargs={"thres": 0.0}, return_keep=True)
    keep = keep.cpu().numpy()
    assert keep[:, 17].all() and keep[:, 400].all() and keep.sum(1).tolist() == [2] * 4
    assert set(tok.cpu().tolist()) <= {17, 400}
    # -0.0 and +0.0 are one logit
    z = np.full((1, 512), -1.0, dtype=np.float32)
    z[0, 5], z[0, 300] = 0.0, -0.0
    _, keep = engine.op_sample(torch.from_numpy(z).cuda(), noise=torch.from_numpy(_noise(1)).cuda(), filter_logits_fn="top_p",
                               filter_kwargs={"thres": 0.0}, return_keep=True)
    assert keep.cpu().numpy()[0].nonzero()[0].tolist() == [5, 300]


@pytest.mark.parametrize("R,scale", [(256, 1), (1030, 3)])
def test_off_values_are_the_unfiltered_sampler_bit_for_bit(R, scale):
    from dimx import engine
    lg, qg = torch.from_numpy(_logits(R, scale)).cuda(), torch.from_numpy(_noise(R)).cuda()
    for temperature in (1.0, 0.7):
        base = engine.op_sample(lg, 0, temperature, qg)
        for kind, kw in (("top_p", {"thres": 1.0}), ("top_p", {"thres": 1.5}), ("min_p", {"min_p": 0.0})):
            tok, keep = engine.op_sample(lg, temperature=temperature, noise=qg, filter_logits_fn=kind, filter_kwargs=kw,
                                         return_keep=True)
            assert torch.equal(tok, base), (kind, kw)
            assert keep.all()


def test_top_p_zero_is_greedy_on_untied_rows():
    from dimx import engine
    l = _logits(256, 3)
    srt = np.sort(l, axis=1)
    untied = srt[:, -1] > srt[:, -2]
    assert untied.sum() >= 250
    tok, keep = engine.op_sample(torch.from_numpy(l).cuda(), noise=torch.from_numpy(_noise(256)).cuda(), filter_logits_fn="top_p",
                                 filter_kwargs={"thres": 0.0}, return_keep=True)
    assert np.array_equal(tok.cpu().numpy()[untied], l.argmax(1)[untied])
    assert (keep.cpu().numpy()[untied].sum(1) == 1).all()


def test_kind_zero_is_dimx_op_sample_bit_for_bit(golden_dir):
    from dimx import engine, sampling
    fx = np.load(os.path.join(golden_dir, "sampler_multinomial.npz"))
    lg, qg = torch.from_numpy(fx["logits"]).cuda(), torch.from_numpy(fx["noise"]).cuda()
    base = engine.op_sample(lg, 52, 1.0, qg)
    assert np.array_equal(base.cpu().numpy(), fx["ids"].astype(np.int32))
    tok, keep = engine.op_sample(lg, 52, 1.0, qg, return_keep=True)                       # dimx_op_sample_filtered, kind 0
    assert torch.equal(tok, base)
    assert np.array_equal(keep.cpu().numpy(), sampling.keep_mask(fx["logits"], "top_k", k=52))
    tok = engine.op_sample(lg, 1, 1.0, qg, filter_logits_fn=sampling.top_k, filter_kwargs={"k": 52})
    assert torch.equal(tok, base)
    for seed, step in ((77, 0), (77, 5)):
        assert torch.equal(engine.op_sample(lg, 52, 1.0, None, seed, step, filter_logits_fn="top_k"),
                           engine.op_sample(lg, 52, 1.0, None, seed, step))
    # a greedy launch still reports its kept set
    tok, keep = engine.op_sample(lg, 52, 0.0, None, filter_logits_fn="min_p", return_keep=True)
    assert np.array_equal(tok.cpu().numpy(), fx["logits"].argmax(1))
    ok = ~sampling.undecidable(fx["logits"], "min_p", MARGIN)
    assert ok.mean() >= 1 - EXCLUDE_CAP
    assert np.array_equal(keep.cpu().numpy()[ok], sampling.keep_mask(fx["logits"], "min_p")[ok])


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("kind,kw", FILTERS)
def test_device_generator_draws_inside_the_kept_set(kind, kw):
    from dimx import engine
    R = 1030
    lg = torch.from_numpy(_logits(R, 1 if kind == "top_p" else 3)).cuda()
    a, keep = engine.op_sample(lg, noise=None, seed=9001, step=3, filter_logits_fn=kind, filter_kwargs=kw, return_keep=True)
    b = engine.op_sample(lg, noise=None, seed=9001, step=3, filter_logits_fn=kind, filter_kwargs=kw)
    c = engine.op_sample(lg, noise=None, seed=9001, step=4, filter_logits_fn=kind, filter_kwargs=kw)
    assert keep.gather(1, a.long()[:, None]).all()
    assert torch.equal(a, b)
    assert not torch.equal(a, c)
    assert not torch.equal(a, lg.argmax(1).to(torch.int32)), "the draw is not the greedy token everywhere"


# ---------------------------------------------------------------------------------------------------------------- 4
B, T, LENS = 3, 12, (12, 9, 6)
PMAX, P0, PLEN = 5, 3, (5, 3, 4)


class _Gen:
    """inputs of the generation cases, built once and left unchanged"""

    def __init__(self):
        from dimx import prng
        self.v_s = torch.from_numpy(prng.normal(9, "s2s.vs", (B, T, 56))).cuda()
        self.v_a = torch.from_numpy(prng.normal(9, "s2s.va", (B, T, 768))).cuda()
        self.z = torch.from_numpy(prng.integers(9, "s2s.z", (B, T), 0, 512))
        mask = torch.zeros(B, T, dtype=torch.bool)
        for j, n in enumerate(LENS):
            mask[j, :n] = True
        self.m8 = mask.to(torch.uint8).cuda()
        self.noise = {S: torch.from_numpy(prng.exponential(11, "sampler.filters.gen.noise.%d" % S, (T - 1, B * S, 512)))
                      for S in (1, 2)}

    def run(self, eng, S=1, prompted=False, temperature=1.0, **kw):
        eng.encode_ctx(self.v_s, self.v_a, self.m8, True, n_samples=S, prompt_frames=P0 if prompted else 1)
        if prompted:
            kw.update(prompt=self.z[:, :PMAX].to(torch.int32).cuda().contiguous(),
                      prompt_len=torch.tensor(PLEN, dtype=torch.int32).cuda(), prefill=P0)
        tok, lg = eng.generate(None if prompted else self.z[:, 0].cuda(), self.m8, T, temperature, 52, self.noise[S].cuda(),
                               return_logits=True, n_samples=S, **kw)
        return tok.cpu().numpy().astype(np.int64), lg.cpu().numpy()


@pytest.fixture(scope="module")
def gen():
    return _Gen()


@pytest.fixture(scope="module")
def eng(full_sd):
    from dimx import engine, lib
    e = engine.Engine("cuda:0", lib.MODE_PARITY_F32)
    e.load_state_dict(full_sd)
    return e


def _check_steps(what, g, tok, lg, S, kind, kw, temperature=1.0, prompted=False):
    """every free step's token is sample_ref of that step's own logits and noise slice; forced columns hold the prompt"""
    from dimx import sampling
    R, n = tok.shape
    assert (R, n) == (B * S, T - 1) and lg.shape == (R, n, 512)
    free = np.ones((R, n), dtype=bool)
    if prompted:
        for r in range(R):
            plen = PLEN[r // S]
            free[r, :plen - 1] = False
            assert np.array_equal(tok[r, :plen - 1], g.z[r // S, 1:plen].numpy()), "forced columns hold the prompt's tokens"
        assert not lg[:, :P0 - 1].any(), "the prefill forms no logits"
    noise = g.noise[S].numpy()
    excluded = mismatches = rows = 0
    for t in range(n):
        sel = free[:, t]
        if not sel.any():
            continue
        l, q = lg[sel, t], noise[t][sel]
        bad = sampling.undecidable(l, kind, MARGIN, noise=q, temperature=temperature, **kw)
        want = sampling.sample_ref(l, q, temperature, kind, **kw)
        keep = sampling.keep_mask(l, kind, **kw)
        got = tok[sel, t]
        rows += int(sel.sum())
        excluded += int(bad.sum())
        mismatches += int((got[~bad] != want[~bad]).sum())
        edge = sampling.undecidable(l, kind, MARGIN, **kw)
        assert keep[np.arange(len(got)), got][~edge].all(), "a free token outside the kept set (step %d)" % t
    _report(what, excluded, rows, mismatches)
    assert excluded <= EXCLUDE_CAP * rows
    assert mismatches == 0
    return rows


GEN_FILTERS = [("top_p", {"thres": 0.9}), ("min_p", {"min_p": 0.1})]


@pytest.mark.parametrize("kind,kw", GEN_FILTERS)
@pytest.mark.parametrize("S,prompted", [(1, False), (2, False), (1, True), (2, True)])
def test_generation_samples_each_step_by_the_definition(eng, gen, S, prompted, kind, kw):
    tok, lg = gen.run(eng, S, prompted, filter_logits_fn=kind, filter_kwargs=kw)
    rows = _check_steps("generate S=%d prompted=%d %s %s" % (S, prompted, kind, kw), gen, tok, lg, S, kind, kw, prompted=prompted)
    assert rows == (B * S * (T - 1) if not prompted else S * sum(T - p for p in PLEN))


def test_generation_other_entries_and_temperature(eng, gen):
    from dimx import sampling
    tok, lg = gen.run(eng, 1, False, temperature=0.7, filter_logits_fn=sampling.top_a)
    _check_steps("generate top_a (object, defaults) T=0.7", gen, tok, lg, 1, "top_a", {}, temperature=0.7)
    tok, lg = gen.run(eng, 1, False, filter_logits_fn="top_k", filter_kwargs={"k": 5})
    _check_steps("generate top_k k=5 through filter_kwargs", gen, tok, lg, 1, "top_k", {"k": 5})


def test_generation_bf16_mode_is_self_consistent(full_sd, gen):
    """the comparison is against the call's own logits, so the mode's rounding does not enter"""
    from dimx import engine, lib
    e = engine.Engine("cuda:0", lib.MODE_PERF_BF16)
    e.load_state_dict(full_sd)
    tok, lg = gen.run(e, 1, False, filter_logits_fn="top_p", filter_kwargs={"thres": 0.9})
    _check_steps("generate bf16 top_p 0.9", gen, tok, lg, 1, "top_p", {"thres": 0.9})
    e.close()


# ---------------------------------------------------------------------------------------------------------------- 5
def test_a_replayed_step_graph_reads_the_new_threshold(eng, gen):
    from dimx import sampling
    tok9, lg9 = gen.run(eng, 1, False, filter_logits_fn="top_p", filter_kwargs={"thres": 0.9})
    tok3, lg3 = gen.run(eng, 1, False, filter_logits_fn="top_p", filter_kwargs={"thres": 0.3})     # same shapes: a graph replay
    _check_steps("replay: top_p 0.9", gen, tok9, lg9, 1, "top_p", {"thres": 0.9})
    _check_steps("replay: top_p 0.3", gen, tok3, lg3, 1, "top_p", {"thres": 0.3})
    # the two thresholds do ask for different tokens here: a stale 0.9 could not pass the 0.3 check
    assert np.array_equal(lg9[:, 0], lg3[:, 0])
    k9, k3 = (sampling.keep_mask(lg9[:, 0], "top_p", thres=t) for t in (0.9, 0.3))
    assert (k9.sum(1) >= k3.sum(1)).all() and (k9.sum(1) > k3.sum(1)).any()
    assert not np.array_equal(tok9, tok3)


def test_the_filter_holds_for_one_call_only(eng, gen, full_sd):
    from dimx import engine, lib
    gen.run(eng, 1, False, filter_logits_fn="min_p", filter_kwargs={"min_p": 0.1})
    tok, lg = gen.run(eng, 1, False)
    fresh = engine.Engine("cuda:0", lib.MODE_PARITY_F32)
    fresh.load_state_dict(full_sd)
    ftok, flg = gen.run(fresh, 1, False)
    fresh.close()
    assert np.array_equal(tok, ftok) and np.array_equal(lg, flg)
    _check_steps("unqualified generate after a filtered one (top-k 52)", gen, tok, lg, 1, "top_k", {"k": 52})


# ---------------------------------------------------------------------------------------------------------------- 6
def test_invalid_settings_leave_the_previous_filter_in_force(eng, gen):
    from dimx import lib
    nan = float("nan")
    invalid = [(4, 0.5, 0.0), (-1, 0.5, 0.0), (1, nan, 0.0), (1, -0.1, 0.0), (2, nan, 0.0), (2, -0.1, 0.0), (2, 1.5, 0.0),
               (3, nan, 0.02), (3, 2.0, nan), (3, -1.0, 0.02), (3, 2.0, -0.02)]
    eng.set_sampler_filter(1, 0.3)
    try:
        for kind, a, b in invalid:
            assert eng.lib.dimx_set_sampler_filter(eng.h, kind, a, b) == ERR_ARG, (kind, a, b)
        with pytest.raises(lib.DimxError):
            eng.set_sampler_filter(2, 1.5)
        tok, lg = gen.run(eng, 1, False)                      # no filter argument: the handle's setting, still top_p 0.3
    finally:
        eng.set_sampler_filter(0)
    _check_steps("generate after the refused settings (top_p 0.3)", gen, tok, lg, 1, "top_p", {"thres": 0.3})
    # the kernel-level entry refuses the same settings before it launches
    lg1 = torch.from_numpy(_logits(4, 3)).cuda()
    out = torch.full((4,), -7, dtype=torch.int32).cuda()
    for kind, a, b in invalid:
        rc = eng.lib.dimx_op_sample_filtered(lib.ptr(lg1), 4, kind, 52, a, b, 1.0, None, 5, 0, lib.ptr(out), None,
                                             lib.stream_ptr(lg1.device))
        assert rc == ERR_ARG, (kind, a, b)
    torch.cuda.synchronize()
    assert (out == -7).all()
