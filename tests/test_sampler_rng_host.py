"""CPU: the host definition of the sampler's on-device noise generator, dimx.prng.sampler_noise (the kernel side is
csrc/sample_pick.hpp; tests/test_gpu_sampler_rng.py holds every device route to this definition).  Checked here: the counters of
a generation never repeat, a shard window is a slice of the whole batch, u is uniform, q is Exp(1), the race
argmax p_i / q_i is a draw from p, and the rows of a step and the steps of a row are uncorrelated.

The thresholds are conditions: the 0.999 quantile of the statistic's distribution under the hypothesis, computed below.  The seeds
were fixed before the statistics were looked at and are not tuned; what they give is recorded in each docstring."""
import math

import numpy as np

SEED = 77                     # of every statistical case
Z999 = 3.0902323061678132     # standard normal quantiles: one-sided 0.999 ...
Z9995 = 3.2905267314919255    # ... and two-sided 0.999


def chi2_q999(dof):
    """0.999 quantile of chi-square(dof) by Wilson-Hilferty (dof = 63: 103.5, dof = 51: 88.0; the exact quantiles are 103.44 and 87.97)"""
    a = 2.0 / (9.0 * dof)
    return dof * (1.0 - a + Z999 * math.sqrt(a)) ** 3


def _chi2(counts, expected):
    return float(((counts - expected) ** 2 / expected).sum())


def _corr(a, b):
    a, b = a.ravel() - a.mean(), b.ravel() - b.mean()
    return float((a * b).sum() / math.sqrt((a * a).sum() * (b * b).sum()))


# ---------------------------------------------------------------------------------------------------------------- counters
def test_counters_of_a_best_of_10_generation_are_pairwise_distinct():
    """T = 299 steps x R = 2560 rows x 512 codes.  Row (t, r) owns the integer range [(t R + r) 512, (t R + r) 512 + 511]: the
    ranges are checked to be disjoint and in order from their end points (no counter is materialised beyond one step), the last
    one ends below 2^64, and splitmix64 is a bijection of the counter for a fixed seed (odd multipliers, xor-shifts), so distinct
    counters are distinct draws' inputs."""
    from dimx import prng
    T, R = 299, 2560
    one = prng.sampler_counters(3, R)
    assert one.dtype == np.uint64 and one.shape == (R, 512)
    assert int(one[0, 0]) == 3 * R * 512 and (np.diff(one.ravel().astype(np.int64)) == 1).all()      # one step: a run of R * 512 integers
    prev_last = -1
    for t in range(T):
        first = prng.sampler_counters(t, 1, R, 0)[0]
        last = prng.sampler_counters(t, 1, R, R - 1)[0]
        lo, hi = int(first[0]), int(last[511])
        assert lo == prev_last + 1, "step %d starts where step %d ended" % (t, t - 1)
        assert hi - lo + 1 == R * 512 and int(first[511]) - lo == 511 and hi - int(last[0]) == 511
        prev_last = hi
    assert prev_last == T * R * 512 - 1 < 2 ** 64
    # the rows in between: every row's range starts 512 after the previous row's (the first and the last step)
    for t in (0, T - 1):
        starts = prng.sampler_counters(t, R)[:, 0].astype(np.int64)
        assert starts[0] == t * R * 512 and (np.diff(starts) == 512).all()


def test_a_shard_window_is_a_slice_of_the_whole_batch():
    from dimx import prng
    R = 2560
    for seed, step in ((SEED, 0), (SEED, 7), (2 ** 63 + 12345, 2 ** 33 + 5), (9001, 2 ** 63)):
        whole = prng.sampler_noise(seed, step, R)
        for off, rows in ((0, 1), (100, 7), (R - 3, 3), (1280, 1280)):
            part = prng.sampler_noise(seed, step, rows, rows_total=R, row_offset=off)
            assert part.dtype == np.float64 and part.shape == (rows, 512)
            assert np.array_equal(part.view(np.uint64), whole[off:off + rows].view(np.uint64)), (seed, step, off, rows)
    # rows_total = None means rows; another total is another stream from step 1 on
    assert np.array_equal(prng.sampler_noise(5, 4, 10), prng.sampler_noise(5, 4, 10, rows_total=10))
    assert np.array_equal(prng.sampler_noise(5, 0, 10), prng.sampler_noise(5, 0, 10, rows_total=22))
    assert not np.array_equal(prng.sampler_noise(5, 1, 10), prng.sampler_noise(5, 1, 10, rows_total=22))
    # step 1 of a 10-row batch starts where its step 0 ended: rows 10 .. 19 of a 20-row step 0
    assert np.array_equal(prng.sampler_noise(5, 1, 10), prng.sampler_noise(5, 0, 20)[10:])


def test_the_transform_by_hand():
    """one element restated with python integers: the counter, the 64-bit wrap, the top 24 bits, the floor"""
    from dimx import prng
    M = (1 << 64) - 1
    for seed, step, total, off, row, code in ((1, 0, 4, 0, 0, 0), (2 ** 63 + 12345, 2 ** 33 + 5, 1000, 300, 17, 511),
                                              (9001, 2 ** 63, 22, 10, 5, 3)):
        ctr = ((step * total + off + row) * 512 + code) & M
        z = (seed + (ctr + 1) * 0x9E3779B97F4A7C15) & M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        r = z ^ (z >> 31)
        u = (r >> 40) / 2.0 ** 24
        got_u = prng.sampler_uniform(seed, step, row + 1, total, off)[row, code]
        got_q = prng.sampler_noise(seed, step, row + 1, total, off)[row, code]
        assert got_u == u and got_q == max(-float(np.log1p(np.float64(-u))), 2.0 ** -30)     # numpy's log1p, as the definition's
    u = prng.sampler_uniform(SEED, 0, 4096)
    assert u.min() >= 0.0 and u.max() < 1.0 and np.array_equal(u * 2 ** 24, np.floor(u * 2 ** 24))     # 24 bits, exact
    q = prng.sampler_noise(SEED, 0, 4096)
    assert q.min() >= 2.0 ** -30 and np.isfinite(q).all()
    assert np.array_equal(q[u == 0.0], np.full(int((u == 0.0).sum()), 2.0 ** -30))


# ---------------------------------------------------------------------------------------------------------------- statistics
def test_u_is_uniform_and_q_is_exponential():
    """64 equal bins over one [16384, 512] draw (seed 77, step 0): chi-square 59.35 at 63 degrees of freedom, bound 103.5.
    q: mean 1.000057, variance 1.000343 over N = 8388608 draws; an Exp(1) sample mean has standard deviation N^-1/2 = 3.45e-4
    and its sample variance (8 / N)^1/2 = 9.77e-4 (fourth central moment 9), the two-sided 0.999 bands are 3.2905 of those:
    1.14e-3 and 3.21e-3.  (The 24-bit grid of u moves either moment by less than 1e-7.)"""
    from dimx import prng
    R = 16384
    u = prng.sampler_uniform(SEED, 0, R)
    counts = np.bincount((u * 64).astype(np.int64).ravel(), minlength=64)
    assert counts.shape == (64,)
    stat = _chi2(counts, u.size / 64.0)
    q = prng.sampler_noise(SEED, 0, R)
    mean, var = float(q.mean()), float(q.var(ddof=1))
    print("uniformity chi-square %.2f (63 dof, bound %.1f); q mean %.6f variance %.6f over %d" % (stat, chi2_q999(63), mean, var, q.size))
    assert stat < chi2_q999(63)
    assert abs(mean - 1.0) < Z9995 / math.sqrt(q.size)
    assert abs(var - 1.0) < Z9995 * math.sqrt(8.0 / q.size)


def multinomial_case(R, seed=SEED, step=0):
    """one row of normal logits at scale 2 tiled R times, top-k 52, T = 1 -> (logits [R,512] f32, q, the top-k softmax [512])"""
    from dimx import prng, sampling
    row = prng.normal(5, "sampler.rng.multinomial.logits", (512,)) * np.float32(2)
    l = np.tile(row, (R, 1))
    keep = sampling.keep_mask(row, "top_k", k=52)[0]
    p = np.where(keep, np.exp(row.astype(np.float64) - float(row.max())), 0.0)
    return l, prng.sampler_noise(seed, step, R), p / p.sum()


def multinomial_statistic(tokens, p):
    """(chi-square of the token counts against R p over the kept cells, cells); a token outside the kept set is an error"""
    counts = np.bincount(np.asarray(tokens, dtype=np.int64), minlength=512).astype(np.float64)
    cells = p > 0
    assert counts[~cells].sum() == 0, "a token outside the kept set"
    return _chi2(counts[cells], len(tokens) * p[cells]), int(cells.sum())


def test_the_race_is_a_multinomial_draw():
    """16384 draws from one row (seed 77, step 0): chi-square of the counts against the top-k softmax 52.18 over 52 cells (51
    degrees of freedom, bound 88.0); the smallest expected count is 78.2."""
    from dimx import sampling
    R = 16384
    l, q, p = multinomial_case(R)
    tok = sampling.sample_ref(l, q, 1.0, "top_k", k=52)
    stat, cells = multinomial_statistic(tok, p)
    print("multinomial chi-square %.2f over %d cells (bound %.1f), smallest expected count %.1f"
          % (stat, cells, chi2_q999(cells - 1), R * p[p > 0].min()))
    assert cells == 52 and R * p[p > 0].min() > 5
    assert stat < chi2_q999(cells - 1)


def test_samples_of_a_clip_and_steps_of_a_row_are_uncorrelated():
    """the best-of-10 shape, R = 2560 rows = 256 clips x 10 samples (seed 77).  Pearson correlation of q between samples 0 and 1
    of every clip at step 0 (n = 256 x 512 pairs): -0.00266, band 3.2905 n^-1/2 = 0.00909; between steps 0 and 1 of every row
    (n = 2560 x 512): -0.00028, band 0.00287; between step 0 and the 2560 rows a stale per-shard total of 256 would reuse
    (whole-batch step 0 against itself shifted by 256 rows): 0.00012 at n = 2304 x 512, band 0.00303."""
    from dimx import prng
    S, R = 10, 2560
    q0, q1 = prng.sampler_noise(SEED, 0, R), prng.sampler_noise(SEED, 1, R)
    a, b = q0[0::S], q0[1::S]
    r_s, r_t, r_sh = _corr(a, b), _corr(q0, q1), _corr(q0[:-256], q0[256:])
    print("correlation: samples %.5f (band %.5f), steps %.5f (band %.5f), shifted rows %.5f (band %.5f)"
          % (r_s, Z9995 / math.sqrt(a.size), r_t, Z9995 / math.sqrt(q0.size), r_sh, Z9995 / math.sqrt(q0[256:].size)))
    assert abs(r_s) < Z9995 / math.sqrt(a.size)
    assert abs(r_t) < Z9995 / math.sqrt(q0.size)
    assert abs(r_sh) < Z9995 / math.sqrt(q0[256:].size)
    # and no two rows of a step, no two steps of a row, share their noise outright
    assert len({q0[r].tobytes() for r in range(R)}) == R
    assert not np.array_equal(q0, q1)
