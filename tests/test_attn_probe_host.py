"""CPU: the float64 reference of the prefill attention (tests/attn_probe.py) checked against torch, and the two probes of
tests/test_gpu_attention_probes.py checked against the reference's own wrong answers at that test's shapes: the rounded reference
passes, every visibility defect fails."""
import pytest
import torch

import attn_probe as P

torch.set_grad_enabled(False)

DS = (48, 64, 96)


def _probe_runs(case, D, dtype=torch.bfloat16):
    """(name, inputs, failures(out)) of the three probe runs of a case"""
    _, Lq, Lk, causal, _, _, _ = case
    B, lens, kmask, kp = P.case_masks(case)
    H, scale = P.HEADS[D]
    runs = []
    q, k, v = P.count_inputs(B, Lq, Lk, H, D, P.SEED)
    runs.append(("count", (q, k, v), lambda out, v=v: P.count_failures(out, kp, v, lens, dtype)))
    for choice in ("last", "hidden"):
        q, k, v, _, hidden = P.locator_inputs(kp, H, D, scale, P.SEED + Lk, choice)
        ref = P.reference(q, k, v, scale, kp, dtype, lens)
        runs.append((choice, (q, k, v), lambda out, ref=ref, hidden=hidden: P.locator_failures(out, ref, kp, lens, Lk, hidden)))
    return runs, kp, lens, scale


def test_keep_is_the_definition():
    lens, kmask = [5, 0, 7], torch.tensor([[1, 0, 1, 1, 1, 1, 1], [1] * 7, [0, 1, 1, 0, 1, 1, 1]], dtype=torch.uint8)
    for causal in (False, True):
        kp = P.keep(4, 7, causal, lens, kmask)
        for b in range(3):
            for i in range(4):
                for j in range(7):
                    assert kp[b, i, j] == (j < min(lens[b], 7) and kmask[b, j] != 0 and (not causal or j <= i))
    assert P.keep(3, 5, True, None, None).shape == (1, 3, 5) and P.keep(2, 2, False, None, None).all()


def test_reference_matches_torch_and_a_row_without_keys_is_the_mean_of_v():
    g = torch.Generator().manual_seed(1)
    B, Lq, Lk, H, D = 3, 9, 21, 2, 48
    q, k, v = (torch.randn(B, n, H, D, generator=g) for n in (Lq, Lk, Lk))
    kmask = P.random_mask(B, Lk, 2)
    kmask[1] = 0
    lens = [21, 21, 0]
    kp = P.keep(Lq, Lk, False, lens, kmask)
    got = P.reference(q, k, v, 0.2, kp, torch.float32, lens)
    bias = torch.zeros(B, 1, Lq, Lk, dtype=torch.float64).masked_fill(~kp[:, None], -torch.finfo(torch.float32).max)
    want = torch.nn.functional.scaled_dot_product_attention(q.double().transpose(1, 2), k.double().transpose(1, 2), v.double().transpose(1, 2),
                                                            attn_mask=bias, scale=0.2).transpose(1, 2)
    assert (got[0] - want[0]).abs().max().item() < 1e-12
    assert (got[1] - want[1]).abs().max().item() < 1e-12                       # torch: equal -max scores, a uniform softmax
    assert (got[1] - P.full_row_value(v)[1][None]).abs().max().item() < 1e-12
    assert (got[2] == 0).all()


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("case", P.CASES, ids=P.CASE_IDS)
def test_the_rounded_reference_passes_and_every_mutant_fails(case, D):
    _, Lq, Lk, causal, _, _, _ = case
    for dtype in (torch.bfloat16, torch.float32):
        runs, kp, lens, scale = _probe_runs(case, D, dtype)
        valid, empty = P.row_classes(kp, lens)
        rows = valid & ~empty[:, None]
        for name, (q, k, v), failures in runs:
            own = P.reference(q, k, v, scale, kp, dtype, lens).to(dtype)
            assert failures(own) == [], (name, dtype)
        if dtype != torch.bfloat16:
            continue
        B, lens_l, kmask, _ = P.case_masks(case)
        n_mut = 0
        for mname, mk, mlens in P.mutants(Lq, Lk, causal, lens_l, kmask, B):
            emptied = torch.zeros_like(empty) if mlens is None else (torch.as_tensor(mlens) == 0) & ~empty
            # with a single key, a row the defect leaves without one is the mean over that key: the same answer, for any kernel
            seen = mk | ~mk.any(-1, keepdim=True) if Lk == 1 else mk
            if not ((seen != kp)[rows].any() or (rows & emptied[:, None]).any()):
                continue                                   # the defect shows on no row that has a visible key
            n_mut += 1
            caught = [name for name, (q, k, v), failures in runs if failures(P.reference(q, k, v, scale, mk, dtype, mlens).to(dtype))]
            assert caught, "%s passes every probe" % mname
        assert n_mut >= 1


@pytest.mark.parametrize("D", DS)
def test_locator_codes_leak_less_than_2_to_the_minus_12_and_hidden_targets_have_a_unique_runner_up(D):
    H, scale = P.HEADS[D]
    n_rows = n_hidden = 0
    for case in P.CASES:
        _, Lq, Lk, causal, _, _, _ = case
        B, lens, kmask, kp = P.case_masks(case)
        base, _ = P.codes(Lk, H, D, P.SEED + Lk)
        gap = P.code_gap(base)
        assert P.leak_bound(Lk, gap, scale) < P.LEAK_MAX, (case[0], gap)
        q, k, v, target, hidden = P.locator_inputs(kp, H, D, scale, P.SEED + Lk, "hidden")
        assert not torch.gather(kp, 2, target[:, :, None])[..., 0][hidden].any()         # a hidden target is invisible
        _, p = P.reference(q, k, v, scale, kp, torch.bfloat16, lens, return_probs=True)
        top2 = p.topk(min(2, Lk), dim=-1).values                                          # [B, H, Lq, <= 2]
        hid = hidden[:, None, :].expand(-1, H, -1)
        assert (top2[..., 0][hid] >= P.HIDDEN_MIN_TOP - 1e-6).all()
        if Lk > 1:
            assert (top2[..., 0] > top2[..., 1])[hid].all()
        valid, empty = P.row_classes(kp, lens)
        has_invisible = valid & ~kp.all(-1) & ~empty[:, None]
        n_rows += int(has_invisible.sum())
        n_hidden += int(hidden.sum())
    print("D = %d: %d of %d rows with an invisible key probe a hidden target" % (D, n_hidden, n_rows))
    assert n_hidden >= 0.9 * n_rows


@pytest.mark.parametrize("D", DS)
def test_one_wrong_key_fails_by_a_wide_margin(D):
    """A one-key defect (causal bound or len off by one) against the acceptance tolerance 2^-7.  Count probe: the key's class column
    moves by (n - c) / (c (n +- 1)) relative -- at least 2^-3 = 16 tolerances on EVERY affected row at these shapes (n <= 257,
    c <= ceil(257 / 48) = 6), or the column was / becomes empty and fails the exact-zero rule.  (A flat 0.3 holds only while the
    key's class has at most three visible keys: 0.24 at 129 visible keys of 193 and 0.16 at 257 for D = 48.)  Somewhere in every head
    width's cases it is 50 tolerances and more.  Locator probe: the row spells another key, so a bit moves by 1 - 2 * 2^-12 or more."""
    H, scale = P.HEADS[D]
    least, most = float("inf"), 0.0
    for case in P.CASES:
        _, Lq, Lk, causal, _, _, _ = case
        B, lens, kmask, kp = P.case_masks(case)
        valid, empty = P.row_classes(kp, lens)
        q, k, v = P.count_inputs(B, Lq, Lk, H, D, P.SEED)
        want = P.reference(q, k, v, scale, kp, torch.bfloat16, lens)
        ql, kl, vl, target, _ = P.locator_inputs(kp, H, D, scale, P.SEED + Lk, "last")
        want_l = P.reference(ql, kl, vl, scale, kp, torch.bfloat16, lens)
        for mname, mk, mlens in P.mutants(Lq, Lk, causal, lens, kmask, B):
            if mname not in ("causal bound + 1", "causal bound - 1", "len + 1", "len - 1"):
                continue
            hit = (mk != kp).any(-1) & valid & mk.any(-1) & ~empty[:, None]
            if not hit.any():
                continue
            assert ((mk != kp).sum(-1)[hit] == 1).all()
            got = P.reference(q, k, v, scale, mk, torch.bfloat16, mlens)
            rel = ((got - want).abs() / want.clamp(min=1e-300))[hit]                      # inf where an empty column filled
            worst = rel.flatten(1).amax(1)
            assert worst.min().item() >= 16 * P.BF16_RTOL, (case[0], mname, worst.min().item())
            least, most = min(least, worst.min().item()), max(most, worst.max().item())
            # the locator sees the defects that hide the target or show a key past it
            got_l = P.reference(ql, kl, vl, scale, mk, torch.bfloat16, mlens)
            moved = (mk != kp) & (torch.arange(Lk)[None, None, :] >= target[:, :, None])
            hit_l = hit & moved.any(-1)
            if mname in ("causal bound - 1", "len - 1") and hit_l.any():
                d = (got_l - want_l).abs()[hit_l].flatten(1).amax(1)
                assert d.min().item() >= 50 * P.BIT_TOL, (case[0], mname, d.min().item())
    print("D = %d: one wrong key moves a count by %.3g .. %.3g relative" % (D, least, most))
    assert most >= 50 * P.BF16_RTOL
