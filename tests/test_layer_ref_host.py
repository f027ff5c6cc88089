"""CPU: the float64 reference of the decoder-layer kernel (tests/layer_ref.py) checked against torch, and the tolerances of
tests/test_gpu_layer_kernel.py checked against the reference's own wrong answers on that test's inputs."""
import pytest
import torch

import layer_ref as R

torch.set_grad_enabled(False)

T, TP, NKEYS = 72, 80, 72


@pytest.fixture(scope="module")
def inp():
    return R.make_inputs(129, T, TP, NKEYS, seed=129)


def test_deferred_form_is_layer_norm_then_linear():
    """rstd * (x . (gamma o W)^T - mean * colsum) == linear(layer_norm(x) * gamma, W) when nothing is rounded"""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(37, R.C, generator=g, dtype=torch.float64) * 1.5 + 0.7
    gamma = torch.rand(R.C, generator=g, dtype=torch.float64) * 0.4 + 0.8
    w = torch.randn(R.INNER, R.C, generator=g, dtype=torch.float64) / R.C ** 0.5
    ws = w * gamma
    mean, var = R.merge_stats(R.partial_stats(x))
    assert (mean - x.mean(1)).abs().max() < 1e-13 and (var - x.var(1, unbiased=False)).abs().max() < 1e-12
    got = R.deferred_q(x, mean, var, ws, ws.sum(1))
    want = torch.nn.functional.linear(torch.nn.functional.layer_norm(x, (R.C,), gamma, None, 1e-5), w)
    assert (got - want).abs().max().item() < 1e-12


def test_attention_matches_torch_and_an_all_masked_row_is_the_mean_of_v(inp):
    rows = torch.arange(6)
    qc = torch.randn(6, R.INNER, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    ck, cv, mask = inp["ck"][rows], inp["cv"][rows], inp["mask"][rows]
    got = R.cross_attn(qc, ck, cv, NKEYS, mask)
    bias = torch.zeros(6, 1, 1, NKEYS, dtype=torch.float64).masked_fill(mask[:, None, None, :] == 0, R.NEG)
    want = torch.nn.functional.scaled_dot_product_attention(qc.view(6, R.H, 1, R.D), ck[:, :, :NKEYS].double(), cv[:, :, :NKEYS].double(),
                                                            attn_mask=bias, scale=R.SCALE).reshape(6, -1)
    assert (got - want).abs().max().item() < 1e-12
    assert mask[3].sum() == 0
    assert (got[3] - cv[3, :, :NKEYS].double().mean(1).reshape(-1)).abs().max().item() < 1e-12


@pytest.mark.parametrize("step,nslab", [(0, 1), (1, 2), (33, 4), (71, 2)])
def test_every_wrong_answer_is_outside_its_stage_tolerance(inp, step, nslab):
    r = R.reference(inp, R.slabs(inp, nslab), step)
    alts = r["alts"]
    assert len(alts["x"]) == (6 if step > 0 else 4) and len(alts["qc"]) == 3 and len(alts["o"]) == 2 and len(alts["stats"]) == 2
    for name, alt in alts["x"]:
        assert ((alt - r["x2"]).abs() > R.X_TOL).any(), name
    for name, alt in alts["qc"]:
        assert ((alt - r["qc"]).abs() > R.QC_TOL).any(), name
    tol = R.attn_tolerance(r["o2_exact"])
    for name, alt in alts["o"]:
        assert ((alt - r["o2_exact"]).abs() > tol).any(), name
    for name, alt in alts["stats"]:
        assert R.stats_separated(r["mean2"], r["var2"], alt), name
    # the precision guard (mean^2 > 64 var) is far from every row: a factor 4 to spare
    for m, v in ((r["mean1"], r["var1"]), (r["mean2"], r["var2"])):
        assert (4 * m * m <= 64 * v).all()
    # y is the rounded residual stream and the statistics recombine to the row's moments
    assert torch.equal(r["y2"], r["x2"].to(torch.bfloat16).double())
    assert (r["mean2"] - r["x2"].mean(1)).abs().max() < 1e-13
    assert ((r["var2"] - r["x2"].var(1, unbiased=False)) / r["var2"]).abs().max() < 1e-12


def test_an_unobservable_rounding_tie_is_resolved_from_the_residual(inp):
    """admissible_bf16: move a few elements that sit at a rounding midpoint to their other neighbour; the residual tells which"""
    r = R.reference(inp, R.slabs(inp, 2), 33)
    exact = r["o1_exact"].clone()
    near = R.bf16r(exact)
    idx = [(0, 5), (0, 700), (17, 64), (128, 767)]
    moved = near.clone()
    for i, j in idx:
        up = (near[i, j].to(torch.bfloat16).view(torch.int16) + 1).view(torch.bfloat16).double()   # the neighbour away from zero
        exact[i, j] = (near[i, j] + up) / 2 - 1e-7 * torch.sign(near[i, j])                        # rounds to near, 1e-7 from the midpoint
        moved[i, j] = up
    assert torch.equal(R.bf16r(exact), near)
    resid = R.project(moved, inp["w_so"]) + 1e-6 * torch.randn(129, R.C, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    got, n = R.admissible_bf16(exact, resid, inp["w_so"])
    assert n == len(idx) and torch.equal(got, moved)
    got, n = R.admissible_bf16(exact, R.project(near, inp["w_so"]), inp["w_so"])
    assert n == 0 and torch.equal(got, near)
