"""CPU: the definition of classifier-free guidance (dimx/guidance.py) -- ``combine``, the null context on the oracle, the per-clip
keep vector of the training dropout, and the autograd checker ``dimx.train.slmft_loss(cond_keep=)`` -- and the generation's
checker tests/guidance_ref.py.  Synthetic SLMFT weights, B = 2, T = 24, lengths 24 / 17."""
import numpy as np
import pytest
import torch

import guidance_ref
import prompt_ref
from test_gpu_prompt import _case

B, T, LENS = 2, 24, (24, 17)


class Case:
    """inputs, the oracle's context and the plain loss, computed once and left unchanged"""

    def __init__(self, sd):
        from dimx import weights
        self.sd = sd
        self.dims = weights.S2SDims()
        self.v_s, self.v_a, self.z, self.mask = _case(B, T, list(LENS))
        self.ctx = prompt_ref.case_context(sd, self.v_s, self.v_a, self.mask)

    def loss(self, P=None, **kw):
        from dimx import train
        return train.slmft_loss(self.sd if P is None else P, self.dims, self.v_s, self.v_a, self.mask, self.z, **kw)

    def grads(self, keep):
        with torch.enable_grad():      # tests/test_gpu_prompt.py switches it off at import
            P = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in self.sd.items()}
            loss, _ = self.loss(P, cond_keep=keep)
            loss.backward()
        return {k: v.grad for k, v in P.items() if v.requires_grad}


@pytest.fixture(scope="module")
def case(full_sd):
    return Case(full_sd)


def test_combine_at_scale_one_is_cond_bit_for_bit():
    from dimx import guidance, prng
    c = prng.normal(5, "guidance.host.c", (7, 512)) * np.float32(3)
    u = prng.normal(5, "guidance.host.u", (7, 512)) * np.float32(3)
    c[0, 0], c[0, 1], u[0, 2] = -0.0, np.float32(1e30), np.float32(-1e30)
    g = guidance.combine(c, u, 1.0)
    assert g.dtype == np.float64 and np.array_equal(g.view(np.uint64), c.astype(np.float64).view(np.uint64))
    # the other form does not have the property, which is why it is not the definition
    other = u.astype(np.float64) + 1.0 * (c.astype(np.float64) - u.astype(np.float64))
    assert not np.array_equal(other, c.astype(np.float64))
    # scale is the float32 the kernel receives; 0 is the unconditional row up to the rounding of c - (c - u), 2 doubles the step
    assert np.array_equal(guidance.combine(c, u, 1.1), guidance.combine(c, u, float(np.float32(1.1))))
    assert not np.array_equal(guidance.combine(c, u, 1.1), c.astype(np.float64) + (1.1 - 1.0) * (c.astype(np.float64) - u))
    assert np.allclose(guidance.combine(c[1:], u[1:], 0.0), u[1:], rtol=0, atol=1e-12)
    assert np.array_equal(guidance.combine(c[1:], u[1:], 2.0), c[1:].astype(np.float64) + (c[1:].astype(np.float64) - u[1:]))


def test_null_context_is_the_decoder_without_cross_sublayers(case):
    """zero rows after the concat: every cross sublayer adds W_o . 0 = 0, whatever the mask; the same logits come from the decoder
    whose cross sublayers contribute nothing (their out-projections zeroed: h = h + 0)"""
    from oracle import ref_cpu
    inp = case.z[:, :-1].clamp(min=0)
    null = guidance_ref.null_context(case.ctx)
    with torch.no_grad():
        l_null = ref_cpu.xt_decoder_logits(case.sd, inp, null, case.mask)
        l_null_nomask = ref_cpu.xt_decoder_logits(case.sd, inp, null[:, :5], torch.ones(B, 5, dtype=torch.bool))
        sd0 = dict(case.sd)
        n_cross = 0
        for k in case.sd:
            if k.startswith("decoder_joint.net.attn_layers.layers.") and k.endswith(".1.to_out.weight") and int(k.split(".")[4]) % 3 == 1:
                sd0[k] = torch.zeros_like(case.sd[k])
                n_cross += 1
        assert n_cross == 4
        l_removed = ref_cpu.xt_decoder_logits(sd0, inp, case.ctx, case.mask)
        l_cond = ref_cpu.xt_decoder_logits(case.sd, inp, case.ctx, case.mask)
    err = (l_null - l_removed).abs().max().item()
    print("null context against the decoder without cross sublayers: max |logits| difference %.2e (against the conditional pass: %.2f)"
          % (err, (l_null - l_cond).abs().max().item()))
    assert err <= 1e-6
    assert (l_null - l_null_nomask).abs().max().item() <= 1e-6      # neither the mask nor the number of rows matters
    assert (l_null - l_cond).abs().max().item() > 0.1               # the context does matter to this decoder
    # no cross projection of the decoder carries a bias: the premise of the equivalence
    assert not [k for k in case.sd if k.startswith("decoder_joint.net.attn_layers.layers.") and ".1.to_" in k and k.endswith("bias")]


def test_cond_keep_is_reproducible_and_keeps_at_its_rate():
    from dimx import guidance
    a = guidance.cond_keep(7, 3, 16, 0.25)
    assert a.dtype == bool and a.shape == (16,)
    assert np.array_equal(a, guidance.cond_keep(7, 3, 16, 0.25))
    assert np.array_equal(a[:5], guidance.cond_keep(7, 3, 5, 0.25))           # clip b's draw does not depend on the batch size
    assert not np.array_equal(a, guidance.cond_keep(7, 4, 16, 0.25)) and not np.array_equal(a, guidance.cond_keep(8, 3, 16, 0.25))
    assert guidance.cond_keep(7, 3, 16, 0.0).all() and not guidance.cond_keep(7, 3, 16, 1.0).any()
    for p in (0.1, 0.25, 0.5):
        draws = np.concatenate([guidance.cond_keep(11, s, 64, p) for s in range(64)])      # 4096 draws
        sd = np.sqrt(p * (1 - p) / draws.size)
        print("cond_keep p=%.2f: keep rate %.4f over %d draws (1 - p = %.2f, 4 sd = %.4f)" % (p, draws.mean(), draws.size, 1 - p, 4 * sd))
        assert abs(draws.mean() - (1 - p)) <= 4 * sd


def test_slmft_loss_cond_keep_all_ones_is_the_plain_loss(case):
    with torch.no_grad():
        l0, g0 = case.loss()
        l1, g1 = case.loss(cond_keep=np.ones(B, dtype=bool))
        l2, g2 = case.loss(cond_keep=torch.ones(B))
    assert torch.equal(l0, l1) and torch.equal(g0, g1) and torch.equal(l0, l2) and torch.equal(g0, g2)


def test_slmft_loss_all_dropped_sends_no_gradient_into_the_context(case):
    g = case.grads(np.zeros(B, dtype=bool))
    ctx_side = [k for k in g if k.startswith(("encoder_s.", "encoder_joint.", "norm_s.", "patch_embed_s")) or k == "patch_embed_dec_s"]
    assert "patch_embed_dec_s" in ctx_side and len(ctx_side) > 20
    for k in ctx_side:
        assert g[k] is None or not g[k].any(), k
    assert g["decoder_joint.net.to_logits.weight"].abs().max().item() > 0
    # with one clip kept the context side does get a gradient
    g1 = case.grads(np.array([True, False]))
    assert g1["patch_embed_dec_s"].abs().max().item() > 0


def test_slmft_loss_dropped_clip_has_the_null_context_logits(case):
    from oracle import ref_cpu
    inp = case.z[:, :-1].clamp(min=0)
    with torch.no_grad():
        _, lg = case.loss(cond_keep=np.array([True, False]))
        _, plain = case.loss()
        null = ref_cpu.xt_decoder_logits(case.sd, inp, guidance_ref.null_context(case.ctx), case.mask)
    assert torch.equal(lg[0], plain[0])
    err = (lg[1] - null[1]).abs().max().item()
    print("dropped clip against the null-context decoder: max |logits| difference %.2e" % err)
    assert err <= 1e-6
    assert (lg[1] - plain[1]).abs().max().item() > 0.1


def test_checker_forced_along_its_own_tokens_repeats_itself(case):
    """guidance_ref.guided_generate: the free-running form and the form forced along the free run's tokens are one computation"""
    from dimx import guidance, prng
    n = 6
    noise = torch.from_numpy(prng.exponential(11, "guidance.host.noise", (n, B, 512)))
    free = guidance_ref.guided_generate(case.sd, case.z[:, :1], None, n, case.ctx, case.mask, 1.5, noise=noise)
    forced = guidance_ref.guided_generate(case.sd, case.z[:, :1], None, n, case.ctx, case.mask, 1.5, noise=noise, force=free["tokens"])
    assert torch.equal(free["tokens"], forced["tokens"])
    assert (free["cond"] - forced["cond"]).abs().max().item() <= 1e-5 and (free["uncond"] - forced["uncond"]).abs().max().item() <= 1e-5
    assert np.array_equal(forced["guided"], guidance.combine(forced["cond"].numpy(), forced["uncond"].numpy(), 1.5))
    # scale 1 is the plain generation's checker
    import online_ref
    plain_tok, plain_lg, _ = online_ref.online_generate(case.sd, case.z[:, :1], None, n, case.ctx, case.mask, None, noise)
    one = guidance_ref.guided_generate(case.sd, case.z[:, :1], None, n, case.ctx, case.mask, 1.0, noise=noise)
    assert torch.equal(one["tokens"], plain_tok) and (one["cond"] - plain_lg).abs().max().item() <= 1e-5
    # a forced prompt is kept
    pr = guidance_ref.guided_generate(case.sd, case.z[:, :4], (4, 2), n, case.ctx, case.mask, 3.0, noise=noise)
    assert torch.equal(pr["tokens"][0, :3], case.z[0, 1:4]) and torch.equal(pr["tokens"][1, :1], case.z[1, 1:2])


def test_pmi_is_the_per_token_difference():
    from dimx import guidance
    from dimx.scoring import sequence_scores
    from dimx import prng
    lg_c = prng.normal(3, "guidance.host.pmi.c", (3, 9, 512))
    lg_n = prng.normal(3, "guidance.host.pmi.n", (3, 9, 512))
    tok = prng.integers(3, "guidance.host.pmi.t", (3, 9), 0, 512)
    last = np.array([9, 5, 0])
    sc, sn = sequence_scores(lg_c, tok, None, last), sequence_scores(lg_n, tok, None, last)
    got = guidance.pmi(sc, sn)
    assert got.shape == (3,) and got[2] == 0.0
    assert np.allclose(got[:2], (np.asarray(sc.score)[:2] - np.asarray(sn.score)[:2]) / last[:2], rtol=0, atol=1e-15)
