"""CPU: the checker of online fine-tuning -- ``dimx.train.slmft_loss(lookahead=L)``, the PyTorch-autograd restatement the HIP
step with ``dimx_set_train_lookahead`` is compared against in tests/test_gpu_online_train.py.  Its cross-attention mask is
``dimx.online.visible_mask``; it leaks nothing from behind the window (logits and gradients, exactly); and it agrees with the
generation's checker (tests/online_ref.py) run with every token forced.  Synthetic SLMFT weights, B = 2, T = 24, lengths 24 / 17."""
import numpy as np
import pytest
import torch

import online_ref
import prompt_ref
from test_gpu_prompt import LOGIT_TOL, _case

B, T, LENS = 2, 24, (24, 17)
CUT = 12


class Case:
    """inputs and the checker's logits per look-ahead, computed once and left unchanged"""

    def __init__(self, sd):
        from dimx import weights
        self.P = {k: v for k, v in sd.items()}
        self.dims = weights.S2SDims()
        self.v_s, self.v_a, self.z, self.mask = _case(B, T, list(LENS))
        self._logits = {}

    def loss(self, *a, v_s=None, v_a=None, **kw):
        from dimx import train
        return train.slmft_loss(self.P, self.dims, self.v_s if v_s is None else v_s, self.v_a if v_a is None else v_a, self.mask,
                                self.z, *a, **kw)

    def logits(self, L):
        if L not in self._logits:
            with torch.no_grad():
                self._logits[L] = self.loss(lookahead=L)[1]
        return self._logits[L]


@pytest.fixture(scope="module")
def case(full_sd):
    return Case(full_sd)


def test_window_off_is_unchanged(case):
    with torch.no_grad():
        l0, g0 = case.loss()
        l1, g1 = case.loss(lookahead=None)
        l2, g2 = case.loss(None, None)                    # kv_mask, lookahead by position
        lt, gt = case.loss(lookahead=T)                   # an all-true window fills nothing
    assert torch.equal(l0, l1) and torch.equal(g0, g1) and torch.equal(l0, l2) and torch.equal(g0, g2)
    assert torch.equal(l0, lt) and torch.equal(g0, gt)
    assert torch.equal(g0, case.logits(T - 2))            # L >= T - 2 is the offline form
    assert not torch.equal(g0, case.logits(0))


@pytest.mark.parametrize("L", [0, -3, 5, -T - 5, T + 5])
def test_cross_mask_is_the_visible_mask(case, L):
    from dimx import train
    from dimx.online import visible_mask
    got = train.online_cross_mask(case.mask, L)
    assert got.dtype == torch.bool and tuple(got.shape) == (B, T - 1, T)
    assert np.array_equal(got.numpy(), visible_mask(T, L, LENS))
    assert bool(got[:, :, 0].all())                       # row 0 stays


@pytest.mark.parametrize("L", [0, -3])
def test_logits_do_not_see_a_perturbed_future(case, L):
    from dimx.online import visible
    v_s, v_a = case.v_s.clone(), case.v_a.clone()
    v_s[:, CUT:] += 1.0
    v_a[:, CUT:] -= 0.5
    with torch.no_grad():
        lg2 = case.loss(v_s=v_s, v_a=v_a, lookahead=L)[1]
    lg = case.logits(L)
    rows = torch.from_numpy(visible(np.arange(T - 1), L, T) <= CUT)
    assert int(rows.sum()) == CUT - 1 - L                 # vis(t) = t + 2 + L <= CUT  <=>  t <= CUT - 2 - L
    assert torch.equal(lg[:, rows], lg2[:, rows])
    assert not torch.equal(lg[0, T - 2], lg2[0, T - 2]) and not torch.equal(lg[1, T - 2], lg2[1, T - 2])
    first = int(rows.sum())                               # the first row whose window holds frame CUT
    assert not torch.equal(lg[0, first], lg2[0, first])
    with torch.no_grad():                                 # the offline step looks at the perturbed rows from row 0 on
        off2 = case.loss(v_s=v_s, v_a=v_a)[1]
    assert not torch.equal(case.logits(T)[0, 0], off2[0, 0])


@pytest.mark.parametrize("L", [0, -3])
def test_no_gradient_reaches_context_rows_behind_the_window(case, L):
    """v_audio row j feeds context row j and nothing else, so d logits[b, t] / d v_audio[b, j] is the gradient with respect to the
    audio half of context row j: exactly zero for j >= visible(t, L, T) (masked_fill passes no gradient), not zero below it."""
    from dimx.online import visible
    v_a = case.v_a.clone().requires_grad_(True)
    with torch.enable_grad():
        logits = case.loss(v_a=v_a, lookahead=L)[1]
        for b in range(B):
            for t in range(T - 1):
                g, = torch.autograd.grad(logits[b, t].sum(), v_a, retain_graph=True)
                vis = visible(t, L, T)
                assert torch.count_nonzero(g[b, vis:]) == 0, (b, t)
                assert torch.count_nonzero(g[1 - b]) == 0, (b, t)
                seen = min(vis, LENS[b])
                assert bool((g[b, :seen].abs().amax(-1) > 0).all()), (b, t)
                assert torch.count_nonzero(g[b, LENS[b]:]) == 0, (b, t)


@pytest.mark.parametrize("L", [0, -3])
def test_agrees_with_the_forced_steps_of_the_generation_checker(case, full_sd, L):
    """a generation whose every token is forced to z, step t under the context mask narrowed to visible(t, L, T) (online_ref), is
    the masked teacher-forced pass: the bound is the one tests/test_online_host.py holds that checker's forced steps to."""
    ctx = prompt_ref.case_context(full_sd, case.v_s, case.v_a, case.mask)
    tok, lg, _ = online_ref.online_generate(full_sd, case.z[:, :T - 1], None, T - 1, ctx, case.mask, L)
    assert torch.equal(tok[:, :T - 2], case.z[:, 1:T - 1].clamp(min=0))
    err = (lg - case.logits(L)).abs().max().item()
    off = (lg - case.logits(T)).abs().max().item()
    print("L=%d: forced online steps against slmft_loss(lookahead=L): max |logits| difference %.2e (against the offline pass: %.2f)"
          % (L, err, off))
    assert err < LOGIT_TOL
    assert off > 100 * LOGIT_TOL                          # the window is not a no-op on these inputs
