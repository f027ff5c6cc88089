"""CPU: the definition of online generation (dimx/online.py) and its checker (tests/online_ref.py) -- what the GPU tests of
tests/test_gpu_online.py compare the library against -- on the SHORT case of tests/test_gpu_prompt.py."""
import numpy as np
import pytest
import torch

import online_ref
import prompt_ref
from test_gpu_prompt import LOGIT_TOL, SHORT, _case, _noise

torch.set_grad_enabled(False)
MIN_MARGIN = 2 * LOGIT_TOL    # a decision closer than this may fall the other way on the device
TOKEN_CASES = [(L, noisy) for L in (SHORT[1], 0, -3) for noisy in (False, True)]   # what test_gpu_online.py compares tokens on


class Short:
    """the SHORT inputs, the oracle's context and the checker's runs, computed once"""

    def __init__(self, sd):
        self.sd = sd
        self.B, self.T, self.lens = SHORT
        self.v_s, self.v_a, self.z, self.mask = _case(self.B, self.T, list(self.lens))
        self.noise = _noise(self.B, self.T)
        self.ctx = prompt_ref.case_context(sd, self.v_s, self.v_a, self.mask)
        self._runs = {}

    def run(self, lookahead, noisy, ctx=None):
        key = (lookahead, noisy, ctx is None)
        if ctx is not None or key not in self._runs:
            out = online_ref.online_generate(self.sd, self.z[:, :1], None, self.T - 1, self.ctx if ctx is None else ctx, self.mask,
                                             lookahead, self.noise if noisy else None)
            if ctx is not None:
                return out
            self._runs[key] = out
        return self._runs[key]


@pytest.fixture(scope="module")
def short(full_sd):
    return Short(full_sd)


def test_visible_values_and_clamps():
    from dimx.online import visible, visible_mask
    assert visible(0, 0, 40) == 2 and visible(5, 0, 40) == 7 and visible(5, 3, 40) == 10 and visible(5, -3, 40) == 4
    assert visible(38, 0, 40) == 40 and visible(39, 0, 40) == 40 and visible(0, 100, 40) == 40      # upper clamp
    assert visible(0, -2, 40) == 1 and visible(0, -100, 40) == 1 and visible(3, -5, 40) == 1        # lower clamp: row 0 stays
    assert visible(0, 2 ** 31 - 1, 40) == 40 and visible(10, -2 ** 31, 40) == 1
    assert np.array_equal(visible(np.arange(4), -1, 3), [1, 2, 3, 3])
    m = visible_mask(6, 0)
    assert m.shape == (1, 5, 6) and m.dtype == bool
    assert np.array_equal(m[0].sum(1), [2, 3, 4, 5, 6])
    assert np.array_equal(m[0, 1], [True, True, True, False, False, False])
    ml = visible_mask(6, 1, lens=[6, 2])
    assert ml.shape == (2, 5, 6)
    assert np.array_equal(ml[0].sum(1), [3, 4, 5, 6, 6]) and np.array_equal(ml[1].sum(1), [2, 2, 2, 2, 2])
    assert visible_mask(6, -100)[0, :, 0].all() and visible_mask(6, -100)[0].sum() == 5
    assert visible_mask(6, 4)[0].all()     # lookahead >= T - 2: everything


@pytest.mark.parametrize("noisy", [False, True])
def test_full_lookahead_is_the_offline_generation(short, noisy):
    from oracle import ref_cpu
    c = short
    ref_tok, ref_lg = ref_cpu.ar_generate(c.sd, c.z[:, 0], c.T - 1, c.ctx, c.mask, c.noise if noisy else None, return_logits=True)
    for L in (c.T - 2, c.T):
        tok, lg, _ = c.run(L, noisy) if L == c.T else online_ref.online_generate(c.sd, c.z[:, :1], None, c.T - 1, c.ctx, c.mask, L,
                                                                                c.noise if noisy else None)
        assert torch.equal(tok, ref_tok) and torch.equal(lg, ref_lg)
    off_tok, off_lg, _ = online_ref.online_generate(c.sd, c.z[:, :1], None, c.T - 1, c.ctx, c.mask, None, c.noise if noisy else None)
    assert torch.equal(off_tok, ref_tok) and torch.equal(off_lg, ref_lg)
    tok0, lg0, _ = c.run(0, noisy)
    differ = (tok0 != ref_tok).float().mean().item()
    print("lookahead 0 against offline, noisy=%d: %.0f %% of the tokens differ, logits by up to %.2f" % (noisy, 100 * differ, (lg0 - ref_lg).abs().max()))
    assert differ > 0.5


@pytest.mark.parametrize("L", [0, -3, 4])
def test_steps_do_not_see_a_perturbed_future(short, L):
    c = short
    P = 20
    v_s, v_a = c.v_s.clone(), c.v_a.clone()
    v_s[:, P:] += 1.0
    v_a[:, P:] -= 0.5
    ctx2 = prompt_ref.case_context(c.sd, v_s, v_a, c.mask)
    assert torch.equal(ctx2[:, :P], c.ctx[:, :P]), "the encoder side is not causal"
    assert not torch.equal(ctx2[0, P], c.ctx[0, P])
    _, lg, _ = c.run(L, False)
    _, lg2, _ = c.run(L, False, ctx=ctx2)
    last = P - 2 - L                 # vis(t) = t + 2 + L <= P  <=>  t <= P - 2 - L
    assert torch.equal(lg[:, :last + 1], lg2[:, :last + 1])
    # clips 0 and 1 are longer than P frames: their next step sees row P
    assert not torch.equal(lg[0, last + 1], lg2[0, last + 1]) and not torch.equal(lg[1, last + 1], lg2[1, last + 1])
    # the offline generation looks at the perturbed rows from its first step on
    _, off, _ = online_ref.online_generate(c.sd, c.z[:, :1], None, 1, c.ctx, c.mask, None)
    _, off2, _ = online_ref.online_generate(c.sd, c.z[:, :1], None, 1, ctx2, c.mask, None)
    print("offline first step moves by %.2f" % (off[:2] - off2[:2]).abs().max())
    assert not torch.equal(off[0], off2[0])


def test_forced_tokens_with_full_lookahead_are_the_teacher_forced_logits(short):
    from oracle import ref_cpu
    c = short
    inp = c.z[:, :-1].clamp(min=0)
    ref = ref_cpu.xt_decoder_logits(c.sd, inp, c.ctx, c.mask)
    tok, lg, _ = online_ref.online_generate(c.sd, c.z[:, :c.T - 1], None, c.T - 1, c.ctx, c.mask, c.T)
    assert torch.equal(tok[:, :c.T - 2], inp[:, 1:])
    err = (lg - ref).abs().max().item()
    print("forced steps against the teacher-forced pass: max |logits| difference %.2e" % err)
    assert err < LOGIT_TOL


@pytest.mark.parametrize("L,noisy", TOKEN_CASES)
def test_decisions_of_the_token_cases_are_not_near_ties(short, L, noisy):
    _, _, margins = short.run(L, noisy)
    keep, left_out = online_ref.compared_steps(margins, MIN_MARGIN)
    print("L=%d noisy=%d: smallest margin %.3e, pairs left out %.4f" % (L, noisy, margins.min().item(), left_out))
    assert margins.min().item() >= MIN_MARGIN
    assert left_out == 0.0 and bool(keep.all())
