"""CPU: the host side of the windowed prefill -- the new exports exist in the built library and in dimx.lib, the
schedule of a session begun from a prompt (dimx.stream.steps_due with done0) against a brute-force restatement, and the begin
condition (dimx.stream.prompt_fits) against what the prefilled rows read under dimx.online.visible."""
import numpy as np
import pytest

import dimx  # noqa: F401
from dimx import lib, online, stream
from test_gpu_prompt import LOGIT_TOL, SHORT, SHORT_CFG, _case, _noise

# what tests/test_gpu_win_prefill.py runs the windowed prompt prefill on: (Pmax, P0, prompt lengths) x look-ahead x greedy / noisy
PROMPT_CFG = SHORT_CFG + [(18, 18, None), (34, 33, (34, 33, 33))]
PROMPT_LOOKAHEADS = [0, -3, 2]
# ... and the sessions from a prompt: 3 clips x 40 frames, (F, P) per look-ahead
SESSION_LOOKAHEADS = [0, -3, 2, 6]
# seed of these inputs (tests/test_gpu_prompt.py _case): with the suite's usual 9 the checker itself has near-ties in a quarter of the
# (clip, step) pairs of some cases; with 10 it has none (the two tests at the end of this file)
WIN_SEED = 10


def session_cases(L):
    return [(17, 17 - max(L, 0)), (33, 20), (2 + max(L, 0), 2)]


MIN_MARGIN = 2 * LOGIT_TOL      # tests/test_gpu_online.py
MAX_LEFT_OUT = 0.02
NEW_EXPORTS = ["dimx_op_cross_attn_win", "dimx_decode_tf_win", "dimx_stream_workspace_bytes_prompt", "dimx_stream_begin_prompted"]


def test_new_exports_are_in_the_library_and_in_lib_py():
    l = lib.load()
    for name in NEW_EXPORTS:
        assert name in lib.SIGNATURES, name
        assert hasattr(l, name), name


def _due_brute(n, L, done0):
    """step t runs once the frames 0 .. t + 1 + max(L, 0) exist, and never fewer than done0 steps count as done"""
    ran = [t for t in range(64) if t + 1 + max(L, 0) <= n - 1]
    assert ran == list(range(len(ran)))      # the steps that may run are a prefix
    return max(done0, len(ran))


@pytest.mark.parametrize("L", [-3, 0, 2, 6])
def test_steps_due_with_a_prompt(L):
    for n in range(25):
        for done0 in (0, 1, 5):
            assert stream.steps_due(n, L, done0=done0) == _due_brute(n, L, done0), (n, L, done0)
        # done0 = 0 is the function as it was: the formula of its docstring
        assert stream.steps_due(n, L, done0=0) == stream.steps_due(n, L) == int(np.clip(n - 1 - max(L, 0), 0, max(n - 1, 0)))
        assert stream.steps_due(n, L, ended=True, done0=0) == stream.steps_due(n, L, ended=True) == max(n - 1, 0)


def test_schedule_of_a_prompted_session():
    L, F, P = 2, 17, 15
    sched = stream.schedule([1, 4, 16, 2], L, F=F, P=P)
    assert sched[0] == (18, 14, 15) and sched[-1] == (40, 37, 39)
    assert all(a[2] == b[1] for a, b in zip(sched, sched[1:]))
    assert stream.schedule([7, 3], 0) == stream.schedule([7, 3], 0, F=0, P=1)


@pytest.mark.parametrize("L", [-3, 0, 2, 6])
def test_begin_condition_is_what_the_prefilled_rows_read(L):
    Tmax = 24
    for F in range(0, Tmax + 3):
        for P in range(-1, Tmax + 3):
            ok = stream.prompt_fits(P, L, F, Tmax)
            if P < 1 or F > Tmax:
                assert not ok, (P, L, F)
                continue
            # rows 0 .. P - 2 are prefilled with the key bound Tmax (the session's while it is open): every key they read ...
            reads = int(online.visible(np.arange(P - 1), L, Tmax).max()) if P > 1 else 0
            # ... and the frame of the prompt's last code with its look-ahead buffer (what the schedule waits for before it runs
            # the step that produced that code) must be among the frames given
            frames = set(range(F))
            waits_for = set(range(P + max(L, 0)))
            assert ok == (waits_for <= frames), (P, L, F)
            if ok:
                assert set(range(reads)) <= frames, (P, L, F, reads)
                assert stream.steps_due(F, L, done0=P - 1) == _due_brute(F, L, 0) >= P - 1
            elif L >= 0 and P >= 2 and P + L <= Tmax:
                assert reads > F, (P, L, F, reads)      # for a look-ahead the condition is exactly "the keys exist"


@pytest.fixture(scope="module")
def short_ctx(full_sd):
    import prompt_ref
    B, T, lens = SHORT
    v_s, v_a, z, mask = _case(B, T, list(lens), seed=WIN_SEED)
    return z, mask, prompt_ref.case_context(full_sd, v_s, v_a, mask), _noise(B, T)


@pytest.mark.parametrize("L", PROMPT_LOOKAHEADS)
@pytest.mark.parametrize("Pmax,P0,plen", PROMPT_CFG)
def test_prompt_cases_stay_inside_the_cap_on_the_checker_alone(full_sd, short_ctx, Pmax, P0, plen, L):
    """the (clip, step) pairs from column P0 - 1 on that a near-tie of the checker takes out of the token comparison: at most
    MAX_LEFT_OUT of them, greedy and noisy"""
    import online_ref
    import torch
    torch.set_grad_enabled(False)
    z, mask, ctx, noise = short_ctx
    for nz in (None, noise):
        _, _, margins = online_ref.online_generate(full_sd, z[:, :Pmax], plen, SHORT[1] - 1, ctx, mask, L, nz)
        _, left_out = online_ref.compared_steps(margins[:, P0 - 1:], MIN_MARGIN)
        print("Pmax=%d P0=%d plen=%s L=%d noisy=%d: smallest margin %.3e, pairs left out %.4f"
              % (Pmax, P0, plen, L, nz is not None, margins[:, P0 - 1:].min().item(), left_out))
        assert left_out <= MAX_LEFT_OUT


@pytest.mark.parametrize("L", SESSION_LOOKAHEADS)
def test_session_cases_stay_inside_the_cap_on_the_checker_alone(full_sd, L):
    import online_ref
    import prompt_ref
    import torch
    torch.set_grad_enabled(False)
    v_s, v_a, z, mask = _case(3, 40, [40] * 3, seed=WIN_SEED)
    ctx = prompt_ref.case_context(full_sd, v_s, v_a, mask)
    for P in sorted({p for _, p in session_cases(L)} | {1}):
        _, _, margins = online_ref.online_generate(full_sd, z[:, :P], None, 39, ctx, mask, L)
        _, left_out = online_ref.compared_steps(margins[:, P - 1:], MIN_MARGIN)
        print("session L=%d P=%d: smallest margin %.3e, pairs left out %.4f" % (L, P, margins[:, P - 1:].min().item(), left_out))
        assert left_out <= MAX_LEFT_OUT
