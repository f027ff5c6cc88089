"""GPU: where dimx_op_lstm_layer (csrc/lstm.hip) puts a clip.  The group kernel deals the up to 128 clips of a launch in equal
runs over min(8, nb) groups (per = ceil(nb / ngrp), at most 16 clips a group), lstm_layer_run cuts a batch into launches of
128 clips, and the no-communication kernel takes 4 clips a block.  Every case here runs both paths on independent random clips
against stock torch.nn.LSTM on the CPU in FLOAT64 with the same weights (tests/converter_ref.py's module), so that a clip
computed from another clip's rows, hidden state or exchange granules is an error of order 0.1.

Tolerance 1e-4 absolute, the one tests/test_gpu_lstm.py derives.  Every case first asserts on the reference alone that torch's own
f32-vs-f64 difference lies 10x below it and that the recurrence carries at least 100x of it (max|y - y(W_hh = 0)| >= 1e-2) --
except at T = 1, where no recurrent term exists (asserted: the difference is exactly 0) and the case is about the walk that makes
no exchange at all.  On a failure the per-clip errors are printed with each clip's launch, group and slot (group path) or block
and slot (safe path)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-4
H = 384
LAUNCH_CLIPS, GROUPS, SAFE_CLIPS = 128, 8, 4
FAULTS = []                           # fault counts seen by the tests of this file, checked by the last one

# clips per group 1..16, a short last group (127 -> 15, 9 -> 1), groups that leave at once (9: 5-7, 17: 6-7); 4 / 5 / 8: the
# 4-clip blocks of the safe kernel at an exact multiple and one past it
DEALING = [(B, 5, 56) for B in (2, 4, 5, 7, 8, 9, 15, 16, 17, 31, 120, 127, 128)]
# second launches of 1, 2 and 16 clips, three launches; one case on the K = 768 projection
LAUNCHES = [(B, T, 56) for B in (129, 130, 144, 257) for T in (2, 9)] + [(130, 3, 768)]
# T = 1: no exchange; T = 2, 3: the first use of each parity buffer
SHORTEST = [(B, T, 56) for T in (1, 2, 3) for B in (1, 5, 17, 129)]
CASES = list(dict.fromkeys(DEALING + LAUNCHES + SHORTEST))


def placement(b, B, safe):
    """where clip ``b`` of a batch of ``B`` runs, by the dealing rule of csrc/lstm.hip"""
    if safe:
        return "block %d slot %d" % (b // SAFE_CLIPS, b % SAFE_CLIPS)
    launch, r = divmod(b, LAUNCH_CLIPS)
    nb = min(LAUNCH_CLIPS, B - launch * LAUNCH_CLIPS)
    ngrp = min(GROUPS, nb)
    per = -(-nb // ngrp)
    return "launch %d group %d slot %d (of %d a group)" % (launch, r // per, r % per, per)


def test_placement_restates_the_dealing_rule():
    assert placement(8, 9, False) == "launch 0 group 4 slot 0 (of 2 a group)"
    assert placement(126, 127, False) == "launch 0 group 7 slot 14 (of 16 a group)"
    assert placement(16, 17, False) == "launch 0 group 5 slot 1 (of 3 a group)"
    assert placement(129, 130, False) == "launch 1 group 1 slot 0 (of 1 a group)"
    assert placement(143, 144, False) == "launch 1 group 7 slot 1 (of 2 a group)"
    assert placement(256, 257, False) == "launch 2 group 0 slot 0 (of 1 a group)"
    assert placement(129, 130, True) == "block 32 slot 1"


def _ref(m, x, dtype, zero_hh=False):
    mm = torch.nn.LSTM(m.input_size, H, 1, batch_first=True, bidirectional=True).to(dtype)
    sd = {k: (torch.zeros_like(v) if zero_hh and k.startswith("weight_hh") else v).to(dtype) for k, v in m.state_dict().items()}
    mm.load_state_dict(sd)
    with torch.no_grad():
        return mm(x.to(dtype))[0]


@functools.lru_cache(maxsize=None)
def _case(B, T, In, scale=1.0):
    """(module, x, float64 reference) of a case, computed once; the two preconditions are asserted on the reference alone"""
    import converter_ref
    m = converter_ref.lstm_module(In, scale=scale, seed=9000 + 7 * B + T + In)
    x = torch.randn(B, T, In, generator=torch.Generator().manual_seed(100 * B + T))
    ref = _ref(m, x, torch.float64)
    noise = (_ref(m, x, torch.float32).double() - ref).abs().max().item()
    share = (ref - _ref(m, x, torch.float64, zero_hh=True)).abs().max().item()
    print("reference B=%d T=%d In=%d scale=%g: max|y|=%.3f, torch f32 vs f64 %.1e, recurrent share %.2e"
          % (B, T, In, scale, ref.abs().max().item(), noise, share))
    assert noise * 10 <= TOL, "torch's own f32 noise %g is not 10x below the tolerance" % noise
    if T == 1:
        assert share == 0.0     # one frame: W_hh meets the zero initial state only
    else:
        assert share >= 100 * TOL, "the case does not exercise the recurrence (share %g)" % share
    return m, x, ref


def _run(m, x, safe):
    import converter_ref
    from dimx import engine as E
    w_ih, w_hh, b_ih, b_hh = converter_ref.pairs(m.state_dict())
    y, faults = E.op_lstm_layer(x.cuda(), w_ih, w_hh, b_ih, b_hh, safe=safe, return_faults=True)
    FAULTS.append(faults)
    return y, faults


def _clip_report(err_clip, B, safe, limit=48):
    bad = [b for b in range(B) if not err_clip[b] < TOL]
    lines = ["  clip %d: err %.2e  %s" % (b, err_clip[b], placement(b, B, safe)) for b in bad[:limit]]
    if len(bad) > limit:
        lines.append("  ... and %d more" % (len(bad) - limit))
    return "%d of %d clips are wrong:\n%s" % (len(bad), B, "\n".join(lines))


def _check_both_paths(m, x, ref, tag):
    B = x.shape[0]
    worst = 0.0
    for safe in (False, True):
        path = "safe" if safe else "group"
        y, faults = _run(m, x, safe)
        err_clip = (y.cpu().double() - ref).abs().amax(dim=(1, 2))
        err = err_clip.max().item()
        worst = max(worst, err)
        print("%s %s path: err=%.2e (worst clip %d, %s) faults=%d"
              % (tag, path, err, int(err_clip.argmax()), placement(int(err_clip.argmax()), B, safe), faults))
        assert faults == 0, "%s: the %s path counted a fault" % (tag, path)
        if not err < TOL:
            report = _clip_report(err_clip.tolist(), B, safe)
            print(report)
            pytest.fail("%s: %s path differs from float64 torch.nn.LSTM by %g; %s" % (tag, path, err, report))
        y2, _ = _run(m, x, safe)
        assert torch.equal(y, y2), "%s: %s path is not bit-identical across two runs" % (tag, path)
    return worst


@pytest.mark.parametrize("B,T,In", CASES)
def test_every_clip_lands_in_its_own_rows(B, T, In):
    m, x, ref = _case(B, T, In)
    _check_both_paths(m, x, ref, "lstm dealing B=%d T=%d In=%d" % (B, T, In))


def test_full_groups_with_a_saturating_recurrence():
    """B = 128: sixteen clips in each of the eight groups -- every thread is a cell-update thread and polls sixteen granules a
    step -- for 27 steps at weights x 4, where the gates saturate (the precondition of tests/test_gpu_lstm.py: max|y_ref| > 0.9)"""
    m, x, ref = _case(128, 27, 56, 4.0)
    assert ref.abs().max().item() > 0.9
    _check_both_paths(m, x, ref, "lstm full occupancy B=128 T=27 In=56 scale=4")


DUPLICATES = (0, 15, 16, 127, 128, 129)


def test_copies_of_a_clip_are_bit_equal_wherever_they_are_dealt():
    """Clip 0's input copied into clips 15, 16, 127, 128 and 129 of a B = 130 batch: the last slot of its own group, the first of
    the next, the last of the launch and both clips of the second launch (block 0 / 3 / 4 / 31 / 32 of the safe path).  The rows go
    through the same GEMM at the same M and a clip's recurrence depends on nothing but the clip, so the six outputs are bit-equal
    on each path.  If they are not, the input projection alone (the layer's own GEMM: K padded to 64, N = 3072) says which half
    differs."""
    from dimx import engine as E
    import converter_ref
    B, T, In = 130, 9, 56
    m, x, _ = _case(B, T, In)
    x = x.clone()
    for b in DUPLICATES[1:]:
        x[b] = x[0]
    ref = _ref(m, x, torch.float64)
    for safe in (False, True):
        path = "safe" if safe else "group"
        y, faults = _run(m, x, safe)
        err = (y.cpu().double() - ref).abs().max().item()
        differ = [b for b in DUPLICATES[1:] if not torch.equal(y[b], y[0])]
        print("lstm duplicate clips %s path: err=%.2e faults=%d, copies that differ from clip 0: %s" % (path, err, faults, differ))
        assert faults == 0 and err < TOL
        if differ:
            (wf, wr), _, (bf, br), (hf, hr) = converter_ref.pairs(m.state_dict())
            w = torch.nn.functional.pad(torch.cat([wf, wr]), (0, 8)).cuda()
            pre = E.op_gemm(torch.nn.functional.pad(x.reshape(B * T, In), (0, 8)).cuda(), w, bias=torch.cat([bf + hf, br + hr]).cuda())
            pre = pre.reshape(B, T, -1)
            pre_differ = [b for b in differ if not torch.equal(pre[b], pre[0])]
            worst = max((y[b] - y[0]).abs().max().item() for b in differ)
            pytest.fail("%s path: copies of clip 0 at %s differ from it by up to %g (%s); the input projection alone differs at %s: "
                        "the %s is not a function of the clip alone"
                        % (path, differ, worst, "; ".join("clip %d: %s" % (b, placement(b, B, safe)) for b in differ), pre_differ,
                           "projection" if pre_differ else "recurrence"))


def _converter():
    from dimx import lib
    from dimx.seq2seq_pretrain import EmocaConverter
    return EmocaConverter(mesh_dim=150, numeric_mode=lib.MODE_PARITY_F32).cuda()


def test_a_second_call_sees_nothing_of_the_first_calls_exchange():
    """The tags of an earlier call (step + 1) are the tags a later call waits for, and a handle keeps one exchange buffer: only the
    clear in front of every launch stands between them.  (B = 17, T = 5), then (B = 17, T = 12) with other inputs, then (B = 17,
    T = 12) with a third input on one engine -- the buffer's place in the workspace depends on B x T, so it is the third call whose
    granules lie exactly where the second left tags 1..11.  The second and the third mesh equal those of a fresh engine with the
    same weights bit for bit, on both paths."""
    g = torch.Generator().manual_seed(31)
    first = torch.randn(17, 5, 56, generator=g).cuda()
    second = torch.randn(17, 12, 56, generator=g).cuda()
    third = torch.randn(17, 12, 56, generator=g).cuda()
    templ = (0.1 * torch.randn(17, 150, generator=g)).cuda()
    for safe in (False, True):
        used = _converter().engine("cuda:0")
        used.mesh_head(first, templ, safe=safe)
        for name, motion in (("second", second), ("third", third)):
            got = used.mesh_head(motion, templ, safe=safe).clone()
            fresh = _converter().engine("cuda:0")
            want = fresh.mesh_head(motion, templ, safe=safe)
            FAULTS.append(fresh.lstm_faults())
            diff = (got - want).abs().max().item()
            print("mesh_head, %s call on a used engine, %s path: max|used - fresh| = %.2e, max|mesh| = %.3f"
                  % (name, "safe" if safe else "group", diff, want.abs().max().item()))
            assert torch.isfinite(want).all() and want.abs().max().item() > 0
            assert torch.equal(got, want), "the %s call on a used engine differs from a fresh engine by %g" % (name, diff)
        FAULTS.append(used.lstm_faults())


def test_zz_no_lstm_fault_was_counted():
    """last in the file: no bounded wait of a group kernel timed out in any call above"""
    assert FAULTS and sum(FAULTS) == 0, FAULTS
