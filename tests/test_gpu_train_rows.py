"""GPU: the whole main training step (dimx_train_forward_backward) across its row-count thresholds, at the library's own
defaults (no environment switches), by an exact decomposition into steps of the shape autograd already pins.

The step's loss is the mean cross entropy over the valid targets and clips do not interact, so for any partition of a batch into
groups g with n_g valid targets (tests/test_train_cpu.py checks this on the oracle in float64 to 1e-10)
    loss(batch) = sum_g n_g loss(g) / sum_g n_g,     grad(batch) = sum_g n_g grad(g) / sum_g n_g.
The reference is the sum over PAIR steps (B = 2, T = 48: the shape test_hip_gradients_match_autograd_over_the_oracle_f32 holds to
autograd over the CPU oracle), accumulated in float64.  44 pairs are built once; their prefixes are the references of
    B =  6   288 rows   bias column sums in 32 slabs (>= 256 rows), still 4 LayerNorm rows per block
    B = 44  2112 rows   GEMM output through the staged epilogue (M >= 2048), still a captured graph
    B = 52  2496 rows   8 LayerNorm rows per block (M > 2400): a wave loops over two rows
    B = 88  4224 rows   (4136 decoder rows) kernel by kernel with the weight gradients on the side stream (>= 4096 rows), bf16
                        GEMMs on gemm256 (M >= 4096), cross entropy over 4136 rows

Measured on an MI355X (parity mode: worst tensor, max |g - reference| relative to the tensor's max; the bound is 1e-3):
    B =  6  2.6e-6  decoder_joint.net.attn_layers.layers.8.0.0.weight      loss 6.3288717 vs 6.3288720
    B = 44  2.7e-6  decoder_joint.net.attn_layers.layers.8.0.0.weight      loss 6.3960958 vs 6.3960959
    B = 52  2.4e-6  encoder_s.attn_layers.layers.2.1.to_k.weight           loss 6.3974791 vs 6.3974785
    B = 88  2.9e-6  encoder_s.attn_layers.layers.0.1.to_v.weight           loss 6.3959694 vs 6.3959696
bf16 mode, B = 88: relative norm to the parity-mode pair sum 0.0042 (bound 0.05).  Per tensor against the bf16 pair sum: the floor
(pairs vs groups of four) is at most 1.04e-2 of a tensor's max, the large batch deviates by at most 9.1e-3; the worst ratio is
1.37 (decoder_joint.net.attn_layers.layers.0.0.0.weight: floor 4.6e-3, large batch 6.3e-3; the bound is 4).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

T = 48
PAIRS = 44
BATCHES = (6, 44, 52, 88)


def _rel_per_tensor(layout, a, b, ref):
    """{name: max |a - b| / max |ref|} over the tensors of the arena layout (float64 device tensors)"""
    out = {}
    for name, off, numel in layout:
        scale = ref[off:off + numel].abs().max().item()
        out[name] = (a[off:off + numel] - b[off:off + numel]).abs().max().item() / max(scale, 1e-30)
    return out


class _Data:
    def __init__(self):
        from dimx import prng
        B = 2 * PAIRS
        self.v_s = torch.from_numpy(prng.normal(53, "rows.vs", (B, T, 56))).cuda()
        self.v_a = torch.from_numpy(prng.normal(53, "rows.va", (B, T, 768))).cuda()
        z = torch.from_numpy(prng.integers(53, "rows.z", (B, T), 0, 512))
        lens = torch.from_numpy(prng.integers(53, "rows.len", (B,), 8, T + 1))        # ragged
        lens[0], lens[3], lens[2 * PAIRS - 1] = T, 2, 2                                 # a full clip, clips of length 2
        self.mask = (torch.arange(T)[None, :] < lens[:, None]).cuda()
        self.z = torch.where(self.mask.cpu(), z, torch.full_like(z, -100)).cuda()
        kv = torch.from_numpy(prng.integers(53, "rows.kv", (B, T - 1), 0, 8)) != 0     # an explicit mask_prob draw per clip
        kv[:, 0] = True                                                                # AutoregressiveWrapper never drops the first token
        self.kv = kv.cuda()
        self.valid = (self.z[:, 1:] >= 0).sum(1).cpu()                                  # valid targets per clip

    def run(self, tr, lo, hi):
        """one forward_backward over clips lo..hi -> (loss as float, valid targets)"""
        loss = tr.forward_backward(self.v_s[lo:hi], None, self.v_a[lo:hi], self.mask[lo:hi], kv_mask=self.kv[lo:hi], z_l=self.z[lo:hi])
        return loss.item(), int(self.valid[lo:hi].sum())


def _trainer(mode):
    from dimx import train_hip
    from dimx.seq2seq_pretrain import SLMFT
    return train_hip.HipTrainer(SLMFT(numeric_mode=mode).cuda())


def _decompose(data, tr, group, stops):
    """count-weighted float64 sums of the gradients / losses of consecutive groups of `group` clips; snapshots {clips: (gradient,
    loss, valid targets)} of the prefixes `stops`, each divided by its valid targets.  The sum is kept in float64 on the device."""
    g = torch.zeros(tr.total, dtype=torch.float64, device="cuda")
    loss_sum, n_sum, snaps = 0.0, 0, {}
    for lo in range(0, max(stops), group):
        loss, n = data.run(tr, lo, lo + group)
        g.add_(tr.grads.double(), alpha=float(n))
        loss_sum += n * loss
        n_sum += n
        if lo + group in stops:
            snaps[lo + group] = (g / n_sum, loss_sum / n_sum, n_sum)
    return snaps


@pytest.fixture(scope="module")
def data():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return _Data()


@pytest.fixture(scope="module")
def parity(data):
    """the parity-mode trainer and the pair-step references of every batch size"""
    from dimx import lib
    tr = _trainer(lib.MODE_PARITY_F32)
    return tr, _decompose(data, tr, 2, set(BATCHES))


@pytest.fixture(scope="module")
def perf(data):
    """the bf16-mode trainer, the pair-step reference of B = 88 and the same sum over groups of four (192 rows: both stay on the
    small-row path)"""
    from dimx import lib
    tr = _trainer(lib.MODE_PERF_BF16)
    return tr, _decompose(data, tr, 2, {88})[88], _decompose(data, tr, 4, {88})[88]


def test_the_fixture_batch_is_ragged_with_clips_of_length_two(data):
    lens = data.mask.sum(1).cpu()
    assert lens.min().item() == 2 and lens.max().item() == T and len(set(lens.tolist())) > 20
    assert data.valid[3].item() == 1 and (data.valid == lens - 1).all() and not data.kv.all()


@pytest.mark.parametrize("B", BATCHES)
def test_parity_step_equals_the_sum_of_its_pair_steps(B, data, parity):
    """One forward_backward of B clips (T = 48) at the library's defaults against the count-weighted float64 sum of its B / 2 pair
    steps.  B = 6: 288 rows -- bias_adjoint / tr_colsum_partial in 32 slabs; B = 44: 2112 rows -- launch_gemm's staged epilogue
    (M >= 2048), with dx accumulated onto itself and the residual stream as the output, still train_use_graph; B = 52: 2496 rows
    -- ln_adjoint at 8 rows per block; B = 88: 4224 rows, 4136 decoder rows -- train_use_side without a graph, tr_prep_fused with
    256-column chunks, ce_count_kernel / sum_scale_kernel over 4136 rows.  Loss 1e-5 relative; every tensor of tr.layout within
    1e-3 of the reference relative to the tensor's max (the project's bar for a gradient); a second run bit-identical;
    dimx_train_graph_stats: a graph launch for B <= 52, kernel by kernel for B = 88."""
    tr, refs = parity
    g_ref, loss_ref, n_ref = refs[B]
    s0 = tr.graph_stats()
    loss, n = data.run(tr, 0, B)
    assert n == n_ref and abs(loss - loss_ref) <= 1e-5 * abs(loss_ref), (loss, loss_ref)
    g1 = tr.grads.clone()
    assert torch.isfinite(g1).all()
    errs = _rel_per_tensor(tr.layout, g1.double(), g_ref, g_ref)
    worst = max(errs, key=errs.get)
    print("parity step B=%d (%d rows): loss %.7f vs pair sum %.7f; worst tensor %s: %.3e of its max" % (B, B * T, loss, loss_ref, worst, errs[worst]))
    bad = {k: v for k, v in errs.items() if not v <= 1e-3}
    assert not bad, "B=%d: %d tensors above 1e-3, e.g. %s" % (B, len(bad), sorted(bad.items(), key=lambda kv: -kv[1])[:5])
    loss2, _ = data.run(tr, 0, B)
    assert loss2 == loss and torch.equal(tr.grads, g1)
    s1 = tr.graph_stats()
    launched = (s1[0] - s0[0], s1[1] - s0[1])
    assert launched == ((1, 1) if B <= 52 else (0, 2)), launched     # first call kernel by kernel; the repeat is captured below 4096 rows


def test_bf16_step_at_4224_rows_stays_at_the_decomposition_floor(data, parity, perf):
    """bf16 mode at B = 88 (gemm256 from M >= 4096, the side stream, every large-row branch at once): within 0.05 in relative norm
    of the parity-mode pair-step reference (the bar of test_hip_training_reduces_the_loss_and_bf16_mode_agrees), and per tensor
    against the bf16 pair-step sum.  For the latter no bound can be derived -- reordered f32 accumulation can flip a bf16 ulp
    downstream -- so the floor is measured: the per-tensor deviation between two bf16 decompositions that never leave the small-row
    path, pairs and groups of four.  The large batch must stay within 4 x that floor (the factor: reordered f32 accumulation in the
    larger tiles)."""
    tr, (g_pairs, loss_pairs, n_pairs), (g_fours, loss_fours, _) = perf
    g_f32 = parity[1][88][0]
    s0 = tr.graph_stats()
    loss, n = data.run(tr, 0, 88)
    s1 = tr.graph_stats()
    assert n == n_pairs and (s1[0] - s0[0], s1[1] - s0[1]) == (0, 1)
    g = tr.grads.double()
    assert torch.isfinite(g).all()
    rel = ((g - g_f32).norm() / g_f32.norm()).item()
    print("bf16 step B=88: loss %.5f (bf16 pairs %.5f, fours %.5f), relative gradient difference to the f32 pair sum %.4f" % (loss, loss_pairs, loss_fours, rel))
    assert rel < 0.05 and abs(loss - loss_pairs) < 2e-2
    floor = _rel_per_tensor(tr.layout, g_fours, g_pairs, g_pairs)
    dev = _rel_per_tensor(tr.layout, g, g_pairs, g_pairs)
    ratio = {k: dev[k] / floor[k] if floor[k] > 0 else (0.0 if dev[k] == 0 else float("inf")) for k in dev}
    worst = max(ratio, key=ratio.get)
    print("bf16 step B=88 per tensor: floor (pairs vs fours) max %.3e, large batch vs pairs max %.3e, worst ratio %.2f at %s (floor %.3e, got %.3e)"
          % (max(floor.values()), max(dev.values()), ratio[worst], worst, floor[worst], dev[worst]))
    bad = {k: (dev[k], floor[k]) for k in dev if not dev[k] <= 4.0 * floor[k]}
    assert not bad, "%d tensors above 4 x their floor, e.g. %s" % (len(bad), sorted(bad.items(), key=lambda kv: -ratio[kv[0]])[:5])
