"""Beam search: what a generation costs against sampling the same number of rows, the cache reorder alone, and the benchmark line.
    python tools/bench_beam.py [--parent-tree DIR] [--pairs 3] [--widths 4 10] [--modes bf16 f32] [--out profiles/beam_search.txt]

One MI355X.  B = 256 clips of T = 300 frames (lengths spread over 24 .. 300), synthetic weights.
a. Engine.generate_beam(W) against Engine.generate(n_samples=W, seed) on the same handle and context: alternating runs, host clock
   around a call that ends in a device synchronise, median of 5 (min .. max).
b. beam_reorder_kernel alone (dimx_op_beam_reorder on one cache [256 W, 12, 300, 64]; the step runs it over 8 such caches in one
   launch) with every clip permuted by a cycle, at c = 149 and c = 298: median of 9 launches between device events, and GB/s of the
   bytes it moves (read + write of W rows x 12 heads x (c + 1) positions x 64 elements per clip).
c. The fraction of clips whose parent vector is the identity (the reorder skips them), per step: one generation's dumped logits
   replayed by the definition in torch float64.
d. python bench.py --gpus 1 --steps 20 --warmup 5, the parent tree and this tree alternating in one visit (--parent-tree: a
   checkout of the parent commit with its library built; without it this part is "not measured")."""
import argparse
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
sys.path.insert(0, "tools")
import dimx  # noqa: F401,E402
from dimx import engine, lib as L, prng, weights  # noqa: E402
import bench_sampler  # noqa: E402

B, T, RUNS = 256, 300, 5


def _inputs():
    lens = np.linspace(24, T, B).astype(int)
    mask = torch.zeros(B, T, dtype=torch.bool)
    for j, n in enumerate(lens):
        mask[j, :n] = True
    v_s = torch.from_numpy(prng.normal(3, "bench.beam.vs", (B, T, 56))).cuda()
    v_a = torch.from_numpy(prng.normal(3, "bench.beam.va", (B, T, 768))).cuda()
    start = torch.from_numpy(prng.integers(3, "bench.beam.start", (B,), 0, 512)).to(torch.int32).cuda()
    return v_s, v_a, mask.to(torch.uint8).cuda(), start


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _identity_fraction(e, start, m8, W):
    """replay of one generation's dumped logits (rows in the order each step ran in) by the definition in torch float64: per step,
    the clips whose W parents are 0 .. W-1 -- frozen steps (past the clip's length) included, they are the identity by definition"""
    _, _, lg = e.generate_beam(start, m8, T, W, return_logits=True)
    n = lg.shape[1]
    last = m8.sum(1).long() - 1
    cum = torch.full((B, W), float("-inf"), dtype=torch.float64, device="cuda")
    cum[:, 0] = 0
    same = torch.zeros(n, device="cuda")
    iota = torch.arange(W, device="cuda")[None, :]
    for c in range(n):
        sc = (cum[:, :, None] + torch.log_softmax(lg[:, c].view(B, W, 512).double(), -1)).view(B, W * 512)
        top, idx = sc.topk(W, dim=1)
        live = (c < last)[:, None]
        parent = torch.where(live, idx // 512, iota)
        cum = torch.where(live, top, cum)
        same[c] = (parent == iota).all(1).float().mean()
    same = same.cpu().numpy()
    return ("identity at %.3f of the (clip, step) pairs; by step: first %.3f, step 1 %.3f, step %d %.3f, last %.3f"
            % (same.mean(), same[0], same[1], n // 2, same[n // 2], same[-1]))


def generation_lines(sd, widths, modes):
    lines = ["a. One generation of %d clips x %d frames (ms; alternating, median of %d, min .. max)" % (B, T, RUNS), ""]
    ident = ["c. Clips whose parent vector is the identity (the reorder skips them), per step of one generation", ""]
    v_s, v_a, m8, start = _inputs()
    for mode in modes:
        e = engine.Engine("cuda:0", L.MODE_PERF_BF16 if mode == "bf16" else L.MODE_PARITY_F32)
        e.load_state_dict(sd)
        for W in widths:
            e.encode_ctx(v_s, v_a, m8, True, n_samples=W)
            beam = lambda: e.generate_beam(start, m8, T, W)
            samp = lambda: e.generate(start, m8, T, 1.0, 52, None, 5, n_samples=W)
            beam(), samp()
            tb, ts = [], []
            for _ in range(RUNS):
                ts.append(_timed(samp))
                tb.append(_timed(beam))
            mb, ms = statistics.median(tb), statistics.median(ts)
            lines.append("   %-4s W = %2d   generate(n_samples=W) %9.1f (%.1f .. %.1f)   generate_beam %9.1f (%.1f .. %.1f)   beam / sample %.2f"
                         % (mode, W, ms, min(ts), max(ts), mb, min(tb), max(tb), mb / ms))
            print(lines[-1], flush=True)
            ident.append("   %-4s W = %2d   %s" % (mode, W, _identity_fraction(e, start, m8, W)))
        e.close()
    return lines + [""] + ident + [""]


def reorder_lines(widths):
    from dimx.engine import op_beam_reorder
    lines = ["b. beam_reorder_kernel alone: one cache [%d W, 12, %d, 64], every clip permuted by a cycle (ms, median of 9; GB/s of read + write)"
             % (B, T), ""]
    for dtype, name, es in ((torch.bfloat16, "bf16", 2), (torch.float32, "f32", 4)):
        for W in widths:
            cache = torch.zeros(B * W, 12, T, 64, dtype=dtype, device="cuda")
            parent = torch.tensor([(w + 1) % W for w in range(W)] * B, dtype=torch.int32, device="cuda")
            for c in (T // 2 - 1, T - 2):
                op_beam_reorder(cache, parent, c, W)
                ts = []
                for _ in range(9):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    op_beam_reorder(cache, parent, c, W)
                    e1.record()
                    torch.cuda.synchronize()
                    ts.append(e0.elapsed_time(e1))
                med = statistics.median(ts)
                gb = 2.0 * B * W * 12 * (c + 1) * 64 * es / 1e9
                lines.append("   %-4s W = %2d  c = %3d   %8.3f ms   %6.3f GB moved   %7.0f GB/s   (x 8 caches per step: %.2f ms)"
                             % (name, W, c, med, gb, gb / med * 1e3, 8 * med))
                print(lines[-1], flush=True)
            del cache
    return lines + [""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--widths", type=int, nargs="+", default=[4, 10])
    ap.add_argument("--modes", nargs="+", default=["bf16", "f32"])
    ap.add_argument("--out", default="profiles/beam_search.txt")
    args = ap.parse_args()
    torch.set_grad_enabled(False)
    if not torch.cuda.is_available():
        raise SystemExit("bench_beam needs a ROCm GPU: nothing is measured without one")
    sd = weights.synth_state_dict(weights.slmft_spec(), 20260928)
    lines = ["Beam search (dimx_generate_beam, csrc/beam.hip): measurements", "=" * 62,
             "One MI355X box, one visit.  tools/bench_beam.py%s" % (" --parent-tree <parent commit, built from its own sources>"
                                                                   if args.parent_tree else ""), ""]
    lines += reorder_lines(args.widths)
    lines += generation_lines(sd, args.widths, args.modes)
    torch.cuda.synchronize()
    d = bench_sampler.bench_lines(args.parent_tree, args.pairs)
    d[0] = "d." + d[0][2:]
    lines += d
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
