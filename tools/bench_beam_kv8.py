"""Beam search over FP8 K/V caches (dimx_set_beam_kv8): what it costs against the plain search, the two reorder kernels
alone, how far the FP8 search drifts from the plain one, and the benchmark line.
    python tools/bench_beam_kv8.py [--parent-tree DIR] [--pairs 3] [--widths 4 10] [--modes bf16 f32] [--out profiles/beam_kv8.txt]

One MI355X.  B = 256 clips of T = 300 frames (lengths spread over 24 .. 300), synthetic weights.
a. Engine.generate_beam(W) plain and with beam_kv8 = "self", "cross" and True (both) on one handle and context: the four variants
   alternating, host clock around a call that ends in a device synchronise, median of 5 (min .. max) after one warm-up round.
b. beam_reorder_kernel on one layer's K cache [256 W, 12, 300, 64] and beam_reorder_kv8_kernel on one layer's K codes
   [256 W, 12, 304, 64] + K scales [256 W, 12, 304], every clip permuted by a cycle, at c = 149 and c = 298: median of 9 launches
   between device events, and GB/s of the bytes moved (read + written).
c. Drift, report only: the free search with both buffers against the plain one (share of clips with the same best hypothesis, mean
   per-token difference of the best hypothesis's score), and dimx.kv8.drift on the teacher-forced logits of 32 clips (the whole clip
   forced through decode steps, W = 4).
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
from dimx import engine, kv8, lib as L, prng, weights  # noqa: E402
import bench_sampler  # noqa: E402
from bench_beam import B, T, RUNS, _inputs, _timed  # noqa: E402

VARIANTS = (("plain", None), ("self", "self"), ("cross", "cross"), ("both", True))
TF_CLIPS, TF_W = 32, 4


def generation_lines(sd, widths, modes):
    lines = ["a. One beam search of %d clips x %d frames (ms; the four variants alternating, median of %d, min .. max; x = against plain)"
             % (B, T, RUNS), ""]
    drift = ["c. Drift of the FP8 search (both buffers) from the plain one -- a report, not a claim: in bf16 the two searches round",
             "   differently at every step and a beam search amplifies the first flipped decision", ""]
    v_s, v_a, m8, start = _inputs()
    count = (m8.sum(1).double() - 1).clamp(min=1)
    for mode in modes:
        e = engine.Engine("cuda:0", L.MODE_PERF_BF16 if mode == "bf16" else L.MODE_PARITY_F32)
        e.load_state_dict(sd)
        for W in widths:
            e.encode_ctx(v_s, v_a, m8, True, n_samples=W)
            run = {name: (lambda kw=kw: e.generate_beam(start, m8, T, W, beam_kv8=kw)) for name, kw in VARIANTS}
            out = {name: fn() for name, fn in run.items()}        # the warm-up round; its results feed the drift report
            ts = {name: [] for name in run}
            for _ in range(RUNS):
                for name, fn in run.items():
                    ts[name].append(_timed(fn))
            med = {name: statistics.median(v) for name, v in ts.items()}
            lines.append("   %-4s W = %2d   " % (mode, W) + "   ".join(
                "%s %8.1f (%.1f .. %.1f)%s" % (name, med[name], min(ts[name]), max(ts[name]),
                                               "" if name == "plain" else " x %.3f" % (med[name] / med["plain"])) for name in run))
            print(lines[-1], flush=True)
            (ptok, psc), (ktok, ksc) = out["plain"], out["both"]
            same = (ptok.view(B, W, -1)[:, 0] == ktok.view(B, W, -1)[:, 0]).all(1).float().mean().item()
            dsc = ((ksc.view(B, W)[:, 0] - psc.view(B, W)[:, 0]) / count).abs()
            drift.append("   %-4s W = %2d   best hypothesis identical in %.3f of the clips; |best score (FP8) - best score (plain)| per token: "
                         "mean %.3e, max %.3e" % (mode, W, same, dsc.mean().item(), dsc.max().item()))
        # teacher-forced: the whole clip as a forced prompt, nothing prefilled -- every step's logits, no decision can diverge
        z = torch.from_numpy(prng.integers(3, "bench.beam_kv8.z", (TF_CLIPS, T - 1), 0, 512)).to(torch.int32).cuda()
        e.encode_ctx(v_s[:TF_CLIPS], v_a[:TF_CLIPS], m8[:TF_CLIPS].contiguous(), True, n_samples=TF_W)
        tf = {}
        for name, kw in (("plain", None), ("both", True)):
            tf[name] = e.generate_beam(None, m8[:TF_CLIPS].contiguous(), T, TF_W, prompt=z, prefill=1, return_logits=True, beam_kv8=kw)[2]
        keep = (torch.arange(T - 1, device="cuda")[None, :] < (m8[:TF_CLIPS].sum(1) - 1)[:, None]).repeat_interleave(TF_W, 0).cpu().numpy()
        d = kv8.drift(tf["both"].cpu().numpy()[keep], tf["plain"].cpu().numpy()[keep])
        drift.append("   %-4s teacher-forced, %d clips x W = %d, columns inside the clips: max |logit difference| %.3e, mean %.3e, max / spread "
                     "of the logits %.3e, same arg-max at %.4f of the (row, step) pairs"
                     % (mode, TF_CLIPS, TF_W, d["logit_max_abs"], d["logit_mean_abs"], d["logit_rel_to_spread"], d["argmax_equal"]))
        print(drift[-1], flush=True)
        e.close()
    return lines + [""], drift + [""]


def reorder_lines(widths):
    from dimx.engine import op_beam_reorder, op_beam_reorder_kv8
    Tp = (T + 7) // 8 * 8
    lines = ["b. The reorder kernels alone on one layer's K planes, every clip permuted by a cycle (ms, median of 9; GB/s of read + written;",
             "   a step runs 8 such planes -- K and V of 4 layers -- in one launch)", ""]

    def timed(fn):
        fn()
        ts = []
        for _ in range(9):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return statistics.median(ts)

    for W in widths:
        parent = torch.tensor([(w + 1) % W for w in range(W)] * B, dtype=torch.int32, device="cuda")
        planes = [("bf16 cache", torch.zeros(B * W, 12, T, 64, dtype=torch.bfloat16, device="cuda"), None, 128),
                  ("f32 cache ", torch.zeros(B * W, 12, T, 64, dtype=torch.float32, device="cuda"), None, 256),
                  ("FP8 planes", torch.zeros(B * W, 12, Tp, 64, dtype=torch.uint8, device="cuda"), torch.ones(B * W, 12, Tp, device="cuda"), 68)]
        for name, a, sc, row_bytes in planes:
            for c in (T // 2 - 1, T - 2):
                fn = (lambda: op_beam_reorder(a, parent, c, W)) if sc is None else (lambda: op_beam_reorder_kv8(a, sc, parent, c, W))
                med = timed(fn)
                gb = 2.0 * B * W * 12 * (c + 1) * row_bytes / 1e9
                lines.append("   %s W = %2d  c = %3d   %8.3f ms   %6.3f GB moved   %7.0f GB/s   (x 8 planes per step: %.2f ms)"
                             % (name, W, c, med, gb, gb / med * 1e3, 8 * med))
                print(lines[-1], flush=True)
        del planes
    return lines + [""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--widths", type=int, nargs="+", default=[4, 10])
    ap.add_argument("--modes", nargs="+", default=["bf16", "f32"])
    ap.add_argument("--out", default="profiles/beam_kv8.txt")
    args = ap.parse_args()
    torch.set_grad_enabled(False)
    if not torch.cuda.is_available():
        raise SystemExit("bench_beam_kv8 needs a ROCm GPU: nothing is measured without one")
    sd = weights.synth_state_dict(weights.slmft_spec(), 20260928)
    lines = ["Beam search over FP8 K/V caches (dimx_set_beam_kv8, csrc/beam.hip beam_reorder_kv8_kernel): measurements", "=" * 100,
             "One MI355X box, one visit.  tools/bench_beam_kv8.py%s" % (" --parent-tree <parent commit, built from its own sources>"
                                                                       if args.parent_tree else ""), ""]
    gen, drift = generation_lines(sd, args.widths, args.modes)
    lines += gen + reorder_lines(args.widths) + drift
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
