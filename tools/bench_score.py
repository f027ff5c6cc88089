"""Sequence log-likelihoods: what the scoring operator costs, what return_scores adds to a generation, and the benchmark line against
the parent commit.
    python tools/bench_score.py [--parent-tree DIR] [--pairs 3] [--out profiles/seq_score.txt]

One MI355X.
a. dimx_op_seq_logprob alone on logits [R, 299, 512] f32 (dimx.prng normals x 3) with per-clip ranges (lens spread over 24 .. 299),
   R = 2560 (256 clips x 10 rows) and R = 256 (one row per clip), against the same outputs (score, count) written in torch float64 on the same GPU:
   log_softmax of a float64 copy, gather at the tokens, masked sum.  Cold inputs: the timed calls rotate over enough input sets
   that their bytes exceed the 256 MB Infinity Cache several times over.  Each call is timed alone between device events after a
   warm-up; the figure is the median of REPS calls (min .. max).  The two forms are compared output for output first.
b. Engine.generate at 256 clips x 300 frames, n_samples = 10, bf16, seeded sampling, with and without return_scores (the context is
   rebuilt before every call, outside the timed region): median of REPS (min .. max), and the difference.
c. python bench.py --gpus 1 --steps 20 --warmup 5, the parent tree and this tree alternating in one visit (--parent-tree: a
   checkout of the parent commit with its library built; without it this part is "not measured").  No code on the benchmark's path
   changes, so the expectation is a difference inside the spread of two handles of one build."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dimx  # noqa: F401,E402
import bench_sampler  # noqa: E402
from dimx import engine as E, lib as L, prng, weights  # noqa: E402

REPS, WARM = 5, 2
N_COLS = 299
SEED = 20260928


def timed_ms(fn, n_sets):
    """median / min / max milliseconds of REPS calls fn(i), i rotating over the input sets, each between its own device events"""
    for i in range(WARM):
        fn(i % n_sets)
    torch.cuda.synchronize()
    out = []
    for i in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn((WARM + i) % n_sets)
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out), min(out), max(out)


def torch_f64_scores(logits, tokens, first, last, rpc):
    """the operator's outputs written in torch float64: (score f64 [R], count int32 [R])"""
    n = logits.shape[1]
    lp = torch.log_softmax(logits.double(), dim=2).gather(2, tokens.long().clamp(0, 511)[..., None])[..., 0]
    cols = torch.arange(n, device=logits.device)[None, :]
    use = (cols >= first.clamp(0, n).repeat_interleave(rpc)[:, None]) & (cols < last.clamp(0, n).repeat_interleave(rpc)[:, None]) \
        & (tokens >= 0) & (tokens < 512)
    return torch.where(use, lp, torch.zeros((), dtype=lp.dtype, device=lp.device)).sum(1), use.sum(1).to(torch.int32)


def operator_lines():
    lines = ["a. dimx_op_seq_logprob alone against torch float64 (log_softmax, gather, masked sum) on the same GPU, n = %d" % N_COLS,
             "   ms per call: median of %d (min .. max), cold inputs" % REPS, ""]
    dev = torch.device("cuda:0")
    for R in (2560, 256):
        n_sets, RPC = (2, 10) if R == 2560 else (6, 1)       # 1.57 GB / 157 MB of logits per set
        sets = []
        for k in range(n_sets):
            lg = torch.empty(R, N_COLS, 512, dtype=torch.float32, device=dev)
            base = torch.from_numpy(prng.normal(31 + k, "bench.score.logits", (64, N_COLS, 512))).to(dev) * 3
            for r0 in range(0, R, 64):       # 64 rows of host normals per set; the further rows are their vocabulary rotations
                lg[r0:r0 + 64] = base.roll(r0 // 64, 2)
            del base
            tok = torch.from_numpy(prng.integers(31 + k, "bench.score.tok", (R, N_COLS), 0, 512).astype(np.int32)).to(dev)
            last = torch.from_numpy(prng.integers(31 + k, "bench.score.len", (R // RPC,), 24, N_COLS + 1).astype(np.int32)).to(dev)
            first = torch.zeros_like(last)
            sets.append((lg, tok, first, last))
        lg, tok, first, last = sets[0]
        mine = E.op_seq_logprob(lg, tok, first, last, rows_per_clip=RPC)
        ref_s, ref_c = torch_f64_scores(lg, tok, first, last, RPC)
        d = ((mine.score - ref_s).abs() / ref_c.clamp(min=1)).max().item()
        assert torch.equal(mine.count, ref_c)
        scored = int(ref_c.sum())
        op = timed_ms(lambda i: E.op_seq_logprob(*sets[i], rows_per_clip=RPC), n_sets)
        th = timed_ms(lambda i: torch_f64_scores(*sets[i], RPC), n_sets)
        gb = scored * 2048 / 1e9
        lines += ["   R = %d, %d row(s) per clip (%d scored columns, %.3f GB of logits in range; worst |operator - torch f64| per counted token %.2e)"
                  % (R, RPC, scored, gb, d),
                  "     dimx_op_seq_logprob   %8.3f (%.3f .. %.3f)   %.0f GB/s of the logits in range" % (op + (gb / op[0] * 1e3,)),
                  "     torch float64         %8.3f (%.3f .. %.3f)   operator %.1fx %s" % (th + (max(th[0], op[0]) / min(th[0], op[0]),
                                                                                              "faster" if op[0] < th[0] else "SLOWER")), ""]
        print("\n".join(lines[-4:]), flush=True)
        del sets, lg, tok, first, last
        torch.cuda.empty_cache()
    return lines


def generate_lines():
    B, T, S = 256, 300, 10
    dev = torch.device("cuda:0")
    eng = E.Engine(dev, L.MODE_PERF_BF16)
    eng.load_state_dict(weights.synth_state_dict(weights.slmft_spec(), SEED))
    v_s = torch.from_numpy(prng.normal(SEED, "bench.v_speaker", (B, T, 56))).to(dev)
    v_a = torch.from_numpy(prng.normal(SEED, "bench.v_audio", (B, T, 768))).to(dev)
    m8 = torch.ones(B, T, dtype=torch.uint8, device=dev)
    start = torch.zeros(B, dtype=torch.int32, device=dev)

    def run(return_scores):
        out = []
        for i in range(WARM + REPS):
            eng.encode_ctx(v_s, v_a, m8, True, n_samples=S)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            res = eng.generate(start, m8, T, 1.0, seed=5, n_samples=S, return_scores=return_scores)
            e1.record()
            torch.cuda.synchronize()
            del res
            if i >= WARM:
                out.append(e0.elapsed_time(e1))
        return statistics.median(out), min(out), max(out)

    plain, scored = run(False), run(True)
    lines = ["b. Engine.generate, %d clips x %d frames, n_samples = %d, bf16, seeded sampling; ms per call: median of %d (min .. max)" % (B, T, S, REPS), "",
             "     without return_scores   %9.2f (%.2f .. %.2f)" % plain,
             "     with return_scores      %9.2f (%.2f .. %.2f)   %+.2f ms: the logits dump (%.2f GB written per call) and the scoring launch"
             % (scored + (scored[0] - plain[0], B * S * (T - 1) * 2048 / 1e9)), ""]
    print("\n".join(lines), flush=True)
    eng.close()
    return lines


def bench_lines(parent_tree, pairs):
    lines = bench_sampler.bench_lines(parent_tree, pairs)      # the same alternating pairs, under this file's numbering
    lines[0] = "c." + lines[0][2:]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--out", default="profiles/seq_score.txt")
    args = ap.parse_args()
    torch.set_grad_enabled(False)
    if not torch.cuda.is_available():
        raise SystemExit("bench_score needs a ROCm GPU: nothing is measured without one")
    lines = ["Sequence log-likelihoods (dimx_op_seq_logprob, return_scores): measurements", "=" * 75,
             "One MI355X box, one visit.  tools/bench_score.py%s" % (" --parent-tree <parent commit, built from its own sources>"
                                                                    if args.parent_tree else ""), ""]
    lines += operator_lines()
    lines += generate_lines()
    torch.cuda.synchronize()
    lines += bench_lines(args.parent_tree, args.pairs)
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
