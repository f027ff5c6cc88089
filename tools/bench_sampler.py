"""Sampler filters: what a launch of sample_kernel costs under each filter kind, and the benchmark line against the parent commit.
    python tools/bench_sampler.py [--parent-tree DIR] [--pairs 3] [--out profiles/sampler_filters.txt]

One MI355X.
1. The sampler launch alone (no fused embedding row): R = 256 and R = 2560 rows of 512 logits, dimx.prng normals at scales 1 and 3,
   temperature 1, noise from the device generator (seed 5).  LAUNCHES launches are captured into one graph, so that the kernels
   follow each other without the host's enqueue in between; the graph is replayed REPS times between device events after a
   warm-up, and the figure is the median time per launch (min .. max).  Lines: dimx_op_sample (top-k 52) of the parent commit's
   library (with --parent-tree), of this tree, and dimx_op_sample_filtered with each new kind.
2. python bench.py --gpus 1 --steps 20 --warmup 5, the parent tree and this tree alternating in one visit (--parent-tree: a
   checkout of the parent commit with its library built; without it this part is "not measured")."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

import torch

sys.path.insert(0, ".")
import dimx  # noqa: F401,E402
from dimx import lib as L, prng, sampling  # noqa: E402

LAUNCHES, REPS, WARM = 500, 9, 3
KINDS = [("top_p", {"thres": 0.9}), ("top_p", {"thres": 0.5}), ("min_p", {"min_p": 0.1}), ("top_a", {})]


def load_other(path):
    lib = ctypes.CDLL(path)
    for name, (res, args) in L.SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
    return lib


def per_launch_us(launch):
    """median / min / max microseconds per launch over REPS replays of a graph of LAUNCHES launches"""
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        launch(L.stream_ptr())
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for _ in range(LAUNCHES):
                launch(L.stream_ptr())
        for _ in range(WARM):
            g.replay()
        torch.cuda.synchronize()
        out = []
        for _ in range(REPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) * 1000.0 / LAUNCHES)
    return statistics.median(out), min(out), max(out)


def sampler_lines(parent):
    tree = L.load()
    lines = ["1. One sampler launch (us; median of %d replays of a graph of %d launches, min .. max), temperature 1, device generator"
             % (REPS, LAUNCHES), ""]
    for R in (256, 2560):
        for scale in (1, 3):
            lg = (torch.from_numpy(prng.normal(7, "bench.sampler.%d.%d" % (R, scale), (R, 512))) * scale).cuda()
            tok = torch.empty(R, dtype=torch.int32).cuda()
            surv = {("%s %s" % (k, kw)): int(sampling.keep_mask(lg[:256].cpu().numpy(), k, **kw).sum(1).mean()) for k, kw in KINDS}
            lines.append("   R = %d, normal logits x %d" % (R, scale))
            rows = []
            if parent is not None:
                rows.append(("parent commit: dimx_op_sample, top-k 52",
                             lambda s: L.check(parent.dimx_op_sample(L.ptr(lg), R, 52, 1.0, None, 5, 0, L.ptr(tok), s))))
            rows.append(("this tree:     dimx_op_sample, top-k 52",
                         lambda s: L.check(tree.dimx_op_sample(L.ptr(lg), R, 52, 1.0, None, 5, 0, L.ptr(tok), s))))
            rows.append(("this tree:     dimx_op_sample_filtered, kind 0, top-k 52",
                         lambda s: L.check(tree.dimx_op_sample_filtered(L.ptr(lg), R, 0, 52, 0.0, 0.0, 1.0, None, 5, 0, L.ptr(tok), None, s))))
            for k, kw in KINDS:
                kind, _, a, b = sampling.resolve(k, kw)
                rows.append(("this tree:     %s %s (mean survivors %d)" % (k, kw or sampling.DEFAULTS[k], surv["%s %s" % (k, kw)]),
                             lambda s, kind=kind, a=a, b=b: L.check(tree.dimx_op_sample_filtered(
                                 L.ptr(lg), R, kind, 0, a, b, 1.0, None, 5, 0, L.ptr(tok), None, s))))
            base = None
            for name, fn in rows:
                med, lo, hi = per_launch_us(fn)
                if name.startswith("this tree:     dimx_op_sample,"):
                    base = med
                extra = "" if base is None or "filtered" not in name else "   %+.2f us against this tree's top-k" % (med - base)
                lines.append("     %-78s %7.2f (%.2f .. %.2f)%s" % (name, med, lo, hi, extra))
                print(lines[-1], flush=True)
            lines.append("")
    return lines


def bench_line(tree_dir):
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"], cwd=tree_dir, capture_output=True,
                       text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError("bench.py failed in %s:\n%s" % (tree_dir, r.stderr[-2000:]))
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    return res


def headline(res):
    """(clips/s, ms per batch) of a bench.py result line"""
    v = float(res["value"])
    return v, 1000.0 * 256 / v


def bench_lines(parent_tree, pairs):
    lines = ["2. python bench.py --gpus 1 --steps 20 --warmup 5 (B = 256, T = 300, bf16, top-k 52), parent / tree alternating, every value", ""]
    if parent_tree is None:
        return lines + ["   not measured (no --parent-tree)", ""]
    lines.append("   pair   parent clips/s   ms per batch     tree clips/s   ms per batch")
    par, tre = [], []
    for i in range(pairs):
        p = headline(bench_line(parent_tree))
        t = headline(bench_line("."))
        par.append(p)
        tre.append(t)
        lines.append("   %d      %10.2f      %10.2f       %10.2f     %10.2f" % (i + 1, p[0], p[1], t[0], t[1]))
        print(lines[-1], flush=True)
    mp, mt = statistics.median(x[1] for x in par), statistics.median(x[1] for x in tre)
    lines += ["", "   median ms per batch: parent %.2f, tree %.2f, tree - parent = %+.2f ms (README: two handles of one build differ by "
              "0.5 - 1.0 ms)" % (mp, mt, mt - mp),
              "   ranges: parent %.2f .. %.2f ms, tree %.2f .. %.2f ms" % (min(x[1] for x in par), max(x[1] for x in par),
                                                                            min(x[1] for x in tre), max(x[1] for x in tre)), ""]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--out", default="profiles/sampler_filters.txt")
    args = ap.parse_args()
    torch.set_grad_enabled(False)
    if not torch.cuda.is_available():
        raise SystemExit("bench_sampler needs a ROCm GPU: nothing is measured without one")
    parent = None
    if args.parent_tree:
        parent = load_other(os.path.join(args.parent_tree, "dyadic-interaction-modeling_amd", "libdimx_hip.so"))
    lines = ["Sampler filters (top-p, min-p, top-a next to top-k): measurements", "=" * 66,
             "One MI355X box, one visit.  tools/bench_sampler.py%s" % (" --parent-tree <parent commit, built from its own sources>"
                                                                      if args.parent_tree else ""), ""]
    lines += sampler_lines(parent)
    torch.cuda.synchronize()
    lines += bench_lines(args.parent_tree, args.pairs)
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
