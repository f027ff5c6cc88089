"""Online generation (dimx_set_cross_lookahead): what the window costs, and that the default path did not move.
    python tools/bench_online.py [--parent-tree PATH] [--out profiles/online_generate.txt] [--pairs 3]

One MI355X.  Two measurements:

 1. Window on against window off on this tree: 256 clips x 300 frames, bf16, lookahead 0, seed 5, top-k 52; device-event time of
    dimx_generate per call.  A change of the setting captures a new step graph, so the two settings are timed in blocks (off, on,
    off, on), each block 2 warm-up calls and 5 timed ones.  With the window on the step streams fewer cross K/V bytes but runs the
    per-op launches instead of the decoder-layer kernel; no speed is promised either way.

 2. The default path against the parent commit: ``bench.py --gpus 1 --steps 20 --warmup 5`` (the flagship leg alone: the side
    legs are switched off by bench.py's own --no-* flags) as a fresh process in a built checkout of the parent commit
    (--parent-tree) and in this tree, alternating, --pairs pairs.  The spread is what the parent's own runs show, max - min of
    its clips/s; the tree's median has to lie no lower than the parent's median minus that spread.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, T, REPS, WARM = 256, 300, 5, 2
BENCH = ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5", "--no-cpu-baseline", "--no-roofline", "--no-mode-compare",
         "--no-parity-mode", "--no-train-step", "--no-shard-check", "--no-best-of-n"]


def window_on_off(lines):
    import torch
    sys.path.insert(0, ROOT)
    import dimx  # noqa: F401
    from dimx import engine, lib as L, prng, weights

    torch.set_grad_enabled(False)
    sd = weights.synth_state_dict(weights.slmft_spec(), 20260928)
    v_s = torch.from_numpy(prng.normal(3, "bo.vs", (B, T, 56))).cuda()
    v_a = torch.from_numpy(prng.normal(3, "bo.va", (B, T, 768))).cuda()
    start = torch.from_numpy(prng.integers(3, "bo.z", (B,), 0, 512)).to(torch.int32).cuda()
    m8 = torch.ones(B, T, dtype=torch.uint8).cuda()
    e = engine.Engine("cuda:0", L.MODE_PERF_BF16)
    e.load_state_dict(sd)
    e.encode_ctx(v_s, v_a, m8, True)

    def block(lookahead):
        e.set_cross_lookahead(lookahead)
        for _ in range(WARM):
            tok = e.generate(start, m8, T, 1.0, 52, None, 5)
        torch.cuda.synchronize()
        out = []
        for _ in range(REPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            tok = e.generate(start, m8, T, 1.0, 52, None, 5)
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1))
        return out, tok

    lines.append("1. window on against window off: dimx_generate, one MI355X, B = %d, T = %d, bf16, seed 5, top-k 52; device-event time per "
                 "call, median of %d after %d warm-up calls (min .. max), blocks in the order run" % (B, T, REPS, WARM))
    meds = {None: [], 0: []}
    toks = {}
    for la in (None, 0, None, 0):
        t, tok = block(la)
        meds[la].append(statistics.median(t))
        toks.setdefault(la, tok)
        lines.append("   %-22s %8.2f ms (%.2f .. %.2f)" % ("window off" if la is None else "window on, lookahead 0", statistics.median(t), min(t), max(t)))
        print(lines[-1], flush=True)
    off, on = statistics.mean(meds[None]), statistics.mean(meds[0])
    differ = (toks[None] != toks[0]).float().mean().item()
    lines.append("   mean of the block medians: off %.2f ms, on %.2f ms: on / off = %.3f; tokens that differ between the two settings: %.1f %%; "
                 "chain faults on this handle: %d" % (off, on, on / off, 100 * differ, e.lib.dimx_chain_faults(e.h)))
    e.set_cross_lookahead(None)
    e.close()


def run_bench(tree):
    r = subprocess.run([sys.executable] + BENCH, cwd=tree, capture_output=True, text=True, timeout=420)   # an error ends the tool
    if r.returncode != 0:
        raise RuntimeError("bench.py in %s ended with %d: %s" % (tree, r.returncode, r.stderr[-2000:]))
    for line in reversed(r.stdout.splitlines()):
        if line.startswith("{") and '"value"' in line:
            out = json.loads(line)
            return float(out["value"]), float(out["ms_per_step"])
    raise RuntimeError("no result line from bench.py in %s" % tree)


def default_path(lines, parent_tree, pairs):
    lines.append("2. the default path against the parent commit: %s, a fresh process per run, parent and tree alternating, %d pairs"
                 % (" ".join(BENCH[:7]), pairs))
    if not parent_tree:
        lines.append("   not measured (no --parent-tree)")
        return
    runs = {"parent": [], "tree": []}
    for i in range(pairs):
        for name, tree in (("parent", parent_tree), ("tree", ROOT)):
            v, ms = run_bench(tree)
            runs[name].append(v)
            lines.append("   pair %d  %-7s %9.2f clips/s  (%.2f ms per step)" % (i + 1, name, v, ms))
            print(lines[-1], flush=True)
    par, tre = runs["parent"], runs["tree"]
    spread = max(par) - min(par)
    mp, mt = statistics.median(par), statistics.median(tre)
    lines.append("   parent: median %.2f clips/s, spread of its %d runs (max - min) %.2f clips/s = %.2f %%" % (mp, len(par), spread, 100 * spread / mp))
    lines.append("   tree:   median %.2f clips/s; tree - parent = %+.2f clips/s (%+.2f %%): %s"
                 % (mt, mt - mp, 100 * (mt - mp) / mp, "inside the parent's spread" if mt >= mp - spread else "SLOWER than the parent by more than its spread"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "online_generate.txt"))
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--skip-window", action="store_true", help="measurement 2 alone")
    args = ap.parse_args()
    lines = ["Online generation (dimx_set_cross_lookahead): measurements of tools/bench_online.py", "=" * 84, ""]
    # measurement 2 first: its fresh processes then never share the GPU with this process's handle
    part2 = []
    default_path(part2, args.parent_tree, args.pairs)
    if not args.skip_window:
        window_on_off(lines)
        lines.append("")
    lines += part2
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
