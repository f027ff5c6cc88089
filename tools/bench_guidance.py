"""Classifier-free guidance (dimx_generate_guided, sample_guided_kernel, dimx_set_train_cond_keep): what guidance costs, and that
the paths without it did not move.
    python tools/bench_guidance.py [--parent-tree PATH] [--out profiles/guided_generate.txt] [--pairs 3]

One MI355X.  Four measurements:

 1. Guided generation against plain generation on this tree: 256 clips x 300 frames, seed 5, top-k 52, bf16 and f32; device-event
    time per call, median of 5 after 2 warm-up calls.  Three lines per mode: the plain generation on its default route (bf16: the
    chain / layer kernels), the plain generation forced onto the one-kernel-per-op route the guided step takes (DIMX_NO_CHAIN=1
    when the handle is made; the f32 mode has no other route), and the guided generation at scale 1.5.  The unconditional half
    should cost the projections, self attention and feed-forward of a step, not a second cross K/V stream: guided / per-op well
    below 2.
 2. The guided sampler launch alone against the plain one: R = 256 rows, normal logits x 3, temperature 1, the device generator;
    tools/bench_sampler.py's method (a graph of 500 launches, median of 9 replays).
 3. ``bench.py --gpus 1 --steps 20 --warmup 5`` (the flagship leg alone) against the parent commit: fresh processes in a built
    checkout of the parent (--parent-tree) and in this tree, alternating, --pairs pairs.
 4. One SLMFT training step with the condition dropout off, 16 clips x 300 frames, bf16, against the parent commit the same way;
    and on this tree with a keep vector set (the two extra launches).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
B, T, REPS, WARM = 256, 300, 5, 2
BENCH = ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5", "--no-cpu-baseline", "--no-roofline", "--no-mode-compare",
         "--no-parity-mode", "--no-train-step", "--no-shard-check", "--no-best-of-n"]
TRAIN_STEP = r"""
import statistics, sys, torch
sys.path.insert(0, ".")
import dimx
from dimx import lib as L, prng, train_hip
from dimx.seq2seq_pretrain import SLMFT
B, T = 16, 300
model = SLMFT(numeric_mode=L.MODE_PERF_BF16).cuda()
tr = train_hip.HipTrainer(model)
g = lambda n, s: torch.from_numpy(prng.normal(5, "bg." + n, s)).cuda()
v_s, v_l, v_a = g("vs", (B, T, 56)), g("vl", (B, T, 56)), g("va", (B, T, 768))
mask = torch.ones(B, T, dtype=torch.bool).cuda()
z = torch.from_numpy(prng.integers(5, "bg.z", (B, T), 0, 512)).cuda()
keep = KEEP
kw = dict(kv_mask=False, z_l=z)
if keep is not None:
    kw["cond_keep"] = torch.tensor(keep, dtype=torch.uint8)
for _ in range(3):
    tr.forward_backward(v_s, v_l, v_a, mask, **kw)
torch.cuda.synchronize()
out = []
for _ in range(9):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); tr.forward_backward(v_s, v_l, v_a, mask, **kw); e1.record()
    torch.cuda.synchronize()
    out.append(e0.elapsed_time(e1))
print("STEP_MS %.4f" % statistics.median(out))
"""


def timed(call):
    import torch
    for _ in range(WARM):
        call()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out), min(out), max(out)


def generation(lines):
    import torch
    import dimx  # noqa: F401
    from dimx import engine, lib as L, prng, weights

    torch.set_grad_enabled(False)
    sd = weights.synth_state_dict(weights.slmft_spec(), 20260928)
    v_s = torch.from_numpy(prng.normal(3, "bo.vs", (B, T, 56))).cuda()
    v_a = torch.from_numpy(prng.normal(3, "bo.va", (B, T, 768))).cuda()
    start = torch.from_numpy(prng.integers(3, "bo.z", (B,), 0, 512)).to(torch.int32).cuda()
    m8 = torch.ones(B, T, dtype=torch.uint8).cuda()
    lines.append("1. guided against plain generation: one MI355X, B = %d, T = %d, seed 5, top-k 52, scale 1.5; device-event time per call, "
                 "median of %d after %d warm-up calls (min .. max)" % (B, T, REPS, WARM))
    for mode_name, mode in (("bf16", L.MODE_PERF_BF16), ("f32", L.MODE_PARITY_F32)):
        res = {}
        for what, no_chain, guided in (("plain, default route", False, False), ("plain, per-op route", True, False), ("guided, scale 1.5", True, True)):
            if mode_name == "f32" and what == "plain, per-op route":
                res[what] = res["plain, default route"]      # the f32 mode has no chain kernels: one route
                continue
            if no_chain:
                os.environ["DIMX_NO_CHAIN"] = "1"
            else:
                os.environ.pop("DIMX_NO_CHAIN", None)
            e = engine.Engine("cuda:0", mode)
            e.load_state_dict(sd)
            e.encode_ctx(v_s, v_a, m8, True, guided=guided)
            res[what] = timed(lambda: e.generate(start, m8, T, 1.0, 52, None, 5, guidance=1.5 if guided else None))
            faults = e.lib.dimx_chain_faults(e.h)
            e.close()
            lines.append("   %-5s %-22s %8.2f ms (%.2f .. %.2f)%s" % ((mode_name, what) + res[what] + ("  chain faults: %d" % faults if faults else "",)))
            print(lines[-1], flush=True)
        os.environ.pop("DIMX_NO_CHAIN", None)
        lines.append("   %-5s guided / plain per-op = %.3f, guided / plain default = %.3f" % (
            mode_name, res["guided, scale 1.5"][0] / res["plain, per-op route"][0], res["guided, scale 1.5"][0] / res["plain, default route"][0]))
        print(lines[-1], flush=True)


def sampler(lines):
    import torch
    import dimx  # noqa: F401
    from dimx import lib as L, prng
    import bench_sampler

    lib = L.load()
    R = 256
    lg = (torch.from_numpy(prng.normal(7, "bench.sampler.%d.%d" % (R, 3), (R, 512))) * 3).cuda()
    un = (torch.from_numpy(prng.normal(7, "bench.guided.u.%d" % R, (R, 512))) * 3).cuda()
    tok = torch.empty(2 * R, dtype=torch.int32).cuda()
    g = torch.empty(R, 512).cuda()
    lines.append("2. one sampler launch, R = %d, normal logits x 3, temperature 1, device generator (us; median of %d replays of a graph of %d "
                 "launches, min .. max)" % (R, bench_sampler.REPS, bench_sampler.LAUNCHES))
    rows = [("dimx_op_sample, top-k 52", lambda s: L.check(lib.dimx_op_sample(L.ptr(lg), R, 52, 1.0, None, 5, 0, L.ptr(tok), s))),
            ("dimx_op_sample_guided, scale 1.5, no dump", lambda s: L.check(lib.dimx_op_sample_guided(
                L.ptr(lg), L.ptr(un), R, 1, R * 512, 1.5, 0, 52, 0.0, 0.0, 1.0, None, 5, 0, L.ptr(tok), None, s))),
            ("dimx_op_sample_guided, scale 1.5, guided dump", lambda s: L.check(lib.dimx_op_sample_guided(
                L.ptr(lg), L.ptr(un), R, 1, R * 512, 1.5, 0, 52, 0.0, 0.0, 1.0, None, 5, 0, L.ptr(tok), L.ptr(g), s)))]
    for name, fn in rows:
        lines.append("   %-48s %7.2f us (%.2f .. %.2f)" % ((name,) + bench_sampler.per_launch_us(fn)))
        print(lines[-1], flush=True)


def run_bench(tree):
    r = subprocess.run([sys.executable] + BENCH, cwd=tree, capture_output=True, text=True, timeout=420)   # an error ends the tool
    if r.returncode != 0:
        raise RuntimeError("bench.py in %s ended with %d: %s" % (tree, r.returncode, r.stderr[-2000:]))
    for line in reversed(r.stdout.splitlines()):
        if line.startswith("{") and '"value"' in line:
            out = json.loads(line)
            return float(out["value"])
    raise RuntimeError("no result line from bench.py in %s" % tree)


def run_train_step(tree, keep=None):
    r = subprocess.run([sys.executable, "-c", TRAIN_STEP.replace("KEEP", repr(keep))], cwd=tree, capture_output=True, text=True, timeout=420)
    if r.returncode != 0:
        raise RuntimeError("the training step in %s ended with %d: %s" % (tree, r.returncode, r.stderr[-2000:]))
    for line in reversed(r.stdout.splitlines()):
        if line.startswith("STEP_MS"):
            return float(line.split()[1])
    raise RuntimeError("no result line from the training step in %s" % tree)


def against_parent(lines, parent_tree, pairs):
    for title, run, unit, better in (("3. %s against the parent commit" % " ".join(BENCH[:7]), run_bench, "clips/s", 1),
                                     ("4. one SLMFT training step, 16 clips x 300 frames, bf16, condition dropout off (median of 9 steps after 3) against "
                                      "the parent commit", run_train_step, "ms", -1)):
        lines.append(title + ": a fresh process per run, parent and tree alternating, %d pairs" % pairs)
        if not parent_tree:
            lines.append("   not measured (no --parent-tree)")
            continue
        runs = {"parent": [], "tree": []}
        for i in range(pairs):
            for name, tree in (("parent", parent_tree), ("tree", ROOT)):
                runs[name].append(run(tree))
                lines.append("   pair %d  %-7s %9.3f %s" % (i + 1, name, runs[name][-1], unit))
                print(lines[-1], flush=True)
        par, tre = runs["parent"], runs["tree"]
        spread = max(par) - min(par)
        mp, mt = statistics.median(par), statistics.median(tre)
        inside = (mt - mp) * better >= -spread
        lines.append("   parent: median %.3f %s, spread of its %d runs (max - min) %.3f = %.2f %%" % (mp, unit, len(par), spread, 100 * spread / mp))
        lines.append("   tree:   median %.3f %s; tree - parent = %+.3f (%+.2f %%): %s"
                     % (mt, unit, mt - mp, 100 * (mt - mp) / mp, "inside the parent's spread" if inside else "WORSE than the parent by more than its spread"))
        lines.append("")
    ones = run_train_step(ROOT, keep=[1] * 16)
    mixed = run_train_step(ROOT, keep=[1, 0] * 8)
    lines.append("   this tree with a keep vector set: all ones %.3f ms, every second clip dropped %.3f ms" % (ones, mixed))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guided_generate.txt"))
    ap.add_argument("--pairs", type=int, default=3)
    args = ap.parse_args()
    lines = ["Classifier-free guidance: measurements of tools/bench_guidance.py", "=" * 84, ""]
    # the fresh processes first: they then never share the GPU with this process's handles
    tail = []
    against_parent(tail, args.parent_tree, args.pairs)
    generation(lines)
    lines.append("")
    sampler(lines)
    lines.append("")
    lines += tail
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
