"""Online fine-tuning (dimx_set_train_lookahead): what the window does to the time of a training step, and that the window-off
step did not move.
    python tools/bench_online_train.py [--parent-tree PATH] [--out profiles/online_train.txt] [--pairs 3]

One MI355X, the shape bench.py --full times the SLMFT training step at: 16 clips x 300 frames (4 800 rows: launched kernel by
kernel, weight gradients on the side stream), AdamW lr 1e-5, clip 1.0, no mask_prob draw, listener codes precomputed.  One step =
HipTrainer.train_step (forward, backward, clip, AdamW) between two device events.

 1. Window on (lookahead 0) against window off on this tree, bf16 and f32: blocks in the order off / on / off / on, each block 2
    warm-up steps and 5 timed ones, median per block.  At lookahead 0 the decoder's cross attention (4 of the step's 12 attention
    sublayers) does roughly half its tile work; whether the step gets measurably faster is reported, not assumed.

 2. The window-off step against the parent commit (--parent-tree: a checkout of the parent with its library built): this file's
    --one mode -- the median of 5 bf16 steps after 2 warm-ups -- as a fresh process per run, parent and tree alternating,
    --pairs pairs.  The tree's median has to lie inside the spread (min .. max) of the parent's own runs; if it does not the
    difference is reported.  --one uses nothing the parent lacks.
"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, T, REPS, WARM = 16, 300, 5, 2


def _setup(root, bf16):
    import torch
    sys.path.insert(0, root)
    import dimx  # noqa: F401
    from dimx import lib as L, prng
    from dimx.seq2seq_pretrain import SLMFT
    from dimx.train_hip import HipTrainer
    dev = torch.device("cuda:0")
    m = SLMFT(numeric_mode=L.MODE_PERF_BF16 if bf16 else L.MODE_PARITY_F32).to(dev)
    tr = HipTrainer(m, lr=1e-5, clip=1.0)
    v_s = torch.from_numpy(prng.normal(7, "bt.vs", (B, T, 56))).to(dev)
    v_l = torch.from_numpy(prng.normal(7, "bt.vl", (B, T, 56))).to(dev)
    v_a = torch.from_numpy(prng.normal(7, "bt.va", (B, T, 768))).to(dev)
    mask = torch.ones(B, T, dtype=torch.bool, device=dev)
    with torch.no_grad():
        _, z = m.forward_vq(v_s, v_l, mask, with_speaker=False)
    return torch, tr, (v_s, v_l, v_a, mask), z


def _block(torch, tr, args, z):
    for _ in range(WARM):
        tr.train_step(*args, kv_mask=False, z_l=z)
    torch.cuda.synchronize()
    out = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        loss = tr.train_step(*args, kv_mask=False, z_l=z)
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    assert bool(torch.isfinite(loss))
    return out


def one(root):
    """--one: the window-off bf16 step of the tree at ``root``, median ms on the last line"""
    torch, tr, args, z = _setup(root, True)
    t = _block(torch, tr, args, z)
    print("%.4f" % statistics.median(t))


def window_on_off(lines):
    lines.append("1. window on (lookahead 0) against window off: HipTrainer.train_step, one MI355X, B = %d, T = %d; device-event time per "
                 "step, median of %d after %d warm-up steps (min .. max), blocks in the order run" % (B, T, REPS, WARM))
    for bf16 in (True, False):
        torch, tr, args, z = _setup(ROOT, bf16)
        meds = {None: [], 0: []}
        for la in (None, 0, None, 0):
            tr.set_lookahead(la)
            t = _block(torch, tr, args, z)
            meds[la].append(statistics.median(t))
            lines.append("   %-4s %-22s %8.3f ms (%.3f .. %.3f)" % ("bf16" if bf16 else "f32", "window off" if la is None else "window on, lookahead 0",
                                                                  statistics.median(t), min(t), max(t)))
            print(lines[-1], flush=True)
        off, on = statistics.mean(meds[None]), statistics.mean(meds[0])
        lines.append("   %-4s mean of the block medians: off %.3f ms, on %.3f ms: on / off = %.3f; spread between the two off blocks %.3f ms"
                     % ("bf16" if bf16 else "f32", off, on, on / off, abs(meds[None][0] - meds[None][1])))
        del tr
        torch.cuda.empty_cache()


def run_one(tree):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", "--root", tree], cwd=tree, capture_output=True, text=True,
                       timeout=300)   # an error ends the tool
    if r.returncode != 0:
        raise RuntimeError("--one in %s ended with %d: %s" % (tree, r.returncode, r.stderr[-2000:]))
    return float(r.stdout.strip().splitlines()[-1])


def against_parent(lines, parent_tree, pairs):
    lines.append("2. the window-off step against the parent commit: bf16, B = %d, T = %d, median of %d steps after %d warm-ups, a fresh "
                 "process per run, parent and tree alternating, %d pairs" % (B, T, REPS, WARM, pairs))
    if not parent_tree:
        lines.append("   not measured (no --parent-tree)")
        return
    runs = {"parent": [], "tree": []}
    for i in range(pairs):
        for name, tree in (("parent", parent_tree), ("tree", ROOT)):
            runs[name].append(run_one(tree))
            lines.append("   pair %d  %-7s %8.3f ms per step" % (i + 1, name, runs[name][-1]))
            print(lines[-1], flush=True)
    par, tre = runs["parent"], runs["tree"]
    mp, mt = statistics.median(par), statistics.median(tre)
    lines.append("   parent: median %.3f ms, its %d runs span %.3f .. %.3f ms" % (mp, len(par), min(par), max(par)))
    lines.append("   tree:   median %.3f ms; tree - parent = %+.3f ms (%+.2f %%): %s"
                 % (mt, mt - mp, 100 * (mt - mp) / mp, "inside the spread of the parent's own runs" if min(par) <= mt <= max(par)
                    else ("FASTER than every run of the parent" if mt < min(par) else "SLOWER than every run of the parent")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "online_train.txt"))
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--skip-window", action="store_true", help="measurement 2 alone")
    ap.add_argument("--one", action="store_true", help="print the window-off bf16 step's median ms of the tree at --root")
    ap.add_argument("--root", default=ROOT)
    args = ap.parse_args()
    if args.one:
        return one(os.path.abspath(args.root))
    lines = ["Online fine-tuning (dimx_set_train_lookahead): measurements of tools/bench_online_train.py", "=" * 92, ""]
    # measurement 2 first: its fresh processes then never share the GPU with this process's handles
    part2 = []
    against_parent(part2, os.path.abspath(args.parent_tree) if args.parent_tree else None, args.pairs)
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
