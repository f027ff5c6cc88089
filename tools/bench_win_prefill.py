"""The windowed prefill: what the many-query windowed cross attention costs, where a windowed prompt prefill beats the
forced decode steps, what one-pass scoring saves, what a session begun from a prompt costs, and that the default path did not move.
    python tools/bench_win_prefill.py [--parent-tree PATH] [--out profiles/win_prefill.txt] [--pairs 3] [--only kernel,generate,...]

One MI355X.  Every section runs as a fresh process of this file (``--section NAME``), after a warm-up of every timed shape, on
device events; a figure is the median of 5 calls with their min .. max.  Sections, in the order they run:

 default   ``bench.py --gpus 1 --steps 20 --warmup 5`` (the flagship leg alone) in a built checkout of the parent commit
           (--parent-tree) and in this tree, alternating, --pairs pairs.  No launch on that path changed.
 forced    generate(prompt of 150 codes, lookahead=0) through forced decode steps at 256 x 300 in the parent tree and in this tree:
           the path the new flag leaves alone.
 kernel    dimx_op_cross_attn_win alone: 256 clips x 12 heads, Lq = 299, n_keys = 300, lookahead 0 and 300 (every key), f32 and bf16.
 generate  generate(prompt, lookahead=0) at 256 x 300, P in {2, 17, 150, 270}: prefill="window" against forced steps.
 score     the online teacher-forced logits at 256 x 300: encode_ctx + decode_tf(lookahead=0) against encode_ctx + the forced-step
           generation SLMFT.score(lookahead=0) runs.
 session   begin(prompt of 150 codes, 150 frames) at B in {1, 16, 256}, Tmax = 300, against the same begin with a one-code prompt (the
           encoder increments and the K / V append alone: the difference is the prefill), against begin + 150 single-frame pushes and
           against begin + one 150-frame push.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, T, REPS, WARM = 256, 300, 5, 2
SECTIONS = ["default", "forced", "kernel", "generate", "score", "session"]
BENCH = ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5", "--no-cpu-baseline", "--no-roofline", "--no-mode-compare",
         "--no-parity-mode", "--no-train-step", "--no-shard-check", "--no-best-of-n"]

# runs in a tree of its own (cwd), the parent's too: a prompt of 150 codes through forced decode steps under lookahead 0
FORCED = r'''
import json, statistics, sys, torch
sys.path.insert(0, ".")
import dimx
from dimx import engine, lib as L, prng, weights
torch.set_grad_enabled(False)
B, T, P = %d, %d, 150
sd = weights.synth_state_dict(weights.slmft_spec(), 20260928)
out = {}
for mode in ("f32", "bf16"):
    e = engine.Engine("cuda:0", L.MODE_PARITY_F32 if mode == "f32" else L.MODE_PERF_BF16)
    e.load_state_dict(sd)
    v_s = torch.from_numpy(prng.normal(3, "bw.vs", (B, T, 56))).cuda()
    v_a = torch.from_numpy(prng.normal(3, "bw.va", (B, T, 768))).cuda()
    z = torch.from_numpy(prng.integers(3, "bw.z", (B, T), 0, 512)).to(torch.int32).cuda()
    m8 = torch.ones(B, T, dtype=torch.uint8).cuda()
    e.encode_ctx(v_s, v_a, m8, True)
    ts = []
    for i in range(7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        e.generate(None, m8, T, 0.0, 52, None, 0, prompt=z[:, :P].contiguous(), lookahead=0)
        e1.record()
        torch.cuda.synchronize()
        if i >= 2:
            ts.append(e0.elapsed_time(e1))
    out[mode] = [statistics.median(ts), min(ts), max(ts)]
    e.close()
print("FORCED " + json.dumps(out))
'''


def timed(fn, reps=REPS, warm=WARM):
    import torch
    ts = []
    for i in range(warm + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if i >= warm:
            ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts), max(ts)


def fmt(t):
    return "%9.3f (%8.3f .. %8.3f)" % t


def _setup():
    import torch
    sys.path.insert(0, ROOT)
    import dimx  # noqa: F401
    from dimx import engine, lib as L, prng, weights
    torch.set_grad_enabled(False)
    sd = weights.synth_state_dict(weights.slmft_spec(), 20260928)

    def eng(mode):
        e = engine.Engine("cuda:0", L.MODE_PARITY_F32 if mode == "f32" else L.MODE_PERF_BF16)
        e.load_state_dict(sd)
        return e

    def clip(b, t=T):
        v_s = torch.from_numpy(prng.normal(3, "bw.vs", (b, t, 56))).cuda()
        v_a = torch.from_numpy(prng.normal(3, "bw.va", (b, t, 768))).cuda()
        z = torch.from_numpy(prng.integers(3, "bw.z", (b, t), 0, 512)).to(torch.int32).cuda()
        return v_s, v_a, z, torch.ones(b, t, dtype=torch.uint8).cuda()

    return torch, engine, eng, clip


def section_kernel(lines):
    torch, engine, _, _ = _setup()
    H, Lq, n_keys, Tp = 12, T - 1, T, 304
    lines.append("kernel: dimx_op_cross_attn_win alone, %d clips x %d heads, Lq = %d, n_keys = %d, us per launch" % (B, H, Lq, n_keys))
    lines.append("   (the offline prefill attention attn_tr_kernel<64,2> takes 183 us per launch for this shape, every key visible: VERDICT round 6)")
    g = torch.Generator().manual_seed(5)
    q = torch.randn(B, Lq, H * 64, generator=g).cuda()
    for dt, name in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
        k = torch.randn(B, H, Tp, 64, generator=g).to(dt).cuda()
        v = torch.randn(B, H, Tp, 64, generator=g).to(dt).cuda()
        out = torch.empty(B, Lq, H * 64, dtype=dt, device="cuda")
        for la in (0, T):
            t = timed(lambda: engine.op_cross_attn_win(q, k, v, la, 0.125, n_keys=n_keys, out=out))
            lines.append("   %-5s lookahead %3d   %s" % (name, la, fmt(tuple(1e3 * x for x in t))))
            print(lines[-1], flush=True)


def section_generate(lines):
    torch, _, eng, clip = _setup()
    lines.append("generate: generate(prompt of P codes, lookahead=0) at %d x %d, greedy, ms per call" % (B, T))
    lines.append("   %-5s %4s   %-32s %-32s %s" % ("mode", "P", "prefill='window'", "forced steps (no flag)", "window / forced"))
    v_s, v_a, z, m8 = clip(B)
    for mode in ("f32", "bf16"):
        e = eng(mode)
        e.encode_ctx(v_s, v_a, m8, True, prompt_frames=270)
        for P in (2, 17, 150, 270):
            prompt = z[:, :P].contiguous()
            w = timed(lambda: e.generate(None, m8, T, 0.0, 52, None, 0, prompt=prompt, prefill=("window", P), lookahead=0))
            f = timed(lambda: e.generate(None, m8, T, 0.0, 52, None, 0, prompt=prompt, prefill=P, lookahead=0))
            lines.append("   %-5s %4d   %s   %s   %.3f" % (mode, P, fmt(w), fmt(f), w[0] / f[0]))
            print(lines[-1], flush=True)
        e.close()


def section_score(lines):
    torch, _, eng, clip = _setup()
    lines.append("score: the teacher-forced logits under lookahead 0 at %d x %d, encode_ctx included, ms per call" % (B, T))
    lines.append("   %-5s   %-32s %-32s %s" % ("mode", "one pass (decode_tf_win)", "forced steps", "one pass / forced"))
    v_s, v_a, z, m8 = clip(B)
    prompt = z[:, :T - 1].contiguous()
    for mode in ("f32", "bf16"):
        e = eng(mode)

        def one():
            e.encode_ctx(v_s, v_a, m8, True)
            e.decode_tf(z, m8, None, lookahead=0)

        def steps():
            e.encode_ctx(v_s, v_a, m8, True)
            e.generate(None, m8, T, 0.0, 52, None, 0, return_logits=True, prompt=prompt, prefill=1, no_prefill=True, lookahead=0)

        a, b = timed(one), timed(steps)
        lines.append("   %-5s   %s   %s   %.3f" % (mode, fmt(a), fmt(b), a[0] / b[0]))
        print(lines[-1], flush=True)
        e.close()


def section_session(lines):
    torch, _, eng, clip = _setup()
    F = 150
    lines.append("session: reaching the state \"%d frames in, %d codes known\" of a session with Tmax = %d, lookahead 0, ms" % (F, F, T))
    lines.append("   %-5s %4s   %-32s %-32s %-32s %s" % ("mode", "B", "begin(prompt, P = 150)", "begin(prompt, P = 1): no prefill",
                                                      "begin + 150 pushes of 1 frame", "begin + 1 push of 150 frames"))
    for mode in ("f32", "bf16"):
        e = eng(mode)
        for b in (1, 16, 256):
            v_s, v_a, z, _ = clip(b, F)
            start = z[:, 0].contiguous()
            s = e.stream(b, T, start, lookahead=0, temperature=0.0)
            s.close()

            def prompted(P):
                s.begin(None, 0.0, prompt=z[:, :P].contiguous(), v_speaker=v_s, v_audio=v_a)
                s.close()

            def pushes(c):
                s.begin(start, 0.0)
                for n in range(0, F, c):
                    s.push(v_s[:, n:n + c], v_a[:, n:n + c])
                s.close()

            r = [timed(lambda: prompted(F), warm=1), timed(lambda: prompted(1), warm=1), timed(lambda: pushes(1), warm=1),
                 timed(lambda: pushes(F), warm=1)]
            lines.append("   %-5s %4d   %s   %s   %s   %s" % (mode, b, fmt(r[0]), fmt(r[1]), fmt(r[2]), fmt(r[3])))
            print(lines[-1], flush=True)
            del s
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


def section_default(lines, parent_tree, pairs):
    lines.append("default: %s, a fresh process per run, parent and tree alternating, %d pairs" % (" ".join(BENCH[:7]), pairs))
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
                 % (mt, mt - mp, 100 * (mt - mp) / mp, "inside the parent's spread" if abs(mt - mp) <= spread else "OUTSIDE the parent's spread"))


def section_forced(lines, parent_tree):
    lines.append("forced: generate(prompt of 150 codes, lookahead=0) without the new flag at %d x %d, ms per call" % (B, T))
    for name, tree in (("parent", parent_tree), ("tree", ROOT)):
        if not tree:
            lines.append("   %-7s not measured (no --parent-tree)" % name)
            continue
        r = subprocess.run([sys.executable, "-c", FORCED % (B, T)], cwd=tree, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise RuntimeError("the forced-step run in %s ended with %d: %s" % (tree, r.returncode, r.stderr[-2000:]))
        out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("FORCED ")][-1][7:])
        lines.append("   %-7s f32 %s   bf16 %s" % (name, fmt(tuple(out["f32"])), fmt(tuple(out["bf16"]))))
        print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "win_prefill.txt"))
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--only", default=",".join(SECTIONS), help="comma-separated sections to run")
    ap.add_argument("--section", default=None, help="(internal) run one section in this process and print its lines as JSON")
    args = ap.parse_args()
    if args.section:
        lines = []
        {"kernel": section_kernel, "generate": section_generate, "score": section_score, "session": section_session}[args.section](lines)
        print("LINES " + json.dumps(lines))
        return
    lines = ["The windowed prefill (DESIGN 26): measurements of tools/bench_win_prefill.py; median of %d calls (min .. max)" % REPS, "=" * 110, ""]
    for name in [s for s in SECTIONS if s in args.only.split(",")]:
        if name == "default":
            section_default(lines, args.parent_tree, args.pairs)
        elif name == "forced":
            section_forced(lines, args.parent_tree)
        else:     # a fresh process per section
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--section", name], cwd=ROOT, capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                raise RuntimeError("section %s ended with %d: %s" % (name, r.returncode, r.stderr[-2000:]))
            lines += json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("LINES ")][-1][6:])
        lines.append("")
        print("section %s done" % name, flush=True)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
