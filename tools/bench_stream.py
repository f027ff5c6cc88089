"""Streaming sessions (dimx_stream_*): what a push costs, what a whole session costs against the whole-clip calls, and that the
default path did not move.
    python tools/bench_stream.py [--parent-tree PATH] [--out profiles/stream_session.txt] [--pairs 3] [--batches 1,16,256]

One MI355X.  Three measurements, in the order they run:

 1. The default path against the parent commit: ``bench.py --gpus 1 --steps 20 --warmup 5`` (the flagship leg alone) as a fresh
    process in a built checkout of the parent commit (--parent-tree) and in this tree, alternating, --pairs pairs.  No launch on
    that path changed; the spread is what the parent's own runs show.

 2. Per-push latency: one 300-frame session per (mode, B, c) after one warm-up session of the same shape, lookahead 0, greedy;
    device events recorded by the push itself (dimx_stream_set_events) at its start, after the encoder increment, after the cross
    K/V append and after the decode steps; the host waits for every push before the next one, as a live caller does.  Reported:
    the median over the session's pushes of the three parts and of the whole push, and the min .. max of the whole.  The order
    is f32 then bf16, B ascending, c = 1 then 8; every configuration runs once, so the spread given is the spread over the pushes
    of one session, not over repeats of the session.

 3. Whole session against the whole-clip calls: the sum of the pushes of (2) with c = 1 and c = 8 against
    ``encode_ctx + generate(lookahead=0)`` on the 300-frame clip at the same B -- of the parent commit when --parent-tree is given
    (a fresh process in that tree), else of this tree -- device-event time, median of 5 calls after 2 warm-up calls.  The session
    loses in total; the ratio is what the per-frame latency costs.

``--kv8 --self-kv8`` (profiles/stream_kv8.txt) measures the FP8 routes of a session (dimx_stream_set_kv8) instead of 2 and
3: (1) as above; per-push medians as in (2) for bf16 and f32 with FP8 off, FP8 cross K/V and FP8 cross + self K/V -- one warm-up session
per variant, then the variants' timed sessions alternating, two rounds, all in this process and build; and one long session at
B = 256, Tmax = 2048, c = 8 in bf16 with FP8 off and with both on, the push time near the start, the middle and the end.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 300
BENCH = ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5", "--no-cpu-baseline", "--no-roofline", "--no-mode-compare",
         "--no-parity-mode", "--no-train-step", "--no-shard-check", "--no-best-of-n"]

# runs in a tree of its own (cwd): encode_ctx + generate(lookahead=0) per call, one JSON line {"mode B": [median, min, max]}
WHOLE = r'''
import json, statistics, sys, torch
sys.path.insert(0, ".")
import dimx
from dimx import engine, lib as L, prng, weights
torch.set_grad_enabled(False)
T = %d
sd = weights.synth_state_dict(weights.slmft_spec(), 20260928)
out = {}
for mode in ("f32", "bf16"):
    e = engine.Engine("cuda:0", L.MODE_PARITY_F32 if mode == "f32" else L.MODE_PERF_BF16)
    e.load_state_dict(sd)
    for B in %r:
        v_s = torch.from_numpy(prng.normal(3, "bs.vs", (B, T, 56))).cuda()
        v_a = torch.from_numpy(prng.normal(3, "bs.va", (B, T, 768))).cuda()
        start = torch.from_numpy(prng.integers(3, "bs.z", (B,), 0, 512)).to(torch.int32).cuda()
        m8 = torch.ones(B, T, dtype=torch.uint8).cuda()
        ts = []
        for i in range(7):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            e.encode_ctx(v_s, v_a, m8, True)
            e.generate(start, m8, T, 0.0, 52, None, 0, lookahead=0)
            e1.record()
            torch.cuda.synchronize()
            if i >= 2:
                ts.append(e0.elapsed_time(e1))
        out["%%s %%d" %% (mode, B)] = [statistics.median(ts), min(ts), max(ts)]
    e.close()
print("WHOLE " + json.dumps(out))
'''


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
    lines.append("1. the default path against the parent commit: %s, a fresh process per run, parent and tree alternating, %d pairs"
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


def whole_clip(tree, batches):
    r = subprocess.run([sys.executable, "-c", WHOLE % (T, list(batches))], cwd=tree, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError("the whole-clip run in %s ended with %d: %s" % (tree, r.returncode, r.stderr[-2000:]))
    for line in r.stdout.splitlines():
        if line.startswith("WHOLE "):
            return json.loads(line[6:])
    raise RuntimeError("no result line from the whole-clip run in %s" % tree)


def sessions(lines, batches):
    import torch
    sys.path.insert(0, ROOT)
    import dimx  # noqa: F401
    from dimx import engine, lib as L, prng, weights

    torch.set_grad_enabled(False)
    sd = weights.synth_state_dict(weights.slmft_spec(), 20260928)
    lines.append("2. per-push latency: a %d-frame session after one warm-up session, lookahead 0, greedy, ms; median over the session's "
                 "pushes (whole push: min .. max)" % T)
    lines.append("   %-5s %4s %2s   %9s %9s %9s   %9s %20s   %10s" % ("mode", "B", "c", "encoder", "K/V", "steps", "push", "", "session"))
    totals = {}
    for mode in ("f32", "bf16"):
        e = engine.Engine("cuda:0", L.MODE_PARITY_F32 if mode == "f32" else L.MODE_PERF_BF16)
        e.load_state_dict(sd)
        for B in batches:
            v_s = torch.from_numpy(prng.normal(3, "bs.vs", (B, T, 56))).cuda()
            v_a = torch.from_numpy(prng.normal(3, "bs.va", (B, T, 768))).cuda()
            start = torch.from_numpy(prng.integers(3, "bs.z", (B,), 0, 512)).to(torch.int32).cuda()
            for c in (1, 8):
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
                for x in ev:
                    x.record()
                parts = []
                s = e.stream(B, T, start, lookahead=0, temperature=0.0)
                for timed in (False, True):
                    if timed:
                        s.begin(start, 0.0)
                        s.set_events(ev)
                    for n in range(0, T, c):
                        s.push(v_s[:, n:n + c], v_a[:, n:n + c])
                        torch.cuda.synchronize()
                        if timed:
                            parts.append([ev[i].elapsed_time(ev[i + 1]) for i in range(3)] + [ev[0].elapsed_time(ev[3])])
                    s.end()
                    torch.cuda.synchronize()
                med = [statistics.median(p[i] for p in parts) for i in range(4)]
                whole = [p[3] for p in parts]
                totals[(mode, B, c)] = sum(whole)
                lines.append("   %-5s %4d %2d   %9.3f %9.3f %9.3f   %9.3f (%7.3f .. %7.3f)   %10.1f"
                             % (mode, B, c, med[0], med[1], med[2], med[3], min(whole), max(whole), sum(whole)))
                print(lines[-1], flush=True)
                del s
        e.close()
    return totals


def _timed_session(torch, s, start, v_s, v_a, frames, c, ev, warm):
    """one session of `frames` frames in pushes of c; -> per push [encoder, append, steps, push] ms (None for a warm-up session)"""
    parts = []
    s.begin(start, 0.0)
    if not warm:
        s.set_events(ev)
    for n in range(0, frames, c):
        s.push(v_s[:, n:n + c], v_a[:, n:n + c])
        torch.cuda.synchronize()
        if not warm:
            parts.append([ev[i].elapsed_time(ev[i + 1]) for i in range(3)] + [ev[0].elapsed_time(ev[3])])
    s.end()
    torch.cuda.synchronize()
    return None if warm else parts


def fp8_sessions(lines, batches, variants, long_session):
    """Measurements of the FP8 routes (dimx_stream_set_kv8): per-push medians of the variants in one process and one build, the
    variants' timed sessions alternating; then one long session at B = 256, Tmax = 2048, c = 8 in bf16."""
    import torch
    sys.path.insert(0, ROOT)
    import dimx  # noqa: F401
    from dimx import engine, lib as L, prng, weights

    torch.set_grad_enabled(False)
    sd = weights.synth_state_dict(weights.slmft_spec(), 20260928)
    names = [n for n, _ in variants]
    ROUNDS = 2
    lines.append("2. per-push latency with FP8 K/V: a %d-frame session per variant after one warm-up session each, lookahead 0, greedy, ms;" % T)
    lines.append("   the variants' timed sessions alternate (%s), %d rounds; median over the pushes of a variant's %d sessions"
                 % (" -> ".join(names), ROUNDS, ROUNDS))
    lines.append("   (whole push: min .. max).  append = the cross K/V projection of the new rows plus, with FP8 cross K/V, their quantisation.")
    lines.append("   %-5s %4s %2s  %-6s  %9s %9s %9s   %9s %20s   %9s" % ("mode", "B", "c", "fp8", "encoder", "append", "steps", "push", "", "vs off"))
    for mode in ("bf16", "f32"):
        e = engine.Engine("cuda:0", L.MODE_PARITY_F32 if mode == "f32" else L.MODE_PERF_BF16)
        e.load_state_dict(sd)
        for B in batches:
            v_s = torch.from_numpy(prng.normal(3, "bs.vs", (B, T, 56))).cuda()
            v_a = torch.from_numpy(prng.normal(3, "bs.va", (B, T, 768))).cuda()
            start = torch.from_numpy(prng.integers(3, "bs.z", (B,), 0, 512)).to(torch.int32).cuda()
            for c in (1, 8):
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
                for x in ev:
                    x.record()
                sess = {}
                for name, (kv8, skv8) in variants:
                    sess[name] = e.stream(B, T, start, lookahead=0, temperature=0.0, kv8=kv8, self_kv8=skv8)
                    sess[name].close()
                    _timed_session(torch, sess[name], start, v_s, v_a, T, c, ev, True)
                parts = {n: [] for n in names}
                for _ in range(ROUNDS):
                    for name in names:
                        parts[name] += _timed_session(torch, sess[name], start, v_s, v_a, T, c, ev, False)
                base = None
                for name in names:
                    p = parts[name]
                    med = [statistics.median(x[i] for x in p) for i in range(4)]
                    whole = [x[3] for x in p]
                    base = med[3] if base is None else base
                    lines.append("   %-5s %4d %2d  %-6s  %9.3f %9.3f %9.3f   %9.3f (%7.3f .. %7.3f)   %+8.1f %%"
                                 % (mode, B, c, name, med[0], med[1], med[2], med[3], min(whole), max(whole), 100 * (med[3] - base) / base))
                    print(lines[-1], flush=True)
                del sess
        e.close()
    if not long_session:
        return
    B, Tmax, c = 256, 2048, 8
    lines.append("")
    lines.append("3. one long session: bf16, B = %d, Tmax = %d frames pushed %d at a time, lookahead 0, greedy, after one warm-up session of 256 frames;"
                 % (B, Tmax, c))
    lines.append("   whole-push ms, median over the pushes whose first frame lies in the range given (every push runs %d steps)" % c)
    e = engine.Engine("cuda:0", L.MODE_PERF_BF16)
    e.load_state_dict(sd)
    CH = 256
    v_s = torch.from_numpy(prng.normal(3, "bs.vs", (B, CH, 56))).cuda()       # the same 256 frames again and again: the cost does not depend on them
    v_a = torch.from_numpy(prng.normal(3, "bs.va", (B, CH, 768))).cuda()
    start = torch.from_numpy(prng.integers(3, "bs.z", (B,), 0, 512)).to(torch.int32).cuda()
    ranges = [(8, 136), (960, 1088), (1912, 2040)]
    first = None
    for name, (kv8, skv8) in (variants[0], variants[-1]):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        for x in ev:
            x.record()
        s = e.stream(B, Tmax, start, lookahead=0, temperature=0.0, kv8=kv8, self_kv8=skv8)
        s.close()
        _timed_session(torch, s, start, v_s, v_a, CH, c, ev, True)
        s.begin(start, 0.0)
        s.set_events(ev)
        rows = []
        for n in range(0, Tmax, c):
            o = n % CH
            s.push(v_s[:, o:o + c], v_a[:, o:o + c])
            torch.cuda.synchronize()
            rows.append((n, [ev[i].elapsed_time(ev[i + 1]) for i in range(3)] + [ev[0].elapsed_time(ev[3])]))
        s.end()
        torch.cuda.synchronize()
        meds = []
        for lo, hi in ranges:
            sel = [p for n, p in rows if lo <= n < hi]
            meds.append([statistics.median(x[i] for x in sel) for i in range(4)])
        first = meds if first is None else first
        lines.append("   fp8 %-6s %s   session %9.1f ms" % (name, "   ".join("frames %4d..%4d: push %7.3f (append %6.3f, steps %7.3f)" % (lo, hi, m[3], m[1], m[2])
                                                                      for (lo, hi), m in zip(ranges, meds)), sum(p[3] for _, p in rows)))
        if first is not meds:
            lines.append("   %s against %s: %s" % (name, variants[0][0], ", ".join("frames %d..%d %+.1f %%" % (lo, hi, 100 * (m[3] - f[3]) / f[3])
                                                                                 for (lo, hi), m, f in zip(ranges, meds, first))))
        print("\n".join(lines[-2:]), flush=True)
        del s
    e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--out", default=None, help="default: profiles/stream_session.txt, profiles/stream_kv8.txt with --kv8 / --self-kv8")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--batches", default="1,16,256")
    ap.add_argument("--skip-default-path", action="store_true", help="measurements 2 and 3 alone")
    ap.add_argument("--kv8", action="store_true", help="the FP8 measurements (dimx_stream_set_kv8): FP8 off against FP8 cross K/V ...")
    ap.add_argument("--self-kv8", action="store_true", help="... and against FP8 cross and self K/V (alone: FP8 off against FP8 self K/V)")
    ap.add_argument("--no-long-session", action="store_true", help="with --kv8 / --self-kv8: without the B = 256, Tmax = 2048 session")
    args = ap.parse_args()
    batches = [int(b) for b in args.batches.split(",")]
    if args.kv8 or args.self_kv8:
        out = args.out or os.path.join(ROOT, "profiles", "stream_kv8.txt")
        variants = [("off", (False, False))]
        if args.kv8:
            variants.append(("cross", (True, False)))
        if args.self_kv8:
            variants.append(("both", (True, True)) if args.kv8 else ("self", (False, True)))
        lines = ["Streaming sessions with FP8 K/V (dimx_stream_set_kv8): measurements of tools/bench_stream.py --kv8 --self-kv8", "=" * 110, ""]
        if not args.skip_default_path:
            default_path(lines, args.parent_tree, args.pairs)
            lines.append("")
        fp8_sessions(lines, batches, variants, not args.no_long_session)
        text = "\n".join(lines) + "\n"
        print(text)
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as fh:
            fh.write(text)
        return
    args.out = args.out or os.path.join(ROOT, "profiles", "stream_session.txt")
    lines = ["Streaming sessions (dimx_stream_*): measurements of tools/bench_stream.py", "=" * 84, ""]
    # the fresh processes first: they then never share the GPU with this process's handles
    if not args.skip_default_path:
        default_path(lines, args.parent_tree, args.pairs)
        lines.append("")
    ref_tree = args.parent_tree or ROOT
    ref = whole_clip(ref_tree, batches)
    totals = sessions(lines, batches)
    lines.append("")
    lines.append("3. whole session against encode_ctx + generate(lookahead=0) of %s on the %d-frame clip (median of 5 calls after 2 "
                 "warm-up calls, min .. max), ms" % ("the parent commit" if args.parent_tree else "this tree", T))
    for mode in ("f32", "bf16"):
        for B in batches:
            w = ref["%s %d" % (mode, B)]
            lines.append("   %-5s %4d   whole clip %9.1f (%.1f .. %.1f)   session c=1 %9.1f = %5.2f x, %.3f ms per frame   session c=8 %9.1f = %5.2f x"
                         % (mode, B, w[0], w[1], w[2], totals[(mode, B, 1)], totals[(mode, B, 1)] / w[0], totals[(mode, B, 1)] / T,
                            totals[(mode, B, 8)], totals[(mode, B, 8)] / w[0]))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
