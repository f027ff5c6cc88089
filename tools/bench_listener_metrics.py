"""Time the listener evaluation metrics (print_metrics + print_metrics_full without SID) at the test protocol's shape on one MI355X
and write profiles/listener_metrics.txt:

  1. the operator (dimx_op_listener_metrics, csrc/listener_metrics.hip), through dimx.engine.op_listener_metrics;
  2. the same outputs written in torch float64 on the same GPU (dimx.metrics.frechet_distances_torch per window, and every entry
     of the per-clip moment rows);
  3. the host route: dimx.mymetrics.compute_metrics(with_sid=False) + compute_metrics_full on the per-clip numpy lists.

    python tools/bench_listener_metrics.py [--clips 256] [--frames 299] [--repeats 5] [--host-clips 256] [--out profiles/listener_metrics.txt]

Inputs: seeded, yt = randn, yp = 0.6 yt + 0.5 randn, x = randn, every clip full length.  The two device forms are timed with HIP events
around one call each, interleaved (operator, torch, operator, ...), after a warm-up call of each; the median, the minimum and the
maximum of the repeats are reported.  WARM: every repeat runs on the same tensors (51 MB, they sit in the 256 MB Infinity Cache).
COLD: the repeats rotate over enough input sets to exceed the Infinity Cache.  The host route is one wall-clock run (it takes tens
of seconds and does not thread).  The two device forms must agree before their times are compared: the largest relative difference
of the per-clip distances and moments is printed.  The tool is one process: the caller runs it under a time limit
(timeout -k 10 300 python tools/bench_listener_metrics.py).  No GPU, no numbers: the tool fails."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dimx  # noqa: E402,F401
from dimx import engine as E  # noqa: E402
from dimx import metrics, mymetrics  # noqa: E402

WINDOWS = [w for _, w in E.LISTENER_WINDOWS]


def torch_f64(yt, yp, x, lens):
    """the operator's outputs written in torch float64 on the device, for full-length clips: -> (fd [B, 6], moments [B, 133] in the
    row layout of include/dimx.h)"""
    fds = []
    for xc0, xF, yc0, yF in WINDOWS:
        a = torch.cat([x[:, :, xc0:xc0 + xF], yt[:, :, yc0:yc0 + yF]], -1)
        c = torch.cat([x[:, :, xc0:xc0 + xF], yp[:, :, yc0:yc0 + yF]], -1)
        fds.append(metrics.frechet_distances_torch(a, c[:, None], lens)[:, 0])
    g, p, xs = yt[:, :, :56].double(), yp[:, :, :56].double(), x[:, :, :56].double()
    d = g - p
    cols = [torch.full((g.shape[0],), float(g.shape[1]), dtype=torch.float64, device=g.device)]
    for c0, c1 in ((0, 6), (6, 56)):
        G, P, X, D = g[:, :, c0:c1], p[:, :, c0:c1], xs[:, :, c0:c1], d[:, :, c0:c1]
        cg, cp, cx = (v - v.mean((1, 2), keepdim=True) for v in (G, P, X))
        cols += [(D * D).sum((1, 2)), G.mean((1, 2)), (cg * cg).sum((1, 2)), P.mean((1, 2)), (cp * cp).sum((1, 2)), X.mean((1, 2)),
                 (cx * cx).sum((1, 2)), (cg * cx).sum((1, 2)), (cp * cx).sum((1, 2)), ((D[:, 1:] - D[:, :-1]) ** 2).sum((1, 2))]
    return torch.stack(fds, 1), torch.cat([torch.stack(cols, 1), d[:, 0], d[:, -1]], 1)


def event_time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out      # ms


def stats(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--frames", type=int, default=299)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sets", type=int, default=8, help="input sets the cold repeats rotate over")
    ap.add_argument("--host-clips", type=int, default=256, help="clips of the host run (0 skips it)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "listener_metrics.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_listener_metrics needs the GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    B, T = args.clips, args.frames
    g = torch.Generator().manual_seed(20261018)
    sets = []
    for _ in range(args.sets):
        yt = torch.randn(B, T, 56, generator=g)
        yp = 0.6 * yt + 0.5 * torch.randn(B, T, 56, generator=g)
        x = torch.randn(B, T, 56, generator=g)
        sets.append((yt.to(dev), yp.to(dev), x.to(dev)))
    lens = [T] * B
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    set_mb = 3 * B * T * 56 * 4 / 1e6

    def run_op(i):
        return E.op_listener_metrics(sets[i][0], sets[i][1], sets[i][2], lens_d)

    def run_torch(i):
        return torch_f64(sets[i][0], sets[i][1], sets[i][2], lens)

    run_op(0), run_torch(0)                                   # warm-up: code objects, workspaces, solver set-up
    torch.cuda.synchronize()
    t = {"op warm": [], "torch warm": [], "op cold": [], "torch cold": []}
    for r in range(args.repeats):
        t["op warm"].append(event_time(lambda: run_op(0))[0])
        t["torch warm"].append(event_time(lambda: run_torch(0))[0])
    for r in range(args.repeats):                              # each form meets set i after the other sets went through the caches
        i = (r + 1) % args.sets
        t["op cold"].append(event_time(lambda: run_op(i))[0])
        t["torch cold"].append(event_time(lambda: run_torch((i + args.sets // 2) % args.sets))[0])
    fd_op, mom_op = run_op(0)
    fd_t, mom_t = run_torch(0)
    torch.cuda.synchronize()
    agree = float(((fd_op - fd_t).abs() / fd_t.abs()).max())
    agree_m = float(((mom_op - mom_t).abs() / mom_t.abs().clamp(min=1e-300)).max())
    sw_t, sw_c = E.listener_metrics_sweeps(dev, B, len(WINDOWS), 112)

    out = ["Listener evaluation metrics (print_metrics + print_metrics_full without SID), MI355X, one GPU.",
           "", "== python tools/bench_listener_metrics.py ==",
           "%d clips x %d frames x 56, seeded; six windows (F = 6, 50, 12, 100, 56, 112) and the per-clip moments, float64." % (B, T),
           "HIP events around one call, operator and torch form interleaved, one warm-up call each; median [min .. max] of %d repeats."
           % args.repeats,
           "WARM: the same %.0f MB of inputs every repeat.  COLD: the repeats rotate over %d input sets = %.0f MB (Infinity Cache 256 MB)."
           % (set_mb, args.sets, set_mb * args.sets), ""]
    for k, label in (("op", "1. operator (2 launches)        "), ("torch", "2. torch float64 on the GPU     ")):
        for c in ("warm", "cold"):
            m, lo, hi = stats(t["%s %s" % (k, c)])
            out.append("  %s %s %10.2f ms   [%.2f .. %.2f]" % (label, c, m, lo, hi))
    mo, mt = stats(t["op warm"])[0], stats(t["torch warm"])[0]
    out += ["  torch / operator (warm medians): %.2f x" % (mt / mo),
            "  the two device forms, largest relative difference of the %d x %d distances: %.2e, of the %d x 133 moments: %.2e"
            % (B, len(WINDOWS), agree, B, agree_m),
            "  Jacobi sweeps: target %d..%d, candidate %d..%d (bound 30)" % (int(sw_t.min()), int(sw_t.max()), int(sw_c.min()),
                                                                              int(sw_c.max()))]
    if args.host_clips > 0:
        n = min(args.host_clips, B)
        gl, pl, xl = ([a[j].cpu().numpy().astype(np.float64) for j in range(n)] for a in sets[0])
        t0 = time.perf_counter()
        m1 = mymetrics.compute_metrics(gl, pl, xl, with_sid=False)
        t1 = time.perf_counter()
        m2 = mymetrics.compute_metrics_full(gl, pl, xl)
        t2 = time.perf_counter()
        out.append("  3. host route, %d clips, one run (wall clock): compute_metrics(with_sid=False) %.2f s + compute_metrics_full %.2f s = %.2f s"
                   % (n, t1 - t0, t2 - t1, t2 - t0))
        if n == B:
            acc = metrics.ListenerMetrics().update(sets[0][0], sets[0][1], sets[0][2], lens_d).result()
            ref = dict(m1, **m2)
            worst = max(float(np.max(np.abs(np.asarray(acc[k]) - np.asarray(ref[k])) / np.abs(np.asarray(ref[k])))) for k in ref)
            out.append("  ListenerMetrics.result() against the host route, largest relative difference over its %d entries: %.2e" % (len(ref), worst))
    text = "\n".join(out)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
