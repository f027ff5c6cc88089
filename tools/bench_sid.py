"""Time the SID diversity metric (calcuate_sid, reference code/metrics/eval_utils.py:51-83) at the test protocol's shape on one MI355X
and write profiles/sid.txt:

  1. the operator route per group (pose: k = 20 on columns 0:6, exp: k = 40 on columns 6:56): one fit on the ground-truth frames and
     two assignments (dimx.metrics.sid_device: dimx_op_kmeans_fit + 2 x dimx_op_sid_assign, csrc/kmeans_sid.hip), with the draws and
     their upload included;
  2. the host route on the same machine: the four calcuate_sid calls print_metrics makes (scikit-learn KMeans on the float32 lists
     the reference hands it), one wall-clock run;
  3. the agreement of the two (pred, gt) pairs -- with scikit-learn on the float32 lists (the reference's own arithmetic) and on
     float64 copies (the operator's definition).

    python tools/bench_sid.py [--clips 256] [--frames 299] [--repeats 5] [--out profiles/sid.txt]

Inputs: seeded, gt = randn, pred = 0.6 gt + 0.5 randn, every clip full length.  HIP events around one call after a warm-up call;
median, minimum and maximum of the repeats.  The tool is one process: the caller runs it under a time limit
(timeout -k 10 300 python tools/bench_sid.py).  No GPU, no numbers: the tool fails."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dimx  # noqa: E402,F401
from dimx import metrics, mymetrics  # noqa: E402


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
    ap.add_argument("--no-host", action="store_true", help="skip the host route")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sid.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_sid needs the GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    B, T = args.clips, args.frames
    g = torch.Generator().manual_seed(20261018)
    yt = torch.randn(B, T, 56, generator=g)
    yp = 0.6 * yt + 0.5 * torch.randn(B, T, 56, generator=g)
    G, P = yt.reshape(B * T, 56).to(dev), yp.reshape(B * T, 56).to(dev)

    out = ["SID (calcuate_sid: KMeans fit on the ground truth, histogram entropy of the assignments), MI355X, one GPU.",
           "", "== python tools/bench_sid.py ==",
           "%d clips x %d frames = %d frames x 56, seeded; pose: k = 20, columns 0:6; exp: k = 40, columns 6:56; float64." % (B, T, B * T),
           "Operator route = one fit + two assignments per group, enqueued as a whole (max_iter = 300, launches after convergence return at",
           "once); HIP events around one call after a warm-up call; median [min .. max] of %d repeats." % args.repeats, ""]
    dev_vals, total = {}, 0.0
    for t in ("pose", "exp"):
        metrics.sid_device(G, P, t)
        torch.cuda.synchronize()
        times = []
        for _ in range(args.repeats):
            ms, r = event_time(lambda: metrics.sid_device(G, P, t))
            times.append(ms)
        sid_p, sid_g, n_iter, status = r.tolist()
        dev_vals[t] = (sid_p, sid_g)
        m, lo, hi = stats(times)
        total += m
        out.append("  1. operator, %-4s fit + 2 assigns %9.2f ms   [%.2f .. %.2f]   %d Lloyd iterations, status %d"
                   % (t, m, lo, hi, int(n_iter), int(status)))
    out.append("     both groups (medians): %.2f ms" % total)
    if not args.no_host:
        gl = [a.numpy() for a in yt]
        pl = [a.numpy() for a in yp]
        try:
            import sklearn
            t0 = time.perf_counter()
            host = {t: (mymetrics.calcuate_sid(gl, pl, t), mymetrics.calcuate_sid(gl, gl, t)) for t in ("pose", "exp")}
            dt = time.perf_counter() - t0
            out.append("  2. host route, the four calcuate_sid calls of print_metrics (scikit-learn %s, float32 lists), one run (wall clock): %.2f s"
                       % (sklearn.__version__, dt))
            out.append("     host / operator: %.0f x" % (dt * 1e3 / total))
            g64, p64 = [a.astype(np.float64) for a in gl], [a.astype(np.float64) for a in pl]
            host64 = {t: (mymetrics.calcuate_sid(g64, p64, t), mymetrics.calcuate_sid(g64, g64, t)) for t in ("pose", "exp")}
            for t in ("pose", "exp"):
                out.append("  3. sid_%-4s operator %.12g %.12g | scikit-learn f32 %.12g %.12g (largest difference %.2e) | scikit-learn on "
                           "float64 copies %.12g %.12g (largest difference %.2e)"
                           % ((t,) + dev_vals[t] + host[t] + (max(abs(a - b) for a, b in zip(dev_vals[t], host[t])),) + host64[t]
                              + (max(abs(a - b) for a, b in zip(dev_vals[t], host64[t])),)))
        except ImportError:
            t0 = time.perf_counter()
            host = {t: mymetrics.sid_f64(gl, pl, t) for t in ("pose", "exp")}
            dt = time.perf_counter() - t0
            out.append("  2. scikit-learn is not installed here: the numpy restatement (mymetrics.sid_f64, one fit per group) took %.2f s" % dt)
            for t in ("pose", "exp"):
                out.append("  3. sid_%-4s operator %.12g %.12g | restatement %.12g %.12g (largest difference %.2e)"
                           % ((t,) + dev_vals[t] + host[t] + (max(abs(a - b) for a, b in zip(dev_vals[t], host[t])),)))
    text = "\n".join(out)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
