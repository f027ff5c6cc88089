"""Time the DIM-Speaker mesh metrics (Lip Vertex Error, FDD) at the workload's shape on one MI355X and write
profiles/mesh_metrics.txt:

  1. the operator (dimx_op_mesh_metrics, csrc/mesh_metrics.hip), through dimx.engine.op_mesh_metrics;
  2. the same formulas written in torch float64 on the same GPU (what a user would write today);
  3. the host route: device-to-host copy of both meshes plus dimx.mymetrics.compute_biwi_metrics on the f32 arrays.

    python tools/bench_mesh_metrics.py [--frames 300] [--mesh-dim 70110] [--n-mouth 4996] [--iters 200] [--out profiles/mesh_metrics.txt]

Shape: B = 1, T = 300, V = 70110, n_mouth = 4996; n_upper is SYNTHETIC (the real regions/fdd.txt is not available), at two sizes,
4996 and 12000; both maps are random distinct vertices (the real maps are contiguous regions, so real gathers touch fewer lines).
Cold case: the timed calls rotate over enough (y_true, y_pred) pairs that their 168 MB per pair exceed the 256 MB Infinity Cache
several times over, so no mesh is read from a cache a previous iteration filled.  In the real pipeline the mesh head's GEMM has
just written the predicted mesh (84 MB, part of it may still sit in the Infinity Cache); the ground truth comes from the loader's
upload.  The cold figure is the conservative one.  Times are HIP events around the whole loop (warm-up first), divided by the
iterations.  "bytes touched" = the distinct 128-byte lines of both meshes and the template that the maps' vertices fall on,
counted per map (each map is read by its own kernel, so the sum can exceed one reading of both meshes: random maps of this density
hit nearly every line); the rate is those bytes over the time, against the 8 TB/s HBM peak.  No GPU, no numbers: the tool fails."""
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
from dimx import mymetrics  # noqa: E402

PEAK = 8.0e12
LINE = 128


def lines_touched(vmap, frames, row_floats):
    """distinct 128-byte lines the map's 12-byte vertices fall on, summed over the frames of one mesh (rows are row_floats * 4 bytes
    apart, so the phase of a vertex inside a line changes from frame to frame)"""
    v = np.unique(np.asarray(vmap, dtype=np.int64))
    total = 0
    for t in range(frames):
        lo = (t * row_floats + 3 * v) * 4
        total += np.unique(np.concatenate([lo // LINE, (lo + 11) // LINE])).size
    return total


def torch_f64(y_true, y_pred, templ, mouth_d, upper_d):
    """the reference's formulas in torch float64 on the device: -> (sum of frame maxima, sigma_gt, sigma_pred) of one clip"""
    T = y_true.shape[0]
    g = y_true.view(T, -1, 3)
    p = y_pred.view(T, -1, 3)
    d = (g[:, mouth_d].double() - p[:, mouth_d].double()).square().sum(-1)
    s_max = d.max(dim=1).values.sum()
    tu = templ.view(-1, 3)[upper_d].double()
    sg = (g[:, upper_d].double() - tu).square().sum(-1).std(dim=0, unbiased=False).mean()
    sp = (p[:, upper_d].double() - tu).square().sum(-1).std(dim=0, unbiased=False).mean()
    return s_max, sg, sp


def timed(fn, n_pairs, warmup, iters):
    for i in range(warmup):
        fn(i % n_pairs)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        fn(i % n_pairs)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters      # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--mesh-dim", type=int, default=70110)
    ap.add_argument("--n-mouth", type=int, default=4996)
    ap.add_argument("--n-upper", type=int, nargs="+", default=[4996, 12000])
    ap.add_argument("--pairs", type=int, default=8, help="(y_true, y_pred) pairs the timed calls rotate over")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_metrics.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_mesh_metrics needs the GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    T, V = args.frames, args.mesh_dim
    nv = V // 3
    g = torch.Generator().manual_seed(20261017)
    templ = (0.1 * torch.randn(1, V, generator=g)).to(dev)
    pairs = []
    for _ in range(args.pairs):
        yt = templ[:, None] + 0.01 * torch.randn(1, T, V, generator=g).to(dev)
        yp = templ[:, None] + 0.01 * torch.randn(1, T, V, generator=g).to(dev)
        pairs.append((yt, yp))
    mouth = torch.randperm(nv, generator=g)[:args.n_mouth].tolist()
    out = ["DIM-Speaker mesh metrics (LVE, FDD), MI355X, one GPU.",
           "", "== python tools/bench_mesh_metrics.py ==",
           "B = 1, T = %d, V = %d (Nv = %d), n_mouth = %d; n_upper SYNTHETIC (regions/fdd.txt is not available); both maps random distinct"
           % (T, V, nv, args.n_mouth),
           "vertices.  COLD case: the calls rotate over %d (y_true, y_pred) pairs = %.0f MB, against 256 MB of Infinity Cache." %
           (args.pairs, args.pairs * 2 * T * V * 4 / 1e6),
           "HIP events around %d calls after %d warm-up calls; host route: wall clock, %d runs.  Rates are bytes of the distinct 128-byte"
           % (args.iters, max(args.pairs, 10), args.host_iters),
           "lines touched over the time, and their share of the 8 TB/s HBM peak.", ""]
    for n_upper in args.n_upper:
        upper = torch.randperm(nv, generator=g)[:n_upper].tolist()
        mouth_d = torch.tensor(sorted(mouth), device=dev)
        upper_d = torch.tensor(sorted(upper), device=dev)
        touched = 2 * LINE * (lines_touched(mouth, T, V) + lines_touched(upper, T, V)) + LINE * lines_touched(upper, 1, V)
        res = {}

        mouth_m, upper_m = E.mesh_map(mouth, nv, dev), E.mesh_map(upper, nv, dev)      # validated and uploaded once, as BiwiMeshMetrics does

        def run_op(i):
            res["op"] = E.op_mesh_metrics(pairs[i][0], pairs[i][1], [T], templ, mouth_m, upper_m)[0]

        def run_torch(i):
            res["torch"] = torch_f64(pairs[i][0][0], pairs[i][1][0], templ[0], mouth_d, upper_d)

        t_op = timed(run_op, args.pairs, max(args.pairs, 10), args.iters)
        t_torch = timed(run_torch, args.pairs, max(args.pairs, 10), max(args.iters // 4, 10))
        # the two device paths must agree before their times are compared (last pair of the rotation on both sides)
        run_op(0)
        run_torch(0)
        torch.cuda.synchronize()
        c = res["op"][0].tolist()
        tt = [float(x) for x in res["torch"]]
        agree = max(abs(c[0] - tt[0]) / tt[0], abs(c[2] - tt[1]) / tt[1], abs(c[3] - tt[2]) / tt[2])
        host = []
        for i in range(args.host_iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            j = (args.host_iters - 1 - i) % args.pairs      # the last run is pair 0, the one the device paths ran last
            yt_h, yp_h, tm_h = pairs[j][0].cpu().numpy(), pairs[j][1].cpu().numpy(), templ.cpu().numpy()
            t1 = time.perf_counter()
            m = mymetrics.compute_biwi_metrics([yt_h[0]], [yp_h[0]], None, [tm_h[0]], mouth, upper)
            t2 = time.perf_counter()
            host.append(((t2 - t0) * 1e6, (t1 - t0) * 1e6))
        t_host, t_copy = sorted(host)[len(host) // 2]
        out += ["n_upper = %d: %.1f MB touched (%.1f%% of the %.0f MB of both meshes)" % (n_upper, touched / 1e6, 100.0 * touched / (2 * T * V * 4),
                                                                                     2 * T * V * 4 / 1e6),
                "  1. operator (3 launches, float64)      %10.1f us   %8.1f GB/s  = %5.2f%% of peak" % (t_op, touched / t_op / 1e3, 100 * touched / (t_op * 1e-6) / PEAK),
                "  2. torch float64 on the GPU             %10.1f us   %8.1f GB/s  = %5.2f%% of peak   (%.2f x the operator's time)"
                % (t_torch, touched / t_torch / 1e3, 100 * touched / (t_torch * 1e-6) / PEAK, t_torch / t_op),
                "  3. host route (D2H of both meshes + compute_biwi_metrics, f32)  %10.1f us of which the copy %.1f us   %8.3f GB/s = %.4f%% of peak"
                % (t_host, t_copy, touched / t_host / 1e3, 100 * touched / (t_host * 1e-6) / PEAK),
                "  operator vs torch float64 on the same clip: max relative difference of (sum max, sigma_gt, sigma_pred) %.2e;  host f32 lve %.6e, operator lve %.6e"
                % (agree, float(m["lve"]), c[0] / c[1]), ""]
    text = "\n".join(out)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
