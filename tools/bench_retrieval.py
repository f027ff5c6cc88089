"""Time the retrieval baselines (NN audio / NN motion: pooling, cosine k-nearest-neighbour search, gather) on one MI355X and write
profiles/retrieval.txt:

  1. the operators (dimx_op_pool_desc / dimx_op_nn_search / dimx_op_nn_gather, csrc/retrieval.hip) through dimx.engine;
  2. the same outputs written in torch float64 on the same GPU: amax / sum over time and a norm; one float64 matmul, the outer
     product of the norms, the eligibility mask and ``topk``; an index gather and a length mask;
  3. the host numpy route of the definition (dimx.retrieval), on a subset of the clips and queries, scaled linearly to the full shape
     (the subset sizes are printed).

    python tools/bench_retrieval.py [--queries 1024] [--library 4096 16384] [--frames 64] [--repeats 5] [--out profiles/retrieval.txt]

Shapes: Q test clips against N training clips of 64 frames (the LM-Listener window), D = 768 with max pooling (NN audio) and D = 56
with mean pooling (NN motion), K = 1 and 16, listener rows of 56 columns.  Every clip has the full length, so the torch form needs
no frame mask.  Every form is timed with HIP events around one call, the forms interleaved, after one warm-up call of each; the
median, the minimum and the maximum of the repeats are reported.  COLD: a 1 GiB buffer is overwritten before every timed call, four
times the 256 MB Infinity Cache.  The two device forms must agree before their times are compared: the largest difference of the
similarities and the number of queries with the same list are printed.  No ratio is promised: rocBLAS's float64 GEMM may well win on
raw time; the operator's case is the torch-free C-ABI, the fixed summation order and the exact ties.  The tool is one process: the
caller runs it under a time limit (timeout -k 10 600 python tools/bench_retrieval.py).  No GPU, no numbers: the tool fails."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dimx  # noqa: E402,F401
from dimx import engine as E  # noqa: E402
from dimx import retrieval  # noqa: E402


def torch_pool(x, kind):
    desc = x.amax(1).double() if kind == "max" else x.double().sum(1) / x.shape[1]
    return desc, desc.pow(2).sum(1).sqrt()


def torch_search(qd, qn, xd, xn, k):
    sim = (qd @ xd.t()) / (qn[:, None] * xn[None, :])
    ok = sim > -1.0                                                    # False for NaN too
    val, idx = torch.where(ok, sim, torch.full_like(sim, float("-inf"))).topk(min(k, sim.shape[1]), dim=1)
    hit = val > float("-inf")
    return torch.where(hit, idx, torch.full_like(idx, -1)).int(), torch.where(hit, val, torch.full_like(val, float("nan"))), hit.sum(1).int()


def torch_gather(lib_seq, lib_lens, idx, q_lens):
    i = idx.long().clamp(min=0)
    n = torch.minimum(q_lens[:, None], lib_lens[i]) * (idx >= 0)
    out = lib_seq[i] * (torch.arange(lib_seq.shape[1], device=idx.device)[None, None, :] < n[..., None])[..., None]
    return out, n.int()


class Timer:
    def __init__(self, dev, repeats):
        self.flush = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
        self.repeats = repeats

    def run(self, forms):
        """forms: name -> callable; interleaved, cold; -> name -> (median, min, max) in ms"""
        for f in forms.values():
            f()
        torch.cuda.synchronize()
        times = {k: [] for k in forms}
        for _ in range(self.repeats):
            for k, f in forms.items():
                self.flush.fill_(1)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                f()
                b.record()
                torch.cuda.synchronize()
                times[k].append(a.elapsed_time(b))
        return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--library", type=int, nargs="+", default=[4096, 16384])
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-clips", type=int, default=128, help="clips of the host pooling subset")
    ap.add_argument("--host-queries", type=int, default=16, help="queries of the host search subset")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retrieval.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_retrieval needs a GPU"
    dev = torch.device("cuda:0")
    Q, T, W = args.queries, args.frames, 56
    timer = Timer(dev, args.repeats)
    lines = ["retrieval baselines on %s: Q = %d queries, %d frames per clip, median (min .. max) of %d cold runs, ms"
             % (torch.cuda.get_device_name(0), Q, T, args.repeats)]

    def fmt(t):
        return "%9.3f (%8.3f .. %8.3f)" % t

    for D, kind in ((768, "max"), (56, "mean")):
        for N in args.library:
            g = torch.Generator(device=dev).manual_seed(1000 + N + D)
            x = torch.randn(N, T, D, generator=g, device=dev)
            qx = torch.randn(Q, T, D, generator=g, device=dev)
            lib_seq = torch.randn(N, T, W, generator=g, device=dev)
            lens, q_lens = torch.full((N,), T, dtype=torch.int32, device=dev), torch.full((Q,), T, dtype=torch.int32, device=dev)
            lines.append("")
            lines.append("D = %d (%s pooling), N = %d training clips" % (D, kind, N))
            r = timer.run({"hip": lambda: E.op_pool_desc(x, lens, kind), "torch": lambda: torch_pool(x, kind)})
            (xd, xn), (txd, txn) = E.op_pool_desc(x, lens, kind), torch_pool(x, kind)
            qd, qn = E.op_pool_desc(qx, q_lens, kind)
            lines.append("  pool library    hip %s   torch f64 %s   largest |difference| of a descriptor %.2e"
                         % (fmt(r["hip"]), fmt(r["torch"]), float((xd - txd).abs().max())))
            t0 = time.perf_counter()
            nh = min(args.host_clips, N)
            hd, _ = retrieval.pool_batch(x[:nh].cpu().numpy(), [T] * nh, kind)
            host_pool = (time.perf_counter() - t0) * 1e3 * N / nh
            lines.append("                  host numpy (definition) %.0f ms, scaled from %d clips (readback included)" % (host_pool, nh))
            for K in (1, 16):
                r = timer.run({"hip": lambda: E.op_nn_search(qd, qn, xd, xn, K), "torch": lambda: torch_search(qd, qn, xd, xn, K)})
                (idx, sim, found), (tidx, tsim, _) = E.op_nn_search(qd, qn, xd, xn, K), torch_search(qd, qn, xd, xn, K)
                same = int((idx == tidx).all(1).sum())
                lines.append("  search K = %-2d   hip %s   torch f64 %s   same list for %d of %d queries, largest |difference| of a similarity %.2e"
                             % (K, fmt(r["hip"]), fmt(r["torch"]), same, Q, float((sim - tsim).abs().max())))
                rg = timer.run({"hip": lambda: E.op_nn_gather(lib_seq, lens, idx, q_lens), "torch": lambda: torch_gather(lib_seq, lens, idx, q_lens)})
                eq = bool(torch.equal(E.op_nn_gather(lib_seq, lens, idx, q_lens)[0], torch_gather(lib_seq, lens, idx, q_lens)[0]))
                lines.append("  gather K = %-2d   hip %s   torch     %s   equal outputs: %s" % (K, fmt(rg["hip"]), fmt(rg["torch"]), eq))
            t0 = time.perf_counter()
            qh = min(args.host_queries, Q)
            xd_h = xd.cpu().numpy()
            hs = retrieval.similarities(qd[:qh].cpu().numpy(), xd_h)
            retrieval.top_k(hs, 16)
            host_search = (time.perf_counter() - t0) * 1e3 * Q / qh
            lines.append("  search K = 16   host numpy (definition) %.0f ms, scaled from %d queries (readback included)" % (host_search, qh))
            del x, qx, lib_seq
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
