"""Wall time of the reference's test-time protocol end to end (x_engine_pt.evaluate_test_epoch: best of 10 generations per clip by
Frechet distance) with the Frechet distances on the host (the reference's scipy arithmetic), in torch on the device and in the HIP
library (dimx_op_fd_select), followed by the selection stage alone for the two device backends.
    python tools/bench_eval.py [B=256] [T=300] [batches=3]"""
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
import dimx  # noqa
from dimx import engine as E
from dimx import lib as L
from dimx import prng, x_engine_pt
from dimx.seq2seq_pretrain import SLMFT

B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
T = int(sys.argv[2]) if len(sys.argv) > 2 else 300
NB = int(sys.argv[3]) if len(sys.argv) > 3 else 3
dev = torch.device("cuda:0")
torch.set_grad_enabled(False)
model = SLMFT(numeric_mode=L.MODE_PERF_BF16).to(dev).eval()
batches = []
for i in range(NB):
    src = torch.from_numpy(prng.normal(40 + i, "ev.src", (B, T, 824)))
    tgt = torch.from_numpy(prng.normal(40 + i, "ev.tgt", (B, T, 56)))
    batches.append((src, tgt, [T] * B, None, ["c%d_%d" % (i, j) for j in range(B)]))
for backend in ("device", "hip"):                                                                       # warm-up
    x_engine_pt.evaluate_test_epoch(model, batches[:1], dev, beam_size=10, seed=5, fd_backend=backend)
res = {}
for backend in ("reference", "device", "hip"):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    yt, yp, xs, ids = x_engine_pt.evaluate_test_epoch(model, batches, dev, beam_size=10, seed=5, fd_backend=backend)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    res[backend] = yp
    print("evaluate_test_epoch fd_backend=%-9s %d batches of %d clips x 10 tries: %6.2f s  (%.1f clips/s end to end)" % (
        backend, NB, B, dt, NB * B / dt), flush=True)
for backend in ("device", "hip"):
    same = sum(int(np.array_equal(a, b)) for a, b in zip(res["reference"], res[backend]))
    print("fd_backend=%-6s same winner as reference for %d of %d clips" % (backend, same, len(res["reference"])))

# ---- the selection stage alone: distances, winner and gather of one batch that already sits on the device (HIP events, the two
# backends interleaved, median of 5 after one warm-up each)
S, Ln, F = 10, T - 1, 56
g = torch.Generator().manual_seed(1)
y_true = torch.randn(B, Ln, F, generator=g).to(dev)
y_pred = (0.6 * y_true.cpu()[:, None] + 0.5 * torch.randn(B, S, Ln, F, generator=g)).to(dev)
lens = [Ln] * B
lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)


def stage_device():
    from dimx.metrics import frechet_distances_torch
    fd = frechet_distances_torch(y_true, y_pred, lens)
    fd = torch.where(torch.isnan(fd), torch.full_like(fd, float("inf")), fd)
    win = fd.argmin(dim=1)
    return win, y_pred[torch.arange(B, device=dev), win]


def stage_hip():
    _, win, _, best = E.op_fd_select(y_true, y_pred, lens_d)
    return win, best


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


stages = {"device": stage_device, "hip": stage_hip}
times = {k: [] for k in stages}
outs = {}
for rep in range(6):
    for k, fn in stages.items():
        ms, outs[k] = timed(fn)
        if rep:
            times[k].append(ms)
print("selection stage alone, B=%d S=%d L=%d F=%d (ms, median of 5 after one warm-up, interleaved; all runs listed):" % (B, S, Ln, F))
for k in stages:
    print("  fd_backend=%-6s median %9.3f ms   runs %s" % (k, float(np.median(times[k])), " ".join("%.3f" % t for t in times[k])))
print("  same winner for %d of %d clips" % (int((outs["device"][0].cpu() == outs["hip"][0].cpu().long()).sum()), B))
sw_t, sw_c = E.fd_select_sweeps(dev, B, S, F)
print("  Jacobi sweeps (bound 30): target factorisation min %d max %d, (clip, try) problems min %d max %d" % (
    int(sw_t.min()), int(sw_t.max()), int(sw_c.min()), int(sw_c.max())))
