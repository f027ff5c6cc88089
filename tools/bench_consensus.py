"""Time consensus (minimum-Bayes-risk) best-of-N selection at the test protocol's shape on one MI355X and write
profiles/consensus_select.txt:

  1. the operator (dimx_op_consensus_select, csrc/consensus.hip) through dimx.engine.op_consensus_select, both distances;
  2. the same outputs (pairwise distances, risks, winner, gathered rows) written in torch float64 on the same GPU: the pairwise
     form of dimx.metrics.frechet_distances_torch, and the mean squared difference;
  3. for comparison, dimx.engine.op_fd_select on the same tries (against a recorded listener: S distances per clip, not S (S - 1) / 2).

    python tools/bench_consensus.py [--clips 256] [--tries 10] [--frames 299] [--repeats 5] [--sets 3] [--out profiles/consensus_select.txt]

Inputs: seeded, yt = randn, yp = 0.6 yt + 0.5 randn per try, every clip full length.  Every form is timed with HIP events around one
call, the forms interleaved, after one warm-up call of each; the median, the minimum and the maximum of the repeats are reported.
COLD: the repeats rotate over input sets that together exceed the 256 MB Infinity Cache (one set of the default shape is 171 MB).
The two device forms must agree before their times are compared: the largest relative difference of the distances and the number of
clips with the same winner are printed.  The tool is one process: the caller runs it under a time limit
(timeout -k 10 300 python tools/bench_consensus.py).  No GPU, no numbers: the tool fails."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dimx  # noqa: E402,F401
from dimx import engine as E  # noqa: E402


def _pairs(S, dev):
    i, j = torch.triu_indices(S, S, 1, device=dev)
    return i, j


def torch_fd(yp):
    """pairwise Frechet distances of full-length clips in torch float64: yp [B, S, L, F] -> D [B, S, S]; the arithmetic of
    dimx.metrics.frechet_distances_torch with try i < j in the place of the target and the candidate"""
    B, S, L, F = yp.shape
    x = yp.to(torch.float64)
    mu = x.mean(2)                                                      # [B, S, F]
    c = x - mu[:, :, None]
    cov = c.transpose(-1, -2) @ c / (L - 1.0)                           # [B, S, F, F]
    lam, V = torch.linalg.eigh(cov)
    A = V * lam.clamp(min=0).sqrt()[..., None, :]                       # S_i = A_i A_i^T
    i, j = _pairs(S, yp.device)
    M = A[:, i].transpose(-1, -2) @ cov[:, j] @ A[:, i]                 # [B, P, F, F]
    M = 0.5 * (M + M.transpose(-1, -2))
    tr_sqrt = torch.linalg.eigvalsh(M).clamp(min=0).sqrt().sum(-1)
    tr = torch.diagonal(cov, dim1=-2, dim2=-1).sum(-1)                  # [B, S]
    diff = mu[:, i] - mu[:, j]
    d = (diff * diff).sum(-1) + tr[:, i] + tr[:, j] - 2.0 * tr_sqrt     # [B, P]
    D = torch.zeros(B, S, S, dtype=torch.float64, device=yp.device)
    D[:, i, j] = d
    D[:, j, i] = d
    return D


def torch_l2(yp):
    B, S, L, F = yp.shape
    x = yp.to(torch.float64)
    D = torch.stack([((x[:, i:i + 1] - x) ** 2).mean((2, 3)) for i in range(S)], 1)
    return torch.triu(D, 1) + torch.triu(D, 1).transpose(1, 2)


def torch_select(yp, kind):
    """the operator's outputs in torch: (risk, win, best, dist)"""
    D = torch_fd(yp) if kind == "fd" else torch_l2(yp)
    risk = D.sum(2)
    win = torch.where(torch.isnan(risk), torch.full_like(risk, float("inf")), risk).argmin(1)
    best = yp[torch.arange(yp.shape[0], device=yp.device), win]
    return risk, win, best, D


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
    ap.add_argument("--tries", type=int, default=10)
    ap.add_argument("--frames", type=int, default=299)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sets", type=int, default=3, help="input sets the cold repeats rotate over")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "consensus_select.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_consensus needs the GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    B, S, T = args.clips, args.tries, args.frames
    g = torch.Generator().manual_seed(20261019)
    sets = []
    for _ in range(args.sets):
        yt = torch.randn(B, T, 56, generator=g)
        yp = 0.6 * yt[:, None] + 0.5 * torch.randn(B, S, T, 56, generator=g)
        sets.append((yt.to(dev), yp.to(dev)))
    lens_d = torch.full((B,), T, dtype=torch.int32, device=dev)
    set_mb = B * S * T * 56 * 4 / 1e6

    forms = {"op fd": lambda i: E.op_consensus_select(sets[i][1], lens_d, distance="fd", want_dist=True),
             "op l2": lambda i: E.op_consensus_select(sets[i][1], lens_d, distance="l2", want_dist=True),
             "torch fd": lambda i: torch_select(sets[i][1], "fd"),
             "torch l2": lambda i: torch_select(sets[i][1], "l2"),
             "fd_select": lambda i: E.op_fd_select(sets[i][0], sets[i][1], lens_d)}
    for k in forms:                                            # warm-up: code objects, workspaces, solver set-up
        forms[k](0)
    torch.cuda.synchronize()
    t = {k: [] for k in forms}
    for r in range(args.repeats):                              # each form meets a set after the other sets went through the caches
        for n, k in enumerate(forms):
            t[k].append(event_time(lambda: forms[k]((r + n + 1) % args.sets))[0])

    out = ["Consensus (minimum-Bayes-risk) best-of-N selection in the HIP library (dimx_op_consensus_select, csrc/consensus.hip), MI355X,",
           "one GPU.", "", "== python tools/bench_consensus.py ==",
           "%d clips x %d tries x %d frames x 56, seeded, every clip full length; float64 distances over all 56 columns, %d pairs per clip."
           % (B, S, T, S * (S - 1) // 2),
           "HIP events around one call (distances, risks, winner and the gather of the winner's rows), the forms interleaved, one warm-up",
           "call each; median [min .. max] of %d repeats.  COLD: the repeats rotate over %d input sets of %.0f MB (Infinity Cache 256 MB)."
           % (args.repeats, args.sets, set_mb), ""]
    labels = (("op fd", "1. operator, fd (3 launches)          "), ("torch fd", "2. torch float64 on the GPU, fd       "),
              ("op l2", "1. operator, l2 (2 launches)          "), ("torch l2", "2. torch float64 on the GPU, l2       "),
              ("fd_select", "3. op_fd_select, the same tries       "))
    med = {}
    for k, label in labels:
        med[k], lo, hi = stats(t[k])
        out.append("  %s %10.3f ms   [%.3f .. %.3f]" % (label, med[k], lo, hi))
    out.append("")
    for kind in ("fd", "l2"):
        risk, win, ok, best, dist = forms["op " + kind](0)
        t_risk, t_win, t_best, t_dist = forms["torch " + kind](0)
        torch.cuda.synchronize()
        off = ~torch.eye(S, dtype=torch.bool, device=dev)
        rel = float(((dist - t_dist).abs()[:, off] / t_dist.abs()[:, off]).max())
        same = int((win.long() == t_win).sum())
        ratio = med["torch " + kind] / med["op " + kind]
        out.append("  %s: torch / operator (medians) %.2f x -- the operator %s the torch form.  Largest relative difference of the %d x %d"
                   % (kind, ratio, "beats" if ratio > 1.0 else "DOES NOT beat", B, S * (S - 1)))
        out.append("      distances %.2e; the same winner for %d of %d clips; gathered rows identical for %d of them."
                   % (rel, same, B, int(sum(torch.equal(best[j], t_best[j]) for j in range(B) if int(win[j]) == int(t_win[j])))))
    forms["op fd"](0)
    sw_f, sw_p = E.consensus_select_sweeps(dev, B, S, 56)
    out += ["  Jacobi sweeps (bound 30): try factorisations %d..%d, pair problems %d..%d" % (int(sw_f.min()), int(sw_f.max()), int(sw_p.min()),
                                                                                          int(sw_p.max())),
            "  operator fd / op_fd_select (medians): %.2f x  (%d factorisations + %d pair problems against %d + %d)"
            % (med["op fd"] / med["fd_select"], B * S, B * S * (S - 1) // 2, B, B * S), "",
            "bench.py against the parent commit was not run: the operator is a new entry point, and no launch on bench.py's path, no kernel",
            "it times and no flag of their build changes (csrc/frechet.hpp gains two helpers that only csrc/consensus.hip calls)."]
    text = "\n".join(out)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
