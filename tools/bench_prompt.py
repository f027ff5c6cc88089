"""Prompted generation: prefill of the decode K/V cache against forced decode steps, device-event time per call.
    python tools/bench_prompt.py [--parent-lib PATH] [--out profiles/prompt_prefill.txt] [--modes bf16,f32] [--P 1,2,30,150,270]

One MI355X, B = 256, T = 300.  Per numeric mode and prompt length P (Pmax = P0 = P, no prompt_len), after a warm-up,
median of 5 calls with the range:
  (a) dimx_generate_prompted with the prefill, (b) with flags bit 0 (the whole prompt through forced decode steps),
  (c) the prefill stage alone (flags bit 2, a hook for this tool outside the documented flag set).
For P = 1 also dimx_generate of this tree and -- with --parent-lib, a libdimx_hip.so built from the parent commit -- of the
parent: two handles of each build, all four with the same workspace size, created and called in interleaved order (tree, parent,
parent, tree), 10 timed calls per handle.  Two handles of the same code show what a handle (its allocations, its graphs) is
worth: the spread the file states is, per build, max - min over its 20 samples on both handles (the larger of the two builds'),
and the two builds' medians must lie within it."""
import argparse
import ctypes
import statistics
import sys

import torch

sys.path.insert(0, ".")
import dimx  # noqa: F401,E402
from dimx import engine, lib as L, prng, weights  # noqa: E402

B, T, REPS, WARM = 256, 300, 5, 2


def load_other(path):
    lib = ctypes.CDLL(path)
    for name, (res, args) in L.SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
    return lib


def make_engine(mode, sd, other_lib=None):
    e = engine.Engine("cuda:0", mode)
    if other_lib is not None:
        # a handle of the other build: destroy the one the constructor made, create one there
        e.close()
        e.lib = other_lib
        h = ctypes.c_void_p()
        rc = other_lib.dimx_create(ctypes.byref(h), e.device.index, ctypes.byref(e.dims), mode)
        assert rc == 0, "dimx_create on the parent library failed (%d)" % rc
        e.h = h
    e.load_state_dict(sd)
    return e


def timed(fn, reps=REPS, warm=WARM):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def fmt(v):
    return "%8.2f ms (%.2f .. %.2f)" % (statistics.median(v), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default="profiles/prompt_prefill.txt")
    ap.add_argument("--modes", default="bf16,f32")
    ap.add_argument("--P", default="1,2,30,150,270")
    args = ap.parse_args()
    torch.set_grad_enabled(False)
    sd = weights.synth_state_dict(weights.slmft_spec(), 20260928)
    v_s = torch.from_numpy(prng.normal(3, "bp.vs", (B, T, 56))).cuda()
    v_a = torch.from_numpy(prng.normal(3, "bp.va", (B, T, 768))).cuda()
    z = torch.from_numpy(prng.integers(3, "bp.z", (B, T), 0, 512)).to(torch.int32).cuda()
    m8 = torch.ones(B, T, dtype=torch.uint8).cuda()
    Ps = [int(p) for p in args.P.split(",")]
    parent = load_other(args.parent_lib) if args.parent_lib else None
    lines = ["prompted generation, one MI355X, B = %d, T = %d, seed 5, top-k 52; device-event time per call, median of %d after %d "
             "warm-up calls (min .. max)" % (B, T, REPS, WARM),
             "(a) prefill + decode steps   (b) flags bit 0: all forced decode steps   (c) the prefill stage alone", ""]
    for mname in args.modes.split(","):
        mode = L.MODE_PERF_BF16 if mname == "bf16" else L.MODE_PARITY_F32
        e = make_engine(mode, sd)
        Pw = max(Ps)
        e.encode_ctx(v_s, v_a, m8, True, prompt_frames=Pw)
        lines.append("mode %s" % mname)

        def gen(**kw):
            return e.generate(z[:, 0].contiguous(), m8, T, 1.0, 52, None, 5, **kw)

        for P in Ps:
            prompt = z[:, :P].contiguous()
            row = "  P = %3d" % P
            if P == 1:
                t_tree = None
                if parent is not None:
                    hs = [make_engine(mode, sd, lib_) for lib_ in (None, parent, parent, None)]   # tree, parent, parent, tree
                    for h_ in hs:
                        h_.encode_ctx(v_s, v_a, m8, True)
                    fns = [lambda h_=h_: h_.generate(z[:, 0].contiguous(), m8, T, 1.0, 52, None, 5) for h_ in hs]
                    for _ in range(WARM):
                        for fn in fns:
                            fn()
                    torch.cuda.synchronize()
                    ts = [[] for _ in hs]
                    for _ in range(2 * REPS):
                        for fn, acc in zip(fns, ts):
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record()
                            fn()
                            e1.record()
                            torch.cuda.synchronize()
                            acc.append(e0.elapsed_time(e1))
                    same = torch.equal(fns[0](), fns[1]())
                    lines.append("  P =   1  dimx_generate, four handles called in turn, %d timed calls each; tokens of tree and parent equal: %s"
                                 % (2 * REPS, same))
                    for name, t_ in zip(("this tree, handle 1", "parent commit, handle 1", "parent commit, handle 2", "this tree, handle 2"), ts):
                        lines.append("           %-24s %s" % (name, fmt(t_)))
                    tree, par = ts[0] + ts[3], ts[1] + ts[2]
                    d = statistics.median(tree) - statistics.median(par)
                    spread = max(max(tree) - min(tree), max(par) - min(par))
                    lines.append("           median(tree, 20 samples) %.2f ms, median(parent, 20 samples) %.2f ms: tree - parent = %+.2f ms; spread "
                                 "(max - min over a build's 20 samples: tree %.2f ms, parent %.2f ms): %s"
                                 % (statistics.median(tree), statistics.median(par), d, max(tree) - min(tree), max(par) - min(par),
                                    "agree within the spread" if abs(d) <= spread else "DIFFER by more than the spread"))
                    for h_ in hs:
                        h_.close()
                else:
                    lines.append("  P =   1  dimx_generate, this tree %s | parent commit: not measured (no --parent-lib)" % fmt(timed(gen)))
            a = timed(lambda: gen(prompt=prompt, prefill=P))
            b = timed(lambda: gen(prompt=prompt, no_prefill=True))
            row += "  (a) %s  (b) %s" % (fmt(a), fmt(b))
            if P > 1:
                tokens = torch.empty(B, T - 1, dtype=torch.int32).cuda()
                ws, wsb = e.workspace(B, T, 1, P)

                def pre():
                    L.check(e.lib.dimx_generate_prompted(e.h, L.ptr(prompt), P, None, P, P, L.ptr(m8), B, T, 1, 1.0, 52, None, 5,
                                                         L.ptr(tokens), None, 4, ws, wsb, e._s()), "prefill only")
                row += "  (c) %s" % fmt(timed(pre))
                row += "  (a) < (b): %s" % (statistics.median(a) < statistics.median(b))
            lines.append(row)
            print(lines[-1], flush=True)
        lines.append("  chain faults on this handle: %d" % e.lib.dimx_chain_faults(e.h))
        lines.append("")
        e.close()
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
