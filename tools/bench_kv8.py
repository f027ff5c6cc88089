"""FP8 cross-attention K/V (dimx_set_cross_kv8): what it costs and what it changes.
    python tools/bench_kv8.py [--parent-tree PATH] [--out profiles/kv8_generate.txt] [--pairs 3] [--rounds 2]

One MI355X, synthetic weights.  Every time is a device-event time after warm-up launches, reported as median (min .. max).

 1. The kernel alone at the step's shape (B = 256, H = 12, 300 keys): decode_attn_kv8_kernel against decode_attn_kernel on bf16
    caches, achieved GB/s of each (K and V bytes, plus the scales for kv8).
 2. The quantiser at the headline shape: the 8 launches of one generation (4 layers, K and V).
 3. Generation at 256 x 300, bf16 and f32: every configuration is a fresh process (``--one``), the rounds alternate between the
    parent commit's default route (--parent-tree, a built checkout) and this tree's configurations: default, kv8 (chain route in
    bf16), kv8 with DIMX_NO_CHAIN=1 (bf16), window (lookahead 0), window + kv8.
 4. ``bench.py --gpus 1 --steps 20 --warmup 5`` (the flagship leg alone), parent and tree alternating: no launch on that path
    changed, so the tree has to lie inside the parent's own spread.
 5. Drift, f32 mode: the logit difference between kv8 and plain teacher-forced along one token sequence, the share of equal tokens
    of free generations, and the Frechet distance between kv8 and plain generations relative to the distance two sampler seeds give
    (dimx/mode_compare.py's comparison).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, T, H = 256, 300, 12
BENCH = ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5", "--no-cpu-baseline", "--no-roofline", "--no-mode-compare",
         "--no-parity-mode", "--no-train-step", "--no-shard-check", "--no-best-of-n"]


def _fmt(t):
    return "%8.3f ms (%.3f .. %.3f)" % (statistics.median(t), min(t), max(t))


def _timed(fn, warm, reps):
    import torch
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


def _inputs(tree):
    import torch
    sys.path.insert(0, tree)
    import dimx  # noqa: F401
    from dimx import prng, weights
    torch.set_grad_enabled(False)
    sd = weights.synth_state_dict(weights.slmft_spec(), 20260928)
    v_s = torch.from_numpy(prng.normal(3, "bk.vs", (B, T, 56))).cuda()
    v_a = torch.from_numpy(prng.normal(3, "bk.va", (B, T, 768))).cuda()
    start = torch.from_numpy(prng.integers(3, "bk.z", (B,), 0, 512)).to(torch.int32).cuda()
    return sd, v_s, v_a, start, torch.ones(B, T, dtype=torch.uint8).cuda()


def one(tree, mode, config):
    """a fresh process: one configuration's generate time -> one JSON line"""
    import torch
    sd, v_s, v_a, start, m8 = _inputs(tree)
    from dimx import engine, lib as L
    e = engine.Engine("cuda:0", L.MODE_PERF_BF16 if mode == "bf16" else L.MODE_PARITY_F32)
    e.load_state_dict(sd)
    e.encode_ctx(v_s, v_a, m8, True)
    kw = {}
    if "kv8" in config:
        kw["kv8"] = True
    if "win" in config:
        kw["lookahead"] = 0
    t = _timed(lambda: e.generate(start, m8, T, 1.0, 52, None, 5, **kw), 2, 5 if mode == "bf16" else 3)
    print(json.dumps({"ms": t, "faults": int(e.lib.dimx_chain_faults(e.h))}))


def kernel_and_quantiser(lines):
    import torch
    sys.path.insert(0, ROOT)
    import dimx  # noqa: F401
    from dimx import engine as E
    torch.set_grad_enabled(False)
    g = torch.Generator().manual_seed(1)
    Tp = (T + 7) // 8 * 8
    kc = torch.randn(B, H, Tp, 64, generator=g).to(torch.bfloat16).cuda()
    vc = torch.randn(B, H, Tp, 64, generator=g).to(torch.bfloat16).cuda()
    q = torch.randn(1, B, H * 64, generator=g).cuda()
    k8, ks = E.op_kv8_quantize(kc, T)
    v8, vs = E.op_kv8_quantize(vc, T)
    m8 = torch.ones(B, T, dtype=torch.uint8).cuda()
    flush = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")     # larger than the 256 MB of last-level cache

    def cold(fn):
        def run():
            flush.fill_(1)
            fn()
        return run
    t_flush = statistics.median(_timed(lambda: flush.fill_(1), 5, 30))
    t_plain = [x - t_flush for x in _timed(cold(lambda: E.op_decode_attn_ex(q, kc, vc, 0.125, n_keys=T, kmask=m8, q_f32=True)), 5, 30)]
    t_kv8 = [x - t_flush for x in _timed(cold(lambda: E.op_decode_attn_kv8(q, k8, ks, v8, vs, 0.125, T, kmask=m8, out_bf16=True)), 5, 30)]
    by_plain = 2 * B * H * T * 128
    by_kv8 = 2 * B * H * T * (64 + 4)
    lines.append("1. the kernel alone, B = %d, H = %d, %d keys (Tp = %d), mask on, automatic wave count, caches flushed before every launch "
                 "(a 512 MB fill, its own median %.3f ms subtracted); 30 launches after 5 warm-ups  [measured]" % (B, H, T, Tp, t_flush))
    lines.append("   decode_attn_kernel, bf16 caches   %s  %6.1f MB  %7.0f GB/s" % (_fmt(t_plain), by_plain / 1e6, by_plain / statistics.median(t_plain) / 1e6))
    lines.append("   decode_attn_kv8_kernel, out bf16  %s  %6.1f MB  %7.0f GB/s" % (_fmt(t_kv8), by_kv8 / 1e6, by_kv8 / statistics.median(t_kv8) / 1e6))
    lines.append("   kv8 / plain = %.3f in time" % (statistics.median(t_kv8) / statistics.median(t_plain)))

    def quant_all():
        for _ in range(4):
            E.op_kv8_quantize(kc, T, k8, ks)
            E.op_kv8_quantize(vc, T, v8, vs)
    tq = _timed(quant_all, 3, 10)
    rd, wr = 8 * B * H * T * 128, 8 * B * H * T * 68
    lines.append("2. the quantiser, one generation's 8 launches (4 layers x K, V) at B = %d, T = %d, bf16 caches: %s; %.2f GB read, %.2f GB written: "
                 "%.0f GB/s  [measured]" % (B, T, _fmt(tq), rd / 1e9, wr / 1e9, (rd + wr) / statistics.median(tq) / 1e6))
    for ln in lines[-6:]:
        print(ln, flush=True)


def _run_one(tree, mode, config, env=None):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", tree, mode, config], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, **(env or {})))
    if r.returncode != 0:
        raise RuntimeError("%s %s %s ended with %d: %s" % (tree, mode, config, r.returncode, r.stderr[-2000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def generation(lines, parent_tree, rounds):
    lines.append("3. generation, B = %d, T = %d, seed 5, top-k 52: dimx_generate per call, a fresh process per configuration and round (2 warm-up "
                 "calls, 5 timed in bf16 / 3 in f32), %d rounds in the order listed  [measured]" % (B, T, rounds))
    for mode in ("bf16", "f32"):
        configs = [("parent default", parent_tree, "default", None)] if parent_tree else []
        configs += [("tree default", ROOT, "default", None), ("tree kv8", ROOT, "kv8", None)]
        if mode == "bf16":
            configs.append(("tree kv8, DIMX_NO_CHAIN=1", ROOT, "kv8", {"DIMX_NO_CHAIN": "1"}))
        configs += [("tree window L=0", ROOT, "win", None), ("tree window L=0 + kv8", ROOT, "win+kv8", None)]
        got = {c[0]: [] for c in configs}
        faults = 0
        for _ in range(rounds):
            for name, tree, config, env in configs:
                out = _run_one(tree, mode, config, env)
                got[name] += out["ms"]
                faults += out["faults"]
        base = statistics.median(got[configs[0][0]])
        lines.append("   %s (ratios against %s; chain faults: %d)" % (mode, configs[0][0], faults))
        for name, *_ in configs:
            lines.append("     %-28s %s   x %.3f" % (name, _fmt(got[name]), statistics.median(got[name]) / base))
            print(lines[-1], flush=True)
    if not parent_tree:
        lines.append("   the parent commit's default route: not measured (no --parent-tree)")


def run_bench(tree):
    r = subprocess.run([sys.executable] + BENCH, cwd=tree, capture_output=True, text=True, timeout=420)
    if r.returncode != 0:
        raise RuntimeError("bench.py in %s ended with %d: %s" % (tree, r.returncode, r.stderr[-2000:]))
    for line in reversed(r.stdout.splitlines()):
        if line.startswith("{") and '"value"' in line:
            return float(json.loads(line)["value"])
    raise RuntimeError("no result line from bench.py in %s" % tree)


def default_path(lines, parent_tree, pairs):
    lines.append("4. %s, a fresh process per run, parent and tree alternating, %d pairs" % (" ".join(BENCH[:7]), pairs))
    if not parent_tree:
        lines.append("   not measured (no --parent-tree)")
        return
    runs = {"parent": [], "tree": []}
    for i in range(pairs):
        for name, tree in (("parent", parent_tree), ("tree", ROOT)):
            runs[name].append(run_bench(tree))
            lines.append("   pair %d  %-7s %9.2f clips/s" % (i + 1, name, runs[name][-1]))
            print(lines[-1], flush=True)
    par, tre = runs["parent"], runs["tree"]
    spread, mp, mt = max(par) - min(par), statistics.median(par), statistics.median(tre)
    lines.append("   parent median %.2f clips/s, spread (max - min) %.2f = %.2f %%; tree median %.2f: %+.2f %%: %s  [measured]"
                 % (mp, spread, 100 * spread / mp, mt, 100 * (mt - mp) / mp,
                    "inside the parent's spread" if mt >= mp - spread else "SLOWER than the parent by more than its spread"))


def drift(lines):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import dimx  # noqa: F401
    from dimx import kv8, metrics as M, prng
    from dimx.seq2seq_pretrain import SLMFT
    torch.set_grad_enabled(False)
    Bd, Td = 64, 150
    model = SLMFT().eval()
    v_s = torch.from_numpy(prng.normal(4, "bk.d.vs", (Bd, Td, 56))).cuda()
    v_l = torch.from_numpy(prng.normal(4, "bk.d.vl", (Bd, Td, 56))).cuda()
    v_a = torch.from_numpy(prng.normal(4, "bk.d.va", (Bd, Td, 768))).cuda()
    mask = torch.ones(Bd, Td, dtype=torch.bool).cuda()
    run = lambda seed, k8: model(v_s, v_l, v_a, mask, mode="val", seed=seed, return_tokens=True, kv8=k8)
    _, _, p0, t0 = run(11, False)
    _, _, p8, t8 = run(11, True)
    _, _, p1, _ = run(12, False)
    clips = lambda p: [c for c in p.float().cpu().numpy().astype(np.float64)]
    same = (t0.reshape(Bd, -1) == t8.reshape(Bd, -1))
    first = torch.where(same.all(1), torch.full((Bd,), same.shape[1], device=same.device), (~same).float().argmax(1)).float().mean().item()
    between, seeds = M.summarize(clips(p0), clips(p8)), M.summarize(clips(p0), clips(p1))
    # teacher-forced along the plain run's tokens: the same token history in both runs
    eng = model.engine(v_s.device)
    m8 = mask.to(torch.uint8)
    z0 = model.forward_vq(v_s, v_l, mask, with_speaker=False)[1][:, :1]
    prompt = torch.cat([z0, t0.reshape(Bd, -1)[:, :Td - 2]], 1).to(torch.int32).contiguous()
    out = {}
    for k8 in (False, True):
        eng.encode_ctx(v_s, v_a, m8, True)
        out[k8] = eng.generate(None, m8, Td, 0.0, 52, None, return_logits=True, prompt=prompt, no_prefill=True, kv8=k8)[1].cpu().numpy()
    d = kv8.drift(out[True], out[False], t8.cpu().numpy(), t0.cpu().numpy())
    lines.append("5. drift, f32 mode, synthetic weights, %d clips x %d frames  [measured; no claim about trained checkpoints]" % (Bd, Td))
    lines.append("   teacher-forced along the plain run's tokens: |logits kv8 - plain| max %.3e, mean %.3e (logit spread %.3f: max = %.3f of it); "
                 "arg-max equal on %.2f %% of the steps" % (d["logit_max_abs"], d["logit_mean_abs"], float(out[False].std()), d["logit_rel_to_spread"],
                                                          100 * d["argmax_equal"]))
    lines.append("   free generations, same sampler seed: %.1f %% of the tokens equal, %.1f steps before the first difference on average"
                 % (100 * d["tokens_equal"], first))
    for part in ("pose", "exp"):
        lines.append("   Frechet distance, %s: kv8 vs plain %.4g, two sampler seeds %.4g: ratio %.3f" % (
            part, between[part]["fd"], seeds[part]["fd"], between[part]["fd"] / seeds[part]["fd"] if seeds[part]["fd"] > 0 else float("nan")))
    for ln in lines[-5:]:
        print(ln, flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        return one(sys.argv[2], sys.argv[3], sys.argv[4])
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv8_generate.txt"))
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--parts", default="1,3,4,5", help="which measurements to run (1 includes 2)")
    args = ap.parse_args()
    parent = os.path.abspath(args.parent_tree) if args.parent_tree else None
    parts = set(args.parts.split(","))
    lines = ["FP8 cross-attention K/V (dimx_set_cross_kv8): measurements of tools/bench_kv8.py", "=" * 84, ""]
    later = []
    # the fresh-process measurements first: they never share the GPU with this process's own handles
    if "4" in parts:
        default_path(later, parent, args.pairs)
        later.append("")
    gen = []
    if "3" in parts:
        generation(gen, parent, args.rounds)
        gen.append("")
    if "1" in parts:
        kernel_and_quantiser(lines)
        lines.append("")
    lines += gen + later
    if "5" in parts:
        drift(lines)
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
