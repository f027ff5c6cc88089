"""FP8 self-attention K/V caches (dimx_set_self_kv8): what they cost and what they change.
    python tools/bench_self_kv8.py [--parent-tree PATH] [--out profiles/self_kv8_generate.txt] [--pairs 3] [--rounds 2]

One MI355X, synthetic weights.  Every time is a device-event time after warm-up launches, reported as median (min .. max); the
helpers are tools/bench_kv8.py's.

 1. The kernel alone at the best-of-10 shape (2560 rows x 12 heads), steps 150 and 299: decode_attn_self_kv8_kernel against the plain
    self launch (decode_attn_kernel, SELF) on bf16 caches, caches flushed, achieved GB/s of each (K and V bytes, plus the scales).
 2. Generation at 256 x 300, one sample per clip, bf16 and f32, a fresh process per configuration, rounds alternating: plain, cross
    kv8, self kv8, both.
 3. Best of 10 at 256 x 300 x 10, bf16 and f32: plain against self kv8.
 4. ``bench.py --gpus 1 --steps 20 --warmup 5``, parent (--parent-tree, a built checkout) and tree alternating: no launch on that
    path changed, so the tree has to lie inside the parent's own spread.
 5. Drift, f32 mode, 64 x 150: the logit difference between self kv8 and plain teacher-forced along one token sequence, the share of
    equal tokens of free generations, and the Frechet distance between the two relative to the distance two sampler seeds give.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_kv8 import BENCH, ROOT, B, T, H, _fmt, _inputs, _timed, default_path   # noqa: E402


def one(tree, mode, config, S):
    """a fresh process: one configuration's generate time -> one JSON line"""
    sd, v_s, v_a, start, m8 = _inputs(tree)
    from dimx import engine, lib as L
    e = engine.Engine("cuda:0", L.MODE_PERF_BF16 if mode == "bf16" else L.MODE_PARITY_F32)
    e.load_state_dict(sd)
    e.encode_ctx(v_s, v_a, m8, True, n_samples=S)
    kw = {}
    if "cross" in config:
        kw["kv8"] = True
    if "self" in config:
        kw["self_kv8"] = True
    t = _timed(lambda: e.generate(start, m8, T, 1.0, 52, None, 5, n_samples=S, **kw), 2, (5 if mode == "bf16" else 3) if S == 1 else 3)
    print(json.dumps({"ms": t, "faults": int(e.lib.dimx_chain_faults(e.h))}))


def kernel(lines):
    import torch
    sys.path.insert(0, ROOT)
    import dimx  # noqa: F401
    from dimx import engine as E
    torch.set_grad_enabled(False)
    g = torch.Generator().manual_seed(1)
    R, Tp = 2560, (T + 7) // 8 * 8
    kc = torch.randn(R // 10, H, T, 64, generator=g).to(torch.bfloat16).cuda().repeat(10, 1, 1, 1)
    vc = torch.randn(R // 10, H, T, 64, generator=g).to(torch.bfloat16).cuda().repeat(10, 1, 1, 1)
    qkv = torch.randn(1, R, 3 * H * 64, generator=g).cuda()
    pad = lambda c: torch.nn.functional.pad(c, (0, 0, 0, Tp - T)).contiguous()
    k8, ks = E.op_kv8_quantize(pad(kc), T)
    v8, vs = E.op_kv8_quantize(pad(vc), T)
    flush = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")     # larger than the 256 MB of last-level cache

    def cold(fn):
        def run():
            flush.fill_(1)
            fn()
        return run
    t_flush = statistics.median(_timed(lambda: flush.fill_(1), 5, 30))
    lines.append("1. the kernel alone, %d rows x %d heads, automatic wave count, caches flushed before every launch (a 512 MB fill, its own median "
                 "%.3f ms subtracted); 20 launches after 5 warm-ups; bytes = the K and V rows read (+ scales)  [measured]" % (R, H, t_flush))
    for n in (150, 299):
        step = torch.tensor([n], dtype=torch.int32, device="cuda")
        t_plain = [x - t_flush for x in _timed(cold(lambda: E.op_decode_attn_ex(qkv, kc, vc, 0.125, step=step, q_f32=True)), 5, 20)]
        t_kv8 = [x - t_flush for x in _timed(cold(lambda: E.op_decode_attn_self_kv8(qkv, k8, ks, v8, vs, 0.125, n, out_bf16=True, step=step)), 5, 20)]
        by_plain, by_kv8 = 2 * R * H * n * 128, 2 * R * H * n * (64 + 4)
        lines.append("   %3d cached rows  decode_attn_kernel (SELF), bf16 caches  %s  %7.1f MB  %6.0f GB/s" % (n, _fmt(t_plain), by_plain / 1e6, by_plain / statistics.median(t_plain) / 1e6))
        lines.append("                    decode_attn_self_kv8_kernel, out bf16   %s  %7.1f MB  %6.0f GB/s   kv8 / plain = %.3f in time"
                     % (_fmt(t_kv8), by_kv8 / 1e6, by_kv8 / statistics.median(t_kv8) / 1e6, statistics.median(t_kv8) / statistics.median(t_plain)))
    for ln in lines[-5:]:
        print(ln, flush=True)


def _run_one(mode, config, S, env=None):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", ROOT, mode, config, str(S)], capture_output=True, text=True, timeout=400,
                       env=dict(os.environ, **(env or {})))
    if r.returncode != 0:
        raise RuntimeError("%s %s S=%d ended with %d: %s" % (mode, config, S, r.returncode, r.stderr[-2000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def generation(lines, rounds, S, configs, title):
    lines.append("%s, B = %d, T = %d, %d sample(s) per clip, seed 5, top-k 52: dimx_generate per call, a fresh process per configuration and round "
                 "(2 warm-up calls, then %s timed), %d rounds in the order listed  [measured]" % (title, B, T, S, "5 in bf16 / 3 in f32" if S == 1 else "3", rounds))
    for mode in ("bf16", "f32"):
        got = {c: [] for c in configs}
        faults = 0
        for _ in range(rounds):
            for c in configs:
                out = _run_one(mode, c, S)
                got[c] += out["ms"]
                faults += out["faults"]
        base = statistics.median(got[configs[0]])
        lines.append("   %s (ratios against %s; chain faults: %d)" % (mode, configs[0], faults))
        for c in configs:
            lines.append("     %-22s %s   x %.3f   %.3f ms per step" % (c, _fmt(got[c]), statistics.median(got[c]) / base, statistics.median(got[c]) / (T - 1)))
            print(lines[-1], flush=True)


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
    run = lambda seed, k8: model(v_s, v_l, v_a, mask, mode="val", seed=seed, return_tokens=True, self_kv8=k8)
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
        out[k8] = eng.generate(None, m8, Td, 0.0, 52, None, return_logits=True, prompt=prompt, no_prefill=True, self_kv8=k8)[1].cpu().numpy()
    d = kv8.drift(out[True], out[False], t8.cpu().numpy(), t0.cpu().numpy())
    lines.append("5. drift, f32 mode, synthetic weights, %d clips x %d frames  [measured; no claim about trained checkpoints]" % (Bd, Td))
    lines.append("   teacher-forced along the plain run's tokens (all four layers on codes): |logits self kv8 - plain| max %.3e, mean %.3e (logit spread "
                 "%.3f: max = %.3f of it); arg-max equal on %.2f %% of the steps" % (d["logit_max_abs"], d["logit_mean_abs"], float(out[False].std()),
                                                                                    d["logit_rel_to_spread"], 100 * d["argmax_equal"]))
    lines.append("   free generations, same sampler seed: %.1f %% of the tokens equal, %.1f steps before the first difference on average"
                 % (100 * d["tokens_equal"], first))
    for part in ("pose", "exp"):
        lines.append("   Frechet distance, %s: self kv8 vs plain %.4g, two sampler seeds %.4g: ratio %.3f" % (
            part, between[part]["fd"], seeds[part]["fd"], between[part]["fd"] / seeds[part]["fd"] if seeds[part]["fd"] > 0 else float("nan")))
    for ln in lines[-5:]:
        print(ln, flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        return one(sys.argv[2], sys.argv[3], sys.argv[4], int(sys.argv[5]))
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "self_kv8_generate.txt"))
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--parts", default="1,2,3,4,5", help="which measurements to run")
    args = ap.parse_args()
    parent = os.path.abspath(args.parent_tree) if args.parent_tree else None
    parts = set(args.parts.split(","))
    lines = ["FP8 self-attention K/V caches (dimx_set_self_kv8): measurements of tools/bench_self_kv8.py", "=" * 92, ""]
    # the fresh-process measurements first: they never share the GPU with this process's own handles
    later, gen = [], []
    if "4" in parts:
        default_path(later, parent, args.pairs)
        later.append("")
    if "2" in parts:
        generation(gen, args.rounds, 1, ["plain", "cross kv8", "self kv8", "cross + self kv8"], "2. generation")
        gen.append("")
    if "3" in parts:
        generation(gen, args.rounds, 10, ["plain", "self kv8"], "3. best of 10")
        gen.append("")
    if "1" in parts:
        kernel(lines)
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
