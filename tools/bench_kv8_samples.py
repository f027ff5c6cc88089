"""FP8 cross K/V for best-of-N generation (dimx_set_cross_kv8_samples): what it costs and what it changes.
    python tools/bench_kv8_samples.py [--parent-tree PATH] [--out profiles/kv8_samples.txt] [--pairs 3] [--rounds 2] [--parts 1,2,3,4]

One MI355X, synthetic weights.  Every time is a device-event time after warm-up launches, reported as median (min .. max); the
helpers are tools/bench_kv8.py's.

 1. The launch alone at the best-of-10 step's shape (256 clips x 12 heads x 300 keys x S = 10), caches flushed before every launch:
    decode_attn_mq_kv8_kernel in its matrix-core form (bf16 q rows, bf16 out) against launch_attention_tr's multi-query launch on bf16
    caches, and in its exact form (f32 slabs, f32 out) against the VALU rows_per_clip launch of decode_attn.hip on f32 caches.  GB/s
    of K and V bytes (codes plus scales for the new launch).
 2. Best of 10 at 256 x 300 x 10, bf16 and f32, a fresh process per configuration, rounds alternating: plain, self kv8, kv8 samples,
    both.
 3. ``bench.py --gpus 1 --steps 20 --warmup 5``, parent (--parent-tree, a built checkout) and tree alternating: no launch on that
    path changed, so the tree has to lie inside the parent's own spread.
 4. Drift against the plain best-of-4, f32 mode, 32 clips x 150 frames x 4 samples: the logit difference teacher-forced along one token
    sequence, the share of equal tokens of free generations, and the Frechet distance between the two relative to the distance two
    sampler seeds give.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_kv8 import ROOT, B, T, H, _fmt, _inputs, _timed, default_path   # noqa: E402

S10 = 10
CONFIGS = ["plain", "self kv8", "kv8 samples", "kv8 samples + self kv8"]


def one(tree, mode, config):
    """a fresh process: one configuration's best-of-10 generate time -> one JSON line"""
    sd, v_s, v_a, start, m8 = _inputs(tree)
    from dimx import engine, lib as L
    e = engine.Engine("cuda:0", L.MODE_PERF_BF16 if mode == "bf16" else L.MODE_PARITY_F32)
    e.load_state_dict(sd)
    e.encode_ctx(v_s, v_a, m8, True, n_samples=S10)
    kw = {}
    if "samples" in config:
        kw["kv8_samples"] = True
    if "self" in config:
        kw["self_kv8"] = True
    t = _timed(lambda: e.generate(start, m8, T, 1.0, 52, None, 5, n_samples=S10, **kw), 2, 3)
    print(json.dumps({"ms": t, "faults": int(e.lib.dimx_chain_faults(e.h))}))


def kernel(lines):
    import torch
    sys.path.insert(0, ROOT)
    import dimx  # noqa: F401
    from dimx import engine as E, lib as L
    torch.set_grad_enabled(False)
    lib = L.load()
    g = torch.Generator().manual_seed(1)
    Tp, R, D = (T + 7) // 8 * 8, B * S10, 64
    kf = torch.randn(B, H, Tp, D, generator=g).cuda()
    vf = torch.randn(B, H, Tp, D, generator=g).cuda()
    kb, vb = kf.to(torch.bfloat16), vf.to(torch.bfloat16)
    k8, ks = E.op_kv8_quantize(kb, T)
    v8, vs = E.op_kv8_quantize(vb, T)
    q32 = torch.randn(1, R, H * D, generator=g).cuda()
    qb = q32[0].to(torch.bfloat16).contiguous()
    m8 = torch.ones(B, T, dtype=torch.uint8).cuda()
    ob, o32 = torch.empty(R, H * D, dtype=torch.bfloat16, device="cuda"), torch.empty(R, H * D, device="cuda")
    flush = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")     # larger than the 256 MB of last-level cache
    arr = lambda s: (ctypes.c_long * 3)(*s)
    st = L.stream_ptr(qb.device)

    def tr_multi():   # cross_attention_multi's launch: Lq = S queries per (clip, head), head-major caches, the key words packed by the call
        L.check(lib.dimx_op_attention_strided(L.ptr(qb), L.ptr(kb), L.ptr(vb), L.ptr(ob), B, H, S10, T, D, arr((S10 * H * D, H * D, D)),
                                              arr((H * Tp * D, D, Tp * D)), arr((H * Tp * D, D, Tp * D)), arr((S10 * H * D, H * D, D)), 0.125, 0,
                                              None, L.ptr(m8), T, 0, st), "dimx_op_attention_strided")

    def cold(fn):
        def run():
            flush.fill_(1)
            fn()
        return run
    t_flush = statistics.median(_timed(lambda: flush.fill_(1), 5, 30))
    sub = lambda fn: [x - t_flush for x in _timed(cold(fn), 5, 20)]
    t_tr = sub(tr_multi)
    t_mq = sub(lambda: E.op_decode_attn_kv8_multi(qb, k8, ks, v8, vs, 0.125, T, S10, kmask=m8, exact=False, out=ob))
    t_mq_slab = sub(lambda: E.op_decode_attn_kv8_multi(q32, k8, ks, v8, vs, 0.125, T, S10, kmask=m8, exact=False, out=ob))
    t_valu = sub(lambda: E.op_decode_attn_ex(q32, kf, vf, 0.125, n_keys=T, kmask=m8, rows_per_clip=S10, q_f32=True))
    t_valu_b = sub(lambda: E.op_decode_attn_ex(q32, kb, vb, 0.125, n_keys=T, kmask=m8, rows_per_clip=S10, q_f32=True))
    t_ex = sub(lambda: E.op_decode_attn_kv8_multi(q32, k8, ks, v8, vs, 0.125, T, S10, kmask=m8, exact=True, out=o32))
    by = lambda per_key: 2 * B * H * T * per_key
    rows = [("attention_tr multi-query, bf16 caches (+ its key-word pack)", t_tr, by(128)),
            ("decode_attn_mq_kv8, matrix-core form, bf16 q rows", t_mq, by(68)),
            ("decode_attn_mq_kv8, matrix-core form, one f32 slab", t_mq_slab, by(68)),
            ("decode_attn VALU rows_per_clip, bf16 caches", t_valu_b, by(128)),
            ("decode_attn VALU rows_per_clip, f32 caches", t_valu, by(256)),
            ("decode_attn_mq_kv8, exact form, one f32 slab", t_ex, by(68))]
    lines.append("1. the launch alone, %d clips x %d heads x %d keys (Tp = %d) x S = %d, mask on, caches flushed before every launch (a 512 MB fill, "
                 "its own median %.3f ms subtracted); 20 launches after 5 warm-ups; bytes = the K and V rows read (+ scales)  [measured]"
                 % (B, H, T, Tp, S10, t_flush))
    for name, t, nbytes in rows:
        lines.append("   %-62s %s  %6.1f MB  %6.0f GB/s" % (name, _fmt(t), nbytes / 1e6, nbytes / statistics.median(t) / 1e6))
    med = statistics.median
    lines.append("   matrix-core form / attention_tr = %.3f in time; exact form / VALU f32 = %.3f in time" % (med(t_mq) / med(t_tr), med(t_ex) / med(t_valu)))
    for ln in lines[-8:]:
        print(ln, flush=True)


def _run_one(mode, config):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", ROOT, mode, config], capture_output=True, text=True, timeout=400)
    if r.returncode != 0:
        raise RuntimeError("%s %s ended with %d: %s" % (mode, config, r.returncode, r.stderr[-2000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def generation(lines, rounds):
    lines.append("2. best of 10, B = %d, T = %d, %d samples per clip, seed 5, top-k 52: dimx_generate per call, a fresh process per configuration and "
                 "round (2 warm-up calls, then 3 timed), %d rounds in the order listed  [measured]" % (B, T, S10, rounds))
    for mode in ("bf16", "f32"):
        got = {c: [] for c in CONFIGS}
        faults = 0
        for _ in range(rounds):
            for c in CONFIGS:
                out = _run_one(mode, c)
                got[c] += out["ms"]
                faults += out["faults"]
        base = statistics.median(got[CONFIGS[0]])
        lines.append("   %s (ratios against %s; chain faults: %d)" % (mode, CONFIGS[0], faults))
        for c in CONFIGS:
            lines.append("     %-24s %s   x %.3f   %.3f ms per step" % (c, _fmt(got[c]), statistics.median(got[c]) / base, statistics.median(got[c]) / (T - 1)))
            print(lines[-1], flush=True)


def drift(lines):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import dimx  # noqa: F401
    from dimx import kv8, metrics as M, prng
    from dimx.seq2seq_pretrain import SLMFT
    torch.set_grad_enabled(False)
    Bd, Td, Sd = 32, 150, 4
    model = SLMFT().eval()
    v_s = torch.from_numpy(prng.normal(4, "bk.d.vs", (Bd, Td, 56))).cuda()
    v_l = torch.from_numpy(prng.normal(4, "bk.d.vl", (Bd, Td, 56))).cuda()
    v_a = torch.from_numpy(prng.normal(4, "bk.d.va", (Bd, Td, 768))).cuda()
    mask = torch.ones(Bd, Td, dtype=torch.bool).cuda()
    run = lambda seed, k8: model(v_s, v_l, v_a, mask, mode="val", seed=seed, return_tokens=True, n_samples=Sd, kv8_samples=k8)
    _, _, p0, t0 = run(11, False)
    _, _, p8, t8 = run(11, True)
    _, _, p1, _ = run(12, False)
    clips = lambda p: [c for c in p.reshape(Bd * Sd, Td - 1, -1).float().cpu().numpy().astype(np.float64)]
    same = (t0.reshape(Bd * Sd, -1) == t8.reshape(Bd * Sd, -1))
    first = torch.where(same.all(1), torch.full((Bd * Sd,), same.shape[1], device=same.device), (~same).float().argmax(1)).float().mean().item()
    between, seeds = M.summarize(clips(p0), clips(p8)), M.summarize(clips(p0), clips(p1))
    # teacher-forced along the plain run's first samples: the same token history in both runs, on all S rows of a clip
    eng = model.engine(v_s.device)
    m8 = mask.to(torch.uint8)
    z0 = model.forward_vq(v_s, v_l, mask, with_speaker=False)[1][:, :1]
    prompt = torch.cat([z0, t0.reshape(Bd, Sd, -1)[:, 0, :Td - 2]], 1).to(torch.int32).contiguous()
    out = {}
    for k8 in (False, True):
        eng.encode_ctx(v_s, v_a, m8, True, n_samples=Sd)
        out[k8] = eng.generate(None, m8, Td, 0.0, 52, None, return_logits=True, n_samples=Sd, prompt=prompt, no_prefill=True,
                               kv8_samples=k8)[1].cpu().numpy()
    d = kv8.drift(out[True], out[False], t8.cpu().numpy(), t0.cpu().numpy())
    lines.append("4. drift against the plain best-of-%d, f32 mode, synthetic weights, %d clips x %d frames x %d samples  [measured; no claim about "
                 "trained checkpoints]" % (Sd, Bd, Td, Sd))
    lines.append("   teacher-forced along the plain run's tokens: |logits kv8 samples - plain| max %.3e, mean %.3e (logit spread %.3f: max = %.3f of "
                 "it); arg-max equal on %.2f %% of the steps" % (d["logit_max_abs"], d["logit_mean_abs"], float(out[False].std()),
                                                               d["logit_rel_to_spread"], 100 * d["argmax_equal"]))
    lines.append("   free generations, same sampler seed: %.1f %% of the tokens equal, %.1f steps before the first difference on average"
                 % (100 * d["tokens_equal"], first))
    for part in ("pose", "exp"):
        lines.append("   Frechet distance, %s: kv8 samples vs plain %.4g, two sampler seeds %.4g: ratio %.3f" % (
            part, between[part]["fd"], seeds[part]["fd"], between[part]["fd"] / seeds[part]["fd"] if seeds[part]["fd"] > 0 else float("nan")))
    for ln in lines[-5:]:
        print(ln, flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        return one(sys.argv[2], sys.argv[3], sys.argv[4])
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv8_samples.txt"))
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--parts", default="1,2,3,4", help="which measurements to run")
    args = ap.parse_args()
    parent = os.path.abspath(args.parent_tree) if args.parent_tree else None
    parts = set(args.parts.split(","))
    lines = ["FP8 cross K/V for best-of-N generation (dimx_set_cross_kv8_samples): measurements of tools/bench_kv8_samples.py", "=" * 108, ""]
    # the fresh-process measurements first: they never share the GPU with this process's own handles
    later, gen = [], []
    if "3" in parts:
        default_path(later, parent, args.pairs)
        later[0] = "3" + later[0][1:]
        later.append("")
    if "2" in parts:
        generation(gen, args.rounds)
        gen.append("")
    if "1" in parts:
        kernel(lines)
        lines.append("")
    lines += gen + later
    if "4" in parts:
        drift(lines)
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
