"""Time the VQ-VAE training step (stage 1): the HIP step (dimx.train_hip.VqHipTrainer: forward + backward + AdamW) against the
PyTorch-autograd restatement (dimx.train.vq_loss + backward + torch.optim.AdamW) on the same GPU, B in {1, 16}, T = 300, in
both numeric modes (the autograd side runs f32, or bf16 autocast for the bf16 row).  Dropout 0.1 as in the reference's train
mode.  Medians of --iters timed steps after --warmup, CUDA events around each step.

    python tools/bench_train_vq.py [--iters 20] [--warmup 5] [--out profiles/vq_train_step.txt]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dimx  # noqa: E402,F401
from dimx import lib, prng  # noqa: E402
from dimx import train as TR  # noqa: E402
from dimx.config import DEFAULT_CONFIG, load_cfg_from_cfg_file  # noqa: E402
from dimx.models import VQAutoEncoder  # noqa: E402
from dimx.train_hip import VqHipTrainer  # noqa: E402


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--T", type=int, default=300)
    ap.add_argument("--batches", default="1,16")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cfg = load_cfg_from_cfg_file(DEFAULT_CONFIG)
    dev = torch.device("cuda:0")
    lines = ["# VQ-VAE training step (forward + backward + AdamW), T = %d, dropout 0.1, median of %d steps (ms); %s"
             % (args.T, args.iters, torch.cuda.get_device_name(0)),
             "%-5s %4s %10s %12s %8s" % ("mode", "B", "HIP (ms)", "autograd (ms)", "speedup")]
    for mode_name, mode in (("f32", lib.MODE_PARITY_F32), ("bf16", lib.MODE_PERF_BF16)):
        for B in (int(b) for b in args.batches.split(",")):
            x = torch.from_numpy(prng.normal(1, "bench.vq", (B, args.T, 56))).to(dev)
            model = VQAutoEncoder(cfg, numeric_mode=mode).to(dev)
            tr = VqHipTrainer(model, dropout=0.1)

            def hip_step():
                tr.forward_backward(x)
                tr.step()
            t_hip = timed(hip_step, args.iters, args.warmup)
            P = {k: v.detach().clone().requires_grad_(not k.endswith(".pe")) for k, v in model.state_dict().items()}
            opt = torch.optim.AdamW([v for k, v in P.items() if not k.endswith(".pe")], lr=1e-4)
            masks = tuple(torch.from_numpy(prng.dropout_scale_mask(1, 0, s, (B, args.T, 384), 0.1)).to(dev) for s in (0, 1))

            def torch_step():
                opt.zero_grad()
                with torch.enable_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=mode_name == "bf16"):
                    loss = TR.vq_loss(P, x, masks=masks)[0]
                loss.backward()
                opt.step()
            t_ag = timed(torch_step, args.iters, args.warmup)
            lines.append("%-5s %4d %10.2f %12.2f %7.1fx" % (mode_name, B, t_hip, t_ag, t_ag / t_hip))
            print(lines[-1], flush=True)
            del tr, model, P, opt
            torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
