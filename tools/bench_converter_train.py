"""One training step of the DIM-Speaker converter head (ConverterHipTrainer: csrc/train.hip conv_run, csrc/lstm.hip,
csrc/train_lstm.hip) on one GPU:
    python tools/bench_converter_train.py [out.txt]     # event-timed table -> profiles/converter_train.txt by default
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_converter_train.py --trace   # one step per path, for a kernel trace
Rows, at B in {1, 8}, T = 300, V = 70110, both numeric modes, default path (forward recurrence on the group kernel) and flags
bit 0 (everything on the no-communication path):
  * step: forward + backward + AdamW;    * fwd+bwd alone;
  * torch: the same step with torch.nn.LSTM / nn.Linear, autograd and torch.optim.AdamW on the same GPU (f32; the comparison row).
The frozen VQ-VAE is outside every row (its output is the input).  Median (min .. max) of 5 device-event timings after 2
warm-up calls, the method of tools/bench_speaker.py."""
import statistics
import sys

import torch

sys.path.insert(0, ".")
import dimx  # noqa: E402,F401
from dimx import lib as L  # noqa: E402
from dimx.seq2seq_pretrain import EmocaConverter  # noqa: E402
from dimx.train_hip import ConverterHipTrainer  # noqa: E402

V = 70110
T = 300
BATCHES = (1, 8)


def timed(fn, warm=2, reps=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts), max(ts)


def torch_step(sd, mouth_idx):
    lstm = torch.nn.LSTM(56, 384, 2, batch_first=True, bidirectional=True)
    lstm.load_state_dict({k[len("vertice_map_reverse_lstm."):]: v for k, v in sd.items() if k.startswith("vertice_map_reverse_lstm.")})
    l1, l2 = torch.nn.Linear(768, 768), torch.nn.Linear(768, V)
    l1.load_state_dict({"weight": sd["vertice_map_reverse.0.weight"], "bias": sd["vertice_map_reverse.0.bias"]})
    l2.load_state_dict({"weight": sd["vertice_map_reverse.2.weight"], "bias": sd["vertice_map_reverse.2.bias"]})
    mods = torch.nn.ModuleList([lstm, l1, l2]).cuda().train()
    opt = torch.optim.AdamW(mods.parameters(), lr=1e-5)
    mse = torch.nn.MSELoss()

    def run(motion, templ, target):
        opt.zero_grad()
        B, Tn, _ = motion.shape
        y, _ = mods[0](motion)
        xp = mods[2](torch.nn.functional.leaky_relu(mods[1](y), 0.2)) + templ[:, None]
        loss = mse(xp, target) + 5 * mse(xp.reshape(B, Tn, V // 3, 3)[:, :, mouth_idx, :], target.reshape(B, Tn, V // 3, 3)[:, :, mouth_idx, :])
        loss.backward()
        opt.step()
        return loss
    return run


def main():
    trace = "--trace" in sys.argv
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else "profiles/converter_train.txt"
    dev = torch.device("cuda:0")
    lines = ["# tools/bench_converter_train.py on %s; ms, median (min .. max) of 5 device-event timings after 2 warm-up calls" % torch.cuda.get_device_name(0),
             "# step = forward + loss + backward + AdamW of 2 x bidirectional LSTM(384) + Linear(768,768) + LeakyReLU + Linear(768,%d); T = %d" % (V, T)]
    mouth_map = list(range(0, V // 3, 5))
    mouth_idx = torch.as_tensor(mouth_map, device=dev)
    for mode, mname in ((L.MODE_PARITY_F32, "f32"), (L.MODE_PERF_BF16, "bf16")):
        model = EmocaConverter(mesh_dim=V, numeric_mode=mode).to(dev)
        tr = ConverterHipTrainer(model)
        th = None
        if mode == L.MODE_PARITY_F32:
            th = torch_step({k: v.detach().cpu() for k, v in model.state_dict().items() if k.startswith("vertice_map_reverse")},
                            mouth_idx)
        for B in BATCHES:
            torch.manual_seed(B)
            motion = torch.randn(B, T, 56, device=dev)
            templ = 0.1 * torch.randn(B, V, device=dev)
            target = templ[:, None] + 0.01 * torch.randn(B, T, V, device=dev)

            def step(flags):
                tr.forward_backward(target, templ, None, mouth_map=mouth_map, flags=flags, motion=motion)
                tr.step()
            cases = [("step        default", lambda: step(0)),
                     ("fwd+bwd     default", lambda: tr.forward_backward(target, templ, None, mouth_map=mouth_map, motion=motion)),
                     ("step        safe   ", lambda: step(1)),
                     ("fwd+bwd     safe   ", lambda: tr.forward_backward(target, templ, None, mouth_map=mouth_map, flags=1, motion=motion))]
            if th is not None:
                cases.append(("torch autograd+AdamW", lambda: th(motion, templ, target)))
            for name, fn in cases:
                if trace:
                    if B == 1 and mode == L.MODE_PARITY_F32:
                        fn()
                        torch.cuda.synchronize()
                    continue
                try:
                    med, lo, hi = timed(fn)
                except RuntimeError as e:
                    if not name.startswith("torch"):
                        raise
                    lines.append("%-4s B=%-3d T=%d  %-20s not run by torch: %s" % (mname, B, T, name, str(e).splitlines()[0][:80]))
                    print(lines[-1], flush=True)
                    continue
                lines.append("%-4s B=%-3d T=%d  %-20s %9.3f  (%.3f .. %.3f)" % (mname, B, T, name, med, lo, hi))
                print(lines[-1], flush=True)
            del motion, templ, target
            torch.cuda.empty_cache()
        lines.append("%-4s lstm faults: %d" % (mname, tr.eng.lstm_faults()))
        print(lines[-1], flush=True)
        del tr, model, th
        torch.cuda.empty_cache()
    if not trace:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
