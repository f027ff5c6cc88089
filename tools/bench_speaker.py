"""The DIM-Speaker converter head (csrc/lstm.hip + the two Linear layers, dimx_mesh_head) on one GPU:
    python tools/bench_speaker.py [out.txt]            # event-timed table -> profiles/speaker_head.txt by default
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_speaker.py --trace    # one short pass per path for a kernel trace
Times, at (B, T) in {(1,300), (8,300), (64,300)} (L = T - 1 frames), both numeric modes:
  * the whole head at V = 70110 on the group path and on the safe path (flags bit 0);
  * the same at V = 8, i.e. the two LSTM layers + Linear(768, 768) alone (the last projection is then negligible);
  * torch.nn.LSTM + the two nn.Linear on the same GPU (what the reference itself runs: MIOpen / rocBLAS), f32 and bf16.
Every figure is a median of device-event timings after warm-up; the group path's time includes its two host waits (it reads a
fault word after each layer)."""
import statistics
import sys

import torch

sys.path.insert(0, ".")
import dimx  # noqa: E402,F401
from dimx import lib as L  # noqa: E402
from dimx import weights  # noqa: E402
from dimx.engine import Engine  # noqa: E402

SHAPES = [(1, 300), (8, 300), (64, 300)]
V_FULL = 70110


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


def torch_head(sd, V, dtype):
    lstm = torch.nn.LSTM(56, 384, 2, batch_first=True, bidirectional=True)
    lstm.load_state_dict({k[len("vertice_map_reverse_lstm."):]: v for k, v in sd.items() if k.startswith("vertice_map_reverse_lstm.")})
    l1, l2 = torch.nn.Linear(768, 768), torch.nn.Linear(768, V)
    l1.load_state_dict({"weight": sd["vertice_map_reverse.0.weight"], "bias": sd["vertice_map_reverse.0.bias"]})
    l2.load_state_dict({"weight": sd["vertice_map_reverse.2.weight"], "bias": sd["vertice_map_reverse.2.bias"]})
    mods = [m.cuda().to(dtype).eval() for m in (lstm, l1, l2)]

    def run(x, templ, full=True):
        y, _ = mods[0](x.to(dtype))
        if not full:
            return y
        return mods[2](torch.nn.functional.leaky_relu(mods[1](y), 0.2)) + templ.to(dtype)[:, None]
    return run


def main():
    trace = "--trace" in sys.argv
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else "profiles/speaker_head.txt"
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    lines = ["# tools/bench_speaker.py on %s; ms, median (min .. max) of 5 device-event timings after 2 warm-up calls" % torch.cuda.get_device_name(0),
             "# head = 2 x bidirectional LSTM(384) + Linear(768,768) + LeakyReLU + Linear(768,V) + template; L = T - 1 frames"]
    sds = {V: weights.synth_state_dict([e for e in weights.emoca_converter_spec(V) if e[2] != "unused"], 1) for V in (V_FULL, 8)}
    for mode, mname in ((L.MODE_PARITY_F32, "f32"), (L.MODE_PERF_BF16, "bf16")):
        engs = {}
        for V in (V_FULL, 8):
            engs[V] = Engine(dev, mode, "speaker", mesh_dim=V)
            engs[V].load_state_dict(sds[V])
        th = torch_head(sds[V_FULL], V_FULL, torch.float32 if mode == L.MODE_PARITY_F32 else torch.bfloat16)
        for B, T in SHAPES:
            if trace and B == 64:
                continue
            Lf = T - 1
            x = torch.randn(B, Lf, 56, device=dev)
            templ = torch.randn(B, V_FULL, device=dev)
            out = torch.empty(B, Lf, V_FULL, device=dev)
            t8 = torch.zeros(B, 8, device=dev)
            cases = [("head V=70110 group", lambda: engs[V_FULL].mesh_head(x, templ, out=out)),
                     ("head V=70110 safe ", lambda: engs[V_FULL].mesh_head(x, templ, safe=True, out=out)),
                     ("lstm+lin1   group", lambda: engs[8].mesh_head(x, t8)),
                     ("lstm+lin1   safe ", lambda: engs[8].mesh_head(x, t8, safe=True)),
                     ("torch head V=70110", lambda: th(x, templ)),
                     ("torch nn.LSTM only", lambda: th(x, templ, full=False))]
            for name, fn in cases:
                if trace:
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
            del out, templ
            torch.cuda.empty_cache()
        faults = sum(e.lstm_faults() for e in engs.values())
        lines.append("%-4s lstm faults: %d" % (mname, faults))
        print(lines[-1], flush=True)
    if not trace:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
