"""One fine-tuning step of the DIM-Speaker model (SpeakerHipTrainer: csrc/train.hip spk_run, csrc/train_spk.hip) on one GPU:
    python tools/bench_speaker_train.py [out.txt]     # event-timed table -> profiles/speaker_train.txt by default
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_speaker_train.py --trace   # one f32 step at T = 300, for a kernel trace
Rows, at B = 1, T in {100, 300}, V = 70110, both numeric modes, with and without the mouth metric (the mesh head over V):
  * step: forward + backward + clip + AdamW;    * fwd+bwd alone;
  * torch: the same step on the PyTorch-autograd checker (dimx.train.speaker_loss) + clip_grad_norm_ + torch.optim.AdamW on the
    same GPU (f32; the comparison row; no mouth metric: it has no gradient and the checker does not compute it).
The frozen listener VQ-VAE's codes are computed once outside every row (they are the step's input).  Median (min .. max) of 5
device-event timings after 2 warm-up calls, the method of tools/bench_converter_train.py."""
import statistics
import sys

import torch

sys.path.insert(0, ".")
import dimx  # noqa: E402,F401
from dimx import lib as L  # noqa: E402
from dimx import train as Tr  # noqa: E402
from dimx.seq2seq_pretrain import SpeakerSLMFT  # noqa: E402
from dimx.train_hip import SpeakerHipTrainer  # noqa: E402

V = 70110
FRAMES = (100, 300)


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


def torch_step(model):
    """the checker's step on a detached copy of the trained tensors (the module itself is left alone)"""
    P = {k: v.detach().clone() for k, v in model.state_dict().items() if not k.startswith(("vertice_map", "squasher", "encoder_"))}
    names = [n for n, _ in Tr.speaker_trainable_parameters(model)]
    params = [P[n].requires_grad_(True) for n in names]
    opt = torch.optim.AdamW(params, lr=1e-5)
    pe = P["speaker_vq.decoder.decoder_pos_embedding.pe"]

    def run(xe, xa, mask, z, ids):
        opt.zero_grad()
        loss, _ = Tr.speaker_loss(P, model.s2s, model.vq_dims, xe, xa, mask, z, pe, speaker_ids=ids)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(params, 1.0)
        opt.step()
        return loss
    return run


def main():
    trace = "--trace" in sys.argv
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else "profiles/speaker_train.txt"
    dev = torch.device("cuda:0")
    lines = ["# tools/bench_speaker_train.py on %s; ms, median (min .. max) of 5 device-event timings after 2 warm-up calls" % torch.cuda.get_device_name(0),
             "# step = forward + backward + clip 1.0 + AdamW of SpeakerSLMFT's fine-tuning step (decoder_joint 4 x 1152, speaker VQ-VAE decoder); B = 1, V = %d" % V]
    mouth_map = list(range(0, V // 3, 5))
    ids = torch.tensor([3], device=dev)
    for mode, mname in ((L.MODE_PARITY_F32, "f32"), (L.MODE_PERF_BF16, "bf16")):
        model = SpeakerSLMFT(mesh_dim=V, numeric_mode=mode).to(dev)
        plain = SpeakerHipTrainer(model, mouth_map=None)
        mouth = SpeakerHipTrainer(model, mouth_map=mouth_map)
        th = torch_step(model) if mode == L.MODE_PARITY_F32 else None
        for T in (FRAMES if not trace else (300,)):
            torch.manual_seed(T)
            xe = torch.randn(1, T, 56, device=dev)
            xa = torch.randn(1, T, 768, device=dev)
            xt = 0.1 * torch.randn(1, V, device=dev)
            xv = xt[:, None] + 0.01 * torch.randn(1, T, V, device=dev)
            mask = torch.ones(1, T, dtype=torch.bool, device=dev)
            with torch.no_grad():
                _, z = model.forward_vq(None, xe, mask)
            cases = [("step      no mouth  ", lambda: plain.train_step(None, xe, xa, mask, None, speaker_ids=ids, z=z)),
                     ("fwd+bwd   no mouth  ", lambda: plain.forward_backward(None, xe, xa, mask, None, speaker_ids=ids, z=z)),
                     ("step      with mouth", lambda: mouth.train_step(xv, xe, xa, mask, xt, speaker_ids=ids, z=z)),
                     ("fwd+bwd   with mouth", lambda: mouth.forward_backward(xv, xe, xa, mask, xt, speaker_ids=ids, z=z))]
            if th is not None:
                cases.append(("torch autograd+AdamW", lambda: th(xe, xa, mask, z, ids)))
            for name, fn in cases:
                if trace:
                    if mode == L.MODE_PARITY_F32 and name.startswith("step      no mouth"):
                        fn()
                        torch.cuda.synchronize()
                    continue
                med, lo, hi = timed(fn)
                lines.append("%-4s B=1 T=%-3d  %-20s %9.3f  (%.3f .. %.3f)" % (mname, T, name, med, lo, hi))
                print(lines[-1], flush=True)
        del plain, mouth, model, th
        torch.cuda.empty_cache()
        if trace:
            break
    if not trace:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
