"""Prompted evaluation: examples/test_s2s_pretrain.py (the reference's code/test_s2s_pretrain.py on the dimx drop-ins) with one
more argument, --prompt-frames N: every generation continues the clip's first N ground-truth listener frames instead of
starting from frame 0 alone (SLMFT.forward(prompt_frames=N); the reference edit is decoder_joint.generate(z_l[:, :N],
seq_len=T-N, ...)).  Selection and metrics stay over the whole clip.  Without the ViCo files / checkpoint it runs on synthetic
clips and weights.

    python examples/continue_s2s_pretrain.py --prompt-frames 30 [--clips 32] [--batch 8] [--beam 10] [--bf16] [--ckpt best_vico_causal.pt]
                                            [--select {fd,likelihood,consensus}] [--consensus-distance {fd,l2}]
                                            [--lookahead L [--window-prefill]]

--select likelihood keeps the continuation the model itself scores highest (the log-likelihood of its sampled tokens past the
prompt) instead of the one nearest to the ground truth: beyond the prompt a deployed continuation has no ground truth to select with.
"""
import argparse
import os
import pickle
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dimx  # noqa: E402,F401
from dimx import lib as L  # noqa: E402
from dimx.dataset.data_loader import get_vico_dataloaders  # noqa: E402   (was: from dataset.data_loader import ...)
from dimx.mymetrics import print_metrics, print_metrics_full  # noqa: E402 (was: from mymetrics import ...)
from dimx.seq2seq_pretrain import SLMFT  # noqa: E402                     (was: from seq2seq_pretrain import SLMFT)
from dimx import sampling  # noqa: E402
from dimx.x_engine_pt import evaluate_test_epoch  # noqa: E402            (was: from x_engine_pt import ...)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--beam", type=int, default=10)
    ap.add_argument("--max-len", type=int, default=300)
    ap.add_argument("--bf16", action="store_true")
    ap.add_argument("--ckpt", default="best_vico_causal.pt")
    ap.add_argument("--out", default="l2l_listener_continuations.pkl")
    ap.add_argument("--prompt-frames", type=int, default=30,
                    help="continue the first N ground-truth listener frames of every clip instead of starting from frame 0 alone")
    ap.add_argument("--select", choices=("fd", "likelihood", "consensus"), default="fd",
                    help="best-of-N by Frechet distance to the ground truth (the reference's protocol), by the model's own log-likelihood, "
                         "or by consensus: the try nearest to the clip's other tries (minimum Bayes risk; no ground truth either)")
    ap.add_argument("--consensus-distance", choices=("fd", "l2"), default="fd",
                    help="the distance between tries of --select consensus: the protocol's Frechet distance or the mean squared difference")
    ap.add_argument("--decode", choices=("sample", "beam"), default="sample",
                    help="the tries of a clip: --beam independent samples (the reference's protocol; its 'beam' is a number of tries) or "
                         "the final hypotheses of one beam search of --beam-width (deterministic)")
    ap.add_argument("--beam-width", type=int, default=None, help="hypotheses of --decode beam (1 < W <= 10; default: --beam)")
    ap.add_argument("--lookahead", type=int, default=None,
                    help="online generation: the token of frame t+1 is drawn from the speaker frames below t + 2 + L (0: up to the frame being "
                         "produced, < 0: a reaction delay, > 0: a look-ahead buffer; default: the whole clip is visible, as in the reference)")
    ap.add_argument("--window-prefill", action="store_true",
                    help="with --lookahead: prefill the prompt in one teacher-forced pass under the window instead of running it through "
                         "forced decode steps (the same definition through other kernels)")
    ap.add_argument("--guidance", type=float, default=None,
                    help="classifier-free guidance scale s (dimx.guidance): every step samples from cond + (s - 1) * (cond - uncond); the prompt "
                         "then runs through forced decode steps.  One sample per clip and pass, --select fd only")
    ap.add_argument("--kv8", action="store_true",
                    help="FP8 cross-attention K/V (dimx.kv8): the context K / V are quantised once per generation and the decode steps stream "
                         "the codes.  One sample per clip and pass, --select fd only")
    ap.add_argument("--self-kv8", action="store_true",
                    help="FP8 self-attention K/V caches (dimx.kv8.self_step): every decode step quantises its k / v row and attends over the "
                         "codes.  Any number of samples per clip; not with --decode beam or --guidance")
    ap.add_argument("--kv8-samples", action="store_true",
                    help="FP8 cross-attention K/V for the batched best-of-N pass (dimx.kv8.attention_rows): the tries of a clip stay one "
                         "generation whose multi-query cross attention reads the codes.  Every --select, with --self-kv8; not with "
                         "--decode beam or --guidance")
    ap.add_argument("--beam-kv8", choices=("self", "cross", "both"), default=None,
                    help="FP8 K/V caches for --decode beam (dimx.kv8.reorder): the self caches, the cross K/V, or both.  Every --select; "
                         "not with --guidance")
    sampling.add_filter_arguments(ap)     # --filter {top_k,top_p,min_p,top_a} --filter-thres --filter-k --min-p --top-a-pow --top-a-ratio
    args = ap.parse_args()
    if args.window_prefill and args.lookahead is None:
        ap.error("--window-prefill applies to --lookahead: offline, a prompt is always prefilled")
    sampler = sampling.filter_from_args(args)
    if sampler:
        print("sampler filter: %s %s" % (sampler["filter_logits_fn"], sampler["filter_kwargs"] or "(defaults)"))

    crank = 0
    device = torch.device("cuda:{}".format(crank))
    model = SLMFT(numeric_mode=L.MODE_PERF_BF16 if args.bf16 else L.MODE_PARITY_F32).to(device)
    if os.path.isfile(args.ckpt):
        model.load_state_dict(torch.load(args.ckpt, map_location="cpu"))
    else:
        print("no checkpoint at %s: synthetic weights" % args.ckpt)

    have_vico = os.path.isdir("../data/vico_processed_30fps")
    if not have_vico:
        print("no ViCo data under ../data: SYNTHETIC clips -- the metrics below are not ViCo results")
    dataset = get_vico_dataloaders(batch_size=args.batch,
                                   synthetic=None if have_vico
                                   else {"n_clips": args.clips, "max_len": args.max_len, "min_len": 24})
    val_loader = dataset["valid"]

    t0 = time.time()
    y_true, y_pred, x, data_ids = evaluate_test_epoch(model, val_loader, device, beam_size=args.beam,
                                                        prompt_frames=args.prompt_frames, select=args.select,
                                                        consensus_distance=args.consensus_distance, decode=args.decode,
                                                        beam_width=args.beam_width, lookahead=args.lookahead,
                                                        window_prefill=args.window_prefill, guidance=args.guidance, kv8=args.kv8, self_kv8=args.self_kv8, kv8_samples=args.kv8_samples,
                                                        beam_kv8=args.beam_kv8, **sampler)
    torch.cuda.synchronize()
    print("generated %d clips x best-of-%d (selected by %s) in %.2f s" % (len(y_true), args.beam, args.select, time.time() - t0))
    print_metrics(y_true, y_pred, x)
    print_metrics_full(y_true, y_pred, x)

    d = {"y_true": y_true, "y_pred": y_pred, "data_ids": data_ids, "synthetic": not have_vico}
    with open(args.out, "wb") as f:
        pickle.dump(d, f, protocol=pickle.HIGHEST_PROTOCOL)


if __name__ == "__main__":
    main()
