"""The listener test protocol with selection AND metrics in the HIP library: ``evaluate_test_epoch(fd_backend="hip", metrics=acc)``
followed by ``ListenerMetrics(sid=True).print`` in place of print_metrics / print_metrics_full on the host, the two SID lines
included (examples/test_s2s_pretrain.py is the reference's driver on its host path and stays as it is).  Without the ViCo files /
checkpoint it runs on synthetic clips and weights.

    python examples/eval_s2s_pretrain_hip.py [--clips 32] [--batch 8] [--beam 10] [--bf16] [--ckpt best_vico_causal.pt] [--no-sid]
                                            [--select {fd,likelihood,consensus}] [--consensus-distance {fd,l2}]
                                            [--out l2l_listener_predictions.pkl]

--select likelihood keeps, per clip, the try the model itself scores highest (its log-likelihood, csrc/seq_score.hip) instead of the
try nearest to the ground truth: the selection a conversation without a recorded listener allows.  --select consensus keeps the
try with the smallest total distance to the clip's other tries (minimum Bayes risk, csrc/consensus.hip): no ground truth either,
and no preference for the modal, low-motion sequence.  For every selection the
perplexity of the ground-truth listener codes over the epoch is printed (SLMFT.score, teacher-forced).

--lookahead L generates online (dimx.online): the listener token of frame t+1 is drawn from the speaker frames below t + 2 + L only.
The perplexity of the ground-truth codes under that visibility is then printed next to the offline one.
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
from dimx.dataset.data_loader import get_vico_dataloaders  # noqa: E402
from dimx.metrics import ListenerMetrics  # noqa: E402
from dimx.guidance import pmi  # noqa: E402
from dimx.scoring import SeqScores, perplexity  # noqa: E402
from dimx.seq2seq_pretrain import SLMFT  # noqa: E402
from dimx import sampling  # noqa: E402
from dimx.x_engine_pt import _prepare, evaluate_test_epoch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--beam", type=int, default=10)
    ap.add_argument("--max-len", type=int, default=300)
    ap.add_argument("--bf16", action="store_true")
    ap.add_argument("--ckpt", default="best_vico_causal.pt")
    ap.add_argument("--out", default="l2l_listener_predictions.pkl")
    ap.add_argument("--no-sid", action="store_true", help="leave out the two SID lines")
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
    ap.add_argument("--guidance", type=float, default=None,
                    help="classifier-free guidance scale s: every step samples from cond + (s - 1) * (cond - uncond), uncond being the decoder "
                         "without the speaker context (1: the model; > 1: more reactive to the speaker; 0: the listener's prior).  One sample "
                         "per clip and pass, --select fd only")
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
                    help="FP8 K/V caches for --decode beam (dimx.kv8.reorder): the self caches (codes and scales reordered by parent "
                         "hypothesis), the cross K/V (the hypotheses of a clip read its codes in one launch), or both.  Every --select; "
                         "not with --guidance")
    sampling.add_filter_arguments(ap)     # --filter {top_k,top_p,min_p,top_a} --filter-thres --filter-k --min-p --top-a-pow --top-a-ratio
    args = ap.parse_args()
    sampler = sampling.filter_from_args(args)
    if sampler:
        print("sampler filter: %s %s" % (sampler["filter_logits_fn"], sampler["filter_kwargs"] or "(defaults)"))

    device = torch.device("cuda:0")
    model = SLMFT(numeric_mode=L.MODE_PERF_BF16 if args.bf16 else L.MODE_PARITY_F32).to(device)
    if os.path.isfile(args.ckpt):
        model.load_state_dict(torch.load(args.ckpt, map_location="cpu"))
    else:
        print("no checkpoint at %s: synthetic weights" % args.ckpt)
    have_vico = os.path.isdir("../data/vico_processed_30fps")
    if not have_vico:
        print("no ViCo data under ../data: SYNTHETIC clips -- the metrics below are not ViCo results")
    dataset = get_vico_dataloaders(batch_size=args.batch,
                                   synthetic=None if have_vico else {"n_clips": args.clips, "max_len": args.max_len, "min_len": 24})

    acc = ListenerMetrics(sid=not args.no_sid)    # SID on the GPU too (csrc/kmeans_sid.hip): no per-clip list is needed to print
    t0 = time.time()
    y_true, y_pred, x, data_ids = evaluate_test_epoch(model, dataset["valid"], device, beam_size=args.beam, fd_backend="hip", metrics=acc,
                                                        select=args.select, consensus_distance=args.consensus_distance,
                                                        decode=args.decode, beam_width=args.beam_width, lookahead=args.lookahead,
                                                        guidance=args.guidance, kv8=args.kv8, self_kv8=args.self_kv8, kv8_samples=args.kv8_samples,
                                                        beam_kv8=args.beam_kv8, **sampler)
    torch.cuda.synchronize()
    print("generated %d clips x best-of-%d (selected by %s) in %.2f s" % (len(y_true), args.beam, args.select, time.time() - t0))
    parts, parts_online, parts_null = [], [], []
    for batch in dataset["valid"]:      # teacher-forced: what the model thinks of the ground-truth listener codes
        src_s_v, src_s_a, tgt, mask, _, _ = _prepare(batch, device)
        parts.append(model.score(src_s_v, tgt, src_s_a, mask))
        parts_null.append(model.score(src_s_v, tgt, src_s_a, mask, context="null"))   # the same codes without the speaker
        if args.lookahead is not None:  # the same codes with the speaker's future withheld
            parts_online.append(model.score(src_s_v, tgt, src_s_a, mask, lookahead=args.lookahead))
    gt = SeqScores(torch.cat([p.score for p in parts]), torch.cat([p.count for p in parts]))
    print("perplexity of the ground-truth listener codes: %.3f over %d tokens" % (perplexity(gt), int(gt.count.sum())))
    null = SeqScores(torch.cat([p.score for p in parts_null]), torch.cat([p.count for p in parts_null]))
    print("  under the null context: %.3f; mean PMI of the speaker context and these codes: %.4f nats per token"
          % (perplexity(null), float(pmi(gt, null).mean())))
    if parts_online:
        on = SeqScores(torch.cat([p.score for p in parts_online]), torch.cat([p.count for p in parts_online]))
        print("perplexity of the ground-truth listener codes, online with lookahead %d: %.3f (offline %.3f)"
              % (args.lookahead, perplexity(on), perplexity(gt)))
    t0 = time.time()
    acc.print()
    print("metrics printed in %.3f s" % (time.time() - t0))

    d = {"y_true": y_true, "y_pred": y_pred, "data_ids": data_ids, "synthetic": not have_vico}    # what postprocess2emoca reads
    with open(args.out, "wb") as f:
        pickle.dump(d, f, protocol=pickle.HIGHEST_PROTOCOL)


if __name__ == "__main__":
    main()
