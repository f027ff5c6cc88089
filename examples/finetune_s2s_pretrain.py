"""The reference's fine-tuning driver (code/finetune_s2s_pretrain.py:105-143) on the dimx drop-ins: AdamW lr 1e-5,
clip 1.0, frozen VQ-VAEs, evaluate_finetune_epoch + print_metrics after every epoch, best checkpoint by FD sum.
Single process or `python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 examples/finetune_s2s_pretrain.py`
(one process per GPU, one flat gradient all-reduce per step over RCCL; every rank reads its own shard of the clips).
The training step -- forward, backward, clip, AdamW -- runs on the hand-written HIP kernels (dimx.train_hip.HipTrainer);
`--backward autograd` selects the PyTorch-autograd restatement that serves as its checker.

    python examples/finetune_s2s_pretrain.py [--epochs 2] [--clips 64] [--batch 4] [--max-len 120] [--backward hip|autograd]
                                             [--lookahead L]

``--lookahead L`` (listener mode) fine-tunes for ONLINE generation (dimx/online.py): every step trains with the
decoder's cross attention of row t limited to the speaker frames below clamp(t + 2 + L, 1, T), the visibility
``SLMFT.forward(mode='val', lookahead=L)`` generates under.  After each epoch the validation perplexity under that same
visibility (``SLMFT.score(lookahead=L)``) is printed next to the offline one.  The reference's report
(evaluate_finetune_epoch + print_metrics, a teacher-forced pass over the whole context) and the checkpoint rule are unchanged.

``--mode speaker --synthetic`` is the reference's SPEAKER branch (DIM-Speaker): ``SpeakerSLMFT`` under ``train_epoch_biwi`` at
batch size 1 (AdamW lr 1e-5, clip 1.0) on the HIP step ``dimx.train_hip.SpeakerHipTrainer``; every tenth epoch
``evaluate_test_epoch_biwi(beam_size=2)`` and the best model by mean squared vertex error saved as
``best_model_biwi_finetune1.pt`` (what examples/test_biwi.py loads).  The BIWI data set is not available: the clips are the
synthetic BIWI-shaped loader of examples/test_biwi.py.  ``--init`` names a checkpoint to start from (the reference's
``gamma`` / ``beta`` LayerNorm keys are renamed to ``weight`` / ``bias``, the load is non-strict).

    python examples/finetune_s2s_pretrain.py --mode speaker --synthetic [--epochs 20] [--clips 4] [--frames 60] [--mesh-dim 70110]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dimx  # noqa: E402,F401
from dimx import dist as ddist  # noqa: E402
from dimx.dataset.data_loader import get_vico_dataloaders  # noqa: E402
from dimx.mymetrics import print_metrics  # noqa: E402
from dimx.seq2seq_pretrain import SLMFT  # noqa: E402
from dimx.x_engine_pt import evaluate_finetune_epoch, train_epoch  # noqa: E402


def speaker_main(args):
    """the reference's speaker branch on the synthetic BIWI-shaped loader"""
    import numpy as np
    from dimx.seq2seq_pretrain import SpeakerSLMFT
    from dimx.x_engine_pt import evaluate_test_epoch_biwi, train_epoch_biwi
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_biwi import synthetic_biwi_loader
    if not args.synthetic:
        sys.exit("the BIWI loader (reference code/dataset/biwi.py) needs the data set and s3prl, which are not available: "
                 "run with --synthetic")
    device = torch.device("cuda:0")
    torch.cuda.set_device(device)
    model = SpeakerSLMFT(mesh_dim=args.mesh_dim).to(device)
    if args.init:
        sd = torch.load(args.init, map_location="cpu")
        sd = {k.replace(".gamma", ".weight").replace(".beta", ".bias"): v for k, v in sd.items()}
        missing, unexpected = model.load_state_dict(sd, strict=False)
        print("loaded %s: %d keys missing, %d unexpected" % (args.init, len(missing), len(unexpected)))
    # the reference's own lines: train_epoch_biwi maps this AdamW onto the HIP fine-tuning step
    optimizer = torch.optim.AdamW(model.parameters(), lr=1e-5)
    clips = 4 if args.clips == 64 else args.clips
    train_loader = synthetic_biwi_loader(clips, args.frames, args.mesh_dim)
    test_loader = synthetic_biwi_loader(max(1, clips // 2), args.frames, args.mesh_dim, seed=12)
    out = "best_model_biwi_finetune1.pt" if args.out == "best_vico_causal.pt" else args.out
    best = float("inf")
    for epoch in range(args.epochs):
        loss = train_epoch_biwi(model, train_loader, optimizer, device, scheduler=None, clip=1.0, print_freq=100, epoch=epoch,
                                backward="auto" if args.backward == "hip" else args.backward)
        if epoch % 10 == 0:
            y_true, y_pred, _, _ = evaluate_test_epoch_biwi(model, test_loader, device, beam_size=2)
            lve = float(np.mean([np.mean((p - t) ** 2) for p, t in zip(y_pred, y_true)]))
            print("epoch %d: mean loss %.4f, mean squared error of the predicted coefficients %.6f (SYNTHETIC clips: not BIWI results)" % (
                epoch, loss, lve))
            if lve < best:
                best = lve
                torch.save(model.state_dict(), out)
                print("saved %s" % out)


def validation_perplexity(model, loader, device, lookahead=None, context=None):
    """teacher-forced perplexity of the validation clips' own listener codes, offline (lookahead None) or under the visibility of
    an online generation, or under the null context of dimx.guidance (context "null": the decoder without the speaker) (SLMFT.score)"""
    from dimx.scoring import SeqScores, perplexity
    from dimx.x_engine_pt import _prepare
    model.eval()
    score, count = [], []
    for batch in loader:
        src_s_v, src_s_a, tgt, mask, _, _ = _prepare(batch, device)
        sc = model.score(src_s_v, tgt, src_s_a, mask, lookahead=lookahead, context=context)
        score.append(sc.score.cpu())
        count.append(sc.count.cpu())
    return perplexity(SeqScores(torch.cat(score), torch.cat(count))) if score else float("nan")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="listener", choices=["listener", "speaker"],
                    help="listener: SLMFT under train_epoch (the default, as before); speaker: SpeakerSLMFT under train_epoch_biwi")
    ap.add_argument("--synthetic", action="store_true", help="speaker mode: synthetic BIWI-shaped clips (the only loader available)")
    ap.add_argument("--frames", type=int, default=60, help="speaker mode: frames per synthetic clip")
    ap.add_argument("--mesh-dim", type=int, default=70110, help="speaker mode: 3 x vertices of the mesh")
    ap.add_argument("--init", default=None, help="speaker mode: checkpoint to start from (non-strict load)")
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--max-len", type=int, default=120)
    ap.add_argument("--out", default="best_vico_causal.pt")
    ap.add_argument("--backward", default="hip", choices=["hip", "autograd"],
                    help="hip: forward + backward + clip + AdamW on csrc/train*.hip; autograd: the PyTorch restatement (checker)")
    ap.add_argument("--lookahead", type=int, default=None,
                    help="listener mode: fine-tune under the visibility of an online generation with this look-ahead "
                         "(0: the frame being produced and its past; negative: a reaction delay; default: offline, the reference)")
    ap.add_argument("--cond-drop", type=float, default=None,
                    help="listener mode: condition dropout for classifier-free guidance -- every step trains each clip without its speaker "
                         "context with this probability (dimx.guidance.cond_keep); the validation perplexity under the null context is printed "
                         "next to the conditional one")
    args = ap.parse_args()
    if args.mode == "speaker" and args.cond_drop is not None:
        ap.error("--cond-drop applies to --mode listener: the DIM-Speaker step takes no condition dropout")
    if args.mode == "speaker" and args.lookahead is not None:
        ap.error("--lookahead applies to --mode listener: the DIM-Speaker step has no online window")
    if args.mode == "speaker":
        return speaker_main(args)
    rank, world, local = ddist.init_from_env()
    device = torch.device("cuda:{}".format(local))
    torch.cuda.set_device(device)
    model = SLMFT().to(device)
    # the reference's own lines (code/finetune_s2s_pretrain.py:118-119): train_epoch maps this AdamW onto the HIP training step
    optimizer = torch.optim.AdamW(model.parameters(), lr=1e-5)
    have_vico = os.path.isdir("../data/vico_processed_30fps")
    if not have_vico and rank == 0:
        print("no ViCo data under ../data: SYNTHETIC clips -- the numbers below are not ViCo results")
    dataset = get_vico_dataloaders(batch_size=args.batch,
                                   synthetic=None if have_vico else {"n_clips": args.clips, "max_len": args.max_len,
                                                                     "min_len": 24, "seed": 20260928})   # same clips on every rank: the sampler shards them
    best = float("inf")
    for epoch in range(args.epochs):
        loss = train_epoch(model, dataset["train"], optimizer, device, scheduler=None, clip=1.0, print_freq=100,
                           epoch=epoch, log=print if rank == 0 else (lambda *_: None), backward=args.backward,
                           lookahead=args.lookahead, cond_drop=args.cond_drop)
        y_true, y_pred, x, _ = evaluate_finetune_epoch(model, dataset["valid"], device)
        if rank == 0:
            a, b = print_metrics(y_true, y_pred, x)
            print("epoch %d: mean loss %.4f, FD pose %.4f + exp %.4f" % (epoch, loss, a, b))
            if args.lookahead is not None:
                print("epoch %d: validation perplexity under lookahead %d: %.3f (offline: %.3f)" % (
                    epoch, args.lookahead, validation_perplexity(model, dataset["valid"], device, args.lookahead),
                    validation_perplexity(model, dataset["valid"], device)))
            if args.cond_drop is not None:
                print("epoch %d: validation perplexity under the null context: %.3f (conditional: %.3f)" % (
                    epoch, validation_perplexity(model, dataset["valid"], device, context="null"),
                    validation_perplexity(model, dataset["valid"], device)))
            if a + b < best:
                best = a + b
                torch.save(model.state_dict(), args.out)
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
