"""The reference's BIWI evaluation driver (code/test_biwi.py) on the dimx drop-ins: the imports are the only lines that
change.  The BIWI data set and the reference's checkpoints are not available, so it runs on a synthetic BIWI-shaped loader
(batches ``(audio [B,T,768], vertices [B,T,V], template [B,V], emoca [B,T,56], file names)``) and synthetic weights unless
``--ckpt`` exists.  Saves ``<out>/gt/<id>.npy`` and ``<out>/pred/<id>.npy`` like the reference.

    python examples/test_biwi.py --synthetic [--clips 4] [--frames 60] [--mesh-dim 70110] [--beam 50] [--bf16]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dimx  # noqa: E402,F401
from dimx import lib as L  # noqa: E402
from dimx import prng  # noqa: E402
from dimx.seq2seq_pretrain import SpeakerSLMFT  # noqa: E402            (was: from seq2seq_pretrain import SLMFT, SpeakerSLMFT)
from dimx.x_engine_pt import BIWI_SPEAKER_IDS, evaluate_test_epoch_biwi  # noqa: E402   (was: from x_engine_pt import ...)


def synthetic_biwi_loader(n_clips, frames, mesh_dim, batch_size=1, seed=11):
    """Batches shaped like the reference's ``dataset.biwi.get_dataloaders(batch_size=1)['valid']``; file names carry a BIWI
    speaker prefix (``F2_e01.npy``, ...), from which the engine derives the speaker id."""
    names = sorted(BIWI_SPEAKER_IDS)
    batches = []
    for b0 in range(0, n_clips, batch_size):
        nb = min(batch_size, n_clips - b0)
        tag = "biwi.%d" % b0
        templ = torch.from_numpy(prng.normal(seed, tag + ".t", (nb, mesh_dim))) * 0.1
        xe = torch.from_numpy(prng.normal(seed, tag + ".e", (nb, frames, 56)))
        xa = torch.from_numpy(prng.normal(seed, tag + ".a", (nb, frames, 768)))
        xv = templ[:, None, :] + 0.01 * torch.from_numpy(prng.normal(seed, tag + ".v", (nb, frames, mesh_dim)))
        ids = ["%s_e%02d.npy" % (names[(b0 + j) % len(names)], b0 + j) for j in range(nb)]
        batches.append((xa, xv, templ, xe, ids))
    return batches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--synthetic", action="store_true", help="synthetic BIWI-shaped clips (the only loader available)")
    ap.add_argument("--clips", type=int, default=4)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--mesh-dim", type=int, default=70110)
    ap.add_argument("--beam", type=int, default=50)
    ap.add_argument("--bf16", action="store_true")
    ap.add_argument("--ckpt", default="best_model_biwi_finetune1.pt")
    ap.add_argument("--out", default="biwi")
    args = ap.parse_args()
    if not args.synthetic:
        sys.exit("the BIWI loader (reference code/dataset/biwi.py) needs the data set and s3prl, which are not available: "
                 "run with --synthetic")

    crank = 0
    device = torch.device("cuda:{}".format(crank))
    model = SpeakerSLMFT(mesh_dim=args.mesh_dim,
                         numeric_mode=L.MODE_PERF_BF16 if args.bf16 else L.MODE_PARITY_F32).to(device)
    if os.path.isfile(args.ckpt):
        model.load_state_dict(torch.load(args.ckpt, map_location="cpu"))
    else:
        print("no checkpoint at %s: synthetic weights" % args.ckpt)

    test_loader = synthetic_biwi_loader(args.clips, args.frames, args.mesh_dim)
    y_true, y_pred, x, data_ids = evaluate_test_epoch_biwi(model, test_loader, device, beam_size=args.beam)
    gt_save_path = os.path.join(args.out, "gt")
    pred_save_path = os.path.join(args.out, "pred")
    os.makedirs(gt_save_path, exist_ok=True)
    os.makedirs(pred_save_path, exist_ok=True)
    for idx, data_id in enumerate(data_ids):
        data_id = data_id.split(".")[0]
        np.save(os.path.join(gt_save_path, data_id + ".npy"), y_true[idx])
        np.save(os.path.join(pred_save_path, data_id + ".npy"), y_pred[idx])
    print("saved %d clips (SYNTHETIC data: not BIWI results) under %s" % (len(data_ids), args.out))


if __name__ == "__main__":
    main()
