"""The reference's stage-1 driver (code/train_vq.py:107-170, 173-226) on the HIP training step: the listener motion VQ-VAE
(dimx.models.VQAutoEncoder) trained with AdamW (lr cfg.base_lr, torch's default weight decay 0.01, no clipping), optional
StepLR / poly-lr, train and validation meters (rec / quant / perplexity), validation every epoch on the inference engine
(model.eval(): no dropout), and the best validation reconstruction loss saved as {'state_dict': ...} at
<save_path>/model/model.pth.tar -- the file SLMFT(vq_listener_ckpt=...) / SLM(vq_listener_ckpt=...) load.  Forward, backward
and AdamW run on the hand-written HIP kernels (dimx.train_hip.VqHipTrainer).

Clips of one batch share one length (no padding in the VQ loop): without ViCo files the driver makes synthetic listener clips
of --max-len frames; with them it runs the reference's batch size 1.

    python examples/train_vq.py [--config dimx/config.yaml] [--epochs 2] [--clips 64] [--max-len 120] [KEY VALUE ...]
    (KEY VALUE: base_lr, batch_size, epochs, StepLR, step_size, gamma, poly_lr, power, quant_loss_weight, dropout, save_path, ...)
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dimx  # noqa: E402,F401
from dimx import config as dcfg  # noqa: E402
from dimx import lib  # noqa: E402
from dimx.dataset.data_loader import get_vico_dataloaders  # noqa: E402
from dimx.models import get_model  # noqa: E402
from dimx.train_hip import VqHipTrainer  # noqa: E402

# the TRAIN / LOSS sections of the reference's code/config.yaml that this loop reads
TRAIN_DEFAULTS = {"base_lr": 1e-4, "batch_size": 1, "epochs": 2, "StepLR": False, "step_size": 20, "gamma": 0.5,
                  "poly_lr": False, "power": 0.9, "quant_loss_weight": 1.0, "dropout": 0.1, "seed": 20260928,
                  "save_path": "RUN/vq", "save_freq": 1, "print_freq": 10, "numeric_mode": "f32"}


class AverageMeter:
    def __init__(self):
        self.sum, self.count = 0.0, 0

    def update(self, v, n=1):
        self.sum += float(v) * n
        self.count += n

    @property
    def avg(self):
        return self.sum / max(self.count, 1)


def poly_learning_rate(base_lr, curr_iter, max_iter, power=0.9):
    """reference code/base/utilities.py"""
    return base_lr * (1 - float(curr_iter) / max_iter) ** power


def listener_batches(loader):
    for batch in loader:
        v_l, lens = batch[1], batch[2]
        if min(lens) != max(lens):
            raise ValueError("the VQ-VAE step takes clips of one length per batch (got %s): use batch_size 1" % (lens,))
        yield v_l


def calc_vq_loss(pred, target, quant_loss, quant_loss_weight=1.0):
    """reference code/metrics/loss.py:6-11 (validation; the training step computes it inside the HIP step)"""
    rec = torch.nn.functional.l1_loss(pred, target)
    return quant_loss.mean() * quant_loss_weight + rec, [rec, quant_loss.mean()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default=dcfg.DEFAULT_CONFIG)
    ap.add_argument("--epochs", type=int, default=None)
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--max-len", type=int, default=120)
    ap.add_argument("opts", nargs=argparse.REMAINDER, help="KEY VALUE overrides")
    args = ap.parse_args()
    cfg = dcfg.load_cfg_from_cfg_file(args.config)
    for k, v in TRAIN_DEFAULTS.items():
        cfg.setdefault(k, v)
    if args.opts:
        cfg = dcfg.merge_cfg_from_list(cfg, args.opts)
    if args.epochs is not None:
        cfg.epochs = args.epochs
    device = torch.device("cuda:0")
    torch.cuda.set_device(device)
    mode = lib.MODE_PERF_BF16 if cfg.numeric_mode == "bf16" else lib.MODE_PARITY_F32
    model = get_model(cfg, numeric_mode=mode).to(device)
    trainer = VqHipTrainer(model, lr=cfg.base_lr, dropout=cfg.dropout, seed=cfg.seed, quant_loss_weight=cfg.quant_loss_weight)

    have_vico = os.path.isdir("../data/vico_processed_30fps")
    if not have_vico:
        print("no listener data under ../data: SYNTHETIC clips -- the losses below say nothing about the real task")
        dataset = get_vico_dataloaders(batch_size=cfg.batch_size, synthetic={"n_clips": args.clips, "max_len": args.max_len,
                                                                             "min_len": args.max_len, "seed": cfg.seed})
    else:
        dataset = get_vico_dataloaders(batch_size=1)
    train_loader, val_loader = dataset["train"], dataset["valid"]
    max_iter = cfg.epochs * len(train_loader)
    best_val = float("inf")
    sav_dir = os.path.join(cfg.save_path, "model")
    for epoch in range(cfg.epochs):
        # ---------------- train (model.train(): dropout on)
        meters = [AverageMeter() for _ in range(3)]
        t0 = time.time()
        for i, v_l in enumerate(listener_batches(train_loader)):
            current_iter = epoch * len(train_loader) + i + 1
            trainer.train_step(v_l.to(device, non_blocking=True))
            d = trainer.last
            for m, key in zip(meters, ("rec_loss", "quant_loss", "perplexity")):
                m.update(d[key].item(), 1)
            if cfg.poly_lr:
                trainer.lr = poly_learning_rate(cfg.base_lr, current_iter, max_iter, power=cfg.power)
            if (i + 1) % cfg.print_freq == 0:
                print("Epoch: [%d/%d][%d/%d] rec %.4f quant %.4f lr %.2e" % (epoch + 1, cfg.epochs, i + 1, len(train_loader),
                                                                             meters[0].avg, meters[1].avg, trainer.lr))
        if cfg.StepLR and (epoch + 1) % cfg.step_size == 0:
            trainer.lr *= cfg.gamma
        print("TRAIN Epoch: %d loss_train: %.6f quant_train: %.6f pp_train: %.3f (%.1f s)"
              % (epoch + 1, meters[0].avg, meters[1].avg, meters[2].avg, time.time() - t0))
        # ---------------- validate (model.eval() under no_grad: the inference engine on the trained weights)
        trainer.sync_to_model()
        model.eval()
        vm = [AverageMeter() for _ in range(3)]
        with torch.no_grad():
            for v_l in listener_batches(val_loader):
                v_l = v_l.to(device)
                out, quant_loss, info = model(v_l)
                _, (rec, quant) = calc_vq_loss(out, v_l, quant_loss, cfg.quant_loss_weight)
                for m, v in zip(vm, (rec, quant, info[0])):
                    m.update(v.item(), 1)
        model.train()
        print("VAL Epoch: %d loss_val: %.6f quant_val: %.6f pp_val: %.3f" % (epoch + 1, vm[0].avg, vm[1].avg, vm[2].avg))
        if (epoch + 1) % cfg.save_freq == 0 and vm[0].avg < best_val:
            best_val = vm[0].avg
            os.makedirs(sav_dir, exist_ok=True)
            torch.save({"state_dict": model.state_dict()}, os.path.join(sav_dir, "model.pth.tar"))
            print("saved %s (val rec %.6f)" % (os.path.join(sav_dir, "model.pth.tar"), best_val))


if __name__ == "__main__":
    main()
