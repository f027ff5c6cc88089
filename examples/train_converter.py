"""The reference's converter training driver (code/train_converter.py) on the dimx drop-ins: EmocaConverter's head (a 2-layer
bidirectional LSTM + two Linear layers, 56 EMOCA coefficients -> mesh vertices) trained on the HIP library
(``dimx.train_hip.ConverterHipTrainer``), best validation loss saved as ``best_converter.pt = model.state_dict()`` -- the
file ``SpeakerSLMFT(converter_ckpt=...)`` loads.  The loop, its two printed lines and the checkpoint rule are the reference's;
like the reference the validation loader IS the train loader.  The BIWI data set is not available, so it runs on the synthetic
BIWI-shaped loader of examples/test_biwi.py.

    python examples/train_converter.py --synthetic [--epochs 2] [--clips 4] [--frames 60] [--mesh-dim 70110] [--bf16]
                                       [--safe] [--mouth-map FILE] [--clip 0.0] [--out best_converter.pt]
                                       [--mesh-metrics [--upper-map FILE]]

``--mouth-map FILE``: comma-separated vertex indices (the reference's ``regions/lve.txt``); without it the synthetic run takes
every 5th vertex.  ``--clip``: 0 by default -- the reference passes 1.0 but clips before ``backward()``, i.e. nothing
(see ConverterHipTrainer).  ``--mesh-metrics`` (off by default; without it the output is unchanged) adds one line per epoch: the
validation Lip Vertex Error and FDD of the reference's ``print_biwi_metrics``, from the meshes the validation pass leaves on the
GPU (``dimx.x_engine_pt.evaluate_mesh_epoch``); ``--upper-map FILE`` is the reference's ``regions/fdd.txt``, without it every 3rd
vertex of the upper half of the index range (synthetic)."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def read_mouth_map(path):
    with open(path) as f:
        return [int(i) for i in f.read().replace("\n", " ").split(",") if i.strip()]


def converter_batches(biwi_batches):
    """``(vertices, template, emoca, names)`` batches, the shape of the reference's ``get_dataloaders_convert``, from the
    ``(audio, vertices, template, emoca, names)`` batches of the synthetic BIWI loader"""
    return [(xv, xt, xe, ids) for _, xv, xt, xe, ids in biwi_batches]


def train_epoch(trainer, loader, device, mouth_map=None, clip=0.0, epoch=0, flags=0):
    trainer.clip = clip
    losses = []
    i = -1
    for i, batch in enumerate(loader):
        xv, xt, xe, _ = batch
        loss, _ = trainer.train_step(xv.to(device), xt.to(device), xe.to(device), mouth_map=mouth_map, flags=flags)
        losses.append(float(loss))
    print('Epoch: [{0}][{1}/{2}]\t'
          'Loss {loss_avg:.4f}\t'.format(epoch, i, len(loader), loss_avg=np.mean(losses)))
    return float(np.mean(losses))


def evaluate_epoch(trainer, loader, device, mouth_map=None, flags=0, upper_map=None):
    """mean validation loss; with an ``upper_map`` also ``(lve, fdd)`` of the same meshes (-> (loss, (lve, fdd)))"""
    losses = []

    def mesh_fn(batch):
        xv, xt, xe, _ = batch
        xv, xt = xv.to(device), xt.to(device)
        d, mesh = trainer.evaluate(xv, xt, xe.to(device), mouth_map=mouth_map, flags=flags)
        losses.append(float(d["loss"]))
        return xv, mesh, [xv.shape[1]] * xv.shape[0], xt

    if upper_map is None:
        for batch in loader:
            mesh_fn(batch)
        return float(np.mean(losses))
    from dimx.x_engine_pt import evaluate_mesh_epoch
    mesh = evaluate_mesh_epoch(mesh_fn, loader, mouth_map, upper_map, backend="hip")
    return float(np.mean(losses)), mesh


def fit(trainer, model, train_loader, val_loader, device, num_epochs, out_path, mouth_map=None, clip=0.0, flags=0, upper_map=None):
    """the reference's epoch loop; returns the best validation loss"""
    best = 10000
    print(f'training for {num_epochs} epochs')
    for epoch in range(num_epochs):
        train_epoch(trainer, train_loader, device, mouth_map=mouth_map, clip=clip, epoch=epoch, flags=flags)
        val_loss = evaluate_epoch(trainer, val_loader, device, mouth_map=mouth_map, flags=flags, upper_map=upper_map)
        if upper_map is not None:
            val_loss, (lve, fdd) = val_loss
        print(f'Epoch {epoch} val loss: {val_loss}')
        if upper_map is not None:
            print('Epoch {} val Lip Vertex Error: {:.4e} FDD: {:.4e}'.format(epoch, lve, fdd))
        if val_loss < best:
            best = val_loss
            trainer.sync_to_model()
            torch.save(model.state_dict(), out_path)
    return best


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--synthetic", action="store_true", help="synthetic BIWI-shaped clips (the only loader available)")
    ap.add_argument("--mesh-dim", type=int, default=70110)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--clips", type=int, default=4)
    ap.add_argument("--epochs", type=int, default=1000)
    ap.add_argument("--bf16", action="store_true", help="Linear layers on bf16 operands (the recurrence stays f32)")
    ap.add_argument("--safe", action="store_true", help="the LSTM layers on the no-communication path")
    ap.add_argument("--mouth-map", default=None, help="file of comma-separated mouth vertex indices")
    ap.add_argument("--clip", type=float, default=0.0)
    ap.add_argument("--lr", type=float, default=1e-5)
    ap.add_argument("--out", default="best_converter.pt")
    ap.add_argument("--mesh-metrics", action="store_true", help="print the validation LVE / FDD (dimx_op_mesh_metrics) per epoch")
    ap.add_argument("--upper-map", default=None, help="file of comma-separated upper-face vertex indices (regions/fdd.txt)")
    args = ap.parse_args(argv)
    if not args.synthetic:
        sys.exit("the BIWI loader (reference code/dataset/biwi.py) needs the data set, which is not available: run with --synthetic")

    import dimx  # noqa: F401
    from dimx import lib as L
    from dimx.seq2seq_pretrain import EmocaConverter
    from dimx.train_hip import ConverterHipTrainer
    from test_biwi import synthetic_biwi_loader

    crank = 0
    device = torch.device("cuda:{}".format(crank))
    model = EmocaConverter(mesh_dim=args.mesh_dim, numeric_mode=L.MODE_PERF_BF16 if args.bf16 else L.MODE_PARITY_F32).to(device)
    if args.mouth_map:
        mouth_map = read_mouth_map(args.mouth_map)
    else:
        mouth_map = list(range(0, args.mesh_dim // 3, 5))
    upper_map = None
    if args.mesh_metrics:
        n_vert = args.mesh_dim // 3
        upper_map = read_mouth_map(args.upper_map) if args.upper_map else list(range(n_vert // 2, n_vert, 3))
    trainer = ConverterHipTrainer(model, lr=args.lr, clip=args.clip)

    # batch_size=1, as the reference trains
    train_loader = converter_batches(synthetic_biwi_loader(args.clips, args.frames, args.mesh_dim))
    val_loader = train_loader
    best = fit(trainer, model, train_loader, val_loader, device, args.epochs, args.out, mouth_map=mouth_map, clip=args.clip,
               flags=1 if args.safe else 0, upper_map=upper_map)
    print("best val loss %g -> %s (SYNTHETIC data: not BIWI results)" % (best, args.out))


if __name__ == "__main__":
    main()
