"""The metrics the reference reports for the speaker side (``print_biwi_metrics``, code/mymetrics.py:122-182; imported by
code/test_biwi.py and code/finetune_s2s_pretrain.py): Lip Vertex Error and FDD of a ``SpeakerSLMFT`` over a BIWI-shaped loader,
computed on the GPU (``dimx.x_engine_pt.evaluate_mesh_epoch_biwi``: one teacher-forced pass per batch, ``dimx_op_mesh_metrics`` on
the meshes where the mesh head left them, one readback at the end).  The BIWI data set and the reference's checkpoints are not
available, so it runs on the synthetic loader of examples/test_biwi.py and synthetic weights unless ``--ckpt`` exists.

    python examples/biwi_metrics.py --synthetic [--clips 4] [--frames 60] [--mesh-dim 70110] [--bf16]
                                    [--mouth-map FILE --upper-map FILE] [--backend hip|reference]

The map files are the reference's ``regions/lve.txt`` / ``regions/fdd.txt`` (``", "``-separated vertex indices); without them
synthetic maps are used (every 5th vertex / every 3rd vertex of the upper half of the index range) and the output says so.
``--backend reference`` copies the meshes to the host and runs ``dimx.mymetrics.compute_biwi_metrics`` (the slow check).
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dimx  # noqa: E402,F401
from dimx import lib as L  # noqa: E402
from dimx.mymetrics import read_region_map  # noqa: E402
from dimx.seq2seq_pretrain import SpeakerSLMFT  # noqa: E402
from dimx.x_engine_pt import evaluate_mesh_epoch_biwi  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--synthetic", action="store_true", help="synthetic BIWI-shaped clips (the only loader available)")
    ap.add_argument("--clips", type=int, default=4)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--mesh-dim", type=int, default=70110)
    ap.add_argument("--bf16", action="store_true")
    ap.add_argument("--ckpt", default="best_model_biwi_finetune1.pt")
    ap.add_argument("--mouth-map", default=None, help="the reference's regions/lve.txt")
    ap.add_argument("--upper-map", default=None, help="the reference's regions/fdd.txt")
    ap.add_argument("--backend", default="hip", choices=["hip", "reference"])
    args = ap.parse_args(argv)
    if not args.synthetic:
        sys.exit("the BIWI loader (reference code/dataset/biwi.py) needs the data set and s3prl, which are not available: "
                 "run with --synthetic")
    from test_biwi import synthetic_biwi_loader

    device = torch.device("cuda:0")
    model = SpeakerSLMFT(mesh_dim=args.mesh_dim,
                         numeric_mode=L.MODE_PERF_BF16 if args.bf16 else L.MODE_PARITY_F32).to(device)
    if os.path.isfile(args.ckpt):
        model.load_state_dict(torch.load(args.ckpt, map_location="cpu"))
    else:
        print("no checkpoint at %s: synthetic weights" % args.ckpt)
    n_vert = args.mesh_dim // 3
    mouth_map = read_region_map(args.mouth_map) if args.mouth_map else list(range(0, n_vert, 5))
    upper_map = read_region_map(args.upper_map) if args.upper_map else list(range(n_vert // 2, n_vert, 3))
    loader = synthetic_biwi_loader(args.clips, args.frames, args.mesh_dim)
    lve, fdd = evaluate_mesh_epoch_biwi(model, loader, device, mouth_map, upper_map, backend=args.backend)
    print('Lip Vertex Error: {:.4e}'.format(lve))
    print('FDD: {:.4e}'.format(fdd))
    print("(SYNTHETIC data%s: not BIWI results)" % ("" if args.mouth_map and args.upper_map else " and SYNTHETIC vertex maps"))
    return lve, fdd


if __name__ == "__main__":
    main()
