"""The retrieval baselines of the DIM-Listener tables (reference code/baselines.py: "NN audio", "NN motion", "Random") on the GPU:
the training split becomes a dimx.retrieval.RetrievalLibrary (csrc/retrieval.hip), the validation split is evaluated with
``evaluate_baseline_epoch`` and every line of print_metrics / print_metrics_full is printed by ``ListenerMetrics(sid=True)``.

    python examples/baselines.py --synthetic --kind {audio,motion,random} [--k K --select {fd,consensus}] [--consensus-distance {fd,l2}]
                                 [--clips 64] [--batch 16] [--max-len 300] [--strict-len] [--seed 0] [--first N] [--no-sid]

--kind audio: nearest training clip by the cosine similarity of the per-dimension maximum over time of the audio features; --kind
motion: of the mean over time of the speaker motion; --kind random: a randomly drawn training clip (--first 5 reproduces the
checked-in script's ``np.random.randint(0, 5)``).  --k K > 1 retrieves the K nearest clips and keeps one of them: --select fd is the
oracle pick by Frechet distance to the ground truth, --select consensus the clip the rest of the list agrees with most.
Without --synthetic the ViCo files must exist under ../data.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dimx  # noqa: E402,F401
from dimx.dataset.data_loader import get_vico_dataloaders  # noqa: E402
from dimx.metrics import ListenerMetrics  # noqa: E402
from dimx.retrieval import RetrievalLibrary  # noqa: E402
from dimx.x_engine_pt import evaluate_baseline_epoch, fill_retrieval_library  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--synthetic", action="store_true", help="synthetic clips (SyntheticDyadDataset) instead of the ViCo files")
    ap.add_argument("--kind", choices=("audio", "motion", "random"), default="audio")
    ap.add_argument("--k", type=int, default=1, help="retrieve the K nearest training clips (1..16); K > 1 needs --select")
    ap.add_argument("--select", choices=("fd", "consensus"), default=None)
    ap.add_argument("--consensus-distance", choices=("fd", "l2"), default="fd")
    ap.add_argument("--clips", type=int, default=64, help="synthetic clips per split")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--max-len", type=int, default=300)
    ap.add_argument("--strict-len", action="store_true", help="drop clips whose retrieved clip has another length (the reference's == 64 test)")
    ap.add_argument("--seed", type=int, default=0, help="--kind random: seed of the host draw")
    ap.add_argument("--first", type=int, default=None, help="--kind random: draw from the first N training clips only")
    ap.add_argument("--no-sid", action="store_true", help="leave out the two SID lines")
    args = ap.parse_args()

    device = torch.device("cuda:0")
    torch.manual_seed(0)       # the training loader shuffles: the same library order at every run
    if args.synthetic:
        print("SYNTHETIC clips -- the metrics below are not ViCo results")
        # speaker motion drawn, not the constant stream of the ViCo files: a constant stream has one motion descriptor for every
        # clip and no correlation with anything (rpcc would be NaN)
        synthetic = {"n_clips": args.clips, "max_len": args.max_len, "min_len": 24, "vico_like": False}
    else:
        synthetic = None
    data = get_vico_dataloaders(batch_size=args.batch, synthetic=synthetic)
    t0 = time.time()
    library = fill_retrieval_library(RetrievalLibrary("motion" if args.kind == "motion" else "audio"), data["train"], device)
    torch.cuda.synchronize()
    print("library: %d training clips (%s) in %.2f s" % (len(library), args.kind, time.time() - t0))

    acc = ListenerMetrics(sid=not args.no_sid)
    t0 = time.time()
    kw = dict(random_seed=args.seed, random_first=args.first) if args.kind == "random" else dict(k=args.k, select=args.select,
                                                                                                   consensus_distance=args.consensus_distance)
    y_true, y_pred, x, data_ids = evaluate_baseline_epoch(library, data["valid"], device, metrics=acc, strict_len=args.strict_len, **kw)
    torch.cuda.synchronize()
    what = "random" if args.kind == "random" else "NN %s, k=%d%s" % (args.kind, args.k, ", select=%s" % args.select if args.select else "")
    print("baseline %s: %d clips in %.2f s" % (what, len(y_true), time.time() - t0))
    acc.print()


if __name__ == "__main__":
    main()
