"""Generate tests/golden/biwi_metrics.json: what the REFERENCE's print_biwi_metrics (code/mymetrics.py:122-182) returns on
synthetic vertex clips at its hard-coded Nv = 23370.

The reference function is imported from the read-only reference tree and run in a temporary working directory that holds the
files it opens by relative path (``../data/BIWI_data/templates.pkl``, ``../data/CodeTalker/BIWI/regions/{lve,fdd}.txt``).
Only the maps, the seed, the shapes and the returned ``(lve, fdd)`` are stored: a clip of 7 frames is 2 MB, so the meshes are
regenerated on both sides from dimx.prng (``clips(case)`` below, which tests/test_biwi_metrics_cpu.py imports; uniform streams
only: bit-identical on every machine).  ``fdd_scale`` = mean over clips of (sigma_gt + sigma_pred) is what an error of fdd is
relative to (fdd is a difference and may be near 0); the reference does not return it, so it is taken from
dimx.mymetrics.compute_biwi_metrics on the float64 arrays -- a scale, not a checked value.

Cases: three clips with (Tg, Tp) = (5, 5), (2, 4), (7, 7), two subjects, maps of 257 and 131 indices with one duplicate each,
float64 and float32 arrays, with and without a constant offset of 1.0 on the motion.

Run:  python tests/golden/make_golden_biwi_metrics.py
"""
import contextlib
import io
import json
import os
import pickle
import sys
import tempfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import numpy as np

import dimx  # noqa: E402,F401
from dimx import prng  # noqa: E402

SEED = 20261017
NV = 23370
FRAMES = [(5, 5), (2, 4), (7, 7)]                      # (Tg, Tp) per clip
NAMES = ["F2_e01.npy", "M3_e02.npy", "F2_e03.npy"]     # two subjects
CASES = [{"name": "%s_off%g" % (dt, off), "dtype": dt, "offset": off} for dt in ("float64", "float32") for off in (0.0, 1.0)]
OUT = os.path.join(HERE, "biwi_metrics.json")


def make_maps():
    """257 mouth and 131 upper-face indices, unsorted, the last one repeating the first"""
    out = []
    for tag, n in (("mouth", 257), ("upper", 131)):
        draw = prng.integers(SEED, "biwi_metrics.map." + tag, (2 * n,), 0, NV).astype(np.int64).tolist()
        idx = list(dict.fromkeys(draw))[:n - 1]      # distinct, in the order drawn
        assert len(idx) == n - 1
        out.append(idx + [idx[0]])
    return out


def templates(dtype):
    return {s: (0.1 * prng.uniform(SEED, "biwi_metrics.templ." + s, (NV, 3), -1.0, 1.0)).astype(dtype)
            for s in sorted({n.split("_")[0] for n in NAMES})}


def clips(case):
    """-> (y_true, y_pred, file_names, templates) of a case: vertices = template + offset + 0.01 * uniform(-1, 1) motion, built in
    float32 and cast to the case's dtype (every float32 is a float64: both dtypes hold the same values)"""
    tm = templates(np.float32)
    y_true, y_pred = [], []
    for i, ((tg, tp), name) in enumerate(zip(FRAMES, NAMES)):
        t = tm[name.split("_")[0]].reshape(1, NV * 3)
        off = np.float32(case["offset"])
        g = t + off + np.float32(0.01) * prng.uniform(SEED, "biwi_metrics.gt.%d" % i, (tg, NV * 3), -1.0, 1.0)
        p = t + off + np.float32(0.01) * prng.uniform(SEED, "biwi_metrics.pred.%d" % i, (tp, NV * 3), -1.0, 1.0)
        y_true.append(g.astype(case["dtype"]))
        y_pred.append(p.astype(case["dtype"]))
    return y_true, y_pred, list(NAMES), {s: v.astype(case["dtype"]) for s, v in tm.items()}


def main():
    import make_golden
    from dimx.mymetrics import compute_biwi_metrics
    sys.path.insert(0, make_golden.REF)
    cwd = os.getcwd()
    os.chdir(make_golden.REF)
    try:
        import mymetrics as ref_mymetrics
    finally:
        os.chdir(cwd)
    mouth, upper = make_maps()
    results = []
    for case in CASES:
        y_true, y_pred, names, tm = clips(case)
        with tempfile.TemporaryDirectory() as tmp:
            work = os.path.join(tmp, "work")
            regions = os.path.join(tmp, "data", "CodeTalker", "BIWI", "regions")
            os.makedirs(work)
            os.makedirs(regions)
            os.makedirs(os.path.join(tmp, "data", "BIWI_data"))
            with open(os.path.join(tmp, "data", "BIWI_data", "templates.pkl"), "wb") as f:
                pickle.dump({s: v.reshape(NV, 3) for s, v in tm.items()}, f, protocol=2)
            for fn, mp in (("lve.txt", mouth), ("fdd.txt", upper)):
                with open(os.path.join(regions, fn), "w") as f:
                    f.write(", ".join(str(i) for i in mp))
            os.chdir(work)
            try:
                buf = io.StringIO()
                with contextlib.redirect_stdout(buf):
                    lve, fdd = ref_mymetrics.print_biwi_metrics(y_true, y_pred, names)
            finally:
                os.chdir(cwd)
        c64 = dict(case, dtype="float64")
        g64, p64, _, t64 = clips(c64)
        scale = compute_biwi_metrics(g64, p64, names, t64, mouth, upper)["fdd_scale"]
        results.append({"name": case["name"], "dtype": case["dtype"], "offset": case["offset"], "lve": float(lve), "fdd": float(fdd),
                        "result_dtype": [type(lve).__name__, type(fdd).__name__], "fdd_scale": float(scale),
                        "printed": buf.getvalue().splitlines()})
        print(results[-1])
    with open(OUT, "w") as f:
        json.dump({"seed": SEED, "n_vert": NV, "frames": FRAMES, "file_names": NAMES, "mouth_map": mouth, "upper_map": upper,
                   "cases": results}, f, indent=1)
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
