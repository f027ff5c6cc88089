"""CPU: dimx.mymetrics.print_biwi_metrics / compute_biwi_metrics against what the reference's print_biwi_metrics returned
(tests/golden/biwi_metrics.json, written by tests/golden/make_golden_biwi_metrics.py; the meshes are regenerated here from
dimx.prng), the readers of the reference's files, and the closed sets of the device path: no CPU fallback, no unknown backend.

Tolerances.  float64 inputs: 1e-12 relative -- a vectorised float64 restatement does the reference's arithmetic (sums of 3 terms,
np.std, np.mean, np.max).  float32 inputs: 1e-5 relative -- float32 results sit about 1e-7 from the float64 value and a
vectorised form is free to sum in another order.  lve is relative to itself; fdd, a difference that may be near 0, is relative to
the stored mean over clips of (sigma_gt + sigma_pred)."""
import json
import os
import pickle
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_biwi_metrics as gen  # noqa: E402

from dimx import mymetrics  # noqa: E402

with open(os.path.join(HERE, "golden", "biwi_metrics.json")) as _f:
    GOLD = json.load(_f)
TOL = {"float64": 1e-12, "float32": 1e-5}


def test_golden_describes_the_generator():
    mouth, upper = gen.make_maps()
    assert GOLD["mouth_map"] == mouth and GOLD["upper_map"] == upper and GOLD["n_vert"] == gen.NV and GOLD["seed"] == gen.SEED
    assert [tuple(f) for f in GOLD["frames"]] == gen.FRAMES and GOLD["file_names"] == gen.NAMES
    assert len(mouth) == 257 and len(set(mouth)) == 256 and len(upper) == 131 and len(set(upper)) == 130
    assert any(tp > tg for tg, tp in gen.FRAMES) and len({n.split("_")[0] for n in gen.NAMES}) == 2
    assert [c["name"] for c in GOLD["cases"]] == [c["name"] for c in gen.CASES]


@pytest.mark.parametrize("case", GOLD["cases"], ids=[c["name"] for c in GOLD["cases"]])
def test_print_biwi_metrics_matches_the_reference(case, capsys):
    y_true, y_pred, names, templates = gen.clips(case)
    assert y_true[0].dtype == np.dtype(case["dtype"])
    lve, fdd = mymetrics.print_biwi_metrics(y_true, y_pred, names, templates=templates, mouth_map=GOLD["mouth_map"],
                                            upper_map=GOLD["upper_map"])
    printed = capsys.readouterr().out.splitlines()
    tol = TOL[case["dtype"]]
    e_lve = abs(float(lve) - case["lve"]) / abs(case["lve"])
    e_fdd = abs(float(fdd) - case["fdd"]) / case["fdd_scale"]
    print("%s: lve %.17g (golden %.17g, rel %.3g)  fdd %.17g (golden %.17g, rel to scale %.3g)"
          % (case["name"], lve, case["lve"], e_lve, fdd, case["fdd"], e_fdd))
    assert e_lve <= tol and e_fdd <= tol
    # the reference computes in the arrays' dtype, and so does the restatement: nothing is upcast
    assert [type(lve).__name__, type(fdd).__name__] == case["result_dtype"]
    # the two printed lines, in the reference's format
    assert printed == ["Lip Vertex Error: {:.4e}".format(lve), "FDD: {:.4e}".format(fdd)]
    if case["dtype"] == "float64":
        assert printed == case["printed"]


def test_compute_biwi_metrics_per_clip_arrays():
    case = GOLD["cases"][0]
    y_true, y_pred, names, templates = gen.clips(case)
    m = mymetrics.compute_biwi_metrics(y_true, y_pred, names, templates, GOLD["mouth_map"], GOLD["upper_map"])
    assert [len(f) for f in m["frame_max"]] == [tg for tg, _ in gen.FRAMES] and m["frames"].tolist() == [tg for tg, _ in gen.FRAMES]
    assert m["lve"] == np.mean(np.concatenate(m["frame_max"]))        # frames weigh equally, not clips
    assert abs(m["fdd"] - np.mean(m["sigma_gt"] - m["sigma_pred"])) <= 1e-15 * m["fdd_scale"]
    assert abs(m["fdd_scale"] - case["fdd_scale"]) <= 1e-12 * case["fdd_scale"]
    # a per-clip template list is the dict looked up by subject
    per_clip = [templates[n.split("_")[0]] for n in names]
    m2 = mymetrics.compute_biwi_metrics(y_true, y_pred, None, per_clip, GOLD["mouth_map"], GOLD["upper_map"])
    assert m2["lve"] == m["lve"] and m2["fdd"] == m["fdd"]


def test_one_frame_clip_has_zero_sigma_and_nv_comes_from_the_data():
    rng = np.random.default_rng(0)
    gt, pred = rng.standard_normal((1, 97 * 3)), rng.standard_normal((3, 97 * 3))
    m = mymetrics.compute_biwi_metrics([gt], [pred], ["F2_x"], None, [5, 5, 96], [0, 7])
    assert m["sigma_gt"][0] == 0.0 and m["sigma_pred"][0] == 0.0 and m["fdd"] == 0.0
    d = ((gt[0].reshape(97, 3) - pred[0].reshape(97, 3)) ** 2).sum(1)
    assert m["lve"] == max(d[5], d[96])


def test_readers_round_trip_and_defaults_come_from_the_reference_paths(tmp_path, monkeypatch, capsys):
    case = GOLD["cases"][0]
    y_true, y_pred, names, templates = gen.clips(case)
    regions = tmp_path / "data" / "CodeTalker" / "BIWI" / "regions"
    regions.mkdir(parents=True)
    (tmp_path / "data" / "BIWI_data").mkdir()
    (tmp_path / "work").mkdir()
    (regions / "lve.txt").write_text(", ".join(str(i) for i in GOLD["mouth_map"]))
    (regions / "fdd.txt").write_text(", ".join(str(i) for i in GOLD["upper_map"]))
    with open(tmp_path / "data" / "BIWI_data" / "templates.pkl", "wb") as f:
        pickle.dump({s: v.reshape(-1, 3) for s, v in templates.items()}, f, protocol=2)
    assert mymetrics.read_region_map(str(regions / "lve.txt")) == GOLD["mouth_map"]
    assert mymetrics.read_region_map(str(regions / "fdd.txt")) == GOLD["upper_map"]
    back = mymetrics.read_biwi_templates(str(tmp_path / "data" / "BIWI_data" / "templates.pkl"))
    assert sorted(back) == sorted(templates) and all(np.array_equal(back[s].reshape(-1), templates[s].reshape(-1)) for s in back)
    monkeypatch.chdir(tmp_path / "work")
    lve, fdd = mymetrics.print_biwi_metrics(y_true, y_pred, names)      # everything read from ../data/...
    capsys.readouterr()
    assert abs(lve - case["lve"]) <= 1e-12 * case["lve"] and abs(fdd - case["fdd"]) <= 1e-12 * case["fdd_scale"]


def test_fewer_predicted_than_true_frames_raises():
    gt, pred = np.zeros((4, 30)), np.zeros((3, 30))
    with pytest.raises(ValueError):
        mymetrics.compute_biwi_metrics([gt], [pred], ["F2_x"], None, [0], [1])


def test_unknown_mesh_metric_backend_raises():
    from dimx import x_engine_pt
    with pytest.raises(ValueError):
        x_engine_pt.evaluate_mesh_epoch_biwi(torch.nn.Identity(), [], torch.device("cpu"), [0], [1], backend="bogus")


def test_op_mesh_metrics_on_cpu_tensors_raises():
    from dimx import engine, lib      # raised before the library is loaded: no build is needed here
    y = torch.zeros(1, 4, 30)
    with pytest.raises(lib.DimxError):
        engine.op_mesh_metrics(y, y, [4], None, [0], [1])
    from dimx import metrics
    with pytest.raises(lib.DimxError):
        metrics.BiwiMeshMetrics([0], [1]).update(y, y, [4], None)
