"""GPU: the DIM-Speaker mesh metrics in the HIP library (dimx_op_mesh_metrics, csrc/mesh_metrics.hip) against the host restatement
of the reference's print_biwi_metrics (dimx.mymetrics.compute_biwi_metrics, pinned by tests/golden/biwi_metrics.json) fed float64
copies of the same f32 values, on the valid frames of each clip.

Tolerance: 1e-11 relative on every entry of clip_out and frame_max (sigma_gt / sigma_pred relative to the entry itself), and for the
final FDD relative to mean(sigma_gt + sigma_pred).  Derivation: float64 sums of at most L * n_upper ~ 3e3 non-negative terms carry
at most n * 2^-53 ~ 3e-13, and the sorted copies of the maps the wrapper uploads reorder inside that.  A one-pass E[s^2] - E[s]^2
variance sits near 1e-9 on case D and fails.  Small cases use Nv = 97: rows of 291 floats = 1164 B are no multiple of 16 bytes and
the 12-byte vertex granules fall at every 4-byte phase.  Every measured error is printed before it is asserted."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-11
NV = 97
V = 3 * NV


def _rand_map(seed, n, nv=NV):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, nv, (n,), generator=g).tolist()


def _dup_map(seed, n, nv=NV):
    """n unsorted entries that are sure to repeat a vertex"""
    m = _rand_map(seed, n, nv)
    if n > 1:
        m[-1] = m[0]
    return m


@functools.lru_cache(maxsize=None)
def _case_a():
    """B = 3, L = 9, lens [9, 5, 1]; y_pred has L + 2 frames, y_true is the [:, 1:] view of a [B, L + 1, V] tensor"""
    g = torch.Generator().manual_seed(101)
    B, L = 3, 9
    templ = 0.1 * torch.randn(B, V, generator=g)
    base = templ[:, None] + 0.05 * torch.randn(B, L + 1, V, generator=g)
    pred = templ[:, None] + 0.05 * torch.randn(B, L + 2, V, generator=g)
    return base, pred, templ, [9, 5, 1], _dup_map(1, 40), _dup_map(2, 23)


@functools.lru_cache(maxsize=None)
def _case_a_dev():
    base, pred, templ, lens, mouth, upper = _case_a()
    base_d = base.cuda()
    return base_d[:, 1:], pred.cuda(), templ.cuda(), lens, mouth, upper


_ORACLES = {}     # case -> oracle result: computed once, shared, never modified


def _oracle(y_true, y_pred, lens, templ, mouth, upper):
    """compute_biwi_metrics on float64 copies of the f32 values (CPU tensors in)"""
    from dimx.mymetrics import compute_biwi_metrics
    gts = [y_true[b, :n].double().numpy() for b, n in enumerate(lens)]
    preds = [y_pred[b, :n].double().numpy() for b, n in enumerate(lens)]
    tm = None if templ is None else [templ[b].double().numpy() for b in range(len(lens))]
    return compute_biwi_metrics(gts, preds, None, tm, mouth, upper)


def _oracle_for(key, *inputs):
    if key not in _ORACLES:
        _ORACLES[key] = _oracle(*inputs)
    return _ORACLES[key]


def _rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    den = np.where(want == 0.0, 1.0, np.abs(want))
    return float(np.max(np.abs(got - want) / den)) if got.size else 0.0


def _check(tag, clip, frames, ref, lens, L):
    """every entry of clip_out and frame_max, then the final (lve, fdd), against the oracle; prints, then asserts"""
    clip = clip.cpu().numpy()
    B = len(lens)
    sum_max = np.array([ref["frame_max"][b].sum() for b in range(B)])
    errs = {"sum_max": _rel(clip[:, 0], sum_max), "sigma_gt": _rel(clip[:, 2], ref["sigma_gt"]), "sigma_pred": _rel(clip[:, 3], ref["sigma_pred"])}
    assert clip[:, 1].tolist() == [float(n) for n in lens]
    if frames is not None:
        fr = frames.cpu().numpy()
        assert fr.shape == (B, L)
        errs["frame_max"] = max(_rel(fr[b, :n], ref["frame_max"][b]) for b, n in enumerate(lens))
        assert all((fr[b, n:] == 0.0).all() for b, n in enumerate(lens))
    lve = clip[:, 0].sum() / clip[:, 1].sum()
    fdd = (clip[:, 2] - clip[:, 3]).mean()
    scale = float(ref["fdd_scale"])
    errs["lve"] = _rel(lve, ref["lve"])
    errs["fdd"] = abs(fdd - float(ref["fdd"])) / scale if scale > 0 else abs(fdd - float(ref["fdd"]))
    print("%s: " % tag + "  ".join("%s %.3g" % kv for kv in errs.items()))
    assert all(e <= TOL for e in errs.values()), errs
    return errs


def _run(y_true, y_pred, lens, templ, mouth, upper, want_frames=True):
    from dimx.engine import op_mesh_metrics
    clip, frames = op_mesh_metrics(y_true, y_pred, lens, templ, mouth, upper, want_frames=want_frames)
    torch.cuda.synchronize()
    return clip, frames


def test_case_a_ragged_lengths_strided_views_one_frame_clip():
    base, pred, templ, lens, mouth, upper = _case_a()
    yt, yp, tm, _, _, _ = _case_a_dev()
    assert not yt.is_contiguous() and yp.shape[1] == yt.shape[1] + 2
    clip, frames = _run(yt, yp, lens, tm, mouth, upper)
    ref = _oracle_for("A", base[:, 1:], pred, tuple(lens), templ, tuple(mouth), tuple(upper))
    _check("A", clip, frames, ref, lens, 9)
    assert clip[2, 2].item() == 0.0 and clip[2, 3].item() == 0.0      # the one-frame clip: sigma = 0 exactly
    assert len(set(mouth)) < len(mouth) and len(set(upper)) < len(upper) and mouth != sorted(mouth)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 300])
@pytest.mark.parametrize("which", ["mouth", "upper"])
def test_case_b_map_sizes_across_wave_and_block_boundaries(n, which):
    base, pred, templ, lens, mouth, upper = _case_a()
    yt, yp, tm, _, _, _ = _case_a_dev()
    mp = _dup_map(1000 + n, n)
    mouth, upper = (mp, upper) if which == "mouth" else (mouth, mp)
    clip, frames = _run(yt, yp, lens, tm, mouth, upper)
    ref = _oracle_for(("B", n, which), base[:, 1:], pred, tuple(lens), templ, tuple(mouth), tuple(upper))
    _check("B %s n=%d" % (which, n), clip, frames, ref, lens, 9)


def test_case_c_identical_meshes_and_the_zero_template():
    yt, _, tm, lens, mouth, upper = _case_a_dev()
    clip, frames = _run(yt, yt, lens, tm, mouth, upper)
    assert (frames == 0.0).all() and (clip[:, 0] == 0.0).all()
    assert torch.equal(clip[:, 2], clip[:, 3]) and clip[0, 2].item() > 0.0
    _, yp, _, _, _, _ = _case_a_dev()
    c_none, f_none = _run(yt, yp, lens, None, mouth, upper)
    c_zero, f_zero = _run(yt, yp, lens, torch.zeros_like(tm), mouth, upper)
    assert torch.equal(c_none, c_zero) and torch.equal(f_none, f_zero)


def test_case_d_cancellation():
    g = torch.Generator().manual_seed(104)
    B, L = 2, 9
    yt = 1.0 + 1e-4 * torch.randn(B, L, V, generator=g)
    yp = 1.0 + 1e-4 * torch.randn(B, L, V, generator=g)
    lens, mouth, upper = [9, 9], _dup_map(3, 40), _dup_map(4, 23)
    clip, frames = _run(yt.cuda(), yp.cuda(), lens, None, mouth, upper)
    ref = _oracle_for("D", yt, yp, tuple(lens), None, tuple(mouth), tuple(upper))
    _check("D", clip, frames, ref, lens, L)


def test_case_e_each_half_alone():
    yt, yp, tm, lens, mouth, upper = _case_a_dev()
    full_c, full_f = _run(yt, yp, lens, tm, mouth, upper)
    c, f = _run(yt, yp, lens, tm, [], upper)           # no mouth map: the FDD half is unchanged, the LVE half 0
    assert (c[:, 0] == 0.0).all() and (f == 0.0).all() and torch.equal(c[:, 1:], full_c[:, 1:])
    c, f = _run(yt, yp, lens, tm, mouth, [])           # no upper map
    assert (c[:, 2:] == 0.0).all() and torch.equal(c[:, :2], full_c[:, :2]) and torch.equal(f, full_f)


def test_case_f_real_row_width():
    g = torch.Generator().manual_seed(106)
    nv, L = 23370, 3
    templ = 0.1 * torch.randn(1, 3 * nv, generator=g)
    yt = templ[:, None] + 0.05 * torch.randn(1, L, 3 * nv, generator=g)
    yp = templ[:, None] + 0.05 * torch.randn(1, L, 3 * nv, generator=g)
    mouth, upper = _rand_map(5, 4996, nv), _rand_map(6, 7000, nv)
    mouth[0], upper[0] = nv - 1, nv - 1                # the last vertex of the row
    clip, frames = _run(yt.cuda(), yp.cuda(), [L], templ.cuda(), mouth, upper)
    ref = _oracle_for("F", yt, yp, (L,), templ, tuple(mouth), tuple(upper))
    _check("F", clip, frames, ref, [L], L)


def test_case_g_clip_offset_beyond_32_bits():
    g = torch.Generator().manual_seed(107)
    B, L, stride = 2, 3, 1 << 30
    yt = torch.randn(B, L, V, generator=g)
    yp = torch.randn(B, L, V, generator=g)
    templ = 0.1 * torch.randn(B, V, generator=g)
    lens, mouth, upper = [3, 3], _dup_map(7, 40), _dup_map(8, 23)
    compact = _run(yt.cuda(), yp.cuda(), lens, templ.cuda(), mouth, upper)
    views = []
    for src in (yt, yp):
        buf = torch.empty(stride + L * V, dtype=torch.float32, device="cuda")      # 4 GiB + one clip; only the clips are written
        view = buf.as_strided((B, L, V), (stride, V, 1))
        view.copy_(src.cuda())
        assert view[1].data_ptr() - view[0].data_ptr() == 1 << 32
        views.append(view)
    spread = _run(views[0], views[1], lens, templ.cuda(), mouth, upper)
    assert torch.equal(spread[0], compact[0]) and torch.equal(spread[1], compact[1])
    assert (compact[0][1] != compact[0][0]).any()
    del views, view, buf
    torch.cuda.empty_cache()


def test_case_h_deterministic_and_padding_never_read():
    yt, yp, tm, lens, mouth, upper = _case_a_dev()
    c1, f1 = _run(yt, yp, lens, tm, mouth, upper)
    c2, f2 = _run(yt, yp, lens, tm, mouth, upper)
    assert torch.equal(c1, c2) and torch.equal(f1, f2)
    yt_p, yp_p = yt.clone(), yp.clone()
    for b, n in enumerate(lens):
        yt_p[b, n:] = float("nan")
        yp_p[b, n:] = float("nan")
    c3, f3 = _run(yt_p, yp_p, lens, tm, mouth, upper)
    assert torch.equal(c1, c3) and torch.equal(f1, f3) and torch.isfinite(c3).all()


def test_case_i_arguments():
    from dimx import lib
    from dimx.engine import op_mesh_metrics
    yt, yp, tm, lens, mouth, upper = _case_a_dev()
    with pytest.raises(lib.DimxError, match=r"\(-1\)"):
        op_mesh_metrics(yt, yp, [9, 0, 1], tm, mouth, upper)
    # an out-of-range index is refused on the host, before any launch
    for bad in ([0, NV], [-1, 3]):
        with pytest.raises(lib.DimxError, match="outside"):
            op_mesh_metrics(yt, yp, lens, tm, bad, upper)
        with pytest.raises(lib.DimxError, match="outside"):
            op_mesh_metrics(yt, yp, lens, tm, mouth, bad)
    # raw C-ABI: a workspace one byte short, B = 0
    L_ = lib.load()
    B, Ln = 3, 9
    yt_c, yp_c = yt.contiguous(), yp[:, :Ln].contiguous()
    md = torch.tensor(mouth, dtype=torch.int32, device="cuda")
    ud = torch.tensor(upper, dtype=torch.int32, device="cuda")
    clip = torch.full((B, 4), -7.0, dtype=torch.float64, device="cuda")
    status = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    need = int(L_.dimx_op_mesh_metrics_ws_bytes(B, Ln, len(mouth), len(upper)))
    assert need > 0 and L_.dimx_op_mesh_metrics_ws_bytes(0, Ln, 1, 1) == 0
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    lens_c = (ctypes.c_int32 * B)(*lens)

    def call(Bc, ws_bytes):
        return L_.dimx_op_mesh_metrics(lib.ptr(yt_c), yt_c.stride(0), yt_c.stride(1), lib.ptr(yp_c), yp_c.stride(0), yp_c.stride(1),
                                       lib.ptr(tm), tm.stride(0), lens_c, Bc, Ln, NV, lib.ptr(md), len(mouth), lib.ptr(ud), len(upper),
                                       lib.ptr(clip), None, lib.ptr(status), lib.ptr(ws), ws_bytes, lib.stream_ptr())
    assert call(B, need - 1) == -1
    assert call(0, need) == -1
    torch.cuda.synchronize()
    assert (clip == -7.0).all() and status.item() == 7 and not ws.any()      # nothing was enqueued
    assert call(B, need) == 0
    torch.cuda.synchronize()
    ref_clip, _ = _run(yt, yp, lens, tm, sorted(mouth), sorted(upper), want_frames=False)
    assert status.item() == 0 and torch.isfinite(clip).all()
    assert _rel(clip.cpu().numpy()[:, [0, 1]], ref_clip.cpu().numpy()[:, [0, 1]]) <= TOL      # unsorted maps: the same values within rounding
    assert _rel(clip.cpu().numpy()[:, 2:], ref_clip.cpu().numpy()[:, 2:]) <= TOL


def test_case_j_accumulator_over_two_updates():
    from dimx.metrics import BiwiMeshMetrics
    from dimx.mymetrics import compute_biwi_metrics
    base, pred, templ, lens, mouth, upper = _case_a()
    yt, yp, tm, _, _, _ = _case_a_dev()
    g = torch.Generator().manual_seed(110)
    B2, L2, lens2 = 2, 11, [11, 10]
    templ2 = 0.1 * torch.randn(B2, V, generator=g)
    yt2 = templ2[:, None] + 0.05 * torch.randn(B2, L2, V, generator=g)
    yp2 = templ2[:, None] + 0.07 * torch.randn(B2, L2, V, generator=g)
    acc = BiwiMeshMetrics(mouth, upper)
    acc.update(yt, yp, lens, tm)
    acc.update(yt2.cuda(), yp2.cuda(), lens2, templ2.cuda())
    lve, fdd = acc.result()
    gts = [base[b, 1:1 + n].double().numpy() for b, n in enumerate(lens)] + [yt2[b, :n].double().numpy() for b, n in enumerate(lens2)]
    preds = [pred[b, :n].double().numpy() for b, n in enumerate(lens)] + [yp2[b, :n].double().numpy() for b, n in enumerate(lens2)]
    tms = [templ[b].double().numpy() for b in range(3)] + [templ2[b].double().numpy() for b in range(B2)]
    ref = compute_biwi_metrics(gts, preds, None, tms, mouth, upper)
    e_lve, e_fdd = _rel(lve, ref["lve"]), abs(fdd - float(ref["fdd"])) / float(ref["fdd_scale"])
    print("J: lve %.3g  fdd %.3g" % (e_lve, e_fdd))
    assert e_lve <= TOL and e_fdd <= TOL


def test_case_k_speaker_driver_hip_equals_reference():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    from test_biwi import synthetic_biwi_loader
    from dimx.seq2seq_pretrain import SpeakerSLMFT
    from dimx.x_engine_pt import evaluate_mesh_epoch_biwi
    mouth, upper = _dup_map(11, 40), _dup_map(12, 23)
    model = SpeakerSLMFT(mesh_dim=V, mouth_map=mouth).cuda()
    loader = synthetic_biwi_loader(2, 12, V)
    dev = torch.device("cuda:0")
    lve_h, fdd_h = evaluate_mesh_epoch_biwi(model, loader, dev, mouth, upper, backend="hip")
    lve_r, fdd_r = evaluate_mesh_epoch_biwi(model, loader, dev, mouth, upper, backend="reference")
    e_lve = abs(lve_h - lve_r) / abs(lve_r)
    e_fdd = abs(fdd_h - fdd_r)      # relative to mean(sigma_gt + sigma_pred), taken from the operator's own per-clip output below
    from dimx.engine import op_mesh_metrics
    from dimx.x_engine_pt import BIWI_SPEAKER_IDS
    scale, clips = 0.0, 0
    with torch.no_grad():
        for xa, xv, xt, xe, ids in loader:
            sid = torch.tensor([BIWI_SPEAKER_IDS[f.split("_")[0]] for f in ids]).long().to(dev)
            mask = torch.ones(xa.shape[:2], dtype=torch.bool, device=dev)
            xv_d, xt_d = xv.to(dev), xt.to(dev)
            mesh = model(xv_d, xe.to(dev), xa.to(dev), mask, xt_d, mode="train", speaker_ids=sid, return_mesh=True)[-1]
            clip, _ = op_mesh_metrics(xv_d[:, 1:], mesh, [mesh.shape[1]] * mesh.shape[0], xt_d, mouth, upper)
            scale += float((clip[:, 2] + clip[:, 3]).sum())
            clips += clip.shape[0]
    e_fdd /= scale / clips
    print("K: hip (%.17g, %.17g) vs reference backend (%.17g, %.17g): lve %.3g fdd %.3g" % (lve_h, fdd_h, lve_r, fdd_r, e_lve, e_fdd))
    assert lve_r > 0.0 and e_lve <= TOL and e_fdd <= TOL
