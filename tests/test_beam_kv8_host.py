"""CPU: beam search over FP8 K/V caches (dimx_set_beam_kv8) -- the definition of the reorder (dimx/kv8.py reorder) against a
direct gather, that it commutes with the dequantiser and leaves kv8.self_step what it is on the ancestor's rows, the C-ABI's three
new symbols, and the module layers: ``beam_kv8`` with a beam, its refusals, and the refusals of self_kv8 / kv8 / kv8_samples with a beam
that stay."""
import os
import re

import numpy as np
import pytest
import torch

from dimx import kv8, lib

torch.set_grad_enabled(False)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, H, TP = 6, 2, 24
CODE_SENTINEL, SCALE_SENTINEL_BITS = 0xAB, 0x7FC00123      # past c: a code no row below holds in every element, a NaN with a payload


def parents(W, kind, nclip):
    """one parent vector per clip (counted within the clip); clip 0 always keeps the identity"""
    ident = list(range(W))
    if kind == "identity":
        p = ident
    elif kind == "swap":
        p = [w ^ 1 if (w ^ 1) < W else w for w in ident]
    elif kind == "cycle":
        p = [(w + 1) % W for w in ident]
    elif kind == "equal":
        p = [min(2, W - 1)] * W
    else:                                       # "invalid": one parent out of range
        p = [(w + 1) % W for w in ident]
        p[W - 1] = W if W % 2 else -1
    return np.array(ident + p * (nclip - 1), dtype=np.int32)


def planes(g, rows, c, heads=H, tp=TP):
    """(codes, scale) with valid rows at the positions <= c and the sentinels past them"""
    codes = g.integers(0, 256, (rows, heads, tp, 64), dtype=np.uint8)
    scale = (g.random((rows, heads, tp)).astype(np.float32) + np.float32(0.01))
    codes[:, :, c + 1:] = CODE_SENTINEL
    scale.view(np.uint32)[:, :, c + 1:] = SCALE_SENTINEL_BITS
    return codes, scale


def gather(codes, scale, parent, c, W):
    """the reorder as one fancy index, written independently of kv8.reorder"""
    rows = np.arange(codes.shape[0])
    src = rows.copy()
    for clip in range(codes.shape[0] // W):
        p = parent[clip * W:(clip + 1) * W]
        if ((p >= 0) & (p < W)).all():
            src[clip * W:(clip + 1) * W] = clip * W + p
    oc, osc = codes.copy(), scale.view(np.uint32).copy()
    oc[:, :, :c + 1] = codes[src][:, :, :c + 1]
    osc[:, :, :c + 1] = scale.view(np.uint32)[src][:, :, :c + 1]
    return oc, osc.view(np.float32)


@pytest.mark.parametrize("c", [0, 5, 23])
@pytest.mark.parametrize("W", [2, 3])
def test_reorder_is_the_gather_by_parent(W, c):
    g = np.random.default_rng(100 * W + c)
    for kind in ("identity", "swap", "equal", "invalid"):
        codes, scale = planes(g, R, c)
        parent = parents(W, kind, R // W)
        before = (codes.copy(), scale.view(np.uint32).copy())
        oc, osc = kv8.reorder(codes, scale, parent, c, W)
        assert np.array_equal(codes, before[0]) and np.array_equal(scale.view(np.uint32), before[1]), "the arguments were written"
        wc, wsc = gather(codes, scale, parent, c, W)
        assert oc.dtype == np.uint8 and osc.dtype == np.float32
        assert np.array_equal(oc, wc) and np.array_equal(osc.view(np.uint32), wsc.view(np.uint32)), (kind, c)
        # positions past c keep their bits
        assert (oc[:, :, c + 1:] == CODE_SENTINEL).all() and (osc.view(np.uint32)[:, :, c + 1:] == SCALE_SENTINEL_BITS).all()
        # clip 0 (identity) and a clip with a parent out of range are untouched
        assert np.array_equal(oc[:W], codes[:W]) and np.array_equal(osc.view(np.uint32)[:W], scale.view(np.uint32)[:W])
        if kind in ("identity", "invalid"):
            assert np.array_equal(oc, codes) and np.array_equal(osc.view(np.uint32), scale.view(np.uint32)), kind
        else:
            assert not np.array_equal(oc[W:, :, :c + 1], codes[W:, :, :c + 1]), kind


@pytest.mark.parametrize("W", [2, 3])
def test_reorder_commutes_with_the_dequantiser(W):
    """dequantize(reorder(x)) == reorder(dequantize(x)) bit for bit: codes and scale move together and no value is formed"""
    g = np.random.default_rng(7 + W)
    c = 17
    codes, scale = kv8.quantize(g.standard_normal((R, H, TP, 64)).astype(np.float32) * np.float32(3))
    scale[1, 0, 3] = 0.0
    codes[1, 0, 3] = 0
    for kind in ("swap", "equal"):
        parent = parents(W, kind, R // W)
        oc, osc = kv8.reorder(codes, scale, parent, c, W)
        left = kv8.dequantize(oc, osc)
        deq = kv8.dequantize(codes, scale)
        src = np.arange(R) // W * W + parent
        right = deq.copy()
        right[:, :, :c + 1] = deq[src][:, :, :c + 1]
        assert np.array_equal(left.view(np.uint32), right.view(np.uint32)), kind


@pytest.mark.parametrize("W", [2, 3])
def test_self_step_on_a_reordered_buffer_is_self_step_on_the_parents_buffer(W):
    g = np.random.default_rng(19 + W)
    n = 9                                   # positions 0 .. n - 1 are cached, the step appends position n
    arrs = []
    for _ in range(2):
        arrs += list(kv8.quantize(g.standard_normal((R, H, TP, 64)).astype(np.float32)))
    kc, ks, vc, vs = arrs
    q, k_new, v_new = (g.standard_normal((R, H, 64)).astype(np.float32) for _ in range(3))
    parent = parents(W, "equal", R // W)
    parent[:W] = parents(W, "swap", 1)[:W]                # no clip keeps the identity here
    src = np.arange(R) // W * W + parent
    rk, rks = kv8.reorder(kc, ks, parent, n - 1, W)
    rv, rvs = kv8.reorder(vc, vs, parent, n - 1, W)
    got = kv8.self_step(q, k_new, v_new, rk, rks, rv, rvs, n)
    # every row on a copy of its parent's buffer, with its own q / k_new / v_new
    pk, pks, pv, pvs = (a[src].copy() for a in (kc, ks, vc, vs))
    want = kv8.self_step(q, k_new, v_new, pk, pks, pv, pvs, n)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    for a, b in ((rk, pk), (rv, pv)):
        assert np.array_equal(a[:, :, :n + 1], b[:, :, :n + 1])
    assert np.array_equal(rks.view(np.uint32)[:, :, :n + 1], pks.view(np.uint32)[:, :, :n + 1])
    # and it is not the step on the rows' own buffers
    own = kv8.self_step(q, k_new, v_new, kc.copy(), ks.copy(), vc.copy(), vs.copy(), n)
    moved = src != np.arange(R)
    assert (np.abs(own - got)[moved].max(axis=(1, 2)) > 1e-3).all() and np.array_equal(own[~moved], got[~moved])


NEW = {"dimx_set_beam_kv8": 2, "dimx_beam_kv8": 2, "dimx_op_beam_reorder_kv8": 9}


def test_symbols_are_declared_exported_and_refuse_bad_arguments_without_a_gpu():
    hdr = open(os.path.join(ROOT, "include", "dimx.h")).read()
    l = lib.load()
    for name, nargs in NEW.items():
        m = re.search(r"\bint %s\(([^;]*)\);" % name, hdr)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(lib.SIGNATURES[name][1]), name
        assert hasattr(l, name)
    assert l.dimx_set_beam_kv8(None, 1) == -1 and b"null handle" in l.dimx_last_error()
    assert l.dimx_beam_kv8(None, None) == -1 and b"null handle" in l.dimx_last_error()

    def op(codes=4096, scale=4096, parent=4096, rows=4, W=2, heads=2, tp=24, c=3):
        return l.dimx_op_beam_reorder_kv8(codes, scale, parent, rows, W, heads, tp, c, None)
    for kw, word in ((dict(codes=None), b"null"), (dict(scale=None), b"null"), (dict(parent=None), b"null"), (dict(rows=5), b"multiple"),
                     (dict(rows=0), b"multiple"), (dict(W=3, rows=6), b"width"), (dict(W=0), b"multiple"), (dict(c=-1), b"outside"),
                     (dict(c=24), b"outside"), (dict(codes=4096 + 8), b"aligned"), (dict(scale=4096 + 2), b"aligned"), (dict(heads=0), b"range")):
        assert op(**kw) == -1, kw
        assert word in l.dimx_last_error(), (kw, l.dimx_last_error())


class _BeamStub(torch.nn.Module):
    """The protocol's view of a model: records the keywords of every forward and returns W tries per clip"""

    def __init__(self):
        super().__init__()
        self.seen = []

    def forward(self, v_speaker, v_listener, v_audio, mask, mode="train", beam_width=None, num_return=1, n_samples=1, **kw):
        self.seen.append(dict(kw, mode=mode, beam_width=beam_width, num_return=num_return))
        B, T, C = v_listener.shape
        S = int(num_return if beam_width else n_samples)
        t = torch.arange(T - 1, dtype=torch.float32)[None, None, :, None]
        s = torch.arange(S, dtype=torch.float32)[None, :, None, None]
        pred = 0.5 * v_listener[:, None, 1:] + torch.sin(0.3 * t + 1.7 * s) * (0.2 + 0.1 * s)
        return torch.zeros(()), {}, pred if S > 1 else pred[:, 0]


def test_module_layers_take_beam_kv8_with_a_beam_and_keep_the_old_refusals():
    import stub_model
    from dimx import x_engine_pt
    from dimx.seq2seq_pretrain import SLMFT
    batches = stub_model.protocol_batches()
    # accepted with decode="beam", in every spelling and with every select: past the argument checks, a CPU device is what beam
    # decoding refuses (tests/test_gpu_beam_kv8.py runs the protocol on the GPU)
    for spelled in ("self", "cross", "both", True):
        for select in ("fd", "likelihood", "consensus"):
            stub = _BeamStub()
            with pytest.raises(lib.DimxError, match="ROCm GPU"):
                x_engine_pt.evaluate_test_epoch(stub, batches, torch.device("cpu"), decode="beam", beam_width=2, beam_kv8=spelled, select=select)
            assert not stub.seen
    # refused without a beam and with guidance
    for kw in ({}, {"decode": "sample"}, {"decode": "beam", "beam_width": 2, "guidance": 1.5}):
        with pytest.raises(ValueError, match="beam_kv8"):
            x_engine_pt.evaluate_test_epoch(_BeamStub(), batches, torch.device("cpu"), beam_size=2, beam_kv8=True, **kw)
    # the three old refusals with a beam still fire, word for word
    for name in ("self_kv8", "kv8", "kv8_samples"):
        with pytest.raises(ValueError, match=r"evaluate_test_epoch\(%s=True\) applies to decode='sample'" % name):
            x_engine_pt.evaluate_test_epoch(_BeamStub(), batches, torch.device("cpu"), decode="beam", beam_width=2, **{name: True})
    model = SLMFT().eval()
    B, T = 2, 8
    args = (torch.zeros(B, T, 56), torch.zeros(B, T, 56), torch.zeros(B, T, 768), torch.ones(B, T, dtype=torch.bool))
    z = torch.zeros(B, T, dtype=torch.long)
    for kw in ({"mode": "train", "beam_width": 2}, {"mode": "val"}, {"mode": "val", "beam_width": 2, "guidance": 1.5}):
        with pytest.raises(ValueError, match="beam_kv8"):
            model(*args, beam_kv8=True, **kw)
        with pytest.raises(ValueError, match="beam_kv8"):
            model.forward_decoder(None, z, args[2], args[3], kw["mode"], v_speaker=args[0], beam_kv8="self", beam_width=kw.get("beam_width", 0),
                                  guidance=kw.get("guidance"), n_samples=kw.get("beam_width", 1))
    old = {"self_kv8": "self_kv8 applies to mode='val' without beam search and without guidance",
           "kv8": "kv8 applies to mode='val' with one sample per clip and without beam search",
           "kv8_samples": "kv8_samples applies to mode='val' without beam search and without guidance"}
    for name, text in old.items():
        with pytest.raises(ValueError) as e:
            model(*args, mode="val", beam_width=2, **{name: True})
        assert str(e.value) == text
        with pytest.raises(ValueError) as e:
            model.forward_decoder(None, z, args[2], args[3], "val", v_speaker=args[0], beam_width=2, n_samples=2, **{name: True})
        assert str(e.value) == text
