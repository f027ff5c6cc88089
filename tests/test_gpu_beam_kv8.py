"""GPU: beam search over FP8 K/V caches (dimx_set_beam_kv8, dimx_op_beam_reorder_kv8; csrc/beam.hip beam_reorder_kv8_kernel).
The operator bit for bit against dimx.kv8.reorder; the switch off is what the library did before it existed; W = 1 is the greedy
generation over the same buffers; the definition dimx.beam fed the device's own logits reproduces the search; the buffers the search
leaves hold every final hypothesis's own rows (the CPU checker of tests/self_kv8_ref.py replays each hypothesis on them); and the host
layers above.  The clips, the prompt and the bounds are those of tests/test_gpu_beam.py."""
import numpy as np
import pytest
import torch

from test_gpu_beam import BOUND, PROMPT, STEP_TOL, WIDTHS, _Case, _check_replay, _dev, _loader, _model_inputs
from test_beam_kv8_host import CODE_SENTINEL, SCALE_SENTINEL_BITS, parents

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
ERR_ARG = -1
NCLIP, H, TP = 3, 2, 24


@pytest.fixture(scope="module")
def engines(full_sd):
    from dimx import engine, lib
    out = {}
    for name, mode in (("f32", lib.MODE_PARITY_F32), ("bf16", lib.MODE_PERF_BF16)):
        out[name] = engine.Engine("cuda:0", mode)
        out[name].load_state_dict(full_sd)
    return out


@pytest.fixture(scope="module")
def clips():
    return _Case()


def _same(a, b):
    """bit equality of two tuples of tensors (floats compared as their bits)"""
    raw = lambda t: t.view(torch.int64) if t.dtype == torch.float64 else (t.view(torch.int32) if t.dtype == torch.float32 else t)
    return len(a) == len(b) and all(torch.equal(raw(x), raw(y)) for x, y in zip(a, b))


def _cleared(e):
    return e.beam_kv8() is False and e.self_kv8() is None and e.cross_kv8() is None


# ---- 1
def _op_planes(W, c):
    """codes: random bytes with 0x7F / 0xFF (the NaN codes) among them; scales: zeros, denormals and normal values; the sentinels past c"""
    g = np.random.default_rng(1000 * W + c)
    codes = g.integers(0, 256, (NCLIP * W, H, TP, 64), dtype=np.uint8)
    codes[:, :, :, 0] = 0x7F
    codes[:, :, :, 63] = 0xFF
    scale = g.random((NCLIP * W, H, TP)).astype(np.float32)
    scale[:, 0, ::3] = 0.0
    scale.view(np.uint32)[:, 1, ::2] = g.integers(1, 1 << 23, scale[:, 1, ::2].shape, dtype=np.uint32)      # denormals
    codes[:, :, c + 1:] = CODE_SENTINEL
    scale.view(np.uint32)[:, :, c + 1:] = SCALE_SENTINEL_BITS
    return codes, scale


@pytest.mark.parametrize("W", WIDTHS)
def test_op_beam_reorder_kv8_is_the_definition_bit_for_bit(W):
    from dimx import kv8
    from dimx.engine import op_beam_reorder_kv8
    for c in (0, 3, 4, 22, 23):
        codes, scale = _op_planes(W, c)
        for kind in ("identity", "swap", "cycle", "equal", "invalid"):
            parent = parents(W, kind, NCLIP)
            wc, ws = kv8.reorder(codes, scale, parent, c, W)
            runs = []
            for _ in range(2):
                dc, ds = torch.from_numpy(codes).to(_dev()), torch.from_numpy(scale).to(_dev())
                oc, osc = op_beam_reorder_kv8(dc, ds, parent, c, W)
                assert oc.data_ptr() == dc.data_ptr() and osc.data_ptr() == ds.data_ptr()
                runs.append((oc.cpu().numpy(), osc.cpu().numpy().view(np.uint32)))
            gc, gs = runs[0]
            assert np.array_equal(gc, wc) and np.array_equal(gs, ws.view(np.uint32)), (W, c, kind)
            assert (gc[:, :, c + 1:] == CODE_SENTINEL).all() and (gs[:, :, c + 1:] == SCALE_SENTINEL_BITS).all(), (W, c, kind)
            assert np.array_equal(gc[:W], codes[:W]) and np.array_equal(gs[:W], scale.view(np.uint32)[:W])      # clip 0: the identity
            if kind in ("identity", "invalid") or W == 1:
                assert np.array_equal(gc, codes) and np.array_equal(gs, scale.view(np.uint32)), (W, c, kind)
            elif kind in ("swap", "cycle"):
                assert not np.array_equal(gc[W:, :, :c + 1], codes[W:, :, :c + 1])
            assert np.array_equal(runs[1][0], gc) and np.array_equal(runs[1][1], gs)


def test_op_beam_reorder_kv8_arguments():
    from dimx import lib as L
    from dimx.engine import op_beam_reorder_kv8
    l = L.load()
    codes = torch.full((4, H, TP, 64 + 1), 0xAB, dtype=torch.uint8, device=_dev()).view(-1)
    scale = torch.full((4 * H * TP + 4,), -7.0, device=_dev())
    parent = torch.tensor([1, 0, 1, 0], dtype=torch.int32, device=_dev())
    good = dict(codes=codes.data_ptr(), scale=scale.data_ptr(), parent=parent.data_ptr(), R=4, W=2, H=H, Tp=TP, c=5)

    def call(**kw):
        a = dict(good, **kw)
        return l.dimx_op_beam_reorder_kv8(a["codes"], a["scale"], a["parent"], a["R"], a["W"], a["H"], a["Tp"], a["c"], L.stream_ptr(_dev()))
    for kw in (dict(codes=None), dict(scale=None), dict(parent=None), dict(R=3), dict(R=0), dict(W=3, R=6), dict(W=0), dict(W=16, R=16), dict(c=-1),
               dict(c=TP), dict(codes=codes.data_ptr() + 8), dict(codes=codes.data_ptr() + 1), dict(scale=scale.data_ptr() + 2), dict(H=0), dict(Tp=0)):
        assert call(**kw) == ERR_ARG, kw
    torch.cuda.synchronize()
    assert bool((codes == 0xAB).all()) and bool((scale == -7.0).all()), "a refused call launched something"
    assert call() == 0
    with pytest.raises(L.DimxError):
        op_beam_reorder_kv8(torch.zeros(4, H, TP, 64, dtype=torch.uint8), torch.zeros(4, H, TP), [0, 1, 0, 1], 0, 2)       # CPU tensors
    with pytest.raises(L.DimxError):
        op_beam_reorder_kv8(torch.zeros(4, H, TP, 64, dtype=torch.uint8, device=_dev()), torch.zeros(4, H, TP + 1, device=_dev()), [0, 1, 0, 1], 0, 2)


# ---- 2
def test_off_is_what_it_was(engines, clips):
    from dimx import lib as L
    e, c, W = engines["f32"], clips, 4
    kw = dict(return_logits=True, return_backptr=True)
    before = c.beam(e, W, True, **kw)
    sbuf = torch.full((e.self_kv8_bytes(c.B * W, c.T),), 0xAB, dtype=torch.uint8, device=_dev())
    cbuf = torch.full((e.cross_kv8_bytes(c.B, c.T),), 0xAB, dtype=torch.uint8, device=_dev())
    assert e.beam_kv8() is False
    for which in ("self", "cross", "both"):
        e.set_self_kv8(sbuf if which != "cross" else None)
        e.set_cross_kv8(cbuf if which != "self" else None)
        try:
            with pytest.raises(L.DimxError, match=r"\(-1\)"):       # the switch is off: the refusal of before, ahead of any launch
                c.beam(e, W, True, **kw)
        finally:
            e.set_self_kv8(None)
            e.set_cross_kv8(None)
    torch.cuda.synchronize()
    assert bool((sbuf == 0xAB).all()) and bool((cbuf == 0xAB).all()), "a refused call launched something"
    # the switch on and no buffer: the plain call's bits
    e.set_beam_kv8(True)
    try:
        assert e.beam_kv8() is True
        on = c.beam(e, W, True, **kw)
    finally:
        e.set_beam_kv8(False)
    assert _same(on, before)
    # generate() does not read the switch: a set buffer with n_samples > 1 is still refused under it
    e.set_beam_kv8(True)
    e.set_cross_kv8(cbuf)
    try:
        c.context(e, W)
        with pytest.raises(L.DimxError, match=r"\(-1\)"):
            e.generate(c.z[:, 0].to(_dev()), c.m8, c.T, 0.0, n_samples=W)
    finally:
        e.set_cross_kv8(None)
        e.set_beam_kv8(False)
    for which in ("self", "cross", True):
        got = c.beam(e, W, True, beam_kv8=which, **kw)
        assert _cleared(e), which
        assert not _same(got[2:3], before[2:3]), "beam_kv8=%r left the logits' bits unchanged" % (which,)
    assert _same(c.beam(e, W, True, **kw), before)
    with pytest.raises(ValueError, match="beam_kv8"):
        c.beam(e, W, beam_kv8="keys")


def test_other_variants_refuse_the_switch():
    from dimx import engine, lib as L
    for variant in ("slm", "legacy"):
        other = engine.Engine("cuda:0", L.MODE_PARITY_F32, variant=variant)
        with pytest.raises(L.DimxError, match=r"\(-1\)"):
            other.set_beam_kv8(True)
        assert other.beam_kv8() is False
        other.close()


# ---- 3
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_width_one_is_the_greedy_generation_over_both_buffers(engines, clips, mode):
    """prompted calls keep layer 0 on its cache in both, so the two calls launch the same attention kernels on the same operands"""
    e, c = engines[mode], clips
    c.context(e, 1, PROMPT["prefill"])
    tok, lg = e.generate(None, c.m8, c.T, 0.0, return_logits=True, prompt=c.prompt, prompt_len=c.plen, prefill=PROMPT["prefill"], kv8=True,
                         self_kv8=True)
    rows = [tuple(t.clone() for t in lay) for lay in e.self_kv8_layers(c.B, c.T)]
    btok, score, blg = c.beam(e, 1, True, return_logits=True, beam_kv8=True)
    assert _cleared(e)
    assert torch.equal(btok, tok) and torch.equal(blg.view(torch.int32), lg.view(torch.int32))
    for a, b in zip(rows, e.self_kv8_layers(c.B, c.T)):      # and the same codes and scales
        assert all(torch.equal(x[:, :, :c.T - 1].contiguous().view(torch.uint8), y[:, :, :c.T - 1].contiguous().view(torch.uint8))
                   for x, y in zip(a, b))


# ---- 4
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("prompted", [False, True], ids=["free", "prompted"])
@pytest.mark.parametrize("W", [2, 4, 10])
def test_replay_of_the_dumped_logits(engines, clips, W, prompted, mode):
    e, c = engines[mode], clips
    tok, score, lg, bp = (t.cpu().numpy() for t in c.beam(e, W, prompted, return_logits=True, return_backptr=True, beam_kv8=True))
    _check_replay(c, W, prompted, tok, score, lg, bp, c.prompt.cpu().numpy())      # scores within BOUND of the definition's
    assert BOUND == 1e-11
    if prompted:
        assert (lg[:, :PROMPT["prefill"] - 1] == 0).all()


# ---- 5
@pytest.fixture(scope="module")
def checker(full_sd, clips):
    """the CPU checker's context and plain cross K / V of the SHORT clips, computed once"""
    import kv8_ref
    import prompt_ref
    ctx = prompt_ref.case_context(full_sd, clips.v_s, clips.v_a, clips.mask)
    return {"ctx": ctx, "cross": kv8_ref.cross_kv(full_sd, ctx)}


@pytest.mark.parametrize("which", ["self", "cross", True], ids=["self", "cross", "both"])
@pytest.mark.parametrize("W", [4, 10])
def test_the_codes_were_reordered(engines, clips, checker, full_sd, W, which):
    """After the call row r of the self buffer must hold, position by position, the rows hypothesis r's ancestors appended.  Every
    final hypothesis is replayed by the CPU checker on the buffers' own dequantised rows (self rows of row r, cross rows of its clip)
    along its own tokens; its logits at column c are compared with the dump at the row that ran step c on the hypothesis's path.  One
    wrong row of one layer moves them by order 1.  The plain-cache teacher-forced logits of the same hypotheses are further away than
    STEP_TOL: the codes are what the search read.
    Measured on MI355X, worst |dump along the ancestry - checker| (against STEP_TOL = 2e-3) and |dump - plain teacher-forced|:
      W = 4:  self 1.5e-6 / 2.8e-2, cross 1.4e-6 / 1.5e-2, both 1.6e-6 / 3.4e-2
      W = 10: self 1.7e-6 / 2.8e-2, cross 1.5e-6 / 1.5e-2, both 1.6e-6 / 3.4e-2"""
    import kv8_ref
    import self_kv8_ref
    e, c = engines["f32"], clips
    tok, score, lg, bp = c.beam(e, W, return_logits=True, return_backptr=True, beam_kv8=which)
    assert _cleared(e)
    R, n = tok.shape
    rows = self_kv8_ref.dequantized(e.self_kv8_layers(R, c.T), n) if which != "cross" else None
    cross = kv8_ref.dequantized(e.cross_kv8_layers(c.B, c.T), c.T) if which != "self" else checker["cross"]
    _, ref_lg, _ = self_kv8_ref.self_kv8_generate(full_sd, c.z[:, :1], None, n, checker["ctx"], c.mask, None, self_kv8_ref.SelfRows(given=rows),
                                                   None, cross_kv=cross, follow=tok.cpu().long(), samples=W)
    ran = (torch.arange(R, device=_dev()) // W * W)[:, None] + bp.long()
    seen = lg[ran, torch.arange(n, device=_dev())[None, :]].cpu()
    err = (seen - ref_lg).abs().amax(-1)
    z = torch.cat([c.z[:, :1].repeat_interleave(W, 0).to(_dev()), tok.long()], 1)
    c.context(e, for_generate=False, repeat=W)
    tf, _, _ = e.decode_tf(z, c.m8.repeat_interleave(W, 0).contiguous(), None)
    away = (seen - tf.cpu()).abs().max().item()
    print("W=%d beam_kv8=%s: worst |dump along the ancestry - checker on the buffers' rows| %.3e (STEP_TOL %.0e); |dump - plain "
          "teacher-forced| %.3e" % (W, which, err.max().item(), STEP_TOL, away))
    assert err.max().item() <= STEP_TOL
    assert away > STEP_TOL


# ---- 6
def test_buffer_contents_do_not_matter_and_replays_equal_a_fresh_handle(full_sd, engines, clips):
    from dimx import engine, lib as L
    e, c, W = engines["f32"], clips, 5
    kw = dict(return_logits=True, return_backptr=True)
    sbuf = torch.zeros(e.self_kv8_bytes(c.B * W, c.T), dtype=torch.uint8, device=_dev())
    cbuf = torch.zeros(e.cross_kv8_bytes(c.B, c.T), dtype=torch.uint8, device=_dev())
    outs = []
    for fill in (0, 0xFF, 0xFF):
        sbuf.fill_(fill)
        cbuf.fill_(fill)
        e.set_self_kv8(sbuf)
        e.set_cross_kv8(cbuf)
        e.set_beam_kv8(True)
        try:
            outs.append(c.beam(e, W, True, **kw))       # the handle's own settings
        finally:
            e.set_beam_kv8(False)
            e.set_self_kv8(None)
            e.set_cross_kv8(None)
    assert _same(outs[1], outs[0]) and _same(outs[2], outs[0])
    fresh = engine.Engine("cuda:0", L.MODE_PARITY_F32)
    fresh.load_state_dict(full_sd)
    try:
        assert _same(c.beam(fresh, W, True, beam_kv8=True, **kw), outs[0])
    finally:
        fresh.close()


# ---- 7
@pytest.fixture(scope="module")
def model():
    from dimx.seq2seq_pretrain import SLMFT
    return SLMFT().eval()


def test_beam_kv8_through_the_model(model, clips):
    c, W = clips, 4
    args = _model_inputs(c)
    out = model(*args, mode="val", beam_width=W, num_return=W, return_tokens=True, return_scores=True, beam_kv8=True)
    assert out[2].shape == (c.B, W, c.T - 1, 56) and out[3].shape == (c.B, W, c.T - 1)
    assert bool((out[4].score[:, :-1] >= out[4].score[:, 1:]).all())
    e = model.engine(args[0].device)
    assert _cleared(e) and e.self_kv8_buffer() is not None and e.cross_kv8_buffer() is not None
    _, z_l = model.forward_vq(args[0], args[1], args[3], with_speaker=False)
    m8 = args[3].to(torch.uint8).contiguous()
    with model.engine_pinned():
        e.encode_ctx(args[0], args[2], m8, True, n_samples=W)
        tok, score = e.generate_beam(z_l[:, 0], m8, c.T, W, beam_kv8=True)
    assert torch.equal(out[3].reshape(c.B * W, -1), tok.long()) and torch.equal(out[4].score.reshape(-1), score)
    plain = model(*args, mode="val", beam_width=W, num_return=W, return_tokens=True, return_scores=True)
    assert not torch.equal(plain[4].score, out[4].score)        # the FP8 route ran: other logits, other scores
    for which in ("self", "cross"):
        one = model(*args, mode="val", beam_width=W, return_tokens=True, beam_kv8=which)
        assert one[3].shape == (c.B, c.T - 1) and _cleared(e)


@pytest.mark.parametrize("select", ["fd", "likelihood", "consensus"])
def test_protocol_with_beam_kv8(model, select):
    from dimx import x_engine_pt
    loader = _loader()
    kw = dict(select=select) if select != "fd" else dict(select=select, fd_backend="hip")
    y_true, y_pred, x, ids = x_engine_pt.evaluate_test_epoch(model, loader, _dev(), decode="beam", beam_width=2, beam_kv8=True, **kw)
    assert len(y_true) == len(y_pred) == len(x) == len(ids) == 6
    k = 0
    for batch in loader:
        src_s_v, src_s_a, tgt, mask, src_len, _ = x_engine_pt._prepare(batch, _dev())
        pred = model(src_s_v, tgt, src_s_a, mask, mode="val", beam_width=2, num_return=2, beam_kv8=True)[2].cpu().numpy()
        for j in range(len(src_len)):
            n = src_len[j] - 1
            assert y_pred[k].shape == (n, 56)
            if select == "likelihood":
                assert np.array_equal(y_pred[k], pred[j, 0, :n])      # the search's best hypothesis is the likelihood winner
            else:
                assert any(np.array_equal(y_pred[k], pred[j, s, :n]) for s in range(2))
            k += 1
    assert _cleared(model.engine(_dev()))
