"""dimx_op_lstm_layer (csrc/lstm.hip) and the two-layer stack against torch.nn.LSTM on the CPU in f32.

Tolerance 1e-4 absolute: the project's coefficient tolerance (BASELINE.json north_star); the outputs lie in (-1, 1).
For the record, on the CPU at T = 299: torch's own f32-vs-f64 difference is 7e-8 at the default weight scale, 2.6e-7 at x2
and 1.8e-6 at x4, and an independently ordered f32 implementation stays within 1.2e-6 of f64, so 1e-4 leaves more than 50x
headroom.  No weight scale above x4: at x8 the recurrence is chaotic (torch f32 and f64 differ by 1.7 there) and no
implementation can be judged.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-4
CASES = [(1, 299, 56), (3, 26, 56), (8, 26, 768), (40, 299, 56)]


def _lstm(In, scale, seed, layers=1):
    torch.manual_seed(seed)
    m = torch.nn.LSTM(In, 384, layers, batch_first=True, bidirectional=True)
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(scale)
    return m.eval()


def _pairs(sd, layer):
    names = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")
    return [(sd["%s_l%d" % (n, layer)], sd["%s_l%d_reverse" % (n, layer)]) for n in names]


def _run(x, sd, layer, safe, dev):
    from dimx import engine as E
    w_ih, w_hh, b_ih, b_hh = _pairs(sd, layer)
    return E.op_lstm_layer(x.to(dev), w_ih, w_hh, b_ih, b_hh, safe=safe, return_faults=True)


@pytest.mark.parametrize("scale", [1.0, 4.0])
@pytest.mark.parametrize("B,T,In", CASES)
def test_layer_both_paths_match_torch(B, T, In, scale):
    dev = torch.device("cuda:0")
    m = _lstm(In, scale, 100 + B + T)
    x = torch.randn(B, T, In)
    with torch.no_grad():
        ref, _ = m(x)
    sd = m.state_dict()
    for safe in (False, True):
        y, faults = _run(x, sd, 0, safe, dev)
        err = (y.cpu() - ref).abs().max().item()
        print("lstm layer B=%d T=%d In=%d scale=%g %s path: max|y|=%.3f err=%.2e faults=%d"
              % (B, T, In, scale, "safe" if safe else "group", ref.abs().max().item(), err, faults))
        assert faults == 0
        assert err < TOL, "%s path differs from torch.nn.LSTM by %g" % ("safe" if safe else "group", err)
        y2, _ = _run(x, sd, 0, safe, dev)
        assert torch.equal(y, y2), "%s path is not bit-identical across two runs" % ("safe" if safe else "group")


@pytest.mark.parametrize("scale", [1.0, 4.0])
@pytest.mark.parametrize("B,T", [(1, 299), (3, 26), (40, 299)])
def test_two_layer_stack_matches_torch(B, T, scale):
    dev = torch.device("cuda:0")
    m = _lstm(56, scale, 7 + B, layers=2)
    x = torch.randn(B, T, 56)
    with torch.no_grad():
        ref, _ = m(x)
    sd = m.state_dict()
    for safe in (False, True):
        y0, f0 = _run(x, sd, 0, safe, dev)
        y1, f1 = _run(y0, sd, 1, safe, dev)
        err = (y1.cpu() - ref).abs().max().item()
        print("lstm stack B=%d T=%d scale=%g %s path: max|y|=%.3f err=%.2e" % (B, T, scale, "safe" if safe else "group",
                                                                              ref.abs().max().item(), err))
        assert f0 == 0 and f1 == 0
        assert err < TOL


def test_saturating_scale_reaches_the_rails():
    """the x4 case is only a saturation test if the gates do saturate: max |y| of the reference's two-layer stack (the
    (40, 299) case above, same seed) is about 0.95"""
    m = _lstm(56, 4.0, 7 + 40, layers=2)
    with torch.no_grad():
        ref, _ = m(torch.randn(40, 299, 56))
    assert ref.abs().max().item() > 0.9


def test_bf16_recurrence_is_refused():
    """the bf16-operand recurrence is not built: the entry point says so instead of running something else"""
    import ctypes
    from dimx import lib as L
    lib = L.load()
    x = torch.zeros(1, 2, 56, device="cuda:0")
    arr = (ctypes.c_void_p * 2)(x.data_ptr(), x.data_ptr())
    rc = lib.dimx_op_lstm_layer(L.BF16, L.ptr(x), 1, 2, 56, 384, arr, arr, arr, arr, L.ptr(x), 0, None, None)
    assert rc == -1
