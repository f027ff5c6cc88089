"""The yardstick of the converter training tests: EmocaConverter's head (reference code/seq2seq_pretrain.py:801-842) and the
loss of the reference's loop (code/train_converter.py:25-34) with stock torch.nn.LSTM / F.linear / F.leaky_relu and autograd on
the CPU, float64 unless asked otherwise.  Nothing here touches the HIP library."""
import torch
import torch.nn.functional as F

NAMES = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")
PRE = "vertice_map_reverse_lstm."


def lstm_module(In, scale=1.0, seed=0, layers=1, hh_scale=1.0):
    """torch.nn.LSTM(In, 384, bidirectional) with its default init times ``scale`` (1.0 = uniform +-0.051, the project's synthetic
    weight scale); ``hh_scale`` multiplies weight_hh on top"""
    torch.manual_seed(seed)
    m = torch.nn.LSTM(In, 384, layers, batch_first=True, bidirectional=True)
    with torch.no_grad():
        for n, p in m.named_parameters():
            p.mul_(scale * (hh_scale if n.startswith("weight_hh") else 1.0))
    return m


def pairs(sd, layer=0):
    return [(sd["%s_l%d" % (n, layer)], sd["%s_l%d_reverse" % (n, layer)]) for n in NAMES]


def layer_grads(m, x, dy, dtype=torch.float64):
    """autograd through one bidirectional layer ``m``: -> (y, dx, dw_ih pair, dw_hh pair, db pair) in ``dtype`` on the CPU"""
    mm = torch.nn.LSTM(m.input_size, m.hidden_size, 1, batch_first=True, bidirectional=True).to(dtype)
    mm.load_state_dict({k: v.to(dtype) for k, v in m.state_dict().items()})
    xx = x.detach().cpu().to(dtype).requires_grad_(True)
    with torch.enable_grad():
        y, _ = mm(xx)
        y.backward(dy.detach().cpu().to(dtype))
    g = {n: p.grad for n, p in mm.named_parameters()}
    assert torch.allclose(g["bias_ih_l0"], g["bias_hh_l0"], rtol=1e-4, atol=1e-6 * float(g["bias_ih_l0"].abs().max()))
    return (y.detach(), xx.grad, (g["weight_ih_l0"], g["weight_ih_l0_reverse"]), (g["weight_hh_l0"], g["weight_hh_l0_reverse"]),
            (g["bias_ih_l0"], g["bias_ih_l0_reverse"]))


def head_keys(sd):
    return [k for k in sd if k.startswith(PRE) or k.startswith("vertice_map_reverse.")]


def literal_loss(xp, xv, mouth_map):
    """the reference's own expression (B = 1): mse(xp, xv) + 5 mse(xp_mouth, xv_mouth) with its reshape(1, -1, V/3, 3) indexing"""
    nv = xp.shape[-1] // 3
    n = len(mouth_map)
    xp_mouth = xp.reshape(1, -1, nv, 3)[:, :, mouth_map, :].reshape(1, -1, n * 3)
    xv_mouth = xv.reshape(1, -1, nv, 3)[:, :, mouth_map, :].reshape(1, -1, n * 3)
    mse = torch.nn.MSELoss()
    return mse(xp, xv) + 5 * mse(xp_mouth, xv_mouth)


def converter_step(sd, motion, template, target, mouth_map=None, dtype=torch.float64):
    """-> ((loss, mse, mouth), {key: gradient}, mesh) of the 20 head tensors of ``sd`` on the CPU in ``dtype``"""
    P = {k: sd[k].detach().cpu().to(dtype) for k in head_keys(sd)}
    In = P[PRE + "weight_ih_l0"].shape[1]
    lstm = torch.nn.LSTM(In, 384, 2, batch_first=True, bidirectional=True).to(dtype)
    lstm.load_state_dict({k[len(PRE):]: v for k, v in P.items() if k.startswith(PRE)})
    l1 = torch.nn.Linear(768, 768).to(dtype)
    l2 = torch.nn.Linear(768, P["vertice_map_reverse.2.weight"].shape[0]).to(dtype)
    l1.load_state_dict({"weight": P["vertice_map_reverse.0.weight"], "bias": P["vertice_map_reverse.0.bias"]})
    l2.load_state_dict({"weight": P["vertice_map_reverse.2.weight"], "bias": P["vertice_map_reverse.2.bias"]})
    x = motion.detach().cpu().to(dtype)
    xv = target.detach().cpu().to(dtype)
    with torch.enable_grad():
        y, _ = lstm(x)
        xp = l2(F.leaky_relu(l1(y), 0.2))
        if template is not None:
            xp = xp + template.detach().cpu().to(dtype)[:, None, :]
        B, T, V = xp.shape
        mse = F.mse_loss(xp, xv)
        mouth = xp.new_zeros(())
        if mouth_map is not None:
            idx = torch.as_tensor(list(mouth_map), dtype=torch.long)
            mouth = F.mse_loss(xp.reshape(B, T, V // 3, 3)[:, :, idx, :], xv.reshape(B, T, V // 3, 3)[:, :, idx, :])
        loss = mse + 5 * mouth
        loss.backward()
    grads = {PRE + n: p.grad for n, p in lstm.named_parameters()}
    grads.update({"vertice_map_reverse.0.weight": l1.weight.grad, "vertice_map_reverse.0.bias": l1.bias.grad,
                  "vertice_map_reverse.2.weight": l2.weight.grad, "vertice_map_reverse.2.bias": l2.bias.grad})
    return (loss.detach(), mse.detach(), mouth.detach()), grads, xp.detach()
