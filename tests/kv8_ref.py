"""CPU checker for generation over FP8 cross K/V (dimx_set_cross_kv8; the definition is dimx/kv8.py): online_ref.online_generate's
loop with every layer's cross K / V -- ``cache[i]["ck"]`` / ``["cv"]`` of oracle.ref_cpu.xt_decoder_layers, which uses cached cross
K/V when present -- pre-filled from given dequantised rows.  Everything else (forced tokens, the window, margins) is that loop."""
import numpy as np
import torch
import torch.nn.functional as F

from dimx import kv8, online
from oracle import ref_cpu

PREFIX = "decoder_joint.net."


def cross_kv(sd, context, depth=4, heads=12, prefix=PREFIX):
    """the checker's own cross K / V of every layer, [(k, v)] of [B, H, J, 64] float32 (what xt_decoder_layers caches)"""
    B, J, _ = context.shape
    out = []
    for i in range(depth):
        pc = "{}attn_layers.layers.{}.1.".format(prefix, 3 * i + 1)
        k = F.linear(context, sd[pc + "to_k.weight"]).view(B, J, heads, 64).permute(0, 2, 1, 3)
        v = F.linear(context, sd[pc + "to_v.weight"]).view(B, J, heads, 64).permute(0, 2, 1, 3)
        out.append((k, v))
    return out


def through_kv8(kv):
    """[(k, v)] float32 -> the same rows through kv8.quantize / kv8.dequantize"""
    out = []
    for k, v in kv:
        out.append(tuple(torch.from_numpy(kv8.dequantize(*kv8.quantize(t.numpy()))) for t in (k, v)))
    return out


def dequantized(layers, J):
    """[(kcodes, vcodes, kscale, vscale)] as a device buffer holds them (tensors, [B, H, Tp, ...]) -> [(k, v)] float32 [B, H, J, 64]"""
    out = []
    for kc, vc, ks, vs in layers:
        k = kv8.dequantize(kc.cpu().numpy()[:, :, :J], ks.cpu().numpy()[:, :, :J])
        v = kv8.dequantize(vc.cpu().numpy()[:, :, :J], vs.cpu().numpy()[:, :, :J])
        out.append((torch.from_numpy(np.ascontiguousarray(k)), torch.from_numpy(np.ascontiguousarray(v))))
    return out


def kv8_generate(sd, prompt, plen, seq_len, context, context_mask, lookahead, kv, noise=None, temperature=1.0, k=52,
                 prefix=PREFIX, depth=4, heads=12):
    """online_ref.online_generate with the cross K / V of layer i taken from kv[i] = (k, v) [B, H, J, 64] instead of projected from
    ``context`` (which is then only asked for its shape).  Returns (tokens, per-step logits, per-step decision margins)."""
    from online_ref import decision_margin
    B, Pmax = prompt.shape
    prompt = prompt.clamp(min=0)
    plen = torch.full((B,), Pmax, dtype=torch.long) if plen is None else torch.as_tensor(plen, dtype=torch.long)
    assert int(plen.min()) >= 1 and int(plen.max()) <= Pmax
    n_keys = context.shape[1]
    cols = torch.arange(n_keys)
    out = prompt[:, :1]
    cache = [{"ck": kv[i][0], "cv": kv[i][1]} for i in range(depth)]
    all_logits, margins = [], []
    for t in range(seq_len):
        cm = context_mask if lookahead is None else context_mask & (cols < online.visible(t, lookahead, n_keys))[None, :]
        h = sd[prefix + "token_emb.emb.weight"][out[:, -1:]]
        h = ref_cpu.xt_decoder_layers(sd, prefix, h, context, cm, None, None, depth, heads, cache)
        logits = F.linear(h[:, -1], sd[prefix + "to_logits.weight"], sd.get(prefix + "to_logits.bias"))
        all_logits.append(logits)
        nz = None if noise is None else noise[t]
        margin = decision_margin(logits, nz, temperature, k)
        tok = ref_cpu.sample_tokens(logits, nz, temperature, k)
        if t + 1 < Pmax:
            tok = torch.where(t + 1 < plen, prompt[:, t + 1], tok)
            margin = torch.where(t + 1 < plen, torch.full_like(margin, float("inf")), margin)
        margins.append(margin)
        out = torch.cat([out, tok.view(B, 1)], dim=1)
    return out[:, 1:], torch.stack(all_logits, 1), torch.stack(margins, 1)
