"""CPU checker for generation over FP8 self-attention K/V caches (dimx_set_self_kv8; the definition is dimx/kv8.py self_step).

oracle.ref_cpu's cached decoder loop attends over the step's own UNQUANTISED key, so this checker owns its loop, built from
ref_cpu._xt_norm, xt_attention(kv=...) and xt_ff.  The self rows of layer i for the positions <= t come from a hook (``SelfRows``):
either given dequantised rows (a device buffer's own), or the checker's own k_new / v_new through the definition
(kv8.quantize / kv8.dequantize), or -- quantisation switched off -- the plain rows, which makes the loop online_ref.online_generate's.
Forced tokens, the window and the margins are that loop's; ``follow`` replays along given tokens, ``samples`` repeats every clip."""
import numpy as np
import torch
import torch.nn.functional as F

from dimx import kv8, online
from oracle import ref_cpu

PREFIX = "decoder_joint.net."


class SelfRows:
    """The hook: ``rows(i, t, k_new, v_new)`` -> (k, v) [R, H, t + 1, 64] float32 of layer i.  ``given[i]`` = (k, v) [R, H, >= t + 1, 64]
    dequantised rows to read instead of the checker's own (None: the layer keeps its own); the own rows of the layers in
    ``quant_layers`` go through the definition, the others stay plain.  ``new[i]`` collects the checker's own k_new / v_new per step."""

    def __init__(self, depth=4, given=None, quant_layers=()):
        self.given = [None] * depth if given is None else list(given)
        self.quant = set(quant_layers)
        self.own = [None] * depth
        self.new = [([], []) for _ in range(depth)]

    def rows(self, i, t, k_new, v_new):
        self.new[i][0].append(k_new)
        self.new[i][1].append(v_new)
        if self.given[i] is not None:
            k, v = self.given[i]
            return k[:, :, :t + 1], v[:, :, :t + 1]
        if i in self.quant:
            k_new, v_new = (torch.from_numpy(kv8.dequantize(*kv8.quantize(x.numpy()))) for x in (k_new, v_new))
        self.own[i] = (k_new, v_new) if self.own[i] is None else tuple(torch.cat([a, b], 2) for a, b in zip(self.own[i], (k_new, v_new)))
        return self.own[i]

    def new_rows(self):
        """[(k_new, v_new)] [R, H, steps, 64]: what the checker itself projected at every step"""
        return [(torch.cat(k, 2), torch.cat(v, 2)) for k, v in self.new]


def dequantized(layers, n):
    """[(kcodes, vcodes, kscale, vscale)] as a device buffer holds them -> [(k, v)] float32 [R, H, n, 64]"""
    out = []
    for kc, vc, ks, vs in layers:
        k = kv8.dequantize(kc.cpu().numpy()[:, :, :n], ks.cpu().numpy()[:, :, :n])
        v = kv8.dequantize(vc.cpu().numpy()[:, :, :n], vs.cpu().numpy()[:, :, :n])
        out.append((torch.from_numpy(np.ascontiguousarray(k)), torch.from_numpy(np.ascontiguousarray(v))))
    return out


def half_spacing(codes):
    """half the distance between neighbouring e4m3fn values at each code (uint8 array): what rounding to that code may have moved"""
    e = (np.asarray(codes, dtype=np.uint8) >> 3) & 15
    return np.exp2(np.maximum(e.astype(np.int32), 1) - 7 - 3 - 1).astype(np.float32)


def self_kv8_generate(sd, prompt, plen, seq_len, context, context_mask, lookahead, hook, noise=None, temperature=1.0, k=52,
                      cross_kv=None, follow=None, samples=1, prefix=PREFIX, depth=4, heads=12):
    """online_ref.online_generate with the self rows of every layer supplied by ``hook`` (a SelfRows).  ``cross_kv``: [(k, v)]
    [B, H, J, 64] per layer instead of the projection of ``context`` (then only asked for its shape).  ``samples`` S: rows are
    b * S + s, noise [seq_len, B * S, 512].  ``follow`` [R, seq_len]: the token fed to step t + 1 is follow[:, t], whatever the step
    chose.  Returns (the steps' own choices [R, seq_len], per-step logits, per-step decision margins)."""
    from online_ref import decision_margin
    rep = lambda x: x.repeat_interleave(samples, 0) if samples > 1 else x
    B, Pmax = prompt.shape
    prompt = rep(prompt.clamp(min=0))
    plen = torch.full((B,), Pmax, dtype=torch.long) if plen is None else torch.as_tensor(plen, dtype=torch.long)
    assert int(plen.min()) >= 1 and int(plen.max()) <= Pmax
    plen = rep(plen)
    R = B * samples
    n_keys = context.shape[1]
    cols = torch.arange(n_keys)
    mask = rep(context_mask)
    if cross_kv is None:
        cross_kv = []
        for i in range(depth):
            pc = "{}attn_layers.layers.{}.1.".format(prefix, 3 * i + 1)
            cross_kv.append(tuple(F.linear(context, sd[pc + w]).view(B, n_keys, heads, 64).permute(0, 2, 1, 3) for w in ("to_k.weight", "to_v.weight")))
    cross_kv = [(rep(ck), rep(cv)) for ck, cv in cross_kv]
    last = prompt[:, :1]
    toks, all_logits, margins = [], [], []
    for t in range(seq_len):
        cm = mask if lookahead is None else mask & (cols < online.visible(t, lookahead, n_keys))[None, :]
        h = sd[prefix + "token_emb.emb.weight"][last]
        for i in range(depth):
            ps = "{}attn_layers.layers.{}.".format(prefix, 3 * i)
            y = ref_cpu._xt_norm(h, sd, ps + "0.0.weight")
            k_new = F.linear(y, sd[ps + "1.to_k.weight"]).view(R, 1, heads, 64).permute(0, 2, 1, 3)
            v_new = F.linear(y, sd[ps + "1.to_v.weight"]).view(R, 1, heads, 64).permute(0, 2, 1, 3)
            o, _ = ref_cpu.xt_attention(y, None, sd, ps + "1.", heads, kv=hook.rows(i, t, k_new, v_new))
            h = h + o
            pc = "{}attn_layers.layers.{}.".format(prefix, 3 * i + 1)
            y = ref_cpu._xt_norm(h, sd, pc + "0.0.weight")
            o, _ = ref_cpu.xt_attention(y, None, sd, pc + "1.", heads, key_mask=cm, kv=cross_kv[i])
            h = h + o
            pf = "{}attn_layers.layers.{}.".format(prefix, 3 * i + 2)
            h = h + ref_cpu.xt_ff(ref_cpu._xt_norm(h, sd, pf + "0.0.weight"), sd, pf + "1.")
        h = ref_cpu._xt_norm(h, sd, prefix + "attn_layers.final_norm.weight")
        logits = F.linear(h[:, -1], sd[prefix + "to_logits.weight"], sd.get(prefix + "to_logits.bias"))
        all_logits.append(logits)
        nz = None if noise is None else noise[t]
        margin = decision_margin(logits, nz, temperature, k)
        tok = ref_cpu.sample_tokens(logits, nz, temperature, k)
        if t + 1 < Pmax:
            tok = torch.where(t + 1 < plen, prompt[:, t + 1], tok)
            margin = torch.where(t + 1 < plen, torch.full_like(margin, float("inf")), margin)   # a forced step decides nothing
        margins.append(margin)
        toks.append(tok.view(R))
        last = (tok if follow is None else follow[:, t]).view(R, 1)
    return torch.stack(toks, 1), torch.stack(all_logits, 1), torch.stack(margins, 1)
