"""CPU checker for online generation (dimx_set_cross_lookahead; the definition is dimx/online.py): prompt_ref.prompted_generate's
loop over oracle.ref_cpu.xt_decoder_layers(..., cache), with the context mask of step t narrowed to the rows the step may see,
``context_mask & (j < visible(t, lookahead, T))``.  The self-attention K/V a step cached under its own visibility stay, as in a
running system.  Tokens may be forced (a prompt with per-clip lengths, as in prompt_ref); a negative entry counts as token 0."""
import torch
import torch.nn.functional as F

from dimx import online
from oracle import ref_cpu


def decision_margin(logits, noise=None, temperature=1.0, k=52):
    """How far the step's decision is from flipping, [B]: top-1 minus top-2 of what the arg-max is taken over -- the raw logits
    for greedy, log softmax(top_k(logits) / temperature) - log(noise) for a noisy step (ref_cpu.sample_tokens)."""
    if noise is None:
        val = logits
    else:
        val = F.log_softmax(ref_cpu.top_k_filter(logits, k) / temperature, dim=-1) - noise.log()
    top = torch.topk(val, 2, dim=-1).values
    return top[:, 0] - top[:, 1]


def online_generate(sd, prompt, plen, seq_len, context, context_mask, lookahead, noise=None, temperature=1.0, k=52,
                    prefix="decoder_joint.net.", depth=4, heads=12):
    """prompt [B,Pmax] int64 (Pmax = 1: the start tokens of a free generation), plen [B] or None (= Pmax): while t + 1 < plen the
    step's token is the prompt's.  lookahead None = the window off.  Returns (tokens [B,seq_len] -- column c is position c + 1 --,
    per-step logits [B,seq_len,512], per-step decision margins [B,seq_len])."""
    B, Pmax = prompt.shape
    prompt = prompt.clamp(min=0)
    plen = torch.full((B,), Pmax, dtype=torch.long) if plen is None else torch.as_tensor(plen, dtype=torch.long)
    assert int(plen.min()) >= 1 and int(plen.max()) <= Pmax
    n_keys = context.shape[1]
    cols = torch.arange(n_keys)
    out = prompt[:, :1]
    cache = [dict() for _ in range(depth)]
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
            margin = torch.where(t + 1 < plen, torch.full_like(margin, float("inf")), margin)   # a forced step decides nothing
        margins.append(margin)
        out = torch.cat([out, tok.view(B, 1)], dim=1)
    return out[:, 1:], torch.stack(all_logits, 1), torch.stack(margins, 1)


def compared_steps(margins, min_margin):
    """[B, n] boolean: the (clip, step) pairs a device run is compared on -- those before the clip's first step whose margin is
    below ``min_margin`` (a near-tie the device may resolve the other way; everything after it follows another history).  Also
    returns the share of pairs left out."""
    B, n = margins.shape
    close = margins < min_margin
    first = torch.where(close.any(1), close.float().argmax(1), torch.full((B,), n))
    keep = torch.arange(n)[None, :] < first[:, None]
    return keep, 1.0 - keep.sum().item() / float(B * n)
