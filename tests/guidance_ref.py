"""CPU checker for guided generation (dimx_generate_guided; the definition is dimx/guidance.py): online_ref.online_generate over
oracle.ref_cpu, run once per branch -- under the clip's context, and under a context of zero rows -- along the SAME tokens, the two
logit rows of every step combined by dimx.guidance.combine and sampled by the definition of dimx/sampling.py.

``force`` [B,seq_len] (column c is position c + 1): both branches are run along these tokens, e.g. a device run's own, so that a
near-tie the device resolved the other way costs that one (clip, step) pair and not the rest of the clip.  Without it the checker
generates: step by step, each step's branches forced along the tokens chosen so far (the decoder is causal, so re-running a prefix
changes nothing of it; n passes of online_generate per branch -- for small cases)."""
import numpy as np
import torch

import online_ref
from dimx import guidance, sampling


def null_context(context):
    """the unconditional branch's context: zero rows *after* the concat [x_s + patch_embed_dec_s | audio]"""
    return torch.zeros_like(context)


def _branches(sd, first, tokens, seq_len, context, context_mask, lookahead):
    """both branches' per-step logits [B,seq_len,512] along ``tokens`` [B,m] (m <= seq_len forced columns; the rest is whatever the
    branch's own greedy continuation is and is not used by the callers)"""
    B = first.shape[0]
    prompt = torch.cat([first.view(B, 1), tokens], dim=1)
    c = online_ref.online_generate(sd, prompt, None, seq_len, context, context_mask, lookahead)[1]
    u = online_ref.online_generate(sd, prompt, None, seq_len, null_context(context), context_mask, lookahead)[1]
    return c, u


def sample_guided(g, noise_t, temperature, kind, kw):
    """the definition's token for guided logits g [B,512] (float64): greedy without noise or at temperature 0"""
    if noise_t is None or temperature <= 0:
        return g.argmax(axis=1)
    return sampling.sample_ref(g, np.asarray(noise_t, dtype=np.float64), temperature, kind, **kw)


def guided_generate(sd, prompt, plen, seq_len, context, context_mask, scale, lookahead=None, noise=None, temperature=1.0,
                    kind="top_k", kw=None, force=None):
    """prompt [B,Pmax] int64 / plen as online_ref.online_generate (forced while t + 1 < plen).  Returns a dict: ``tokens``
    [B,seq_len] int64 (the definition's token on every step's own guided logits; the prompt's inside it), ``cond`` / ``uncond``
    [B,seq_len,512] float32 branch logits, ``guided`` float64 = combine(cond, uncond, scale)."""
    kw = {"k": 52} if kw is None and kind == "top_k" else (kw or {})
    B, Pmax = prompt.shape
    prompt = prompt.clamp(min=0)
    plen_t = torch.full((B,), Pmax, dtype=torch.long) if plen is None else torch.as_tensor(plen, dtype=torch.long)

    def pick(t, g_t):
        tok = torch.from_numpy(np.asarray(sample_guided(g_t, None if noise is None else noise[t].numpy(), temperature, kind, kw))).long()
        if t + 1 < Pmax:
            tok = torch.where(t + 1 < plen_t, prompt[:, t + 1], tok)
        return tok

    if force is not None:
        force = torch.as_tensor(force).long()
        c, u = _branches(sd, prompt[:, 0], force, seq_len, context, context_mask, lookahead)
        g = guidance.combine(c.numpy(), u.numpy(), scale)
        tokens = torch.stack([pick(t, g[:, t]) for t in range(seq_len)], dim=1)
        return {"tokens": tokens, "cond": c, "uncond": u, "guided": g}
    tokens = torch.zeros(B, 0, dtype=torch.long)
    for t in range(seq_len):
        c, u = _branches(sd, prompt[:, 0], tokens, t + 1, context, context_mask, lookahead)
        g = guidance.combine(c.numpy(), u.numpy(), scale)
        tokens = torch.cat([tokens, pick(t, g[:, t]).view(B, 1)], dim=1)
    return {"tokens": tokens, "cond": c, "uncond": u, "guided": g}
