"""CPU checker for prompted generation (dimx_generate_prompted): oracle.ref_cpu.ar_generate's cached loop
(xt_decoder_layers with ``cache``, sample_tokens) with the sampled token overridden by the prompt's own token while
``t + 1 < plen``.  Step t consumes the token at position t and produces position t + 1; a negative prompt entry (the -100
padding of forward_vq) counts as token 0, as dimx_decode_tf treats it."""
import torch
import torch.nn.functional as F

from oracle import ref_cpu


def case_context(sd, v_s, v_a, mask):
    """the decoder context of a tests/test_gpu_s2s.py ``_case``"""
    x_s = ref_cpu.slmft_forward_encoder(sd, v_s, mask)
    return ref_cpu.slmft_context(sd, x_s, v_a)


def prompted_generate(sd, prompt, plen, seq_len, context, context_mask, noise=None, temperature=1.0, k=52,
                      prefix="decoder_joint.net.", depth=4, heads=12):
    """prompt [B,Pmax] int64, plen [B] (1 <= plen <= Pmax) or None (= Pmax for every clip).  Returns (tokens [B,seq_len]
    -- column c is position c + 1, columns < plen - 1 hold the prompt's own tokens -- and the per-step logits
    [B,seq_len,512])."""
    B, Pmax = prompt.shape
    prompt = prompt.clamp(min=0)
    plen = torch.full((B,), Pmax, dtype=torch.long) if plen is None else torch.as_tensor(plen, dtype=torch.long)
    assert int(plen.min()) >= 1 and int(plen.max()) <= Pmax
    out = prompt[:, :1]
    cache = [dict() for _ in range(depth)]
    all_logits = []
    for t in range(seq_len):
        h = sd[prefix + "token_emb.emb.weight"][out[:, -1:]]
        h = ref_cpu.xt_decoder_layers(sd, prefix, h, context, context_mask, None, None, depth, heads, cache)
        logits = F.linear(h[:, -1], sd[prefix + "to_logits.weight"], sd.get(prefix + "to_logits.bias"))
        all_logits.append(logits)
        tok = ref_cpu.sample_tokens(logits, None if noise is None else noise[t], temperature, k)
        if t + 1 < Pmax:
            tok = torch.where(t + 1 < plen, prompt[:, t + 1], tok)
        out = torch.cat([out, tok.view(B, 1)], dim=1)
    return out[:, 1:], torch.stack(all_logits, 1)
