"""CPU checker for beam search (dimx_generate_beam): oracle.ref_cpu's cached decoder loop (xt_decoder_layers with ``cache``) over
B x W rows, every step decided by the definition dimx.beam.beam_step and followed by the reorder of the self-attention caches by
parent row (``c["k"][rows]``).  Step t consumes the token at position t and produces position t + 1, as in tests/prompt_ref.py."""
import numpy as np
import torch
import torch.nn.functional as F

from dimx import beam, scoring
from oracle import ref_cpu


def beam_generate(sd, prompt, plen, lens, seq_len, T, W, context, context_mask, prefix="decoder_joint.net.", depth=4, heads=12):
    """prompt [B, Pmax] int64 (Pmax = 1: the start tokens), plen [B] or None, lens [B] -> dict of
    tokens [B*W, seq_len] (whole hypotheses, best first), scores [B*W], backptr [B*W, seq_len],
    logits [B*W, seq_len, 512] (rows in the order each step ran in), and per step c: parent / token [seq_len, B, W],
    cum [seq_len, B, W] (after the step), margins [seq_len, B, 2] (keep, order; inf for a step that is not live)."""
    B, Pmax = prompt.shape
    prompt = prompt.clamp(min=0)
    plen_a = None if plen is None else np.asarray(plen)
    first, last = scoring.scored_columns(T, seq_len, np.asarray(lens), plen_a)
    ctx = context.repeat_interleave(W, 0)
    cmask = context_mask.repeat_interleave(W, 0)
    inp = prompt[:, 0].repeat_interleave(W)
    cache = [dict() for _ in range(depth)]
    cum = np.stack([beam.start_scores(W) for _ in range(B)])
    tokens = np.zeros((B, W, seq_len), dtype=np.int32)
    backptr = np.zeros((B, W, seq_len), dtype=np.int32)
    out = dict(logits=[], parent=[], token=[], cum=[], margins=[])
    for c in range(seq_len):
        h = sd[prefix + "token_emb.emb.weight"][inp[:, None]]
        h = ref_cpu.xt_decoder_layers(sd, prefix, h, ctx, cmask, None, None, depth, heads, cache)
        logits = F.linear(h[:, -1], sd[prefix + "to_logits.weight"], sd.get(prefix + "to_logits.bias"))
        out["logits"].append(logits)
        lg = logits.numpy().reshape(B, W, -1)
        par_c, tok_c, mar_c = np.zeros((B, W), np.int32), np.zeros((B, W), np.int32), np.full((B, 2), np.inf)
        for b in range(B):
            mode = beam.column_mode(c, int(first[b]), int(last[b]))
            if mode == beam.LIVE:
                mar_c[b] = beam.margins(lg[b], cum[b])
            par_c[b], tok_c[b], cum[b] = beam.beam_step(lg[b], cum[b], mode, int(prompt[b, c + 1]) if mode == beam.FORCED else 0)
            tokens[b], backptr[b] = tokens[b][par_c[b]], backptr[b][par_c[b]]
            tokens[b, :, c], backptr[b, :, c] = tok_c[b], par_c[b]
        rows = torch.from_numpy((np.arange(B)[:, None] * W + par_c).reshape(-1).astype(np.int64))
        for cc in cache:
            cc["k"], cc["v"] = cc["k"][rows], cc["v"][rows]
        inp = torch.from_numpy(tok_c.reshape(-1).astype(np.int64))
        out["parent"].append(par_c)
        out["token"].append(tok_c)
        out["cum"].append(cum.copy())
        out["margins"].append(mar_c)
    res = {k: np.stack(v) for k, v in out.items() if k != "logits"}
    res["logits"] = torch.stack(out["logits"], 1)
    res.update(tokens=tokens.reshape(B * W, seq_len), scores=cum.reshape(-1).copy(), backptr=backptr.reshape(B * W, seq_len))
    return res
