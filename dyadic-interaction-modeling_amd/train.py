"""Training step of the DIM-Listener fine-tuning model: reference ``train_epoch``
(code/x_engine_pt.py:9-60) as driven by code/finetune_s2s_pretrain.py:105-143 (AdamW lr 1e-5, clip 1.0, frozen VQ-VAEs).

What is differentiated is the teacher-forced path of ``SLMFT.forward(mode='train')`` (code/seq2seq_pretrain.py:496-514):
encoder_s -> encoder_joint -> norm_s -> context -> AutoregressiveWrapper.forward -> cross entropy.  The continuous
loss has no gradient path in the reference either (its ``pred`` comes from an argmax / one-hot of the logits, :454-464),
and both VQ-VAEs are frozen (:348-366), so the listener code targets and the decoded motion are taken from the HIP engine
(no graph).

Two implementations of that step live in the package:
  * ``dimx.train_hip.HipTrainer`` -- forward + backward + clip + AdamW on hand-written HIP kernels (csrc/train.hip), the
    one ``x_engine_pt.train_epoch`` uses when it is handed a HipTrainer;
  * this module -- the same mathematics on PyTorch-ROCm autograd (rocBLAS / hipBLASLt GEMMs), kept as the
    ``torch.optim`` route of ``train_epoch`` and as the functional layers the LEGACY generator's loop (``legacy_loss``,
    reference code/x_engine.py:8-36) differentiates.  After ``optimizer.step()`` the engine notices the changed
    parameters and re-packs them before its next launch.

Multi-GPU: one process per GPU, replicated weights, per-rank batch shard; ``all_reduce_grads`` averages the gradients in
~64 MiB flat buckets over RCCL (xGMI ring: a few large collectives instead of one per tensor) before clipping.
"""
import math

import torch
import torch.nn.functional as F

from . import dist as ddist

FROZEN_PREFIXES = ("speaker_vq.", "listener_vq.")


def trainable_parameters(model):
    """(name, parameter) of everything the reference trains: all but the two VQ-VAEs (and their ``pe`` buffers)."""
    return [(n, p) for n, p in model.named_parameters() if not n.startswith(FROZEN_PREFIXES)]


def set_trainable(model, flag=True):
    for _, p in trainable_parameters(model):
        p.requires_grad_(flag)
    return model


# ---------------------------------------------------------------------------------------------------------------------
# x-transformers 1.30.16 layers, functional, on a {key: tensor} view of the module's own parameters
# ---------------------------------------------------------------------------------------------------------------------
def _ln(x, w, b=None):
    return F.layer_norm(x, (x.shape[-1],), w, b, 1e-5)


def _attention(x, ctx, P, pre, heads, key_mask=None, attn_mask=None):
    B, n, _ = x.shape
    q = F.linear(x, P[pre + "to_q.weight"]).view(B, n, heads, -1).transpose(1, 2)
    k = F.linear(ctx, P[pre + "to_k.weight"]).view(B, ctx.shape[1], heads, -1).transpose(1, 2)
    v = F.linear(ctx, P[pre + "to_v.weight"]).view(B, ctx.shape[1], heads, -1).transpose(1, 2)
    dots = torch.matmul(q, k.transpose(-1, -2)) * (q.shape[-1] ** -0.5)
    neg = -torch.finfo(dots.dtype).max
    if key_mask is not None:
        dots = dots.masked_fill(~key_mask[:, None, None, :], neg)
    if attn_mask is not None:
        dots = dots.masked_fill(~attn_mask, neg)
    out = torch.matmul(dots.softmax(dim=-1, dtype=torch.float32).to(dots.dtype), v)
    return F.linear(out.transpose(1, 2).reshape(B, n, -1), P[pre + "to_out.weight"])


def _ff(x, P, pre):
    h = F.gelu(F.linear(x, P[pre + "ff.0.0.weight"], P[pre + "ff.0.0.bias"]))
    return F.linear(h, P[pre + "ff.2.weight"], P[pre + "ff.2.bias"])


def xt_encoder(P, pre, x, mask, causal, depth, heads):
    """ContinuousTransformerWrapper(..., return_embeddings=True) with an Encoder of (attention, feed-forward) x depth."""
    T = x.shape[1]
    h = F.linear(x, P[pre + "project_in.weight"], P.get(pre + "project_in.bias"))   # optional tensor: models._adopt_optional_tensors
    h = h + P[pre + "pos_emb.emb.weight"][:T] * (h.shape[-1] ** -0.5)
    am = torch.ones(T, T, dtype=torch.bool, device=x.device).tril() if causal else None
    L = pre + "attn_layers.layers."
    for i in range(depth):
        h = h + _self(h, P, L, 2 * i, heads, mask, am)
        h = h + _ff(_ln(h, P[L + "%d.0.0.weight" % (2 * i + 1)]), P, L + "%d.1." % (2 * i + 1))
    return _ln(h, P[pre + "attn_layers.final_norm.weight"])


def _self(h, P, L, li, heads, key_mask, attn_mask):
    y = _ln(h, P[L + "%d.0.0.weight" % li])
    return _attention(y, y, P, L + "%d.1." % li, heads, key_mask, attn_mask)


def xt_decoder_logits(P, pre, tokens, context, context_mask, self_kv_mask, depth, heads, pos_emb=False, cross_attn_mask=None):
    """TransformerWrapper(num_tokens, attn_layers=Decoder(cross_attend=True)) on a token prefix -> logits.
    cross_attn_mask: bool, broadcastable to [B, heads, n, keys]; False entries of every layer's cross attention are filled like
    masked keys (``online_cross_mask``: the visibility of an online generation)."""
    n = tokens.shape[1]
    h = P[pre + "token_emb.emb.weight"][tokens]
    if pos_emb:
        h = h + P[pre + "pos_emb.emb.weight"][:n] * (h.shape[-1] ** -0.5)
    causal = torch.ones(n, n, dtype=torch.bool, device=tokens.device).tril()
    L = pre + "attn_layers.layers."
    for i in range(depth):
        h = h + _self(h, P, L, 3 * i, heads, self_kv_mask, causal)
        y = _ln(h, P[L + "%d.0.0.weight" % (3 * i + 1)])
        h = h + _attention(y, context, P, L + "%d.1." % (3 * i + 1), heads, context_mask, cross_attn_mask)
        h = h + _ff(_ln(h, P[L + "%d.0.0.weight" % (3 * i + 2)]), P, L + "%d.1." % (3 * i + 2))
    h = _ln(h, P[pre + "attn_layers.final_norm.weight"])
    return F.linear(h, P[pre + "to_logits.weight"], P.get(pre + "to_logits.bias"))


def online_cross_mask(mask, lookahead):
    """[B, T-1, T] bool: decoder row t (it consumes token t and predicts t+1: step t of dimx.online) keeps context row j iff
    j < visible(t, lookahead, T) and ``mask`` [B, T] keeps j -- ``dimx.online.visible_mask`` on the device of ``mask``."""
    from .online import visible
    T = mask.shape[1]
    vis = torch.as_tensor(visible(range(T - 1), lookahead, T), device=mask.device)                   # [T-1]
    return (torch.arange(T, device=mask.device)[None, :] < vis[:, None])[None] & mask.bool()[:, None, :]


def slmft_loss(P, dims, v_speaker, v_audio, mask, z_l, kv_mask=None, lookahead=None, cond_keep=None):
    """Differentiable l_ce_l of SLMFT.forward(mode='train').  P: {key: tensor} (parameters carry the graph); z_l [B,T]
    listener codes with -100 on padding (from the frozen VQ-VAE); kv_mask [B,T-1] keep-mask (AutoregressiveWrapper's
    mask_prob draw) or None.  lookahead: an integer L trains under the visibility of an online generation (``online_cross_mask``
    on the decoder's cross attention; the checker of dimx_set_train_lookahead), None = the reference's offline step.
    cond_keep [B] (bool or 0/1; ``dimx.guidance.cond_keep``): condition dropout -- a clip with keep = 0 is trained under the null
    context (zero rows after the concat, no rescaling) and sends no gradient into its context; None = every clip keeps its own.
    Returns (loss, logits)."""
    x = v_speaker + P["patch_embed_s"]
    x = xt_encoder(P, "encoder_s.", x, mask, True, dims.enc_depth, dims.heads)
    x = xt_encoder(P, "encoder_joint.", x, mask, True, dims.enc_depth, dims.heads)
    x_s = _ln(x, P["norm_s.weight"], P["norm_s.bias"])
    ctx = torch.cat([x_s + P["patch_embed_dec_s"], v_audio], dim=-1)
    if cond_keep is not None:
        ctx = ctx * torch.as_tensor(cond_keep, device=ctx.device).to(ctx.dtype)[:, None, None]
    inp = z_l[:, :-1].clamp(min=0)                                   # pad_value 0 where the target is ignored
    cam = None if lookahead is None else online_cross_mask(mask, lookahead)[:, None]
    logits = xt_decoder_logits(P, "decoder_joint.net.", inp, ctx, mask, kv_mask, dims.dec_depth, dims.heads, cross_attn_mask=cam)
    loss = F.cross_entropy(logits.reshape(-1, logits.shape[-1]), z_l[:, 1:].reshape(-1), ignore_index=-100)
    return loss, logits


# ---------------------------------------------------------------------------------------------------------------------
# legacy ListenerGenerator (reference code/seq2seq.py:138-278) -- what code/x_engine.py:8-36 trains
# ---------------------------------------------------------------------------------------------------------------------
LEGACY_TRAINABLE_PREFIXES = ("generator.", "listener_vq.decoder.", "speaker_embeddings.", "listener_embeddings.",
                             "fc_speaker.", "fc_listener.")


def legacy_trainable_parameters(model):
    """reference code/seq2seq.py:165-176: the speaker VQ-VAE and the listener VQ-VAE's encoder + codebook are frozen,
    the listener VQ-VAE's DECODER, the generator and the id-embedding layers train."""
    return [(n, p) for n, p in model.named_parameters() if n.startswith(LEGACY_TRAINABLE_PREFIXES)]


def set_legacy_trainable(model, flag=True):
    for _, p in legacy_trainable_parameters(model):
        p.requires_grad_(flag)
    return model


def _gelu_tanh(x):
    return x * (0.5 * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x * x * x))))


def _vq_blocks(P, net, h, heads, layers):
    """``layers`` pre-LN {attention with packed qkv and scale hidden^-0.5, tanh-GELU MLP} blocks of the VQ-VAE's Transformer
    (reference code/models/lib/base_models.py); net: the "...transformer.net." prefix."""
    B, n, H = h.shape
    for i in range(layers):
        a = "%s%d.fn." % (net, 2 * i)
        y = F.layer_norm(h, (H,), P[a + "norm.weight"], P[a + "norm.bias"], 1e-5)
        q, k, v = F.linear(y, P[a + "fn.to_qkv.weight"]).view(B, n, 3, heads, H // heads).permute(2, 0, 3, 1, 4)
        att = torch.softmax(torch.matmul(q, k.transpose(-1, -2)) * (H ** -0.5), dim=-1)
        o = torch.matmul(att, v).transpose(1, 2).reshape(B, n, H)
        h = h + F.linear(o, P[a + "fn.to_out.weight"], P[a + "fn.to_out.bias"])
        m = "%s%d.fn." % (net, 2 * i + 1)
        y = F.layer_norm(h, (H,), P[m + "norm.weight"], P[m + "norm.bias"], 1e-5)
        y = _gelu_tanh(F.linear(y, P[m + "fn.l1.weight"], P[m + "fn.l1.bias"]))
        h = h + F.linear(y, P[m + "fn.l2.weight"], P[m + "fn.l2.bias"])
    return h


def _instance_norm(x, eps=1e-5):
    """F.instance_norm over the last dim of [B,C,n]; torch refuses a single frame (n = 1), where the definition still holds
    (mean = x, biased variance 0: the output is zero and passes no gradient)"""
    if x.shape[-1] > 1:
        return F.instance_norm(x, eps=eps)
    xm = x - x.mean(-1, keepdim=True)
    return xm * torch.rsqrt(x.var(-1, unbiased=False, keepdim=True) + eps)


def vq_decoder(P, pre, zq, heads, layers, pe, drop=None):
    """Differentiable TransformerDecoder of the listener VQ-VAE (reference code/models/stage1_BIWI.py:376-393): linear,
    Conv1d(k5, replicate) + LeakyReLU(0.2) + InstanceNorm over time, linear, + pe[batch row], ``layers`` pre-LN
    {attention with packed qkv and scale hidden^-0.5, tanh-GELU MLP} blocks, bias-free output map.  zq [B,L,128].
    drop: optional [B,L,hidden] multiplier of the PositionalEncoding's dropout (train mode; None = eval)."""
    B, n, _ = zq.shape
    c = pre + "decoder."
    h = F.linear(zq, P[c + "decoder_linear_embedding_pre.net.weight"], P[c + "decoder_linear_embedding_pre.net.bias"])
    x = F.conv1d(F.pad(h.transpose(1, 2), (2, 2), mode="replicate"), P[c + "expander.0.0.weight"], P[c + "expander.0.0.bias"])
    h = _instance_norm(F.leaky_relu(x, 0.2)).transpose(1, 2)
    h = F.linear(h, P[c + "decoder_linear_embedding.net.weight"], P[c + "decoder_linear_embedding.net.bias"])
    h = h + pe[:B]
    if drop is not None:
        h = h * drop
    h = _vq_blocks(P, c + "decoder_transformer.net.", h, heads, layers)
    return F.linear(h, P[c + "vertice_map_reverse.weight"])


def vq_encoder(P, pre, x, heads, layers, pe, drop=None):
    """Differentiable TransformerEncoder of the VQ-VAE (reference code/models/stage1_BIWI.py:254-317, quant_factor 0):
    Linear + LeakyReLU(0.2), Conv1d(k5, replicate) + LeakyReLU + InstanceNorm over time, linear, + pe[batch row] (then the
    PositionalEncoding's dropout multiplier ``drop``), the pre-LN blocks, linear -> z [B,L,128]."""
    B = x.shape[0]
    c = pre + "encoder."
    h = F.leaky_relu(F.linear(x, P[c + "vertice_mapping.0.weight"], P[c + "vertice_mapping.0.bias"]), 0.2)
    y = F.conv1d(F.pad(h.transpose(1, 2), (2, 2), mode="replicate"), P[c + "squasher.0.0.weight"], P[c + "squasher.0.0.bias"])
    h = F.instance_norm(F.leaky_relu(y, 0.2), eps=1e-5).transpose(1, 2)
    h = F.linear(h, P[c + "encoder_linear_embedding.net.weight"], P[c + "encoder_linear_embedding.net.bias"])
    h = h + pe[:B]
    if drop is not None:
        h = h * drop
    h = _vq_blocks(P, c + "encoder_transformer.net.", h, heads, layers)
    return F.linear(h, P[c + "encoder_linear_embedding_post.net.weight"], P[c + "encoder_linear_embedding_post.net.bias"])


def vq_loss(P, x, masks=None, beta=0.25, quant_loss_weight=1.0, pre="", heads=8, layers=6, idx=None):
    """Differentiable stage-1 step of the reference (code/train_vq.py:173-196): ``VQAutoEncoder.forward`` (encoder, quantiser
    code/models/lib/quantizer.py:35-66, decoder on the straight-through latent) and ``calc_vq_loss`` (code/metrics/loss.py:6-11).
    P: {key: tensor} of one VQ-VAE (keys ``pre + "encoder."...``, its pe buffers included); x [B,T,in_dim].  masks: None (eval,
    no dropout) or (enc, dec) [B,T,hidden] dropout multipliers (dimx.prng.dropout_scale_mask).  idx: optional [B*T] code indices
    to use instead of the argmin (a checker that follows another implementation's choice at a near tie).
    Returns (loss, rec_loss, quant_loss, perplexity, pred [B,T,in_dim], idx [B*T])."""
    B, T, _ = x.shape
    m_enc, m_dec = masks if masks is not None else (None, None)
    z = vq_encoder(P, pre, x, heads, layers, P[pre + "encoder.encoder_pos_embedding.pe"], m_enc)
    E = P[pre + "quantize.embedding.weight"]
    zf = z.reshape(-1, E.shape[1])
    if idx is None:
        with torch.no_grad():
            d = torch.sum(zf ** 2, dim=1, keepdim=True) + torch.sum(E ** 2, dim=1) - 2 * torch.matmul(zf, E.t())
            idx = torch.argmin(d, dim=1)
    idx = idx.reshape(-1).long()
    e = E[idx].view_as(z)
    quant = beta * torch.mean((e.detach() - z) ** 2) + torch.mean((e - z.detach()) ** 2)
    z_st = z + (e - z).detach()
    with torch.no_grad():
        e_mean = torch.bincount(idx, minlength=E.shape[0]).to(z.dtype) / idx.numel()
        perplexity = torch.exp(-torch.sum(e_mean * torch.log(e_mean + 1e-10)))
    pred = vq_decoder(P, pre, z_st, heads, layers, P[pre + "decoder.decoder_pos_embedding.pe"], m_dec)
    rec = F.l1_loss(pred, x)
    return quant_loss_weight * quant + rec, rec, quant, perplexity, pred, idx


def converter_head(P, motion):
    """``vertice_map_reverse(vertice_map_reverse_lstm(motion))`` of EmocaConverter (reference code/seq2seq_pretrain.py:801-819,
    applied at :834-836) with stock torch modules loaded from the state dict P: motion [B,T,56] -> [B,T,V], differentiable in P."""
    pre = "vertice_map_reverse_lstm."
    w0 = P[pre + "weight_ih_l0"]
    lstm = torch.nn.LSTM(w0.shape[1], w0.shape[0] // 4, 2, batch_first=True, bidirectional=True).to(device=w0.device, dtype=w0.dtype)
    flat = []
    for layer in range(2):
        for sfx in ("", "_reverse"):
            flat += [P[pre + "%s_l%d%s" % (n, layer, sfx)] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    names = [n for n, _ in lstm.named_parameters()]
    y, _ = torch.func.functional_call(lstm, dict(zip(names, flat)), (motion,))
    a1 = F.leaky_relu(F.linear(y, P["vertice_map_reverse.0.weight"], P["vertice_map_reverse.0.bias"]), 0.2)
    return F.linear(a1, P["vertice_map_reverse.2.weight"], P["vertice_map_reverse.2.bias"])


def mouth_vertex_weights(mouth_map, n_vertices, device=None):
    """[n_vertices] f32: how often each vertex occurs in ``mouth_map`` (duplicates count, as fancy indexing counts them)"""
    idx = torch.as_tensor([int(i) for i in mouth_map], dtype=torch.long)
    assert idx.numel() > 0 and int(idx.min()) >= 0 and int(idx.max()) < n_vertices, "mouth_map holds vertex indices in [0, V / 3)"
    return torch.bincount(idx, minlength=n_vertices).to(torch.float32).to(device or "cpu")


def converter_loss(model_or_sd, vertices, template, emoca, mouth_map=None, motion=None, vq_heads=8, vq_layers=6):
    """Differentiable step of the reference's converter loop (code/train_converter.py:25-33 over EmocaConverter.forward,
    code/seq2seq_pretrain.py:826-842): the PyTorch-autograd CHECKER of ``ConverterHipTrainer``.
    model_or_sd: the module or {key: tensor}; vertices [B,T,V] (target), template [B,V] or None, emoca [B,T,56].  The frozen
    speaker VQ-VAE runs without a graph in eval arithmetic (``motion`` [B,T,56] may be handed in instead, e.g. the HIP engine's);
    the head is stock ``nn.LSTM`` / ``F.linear`` / ``F.leaky_relu``.  loss = mse + 5 * mse over ``mouth_map`` (mean over all B
    clips; the reference's ``reshape(1, -1, V/3, 3)`` is B = 1, where the two agree).  Returns (loss, mse, mouth, mesh)."""
    P = model_or_sd if isinstance(model_or_sd, dict) else dict(model_or_sd.state_dict(keep_vars=True))
    if motion is None:
        with torch.no_grad():
            Pd = {k: v.detach() for k, v in P.items() if k.startswith("speaker_vq.")}
            motion = vq_loss(Pd, emoca, pre="speaker_vq.", heads=vq_heads, layers=vq_layers)[4]
    mesh = converter_head(P, motion.detach())
    if template is not None:
        mesh = mesh + template[:, None, :]
    B, T, V = mesh.shape
    mse = F.mse_loss(mesh, vertices)
    mouth = mesh.new_zeros(())
    if mouth_map is not None:
        idx = torch.as_tensor([int(i) for i in mouth_map], dtype=torch.long, device=mesh.device)
        mouth = F.mse_loss(mesh.reshape(B, T, V // 3, 3)[:, :, idx, :], vertices.reshape(B, T, V // 3, 3)[:, :, idx, :])
    return mse + 5 * mouth, mse, mouth, mesh


def legacy_loss(P, dims, vq_dims, x_speaker, z_l, v_listener, mask, pe, speaker_ids=None, listener_ids=None):
    """Differentiable ``ListenerGenerator.forward`` (reference code/seq2seq.py:235-278 with Transformer.forward :46-67).
    x_speaker [B,T,1024] and z_l [B,T] (-100 on padding) come from the frozen VQ-VAEs (HIP engine, no graph); ``pe`` is
    the listener decoder's positional buffer.  ``listener_ids`` (the call of code/x_engine.py:24) prepends
    fc_listener(relu(listener_embeddings[id])) to the encoder output, a True to the context mask and a -100 to the
    targets; ``speaker_ids`` prepends fc_speaker(relu(speaker_embeddings[id])) to the encoder INPUT.
    Returns (loss = cross entropy + continuous loss, pred_cont_seq [B,T-1,56], logits [B,T-1,512])."""
    B = x_speaker.shape[0]
    one = torch.ones(B, 1, dtype=torch.bool, device=mask.device)
    cmask = mask
    if speaker_ids is not None:
        sid = F.linear(F.relu(P["speaker_embeddings.weight"][speaker_ids]), P["fc_speaker.weight"], P["fc_speaker.bias"])
        x_speaker = torch.cat([sid[:, None], x_speaker], dim=1)
        cmask = torch.cat([one, cmask], dim=1)
    enc = xt_encoder(P, "generator.encoder.", x_speaker, cmask, False, dims.depth, dims.heads)
    tgt = z_l
    if listener_ids is not None:
        lid = F.linear(F.relu(P["listener_embeddings.weight"][listener_ids]), P["fc_listener.weight"], P["fc_listener.bias"])
        enc = torch.cat([lid[:, None], enc], dim=1)
        cmask = torch.cat([one, cmask], dim=1)
        tgt = torch.cat([torch.full_like(z_l[:, :1], -100), z_l], dim=1)
    inp, target = tgt[:, :-1].clamp(min=0), tgt[:, 1:]
    logits = xt_decoder_logits(P, "generator.decoder.net.", inp, enc, cmask, None, dims.depth, dims.heads, pos_emb=True)
    loss = F.cross_entropy(logits.reshape(-1, logits.shape[-1]), target.reshape(-1), ignore_index=-100)
    if listener_ids is not None:
        logits = logits[:, 1:]
    zq = P["listener_vq.quantize.embedding.weight"][logits.argmax(-1)]
    pred = vq_decoder(P, "listener_vq.", zq, vq_dims.heads, vq_dims.layers, pe)
    m = mask[:, 1:].reshape(-1)
    p = pred.reshape(-1, pred.shape[-1])[m]
    t = v_listener[:, 1:].reshape(-1, pred.shape[-1])[m]
    loss_cont = F.pairwise_distance(p[:, 6:], t[:, 6:]).mean() + F.pairwise_distance(p[:, :6], t[:, :6]).mean()
    return loss + loss_cont, pred, logits


# ---------------------------------------------------------------------------------------------------------------------
# SLM pre-training (reference code/seq2seq_pretrain.py:72-323) -- what code/train_s2s_pretrain.py:41-64 trains with
# x_engine_pt.train_epoch
# ---------------------------------------------------------------------------------------------------------------------
SLM_FROZEN_PREFIXES = ("speaker_vq.encoder.", "speaker_vq.quantize.", "listener_vq.encoder.", "listener_vq.quantize.")


def slm_trainable_parameters(model):
    """reference :98-113: both VQ-VAEs' encoders and codebooks are frozen, their DECODERS and everything else train."""
    return [(n, p) for n, p in model.named_parameters() if not n.startswith(SLM_FROZEN_PREFIXES)]


def set_slm_trainable(model, flag=True):
    for _, p in slm_trainable_parameters(model):
        p.requires_grad_(flag)
    return model


def _masked_pairwise(pred, target, sel):
    m = sel[:, 1:].reshape(-1)
    p = pred.reshape(-1, pred.shape[-1])[m]
    t = target[:, 1:].reshape(-1, pred.shape[-1])[m]
    return F.pairwise_distance(p[:, 6:], t[:, 6:]).mean() + F.pairwise_distance(p[:, :6], t[:, :6]).mean()


def slm_loss(P, dims, vq_dims, v_speaker, v_listener, v_audio, mask, mask_speaker, mask_listener, z_s, z_l, pe_s, pe_l):
    """Differentiable ``SLM.forward`` (reference :300-323): masked speaker / listener streams through encoder_s / encoder_l
    (bidirectional, key padding), the joint encoder over the 2T concatenation and over each stream alone (:200-221), InfoNCE
    between the clip means (:270-289), the two cross-predicting decoders with absolute positional embedding (z_s from the
    listener half of x_joint, z_l from the speaker half, :223-243), and the continuous losses of the decoded arg-max codes,
    which train the two VQ-VAE DECODERS.  z_s / z_l [B,T]: codes from the frozen VQ encoders (HIP engine), unmasked;
    mask_speaker / mask_listener: True = masked frame (its code is a target).  Returns (total, dict)."""
    depth, heads = dims.enc_depth, dims.heads
    vs = (v_speaker + P["patch_embed_s"]).masked_fill(mask_speaker[..., None], 0.0)
    vl = (v_listener + P["patch_embed_l"]).masked_fill(mask_listener[..., None], 0.0)
    x_s = xt_encoder(P, "encoder_s.", vs, mask, False, depth, heads)
    x_l = xt_encoder(P, "encoder_l.", vl, mask, False, depth, heads)
    x_joint = xt_encoder(P, "encoder_joint.", torch.cat([x_s, x_l], dim=1), torch.cat([mask, mask], dim=-1), False, depth, heads)
    x_l = xt_encoder(P, "encoder_joint.", x_l, mask, False, depth, heads)
    x_s = xt_encoder(P, "encoder_joint.", x_s, mask, False, depth, heads)
    x_s, x_l = _ln(x_s, P["norm_s.weight"], P["norm_s.bias"]), _ln(x_l, P["norm_l.weight"], P["norm_l.bias"])
    x_joint = _ln(x_joint, P["norm.weight"], P["norm.bias"])
    valid = mask[..., None].to(x_s.dtype)
    n = valid.sum(1)
    s = F.normalize((x_s * valid).sum(1) / n, dim=-1)
    l_ = F.normalize((x_l * valid).sum(1) / n, dim=-1)
    total = s @ l_.t() / 0.05
    nce = -torch.mean(torch.diag(F.log_softmax(total, dim=0)))
    c_acc = (F.softmax(total.detach(), dim=0).argmax(0) == torch.arange(total.shape[0], device=total.device)).sum() / total.shape[0]
    T = mask.shape[1]
    out = {}
    for tag, z, msk, xj, patch, vq, pe, tgt in (("s", z_s, mask_speaker, x_joint[:, T:], "patch_embed_dec_l", "speaker_vq.", pe_s, v_speaker),
                                                ("l", z_l, mask_listener, x_joint[:, :T], "patch_embed_dec_s", "listener_vq.", pe_l, v_listener)):
        z = torch.where(msk, z, torch.full_like(z, -100))
        ctx = torch.cat([xj + P[patch], v_audio], dim=-1)
        logits = xt_decoder_logits(P, "decoder_joint.net.", z[:, :-1].clamp(min=0), ctx, mask, None, dims.dec_depth, heads, pos_emb=True)
        out["l_ce_" + tag] = F.cross_entropy(logits.reshape(-1, logits.shape[-1]), z[:, 1:].reshape(-1), ignore_index=-100)
        pred = vq_decoder(P, vq, P[vq + "quantize.embedding.weight"][logits.argmax(-1)], vq_dims.heads, vq_dims.layers, pe)
        out["l_cont_" + tag] = _masked_pairwise(pred, tgt, msk)
    out["nce"], out["c_acc"] = nce, c_acc
    return out["l_ce_s"] + out["l_ce_l"] + out["l_cont_s"] + out["l_cont_l"] + nce, out


# ---------------------------------------------------------------------------------------------------------------------
# DIM-Speaker fine-tuning (reference code/seq2seq_pretrain.py:708-757) -- what code/finetune_s2s_pretrain.py trains with
# x_engine_pt.train_epoch_biwi
# ---------------------------------------------------------------------------------------------------------------------
SPEAKER_TRAINABLE_PREFIXES = ("decoder_joint.", "speaker_vq.decoder.")
SPEAKER_TRAINABLE_NAMES = ("patch_embed_dec_l", "speaker_embed.weight")


def speaker_trainable_parameters(model):
    """(name, parameter) of what ``SpeakerSLMFT.forward(mode='train')`` leaves a gradient on in the reference, in state-dict
    order: the cross entropy reaches ``decoder_joint.*``, ``patch_embed_dec_l`` and ``speaker_embed.weight``; the EMOCA loss
    reaches ``speaker_vq.decoder.*`` only (the arg-max cuts the graph).  Every other parameter keeps ``grad = None`` there, so
    the reference's AdamW and its clip norm skip it."""
    return [(n, p) for n, p in model.named_parameters()
            if n.startswith(SPEAKER_TRAINABLE_PREFIXES) or n in SPEAKER_TRAINABLE_NAMES]


def set_speaker_trainable(model, flag=True):
    for _, p in speaker_trainable_parameters(model):
        p.requires_grad_(flag)
    return model


def speaker_loss(P, dims, vq_dims, v_emoca, v_audio, mask, z, pe_s, speaker_ids=None, tokens=None):
    """Differentiable ``SpeakerSLMFT.forward(mode='train')`` (reference :708-757): the PyTorch-autograd CHECKER of
    ``SpeakerHipTrainer``.  P: {key: tensor} (parameters carry the graph); v_emoca [B,T,56]; v_audio [B,T,768]; mask [B,T] bool;
    z [B,T]: the listener VQ-VAE's codes of v_emoca with -100 on padding (from the frozen VQ-VAE, no graph); pe_s: the speaker
    VQ-VAE decoder's positional buffer; speaker_ids [B] long or None (a zero embedding row).  tokens [B,T-1]: code indices to
    decode instead of this function's own arg-max (a checker that follows another implementation's choice at a near tie).
    The codebook is frozen (no gradient through the lookup); the mean squared error runs over all B (T-1) 56 elements, padded
    frames included, as the reference's does.  Returns (total = l_ce + l_emoca, {l_ce, l_emoca, logits, tokens, pred})."""
    B, T = z.shape
    patch = P["patch_embed_dec_l"].reshape(1, 1, -1)
    if speaker_ids is None:
        x_l = torch.zeros(B, T, patch.shape[-1], dtype=v_audio.dtype, device=v_audio.device)
    else:
        x_l = P["speaker_embed.weight"][speaker_ids.long()][:, None, :].expand(B, T, -1)
    ctx = torch.cat([x_l + patch, v_audio], dim=-1)
    logits = xt_decoder_logits(P, "decoder_joint.net.", z[:, :-1].clamp(min=0), ctx, mask, None, dims.dec_depth, dims.heads, pos_emb=True)
    l_ce = F.cross_entropy(logits.reshape(-1, logits.shape[-1]), z[:, 1:].reshape(-1), ignore_index=-100)
    tok = logits.detach().argmax(-1) if tokens is None else tokens.reshape(B, T - 1).long()
    zq = P["speaker_vq.quantize.embedding.weight"].detach()[tok]
    pred = vq_decoder(P, "speaker_vq.", zq, vq_dims.heads, vq_dims.layers, pe_s)
    l_emoca = F.mse_loss(pred, v_emoca[:, 1:, :].to(pred.dtype))
    return l_ce + l_emoca, {"l_ce": l_ce, "l_emoca": l_emoca, "logits": logits, "tokens": tok, "pred": pred}


def speaker_context_adjoint(dctx, ids, rows, slices=8):
    """Host restatement of the context adjoint of csrc/train_spk.hip in ITS summation order: dctx [B,T,C] (the first C columns of
    the context gradient) -> (d patch_embed_dec_l [C], d speaker_embed.weight [rows,C]).  Per clip the frames are added in
    ascending t inside ``slices`` time slices and the slices in ascending order; the patch gradient adds the clips in ascending b;
    table row r adds the clips with ids[b] == r in ascending b (a gather per row: duplicated ids need no scatter), rows no clip
    names stay zero, ids None leaves the whole table zero."""
    B, T, C = dctx.shape
    per = -(-T // slices)
    clip = torch.zeros(B, C, dtype=dctx.dtype)
    for b in range(B):
        for s in range(slices):
            part = torch.zeros(C, dtype=dctx.dtype)
            for t in range(s * per, min(T, (s + 1) * per)):
                part = part + dctx[b, t]
            clip[b] = clip[b] + part
    d_patch = torch.zeros(C, dtype=dctx.dtype)
    for b in range(B):
        d_patch = d_patch + clip[b]
    d_embed = torch.zeros(rows, C, dtype=dctx.dtype)
    if ids is not None:
        for r in range(rows):
            for b in range(B):
                if int(ids[b]) == r:
                    d_embed[r] = d_embed[r] + clip[b]
    return d_patch, d_embed


# ---------------------------------------------------------------------------------------------------------------------
# gradient synchronisation
# ---------------------------------------------------------------------------------------------------------------------
def all_reduce_grads(params, bucket_bytes=64 << 20):
    """Average .grad over the ranks of the default process group in flat buckets (sum all-reduce, then / world).
    xGMI is point-to-point, ring collectives are per-link bound: few large buckets beat one collective per tensor."""
    world = ddist.world_size()
    if world == 1:
        return 0
    import torch.distributed as dist
    # every trainable parameter takes part on every rank, in the same order: a parameter without a gradient on this rank
    # (unused in this batch) contributes zeros -- buckets built from "has a grad" could differ between ranks and hang
    for p in params:
        if p.grad is None:
            p.grad = torch.zeros_like(p)
    grads = [p.grad for p in params]
    n_coll, i = 0, 0
    while i < len(grads):
        j, size = i, 0
        while j < len(grads) and (size == 0 or size + grads[j].numel() * grads[j].element_size() <= bucket_bytes):
            size += grads[j].numel() * grads[j].element_size()
            j += 1
        flat = torch.cat([g.reshape(-1) for g in grads[i:j]])
        dist.all_reduce(flat)
        flat.div_(world)
        o = 0
        for g in grads[i:j]:
            g.copy_(flat[o:o + g.numel()].view_as(g))
            o += g.numel()
        n_coll += 1
        i = j
    return n_coll


def broadcast_parameters(params, src=0):
    """Make every rank start from rank `src`'s parameters (flat buckets, like the gradients); without it the job relies on
    bit-identical construction on every rank."""
    if ddist.world_size() == 1:
        return 0
    import torch.distributed as dist
    n = 0
    with torch.no_grad():
        i = 0
        while i < len(params):
            j, size = i, 0
            while j < len(params) and (size == 0 or size + params[j].numel() * params[j].element_size() <= (64 << 20)):
                size += params[j].numel() * params[j].element_size()
                j += 1
            flat = torch.cat([p.detach().reshape(-1) for p in params[i:j]])
            dist.broadcast(flat, src)
            o = 0
            for p in params[i:j]:
                p.copy_(flat[o:o + p.numel()].view_as(p))
                o += p.numel()
            n += 1
            i = j
    return n


assert_same_batch_count = ddist.assert_same_batch_count   # lives in dist.py: the HIP training loops use it without importing this module


def train_step(model, optimizer, v_speaker, v_listener, v_audio, mask, clip=1.0, kv_mask=None, scheduler=None):
    """One optimisation step exactly as the reference's loop body (zero_grad, forward(mode='train'), backward, clip,
    step), with the gradient all-reduce in between for N > 1."""
    optimizer.zero_grad()
    loss, d, pred = model(v_speaker, v_listener, v_audio, mask, mode="train", kv_mask=kv_mask)
    loss.mean().backward()
    params = [p for _, p in trainable_parameters(model)]
    all_reduce_grads(params)
    if clip > 0:
        torch.nn.utils.clip_grad_norm_(params, clip)
    optimizer.step()
    if scheduler is not None:
        scheduler.step()
    return loss.detach(), d, pred


def make_optimizer(model, lr=1e-5):
    """reference code/finetune_s2s_pretrain.py:119: AdamW over the trainable parameters."""
    set_trainable(model, True)
    return torch.optim.AdamW([p for _, p in trainable_parameters(model)], lr=lr)
