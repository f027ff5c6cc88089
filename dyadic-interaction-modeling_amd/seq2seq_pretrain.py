"""Drop-in ``SLMFT`` (DIM-Listener): same constructor surface, parameter names, method names and
``forward`` signature/return as the reference ``code/seq2seq_pretrain.py:325-514``, computing on the
HIP library (``include/dimx.h``) through ``dimx.engine.Engine``.

Differences that are deliberate and documented:
  * the no-arg constructor still works, but since the reference's checkpoint files do not exist here the
    VQ-VAEs start from deterministic synthetic weights; ``vq_speaker_ckpt`` / ``vq_listener_ckpt`` accept
    the reference's ``model.pth.tar`` files (``{'state_dict': ...}``) when they do exist;
  * randomness is injectable: ``noise`` (Exp(1) sampling noise, [T-1,B,512]), ``kv_mask`` (the
    AutoregressiveWrapper key mask, [B,T-1] bool), ``greedy`` and ``seed``; the defaults draw fresh
    randomness like the reference;
  * ``forward_vq`` encodes each stream once, batched over ragged clips on the GPU (the reference encodes
    batch-1 clips in a Python loop, twice, code/seq2seq_pretrain.py:497-500); results are identical.
"""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import config as _config
from . import lib as L
from . import weights as W
from .models import _EngineOwner, build_param_tree, get_model


def _masked_pairwise_loss(pred, target, m):
    """mean_{valid} ||p[6:] - t[6:] + eps|| + mean_{valid} ||p[:6] - t[:6] + eps||  (F.pairwise_distance, eps 1e-6),
    without a device -> host synchronisation; an all-False mask gives NaN like the mean of an empty selection."""
    m = m.bool()
    d = F.pairwise_distance(pred[..., 6:], target[..., 6:]) + F.pairwise_distance(pred[..., 0:6], target[..., 0:6])
    zero = torch.zeros((), dtype=d.dtype, device=d.device)
    return torch.where(m, d, zero).sum() / m.sum()


def mark_prefix(mask):
    """Declare that every row of ``mask`` is True on a prefix [0, len) and False after it (what the engine protocol builds
    from ``src_len``, reference code/x_engine_pt.py:203-206).  compact_by_mask then has nothing to move and skips its
    stable argsort + gather over [B,T,56]; the claim is the caller's (a Python attribute on the tensor, lost by any op
    that creates a new tensor -- the safe direction)."""
    mask.dimx_prefix = True
    return mask


def compact_by_mask(x, mask):
    """Left-align the valid frames of every clip (``v[i][mask[i]]`` of the reference, batched).
    Returns (x_compact, lens int32).  A prefix mask (the engine protocol) keeps its valid frames where they are; frames past
    a clip's length are zero unless the mask was declared a prefix mask (mark_prefix) -- the engine never reads them."""
    lens = mask.sum(1).to(torch.int32)
    if getattr(mask, "dimx_prefix", False):
        return x, lens
    T = mask.shape[1]
    prefix = torch.arange(T, device=mask.device)[None, :] < lens[:, None]
    if not x.is_cuda and torch.equal(prefix, mask):
        return x, lens
    # On the GPU the same arithmetic runs for every mask (for a prefix mask the stable argsort is the identity): testing
    # `mask == prefix` on the host would synchronise with the device at the head of every forward call, and the GPU then
    # idles (1.3 ms per 256-clip batch in the round-2 trace) while the host queues the first kernels of the next batch.
    order = torch.argsort((~mask).to(torch.int8), dim=1, stable=True)
    xc = torch.gather(x, 1, order[..., None].expand(-1, -1, x.shape[-1]))
    return torch.where(prefix[..., None], xc, torch.zeros((), dtype=x.dtype, device=x.device)), lens


def prompt_lengths(mask, prompt_frames, lengths=None):
    """Prompted generation from a validity mask [B,T]: ``prompt_len`` [B] int32 on the mask's device =
    clamp(valid frames per clip, 1, prompt_frames), and the host integer ``P0`` = the prefix every clip has, which is the part
    that is prefilled: min(prompt_frames, min(lengths)) when the caller knows the clip lengths on the host (``lengths``, a
    list of ints: the engine loops have ``src_len``), else the minimum of ``prompt_len`` -- ONE ``.item()``, a host
    synchronisation per call."""
    prompt_frames = int(prompt_frames)
    plen = mask.bool().sum(1).clamp(1, prompt_frames).to(torch.int32)
    if lengths is not None:
        p0 = min(prompt_frames, min(int(n) for n in lengths))
    else:
        p0 = int(plen.min().item())
    return plen, max(1, p0)


def _check_prompt_frames(prompt_frames, T):
    prompt_frames = int(prompt_frames)
    if prompt_frames == 1:
        return 1
    if prompt_frames < 1 or prompt_frames >= T:
        raise ValueError("prompt_frames=%d: a prompt holds 1 .. T-1 = %d frames (T=%d frames per clip)" % (prompt_frames, T - 1, T))
    return prompt_frames


class SLMFT(_EngineOwner):
    def __init__(self, config_path=None, vq_speaker_ckpt=None, vq_listener_ckpt=None,
                 synthetic_seed=20260928, numeric_mode=L.MODE_PARITY_F32):
        super().__init__(numeric_mode)
        config_path = config_path or ("./config.yaml" if os.path.isfile("./config.yaml") else _config.DEFAULT_CONFIG)
        cfg_s = _config.load_cfg_from_cfg_file(config_path)
        cfg_l = _config.load_cfg_from_cfg_file(config_path)
        self.speaker_vq = get_model(cfg_s, synthetic_seed=synthetic_seed, weight_prefix="speaker_vq.", which=0,
                                    numeric_mode=numeric_mode)
        self.listener_vq = get_model(cfg_l, synthetic_seed=synthetic_seed, weight_prefix="listener_vq.", which=1,
                                     numeric_mode=numeric_mode)
        for m, ck in ((self.speaker_vq, vq_speaker_ckpt), (self.listener_vq, vq_listener_ckpt)):
            if ck is not None:
                m.load_state_dict(torch.load(ck, map_location="cpu")["state_dict"])
            m.eval()
        self.speaker_face_quan_num = cfg_s.face_quan_num
        self.speaker_zquant_dim = cfg_s.zquant_dim
        self.s2s = W.S2SDims()
        spec = [e for e in W.slmft_spec(self.speaker_vq.dims, self.s2s)
                if not (e[0].startswith("speaker_vq.") or e[0].startswith("listener_vq."))]
        build_param_tree(self, spec, W.synth_state_dict(spec, synthetic_seed))
        self.mask_prob = self.s2s.mask_prob

    # ------------------------------------------------------------------ engine plumbing
    def _engine_state_dict(self):
        return self.state_dict()

    def _mask8(self, mask):
        return mask.to(torch.uint8).contiguous()

    # ------------------------------------------------------------------ reference sub-APIs
    @torch.no_grad()
    def forward_vq(self, v_speaker, v_listener, mask, with_speaker=True):
        """reference :480-494 -> (z_speaker [B,T] padded with 0, z_listener [B,T] padded with -100), int64."""
        eng = self.engine(v_speaker.device)
        xl, lens = compact_by_mask(v_listener, mask)
        z_l = eng.vq_encode(1, xl, lens, pe_mode=0, pad_value=-100).long()
        z_s = None
        if with_speaker:
            xs, _ = compact_by_mask(v_speaker, mask)
            z_s = eng.vq_encode(0, xs, lens, pe_mode=0, pad_value=0).long()
        return z_s, z_l

    @torch.no_grad()
    def forward_encoder(self, v_speaker, mask):
        """reference :431-442 -> x_s [B,T,384] (rows of padded frames are unspecified)."""
        return self.engine(v_speaker.device).encode_speaker(v_speaker, self._mask8(mask.bool()))

    def _build_context(self, eng, x_s, v_speaker, x_a, m8, for_generate, n_samples=1, prompt_frames=1, guided=False):
        # x_s given (the reference's call shape): context straight from it; x_s None + v_speaker: the fused stage that
        # keeps the encoder output inside the workspace (what forward() uses)
        if x_s is not None:
            eng.set_context(x_s, x_a, which_patch=0, for_generate=for_generate, n_samples=n_samples, prompt_frames=prompt_frames,
                            guided=guided)
        else:
            assert v_speaker is not None, "forward_decoder needs x_s (reference call) or v_speaker= (fused path)"
            eng.encode_ctx(v_speaker, x_a, m8, for_generate, n_samples=n_samples, prompt_frames=prompt_frames, guided=guided)

    def _null_context(self, eng, B, T, x_a):
        """the null context of dimx.guidance: zero rows after the concat [x + patch_embed_dec_s | audio] -- x = -patch_embed_dec_s
        (x + p is then exactly 0) and zero audio features"""
        p = self.state_dict()["patch_embed_dec_s"].detach().to(x_a.device, torch.float32)
        eng.set_context((-p).reshape(1, 1, -1).expand(B, T, -1).contiguous(), torch.zeros_like(x_a, dtype=torch.float32), which_patch=0,
                        for_generate=False)

    @staticmethod
    def _user_seed(seed):
        """seed -> non-zero generator key (the C-ABI reserves 0 for 'greedy when no noise is given')."""
        if seed is None:
            return int(torch.randint(1, 2 ** 62, (1,)).item())
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        return seed if seed != 0 else 0x9E3779B97F4A7C15

    @torch.no_grad()
    def forward_decoder(self, x_s, z_l, x_a, mask, mode, v_speaker=None, noise=None, kv_mask=None, greedy=False,
                        seed=None, temperature=1.0, n_samples=1, prompt_frames=1, lengths=None, filter_logits_fn=None,
                        filter_kwargs=None, return_scores=False, beam_width=0, lookahead=None, window_prefill=False, guidance=None,
                        kv8=False, self_kv8=False, kv8_samples=False, beam_kv8=None):
        """reference :444-452, same positional call: ``forward_decoder(x_s, z_l, x_a, mask, mode)`` with the ``x_s``
        that ``forward_encoder`` returned.  ``forward()`` passes ``x_s=None, v_speaker=...`` instead, which keeps the
        encoder output inside the engine workspace (no round trip through a tensor).

        ``prompt_frames`` P > 1 (mode 'val'): the generation continues the ground-truth listener codes ``z_l[:, :P]``
        instead of starting from ``z_l[:, 0]`` alone (the reference edit: ``decoder_joint.generate(z_l[:, :P], seq_len=T-P,
        ...)``); a clip with fewer than P valid frames is prompted with the frames it has.  ``lengths`` (host list of the
        clips' valid frame counts) spares the one ``.item()`` that otherwise finds the common prefix (``prompt_lengths``).
        The returned tokens keep the shape [B*S, T-1]: their first plen-1 columns repeat ``z_l[:, 1:plen]``.

        ``filter_logits_fn`` / ``filter_kwargs`` (mode 'val'): the sampler filter, as AutoregressiveWrapper.generate takes it --
        ``top_k``, ``top_p``, ``min_p`` or ``top_a`` of dimx.sampling (object or name).  The default is the reference's call:
        top_k with k = ceil(0.1 * 512) = 52.

        ``return_scores`` (mode 'val'): a third value, the SeqScores [B*S] of the sampled sequences (Engine.generate).

        ``beam_width`` W >= 1 (mode 'val'): beam search instead of sampling (Engine.generate_beam; ``n_samples`` must be W, the
        sampler's arguments are not used): tokens [B*W, T-1], whole hypotheses, row b*W the best; the SeqScores are the search's
        own running scores and the number of scored columns.

        ``lookahead`` L (mode 'val', no beam search): online generation (dimx.online) -- the step that produces frame t+1 sees the
        speaker frames below clamp(t + 2 + L, 1, T) only; a prompt then runs through forced decode steps instead of a prefill,
        unless ``window_prefill`` asks for the prefill under the window (``Engine.generate(prefill="window")``; same definition,
        other kernels).  None: the whole clip is visible, as in the reference.

        ``guidance`` s (mode 'val', one sample per clip, no beam search): classifier-free guidance (dimx.guidance,
        ``Engine.generate(guidance=s)``) -- every step samples from cond + (s - 1) * (cond - uncond), uncond being the decoder
        without a context.  A prompt then runs through forced decode steps; scores are taken under the guided logits.  None
        is the call without the argument, launch for launch.

        ``kv8`` (mode 'val', one sample per clip, no beam search): the decode steps' cross attention reads an FP8 copy of the
        context K / V, quantised once per generation (dimx.kv8, ``Engine.generate(kv8=True)``).  False is the call without the
        argument, launch for launch.

        ``self_kv8`` (mode 'val', any ``n_samples``, no beam search, no guidance): FP8 self-attention K/V caches -- every decode step
        quantises its k / v row and attends over the codes (dimx.kv8.self_step, ``Engine.generate(self_kv8=True)``).  False is the
        call without the argument, launch for launch.

        ``kv8_samples`` (mode 'val', any ``n_samples``, no beam search, no guidance): ``kv8`` for best-of-N -- the S queries of a clip
        read that clip's FP8 codes in one multi-query launch per layer (dimx.kv8.attention_rows,
        ``Engine.generate(kv8_samples=True)``).  False is the call without the argument, launch for launch.

        ``beam_kv8`` (mode 'val', with ``beam_width``, no guidance): "self", "cross" or True (both) -- the beam search runs on FP8
        self caches and / or an FP8 copy of the cross K/V (dimx.kv8.reorder, ``Engine.generate_beam(beam_kv8=...)``).  None is the
        call without the argument, launch for launch."""
        if beam_kv8 and (mode != "val" or not beam_width or guidance is not None):
            raise ValueError("beam_kv8 applies to mode='val' with beam_width and without guidance")
        if kv8_samples and (mode != "val" or beam_width or guidance is not None):
            raise ValueError("kv8_samples applies to mode='val' without beam search and without guidance")
        if self_kv8 and (mode != "val" or beam_width or guidance is not None):
            raise ValueError("self_kv8 applies to mode='val' without beam search and without guidance")
        if guidance is not None and (mode != "val" or beam_width or int(n_samples) != 1):
            raise ValueError("guidance applies to mode='val' with one sample per clip and without beam search")
        if kv8 and (mode != "val" or beam_width or int(n_samples) != 1):
            raise ValueError("kv8 applies to mode='val' with one sample per clip and without beam search")
        if beam_width and (mode != "val" or int(n_samples) != int(beam_width)):
            raise ValueError("beam_width applies to mode='val' with n_samples == beam_width")
        if lookahead is not None and (mode != "val" or beam_width):
            raise ValueError("lookahead applies to mode='val' without beam search")
        if return_scores and mode != "val":
            raise ValueError("return_scores applies to mode='val' (SLMFT.score is the teacher-forced form)")
        prompt_frames = _check_prompt_frames(prompt_frames, z_l.shape[1])
        dev = (x_s if x_s is not None else v_speaker).device
        eng = self.engine(dev)
        m8 = self._mask8(mask.bool())
        B, T = z_l.shape
        if mode == "train":
            self._build_context(eng, x_s, v_speaker, x_a, m8, False)
            if kv_mask is None:
                kv_mask = self.draw_kv_mask(B, T, dev)
            elif kv_mask is False:
                kv_mask = None
            logits, row_loss, _ = eng.decode_tf(z_l, m8, self._mask8(kv_mask) if kv_mask is not None else None)
            n_valid = (z_l[:, 1:] != -100).sum().clamp(min=1)
            return row_loss.sum() / n_valid, logits
        plen, p0 = prompt_lengths(mask, prompt_frames, lengths) if prompt_frames > 1 else (None, 1)
        gkw = {}
        if guidance is not None:      # the guided step forces the whole prompt: no prefill scratch, 2B rows of self-attention caches
            p0, gkw = 1, {"guidance": float(guidance)}
        if kv8:
            gkw = dict(gkw, kv8=True)
        if self_kv8:
            gkw = dict(gkw, self_kv8=True)
        if kv8_samples:
            gkw = dict(gkw, kv8_samples=True)
        self._build_context(eng, x_s, v_speaker, x_a, m8, True, n_samples=n_samples, prompt_frames=p0, guided=guidance is not None)
        if beam_width:
            from .scoring import SeqScores, scored_columns
            tokens, score = eng.generate_beam(z_l[:, 0], m8, T, int(beam_width), prompt=z_l[:, :prompt_frames] if prompt_frames > 1 else None,
                                              prompt_len=plen, prefill=p0, beam_kv8=beam_kv8 or None)
            if not return_scores:
                return 0.0, tokens.long()
            n = tokens.shape[1]
            first, last = scored_columns(T, n, m8.sum(1, dtype=torch.int32), plen)
            count = (last.clamp(0, n) - (first + torch.zeros_like(last)).clamp(0, n)).clamp(min=0).to(torch.int32)
            return 0.0, tokens.long(), SeqScores(score, count.repeat_interleave(int(beam_width)))
        if greedy:
            temperature, seed_v = 0.0, 0
        else:
            seed_v = 0 if noise is not None else self._user_seed(seed)
        if prompt_frames > 1:
            out = eng.generate(None, m8, T, temperature, 52, noise, seed_v, n_samples=n_samples,
                               prompt=z_l[:, :prompt_frames], prompt_len=plen,
                               prefill=("window", p0) if (window_prefill and lookahead is not None) else p0,
                               filter_logits_fn=filter_logits_fn, filter_kwargs=filter_kwargs, return_scores=return_scores,
                               lookahead=lookahead, **gkw)
        else:
            out = eng.generate(z_l[:, 0], m8, T, temperature, 52, noise, seed_v, n_samples=n_samples,
                               filter_logits_fn=filter_logits_fn, filter_kwargs=filter_kwargs, return_scores=return_scores,
                               lookahead=lookahead, **gkw)
        if return_scores:
            return 0.0, out[0].long(), out[1]
        return 0.0, out.long()

    @torch.no_grad()
    def stream(self, B, Tmax, start, lookahead=0, greedy=False, noise=None, seed=None, temperature=1.0, top_k=52, prompt=None,
               v_speaker=None, v_audio=None, kv8=False, self_kv8=False):
        """A streaming session (dimx.engine.StreamSession; dimx.stream is the schedule): push the speaker's motion and audio
        frames in pieces, receive the listener tokens as they fall due.  ``start`` [B]: the listener's first codes, the caller's --
        a live system has no ground-truth first code.  The sampler arguments are ``forward_decoder``'s.  Fed a whole clip, the
        session emits the tokens of ``forward(mode='val', lookahead=lookahead)`` with ``start`` = that clip's first code.
        ``prompt`` [B, P] codes with ``v_speaker`` / ``v_audio`` [B, F, .]: the session starts from its first P codes and F frames
        (``Engine.stream``; ``start`` is ignored) -- how a conversation that outlasts a session carries on in the next one.  Nothing
        was trained on restarted clips: what such a session emits is a definition, not a claim about quality.
        ``kv8`` / ``self_kv8``: FP8 cross / self K/V for the session (``Engine.stream``): the steps read codes, and what the
        session emits is ``forward(mode='val', lookahead=lookahead, kv8=True, self_kv8=True)`` up to the rounding of the two encoders."""
        eng = self.engine(start.device)
        if greedy:
            temperature, seed_v = 0.0, 0
        else:
            seed_v = 0 if noise is not None else self._user_seed(seed)
        return eng.stream(B, Tmax, start, lookahead, temperature, top_k, noise, seed_v, prompt, v_speaker, v_audio, kv8, self_kv8)

    def draw_kv_mask(self, B, T, device, generator=None):
        """AutoregressiveWrapper(mask_prob=0.15) key mask (reference ctor :419): keep-mask [B,T-1]."""
        n = T - 1
        rand = torch.randn(B, n, device=device, generator=generator)
        rand[:, 0] = -torch.finfo(rand.dtype).max
        num_mask = min(int(T * self.mask_prob), T - 1)
        idx = rand.topk(num_mask, dim=-1).indices
        return ~torch.zeros(B, n, device=device).scatter(1, idx, 1.0).bool()

    @torch.no_grad()
    def forward_vq_decoder(self, logits_l, mode="train", batch_row_offset=0, rows_per_clip=1):
        """reference :454-464: argmax (train) / tokens (val) -> codebook lookup -> listener_vq.decode."""
        pred_seq_l = torch.argmax(logits_l, dim=-1) if mode == "train" else logits_l
        return self.engine(pred_seq_l.device).vq_decode(1, pred_seq_l, batch_row_offset, rows_per_clip)

    def forward_continuous_loss(self, pred, target, mask):
        """reference :466-478: mean pairwise distance over the valid frames, expression part + pose part.  Written as
        masked sums / count instead of boolean indexing: ``x[m]`` synchronises with the device (nonzero) and left the GPU
        idle for ~0.6 ms per call inside the timed forward."""
        return _masked_pairwise_loss(pred, target[:, 1:, :], mask[:, 1:])

    # ------------------------------------------------------------------ training
    def dimx_trainable_parameters(self):
        from . import train as T
        return T.trainable_parameters(self)

    def _wants_grad(self, mode):
        return (mode == "train" and self.training and torch.is_grad_enabled()
                and any(p.requires_grad for p in self.parameters()))

    def train(self, mode=True):
        """nn.Module.train, with the reference's frozen parts kept in eval (code/seq2seq_pretrain.py:348-366)."""
        super().train(mode)
        self.speaker_vq.eval()
        self.listener_vq.eval()
        return self

    def _forward_autograd(self, v_speaker, v_listener, v_audio, mask, kv_mask=None, z_l=None, return_tokens=False, lookahead=None,
                          cond_keep=None):
        """mode='train' with a graph: differentiable cross entropy (dimx.train.slmft_loss on this module's own
        parameters); listener codes and decoded motion come from the HIP engine without a graph.
        ``lookahead`` L: online fine-tuning -- the decoder's cross attention of row t sees the context rows below
        clamp(t + 2 + L, 1, T) only (dimx.online); ``x_engine_pt.train_epoch(lookahead=L)`` is what passes it."""
        from . import train as T
        mask = mask.bool()
        B, Tn = mask.shape
        on_gpu = v_speaker.is_cuda
        if z_l is None:
            with torch.no_grad():
                _, z_l = self.forward_vq(v_speaker, v_listener, mask, with_speaker=False)
        if kv_mask is None:
            kv_mask = self.draw_kv_mask(B, Tn, v_speaker.device)
        elif kv_mask is False:
            kv_mask = None
        P = dict(self.named_parameters())
        l_ce_l, logits = T.slmft_loss(P, self.s2s, v_speaker.float(), v_audio.float(), mask, z_l.long(),
                                      kv_mask.bool() if kv_mask is not None else None, lookahead=lookahead, cond_keep=cond_keep)
        pred, l_cont_l = None, torch.zeros((), device=v_speaker.device)
        if on_gpu:     # the continuous loss has no gradient path in the reference either (argmax -> one-hot, :454-464)
            with torch.no_grad():
                pred = self.forward_vq_decoder(logits.detach(), mode="train")
                l_cont_l = self.forward_continuous_loss(pred, v_listener, mask)
        total_loss = l_ce_l + l_cont_l
        d = {"l_ce_s": 0, "l_ce_l": l_ce_l.detach(), "l_cont_s": 0, "l_cont_l": l_cont_l, "nce": 0, "c_acc": 0}
        if return_tokens:
            return total_loss, d, pred, logits.detach().argmax(-1)
        return total_loss, d, pred

    # ------------------------------------------------------------------ forward
    def forward(self, v_speaker, v_listener, v_audio, mask, mode="train", speaker_ids=None, listener_ids=None,
                noise=None, kv_mask=None, greedy=False, seed=None, temperature=1.0, batch_row_offset=0,
                return_tokens=False, n_samples=1, shard=None, z_l=None, prompt_frames=1, lengths=None, filter_logits_fn=None,
                filter_kwargs=None, return_scores=False, beam_width=None, num_return=1, lookahead=None, window_prefill=False,
                guidance=None, kv8=False, self_kv8=False, kv8_samples=False, beam_kv8=None):
        """reference :496-514.  In training (``model.train()``, grad enabled, parameters requiring grad) the
        teacher-forced pass returns a loss with an autograd graph; everything else is the HIP inference path.

        ``prompt_frames`` P > 1 (mode 'val'): continue the clip's first P ground-truth listener codes (see
        ``forward_decoder``; ``lengths`` = host list of valid frames per clip, optional).  ``pred`` keeps its shape
        [B,T-1,56]: its first plen-1 frames are the VQ decoder's rendering of the ground-truth codes, the rest is
        generated.  P >= T raises ValueError.

        ``filter_logits_fn`` / ``filter_kwargs`` (mode 'val'): the sampler filter (see ``forward_decoder``).

        ``return_scores`` (mode 'val'; any other mode raises ValueError): the log-likelihood of every generated sequence under the
        model (dimx.scoring.SeqScores: score f64 and count int32, [B] or [B,S]) is appended after ``pred``, or after ``tokens``
        with ``return_tokens``.  Cost and scored columns: ``Engine.generate``.

        ``beam_width`` W in {1, 2, 4, 5, 8, 10} (mode 'val'): beam search (dimx.beam, ``Engine.generate_beam``) instead of sampling --
        deterministic, ``noise`` / ``greedy`` / ``seed`` / ``temperature`` / the filter / ``n_samples`` are not used.  ``num_return``
        = 1: the best hypothesis, shapes as without the argument; ``num_return`` = W: all W, best first, shapes as with
        ``n_samples=W`` (pred [B,W,T-1,56]).  With ``return_scores`` the SeqScores hold the search's own scores.

        ``lookahead`` L (mode 'val', no beam search): online generation (dimx.online; ``forward_decoder``) -- the listener token of
        frame t+1 is drawn from the speaker frames below clamp(t + 2 + L, 1, T).  The tokens are causal in the speaker; ``pred`` is
        still the VQ decoder's rendering of the whole token sequence.  ``window_prefill`` (with ``prompt_frames`` and ``lookahead``): the
        prompt is prefilled in one pass under the window instead of running through forced decode steps (``forward_decoder``).

        ``guidance`` s (mode 'val', ``n_samples`` 1, no beam search): classifier-free guidance (dimx.guidance; ``forward_decoder``):
        s = 1 is the model, s > 1 makes the listener more reactive to the speaker, s = 0 generates from the listener's prior.

        ``kv8`` (mode 'val', ``n_samples`` 1, no beam search): FP8 cross-attention K/V for the generation (dimx.kv8;
        ``forward_decoder``).

        ``self_kv8`` (mode 'val', any ``n_samples``, no beam search, no guidance): FP8 self-attention K/V caches for the generation
        (dimx.kv8.self_step; ``forward_decoder``) -- the protocol's best-of-N runs take it.

        ``kv8_samples`` (mode 'val', any ``n_samples``, no beam search, no guidance): FP8 cross-attention K/V for a best-of-N
        generation (dimx.kv8.attention_rows; ``forward_decoder``); combines with ``self_kv8``.

        ``beam_kv8`` (mode 'val', with ``beam_width``, no guidance): "self", "cross" or True (both) -- FP8 self caches and / or FP8
        cross K/V for the beam search (dimx.kv8.reorder; ``forward_decoder``)."""
        if beam_kv8 and (mode != "val" or beam_width is None or guidance is not None):
            raise ValueError("beam_kv8 applies to mode='val' with beam_width and without guidance")
        if kv8_samples and (mode != "val" or beam_width is not None or guidance is not None):
            raise ValueError("kv8_samples applies to mode='val' without beam search and without guidance")
        if self_kv8 and (mode != "val" or beam_width is not None or guidance is not None):
            raise ValueError("self_kv8 applies to mode='val' without beam search and without guidance")
        if guidance is not None and (mode != "val" or beam_width is not None or int(n_samples) != 1):
            raise ValueError("guidance applies to mode='val' with one sample per clip and without beam search")
        if kv8 and (mode != "val" or beam_width is not None or int(n_samples) != 1):
            raise ValueError("kv8 applies to mode='val' with one sample per clip and without beam search")
        if lookahead is not None and (mode != "val" or beam_width is not None):
            raise ValueError("lookahead applies to mode='val' without beam search")
        if beam_width is not None:
            if mode != "val" or int(num_return) not in (1, int(beam_width)):
                raise ValueError("beam_width applies to mode='val' with num_return 1 or beam_width")
        prompt_frames = _check_prompt_frames(prompt_frames, mask.shape[1])
        if prompt_frames > 1 and mode != "val":
            raise ValueError("prompt_frames applies to mode='val'")
        if return_scores and mode != "val":
            raise ValueError("return_scores applies to mode='val' (SLMFT.score is the teacher-forced form)")
        if self._wants_grad(mode):
            return self._forward_autograd(v_speaker, v_listener, v_audio, mask, kv_mask=kv_mask, z_l=z_l,
                                          return_tokens=return_tokens)
        with self.engine_pinned():     # one weights check per forward, not one per stage
            return self._forward_nograd(v_speaker, v_listener, v_audio, mask, mode=mode, noise=noise, kv_mask=kv_mask,
                                        greedy=greedy, seed=seed, temperature=temperature,
                                        batch_row_offset=batch_row_offset, return_tokens=return_tokens,
                                        n_samples=n_samples, shard=shard, prompt_frames=prompt_frames, lengths=lengths,
                                        filter_logits_fn=filter_logits_fn, filter_kwargs=filter_kwargs, return_scores=return_scores,
                                        beam_width=beam_width, num_return=num_return, lookahead=lookahead,
                                        window_prefill=window_prefill, guidance=guidance, kv8=kv8, self_kv8=self_kv8,
                                        kv8_samples=kv8_samples, beam_kv8=beam_kv8)

    @torch.no_grad()
    def _forward_nograd(self, v_speaker, v_listener, v_audio, mask, mode="train", speaker_ids=None, listener_ids=None,
                        noise=None, kv_mask=None, greedy=False, seed=None, temperature=1.0, batch_row_offset=0,
                        return_tokens=False, n_samples=1, shard=None, prompt_frames=1, lengths=None, filter_logits_fn=None,
                        filter_kwargs=None, return_scores=False, beam_width=None, num_return=1, lookahead=None, window_prefill=False,
                        guidance=None, kv8=False, self_kv8=False, kv8_samples=False, beam_kv8=None):
        """reference :496-514 -> (total_loss, dict, pred_cont_seq_l [B,T-1,56]).

        ``n_samples`` S > 1 (mode 'val' only): S independent generations per clip in ONE pass -- what the
        reference's evaluation loop obtains from S separate forward calls (code/x_engine_pt.py:257) -- sharing the
        VQ encode, the encoder stack and the context K/V stream; pred is then [B,S,T-1,56], tokens [B,S,T-1]."""
        mask = mask.bool()
        W = int(beam_width or 0)
        S = W if W else int(n_samples)
        assert S == 1 or mode != "train", "n_samples applies to mode='val'"
        _, z_l = self.forward_vq(v_speaker, v_listener, mask, with_speaker=False)
        # shard = (first clip row, clips in the whole batch) when this call is one rank's slice of a batch: together
        # with batch_row_offset it makes the slice reproduce the same rows of a single-process call
        eng = self.engine(v_speaker.device)
        eng.set_shard(*(shard if shard is not None else (0, 0)))
        try:
            l_ce_l, px_l, *scores = self.forward_decoder(None, z_l, v_audio, mask, mode, v_speaker=v_speaker, noise=noise,
                                                         kv_mask=kv_mask, greedy=greedy, seed=seed, temperature=temperature,
                                                         n_samples=S, prompt_frames=prompt_frames, lengths=lengths,
                                                         filter_logits_fn=filter_logits_fn, filter_kwargs=filter_kwargs,
                                                         return_scores=return_scores, beam_width=W, lookahead=lookahead,
                                                         window_prefill=window_prefill, guidance=guidance, kv8=kv8, self_kv8=self_kv8,
                                                         kv8_samples=kv8_samples, beam_kv8=beam_kv8)
        finally:
            eng.set_shard(0, 0)
        if W and int(num_return) == 1:    # the best hypothesis is row 0 of its clip
            px_l = px_l.view(mask.shape[0], W, -1)[:, 0].contiguous()
            scores = [type(sc)(sc.score.view(-1, W)[:, 0], sc.count.view(-1, W)[:, 0]) for sc in scores]
            S = 1
        pred = self.forward_vq_decoder(px_l, mode=mode, batch_row_offset=batch_row_offset, rows_per_clip=S)
        if S > 1:
            B, T = mask.shape
            pred = pred.view(B, S, T - 1, -1)
            l_cont_l = torch.stack([self.forward_continuous_loss(pred[:, i], v_listener, mask) for i in range(S)]).mean()
        else:
            l_cont_l = self.forward_continuous_loss(pred, v_listener, mask)
        total_loss = l_ce_l + l_cont_l
        d = {"l_ce_s": 0, "l_ce_l": l_ce_l, "l_cont_s": 0, "l_cont_l": l_cont_l, "nce": 0, "c_acc": 0}
        out = (total_loss, d, pred)
        if return_tokens:
            tokens = px_l if mode != "train" else torch.argmax(px_l, dim=-1)
            if S > 1:
                tokens = tokens.view(mask.shape[0], S, -1)
            out += (tokens,)
        if return_scores:
            shape = (mask.shape[0], S) if S > 1 else (mask.shape[0],)
            out += (type(scores[0])(scores[0].score.view(shape), scores[0].count.view(shape)),)
        return out


    @torch.no_grad()
    def forward_online_tf(self, v_speaker, v_listener, v_audio, mask, lookahead, z_l=None):
        """The teacher-forced forward under online visibility, without a graph: ``forward(mode='train')``'s return values
        (total_loss, dict, pred [B,T-1,56]) with the decoder's cross attention of row t bounded to the context rows below
        clamp(t + 2 + L, 1, T) -- one ``decode_tf(lookahead=L)`` pass (dimx_decode_tf_win), no random key mask.  The validation
        counterpart of an online fine-tuning (``x_engine_pt.evaluate_finetune_epoch(lookahead=L)``)."""
        with self.engine_pinned():
            mask = mask.bool()
            eng = self.engine(v_speaker.device)
            if z_l is None:
                _, z_l = self.forward_vq(v_speaker, v_listener, mask, with_speaker=False)
            m8 = self._mask8(mask)
            self._build_context(eng, None, v_speaker, v_audio, m8, True)
            logits, row_loss, _ = eng.decode_tf(z_l, m8, None, lookahead=int(lookahead))
            l_ce_l = row_loss.sum() / (z_l[:, 1:] != -100).sum().clamp(min=1)
            pred = self.forward_vq_decoder(logits, mode="train")
            l_cont_l = self.forward_continuous_loss(pred, v_listener, mask)
            d = {"l_ce_s": 0, "l_ce_l": l_ce_l, "l_cont_s": 0, "l_cont_l": l_cont_l, "nce": 0, "c_acc": 0}
            return l_ce_l + l_cont_l, d, pred

    @torch.no_grad()
    def score(self, v_speaker, v_listener, v_audio, mask, z_l=None, lookahead=None, one_pass=False, context=None):
        """Teacher-forced log-likelihood of the clip's own listener codes (``forward_vq`` of ``v_listener``) or of given codes
        ``z_l`` [B,T] under the model: one ``decode_tf`` pass with NO random key mask, then dimx_op_seq_logprob on its logits with the
        tokens ``z_l[:, 1:]`` over the columns inside each clip's length -> dimx.scoring.SeqScores [B] (score f64, count int32).
        ``dimx.scoring.perplexity`` of it is the model's perplexity on these codes.

        ``lookahead`` L: the same log-likelihood under online visibility (dimx.online) -- position t+1 is predicted from the
        speaker frames below clamp(t + 2 + L, 1, T).  The logits then come from a generation whose every token is forced to ``z_l``
        (a prompt of T-1 tokens through decode steps, no prefill), scored over the same columns.  ``one_pass=True`` takes them from
        one teacher-forced pass under the window instead (``decode_tf(lookahead=L)``, dimx_decode_tf_win): the same definition through
        other kernels, so the same score within the decode steps' tolerance, not the same bits.

        ``context="null"``: the same codes under the null context of dimx.guidance (zero rows after the concat: the decoder
        without its cross sublayers, the listener's prior) -- host code only, ``set_context`` with zero rows and ``decode_tf``.
        Not with ``lookahead`` (a window over zero rows is the same zero rows)."""
        if context not in (None, "null"):
            raise ValueError("score(context=%r): None or 'null'" % (context,))
        if context == "null" and lookahead is not None:
            raise ValueError("score(context='null') takes no lookahead")
        from .engine import op_seq_logprob
        from .scoring import scored_columns
        with self.engine_pinned():
            mask = mask.bool()
            eng = self.engine(v_speaker.device)
            if z_l is None:
                _, z_l = self.forward_vq(v_speaker, v_listener, mask, with_speaker=False)
            m8 = self._mask8(mask)
            T = mask.shape[1]
            if lookahead is not None:
                self._build_context(eng, None, v_speaker, v_audio, m8, True)
                if one_pass:
                    logits, _, _ = eng.decode_tf(z_l, m8, None, lookahead=lookahead)
                else:
                    _, logits = eng.generate(None, m8, T, 0.0, 52, None, 0, return_logits=True, prompt=z_l[:, :T - 1], prefill=1,
                                             no_prefill=True, lookahead=lookahead)
            else:
                if context == "null":
                    self._null_context(eng, mask.shape[0], T, v_audio)
                else:
                    self._build_context(eng, None, v_speaker, v_audio, m8, False)
                logits, _, _ = eng.decode_tf(z_l, m8, None)
            first, last = scored_columns(T, T - 1, mask.sum(1, dtype=torch.int32))
            return op_seq_logprob(logits, z_l[:, 1:], first, last)

    @torch.no_grad()
    def pmi(self, v_speaker, v_listener, v_audio, mask, z_l=None):
        """Per-clip pointwise mutual information between the speaker context and the clip's own listener codes (or given codes
        ``z_l``), per counted token: ``dimx.guidance.pmi(score(...), score(..., context="null"))`` -> float64 numpy [B].  How much
        the speaker explains this listener under the model; 0 for a model that ignores its context."""
        from . import guidance
        if z_l is None:
            _, z_l = self.forward_vq(v_speaker, v_listener, mask.bool(), with_speaker=False)
        return guidance.pmi(self.score(v_speaker, v_listener, v_audio, mask, z_l=z_l),
                            self.score(v_speaker, v_listener, v_audio, mask, z_l=z_l, context="null"))


class SLM(_EngineOwner):
    """Drop-in ``SLM`` (the pre-training model, reference ``code/seq2seq_pretrain.py:58-323``), forward pass only:
    ``forward(v_speaker, v_listener, v_audio, mask, ...) -> (total_loss, dict, None)`` with the reference's six
    dict entries.  The random frame masks of ``random_masking_unstructured`` (:170-183) are injectable
    (``mask_speaker`` / ``mask_listener`` bool [B,T], True = masked); by default they are drawn like the reference.
    The InfoNCE term (:270-289) is a handful of [B,384] torch ops on the engine's encoder outputs.
    In training (``model.train()``, grad enabled, parameters requiring grad -- what ``x_engine_pt.train_epoch`` sets up for
    code/train_s2s_pretrain.py:41-64) the loss carries an autograd graph (``dimx.train.slm_loss``; the frozen VQ encoders
    run on the HIP engine); everything else is the HIP inference path."""
    engine_variant = "slm"

    def __init__(self, config_path=None, vq_speaker_ckpt=None, vq_listener_ckpt=None, synthetic_seed=20260928,
                 numeric_mode=L.MODE_PARITY_F32):
        super().__init__(numeric_mode)
        config_path = config_path or ("./config.yaml" if os.path.isfile("./config.yaml") else _config.DEFAULT_CONFIG)
        cfg = _config.load_cfg_from_cfg_file(config_path)
        self.vq_dims = W.VQDims.from_cfg(cfg)
        self.s2s = W.S2SDims()
        self.speaker_face_quan_num = cfg.face_quan_num
        self.speaker_zquant_dim = cfg.zquant_dim
        spec = W.slm_spec(self.vq_dims, self.s2s)
        build_param_tree(self, spec, W.synth_state_dict(spec, synthetic_seed))
        for pre, ck in (("speaker_vq.", vq_speaker_ckpt), ("listener_vq.", vq_listener_ckpt)):
            if ck is not None:
                sd = torch.load(ck, map_location="cpu")["state_dict"]
                own = self.state_dict()
                self.load_state_dict({pre + k.replace("module.", "", 1): v for k, v in sd.items()
                                      if pre + k.replace("module.", "", 1) in own}, strict=False)
        self.eval()

    def _engine_state_dict(self):
        return self.state_dict()

    @staticmethod
    def random_masking_unstructured(x, mask, mask_ratio, generator=None):
        """reference :170-183 -> bool [N,L], True = masked."""
        N, L_ = mask.shape
        out = torch.zeros(N, L_, dtype=torch.bool)
        lens = mask.sum(1).tolist()
        for i, n in enumerate(lens):
            idx = torch.randperm(int(n), generator=generator)[:int(n * mask_ratio)]
            out[i, :int(n)][idx] = True
        return out.to(mask.device)

    @torch.no_grad()
    def forward_vq(self, v_speaker, v_listener, mask):
        eng = self.engine(v_speaker.device)
        xl, lens = compact_by_mask(v_listener, mask)
        xs, _ = compact_by_mask(v_speaker, mask)
        z_l = eng.vq_encode(1, xl.contiguous(), lens, pe_mode=0, pad_value=-100).long()
        z_s = eng.vq_encode(0, xs.contiguous(), lens, pe_mode=0, pad_value=0).long()
        return z_s, z_l

    @torch.no_grad()
    def forward_encoder(self, v_speaker, v_listener, mask, mask_ratio=0.15, mask_speaker=None, mask_listener=None):
        if mask_speaker is None:
            mask_speaker = self.random_masking_unstructured(v_speaker, mask, mask_ratio)
        if mask_listener is None:
            mask_listener = self.random_masking_unstructured(v_listener, mask, mask_ratio)
        eng = self.engine(v_speaker.device)
        u8 = lambda m: m.to(torch.uint8).contiguous()
        x_s, x_l, x_joint = eng.slm_encode(v_speaker, v_listener, u8(mask), u8(mask_speaker), u8(mask_listener))
        return x_s, x_l, x_joint, mask_speaker, mask_listener

    @staticmethod
    def forward_contrastive(s_rep, l_rep, mask, bidirect_contrast=False):
        """reference :270-298."""
        valid = mask[..., None].to(s_rep.dtype)
        n = valid.sum(1)
        s = F.normalize((s_rep * valid).sum(1) / n, dim=-1)
        l_ = F.normalize((l_rep * valid).sum(1) / n, dim=-1)
        total = s @ l_.t() / 0.05
        ar = torch.arange(total.shape[0], device=total.device)

        def one(t):
            return (-torch.mean(torch.diag(F.log_softmax(t, dim=0))),
                    (F.softmax(t, dim=0).argmax(0) == ar).sum() / t.shape[0])
        nce, acc = one(total)
        if bidirect_contrast:
            n2, a2 = one(total.t())
            nce, acc = (nce + n2) / 2, (acc + a2) / 2
        return nce, acc

    @torch.no_grad()
    def _decode_tf(self, eng, x_joint, half, patch, z, v_audio, m8):
        T = z.shape[1]
        eng.set_context(x_joint[:, half * T:], v_audio, which_patch=patch, T=T)
        logits, row_loss, amax = eng.decode_tf(z, m8, None)
        n_valid = (z[:, 1:] != -100).sum().clamp(min=1)
        return row_loss.sum() / n_valid, logits, amax

    def forward_continuous_loss(self, pred, target, mask):
        return _masked_pairwise_loss(pred, target[:, 1:, :], mask[:, 1:])

    # ------------------------------------------------------------------ training
    def dimx_trainable_parameters(self):
        from . import train as T
        return T.slm_trainable_parameters(self)

    def train(self, mode=True):
        """nn.Module.train with both VQ-VAEs kept in eval (reference :96, :105)."""
        super().train(mode)
        self.speaker_vq.eval()
        self.listener_vq.eval()
        return self

    def _forward_autograd(self, v_speaker, v_listener, v_audio, mask, mask_ratio=0.15, mask_speaker=None, mask_listener=None,
                          z_s=None, z_l=None):
        from . import train as T
        mask = mask.bool()
        if z_s is None or z_l is None:
            z_s, z_l = self.forward_vq(v_speaker, v_listener, mask)
        if mask_speaker is None:
            mask_speaker = self.random_masking_unstructured(v_speaker, mask, mask_ratio)
        if mask_listener is None:
            mask_listener = self.random_masking_unstructured(v_listener, mask, mask_ratio)
        total, d = T.slm_loss(dict(self.named_parameters()), self.s2s, self.vq_dims, v_speaker.float(), v_listener.float(),
                              v_audio.float(), mask, mask_speaker.bool(), mask_listener.bool(), z_s.long(), z_l.long(),
                              self.speaker_vq.decoder.decoder_pos_embedding.pe, self.listener_vq.decoder.decoder_pos_embedding.pe)
        return total, {k: (v.detach() if torch.is_tensor(v) else v) for k, v in d.items()}, None

    def forward(self, v_speaker, v_listener, v_audio, mask, speaker_ids=None, listener_ids=None, mode="train",
                mask_speaker=None, mask_listener=None, return_aux=False, z_s=None, z_l=None):
        """reference :300-323 -> (total_loss, d, None)."""
        if (self.training and torch.is_grad_enabled() and not return_aux
                and any(p.requires_grad for p in self.parameters())):
            return self._forward_autograd(v_speaker, v_listener, v_audio, mask, mask_speaker=mask_speaker,
                                          mask_listener=mask_listener, z_s=z_s, z_l=z_l)
        with torch.no_grad():
            return self._forward_nograd(v_speaker, v_listener, v_audio, mask, mask_speaker, mask_listener, return_aux)

    def _forward_nograd(self, v_speaker, v_listener, v_audio, mask, mask_speaker=None, mask_listener=None, return_aux=False):
        mask = mask.bool()
        eng = self.engine(v_speaker.device)
        z_s, z_l = self.forward_vq(v_speaker, v_listener, mask)
        x_s, x_l, x_joint, mask_speaker, mask_listener = self.forward_encoder(
            v_speaker, v_listener, mask, mask_speaker=mask_speaker, mask_listener=mask_listener)
        nce, c_acc = self.forward_contrastive(x_s, x_l, mask)
        z_s = torch.where(mask_speaker, z_s, torch.full_like(z_s, -100))
        z_l = torch.where(mask_listener, z_l, torch.full_like(z_l, -100))
        m8 = mask.to(torch.uint8).contiguous()
        # z_s is predicted from the listener half of x_joint, z_l from the speaker half (:227-228)
        l_ce_s, px_s, am_s = self._decode_tf(eng, x_joint, 1, 1, z_s, v_audio, m8)
        l_ce_l, px_l, am_l = self._decode_tf(eng, x_joint, 0, 0, z_l, v_audio, m8)
        pred_s = eng.vq_decode(0, am_s, 0)
        pred_l = eng.vq_decode(1, am_l, 0)
        l_cont_s = self.forward_continuous_loss(pred_s, v_speaker, mask_speaker)
        l_cont_l = self.forward_continuous_loss(pred_l, v_listener, mask_listener)
        total_loss = l_ce_s + l_ce_l + l_cont_s + l_cont_l + nce
        d = {"l_ce_s": l_ce_s, "l_ce_l": l_ce_l, "l_cont_s": l_cont_s, "l_cont_l": l_cont_l, "nce": nce, "c_acc": c_acc}
        if return_aux:
            return total_loss, d, None, {"x_s": x_s, "x_l": x_l, "x_joint": x_joint, "px_s": px_s, "px_l": px_l,
                                         "pred_s": pred_s, "pred_l": pred_l}
        return total_loss, d, None


class SpeakerSLMFT(_EngineOwner):
    """Drop-in ``SpeakerSLMFT`` (DIM-Speaker, reference ``code/seq2seq_pretrain.py:516-757``):
    ``forward(v_speaker, v_speaker_emoca, v_audio, mask, template, mode, speaker_ids) -> (total_loss, d,
    pred_cont_seq_s_emoca [B,T-1,56])`` on the HIP library -- the SLM-geometry decoder (absolute positional embedding,
    context ``cat(x_l + patch_embed_dec_l, v_audio)``, teacher forcing without key masking: the reference builds its
    AutoregressiveWrapper without ``mask_prob``, :624), the speaker VQ-VAE decoder, and the converter head
    (``vertice_map_reverse_lstm`` + ``vertice_map_reverse``: ``dimx_mesh_head``, a HIP bidirectional LSTM).

    Deliberate differences:
      * the reference also maps the 70110-d input through ``vertice_mapping`` / ``squasher`` and encodes it with the
        speaker VQ-VAE (``z_s``, :712-715) and uses neither result; both are skipped here (as SLMFT's unused ``z_s``
        is); their parameters stay in the state dict;
      * ``mouth_map`` (vertex indices of the lip region) is a constructor argument: the reference reads
        ``../data/CodeTalker/BIWI/regions/lve.txt`` (:627).  With a map ``d['l_cont_s']`` is
        ``mse(mesh[..., map, :], v_speaker[:, 1:][..., map, :])`` over all clips (the reference's own indexing, :738,
        only type-checks at B = 1, where the two agree); with ``None`` the mesh head is not run in ``forward`` and the
        entry is 0;
      * ``v_speaker_emoca=None`` raises ``ValueError`` (the reference's ``evaluate_epoch_biwi`` passes None and fails
        inside ``forward_vq``);
      * randomness is injectable like SLMFT's (``noise``, ``greedy``, ``seed``, ``temperature``), and
        ``return_tokens`` / ``return_mesh`` append the code indices / the mesh to the result;
      * ``forward`` builds no autograd graph, whatever the grad mode.  Training lives beside it: the fine-tuning step of
        the reference's ``train_epoch_biwi`` is ``dimx.train_hip.SpeakerHipTrainer`` (forward and backward on the HIP
        library, over ``dimx_trainable_parameters()``), driven by ``dimx.x_engine_pt.train_epoch_biwi``;
        ``dimx.train.speaker_loss`` is its PyTorch-autograd checker.  The converter head receives no gradient there; it is
        trained through ``EmocaConverter`` (``dimx.train_hip.ConverterHipTrainer``, examples/train_converter.py), whose
        ``best_converter.pt`` is what ``converter_ckpt`` loads."""
    engine_variant = "speaker"

    def __init__(self, config_path=None, mesh_dim=70110, mouth_map=None, numeric_mode=L.MODE_PARITY_F32,
                 synthetic_seed=20260928, vq_speaker_ckpt=None, vq_listener_ckpt=None, converter_ckpt=None):
        super().__init__(numeric_mode)
        config_path = config_path or ("./config.yaml" if os.path.isfile("./config.yaml") else _config.DEFAULT_CONFIG)
        cfg = _config.load_cfg_from_cfg_file(config_path)
        self.vq_dims = W.VQDims.from_cfg(cfg)
        self.s2s = W.S2SDims()
        self.mesh_dim = int(mesh_dim)
        self.engine_mesh_dim = self.mesh_dim
        self.speaker_face_quan_num = cfg.face_quan_num
        self.speaker_zquant_dim = cfg.zquant_dim
        self.mouth_map = None if mouth_map is None else [int(i) for i in mouth_map]
        if self.mouth_map is not None:
            assert self.mesh_dim % 3 == 0 and all(0 <= i < self.mesh_dim // 3 for i in self.mouth_map), \
                "mouth_map holds vertex indices in [0, mesh_dim / 3)"
        spec = W.speaker_slmft_spec(self.mesh_dim, self.vq_dims, self.s2s)
        build_param_tree(self, spec, W.synth_state_dict(spec, synthetic_seed))
        for pre, ck in (("speaker_vq.", vq_speaker_ckpt), ("listener_vq.", vq_listener_ckpt)):
            if ck is not None:
                sd = torch.load(ck, map_location="cpu")["state_dict"]
                own = self.state_dict()
                self.load_state_dict({pre + k.replace("module.", "", 1): v for k, v in sd.items()
                                      if pre + k.replace("module.", "", 1) in own}, strict=False)
        if converter_ckpt is not None:      # EmocaConverter.state_dict() (best_converter.pt, reference :549-552)
            sd = torch.load(converter_ckpt, map_location="cpu")
            own = self.state_dict()
            self.load_state_dict({k: v for k, v in sd.items() if k in own and not k.startswith("speaker_vq.")}, strict=False)
        self.eval()

    def _engine_state_dict(self):
        return self.state_dict()

    def dimx_trainable_parameters(self):
        """(name, parameter) of what the reference's fine-tuning step gives a gradient, in state-dict order:
        ``decoder_joint.*``, ``patch_embed_dec_l``, ``speaker_embed.weight`` and ``speaker_vq.decoder.*`` -- what
        ``SpeakerHipTrainer`` keeps in its arenas.  Everything else keeps ``grad = None`` in the reference."""
        from . import train as T
        return T.speaker_trainable_parameters(self)

    # ------------------------------------------------------------------ reference sub-APIs
    @torch.no_grad()
    def forward_vq(self, v_speaker, v_listener, mask):
        """reference :692-706 with the tensors ``forward`` hands it: -> (None, z_listener [B,T] int64 padded with -100), the
        LISTENER VQ-VAE's codes of ``v_listener`` (``forward`` passes the speaker's EMOCA stream there).  The speaker
        VQ-VAE encoding of the first argument is never used by the reference and is not computed."""
        eng = self.engine(v_listener.device)
        xl, lens = compact_by_mask(v_listener, mask.bool())
        return None, eng.vq_encode(1, xl.contiguous(), lens, pe_mode=0, pad_value=-100).long()

    def forward_encoder(self, v_speaker, mask):
        """reference :638-648, never called by the reference's ``forward``.  It is encoder_s -> encoder_joint -> norm_s on
        the speaker stream alone; the library's variant-2 encoder stage (``dimx_slm_encode``) runs encoder_joint over the
        concatenated speaker + listener sequence, so its speaker output is a different function and this method does not
        map onto it."""
        raise NotImplementedError("SpeakerSLMFT.forward_encoder is not built: the reference's forward never calls it, and "
                                  "dimx_slm_encode's joint encoder sees the listener half too")

    @torch.no_grad()
    def forward_decoder(self, x_l, z_s, x_a, mask, mode="train", noise=None, greedy=False, seed=None, temperature=1.0,
                        filter_logits_fn=None, filter_kwargs=None):
        """reference :650-658 -> (l_ce_s, logits [B,T-1,512]) for mode 'train', (0.0, tokens [B,T-1]) otherwise.
        ``filter_logits_fn`` / ``filter_kwargs``: the sampler filter of the generation (SLMFT.forward_decoder)."""
        eng = self.engine(x_a.device)
        m8 = mask.bool().to(torch.uint8).contiguous()
        B, T = z_s.shape
        if mode == "train":
            eng.set_context(x_l, x_a, which_patch=1, for_generate=False)
            logits, row_loss, _ = eng.decode_tf(z_s, m8, None)
            n_valid = (z_s[:, 1:] != -100).sum().clamp(min=1)
            return row_loss.sum() / n_valid, logits
        eng.set_context(x_l, x_a, which_patch=1, for_generate=True)
        if greedy:
            temperature, seed_v = 0.0, 0
        else:
            seed_v = 0 if noise is not None else SLMFT._user_seed(seed)
        tokens = eng.generate(z_s[:, 0], m8, T, temperature, 52, noise, seed_v, filter_logits_fn=filter_logits_fn,
                              filter_kwargs=filter_kwargs)
        return 0.0, tokens.long()

    @torch.no_grad()
    def forward_vq_decoder(self, logits_s, type="emoca", mode="train", template=None):
        """reference :660-676: argmax (train) / tokens (val) -> SPEAKER VQ-VAE codebook + decoder -> converter head ->
        (mesh [B,L,V], emoca [B,L,56]).  ``template`` [B,V] (optional) is added to the mesh inside the head's last GEMM
        (the reference adds it in ``forward``, :730)."""
        if type != "emoca":
            raise NotImplementedError("forward_vq_decoder(type=%r): the vertice_map_reverse_lstm_2 / vertice_map_reverse2 "
                                      "head is dead code in the reference (:728) and is not built" % (type,))
        pred_seq_s = torch.argmax(logits_s, dim=-1) if mode == "train" else logits_s
        eng = self.engine(pred_seq_s.device)
        emoca = eng.vq_decode(0, pred_seq_s, 0)
        return eng.mesh_head(emoca, template), emoca

    # ------------------------------------------------------------------ forward
    def forward(self, v_speaker, v_speaker_emoca, v_audio, mask, template, mode="train", speaker_ids=None, noise=None,
                greedy=False, seed=None, temperature=1.0, return_tokens=False, return_mesh=False, filter_logits_fn=None,
                filter_kwargs=None):
        """reference :708-757 -> (total_loss, d, pred_cont_seq_s_emoca [B,T-1,56]) (+ tokens [B,T-1], + mesh [B,T-1,V])."""
        if v_speaker_emoca is None:
            raise ValueError("SpeakerSLMFT.forward needs v_speaker_emoca (the EMOCA stream the codes are taken from)")
        with torch.no_grad(), self.engine_pinned():
            mask = mask.bool()
            dev = v_audio.device
            B, T = mask.shape
            _, z = self.forward_vq(None, v_speaker_emoca, mask)
            if speaker_ids is None:
                x_l = torch.zeros(B, T, self.s2s.dim, device=dev)
            else:
                x_l = self.speaker_embed.weight[speaker_ids.long()].unsqueeze(1).repeat(1, T, 1).contiguous()
            l_ce_s, px_s = self.forward_decoder(x_l, z, v_audio, mask, mode=mode, noise=noise, greedy=greedy, seed=seed,
                                                temperature=temperature, filter_logits_fn=filter_logits_fn,
                                                filter_kwargs=filter_kwargs)
            eng = self.engine(dev)
            tokens = torch.argmax(px_s, dim=-1) if mode == "train" else px_s
            pred_emoca = eng.vq_decode(0, tokens, 0)
            mesh = None
            l_mouth = 0
            if self.mouth_map is not None or return_mesh:
                mesh = eng.mesh_head(pred_emoca, template)
            if self.mouth_map is not None:
                idx = torch.as_tensor(self.mouth_map, device=dev, dtype=torch.long)
                tgt = v_speaker[:, 1:, :].reshape(B, T - 1, -1, 3)[:, :, idx, :]
                l_mouth = F.mse_loss(mesh.view(B, T - 1, -1, 3)[:, :, idx, :], tgt.to(mesh.dtype))
            l_emoca = F.mse_loss(pred_emoca, v_speaker_emoca[:, 1:, :].to(pred_emoca.dtype))
            total_loss = l_ce_s + l_emoca
            d = {"l_ce_s": 0, "l_ce_l": l_ce_s, "l_cont_s": l_mouth, "l_cont_l": l_emoca, "nce": 0, "c_acc": 0}
            out = (total_loss, d, pred_emoca)
            if return_tokens:
                out += (tokens,)
            if return_mesh:
                out += (mesh,)
            return out


class EmocaConverter(_EngineOwner):
    """Drop-in ``EmocaConverter`` (reference ``code/seq2seq_pretrain.py:759-842``):
    ``forward(inputs, template, v_speaker) -> (mesh [B,L,V], None)`` = ``vertice_map_reverse(vertice_map_reverse_lstm(
    speaker_vq(v_speaker)[0])) + template[:, None]``; ``inputs`` is unused, as in the reference (:829-831 are commented
    out).  The state dict has the reference's keys (``speaker_vq.*`` and the converter tensors).  ``forward`` builds no
    autograd graph; the head is trained by ``dimx.train_hip.ConverterHipTrainer`` (forward and backward on the HIP library)
    over ``dimx_trainable_parameters()``."""
    engine_variant = "speaker"

    def __init__(self, config_path=None, mesh_dim=70110, numeric_mode=L.MODE_PARITY_F32, synthetic_seed=20260928,
                 vq_speaker_ckpt=None):
        super().__init__(numeric_mode)
        config_path = config_path or ("./config.yaml" if os.path.isfile("./config.yaml") else _config.DEFAULT_CONFIG)
        cfg = _config.load_cfg_from_cfg_file(config_path)
        self.vq_dims = W.VQDims.from_cfg(cfg)
        self.mesh_dim = int(mesh_dim)
        self.engine_mesh_dim = self.mesh_dim
        self.speaker_face_quan_num = cfg.face_quan_num
        self.speaker_zquant_dim = cfg.zquant_dim
        spec = W.vq_spec(self.vq_dims, "speaker_vq.") + W.emoca_converter_spec(self.mesh_dim, self.vq_dims.in_dim)
        build_param_tree(self, spec, W.synth_state_dict(spec, synthetic_seed))
        if vq_speaker_ckpt is not None:
            sd = torch.load(vq_speaker_ckpt, map_location="cpu")["state_dict"]
            own = self.state_dict()
            self.load_state_dict({"speaker_vq." + k.replace("module.", "", 1): v for k, v in sd.items()
                                  if "speaker_vq." + k.replace("module.", "", 1) in own}, strict=False)
        self.criterion = nn.MSELoss()
        self.eval()

    def _engine_state_dict(self):
        return self.state_dict()

    def dimx_trainable_parameters(self):
        """the 20 tensors the reference's loop gives a gradient (``vertice_map_reverse_lstm.*``, ``vertice_map_reverse.*``), in
        state-dict order: what ``ConverterHipTrainer`` keeps in its arenas.  ``speaker_vq.*`` is frozen."""
        return [p for n, p in self.named_parameters()
                if n.startswith("vertice_map_reverse_lstm.") or n.startswith("vertice_map_reverse.")]

    @torch.no_grad()
    def forward(self, inputs, template, v_speaker):
        with self.engine_pinned():
            eng = self.engine(v_speaker.device)
            idx, _ = eng.vq_encode(0, v_speaker, None, pe_mode=1, return_z=True)
            dec = eng.vq_decode(0, idx, 0)      # VQAutoEncoder.forward: decode(quant) of the codebook rows
            return eng.mesh_head(dec, template), None
