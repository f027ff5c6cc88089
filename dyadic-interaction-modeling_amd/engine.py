"""Engine: one libdimx_hip handle on one GPU + its device workspace.

This is the thin host layer above the C-ABI: it owns the handle, uploads a reference-shaped
state dict, sizes the workspace with ``dimx_workspace_bytes`` and forwards torch CUDA tensors
as raw pointers on the current HIP stream.  All arithmetic happens in the HIP library.
"""
import ctypes

import numpy as np
import torch

from . import lib as L
from . import sampling


class Engine:
    def __init__(self, device=None, mode=L.MODE_PARITY_F32, variant="slmft", mesh_dim=0):
        """variant: "slmft" (DIM-Listener, code/seq2seq_pretrain.py), "legacy" (ListenerGenerator, code/seq2seq.py),
        "slm" (the pre-training model) or "speaker" (DIM-Speaker: the "slm" geometry plus the mesh head of width
        ``mesh_dim``)."""
        if not torch.cuda.is_available():
            raise L.DimxError("dimx needs a ROCm GPU (torch.cuda.is_available() is False); "
                              "there is no CPU fallback")
        self.device = torch.device(device if device is not None else "cuda:0")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.lib = L.load()
        self.mode = mode
        assert variant in ("slmft", "legacy", "slm", "speaker")
        self.variant = variant
        if variant == "speaker":
            assert mesh_dim > 0, "the speaker variant needs mesh_dim"
            self.dims = L.speaker_dims(mesh_dim)
        else:
            self.dims = {"slmft": L.default_dims, "legacy": L.legacy_dims, "slm": L.slm_dims}[variant]()
        h = ctypes.c_void_p()
        L.check(self.lib.dimx_create(ctypes.byref(h), self.device.index, ctypes.byref(self.dims), mode),
                "dimx_create")
        self.h = h
        self._ws = None
        self._ws_bytes = 0

    def close(self):
        if getattr(self, "h", None):
            self.lib.dimx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ weights
    def load_state_dict(self, sd, new_checkpoint=True):
        """Upload every tensor of a reference-shaped state dict (extra reference keys that
        are not on the hot path are ignored by the library).  ``new_checkpoint`` (default): ``sd`` is a whole checkpoint, the
        optional tensors an earlier one brought (``project_in.bias`` / ``to_logits.bias``) are forgotten first
        (``dimx_begin_checkpoint``); pass False for the further chunks of a checkpoint loaded in pieces."""
        if new_checkpoint:
            L.check(self.lib.dimx_begin_checkpoint(self.h), "dimx_begin_checkpoint")
        keep, descs = [], []
        for name, t in sd.items():
            a = t.detach().to("cpu", torch.float32).contiguous().numpy()
            keep.append(a)
            d = L.WeightDesc()
            d.name = name.encode()
            d.data = a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
            d.ndim = a.ndim
            for i, s in enumerate(a.shape):
                d.shape[i] = s
            descs.append(d)
        arr = (L.WeightDesc * len(descs))(*descs)
        L.check(self.lib.dimx_load_weights(self.h, arr, len(descs)), "dimx_load_weights")

    def missing_weights(self):
        return self.lib.dimx_missing_weights(self.h)

    # ------------------------------------------------------------------ workspace
    def workspace(self, B, T, n_samples=1, prompt_frames=1, guided=False):
        """``prompt_frames`` P0 > 1: room for the prefill of a prompted generation too (dimx_workspace_bytes_prompt).
        ``guided``: room for a guided generation (dimx_workspace_bytes_guided: 2B rows of self-attention caches)."""
        if guided:
            need = max(self.lib.dimx_workspace_bytes_guided(self.h, B, T), self.lib.dimx_workspace_bytes_samples(self.h, B, T, n_samples))
        elif prompt_frames > 1:
            need = self.lib.dimx_workspace_bytes_prompt(self.h, B, T, n_samples, int(prompt_frames))
        else:
            need = self.lib.dimx_workspace_bytes_samples(self.h, B, T, n_samples)
        if need == 0:
            raise L.DimxError("dimx_workspace_bytes(%d,%d) = 0" % (B, T))
        if self._ws is None or self._ws_bytes < need:
            self._ws = None
            self._ws = torch.empty(need + 256, dtype=torch.uint8, device=self.device)
            self._ws_bytes = need
        base = self._ws.data_ptr()
        aligned = (base + 255) // 256 * 256
        return ctypes.c_void_p(aligned), self._ws_bytes - (aligned - base) + 256

    def _s(self):
        return L.stream_ptr(self.device)

    def _chk(self, *ts):
        for t in ts:
            if t is not None:
                assert t.device == self.device and t.is_contiguous(), "tensor must be contiguous on %s" % self.device

    # ------------------------------------------------------------------ stages
    def vq_encode(self, which, x, lens=None, pe_mode=0, row_offset=0, pad_value=-100, return_z=False):
        B, T, _ = x.shape
        x = x.to(torch.float32).contiguous()
        self._chk(x, lens)
        fqn = self.dims.spk_face_quan_num if (self.variant == "legacy" and which == 0) else 1
        idx = torch.empty(B, T * fqn, dtype=torch.int32, device=self.device)
        z = torch.empty(B, T, fqn * self.dims.vq_zdim, dtype=torch.float32, device=self.device) if return_z else None
        ws, wsb = self.workspace(B, T)
        L.check(self.lib.dimx_vq_encode(self.h, which, L.ptr(x), L.ptr(lens), B, T, pe_mode, row_offset,
                                        pad_value, L.ptr(idx), L.ptr(z), ws, wsb, self._s()), "dimx_vq_encode")
        return (idx, z) if return_z else idx

    def vq_argmin(self, which, z, with_stats=False):
        z = z.to(torch.float32).contiguous()
        N = z.shape[0]
        idx = torch.empty(N, dtype=torch.int32, device=self.device)
        bd = torch.empty(N, dtype=torch.float32, device=self.device) if with_stats else None
        mg = torch.empty(N, dtype=torch.float32, device=self.device) if with_stats else None
        L.check(self.lib.dimx_vq_argmin(self.h, which, L.ptr(z), N, L.ptr(idx), L.ptr(bd), L.ptr(mg), self._s()),
                "dimx_vq_argmin")
        return (idx, bd, mg) if with_stats else idx

    def vq_decode(self, which, idx, row_offset=0, rows_per_clip=1):
        B, Lq = idx.shape
        idx = idx.to(torch.int32).contiguous()
        self._chk(idx)
        out = torch.empty(B, Lq, self.dims.vq_in_dim, dtype=torch.float32, device=self.device)
        ws, wsb = self.workspace(B, Lq)
        L.check(self.lib.dimx_vq_decode(self.h, which, L.ptr(idx), B, Lq, row_offset, rows_per_clip, L.ptr(out), ws, wsb,
                                        self._s()), "dimx_vq_decode")
        return out

    def vq_decode_latent(self, which, z, row_offset=0):
        """z [B,L,128] f32 (time-major latents, quantised or not) -> [B,L,56]: VQAutoEncoder.decode on what it is given."""
        B, Lq, _ = z.shape
        z = z.to(torch.float32).contiguous()
        self._chk(z)
        out = torch.empty(B, Lq, self.dims.vq_in_dim, dtype=torch.float32, device=self.device)
        ws, wsb = self.workspace(B, Lq)
        L.check(self.lib.dimx_vq_decode_latent(self.h, which, L.ptr(z), B, Lq, row_offset, L.ptr(out), ws, wsb,
                                               self._s()), "dimx_vq_decode_latent")
        return out

    def encode_speaker(self, v_speaker, mask_u8):
        """SLMFT.forward_encoder alone -> x_s [B,T,384] f32 (no audio, no context, no K/V projection)."""
        B, T, _ = v_speaker.shape
        v_speaker = v_speaker.to(torch.float32).contiguous()
        self._chk(v_speaker, mask_u8)
        x_s = torch.empty(B, T, self.dims.dim, dtype=torch.float32, device=self.device)
        ws, wsb = self.workspace(B, T)
        L.check(self.lib.dimx_encode_speaker(self.h, L.ptr(v_speaker), L.ptr(mask_u8), B, T, L.ptr(x_s), ws, wsb,
                                             self._s()), "dimx_encode_speaker")
        return x_s

    def set_shard(self, row_offset=0, rows_total=0):
        """This engine generates clips [row_offset, row_offset+B) of a sharded batch of rows_total clips (only the
        sampler's counter-based generator depends on it); (0, 0) = unsharded."""
        L.check(self.lib.dimx_set_shard(self.h, int(row_offset), int(rows_total)), "dimx_set_shard")

    def encode_ctx(self, v_speaker, v_audio, mask_u8, for_generate, return_x_s=False, n_samples=1, prompt_frames=1, guided=False):
        """``guided``: the context of a ``generate(guidance=)`` call -- the workspace is sized for it (a workspace grown between
        the two calls would drop the context)."""
        B, T, _ = v_speaker.shape
        v_speaker = v_speaker.to(torch.float32).contiguous()
        v_audio = v_audio.to(torch.float32).contiguous() if v_audio is not None else None
        if self.variant == "slmft" and v_audio is None:
            raise L.DimxError("encode_ctx: the SLMFT variant needs v_audio")
        self._chk(v_speaker, v_audio, mask_u8)
        x_s = torch.empty(B, T, self.dims.dim, dtype=torch.float32, device=self.device) if return_x_s else None
        ws, wsb = self.workspace(B, T, n_samples, prompt_frames, guided)   # the generate call that follows must see the same workspace
        L.check(self.lib.dimx_encode_ctx(self.h, L.ptr(v_speaker), L.ptr(v_audio), L.ptr(mask_u8), B, T,
                                         1 if for_generate else 0, L.ptr(x_s), ws, wsb, self._s()),
                "dimx_encode_ctx")
        return x_s

    def slm_encode(self, v_speaker, v_listener, mask_u8, mask_speaker_u8=None, mask_listener_u8=None):
        """SLM.forward_encoder -> (x_s, x_l [B,T,384], x_joint [B,2T,384]) f32."""
        B, T, _ = v_speaker.shape
        v_speaker = v_speaker.to(torch.float32).contiguous()
        v_listener = v_listener.to(torch.float32).contiguous()
        self._chk(v_speaker, v_listener, mask_u8, mask_speaker_u8, mask_listener_u8)
        dim = self.dims.dim
        x_s = torch.empty(B, T, dim, dtype=torch.float32, device=self.device)
        x_l = torch.empty(B, T, dim, dtype=torch.float32, device=self.device)
        x_j = torch.empty(B, 2 * T, dim, dtype=torch.float32, device=self.device)
        ws, wsb = self.workspace(B, T)
        L.check(self.lib.dimx_slm_encode(self.h, L.ptr(v_speaker), L.ptr(v_listener), L.ptr(mask_u8),
                                         L.ptr(mask_speaker_u8), L.ptr(mask_listener_u8), B, T, L.ptr(x_s), L.ptr(x_l),
                                         L.ptr(x_j), ws, wsb, self._s()), "dimx_slm_encode")
        return x_s, x_l, x_j

    def set_context(self, x, v_audio, which_patch=0, for_generate=False, T=None, n_samples=1, prompt_frames=1, guided=False):
        """context = cat(x[:, :T] + patch_embed_dec_{s|l}, v_audio) + cross K/V; x [B, rows>=T, dim] f32."""
        B, rows, _ = x.shape
        T = T or rows
        x = x.to(torch.float32)
        v_audio = v_audio.to(torch.float32).contiguous()
        assert x.stride(2) == 1 and x.stride(1) == x.shape[2], "x rows must be dense"
        ldx_rows = x.stride(0) // x.shape[2]
        ws, wsb = self.workspace(B, T, n_samples, prompt_frames, guided)
        L.check(self.lib.dimx_set_context(self.h, ctypes.c_void_p(x.data_ptr()), ldx_rows, which_patch, L.ptr(v_audio),
                                          B, T, 1 if for_generate else 0, ws, wsb, self._s()), "dimx_set_context")

    def legacy_speaker_features(self, v_speaker, mask_u8, return_idx=False):
        """x_speaker [B,T,1024] of ListenerGenerator.forward (code/seq2seq.py:224-241); v_speaker must hold each
        clip's valid frames first."""
        B, T, _ = v_speaker.shape
        v_speaker = v_speaker.to(torch.float32).contiguous()
        self._chk(v_speaker, mask_u8)
        fqn = self.dims.spk_face_quan_num
        x = torch.empty(B, T, fqn * self.dims.vq_zdim, dtype=torch.float32, device=self.device)
        idx = torch.empty(B, T * fqn, dtype=torch.int32, device=self.device) if return_idx else None
        ws, wsb = self.workspace(B, T)
        L.check(self.lib.dimx_legacy_speaker_features(self.h, L.ptr(v_speaker), L.ptr(mask_u8), B, T, L.ptr(x),
                                                      L.ptr(idx), ws, wsb, self._s()),
                "dimx_legacy_speaker_features")
        return (x, idx) if return_idx else x

    def n_gen(self, T):
        """tokens generated per sequence: T-1 (SLMFT) / T (legacy, code/seq2seq.py:300)."""
        return T if self.variant == "legacy" else T - 1

    def decode_tf(self, z_l, mask_u8, kv_mask_u8=None, lookahead=None):
        """Teacher-forced decoder pass -> (logits [B,T-1,V], row_loss, argmax).  With an integer ``lookahead`` L the pass runs under
        online visibility (dimx_decode_tf_win; the definition is dimx.online): row t sees the context rows below
        clamp(t + 2 + L, 1, T).  That form reads a context built with ``for_generate=True`` and takes no random key mask."""
        B, T = z_l.shape
        z_l = z_l.to(torch.int32).contiguous()
        self._chk(z_l, mask_u8, kv_mask_u8)
        n = T - 1
        logits = torch.empty(B, n, self.dims.num_tokens, dtype=torch.float32, device=self.device)
        row_loss = torch.empty(B, n, dtype=torch.float32, device=self.device)
        amax = torch.empty(B, n, dtype=torch.int32, device=self.device)
        ws, wsb = self.workspace(B, T)
        if lookahead is not None:
            if kv_mask_u8 is not None:
                raise L.DimxError("decode_tf(lookahead=): the windowed pass takes no random key mask")
            L.check(self.lib.dimx_decode_tf_win(self.h, L.ptr(z_l), L.ptr(mask_u8), B, T, int(lookahead), L.ptr(logits), L.ptr(row_loss),
                                                L.ptr(amax), ws, wsb, self._s()), "dimx_decode_tf_win")
            return logits, row_loss, amax
        L.check(self.lib.dimx_decode_tf(self.h, L.ptr(z_l), L.ptr(mask_u8), L.ptr(kv_mask_u8), B, T, L.ptr(logits),
                                        L.ptr(row_loss), L.ptr(amax), ws, wsb, self._s()), "dimx_decode_tf")
        return logits, row_loss, amax

    def set_sampler_filter(self, kind=0, a=0.0, b=0.0):
        """The handle's sampler filter (dimx_set_sampler_filter): kind 0 = the call's top_k.  ``generate`` sets and restores it
        around a call with ``filter_logits_fn``; an invalid setting raises and leaves the previous one in force."""
        L.check(self.lib.dimx_set_sampler_filter(self.h, int(kind), float(a), float(b)), "dimx_set_sampler_filter")

    def set_cross_lookahead(self, lookahead=None):
        """Online generation (dimx_set_cross_lookahead; the definition is dimx.online): with an integer ``lookahead`` L the cross
        attention of decode step t sees the context rows j < clamp(t + 2 + L, 1, T) only; None switches the window off (every
        row, the reference's behaviour).  Holds for this engine's generate calls until it is set again."""
        L.check(self.lib.dimx_set_cross_lookahead(self.h, 0 if lookahead is None else 1, 0 if lookahead is None else int(lookahead)),
                "dimx_set_cross_lookahead")

    def cross_lookahead(self):
        """The engine's cross-attention window: the look-ahead, or None while it is off."""
        on, la = ctypes.c_int(0), ctypes.c_int(0)
        L.check(self.lib.dimx_cross_lookahead(self.h, ctypes.byref(on), ctypes.byref(la)), "dimx_cross_lookahead")
        return la.value if on.value else None

    def cross_kv8_bytes(self, B, T):
        """Bytes of the FP8 cross K/V buffer of a B x T generation (dimx_cross_kv8_bytes; 0 = shape not supported)."""
        return int(self.lib.dimx_cross_kv8_bytes(self.h, int(B), int(T)))

    def set_cross_kv8(self, buf=None):
        """FP8 cross-attention K/V (dimx_set_cross_kv8; the definition is dimx.kv8): with a uint8 device tensor ``buf`` of at least
        ``cross_kv8_bytes(B, T)`` bytes, this engine's generate calls quantise the context K / V into it once and every decode
        step's cross attention reads the codes; None switches it off.  ``generate(kv8=True)`` does both around one call."""
        if buf is None:
            L.check(self.lib.dimx_set_cross_kv8(self.h, None, 0), "dimx_set_cross_kv8")
            return
        assert buf.dtype == torch.uint8 and buf.is_contiguous() and buf.device == self.device
        L.check(self.lib.dimx_set_cross_kv8(self.h, L.ptr(buf), buf.numel()), "dimx_set_cross_kv8")

    def cross_kv8(self):
        """(pointer, bytes) of the buffer in force, or None while FP8 cross K/V is off."""
        p, n = ctypes.c_void_p(None), ctypes.c_size_t(0)
        L.check(self.lib.dimx_cross_kv8(self.h, ctypes.byref(p), ctypes.byref(n)), "dimx_cross_kv8")
        return (p.value, n.value) if p.value else None

    def set_cross_kv8_samples(self, on=True):
        """FP8 cross K/V for best-of-N (dimx_set_cross_kv8_samples; dimx.kv8.attention_rows): with this on and a cross buffer set,
        generate calls take ``n_samples > 1`` and every layer's multi-query cross attention reads the codes.
        ``generate(kv8_samples=True)`` sets buffer and flag around one call."""
        L.check(self.lib.dimx_set_cross_kv8_samples(self.h, 1 if on else 0), "dimx_set_cross_kv8_samples")

    def cross_kv8_samples(self):
        """The handle's current setting (bool)."""
        on = ctypes.c_int(0)
        L.check(self.lib.dimx_cross_kv8_samples(self.h, ctypes.byref(on)), "dimx_cross_kv8_samples")
        return bool(on.value)

    def cross_kv8_buffer(self):
        """The uint8 tensor the last ``generate(kv8=True)`` quantised into (None before the first); ``cross_kv8_layers`` views it."""
        return getattr(self, "_kv8", None)

    def cross_kv8_layers(self, B, T, buf=None):
        """Per decoder layer (kcodes, vcodes [B, H, Tp, 64] uint8, kscale, vscale [B, H, Tp] f32): views into ``buf`` (default: the
        engine's buffer) by the layout of include/dimx.h (dimx.kv8.buffer_layout)."""
        from . import kv8 as _kv8
        buf = self.cross_kv8_buffer() if buf is None else buf
        H, Tp = self.dims.heads, (T + 7) // 8 * 8
        lay, total = _kv8.buffer_layout(self.dims.dec_depth, B, H, Tp)
        assert buf.numel() >= total
        nc, ns = B * H * Tp * 64, B * H * Tp * 4
        return [(buf[o["kcodes"]:o["kcodes"] + nc].view(B, H, Tp, 64), buf[o["vcodes"]:o["vcodes"] + nc].view(B, H, Tp, 64),
                 buf[o["kscale"]:o["kscale"] + ns].view(torch.float32).view(B, H, Tp),
                 buf[o["vscale"]:o["vscale"] + ns].view(torch.float32).view(B, H, Tp)) for o in lay]

    def self_kv8_bytes(self, R, T):
        """Bytes of the FP8 self K/V buffer of a generation of R = B * n_samples sequences of T frames (dimx_self_kv8_bytes; 0 = shape
        not supported)."""
        return int(self.lib.dimx_self_kv8_bytes(self.h, int(R), int(T)))

    def set_self_kv8(self, buf=None):
        """FP8 self-attention K/V caches (dimx_set_self_kv8; the definition is dimx.kv8.self_step): with a uint8 device tensor ``buf``
        of at least ``self_kv8_bytes(B * n_samples, T)`` bytes, every decode step of this engine's generate calls quantises its k / v
        row into it and attends over the codes; None switches it off.  ``generate(self_kv8=True)`` does both around one call."""
        if buf is None:
            L.check(self.lib.dimx_set_self_kv8(self.h, None, 0), "dimx_set_self_kv8")
            return
        assert buf.dtype == torch.uint8 and buf.is_contiguous() and buf.device == self.device
        L.check(self.lib.dimx_set_self_kv8(self.h, L.ptr(buf), buf.numel()), "dimx_set_self_kv8")

    def self_kv8(self):
        """(pointer, bytes) of the buffer in force, or None while FP8 self K/V is off."""
        p, n = ctypes.c_void_p(None), ctypes.c_size_t(0)
        L.check(self.lib.dimx_self_kv8(self.h, ctypes.byref(p), ctypes.byref(n)), "dimx_self_kv8")
        return (p.value, n.value) if p.value else None

    def set_beam_kv8(self, on=True):
        """FP8 K/V caches for beam search (dimx_set_beam_kv8; dimx.kv8.reorder): with this on, ``generate_beam`` takes the cross
        and / or self buffer in force instead of refusing them.  ``generate_beam(beam_kv8=...)`` sets buffers and switch around
        one call."""
        L.check(self.lib.dimx_set_beam_kv8(self.h, 1 if on else 0), "dimx_set_beam_kv8")

    def beam_kv8(self):
        """The handle's current setting (bool)."""
        on = ctypes.c_int(0)
        L.check(self.lib.dimx_beam_kv8(self.h, ctypes.byref(on)), "dimx_beam_kv8")
        return bool(on.value)

    def self_kv8_buffer(self):
        """The uint8 tensor the last ``generate(self_kv8=True)`` appended to (None before the first); ``self_kv8_layers`` views it."""
        return getattr(self, "_skv8", None)

    def self_kv8_layers(self, R, T, buf=None):
        """Per decoder layer (kcodes, vcodes [R, H, Tp, 64] uint8, kscale, vscale [R, H, Tp] f32): views into ``buf`` (default: the
        engine's buffer) by dimx.kv8.buffer_layout with the R sequences in place of the clips.  Positions a generation did not reach
        (and layer 0 where its self attention read the token table) hold what the buffer held before."""
        return self.cross_kv8_layers(R, T, self.self_kv8_buffer() if buf is None else buf)

    def generate(self, start, mask_u8, T, temperature=1.0, top_k=52, noise=None, seed=0, return_logits=False,
                 n_samples=1, prompt=None, prompt_len=None, prefill=None, no_prefill=False, filter_logits_fn=None,
                 filter_kwargs=None, return_scores=False, lookahead=None, guidance=None, return_branches=False, kv8=False, self_kv8=False,
                 kv8_samples=False):
        """n_samples S > 1: S sequences per clip in one pass (rows b*S+s), sharing the clip's context K/V.

        ``kv8_samples``: ``kv8`` for any ``n_samples`` (``set_cross_kv8_samples``; dimx.kv8.attention_rows): the cross buffer and
        the flag are set for the call and cleared afterwards; with S > 1 every layer's cross attention is the multi-query launch
        over the codes.  Works with ``self_kv8``, ``lookahead``, ``prompt``, ``filter_logits_fn``, ``return_logits`` and
        ``return_scores``; ``guidance`` with S > 1 is refused by the library.  ``kv8=True`` alone stays as it is.

        ``self_kv8``: FP8 self-attention K/V caches for this call (``set_self_kv8``; dimx.kv8.self_step): the engine allocates (or
        reuses) its buffer, sets it for the call and clears the setting afterwards.  Any ``n_samples``; works with ``lookahead``,
        ``prompt``, ``filter_logits_fn``, ``return_logits``, ``return_scores`` and, at one sample per clip, ``kv8``; ``guidance`` is
        refused by the library.  False leaves the engine's setting as it is.

        ``kv8``: FP8 cross-attention K/V for this call (``set_cross_kv8``; dimx.kv8): the engine allocates (or reuses) its buffer,
        sets it for the call and clears the setting afterwards.  Works with ``lookahead``, ``prompt``, ``guidance``,
        ``filter_logits_fn``, ``return_logits`` and ``return_scores``; ``n_samples > 1`` is refused by the library.  False leaves
        the engine's setting as it is.

        ``guidance``: classifier-free guidance with this scale (dimx_generate_guided, include/dimx.h; the definition is
        dimx.guidance): every step samples from cond + (scale - 1) * (cond - uncond), the second branch being the decoder without
        a context.  None is today's call, launch for launch; 1.0 computes the same tokens by the guided step.  The context must
        have been built with ``guided=True`` (``encode_ctx`` / ``set_context``).  ``return_logits`` / ``return_scores`` then refer to
        the GUIDED logits; ``return_branches`` appends both branches' raw logits [2, B, n, 512] to the return value.  A prompt goes
        through forced decode steps; ``filter_logits_fn`` and ``lookahead`` act as without guidance.  One sample per clip.

        ``return_scores``: the return value gains a trailing dimx.scoring.SeqScores (score f64, count int32, both [B*S]): the
        log-likelihood of every sampled sequence under softmax(raw logits) over the columns dimx.scoring.scored_columns names
        (positions inside the clip's length and past its prompt), by dimx_op_seq_logprob on this call's logits dump.  The dump is
        requested internally whether or not ``return_logits`` is set and costs R x n x 2 KiB of device memory for the call -- 1.57 GB
        at 256 clips x 10 tries x 300 frames; lengths and prompt lengths are derived on the device, nothing is read back.

        ``filter_logits_fn`` / ``filter_kwargs``: the sampler filter of AutoregressiveWrapper.generate -- ``top_k``, ``top_p``,
        ``min_p`` or ``top_a`` of dimx.sampling, as the object or its name, with that function's keyword arguments.  None is
        top-k with the given ``top_k``.  The filter holds for this call only.

        ``prompt`` [B,Pmax] (1 <= Pmax <= T-1; ``start`` is then ignored and may be None): continue the given tokens
        (dimx_generate_prompted, include/dimx.h).  ``prompt_len`` [B] int32 on the device: per-clip prompt lengths, clamped to
        [prefill, Pmax]; None = Pmax.  ``prefill`` is P0, the prefix that is prefilled by one teacher-forced pass (default:
        Pmax when ``prompt_len`` is None, else 1); the context must have been built with ``prompt_frames >= prefill`` (a
        workspace grown in between invalidates it).  ``no_prefill``: the whole prompt goes through forced decode steps.
        Returned tokens keep their shape: column c is position c+1, columns < plen-1 repeat the prompt; with
        ``return_logits`` the columns < P0-1 are zero.

        ``lookahead``: online generation for this call (``set_cross_lookahead``; the previous setting is restored afterwards).
        None leaves the engine's setting as it is.  With the window on, a prompt goes through forced decode steps (as
        ``no_prefill``) unless ``prefill`` is ``"window"`` (P0 by the default rule above) or ``("window", P0)``: then the first P0
        codes are prefilled by one teacher-forced pass under the window (flags bit 1 of dimx_generate_prompted).  With
        the window off that spelling is the plain prefill."""
        if kv8_samples:
            self.set_cross_kv8_samples(True)
            try:
                return self.generate(start, mask_u8, T, temperature, top_k, noise, seed, return_logits, n_samples, prompt, prompt_len,
                                     prefill, no_prefill, filter_logits_fn, filter_kwargs, return_scores, lookahead, guidance,
                                     return_branches, True, self_kv8)
            finally:
                self.set_cross_kv8_samples(False)
        if self_kv8:
            R = (prompt if prompt is not None else start).shape[0] * int(n_samples)
            need = self.self_kv8_bytes(R, T)
            if need == 0:
                raise L.DimxError("generate(self_kv8=True): dimx_self_kv8_bytes(%d, %d) = 0 (shape or variant not supported)" % (R, T))
            if self.self_kv8_buffer() is None or self._skv8.numel() < need:
                self._skv8 = None
                self._skv8 = torch.zeros(need, dtype=torch.uint8, device=self.device)
            self.set_self_kv8(self._skv8)
            try:
                return self.generate(start, mask_u8, T, temperature, top_k, noise, seed, return_logits, n_samples, prompt, prompt_len,
                                     prefill, no_prefill, filter_logits_fn, filter_kwargs, return_scores, lookahead, guidance,
                                     return_branches, kv8)
            finally:
                self.set_self_kv8(None)
        if kv8:
            B = (prompt if prompt is not None else start).shape[0]
            need = self.cross_kv8_bytes(B, T)
            if need == 0:
                raise L.DimxError("generate(kv8=True): dimx_cross_kv8_bytes(%d, %d) = 0 (shape or variant not supported)" % (B, T))
            if self.cross_kv8_buffer() is None or self._kv8.numel() < need:
                self._kv8 = None
                self._kv8 = torch.zeros(need, dtype=torch.uint8, device=self.device)
            self.set_cross_kv8(self._kv8)
            try:
                return self.generate(start, mask_u8, T, temperature, top_k, noise, seed, return_logits, n_samples, prompt, prompt_len,
                                     prefill, no_prefill, filter_logits_fn, filter_kwargs, return_scores, lookahead, guidance,
                                     return_branches)
            finally:
                self.set_cross_kv8(None)
        if lookahead is not None:
            prev = self.cross_lookahead()
            self.set_cross_lookahead(lookahead)
            try:
                return self.generate(start, mask_u8, T, temperature, top_k, noise, seed, return_logits, n_samples, prompt, prompt_len,
                                     prefill, no_prefill, filter_logits_fn, filter_kwargs, return_scores, None, guidance, return_branches)
            finally:
                self.set_cross_lookahead(prev)
        if filter_logits_fn is not None or filter_kwargs:
            kind, top_k, fa, fb = sampling.resolve(filter_logits_fn, filter_kwargs, top_k)
            if kind != 0:
                self.set_sampler_filter(kind, fa, fb)
                try:
                    return self.generate(start, mask_u8, T, temperature, top_k, noise, seed, return_logits, n_samples, prompt,
                                         prompt_len, prefill, no_prefill, return_scores=return_scores, guidance=guidance,
                                         return_branches=return_branches)
                finally:
                    self.set_sampler_filter(0)
        if guidance is not None:
            return self._generate_guided(float(guidance), start, prompt, prompt_len, mask_u8, T, temperature, top_k, noise, seed,
                                         return_logits, n_samples, return_scores, return_branches)
        if return_branches:
            raise ValueError("return_branches needs guidance=")
        if prompt is not None:
            return self._generate_prompted(prompt, prompt_len, prefill, no_prefill, mask_u8, T, temperature, top_k, noise, seed,
                                           return_logits, n_samples, return_scores)
        B = start.shape[0]
        R = B * n_samples
        start = start.to(torch.int32).contiguous()
        if noise is not None:
            noise = noise.to(torch.float32).contiguous()
            assert tuple(noise.shape) == (self.n_gen(T), R, self.dims.num_tokens)
        self._chk(start, mask_u8, noise)
        n = self.n_gen(T)
        tokens = torch.empty(R, n, dtype=torch.int32, device=self.device)
        lg = torch.empty(R, n, self.dims.num_tokens, dtype=torch.float32, device=self.device) \
            if (return_logits or return_scores) else None
        ws, wsb = self.workspace(B, T, n_samples)
        L.check(self.lib.dimx_generate(self.h, L.ptr(start), L.ptr(mask_u8), B, T, int(n_samples), float(temperature),
                                       int(top_k),
                                       L.ptr(noise), int(seed) & 0xFFFFFFFFFFFFFFFF, L.ptr(tokens), L.ptr(lg), ws,
                                       wsb, self._s()), "dimx_generate")
        return self._generated(tokens, lg, mask_u8, T, n_samples, None, return_logits, return_scores)

    def stream(self, B, Tmax, start, lookahead=0, temperature=1.0, top_k=52, noise=None, seed=0, prompt=None, v_speaker=None,
               v_audio=None, kv8=False, self_kv8=False):
        """Open a streaming session (dimx_stream_begin, include/dimx.h): B clips in lockstep, at most ``Tmax`` frames,
        ``start`` [B] the listener's first codes, the sampler's arguments as ``generate`` takes them (``noise`` [Tmax-1, B, 512]).
        Returns a StreamSession with a workspace of its own; one session per engine at a time.

        ``prompt`` [B, P] with ``v_speaker`` [B, F, 56] and ``v_audio`` [B, F, 768] (``start`` is then ignored and may be None): the
        session starts from its first P codes and F frames (dimx_stream_begin_prompted; ``dimx.stream.prompt_fits``).

        ``kv8`` / ``self_kv8``: FP8 cross / self K/V for the session (dimx_stream_set_kv8; dimx.kv8 append, self_step):
        the session allocates and owns the buffers, every push quantises the cross rows it appends, and the steps read codes."""
        return StreamSession(self, B, Tmax, start, lookahead, temperature, top_k, noise, seed, prompt, v_speaker, v_audio, kv8, self_kv8)

    def stream_set_kv8(self, cross_buf=None, self_buf=None):
        """The FP8 buffers the next session begins take (dimx_stream_set_kv8): uint8 device tensors or None (that route off)."""
        self._chk(cross_buf, self_buf)
        L.check(self.lib.dimx_stream_set_kv8(self.h, L.ptr(cross_buf), cross_buf.numel() if cross_buf is not None else 0, L.ptr(self_buf),
                                             self_buf.numel() if self_buf is not None else 0), "dimx_stream_set_kv8")

    def stream_kv8(self):
        """((cross pointer, bytes) or None, (self pointer, bytes) or None): the handle's setting (dimx_stream_kv8)."""
        cp, cn, sp, sn = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_void_p(), ctypes.c_size_t()
        L.check(self.lib.dimx_stream_kv8(self.h, ctypes.byref(cp), ctypes.byref(cn), ctypes.byref(sp), ctypes.byref(sn)), "dimx_stream_kv8")
        return ((cp.value, cn.value) if cp.value else None, (sp.value, sn.value) if sp.value else None)

    def _generated(self, tokens, lg, mask_u8, T, n_samples, plen, return_logits, return_scores):
        """generate()'s return value: tokens[, logits][, SeqScores of the sampled columns (``plen``: effective prompt lengths)]"""
        out = (tokens, lg) if return_logits else (tokens,)
        if return_scores:
            from .scoring import scored_columns
            first, last = scored_columns(T, tokens.shape[1], mask_u8.sum(1, dtype=torch.int32), plen)
            out += (op_seq_logprob(lg, tokens, first, last, rows_per_clip=n_samples),)
        return out if len(out) > 1 else out[0]

    def _generate_guided(self, scale, start, prompt, prompt_len, mask_u8, T, temperature, top_k, noise, seed, return_logits, n_samples,
                         return_scores, return_branches):
        if n_samples != 1:
            raise L.DimxError("generate(guidance=): one sample per clip (n_samples = %d)" % n_samples)
        if prompt is None:
            prompt = start.reshape(-1, 1)
        B, Pmax = prompt.shape
        prompt = prompt.to(torch.int32).contiguous()
        prompt_len = prompt_len.to(torch.int32).contiguous() if prompt_len is not None else None
        n, V = self.n_gen(T), self.dims.num_tokens
        if noise is not None:
            noise = noise.to(torch.float32).contiguous()
            assert tuple(noise.shape) == (n, B, V)
        self._chk(prompt, prompt_len, mask_u8, noise)
        tokens = torch.empty(B, n, dtype=torch.int32, device=self.device)
        lg = torch.empty(B, n, V, dtype=torch.float32, device=self.device) if (return_logits or return_scores) else None
        br = torch.empty(2, B, n, V, dtype=torch.float32, device=self.device) if return_branches else None
        # the workspace the context was built in (guided=True), never grown here: that would drop the context
        ws, wsb = self.workspace(B, T, 1)
        L.check(self.lib.dimx_generate_guided(self.h, L.ptr(prompt), int(prompt.stride(0)), L.ptr(prompt_len), int(Pmax), L.ptr(mask_u8), B, T,
                                              scale, float(temperature), int(top_k), L.ptr(noise), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                              L.ptr(tokens), L.ptr(lg), L.ptr(br), ws, wsb, self._s()), "dimx_generate_guided")
        plen = None
        if return_scores and Pmax > 1:
            plen = prompt_len.clamp(1, Pmax) if prompt_len is not None else torch.full((B,), Pmax, dtype=torch.int32, device=self.device)
        out = self._generated(tokens, lg, mask_u8, T, 1, plen, return_logits, return_scores)
        if return_branches:
            out = (out if isinstance(out, tuple) else (out,)) + (br,)
        return out

    def _generate_prompted(self, prompt, prompt_len, prefill, no_prefill, mask_u8, T, temperature, top_k, noise, seed,
                           return_logits, n_samples, return_scores=False):
        B, Pmax = prompt.shape
        R = B * n_samples
        prompt = prompt.to(torch.int32).contiguous()
        prompt_len = prompt_len.to(torch.int32).contiguous() if prompt_len is not None else None
        window = False
        if isinstance(prefill, str) or isinstance(prefill, tuple):
            kind, prefill = (prefill, None) if isinstance(prefill, str) else prefill
            if kind != "window":
                raise ValueError("prefill=%r: an integer P0, 'window' or ('window', P0)" % (kind,))
            window = True
        P0 = int(prefill) if prefill is not None else (Pmax if prompt_len is None else 1)
        if noise is not None:
            noise = noise.to(torch.float32).contiguous()
            assert tuple(noise.shape) == (self.n_gen(T), R, self.dims.num_tokens)
        self._chk(prompt, prompt_len, mask_u8, noise)
        n = self.n_gen(T)
        tokens = torch.empty(R, n, dtype=torch.int32, device=self.device)
        lg = torch.empty(R, n, self.dims.num_tokens, dtype=torch.float32, device=self.device) if (return_logits or return_scores) else None
        # the workspace the context was built in, never grown here (that would drop the context): the library refuses a
        # prefill it is too small for (DIMX_ERR_WORKSPACE, before any launch) -- build the context with prompt_frames >= prefill
        ws, wsb = self.workspace(B, T, n_samples)
        L.check(self.lib.dimx_generate_prompted(self.h, L.ptr(prompt), int(prompt.stride(0)), L.ptr(prompt_len), int(Pmax), P0,
                                                L.ptr(mask_u8), B, T, int(n_samples), float(temperature), int(top_k), L.ptr(noise),
                                                int(seed) & 0xFFFFFFFFFFFFFFFF, L.ptr(tokens), L.ptr(lg),
                                                (1 if no_prefill else 0) | (2 if window else 0), ws, wsb, self._s()), "dimx_generate_prompted")
        plen = None
        if return_scores:    # the library's clamp (include/dimx.h): prompt_len into [P0, Pmax] (no prefill: P0 = 1), no prompt_len = Pmax
            no_prefill = no_prefill or (self.cross_lookahead() is not None and not window)
            plen = prompt_len.clamp(1 if no_prefill else P0, Pmax) if prompt_len is not None \
                else torch.full((B,), Pmax, dtype=torch.int32, device=self.device)
        return self._generated(tokens, lg, mask_u8, T, n_samples, plen, return_logits, return_scores)

    def generate_beam(self, start, mask_u8, T, beam_width, prompt=None, prompt_len=None, prefill=None, return_logits=False,
                      return_backptr=False, beam_kv8=None):
        """Beam search (dimx_generate_beam, csrc/beam.hip; the definition is dimx.beam): W = ``beam_width`` hypotheses per clip in
        one pass (rows b*W + w, sharing the clip's context K/V like ``n_samples``), deterministic, no temperature / filter / seed.
        -> (tokens [B*W, n] int32 -- whole hypotheses, row b*W the best --, scores f64 [B*W], descending within a clip[, logits
        [B*W, n, 512] in the row order each step ran in][, backptr [B*W, n] int32: the row that ran step c on the hypothesis's path]).
        The scored columns are those of dimx.scoring.scored_columns (inside the clip's length, past its prompt); the lengths come
        from ``mask_u8`` on the device.  ``prompt`` / ``prompt_len`` / ``prefill`` as in ``generate``; the context must have been
        built with ``n_samples=beam_width`` (and ``prompt_frames >= prefill``).

        ``beam_kv8``: None (today's call), "self", "cross" or True (both): the search runs on FP8 self caches and / or an FP8 copy
        of the cross K/V (``set_beam_kv8``; dimx.kv8.reorder, self_step, attention_rows).  The engine allocates (or
        reuses) the buffers ``generate(self_kv8=, kv8_samples=)`` use -- ``self_kv8_bytes(B * W, T)`` / ``cross_kv8_bytes(B, T)`` --
        sets them and the switch for the call and clears all three afterwards; ``self_kv8_layers(B * W, T)`` / ``cross_kv8_layers(B, T)``
        view what the search left."""
        W = int(beam_width)
        if beam_kv8 is not None and beam_kv8 is not False:
            beam_kv8 = True if beam_kv8 == "both" else beam_kv8     # the command-line spelling of True
            if beam_kv8 not in (True, "self", "cross"):
                raise ValueError("beam_kv8=%r: one of None, 'self', 'cross', True" % (beam_kv8,))
            B = (prompt if prompt is not None else start).shape[0]
            if beam_kv8 in (True, "self"):
                need = self.self_kv8_bytes(B * W, T)
                if need == 0:
                    raise L.DimxError("generate_beam(beam_kv8=%r): dimx_self_kv8_bytes(%d, %d) = 0 (shape or variant not supported)"
                                      % (beam_kv8, B * W, T))
                if self.self_kv8_buffer() is None or self._skv8.numel() < need:
                    self._skv8 = None
                    self._skv8 = torch.zeros(need, dtype=torch.uint8, device=self.device)
            if beam_kv8 in (True, "cross"):
                need = self.cross_kv8_bytes(B, T)
                if need == 0:
                    raise L.DimxError("generate_beam(beam_kv8=%r): dimx_cross_kv8_bytes(%d, %d) = 0 (shape or variant not supported)"
                                      % (beam_kv8, B, T))
                if self.cross_kv8_buffer() is None or self._kv8.numel() < need:
                    self._kv8 = None
                    self._kv8 = torch.zeros(need, dtype=torch.uint8, device=self.device)
            try:
                if beam_kv8 in (True, "self"):
                    self.set_self_kv8(self._skv8)
                if beam_kv8 in (True, "cross"):
                    self.set_cross_kv8(self._kv8)
                self.set_beam_kv8(True)
                return self.generate_beam(start, mask_u8, T, W, prompt, prompt_len, prefill, return_logits, return_backptr)
            finally:
                self.set_beam_kv8(False)
                self.set_self_kv8(None)
                self.set_cross_kv8(None)
        if prompt is None:
            prompt, prompt_len, prefill = start.reshape(-1, 1), None, 1
        B, Pmax = prompt.shape
        R = B * W
        prompt = prompt.to(torch.int32).contiguous()
        prompt_len = prompt_len.to(torch.int32).contiguous() if prompt_len is not None else None
        P0 = int(prefill) if prefill is not None else (Pmax if prompt_len is None else 1)
        lens = mask_u8.sum(1, dtype=torch.int32)
        self._chk(prompt, prompt_len, mask_u8)
        n = self.n_gen(T)
        tokens = torch.empty(R, n, dtype=torch.int32, device=self.device)
        scores = torch.empty(R, dtype=torch.float64, device=self.device)
        lg = torch.empty(R, n, self.dims.num_tokens, dtype=torch.float32, device=self.device) if return_logits else None
        bp = torch.empty(R, n, dtype=torch.int32, device=self.device) if return_backptr else None
        state = torch.empty(2 * R, dtype=torch.float64, device=self.device)    # DIMX_BEAM_STATE_BYTES = 16 * B * W
        ws, wsb = self.workspace(B, T, W)   # the workspace the context was built in, never grown here (see _generate_prompted)
        L.check(self.lib.dimx_generate_beam(self.h, L.ptr(prompt), int(prompt.stride(0)), L.ptr(prompt_len), int(Pmax), P0,
                                            L.ptr(mask_u8), L.ptr(lens), B, T, W, L.ptr(tokens), L.ptr(scores), L.ptr(bp), L.ptr(lg),
                                            L.ptr(state), state.numel() * 8, 0, ws, wsb, self._s()), "dimx_generate_beam")
        return (tokens, scores) + ((lg,) if return_logits else ()) + ((bp,) if return_backptr else ())

    def mesh_head(self, motion, template=None, safe=False, out=None):
        """EmocaConverter head: motion [B,L,56] -> mesh [B,L,V] = vertice_map_reverse(vertice_map_reverse_lstm(motion)) +
        template[:, None] (template [B,V] or None).  ``safe``: the LSTM layers on the no-communication path.  ``out``: a
        preallocated [B,L,V] f32 tensor to write into."""
        B, Lq, _ = motion.shape
        V = self.dims.mesh_dim
        motion = motion.to(torch.float32).contiguous()
        template = template.to(torch.float32).contiguous() if template is not None else None
        if template is not None:
            assert tuple(template.shape) == (B, V), "template must be [B, mesh_dim]"
        if out is None:
            out = torch.empty(B, Lq, V, dtype=torch.float32, device=self.device)
        assert tuple(out.shape) == (B, Lq, V) and out.dtype == torch.float32
        self._chk(motion, template, out)
        ws, wsb = self.workspace(B, Lq)
        L.check(self.lib.dimx_mesh_head(self.h, L.ptr(motion), L.ptr(template), B, Lq, L.ptr(out), 1 if safe else 0, ws, wsb,
                                        self._s()), "dimx_mesh_head")
        return out

    def lstm_faults(self):
        """LSTM layers of this handle whose group kernel reported a fault and that were rerun on the safe path."""
        return int(self.lib.dimx_lstm_faults(self.h))

    def chain_faults(self):
        """generate() calls of this handle whose XCD-local chain kernels reported a placement / barrier fault; each was
        regenerated on the one-kernel-per-op step before generate() returned (0 = never happened)."""
        return int(self.lib.dimx_chain_faults(self.h))

    def qkv0_table_builds(self):
        """how often this handle built the first decoder layer's q/k/v table (once per rows-per-call, numeric mode and set
        of decoder weights; 0 = generate() projects q/k/v at every step)."""
        return int(self.lib.dimx_qkv0_table_builds(self.h))

    def kv0_table_generations(self):
        """how many generations of this handle read the first decoder layer's self-attention K/V from the token table
        instead of that layer's cache (0 = the cache: beam search, a prompt, no q/k/v table, or DIMX_NO_KV0_TABLE=1)."""
        return int(self.lib.dimx_kv0_table_generations(self.h))

    def sample_head_generations(self):
        """how many generations of this handle sampled inside the first decoder layer's launch instead of a sampler launch
        per step (0 = the sampler launch: any route but the bf16 layer-kernel one with the token table and the top-k
        filter, or DIMX_NO_SAMPLE_HEAD=1)."""
        return int(self.lib.dimx_sample_head_generations(self.h))

    def debug_chain_fault(self, n_calls=1):
        """test hook: the next n_calls generate() calls run their chain kernels on a non-bijective placement."""
        L.check(self.lib.dimx_debug_chain_fault(self.h, int(n_calls)), "dimx_debug_chain_fault")


# ---------------------------------------------------------------------- kernel-level wrappers (tests)
class StreamSession:
    """One streaming session of an Engine (Engine.stream): push speaker frames in pieces, receive the listener tokens that are due.
    A context manager; ``close()`` aborts a session that is still open.  ``tokens`` are all tokens so far [B, steps].  After
    ``end`` or ``close`` the object may ``begin`` another clip in the same workspace."""

    def __init__(self, eng, B, Tmax, start, lookahead=0, temperature=1.0, top_k=52, noise=None, seed=0, prompt=None, v_speaker=None,
                 v_audio=None, kv8=False, self_kv8=False):
        self.eng, self.B, self.Tmax, self.lookahead = eng, int(B), int(Tmax), int(lookahead)
        self._open = False
        lib, dev = eng.lib, eng.device
        need = lib.dimx_stream_workspace_bytes(eng.h, self.B, self.Tmax)
        if need == 0:
            raise L.DimxError("dimx_stream_workspace_bytes(%d,%d) = 0: sessions need the SLMFT variant and 2 <= Tmax <= 2048" % (B, Tmax))
        self._ws = torch.empty(need + 256, dtype=torch.uint8, device=dev)   # the library needs no initialised workspace
        self._V = eng.dims.num_tokens
        self._tok = torch.zeros(self.B, self.Tmax - 1, dtype=torch.int32, device=dev)
        self._lg = None
        # FP8 K/V (dimx_stream_set_kv8): the session owns its buffers, sets them before every begin and clears the setting when it closes
        self._kv8 = self._skv8 = None
        if kv8 or self_kv8:
            need8 = eng.cross_kv8_bytes(self.B, self.Tmax)
            if need8 == 0:
                raise L.DimxError("stream(kv8=/self_kv8=): dimx_cross_kv8_bytes(%d, %d) = 0 (shape or variant not supported)" % (B, Tmax))
            if kv8:
                self._kv8 = torch.zeros(need8, dtype=torch.uint8, device=dev)
            if self_kv8:
                self._skv8 = torch.zeros(eng.self_kv8_bytes(self.B, self.Tmax), dtype=torch.uint8, device=dev)
        self._ckv = None
        self.begin(start, temperature, top_k, noise, seed, prompt, v_speaker, v_audio)

    def _ws_ptr(self):
        base = self._ws.data_ptr()
        aligned = (base + 255) // 256 * 256
        return ctypes.c_void_p(aligned), self._ws.numel() - (aligned - base)

    def _fp8(self):
        return self._kv8 is not None or self._skv8 is not None

    def _begun(self, call, what):
        """one begin call between setting the session's FP8 buffers and noting where its plain cross K/V caches lie"""
        if self._fp8():
            self.eng.stream_set_kv8(self._kv8, self._skv8)
        try:
            L.check(call(), what)
        except Exception:
            self._clear_kv8()
            raise
        k, v = ctypes.c_void_p(), ctypes.c_void_p()
        self._ckv = []
        for l in range(self.eng.dims.dec_depth):
            L.check(self.eng.lib.dimx_stream_cross_kv(self.eng.h, l, ctypes.byref(k), ctypes.byref(v)), "dimx_stream_cross_kv")
            self._ckv.append((k.value - self._ws.data_ptr(), v.value - self._ws.data_ptr()))

    def _clear_kv8(self):
        if self._fp8() and getattr(self.eng, "h", None):
            self.eng.lib.dimx_stream_set_kv8(self.eng.h, None, 0, None, 0)

    def cross_kv_layers(self):
        """Per decoder layer (K, V [B, H, Tp, 64] in the engine's operand type): views of the session's plain cross K/V caches in its
        workspace.  Rows below the frames pushed hold the context rows' projections; they stay after ``end`` until the next begin."""
        H, Tp = self.eng.dims.heads, (self.Tmax + 7) // 8 * 8
        dt = torch.bfloat16 if self.eng.mode == L.MODE_PERF_BF16 else torch.float32
        nb = self.B * H * Tp * 64 * (2 if dt == torch.bfloat16 else 4)
        return [tuple(self._ws[o:o + nb].view(dt).view(self.B, H, Tp, 64) for o in kv) for kv in self._ckv]

    def cross_kv8_layers(self):
        """Per decoder layer (kcodes, vcodes, kscale, vscale): views of the session's FP8 cross buffer (Engine.cross_kv8_layers)."""
        return self.eng.cross_kv8_layers(self.B, self.Tmax, self._kv8)

    def self_kv8_layers(self):
        """... and of its FP8 self buffer; positions the session did not reach hold what the buffer held before."""
        return self.eng.cross_kv8_layers(self.B, self.Tmax, self._skv8)

    def begin(self, start=None, temperature=1.0, top_k=52, noise=None, seed=0, prompt=None, v_speaker=None, v_audio=None):
        """Start (another) clip: the arguments of Engine.stream; B, Tmax and the look-ahead are the session's."""
        if self._open:
            raise L.DimxError("StreamSession.begin: the session is open (end() or close() first)")
        if noise is not None:
            noise = noise.to(torch.float32).contiguous()
            assert tuple(noise.shape) == (self.Tmax - 1, self.B, self._V)
        if prompt is not None:
            return self._begin_prompted(prompt, v_speaker, v_audio, temperature, top_k, noise, seed)
        start = start.to(torch.int32).contiguous()
        self.eng._chk(start, noise)
        assert tuple(start.shape) == (self.B,)
        self._noise = noise    # the session reads it at every step
        self._last = (0, 0)    # token columns the last push (or end) emitted
        ws, wsb = self._ws_ptr()
        self._begun(lambda: self.eng.lib.dimx_stream_begin(self.eng.h, L.ptr(start), self.B, self.Tmax, self.lookahead, float(temperature),
                                                           int(top_k), L.ptr(self._noise), int(seed) & 0xFFFFFFFFFFFFFFFF, ws, wsb,
                                                           self.eng._s()), "dimx_stream_begin")
        self._open = True
        self.frames = 0
        self.steps = 0

    def _begin_prompted(self, prompt, v_speaker, v_audio, temperature, top_k, noise, seed):
        """The first P codes and F frames are given: encoder increments and K / V append of the frames, one windowed prefill of the
        positions 0 .. P - 2, the step counter at P - 1.  Token columns below P - 1 repeat the prompt, their logits read zero; the
        steps the F frames make due beyond P - 1 run with the next push (or ``end``)."""
        from . import stream as _stream
        prompt = prompt.to(torch.int32).contiguous()
        v_speaker = v_speaker.to(torch.float32).contiguous()
        v_audio = v_audio.to(torch.float32).contiguous()
        self.eng._chk(prompt, v_speaker, v_audio, noise)
        B, P = prompt.shape
        F = v_speaker.shape[1]
        assert B == self.B and v_speaker.shape[0] == B and tuple(v_audio.shape[:2]) == (B, F)
        if not _stream.prompt_fits(P, self.lookahead, F, self.Tmax):
            raise ValueError("a session cannot start from P=%d codes and F=%d frames: need 1 <= P and P + max(lookahead, 0) = %d <= F <= Tmax = %d"
                             % (P, F, P + max(self.lookahead, 0), self.Tmax))
        need = self.eng.lib.dimx_stream_workspace_bytes_prompt(self.eng.h, self.B, self.Tmax)
        if self._ws.numel() < need + 256:     # the generate part holds the prefill scratch too
            self._ws = None
            self._ws = torch.empty(need + 256, dtype=torch.uint8, device=self.eng.device)
        self._noise = noise
        ws, wsb = self._ws_ptr()
        self._begun(lambda: self.eng.lib.dimx_stream_begin_prompted(self.eng.h, L.ptr(prompt), P, P, L.ptr(v_speaker), L.ptr(v_audio), F, self.B,
                                                                    self.Tmax, self.lookahead, float(temperature), int(top_k),
                                                                    L.ptr(self._noise), int(seed) & 0xFFFFFFFFFFFFFFFF, ws, wsb,
                                                                    self.eng._s()), "dimx_stream_begin_prompted")
        self._open = True
        self.frames = F
        self.steps = P - 1
        self._last = (P - 1, P - 1)
        self._tok[:, :P - 1] = prompt[:, 1:]
        if self._lg is not None:
            self._lg[:, :P - 1] = 0

    def _logits(self):
        if self._lg is None:
            self._lg = torch.zeros(self.B, self.Tmax - 1, self._V, dtype=torch.float32, device=self.eng.device)
        return self._lg

    def _took(self, n_new, return_logits, extra=()):
        lo, hi = self.steps, self.steps + n_new
        self.steps = hi
        self._last = (lo, hi)
        out = (self._tok[:, lo:hi],)
        if return_logits:
            out += (self._lg[:, lo:hi],)
        out += tuple(extra)
        return out if len(out) > 1 else out[0]

    def push(self, v_speaker, v_audio, return_logits=False, return_x_s=False):
        """v_speaker [B, c, 56], v_audio [B, c, 768]: the next c >= 1 frames of every clip -> the new tokens [B, n_new] (views of
        the session's token rows)[, their logits [B, n_new, 512]][, the c new encoder rows x_s [B, c, 384]]."""
        if not self._open:
            raise L.DimxError("StreamSession.push: the session is closed")
        B, c, _ = v_speaker.shape
        v_speaker = v_speaker.to(torch.float32).contiguous()
        v_audio = v_audio.to(torch.float32).contiguous()
        self.eng._chk(v_speaker, v_audio)
        assert B == self.B and v_audio.shape[:2] == (B, c)
        x_s = torch.empty(B, c, self.eng.dims.dim, dtype=torch.float32, device=self.eng.device) if return_x_s else None
        lg = self._logits() if return_logits else None
        n_new = ctypes.c_int(0)
        L.check(self.eng.lib.dimx_stream_push(self.eng.h, L.ptr(v_speaker), L.ptr(v_audio), c, L.ptr(self._tok), self.Tmax - 1, L.ptr(lg),
                                              L.ptr(x_s), ctypes.byref(n_new), self.eng._s()), "dimx_stream_push")
        self.frames += c
        return self._took(n_new.value, return_logits, (x_s,) if return_x_s else ())

    def end(self, return_logits=False):
        """The clip is over: T = the frames pushed.  Runs the remaining steps, returns their tokens and closes the session."""
        if not self._open:
            raise L.DimxError("StreamSession.end: the session is closed")
        lg = self._logits() if return_logits else None
        n_new = ctypes.c_int(0)
        L.check(self.eng.lib.dimx_stream_end(self.eng.h, L.ptr(self._tok), self.Tmax - 1, L.ptr(lg), ctypes.byref(n_new), self.eng._s()),
                "dimx_stream_end")
        self._open = False
        self._clear_kv8()
        return self._took(n_new.value, return_logits)

    @property
    def tokens(self):
        return self._tok[:, :self.steps]

    @property
    def is_open(self):
        return self._open

    def state(self):
        """(frames, steps, open) as the library holds them (dimx_stream_state)."""
        f, s, o = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        L.check(self.eng.lib.dimx_stream_state(self.eng.h, ctypes.byref(f), ctypes.byref(s), ctypes.byref(o)), "dimx_stream_state")
        return f.value, s.value, bool(o.value)

    def set_events(self, events):
        """Measurement: four recorded ``torch.cuda.Event(enable_timing=True)`` (or None to stop) that every later push records at
        its start, after the encoder increment, after the cross K/V append and after the decode steps (dimx_stream_set_events)."""
        self._events = events      # kept alive: the library holds their handles
        hs = [ctypes.c_void_p(e.cuda_event) for e in events] if events else [None] * 4
        L.check(self.eng.lib.dimx_stream_set_events(self.eng.h, *hs), "dimx_stream_set_events")

    def motion(self, window=None, all_rows=False):
        """Chunked VQ decode: ``Engine.vq_decode(1, tokens[:, lo:hi])`` with hi = the tokens so far and lo = hi - ``window`` (0 for
        None), positions restarting at the slice; returns the rows [B, n_new, 56] of the tokens the last push (or ``end``) emitted
        -- the slice is widened to hold them all -- or, with ``all_rows``, every row of the slice.  A windowed decode is another
        function of the tokens than the whole-clip decode, and nothing was trained for it; after ``end``,
        ``motion(None, all_rows=True)`` is the whole-clip decode."""
        lo_new, hi = self._last
        lo = 0 if window is None else max(hi - int(window), 0)
        lo = min(lo, lo_new)
        if hi == lo or (hi == lo_new and not all_rows):
            return torch.empty(self.B, 0, self.eng.dims.vq_in_dim, dtype=torch.float32, device=self.eng.device)
        out = self.eng.vq_decode(1, self._tok[:, lo:hi].contiguous())
        return out if all_rows else out[:, lo_new - lo:]

    def close(self):
        if self._open and getattr(self.eng, "h", None):
            self.eng.lib.dimx_stream_abort(self.eng.h)
            self._clear_kv8()
        self._open = False

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _pad_k(w, mult):
    N, K = w.shape
    Kp = (K + mult - 1) // mult * mult
    if Kp == K:
        return w.contiguous()
    out = torch.zeros(N, Kp, dtype=w.dtype, device=w.device)
    out[:, :K] = w
    return out


def tile_weight(w_, bk):
    """[N, Kp] -> blocks of 8 rows x bk elements (128 B), block (n // 8, k // bk) contiguous: the layout the decode-step
    GEMM reads with one contiguous KiB per LDS-DMA piece (GemmArgs.w_tiled)."""
    N, Kp = w_.shape
    assert N % 8 == 0 and Kp % bk == 0
    return w_.view(N // 8, 8, Kp // bk, bk).permute(0, 2, 1, 3).contiguous().view(N, Kp)


def op_split_x3(w):
    """f32 [..] -> the three bf16 planes [3, ..] whose sum is ``w`` exactly (csrc/gemm_x3.hip split_x3_kernel)."""
    lib = L.load()
    w_ = w.float().contiguous()
    planes = torch.empty((3,) + tuple(w_.shape), dtype=torch.bfloat16, device=w.device)
    L.check(lib.dimx_op_split_x3(L.ptr(w_), L.ptr(planes), w_.numel(), L.stream_ptr(w.device)), "dimx_op_split_x3")
    return planes


def op_gemm_x3(a, w, bias=None, act=0, residual=None, slabs=False, planes=None):
    """The f32 parity mode's split-bf16 decode GEMM (csrc/gemm_x3.hip): epilogue(a[M,K] @ w[N,K]^T), f32 in and out,
    K % 32 == 0.  ``slabs``: the split-K partial sums [splits, M, N] as the decode step's consumers get them (the kernel plans
    the count from (N, K)).  ``planes``: the pre-split weight (op_split_x3), as the model keeps it."""
    lib = L.load()
    a_ = a.float().contiguous()
    if planes is None:
        planes = op_split_x3(w)
    (M, K), N = a_.shape, planes.shape[1]
    flags = 4 if slabs else 0
    ns = lib.dimx_op_gemm_slabs(L.F32, M, N, K, 16 | 5) if slabs else 0
    out = torch.full((ns, M, N) if slabs else (M, N), float("nan"), dtype=torch.float32, device=a.device)
    L.check(lib.dimx_op_gemm_x3(L.ptr(a_), K, L.ptr(planes), L.ptr(out), N, M, N, K, L.ptr(bias), act, L.ptr(residual),
                                residual.shape[1] if residual is not None else 0, flags, L.stream_ptr(a.device)), "dimx_op_gemm_x3")
    return out


def op_gemm(a, w, bias=None, act=0, residual=None, bf16=False, out_bf16=False, conv_T=0, conv_lens=None,
            slabs=0, force_simple=False, cfg=0, w_tiled=False):
    """epilogue(a[M,K] @ w[N,K]^T); conv_T > 0: a is [B*conv_T, C], w is [N, C, 5]."""
    lib = L.load()
    dev = a.device
    if conv_T > 0:
        N, C, _ = w.shape
        wk = w.permute(0, 2, 1).reshape(N, 5 * C)
        K = 5 * C
    else:
        wk, K = w, w.shape[1]
        N = w.shape[0]
    dt = torch.bfloat16 if bf16 else torch.float32
    a_ = a.to(dt).contiguous()
    w_ = _pad_k(wk.to(dt), 64 if bf16 else 32)
    if w_tiled:
        w_ = tile_weight(w_, 64 if bf16 else 32)
    M = a_.shape[0]
    if slabs:   # split-K partial sums as `slabs` f32 slabs [slabs, M, N] (the decode-step projections)
        out = torch.full((slabs, M, N), float("nan"), dtype=torch.float32, device=dev)
    else:
        out = torch.empty(M, N, dtype=torch.bfloat16 if out_bf16 else torch.float32, device=dev)
    flags = (5 if slabs else 0) | (2 if force_simple else 0) | (8 if w_tiled else 0) | (cfg << 8) | (slabs << 16)
    L.check(lib.dimx_op_gemm(L.BF16 if bf16 else L.F32, L.BF16 if out_bf16 else L.F32, L.ptr(a_), a_.shape[1],
                             L.ptr(w_), w_.shape[1], L.ptr(out), N, M, N, K, L.ptr(bias), act, L.ptr(residual),
                             residual.shape[1] if residual is not None else 0, conv_T, L.ptr(conv_lens), flags,
                             L.stream_ptr(dev)), "dimx_op_gemm")
    return out


def _gemm_map_args(a, w, segs, rowT, bias, act, residual, bf16, rowadd, rowadd_mode, rowadd_scale, rowadd_off, rowadd_div,
                   force_simple, cfg):
    """The argument list dimx_op_gemm_map and dimx_op_gemm_route share (without the stream), and the tensors that must stay alive."""
    dt = torch.bfloat16 if bf16 else torch.float32
    a_ = a.to(dt).contiguous()
    w_ = _pad_k(w.to(dt), 64 if bf16 else 32)
    (M, K), N = a.shape, w.shape[0]
    odt = segs[0][0].dtype
    assert odt in (torch.float32, torch.bfloat16) and all(s[0].dtype == odt and s[0].device == a.device for s in segs)
    n = len(segs)
    ptrs = (ctypes.c_void_p * n)(*(s[0].data_ptr() for s in segs))
    strides = (ctypes.c_int64 * (4 * n))(*(int(v) for s in segs for v in s[1:5]))
    heads = (ctypes.c_int32 * n)(*(int(s[5]) for s in segs))
    flags = (2 if force_simple else 0) | (cfg << 8)
    args = [L.BF16 if bf16 else L.F32, L.BF16 if odt == torch.bfloat16 else L.F32, L.ptr(a_), a_.shape[1], L.ptr(w_), w_.shape[1],
            M, N, K, L.ptr(bias), act, L.ptr(residual), residual.shape[1] if residual is not None else 0, rowT, n, ptrs, strides, heads,
            L.ptr(rowadd), rowadd.shape[1] if rowadd is not None else 0, rowadd_mode, float(rowadd_scale), rowadd_off, rowadd_div, flags]
    return args, (a_, w_, ptrs, strides, heads)


def op_gemm_map(a, w, segs, rowT=1, bias=None, act=0, residual=None, bf16=False, rowadd=None, rowadd_mode=0, rowadd_scale=1.0,
                rowadd_off=0, rowadd_div=1, force_simple=False, cfg=0):
    """epilogue(a[M,K] @ w[N,K]^T) scattered through an output map (dimx_op_gemm_map): ``segs`` is a list of 1..3 tuples
    (tensor, sb, sh, st, sd, D) -- the tensor's first element is the segment's base, the strides are in elements -- and row
    m = b * rowT + t, column nn of segment s lands at base + b*sb + t*st + (nn // D)*sh + (nn % D)*sd.  The destinations' dtype is
    the output dtype; they are written in place, nothing is returned."""
    args, keep = _gemm_map_args(a, w, segs, rowT, bias, act, residual, bf16, rowadd, rowadd_mode, rowadd_scale, rowadd_off,
                                rowadd_div, force_simple, cfg)
    L.check(L.load().dimx_op_gemm_map(*args, L.stream_ptr(a.device)), "dimx_op_gemm_map")
    del keep


def op_gemm_route(a, w, segs, **kw):
    """What ``op_gemm_map`` with the same arguments would launch, from the launcher's own decision (dimx_op_gemm_route; nothing
    runs): (kernel, staged, packed) -- kernel = the LDS-DMA cfg id, 256 for the 256 x 256 kernel, 1064 / 1128 for the
    register-staged kernel; staged = the through-LDS epilogue; packed = 4-row packed stores of transposed segments."""
    names = ("rowT", "bias", "act", "residual", "bf16", "rowadd", "rowadd_mode", "rowadd_scale", "rowadd_off", "rowadd_div",
             "force_simple", "cfg")
    defaults = dict(zip(names, (1, None, 0, None, False, None, 0, 1.0, 0, 1, False, 0)))
    assert set(kw) <= set(names), set(kw) - set(names)
    defaults.update(kw)
    args, keep = _gemm_map_args(a, w, segs, *(defaults[k] for k in names))
    word = L.load().dimx_op_gemm_route(*args)
    del keep
    if word < 0:
        L.check(word, "dimx_op_gemm_route")
    return word & 0xffff, bool(word >> 16 & 1), bool(word >> 17 & 1)


def op_lstm_layer(x, w_ih, w_hh, b_ih, b_hh, safe=False, return_faults=False):
    """One bidirectional LSTM layer (csrc/lstm.hip): x [B,T,In] f32; w_ih / w_hh / b_ih / b_hh: pairs (forward, reverse) of
    tensors shaped like torch.nn.LSTM's -> y [B,T,768] f32.  ``safe``: the no-communication path (flags bit 0)."""
    lib = L.load()
    dev = x.device
    B, T, In = x.shape
    H = w_hh[0].shape[1]
    x_ = x.float().contiguous()
    keep = [[t.to(dev, torch.float32).contiguous() for t in pair] for pair in (w_ih, w_hh, b_ih, b_hh)]
    arrs = [(ctypes.c_void_p * 2)(*(t.data_ptr() for t in pair)) for pair in keep]
    y = torch.empty(B, T, 2 * H, dtype=torch.float32, device=dev)
    faults = ctypes.c_int(0)
    L.check(lib.dimx_op_lstm_layer(L.F32, L.ptr(x_), B, T, In, H, arrs[0], arrs[1], arrs[2], arrs[3], L.ptr(y), 1 if safe else 0,
                                   ctypes.byref(faults), L.stream_ptr(dev)), "dimx_op_lstm_layer")
    return (y, faults.value) if return_faults else y


def op_lstm_layer_bwd(x, w_ih, w_hh, b_ih, b_hh, dy, safe=False, need_dx=True, return_faults=False):
    """The adjoint of one bidirectional LSTM layer (csrc/train_lstm.hip): x [B,T,In], dy [B,T,768] f32 and the weight pairs of
    ``op_lstm_layer`` -> (dx [B,T,In] or None, dw_ih pair, dw_hh pair, db pair); db is the gradient of bias_ih and of bias_hh."""
    lib = L.load()
    dev = x.device
    B, T, In = x.shape
    H = w_hh[0].shape[1]
    x_ = x.float().contiguous()
    dy_ = dy.to(dev, torch.float32).contiguous()
    keep = [[t.to(dev, torch.float32).contiguous() for t in pair] for pair in (w_ih, w_hh, b_ih, b_hh)]
    arrs = [(ctypes.c_void_p * 2)(*(t.data_ptr() for t in pair)) for pair in keep]
    outs = [[torch.empty_like(t) for t in keep[i]] for i in (0, 1, 2)]
    oarrs = [(ctypes.c_void_p * 2)(*(t.data_ptr() for t in pair)) for pair in outs]
    dx = torch.empty_like(x_) if need_dx else None
    faults = ctypes.c_int(0)
    L.check(lib.dimx_op_lstm_layer_bwd(L.F32, L.ptr(x_), B, T, In, H, arrs[0], arrs[1], arrs[2], arrs[3], L.ptr(dy_), L.ptr(dx),
                                       oarrs[0], oarrs[1], oarrs[2], 1 if safe else 0, ctypes.byref(faults), L.stream_ptr(dev)),
            "dimx_op_lstm_layer_bwd")
    out = (dx, tuple(outs[0]), tuple(outs[1]), tuple(outs[2]))
    return out + (faults.value,) if return_faults else out


def op_layernorm(x, gamma, beta=None, out_bf16=False):
    lib = L.load()
    M, C = x.shape
    y = torch.empty(M, C, dtype=torch.bfloat16 if out_bf16 else torch.float32, device=x.device)
    L.check(lib.dimx_op_layernorm(L.BF16 if out_bf16 else L.F32, L.ptr(x.contiguous()), L.ptr(y), L.ptr(gamma),
                                  L.ptr(beta), M, C, L.stream_ptr(x.device)), "dimx_op_layernorm")
    return y


def op_instnorm(x, lens=None, out_bf16=False):
    lib = L.load()
    B, T, C = x.shape
    y = torch.empty(B, T, C, dtype=torch.bfloat16 if out_bf16 else torch.float32, device=x.device)
    L.check(lib.dimx_op_instnorm(L.BF16 if out_bf16 else L.F32, L.ptr(x.contiguous()), L.ptr(y), L.ptr(lens), B, T,
                                 C, L.stream_ptr(x.device)), "dimx_op_instnorm")
    return y


ATTN_CANARY = -7.0   # what op_attention(layout=...) leaves where the kernel must not write


def _op_attention_strided(q, k, v, scale, causal, lens, kmask, layout, tp, ld_o, prepacked, kmask_ld, return_buffer):
    """The test entry with every stride given (bf16, row-major v).  Everything the kernel must not read is NaN, everything it must
    not write ATTN_CANARY: packed -- q / k / v [B,L,H*D] followed by eight NaN rows; headmajor -- k / v as the cross-attention
    caches [B,H,tp,D] with rows Lk..tp-1 NaN.  The output buffer is [B, Lq + 2, ld_o]; kmask rows are kmask_ld apart (ones past Lk)."""
    lib = L.load()
    B, Lq, H, D = q.shape
    Lk = k.shape[1]
    dev, bf, nan = q.device, torch.bfloat16, float("nan")
    ld_o = H * D if ld_o is None else ld_o

    def packed(t, n):
        buf = torch.full((B * n + 8, H * D), nan, dtype=bf, device=dev)
        buf[:B * n] = t.to(bf).reshape(B * n, H * D)
        return buf, (n * H * D, H * D, D)

    q_, q_str = packed(q, Lq)
    if layout == "packed":
        (k_, k_str), (v_, v_str) = packed(k, Lk), packed(v, Lk)
    elif layout == "headmajor":
        tp = Lk if tp is None else tp
        assert tp >= Lk
        k_, v_ = (torch.full((B, H, tp, D), nan, dtype=bf, device=dev) for _ in range(2))
        k_[:, :, :Lk] = k.to(bf).permute(0, 2, 1, 3)
        v_[:, :, :Lk] = v.to(bf).permute(0, 2, 1, 3)
        k_str = v_str = (H * tp * D, D, tp * D)
    else:
        raise ValueError("op_attention: layout %r" % (layout,))
    out = torch.full((B, Lq + 2, ld_o), ATTN_CANARY, dtype=bf, device=dev)
    o_str = ((Lq + 2) * ld_o, ld_o, D)
    km = None
    if kmask is not None:
        kmask_ld = Lk if kmask_ld is None else kmask_ld
        km = torch.ones(B, kmask_ld, dtype=torch.uint8, device=dev)
        km[:, :Lk] = kmask
    arr = lambda s: (ctypes.c_long * 3)(*s)
    L.check(lib.dimx_op_attention_strided(L.ptr(q_), L.ptr(k_), L.ptr(v_), L.ptr(out), B, H, Lq, Lk, D, arr(q_str), arr(k_str),
                                          arr(v_str), arr(o_str), float(scale), 1 if causal else 0, L.ptr(lens), L.ptr(km),
                                          kmask_ld if km is not None else 0, 1 if prepacked else 0, L.stream_ptr(dev)),
            "dimx_op_attention_strided")
    res = out[:, :Lq, :H * D].reshape(B, Lq, H, D)
    return (res, out) if return_buffer else res


def op_attention(q, k, v, scale, causal=False, lens=None, kmask=None, bf16=False, row_v=False, layout=None, tp=None, ld_o=None,
                 prepacked=False, kmask_ld=None, return_buffer=False):
    """q [B,Lq,H,D], k/v [B,Lk,H,D] -> [B,Lq,H,D]; v is transposed to [B,H,D,Lk_pad] here, or (row_v, bf16) handed over
    row-major like k.  layout "packed" / "headmajor" (tests): the strided entry of the row-major-v kernel."""
    if layout is not None:
        return _op_attention_strided(q, k, v, scale, causal, lens, kmask, layout, tp, ld_o, prepacked, kmask_ld, return_buffer)
    lib = L.load()
    B, Lq, H, D = q.shape
    Lk = k.shape[1]
    if row_v:
        q_, k_, v_ = (t.to(torch.bfloat16).reshape(B, -1, H * D).contiguous() for t in (q, k, v))
        out = torch.empty(B, Lq, H * D, dtype=torch.bfloat16, device=q.device)
        L.check(lib.dimx_op_attention_rowv(L.ptr(q_), L.ptr(k_), L.ptr(v_), L.ptr(out), B, H, Lq, Lk, D, H * D, H * D, H * D, H * D,
                                           float(scale), 1 if causal else 0, L.ptr(lens), L.ptr(kmask), L.stream_ptr(q.device)),
                "dimx_op_attention_rowv")
        return out.view(B, Lq, H, D)
    dt = torch.bfloat16 if bf16 else torch.float32
    Lp = (Lk + 7) // 8 * 8
    q_ = q.to(dt).reshape(B, Lq, H * D).contiguous()
    k_ = k.to(dt).reshape(B, Lk, H * D).contiguous()
    vt = torch.full((B, H, D, Lp), float("nan"), dtype=dt, device=q.device)   # padding must be ignored
    vt[..., :Lk] = v.to(dt).permute(0, 2, 3, 1)
    out = torch.empty(B, Lq, H * D, dtype=dt, device=q.device)
    L.check(lib.dimx_op_attention(L.BF16 if bf16 else L.F32, L.ptr(q_), L.ptr(k_), L.ptr(vt), L.ptr(out), B, H, Lq,
                                  Lk, D, H * D, H * D, Lp, H * D, float(scale), 1 if causal else 0, L.ptr(lens),
                                  L.ptr(kmask), L.stream_ptr(q.device)), "dimx_op_attention")
    return out.view(B, Lq, H, D)


def op_train_attention(q, k, v, scale, d_o=None, causal=False, kmask=None, kmask2=None, mfma=False, lookahead=None):
    """The training step's attention operator alone: q [B,Lq,H*64], k / v [B,Lk,H*64] f32 -> (o, lse) and, with d_o,
    (o, lse, dq, dk, dv).  mfma: 0 / False = the f32 VALU kernels, 1 / True = the bf16 matrix-core kernels of the perf mode,
    2 = the exact-f32 matrix-core kernels of the parity mode.  lookahead: an integer L puts the online window on (query i keeps
    key j < dimx.online.visible(i, L, Lk); dimx_op_train_attention_win), None leaves it off."""
    lib = L.load()
    B, Lq, C = q.shape
    Lk, H = k.shape[1], C // 64
    f = lambda t: None if t is None else t.float().contiguous()
    u8 = lambda t: None if t is None else t.to(torch.uint8).contiguous()
    q, k, v, d_o, kmask, kmask2 = f(q), f(k), f(v), f(d_o), u8(kmask), u8(kmask2)
    o = torch.empty_like(q)
    lse = torch.empty(B, H, Lq, dtype=torch.float32, device=q.device)
    delta = dq = dk = dv = None
    if d_o is not None:
        delta, dq, dk, dv = torch.empty_like(lse), torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    if lookahead is None:
        L.check(lib.dimx_op_train_attention(int(mfma), L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(d_o), L.ptr(kmask), L.ptr(kmask2),
                                            B, H, Lq, Lk, 1 if causal else 0, float(scale), L.ptr(o), L.ptr(lse), L.ptr(delta),
                                            L.ptr(dq), L.ptr(dk), L.ptr(dv), L.stream_ptr(q.device)), "dimx_op_train_attention")
    else:
        L.check(lib.dimx_op_train_attention_win(int(mfma), L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(d_o), L.ptr(kmask), L.ptr(kmask2),
                                                B, H, Lq, Lk, 1 if causal else 0, float(scale), 1, int(lookahead), L.ptr(o),
                                                L.ptr(lse), L.ptr(delta), L.ptr(dq), L.ptr(dk), L.ptr(dv),
                                                L.stream_ptr(q.device)), "dimx_op_train_attention_win")
    return (o, lse) if d_o is None else (o, lse, dq, dk, dv)


def _nan(shape, device, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=device)


def op_train_layernorm_bwd(x, gamma, dy, dx=None, with_beta=True):
    """The training step's LayerNorm adjoint alone (ln_adjoint -> tr_layernorm_bwd_fused + tr_multi_finish): x, dy [M,C] f32,
    gamma [C] -> (dx, d gamma, d beta or None).  ``dx`` given: the adjoint is ADDED to it in place (the residual stream's
    accumulate form).  Outputs start as NaN, so an element the kernels leave unwritten shows."""
    lib = L.load()
    M, C = x.shape
    dev = x.device
    x, gamma, dy = x.float().contiguous(), gamma.float().contiguous(), dy.float().contiguous()
    accumulate = dx is not None
    if dx is None:
        dx = _nan((M, C), dev)
    dg = _nan((C,), dev)
    db = _nan((C,), dev) if with_beta else None
    scratch = _nan((2 * (600 * C + 64),), dev)
    L.check(lib.dimx_op_train_layernorm_bwd(L.ptr(x), L.ptr(gamma), L.ptr(dy), L.ptr(dx), 1 if accumulate else 0, M, C, L.ptr(dg),
                                            L.ptr(db), L.ptr(scratch), scratch.numel(), L.stream_ptr(dev)),
            "dimx_op_train_layernorm_bwd")
    return dx, dg, db


def op_train_colsum(dy):
    """Column sums of dy [M,C] f32 as the training step forms a bias gradient (bias_adjoint -> tr_colsum_partial +
    tr_multi_finish) -> [C]."""
    lib = L.load()
    M, C = dy.shape
    dy = dy.float().contiguous()
    out = _nan((C,), dy.device)
    scratch = _nan((32 * C + 64,), dy.device)
    L.check(lib.dimx_op_train_colsum(L.ptr(dy), M, C, L.ptr(out), L.ptr(scratch), scratch.numel(), L.stream_ptr(dy.device)),
            "dimx_op_train_colsum")
    return out


def op_train_prep(src, mode=0, bf16=False, src2=None, gamma=None, beta=None, colpart=False):
    """The operand copy in front of every training GEMM (tr_prep_fused): src [rows,cols] f32, last dimension contiguous, any row
    stride (a column slice of a wider buffer is passed as it lies) -> (o [rows,Kp], t [cols,Mp], colpart [n_part,cols] or None) in
    the operand type; Kp / Mp are cols / rows padded to its k-tile.  Modes as in include/dimx.h.  Outputs start as NaN."""
    lib = L.load()
    assert src.dtype == torch.float32 and src.dim() == 2 and src.stride(1) == 1
    assert src2 is None or (src2.dtype == torch.float32 and src2.stride(1) == 1 and src2.shape == src.shape)
    rows, cols = src.shape
    dev = src.device
    dt = torch.bfloat16 if bf16 else torch.float32
    bk = 64 if bf16 else 32
    Kp, Mp, n_part = -(-cols // bk) * bk, -(-rows // bk) * bk, -(-rows // 32)
    o, t = _nan((rows, Kp), dev, dt), _nan((cols, Mp), dev, dt)
    part = _nan((n_part, cols), dev) if colpart else None
    f = lambda v: None if v is None else v.float().contiguous()
    gamma, beta = f(gamma), f(beta)
    dims = (ctypes.c_int * 3)()
    raw = lambda v: None if v is None else ctypes.c_void_p(v.data_ptr())      # row-strided views: L.ptr takes contiguous tensors only
    L.check(lib.dimx_op_train_prep(L.BF16 if bf16 else L.F32, mode, raw(src), src.stride(0), raw(src2),
                                   src2.stride(0) if src2 is not None else 0, L.ptr(gamma), L.ptr(beta), rows, cols, L.ptr(o), o.numel(),
                                   L.ptr(t), t.numel(), L.ptr(part), part.numel() if colpart else 0, dims, L.stream_ptr(dev)),
            "dimx_op_train_prep")
    if tuple(dims) != (Kp, Mp, n_part):
        raise L.DimxError("dimx_op_train_prep planned (Kp, Mp, n_part) = %s, expected %s" % (tuple(dims), (Kp, Mp, n_part)))
    return o, t, part


def op_train_cross_entropy(logits, targets):
    """The training step's cross entropy (tr_cross_entropy): logits [R,512] f32, targets [R] (a value outside [0, 512), e.g. -100,
    is ignored) -> (mean loss over the valid targets, 1 / max(count, 1), d logits [R,512])."""
    lib = L.load()
    R = logits.shape[0]
    dev = logits.device
    logits = logits.float().contiguous()
    targets = targets.to(torch.int32).contiguous()
    row_loss, dlogits, out2 = _nan((R,), dev), _nan((R, 512), dev), _nan((2,), dev)
    L.check(lib.dimx_op_train_cross_entropy(L.ptr(logits), L.ptr(targets), R, L.ptr(row_loss), L.ptr(dlogits), L.ptr(out2),
                                            L.stream_ptr(dev)), "dimx_op_train_cross_entropy")
    return out2[0], out2[1], dlogits


def op_sample(logits, top_k=52, temperature=1.0, noise=None, seed=0, step=0, filter_logits_fn=None, filter_kwargs=None,
              return_keep=False):
    """One sampler launch on logits [R,512].  ``filter_logits_fn`` / ``filter_kwargs`` as in Engine.generate (None: top-k with
    ``top_k``, the dimx_op_sample launch); ``return_keep``: also the kept set the kernel used, bool [R,512]."""
    lib = L.load()
    R = logits.shape[0]
    tok = torch.empty(R, dtype=torch.int32, device=logits.device)
    if filter_logits_fn is not None or filter_kwargs or return_keep:
        kind, top_k, fa, fb = sampling.resolve(filter_logits_fn, filter_kwargs, top_k)
        keep = torch.empty(R, 512, dtype=torch.uint8, device=logits.device) if return_keep else None
        L.check(lib.dimx_op_sample_filtered(L.ptr(logits.contiguous()), R, kind, int(top_k), fa, fb, float(temperature),
                                            L.ptr(noise), int(seed), int(step), L.ptr(tok), L.ptr(keep),
                                            L.stream_ptr(logits.device)), "dimx_op_sample_filtered")
        return (tok, keep.bool()) if return_keep else tok
    L.check(lib.dimx_op_sample(L.ptr(logits.contiguous()), R, top_k, float(temperature), L.ptr(noise), int(seed),
                               int(step), L.ptr(tok), L.stream_ptr(logits.device)), "dimx_op_sample")
    return tok


def op_sample_guided(cond, uncond, scale, top_k=52, temperature=1.0, noise=None, seed=0, step=0, filter_logits_fn=None,
                     filter_kwargs=None, return_guided=True):
    """One guided sampler launch (dimx_op_sample_guided; the definition is dimx.guidance): cond / uncond [R,512], or
    [nslab,R,512] split slabs that the kernel adds in slab order; the other arguments as ``op_sample``.  Returns tokens [2R]
    (row r again at r + R: what the guided step feeds its unconditional half) and, with ``return_guided``, the guided logits
    [R,512] the kernel sampled from."""
    lib = L.load()
    assert cond.shape == uncond.shape and cond.dtype == torch.float32 and uncond.dtype == torch.float32
    cond, uncond = cond.contiguous(), uncond.contiguous()
    nslab = cond.shape[0] if cond.dim() == 3 else 1
    R = cond.shape[-2]
    kind, top_k, fa, fb = sampling.resolve(filter_logits_fn, filter_kwargs, top_k)
    tok = torch.empty(2 * R, dtype=torch.int32, device=cond.device)
    g = torch.empty(R, 512, dtype=torch.float32, device=cond.device) if return_guided else None
    L.check(lib.dimx_op_sample_guided(L.ptr(cond), L.ptr(uncond), R, nslab, R * 512, float(scale), kind, int(top_k), fa, fb,
                                      float(temperature), L.ptr(noise), int(seed), int(step), L.ptr(tok), L.ptr(g),
                                      L.stream_ptr(cond.device)), "dimx_op_sample_guided")
    return (tok, g) if return_guided else tok


def op_chain(x, gamma, a1=None, w1=None, slabs=None, w2=None):
    """One XCD-local chain launch (csrc/chain.hip): x [B,C] f32 is updated in place; returns (y bf16 [B,C],
    out2 f32 [B,N2] or None).  a1 [B,K1] / w1 [C,K1] / w2 [N2,C] are converted to bf16."""
    lib = L.load()
    dev = x.device
    B, C = x.shape
    bf = lambda t: None if t is None else t.to(torch.bfloat16).contiguous()
    a1, w1, w2 = bf(a1), bf(w1), bf(w2)
    y = torch.empty(B, C, dtype=torch.bfloat16, device=dev)
    out2 = torch.empty(B, w2.shape[0], dtype=torch.float32, device=dev) if w2 is not None else None
    scratch = torch.zeros(512 + B * C, dtype=torch.int32, device=dev)
    nslab = 0 if slabs is None else slabs.shape[0]
    L.check(lib.dimx_op_chain(L.ptr(a1), a1.shape[1] if a1 is not None else 0, L.ptr(w1), L.ptr(x),
                              L.ptr(slabs.contiguous()) if slabs is not None else None, nslab, L.ptr(gamma), L.ptr(y),
                              L.ptr(w2), w2.shape[0] if w2 is not None else 0, L.ptr(out2), B, C, L.ptr(scratch),
                              L.stream_ptr(dev)), "dimx_op_chain")
    torch.cuda.synchronize(dev)
    flags = int(scratch[129].item())
    if flags:
        raise L.DimxError("chain kernel error flags 0x%x (1 = (XCD, slot) claimed twice, 2 = group barrier timeout)" % flags)
    return y, out2


def op_chain_ln(x, a1, w1, w2s=None, colsum2=None, return_flags=False):
    """Deferred-LayerNorm chain launch: x [B,C] f32 += a1 . w1^T in place; returns (y = bf16(x) [B,C], stats [8,32,32,2],
    out2 [B,N2] or None) with out2 = LayerNorm(x) * gamma . W2^T when w2s = gamma o W2 (bf16) and colsum2 = w2s row sums.
    stats[g, c, r] = {sum, centred sum of squares} of CU c's column slice of row 32 g + r.  return_flags: also the kernel's
    flag word (bit 2 = precision guard: some row's |mean| > 8 std)."""
    lib = L.load()
    dev = x.device
    B, C = x.shape
    a1, w1 = a1.to(torch.bfloat16).contiguous(), w1.to(torch.bfloat16).contiguous()
    y = torch.empty(B, C, dtype=torch.bfloat16, device=dev)
    stats = torch.zeros(8, 32, 32, 2, dtype=torch.float32, device=dev)
    out2 = torch.empty(B, w2s.shape[0], dtype=torch.float32, device=dev) if w2s is not None else None
    scratch = torch.zeros(512 + B * C, dtype=torch.int32, device=dev)
    L.check(lib.dimx_op_chain_ln(L.ptr(a1), a1.shape[1], L.ptr(w1), L.ptr(x), L.ptr(y), L.ptr(stats), L.ptr(w2s),
                                 L.ptr(colsum2), w2s.shape[0] if w2s is not None else 0, L.ptr(out2), B, C, L.ptr(scratch),
                                 L.stream_ptr(dev)), "dimx_op_chain_ln")
    torch.cuda.synchronize(dev)
    flags = int(scratch[129].item())
    if flags & 3:
        raise L.DimxError("chain kernel error flags 0x%x (1 = (XCD, slot) claimed twice, 2 = group barrier timeout)" % flags)
    return (y, stats, out2, flags) if return_flags else (y, stats, out2)


def op_gemm_ln(a, ws, stats, colsum, bias=None, act=0, out_bf16=False):
    """act(LayerNorm-corrected a . ws^T + bias): a = bf16(x) un-normalised, ws = gamma o W (bf16), stats from op_chain_ln."""
    lib = L.load()
    M, K = a.shape
    N = ws.shape[0]
    out = torch.empty(M, N, dtype=torch.bfloat16 if out_bf16 else torch.float32, device=a.device)
    L.check(lib.dimx_op_gemm_ln(L.BF16 if out_bf16 else L.F32, L.ptr(a), L.ptr(ws), L.ptr(out), M, N, K, L.ptr(bias), act,
                                L.ptr(stats), L.ptr(colsum), L.stream_ptr(a.device)), "dimx_op_gemm_ln")
    return out


def op_decode_attn(q, kcache, vcache, n_keys, scale, kmask=None, nsplit=0):
    """q [B,H*64]; kcache/vcache [B,H,Tmax,64] (f32 or bf16) -> [B,H*64]."""
    lib = L.load()
    B, H, Tmax, _ = kcache.shape
    bf = kcache.dtype == torch.bfloat16
    q_f32 = q.dtype == torch.float32 and bf      # f32 projection slab feeding a bf16 cache (generate's form)
    out = torch.empty(q.shape, dtype=kcache.dtype, device=q.device)
    L.check(lib.dimx_op_decode_attn(L.BF16 if bf else L.F32, L.ptr(q), L.ptr(kcache), L.ptr(vcache), L.ptr(out), B, H,
                                    Tmax, n_keys, float(scale), L.ptr(kmask), nsplit, 1 if q_f32 else 0,
                                    L.stream_ptr(q.device)),
            "dimx_op_decode_attn")
    return out


def op_append_attn(qkv, kcache, vcache, n0, scale):
    """Append attention (dimx_op_append_attn): qkv [B, c, 3*H*64] f32 (q | k | v of the c new rows of every clip), kcache / vcache
    [B, H, Tmax, 64] (f32 or bf16) holding n0 rows.  The k / v rows become cache rows [n0, n0 + c) (in place), query i attends over
    the rows 0 .. n0 + i -> [B, c, H*64] in the cache type."""
    lib = L.load()
    B, H, Tmax, _ = kcache.shape
    Bq, c, ld = qkv.shape
    assert Bq == B and qkv.dtype == torch.float32 and qkv.is_contiguous() and kcache.is_contiguous() and vcache.is_contiguous()
    bf = kcache.dtype == torch.bfloat16
    out = torch.empty(B, c, H * 64, dtype=kcache.dtype, device=qkv.device)
    L.check(lib.dimx_op_append_attn(L.BF16 if bf else L.F32, L.ptr(qkv), ld, L.ptr(kcache), L.ptr(vcache), L.ptr(out), B, H, Tmax,
                                    int(n0), c, float(scale), L.stream_ptr(qkv.device)), "dimx_op_append_attn")
    return out


def op_cross_attn_win(q, kcache, vcache, lookahead, scale, t0=0, n_keys=None, kmask=None, out=None):
    """Windowed cross attention for many queries (dimx_op_cross_attn_win): q [B, Lq, H*64] f32, query row i of a clip at position
    t0 + i; kcache / vcache [B, H, Tp, 64] (f32 or bf16), of which the first ``n_keys`` rows are keys (default Tp); kmask [B, >= n_keys]
    uint8 keep-mask or None.  Row i attends over the kept keys j < clamp(t0 + i + 2 + lookahead, 1, n_keys) (dimx.online)
    -> [B, Lq, H*64] in the cache type (``out``: a contiguous tensor of that shape and type to write into)."""
    lib = L.load()
    B, H, Tp, _ = kcache.shape
    Bq, Lq, ld = q.shape
    assert Bq == B and q.dtype == torch.float32 and q.is_contiguous() and kcache.is_contiguous() and vcache.is_contiguous()
    assert kmask is None or (kmask.dtype == torch.uint8 and kmask.is_contiguous() and kmask.shape[0] == B)
    bf = kcache.dtype == torch.bfloat16
    if out is None:
        out = torch.empty(B, Lq, H * 64, dtype=kcache.dtype, device=q.device)
    assert tuple(out.shape) == (B, Lq, H * 64) and out.dtype == kcache.dtype and out.is_contiguous()
    L.check(lib.dimx_op_cross_attn_win(L.BF16 if bf else L.F32, L.ptr(q), ld, L.ptr(kcache), L.ptr(vcache), Tp, L.ptr(out), H * 64, B, H, Lq,
                                       int(t0), Tp if n_keys is None else int(n_keys), int(lookahead), L.ptr(kmask),
                                       kmask.shape[1] if kmask is not None else 0, float(scale), L.stream_ptr(q.device)),
            "dimx_op_cross_attn_win")
    return out


def op_decode_attn_ex(q, kcache, vcache, scale, n_keys=0, step=None, kmask=None, kmask_ld=None, rows_per_clip=1, nsplit=0,
                      q_f32=None, lookahead=None, tab=None, hist=None, tab_koff=0, tab_voff=0, tab_rows=None):
    """Every form of the decode step's attention as dimx_generate launches it (include/dimx.h dimx_op_decode_attn_ex).
    q: [R, q_ld] or f32 split-K slabs [nslab, R, q_ld] (R = B * rows_per_clip); kcache / vcache [B, H, Tmax, 64] (f32 or bf16).
    step (int32 device scalar) selects the self form: q's rows hold q | k | v, k / v are appended at *step; otherwise the cross
    form over n_keys keys with an optional kmask [B, kmask_ld] (uint8).  q_f32: q holds f32 slabs (default: q is f32).
    lookahead (int): the windowed cross form of an online generation (dimx_op_decode_attn_win) -- step is then the decode step
    counter and the keys are j < dimx.online.visible(*step, lookahead, n_keys).
    tab [rows, tab_ld] (cache type) with hist [B, hist_ld] int32: the table form of the self form (dimx_op_decode_attn_tab) -- the
    cached K / V row of position j is row hist[b, j] of tab (K of head h at column tab_koff + h*64, V at tab_voff + h*64; ids are
    clamped to tab_rows - 1, default the table's row count), nothing is appended and kcache / vcache are not touched."""
    lib = L.load()
    B, H, Tmax, _ = kcache.shape
    bf = kcache.dtype == torch.bfloat16
    qs = q if q.dim() == 3 else q.unsqueeze(0)
    nslab, R, q_ld = qs.shape
    if q_f32 is None:
        q_f32 = q.dtype == torch.float32
    S = rows_per_clip if rows_per_clip > 1 else 1
    out = torch.empty(R, H * 64, dtype=kcache.dtype, device=q.device)
    kld = kmask_ld if kmask_ld is not None else (kmask.shape[1] if kmask is not None else 0)
    if tab is not None:
        L.check(lib.dimx_op_decode_attn_tab(L.BF16 if bf else L.F32, L.ptr(qs), q_ld, 1 if q_f32 else 0, nslab, qs.stride(0),
                                            L.ptr(kcache), L.ptr(vcache), L.ptr(out), H * 64, B, H, Tmax, L.ptr(step), float(scale),
                                            nsplit, L.ptr(tab), tab.stride(0), int(tab_koff), int(tab_voff),
                                            tab.shape[0] if tab_rows is None else int(tab_rows), L.ptr(hist), hist.stride(0),
                                            L.stream_ptr(q.device)), "dimx_op_decode_attn_tab")
        return out
    if lookahead is not None:
        L.check(lib.dimx_op_decode_attn_win(L.BF16 if bf else L.F32, L.ptr(qs), q_ld, 1 if q_f32 else 0, nslab, qs.stride(0),
                                            L.ptr(kcache), L.ptr(vcache), L.ptr(out), H * 64, B, H, Tmax, L.ptr(step), n_keys,
                                            L.ptr(kmask), kld, S, float(scale), nsplit, int(lookahead), L.stream_ptr(q.device)),
                "dimx_op_decode_attn_win")
        return out
    L.check(lib.dimx_op_decode_attn_ex(L.BF16 if bf else L.F32, L.ptr(qs), q_ld, 1 if q_f32 else 0, nslab, qs.stride(0),
                                       1 if step is not None else 0, L.ptr(kcache), L.ptr(vcache), L.ptr(out), H * 64, B, H, Tmax,
                                       L.ptr(step), n_keys, L.ptr(kmask), kld, S, float(scale), nsplit, L.stream_ptr(q.device)),
            "dimx_op_decode_attn_ex")
    return out


def op_kv8_quantize(cache, T=None, codes=None, scales=None):
    """FP8 cross K/V, the quantiser (dimx_op_kv8_quantize; dimx.kv8.quantize): cache [B, H, Tp, 64] f32 or bf16; rows 0 .. T - 1
    (default Tp) of every (clip, head) -> (codes [B, H, Tp, 64] uint8, scales [B, H, Tp] f32).  ``codes`` / ``scales``: tensors to
    write into (rows at or past T are left as they are); default: zero-filled ones."""
    lib = L.load()
    B, H, Tp, _ = cache.shape
    assert cache.shape[3] == 64
    codes = torch.zeros(B, H, Tp, 64, dtype=torch.uint8, device=cache.device) if codes is None else codes
    scales = torch.zeros(B, H, Tp, dtype=torch.float32, device=cache.device) if scales is None else scales
    L.check(lib.dimx_op_kv8_quantize(L.BF16 if cache.dtype == torch.bfloat16 else L.F32, L.ptr(cache), B, H, Tp, Tp if T is None else int(T),
                                     L.ptr(codes), L.ptr(scales), L.stream_ptr(cache.device)), "dimx_op_kv8_quantize")
    return codes, scales


def op_kv8_append(caches, codes, scales, n0, c):
    """The incremental quantiser (dimx_op_kv8_append; dimx.kv8.append), one launch: ``caches`` a list of 2 * depth tensors
    [B, H, Tc, 64] f32 or bf16 -- K of layer 0, V of layer 0, K of layer 1, ... -- whose rows [n0, n0 + c) of every (clip, head) go,
    quantised, into the same rows of ``codes`` (2 * depth tensors [B, H, Tp, 64] uint8) and ``scales`` ([B, H, Tp] f32), in place."""
    lib = L.load()
    n = len(caches)
    assert n % 2 == 0 and len(codes) == n and len(scales) == n
    B, H, Tc, _ = caches[0].shape
    Tp = codes[0].shape[2]
    for a, cd, sc in zip(caches, codes, scales):
        assert tuple(a.shape) == (B, H, Tc, 64) and a.dtype == caches[0].dtype and tuple(cd.shape) == (B, H, Tp, 64) and tuple(sc.shape) == (B, H, Tp)
    arr = lambda ts: (ctypes.c_void_p * n)(*[L.ptr(t).value for t in ts])
    L.check(lib.dimx_op_kv8_append(L.BF16 if caches[0].dtype == torch.bfloat16 else L.F32, arr(caches), arr(codes), arr(scales), n // 2, B, H,
                                   Tc, Tp, int(n0), int(c), L.stream_ptr(caches[0].device)), "dimx_op_kv8_append")


def op_decode_attn_kv8(q, kcodes, kscale, vcodes, vscale, scale, n_keys, kmask=None, kmask_ld=None, nsplit=0, out_bf16=False, step=None,
                       lookahead=None, rows_per_clip=1):
    """The decode step's cross attention over FP8 codes (dimx_op_decode_attn_kv8; dimx.kv8.attention): q [B, q_ld] f32 or split-K
    slabs [nslab, B, q_ld]; kcodes / vcodes [B, H, Tmax, 64] uint8, kscale / vscale [B, H, Tmax] f32; kmask [B, kmask_ld] uint8 or
    None -> [B, H*64] f32 (bf16 with ``out_bf16``).  lookahead (int) with step (int32 device scalar): the windowed form, keys
    j < dimx.online.visible(*step, lookahead, n_keys)."""
    lib = L.load()
    B, H, Tmax, _ = kcodes.shape
    qs = q if q.dim() == 3 else q.unsqueeze(0)
    nslab, R, q_ld = qs.shape
    out = torch.empty(R, H * 64, dtype=torch.bfloat16 if out_bf16 else torch.float32, device=q.device)
    kld = kmask_ld if kmask_ld is not None else (kmask.shape[1] if kmask is not None else 0)
    L.check(lib.dimx_op_decode_attn_kv8(L.BF16 if out_bf16 else L.F32, L.ptr(qs), q_ld, 1 if q.dtype == torch.float32 else 0, nslab,
                                        qs.stride(0), L.ptr(kcodes), L.ptr(kscale), L.ptr(vcodes), L.ptr(vscale), L.ptr(out), H * 64, B, H,
                                        Tmax, L.ptr(step), int(n_keys), L.ptr(kmask), kld, int(rows_per_clip), float(scale), int(nsplit),
                                        0 if lookahead is None else int(lookahead), 0 if lookahead is None else 1,
                                        L.stream_ptr(q.device)), "dimx_op_decode_attn_kv8")
    return out


def op_decode_attn_kv8_multi(q, kcodes, kscale, vcodes, vscale, scale, n_keys, rows_per_clip, kmask=None, kmask_ld=None, out_bf16=False,
                             step=None, lookahead=None, exact=None, out=None):
    """S = ``rows_per_clip`` query rows per clip over FP8 codes on the matrix cores (dimx_op_decode_attn_kv8_multi;
    dimx.kv8.attention_rows): q [B*S, q_ld] f32, split-K slabs [nslab, B*S, q_ld] f32 or one bf16 row array [B*S, q_ld]; rows
    b*S .. b*S+S-1 share clip b's kcodes / vcodes [B, H, Tmax, 64] uint8, kscale / vscale [B, H, Tmax] f32 and kmask row.
    ``exact``: True = the exact form (three bf16 planes), False = the matrix-core form (q and p * vscale rounded to bf16); None =
    what a handle of the output type takes (exact for f32 out).  ``out``: a [>= B*S, o_ld] tensor to write rows 0 .. B*S-1 of
    (columns past H*64 and rows past B*S are left alone); default a fresh [B*S, H*64].  lookahead with step: the windowed form."""
    lib = L.load()
    B, H, Tmax, _ = kcodes.shape
    qs = q if q.dim() == 3 else q.unsqueeze(0)
    nslab, R, q_ld = qs.shape
    if out is None:
        out = torch.empty(R, H * 64, dtype=torch.bfloat16 if out_bf16 else torch.float32, device=q.device)
    out_bf16 = out.dtype == torch.bfloat16
    if exact is None:
        exact = not out_bf16
    kld = kmask_ld if kmask_ld is not None else (kmask.shape[1] if kmask is not None else 0)
    L.check(lib.dimx_op_decode_attn_kv8_multi(L.BF16 if out_bf16 else L.F32, L.ptr(qs), q_ld, 1 if q.dtype == torch.float32 else 0, nslab,
                                              qs.stride(0), L.ptr(kcodes), L.ptr(kscale), L.ptr(vcodes), L.ptr(vscale), L.ptr(out),
                                              out.stride(0), B, H, Tmax, L.ptr(step), int(n_keys), L.ptr(kmask), kld, int(rows_per_clip),
                                              float(scale), 0, 0 if lookahead is None else int(lookahead), 0 if lookahead is None else 1,
                                              1 if exact else 0, L.stream_ptr(q.device)), "dimx_op_decode_attn_kv8_multi")
    return out


def op_decode_attn_self_kv8(qkv, kcodes, kscale, vcodes, vscale, scale, n, nsplit=0, out_bf16=False, step=None):
    """The decode step's self attention over FP8 self caches (dimx_op_decode_attn_self_kv8; dimx.kv8.self_step): qkv [R, ld] f32 or
    split-K slabs [nslab, R, ld], rows q | k | v (ld >= 3*H*64); kcodes / vcodes [R, H, Tmax, 64] uint8, kscale / vscale [R, H, Tmax]
    f32 with rows 0 .. n - 1 cached.  Row n of the four arrays is written in place -> [R, H*64] f32 (bf16 with ``out_bf16``).
    ``step``: an int32 device scalar the kernel reads n from (clamped to 0 .. n); default: a fresh one holding n."""
    lib = L.load()
    B, H, Tmax, _ = kcodes.shape
    qs = qkv if qkv.dim() == 3 else qkv.unsqueeze(0)
    nslab, R, ld = qs.shape
    assert qs.dtype == torch.float32 and R == B
    if step is None:
        step = torch.tensor([int(n)], dtype=torch.int32, device=qkv.device)
    out = torch.empty(R, H * 64, dtype=torch.bfloat16 if out_bf16 else torch.float32, device=qkv.device)
    L.check(lib.dimx_op_decode_attn_self_kv8(L.BF16 if out_bf16 else L.F32, L.ptr(qs), ld, nslab, qs.stride(0), L.ptr(kcodes), L.ptr(kscale),
                                             L.ptr(vcodes), L.ptr(vscale), L.ptr(out), H * 64, B, H, Tmax, L.ptr(step), int(n), float(scale),
                                             int(nsplit), L.stream_ptr(qkv.device)), "dimx_op_decode_attn_self_kv8")
    return out


def op_layer_chain(qkv, sk, sv, ck, cv, n_keys, kmask, w_so, w_cq, colsum_cq, w_co, x, step, B=None, call_index=0, scale=0.125,
                   o=None, qc=None, y=None, stats=None, scratch=None, prof=None, tab=None, hist=None, tab_koff=0, tab_voff=768,
                   tab_rows=None):
    """The attention half of one decoder layer as one launch (csrc/chain.hip xcd_layer_kernel; include/dimx.h dimx_op_layer_chain):
    qkv f32 slabs [nslab, rows, 2304]; sk / sv [rows, 12, T, 64] and ck / cv [rows, 12, Tp, 64] bf16; kmask [rows, n_keys] uint8 or
    None; w_so / w_co [1152, 768], w_cq [768, 1152] bf16 (w_cq = gamma o Wq) with colsum_cq its f32 row sums; x [rows, 1152] f32 is
    updated in place; step an int32 device scalar (cached self-attention keys).  B clips (default: the rows of x; buffers may carry
    more rows, which the launch leaves alone).  o [rows, 768] bf16, qc [rows, 768] f32, y [rows, 1152] bf16, stats [8, 32, 32, 2] f32
    and a zeroed 1024-word int32 scratch are allocated unless passed; call_index = 0, 1, 2, ... for consecutive calls on one
    scratch.  tab / hist: the table form of the self attention (dimx_op_layer_chain_tab; arguments as op_decode_attn_ex).
    Synchronises and returns (y, o, qc, stats, flags) with flags = scratch[768] (0 = ok, 1 = an (XCD, slot) claimed twice, 2 = a
    group barrier timed out, 4 = precision guard: some row's |mean| > 8 std)."""
    lib = L.load()
    dev = x.device
    rows = x.shape[0]
    B = rows if B is None else int(B)
    qs = qkv if qkv.dim() == 3 else qkv.unsqueeze(0)
    o = torch.empty(rows, 768, dtype=torch.bfloat16, device=dev) if o is None else o
    qc = torch.empty(rows, 768, dtype=torch.float32, device=dev) if qc is None else qc
    y = torch.empty(rows, 1152, dtype=torch.bfloat16, device=dev) if y is None else y
    stats = torch.zeros(8, 32, 32, 2, dtype=torch.float32, device=dev) if stats is None else stats
    scratch = torch.zeros(1024, dtype=torch.int32, device=dev) if scratch is None else scratch
    args = [L.ptr(qs), qs.shape[0], qs.stride(0), L.ptr(sk), L.ptr(sv), sk.shape[2], L.ptr(ck), L.ptr(cv), ck.shape[2], int(n_keys),
            L.ptr(kmask), L.ptr(w_so), L.ptr(w_cq), L.ptr(colsum_cq), L.ptr(w_co), L.ptr(x), L.ptr(y), L.ptr(o), L.ptr(qc),
            L.ptr(stats), B, L.ptr(step), int(call_index), float(scale), L.ptr(scratch), L.ptr(prof)]
    if tab is not None:
        L.check(lib.dimx_op_layer_chain_tab(*args, L.ptr(tab), tab.stride(0), int(tab_koff), int(tab_voff),
                                            tab.shape[0] if tab_rows is None else int(tab_rows), L.ptr(hist), hist.stride(0),
                                            L.stream_ptr(dev)), "dimx_op_layer_chain_tab")
    else:
        L.check(lib.dimx_op_layer_chain(*args, L.stream_ptr(dev)), "dimx_op_layer_chain")
    torch.cuda.synchronize(dev)
    return y, o, qc, stats, int(scratch[768].item())


def op_layer_chain_head(qkv0, logits, top_k, noise, rows_total, tokens, emb, params, hist, tab, ck, cv, n_keys, kmask, w_so, w_cq,
                        colsum_cq, w_co, x, B, scale=0.125, tab_koff=0, tab_voff=768, tab_rows=512, logits_out=None):
    """The first decoder layer's launch with the sampling head (include/dimx.h dimx_op_layer_chain_head): params is the 16-word
    int32 parameter block, tokens [rows, n] int32, hist [rows, T] int32, the other operands as op_layer_chain's table form.
    Synchronises and returns (y, o, qc, stats, flags)."""
    lib = L.load()
    dev = x.device
    rows = x.shape[0]
    o = torch.empty(rows, 768, dtype=torch.bfloat16, device=dev)
    qc = torch.empty(rows, 768, dtype=torch.float32, device=dev)
    y = torch.empty(rows, 1152, dtype=torch.bfloat16, device=dev)
    stats = torch.zeros(8, 32, 32, 2, dtype=torch.float32, device=dev)
    scratch = torch.zeros(1024, dtype=torch.int32, device=dev)
    dummy = torch.zeros(16, dtype=torch.bfloat16, device=dev)   # the table form touches no self-attention cache
    L.check(lib.dimx_op_layer_chain_head(L.ptr(qkv0), L.ptr(logits), int(top_k), L.ptr(noise), int(rows_total), L.ptr(tokens),
                                         tokens.stride(0), L.ptr(logits_out), L.ptr(emb), L.ptr(params), L.ptr(dummy), L.ptr(dummy),
                                         hist.shape[1], L.ptr(ck), L.ptr(cv), ck.shape[2], int(n_keys), L.ptr(kmask), L.ptr(w_so),
                                         L.ptr(w_cq), L.ptr(colsum_cq), L.ptr(w_co), L.ptr(x), L.ptr(y), L.ptr(o), L.ptr(qc), L.ptr(stats),
                                         int(B), float(scale), L.ptr(scratch), None, L.ptr(tab), tab.stride(0), int(tab_koff),
                                         int(tab_voff), int(tab_rows), L.ptr(hist), hist.stride(0), L.stream_ptr(dev)),
            "dimx_op_layer_chain_head")
    torch.cuda.synchronize(dev)
    return y, o, qc, stats, int(scratch[768].item())


def op_sample_step(logits, R, top_k, noise, rows_total, tokens, emb, x_next, qkv0, qkv0_out, hist, params, logits_out=None):
    """The sampler launch of a generation step on a 16-word parameter block (include/dimx.h dimx_op_sample_step)."""
    lib = L.load()
    L.check(lib.dimx_op_sample_step(L.ptr(logits), int(R), int(top_k), L.ptr(noise), int(rows_total), L.ptr(tokens), tokens.stride(0),
                                    L.ptr(logits_out), L.ptr(emb), emb.shape[1], L.ptr(x_next), L.ptr(qkv0), L.ptr(qkv0_out),
                                    qkv0.shape[1], L.ptr(hist), hist.stride(0), L.ptr(params), L.stream_ptr(logits.device)),
            "dimx_op_sample_step")
    torch.cuda.synchronize(logits.device)


# ---------------------------------------------------------------- host plumbing of the metric operators
def _device_key(device):
    device = torch.device(device)
    return device.index if device.index is not None else torch.cuda.current_device()


def _workspace(cache, device, need, floor=8):
    """The uint8 workspace of one operator on ``device``: ``cache`` maps device index -> tensor, grown on demand and never shrunk.
    One dict per operator: the operators may be in flight together on one stream, and the *_sweeps readers take the last call's."""
    key = _device_key(device)
    ws = cache.get(key)
    if ws is None or ws.numel() < need:
        ws = cache[key] = torch.empty(max(need, floor), dtype=torch.uint8, device=device)
    return ws


def _lens_i32(lens, device, B, what):
    """lens (tensor or host sequence) -> int32 [B] on ``device``."""
    if torch.is_tensor(lens):
        lens_d = lens.to(device=device, dtype=torch.int32).contiguous()
    else:
        lens_d = torch.tensor([int(n) for n in lens], dtype=torch.int32).to(device)
    if lens_d.numel() != B:
        raise L.DimxError("%s: %d lens for %d clips" % (what, lens_d.numel(), B))
    return lens_d


def _f32_rows(t, copy_strided=True):
    """float32 with a feature (last) stride of 1: every other stride is passed to the kernel as it is."""
    t = t if t.dtype == torch.float32 else t.float()
    return t.contiguous() if copy_strided and t.stride(-1) != 1 else t


_FD_WS = {}     # device index -> uint8 workspace of op_fd_select


def op_fd_select(y_true, y_pred, lens, cols=(0, None), want_best=True):
    """Best-of-S selection by Frechet distance (dimx_op_fd_select, csrc/fd_select.hip): y_true [B, L, W] f32, y_pred [B, S, L, W]
    f32 on one GPU, lens[j] = valid frames of clip j, cols = (c0, c1) the columns that enter the distance (None = the row's
    end) -> (fd [B, S] f64, win [B] int32, ok [B] uint8, best [B, L, W] f32 or None).  The clip / sample / frame strides are taken
    from the tensors (views such as ``tgt[lo:hi, 1:]`` are passed as they are); only a feature stride other than 1 is copied.
    Asynchronous on the current stream.  CPU tensors raise: there is no CPU fallback."""
    if not (torch.is_tensor(y_true) and torch.is_tensor(y_pred) and y_true.is_cuda and y_pred.is_cuda):
        raise L.DimxError("op_fd_select runs on the GPU only: y_true / y_pred must be CUDA tensors (no CPU fallback)")
    if y_true.dim() != 3 or y_pred.dim() != 4 or y_pred.shape[0] != y_true.shape[0] or y_pred.shape[2] != y_true.shape[1] \
            or y_pred.shape[3] != y_true.shape[2] or y_pred.device != y_true.device:
        raise L.DimxError("op_fd_select: y_true [B, L, W] and y_pred [B, S, L, W] expected, got %s and %s" % (tuple(y_true.shape),
                                                                                                           tuple(y_pred.shape)))
    lib = L.load()
    dev = y_pred.device
    B, S, Ln, W = y_pred.shape
    y_true, y_pred = _f32_rows(y_true, W > 1), _f32_rows(y_pred, W > 1)
    c0 = int(cols[0])
    F = (W if cols[1] is None else int(cols[1])) - c0
    lens_d = _lens_i32(lens, dev, B, "op_fd_select")
    fd = torch.empty(B, S, dtype=torch.float64, device=dev)
    win = torch.empty(B, dtype=torch.int32, device=dev)
    ok = torch.empty(B, dtype=torch.uint8, device=dev)
    best = torch.empty(B, Ln, W, dtype=torch.float32, device=dev) if want_best else None
    need = int(lib.dimx_op_fd_select_ws_bytes(B, S, F))
    ws = _workspace(_FD_WS, dev, need)
    with torch.cuda.device(dev):
        L.check(lib.dimx_op_fd_select(ctypes.c_void_p(y_true.data_ptr()), y_true.stride(0), y_true.stride(1),
                                      ctypes.c_void_p(y_pred.data_ptr()), y_pred.stride(0), y_pred.stride(1), y_pred.stride(2),
                                      L.ptr(lens_d), B, S, Ln, W, c0, F, L.ptr(fd), L.ptr(win), L.ptr(ok), L.ptr(best),
                                      ctypes.c_void_p(ws.data_ptr()), ws.numel(), L.stream_ptr(dev)), "dimx_op_fd_select")
    return fd, win, ok, best


def op_seq_logprob(logits, tokens, first=None, last=None, rows_per_clip=1, want_tokens=False):
    """Sequence log-likelihoods over dumped logits (dimx_op_seq_logprob, csrc/seq_score.hip; the definition is dimx.scoring):
    logits [R, n, 512] f32 and tokens [R, n] on one GPU, first / last [R / rows_per_clip] (tensors or host sequences; None = 0 / n)
    -> SeqScores(score f64 [R], count int32 [R]); with ``want_tokens`` (SeqScores, per-token f64 [R, n]).  Strided views of ``logits``
    and ``tokens`` are passed as they are: only the innermost stride must be 1 (tokens of another dtype than int32 are converted).
    Asynchronous on the current stream.  CPU tensors raise: there is no CPU fallback (dimx.scoring.sequence_scores is the host form)."""
    from .scoring import VOCAB, SeqScores
    if not (torch.is_tensor(logits) and torch.is_tensor(tokens) and logits.is_cuda and tokens.is_cuda):
        raise L.DimxError("op_seq_logprob runs on the GPU only: logits / tokens must be CUDA tensors (no CPU fallback)")
    if logits.dim() != 3 or logits.shape[2] != VOCAB or tuple(tokens.shape) != tuple(logits.shape[:2]) or tokens.device != logits.device:
        raise L.DimxError("op_seq_logprob: logits [R, n, %d] and tokens [R, n] on one device expected, got %s and %s"
                          % (VOCAB, tuple(logits.shape), tuple(tokens.shape)))
    lib = L.load()
    dev = logits.device
    R, n = int(logits.shape[0]), int(logits.shape[1])
    rpc = int(rows_per_clip)
    logits = logits if logits.dtype == torch.float32 else logits.float()
    if logits.stride(2) != 1:
        logits = logits.contiguous()
    tokens = tokens if tokens.dtype == torch.int32 else tokens.to(torch.int32)
    if tokens.stride(1) != 1 and n > 1:
        tokens = tokens.contiguous()
    clips = R // rpc if rpc >= 1 and R % rpc == 0 else -1      # the library refuses the call; no lens are uploaded for it
    first_d = _lens_i32(first, dev, clips, "op_seq_logprob(first)") if first is not None and clips >= 0 else None
    last_d = _lens_i32(last, dev, clips, "op_seq_logprob(last)") if last is not None and clips >= 0 else None
    score = torch.empty(R, dtype=torch.float64, device=dev)
    count = torch.empty(R, dtype=torch.int32, device=dev)
    tok_lp = torch.empty(R, n, dtype=torch.float64, device=dev) if want_tokens else None
    step_stride = logits.stride(1) if n > 1 else VOCAB     # a dimension of one entry has no meaningful stride
    with torch.cuda.device(dev):
        L.check(lib.dimx_op_seq_logprob(ctypes.c_void_p(logits.data_ptr()), logits.stride(0), step_stride,
                                        ctypes.c_void_p(tokens.data_ptr()), tokens.stride(0), L.ptr(first_d), L.ptr(last_d), rpc, R, n,
                                        L.ptr(tok_lp), L.ptr(score), L.ptr(count), L.stream_ptr(dev)), "dimx_op_seq_logprob")
    out = SeqScores(score, count)
    return (out, tok_lp) if want_tokens else out


def op_beam_step(logits, cum, mode, forced_tok=None, beam_width=1):
    """One beam-search selection (dimx_op_beam_step, csrc/beam.hip; the definition is dimx.beam.beam_step): logits [B*W, 512] f32,
    cum [B*W] f64, mode [B] (dimx.beam.LIVE / FORCED / FROZEN), forced_tok [B] or None -> (parent int32 [B*W], token int32 [B*W],
    cum' f64 [B*W]).  Asynchronous on the current stream.  CPU tensors raise: dimx.beam.beam_step is the host form."""
    if not (torch.is_tensor(logits) and logits.is_cuda and torch.is_tensor(cum) and cum.is_cuda):
        raise L.DimxError("op_beam_step runs on the GPU only: logits / cum must be CUDA tensors (no CPU fallback)")
    W, dev = int(beam_width), logits.device
    if logits.dim() != 2 or logits.shape[1] != 512 or W < 1 or logits.shape[0] % W or cum.numel() != logits.shape[0]:
        raise L.DimxError("op_beam_step: logits [B*W, 512] and cum [B*W] expected, got %s and %s" % (tuple(logits.shape), tuple(cum.shape)))
    R = int(logits.shape[0])
    B = R // W
    logits = logits.to(torch.float32).contiguous()
    cum = cum.to(torch.float64).contiguous()
    mode_d = _lens_i32(mode, dev, B, "op_beam_step(mode)")
    forced_d = _lens_i32(forced_tok, dev, B, "op_beam_step(forced_tok)") if forced_tok is not None else None
    parent = torch.empty(R, dtype=torch.int32, device=dev)
    token = torch.empty(R, dtype=torch.int32, device=dev)
    out = torch.empty(R, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        L.check(L.load().dimx_op_beam_step(L.ptr(logits), L.ptr(cum), L.ptr(mode_d), L.ptr(forced_d), B, W, L.ptr(parent), L.ptr(token),
                                           L.ptr(out), L.stream_ptr(dev)), "dimx_op_beam_step")
    return parent, token, out


def op_beam_reorder(cache, parent, c, beam_width):
    """In-place reorder of a self-attention cache by parent beam (dimx_op_beam_reorder, csrc/beam.hip): cache [R, H, T, 64] f32 or
    bf16, contiguous, parent [R] int32 -> cache[clip*W + w, :, :c+1] = old cache[clip*W + parent[w], :, :c+1]; returns ``cache``."""
    if not (torch.is_tensor(cache) and cache.is_cuda and cache.is_contiguous() and cache.dim() == 4 and cache.shape[3] == 64
            and cache.dtype in (torch.float32, torch.bfloat16)):
        raise L.DimxError("op_beam_reorder: a contiguous CUDA cache [R, H, T, 64] of float32 or bfloat16 expected")
    dev = cache.device
    R, H, T, _ = (int(v) for v in cache.shape)
    parent_d = _lens_i32(parent, dev, R, "op_beam_reorder(parent)")
    with torch.cuda.device(dev):
        L.check(L.load().dimx_op_beam_reorder(L.ptr(cache), L.BF16 if cache.dtype == torch.bfloat16 else L.F32, L.ptr(parent_d), R,
                                              int(beam_width), H, T, int(c), L.stream_ptr(dev)), "dimx_op_beam_reorder")
    return cache


def op_beam_reorder_kv8(codes, scale, parent, c, beam_width):
    """In-place reorder of one FP8 code plane and its scale plane by parent beam (dimx_op_beam_reorder_kv8, csrc/beam.hip; the
    definition is dimx.kv8.reorder): codes [R, H, Tp, 64] uint8 and scale [R, H, Tp] float32, contiguous, parent [R] int32 -> codes
    and scale of the positions 0 .. c of row clip*W + w become those of row clip*W + parent[w]; returns ``(codes, scale)``."""
    if not (torch.is_tensor(codes) and torch.is_tensor(scale) and codes.is_cuda and scale.is_cuda and codes.is_contiguous()
            and scale.is_contiguous() and codes.dim() == 4 and codes.shape[3] == 64 and codes.dtype == torch.uint8
            and scale.dtype == torch.float32 and tuple(scale.shape) == tuple(codes.shape[:3]) and scale.device == codes.device):
        raise L.DimxError("op_beam_reorder_kv8: contiguous CUDA planes codes [R, H, Tp, 64] uint8 and scale [R, H, Tp] float32 expected")
    dev = codes.device
    R, H, Tp, _ = (int(v) for v in codes.shape)
    parent_d = _lens_i32(parent, dev, R, "op_beam_reorder_kv8(parent)")
    with torch.cuda.device(dev):
        L.check(L.load().dimx_op_beam_reorder_kv8(L.ptr(codes), L.ptr(scale), L.ptr(parent_d), R, int(beam_width), H, Tp, int(c),
                                                  L.stream_ptr(dev)), "dimx_op_beam_reorder_kv8")
    return codes, scale


def op_score_select(score, y_pred, lens, tokens=None):
    """Best-of-S selection by sequence log-likelihood (dimx_op_score_select, csrc/seq_score.hip): score [B, S] f64 (or [B*S]),
    y_pred [B, S, L, W] f32 on the same GPU, lens[j] = valid frames of clip j, tokens [B*S, n] (optional)
    -> (win [B] int32, ok [B] uint8, best [B, L, W] f32[, best_tokens [B, n] int32]): the first maximum of each row (NaN
    counts as -inf), ok = 0 when no try of the clip has a finite score, the winner's rows (zero for t >= lens[j] and for ok = 0) and
    its token row (-100 for ok = 0).  Strides as in op_fd_select.  Asynchronous on the current stream.  CPU tensors raise."""
    if not (torch.is_tensor(score) and torch.is_tensor(y_pred) and score.is_cuda and y_pred.is_cuda):
        raise L.DimxError("op_score_select runs on the GPU only: score / y_pred must be CUDA tensors (no CPU fallback)")
    if y_pred.dim() != 4 or score.numel() != y_pred.shape[0] * y_pred.shape[1] or score.device != y_pred.device:
        raise L.DimxError("op_score_select: score [B, S] and y_pred [B, S, L, W] on one device expected, got %s and %s"
                          % (tuple(score.shape), tuple(y_pred.shape)))
    lib = L.load()
    dev = y_pred.device
    B, S, Ln, W = (int(v) for v in y_pred.shape)
    score = score.to(torch.float64).reshape(B, S).contiguous()
    y_pred = _f32_rows(y_pred, W > 1)
    lens_d = _lens_i32(lens, dev, B, "op_score_select")
    n, tok_rs = 0, 0
    if tokens is not None:
        if not (torch.is_tensor(tokens) and tokens.is_cuda and tokens.device == dev and tokens.dim() == 2 and tokens.shape[0] == B * S):
            raise L.DimxError("op_score_select: tokens [B*S, n] on the scores' device expected")
        tokens = tokens if tokens.dtype == torch.int32 else tokens.to(torch.int32)
        n = int(tokens.shape[1])
        if tokens.stride(1) != 1 and n > 1:
            tokens = tokens.contiguous()
        tok_rs = tokens.stride(0)
    win = torch.empty(B, dtype=torch.int32, device=dev)
    ok = torch.empty(B, dtype=torch.uint8, device=dev)
    best = torch.empty(B, Ln, W, dtype=torch.float32, device=dev)
    best_tok = torch.empty(B, n, dtype=torch.int32, device=dev) if tokens is not None else None
    with torch.cuda.device(dev):
        L.check(lib.dimx_op_score_select(L.ptr(score), ctypes.c_void_p(y_pred.data_ptr()), y_pred.stride(0), y_pred.stride(1),
                                         y_pred.stride(2), L.ptr(lens_d), None if tokens is None else ctypes.c_void_p(tokens.data_ptr()),
                                         tok_rs, B, S, Ln, W, n, L.ptr(win), L.ptr(ok), L.ptr(best), L.ptr(best_tok), L.stream_ptr(dev)),
                "dimx_op_score_select")
    return (win, ok, best) if tokens is None else (win, ok, best, best_tok)


def fd_select_sweeps(device, B, S, F):
    """Jacobi sweeps of the last op_fd_select(B, S, F) call on ``device``, read from its workspace: (target factorisations [B],
    (clip, try) problems [B, S]) as int32 tensors (include/dimx.h: the last B + B*S int32 of the workspace)."""
    lib = L.load()
    need = int(lib.dimx_op_fd_select_ws_bytes(B, S, F))
    ws = _FD_WS[_device_key(device)]
    sw = ws[need - 4 * (B + B * S):need].view(torch.int32)
    return sw[:B].clone(), sw[B:].reshape(B, S).clone()


_CS_WS = {}     # device index -> uint8 workspace of op_consensus_select


def op_consensus_select(y_pred, lens, cols=(0, None), distance="fd", tokens=None, want_best=True, want_dist=False):
    """Consensus (minimum-Bayes-risk) best-of-S selection (dimx_op_consensus_select, csrc/consensus.hip; the definition is
    dimx.consensus): y_pred [B, S, L, W] f32 on a GPU, lens[j] = valid frames of clip j, cols = (c0, c1) the columns that enter the
    distance (None = the row's end), distance "fd" (the Frechet distance of op_fd_select between tries) or "l2", tokens [B*S, n]
    (optional) -> (risk [B, S] f64, win [B] int32, ok [B] uint8, best [B, L, W] f32 or None[, best_tokens [B, n] int32][, dist
    [B, S, S] f64]): per clip the try with the smallest summed distance to the others (the first minimum, NaN counting as +inf),
    ok = 0 when no risk of the clip is finite, the winner's rows (zero for t >= lens[j] and for ok = 0) and its token row (-100 for
    ok = 0).  Strides as in op_fd_select: views are passed as they are.  Asynchronous on the current stream.  CPU tensors raise:
    there is no CPU fallback (dimx.consensus.select is the host form)."""
    from .consensus import kind_index
    kind = kind_index(distance)
    if not (torch.is_tensor(y_pred) and y_pred.is_cuda):
        raise L.DimxError("op_consensus_select runs on the GPU only: y_pred must be a CUDA tensor (no CPU fallback)")
    if y_pred.dim() != 4:
        raise L.DimxError("op_consensus_select: y_pred [B, S, L, W] expected, got %s" % (tuple(y_pred.shape),))
    lib = L.load()
    dev = y_pred.device
    B, S, Ln, W = (int(v) for v in y_pred.shape)
    y_pred = _f32_rows(y_pred, W > 1)
    c0 = int(cols[0])
    F = (W if cols[1] is None else int(cols[1])) - c0
    lens_d = _lens_i32(lens, dev, B, "op_consensus_select")
    n, tok_rs = 0, 0
    if tokens is not None:
        if not (torch.is_tensor(tokens) and tokens.is_cuda and tokens.device == dev and tokens.dim() == 2 and tokens.shape[0] == B * S):
            raise L.DimxError("op_consensus_select: tokens [B*S, n] on the tries' device expected")
        tokens = tokens if tokens.dtype == torch.int32 else tokens.to(torch.int32)
        n = int(tokens.shape[1])
        if tokens.stride(1) != 1 and n > 1:
            tokens = tokens.contiguous()
        tok_rs = tokens.stride(0)
    dist = torch.empty(B, S, S, dtype=torch.float64, device=dev) if want_dist else None
    risk = torch.empty(B, S, dtype=torch.float64, device=dev)
    win = torch.empty(B, dtype=torch.int32, device=dev)
    ok = torch.empty(B, dtype=torch.uint8, device=dev)
    best = torch.empty(B, Ln, W, dtype=torch.float32, device=dev) if want_best else None
    best_tok = torch.empty(B, n, dtype=torch.int32, device=dev) if tokens is not None else None
    need = int(lib.dimx_op_consensus_select_ws_bytes(B, S, F, kind))
    ws = _workspace(_CS_WS, dev, need)
    with torch.cuda.device(dev):
        L.check(lib.dimx_op_consensus_select(ctypes.c_void_p(y_pred.data_ptr()), y_pred.stride(0), y_pred.stride(1), y_pred.stride(2),
                                             L.ptr(lens_d), B, S, Ln, W, c0, F, kind, L.ptr(dist), L.ptr(risk), L.ptr(win), L.ptr(ok),
                                             L.ptr(best), None if tokens is None else ctypes.c_void_p(tokens.data_ptr()), tok_rs, n,
                                             L.ptr(best_tok), ctypes.c_void_p(ws.data_ptr()), ws.numel(), L.stream_ptr(dev)),
                "dimx_op_consensus_select")
    out = (risk, win, ok, best)
    if tokens is not None:
        out += (best_tok,)
    if want_dist:
        out += (dist,)
    return out


def consensus_select_sweeps(device, B, S, F):
    """Jacobi sweeps of the last op_consensus_select(B, S, F, distance="fd") call on ``device``, read from its workspace: (try
    factorisations [B, S], pair problems [B, S*(S-1)/2] in the order (0,1), (0,2), .., (1,2), ..) as int32 tensors (include/dimx.h:
    the last B*S + B*S*(S-1)/2 int32 of the workspace)."""
    lib = L.load()
    need = int(lib.dimx_op_consensus_select_ws_bytes(B, S, F, 0))
    ws = _CS_WS[_device_key(device)]
    P = S * (S - 1) // 2
    sw = ws[need - 4 * (B * S + B * P):need].view(torch.int32)
    return sw[:B * S].reshape(B, S).clone(), sw[B * S:].reshape(B, P).clone()


_NS_WS = {}     # device index -> uint8 workspace of op_nn_search


def op_pool_desc(x, lens, kind):
    """Clip descriptors of the retrieval baselines (dimx_op_pool_desc, csrc/retrieval.hip; the definition is dimx.retrieval.pool):
    x [N, T, D] f32 on a GPU, lens[i] = valid frames of clip i, kind "max" (per-dimension maximum over time: NN audio) or "mean"
    (NN motion) -> (desc [N, D] f64, norm [N] f64).  The clip and frame strides are taken from the tensor (views such as
    ``src[:, :, 56:]`` are passed as they are); only a feature stride other than 1 is copied.  Asynchronous on the current stream.
    CPU tensors raise: there is no CPU fallback (dimx.retrieval.pool_batch is the host form)."""
    from .retrieval import kind_index
    k = kind_index(kind)
    if not (torch.is_tensor(x) and x.is_cuda):
        raise L.DimxError("op_pool_desc runs on the GPU only: x must be a CUDA tensor (no CPU fallback)")
    if x.dim() != 3:
        raise L.DimxError("op_pool_desc: x [N, T, D] expected, got %s" % (tuple(x.shape),))
    dev = x.device
    N, T, D = (int(v) for v in x.shape)
    x = _f32_rows(x, D > 1)
    lens_d = _lens_i32(lens, dev, N, "op_pool_desc")
    desc = torch.empty(N, D, dtype=torch.float64, device=dev)
    norm = torch.empty(N, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        L.check(L.load().dimx_op_pool_desc(ctypes.c_void_p(x.data_ptr()), x.stride(0), x.stride(1), L.ptr(lens_d), N, T, D, k,
                                           L.ptr(desc), L.ptr(norm), L.stream_ptr(dev)), "dimx_op_pool_desc")
    return desc, norm


def _f64_rows(t):
    t = t if t.dtype == torch.float64 else t.double()
    return t.contiguous() if t.shape[-1] > 1 and t.stride(-1) != 1 else t


def op_nn_search(q_desc, q_norm, x_desc, x_norm, k, want_sim=False):
    """Cosine k-nearest-neighbour search (dimx_op_nn_search, csrc/retrieval.hip; the definition is dimx.retrieval.search):
    q_desc [Q, D] / q_norm [Q] and x_desc [N, D] / x_norm [N] f64 on one GPU, 1 <= k <= 16 -> (idx [Q, k] int32, sim [Q, k] f64,
    found [Q] int32[, sim_all [Q, N] f64 with ``want_sim``]): the k library entries of largest similarity, ties to the smaller index;
    NaN and similarities <= -1 are not eligible, unfilled slots hold -1 / NaN.  Row-strided views (``x_desc[5:30]``) are passed as
    they are.  Asynchronous on the current stream.  CPU tensors raise: there is no CPU fallback."""
    ts = (q_desc, q_norm, x_desc, x_norm)
    if not all(torch.is_tensor(t) and t.is_cuda for t in ts):
        raise L.DimxError("op_nn_search runs on the GPU only: descriptors and norms must be CUDA tensors (no CPU fallback)")
    if q_desc.dim() != 2 or x_desc.dim() != 2 or q_desc.shape[1] != x_desc.shape[1] or q_norm.numel() != q_desc.shape[0] \
            or x_norm.numel() != x_desc.shape[0] or any(t.device != q_desc.device for t in ts):
        raise L.DimxError("op_nn_search: q_desc [Q, D], q_norm [Q], x_desc [N, D], x_norm [N] on one device expected, got %s"
                          % ([tuple(t.shape) for t in ts],))
    lib = L.load()
    dev = q_desc.device
    Q, D = (int(v) for v in q_desc.shape)
    N, K = int(x_desc.shape[0]), int(k)
    q_desc, x_desc = _f64_rows(q_desc), _f64_rows(x_desc)
    q_norm, x_norm = q_norm.to(torch.float64).contiguous(), x_norm.to(torch.float64).contiguous()
    idx = torch.empty(Q, max(K, 0), dtype=torch.int32, device=dev)
    sim = torch.empty(Q, max(K, 0), dtype=torch.float64, device=dev)
    found = torch.empty(Q, dtype=torch.int32, device=dev)
    sim_all = torch.empty(Q, N, dtype=torch.float64, device=dev) if want_sim else None
    ws = _workspace(_NS_WS, dev, int(lib.dimx_op_nn_search_ws_bytes(Q, N, D, K)))
    with torch.cuda.device(dev):
        L.check(lib.dimx_op_nn_search(ctypes.c_void_p(q_desc.data_ptr()), q_desc.stride(0) if Q > 1 else D, L.ptr(q_norm),
                                      ctypes.c_void_p(x_desc.data_ptr()), x_desc.stride(0) if N > 1 else D, L.ptr(x_norm), Q, N, D, K,
                                      L.ptr(idx), L.ptr(sim), L.ptr(found), L.ptr(sim_all), ctypes.c_void_p(ws.data_ptr()), ws.numel(),
                                      L.stream_ptr(dev)), "dimx_op_nn_search")
    return (idx, sim, found, sim_all) if want_sim else (idx, sim, found)


def op_nn_gather(lib_seq, lib_lens, idx, q_lens, L=None):
    """The retrieved sequences (dimx_op_nn_gather, csrc/retrieval.hip; the definition is dimx.retrieval.gather): lib_seq [N, Lmax, W]
    f32 on a GPU, lib_lens [N], idx [Q, k] int32 (-1 = no entry), q_lens [Q], L = output frames (default Lmax) -> (out [Q, k, L, W]
    f32, out_len [Q, k] int32) with out_len = min(q_lens[q], lib_lens[idx]) and zero rows at and beyond it.  Strided library views
    (a slice of a longer or wider buffer) are passed as they are.  Asynchronous on the current stream.  CPU tensors raise."""
    from . import lib as _L
    if not (torch.is_tensor(lib_seq) and lib_seq.is_cuda and torch.is_tensor(idx) and idx.is_cuda and idx.device == lib_seq.device):
        raise _L.DimxError("op_nn_gather runs on the GPU only: lib_seq / idx must be CUDA tensors on one device (no CPU fallback)")
    if lib_seq.dim() != 3 or idx.dim() != 2:
        raise _L.DimxError("op_nn_gather: lib_seq [N, Lmax, W] and idx [Q, k] expected, got %s and %s" % (tuple(lib_seq.shape),
                                                                                                         tuple(idx.shape)))
    dev = lib_seq.device
    N, Lmax, W = (int(v) for v in lib_seq.shape)
    Q, K = (int(v) for v in idx.shape)
    Lo = Lmax if L is None else int(L)
    lib_seq = _f32_rows(lib_seq, W > 1)
    idx = idx.to(torch.int32).contiguous()
    ll = _lens_i32(lib_lens, dev, N, "op_nn_gather(lib_lens)")
    ql = _lens_i32(q_lens, dev, Q, "op_nn_gather(q_lens)")
    out = torch.empty(Q, K, max(Lo, 0), W, dtype=torch.float32, device=dev)
    out_len = torch.empty(Q, K, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _L.check(_L.load().dimx_op_nn_gather(_L.ptr(idx), ctypes.c_void_p(lib_seq.data_ptr()), lib_seq.stride(0), lib_seq.stride(1),
                                             _L.ptr(ll), _L.ptr(ql), Q, K, N, Lmax, Lo, W, _L.ptr(out), _L.ptr(out_len),
                                             _L.stream_ptr(dev)), "dimx_op_nn_gather")
    return out, out_len


_MM_WS = {}      # device index -> uint8 workspace of op_mesh_metrics
_MM_MAPS = {}    # (device index, n_vert, sorted map bytes) -> MeshMap; keyed on content
_MM_LENS = {}    # device index -> the host lens array of the last call (kept until the next call has replaced it)


class MeshMap:
    """A validated vertex map on a device (mesh_map): the sorted int32 copy the kernel reads, its length, and the mesh it was checked
    against.  op_mesh_metrics takes one in place of a host sequence and then skips validation, sort and cache lookup."""
    __slots__ = ("data", "n", "n_vert", "device_key")

    def __init__(self, data, n, n_vert, device_key):
        self.data, self.n, self.n_vert, self.device_key = data, n, n_vert, device_key


def mesh_map(seq, n_vert, device, what="map"):
    """Validate a vertex map on the host (every index in [0, n_vert), DimxError otherwise) and return its MeshMap on ``device``: the
    SORTED copy is uploaded once per (device, n_vert, content) and cached."""
    if isinstance(seq, MeshMap):
        if seq.n_vert != n_vert or seq.device_key != _device_key(device):
            raise L.DimxError("op_mesh_metrics: %s was prepared for %d vertices on device %d" % (what, seq.n_vert, seq.device_key))
        return seq
    if torch.is_tensor(seq):
        seq = seq.detach().cpu().numpy()
    arr = np.asarray(seq if seq is not None else [])
    if arr.size and not np.issubdtype(arr.dtype, np.integer):
        raise L.DimxError("op_mesh_metrics: %s holds non-integer entries" % what)
    arr = arr.astype(np.int64).reshape(-1)
    if arr.size and (arr.min() < 0 or arr.max() >= n_vert):
        raise L.DimxError("op_mesh_metrics: %s holds an index outside [0, %d) (min %d, max %d)" % (what, n_vert, arr.min(), arr.max()))
    srt = np.sort(arr).astype(np.int32)
    key = _device_key(device)
    ck = (key, int(n_vert), srt.tobytes())
    hit = _MM_MAPS.get(ck)
    if hit is None:
        if len(_MM_MAPS) >= 16:      # a handful of maps per process is the use; never grow without bound
            _MM_MAPS.pop(next(iter(_MM_MAPS)))
        hit = _MM_MAPS[ck] = MeshMap(torch.from_numpy(srt).to(device) if srt.size else None, int(srt.size), int(n_vert), key)
    return hit


def op_mesh_metrics(y_true, y_pred, lens, template, mouth_map, upper_map, want_frames=False, return_status=False):
    """Lip Vertex Error / upper-Face Dynamics Deviation partials (dimx_op_mesh_metrics, csrc/mesh_metrics.hip): y_true [B, Lt, 3*Nv],
    y_pred [B, Lp, 3*Nv] f32 on one GPU (Lt, Lp >= max(lens); only the first lens[b] frames of clip b are read), lens[b] = valid
    frames (host sequence; a CUDA tensor is read back first), template [B, 3*Nv] or [3*Nv] or None (zero), mouth_map / upper_map
    host sequences of vertex indices (or their MeshMap from ``mesh_map``) -> (clip [B, 4] f64 = {sum_t max_m d, frames, sigma_gt, sigma_pred}, frame_max [B, L] f64 or
    None, with L = min(Lt, Lp)).  Clip and frame strides are taken from the tensors (``v_speaker[:, 1:]`` is passed as it is); only
    an element stride other than 1 is copied.  The maps are validated here, before any launch, and uploaded once per content as
    sorted copies.  Asynchronous on the current stream.  CPU tensors raise: there is no CPU fallback.  ``return_status=True`` appends
    the call's device status word (int32 [1]: 0; 1 = the kernel met an index outside the mesh, which the host check makes
    unreachable)."""
    if not (torch.is_tensor(y_true) and torch.is_tensor(y_pred) and y_true.is_cuda and y_pred.is_cuda):
        raise L.DimxError("op_mesh_metrics runs on the GPU only: y_true / y_pred must be CUDA tensors (no CPU fallback)")
    if y_true.dim() != 3 or y_pred.dim() != 3 or y_pred.shape[0] != y_true.shape[0] or y_pred.shape[2] != y_true.shape[2] \
            or y_pred.device != y_true.device:
        raise L.DimxError("op_mesh_metrics: y_true [B, L, 3*Nv] and y_pred [B, L', 3*Nv] on one device expected, got %s and %s"
                          % (tuple(y_true.shape), tuple(y_pred.shape)))
    B, V = int(y_true.shape[0]), int(y_true.shape[2])
    if V % 3 != 0 or V < 3:
        raise L.DimxError("op_mesh_metrics: rows of %d floats are not xyz triples" % V)
    n_vert = V // 3
    Ln = int(min(y_true.shape[1], y_pred.shape[1]))
    lib = L.load()
    dev = y_pred.device
    key = _device_key(dev)
    y_true, y_pred = _f32_rows(y_true), _f32_rows(y_pred)
    templ, templ_cs = None, 0
    if template is not None:
        if not (torch.is_tensor(template) and template.is_cuda and template.device == dev):
            raise L.DimxError("op_mesh_metrics: template must be a CUDA tensor on the meshes' device")
        templ = template if template.dtype == torch.float32 else template.float()
        if templ.dim() == 1:
            templ = templ[None].expand(B, V)
        if tuple(templ.shape) != (B, V):
            raise L.DimxError("op_mesh_metrics: template %s for meshes [%d, ., %d]" % (tuple(template.shape), B, V))
        if templ.stride(1) != 1:
            templ = templ.contiguous()
        templ_cs = templ.stride(0)
    lens_h = [int(n) for n in (lens.tolist() if torch.is_tensor(lens) else lens)]
    if len(lens_h) != B:
        raise L.DimxError("op_mesh_metrics: %d lens for %d clips" % (len(lens_h), B))
    if B < 1 or Ln < 1:
        raise L.DimxError("op_mesh_metrics: B=%d L=%d must be positive" % (B, Ln))
    mouth, upper = mesh_map(mouth_map, n_vert, dev, "mouth_map"), mesh_map(upper_map, n_vert, dev, "upper_map")
    mouth_d, n_mouth, upper_d, n_upper = mouth.data, mouth.n, upper.data, upper.n
    lens_c = (ctypes.c_int32 * B)(*lens_h)
    clip = torch.empty(B, 4, dtype=torch.float64, device=dev)
    frames = torch.empty(B, Ln, dtype=torch.float64, device=dev) if want_frames else None
    status = torch.empty(1, dtype=torch.int32, device=dev)
    need = int(lib.dimx_op_mesh_metrics_ws_bytes(B, Ln, n_mouth, n_upper))
    ws = _workspace(_MM_WS, dev, need)
    with torch.cuda.device(dev):
        L.check(lib.dimx_op_mesh_metrics(ctypes.c_void_p(y_true.data_ptr()), y_true.stride(0), y_true.stride(1),
                                         ctypes.c_void_p(y_pred.data_ptr()), y_pred.stride(0), y_pred.stride(1),
                                         None if templ is None else ctypes.c_void_p(templ.data_ptr()), templ_cs, lens_c, B, Ln, n_vert,
                                         L.ptr(mouth_d), n_mouth, L.ptr(upper_d), n_upper, L.ptr(clip), L.ptr(frames), L.ptr(status),
                                         ctypes.c_void_p(ws.data_ptr()), ws.numel(), L.stream_ptr(dev)), "dimx_op_mesh_metrics")
    _MM_LENS[key] = lens_c
    return (clip, frames, status) if return_status else (clip, frames)


# the column windows of print_metrics / print_metrics_full (reference code/mymetrics.py:7-120) as (xc0, xF, yc0, yF): the operand
# rows are [x[:, xc0:xc0+xF] | y[:, yc0:yc0+yF]]
LISTENER_WINDOWS = (("fid_pose", (0, 0, 0, 6)), ("fid_exp", (0, 0, 6, 50)), ("pfid_pose", (0, 6, 0, 6)), ("pfid_exp", (6, 50, 6, 50)),
                    ("fid", (0, 0, 0, 56)), ("pfid", (0, 56, 0, 56)))
LM_ROW = 133     # DIMX_LM_ROW of include/dimx.h
_LM_WS = {}      # device index -> uint8 workspace of op_listener_metrics


def op_listener_metrics(y_true, y_pred, x, lens, windows=tuple(w for _, w in LISTENER_WINDOWS)):
    """The listener evaluation metrics per clip (dimx_op_listener_metrics, csrc/listener_metrics.hip): y_true, y_pred [B, L, >=56],
    x [B, L', >=56] (the speaker motion) f32 on one GPU, lens[b] = valid frames of clip b, windows = rows (xc0, xF, yc0, yF)
    -> (fd [B, n_win] f64, moments [B, 133] f64; the row layout is include/dimx.h's).  Only the first min(L, L', ...) frames of
    each tensor can count.  The clip and frame strides are taken from the tensors (views such as ``tgt[:, 1:]`` are passed as they
    are); only a feature stride other than 1 is copied.  Asynchronous on the current stream.  CPU tensors raise: there is no CPU
    fallback (dimx.mymetrics.compute_metrics is the host form)."""
    ts = (y_true, y_pred, x)
    if not all(torch.is_tensor(t) and t.is_cuda for t in ts):
        raise L.DimxError("op_listener_metrics runs on the GPU only: y_true / y_pred / x must be CUDA tensors (no CPU fallback)")
    if any(t.dim() != 3 or t.shape[0] != y_pred.shape[0] or t.device != y_pred.device for t in ts) or y_true.shape[2] != y_pred.shape[2]:
        raise L.DimxError("op_listener_metrics: y_true, y_pred [B, L, W] and x [B, L, Wx] on one device expected, got %s, %s and %s"
                          % tuple(tuple(t.shape) for t in ts))
    lib = L.load()
    dev = y_pred.device
    B, Ln = int(y_pred.shape[0]), int(min(t.shape[1] for t in ts))
    y_true, y_pred, x = [_f32_rows(t) for t in ts]
    win = [tuple(int(v) for v in w) for w in windows]
    if any(len(w) != 4 for w in win):
        raise L.DimxError("op_listener_metrics: windows are rows (xc0, xF, yc0, yF), got %r" % (windows,))
    n_win = len(win)
    win_c = (ctypes.c_int32 * (4 * max(n_win, 1)))(*[v for w in win for v in w])
    lens_d = _lens_i32(lens, dev, B, "op_listener_metrics")
    fd = torch.empty(B, n_win, dtype=torch.float64, device=dev)
    mom = torch.empty(B, LM_ROW, dtype=torch.float64, device=dev)
    need = int(lib.dimx_op_listener_metrics_ws_bytes(B, n_win, max([w[1] + w[3] for w in win] or [0])))
    ws = _workspace(_LM_WS, dev, need)
    with torch.cuda.device(dev):
        L.check(lib.dimx_op_listener_metrics(ctypes.c_void_p(y_true.data_ptr()), y_true.stride(0), y_true.stride(1),
                                             ctypes.c_void_p(y_pred.data_ptr()), y_pred.stride(0), y_pred.stride(1),
                                             ctypes.c_void_p(x.data_ptr()), x.stride(0), x.stride(1), L.ptr(lens_d), B, Ln,
                                             int(y_pred.shape[2]), int(x.shape[2]), win_c, n_win, L.ptr(fd), L.ptr(mom),
                                             ctypes.c_void_p(ws.data_ptr()), ws.numel(), L.stream_ptr(dev)), "dimx_op_listener_metrics")
    return fd, mom


def listener_metrics_sweeps(device, B, n_win, F):
    """Jacobi sweeps of the last op_listener_metrics call of these sizes on ``device`` (F = its widest window), read from its
    workspace: (target factorisations, candidate problems), each int32 [n_win, B] (include/dimx.h)."""
    lib = L.load()
    need = int(lib.dimx_op_listener_metrics_ws_bytes(B, n_win, F))
    ws = _LM_WS[_device_key(device)]
    sw = ws[need - 8 * B * n_win:need].view(torch.int32).reshape(2, n_win, B)
    return sw[0].clone(), sw[1].clone()


# ---------------------------------------------------------------- SID: float64 KMeans fit + assign (csrc/kmeans_sid.hip)
_KM_WS = {}      # device index -> uint8 workspace of op_kmeans_fit


def _km_frames(frames, cols, what):
    if not (torch.is_tensor(frames) and frames.is_cuda):
        raise L.DimxError("%s runs on the GPU only: frames must be a CUDA tensor (no CPU fallback; dimx.mymetrics.sid_f64 is the "
                          "host form)" % what)
    if frames.dim() != 2:
        raise L.DimxError("%s: frames [N, W] expected, got %s" % (what, tuple(frames.shape)))
    frames = frames if frames.dtype == torch.float32 else frames.float()
    if frames.stride(1) != 1 or (frames.shape[0] > 1 and frames.stride(0) < frames.shape[1]):
        frames = frames.contiguous()
    c0 = int(cols[0])
    c1 = int(frames.shape[1]) if cols[1] is None else int(cols[1])
    return frames, c0, c1 - c0


def kmeans_empty_cluster_error(status, what="op_kmeans_fit"):
    return L.DimxError("%s: a cluster was left without a frame at Lloyd iteration %d; scikit-learn relocates such a centre and the "
                       "operator does not restate that -- the host form is dimx.mymetrics.calcuate_sid" % (what, int(status)))


def op_kmeans_fit(frames, k, cols=(0, None), seed=0, tol=1e-4, max_iter=300, want_labels=False, check=True):
    """KMeans(k, random_state=seed, n_init='auto').fit of scikit-learn on float64 copies of the f32 frames (dimx_op_kmeans_fit,
    csrc/kmeans_sid.hip; the definition is dimx.mymetrics.kmeans_fit_f64): frames [N, W] f32 on a GPU (the row stride is taken from
    the tensor), cols = (c0, c1) the columns that enter -> (centers [k, c1 - c0] f64 on that GPU, n_iter).  The random numbers of the
    initialisation are drawn here (mymetrics.kmeans_draws) and uploaded; the fit itself is enqueued as a whole on the current
    stream.  ``check=True`` reads the status word back (one synchronisation) and raises DimxError when a cluster was left empty;
    ``check=False`` returns (centers, info) with info = int32 [2] {n_iter, status} on the GPU and synchronises nothing.
    ``want_labels=True`` appends the int32 [N] assignment the returned means were taken over.  CPU tensors raise: no CPU fallback."""
    from .mymetrics import kmeans_draws
    frames, c0, F = _km_frames(frames, cols, "op_kmeans_fit")
    lib = L.load()
    dev = frames.device
    N, W, k = int(frames.shape[0]), int(frames.shape[1]), int(k)
    if k < 1 or N < k:
        raise L.DimxError("op_kmeans_fit: %d frames for %d clusters" % (N, k))
    first, U = kmeans_draws(N, k, seed)
    U_d = torch.from_numpy(np.ascontiguousarray(U)).to(dev) if U.size else None
    centers = torch.empty(k, max(F, 0), dtype=torch.float64, device=dev)
    info = torch.zeros(2, dtype=torch.int32, device=dev)
    labels = torch.empty(N, dtype=torch.int32, device=dev) if want_labels else None
    need = int(lib.dimx_op_kmeans_fit_ws_bytes(N, k, F))
    ws = _workspace(_KM_WS, dev, need, floor=256)
    with torch.cuda.device(dev):
        L.check(lib.dimx_op_kmeans_fit(ctypes.c_void_p(frames.data_ptr()), frames.stride(0) if N > 1 else W, N, W, c0, F, k, first,
                                       L.ptr(U_d), int(U.shape[1]), float(tol), int(max_iter), L.ptr(centers),
                                       ctypes.c_void_p(info.data_ptr()), ctypes.c_void_p(info.data_ptr() + 4), L.ptr(labels),
                                       ctypes.c_void_p(ws.data_ptr()), ws.numel(), L.stream_ptr(dev)), "dimx_op_kmeans_fit")
    if check:
        n_iter, status = info.tolist()
        if status:
            raise kmeans_empty_cluster_error(status)
        info = n_iter
    return (centers, info, labels) if want_labels else (centers, info)


def op_sid_assign(frames, centers, cols=(0, None), want_labels=False):
    """Nearest centre (the first index on ties) of every frame, the histogram and its entropy (dimx_op_sid_assign,
    csrc/kmeans_sid.hip): frames [M, W] f32 on a GPU, centers [K, c1 - c0] f64 on it, cols = (c0, c1) -> (hist int64 [K],
    sid f64 [1] = -sum h log2(h + 1e-6)), with ``want_labels`` also the int32 [M] labels.  Asynchronous on the current stream.  CPU
    tensors raise: there is no CPU fallback."""
    frames, c0, F = _km_frames(frames, cols, "op_sid_assign")
    if not (torch.is_tensor(centers) and centers.is_cuda and centers.device == frames.device and centers.dim() == 2):
        raise L.DimxError("op_sid_assign: centers [K, F] must be a CUDA tensor on the frames' device")
    if centers.shape[1] != F:
        raise L.DimxError("op_sid_assign: centers of %d columns for a window of %d" % (centers.shape[1], F))
    lib = L.load()
    dev = frames.device
    M, W, K = int(frames.shape[0]), int(frames.shape[1]), int(centers.shape[0])
    centers = centers.to(torch.float64).contiguous()
    hist = torch.empty(K, dtype=torch.int64, device=dev)
    sid = torch.empty(1, dtype=torch.float64, device=dev)
    labels = torch.empty(M, dtype=torch.int32, device=dev) if want_labels else None
    with torch.cuda.device(dev):
        L.check(lib.dimx_op_sid_assign(ctypes.c_void_p(frames.data_ptr()), frames.stride(0) if M > 1 else W, M, W, c0, F,
                                       L.ptr(centers), K, L.ptr(hist), L.ptr(sid), L.ptr(labels), L.stream_ptr(dev)),
                "dimx_op_sid_assign")
    return (hist, sid, labels) if want_labels else (hist, sid)
