"""Training step of the DIM-Listener fine-tuning model on hand-written HIP kernels.

Reference: ``train_epoch`` (code/x_engine_pt.py:9-60) as driven by code/finetune_s2s_pretrain.py:105-143 -- AdamW
(lr 1e-5), gradient clipping at 1.0, both VQ-VAEs frozen.  The reference differentiates ``SLMFT.forward(mode='train')``
with autograd; here the forward AND the backward pass of the teacher-forced stack run in libdimx_hip.so
(csrc/train.hip, csrc/train_kernels.hip): every Linear and both of its adjoints on the library's MFMA GEMM, attention /
LayerNorm / GELU / cross-entropy adjoints as HIP kernels, fused clip + AdamW.  ``dimx.train`` (the PyTorch-autograd
restatement of round 2) stays as the CHECKER of this path (tests/test_gpu_train_hip.py) and as the CPU fallback-free
reference of the gradient math; it is no longer what ``x_engine_pt.train_epoch`` runs on a GPU.

State: parameters, gradients and the two AdamW moments are four flat f32 device tensors laid out by the library
(``dimx_train_param_info``); the module's ``nn.Parameter``s are written back by ``sync_to_model()`` (end of an epoch,
before evaluation or ``state_dict()``).  Multi-GPU: one process per GPU, replicated weights, per-rank batch shard, and
ONE all-reduce of the flat gradient tensor per step over RCCL (xGMI rings are per-link bound: one 0.4 GB collective
instead of one per tensor)."""
import ctypes

import torch

from . import dist as ddist
from . import lib as L


class HipTrainer:
    # what a step's trainer states about its entry points in libdimx_hip.so (include/dimx.h)
    _ABI = "dimx_train"                          # <_ABI>_num_params / _param_info / _total report the arena layout
    _SIZER = "dimx_train_workspace_bytes"        # the step's sizing function
    _LOSS_FLOATS = 2                             # floats the step writes to loss_out
    _UNGRAPHED = None                            # name of a step that is launched kernel by kernel (no graph_stats)

    def __init__(self, model, lr=1e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, clip=1.0, device=None, lookahead=None,
                 cond_drop=0.0, seed=20260928):
        """AdamW defaults are torch.optim.AdamW's (the reference passes only lr, code/finetune_s2s_pretrain.py:119).
        lookahead: online fine-tuning (``set_lookahead``); None = the offline step of the reference.
        cond_drop: condition dropout (dimx_set_train_cond_keep; the definition is dimx.guidance): every step trains each clip under
        the null context with this probability, drawn by ``dimx.guidance.cond_keep(seed, step, B, cond_drop)``; 0 = off, the
        plain step launch for launch.  Only the SLMFT step (this class itself) takes it."""
        self.model = model
        self.lookahead = None
        self.cond_drop, self.cond_seed = float(cond_drop), int(seed)   # not .seed: the VQ-VAE trainer's dropout seed is a subclass's
        self._keep = None
        if self.cond_drop > 0 and type(self) is not HipTrainer:
            raise L.DimxError("cond_drop: only the SLMFT fine-tuning step (HipTrainer) takes condition dropout")
        self.device = torch.device(device if device is not None else next(model.parameters()).device)
        if self.device.type != "cuda":
            raise L.DimxError("HipTrainer needs the module on a ROCm GPU (model.to('cuda:0')); there is no CPU path")
        self.lr, self.betas, self.eps, self.weight_decay, self.clip = lr, betas, eps, weight_decay, clip
        self.lib = L.load()
        self.eng = model.engine(self.device)
        self.total, self.layout = self._arena_layout(self.eng.h)
        kw = dict(dtype=torch.float32, device=self.device)
        self.params = torch.zeros(self.total, **kw)
        self.grads = torch.zeros(self.total, **kw)
        self.exp_avg = torch.zeros(self.total, **kw)
        self.exp_avg_sq = torch.zeros(self.total, **kw)
        self._scratch = torch.zeros(1026, **kw)
        self._loss = torch.zeros(self._LOSS_FLOATS, **kw)
        self._ws, self._ws_bytes = None, 0
        self._stage = {}
        self.step_count = 0
        self.load_from_model()
        if lookahead is not None:
            self.set_lookahead(lookahead)
        if ddist.world_size() > 1:                      # every rank starts from rank 0's parameters
            import torch.distributed as dist
            dist.broadcast(self.params, 0)

    def _abi_args(self):
        """what the layout functions take after the handle"""
        return ()

    def _arena_layout(self, h):
        """(floats per arena, [(name, offset, numel)]) of the step's flat arenas, as the library lays them out"""
        args = (h,) + self._abi_args()
        n = getattr(self.lib, self._ABI + "_num_params")(*args)
        if n <= 0:
            L.check(n, self._ABI + "_num_params")
        param_info = getattr(self.lib, self._ABI + "_param_info")
        layout = []
        for i in range(n):
            name, off, numel = ctypes.c_char_p(), ctypes.c_int64(), ctypes.c_int64()
            L.check(param_info(*args, i, ctypes.byref(name), ctypes.byref(off), ctypes.byref(numel)), self._ABI + "_param_info")
            layout.append((name.value.decode(), int(off.value), int(numel.value)))
        return int(getattr(self.lib, self._ABI + "_total")(*args)), layout

    # ------------------------------------------------------------------ arena <-> module
    def _named(self):
        return dict(self.model.named_parameters())

    def _versions(self):
        named = self._named()
        return tuple(int(named[name]._version) for name, _, _ in self.layout)

    def load_from_model(self):
        named = self._named()
        with torch.no_grad():
            for name, off, numel in self.layout:
                self.params[off:off + numel].copy_(named[name].detach().reshape(-1).to(self.device, torch.float32))
        self._synced_versions = self._versions()

    def refresh_from_model_if_changed(self):
        """the arenas are the master copy between ``sync_to_model()`` calls; if somebody wrote the module's parameters in the
        meantime (``load_state_dict`` of a checkpoint, a manual re-initialisation), adopt them instead of overwriting them at the
        end of the next epoch.  Detected through the tensors' version counters.  Returns True when the arena was reloaded."""
        if getattr(self, "_synced_versions", None) == self._versions():
            return False
        self.load_from_model()
        return True

    def sync_to_model(self):
        """write the trained parameters back into the nn.Module (its engine re-packs them before its next launch)."""
        named = self._named()
        with torch.no_grad():
            for name, off, numel in self.layout:
                p = named[name]
                p.copy_(self.params[off:off + numel].view_as(p))
        self._synced_versions = self._versions()

    # ------------------------------------------------------------------ torch.optim.AdamW <-> arenas
    def import_optimizer_state(self, optimizer):
        """adopt the moments / step count a torch.optim.AdamW already holds for the trained parameters (resuming from an
        ``optimizer.load_state_dict``); parameters without state start from zero moments like a fresh AdamW."""
        named = self._named()
        step = 0
        with torch.no_grad():
            for name, off, numel in self.layout:
                st = optimizer.state.get(named[name])
                if not st:
                    # no state = a fresh AdamW for this parameter: ZERO moments, not whatever the arena held (a cleared
                    # optimizer.state or a reload after an interrupted epoch resumed on stale moments)
                    self.exp_avg[off:off + numel].zero_()
                    self.exp_avg_sq[off:off + numel].zero_()
                    continue
                self.exp_avg[off:off + numel].copy_(st["exp_avg"].reshape(-1).to(self.device, torch.float32))
                self.exp_avg_sq[off:off + numel].copy_(st["exp_avg_sq"].reshape(-1).to(self.device, torch.float32))
                step = max(step, int(st["step"]))
        # the optimizer is the authority at this point (a freshly loaded state_dict may carry a SMALLER step count than the
        # arenas' last one): take its count, not the maximum
        self.step_count = step
        self._state_sig = self._optimizer_state_signature(optimizer)

    def _optimizer_state_signature(self, optimizer):
        """identity + version of the moment tensors torch keeps for the trained parameters: changes when optimizer.load_state_dict
        replaced them or an autograd epoch stepped them in place since the last import / export"""
        named = self._named()
        sig = []
        for name, _, _ in self.layout:
            st = optimizer.state.get(named[name])
            if st and "exp_avg" in st:
                sig.append((id(st["exp_avg"]), st["exp_avg"]._version, id(st["exp_avg_sq"]), st["exp_avg_sq"]._version))
            else:
                sig.append(None)
        return sig

    def optimizer_state_changed(self, optimizer):
        return getattr(self, "_state_sig", None) != self._optimizer_state_signature(optimizer)

    def export_optimizer_state(self, optimizer):
        """write the moments and the step count into ``optimizer.state`` (the entries torch.optim.AdamW keeps per parameter), so
        ``optimizer.state_dict()`` / a later autograd epoch continue from what the HIP steps left."""
        named = self._named()
        with torch.no_grad():
            for name, off, numel in self.layout:
                p = named[name]
                st = optimizer.state[p]
                for key, arena in (("exp_avg", self.exp_avg), ("exp_avg_sq", self.exp_avg_sq)):
                    src = arena[off:off + numel].view_as(p)
                    if key in st and st[key].shape == p.shape and st[key].device == p.device:
                        st[key].copy_(src)
                    else:
                        st[key] = src.to(p.device, copy=True)
                st["step"] = torch.tensor(float(self.step_count))
        self._state_sig = self._optimizer_state_signature(optimizer)

    def view(self, arena, name):
        for n, off, numel in self.layout:
            if n == name:
                return arena[off:off + numel].view(self._named()[name].shape)
        raise KeyError(name)

    def grad(self, name):
        return self.view(self.grads, name)

    # ------------------------------------------------------------------ one step
    def _workspace(self, B, T):
        """(256-byte aligned workspace pointer, its bytes) for one step at (B, T); grown when the step needs more"""
        need = int(getattr(self.lib, self._SIZER)(self.eng.h, B, T))
        if need == 0:
            raise L.DimxError("%s(B=%d, T=%d) = 0: %s" % (self._SIZER, B, T, (self.lib.dimx_last_error() or b"").decode()))
        if need > self._ws_bytes:
            self._ws = torch.empty(need + 256, dtype=torch.uint8, device=self.device)
            self._ws_bytes = need
        base = self._ws.data_ptr()
        return ctypes.c_void_p((base + 255) // 256 * 256), self._ws.numel() - 256

    def _staging(self, B, T, d_s, d_a):
        st = self._stage.get((B, T, d_s, d_a))
        if st is None:
            kw = dict(device=self.device)
            st = {"v_s": torch.empty(B, T, d_s, dtype=torch.float32, **kw), "v_a": torch.empty(B, T, d_a, dtype=torch.float32, **kw),
                  "mask": torch.empty(B, T, dtype=torch.uint8, **kw), "z": torch.empty(B, T, dtype=torch.int32, **kw),
                  "kv": torch.empty(B, T - 1, dtype=torch.uint8, **kw)}
            box = {}

            def logits():
                if "t" not in box:
                    box["t"] = torch.empty(B, T - 1, 512, dtype=torch.float32, **kw)
                return box["t"]
            st["logits"] = logits
            if len(self._stage) >= 8:          # a handful of (B, T) buckets; ragged epochs do not grow it without bound
                self._stage.pop(next(iter(self._stage)))
            self._stage[(B, T, d_s, d_a)] = st
        return st

    def set_lookahead(self, lookahead=None):
        """Online fine-tuning (dimx_set_train_lookahead; the definition is dimx.online): with an integer ``lookahead`` L the
        decoder's cross attention of every following step lets row t see the context rows j < visible(t, L, T) only -- what an
        online generation with the same L (``SLMFT.generate(lookahead=L)``) shows step t.  None: the offline step.  The setting is
        the trainer's; it is written to the engine handle before each step, so trainers that share a model do not disturb each
        other.  Only the SLMFT step (this class itself) takes it."""
        if lookahead is not None and type(self) is not HipTrainer:
            raise L.DimxError("set_lookahead: only the SLMFT fine-tuning step (HipTrainer) trains under the online window")
        if lookahead is not None:                       # refused by the library for a handle of another variant
            L.check(self.lib.dimx_set_train_lookahead(self.eng.h, 1, int(lookahead)), "dimx_set_train_lookahead")
        self.lookahead = None if lookahead is None else int(lookahead)

    def _apply_lookahead(self):
        la = self.lookahead
        L.check(self.lib.dimx_set_train_lookahead(self.eng.h, 0 if la is None else 1, 0 if la is None else la), "dimx_set_train_lookahead")

    def _apply_cond_keep(self, B, cond_keep):
        """the step's keep vector: the given one ([B] bool / 0-1), else this step's draw when ``cond_drop`` > 0, else off.  It lives
        in one persistent device vector: its address keys the captured step, its contents do not."""
        if cond_keep is None and self.cond_drop > 0:
            from . import guidance
            cond_keep = guidance.cond_keep(self.cond_seed, self.step_count, B, self.cond_drop)
        if cond_keep is None:
            L.check(self.lib.dimx_set_train_cond_keep(self.eng.h, None), "dimx_set_train_cond_keep")
            return
        if self._keep is None or self._keep.numel() < B:
            self._keep = torch.ones(max(B, 256), dtype=torch.uint8, device=self.device)
        self._keep[:B].copy_(torch.as_tensor(cond_keep).reshape(B).to(torch.uint8), non_blocking=True)
        L.check(self.lib.dimx_set_train_cond_keep(self.eng.h, L.ptr(self._keep)), "dimx_set_train_cond_keep")

    def graph_stats(self):
        """(steps replayed from the captured hipGraph, steps launched kernel by kernel, nodes of the captured graph)"""
        if self._UNGRAPHED:
            raise L.DimxError("the %s step is launched kernel by kernel (no captured graph)" % self._UNGRAPHED)
        out = (ctypes.c_int64 * 3)()
        L.check(self.lib.dimx_train_graph_stats(self.eng.h, ctypes.cast(out, ctypes.c_void_p)), "dimx_train_graph_stats")
        return int(out[0]), int(out[1]), int(out[2])

    def forward_backward(self, v_speaker, v_listener, v_audio, mask, kv_mask=None, z_l=None, return_logits=False, _alias_logits=False,
                         cond_keep=None):
        """loss (0-dim device tensor, mean cross entropy over the valid listener codes) and the gradients in ``self.grads``.
        cond_keep: [B] keep flags of the condition dropout for this step (None: the trainer's own draw, or off).
        kv_mask: keep-mask [B,T-1] of the mask_prob draw; None draws one like the reference, False disables it.
        return_logits: a tensor of the caller's own (the step writes into a staging buffer that the next call with the same (B, T)
        overwrites -- possibly from a hipGraph replay; only train_step, which consumes the logits at once, takes the alias)."""
        mask = mask.bool()
        B, T = mask.shape
        if z_l is None:
            with torch.no_grad():
                _, z_l = self.model.forward_vq(v_speaker, v_listener, mask, with_speaker=False)
        if kv_mask is None:
            kv_mask = self.model.draw_kv_mask(B, T, self.device)
        elif kv_mask is False:
            kv_mask = None
        # the batch is staged in buffers that persist per (B, T): a call whose pointers equal the previous call's is replayed
        # from the captured hipGraph of the step (dimx_train_forward_backward), fresh tensors every step would keep it on the
        # kernel-by-kernel path
        st = self._staging(B, T, int(v_speaker.shape[-1]), int(v_audio.shape[-1]))
        v_s, v_a, m8, z32 = st["v_s"], st["v_a"], st["mask"], st["z"]
        v_s.copy_(v_speaker, non_blocking=True)
        v_a.copy_(v_audio, non_blocking=True)
        m8.copy_(mask, non_blocking=True)
        z32.copy_(z_l, non_blocking=True)
        kv8 = None
        if kv_mask is not None:
            kv8 = st["kv"]
            kv8.copy_(kv_mask, non_blocking=True)
        logits = st["logits"]() if return_logits else None
        ws, wsb = self._workspace(B, T)
        self._apply_lookahead()
        self._apply_cond_keep(B, cond_keep)
        L.check(self.lib.dimx_train_forward_backward(self.eng.h, L.ptr(self.params), L.ptr(self.grads), L.ptr(v_s), L.ptr(v_a),
                                                     L.ptr(m8), L.ptr(z32), L.ptr(kv8), B, T, L.ptr(self._loss), L.ptr(logits), ws,
                                                     wsb, L.stream_ptr(self.device)), "dimx_train_forward_backward")
        loss = self._loss[0].clone()
        if return_logits and not _alias_logits:
            logits = logits.clone()
        return (loss, logits) if return_logits else loss

    def all_reduce_grads(self):
        world = ddist.world_size()
        if world > 1:
            import torch.distributed as dist
            dist.all_reduce(self.grads)
            self.grads.div_(world)

    def step(self):
        """clip (torch.nn.utils.clip_grad_norm_ semantics) + AdamW; returns the gradient norm before clipping (device scalar)."""
        self.step_count += 1
        L.check(self.lib.dimx_train_adamw(L.ptr(self.params), L.ptr(self.grads), L.ptr(self.exp_avg), L.ptr(self.exp_avg_sq),
                                          self.total, float(self.lr), float(self.betas[0]), float(self.betas[1]), float(self.eps),
                                          float(self.weight_decay), self.step_count, float(self.clip or 0.0), L.ptr(self._scratch),
                                          L.stream_ptr(self.device)), "dimx_train_adamw")
        return self._scratch[1024]

    def train_step(self, v_speaker, v_listener, v_audio, mask, kv_mask=None, z_l=None, with_cont_loss=False):
        """one optimisation step; returns l_ce_l (device scalar), or (total, dict) like SLMFT.forward(mode='train') when
        with_cont_loss: the reference's total also carries the continuous loss of the decoded arg-max codes, which has no
        gradient path (code/seq2seq_pretrain.py:454-478) -- it is evaluated from this step's logits on the HIP engine."""
        if not with_cont_loss:
            loss = self.forward_backward(v_speaker, v_listener, v_audio, mask, kv_mask=kv_mask, z_l=z_l)
            self.all_reduce_grads()
            self.step()
            return loss
        l_ce, logits = self.forward_backward(v_speaker, v_listener, v_audio, mask, kv_mask=kv_mask, z_l=z_l, return_logits=True,
                                             _alias_logits=True)
        self.all_reduce_grads()
        self.step()
        with torch.no_grad():
            pred = self.model.forward_vq_decoder(logits, mode="train")
            l_cont = self.model.forward_continuous_loss(pred, v_listener.to(self.device), mask.bool().to(self.device))
        return l_ce + l_cont, {"l_ce_s": 0, "l_ce_l": l_ce, "l_cont_s": 0, "l_cont_l": l_cont, "nce": 0, "c_acc": 0}


class LegacyHipTrainer(HipTrainer):
    """The legacy ListenerGenerator's training step on the HIP kernels (reference loop code/x_engine.py:8-36):
    the generator (bidirectional encoder, decoder with absolute positions), the listener-id conditioning and the listener
    VQ-VAE's DECODER train; the frozen halves (speaker features, listener codes) come from the engine without a graph.  Same
    flat arenas, clip + AdamW and gradient all-reduce as HipTrainer; ``dimx.train.legacy_loss`` (PyTorch autograd) is its checker
    (tests/test_gpu_train_legacy.py)."""

    _SIZER = "dimx_train_legacy_workspace_bytes"
    _LOSS_FLOATS = 4

    def forward_backward(self, v_speaker, v_listener, mask, listener_ids=None, return_logits=False):
        """-> (total loss = cross entropy + continuous loss, dict, pred [B,T-1,56][, logits]); gradients in ``self.grads``."""
        m = self.model
        mask = mask.bool()
        B, T = mask.shape
        with torch.no_grad():
            eng, xs, xl, lens, m8 = m._prepare(v_speaker, v_listener, mask)
            z_l = eng.vq_encode(1, xl, lens, pe_mode=0, pad_value=-100).to(torch.int32).contiguous()
            x_speaker = eng.legacy_speaker_features(xs, m8).float().contiguous().clone()
        v_l = v_listener.to(self.device, torch.float32).contiguous()
        ids = listener_ids.to(self.device, torch.int32).contiguous() if listener_ids is not None else None
        book = m.listener_vq.quantize.embedding.weight.detach().to(self.device, torch.float32).contiguous()
        pe = m.listener_vq.decoder.decoder_pos_embedding.pe.detach().to(self.device, torch.float32).contiguous()
        nd = T if ids is not None else T - 1
        pred = torch.empty(B, T - 1, 56, dtype=torch.float32, device=self.device)
        logits = torch.empty(B, nd, 512, dtype=torch.float32, device=self.device) if return_logits else None
        ws, wsb = self._workspace(B, T)
        L.check(self.lib.dimx_train_legacy_forward_backward(
            self.eng.h, L.ptr(self.params), L.ptr(self.grads), L.ptr(x_speaker), L.ptr(z_l), L.ptr(v_l), L.ptr(m8), L.ptr(ids), L.ptr(book),
            L.ptr(pe), B, T, L.ptr(self._loss), L.ptr(pred), L.ptr(logits), ws, wsb, L.stream_ptr(self.device)),
            "dimx_train_legacy_forward_backward")
        l_ce, l_cont = self._loss[0].clone(), self._loss[2].clone()
        out = (l_ce + l_cont, {"l_ce": l_ce, "l_cont": l_cont}, pred)
        return out + (logits,) if return_logits else out

    def train_step(self, v_speaker, v_listener, mask, listener_ids=None):
        """one optimisation step of the reference loop's body; returns (loss, pred) like ``model(src, tgt, mask, listener_ids=...)``."""
        loss, _, pred = self.forward_backward(v_speaker, v_listener, mask, listener_ids=listener_ids)
        self.all_reduce_grads()
        self.step()
        return loss, pred


class SlmHipTrainer(HipTrainer):
    """The SLM pre-training step on the HIP kernels (reference loop code/train_s2s_pretrain.py:41-64 ->
    x_engine_pt.train_epoch over SLM.forward, code/seq2seq_pretrain.py:300-323): the three encoders (the joint one over the 2T
    concatenation and over each stream, one pass), InfoNCE, the decoder for both streams (one pass over 2B sequences), both cross
    entropies and the continuous losses through BOTH VQ-VAE decoders, which train.  The frozen VQ encoders run on the inference
    engine.  Same flat arenas, clip + AdamW and gradient all-reduce as HipTrainer; ``dimx.train.slm_loss`` (PyTorch autograd) is
    its checker (tests/test_gpu_train_slm.py)."""

    _SIZER = "dimx_train_slm_workspace_bytes"
    _LOSS_FLOATS = 10
    KEYS = ("l_ce_s", "l_ce_l", "l_cont_s", "l_cont_l", "nce", "c_acc")

    def _frozen(self):
        m = self.model
        c = getattr(self, "_frozen_cache", None)
        if c is None:
            f = lambda t: t.detach().to(self.device, torch.float32).contiguous()
            c = (f(m.speaker_vq.quantize.embedding.weight), f(m.listener_vq.quantize.embedding.weight),
                 f(m.speaker_vq.decoder.decoder_pos_embedding.pe), f(m.listener_vq.decoder.decoder_pos_embedding.pe))
            self._frozen_cache = c
        return c

    def forward_backward(self, v_speaker, v_listener, v_audio, mask, mask_speaker=None, mask_listener=None, z_s=None, z_l=None,
                         mask_ratio=0.15):
        """-> (total loss, dict of the reference's six entries) as device scalars; gradients in ``self.grads``.  mask_speaker /
        mask_listener (True = frame masked out) are drawn like the reference when not given."""
        m = self.model
        mask = mask.bool()
        B, T = mask.shape
        with torch.no_grad():
            if z_s is None or z_l is None:
                z_s, z_l = m.forward_vq(v_speaker, v_listener, mask)
            if mask_speaker is None:
                mask_speaker = m.random_masking_unstructured(v_speaker, mask, mask_ratio)
            if mask_listener is None:
                mask_listener = m.random_masking_unstructured(v_listener, mask, mask_ratio)
        f = lambda t: t.to(self.device, torch.float32).contiguous()
        u8 = lambda t: t.to(self.device).to(torch.uint8).contiguous()
        i32 = lambda t: t.to(self.device).to(torch.int32).contiguous()
        v_s, v_l, v_a = f(v_speaker), f(v_listener), f(v_audio)
        m8, ms8, ml8, zs, zl = u8(mask), u8(mask_speaker), u8(mask_listener), i32(z_s), i32(z_l)
        book_s, book_l, pe_s, pe_l = self._frozen()
        ws, wsb = self._workspace(B, T)
        L.check(self.lib.dimx_train_slm_forward_backward(
            self.eng.h, L.ptr(self.params), L.ptr(self.grads), L.ptr(v_s), L.ptr(v_l), L.ptr(v_a), L.ptr(m8), L.ptr(ms8), L.ptr(ml8),
            L.ptr(zs), L.ptr(zl), L.ptr(book_s), L.ptr(book_l), L.ptr(pe_s), L.ptr(pe_l), B, T, L.ptr(self._loss), ws, wsb,
            L.stream_ptr(self.device)), "dimx_train_slm_forward_backward")
        out = self._loss.clone()
        d = {"l_ce_s": out[0], "l_ce_l": out[2], "l_cont_s": out[4], "l_cont_l": out[6], "nce": out[8], "c_acc": out[9]}
        return out[0] + out[2] + out[4] + out[6] + out[8], d

    def train_step(self, v_speaker, v_listener, v_audio, mask, with_cont_loss=True, **kw):
        """one optimisation step of the reference loop's body; returns (total, d) like ``SLM.forward`` (its third value is None)."""
        total, d = self.forward_backward(v_speaker, v_listener, v_audio, mask, **kw)
        self.all_reduce_grads()
        self.step()
        return total, d


class VqHipTrainer(HipTrainer):
    """The VQ-VAE's own training step (stage 1) on the HIP kernels: reference loop code/train_vq.py:173-196 -- out, quant_loss,
    info = model(data); calc_vq_loss; AdamW(lr 1e-4, torch's default weight decay 0.01, no clipping) -- over every parameter of
    ``dimx.models.VQAutoEncoder`` (encoder, decoder, codebook).  Forward AND backward run in libdimx_hip.so (csrc/train.hip
    vq_run, csrc/train_vq.hip); the module's own encode / decode stay inference-only and see the trained weights after
    ``sync_to_model()``.  ``dropout``: the PositionalEncoding's Dropout of the reference's train mode, with a counter-based keep
    mask of (seed, step, site, b, t, c) (``dimx.prng.dropout_keep``) instead of torch's RNG; 0 = deterministic eval-mode step.
    Same flat arenas, AdamW, optimiser-state import / export and gradient all-reduce as HipTrainer; ``dimx.train.vq_loss``
    (PyTorch autograd) is its checker (tests/test_gpu_train_vq.py)."""

    _ABI = "dimx_train_vq"
    _SIZER = "dimx_train_vq_workspace_bytes"
    _LOSS_FLOATS = 4
    _UNGRAPHED = "VQ-VAE"

    def __init__(self, model, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, clip=0.0, dropout=0.1, seed=20260928,
                 beta=0.25, quant_loss_weight=1.0, device=None):
        self.which = int(getattr(model, "which", 1))
        self.prefix = "listener_vq." if self.which == 1 else "speaker_vq."
        self.dropout, self.seed = float(dropout), int(seed)
        self.beta, self.quant_loss_weight = float(beta), float(quant_loss_weight)
        super().__init__(model, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, clip=clip, device=device)

    def _abi_args(self):
        return (self.which,)

    def _named(self):
        # the library names the slot's tensors with their prefix (the handle holds both VQ-VAE slots); the module's are unprefixed
        return {self.prefix + n: p for n, p in self.model.named_parameters()}

    def forward_backward(self, x, step=None, dropout=None):
        """x [B,T,56] -> ({loss, rec_loss, quant_loss, perplexity} device scalars, pred [B,T,56], idx [B*T] int32); gradients in
        ``self.grads``.  step: the dropout mask's step counter (default: optimiser steps taken so far); dropout: override p."""
        x = x.to(self.device, torch.float32).contiguous()
        B, T, _ = x.shape
        ws, wsb = self._workspace(B, T)
        pred = torch.empty(B, T, x.shape[-1], dtype=torch.float32, device=self.device)
        idx = torch.empty(B * T, dtype=torch.int32, device=self.device)
        p = self.dropout if dropout is None else float(dropout)
        L.check(self.lib.dimx_train_vq_forward_backward(
            self.eng.h, self.which, L.ptr(self.params), L.ptr(self.grads), L.ptr(x), B, T, self.beta, self.quant_loss_weight, p,
            self.seed, int(self.step_count if step is None else step), L.ptr(self._loss), L.ptr(pred), L.ptr(idx), ws, wsb,
            L.stream_ptr(self.device)), "dimx_train_vq_forward_backward")
        out = self._loss.clone()
        d = {"loss": out[0], "rec_loss": out[1], "quant_loss": out[2], "perplexity": out[3]}
        return d, pred, idx

    def train_step(self, x):
        """one optimisation step of the reference loop's body; returns (out, quant_loss, info) like ``model(data)`` there, info =
        (perplexity, one-hot codes [B*T,512], idx [B*T,1]); the losses of the step are in ``self.last``."""
        d, pred, idx = self.forward_backward(x)
        self.all_reduce_grads()
        self.step()
        self.last = d
        onehot = torch.zeros(idx.numel(), 512, dtype=torch.float32, device=self.device)
        onehot.scatter_(1, idx.long()[:, None], 1.0)
        return pred, d["quant_loss"], (d["perplexity"], onehot, idx.long()[:, None])


class ConverterHipTrainer(HipTrainer):
    """The DIM-Speaker converter's training step on the HIP kernels: reference loop code/train_converter.py:17-96 over
    ``EmocaConverter.forward`` (code/seq2seq_pretrain.py:826-842) -- ``loss = mse(mesh, vertices) + 5 mse`` over the mouth vertices,
    AdamW(lr 1e-5, torch's defaults otherwise).  What trains is the head ``dimx_mesh_head`` runs (20 tensors:
    ``vertice_map_reverse_lstm.*`` and ``vertice_map_reverse.*``); forward, the LSTM's back-propagation through time and every
    weight gradient run in libdimx_hip.so (csrc/train.hip conv_run, csrc/lstm.hip, csrc/train_lstm.hip).  The frozen speaker
    VQ-VAE runs through the inference engine exactly as ``EmocaConverter.forward`` does (``vq_encode(0, ..., pe_mode=1)`` then
    ``vq_decode``); its result is the head's input.  Same flat arenas, AdamW, optimiser-state import / export, ``sync_to_model()``
    and ``all_reduce_grads()`` as HipTrainer; ``dimx.train.converter_loss`` (PyTorch autograd) is its checker
    (tests/test_gpu_train_converter.py).

    Reference behaviour kept, and deliberate differences:
      * clipping: the reference calls ``clip_grad_norm_`` BEFORE ``backward()``, right after ``zero_grad()``
        (train_converter.py:22,35-37); with its torch the gradients are None there, so its ``clip=1.0`` clips nothing.  The
        drop-in default is therefore ``clip=0.0``; ``clip > 0`` clips the real gradients and is an opt-in;
      * the reference's optimiser also holds ``vertice_mapping.*``, ``squasher.*``, ``vertice_map_reverse_lstm_2.*`` and
        ``vertice_map_reverse2.*``; they never receive a gradient, so AdamW skips them (weight decay included).  They are not in
        the arena and come back untouched from ``sync_to_model()``; ``speaker_vq.*`` is frozen;
      * ``model.train()`` in the reference loop also flips the frozen VQ-VAE into train mode, so its two ``Dropout(0.1)`` fire
        during training -- an accident of calling ``.train()`` on the parent.  Here the frozen VQ-VAE runs in eval arithmetic in
        ``train_step`` and in ``evaluate``;
      * batch size: the reference reshapes with a leading 1 (B = 1 only); here the loss is the mean over all B clips (equal at B = 1);
      * ``mouth_map`` is passed in (the reference reads ``../data/CodeTalker/BIWI/regions/lve.txt``);
      * the adjoint recurrence runs on the no-communication safe path on every device (the weight-stationary group kernel
        exists for the forward only); ``flags`` bit 0 puts the forward on that path too."""

    _ABI = "dimx_train_conv"
    _SIZER = "dimx_train_conv_workspace_bytes"
    _LOSS_FLOATS = 4
    _UNGRAPHED = "converter"

    def __init__(self, model, lr=1e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, clip=0.0, device=None):
        super().__init__(model, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, clip=clip, device=device)
        self._vw = {}

    def vertex_weights(self, mouth_map):
        """(the [V/3] f32 multiplicity vector of ``mouth_map`` on the device, len(mouth_map)); cached per map"""
        from .train import mouth_vertex_weights
        key = tuple(int(i) for i in mouth_map)
        if key not in self._vw:
            if len(self._vw) >= 4:
                self._vw.pop(next(iter(self._vw)))
            self._vw[key] = mouth_vertex_weights(key, self.model.mesh_dim // 3, self.device).contiguous()
        return self._vw[key], len(key)

    @torch.no_grad()
    def motion(self, emoca):
        """the frozen speaker VQ-VAE's reconstruction of ``emoca`` [B,T,56], as EmocaConverter.forward computes it"""
        with self.model.engine_pinned():
            eng = self.model.engine(self.device)
            idx, _ = eng.vq_encode(0, emoca.to(self.device, torch.float32).contiguous(), None, pe_mode=1, return_z=True)
            return eng.vq_decode(0, idx, 0).to(torch.float32).contiguous()

    def _run(self, vertices, template, emoca, mouth_map, flags, with_grads, motion=None):
        motion = self.motion(emoca) if motion is None else motion.to(self.device, torch.float32).contiguous()
        B, T, _ = motion.shape
        V = self.model.mesh_dim
        target = vertices.to(self.device, torch.float32).reshape(B, T, V).contiguous()
        templ = template.to(self.device, torch.float32).reshape(B, V).contiguous() if template is not None else None
        vw, n_mouth = (None, 0) if mouth_map is None else self.vertex_weights(mouth_map)
        ws, wsb = self._workspace(B, T)
        mesh = torch.empty(B, T, V, dtype=torch.float32, device=self.device)
        L.check(self.lib.dimx_train_conv_forward_backward(
            self.eng.h, L.ptr(self.params), L.ptr(self.grads) if with_grads else None, L.ptr(motion), L.ptr(templ), L.ptr(target),
            L.ptr(vw), n_mouth, B, T, int(flags), L.ptr(self._loss), L.ptr(mesh), ws, wsb,
            L.stream_ptr(self.device)), "dimx_train_conv_forward_backward")
        out = self._loss.clone()
        return {"loss": out[0], "mse": out[1], "mouth": out[2]}, mesh

    def forward_backward(self, vertices, template, emoca, mouth_map=None, flags=0, motion=None):
        """vertices [B,T,V] (target), template [B,V] or None, emoca [B,T,56] -> ({loss, mse, mouth} device scalars, mesh [B,T,V]);
        gradients in ``self.grads``.  flags bit 0: the safe LSTM path."""
        return self._run(vertices, template, emoca, mouth_map, flags, True, motion)

    def evaluate(self, vertices, template, emoca, mouth_map=None, flags=0, motion=None):
        """forward and loss only (the reference's evaluate_epoch body); ``self.grads`` is not touched"""
        return self._run(vertices, template, emoca, mouth_map, flags, False, motion)

    def train_step(self, vertices, template, emoca, mouth_map=None, flags=0):
        """one optimisation step of the reference loop's body; returns (loss, mesh) like ``loss, vertices_pred`` there; the three
        losses of the step are in ``self.last``."""
        d, mesh = self.forward_backward(vertices, template, emoca, mouth_map=mouth_map, flags=flags)
        self.all_reduce_grads()
        self.step()
        self.last = d
        return d["loss"], mesh


class SpeakerHipTrainer(HipTrainer):
    """The DIM-Speaker fine-tuning step on the HIP kernels: reference loop ``train_epoch_biwi`` (code/x_engine_pt.py:62-132) over
    ``SpeakerSLMFT.forward(mode='train')`` (code/seq2seq_pretrain.py:708-757) as code/finetune_s2s_pretrain.py's speaker branch
    drives it -- AdamW(lr 1e-5, torch's defaults otherwise), ``clip=1.0``, batch size 1.  ``total = l_ce + l_emoca``: the cross
    entropy of the teacher-forced decoder over the listener VQ-VAE's codes of the EMOCA stream, and the mean squared error of the
    decoded arg-max codes through the speaker VQ-VAE's decoder.  What trains is what that forward leaves a gradient on
    (``SpeakerSLMFT.dimx_trainable_parameters()``): ``decoder_joint.*`` (positional table included), ``patch_embed_dec_l`` and
    ``speaker_embed.weight`` through the cross entropy, ``speaker_vq.decoder.*`` through the EMOCA loss (the arg-max cuts the
    graph in front of it).  ``speaker_embed.weight`` gets a dense gradient: rows no clip names get zeros, and AdamW still decays
    them, as torch's does.  Forward and backward run in libdimx_hip.so (csrc/train.hip spk_run, csrc/train_spk.hip); the frozen
    listener VQ-VAE encodes through the inference engine exactly as ``SpeakerSLMFT.forward`` does.  Same flat arenas, clip +
    AdamW, optimiser-state import / export, ``sync_to_model()`` and ``all_reduce_grads()`` as HipTrainer;
    ``dimx.train.speaker_loss`` (PyTorch autograd) is its checker (tests/test_gpu_train_speaker.py).

    Reference behaviour kept, and deliberate differences:
      * clipping: here the reference clips AFTER ``backward()`` (x_engine_pt.py:108-110), so its ``clip=1.0`` really clips: the
        global norm runs over the whole arena, which is exactly the set of tensors that have a gradient in the reference;
      * everything outside the arena (the three encoders, ``norm*``, ``W``, the LSTM head ``vertice_map_reverse*``,
        ``vertice_mapping``, ``squasher``, the ``_2`` head, ``patch_embed_{s,l,dec_s}``, both VQ encoders and codebooks, the
        listener VQ-VAE) keeps ``grad = None`` in the reference: AdamW skips it (weight decay included) and it comes back
        untouched from ``sync_to_model()``.  The converter head only REPORTS ``d['l_cont_s']``; it adds nothing to ``total``;
      * ``model.train()`` in the reference loop also flips the VQ-VAEs into train mode, so the ``Dropout(0.1)`` behind their
        positional encodings fires during training -- an accident of calling ``.train()`` on the parent.  Here both VQ-VAEs run
        in eval arithmetic;
      * batch size: the reference's mouth indexing only type-checks at B = 1; here every mean runs over all B clips (equal at
        B = 1);
      * ``mouth_map`` is a constructor argument (default: the model's; the reference reads
        ``../data/CodeTalker/BIWI/regions/lve.txt``).  Without a map ``d['l_cont_s']`` is 0 and the mesh head is not launched;
      * the reference's ``evaluate_epoch_biwi`` passes ``v_speaker_emoca=None`` and fails inside ``forward_vq``; it is not
        built (``SpeakerSLMFT.forward`` raises ``ValueError`` for None) and the driver never calls it."""

    _ABI = "dimx_train_spk"
    _SIZER = "dimx_train_spk_workspace_bytes"
    _LOSS_FLOATS = 4
    _UNGRAPHED = "DIM-Speaker"
    _MODEL_MAP = object()

    def __init__(self, model, lr=1e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, clip=1.0, mouth_map=_MODEL_MAP, device=None):
        super().__init__(model, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, clip=clip, device=device)
        mm = getattr(model, "mouth_map", None) if mouth_map is SpeakerHipTrainer._MODEL_MAP else mouth_map
        self.mouth_map = None if mm is None else [int(i) for i in mm]
        if self.mouth_map is not None:
            assert all(0 <= i < model.mesh_dim // 3 for i in self.mouth_map), "mouth_map holds vertex indices in [0, mesh_dim / 3)"
        self.last_out = {}

    def _mouth(self, pred, vertices, template):
        """the reported mouth term of ``SpeakerSLMFT.forward``: mse over the map's vertices of the mesh head's output (no graph)"""
        import torch.nn.functional as F
        with torch.no_grad(), self.model.engine_pinned():
            B, n, _ = pred.shape
            templ = template.to(self.device, torch.float32).contiguous() if template is not None else None
            mesh = self.model.engine(self.device).mesh_head(pred, templ)
            idx = torch.as_tensor(self.mouth_map, device=self.device, dtype=torch.long)
            tgt = vertices.to(self.device)[:, 1:, :].reshape(B, n, -1, 3)[:, :, idx, :]
            return F.mse_loss(mesh.view(B, n, -1, 3)[:, :, idx, :], tgt.to(mesh.dtype))

    def forward_backward(self, vertices, emoca, audio, mask, template, speaker_ids=None, z=None, return_logits=False):
        """vertices [B,T,V], emoca [B,T,56], audio [B,T,768], mask [B,T] bool, template [B,V] or None, speaker_ids [B] or None ->
        (total = l_ce + l_emoca, d with the reference's six keys) as device scalars; gradients in ``self.grads``.  z [B,T]: the
        listener VQ-VAE's codes of ``emoca`` (-100 on padding; default: ``model.forward_vq``).  The step's code indices
        [B*(T-1)] int32, decoded coefficients [B,T-1,56] and (``return_logits``) logits [B,T-1,512] are left in ``self.last_out``.
        ``vertices`` / ``template`` only feed the reported mouth term and may be None without a ``mouth_map``."""
        m = self.model
        mask = mask.bool()
        B, T = mask.shape
        if z is None:
            with torch.no_grad():
                _, z = m.forward_vq(None, emoca.to(self.device), mask.to(self.device))
        f = lambda t: t.detach().to(self.device, torch.float32).contiguous()
        v_e, v_a = f(emoca), f(audio)
        m8 = mask.to(self.device).to(torch.uint8).contiguous()
        z32 = z.to(self.device).to(torch.int32).contiguous()
        ids = speaker_ids.to(self.device).to(torch.int32).contiguous() if speaker_ids is not None else None
        book, pe = f(m.speaker_vq.quantize.embedding.weight), f(m.speaker_vq.decoder.decoder_pos_embedding.pe)
        ws, wsb = self._workspace(B, T)
        kw = dict(device=self.device)
        logits = torch.empty(B, T - 1, 512, dtype=torch.float32, **kw) if return_logits else None
        idx = torch.empty(B * (T - 1), dtype=torch.int32, **kw)
        pred = torch.empty(B, T - 1, 56, dtype=torch.float32, **kw)
        L.check(self.lib.dimx_train_spk_forward_backward(
            self.eng.h, L.ptr(self.params), L.ptr(self.grads), L.ptr(v_e), L.ptr(v_a), L.ptr(m8), L.ptr(z32), L.ptr(ids), L.ptr(book),
            L.ptr(pe), B, T, L.ptr(self._loss), L.ptr(logits), L.ptr(idx), L.ptr(pred), ws, wsb,
            L.stream_ptr(self.device)), "dimx_train_spk_forward_backward")
        out = self._loss.clone()
        l_ce, l_emoca = out[0], out[2]
        l_mouth = self._mouth(pred, vertices, template) if self.mouth_map is not None else 0
        self.last_out = {"idx": idx, "pred": pred, "logits": logits}
        d = {"l_ce_s": 0, "l_ce_l": l_ce, "l_cont_s": l_mouth, "l_cont_l": l_emoca, "nce": 0, "c_acc": 0}
        return l_ce + l_emoca, d

    def train_step(self, vertices, emoca, audio, mask, template, speaker_ids=None, z=None):
        """one optimisation step of the reference loop's body; returns (total, d) like ``model(xv, xe, xa, mask, xt,
        speaker_ids=...)`` there (its third value is ``self.last_out['pred']``)."""
        total, d = self.forward_backward(vertices, emoca, audio, mask, template, speaker_ids=speaker_ids, z=z)
        self.all_reduce_grads()
        self.step()
        return total, d
