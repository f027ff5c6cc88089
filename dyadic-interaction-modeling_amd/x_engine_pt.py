"""Evaluation engine with the batch protocol of reference code/x_engine_pt.py:201-277.

The loader yields ``(src [B,T,824] zero-padded, tgt [B,T,56], src_len list[int], ids, data_ids)``; the
engine builds the prefix mask, splits ``src`` into speaker motion (56) and audio features (768), calls
``model(src_s_v, tgt, src_s_a, mask, mode=...)`` and accumulates per-clip numpy arrays cut to
``src_len - 1`` frames.  ``evaluate_test_epoch`` keeps, per clip, the best of ``beam_size`` stochastic
generations by Frechet distance to the ground truth, exactly like the reference.

Multi-GPU: clips are independent, so each rank evaluates its own shard of every batch (weights
replicated) and the per-clip predictions are all-gathered to every rank (``dimx.dist``); with one
process the gather is the identity.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import dist as ddist
from . import lib as L
from .metrics import clip_fd

_POOL = None


def _metric_pool():
    """Background worker(s) of the host-side Frechet distances.  One by default: scipy's sqrtm spends its 1.4 ms per (clip, try)
    mostly under the GIL, more threads made it SLOWER (8 threads: 3.2 ms each on an 8-core host) -- the worker exists so that
    the scoring of batch i overlaps the generation of batch i + 1, not to parallelise it.  DIMX_METRIC_THREADS overrides."""
    global _POOL
    n = int(os.environ.get("DIMX_METRIC_THREADS", "0")) or 1
    if _POOL is None or _POOL._max_workers != n:
        _POOL = ThreadPoolExecutor(max_workers=n, thread_name_prefix="dimx-fd")
    return _POOL


def _fd_or_error(gt, pred):
    try:
        return float(clip_fd(gt, pred)), None
    except ValueError as e:          # scipy's "Imaginary component" on a degenerate clip
        return float("inf"), e


def _mask_from_lens(src, src_len, device):
    mask = torch.zeros((src.shape[0], src.shape[1]), dtype=torch.bool)
    for j in range(src.shape[0]):
        mask[j, :src_len[j]] = True
    from .seq2seq_pretrain import mark_prefix
    return mark_prefix(mask.to(device))     # built as a prefix mask: SLMFT.forward_vq has nothing to compact


def _prepare(batch, device):
    src, tgt, src_len, _, data_ids = batch
    src = src.to(device, non_blocking=True)     # pinned host batches (dimx.dataset.data_loader) copy asynchronously
    tgt = tgt.to(device, non_blocking=True)
    src_s_v, src_s_a = torch.split(src, [56, 768], dim=2)
    mask = _mask_from_lens(src, src_len, device)
    return src_s_v.contiguous(), src_s_a.contiguous(), tgt, mask, list(src_len), data_ids


def evaluate_epoch(model, loader, device, log=print):
    """reference code/x_engine_pt.py:134-165 (the validation pass of code/train_s2s_pretrain.py:60): mean of
    ``model(src_s_v, tgt, src_s_a, mask)[0]`` over the loader; the six loss terms averaged over the batches are printed."""
    model.eval()
    losses = []
    d = {k: 0.0 for k in ("l_ce_s", "l_ce_l", "l_cont_s", "l_cont_l", "nce", "c_acc")}
    n = 0
    with torch.no_grad():
        for batch in loader:
            src_s_v, src_s_a, tgt, mask, _, _ = _prepare(batch, device)
            loss, d_step, _ = model(src_s_v, tgt, src_s_a, mask)
            losses.append(float(loss.mean().item()))
            for k in d:
                v = d_step.get(k, 0)
                d[k] += float(v.mean().item()) if torch.is_tensor(v) else float(v)
            n += 1
    for k in d:
        d[k] /= max(n, 1)
    log(d)
    return float(np.mean(losses)) if losses else float("nan")


def evaluate_finetune_epoch(model, loader, device, lookahead=None):
    """reference code/x_engine_pt.py:201-230 (teacher-forced forward, mode='train').

    ``lookahead`` L (SLMFT): the validation epoch of an online fine-tuning (``train_epoch(lookahead=L)``) -- the same
    teacher-forced pass under the visibility the model was trained with (``SLMFT.forward_online_tf``: one windowed pass per batch,
    no random key mask).  The return value then gains a fifth entry, the epoch's validation loss: the mean over the batches of the
    batch's cross entropy (row losses summed over the valid targets / their number, as ``forward(mode='train')`` forms ``l_ce_l``).
    None (default) is the reference's offline epoch and its four lists."""
    y_trues_all, y_preds_all, x_all, data_ids_all = [], [], [], []
    losses = []
    model.eval()
    with torch.no_grad():
        for batch in loader:
            src_s_v, src_s_a, tgt, mask, src_len, data_ids = _prepare(batch, device)
            if lookahead is None:
                _, _, y_preds = model(src_s_v, tgt, src_s_a, mask, mode="train")
            else:
                _, d_val, y_preds = getattr(model, "module", model).forward_online_tf(src_s_v, tgt, src_s_a, mask, int(lookahead))
                losses.append(d_val["l_ce_l"])
            y_true = tgt[:, 1:, :]
            yp, yt, xs = y_preds.cpu().numpy(), y_true.cpu().numpy(), src_s_v.cpu().numpy()
            for j in range(len(yp)):
                n = src_len[j] - 1
                y_preds_all.append(yp[j][:n])
                y_trues_all.append(yt[j][:n])
                x_all.append(xs[j][:n])
                data_ids_all.append(data_ids[j])
    if lookahead is not None:
        return y_trues_all, y_preds_all, x_all, data_ids_all, float(torch.stack(losses).mean()) if losses else float("nan")
    return y_trues_all, y_preds_all, x_all, data_ids_all


BATCHED_SAMPLE_COUNTS = (2, 4, 5, 8, 10)


def _gather_ragged(best, n_local, width, feat, device, total=None):
    """all-gather a rank's list of [n_j, feat] arrays (None = no candidate was ever better than inf, as in the
    reference) in shard order; returns the list for the whole batch.  ONE collective: the valid lengths ride in the same
    buffer as the padded rows, and with ``total`` (rows of the whole batch) the shard sizes follow from shard_bounds on every
    rank -- no count exchange, no host synchronisation before the payload."""
    lens = torch.tensor([-1 if b is None else b.shape[0] for b in best], dtype=torch.int32, device=device).reshape(n_local, 1)
    pad = torch.zeros(n_local, width, feat, dtype=torch.float32, device=device)
    for j, b in enumerate(best):
        if b is not None and b.shape[0]:
            pad[j, :b.shape[0]] = torch.from_numpy(np.ascontiguousarray(b)).to(device)
    counts = ddist.shard_counts(total) if total is not None else None
    buf = ddist.all_gather_rows(ddist.pack_rows(lens, pad), counts)
    lens_all, pad_all = ddist.unpack_rows(buf, [((1,), torch.int32), ((width, feat), torch.float32)])
    lens_all = lens_all.reshape(-1).cpu().tolist()
    pad_all = pad_all.cpu().numpy()
    return [None if n < 0 else pad_all[j, :n].copy() for j, n in enumerate(lens_all)]


def _select_device(y_true, y_preds, lens, world, device, total=None):
    """fd_backend="device": distances of all (clip, try) pairs in one batched float64 computation on the GPU; the first minimum
    per clip wins (= the strict '<' of the reference's loop), a clip whose distances are all inf / nan keeps None."""
    from .metrics import frechet_distances_torch
    fd = frechet_distances_torch(y_true, y_preds, lens)                   # [nl, S]
    fd = torch.where(torch.isnan(fd), torch.full_like(fd, float("inf")), fd)
    win = fd.argmin(dim=1)
    ok = torch.isfinite(fd.gather(1, win[:, None])[:, 0]).cpu().tolist()
    chosen = y_preds[torch.arange(len(lens), device=y_preds.device), win].cpu().numpy()
    best = [chosen[j][:lens[j]].copy() if ok[j] else None for j in range(len(lens))]
    if world > 1:
        best = _gather_ragged(best, len(lens), y_preds.shape[2], y_preds.shape[3], device, total)
    return best


def _select_hip(y_true, y_preds, lens, world, device, total=None, metrics=None, x=None):
    """fd_backend="hip": distances, winner and gather in the HIP library (dimx.engine.op_fd_select, csrc/fd_select.hip) on the
    stream the generation ran on; only the winners' frames and the ok flags cross to the host.  A clip without a finite distance
    keeps None, as in _select_device."""
    from .engine import op_fd_select
    _, _, ok, best = op_fd_select(y_true, y_preds, lens)
    return _winners_to_host(y_true, y_preds, ok, best, lens, world, device, total, metrics, x)


def _select_likelihood(y_true, y_preds, scores, lens, world, device, total=None, metrics=None, x=None):
    """select="likelihood": the try the model itself scores highest (dimx.engine.op_score_select, csrc/seq_score.hip, on the
    generation's own SeqScores); no distance is computed and ``y_true`` is read by ``metrics`` only.  A clip with nothing to score
    has all scores 0.0: try 0 wins with ok = 1 and the clip keeps an empty array."""
    from .engine import op_score_select
    _, ok, best = op_score_select(scores.score, y_preds, lens)
    return _winners_to_host(y_true, y_preds, ok, best, lens, world, device, total, metrics, x)


def _select_consensus(y_true, y_preds, distance, lens, world, device, total=None, metrics=None, x=None):
    """select="consensus": the try with the smallest summed distance to the clip's other tries (dimx.engine.op_consensus_select,
    csrc/consensus.hip; the definition is dimx.consensus); ``y_true`` is read by ``metrics`` only.  A clip with fewer than 2
    valid frames has no distances and keeps None."""
    from .engine import op_consensus_select
    _, _, ok, best = op_consensus_select(y_preds, lens, distance=distance)
    return _winners_to_host(y_true, y_preds, ok, best, lens, world, device, total, metrics, x)


def _winners_to_host(y_true, y_preds, ok, best, lens, world, device, total, metrics, x):
    """the tail of a selection in the HIP library: ``best`` [nl, L, W] and ``ok`` [nl] lie on the device"""
    if metrics is not None:      # the winners where they lie: enqueued behind the selection, nothing is synchronised
        metrics.update(y_true, best, x, lens)
    ok = ok.cpu().tolist()
    chosen = best.cpu().numpy()
    best = [chosen[j][:lens[j]].copy() if ok[j] else None for j in range(len(lens))]
    if world > 1:
        best = _gather_ragged(best, len(lens), y_preds.shape[2], y_preds.shape[3], device, total)
    return best


def _select(pending, skip_degenerate, world, device):
    """Best of the tries per clip, in the reference's order of evaluation (try-major, clip-minor; a candidate replaces the
    current best only when its distance is strictly smaller; the first ValueError in that order propagates unless
    skip_degenerate scores it as inf).  The distances come from the worker threads; which candidate wins does not depend
    on how many there are."""
    futs, samples, lens, nl, width, feat, total = pending
    cur_best = [float("inf")] * nl
    best = [None] * nl
    for s_i, yp in enumerate(samples):
        for j in range(nl):
            cfid, err = futs[s_i][j].result()
            if err is not None and not skip_degenerate:
                raise err
            if cfid < cur_best[j]:
                best[j] = yp[j][:lens[j]].copy()
                cur_best[j] = cfid
    if world > 1:
        best = _gather_ragged(best, nl, width, feat, device, total)
    return best


def evaluate_test_epoch(model, loader, device, beam_size=10, batched_samples=True, skip_degenerate=False,
                        fd_backend="reference", metrics=None, prompt_frames=1, filter_logits_fn=None, filter_kwargs=None,
                        select="fd", decode="sample", beam_width=None, consensus_distance="fd", lookahead=None, window_prefill=False, guidance=None,
                        kv8=False, self_kv8=False, kv8_samples=False, beam_kv8=None, **forward_kw):
    """reference code/x_engine_pt.py:232-277 (autoregressive generation, best of ``beam_size`` by FD; a candidate
    replaces the current best only when its FD is strictly smaller, and scipy's "Imaginary component" ValueError on a
    degenerate clip propagates, both as in the reference; ``skip_degenerate=True`` scores such a candidate as inf).

    ``batched_samples``: draw the ``beam_size`` generations of a clip in ONE forward pass (n_samples) instead of
    ``beam_size`` passes -- same distribution (independent multinomial draws given the same inputs), but the VQ
    encode, the encoder stack and the context K/V stream are shared.  Falls back to the reference's loop for
    sample counts the kernels are not instantiated for.

    Multi-GPU (default process group initialised): every rank receives the full batch from its loader, generates and
    scores rows [lo, hi) of it (``batch_row_offset=lo`` and ``shard=(lo, B)`` keep positional rows and sampler
    streams those of the unsharded batch) and the selected predictions are all-gathered, so every rank returns the
    complete lists.

    Host side: the beam_size x B Frechet distances of a batch (numpy covariance + scipy sqrtm in float64, the reference's own
    arithmetic, 1.4 ms each) are computed by a background thread while the GPU generates the next batch, and the winner is then
    picked in the reference's order -- same selections, bit for bit (tests/test_host_protocol_golden.py).  That arithmetic is
    1.4 ms per (clip, try) of single-threaded scipy (it does not scale over threads): 3.6 s for 256 clips x 10 tries against
    0.7 s of generation.  ``fd_backend="device"`` computes the same quantity for the whole batch in torch float64 on the GPU
    (dimx.metrics.frechet_distances_torch: eigenvalues instead of scipy's sqrtm, so the last digits differ and rank-deficient
    clips do not raise) and brings only the winners to the host.  ``fd_backend="hip"`` follows the same path with the distances,
    the winner and the gather of the winning sequences all in the project's own kernels (dimx.engine.op_fd_select, csrc/fd_select.hip;
    GPU only: a CPU device raises lib.DimxError).

    ``prompt_frames`` P > 1: every generation continues the clip's first P ground-truth listener codes (SLMFT.forward
    ``prompt_frames``, with the batch's ``src_len`` as ``lengths``); selection and the returned lists stay over the whole clip.

    ``metrics``: a dimx.metrics.ListenerMetrics that is updated per batch with the device-resident winners, ``tgt[:, 1:]``, the
    speaker motion and the lens right after the selection (dimx_op_listener_metrics, csrc/listener_metrics.hip), so that
    print_metrics / print_metrics_full need no host pass over the returned lists.  It needs ``fd_backend="hip"``, a GPU and one
    process; anything else raises.  The default None leaves every path as it is.

    ``filter_logits_fn`` / ``filter_kwargs``: the sampler filter of every generation (AutoregressiveWrapper.generate's arguments:
    ``top_k``, ``top_p``, ``min_p`` or ``top_a`` of dimx.sampling, object or name); None is the reference's top-k 52.  A rank
    of a sharded batch filters and draws exactly what the single-process batch would: the filter acts on a row's own logits.

    ``select``: "fd" (default) is the protocol above.  "likelihood" keeps, per clip, the try with the largest log-likelihood under
    the model itself (``SLMFT.forward(return_scores=True)`` + dimx.engine.op_score_select): the selection that needs no ground
    truth, for conversations without a recorded listener.  ``fd_backend`` is not consulted, no distance is computed and ``tgt`` is
    used for the returned lists (and by ``metrics``) only; the winners stay on the device, so ``metrics`` works as with
    ``fd_backend="hip"``.  It needs a batched sample count (BATCHED_SAMPLE_COUNTS, ValueError otherwise) and a ROCm GPU (a CPU
    device raises lib.DimxError: there is no CPU fallback).  "consensus" keeps, per clip, the try with the smallest total distance
    to the clip's other tries (minimum Bayes risk, the medoid; dimx.engine.op_consensus_select, definition dimx.consensus): it needs
    no ground truth either and does not share the likelihood pick's preference for the modal, low-motion sequence.
    ``consensus_distance`` is "fd" (default: the protocol's own Frechet distance, between tries) or "l2".  The same conditions hold as
    for "likelihood": ``tgt`` is not read for the selection, the winners stay on the device (``metrics`` works), a batched sample
    count and a ROCm GPU are needed.  Any other value of ``select`` or ``consensus_distance`` raises ValueError.

    ``decode``: "sample" (default) is the protocol above; ``beam_size`` is, as in the reference, the NUMBER OF TRIES of a clip --
    independent samples, not a beam.  "beam" replaces the tries by the ``beam_width`` final hypotheses of ONE beam search per clip
    (``SLMFT.forward(beam_width=W, num_return=W)``, dimx.beam; W in BATCHED_SAMPLE_COUNTS, default ``beam_size``): a deterministic
    n-best list, best first, that goes through the same ``select`` ("likelihood" picks by the search's own scores, that is row 0;
    "consensus" picks the hypothesis the rest of the list agrees with most).
    ``beam_size``, ``batched_samples`` and the sampler filter are not consulted then.  It needs a ROCm GPU.

    ``lookahead`` L: every generation is an online one (dimx.online, ``SLMFT.forward(lookahead=L)``): the listener token of frame
    t+1 is drawn from the speaker frames below clamp(t + 2 + L, 1, T).  Selection, metrics and the returned lists are unchanged.
    None (default) is the reference's offline protocol.  Not with ``decode="beam"`` (ValueError).  ``window_prefill`` (with
    ``prompt_frames`` and ``lookahead``): the prompts are prefilled in one pass under the window instead of running through forced
    decode steps (``SLMFT.forward(window_prefill=True)``).

    ``guidance`` s: every generation is a guided one (dimx.guidance, ``SLMFT.forward(guidance=s)``).  A guided generation draws one
    sample per clip, so the ``beam_size`` tries are ``beam_size`` passes (the reference's loop) and ``select`` must be "fd"; not with
    ``decode="beam"`` (ValueError).  None (default) leaves every path as it is.

    ``kv8``: every generation reads an FP8 copy of the context K / V in its decode steps (dimx.kv8, ``SLMFT.forward(kv8=True)``).
    Such a generation draws one sample per clip too, so the tries are ``beam_size`` passes and ``select`` must be "fd"; not with
    ``decode="beam"`` (ValueError).  False (default) leaves every path as it is.

    ``self_kv8``: every generation keeps its self-attention K / V caches in FP8 (dimx.kv8.self_step, ``SLMFT.forward(self_kv8=True)``).
    The batched best-of-``beam_size`` pass takes it as it is, with every ``select``; not with ``decode="beam"`` or ``guidance``
    (ValueError).  False (default) leaves every path as it is.

    ``kv8_samples``: ``kv8`` for the batched pass (dimx.kv8.attention_rows, ``SLMFT.forward(kv8_samples=True)``): the
    ``beam_size`` tries of a clip stay ONE generation whose multi-query cross attention reads the FP8 codes, with every ``select``
    and with ``self_kv8``; not with ``decode="beam"`` or ``guidance`` (ValueError).  False (default) leaves every path as it is.

    ``beam_kv8``: "self", "cross", "both" or True with ``decode="beam"``: every beam search runs on FP8 self caches and / or an FP8
    copy of the cross K/V (dimx.kv8.reorder, ``SLMFT.forward(beam_kv8=...)``), with every ``select``; without ``decode="beam"`` or
    with ``guidance`` it raises ValueError.  None (default) leaves every path as it is."""
    if beam_kv8:
        if decode != "beam" or guidance is not None:
            raise ValueError("evaluate_test_epoch(beam_kv8=...) applies to decode='beam' without guidance")
        forward_kw = dict(forward_kw, beam_kv8=True if beam_kv8 == "both" else beam_kv8)
    if kv8_samples:
        if decode == "beam" or guidance is not None:
            raise ValueError("evaluate_test_epoch(kv8_samples=True) applies to decode='sample' without guidance")
        forward_kw = dict(forward_kw, kv8_samples=True)
    if self_kv8:
        if decode == "beam" or guidance is not None:
            raise ValueError("evaluate_test_epoch(self_kv8=True) applies to decode='sample' without guidance")
        forward_kw = dict(forward_kw, self_kv8=True)
    if kv8:
        if decode == "beam" or select != "fd":
            raise ValueError("evaluate_test_epoch(kv8=True) applies to decode='sample' with select='fd': an FP8 cross K/V generation "
                             "draws one sample per clip")
        batched_samples = False
        forward_kw = dict(forward_kw, kv8=True)
    if guidance is not None:
        if decode == "beam" or select != "fd":
            raise ValueError("evaluate_test_epoch(guidance=...) applies to decode='sample' with select='fd': a guided generation "
                             "draws one sample per clip")
        batched_samples = False
        forward_kw = dict(forward_kw, guidance=float(guidance))
    if decode not in ("sample", "beam"):
        raise ValueError("decode=%r: one of 'sample', 'beam'" % (decode,))
    if lookahead is not None:
        if decode == "beam":
            raise ValueError("evaluate_test_epoch(lookahead=...) applies to decode='sample': beam search has no online form")
        forward_kw = dict(forward_kw, lookahead=int(lookahead))
        if window_prefill:
            forward_kw["window_prefill"] = True
    if decode == "beam":
        beam_size = int(beam_width if beam_width is not None else beam_size)
        if beam_size not in BATCHED_SAMPLE_COUNTS:
            raise ValueError("evaluate_test_epoch(decode='beam'): beam_width must be one of %s (got %d)" % (BATCHED_SAMPLE_COUNTS, beam_size))
        if torch.device(device).type != "cuda":
            raise L.DimxError("evaluate_test_epoch(decode='beam') runs on a ROCm GPU only (device %s): there is no CPU fallback" % (device,))
        batched_samples, filter_logits_fn, filter_kwargs = True, None, None
        tries_kw = dict(beam_width=beam_size, num_return=beam_size)
    else:
        tries_kw = dict(n_samples=beam_size)
    if filter_logits_fn is not None or filter_kwargs:
        forward_kw = dict(forward_kw, filter_logits_fn=filter_logits_fn, filter_kwargs=filter_kwargs)
    if select not in ("fd", "likelihood", "consensus"):
        raise ValueError("select=%r: one of 'fd', 'likelihood', 'consensus'" % (select,))
    if consensus_distance not in ("fd", "l2"):
        raise ValueError("consensus_distance=%r: one of 'fd', 'l2'" % (consensus_distance,))
    by_likelihood, by_consensus = select == "likelihood", select == "consensus"
    if by_likelihood or by_consensus:
        if torch.device(device).type != "cuda":
            raise L.DimxError("evaluate_test_epoch(select='%s') runs on a ROCm GPU only (device %s): there is no CPU fallback; "
                              "select='fd' with fd_backend='reference' or 'device' runs there" % (select, device))
        if not (batched_samples and beam_size in BATCHED_SAMPLE_COUNTS):
            raise ValueError("evaluate_test_epoch(select='%s') %s the tries of one batched generation: beam_size must be "
                             "one of %s with batched_samples (got %d)" % (select, "scores" if by_likelihood else "compares",
                                                                          BATCHED_SAMPLE_COUNTS, beam_size))
        fd_backend = "hip"      # not consulted for the selection: the winners are handled where the HIP selection leaves its own
    assert fd_backend in ("reference", "device", "hip")
    if metrics is not None:
        if fd_backend != "hip":
            raise ValueError("evaluate_test_epoch(metrics=...) needs fd_backend='hip' (got %r): the accumulator reads the winners "
                             "the HIP selection leaves on the device" % (fd_backend,))
        if torch.device(device).type != "cuda":
            raise L.DimxError("evaluate_test_epoch(metrics=...) runs on a ROCm GPU only (device %s): there is no CPU fallback; "
                              "dimx.mymetrics.print_metrics is the host form" % (device,))
        if ddist.world_size() > 1:
            raise ValueError("evaluate_test_epoch(metrics=...) accumulates on one process; world_size is %d" % ddist.world_size())
    if fd_backend == "hip" and torch.device(device).type != "cuda":
        raise L.DimxError("evaluate_test_epoch(fd_backend='hip') runs on a ROCm GPU only (device %s): there is no CPU fallback; "
                          "fd_backend='reference' and 'device' run there" % (device,))
    on_device = fd_backend in ("device", "hip")
    select_on_device = _select_hip if fd_backend == "hip" else _select_device
    y_trues_all, y_preds_all, x_all, data_ids_all = [], [], [], []
    model.eval()
    batched = batched_samples and beam_size in BATCHED_SAMPLE_COUNTS
    rank, world = ddist.rank(), ddist.world_size()
    pool = _metric_pool()
    pending = None
    with torch.no_grad():
        for batch in loader:
            src_s_v, src_s_a, tgt, mask, src_len, data_ids = _prepare(batch, device)
            y_true = tgt[:, 1:, :].cpu().numpy()
            xs = src_s_v.cpu().numpy()
            B = src_s_v.shape[0]
            for j in range(B):
                n = src_len[j] - 1
                y_trues_all.append(y_true[j][:n])
                data_ids_all.append(data_ids[j])
                x_all.append(xs[j][:n])
            lo, hi = ddist.shard_bounds(B, rank, world)
            nl = hi - lo
            samples = []                 # per try: [nl, T-1, 56] numpy
            if nl > 0:
                kw = dict(forward_kw)
                if world > 1:
                    kw.update(batch_row_offset=lo, shard=(lo, B))
                if prompt_frames != 1:
                    kw.update(prompt_frames=prompt_frames, lengths=src_len[lo:hi])
                sl = [t[lo:hi].contiguous() for t in (src_s_v, tgt, src_s_a, mask)]
                if by_likelihood:
                    _, _, y_preds, scores = model(sl[0], sl[1], sl[2], sl[3], mode="val", return_scores=True, **tries_kw, **kw)
                    extra = dict(metrics=metrics, x=src_s_v[lo:hi]) if metrics is not None else {}
                    y_preds_all.extend(_select_likelihood(tgt[lo:hi, 1:], y_preds, scores, [src_len[lo + j] - 1 for j in range(nl)],
                                                          world, device, B, **extra))
                    continue
                if by_consensus:
                    _, _, y_preds = model(sl[0], sl[1], sl[2], sl[3], mode="val", **tries_kw, **kw)
                    extra = dict(metrics=metrics, x=src_s_v[lo:hi]) if metrics is not None else {}
                    y_preds_all.extend(_select_consensus(tgt[lo:hi, 1:], y_preds, consensus_distance,
                                                         [src_len[lo + j] - 1 for j in range(nl)], world, device, B, **extra))
                    continue
                if batched:
                    _, _, y_preds = model(sl[0], sl[1], sl[2], sl[3], mode="val", **tries_kw, **kw)
                else:
                    y_preds = torch.stack([model(sl[0], sl[1], sl[2], sl[3], mode="val", **kw)[2] for _ in range(beam_size)], 1)
                if on_device:                   # [nl, S, T-1, 56] stays on the device; only the winners travel
                    if pending is not None:
                        y_preds_all.extend(_select(pending, skip_degenerate, world, device))
                        pending = None
                    extra = dict(metrics=metrics, x=src_s_v[lo:hi]) if metrics is not None else {}
                    y_preds_all.extend(select_on_device(tgt[lo:hi, 1:], y_preds, [src_len[lo + j] - 1 for j in range(nl)], world,
                                                        device, B, **extra))
                    continue
                yp_all = y_preds.cpu().numpy()
                samples = [yp_all[:, s_i] for s_i in range(beam_size)]
            elif on_device:
                y_preds_all.extend(_gather_ragged([], 0, tgt.shape[1] - 1, tgt.shape[2], device, B) if world > 1 else [])
                continue
            # this batch's distances go to the worker threads; the PREVIOUS batch's are collected now, after this batch's
            # generation has run in the meantime -- host scoring overlaps the GPU
            if pending is not None:
                y_preds_all.extend(_select(pending, skip_degenerate, world, device))
            lens = [src_len[lo + j] - 1 for j in range(nl)]
            futs = [[pool.submit(_fd_or_error, y_true[lo + j][:lens[j]], yp[j][:lens[j]]) for j in range(nl)] for yp in samples]
            pending = (futs, samples, lens, nl, tgt.shape[1] - 1, tgt.shape[2], B)
        if pending is not None:
            y_preds_all.extend(_select(pending, skip_degenerate, world, device))
    _report_epoch(model, device, "evaluate_test_epoch", len(y_trues_all), None if by_likelihood or by_consensus else fd_backend)
    return y_trues_all, y_preds_all, x_all, data_ids_all


def _baseline_features(library, src_s_v, src_s_a):
    return src_s_a if library.kind == "audio" else src_s_v


def fill_retrieval_library(library, loader, device):
    """The training split into a dimx.retrieval.RetrievalLibrary, batch by batch in the protocol of evaluate_test_epoch: a clip is
    described by all ``src_len`` frames of its audio features (kind "audio") or speaker motion ("motion"), and what it offers as a
    prediction are the listener frames the protocol scores, ``tgt[:, 1:]`` cut to ``src_len - 1``.  Returns the library."""
    if torch.device(device).type != "cuda":
        raise L.DimxError("fill_retrieval_library runs on a ROCm GPU only (device %s): there is no CPU fallback" % (device,))
    for batch in loader:
        src_s_v, src_s_a, tgt, _, src_len, _ = _prepare(batch, device)
        library.add(_baseline_features(library, src_s_v, src_s_a), tgt[:, 1:], src_len, listener_lens=[n - 1 for n in src_len])
    return library


def evaluate_baseline_epoch(library, loader, device, k=1, select=None, consensus_distance="fd", metrics=None, strict_len=False,
                            random_seed=None, random_first=None):
    """The retrieval baselines of reference code/baselines.py:30-103 over a test loader, with the batch and mask protocol of
    evaluate_test_epoch: per test clip the listener sequence of the nearest training clip of ``library`` (a filled
    dimx.retrieval.RetrievalLibrary: "audio" = NN audio, "motion" = NN motion), cut to the shorter of the two clips.  Returns
    ``(y_trues, y_preds, x, data_ids)`` like evaluate_test_epoch, every array cut to the length of the clip's prediction.  A clip
    for which no library entry is eligible (a zero descriptor) gets training clip 0, as the reference's ``best_index = 0`` does.

    ``k`` = 1 is the reference baseline.  ``k`` > 1 retrieves the k nearest clips as an n-best list and hands it to the selectors of
    evaluate_test_epoch: ``select="fd"`` (the oracle pick by Frechet distance to the ground truth, dimx.engine.op_fd_select) or
    ``"consensus"`` (dimx.engine.op_consensus_select with ``consensus_distance``); the clip's length is then the minimum length of
    its list, and a clip whose list has fewer than k entries raises ValueError.  ``select="likelihood"`` raises ValueError:
    retrieved sequences have no model score.  ``random_seed`` (an int) replaces the search by the Random baseline: one host-drawn
    training clip per test clip (``random_first=5`` draws from the first five, the checked-in script's leftover).
    ``strict_len=True`` drops the clips whose retrieved clip has another length than their own, as the reference's ``== 64`` test
    does.  ``metrics``: a dimx.metrics.ListenerMetrics, updated per batch with the device-resident predictions (it needs every kept
    clip to have at least 2 frames).  GPU only: a CPU device raises lib.DimxError."""
    if select == "likelihood":
        raise ValueError("evaluate_baseline_epoch(select='likelihood'): retrieved sequences have no model score")
    if select not in (None, "fd", "consensus"):
        raise ValueError("select=%r: one of None, 'fd', 'consensus'" % (select,))
    if consensus_distance not in ("fd", "l2"):
        raise ValueError("consensus_distance=%r: one of 'fd', 'l2'" % (consensus_distance,))
    k = int(k)
    if k > 1 and select is None:
        raise ValueError("evaluate_baseline_epoch(k=%d) needs select='fd' or 'consensus' to pick one of the k retrieved clips" % k)
    if random_seed is not None and k != 1:
        raise ValueError("evaluate_baseline_epoch(random_seed=...) draws one clip per test clip: k must be 1")
    if torch.device(device).type != "cuda":
        raise L.DimxError("evaluate_baseline_epoch runs on a ROCm GPU only (device %s): there is no CPU fallback; dimx.retrieval holds "
                          "the host definition" % (device,))
    from .engine import op_nn_gather
    y_trues_all, y_preds_all, x_all, data_ids_all = [], [], [], []
    _, _, lib_seq, lib_lens = library.buffers()
    with torch.no_grad():
        for n_batch, batch in enumerate(loader):
            src_s_v, src_s_a, tgt, _, src_len, data_ids = _prepare(batch, device)
            B, Lo = src_s_v.shape[0], tgt.shape[1] - 1
            lens = [n - 1 for n in src_len]
            y_true = tgt[:, 1:]
            if random_seed is not None:
                idx, y_list, out_len = library.query_random(B, lens, int(random_seed) + n_batch, first=random_first, L=Lo)
            else:
                idx, _, found, y_list, out_len = library.query(_baseline_features(library, src_s_v, src_s_a), src_len, k=k,
                                                               out_lens=lens, L=Lo)
                found_h = found.cpu().tolist()
                if k > 1 and min(found_h) < k:
                    raise ValueError("evaluate_baseline_epoch(k=%d): a clip of batch %d has only %d eligible library entries"
                                     % (k, n_batch, min(found_h)))
                if min(found_h) == 0:      # k = 1: the reference keeps best_index = 0 (dimx.retrieval.reference_index)
                    idx = idx.clamp(min=0)
                    y_list, out_len = op_nn_gather(lib_seq, lib_lens, idx, lens, L=Lo)
            n_h = out_len.min(dim=1)[0].cpu().tolist()
            keep = list(range(B))
            if strict_len:
                same = (lib_lens[idx.long()] == torch.tensor(lens, dtype=torch.int32, device=idx.device)[:, None]).all(dim=1).cpu().tolist()
                keep = [j for j in keep if same[j]]
            if not keep:
                continue
            if len(keep) < B:
                kj = torch.tensor(keep, device=y_list.device)
                y_true, y_list, x = y_true[kj], y_list[kj], src_s_v[kj]
            else:
                x = src_s_v
            n_k = [n_h[j] for j in keep]
            if k == 1:
                ok = torch.ones(len(keep), dtype=torch.uint8, device=y_list.device)
                best = _winners_to_host(y_true, y_list, ok, y_list[:, 0], n_k, 1, device, None, metrics, x)
            elif select == "fd":
                best = _select_hip(y_true, y_list, n_k, 1, device, None, metrics=metrics, x=x)
            else:
                best = _select_consensus(y_true, y_list, consensus_distance, n_k, 1, device, None, metrics=metrics, x=x)
            yt, xs = y_true.cpu().numpy(), x.cpu().numpy()
            for i, j in enumerate(keep):
                y_trues_all.append(yt[i][:n_k[i]])
                y_preds_all.append(best[i])
                x_all.append(xs[i][:n_k[i]])
                data_ids_all.append(data_ids[j])
    return y_trues_all, y_preds_all, x_all, data_ids_all


# speaker id of a BIWI recording, keyed on the part of the file name before the first '_' (reference code/x_engine_pt.py:286-301)
BIWI_SPEAKER_IDS = {"F2": 0, "F3": 1, "F4": 2, "M3": 3, "M4": 4, "M5": 5, "F1": 6, "F5": 7, "F6": 8, "F7": 9, "F8": 10, "M1": 11,
                    "M2": 12, "M6": 13}


def evaluate_test_epoch_biwi(model, loader, device, beam_size=10, filter_logits_fn=None, filter_kwargs=None):
    """reference code/x_engine_pt.py:279-338, restated with its quirks.  The loader yields ``(xa [B,T,768] audio, xv [B,T,V]
    vertices, xt [B,V] template, xe [B,T,56] EMOCA, data_ids)``; the mask is all ones; the model runs ``beam_size`` times in
    ``mode='train'`` (teacher forcing: every pass of a deterministic model gives the same prediction); per clip the candidate with
    the smallest ``mean_t ||pred_t - true_t||_2`` is kept, a later candidate replaces it only when STRICTLY smaller.  ``y_true`` is
    ``xe[:, 1:]`` and is cut by one more frame when stored (and so are the predictions): the stored arrays have T - 2 frames.
    Returns ``(y_trues_all, y_preds_all, x_all, data_ids_all)``; ``x_all`` stays empty.  ``filter_logits_fn`` /
    ``filter_kwargs`` are handed to the model (SpeakerSLMFT.forward); the teacher-forced pass of this protocol samples nothing, so
    they change its result only for a model that generates."""
    fkw = dict(filter_logits_fn=filter_logits_fn, filter_kwargs=filter_kwargs) if (filter_logits_fn is not None or filter_kwargs) else {}
    y_trues_all, y_preds_all, x_all, data_ids_all = [], [], [], []
    model.eval()
    with torch.no_grad():
        for batch in loader:
            xa, xv, xt, xe, data_ids = batch
            xa, xv, xt, xe = xa.to(device), xv.to(device), xt.to(device), xe.to(device)
            y_true = xe[:, 1:, :]
            n = xv.shape[0]
            speaker_ids = torch.tensor([BIWI_SPEAKER_IDS[f.split("_")[0]] for f in data_ids]).long().to(device)
            mask = torch.ones((xa.shape[0], xa.shape[1]), dtype=torch.bool).to(device)
            for j in range(n):
                y_trues_all.append(y_true[j, 1:, :].cpu().numpy())
                data_ids_all.append(data_ids[j])
            cur_best = [float("inf")] * n
            best = [None] * n
            for _ in range(beam_size):
                _, _, y_preds = model(xv, xe, xa, mask, xt, mode="train", speaker_ids=speaker_ids, **fkw)
                for j in range(n):
                    cp = y_preds[j, 1:, :].cpu().numpy()
                    ct = y_true[j, 1:, :].cpu().numpy()
                    distance = np.mean(np.sqrt(np.sum((cp - ct) ** 2, axis=1)))
                    if distance < cur_best[j]:
                        best[j] = cp
                        cur_best[j] = distance
            y_preds_all.extend(best)
    return y_trues_all, y_preds_all, x_all, data_ids_all


MESH_METRIC_BACKENDS = ("hip", "reference")


def evaluate_mesh_epoch(mesh_fn, loader, mouth_map, upper_map, backend="hip"):
    """Lip Vertex Error and upper-Face Dynamics Deviation (reference print_biwi_metrics, code/mymetrics.py:122-182) of whatever
    produces meshes: ``mesh_fn(batch) -> (y_true [B,Lt,3*Nv], y_pred [B,Lp,3*Nv], lens, template [B,3*Nv] or None)`` on a GPU, the
    first ``lens[b]`` frames of clip b counting.  ``backend="hip"``: dimx.metrics.BiwiMeshMetrics -- the meshes stay on the GPU,
    float64, one readback at the end.  ``backend="reference"``: every mesh is copied to the host and
    dimx.mymetrics.compute_biwi_metrics runs on float64 copies of the f32 values -- what the operator is defined as; the slow
    check.  Any other value raises ValueError.
    Returns ``(lve, fdd)`` as floats."""
    if backend not in MESH_METRIC_BACKENDS:
        raise ValueError("backend=%r: one of %s" % (backend, ", ".join(MESH_METRIC_BACKENDS)))
    if backend == "hip":
        from .metrics import BiwiMeshMetrics
        acc = BiwiMeshMetrics(mouth_map, upper_map)
        for batch in loader:
            acc.update(*mesh_fn(batch))
        return acc.result()
    from .mymetrics import compute_biwi_metrics
    gts, preds, templs = [], [], []
    for batch in loader:
        y_true, y_pred, lens, template = mesh_fn(batch)
        for j, n in enumerate(lens):
            gts.append(y_true[j, :int(n)].cpu().double().numpy())
            preds.append(y_pred[j, :int(n)].cpu().double().numpy())
            templs.append(None if template is None else template[j].cpu().double().numpy())
    if all(t is None for t in templs):
        templs = None
    m = compute_biwi_metrics(gts, preds, None, templs, mouth_map, upper_map)
    return float(m["lve"]), float(m["fdd"])


def evaluate_mesh_epoch_biwi(model, loader, device, mouth_map, upper_map, backend="hip"):
    """The mesh metrics of a ``SpeakerSLMFT`` over the BIWI batches ``evaluate_test_epoch_biwi`` takes (``(xa, xv, xt, xe, ids)``):
    one teacher-forced ``forward(..., mode="train", return_mesh=True)`` per batch (the model is deterministic: no beam), the mesh
    [B,T-1,V] against ``xv[:, 1:]`` (a view, not a copy) with the template ``xt`` -> ``(lve, fdd)``; backends as
    ``evaluate_mesh_epoch``."""
    if backend not in MESH_METRIC_BACKENDS:
        raise ValueError("backend=%r: one of %s" % (backend, ", ".join(MESH_METRIC_BACKENDS)))
    model.eval()

    def mesh_fn(batch):
        xa, xv, xt, xe, data_ids = batch
        xa, xv, xt, xe = xa.to(device), xv.to(device), xt.to(device), xe.to(device)
        speaker_ids = torch.tensor([BIWI_SPEAKER_IDS[f.split("_")[0]] for f in data_ids]).long().to(device)
        mask = torch.ones((xa.shape[0], xa.shape[1]), dtype=torch.bool).to(device)
        mesh = model(xv, xe, xa, mask, xt, mode="train", speaker_ids=speaker_ids, return_mesh=True)[-1]
        return xv[:, 1:], mesh, [mesh.shape[1]] * mesh.shape[0], xt

    with torch.no_grad():
        return evaluate_mesh_epoch(mesh_fn, loader, mouth_map, upper_map, backend=backend)


last_eval_report = {}


def _report_epoch(model, device, what, n_clips, fd_backend=None):
    """What an evaluation epoch leaves behind besides its lists (the reference's return value is kept as it is): the number of
    generate() calls whose XCD-local chain kernels reported a fault and were repaired by regeneration (csrc/chain.hip) -- a handle
    on a shared / partitioned GPU silently takes the slower step from then on, so the epoch says so."""
    faults = 0
    try:
        eng = model.engine(device) if hasattr(model, "engine") else None
        faults = int(eng.chain_faults()) if eng is not None and hasattr(eng, "chain_faults") else 0
    except Exception:   # a stub model of the host-protocol tests has no engine
        faults = 0
    last_eval_report.clear()
    last_eval_report.update(epoch=what, clips=int(n_clips), chain_faults=faults, fd_backend=fd_backend, world_size=ddist.world_size())
    if faults:
        import warnings
        warnings.warn("%s: %d generate() call(s) of this handle reported a chain-kernel fault; those batches were regenerated on the "
                      "one-kernel-per-op step and the handle keeps that (slower) step" % (what, faults))
    return last_eval_report


def generate_sharded(model, v_speaker, v_listener, v_audio, mask, **forward_kw):
    """One evaluation batch across the ranks of the default process group: every rank receives the FULL
    batch (or just its shard with ``pre_sharded=True``), evaluates rows [lo, hi) and the generated code indices +
    decoded coefficients are all-gathered (RCCL over xGMI on GPUs).  The shard is run with
    ``batch_row_offset=lo`` (the VQ decoder's batch-row positional quirk) and ``shard=(lo, B)`` (the sampler's
    counter-based generator is indexed by the global row), so the gathered result equals the single-process
    result for the same seed / injected noise.  ``filter_logits_fn`` / ``filter_kwargs`` (the sampler filter, SLMFT.forward)
    travel in ``forward_kw`` like every other argument of the forward pass: the filter acts on a row's own logits, so a rank
    filters what the single-process batch would.  Returns (tokens [B,T-1] int32, pred [B,T-1,56]) on every rank."""
    pre_sharded = forward_kw.pop("pre_sharded", False)
    rank, world = ddist.rank(), ddist.world_size()
    if pre_sharded:
        counts = ddist.all_gather_counts(v_speaker.shape[0], v_speaker.device)
        lo, total = sum(counts[:rank]), sum(counts)
    else:
        total = v_speaker.shape[0]
        lo, hi = ddist.shard_bounds(total, rank, world)
        noise = forward_kw.get("noise")
        if noise is not None:                       # injected sampling noise [T-1, B, 512]: this shard's columns
            forward_kw["noise"] = noise[:, lo:hi].contiguous()
        v_speaker, v_listener, v_audio, mask = (t[lo:hi].contiguous() for t in (v_speaker, v_listener, v_audio, mask))
    if world > 1:
        forward_kw.setdefault("batch_row_offset", lo)
        forward_kw.setdefault("shard", (lo, total))
    if v_speaker.shape[0] > 0:
        _, _, pred, tokens = model(v_speaker, v_listener, v_audio, mask, mode="val", return_tokens=True, **forward_kw)
    else:
        T = v_speaker.shape[1]
        pred = torch.zeros(0, T - 1, v_listener.shape[2], device=v_speaker.device)
        tokens = torch.zeros(0, T - 1, dtype=torch.int32, device=v_speaker.device)
    # ONE collective: the code indices and the decoded coefficients travel in the same buffer; the shard sizes follow from
    # shard_bounds on every rank (pre_sharded callers exchanged theirs above), so nothing synchronises with the host first
    if world > 1:
        counts = counts if pre_sharded else ddist.shard_counts(total)
        Tm1, F = pred.shape[1], pred.shape[2]
        buf = ddist.all_gather_rows(ddist.pack_rows(tokens.to(torch.int32), pred.float()), counts)
        tokens, pred = ddist.unpack_rows(buf, [((Tm1,), torch.int32), ((Tm1, F), torch.float32)])
    else:
        tokens = tokens.to(torch.int32)
    return tokens, pred


def _set_epoch(loader, epoch):
    """a DistributedSampler reshuffles per epoch only when told the epoch (otherwise every epoch replays the same order and
    every rank keeps the same fixed subset)."""
    sampler = getattr(loader, "sampler", None)
    if sampler is not None and hasattr(sampler, "set_epoch"):
        sampler.set_epoch(epoch)


def _adopt_hyperparameters(trainer, optimizer):
    """lr / betas / eps / weight_decay of a torch.optim.AdamW, read from its param_groups at every step (so a torch LR scheduler
    attached to that optimizer drives the HIP step)."""
    g = optimizer.param_groups[0]
    trainer.lr, trainer.betas, trainer.eps, trainer.weight_decay = float(g["lr"]), tuple(g["betas"]), float(g["eps"]), float(g["weight_decay"])


def _is_dimx_model(model):
    """a module of this package (it owns an engine on libdimx_hip.so), as opposed to any other nn.Module handed to the loops"""
    inner = getattr(model, "module", model)
    return getattr(inner, "engine_variant", None) is not None and hasattr(inner, "engine")


def _no_hip_step(model, what, log):
    """backward='auto' and no HIP step for this call.  A model of this package must not change backend behind the caller's back
    (VERDICT round 4): the call raises with the reason, and ``backward='autograd'`` selects the PyTorch-autograd restatement (the
    checker of the HIP step) explicitly.  Any other nn.Module (the reference's loops are generic) has no HIP backend to leave: it
    runs on torch as the reference would."""
    why = getattr(_hip_trainer_for, "last_reason", None) or "no HIP training step"
    if _is_dimx_model(model):
        raise L.DimxError("%s(backward='auto'): %s.  The HIP training step is the product path; pass backward='autograd' to run the "
                          "PyTorch-autograd restatement (its checker) on purpose" % (what, why))
    log("%s: %s is not a dimx model -- the reference loop on torch autograd" % (what, type(getattr(model, "module", model)).__name__))


def _hip_trainer_for(model, optimizer, device, log):
    """The HIP trainer that stands in for ``optimizer`` (a torch.optim.AdamW over this module's parameters), or None when the
    reference call cannot be mapped onto a HIP step (the reason is left in ``_hip_trainer_for.last_reason``; see _no_hip_step).
    SLMFT -> HipTrainer, SLM -> SlmHipTrainer, the legacy ListenerGenerator -> LegacyHipTrainer (dimx.x_engine.train_epoch),
    SpeakerSLMFT -> SpeakerHipTrainer (train_epoch_biwi).
    Cached on the module per optimizer object: the AdamW moments and the step count live in the trainer's flat arenas between
    epochs and are exported into ``optimizer.state`` at the end of every epoch (``optimizer.state_dict()`` stays meaningful)."""
    from . import train_hip
    inner = getattr(model, "module", model)
    why = None
    cls = {"slmft": train_hip.HipTrainer, "slm": train_hip.SlmHipTrainer, "legacy": train_hip.LegacyHipTrainer,
           "speaker": train_hip.SpeakerHipTrainer}.get(getattr(inner, "engine_variant", None))
    if cls is train_hip.SpeakerHipTrainer and not hasattr(inner, "speaker_embed"):
        cls = None      # EmocaConverter shares the engine variant; its own loop is ConverterHipTrainer's (examples/train_converter.py)
    if cls is None or not hasattr(inner, "engine"):
        why = "no HIP training step for %s" % type(inner).__name__
    elif type(optimizer) is not torch.optim.AdamW:
        why = "optimizer %s is not torch.optim.AdamW" % type(optimizer).__name__
    elif torch.device(device).type != "cuda" or next(inner.parameters()).device.type != "cuda":
        why = "module / device not on a ROCm GPU"
    else:
        gs = optimizer.param_groups
        keys = ("lr", "betas", "eps", "weight_decay")
        if any(g.get("amsgrad") or g.get("maximize") for g in gs):
            why = "amsgrad / maximize are not implemented in dimx_train_adamw"
        elif any(tuple(map(str, (g[k] for k in keys))) != tuple(map(str, (gs[0][k] for k in keys))) for g in gs[1:]):
            why = "param_groups with different hyper-parameters"
    if why is None:
        cached = getattr(inner, "_dimx_hip_trainer", None)
        if cached is not None and cached[0] is optimizer:
            return cached[1]
        tr = cls(inner, device=device)
        have = {id(p) for g in optimizer.param_groups for p in g["params"]}
        named = dict(inner.named_parameters())
        missing = [n for n, _, _ in tr.layout if id(named[n]) not in have]
        if missing:
            why = "the optimizer does not hold %d of the %d trained tensors (first: %s)" % (len(missing), len(tr.layout), missing[0])
        else:
            tr.import_optimizer_state(optimizer)
            inner._dimx_hip_trainer = (optimizer, tr)
            return tr
    _hip_trainer_for.last_reason = why
    return None


def _train_epoch_hip(model, loader, trainer, device, scheduler, print_freq, epoch, log, clip=None, optimizer=None):
    """train_epoch on the hand-written HIP training step (dimx.train_hip.HipTrainer): forward, backward, the gradient
    all-reduce (one flat RCCL collective), clipping and AdamW all run in libdimx_hip.so; the loop only feeds batches.  The
    trained parameters are written back into the module at the end of the epoch (evaluation / state_dict see them).
    ``clip`` (when given) is the reference's argument and replaces the trainer's own; ``optimizer`` (a torch.optim.AdamW the
    trainer stands in for) supplies lr / betas / eps / weight_decay per step and receives the moments at the end."""
    model.train()
    changed = trainer.refresh_from_model_if_changed()
    if changed:
        log("train_epoch: the module's parameters changed since the HIP trainer last synchronised (load_state_dict?): arena reloaded from the module")
    if optimizer is not None and type(optimizer) is torch.optim.AdamW and (changed or trainer.optimizer_state_changed(optimizer)):
        # optimizer.load_state_dict / an autograd epoch in between: the arenas' moments and step count are stale, and exporting
        # them at the end of this epoch would overwrite the optimizer's fresh state
        trainer.import_optimizer_state(optimizer)
        log("train_epoch: the optimizer's state changed since the HIP trainer last exported it: moments and step count re-imported")
    if clip is not None:
        trainer.clip = float(clip)
    if scheduler is not None and optimizer is None:
        optimizer = getattr(scheduler, "optimizer", None)
        if optimizer is None or not hasattr(optimizer, "param_groups"):
            raise L.DimxError("train_epoch: a scheduler needs a torch optimizer whose param_groups carry the learning rate; "
                              "build it on torch.optim.AdamW and pass that optimizer, or set trainer.lr yourself")
    if ddist.world_size() > 1 and hasattr(loader, "__len__"):
        ddist.assert_same_batch_count(len(loader), device)
    _set_epoch(loader, epoch)
    losses, parts, all_losses = [], {}, []
    for i, batch in enumerate(loader):
        src_s_v, src_s_a, tgt, mask, _, _ = _prepare(batch, device)
        if optimizer is not None:
            _adopt_hyperparameters(trainer, optimizer)
            optimizer._opt_called = True      # the trainer steps in its place (silences torch's scheduler-before-optimizer warning)
        loss, d_step = trainer.train_step(src_s_v, tgt, src_s_a, mask, with_cont_loss=True)   # the reference's total loss
        if scheduler is not None:
            scheduler.step()
        losses.append(loss)                      # device scalars: no host synchronisation per batch
        for k, v in d_step.items():
            if torch.is_tensor(v):
                parts.setdefault(k, []).append(v)
        if i % print_freq == 0:
            vals = [float(v) for v in torch.stack(losses).cpu()]
            all_losses += vals
            log("Epoch %d Batch %d:\tLoss %.4f\t" % (epoch, i, float(np.mean(vals))) +
                "\t".join("%s %.4f" % (k, float(torch.stack(v).mean())) for k, v in parts.items()))
            losses, parts = [], {}
    if losses:
        all_losses += [float(v) for v in torch.stack(losses).cpu()]
    trainer.sync_to_model()
    if optimizer is not None and type(optimizer) is torch.optim.AdamW:
        trainer.export_optimizer_state(optimizer)
    return float(np.mean(all_losses)) if all_losses else float("nan")


def train_epoch(model, loader, optimizer, device, scheduler=None, clip=None, print_freq=2000, epoch=0, log=print, backward="auto",
                lookahead=None, cond_drop=None, seed=20260928):
    """reference code/x_engine_pt.py:9-60: one pass over the loader with zero_grad / forward(mode='train') / backward /
    clip / step (``clip`` None = the reference's default 0., no clipping).

    The reference's own call -- ``train_epoch(model, loader, torch.optim.AdamW(model.parameters(), lr=1e-5), device, clip=1.0)``
    (code/finetune_s2s_pretrain.py:118-132) -- lands on the hand-written HIP training step: for an SLMFT on a GPU a
    ``HipTrainer`` stands in for the AdamW (hyper-parameters read from its param_groups at every step, so torch schedulers
    work; moments exported into ``optimizer.state`` after the epoch; ``sync_to_model()`` at the end of the epoch).  A
    ``HipTrainer`` may also be passed as ``optimizer`` directly.  ``backward="auto"`` (default) and ``"hip"`` RAISE when a model
    of this package cannot be stepped by the HIP kernels (another optimiser class, amsgrad, unequal param_groups, CPU tensors):
    the PyTorch-autograd restatement (dimx.train) is the checker of the HIP path and runs only with ``backward="autograd"``.  For N > 1 processes the gradients are averaged over RCCL before
    clipping; every rank feeds its own loader shard (get_vico_dataloaders shards the training loaders by rank; the sampler is
    told the epoch here); the ranks must see the same number of batches (checked) and start from rank 0's parameters.

    ``lookahead`` L (SLMFT only): online fine-tuning -- every step trains under the visibility of an online generation with the
    same L (dimx.online: decoder row t sees the context rows below clamp(t + 2 + L, 1, T)), on the HIP step
    (``HipTrainer.set_lookahead``) and on the autograd route (``dimx.train.slmft_loss(lookahead=L)``) alike.  None: the
    reference's offline step; a ``HipTrainer`` passed as ``optimizer`` then keeps its own setting.

    ``cond_drop`` p (SLMFT only): condition dropout for classifier-free guidance (dimx.guidance) -- every step trains each clip under
    the null context with probability p, drawn by ``dimx.guidance.cond_keep(seed, step, B, p)``: on the HIP step
    (``HipTrainer(cond_drop=)``, dimx_set_train_cond_keep) and on the autograd route (``dimx.train.slmft_loss(cond_keep=)``) alike.
    None: a ``HipTrainer`` passed as ``optimizer`` keeps its own setting, every other route trains without it."""
    from .seq2seq_pretrain import SLMFT
    from .train_hip import HipTrainer
    inner = getattr(model, "module", model)
    if lookahead is not None and not isinstance(inner, SLMFT):
        raise L.DimxError("train_epoch(lookahead=...): online fine-tuning is built for SLMFT, not %s" % type(inner).__name__)
    if cond_drop is not None and not isinstance(inner, SLMFT):
        raise L.DimxError("train_epoch(cond_drop=...): condition dropout is built for SLMFT, not %s" % type(inner).__name__)
    if isinstance(optimizer, HipTrainer):
        if lookahead is not None:
            optimizer.set_lookahead(lookahead)
        if cond_drop is not None:
            optimizer.cond_drop, optimizer.cond_seed = float(cond_drop), int(seed)
        return _train_epoch_hip(model, loader, optimizer, device, scheduler, print_freq, epoch, log, clip=clip)
    if backward not in ("auto", "hip", "autograd"):
        raise ValueError("backward must be 'auto', 'hip' or 'autograd'")
    if backward != "autograd":
        tr = _hip_trainer_for(model, optimizer, device, log)
        if tr is not None:
            if type(tr) is HipTrainer:        # the cached stand-in follows this call's argument, None included
                tr.set_lookahead(lookahead)
                tr.cond_drop, tr.cond_seed = float(cond_drop or 0.0), int(seed)
            return _train_epoch_hip(model, loader, tr, device, scheduler, print_freq, epoch, log,
                                    clip=0.0 if clip is None else clip, optimizer=optimizer)
        if backward == "hip":
            raise L.DimxError("train_epoch(backward='hip'): %s" % _hip_trainer_for.last_reason)
        _no_hip_step(model, "train_epoch", log)     # raises for a dimx model: the autograd route is an explicit opt-in
    from . import train as T                        # the PyTorch-autograd restatement: imported only when it is asked for
    clip = 0.0 if clip is None else clip
    _set_epoch(loader, epoch)
    model.train()
    # what the reference trains differs per model: SLMFT freezes both VQ-VAEs (:348-366), SLM only their encoders + codebooks (:98-113)
    named = inner.dimx_trainable_parameters() if hasattr(inner, "dimx_trainable_parameters") else T.trainable_parameters(model)
    for _, p in named:
        p.requires_grad_(True)
    params = [p for _, p in named]
    if ddist.world_size() > 1:
        if hasattr(loader, "__len__"):
            T.assert_same_batch_count(len(loader), device if torch.device(device).type == "cuda" else None)
        if not getattr(model, "_dimx_params_broadcast", False):     # once per model: every rank starts from rank 0's weights
            T.broadcast_parameters(params)
            model._dimx_params_broadcast = True
    d = {k: 0.0 for k in ("l_ce_s", "l_ce_l", "l_cont_s", "l_cont_l", "nce", "c_acc")}
    losses, all_losses = [], []
    for i, batch in enumerate(loader):
        src_s_v, src_s_a, tgt, mask, _, _ = _prepare(batch, device)
        optimizer.zero_grad()
        if lookahead is None and not cond_drop:
            loss, d_step, _ = model(src_s_v, tgt, src_s_a, mask, mode="train")
        else:      # the windowed teacher-forced pass exists with a graph only (SLMFT.forward keeps lookahead for mode='val')
            keep = None
            if cond_drop:
                from .guidance import cond_keep
                step = (epoch * len(loader) if hasattr(loader, "__len__") else 0) + i
                keep = torch.from_numpy(cond_keep(seed, step, mask.shape[0], cond_drop)).to(device)
            loss, d_step, _ = inner._forward_autograd(src_s_v, tgt, src_s_a, mask, lookahead=None if lookahead is None else int(lookahead),
                                                      cond_keep=keep)
        loss.mean().backward()
        T.all_reduce_grads(params)
        if clip > 0:
            torch.nn.utils.clip_grad_norm_(params, clip)
        optimizer.step()
        if scheduler is not None:
            scheduler.step()
        for k in d:
            v = d_step.get(k, 0)
            d[k] += float(v.mean().item()) if torch.is_tensor(v) else float(v)
        losses.append(float(loss.mean().item()))
        all_losses.append(losses[-1])
        if i % print_freq == 0:
            log("Epoch %d Batch %d:\tLoss %.4f\t" % (epoch, i, float(np.mean(losses))) +
                "\t".join("%s %.4f" % (k, d[k] / print_freq) for k in d))
            d = {k: 0.0 for k in d}
            losses = []
    return float(np.mean(all_losses)) if all_losses else float("nan")


_BIWI_KEYS = ("l_ce_s", "l_ce_l", "l_cont_s", "l_cont_l", "nce", "c_acc")
_BIWI_LABELS = ("CE_s", "CE_l", "Cont_s", "Cont_l", "NCE", "C_acc")


def _biwi_line(epoch, i, loss, d):
    """the reference loop's progress line (code/x_engine_pt.py:124)"""
    return "Epoch %d Batch %d:\tLoss %.4f\t" % (epoch, i, loss) + "\t".join("%s %.4f" % (lab, d[k]) for lab, k in zip(_BIWI_LABELS, _BIWI_KEYS))


def _biwi_batch(batch, device):
    xa, xv, xt, xe, fnames = batch
    xa, xv, xt, xe = (t.to(device, non_blocking=True) for t in (xa, xv, xt, xe))
    speaker_ids = torch.tensor([BIWI_SPEAKER_IDS[f.split("_")[0]] for f in fnames], dtype=torch.long).to(device)
    mask = torch.ones((xa.shape[0], xa.shape[1]), dtype=torch.bool, device=device)
    return xa, xv, xt, xe, speaker_ids, mask


def _train_epoch_biwi_hip(model, loader, trainer, device, scheduler, print_freq, epoch, log, clip=None, optimizer=None):
    """train_epoch_biwi on the hand-written HIP step (dimx.train_hip.SpeakerHipTrainer); same hand-over of hyper-parameters,
    optimiser state and trained weights as _train_epoch_hip."""
    model.train()
    changed = trainer.refresh_from_model_if_changed()
    if changed:
        log("train_epoch_biwi: the module's parameters changed since the HIP trainer last synchronised (load_state_dict?): arena reloaded from the module")
    if optimizer is not None and type(optimizer) is torch.optim.AdamW and (changed or trainer.optimizer_state_changed(optimizer)):
        trainer.import_optimizer_state(optimizer)
        log("train_epoch_biwi: the optimizer's state changed since the HIP trainer last exported it: moments and step count re-imported")
    if clip is not None:
        trainer.clip = float(clip)
    if scheduler is not None and optimizer is None:
        optimizer = getattr(scheduler, "optimizer", None)
        if optimizer is None or not hasattr(optimizer, "param_groups"):
            raise L.DimxError("train_epoch_biwi: a scheduler needs a torch optimizer whose param_groups carry the learning rate; "
                              "build it on torch.optim.AdamW and pass that optimizer, or set trainer.lr yourself")
    if ddist.world_size() > 1 and hasattr(loader, "__len__"):
        ddist.assert_same_batch_count(len(loader), device)
    _set_epoch(loader, epoch)
    losses, parts, all_losses = [], {k: [] for k in _BIWI_KEYS}, []
    for i, batch in enumerate(loader):
        xa, xv, xt, xe, speaker_ids, mask = _biwi_batch(batch, device)
        if optimizer is not None:
            _adopt_hyperparameters(trainer, optimizer)
            optimizer._opt_called = True      # the trainer steps in its place (silences torch's scheduler-before-optimizer warning)
        loss, d_step = trainer.train_step(xv, xe, xa, mask, xt, speaker_ids=speaker_ids)
        if scheduler is not None:
            scheduler.step()
        losses.append(loss)                      # device scalars: no host synchronisation per batch
        for k in _BIWI_KEYS:
            if torch.is_tensor(d_step[k]):
                parts[k].append(d_step[k])
        if i % print_freq == 0:
            vals = [float(v) for v in torch.stack(losses).cpu()]
            all_losses += vals
            # the reference divides its running sums by print_freq, whatever the number of batches behind them
            log(_biwi_line(epoch, i, float(np.mean(vals)), {k: (float(torch.stack(v).sum()) / print_freq if v else 0.0) for k, v in parts.items()}))
            losses, parts = [], {k: [] for k in _BIWI_KEYS}
    if losses:
        all_losses += [float(v) for v in torch.stack(losses).cpu()]
    trainer.sync_to_model()
    if optimizer is not None and type(optimizer) is torch.optim.AdamW:
        trainer.export_optimizer_state(optimizer)
    return float(np.mean(all_losses)) if all_losses else float("nan")


def _speaker_codes(model, P, xe, mask):
    """[B,T] codes of the frozen listener VQ-VAE for the autograd route: the HIP engine's on a GPU (what SpeakerSLMFT.forward
    uses), the torch restatement of the same encoder on the CPU (each clip alone, as the reference encodes them)"""
    from . import train as T
    if xe.is_cuda:
        return model.forward_vq(None, xe, mask)[1]
    B, Tn = mask.shape
    z = torch.full((B, Tn), -100, dtype=torch.long)
    Pd = {k: v.detach() for k, v in P.items() if k.startswith("listener_vq.")}
    for b in range(B):
        n = int(mask[b].sum())
        z[b, :n] = T.vq_loss(Pd, xe[b:b + 1, :n].float(), pre="listener_vq.", heads=model.vq_dims.heads, layers=model.vq_dims.layers)[5]
    return z


def train_epoch_biwi(model, loader, optimizer, device, scheduler=None, clip=0.0, print_freq=2000, epoch=0, log=print, backward="auto"):
    """reference code/x_engine_pt.py:62-132: one pass of the DIM-Speaker fine-tuning over a loader that yields ``(xa [B,T,768]
    audio, xv [B,T,V] vertices, xt [B,V] template, xe [B,T,56] EMOCA, file names)``; the mask is all ones and the speaker ids
    come from the file-name prefix (``BIWI_SPEAKER_IDS``).  Per batch: zero_grad / ``model(xv, xe, xa, mask, xt,
    speaker_ids=...)`` / backward / clip (after backward, so it really clips) / step, and the reference's progress line.

    ``optimizer`` is a ``torch.optim.AdamW`` over the model's parameters (the reference's call: a ``SpeakerHipTrainer`` then
    stands in for it exactly as ``train_epoch`` arranges it for SLMFT) or a ``SpeakerHipTrainer``.  ``backward="auto"`` /
    ``"hip"`` RAISE when a model of this package cannot be stepped by the HIP kernels; ``backward="autograd"`` runs the
    PyTorch-autograd restatement ``dimx.train.speaker_loss`` (the checker of the HIP step) on purpose.  Deliberate differences
    from the reference are listed in ``SpeakerHipTrainer``'s docstring; the reference's ``evaluate_epoch_biwi`` is not built."""
    from .train_hip import HipTrainer
    if isinstance(optimizer, HipTrainer):
        return _train_epoch_biwi_hip(model, loader, optimizer, device, scheduler, print_freq, epoch, log, clip=clip)
    if backward not in ("auto", "hip", "autograd"):
        raise ValueError("backward must be 'auto', 'hip' or 'autograd'")
    inner = getattr(model, "module", model)
    if backward != "autograd":
        tr = _hip_trainer_for(model, optimizer, device, log) if hasattr(inner, "speaker_embed") else None
        if tr is not None:
            return _train_epoch_biwi_hip(model, loader, tr, device, scheduler, print_freq, epoch, log, clip=clip, optimizer=optimizer)
        if not hasattr(inner, "speaker_embed"):
            _hip_trainer_for.last_reason = "no HIP fine-tuning step for %s (train_epoch_biwi steps a SpeakerSLMFT)" % type(inner).__name__
        if backward == "hip":
            raise L.DimxError("train_epoch_biwi(backward='hip'): %s" % _hip_trainer_for.last_reason)
        _no_hip_step(model, "train_epoch_biwi", log)     # raises for a dimx model: the autograd route is an explicit opt-in
    from . import train as T
    import torch.nn.functional as F
    _set_epoch(loader, epoch)
    model.train()
    if not _is_dimx_model(model):                        # any other nn.Module: the reference's loop as it stands, on torch
        losses = []
        for i, batch in enumerate(loader):
            xa, xv, xt, xe, speaker_ids, mask = _biwi_batch(batch, device)
            optimizer.zero_grad()
            loss, d_step, _ = model(xv, xe, xa, mask, xt, speaker_ids=speaker_ids)
            loss.mean().backward()
            if clip > 0:
                torch.nn.utils.clip_grad_norm_(model.parameters(), clip)
            optimizer.step()
            if scheduler is not None:
                scheduler.step()
            losses.append(float(loss.mean()))
            if i % print_freq == 0:
                log(_biwi_line(epoch, i, float(np.mean(losses)), {k: (float(torch.as_tensor(d_step.get(k, 0)).float().mean()) / print_freq) for k in _BIWI_KEYS}))
        return float(np.mean(losses)) if losses else float("nan")
    if not hasattr(inner, "speaker_embed"):
        raise L.DimxError("train_epoch_biwi(backward='autograd'): dimx.train.speaker_loss restates SpeakerSLMFT, not %s" % type(inner).__name__)
    named = inner.dimx_trainable_parameters()
    for _, p in named:
        p.requires_grad_(True)
    params = [p for _, p in named]
    d = {k: 0.0 for k in _BIWI_KEYS}
    losses, all_losses = [], []
    for i, batch in enumerate(loader):
        xa, xv, xt, xe, speaker_ids, mask = _biwi_batch(batch, device)
        P = dict(inner.state_dict(keep_vars=True))
        with torch.no_grad():
            z = _speaker_codes(inner, P, xe, mask).to(xe.device)
        optimizer.zero_grad()
        with torch.enable_grad():
            loss, o = T.speaker_loss(P, inner.s2s, inner.vq_dims, xe.float(), xa.float(), mask, z, P["speaker_vq.decoder.decoder_pos_embedding.pe"],
                                     speaker_ids=speaker_ids)
            loss.backward()
        T.all_reduce_grads(params)
        if clip > 0:
            torch.nn.utils.clip_grad_norm_(params, clip)
        optimizer.step()
        if scheduler is not None:
            scheduler.step()
        l_mouth = 0.0
        if inner.mouth_map is not None:     # the reported mouth term: the converter head on the decoded coefficients, no graph
            with torch.no_grad():
                mesh = T.converter_head({k: v.detach() for k, v in P.items()}, o["pred"].detach()) + xt[:, None, :]
                B, n = mesh.shape[:2]
                idx = torch.as_tensor(inner.mouth_map, device=mesh.device, dtype=torch.long)
                l_mouth = float(F.mse_loss(mesh.view(B, n, -1, 3)[:, :, idx, :], xv[:, 1:].reshape(B, n, -1, 3)[:, :, idx, :].to(mesh.dtype)))
        d["l_ce_l"] += float(o["l_ce"].detach())
        d["l_cont_l"] += float(o["l_emoca"].detach())
        d["l_cont_s"] += l_mouth
        losses.append(float(loss.detach()))
        all_losses.append(losses[-1])
        if i % print_freq == 0:
            log(_biwi_line(epoch, i, float(np.mean(losses)), {k: d[k] / print_freq for k in d}))
            d = {k: 0.0 for k in d}
            losses = []
    return float(np.mean(all_losses)) if all_losses else float("nan")
