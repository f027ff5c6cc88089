"""Classifier-free guidance: the definition (numpy float64, no GPU needed) of what sample_guided_kernel (csrc/elementwise.hip),
the guided decode step (csrc/generate.hip, dimx_generate_guided) and the training step's condition dropout compute.

The model is p(listener token | listener tokens so far, speaker context).  Guidance runs the decoder with and without the
context and samples from

    g = cond + (scale - 1) * (cond - uncond)                                   (raw logits, per vocabulary entry)

scale = 1 is the model as it is (g is ``cond`` bit for bit -- the reason this form, and not uncond + scale * (cond - uncond), is
the definition), scale > 1 makes the listener more reactive to the speaker, scale = 0 is the listener's prior.

The null context.  The unconditional branch sees a context of zero rows *after* the concat [x_s + patch_embed_dec_s | audio].
Every cross-attention projection of decoder_joint is bias-free (to_q / to_k / to_v / to_out), so zero rows give K = V = 0, a
uniform softmax over zeros, an attention output of 0 and W_o . 0 = 0: each cross sublayer adds exactly nothing to the residual
stream.  The null context is therefore equivalent to the decoder with its cross sublayers removed, whatever the context mask and
the number of rows -- which is how the device runs it: the unconditional rows skip the sublayer and own no cross K/V.

Order of operations.  Guidance acts on the raw logits; the handle's sampler filter, the temperature and the noise then act on g
exactly as dimx/sampling.py defines them for raw logits; scores (dimx/scoring.py) are taken under softmax(g).

Condition dropout (training).  So that the unconditional branch is something a checkpoint has seen, a training step may replace
the context of whole clips by the null context: clip b keeps its context iff ``cond_keep(seed, step, B, p)[b]``.  There is no
rescaling -- a dropped clip's context is zero, a kept one is unchanged -- and no gradient flows into the context of a dropped clip.
"""
import numpy as np

from . import prng

# The site id of the per-clip draw in dimx.prng.dropout_key: the VQ-VAE's two element-wise sites are 0 and 1 and the key is a
# function of 2 * step + site, so a small id would repeat another site's key of a neighbouring step; this one does not for any
# step below 2^39.
DROPOUT_SITE_COND = 1 << 40


def combine(cond, uncond, scale):
    """cond + (scale - 1) * (cond - uncond) in float64; ``scale`` is taken as the float32 value the kernel receives."""
    s = float(np.float32(scale))
    cond = np.asarray(cond, dtype=np.float64)
    if s == 1.0:
        return cond.copy()
    return cond + (s - 1.0) * (cond - np.asarray(uncond, dtype=np.float64))


def combine_bound(cond, uncond, scale):
    """Per-entry bound on |f32 kernel - combine|: three float32 roundings (c - u, the product, the sum) and that of scale - 1,
    4 * 2^-24 * (|scale - 1| * |cond - uncond| + |g|)."""
    s = float(np.float32(scale))
    c, u = np.asarray(cond, dtype=np.float64), np.asarray(uncond, dtype=np.float64)
    return 4.0 * 2.0 ** -24 * (abs(s - 1.0) * np.abs(c - u) + np.abs(combine(c, u, s)))


def pmi(score_cond, score_null):
    """Pointwise mutual information between a clip's speaker context and the given listener codes, per sequence and per counted
    token: (log p(codes | context) - log p(codes | null context)) / count.  Both arguments are dimx.scoring.SeqScores-like
    (``score`` float64 [R], ``count`` int [R]) over the same columns; a sequence without counted tokens gives 0."""
    sc = np.asarray(_host(score_cond.score), dtype=np.float64)
    sn = np.asarray(_host(score_null.score), dtype=np.float64)
    cc, cn = np.asarray(_host(score_cond.count)), np.asarray(_host(score_null.count))
    assert np.array_equal(cc, cn), "pmi: the two scores count different columns"
    return np.where(cc > 0, (sc - sn) / np.maximum(cc, 1), 0.0)


def _host(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else t


def cond_keep(seed, step, B, p):
    """[B] bool: which clips of training step ``step`` keep their context under condition dropout with probability ``p`` of
    dropping (dimx.prng.dropout_keep's counter-based draw at element (b, 0, 0) of site DROPOUT_SITE_COND)."""
    return prng.dropout_keep(seed, step, DROPOUT_SITE_COND, (int(B), 1, 1), p)[:, 0, 0]
