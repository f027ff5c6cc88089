"""Online generation: the definition (plain numpy, no GPU needed) of which speaker frames a decode step may see
(dimx_set_cross_lookahead, include/dimx.h; the kernel form is WIN in csrc/decode_attn_body.hpp).

Positions are 0 .. T-1.  Decode step t consumes the listener token at position t and produces position t+1.  With a signed
integer ``lookahead`` L the cross attention of step t attends over the context rows

    j < vis(t) = clamp(t + 2 + L, 1, n_keys)

L = 0: the frame being produced (t+1) and everything before it.  L < 0: a reaction delay of -L frames.  L > 0: a look-ahead
buffer of L frames.  Row 0 is always visible, so no softmax is empty; L >= n_keys - 2 is the offline mode (every row at every
step).  The speaker encoder is causal, so context row j depends on frames <= j only: the token of position t+1 is a function of
the speaker frames below vis(t) and nothing else.

What the mode does not make causal: the audio features are whatever the caller's extractor produced, and the listener VQ-VAE
decoder runs over the whole token sequence.  The guarantee is about the tokens.

This module says what a step may read; *when* a step runs as the frames arrive is dimx/stream.py (streaming sessions).
"""
import numpy as np


def visible(t, lookahead, n_keys):
    """Number of context rows step ``t`` sees; ``t`` may be an integer or an integer array."""
    v = np.clip(np.asarray(t, dtype=np.int64) + 2 + int(lookahead), 1, int(n_keys))
    return int(v) if v.ndim == 0 else v


def visible_mask(T, lookahead, lens=None):
    """[B, T-1, T] boolean: entry [b, t, j] says whether step t of clip b attends to context row j (B = 1 without ``lens``).
    ``lens`` [B]: clip lengths; rows at or past a clip's length are masked as the context mask masks them."""
    T = int(T)
    vis = visible(np.arange(T - 1), lookahead, T)                  # [T-1]
    m = np.arange(T)[None, :] < vis[:, None]                        # [T-1, T]
    if lens is None:
        return m[None]
    lens = np.asarray(lens, dtype=np.int64).reshape(-1)
    return m[None] & (np.arange(T)[None, None, :] < lens[:, None, None])
