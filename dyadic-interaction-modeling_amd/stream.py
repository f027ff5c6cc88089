"""Streaming sessions: the schedule (plain numpy, no GPU needed) of the decode steps of a generation whose speaker frames
arrive in pieces (dimx_stream_begin / push / end, include/dimx.h; csrc/stream.hip).

``dimx.online.visible`` stays the definition of what decode step t may read.  A session adds only *when* the step runs.  Step t
consumes the listener token at position t and produces position t+1; it runs as soon as the frames 0 .. t + 1 + max(L, 0)
exist: it waits for its look-ahead buffer, and it never runs ahead of real time -- the token of position t+1 is not produced
before frame t+1 is there.  With L < 0 the step runs at the same moment as with L = 0 and reads the fewer rows
``online.visible`` gives it.  ``end`` fixes T = the frames pushed, and every remaining step up to T - 2 runs.

A session fed a clip in pieces, in any chunking, emits the tokens of ``Engine.generate(lookahead=L)`` on the whole clip.
"""
import numpy as np


def steps_due(n_frames, lookahead, ended=False, T=None):
    """Decode steps that must have run once ``n_frames`` speaker frames are pushed: the steps 0 .. steps_due - 1.
    Open session: clamp(n_frames - 1 - max(L, 0), 0, n_frames - 1).  After ``end`` (``T`` = the frames pushed, default
    ``n_frames``): T - 1."""
    n = int(n_frames)
    if ended:
        return max(int(n if T is None else T) - 1, 0)
    hi = max(n - 1, 0)
    return int(np.clip(n - 1 - max(int(lookahead), 0), 0, hi))


def chunks(T, pattern):
    """The chunk sizes of a clip of ``T`` frames fed by ``pattern``: an integer c (chunks of c frames, the last one shorter) or a
    sequence of sizes that is repeated until the clip is covered (the last chunk is cut to fit)."""
    T = int(T)
    pat = [int(pattern)] if np.ndim(pattern) == 0 else [int(c) for c in pattern]
    if not pat or min(pat) < 1:
        raise ValueError("chunk sizes must be >= 1")
    out, n, i = [], 0, 0
    while n < T:
        c = min(pat[i % len(pat)], T - n)
        out.append(c)
        n += c
        i += 1
    return out


def schedule(chunking, lookahead):
    """[(frames after the push, first step, one past the last step)] for every push of ``chunking``, then the same for ``end``."""
    out, n, done = [], 0, 0
    for c in chunking:
        n += int(c)
        due = steps_due(n, lookahead)
        out.append((n, done, due))
        done = due
    out.append((n, done, steps_due(n, lookahead, ended=True)))
    return out
