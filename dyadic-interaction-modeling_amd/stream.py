"""Streaming sessions: the schedule (plain numpy, no GPU needed) of the decode steps of a generation whose speaker frames
arrive in pieces (dimx_stream_begin / push / end, include/dimx.h; csrc/stream.hip).

``dimx.online.visible`` stays the definition of what decode step t may read.  A session adds only *when* the step runs.  Step t
consumes the listener token at position t and produces position t+1; it runs as soon as the frames 0 .. t + 1 + max(L, 0)
exist: it waits for its look-ahead buffer, and it never runs ahead of real time -- the token of position t+1 is not produced
before frame t+1 is there.  With L < 0 the step runs at the same moment as with L = 0 and reads the fewer rows
``online.visible`` gives it.  ``end`` fixes T = the frames pushed, and every remaining step up to T - 2 runs.

A session fed a clip in pieces, in any chunking, emits the tokens of ``Engine.generate(lookahead=L)`` on the whole clip.

A session may also start from a prompt (dimx_stream_begin_prompted): its first F frames and first P listener codes are given, the
positions 0 .. P - 2 are prefilled in one teacher-forced pass under the window, and the first decode step is P - 1
(``done0`` below).  Teacher-forced row P - 2 reads the keys below P + L, which must be among the F frames: ``prompt_fits``.  That
is the state a session with look-ahead L >= 0 is in after F frames (F - L codes known), so carrying the last K frames and their
K - max(L, 0) codes into a new session is always a valid start.  Such a session emits the tokens of
``Engine.generate(prompt=codes[:, :P], lookahead=L)`` on the clip of the frames given plus the frames pushed.
"""
import numpy as np


def steps_due(n_frames, lookahead, ended=False, T=None, done0=0):
    """Decode steps that must have run once ``n_frames`` speaker frames are there: the steps 0 .. steps_due - 1.
    Open session: clamp(n_frames - 1 - max(L, 0), 0, n_frames - 1).  After ``end`` (``T`` = the frames pushed, default
    ``n_frames``): T - 1.  ``done0`` = P - 1 for a session begun from a prompt of P codes: the positions below it were
    prefilled, never fewer steps count as done."""
    n = int(n_frames)
    if ended:
        return max(int(done0), int(n if T is None else T) - 1, 0)
    hi = max(n - 1, 0)
    return max(int(done0), int(np.clip(n - 1 - max(int(lookahead), 0), 0, hi)))


def prompt_fits(P, lookahead, F, Tmax=None):
    """May a session start from ``P`` codes and ``F`` frames?  1 <= P and P + max(L, 0) <= F (<= ``Tmax``): every key the
    prefilled rows 0 .. P - 2 read under ``dimx.online.visible`` is one of the frames given, and the prompt's last code is of a
    frame that exists."""
    P, F = int(P), int(F)
    return P >= 1 and P + max(int(lookahead), 0) <= F and (Tmax is None or F <= int(Tmax))


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


def schedule(chunking, lookahead, F=0, P=1):
    """[(frames after the push, first step, one past the last step)] for every push of ``chunking``, then the same for ``end``.
    ``F``, ``P``: the session was begun from F frames and P codes (``prompt_fits``)."""
    out, n, done = [], int(F), int(P) - 1
    for c in chunking:
        n += int(c)
        due = steps_due(n, lookahead, done0=P - 1)
        out.append((n, done, due))
        done = due
    out.append((n, done, steps_due(n, lookahead, ended=True, done0=P - 1)))
    return out
