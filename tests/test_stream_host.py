"""CPU: the schedule of a streaming session (dimx/stream.py) against the visibility definition (dimx/online.py), and the session's
C-ABI: the built library exports dimx_stream_* and dimx_op_append_attn with the signatures include/dimx.h declares."""
import ctypes
import os
import re

import pytest

import dimx  # noqa: F401
from dimx import lib, online, stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 40
CHUNKINGS = [[1] * 40, [7] * 5 + [5], [16, 16, 8], [17, 1, 22], [40]]
LOOKAHEADS = [-3, 0, 2, 6, 40]


@pytest.mark.parametrize("L", LOOKAHEADS)
@pytest.mark.parametrize("chunking", CHUNKINGS, ids=lambda c: "x".join(map(str, c[:3])) + "_%d" % len(c))
def test_every_step_runs_once_in_order_never_early(chunking, L):
    assert sum(chunking) == T
    ran = []          # (step, frames pushed when it ran, ended)
    n, done = 0, 0
    for c in chunking:
        n += c
        due = stream.steps_due(n, L)
        assert done <= due <= max(n - 1, 0)
        ran += [(t, n, False) for t in range(done, due)]
        done = due
    due = stream.steps_due(n, L, ended=True)
    assert due == T - 1 and stream.steps_due(n, L, ended=True, T=T) == T - 1
    ran += [(t, n, True) for t in range(done, due)]
    assert [t for t, _, _ in ran] == list(range(T - 1))          # every step 0 .. T-2 exactly once, in order
    for t, frames, ended in ran:
        assert t <= frames - 2                                    # position t + 1 is never produced before frame t + 1 exists
        if not ended:
            # what the step reads exists, and under the session's open key bound (any Tmax >= T) it is what the whole clip gives it
            assert online.visible(t, L, T) <= frames
            assert online.visible(t, L, 2048) == online.visible(t, L, T)
        else:
            assert online.visible(t, L, T) <= frames == T
    # the schedule is as early as those two conditions allow: an open step waits for nothing else
    n = 0
    for c in chunking:
        n += c
        for t in range(stream.steps_due(n, L), n - 1):
            assert t + 2 + max(L, 0) > n
    assert stream.schedule(chunking, L)[-1] == (T, done, T - 1)


def test_steps_due_edges():
    assert stream.steps_due(0, 0) == 0 and stream.steps_due(1, 0) == 0 and stream.steps_due(2, 0) == 1
    assert stream.steps_due(2, -5) == 1 and stream.steps_due(10, 3) == 6 and stream.steps_due(3, 40) == 0
    assert stream.steps_due(1, 0, ended=True) == 0 and stream.steps_due(7, 40, ended=True) == 6


def test_chunks():
    assert stream.chunks(40, 7) == [7] * 5 + [5]
    assert stream.chunks(40, [17, 1, 22]) == [17, 1, 22]
    assert stream.chunks(5, [2]) == [2, 2, 1] and stream.chunks(3, 16) == [3]
    with pytest.raises(ValueError):
        stream.chunks(4, 0)


_CTYPE = {"int": ctypes.c_int, "float": ctypes.c_float, "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t,
          "dimx_handle": ctypes.c_void_p}
NEW = ["dimx_stream_workspace_bytes", "dimx_stream_begin", "dimx_stream_push", "dimx_stream_end", "dimx_stream_abort",
       "dimx_stream_state", "dimx_stream_set_events", "dimx_op_append_attn"]


def _declared(hdr, name):
    m = re.search(r"^(\w+)\s+%s\(([^;]*)\);" % name, hdr, re.M)
    assert m, "%s is not declared in include/dimx.h" % name
    res = _CTYPE[m.group(1)]
    args = []
    for p in m.group(2).split(","):
        p = " ".join(p.replace("const", " ").split())
        if p == "int* n_new" or re.fullmatch(r"int\* (frames|steps|open)", p):
            args.append(ctypes.POINTER(ctypes.c_int))
        elif "*" in p:
            args.append(ctypes.c_void_p)
        else:
            args.append(_CTYPE[p.split()[0]])
    return res, args


def test_session_symbols_are_exported_with_the_headers_signatures():
    hdr = open(os.path.join(ROOT, "include", "dimx.h")).read()
    l = lib.load()
    for name in NEW:
        res, args = _declared(hdr, name)
        assert name in lib.SIGNATURES, name
        assert lib.SIGNATURES[name] == (res, args), name
        fn = getattr(l, name)          # AttributeError: the library was not built from these sources
        assert fn.restype is res and list(fn.argtypes) == args
    # the calls that need no device answer before anything is launched
    assert l.dimx_stream_workspace_bytes(None, 1, 8) == 0
    assert l.dimx_stream_abort(None) == -1 and l.dimx_stream_state(None, None, None, None) == -1
    n_new = ctypes.c_int(7)
    assert l.dimx_stream_push(None, None, None, 1, None, 0, None, None, ctypes.byref(n_new), None) == -1
