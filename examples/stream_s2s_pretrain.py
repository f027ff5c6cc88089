"""Streaming DIM-Listener: feed a dyad clip to the model in chunks of speaker frames, as a live system would, and receive the
listener tokens (and their decoded motion) as they fall due (SLMFT.stream; the schedule is dimx/stream.py).

    python examples/stream_s2s_pretrain.py --synthetic --chunk 8 --lookahead 0 [--frames 120] [--batch 2] [--window 32] [--bf16]
    python examples/stream_s2s_pretrain.py --synthetic --chunk 8 --lookahead 0 --frames 600 --segment 200 --carry 50

Prints, per push, the frames in, the tokens out and the device-event time of the push; at the end, whether the session's tokens
equal ``forward(mode="val", lookahead=L)`` on the whole clip.  Without ``--synthetic`` a checkpoint is loaded from ``--ckpt``; the
clip itself is synthetic either way (a live source is the caller's).

``--segment N --carry K``: a conversation that outlasts a session.  The clip is fed through consecutive sessions of at most N
frames; each but the first is begun from the last K frames of the one before and the K - max(L, 0) codes it produced for them
(``SLMFT.stream(prompt=...)``, dimx_stream_begin_prompted) -- the carried frames sit at positions 0 .. K - 1 of a new
clip.  The time of every begin is printed next to the pushes.  Nothing was trained on restarted clips: this shows the mechanism
and its cost, not a quality.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dimx  # noqa: E402,F401
from dimx import lib as L  # noqa: E402
from dimx import prng, stream  # noqa: E402
from dimx.seq2seq_pretrain import SLMFT  # noqa: E402


def segments(model, args, v_s, v_a, z_l):
    """the clip through consecutive sessions of --segment frames, each begun from the last --carry frames and their codes"""
    B, T, Lh, N, K = args.batch, args.frames, args.lookahead, args.segment, args.carry
    P = K - max(Lh, 0)
    if not (2 <= N <= 2048 and K < N and stream.prompt_fits(P, Lh, K, N)):
        sys.exit("--segment %d --carry %d: need 2 <= segment <= 2048 and 1 <= carry - max(lookahead, 0), carry < segment" % (N, K))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return out, e0.elapsed_time(e1)

    s, t_begin = timed(lambda: model.stream(B, N, z_l[:, 0], lookahead=Lh, greedy=True, kv8=args.kv8, self_kv8=args.self_kv8))
    print("session 0: begin %.3f ms" % t_begin)
    codes = z_l[:, :1].to(torch.int32)      # all listener codes so far: position 0 is given, the rest are the sessions' tokens
    fed, k, t_push, t_begins = 0, 0, 0.0, []
    while fed < T:
        if s.frames == N:                     # the session is full: carry the last K frames and their P codes into a new one
            s.close()
            k += 1
            prompt = codes[:, fed - K:fed - K + P].contiguous()
            _, t_begin = timed(lambda: s.begin(prompt=prompt, v_speaker=v_s[:, fed - K:fed], v_audio=v_a[:, fed - K:fed]))
            t_begins.append(t_begin)
            print("session %d: begun from frames %d .. %d and %d codes in %.3f ms" % (k, fed - K, fed - 1, P, t_begin))
        c = min(args.chunk, T - fed, N - s.frames)
        new, ms = timed(lambda: s.push(v_s[:, fed:fed + c], v_a[:, fed:fed + c]))
        fed += c
        t_push += ms
        codes = torch.cat([codes, new], 1)
        print("frames %4d -> %4d   tokens out %3d (codes %4d)   push %.3f ms" % (fed - c, fed, new.shape[1], codes.shape[1], ms))
    codes = torch.cat([codes, s.end()], 1)
    s.close()
    print("end: %d codes for %d frames; pushes %.1f ms = %.3f ms per frame; %d restarts, %s ms each"
          % (codes.shape[1], T, t_push, t_push / T, len(t_begins), ", ".join("%.3f" % t for t in t_begins) or "-"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--synthetic", action="store_true", help="synthetic weights (no checkpoint)")
    ap.add_argument("--ckpt", default="best_vico_causal.pt")
    ap.add_argument("--chunk", type=int, default=8, help="speaker frames per push")
    ap.add_argument("--lookahead", type=int, default=0, help="L of dimx.online: < 0 a reaction delay, > 0 a look-ahead buffer")
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--window", type=int, default=32, help="tokens the chunked VQ decode sees (0: all so far)")
    ap.add_argument("--bf16", action="store_true")
    ap.add_argument("--segment", type=int, default=0, help="frames per session (0: one session for the whole clip)")
    ap.add_argument("--carry", type=int, default=0, help="with --segment: frames (and their codes) carried into the next session")
    ap.add_argument("--kv8", action="store_true", help="FP8 cross K/V in the session (dimx_stream_set_kv8; DESIGN 31)")
    ap.add_argument("--self-kv8", action="store_true", help="FP8 self K/V in the session")
    args = ap.parse_args()
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    model = SLMFT(numeric_mode=L.MODE_PERF_BF16 if args.bf16 else L.MODE_PARITY_F32).eval()
    if not args.synthetic:
        if not os.path.isfile(args.ckpt):
            sys.exit("no checkpoint at %s (pass --synthetic for synthetic weights)" % args.ckpt)
        model.load_state_dict(torch.load(args.ckpt, map_location="cpu")["state_dict"])
    B, T, Lh = args.batch, args.frames, args.lookahead
    v_s = torch.from_numpy(prng.normal(5, "stream.vs", (B, T, 56))).to(dev)
    v_l = torch.from_numpy(prng.normal(5, "stream.vl", (B, T, 56))).to(dev)
    v_a = torch.from_numpy(prng.normal(5, "stream.va", (B, T, 768))).to(dev)
    mask = torch.ones(B, T, dtype=torch.bool, device=dev)
    # the whole-clip call starts from the ground-truth first listener code; the session is given the same one
    _, z_l = model.forward_vq(v_s, v_l, mask, with_speaker=False)
    window = args.window or None
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    total = 0.0
    if args.segment:
        return segments(model, args, v_s, v_a, z_l)
    with model.stream(B, T, z_l[:, 0], lookahead=Lh, greedy=True, kv8=args.kv8, self_kv8=args.self_kv8) as s:
        for c in stream.chunks(T, args.chunk):
            n = s.frames
            e0.record()
            new = s.push(v_s[:, n:n + c], v_a[:, n:n + c])
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1)
            total += ms
            motion = s.motion(window)
            print("frames %4d -> %4d   tokens out %3d (steps %4d)   motion rows %3d   push %.3f ms" % (n, s.frames, new.shape[1], s.steps, motion.shape[1], ms))
        tail = s.end()
        print("end: %d more tokens, %d in all; pushes took %.1f ms = %.3f ms per frame" % (tail.shape[1], s.steps, total, total / T))
        tokens = s.tokens.long()
    if args.kv8 or args.self_kv8:
        # the incremental and the batch encoder agree to about 1e-6, not to the bit, so a code may land on the other side of a rounding
        # boundary: the comparison with the whole-clip FP8 call is a count, not an equality
        _, _, _, ref = model(v_s, v_l, v_a, mask, mode="val", greedy=True, lookahead=Lh, return_tokens=True, kv8=args.kv8, self_kv8=args.self_kv8)
        print("session tokens that differ from forward(mode='val', lookahead=%d, kv8=%s, self_kv8=%s) on the whole clip: %d of %d"
              % (Lh, args.kv8, args.self_kv8, int((tokens != ref).sum()), tokens.numel()))
        return
    _, _, _, ref = model(v_s, v_l, v_a, mask, mode="val", greedy=True, lookahead=Lh, return_tokens=True)
    same = bool(torch.equal(tokens, ref))
    print("session tokens equal forward(mode='val', lookahead=%d) on the whole clip: %s" % (Lh, same))
    if not same:
        first = (tokens != ref).long().argmax(1).tolist()
        print("first differing step per clip: %s (a near-tie of two logits may fall either way between two launch shapes)" % first)


if __name__ == "__main__":
    main()
