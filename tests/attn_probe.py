"""The prefill attention (csrc/attention_tr.hip, csrc/attention.hip) in float64, two probes whose outputs say exactly WHICH keys a
query saw, and the same reference with one visibility defect switched on.  For tests/test_gpu_attention_probes.py (the kernels)
and tests/test_attn_probe_host.py (that the probes would notice every defect listed here, on the CPU).

Visibility.  keep(): key j is visible to query i of clip b iff j < min(len_b, Lk), kmask[b, j] != 0 and, if causal, j <= i.

Reference.  reference(): softmax over the visible keys of q . k * scale on operands rounded to the kernel's input type, float64
sums.  A row without a visible key: x-transformers fills masked scores with -finfo.max, so all Lk scores are equal and the row is
the plain mean of V over all Lk keys (full_row_value()).  The kernels agree in the non-causal case when the clip's length does not
cut keys off (len_b >= Lk: the only form a caller produces); rows of a clip with len_b == 0 are zero.

Count probe.  q = 0, V[b, j, h, d] = 1 iff (j + h + 3 b) % D == d.  Every visible score is exactly 0, so row i is c_d / n with n
the number of visible keys and c_d the number of them in residue class d: integers, exact products, one rounding (the output's).
Accepted: columns with c_d == 0 exactly 0, the others within a relative 2^-7 (bf16: the output's rounding is at most 2^-8) or 1e-6 (f32).
One wrong key changes its class's column by (n - c) / (c (n +- 1)) relative: 0.16 at the largest shape here (n = 257, c = 6),
1 or more where the class had at most one key, and a column that was or becomes empty fails the exact-zero rule outright.

Locator probe.  k[j] = a +-1 code (the same table for every clip and head, times a per-head sign pattern so the heads' data differ
and their products do not), q[i] = 32 * k[t(i)], V[j] = the bits of j in columns h .. h + nb - 1 (mod D) and a one in column
h + nb.  All exact in bf16.  The softmax is one-hot at the best-scoring visible key, so the output row spells a key index.
    target "last":   t(i) = the last visible key of row i.  The row must spell t(i), bits within 2^-7 of 0 or 1.
    target "hidden": t(i) = an invisible key, where the row has a usable one: the candidate nearest to last + 1 whose best-scoring
                     visible key is unique and holds at least 3/4 of the reference's weight (with c = 32 a lead of one code step,
                     2 in the product, is 3.3 nats at D = 48: the runner-up keeps 4 % and the bits are NOT within 2^-7 of 0 / 1).
                     The row must spell the reference's best visible key, bits within 2^-7 of the REFERENCE's value.
                     Rows without a usable candidate keep the "last" target.
Columns outside the bits and the one are exactly 0.

Mutants.  mutants() yields keep() with one defect of the kind the kernels could have: key mask rolled by one, causal bound +-1,
len +-1, the key word of tile t swapped with tile t + 1, the two 4-key nibbles of every 8 keys swapped (the `half` packing), one
nibble pair swapped, a fully masked leading tile treated as visible."""
import math

import torch

C_LOC = 32.0
BF16_RTOL = 2.0 ** -7
F32_RTOL = 1e-6
BIT_TOL = 2.0 ** -7
LEAK_MAX = 2.0 ** -12         # target "last": weight not on the target, bound checked by the host test
HIDDEN_MIN_TOP = 0.75         # target "hidden": least weight of the best visible key

HEADS = {48: (8, 384 ** -0.5), 64: (12, 0.125), 96: (8, 768 ** -0.5)}    # D -> (H, scale): the model's three head shapes


def rnd(x, dtype):
    return x.to(dtype).double()


# ------------------------------------------------------------------ visibility

def key_bits(Lk, lens, kmask, B):
    """[B, Lk] bool: key j of clip b is a key at all (below its length, kept by its mask) -- one bit of the kernels' key words"""
    kb = torch.ones(B, Lk, dtype=torch.bool)
    if lens is not None:
        kb &= torch.arange(Lk)[None, :] < torch.as_tensor(lens).clamp(max=Lk)[:, None]
    if kmask is not None:
        kb &= torch.as_tensor(kmask).bool()
    return kb


def apply_rows(kb, Lq, causal, shift=0):
    """[B, Lq, Lk] from key bits: causal keeps j <= i + shift"""
    B, Lk = kb.shape
    kp = kb[:, None, :].expand(B, Lq, Lk).clone()
    if causal:
        kp &= (torch.arange(Lk)[None, :] <= torch.arange(Lq)[:, None] + shift)[None]
    return kp


def batch_of(lens, kmask, B=None):
    if lens is not None:
        return len(lens)
    if kmask is not None:
        return len(kmask)
    return 1 if B is None else B


def keep(Lq, Lk, causal, lens, kmask, B=None):
    """[B, Lq, Lk] bool, the definition of visibility"""
    return apply_rows(key_bits(Lk, lens, kmask, batch_of(lens, kmask, B)), Lq, causal)


def mutants(Lq, Lk, causal, lens, kmask, B=None):
    """(name, keep with one defect, the clip lengths the defective kernel works with) for every defect that applies to the case"""
    B = batch_of(lens, kmask, B)
    kb = key_bits(Lk, lens, kmask, B)
    lens_t = torch.full((B,), Lk, dtype=torch.long) if lens is None else torch.as_tensor(lens).long()
    out = []
    if kmask is not None:
        out.append(("mask rolled by one", apply_rows(key_bits(Lk, lens, torch.roll(torch.as_tensor(kmask), 1, 1), B), Lq, causal)))
    if causal:
        out.append(("causal bound + 1", apply_rows(kb, Lq, True, 1)))
        out.append(("causal bound - 1", apply_rows(kb, Lq, True, -1)))
    for name, lm in (("len + 1", (lens_t + 1).tolist()), ("len - 1", (lens_t - 1).clamp(min=0).tolist())):
        out.append((name, apply_rows(key_bits(Lk, lm, kmask, B), Lq, causal), lm))
    nt = (Lk + 63) // 64
    pad = torch.zeros(B, nt * 64, dtype=torch.bool)
    pad[:, :Lk] = kb
    words = pad.view(B, nt, 64)
    for t in range(nt - 1):
        w = words.clone()
        w[:, t], w[:, t + 1] = words[:, t + 1], words[:, t]
        out.append(("key words of tiles %d and %d swapped" % (t, t + 1), apply_rows(w.reshape(B, -1)[:, :Lk].contiguous(), Lq, causal)))
    j = torch.arange(nt * 64)
    out.append(("nibbles swapped (half)", apply_rows(pad[:, j ^ 4][:, :Lk].contiguous(), Lq, causal)))
    for t in range(nt):
        for m in range(8):
            a = 64 * t + 8 * m
            if not torch.equal(pad[:, a:a + 4], pad[:, a + 4:a + 8]):
                w = pad.clone()
                w[:, a:a + 4], w[:, a + 4:a + 8] = pad[:, a + 4:a + 8], pad[:, a:a + 4]
                out.append(("nibbles at key %d swapped" % a, apply_rows(w[:, :Lk].contiguous(), Lq, causal)))
                break
    lead = ~words[:, 0].any(1) & (lens_t > 0)
    if lead.any():
        w = pad.clone()
        w[lead, :64] = True
        out.append(("masked leading tile visible", apply_rows(w[:, :Lk].contiguous(), Lq, causal)))
    return [m if len(m) == 3 else m + (lens,) for m in out]


# ------------------------------------------------------------------ reference

def full_row_value(v):
    """a row without a visible key: equal -finfo.max scores, the mean of V over all Lk keys.  v [B, Lk, H, D] -> [B, H, D]"""
    return v.double().mean(1)


def reference(q, k, v, scale, kp, dtype=torch.bfloat16, lens=None, return_probs=False):
    """[B, Lq, H, D] float64.  kp [B, Lq, Lk] from keep() (or a mutant).  Rows of a clip with len == 0 are zero."""
    qd, kd, vd = rnd(q, dtype), rnd(k, dtype), rnd(v, dtype)
    s = torch.einsum("bihd,bjhd->bhij", qd, kd) * scale
    kp = kp.expand(q.shape[0], -1, -1)
    s = s.masked_fill(~kp[:, None], float("-inf"))
    s = s.masked_fill(~kp.any(-1)[:, None, :, None], 0.0)
    p = torch.softmax(s, -1)
    o = torch.einsum("bhij,bjhd->bihd", p, vd)
    if lens is not None:
        o[torch.as_tensor(lens) == 0] = 0.0
    return (o, p) if return_probs else o


def row_classes(kp, lens):
    """valid [B, Lq]: the row has a visible key; empty [B]: the clip has len == 0 (its rows are zero)"""
    B = kp.shape[0]
    empty = torch.zeros(B, dtype=torch.bool) if lens is None else torch.as_tensor(lens) == 0
    return kp.any(-1), empty


# ------------------------------------------------------------------ count probe

def count_inputs(B, Lq, Lk, H, D, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.zeros(B, Lq, H, D)
    k = torch.randn(B, Lk, H, D, generator=g)
    cls = (torch.arange(Lk)[None, :, None] + torch.arange(H)[None, None, :] + 3 * torch.arange(B)[:, None, None]) % D
    v = torch.nn.functional.one_hot(cls, D).float()
    return q, k, v


def count_expected(kp, v):
    """c [B, Lq, H, D] and n [B, Lq]: integer counts, as float64"""
    c = torch.einsum("bij,bjhd->bihd", kp.double(), v.double())
    return c, kp.sum(-1).double()


def count_failures(out, kp, v, lens, dtype, full_rows_exact=False):
    """list of strings, empty when `out` [B, Lq, H, D] passes.  Rows without a visible key (len > 0) must be finite, or, with
    full_rows_exact, the mean of V over all Lk keys to the same rule."""
    out = out.double()
    valid, empty = row_classes(kp, lens)
    c, n = count_expected(kp, v)
    if full_rows_exact:
        full = ~valid & ~empty[:, None]
        c = torch.where(full[:, :, None, None], v.double().sum(1)[:, None].expand_as(c), c)
        n = torch.where(full, torch.full_like(n, float(v.shape[1])), n)
        valid = valid | full
    fails = []
    if not torch.isfinite(out).all():
        fails.append("not finite")
    if (out[empty] != 0).any():
        fails.append("a row of an empty clip is not zero")
    rows = valid & ~empty[:, None]
    want = (c / n.clamp(min=1)[:, :, None, None])[rows]
    got = out[rows]
    if ((want == 0) & (got != 0)).any():
        fails.append("a column without a visible key is not exactly zero")
    rel = ((got - want).abs() / want.clamp(min=1e-30))[want > 0]
    rtol = BF16_RTOL if dtype == torch.bfloat16 else F32_RTOL
    if rel.numel() and rel.max().item() > rtol:
        fails.append("count off by %.3g relative (allowed %.3g)" % (rel.max().item(), rtol))
    return fails


# ------------------------------------------------------------------ locator probe

def codes(Lk, H, D, seed):
    """base [Lk, D] and per-head sign patterns [H, D], all +-1"""
    g = torch.Generator().manual_seed(seed)
    base = (torch.randint(0, 2, (Lk, D), generator=g) * 2 - 1).double()
    sign = (torch.randint(0, 2, (H, D), generator=g) * 2 - 1).double()
    return base, sign


def code_gap(base):
    """the smallest lead of a key's product with itself over any other key's product with it"""
    if base.shape[0] < 2:
        return float(base.shape[1])
    gram = base @ base.t()
    gram.fill_diagonal_(-1e9)
    return base.shape[1] - gram.max().item()


def leak_bound(Lk, gap, scale):
    return Lk * 2.0 ** -(C_LOC * gap * scale * math.log2(math.e))


def n_bits(Lk):
    return max(1, (Lk - 1).bit_length())


def hidden_targets(kp, base, scale):
    """[B, Lq] target keys of the "hidden" choice and a mask of the rows that got one (the others keep their last visible key)"""
    B, Lq, Lk = kp.shape
    gram = (base @ base.t()).float() * float(C_LOC * scale)                  # score of key j for target t: gram[t, j]
    last = (kp.long() * torch.arange(Lk)).amax(-1)
    target, hidden = last.clone(), torch.zeros(B, Lq, dtype=torch.bool)
    for b in range(B):
        rows, inv = torch.unique(kp[b], dim=0, return_inverse=True)
        for u in range(rows.shape[0]):
            vis = rows[u]
            if not vis.any() or vis.all():
                continue
            s = gram[:, vis]                                                 # [candidate t, visible j]
            top2 = s.topk(min(2, s.shape[1]), dim=1).values
            w_top = 1.0 / torch.exp(s - top2[:, :1]).sum(1)
            ok = ~vis & (w_top >= HIDDEN_MIN_TOP)
            if top2.shape[1] == 2:
                ok &= top2[:, 0] > top2[:, 1]
            if not ok.any():
                continue
            cand = torch.nonzero(ok)[:, 0]
            for i in torch.nonzero(inv == u)[:, 0].tolist():
                target[b, i] = cand[(cand - (last[b, i] + 1)).abs().argmin()]
                hidden[b, i] = True
    return target, hidden


def locator_inputs(kp, H, D, scale, seed, choice):
    """q, k, v [B, L, H, D] and the target [B, Lq]; choice "last" or "hidden" """
    B, Lq, Lk = kp.shape
    base, sign = codes(Lk, H, D, seed)
    last = (kp.long() * torch.arange(Lk)).amax(-1)
    if choice == "last":
        target, hidden = last, torch.zeros(B, Lq, dtype=torch.bool)
    else:
        target, hidden = hidden_targets(kp, base, scale)
    kh = base[:, None, :] * sign[None]                                       # [Lk, H, D]
    k = kh[None].expand(B, Lk, H, D).float().contiguous()
    q = (C_LOC * kh[target]).float()                                          # [B, Lq, H, D]
    nb = n_bits(Lk)
    v = torch.zeros(B, Lk, H, D)
    j = torch.arange(Lk)
    for h in range(H):
        for bit in range(nb):
            v[:, :, h, (h + bit) % D] = ((j >> bit) & 1).float()
        v[:, :, h, (h + nb) % D] = 1.0
    return q, k, v, target, hidden


def decode(out, Lk):
    """[B, Lq, H] key index a locator output spells; the bit columns [B, Lq, H, nb]; the one column [B, Lq, H]; the largest
    magnitude among the other columns"""
    B, Lq, H, D = out.shape
    nb = n_bits(Lk)
    cols = (torch.arange(H)[:, None] + torch.arange(nb + 1)[None, :]) % D                  # [H, nb + 1]
    picked = torch.gather(out.double(), 3, cols[None, None].expand(B, Lq, H, nb + 1))
    bits = picked[..., :nb]
    index = ((bits > 0.5).long() << torch.arange(nb)).sum(-1)
    used = torch.zeros(H, D, dtype=torch.bool).scatter_(1, cols, True)
    rest = out.double().masked_fill(used[None, None], 0.0).abs().amax(-1)
    return index, bits, picked[..., nb], rest


def locator_failures(out, ref, kp, lens, Lk, hidden):
    """list of strings, empty when `out` passes against the float64 reference `ref` of the same inputs"""
    valid, empty = row_classes(kp, lens)
    rows = valid & ~empty[:, None]
    gi, gb, gone, grest = decode(out, Lk)
    ri, rb, _, _ = decode(ref, Lk)
    fails = []
    if not torch.isfinite(out.double()).all():
        fails.append("not finite")
    if (out.double()[empty] != 0).any():
        fails.append("a row of an empty clip is not zero")
    if (gi != ri)[rows].any():
        r = torch.nonzero((gi != ri) & rows[:, :, None])[0].tolist()
        fails.append("row %s spells key %d, the reference %d" % (r, gi[tuple(r)], ri[tuple(r)]))
    plain = rows & ~hidden
    d01 = torch.minimum(gb.abs(), (gb - 1).abs())[plain]
    if d01.numel() and d01.max().item() > BIT_TOL:
        fails.append("a bit is %.3g from 0 / 1" % d01.max().item())
    dref = (gb - rb).abs()[rows & hidden]
    if dref.numel() and dref.max().item() > BIT_TOL:
        fails.append("a bit is %.3g from the reference" % dref.max().item())
    if ((gone - 1).abs()[rows] > BIT_TOL).any():
        fails.append("the weights do not sum to one")
    if (grest[rows] != 0).any():
        fails.append("a column outside the index is not exactly zero")
    return fails


# ------------------------------------------------------------------ the shapes both test files use

def random_mask(B, Lk, seed):
    m = (torch.rand(B, Lk, generator=torch.Generator().manual_seed(seed)) < 0.7).to(torch.uint8)
    m[:, 0] = 1
    return m


def build_mask(B, Lk, spec, seed):
    """spec: None, "random", or one entry per clip of "random", "all", ("hide", a, b) = keys a .. b - 1 masked, "last" = only key
    Lk - 1 visible"""
    if spec is None:
        return None
    rm = random_mask(B, Lk, seed)
    if spec == "random":
        return rm
    m = torch.ones(B, Lk, dtype=torch.uint8)
    for b, s in enumerate(spec):
        if s == "random":
            m[b] = rm[b]
        elif s == "last":
            m[b] = 0
            m[b, Lk - 1] = 1
        elif s != "all":
            m[b, s[1]:s[2]] = 0
    return m


# name, Lq, Lk, causal, lens, mask spec, also run random data
CASES = [
    ("n1x1", 1, 1, False, (1, 0, 1), None, False),
    ("n32x63", 32, 63, False, (63, 0, 63), "random", False),
    ("n33x64", 33, 64, False, None, ("random", "last", "all"), False),
    ("n128x65", 128, 65, False, (64, 65, 63), None, False),
    ("n129x128", 129, 128, False, None, (("hide", 0, 64), ("hide", 0, 71), "random"), False),
    ("n257x129", 257, 129, False, (129, 0, 129), "random", True),
    ("n1x193", 1, 193, False, None, (("hide", 0, 64), ("hide", 0, 71), ("hide", 64, 128)), False),
    ("n129x193", 129, 193, False, (193, 64, 1), (("hide", 64, 128), "random", "random"), True),
    ("c1", 1, 1, True, (1, 0, 1), None, False),
    ("c33", 33, 33, True, None, ("random", "last", "random"), False),
    ("c64", 64, 64, True, (64, 1, 63), None, False),
    ("c65", 65, 65, True, (65, 0, 65), "random", True),
    ("c129", 129, 129, True, None, (("hide", 0, 64), ("hide", 0, 71), "random"), True),
    ("c130", 130, 130, True, (130, 1, 65), (("hide", 64, 128), "all", "random"), False),
    ("c257", 257, 257, True, (257, 63, 64), "random", True),
]
CASE_IDS = [c[0] for c in CASES]
SEED = 20


def case_masks(case):
    """(B, lens list or None, kmask uint8 [B, Lk] or None, keep [B, Lq, Lk])"""
    name, Lq, Lk, causal, lens, spec, _ = case
    B = 3
    kmask = build_mask(B, Lk, spec, SEED + Lk)
    lens = list(lens) if lens is not None else None
    return B, lens, kmask, keep(Lq, Lk, causal, lens, kmask, B)
