"""The attention half of one decoder layer of the decode step in float64 (what csrc/chain.hip xcd_layer_kernel computes in one
launch), stage by stage, for tests/test_gpu_layer_kernel.py and tests/test_layer_ref_host.py.

It follows the kernel's OPERANDS, not its summation order: every sum is a float64 sum of the values the kernel multiplies --
bf16 weights, bf16 cache rows, this step's q / k / v as the f32 slab-order sum (the one f32 step), bf16(o) and bf16(x) where the
kernel rounds.  All functions work on rows: a tensor's first dimension is whatever subset of clips the caller passes.

    qkv   f32 slab-order sum of the projection's split-K slabs
    o1    self attention over `step` cached bf16 keys + this step's f32 k / v, rounded to bf16
    x1    x0 + o1 . Wso^T
    y1    bf16(x1); mean / variance of x1 (the kernel merges 32 partial {sum, centred squares} of 36 columns)
    qc    rstd * (y1 . Wcq'^T - mean * colsum)        (Wcq' = gamma o Wq in bf16, colsum its f32 row sums)
    o2    cross attention of qc over n_keys masked bf16 keys (masked score = -FLT_MAX: an all-masked row is the mean of V), bf16
    x2    x1 + o2 . Wco^T
    y2    bf16(x2); partial statistics of x2 per (row, CU column slice)

A stage can start from the kernel's own observable output of the stage before it (qc, the final o): every function takes its
input as an argument.  The wrong answers the tolerance self-checks need are the same functions with one defect switched on."""
import torch

H, D, C = 12, 64, 1152
INNER = H * D
SCALE = 0.125
CUS = 32                    # column slices (CUs of an XCD) of a projection
NEG = -torch.finfo(torch.float32).max
X_TOL = 2e-4                # residual stream, absolute (test_chain_deferred_layernorm_matches_torch)
MEAN_TOL = 2e-5             # row mean recombined from the partial statistics, absolute
VAR_RTOL = 1e-5             # row variance recombined from the partial statistics, relative
QC_TOL = 2e-3               # deferred-LayerNorm projection against float64 on the kernel's own operands
TIE = 1e-5                  # f32 accumulation term of the attention tolerance: a value this close to a bf16 rounding midpoint
SLICE = 5                   # the CU whose column slice the "shifted slice" wrong answers move


def masks(B, n, ld, g):
    """tests/test_gpu_decode_step.py masks(): clip 0 random, 1 only key 0 kept, 2 only the last key kept, 3 every key masked,
    4.. random with a ragged tail"""
    m = (torch.rand(B, ld, generator=g) > 0.4).to(torch.uint8)
    m[1:4] = 0
    m[1, 0] = 1
    m[2, n - 1] = 1
    for b in range(4, B):
        m[b, n - b:] = 0
        m[b, 0] = 1
    m[:, n:] = 7
    return m


def make_inputs(B, T, Tp, n_keys, seed, device="cpu", pad=3):
    """Unit-scale inputs of one layer for B clips (+ pad sentinel rows in every per-clip buffer).  The large tensors are drawn on
    `device`.  sk / sv hold T valid rows per (clip, head): a test NaNs the rows at and past its step (live_cache)."""
    g = torch.Generator().manual_seed(seed)
    gd = torch.Generator(device=device).manual_seed(seed)
    R = B + pad
    rn = lambda *s: torch.randn(*s, generator=gd, device=device)
    bf = torch.bfloat16
    gamma = (torch.rand(C, generator=g) * 0.4 + 0.8).to(device)
    wq = rn(INNER, C) / C ** 0.5
    inp = dict(B=B, T=T, Tp=Tp, n_keys=n_keys, R=R, gamma=gamma, wq=wq,
               w_so=(rn(C, INNER) / INNER ** 0.5).to(bf), w_cq=(wq * gamma).to(bf), w_co=(rn(C, INNER) / INNER ** 0.5).to(bf))
    inp["colsum"] = inp["w_cq"].float().sum(1).contiguous()
    x0 = torch.full((R, C), 12345.0, device=device)
    x0[:B] = rn(B, C) * 1.5 + 0.7
    inp["x0"] = x0
    qkv = torch.full((4, R, 3 * INNER), float("nan"), device=device)
    qkv[:, :B] = rn(4, B, 3 * INNER)
    inp["qkv4"] = qkv       # slabs(inp, nslab) scales the first nslab of them
    nan = float("nan")
    for name, rows, live in (("sk", T, T), ("sv", T, T), ("ck", Tp, n_keys), ("cv", Tp, n_keys)):
        c = torch.full((R, H, rows, D), nan, dtype=bf, device=device)
        c[:B, :, :live] = rn(B, H, live, D).to(bf)
        inp[name] = c
    m = torch.zeros(R, n_keys, dtype=torch.uint8)
    m[:B] = masks(B, n_keys, n_keys, g)
    inp["mask"] = m.to(device)
    return inp


def slabs(inp, nslab):
    """[nslab, R, 2304] f32 split-K slabs whose sum is unit scale"""
    return (inp["qkv4"][:nslab] / nslab ** 0.5).contiguous()


def live_cache(c, n):
    """a copy of a self cache with the rows at and past n NaN"""
    c = c.clone()
    c[:, :, n:] = float("nan")
    return c


def slab_sum(qkv):
    """slab order, float32: what the kernel sums"""
    s = qkv[0].clone()
    for i in range(1, qkv.shape[0]):
        s += qkv[i]
    return s


def bf16r(t):
    """float64 -> the nearest bf16, as float64"""
    return t.to(torch.bfloat16).double()


def attn(q, k, v, mask=None):
    """q [R, H, 64], k / v [R, H, n, 64], mask [R, n] (0 = masked) -> [R, H * 64], all float64"""
    s = torch.einsum("bhd,bhjd->bhj", q, k) * SCALE
    if mask is not None:
        s = s.masked_fill(mask[:, None, :] == 0, NEG)
    return torch.einsum("bhj,bhjd->bhd", s.softmax(-1), v).reshape(q.shape[0], -1)


def self_attn(qkv_sum, sk, sv, step, defect=None):
    """qkv_sum [R, 2304] f32; sk / sv [R, H, T, 64] bf16 with at least `step` valid rows (step + 1 for defect "shift").
    defect: None | "drop" (the first cached key missing) | "shift" (cached keys 1 .. step instead of 0 .. step - 1)"""
    R = qkv_sum.shape[0]
    q, kn, vn = (qkv_sum[:, i * INNER:(i + 1) * INNER].double().view(R, H, 1, D) for i in range(3))
    lo, hi = {None: (0, step), "drop": (1, step), "shift": (1, step + 1)}[defect]
    k = torch.cat([sk[:, :, lo:hi].double(), kn], 2)
    v = torch.cat([sv[:, :, lo:hi].double(), vn], 2)
    return attn(q.view(R, H, D), k, v)


def cross_attn(qc, ck, cv, n_keys, mask, defect=None):
    """qc [R, 768]; defect: None | "drop" (the last key missing) | "nomask\""""
    R = qc.shape[0]
    n = n_keys - 1 if defect == "drop" else n_keys
    m = None if (mask is None or defect == "nomask") else mask[:, :n]
    return attn(qc.double().view(R, H, D), ck[:, :, :n].double(), cv[:, :, :n].double(), m)


def project(a, w, defect=None):
    """a [R, K] . w [N, K]^T in float64.  defect: None | "ktile" (k columns 64 .. 127 missing) | "slice" (the columns of CU SLICE
    computed one column to the right)"""
    a, w = a.double(), w.double()
    if defect == "ktile":
        a = a.clone()
        a[:, 64:128] = 0
    out = a @ w.t()
    if defect == "slice":
        n = w.shape[0] // CUS
        out[:, SLICE * n:(SLICE + 1) * n] = a @ w[SLICE * n + 1:(SLICE + 1) * n + 1].t()
    return out


def partial_stats(x, defect=None):
    """x [R, C] -> [R, 32, 2]: {sum, centred sum of squares} of each CU's 36-column slice.  defect: None | "nocentre" (plain sum
    of squares) | "slice" (CU SLICE sums the columns one to the right)"""
    R = x.shape[0]
    n = C // CUS
    xs = x.double().view(R, CUS, n).clone()
    if defect == "slice":
        xs[:, SLICE] = x.double()[:, SLICE * n + 1:(SLICE + 1) * n + 1]
    s1 = xs.sum(2)
    d = xs if defect == "nocentre" else xs - s1[:, :, None] / n
    return torch.stack([s1, (d * d).sum(2)], 2)


def merge_stats(st, defect=None):
    """[R, 32, 2] -> (mean [R], variance [R]) by the parallel-variance formula.  defect "nocentre": the between-slice term missing"""
    st = st.double()
    n = C // CUS
    mean = st[..., 0].sum(1) / C
    between = 0 if defect == "nocentre" else n * (st[..., 0] / n - mean[:, None]) ** 2
    return mean, (st[..., 1] + between).sum(1) / C


def deferred_q(y, mean, var, w_cq, colsum, defect=None):
    """rstd * (y . Wcq'^T - mean * colsum): LayerNorm(x) * gamma . Wq^T when y = x and Wcq' = gamma o Wq"""
    return (project(y, w_cq, defect) - mean[:, None] * colsum.double()) / torch.sqrt(var + 1e-5)[:, None]


def admissible_bf16(o1_exact, resid, w_so):
    """A bf16 operand of a projection that is not observable, only resid = bf16(exact) . w^T [R, N] is (w [N, K]): the first
    self-attention output o1 behind x1 = x0 + bf16(o1) . Wso^T, and y1 = bf16(x1) behind the cross-q projection.  Where the float64
    value lies within TIE (the attention tolerance's f32 accumulation term; also above the f32 noise of the reconstructed x1) of a
    bf16 rounding midpoint, both neighbours are within tolerance, and one bf16 ulp of the operand moves the projection by more
    than its bound.  So: the nearest bf16 everywhere, and for the elements that close to a midpoint the neighbour that the
    observed resid asks for (its projection on the element's weight column).  Returns (operand [R, K] float64 holding bf16
    values, number of elements moved)."""
    near_b = o1_exact.to(torch.bfloat16)
    near = near_b.double()
    bits = near_b.view(torch.int16).to(torch.int32)             # sign-magnitude: + 1 is the neighbour away from zero
    step = torch.where(o1_exact.abs() > near.abs(), 1, -1)      # the neighbour on the other side of o1_exact
    other = (bits + step).to(torch.int16).view(torch.bfloat16).double()
    # (steps below 4 TIE are left alone: either neighbour moves x1 by less than 1e-5, and the residual's f32 noise could not tell them apart)
    tie = (((near + other) / 2 - o1_exact).abs() < TIE) & ((other - near).abs() > 4 * TIE)
    w = w_so.double()
    norm = (w * w).sum(0)
    cur = near.clone()
    for _ in range(3):      # a large moved element leaks ~3 % of its step into the other columns' amplitudes: decide, subtract, repeat
        coef = ((resid.double() - cur @ w.t()) @ w) / norm      # least-squares amplitude of each weight column in the residual
        want = torch.where(cur == near, other, near)
        delta = torch.where(tie, want - cur, torch.ones_like(cur))
        cur = torch.where(tie & (coef / delta > 0.5), want, cur)
    return cur, int((cur != near).sum())


def reference(inp, qkv, step, rows=None, obs=None):
    """Every stage for the clips `rows` (index tensor; default all B).  obs: the kernel's observable outputs {"x", "qc", "o"} (full
    buffers); with it stage k starts from the kernel's stage k - 1: x1 = x - o . Wco^T, the cross attention from the kernel's
    qc, x2 from the kernel's o.  Returns the stages and "alts": stage -> [(name, wrong answer)]."""
    dev = inp["x0"].device
    rows = torch.arange(inp["B"], device=dev) if rows is None else rows.to(dev)
    sel = lambda t: t[rows]
    x0 = sel(inp["x0"]).double()
    sk, sv, ck, cv, mask = (sel(inp[k]) for k in ("sk", "sv", "ck", "cv", "mask"))
    w_so, w_cq, w_co, colsum, n_keys = inp["w_so"], inp["w_cq"], inp["w_co"], inp["colsum"], inp["n_keys"]
    r = {"qkv": slab_sum(qkv)[rows]}
    r["o1_exact"] = self_attn(r["qkv"], sk, sv, step)
    alts = {"x": [], "qc": [], "o": [], "stats": []}
    if obs is None:
        r["o1"], r["moved"] = bf16r(r["o1_exact"]), 0
        r["x1"] = x0 + project(r["o1"], w_so)
    else:
        o_obs, x_obs = sel(obs["o"]).double(), sel(obs["x"]).double()
        r["x1"] = x_obs - project(o_obs, w_co)              # reconstructed: the kernel's own x1 up to f32 rounding
        r["o1"], r["moved"] = admissible_bf16(r["o1_exact"], r["x1"] - x0, w_so)
    r["mean1"], r["var1"] = merge_stats(partial_stats(r["x1"]))
    if obs is None:
        r["y1"] = bf16r(r["x1"])
    else:       # y1 . Wcq'^T as the kernel's qc implies it; x1 is reconstructed, so its rounding to bf16 can tie as o1's can
        y_proj = sel(obs["qc"]).double() * torch.sqrt(r["var1"] + 1e-5)[:, None] + r["mean1"][:, None] * colsum.double()
        r["y1"], moved_y = admissible_bf16(r["x1"], y_proj, w_cq)
        r["moved"] += moved_y
    r["qc"] = deferred_q(r["y1"], r["mean1"], r["var1"], w_cq, colsum)
    qc_in = r["qc"] if obs is None else sel(obs["qc"]).double()
    r["o2_exact"] = cross_attn(qc_in, ck, cv, n_keys, mask)
    r["o2"] = bf16r(r["o2_exact"])
    o2_in = r["o2"] if obs is None else o_obs
    r["x2"] = x0 + project(r["o1"], w_so) + project(o2_in, w_co)
    x2_in = r["x2"] if obs is None else x_obs
    r["y2"] = bf16r(x2_in)
    r["stats"] = partial_stats(x2_in)
    r["mean2"], r["var2"] = merge_stats(r["stats"])

    # ---- the wrong answers
    if step > 0:
        for name, defect in (("one self key dropped", "drop"), ("self keys shifted by one", "shift")):
            if defect == "shift" and step + 1 > sk.shape[2]:
                continue
            o1w = bf16r(self_attn(r["qkv"], sel(inp["sk"]), sel(inp["sv"]), step, defect))
            alts["x"].append((name, x0 + project(o1w, w_so) + project(o2_in, w_co)))
    for name, d1, d2 in (("a k-tile missing from the self out-projection", "ktile", None),
                         ("a k-tile missing from the cross out-projection", None, "ktile"),
                         ("a CU's slice of the self out-projection shifted by one column", "slice", None),
                         ("a CU's slice of the cross out-projection shifted by one column", None, "slice")):
        alts["x"].append((name, x0 + project(r["o1"], w_so, d1) + project(o2_in, w_co, d2)))
    alts["qc"].append(("a k-tile missing from the cross-q projection", deferred_q(r["y1"], r["mean1"], r["var1"], w_cq, colsum, "ktile")))
    alts["qc"].append(("a CU's slice of the cross-q projection shifted by one column",
                       deferred_q(r["y1"], r["mean1"], r["var1"], w_cq, colsum, "slice")))
    m_nc, v_nc = merge_stats(partial_stats(r["x1"]), "nocentre")
    alts["qc"].append(("statistics merged without the centring term", deferred_q(r["y1"], m_nc, v_nc, w_cq, colsum)))
    alts["o"].append(("one cross key dropped", cross_attn(qc_in, ck, cv, n_keys, mask, "drop")))
    alts["o"].append(("the mask ignored", cross_attn(qc_in, ck, cv, n_keys, mask, "nomask")))
    alts["stats"].append(("partial statistics without the centring term", merge_stats(partial_stats(x2_in, "nocentre"))))
    alts["stats"].append(("a CU's statistics slice shifted by one column", merge_stats(partial_stats(x2_in, "slice"))))
    r["alts"] = alts
    return r


def attn_tolerance(ref):
    """tests/test_gpu_decode_step.py tolerance() for bf16: one ulp of the bf16 output plus the f32 accumulation"""
    return torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -100))) - 7) + TIE


def stats_separated(mean, var, alt):
    """whether a wrong (mean, variance) lies outside MEAN_TOL / VAR_RTOL of the right one somewhere"""
    return bool(((alt[0] - mean).abs() > MEAN_TOL).any() or (((alt[1] - var) / var).abs() > VAR_RTOL).any())
