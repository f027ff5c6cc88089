"""Deterministic, machine-independent tensor generator.

No checkpoints or datasets of the reference are available, so every weight and
every synthetic dyad clip is *regenerated* from integers: a counter-based
splitmix64 stream keyed by ``seed`` and the FNV-1a hash of the tensor name.  The
integer part is exact on any machine; the affine map to floats is done in float64
and rounded once to float32, so uniform tensors are bit-identical everywhere
(golden fixtures under tests/golden rely on this: the 93 MB of VQ-VAE weights are
not committed, they are regenerated on both sides).
"""
import numpy as np

_GOLD = np.uint64(0x9E3779B97F4A7C15)
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)
_MASK = (1 << 64) - 1


def fnv1a64(name: str) -> int:
    h = 0xCBF29CE484222325
    for b in name.encode("utf-8"):
        h ^= b
        h = (h * 0x100000001B3) & _MASK
    return h


def _mix(z: np.ndarray) -> np.ndarray:
    z = (z ^ (z >> np.uint64(30))) * _M1
    z = (z ^ (z >> np.uint64(27))) * _M2
    return z ^ (z >> np.uint64(31))


def raw_u64(seed: int, name: str, n: int, offset: int = 0) -> np.ndarray:
    """n 64-bit words of stream (seed, name), starting at counter ``offset``."""
    key = np.uint64((int(seed) ^ fnv1a64(name)) & _MASK)
    with np.errstate(over="ignore"):
        ctr = np.arange(offset + 1, offset + n + 1, dtype=np.uint64)
        return _mix(key + ctr * _GOLD)


def uniform01(seed: int, name: str, n: int, offset: int = 0) -> np.ndarray:
    """float64 in [0,1) with 24 significant bits (exactly representable in f32)."""
    return (raw_u64(seed, name, n, offset) >> np.uint64(40)).astype(np.float64) * (1.0 / (1 << 24))


def uniform(seed: int, name: str, shape, lo: float, hi: float) -> np.ndarray:
    n = int(np.prod(shape)) if len(shape) else 1
    u = uniform01(seed, name, n)
    return (lo + (hi - lo) * u).astype(np.float32).reshape(shape)


def normal(seed: int, name: str, shape) -> np.ndarray:
    """Box-Muller N(0,1) in float64, rounded once to float32."""
    n = int(np.prod(shape)) if len(shape) else 1
    m = (n + 1) // 2
    u = uniform01(seed, name, 2 * m)
    u1 = 1.0 - u[:m]            # (0,1]
    u2 = u[m:]
    r = np.sqrt(-2.0 * np.log(u1))
    z = np.concatenate([r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)])[:n]
    return z.astype(np.float32).reshape(shape)


def exponential(seed: int, name: str, shape) -> np.ndarray:
    """Exp(1) noise for the injected-noise sampler, strictly positive."""
    n = int(np.prod(shape)) if len(shape) else 1
    u = uniform01(seed, name, n)
    e = -np.log1p(-u)           # u in [0,1) -> e in [0, inf)
    e = np.maximum(e, 2.0 ** -30)
    return e.astype(np.float32).reshape(shape)


def integers(seed: int, name: str, shape, lo: int, hi: int) -> np.ndarray:
    """ints uniform in [lo, hi)."""
    n = int(np.prod(shape)) if len(shape) else 1
    r = raw_u64(seed, name, n) >> np.uint64(11)
    return (lo + (r % np.uint64(hi - lo)).astype(np.int64)).reshape(shape)


# ---------------------------------------------------------------------------------------------------------------------
# Exp(1) noise of the sampler's on-device generator (csrc/sample_pick.hpp, sample_survivor; include/dimx.h dimx_set_shard)
# ---------------------------------------------------------------------------------------------------------------------
SAMPLER_VOCAB = 512
SAMPLER_NOISE_FLOOR = 2.0 ** -30


def sampler_counters(step: int, rows: int, rows_total=None, row_offset: int = 0) -> np.ndarray:
    """uint64 [rows, 512]: ctr = ((step * rows_total + row_offset + row) * 512 + code) mod 2^64."""
    rows = int(rows)
    total = rows if rows_total is None else int(rows_total)
    first = (int(step) * total + int(row_offset)) & _MASK           # python integers: the product wraps like the device's
    with np.errstate(over="ignore"):
        row = np.uint64(first) + np.arange(rows, dtype=np.uint64)[:, None]
        return row * np.uint64(SAMPLER_VOCAB) + np.arange(SAMPLER_VOCAB, dtype=np.uint64)[None, :]


def sampler_uniform(seed: int, step: int, rows: int, rows_total=None, row_offset: int = 0) -> np.ndarray:
    """float64 [rows, 512], exact: u = (mix(seed + (ctr + 1) * GOLD) >> 40) / 2^24, mix = splitmix64's finaliser."""
    with np.errstate(over="ignore"):
        ctr = sampler_counters(step, rows, rows_total, row_offset)
        r = _mix(np.uint64(int(seed) & _MASK) + (ctr + np.uint64(1)) * _GOLD)
    return (r >> np.uint64(40)).astype(np.float64) * (1.0 / (1 << 24))


def sampler_noise(seed: int, step: int, rows: int, rows_total=None, row_offset: int = 0) -> np.ndarray:
    """What a seeded sampler call (no noise tensor, seed != 0) divides the probabilities by: float64 [rows, 512],
        q = max(-log1p(-u), 2^-30),   u = sampler_uniform(...),
    for the rows [row_offset, row_offset + rows) of a step of ``rows_total`` rows (None: ``rows``).  Counter-based: no state, the
    rows of a shard or a clip group are the rows of the whole batch.  A generation of S samples per clip numbers its rows
    (shard_row_offset + b) * S + s out of shard_rows_total * S; ``step`` is the decode step (token column), up to 2^63.
    The kernel evaluates log1pf in float32; this definition does not restate that rounding (tests leave out the rows whose two best
    scores it could reorder, dimx.sampling.undecidable)."""
    return np.maximum(-np.log1p(-sampler_uniform(seed, step, rows, rows_total, row_offset)), SAMPLER_NOISE_FLOOR)


# ---------------------------------------------------------------------------------------------------------------------
# Dropout keep-mask of the VQ-VAE training step (csrc/train_vq.hip mirrors it bit for bit)
# ---------------------------------------------------------------------------------------------------------------------
DROPOUT_SITE_ENCODER = 0
DROPOUT_SITE_DECODER = 1


def dropout_key(seed: int, step: int, site: int) -> int:
    """key(seed, step, site) = mix(seed + (2 step + site + 1) * GOLD) (mod 2^64)."""
    z = (int(seed) + (2 * int(step) + int(site) + 1) * 0x9E3779B97F4A7C15) & _MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK
    return z ^ (z >> 31)


def dropout_threshold(p: float) -> int:
    """keep iff the 24-bit draw >= floor(p * 2^24), p taken as float32 (what the C-ABI receives)."""
    return int(float(np.float32(p)) * 16777216.0)


def dropout_keep(seed: int, step: int, site: int, shape, p: float) -> np.ndarray:
    """Keep-mask [B,T,C] (bool) of Dropout(p) after the positional encoding of the VQ-VAE's encoder (site 0) or decoder
    (site 1) in training step ``step``: element (b, t, c) is kept iff
        (mix(key(seed, step, site) + (ctr + 1) * GOLD) >> 40) >= floor(p * 2^24),   ctr = (b * 65536 + t) * 512 + c,
    mix = splitmix64's finaliser.  Counter-based: no state, any element can be regenerated alone (the backward pass keeps
    nothing but (seed, step)).  Needs T <= 65536 and C <= 512."""
    B, T, C = (int(s) for s in shape)
    assert T <= 65536 and C <= 512
    key = np.uint64(dropout_key(seed, step, site))
    b = np.arange(B, dtype=np.uint64)[:, None, None]
    t = np.arange(T, dtype=np.uint64)[None, :, None]
    c = np.arange(C, dtype=np.uint64)[None, None, :]
    with np.errstate(over="ignore"):
        ctr = (b * np.uint64(65536) + t) * np.uint64(512) + c
        r = _mix(key + (ctr + np.uint64(1)) * _GOLD)
    return (r >> np.uint64(40)) >= np.uint64(dropout_threshold(p))


def dropout_scale_mask(seed: int, step: int, site: int, shape, p: float):
    """float32 multiplier [B,T,C]: keep / (1 - p) (torch.nn.Dropout's scaling), 0 where dropped."""
    keep = dropout_keep(seed, step, site, shape, p)
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    return np.where(keep, scale, np.float32(0.0)).astype(np.float32)
