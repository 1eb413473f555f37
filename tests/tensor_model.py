"""The yardstick of the tensor export: a numpy / fractions.Fraction model of the arithmetic in
include/mp2vg.h ("tensor export").  It shares no code with the library: the tap table comes from
the contract's rationals, the two passes are whole-array integer arithmetic on top of
export_model.export (the source image), and the normalise is a lookup table over the 16,321 values
of Q, built from exact rationals and rounded once.

    taps(src, out)                      -> (first[out], count[out], weights[out][max count])
    resize(P, size)                     -> Q, int32, P = (..., h, w) 8-bit image(s) -> (..., oh, ow)
    q_image(planes, cf, matrix, linear, size, crop) -> Q (3, oh, ow) of one frame
    lut(scale, bias, dtype)             -> the output element (as its bit pattern) of every Q
    tensor(planes, cf, matrix, linear, packed, size, crop, dtype, scale, bias)
                                        -> (3, oh, ow) or (oh, ow, 3) array of bit patterns
    bits(array)                         -> the bit patterns of a library result, to compare

Against torch's CPU interpolate(mode="bilinear", antialias=True) in float64 the model's Q / 64
differs by at most 0.0226 of an 8-bit step over the seven shapes of tests/test_tensor_cpu.py with
its seeded images (bound: 1/16 = the two roundings of 1/128 each plus the weight quantisation); the
identity size is exact.
"""
from fractions import Fraction as F
from functools import lru_cache

import numpy as np

import export_model

DTYPES = ("uint8", "float16", "bfloat16", "float32")
BITS = {"uint8": np.uint8, "float16": np.uint16, "bfloat16": np.uint16, "float32": np.uint32}
QMAX = 16320


@lru_cache(maxsize=None)
def taps(src, out):
    r = F(src, out)
    s = max(r, F(1))  # (any ratio: r <= 32 is the library's limit, not the definition's)
    rows = []
    for o in range(out):
        c = (o + F(1, 2)) * r
        first = max(0, (c - s + F(1, 2)).__floor__())
        end = min(src, (c + s + F(1, 2)).__floor__())
        t = [max(F(0), 1 - abs(j + F(1, 2) - c) / s) for j in range(first, end)]
        total = sum(t)
        q = [(tj / total * 2 ** 14 + F(1, 2)).__floor__() for tj in t]
        q[t.index(max(t))] += 2 ** 14 - sum(q)  # list.index: the lowest j on a tie
        rows.append((first, q))
    n = max(len(q) for _, q in rows)
    first = np.array([f for f, _ in rows], np.int32)
    count = np.array([len(q) for _, q in rows], np.int32)
    weights = np.array([q + [0] * (n - len(q)) for _, q in rows], np.int32)
    return first, count, weights


def _pass(P, src_axis_taps, shift, half):
    """One pass over the last axis of int32 P."""
    first, count, weights = src_axis_taps
    out = np.empty(P.shape[:-1] + (len(first),), np.int32)
    for o in range(len(first)):
        seg = P[..., first[o]:first[o] + count[o]].astype(np.int64)
        acc = (seg * weights[o, :count[o]].astype(np.int64)).sum(axis=-1) + half
        assert acc.max() < 2 ** 31
        out[..., o] = acc >> shift
    return out


def resize(P, size):
    """P: (..., h, w) values 0..255; size = (out_w, out_h); returns Q in 1/64 steps."""
    P = np.asarray(P).astype(np.int32)
    h, w = P.shape[-2:]
    V = np.swapaxes(_pass(np.swapaxes(P, -1, -2), taps(h, size[1]), 8, 128), -1, -2)  # vertical first
    return _pass(V, taps(w, size[0]), 14, 8192)


def q_image(planes, cf, matrix, linear, size, crop=None):
    rgb = export_model.export(planes, cf, matrix, linear, False)  # the whole coded frame, (3, h, w)
    if crop is not None:
        x, y, w, h = crop
        rgb = rgb[:, y:y + h, x:x + w]
    return resize(rgb, size)


def _f32_bits(x):
    """Bit pattern of the float32 nearest to the rational x (ties to even, overflow to infinity)."""
    sign = 0x80000000 if x < 0 else 0
    x = abs(x)
    if x == 0:
        return sign
    e = max(x.numerator.bit_length() - x.denominator.bit_length(), -126)
    while F(2) ** e > x and e > -126:
        e -= 1
    while F(2) ** (e + 1) <= x:
        e += 1
    m = x / F(2) ** (e - 23)  # in [2^23, 2^24), or below 2^23 for a subnormal
    n = m.__floor__()
    rem = m - n
    if rem > F(1, 2) or (rem == F(1, 2) and n & 1):
        n += 1
    if n == 1 << 24:
        n, e = 1 << 23, e + 1
    if e > 127:
        return sign | 0x7F800000
    if n < 1 << 23:
        return sign | n  # subnormal (biased exponent 0)
    return sign | ((e + 127) << 23) | (n - (1 << 23))


def _f32_to_f16_bits(u):
    """float32 bit patterns (finite or infinite) to float16 bit patterns, nearest even."""
    u = u.astype(np.int64)
    sign = (u >> 16) & 0x8000
    e = ((u >> 23) & 0xFF) - 127
    m = (u & 0x7FFFFF) | np.where(((u >> 23) & 0xFF) != 0, 0x800000, 0)
    e = np.where(((u >> 23) & 0xFF) == 0, -126, e)
    # value = m 2^(e - 23); float16 quantum 2^(max(e, -14) - 10)
    shift = 13 + np.maximum(-14 - e, 0)
    shift = np.minimum(shift, 40)
    n = m >> shift
    rem = m & ((np.int64(1) << shift) - 1)
    half = np.int64(1) << (shift - 1)
    n = n + ((rem > half) | ((rem == half) & (n & 1 == 1)))
    eb = np.where(e >= -14, e + 15, 1)  # n carries the implicit bit: bits = (eb - 1) << 10 + n
    bits = ((eb - 1) << 10) + n
    bits = np.where(e < -14, n, bits)
    bits = np.where((bits >= 0x7C00) | (((u >> 23) & 0xFF) == 0xFF), 0x7C00, bits)
    return (sign | bits).astype(np.uint16)


def _f32_to_bf16_bits(u):
    u = u.astype(np.int64)
    keep, rem = u >> 16, u & 0xFFFF
    keep = keep + ((rem > 0x8000) | ((rem == 0x8000) & (keep & 1 == 1)))
    return keep.astype(np.uint16)


def _dyadic(bits):
    """(n, e) with float32(bits) = n 2^e exactly (finite values)."""
    sign = -1 if bits >> 31 else 1
    eb, m = (bits >> 23) & 0xFF, bits & 0x7FFFFF
    assert eb != 0xFF
    return (sign * (m | 0x800000), eb - 150) if eb else (sign * m, -149)


def _f32_bits_dyadic(n, e):
    """_f32_bits of the rational n 2^e, in integers (the table's 49k entries; same rounding)."""
    sign = 0x80000000 if n < 0 else 0
    n = abs(n)
    if n == 0:
        return sign
    top = n.bit_length() - 1 + e           # 2^top <= value < 2^(top + 1)
    shift = max(top, -126) - 23 - e        # value = m 2^(max(top, -126) - 23), m = n / 2^shift
    if shift <= 0:
        m = n << -shift
    else:
        m, rem, half = n >> shift, n & ((1 << shift) - 1), 1 << (shift - 1)
        if rem > half or (rem == half and m & 1):
            m += 1
    ex = max(top, -126)
    if m == 1 << 24:
        m, ex = 1 << 23, ex + 1
    if ex > 127:
        return sign | 0x7F800000
    if m < 1 << 23:
        return sign | m
    return sign | ((ex + 127) << 23) | (m - (1 << 23))


@lru_cache(maxsize=None)
def _lut1(scale_bits, bias_bits, dtype):
    (ns, es), (nb, eb) = _dyadic(scale_bits), _dyadic(bias_bits)
    es -= 6                                 # Q / 64
    e = min(es, eb)
    f32 = np.array([_f32_bits_dyadic((q * ns << (es - e)) + (nb << (eb - e)), e) for q in range(QMAX + 1)], np.uint32)
    if dtype == "float32":
        return f32
    return _f32_to_f16_bits(f32) if dtype == "float16" else _f32_to_bf16_bits(f32)


def lut(scale, bias, dtype):
    """(3, 16321) bit patterns: the output element of channel c for every Q.  scale, bias: float32."""
    if dtype == "uint8":
        return np.tile(((np.arange(QMAX + 1) + 32) >> 6).astype(np.uint8), (3, 1))
    sb = np.asarray(scale, np.float32).view(np.uint32), np.asarray(bias, np.float32).view(np.uint32)
    return np.stack([_lut1(int(sb[0][c]), int(sb[1][c]), dtype) for c in range(3)])


def normalise(Q, dtype, scale, bias):
    """Q (3, oh, ow) -> bit patterns (3, oh, ow)."""
    table = lut(scale, bias, dtype)
    return np.stack([table[c][Q[c]] for c in range(3)])


def tensor(planes, cf, matrix, linear, packed, size, crop=None, dtype="uint8", scale=(1, 1, 1), bias=(0, 0, 0)):
    out = normalise(q_image(planes, cf, matrix, linear, size, crop), dtype, scale, bias)
    return np.ascontiguousarray(np.moveaxis(out, 0, -1)) if packed else out


def scale_bias(mean=None, std=None, dtype="float16"):
    """float32 scale and bias of the Python interface's mean / std (0..1 units)."""
    if dtype == "uint8":
        return np.ones(3, np.float32), np.zeros(3, np.float32)
    if mean is None:
        return np.full(3, np.float32(1.0 / 255.0)), np.zeros(3, np.float32)
    return (np.array([1.0 / (255.0 * s) for s in std]).astype(np.float32),
            np.array([-m / s for m, s in zip(mean, std)]).astype(np.float32))


def bits(a, dtype):
    """A library result (numpy array of the element type, or of raw bytes) as bit patterns."""
    return np.ascontiguousarray(a).view(BITS[dtype])
