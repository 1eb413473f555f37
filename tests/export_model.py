"""The yardstick of the RGB export: a plain numpy / fractions.Fraction model of the arithmetic in
include/mp2vg.h ("RGB export").  It shares no code with the library: the coefficients are derived
here from Kr and Kb in exact rationals, and the pixels with whole-array integer arithmetic.

    coefficients(matrix)                       -> (cy, crv, cgu, cgv, cbu)
    chroma_at(C, cf, linear, w, h)             -> the 8-bit chroma sample of every luma position
    export(planes, cf, matrix, linear, packed, size) -> (3, h, w) or (h, w, 3) uint8
"""
from fractions import Fraction as F

import numpy as np

# matrix_coefficients code (ISO/IEC 13818-2 Table 6-9) -> (Kr, Kb)
KR_KB = {1: (F(2126, 10000), F(722, 10000)),   # BT.709
         4: (F(30, 100), F(11, 100)),          # FCC
         5: (F(299, 1000), F(114, 1000)),      # BT.470BG
         6: (F(299, 1000), F(114, 1000)),      # SMPTE 170M
         7: (F(212, 1000), F(87, 1000))}       # SMPTE 240M
MATRICES = (1, 4, 5, 6, 7)


def _q14(x):
    """floor(x 2^14 + 1/2) of a non-negative rational."""
    assert x >= 0
    return (x * 2 ** 14 + F(1, 2)).__floor__()


def coefficients(matrix):
    kr, kb = KR_KB[matrix]
    kg = 1 - kr - kb
    s = F(255, 224)
    cy = _q14(F(255, 219))
    crv = _q14(s * 2 * (1 - kr))
    cbu = _q14(s * 2 * (1 - kb))
    cgu = -_q14(s * 2 * (1 - kb) * kb / kg)
    cgv = -_q14(s * 2 * (1 - kr) * kr / kg)
    return cy, crv, cgu, cgv, cbu


def chroma_at(C, cf, linear, w, h):
    """C: the whole coded chroma plane (the taps clamp to it, not to the w x h rectangle)."""
    C = np.asarray(C).astype(np.int32)
    ys, xs = np.arange(h), np.arange(w)
    if cf == 1:
        j = ys >> 1
        j1 = np.clip(np.where(ys % 2 == 0, j - 1, j + 1), 0, C.shape[0] - 1)
        wv0, wv1 = 3, 1
    else:
        j = j1 = ys
        wv0, wv1 = 4, 0
    if cf == 3:
        k = k1 = xs
    else:
        k = xs >> 1
        k1 = np.clip(np.where(xs % 2 == 0, k, k + 1), 0, C.shape[1] - 1)
    if not linear:
        return C[j][:, k]
    return (wv0 * (C[j][:, k] + C[j][:, k1]) + wv1 * (C[j1][:, k] + C[j1][:, k1]) + 4) >> 3


def convert(Y, Cb, Cr, matrix):
    """(R, G, B) uint8 arrays of same-shape 8-bit Y, Cb, Cr arrays; signed 32-bit arithmetic."""
    cy, crv, cgu, cgv, cbu = (np.int32(v) for v in coefficients(matrix))
    Y, Cb, Cr = (np.asarray(a).astype(np.int32) for a in (Y, Cb, Cr))
    yt = cy * (Y - 16) + 8192
    r = (yt + crv * (Cr - 128)) >> 14
    g = (yt + cgu * (Cb - 128) + cgv * (Cr - 128)) >> 14
    b = (yt + cbu * (Cb - 128)) >> 14
    return tuple(np.clip(c, 0, 255).astype(np.uint8) for c in (r, g, b))


def export(planes, cf, matrix, linear, packed, size=None):
    """planes: [Y, Cb, Cr], each its whole coded plane (no stride padding)."""
    Y, Cb, Cr = planes
    w, h = size if size else (Y.shape[1], Y.shape[0])
    rgb = convert(Y[:h, :w], chroma_at(Cb, cf, linear, w, h), chroma_at(Cr, cf, linear, w, h), matrix)
    return np.stack(rgb, axis=-1 if packed else 0)
