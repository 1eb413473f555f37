"""The yardstick of the tensor export's field modes: a numpy model of "Field modes" in
include/mp2vg.h.  It shares no code with the library.  Only step 1 of the tensor contract (the 8-bit
source image P of the whole coded frame) depends on the mode; the matrix arithmetic is
export_model.convert, the crop and the two filter passes tensor_model.resize, the normalisation
tensor_model.normalise.

    field_chroma(C, cf, linear, w, h)   -> the 8-bit field-sited chroma sample of every luma position
    lines(planes, cf, matrix, linear)   -> (3, H, W): row y is L_{y & 1}[y]
    source(planes, cf, matrix, linear, mode) -> (3, H, W) uint8, the source image P of the mode
    q_image(planes, cf, matrix, linear, mode, size, crop) -> Q (3, oh, ow)
    tensor(planes, cf, matrix, linear, mode, packed, size, crop, dtype, scale, bias) -> bit patterns
"""
import numpy as np

import export_model
import tensor_model as T

PROGRESSIVE, TOP, BOTTOM, WEAVE = 0, 1, 2, 3
MODES = {"progressive": PROGRESSIVE, "top": TOP, "bottom": BOTTOM, "weave": WEAVE}
# 4:2:0 LINEAR: y mod 4 -> (step from j to j1, wv0, wv1)
TAPS_420 = {0: (-2, 7, 1), 1: (-2, 5, 3), 2: (2, 5, 3), 3: (2, 7, 1)}


def field_chroma(C, cf, linear, w, h):
    """C: the whole coded chroma plane.  4:2:2 and 4:4:4 have no vertical subsampling: the field
    chroma of line y is its progressive chroma."""
    if cf != 1:
        return export_model.chroma_at(C, cf, linear, w, h)
    C = np.asarray(C).astype(np.int32)
    ch, cw = C.shape
    out = np.empty((h, w), np.int32)
    xs = np.arange(w)
    k = xs >> 1
    k1 = np.where(xs % 2 == 0, k, np.minimum(k + 1, cw - 1))
    for y in range(h):
        j = 2 * (y >> 2) + (y & 1)  # the chroma row of the same field
        step, wv0, wv1 = TAPS_420[y % 4]
        j1 = j + step
        if j1 < 0 or j1 > ch - 1:
            j1 = j                   # never leaves the field
        if linear:
            out[y] = (wv0 * (C[j, k] + C[j, k1]) + wv1 * (C[j1, k] + C[j1, k1]) + 8) >> 4
        else:
            out[y] = C[j, k]
    return out


def lines(planes, cf, matrix, linear):
    """(3, H, W) uint8: row y is L_{y & 1}[y], line y with the chroma of its own field."""
    Y, Cb, Cr = planes
    h, w = Y.shape
    return np.stack(export_model.convert(Y, field_chroma(Cb, cf, linear, w, h), field_chroma(Cr, cf, linear, w, h),
                                         matrix))


def source(planes, cf, matrix, linear, mode):
    """The 8-bit R'G'B' source image P of the whole coded frame in one mode."""
    if mode == PROGRESSIVE:
        return export_model.export(planes, cf, matrix, linear, False)
    L = lines(planes, cf, matrix, linear)
    if mode == WEAVE:
        return L
    p = 0 if mode == TOP else 1
    H = L.shape[1]
    assert H % 2 == 0
    P = np.empty_like(L)
    for y in range(H):
        if y % 2 == p:
            P[:, y] = L[:, y]
            continue
        a, b = y - 1, y + 1
        if a < 0:
            a = b
        if b > H - 1:
            b = a
        P[:, y] = (L[:, a].astype(np.int32) + L[:, b].astype(np.int32) + 1) >> 1
    return P


def q_image(planes, cf, matrix, linear, mode, size, crop=None):
    rgb = source(planes, cf, matrix, linear, mode)
    if crop is not None:
        x, y, w, h = crop
        rgb = rgb[:, y:y + h, x:x + w]
    return T.resize(rgb, size)


def tensor(planes, cf, matrix, linear, mode, packed, size, crop=None, dtype="uint8", scale=(1, 1, 1), bias=(0, 0, 0)):
    out = T.normalise(q_image(planes, cf, matrix, linear, mode, size, crop), dtype, scale, bias)
    return np.ascontiguousarray(np.moveaxis(out, 0, -1)) if packed else out
