"""The yardstick of the placed tensor export: a numpy / fractions.Fraction model of "Placement" in
include/mp2vg.h and of the two host helpers that compute a placement.  It shares no code with the
library, and changes neither tensor_model nor field_model: the picture is field_model.q_image at the
rectangle's size, pasted into a canvas of 64 * pad[c]; the normalise and the layout are tensor_model's
over the whole canvas.

    q_canvas(planes, cf, matrix, linear, mode, size, crop, rect, pad) -> Q (3, out_h, out_w)
    paste(q_img, size, rect, pad)       -> the same from a Q image computed elsewhere
    tensor(planes, cf, matrix, linear, mode, packed, size, crop, rect, pad, dtype, scale, bias)
    fit(mode, src, par, size)           -> (src_out, dst_out), in exact rationals
    pixel_aspect(code, W, H)            -> (n, d), or None for a code that gives none
"""
from fractions import Fraction as F

import numpy as np

import field_model as FM
import tensor_model as T

STRETCH, CONTAIN, COVER = 0, 1, 2
FITS = {"stretch": STRETCH, "contain": CONTAIN, "cover": COVER}
DAR = {2: F(4, 3), 3: F(16, 9), 4: F(221, 100)}


def paste(q_img, size, rect, pad):
    """q_img (3, dst_h, dst_w) at rect = (x, y, w, h) of a (3, out_h, out_w) canvas of 64 * pad[c]."""
    x, y, w, h = rect
    assert q_img.shape == (3, h, w) and 0 <= x and 0 <= y and x + w <= size[0] and y + h <= size[1]
    canvas = np.empty((3, size[1], size[0]), np.int32)
    for c in range(3):
        canvas[c] = 64 * int(pad[c])
    canvas[:, y:y + h, x:x + w] = q_img
    return canvas


def q_canvas(planes, cf, matrix, linear, mode, size, crop=None, rect=None, pad=(0, 0, 0)):
    rect = (0, 0, size[0], size[1]) if rect is None else rect
    return paste(FM.q_image(planes, cf, matrix, linear, mode, (rect[2], rect[3]), crop), size, rect, pad)


def tensor(planes, cf, matrix, linear, mode, packed, size, crop=None, rect=None, pad=(0, 0, 0), dtype="uint8",
           scale=(1, 1, 1), bias=(0, 0, 0)):
    out = T.normalise(q_canvas(planes, cf, matrix, linear, mode, size, crop, rect, pad), dtype, scale, bias)
    return np.ascontiguousarray(np.moveaxis(out, 0, -1)) if packed else out


def _round(v):
    """floor(v + 1/2) of a rational."""
    return (v + F(1, 2)).__floor__()


def _clamp(v, lo, hi):
    return min(max(v, lo), hi)


def fit(mode, src, par, size):
    """The rectangles of mp2vg_tensor_fit from the shapes as rationals: the source is shown at
    width : height = (w par_n) : (h par_d)."""
    mode = FITS.get(mode, mode)
    x, y, w, h = src
    ow, oh = size
    shape = F(w * par[0], h * par[1])          # of the displayed source
    if mode == STRETCH:
        return (x, y, w, h), (0, 0, ow, oh)
    if mode == CONTAIN:
        if shape >= F(ow, oh):                 # at least as wide as the output: full width, bars above and below
            dw, dh = ow, _clamp(_round(ow / shape), 1, oh)
        else:
            dw, dh = _clamp(_round(oh * shape), 1, ow), oh
        return (x, y, w, h), ((ow - dw) // 2, (oh - dh) // 2, dw, dh)
    assert mode == COVER
    pixel = F(par[0], par[1])
    if shape >= F(ow, oh):                     # too wide: keep the height, cut the width to the output's shape
        w2 = _clamp(_round(h * F(ow, oh) / pixel), 1, w)
        return (x + (w - w2) // 2, y, w2, h), (0, 0, ow, oh)
    h2 = _clamp(_round(w * pixel / F(ow, oh)), 1, h)
    return (x, y + (h - h2) // 2, w, h2), (0, 0, ow, oh)


def pixel_aspect(code, W, H):
    """13818-2 6.3.3: code 1 square pixels; 2..4 a display aspect ratio of W x H."""
    if code == 1:
        return 1, 1
    if code not in DAR:
        return None
    p = DAR[code] * F(H, W)
    return p.numerator, p.denominator
