"""The residual export's definition (include/mp2vg.h "residual export") in numpy over the oracle
library's public entry points, which test_oracle_golden.py pins to the compiled reference: for
each coded block the words of its block index go through oracle_dequant_block, and the block
through the oracle's IDCT twice, added to a prediction of all 0 and of all 255:

    r_pos = out0            (= clip(r, 0, 255))
    r_neg = out255 - 255    (= clip(r, -255, 0))
    R16 = r_pos + r_neg     (= clip(r, -255, 255)),   R8 = clip(R16, -128, 127)

placed with the rule of block_origin (oracle/mp2v_oracle.c), restated here."""
import ctypes

import numpy as np

import _oracle
from tiny_mp2v_dec_amd._lib import MB_DCT_FIELD, MB_INTRA

NB = {1: 6, 2: 8, 3: 12}
_P0 = np.zeros(64, np.uint8)
_P255 = np.full(64, 255, np.uint8)
_cache = {}


def plane_shapes(width, height, cf):
    cw = width if cf == 3 else width // 2
    ch = height // 2 if cf == 1 else height
    return (height, width), (ch, cw), (ch, cw)


def block_origin(cf, b, dct_field):
    """(plane, x, y, row step) of block b inside its MB."""
    if b < 4:
        return (0, (b & 1) * 8, b >> 1, 2) if dct_field else (0, (b & 1) * 8, (b >> 1) * 8, 1)
    plane = 2 if b & 1 else 1
    k = (b - 4) >> 1
    x = 8 if k >= 2 else 0
    lower = k in (1, 3)
    if dct_field and cf != 1:
        return plane, x, 1 if lower else 0, 2
    return plane, x, 8 if lower else 0, 1


def dequant(words, W, qs, intra, alt):
    """QFS int16[64] of a block's words (oracle_dequant_block)."""
    words = np.ascontiguousarray(words, np.uint32)
    W = np.ascontiguousarray(W, np.uint8)
    qfs = np.zeros(64, np.int16)
    vp = ctypes.c_void_p
    _oracle.lib().oracle_dequant_block(words.ctypes.data_as(vp), len(words), W.ctypes.data_as(vp), int(qs),
                                       1 if intra else 0, int(alt), qfs.ctypes.data_as(vp))
    return qfs


def block_residual(words, W, qs, intra, alt):
    """R16 (8, 8) int16 of one coded block."""
    key = (np.asarray(words, np.uint32).tobytes(), np.asarray(W, np.uint8).tobytes(), int(qs), bool(intra), int(alt))
    r = _cache.get(key)
    if r is None:
        F = dequant(words, W, qs, intra, alt)
        r_pos = _oracle.idct(F, _P0).astype(np.int16)
        r_neg = _oracle.idct(F, _P255).astype(np.int16) - 255
        r = _cache[key] = (r_pos + r_neg).reshape(8, 8)
    return r


def picture(pic, mbs, coefs, width, height, cf, zero_intra=False):
    """[y, cb, cr] int16 of one picture record."""
    nb = NB[cf]
    out = [np.zeros(s, np.int16) for s in plane_shapes(width, height, cf)]
    mbw, mbh = width // 16, height // 16
    mw = [16, 16 if cf == 3 else 8, 16 if cf == 3 else 8]
    mh = [16, 8 if cf == 1 else 16, 8 if cf == 1 else 16]
    first = int(pic["mb_first"])
    alt = int(pic["alternate_scan"])
    for i in range(mbw * mbh):
        m = mbs[first + i]
        cbp = int(m["cbp"])
        intra = bool(int(m["flags"]) & MB_INTRA)
        if not cbp or (zero_intra and intra):
            continue
        w = coefs[int(m["coef_off"]):int(m["coef_off"]) + int(m["ncoef"])]
        wb = (w >> 22) & 15
        dctf = bool(int(m["flags"]) & MB_DCT_FIELD)
        mx, my = i % mbw, i // mbw
        for b in range(nb):
            if not cbp >> b & 1:
                continue
            R = block_residual(w[wb == b], pic["W"][(0 if b < 6 else 2) + (0 if intra else 1)], m["qscale"], intra, alt)
            plane, x, y, step = block_origin(cf, b, dctf)
            X, Y = mx * mw[plane] + x, my * mh[plane] + y
            out[plane][Y:Y + 8 * step:step, X:X + 8] = R
    return out


def constant_reference(pics, slot):
    """A copy of the picture records in which every P and B picture predicts from `slot` alone (a
    slot no picture of the batch writes): filled with a constant c, every prediction is c whatever
    the vectors, so a decoded sample is clip8(c + r).  The second yardstick: with c = 0 and c = 255,
    out0 + out255 - 255 == R16 on non-intra MBs and out == clip(R16, 0, 255) on intra MBs."""
    pics = np.array(pics, copy=True)
    assert slot not in [int(s) for s in pics["dst_slot"]]
    for p in pics:
        t = int(p["picture_coding_type"])
        p["fwd_slot"] = slot if t > 1 else -1
        p["bwd_slot"] = slot if t == 3 else -1
    return pics


def intra_mask(pic, mbs, width, height, cf):
    """Per plane, a bool array that is True on the samples of intra MBs."""
    mbw, mbh = width // 16, height // 16
    intra = (mbs["flags"][int(pic["mb_first"]):int(pic["mb_first"]) + mbw * mbh] & MB_INTRA).astype(bool).reshape(mbh, mbw)
    return [np.repeat(np.repeat(intra, h // mbh, 0), w // mbw, 1) for h, w in plane_shapes(width, height, cf)]


def check_identity(R16, dec0, dec255, mask):
    """The whole-picture identity for one picture: planes R16 (int16), the two decodes (uint8)."""
    for k in range(3):
        r, a, b, m = R16[k].astype(np.int32), dec0[k].astype(np.int32), dec255[k].astype(np.int32), mask[k]
        assert np.array_equal((a + b - 255)[~m], r[~m]), ("non-intra", k)
        assert np.array_equal(a[m], np.clip(r, 0, 255)[m]) and np.array_equal(b[m], a[m]), ("intra", k)


def model(pics, mbs, coefs, width, height, cf, order=None, dtype="int16", zero_intra=False):
    """(y, cb, cr) as the export defines them, pictures stacked in `order` (None: batch order)."""
    coefs = np.asarray(coefs, np.uint32)
    order = range(len(pics)) if order is None else [int(o) for o in order]
    done = {}
    for o in order:
        if o not in done:
            done[o] = picture(pics[o], mbs, coefs, width, height, cf, zero_intra)
    planes = [np.stack([done[o][k] for o in order]) for k in range(3)]
    if dtype == "int8":
        planes = [np.clip(p, -128, 127).astype(np.int8) for p in planes]
    return tuple(planes)
