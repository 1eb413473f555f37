"""The yardstick of the items launch of the tensor export: a numpy model of "Items" in
include/mp2vg.h.  It shares no code with the library.  An item is (slot, mode, crop, flip): its image
is field_model.q_image of its rectangle under its field mode, mirrored by [..., ::-1] when flipped,
then tensor_model.normalise; the launch is the stack of its items, planar output in clip order by a
reshape and a transpose (not by the contract's index formula).

    tensor(frames, cf, matrix, linear, items, size, dtype, scale, bias, packed, clip_len)
                                        -> bit patterns, (n, h, w, 3), (n, 3, h, w) or (n / T, 3, T, h, w)
    segments(src_w, out_w)              -> segment count of a horizontal table (the 2,048-column window rule)
    plan(items, coded, size)            -> the expected mp2vg_tensor_items_plan result
"""
import numpy as np

import field_model as FM
import tensor_model as T

SEG_COLS = 2048     # source columns one workgroup keeps (include/mp2vg.h says nothing: the kernel's window)
RECORD_WORDS = 16   # int32 words of one staged item record


class Frames:
    """The frames of a launch (a dict or list of planes per slot) with the Q image of every (slot,
    mode, size, crop) computed once and left unchanged."""

    def __init__(self, frames, cf, matrix=1, linear=True):
        self.frames, self.cf, self.matrix, self.linear = frames, cf, matrix, linear
        self.memo = {}

    def q(self, slot, mode, size, crop):
        key = (slot, mode, tuple(size), None if crop is None else tuple(crop))
        if key not in self.memo:
            q = FM.q_image(self.frames[slot], self.cf, self.matrix, self.linear, mode, size, crop)
            q.setflags(write=False)
            self.memo[key] = q
        return self.memo[key]

    def image(self, item, size, dtype, scale, bias):
        """(3, h, w) bit patterns of one item."""
        slot, mode, crop, flip = item
        q = self.q(slot, mode, size, crop)
        if flip:
            q = q[..., ::-1]
        return T.normalise(q, dtype, scale, bias)

    def tensor(self, items, size, dtype="uint8", scale=(1, 1, 1), bias=(0, 0, 0), packed=False, clip_len=1):
        imgs = np.stack([self.image(it, size, dtype, scale, bias) for it in items])   # (n, 3, h, w)
        n, _, h, w = imgs.shape
        if packed:
            return np.ascontiguousarray(np.moveaxis(imgs, 1, -1))
        assert clip_len >= 1 and n % clip_len == 0
        if clip_len == 1:
            return imgs
        return np.ascontiguousarray(imgs.reshape(n // clip_len, clip_len, 3, h, w).transpose(0, 2, 1, 3, 4))


def segments(src_w, out_w):
    """Runs of output columns whose taps fit one window of SEG_COLS source columns, greedily from
    the left: the count."""
    first, count, _ = T.taps(src_w, out_w)
    n, o = 0, 0
    while o < out_w:
        base, e = int(first[o]), o
        while e < out_w and int(first[e] + count[e]) <= base + SEG_COLS:
            e += 1
        assert e > o
        n, o = n + 1, e
    return n


def plan(items, coded, size):
    """items: (slot, mode, crop, flip) each; coded = (w, h); size = (out_w, out_h).  Tables are
    per distinct src_w / src_h in order of first use; a table holds its segment list (4 words a
    segment), one `first` per output and the weights at the table's longest tap count (vertical: a
    `count` per output too)."""
    ws, hs, htab, vtab = [], [], [], []
    for _, _, crop, _ in items:
        sw, sh = coded if crop is None else crop[2:]
        if sw not in ws:
            ws.append(sw)
        if sh not in hs:
            hs.append(sh)
        htab.append(ws.index(sw))
        vtab.append(hs.index(sh))
    nsegs = [segments(sw, size[0]) for sw in ws]
    words = RECORD_WORDS * len(items)
    for sw, ns in zip(ws, nsegs):
        words += 4 * ns + size[0] + size[0] * T.taps(sw, size[0])[2].shape[1]
    for sh in hs:
        words += 2 * size[1] + size[1] * T.taps(sh, size[1])[2].shape[1]
    return {"htab": htab, "vtab": vtab, "n_htab": len(ws), "n_vtab": len(hs),
            "grid_x": max(nsegs[k] for k in htab), "words": words}
