"""Plain numpy / Python-int model of the motion export (include/mp2vg.h "motion export"), written
from the definition; it never calls the library.  model(pics, mbs, coefs, cf, order) -> (mv, info,
act) as the export lays them out."""
import numpy as np

INTRA, FWD, BWD, FIELD_MC = 1, 2, 4, 8
COEF_DC = 1 << 30
NBLOCKS = {1: 6, 2: 8, 3: 12}


def mb_vectors(flags, mv):
    """The 8 mv channels of one MB: flags an int, mv[r][s][k] ints."""
    out = [0] * 8
    if flags & INTRA:
        return out
    used = [bool(flags & FWD) or not flags & BWD, bool(flags & BWD)]
    for s in range(2):
        if not used[s]:
            continue
        for r in range(2):
            if flags & FIELD_MC:
                sel = 1 if flags & (1 << (8 + 2 * r + s)) else 0
                x, y = mv[r][s][0], 2 * mv[r][s][1] + 2 * (sel - r)
            else:
                x, y = mv[0][s][0], mv[0][s][1]
            out[4 * s + 2 * r + 0] = x
            out[4 * s + 2 * r + 1] = y
    return out


def mb_activity(words, nb):
    """(count[nb], sum[nb]) over the coefficient words (Python ints) of one MB."""
    cnt, tot = [0] * nb, [0] * nb
    for w in words:
        b = (w >> 22) & 15
        if b >= nb:
            continue
        cnt[b] += 1
        if not w & COEF_DC:
            level = w & 0xFFFF
            level -= 0x10000 if level & 0x8000 else 0
            tot[b] += abs(level)
    return cnt, tot


def model(pics, mbs, coefs, cf, order=None):
    nb = NBLOCKS[cf]
    order = list(range(len(pics))) if order is None else [int(i) for i in order]
    mbw, mbh = int(pics[0]["mb_width"]), int(pics[0]["mb_height"])
    M = mbw * mbh
    n = len(order)
    mv = np.zeros((n, 8, M), np.int64)
    info = np.zeros((n, 4, M), np.int64)
    act = np.zeros((n, 2, nb, M), np.int64)
    words = [int(w) for w in np.asarray(coefs, np.uint32)]
    for f, p in enumerate(order):
        first = int(pics[p]["mb_first"])
        for i in range(M):
            m = mbs[first + i]
            flags = int(m["flags"])
            mv[f, :, i] = mb_vectors(flags, [[[int(m["mv"][r, s, k]) for k in range(2)] for s in range(2)]
                                             for r in range(2)])
            info[f, :, i] = (flags & 0x0F1F, int(m["cbp"]), int(m["qscale"]), int(m["ncoef"]))
            off, nc = int(m["coef_off"]), int(m["ncoef"])
            cnt, tot = mb_activity(words[off:off + nc], nb)
            act[f, 0, :, i] = cnt
            act[f, 1, :, i] = tot
    assert mv.min(initial=0) >= -32768 and mv.max(initial=0) <= 32767
    return (mv.astype(np.int16).reshape(n, 8, mbh, mbw), info.astype(np.uint16).reshape(n, 4, mbh, mbw),
            act.astype(np.int32).reshape(n, 2, nb, mbh, mbw))
