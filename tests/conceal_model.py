"""The concealment rule (MP2VG_PARSE_CONCEAL, include/mp2vg.h) stated in plain numpy, from a
pristine Parsed (no flag) and the rows to replace.  It never calls the library's conceal path: the
expected picture records, MB records, compacted coefficient words and damage order come from the
pristine records alone.

The rule: a damaged slice, or a row without a slice, is replaced as a whole row of mb_width
records with qscale 1 and coef_off the running word offset:
  P picture                      flags FWD, vectors 0, cbp 0, no words
  B picture                      FWD when the picture has a forward reference, else BWD
  I picture after an anchor      as P, from that anchor (its conceal reference); the picture
                                 record becomes type 2 (fwd_slot holds the conceal reference in
                                 every I picture's record under the flag, damaged or not)
  no reference at all            intra, every block coded by one DC word, mid-grey
The grey DC word carries the level the emitter would pack for a zero differential after a
predictor reset: (1 << (intra_dc_precision + 7)) << (3 - intra_dc_precision) = 1024 for every
precision.
A picture's words are its slices' in stream order (a replaced slice's words in the slice's place),
then those of its missing rows, rows ascending; the damage list has the same order."""
import numpy as np

from tiny_mp2v_dec_amd._lib import COEF_DC, MB_BWD, MB_DTYPE, MB_FWD, MB_INTRA, PIC_DTYPE

NBLOCKS = {1: 6, 2: 8, 3: 12}
GREY_DC = 1024


def conceal_refs(pics):
    """per picture: the newest anchor (I or P, by the coded type) before it in decode order, -1 if none"""
    out, last = np.full(len(pics), -1, np.int32), -1
    for p, rec in enumerate(pics):
        out[p] = last
        if int(rec["picture_coding_type"]) != 3:
            last = p
    return out


def flagged_pictures(pics):
    """the picture records of an undamaged stream under the flag: I pictures carry their conceal
    reference (a decode index = slot in a Parsed) in fwd_slot"""
    out = np.array(pics, PIC_DTYPE)
    refs = conceal_refs(pics)
    i_pic = out["picture_coding_type"] == 1
    out["fwd_slot"][i_pic] = refs[i_pic]
    return out


def replacement_row(pic, ref, y, mbw, cf):
    """(records with coef_off relative to the row, words) of row y of picture record `pic` (coded
    type, pristine references) whose conceal reference is `ref`"""
    nb = NBLOCKS[cf]
    row = np.zeros(mbw, MB_DTYPE)
    row["x"], row["y"], row["qscale"] = np.arange(mbw), y, 1
    t = int(pic["picture_coding_type"])
    if t == 2:
        flags = MB_FWD
    elif t == 3:
        flags = MB_FWD if int(pic["fwd_slot"]) >= 0 else (MB_BWD if int(pic["bwd_slot"]) >= 0 else None)
    else:
        flags = MB_FWD if ref >= 0 else None
    if flags is not None:
        row["flags"] = flags
        return row, np.zeros(0, np.uint32)
    row["flags"], row["cbp"], row["ncoef"] = MB_INTRA, (1 << nb) - 1, nb
    row["coef_off"] = np.arange(mbw) * nb
    x, b = np.meshgrid(np.arange(mbw), np.arange(nb), indexing="ij")
    words = (GREY_DC | (b << 22) | COEF_DC | ((x & 7) << 26)).astype(np.uint32).ravel()
    return row, words


def conceal(parsed, damaged=(), missing=()):
    """(pics, mbs, coefs, damage rows) expected of the flagged parse of a stream whose slices
    `damaged` [(picture, row)] fail and whose slices `missing` [(picture, row)] are absent, given the
    pristine stream's Parsed.  damage rows: [(picture, row)] in the order the library reports."""
    mbw, mbh = parsed.width // 16, parsed.height // 16
    per = mbw * mbh
    damaged, missing = set(map(tuple, damaged)), set(map(tuple, missing))
    assert not damaged & missing
    refs = conceal_refs(parsed.pics)
    pics = flagged_pictures(parsed.pics)
    mbs = np.array(parsed.mbs, MB_DTYPE)
    words, order, nw = [], [], 0
    for p in range(parsed.npics):
        rec = parsed.pics[p]
        first = int(rec["mb_first"])
        rows = [mbs[first + y * mbw: first + (y + 1) * mbw] for y in range(mbh)]  # views
        # stream order of the pristine slices: by their first word (rows without words tie: any order)
        stream = sorted(range(mbh), key=lambda y: (int(parsed.mbs["coef_off"][first + y * mbw]), y))
        todo = [y for y in stream if (p, y) not in missing] + sorted(y for y in range(mbh) if (p, y) in missing)
        for y in todo:
            if (p, y) in damaged or (p, y) in missing:
                row, w = replacement_row(rec, int(refs[p]), y, mbw, parsed.chroma_format)
                order.append((p, y))
            else:
                row = rows[y].copy()
                c0 = int(row["coef_off"][0])
                w = parsed.coefs[c0:c0 + int(row["ncoef"].sum())]
                row["coef_off"] -= c0
            row["coef_off"] += nw
            rows[y][:] = row
            words.append(w)
            nw += len(w)
        if any(q == p for q, _ in order) and int(rec["picture_coding_type"]) == 1 and refs[p] >= 0:
            pics["picture_coding_type"][p] = 2
    coefs = np.concatenate(words).astype(np.uint32) if words else np.zeros(0, np.uint32)
    assert per * parsed.npics == len(mbs)
    return pics, mbs, coefs, order
