"""Damaged streams for the concealment tests (CPU and GPU) and tests/golden/make_conceal_fixtures.py:
a chosen slice of any stream made to fail (parse_mutants.failing_substitution does this for
one-slice pictures only), slices deleted, the multi-fault stream, the geometry corners, and the
repaired twin of a damaged stream, whose replacement slice comes from the independent writer of
directed_syntax.py.  One place, so that the CPU tests, the GPU tests and the fixture maker cannot
drift apart."""
import json
import os
import re

import directed_syntax as DS
import parse_mutants as PM
from tiny_mp2v_dec_amd import _lib
from tiny_mp2v_dec_amd.records import Scan, generate_es

FIXTURES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conceal")
UNCOVERED = "picture with a macroblock row not covered by any slice"
# every slice-level rejection text (sp_reason_text of SP_R_MB_BEYOND_ROW .. SP_R_ROW_NOT_WHOLE)
SLICE_LEVEL = PM.SLICE_REASONS + [PM.VLC0_REASON, "bad dct_dc_size", "slice overruns the buffer"]


def slice_level(msg):
    """the message blames one slice for a reason the flag conceals"""
    return PM.blamed_picture(msg) is not None and any(r in msg for r in SLICE_LEVEL)


def slice_table(es):
    """[(picture, row, start, end)] of the slices in stream order, found without the library:
    end is the next start code (streams of at most 175 rows)"""
    codes = [m.start() for m in re.finditer(rb"\x00\x00\x01", es)]
    out, pic = [], -1
    for i, o in enumerate(codes):
        c = es[o + 3]
        if c == 0x00:
            pic += 1
        elif 0x01 <= c <= 0xAF:
            out.append((pic, c - 1, o, codes[i + 1] if i + 1 < len(codes) else len(es)))
    return out


def failing_substitution(es, w, h, cf, j, other_than=None):
    """The first single-byte substitution (positions ascending, then values ascending) in the
    payload of slice j (stream order) that the scan lets through with the same pictures and slices
    and that makes exactly that slice fail in the twin for a slice-level reason, optionally one
    other than `other_than`.  Returns (position, value, reason text)."""
    table = slice_table(es)
    pic, _, lo, hi = table[j]
    with Scan(es, w, h, cf) as sc:
        n, ns = sc.npics, sc.nslices
    for pos in range(lo + 4, hi):
        for val in range(256):
            if val == es[pos]:
                continue
            b = PM.mutate(es, pos, val)
            try:
                s2 = Scan(b, w, h, cf)
            except _lib.Mp2vgError:
                continue
            with s2:
                if s2.npics != n or s2.nslices != ns:
                    continue
                try:
                    s2.parse_host(pic, 1)
                except _lib.Mp2vgError as e:
                    why = PM.detail(str(e)).split(": ", 1)[1]
                    if PM.blamed_picture(str(e)) == (pic, lo) and slice_level(str(e)) and why != other_than:
                        return pos, val, why
    raise AssertionError(f"no single-byte substitution makes slice {j} fail")


def damage_slices(es, w, h, cf, js):
    """es with the slices `js` (stream order) made to fail, the later ones for reasons other than
    the first one's.  Returns (bytes, {j: reason text})."""
    js = sorted(js)
    out, why = es, {}
    for j in js:
        pos, val, r = failing_substitution(es, w, h, cf, j, other_than=why.get(js[0]))
        out = PM.mutate(out, pos, val)
        why[j] = r
    return out, why


def delete_slices(es, js):
    """es without the bytes of slices `js`: what a lost packet leaves"""
    table = slice_table(es)
    for j in sorted(js, reverse=True):
        es = es[:table[j][2]] + es[table[j][3]:]
    return es


# ---- the multi-fault stream -------------------------------------------------------------------------
# decode order I B B P B B | I B B P B B; the first GOP's leading B pictures have no forward reference
MULTI = dict(width=176, height=48, chroma_format=1, n_gops=2, gop_n=6, gop_m=3, seed=77)
MULTI_DAMAGE = [(0, 1),          # the stream's first anchor: grey
                (1, 0),          # a B picture without a forward reference: backward
                (3, 2),          # a P picture
                (4, 1),          # a B picture with both references: forward
                (6, 0),          # the second GOP's I picture: re-typed, from picture 3
                (9, 0), (9, 2)]  # two rows of one picture
# damage that leaves the first GOP alone (its pictures then equal the pristine decode)
LATE_DAMAGE = [(9, 1), (10, 2)]


def damaged_stream(kw, rows):
    """(damaged bytes, pristine bytes, width, height, chroma format, {(picture, row): reason text})
    of generate_es(**kw) with the slices of `rows` [(picture, row)] made to fail"""
    es = generate_es(**kw)
    w, h, cf = PM.geom(kw)
    table = slice_table(es)
    index = {(p, r): j for j, (p, r, _, _) in enumerate(table)}
    bad, why = damage_slices(es, w, h, cf, [index[pr] for pr in rows])
    return bad, es, w, h, cf, {(table[j][0], table[j][1]): r for j, r in why.items()}


# ---- geometry corners: the first picture's first row fails (grey), and a later picture's ------------
CORNERS = {
    "mbw1": dict(width=16, height=48, chroma_format=1, n_gops=1, gop_n=3, gop_m=1, leading_b=0, seed=31),
    "mbh1": dict(width=176, height=16, chroma_format=1, n_gops=1, gop_n=3, gop_m=1, leading_b=0, seed=32),
    "cf422": dict(width=48, height=32, chroma_format=2, n_gops=1, gop_n=3, gop_m=1, leading_b=0, seed=33),
    "cf444": dict(width=48, height=32, chroma_format=3, n_gops=1, gop_n=3, gop_m=1, leading_b=0, seed=34),
}
CORNER_DAMAGE = [(0, 0), (2, 0)]


# ---- repaired streams: the damaged slice replaced by one that codes the replacement row legally -----
class _Writer(DS.Stream):
    def ev(self, name):  # (the syntax event log belongs to the directed streams)
        pass


def legal_copy_slice(width, height, cf, pct, row):
    """Bytes of a slice of a P (pct 2) or B (3) picture with frame_pred_frame_dct = 1, written by the
    independent writer: first and last macroblock "MC, not coded" forward with zero vectors, the
    macroblocks between skipped.  It decodes to a copy of the forward reference's row."""
    S = _Writer("repair", width, height, cf)
    S.bw = DS.Bits()
    mbw = width // 16
    assert mbw >= 2
    zero = {0: [(0, (0, 0))]}
    S.slice(DS.Pic(pct, [None] * (height // 16), fpfd=1), row,
            DS.Row([DS.MB(DS.FWD, mv=zero), DS.MB(DS.FWD, skip=mbw - 2, mv=zero)]))
    return S.bw.bytes()


def repaired(es, width, height, cf, pct, pic, row):
    """es with slice (pic, row) replaced, byte-spliced between start codes, by legal_copy_slice"""
    _, _, lo, hi = next(t for t in slice_table(es) if t[:2] == (pic, row))
    return es[:lo] + legal_copy_slice(width, height, cf, pct, row) + es[hi:]


# the committed pairs (tests/golden/conceal/, written by tests/golden/make_conceal_fixtures.py):
# name -> generator parameters, the picture's coding type, (picture, row) of the damaged slice
REPAIR = dict(width=176, height=48, chroma_format=1, n_gops=1, gop_n=6, gop_m=3, leading_b=0, seed=55,
              frame_pred_frame_dct=1)  # decode order I P B B
REPAIR_CASES = {"p_row": (2, (1, 1)), "b_row": (3, (2, 2))}


def load_fixtures():
    with open(os.path.join(FIXTURES, "manifest.json")) as f:
        man = json.load(f)
    for e in man:
        for k in ("damaged", "repaired"):
            with open(os.path.join(FIXTURES, e[k]), "rb") as f:
                e[k + "_es"] = f.read()
    return man
