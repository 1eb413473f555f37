"""Twin streams for MP2VG_PARSE_SLICES from the independent writer of tests/directed_syntax.py.

The compiled reference cannot pin a stream whose slices start in the middle of a row: it runs
skipped-macroblock prediction over the macroblocks in front of such a slice.  It decodes
the twin.  So every picture model here is written twice:

  "ms"   rows cut into slices at given columns; a slice's first macroblock_address_increment names
         its start column, its header carries the quantiser code in force (or a new one);
  "ref"  the same model with one slice per row, which the compiled reference decodes.

The macroblock models carry absolute vectors, absolute DC values (dc_abs) and quantiser codes, so the
writer codes each against the predictors of the form it writes (reset at every slice start in "ms",
carried across the cut in "ref") and both forms give ONE set of expected records.  A slice that
changes the quantiser carries the new code in its header in "ms"; in "ref" its first macroblock
carries it (macroblock_type | QUANT), so such a macroblock has a type that exists with QUANT.  No
slice begins or ends with a skipped macroblock, and vectors are small, so every delta fits f_code in
both forms.

directed_syntax.Stream writes one slice per row from column 0; SlStream overrides slice() and
macroblock() and leaves that file alone.
"""
import json
import os

import directed_syntax as DS
from directed_syntax import BWD, FWD, INTRA, PAT, QUANT, Block, MB, Pic, Row, fr, tex_mb

GOLDEN = os.path.join(DS.GOLDEN, "slices")


def _required():
    ev = [f"sl:split:{k}" for k in ("1_rest", "rest_1", "halves", "one_per_mb")]
    ev += [f"sl:pic:{t}:{cf}" for t in "IPB" for cf in (420, 422, 444)]
    ev += [f"sl:escapes:{n}" for n in (0, 1, 2, 31)]
    ev += [f"sl:x0:{x}" for x in (32, 33, 34, 66, 1023)]
    ev += ["sl:pmv_not_reset_in_ref:P", "sl:pmv_not_reset_in_ref:B", "sl:dc_not_reset_in_ref"]
    ev += ["sl:field_mc_both_sides", "sl:qcode_from_header", "sl:hdr_ext_mid_row", "sl:zero_bytes_mid_row",
           "sl:stuffing_mid_row", "sl:vpos_ext_with_cut", "sl:skip_inside_slice", "sl:more_slices_than_1024"]
    return ev


REQUIRED_EVENTS = _required()
_REQUIRED = set(REQUIRED_EVENTS)


class Cut:
    """A slice start at column x.  qcode = None: the header repeats the code in force; a number: the
    slice changes the quantiser.  ext, zero_bytes as directed_syntax.Row's (zero bytes after the slice)."""

    def __init__(self, x, qcode=None, ext=None, zero_bytes=0):
        self.x, self.qcode, self.ext, self.zero_bytes = x, qcode, ext, zero_bytes


class SRow(Row):
    """A row of the model: mbs cover [0, mbw) with no skip at a cut; cuts = [Cut] ascending, x > 0.
    Row.qcode / ext / zero_bytes belong to the slice that starts at column 0."""

    def __init__(self, mbs, cuts=(), **kw):
        Row.__init__(self, mbs, **kw)
        self.cuts = [c if isinstance(c, Cut) else Cut(c) for c in cuts]


class SlStream(DS.Stream):
    """form "ms" or "ref".  A negative stream (_negative) is written in "ms" only, from explicit
    slices: Pic.slices = [(row, start column, [MB], qcode)] in stream order."""

    def __init__(self, name, width, height, cf, form, **kw):
        DS.Stream.__init__(self, name, width, height, cf, **kw)
        assert form in ("ms", "ref")
        self.form = form
        self._first_inc = None
        self.nslices = 0
        self.slice_table = []  # ms: (picture, row, x0, x1) of every slice, in stream order

    def ev(self, name):
        if name.startswith("sl:"):
            assert name in _REQUIRED, name
            self.events.add(name)
        else:
            DS.Stream.ev(self, name)

    # ---- one row ---------------------------------------------------------------------------------
    def _columns(self, row):
        """[(column, MB)] of the coded macroblocks of a row"""
        out, x = [], 0
        for mb in row.mbs:
            x += mb.skip
            out.append((x, mb))
            x += 1
        assert x == self.mbw
        return out

    def slice(self, P, y, row):
        if getattr(P, "slices", None) is not None:  # a negative stream: explicit slices, written once
            if y == 0:
                for yy, x0, mbs, qcode in P.slices:
                    self._slice_ms(P, yy, x0, mbs, qcode, None, 0)
            return
        cuts = getattr(row, "cuts", [])
        cols = self._columns(row)
        starts = {x for x, _ in cols}
        for c in cuts:
            assert 0 < c.x < self.mbw and c.x in starts and c.x - 1 in starts, (self.name, y, c.x)
            assert dict(cols)[c.x].skip == 0
        if self.form == "ref":
            # the slice's new quantiser code travels in its first macroblock
            q_at = {c.x: c.qcode for c in cuts if c.qcode is not None}
            mbs = []
            for x, mb in cols:
                if x in q_at:
                    assert not mb.t & QUANT and (mb.t | QUANT) in DS.MBTYPE[P.pct], (self.name, y, x)
                    mb = MB(mb.t | QUANT, skip=mb.skip, q=q_at[x], field=mb.field, dct=mb.dct, mv=mb.mv, cmv=mb.cmv,
                            cbp=mb.cbp, blocks=mb.blocks)
                mbs.append(mb)
            return DS.Stream.slice(self, P, y, Row(mbs, qcode=row.qcode, ext=row.ext, zero_bytes=row.zero_bytes))
        # "ms": the events of the model are those of what the cuts separate in the ref form
        self._cut_events(P, y, row, cols, cuts)
        bounds = [0] + [c.x for c in cuts] + [self.mbw]
        heads = [Cut(0, row.qcode, row.ext, row.zero_bytes)] + list(cuts)
        code = row.qcode
        for k, c in enumerate(heads):
            code = c.qcode if c.qcode is not None else code
            mbs = [mb for x, mb in cols if bounds[k] <= x < bounds[k + 1]]
            code = self._slice_ms(P, y, c.x, mbs, code, c.ext, c.zero_bytes)

    def _cut_events(self, P, y, row, cols, cuts):
        t, cf = "IPB"[P.pct - 1], {1: 420, 2: 422, 3: 444}[self.cf]
        if not cuts:
            return
        self.ev(f"sl:pic:{t}:{cf}")
        xs = [c.x for c in cuts]
        if xs == [1] and self.mbw > 2:
            self.ev("sl:split:1_rest")
        if xs == [self.mbw - 1] and self.mbw > 2:
            self.ev("sl:split:rest_1")
        if xs == [self.mbw // 2]:
            self.ev("sl:split:halves")
        if xs == list(range(1, self.mbw)):
            self.ev("sl:split:one_per_mb")
        by_x = dict(cols)
        for c in cuts:
            a, b = by_x[c.x - 1], by_x[c.x]
            vec = lambda m: not m.t & INTRA and m.t & (FWD | BWD)  # noqa: E731
            if P.pct > 1 and vec(a) and vec(b) and any(v for s in a.mv.values() for _, tv in s for v in tv):
                if set(a.mv) & set(b.mv):
                    self.ev(f"sl:pmv_not_reset_in_ref:{t}")
                if a.field and b.field:
                    self.ev("sl:field_mc_both_sides")
            if a.t & INTRA and b.t & INTRA and not b.skip:
                self.ev("sl:dc_not_reset_in_ref")  # (dc_abs textures: the predictors are never at reset)
            if c.qcode is not None and c.qcode != row.qcode:
                self.ev("sl:qcode_from_header")
            if c.ext is not None:
                self.ev("sl:hdr_ext_mid_row")
            if c.zero_bytes:
                self.ev("sl:zero_bytes_mid_row")
            if self.vext:
                self.ev("sl:vpos_ext_with_cut")
            if c.x in (32, 33, 34, 66, 1023):
                self.ev(f"sl:x0:{c.x}")
            if c.x // 33 in (0, 1, 2, 31) and c.x >= 32:
                self.ev(f"sl:escapes:{c.x // 33}")

    def _slice_ms(self, P, y, x0, mbs, qcode, ext, zero_bytes):
        """one slice of the "ms" form: the header and slice-state reset of directed_syntax.Stream.slice
        (6.2.4, 7.2.1, 7.6.3.4), then the macroblocks from column x0"""
        b = self.bw
        if self.vext:
            b.start_code((y & 127) + 1)
            b.put(y >> 7, 3)
        else:
            assert y < 175
            b.start_code(y + 1)
        b.put(qcode, 5)
        if ext is not None:
            intra_slice, info = ext
            b.put(1, 1), b.put(intra_slice, 1), b.put(0, 7)
            for byte in info:
                b.put(1, 1), b.put(byte, 8)
        b.put(0, 1)
        self.P, self.y = P, y
        self.PMV = [[[0, 0], [0, 0]], [[0, 0], [0, 0]]]
        self.dc_reset = 1 << (P.prec + 7)
        self.dc = [self.dc_reset] * 3
        self.q = DS.qscale_of(qcode, P.qst)
        self._qcode = qcode
        self.prev = None
        self.hist = {0: [], 1: []}
        self.pending_reset = None
        self.copy_pending = None
        self.skipped_before = False
        self.q_from_mb = False
        self._dc_nonintra = False
        x = x0
        self._first_inc = x0 + 1
        for mb in mbs:
            assert not (self._first_inc is not None and mb.skip) or self._negative
            if mb.skip and self._first_inc is None:
                self.ev("sl:skip_inside_slice")
            x = self.macroblock(mb, x)
            if mb.t & QUANT:
                self._qcode = mb.q
        self.slice_table.append((self.npics, y, x0, x))
        self.nslices += 1
        k = b.align()
        if x0 and k and not self._negative:
            self.ev("sl:stuffing_mid_row")
        b.put(0, 8 * zero_bytes)
        return self._qcode

    def macroblock(self, mb, x):
        if self.form == "ref" or self._first_inc is None:
            return DS.Stream.macroblock(self, mb, x)
        # the slice's first macroblock: its increment is the start column + 1, and no skip run.
        # directed_syntax writes '1' (increment 1) first; everything after that code is kept.
        inc, self._first_inc = self._first_inc, None
        if mb.skip:  # (negative streams only)
            inc += mb.skip
            mb = MB(mb.t, q=mb.q, field=mb.field, dct=mb.dct, mv=mb.mv, cmv=mb.cmv, cbp=mb.cbp, blocks=mb.blocks)
        real, self.bw = self.bw, DS.Bits()
        try:
            x = DS.Stream.macroblock(self, mb, x)
        finally:
            tmp, self.bw = self.bw, real
        assert tmp.s[0] == DS.MBA[1] == "1"
        n = inc - 1
        while n + 1 > 33:
            real.code(DS.MB_ESCAPE)
            n -= 33
        real.code(DS.MBA[n + 1])
        for c in tmp.s[1:]:
            real.code(c)
        return x


# ---- picture content ----------------------------------------------------------------------------------
def _big(rng, n=3):
    return DS._ac(rng, n, big=7)


def intra_mb(S, rng, **kw):
    m = tex_mb(S, rng, nac=0, **kw)
    for b in m.blocks.values():
        b.coefs = _big(rng)
    return m


def inter_mb(S, rng, t, **kw):
    cbp = int(rng.integers(1, 1 << S.nblocks)) | 1
    return MB(t, cbp=cbp, blocks={b: Block(_big(rng, 2)) for b in range(S.nblocks) if cbp >> b & 1}, **kw)


def _vec(S, rng, x, y, k=0):
    """a small non-zero vector whose reads stay inside the planes from column x, row y (and from the
    skipped columns after it)"""
    vx = -(1 + k % 2) if x == S.mbw - 1 else 1 + (x + k) % 3
    vy = 0 if S.mbh == 1 else ((1 + k % 2) if y == 0 else -(1 + k % 2))
    return vx, vy


def _field(S, rng, x, y, k):
    vx, _ = _vec(S, rng, x, y, k)
    vy = 0 if S.mbh == 1 or y == 0 else -2
    return [((x + k) & 1, (vx, vy)), ((x + k + 1) >> 1 & 1, (-vx if 0 < x < S.mbw - 1 else vx, vy))]


def gen_row(S, rng, pct, y, cuts, field_at=None, skips=True, **kw):
    """a row of picture type pct whose macroblocks next to every cut are coded (I: intra; P, B:
    vectors in the same direction on both sides, field vectors where field_at names the cut), with
    intra, pattern-only, vector-only and skipped macroblocks in between"""
    cut_x = [c.x if isinstance(c, Cut) else c for c in cuts]
    keep = {0, S.mbw - 1} | set(cut_x) | {c - 1 for c in cut_x}
    mbs, skip = [], 0
    for x in range(S.mbw):
        if pct == 1:
            mbs.append(intra_mb(S, rng))
            continue
        near = x in cut_x or x + 1 in cut_x
        if skips and x not in keep and rng.integers(0, 3) == 0:
            skip += 1
            continue
        fld = field_at is not None and (x == field_at or x + 1 == field_at)
        kind = 0 if near else int(rng.integers(0, 4))
        if kind == 3:
            m = intra_mb(S, rng, skip=skip)
        elif pct == 2:
            if kind == 2:
                m = inter_mb(S, rng, PAT, skip=skip)
            else:
                mv = {0: _field(S, rng, x, y, 0) if fld else fr(*_vec(S, rng, x, y))}
                m = inter_mb(S, rng, FWD | PAT, skip=skip, mv=mv, field=fld) if kind == 0 else MB(FWD, skip=skip, mv=mv)
        else:
            dirs = (FWD | BWD) if near else (FWD, BWD, FWD | BWD)[int(rng.integers(0, 3))]
            mv = {s: (_field(S, rng, x, y, s) if fld else fr(*_vec(S, rng, x, y, s))) for s in (0, 1) if dirs & (FWD >> s)}
            m = inter_mb(S, rng, dirs | PAT, skip=skip, mv=mv, field=fld) if kind != 1 else MB(dirs, skip=skip, mv=mv)
        skip = 0
        mbs.append(m)
    return SRow(mbs, cuts, **kw)


def gen_pic(S, rng, pct, cuts_of_row, **kw):
    """cuts_of_row(y) -> (cuts, gen_row keywords)"""
    rows = []
    for y in range(S.mbh):
        cuts, rk = cuts_of_row(y)
        rows.append(gen_row(S, rng, pct, y, cuts, **rk))
    return Pic(pct, rows, fpfd=0, **kw)


def _stream(name, width, height, cf, make, **skw):
    def build(form):
        S = SlStream(name, width, height, cf, form, **skw)
        rng = DS._rng(name)
        pics, trefs = make(S, rng)
        S.es = S.write(pics, trefs)
        if S.form == "ms" and S.nslices > 1024:
            S.ev("sl:more_slices_than_1024")
        return S
    build.__name__ = name
    return build


EXT = (1, [0x5A, 0x81])


def _small(S, rng):
    """64 x 48 (4 x 3 macroblocks), I P B: row 0 [1, 3], row 1 [3, 1], row 2 halves in the I picture;
    the P and B pictures rotate the splits, and one row of each has a slice per macroblock"""
    w = S.mbw
    splits = [[1], [w - 1], [w // 2], list(range(1, w))]

    def rows(p):
        def of(y):
            xs = splits[(y + p) % 3] if not (p and y == 1) else splits[3]
            cuts = [Cut(x, qcode=(9 + 2 * y + x if (x + y + p) & 1 else None), ext=(EXT if x == xs[0] and y == 2 else None),
                        zero_bytes=(y + x) % 3 if y else 0) for x in xs]
            return cuts, dict(qcode=5 + y, field_at=xs[0] if y == 2 else None)
        return of
    return [gen_pic(S, rng, 1, rows(0)), gen_pic(S, rng, 2, rows(1)), gen_pic(S, rng, 3, rows(2))], [0, 2, 1]


def _qcif(S, rng):
    """176 x 144 (11 x 9), I P B B: every split kind in every picture type, rows without a cut between"""
    w = S.mbw
    kinds = [[1], [w - 1], [w // 2], list(range(1, w)), [], [2, 3, 7], [w // 2], [4, 8], [1, w - 1]]

    def rows(p):
        def of(y):
            xs = kinds[(y + 2 * p) % len(kinds)]
            cuts = [Cut(x, qcode=(3 + (5 * x + y + p) % 28 if (x + p) & 1 else None), zero_bytes=(x + y) % 4 == 0) for x in xs]
            return cuts, dict(qcode=4 + y, field_at=xs[0] if xs and y & 1 else None)
        return of
    return ([gen_pic(S, rng, 1, rows(0)), gen_pic(S, rng, 2, rows(1)), gen_pic(S, rng, 3, rows(2)),
             gen_pic(S, rng, 3, rows(3))], [0, 3, 1, 2])


def _w560(S, rng):
    """560 x 16 (35 macroblocks): slices at columns 32, 33, 34: increments 33 (the longest code), 34 and
    35 (one escape), in I, P and B"""
    def of(y):
        return [Cut(32), Cut(33, qcode=17), Cut(34)], dict(qcode=6)
    return [gen_pic(S, rng, 1, of), gen_pic(S, rng, 2, of), gen_pic(S, rng, 3, of)], [0, 2, 1]


def _w16384(S, rng):
    """16384 x 16 (1024 macroblocks): slices at columns 66 (two escapes) and 1023 (31 escapes)"""
    def of(y):
        return [Cut(66, qcode=11), Cut(1023)], dict(qcode=7)
    return [gen_pic(S, rng, 1, of), gen_pic(S, rng, 2, of)], [0, 1]


def _tall(S, rng):
    """32 x 2816 (2 x 176): slice_vertical_position_extension in every slice, a cut in every other row"""
    def of(y):
        return ([Cut(1, qcode=(8 + y % 9 if y % 3 == 0 else None))] if y % 2 == 0 or y > 170 else []), dict(qcode=3 + y % 5)
    return [gen_pic(S, rng, 1, of), gen_pic(S, rng, 2, of)], [0, 1]


def _many(S, rng):
    """176 x 144, eleven pictures (I and ten P) with a slice per macroblock: 1,089 slices"""
    def of(y):
        return list(range(1, S.mbw)), dict(qcode=5 + y, skips=False)
    return [gen_pic(S, rng, 1 if k == 0 else 2, of) for k in range(11)], list(range(11))


BUILDERS = [
    _stream("sl_420", 64, 48, 1, _small), _stream("sl_422", 64, 48, 2, _small), _stream("sl_444", 64, 48, 3, _small),
    _stream("sl_qcif", 176, 144, 1, _qcif), _stream("sl_560", 560, 16, 1, _w560),
    _stream("sl_16384", 16384, 16, 1, _w16384, hsize=16383), _stream("sl_tall", 32, 2816, 1, _tall),
    _stream("sl_11x11", 176, 144, 1, _many),
]
MANY = "sl_11x11"

# what the flag-clear library says to an ms stream: its first slice ends short of the row's end, or
# (where that slice is a row of its own in front of the first cut row) the second slice of a row
CLEAR_STATUS = -2
CLEAR_REASONS = ("slice does not cover the whole macroblock row", "two slices in one macroblock row")


def build_all():
    """[(ms, ref)] of every twin stream, in a fixed order"""
    return [(b("ms"), b("ref")) for b in BUILDERS]


# ---- negative streams: explicit slices (row, start column, macroblocks, quantiser code) ------------------
GAP, OVERLAP = "slices of a macroblock row leave a gap", "slices of a macroblock row overlap or are out of order"
TWO, BEYOND = "two slices in one macroblock row", "macroblock beyond the end of the row"


def _neg(name, slices_of):
    """a 64 x 32 I picture (4 x 2) whose slices are slices_of(row 0's macroblocks, row 1's)"""
    def build():
        S = SlStream(name, 64, 32, 1, "ms")
        S._negative = True
        rng = DS._rng(name)
        r = [[intra_mb(S, rng) for _ in range(4)] for _ in range(2)]
        P = Pic(1, [Row(r[0]), Row(r[1])], fpfd=0)
        P.slices = slices_of(r[0], r[1])
        S.es = S.write([P])
        return S
    build.__name__ = name
    return build


# (builder, status, reason, index of the blamed slice in stream order)
NEGATIVE = [
    (_neg("neg_gap_start", lambda a, b: [(0, 1, a[1:], 8), (1, 0, b, 8)]), -2, GAP, 0),
    (_neg("neg_gap_middle", lambda a, b: [(0, 0, a[:1], 8), (0, 2, a[2:], 8), (1, 0, b, 8)]), -2, GAP, 1),
    (_neg("neg_gap_end", lambda a, b: [(0, 0, a, 8), (1, 0, b[:2], 8), (1, 2, b[2:3], 8)]), -2, GAP, 2),
    (_neg("neg_overlap", lambda a, b: [(0, 0, a[:2], 8), (0, 1, a[1:], 8), (1, 0, b, 8)]), -2, OVERLAP, 1),
    (_neg("neg_runs_past", lambda a, b: [(0, 0, a, 8), (1, 0, b[:3], 8), (1, 2, b[2:], 8)]), -2, OVERLAP, 2),
    (_neg("neg_wrong_order", lambda a, b: [(0, 2, a[2:], 8), (0, 0, a[:2], 8), (1, 0, b, 8)]), -2, GAP, 0),
    (_neg("neg_repeat_later", lambda a, b: [(0, 0, a[:2], 8), (1, 0, b, 8), (0, 2, a[2:], 8)]), -2, TWO, 2),
    (_neg("neg_x0_beyond", lambda a, b: [(0, 0, a, 8), (1, 0, b[:2], 8), (1, 4, b[2:], 8)]), -6, BEYOND, 2),
]


def load_manifest():
    with open(os.path.join(GOLDEN, "manifest.json")) as f:
        return json.load(f)


def read(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


# ---- damaged ms streams for the concealment tests (CPU and GPU) ---------------------------------------
def slice_table(es):
    """[(picture, row, start, end)] of the slices in stream order, found without the library"""
    import conceal_streams as CS
    return CS.slice_table(es)


def failing_substitution(es, w, h, cf, j):
    """conceal_streams.failing_substitution under the flag: the first single-byte substitution in the
    payload of slice j that keeps the scan's pictures and slices and makes exactly that slice fail
    its parse in the twin.  Returns (position, value, reason text)."""
    import conceal_streams as CS
    import parse_mutants as PM
    from tiny_mp2v_dec_amd import _lib
    from tiny_mp2v_dec_amd.records import Scan
    pic, _, lo, hi = slice_table(es)[j]
    with Scan(es, w, h, cf, slices=True) as sc:
        n, ns = sc.npics, sc.nslices
    for pos in range(lo + 4, hi):
        for val in range(256):
            if val == es[pos]:
                continue
            b = PM.mutate(es, pos, val)
            try:
                s2 = Scan(b, w, h, cf, slices=True)
            except _lib.Mp2vgError:
                continue
            with s2:
                if s2.npics != n or s2.nslices != ns:
                    continue
                try:
                    s2.parse_host(pic, 1)
                except _lib.Mp2vgError as e:
                    if PM.blamed_picture(str(e)) == (pic, lo) and CS.slice_level(str(e)):
                        return pos, val, PM.detail(str(e)).split(": ", 1)[1]
    raise AssertionError(f"no single-byte substitution makes slice {j} fail")


# rows of sl_qcif that hold three slices ([1, mbw - 1]): (picture, row) in the I, the P and a B picture
CONCEAL_STREAM = "sl_qcif"
THREE_SLICE_ROWS = {"I": (0, 8), "P": (1, 6), "B": (2, 4)}


def conceal_cases(es, w, h, cf):
    """[(name, bytes, damaged rows, missing rows, expected damage)] on the ms form of CONCEAL_STREAM;
    expected damage = [(picture, row, status or None, reason text, byte offset)] as the library reports
    it: the blamed slice's status, reason and offset (a missing row: the picture's start code)."""
    table = slice_table(es)
    out = []
    for t, (p, y) in THREE_SLICE_ROWS.items():
        js = [j for j, s in enumerate(table) if s[:2] == (p, y)]
        assert len(js) == 3, (t, js)
        pos, val, why = failing_substitution(es, w, h, cf, js[1])
        bad = es[:pos] + bytes([val]) + es[pos + 1:]
        out.append((f"damaged_{t}", bad, [(p, y)], [], [(p, y, None, why, table[js[1]][2])]))
    p, y = THREE_SLICE_ROWS["P"]
    js = [j for j, s in enumerate(table) if s[:2] == (p, y)]
    cut = es[:table[js[1]][2]] + es[table[js[1]][3]:]
    out.append(("middle_deleted", cut, [(p, y)], [], [(p, y, -2, GAP, table[js[1]][2])]))  # (the third slice moved up)
    p, y = THREE_SLICE_ROWS["B"]
    js = [j for j, s in enumerate(table) if s[:2] == (p, y)]
    cut = es[:table[js[0]][2]] + es[table[js[2]][3]:]
    pic_start = [m for m in range(len(es) - 3) if es[m:m + 4] == b"\x00\x00\x01\x00"][p]
    out.append(("row_deleted", cut, [], [(p, y)],
                [(p, y, -2, "picture with a macroblock row not covered by any slice", pic_start)]))
    return out
