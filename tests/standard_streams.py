"""Twin streams for MP2VG_PARSE_STANDARD from the independent writer of tests/directed_syntax.py.

The compiled reference cannot decode a stream in the standard's ordinary form (matrices in the
sequence header or none at all, partial quant_matrix_extensions, intra_vlc_format = 0), but it
decodes its twin.  So every picture model here is written twice:

  S'  ("std")  the standard form: sequence-header matrices, partial or no extensions, the
               picture's own intra_vlc_format;
  S   ("ref")  the reference's subset: intra_vlc_format = 1 and a full quant_matrix_extension on
               every picture that carries the four EFFECTIVE matrices of that picture.

The effective matrices come from this module's own statement of 13818-2 6.3.3 / 6.3.11
(MatrixState), never from the library.  Both forms give one set of expected records (the slice
model of directed_syntax.Stream), so S' under the flag must give the records, words and W that S
gives without it, and its frames carry the MD5s the reference computed for S
(tests/golden/make_standard_fixtures.py -> tests/golden/standard/).

directed_syntax.py fixes intra_vlc_format = 1 (picture_headers, and the `tab` of macroblock) and
a full extension per picture; StdStream overrides those methods and leaves that file alone.
"""
import contextlib
import json
import os

import directed_syntax as DS
from directed_syntax import BWD, FWD, INTRA, PAT, Block, MB, Pic, Row, fr, tex_mb

GOLDEN = os.path.join(DS.GOLDEN, "standard")

# ---- the matrix rule (13818-2 6.3.3, 6.3.11), stated here on its own -------------------------------
# the default intra matrix as 6.3.11 prints it: raster order, row by row
DEFAULT_INTRA_RASTER = [
    8, 16, 19, 22, 26, 27, 29, 34,
    16, 16, 22, 24, 27, 29, 34, 37,
    19, 22, 26, 27, 29, 34, 34, 38,
    22, 22, 26, 27, 29, 34, 37, 40,
    22, 26, 27, 29, 32, 35, 40, 48,
    26, 27, 29, 32, 35, 40, 48, 58,
    26, 27, 29, 34, 38, 46, 56, 69,
    27, 29, 35, 38, 46, 56, 69, 83]


def zigzag():
    """raster index 8 v + u of each zigzag position (figure 7-2): the anti-diagonals u + v = s in
    turn, downwards (v rising) for odd s and upwards for even s"""
    order = []
    for s in range(15):
        vs = [v for v in range(8) if 0 <= s - v < 8]
        for v in (vs if s & 1 else reversed(vs)):
            order.append(8 * v + (s - v))
    return order


ZIGZAG = zigzag()
assert ZIGZAG[:10] == [0, 1, 8, 16, 9, 2, 3, 10, 17, 24] and sorted(ZIGZAG) == list(range(64))
# matrices travel in zigzag order, so that is the order of everything below
DEFAULT_INTRA = [DEFAULT_INTRA_RASTER[r] for r in ZIGZAG]
DEFAULT_NON_INTRA = [16] * 64
assert DEFAULT_INTRA != DEFAULT_INTRA_RASTER  # (the matrix is not symmetric: a missing conversion shows)


class MatrixState:
    """[intra, non_intra, chroma_intra, chroma_non_intra], in coding order"""

    def __init__(self):
        self.sequence_header(None, None)

    def sequence_header(self, intra, non_intra):
        """loaded matrices or None: what is not loaded returns to its default"""
        a = list(intra) if intra else list(DEFAULT_INTRA)
        b = list(non_intra) if non_intra else list(DEFAULT_NON_INTRA)
        self.m = [a, b, list(a), list(b)]

    def extension(self, loads):
        """{0..3: matrix}, in the extension's field order: a luma load replaces its chroma matrix too"""
        for k in sorted(loads):
            self.m[k] = list(loads[k])
            if k < 2:
                self.m[k + 2] = list(loads[k])

    def effective(self):
        return [list(k) for k in self.m]


def w_of(mats, alt):
    """a picture record's W: matrix entry of each position of the picture's own scan
    (include/mp2vg.h: 'quantiser matrices in scan order')"""
    alt_scan = [0, 8, 16, 24, 1, 9, 2, 10, 17, 25, 32, 40, 48, 56, 57, 49, 41, 33, 26, 18, 3, 11, 4, 12, 19, 27, 34,
                42, 50, 58, 35, 43, 51, 59, 20, 28, 5, 13, 6, 14, 21, 29, 36, 44, 52, 60, 37, 45, 53, 61, 22, 30, 7,
                15, 23, 31, 38, 46, 54, 62, 39, 47, 55, 63]  # figure 7-3, raster index per scan position
    scan = alt_scan if alt else ZIGZAG
    zz_of_raster = {r: i for i, r in enumerate(ZIGZAG)}
    return [[m[zz_of_raster[scan[i]]] for i in range(64)] for m in mats]


# ---- events ------------------------------------------------------------------------------------------
MATRIX_CASES = ["none", "seq_intra", "seq_non_intra", "seq_both", "partial_ext_pic0", "partial_ext_later_ibbp",
                "second_seq_resets", "second_seq_loads", "alt_scan_defaults", "422_intra_copied", "422_chroma_equal"]
B14_PAIRS = sorted(DS.COEF[0])


def _required():
    ev = [f"std:matrices:{c}" for c in MATRIX_CASES]
    ev += [f"std:ivf0:{t}:{cf}" for t in "IPB" for cf in (420, 422)]
    ev += [f"std:b14_intra:{r}:{lv}" for r, lv in B14_PAIRS]
    ev += ["std:dc_only", "std:first_ac_11s:pos", "std:first_ac_11s:neg", "std:block_of_64"]
    ev += [f"std:escape:run0:{lv}" for lv in (1, -1, 2047, -2047)]    # in intra blocks (their largest run is 62)
    ev += [f"std:escape:run63:{lv}" for lv in (1, -1, 2047, -2047)]   # in non-intra blocks of format-0 pictures
    ev += [f"std:intra_after_nonintra:{t}" for t in "PB"] + [f"std:intra_after_skip:{t}" for t in "PB"]
    ev += ["std:formats_alternate"]
    return ev


REQUIRED_EVENTS = _required()
_REQUIRED = set(REQUIRED_EVENTS)


@contextlib.contextmanager
def _intra_blocks_in_b14():
    """directed_syntax.Stream.macroblock picks table 1 (B.15 and its end of block) for an intra
    macroblock; while an intra macroblock of a format-0 picture is written, table 1 IS B.14"""
    coef1, eob1 = DS.COEF[1], DS.EOB[1]
    DS.COEF[1], DS.EOB[1] = DS.COEF[0], DS.EOB[0]
    try:
        yield
    finally:
        DS.COEF[1], DS.EOB[1] = coef1, eob1


class SPic(Pic):
    """A picture of the model.  ivf = intra_vlc_format; ext = None or {0..3: matrix}, its (partial)
    quant_matrix_extension; seq = None or (intra or None, non_intra or None): a sequence header in
    front of it with these loads (picture 0 always has one; default: no loads)."""

    def __init__(self, pct, rows, ivf=1, ext=None, seq=None, **kw):
        Pic.__init__(self, pct, rows, **kw)
        self.ivf, self.ext, self.seq = ivf, ext, seq


class StdStream(DS.Stream):
    """form "std": S'; form "ref": its twin S.  full_ext=True (std only) writes the effective
    matrices as a full extension on every picture and keeps the rest of the standard form: the
    stream on which only intra_vlc_format = 0 stands between it and the flag-clear parser."""

    def __init__(self, name, width, height, cf, form, full_ext=False):
        DS.Stream.__init__(self, name, width, height, cf)
        assert form in ("std", "ref")
        self.form, self.full_ext = form, full_ext
        self.state = MatrixState()
        self.effective = []  # per picture: its four matrices (zigzag order)
        self.W = []          # per picture: the expected W
        self._loads = (None, None)

    def ev(self, name):
        if name.startswith("std:"):
            assert name in _REQUIRED, name
            self.events.add(name)
        else:
            DS.Stream.ev(self, name)

    # ---- headers -----------------------------------------------------------------------------------
    def sequence(self):
        if self.form == "ref":
            return DS.Stream.sequence(self)
        b = self.bw
        b.start_code(0xB3)
        b.put(self.hsize & 0xFFF, 12), b.put(self.vsize & 0xFFF, 12), b.put(1, 4), b.put(3, 4), b.put(0x3FFFF, 18)
        b.put(1, 1), b.put(0x3FF, 10), b.put(0, 1)
        for m in self._loads:  # load_intra_quantiser_matrix, load_non_intra_quantiser_matrix
            b.put(1 if m else 0, 1)
            for v in m or ():
                b.put(v, 8)
        b.start_code(0xB5)
        b.put(1, 4), b.put(0x44, 8), b.put(0, 1), b.put(self.cf, 2), b.put(self.hsize >> 12, 2), b.put(self.vsize >> 12, 2)
        b.put(0, 12), b.put(1, 1), b.put(0, 8), b.put(0, 1), b.put(0, 2), b.put(0, 5)
        b.start_code(0xB8)
        b.put(0, 25), b.put(1, 1), b.put(0, 1)

    def write(self, pics, trefs=None):
        self._loads = pics[0].seq or (None, None)
        return DS.Stream.write(self, pics, trefs)

    def picture_headers(self, P, tref):
        first = self.npics == 0
        if first or P.seq is not None:
            self._loads = P.seq or (None, None)
            self.state.sequence_header(*self._loads)
            if not first and self.form == "std":
                self.sequence()  # (the twin needs none: its pictures carry their matrices themselves)
        if P.ext:
            self.state.extension(P.ext)
        P.mats = self.state.effective()
        self.effective.append(P.mats)
        self.W.append(w_of(P.mats, P.alt))
        if self.form == "ref":
            return DS.Stream.picture_headers(self, P, tref)  # intra_vlc_format 1, the four matrices
        b = self.bw
        b.start_code(0x00)
        b.put(tref, 10), b.put(P.pct, 3), b.put(0xFFFF, 16)
        if P.pct in (2, 3):
            b.put(0, 1), b.put(7, 3)
        if P.pct == 3:
            b.put(0, 1), b.put(7, 3)
        b.put(0, 1)
        b.start_code(0xB5)
        b.put(8, 4)
        for s in range(2):
            for t in range(2):
                b.put(P.fcode[s][t], 4)
        b.put(P.prec, 2), b.put(3, 2), b.put(1, 1), b.put(P.fpfd, 1), b.put(P.cmv, 1), b.put(P.qst, 1)
        b.put(P.ivf, 1), b.put(P.alt, 1), b.put(0, 1), b.put(P.fpfd, 1), b.put(P.fpfd, 1), b.put(0, 1)
        ext = dict(enumerate(P.mats)) if self.full_ext else P.ext
        if ext:
            b.start_code(0xB5)
            b.put(3, 4)
            for k in range(4):
                b.put(1 if k in ext else 0, 1)
                for v in ext.get(k, ()):
                    b.put(v, 8)
        if P.ivf == 0:
            self.ev(f"std:ivf0:{'IPB'[P.pct - 1]}:{420 if self.cf == 1 else 422}")

    # ---- macroblocks ---------------------------------------------------------------------------------
    def macroblock(self, mb, x):
        P = self.P
        if self.form == "ref" or P.ivf:
            return DS.Stream.macroblock(self, mb, x)
        if not mb.t & INTRA:
            for B in mb.blocks.values():
                for c in B.coefs:
                    run, level = c[0], c[1]
                    if run == 63 and level in (1, -1, 2047, -2047):
                        self.ev(f"std:escape:run63:{level}")
            return DS.Stream.macroblock(self, mb, x)
        t = "IPB"[P.pct - 1]
        if P.pct > 1:
            if mb.skip:
                self.ev(f"std:intra_after_skip:{t}")
            elif self.prev is not None and not self.prev.t & INTRA:
                self.ev(f"std:intra_after_nonintra:{t}")
        for blk in range(self.nblocks):
            B = mb.blocks.get(blk) or Block()
            if not B.coefs:
                self.ev("std:dc_only")
            for k, c in enumerate(B.coefs):
                run, level, esc = (tuple(c) + (False,))[:3]
                if not esc and (run, abs(level)) in DS.COEF[0]:
                    self.ev(f"std:b14_intra:{run}:{abs(level)}")
                    if k == 0 and run == 0 and abs(level) == 1:
                        self.ev("std:first_ac_11s:" + ("neg" if level < 0 else "pos"))
                elif run == 0 and level in (1, -1, 2047, -2047):
                    self.ev(f"std:escape:run0:{level}")
            if len(B.coefs) == 63:
                self.ev("std:block_of_64")
        with _intra_blocks_in_b14():
            return DS.Stream.macroblock(self, mb, x)


# ---- picture content -----------------------------------------------------------------------------------
def rising(k):
    """a matrix whose 64 entries all differ (no two positions can change places unseen), one per k"""
    return [17 + 5 * k + 3 * i if i else 8 + k for i in range(64)]  # 8.. at DC, 20 .. 221 after it


def _big(rng, n=5):
    return DS._ac(rng, n, big=9)


def intra_mb(S, rng, **kw):
    m = tex_mb(S, rng, nac=0, **kw)
    for b in m.blocks.values():
        b.coefs = _big(rng)
    return m


def inter_mb(S, rng, t=PAT, **kw):
    return MB(t, cbp=(1 << S.nblocks) - 1, blocks={b: Block(_big(rng)) for b in range(S.nblocks)}, **kw)


def i_rows(S, rng):
    return [Row([intra_mb(S, rng) for _ in range(S.mbw)], qcode=5 + y) for y in range(S.mbh)]


def p_rows(S, rng):
    """each row: non-intra, intra after it, a skipped macroblock, intra after the skip"""
    rows = []
    for y in range(S.mbh):
        mbs = [inter_mb(S, rng, FWD | PAT, mv={0: fr(1, 1 if y == 0 else -1)}), intra_mb(S, rng)]
        mbs += [inter_mb(S, rng) for _ in range(S.mbw - 4)]
        mbs += [intra_mb(S, rng, skip=1)] if S.mbw >= 4 else []
        rows.append(Row(mbs, qcode=4 + y))
    return rows


def b_rows(S, rng):
    """even rows: forward, a skipped macroblock that repeats it, intra after the skip, ...,
    bidirectional with a pattern; odd rows: backward with a pattern, intra after it, forward, ..."""
    rows = []
    for y in range(S.mbh):
        vy = 1 if y == 0 else -1
        last = inter_mb(S, rng, FWD | BWD | PAT, mv={0: fr(-1, vy), 1: fr(-2, vy)})
        if S.mbw >= 4 and not y & 1:
            mbs = [MB(FWD, mv={0: fr(1, vy)}), intra_mb(S, rng, skip=1)]
            mbs += [inter_mb(S, rng, BWD | PAT, mv={1: fr(-1, vy)}) for _ in range(S.mbw - 4)] + [last]
        elif S.mbw >= 4:
            mbs = [inter_mb(S, rng, BWD | PAT, mv={1: fr(1, vy)}), intra_mb(S, rng), MB(FWD, mv={0: fr(1, vy)})]
            mbs += [inter_mb(S, rng, BWD | PAT, mv={1: fr(-1, vy)}) for _ in range(S.mbw - 4)] + [last]
        else:  # two macroblocks: non-intra then intra, and the other way round
            mbs = [inter_mb(S, rng, FWD | BWD | PAT, mv={0: fr(1, vy), 1: fr(0, vy)}), intra_mb(S, rng)]
            if y & 1:
                mbs = [intra_mb(S, rng), inter_mb(S, rng, BWD | PAT, mv={1: fr(-1, vy)})]
        rows.append(Row(mbs, qcode=6 + y))
    return rows


ROWS = {1: i_rows, 2: p_rows, 3: b_rows}


def pic(S, rng, pct, **kw):
    return SPic(pct, ROWS[pct](S, rng), **kw)


def ipbb(S, rng, per_pic=None, gops=1):
    """I B B P in display order, coded I P B B; per_pic = {coding index: SPic keywords}"""
    pics, trefs = [], []
    for g in range(gops):
        for k, (pct, tref) in enumerate(((1, 0), (2, 3), (3, 1), (3, 2))):
            pics.append(pic(S, rng, pct, **(per_pic or {}).get(4 * g + k, {})))
            trefs.append(4 * g + tref)
    return pics, trefs


# ---- the streams: builders take the form and return a finished StdStream -----------------------------
def _matrix_stream(name, case, cf, make):
    def build(form, **kw):
        S = StdStream(name, 64, 48, cf, form, **kw)
        rng = DS._rng(name)
        pics, trefs = make(S, rng)
        S.es = S.write(pics, trefs)
        S.ev(f"std:matrices:{case}")
        return S
    build.__name__ = name
    return build


def _m_none(S, rng):
    return ipbb(S, rng)


def _m_seq(intra, non_intra):
    return lambda S, rng: ipbb(S, rng, {0: dict(seq=(rising(0) if intra else None, rising(1) if non_intra else None))})


def _m_partial0(S, rng):       # picture 0 loads non_intra and chroma_intra only
    return ipbb(S, rng, {0: dict(ext={1: rising(2), 2: rising(3)})})


def _m_partial_later(S, rng):  # the P picture, coded second and shown last: both B pictures inherit it
    return ipbb(S, rng, {1: dict(ext={0: rising(1), 3: rising(2)})})


def _m_second_seq_resets(S, rng):
    return ipbb(S, rng, {0: dict(seq=(rising(0), None)), 1: dict(ext={1: rising(3), 2: rising(1)}), 4: dict(seq=(None, None))},
                gops=2)


def _m_second_seq_loads(S, rng):
    return ipbb(S, rng, {1: dict(ext={0: rising(2)}), 4: dict(seq=(rising(3), rising(0)))}, gops=2)


def _m_alt(S, rng):
    return ipbb(S, rng, {k: dict(alt=1) for k in range(4)})


def _m_422_intra(S, rng):
    return ipbb(S, rng, {0: dict(seq=(rising(1), None))})


def _m_422_equal(S, rng):      # chroma loads equal to the luma ones: on picture 0, and again on the P picture
    return ipbb(S, rng, {0: dict(ext={0: rising(0), 1: rising(2), 2: rising(0), 3: rising(2)}),
                         1: dict(ext={2: rising(0), 3: rising(2)})})


MATRIX_BUILDERS = [
    _matrix_stream("mat_none", "none", 1, _m_none),
    _matrix_stream("mat_seq_intra", "seq_intra", 1, _m_seq(True, False)),
    _matrix_stream("mat_seq_non_intra", "seq_non_intra", 1, _m_seq(False, True)),
    _matrix_stream("mat_seq_both", "seq_both", 1, _m_seq(True, True)),
    _matrix_stream("mat_partial_ext_pic0", "partial_ext_pic0", 1, _m_partial0),
    _matrix_stream("mat_partial_ext_later", "partial_ext_later_ibbp", 1, _m_partial_later),
    _matrix_stream("mat_second_seq_resets", "second_seq_resets", 1, _m_second_seq_resets),
    _matrix_stream("mat_second_seq_loads", "second_seq_loads", 1, _m_second_seq_loads),
    _matrix_stream("mat_alt_scan", "alt_scan_defaults", 1, _m_alt),
    _matrix_stream("mat_422_intra_copied", "422_intra_copied", 2, _m_422_intra),
    _matrix_stream("mat_422_chroma_equal", "422_chroma_equal", 2, _m_422_equal),
]


def refused_422(form="std", **kw):
    """4:2:2 with a chroma_intra load that differs from intra, on the P picture (coding index 1):
    refused at the picture level under the flag.  No twin."""
    S = StdStream("neg_422_chroma_differs", 64, 48, 2, form, **kw)
    rng = DS._rng(S.name)
    pics, trefs = ipbb(S, rng, {1: dict(ext={2: rising(3)})})
    S.es = S.write(pics, trefs)
    return S


REFUSED_422_PICTURE = 1
REFUSED_422_REASON = "picture 1: chroma quantiser matrices differ from the luma ones in 4:2:2"


# ---- intra_vlc_format = 0 ---------------------------------------------------------------------------
def b14_blocks():
    """intra blocks (coefficient lists) that together hold every (run, level) of B.14 once, signs
    alternating, packed in table order into as few blocks as the 63 AC positions allow"""
    blocks, cur, pos = [], [], 1
    for k, (run, level) in enumerate(B14_PAIRS):
        if pos + run > 63:
            blocks.append(cur)
            cur, pos = [], 1
        cur.append((run, level if k & 1 else -level))
        pos += run + 1
    blocks.append(cur)
    return blocks


def _special_intra_blocks():
    return [
        [],                                                   # DC only: '10' straight after the DC
        [(0, 1), (0, -1), (3, 2)],                            # '11s' as the first AC coefficient
        [(0, -1), (1, 1)],
        [(0, 1, True), (0, -1, True), (0, 2047), (0, -2047)],  # escapes at run 0
        [(0, 1 + (i % 2)) for i in range(63)],                # 64 words
        [(62, -3)],                                           # the longest run an intra block holds
    ]


def format0(cf):
    """I, P and B pictures with intra_vlc_format = 0 (I P B B, coded order), 64 x 48"""
    name = f"ivf0_{420 if cf == 1 else 422}"

    def build(form, **kw):
        S = StdStream(name, 64, 48, cf, form, **kw)
        rng = DS._rng(name)
        pics, trefs = ipbb(S, rng, {k: dict(ivf=0) for k in range(4)})
        lists = b14_blocks() + _special_intra_blocks()
        # the I picture's intra blocks take the lists in turn; the P and B pictures' intra macroblocks
        # take them again from the other end, so each list stands in an I and in a P or B picture
        for P, order in ((pics[0], lists), (pics[1], lists[::-1]), (pics[2], lists[::2]), (pics[3], lists[1::2])):
            slots = [b for row in P.rows for m in row.mbs if m.t & INTRA for _, b in sorted(m.blocks.items())]
            assert len(slots) >= len(order) or P is not pics[0], (name, len(slots), len(order))
            for b, coefs in zip(slots, order):
                b.coefs = list(coefs)
        # escapes at run 63 live in non-intra blocks (an intra block's runs end at 62)
        m = pics[1].rows[0].mbs[0]
        for b, lv in enumerate((1, -1, 2047, -2047)):
            m.blocks[b].coefs = [(63, lv)]
        S.es = S.write(pics, trefs)
        return S
    build.__name__ = name
    return build


def alternating(form, **kw):
    """32 x 32, 40 pictures (ten I P B B groups) whose intra_vlc_format alternates 0, 1, 0, 1 in coding
    order: 80 slices, so the device parse's first wave mixes both tables and a second is partly
    filled.  A partial extension on picture 3, a second sequence header (no loads) at picture 20."""
    S = StdStream("ivf_alternating", 32, 32, 1, form, **kw)
    rng = DS._rng(S.name)
    per = {k: dict(ivf=k & 1) for k in range(40)}
    per[3].update(ext={0: rising(2), 3: rising(1)})
    per[20].update(seq=(None, None))
    pics, trefs = ipbb(S, rng, per, gops=10)
    S.es = S.write(pics, trefs)
    S.ev("std:formats_alternate")
    return S


FORMAT0_BUILDERS = [format0(1), format0(2), alternating]
BUILDERS = MATRIX_BUILDERS + FORMAT0_BUILDERS

# what the flag-clear library says to every S' (its first picture has no full extension)
CLEAR_STATUS, CLEAR_REASON = -2, "picture without a full quant_matrix_extension"
# ... and to an S' that carries full extensions: its first intra macroblock of a format-0 picture
CLEAR_IVF0_REASON = "intra macroblock with intra_vlc_format=0"


def build_all():
    """[(S', S)] of every twin stream, in a fixed order"""
    return [(b("std"), b("ref")) for b in BUILDERS]


def load_manifest():
    with open(os.path.join(GOLDEN, "manifest.json")) as f:
        return json.load(f)


def read(entry, form):
    with open(os.path.join(GOLDEN, entry[form]), "rb") as f:
        return f.read()
