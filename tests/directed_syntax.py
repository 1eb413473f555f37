"""Directed slice-syntax streams from a writer that shares nothing with the parsers.

A plain-Python bit writer and slice-state model, written from ISO/IEC 13818-2 6.2.4-6.2.6
(slice, macroblock, block syntax), 7.2 (variable length decoding) and 7.6.3 (motion vectors).
The code tables come from tests/golden/vlc_vectors.npz, which holds every table entry of the
compiled reference's own tables (bits, length, value); the four codes the fixture does not hold
(macroblock_escape, the two end-of-block codes, the coefficient escape) are written out by hand.
Nothing here calls the library: neither its stream writer nor its table decoder.

For every stream the model returns the bytes, the EXPECTED RECORDS (include/mp2vg.h: one 32-byte
record per macroblock and the coefficient words) and the set of SYNTAX EVENTS the stream holds.
tests/test_syntax_cpu.py compares host emitter and CPU twin with the expected records and the
union of the event logs with REQUIRED_EVENTS; tests/golden/make_syntax_fixtures.py pins the
decoded frames of every stream to the compiled reference.

The streams keep to the accepted contract (csrc/parse.cpp header comment): one slice per row from
column 0 with the last macroblock coded, MC reads inside the planes, no dual prime, no 4:4:4 field
DCT, intra_vlc_format 1, a full quant_matrix_extension per picture.

Where the reference decodes a construct differently from the standard, the model states the
reference's behaviour and says so at that line (search for "REFERENCE").
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# macroblock_type flags (6.3.17.1, tables B.2-B.4)
QUANT, FWD, BWD, PAT, INTRA = 0x20, 0x10, 0x08, 0x04, 0x02
# record flags and coefficient word flags (include/mp2vg.h)
R_INTRA, R_FWD, R_BWD, R_FIELD, R_DCTF = 1, 2, 4, 8, 16
W_FIRST1S, W_DC = 1 << 29, 1 << 30

# codes the fixture does not hold (B.1 macroblock_escape; B.14 / B.15 end of block; escape)
MB_ESCAPE = "00000001000"
EOB = {0: "10", 1: "0110"}
COEF_ESCAPE = "000001"


def _load_tables():
    v = np.load(os.path.join(GOLDEN, "vlc_vectors.npz"))
    out = {}
    for t, e, bits, val, aux, n in zip(v["table"], v["entry"], v["bits"], v["value"], v["aux"], v["code_len"]):
        out.setdefault(int(t), {}).setdefault(int(e), (format(int(bits), "064b")[:int(n)], int(val), int(aux)))
    return out


_T = _load_tables()
MBA = {val: code for code, val, _ in _T[10].values()}                    # increment 1..33 -> code
MBTYPE = {p: {val: code for code, val, _ in _T[p].values()} for p in (1, 2, 3)}  # flags -> code
CBP = {val: code for code, val, _ in _T[4].values()}                     # coded_block_pattern_420 -> code
MOTION = {val: code for code, val, _ in _T[5].values()}                  # signed motion_code -> code + sign
DCSIZE = [{val: code for code, val, _ in _T[6].values()}, {val: code for code, val, _ in _T[7].values()}]
COEF = [{(val, aux): code for code, val, aux in _T[8].values()},         # B.14: (run, level) -> code
        {(val, aux): code for code, val, aux in _T[9].values()}]         # B.15


def _required_events():
    ev = []
    ev += [f"fcode_slot:{s}{t}:{v}" for s in range(2) for t in range(2) for v in range(1, 10)]
    ev += ["fcode4:frame", "fcode4:field"]
    # the f_codes whose wrap fits (wrap_pictures): a wrap above `high` needs two vectors 16 f + 1
    # half samples apart, one below `low` two vectors 16 f apart with the lower one in an earlier
    # column; the pair of a vertical wrap stands in one row
    ev += [f"wrap_high:h:{fc}" for fc in range(1, 9)] + [f"wrap_low:h:{fc}" for fc in range(1, 8)]  # <= 1040x16
    ev += [f"wrap_high:v:{fc}" for fc in range(1, 5)] + [f"wrap_low:v:{fc}" for fc in range(1, 6)]  # <= 176x144
    ev += ["delta0_fcode_gt1", "field_vert_pred:odd_neg", "field_vert_pred:odd_pos"]
    ev += [f"seq:{k}:{d}" for k in ("frame_field_frame", "field_field_fs") for d in ("fwd", "bwd")]
    ev += [f"pmv_reset:{k}" for k in ("intra_P", "intra_B", "pattern_only_P", "slice_start")]
    ev += [f"pmv_copy:{k}" for k in ("fwd", "bwd", "bi")]
    ev += ["skip_P:after_nonzero_pmv", "skip_P:after_field"]
    ev += [f"skip_B:after_{k}" for k in ("fwd", "bwd", "bi", "field")]
    ev += [f"skip_run:{n}" for n in (1, 32, 33, 34, 67)]
    ev += ["skip_ends_at_mbw-2", "dc_reset:skip", "qscale_across_skip"]
    ev += [f"mbtype:{p}:{f}" for p in (1, 2, 3) for f in sorted(MBTYPE[p])]
    ev += [f"qcode_{w}:{q}:{c}" for w in ("slice", "mb") for q in (0, 1) for c in range(1, 32)]
    ev += [f"dct_type:{d}:{k}" for d in (0, 1) for k in ("intra", "pattern")]
    ev += [f"cbp420:{v}" for v in range(1, 64)]
    ev += [f"cbp422:{k}:{e}" for k in ("zero", "nonzero") for e in range(4)]
    ev += ["cbp444:none", "cbp444:all"] + [f"cbp444:bit{i}" for i in range(6)]
    ev += ["dc:luma:0", "dc:chroma:0"]
    ev += [f"dc:{c}:{s}:{m}:{g}" for c in ("luma", "chroma") for s in range(1, 12) for m in ("min", "max")
           for g in ("neg", "pos")]
    ev += [f"dc_prec:{p}:{s}" for p in range(4) for s in range(0, 9 + p)]
    ev += ["dc_chains:422", "dc_chains:444", "dc_reset:slice_start", "dc_reset:after_nonintra",
           "intra_in:P", "intra_in:B"]
    ev += ["coef:first_1s", "coef:later_11s", "coef:block_of_one", "coef:run_ends_63", "coef:block_of_64"]
    ev += [f"escape:run{r}:{lv}" for r in (0, 63) for lv in (1, -1, 2047, -2047)]
    ev += ["b15:I", "b15:P", "b15:B", "b14_b15_neighbours:P", "b14_b15_neighbours:B"]
    ev += [f"piclevel:{a}:{q}:{p}" for a in (0, 1) for q in (0, 1) for p in range(4)]
    ev += [f"matrices4:{cf}" for cf in (1, 2, 3)]
    ev += [f"slice_ext:{i}:{n}" for i in (0, 1) for n in (0, 1, 3)]
    ev += [f"stuffing_bits:{n}" for n in range(8)] + [f"zero_bytes:{n}" for n in range(4)]
    ev += ["last_mb_byte_aligned"]
    # sizes above 4095 (6.2.2.3 horizontal_size_extension, vertical_size_extension) and slices below
    # row 127 (6.2.4 slice_vertical_position_extension)
    ev += [f"hsize_ext:{n}" for n in (1, 2, 3)] + [f"vsize_ext:{n}" for n in (1, 2, 3)]
    ev += [f"vpos_ext:{n}" for n in range(8)]
    ev += ["wrap_high:h:9", "wrap_low:h:9"]  # these fit from 8192 wide on (wide_16384)
    return ev


# Left the list: concealment motion vectors in I pictures.  REFERENCE: parse_modes leaves
# motion_vector_count 0 for an intra macroblock (mb_decoder.cpp:364-367), so parse_motion_vectors
# takes the two-vector branch (:512-517) and reads two field selects and two vectors where the
# stream holds one vector: the parse derails, and the compiled reference crashed on the stream
# neg_cmv_in_i.  The construct is out of contract; both parsers reject it (NEGATIVE).


REQUIRED_EVENTS = _required_events()
_REQUIRED = set(REQUIRED_EVENTS)


def qscale_of(code, q_scale_type):
    """quantiser_scale (7.4.2.2, table 7-6)"""
    if not q_scale_type:
        return 2 * code
    nonlinear = [0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 18, 20, 22, 24, 28, 32, 36, 40, 44, 48, 52, 56, 64, 72,
                 80, 88, 96, 104, 112]
    return nonlinear[code]


class Bits:
    def __init__(self):
        self.s = []
        self.n = 0

    def put(self, value, n):
        if n:
            assert 0 <= value < (1 << n), (value, n)
            self.code(format(value, f"0{n}b"))

    def code(self, c):
        self.s.append(c)
        self.n += len(c)

    def align(self):
        k = -self.n % 8
        self.put(0, k)
        return k

    def start_code(self, code):
        self.align()
        self.put(0x00000100 | code, 32)

    def bytes(self):
        s = "".join(self.s)
        assert len(s) % 8 == 0
        return int(s, 2).to_bytes(len(s) // 8, "big") if s else b""


class Block:
    """One coded block: dc = the DC differential (intra), coefs = [(run, level)] or
    [(run, level, True)] to force the escape."""

    def __init__(self, coefs=(), dc=0, dc_abs=None):
        self.dc, self.dc_abs, self.coefs = dc, dc_abs, list(coefs)  # dc_abs: the predictor's value after it


class MB:
    """One coded macroblock.  skip = skipped macroblocks in front of it; t = macroblock_type flags;
    q = quantiser_scale_code (with QUANT); field = field motion vectors; dct = dct_type;
    mv = {s: [(field select, (x, y)), ...]} target vectors; cmv = concealment vector target (x, y);
    cbp = record-style pattern (bit b = block b); blocks = {b: Block} (absent ones are empty)."""

    def __init__(self, t, skip=0, q=None, field=False, dct=0, mv=None, cmv=None, cbp=0, blocks=None):
        self.t, self.skip, self.q, self.field, self.dct = t, skip, q, field, dct
        self.mv, self.cmv, self.cbp, self.blocks = mv or {}, cmv, cbp, blocks or {}


class Row:
    """One slice.  ext = None or (intra_slice, [extra_information_slice bytes]);
    zero_bytes = zero bytes after the slice, before the next start code."""

    def __init__(self, mbs, qcode=8, ext=None, zero_bytes=0):
        self.mbs, self.qcode, self.ext, self.zero_bytes = mbs, qcode, ext, zero_bytes


def flat_matrices():
    return [[16] * 64 for _ in range(4)]


class Pic:
    def __init__(self, pct, rows, fcode=None, prec=0, fpfd=1, cmv=0, qst=0, alt=0, mats=None):
        self.pct, self.rows, self.prec, self.fpfd, self.cmv, self.qst, self.alt = pct, rows, prec, fpfd, cmv, qst, alt
        if fcode is None:
            fcode = {1: ((15, 15), (15, 15)), 2: ((2, 2), (15, 15)), 3: ((2, 2), (2, 2))}[pct]
        self.fcode = fcode
        self.mats = mats or flat_matrices()


class Stream:
    """The writer and the slice-state model.  write(pics) gives the bytes; .mbs and .coefs are the
    expected records in decode order and .events the syntax events met."""

    def __init__(self, name, width, height, cf, hsize=None, vsize=None, vext=None):
        """width, height: the coded size.  hsize, vsize: horizontal_size and vertical_size as the
        headers carry them (14 bits; default the coded size), of which the coded size is the
        multiple of 16 above.  vext: slices carry slice_vertical_position_extension; the default
        is the standard's rule, vertical_size > 2800 (6.2.4)."""
        self.name, self.width, self.height, self.cf = name, width, height, cf
        self.hsize, self.vsize = hsize or width, vsize or height
        assert (self.hsize + 15) // 16 * 16 == width and (self.vsize + 15) // 16 * 16 == height
        self.vext = self.vsize > 2800 if vext is None else vext
        self._negative = False
        self.mbw, self.mbh = width // 16, height // 16
        self.nblocks = {1: 6, 2: 8, 3: 12}[cf]
        self.events = set()
        self.mbs = []    # dicts: x, y, flags, cbp, qscale, ncoef, coef_off, mv[2][2][2]
        self.coefs = []  # words
        self.npics = 0
        self.bw = Bits()
        self.stuffing = []  # stuffing bits after each slice
        self._row_end_pmv = False
        self._row_end_dc = False

    # ---- events --------------------------------------------------------------------------------
    def ev(self, name):
        assert name in _REQUIRED, name
        self.events.add(name)

    # ---- headers (6.2.2, 6.2.3) ----------------------------------------------------------------
    def sequence(self):
        b = self.bw
        b.start_code(0xB3)
        # horizontal_size_value, vertical_size_value: the 12 least significant bits (6.3.3)
        assert self.hsize & 0xFFF and self.vsize & 0xFFF  # (a value of 0 is forbidden)
        b.put(self.hsize & 0xFFF, 12), b.put(self.vsize & 0xFFF, 12), b.put(1, 4), b.put(3, 4), b.put(0x3FFFF, 18)
        b.put(1, 1), b.put(0x3FF, 10), b.put(0, 1), b.put(0, 1), b.put(0, 1)
        b.start_code(0xB5)
        # horizontal_size_extension, vertical_size_extension: the 2 most significant bits (6.3.5)
        b.put(1, 4), b.put(0x44, 8), b.put(0, 1), b.put(self.cf, 2), b.put(self.hsize >> 12, 2), b.put(self.vsize >> 12, 2)
        b.put(0, 12)
        if not self._negative:
            if self.hsize >> 12:
                self.ev(f"hsize_ext:{self.hsize >> 12}")
            if self.vsize >> 12:
                self.ev(f"vsize_ext:{self.vsize >> 12}")
        b.put(1, 1), b.put(0, 8), b.put(0, 1), b.put(0, 2), b.put(0, 5)
        b.start_code(0xB8)
        b.put(0, 25), b.put(1, 1), b.put(0, 1)

    def picture_headers(self, P, tref):
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
        b.put(1, 1), b.put(P.alt, 1), b.put(0, 1), b.put(P.fpfd, 1), b.put(P.fpfd, 1), b.put(0, 1)
        b.start_code(0xB5)
        b.put(3, 4)
        for m in P.mats:
            b.put(1, 1)
            for v in m:
                b.put(v, 8)

    # ---- the stream ----------------------------------------------------------------------------
    def write(self, pics, trefs=None):
        self.sequence()
        for i, P in enumerate(pics):
            assert len(P.rows) == self.mbh
            self.picture_headers(P, trefs[i] if trefs else i)
            self.ev(f"piclevel:{P.alt}:{P.qst}:{P.prec}")
            self._pic_stats = dict(intra=False, inter=False, chroma_intra=False, chroma_inter=False)
            for y, row in enumerate(P.rows):
                self.slice(P, y, row)
            self._matrices_event(P)
            self.npics += 1
        self.bw.start_code(0xB7)
        return self.bw.bytes()

    def _matrices_event(self, P):
        m = P.mats
        distinct = all(m[a] != m[b] for a in range(4) for b in range(a))
        # asymmetric in the position: all 64 entries differ, so no two positions can change places unseen
        asym = all(len(set(k)) == 64 for k in m)
        st = self._pic_stats
        if distinct and asym and st["intra"] and st["inter"] and st["chroma_intra"] and st["chroma_inter"]:
            self.ev(f"matrices4:{self.cf}")

    # ---- one slice (6.2.4) ---------------------------------------------------------------------
    def slice(self, P, y, row):
        b = self.bw
        if self.vext:  # mb_row = (slice_vertical_position_extension << 7) + slice_vertical_position - 1
            b.start_code((y & 127) + 1)
            b.put(y >> 7, 3)
            if not self._negative:
                self.ev(f"vpos_ext:{y >> 7}")
        else:
            assert y < 175
            b.start_code(y + 1)
        b.put(row.qcode, 5)
        self.ev(f"qcode_slice:{P.qst}:{row.qcode}")
        if row.ext is not None:
            intra_slice, info = row.ext
            b.put(1, 1), b.put(intra_slice, 1), b.put(0, 7)  # intra_slice_flag, intra_slice, reserved_bits
            for byte in info:
                b.put(1, 1), b.put(byte, 8)                  # extra_bit_slice, extra_information_slice
            self.ev(f"slice_ext:{intra_slice}:{len(info)}")
        b.put(0, 1)                                          # extra_bit_slice
        # slice state: predictors reset at the start of each slice (7.2.1, 7.6.3.4)
        self.P, self.y = P, y
        self.PMV = [[[0, 0], [0, 0]], [[0, 0], [0, 0]]]  # [r][s][t]
        self.dc_reset = 1 << (P.prec + 7)
        self.dc = [self.dc_reset] * 3
        self.q = qscale_of(row.qcode, P.qst)
        self.prev = None           # the previous coded macroblock (MB) of this slice
        self.hist = {0: [], 1: []}  # per direction: kinds of the vectors of consecutive macroblocks
        self.pending_reset = "slice_start" if (y > 0 and self._row_end_pmv) else None
        self.copy_pending = None
        if y > 0 and self._row_end_dc and row.mbs[0].t & INTRA:
            self.ev("dc_reset:slice_start")
        self.skipped_before = False
        self.q_from_mb = False
        self._dc_nonintra = False
        x = 0
        for mb in row.mbs:
            x = self.macroblock(mb, x)
        assert x == self.mbw or self._negative, (self.name, y, x)
        self._row_end_pmv = any(v for r in self.PMV for s in r for v in s)
        self._row_end_dc = any(d != self.dc_reset for d in self.dc)
        k = b.align()
        self.stuffing.append(k)
        self.ev(f"stuffing_bits:{k}")
        if k == 0:
            self.ev("last_mb_byte_aligned")
        b.put(0, 8 * row.zero_bytes)
        self.ev(f"zero_bytes:{row.zero_bytes}")

    def _record(self, x, flags, cbp, mv):
        m = dict(x=x, y=self.y, flags=flags, cbp=cbp, qscale=self.q, ncoef=0, coef_off=len(self.coefs), mv=mv)
        self.mbs.append(m)
        return m

    def _inside(self, x, vx, vy, field, fs):
        """every MC read of the vector stays inside every plane (the accepted contract)"""
        for plane in range(3):
            mx, my = vx, vy
            w, h, pw, ph = 16, 16, self.width, self.height
            if plane:
                if self.cf < 3:
                    mx, w, pw = mx >> 1, 8, pw // 2
                if self.cf < 2:
                    my, h, ph = my >> 1, 8, ph // 2
            x0 = x * w + (mx >> 1)
            x1 = x0 + w - 1 + (mx & 1)
            if not field:
                y0 = self.y * h + (my >> 1)
                y1 = y0 + h - 1 + (my & 1)
            else:
                y0 = self.y * h + fs + 2 * (my >> 1)
                y1 = y0 + 2 * (h // 2 - 1) + 2 * (my & 1)
            if x0 < 0 or y0 < 0 or x1 > pw - 1 or y1 > ph - 1:
                return False
        return True

    # ---- skipped macroblocks (7.6.6) -----------------------------------------------------------
    def _skips(self, n, x):
        P = self.P
        assert P.pct != 1 or self._negative, "skipped macroblock in an I picture"
        if n in (1, 32, 33, 34, 67):
            self.ev(f"skip_run:{n}")
        prev = self.prev
        if P.pct == 2:
            if any(v for r in self.PMV for s in r for v in s):
                self.pending_reset = "skip_P"
            if prev is not None and prev.field and prev.t & FWD:
                self.ev("skip_P:after_field")
            self.PMV = [[[0, 0], [0, 0]], [[0, 0], [0, 0]]]  # 7.6.3.4
            flags = R_FWD
            mv = [[[0, 0], [0, 0]], [[0, 0], [0, 0]]]
        else:
            # B picture: the direction(s) of the previous macroblock, the predictors unchanged.
            # REFERENCE: the standard predicts a skipped B macroblock with PMV[0][s]; the reference
            # runs base_motion_compensation<frame, two_vect = true, skipped = true> on cache.PMVs
            # (mb_decoder.cpp:546-548), whose second vector's prediction (:304-308, :314-318,
            # :324-328) overwrites the first's, so the vectors that count are PMV[1][s].  They
            # differ from PMV[0][s] only after a field macroblock.
            t = prev.t if prev is not None else 0
            flags = (R_FWD if t & FWD else 0) | (R_BWD if t & BWD else 0)
            if not flags:
                flags = R_FWD
            # (the record of a skipped macroblock carries the predictors of both directions)
            mv = [[list(self.PMV[1][0]), list(self.PMV[1][1])], [[0, 0], [0, 0]]]
            if prev is not None and not (prev.t & INTRA):
                if prev.field:
                    if self.PMV[1] != self.PMV[0]:
                        self.ev("skip_B:after_field")
                else:
                    self.ev("skip_B:after_" + {FWD: "fwd", BWD: "bwd", FWD | BWD: "bi"}[prev.t & (FWD | BWD)])
        for i in range(n):
            for s in range(2):
                if flags & (R_FWD << s):
                    assert self._inside(x + i, mv[0][s][0], mv[0][s][1], False, 0), (self.name, self.y, x + i)
            self._record(x + i, flags, 0, [[list(v) for v in r] for r in mv])
        if x + n == self.mbw - 1 and not self._negative:
            self.ev("skip_ends_at_mbw-2")
        self.skipped_before = True
        for s in range(2):
            self.hist[s] = []
        self.copy_pending = None
        return x + n

    # ---- motion vectors (6.2.5.2, 6.2.5.2.1, 7.6.3) ----------------------------------------------
    def _motion(self, s, field, vecs, x, record=True):
        P, b = self.P, self.bw
        four = P.pct == 3 and len({P.fcode[0][0], P.fcode[0][1], P.fcode[1][0], P.fcode[1][1]}) == 4
        for r, (fs, target) in enumerate(vecs):
            if field:
                b.put(fs, 1)  # motion_vertical_field_select[r][s]
            for t in range(2):
                fc = P.fcode[s][t]
                assert 1 <= fc <= 9
                f = 1 << (fc - 1)
                low, high, rng = -16 * f, 16 * f - 1, 32 * f
                fv = field and t == 1
                pmv = self.PMV[r][s][t]
                pred = pmv // 2 if fv else pmv  # DIV: towards minus infinity (4.1)
                if fv and pmv % 2 and record:
                    self.ev("field_vert_pred:odd_neg" if pmv < 0 else "field_vert_pred:odd_pos")
                delta = target[t] - pred
                if delta < low:
                    delta += rng
                if delta > high:
                    delta -= rng
                assert low <= delta <= high and low <= target[t] <= high, (self.name, target, pred, fc)
                if record and pred + delta > high:
                    self.ev(f"wrap_high:{'hv'[t]}:{fc}")
                if record and pred + delta < low:
                    self.ev(f"wrap_low:{'hv'[t]}:{fc}")
                if delta == 0:
                    b.code(MOTION[0])
                    if fc > 1 and record:
                        self.ev("delta0_fcode_gt1")
                else:
                    a = abs(delta) - 1
                    code = a // f + 1
                    b.code(MOTION[code if delta > 0 else -code])  # (the table's code carries the sign)
                    b.put(a % f, fc - 1)                          # motion_residual
                    if four and record:
                        self.ev(f"fcode_slot:{s}{t}:{fc}")
                        self.ev("fcode4:field" if field else "fcode4:frame")
                self.PMV[r][s][t] = target[t] * 2 if fv else target[t]
            if record:
                assert self._inside(x, target[0], target[1], field, fs), (self.name, self.y, x, target)
        if not field:  # table 7-9: PMV[1][s] = PMV[0][s] after a frame vector
            self.PMV[1][s] = list(self.PMV[0][s])

    # ---- one coded macroblock (6.2.5) ------------------------------------------------------------
    def macroblock(self, mb, x):
        P, b = self.P, self.bw
        n = mb.skip
        while n + 1 > 33:
            b.code(MB_ESCAPE)
            n -= 33
        b.code(MBA[n + 1])
        if mb.skip:
            x = self._skips(mb.skip, x)
        t = mb.t
        intra, fwd, bwd, pat = bool(t & INTRA), bool(t & FWD), bool(t & BWD), bool(t & PAT)
        b.code(MBTYPE[P.pct][t])
        self.ev(f"mbtype:{P.pct}:{t}")
        field = mb.field and (fwd or bwd) and not intra
        if (fwd or bwd) and P.fpfd == 0:
            b.put(1 if field else 2, 2)  # frame_motion_type: field-based / frame-based
        else:
            assert not field
        if P.fpfd == 0 and (intra or pat):
            b.put(mb.dct, 1)
            self.ev(f"dct_type:{mb.dct}:{'intra' if intra else 'pattern'}")
            assert not (mb.dct and self.cf == 3)
        else:
            assert not mb.dct
        if t & QUANT:
            b.put(mb.q, 5)
            self.q = qscale_of(mb.q, P.qst)
            self.ev(f"qcode_mb:{P.qst}:{mb.q}")
            self.q_from_mb = True
        elif (intra or pat) and self.skipped_before and self.q_from_mb:
            self.ev("qscale_across_skip")

        # vectors
        had_pmv = any(v for r in self.PMV for s in r for v in s)
        before = [[list(v) for v in r] for r in self.PMV]
        if intra and P.cmv:
            assert P.pct == 1 or self._negative
            self._motion(0, False, [(0, mb.cmv)], x, record=False)
            b.put(1, 1)  # marker_bit
        for s, on in ((0, fwd), (1, bwd)):
            if not on or intra:
                continue
            vecs = mb.mv[s]
            assert len(vecs) == (2 if field else 1)
            if self.pending_reset and self.pending_reset != "skip_P":
                self.ev(f"pmv_reset:{self.pending_reset}")
            elif self.pending_reset == "skip_P":
                self.ev("skip_P:after_nonzero_pmv")
            if field and self.copy_pending and self.copy_pending[s]:
                # the field macroblock's second vector is predicted from the copy PMV[1][s] <- PMV[0][s]
                self.ev("pmv_copy:" + self.copy_pending[2])
            self._motion(s, field, vecs, x)
        if fwd or bwd:
            self.pending_reset = None
        if not intra:
            for s, on in ((0, fwd), (1, bwd)):
                h = self.hist[s]
                if not on:
                    h.clear()
                    continue
                h.append(("field", tuple(v[0] for v in mb.mv[s])) if field else ("frame", None))
                name = "fwd" if s == 0 else "bwd"
                if [k for k, _ in h[-3:]] == ["frame", "field", "frame"]:
                    self.ev(f"seq:frame_field_frame:{name}")
                if len(h) >= 2 and h[-1][0] == h[-2][0] == "field" and h[-1][1] != h[-2][1]:
                    self.ev(f"seq:field_field_fs:{name}")
        else:
            self.hist = {0: [], 1: []}

        # predictor resets (7.6.3.4) and the record
        mv = [[[0, 0], [0, 0]], [[0, 0], [0, 0]]]
        flags = 0
        if intra:
            flags |= R_INTRA
            if P.pct != 1:
                self.ev(f"intra_in:{'PB'[P.pct - 2]}")
                if not P.cmv:
                    if had_pmv:
                        self.pending_reset = "intra_" + "PB"[P.pct - 2]
                    self.PMV = [[[0, 0], [0, 0]], [[0, 0], [0, 0]]]
            self.copy_pending = None
        else:
            if P.pct == 2 and not fwd:  # pattern only: zero forward vector, predictors reset
                if had_pmv:
                    self.pending_reset = "pattern_only_P"
                self.PMV = [[[0, 0], [0, 0]], [[0, 0], [0, 0]]]
                flags |= R_FWD
                self.copy_pending = None
            else:
                flags |= (R_FWD if fwd else 0) | (R_BWD if bwd else 0) | (R_FIELD if field else 0)
                for s, on in ((0, fwd), (1, bwd)):
                    if on:
                        for r, (fs, target) in enumerate(mb.mv[s]):
                            mv[r][s] = list(target)
                            if field and fs:
                                flags |= 1 << (8 + 2 * r + s)
                if field:
                    self.copy_pending = None
                else:
                    # a copy shows only where PMV[1][s] changes to something a field vector reads
                    ch = [on and before[1][s] != self.PMV[1][s] for s, on in ((0, fwd), (1, bwd))]
                    self.copy_pending = (ch[0], ch[1], {FWD: "fwd", BWD: "bwd", FWD | BWD: "bi"}[t & (FWD | BWD)])
        if mb.dct and (intra or pat):
            flags |= R_DCTF

        # DC predictors (7.2.1): reset after a skip and after a non-intra macroblock
        if mb.skip or not intra:
            dirty = any(d != self.dc_reset for d in self.dc)
            if dirty and intra and mb.skip and self.prev is not None and self.prev.t & INTRA:
                self.ev("dc_reset:skip")
            if dirty and not intra and not mb.skip:
                self._dc_nonintra = True  # shown by the next intra macroblock
            self.dc = [self.dc_reset] * 3
        if intra:
            if self._dc_nonintra and not mb.skip:
                self.ev("dc_reset:after_nonintra")
            self._dc_nonintra = False

        # coded_block_pattern (6.2.5.3)
        cbp = (1 << self.nblocks) - 1 if intra else 0
        if pat:
            cbp = mb.cbp
            v420 = sum(((cbp >> i) & 1) << (5 - i) for i in range(6))
            b.code(CBP[v420])
            if self.cf == 1:
                assert v420
                self.ev(f"cbp420:{v420}")
            elif self.cf == 2:
                ext = (((cbp >> 6) & 1) << 1) | ((cbp >> 7) & 1)  # coded_block_pattern_1: block 6 first
                b.put(ext, 2)
                self.ev(f"cbp422:{'nonzero' if v420 else 'zero'}:{ext}")
            else:
                ext = sum(((cbp >> (6 + i)) & 1) << (5 - i) for i in range(6))  # coded_block_pattern_2
                b.put(ext, 6)
                bits = [i for i in range(6) if ext >> (5 - i) & 1]
                if len(bits) == 0:
                    self.ev("cbp444:none")
                elif len(bits) == 6:
                    self.ev("cbp444:all")
                elif len(bits) == 1:
                    self.ev(f"cbp444:bit{bits[0]}")
        rec = self._record(x, flags, cbp, mv)

        # blocks (6.2.6, 7.2)
        if intra:
            self.ev(f"b15:{'IPB'[P.pct - 1]}")
            if self.prev is not None and self.prev.t & PAT and not self.prev.t & INTRA and not mb.skip and P.pct > 1:
                self.ev(f"b14_b15_neighbours:{'PB'[P.pct - 2]}")
        elif pat and self.prev is not None and self.prev.t & INTRA and not mb.skip:
            self.ev(f"b14_b15_neighbours:{'PB'[P.pct - 2]}")
        tag = (x & 7) << 26
        for blk in range(self.nblocks):
            if not cbp >> blk & 1:
                assert blk not in mb.blocks or not (mb.blocks[blk].coefs or mb.blocks[blk].dc)
                continue
            B = mb.blocks.get(blk) or Block()
            i = 0
            words = []
            if intra:
                comp = 0 if blk < 4 else (2 if blk & 1 else 1)  # Y, Cb (even blocks), Cr (odd blocks)
                self._dc(B.dc if B.dc_abs is None else B.dc_abs - self.dc[comp], comp)
                dcv = self.dc[comp] << (3 - P.prec)              # intra_dc_mult (7.4.1)
                words.append((dcv & 0xFFFF) | (blk << 22) | tag | W_DC)
                i = 1
                self._pic_stats["intra"] = self._pic_stats["intra"] or (blk < 4 and len(B.coefs) > 1)
                self._pic_stats["chroma_intra"] = self._pic_stats["chroma_intra"] or (blk >= 4 and len(B.coefs) > 1)
            else:
                assert B.coefs, "a coded non-intra block has a coefficient"
                self._pic_stats["inter"] = self._pic_stats["inter"] or (blk < 4 and len(B.coefs) > 1)
                self._pic_stats["chroma_inter"] = self._pic_stats["chroma_inter"] or (blk >= 4 and len(B.coefs) > 1)
            tab = 1 if intra else 0  # intra_vlc_format 1: B.15 for intra blocks, B.14 otherwise
            levels_1s = None
            for k, c in enumerate(B.coefs):
                run, level, esc = (c + (False,))[:3]
                assert level and -2047 <= level <= 2047
                pos = i + run
                assert pos <= 63, (self.name, x, blk, pos)
                if not intra and k == 0 and run == 0 and abs(level) == 1 and not esc:
                    b.code("1"), b.put(level < 0, 1)   # first coefficient of a non-intra block: '1s'
                    words.append((level & 0xFFFF) | (blk << 22) | tag | W_FIRST1S)
                    self.ev("coef:first_1s")
                    levels_1s = level
                else:
                    code = None if esc else COEF[tab].get((run, abs(level)))
                    if code is None:
                        b.code(COEF_ESCAPE), b.put(run, 6), b.put(level & 0xFFF, 12)
                        if run in (0, 63) and level in (1, -1, 2047, -2047):
                            self.ev(f"escape:run{run}:{level}")
                    else:
                        b.code(code), b.put(level < 0, 1)
                        if tab == 0 and k > 0 and run == 0 and level == levels_1s:
                            assert code == "11"
                            self.ev("coef:later_11s")
                    words.append((level & 0xFFFF) | (pos << 16) | (blk << 22) | tag)
                if pos == 63 and run > 0:
                    self.ev("coef:run_ends_63")
                i = pos + 1
            b.code(EOB[tab])
            if len(words) == 1 and not intra:
                self.ev("coef:block_of_one")
            if len(words) == 64:
                self.ev("coef:block_of_64")
            self.coefs += words
            rec["ncoef"] += len(words)
        cb = [mb.blocks[k].dc for k in range(4, self.nblocks, 2) if k in mb.blocks and mb.blocks[k].dc_abs is None]
        cr = [mb.blocks[k].dc for k in range(5, self.nblocks, 2) if k in mb.blocks and mb.blocks[k].dc_abs is None]
        if intra and len(cb) >= 2 and len(cr) >= 2 and cb != cr and any(cb) and any(cr):
            self.ev(f"dc_chains:{'422' if self.cf == 2 else '444'}")
        self.prev = mb
        self.skipped_before = False
        return x + 1

    def _dc(self, diff, comp):
        """dct_dc_size and dct_dc_differential (7.2.1)"""
        b, P = self.bw, self.P
        size = abs(diff).bit_length()
        assert size <= 11
        b.code(DCSIZE[1 if comp else 0][size])
        if size:
            b.put(diff if diff > 0 else diff + (1 << size) - 1, size)
        self.dc[comp] += diff
        assert 0 <= self.dc[comp] < (256 << P.prec), (self.name, self.dc, diff)
        name = "chroma" if comp else "luma"
        self.ev(f"dc_prec:{P.prec}:{size}")
        if size == 0:
            self.ev(f"dc:{name}:0")
        else:
            for m, mag in (("min", 1 << (size - 1)), ("max", (1 << size) - 1)):
                if abs(diff) == mag:
                    self.ev(f"dc:{name}:{size}:{m}:{'neg' if diff < 0 else 'pos'}")

    _negative = False


# =================================================================================================
# The directed streams.  Every builder returns a finished Stream (bytes in .es).  Pictures are the
# smallest that hold the case; each has at least one macroblock that changes pixels, and the
# random textures differ from picture to picture, so no two frames of a stream are equal.
# =================================================================================================
def _rng(name):
    return np.random.default_rng(int.from_bytes(name.encode(), "big") % (1 << 63))


def _ac(rng, n, big=3):
    """n coefficients at rising positions"""
    return [(int(rng.integers(0, 3)), int(rng.choice([-1, 1])) * int(rng.integers(1, big + 1))) for _ in range(n)]


def tex_mb(S, rng, prec=0, nac=2, **kw):
    """an intra macroblock of random texture: absolute DC values, a few AC coefficients"""
    t = kw.pop("t", INTRA)
    blocks = {b: Block(_ac(rng, nac), dc_abs=int(rng.integers(60, 200)) << prec) for b in range(S.nblocks)}
    return MB(t, blocks=blocks, **kw)


def tex_pic(S, rng, **kw):
    prec = kw.get("prec", 0)
    return Pic(1, [Row([tex_mb(S, rng, prec) for _ in range(S.mbw)]) for _ in range(S.mbh)], **kw)


def pat(S, level, t=PAT, cbp=1, **kw):
    """a macroblock with coded blocks of one strong coefficient each (it changes pixels)"""
    blocks = {b: Block([(0, level)]) for b in range(S.nblocks) if cbp >> b & 1}
    return MB(t, cbp=cbp, blocks=blocks, **kw)


def skip_row(S, level, first=None):
    """a P/B row with as little as the contract allows: first and last macroblock coded"""
    return Row([first or pat(S, level), pat(S, -level, skip=S.mbw - 2)])


def _finish(S, pics):
    S.es = S.write(pics)
    return S


def fr(x, y):
    return [(0, (x, y))]


# ---- four pairwise different f_codes in one B picture ----------------------------------------------
def fcode4(k):
    S = Stream(f"fcode4_{k}", 64, 48, 1)
    rng = _rng(S.name)
    pics = [tex_pic(S, rng, fpfd=0), None]
    p_rows = [Row([MB(FWD, mv={0: fr(1, 1)}), pat(S, 9, FWD | PAT, mv={0: fr(2, 0)}), MB(FWD, mv={0: fr(-1, 1)}),
                   pat(S, -8, FWD | PAT, mv={0: fr(-2, 0)})]),
              skip_row(S, 7), skip_row(S, -6)]
    pics[1] = Pic(2, p_rows, fpfd=0)
    for a in (2 * k, 2 * k + 1):
        if a >= 9:
            break
        fc = [(a + 2 * j) % 9 + 1 for j in range(4)]  # slot j of assignment a: every value in every slot
        fcode = ((fc[0], fc[1]), (fc[2], fc[3]))
        sig = 6 + a
        rows = [
            Row([MB(FWD, mv={0: fr(2, 1)}), MB(BWD, mv={1: fr(1, 2)}),
                 MB(FWD | BWD, mv={0: fr(-1, 2), 1: fr(-2, 1)}),
                 pat(S, sig, FWD | BWD | PAT, mv={0: fr(-2, 1), 1: fr(-1, 2)})]),
            Row([MB(FWD, field=True, mv={0: [(0, (1, 1)), (1, (2, -1))]}),
                 MB(BWD, field=True, mv={1: [(1, (2, -1)), (0, (1, 1))]}),
                 MB(FWD | BWD, field=True, mv={0: [(1, (-1, -1)), (1, (-2, 1))], 1: [(0, (-1, 1)), (1, (-2, -1))]}),
                 pat(S, -sig, FWD | BWD | PAT, field=True,
                     mv={0: [(0, (-2, 1)), (0, (-1, -1))], 1: [(1, (-2, -1)), (0, (-1, 1))]})]),
            Row([MB(BWD, mv={1: fr(1, -1)}), pat(S, sig + 1, FWD | PAT, mv={0: fr(-1, -2)}, skip=2)]),
        ]
        pics.append(Pic(3, rows, fcode=fcode, fpfd=0))
    return _finish(S, pics)


# ---- wraps below `low` and above `high` --------------------------------------------------------------
def wrap_h(name, fcs):
    """1040x16 P pictures, one per horizontal f_code.  With f = 1 << (f_code - 1): column 0 carries
    16 f - 2 (8 f - 1 samples to the right: its last read is sample 8 f + 14 <= 1039 for f_code 8),
    column 1 the target -4, which is 16 f + 2 below it (a wrap above high), column 2 the target
    16 f - 4, which is 16 f above it (a wrap below low; for f_code 8 its reads would end at sample
    1069, so that wrap does not fit)."""
    S = Stream(name, 1040, 16, 1)
    rng = _rng(name)
    pics = [tex_pic(S, rng)]
    for fc in fcs:
        f = 1 << (fc - 1)
        mbs = [MB(FWD, mv={0: fr(16 * f - 2, 0)}), MB(FWD, mv={0: fr(-4, 0)})]
        if fc < 8:
            mbs.append(MB(FWD, mv={0: fr(16 * f - 4, 0)}))
        mbs.append(pat(S, 5 + fc, skip=S.mbw - 1 - len(mbs)))
        pics.append(Pic(2, [Row(mbs)], fcode=((fc, 1), (15, 15))))
    return _finish(S, pics)


def wrap_v(name, fcs):
    """176x144 P pictures, one per vertical f_code, the vectors in row 4 (samples 64..79): -8 f
    (4 f samples up: row 0 of the picture for f_code 5), then 8 f, 16 f above it (a wrap below low;
    its last read is line 79 + 4 f <= 143), then 8 f + 2 and -8 f, 16 f + 2 below it (a wrap above
    high; for f_code 5 the half-sample read of 8 f + 2 would end at line 144, so it does not fit)."""
    S = Stream(name, 176, 144, 1)
    rng = _rng(name)
    pics = [tex_pic(S, rng)]
    for fc in fcs:
        f = 1 << (fc - 1)
        mbs = [MB(FWD, mv={0: fr(0, -8 * f)}), MB(FWD, mv={0: fr(0, 8 * f)})]
        if fc < 5:
            mbs += [MB(FWD, mv={0: fr(0, 8 * f + 2)}), MB(FWD, mv={0: fr(0, -8 * f)})]
        mbs.append(pat(S, 5 + fc, skip=S.mbw - 1 - len(mbs)))
        rows = [skip_row(S, 4 + y + fc) for y in range(S.mbh)]
        rows[4] = Row(mbs)
        pics.append(Pic(2, rows, fcode=((1, fc), (15, 15))))
    return _finish(S, pics)


# ---- predictor sequences, resets, copies and skips --------------------------------------------------
def mv_seq():
    S = Stream("mv_seq", 112, 48, 1)
    rng = _rng(S.name)
    F, Bk = FWD, BWD
    intra = lambda **kw: tex_mb(S, rng, **kw)  # noqa: E731
    p_rows = [
        Row([MB(F, mv={0: fr(2, 3)}),                                        # odd positive vertical PMV
             MB(F, field=True, mv={0: [(0, (2, 1)), (1, (3, 2))]}),          # field after frame
             MB(F, mv={0: fr(1, 2)}),                                        # frame after field
             intra(),                                                        # PMV reset by intra
             pat(S, 9, F | PAT, mv={0: fr(-2, 1)}),                          # shows the reset; B.14 after B.15
             MB(F, mv={0: fr(-2, 1)}),                                       # delta 0 under f_code 2
             intra()]),                                                      # DC reset after non-intra
        Row([MB(F, mv={0: fr(2, -3)}),                                       # slice start reset; odd negative
             MB(F, field=True, mv={0: [(1, (1, -2)), (0, (2, -1))]}),
             MB(F, field=True, mv={0: [(0, (1, -1)), (1, (2, -2))]}),        # other field selects
             MB(F, skip=1, mv={0: fr(1, 1)}),                                # P skip after field, PMV != 0
             MB(F, mv={0: fr(1, 1)}),
             pat(S, -9)]),
        Row([MB(F, mv={0: fr(2, -2)}),
             pat(S, 8),                                                      # pattern only: PMV reset
             MB(F, mv={0: fr(1, -1)}),
             MB(F, mv={0: fr(-1, -1)}),
             intra(t=INTRA | QUANT, q=5),
             intra(skip=1)]),                                                # DC reset by the skip, q kept
    ]
    b0 = [
        Row([MB(F, mv={0: fr(2, 2)}),
             MB(Bk, skip=1, mv={1: fr(2, 1)}),                               # B skip after forward
             MB(F | Bk, skip=1, mv={0: fr(1, 2), 1: fr(1, 1)}),              # ... after backward
             pat(S, 7, F | PAT, skip=1, mv={0: fr(-1, 1)})]),                # ... after bidirectional
        Row([MB(F, mv={0: fr(3, -1)}),                                       # copy PMV[1][0] <- PMV[0][0]
             MB(F, field=True, mv={0: [(0, (2, 1)), (1, (1, -1))]}),
             MB(F, mv={0: fr(1, 1)}),
             MB(Bk, mv={1: fr(2, 1)}),                                       # copy PMV[1][1] <- PMV[0][1]
             MB(Bk, field=True, mv={1: [(1, (1, 1)), (0, (-1, -1))]}),
             MB(Bk, mv={1: fr(-1, 1)}),
             intra()]),
        Row([MB(F | Bk, mv={0: fr(2, -1), 1: fr(1, -2)}),                    # both copies
             MB(F | Bk, field=True, mv={0: [(0, (1, -1)), (1, (2, -2))], 1: [(1, (1, -1)), (0, (2, 0))]}),
             MB(Bk, field=True, mv={1: [(0, (1, -2)), (1, (-1, -1))]}),      # other field selects
             intra(skip=1),                                                  # B skip after field; PMV reset by intra
             pat(S, -7, F | PAT, mv={0: fr(-1, -1)}),                        # shows it; B.14 after B.15
             pat(S, 6, Bk | PAT, mv={1: fr(-1, 0)})]),
    ]
    pics = [tex_pic(S, rng, fpfd=0), Pic(2, p_rows, fpfd=0), Pic(3, b0, fpfd=0)]
    return _finish(S, pics)


def skip_runs():
    """one-row pictures of 70 macroblocks: runs of 67 (two escapes), 34 and 33 (one), 32 and 1 (none)"""
    S = Stream("skip_runs", 1120, 16, 1)
    rng = _rng(S.name)
    rows = [Row([pat(S, 9), pat(S, -8, skip=67), pat(S, 7)]),
            Row([pat(S, 6), pat(S, -9, skip=34), pat(S, 8, skip=33)]),
            Row([pat(S, 5), pat(S, -6, skip=32), pat(S, 9, skip=1), pat(S, -7, skip=33)])]
    return _finish(S, [tex_pic(S, rng)] + [Pic(2, [r]) for r in rows])


# ---- macroblock types, quantiser codes, dct_type -----------------------------------------------------
def mbtypes():
    S = Stream("mbtypes", 176, 16, 1)
    rng = _rng(S.name)

    def of_type(t, x, k):
        kw = dict(q=3 + k % 9) if t & QUANT else {}
        dct = k & 1
        if t & INTRA:
            return tex_mb(S, rng, t=t, dct=dct, **kw)
        mv = {}
        sx = 1 if x < 5 else -1
        if t & FWD:
            mv[0] = fr(sx * (1 + k % 3), 0)
        if t & BWD:
            mv[1] = fr(sx * (1 + (k + 1) % 3), 0)
        if t & PAT:
            return pat(S, 5 + k, t, cbp=1 + k % 63, dct=dct, mv=mv, **kw)
        return MB(t, mv=mv, **kw)

    i_row = [of_type([INTRA, INTRA | QUANT][x & 1], x, x + (x >> 1)) for x in range(11)]
    ptypes = sorted(MBTYPE[2])
    p_row = [of_type(ptypes[x % 7], x, x + (x >= 7)) for x in range(11)]
    b_row = [of_type(t, x, x) for x, t in enumerate(sorted(MBTYPE[3], reverse=True))]
    b_row[-1], b_row[5] = b_row[5], b_row[-1]  # (a B skip must not follow intra: none here anyway)
    for x, m in enumerate(b_row):  # vectors point inward at their final column
        for s in m.mv:
            v = m.mv[s][0][1]
            m.mv[s] = fr(abs(v[0]) if x < 5 else -abs(v[0]), 0)
    return _finish(S, [Pic(1, [Row(i_row)], fpfd=0), Pic(2, [Row(p_row)], fpfd=0), Pic(3, [Row(b_row)], fpfd=0)])


def quant(qst):
    """every quantiser_scale_code once from the slice header and once from macroblock_quant"""
    S = Stream(f"quant_q{qst}", 32, 256, 1)
    rng = _rng(S.name)
    pics = []
    for half in range(2):
        rows = []
        for y in range(16):
            c = 1 + (16 * half + y) % 31
            rows.append(Row([tex_mb(S, rng), tex_mb(S, rng, t=INTRA | QUANT, q=32 - c)], qcode=c))
        pics.append(Pic(1, rows, qst=qst))
    return _finish(S, pics)


# ---- coded block pattern -----------------------------------------------------------------------------
def _rec_cbp(v420, ext, next_bits):
    """record-style pattern (bit b = block b) from coded_block_pattern_420 and the extension"""
    c = sum(((v420 >> (5 - i)) & 1) << i for i in range(6))
    return c | sum(((ext >> (next_bits - 1 - i)) & 1) << (6 + i) for i in range(next_bits))


def cbp420():
    S = Stream("cbp420", 176, 96, 1)
    rng = _rng(S.name)
    mbs = [pat(S, 4 + v % 7, PAT if v % 3 else FWD | PAT, cbp=_rec_cbp(1 + v % 63, 0, 0),
               **({} if v % 3 else dict(mv={0: fr(0, 0)}))) for v in range(66)]
    rows = [Row(mbs[11 * y:11 * y + 11]) for y in range(6)]
    return _finish(S, [tex_pic(S, rng), Pic(2, rows)])


def cbp422():
    S = Stream("cbp422", 64, 32, 2)
    rng = _rng(S.name)
    cases = [(v, e) for v in (0, 0b101101) for e in range(4)]
    mbs = [pat(S, 5 + i, cbp=_rec_cbp(v, e, 2)) for i, (v, e) in enumerate(cases)]
    mbs[0], mbs[1] = mbs[1], mbs[0]
    return _finish(S, [tex_pic(S, rng), Pic(2, [Row(mbs[:4]), Row(mbs[4:])])])


def cbp444():
    S = Stream("cbp444", 64, 32, 3)
    rng = _rng(S.name)
    cases = [(0b110011, 0), (0b011110, 63)] + [(0 if i & 1 else 1 << i, 1 << i) for i in range(6)]
    mbs = [pat(S, 5 + i, cbp=_rec_cbp(v, e, 6)) for i, (v, e) in enumerate(cases)]
    return _finish(S, [tex_pic(S, rng), Pic(2, [Row(mbs[:4]), Row(mbs[4:])])])


# ---- DC ------------------------------------------------------------------------------------------------
def dc_units(prec):
    """closed walks of four differentials from the reset value 128 << prec: for each dct_dc_size
    the least and the greatest differential in both signs.  Sizes up to 7 + prec step out and
    back; size 8 + prec, the largest the precision reaches, goes 0 -> maximum -> 0 -> reset."""
    units = [[0, 0, 0, 0]]
    for size in range(1, 9 + prec):
        lo, hi = 1 << (size - 1), (1 << size) - 1
        units.append([lo, -lo, hi, -hi] if size < 8 + prec else [-lo, hi, -hi, lo])
    return units


def dc(prec, cf):
    units = dc_units(prec)
    n = len(units)
    per_mb = 2 if cf == 2 else 4               # blocks of each chroma component in a macroblock
    rows_n = n * 4 // (2 * per_mb)             # two macroblocks per row
    S = Stream(f"dc_p{prec}_{'420 422 444'.split()[cf - 1]}", 32, 16 * rows_n, cf)
    rng = _rng(S.name)
    cb = [d for u in units for d in u]
    cr = [d for u in reversed(units) for d in u]  # the Cr chain runs the sizes the other way
    rows, k = [], 0
    for y in range(rows_n):
        mbs = []
        for x in range(2):
            u = units[(2 * y + x) % n]
            blocks = {b: Block(_ac(rng, 1), dc=u[b]) for b in range(4)}
            for j in range(per_mb):
                blocks[4 + 2 * j] = Block(_ac(rng, 1), dc=cb[k + j])
                blocks[5 + 2 * j] = Block(_ac(rng, 1), dc=cr[k + j])
            k += per_mb
            mbs.append(MB(INTRA, blocks=blocks))
        rows.append(Row(mbs))
    return _finish(S, [Pic(1, rows, prec=prec)])


# ---- coefficients ------------------------------------------------------------------------------------------
def coefs():
    S = Stream("coefs", 64, 32, 1)
    rng = _rng(S.name)
    dense = [(0, 1 + (i % 2)) for i in range(63)]
    i_rows = [Row([tex_mb(S, rng) for _ in range(4)]) for _ in range(2)]
    i_rows[0].mbs[1].blocks[0] = Block(dense, dc_abs=100)                         # 64 coefficients, B.15
    i_rows[0].mbs[2].blocks[1] = Block([(0, 1, True), (0, -1, True), (3, 2047), (0, -2047)], dc_abs=90)
    i_rows[1].mbs[0].blocks[2] = Block([(4, 2), (57, -3)], dc_abs=120)            # run ends at position 63
    nb = lambda *bl: MB(PAT, cbp=(1 << len(bl)) - 1, blocks=dict(enumerate(bl)))  # noqa: E731
    p_rows = [
        Row([nb(Block([(0, 1)]), Block([(0, -1), (0, -1), (2, 3)]), Block([(5, 3), (57, 2)])),
             nb(Block([(0, 1)] + [(0, 1 + (i % 2)) for i in range(63)])),         # 64 coefficients, B.14
             nb(Block([(0, 1, True), (0, -1, True)]), Block([(0, 2047), (0, -2047)])),
             nb(Block([(63, 1)]), Block([(63, -1)]), Block([(63, 2047)]), Block([(63, -2047)]))]),
        skip_row(S, 9),
    ]
    return _finish(S, [Pic(1, i_rows), Pic(2, p_rows)])


# ---- picture level -----------------------------------------------------------------------------------------
def asym_matrices():
    """four pairwise different matrices, every entry a strictly rising function of its position in
    the transmitted (zig-zag) order: no two positions and no two matrices can be swapped unseen"""
    return [[16 + 3 * k + i for i in range(64)] for k in range(4)]


def piclevel(prec):
    S = Stream(f"piclevel_p{prec}", 32, 16, 1)
    rng = _rng(S.name)
    pics = [Pic(1, [Row([tex_mb(S, rng, prec, nac=6) for _ in range(2)], qcode=6)], prec=prec, qst=q, alt=a,
                mats=asym_matrices()) for a in (0, 1) for q in (0, 1)]
    return _finish(S, pics)


def matrices(cf):
    S = Stream(f"matrices_{'420 422 444'.split()[cf - 1]}", 48, 32, cf)
    rng = _rng(S.name)
    big = lambda: _ac(rng, 5, big=9)  # noqa: E731

    def inter(t=PAT, **kw):
        return MB(t, cbp=(1 << S.nblocks) - 1, blocks={b: Block(big()) for b in range(S.nblocks)}, **kw)

    def intra():
        m = tex_mb(S, rng, nac=0)
        for b in m.blocks.values():
            b.coefs = big()
        return m

    i_pic = Pic(1, [Row([intra() for _ in range(3)], qcode=6) for _ in range(2)], mats=asym_matrices())
    p_pic = Pic(2, [Row([inter(), intra(), inter(FWD | PAT, mv={0: fr(-1, 1)})], qcode=5),
                    Row([intra(), inter(), inter()], qcode=7)], alt=1, mats=asym_matrices())
    return _finish(S, [i_pic, p_pic])


# ---- slice header and slice end ----------------------------------------------------------------------------
SLICE_EXT = [(0, []), (1, []), (0, [0xA5]), (1, [0x5A]), (0, [0xFF, 0x01, 0x80]), (1, [0x00, 0xFE, 0x7F]), None, None]


def slice_hdr():
    """eight one-macroblock rows: the six slice-header extensions, 0..7 stuffing bits (row y ends
    with y stuffing bits, so row 0's last macroblock ends on a byte boundary) and 0..3 zero bytes
    before the next start code.  The stuffing is steered by the count of 3-bit codes (B.15 '10s')
    in the row's last block."""
    def build(extra):
        S = Stream("slice_hdr", 16, 128, 1)
        rng = _rng(S.name)
        rows = []
        for y in range(8):
            m = tex_mb(S, rng)
            m.blocks[5].coefs = [(0, 1)] * extra[y]
            rows.append(Row([m], ext=SLICE_EXT[y], zero_bytes=y % 4))
        return _finish(S, [Pic(1, rows)])

    extra = [0] * 8
    for y in range(8):
        for n in range(8):
            extra[y] = n
            if build(extra).stuffing[y] == y:
                break
        else:
            raise AssertionError("no count of 3-bit codes gives the stuffing")
    return build(extra)


# ---- the geometry limits: sizes above 4095, slices below row 127 ---------------------------------------------
# REFERENCE: the standard has slice_vertical_position_extension when vertical_size (14 bits) is above
# 2800 (6.2.4); the reference asks the 12-bit vertical_size_value (mp2v_hdr.h:347, decoder.cpp:119).
# A coded height of 4096 or more is therefore decodable only through a vertical_size whose low 12
# bits are above 2800: 8192 as 8191, 12288 as 12287, 16384 as 16383.  neg_vsize_4112 is the other kind.
def _v(vy, fs=None):
    return [(0, (0, vy))] if fs is None else [(fs[0], (0, vy)), (fs[1], (0, vy))]


def tall(name, width, height, vsize, long_fc):
    """I, P and B at `width` x `height` (one or two MBs per row): every row is a slice, so every
    value of slice_vertical_position_extension the height reaches is written.  P: vertical vectors
    that cross the 128-row boundaries of the extension in both directions (the rows next to each
    boundary), the longest vectors of vertical f_code long_fc from row 0 and from the last row, and
    short ones between.  B: bidirectional frame vectors, and field MC with every pair of field
    selects in the last four rows."""
    S = Stream(name, width, height, 1, vsize=vsize)
    rng = _rng(name)
    f = 1 << (long_fc - 1)
    mbh = S.mbh

    def first(y, lvl, t, **kw):  # the row's first MB; coded blocks where a one-MB row needs its pattern
        return pat(S, lvl, t | PAT, **kw) if S.mbw == 1 else MB(t, **kw)

    def rest(lvl, t=0):
        return [pat(S, lvl, t | PAT, skip=S.mbw - 2, **({"mv": {0: _v(0)}} if t else {}))] if S.mbw > 1 else []

    p_rows, b_rows = [], []
    for y in range(mbh):
        if y == 0:
            vy = 16 * f - 1                        # the longest vector downward (half sample)
        elif y == mbh - 1:
            vy = -16 * f                           # the longest upward
        elif y % 128 == 0:
            vy = -49                               # 24.5 lines up: across the boundary above
        elif y % 128 == 127:
            vy = 47                                # 23.5 lines down: across the boundary below
        else:
            vy = (y * 7) % 31 - 15
        p_rows.append(Row([first(y, 5 + y % 5, FWD, mv={0: _v(vy)})] + rest(-4 - y % 3), qcode=4 + y % 8))
        if y >= mbh - 4:
            k = y - (mbh - 4)
            m = first(y, 6 + k, FWD | BWD, field=True,
                      mv={0: _v(-6 - 2 * k, (k & 1, k >> 1)), 1: _v(-3 - 2 * k, (k >> 1, 1 - (k & 1)))})
        else:  # forward from above and backward from below, both from the one side that exists at the ends
            up, down = -((y * 5) % 29 + 2), (y * 3) % 31 + 1
            m = first(y, 4 + y % 6, FWD | BWD, mv={0: _v(up if y else down + 2), 1: _v(down if y < mbh - 1 else up - 3)})
        b_rows.append(Row([m] + rest(5 + y % 4, FWD), qcode=3 + y % 9))
    pics = [tex_pic(S, rng, fpfd=0), Pic(2, p_rows, fcode=((1, long_fc), (15, 15)), fpfd=0),
            Pic(3, b_rows, fcode=((1, long_fc), (1, long_fc)), fpfd=0)]
    return _finish(S, pics)


def wide(name, width, height, hsize):
    """I, P and B with rows of 1024 (1023) MBs.  P: horizontal f_code 9 in its full range, +4095
    down to +4082 in the first columns, a run of more than 990 skipped macroblocks (30 or more
    macroblock_escapes), then -4096 up to -4081 in the last columns.  B: the same range in both
    directions, a wrap below low and one above high under f_code 9 (column 400), a skip run that
    repeats a bidirectional macroblock 391 times and one that repeats a forward macroblock with
    the vector -4090."""
    S = Stream(name, width, height, 1, hsize=hsize)
    rng = _rng(name)
    mbw = S.mbw
    p_rows, b_rows = [], []
    for y in range(S.mbh):
        head = [MB(FWD, mv={0: fr(4095 - k, 0)}) for k in range(14)]
        tail = [MB(FWD, mv={0: fr(-4096 + k, 0)}) for k in range(15)]
        p_rows.append(Row(head + [pat(S, 7 + y, FWD | PAT, skip=mbw - 30, mv={0: fr(-4096, 0)})] + tail[1:] +
                          [pat(S, -6 - y)]))
        head = [MB(FWD | BWD, mv={0: fr(4095 - 2 * k, 0), 1: fr(4094 - 2 * k, 0)}) for k in range(8)]
        head.append(MB(FWD | BWD, mv={0: fr(3, 0), 1: fr(-1 if y == 0 else 1, 0)}))  # the one the skips repeat
        # column 400: -4096, +4095 (8191 above it: a wrap below low), -4090 (a wrap above high)
        mid = [pat(S, 8 - y, BWD | PAT, skip=391, mv={1: fr(-4095, 0)}), MB(FWD, mv={0: fr(-4096, 0)}),
               MB(FWD, mv={0: fr(4095, 0)}), MB(FWD, mv={0: fr(-4090, 0)})]
        tail = [MB(BWD if k % 2 else FWD, mv={k % 2: fr(-4096 + 3 * k, 0)}) for k in range(12)]
        b_rows.append(Row(head + mid + [pat(S, 7 + y, FWD | PAT, skip=mbw - 418, mv={0: fr(-4093, 0)})] +
                          tail + [pat(S, -5 - y, FWD | PAT, mv={0: fr(-4090, 0)})]))
    pics = [tex_pic(S, rng), Pic(2, p_rows, fcode=((9, 1), (15, 15))), Pic(3, b_rows, fcode=((9, 1), (9, 1)))]
    return _finish(S, pics)


def size_ext(name, width, height, hsize=None, vsize=None):
    """an I and a P picture at a size whose extension value no other stream has"""
    S = Stream(name, width, height, 1, hsize=hsize, vsize=vsize)
    rng = _rng(name)
    if S.mbw > 1:
        rows = [skip_row(S, 5 + y % 4) for y in range(S.mbh)]
    else:
        rows = [Row([pat(S, 5 + y % 4, FWD | PAT, mv={0: _v((y * 5) % 9 - 4 if 0 < y < S.mbh - 1 else 0)})])
                for y in range(S.mbh)]
    return _finish(S, [tex_pic(S, rng), Pic(2, rows)])


LIMIT_BUILDERS = [lambda: tall("tall_16384", 16, 16384, 16383, 9), lambda: tall("tall_8192", 32, 8192, 8191, 8),
                  lambda: wide("wide_16384", 16384, 16, 16383), lambda: wide("wide_16368", 16368, 32, 16368),
                  lambda: size_ext("tall_12288", 16, 12288, vsize=12287), lambda: size_ext("wide_4112", 4112, 16),
                  lambda: size_ext("wide_8208", 8208, 16)]
LIMIT_NAMES = ["tall_16384", "tall_8192", "wide_16384", "wide_16368", "tall_12288", "wide_4112", "wide_8208"]


# ---- negative streams ------------------------------------------------------------------------------------------
def neg_vsize_4112():
    """A conforming 16 x 4112 stream: vertical_size 4112 (value 16, extension 1), so every slice
    carries slice_vertical_position_extension.  REFERENCE: it asks the 12-bit value, 16, reads no
    extension and takes the extension's bits for the quantiser code: outside its subset."""
    S = Stream("neg_vsize_4112", 16, 4112, 1)
    S._negative = True
    assert S.vext and S.vsize >> 12 == 1 and S.vsize & 0xFFF == 16
    return _finish(S, [tex_pic(S, _rng(S.name))])


def _neg(name):
    S = Stream(name, 64, 32, 1)
    S._negative = True
    return S, _rng(name)


def neg_row_ends_skipped():
    """a P row whose last coded macroblock is in column mbw - 2: the last one would be skipped"""
    S, rng = _neg("neg_row_ends_skipped")
    rows = [skip_row(S, 8), Row([pat(S, 7), pat(S, -7, skip=1)])]
    return _finish(S, [tex_pic(S, rng), Pic(2, rows)])


def neg_skip_in_i():
    S, rng = _neg("neg_skip_in_i")
    P = tex_pic(S, rng)
    P.rows[1].mbs = [P.rows[1].mbs[0], tex_mb(S, rng, skip=2)]
    return _finish(S, [P])


def neg_cmv_in_p():
    S, rng = _neg("neg_cmv_in_p")
    rows = [Row([tex_mb(S, rng, cmv=(2, 2)) for _ in range(4)]) for _ in range(2)]
    return _finish(S, [tex_pic(S, rng), Pic(2, rows, cmv=1)])


def neg_cmv_in_i():
    """f_code[0] = (3, 5), non-zero concealment vectors and the marker bit in every macroblock of
    two rows of four (the stream the compiled reference crashed on)"""
    S, rng = _neg("neg_cmv_in_i")
    vec = [[(5, -37), (-20, 100), (33, -7), (-1, 64)], [(-60, 3), (2, -200), (63, 255), (-64, -256)]]
    rows = [Row([tex_mb(S, rng, cmv=vec[y][x]) for x in range(4)]) for y in range(2)]
    return _finish(S, [Pic(1, rows, fcode=((3, 5), (15, 15)), cmv=1)])


NEGATIVE = [  # builder, status, reason of the host emitter
    (neg_row_ends_skipped, -2, "slice does not cover the whole macroblock row"),
    (neg_skip_in_i, -2, "skipped macroblock in an I picture"),
    (neg_cmv_in_p, -2, "concealment motion vectors in a P/B picture"),
    (neg_cmv_in_i, -2, "concealment motion vectors in an I picture"),
    (neg_vsize_4112, -2, "vertical_size 4112"),
]

BUILDERS = ([lambda k=k: fcode4(k) for k in range(5)] +
            [lambda: wrap_h("wrap_h_a", (1, 2, 3)), lambda: wrap_h("wrap_h_b", (4, 5, 6)),
             lambda: wrap_h("wrap_h_c", (7, 8)), lambda: wrap_v("wrap_v_a", (1, 2, 3)),
             lambda: wrap_v("wrap_v_b", (4, 5)), mv_seq, skip_runs, mbtypes, lambda: quant(0), lambda: quant(1),
             cbp420, cbp422, cbp444, lambda: dc(0, 2), lambda: dc(1, 3), lambda: dc(2, 2), lambda: dc(3, 3), coefs] +
            [lambda p=p: piclevel(p) for p in range(4)] + [lambda cf=cf: matrices(cf) for cf in (1, 2, 3)] +
            [slice_hdr] + LIMIT_BUILDERS)


def build_all():
    """every directed stream, in a fixed order"""
    return [b() for b in BUILDERS]


def records(S):
    """(mbs, coefs) of a Stream as numpy arrays in the library's record layout (include/mp2vg.h)"""
    dt = np.dtype([("x", "<u2"), ("y", "<u2"), ("flags", "<u2"), ("cbp", "<u2"), ("qscale", "u1"),
                   ("reserved", "u1"), ("ncoef", "<u2"), ("coef_off", "<u4"), ("mv", "<i2", (2, 2, 2))])
    mbs = np.zeros(len(S.mbs), dt)
    for i, m in enumerate(S.mbs):
        for k in ("x", "y", "flags", "cbp", "qscale", "ncoef", "coef_off"):
            mbs[i][k] = m[k]
        mbs[i]["mv"] = m["mv"]
    return mbs, np.array(S.coefs, "<u4")
