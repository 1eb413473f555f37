"""Directed dequantisation / mismatch-control batches (plain Python, no GPU).

model_qfs is parse_block's arithmetic in Python ints, written from include/mp2vg.h's word contract
and ISO 13818-2 7.4 (never by calling the oracle), with named mutants: one plausible kernel
mistake each.  The value cases are found by enumerating the legal domain, the mismatch cases are
built around the values at scan position 63 whose toggle the SSE2 transform can show, and
dequant_batch places every case in every cell of every MB kind: block index, MB position in the
4-MB group, the one-MB trailing group, and word source.  What a finished batch covers is recomputed
from its records by the model (batch_blocks, coverage), never taken from the way the records were chosen.
tests/test_dequant_cpu.py asserts model == oracle, the coverage and that every mutant is seen;
tests/test_gpu_dequant.py decodes the batches against the oracle."""
import numpy as np

import _oracle
from directed import NB, PREFETCH_WORDS, _Builder
from tiny_mp2v_dec_amd._lib import COEF_DC, COEF_FIRST1S, MB_BWD, MB_FWD, MB_INTRA

# scan position -> raster index (row = vertical frequency), ISO 13818-2 figures 7-2 and 7-3
ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20,
          13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52,
          45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]
ALTERNATE = [0, 8, 16, 24, 1, 9, 2, 10, 17, 25, 32, 40, 48, 56, 57, 49, 41, 33, 26, 18, 3, 11, 4, 12, 19, 27,
             34, 42, 50, 58, 35, 43, 51, 59, 20, 28, 5, 13, 6, 14, 21, 29, 36, 44, 52, 60, 37, 45, 53, 61, 22,
             30, 7, 15, 23, 31, 38, 46, 54, 62, 39, 47, 55, 63]
# QFS is stored transposed: position i lands at QFS[column * 8 + row]
QFS_OF_POS = [[(r & 7) * 8 + (r >> 3) for r in t] for t in (ZIGZAG, ALTERNATE)]

# quantiser_scale: the 42 values of the two q_scale_type tables (ISO 13818-2 table 7-6)
QSCALES = sorted(set(range(2, 63, 2)) | set(range(1, 9)) | set(range(10, 25, 2)) | set(range(28, 57, 4)) |
                 set(range(64, 113, 8)))
assert len(QSCALES) == 42

# mutants of one block's arithmetic (model_qfs) ...
BLOCK_MUTANTS = ("floor", "no_int16", "clamp2047", "mul24", "no_mismatch", "dc_in_parity", "parity_unclamped",
                 "ones_clamped", "ones_no_parity", "ones_sign_ignored")
# ... and of where a block's parameters come from (block_context)
CONTEXT_MUTANTS = ("chroma_matrix", "intra_nonintra_matrix", "next_qs", "other_alt", "other_matrices")
MUTANTS = BLOCK_MUTANTS + CONTEXT_MUTANTS
MUTANT_TEXT = {
    "floor": "floor instead of truncation toward zero",
    "no_int16": "clamp without the int16 truncation",
    "clamp2047": "clamp to +-2047",
    "mul24": "signed product reduced mod 2^24 before the shift",
    "no_mismatch": "mismatch control skipped",
    "dc_in_parity": "intra DC counted in the parity",
    "parity_unclamped": "parity of the unclamped values",
    "ones_clamped": "'1s' word clamped",
    "ones_no_parity": "'1s' word left out of the parity",
    "ones_sign_ignored": "'1s' sign ignored",
    "chroma_matrix": "chroma blocks with the other matrix pair",
    "intra_nonintra_matrix": "intra MB of a P/B picture with the non-intra matrix",
    "next_qs": "quantiser scale of the next MB of the group",
    "other_alt": "alternate_scan of the other picture",
    "other_matrices": "matrices of the other picture",
}


def _i16(v):
    return ((v + 32768) & 0xFFFF) - 32768


def dequant_value(level, W, qs, intra, mutant=None):
    """One run-level word: (value stored, int16 value before the clamp).  Intra (|L| W qs) >> 4,
    non-intra ((2 |L| + 1) W qs) >> 5, the sign applied after the shift, int16 truncation, clamp.

    Mutant mul24: the signed product's low 24 bits, zero-extended, are shifted.  (Reducing the
    product of the magnitudes mod 2^24 cannot be seen at all: it moves the shifted value by a
    multiple of 2^20 or 2^19, which the int16 truncation removes; test_dequant_cpu pins that.)"""
    mag = -level if level < 0 else level
    prod = mag * W * qs if intra else (2 * mag + 1) * W * qs
    sh = 4 if intra else 5
    if mutant == "floor":
        val = (-prod if level < 0 else prod) >> sh
    elif mutant == "mul24":
        val = ((-prod if level < 0 else prod) & 0xFFFFFF) >> sh
    else:
        val = prod >> sh
        if level < 0:
            val = -val
    t = val if mutant == "no_int16" else ((val + 32768) & 0xFFFF) - 32768
    lo = -2047 if mutant == "clamp2047" else -2048
    return (lo if t < lo else (2047 if t > 2047 else t)), t


def model_qfs(words, W, qs, intra, alt, mutant=None):
    """QFS[64] (transposed layout) of one block's coefficient words; W: the block's matrix in scan
    order."""
    Q = [0] * 64
    s = 0
    scan = QFS_OF_POS[alt]
    for w in words:
        w = int(w)
        level = ((w & 0xFFFF) ^ 0x8000) - 0x8000
        i = (w >> 16) & 63
        if w & COEF_DC:  # the value as is, outside the sum
            Q[0] = level
            if mutant == "dc_in_parity":
                s += level
            continue
        if w & COEF_FIRST1S:  # (3 W[0] qs) >> 5, int16, sign applied, unclamped, inside the sum
            val = _i16((3 * W[i] * qs) >> 5)
            if mutant == "ones_clamped":
                val = min(val, 2047)
            v = -val if level < 0 and mutant != "ones_sign_ignored" else val
            Q[i] = v
            if mutant != "ones_no_parity":
                s += v
            continue
        v, t = dequant_value(level, W[i], qs, intra, mutant)
        Q[scan[i]] = v
        s += t if mutant == "parity_unclamped" else v
    if mutant != "no_mismatch" and s % 2 == 0:
        Q[63] ^= 1
    return Q


def oracle_qfs(words, W, qs, intra, alt):
    words = np.ascontiguousarray(words, np.uint32)
    Wm = np.ascontiguousarray(W, np.uint8)
    out = np.zeros(64, np.int16)
    _oracle.lib().oracle_dequant_block(_oracle._ptr(words), len(words), _oracle._ptr(Wm), int(qs), int(bool(intra)),
                                       int(alt), _oracle._ptr(out))
    return out.tolist()


_FLAT = np.full(64, 128, np.uint8)


def render(Q, intra):
    """The block's 64 output bytes: put for intra, add onto the flat 128 prediction otherwise."""
    return _oracle.idct(np.array(Q, np.int16), None if intra else _FLAT).tobytes()


def visible_pairs():
    """The (x, x ^ 1) pairs at QFS[63] that the transform's first product can tell apart:
    floor(25570 x / 65536) differs; every other pair gives the same bytes whatever the block."""
    return [(x, x ^ 1) for x in range(-2048, 2048, 2) if (25570 * x) >> 16 != (25570 * (x ^ 1)) >> 16]


# ---------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------
BOUNDARIES = (0, 2047, 32767, 65535, 67583, 98303)  # B | B + 1 of the shifted product
DOMAIN_MAX = {True: (2047 * 255 * 112) >> 4, False: (4095 * 255 * 112) >> 5}
assert DOMAIN_MAX == {True: 3653895, False: 3654787}
ONES_TARGETS = (0, 1, 2047, 2048, 2677)
DC_VALUES = (0, 1, 1023, 1024, 2040, 2047)
V63 = (2, 3, -6, -5, 10, 11, -2048, -2047)
SITUATIONS = {True: ("dc0E", "dc1E", "dc1O", "lane0", "lane1", "lane2", "lane3", "clamp"),
              False: ("E", "lane0", "lane1", "lane2", "lane3", "1s", "clamp")}

_reach = {}


def _reachable(intra):
    """Products below the limit the boundaries need: a (level, W, qs) realising each."""
    if intra in _reach:
        return _reach[intra]
    sh = 4 if intra else 5
    lim = (98304 + 64) << sh
    lev = np.zeros(lim, np.int16)
    wof = np.zeros(lim, np.uint8)
    qof = np.zeros(lim, np.uint8)
    L = np.arange(1, 2048, dtype=np.int64)
    f = (L if intra else 2 * L + 1)[:, None] * np.arange(1, 256, dtype=np.int64)[None, :]
    Lm = np.broadcast_to(L[:, None], f.shape)
    Wm = np.broadcast_to(np.arange(1, 256, dtype=np.int64)[None, :], f.shape)
    for q in [1] + QSCALES[:0:-1]:  # small quantiser scales win, but 1 (the mismatch blocks') only where needed
        p = f * q
        m = p < lim
        lev[p[m]], wof[p[m]], qof[p[m]] = Lm[m], Wm[m], q
    _reach[intra] = (lev, wof, qof)
    return _reach[intra]


class Case:
    def __init__(self, label, kind, intra, **kw):
        self.label, self.kind, self.intra = label, kind, intra
        self.__dict__.update(kw)

    def __repr__(self):
        return self.label


_cases = {}


def value_cases(intra):
    """Per boundary and side the nearest reachable shifted product, with discarded low bits 0, 1
    and all ones where a (level, W, qs) of the domain gives them, both level signs; and the domain
    maximum."""
    lev, wof, qof = _reachable(intra)
    sh = 4 if intra else 5
    mask = (1 << sh) - 1
    ok = (lev > 0)
    vals = np.unique(np.nonzero(ok)[0] >> sh)
    out = []
    for B in BOUNDARIES:
        lo = int(vals[np.searchsorted(vals, B, side="right") - 1]) if B > 0 or vals[0] == 0 else None
        hi = int(vals[np.searchsorted(vals, B + 1, side="left")])
        for side, V in (("lo", lo), ("hi", hi)):
            if V is None:
                continue
            ds = [d for d in (0, 1, mask) if ok[(V << sh) | d]]
            if not ds:
                ds = [int(np.nonzero(ok[V << sh:(V + 1) << sh])[0][0])]
            for d in ds:
                P = (V << sh) | d
                for sg in (1, -1):
                    out.append(Case("value %d|%d %s=%d low=%d %s" % (B, B + 1, side, V, d, "+-"[sg < 0]), "value", intra,
                                    level=sg * int(lev[P]), W=int(wof[P]), qs=int(qof[P]), shifted=V))
    for sg in (1, -1):
        out.append(Case("value domain max %d %s" % (DOMAIN_MAX[intra], "+-"[sg < 0]), "value", intra,
                        level=sg * 2047, W=255, qs=112, shifted=DOMAIN_MAX[intra]))
    return out


def ones_cases():
    """'1s' words whose value is 0, 1, the nearest reachable ones at or below 2047 and at or above
    2048, and the maximum 2677, both signs."""
    best = {}
    for q in QSCALES:
        for W in range(1, 256):
            best.setdefault((3 * W * q) >> 5, (W, q))
    vals = sorted(best)
    assert vals[-1] == 2677
    out = []
    for tgt in ONES_TARGETS:
        v = max(x for x in vals if x <= tgt) if tgt != 2048 else min(x for x in vals if x >= tgt)
        W, q = best[v]
        for sg in (1, -1):
            out.append(Case("1s target %d value %d %s" % (tgt, v, "+-"[sg < 0]), "ones", False, level=sg, W=W, qs=q,
                            value=v))
    return out


def cases(intra):
    """The whole case list of intra (True) or non-intra (False) blocks."""
    if intra in _cases:
        return _cases[intra]
    out = value_cases(intra)
    if intra:
        out += [Case("dc %d" % v, "dc", True, dc=v, qs=None) for v in DC_VALUES]
    else:
        out += ones_cases()
    for v in V63 + (None,):
        for sit in SITUATIONS[intra] if v is not None else SITUATIONS[intra][:1] + ("lane0",):
            out.append(Case("mismatch v63=%s %s" % (v, sit), "mm", intra, v63=v, sit=sit, qs=None))
    for i, c in enumerate(out):
        c.index = i
    _cases[intra] = out
    return out


_levels = {}


def level_of_value(v, W, qs, intra):
    """level_for an exact value, remembered."""
    k = (v, W, qs, intra)
    if k not in _levels:
        _levels[k] = level_for(lambda t: t == v, W, qs, intra)
    return _levels[k]


def level_for(want, W, qs, intra):
    """A positive level whose dequantised value before the clamp satisfies want(t), or None."""
    for L in range(1, 2048):
        if want(dequant_value(L, W, qs, intra)[1]):
            return L
    return None


# The default matrix entry of a picture's row r is ROW_W[(picture + r) % 3] and the picture's mismatch
# blocks use quantiser scale MM_QS, so W * qs is just above 16: small values are mostly reachable (a
# mismatch case whose values a row cannot give waits for another picture; 2047 non-intra needs 17),
# and values above 2047 exist for the clamp.  Rows r, r ^ 1 and r ^ 2 always differ.
ROW_W = (17, 18, 20)
MM_QS = 1


# ---------------------------------------------------------------------------------------------
# the batch builder
# ---------------------------------------------------------------------------------------------
LOW = list(range(1, 13))      # value cases: low-frequency scan positions, matrix entry set per case
MID = list(range(13, 63))     # carriers and parity makers: the picture row's default entry
PAD_QS = (22, 24)  # no case needs them
KINDS = {"I": ("intra I",), "P": ("intra P", "inter P"), "B": ("intra B", "inter B"), "mixed": ("inter mixed",)}
VALUE_MUTANTS = ("floor", "no_int16", "clamp2047", "mul24")


def block_row(b, intra):
    """The quantiser matrix of block b: blocks 0-5 the luma pair, 6-11 the chroma pair."""
    return (0 if b < 6 else 2) + (0 if intra else 1)


class _Placer:
    """One batch under construction: pictures with per-row matrices (a default entry from
    ROW_W, entries of the value cases' positions set when first used and then frozen)."""

    def __init__(self, width, height, cf, launch, seed):
        self.B = _Builder(width, height, cf, seed)
        self.cf, self.launch = cf, launch
        self.rng = np.random.default_rng(seed)
        self.W = []       # per picture: int array [4][64]
        self.frozen = []  # per picture: [4] dicts pos -> W
        self.kinds = KINDS[launch]
        self.fails = {}
        self.needs = {}
        cells = ([("b", b) for b in range(self.B.nb)] + [("k", k) for k in range(4 + (self.B.mbw % 4 != 0))] +
                 [("src", "prefetch"), ("src", "second")])
        for kind in self.kinds:
            self.needs[kind] = [set(cells) for _ in cases(kind.startswith("intra"))]
        self.T = PREFETCH_WORDS["I" if launch == "I" else "P"][cf]

    # -- pictures
    def picture(self, ptype, fwd=-1, bwd=-1, flat=False):
        p = self.B.picture(ptype, fwd, bwd)
        W = np.zeros((4, 64), np.int64)
        for r in range(4):
            W[r] = 16 if flat else ROW_W[(p + r) % 3]
        self.W.append(W)
        self.frozen.append([{} for _ in range(4)])
        return p

    def alloc(self, p, r, Wc, positions):
        """A position of row r whose entry is, or can be set to, Wc while the other rows differ."""
        for pos in positions:
            if self.can_alloc(p, r, Wc, pos):
                self.W[p][r][pos] = Wc
                self.frozen[p][r][pos] = Wc
                return pos
        return None

    def can_alloc(self, p, r, Wc, pos):
        fz = self.frozen[p][r].get(pos)
        others = (r ^ 2,) if pos == 0 else (r ^ 1, r ^ 2)  # ('1s' words exist in non-intra blocks only)
        return (fz is None or fz == Wc) and all(self.W[p][o][pos] != Wc for o in others)

    def read(self, p, r, pos):
        self.frozen[p][r].setdefault(pos, int(self.W[p][r][pos]))
        return int(self.W[p][r][pos])

    # -- blocks
    def carriers(self, p, r, qs, intra, n, even, avoid):
        """n companion words at mid positions, |value| <= 60 where the matrix allows (even values
        only for the mismatch blocks, so the parity situation stays as built)."""
        out = []
        for pos in self.rng.choice([q for q in MID if q not in avoid], n, replace=False).tolist():
            W = self.read(p, r, pos)
            tv = int(self.rng.integers(4, 31)) * 2 if even else int(self.rng.integers(8, 61))
            L = level_for(lambda t: t >= tv and (not even or t % 2 == 0), W, qs, intra) or 1
            if even and dequant_value(L, W, qs, intra)[0] % 2:
                continue
            out.append((int(self.rng.choice([-1, 1])) * L, pos, 0))
        return out

    def block(self, case, p, b, qs, intra, alt):
        """The words [(level, position, flags)] of `case` in block b of picture p, or None when the
        picture cannot hold it (a matrix entry taken, the row's quantiser scale another one)."""
        r = block_row(b, intra)
        Wrow = self.W[p][r]
        base = [(1024, 0, COEF_DC)] if intra else []
        if case.kind == "value":
            if case.qs != qs:
                return None
            # the position too is tried: at some, a large value saturates inside the transform
            for pos in LOW:
                if not self.can_alloc(p, r, case.W, pos):
                    continue
                Wtry = Wrow.copy()
                Wtry[pos] = case.W
                core = base + [(case.level, pos, 0)]
                for _ in range(6):
                    ws = core + self.carriers(p, r, qs, intra, int(self.rng.integers(2, 4)), False, {0, pos})
                    if self.shows(ws, Wtry, qs, intra, alt, "value"):
                        assert self.alloc(p, r, case.W, [pos]) == pos
                        return sorted(ws, key=lambda t: (t[1], -t[2]))
            return None
        if case.kind == "ones":
            if case.qs != qs or not self.can_alloc(p, r, case.W, 0):
                return None
            Wtry = Wrow.copy()
            Wtry[0] = case.W
            core, even, check = [(case.level, 0, COEF_FIRST1S)], False, "value"
            if case.value > 1000:  # alone it saturates every pixel: a large wave brings some back into range
                pos = (1, 8)[b & 1]
                L = level_for(lambda t: t >= 1500, self.read(p, r, pos), qs, intra)
                core.append((-L if case.level > 0 else L, pos, 0))
        elif case.kind == "dc":
            Wtry = Wrow
            core, even, check = [(case.dc, 0, COEF_DC)], False, None
        else:
            if qs != MM_QS:
                return None
            Wtry = Wrow
            core = self.mismatch_core(case, p, r, qs, intra, alt)
            if core is None:
                return None
            even, check = True, ("toggle" if case.v63 is not None else None)
        avoid = {pos for _, pos, _ in core}
        for _ in range(24):
            ws = core + self.carriers(p, r, qs, intra, int(self.rng.integers(2, 4)), even, avoid)
            if check is None or self.shows(ws, Wtry, qs, intra, alt, check):
                if case.kind == "ones":
                    assert self.alloc(p, r, case.W, [0]) == 0
                return sorted(ws, key=lambda t: (t[1], -t[2]))
        return None

    def shows(self, ws, W, qs, intra, alt, check):
        words = [_pack(l, pos, 0, fl) for l, pos, fl in ws]
        Q = model_qfs(words, W, qs, intra, alt)
        out = render(Q, intra)
        if check == "toggle":
            Q2 = list(Q)
            Q2[63] ^= 1
            return render(Q2, intra) != out
        for m in VALUE_MUTANTS + ("ones_clamped", "ones_sign_ignored"):
            Qm = model_qfs(words, W, qs, intra, alt, m)
            if Qm != Q and render(Qm, intra) == out:
                return False
        return True

    def mismatch_core(self, case, p, r, qs, intra, alt):
        W = self.read(p, r, 63)  # the row's default entry, as at every mid position

        def word(value, pos):
            if value == -2048:
                L = level_for(lambda t: t >= 2048, W, qs, intra)
            else:
                L = level_of_value(abs(value), W, qs, intra)
            return None if L is None else (-L if value < 0 else L, pos, 0)

        def lane_pos(j, taken):
            for pos in MID:
                if QFS_OF_POS[alt][pos] >> 4 == j and pos not in taken:
                    return pos

        sit, core = case.sit, []
        if intra:
            core.append((1023 if sit.startswith("dc1") else 1024, 0, COEF_DC))
        if sit == "1s":
            if 0 not in self.frozen[p][r] and p % 2 == 0:
                return None  # even pictures keep the row's entry 0 for the '1s' value cases
            if (3 * self.read(p, r, 0) * qs) >> 5 & 1 == 0:
                return None
            core.append((int(self.rng.choice([-1, 1])), 0, COEF_FIRST1S))
        if sit.startswith("lane") or sit == "dc1O":
            j = int(sit[4]) if sit.startswith("lane") else int(self.rng.integers(4))
            pos = lane_pos(j, ())
            self.read(p, r, pos)
            core.append(next(w for w in (word(v * int(self.rng.choice([-1, 1])), pos) for v in (3, 5, 1, 7)) if w))
        if sit == "clamp":  # an even value above 2047 that the clamp makes 2047
            pos = int(self.rng.choice(MID))
            self.read(p, r, pos)
            L = level_for(lambda t: t >= 2048 and t % 2 == 0, W, qs, intra)
            assert L is not None
            core.append((L, pos, 0))
        if case.v63 is not None:
            core.append(word(case.v63, 63))
        return None if None in core else core


def _pack(level, pos, b, fl):
    return (level & 0xFFFF) | (pos << 16) | (b << 22) | fl


def _pad_blocks(P, intra):
    """A pad MB: every block 64 words of level +-1 (so later MBs' words come from the second loop)."""
    out = {}
    for b in range(P.B.nb):
        ws = [(1024, 0, COEF_DC)] if intra else []
        ws += [(int(P.rng.choice([-1, 1])), pos, 0) for pos in range(1 if intra else 0, 64)]
        out[b] = ws
    return out


class DequantBatch:
    def __init__(self, width, height, cf, launch, pics, mbs, coefs, first_case_pic):
        self.width, self.height, self.cf, self.launch = width, height, cf, launch
        self.pics, self.mbs, self.coefs = pics, mbs, coefs
        self.first_case_pic = first_case_pic
        self._blocks = None

    def key(self):
        return ("dequant", self.width, self.height, self.cf, self.launch)


_batches = {}
MAX_PICTURES = 160
# the flat anchor's DC: the reference transform renders 1025..1032 as 128 everywhere (1024 as 127)
ANCHOR_DC = 1028


def dequant_batch(width, height, cf, launch, seed=4100):
    """launch I: I pictures.  P: a flat I anchor, then P pictures (zero vector) holding intra and
    non-intra MBs.  B: flat I and P anchors, then two-direction B pictures (intra and bidirectional
    MBs).  mixed: the anchors, then backward-only and two-direction B pictures in turn (one mixed
    launch).  Consecutive pictures alternate alternate_scan and rotate their matrices; the four
    MBs of a group have four quantiser scales; a third of the full groups (drawn) start with two pad MBs of 64
    words per block and one MB of a group is kept for the mismatch blocks, its position moving from
    group to group.  MBs are filled until every case of the launch's MB kinds has been in every
    block index, every MB position of the group (and the one-MB trailing group of an 80-wide row)
    and both word sources; a case that no MB can hold fails the build."""
    ck = (width, height, cf, launch, seed)
    if ck in _batches:
        return _batches[ck]
    P = _Placer(width, height, cf, launch, seed + 100 * cf + width + height + sum(map(ord, launch)))
    B = P.B
    mbw, mbh, nb = B.mbw, B.mbh, B.nb
    zero = np.zeros((2, 2, 2), np.int16)
    if launch != "I":
        P.picture(1, flat=True)
        for _ in range(mbw * mbh):
            B.mb(MB_INTRA, {b: [(ANCHOR_DC, 0, COEF_DC)] for b in range(nb)}, 2)
    if launch in ("B", "mixed"):
        P.picture(2, 0, flat=True)
        for _ in range(mbw * mbh):
            B.mb(MB_FWD, {}, 2, zero)
    first = len(B.pics)
    gcount = 0
    while any(n for kind in P.kinds for n in P.needs[kind]):
        assert len(B.pics) < MAX_PICTURES, ("cases that no MB can hold", launch,
                                            [(k, cases(k.startswith("intra"))[i], n) for k in P.kinds
                                             for i, n in enumerate(P.needs[k]) if n][-8:])
        if launch == "I":
            p = P.picture(1)
        elif launch == "P":
            p = P.picture(2, 0)
        else:
            p = P.picture(3, 0 if launch == "B" or len(B.pics) % 2 else -1, 1)
        P.fails.clear()  # what a picture could not hold, the next may
        one_dir = launch == "mixed" and B.pics[p][1] < 0
        alt = p & 1
        # a P or B picture keeps its launch mode through one non-intra MB at least
        forced = int(P.rng.integers(mbw * mbh)) if len(P.kinds) > 1 else -1
        for y in range(mbh):
            for g0 in range(0, mbw, 4):
                nmb = min(4, mbw - g0)
                pad = 2 if nmb == 4 and P.rng.random() < 1 / 3 else 0
                # the MB kept for the mismatch blocks (and the other cases of their quantiser scale): the
                # position most of them still need, drawn among equals (a fixed rotation can stay in
                # step with the matrices' rotation)
                want = [sum(("k", k) in n for kd in P.kinds for c, n in zip(cases(kd.startswith("intra")), P.needs[kd])
                            if c.qs in (None, MM_QS)) + P.rng.random() for k in range(pad, 4)]
                mmslot = pad + int(np.argmax(want))
                gcount += 1
                used, gwords = set(PAD_QS[:pad]), 0
                for k in range(nmb):
                    kappa = k if nmb == 4 else 4
                    open_kinds = [kd for kd in P.kinds if any(P.needs[kd])] or list(P.kinds)
                    kind = open_kinds[int(P.rng.integers(len(open_kinds)))]
                    if B.k == forced:
                        kind = P.kinds[1]
                    intra = kind.startswith("intra")
                    flags = MB_INTRA if intra else (MB_FWD if launch == "P" else (MB_BWD if one_dir else MB_FWD | MB_BWD))
                    if k < pad:
                        blocks, qs = _pad_blocks(P, intra), PAD_QS[k]
                    else:
                        blocks, qs = _fill_mb(P, kind, intra, p, alt, kappa, used, gwords, nmb < 4 or k == mmslot)
                    used.add(qs)
                    gwords += sum(len(v) for v in blocks.values())
                    B.mb(flags, blocks, qs, None if intra else zero)
    pics, mbs, coefs = B.finish()
    for p in range(len(pics)):
        pics[p]["W"] = P.W[p]
        pics[p]["alternate_scan"] = p & 1
    _batches[ck] = DequantBatch(width, height, cf, launch, pics, mbs, coefs, first)
    return _batches[ck]


def _fill_mb(P, kind, intra, p, alt, kappa, used, gwords, mm_ok):
    """One case MB: the quantiser scale of the neediest case that fits the group, then per block
    the case that gains most cells."""
    cs, needs, nb = cases(intra), P.needs[kind], P.B.nb
    desig = {MM_QS}
    mm_pending = any(needs[i] for i in range(len(cs)) if cs[i].kind == "mm")

    def qs_options(c):
        if c.kind == "mm":
            return sorted(desig) if mm_ok else []
        if c.kind == "dc":
            return [16, 12, 28, 30, 26]
        # one MB of a group is kept for the mismatch blocks, and with it the rows' quantiser scales
        return [c.qs] if mm_ok or not mm_pending or c.qs not in desig else []

    src0 = ("src", "second" if gwords >= P.T else "prefetch")

    def score(i):
        return -4 * P.fails.get((kind, i), 0) + len(needs[i]) + 10 * (("k", kappa) in needs[i]) + 10 * (src0 in needs[i]) + 100 * (mm_ok and cs[i].kind == "mm" and bool(needs[i]))

    order = sorted(range(len(cs)), key=lambda i: -score(i))
    qs = None
    here = {("b", b) for b in range(nb)} | {("k", kappa), src0, ("src", "second")}
    for i in order:
        if not needs[i] & here:  # nothing this MB could give it: its quantiser scale stays free for a later MB
            continue
        for q in qs_options(cs[i]):
            if q not in used and q not in PAD_QS:
                qs = q
                break
        if qs is not None:
            break
    if qs is None:
        qs = next(q for q in (16, 12, 28, 30, 26) if q not in used)
    cand = [i for i in order if cs[i].kind == "dc" or cs[i].qs == qs or (cs[i].kind == "mm" and qs in desig)]
    blocks = {}
    lead, placed = next((i for i in order if needs[i] & here), order[0]), set()
    for b in range(nb):
        ws = None
        cells = {("b", b), ("k", kappa), ("src", "second" if gwords >= P.T else "prefetch")}
        for i in sorted(cand, key=lambda i: -len(needs[i] & cells)):
            if not intra and not needs[i] & cells:
                break  # nothing to gain: a non-intra block may stay uncoded
            ws = P.block(cs[i], p, b, qs, intra, alt)
            if ws is not None:
                placed.add(i)
                if gwords < P.T < gwords + len(ws):  # the block straddles the two word sources
                    cells = {("b", b), ("k", kappa)}
                needs[i] -= cells
                break
        if ws is None:
            if not intra:
                continue
            ws = [(1024, 0, COEF_DC)]
        blocks[b] = ws
        gwords += len(ws)
    if lead not in placed:
        P.fails[(kind, lead)] = P.fails.get((kind, lead), 0) + 1
    return blocks, qs


# ---------------------------------------------------------------------------------------------
# what a finished batch holds, from its records
# ---------------------------------------------------------------------------------------------
def mb_kind(batch, p, i):
    t = int(batch.pics[p]["picture_coding_type"])
    if int(batch.mbs["flags"][i]) & MB_INTRA:
        return "intra " + "IPB"[t - 1]
    return "inter " + ("P" if t == 2 else ("mixed" if batch.launch == "mixed" else "B"))


def partner(batch, p):
    """The other picture of the launch that a wrong picture index would take."""
    n = len(batch.pics)
    return p + 1 if p + 1 < n else p - 1


def block_context(batch, p, i, b, mutant=None):
    """(W, qs, intra, alt) of block b of MB record i of picture p, as the records say, or as a
    context mutant would take them."""
    pics, mbs = batch.pics, batch.mbs
    intra = bool(int(mbs["flags"][i]) & MB_INTRA)
    row = block_row(b, intra)
    src = p
    alt = int(pics[p]["alternate_scan"])
    qs = int(mbs["qscale"][i])
    if mutant == "chroma_matrix" and b >= 4:
        row ^= 2
    elif mutant == "intra_nonintra_matrix" and intra and int(pics[p]["picture_coding_type"]) != 1:
        row += 1
    elif mutant == "next_qs":
        mbw = batch.width // 16
        x = int(mbs["x"][i])
        g0 = x & ~3
        n = min(4, mbw - g0)
        qs = int(mbs["qscale"][i - x + g0 + (x - g0 + 1) % n])
    elif mutant == "other_alt":
        alt = int(pics[partner(batch, p)]["alternate_scan"])
    elif mutant == "other_matrices":
        src = partner(batch, p)
    return pics[src]["W"][row].tolist(), qs, intra, alt


def classify(words, W, qs, intra, alt):
    """The case labels a block realises, from its words and parameters alone (batch_blocks asks for
    blocks of fewer than 16 words only: the pad MBs' full blocks are no cases).  A mismatch
    situation is recognised only in its built form: the rest of the sum even with no odd
    coefficient at all, or odd through exactly one odd coefficient (laneN: its pass-1 lane; the
    non-intra 'rest odd' situations exist only as these), or through the '1s' word alone, or
    through the one coefficient whose parity the clamp changed."""
    labels = set()
    table = _case_table(intra)
    v63, dc, ones, rest = None, None, None, []
    for w in words:
        level = ((w & 0xFFFF) ^ 0x8000) - 0x8000
        i = (w >> 16) & 63
        if w & COEF_DC:
            dc = level
            if ("dc", level) in table:
                labels.add(table[("dc", level)])
        elif w & COEF_FIRST1S:
            ones = _i16((3 * W[i] * qs) >> 5) * (-1 if level < 0 else 1)
            if ("ones", abs(ones), level < 0) in table:
                labels.add(table[("ones", abs(ones), level < 0)])
        else:
            key = ("value", level, W[i], qs)
            if key in table:
                labels.add(table[key])
            v, t = dequant_value(level, W[i], qs, intra)
            if i == 63:
                v63 = v
            else:
                rest.append((v, t, QFS_OF_POS[alt][i] >> 4))
    if not rest and ones is None:
        return labels, v63
    changed = [x for x in rest if (x[0] ^ x[1]) & 1]
    odd = [x for x in rest if x[0] & 1]
    sit = None
    if changed:
        if len(changed) == 1 and odd == changed and ones is None and not (dc or 0) & 1:
            sit = "clamp"
    elif ones is not None:
        if ones & 1 and not odd:
            sit = "1s"
    elif not odd:
        sit = ("dc1E" if dc & 1 else "dc0E") if intra else "E"
    elif len(odd) == 1:
        sit = "dc1O" if intra and dc & 1 else "lane%d" % odd[0][2]
    if sit is not None and ("mm", v63, sit) in table:
        labels.add(table[("mm", v63, sit)])
    return labels, v63


_tables = {}


def _case_table(intra):
    if intra not in _tables:
        t = {}
        for c in cases(intra):
            if c.kind == "value":
                t[("value", c.level, c.W, c.qs)] = c.label
            elif c.kind == "ones":
                t[("ones", c.value, c.level < 0)] = c.label
            elif c.kind == "dc":
                t[("dc", c.dc)] = c.label
            else:
                t[("mm", c.v63, c.sit)] = c.label
        _tables[intra] = t
    return _tables[intra]


class Block:
    __slots__ = ("p", "mb", "b", "kind", "k", "src", "words", "labels", "v63", "Q", "toggled", "x", "y", "intra")


def batch_blocks(batch):
    """Every coded block of the case pictures: its cell (MB kind, block index, MB position k in the
    group, 4 = the one-MB trailing group, word source), the model's QFS and its case labels."""
    if batch._blocks is not None:
        return batch._blocks
    pics, mbs, coefs = batch.pics, batch.mbs, batch.coefs
    mbw, mbh = batch.width // 16, batch.height // 16
    T = PREFETCH_WORDS["I" if batch.launch == "I" else "P"][batch.cf]
    out = []
    cl = coefs.tolist()
    for p in range(batch.first_case_pic, len(pics)):
        first = int(pics[p]["mb_first"])
        for y in range(mbh):
            for g0 in range(0, mbw, 4):
                n = min(4, mbw - g0)
                i0 = first + y * mbw + g0
                gstart = int(mbs["coef_off"][i0])
                for i in range(i0, i0 + n):
                    off, nc = int(mbs["coef_off"][i]), int(mbs["ncoef"][i])
                    ws = cl[off:off + nc]
                    j = 0
                    while j < nc:
                        b = (ws[j] >> 22) & 15
                        e = j
                        while e < nc and (ws[e] >> 22) & 15 == b:
                            e += 1
                        bl = Block()
                        bl.p, bl.mb, bl.b, bl.words = p, i, b, ws[j:e]
                        bl.x, bl.y = g0 + i - i0, y
                        bl.kind = mb_kind(batch, p, i)
                        bl.k = i - i0 if n == 4 else 4
                        a, z = off + j - gstart, off + e - 1 - gstart
                        bl.src = "second" if a >= T else ("prefetch" if z < T else "straddle")
                        W, qs, intra, alt = block_context(batch, p, i, b)
                        bl.intra = intra
                        bl.Q = model_qfs(bl.words, W, qs, intra, alt)
                        bl.toggled = bl.Q != model_qfs(bl.words, W, qs, intra, alt, "no_mismatch")
                        bl.labels, bl.v63 = classify(bl.words, W, qs, intra, alt) if e - j < 16 else (set(), None)
                        out.append(bl)
                        j = e
    batch._blocks = out
    return out


def block_cells(bl):
    return [("b", bl.b), ("k", bl.k)] + ([("src", bl.src)] if bl.src != "straddle" else [])


def coverage(batch):
    """{MB kind: {cell: set of case labels present}}."""
    cov = {}
    for bl in batch_blocks(batch):
        c = cov.setdefault(bl.kind, {})
        for cell in block_cells(bl):
            c.setdefault(cell, set()).update(bl.labels)
    return cov


def expected_cells(batch):
    nb = NB[batch.cf]
    return ([("b", b) for b in range(nb)] + [("k", k) for k in range(4 + ((batch.width // 16) % 4 != 0))] +
            [("src", "prefetch"), ("src", "second")])


def coverage_table(batch, cov):
    lines = ["%-12s %-16s %s" % ("MB kind", "cell", "cases present")]
    for kind in KINDS[batch.launch]:
        total = len(cases(kind.startswith("intra")))
        for cell in expected_cells(batch):
            lines.append("%-12s %-16s %4d/%d" % (kind, "%s %s" % cell, len(cov.get(kind, {}).get(cell, ())), total))
    return "\n".join(lines)


def mutant_applies(m, kind, cell):
    intra = kind.startswith("intra")
    if m == "dc_in_parity" and not intra:
        return False
    if m.startswith("ones_") and intra:
        return False
    if m == "intra_nonintra_matrix" and (not intra or kind == "intra I"):
        return False
    if m == "chroma_matrix" and cell[0] == "b" and cell[1] < 4:
        return False
    if m == "next_qs" and cell == ("k", 4):
        return False
    return True


def mutant_kills(batch):
    """{(mutant, MB kind, cell): blocks whose output bytes the mutant changes}; a mutant is only
    evaluated on blocks that still have a cell it has not been seen in."""
    kills = {}
    for kind in KINDS[batch.launch]:
        for cell in expected_cells(batch):
            for m in MUTANTS:
                if mutant_applies(m, kind, cell):
                    kills[(m, kind, cell)] = 0
    for bl in batch_blocks(batch):
        cells = block_cells(bl)
        out = None
        for m in MUTANTS:
            keys = [(m, bl.kind, c) for c in cells if (m, bl.kind, c) in kills]
            if not keys or all(kills[k] for k in keys):
                continue
            if m == "chroma_matrix" and bl.b < 4:
                continue
            if m in BLOCK_MUTANTS:
                W, qs, intra, alt = block_context(batch, bl.p, bl.mb, bl.b)
                Qm = model_qfs(bl.words, W, qs, intra, alt, m)
            else:
                W, qs, intra, alt = block_context(batch, bl.p, bl.mb, bl.b, m)
                Qm = model_qfs(bl.words, W, qs, intra, alt)
            if Qm == bl.Q:
                continue
            if out is None:
                out = render(bl.Q, bl.intra)
            if render(Qm, bl.intra) != out:
                for k in keys:
                    kills[k] += 1
    return kills


def visible_toggles(blocks):
    """Blocks whose mismatch toggle happened, and those of them whose output it changed."""
    toggled = seen = 0
    vis = []
    for bl in blocks:
        if not bl.toggled:
            continue
        toggled += 1
        Q2 = list(bl.Q)
        Q2[63] ^= 1
        if render(Q2, bl.intra) != render(bl.Q, bl.intra):
            seen += 1
            vis.append(bl)
    return toggled, seen, vis


def block_origin(cf, b):
    """(plane, x, y) of block b inside its MB (frame DCT)."""
    if b < 4:
        return 0, (b & 1) * 8, (b >> 1) * 8
    k = (b - 4) >> 1
    return 1 + (b & 1), (8 if k >= 2 else 0), (8 if k in (1, 3) else 0)
