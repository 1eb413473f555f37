"""Directed record batches (plain Python, no GPU): textured anchors, a motion-vector sweep that
enumerates the tap's address / phase space and its edge contacts, and batches whose 4-MB groups
carry exact coefficient-word counts.  Everything is deterministic from a seed; the coverage a
batch achieves is recomputed from its finished records (sweep_coverage, group_totals), never taken
from the way the records were chosen.  tests/test_directed_cpu.py asserts the coverage,
tests/test_gpu_directed.py decodes the batches against the oracle.  The same builders at the
geometry limits (16384 wide or high), the vertical long-vector batch, the tap sweep at the far
corner and the sparse 16384 x 16384 frame are decoded by tests/test_gpu_limits.py."""
import numpy as np

from test_gpu_parity import _P, _inside  # noqa: F401  (_P re-exported for the directed tests)
from tiny_mp2v_dec_amd import records as R
from tiny_mp2v_dec_amd._lib import (COEF_DC, MB_BWD, MB_DCT_FIELD, MB_FIELD_MC, MB_FWD, MB_INTRA, coef_pack,
                                    mb_fs_bit)

NB = {1: 6, 2: 8, 3: 12}

# tap modes: which loop of the kernel applies the vector, and as which tap (recon.hip issue_pass)
TAP_MODES = ("P picture fwd", "P-loop B fwd-only", "P-loop B bwd-only", "B-loop fwd-only MB",
             "B-loop bwd-only MB", "B-loop bidir fwd tap", "B-loop bidir bwd tap")
MC_TYPES = ("frame", "field r0 fs0", "field r0 fs1", "field r1 fs0", "field r1 fs1")
KEYS = [(t, c) for t in range(len(TAP_MODES)) for c in range(len(MC_TYPES))]


def key_name(key):
    return "%s / %s" % (TAP_MODES[key[0]], MC_TYPES[key[1]])


def _mc_type(field, r, fs):
    return 1 + 2 * r + fs if field else 0


def plane_dims(width, height, cf):
    """Plane sizes and the MB's size in each plane."""
    pw = [width] + [width if cf == 3 else width // 2] * 2
    ph = [height] + [height if cf != 1 else height // 2] * 2
    bw = [16] + [16 if cf == 3 else 8] * 2
    bh = [16] + [8 if cf == 1 else 16] * 2
    return pw, ph, bw, bh


def tap_rect(width, height, cf, plane, mbx, mby, mvx, mvy, field, fs):
    """The reference pixels one vector reads in one plane, with the formulas of _inside:
    (x0, x1, y0, y1, hx, hy); field MC reads every second row from y0 to y1."""
    pw, ph, bw, bh = plane_dims(width, height, cf)
    mx, my = mvx, mvy
    if plane:
        if cf < 3:
            mx >>= 1
        if cf < 2:
            my >>= 1
    w, h = bw[plane], bh[plane]
    x0 = mbx * w + (mx >> 1)
    x1 = x0 + w - 1 + (mx & 1)
    if not field:
        y0 = mby * h + (my >> 1)
        y1 = y0 + h - 1 + (my & 1)
    else:
        y0 = mby * h + fs + 2 * (my >> 1)
        y1 = y0 + 2 * (h // 2 - 1) + 2 * (my & 1)
    return x0, x1, y0, y1, mx & 1, my & 1


def tap_contacts(width, height, cf, plane, mbx, mby, mvx, mvy, field, fs):
    """Edge contacts of one tap in one plane: L/R/T/B + the half-pel flag of that axis.  A field
    tap's top and bottom are the first and last row of its field (rows fs and ph - 2 + fs)."""
    pw, ph, _, _ = plane_dims(width, height, cf)
    x0, x1, y0, y1, hx, hy = tap_rect(width, height, cf, plane, mbx, mby, mvx, mvy, field, fs)
    out = set()
    if x0 == 0:
        out.add("L%d" % hx)
    if x1 == pw[plane] - 1:
        out.add("R%d" % hx)
    if y0 == (fs if field else 0):
        out.add("T%d" % hy)
    if y1 == (ph[plane] - 2 + fs if field else ph[plane] - 1):
        out.add("B%d" % hy)
    return out


class _Builder:
    """Collects pictures, MB records and coefficient words; every picture's MBs in raster order."""

    def __init__(self, width, height, cf, seed):
        self.width, self.height, self.cf = width, height, cf
        self.mbw, self.mbh, self.nb = width // 16, height // 16, NB[cf]
        self.rng = np.random.default_rng(seed)
        self.pics, self.mbs, self.coefs = [], [], []
        self.k = 0

    def picture(self, ptype, fwd=-1, bwd=-1, qmat=16):
        if self.pics:
            assert self.k == self.mbw * self.mbh
        self.pics.append((ptype, fwd, bwd, len(self.mbs), qmat))
        self.k = 0
        return len(self.pics) - 1

    def pos(self):
        return self.k % self.mbw, self.k // self.mbw

    def mb(self, flags, blocks, qscale, mv=None):
        """blocks: {block index: [(level, scan position, word flags), ...]}"""
        x, y = self.pos()
        off = len(self.coefs)
        cbp = 0
        for b in sorted(blocks):
            cbp |= 1 << b
            for lvl, pos, fl in blocks[b]:
                self.coefs.append(coef_pack(lvl, pos, b, fl, x))
        self.mbs.append((x, y, flags, cbp, qscale, len(self.coefs) - off, off, mv))
        self.k += 1

    def finish(self):
        assert self.k == self.mbw * self.mbh
        pics = np.zeros(len(self.pics), R.PIC_DTYPE)
        for p, (ptype, fwd, bwd, first, qmat) in enumerate(self.pics):
            pics[p]["dst_slot"], pics[p]["fwd_slot"], pics[p]["bwd_slot"] = p, fwd, bwd
            pics[p]["picture_coding_type"] = ptype
            pics[p]["mb_first"], pics[p]["mb_width"], pics[p]["mb_height"] = first, self.mbw, self.mbh
            pics[p]["W"] = qmat
        mbs = np.zeros(len(self.mbs), R.MB_DTYPE)
        for i, (x, y, flags, cbp, qscale, ncoef, off, mv) in enumerate(self.mbs):
            m = mbs[i]
            m["x"], m["y"], m["flags"], m["cbp"], m["qscale"] = x, y, flags, cbp, qscale
            m["ncoef"], m["coef_off"] = ncoef, off
            if mv is not None:
                m["mv"] = mv
        return pics, mbs, np.array(self.coefs, dtype=np.uint32)

    # -- textured anchors: every block coded, W = 16, qscale 2, DC 480..1567, 12 AC words at
    # distinct scan positions with |level| 1..8 (a P anchor carries the same AC recipe as residual)
    def textured_blocks(self, intra):
        out = {}
        for b in range(self.nb):
            ws = [(int(self.rng.integers(480, 1568)), 0, COEF_DC)] if intra else []
            for pos in sorted(self.rng.choice(np.arange(1, 64), 12, replace=False).tolist()):
                ws.append((int(self.rng.choice([-1, 1])) * int(self.rng.integers(1, 9)), int(pos), 0))
            out[b] = ws
        return out

    def textured_i_picture(self):
        p = self.picture(1)
        for _ in range(self.mbw * self.mbh):
            self.mb(MB_INTRA, self.textured_blocks(True), 2)
        return p

    def half_pel_vector(self):
        """A small vector with both components odd that keeps this MB's reads inside (in a picture
        one MB wide or high, where no odd component is legal on that axis, that component is 0)."""
        x, y = self.pos()
        odd = (-3, -1, 1, 3)
        c = [(a, b) for a in (odd if self.mbw > 1 else (0,)) for b in (odd if self.mbh > 1 else (0,))
             if _inside(self.width, self.height, self.cf, x, y, a, b, False, 0)]
        return c[int(self.rng.integers(len(c)))]

    def textured_p_picture(self, fwd):
        p = self.picture(2, fwd)
        for _ in range(self.mbw * self.mbh):
            mv = np.zeros((2, 2, 2), np.int16)
            mv[0, 0] = self.half_pel_vector()
            self.mb(MB_FWD, self.textured_blocks(False), 2, mv)
        return p

    def textured_picture_np(self, ptype, fwd=-1):
        """textured_i_picture (ptype 1) or textured_p_picture (ptype 2) for pictures of thousands of
        MBs: the same recipe with the words of every block drawn at once in numpy (other random
        numbers than the per-MB builders draw)."""
        p = self.picture(ptype, fwd)
        n, nb, intra, rng = self.mbw * self.mbh, self.nb, ptype == 1, self.rng
        pos = np.sort(np.argsort(rng.random((n, nb, 63)), axis=2)[:, :, :12] + 1, axis=2)  # distinct, 1..63
        lvl = rng.integers(1, 9, (n, nb, 12)) * rng.choice([-1, 1], (n, nb, 12))
        col = ((np.arange(n) % self.mbw) & 7) << 26  # coef_pack's column bits
        blk = np.arange(nb) << 22
        words = (lvl & 0xFFFF) | pos << 16 | blk[None, :, None] | col[:, None, None]
        if intra:
            dc = rng.integers(480, 1568, (n, nb)) | blk[None, :] | col[:, None] | COEF_DC
            words = np.concatenate([dc[:, :, None], words], axis=2)
        per, off = words.shape[1] * words.shape[2], len(self.coefs)
        self.coefs.extend(words.reshape(-1).tolist())
        for k in range(n):
            x, y = self.pos()
            mv = None
            if not intra:
                mv = np.zeros((2, 2, 2), np.int16)
                mv[0, 0] = self.half_pel_vector()
            self.mbs.append((x, y, MB_INTRA if intra else MB_FWD, (1 << nb) - 1, 2, per, off + k * per, mv))
            self.k += 1
        return p

    def small_residual(self):
        """A few words per coded block, |level| <= 3: (2 * 3 + 1) * 16 * 2 >> 5 = 7 at most."""
        out = {}
        for b in range(self.nb):
            if b and self.rng.random() < 0.5:
                continue
            out[b] = [(int(self.rng.choice([-1, 1])) * int(self.rng.integers(1, 4)), int(pos), 0)
                      for pos in sorted(self.rng.choice(64, 3, replace=False).tolist())]
        return out


def row_width_batch(width, height, cf):
    """random_batch (every record feature, field MC, saturating levels) at a directed row width."""
    from test_gpu_parity import random_batch
    return random_batch(width, height, cf, 5, seed=3300 + cf + width, field=True, big=True)


_frames = {}


def expected_frames(key, width, height, cf, pics, mbs, coefs):
    """The oracle's frames of a directed batch, computed once per key and shared by the tests
    (read-only)."""
    if key not in _frames:
        from helpers import oracle_frames
        _frames[key] = oracle_frames(_P(width, height, cf, pics, mbs, coefs))
    return _frames[key]


def split_batch(pics, mbs, coefs, k):
    """The batch as two batches, pictures [0, k) and [k, n), the second rebased to its own arrays."""
    m0 = int(pics["mb_first"][k])
    c0 = int(mbs["coef_off"][m0])
    p2 = pics[k:].copy()
    p2["mb_first"] -= m0
    m2 = mbs[m0:].copy()
    m2["coef_off"] -= c0
    return (pics[:k], mbs[:m0], coefs[:c0]), (p2, m2, coefs[c0:])


# ---------------------------------------------------------------------------------------------
# motion-vector sweep
# ---------------------------------------------------------------------------------------------
def sweep_vector_residues(n):
    """Vector n of 64: (mvx mod 32, mvy mod 32).  The 64 vectors realise every (mvx mod 32,
    mvy & 1) pair and every (mvy mod 32, mvx & 1) pair."""
    return n & 31, 2 * ((n >> 1) & 15) + (n >> 5)


def _first_legal(cands, ok):
    for v in cands:
        if ok(v):
            return v
    return None


def _key_jobs(width, height, field):
    """The vectors one coverage key must hold: [((column or None, row or None), fn)], fn(mbx,
    mby, ok_x, ok_y) -> vector or None; ok_x / ok_y tell whether a component keeps the MB's reads
    inside (the two axes are independent in _inside)."""
    mbw, mbh = width // 16, height // 16
    jobs = []

    def exact(where, fn):
        jobs.append((where, lambda x, y, okx, oky: fn(x, y)))

    # corners: the zero vector, and the longest legal vector towards the opposite corner
    for cx in (0, mbw - 1):
        for cy in (0, mbh - 1):
            lx = 2 * (width - 16) * (1 if cx == 0 else -1) if mbw > 1 else 0
            ly = (height - 16) * (1 if field else 2) * (1 if cy == 0 else -1) if mbh > 1 else 0
            exact((cx, cy), lambda x, y: (0, 0))
            exact((cx, cy), lambda x, y, v=(lx, ly): v)
    # the last column with mvx = -1 and the last row with mvy = -1: right / bottom edge contact with
    # half-pel, in chroma too where chroma is subsampled ((-1) >> 1 = -1)
    exact((mbw - 1, None), lambda x, y: (-1, 0))
    exact((None, mbh - 1), lambda x, y: (0, -1))
    # edge contacts from anywhere: first column 0, last column pw - 1, first row, last row (of the
    # field for field MC), each with and without the half-pel flag of that axis
    vs = 1 if field else 2  # vertical units per pixel row of the MB grid
    for hp in (0, 1):
        exact((None, None), lambda x, y, hp=hp: (-32 * x + hp, 0))
        exact((None, None), lambda x, y, hp=hp: (2 * (width - 16 - 16 * x) - hp, 0))
        exact((None, None), lambda x, y, hp=hp: (0, -16 * vs * y + hp))
        exact((None, None), lambda x, y, hp=hp: (0, vs * (height - 16 - 16 * y) - hp))
    # the chroma >> 1 cases
    for v in ((-1, -1), (-1, -3), (-3, -1), (-3, -3)):
        exact((None, None), lambda x, y, v=v: v)
    # the 64 residue vectors, preferred signs alternating; the nearest legal one is taken
    for n in range(64):
        rx, ry = sweep_vector_residues(n)
        sx, sy = (1 if n & 2 else -1), (1 if n & 4 else -1)

        def fn(x, y, okx, oky, rx=rx, ry=ry, sx=sx, sy=sy):
            def order(r, s):
                return sorted((r + 32 * k for k in range(-70, 70)), key=lambda v: (v * s <= 0, abs(v)))
            vx = _first_legal(order(rx, sx), okx)
            vy = _first_legal(order(ry, sy), oky)
            return None if vx is None or vy is None else (vx, vy)
        jobs.append(((None, None), fn))
    return jobs


class _Sweep:
    def __init__(self, width, height, cf, seed):
        self.B = _Builder(width, height, cf, seed)
        self.jobs = {(t, c): _key_jobs(width, height, c != 0) for t, c in KEYS}

    def pending(self, modes):
        return sum(len(self.jobs[(t, c)]) for t in modes for c in range(len(MC_TYPES)))

    @staticmethod
    def templates(taps):
        """taps: [(direction s, tap mode)] of the MB kind.  Frame MC, and field MC with every
        combination of field selects: (field, fs bits, [(r, s, key)])."""
        out = [(False, 0, [(0, s, (t, 0)) for s, t in taps])]
        rs = [(r, s, t) for r in range(2) for s, t in taps]
        for bits in range(1 << len(rs)):
            fsb, tp = 0, []
            for i, (r, s, t) in enumerate(rs):
                fs = bits >> i & 1
                fsb |= mb_fs_bit(r, s) if fs else 0
                tp.append((r, s, (t, _mc_type(True, r, fs))))
            out.append((True, fsb, tp))
        return out

    def _score(self, key, x, y):
        sc = 0
        for where, _ in self.jobs[key]:
            if where[0] in (None, x) and where[1] in (None, y):
                sc += 1 + 100 * (where[0] is not None) + 100 * (where[1] is not None)
        return sc

    def _take(self, key, x, y, field, fs):
        B = self.B

        def okx(v):
            return _inside(B.width, B.height, B.cf, x, y, v, 0, field, fs)

        def oky(v):
            return _inside(B.width, B.height, B.cf, x, y, 0, v, field, fs)
        best = None
        for i, (where, fn) in enumerate(self.jobs[key]):
            if where[0] not in (None, x) or where[1] not in (None, y):
                continue
            rank = (where[0] is None) + (where[1] is None)
            if best is not None and rank >= best[0]:
                continue
            v = fn(x, y, okx, oky)
            if v is None or not okx(v[0]) or not oky(v[1]):
                continue
            best = (rank, i, v)
        if best is None:
            return (0, 0)  # nothing left for this key here: the zero vector
        del self.jobs[key][best[1]]
        return best[2]

    def mb(self, dirs, taps, textured=False):
        """One sweep MB of a kind (direction flags, [(s, tap mode)])."""
        B = self.B
        x, y = B.pos()
        tmpl = max(self.templates(taps), key=lambda tp: sum(self._score(k, x, y) for _, _, k in tp[2]))
        field, fsb, tp = tmpl
        mv = np.zeros((2, 2, 2), np.int16)
        for r, s, key in tp:
            mv[r, s] = self._take(key, x, y, field, (fsb >> (8 + 2 * r + s)) & 1)
        flags = dirs | fsb | (MB_FIELD_MC if field else 0)
        if textured:
            B.mb(flags, B.textured_blocks(False), 2, mv)
        elif B.k % 4 == 3:  # every fourth MB: a small residual, field DCT where the format allows
            if B.cf != 3 and (B.k // 4) % 2 == 0:
                flags |= MB_DCT_FIELD
            B.mb(flags, B.small_residual(), 2, mv)
        else:
            B.mb(flags, {}, 2, mv)


class SweepBatch:
    """mc_sweep's result: the records, the index of the first two-direction B picture (pictures
    before it need only picture 0 and 1 decoded), and the coverage recomputed from the records."""

    def __init__(self, width, height, cf, pics, mbs, coefs, first_two_dir):
        self.width, self.height, self.cf = width, height, cf
        self.pics, self.mbs, self.coefs = pics, mbs, coefs
        self.first_two_dir = first_two_dir
        self.coverage = sweep_coverage(width, height, cf, pics, mbs)

    def parsed(self):
        return _P(self.width, self.height, self.cf, self.pics, self.mbs, self.coefs)


_KINDS = {"P": (MB_FWD, [(0, 0)]), "BF": (MB_FWD, [(0, 1)]), "BB": (MB_BWD, [(1, 2)]),
          "F": (MB_FWD, [(0, 3)]), "K": (MB_BWD, [(1, 4)]), "D": (MB_FWD | MB_BWD, [(0, 5), (1, 6)])}
_sweeps = {}


def mc_sweep(width, height, cf, seed=2024):
    """Picture 0: textured I.  Picture 1: textured P from picture 0, the first picture of the P
    sweep.  Then P pictures from picture 0, forward-only B pictures from picture 0 and
    backward-only B pictures from picture 1 (the P loop), and two-direction B pictures (forward 0,
    backward 1) whose MBs are forward-only, backward-only and bidirectional in turn.  The vectors
    are enumerated per coverage key (tap mode, MC type): see _key_jobs."""
    ck = (width, height, cf, seed)
    if ck in _sweeps:
        return _sweeps[ck]
    S = _Sweep(width, height, cf, seed + cf)
    B = S.B
    n = B.mbw * B.mbh
    B.textured_i_picture()
    for kind, ptype, fwd, bwd in (("P", 2, 0, -1), ("BF", 3, 0, -1), ("BB", 3, -1, 1)):
        dirs, taps = _KINDS[kind]
        modes = [t for _, t in taps]
        while S.pending(modes) or len(B.pics) == 1:
            assert len(B.pics) < 400, "sweep jobs that no MB can hold"
            B.picture(ptype, fwd, bwd)
            for _ in range(n):
                S.mb(dirs, taps, textured=len(B.pics) == 2)
    first_two_dir = len(B.pics)
    while S.pending([3, 4, 5, 6]):
        assert len(B.pics) < 400, "sweep jobs that no MB can hold"
        p = B.picture(3, 0, 1)
        for k in range(n):
            S.mb(*_KINDS["FKD"[(k + p) % 3]])
    pics, mbs, coefs = B.finish()
    _sweeps[ck] = SweepBatch(width, height, cf, pics, mbs, coefs, first_two_dir)
    return _sweeps[ck]


def picture_uses(pics, mbs, p):
    """(forward used, backward used) over the picture's non-intra MBs, as the planner counts it."""
    first = int(pics[p]["mb_first"])
    fl = mbs["flags"][first:first + int(pics[p]["mb_width"]) * int(pics[p]["mb_height"])].astype(np.int64)
    inter = (fl & MB_INTRA) == 0
    return (bool((inter & (((fl & MB_FWD) != 0) | ((fl & MB_BWD) == 0))).any()),
            bool((inter & ((fl & MB_BWD) != 0)).any()))


def mb_taps(pics, mbs, p, i):
    """The vectors MB record i of picture p applies: [(key, r, s, mvx, mvy, field, fs)]."""
    m = mbs[i]
    fl = int(m["flags"])
    if fl & MB_INTRA:
        return []
    fwd, bwd = bool(fl & MB_FWD) or not fl & MB_BWD, bool(fl & MB_BWD)
    uf, ub = picture_uses(pics, mbs, p)
    field = bool(fl & MB_FIELD_MC)
    out = []
    for r in range(2 if field else 1):
        for s in range(2):
            if not (fwd, bwd)[s]:
                continue
            if int(pics[p]["picture_coding_type"]) == 2:
                t = 0
            elif not (uf and ub):
                t = 1 + s
            else:
                t = 5 + s if fwd and bwd else 3 + s
            fs = (fl >> (8 + 2 * r + s)) & 1
            out.append(((t, _mc_type(field, r, fs)), r, s, int(m["mv"][r, s, 0]), int(m["mv"][r, s, 1]), field, fs))
    return out


def sweep_coverage(width, height, cf, pics, mbs, window=None):
    """Per coverage key, from the records alone: the (mvx mod 32, mvy & 1) and (mvy mod 32,
    mvx & 1) pairs, the signs of each component, the vectors, and the edge contacts per plane.
    window = (first MB column, first MB row): only the MBs from there to the far corner count."""
    cov = {k: dict(xphase=set(), yphase=set(), sx=set(), sy=set(), vecs=set(), contacts=set(),
                   corners=set()) for k in KEYS}
    mbw, mbh = width // 16, height // 16
    for p in range(len(pics)):
        first = int(pics[p]["mb_first"])
        for i in range(first, first + mbw * mbh):
            x, y = int(mbs["x"][i]), int(mbs["y"][i])
            if window is not None and (x < window[0] or y < window[1]):
                continue
            for key, r, s, vx, vy, field, fs in mb_taps(pics, mbs, p, i):
                c = cov[key]
                c["xphase"].add((vx % 32, vy & 1))
                c["yphase"].add((vy % 32, vx & 1))
                c["sx"].add((vx > 0) - (vx < 0))
                c["sy"].add((vy > 0) - (vy < 0))
                c["vecs"].add((vx, vy))
                for plane in range(3):
                    for name in tap_contacts(width, height, cf, plane, x, y, vx, vy, field, fs):
                        c["contacts"].add((plane, name))
                if x in (0, mbw - 1) and y in (0, mbh - 1):
                    # zero, or the longest vector towards the opposite corner: it touches the two
                    # opposite luma edges
                    far = {"R0" if x == 0 else "L0", "B0" if y == 0 else "T0"}
                    if (vx, vy) == (0, 0):
                        c["corners"].add((x, y, "zero"))
                    if far <= tap_contacts(width, height, cf, 0, x, y, vx, vy, field, fs):
                        c["corners"].add((x, y, "far"))
                if x == mbw - 1 and vx == -1:
                    c["corners"].add("last column mvx -1")
                if y == mbh - 1 and vy == -1:
                    c["corners"].add("last row mvy -1")
    return cov


def coverage_table(cov):
    """The table the CPU test prints: one line per key."""
    lines = ["%-22s %-13s %7s %7s %s" % ("tap mode", "MC type", "x-phase", "y-phase", "luma contacts")]
    for k in KEYS:
        c = cov[k]
        lines.append("%-22s %-13s %4d/64 %4d/64 %s" % (TAP_MODES[k[0]], MC_TYPES[k[1]], len(c["xphase"]),
                                                        len(c["yphase"]),
                                                        " ".join(sorted(n for pl, n in c["contacts"] if pl == 0))))
    return "\n".join(lines)


# ---------------------------------------------------------------------------------------------
# exact coefficient-word counts per 4-MB group
# ---------------------------------------------------------------------------------------------
# recon.hip recon_kernel: a group's first 64 * NCW words come from the prefetch registers (NCW = 8 /
# 12 / 24 in the I kernel for 4:2:0 / 4:2:2 / 4:4:4, 2 in the P/B kernels), words beyond from a
# second loop in rounds of 64 * XW (XW = 8 in the I kernel, 2 in the P/B kernels)
PREFETCH_WORDS = {"I": {1: 512, 2: 768, 3: 1536}, "P": {1: 128, 2: 128, 3: 128}, "B": {1: 128, 2: 128, 3: 128}}
ROUND_WORDS = {"I": 512, "P": 128, "B": 128}


def required_totals(cf, kind):
    """Group totals a word_count_batch must hold in its full (4-MB) groups."""
    T, Rr = PREFETCH_WORDS[kind][cf], ROUND_WORDS[kind]
    out = [T - 1, T, T + 1, T + 63, T + 64, T + 65, T + Rr - 1, T + Rr, T + Rr + 1, 4 * NB[cf] * 64]
    return out + ([0, 1, 63, 64, 65] if kind != "I" else [])


def required_trailing_totals(cf, kind):
    """Totals of the one-MB trailing group of an 80-wide row: 0, 1, 64 and NB * 64.  An intra MB
    codes every block (a DC word each), so the I kind's smallest totals are NB, NB + 1, NB + 64."""
    nb = NB[cf]
    return [nb, nb + 1, nb + 64, nb * 64] if kind == "I" else [0, 1, 64, nb * 64]


def _group_blocks(B, nmb, intra, total, start):
    """Words of a group of nmb MBs: every intra block gets its DC word, then blocks are filled
    from scan position 0 upward (a full block is 64 words), MB by MB starting at MB `start`, until
    the group holds `total` words.  Returns one {block: words} per MB."""
    nb = B.nb
    blocks = [{b: [(int(B.rng.integers(480, 1568)), 0, COEF_DC)] for b in range(nb)} if intra[m] else {}
              for m in range(nmb)]
    left = total - nb * sum(intra)
    assert 0 <= left <= sum((63 if intra[m] else 64) * nb for m in range(nmb)), (total, intra)
    for m in [(start + j) % nmb for j in range(nmb)]:
        for b in range(nb):
            lo = 1 if intra[m] else 0
            take = min(left, 64 - lo)
            if take == 0:
                break
            blocks[m].setdefault(b, []).extend(
                (int(B.rng.choice([-2, -1, 1, 2])), pos, 0) for pos in range(lo, lo + take))
            left -= take
    assert left == 0
    return blocks


_word_batches = {}


def word_count_batch(width, height, cf, kind, seed=77):
    """I: I pictures.  P: a textured I picture, then P pictures predicted from it.  B: textured I
    and P anchors, then two-direction B pictures.  Every full group's word total is one of
    required_totals (P/B: some of them again with an intra MB in the group), every one-MB
    trailing group's (width % 64 == 16) one of required_trailing_totals; W = 16, qscale 1,
    |level| <= 2.  Returns (pics, mbs, coefs)."""
    ck = (width, height, cf, kind, seed)
    if ck in _word_batches:
        return _word_batches[ck]
    B = _Builder(width, height, cf, seed + 10 * cf + ord(kind))
    mbw, mbh, nb = B.mbw, B.mbh, B.nb
    T, Rr = PREFETCH_WORDS[kind][cf], ROUND_WORDS[kind]
    full = [(t, None) for t in required_totals(cf, kind)]
    if kind != "I":  # groups that hold an intra MB (MB j of the group)
        full += [(t, j % 4) for j, t in enumerate((T - 1, T, T + 1, T + Rr, T + Rr + 1, 4 * nb * 64, 64, 65))]
    trail = [(t, None) for t in required_trailing_totals(cf, kind)]
    if kind != "I":
        trail += [(nb, 0), (nb * 64, 0)]
    if mbw % 4 == 0:
        trail = []
    assert mbw % 4 in (0, 1)
    if kind != "I":
        B.textured_i_picture()
    if kind == "B":
        B.textured_p_picture(0)
    gi = 0
    while full or trail:
        if kind == "I":
            B.picture(1)
        else:
            B.picture(2 if kind == "P" else 3, 0, 1 if kind == "B" else -1)
        for _ in range(mbh):
            for g0 in range(0, mbw, 4):
                nmb = min(4, mbw - g0)
                todo = full if nmb == 4 else trail
                total, im = todo.pop(0) if todo else ((nb * nmb if kind == "I" else 0), None)
                intra = [kind == "I" or m == im for m in range(nmb)]
                for m, blocks in enumerate(_group_blocks(B, nmb, intra, total, gi % nmb)):
                    if intra[m]:
                        B.mb(MB_INTRA, blocks, 1)
                        continue
                    mv = np.zeros((2, 2, 2), np.int16)
                    mv[0, 0], mv[0, 1] = B.half_pel_vector(), B.half_pel_vector()
                    dirs = MB_FWD if kind == "P" else (MB_FWD | MB_BWD, MB_FWD, MB_BWD)[B.k % 3]
                    B.mb(dirs, blocks, 1, mv)
                gi += 1
    _word_batches[ck] = B.finish()
    return _word_batches[ck]


def group_totals(width, height, pics, mbs, p):
    """Coefficient words of every 4-MB group of picture p, from the records: [(MBs in the group,
    total, the group holds an intra MB)] in raster order (groups never straddle rows here)."""
    mbw, mbh = width // 16, height // 16
    first = int(pics[p]["mb_first"])
    out = []
    for y in range(mbh):
        for g0 in range(0, mbw, 4):
            sl = slice(first + y * mbw + g0, first + y * mbw + min(g0 + 4, mbw))
            out.append((sl.stop - sl.start, int(mbs["ncoef"][sl].sum()),
                        bool((mbs["flags"][sl] & MB_INTRA).any())))
    return out


# ---------------------------------------------------------------------------------------------
# long vectors
# ---------------------------------------------------------------------------------------------
def long_vector_batch(width, height, cf, seed=909):
    """A wide, two-MB-row picture set (1040x32): textured I and P anchors, a P picture and a
    two-direction B picture whose horizontal vectors step from +(2 * (width - 16) - 1) in column 0
    to the negative of that in the last column (+-2047 at 1040: the range of f_code 9).  Row 0 is
    frame MC, row 1 field MC; the B picture's MBs are bidirectional (the backward vector the
    longest the column allows, left and right in turn) with every third one forward-only or
    backward-only."""
    B = _Builder(width, height, cf, seed + cf)
    mbw, mbh = B.mbw, B.mbh
    assert mbh == 2 and mbw > 1
    far = 2 * (width - 16) - 1

    def mvx(c):
        return far - (2 * far * c + (mbw - 1) // 2) // (mbw - 1)

    def vectors(x, y, field, flags):
        mv = np.zeros((2, 2, 2), np.int16)
        for r in range(2 if field else 1):
            for s in range(2):
                # backward: the longest vector of the column, to column 0 and to the last column
                # (with half-pel) in turn
                vx = mvx(x) if s == 0 else (-32 * x if x % 2 == 0 else 2 * (width - 16 - 16 * x) - 1)
                fs = (flags >> (8 + 2 * r + s)) & 1
                vy = _first_legal([(3, 1, -1, -3)[(x + r + s + j) % 4] for j in range(4)] + [0],
                                  lambda v: _inside(width, height, cf, x, y, 0, v, field, fs))
                assert _inside(width, height, cf, x, y, vx, vy, field, fs), (x, y, vx, vy)
                mv[r, s] = (vx, vy)
        return mv

    if mbw * mbh > 1024:  # (the per-MB anchors take seconds there)
        B.textured_picture_np(1)
        B.textured_picture_np(2, 0)
    else:
        B.textured_i_picture()
        B.textured_p_picture(0)
    for ptype in (2, 3):
        B.picture(ptype, 0, 1 if ptype == 3 else -1)
        for k in range(mbw * mbh):
            x, y = B.pos()
            field = y == 1
            flags = (MB_FIELD_MC | (k * 5 % 16) << 8) if field else 0
            flags |= MB_FWD if ptype == 2 else (MB_FWD | MB_BWD, MB_FWD | MB_BWD, MB_FWD, MB_FWD | MB_BWD,
                                                MB_FWD | MB_BWD, MB_BWD)[k % 6]
            B.mb(flags, B.small_residual() if k % 4 == 3 else {}, 2, vectors(x, y, field, flags))
    return B.finish()


def long_vertical_far(height, field):
    """The longest legal vertical vector with half-pel: from MB row 0 to the last MB row, in frame
    half-pels (frame MC) or field half-pels (field MC)."""
    return (2 if not field else 1) * (height - 16) - 1


_vertical = {}


def long_vertical_batch(width, height, cf, seed=919):
    """The vertical twin of long_vector_batch, on a narrow and tall picture: textured I and P
    anchors (pictures 0 and 1), then a P picture from picture 0, a forward-only B picture from
    picture 0, a backward-only B picture from picture 1 (both through the P loop) and a
    two-direction B picture whose MBs are bidirectional, forward-only and backward-only in turn.
    The first vector of an MB in row y steps from +long_vertical_far in row 0 to the negative of
    that in the last row; the other direction of a bidirectional MB is the longest vector of its
    row, to row 0 and to the last row (with half-pel) in turn.  MBs alternate between frame MC and
    field MC like a chessboard, the field MBs running through all four (r0, r1) field selects per
    direction every eight rows.  Every fourth MB carries a small residual."""
    ck = (width, height, cf, seed)
    if ck in _vertical:
        return _vertical[ck]
    B = _Builder(width, height, cf, seed + cf)
    mbw, mbh = B.mbw, B.mbh
    assert mbh > 48 and mbw > 1

    def towards_zero(v, ok):
        """v, or the nearest vector towards zero that keeps the reads inside."""
        while v and not ok(v):
            v -= 1 if v > 0 else -1
        return v

    def vectors(x, y, field, flags):
        far = long_vertical_far(height, field)
        unit = 1 if field else 2
        mv = np.zeros((2, 2, 2), np.int16)
        for r in range(2 if field else 1):
            for s in range(2):
                first = s == 0 if flags & MB_FWD else s == 1  # the direction that carries the stepped vector
                if first:
                    vy = far - (2 * far * y + (mbh - 1) // 2) // (mbh - 1)
                else:
                    vy = -16 * unit * y if (x + y // 2) % 2 == 0 else unit * (height - 16 - 16 * y) - 1
                fs = (flags >> (8 + 2 * r + s)) & 1
                vy = towards_zero(vy, lambda v: _inside(width, height, cf, x, y, 0, v, field, fs))
                vx = _first_legal([(3, 1, -1, -3)[(y + r + s + j) % 4] for j in range(4)] + [0],
                                  lambda v: _inside(width, height, cf, x, y, v, 0, field, fs))
                assert _inside(width, height, cf, x, y, vx, vy, field, fs), (x, y, vx, vy)
                mv[r, s] = (vx, vy)
        return mv

    B.textured_picture_np(1)
    B.textured_picture_np(2, 0)
    for ptype, fwd, bwd, kinds in ((2, 0, -1, (MB_FWD,)), (3, 0, -1, (MB_FWD,)), (3, -1, 1, (MB_BWD,)),
                                   (3, 0, 1, (MB_FWD | MB_BWD, MB_FWD, MB_BWD))):
        B.picture(ptype, fwd, bwd)
        for k in range(mbw * mbh):
            x, y = B.pos()
            field = (x + y) % 2 == 1
            flags = kinds[(x + y // 2) % len(kinds)]
            if field:  # field selects (r0, r1): forward combination y // 2 mod 4, backward the next one
                a, b = (y // 2) % 4, (y // 2 + 1) % 4
                flags |= MB_FIELD_MC
                flags |= (mb_fs_bit(0, 0) if a & 1 else 0) | (mb_fs_bit(1, 0) if a & 2 else 0)
                flags |= (mb_fs_bit(0, 1) if b & 1 else 0) | (mb_fs_bit(1, 1) if b & 2 else 0)
            B.mb(flags, B.small_residual() if k % 4 == 3 else {}, 2, vectors(x, y, field, flags))
    _vertical[ck] = B.finish()
    return _vertical[ck]


def long_vertical_coverage(width, height, pics, mbs):
    """Per coverage key, from the records alone: (the largest mvy, the smallest mvy) over the MBs
    that apply a vector of that key; keys that no MB holds are missing."""
    mbw, mbh = width // 16, height // 16
    out = {}
    for p in range(len(pics)):
        first = int(pics[p]["mb_first"])
        for i in range(first, first + mbw * mbh):
            for key, r, s, vx, vy, field, fs in mb_taps(pics, mbs, p, i):
                hi, lo = out.get(key, (vy, vy))
                out[key] = (max(hi, vy), min(lo, vy))
    return out


# ---------------------------------------------------------------------------------------------
# a frame of zero-vector MBs with a few hundred directed ones
# ---------------------------------------------------------------------------------------------
def sparse_frame_batch(width, height, cf, seed=16384):
    """Records of a P picture (slot 2, forward slot 0) and a two-direction B picture (slot 3,
    forward slot 0, backward slot 1), built in numpy for frames of a million MBs: every MB
    predicts with the zero vector and no residual, except the directed ones -- the 8 x 8 MBs of
    each corner and every fourth MB of the last MB row (the last luma tile bands).  A directed MB
    draws its vectors over the whole legal range (its taps land anywhere in the reference, the end
    of the last plane included), frame or field MC, P: forward, B: bidirectional, forward or
    backward, with a small residual on every second one; MB (0, 0) and the last MB take the longest
    vector towards the opposite corner.  Returns (pics, mbs, coefs, the directed MBs' record
    indices per picture)."""
    mbw, mbh, nb = width // 16, height // 16, NB[cf]
    assert mbw >= 20 and mbh >= 16
    n = mbw * mbh
    rng = np.random.default_rng(seed)
    pics = np.zeros(2, R.PIC_DTYPE)
    pics["dst_slot"], pics["fwd_slot"], pics["bwd_slot"] = [2, 3], [0, 0], [-1, 1]
    pics["picture_coding_type"], pics["mb_first"] = [2, 3], [0, n]
    pics["mb_width"], pics["mb_height"], pics["W"] = mbw, mbh, 16
    mbs = np.zeros(2 * n, R.MB_DTYPE)
    mbs["x"], mbs["y"] = np.tile(np.arange(mbw), 2 * mbh), np.tile(np.repeat(np.arange(mbh), mbw), 2)
    mbs["flags"][:n], mbs["flags"][n:], mbs["qscale"] = MB_FWD, MB_FWD | MB_BWD, 2
    ex, ey = list(range(8)) + list(range(mbw - 8, mbw)), list(range(8)) + list(range(mbh - 8, mbh))
    where = [(x, y) for y in ey for x in ex] + [(x, mbh - 1) for x in range(10, mbw - 8, 4)]
    where.sort(key=lambda xy: (xy[1], xy[0]))  # raster order: the words follow their MBs
    coefs, ncoef, directed = [], np.zeros(2 * n, np.int64), []
    for p in range(2):
        directed.append(np.array([p * n + y * mbw + x for x, y in where]))
        for j, (x, y) in enumerate(where):
            i = p * n + y * mbw + x
            field = bool(rng.integers(0, 3) == 0) and (x, y) not in ((0, 0), (mbw - 1, mbh - 1))
            flags = MB_FWD if p == 0 else (MB_FWD | MB_BWD, MB_FWD, MB_BWD)[j % 3]
            if field:
                flags |= MB_FIELD_MC | int(rng.integers(0, 16)) << 8
            vs = 1 if field else 2
            for r in range(2 if field else 1):
                for s in range(2):
                    fs = 1 if flags & mb_fs_bit(r, s) else 0
                    vx = int(rng.integers(-32 * x, 2 * (width - 16 - 16 * x) + 1))
                    vy = int(rng.integers(-16 * vs * y, vs * (height - 16 - 16 * y) + 1))
                    if (x, y) == (0, 0):
                        vx, vy = 2 * (width - 16) - 1, vs * (height - 16) - 1
                    if (x, y) == (mbw - 1, mbh - 1):
                        vx, vy = -2 * (width - 16), -vs * (height - 16)
                    assert _inside(width, height, cf, x, y, vx, vy, field, fs), (x, y, vx, vy, field, fs)
                    mbs["mv"][i, r, s] = (vx, vy)
            mbs["flags"][i] = flags
            if j % 2:
                cbp = 0
                for b in sorted(rng.choice(nb, 4, replace=False).tolist()):
                    cbp |= 1 << b
                    for pos in sorted(rng.choice(64, 3, replace=False).tolist()):
                        coefs.append(coef_pack(int(rng.choice([-3, -2, -1, 1, 2, 3])), int(pos), b, 0, x))
                        ncoef[i] += 1
                mbs["cbp"][i] = cbp
    mbs["ncoef"] = ncoef
    mbs["coef_off"] = np.cumsum(ncoef) - ncoef
    return pics, mbs, np.array(coefs, np.uint32), directed


def textured_bytes(rng, n):
    """n full-range bytes: 8 MiB + 13 seeded bytes, repeated (seconds faster than n random bytes
    for a slot of 768 MiB; the period is no multiple of any row, tile or plane size)."""
    return np.resize(np.frombuffer(rng.bytes(min(n, (8 << 20) + 13)), np.uint8), n)


def sparse_frame_expected(exp, pics, mbs, coefs, directed):
    """Slots 2 and 3 of exp (a helpers.SlotOracle whose slots 0 and 1 hold the references) after
    sparse_frame_batch.  The zero-vector MBs come from their definition, whole slots at a time:
    the forward reference's bytes in the P picture, (forward + backward + 1) >> 1 in the B picture
    (as a | b - ((a ^ b) >> 1), which stays in uint8).  The directed MBs are then decoded by the
    oracle, as pictures that hold those MB records alone (the oracle places an MB by its x and y)."""
    sb = int(exp.g.slot_bytes)
    a, b = exp.pool[:sb], exp.pool[sb:2 * sb]
    exp.pool[2 * sb:3 * sb] = a
    avg = exp.pool[3 * sb:4 * sb]
    np.bitwise_or(a, b, out=avg)
    avg -= (a ^ b) >> 1
    sub = pics.copy()
    sub["mb_first"] = [0, len(directed[0])]
    sub["mb_width"], sub["mb_height"] = len(directed[0]), 1
    exp.decode(sub, np.concatenate([mbs[directed[0]], mbs[directed[1]]]), coefs)


# ---------------------------------------------------------------------------------------------
# the tap sweep at the far corner of a large picture
# ---------------------------------------------------------------------------------------------
_corner = {}


def corner_sweep(width, height, cf, sw, sh):
    """mc_sweep(sw, sh) embedded at the far corner of a width x height picture: the MB records of
    the small sweep, moved by (width - sw, height - sh) with their vectors, flags and words as they
    are, so every tap of the sweep reads the same place of its window, now at the largest tile
    columns (or bands) of the large reference, and the sweep's right and bottom edge contacts are
    the large picture's.  Outside the window the two anchors are textured over the whole plane
    (textured_picture_np's recipe) and every other picture predicts with the zero vector in its
    own directions, without residual.  Returns a SweepBatch (its coverage: the window's)."""
    ck = (width, height, cf, sw, sh)
    if ck in _corner:
        return _corner[ck]
    s = mc_sweep(sw, sh, cf)
    mbw, mbh, smw, smh = width // 16, height // 16, sw // 16, sh // 16
    x0, y0 = mbw - smw, mbh - smh
    assert x0 % 8 == 0  # the words carry their MB's column mod 8
    n, sn = mbw * mbh, smw * smh
    T = _Builder(width, height, cf, 4000 + cf)
    T.textured_picture_np(1)
    T.textured_picture_np(2, 0)
    _, tm, tc = T.finish()
    inside = ((tm["x"][:n] >= x0) & (tm["y"][:n] >= y0))
    where = np.nonzero(inside)[0]  # raster order, as the small picture's MBs
    assert len(where) == sn
    pics = np.zeros(len(s.pics), R.PIC_DTYPE)
    mbs = np.zeros(len(s.pics) * n, R.MB_DTYPE)
    words = []
    for p in range(len(s.pics)):
        pics[p] = s.pics[p]
        pics[p]["mb_first"], pics[p]["mb_width"], pics[p]["mb_height"] = p * n, mbw, mbh
        M = mbs[p * n:(p + 1) * n]
        small = s.mbs[p * sn:(p + 1) * sn]
        if p < 2:
            M[:] = tm[p * n:(p + 1) * n]
        else:
            M["x"], M["y"], M["qscale"] = tm["x"][:n], tm["y"][:n], 2
            uf, ub = picture_uses(s.pics, s.mbs, p)
            M["flags"] = (MB_FWD if uf else 0) | (MB_BWD if ub else 0)
        M["ncoef"][where] = small["ncoef"]
        for k in ("flags", "cbp", "qscale", "mv"):
            M[k][where] = small[k]
        # the words in raster order: the window's MBs take the small sweep's
        if p < 2:
            per, o = int(tm["ncoef"][p * n]), int(tm["coef_off"][p * n])
            big = tc[o:o + n * per].reshape(n, per)
            rows = [big[i] for i in range(n)]
        else:
            rows = [np.zeros(0, np.uint32)] * n
        for j, i in enumerate(where):
            o = int(small["coef_off"][j])
            rows[i] = s.coefs[o:o + int(small["ncoef"][j])]
        words.append(np.concatenate(rows))
    nc = mbs["ncoef"].astype(np.int64)
    mbs["coef_off"] = np.cumsum(nc) - nc
    out = SweepBatch.__new__(SweepBatch)
    out.width, out.height, out.cf = width, height, cf
    out.pics, out.mbs, out.coefs = pics, mbs, np.concatenate(words).astype(np.uint32)
    out.first_two_dir = s.first_two_dir
    out.window = (x0, y0)
    out.coverage = sweep_coverage(width, height, cf, pics, mbs, window=out.window)
    _corner[ck] = out
    return out
