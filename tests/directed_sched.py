"""Directed tests of the level scheduler (runtime.cpp plan_batch / plan_from_uses / TilePlan /
batch_decode, recon.hip recon_kernel's unit mapping): which kernel runs on which picture, in which
order, on which stream, with which tile state.

Three parts, shared by tests/test_sched_cpu.py (no device) and tests/test_gpu_sched.py:

* check_plan: what ANY correct plan of a batch must satisfy, stated over the plan the library dumps
  (records.plan_dump = mp2vg_batch_plan), not a restatement of the planner: it derives the hazards,
  the slot sharing and the tile reads from the picture records and the used references alone and
  checks the dumped slices, launches, tile plan and footprints against them.  A violation raises
  PlanError naming the requirement: cover, hazard, sets, mode, tiles or foot.
* MUTANTS: named corruptions of a dumped, valid plan, each of which check_plan must reject under
  the requirement it breaks (the checker's own test).
* directed batches: builders of (pics, mbs, coefs, uses) whose slot reuse makes the WAW and WAR
  terms bind, puts I pictures into mixed launches, shifts the slice pairing across clusters and
  picture types, and walks the degenerate routes (all-intra P / B pictures without reference
  slots, B pictures read by B pictures) -- none of which a closed-GOP stream planned one slot per
  picture reaches.
"""
import copy

import numpy as np

from helpers import fill_mb
from tiny_mp2v_dec_amd import records as R
from tiny_mp2v_dec_amd._lib import COEF_DC, MB_BWD, MB_FWD, MB_INTRA

SIZES = [(64, 48), (128, 48), (80, 32)]
REQUIREMENTS = ("cover", "hazard", "sets", "mode", "tiles", "foot")


# ---- batches from picture specs ---------------------------------------------------------------
# One picture: (type, dst, fwd, bwd, kind).  type "I" / "P" / "B"; kind says what its macroblocks
# do: "i" all intra, "f" forward, "b" backward, "fb" every direction mix, "n" inter MBs that carry
# neither direction flag (forward prediction by definition, P pictures), "d" both directions in every
# inter MB (a two-direction B picture even where the picture is one MB).
def pic(t, dst, fwd=-1, bwd=-1, kind=None):
    kind = kind or {"I": "i", "P": "f", "B": "fb"}[t]
    return (t, dst, fwd, bwd, kind)


DIRS = {"f": [MB_FWD], "b": [MB_BWD], "fb": [MB_FWD, MB_BWD, MB_FWD | MB_BWD], "n": [0], "d": [MB_FWD | MB_BWD]}
USES = {"i": (False, False), "f": (True, False), "b": (False, True), "fb": (True, True), "n": (True, False),
        "d": (True, True)}


def used_refs(pics, mbs):
    """(npics, 2) bool: forward used iff some non-intra MB has FWD or lacks BWD; backward used iff
    some MB has BWD (intra MBs carry no direction flags)."""
    out = np.zeros((len(pics), 2), bool)
    for p, P in enumerate(pics):
        n = int(P["mb_width"]) * int(P["mb_height"])
        f = mbs["flags"][int(P["mb_first"]):int(P["mb_first"]) + n].astype(np.int64)
        inter = (f & MB_INTRA) == 0
        out[p, 0] = bool(np.any(inter & (((f & MB_FWD) != 0) | ((f & MB_BWD) == 0))))
        out[p, 1] = bool(np.any(inter & ((f & MB_BWD) != 0)))
    return out


def build(width, height, cf, spec, seed=1, dense=True):
    """(pics, mbs, coefs, uses) of a picture spec.  dense: random_batch's record filling (every MB
    feature, in-plane vectors, dense residuals); else the lightest valid records (DC-only intra
    MBs, zero vectors, no residual), for plans that do not depend on the content."""
    rng = np.random.default_rng(seed)
    mbw, mbh = width // 16, height // 16
    nb = {1: 6, 2: 8, 3: 12}[cf]
    n = mbw * mbh
    pics = np.zeros(len(spec), R.PIC_DTYPE)
    mbs = np.zeros(n * len(spec), R.MB_DTYPE)
    coefs = []
    for p, (t, dst, fwd, bwd, kind) in enumerate(spec):
        P = pics[p]
        P["dst_slot"], P["fwd_slot"], P["bwd_slot"] = dst, fwd, bwd
        P["picture_coding_type"] = "IPB".index(t) + 1
        P["mb_first"] = p * n
        P["mb_width"], P["mb_height"] = mbw, mbh
        P["alternate_scan"] = rng.integers(0, 2)
        P["W"] = rng.integers(1, 48, size=(4, 64))
        M = mbs[p * n:(p + 1) * n]
        M["x"], M["y"] = np.arange(n) % mbw, np.arange(n) // mbw
        if not dense:
            M["qscale"] = 8
            if kind == "i":
                M["flags"], M["cbp"], M["ncoef"] = MB_INTRA, (1 << nb) - 1, nb
                M["coef_off"] = len(coefs) + nb * np.arange(n)
                words = (128 | COEF_DC | (np.arange(nb) << 22))[None, :] | ((M["x"].astype(np.int64) & 7) << 26)[:, None]
                coefs.extend(words.reshape(-1).tolist())
            else:
                M["flags"] = np.array(DIRS[kind])[np.arange(n) % len(DIRS[kind])]
                M["coef_off"] = len(coefs)
            continue
        for k in range(n):
            m = M[k]
            # the first MBs of a predicted picture are inter, one per direction choice, so the
            # picture uses exactly the references its kind names whatever the draws
            force = kind != "i" and k < len(DIRS[kind])
            while True:
                c0 = len(coefs)
                fill_mb(rng, m, coefs, width, height, cf, kind == "i", [DIRS[kind][k]] if force else DIRS.get(kind), True)
                if not force or not (int(m["flags"]) & MB_INTRA):
                    break
                del coefs[c0:]
    coefs = np.array(coefs, dtype=np.uint32)
    uses = used_refs(pics, mbs)
    for p, s in enumerate(spec):
        assert tuple(uses[p]) == USES[s[4]], (p, s)
    return pics, mbs, coefs, uses


def nslots_of(spec):
    return 1 + max(max(s[1], s[2], s[3]) for s in spec)


def gop_ring(nslots, ngops=3, nsub=2):
    """ngops closed GOPs in decode order (I P B B P B B) over a ring of nslots slots: the B
    pictures share one slot, each overwritten by the next (WAW); the anchors rotate over the other
    nslots - 1, each overwritten once nothing later reads it (WAR: its last readers are B
    pictures).  An I picture has no reference to wait for, so its level is set by WAW / WAR alone."""
    spec, a, na, bslot = [], 0, nslots - 1, nslots - 1
    for _ in range(ngops):
        spec.append(pic("I", a % na))
        a += 1
        for _ in range(nsub):
            spec.append(pic("P", a % na, (a - 1) % na))
            a += 1
            spec += [pic("B", bslot, (a - 2) % na, (a - 1) % na)] * 2
    return spec


def ring_delay():
    """A ring of 5 slots in which WAR delays I picture 5 (it overwrites slot 0, which B pictures 2
    and 3 read at level 2) into level 3, beside B picture 6 and P picture 7: an I picture inside a
    mixed launch.  P picture 8 reads it, so it stores its tiles from the mixed kernel's I loop."""
    return [pic("I", 0), pic("P", 1, 0), pic("B", 2, 0, 1), pic("B", 3, 0, 1), pic("P", 4, 1),
            pic("I", 0), pic("B", 2, 1, 4), pic("P", 3, 4),
            pic("P", 4, 0), pic("B", 2, 0, 4), pic("B", 1, 3, 4)]


def mixed_i_p():
    """Level 2 holds {I, P}: WAR puts I picture 2 there (slot 0, read by P picture 1 at level 1);
    P picture 4 reads it."""
    return [pic("I", 0), pic("P", 1, 0), pic("I", 0), pic("P", 2, 1), pic("P", 3, 0), pic("B", 4, 2, 3)]


def mixed_i_b():
    """Level 2 holds {I, B}: I picture 3 (WAR on slot 0) beside two-direction B picture 4; P
    picture 5 reads the I picture."""
    return [pic("I", 0), pic("I", 3), pic("P", 1, 0), pic("I", 0), pic("B", 2, 1, 3), pic("P", 4, 0),
            pic("B", 2, 0, 4)]


def mixed_b1_b2():
    """Level 2 holds a two-direction and two one-direction B pictures (backward only, forward
    only): kinds P-loop and B-loop in one launch, no P picture."""
    return [pic("I", 0), pic("P", 1, 0), pic("B", 2, 0, 1), pic("B", 3, -1, 1, "b"), pic("B", 4, 0, -1, "f")]


def pair_shift(ngops):
    """MB height 3, one chain of launches.  Level 2 is the odd cluster {B, B, P} (9 slices: the
    launch's last workgroup holds one).  Level 3 holds I picture 5 (WAR on slot 0; 3 slices, an
    odd cluster of its own) followed by the odd cluster {B, one-direction B, P}: every later slice
    pairs across pictures.  With three GOPs level 3 goes on with I picture 9 (WAW on slot 2) and P
    picture 10 on its own: an I slice and a P slice in one workgroup.  Pictures 11 / 12 read the I
    pictures, which therefore store their tiles inside the mixed kernel."""
    spec = [pic("I", 0), pic("P", 1, 0), pic("B", 2, 0, 1), pic("B", 3, 0, 1), pic("P", 4, 1),
            pic("I", 0), pic("B", 5, 1, 4), pic("B", 6, -1, 4, "b"), pic("P", 7, 4)]
    if ngops == 3:
        spec += [pic("I", 2), pic("P", 3, 4), pic("P", 8, 2), pic("B", 9, 0, 8)]
    else:
        spec += [pic("P", 8, 0)]
    return spec


def degenerate_intra():
    """All-intra P and B pictures with fwd_slot == bwd_slot == -1: inside a mixed launch (level 0:
    {I, P, B}) and in a launch of their own (level 2: mode 1); P picture 7's inter MBs carry
    neither direction flag.  B pictures read by later pictures get their tiles by conversion after
    a mode 3 launch (picture 2), a mode 1 launch (pictures 6 and 8) and a mode 2 launch (picture 9)."""
    return [pic("I", 0), pic("P", 1, kind="i"), pic("B", 2, kind="i"),
            pic("B", 3, 0, 1), pic("B", 4, 2, 0),
            pic("P", 3, kind="i"), pic("B", 4, kind="i"),
            pic("P", 5, 3, kind="n"), pic("B", 6, 4, -1, "f"),
            pic("B", 7, 5, 6), pic("B", 8, 7, 5)]


def degenerate_clusters():
    """Reference-sharing clusters of 4 (the cap), 1, 2 and 3 pictures."""
    return [pic("I", 0), pic("P", 1, 0)] + [pic("B", 2 + i, 0, 1) for i in range(4)] + [pic("P", 6, 1)] + \
           [pic("B", 2, 1, 6), pic("B", 3, 1, 6)] + [pic("P", 7, 6), pic("B", 4, 6, 7), pic("B", 5, 6, 7), pic("P", 8, 7)]


def units(n):
    """n I pictures, then n P pictures each predicted from its own I picture (64 x 16: one slice
    per picture).  On one stream: an I launch of n workgroups and a P launch of ceil(n / 2), so
    n = 1..18 walks every residue of recon_kernel's XCD unit bijection with q8 == 0 and q8 > 0."""
    return [pic("I", i) for i in range(n)] + [pic("P", n + i, i) for i in range(n)]


def two_components(long_chain=8):
    """Two slot-disjoint components: slots 0-3 (I P B B), dealt to set 0, and slots 4-7 with a
    chain of long_chain dependent launches (I, then P pictures each predicted from the one before
    over a ring of 4 slots), dealt to set 1."""
    spec = [pic("I", 0), pic("I", 4), pic("P", 1, 0), pic("B", 2, 0, 1), pic("B", 3, 0, 1)]
    spec += [pic("P", 4 + (i % 4), 4 + ((i - 1) % 4)) for i in range(1, long_chain)]
    return spec


DIRECTED = {
    "ring4": lambda: gop_ring(4), "ring5": lambda: gop_ring(5), "ring_delay": ring_delay,
    "mixed_i_p": mixed_i_p, "mixed_i_b": mixed_i_b, "mixed_b1_b2": mixed_b1_b2,
    "pair_shift2": lambda: pair_shift(2), "pair_shift3": lambda: pair_shift(3),
    "degenerate_intra": degenerate_intra, "degenerate_clusters": degenerate_clusters,
    "two_components": two_components,
}


def seed_of(name, width, cf):
    return 1000 * sorted(DIRECTED).index(name) + 10 * width + cf


# ---- the requirement checker --------------------------------------------------------------------
class PlanError(AssertionError):
    def __init__(self, requirement, detail):
        assert requirement in REQUIREMENTS
        self.requirement = requirement
        super().__init__(f"{requirement}: {detail}")


def _need(ok, requirement, detail):
    if not ok:
        raise PlanError(requirement, detail)


def read_slots(pics, uses, p):
    """The reference slots picture p actually reads."""
    return [int(pics[p][f]) for f, u in (("fwd_slot", uses[p][0]), ("bwd_slot", uses[p][1])) if u]


def hazards(pics, uses):
    """[(p, q, kind)] for p < q in decode order: RAW (q reads p's slot), WAW, WAR (q overwrites a
    slot p reads)."""
    out = []
    for q in range(len(pics)):
        for p in range(q):
            dp, dq = int(pics[p]["dst_slot"]), int(pics[q]["dst_slot"])
            if dp in read_slots(pics, uses, q):
                out.append((p, q, "RAW"))
            if dp == dq:
                out.append((p, q, "WAW"))
            if dq in read_slots(pics, uses, p):
                out.append((p, q, "WAR"))
    return out


def kind_of(pics, uses, p):
    """The loop a picture runs: "I", "P" (P pictures and B pictures that do not use both
    directions) or "B"."""
    t = int(pics[p]["picture_coding_type"])
    return "I" if t == 1 else ("B" if t == 3 and uses[p][0] and uses[p][1] else "P")


def launch_of_pics(dump, npics):
    """Launch index of each picture (the launch of its first slice; -1: none)."""
    of = [-1] * npics
    for li, L in enumerate(dump["launches"]):
        for k in range(int(L[0]), min(int(L[1]), len(dump["slices"]))):
            q = int(dump["slices"][k][0])
            if 0 <= q < npics and of[q] < 0:
                of[q] = li
    return of


def check_plan(pics, uses, geometry, nstreams, dump):
    """Raise PlanError(requirement, ...) unless the dumped plan satisfies every requirement of a
    correct plan of the batch (module docstring)."""
    width, height, _cf = geometry
    mbw, mbh = width // 16, height // 16
    n, npics = mbw * mbh, len(pics)
    S, L = dump["slices"], dump["launches"]
    dst = [int(P["dst_slot"]) for P in pics]
    ptype = [int(P["picture_coding_type"]) for P in pics]

    # cover: every MB record once, in slices of one launch; slice shapes and mates
    owner = np.full(len(S), -1)
    for li, (b, e, _mode, _level, _set, _mates) in enumerate(L):
        _need(0 <= b <= e <= len(S), "cover", f"launch {li} slice range [{b}, {e}) outside the slices")
        _need(np.all(owner[b:e] < 0), "cover", f"launch {li} shares slices with an earlier launch")
        owner[b:e] = li
    _need(np.all(owner >= 0), "cover", "slices outside every launch")
    seen = np.zeros((npics, n), np.int64)
    lof = [-1] * npics
    inloop = [True] * npics  # every slice of the picture stores its tiles in the loop (bit 0)
    for k, (q, mb0, cnt, fl) in enumerate(S):
        li = int(owner[k])
        mates = int(L[li][5])
        _need(0 <= q < npics, "cover", f"slice {k} names picture {q}")
        lo = int(mb0) - int(pics[q]["mb_first"])
        _need(cnt > 0 and lo >= 0 and lo + cnt <= n, "cover", f"slice {k} leaves picture {q}'s MB records")
        seen[q, lo:lo + cnt] += 1
        _need(lof[q] in (-1, li), "cover", f"picture {q} in launches {lof[q]} and {li}")
        lof[q] = li
        inloop[q] = inloop[q] and bool(fl & 1)
        if mbw % 4 == 0:
            _need(lo % 4 == 0 and (lo + cnt) % 4 == 0, "cover", f"slice {k} is cut inside a 4-MB group")
        else:
            _need(lo % mbw == 0 and cnt == mbw, "cover", f"slice {k} is not one whole row (mb_width {mbw})")
            _need(mates == 0, "cover", f"launch {li}: mates {mates} at mb_width {mbw}")
    for q in range(npics):
        _need(np.all(seen[q] == 1), "cover", f"picture {q}: MB records covered {sorted(set(seen[q].tolist()))} times")
    for li, (b, e, mode, _level, _set, mates) in enumerate(L):
        inside = sorted({int(S[k][0]) for k in range(b, e)})
        if inside and all(ptype[q] == 1 for q in inside):
            _need(mates == 0, "cover", f"I launch {li} with mates {mates}")
        if mode in (1, 2, 3) and mbw % 4 == 0:
            _need(mates == 2, "cover", f"launch {li} (mode {mode}) with mates {mates}")
            for k in range(b, e):
                lo = int(S[k][1]) - int(pics[int(S[k][0])]["mb_first"])
                _need(lo // mbw == (lo + int(S[k][2]) - 1) // mbw, "cover", f"slice {k} of launch {li} spans rows")

    # hazard: ordered inside one set's chain (launches of a set are enqueued in list order)
    set_of = [int(L[lof[q]][4]) for q in range(npics)]
    for p, q, kind in hazards(pics, uses):
        _need(lof[p] != lof[q], "hazard", f"{kind} pictures {p} and {q} share launch {lof[p]}")
        _need(set_of[p] == set_of[q], "hazard", f"{kind} pictures {p} and {q} in sets {set_of[p]} and {set_of[q]}")
        _need(lof[p] < lof[q], "hazard", f"{kind}: picture {q} (launch {lof[q]}) not after picture {p} (launch {lof[p]})")

    # sets: slot sharers together, no more sets than streams or pictures
    nsets_max = max(1, min(nstreams, npics))
    holder = {}
    for q in range(npics):
        _need(0 <= set_of[q] < nsets_max, "sets", f"picture {q} in set {set_of[q]} of {nsets_max}")
        for s in [dst[q]] + read_slots(pics, uses, q):
            _need(holder.setdefault(s, set_of[q]) == set_of[q], "sets", f"slot {s} is touched from sets {holder[s]} and {set_of[q]}")

    # mode and slice flag bits
    for li, (b, e, mode, _level, _set, _mates) in enumerate(L):
        kinds = {kind_of(pics, uses, int(S[k][0])) for k in range(b, e)}
        if not kinds:  # (an empty launch is not enqueued)
            continue
        want = {"I": 0, "P": 1, "B": 2}[next(iter(kinds))] if len(kinds) == 1 else 3
        _need(mode == want, "mode", f"launch {li} of kinds {sorted(kinds)} has mode {mode}")
    for k, (q, _mb0, _cnt, fl) in enumerate(S):
        isb = ptype[q] == 3
        _need(bool(fl & 2) == (isb and not (uses[q][0] and uses[q][1])), "mode", f"slice {k} (picture {q}): bit 1 is {fl >> 1 & 1}")
        _need(bool(fl & 4) == (isb and uses[q][1] and not uses[q][0]), "mode", f"slice {k} (picture {q}): bit 2 is {fl >> 2 & 1}")
        _need(not (fl & 1) or not isb, "mode", f"slice {k}: bit 0 set on B picture {q}")
        _need(fl < 8, "mode", f"slice {k}: unknown flag bits {fl}")

    # tiles: every in-batch read finds fresh tiles; external reads and final tile states declared
    post = [(int(a), int(b)) for a, b in dump["post"]]
    for a, s in post:
        _need(0 <= a < len(L) and any(lof[q] == a and dst[q] == s for q in range(npics)), "tiles",
              f"post entry (launch {a}, slot {s}) names no picture of that launch")
    stores = [inloop[q] or (lof[q], dst[q]) in post for q in range(npics)]
    writer, ext = {}, {}
    for q in range(npics):
        for s in read_slots(pics, uses, q):
            if s in writer:
                p = writer[s]
                _need(stores[p], "tiles", f"picture {q} reads slot {s} of picture {p}, which stores no tiles")
            else:
                ext.setdefault(s, set_of[q])
        writer[dst[q]] = q
    got = [(int(a), int(b)) for a, b in dump["ext_reads"]]
    _need(sorted(got) == sorted(ext.items()), "tiles", f"ext_reads {sorted(got)}, external reads {sorted(ext.items())}")
    W = dump["writes"]
    _need(len(W) == npics, "tiles", f"{len(W)} writes for {npics} pictures")
    for q in range(npics):
        _need(int(W[q][0]) == dst[q] and int(W[q][1]) == int(stores[q]), "tiles",
              f"writes[{q}] = {tuple(int(x) for x in W[q])}, picture writes slot {dst[q]}, stores tiles: {stores[q]}")
    for q in [q for q in range(npics) if ptype[q] != 3][-2:]:
        _need(stores[q], "tiles", f"picture {q}, one of the batch's last two anchors, stores no tiles")

    # foot: exactly the slots each set touches
    foot = dump["foot"]
    _need(len(foot) <= nsets_max and len(foot) > max(set_of), "foot", f"{len(foot)} footprints")
    for t in range(len(foot)):
        want = sorted({s for q in range(npics) if set_of[q] == t for s in [dst[q]] + read_slots(pics, uses, q)})
        _need(sorted(int(x) for x in foot[t]) == want, "foot", f"set {t}: foot {sorted(int(x) for x in foot[t])}, touches {want}")


# ---- what a plan exercises (coverage) -----------------------------------------------------------
def binding_hazards(pics, uses):
    """Which hazard kinds are some picture's binding constraint: with levels from all hazards
    (level = 1 + the highest level among hazard predecessors), a kind binds for q when leaving
    that kind's pairs out would lower q's level."""
    hz = hazards(pics, uses)
    lv = [0] * len(pics)
    for p, q, _kind in hz:  # sorted by q, and p < q: lv[p] is final when q is reached
        lv[q] = max(lv[q], lv[p] + 1)
    out = set()
    for kind in ("RAW", "WAW", "WAR"):
        rest = [0] * len(pics)
        for p, q, k in hz:
            if k != kind:
                rest[q] = max(rest[q], lv[p] + 1)
        if any(rest[q] < lv[q] for q in range(len(pics))):
            out.add(kind)
    return out


def clusters_of(dump, li):
    """Picture groups of launch li whose slices interleave (reference-sharing clusters show as
    row-by-row interleave when a picture has more than one slice)."""
    b, e = int(dump["launches"][li][0]), int(dump["launches"][li][1])
    span = {}
    for k in range(b, e):
        q = int(dump["slices"][k][0])
        span[q] = (span.get(q, (k, k))[0], k)
    out = []
    for q, (lo, hi) in sorted(span.items(), key=lambda x: x[1]):
        if out and lo <= out[-1][1]:
            out[-1][0].append(q)
            out[-1][1] = max(out[-1][1], hi)
        else:
            out.append([[q], hi])
    return [c[0] for c in out]


def unit_pairs(pics, uses, dump, li):
    """Per workgroup unit (slices 2k, 2k + 1) of a mates == 2 launch: ((kind, picture), (kind,
    picture) or None).  kind: "I", "P", "B1" (one-direction B) or "B2"."""
    def k4(q):
        t = int(pics[q]["picture_coding_type"])
        return "I" if t == 1 else "P" if t == 2 else ("B2" if uses[q][0] and uses[q][1] else "B1")
    b, e = int(dump["launches"][li][0]), int(dump["launches"][li][1])
    qs = [int(dump["slices"][k][0]) for k in range(b, e)]
    return [((k4(qs[i]), qs[i]), (k4(qs[i + 1]), qs[i + 1]) if i + 1 < len(qs) else None) for i in range(0, len(qs), 2)]


# ---- plan mutants -------------------------------------------------------------------------------
def mutant_spec():
    """One small batch with everything the mutants corrupt: two P pictures that share only an
    external reference (slot 0), a B picture read by a B picture (post), a backward-only B picture,
    and a second component (slots 6-7) for the other set."""
    return [pic("P", 1, 0), pic("P", 2, 0), pic("B", 3, 1, 2), pic("B", 4, 3, 1), pic("B", 5, -1, 2, "b"),
            pic("I", 6), pic("P", 7, 6)]


def _rows_of(d, q):
    return [k for k in range(len(d["slices"])) if int(d["slices"][k][0]) == q]


def _delete_slice(d, k):
    d["slices"] = np.delete(d["slices"], k, axis=0)
    for L in d["launches"]:
        L[0] -= L[0] > k
        L[1] -= L[1] > k


def _insert_slice(d, k, row):
    """Insert a slice at index k, inside the launch that holds slice k - 1."""
    d["slices"] = np.insert(d["slices"], k, row, axis=0)
    for L in d["launches"]:
        L[0] += L[0] >= k
        L[1] += L[1] >= k


def _swap_pictures(d, pics, p, q):
    for k in _rows_of(d, p) + _rows_of(d, q):
        a = int(d["slices"][k][0])
        b = q if a == p else p
        d["slices"][k][1] += int(pics[b]["mb_first"]) - int(pics[a]["mb_first"])
        d["slices"][k][0] = b


def _move_into_launch(d, q, li):
    rows = [d["slices"][k].copy() for k in _rows_of(d, q)]
    for k in reversed(_rows_of(d, q)):
        _delete_slice(d, k)
    for row in rows:
        _insert_slice(d, int(d["launches"][li][1]), row)


def _set_mode_2_on_p_launch(d, pics):
    li = next(li for li, L in enumerate(d["launches"])
              if any(int(pics[int(d["slices"][k][0])]["picture_coding_type"]) == 2 for k in range(L[0], L[1])))
    d["launches"][li][2] = 2


def _flag(d, q, bit, value=None):
    for k in _rows_of(d, q):
        d["slices"][k][3] = d["slices"][k][3] ^ bit if value is None else (d["slices"][k][3] & ~bit) | (bit if value else 0)


def _drop_foot(d):
    d["foot"][0] = d["foot"][0][1:]


def _cut_off_boundary(d):
    k = 0
    q, mb0, cnt, fl = (int(x) for x in d["slices"][k])
    d["slices"][k][2] = 2
    _insert_slice(d, k + 1, [q, mb0 + 2, cnt - 2, fl])


def _other_set(d, pics, q):
    """Picture q, alone in its launch, runs on the other set's stream."""
    li = launch_of_pics(d, len(pics))[q]
    d["launches"][li][4] ^= 1


def _set_mates(d):
    for L in d["launches"]:
        if L[2] != 0:
            L[5] = 2


# name -> (geometry, mutation(dump, pics), the requirement check_plan must name).  All on
# mutant_spec(), two streams; pictures 0 / 1 are the P pictures, 2-4 the B pictures.
MUTANTS = {
    "swap_dependent_pictures": ((64, 48, 1), lambda d, pics: _swap_pictures(d, pics, 2, 3), "hazard"),
    "dependent_into_producers_launch": ((64, 48, 1), lambda d, pics: _move_into_launch(d, 3, launch_of_pics(d, len(pics))[2]), "hazard"),
    "picture_to_other_set": ((64, 48, 1), lambda d, pics: _other_set(d, pics, 6), "hazard"),
    "slot_sharer_to_other_set": ((64, 48, 1), None, "sets"),  # (its own batch: mutant_sharers)
    "row_dropped": ((64, 48, 1), lambda d, pics: _delete_slice(d, _rows_of(d, 2)[1]), "cover"),
    "row_duplicated": ((64, 48, 1), lambda d, pics: _insert_slice(d, _rows_of(d, 2)[1], d["slices"][_rows_of(d, 2)[1]].copy()), "cover"),
    "slice_cut_off_group_boundary": ((64, 48, 1), lambda d, pics: _cut_off_boundary(d), "cover"),
    "post_entry_dropped": ((64, 48, 1), lambda d, pics: d.__setitem__("post", d["post"][1:]), "tiles"),
    "ext_read_dropped": ((64, 48, 1), lambda d, pics: d.__setitem__("ext_reads", d["ext_reads"][1:]), "tiles"),
    "bit0_cleared_on_read_anchor": ((64, 48, 1), lambda d, pics: _flag(d, 1, 1, False), "tiles"),
    "bit0_set_on_b_picture": ((64, 48, 1), lambda d, pics: _flag(d, 2, 1, True), "mode"),
    "bit2_flipped": ((64, 48, 1), lambda d, pics: _flag(d, 4, 4), "mode"),
    "slot_dropped_from_foot": ((64, 48, 1), lambda d, pics: _drop_foot(d), "foot"),
    "mates_2_at_mbw_5": ((80, 32, 1), lambda d, pics: _set_mates(d), "cover"),
    "mode_2_on_p_launch": ((64, 48, 1), lambda d, pics: _set_mode_2_on_p_launch(d, pics), "mode"),
}


def mutant_sharers():
    """Two P pictures whose only common slot is an external reference they both read: no hazard
    orders them, yet they belong to one set (the reference's tiles are rebuilt on one stream).
    A third, unrelated picture takes the other set."""
    return [pic("P", 1, 0), pic("I", 3), pic("P", 2, 0)]


def run_mutant(name):
    """(valid dump, mutated dump, pics, uses, geometry) of a mutant."""
    geometry, fn, _req = MUTANTS[name]
    spec = mutant_sharers() if fn is None else mutant_spec()
    pics, mbs, coefs, uses = build(*geometry, spec, dense=False)
    good = R.plan_dump(*geometry, nslots_of(spec), pics, mbs, coefs)
    bad = copy.deepcopy(good)
    if fn is None:
        # pictures 0 and 2 share a launch of set 0: picture 2's slices, moved to the launch's end,
        # become a launch of their own on the other set
        li = launch_of_pics(bad, len(pics))[2]
        b, e = int(bad["launches"][li][0]), int(bad["launches"][li][1])
        rows = [k for k in range(b, e) if int(bad["slices"][k][0]) != 2] + _rows_of(bad, 2)
        assert sorted(rows) == list(range(b, e))
        bad["slices"][b:e] = bad["slices"][rows]
        cut = e - len(_rows_of(bad, 2))
        new = bad["launches"][li].copy()
        bad["launches"][li][1] = cut
        new[0], new[4] = cut, new[4] ^ 1
        bad["launches"] = np.insert(bad["launches"], li + 1, new, axis=0)
        bad["post"] = np.array([[a + (a > li), s] for a, s in bad["post"]], np.int32).reshape(-1, 2)
    else:
        fn(bad, pics)
    return good, bad, pics, uses, geometry


# ---- seeded random batches (plans only) ---------------------------------------------------------
def random_spec(rng):
    """A valid batch by construction: 2-16 pictures over a pool of 3-6 slots, each picture's slots
    drawn at random; random types and used directions; no own-slot prediction, no backward
    prediction in P pictures; a reference not yet written in the batch is an external read.
    Unused reference fields hold -1 or any slot (the destination included): they must not count."""
    nslots = int(rng.integers(3, 7))
    spec = []
    for _ in range(int(rng.integers(2, 17))):
        t = "IPB"[int(rng.integers(0, 3))]
        dst = int(rng.integers(0, nslots))
        kind = "i" if t == "I" else str(rng.choice(["f", "i", "n"] if t == "P" else ["fb", "f", "b", "i"]))
        other = [s for s in range(nslots) if s != dst]
        ref = [int(rng.choice(other)) if u else int(rng.integers(-1, nslots)) for u in USES[kind]]
        spec.append((t, dst, ref[0], ref[1], kind))
    return spec, nslots


# ---- shared, cached batches and coverage ----------------------------------------------------------
_CACHE = {}


def batch(name, width, height, cf, dense=True):
    """(spec, pics, mbs, coefs, uses) of a directed batch (DIRECTED, or "units<n>"), built once."""
    key = (name, width, height, cf, dense)
    if key not in _CACHE:
        spec = units(int(name[5:])) if name.startswith("units") else DIRECTED[name]()
        seed = 77 + int(name[5:]) if name.startswith("units") else seed_of(name, width, cf)
        _CACHE[key] = (spec,) + build(width, height, cf, spec, seed=seed, dense=dense)
    return _CACHE[key]


def components(pics, uses):
    """Number of slot-sharing components of the batch's pictures."""
    parent = list(range(len(pics)))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x
    owner = {}
    for q in range(len(pics)):
        for s in [int(pics[q]["dst_slot"])] + read_slots(pics, uses, q):
            if s in owner:
                parent[find(q)] = find(owner[s])
            else:
                owner[s] = q
    return len({find(q) for q in range(len(pics))})


def coverage(pics, uses, dump):
    """Tags of what the batch and its plan exercise (tests/test_sched_cpu.py asserts their union)."""
    tags = {"bind:" + k for k in binding_hazards(pics, uses)}
    L = dump["launches"]
    for li in range(len(L)):
        mode = int(L[li][2])
        tags.add(f"mode:{mode}")
        kinds = {a[0] for u in unit_pairs(pics, uses, dump, li) for a in u if a}
        if mode == 3:
            tags.add("mix:" + "+".join(sorted(kinds)))
        if int(pics[0]["mb_height"]) > 1:
            tags.update(f"cluster:{len(c)}" for c in clusters_of(dump, li))
    if components(pics, uses) > len({int(x[4]) for x in L}):
        tags.add("components>sets")
    tags.update(f"post_after_mode:{int(L[int(a)][2])}" for a, _s in dump["post"])
    if len(dump["ext_reads"]):
        tags.add("ext_reads")
    return tags


def split(pics, mbs, coefs, k):
    """The batch as two: pictures [0, k) and [k, n), each with its own record arrays."""
    n = int(pics[0]["mb_width"]) * int(pics[0]["mb_height"])
    c0 = int(mbs["coef_off"][k * n]) if k < len(pics) else len(coefs)
    p2, m2 = pics[k:].copy(), mbs[k * n:].copy()
    p2["mb_first"] -= k * n
    m2["coef_off"] -= c0
    return (pics[:k], mbs[:k * n], coefs[:c0]), (p2, m2, coefs[c0:])
