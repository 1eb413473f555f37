"""CPU: the int64 model of tests/directed_idct.py, the oracle and the reference's own outputs
(tests/golden/idct_directed.npz) agree on every witness vector; the seeded search reproduces the
fixture; every named mutant is killed on final bytes by its witnesses, per form and line, or
excluded by a bound; the directed batches hold what they claim, and every mutant would change their
expected frames."""
import numpy as np
import pytest

import directed as D
import directed_idct as I
from tiny_mp2v_dec_amd import records as R

SIZES = [(128, 16), (80, 32), (96, 32), (112, 32)]
LAUNCHES = ["I", "P", "B", "mixed"]
MODE = {"I": 0, "P": 1, "B": 2, "mixed": 3}
BY_NAME = dict(zip(I.NAMES, I.MUTANTS))


def _size_id(s):
    return "%dx%d" % s


def _same(a, b):
    return all(np.array_equal(a[p][k], b[p][k]) for p in range(len(b)) for k in range(3))


def test_model_oracle_and_reference_agree():
    """Every vector through both forms: model == oracle_idct == the reference binary's bytes."""
    V = I.vectors()
    p = V.p.astype(np.int64)
    assert np.array_equal(I.model_idct(V.F), V.put) and np.array_equal(I.oracle_idct(V.F), V.put)
    assert np.array_equal(I.model_idct(V.F, p), V.add) and np.array_equal(I.oracle_idct(V.F, p), V.add)
    # the corner blocks: QFS from their words by the dequant model and by the oracle, then the same
    C = V.corner
    for c, (kind, words) in enumerate(I.corner_blocks()):
        wd = [I.Q._pack(l, pos, 0, fl) for l, pos, fl in words]
        Wm = I.corner_matrices()[0 if kind.startswith("intra") else 1].tolist()
        intra = kind.startswith("intra")
        assert I.corner_qfs(kind, words) == C["F"][c].tolist() == I.Q.oracle_qfs(wd, Wm, I.QS_OF[kind], intra, 0)
    assert C["F"][:, 1:].min() == -2048 and C["F"][:, 1:].max() == 2047
    assert {-2677, 2677, -32768, 32767} <= set(C["F"][:, 0].tolist())
    assert np.array_equal(I.model_idct(C["F"]), C["put"]) and np.array_equal(I.oracle_idct(C["F"]), C["put"])
    assert np.array_equal(I.model_idct(C["F"], C["pred"]), C["add"])
    assert np.array_equal(I.oracle_idct(C["F"], C["pred"]), C["add"])
    rng = np.random.default_rng(5)
    F = rng.integers(-2048, 2048, (2000, 64))
    F[:700, 0] = rng.integers(-32768, 32768, 700)
    F[700:1400] *= rng.random((700, 64)) < 0.1
    pr = rng.integers(0, 256, (2000, 64))
    assert np.array_equal(I.model_idct(F), I.oracle_idct(F))
    assert np.array_equal(I.model_idct(F, pr), I.oracle_idct(F, pr))


@pytest.fixture(scope="module")
def searched():
    return I.search()


def test_search_reproduces_the_fixture(searched):
    V, S = I.vectors(), searched
    assert np.array_equal(S.F, V.F) and np.array_equal(S.pred(), V.pred()) and np.array_equal(S.form, V.form)
    assert S.conds == V.conds and S.bounded == V.bounded
    # the vectors are of the legal domain, at matrices 16 and quantiser scale 1
    assert np.abs(V.F[:, 1:].astype(int)).max() <= 2047 and np.abs(V.F[V.form == 1, 0].astype(int)).max() <= 2047
    assert set(V.p[V.form == 1].tolist()) <= set(I.P_VALUES)


def test_every_mutant_is_killed_or_bounded(searched):
    """Per (mutant, form, line): the fixture's witness changes a final byte under the mutant applied
    to that line alone, or bounded() excludes it.  Both halves of the pair and all four lanes are
    lines of their own."""
    V = I.vectors()
    wit = {(n, f, ln): v for n, f, ln, v in V.conds}
    bnd = set(V.bounded)
    missing = list(searched.unkilled)
    for m, form, line in I.conditions():
        key = (I.mutant_name(m), form, line)
        if key in bnd:
            assert I.bounded(m, form == 0, line), key
            continue
        if key not in wit:
            missing.append(key)
            continue
        v = wit[key]
        assert V.form[v] == form, key
        pred = None if form == 0 else V.p[v:v + 1].astype(np.int64)
        if m[0] == "add_for_put":
            pred = np.array([128])
        base = I.model_idct(V.F[v:v + 1], None if form == 0 else V.p[v:v + 1].astype(np.int64))
        assert (I.model_idct(V.F[v:v + 1], pred, m, None if line < 0 else line) != base).any(), key
    summary = bounded_summary(V)
    print("\n".join(summary))
    assert not missing, ("neither killed nor bounded", missing, "bounded:", summary)
    # halves and lanes: every killed arithmetic mutant has a low-half and a high-half line, and all lanes
    for m in I.ARITH:
        for form in (0, 1):
            lines = [ln for (n, f, ln) in wit if n == I.mutant_name(m) and f == form]
            free = [ln for ln in range(8) if (I.mutant_name(m), form, ln) not in bnd]
            assert sorted(lines) == free
            if len(free) == 8:
                assert {I.is_high(m[1], ln) for ln in lines} == {False, True}
                assert {I.lane_of(m[1], ln) for ln in lines} == {0, 1, 2, 3}


def bounded_summary(V):
    by = {}
    for n, f, ln in V.bounded:
        by.setdefault(n, {}).setdefault(f, []).append(ln)
    out = []
    for n in I.NAMES:
        if n in by:
            out.append("%-22s %s" % (n, "; ".join("%s lines %s" % (("put", "add")[f], "".join(map(str, sorted(ls))))
                                                   for f, ls in sorted(by[n].items()))))
    return out


def test_bounds_hold_on_samples_and_cover_the_kernel_comments():
    """bound(): no bounded node saturates on the corners and a million random lines of the domain;
    the kernel's comment bounds on the pass-1 folds hold by the same code."""
    rng = np.random.default_rng(11)
    n = 1_000_000
    for intra, line0 in ((True, True), (False, True), (True, False)):
        b = I.bound(0, intra, 0 if line0 else 3)
        for name, lim in I.KERNEL_BOUNDS.items():
            lo, hi = b.range[name]
            assert -lim <= lo and hi <= lim, (name, lo, hi)
        assert max(abs(b.lo[1:]).max(), b.hi[1:].max()) <= 8191
        s = [rng.choice([-2048, -2047, 2047], n) if i % 2 else rng.integers(-2048, 2048, n) for i in range(8)]
        s[7][: n // 2] = rng.choice([-2048, 2047], n // 2)
        s[0] = rng.integers(int(b.lo[0]), int(b.hi[0]) + 1, n)
        rec = {}
        I.idct_1d([x[None] for x in s], False, I._Num(0, rec=rec))
        for (ps, name, rail), fl in rec.items():
            if not b.may[(name, rail)]:
                assert not fl.any(), (intra, line0, name, rail)
    b = I.bound(1, True, 0)
    assert not b.may[("v14", "+")] and not b.may[("v14", "-")] and not b.may[("v14.op1", "+")]
    assert sum(b.may.values()) == len(b.may) - 4 - 5  # pass 2: all but v14, its inner subs and the five slli(mulhi, 1)


def test_uni_round_table():
    """The 4:2:0 I kernel's round selection as the batches restate it: groups of 1 and 2 MBs run
    every item in the exact form; groups of 3 and 4 run pass-1 slots 0-15 folded and the rest
    (2 or 8 slots) in the exact form, in a round shared with pass-2 items."""
    T = {g: I.uni_rounds(g) for g in (1, 2, 3, 4)}
    assert [(b, f) for b, f, _, _ in T[1]] == [(0, "exact"), (64, "exact")]
    assert [(b, f) for b, f, _, _ in T[2]] == [(0, "exact"), (64, "exact")]
    assert [(b, f) for b, f, _, _ in T[3]] == [(0, "fold"), (64, "exact"), (128, "exact")]
    assert [(b, f) for b, f, _, _ in T[4]] == [(0, "fold"), (64, "exact"), (128, "exact")]
    assert T[3][1][2] == [16, 17] and T[3][1][3] == list(range(14)) and T[3][2][3] == list(range(14, 18))
    assert T[4][1][2] == list(range(16, 24)) and T[4][1][3] == list(range(8)) and T[4][2][3] == list(range(8, 24))
    for g in T:
        for _, form, s1, s2 in T[g]:
            assert form == "exact" or not s2  # pass 2 never runs folded
        assert sorted(s for r in T[g] for s in r[2]) == sorted(s for r in T[g] for s in r[3]) == list(range(6 * g))
    for g in T:
        print("group of %d: %s" % (g, "; ".join("items %d-%d %s, pass-1 slots %s, pass-2 slots %s" % (
            b, b + 63, f, "%d-%d" % (s1[0], s1[-1]) if s1 else "-", "%d-%d" % (s2[0], s2[-1]) if s2 else "-")
            for b, f, s1, s2 in T[g])))


def _check_modes(bt):
    n = len(bt.pics)
    of_pic, modes = R.plan_batch(bt.width, bt.height, bt.cf, n, bt.pics, bt.mbs, bt.coefs)
    assert all(modes[of_pic[p]] == MODE[bt.launch] for p in range(bt.first_case_pic, n)), modes[of_pic]
    if bt.launch != "I":
        a, b = D.split_batch(bt.pics, bt.mbs, bt.coefs, bt.first_case_pic)
        R.plan_batch(bt.width, bt.height, bt.cf, n, *a)
        of_b, modes_b = R.plan_batch(bt.width, bt.height, bt.cf, n, *b)
        assert all(modes_b[of_b[p]] == MODE[bt.launch] for p in range(len(b[0])))


@pytest.mark.parametrize("cf", [1, 2, 3])
@pytest.mark.parametrize("launch", LAUNCHES)
@pytest.mark.parametrize("size", SIZES, ids=_size_id)
def test_directed_batch(cf, launch, size):
    """One batch: the launch mode; the oracle's frames == the model's frames, byte for byte; every
    vector in every MB kind; every cell's witness; every mutant changes a block that is there."""
    w, h = size
    bt = I.idct_batch(w, h, cf, launch)
    _check_modes(bt)
    exp = D.expected_frames(bt.key(), w, h, cf, bt.pics, bt.mbs, bt.coefs)
    assert _same(I.model_frames(bt), exp)
    V = I.vectors()
    kinds, cells = I.coverage(bt)
    print("\n%dx%d cf %d %s: %d pictures\n%s" % (w, h, cf, launch, len(bt.pics), I.coverage_table(bt)))
    for kind in I.KINDS[launch]:
        want = set(np.nonzero((V.form == 1) == kind.startswith("inter"))[0].tolist())
        assert kinds.get(kind, set()) == want, (kind, sorted(want - kinds.get(kind, set())))
    assert I.needs(w, cf, launch) <= cells, sorted(I.needs(w, cf, launch) - cells)
    # every corner block, in an MB of its kind
    want = {c for c, (kd, _) in enumerate(I.corner_blocks()) if launch != "I" or kd.startswith("intra")}
    assert {bl.corner for bl in I.batch_blocks(bt)} - {-1} == want
    sizes = {(bl.gsize) for bl in I.batch_blocks(bt)}
    assert sizes == {4} | ({(w // 16) % 4} - {0})
    if launch != "I":
        assert {bl.slot for bl in I.batch_blocks(bt)} == set(range(4 * D.NB[cf]))
    # every mutant with a witness of a form the batch holds changes the bytes of a block in it
    present = {f: sorted({bl.vec for bl in I.batch_blocks(bt) if bl.vec >= 0 and V.form[bl.vec] == f}) for f in (0, 1)}
    missed = []
    for name in sorted({c[0] for c in V.conds}):
        m = BY_NAME[name]
        for f in sorted({c[1] for c in V.conds if c[0] == name}):
            if present[f] and not (m[0] == "add_for_put" and launch == "I"):
                if not I.Vectors.killed_by(V, m)[present[f]].any():
                    missed.append((name, f))
    assert not missed, missed
    if cf != 3:
        assert not _same(I.model_frames(bt, "field_step_ignored"), exp)
    # one arithmetic mutant through the whole frame path, as a check of the shortcut above
    assert not _same(I.model_frames(bt, BY_NAME["p2.wrap.o0+"]), exp)


@pytest.mark.parametrize("cf", [1, 2, 3])
@pytest.mark.parametrize("launch", LAUNCHES)
def test_stale_lds_batch(cf, launch):
    """512x16: the oracle's frames == the model's; whichever group stride the launch runs its waves
    with, every slot sees a sparse block after a dense one in the same wave, and leaving any one
    chunk unzeroed changes the expected frames."""
    bt = I.stale_batch(cf, launch)
    _check_modes(bt)
    exp = D.expected_frames(bt.key(), 512, 16, cf, bt.pics, bt.mbs, bt.coefs)
    assert _same(I.model_frames(bt), exp)
    for stride in I.WAVE_STRIDES:
        succ = I.stale_successions(bt, stride)
        assert set(succ) == set(range(4 * D.NB[cf])), (stride, sorted(succ))
        for chunk in range(8):
            assert not _same(I.model_frames(bt, ("chunk_unzeroed", chunk, stride)), exp), (stride, chunk)
    # the sparse blocks: position 0 only and position 63 only (an intra block's DC word comes with it)
    sparse = {(bl.intra, bl.pos) for bl in I.batch_blocks(bt) if len(bl.pos) <= 2}
    assert {(True, (0,)), (True, (0, 63))} <= sparse
    assert launch == "I" or {(False, (0,)), (False, (63,))} <= sparse
