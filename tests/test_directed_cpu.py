"""CPU: the directed batches of tests/directed.py cover what they claim (every tap phase pair, sign,
edge contact and corner per coverage key; the group word counts at the kernel's switch points), on
textured references, pass the upload validation and plan into the intended launch modes; and the
host check that alone keeps field-MC and chroma reads inside the planes is pinned."""
import numpy as np
import pytest

import directed as D
from test_gpu_parity import _inside
from tiny_mp2v_dec_amd import _lib
from tiny_mp2v_dec_amd import records as R

SWEEP_SIZES = [(128, 64), (144, 80)]
WORD_SIZES = [(128, 32), (80, 32)]
LONG_SIZE = (1040, 32)
ROW_WIDTH_SIZES = [(16, 16), (32, 32), (48, 48), (64, 16), (80, 48), (112, 32), (144, 48), (208, 32)]


def _size_id(s):
    return "%dx%d" % s


def _equal_pair_shares(a):
    a = a.astype(np.int16)
    return float((a[:, 1:] == a[:, :-1]).mean()), float((a[1:] == a[:-1]).mean())


def _assert_textured_references(frames, pics, what):
    """Every plane of every picture used as a reference: no pixel 0 or 255, at most 0.10 of the
    horizontally / vertically adjacent pairs equal."""
    refs = sorted({int(s) for s in np.concatenate([pics["fwd_slot"], pics["bwd_slot"]]) if s >= 0})
    assert refs
    for p in refs:
        for k in range(3):
            a = frames[p][k]
            eh, ev = _equal_pair_shares(a)
            print("%s picture %d plane %d: range %d..%d, equal pairs h %.3f v %.3f" % (what, p, k, a.min(), a.max(), eh, ev))
            assert a.min() > 0 and a.max() < 255, (what, p, k)
            assert eh <= 0.10 and ev <= 0.10, (what, p, k, eh, ev)


@pytest.mark.parametrize("cf", [1, 2, 3])
@pytest.mark.parametrize("size", SWEEP_SIZES, ids=_size_id)
def test_sweep_coverage_is_complete(cf, size):
    """Each of the 35 keys (7 tap modes x 5 MC types) holds all 64 (mvx mod 32, mvy & 1) pairs and
    all 64 (mvy mod 32, mvx & 1) pairs, both signs of both components, the four {-1, -3} vectors,
    every edge contact with and without the half-pel flag, the four corners with the zero and the
    longest vector, and mvx = -1 in the last column / mvy = -1 in the last row (chroma right and
    bottom edge with chroma half-pel)."""
    s = D.mc_sweep(size[0], size[1], cf)
    cov = s.coverage
    print("\n%dx%d cf %d: %d pictures\n%s" % (size[0], size[1], cf, len(s.pics), D.coverage_table(cov)))
    mbw, mbh = size[0] // 16, size[1] // 16
    for key in D.KEYS:
        c, name = cov[key], D.key_name(key)
        assert len(c["xphase"]) == 64 and len(c["yphase"]) == 64, name
        assert c["xphase"] == {(a, b) for a in range(32) for b in range(2)}, name
        assert {-1, 1} <= c["sx"] and {-1, 1} <= c["sy"], name
        assert {(-1, -1), (-1, -3), (-3, -1), (-3, -3)} <= c["vecs"], name
        frame = key[1] == 0
        want = {"T0", "T1", "B0", "B1"} | ({"L0", "L1", "R0", "R1"} if frame else set())
        assert want <= {n for pl, n in c["contacts"] if pl == 0}, (name, c["contacts"])
        # chroma right / bottom edge with the chroma half-pel flag
        for pl in (1, 2):
            assert {(pl, "R1"), (pl, "B1")} <= c["contacts"], (name, pl)
        for cx in (0, mbw - 1):
            for cy in (0, mbh - 1):
                assert {(cx, cy, "zero"), (cx, cy, "far")} <= c["corners"], (name, cx, cy)
        assert {"last column mvx -1", "last row mvy -1"} <= c["corners"], name


@pytest.mark.parametrize("cf", [1, 2, 3])
@pytest.mark.parametrize("size", SWEEP_SIZES, ids=_size_id)
def test_sweep_references_are_textured_and_launch_modes(cf, size):
    """The sweep's two references (textured I and P pictures) in the oracle's frames; the batch
    passes the upload validation; decoded as two batches (everything up to the one-direction B
    pictures, then the two-direction B pictures) the P and one-direction B pictures run in P
    launches (mode 1) and the two-direction B pictures in a B launch (mode 2); as one batch the
    backward-only B pictures share their level with the two-direction ones, a mixed launch (3)."""
    w, h = size
    s = D.mc_sweep(w, h, cf)
    frames = D.expected_frames(("sweep", w, h, cf), w, h, cf, s.pics, s.mbs, s.coefs)
    _assert_textured_references(frames, s.pics, "sweep")
    n = len(s.pics)
    kinds = []
    for p in range(n):
        t = int(s.pics[p]["picture_coding_type"])
        uf, ub = D.picture_uses(s.pics, s.mbs, p)
        kinds.append("I" if t == 1 else ("P" if t == 2 else ("B2" if uf and ub else "B1")))
    assert kinds[:2] == ["I", "P"] and {"P", "B1", "B2"} <= set(kinds)
    assert all(k == "B2" for k in kinds[s.first_two_dir:]) and "B2" not in kinds[:s.first_two_dir]
    a, b = D.split_batch(s.pics, s.mbs, s.coefs, s.first_two_dir)
    of_a, modes_a = R.plan_batch(w, h, cf, n, *a)
    assert modes_a[of_a[0]] == 0
    assert all(modes_a[of_a[p]] == 1 for p in range(1, s.first_two_dir))
    of_b, modes_b = R.plan_batch(w, h, cf, n, *b)
    assert all(modes_b[of_b[p]] == 2 for p in range(len(b[0])))
    of_pic, modes = R.plan_batch(w, h, cf, n, s.pics, s.mbs, s.coefs)
    for p in range(n):
        m = modes[of_pic[p]]
        bwd_only_b = kinds[p] == "B1" and D.picture_uses(s.pics, s.mbs, p)[1]
        assert m == {"I": 0, "P": 1, "B1": 3 if bwd_only_b else 1, "B2": 3}[kinds[p]], (p, kinds[p], m)


@pytest.mark.parametrize("cf", [1, 2, 3])
def test_sweep_shows_a_tap_one_half_pel_or_one_field_off(cf):
    """What the textured references are for: in every coverage key, a tap moved by one half-pel
    in x or in y, or reading the other field, changes the oracle's picture inside that MB (on the
    mostly flat, clipped pictures of random_batch about half such errors give the same bytes).
    The floor: with at most a tenth of adjacent reference pixels equal, a one-direction tap moved
    by half a pel changes most of its bytes; in a bidirectional MB the other direction's average
    keeps about half of the +-1 changes, so at least a quarter of the tap's bytes must differ."""
    w, h = SWEEP_SIZES[0]
    s = D.mc_sweep(w, h, cf)
    exp = D.expected_frames(("sweep", w, h, cf), w, h, cf, s.pics, s.mbs, s.coefs)
    n, per = len(s.pics), (w // 16) * (h // 16)
    _, _, bw, bh = D.plane_dims(w, h, cf)
    seen, low = set(), 1.0
    for p in range(1, n):
        for i in range(p * per, (p + 1) * per):
            for key, r, sdir, vx, vy, field, fs in D.mb_taps(s.pics, s.mbs, p, i):
                if key in seen:
                    continue
                x, y = int(s.mbs["x"][i]), int(s.mbs["y"][i])
                muts = [(dx, dy, fs) for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1))
                        if _inside(w, h, cf, x, y, vx + dx, vy + dy, field, fs)]
                muts = [m for m in muts if m[0]][:1] + [m for m in muts if m[1]][:1]
                if field and _inside(w, h, cf, x, y, vx, vy, field, fs ^ 1):
                    muts.append((0, 0, fs ^ 1))
                if len(muts) < (3 if field else 2):
                    continue
                seen.add(key)
                for dx, dy, nfs in muts:
                    mbs = s.mbs.copy()
                    mbs["mv"][i, r, sdir] = (vx + dx, vy + dy)
                    if nfs != fs:
                        mbs["flags"][i] ^= _lib.mb_fs_bit(r, sdir)
                    sub = D._P(w, h, cf, s.pics[sorted({0, 1, p})], mbs, s.coefs)
                    sub.npics = n  # slots
                    from helpers import oracle_frames
                    got = oracle_frames(sub)[p]
                    for k in range(3):
                        a = got[k][y * bh[k]:(y + 1) * bh[k], x * bw[k]:(x + 1) * bw[k]]
                        b = exp[p][k][y * bh[k]:(y + 1) * bh[k], x * bw[k]:(x + 1) * bw[k]]
                        # (a half-pel step of the luma vector can leave the chroma vector as it was)
                        if k == 0 or cf == 3:
                            share = float((a != b).mean()) * (2 if field else 1)  # a field tap: half the rows
                            low = min(low, share)
                            assert share > 0.25, (D.key_name(key), p, x, y, (dx, dy, nfs), k, share)
    print("cf %d: smallest share of the tap's bytes changed by a mutation: %.2f" % (cf, low))
    assert seen == set(D.KEYS)


@pytest.mark.parametrize("cf", [1, 2, 3])
@pytest.mark.parametrize("kind", ["I", "P", "B"])
@pytest.mark.parametrize("size", WORD_SIZES, ids=_size_id)
def test_word_count_batches_hit_the_switch_points(cf, kind, size):
    """Full groups hold every required total (P/B: some again with an intra MB in the group), the
    one-MB trailing groups of the 80-wide rows theirs; at most 5 % of the oracle's output pixels
    are 0 or 255; the anchors are textured; the launches are the kind's."""
    w, h = size
    pics, mbs, coefs = D.word_count_batch(w, h, cf, kind)
    groups = [g for p in range(len(pics)) for g in D.group_totals(w, h, pics, mbs, p)
              if int(pics[p]["picture_coding_type"]) == {"I": 1, "P": 2, "B": 3}[kind] and (kind == "I" or p > 0)]
    full = {t for nmb, t, intra in groups if nmb == 4}
    print("\n%dx%d cf %d %s: %d pictures, full-group totals %s" % (w, h, cf, kind, len(pics), sorted(full)))
    assert set(D.required_totals(cf, kind)) <= full
    T, Rr = D.PREFETCH_WORDS[kind][cf], D.ROUND_WORDS[kind]
    assert max(full) == 4 * D.NB[cf] * 64 and {T, T + Rr} <= full
    if kind != "I":
        with_intra = {t for nmb, t, intra in groups if nmb == 4 and intra}
        assert {T, T + 1, T + Rr, 4 * D.NB[cf] * 64} <= with_intra
    if w % 64 == 16:
        trail = {t for nmb, t, intra in groups if nmb == 1}
        assert set(D.required_trailing_totals(cf, kind)) <= trail
    else:
        assert all(nmb == 4 for nmb, _, _ in groups)
    assert (pics["W"] == 16).all() and (np.abs(coefs[(coefs >> 30) == 0].astype(np.uint16).view(np.int16)) <= 8).all()
    frames = D.expected_frames(("words", w, h, cf, kind), w, h, cf, pics, mbs, coefs)
    px = np.concatenate([pl.reshape(-1) for f in frames for pl in f])
    sat = float(((px == 0) | (px == 255)).mean())
    print("saturated share %.4f" % sat)
    assert sat <= 0.05
    if kind != "I":
        _assert_textured_references(frames, pics, "words")
    of_pic, modes = R.plan_batch(w, h, cf, len(pics), pics, mbs, coefs)
    want = {"I": {0}, "P": {0, 1}, "B": {0, 1, 2}}[kind]
    assert set(modes.tolist()) == want
    assert modes[of_pic[len(pics) - 1]] == max(want)


@pytest.mark.parametrize("cf", [1, 3])
def test_long_vector_batch(cf):
    """+-2047 at the two ends of a 65-MB row, stepped through between, on textured anchors."""
    w, h = LONG_SIZE
    pics, mbs, coefs = D.long_vector_batch(w, h, cf)
    R.plan_batch(w, h, cf, len(pics), pics, mbs, coefs)
    n = (w // 16) * (h // 16)
    for p in (2, 3):
        vx = mbs["mv"][p * n:p * n + w // 16, 0, 0, 0].astype(int)
        assert vx[0] == 2047 and vx[-1] == -2047 and (np.diff(vx) < 0).all()
    bx = mbs["mv"][3 * n:3 * n + w // 16, 0, 1, 0].astype(int)
    assert bx.max() >= 1983 and bx.min() <= -1984
    frames = D.expected_frames(("long", w, h, cf), w, h, cf, pics, mbs, coefs)
    _assert_textured_references(frames, pics, "long")


@pytest.mark.parametrize("cf", [1, 2, 3])
@pytest.mark.parametrize("size", ROW_WIDTH_SIZES, ids=_size_id)
def test_row_width_batches_validate(cf, size):
    """mbw 1, 2, 3, 4, 5, 7, 9, 13: every remainder mod 4, and rows narrower than one group."""
    w, h = size
    pics, mbs, coefs = D.row_width_batch(w, h, cf)
    R.plan_batch(w, h, cf, 5, pics, mbs, coefs)
    a, b = D.split_batch(pics, mbs, coefs, 3)
    R.plan_batch(w, h, cf, 5, *a)
    R.plan_batch(w, h, cf, 5, *b)
    assert {(w // 16) % 4 for w, _ in ROW_WIDTH_SIZES} == {0, 1, 2, 3}


# ---- the batches of tests/test_gpu_limits.py ---------------------------------------------------------

LIMIT_W, LIMIT_W1, LIMIT_T, LIMIT_T1 = (16384, 32), (16368, 32), (32, 16384), (16, 16384)


@pytest.mark.parametrize("cf", [1, 2, 3])
@pytest.mark.parametrize("size", [LIMIT_W, LIMIT_W1, LIMIT_T, LIMIT_T1], ids=_size_id)
def test_limit_row_width_batches(cf, size):
    """row_width_batch at the limit sizes passes the upload validation and plans into I, P and B
    (or mixed) launches; its records reach MB column 1023 (1022 at 16368) or MB row 1023, and
    hold intra, forward, backward, bidirectional and field-MC MBs in the last eight MBs' columns
    or rows."""
    w, h = size
    pics, mbs, coefs = D.row_width_batch(w, h, cf)
    of_pic, modes = R.plan_batch(w, h, cf, 5, pics, mbs, coefs)
    assert modes[of_pic[0]] == 0 and modes[of_pic[1]] == 1 and {int(modes[of_pic[p]]) for p in (2, 3, 4)} <= {2, 3}
    assert int(mbs["x"].max()) == w // 16 - 1 and int(mbs["y"].max()) == h // 16 - 1
    far = mbs[(mbs["x"] >= w // 16 - 8) & (mbs["y"] >= h // 16 - 8)]
    fl = far["flags"].astype(np.int64)
    assert (fl & _lib.MB_INTRA).any() and (fl & _lib.MB_FIELD_MC).any()
    inter = fl[(fl & _lib.MB_INTRA) == 0] & (_lib.MB_FWD | _lib.MB_BWD)
    assert {_lib.MB_FWD, _lib.MB_BWD, _lib.MB_FWD | _lib.MB_BWD} <= set(inter.tolist())


@pytest.mark.parametrize("cf", [1, 2, 3])
@pytest.mark.parametrize("size", [LIMIT_W, LIMIT_W1], ids=_size_id)
def test_limit_long_vector_batch(cf, size):
    """+-(2 * (width - 16) - 1) at the two ends of the row (32735 at 16384: int16's end but 32),
    stepped through between, frame MC in row 0 and field MC in row 1, forward in the P picture and
    in both directions in the B picture, on textured anchors."""
    w, h = size
    pics, mbs, coefs = D.long_vector_batch(w, h, cf)
    of_pic, modes = R.plan_batch(w, h, cf, len(pics), pics, mbs, coefs)
    assert [int(modes[of_pic[p]]) for p in range(4)] == [0, 1, 1, 2]
    n, mbw, far = (w // 16) * (h // 16), w // 16, 2 * (w - 16) - 1
    for p in (2, 3):
        for row in (0, 1):
            m = mbs[p * n + row * mbw:p * n + (row + 1) * mbw]
            assert ((m["flags"] & _lib.MB_FIELD_MC) != 0).all() == (row == 1)
            fwd = (m["flags"] & _lib.MB_FWD) != 0
            vx = m["mv"][:, 0, 0, 0].astype(int)[fwd]
            assert vx[0] == far and (np.diff(vx) < 0).all() and vx[-1] <= -far + 64, (p, row)
    bx = mbs["mv"][3 * n:4 * n, 0, 1, 0].astype(int)
    assert bx.max() >= far - 64 and bx.min() <= -far + 63
    frames = D.expected_frames(("long", w, h, cf), w, h, cf, pics, mbs, coefs)
    _assert_textured_references(frames, pics, "long")


@pytest.mark.parametrize("cf", [1, 2, 3])
@pytest.mark.parametrize("size", [LIMIT_T, (48, 4128)], ids=_size_id)
def test_limit_long_vertical_batch(cf, size):
    """Per coverage key (7 tap modes x 5 MC types), recomputed from the records: the largest and
    the smallest mvy.  The stepped vector loses 2 * far / (mbh - 1) per MB row, and every key
    comes round within 24 rows of either end (frame / field alternate, the MB kinds of the
    two-direction picture have period 3, the field selects period 8), so each key must hold a
    vector within 48 / (mbh - 1) of the longest legal one in both signs; the longest itself
    (+-32735 frame, +-16367 field at 16384 lines) is applied in row 0 and in the last row."""
    w, h = size
    pics, mbs, coefs = D.long_vertical_batch(w, h, cf)
    of_pic, modes = R.plan_batch(w, h, cf, len(pics), pics, mbs, coefs)
    assert [int(modes[of_pic[p]]) for p in range(6)] == [0, 1, 1, 1, 3, 3]
    cov = D.long_vertical_coverage(w, h, pics, mbs)
    mbh = h // 16
    print("\n%dx%d cf %d: largest / smallest mvy per key" % (w, h, cf))
    for key in D.KEYS:
        far = D.long_vertical_far(h, key[1] != 0)
        hi, lo = cov[key]
        print("%-40s %+6d %+6d of +-%d" % (D.key_name(key), hi, lo, far))
        assert hi <= far and lo >= -far
        assert hi >= far * (1 - 48 / (mbh - 1)) and lo <= -far * (1 - 48 / (mbh - 1)), D.key_name(key)
    for t in (0, 1, 2):  # the P loop's pictures: the longest vector itself, frame and field
        assert cov[(t, 0)] == (D.long_vertical_far(h, False), -D.long_vertical_far(h, False))
        assert max(cov[(t, c)][0] for c in (1, 2, 3, 4)) == D.long_vertical_far(h, True)
        assert min(cov[(t, c)][1] for c in (1, 2, 3, 4)) == -D.long_vertical_far(h, True)
    if h == 16384:
        assert D.long_vertical_far(h, False) == 32735 and D.long_vertical_far(h, True) == 16367
    frames = D.expected_frames(("vertical", w, h, cf), w, h, cf, pics, mbs, coefs)
    _assert_textured_references(frames, pics, "vertical")


@pytest.mark.parametrize("cf", [1, 2, 3])
@pytest.mark.parametrize("case", [LIMIT_W + (128, 32), LIMIT_T + (32, 64)], ids=lambda c: "%dx%d" % c[:2])
def test_limit_corner_sweep_coverage(case, cf):
    """sweep_coverage restricted to the window at the far corner (the last 8 MB columns of
    16384 x 32, the last 4 MB rows of 32 x 16384): each of the 35 keys holds all 64 x-phase and all
    64 y-phase pairs and both signs, and touches the picture's bottom edge (frame MC: and its right
    edge) with and without the half-pel flag, in luma and, with the chroma half-pel flag, in
    chroma; the anchors are textured over the whole plane; the batch passes the upload validation."""
    w, h, sw, sh = case
    s = D.corner_sweep(w, h, cf, sw, sh)
    R.plan_batch(w, h, cf, len(s.pics), s.pics, s.mbs, s.coefs)
    assert s.window == (w // 16 - sw // 16, h // 16 - sh // 16)
    for key in D.KEYS:
        c, name = s.coverage[key], D.key_name(key)
        assert c["xphase"] == c["yphase"] == {(a, b) for a in range(32) for b in range(2)}, name
        assert {-1, 1} <= c["sx"] and {-1, 1} <= c["sy"], name
        want = {"B0", "B1"} | ({"R0", "R1"} if key[1] == 0 else set())
        assert want <= {n for pl, n in c["contacts"] if pl == 0}, (name, c["contacts"])
        for pl in (1, 2):
            assert {(pl, "R1"), (pl, "B1")} <= c["contacts"], (name, pl)
    frames = D.expected_frames(("corner", w, h, cf), w, h, cf, s.pics, s.mbs, s.coefs)
    _assert_textured_references(frames, s.pics, "corner")


@pytest.mark.parametrize("cf", [1, 2, 3])
@pytest.mark.parametrize("kind", ["I", "P", "B"])
def test_limit_word_count_batch(cf, kind):
    """At 16384 x 16 the 256 groups of the one row hold every required total."""
    w, h = 16384, 16
    pics, mbs, coefs = D.word_count_batch(w, h, cf, kind)
    R.plan_batch(w, h, cf, len(pics), pics, mbs, coefs)
    p = len(pics) - 1
    assert int(pics[p]["picture_coding_type"]) == {"I": 1, "P": 2, "B": 3}[kind]
    groups = D.group_totals(w, h, pics, mbs, p)
    assert len(groups) == 256 and all(nmb == 4 for nmb, _, _ in groups)
    assert set(D.required_totals(cf, kind)) <= {t for _, t, _ in groups}


@pytest.mark.parametrize("size,cf", [((320, 288), 3), ((336, 256), 1), ((320, 272), 2)])
def test_sparse_frame_expected_is_the_oracles_frame(size, cf):
    """sparse_frame_expected (zero-vector MBs from their definition, the directed MBs alone through
    the oracle) gives the bytes the oracle gives on the whole batch, at sizes where that is cheap:
    what tests/test_gpu_limits.py compares the 16384 x 16384 frame with."""
    from helpers import SlotOracle
    w, h = size
    pics, mbs, coefs, directed = D.sparse_frame_batch(w, h, cf)
    R.plan_batch(w, h, cf, 4, pics, mbs, coefs)
    full, short = SlotOracle(w, h, cf, 4), SlotOracle(w, h, cf, 4)
    sb = int(full.g.slot_bytes)
    full.pool[:2 * sb] = short.pool[:2 * sb] = D.textured_bytes(np.random.default_rng(5), 2 * sb)
    full.decode(pics, mbs, coefs)
    D.sparse_frame_expected(short, pics, mbs, coefs, directed)
    for s in range(4):
        for a, b in zip(full.planes(s), short.planes(s)):
            assert np.array_equal(a, b), s
    assert not np.array_equal(full.planes(2)[0], full.planes(0)[0])  # the directed MBs changed something


def test_sparse_frame_batch_at_the_largest_size():
    """At 16384 x 16384, 4:4:4: the batch passes the upload validation as one mixed launch; the
    directed MBs sit in the four corners and in the last MB row, hold frame and field MC, all three
    direction kinds and residuals, and the two longest vectors; some tap reads the last tile band
    of the Cr plane (rows from 16380), the end of the tile slot."""
    w, h, cf = 16384, 16384, 3
    pics, mbs, coefs, directed = D.sparse_frame_batch(w, h, cf)
    assert R.plan_batch(w, h, cf, 4, pics, mbs, coefs)[1].tolist() == [3]
    assert _lib.geometry(w, h, cf)[3] == 805306368
    n = 1 << 20
    for p in range(2):
        d = mbs[directed[p]]
        corners = {(int(x) >= 512, int(y) >= 512) for x, y in zip(d["x"], d["y"])}
        assert len(corners) == 4 and (d["y"] == 1023).sum() > 200
        fl = d["flags"].astype(np.int64)
        assert (fl & _lib.MB_FIELD_MC).any() and not (fl & _lib.MB_FIELD_MC).all() and (d["ncoef"] > 0).sum() > 100
        if p:
            assert {int(f) & 6 for f in fl} == {2, 4, 6}
        rest = np.ones(n, bool)
        rest[directed[p] - p * n] = False
        m = mbs[p * n:(p + 1) * n][rest]
        assert not m["mv"].any() and not m["ncoef"].any() and (m["flags"] == (2 if p == 0 else 6)).all()
        last_rows = 0
        for i in directed[p]:
            f = int(mbs["flags"][i])
            field = bool(f & _lib.MB_FIELD_MC)
            for r in range(2 if field else 1):
                for s in range(2):
                    if f & (_lib.MB_FWD, _lib.MB_BWD)[s]:
                        vx, vy = (int(v) for v in mbs["mv"][i, r, s])
                        fs = 1 if f & _lib.mb_fs_bit(r, s) else 0
                        y1 = D.tap_rect(w, h, cf, 2, int(mbs["x"][i]), int(mbs["y"][i]), vx, vy, field, fs)[3]
                        last_rows += y1 >= h - 4
        assert last_rows > 0
    assert tuple(mbs["mv"][0, 0, 0]) == (32735, 32735) and tuple(mbs["mv"][n - 1, 0, 0])[0] == -32736


def _one_mb_batch(w, h, cf, x, y, field, fs, vec):
    """An I picture and a P picture whose MB (x, y) applies `vec` (field MC: as both vectors, with
    field select fs); every other MB the zero vector."""
    B = D._Builder(w, h, cf, 1)
    B.textured_i_picture()
    B.picture(2, 0)
    for _ in range(B.mbw * B.mbh):
        mv = np.zeros((2, 2, 2), np.int16)
        flags = _lib.MB_FWD
        if B.pos() == (x, y):
            mv[:, 0] = vec
            if field:
                flags |= _lib.MB_FIELD_MC | (_lib.mb_fs_bit(0, 0) | _lib.mb_fs_bit(1, 0) if fs else 0)
        B.mb(flags, {}, 2, mv)
    return B.finish()


def _accepts(w, h, cf, batch):
    try:
        R.validate_batch(w, h, cf, 2, *batch)
        return True
    except _lib.Mp2vgError as e:
        assert "reads outside the reference" in str(e)
        return False


@pytest.mark.parametrize("cf", [1, 2, 3])
@pytest.mark.parametrize("fs", [0, 1])
def test_field_vectors_at_the_field_edges(cf, fs):
    """Field MC (vertical components in field units): the vector whose first row is the field's
    first row, or whose last row is the field's last row, is accepted for each field select, and
    one half-pel further is refused.  The kernel's row offsets are not clamped, so this host check
    is the only guard."""
    w, h = 64, 48
    for x, y in ((1, 0), (2, 1), (0, 2)):
        top, bottom = -16 * y, h - 16 - 16 * y
        for vy, ok in ((top, True), (top - 1, False), (top + 1, True), (bottom, True), (bottom + 1, False),
                       (bottom - 1, True)):
            assert _inside(w, h, cf, x, y, 0, vy, True, fs) == ok
            assert _accepts(w, h, cf, _one_mb_batch(w, h, cf, x, y, True, fs, (0, vy))) == ok, (x, y, vy)
    # horizontally a field vector is bounded as a frame vector
    assert _accepts(w, h, cf, _one_mb_batch(w, h, cf, 1, 1, True, fs, (-32, 0)))
    assert not _accepts(w, h, cf, _one_mb_batch(w, h, cf, 1, 1, True, fs, (-33, 0)))
    assert _accepts(w, h, cf, _one_mb_batch(w, h, cf, 1, 1, True, fs, (2 * (w - 32), 0)))
    assert not _accepts(w, h, cf, _one_mb_batch(w, h, cf, 1, 1, True, fs, (2 * (w - 32) + 1, 0)))


@pytest.mark.parametrize("cf", [1, 2, 3])
def test_no_vector_leaves_only_the_chroma_plane(cf):
    """A vector whose luma reads stay inside but whose chroma reads (after the arithmetic >> 1)
    leave the plane would be guarded by the host check alone.  No chroma format has one: with a =
    mv >> 1 the luma bound a + (mv & 1) <= 2M gives ceil(a / 2) <= M, the chroma bound, and a >=
    -2N gives a >> 1 >= -N (4:2:0 in both axes, 4:2:2 horizontally; 4:4:4 chroma is luma).  Shown
    here by enumeration, frame and field MC, every MB of a 64x48 picture; and the upload accepts
    the extreme luma-legal vectors of the edge MBs, whose chroma taps touch the plane edges."""
    w, h = 64, 48
    for field in (False, True):
        for fs in ((0, 1) if field else (0,)):
            for x in range(w // 16):
                for y in range(h // 16):
                    for vx in range(-2 * w, 2 * w + 1):
                        r = D.tap_rect(w, h, cf, 0, x, y, vx, 0, field, fs)
                        assert (r[0] >= 0 and r[1] <= w - 1) == _inside(w, h, cf, x, y, vx, 0, field, fs)
                    for vy in range(-2 * h, 2 * h + 1):
                        r = D.tap_rect(w, h, cf, 0, x, y, 0, vy, field, fs)
                        assert (r[2] >= 0 and r[3] <= h - 1) == _inside(w, h, cf, x, y, 0, vy, field, fs)
    for x, y, vec in ((3, 2, (-96, -64)), (3, 2, (-95, -63)), (0, 0, (96, 64)), (0, 0, (95, 63)),
                      (3, 0, (-1, 63)), (0, 2, (95, -1))):
        assert _accepts(w, h, cf, _one_mb_batch(w, h, cf, x, y, False, 0, vec)), (x, y, vec)
    for x, y, vec in ((3, 2, (-97, 0)), (3, 2, (1, 0)), (3, 2, (0, 1)), (0, 0, (97, 0)), (0, 0, (0, 65)), (0, 0, (-1, 0))):
        assert not _accepts(w, h, cf, _one_mb_batch(w, h, cf, x, y, False, 0, vec)), (x, y, vec)
