"""GPU parity on directed inputs (tests/directed.py): the full tap phase / edge sweep on textured
references, every row-width class, group word counts at the kernel's switch points, and the
longest vectors across a 65-MB row.  Every plane of every picture byte for byte vs the oracle."""
import numpy as np
import pytest

import directed as D
from tiny_mp2v_dec_amd import records as R

pytestmark = pytest.mark.gpu


def _size_id(s):
    return "%dx%d" % s


def gpu_frames(w, h, cf, nslots, batches):
    """Decode the batches in turn in one context; the frame of every slot."""
    with R.DeviceContext(w, h, cf, slots=nslots) as ctx:
        for pics, mbs, coefs in batches:
            ctx.upload(pics, mbs, coefs)
            ctx.decode()
        ctx.synchronize()
        return [ctx.download(p) for p in range(nslots)]


def assert_frames_equal(got, exp, w, h, cf, pics, mbs, what=""):
    """On a mismatch: the first differing picture, plane and MB, and that MB's coverage keys."""
    _, _, bw, bh = D.plane_dims(w, h, cf)
    for p in range(len(exp)):
        for k in range(3):
            if np.array_equal(got[p][k], exp[p][k]):
                continue
            ys, xs = np.nonzero(got[p][k] != exp[p][k])
            mbx, mby = int(xs[0]) // bw[k], int(ys[0]) // bh[k]
            i = int(pics[p]["mb_first"]) + mby * (w // 16) + mbx
            taps = ["%s mv (%d, %d)" % (D.key_name(t[0]), t[3], t[4]) for t in D.mb_taps(pics, mbs, p, i)]
            pytest.fail("%s picture %d plane %d: %d bytes differ, first at (x %d, y %d) in MB (%d, %d) "
                        "[flags 0x%x, cbp 0x%x, %d words]: %s; got %d, expected %d" %
                        (what, p, k, len(xs), xs[0], ys[0], mbx, mby, int(mbs["flags"][i]), int(mbs["cbp"][i]),
                         int(mbs["ncoef"][i]), taps or "intra", got[p][k][ys[0], xs[0]], exp[p][k][ys[0], xs[0]]))


@pytest.mark.parametrize("cf", [1, 2, 3])
@pytest.mark.parametrize("size", [(128, 64), (144, 80)], ids=_size_id)
def test_mc_phase_and_edge_sweep(cf, size):
    """mc_sweep: every (tap mode, MC type) key with all 64 x-phase and y-phase pairs, both signs,
    the chroma >> 1 vectors, every edge contact and the corners (tests/test_directed_cpu.py asserts
    the coverage), on textured references and mostly without residual.  128x64: 8-MB rows, mates;
    144x80: 9-MB rows, a one-MB trailing group.  Decoded as two batches (the P and one-direction
    B pictures in P launches, the two-direction B pictures in a B launch) and as one batch (the
    backward-only B pictures inside a mixed launch)."""
    w, h = size
    s = D.mc_sweep(w, h, cf)
    exp = D.expected_frames(("sweep", w, h, cf), w, h, cf, s.pics, s.mbs, s.coefs)
    n = len(s.pics)
    got = gpu_frames(w, h, cf, n, D.split_batch(s.pics, s.mbs, s.coefs, s.first_two_dir))
    assert_frames_equal(got, exp, w, h, cf, s.pics, s.mbs, "two batches:")
    got = gpu_frames(w, h, cf, n, [(s.pics, s.mbs, s.coefs)])
    assert_frames_equal(got, exp, w, h, cf, s.pics, s.mbs, "one batch:")


@pytest.mark.parametrize("cf", [1, 2, 3])
@pytest.mark.parametrize("size", [(16, 16), (32, 32), (48, 48), (64, 16), (80, 48), (112, 32), (144, 48), (208, 32)],
                         ids=_size_id)
def test_row_width_classes(cf, size):
    """MB rows of 1, 2, 3, 4, 5, 7, 9 and 13 MBs: every remainder mod the 4-MB group (one-row
    slices, no mates, a partial last group whose tile columns are all stored) and rows narrower
    than one group, at one to three MB rows.  80x48 also as two batches, pictures 0-2 then 3-4:
    the partial group's anchor tiles across a batch boundary."""
    w, h = size
    pics, mbs, coefs = D.row_width_batch(w, h, cf)
    exp = D.expected_frames(("rows", w, h, cf), w, h, cf, pics, mbs, coefs)
    got = gpu_frames(w, h, cf, 5, [(pics, mbs, coefs)])
    assert_frames_equal(got, exp, w, h, cf, pics, mbs)
    if size == (80, 48):
        got = gpu_frames(w, h, cf, 5, D.split_batch(pics, mbs, coefs, 3))
        assert_frames_equal(got, exp, w, h, cf, pics, mbs, "two batches:")


@pytest.mark.parametrize("cf", [1, 2, 3])
@pytest.mark.parametrize("kind", ["I", "P", "B"])
def test_group_word_count_boundaries(cf, kind):
    """Groups of exactly T - 1, T, T + 1, T + 63 .. T + 65, T + R - 1 .. T + R + 1 and the maximum
    4 * NB * 64 coefficient words (T: the prefetch registers' 64 * NCW words, R: a round of the
    second loop, 64 * XW; P/B also 0, 1, 63 .. 65, and groups that hold an intra MB), at 128x32 and
    at 80x32 with its one-MB trailing groups."""
    for w, h in ((128, 32), (80, 32)):
        pics, mbs, coefs = D.word_count_batch(w, h, cf, kind)
        exp = D.expected_frames(("words", w, h, cf, kind), w, h, cf, pics, mbs, coefs)
        got = gpu_frames(w, h, cf, len(pics), [(pics, mbs, coefs)])
        for p in range(len(pics)):  # name the group's word total on a mismatch
            if not all(np.array_equal(got[p][k], exp[p][k]) for k in range(3)):
                print("picture %d group totals: %s" % (p, D.group_totals(w, h, pics, mbs, p)))
        assert_frames_equal(got, exp, w, h, cf, pics, mbs, "%dx%d:" % (w, h))


@pytest.mark.parametrize("cf", [1, 3])
def test_long_vectors_1040_wide(cf):
    """65-MB rows (remainder 1): mvx = +2047 in column 0 down to -2047 in the last column, frame
    and field MC, P and two-direction B, on textured anchors: the tap's tile column and row
    arithmetic over 64 tile columns."""
    w, h = 1040, 32
    pics, mbs, coefs = D.long_vector_batch(w, h, cf)
    exp = D.expected_frames(("long", w, h, cf), w, h, cf, pics, mbs, coefs)
    got = gpu_frames(w, h, cf, len(pics), [(pics, mbs, coefs)])
    assert_frames_equal(got, exp, w, h, cf, pics, mbs)
