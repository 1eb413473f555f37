"""GPU parity on the directed IDCT batches (tests/directed_idct.py): every witness vector of every
saturating node, rail, pass, pair half and lane, in every coded-block slot of the I, P, B and mixed
kernels, in full groups and trailing groups of 1, 2 and 3 MBs, frame and field DCT, for the three
chroma formats; and the dense-then-sparse blocks of the stale-LDS batch.  Every plane of every
picture byte for byte vs the oracle (tests/test_idct_directed_cpu.py shows that the oracle's frames
equal the model's and that every named mutant would change them)."""
import numpy as np
import pytest

import directed as D
import directed_idct as I
from test_gpu_directed import gpu_frames

pytestmark = pytest.mark.gpu

# 128x16: full groups, two slices per workgroup in P/B; 80 / 96 / 112 x 32: a trailing group of 1 / 2 / 3 MBs
SIZES = [(128, 16), (80, 32), (96, 32), (112, 32)]


def _size_id(s):
    return "%dx%d" % s


def assert_blocks_equal(got, exp, bt, what=""):
    """On a mismatch: the block, its place in the kernel and the mutants it witnesses."""
    w, h, cf = bt.width, bt.height, bt.cf
    if all(np.array_equal(got[p][k], exp[p][k]) for p in range(len(exp)) for k in range(3)):
        return
    V = I.vectors()
    _, _, bw, bh = D.plane_dims(w, h, cf)
    for bl in I.batch_blocks(bt):
        plane, x0, y0, ys = I.placement(cf, bl.b, bl.dctf)
        X, Y = bl.x * bw[plane] + x0, bl.y * bh[plane] + y0
        a, b = got[bl.p][plane][Y:Y + 8 * ys:ys, X:X + 8], exp[bl.p][plane][Y:Y + 8 * ys:ys, X:X + 8]
        if not np.array_equal(a, b):
            r, c = [int(t[0]) for t in np.nonzero(a != b)]
            names = sorted({n for n, _, _, v in V.conds if v == bl.vec})
            pytest.fail("%s picture %d MB (%d, %d) block %d [%s, slot %d, MB %d of a group of %d, %s DCT, vector %d]: "
                        "%d bytes differ, first at row %d column %d: got %d, expected %d; witnesses %s" %
                        (what, bl.p, bl.x, bl.y, bl.b, bl.kind, bl.slot, bl.k, bl.gsize, "field" if bl.dctf else "frame",
                         bl.vec, int((a != b).sum()), r, c, a[r, c], b[r, c], names[:12]))
    for p in range(len(exp)):
        for k in range(3):
            assert np.array_equal(got[p][k], exp[p][k]), (what, "outside the coded blocks", p, k)


def _run(bt):
    w, h, cf = bt.width, bt.height, bt.cf
    exp = D.expected_frames(bt.key(), w, h, cf, bt.pics, bt.mbs, bt.coefs)
    n = len(bt.pics)
    got = gpu_frames(w, h, cf, n, [(bt.pics, bt.mbs, bt.coefs)])
    assert_blocks_equal(got, exp, bt, "one batch:")
    if bt.launch != "I":
        got = gpu_frames(w, h, cf, n, D.split_batch(bt.pics, bt.mbs, bt.coefs, bt.first_case_pic))
        assert_blocks_equal(got, exp, bt, "two batches:")


@pytest.mark.parametrize("cf", [1, 2, 3])
@pytest.mark.parametrize("launch", ["I", "P", "B", "mixed"])
@pytest.mark.parametrize("size", SIZES, ids=_size_id)
def test_idct_witnesses(cf, launch, size):
    """The witness vectors in every MB kind, slot and group size of the launch; P, B and mixed once
    more as two batches, the flat anchors first."""
    _run(I.idct_batch(size[0], size[1], cf, launch))


@pytest.mark.parametrize("cf", [1, 2, 3])
@pytest.mark.parametrize("launch", ["I", "P", "B", "mixed"])
def test_stale_lds(cf, launch):
    """512x16: a wave's dense blocks (64 coefficients at +-2047) followed by single-coefficient
    blocks in the same slots: what pass 2 must have zeroed."""
    _run(I.stale_batch(cf, launch))
