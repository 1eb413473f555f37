"""GPU parity on the directed dequantisation / mismatch-control batches (tests/directed_dequant.py):
every value boundary of the dequant arithmetic and every position-63 pair whose toggle shows, in
every block index of every MB kind, in the I, P, B and mixed kernels, for the three chroma formats.
Every plane of every picture byte for byte vs the oracle (tests/test_dequant_cpu.py shows that the
oracle's frames tell every named mutant apart)."""
import numpy as np
import pytest

import directed as D
import directed_dequant as Q
from test_gpu_directed import gpu_frames

pytestmark = pytest.mark.gpu

SIZES = [(128, 16), (128, 32), (80, 32)]


def _size_id(s):
    return "%dx%d" % s


def assert_blocks_equal(got, exp, bt, what=""):
    """On a mismatch: the block, its cell and case labels, and the model's QFS[63] before and
    after the toggle."""
    w, h, cf = bt.width, bt.height, bt.cf
    _, _, bw, bh = D.plane_dims(w, h, cf)
    if all(np.array_equal(got[p][k], exp[p][k]) for p in range(len(exp)) for k in range(3)):
        return
    for bl in Q.batch_blocks(bt):
        plane, bx, by = Q.block_origin(cf, bl.b)
        x0, y0 = bl.x * bw[plane] + bx, bl.y * bh[plane] + by
        a, b = got[bl.p][plane][y0:y0 + 8, x0:x0 + 8], exp[bl.p][plane][y0:y0 + 8, x0:x0 + 8]
        if not np.array_equal(a, b):
            after = bl.Q[63]
            pytest.fail("%s picture %d MB (%d, %d) block %d [%s, k %d, %s words, labels %s]: %d bytes differ; model "
                        "QFS[63] %d before, %d after the toggle" %
                        (what, bl.p, bl.x, bl.y, bl.b, bl.kind, bl.k, bl.src, sorted(bl.labels), int((a != b).sum()),
                         after ^ 1 if bl.toggled else after, after))
    for p in range(len(exp)):
        for k in range(3):
            assert np.array_equal(got[p][k], exp[p][k]), (what, "outside the coded blocks", p, k)


@pytest.mark.parametrize("cf", [1, 2, 3])
@pytest.mark.parametrize("launch", ["I", "P", "B", "mixed"])
@pytest.mark.parametrize("size", SIZES, ids=_size_id)
def test_dequant_and_mismatch_cases(cf, launch, size):
    """128x16: a workgroup's two slices come from two pictures (the other scan, other matrices);
    128x32: they may come from one; 80x32: no mates, a one-MB trailing group.  The P, B and mixed
    batches once more as two batches, the flat anchors first."""
    w, h = size
    bt = Q.dequant_batch(w, h, cf, launch)
    exp = D.expected_frames(bt.key(), w, h, cf, bt.pics, bt.mbs, bt.coefs)
    n = len(bt.pics)
    got = gpu_frames(w, h, cf, n, [(bt.pics, bt.mbs, bt.coefs)])
    assert_blocks_equal(got, exp, bt, "one batch:")
    if launch != "I":
        got = gpu_frames(w, h, cf, n, D.split_batch(bt.pics, bt.mbs, bt.coefs, bt.first_case_pic))
        assert_blocks_equal(got, exp, bt, "two batches:")
