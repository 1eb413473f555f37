"""CPU: the helpers and the preconditions of tests/test_gpu_slot_state.py (tests/slot_state.py).
Geometry agreement between the oracle and the library for every size used, the oracle run on a
preloaded pool, the pool size of a growth history, and -- recomputed from the dumped plans, never
taken from how a batch was built -- what each batch of the state matrix, the growth test, the
calibration tests and the second-trip test claims about its reads, writes and tile flags."""
import numpy as np
import pytest

import directed as D
import directed_sched as DS
import slot_state as S
from helpers import SlotOracle
from test_gpu_parity import random_batch
from tiny_mp2v_dec_amd import records as R

CFS = pytest.mark.parametrize("cf", [1, 2, 3])


@CFS
def test_geometry_agreement(cf):
    """oracle_geometry and mp2vg_frame_geometry agree for every size the GPU tests use; the padded
    sizes really are padded, and a slot image round-trips with no padding byte zero."""
    for w, h in S.ALL_SIZES:
        g = S.geometry(w, h, cf)
        planes = S.random_planes(g, 1)
        image = S.slot_image(g, planes, 2)
        assert all(np.array_equal(a, b) for a, b in zip(S.image_planes(g, image), planes))
        pads = [image[int(g.plane_off[p]): int(g.plane_off[p]) + g.stride[p] * g.ph[p]]
                .reshape(g.ph[p], g.stride[p])[:, g.pw[p]:] for p in range(3)]
        assert all((q != 0).all() for q in pads)
        for b in planes:
            assert b.min() == 0 and b.max() == 255 and (b[b.shape[0] // 2, : b.shape[1] // 2] == 255).all()
            assert (b[0, 0], b[0, -1], b[-1, 0], b[-1, -1]) == (0, 255, 255, 0)
    g = S.geometry(80, 48, cf)
    assert (g.pw[0], g.stride[0]) == (80, 128) and (g.pw[1], g.stride[1]) == ((80, 128) if cf == 3 else (40, 64))
    g = S.geometry(16, 16, cf)
    assert g.stride[0] == 64 and (g.pw[1], g.stride[1]) == ((16, 64) if cf == 3 else (8, 64))
    g = S.geometry(*S.TRIP_SIZE, cf)
    assert g.stride[0] * g.ph[0] == 270336 > 128 * 256 * 8


@CFS
def test_preloaded_oracle(cf):
    """A 3-picture batch; picture 0's slot alone preloaded into a fresh pool and pictures 1-2
    reconstructed on it give the same frames; preloaded random_planes content gives other frames
    than the zero pool, so the preload is really read."""
    w, h = 96, 64
    pics, mbs, coefs = random_batch(w, h, cf, 3, seed=6100 + cf)
    full = SlotOracle(w, h, cf, 3)
    full.decode(pics, mbs, coefs)
    rest = D.split_batch(pics, mbs, coefs, 1)[1]
    pre = SlotOracle(w, h, cf, 3)
    pre.preload(0, full.planes(0))
    pre.decode(*rest)
    zero = SlotOracle(w, h, cf, 3)
    zero.decode(*rest)
    rnd = SlotOracle(w, h, cf, 3)
    rnd.preload(0, S.random_planes(rnd.g, 61))
    rnd.decode(*rest)
    for s in (1, 2):
        assert all(np.array_equal(a, b) for a, b in zip(pre.planes(s), full.planes(s)))
        assert not all(np.array_equal(a, b) for a, b in zip(rnd.planes(s), zero.planes(s)))
        assert not all(np.array_equal(a, b) for a, b in zip(zero.planes(s), full.planes(s)))
    assert all(np.array_equal(a, b) for a, b in zip(rnd.planes(0), S.random_planes(rnd.g, 61)))
    grown = SlotOracle(w, h, cf, 3)
    grown.preload(2, full.planes(2))
    grown.grow(5)
    assert all(np.array_equal(a, b) for a, b in zip(grown.planes(2), full.planes(2))) and not grown.planes(4)[0].any()


def dump_at(w, h, cf, nslots):
    return lambda pics, mbs, coefs, one=False: R.plan_dump(w, h, cf, nslots, pics, mbs, coefs, one_stream=one)


@CFS
@pytest.mark.parametrize("size", S.SIZES, ids=lambda s: "%dx%d" % s)
def test_state_matrix_plans(size, cf):
    """Batch 1 leaves the states the matrix names (writes: tile flag 1 for the S1 / S6 anchors, 0
    for the S2 anchors and the S3 B picture; S4 and S5 untouched); batches 2 and 3 read all eight
    slots from outside, one group per reading set with two streams and all on set 0 with one,
    convert a B picture inside the batch, and write none of the slots they read from outside."""
    S.check_matrix_plans(*size, cf, dump_at(*size, cf, S.NSLOTS))
    specs = [b[0] for b in S.matrix_batches(*size, cf)]
    readers = {x: set() for x in range(8)}
    for spec in specs[1:]:
        for t, _dst, fwd, bwd, kind in spec:
            for x, used in ((fwd, DS.USES[kind][0]), (bwd, DS.USES[kind][1])):
                if used and x in readers:
                    readers[x].add((t, kind, "fwd" if x == fwd else "bwd"))
    for x in range(8):  # every state: a P picture, a two-direction B both ways, one-direction B both ways
        two = "d" if size == (16, 16) else "fb"
        assert readers[x] >= {("P", "f", "fwd"), ("B", two, "fwd"), ("B", two, "bwd"), ("B", "f", "fwd"),
                              ("B", "b", "bwd")}, (x, readers[x])


@CFS
def test_growth_and_calibration_plans(cf):
    w, h = S.GROW_SIZE
    a, b, c, d = [DS.build(w, h, cf, spec, seed=1, dense=False)[:3] for spec in S.growth_specs()]
    da = dump_at(w, h, cf, 5)(*a)
    assert [int(s) for s, _t in da["writes"]] == [0, 1, 2, 3, 4] and int(da["writes"][4][1]) == 0  # B picture, no tiles
    assert int(da["writes"][0][1]) == 1
    db = dump_at(w, h, cf, 20)(*b)
    assert sorted(int(s) for s, _t in db["ext_reads"]) == [0, 1, 4, 7]
    assert sorted(int(s) for s, _t in db["writes"]) == list(range(5, 20))
    with pytest.raises(RuntimeError):
        dump_at(w, h, cf, 5)(*b)   # the batch needs the grown pool
    dc = dump_at(w, h, cf, 20)(*c)
    assert {1, 4, 13, 15, 19} <= {int(s) for s, _t in dc["ext_reads"]}
    dd = dump_at(w, h, cf, 33)(*d)
    assert {1, 5, 31} <= {int(s) for s, _t in dd["ext_reads"]} and 32 in {int(s) for s, _t in dd["writes"]}
    with pytest.raises(RuntimeError):
        dump_at(w, h, cf, 20)(*d)
    first, second = [DS.build(w, h, cf, spec, seed=1, dense=False)[:3] for spec in S.calibrated_specs()]
    d1 = dump_at(w, h, cf, 8)(*first)
    assert d1["ext_reads"].tolist() == [[0, int(d1["ext_reads"][0][1])]] and len(d1["foot"]) == 2
    assert 0 not in {int(s) for s, _t in d1["writes"]} and [int(s) for _l, s in d1["post"]] == [2]
    d2 = dump_at(w, h, cf, 8)(*second)
    assert [int(s) for s, _t in d2["ext_reads"]] == [0]
    for spec in S.ordinary_specs():
        o = dump_at(w, h, cf, 4)(*DS.build(w, h, cf, spec, seed=1, dense=False)[:3])
        assert not {int(s) for s, _t in o["ext_reads"]} & {int(s) for s, _t in o["writes"]}


@pytest.mark.parametrize("cf", [1, 3])
def test_second_trip_batch(cf):
    """The P picture predicts from slot 0, the B picture from slots 0 and 1, and in each picture's
    last MB row (whose luma tiles only tile_convert_kernel's second trip builds: the first covers
    128 x 256 x 8 = 262,144 luma bytes, 512 of the 528 rows) inter MBs use each reference."""
    pics, mbs, coefs = S.trip_batch(cf)
    d = dump_at(*S.TRIP_SIZE, cf, 4)(pics, mbs, coefs)
    assert sorted(int(s) for s, _t in d["ext_reads"]) == [0, 1]
    assert S.last_row_uses(pics, mbs, 0) == (True, False)
    assert S.last_row_uses(pics, mbs, 1) == (True, True)
    assert (512 * 528 - 128 * 256 * 8) // 512 == 16  # exactly the last MB row is left to the second trip


def test_pool_bytes():
    """Hand-computed: 9,216-B slots (128x48 4:2:0); one block of 4 slots is 4 x 9,216 + 69,632 of
    frames and 4 x 18,432 of tiles; grown to 64 it adds blocks of 16, 16, 16 and 12 slots.  And
    1,000-B slots (tiles 2,048 per slot): 17 slots are blocks of 16 and 1."""
    assert S.pool_bytes(9216, [4]) == 4 * 9216 + 69632 + 4 * 18432 == 180224
    assert S.pool_bytes(9216, [4, 64]) == 64 * 9216 + 5 * 69632 + 64 * 18432 == 2117632
    assert S.pool_bytes(1000, [17]) == 17 * 1000 + 2 * 69632 + 17 * 2048 == 191080
    assert S.pool_bytes(1000, [5, 5, 3, 20]) == 20 * 1000 + 2 * 69632 + 20 * 2048
    # the history counts, not only the size: blocks of 5, 16 and 1 slots against blocks of 16 and 6
    assert S.pool_bytes(1000, [5, 22]) == S.pool_bytes(1000, [22]) + 69632


def test_threshold_straddle():
    """The calibration test's pools: 4 slots below 1 MiB, 4 grown to 64 above it."""
    g = S.geometry(*S.GROW_SIZE, 1)
    assert int(g.slot_bytes) == 9216
    assert S.pool_bytes(9216, [4]) < (1 << 20) <= S.pool_bytes(9216, [4, 64])
