"""GPU: what a context carries between calls (tests/slot_state.py): the tile flag of every slot
state and tile_convert_kernel on padded rows, odd geometries and its second grid-stride trip;
mp2vg_reserve_slots after create; the placement calibration's slot pointers and batch history; and
the slot readers (download with strides, packed copy, digests) on slots whose padding bytes are
garbage.  Every comparison is array_equal against the C oracle run on the same slot contents
(helpers.SlotOracle) or a numpy twin; tests/test_slot_state_cpu.py asserts the preconditions."""
import ctypes

import numpy as np
import pytest

import directed as D
import directed_sched as DS
import slot_state as S
from helpers import SlotOracle
from tiny_mp2v_dec_amd import _lib
from tiny_mp2v_dec_amd import records as R

pytestmark = pytest.mark.gpu

CFS = pytest.mark.parametrize("cf", [1, 2, 3])
STREAMS = pytest.mark.parametrize("one_stream", [False, True], ids=["two_streams", "one_stream"])
GUARD = 0xA5


def _size_id(s):
    return "%dx%d" % s


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def assert_slots(ctx, exp, slots, what):
    for s in slots:
        got = ctx.download(s)
        for k, e in enumerate(exp.planes(s)):
            assert np.array_equal(got[k], e), (what, "slot", s, "plane", k)


def outside_write(ctx, exp, slot, planes, pad_seed):
    """An outside producer's write of a slot: write_slot, the layout shown by reading the slot back,
    invalidate; the oracle's slot gets the same planes."""
    S.write_slot(ctx, slot, planes, pad_seed)
    assert same(ctx.download(slot), planes), ("slot image layout", slot)
    ctx.invalidate(slot)
    if exp is not None:
        exp.preload(slot, planes)


def pointers(ctx, slots):
    return [ctx.slot_ptr(s) for s in slots]


def build(w, h, cf, spec, seed):
    return DS.build(w, h, cf, spec, seed=seed)[:3]


# ---- a. the full tap sweep on tiles built by conversion --------------------------------------------

@STREAMS
@CFS
@pytest.mark.parametrize("size", S.SWEEP_SIZES, ids=_size_id)
def test_tap_sweep_on_converted_tiles(size, cf, one_stream):
    """mc_sweep's references (pictures 0 and 1) written into slots 0 and 1 from outside, padding
    bytes garbage, and invalidated: every tap mode, MC type, phase, edge contact and corner
    (tests/test_directed_cpu.py asserts the coverage) reads tiles that tile_convert_kernel built from
    frames with padded rows."""
    w, h = size
    s = D.mc_sweep(w, h, cf)
    exp = D.expected_frames(("sweep", w, h, cf), w, h, cf, s.pics, s.mbs, s.coefs)
    n = len(s.pics)
    rest = D.split_batch(s.pics, s.mbs, s.coefs, 2)[1]
    dump = R.plan_dump(w, h, cf, n, *rest, one_stream=one_stream)
    assert sorted(int(x) for x, _t in dump["ext_reads"]) == [0, 1]
    with R.DeviceContext(w, h, cf, slots=n, one_stream=one_stream) as ctx:
        for k in (0, 1):
            outside_write(ctx, None, k, exp[k], 300 + k)
        ctx.upload(*rest)
        ctx.decode()
        ctx.synchronize()
        for p in range(n):
            assert same(ctx.download(p), exp[p]), ("picture", p)


# ---- b. the state matrix ---------------------------------------------------------------------------

MATRIX = [(size, cf, True) for size in S.SIZES for cf in (1, 2, 3)] + [((128, 48), cf, False) for cf in (1, 2, 3)]


@pytest.mark.parametrize("size,cf,sync", MATRIX, ids=["%dx%d-cf%d-%s" % (s + (c, "sync" if y else "no_host_sync"))
                                                        for s, c, y in MATRIX])
def test_state_matrix(size, cf, sync):
    """Batch 1 leaves slots 0-7 in the states of slot_state.STATE_OF_SLOT (S5 and S6 by outside
    writes of random_planes content); batch 2 reads every one of them with a P picture, a
    two-direction and a one-direction B picture, is decoded twice (the first decode converts, the
    second must not need to) and compared; batch 3 reads the same slots again with the directions
    swapped.  Without host synchronisation: S5 is written before batch 1 is decoded (the batch never
    touches slot 5), slot 6 stays as decoded, and batch 2 is uploaded and decoded behind batch 1
    with no wait in between."""
    w, h = size
    (_s1, *b1), (_s2, *b2), (_s3, *b3) = S.matrix_batches(w, h, cf)
    exp = SlotOracle(w, h, cf, S.NSLOTS)
    g = exp.g
    with R.DeviceContext(w, h, cf, slots=S.NSLOTS) as ctx:
        if not sync:
            outside_write(ctx, exp, 5, S.random_planes(g, 55), 56)
        ctx.upload(*b1)
        ctx.decode()
        exp.decode(*b1)
        if sync:
            ctx.synchronize()
            assert_slots(ctx, exp, range(8), "batch 1")
            outside_write(ctx, exp, 5, S.random_planes(g, 55), 56)
            outside_write(ctx, exp, 6, S.random_planes(g, 65), 66)
        ctx.upload(*b2)
        ctx.decode()
        ctx.decode()
        ctx.synchronize()
        exp.decode(*b2)
        assert_slots(ctx, exp, range(S.NSLOTS), "batch 2")
        ctx.upload(*b3)
        ctx.decode()
        ctx.synchronize()
        exp.decode(*b3)
        assert_slots(ctx, exp, range(S.NSLOTS), "batch 3")


# ---- c. growth -------------------------------------------------------------------------------------

@CFS
def test_reserve_after_create(cf):
    """mp2vg_reserve_slots on a context that has decoded: the slots it had keep their addresses,
    contents and tile state (inline tiles, none for the B picture, invalidated after an outside
    write), the new slots read as zero and predict as zero, a batch uploaded before the growth is
    decoded after it, and the digests of old and new slots are the host twin's; across three block
    boundaries (5 -> 20 -> 33 -> 49 slots)."""
    w, h = S.GROW_SIZE
    a, b, c, d = [build(w, h, cf, spec, 7300 + 10 * i + cf) for i, spec in enumerate(S.growth_specs())]
    exp = SlotOracle(w, h, cf, 5)
    with R.DeviceContext(w, h, cf, slots=5) as ctx:
        ctx.upload(*a)
        ctx.decode()
        ctx.synchronize()
        exp.decode(*a)
        assert_slots(ctx, exp, range(5), "before the growth")
        outside_write(ctx, exp, 1, S.random_planes(exp.g, 71), 72)
        old = pointers(ctx, range(5))
        ctx.reserve(20)
        exp.grow(20)
        assert pointers(ctx, range(5)) == old
        assert_slots(ctx, exp, range(20), "after reserve(20)")
        assert not any(p.any() for s in range(5, 20) for p in ctx.download(s))
        for n in (20, 7, 1):  # at or below the current size: nothing changes
            ctx.reserve(n)
        old = pointers(ctx, range(20))
        assert old[:5] == pointers(ctx, range(5)) and len(set(old)) == 20
        ctx.upload(*b)
        ctx.decode()
        ctx.synchronize()
        exp.decode(*b)
        assert_slots(ctx, exp, range(20), "batch on the grown pool")
        ctx.upload(*c)       # uploaded at 20 slots
        ctx.reserve(33)
        exp.grow(33)
        ctx.decode()         # decoded at 33
        ctx.synchronize()
        exp.decode(*c)
        assert pointers(ctx, range(20)) == old
        assert_slots(ctx, exp, range(33), "uploaded before reserve(33)")
        old = pointers(ctx, range(33))
        ctx.upload(*d)       # reads slot 31 (new, zeros) and writes slots 20, 25, 31 and 32
        ctx.reserve(49)
        exp.grow(49)
        ctx.decode()
        ctx.synchronize()
        exp.decode(*d)
        assert pointers(ctx, range(33)) == old and len(set(pointers(ctx, range(49)))) == 49
        assert_slots(ctx, exp, range(49), "uploaded before reserve(49)")
        mixed = [48, 0, 32, 1, 20, 4, 33, 16, 31, 5]
        assert [int(x) for x in ctx.digests(mixed)] == [R.planes_digest(exp.planes(s)) for s in mixed]
        with pytest.raises(_lib.Mp2vgError):
            ctx.slot_ptr(49)


# ---- d. calibration --------------------------------------------------------------------------------

def _two_more_ordinary_batches(ctx, exp, w, h, cf, nslots, ptrs):
    for i, spec in enumerate(S.ordinary_specs()):
        batch = build(w, h, cf, spec, 7500 + i)
        ctx.upload(*batch)
        ctx.decode()
        ctx.synchronize()
        exp.decode(*batch)
        assert ctx.placement() == ([], -1), ("calibrated at a later decode", i)
        assert pointers(ctx, range(nslots)) == ptrs, ("slot pointers moved after the first decode", i)
        assert_slots(ctx, exp, range(4), ("ordinary batch", i))


def test_calibration_is_decided_at_the_first_decode_overwritten_read(monkeypatch):
    """The first batch reads slot 0 from outside and overwrites it, so it is not calibrated
    (test_gpu_sched.py); the pointers fetched after it stay valid: two ordinary batches later the
    calibration still has not run and no slot has moved."""
    monkeypatch.setenv("MP2VG_PLACE_CANDIDATES", "3")
    monkeypatch.setenv("MP2VG_PLACE_MIN_MB", "0")
    w, h, cf = 128, 48, 1
    spec = [DS.pic("I", 0), DS.pic("P", 1, 0), DS.pic("B", 2, 0, 1), DS.pic("I", 0), DS.pic("P", 3, 0)]
    pics, mbs, coefs, _ = DS.build(w, h, cf, spec, seed=4400)
    a, b = DS.split(pics, mbs, coefs, 1)
    assert R.plan_dump(w, h, cf, 4, *b)["ext_reads"].tolist() == [[0, 0]]
    exp = SlotOracle(w, h, cf, 4)
    exp.decode(*a)
    with R.DeviceContext(w, h, cf, slots=4) as ctx:
        outside_write(ctx, None, 0, [p.copy() for p in exp.planes(0)], 74)
        ctx.upload(*b)
        ctx.decode()
        ctx.synchronize()
        exp.decode(*b)
        assert ctx.placement() == ([], -1)
        assert_slots(ctx, exp, range(4), "first batch")
        _two_more_ordinary_batches(ctx, exp, w, h, cf, 4, pointers(ctx, range(4)))


def test_calibration_is_decided_at_the_first_decode_small_pool(monkeypatch):
    """A pool below MP2VG_PLACE_MIN_MB at its first decode is not calibrated, and not later either
    when mp2vg_reserve_slots has grown it past the threshold: the pointers fetched after the first
    decode stay the slots' addresses."""
    monkeypatch.setenv("MP2VG_PLACE_CANDIDATES", "3")
    monkeypatch.setenv("MP2VG_PLACE_MIN_MB", "1")
    w, h, cf = 128, 48, 1
    exp = SlotOracle(w, h, cf, 4)
    assert S.pool_bytes(int(exp.g.slot_bytes), [4]) < (1 << 20) <= S.pool_bytes(int(exp.g.slot_bytes), [4, 64])
    first = build(w, h, cf, [DS.pic("I", 0), DS.pic("P", 1, 0), DS.pic("B", 2, 0, 1), DS.pic("P", 3, 1)], 7600)
    with R.DeviceContext(w, h, cf, slots=4) as ctx:
        ctx.upload(*first)
        ctx.decode()
        ctx.synchronize()
        exp.decode(*first)
        assert ctx.placement() == ([], -1)
        ptrs = pointers(ctx, range(4))
        ctx.reserve(64)
        exp.grow(64)
        ptrs += pointers(ctx, range(4, 64))
        assert ptrs[:4] == pointers(ctx, range(4))
        _two_more_ordinary_batches(ctx, exp, w, h, cf, 64, ptrs)
        assert not any(p.any() for s in range(4, 64) for p in ctx.download(s))


@pytest.mark.parametrize("hold", ["0", "1"], ids=["candidates_freed", "candidates_held"])
def test_calibrated_batch_reads_outside_content(monkeypatch, hold):
    """A calibrated first batch (two picture sets) that predicts from an outside-written,
    invalidated slot it never writes, with a B picture read inside the batch: every candidate pool
    starts from the entry tile state, so every slot equals the oracle's.  The pointer fetched after
    that decode is the slot the kernels read: new content written through it is what the next batch
    predicts from, whether the other candidates were held or freed."""
    monkeypatch.setenv("MP2VG_PLACE_CANDIDATES", "3")
    monkeypatch.setenv("MP2VG_PLACE_MIN_MB", "0")
    monkeypatch.setenv("MP2VG_PLACE_HOLD", hold)
    w, h, cf, nslots = 128, 48, 1, 8
    first, second = [build(w, h, cf, spec, 7700 + i) for i, spec in enumerate(S.calibrated_specs())]
    dump = R.plan_dump(w, h, cf, nslots, *first)
    assert len(dump["foot"]) == 2 and len(dump["post"]) == 1 and dump["ext_reads"][:, 0].tolist() == [0]
    exp = SlotOracle(w, h, cf, nslots)
    with R.DeviceContext(w, h, cf, slots=nslots) as ctx:
        outside_write(ctx, exp, 0, S.random_planes(exp.g, 77), 78)
        ctx.upload(*first)
        ctx.decode()
        ctx.synchronize()
        exp.decode(*first)
        ms, kept = ctx.placement()
        assert len(ms) == 6 and 0 <= kept < 3 and all(t > 0 for t in ms)
        assert_slots(ctx, exp, range(nslots), "calibrated batch")
        outside_write(ctx, exp, 0, S.random_planes(exp.g, 79), 80)  # through the pointer as it is now
        ctx.upload(*second)
        ctx.decode()
        ctx.synchronize()
        exp.decode(*second)
        assert ctx.placement() == (ms, kept)
        assert_slots(ctx, exp, range(nslots), "after the calibration")


def test_calibrated_decode_is_one_batch_of_the_history(monkeypatch):
    """The calibration decodes the batch 2 + 2 x 3 times; the caller decoded once: mp2vg_batch_times
    knows one batch (a timed run with its launches), then one more per decode."""
    monkeypatch.setenv("MP2VG_PLACE_CANDIDATES", "3")
    monkeypatch.setenv("MP2VG_PLACE_MIN_MB", "0")
    w, h, cf = 128, 48, 1
    _spec, pics, mbs, coefs, _ = DS.batch("ring5", w, h, cf)
    with R.DeviceContext(w, h, cf, slots=5) as ctx:
        ctx.upload(pics, mbs, coefs)
        ctx.decode()
        ctx.synchronize()
        ms, kept = ctx.placement()
        assert len(ms) == 6 and 0 <= kept < 3
        span, launches = ctx.batch_times(0)
        assert span > 0 and launches and all(t > 0 for t in launches)
        assert ctx.batches_span(0, 0) > 0
        with pytest.raises(_lib.Mp2vgError):
            ctx.batch_times(1)
        ctx.decode()
        ctx.decode()
        ctx.synchronize()
        assert all(ctx.batch_times(back)[0] > 0 for back in range(3))
        with pytest.raises(_lib.Mp2vgError):
            ctx.batch_times(3)


# ---- e. the slot readers ---------------------------------------------------------------------------

def download_strided(ctx, slot, strides):
    bufs = [np.full((ctx.ph[p] + 2, strides[p]), GUARD, np.uint8) for p in range(3)]
    ptrs = (ctypes.c_void_p * 3)(*[b[1:].ctypes.data for b in bufs])
    _lib.check(_lib.lib().mp2vg_download_slot(ctx.h, slot, ptrs, (ctypes.c_int32 * 3)(*strides)), "download_slot")
    return bufs


@CFS
@pytest.mark.parametrize("size", S.READER_SIZES, ids=_size_id)
def test_slot_readers_on_garbage_padding(size, cf):
    """Slots 0 and 1 hold different planes, slot 2 the planes of slot 0 with other padding bytes;
    no padding byte is zero or equal between the slots.  download, download with destination
    strides, the packed copy to the host and to the device, and the digests see the visible planes
    alone and write nothing else."""
    from tiny_mp2v_dec_amd.decoder import _hip_lib
    hip = _hip_lib()
    hip.hipMalloc.argtypes, hip.hipFree.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t], [ctypes.c_void_p]
    w, h = size
    g = S.geometry(w, h, cf)
    A, B = S.random_planes(g, 81), S.random_planes(g, 82)
    packed = {0: np.concatenate([p.reshape(-1) for p in A]), 1: np.concatenate([p.reshape(-1) for p in B])}
    with R.DeviceContext(w, h, cf, slots=3) as ctx:
        for slot, planes, seed in ((0, A, 83), (1, B, 84), (2, A, 85)):
            S.write_slot(ctx, slot, planes, seed)
            assert same(ctx.download(slot), planes), ("download", slot)
        for strides in ([x + 5 for x in ctx.pw], list(ctx.stride)):
            for slot, planes in ((0, A), (1, B)):
                for p, buf in enumerate(download_strided(ctx, slot, strides)):
                    assert np.array_equal(buf[1:-1, :ctx.pw[p]], planes[p]), (strides, slot, p)
                    assert (buf[0] == GUARD).all() and (buf[-1] == GUARD).all() and (buf[:, ctx.pw[p]:] == GUARD).all()
        nbytes = ctx.frame_bytes()
        assert nbytes == len(packed[0])
        dev = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(dev), nbytes + 128) == 0
        for slot in (0, 1):
            host = np.full(nbytes + 128, GUARD, np.uint8)
            ctx.copy_packed(slot, host.ctypes.data + 64, False)
            assert np.array_equal(host[64:64 + nbytes], packed[slot]), ("packed to host", slot)
            assert (host[:64] == GUARD).all() and (host[64 + nbytes:] == GUARD).all()
            got = np.full(nbytes + 128, GUARD, np.uint8)
            assert hip.hipMemcpy(dev.value, got.ctypes.data, got.nbytes, 1) == 0  # host to device
            ctx.copy_packed(slot, dev.value + 64, True)
            assert hip.hipMemcpy(got.ctypes.data, dev.value, got.nbytes, 2) == 0  # device to host
            assert np.array_equal(got[64:64 + nbytes], packed[slot]), ("packed to device", slot)
            assert (got[:64] == GUARD).all() and (got[64 + nbytes:] == GUARD).all()
        assert hip.hipFree(dev) == 0
        dA, dB = R.planes_digest(A), R.planes_digest(B)
        assert dA != dB
        assert [int(x) for x in ctx.digests([1])] == [dB]
        assert [int(x) for x in ctx.digests([1, 0])] == [dB, dA]
        order = [2, 1, 1, 0, 2, 0, 1][::-1] * 43
        assert len(order) > 300
        assert [int(x) for x in ctx.digests(order[:300])] == [(dA, dB, dA)[s] for s in order[:300]]  # the buffers grow
        assert [int(x) for x in ctx.digests([0, 2])] == [dA, dA]  # padding is no part of the digest
        # the last visible byte of a row of each plane, next to the padding
        for p in range(3):
            C = [x.copy() for x in A]
            C[p][ctx.ph[p] // 2, -1] ^= 0x10
            S.write_slot(ctx, 1, C, 86 + p)
            dC = int(ctx.digests([1])[0])
            assert dC == R.planes_digest(C) and dC != dA, ("padding-adjacent byte", p)
            assert np.array_equal(ctx.download(1)[p], C[p])


# ---- f. the conversion's second grid-stride trip ---------------------------------------------------

@pytest.mark.parametrize("cf", [1, 3])
def test_tile_conversion_second_trip(cf):
    """512x528: the luma plane has 33,792 16-B tile chunks, more than tile_convert_kernel's
    128 x 256 threads, so the tiles of the last MB row are built by its second trip; a P and a B
    picture predict from outside content in slots 0 and 1 there (tests/test_slot_state_cpu.py)."""
    w, h = S.TRIP_SIZE
    pics, mbs, coefs = S.trip_batch(cf)
    assert S.last_row_uses(pics, mbs, 0) == (True, False) and S.last_row_uses(pics, mbs, 1) == (True, True)
    exp = SlotOracle(w, h, cf, 4)
    assert exp.g.stride[0] * exp.g.ph[0] > 262144
    with R.DeviceContext(w, h, cf, slots=4) as ctx:
        outside_write(ctx, exp, 0, S.random_planes(exp.g, 91), 92)
        outside_write(ctx, exp, 1, S.random_planes(exp.g, 93), 94)
        ctx.upload(pics, mbs, coefs)
        ctx.decode()
        ctx.synchronize()
        exp.decode(pics, mbs, coefs)
        assert_slots(ctx, exp, range(4), "second trip")
