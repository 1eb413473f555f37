"""GPU: the level scheduler end to end (runtime.cpp plan_batch / TilePlan / batch_decode, recon.hip
recon_kernel's unit mapping) on the directed batches of tests/directed_sched.py.  Every test is
bit-exact against the C oracle run sequentially in decode order; tests/test_sched_cpu.py shows that
the oracle is indexed by slot, which makes the prefix method sound, and checks the plans themselves
(hazards, sets, tiles, footprints) without a device."""
import ctypes

import numpy as np
import pytest

import _oracle
import directed_sched as D
from directed_sched import pic
from tiny_mp2v_dec_amd import _lib
from tiny_mp2v_dec_amd import records as R

pytestmark = pytest.mark.gpu

STREAMS = pytest.mark.parametrize("one_stream", [False, True], ids=["two_streams", "one_stream"])
CFS = pytest.mark.parametrize("cf", [1, 2, 3])


class Oracle:
    """The oracle's slots after decoding pics in order (slots start as zeros, like a new context's)."""

    def __init__(self, w, h, cf, pics, mbs, coefs, nslots):
        self.g, self.pool = _oracle.reconstruct(w, h, cf, np.ascontiguousarray(pics), mbs, coefs, nslots)

    def planes(self, s):
        g, base = self.g, s * int(self.g.slot_bytes)
        return [self.pool[base + g.plane_off[p]: base + g.plane_off[p] + g.stride[p] * g.ph[p]]
                .reshape(g.ph[p], g.stride[p])[:, :g.pw[p]] for p in range(3)]


def assert_slots(ctx, exp, slots, what):
    for s in slots:
        got = ctx.download(s)
        for k, e in enumerate(exp.planes(s)):
            assert np.array_equal(got[k], e), (what, "slot", s, "plane", k)


def live_slots(pics):
    return sorted({int(P["dst_slot"]) for P in pics})


@STREAMS
@CFS
@pytest.mark.parametrize("name", sorted(D.DIRECTED))
def test_directed_batches_every_prefix(name, cf, one_stream):
    """Every picture of every directed batch: each prefix pics[:k] is decoded on a fresh context
    and every slot written so far compared, so a picture whose slot the batch overwrites later is
    checked at the prefix that ends at it."""
    for w, h in D.SIZES:
        spec, pics, mbs, coefs, _ = D.batch(name, w, h, cf)
        nslots = D.nslots_of(spec)
        for k in range(1, len(pics) + 1):
            (p1, m1, c1), _rest = D.split(pics, mbs, coefs, k)
            exp = Oracle(w, h, cf, p1, mbs, coefs, nslots)
            with R.DeviceContext(w, h, cf, slots=nslots, one_stream=one_stream) as ctx:
                ctx.upload(p1, m1, c1)
                ctx.decode()
                ctx.synchronize()
                assert_slots(ctx, exp, live_slots(p1), (w, h, "prefix", k))


@CFS
@pytest.mark.parametrize("name", ["ring4", "ring5", "ring_delay", "degenerate_intra", "degenerate_clusters"])
def test_two_batch_splits(name, cf):
    """The ring and degenerate batches as two batches at every split point, two streams, no host
    synchronisation between the decodes: the second batch's external reads (TilePlan.ext_reads)
    find slots whose last writer was a B picture, or an anchor that stored no tiles, and rebuild
    their tiles on the reading set's stream."""
    w, h = D.SIZES[cf - 1]
    spec, pics, mbs, coefs, _ = D.batch(name, w, h, cf)
    nslots = D.nslots_of(spec)
    exp = Oracle(w, h, cf, pics, mbs, coefs, nslots)
    for k in range(1, len(pics)):
        a, b = D.split(pics, mbs, coefs, k)
        with R.DeviceContext(w, h, cf, slots=nslots) as ctx:
            ctx.upload(*a)
            ctx.decode()
            ctx.upload(*b)
            ctx.decode()
            ctx.synchronize()
            assert_slots(ctx, exp, live_slots(pics), ("split", k))


def _cross_set_batches(mirrored):
    """Batch 1: two slot-disjoint components, a short one (I P B B) and a chain of 8 dependent
    launches whose last picture writes slot 7.  Batch 2: a component that reads slot 7 at its
    first launch and then overwrites slot 6, which the chain's last picture read (WAR).  Plain:
    the chain runs on set 1 and batch 2's reader on set 0; mirrored: the chain on set 0 and the
    reader -- behind a decoy component on untouched slots -- on set 1."""
    short = [pic("I", 0), pic("P", 1, 0), pic("B", 2, 0, 1), pic("B", 3, 0, 1)]
    chain = [pic("I", 4)] + [pic("P", 4 + (i % 4), 4 + ((i - 1) % 4)) for i in range(1, 8)]
    b1 = chain[:1] + short[:1] + chain[1:] + short[1:] if mirrored else short[:1] + chain[:1] + short[1:] + chain[1:]
    b2 = ([pic("I", 8)] if mirrored else []) + [pic("P", 9, 7), pic("P", 6, 9), pic("B", 10, 6, 9)]
    return b1, b2


def _sets_of(w, h, cf, nslots, pics, mbs, coefs):
    dump = R.plan_dump(w, h, cf, nslots, pics, mbs, coefs)
    lof = D.launch_of_pics(dump, len(pics))
    return [int(dump["launches"][lof[q]][4]) for q in range(len(pics))], dump


@pytest.mark.parametrize("mirrored", [False, True], ids=["reader_on_set0", "reader_on_set1"])
@CFS
def test_cross_set_ordering(cf, mirrored):
    """A set of batch 2 waits for the set of batch 1 whose slots it touches (batch_decode: by slot
    footprint), not only for its own stream's earlier work.  upload, decode, upload, decode with no
    host synchronisation; a missing wait lets batch 2 read slot 7 before the 8-launch chain has
    written it, or overwrite slot 6 under the chain's last picture, which shows here only with
    high probability: the deterministic half is the `foot` requirement of the CPU test."""
    w, h, nslots = 128, 48, 11
    s1, s2 = _cross_set_batches(mirrored)
    pics, mbs, coefs, _ = D.build(w, h, cf, s1 + s2, seed=4100 + cf)
    a, b = D.split(pics, mbs, coefs, len(s1))
    chain_set = 0 if mirrored else 1
    sets1, dump1 = _sets_of(w, h, cf, nslots, *a)
    assert all(sets1[q] == (chain_set if s1[q][1] >= 4 else 1 - chain_set) for q in range(len(s1)))
    assert sum(int(L[4]) == chain_set for L in dump1["launches"]) >= 8
    sets2, dump2 = _sets_of(w, h, cf, nslots, *b)
    assert sets2 == ([0, 1, 1, 1] if mirrored else [0, 0, 0])
    assert {6, 7} <= set(dump2["foot"][1 - chain_set].tolist()) and {6, 7} <= set(dump1["foot"][chain_set].tolist())
    exp = Oracle(w, h, cf, pics, mbs, coefs, nslots)
    with R.DeviceContext(w, h, cf, slots=nslots) as ctx:
        ctx.upload(*a)
        ctx.decode()
        ctx.upload(*b)
        ctx.decode()
        ctx.synchronize()
        assert_slots(ctx, exp, live_slots(pics), "two batches")


@CFS
def test_cross_set_ordering_over_three_batches(cf):
    """Batch N - 1 as above (the chain on set 1), batch N a single picture on untouched slots (set
    0 alone: the context then remembers no footprint of set 1), batch N + 1 reads slot 7, which set
    1 wrote in batch N - 1, on set 0.  What orders them is the upload of batch N + 1: it reuses
    batch N - 1's record bank and so waits for that batch's whole decode (two banks)."""
    w, h, nslots = 128, 48, 12
    s1, s3 = _cross_set_batches(False)
    s2 = [pic("I", 11)]
    pics, mbs, coefs, _ = D.build(w, h, cf, s1 + s2 + s3, seed=4200 + cf)
    a, rest = D.split(pics, mbs, coefs, len(s1))
    b, c = D.split(*rest, 1)
    exp = Oracle(w, h, cf, pics, mbs, coefs, nslots)
    with R.DeviceContext(w, h, cf, slots=nslots) as ctx:
        for batch in (a, b, c):
            ctx.upload(*batch)
            ctx.decode()
        ctx.synchronize()
        assert_slots(ctx, exp, live_slots(pics), "three batches")


@CFS
def test_decode_three_times_then_next_upload(cf):
    """decode() three times on one upload (the batch reads nothing from before it, so decoding it
    again is exact), then the next batch, which reads across sets; no host synchronisation."""
    w, h, nslots = 128, 48, 11
    s1, s2 = _cross_set_batches(False)
    pics, mbs, coefs, _ = D.build(w, h, cf, s1 + s2, seed=4300 + cf)
    a, b = D.split(pics, mbs, coefs, len(s1))
    exp = Oracle(w, h, cf, pics, mbs, coefs, nslots)
    with R.DeviceContext(w, h, cf, slots=nslots) as ctx:
        ctx.upload(*a)
        for _ in range(3):
            ctx.decode()
        ctx.upload(*b)
        ctx.decode()
        ctx.synchronize()
        assert_slots(ctx, exp, live_slots(pics), "three decodes")


@CFS
def test_units_every_launch_size(cf):
    """One slice per picture (64 x 16), n I pictures then n P pictures, one stream: I launches of
    n = 1..18 workgroups and P launches of 1..9 (two slices each, the last one slice when n is
    odd): every residue of recon_kernel's XCD unit bijection, with q8 == 0 and q8 > 0."""
    w, h = 64, 16
    for n in range(1, 19):
        spec, pics, mbs, coefs, _ = D.batch(f"units{n}", w, h, cf)
        exp = Oracle(w, h, cf, pics, mbs, coefs, 2 * n)
        with R.DeviceContext(w, h, cf, slots=2 * n, one_stream=True) as ctx:
            ctx.upload(pics, mbs, coefs)
            ctx.decode()
            ctx.synchronize()
            assert_slots(ctx, exp, range(2 * n), ("units", n))


def test_placement_calibration_on_a_ring(monkeypatch):
    """The placement calibration (calibrate_placement decodes the first batch several times on
    candidate pools) forced on a small pool whose first batch is the 5-slot ring: it rewrites its
    slots but reads none from before the batch, so the calibration runs, and every live slot
    equals the oracle's."""
    monkeypatch.setenv("MP2VG_PLACE_CANDIDATES", "3")
    monkeypatch.setenv("MP2VG_PLACE_MIN_MB", "0")
    w, h, cf = 128, 48, 1
    spec, pics, mbs, coefs, _ = D.batch("ring5", w, h, cf)
    exp = Oracle(w, h, cf, pics, mbs, coefs, 5)
    with R.DeviceContext(w, h, cf, slots=5) as ctx:
        ctx.upload(pics, mbs, coefs)
        ctx.decode()
        ctx.synchronize()
        ms, kept = ctx.placement()
        assert len(ms) == 6 and 0 <= kept < 3 and all(t > 0 for t in ms)
        assert_slots(ctx, exp, live_slots(pics), "calibrated ring")


def test_placement_calibration_skips_a_batch_that_overwrites_what_it_read(monkeypatch):
    """The first batch reads slot 0 from outside (written through mp2vg_slot_device_ptr and
    mp2vg_invalidate_slot) and later overwrites it: decoding it again would predict from its own
    output, so the calibration must not run (placement() reports none), and the frames equal the
    oracle's."""
    from tiny_mp2v_dec_amd.decoder import _hip_lib
    monkeypatch.setenv("MP2VG_PLACE_CANDIDATES", "3")
    monkeypatch.setenv("MP2VG_PLACE_MIN_MB", "0")
    w, h, cf = 128, 48, 1
    spec = [pic("I", 0), pic("P", 1, 0), pic("B", 2, 0, 1), pic("I", 0), pic("P", 3, 0)]
    pics, mbs, coefs, _ = D.build(w, h, cf, spec, seed=4400)
    a, b = D.split(pics, mbs, coefs, 1)
    assert R.plan_dump(w, h, cf, 4, *b)["ext_reads"].tolist() == [[0, 0]]
    exp = Oracle(w, h, cf, pics, mbs, coefs, 4)
    with R.DeviceContext(w, h, cf, slots=4) as src, R.DeviceContext(w, h, cf, slots=4) as dst:
        src.upload(*a)
        src.decode()
        src.synchronize()
        ps, pd = ctypes.c_void_p(), ctypes.c_void_p()
        _lib.check(_lib.lib().mp2vg_slot_device_ptr(src.h, 0, ctypes.byref(ps)), "slot_device_ptr")
        _lib.check(_lib.lib().mp2vg_slot_device_ptr(dst.h, 0, ctypes.byref(pd)), "slot_device_ptr")
        assert _hip_lib().hipMemcpy(pd.value, ps.value, int(src.slot_bytes), 3) == 0  # device to device
        _lib.check(_lib.lib().mp2vg_invalidate_slot(dst.h, 0), "invalidate_slot")
        dst.upload(*b)
        dst.decode()
        dst.synchronize()
        assert dst.placement() == ([], -1)
        assert_slots(dst, exp, [0, 1, 2, 3], "uncalibrated batch")
