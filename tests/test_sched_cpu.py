"""CPU: the level scheduler's plan (mp2vg_batch_plan, no device) against the requirements any
correct plan must satisfy (tests/directed_sched.py check_plan): the directed batches, 300 seeded
random batches and the c1 I-only batch; the plan mutants (the checker rejects every corruption
under the requirement it breaks); what the batches exercise; and the soundness of the GPU tests'
prefix method (the oracle is indexed by slot)."""
import numpy as np
import pytest

import _oracle
import directed_sched as D
from tiny_mp2v_dec_amd import records as R

GEOMETRIES = [(w, h, cf) for (w, h) in D.SIZES for cf in (1, 2, 3)]
UNITS = [f"units{n}" for n in range(1, 19)]
_COVER = set()


def _plan_and_check(spec, pics, mbs, coefs, uses, geometry, one_stream):
    dump = R.plan_dump(*geometry, D.nslots_of(spec), pics, mbs, coefs, one_stream=one_stream)
    D.check_plan(pics, uses, geometry, 1 if one_stream else 2, dump)
    _COVER.update(D.coverage(pics, uses, dump))
    return dump


@pytest.mark.parametrize("one_stream", [False, True], ids=["two_streams", "one_stream"])
@pytest.mark.parametrize("name", sorted(D.DIRECTED))
def test_directed_batches_plan_correctly(name, one_stream):
    """Every directed batch at 64x48, 128x48 and 80x32 in the three chroma formats."""
    for geometry in GEOMETRIES:
        spec, pics, mbs, coefs, uses = D.batch(name, *geometry, dense=False)
        _plan_and_check(spec, pics, mbs, coefs, uses, geometry, one_stream)


@pytest.mark.parametrize("one_stream", [False, True], ids=["two_streams", "one_stream"])
def test_units_batches_plan_correctly(one_stream):
    """n I pictures then n P pictures at 64x16, n = 1..18; on one stream the I launch has n slices
    and the P launch n slices, two per workgroup: I launches of 1..18 units, P launches of 1..9."""
    for cf in (1, 2, 3):
        for n in range(1, 19):
            spec, pics, mbs, coefs, uses = D.batch(f"units{n}", 64, 16, cf, dense=False)
            dump = _plan_and_check(spec, pics, mbs, coefs, uses, (64, 16, cf), one_stream)
            if one_stream:
                assert [tuple(int(x) for x in L[[0, 1, 2, 5]]) for L in dump["launches"]] == [(0, n, 0, 0), (n, 2 * n, 1, 2)]


def test_random_batches_plan_correctly():
    """300 seeded random batches, valid by construction (D.random_spec): a batch the library
    refuses fails, none is skipped."""
    for seed in range(300):
        rng = np.random.default_rng(5000 + seed)
        spec, nslots = D.random_spec(rng)
        pics, mbs, coefs, uses = D.build(64, 32, 1, spec, dense=False)
        for one_stream in (False, True):
            dump = R.plan_dump(64, 32, 1, nslots, pics, mbs, coefs, one_stream=one_stream)
            try:
                D.check_plan(pics, uses, (64, 32, 1), 1 if one_stream else 2, dump)
            except D.PlanError as e:
                raise AssertionError(f"seed {seed}, one_stream {one_stream}, spec {spec}: {e}") from e
            _COVER.update(D.coverage(pics, uses, dump))


@pytest.mark.parametrize("name", sorted(D.MUTANTS))
def test_plan_mutant_rejected(name):
    """The valid plan passes; the corrupted one is rejected under the requirement it breaks."""
    good, bad, pics, uses, geometry = D.run_mutant(name)
    D.check_plan(pics, uses, geometry, 2, good)
    with pytest.raises(D.PlanError) as e:
        D.check_plan(pics, uses, geometry, 2, bad)
    assert e.value.requirement == D.MUTANTS[name][2], str(e.value)


def test_every_requirement_has_a_mutant():
    assert len(D.MUTANTS) == 15 and {m[2] for m in D.MUTANTS.values()} == set(D.REQUIREMENTS)


def test_coverage_of_directed_and_random_batches():
    """Over the directed and random batches together: each hazard kind is some picture's binding
    constraint, every mode 0-3 and mixed combination occurs, clusters of 1-4 pictures, more
    components than sets, tile conversions after launches of modes 1, 2 and 3, external reads."""
    if not _COVER:  # run alone: collect from the batches itself
        for name in sorted(D.DIRECTED) + UNITS:
            g = (64, 16, 1) if name.startswith("units") else (64, 48, 1)
            for one in (False, True):
                _plan_and_check(*D.batch(name, *g, dense=False), g, one)
        test_random_batches_plan_correctly()
    want = {"bind:RAW", "bind:WAW", "bind:WAR", "mode:0", "mode:1", "mode:2", "mode:3",
            "mix:I+P", "mix:B2+I", "mix:B2+I+P", "mix:B1+B2", "mix:B2+P",
            "cluster:1", "cluster:2", "cluster:3", "cluster:4", "components>sets",
            "post_after_mode:1", "post_after_mode:2", "post_after_mode:3", "ext_reads"}
    assert want <= _COVER, sorted(want - _COVER)


def test_pair_shift_units_from_the_dump():
    """MB height 3, one stream: odd clusters followed by further clusters shift the pairing, so
    workgroup units (slices 2k, 2k + 1) hold a P with a B slice, an I with a B slice, an I with a
    P slice, a one-direction with a two-direction B slice and two rows of one picture; and a
    launch's last unit holds one slice."""
    for w, h in [(64, 48), (128, 48)]:
        seen, single = set(), False
        for name in ("pair_shift2", "pair_shift3"):
            spec, pics, mbs, coefs, uses = D.batch(name, w, h, 1, dense=False)
            dump = R.plan_dump(w, h, 1, D.nslots_of(spec), pics, mbs, coefs, one_stream=True)
            per = set()
            for li, L in enumerate(dump["launches"]):
                if int(L[5]) != 2:
                    continue
                units = D.unit_pairs(pics, uses, dump, li)
                single |= units[-1][1] is None
                for a, b in units:
                    if b is not None:
                        per.add("same" if a[1] == b[1] else "+".join(sorted((a[0], b[0]))))
            assert {"B2+P", "B2+I", "B1+B2", "same"} <= per, (name, per)
            seen |= per
        assert {"B2+P", "B2+I", "I+P", "B1+B2", "same"} <= seen and single, (seen, single)


def test_c1_i_only_plan_covers_cross_row_slices():
    """The c1 geometry (1920x1088 4:2:0, 120 I pictures): the planner cuts I slices across MB rows
    (i_slice_groups); every MB record once, slices on 4-MB group boundaries (cover)."""
    w, h, cf, n = 1920, 1088, 1, 120
    pics, mbs, coefs, uses = D.build(w, h, cf, [D.pic("I", p) for p in range(n)], dense=False)
    dump = R.plan_dump(w, h, cf, n, pics, mbs, coefs)
    D.check_plan(pics, uses, (w, h, cf), 2, dump)
    assert np.any(dump["slices"][:, 2] > w // 16), "no slice crosses a row"
    assert set(dump["launches"][:, 2].tolist()) == {0}


LIMIT_SIZES = [(16384, 32), (16368, 32), (32, 16384), (16, 16384)]


@pytest.mark.parametrize("one_stream", [False, True], ids=["two_streams", "one_stream"])
@pytest.mark.parametrize("size", LIMIT_SIZES, ids=lambda s: "%dx%d" % s)
def test_limit_geometries_plan_correctly(size, one_stream):
    """An I, P, B batch and an I-only batch at the sizes of tests/test_gpu_limits.py, in the three
    chroma formats: the plan meets every requirement (check_plan), and from the dump: every P and
    B slice is one whole row, of 1024 (1023) MBs or, at 32 and 16 wide, of 2 and 1 (1024 slices per
    picture); the P and B launches pair their slices (mates) at 16384 alone, where a row is a
    multiple of the 4-MB group.  I slices, on one stream and on two, in both batches: the planner's
    slice of an I launch is one row, two rows in 4:4:4 where a row is a multiple of the group
    (runtime.cpp rows_i), so at 16384 x 32 in 4:4:4 every I slice runs across both rows of its
    picture (2048 MBs), and everywhere else (4:2:0 and 4:2:2 there; every format at 16368 x 32,
    32 x 16384 and 16 x 16384) every I slice is exactly one row.  The cut on group boundaries
    inside a row (i_slice_groups, test_c1_i_only_plan_covers_cross_row_slices) is chosen at none of
    these sizes: every I slice starts on a row and holds whole rows."""
    w, h = size
    mbw, mbh = w // 16, h // 16
    ipb = [D.pic("I", 0), D.pic("P", 1, 0), D.pic("B", 2, 0, 1)]
    for cf in (1, 2, 3):
        rows_i = 2 if cf == 3 and mbw % 4 == 0 else 1
        for spec in (ipb, [D.pic("I", p) for p in range(4)]):
            pics, mbs, coefs, uses = D.build(w, h, cf, spec, seed=16384 + cf, dense=False)
            dump = _plan_and_check(spec, pics, mbs, coefs, uses, (w, h, cf), one_stream)
            sl = dump["slices"]
            assert int(sl[:, 2].sum()) == len(spec) * mbw * mbh
            for L in dump["launches"]:
                s = sl[int(L[0]):int(L[1])]
                if int(L[2]) == 0:
                    assert (s[:, 2] == rows_i * mbw).all() and (s[:, 1] % (rows_i * mbw) == 0).all(), (size, cf)
                    assert int(L[5]) == 0
                    continue
                assert (s[:, 2] == mbw).all() and (s[:, 1] % mbw == 0).all() and len(s) % mbh == 0
                assert int(L[5]) == (2 if mbw % 4 == 0 else 0), (size, cf, L.tolist())


@pytest.mark.parametrize("name", sorted(D.DIRECTED) + ["units5"])
def test_oracle_is_indexed_by_slot(name):
    """Decoding the prefix pics[:k] gives, for every slot picture k - 1 does not write, the bytes
    of the prefix pics[:k - 1], and decoding is deterministic: so a picture overwritten later in a
    batch can be checked by decoding the prefix that ends at it."""
    for w, h, cf in ([(64, 16, 1)] if name.startswith("units") else [(64, 48, 1), (128, 48, 2), (80, 32, 3)]):
        spec, pics, mbs, coefs, _ = D.batch(name, w, h, cf)
        nslots = D.nslots_of(spec)
        g, prev = _oracle.reconstruct(w, h, cf, pics[:1], mbs, coefs, nslots)
        sb = int(g.slot_bytes)
        changed = False
        for k in range(2, len(pics) + 1):
            _, pool = _oracle.reconstruct(w, h, cf, pics[:k], mbs, coefs, nslots)
            d = int(pics[k - 1]["dst_slot"])
            for s in range(nslots):
                if s != d:
                    assert np.array_equal(pool[s * sb:(s + 1) * sb], prev[s * sb:(s + 1) * sb]), (k, s)
            changed |= not np.array_equal(pool[d * sb:(d + 1) * sb], prev[d * sb:(d + 1) * sb])
            prev = pool
        assert changed
