"""CPU: what the directed GPU device-parse tests (test_gpu_device_parse_directed.py) take for
granted, checked against the live host emitter and the CPU twin: the committed mutant fixture is
current, start-code stuffing is accepted with unchanged records, the tail streams cover every
span length mod 4, a chosen slice can be made to fail, and mutants at the end of a sub-range are
accepted or rejected alike by the host emitter on the whole stream and the twin on the range."""
import importlib.util
import os

import pytest

import parse_mutants as PM
from conftest import GOLDEN, load_manifest, read_stream
from tiny_mp2v_dec_amd.records import generate_es

BY_NAME = {e["name"]: e for e in load_manifest()}
FIX = PM.load_fixture()


@pytest.fixture(scope="module")
def bases():
    return [(es, w, h, cf, PM.host(es, w, h, cf)[2]) for es, w, h, cf in PM.base_streams()]


def test_fixture_is_what_the_committed_script_writes():
    spec = importlib.util.spec_from_file_location("make_parse_mutants", os.path.join(GOLDEN, "make_parse_mutants.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(PM.FIXTURE) as f:
        assert f.read() == mod.dumps(mod.make())


def test_fixture_names_the_helpers_streams_and_walk():
    assert FIX["streams"] == PM.STREAMS and FIX["walk_seed"] == PM.WALK_SEED
    assert FIX["mutants_per_stream"] == PM.FIXTURE_MUTANTS_PER_STREAM >= PM.MUTANTS_PER_STREAM
    assert FIX["intra_vlc_format0"]["stream"] == PM.VLC0_STREAM
    assert sorted(FIX["rejected"]) == sorted(PM.SLICE_REASONS)
    walks = [set(PM.walk(si, b[0], PM.FIXTURE_MUTANTS_PER_STREAM)) for si, b in enumerate(PM.base_streams())]
    for si, pos, val, *_ in [m for v in FIX["rejected"].values() for m in v] + FIX["accepted"]:
        assert (pos, val) in walks[si]


@pytest.mark.parametrize("reason", PM.SLICE_REASONS)
def test_rejected_entries_replay_with_the_recorded_status_and_message(bases, reason):
    entries = FIX["rejected"][reason]
    assert len(entries) >= 3
    for si, pos, val, status, det, by_scan in entries:
        es, w, h, cf, _ = bases[si]
        b = PM.mutate(es, pos, val)
        hs, hm, _ = PM.host(b, w, h, cf)
        ts, tm, _, scanned = PM.twin(b, w, h, cf)
        assert status != 0 and reason in det and not by_scan and not scanned
        assert (hs, PM.detail(hm)) == (status, det)
        assert (ts, PM.detail(tm)) == (status, det)


def test_intra_vlc_format_zero_entry_replays():
    es, w, h, cf = PM.vlc0_stream()
    want = (FIX["intra_vlc_format0"]["status"], FIX["intra_vlc_format0"]["detail"])
    assert want[0] == -2 and PM.VLC0_REASON in want[1]
    hs, hm, _ = PM.host(es, w, h, cf)
    ts, tm, _, scanned = PM.twin(es, w, h, cf)
    assert not scanned and (hs, PM.detail(hm)) == want and (ts, PM.detail(tm)) == want


def test_accepted_entries_replay_with_records_that_differ_from_the_base_streams(bases):
    differ = 0
    for si, pos, val, status, det, by_scan in FIX["accepted"]:
        es, w, h, cf, base = bases[si]
        b = PM.mutate(es, pos, val)
        hs, hm, p = PM.host(b, w, h, cf)
        ts, tm, rec, _ = PM.twin(b, w, h, cf)
        assert (status, det, by_scan) == (0, "", False) and hs == 0 and ts == 0, (hm, tm)
        assert PM.same_records(p, rec)
        differ += not PM.same_records(base, rec)
    assert differ >= 24


# ---- the reader's start residues and tail -----------------------------------------------------------
def test_stuffing_before_a_start_code_is_accepted_with_the_same_records():
    """k zero bytes in front of the second slice's start code (next_start_code() stuffing) move
    every later slice by k: each stuffed stream starts slices at all four address residues, and
    the host emitter and the twin give the records of the unstuffed stream"""
    w, h, cf = PM.geom(PM.STUFF_STREAM)
    es = generate_es(**PM.STUFF_STREAM)
    base = PM.host(es, w, h, cf)[2]
    firsts = []
    for k in range(4):
        b = PM.stuffed(es, k)
        assert len(b) == len(es) + k
        hs, hm, p = PM.host(b, w, h, cf)
        ts, tm, rec, _ = PM.twin(b, w, h, cf)
        assert hs == 0 and ts == 0, (k, hm, tm)
        assert PM.same_records(base, (p.mbs, p.coefs)) and PM.same_records(base, rec)
        assert all(PM.slice_residues(b)), k
        s = PM.slice_starts(b)
        firsts.append((s[1] - s[0]) & 3)
    assert sorted(firsts) == [0, 1, 2, 3]  # the slice behind the stuffing, at each residue once


def test_tail_seeds_cover_every_span_length_mod_4():
    assert sorted(PM.tail_span(PM.tail_stream(s)) % 4 for s in PM.TAIL_SEEDS) == [0, 1, 2, 3]
    for s in PM.TAIL_SEEDS:
        es = PM.tail_stream(s)
        hs, _, p = PM.host(es, 64, 32, 1)
        ts, _, rec, _ = PM.twin(es, 64, 32, 1)
        assert hs == 0 and ts == 0 and PM.same_records(p, rec)


# ---- a chosen slice made to fail ------------------------------------------------------------------------
@pytest.mark.parametrize("ks", [(0,), (129,), (70, 5), (64, 63)], ids=str)
def test_failing_slices_are_blamed_first_in_stream_order(ks):
    es = PM.one_slice_pictures(130, 130)
    bad, why = PM.stream_with_failing_slices(es, 16, 16, 1, ks)
    k = min(ks)
    if len(ks) == 2:
        assert why[min(ks)] != why[max(ks)]
    hs, hm, _ = PM.host(bad, 16, 16, 1)
    ts, tm, _, scanned = PM.twin(bad, 16, 16, 1)
    assert hs != 0 and not scanned and (ts, PM.detail(tm)) == (hs, PM.detail(hm))
    assert PM.blamed_picture(hm) == (k, PM.slice_starts(es)[k]) and why[k] in hm
    for j in ks:  # each of them fails on its own, for the reason found
        tj = PM.twin(bad, 16, 16, 1, j, 1)
        assert tj[0] != 0 and why[j] in tj[1]


# ---- mutants at the end of a sub-range ----------------------------------------------------------------------
@pytest.mark.parametrize("case", PM.SUBRANGE_CASES, ids=[c[0] for c in PM.SUBRANGE_CASES])
def test_mutants_in_the_last_slice_of_a_sub_range(case):
    """Past the range's end the twin (and the device) read zeros where the host emitter reads the
    rest of the stream.  Measured here: of 194 + 161 rejected mutants none differs in status or
    message, and no mutant is accepted by one side only."""
    name, first, n, _ = case
    e = BY_NAME[name]
    assert first + n < len(e["md5"])  # the range ends before the last picture
    ms = PM.subrange_mutants(read_stream(e), e["width"], e["height"], e["chroma_format"], *case[1:])
    assert len(ms) == PM.SUBRANGE_MUTANTS
    accepted = [m for m in ms if m[2] == 0]
    rejected = [m for m in ms if m[2] != 0]
    assert len(accepted) >= 50 and len(rejected) >= 50
    for pos, val, hs, hm, ts, tm, by_scan, same in ms:
        assert (hs == 0) == (ts == 0), (pos, val, hm, tm)
        assert same in (None, True), (pos, val)
    differing = [m for m in rejected if not m[6] and (m[4] != m[2] or PM.detail(m[5]) != PM.detail(m[3]))]
    print(f"{name}: {len(accepted)} accepted, {len(rejected)} rejected, {len(differing)} differ in status or message")
    assert len(differing) == 0, differing[:3]
