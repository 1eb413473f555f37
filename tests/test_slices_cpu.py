"""CPU: MP2VG_PARSE_SLICES in the host emitter (csrc/parse.cpp) and the CPU twin of the device parse
(csrc/slice_parse.h).

The pin is the twin streams of tests/slices_streams.py (tests/golden/slices/): the "ms" form, rows
cut into several slices, under the flag must give the macroblock records, coefficient words and
picture records of the writer's model, which are those the "ref" form (one slice per row) gives
with the flag clear; so its frames carry the MD5s the compiled reference computed for the ref form.
With the flag clear every ms stream is refused with today's texts.  The negative streams are
refused alike by both parsers, and under MP2VG_PARSE_CONCEAL broken rows are replaced as whole rows
(tests/conceal_model.py states the rule).

Planted defects (each applied in a scratch copy of parse.cpp and, separately, of slice_parse.h;
profiles/device_parse/slices.md records the tests that then fail): no PMV reset at a mid-row slice start, no DC reset there, the quantiser
not taken from the slice header, x0 off by one, records emitted for the initial increment, the
cover check accepting a gap, accepting an overlap, the words of a dropped entry kept."""
import json
import os
import subprocess

import numpy as np
import pytest

import conceal_model as CM
import directed_syntax as DS
import parse_mutants as PM
import slices_streams as SL
from conftest import GOLDEN
from helpers import oracle_frames, yuv_md5
from tiny_mp2v_dec_amd import _lib
from tiny_mp2v_dec_amd.records import Parsed, Scan, damage_reason

MANIFEST = SL.load_manifest()
TWINS = [e for e in MANIFEST if e["md5"] is not None]
NEGATIVE = [e for e in MANIFEST if e["md5"] is None]
BY_NAME = {e["name"]: e for e in MANIFEST}
IDS = [e["name"] for e in TWINS]
FIELDS = ("x", "y", "flags", "cbp", "qscale", "ncoef", "coef_off", "mv")


def geom(e):
    return e["width"], e["height"], e["chroma_format"]


def host(es, w, h, cf, threads=1, **kw):
    try:
        return 0, "", Parsed(es, w, h, cf, threads=threads, **kw)
    except _lib.Mp2vgError as e:
        return e.status, str(e), None


def twin(es, w, h, cf, **kw):
    try:
        with Scan(es, w, h, cf, **kw) as sc:
            return 0, "", sc.pics.copy(), sc.parse_host()
    except _lib.Mp2vgError as e:
        return e.status, str(e), None, None


@pytest.fixture(scope="module")
def written():
    return {ms.name: (ms, ref) for ms, ref in SL.build_all()}


@pytest.fixture(scope="module")
def refs():
    """{name: Parsed of the ref form, flag clear}"""
    return {e["name"]: Parsed(SL.read(e["ref"]), *geom(e), threads=1) for e in TWINS}


def test_the_flag_is_value_32_and_additive():
    assert _lib.MP2VG_PARSE_SLICES == 32 and _lib.parse_flags(slices=True) == 32
    assert _lib.parse_flags(True, True, True) == 8 | 16 | 32
    assert _lib.lib().mp2vg_abi_version() == 2


# ---- the fixtures ------------------------------------------------------------------------------------
def test_fixture_is_what_the_writer_writes(written):
    assert sorted(written) == sorted(IDS)
    for e in TWINS:
        ms, ref = written[e["name"]]
        assert SL.read(e["ms"]) == ms.es and SL.read(e["ref"]) == ref.es, e["name"]
        assert geom(e) + (e["frames"], e["slices"]) == (ms.width, ms.height, ms.cf, ms.npics, ms.nslices)
        assert (ms.mbs, ms.coefs) == (ref.mbs, ref.coefs)  # one picture model
        assert e["events"] == sorted(ms.events)
    for (build, status, reason, blamed), e in zip(SL.NEGATIVE, NEGATIVE):
        S = build()
        assert SL.read(e["ms"]) == S.es and (e["status"], e["reason"], e["blamed_slice"]) == (status, reason, blamed)
    assert len(NEGATIVE) == len(SL.NEGATIVE)
    assert {(e["width"], e["height"]) for e in TWINS} >= {(64, 48), (176, 144), (560, 16), (16384, 16)}
    total = sum(os.path.getsize(os.path.join(SL.GOLDEN, n)) for n in os.listdir(SL.GOLDEN))
    assert total < 512 * 1024


def test_every_event_is_exercised(written):
    got = {e for ms, _ in written.values() for e in ms.events if e.startswith("sl:")}
    want = set(SL.REQUIRED_EVENTS)
    assert len(want) == len(SL.REQUIRED_EVENTS)
    assert not want - got, sorted(want - got)
    assert got == want
    assert {e for m in TWINS for e in m["events"] if e.startswith("sl:")} == want


# ---- emitter, twin, oracle -----------------------------------------------------------------------------
@pytest.mark.parametrize("e", TWINS, ids=IDS)
def test_emitter_and_twin_under_the_flag_give_the_model_and_the_twin_streams_records(e, refs, written):
    ms, _ = written[e["name"]]
    q = refs[e["name"]]
    want_mbs, want_coefs = DS.records(ms)
    hs, hm, p = host(ms.es, *geom(e), slices=True)
    assert hs == 0, hm
    assert p.npics == q.npics == e["frames"] and len(p.mbs) == len(want_mbs)
    for f in FIELDS:  # field by field, so that a failure names the field and the macroblock
        bad = np.nonzero((p.mbs[f] != want_mbs[f]).reshape(len(want_mbs), -1).any(1))[0]
        assert not len(bad), (f, [(int(want_mbs["y"][i]), int(want_mbs["x"][i]), i // (ms.mbw * ms.mbh),
                                   p.mbs[f][i].tolist(), want_mbs[f][i].tolist()) for i in bad[:3]])
    assert np.array_equal(p.coefs, want_coefs)
    assert p.mbs.tobytes() == q.mbs.tobytes() and p.coefs.tobytes() == q.coefs.tobytes()
    assert p.pics.tobytes() == q.pics.tobytes() and p.display.tolist() == q.display.tolist()
    ts, tm, pics, rec = twin(ms.es, *geom(e), slices=True)
    assert ts == 0, tm
    assert pics.tobytes() == q.pics.tobytes() and PM.same_records(q, rec)
    # several workers: a row's slices are parsed side by side
    hs, hm, p4 = host(ms.es, *geom(e), threads=4, slices=True)
    assert hs == 0 and PM.same_records(q, (p4.mbs, p4.coefs))
    # picture ranges that start inside the stream
    if q.npics > 2:
        with Scan(ms.es, *geom(e), slices=True) as sc:
            assert sc.nslices == e["slices"]
            for first, n in ((1, 2), (q.npics - 1, 1)):
                want = PM.range_of_whole(q, first, n)
                got = sc.parse_host(first, n)
                assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


@pytest.mark.parametrize("e", TWINS, ids=IDS)
def test_oracle_frames_carry_the_reference_md5s(e):
    p = Parsed(SL.read(e["ms"]), *geom(e), threads=1, slices=True)
    frames = oracle_frames(p)
    assert [yuv_md5(frames[d]) for d in p.display] == e["md5"]


@pytest.mark.parametrize("e", TWINS, ids=IDS)
def test_the_other_flags_change_nothing_on_a_clean_stream(e, refs):
    q = refs[e["name"]]
    es = SL.read(e["ms"])
    c = Parsed(es, *geom(e), threads=1, slices=True, conceal=True, standard=True)
    assert len(c.damage) == 0 and PM.same_records(q, (c.mbs, c.coefs))
    assert c.pics.tobytes() == CM.flagged_pictures(q.pics).tobytes()
    st, msg, pics, rec = twin(es, *geom(e), slices=True, conceal=True, standard=True)
    assert st == 0 and PM.same_records(q, rec), msg
    # ... and the flag changes nothing on the one-slice-per-row form
    r = Parsed(SL.read(e["ref"]), *geom(e), threads=1, slices=True)
    assert PM.same_records(q, (r.mbs, r.coefs)) and r.pics.tobytes() == q.pics.tobytes()
    st, msg, pics, rec = twin(SL.read(e["ref"]), *geom(e), slices=True)
    assert st == 0 and PM.same_records(q, rec), msg


# ---- the flag clear --------------------------------------------------------------------------------------
@pytest.mark.parametrize("conceal", [False, True], ids=["plain", "conceal"])
@pytest.mark.parametrize("e", TWINS, ids=IDS)
def test_flag_clear_refuses_every_ms_stream_with_todays_texts(e, conceal):
    es = SL.read(e["ms"])
    first = PM.slice_starts(es)[0]
    hs, hm, _ = host(es, *geom(e), conceal=conceal)
    ts, tm, _, _ = twin(es, *geom(e), conceal=conceal)
    assert hs == ts == SL.CLEAR_STATUS
    # the scan meets the row's second slice before any slice is parsed; the emitter parses first
    assert PM.detail(tm).startswith("picture 0 slice @") and PM.detail(tm).endswith(SL.CLEAR_REASONS[1])
    if conceal:  # the short slice is concealed, the second slice of the row names no row of its own
        assert PM.detail(hm) == PM.detail(tm)
    else:
        assert PM.detail(hm) == f"picture 0 slice @{first}: {SL.CLEAR_REASONS[0]}"


# ---- negative streams ------------------------------------------------------------------------------------
@pytest.mark.parametrize("e", NEGATIVE, ids=[e["name"] for e in NEGATIVE])
def test_negative_streams_are_refused_alike(e):
    es = SL.read(e["ms"])
    off = PM.slice_starts(es)[e["blamed_slice"]]
    want = f"picture 0 slice @{off}: {e['reason']}"
    for threads in (1, 3):
        hs, hm, _ = host(es, *geom(e), threads=threads, slices=True)
        assert (hs, PM.detail(hm)) == (e["status"], want)
    ts, tm, _, _ = twin(es, *geom(e), slices=True)
    assert (ts, PM.detail(tm)) == (e["status"], want)
    # under CONCEAL the row is replaced and reported once, with the blamed slice; coming back to a row stays refused
    hs, hm, p = host(es, *geom(e), slices=True, conceal=True)
    ts, tm, pics, rec = twin(es, *geom(e), slices=True, conceal=True)
    if e["reason"] == SL.TWO:
        assert (hs, PM.detail(hm)) == (ts, PM.detail(tm)) == (e["status"], want)
        return
    assert hs == ts == 0, (hm, tm)
    assert PM.same_records(p, rec)
    row = next(t[1] for t in SL.slice_table(es) if t[2] == off)
    assert [(int(d["pic"]), int(d["mb_row"]), int(d["status"]), damage_reason(d["reason"]), int(d["byte_off"]))
            for d in p.damage] == [(0, row, e["status"], e["reason"], off)]
    grey, words = CM.replacement_row(p.pics[0], -1, row, 4, 1)
    got = p.mbs[row * 4:(row + 1) * 4].copy()
    c0 = int(got["coef_off"][0])
    got["coef_off"] -= c0
    assert got.tobytes() == grey.tobytes() and p.coefs[c0:c0 + len(words)].tobytes() == words.tobytes()
    assert int(p.mbs["ncoef"].sum()) == len(p.coefs)  # no word of a dropped slice is kept


# ---- concealment ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def conceal_cases():
    e = BY_NAME[SL.CONCEAL_STREAM]
    return e, {c[0]: c for c in SL.conceal_cases(SL.read(e["ms"]), *geom(e))}


@pytest.mark.parametrize("name", ["damaged_I", "damaged_P", "damaged_B", "middle_deleted", "row_deleted"])
def test_a_broken_row_is_replaced_as_a_whole(name, conceal_cases, refs):
    e, cases = conceal_cases
    _, es, damaged, missing, want_damage = cases[name]
    q = refs[e["name"]]
    pics, mbs, coefs, order = CM.conceal(q, damaged, missing)
    for parse in ("host", "host4", "twin"):
        if parse == "twin":
            st, msg, got_pics, rec = twin(es, *geom(e), slices=True, conceal=True)
            assert st == 0, msg
        else:
            st, msg, p = host(es, *geom(e), threads=4 if parse == "host4" else 1, slices=True, conceal=True)
            assert st == 0, msg
            got_pics, rec = p.pics, (p.mbs, p.coefs)
            got = [(int(d["pic"]), int(d["mb_row"]), int(d["status"]), damage_reason(d["reason"]), int(d["byte_off"]))
                   for d in p.damage]
            assert [g[:2] for g in got] == order
            for g, w in zip(got, want_damage):
                assert g[:2] == w[:2] and g[3:] == w[3:] and (w[2] is None or g[2] == w[2]), (g, w)
        assert got_pics.tobytes() == pics.tobytes(), parse
        assert rec[0].tobytes() == mbs.tobytes() and rec[1].tobytes() == coefs.tobytes(), parse
    # without CONCEAL the same stream is refused, by both alike, at the blamed slice
    hs, hm, _ = host(es, *geom(e), slices=True)
    ts, tm, _, _ = twin(es, *geom(e), slices=True)
    assert hs == ts != 0 and PM.detail(hm) == PM.detail(tm)
    if missing:
        assert PM.detail(hm) == want_damage[0][3]
    else:
        assert PM.detail(hm) == f"picture {want_damage[0][0]} slice @{want_damage[0][4]}: {want_damage[0][3]}"


# ---- the emitter, the scan and the twin under the sanitizers ------------------------------------------------
@pytest.fixture(scope="module")
def slices_check(tmp_path_factory):
    """tests/fuzz/slices_check.cpp, a program of its own, with parse.cpp and tables.cpp under
    AddressSanitizer and UndefinedBehaviorSanitizer (CPU only)"""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(repo, "tiny_mp2v_dec_amd", "csrc")
    exe = str(tmp_path_factory.mktemp("san_slices") / "slices_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I", csrc,
           "-I", os.path.join(repo, "include"), os.path.join(repo, "tests", "fuzz", "slices_check.cpp"),
           os.path.join(csrc, "parse.cpp"), os.path.join(csrc, "tables.cpp"), "-o", exe, "-pthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        pytest.fail(f"sanitizer build failed:\n{r.stderr[-2000:]}")
    return exe


def test_emitter_scan_and_twin_under_asan_ubsan(slices_check):
    args = []
    for e in MANIFEST:
        if e["width"] * e["height"] > 176 * 144:  # (the mutant sweep keeps to the small pictures)
            continue
        args += [os.path.join(SL.GOLDEN, e["ms"]), str(e["width"]), str(e["height"]), str(e["chroma_format"])]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([slices_check, "120", "16"] + args, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    res = json.loads(r.stdout.strip().splitlines()[-1])
    print(res)
    assert res["streams"] == len(args) // 4 and res["accepted"] > 100 and res["rejected"] > 100
    assert res["concealed"] > 100 and res["cover_failures"] > 0
