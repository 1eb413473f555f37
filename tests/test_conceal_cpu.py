"""CPU: concealment (MP2VG_PARSE_CONCEAL) of the host emitter and the CPU twin of the device parse
against the plain-numpy statement of the rule (conceal_model.py), the C oracle and streams repaired
by an independent writer and decoded by the compiled reference (tests/golden/conceal/).

Planted defects (each applied in a scratch copy of slice_parse.h / parse.cpp; DESIGN.md §3 records
the tests that then fail): concealing from the fault onwards, a wrong coef_off after a grey row,
not re-typing the I picture, forward in a B picture without a forward reference."""
import types

import numpy as np
import pytest

import conceal_model as CM
import conceal_streams as CS
import parse_mutants as PM
from conftest import load_manifest, read_stream
from helpers import oracle_frames, yuv_md5
from tiny_mp2v_dec_amd import _lib
from tiny_mp2v_dec_amd.records import Parsed, Scan, damage_reason, generate_es, validate_batch

FIX = PM.load_fixture()


@pytest.fixture(scope="module")
def bases():
    return [(es, w, h, cf, PM.host(es, w, h, cf)[2]) for es, w, h, cf in PM.base_streams()]


def flagged(es, w, h, cf):
    """(Parsed of the host emitter, (mbs, coefs) of the twin), both under the flag"""
    p = Parsed(es, w, h, cf, threads=1, conceal=True)
    with Scan(es, w, h, cf, conceal=True) as sc:
        rec = sc.parse_host()
        # the scan's picture records are the emitter's before any re-typing (the upload re-types its own copy)
        coded = p.pics.copy()
        coded["picture_coding_type"][(p.flags & _lib.PIC_RETYPED_I) != 0] = 1
        assert sc.pics.tobytes() == coded.tobytes() and sc.nshards == p.nshards
    return p, rec


def same_as_model(p, model):
    pics, mbs, coefs, _ = model
    assert p.mbs.tobytes() == mbs.tobytes()
    assert p.coefs.tobytes() == coefs.tobytes()
    assert p.pics.tobytes() == pics.tobytes()


def damage_rows(p):
    return [(int(d["pic"]), int(d["mb_row"])) for d in p.damage]


def validates(p, mbs=None, coefs=None):
    validate_batch(p.width, p.height, p.chroma_format, p.npics, p.pics, p.mbs if mbs is None else mbs,
                   p.coefs if coefs is None else coefs)


def as_parsed(like, pics, mbs, coefs):
    return types.SimpleNamespace(width=like.width, height=like.height, chroma_format=like.chroma_format, pics=pics,
                                 mbs=mbs, coefs=coefs, npics=len(pics))


# ---- the rejected mutants of the committed fixture --------------------------------------------------
@pytest.mark.parametrize("reason", PM.SLICE_REASONS)
def test_rejected_fixture_mutants_parse_to_the_model_of_the_blamed_row(bases, reason):
    entries = FIX["rejected"][reason]
    assert len(entries) >= 3
    for si, pos, val, status, det, _ in entries:
        es, w, h, cf, base = bases[si]
        b = PM.mutate(es, pos, val)
        hs, hm, _ = PM.host(b, w, h, cf)
        assert (hs, PM.detail(hm)) == (status, det)  # without the flag: the recorded rejection
        pic, off = PM.blamed_picture(det)
        row = b[off + 3] - 1
        p, rec = flagged(b, w, h, cf)
        same_as_model(p, CM.conceal(base, [(pic, row)]))
        assert PM.same_records(p, rec)
        assert len(p.damage) == 1
        d = p.damage[0]
        assert (int(d["pic"]), int(d["mb_row"]), int(d["status"]), int(d["byte_off"])) == (pic, row, status, off)
        assert det.endswith(": " + damage_reason(d["reason"])) and reason in damage_reason(d["reason"])
        assert p.flags[pic] & _lib.PIC_CONCEALED
        validates(p)


def test_intra_vlc_format_zero_stream_is_concealed_row_by_row():
    """every slice of this stream holds an intra macroblock, so every row is blamed"""
    es, w, h, cf = PM.vlc0_stream()
    assert PM.host(es, w, h, cf)[0] == FIX["intra_vlc_format0"]["status"]
    base = Parsed(generate_es(**PM.VLC0_STREAM), w, h, cf)
    p, rec = flagged(es, w, h, cf)
    rows = [(q, y) for q in range(base.npics) for y in range(h // 16)]
    same_as_model(p, CM.conceal(base, rows))
    assert PM.same_records(p, rec) and damage_rows(p) == rows
    assert all(PM.VLC0_REASON in damage_reason(r) for r in p.damage["reason"])
    validates(p)


# ---- streams that parse without the flag are untouched by it ---------------------------------------
def unchanged_by_the_flag(es, w, h, cf):
    plain = Parsed(es, w, h, cf, threads=1)
    p, rec = flagged(es, w, h, cf)
    assert len(p.damage) == 0
    assert p.mbs.tobytes() == plain.mbs.tobytes() and p.coefs.tobytes() == plain.coefs.tobytes()
    assert PM.same_records(plain, rec)
    assert p.pics.tobytes() == CM.flagged_pictures(plain.pics).tobytes()  # only I pictures' fwd_slot differs
    assert np.array_equal(p.flags, plain.flags) and np.array_equal(p.display, plain.display)
    return plain, p


def test_accepted_fixture_mutants_are_unchanged_by_the_flag(bases):
    assert len(FIX["accepted"]) >= 24
    for si, pos, val, *_ in FIX["accepted"]:
        es, w, h, cf, _ = bases[si]
        unchanged_by_the_flag(PM.mutate(es, pos, val), w, h, cf)


@pytest.mark.parametrize("entry", [e for e in load_manifest() if e.get("md5")], ids=lambda e: e["name"])
def test_golden_streams_are_unchanged_by_the_flag(entry):
    plain, p = unchanged_by_the_flag(read_stream(entry), entry["width"], entry["height"], entry["chroma_format"])
    # one shard whenever an I picture has a conceal reference
    has_ref = bool(((p.pics["picture_coding_type"] == 1) & (p.pics["fwd_slot"] >= 0)).any())
    assert p.nshards == (1 if has_ref else plain.nshards)
    validates(p)


# ---- the walk of the byte-mutant sweep -------------------------------------------------------------
UNOWNED = ("slice row outside the picture", "two slices in one macroblock row")


def unowned_rows(es, h):
    """a slice start code of the stream names a row outside the picture, or a row of its picture
    a second time (found without the library)"""
    seen = set()
    for pic, row, _, _ in CS.slice_table(es):
        if row >= h // 16 or (pic, row) in seen:
            return True
        seen.add((pic, row))
    return False


@pytest.mark.parametrize("si", range(len(PM.STREAMS)))
def test_walk_mutants_conceal_every_slice_level_rejection(bases, si):
    es, w, h, cf, _ = bases[si]
    n = {"accepted": 0, "concealed": 0, "rejected": 0}
    for pos, val in PM.walk(si, es):
        b = PM.mutate(es, pos, val)
        hs, hm, plain = PM.host(b, w, h, cf)
        try:
            p, rec = flagged(b, w, h, cf)
            fs, fm = 0, ""
        except _lib.Mp2vgError as e:
            fs, fm, p = e.status, str(e), None
        if hs == 0:
            assert fs == 0 and len(p.damage) == 0 and PM.same_records(plain, rec), (pos, val, fm)
            n["accepted"] += 1
        elif (CS.slice_level(hm) or CS.UNCOVERED in hm) and unowned_rows(b, h):
            # the blamed slice is concealable, but the mutation also made a start code whose slice
            # names a row outside the picture or a row that has a slice already: that stays a
            # rejection under the flag (include/mp2vg.h), from the emitter and from the scan alike
            assert fs == -2 and any(t in fm for t in UNOWNED), (pos, val, hm, fm)
            with pytest.raises(_lib.Mp2vgError) as ei:
                Scan(b, w, h, cf, conceal=True)
            assert ei.value.status == -2 and any(t in str(ei.value) for t in UNOWNED)
            n["rejected"] += 1
        elif CS.slice_level(hm) or CS.UNCOVERED in hm:
            assert fs == 0, (pos, val, hm, fm)
            assert len(p.damage) >= 1 and PM.same_records(p, rec), (pos, val)
            first = p.damage[0]  # the unflagged call blames the first damaged slice in stream order
            if CS.slice_level(hm):
                assert (int(first["pic"]), int(first["byte_off"])) == PM.blamed_picture(hm), (pos, val)
                assert PM.detail(hm).endswith(": " + damage_reason(first["reason"])) and int(first["status"]) == hs
            validates(p)
            n["concealed"] += 1
        else:  # picture level, stream level, or a slice that names no row of its own
            assert (fs, PM.detail(fm)) == (hs, PM.detail(hm)), (pos, val)
            with pytest.raises(_lib.Mp2vgError) as ei:
                with Scan(b, w, h, cf, conceal=True) as sc:
                    sc.parse_host()
            assert ei.value.status == hs
            n["rejected"] += 1
    print(f"stream {si}: {n}")
    assert sum(n.values()) == PM.MUTANTS_PER_STREAM and n["concealed"] >= 100 and n["accepted"] >= 50


# ---- several kinds of damage in one stream ----------------------------------------------------------
@pytest.fixture(scope="module")
def multi():
    bad, es, w, h, cf, why = CS.damaged_stream(CS.MULTI, CS.MULTI_DAMAGE)
    return bad, Parsed(es, w, h, cf), why


def test_multi_fault_stream_equals_the_model_and_decodes(multi):
    bad, base, why = multi
    w, h, cf = base.width, base.height, base.chroma_format
    assert list(base.pics["picture_coding_type"]) == [1, 3, 3, 2, 3, 3] * 2
    assert base.pics["fwd_slot"][1] < 0 <= base.pics["bwd_slot"][1] and base.pics["fwd_slot"][4] >= 0
    assert len(set(why.values())) >= 2 and PM.host(bad, w, h, cf)[0] != 0
    p, rec = flagged(bad, w, h, cf)
    model = CM.conceal(base, CS.MULTI_DAMAGE)
    same_as_model(p, model)
    assert PM.same_records(p, rec)
    assert damage_rows(p) == model[3] == sorted(CS.MULTI_DAMAGE)
    assert [damage_reason(r) for r in p.damage["reason"]] == [why[k] for k in sorted(why)]
    validates(p)
    # what each kind of damage becomes
    mbw = w // 16
    row = lambda q, y: p.mbs[(q * (h // 16) + y) * mbw:(q * (h // 16) + y + 1) * mbw]  # noqa: E731
    assert (row(0, 1)["flags"] == _lib.MB_INTRA).all() and (row(0, 1)["ncoef"] == 6).all()
    assert (row(1, 0)["flags"] == _lib.MB_BWD).all()
    for q, y in [(3, 2), (4, 1), (6, 0), (9, 0), (9, 2)]:
        assert (row(q, y)["flags"] == _lib.MB_FWD).all() and not row(q, y)["ncoef"].any() and not row(q, y)["mv"].any()
    assert p.pics["picture_coding_type"][6] == 2 and p.pics["fwd_slot"][6] == 3
    assert p.flags[6] & _lib.PIC_RETYPED_I and not p.flags[0] & _lib.PIC_RETYPED_I
    assert [bool(f & _lib.PIC_CONCEALED) for f in p.flags] == [q in {0, 1, 3, 4, 6, 9} for q in range(12)]
    assert p.nshards == 1 and base.nshards == 2
    # the oracle decodes the records; an I picture's rows outside the damage are the pristine decode's
    got, want = oracle_frames(p), oracle_frames(base)
    ch = 8  # chroma rows per macroblock row (4:2:0)
    for q, bad_rows in [(0, {1}), (6, {0})]:
        for y in set(range(3)) - bad_rows:
            assert np.array_equal(got[q][0][16 * y:16 * y + 16], want[q][0][16 * y:16 * y + 16])
            for k in (1, 2):
                assert np.array_equal(got[q][k][ch * y:ch * y + ch], want[q][k][ch * y:ch * y + ch])
    # the replaced rows are what the rule says: grey, and copies of the reference's rows
    assert abs(int(got[0][0][16:32].astype(int).mean()) - 128) <= 1  # (mid-grey up to the mismatch control's toggle)
    assert np.array_equal(got[6][0][0:16], got[3][0][0:16])
    assert np.array_equal(got[1][0][0:16], got[0][0][0:16])  # backward, from picture 0
    assert np.array_equal(got[4][0][16:32], got[0][0][16:32])  # forward, from picture 0


def test_damage_confined_to_late_pictures_leaves_the_rest_as_the_pristine_decode():
    bad, es, w, h, cf, _ = CS.damaged_stream(CS.MULTI, CS.LATE_DAMAGE)
    base = Parsed(es, w, h, cf)
    p, rec = flagged(bad, w, h, cf)
    same_as_model(p, CM.conceal(base, CS.LATE_DAMAGE))
    assert PM.same_records(p, rec)
    got, want = oracle_frames(p), oracle_frames(base)
    # pictures 9 (P) and 10 (B, which also predicts from 9) are touched, 11 predicts from 9
    for q in range(12):
        same = all(np.array_equal(a, b) for a, b in zip(got[q], want[q]))
        assert same == (q < 9), q
    for q, y in [(9, 0), (9, 2)]:  # rows outside the damage of a picture whose references are clean
        assert np.array_equal(got[q][0][16 * y:16 * y + 16], want[q][0][16 * y:16 * y + 16])
    assert not np.array_equal(got[9][0][16:32], want[9][0][16:32])


# ---- missing slices ---------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [[(4, 0)], [(4, 1)], [(4, 2)], [(0, 0), (0, 2)], [(6, 1), (11, 2)]], ids=str)
def test_missing_slices_are_concealed_as_uncovered_rows(rows):
    es = generate_es(**CS.MULTI)
    w, h, cf = PM.geom(CS.MULTI)
    base = Parsed(es, w, h, cf)
    table = CS.slice_table(es)
    cut = CS.delete_slices(es, [j for j, t in enumerate(table) if t[:2] in rows])
    assert len(cut) < len(es)
    hs, hm, _ = PM.host(cut, w, h, cf)
    assert hs == -2 and CS.UNCOVERED in hm
    p, rec = flagged(cut, w, h, cf)
    model = CM.conceal(base, missing=rows)
    same_as_model(p, model)
    assert PM.same_records(p, rec) and damage_rows(p) == model[3] == sorted(rows)
    assert all(damage_reason(r) == CS.UNCOVERED for r in p.damage["reason"]) and (p.damage["status"] == -2).all()
    pic_starts = PM.start_codes(cut, 0x00)
    assert [int(o) for o in p.damage["byte_off"]] == [pic_starts[q] for q, _ in sorted(rows)]
    validates(p)
    oracle_frames(p)


def test_a_damaged_and_a_missing_slice_of_one_picture():
    bad, es, w, h, cf, _ = CS.damaged_stream(CS.MULTI, [(3, 1)])
    table = CS.slice_table(bad)
    cut = CS.delete_slices(bad, [j for j, t in enumerate(table) if t[:2] == (3, 0)])
    p, rec = flagged(cut, w, h, cf)
    model = CM.conceal(Parsed(es, w, h, cf), damaged=[(3, 1)], missing=[(3, 0)])
    same_as_model(p, model)
    assert PM.same_records(p, rec) and damage_rows(p) == model[3] == [(3, 1), (3, 0)]
    validates(p)


def test_a_picture_without_any_slice_is_still_rejected():
    es = generate_es(**CS.MULTI)
    w, h, cf = PM.geom(CS.MULTI)
    cut = CS.delete_slices(es, [j for j, t in enumerate(CS.slice_table(es)) if t[0] == 4])
    plain = PM.host(cut, w, h, cf)
    assert plain[0] == -6 and "picture without slices" in plain[1]
    for make in (lambda: Parsed(cut, w, h, cf, conceal=True), lambda: Scan(cut, w, h, cf, conceal=True)):
        with pytest.raises(_lib.Mp2vgError) as ei:
            make()
        assert (ei.value.status, PM.detail(str(ei.value))) == (plain[0], PM.detail(plain[1]))


def test_rows_outside_the_picture_and_doubled_rows_stay_rejections():
    es = generate_es(**CS.MULTI)
    w, h, cf = PM.geom(CS.MULTI)
    table = CS.slice_table(es)
    for row_byte, text in [(4, "slice row outside the picture"), (1, "two slices in one macroblock row")]:
        b = PM.mutate(es, table[4][2] + 3, row_byte)  # picture 1 row 1 renamed
        plain = PM.host(b, w, h, cf)
        assert plain[0] == -2 and text in plain[1]
        for make in (lambda: Parsed(b, w, h, cf, threads=1, conceal=True), lambda: Scan(b, w, h, cf, conceal=True)):
            with pytest.raises(_lib.Mp2vgError) as ei:
                make()
            assert ei.value.status == -2 and text in str(ei.value)


# ---- geometry corners ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CS.CORNERS))
def test_geometry_corners(name):
    kw = CS.CORNERS[name]
    bad, es, w, h, cf, _ = CS.damaged_stream(kw, CS.CORNER_DAMAGE)
    base = Parsed(es, w, h, cf)
    assert list(base.pics["picture_coding_type"]) == [1, 2, 2]
    p, rec = flagged(bad, w, h, cf)
    model = CM.conceal(base, CS.CORNER_DAMAGE)
    same_as_model(p, model)
    assert PM.same_records(p, rec) and damage_rows(p) == CS.CORNER_DAMAGE
    mbw, nb = w // 16, CM.NBLOCKS[cf]
    grey = p.mbs[:mbw]
    assert (grey["ncoef"] == nb).all() and (grey["cbp"] == (1 << nb) - 1).all()
    assert list(grey["coef_off"]) == [x * nb for x in range(mbw)]
    # the words after the grey row start where it ends
    if h > 16:
        assert p.mbs["coef_off"][mbw] == mbw * nb
    else:
        assert p.mbs["coef_off"][mbw] == mbw * nb == int(p.pics["mb_first"][1]) * nb
    validates(p)
    # (no literal pixel value: the DC word is outside the mismatch control, which so toggles
    # coefficient 63 of every grey block; the oracle's output on the model's records is the statement)
    got, want = oracle_frames(p), oracle_frames(as_parsed(p, *model[:3]))
    assert all(np.array_equal(x, y) for a, b in zip(got, want) for x, y in zip(a, b))
    assert abs(int(got[0][0][:16].astype(int).mean()) - 128) <= 1


# ---- pinned by the compiled reference ----------------------------------------------------------------------
def test_fixtures_are_what_the_committed_script_builds():
    for e in CS.load_fixtures():
        pct, (pic, row) = CS.REPAIR_CASES[e["name"]]
        bad, es, w, h, cf, why = CS.damaged_stream(CS.REPAIR, [(pic, row)])
        assert (e["picture"], e["row"], e["picture_coding_type"], e["reason"]) == (pic, row, pct, why[(pic, row)])
        assert bad == e["damaged_es"] and CS.repaired(bad, w, h, cf, pct, pic, row) == e["repaired_es"]


@pytest.mark.parametrize("e", CS.load_fixtures(), ids=lambda e: e["name"])
def test_concealed_stream_decodes_as_the_repaired_stream_the_reference_decoded(e):
    w, h, cf = e["width"], e["height"], e["chroma_format"]
    hs, hm, _ = PM.host(e["damaged_es"], w, h, cf)
    assert hs != 0 and e["reason"] in hm
    fixed = Parsed(e["repaired_es"], w, h, cf)  # no flag: the repaired stream is legal
    p, rec = flagged(e["damaged_es"], w, h, cf)
    assert damage_rows(p) == [(e["picture"], e["row"])] and PM.same_records(p, rec)
    got, want = oracle_frames(p), oracle_frames(fixed)
    assert len(got) == len(want) == e["frames"]
    for a, b in zip(got, want):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert [yuv_md5(got[int(d)]) for d in p.display] == e["md5"]
    assert [yuv_md5(want[int(d)]) for d in fixed.display] == e["md5"]


# ---- the emitter and the twin under the sanitizers -----------------------------------------------------------
@pytest.fixture(scope="module")
def conceal_check(tmp_path_factory):
    """tests/fuzz/conceal_check.cpp, a program of its own, with the host emitter, the scan, the twin
    and the batch validation under AddressSanitizer and UndefinedBehaviorSanitizer (CPU only)"""
    import os
    import subprocess
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(repo, "tiny_mp2v_dec_amd", "csrc")
    exe = str(tmp_path_factory.mktemp("san_conceal") / "conceal_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I", csrc,
           "-I", os.path.join(repo, "include"), os.path.join(repo, "tests", "fuzz", "conceal_check.cpp"),
           os.path.join(csrc, "parse.cpp"), os.path.join(csrc, "tables.cpp"), os.path.join(csrc, "runtime.cpp"),
           "-o", exe, "-pthread", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        pytest.fail(f"sanitizer build failed:\n{r.stderr[-2000:]}")
    return exe


def test_emitter_and_twin_conceal_mutants_under_asan_ubsan(conceal_check, tmp_path):
    import json
    import os
    import subprocess
    from conftest import STREAMS
    man = {m["name"]: m for m in load_manifest()}
    multi = tmp_path / "multi.m2v"
    multi.write_bytes(generate_es(**CS.MULTI))  # two GOPs: re-typed I pictures
    args = [str(multi)] + [str(v) for v in PM.geom(CS.MULTI)]
    for n in ("ipb420_field", "ipb422_field", "ipb444_field"):
        m = man[n]
        args += [os.path.join(STREAMS, m["file"]), str(m["width"]), str(m["height"]), str(m["chroma_format"])]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([conceal_check, "500", "11"] + args, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    res = json.loads(r.stdout.strip().splitlines()[-1])
    print(res)
    assert res["mutants_concealed"] > 500 and res["rows_replaced"] > res["mutants_concealed"]
    assert res["mutants_rejected"] > 100 and res["mutants_clean"] > 0 and res["pictures_retyped"] > 0
