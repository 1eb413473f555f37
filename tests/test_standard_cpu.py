"""CPU: MP2VG_PARSE_STANDARD in the host emitter (csrc/parse.cpp) and the CPU twin of the device
parse (csrc/slice_parse.h), and mp2vg_probe_es.

The pin is the twin streams of tests/standard_streams.py (tests/golden/standard/): S' in the
standard's form under the flag must give the macroblock records, coefficient words and picture
records (W among them) that S, the same pictures in the reference's subset, gives without it, and
so its frames carry the MD5s the compiled reference computed for S.  With the flag clear nothing
changes: every S' is rejected as it was, and every existing syntax fixture parses to the same bytes
under the flag, but for the 4:2:2 and 4:4:4 ones with chroma matrices of their own, which meet the
one limit the flag keeps.

Planted defects (each applied in a scratch copy of parse.cpp / slice_parse.h; DESIGN.md §3 records
the tests that then fail): no reset at a repeated sequence header, an intra load not copied to
chroma, a partial extension clearing what it does not load, the default intra matrix taken as
zigzag, state in display order, '1s' in a format-0 intra block, '10' after the DC read as a
coefficient, format 0 for the whole stream, the 4:2:2 limit not enforced."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import directed_syntax as DS
import parse_mutants as PM
import standard_streams as SS
from conftest import GOLDEN
from helpers import oracle_frames, yuv_md5
from tiny_mp2v_dec_amd import _lib
from tiny_mp2v_dec_amd.records import Parsed, Scan, damage_reason, probe

MANIFEST = SS.load_manifest()
TWINS = [e for e in MANIFEST if e["md5"] is not None]
REFUSED = [e for e in MANIFEST if e["md5"] is None]
IDS = [e["name"] for e in TWINS]
SYNTAX = os.path.join(GOLDEN, "syntax")
with open(os.path.join(SYNTAX, "manifest.json")) as _f:
    SYNTAX_MANIFEST = json.load(_f)
# the existing fixtures whose pictures load chroma matrices of their own in 4:2:2 / 4:4:4
CHROMA_OF_THEIR_OWN = {"matrices_422", "matrices_444"}


def geom(e):
    return e["width"], e["height"], e["chroma_format"]


def host(es, w, h, cf, **kw):
    try:
        return 0, "", Parsed(es, w, h, cf, threads=1, **kw)
    except _lib.Mp2vgError as e:
        return e.status, str(e), None


def twin(es, w, h, cf, **kw):
    """(status, message, scan's picture records, (mbs, coefs)) of the scan and the CPU twin"""
    try:
        with Scan(es, w, h, cf, **kw) as sc:
            return 0, "", sc.pics.copy(), sc.parse_host()
    except _lib.Mp2vgError as e:
        return e.status, str(e), None, None


@pytest.fixture(scope="module")
def written():
    """every twin pair, written once: {name: (S', S)}"""
    return {std.name: (std, ref) for std, ref in SS.build_all()}


@pytest.fixture(scope="module")
def refs():
    """{name: Parsed of the twin S, without the flag}: what every parse of S' under the flag must give"""
    return {e["name"]: Parsed(SS.read(e, "ref"), *geom(e), threads=1) for e in TWINS}


@pytest.fixture(scope="module")
def flagged():
    """name -> Parsed of S' by the host emitter under the flag, parsed on first use (a stream the
    emitter refuses fails the tests that ask for it, not the others)"""
    done = {}

    def get(e):
        if e["name"] not in done:
            done[e["name"]] = Parsed(SS.read(e, "std"), *geom(e), threads=1, standard=True)
        return done[e["name"]]
    return get


# ---- the fixtures ------------------------------------------------------------------------------------
def test_fixture_is_what_the_writer_writes(written):
    assert sorted(written) == sorted(IDS)
    for e in TWINS:
        std, ref = written[e["name"]]
        assert SS.read(e, "std") == std.es and SS.read(e, "ref") == ref.es, e["name"]
        assert geom(e) + (e["frames"],) == (std.width, std.height, std.cf, std.npics)
        assert e["events"] == sorted(std.events)
        assert max(std.width, ref.width) <= 64 and max(std.height, ref.height) <= 48
    S = SS.refused_422()
    assert SS.read(REFUSED[0], "std") == S.es and REFUSED[0]["reason"] == SS.REFUSED_422_REASON
    total = sum(os.path.getsize(os.path.join(SS.GOLDEN, n)) for n in os.listdir(SS.GOLDEN))
    assert total < 256 * 1024


def test_every_event_is_exercised(written):
    got = set().union(*(std.events for std, _ in written.values()))
    got = {e for e in got if e.startswith("std:")}
    want = set(SS.REQUIRED_EVENTS)
    assert len(want) == len(SS.REQUIRED_EVENTS)
    assert not want - got, sorted(want - got)
    assert got == want
    assert {e for m in TWINS for e in m["events"] if e.startswith("std:")} == want  # and so says the fixture


def test_the_writer_states_the_matrix_rule_itself():
    """spot checks of MatrixState against 6.3.11's text, so that a twin S is known to carry what the
    standard says and not what the library computes"""
    st = SS.MatrixState()
    assert st.m[0][:6] == [8, 16, 16, 19, 16, 19] and st.m[0][63] == 83 and st.m[1] == [16] * 64
    assert st.m[0][6:12] == [22] * 6 and st.m[0][12] == 26  # raster 3, 10, 17, 24, 32, 25; then 18
    assert st.m[2] == st.m[0] and st.m[3] == st.m[1]
    a, b, c = SS.rising(0), SS.rising(1), SS.rising(2)
    st.extension({0: a})
    assert st.m == [a, [16] * 64, a, [16] * 64]
    st.extension({1: b, 2: c})
    assert st.m == [a, b, c, b]
    st.extension({0: b, 2: a})  # field order: intra (and its copy) first, then chroma_intra itself
    assert st.m == [b, b, a, b]
    st.sequence_header(None, c)
    assert st.m == [SS.DEFAULT_INTRA, c, SS.DEFAULT_INTRA, c]


# ---- 1-3: emitter, twin, oracle ---------------------------------------------------------------------------
@pytest.mark.parametrize("e", TWINS, ids=IDS)
def test_emitter_under_the_flag_equals_the_emitter_on_the_twin(e, flagged, refs, written):
    p, q = flagged(e), refs[e["name"]]
    assert p.npics == q.npics == e["frames"]
    assert p.mbs.tobytes() == q.mbs.tobytes()
    assert p.coefs.tobytes() == q.coefs.tobytes()
    for k in range(p.npics):  # picture by picture, matrix by matrix, so that a failure names them
        for m in range(4):
            assert p.pics["W"][k][m].tolist() == q.pics["W"][k][m].tolist(), (k, m)
    assert p.pics.tobytes() == q.pics.tobytes()
    assert p.display.tolist() == q.display.tolist()
    # ... and both are the writer's model: its records, and the W of its own statement of the rule
    std, _ = written[e["name"]]
    want_mbs, want_coefs = DS.records(std)
    assert p.mbs.tobytes() == want_mbs.tobytes() and p.coefs.tobytes() == want_coefs.tobytes()
    assert p.pics["W"].tolist() == std.W


@pytest.mark.parametrize("e", TWINS, ids=IDS)
def test_cpu_twin_under_the_flag_gives_the_same_bytes(e, refs):
    p = refs[e["name"]]  # (the twin S by the emitter without the flag: no code under test but the twin's)
    st, msg, pics, rec = twin(SS.read(e, "std"), *geom(e), standard=True)
    assert st == 0, msg
    assert pics.tobytes() == p.pics.tobytes()
    assert PM.same_records(p, rec)
    # picture ranges that start inside the stream (the drop-in's chunks): the state is the scan's
    if p.npics > 4:
        with Scan(SS.read(e, "std"), *geom(e), standard=True) as sc:
            for first, n in ((3, 2), (p.npics - 3, 3)):
                want = PM.range_of_whole(p, first, n)
                got = sc.parse_host(first, n)
                assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


@pytest.mark.parametrize("e", TWINS, ids=IDS)
def test_oracle_frames_carry_the_reference_md5s(e, flagged):
    p = flagged(e)
    frames = oracle_frames(p)
    assert [yuv_md5(frames[d]) for d in p.display] == e["md5"]


@pytest.mark.parametrize("e", TWINS, ids=IDS)
def test_flag_with_conceal_changes_nothing_on_a_clean_stream(e, refs):
    p = refs[e["name"]]
    c = Parsed(SS.read(e, "std"), *geom(e), threads=1, standard=True, conceal=True)
    assert len(c.damage) == 0 and PM.same_records(p, (c.mbs, c.coefs))
    assert c.pics["W"].tobytes() == p.pics["W"].tobytes()
    st, msg, _, rec = twin(SS.read(e, "std"), *geom(e), standard=True, conceal=True)
    assert st == 0 and PM.same_records(p, rec), msg


# ---- 4: the flag clear ---------------------------------------------------------------------------------
@pytest.mark.parametrize("e", TWINS, ids=IDS)
def test_flag_clear_rejects_every_standard_stream_as_before(e):
    es = SS.read(e, "std")
    hs, hm, _ = host(es, *geom(e))
    ts, tm, _, _ = twin(es, *geom(e))
    assert hs == ts == SS.CLEAR_STATUS
    assert SS.CLEAR_REASON in hm and PM.detail(hm) == PM.detail(tm)
    assert PM.detail(hm) == "picture without a full quant_matrix_extension (reference decoder.cpp:185-191)"


@pytest.mark.parametrize("build", SS.FORMAT0_BUILDERS, ids=lambda b: b.__name__)
def test_flag_clear_keeps_the_intra_vlc_format_rejection(build):
    """S' with a full extension on every picture: the flag-clear parsers get as far as the first
    intra macroblock of the first format-0 picture (picture 0, row 0) and refuse it there, as ever;
    under CONCEAL alone every row of a format-0 picture that holds an intra macroblock is replaced;
    under the flag the stream gives the records of its twin."""
    S = build("std", full_ext=True)
    w, h, cf = S.width, S.height, S.cf
    hs, hm, _ = host(S.es, w, h, cf)
    ts, tm, _, _ = twin(S.es, w, h, cf)
    assert hs == ts == -2 and PM.detail(hm) == PM.detail(tm)
    assert PM.detail(hm).startswith("picture 0 slice @") and SS.CLEAR_IVF0_REASON in hm
    c = Parsed(S.es, w, h, cf, threads=1, conceal=True)
    assert len(c.damage) and all(damage_reason(d["reason"]).startswith(SS.CLEAR_IVF0_REASON) for d in c.damage)
    assert (0, 0) in [(int(d["pic"]), int(d["mb_row"])) for d in c.damage]
    ref = build("ref")
    p, q = Parsed(S.es, w, h, cf, threads=1, standard=True), Parsed(ref.es, w, h, cf, threads=1)
    assert PM.same_records(p, (q.mbs, q.coefs)) and p.pics.tobytes() == q.pics.tobytes()


def test_flag_clear_ignores_sequence_header_matrices():
    """sequence-header matrices stay parsed and ignored without the flag: W is the extension's"""
    S = SS.MATRIX_BUILDERS[3]("std", full_ext=True)  # the header loads both, every picture a full extension
    p = Parsed(S.es, S.width, S.height, S.cf, threads=1)
    assert p.pics["W"].tolist() == S.W
    sh = p.headers.sequence_header
    assert sh.load_intra_quantiser_matrix == 1 and list(sh.intra_quantiser_matrix) == SS.rising(0)
    assert sh.load_non_intra_quantiser_matrix == 1 and list(sh.non_intra_quantiser_matrix) == SS.rising(1)


# ---- the limit that stays: chroma matrices of their own in 4:2:2 / 4:4:4 -------------------------------------
def test_422_with_a_different_chroma_matrix_is_refused_at_the_picture_level():
    e = REFUSED[0]
    es = SS.read(e, "std")
    hs, hm, _ = host(es, *geom(e), standard=True)
    ts, tm, _, _ = twin(es, *geom(e), standard=True)
    assert hs == ts == e["status"] == -2
    assert PM.detail(hm) == PM.detail(tm) and PM.detail(hm).startswith(e["reason"])
    assert "slice" not in hm  # a picture-level refusal, not a row's
    hs, hm, _ = host(es, *geom(e), standard=True, conceal=True)  # ... which CONCEAL does not soften
    assert hs == -2 and e["reason"] in hm
    # the same pictures in 4:2:0 are the standard's own case and decode
    S = SS.StdStream("p", 64, 48, 1, "std")
    pics, trefs = SS.ipbb(S, DS._rng("p"), {1: dict(ext={2: SS.rising(3)})})
    p = Parsed(S.write(pics, trefs), 64, 48, 1, threads=1, standard=True)
    assert p.pics["W"].tolist() == S.W and S.W[1][2] != S.W[1][0]


# ---- 5: the existing syntax fixtures under the flag --------------------------------------------------------------
@pytest.mark.parametrize("e", SYNTAX_MANIFEST, ids=[e["name"] for e in SYNTAX_MANIFEST])
def test_existing_syntax_fixtures_under_the_flag(e):
    with open(os.path.join(SYNTAX, e["file"]), "rb") as f:
        es = f.read()
    hs0, hm0, p0 = host(es, *geom(e))
    hs, hm, p = host(es, *geom(e), standard=True)
    ts, tm, pics, rec = twin(es, *geom(e), standard=True)
    if e["name"] in CHROMA_OF_THEIR_OWN:
        assert hs0 == 0 and hs == ts == -2
        assert PM.detail(hm) == PM.detail(tm)
        assert PM.detail(hm).startswith("picture 0: chroma quantiser matrices differ from the luma ones in 4:")
    elif e["md5"] is None:  # the out-of-contract streams stay out of it, for the same reason
        assert (hs, PM.detail(hm)) == (hs0, PM.detail(hm0)) and hs == e["status"] and e["reason"] in hm
        assert ts == hs and PM.detail(tm) == PM.detail(hm)
    else:
        assert hs0 == hs == ts == 0, (hm0, hm, tm)
        assert p.pics.tobytes() == p0.pics.tobytes() == pics.tobytes()
        assert PM.same_records(p0, (p.mbs, p.coefs)) and PM.same_records(p0, rec)


# ---- 6: mp2vg_probe_es --------------------------------------------------------------------------------------
def headers(h, v, cf=1, progressive=1, mpeg1=False, display=None, aspect=1, user_data=False):
    """a sequence_header, its sequence_extension (not for mpeg1), optionally user data and a
    sequence_display_extension, then a group_of_pictures_header"""
    b = DS.Bits()
    b.start_code(0xB3)
    b.put(h & 0xFFF, 12), b.put(v & 0xFFF, 12), b.put(aspect, 4), b.put(3, 4), b.put(0x3FFFF, 18)
    b.put(1, 1), b.put(0x3FF, 10), b.put(0, 1), b.put(0, 1), b.put(0, 1)
    if not mpeg1:
        b.start_code(0xB5)
        b.put(1, 4), b.put(0x44, 8), b.put(progressive, 1), b.put(cf, 2), b.put(h >> 12, 2), b.put(v >> 12, 2)
        b.put(0, 12), b.put(1, 1), b.put(0, 8), b.put(0, 1), b.put(0, 2), b.put(0, 5)
    if user_data:
        b.start_code(0xB2)
        b.put(0x55AA, 16)
    if display:
        b.start_code(0xB5)
        b.put(2, 4), b.put(1, 3), b.put(1, 1), b.put(5, 8), b.put(5, 8), b.put(5, 8)
        b.put(display[0], 14), b.put(1, 1), b.put(display[1], 14)
    b.start_code(0xB8)
    b.put(0, 25), b.put(1, 1), b.put(0, 1)
    b.align()
    return b.bytes()


@pytest.mark.parametrize("h,v,progressive,cf,want", [
    (16, 16, 1, 1, (16, 16)), (16, 16, 0, 1, (16, 32)),
    (1920, 1080, 1, 1, (1920, 1088)), (1920, 1080, 0, 1, (1920, 1088)),
    (1280, 720, 0, 1, (1280, 736)), (1280, 720, 1, 1, (1280, 720)),
    (720, 576, 0, 2, (720, 576)), (360, 243, 1, 3, (368, 256)), (360, 243, 0, 3, (368, 256)),
    (4097, 2801, 1, 1, (4112, 2816)), (16383, 16383, 1, 1, (16384, 16384)), (16383, 16383, 0, 2, (16384, 16384)),
])
def test_probe_coded_size(h, v, progressive, cf, want):
    r = probe(headers(h, v, cf, progressive))
    assert (r["width"], r["height"]) == want and r["chroma_format"] == cf
    assert (r["display_width"], r["display_height"]) == (h, v)
    assert r["headers"].sequence_extension.progressive_sequence == progressive
    _lib.geometry(r["width"], r["height"], cf)  # a config every other entry point takes


def test_probe_headers_and_untouched_fields():
    es = b"\x00\x00\x01\xb2junk" + headers(720, 576, 2, 0, display=(704, 572), aspect=3, user_data=True)
    cfg = _lib.make_config(1, 2, 3, pool=7, threads=5, reordering=False, device=2, flags=24)
    hd = _lib.StreamHeaders()
    buf = np.frombuffer(es, np.uint8)
    assert _lib.lib().mp2vg_probe_es(buf.ctypes.data_as(ctypes.c_void_p), len(es), ctypes.byref(cfg), ctypes.byref(hd)) == 0
    assert (cfg.width, cfg.height, cfg.chroma_format) == (720, 576, 2)
    assert (cfg.pictures_pool_size, cfg.num_threads, cfg.reordering, cfg.device, cfg.reserved) == (7, 5, 0, 2, 24)
    assert hd.have_sequence_display_extension == 1 and hd.have_group_of_pictures_header == 0
    de = hd.sequence_display_extension
    assert (de.display_horizontal_size, de.display_vertical_size, de.matrix_coefficients) == (704, 572, 5)
    assert hd.sequence_header.aspect_ratio_information == 3
    from tiny_mp2v_dec_amd.records import export_matrix, pixel_aspect
    assert export_matrix(hd) == 5 and pixel_aspect(hd) == (13, 9)  # 16:9 of 704 x 572: (16 * 572) : (9 * 704)
    # the headers argument is optional
    cfg2 = _lib.make_config(0, 0, 0)
    assert _lib.lib().mp2vg_probe_es(buf.ctypes.data_as(ctypes.c_void_p), len(es), ctypes.byref(cfg2), None) == 0
    assert (cfg2.width, cfg2.height, cfg2.chroma_format) == (720, 576, 2)


@pytest.mark.parametrize("e", MANIFEST, ids=[e["name"] for e in MANIFEST])
def test_probe_on_the_fixtures(e):
    r = probe(SS.read(e, "std"))
    # (the writer's sequences are interlaced, progressive_sequence = 0, though its pictures hold the
    # 3 macroblock rows of a progressive one: 48 lines probe as 64 coded lines, 32 as 32)
    assert (r["width"], r["chroma_format"]) == (e["width"], e["chroma_format"])
    assert r["display_height"] == e["height"] and r["height"] == (e["height"] + 31) // 32 * 32


def test_probe_refusals():
    def refused(es):
        with pytest.raises(_lib.Mp2vgError) as x:
            probe(es)
        return x.value.status, str(x.value)

    st, msg = refused(headers(352, 288, mpeg1=True))
    assert st == -2 and "MPEG-1" in msg
    st, msg = refused(b"")
    assert st == -6 and "no sequence_header" in msg  # MP2VG_E_BITSTREAM
    st, msg = refused(headers(352, 288)[4:])  # the start code cut off: extension and group header only
    assert st == -6
    st, msg = refused(b"\x00\x00\x01")
    assert st == -6
    # No stream can carry a size above MP2VG_MAX_DIMENSION: 12 + 2 bits end at 16383, coded as 16384
    # (test_probe_coded_size).  The size a stream CAN carry outside the limits is 0.
    st, msg = refused(headers(0, 288))
    assert st == -2 and "MP2VG_MAX_DIMENSION" in msg
    st, msg = refused(headers(352, 288, cf=0))
    assert st == -2 and "chroma_format" in msg
    cfg = _lib.make_config(5, 6, 7)
    assert _lib.lib().mp2vg_probe_es(None, 0, None, None) == -1
    es = np.frombuffer(headers(352, 288, mpeg1=True), np.uint8)
    assert _lib.lib().mp2vg_probe_es(es.ctypes.data_as(ctypes.c_void_p), len(es), ctypes.byref(cfg), None) == -2
    assert (cfg.width, cfg.height, cfg.chroma_format) == (5, 6, 7)  # written only on success


# ---- 8: the emitter, the scan and the twin under the sanitizers ------------------------------------------------
@pytest.fixture(scope="module")
def standard_check(tmp_path_factory):
    """tests/fuzz/standard_check.cpp, a program of its own, with parse.cpp and tables.cpp under
    AddressSanitizer and UndefinedBehaviorSanitizer (CPU only)"""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(repo, "tiny_mp2v_dec_amd", "csrc")
    exe = str(tmp_path_factory.mktemp("san_standard") / "standard_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I", csrc,
           "-I", os.path.join(repo, "include"), os.path.join(repo, "tests", "fuzz", "standard_check.cpp"),
           os.path.join(csrc, "parse.cpp"), os.path.join(csrc, "tables.cpp"), "-o", exe, "-pthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        pytest.fail(f"sanitizer build failed:\n{r.stderr[-2000:]}")
    return exe


def test_emitter_scan_and_twin_under_asan_ubsan(standard_check):
    args = []
    for e in MANIFEST:
        args += [os.path.join(SS.GOLDEN, e["std"]), str(e["width"]), str(e["height"]), str(e["chroma_format"])]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([standard_check, "150", "16"] + args, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    res = json.loads(r.stdout.strip().splitlines()[-1])
    print(res)
    assert res["streams"] == len(MANIFEST) and res["accepted"] > 200 and res["rejected"] > 200
    assert res["concealed"] > 100 and res["probe_ok"] > 200
