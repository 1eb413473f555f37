"""CPU: the motion export's definition (include/mp2vg.h "motion export") through its host twin,
mp2vg_motion_records: literal cases with the expected numbers written out, the vertical conversion
and the sign convention pinned to the oracle's decoded pixels, the numpy model (motion_model.py)
against the twin on every golden stream and on the independent writer's records, the arguments,
reference_pictures / dist, and the twin under AddressSanitizer + UndefinedBehaviorSanitizer in a
stand-alone program (tests/fuzz/motion_check.cpp)."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import directed_syntax as DS
import motion_model as MM
from conftest import GOLDEN, load_manifest, read_stream
from helpers import _inside, fill_mb, oracle_frames
from tiny_mp2v_dec_amd import _lib
from tiny_mp2v_dec_amd import records as R
from tiny_mp2v_dec_amd._lib import COEF_DC, COEF_FIRST1S, MB_BWD, MB_FIELD_MC, MB_FWD, MB_INTRA, mb_fs_bit

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "tiny_mp2v_dec_amd", "csrc")
MANIFEST = load_manifest()
SYNTAX = os.path.join(GOLDEN, "syntax")
with open(os.path.join(SYNTAX, "manifest.json")) as _f:
    SYNTAX_POSITIVE = [e for e in json.load(_f) if e["md5"] is not None]
NB = {1: 6, 2: 8, 3: 12}


class Holder:  # what oracle_frames reads of a Parsed
    def __init__(self, w, h, cf, pics, mbs, coefs):
        self.width, self.height, self.chroma_format = w, h, cf
        self.pics, self.mbs, self.coefs, self.npics = pics, mbs, coefs, len(pics)


def make_pics(types, refs, mbw, mbh):
    """Picture records: types[i] = 1 / 2 / 3, refs[i] = (fwd_slot, bwd_slot); slot = index."""
    pics = np.zeros(len(types), R.PIC_DTYPE)
    for p, (t, (f, b)) in enumerate(zip(types, refs)):
        pics[p]["dst_slot"], pics[p]["fwd_slot"], pics[p]["bwd_slot"] = p, f, b
        pics[p]["picture_coding_type"] = t
        pics[p]["mb_first"] = p * mbw * mbh
        pics[p]["mb_width"], pics[p]["mb_height"] = mbw, mbh
        pics[p]["W"] = 16
    return pics


def both(pics, mbs, coefs, w, h, cf, order=None):
    """(mv, info, act) of the model after checking that the host twin gives the same."""
    want = MM.model(pics, mbs, coefs, cf, order)
    got = R.motion_host(pics, mbs, coefs, w, h, cf, order)
    for name, a, b in zip(("mv", "info", "act"), got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, name
        assert np.array_equal(a, b), name
    return want


# ---- literal cases ----------------------------------------------------------------------------
def literal_batch():
    """64 x 64 4:2:0: I, P, then a B picture whose MBs are written by hand (the others: skipped-like
    forward MBs with a zero vector)."""
    w = h = 64
    mbw = mbh = 4
    n = mbw * mbh
    pics = make_pics([1, 2, 3], [(-1, -1), (0, -1), (0, 1)], mbw, mbh)
    mbs = np.zeros(3 * n, R.MB_DTYPE)
    coefs = []
    for p in range(3):
        for k in range(n):
            m = mbs[p * n + k]
            m["x"], m["y"], m["qscale"] = k % mbw, k // mbw, 8
            m["flags"], m["cbp"] = (MB_INTRA, 63) if p == 0 else (MB_FWD, 0)
    B = mbs[2 * n:]

    def tag(m):
        return (int(m["x"]) & 7) << 26

    # (1, 1): field MC forward, r = 0 reads the bottom field (sel = 1), r = 1 the top field (sel = 0)
    m = B[1 * mbw + 1]
    m["flags"] = MB_FWD | MB_FIELD_MC | mb_fs_bit(0, 0)
    m["mv"][0, 0], m["mv"][1, 0] = (2, -3), (-2, 5)
    m["mv"][0, 1], m["mv"][1, 1] = (123, -321), (-77, 55)  # junk in the unused backward vectors
    # (2, 1): frame MC forward, junk in vector 1
    m = B[1 * mbw + 2]
    m["flags"] = MB_FWD
    m["mv"][0, 0], m["mv"][1, 0] = (3, -2), (99, 77)
    # (1, 2): intra with junk vectors; a DC word and one AC word in block 0
    m = B[2 * mbw + 1]
    m["flags"], m["cbp"] = MB_INTRA, 63
    m["mv"][:] = [[[11, -12], [13, -14]], [[15, -16], [17, -18]]]
    # (2, 2): backward only, junk in the forward vectors
    m = B[2 * mbw + 2]
    m["flags"] = MB_BWD
    m["mv"][0, 1], m["mv"][0, 0], m["mv"][1, 0] = (4, 2), (1000, -1000), (-999, 999)
    # (0, 3): not intra, neither direction bit: forward
    m = B[3 * mbw + 0]
    m["flags"] = 0
    m["mv"][0, 0] = (4, -6)
    # (3, 3): bidirectional field MC
    m = B[3 * mbw + 3]
    m["flags"] = MB_FWD | MB_BWD | MB_FIELD_MC | mb_fs_bit(1, 0) | mb_fs_bit(0, 1)
    m["mv"][0, 0], m["mv"][1, 0], m["mv"][0, 1], m["mv"][1, 1] = (-6, -4), (-8, -2), (0, -1), (-1, -7)
    # (3, 0): forward with residual: a '1s' word of level -1 and a run-level word in block 2
    m = B[0 * mbw + 3]
    m["cbp"] = 1 << 2
    # coefficient words, laid out in raster order (rows contiguous)
    for p in range(3):
        for k in range(n):
            m = mbs[p * n + k]
            m["coef_off"] = len(coefs)
            if p == 2 and k == 2 * mbw + 1:
                coefs += [(100 & 0xFFFF) | (0 << 22) | COEF_DC | tag(m), (5 & 0xFFFF) | (1 << 16) | tag(m),
                          (-9 & 0xFFFF) | (2 << 16) | (5 << 22) | tag(m)]
            if p == 2 and k == 3:
                coefs += [(-1 & 0xFFFF) | (2 << 22) | COEF_FIRST1S | tag(m), (-7 & 0xFFFF) | (3 << 16) | (2 << 22) | tag(m)]
            m["ncoef"] = len(coefs) - int(m["coef_off"])
    return w, h, pics, mbs, np.array(coefs, np.uint32)


def test_literal_cases():
    w, h, pics, mbs, coefs = literal_batch()
    R.validate_batch(w, h, 1, 3, pics, mbs, coefs)  # the junk-carrying records are in contract
    mv, info, act = both(pics, mbs, coefs, w, h, 1)
    b = 2

    def vec(x, y):
        return mv[b, :, y, x].tolist()

    # channel c = 4 s + 2 r + k
    assert vec(1, 1) == [2, -4, -2, 8, 0, 0, 0, 0]       # mv_y -3, sel 1, r 0: -4;  mv_y 5, sel 0, r 1: 8
    assert vec(2, 1) == [3, -2, 3, -2, 0, 0, 0, 0]       # frame MC: duplicated into r = 1
    assert vec(1, 2) == [0] * 8                          # intra: junk ignored
    assert vec(2, 2) == [0, 0, 0, 0, 4, 2, 4, 2]         # backward only: forward junk ignored
    assert vec(0, 3) == [4, -6, 4, -6, 0, 0, 0, 0]       # neither bit: forward
    assert vec(3, 3) == [-6, -8, -8, -4, 0, 0, -1, -16]  # fwd (r0 sel0, r1 sel1), bwd (r0 sel1, r1 sel0)
    assert vec(0, 0) == [0] * 8 and mv[0].any() == False and mv[1].any() == False  # noqa: E712
    assert info[b, :, 1, 1].tolist() == [MB_FWD | MB_FIELD_MC | 0x100, 0, 8, 0]
    assert info[b, :, 2, 1].tolist() == [MB_INTRA, 63, 8, 3]
    assert info[b, :, 0, 3].tolist() == [MB_FWD, 4, 8, 2]
    assert info[0, :, 0, 0].tolist() == [MB_INTRA, 63, 8, 0]
    # intra MB: the DC word is counted in plane 0 and not summed in plane 1
    assert act[b, 0, :, 2, 1].tolist() == [2, 0, 0, 0, 0, 1] and act[b, 1, :, 2, 1].tolist() == [5, 0, 0, 0, 0, 9]
    # '1s' word of level -1 adds 1
    assert act[b, 0, :, 0, 3].tolist() == [0, 0, 2, 0, 0, 0] and act[b, 1, :, 0, 3].tolist() == [0, 0, 8, 0, 0, 0]
    assert act.sum() == 2 + 1 + 2 + 5 + 9 + 8


def test_words_of_blocks_the_format_lacks_are_ignored():
    """The MODEL's per-word rule alone: block index >= B adds nothing.  This covers only
    motion_model.mb_activity, not the library: the validation of mp2vg_batch_upload and of
    mp2vg_motion_records refuses a word of a block the MB's cbp does not code (and a cbp bit
    >= B), so no batch a test can make resident reaches that branch of motion_word."""
    words = [(3 & 0xFFFF) | (7 << 22), (-32768 & 0xFFFF) | (5 << 22), (4 & 0xFFFF) | (11 << 22)]
    assert MM.mb_activity(words, 6) == ([0, 0, 0, 0, 0, 1], [0, 0, 0, 0, 0, 32768])
    assert MM.mb_activity(words, 8)[0] == [0, 0, 0, 0, 0, 1, 0, 1]


# ---- the formula pinned to decoded pixels -----------------------------------------------------
def fullpel_batch(seed=7):
    """96 x 96 4:2:0: a random intra picture, then P (forward from it), a backward-only B and a
    forward-only B, every MB non-intra with cbp = 0 and full-pel luma vectors after conversion."""
    w = h = 96
    mbw = mbh = 6
    n = mbw * mbh
    rng = np.random.default_rng(seed)
    pics = make_pics([1, 2, 3, 3], [(-1, -1), (0, -1), (0, 1), (0, 1)], mbw, mbh)
    pics[0]["W"] = rng.integers(8, 40, size=(4, 64))
    mbs = np.zeros(4 * n, R.MB_DTYPE)
    coefs = []
    for k in range(n):
        m = mbs[k]
        m["x"], m["y"] = k % mbw, k // mbw
        fill_mb(rng, m, coefs, w, h, 1, True, [MB_FWD])
    for p, direction in ((1, MB_FWD), (2, MB_BWD), (3, MB_FWD)):
        s = 1 if direction == MB_BWD else 0
        for k in range(n):
            m = mbs[p * n + k]
            m["x"], m["y"], m["qscale"], m["coef_off"] = k % mbw, k // mbw, 4, len(coefs)
            field = (k + p) % 3 != 0
            flags = direction | (MB_FIELD_MC if field else 0)
            for r in range(2 if field else 1):
                for _ in range(200):
                    sel = int(rng.integers(0, 2)) if field else 0
                    mx, my = 2 * int(rng.integers(-12, 13)), 2 * int(rng.integers(-12, 13))
                    if _inside(w, h, 1, k % mbw, k // mbw, mx, my, field, sel):
                        break
                else:
                    raise AssertionError("no vector fits")
                m["mv"][r, s] = (mx, my)
                m["mv"][r, 1 - s] = (2 * int(rng.integers(-300, 300)) + 1, 77)  # junk in the unused direction
                if sel:
                    flags |= mb_fs_bit(r, s)
            m["flags"] = flags
    return w, h, pics, mbs, np.array(coefs, np.uint32)


def test_vectors_point_at_the_pixels_the_oracle_copies():
    w, h, pics, mbs, coefs = fullpel_batch()
    R.validate_batch(w, h, 1, 4, pics, mbs, coefs)
    luma = [f[0].astype(np.int32) for f in oracle_frames(Holder(w, h, 1, pics, mbs, coefs))]
    assert len(np.unique(luma[0])) > 64  # a reference with content
    mv, info, _ = R.motion_host(pics, mbs, coefs, w, h, 1)
    classes, signs = set(), set()
    for p, s, ref in ((1, 0, 0), (2, 1, 1), (3, 0, 0)):
        for my in range(h // 16):
            for mx in range(w // 16):
                fl = int(info[p, 0, my, mx])
                assert not fl & MB_INTRA and int(info[p, 1, my, mx]) == 0
                assert mv[p, 4 * (1 - s):4 * (1 - s) + 4, my, mx].tolist() == [0, 0, 0, 0]
                for r in range(2):
                    vx, vy = int(mv[p, 4 * s + 2 * r, my, mx]), int(mv[p, 4 * s + 2 * r + 1, my, mx])
                    assert vx % 2 == 0 and vy % 2 == 0
                    classes.add(("field", r, 1 if fl & mb_fs_bit(r, s) else 0) if fl & MB_FIELD_MC else "frame")
                    signs |= {("x", np.sign(vx)), ("y", np.sign(vy))}
                    y0, x0 = 16 * my, 16 * mx
                    rows = y0 + r + 2 * np.arange(8)
                    cur = luma[p][rows, x0:x0 + 16]
                    src = luma[ref][rows + vy // 2, x0 + vx // 2:x0 + vx // 2 + 16]
                    assert np.array_equal(cur, src), (p, mx, my, r, vx, vy)
    assert classes == {"frame", ("field", 0, 0), ("field", 0, 1), ("field", 1, 0), ("field", 1, 1)}
    assert signs >= {("x", -1), ("x", 1), ("y", -1), ("y", 1)}


# ---- model against the host twin --------------------------------------------------------------
@pytest.fixture(scope="module")
def parsed_streams():
    cache = {}

    def get(name):
        if name not in cache:
            e = next(m for m in MANIFEST if m["name"] == name)
            cache[name] = R.Parsed(read_stream(e), e["width"], e["height"], e["chroma_format"])
        return cache[name]
    return get


@pytest.fixture(scope="module")
def syntax_streams():
    return {S.name: S for S in DS.build_all()}


@pytest.mark.parametrize("entry", MANIFEST, ids=[e["name"] for e in MANIFEST])
def test_golden_streams_model_equals_twin(parsed_streams, entry):
    p = parsed_streams(entry["name"])
    mv, info, act = both(p.pics, p.mbs, p.coefs, p.width, p.height, p.chroma_format)
    assert int(act[:, 0].sum()) == len(p.coefs)  # every word is a word of some block
    assert np.array_equal(info[:, 3].astype(np.int64), act[:, 0].sum(axis=1))


@pytest.mark.parametrize("entry", SYNTAX_POSITIVE, ids=[e["name"] for e in SYNTAX_POSITIVE])
def test_directed_syntax_records_model_equals_twin(syntax_streams, entry):
    """Records from the independent writer's own expectation, pictures from the library's scan."""
    S = syntax_streams[entry["name"]]
    mbs, coefs = DS.records(S)
    with R.Scan(S.es, S.width, S.height, S.cf) as scan:
        pics = scan.pics.copy()
    both(pics, mbs.astype(R.MB_DTYPE), coefs, S.width, S.height, S.cf)


# ---- arguments --------------------------------------------------------------------------------
def test_motion_bytes():
    for cf in (1, 2, 3):
        assert R.motion_bytes(176, 144, cf, 5) == (5 * 8 * 99 * 2, 5 * 4 * 99 * 2, 5 * 2 * NB[cf] * 99 * 4)
    assert R.motion_bytes(16, 16, 1, 1) == (16, 8, 48)
    assert R.motion_bytes(4096, 2176, 3, 65535)[2] == 65535 * 2 * 12 * 256 * 136 * 4
    for n in (0, -1, 65536):
        with pytest.raises(_lib.Mp2vgError) as e:
            R.motion_bytes(176, 144, 1, n)
        assert e.value.status == -1
    with pytest.raises(_lib.Mp2vgError):
        R.motion_bytes(100, 64, 1, 1)
    cfg = _lib.make_config(176, 144, 1)
    assert _lib.lib().mp2vg_motion_bytes(ctypes.byref(cfg), 1, None) == -1
    assert _lib.lib().mp2vg_motion_bytes(None, 1, (ctypes.c_uint64 * 3)()) == -1


def test_order_repeats_and_reverse(parsed_streams):
    p = parsed_streams("ipb420_field")
    full = R.motion_host(p.pics, p.mbs, p.coefs, p.width, p.height, 1)
    for order in (list(range(p.npics))[::-1], [2, 2, 0, p.npics - 1, 2], [1], list(p.display)):
        got = both(p.pics, p.mbs, p.coefs, p.width, p.height, 1, order)
        for a, b in zip(got, full):
            assert np.array_equal(a, b[np.array(order)])


def raw_records(p, order, n=None, mv=True, info=True, act=True, pics=None, cfg=None):
    """(status, the three guarded destination arrays) of the C entry point itself."""
    L = _lib.lib()
    cfg = cfg or _lib.make_config(p.width, p.height, p.chroma_format)
    order = np.ascontiguousarray(order, np.int32)
    n = len(order) if n is None else n
    nbytes = R.motion_bytes(p.width, p.height, p.chroma_format, max(1, min(len(order), 8)))
    dst = [np.full(b, 0xA5, np.uint8) for b in nbytes]
    vp = ctypes.c_void_p
    pics = p.pics if pics is None else pics
    rc = L.mp2vg_motion_records(ctypes.byref(cfg), pics.ctypes.data_as(vp), len(pics), p.mbs.ctypes.data_as(vp),
                                len(p.mbs), p.coefs.ctypes.data_as(vp), len(p.coefs),
                                order.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), n,
                                dst[0].ctypes.data_as(vp) if mv else None, dst[1].ctypes.data_as(vp) if info else None,
                                dst[2].ctypes.data_as(vp) if act else None)
    return rc, dst


def test_rejected_arguments_leave_destinations_untouched(parsed_streams):
    p = parsed_streams("ipb420_qcif")
    clean = lambda dst: all((d == 0xA5).all() for d in dst)  # noqa: E731
    rc, dst = raw_records(p, [0, 1])
    assert rc == 0 and not any((d == 0xA5).all() for d in dst)
    rc, dst = raw_records(p, [0], mv=False, act=False)  # one output alone
    assert rc == 0 and clean([dst[0], dst[2]]) and not (dst[1] == 0xA5).all()
    for order in ([0, p.npics], [-1], [0, 1 << 30]):
        rc, dst = raw_records(p, order)
        assert rc == -1 and clean(dst) and b"order[" in _lib.lib().mp2vg_last_error()
    for n in (0, -3, 65536):
        rc, dst = raw_records(p, [0], n=n)
        assert rc == -1 and clean(dst)
    rc, dst = raw_records(p, [0], mv=False, info=False, act=False)
    assert rc == -1 and clean(dst)
    # a record batch the upload refuses is refused alike, with its reason
    bad = p.pics.copy()
    bad[1]["mb_first"] = len(p.mbs)
    rc, dst = raw_records(p, [0], pics=bad)
    assert rc == -1 and clean(dst) and b"picture MB range outside the batch" in _lib.lib().mp2vg_last_error()
    with pytest.raises(_lib.Mp2vgError) as e:
        R.validate_batch(p.width, p.height, 1, p.npics, bad, p.mbs, p.coefs)
    assert "picture MB range outside the batch" in str(e.value)
    mbs = p.mbs.copy()
    k = int(np.nonzero(mbs["ncoef"] > 0)[0][-1])
    mbs[k]["coef_off"] = len(p.coefs)
    with pytest.raises(_lib.Mp2vgError) as e:
        R.motion_host(p.pics, mbs, p.coefs, p.width, p.height, 1)
    assert e.value.status == -1 and "coefficient range outside the batch" in str(e.value)
    rc, dst = raw_records(p, [0], cfg=_lib.make_config(192, 144, 1))
    assert rc == -1 and clean(dst)


# ---- reference_pictures and dist --------------------------------------------------------------
def expected_references(p):
    """From Parsed alone: slot = decode index, so a reference slot names its picture."""
    ref = np.full((p.npics, 2), -1, np.int64)
    for i in range(p.npics):
        for s, name in enumerate(("fwd_slot", "bwd_slot")):
            slot = int(p.pics[i][name])
            assert slot < i
            ref[i, s] = slot
    pos = {int(d): k for k, d in enumerate(p.display)}
    dist = np.array([[pos[int(ref[d, s])] - k if ref[d, s] >= 0 else 0 for s in range(2)]
                     for k, d in enumerate(p.display)], np.int32)
    return ref.astype(np.int32), dist


@pytest.mark.parametrize("name", ["ipb420_qcif_openb", "two_gops"])
def test_reference_pictures_and_dist(parsed_streams, name):
    if name == "two_gops":
        es = R.generate_es(width=64, height=48, chroma_format=1, n_gops=2, gop_n=7, gop_m=3, seed=5)
        p = R.Parsed(es, 64, 48, 1)
    else:
        p = parsed_streams(name)
    assert [int(s) for s in p.pics["dst_slot"]] == list(range(p.npics))
    ref, dist = expected_references(p)
    assert np.array_equal(R.reference_pictures(p.pics), ref)
    got = R.reference_distances(p.pics, p.display)
    assert got.dtype == np.int32 and np.array_equal(got, dist)
    types = p.pics["picture_coding_type"][p.display]
    assert (dist[types == 3, 0] < 0).any() and (dist[types == 3, 1] > 0).all()  # B: past and future anchors
    assert (dist[types == 2, 0] < 0).all() and (dist[:, 0] <= 0).all()
    # slots reused by a later batch: the last earlier writer counts
    pics = p.pics.copy()
    pics["dst_slot"] %= 3
    pics["fwd_slot"] = np.where(pics["fwd_slot"] >= 0, pics["fwd_slot"] % 3, -1)
    pics["bwd_slot"] = -1
    want = [[max([j for j in range(i) if pics[j]["dst_slot"] == pics[i]["fwd_slot"]], default=-1), -1]
            for i in range(p.npics)]
    assert R.reference_pictures(pics).tolist() == want


# ---- the twin under the sanitizers ------------------------------------------------------------
@pytest.fixture(scope="module")
def motion_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("san_motion") / "motion_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I", CSRC,
           "-I", os.path.join(REPO, "include"), os.path.join(REPO, "tests", "fuzz", "motion_check.cpp"),
           os.path.join(CSRC, "motion.cpp"), os.path.join(CSRC, "parse.cpp"), os.path.join(CSRC, "tables.cpp"),
           os.path.join(CSRC, "runtime.cpp"), "-o", exe, "-pthread", "-L/opt/rocm/lib", "-lamdhip64",
           "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        pytest.fail(f"sanitizer build failed:\n{r.stderr[-2000:]}")
    return exe


def test_host_twin_under_asan_ubsan(motion_check):
    args = []
    for name in ("ipb420_field", "w80_422_field", "intra444_dense"):
        e = next(m for m in MANIFEST if m["name"] == name)
        args += [os.path.join(GOLDEN, "streams", e["file"]), str(e["width"]), str(e["height"]), str(e["chroma_format"])]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([motion_check] + args, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["streams"] == 3 and res["exports"] > 0 and res["rejected"] > 0
