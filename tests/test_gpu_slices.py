"""GPU: MP2VG_PARSE_SLICES on the device parse (parse.hip, parse_dev.cpp: the count and emit
kernels write records [x0, x1) of a row, the row kernel applies the cover rule), the reconstruct,
the exports and the drop-in decoder, against the host emitter (held to the twin streams by
test_slices_cpu.py) and the MD5s the compiled reference computed for the one-slice-per-row twins
(tests/golden/slices/).  Every comparison is exact.

Every stream sent to the device has gone through the CPU twin first (which asserts sp_iter_bound
and returns a status), and once a call here returns MP2VG_E_HIP the rest of the file is skipped."""
import hashlib

import numpy as np
import pytest

import parse_mutants as PM
import slices_streams as SL
from helpers import oracle_frames
from tiny_mp2v_dec_amd import _lib
from tiny_mp2v_dec_amd import records as R
from tiny_mp2v_dec_amd.decoder import decoder_config_t, mp2v_decoder_c

pytestmark = pytest.mark.gpu

MANIFEST = SL.load_manifest()
TWINS = [e for e in MANIFEST if e["md5"] is not None]
NEGATIVE = [e for e in MANIFEST if e["md5"] is None]
BY_NAME = {e["name"]: e for e in MANIFEST}
E_HIP = -3
_HIP = {"failed": False}


@pytest.fixture(scope="module", autouse=True)
def _torch_runtime_first():
    """torch brings its own HIP runtime: it has to open the device before the library's does"""
    import torch
    torch.zeros(1, device="cuda")


@pytest.fixture(scope="module", autouse=True)
def _watch_for_hip_errors():
    real = R.check

    def check(status, what):
        if status == E_HIP:
            _HIP["failed"] = True
        return real(status, what)

    mp = pytest.MonkeyPatch()
    mp.setattr(R, "check", check)
    yield
    mp.undo()


@pytest.fixture(autouse=True)
def _nothing_more_after_a_hip_error(_watch_for_hip_errors):
    if _HIP["failed"]:
        pytest.skip("an earlier call in this file returned MP2VG_E_HIP: nothing more is launched on the device")


@pytest.fixture(scope="module")
def contexts():
    """one DeviceContext per geometry, kept for the module"""
    by_geom = {}

    def get(w, h, cf):
        if (w, h, cf) not in by_geom:
            by_geom[(w, h, cf)] = R.DeviceContext(w, h, cf, slots=12)
        return by_geom[(w, h, cf)]

    yield get
    for c in by_geom.values():
        c.close()


def geom(e):
    return e["width"], e["height"], e["chroma_format"]


def _upload_and_compare(ctx, es, w, h, cf, p, **flags):
    """the twin first, then upload_es: the device's records are the host emitter's p's"""
    scan = R.Scan(es, w, h, cf, **flags)
    rec = scan.parse_host()
    assert PM.same_records(p, rec)
    ctx.upload_es(scan)
    dev = ctx.download_records()
    assert dev[0].tobytes() == p.mbs.tobytes(), "macroblock records differ"
    assert dev[1].tobytes() == p.coefs.tobytes(), "coefficient words differ"
    return scan


def _md5s(ctx, display):
    from helpers import yuv_md5
    return [yuv_md5(ctx.download(int(d))) for d in display]


def _refused_alike(ctx, es, w, h, cf, **flags):
    """(status, message) of upload_es, which must be the twin's"""
    scan = R.Scan(es, w, h, cf, **flags)
    with pytest.raises(_lib.Mp2vgError) as tw:
        scan.parse_host()
    with pytest.raises(_lib.Mp2vgError) as ei:
        ctx.upload_es(scan)
    assert (ei.value.status, PM.detail(str(ei.value))) == (tw.value.status, PM.detail(str(tw.value)))
    return ei.value.status, PM.detail(str(ei.value))


# ---- 1: every fixture through upload_es (the 560 x 16 and 16384 x 16 streams among them) -------------------
@pytest.mark.parametrize("e", TWINS, ids=[e["name"] for e in TWINS])
def test_device_parse_under_the_flag_gives_the_emitters_records_and_the_reference_frames(contexts, e):
    es, (w, h, cf) = SL.read(e["ms"]), geom(e)
    p = R.Parsed(es, w, h, cf, threads=1, slices=True)
    ctx = contexts(w, h, cf)
    scan = _upload_and_compare(ctx, es, w, h, cf, p, slices=True)
    assert scan.nslices == e["slices"] and scan.pics.tobytes() == p.pics.tobytes()
    ctx.decode()
    ctx.synchronize()
    got = [ctx.download(k) for k in range(p.npics)]
    exp = oracle_frames(p)
    for k in range(p.npics):
        for plane in range(3):
            assert np.array_equal(got[k][plane], exp[k][plane]), (k, plane)
    assert _md5s(ctx, scan.display) == e["md5"]
    # the other two flags on top change nothing on a clean stream
    _upload_and_compare(ctx, es, w, h, cf, p, slices=True, conceal=True, standard=True)
    assert len(ctx.last_damage()) == 0


# ---- 2: more table entries than the scan kernel has lanes -----------------------------------------------------
def test_1089_slices_whole_and_in_ranges_that_end_inside_a_wave(contexts):
    """176 x 144, a slice per macroblock, eleven pictures: 1,089 entries, so each of the scan
    kernel's 1,024 lanes sums a run of two, and rows of eleven entries straddle the waves of the
    count, row and emit kernels.  Sub-ranges of 1, 3, 4 and 3 pictures hold 99, 297, 396 and 297
    entries: none is a multiple of 64."""
    e = BY_NAME[SL.MANY]
    es, (w, h, cf) = SL.read(e["ms"]), geom(e)
    p = R.Parsed(es, w, h, cf, threads=1, slices=True)
    assert p.npics == 11 and e["slices"] == 1089 > 1024
    ctx = contexts(w, h, cf)
    scan = _upload_and_compare(ctx, es, w, h, cf, p, slices=True)
    ctx.decode()
    ctx.synchronize()
    assert _md5s(ctx, p.display) == e["md5"]
    for first, n in ((0, 1), (1, 3), (4, 4), (8, 3)):
        want = PM.range_of_whole(p, first, n)
        ctx.upload_es(scan, first, n)
        dev = ctx.download_records()
        assert dev[0].tobytes() == want[0].tobytes() and dev[1].tobytes() == want[1].tobytes(), first


# ---- 3: concealment and the negative streams ------------------------------------------------------------------
@pytest.fixture(scope="module")
def conceal_cases():
    e = BY_NAME[SL.CONCEAL_STREAM]
    return e, {c[0]: c for c in SL.conceal_cases(SL.read(e["ms"]), *geom(e))}


@pytest.mark.parametrize("name", ["damaged_I", "damaged_P", "damaged_B", "middle_deleted", "row_deleted"])
def test_a_broken_row_is_replaced_on_the_device_as_on_the_host(contexts, conceal_cases, name):
    e, cases = conceal_cases
    _, es, damaged, missing, want_damage = cases[name]
    w, h, cf = geom(e)
    ctx = contexts(w, h, cf)
    p = R.Parsed(es, w, h, cf, threads=1, slices=True, conceal=True)
    _upload_and_compare(ctx, es, w, h, cf, p, slices=True, conceal=True)
    dmg = ctx.last_damage()
    assert dmg.tobytes() == p.damage.tobytes() and len(dmg) == 1
    assert (int(dmg[0]["pic"]), int(dmg[0]["mb_row"]), int(dmg[0]["byte_off"])) == want_damage[0][:2] + want_damage[0][4:]
    ctx.decode()
    ctx.synchronize()
    exp = oracle_frames(p)
    for k in range(p.npics):
        got = ctx.download(k)
        for plane in range(3):
            assert np.array_equal(got[plane], exp[k][plane]), (k, plane)
    # without CONCEAL the device refuses as the twin does, and the context stays usable
    if missing:  # (a row without any slice: the scan itself refuses, nothing reaches the device)
        with pytest.raises(_lib.Mp2vgError) as ei:
            R.Scan(es, w, h, cf, slices=True)
        assert ei.value.status == -2 and want_damage[0][3] in str(ei.value)
        return
    st, msg = _refused_alike(ctx, es, w, h, cf, slices=True)
    assert st != 0 and want_damage[0][3] in msg
    _upload_and_compare(ctx, es, w, h, cf, p, slices=True, conceal=True)


@pytest.mark.parametrize("e", NEGATIVE, ids=[e["name"] for e in NEGATIVE])
def test_negative_streams_on_the_device(contexts, e):
    es, (w, h, cf) = SL.read(e["ms"]), geom(e)
    ctx = contexts(w, h, cf)
    off = PM.slice_starts(es)[e["blamed_slice"]]
    want = (e["status"], f"picture 0 slice @{off}: {e['reason']}")
    if e["reason"] == SL.TWO:  # the scan itself refuses, with and without CONCEAL: nothing reaches the device
        for flags in (dict(slices=True), dict(slices=True, conceal=True)):
            with pytest.raises(_lib.Mp2vgError) as ei:
                R.Scan(es, w, h, cf, **flags)
            assert (ei.value.status, PM.detail(str(ei.value))) == want
        return
    assert _refused_alike(ctx, es, w, h, cf, slices=True) == want
    p = R.Parsed(es, w, h, cf, threads=1, slices=True, conceal=True)
    _upload_and_compare(ctx, es, w, h, cf, p, slices=True, conceal=True)  # ... and the context is still usable
    dmg = ctx.last_damage()
    assert dmg.tobytes() == p.damage.tobytes() and len(dmg) == 1
    assert (int(dmg[0]["status"]), R.damage_reason(dmg[0]["reason"]), int(dmg[0]["byte_off"])) == (e["status"], e["reason"], off)


# ---- 4: the flag clear ------------------------------------------------------------------------------------------
def test_flag_clear_is_refused_on_the_device_as_the_twin_refuses(contexts):
    """a stream whose rows the scan lets through without the flag (one slice per row) but whose
    slices start after column 0 or end short: the kernels refuse as the twin does.  The ms fixtures
    themselves stop in the flag-clear scan ("two slices in one macroblock row")."""
    for name, reason in (("neg_gap_start", "slice does not start at column 0"),
                         ("neg_gap_end", "two slices in one macroblock row")):
        e = BY_NAME[name]
        es, (w, h, cf) = SL.read(e["ms"]), geom(e)
        ctx = contexts(w, h, cf)
        if "two slices" in reason:
            with pytest.raises(_lib.Mp2vgError) as ei:
                R.Scan(es, w, h, cf)
            assert ei.value.status == -2 and reason in str(ei.value)
        else:
            st, msg = _refused_alike(ctx, es, w, h, cf)
            assert st == -2 and msg.endswith(reason)
    for e in TWINS:
        with pytest.raises(_lib.Mp2vgError) as ei:
            R.Scan(SL.read(e["ms"]), *geom(e))
        assert ei.value.status == SL.CLEAR_STATUS and SL.CLEAR_REASONS[1] in str(ei.value)
    # a short first slice alone (the second slice of row 1 cut off): "does not cover the whole row"
    e = BY_NAME["neg_gap_end"]
    es, (w, h, cf) = SL.read(e["ms"]), geom(e)
    last = PM.slice_starts(es)[2]
    cut = es[:last] + es[es.index(b"\x00\x00\x01\xb7", last):]
    st, msg = _refused_alike(contexts(w, h, cf), cut, w, h, cf)
    assert st == -2 and msg.endswith(SL.CLEAR_REASONS[0])


# ---- 5: the drop-in and the one-call wrappers ---------------------------------------------------------------------
@pytest.mark.parametrize("device_parse", [True, False], ids=["device_parse", "host_parse"])
def test_through_the_dropin(device_parse):
    e = BY_NAME[SL.MANY]  # eleven pictures: the drop-in feeds them in chunks
    es, (w, h, cf) = SL.read(e["ms"]), geom(e)
    R.Scan(es, w, h, cf, slices=True).parse_host()  # the twin first
    got = []
    dec = mp2v_decoder_c(decoder_config_t(w, h, cf, device_parse=device_parse, slices=True),
                         lambda f: got.append(hashlib.md5(f.yuv_bytes()).hexdigest()))
    try:
        assert dec.decode(es) and got == e["md5"]
        assert dec.damage_count() == 0
    finally:
        dec.close()
    dec = mp2v_decoder_c(decoder_config_t(w, h, cf, device_parse=device_parse), lambda f: None)
    try:
        with pytest.raises(_lib.Mp2vgError) as ei:
            dec.decode(es)
        assert ei.value.status == SL.CLEAR_STATUS and any(r in str(ei.value) for r in SL.CLEAR_REASONS)
    finally:
        dec.close()


def test_decode_rgb_and_motion_take_the_flag():
    e = BY_NAME["sl_422"]
    w, h, cf = geom(e)
    ms, ref = SL.read(e["ms"]), SL.read(e["ref"])
    R.Scan(ms, w, h, cf, slices=True).parse_host()  # the twin first
    with pytest.raises(_lib.Mp2vgError):
        R.decode_rgb(ms, w, h, cf)
    want = R.decode_rgb(ref, w, h, cf)
    assert tuple(want.shape) == (e["frames"], 3, h, w)
    for device_parse in (False, True):
        assert bool((R.decode_rgb(ms, w, h, cf, device_parse=device_parse, slices=True) == want).all())
    for parse in ("device", "host"):
        a, b = R.decode_motion(ms, w, h, cf, parse=parse, slices=True), R.decode_motion(ref, w, h, cf, parse=parse)
        assert sorted(a) == sorted(b)
        for k in a:
            x, y = a[k], b[k]
            assert bool((x == y).all()) if hasattr(x, "shape") else x == y, k
