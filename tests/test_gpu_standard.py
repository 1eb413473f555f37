"""GPU: MP2VG_PARSE_STANDARD on the device parse (parse.hip, parse_dev.cpp), the reconstruct, the
exports and the drop-in decoder, against the host emitter (held to the twin streams by
test_standard_cpu.py) and the MD5s the compiled reference computed for the twins
(tests/golden/standard/).  Every comparison is exact.

Every stream sent to the device has gone through the CPU twin first (which asserts sp_iter_bound
and returns a status), and once a call here returns MP2VG_E_HIP the rest of the file is skipped."""
import hashlib

import numpy as np
import pytest

import conceal_streams as CS
import parse_mutants as PM
import standard_streams as SS
from tiny_mp2v_dec_amd import _lib
from tiny_mp2v_dec_amd import records as R
from tiny_mp2v_dec_amd.decoder import decoder_config_t, mp2v_decoder_c

pytestmark = pytest.mark.gpu

MANIFEST = SS.load_manifest()
TWINS = [e for e in MANIFEST if e["md5"] is not None]
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
            by_geom[(w, h, cf)] = R.DeviceContext(w, h, cf, slots=40)
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


# ---- 1: every fixture through upload_es -------------------------------------------------------------------
@pytest.mark.parametrize("e", TWINS, ids=[e["name"] for e in TWINS])
def test_device_parse_under_the_flag_gives_the_emitters_records_and_the_reference_frames(contexts, e):
    es, (w, h, cf) = SS.read(e, "std"), geom(e)
    p = R.Parsed(es, w, h, cf, threads=1, standard=True)
    ctx = contexts(w, h, cf)
    scan = _upload_and_compare(ctx, es, w, h, cf, p, standard=True)
    assert scan.pics.tobytes() == p.pics.tobytes()
    ctx.decode()
    ctx.synchronize()
    assert _md5s(ctx, scan.display) == e["md5"]


# ---- 2: 40 pictures that alternate the two tables ------------------------------------------------------------
def test_alternating_formats_through_upload_es(contexts):
    """80 slices: the first wave's 64 lanes mix B.14 and B.15 pictures, the second holds 16; an
    extension load on picture 3 and a second sequence header at picture 20.  The whole stream in
    one upload, then as the ranges the drop-in would feed (16, 16, 8)."""
    e = BY_NAME["ivf_alternating"]
    es, (w, h, cf) = SS.read(e, "std"), geom(e)
    p = R.Parsed(es, w, h, cf, threads=1, standard=True)
    assert p.npics == 40 and len(p.mbs) == 160
    assert not np.array_equal(p.pics["W"][2], p.pics["W"][3]) and not np.array_equal(p.pics["W"][19], p.pics["W"][20])
    ctx = contexts(w, h, cf)
    scan = _upload_and_compare(ctx, es, w, h, cf, p, standard=True)
    assert scan.nslices == 80
    ctx.decode()
    ctx.synchronize()
    assert _md5s(ctx, p.display) == e["md5"]
    for first, n in ((0, 16), (16, 16), (32, 8)):
        want = PM.range_of_whole(p, first, n)
        ctx.upload_es(scan, first, n)
        dev = ctx.download_records()
        assert dev[0].tobytes() == want[0].tobytes() and dev[1].tobytes() == want[1].tobytes(), first


@pytest.mark.parametrize("device_parse", [True, False], ids=["device_parse", "host_parse"])
def test_alternating_formats_through_the_dropin(device_parse):
    """the drop-in feeds 16-picture chunks: the matrix state (picture 3's load, picture 20's reset)
    crosses their borders"""
    e = BY_NAME["ivf_alternating"]
    es, (w, h, cf) = SS.read(e, "std"), geom(e)
    R.Scan(es, w, h, cf, standard=True).parse_host()  # the twin first
    got = []
    dec = mp2v_decoder_c(decoder_config_t(w, h, cf, device_parse=device_parse, standard=True),
                         lambda f: got.append(hashlib.md5(f.yuv_bytes()).hexdigest()))
    try:
        assert dec.decode(es) and got == e["md5"]
        assert dec.damage_count() == 0
    finally:
        dec.close()
    # without the flag decode() fails as it does today
    dec = mp2v_decoder_c(decoder_config_t(w, h, cf, device_parse=device_parse), lambda f: None)
    try:
        with pytest.raises(_lib.Mp2vgError) as ei:
            dec.decode(es)
        assert ei.value.status == SS.CLEAR_STATUS and SS.CLEAR_REASON in str(ei.value)
    finally:
        dec.close()


# ---- 3: the flag clear ------------------------------------------------------------------------------------------
def test_flag_clear_rejects_on_the_device_as_the_twin_does_and_the_context_stays_usable(contexts):
    """S' with full extensions gets past the scan; the kernels, like the twin, refuse its first
    intra macroblock of a format-0 picture.  The next upload on the context is unharmed."""
    S = SS.FORMAT0_BUILDERS[0]("std", full_ext=True)
    w, h, cf = S.width, S.height, S.cf
    ctx = contexts(w, h, cf)
    scan = R.Scan(S.es, w, h, cf)
    with pytest.raises(_lib.Mp2vgError) as tw:
        scan.parse_host()
    with pytest.raises(_lib.Mp2vgError) as ei:
        ctx.upload_es(scan)
    assert (ei.value.status, PM.detail(str(ei.value))) == (tw.value.status, PM.detail(str(tw.value)))
    assert ei.value.status == -2 and SS.CLEAR_IVF0_REASON in str(ei.value)
    # every S' as it is stored stops in the scan, so nothing reaches the device
    e = BY_NAME["ivf0_420"]
    with pytest.raises(_lib.Mp2vgError) as ei:
        R.Scan(SS.read(e, "std"), *geom(e))
    assert ei.value.status == SS.CLEAR_STATUS and SS.CLEAR_REASON in str(ei.value)
    p = R.Parsed(S.es, w, h, cf, threads=1, standard=True)
    _upload_and_compare(ctx, S.es, w, h, cf, p, standard=True)
    ctx.decode()
    ctx.synchronize()
    assert _md5s(ctx, p.display) == e["md5"]


def test_refused_422_stream_through_the_scan_and_the_dropin():
    e = BY_NAME["neg_422_chroma_differs"]
    es, (w, h, cf) = SS.read(e, "std"), geom(e)
    with pytest.raises(_lib.Mp2vgError) as ei:
        R.Scan(es, w, h, cf, standard=True)
    assert ei.value.status == -2 and PM.detail(str(ei.value)).startswith(e["reason"])
    for device_parse in (False, True):
        dec = mp2v_decoder_c(decoder_config_t(w, h, cf, device_parse=device_parse, standard=True), lambda f: None)
        try:
            with pytest.raises(_lib.Mp2vgError) as ei:
                dec.decode(es)
            assert ei.value.status == -2 and PM.detail(str(ei.value)).startswith(e["reason"])
        finally:
            dec.close()


# ---- 4: a lost slice in S' and in S ------------------------------------------------------------------------------
@pytest.mark.parametrize("name,pic,row", [("ivf0_420", 1, 1), ("ivf0_422", 2, 0)])
def test_a_lost_slice_is_concealed_alike_in_both_twins(contexts, name, pic, row):
    """the same slice removed from S' (CONCEAL | STANDARD) and from S (CONCEAL): one damaged row
    each, at the same place for the same reason, and equal frames: the other rows of the format-0
    pictures are decoded, not greyed"""
    e = BY_NAME[name]
    w, h, cf = geom(e)
    ctx = contexts(w, h, cf)
    frames, damage = [], []
    for form, flags in (("std", dict(conceal=True, standard=True)), ("ref", dict(conceal=True))):
        es = SS.read(e, form)
        cut = CS.delete_slices(es, [j for j, t in enumerate(CS.slice_table(es)) if t[:2] == (pic, row)])
        assert len(cut) < len(es)
        p = R.Parsed(cut, w, h, cf, threads=1, **flags)
        _upload_and_compare(ctx, cut, w, h, cf, p, **flags)
        dmg = ctx.last_damage()
        assert dmg.tobytes() == p.damage.tobytes()
        damage.append([(int(d["pic"]), int(d["mb_row"]), int(d["status"]), int(d["reason"])) for d in dmg])
        ctx.decode()
        ctx.synchronize()
        frames.append(_md5s(ctx, p.display))
    assert damage[0] == damage[1] and [d[:2] for d in damage[0]] == [(pic, row)]
    assert frames[0] == frames[1]
    shown = list(R.Parsed(SS.read(e, "ref"), w, h, cf).display)
    same = [a == b for a, b in zip(frames[0], e["md5"])]
    assert not same[shown.index(pic)] and same[shown.index(0)]  # the damaged picture differs, the I picture does not


# ---- 5: the one-call wrappers ---------------------------------------------------------------------------------
def test_decode_rgb_motion_and_residual_take_the_flag():
    e = BY_NAME["ivf0_422"]
    w, h, cf = geom(e)
    std, ref = SS.read(e, "std"), SS.read(e, "ref")
    R.Scan(std, w, h, cf, standard=True).parse_host()  # the twin first
    with pytest.raises(_lib.Mp2vgError):
        R.decode_rgb(std, w, h, cf)
    want = R.decode_rgb(ref, w, h, cf)
    assert tuple(want.shape) == (e["frames"], 3, h, w)
    for device_parse in (False, True):
        assert bool((R.decode_rgb(std, w, h, cf, device_parse=device_parse, standard=True) == want).all())
    t = R.decode_tensor(std, w, h, cf, (w, h), dtype="uint8", device_parse=True, standard=True)
    assert bool((t == R.decode_tensor(ref, w, h, cf, (w, h), dtype="uint8")).all())
    for parse in ("device", "host"):
        a, b = R.decode_motion(std, w, h, cf, parse=parse, standard=True), R.decode_motion(ref, w, h, cf, parse=parse)
        assert sorted(a) == sorted(b)
        for k in a:
            x, y = a[k], b[k]
            assert bool((x == y).all()) if hasattr(x, "shape") else x == y, k
        a, b = R.decode_residual(std, w, h, cf, parse=parse, standard=True), R.decode_residual(ref, w, h, cf, parse=parse)
        assert sorted(a) == sorted(b)
        for k in a:
            x, y = a[k], b[k]
            assert bool((x == y).all()) if hasattr(x, "shape") else x == y, k
    r = R.probe(std)
    assert (r["width"], r["chroma_format"], r["display_height"]) == (w, cf, h)
