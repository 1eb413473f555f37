"""GPU: concealment (MP2VG_PARSE_CONCEAL) on the device parse (parse.hip, parse_dev.cpp), the
reconstruct of concealed batches, the exports and the drop-in decoder, against the host emitter
(itself held to conceal_model.py by test_conceal_cpu.py), the C oracle and the repaired streams
the compiled reference decoded.  Every comparison is exact.

The mutants run on the device only what the device-parse tests already run on them: a damaged
slice ends in a status, not a fault.  Every stream sent to the device has gone through the twin
first (which asserts sp_iter_bound and returns a status), and once a call here returns
MP2VG_E_HIP the rest of the file is skipped."""
import hashlib

import numpy as np
import pytest

import conceal_model as CM
import conceal_streams as CS
import parse_mutants as PM
from helpers import oracle_frames, yuv_md5
from tiny_mp2v_dec_amd import _lib
from tiny_mp2v_dec_amd import records as R
from tiny_mp2v_dec_amd.decoder import decoder_config_t, mp2v_decoder_c

pytestmark = pytest.mark.gpu

FIX = PM.load_fixture()
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


class Contexts:
    """one DeviceContext per geometry, kept for the module: damaged and clean uploads follow each
    other on the same context, as they do in use"""

    def __init__(self):
        self.by_geom = {}

    def get(self, w, h, cf):
        key = (w, h, cf)
        if key not in self.by_geom:
            self.by_geom[key] = R.DeviceContext(w, h, cf, slots=3073 if (w, h) == (16, 16) else 32)
        return self.by_geom[key]

    def close(self):
        for c in self.by_geom.values():
            c.close()


@pytest.fixture(scope="module")
def contexts():
    c = Contexts()
    yield c
    c.close()


def _same_damage(a, b):
    return a.dtype == b.dtype == _lib.DAMAGE_DTYPE and a.tobytes() == b.tobytes()


def _frames_equal(got, want):
    assert len(got) == len(want)
    for d, (a, b) in enumerate(zip(got, want)):
        for k in range(3):
            assert np.array_equal(a[k], b[k]), (d, k)


def _host(es, w, h, cf):
    return R.Parsed(es, w, h, cf, threads=1, conceal=True)


def _device_parity(ctx, es, w, h, cf, decode=True):
    """The stream under the flag through the twin, then through upload_es on ctx: the device's
    records and damage list are the host emitter's; decoded from host records and from the device
    parse, the frames are the oracle's on the emitter's records.  Returns the emitter's Parsed."""
    p = _host(es, w, h, cf)
    scan = R.Scan(es, w, h, cf, conceal=True)
    rec = scan.parse_host()  # the twin first
    assert PM.same_records(p, rec)
    ctx.upload_es(scan)
    dev = ctx.download_records()
    assert dev[0].tobytes() == p.mbs.tobytes(), "macroblock records differ"
    assert dev[1].tobytes() == p.coefs.tobytes(), "coefficient words differ"
    assert _same_damage(ctx.last_damage(), p.damage)
    if decode:
        want = oracle_frames(p)
        ctx.decode()
        ctx.synchronize()
        _frames_equal([ctx.download(q) for q in range(p.npics)], want)
        ctx.upload(p.pics, p.mbs, p.coefs)
        ctx.decode()
        ctx.synchronize()
        _frames_equal([ctx.download(q) for q in range(p.npics)], want)
    return p


# ---- record and decode parity ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bases():
    return [(es, w, h, cf) for es, w, h, cf in PM.base_streams()]


@pytest.mark.parametrize("reason", PM.SLICE_REASONS)
def test_rejected_fixture_mutants_are_concealed_as_the_host_emitter_does(contexts, bases, reason):
    for si, pos, val, status, det, _ in FIX["rejected"][reason]:
        es, w, h, cf = bases[si]
        p = _device_parity(contexts.get(w, h, cf), PM.mutate(es, pos, val), w, h, cf)
        assert len(p.damage) == 1 and int(p.damage["status"][0]) == status
        assert det.endswith(": " + R.damage_reason(p.damage["reason"][0]))


def test_intra_vlc_format_zero_stream(contexts):
    es, w, h, cf = PM.vlc0_stream()
    p = _device_parity(contexts.get(w, h, cf), es, w, h, cf)
    assert len(p.damage) == p.npics * (h // 16)


def test_multi_fault_stream(contexts):
    bad, es, w, h, cf, _ = CS.damaged_stream(CS.MULTI, CS.MULTI_DAMAGE)
    p = _device_parity(contexts.get(w, h, cf), bad, w, h, cf)
    pics, mbs, coefs, order = CM.conceal(R.Parsed(es, w, h, cf), CS.MULTI_DAMAGE)
    assert (p.pics.tobytes(), p.mbs.tobytes(), p.coefs.tobytes()) == (pics.tobytes(), mbs.tobytes(), coefs.tobytes())
    assert [(int(d["pic"]), int(d["mb_row"])) for d in p.damage] == order


@pytest.mark.parametrize("rows", [[(4, 0)], [(4, 2)], [(0, 0), (0, 2)], [(6, 1), (11, 2)]], ids=str)
def test_missing_slices(contexts, rows):
    es = R.generate_es(**CS.MULTI)
    w, h, cf = PM.geom(CS.MULTI)
    cut = CS.delete_slices(es, [j for j, t in enumerate(CS.slice_table(es)) if t[:2] in rows])
    p = _device_parity(contexts.get(w, h, cf), cut, w, h, cf)
    assert all(R.damage_reason(r) == CS.UNCOVERED for r in p.damage["reason"]) and len(p.damage) == len(rows)


@pytest.mark.parametrize("name", list(CS.CORNERS))
def test_geometry_corners(name):
    bad, _, w, h, cf, _ = CS.damaged_stream(CS.CORNERS[name], CS.CORNER_DAMAGE)
    with R.DeviceContext(w, h, cf, slots=4) as ctx:
        p = _device_parity(ctx, bad, w, h, cf)
    assert len(p.damage) == 2 and p.mbs["ncoef"][0] == CM.NBLOCKS[cf]


@pytest.mark.parametrize("e", CS.load_fixtures(), ids=lambda e: e["name"])
def test_concealed_stream_decodes_to_the_reference_frames_of_the_repaired_stream(contexts, e):
    w, h, cf = e["width"], e["height"], e["chroma_format"]
    ctx = contexts.get(w, h, cf)
    p = _device_parity(ctx, e["damaged_es"], w, h, cf)  # leaves the host records' decode in the slots
    assert [yuv_md5(ctx.download(int(d))) for d in p.display] == e["md5"]
    scan = R.Scan(e["damaged_es"], w, h, cf, conceal=True)
    ctx.upload_es(scan)
    ctx.decode()
    ctx.synchronize()
    assert [yuv_md5(ctx.download(int(d))) for d in scan.display] == e["md5"]


# ---- the scan kernel's lanes with several slices ------------------------------------------------------------
# n slices over 1024 lanes of ceil(n / 1024) each.  1023: one per lane.  1025: two (lane 150 holds 300
# and 301, lane 200 holds 400 and 401; 511 | 512, 513 straddle lanes 255 and 256).  3073: four (lane
# 100 holds 400..403; 2047 | 2048, 2049 straddle lanes 511 and 512; 3072 is alone in lane 768).
LANES = [(1023, (0, 500, 501, 502, 1022)), (1025, (300, 401, 511, 512, 513, 1024)),
         (3073, (0, 400, 403, 2047, 2048, 2049, 3072))]


@pytest.mark.parametrize("n,ks", LANES, ids=[str(n) for n, _ in LANES])
def test_scan_kernel_counts_damage_in_lanes_with_several_slices(contexts, n, ks):
    """one slice per picture, every picture an I picture: slice 0 turns grey, the others are
    re-typed and copy the picture before them.  The words are where the host emitter puts them only
    if base[] takes the replacement rows' counts, the damage list only if the count and every
    result come back, and the decode only if the per-picture usage bits carry the new forward read."""
    es = PM.one_slice_pictures(n, 7000 + n)
    bad, why = PM.stream_with_failing_slices(es, 16, 16, 1, ks)
    p = _device_parity(contexts.get(16, 16, 1), bad, 16, 16, 1)
    assert [int(d["pic"]) for d in p.damage] == sorted(ks)
    assert [R.damage_reason(r) for r in p.damage["reason"]] == [why[k] for k in sorted(ks)]
    types = np.ones(n, np.int32)
    types[[k for k in ks if k]] = 2
    assert np.array_equal(p.pics["picture_coding_type"], types)


# ---- sub-ranges -------------------------------------------------------------------------------------------------
def test_damage_in_the_first_and_the_last_slice_of_an_uploaded_range(contexts):
    """the second GOP of the multi-fault stream as a range of its own: its I picture is damaged
    (first slice of the range) and re-typed, and reads picture 3, decoded by the upload before;
    the last slice of the range is damaged too; pic is relative to the range"""
    first, n = 6, 6
    bad, es, w, h, cf, _ = CS.damaged_stream(CS.MULTI, [(6, 0), (11, 2)])
    p = _host(bad, w, h, cf)
    scan = R.Scan(bad, w, h, cf, conceal=True)
    want = PM.range_of_whole(p, first, n)
    rec = scan.parse_host(first, n)
    assert rec[0].tobytes() == want[0].tobytes() and rec[1].tobytes() == want[1].tobytes()
    ctx = contexts.get(w, h, cf)
    ctx.upload_es(scan, 0, first)
    assert len(ctx.last_damage()) == 0
    ctx.decode()
    ctx.upload_es(scan, first, n)
    dev = ctx.download_records()
    assert dev[0].tobytes() == want[0].tobytes() and dev[1].tobytes() == want[1].tobytes()
    dmg = ctx.last_damage()
    assert [(int(d["pic"]), int(d["mb_row"])) for d in dmg] == [(0, 0), (5, 2)]
    assert np.array_equal(dmg["byte_off"], p.damage["byte_off"]) and np.array_equal(dmg["reason"], p.damage["reason"])
    ctx.decode()
    ctx.synchronize()
    _frames_equal([ctx.download(q) for q in range(p.npics)], oracle_frames(p))


@pytest.mark.parametrize("case", PM.SUBRANGE_CASES, ids=[c[0] for c in PM.SUBRANGE_CASES])
def test_sub_range_cases_first_and_last_slice(contexts, case):
    from conftest import load_manifest, read_stream
    name, first, n, _ = case
    e = {m["name"]: m for m in load_manifest()}[name]
    es, w, h, cf = read_stream(e), e["width"], e["height"], e["chroma_format"]
    rows = h // 16
    bad, why = CS.damage_slices(es, w, h, cf, [first * rows, (first + n) * rows - 1])
    p = _host(bad, w, h, cf)
    scan = R.Scan(bad, w, h, cf, conceal=True)
    want = scan.parse_host(first, n)
    whole = PM.range_of_whole(p, first, n)
    assert want[0].tobytes() == whole[0].tobytes() and want[1].tobytes() == whole[1].tobytes()
    with R.DeviceContext(w, h, cf, slots=p.npics) as ctx:
        ctx.upload_es(scan, first, n)
        dev = ctx.download_records()
        assert dev[0].tobytes() == want[0].tobytes() and dev[1].tobytes() == want[1].tobytes()
        dmg = ctx.last_damage()
    assert [(int(d["pic"]), int(d["mb_row"])) for d in dmg] == [(0, 0), (n - 1, rows - 1)]
    assert np.array_equal(dmg["pic"] + first, p.damage["pic"]) and np.array_equal(dmg["byte_off"], p.damage["byte_off"])


# ---- repeat uploads ------------------------------------------------------------------------------------------------
def test_a_clean_upload_after_a_damaged_one_has_no_damage_and_clean_records(contexts):
    bad, es, w, h, cf, _ = CS.damaged_stream(CS.MULTI, CS.MULTI_DAMAGE)
    ctx = contexts.get(w, h, cf)
    p = _device_parity(ctx, bad, w, h, cf, decode=False)
    assert len(ctx.last_damage()) == len(CS.MULTI_DAMAGE) == len(p.damage)
    clean = R.Parsed(es, w, h, cf)
    for conceal in (True, False):
        scan = R.Scan(es, w, h, cf, conceal=conceal)
        scan.parse_host()
        ctx.upload_es(scan)
        dev = ctx.download_records()
        assert dev[0].tobytes() == clean.mbs.tobytes() and dev[1].tobytes() == clean.coefs.tobytes()
        assert len(ctx.last_damage()) == 0
        ctx.decode()
        ctx.synchronize()
        _frames_equal([ctx.download(q) for q in range(clean.npics)], oracle_frames(clean))
    # and without the flag the damaged stream fails as before, with nothing resident
    plain = PM.host(bad, w, h, cf)
    with pytest.raises(_lib.Mp2vgError) as ei:
        ctx.upload_es(R.Scan(bad, w, h, cf))
    assert (ei.value.status, PM.detail(str(ei.value))) == (plain[0], PM.detail(plain[1]))
    assert len(ctx.last_damage()) == 0


# ---- exports ------------------------------------------------------------------------------------------------------------
def test_motion_and_residual_exports_of_a_damaged_batch_equal_their_host_twins(contexts):
    bad, _, w, h, cf, _ = CS.damaged_stream(CS.MULTI, CS.MULTI_DAMAGE)
    p = _host(bad, w, h, cf)
    ctx = contexts.get(w, h, cf)
    scan = R.Scan(bad, w, h, cf, conceal=True)
    scan.parse_host()
    ctx.upload_es(scan)
    for got, want in zip(ctx.export_motion(), R.motion_host(p.pics, p.mbs, p.coefs, w, h, cf)):
        assert np.array_equal(got.cpu().numpy().view(want.dtype), want)
    for got, want in zip(ctx.export_residual(), R.residual_host(p.pics, p.mbs, p.coefs, w, h, cf)):
        assert np.array_equal(got.cpu().numpy(), want)
    for parse in ("device", "host"):
        m = R.decode_motion(bad, w, h, cf, parse=parse, conceal=True)
        r = R.decode_residual(bad, w, h, cf, parse=parse, conceal=True)
        assert _same_damage(m["damage"], p.damage) and _same_damage(r["damage"], p.damage)
        assert np.array_equal(r["types"], p.pics["picture_coding_type"][p.display])
        assert m["dist"][list(p.display).index(6), 0] != 0  # the re-typed I picture has a forward reference


def test_decode_rgb_and_decode_tensor_take_the_flag():
    bad, _, w, h, cf, _ = CS.damaged_stream(CS.MULTI, CS.MULTI_DAMAGE)
    p = _host(bad, w, h, cf)
    with pytest.raises(_lib.Mp2vgError):
        R.decode_rgb(bad, w, h, cf)
    a, da = R.decode_rgb(bad, w, h, cf, conceal=True, return_damage=True)
    b, db = R.decode_rgb(bad, w, h, cf, conceal=True, return_damage=True, device_parse=True)
    assert _same_damage(da, p.damage) and _same_damage(db, p.damage) and bool((a == b).all())
    assert tuple(a.shape) == (p.npics, 3, h, w)
    t, dt = R.decode_tensor(bad, w, h, cf, (w, h), dtype="uint8", conceal=True, return_damage=True, device_parse=True)
    assert _same_damage(dt, p.damage) and tuple(t.shape) == (p.npics, 3, h, w)
    assert bool((R.decode_tensor(bad, w, h, cf, (w, h), dtype="uint8", conceal=True) == t).all())


# ---- the drop-in decoder ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device_parse", [False, True], ids=["host_parse", "device_parse"])
@pytest.mark.parametrize("device_frames", [False, True], ids=["host_frames", "device_frames"])
def test_dropin_decodes_damaged_streams_with_the_flag(device_parse, device_frames):
    """24 pictures, so the decoder's second 16-picture chunk starts inside a GOP and picture 18, a damaged I
    picture, reads its conceal reference (picture 15) across the chunks; the frames are the
    Python path's (oracle-exact above), the count is the emitter's; without the flag decode() fails
    as it does today"""
    kw = dict(CS.MULTI, n_gops=4, seed=78)
    rows = [(0, 2), (6, 0), (13, 1), (16, 2), (17, 0), (18, 0), (18, 1)]
    bad, _, w, h, cf, _ = CS.damaged_stream(kw, rows)
    p = _host(bad, w, h, cf)
    assert p.npics == 24 and p.pics["picture_coding_type"][18] == 2 and p.flags[18] & _lib.PIC_RETYPED_I
    R.Scan(bad, w, h, cf, conceal=True).parse_host()  # the twin first
    want = oracle_frames(p)
    exp = [(int(d), hashlib.md5(R.frame_yuv_bytes(want[int(d)])).hexdigest()) for d in p.display]
    got = []
    dec = mp2v_decoder_c(decoder_config_t(w, h, cf, device_frames=device_frames, device_parse=device_parse,
                                          conceal=True),
                         lambda f: got.append((f.decode_index, hashlib.md5(f.yuv_bytes()).hexdigest())))
    try:
        assert dec.decode(bad) and got == exp
        assert dec.damage_count() == len(rows) == len(p.damage)
    finally:
        dec.close()
    plain = PM.host(bad, w, h, cf)
    dec = mp2v_decoder_c(decoder_config_t(w, h, cf, device_frames=device_frames, device_parse=device_parse),
                         lambda f: None)
    try:
        with pytest.raises(_lib.Mp2vgError) as ei:
            dec.decode(bad)
        assert (ei.value.status, PM.detail(str(ei.value))) == (plain[0], PM.detail(plain[1]))
        assert dec.damage_count() == 0
    finally:
        dec.close()
