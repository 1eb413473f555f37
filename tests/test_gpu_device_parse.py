"""GPU: the device parse (parse.hip through mp2vg_batch_upload_es): the records it leaves in HBM
equal the host emitter's byte for byte, the batch plans and decodes like the same batch uploaded
from host records, and the public paths that opt into it deliver the same frames."""
import hashlib

import numpy as np
import pytest

import parse_mutants as PM
from conftest import load_manifest, read_stream
from helpers import oracle_frames, yuv_md5
from tiny_mp2v_dec_amd import _lib
from tiny_mp2v_dec_amd import records as R

pytestmark = pytest.mark.gpu

MANIFEST = load_manifest()
BY_NAME = {e["name"]: e for e in MANIFEST}


@pytest.fixture(scope="module", autouse=True)
def _torch_runtime_first():
    """torch brings its own HIP runtime: it has to open the device before the library's does (as
    decode_rgb / decode_tensor do, which allocate the output tensor before they create a context),
    or torch finds no GPU when this file runs on its own."""
    import torch
    torch.zeros(1, device="cuda")


def _geom(e):
    return e["width"], e["height"], e["chroma_format"]


def _device_decode(es, w, h, cf):
    """(host-parsed records, frames in decode order decoded from device-parsed records, their
    records as downloaded, launch count)"""
    parsed, scan = R.Parsed(es, w, h, cf), R.Scan(es, w, h, cf)
    with R.DeviceContext(w, h, cf, slots=parsed.npics) as ctx:
        ctx.upload_es(scan)
        mbs, coefs = ctx.download_records()
        ctx.decode()
        ctx.synchronize()
        frames = [ctx.download(int(p["dst_slot"])) for p in scan.pics]
        return parsed, frames, (mbs, coefs), len(ctx.launch_times_ms())


def _assert_frames_equal(got, want):
    assert len(got) == len(want)
    for d, (a, b) in enumerate(zip(got, want)):
        for p in range(3):
            assert np.array_equal(a[p], b[p]), (d, p)


@pytest.mark.parametrize("entry", MANIFEST, ids=[e["name"] for e in MANIFEST])
def test_golden_streams_records_launches_and_frames(entry):
    es = read_stream(entry)
    parsed, frames, (mbs, coefs), nlaunch = _device_decode(es, *_geom(entry))
    assert mbs.tobytes() == parsed.mbs.tobytes()
    assert coefs.tobytes() == parsed.coefs.tobytes()
    with R.DeviceContext(*_geom(entry), slots=parsed.npics) as ctx:  # the same batch from host records
        ctx.upload(parsed.pics, parsed.mbs, parsed.coefs)
        ctx.decode()
        ctx.synchronize()
        assert nlaunch == len(ctx.launch_times_ms())
    assert [yuv_md5(frames[d]) for d in parsed.display] == entry["md5"]


@pytest.mark.parametrize("nslices", [1, 63, 64, 65, 130])
def test_lane_and_wave_edges(nslices):
    """I-only streams of one-row 16x16 pictures: one slice per picture, so the slice count is the
    picture count: one lane, a wave less one, a full wave, a wave and a lane, two waves and two"""
    es = R.generate_es(width=16, height=16, n_gops=nslices, gop_n=1, gop_m=1, mix=1, leading_b=0, seed=nslices)
    parsed, frames, (mbs, coefs), _ = _device_decode(es, 16, 16, 1)
    assert parsed.npics == nslices and R.Scan(es, 16, 16, 1).nslices == nslices
    assert mbs.tobytes() == parsed.mbs.tobytes() and coefs.tobytes() == parsed.coefs.tobytes()
    _assert_frames_equal(frames, oracle_frames(parsed))


@pytest.mark.parametrize("kw", [
    dict(width=48, height=32, chroma_format=3, n_gops=2, gop_n=6, gop_m=3),
    dict(width=80, height=32, chroma_format=2, n_gops=2, gop_n=6, gop_m=3, frame_pred_frame_dct=0),
    dict(width=176, height=144, chroma_format=1, n_gops=1, gop_n=8, gop_m=2),  # 72 slices: a partial second wave
], ids=["48x32_444", "80x32_422_field", "176x144_420_ipb"])
def test_generated_streams_vs_oracle(kw):
    es = R.generate_es(seed=3, escape_permille=100, **kw)
    w, h, cf = kw["width"], kw["height"], kw["chroma_format"]
    parsed, frames, (mbs, coefs), _ = _device_decode(es, w, h, cf)
    if w == 176:
        assert R.Scan(es, w, h, cf).nslices == 72
    if kw.get("frame_pred_frame_dct") == 0:
        assert np.any(parsed.mbs["flags"] & _lib.MB_FIELD_MC)
    assert mbs.tobytes() == parsed.mbs.tobytes() and coefs.tobytes() == parsed.coefs.tobytes()
    _assert_frames_equal(frames, oracle_frames(parsed))


@pytest.mark.parametrize("seed", PM.TAIL_SEEDS)
def test_reader_tail_last_slice_ends_at_the_last_byte(seed):
    """no sequence_end_code after the last slice: its last byte is the buffer's last byte, and the
    reader's refills run into the pad.  The four streams' uploaded spans are 0, 1, 2 and 3 bytes
    past a multiple of 4 long, so the hand-over from aligned loads to the byte-wise tail is met at
    each distance from the hard end."""
    assert sorted(PM.tail_span(PM.tail_stream(s)) % 4 for s in PM.TAIL_SEEDS) == [0, 1, 2, 3]
    es = PM.tail_stream(seed)  # (asserts the end code before it strips it)
    assert not es.endswith(b"\x00\x00\x01\xb7")
    parsed, frames, (mbs, coefs), _ = _device_decode(es, 64, 32, 1)
    assert mbs.tobytes() == parsed.mbs.tobytes() and coefs.tobytes() == parsed.coefs.tobytes()
    _assert_frames_equal(frames, oracle_frames(parsed))


def test_sub_ranges_two_batches_with_remapped_slots():
    """one stream as two consecutive upload_es batches (so both record banks are used), slots
    remapped by the caller; the second batch predicts from slots the first one wrote"""
    w, h, cf = 176, 144, 1
    es = R.generate_es(width=w, height=h, n_gops=1, gop_n=10, gop_m=3, leading_b=0, seed=9)
    parsed, scan = R.Parsed(es, w, h, cf), R.Scan(es, w, h, cf)
    n, per = scan.npics, (w // 16) * (h // 16)
    cut = next(i for i in range(3, n) if parsed.pics["picture_coding_type"][i] != 3)  # second batch starts at a P
    later_fwd = parsed.pics["fwd_slot"][cut:]
    assert np.any((later_fwd >= 0) & (later_fwd < cut))  # the second batch reads the first one's slots
    slot = lambda s: -1 if s < 0 else n - 1 - int(s)  # noqa: E731  (any permutation of the slots)
    with R.DeviceContext(w, h, cf, slots=n) as ctx:
        got = {}
        for first, cnt in ((0, cut), (cut, n - cut)):
            pics = scan.pics[first:first + cnt].copy()
            for i, p in enumerate(pics):
                p["dst_slot"], p["fwd_slot"], p["bwd_slot"] = slot(p["dst_slot"]), slot(p["fwd_slot"]), slot(p["bwd_slot"])
                p["mb_first"] = (cnt - 1 - i) * per  # records in reverse picture order
            ctx.upload_es(scan, first, cnt, pics=pics)
            mbs, coefs = ctx.download_records()
            for i in range(cnt):  # each picture's records are the host's, words rebased to the batch
                a = mbs[(cnt - 1 - i) * per:(cnt - i) * per]
                b = parsed.mbs[(first + i) * per:(first + i + 1) * per]
                for f in ("x", "y", "flags", "cbp", "qscale", "ncoef", "mv"):
                    assert np.array_equal(a[f], b[f])
                assert np.array_equal(a["coef_off"] - a["coef_off"][0], b["coef_off"] - b["coef_off"][0])
            ctx.decode()
            ctx.synchronize()
            for i in range(first, first + cnt):
                got[i] = ctx.download(slot(i))
    _assert_frames_equal([got[i] for i in range(n)], oracle_frames(parsed))


def test_rejected_slice_returns_the_twins_status_and_leaves_the_context_usable():
    w, h, cf = 176, 144, 1
    good = R.generate_es(width=w, height=h, n_gops=1, gop_n=4, gop_m=1, leading_b=0)
    cutat = good.rfind(b"\x00\x00\x01\x09")
    bad = good[:cutat + 12]  # every row has its slice; the last one ends early
    scan = R.Scan(bad, w, h, cf)
    with pytest.raises(_lib.Mp2vgError) as twin:
        scan.parse_host()
    assert twin.value.status == -6
    with R.DeviceContext(w, h, cf, slots=scan.npics) as ctx:
        with pytest.raises(_lib.Mp2vgError) as dev:
            ctx.upload_es(scan)
        assert dev.value.status == twin.value.status
        assert str(dev.value).split("(", 1)[1] == str(twin.value).split("(", 1)[1]
        with pytest.raises(_lib.Mp2vgError) as st:
            ctx.decode()
        assert st.value.status == -5  # MP2VG_E_STATE
        parsed, ok = R.Parsed(good, w, h, cf), R.Scan(good, w, h, cf)
        ctx.upload_es(ok)
        ctx.decode()
        ctx.synchronize()
        _assert_frames_equal([ctx.download(int(p["dst_slot"])) for p in ok.pics], oracle_frames(parsed))
        assert len(ctx.parse_times_ms()) == 3 and all(t >= 0 for t in ctx.parse_times_ms())


def test_decode_tensor_with_device_parse_is_byte_identical():
    import torch
    e = BY_NAME["ipb420_qcif"]
    es = read_stream(e)
    a = R.decode_tensor(es, *_geom(e), size=(96, 80), dtype="float16")
    b = R.decode_tensor(es, *_geom(e), size=(96, 80), dtype="float16", device_parse=True)
    assert a.shape == b.shape and torch.equal(a.view(torch.int16), b.view(torch.int16))
    c = R.decode_rgb(es, *_geom(e))
    d = R.decode_rgb(es, *_geom(e), device_parse=True)
    assert torch.equal(c, d)


@pytest.mark.parametrize("device_frames", [False, True], ids=["host_frames", "device_frames"])
@pytest.mark.parametrize("name", ["ipb420_qcif", "ipb422_field"])
def test_dropin_decoder_with_device_parse(name, device_frames):
    from tiny_mp2v_dec_amd.decoder import decoder_config_t, mp2v_decoder_c
    e = BY_NAME[name]
    md5 = []

    def render(f):
        md5.append(hashlib.md5(f.yuv_bytes()).hexdigest())

    dec = mp2v_decoder_c(decoder_config_t(*_geom(e), device_frames=device_frames, device_parse=True), render)
    try:
        dec.decode(read_stream(e))
    finally:
        dec.close()
    assert md5 == e["md5"]
