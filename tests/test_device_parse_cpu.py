"""CPU: the host scan (mp2vg_scan_es) and the CPU twin of the device slice parser
(mp2vg_scan_parse_host, which runs csrc/slice_parse.h, the kernels' own source) against the host
record emitter (mp2vg_parse_es), the yardstick: same pictures, same records byte for byte, same
status and message for every slice-level rejection."""
import ctypes

import numpy as np
import pytest

import parse_mutants as PM
from conftest import load_manifest, read_stream
from tiny_mp2v_dec_amd import _lib
from tiny_mp2v_dec_amd.records import Parsed, Scan, generate_es

MANIFEST = load_manifest()
BY_NAME = {e["name"]: e for e in MANIFEST}


def _geom(e):
    return e["width"], e["height"], e["chroma_format"]


_host, _twin, _detail, _same_records = PM.host, PM.twin, PM.detail, PM.same_records


@pytest.mark.parametrize("entry", MANIFEST, ids=[e["name"] for e in MANIFEST])
def test_scan_equals_parsed_and_twin_records_are_byte_identical(entry):
    es = read_stream(entry)
    p, s = Parsed(es, *_geom(entry)), Scan(es, *_geom(entry))
    assert s.pics.tobytes() == p.pics.tobytes()  # W matrices, slots, mb_first, types
    assert np.array_equal(s.display, p.display) and np.array_equal(s.gop, p.gop)
    assert np.array_equal(s.shard, p.shard) and s.nshards == p.nshards
    assert bytes(s.headers) == bytes(p.headers)
    assert s.nslices == p.npics * (entry["height"] // 16)
    assert _same_records(p, s.parse_host())


def test_twin_sub_range_is_the_range_of_the_whole():
    """pictures [first, first + n): the same records, rebased to the range (record 0, word 0)"""
    e = BY_NAME["ipb420_qcif"]
    es = read_stream(e)
    p, s = Parsed(es, *_geom(e)), Scan(es, *_geom(e))
    per = (e["width"] // 16) * (e["height"] // 16)
    first, n = 5, 7
    mbs, coefs = s.parse_host(first, n)
    want = p.mbs[first * per:(first + n) * per].copy()
    c0 = int(want["coef_off"][0])
    want["coef_off"] -= c0
    assert mbs.tobytes() == want.tobytes()
    assert coefs.tobytes() == p.coefs[c0:c0 + len(coefs)].tobytes()
    assert c0 + len(coefs) == int(p.mbs["coef_off"][(first + n) * per])


SWEEP = [
    # chroma format, frame_pred_frame_dct, width, f_code, leading_b
    (1, 1, 48, 1, 0), (1, 0, 64, 2, 1), (1, 0, 176, 3, 1), (2, 1, 64, 4, 0), (2, 0, 48, 2, 1),
    (2, 0, 176, 1, 0), (3, 1, 176, 3, 1), (3, 1, 48, 4, 0), (3, 0, 64, 2, 1),
]


@pytest.mark.parametrize("seed", range(1, 9))
def test_twin_equals_host_on_a_generator_sweep(seed):
    """every chroma format, frame and field MC / DCT, random scan, quantiser scale type and DC
    precision per picture, escapes and large levels raised, f_code 1-4, leading B pictures,
    row widths 48 (not a multiple of 4 macroblocks), 64 and 176"""
    for k, (cf, fpfd, width, f_code, leading_b) in enumerate(SWEEP):
        if (k + seed) % 3 == 0:  # each seed runs two thirds of the sweep, every case under 5+ seeds
            continue
        es = generate_es(width=width, height=48, chroma_format=cf, n_gops=2, gop_n=6, gop_m=3, seed=100 * seed + k,
                         frame_pred_frame_dct=fpfd, alternate_scan=-1, q_scale_type=-1, intra_dc_precision=-1,
                         escape_permille=250, big_level_permille=150, f_code=f_code, leading_b=leading_b)
        p, s = Parsed(es, width, 48, cf), Scan(es, width, 48, cf)
        assert s.pics.tobytes() == p.pics.tobytes()
        assert _same_records(p, s.parse_host()), (seed, cf, fpfd, width, f_code, leading_b)


# ---- rejections -----------------------------------------------------------------------------
_start_codes = PM.start_codes


def _gen(**kw):
    return generate_es(width=176, height=144, n_gops=1, gop_n=4, gop_m=1, leading_b=0, **kw)


def _check_same_rejection(es, status, reason, w=176, h=144, cf=1):
    hs, hm, _ = _host(es, w, h, cf)
    ts, tm, _, _ = _twin(es, w, h, cf)
    assert hs == status and reason in hm, hm
    assert ts == status and _detail(tm) == _detail(hm), (tm, hm)


def test_scan_rejects_a_slice_row_outside_the_picture():
    es = _gen()
    o = _start_codes(es, 0x03)[0]
    es = es[:o + 3] + bytes([0x0A]) + es[o + 4:]  # row 9 of a 9-row picture
    _check_same_rejection(es, -2, "slice row outside the picture")


def test_scan_rejects_two_slices_in_one_row():
    es = _gen()
    o = _start_codes(es, 0x03)[0]
    es = es[:o + 3] + bytes([0x02]) + es[o + 4:]
    _check_same_rejection(es, -2, "two slices in one macroblock row")


def test_scan_rejects_an_uncovered_row():
    es = _gen()
    o = _start_codes(es, 0x09)[-1]  # the last picture loses its last slice
    nxt = es.find(b"\x00\x00\x01", o + 4)
    es = es[:o] + (es[nxt:] if nxt >= 0 else b"")
    _check_same_rejection(es, -2, "row not covered by any slice")


def test_twin_rejects_intra_vlc_format_zero():
    es = PM.vlc0_stream()[0]
    _check_same_rejection(es, -2, "intra_vlc_format=0")


def test_twin_rejects_a_truncated_last_slice():
    """every row still has its slice, the last one ends early: the reader runs into the zeros past
    the buffer (the GPU error test uploads this stream)"""
    es = _gen()
    o = _start_codes(es, 0x09)[-1]
    es = es[:o + 12]
    hs, hm, _ = _host(es, 176, 144, 1)
    ts, tm, _, by_scan = _twin(es, 176, 144, 1)
    assert hs == -6 and not by_scan
    assert ts == hs and _detail(tm) == _detail(hm)


SLICE_REASONS = PM.SLICE_REASONS  # (and why four reasons are not in the list)


@pytest.fixture(scope="module")
def mutants():
    """Fixed-seed single-byte mutants of four small streams, each through the host emitter and the
    twin once: (host status, host message, twin status, twin message, rejected by the scan,
    records equal when both accept).  Byte mutations inside one slice give one failing slice, so
    status and message must agree exactly unless the scan itself rejected."""
    out = []
    for si, (es, w, h, cf) in enumerate(PM.base_streams()):
        for pos, val in PM.walk(si, es):
            b = PM.mutate(es, pos, val)
            hs, hm, p = _host(b, w, h, cf)
            ts, tm, rec, by_scan = _twin(b, w, h, cf)
            same = _same_records(p, rec) if hs == 0 and ts == 0 else None
            out.append((hs, hm, ts, tm, by_scan, same))
    return out


def test_mutants_accepted_iff_accepted_with_identical_records(mutants):
    assert sum(1 for m in mutants if m[0] == 0) > 50 and sum(1 for m in mutants if m[0] != 0) > 500
    for hs, hm, ts, tm, by_scan, same in mutants:
        assert (hs == 0) == (ts == 0), (hm, tm)
        assert same in (None, True)
        if hs != 0 and not by_scan:
            assert ts == hs and _detail(tm) == _detail(hm), (hm, tm)


@pytest.mark.parametrize("reason", SLICE_REASONS)
def test_each_slice_level_rejection_has_the_host_status_and_message(mutants, reason):
    hits = [m for m in mutants if reason in m[1] and not m[4]]
    assert hits, f"no mutant is rejected by the host emitter with '{reason}'"
    for hs, hm, ts, tm, _, _ in hits:
        assert ts == hs and _detail(tm) == _detail(hm)


@pytest.mark.parametrize("name", ["ipb420_field", "ipb422_qcif", "ipb444_field"])
def test_truncations_and_bit_flips_of_golden_streams(name):
    e = BY_NAME[name]
    es = read_stream(e)
    rng = np.random.default_rng(sum(name.encode()))
    accepted = rejected = 0
    for it in range(120):
        b = bytearray(es)
        if it % 2:
            b = b[:int(rng.integers(0, len(b)))]
        else:
            for _ in range(int(rng.integers(1, 4))):
                b[int(rng.integers(0, len(b)))] ^= 1 << int(rng.integers(0, 8))
        hs, hm, p = _host(bytes(b), *_geom(e))
        ts, tm, rec, _ = _twin(bytes(b), *_geom(e))
        assert (hs == 0) == (ts == 0), (it, hm, tm)
        if hs == 0:
            accepted += 1
            assert _same_records(p, rec), it
        else:
            rejected += 1
    assert accepted and rejected


# ---- arguments, and no CPU fallback ------------------------------------------------------------
def test_invalid_arguments():
    L = _lib.lib()
    e = BY_NAME["ipb420_qcif"]
    s = Scan(read_stream(e), *_geom(e))
    h = ctypes.c_void_p()
    cfg = _lib.make_config(*_geom(e))
    assert L.mp2vg_scan_es(None, 0, ctypes.byref(cfg), ctypes.byref(h)) == -1
    assert L.mp2vg_scan_es(s._buf.ctypes.data_as(ctypes.c_void_p), 10, None, ctypes.byref(h)) == -1
    assert L.mp2vg_scan_counts(None, None, None) == -1
    assert L.mp2vg_scan_parse_host(None, 0, 1, None, 0, None, 0, None, None) == -1
    for first, n in ((-1, 1), (0, 0), (0, s.npics + 1), (s.npics, 1)):
        assert L.mp2vg_scan_parse_host(s.h, first, n, None, 0, None, 0, None, None) == -1
    mbs = np.zeros(5, _lib.MB_DTYPE)  # not the range's macroblock count
    assert L.mp2vg_scan_parse_host(s.h, 0, 1, mbs.ctypes.data_as(ctypes.c_void_p), 5, None, 0, None, None) == -1
    assert L.mp2vg_batch_upload_es(None, s.h, None, 0, 1) == -1
    assert L.mp2vg_batch_record_counts(None, None, None) == -1
    assert L.mp2vg_batch_download_records(None, None, 0, None, 0) == -1
    assert L.mp2vg_last_parse_times(None, None) == -1


def test_no_cpu_fallback_for_the_device_parse_without_gpu():
    """Without a device there is no context to upload to: the device-parse paths fail with
    MP2VG_E_HIP as mp2vg_create does, and never fall back to the host emitter."""
    try:
        import torch
        if torch.cuda.is_available():
            pytest.skip("a GPU is present")
    except ImportError:
        pass
    from tiny_mp2v_dec_amd.decoder import decoder_config_t, mp2v_decoder_c
    from tiny_mp2v_dec_amd.records import DeviceContext
    e = BY_NAME["ipb420_qcif"]
    s = Scan(read_stream(e), *_geom(e))
    with pytest.raises(_lib.Mp2vgError) as ei:
        with DeviceContext(*_geom(e), slots=s.npics) as ctx:
            ctx.upload_es(s)
    assert ei.value.status == -3
    with pytest.raises(_lib.Mp2vgError) as ei:
        mp2v_decoder_c(decoder_config_t(*_geom(e), device_parse=True), lambda f: None)
    assert ei.value.status == -3
