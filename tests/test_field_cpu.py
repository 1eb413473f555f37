"""CPU: the field modes of the tensor export (include/mp2vg.h "Field modes"): the numpy yardstick
(tests/field_model.py) against hand-computed cases and its own invariants, the per-picture interlace
flags of both parsers against an independent bit reader, the generator's top_field_first, and the
argument validation of mp2vg_tensor_planes_field before any HIP call."""
import ctypes
import itertools

import numpy as np
import pytest

import export_model
import field_model as FM
from helpers import oracle_frames
from test_gpu_export import random_planes, visible
from tiny_mp2v_dec_amd import _lib
from tiny_mp2v_dec_amd import records as R

E_INVALID = -1


def planes(cf, w=16, h=8, seed=1):
    return visible(random_planes(cf, w, h, 64, seed), cf, w, h)


# ---- the model -------------------------------------------------------------------------------------

@pytest.mark.parametrize("linear", (False, True))
def test_weave_is_progressive_without_vertical_subsampling(linear):
    for cf in (2, 3):
        p = planes(cf, seed=10 + cf)
        assert np.array_equal(FM.source(p, cf, 1, linear, FM.WEAVE), FM.source(p, cf, 1, linear, FM.PROGRESSIVE))
    p = planes(1, seed=11)
    assert not np.array_equal(FM.source(p, 1, 1, linear, FM.WEAVE), FM.source(p, 1, 1, linear, FM.PROGRESSIVE))


@pytest.mark.parametrize("cf,linear,mode", itertools.product((1, 2, 3), (False, True), (FM.TOP, FM.BOTTOM)))
def test_a_single_field_never_reads_the_other(cf, linear, mode):
    """Randomise the other field's luma lines and its rows of both chroma planes (4:2:0: chroma rows
    of the other parity; else the lines themselves): the image must not change."""
    p = planes(cf, seed=20 + cf)
    want = FM.source(p, cf, 5, linear, mode)
    other = 1 if mode == FM.TOP else 0
    rng = np.random.default_rng(7)
    q = [a.copy() for a in p]
    for a in q:
        a[other::2] = rng.integers(0, 256, a[other::2].shape, dtype=np.uint8)
    assert not np.array_equal(q[0], p[0]) and not np.array_equal(q[1], p[1])
    assert np.array_equal(FM.source(q, cf, 5, linear, mode), want)
    # and it does read its own field
    q = [a.copy() for a in p]
    q[0][1 - other::2] ^= 0x80
    assert not np.array_equal(FM.source(q, cf, 5, linear, mode), want)


def grey(Y):
    """4 x 4 4:4:4 planes with neutral chroma: R = G = B = a function of Y alone."""
    Y = np.array(Y, np.uint8)
    return [Y, np.full_like(Y, 128), np.full_like(Y, 128)]


def test_hand_computed_line_averages_and_edges():
    """Luma 16 + 219 k / 255 rounded gives R = k for chosen k; use 16 -> 0, 235 -> 255, 126 -> 128:
    rows of constant value, so the averages can be done by hand."""
    rows = [16, 235, 126, 16]
    rgb = [0, 255, 128, 0]
    p = grey([[v] * 4 for v in rows])
    assert FM.source(p, 3, 1, False, FM.PROGRESSIVE)[0, :, 0].tolist() == rgb
    assert FM.source(p, 3, 1, False, FM.WEAVE)[0, :, 0].tolist() == rgb
    # TOP keeps lines 0, 2; line 1 = (0 + 128 + 1) >> 1 = 64; line 3: b = 4 > H - 1 -> b = a = 2: 128
    assert FM.source(p, 3, 1, False, FM.TOP)[0, :, 0].tolist() == [0, 64, 128, 128]
    # BOTTOM keeps lines 1, 3; line 0: a = -1 -> a = b = 1: 255; line 2 = (255 + 0 + 1) >> 1 = 128
    assert FM.source(p, 3, 1, False, FM.BOTTOM)[0, :, 0].tolist() == [255, 255, 128, 0]
    # the average rounds up: (0 + 255 + 1) >> 1 = 128, per channel, formed from 8-bit values
    p = grey([[16] * 4, [99] * 4, [235] * 4, [99] * 4])
    assert FM.source(p, 3, 1, False, FM.TOP)[0, :, 0].tolist() == [0, 128, 255, 255]


def test_hand_computed_420_chroma_taps():
    """8 luma lines, 4 chroma rows of constant value c[j]: every y mod 4 tap and both clamps."""
    c = [0, 160, 32, 240]
    C = np.array([[v] * 2 for v in c], np.uint8)
    got = FM.field_chroma(C, 1, True, 4, 8)[:, 0].tolist()
    # y: j, j1 (clamped to j when outside 0..3), weights
    want = [(2 * (7 * c[0] + 1 * c[0]) + 8) >> 4,   # y 0: j 0, j1 -2 -> 0; 7, 1
            (2 * (5 * c[1] + 3 * c[1]) + 8) >> 4,   # y 1: j 1, j1 -1 -> 1; 5, 3
            (2 * (5 * c[0] + 3 * c[2]) + 8) >> 4,   # y 2: j 0, j1 2; 5, 3
            (2 * (7 * c[1] + 1 * c[3]) + 8) >> 4,   # y 3: j 1, j1 3; 7, 1
            (2 * (7 * c[2] + 1 * c[0]) + 8) >> 4,   # y 4: j 2, j1 0; 7, 1
            (2 * (5 * c[3] + 3 * c[1]) + 8) >> 4,   # y 5: j 3, j1 1; 5, 3
            (2 * (5 * c[2] + 3 * c[2]) + 8) >> 4,   # y 6: j 2, j1 4 -> 2; 5, 3
            (2 * (7 * c[3] + 1 * c[3]) + 8) >> 4]   # y 7: j 3, j1 5 -> 3; 7, 1
    assert got == want == [0, 160, 12, 170, 28, 210, 32, 240]
    assert FM.field_chroma(C, 1, False, 4, 8)[:, 0].tolist() == [c[0], c[1], c[0], c[1], c[2], c[3], c[2], c[3]]
    # horizontal: odd x averages samples k and k + 1 (k1 clamps at the plane's edge)
    C = np.array([[0, 100]] * 4, np.uint8)
    assert FM.field_chroma(C, 1, True, 4, 8)[0].tolist() == [0, 50, 100, 100]


def test_progressive_rule_in_sixteenths():
    """(3 A + B + 4) >> 3 == (6 A + 2 B + 8) >> 4 for every pair of 8-bit pair sums A, B."""
    A, B = np.meshgrid(np.arange(511), np.arange(511))
    assert np.array_equal((3 * A + B + 4) >> 3, (6 * A + 2 * B + 8) >> 4)
    assert np.array_equal((4 * A + 4) >> 3, (8 * A + 8) >> 4)  # 4:2:2


def test_model_progressive_mode_is_the_tensor_model():
    import tensor_model as T
    p = planes(1, 48, 32, seed=31)
    for linear in (False, True):
        assert np.array_equal(FM.q_image(p, 1, 1, linear, FM.PROGRESSIVE, (10, 7), (1, 1, 45, 29)),
                              T.q_image(p, 1, 1, linear, (10, 7), (1, 1, 45, 29)))


# ---- picture flags ---------------------------------------------------------------------------------

def read_flags(es):
    """MP2VG_PIC_* of every picture_coding_extension (00 00 01 B5, id 8), read bit by bit."""
    out = []
    at = es.find(b"\x00\x00\x01\xb5")
    while at >= 0:
        body = es[at + 4:at + 12]
        bits = "".join(f"{b:08b}" for b in body)
        if int(bits[0:4], 2) == 8:
            # id 4, f_code 16, intra_dc_precision 2, picture_structure 2, then single-bit flags
            tff, rff, prog = int(bits[24]), int(bits[30]), int(bits[32])
            out.append(prog * 1 + tff * 2 + rff * 4)
        at = es.find(b"\x00\x00\x01\xb5", at + 4)
    return out


def stream(fpfd, tff, seed=77, cf=1):
    return R.generate_es(width=64, height=48, chroma_format=cf, n_gops=2, gop_n=6, gop_m=3, seed=seed,
                         frame_pred_frame_dct=fpfd, top_field_first=tff)


@pytest.mark.parametrize("fpfd,tff", itertools.product((0, 1), (0, 1, -1)))
def test_flags_of_both_parsers_equal_an_independent_reader(fpfd, tff):
    es = stream(fpfd, tff)
    want = read_flags(es)
    parsed = R.Parsed(es, 64, 48, 1)
    assert len(want) == parsed.npics == 12
    assert parsed.flags.dtype == np.uint32 and parsed.flags.tolist() == want
    with R.Scan(es, 64, 48, 1) as scan:
        assert scan.flags.dtype == np.uint32 and scan.flags.tolist() == want
    if fpfd:      # progressive_frame = 1: top_field_first is never written as 1
        assert want == [_lib.PIC_PROGRESSIVE_FRAME] * 12
    elif tff == 0:
        assert want == [0] * 12
    elif tff == 1:
        assert want == [_lib.PIC_TOP_FIELD_FIRST] * 12
    else:
        assert set(want) == {0, _lib.PIC_TOP_FIELD_FIRST}


def test_repeat_first_field_is_reported():
    """Set the repeat_first_field bit of one picture by hand: both parsers report it and nothing else
    changes (the bit is not part of what the decodable subset depends on)."""
    es = bytearray(stream(0, 1))
    at = -1
    for _ in range(3):
        at = es.find(b"\x00\x00\x01\xb5", at + 1)
        while es[at + 4] >> 4 != 8:
            at = es.find(b"\x00\x00\x01\xb5", at + 1)
    es[at + 4 + 3] |= 0x02  # bit 30 of the extension body
    es = bytes(es)
    want = read_flags(es)
    assert want.count(_lib.PIC_TOP_FIELD_FIRST | _lib.PIC_REPEAT_FIRST_FIELD) == 1
    assert R.Parsed(es, 64, 48, 1).flags.tolist() == want
    with R.Scan(es, 64, 48, 1) as scan:
        assert scan.flags.tolist() == want


def test_flag_accessors_check_their_arguments():
    L = _lib.lib()
    buf = (ctypes.c_uint32 * 4)()
    assert L.mp2vg_parsed_picture_flags(None, buf, 4) == E_INVALID
    assert L.mp2vg_scan_picture_flags(None, buf, 4) == E_INVALID
    es = stream(0, 1)
    with R.Scan(es, 64, 48, 1) as scan:
        assert L.mp2vg_scan_picture_flags(scan.h, buf, 4) == E_INVALID  # 12 pictures do not fit
        assert L.mp2vg_scan_picture_flags(scan.h, None, 12) == E_INVALID


def test_default_stream_is_byte_identical_and_struct_size_kept():
    assert ctypes.sizeof(_lib.GenParams) == 27 * 4
    p = R.gen_params()
    assert p.top_field_first == 0 and list(p.reserved) == [0] * 4
    for fpfd in (0, 1):
        a = R.generate_es(width=64, height=48, n_gops=1, gop_n=6, gop_m=3, seed=5, frame_pred_frame_dct=fpfd)
        b = R.generate_es(width=64, height=48, n_gops=1, gop_n=6, gop_m=3, seed=5, frame_pred_frame_dct=fpfd,
                          top_field_first=0)
        assert a == b


@pytest.mark.parametrize("cf", (1, 2))
def test_top_field_first_does_not_touch_pixels(cf):
    """The same stream with top_field_first = 0 and 1: the same records from both parsers, and the
    same frames from the oracle."""
    a, b = stream(0, 0, seed=91, cf=cf), stream(0, 1, seed=91, cf=cf)
    assert a != b and len(a) == len(b)
    pa, pb = R.Parsed(a, 64, 48, cf), R.Parsed(b, 64, 48, cf)
    assert pb.flags.tolist() == [_lib.PIC_TOP_FIELD_FIRST] * pb.npics
    assert pa.pics.tobytes() == pb.pics.tobytes() and pa.mbs.tobytes() == pb.mbs.tobytes()
    assert np.array_equal(pa.coefs, pb.coefs)
    with R.Scan(b, 64, 48, cf) as scan:
        mbs, coefs = scan.parse_host()
        assert mbs.tobytes() == pb.mbs.tobytes() and np.array_equal(coefs, pb.coefs)
    fa, fb = oracle_frames(pa), oracle_frames(pb)
    assert len(fa) == len(fb) == pa.npics
    for x, y in zip(fa, fb):
        assert all(np.array_equal(x[k], y[k]) for k in range(3))


# ---- validation without a device -------------------------------------------------------------------

def planes_field(cf, w, h, field, t=None):
    """mp2vg_tensor_planes_field on host addresses that are never dereferenced: every argument is
    checked before the first HIP call, so a refusal needs no device."""
    t = t or _lib.make_tensor((8, 4), dtype="uint8")
    buf = np.zeros(4096, np.uint8)
    ptrs = (ctypes.c_void_p * 3)(*[buf.ctypes.data] * 3)
    return _lib.lib().mp2vg_tensor_planes_field(0, ptrs, (ctypes.c_int32 * 3)(64, 64, 64), cf, w, h, field,
                                                ctypes.byref(t), ctypes.c_void_p(buf.ctypes.data), 3 * 8 * 4)


def test_planes_field_validation_before_any_hip_call():
    L = _lib.lib()
    for field in (-1, 4, 1 << 20):
        assert planes_field(1, 48, 32, field) == E_INVALID
        assert b"field" in L.mp2vg_last_error()
    for field in (1, 2, 3):
        assert planes_field(1, 48, 30, field) == E_INVALID      # 4:2:0 needs a multiple of 4
        assert b"field" in L.mp2vg_last_error()
        assert planes_field(2, 48, 31, field) == E_INVALID      # an odd height
        assert planes_field(3, 48, 31, field) == E_INVALID
    # the same arguments with a valid combination get past the validation: without a device that is
    # a HIP error, with one the call would run (not tried here: the addresses are host memory)
    import torch
    if not torch.cuda.is_available():
        assert planes_field(2, 48, 30, 1) == -3
        assert planes_field(1, 48, 30, 0) == -3


def test_python_field_spellings():
    assert [_lib.field_mode(n) for n in ("progressive", "top", "bottom", "weave")] == [0, 1, 2, 3]
    assert _lib.field_modes(None, 3) is None
    assert _lib.field_modes("top", 3).tolist() == [1, 1, 1]
    assert _lib.field_modes(["top", 2, "weave"], 3).tolist() == [1, 2, 3]
    for bad in ("both", 4, -1):
        with pytest.raises(ValueError):
            _lib.field_mode(bad)
    with pytest.raises(ValueError):
        _lib.field_modes(["top"], 2)
    # decode_tensor's plans: display order, flags in decode order
    display, flags = [0, 2, 1], np.array([1, 2, 0], np.uint32)  # progressive, tff (shown last), bff
    assert R.field_plan(display, flags, None)[1] is None
    s, m = R.field_plan(display, flags, "first")
    assert s.tolist() == [0, 2, 1] and m.tolist() == [0, 2, 1]
    s, m = R.field_plan(display, flags, "both")
    assert s.tolist() == [0, 0, 2, 2, 1, 1] and m.tolist() == [0, 0, 2, 1, 1, 2]
    assert R.field_plan(display, flags, "weave")[1].tolist() == [3, 3, 3]
    with pytest.raises(ValueError):
        R.field_plan(display, flags, "second")
