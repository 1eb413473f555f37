"""CPU: the placed tensor export (include/mp2vg.h "Placement"): mp2vg_tensor_fit and
mp2vg_stream_pixel_aspect against the Fraction model (tests/place_model.py), the argument validation
of mp2vg_tensor_planes_placed before any HIP call, the numpy yardstick against hand-computed values,
and the Python spellings.  Every comparison is exact."""
import ctypes
import itertools
import random

import numpy as np
import pytest

import field_model as FM
import place_model as PM
from test_gpu_export import random_planes, visible
from tiny_mp2v_dec_amd import _lib
from tiny_mp2v_dec_amd import records as R

E_INVALID, E_UNSUPPORTED = -1, -2
PARS = ((1, 1), (64, 45), (16, 15), (8, 9), (12, 11), (10, 11))
MODES = (PM.STRETCH, PM.CONTAIN, PM.COVER)


# ---- mp2vg_tensor_fit ------------------------------------------------------------------------------

def c_fit(mode, src, par, size):
    """(status, src_out, dst_out) of the library."""
    so, do = (ctypes.c_int32 * 4)(), (ctypes.c_int32 * 4)()
    rc = _lib.lib().mp2vg_tensor_fit(mode, (ctypes.c_int32 * 4)(*src), par[0], par[1], size[0], size[1], so, do)
    return rc, tuple(so), tuple(do)


def check_invariants(mode, src, size, so, do):
    x, y, w, h = src
    ow, oh = size
    assert so[0] >= x and so[1] >= y and so[2] >= 1 and so[3] >= 1 and so[0] + so[2] <= x + w and so[1] + so[3] <= y + h
    assert do[0] >= 0 and do[1] >= 0 and do[2] >= 1 and do[3] >= 1 and do[0] + do[2] <= ow and do[1] + do[3] <= oh
    if mode == PM.STRETCH:
        assert so == tuple(src) and do == (0, 0, ow, oh)
    if mode == PM.CONTAIN:  # the whole source, touching two opposite edges of the canvas, centred
        assert so == tuple(src)
        assert (do[0] == 0 and do[2] == ow) or (do[1] == 0 and do[3] == oh)
        assert do[0] == (ow - do[2]) // 2 and do[1] == (oh - do[3]) // 2
    if mode == PM.COVER:    # the whole canvas from a crop that keeps one side of the source whole
        assert do == (0, 0, ow, oh)
        assert (so[0] == x and so[2] == w) or (so[1] == y and so[3] == h)


def test_fit_exhaustive_small_sizes():
    """Every w, h, out_w, out_h in 1..12 with six pixel aspects and the three modes (no ratio is
    above 32 here, so every case succeeds)."""
    n = 0
    for par in PARS:
        for w, h, ow, oh in itertools.product(range(1, 13), repeat=4):
            src = (w % 3, h % 2, w, h)
            for mode in MODES:
                rc, so, do = c_fit(mode, src, par, (ow, oh))
                assert rc == 0 and (so, do) == PM.fit(mode, src, par, (ow, oh)), (mode, src, par, ow, oh)
                if (w + ow) % 4 == 0:
                    check_invariants(mode, src, (ow, oh), so, do)
                n += 1
    assert n == 12 ** 4 * 6 * 3


def test_fit_random_large_sizes():
    """2,000 seeded cases with sizes up to 16384 and par up to 2^24 (the 64-bit products): equal to
    the model, or MP2VG_E_INVALID exactly when the model's result has a ratio above 32."""
    rng = random.Random(20261)

    def size():  # small, medium and extreme values all occur
        return rng.choice((rng.randint(1, 40), rng.randint(1, 2000), rng.randint(1, 16384), 16384))

    refused = 0
    for i in range(2000):
        src = (rng.randint(0, 100), rng.randint(0, 100), size(), size())
        out = (size(), size())
        par = rng.choice((rng.choice(PARS), (rng.randint(1, 1 << 24), rng.randint(1, 1 << 24)), (1 << 24, 1),
                          (1, 1 << 24)))
        mode = MODES[i % 3]
        rc, so, do = c_fit(mode, src, par, out)
        want = PM.fit(mode, src, par, out)
        if want[0][2] > 32 * want[1][2] or want[0][3] > 32 * want[1][3]:
            assert rc == E_INVALID and b"ratio" in _lib.lib().mp2vg_last_error(), (mode, src, par, out)
            refused += 1
        else:
            assert rc == 0 and (so, do) == want, (mode, src, par, out)
            check_invariants(mode, src, out, so, do)
    assert 0 < refused < 1500


def test_fit_hand_computed_ties_and_clamps():
    C, V = PM.CONTAIN, PM.COVER
    cases = [
        # 4:2 into 5 x 5: the height 2 * 5 / 4 = 2.5 rounds up to 3; (5 - 3) >> 1 = 1
        (C, (0, 0, 4, 2), (1, 1), (5, 5), (0, 0, 4, 2), (0, 1, 5, 3)),
        # 3:2 into 5 x 5: 10 / 3 = 3.33 -> 3
        (C, (0, 0, 3, 2), (1, 1), (5, 5), (0, 0, 3, 2), (0, 1, 5, 3)),
        # 2:4 into 5 x 5 (pillarbox): the width 2 * 5 / 4 = 2.5 -> 3, x = 1
        (C, (0, 0, 2, 4), (1, 1), (5, 5), (0, 0, 2, 4), (1, 0, 3, 5)),
        # the same shape from non-square pixels: 4 x 4 with pixels 1:2 wide is shown 2:4
        (C, (0, 0, 4, 4), (1, 2), (5, 5), (0, 0, 4, 4), (1, 0, 3, 5)),
        # 720 x 576 with 64:45 pixels is 16:9: 640 x 360 in 640 x 640, rows 140..499
        (C, (0, 0, 720, 576), (64, 45), (640, 640), (0, 0, 720, 576), (0, 140, 640, 360)),
        (C, (0, 0, 1920, 1080), (1, 1), (640, 640), (0, 0, 1920, 1080), (0, 140, 640, 360)),
        # 12:1 into 2 x 2: 2 / 12 rounds to 0 and is clamped to 1; (2 - 1) >> 1 = 0
        (C, (0, 0, 12, 1), (1, 1), (2, 2), (0, 0, 12, 1), (0, 0, 2, 1)),
        # an exact fit has no bars
        (C, (3, 5, 8, 6), (1, 1), (4, 3), (3, 5, 8, 6), (0, 0, 4, 3)),
        # cover, 4:2 into a square: the width 2 * 3 / 3 = 2, x = (4 - 2) >> 1 = 1
        (V, (0, 0, 4, 2), (1, 1), (3, 3), (1, 0, 2, 2), (0, 0, 3, 3)),
        # cover, 5:2 into 5 x 4: the width 2 * 5 / 4 = 2.5 -> 3, x = 1
        (V, (0, 0, 5, 2), (1, 1), (5, 4), (1, 0, 3, 2), (0, 0, 5, 4)),
        # cover with an odd remainder and an origin: width 2 of 7, x = 2 + (5 >> 1) = 4
        (V, (2, 3, 7, 2), (1, 1), (1, 1), (4, 3, 2, 2), (0, 0, 1, 1)),
        # cover, 2:6 into a square (too tall): the height 2, y = 1 + ((6 - 2) >> 1) = 3
        (V, (1, 1, 2, 6), (1, 1), (4, 4), (1, 3, 2, 2), (0, 0, 4, 4)),
        # cover, 720 x 576 at 64:45 into a square: the width 576 * 45 / 64 = 405, x = 157
        (V, (0, 0, 720, 576), (64, 45), (224, 224), (157, 0, 405, 576), (0, 0, 224, 224)),
    ]
    for mode, src, par, size, so, do in cases:
        assert c_fit(mode, src, par, size) == (0, so, do), (mode, src, par, size)
        assert PM.fit(mode, src, par, size) == (so, do), (mode, src, par, size)
    assert _lib.tensor_fit("contain", (0, 0, 4, 2), (1, 1), (5, 5)) == ((0, 0, 4, 2), (0, 1, 5, 3))


def test_fit_refusals():
    ok = (PM.CONTAIN, (0, 0, 16, 8), (1, 1), (8, 8))
    assert c_fit(*ok)[0] == 0
    bad = [(-1,) + ok[1:], (3,) + ok[1:],
           (ok[0], (0, 0, 0, 8)) + ok[2:], (ok[0], (0, 0, 16, 0)) + ok[2:], (ok[0], (-1, 0, 16, 8)) + ok[2:],
           (ok[0], (0, -1, 16, 8)) + ok[2:], (ok[0], (0, 0, 16385, 8)) + ok[2:],
           ok[:2] + ((0, 1), ok[3]), ok[:2] + ((1, 0), ok[3]), ok[:2] + (((1 << 24) + 1, 1), ok[3]),
           ok[:2] + ((1, (1 << 24) + 1), ok[3]),
           ok[:3] + ((0, 8),), ok[:3] + ((8, 0),), ok[:3] + ((16385, 8),), ok[:3] + ((8, 16385),)]
    for case in bad:
        assert c_fit(*case)[0] == E_INVALID, case
    # the ratio: 66 rows into 2 is 33:1; letterboxed, 1320 x 33 becomes 40 x 1, 33 rows into 1
    assert c_fit(PM.STRETCH, (0, 0, 8, 66), (1, 1), (8, 2))[0] == E_INVALID
    assert c_fit(PM.STRETCH, (0, 0, 8, 64), (1, 1), (8, 2))[0] == 0
    assert c_fit(PM.CONTAIN, (0, 0, 1320, 33), (1, 1), (40, 40)) == (E_INVALID, (0,) * 4, (0,) * 4)  # nothing written
    L = _lib.lib()
    four = (ctypes.c_int32 * 4)(0, 0, 4, 4)
    assert L.mp2vg_tensor_fit(1, None, 1, 1, 4, 4, four, four) == E_INVALID
    assert L.mp2vg_tensor_fit(1, four, 1, 1, 4, 4, None, four) == E_INVALID
    assert L.mp2vg_tensor_fit(1, four, 1, 1, 4, 4, four, None) == E_INVALID
    with pytest.raises(ValueError):
        _lib.tensor_fit("letterbox", (0, 0, 4, 4), (1, 1), (4, 4))
    with pytest.raises(_lib.Mp2vgError):
        _lib.tensor_fit("contain", (0, 0, 4, 4), (0, 1), (4, 4))


# ---- mp2vg_stream_pixel_aspect ---------------------------------------------------------------------

def headers(code, w, h, display=None, ext=(0, 0)):
    hd = _lib.StreamHeaders()
    hd.sequence_header.aspect_ratio_information = code
    hd.sequence_header.horizontal_size_value, hd.sequence_header.vertical_size_value = w, h
    hd.sequence_extension.horizontal_size_extension, hd.sequence_extension.vertical_size_extension = ext
    if display is not None:
        hd.have_sequence_display_extension = 1
        hd.sequence_display_extension.display_horizontal_size = display[0]
        hd.sequence_display_extension.display_vertical_size = display[1]
    return hd


def test_pixel_aspect_of_header_fields():
    cases = [((2, 720, 576), (16, 15)), ((3, 720, 576), (64, 45)), ((2, 720, 480), (8, 9)), ((3, 720, 480), (32, 27)),
             ((3, 1920, 1080), (1, 1)), ((1, 720, 576), (1, 1)), ((4, 720, 576), (221, 125)),
             ((2, 704, 576), (12, 11)), ((2, 704, 480), (10, 11)), ((2, 352, 288), (12, 11))]
    for (code, w, h), want in cases:
        assert R.pixel_aspect(headers(code, w, h)) == want == PM.pixel_aspect(code, w, h), (code, w, h)
        # a display extension of the same size changes nothing; one of zero size is not used
        assert R.pixel_aspect(headers(code, w, h, (w, h))) == want
        assert R.pixel_aspect(headers(code, w, h, (0, h))) == want
        assert R.pixel_aspect(headers(code, w, h, (w, 0))) == want
    # the display sizes win over the coded ones: 1920 x 1088 coded, 1920 x 1080 shown at 16:9
    assert R.pixel_aspect(headers(3, 1920, 1088)) == (136, 135) == PM.pixel_aspect(3, 1920, 1088)
    assert R.pixel_aspect(headers(3, 1920, 1088, (1920, 1080))) == (1, 1)
    assert R.pixel_aspect(headers(2, 720, 576, (704, 576))) == (12, 11)
    assert R.pixel_aspect(headers(1, 720, 576, (704, 576))) == (1, 1)
    # the size extensions are the bits above the 12 of the size values: 4096 + 704 = 4800 x 2700 at 16:9
    assert R.pixel_aspect(headers(3, 704, 2700, ext=(1, 0))) == (1, 1)
    assert R.pixel_aspect(headers(2, 1024, 1024, ext=(0, 1))) == PM.pixel_aspect(2, 1024, 4096 + 1024) == (20, 3)
    L = _lib.lib()
    n, d = ctypes.c_int32(7), ctypes.c_int32(7)
    for code in (0, 5, 6, 15):
        assert PM.pixel_aspect(code, 720, 576) is None
        assert L.mp2vg_stream_pixel_aspect(ctypes.byref(headers(code, 720, 576)), ctypes.byref(n),
                                           ctypes.byref(d)) == E_UNSUPPORTED
        assert b"aspect_ratio_information" in L.mp2vg_last_error()
        with pytest.raises(_lib.Mp2vgError):
            R.pixel_aspect(headers(code, 720, 576))
    assert L.mp2vg_stream_pixel_aspect(ctypes.byref(headers(2, 0, 576)), ctypes.byref(n), ctypes.byref(d)) == E_INVALID
    assert L.mp2vg_stream_pixel_aspect(None, ctypes.byref(n), ctypes.byref(d)) == E_INVALID
    assert L.mp2vg_stream_pixel_aspect(ctypes.byref(headers(2, 720, 576)), None, ctypes.byref(d)) == E_INVALID


def with_aspect(es, code):
    """The stream with aspect_ratio_information = code: the high nibble of byte 7 of the sequence
    header (start code 4 bytes, two 12-bit sizes 3 bytes)."""
    es = bytearray(es)
    at = es.find(b"\x00\x00\x01\xb3")
    assert at >= 0
    es[at + 7] = (code << 4) | (es[at + 7] & 0x0F)
    return bytes(es)


def with_display_extension(es, w, h):
    """The stream with a sequence_display_extension (no colour description) of w x h behind its
    sequence_extension: id 2 (4 bits), video_format 5 (3), colour_description 0 (1),
    display_horizontal_size (14), marker (1), display_vertical_size (14), 3 bits of padding."""
    at = es.find(b"\x00\x00\x01\xb5", es.find(b"\x00\x00\x01\xb3"))
    nxt = es.find(b"\x00\x00\x01", at + 4)
    bits = (2 << 36) | (5 << 33) | (0 << 32) | (w << 18) | (1 << 17) | (h << 3)
    return es[:nxt] + b"\x00\x00\x01\xb5" + bits.to_bytes(5, "big") + es[nxt:]


@pytest.fixture(scope="module")
def pal_stream():
    return R.generate_es(width=720, height=576, chroma_format=1, n_gops=1, gop_n=1, gop_m=1, seed=3)


def test_pixel_aspect_of_a_patched_stream(pal_stream):
    for code, want in ((1, (1, 1)), (2, (16, 15)), (3, (64, 45)), (4, (221, 125))):
        es = with_aspect(pal_stream, code)
        parsed = R.Parsed(es, 720, 576, 1)
        assert parsed.headers.sequence_header.aspect_ratio_information == code
        assert parsed.headers.have_sequence_display_extension == 0
        assert R.pixel_aspect(parsed.headers) == want
        with R.Scan(es, 720, 576, 1) as scan:
            assert R.pixel_aspect(scan.headers) == want
        shown = R.Parsed(with_display_extension(es, 704, 576), 720, 576, 1).headers
        assert shown.have_sequence_display_extension == 1
        assert (shown.sequence_display_extension.display_horizontal_size,
                shown.sequence_display_extension.display_vertical_size) == (704, 576)
        assert R.pixel_aspect(shown) == PM.pixel_aspect(code, 704, 576)
    assert R.pixel_aspect(R.Parsed(with_display_extension(with_aspect(pal_stream, 2), 704, 576), 720, 576, 1).headers) \
        == (12, 11)
    for code in (0, 5):
        parsed = R.Parsed(with_aspect(pal_stream, code), 720, 576, 1)
        with pytest.raises(_lib.Mp2vgError) as e:
            R.pixel_aspect(parsed.headers)
        assert e.value.status == E_UNSUPPORTED


# ---- validation without a device -------------------------------------------------------------------

def planes_placed(t, place, coded=(64, 64), nbytes=None, cf=3, field=0):
    """mp2vg_tensor_planes_placed on host addresses that are never dereferenced: every argument is
    checked before the first HIP call, so a refusal needs no device.  The status and the reason."""
    buf = np.zeros(8192, np.uint8)
    ptrs = (ctypes.c_void_p * 3)(*[buf.ctypes.data] * 3)
    nbytes = 3 * t.out_w * t.out_h * (1, 2, 2, 4)[t.dtype] if nbytes is None else nbytes
    L = _lib.lib()
    rc = L.mp2vg_tensor_planes_placed(0, ptrs, (ctypes.c_int32 * 3)(64, 64, 64), cf, coded[0], coded[1], field,
                                      ctypes.byref(t), None if place is None else ctypes.byref(place),
                                      ctypes.c_void_p(buf.ctypes.data), nbytes)
    return rc, L.mp2vg_last_error()


def passes_validation(t, place, coded=(64, 64)):
    """The tensor and the placement are accepted: with a dst_bytes that is off by one, the refusal
    is the one about dst_bytes, which is checked after them and before any HIP call (so nothing
    runs, with or without a device)."""
    rc, why = planes_placed(t, place, coded, nbytes=3 * t.out_w * t.out_h * (1, 2, 2, 4)[t.dtype] + 1)
    assert rc == E_INVALID
    return b"dst_bytes" in why


def test_planes_placed_validation_before_any_hip_call():
    t = _lib.make_tensor((24, 21), dtype="uint8")
    assert passes_validation(t, None)
    assert passes_validation(t, _lib.make_place((3, 5, 16, 11), (1, 128, 254)))
    assert passes_validation(t, _lib.make_place((0, 0, 24, 21)))
    assert passes_validation(t, _lib.make_place((22, 19, 2, 2)))
    # each rectangle rule
    for rect in ((-1, 5, 16, 11), (3, -1, 16, 11), (3, 5, 0, 11), (3, 5, 16, 0), (3, 5, -4, 11), (3, 5, 16, -1),
                 (9, 5, 16, 11), (3, 11, 16, 11), (0, 0, 25, 21), (0, 0, 24, 22), (24, 0, 1, 1), (0, 21, 1, 1),
                 (1 << 30, 0, 1 << 30, 1), (0, 0, 0, 21), (0, 0, 24, 0), (1, 0, 0, 0), (0, 1, 0, 0)):
        rc, why = planes_placed(t, _lib.make_place(rect))
        assert rc == E_INVALID and b"placement" in why, rect
        assert not passes_validation(t, _lib.make_place(rect))
    # the ratio is judged on the rectangle, not on the output: 64 into dst_w = 1 is 64:1 although
    # out_w = 64; 64 into 2 is 32:1 and passes with out_w = 2
    wide = _lib.make_tensor((64, 64), dtype="uint8")
    for rect in ((0, 0, 1, 64), (5, 0, 1, 64), (0, 0, 64, 1), (0, 63, 64, 1)):
        rc, why = planes_placed(wide, _lib.make_place(rect))
        assert rc == E_INVALID and b"ratio" in why, rect
    assert passes_validation(wide, _lib.make_place((0, 0, 2, 64)))
    assert passes_validation(wide, _lib.make_place((62, 62, 2, 2)))
    assert passes_validation(_lib.make_tensor((2, 2), dtype="uint8"), _lib.make_place((0, 0, 2, 2)))
    assert passes_validation(_lib.make_tensor((2, 2), dtype="uint8"), None)
    rc, why = planes_placed(_lib.make_tensor((1, 64), dtype="uint8"), None)
    assert rc == E_INVALID and b"ratio" in why
    # the all-zero rectangle is the whole output: judged on out_w, pad ignored
    assert passes_validation(t, _lib.make_place((0, 0, 0, 0), (9, 9, 9)))
    rc, why = planes_placed(_lib.make_tensor((1, 64), dtype="uint8"), _lib.make_place((0, 0, 0, 0)))
    assert rc == E_INVALID and b"ratio" in why
    # reserved fields, of the placement (also with the all-zero rectangle) and of the tensor
    for name, i in (("reserved0", None), ("reserved", 0), ("reserved", 1), ("reserved", 2)):
        for rect in ((3, 5, 16, 11), (0, 0, 0, 0)):
            p = _lib.make_place(rect)
            if i is None:
                p.reserved0 = 1
            else:
                p.reserved[i] = 1
            rc, why = planes_placed(t, p)
            assert rc == E_INVALID and b"reserved" in why, (name, i, rect)
    bad = _lib.make_tensor((24, 21), dtype="uint8")
    bad.reserved[2] = 1
    rc, why = planes_placed(bad, _lib.make_place((3, 5, 16, 11)))
    assert rc == E_INVALID and b"reserved" in why
    # the checks of the entry point it extends still hold: field mode, null pointers, dst size
    assert planes_placed(t, _lib.make_place((3, 5, 16, 11)), field=4)[0] == E_INVALID
    assert planes_placed(t, _lib.make_place((3, 5, 16, 11)), coded=(64, 62), cf=1, field=1)[0] == E_INVALID
    assert planes_placed(t, _lib.make_place((3, 5, 16, 11)), nbytes=3 * 16 * 11)[0] == E_INVALID  # not the rectangle's
    # valid arguments get past the validation: without a device that is a HIP error (with one the
    # call would run: not tried here, the addresses are host memory)
    import torch
    if not torch.cuda.is_available():
        assert planes_placed(t, _lib.make_place((3, 5, 16, 11), (1, 128, 254)))[0] == -3
        assert planes_placed(t, None)[0] == -3


def test_struct_sizes():
    assert ctypes.sizeof(_lib.Place) == 32
    assert ctypes.sizeof(_lib.Tensor) == 80
    assert _lib.Place.pad.offset == 16 and _lib.Place.reserved0.offset == 19 and _lib.Place.reserved.offset == 20
    assert _lib.lib().mp2vg_abi_version() == 2


# ---- the model -------------------------------------------------------------------------------------

def planes(cf, w=16, h=8, seed=1):
    return visible(random_planes(cf, w, h, 64, seed), cf, w, h)


@pytest.mark.parametrize("cf,mode", itertools.product((1, 2, 3), (FM.PROGRESSIVE, FM.TOP, FM.WEAVE)))
def test_model_whole_rectangle_is_the_field_model(cf, mode):
    p = planes(cf, seed=40 + cf)
    s, b = np.array([0.5, 0.25, 2.0], np.float32), np.array([1.0, -2.0, 0.5], np.float32)
    for size, crop, dtype, packed in (((10, 7), None, "uint8", True), ((5, 3), (1, 1, 13, 6), "float16", False)):
        sb = ((1, 1, 1), (0, 0, 0)) if dtype == "uint8" else (s, b)
        want = FM.tensor(p, cf, 1, True, mode, packed, size, crop, dtype, *sb)
        for rect in (None, (0, 0) + size):
            assert np.array_equal(PM.tensor(p, cf, 1, True, mode, packed, size, crop, rect, (7, 8, 9), dtype, *sb), want)


def test_model_pastes_the_picture_of_the_rectangles_size():
    p = planes(1, 16, 8, seed=44)
    q = PM.q_canvas(p, 1, 1, True, FM.TOP, (11, 9), (2, 1, 12, 6), (3, 2, 5, 4), (1, 128, 254))
    assert np.array_equal(q[:, 2:6, 3:8], FM.q_image(p, 1, 1, True, FM.TOP, (5, 4), (2, 1, 12, 6)))
    mask = np.ones((9, 11), bool)
    mask[2:6, 3:8] = False
    for c, v in enumerate((64, 8192, 16256)):
        assert (q[c][mask] == v).all()


def bf16(values):
    """bit patterns of values that bfloat16 holds exactly"""
    u = np.array(values, np.float32).view(np.uint32)
    assert (u & 0xFFFF == 0).all()
    return (u >> 16).astype(np.uint16)


def test_hand_computed_2x2_picture_in_a_4x3_canvas():
    """4:4:4, neutral chroma: luma 16 -> 0, 235 -> 255, 126 -> 128 on every channel (test_field_cpu).
    The 2 x 2 picture at its own size (identity: Q = 64 P) at (1, 0) of a 4 x 3 canvas, pad (1, 128, 254),
    scale (1/2, 1/4, 2), bias (1, -2, 1/2): every value below is p * scale + bias by hand."""
    Y = np.array([[16, 235], [126, 16]], np.uint8)
    p = [Y, np.full_like(Y, 128), np.full_like(Y, 128)]
    pad, rect, size = (1, 128, 254), (1, 0, 2, 2), (4, 3)
    scale, bias = np.array([0.5, 0.25, 2.0], np.float32), np.array([1.0, -2.0, 0.5], np.float32)

    def canvas(padv, pix):  # pix = the values of P = 0, 255, 128
        a, b, c = pix
        return [[padv, a, b, padv], [padv, c, a, padv], [padv] * 4]

    got = PM.tensor(p, 3, 1, False, FM.PROGRESSIVE, False, size, None, rect, pad, "uint8")
    assert got.dtype == np.uint8 and got.tolist() == [canvas(v, (0, 255, 128)) for v in pad]
    f32 = [canvas(1.5, (1.0, 128.5, 65.0)), canvas(30.0, (-2.0, 61.75, 30.0)), canvas(508.5, (0.5, 510.5, 256.5))]
    got = PM.tensor(p, 3, 1, False, FM.PROGRESSIVE, False, size, None, rect, pad, "float32", scale, bias)
    assert np.array_equal(got, np.array(f32, np.float32).view(np.uint32))
    # float16 has 11 significant bits: all of these are exact
    got = PM.tensor(p, 3, 1, False, FM.PROGRESSIVE, False, size, None, rect, pad, "float16", scale, bias)
    assert np.array_equal(got, np.array(f32, np.float16).view(np.uint16))
    # bfloat16 has 8: 128.5 is a tie between 128 and 129 and goes to the even 128; between 256 and 512
    # the step is 2: 508.5 -> 508, 510.5 -> 510, 256.5 -> 256
    b16 = [canvas(1.5, (1.0, 128.0, 65.0)), canvas(30.0, (-2.0, 61.75, 30.0)), canvas(508.0, (0.5, 510.0, 256.0))]
    got = PM.tensor(p, 3, 1, False, FM.PROGRESSIVE, False, size, None, rect, pad, "bfloat16", scale, bias)
    assert np.array_equal(got, bf16(b16).reshape(3, 3, 4))
    # packed: the same values, channel last
    got = PM.tensor(p, 3, 1, False, FM.PROGRESSIVE, True, size, None, rect, pad, "float32", scale, bias)
    assert np.array_equal(got, np.moveaxis(np.array(f32, np.float32), 0, -1).view(np.uint32))


# ---- Python spellings ------------------------------------------------------------------------------

def test_python_placement_spellings():
    # the defaults build the call without a placement
    assert _lib.placement((8, 8), None, (64, 48)) == (None, None)
    assert _lib.placement((8, 8), (1, 2, 3, 4), (64, 48), pad=(9, 9, 9)) == ((1, 2, 3, 4), None)
    with pytest.raises(ValueError):
        _lib.placement((8, 8), None, (64, 48), place=(0, 0, 4, 4), fit="contain")
    crop, pl = _lib.placement((8, 8), (1, 2, 3, 4), (64, 48), place=(2, 1, 4, 5), pad=(1, 128, 254))
    assert crop == (1, 2, 3, 4) and (pl.dst_x, pl.dst_y, pl.dst_w, pl.dst_h) == (2, 1, 4, 5)
    assert list(pl.pad) == [1, 128, 254] and pl.reserved0 == 0 and list(pl.reserved) == [0, 0, 0]
    # fit takes the crop, or else the coded frame, at the pixel aspect given
    crop, pl = _lib.placement((8, 8), None, (64, 32), fit="contain")
    assert crop == (0, 0, 64, 32) and (pl.dst_x, pl.dst_y, pl.dst_w, pl.dst_h) == (0, 2, 8, 4)
    crop, pl = _lib.placement((8, 8), (2, 0, 32, 32), (64, 32), fit="contain", pixel_aspect=(2, 1), pad=(5, 6, 7))
    assert crop == (2, 0, 32, 32) and (pl.dst_x, pl.dst_y, pl.dst_w, pl.dst_h) == (0, 2, 8, 4) and list(pl.pad) == [5, 6, 7]
    crop, pl = _lib.placement((8, 8), None, (64, 32), fit="cover")
    assert crop == (16, 0, 32, 32) and (pl.dst_x, pl.dst_y, pl.dst_w, pl.dst_h) == (0, 0, 8, 8)
    crop, pl = _lib.placement((8, 8), None, (64, 32), fit="stretch")
    assert crop == (0, 0, 64, 32) and (pl.dst_x, pl.dst_y, pl.dst_w, pl.dst_h) == (0, 0, 8, 8)
    for bad in ((1, 2), (0, 0, 256), (-1, 0, 0)):
        with pytest.raises(ValueError):
            _lib.make_place((0, 0, 4, 4), bad)
    with pytest.raises(ValueError):
        _lib.placement((8, 8), None, (64, 32), fit="fill")
    for name in ("mp2vg_tensor_slots_placed", "mp2vg_tensor_planes_placed", "mp2vg_tensor_fit",
                 "mp2vg_stream_pixel_aspect"):
        assert name in _lib.EXPORTS and getattr(_lib.lib(), name).argtypes


def test_python_signatures_keep_their_defaults():
    import inspect
    from tiny_mp2v_dec_amd.decoder import frame_c
    for fn in (R.DeviceContext.export_tensor, frame_c.export_tensor):
        p = inspect.signature(fn).parameters
        assert (p["place"].default, p["fit"].default, p["pixel_aspect"].default, p["pad"].default) == \
            (None, None, (1, 1), (0, 0, 0))
    p = inspect.signature(R.decode_tensor).parameters
    assert (p["fit"].default, p["pad"].default, p["pixel_aspect"].default) == (None, (0, 0, 0), "stream")
