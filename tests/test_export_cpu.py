"""CPU: the host side of the RGB export (include/mp2vg.h "RGB export") and its numpy yardstick
(tests/export_model.py): coefficients, stream matrix choice, sizes, argument validation before any
HIP call, and no CPU fallback."""
import ctypes
import itertools

import numpy as np
import pytest

import export_model as M
from tiny_mp2v_dec_amd import _lib

OK, E_INVALID, E_UNSUPPORTED, E_HIP = 0, -1, -2, -3

# (cy, crv, cgu, cgv, cbu) per matrix_coefficients code, as published with the contract
TABLE = {1: (19077, 29372, -3494, -8731, 34610),
         4: (19077, 26112, -6190, -13277, 33200),
         5: (19077, 26149, -6419, -13320, 33050),
         6: (19077, 26149, -6419, -13320, 33050),
         7: (19077, 29395, -4227, -8890, 34058)}


def lib_coefficients(matrix):
    out = (ctypes.c_int32 * 5)()
    rc = _lib.lib().mp2vg_export_coefficients(matrix, out)
    return rc, tuple(out)


@pytest.mark.parametrize("matrix", M.MATRICES)
def test_coefficients_equal_the_rational_derivation(matrix):
    assert M.coefficients(matrix) == TABLE[matrix]
    assert lib_coefficients(matrix) == (OK, TABLE[matrix])


@pytest.mark.parametrize("matrix", [-1, 0, 2, 3, 8, 9, 255])
def test_coefficients_reject_other_codes(matrix):
    assert lib_coefficients(matrix)[0] == E_INVALID
    assert _lib.lib().mp2vg_export_coefficients(1, None) == E_INVALID


def const_planes(cf, y, cb, cr, w=16, h=8):
    cw, ch = (w if cf == 3 else w // 2), (h // 2 if cf == 1 else h)
    return [np.full((h, w), y, np.uint8), np.full((ch, cw), cb, np.uint8), np.full((ch, cw), cr, np.uint8)]


@pytest.mark.parametrize("cf,linear", itertools.product((1, 2, 3), (False, True)))
def test_model_landmarks(cf, linear):
    for matrix in M.MATRICES:
        for (y, want) in ((16, 0), (235, 255), (126, 128)):
            for packed in (False, True):
                got = M.export(const_planes(cf, y, 128, 128), cf, matrix, linear, packed, (15, 7))
                assert got.shape == ((7, 15, 3) if packed else (3, 7, 15))
                assert (got == want).all(), (matrix, y)
    # constant chroma: the LINEAR taps reproduce it, so LINEAR equals NEAREST whatever the luma
    rng = np.random.default_rng(7)
    planes = const_planes(cf, 0, 77, 201)
    planes[0] = rng.integers(0, 256, planes[0].shape, dtype=np.uint8)
    assert np.array_equal(M.export(planes, cf, 5, linear, False), M.export(planes, cf, 5, False, False))


def test_model_linear_taps_by_hand():
    """4:2:0 LINEAR on a 4 x 4 frame, worked out by hand from the contract."""
    C = np.array([[0, 80], [160, 240]], np.uint8)
    got = M.chroma_at(C, 1, True, 4, 4)
    # rows: y = 0 (j 0, j1 clamps to 0), 1 (j 0, j1 1), 2 (j 1, j1 0), 3 (j 1, j1 clamps to 1)
    # columns: x = 0 (k 0), 1 (k 0, k1 1), 2 (k 1), 3 (k 1, k1 clamps to 1)
    col = lambda a, b: [(2 * a + 4) >> 3, (a + b + 4) >> 3, (2 * b + 4) >> 3, (2 * b + 4) >> 3]  # noqa: E731
    want = [col(4 * 0, 4 * 80), col(3 * 0 + 160, 3 * 80 + 240), col(3 * 160 + 0, 3 * 240 + 80), col(4 * 160, 4 * 240)]
    assert got.tolist() == want
    assert M.chroma_at(C, 1, False, 4, 4).tolist() == [[0, 0, 80, 80]] * 2 + [[160, 160, 240, 240]] * 2


def test_model_variants_differ():
    """Every (matrix, chroma mode) variant differs from every other in a large share of the pixels
    of random input, so a wrong table or mode cannot pass the parity tests."""
    rng = np.random.default_rng(3)
    planes = [rng.integers(0, 256, s, dtype=np.uint8) for s in ((32, 48), (16, 24), (16, 24))]
    outs = {(m, lin): M.export(planes, 1, m, lin, True) for m in (1, 4, 5, 7) for lin in (False, True)}
    for a, b in itertools.combinations(outs, 2):
        assert (outs[a] != outs[b]).any(axis=-1).mean() > 0.15, (a, b)


def headers(ext=True, desc=1, code=1):
    h = _lib.StreamHeaders()
    h.have_sequence_display_extension = 1 if ext else 0
    h.sequence_display_extension.colour_description = desc
    h.sequence_display_extension.matrix_coefficients = code
    return h


def export_matrix(h):
    m = ctypes.c_int32(-99)
    rc = _lib.lib().mp2vg_export_matrix(ctypes.byref(h), ctypes.byref(m))
    return rc, m.value


def test_export_matrix_from_stream_headers():
    assert export_matrix(headers(ext=False, code=5)) == (OK, 1)   # no sequence display extension
    assert export_matrix(headers(desc=0, code=5)) == (OK, 1)      # no colour description
    for code in range(9):
        rc, m = export_matrix(headers(code=code))
        if code in (1, 4, 5, 6, 7):
            assert (rc, m) == (OK, code)
        elif code == 2:
            assert (rc, m) == (OK, 1)
        else:
            assert rc == E_UNSUPPORTED, code
    L = _lib.lib()
    assert L.mp2vg_export_matrix(None, ctypes.byref(ctypes.c_int32())) == E_INVALID
    assert L.mp2vg_export_matrix(ctypes.byref(headers()), None) == E_INVALID


def export_bytes(cfg, exp, n):
    b = ctypes.c_uint64(0)
    rc = _lib.lib().mp2vg_export_bytes(ctypes.byref(cfg) if cfg else None, ctypes.byref(exp) if exp else None, n,
                                       ctypes.byref(b))
    return rc, b.value


def test_export_bytes():
    cfg = _lib.make_config(1920, 1088, 1)
    assert export_bytes(cfg, _lib.make_export(), 7) == (OK, 7 * 3 * 1920 * 1088)
    assert export_bytes(cfg, _lib.make_export("nhwc", "nearest", 5, (1920, 1080)), 256) == (OK, 256 * 3 * 1920 * 1080)
    assert export_bytes(cfg, _lib.make_export(size=(1, 1)), 1) == (OK, 3)
    assert export_bytes(cfg, _lib.make_export(size=(0, 1080)), 1) == (OK, 3 * 1920 * 1080)  # 0 = coded
    big = _lib.make_config(4096, 4096, 3)
    assert export_bytes(big, _lib.make_export(), 60000) == (OK, 60000 * 3 * 4096 * 4096)  # past 2^32
    for bad in (None, _lib.make_config(100, 64, 1), _lib.make_config(176, 144, 4)):
        assert export_bytes(bad, _lib.make_export(), 1)[0] == E_INVALID
    assert export_bytes(cfg, None, 1)[0] == E_INVALID
    assert export_bytes(cfg, _lib.make_export(), 0)[0] == E_INVALID
    assert export_bytes(cfg, _lib.make_export(), -3)[0] == E_INVALID
    assert _lib.lib().mp2vg_export_bytes(ctypes.byref(cfg), ctypes.byref(_lib.make_export()), 1, None) == E_INVALID


def bad_exports(coded_w, coded_h):
    """Every way an mp2vg_export_t can be wrong for a coded_w x coded_h frame."""
    out = []
    for field, values in (("layout", (-1, 2)), ("chroma", (-1, 2)), ("matrix", (0, 2, 3, 8, -1)),
                          ("width", (-1, coded_w + 1)), ("height", (-1, coded_h + 1))):
        for v in values:
            e = _lib.make_export()
            setattr(e, field, v)
            out.append((f"{field}={v}", e))
    for i in range(3):
        e = _lib.make_export()
        e.reserved[i] = 1
        out.append((f"reserved[{i}]", e))
    return out


def test_export_bytes_validates_the_export():
    cfg = _lib.make_config(176, 144, 1)
    for what, e in bad_exports(176, 144):
        assert export_bytes(cfg, e, 1)[0] == E_INVALID, what


def planes_call(planes=(4096, 8192, 12288), stride=(64, 64, 64), cf=1, cw=48, ch=32, exp="default", dst=65536,
                dst_bytes=None, device=0, planes_null=False, stride_null=False):
    """mp2vg_export_planes with made-up (never dereferenced) device addresses."""
    e = _lib.make_export() if exp == "default" else exp
    if dst_bytes is None:
        dst_bytes = 3 * ((e.width if e else 0) or cw) * ((e.height if e else 0) or ch)
    p = None if planes_null else (ctypes.c_void_p * 3)(*planes)
    s = None if stride_null else (ctypes.c_int32 * 3)(*stride)
    return _lib.lib().mp2vg_export_planes(device, p, s, cf, cw, ch, ctypes.byref(e) if e else None,
                                          ctypes.c_void_p(dst), dst_bytes)


def test_export_planes_validation_happens_before_any_hip_call():
    """Each of these is MP2VG_E_INVALID on a machine without a device (where any HIP call fails)."""
    assert planes_call(planes_null=True) == E_INVALID
    assert planes_call(stride_null=True) == E_INVALID
    assert planes_call(exp=None) == E_INVALID
    assert planes_call(dst=0) == E_INVALID
    assert planes_call(planes=(4096, 0, 12288)) == E_INVALID          # a null plane
    assert planes_call(planes=(4096, 8194, 12288)) == E_INVALID       # plane not 4-byte aligned
    assert planes_call(stride=(64, 62, 64)) == E_INVALID              # stride not a multiple of 4
    assert planes_call(stride=(44, 64, 64)) == E_INVALID              # stride below the plane width
    assert planes_call(stride=(64, 64, 20)) == E_INVALID
    assert planes_call(cf=0) == E_INVALID
    assert planes_call(cf=4) == E_INVALID
    assert planes_call(cw=0) == E_INVALID
    assert planes_call(ch=-2) == E_INVALID
    assert planes_call(device=-1) == E_INVALID
    assert planes_call(dst_bytes=3 * 48 * 32 - 1) == E_INVALID        # wrong dst_bytes
    assert planes_call(dst_bytes=3 * 48 * 32 + 1) == E_INVALID
    assert planes_call(exp=_lib.make_export(size=(45, 29)), dst_bytes=3 * 48 * 32) == E_INVALID
    for what, e in bad_exports(48, 32):
        assert planes_call(exp=e, dst_bytes=3 * 48 * 32) == E_INVALID, what


def test_export_slots_rejects_bad_arguments_without_a_context():
    L = _lib.lib()
    e = _lib.make_export()
    slots = (ctypes.c_int32 * 1)(0)
    assert L.mp2vg_export_slots(None, slots, 1, ctypes.byref(e), ctypes.c_void_p(65536), 3 * 48 * 32) == E_INVALID


def test_make_export_spelling():
    e = _lib.make_export("nhwc", "nearest", 7, (170, 139))
    assert (e.layout, e.chroma, e.matrix, e.width, e.height, list(e.reserved)) == (1, 0, 7, 170, 139, [0, 0, 0])
    assert _lib.export_shape(e, 5, 176, 144) == (5, 139, 170, 3)
    assert _lib.export_shape(_lib.make_export(), 2, 176, 144) == (2, 3, 144, 176)
    with pytest.raises(ValueError):
        _lib.make_export(layout="chw")
    with pytest.raises(ValueError):
        _lib.make_export(chroma="cubic")
    assert ctypes.sizeof(_lib.Export) == 32


def test_no_cpu_fallback_without_gpu():
    """A valid export on a machine without a device is a HIP error, never a CPU conversion."""
    try:
        import torch
        if torch.cuda.is_available():
            pytest.skip("a GPU is present")
    except ImportError:
        pass
    assert planes_call() == E_HIP
    assert planes_call(cf=3, stride=(48, 48, 48), exp=_lib.make_export("nhwc", "nearest", 7, (45, 29))) == E_HIP
