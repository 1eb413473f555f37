"""CPU: the host side of the tensor export (include/mp2vg.h "tensor export") and its numpy
yardstick (tests/tensor_model.py): the integer tap table against the rational model, the model
against torch's antialiased bilinear, the identity, and argument validation before any HIP call."""
import ctypes
import itertools
import math

import numpy as np
import pytest

import export_model
import tensor_model as T
from tiny_mp2v_dec_amd import _lib

OK, E_INVALID, E_HIP = 0, -1, -3


# ---- tap table -------------------------------------------------------------------------------------

def check_axis(src, out):
    first, count, w = _lib.tensor_weights(src, out)
    mf, mc, mw = T.taps(src, out)
    assert np.array_equal(first, mf) and np.array_equal(count, mc), (src, out)
    assert w.shape == mw.shape and np.array_equal(w, mw), (src, out)
    assert (w.sum(axis=1) == 16384).all() and (w >= 0).all(), (src, out)
    assert (first >= 0).all() and (count >= 1).all() and (first + count <= src).all(), (src, out)
    assert count.max() <= 65
    assert all((w[o, count[o]:] == 0).all() for o in range(out))


def test_weights_equal_the_rational_model_1_to_64():
    n = 0
    for src, out in itertools.product(range(1, 65), range(1, 65)):
        if src <= 32 * out:
            check_axis(src, out)
            n += 1
    assert n == 64 * 64 - 32  # only out = 1 with src 33..64 is above 32


@pytest.mark.parametrize("src,out", [(1920, 224), (1088, 224), (3840, 224), (1080, 1080)])
def test_weights_equal_the_rational_model_real_sizes(src, out):
    check_axis(src, out)


def test_weights_extremes_and_rejections():
    first, count, w = _lib.tensor_weights(64, 2)  # the 32:1 ratio: 64 taps wide at most 65
    assert count.max() <= 65 and w.shape[1] == count.max()
    first, count, w = _lib.tensor_weights(7, 7)   # the identity: one tap of full weight
    assert first.tolist() == list(range(7)) and (w.max(axis=1) == 16384).all()
    L = _lib.lib()
    i32p = ctypes.POINTER(ctypes.c_int32)
    f, c, ww = np.zeros(4, np.int32), np.zeros(4, np.int32), np.zeros(4 * 65, np.int32)
    args = (f.ctypes.data_as(i32p), c.ctypes.data_as(i32p), ww.ctypes.data_as(i32p))
    assert L.mp2vg_tensor_weights(33, 1, *args, 65) == E_INVALID   # ratio 33
    assert L.mp2vg_tensor_weights(129, 4, *args, 65) == E_INVALID
    assert L.mp2vg_tensor_weights(128, 4, *args, 65) == OK
    assert L.mp2vg_tensor_weights(0, 4, *args, 65) == E_INVALID
    assert L.mp2vg_tensor_weights(4, 0, *args, 65) == E_INVALID
    assert L.mp2vg_tensor_weights(128, 4, *args, 8) == E_INVALID   # more taps than max_taps
    assert L.mp2vg_tensor_weights(4, 4, None, args[1], args[2], 65) == E_INVALID
    assert L.mp2vg_tensor_weights(4, 4, args[0], None, args[2], 65) == E_INVALID
    assert L.mp2vg_tensor_weights(4, 4, args[0], args[1], None, 65) == E_INVALID


# ---- the model -------------------------------------------------------------------------------------

SHAPES = [((48, 32), (10, 7)), ((47, 31), (47, 31)), ((48, 32), (77, 50)), ((240, 135), (50, 28)),
          ((96, 64), (3, 2)), ((40, 33), (1, 1)), ((16, 16), (5, 16))]


def test_model_against_torch_antialiased_bilinear():
    """Q / 64 against torch's CPU interpolate in float64: at most 1/16 of an 8-bit step (the two
    roundings of 1/128 each plus the weight quantisation)."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(11)
    worst = 0.0
    for (w, h), (ow, oh) in SHAPES:
        P = rng.integers(0, 256, (3, h, w), dtype=np.uint8)
        P[0, 0, :] = 255
        P[1, :, 0] = 0
        ref = torch.nn.functional.interpolate(torch.from_numpy(P.astype(np.float64))[None], size=(oh, ow),
                                              mode="bilinear", antialias=True, align_corners=False)[0].numpy()
        d = float(np.abs(T.resize(P, (ow, oh)) / 64.0 - ref).max())
        print(f"{w}x{h} -> {ow}x{oh}: max |model - torch| = {d:.4f}")
        if (w, h) == (ow, oh):
            assert d == 0.0
        worst = max(worst, d)
    print(f"worst {worst:.4f}")
    assert worst <= 1 / 16


def test_model_identity_is_64_p_and_u8_is_the_rgb_export():
    rng = np.random.default_rng(5)
    for cf, linear in itertools.product((1, 2, 3), (False, True)):
        planes = [rng.integers(0, 256, s, dtype=np.uint8) for s in
                  ((32, 48), (16 if cf == 1 else 32, 48 if cf == 3 else 24), (16 if cf == 1 else 32, 48 if cf == 3 else 24))]
        rgb = export_model.export(planes, cf, 5, linear, False)
        assert np.array_equal(T.q_image(planes, cf, 5, linear, (48, 32)), 64 * rgb.astype(np.int32))
        assert np.array_equal(T.q_image(planes, cf, 5, linear, (16, 9), (5, 3, 16, 9)),
                              64 * rgb[:, 3:12, 5:21].astype(np.int32))
        for packed in (False, True):
            assert np.array_equal(T.tensor(planes, cf, 5, linear, packed, (48, 32)),
                                  export_model.export(planes, cf, 5, linear, packed))


def test_model_lookup_tables():
    """The normalise table against independent spot values, and float16 / bfloat16 rounding
    against numpy / torch on every float32 the table can hold."""
    s, b = T.scale_bias((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    f32 = T.lut(s, b, "float32").view(np.float32)
    for c, q in itertools.product(range(3), (0, 1, 63, 64, 8000, 16319, 16320)):
        exact = q / 64 * float(s[c]) + float(b[c])  # float64: close to, not always equal to, one rounding
        assert abs(float(f32[c, q]) - exact) <= abs(exact) * 2.0 ** -24 + 2.0 ** -149
    for sc, bi in ((s, b), (np.float32([3e36, -0.7, 2.0 ** -140]), np.float32([0.0, 0.1, -2.0 ** -126]))):
        bits32 = T.lut(sc, bi, "float32")  # the table's integer rounding against the rational one
        for c, q in itertools.product(range(3), list(range(0, 16321, 97)) + [16320]):
            assert int(bits32[c, q]) == T._f32_bits(T.F(q, 64) * T.F(float(sc[c])) + T.F(float(bi[c]))), (c, q)
    assert np.array_equal(T.lut(s, b, "float16"), f32.astype(np.float16).view(np.uint16))
    big = T.lut(np.full(3, 1000.0, np.float32), np.full(3, -70000.0, np.float32), "float32").view(np.float32)
    with np.errstate(over="ignore"):
        want = big.astype(np.float16).view(np.uint16)  # overflows to -inf and +inf at the ends
    got = T.lut(np.full(3, 1000.0, np.float32), np.full(3, -70000.0, np.float32), "float16")
    assert np.array_equal(got, want) and (want == 0xFC00).any() and (want == 0x7C00).any()
    tiny = T.lut(np.full(3, 2.0 ** -20, np.float32), np.zeros(3, np.float32), "float16")  # float16 subnormals
    assert np.array_equal(tiny, T.lut(np.full(3, 2.0 ** -20, np.float32), np.zeros(3, np.float32),
                                      "float32").view(np.float32).astype(np.float16).view(np.uint16))
    torch = pytest.importorskip("torch")
    for table in (f32, big):
        want = torch.from_numpy(table.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
        assert np.array_equal(T._f32_to_bf16_bits(table.view(np.uint32)), want)
    assert T._f32_bits(T.F(2) ** 128) == 0x7F800000 and T._f32_bits(-T.F(1, 3)) == int(np.float32(-1 / 3).view(np.uint32))
    assert T._f32_bits(T.F(3, 2 ** 150)) == 2  # subnormal, tie to even: 1.5 quanta -> 2
    assert np.array_equal(T.lut(s, b, "uint8")[1], np.clip((np.arange(16321) + 32) >> 6, 0, 255))


# ---- validation with no device ---------------------------------------------------------------------

def tensor_bytes(cfg, t, n):
    b = ctypes.c_uint64(0)
    rc = _lib.lib().mp2vg_tensor_bytes(ctypes.byref(cfg) if cfg else None, ctypes.byref(t) if t else None, n,
                                       ctypes.byref(b))
    return rc, b.value


def bad_tensors(coded_w, coded_h):
    """Every way an mp2vg_tensor_t can be wrong for a coded_w x coded_h frame."""
    out = []

    def bad(what, **kw):
        t = _lib.make_tensor((16, 8), dtype=kw.pop("dtype") if isinstance(kw.get("dtype"), str) else "float32")
        for k, v in kw.items():
            if k in ("scale", "bias"):
                getattr(t, k)[v[0]] = v[1]
            elif k == "reserved":
                t.reserved[v] = 1
            else:
                setattr(t, k, v)
        out.append((what, t))

    for field, values in (("layout", (-1, 2)), ("chroma", (-1, 2)), ("matrix", (0, 2, 3, 8, -1)), ("dtype", (-1, 4)),
                          ("out_w", (0, -1, 16385)), ("out_h", (0, -1, 16385))):
        for v in values:
            bad(f"{field}={v}", **{field: v})
    bad("ratio 33 (w)", out_w=coded_w // 33)
    bad("ratio above 32 (h)", out_h=(coded_h - 1) // 32)
    for i in range(4):
        bad(f"reserved[{i}]", reserved=i)
    for rect in ((1, 0, coded_w, coded_h), (0, 1, coded_w, coded_h), (0, 0, coded_w + 1, coded_h),
                 (0, 0, coded_w, coded_h + 1), (-1, 0, 8, 8), (0, -1, 8, 8), (0, 0, 8, 0), (0, 0, 0, 8), (1, 1, 0, 0),
                 (coded_w - 3, 0, 4, 4), (0, coded_h - 3, 4, 4), (0, 0, -8, 8)):
        bad(f"rectangle {rect}", **dict(zip(("src_x", "src_y", "src_w", "src_h"), rect)))
    for c, v in itertools.product(range(3), (math.nan, math.inf, -math.inf)):
        bad(f"scale[{c}]={v}", scale=(c, v))
        bad(f"bias[{c}]={v}", bias=(c, v))
    for c in range(3):
        bad(f"U8 scale[{c}]", dtype="uint8", scale=(c, 0.5))
        bad(f"U8 bias[{c}]", dtype="uint8", bias=(c, 1.0))
    return out


def test_tensor_bytes():
    cfg = _lib.make_config(1920, 1088, 1)
    for dtype, elem in (("uint8", 1), ("float16", 2), ("bfloat16", 2), ("float32", 4)):
        assert tensor_bytes(cfg, _lib.make_tensor((224, 224), dtype=dtype), 7) == (OK, 7 * 3 * 224 * 224 * elem)
    assert tensor_bytes(cfg, _lib.make_tensor((640, 360), (0, 0, 1920, 1080)), 256) == (OK, 256 * 3 * 640 * 360 * 2)
    assert tensor_bytes(cfg, _lib.make_tensor((60, 34)), 1) == (OK, 3 * 60 * 34 * 2)     # exactly 32:1
    assert tensor_bytes(cfg, _lib.make_tensor((1, 1), (1919, 1087, 1, 1)), 1) == (OK, 6)
    assert tensor_bytes(cfg, _lib.make_tensor((16384, 16384), dtype="float32"), 65535) == \
        (OK, 65535 * 3 * 16384 * 16384 * 4)                                              # past 2^32
    for bad in (None, _lib.make_config(100, 64, 1), _lib.make_config(176, 144, 4)):
        assert tensor_bytes(bad, _lib.make_tensor((16, 8)), 1)[0] == E_INVALID
    assert tensor_bytes(cfg, None, 1)[0] == E_INVALID
    assert tensor_bytes(cfg, _lib.make_tensor((16, 8)), 0)[0] == E_INVALID
    assert _lib.lib().mp2vg_tensor_bytes(ctypes.byref(cfg), ctypes.byref(_lib.make_tensor((224, 224))), 1, None) == E_INVALID
    for what, t in bad_tensors(176, 144):
        assert tensor_bytes(_lib.make_config(176, 144, 1), t, 1)[0] == E_INVALID, what


def planes_call(planes=(4096, 8192, 12288), stride=(64, 64, 64), cf=1, cw=48, ch=32, t="default", dst=65536,
                dst_bytes=None, device=0, planes_null=False, stride_null=False):
    """mp2vg_tensor_planes with made-up (never dereferenced) device addresses."""
    t = _lib.make_tensor((10, 7), dtype="float32") if t == "default" else t
    if dst_bytes is None:
        dst_bytes = 3 * t.out_w * t.out_h * (1, 2, 2, 4)[t.dtype] if t is not None and 0 <= t.dtype < 4 else 0
    p = None if planes_null else (ctypes.c_void_p * 3)(*planes)
    s = None if stride_null else (ctypes.c_int32 * 3)(*stride)
    return _lib.lib().mp2vg_tensor_planes(device, p, s, cf, cw, ch, ctypes.byref(t) if t is not None else None,
                                          ctypes.c_void_p(dst), dst_bytes)


def test_tensor_planes_validation_happens_before_any_hip_call():
    """Each of these is MP2VG_E_INVALID on a machine without a device (where any HIP call fails)."""
    assert planes_call(planes_null=True) == E_INVALID
    assert planes_call(stride_null=True) == E_INVALID
    assert planes_call(t=None) == E_INVALID
    assert planes_call(dst=0) == E_INVALID
    assert planes_call(planes=(4096, 0, 12288)) == E_INVALID
    assert planes_call(planes=(4096, 8194, 12288)) == E_INVALID
    assert planes_call(stride=(64, 62, 64)) == E_INVALID
    assert planes_call(stride=(44, 64, 64)) == E_INVALID
    assert planes_call(cf=0) == E_INVALID
    assert planes_call(cf=4) == E_INVALID
    assert planes_call(cw=0) == E_INVALID
    assert planes_call(cw=47) == E_INVALID                             # odd size, subsampled chroma
    assert planes_call(device=-1) == E_INVALID
    assert planes_call(dst_bytes=3 * 10 * 7 * 4 - 1) == E_INVALID      # not n 3 w h elemsize
    assert planes_call(dst_bytes=3 * 10 * 7 * 2) == E_INVALID
    assert planes_call(dst=65538) == E_INVALID                         # float32 at a 2-byte address
    assert planes_call(t=_lib.make_tensor((10, 7), dtype="float16"), dst=65537) == E_INVALID
    assert planes_call(t=_lib.make_tensor((1, 1), dtype="float32"), ch=34) == E_INVALID   # 34:1
    for what, t in bad_tensors(48, 32):
        assert planes_call(t=t) == E_INVALID, what


def test_tensor_slots_rejects_bad_arguments_without_a_context():
    t = _lib.make_tensor((10, 7))
    slots = (ctypes.c_int32 * 1)(0)
    assert _lib.lib().mp2vg_tensor_slots(None, slots, 1, ctypes.byref(t), ctypes.c_void_p(65536), 3 * 10 * 7 * 2) == E_INVALID


def test_make_tensor_spelling():
    t = _lib.make_tensor((224, 200), (5, 3, 160, 90), "bfloat16", (0.5, 0.25, 0.125), (0.5, 0.25, 2.0), "nhwc", "nearest", 7)
    assert (t.layout, t.matrix, t.chroma, t.src_x, t.src_y, t.src_w, t.src_h, t.out_w, t.out_h, t.dtype) == \
        (1, 7, 0, 5, 3, 160, 90, 224, 200, 2)
    assert list(t.scale) == [np.float32(1 / (255 * s)) for s in (0.5, 0.25, 2.0)]
    assert list(t.bias) == [-1.0, -1.0, -0.0625] and list(t.reserved) == [0] * 4
    assert _lib.tensor_shape(t, 5) == (5, 200, 224, 3)
    s, b = T.scale_bias((0.5, 0.25, 0.125), (0.5, 0.25, 2.0))
    assert list(t.scale) == list(s) and list(t.bias) == list(b)
    t = _lib.make_tensor((8, 4))
    assert list(t.scale) == [np.float32(1 / 255)] * 3 and list(t.bias) == [0.0] * 3 and t.dtype == 1
    assert _lib.tensor_shape(t, 2) == (2, 3, 4, 8)
    t = _lib.make_tensor((8, 4), dtype="uint8")
    assert list(t.scale) == [1.0] * 3 and list(t.bias) == [0.0] * 3
    for kw in (dict(dtype="float64"), dict(mean=(0, 0, 0)), dict(dtype="uint8", mean=(0, 0, 0), std=(1, 1, 1)),
               dict(mean=(0, 0), std=(1, 1)), dict(layout="chw")):
        with pytest.raises(ValueError):
            _lib.make_tensor((8, 4), **kw)
    assert ctypes.sizeof(_lib.Tensor) == 80


def test_no_cpu_fallback_without_gpu():
    """A valid tensor export on a machine without a device is a HIP error, never a CPU resize."""
    try:
        import torch
        if torch.cuda.is_available():
            pytest.skip("a GPU is present")
    except ImportError:
        pass
    assert planes_call() == E_HIP
