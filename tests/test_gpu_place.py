"""GPU: the placed tensor export (tensor.hip, PLACED) through mp2vg_tensor_planes_placed,
mp2vg_tensor_slots_placed and the Python interface.  Every comparison is array_equal on bit patterns
against the numpy model (tests/place_model.py).  Every destination is prefilled with FILL and has
guard bytes on both sides, so an element of the canvas nobody wrote and a write outside it both show;
pad colours, scales and biases differ per channel."""
import ctypes
import itertools

import numpy as np
import pytest

import field_model as FM
import place_model as PM
import tensor_model as T
from conftest import load_manifest, read_stream
from test_gpu_export import FILL, GUARD, decoded_frames, gop, host_frames, random_planes
from test_gpu_field import FieldSource
from test_gpu_tensor import IMAGENET, NORM
from tiny_mp2v_dec_amd import _lib
from tiny_mp2v_dec_amd import records as R
from tiny_mp2v_dec_amd.decoder import decoder_config_t, mp2v_decoder_c

pytestmark = pytest.mark.gpu

E_INVALID = -1
PAD = (1, 128, 254)
ELEM = {"uint8": 1, "float16": 2, "bfloat16": 2, "float32": 4}
INT = {1: "uint8", 2: "int16", 4: "int32"}


class PlaceSource(FieldSource):
    """test_gpu_field.FieldSource through mp2vg_tensor_planes_placed; the model's Q image of each
    (matrix, chroma, mode, rectangle size, crop) is computed once and shared."""

    def call_placed(self, t, field, place, offset=0):
        torch = self.torch
        elem = (1, 2, 2, 4)[t.dtype]
        nbytes = 3 * t.out_w * t.out_h * elem
        buf = torch.full((GUARD + 16 + nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        at = GUARD + offset * elem
        ptrs = (ctypes.c_void_p * 3)(*[x.data_ptr() for x in self.t])
        rc = _lib.lib().mp2vg_tensor_planes_placed(0, ptrs, (ctypes.c_int32 * 3)(*self.stride), self.cf, self.cw,
                                                   self.ch, field, ctypes.byref(t),
                                                   None if place is None else ctypes.byref(place),
                                                   ctypes.c_void_p(buf.data_ptr() + at), nbytes)
        got = buf.cpu().numpy()
        clean = (got[:at] == FILL).all() and (got[at + nbytes:] == FILL).all()
        return rc, got[at:at + nbytes], clean

    def check_placed(self, size, rect, mode="progressive", crop=None, dtype="uint8", mean=None, std=None, layout="nchw",
                     chroma="linear", matrix=1, pad=PAD, offset=0):
        t = _lib.make_tensor(size, crop, dtype, mean, std, layout, chroma, matrix)
        what = (self.cf, size, rect, mode, crop, dtype, layout, chroma, matrix, offset)
        rc, got, clean = self.call_placed(t, FM.MODES[mode], _lib.make_place(rect, pad), offset)
        assert rc == 0, (what, _lib.lib().mp2vg_last_error())
        q = PM.paste(self.field_q(matrix, chroma, mode, (rect[2], rect[3]), crop), size, rect, pad)
        want = T.normalise(q, dtype, np.array(t.scale, np.float32), np.array(t.bias, np.float32))
        if layout == "nhwc":
            want = np.moveaxis(want, 0, -1)
        assert np.array_equal(T.bits(got, dtype).reshape(want.shape), want), what
        assert clean, ("bytes outside dst written", what)

    def check_both(self, size, rect, **kw):
        """uint8 packed and normalised float16 planar"""
        self.check_placed(size, rect, dtype="uint8", layout="nhwc", **kw)
        self.check_placed(size, rect, dtype="float16", mean=IMAGENET[0], std=IMAGENET[1], layout="nchw", **kw)


def source(cf, w=32, h=16, seed=700):
    return PlaceSource(random_planes(cf, w, h, (w + 63) // 64 * 64, seed=seed + cf), cf, w, h)


# ---- mp2vg_tensor_planes_placed --------------------------------------------------------------------

@pytest.mark.parametrize("cf,mode", itertools.product((1, 2, 3), ("progressive", "top", "weave")))
def test_no_placement_is_the_old_entry_point(cf, mode):
    """place = NULL and the all-zero rectangle (its pad never written) both equal
    mp2vg_tensor_planes_field byte for byte; so does the rectangle that is the whole output."""
    src = source(cf)
    for chroma, dtype, size, crop in itertools.product(("nearest", "linear"), ("uint8", "float16"), ((24, 21), (32, 16)),
                                                       (None, (1, 1, 29, 14))):
        t = _lib.make_tensor(size, crop, dtype, *NORM[dtype], chroma=chroma)
        rc0, old, clean0 = src.call_field(t, FM.MODES[mode])
        assert rc0 == 0 and clean0
        for place in (None, _lib.make_place((0, 0, 0, 0), PAD), _lib.make_place((0, 0) + size, PAD)):
            rc1, new, clean1 = src.call_placed(t, FM.MODES[mode], place)
            assert rc1 == 0 and clean1 and np.array_equal(old, new), (cf, mode, chroma, dtype, size, crop)


# (canvas, rectangle): which rows of a workgroup's pair are picture rows
STRADDLES = {
    "pad|first .. last|picture (dst_y odd, dst_h odd)": ((24, 21), (3, 5, 16, 11)),
    "pad|first .. last|pad (dst_y odd, dst_h even)": ((24, 21), (3, 5, 16, 10)),
    "first|second .. last|pad (dst_y even, dst_h odd)": ((24, 21), (3, 4, 16, 11)),
    "whole pairs (dst_y even, dst_h even)": ((24, 21), (3, 4, 16, 12)),
    "one row, the upper of its pair": ((24, 21), (3, 6, 16, 1)),
    "one row, the lower of its pair": ((24, 21), (3, 7, 16, 1)),
    "odd out_h, the single last row is pad": ((24, 21), (3, 9, 16, 11)),
    "odd out_h, the single last row is picture": ((24, 21), (3, 10, 16, 11)),
    "odd out_h, the single last row is the only picture row": ((24, 21), (3, 20, 16, 1)),
    "out_h = 1": ((24, 1), (3, 0, 16, 1)),
    "out_h = 2, pad above": ((24, 2), (3, 1, 16, 1)),
    "first rows": ((24, 21), (3, 0, 16, 3)),
}


@pytest.mark.parametrize("case", sorted(STRADDLES))
def test_row_pair_straddles(case):
    size, rect = STRADDLES[case]
    src = source(1)
    src.check_both(size, rect)
    src.check_both(size, rect, crop=(1, 1, 29, 14), chroma="nearest")


def test_columns():
    """dst_x 0..4 (every alignment of the row's stores), one column, the picture flush to each edge
    of the canvas, and the canvas all picture but for one pad column or one pad row."""
    src = source(1)
    for x in range(5):
        src.check_both((24, 9), (x, 2, 16, 5))
    for rect in ((0, 2, 1, 5), (11, 2, 1, 5), (23, 2, 1, 5),                    # dst_w = 1
                 (0, 0, 16, 5), (8, 0, 16, 5), (0, 4, 16, 5), (8, 4, 16, 5),    # the corners
                 (0, 2, 24, 5), (4, 0, 16, 9),                                  # full width, full height
                 (1, 0, 23, 9), (0, 0, 23, 9), (0, 1, 24, 8), (0, 0, 24, 8)):   # one pad column / row
        src.check_both((24, 9), rect)


@pytest.mark.parametrize("cf", (1, 2, 3))
def test_dtypes_layouts_and_chroma_modes(cf):
    src = source(cf, seed=720)
    for dtype, layout, chroma in itertools.product(T.DTYPES, ("nchw", "nhwc"), ("nearest", "linear")):
        src.check_placed((24, 21), (3, 5, 16, 10), "progressive", (1, 1, 29, 14), dtype, *NORM[dtype], layout=layout,
                         chroma=chroma, matrix=5 if dtype == "bfloat16" else 1, offset=1 if layout == "nhwc" else 0)


def test_ratios_into_the_rectangle():
    """32:1 on both axes into the rectangle (the output itself is larger: the ratio rule is the
    rectangle's), and upscaling."""
    src = PlaceSource(random_planes(1, 64, 64, 64, seed=731), 1, 64, 64)
    src.check_both((7, 5), (3, 1, 2, 2))
    src.check_both((7, 5), (0, 3, 2, 2), chroma="nearest")
    # refused before anything is written: 64 into a rectangle 1 wide, although out_w = 7
    t = _lib.make_tensor((7, 5), dtype="uint8")
    rc, got, clean = src.call_placed(t, 0, _lib.make_place((3, 1, 1, 2), PAD))
    assert rc == E_INVALID and clean and (got == FILL).all()
    up = PlaceSource(random_planes(2, 8, 8, 64, seed=732), 2, 8, 8)
    up.check_both((23, 17), (2, 3, 20, 12))
    up.check_both((23, 17), (3, 5, 20, 12), mode="bottom")


def test_more_than_one_segment():
    """A 4:4:4 source 4112 wide into a picture 2100 wide at dst_x = 3 of a canvas 2110 wide: the taps
    of a row do not fit one window of 2048 source columns, so the left pad, the seam between the
    segments and the right pad are written by different workgroups."""
    cw = 4112
    src = PlaceSource(random_planes(3, cw, 4, cw + 48, seed=741), 3, cw, 4)
    first, count, _ = _lib.tensor_weights(cw, 2100)
    assert int(first[-1] + count[-1] - first[0]) > 2048
    src.check_placed((2110, 5), (3, 1, 2100, 3), dtype="uint8", layout="nhwc")
    src.check_placed((2110, 4), (3, 1, 2100, 2), dtype="float32", mean=IMAGENET[0], std=IMAGENET[1], layout="nchw")


@pytest.mark.parametrize("mode", ("top", "bottom", "weave"))
def test_field_modes_with_placement(mode):
    src = source(1, 16, 8, seed=750)
    for chroma in ("nearest", "linear"):
        src.check_both((20, 11), (2, 3, 16, 8), mode=mode, chroma=chroma)   # identity size: the source image itself
        src.check_both((20, 11), (1, 1, 10, 5), mode=mode, chroma=chroma)
        src.check_both((20, 11), (3, 5, 12, 6), mode=mode, chroma=chroma, crop=(1, 1, 14, 6))


# ---- mp2vg_tensor_slots_placed ---------------------------------------------------------------------

def golden(name):
    e = next(m for m in load_manifest() if m["name"] == name)
    return read_stream(e), e["width"], e["height"], e["chroma_format"]


def slots_placed(ctx, slots, fields, t, place, buf, nbytes):
    s = np.asarray(slots, np.int32)
    i32p = ctypes.POINTER(ctypes.c_int32)
    f = None if fields is None else np.asarray(fields, np.int32)
    return _lib.lib().mp2vg_tensor_slots_placed(ctx.h, s.ctypes.data_as(i32p), None if f is None else f.ctypes.data_as(i32p),
                                                len(s), ctypes.byref(t), None if place is None else ctypes.byref(place),
                                                ctypes.c_void_p(buf.data_ptr() + GUARD), nbytes)


def test_slots_one_launch_over_a_golden_field_stream():
    """The smallest field-coded golden stream: one launch whose list repeats a slot and mixes all
    four modes, letterboxed (CONTAIN) for pixels of 64:45, against the model over the frames the
    context holds.  The Python spelling gives the same bytes; a bad rectangle is refused with
    nothing written and the context still usable."""
    import torch
    fields = [e for e in load_manifest() if e["name"].endswith("_field")]
    name = min(fields, key=lambda e: e["width"] * e["height"] * (1, 2, 3)[e["chroma_format"] - 1])["name"]
    es, w, h, cf = golden(name)
    parsed = R.Parsed(es, w, h, cf)
    assert parsed.npics >= 3
    slots = [int(d) for d in parsed.display[:4]] + [int(parsed.display[1])]
    modes = [1, 2, 3, 0, 1]
    size, par = (40, 40), (64, 45)
    crop, rect = PM.fit("contain", (0, 0, w, h), par, size)
    assert rect[1] > 0 and rect[2] == 40 and rect[3] < 40 and crop == (0, 0, w, h)
    assert _lib.tensor_fit("contain", (0, 0, w, h), par, size) == (crop, rect)
    t = _lib.make_tensor(size, crop, "float16", *IMAGENET, layout="nchw", chroma="linear", matrix=5)
    nbytes = len(slots) * 3 * size[0] * size[1] * 2
    with R.DeviceContext(w, h, cf, slots=parsed.npics) as ctx:
        ctx.upload(parsed.pics, parsed.mbs, parsed.coefs)
        ctx.decode()
        buf = torch.full((GUARD + nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        for bad in ((0, rect[1], 41, rect[3]), (0, -1, 40, 10), (0, 0, 40, 41)):
            assert slots_placed(ctx, slots, modes, t, _lib.make_place(bad, PAD), buf, nbytes) == E_INVALID
        ctx.synchronize()
        assert (buf.cpu().numpy() == FILL).all()
        assert slots_placed(ctx, slots, modes, t, _lib.make_place(rect, PAD), buf, nbytes) == 0
        ctx.synchronize()
        got = buf.cpu().numpy()
        named = ctx.export_tensor(slots, size, dtype="float16", mean=IMAGENET[0], std=IMAGENET[1], matrix=5,
                                  fields=modes, fit="contain", pixel_aspect=par, pad=PAD)
        placed = ctx.export_tensor(slots, size, dtype="float16", mean=IMAGENET[0], std=IMAGENET[1], matrix=5,
                                   fields=modes, place=rect, pad=PAD)
        frames = {s: ctx.download(s) for s in set(slots)}
    assert (got[:GUARD] == FILL).all() and (got[GUARD + nbytes:] == FILL).all()
    s, b = T.scale_bias(*IMAGENET, "float16")
    want = np.stack([PM.tensor(frames[k], cf, 5, True, f, False, size, crop, rect, PAD, "float16", s, b)
                     for k, f in zip(slots, modes)])
    assert np.array_equal(T.bits(got[GUARD:GUARD + nbytes], "float16").reshape(want.shape), want)
    assert np.array_equal(T.bits(named.view(torch.int16).cpu().numpy(), "float16"), want)
    assert np.array_equal(T.bits(placed.view(torch.int16).cpu().numpy(), "float16"), want)
    # the repeated slot in another mode is another picture
    assert not np.array_equal(want[1], want[4])


def test_slots_placed_export_then_a_batch_that_overwrites_the_slots():
    """decode A, placed export of A's slots, decode B into the same slots, one synchronise: the export
    read A's frames (it shares the events of the exports it extends, so the batch waits for it).
    The export is long: its slot list repeats 512 times.  uint8, the picture at its own size: the
    RGB export's bytes inside the rectangle, the pad colour around it."""
    import torch
    import export_model
    a, b = gop(1, seed=951), gop(1, seed=952)
    assert a.npics == b.npics
    frames_a, frames_b = decoded_frames(a), decoded_frames(b)
    assert not np.array_equal(frames_a[0][0], frames_b[0][0])
    slots = np.tile(np.arange(a.npics, dtype=np.int32), 512)
    size, rect = (180, 149), (3, 5, 176, 144)
    with R.DeviceContext(176, 144, 1, slots=a.npics) as ctx:
        out_a = torch.full((len(slots), size[1], size[0], 3), FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.upload(a.pics, a.mbs, a.coefs)
        ctx.decode()
        ctx.export_tensor(slots, size, dtype="uint8", layout="nhwc", out=out_a, sync=False, place=rect, pad=PAD)
        ctx.upload(b.pics, b.mbs, b.coefs)
        ctx.decode()
        ctx.synchronize()
        after = ctx.export_tensor(np.arange(a.npics, dtype=np.int32), size, dtype="uint8", layout="nhwc", place=rect,
                                  pad=PAD)

    def canvases(frames):
        want = np.empty((a.npics, size[1], size[0], 3), np.uint8)
        want[:] = np.array(PAD, np.uint8)
        for k in range(a.npics):
            want[k, rect[1]:rect[1] + rect[3], rect[0]:rect[0] + rect[2]] = export_model.export(frames[k], 1, 1, True, True)
        return torch.from_numpy(want).cuda()

    idx = torch.from_numpy(slots.astype(np.int64)).cuda()
    assert torch.equal(out_a, canvases(frames_a)[idx])
    assert torch.equal(after, canvases(frames_b))


# ---- Python interface ------------------------------------------------------------------------------

def with_aspect(es, code):
    es = bytearray(es)
    at = es.find(b"\x00\x00\x01\xb3")
    es[at + 7] = (code << 4) | (es[at + 7] & 0x0F)  # aspect_ratio_information: the high nibble of byte 7
    return bytes(es)


def test_decode_tensor_fit_takes_the_streams_pixel_aspect():
    import torch
    import tiny_mp2v_dec_amd
    es = with_aspect(R.generate_es(width=64, height=48, chroma_format=1, n_gops=1, gop_n=6, gop_m=3, seed=811), 3)
    parsed = R.Parsed(es, 64, 48, 1)
    par = R.pixel_aspect(parsed.headers)
    assert par == PM.pixel_aspect(3, 64, 48) == (4, 3)          # 64 x 48 shown at 16:9
    frames, _ = host_frames(es, 64, 48, 1)
    size = (40, 40)
    s, b = T.scale_bias(*IMAGENET, "float16")
    for fit in ("contain", "cover"):
        crop, rect = PM.fit(fit, (0, 0, 64, 48), par, size)
        assert (rect == (0, 8, 40, 23)) if fit == "contain" else (crop == (14, 0, 36, 48) and rect == (0, 0, 40, 40))
        out = tiny_mp2v_dec_amd.decode_tensor(es, 64, 48, 1, size, mean=IMAGENET[0], std=IMAGENET[1], fit=fit, pad=PAD)
        assert out.dtype == torch.float16 and tuple(out.shape) == (len(frames), 3, 40, 40)
        want = np.stack([PM.tensor(p, 1, 1, True, FM.PROGRESSIVE, False, size, crop, rect, PAD, "float16", s, b)
                         for p in frames])
        assert np.array_equal(T.bits(out.view(torch.int16).cpu().numpy(), "float16"), want), fit
    # a pixel aspect given by the caller overrides the stream's; a crop is the rectangle that is fitted
    crop, rect = PM.fit("contain", (4, 2, 50, 20), (1, 1), size)
    out = tiny_mp2v_dec_amd.decode_tensor(es, 64, 48, 1, size, crop=(4, 2, 50, 20), dtype="uint8", layout="nhwc",
                                          fit="contain", pad=PAD, pixel_aspect=(1, 1), fields="top", device_parse=True)
    want = np.stack([PM.tensor(p, 1, 1, True, FM.TOP, True, size, crop, rect, PAD, "uint8") for p in frames])
    assert np.array_equal(out.cpu().numpy(), want)
    # without fit the result is the one from before placements existed (pad and pixel_aspect unused)
    plain = tiny_mp2v_dec_amd.decode_tensor(es, 64, 48, 1, size, mean=IMAGENET[0], std=IMAGENET[1])
    same = tiny_mp2v_dec_amd.decode_tensor(es, 64, 48, 1, size, mean=IMAGENET[0], std=IMAGENET[1], fit=None, pad=PAD)
    want = np.stack([T.tensor(p, 1, 1, True, False, size, (0, 0, 64, 48), "float16", s, b) for p in frames])
    assert np.array_equal(T.bits(plain.view(torch.int16).cpu().numpy(), "float16"), want) and plain.equal(same)
    # an aspect code that gives no pixel aspect is an error, not a guess
    with pytest.raises(_lib.Mp2vgError):
        tiny_mp2v_dec_amd.decode_tensor(with_aspect(es, 5), 64, 48, 1, size, fit="contain")


def test_frame_export_tensor_fit_in_the_render_callback():
    import torch
    es, w, h, cf = golden("ipb420_field")
    frames, _ = host_frames(es, w, h, cf)
    size, par = (48, 48), (16, 15)
    crop, rect = PM.fit("contain", (1, 1, 171, 141), par, size)
    assert rect[1] > 0
    got = []

    def render(frame):
        got.append(frame.export_tensor(size, crop=(1, 1, 171, 141), dtype=torch.bfloat16, mean=IMAGENET[0],
                                       std=IMAGENET[1], matrix=5, field="bottom", fit="contain", pixel_aspect=par,
                                       pad=PAD))
        if len(got) == 1:
            with pytest.raises(ValueError):
                frame.export_tensor(size, fit="contain", place=(0, 0, 8, 8))

    d = mp2v_decoder_c(decoder_config_t(w, h, cf, device_frames=True), render)
    d.decode(es, len(es))
    d.close()
    assert len(got) == len(frames)
    s, b = T.scale_bias(*IMAGENET, "bfloat16")
    for t, planes in zip(got, frames):
        want = PM.tensor(planes, cf, 5, True, FM.BOTTOM, False, size, crop, rect, PAD, "bfloat16", s, b)
        assert np.array_equal(T.bits(t.view(torch.int16).cpu().numpy(), "bfloat16")[0], want)
