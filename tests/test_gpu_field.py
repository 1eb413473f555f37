"""GPU: the field modes of the tensor export kernel (tensor.hip) through mp2vg_tensor_planes_field,
mp2vg_tensor_slots_fields and the Python interface.  Every comparison is array_equal on bit patterns
against the numpy model (tests/field_model.py): the arithmetic is a bit-exact contract."""
import ctypes
import itertools

import numpy as np
import pytest

import field_model as FM
import tensor_model as T
from conftest import load_manifest, read_stream
from test_gpu_export import FILL, GUARD, host_frames, random_planes
from test_gpu_tensor import IMAGENET, NORM, Source
from tiny_mp2v_dec_amd import _lib
from tiny_mp2v_dec_amd import records as R
from tiny_mp2v_dec_amd.decoder import decoder_config_t, mp2v_decoder_c

pytestmark = pytest.mark.gpu

E_INVALID = -1
MODES = ("progressive", "top", "bottom", "weave")
FM_NAME = {v: k for k, v in FM.MODES.items()}


class FieldSource(Source):
    """test_gpu_tensor.Source through mp2vg_tensor_planes_field: the model's source image of each
    (chroma, mode) and its Q image of each (size, crop) are computed once and shared."""

    def __init__(self, planes, cf, cw, ch):
        super().__init__(planes, cf, cw, ch)
        self.src = {}

    def call_field(self, t, field, offset=0):
        torch = self.torch
        elem = (1, 2, 2, 4)[t.dtype]
        nbytes = 3 * t.out_w * t.out_h * elem
        buf = torch.full((GUARD + 16 + nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        at = GUARD + offset * elem
        ptrs = (ctypes.c_void_p * 3)(*[x.data_ptr() for x in self.t])
        rc = _lib.lib().mp2vg_tensor_planes_field(0, ptrs, (ctypes.c_int32 * 3)(*self.stride), self.cf, self.cw,
                                                  self.ch, field, ctypes.byref(t),
                                                  ctypes.c_void_p(buf.data_ptr() + at), nbytes)
        got = buf.cpu().numpy()
        clean = (got[:at] == FILL).all() and (got[at + nbytes:] == FILL).all()
        return rc, got[at:at + nbytes], clean

    def field_q(self, matrix, chroma, mode, size, crop):
        key = (matrix, chroma, mode)
        if key not in self.src:
            self.src[key] = FM.source(self.vis, self.cf, matrix, chroma == "linear", FM.MODES[mode])
        qkey = key + (size, crop)
        if qkey not in self.q:
            rgb = self.src[key]
            if crop is not None:
                x, y, w, h = crop
                rgb = rgb[:, y:y + h, x:x + w]
            self.q[qkey] = T.resize(rgb, size)
        return self.q[qkey]

    def check_field(self, mode, size, crop=None, dtype="uint8", mean=None, std=None, layout="nchw", chroma="linear",
                    matrix=1, offset=0):
        t = _lib.make_tensor(size, crop, dtype, mean, std, layout, chroma, matrix)
        what = (self.cf, mode, size, crop, dtype, layout, chroma, matrix, offset)
        rc, got, clean = self.call_field(t, FM.MODES[mode], offset)
        assert rc == 0, (what, _lib.lib().mp2vg_last_error())
        q = self.field_q(matrix, chroma, mode, size, crop)
        want = T.normalise(q, dtype, np.array(t.scale, np.float32), np.array(t.bias, np.float32))
        if layout == "nhwc":
            want = np.moveaxis(want, 0, -1)
        assert np.array_equal(T.bits(got, dtype).reshape(want.shape), want), what
        assert clean, ("bytes outside dst written", what)


SIZES = [(48, 32), (10, 7), (77, 50)]
# whole frame; odd origin; even origin; one row at the top and at the bottom edge of the frame (the
# a = b rules and the chroma clamps); two rows ending at the bottom edge
CROPS = [None, (1, 1, 45, 29), (5, 2, 16, 9), (0, 0, 48, 1), (0, 31, 48, 1), (3, 30, 8, 2)]


@pytest.mark.parametrize("cf,mode", itertools.product((1, 2, 3), MODES))
def test_planes_modes_sizes_and_crops(cf, mode):
    """Coded 48 x 32, stride 64: chroma mode x dtype x size x crop in one field mode.  The identity
    size of the whole frame shows the source image itself; each crop is also exported at its own
    size (identity: one tap per row, so a wrong line shows undiluted)."""
    src = FieldSource(random_planes(cf, 48, 32, 64, seed=500 + cf), cf, 48, 32)
    for chroma, dtype, crop in itertools.product(("nearest", "linear"), ("uint8", "float16"), CROPS):
        for size in SIZES + ([crop[2:]] if crop else []):
            src.check_field(mode, size, crop, dtype, *NORM[dtype], chroma=chroma,
                            layout="nhwc" if dtype == "uint8" else "nchw")


@pytest.mark.parametrize("mode", MODES)
def test_planes_32_to_1(mode):
    """Coded 96 x 64 -> 3 x 2: 32:1 on both axes, 48 tap rows per output row, 4:2:0."""
    src = FieldSource(random_planes(1, 96, 64, 128, seed=520), 1, 96, 64)
    for chroma, dtype in itertools.product(("nearest", "linear"), ("uint8", "float16")):
        src.check_field(mode, (3, 2), None, dtype, *NORM[dtype], chroma=chroma)


@pytest.mark.parametrize("mode", ("top", "weave"))
def test_planes_row_wider_than_a_workgroup_pass(mode):
    """528 wide, stride 576: more 4-pixel units in a row than the workgroup's 256 lanes."""
    src = FieldSource(random_planes(1, 528, 32, 576, seed=528), 1, 528, 32)
    src.check_field(mode, (528, 32), None, "uint8")
    src.check_field(mode, (257, 13), (3, 1, 523, 30), "float16", *IMAGENET, layout="nhwc", matrix=5, offset=1)


@pytest.mark.parametrize("cf", (1, 2, 3))
def test_progressive_field_is_the_old_entry_point(cf):
    """mp2vg_tensor_planes_field(field = 0) equals mp2vg_tensor_planes byte for byte."""
    src = FieldSource(random_planes(cf, 48, 32, 64, seed=540 + cf), cf, 48, 32)
    for chroma, dtype, size, crop in itertools.product(("nearest", "linear"), ("uint8", "float16"), SIZES, CROPS[:3]):
        t = _lib.make_tensor(size, crop, dtype, *NORM[dtype], chroma=chroma)
        rc0, old, clean0 = src.call(t)
        rc1, new, clean1 = src.call_field(t, 0)
        assert rc0 == 0 and rc1 == 0 and clean0 and clean1
        assert np.array_equal(old, new), (cf, chroma, dtype, size, crop)


# ---- mp2vg_tensor_slots_fields ---------------------------------------------------------------------

def golden(name):
    e = next(m for m in load_manifest() if m["name"] == name)
    return read_stream(e), e["width"], e["height"], e["chroma_format"]


def slots_fields(ctx, slots, fields, t, buf, nbytes=None):
    s = np.asarray(slots, np.int32)
    i32p = ctypes.POINTER(ctypes.c_int32)
    f = None if fields is None else np.asarray(fields, np.int32)
    nbytes = len(s) * 3 * t.out_w * t.out_h * (1, 2, 2, 4)[t.dtype] if nbytes is None else nbytes
    fp = None if f is None else f.ctypes.data_as(i32p)
    return _lib.lib().mp2vg_tensor_slots_fields(ctx.h, s.ctypes.data_as(i32p), fp, len(s), ctypes.byref(t),
                                                ctypes.c_void_p(buf.data_ptr() + GUARD), nbytes)


@pytest.mark.parametrize("name", ("ipb420_field", "ipb422_field"))
def test_slots_mixed_modes_in_one_launch(name):
    """Decode a golden field-coded stream, then one launch whose list repeats slots and mixes all
    four modes per frame; a fields = NULL launch equals mp2vg_tensor_slots; a bad field value is
    refused with nothing written and the context still usable."""
    import torch
    es, w, h, cf = golden(name)
    parsed = R.Parsed(es, w, h, cf)
    slots = [int(d) for d in parsed.display[:5]] + [int(parsed.display[1]), int(parsed.display[1])]
    fields = [1, 2, 3, 0, 2, 1, 0]
    size, crop = (50, 37), (3, 5, 170, 135)
    t = _lib.make_tensor(size, crop, "float16", *IMAGENET, layout="nchw", chroma="linear", matrix=5)
    nbytes = len(slots) * 3 * size[0] * size[1] * 2
    with R.DeviceContext(w, h, cf, slots=parsed.npics) as ctx:
        ctx.upload(parsed.pics, parsed.mbs, parsed.coefs)
        ctx.decode()
        buf = torch.full((GUARD + nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        # refused before anything is enqueued: guards and destination untouched
        for bad in (4, -1):
            assert slots_fields(ctx, slots, fields[:3] + [bad] + fields[4:], t, buf) == E_INVALID
        ctx.synchronize()
        assert (buf.cpu().numpy() == FILL).all()
        assert slots_fields(ctx, slots, fields, t, buf) == 0
        ctx.synchronize()
        got = buf.cpu().numpy()
        # the Python spelling of the same launch, and the two all-progressive spellings
        named = ctx.export_tensor(slots, size, crop=crop, dtype="float16", mean=IMAGENET[0], std=IMAGENET[1], matrix=5,
                                  fields=[FM_NAME[f] for f in fields])
        old = ctx.export_tensor(slots, size, crop=crop, dtype="float16", mean=IMAGENET[0], std=IMAGENET[1], matrix=5)
        buf0 = torch.full((GUARD + nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert slots_fields(ctx, slots, None, t, buf0) == 0
        ctx.synchronize()
        zeros = ctx.export_tensor(slots, size, crop=crop, dtype="float16", mean=IMAGENET[0], std=IMAGENET[1], matrix=5,
                                  fields="progressive")
        frames = {s: ctx.download(s) for s in set(slots)}
    assert (got[:GUARD] == FILL).all() and (got[GUARD + nbytes:] == FILL).all()
    s, b = T.scale_bias(*IMAGENET, "float16")
    want = np.stack([FM.tensor(frames[k], cf, 5, True, f, False, size, crop, "float16", s, b)
                     for k, f in zip(slots, fields)])
    assert np.array_equal(T.bits(got[GUARD:GUARD + nbytes], "float16").reshape(want.shape), want)
    assert np.array_equal(T.bits(named.view(torch.int16).cpu().numpy(), "float16"), want)
    old_bits = old.view(torch.int16).cpu().numpy()
    assert np.array_equal(T.bits(buf0.cpu().numpy()[GUARD:GUARD + nbytes], "float16").reshape(want.shape),
                          T.bits(old_bits, "float16"))
    assert np.array_equal(zeros.view(torch.int16).cpu().numpy(), old_bits)
    # the modes differ on real content: the first frame (TOP) is not its progressive export
    assert not np.array_equal(want[0], FM.tensor(frames[slots[0]], cf, 5, True, FM.PROGRESSIVE, False, size, crop,
                                                 "float16", s, b))


# ---- Python interface ------------------------------------------------------------------------------

def test_decode_tensor_both_fields_in_temporal_order():
    """A generated interlaced stream with top_field_first drawn per picture: fields="both" gives 2n
    frames, each picture's first field and then its second, in display order."""
    import torch
    import tiny_mp2v_dec_amd
    es = R.generate_es(width=64, height=48, chroma_format=1, n_gops=2, gop_n=6, gop_m=3, seed=611,
                       frame_pred_frame_dct=0, top_field_first=-1)
    parsed = R.Parsed(es, 64, 48, 1)
    tff = (parsed.flags[parsed.display] & _lib.PIC_TOP_FIELD_FIRST) != 0
    assert (parsed.flags & _lib.PIC_PROGRESSIVE_FRAME == 0).all() and tff.any() and not tff.all()
    frames, _ = host_frames(es, 64, 48, 1)
    out = tiny_mp2v_dec_amd.decode_tensor(es, 64, 48, 1, (40, 30), dtype="uint8", layout="nhwc", fields="both")
    assert tuple(out.shape) == (2 * parsed.npics, 30, 40, 3) and out.dtype == torch.uint8
    got = out.cpu().numpy()
    for i, planes in enumerate(frames):
        order = (FM.TOP, FM.BOTTOM) if tff[i] else (FM.BOTTOM, FM.TOP)
        for k, mode in enumerate(order):
            want = FM.tensor(planes, 1, 1, True, mode, True, (40, 30), None, "uint8")
            assert np.array_equal(got[2 * i + k], want), (i, k)
    first = tiny_mp2v_dec_amd.decode_tensor(es, 64, 48, 1, (40, 30), dtype="uint8", layout="nhwc", fields="first",
                                            device_parse=True)
    assert np.array_equal(first.cpu().numpy(), got[0::2])
    top = tiny_mp2v_dec_amd.decode_tensor(es, 64, 48, 1, (40, 30), dtype="uint8", layout="nhwc", fields="top")
    want = np.stack([FM.tensor(p, 1, 1, True, FM.TOP, True, (40, 30), None, "uint8") for p in frames])
    assert np.array_equal(top.cpu().numpy(), want)


def test_decode_tensor_first_on_a_progressive_stream_is_the_default():
    import tiny_mp2v_dec_amd
    es = R.generate_es(width=64, height=48, chroma_format=1, n_gops=1, gop_n=6, gop_m=3, seed=612,
                       frame_pred_frame_dct=1, top_field_first=-1)
    a = tiny_mp2v_dec_amd.decode_tensor(es, 64, 48, 1, (40, 30), mean=IMAGENET[0], std=IMAGENET[1])
    b = tiny_mp2v_dec_amd.decode_tensor(es, 64, 48, 1, (40, 30), mean=IMAGENET[0], std=IMAGENET[1], fields="first")
    both = tiny_mp2v_dec_amd.decode_tensor(es, 64, 48, 1, (40, 30), mean=IMAGENET[0], std=IMAGENET[1], fields="both")
    assert a.shape[0] == 6 and a.equal(b)
    assert both.shape[0] == 12 and both[0::2].equal(a) and both[1::2].equal(a)


def test_frame_export_tensor_bottom_field_in_the_render_callback():
    import torch
    es, w, h, cf = golden("ipb420_field")
    frames, _ = host_frames(es, w, h, cf)
    got = []

    def render(frame):
        got.append(frame.export_tensor((60, 45), crop=(1, 1, 171, 141), dtype=torch.float16, mean=IMAGENET[0],
                                       std=IMAGENET[1], matrix=5, field="bottom"))
        if len(got) == 1:
            with pytest.raises(ValueError):
                frame.export_tensor((60, 45), field="first")

    d = mp2v_decoder_c(decoder_config_t(w, h, cf, device_frames=True), render)
    d.decode(es, len(es))
    d.close()
    assert len(got) == len(frames)
    s, b = T.scale_bias(*IMAGENET, "float16")
    for t, planes in zip(got, frames):
        want = FM.tensor(planes, cf, 5, True, FM.BOTTOM, False, (60, 45), (1, 1, 171, 141), "float16", s, b)
        assert np.array_equal(T.bits(t.view(torch.int16).cpu().numpy(), "float16")[0], want)
