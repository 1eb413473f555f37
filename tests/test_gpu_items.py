"""GPU: the items launch of the tensor export (tensor.hip, ITEMS) through mp2vg_tensor_planes_items,
mp2vg_tensor_items and the Python interface.  Every comparison is array_equal on bit patterns: against
the entry points from before items existed (one call per rectangle) and against the numpy model
(tests/items_model.py).  Every destination is prefilled with FILL and has guard bytes on both sides;
scales and biases differ per channel."""
import ctypes
import itertools

import numpy as np
import pytest

import field_model as FM
import items_model as IM
import tensor_model as T
from conftest import load_manifest, read_stream
from test_gpu_export import FILL, GUARD, decoded_frames, gop, host_frames, random_planes
from test_gpu_field import FieldSource
from test_gpu_tensor import IMAGENET, NORM
from test_items_cpu import BAD_ITEMS, arr, raw
from tiny_mp2v_dec_amd import _lib
from tiny_mp2v_dec_amd import records as R
from tiny_mp2v_dec_amd.decoder import decoder_config_t, mp2v_decoder_c

pytestmark = pytest.mark.gpu

E_INVALID = -1
ELEM = {"uint8": 1, "float16": 2, "bfloat16": 2, "float32": 4}
P, TOP, BOT, WEAVE = "progressive", "top", "bottom", "weave"


def c_items(items):
    """(mode name, crop, flip) tuples, every one of slot 0, as the C array."""
    return _lib.make_items(None, [it[1] for it in items], [bool(it[2]) for it in items], [it[0] for it in items])


def shape_of(n, size, layout, clip_len=1):
    if layout == "nhwc":
        return (n, size[1], size[0], 3)
    return (n, 3, size[1], size[0]) if clip_len == 1 else (n // clip_len, 3, clip_len, size[1], size[0])


class ItemsSource(FieldSource):
    """test_gpu_field.FieldSource through mp2vg_tensor_planes_items; the model's Q image of each
    (matrix, chroma, mode, size, crop) is computed once and shared (items_model.Frames)."""

    def __init__(self, planes, cf, cw, ch):
        super().__init__(planes, cf, cw, ch)
        self.models = {}

    def call_items(self, items, t, clip_len=1, offset=0):
        """(status, result bytes as a flat uint8 array, guards untouched?); items: the C array."""
        torch = self.torch
        elem = (1, 2, 2, 4)[t.dtype]
        nbytes = len(items) * 3 * t.out_w * t.out_h * elem
        buf = torch.full((GUARD + 16 + nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        at = GUARD + offset * elem
        ptrs = (ctypes.c_void_p * 3)(*[x.data_ptr() for x in self.t])
        rc = _lib.lib().mp2vg_tensor_planes_items(0, ptrs, (ctypes.c_int32 * 3)(*self.stride), self.cf, self.cw, self.ch,
                                                  items, len(items), ctypes.byref(t), clip_len,
                                                  ctypes.c_void_p(buf.data_ptr() + at), nbytes)
        got = buf.cpu().numpy()
        clean = (got[:at] == FILL).all() and (got[at + nbytes:] == FILL).all()
        return rc, got[at:at + nbytes], clean

    def model(self, matrix, chroma):
        key = (matrix, chroma)
        if key not in self.models:
            self.models[key] = IM.Frames({0: self.vis}, self.cf, matrix, chroma == "linear")
        return self.models[key]

    def check_items(self, items, size, dtype="uint8", mean=None, std=None, layout="nchw", chroma="linear", matrix=1,
                    clip_len=1, offset=0):
        """One launch against the model; returns the launch's bit patterns in its own shape."""
        t = _lib.make_tensor(size, None, dtype, mean, std, layout, chroma, matrix)
        what = (self.cf, items, size, dtype, layout, chroma, matrix, clip_len, offset)
        rc, got, clean = self.call_items(c_items(items), t, clip_len, offset)
        assert rc == 0, (what, _lib.lib().mp2vg_last_error())
        want = self.model(matrix, chroma).tensor([(0, FM.MODES[m], crop, flip) for m, crop, flip in items], size, dtype,
                                                 np.array(t.scale, np.float32), np.array(t.bias, np.float32),
                                                 layout == "nhwc", clip_len)
        assert want.shape == shape_of(len(items), size, layout, clip_len)
        got = T.bits(got, dtype).reshape(want.shape)
        assert np.array_equal(got, want), what
        assert clean, ("bytes outside dst written", what)
        return got

    def check_both(self, items, size, **kw):
        """uint8 packed and normalised float16 planar"""
        self.check_items(items, size, dtype="uint8", layout="nhwc", **kw)
        self.check_items(items, size, dtype="float16", mean=IMAGENET[0], std=IMAGENET[1], layout="nchw", **kw)

    def old_call(self, mode, crop, size, dtype, layout, chroma, matrix=1):
        """One rectangle through mp2vg_tensor_planes_field, as (3, h, w) or (h, w, 3) bit patterns."""
        t = _lib.make_tensor(size, crop, dtype, *NORM[dtype], layout=layout, chroma=chroma, matrix=matrix)
        rc, got, clean = self.call_field(t, FM.MODES[mode])
        assert rc == 0 and clean
        return T.bits(got, dtype).reshape(shape_of(1, size, layout)[1:])


def source(cf, w=32, h=16, seed=800):
    return ItemsSource(random_planes(cf, w, h, (w + 63) // 64 * 64, seed=seed + cf), cf, w, h)


_wide = []


def wide_source():
    """2,560 x 8, 4:4:4: a rectangle 2,500 wide needs two segments.  Shared: its model images are
    computed once."""
    if not _wide:
        _wide.append(ItemsSource(random_planes(3, 2560, 8, 2560, seed=833), 3, 2560, 8))
    return _wide[0]


# ---- the old path, bit for bit -----------------------------------------------------------------------

@pytest.mark.parametrize("cf,mode", itertools.product((1, 2, 3), (P, TOP, WEAVE)))
def test_one_common_rectangle_is_the_old_entry_point(cf, mode):
    """Items of one common rectangle, no flip, clip_len 1: every image equals
    mp2vg_tensor_planes_field with t.src_* set to that rectangle, byte for byte."""
    src = source(cf)
    for chroma, dtype, size, crop in itertools.product(("nearest", "linear"), ("uint8", "float16"), ((24, 21), (32, 16)),
                                                       (None, (1, 1, 29, 14))):
        layout = "nhwc" if dtype == "uint8" else "nchw"
        old = src.old_call(mode, crop, size, dtype, layout, chroma)
        t = _lib.make_tensor(size, None, dtype, *NORM[dtype], layout=layout, chroma=chroma)
        rc, got, clean = src.call_items(c_items([(mode, crop, False)] * 3), t)
        assert rc == 0 and clean, _lib.lib().mp2vg_last_error()
        got = T.bits(got, dtype).reshape((3,) + old.shape)
        for i in range(3):
            assert np.array_equal(got[i], old), (cf, mode, chroma, dtype, size, crop, i)
    # the whole frame spelled as its rectangle
    whole = src.check_items([(mode, None, False), (mode, (0, 0, 32, 16), False)], (24, 21))
    assert np.array_equal(whole[0], whole[1])


# ---- item independence ---------------------------------------------------------------------------------

MIXED = [(P, (0, 0, 32, 16), False), (TOP, (1, 1, 29, 14), True), (WEAVE, (5, 2, 16, 9), False), (BOT, (3, 3, 8, 12), True),
         (P, (7, 5, 16, 9), True), (P, None, False), (TOP, (5, 2, 16, 9), False)]


@pytest.mark.parametrize("cf", (1, 2, 3))
def test_every_item_is_its_own_single_call(cf):
    """A launch of mixed rectangles, modes and flips: item i equals the single-frame call of the
    old entry point with its rectangle and mode, mirrored on the host when flipped; the launch
    equals the model."""
    src = source(cf, seed=810)
    for dtype, layout, chroma in (("uint8", "nhwc", "linear"), ("float16", "nchw", "nearest"), ("float32", "nchw", "linear")):
        got = src.check_items(MIXED, (20, 11), dtype, *NORM[dtype], layout=layout, chroma=chroma)
        for i, (mode, crop, flip) in enumerate(MIXED):
            old = src.old_call(mode, crop, (20, 11), dtype, layout, chroma)
            if flip:
                old = old[:, ::-1] if layout == "nhwc" else old[:, :, ::-1]
            assert np.array_equal(got[i], old), (cf, dtype, layout, i)


# ---- different tables in one launch --------------------------------------------------------------------

def test_two_taps_next_to_sixty_five():
    """Coded 96 x 64 into 3 x 2: 96 -> 3 and 64 -> 2 are 32:1 (the longest tap rows), 2 -> 3 and
    1 -> 2 upscale (two taps): the extremes on each axis in turn and on both, in one launch, so
    hmax and vmax differ between the items of a workgroup's neighbours."""
    src = ItemsSource(random_planes(1, 96, 64, 128, seed=841), 1, 96, 64)
    assert int(_lib.tensor_weights(96, 3)[1].max()) == 64 and int(_lib.tensor_weights(2, 3)[1].max()) == 2
    items = [(P, (4, 3, 2, 1), False), (P, (0, 0, 96, 1), False), (P, (7, 0, 2, 64), True), (P, None, False),
             (TOP, (0, 0, 96, 64), True), (P, (94, 63, 2, 1), False), (WEAVE, (0, 5, 96, 2), False)]
    src.check_both(items, (3, 2))
    src.check_both(items[::-1], (3, 2), chroma="nearest")


def test_shared_and_unshared_tables():
    """Two items sharing src_w but not src_h and the reverse; equal sizes at different origins (odd
    x and odd y); rectangles flush to each edge and corner of the coded frame; 1 x 1 rectangles."""
    src = source(1, seed=850)
    src.check_both([(P, (0, 0, 20, 10), False), (P, (3, 1, 20, 7), False), (P, (4, 2, 11, 7), True), (P, (1, 3, 20, 10), False)],
                   (12, 9))
    src.check_both([(P, (0, 0, 16, 8), False), (P, (1, 1, 16, 8), False), (P, (7, 3, 16, 8), True), (P, (15, 7, 16, 8), False),
                    (P, (16, 8, 16, 8), False)], (12, 9))
    edges = [(0, 0, 9, 5), (23, 0, 9, 5), (0, 11, 9, 5), (23, 11, 9, 5),          # the corners
             (0, 4, 9, 5), (23, 4, 9, 5), (11, 0, 9, 5), (11, 11, 9, 5),          # the edges
             (0, 0, 32, 1), (0, 15, 32, 1), (0, 0, 1, 16), (31, 0, 1, 16)]        # whole first / last row and column
    for mode in (P, BOT):
        src.check_both([(mode, r, i % 3 == 0) for i, r in enumerate(edges)], (12, 9))
    ones = [(0, 0, 1, 1), (31, 0, 1, 1), (0, 15, 1, 1), (31, 15, 1, 1), (13, 7, 1, 1), (14, 8, 1, 1)]
    for cf in (1, 2, 3):
        s = source(cf, seed=851)
        s.check_both([(P, r, False) for r in ones] + [(TOP, r, True) for r in ones], (3, 2))
        s.check_both([(WEAVE, r, False) for r in ones], (1, 1))


# ---- different segment counts in one launch ------------------------------------------------------------

NARROW = [(9, 1, 32, 5), (2528, 3, 32, 5)]


@pytest.mark.parametrize("order", ("two segments first", "one segment first", "between"))
def test_segment_counts(order):
    """A rectangle 2,500 wide needs two segments, the 32-wide ones one: grid.x is 2, and the second
    workgroup of a one-segment item returns at once and writes nothing.  float32: the FILL pattern
    is no value the export produces, so it must survive nowhere inside dst (the model says what is
    there) and everywhere outside."""
    src = wide_source()
    size = (90, 4)
    assert IM.segments(2500, 90) == 2 and IM.segments(32, 90) == 1
    plan = R.items_plan(2560, 16, 3, size, [(3, 0, 2500, 8)] + NARROW)
    assert plan["grid_x"] == 2 and plan["n_htab"] == 2
    for flips in ((False, False, False), (True, True, True), (True, False, True)):
        wide = (P, (3, 0, 2500, 8), flips[0])
        narrow = [(P, r, f) for r, f in zip(NARROW, flips[1:])]
        items = {"two segments first": [wide] + narrow, "one segment first": narrow + [wide],
                 "between": [narrow[0], wide, narrow[1]]}[order]
        got = src.check_items(items, size, "float32", *IMAGENET, layout="nchw" if flips[0] else "nhwc")
        assert not (got == 0xA5A5A5A5).any()
    # the flipped and the unflipped two-segment item in one launch
    got = src.check_items([(P, (3, 0, 2500, 8), False), (P, (3, 0, 2500, 8), True)], size)
    assert np.array_equal(got[0], got[1][:, :, ::-1])


# ---- flip ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("out_w", (1, 2, 5, 24))
def test_flip(out_w):
    """out_w of 1, 2, odd and even, packed and planar, every dtype; flipped and unflipped copies of
    one rectangle in one launch mirror each other."""
    src = source(1, seed=860)
    items = [(P, (1, 1, 29, 14), False), (P, (1, 1, 29, 14), True), (BOT, (4, 3, 16, 9), True), (BOT, (4, 3, 16, 9), False)]
    for dtype, layout in itertools.product(T.DTYPES, ("nchw", "nhwc")):
        got = src.check_items(items, (out_w, 7), dtype, *NORM[dtype], layout=layout, offset=1 if layout == "nhwc" else 0)
        mirror = (lambda a: a[:, ::-1]) if layout == "nhwc" else (lambda a: a[:, :, ::-1])
        assert np.array_equal(got[0], mirror(got[1])) and np.array_equal(got[2], mirror(got[3]))


# ---- field modes per item --------------------------------------------------------------------------------

@pytest.mark.parametrize("cf", (1, 2))
def test_field_modes_per_item(cf):
    """All four modes of one frame in one launch, each with its own rectangle: src_y odd and even,
    rectangles whose first or last row is the frame's first or last line (the a = b rules)."""
    src = source(cf, seed=870)
    rects = [(0, 0, 32, 16), (1, 1, 29, 14), (5, 2, 16, 9), (3, 0, 20, 1), (3, 15, 20, 1), (2, 13, 9, 3), (6, 0, 9, 2),
             (0, 7, 32, 2)]
    for chroma in ("nearest", "linear"):
        for k in range(4):  # every rectangle meets every mode
            items = [((TOP, BOT, WEAVE, P)[(i + k) % 4], r, i % 2 == 1) for i, r in enumerate(rects)]
            src.check_both(items, (12, 9), chroma=chroma)
    # identity size: the source lines themselves
    src.check_both([(m, (4, y, 12, 9), False) for m in (TOP, BOT, WEAVE, P) for y in (2, 3, 7)], (12, 9))


# ---- clip layout -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", ((10, 7), (10, 1), (3, 4)))
def test_clip_layout(size):
    """n = 6 with clip_len 1, 2, 3 and 6, planar, every dtype: [n / T][3][T][h][w].  Packed output
    ignores clip_len beyond checking it."""
    src = source(2, seed=880)
    items = [(P, (0, 0, 32, 16), False), (P, (1, 1, 29, 14), True), (TOP, (5, 2, 16, 9), False), (P, (3, 3, 8, 12), True),
             (WEAVE, (7, 5, 16, 9), False), (P, (2, 0, 9, 16), True)]
    for dtype in T.DTYPES:
        flat = src.check_items(items, size, dtype, *NORM[dtype], clip_len=1)
        for clip_len in (2, 3, 6):
            got = src.check_items(items, size, dtype, *NORM[dtype], clip_len=clip_len)
            for i in range(6):
                assert np.array_equal(got[i // clip_len, :, i % clip_len], flat[i])
    one = src.check_items(items, size, "float16", *IMAGENET, layout="nhwc", clip_len=1)
    three = src.check_items(items, size, "float16", *IMAGENET, layout="nhwc", clip_len=3)
    assert np.array_equal(one, three)


# ---- the slots form on decoded frames ----------------------------------------------------------------------

def golden(name):
    e = next(m for m in load_manifest() if m["name"] == name)
    return read_stream(e), e["width"], e["height"], e["chroma_format"]


QCIF_ITEMS = [  # (display index, mode, crop, flip)
    (0, 0, (10, 7, 120, 90), False), (2, 0, (1, 1, 175, 143), True), (0, 0, (10, 7, 120, 90), True), (3, 1, (31, 20, 64, 64), False),
    (1, 3, None, True), (2, 2, (100, 3, 76, 141), False), (3, 0, (0, 0, 1, 1), False), (1, 0, (50, 50, 120, 90), False),
]


def test_slots_form_over_a_golden_stream():
    """ipb420_qcif: one launch whose items come from different pictures, in any order and with
    repeats, through the C entry point into a guarded buffer and through export_items, against the
    model over the frames the context holds; then in clip order.  A refused launch writes nothing
    and leaves the context usable."""
    import torch
    es, w, h, cf = golden("ipb420_qcif")
    parsed = R.Parsed(es, w, h, cf)
    assert parsed.npics >= 4
    size = (40, 30)
    slots = [int(parsed.display[d]) for d, _, _, _ in QCIF_ITEMS]
    crops, flips, modes = [i[2] for i in QCIF_ITEMS], [i[3] for i in QCIF_ITEMS], [i[1] for i in QCIF_ITEMS]
    items = _lib.make_items(slots, crops, flips, modes)
    n = len(items)
    t = _lib.make_tensor(size, None, "float16", *IMAGENET, layout="nchw", chroma="linear", matrix=5)
    nbytes = n * 3 * size[0] * size[1] * 2
    with R.DeviceContext(w, h, cf, slots=parsed.npics) as ctx:
        ctx.upload(parsed.pics, parsed.mbs, parsed.coefs)
        ctx.decode()
        buf = torch.full((GUARD + nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

        def call(its, clip_len=1, count=None):
            return _lib.lib().mp2vg_tensor_items(ctx.h, its, len(its) if count is None else count, ctypes.byref(t), clip_len,
                                                 ctypes.c_void_p(buf.data_ptr() + GUARD), nbytes)

        bad_slot = _lib.make_items([slots[0], parsed.npics] + slots[2:], crops, flips, modes)
        assert call(bad_slot) == E_INVALID and b"item 1:" in _lib.lib().mp2vg_last_error()
        outside = _lib.make_items(slots, crops[:5] + [(100, 3, 77, 141)] + crops[6:], flips, modes)
        assert call(outside) == E_INVALID and b"item 5:" in _lib.lib().mp2vg_last_error()
        assert call(items, clip_len=3) == E_INVALID and call(items, count=0) == E_INVALID
        ctx.synchronize()
        assert (buf.cpu().numpy() == FILL).all()
        assert call(items) == 0, _lib.lib().mp2vg_last_error()
        ctx.synchronize()
        got = buf.cpu().numpy()
        named = ctx.export_items(slots, size, crops, flips, modes, dtype="float16", mean=IMAGENET[0], std=IMAGENET[1],
                                 matrix=5)
        clips = ctx.export_items(slots, size, crops, flips, modes, clip_len=4, dtype=torch.float16, mean=IMAGENET[0],
                                 std=IMAGENET[1], matrix=5)
        packed = ctx.export_items(slots, size, crops, flips, modes, clip_len=2, dtype="uint8", layout="nhwc", matrix=5)
        frames = {s: ctx.download(s) for s in set(slots)}
    assert (got[:GUARD] == FILL).all() and (got[GUARD + nbytes:] == FILL).all()
    model = IM.Frames(frames, cf, 5, True)
    its = list(zip(slots, modes, crops, flips))
    s, b = T.scale_bias(*IMAGENET, "float16")
    want = model.tensor(its, size, "float16", s, b)
    assert np.array_equal(T.bits(got[GUARD:GUARD + nbytes], "float16").reshape(want.shape), want)
    assert tuple(named.shape) == (n, 3, 30, 40) and tuple(clips.shape) == (2, 3, 4, 30, 40)
    assert np.array_equal(T.bits(named.view(torch.int16).cpu().numpy(), "float16"), want)
    assert np.array_equal(T.bits(clips.view(torch.int16).cpu().numpy(), "float16"),
                          model.tensor(its, size, "float16", s, b, clip_len=4))
    assert tuple(packed.shape) == (n, 30, 40, 3)
    assert np.array_equal(packed.cpu().numpy(), model.tensor(its, size, "uint8", packed=True))
    # the same rectangle of the same picture, flipped and not; another picture is another image
    assert np.array_equal(want[0], want[2][:, :, ::-1]) and not np.array_equal(want[0], want[7])


def test_slots_items_exports_then_a_batch_that_overwrites_the_slots():
    """decode A, two items exports of A's slots back to back, decode B into the same slots, one
    synchronise: both exports read A's frames (they share the events of the exports they extend, so
    the batch waits for them, and the staging ring keeps the first export's blob while the second is
    staged).  The exports are long: their item lists repeat the slots 256 times.  uint8 at the
    rectangle's own size: the RGB export's bytes, mirrored when flipped."""
    import torch
    import export_model
    a, b = gop(1, seed=961), gop(1, seed=962)
    assert a.npics == b.npics
    frames_a, frames_b = decoded_frames(a), decoded_frames(b)
    assert not np.array_equal(frames_a[0][0], frames_b[0][0])
    slots = np.tile(np.arange(a.npics, dtype=np.int32), 256)
    rects = [(3, 5, 160, 120), (16, 24, 160, 120)]
    crops = [[rects[(i // a.npics + k) % 2] for i in range(len(slots))] for k in (0, 1)]
    flips = [bool((i // a.npics) & 2) for i in range(len(slots))]
    with R.DeviceContext(176, 144, 1, slots=a.npics) as ctx:
        outs = [torch.full((len(slots), 120, 160, 3), FILL, dtype=torch.uint8, device="cuda") for _ in (0, 1)]
        torch.cuda.synchronize()
        ctx.upload(a.pics, a.mbs, a.coefs)
        ctx.decode()
        for k in (0, 1):
            ctx.export_items(slots, (160, 120), crops[k], flips, dtype="uint8", layout="nhwc", out=outs[k], sync=False)
        ctx.upload(b.pics, b.mbs, b.coefs)
        ctx.decode()
        ctx.synchronize()
        after = ctx.export_items(np.arange(a.npics), (160, 120), [rects[0]] * a.npics, dtype="uint8", layout="nhwc")

    def images(frames):
        """[rectangle][flip][slot] on the device"""
        rgb = [export_model.export(f, 1, 1, True, True) for f in frames]
        return torch.from_numpy(np.stack([np.stack([np.stack([im[y:y + h, x:x + w][:, ::-1] if fl else im[y:y + h, x:x + w]
                                                              for im in rgb]) for fl in (0, 1)])
                                          for x, y, w, h in rects])).cuda()

    ia = images(frames_a)
    idx = torch.from_numpy(slots.astype(np.int64)).cuda()
    fl = torch.tensor(flips, dtype=torch.int64, device="cuda")
    for k in (0, 1):
        r = torch.tensor([(i // a.npics + k) % 2 for i in range(len(slots))], dtype=torch.int64, device="cuda")
        assert torch.equal(outs[k], ia[r, fl, idx]), k
    assert torch.equal(after, images(frames_b)[0, 0])


def test_frame_export_items_in_the_render_callback():
    """Many rectangles of one device frame inside the render callback (the two-stage inference
    case), against the model over the host-frame decoder's planes."""
    import torch
    es, w, h, cf = golden("ipb420_qcif")
    frames, _ = host_frames(es, w, h, cf)
    size = (24, 24)
    boxes = [(10, 7, 120, 90), (31, 20, 64, 64), None, (100, 3, 76, 141), (0, 0, 24, 24), (151, 119, 24, 24)]
    flips = [False, True, False, True, False, True]
    got = []

    def render(frame):
        got.append(frame.export_items(boxes, size, flips, fields=[0, 0, 3, 0, 1, 2], clip_len=3, dtype=torch.bfloat16,
                                      mean=IMAGENET[0], std=IMAGENET[1], matrix=5))

    d = mp2v_decoder_c(decoder_config_t(w, h, cf, device_frames=True), render)
    d.decode(es, len(es))
    d.close()
    assert len(got) == len(frames) and tuple(got[0].shape) == (2, 3, 3, 24, 24)
    s, b = T.scale_bias(*IMAGENET, "bfloat16")
    for t, planes in list(zip(got, frames))[:3]:
        want = IM.Frames({0: planes}, cf, 5, True).tensor(list(zip([0] * 6, [0, 0, 3, 0, 1, 2], boxes, flips)), size,
                                                          "bfloat16", s, b, clip_len=3)
        assert np.array_equal(T.bits(t.view(torch.int16).cpu().numpy(), "bfloat16"), want)


# ---- rejections on the device entry point ------------------------------------------------------------------

def test_rejections_write_nothing():
    """Every rejection of tests/test_items_cpu.py through mp2vg_tensor_planes_items with real planes
    and a real destination: MP2VG_E_INVALID, dst keeps FILL.  Coded 96 x 64 into 16 x 8."""
    src = ItemsSource(random_planes(1, 96, 64, 128, seed=890), 1, 96, 64)

    def refused(items, t=None, clip_len=1):
        rc, got, clean = src.call_items(items, t or _lib.make_tensor((16, 8), None, "uint8"), clip_len)
        return rc == E_INVALID and clean and (got == FILL).all()

    for case, bad in sorted(BAD_ITEMS.items()):
        assert refused(arr(raw(), bad)), case
        assert b"item 1:" in _lib.lib().mp2vg_last_error(), case
    assert refused(arr(raw(), raw(slot=1)))                                  # the planes form takes slot 0 only
    assert refused(arr(raw(), raw(rect=(0, 0, 64, 32))), _lib.make_tensor((1, 8), None, "uint8"))   # 64:1
    assert refused(arr(raw(rect=(0, 0, 16, 33))), _lib.make_tensor((16, 1), None, "uint8"))         # 33:1
    for k in ("src_x", "src_y", "src_w", "src_h"):
        t = _lib.make_tensor((16, 8), None, "uint8")
        setattr(t, k, 1)
        assert refused(arr(raw(), raw()), t), k
    for clip_len in (0, -1, 3):
        assert refused(arr(raw(), raw()), clip_len=clip_len), clip_len
    # n = 0 and n = 65536: the array is not read
    t = _lib.make_tensor((16, 8), None, "uint8")
    ptrs = (ctypes.c_void_p * 3)(*[x.data_ptr() for x in src.t])
    buf = src.torch.full((1024,), FILL, dtype=src.torch.uint8, device="cuda")
    for n in (0, 65536):
        assert _lib.lib().mp2vg_tensor_planes_items(0, ptrs, (ctypes.c_int32 * 3)(*src.stride), 1, 96, 64, arr(raw()), n,
                                                    ctypes.byref(t), 1, ctypes.c_void_p(buf.data_ptr()),
                                                    n * 3 * 16 * 8) == E_INVALID
    assert (buf.cpu().numpy() == FILL).all()
    # a field mode on a 4:2:0 coded height that is no multiple of 4: the same planes read as 96 x 62
    rc = _lib.lib().mp2vg_tensor_planes_items(0, ptrs, (ctypes.c_int32 * 3)(*src.stride), 1, 96, 62,
                                              arr(raw(), raw(field=1)), 2, ctypes.byref(t), 1,
                                              ctypes.c_void_p(buf.data_ptr()), 2 * 3 * 16 * 8)
    assert rc == E_INVALID and b"item 1:" in _lib.lib().mp2vg_last_error() and (buf.cpu().numpy() == FILL).all()
    # and the launch that is fine still runs
    src.check_items([(P, (4, 2, 64, 32), False), (TOP, (4, 2, 64, 32), True)], (16, 8))
