"""CPU: the items launch of the tensor export (include/mp2vg.h "Items"): the launch plan
(mp2vg_tensor_items_plan) against the model (tests/items_model.py), every rejection of the three
entry points' shared validation with the item's index in the error text (the device entry points
check every argument before the first HIP call, so their rejections run here), the ABI, the model
against hand-computed values and the Python spellings.  Every comparison is exact."""
import ctypes
import random

import numpy as np
import pytest

import field_model as FM
import items_model as IM
import tensor_model as T
from test_gpu_export import random_planes, visible
from tiny_mp2v_dec_amd import _lib
from tiny_mp2v_dec_amd import records as R

E_INVALID = -1
CODED = (2560, 1088)   # a configuration's sides are multiples of 16


def to_items(items):
    """(slot, mode, crop, flip) tuples of the model as the C array."""
    return _lib.make_items([it[0] for it in items], [it[2] for it in items], [bool(it[3]) for it in items],
                           [it[1] for it in items])


def check_plan(items, size, coded=CODED, cf=1, clip_len=1):
    got = R.items_plan(coded[0], coded[1], cf, size, None, clip_len=clip_len, items=to_items(items))
    want = IM.plan(items, coded, size)
    assert got["htab"].tolist() == want["htab"] and got["vtab"].tolist() == want["vtab"], (items, size)
    for k in ("n_htab", "n_vtab", "grid_x", "words"):
        assert got[k] == want[k], (k, got[k], want[k], items, size)
    return got


# ---- the plan ----------------------------------------------------------------------------------------

DIRECTED = {
    "one item, the whole frame": ([(0, 0, None, 0)], (96, 40)),
    "the whole frame is the table of its size": ([(0, 0, None, 0), (1, 0, (0, 0, 2560, 1088), 1), (0, 0, (1, 1, 2559, 1087), 0)],
                                                 (96, 40)),
    "same src_w, other src_h; origins and flips do not matter": (
        [(0, 0, (0, 0, 300, 200), 0), (3, 1, (17, 9, 300, 100), 1), (0, 0, (5, 5, 300, 200), 1), (0, 3, (0, 0, 150, 100), 0)],
        (24, 21)),
    "same src_h, other src_w": ([(0, 0, (0, 0, 300, 200), 0), (0, 0, (1, 3, 150, 200), 0), (0, 0, (0, 0, 31, 200), 0)], (24, 21)),
    "2 taps next to 65": ([(0, 0, (0, 0, 8, 8), 0), (0, 0, (0, 0, 320, 224), 0), (0, 0, (0, 0, 8, 224), 0),
                           (0, 0, (0, 0, 320, 8), 0)], (10, 7)),
    "two segments next to one, both orders": ([(0, 0, (3, 0, 2500, 8), 0), (0, 0, (9, 1, 32, 5), 0), (0, 0, (0, 0, 2500, 4), 1)],
                                              (100, 4)),
    "one segment first, then two": ([(0, 0, (9, 1, 32, 5), 1), (0, 0, (3, 0, 2500, 8), 0)], (100, 4)),
    "1 x 1 rectangles": ([(0, 0, (0, 0, 1, 1), 0), (0, 0, (2559, 1087, 1, 1), 1)], (5, 3)),
    "upscaling wider than the window": ([(0, 0, (0, 0, 2560, 16), 0), (0, 0, (0, 0, 16, 16), 0)], (2600, 2)),
}


@pytest.mark.parametrize("case", sorted(DIRECTED))
def test_plan_directed(case):
    items, size = DIRECTED[case]
    check_plan(items, size)


def test_plan_counts_by_hand():
    """Three widths and two heights among five items: the counts, the indices in order of first use,
    and the blob size written out: 16 words a record; a horizontal table 4 words a segment, out_w
    firsts and out_w x hmax weights; a vertical one out_h firsts, out_h counts, out_h x vmax weights."""
    items = [(0, 0, (0, 0, 64, 32), 0), (0, 0, (1, 1, 32, 32), 0), (0, 0, (2, 2, 64, 16), 1), (0, 0, (3, 3, 16, 32), 0),
             (0, 0, (4, 4, 32, 16), 0)]
    got = check_plan(items, (16, 8))
    assert got["htab"].tolist() == [0, 1, 0, 2, 1] and got["vtab"].tolist() == [0, 0, 1, 0, 1]
    assert (got["n_htab"], got["n_vtab"], got["grid_x"]) == (3, 2, 1)
    # ratio 4 has 8 taps and ratio 2 has 4; the identity's table width is the model's
    hm = [T.taps(s, 16)[2].shape[1] for s in (64, 32, 16)]
    vm = [T.taps(s, 8)[2].shape[1] for s in (32, 16)]
    assert hm[:2] == [8, 4] and vm == [8, 4]
    assert got["words"] == 5 * 16 + sum(4 + 16 + 16 * m for m in hm) + sum(8 + 8 + 8 * m for m in vm)


def test_plan_random_lists():
    """Seeded random item lists over a 2560 x 1088 frame: a few distinct sizes drawn many times, so
    tables are shared, and now and then a rectangle wide enough for two segments."""
    rng = random.Random(4711)
    for trial in range(12):
        size = (rng.choice((7, 24, 96)), rng.choice((5, 16, 40)))
        ws = [rng.randint(max(1, size[0] // 4), min(32 * size[0], 2560)) for _ in range(rng.randint(1, 4))]
        hs = [rng.randint(max(1, size[1] // 4), min(32 * size[1], 1088)) for _ in range(rng.randint(1, 4))]
        if trial % 3 == 0 and size[0] == 96:
            ws.append(2500)
        items = []
        for _ in range(rng.randint(1, 24)):
            w, h = rng.choice(ws), rng.choice(hs)
            items.append((rng.randint(0, 5), rng.randint(0, 3), (rng.randint(0, 2560 - w), rng.randint(0, 1088 - h), w, h),
                          rng.randint(0, 1)))
        n = len(items)
        check_plan(items, size, clip_len=rng.choice([d for d in range(1, n + 1) if n % d == 0]))


def test_many_crops_of_few_sizes_stage_little():
    """1,000 items of eight distinct sizes stage eight tables per axis, not a thousand."""
    rng = random.Random(99)
    sizes = [(rng.randint(100, 900), rng.randint(100, 900)) for _ in range(8)]
    items = []
    for i in range(1000):
        w, h = sizes[i % 8]
        items.append((0, 0, (rng.randint(0, 2560 - w), rng.randint(0, 1088 - h), w, h), i & 1))
    got = check_plan(items, (56, 56))
    assert got["n_htab"] <= 8 and got["n_vtab"] <= 8
    assert got["words"] < 1000 * 16 + 16 * (4 + 2 * 56 + 56 * 65)


# ---- rejections --------------------------------------------------------------------------------------

GOOD = (0, 0, (4, 2, 64, 32), 0)


def last_error():
    return _lib.lib().mp2vg_last_error().decode()


def c_plan(items, size=(16, 8), coded=(96, 64), cf=1, clip_len=1, n=None, t=None):
    cfg = _lib.make_config(coded[0], coded[1], cf)
    t = t or _lib.make_tensor(size, None, "uint8")
    summary = (ctypes.c_int32 * 4)()
    return _lib.lib().mp2vg_tensor_items_plan(ctypes.byref(cfg), ctypes.byref(t), items, len(items) if n is None else n,
                                              clip_len, None, None, summary)


def c_planes(items, size=(16, 8), coded=(96, 64), cf=1, clip_len=1, n=None, t=None):
    """mp2vg_tensor_planes_items with plane and destination addresses that are never used: every
    call here is refused before the first HIP call."""
    t = t or _lib.make_tensor(size, None, "uint8")
    n = len(items) if n is None else n
    planes = (ctypes.c_void_p * 3)(4096, 8192, 12288)
    stride = (ctypes.c_int32 * 3)(coded[0], coded[0], coded[0])
    return _lib.lib().mp2vg_tensor_planes_items(0, planes, stride, cf, coded[0], coded[1], items, n, ctypes.byref(t),
                                                clip_len, ctypes.c_void_p(65536), n * 3 * t.out_w * t.out_h)


def raw(slot=0, field=0, rect=(4, 2, 64, 32), flags=0, reserved=0):
    return _lib.Item(slot, field, *rect, flags, reserved)


def arr(*items):
    return (_lib.Item * len(items))(*items)


# on a 96 x 64 frame into 16 x 8: what is wrong with the item behind a good one
BAD_ITEMS = {
    "unknown flag bit": raw(flags=2),
    "unknown flag bit next to the flip": raw(flags=3),
    "reserved": raw(reserved=1),
    "one pixel past the right edge": raw(rect=(33, 2, 64, 32)),
    "one pixel past the bottom edge": raw(rect=(4, 33, 64, 32)),
    "one pixel past the left edge": raw(rect=(-1, 2, 64, 32)),
    "one pixel past the top edge": raw(rect=(4, -1, 64, 32)),
    "negative origin": raw(rect=(-5, -7, 16, 8)),
    "negative size": raw(rect=(4, 2, -3, 8)),
    "an origin with the whole-frame size": raw(rect=(1, 0, 0, 0)),
    "a width without a height": raw(rect=(0, 0, 16, 0)),
    "field mode 4": raw(field=4),
    "field mode -1": raw(field=-1),
    "negative slot": raw(slot=-1),
}


@pytest.mark.parametrize("case", sorted(BAD_ITEMS))
def test_a_bad_item_is_named_by_its_index(case):
    bad = BAD_ITEMS[case]
    for items, at in ((arr(raw(), bad), 1), (arr(raw(), raw(flags=1), raw(rect=(0, 0, 0, 0)), bad, raw()), 3), (arr(bad), 0)):
        for call in (c_plan, c_planes):
            assert call(items) == E_INVALID, (case, call.__name__)
            assert f"item {at}:" in last_error(), (case, call.__name__, last_error())
    assert c_plan(arr(raw(), raw(flags=1))) == 0 and c_plan(arr(raw(rect=(32, 32, 64, 32)))) == 0


def test_ratio_is_judged_per_item_and_per_axis():
    """33:1 on one axis of one item is refused; 32:1 passes; the whole frame is not judged when no
    item takes it (96 x 64 into 2 x 1 would be 48:1 and 64:1)."""
    for size, rect, ok in (((2, 8), (0, 0, 64, 32), True), ((2, 8), (0, 0, 65, 32), False), ((2, 8), (0, 0, 66, 32), False),
                           ((16, 1), (0, 0, 64, 32), True), ((16, 1), (0, 0, 64, 33), False)):
        for call in (c_plan, c_planes):
            rc = call(arr(raw(rect=(0, 0, 2, 1)), raw(rect=rect)), size=size)
            if ok and call is c_plan:
                assert rc == 0, (size, rect)
            if not ok:
                assert rc == E_INVALID and "item 1:" in last_error() and "ratio" in last_error(), (size, rect, last_error())
    assert c_plan(arr(raw(rect=(0, 0, 0, 0))), size=(2, 1)) == E_INVALID and "item 0:" in last_error()
    assert c_plan(arr(raw(rect=(0, 0, 64, 32))), size=(2, 1)) == 0


def test_launch_arguments():
    """t->src_* non-zero, clip_len below 1 or not a divisor of n, n = 0 and n = 65536."""
    two = arr(raw(), raw())
    for call in (c_plan, c_planes):
        for k in ("src_x", "src_y", "src_w", "src_h"):
            t = _lib.make_tensor((16, 8), None, "uint8")
            setattr(t, k, 1)
            assert call(two, t=t) == E_INVALID and "src_" in last_error(), k
        t = _lib.make_tensor((16, 8), (0, 0, 96, 64), "uint8")    # even the rectangle that is the whole frame
        assert call(two, t=t) == E_INVALID
        for clip_len in (0, -1, 3, 4):
            assert call(two, clip_len=clip_len) == E_INVALID and "clip_len" in last_error(), clip_len
        assert call(arr(raw(), raw(), raw()), clip_len=2) == E_INVALID
        assert call(two, n=0) == E_INVALID and call(two, n=-1) == E_INVALID
        big = (_lib.Item * 65536)()
        for i in range(65536):
            big[i] = raw()
        assert call(big) == E_INVALID and "65535" in last_error()
        # what every tensor export refuses in t is refused here too
        t = _lib.make_tensor((16, 8), None, "uint8")
        t.dtype = 4
        assert call(two, t=t) == E_INVALID
        t = _lib.make_tensor((16, 8), None, "uint8")
        t.reserved[2] = 1
        assert call(two, t=t) == E_INVALID
    assert c_plan(two, clip_len=2) == 0 and c_plan(two, clip_len=1) == 0
    big = (_lib.Item * 65535)()
    for i in range(65535):
        big[i] = raw()
    assert c_plan(big) == 0 and c_plan(big, clip_len=5) == 0    # 65535 = 3 * 5 * 17 * 257


def test_clip_len_is_checked_for_packed_output_too():
    t = _lib.make_tensor((16, 8), None, "uint8", layout="nhwc")
    assert c_plan(arr(raw(), raw(), raw()), clip_len=2, t=t) == E_INVALID
    assert c_plan(arr(raw(), raw(), raw()), clip_len=3, t=t) == 0


def test_field_modes_need_the_coded_height():
    """A field mode on a 4:2:0 coded height that is no multiple of 4 (4:2:2: odd) is refused with
    the item's index; PROGRESSIVE items of the same launch are not.  Only the planes call can see
    such a height: a configuration's is a multiple of 16."""
    for cf, h, ok in ((1, 62, False), (1, 64, True), (2, 62, True), (2, 63, False), (3, 63, False)):
        for mode in (1, 2, 3):
            rc = c_planes(arr(raw(rect=(0, 0, 64, 32)), raw(field=mode, rect=(0, 0, 64, 32))), coded=(96, h), cf=cf)
            if not ok:
                assert rc == E_INVALID and "item 1:" in last_error() and "field" in last_error(), (cf, h, mode)
    assert c_planes(arr(raw(field=1)), coded=(96, 62)) == E_INVALID and "item 0:" in last_error()


def test_planes_form_takes_slot_0_only():
    assert c_planes(arr(raw(), raw(slot=1))) == E_INVALID and "item 1:" in last_error() and "slot" in last_error()
    assert c_plan(arr(raw(), raw(slot=1))) == 0    # the plan does not know the context's slot count


# ---- ABI ---------------------------------------------------------------------------------------------

def test_abi():
    assert ctypes.sizeof(_lib.Item) == 32
    assert [f[0] for f in _lib.Item._fields_] == ["slot", "field", "src_x", "src_y", "src_w", "src_h", "flags", "reserved"]
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("mp2vg_tensor_items", "mp2vg_tensor_planes_items", "mp2vg_tensor_items_plan"):
        assert hasattr(L, name), name
        assert name in _lib.EXPORTS
    assert _lib.ITEM_HFLIP == 1


# ---- the model and the Python spellings ------------------------------------------------------------------

def test_model_by_hand():
    """The identity size shows the source pixels: a flipped item is the mirrored crop, and the clip
    layout puts item b T + k at [b, :, k]."""
    planes = visible(random_planes(3, 16, 8, 64, seed=5), 3, 16, 8)
    fr = IM.Frames({0: planes, 1: [p[::-1].copy() for p in planes]}, 3, 1, False)
    rgb = [FM.source(fr.frames[s], 3, 1, False, FM.PROGRESSIVE) for s in (0, 1)]
    items = [(0, 0, (1, 2, 5, 3), 0), (0, 0, (1, 2, 5, 3), 1), (1, 0, (0, 0, 5, 3), 0), (1, 0, (11, 5, 5, 3), 1)]
    out = fr.tensor(items, (5, 3), "uint8")
    assert out.shape == (4, 3, 3, 5)
    assert np.array_equal(out[0], rgb[0][:, 2:5, 1:6]) and np.array_equal(out[1], rgb[0][:, 2:5, 1:6][:, :, ::-1])
    assert np.array_equal(out[3], rgb[1][:, 5:8, 11:16][:, :, ::-1])
    clip = fr.tensor(items, (5, 3), "uint8", clip_len=2)
    assert clip.shape == (2, 3, 2, 3, 5)
    for i in range(4):
        assert np.array_equal(clip[i // 2, :, i % 2], out[i])
        for c in range(3):  # the contract's index formula
            at = (((i // 2) * 3 + c) * 2 + i % 2) * 3 * 5
            assert np.array_equal(clip.ravel()[at:at + 15], out[i, c].ravel())
    packed = fr.tensor(items, (5, 3), "uint8", packed=True, clip_len=2)
    assert packed.shape == (4, 3, 5, 3) and np.array_equal(packed[1], np.moveaxis(out[1], 0, -1))
    assert IM.segments(2048, 2048) == 1 and IM.segments(2560, 2560) == 2 and IM.segments(2500, 100) == 2


def test_python_spellings():
    items = _lib.make_items([3, 1], [(1, 2, 5, 3), None], [True, False], ["top", 3])
    assert [(i.slot, i.field, i.src_x, i.src_y, i.src_w, i.src_h, i.flags, i.reserved) for i in items] == \
        [(3, 1, 1, 2, 5, 3, 1, 0), (1, 3, 0, 0, 0, 0, 0, 0)]
    items = _lib.make_items(None, [None, (0, 0, 4, 4), (1, 1, 2, 2)], True, "weave")
    assert [(i.slot, i.field, i.flags) for i in items] == [(0, 3, 1)] * 3
    assert len(_lib.make_items(2, None, None, None, 4)) == 4
    for bad in (dict(slots=[0], crops=[None, None]), dict(slots=None, crops=[None], flips=[True, False]),
                dict(slots=None, crops=[None], fields=["top", "top"]), dict(slots=None, crops=[None], fields="left")):
        with pytest.raises(ValueError):
            _lib.make_items(**bad)
    t = _lib.make_tensor((5, 3), None, "float16")
    assert _lib.items_shape(t, 6, 1) == (6, 3, 3, 5) and _lib.items_shape(t, 6, 3) == (2, 3, 3, 3, 5)
    assert _lib.items_shape(_lib.make_tensor((5, 3), None, "float16", layout="nhwc"), 6, 3) == (6, 3, 5, 3)
    with pytest.raises(ValueError):
        _lib.items_shape(t, 6, 4)
    got = R.items_plan(96, 64, 1, (16, 8), [(0, 0, 64, 32), None, (5, 5, 64, 16)], flips=[False, True, True])
    assert got["htab"].tolist() == [0, 1, 0] and got["vtab"].tolist() == [0, 1, 2] and got["grid_x"] == 1
    with pytest.raises(_lib.Mp2vgError, match="item 1"):
        R.items_plan(96, 64, 1, (16, 8), [None, (90, 0, 16, 8)])
