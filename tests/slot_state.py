"""Directed tests of what a context carries between calls: the per-slot tile flag (runtime.cpp
tiles_ok, which decides whether tile_convert_kernel runs before a batch reads a slot), the slot table
mp2vg_reserve_slots rebuilds when the pool grows, the slot pointers the placement calibration may
move, and the slot readers every test relies on (download, packed copy, digests).

This module is plain Python (no device): slot images in device layout with garbage in every padding
byte, the pool size the runtime computes for a growth history, and the batches of the state matrix,
shared by tests/test_slot_state_cpu.py (which checks their preconditions from the dumped plans) and
tests/test_gpu_slot_state.py."""
import numpy as np

import _oracle
import directed_sched as DS
from directed_sched import pic
from tiny_mp2v_dec_amd import _lib

SIZES = [(80, 48), (16, 16), (128, 48)]          # state matrix
READER_SIZES = [(16, 16), (80, 48), (1040, 16)]  # slot readers
SWEEP_SIZES = [(128, 64), (144, 80)]             # tests/directed.py mc_sweep
GROW_SIZE = (128, 48)
TRIP_SIZE = (512, 528)                           # tile_convert_kernel's second grid-stride trip
ALL_SIZES = sorted(set(SIZES + READER_SIZES + SWEEP_SIZES + [GROW_SIZE, TRIP_SIZE]))

POOL_PAD = 4096 + 65536  # runtime.cpp kPoolPad: slack after the last slot of a frames block
CHUNK = 16               # slots per pool block


def geometry(width, height, cf):
    """The oracle's geometry, after checking that mp2vg_frame_geometry gives the same plane sizes,
    strides and slot size, and that the planes are consecutive (the layout slot_image writes)."""
    g = _oracle.geometry(width, height, cf)
    pw, ph, stride, slot_bytes = _lib.geometry(width, height, cf)
    assert (list(g.pw), list(g.ph), list(g.stride), int(g.slot_bytes)) == (pw, ph, stride, slot_bytes), (width, height, cf)
    off = 0
    for p in range(3):
        assert int(g.plane_off[p]) == off and g.pw[p] <= g.stride[p]
        off += g.stride[p] * g.ph[p]
    assert off == int(g.slot_bytes)
    return g


def random_planes(g, seed):
    """Visible planes [Y, Cb, Cr] of seeded full-range bytes with planted extremes: corners and
    scattered samples at 0 and 255, a whole row at each, a half row at 255."""
    rng = np.random.default_rng(seed)
    out = []
    for p in range(3):
        h, w = g.ph[p], g.pw[p]
        b = rng.integers(0, 256, (h, w), dtype=np.uint8)
        for v in (0, 255):
            b[rng.integers(0, h, 24), rng.integers(0, w, 24)] = v
        b[(h - 1) // 3, :] = 0
        b[(2 * h) // 3, :] = 255
        b[h // 2, : w // 2] = 255
        b[0, 0], b[0, w - 1], b[h - 1, 0], b[h - 1, w - 1] = 0, 255, 255, 0
        out.append(b)
    return out


def slot_image(g, planes, pad_seed):
    """The slot_bytes image of a slot in device layout: planes consecutive, plane p in rows of
    stride[p] bytes, every padding byte (columns [pw[p], stride[p]) of every row) seeded garbage
    that is never zero."""
    geometry(g.width, g.height, g.chroma_format)
    rng = np.random.default_rng(pad_seed)
    parts = []
    for p in range(3):
        assert planes[p].shape == (g.ph[p], g.pw[p]) and planes[p].dtype == np.uint8
        rows = rng.integers(1, 256, (g.ph[p], g.stride[p]), dtype=np.uint8)
        rows[:, :g.pw[p]] = planes[p]
        parts.append(rows.reshape(-1))
    image = np.concatenate(parts)
    assert len(image) == int(g.slot_bytes)
    return image


def image_planes(g, image):
    """The visible planes of a slot image (views)."""
    return [image[int(g.plane_off[p]): int(g.plane_off[p]) + g.stride[p] * g.ph[p]].reshape(g.ph[p], g.stride[p])[:, :g.pw[p]]
            for p in range(3)]


def write_slot(ctx, slot, planes, pad_seed):
    """slot_image(planes) copied to the slot's device address with a synchronous host-to-device
    hipMemcpy, as an outside producer would.  Does not invalidate: that is the caller's step."""
    from tiny_mp2v_dec_amd.decoder import _hip_lib
    g = geometry(ctx.width, ctx.height, ctx.chroma_format)
    image = slot_image(g, planes, pad_seed)
    assert _hip_lib().hipMemcpy(ctx.slot_ptr(slot), image.ctypes.data, image.nbytes, 1) == 0  # host to device
    return image


def pool_bytes(slot_bytes, history):
    """Bytes of the pool the runtime holds after a growth history ([4, 64]: created with 4 slots,
    grown to 64): each growth adds blocks of at most 16 slots, each block one frames allocation
    (the slots plus the pad) and one tiles allocation (2 x the slot, rounded up to 256 B, per slot).
    This is the size calibrate_placement compares with MP2VG_PLACE_MIN_MB."""
    tile = (2 * slot_bytes + 255) // 256 * 256
    total, have = 0, 0
    for n in history:
        for s0 in range(have, n, CHUNK):
            k = min(CHUNK, n - s0)
            total += slot_bytes * k + POOL_PAD + tile * k
        have = max(have, n)
    return total


# ---- the state matrix ----------------------------------------------------------------------------
# How each reference slot of batches 2 and 3 got its content:
#   S1 anchor that stored its tiles inline             slots 0 (read in its batch), 7 (a last anchor)
#   S2 anchor that stored none (batch 1 has five anchors; these are not read in it and are not its
#      last two)                                        slot 1 (I picture), slot 2 (P picture)
#   S3 B picture never read in its batch                slot 3
#   S4 never written                                    slot 4
#   S5 written from outside, then invalidated           slot 5
#   S6 decoded with inline tiles, then overwritten from outside and invalidated    slot 6
STATE_OF_SLOT = {0: "S1", 7: "S1", 1: "S2", 2: "S2", 3: "S3", 4: "S4", 5: "S5", 6: "S6"}
STORES_TILES = {0: 1, 1: 0, 2: 0, 3: 0, 6: 1, 7: 1}  # batch 1's writes, by slot
# two groups that share no slot, so that two streams give two reading sets
GROUPS = [(0, 1, 2, 3), (7, 4, 5, 6)]
NSLOTS = 8 + 3 * 8 + 2


def batch1_spec(two="fb"):
    return [pic("I", 0), pic("I", 1), pic("P", 2, 0), pic("I", 6), pic("P", 7, 6), pic("B", 3, 0, 7, two)]


def reader_spec(flip, two="fb"):
    """Every state slot X read by a P picture, by a two-direction B picture (with the next slot of
    its group as the other reference; X forward, or backward with flip) and by a one-direction B
    picture (forward and backward in turn), each into a slot of its own; then, per group, a B
    picture that reads one of those B pictures (a tile conversion inside the batch, TilePlan.post)
    and a state slot.  two: the MB kind of the two-direction B pictures ("d" where a picture is
    one MB)."""
    spec, dst = [], 8
    for grp in GROUPS:
        first_b = None
        for i, x in enumerate(grp):
            y = grp[(i + 1) % len(grp)]
            spec.append(pic("P", dst, x))
            spec.append(pic("B", dst + 1, *((y, x) if flip else (x, y)), two))
            first_b = dst + 1 if first_b is None else first_b
            spec.append(pic("B", dst + 2, x, -1, "f") if (i + flip) % 2 == 0 else pic("B", dst + 2, -1, x, "b"))
            dst += 3
        spec.append(pic("B", 32 + GROUPS.index(grp), first_b, grp[-1], two))
    assert dst == 32
    return spec


_matrix = {}


def matrix_batches(width, height, cf):
    """[(spec, pics, mbs, coefs)] of the three batches of the state matrix, built once."""
    key = (width, height, cf)
    if key not in _matrix:
        out = []
        two = "d" if width * height < 3 * 256 else "fb"
        for k, spec in enumerate((batch1_spec(two), reader_spec(0, two), reader_spec(1, two))):
            pics, mbs, coefs, _uses = DS.build(width, height, cf, spec, seed=7000 + 100 * k + 10 * (width % 97) + cf)
            out.append((spec, pics, mbs, coefs))
        _matrix[key] = out
    return _matrix[key]


def check_matrix_plans(width, height, cf, dump_fn):
    """The preconditions of the state matrix, from the dumped plans alone (dump_fn(pics, mbs,
    coefs, one_stream) = records.plan_dump at NSLOTS slots)."""
    (s1, *b1), (s2, *b2), (s3, *b3) = matrix_batches(width, height, cf)
    d1 = dump_fn(*b1, False)
    writes = {int(s): int(t) for s, t in d1["writes"]}
    assert writes == STORES_TILES, writes
    assert len(d1["ext_reads"]) == 0 and len(d1["post"]) == 0
    assert not set(writes) & {4, 5}  # S4 and S5: batch 1 never touches them
    for b in (b2, b3):
        d = dump_fn(*b, False)
        ext = {int(s): int(t) for s, t in d["ext_reads"]}
        assert sorted(ext) == list(range(8)), ext          # every state slot is read from outside
        for grp in GROUPS:
            assert len({ext[s] for s in grp}) == 1
        assert {ext[GROUPS[0][0]], ext[GROUPS[1][0]]} == {0, 1}  # one group per reading set
        assert set(dump_fn(*b, True)["ext_reads"][:, 1].tolist()) == {0}
        assert sorted(int(s) for _l, s in d["post"]) == [9, 21]   # the B pictures read inside the batch
        assert not {int(s) for s, _t in d["writes"]} & set(range(8))  # decoding it again is exact
    return d1


# ---- growth ----------------------------------------------------------------------------------------
def growth_specs():
    """The batches of the growth test: into slots 0-4 (B picture in slot 4); after the growth to
    20 slots one that predicts from slot 1 (outside content), 4 (B picture), 0 (inline tiles) and 7
    (new: zeros, overwritten later in the batch) and writes slots 5-19; one uploaded at 20 slots
    and decoded at 33; one uploaded at 33 and decoded at 49."""
    a = [pic("I", 0), pic("P", 1, 0), pic("P", 2, 1), pic("I", 3), pic("B", 4, 0, 1, "d")]
    b = [pic("P", 5, 1), pic("B", 6, 4, 0), pic("P", 8, 7), pic("B", 9, 1, 7), pic("B", 10, 4, -1, "f"),
         pic("B", 11, -1, 0, "b"), pic("I", 7), pic("P", 12, 7), pic("B", 13, 5, 8), pic("P", 14, 0),
         pic("B", 15, 12, 14), pic("P", 16, 4), pic("I", 17), pic("P", 18, 17), pic("B", 19, 17, 18)]
    assert sorted(s[1] for s in b) == list(range(5, 20))
    c = [pic("P", 5, 19), pic("B", 6, 1, 4), pic("P", 2, 13), pic("B", 0, 15, 6)]
    d = [pic("P", 20, 5), pic("B", 32, 20, 1), pic("P", 25, 31), pic("I", 31), pic("B", 16, 32, 31)]
    return a, b, c, d


# ---- calibration -----------------------------------------------------------------------------------
def calibrated_specs():
    """First batch of the calibrated case: two components (two picture sets on two streams); slot 0
    is read from outside and never written; B picture 2 is read by B picture 3 (a conversion inside
    the batch).  Second batch: predicts from slot 0 after it was rewritten from outside."""
    first = [pic("P", 1, 0), pic("B", 2, 0, 1), pic("B", 3, 2, 1), pic("I", 4), pic("P", 5, 4), pic("B", 6, 4, 5)]
    second = [pic("P", 7, 0), pic("B", 3, 0, 7)]
    return first, second


def ordinary_specs():
    """Two ordinary batches over 4 slots (nothing read from outside that the batch overwrites)."""
    return [pic("I", 0), pic("P", 1, 0), pic("B", 2, 0, 1)], [pic("P", 3, 1), pic("B", 2, 0, 3)]


# ---- the conversion's second trip ------------------------------------------------------------------
_trip = {}


def trip_batch(cf):
    """At 512x528 (luma 270,336 B: more 16-B chunks than tile_convert_kernel's 128 x 256 threads),
    a P picture (slot 2, forward slot 0) and a B picture (slot 3, forward slot 0, backward slot 1)
    of test_gpu_parity.random_batch: (pics, mbs, coefs)."""
    if cf not in _trip:
        from test_gpu_parity import random_batch
        pics, mbs, coefs = random_batch(*TRIP_SIZE, cf, 2, seed=8800 + cf, n_intra=0)
        pics["dst_slot"], pics["fwd_slot"], pics["bwd_slot"] = [2, 3], [0, 0], [-1, 1]
        _trip[cf] = (pics, mbs, coefs)
    return _trip[cf]


def last_row_uses(pics, mbs, p):
    """(forward used, backward used) by the inter MBs of picture p's last MB row."""
    from tiny_mp2v_dec_amd._lib import MB_BWD, MB_FWD, MB_INTRA
    n = int(pics[p]["mb_width"]) * int(pics[p]["mb_height"])
    m = mbs[int(pics[p]["mb_first"]):int(pics[p]["mb_first"]) + n]
    m = m[m["y"] == int(pics[p]["mb_height"]) - 1]
    f = m["flags"].astype(np.int64)
    inter = (f & MB_INTRA) == 0
    return bool(np.any(inter & (((f & MB_FWD) != 0) | ((f & MB_BWD) == 0)))), bool(np.any(inter & ((f & MB_BWD) != 0)))
