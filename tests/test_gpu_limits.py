"""GPU: the kernels at the geometry limits (MP2VG_MAX_DIMENSION = 16384): 1024-MB rows, 1023-MB rows
in a 16384-byte stride, 1024 MB rows, vectors at the ends of int16, tiles converted from padded
16384-byte rows and from 4096 tile bands, and the slot readers and exports on such slots.  The sizes
are the smallest that reach the limits:
  W  = 16384 x 32   1024-MB rows, 1024 tile columns
  W' = 16368 x 32   1023-MB rows (remainder 3 mod the 4-MB group), luma pw 16368 in a 16384 stride
  T  = 32 x 16384   1024 MB rows, 4096 luma tile bands
  T' = 16 x 16384   rows narrower than a group
Every comparison is array_equal: against the C oracle on the same records (tests/directed.py) or
slot contents (helpers.SlotOracle), the numpy models of the exports, or the compiled reference's
MD5s.  tests/test_directed_cpu.py asserts what the batches cover; tests/test_abi.py the bound."""
import ctypes
import hashlib

import numpy as np
import pytest

import directed as D
import export_model
import motion_model
import residual_model
import slot_state as S
import tensor_model
from conftest import load_manifest, read_stream
from helpers import SlotOracle
from test_gpu_directed import assert_frames_equal, gpu_frames
from tiny_mp2v_dec_amd import _lib
from tiny_mp2v_dec_amd import records as R

pytestmark = pytest.mark.gpu

W, W1, T, T1 = (16384, 32), (16368, 32), (32, 16384), (16, 16384)
CFS = pytest.mark.parametrize("cf", [1, 2, 3])
GUARD = 0xA5
MANIFEST = {e["name"]: e for e in load_manifest()}


def _size_id(s):
    return "%dx%d" % s


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    """torch brings its own HIP runtime: it is loaded and initialised before this module's first
    context (tests/test_gpu_motion.py)."""
    import torch
    torch.cuda.init()


# ---- the bound on the device entry points ------------------------------------------------------------

def test_create_refuses_sizes_above_the_limit():
    """mp2vg_create and mp2vg_decoder_create: 16384 in either dimension is accepted, 16400 and
    1 << 20 are refused with MP2VG_E_INVALID and a message that names the limit."""
    L = _lib.lib()
    fn = _lib.RENDER_FN(lambda user, frame: None)
    for w, h in ((16384, 16), (16, 16384)):
        cfg, ctx, dec = _lib.make_config(w, h, 1, pool=2), ctypes.c_void_p(), ctypes.c_void_p()
        _lib.check(L.mp2vg_create(ctypes.byref(cfg), ctypes.byref(ctx)), "create")
        _lib.check(L.mp2vg_destroy(ctx), "destroy")
        _lib.check(L.mp2vg_decoder_create(ctypes.byref(cfg), fn, None, ctypes.byref(dec)), "decoder_create")
        _lib.check(L.mp2vg_decoder_destroy(dec), "decoder_destroy")
    for w, h in ((16400, 16), (16, 16400), (1 << 20, 16), (16, 1 << 20)):
        cfg, ctx, dec = _lib.make_config(w, h, 1, pool=2), ctypes.c_void_p(), ctypes.c_void_p()
        assert L.mp2vg_create(ctypes.byref(cfg), ctypes.byref(ctx)) == -1 and not ctx
        assert b"16384" in L.mp2vg_last_error()
        assert L.mp2vg_decoder_create(ctypes.byref(cfg), fn, None, ctypes.byref(dec)) == -1 and not dec
        assert b"16384" in L.mp2vg_last_error()


# ---- the recon kernels against the oracle ------------------------------------------------------------

@CFS
@pytest.mark.parametrize("size", [W, W1, T, T1], ids=_size_id)
def test_row_widths_at_the_limits(size, cf):
    """D.row_width_batch (every record feature, field MC, saturating levels; I, P and three B
    pictures): one-row slices of 1024 and 1023 MBs with and without mates, 1024 slices per picture,
    and 1024 rows narrower than a group."""
    w, h = size
    pics, mbs, coefs = D.row_width_batch(w, h, cf)
    exp = D.expected_frames(("rows", w, h, cf), w, h, cf, pics, mbs, coefs)
    got = gpu_frames(w, h, cf, 5, [(pics, mbs, coefs)])
    assert_frames_equal(got, exp, w, h, cf, pics, mbs)


@CFS
@pytest.mark.parametrize("size", [W, W1], ids=_size_id)
def test_long_horizontal_vectors_at_the_limits(size, cf):
    """D.long_vector_batch: mvx from +32735 in column 0 to -32735 in the last column at 16384 (the
    ends of int16 but one; +-32703 at 16368), frame and field MC, P and two-direction B: the tap's
    tile column over 1024 columns."""
    w, h = size
    pics, mbs, coefs = D.long_vector_batch(w, h, cf)
    fwd = mbs["mv"][:, 0, 0, 0].astype(int)  # (the backward vectors reach -32 * 1022 = -32704 at 16368)
    assert int(fwd.max()) == 2 * (w - 16) - 1 == -int(fwd.min())
    exp = D.expected_frames(("long", w, h, cf), w, h, cf, pics, mbs, coefs)
    got = gpu_frames(w, h, cf, len(pics), [(pics, mbs, coefs)])
    assert_frames_equal(got, exp, w, h, cf, pics, mbs)


@CFS
@pytest.mark.parametrize("size", [T, (48, 4128)], ids=_size_id)
def test_long_vertical_vectors_at_the_limits(size, cf):
    """D.long_vertical_batch: mvy from +32735 in row 0 to -32735 in the last row (frame MC; +-16367
    field MC) at 16384 lines, every tap mode and MC type: the tap's tile band over 4096 bands.
    48 x 4128: 3-MB rows, tile bands past 1024 and rows past 4096."""
    w, h = size
    pics, mbs, coefs = D.long_vertical_batch(w, h, cf)
    exp = D.expected_frames(("vertical", w, h, cf), w, h, cf, pics, mbs, coefs)
    got = gpu_frames(w, h, cf, len(pics), [(pics, mbs, coefs)])
    assert_frames_equal(got, exp, w, h, cf, pics, mbs)


@CFS
@pytest.mark.parametrize("case", [W + (128, 32), T + (32, 64)], ids=lambda c: "%dx%d" % c[:2])
def test_tap_sweep_at_the_far_corner(case, cf):
    """D.corner_sweep: the whole tap sweep (every tap mode and MC type with all 64 x-phase and
    y-phase pairs, the right and bottom edge contacts with and without half-pel:
    tests/test_directed_cpu.py) in the last 8 MB columns of 16384 x 32 and in the last 4 MB rows of
    32 x 16384, on anchors textured over the whole plane: the taps' tile offsets at columns 1016 to
    1023 and at bands 4080 to 4095."""
    w, h, sw, sh = case
    s = D.corner_sweep(w, h, cf, sw, sh)
    exp = D.expected_frames(("corner", w, h, cf), w, h, cf, s.pics, s.mbs, s.coefs)
    got = gpu_frames(w, h, cf, len(s.pics), [(s.pics, s.mbs, s.coefs)])
    assert_frames_equal(got, exp, w, h, cf, s.pics, s.mbs)


@CFS
@pytest.mark.parametrize("kind", ["I", "P", "B"])
def test_group_word_counts_in_a_1024_mb_row(cf, kind):
    """D.word_count_batch at 16384 x 16: the directed word totals in a row of 256 groups, which a
    wave walks with its group stride; the other groups hold the smallest total."""
    w, h = 16384, 16
    pics, mbs, coefs = D.word_count_batch(w, h, cf, kind)
    exp = D.expected_frames(("words", w, h, cf, kind), w, h, cf, pics, mbs, coefs)
    got = gpu_frames(w, h, cf, len(pics), [(pics, mbs, coefs)])
    assert_frames_equal(got, exp, w, h, cf, pics, mbs)


# ---- conversion, slot readers and exports on slots written from outside -------------------------------

_readers = {}


def reader_batch(w, h, cf):
    """A P picture (slot 2, forward slot 0) and a two-direction B picture (slot 3, forward slot 0,
    backward slot 1) of test_gpu_parity.random_batch."""
    if (w, h, cf) not in _readers:
        from test_gpu_parity import random_batch
        pics, mbs, coefs = random_batch(w, h, cf, 2, seed=9900 + cf + w, n_intra=0)
        pics["dst_slot"], pics["fwd_slot"], pics["bwd_slot"] = [2, 3], [0, 0], [-1, 1]
        _readers[(w, h, cf)] = (pics, mbs, coefs)
    return _readers[(w, h, cf)]


def tail_uses(pics, mbs, p):
    """(forward used, backward used) by the inter MBs of picture p's last eight MBs: the last tile
    columns of the last rows, or the last tile bands of a narrow picture."""
    from tiny_mp2v_dec_amd._lib import MB_BWD, MB_FWD, MB_INTRA
    n = int(pics[p]["mb_width"]) * int(pics[p]["mb_height"])
    f = mbs["flags"][int(pics[p]["mb_first"]) + n - 8:int(pics[p]["mb_first"]) + n].astype(np.int64)
    inter = (f & MB_INTRA) == 0
    return bool(np.any(inter & (((f & MB_FWD) != 0) | ((f & MB_BWD) == 0)))), bool(np.any(inter & ((f & MB_BWD) != 0)))


def download_strided(ctx, slot, strides):
    bufs = [np.full((ctx.ph[p] + 2, strides[p]), GUARD, np.uint8) for p in range(3)]
    ptrs = (ctypes.c_void_p * 3)(*[b[1:].ctypes.data for b in bufs])
    _lib.check(_lib.lib().mp2vg_download_slot(ctx.h, slot, ptrs, (ctypes.c_int32 * 3)(*strides)), "download_slot")
    return bufs


def far_corner(w, h):
    """(crop at the far corner at the largest ratio (32:1), its output size, the output size of
    the whole frame within that ratio)"""
    if w > h:
        return (w - 7168, 0, 7168, h), (224, 8), (512, 8)
    return (0, h - 7168, w, 7168), (8, 224), (8, 512)


@CFS
@pytest.mark.parametrize("size", [W1, T], ids=_size_id)
def test_converted_tiles_readers_and_exports_at_the_limits(size, cf):
    """Slots 0 and 1 written from outside (slot_state.slot_image: garbage in every padding byte, 16
    bytes per luma row at 16368) and invalidated, then read by a P and a two-direction B picture:
    tile_convert_kernel builds the tiles from padded 16384-byte rows and from 4096 tile bands.  On
    those slots and the decoded ones: download (with destination strides), the packed copy, the
    digests, the RGB export and the tensor export (the far corner at 32:1, the whole frame inside
    32:1) against their numpy twins."""
    w, h = size
    pics, mbs, coefs = reader_batch(w, h, cf)
    assert tail_uses(pics, mbs, 0) == (True, False) and tail_uses(pics, mbs, 1) == (True, True)
    exp = SlotOracle(w, h, cf, 4)
    g = exp.g
    A, B = S.random_planes(g, 101), S.random_planes(g, 102)
    with R.DeviceContext(w, h, cf, slots=4) as ctx:
        for slot, planes, seed in ((0, A, 103), (1, B, 104)):
            S.write_slot(ctx, slot, planes, seed)
            ctx.invalidate(slot)
            exp.preload(slot, planes)
        ctx.upload(pics, mbs, coefs)
        ctx.decode()
        ctx.synchronize()
        exp.decode(pics, mbs, coefs)
        frames = [exp.planes(s) for s in range(4)]
        for s in range(4):
            got = ctx.download(s)
            for k in range(3):
                assert np.array_equal(got[k], frames[s][k]), ("slot", s, "plane", k)
        # the readers
        for strides in ([x + 5 for x in ctx.pw], list(ctx.stride)):
            for p, buf in enumerate(download_strided(ctx, 1, strides)):
                assert np.array_equal(buf[1:-1, :ctx.pw[p]], B[p]), (strides, p)
                assert (buf[0] == GUARD).all() and (buf[-1] == GUARD).all() and (buf[:, ctx.pw[p]:] == GUARD).all()
        nbytes = ctx.frame_bytes()
        for s in (0, 3):
            host = np.full(nbytes + 128, GUARD, np.uint8)
            ctx.copy_packed(s, host.ctypes.data + 64, False)
            assert np.array_equal(host[64:64 + nbytes], np.concatenate([p.reshape(-1) for p in frames[s]])), s
            assert (host[:64] == GUARD).all() and (host[64 + nbytes:] == GUARD).all()
        order = [3, 0, 1, 2, 0]
        assert [int(x) for x in ctx.digests(order)] == [R.planes_digest(frames[s]) for s in order]
        C = [x.copy() for x in A]
        C[0][-1, -1] ^= 0x10  # the last visible byte of the slot's luma, next to the padding
        S.write_slot(ctx, 0, C, 105)
        assert int(ctx.digests([0])[0]) == R.planes_digest(C) != R.planes_digest(A)
        frames[0] = C
        # the exports
        for layout in ("nchw", "nhwc"):
            got = ctx.export_rgb([1, 3], layout=layout, matrix=5).cpu().numpy()
            for i, s in enumerate((1, 3)):
                assert np.array_equal(got[i], export_model.export(frames[s], cf, 5, True, layout == "nhwc")), (layout, s)
        crop, size_c, size_f = far_corner(w, h)
        for cr, sz, dtype, layout in ((crop, size_c, "float16", "nchw"), (None, size_f, "uint8", "nhwc"),
                                      (crop, size_c, "float32", "nhwc")):
            got = ctx.export_tensor([0, 2], sz, crop=cr, dtype=dtype, layout=layout).cpu().numpy()
            scale, bias = tensor_model.scale_bias(dtype=dtype)
            for i, s in enumerate((0, 2)):
                want = tensor_model.tensor(frames[s], cf, 1, True, layout == "nhwc", sz, cr, dtype, scale, bias)
                assert np.array_equal(tensor_model.bits(got[i], dtype), want), (cr, sz, dtype, layout, s)


@CFS
@pytest.mark.parametrize("size", [W, T], ids=_size_id)
def test_motion_and_residual_exports_at_the_limits(size, cf):
    """mp2vg_motion_batch and mp2vg_residual_batch on the resident records of D.row_width_batch:
    planes of 1024 MBs per row and of 1024 MB rows against their numpy models."""
    w, h = size
    pics, mbs, coefs = D.row_width_batch(w, h, cf)
    order = [4, 0, 1]
    with R.DeviceContext(w, h, cf, slots=5) as ctx:
        ctx.upload(pics, mbs, coefs)
        got = ctx.export_motion(order)
        want = motion_model.model(pics, mbs, coefs, cf, order=order)
        for name, a, b in zip(("mv", "info", "act"), got, want):
            assert np.array_equal(a.cpu().numpy(), b), name
        got = ctx.export_residual(order, dtype="int16")
        want = residual_model.model(pics, mbs, coefs, w, h, cf, order=order, dtype="int16")
        for name, a, b in zip(("y", "cb", "cr"), got, want):
            assert np.array_equal(a.cpu().numpy(), b), name


# ---- the largest frame ---------------------------------------------------------------------------------

def test_largest_frame(monkeypatch):
    """16384 x 16384 at 4:4:4, the only shape whose tile offsets pass 2^30 (the Cr tile plane starts
    at 2^30 of a 1.5 GiB tile slot): two references written from outside and invalidated (tiles
    converted from 4096 bands of 1024 columns), the P and the two-direction B picture of
    D.sparse_frame_batch, and every byte of both decoded slots against D.sparse_frame_expected
    (the oracle on the directed MBs, the definition of a zero-vector MB on the others;
    tests/test_directed_cpu.py shows that this is the oracle's frame).  The context's four slots
    (9 GiB with tiles) are above the placement calibration's default threshold:
    MP2VG_PLACE_MIN_MB is set far above the pool, so the calibration (three pools of that size,
    the batch decoded on each) does not run; it moves slots and changes no byte
    (tests/test_gpu_slot_state.py)."""
    monkeypatch.setenv("MP2VG_PLACE_MIN_MB", str(1 << 20))
    w, h, cf = 16384, 16384, 3
    need = 7 * 805306368  # the oracle's four slots, a reference image, a downloaded slot, slack
    avail = [int(line.split()[1]) * 1024 for line in open("/proc/meminfo") if line.startswith("MemAvailable")]
    if avail and avail[0] < need:
        pytest.skip("the host has %.1f GiB available, the oracle's pool and the frames need %.1f" %
                    (avail[0] / 2**30, need / 2**30))
    from tiny_mp2v_dec_amd.decoder import _hip_lib
    pics, mbs, coefs, directed = D.sparse_frame_batch(w, h, cf)
    assert R.plan_batch(w, h, cf, 4, pics, mbs, coefs)[1].tolist() == [3]  # one mixed launch
    exp = SlotOracle(w, h, cf, 4)
    g, sb = exp.g, 805306368
    assert int(g.slot_bytes) == sb and list(g.stride) == [16384] * 3  # no padding: the image is the planes
    assert 2 * int(g.plane_off[2]) == 1 << 30
    rng = np.random.default_rng(2 ** 14)
    with R.DeviceContext(w, h, cf, slots=4) as ctx:
        for slot in (0, 1):
            image = exp.pool[slot * sb:(slot + 1) * sb]
            image[:] = D.textured_bytes(rng, sb)
            assert _hip_lib().hipMemcpy(ctx.slot_ptr(slot), image.ctypes.data, sb, 1) == 0  # host to device
            ctx.invalidate(slot)
        ctx.upload(pics, mbs, coefs)
        ctx.decode()
        D.sparse_frame_expected(exp, pics, mbs, coefs, directed)  # (while the device decodes)
        ctx.synchronize()
        assert ctx.placement() == ([], -1)
        for slot in (2, 3):
            got = ctx.download(slot)
            for k, e in enumerate(exp.planes(slot)):
                if not np.array_equal(got[k], e):
                    ys, xs = np.nonzero(got[k] != e)
                    pytest.fail("slot %d plane %d: %d bytes differ, first at (x %d, y %d)" %
                                (slot, k, len(xs), xs[0], ys[0]))
            del got


# ---- the drop-in decoder on the limit streams ----------------------------------------------------------

@pytest.mark.parametrize("name", ["tall_16384_420", "wide_16384_422"])
@pytest.mark.parametrize("device_frames", [False, True], ids=["host_frames", "device_frames"])
def test_dropin_decodes_the_limit_streams(name, device_frames):
    """16 x 16384 (vertical_size 16383, slices in all eight values of
    slice_vertical_position_extension) and 16384 x 16 (horizontal_size 16383, f_code 9) through
    mp2v_decoder_c: the compiled reference's frames, in its display order."""
    from tiny_mp2v_dec_amd.decoder import decoder_config_t, mp2v_decoder_c
    e = MANIFEST[name]
    md5 = []
    dec = mp2v_decoder_c(decoder_config_t(e["width"], e["height"], e["chroma_format"], device_frames=device_frames),
                         lambda f: md5.append(hashlib.md5(f.yuv_bytes()).hexdigest()))
    es = read_stream(e)
    assert dec.decode(es, len(es))
    dec.close()
    assert md5 == e["md5"]


@pytest.mark.parametrize("name", ["tall_16384_420", "wide_16384_422"])
def test_device_parse_of_the_limit_streams(name):
    """The limit streams through mp2vg_batch_upload_es: the device's records are the host
    emitter's byte for byte, and the frames the compiled reference's."""
    from helpers import yuv_md5
    e = MANIFEST[name]
    w, h, cf = e["width"], e["height"], e["chroma_format"]
    es = read_stream(e)
    parsed = R.Parsed(es, w, h, cf)
    with R.Scan(es, w, h, cf) as scan, R.DeviceContext(w, h, cf, slots=parsed.npics) as ctx:
        ctx.upload_es(scan)
        mbs, coefs = ctx.download_records()
        assert mbs.tobytes() == parsed.mbs.tobytes() and coefs.tobytes() == parsed.coefs.tobytes()
        ctx.decode()
        ctx.synchronize()
        assert [yuv_md5(ctx.download(int(d))) for d in parsed.display] == e["md5"]
