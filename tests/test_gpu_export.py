"""GPU: the RGB export kernel (export.hip) through mp2vg_export_planes, mp2vg_export_slots and the
Python interface.  Every comparison is array_equal against the numpy model (tests/export_model.py):
the arithmetic is a bit-exact contract."""
import ctypes
import itertools

import numpy as np
import pytest

import export_model as M
from conftest import load_manifest, read_stream
from tiny_mp2v_dec_amd import _lib
from tiny_mp2v_dec_amd import records as R
from tiny_mp2v_dec_amd.decoder import decoder_config_t, mp2v_decoder_c

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0xA5


def plane_sizes(cf, cw, ch):
    return [(ch, cw)] + [(ch // 2 if cf == 1 else ch, cw if cf == 3 else cw // 2)] * 2


def random_planes(cf, cw, ch, stride, seed):
    """Strided planes [Y, Cb, Cr] of seeded random full-range bytes with planted extremes (rows,
    corners and scattered samples at 0 and 255); chroma stride = stride (4:4:4) or stride / 2."""
    rng = np.random.default_rng(seed)
    out = []
    for p, (h, w) in enumerate(plane_sizes(cf, cw, ch)):
        st = stride if (p == 0 or cf == 3) else stride // 2
        b = rng.integers(0, 256, (h, st), dtype=np.uint8)
        for v in (0, 255):
            b[rng.integers(0, h, 24), rng.integers(0, w, 24)] = v
        b[0, 0], b[0, w - 1], b[h - 1, 0], b[h - 1, w - 1] = 0, 255, 255, 0
        b[h // 2, : w // 2] = 255 * (p % 2)
        out.append(b)
    return out


def visible(planes, cf, cw, ch):
    return [b[:, :w] for b, (h, w) in zip(planes, plane_sizes(cf, cw, ch))]


class Planes:
    """Source planes on the device, exported with mp2vg_export_planes into a guarded buffer."""

    def __init__(self, planes):
        import torch
        self.torch = torch
        self.t = [torch.from_numpy(np.ascontiguousarray(b)).cuda() for b in planes]
        self.stride = [b.shape[1] for b in planes]

    def export(self, cf, cw, ch, exp, offset=0):
        """(exported bytes as a flat numpy array, guards untouched?)"""
        torch = self.torch
        w, h = exp.width or cw, exp.height or ch
        nbytes = 3 * w * h
        buf = torch.full((GUARD + 4 + nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 4 == 0
        at = GUARD + offset
        ptrs = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in self.t])
        _lib.check(_lib.lib().mp2vg_export_planes(0, ptrs, (ctypes.c_int32 * 3)(*self.stride), cf, cw, ch,
                                                  ctypes.byref(exp), ctypes.c_void_p(buf.data_ptr() + at), nbytes),
                   "export_planes")
        got = buf.cpu().numpy()
        clean = (got[:at] == FILL).all() and (got[at + nbytes:] == FILL).all()
        return got[at:at + nbytes], clean


def check_planes(src, planes_np, cf, cw, ch, layout, chroma, matrix, size, offset=0):
    exp = _lib.make_export(layout, chroma, matrix, size)
    got, clean = src.export(cf, cw, ch, exp, offset)
    want = M.export(visible(planes_np, cf, cw, ch), cf, matrix, chroma == "linear", layout == "nhwc", size)
    what = (cf, layout, chroma, matrix, size, offset)
    assert np.array_equal(got.reshape(want.shape), want), what
    assert clean, ("bytes outside dst written", what)


SIZES = [(48, 32), (47, 31), (46, 30), (45, 29), (2, 2), (1, 1)]


@pytest.mark.parametrize("cf,layout", itertools.product((1, 2, 3), ("nchw", "nhwc")))
def test_planes_all_combinations(cf, layout):
    """chroma format x layout x chroma mode x matrix x exported size, coded 48 x 32, stride 64."""
    planes = random_planes(cf, 48, 32, 64, seed=100 + cf)
    src = Planes(planes)
    for chroma, matrix, size in itertools.product(("nearest", "linear"), (1, 4, 5, 7), SIZES):
        check_planes(src, planes, cf, 48, 32, layout, chroma, matrix, size)


@pytest.mark.parametrize("layout", ("nchw", "nhwc"))
def test_planes_rows_longer_than_a_wave(layout):
    for cw, stride, widths in ((272, 320, (272, 271, 259, 257, 256, 255)), (528, 576, (527, 513))):
        planes = random_planes(1, cw, 32, stride, seed=cw)
        src = Planes(planes)
        for w in widths:
            check_planes(src, planes, 1, cw, 32, layout, "linear", 1, (w, 32))
            check_planes(src, planes, 1, cw, 32, layout, "linear", 5, (w, 31), offset=1)


@pytest.mark.parametrize("cf", (1, 2, 3))
def test_planes_dst_alignment_and_guards(cf):
    planes = random_planes(cf, 48, 32, 64, seed=200 + cf)
    src = Planes(planes)
    for layout, chroma, offset in itertools.product(("nchw", "nhwc"), ("nearest", "linear"), (0, 1, 2, 3)):
        check_planes(src, planes, cf, 48, 32, layout, chroma, 6, (45, 29), offset)
        check_planes(src, planes, cf, 48, 32, layout, chroma, 7, (3, 2), offset)


@pytest.mark.parametrize("matrix", (1, 4, 5, 7))
def test_planes_every_input_value(matrix):
    """A 4096 x 4096 4:4:4 frame holding every (Y, Cb, Cr) triple, NEAREST, planar."""
    import torch
    i = torch.arange(1 << 24, dtype=torch.int32, device="cuda").reshape(4096, 4096)
    t = [(i & 255).to(torch.uint8), ((i >> 8) & 255).to(torch.uint8), (i >> 16).to(torch.uint8)]
    out = torch.empty((3, 4096, 4096), dtype=torch.uint8, device="cuda")
    exp = _lib.make_export("nchw", "nearest", matrix)
    ptrs = (ctypes.c_void_p * 3)(*[x.data_ptr() for x in t])
    _lib.check(_lib.lib().mp2vg_export_planes(0, ptrs, (ctypes.c_int32 * 3)(4096, 4096, 4096), 3, 4096, 4096,
                                              ctypes.byref(exp), ctypes.c_void_p(out.data_ptr()), out.numel()),
               "export_planes")
    n = np.arange(1 << 24, dtype=np.int32).reshape(4096, 4096)
    want = np.stack(M.convert(n & 255, (n >> 8) & 255, n >> 16, matrix))
    assert np.array_equal(out.cpu().numpy(), want)


# ---- mp2vg_export_slots ------------------------------------------------------------------------

def gop(cf, seed):
    es = R.generate_es(width=176, height=144, chroma_format=cf, n_gops=1, gop_n=6, gop_m=3, seed=seed,
                       frame_pred_frame_dct=0)
    return R.Parsed(es, 176, 144, cf)


def decoded_frames(parsed):
    """The stream's frames by slot, from a context of their own."""
    with R.DeviceContext(176, 144, parsed.chroma_format, slots=parsed.npics) as ctx:
        ctx.upload(parsed.pics, parsed.mbs, parsed.coefs)
        ctx.decode()
        ctx.synchronize()
        return [ctx.download(s) for s in range(parsed.npics)]


def model_frames(frames, slots, cf, matrix, chroma, layout, size):
    one = {s: M.export(frames[s], cf, matrix, chroma == "linear", layout == "nhwc", size) for s in set(slots)}
    return np.stack([one[s] for s in slots])


@pytest.mark.parametrize("cf", (1, 2))
def test_slots_decoded_content(cf):
    """Decode, then export with no host synchronise in between; display order plus one repeat,
    cropped to 170 x 139."""
    parsed = gop(cf, seed=900 + cf)
    slots = [int(d) for d in parsed.display] + [int(parsed.display[1])]
    with R.DeviceContext(176, 144, cf, slots=parsed.npics) as ctx:
        ctx.upload(parsed.pics, parsed.mbs, parsed.coefs)
        ctx.decode()
        outs = {k: ctx.export_rgb(slots, layout=k[0], chroma=k[1], matrix=k[2], size=(170, 139), sync=False)
                for k in (("nchw", "linear", 1), ("nhwc", "linear", 5), ("nchw", "nearest", 7), ("nhwc", "nearest", 4))}
        ctx.synchronize()
        frames = [ctx.download(s) for s in range(parsed.npics)]
    for (layout, chroma, matrix), out in outs.items():
        assert tuple(out.shape) == ((7, 3, 139, 170) if layout == "nchw" else (7, 139, 170, 3))
        want = model_frames(frames, slots, cf, matrix, chroma, layout, (170, 139))
        assert np.array_equal(out.cpu().numpy(), want), (layout, chroma, matrix)


@pytest.mark.parametrize("cf,layout", ((1, "nchw"), (1, "nhwc"), (2, "nchw"), (2, "nhwc")))
def test_slots_dst_alignment_and_guards(cf, layout):
    """n = 3 frames of 45 x 29: frame starts (3 * 45 * 29 bytes apart) drift in alignment."""
    import torch
    parsed = gop(cf, seed=910 + cf)
    slots = np.array([2, 0, 2], np.int32)
    exp = _lib.make_export(layout, "linear", 1, (45, 29))
    nbytes = 3 * 3 * 45 * 29
    with R.DeviceContext(176, 144, cf, slots=parsed.npics) as ctx:
        ctx.upload(parsed.pics, parsed.mbs, parsed.coefs)
        ctx.decode()
        bufs = []
        for offset in range(4):
            buf = torch.full((GUARD + 4 + nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()  # the fill runs on torch's stream, the export on the context's
            _lib.check(_lib.lib().mp2vg_export_slots(ctx.h, slots.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), 3,
                                                     ctypes.byref(exp), ctypes.c_void_p(buf.data_ptr() + GUARD + offset),
                                                     nbytes), "export_slots")
            bufs.append(buf)
        ctx.synchronize()
        frames = [ctx.download(s) for s in range(parsed.npics)]
    want = model_frames(frames, [2, 0, 2], cf, 1, "linear", layout, (45, 29))
    for offset, buf in enumerate(bufs):
        got = buf.cpu().numpy()
        at = GUARD + offset
        assert np.array_equal(got[at:at + nbytes].reshape(want.shape), want), offset
        assert (got[:at] == FILL).all() and (got[at + nbytes:] == FILL).all(), offset


def test_slots_validation():
    """Argument checks that need a context: slot range, rectangle, dst_bytes, n."""
    import torch
    L = _lib.lib()
    buf = torch.zeros(3 * 176 * 144 * 2, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with R.DeviceContext(176, 144, 1, slots=4) as ctx:
        def call(slots, exp=None, nbytes=None, n=None, dst=buf.data_ptr()):
            s = np.array(slots, np.int32)
            e = exp or _lib.make_export()
            n = len(s) if n is None else n
            nbytes = n * 3 * (e.width or 176) * (e.height or 144) if nbytes is None else nbytes
            return L.mp2vg_export_slots(ctx.h, s.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), n, ctypes.byref(e),
                                        ctypes.c_void_p(dst), nbytes)
        assert call([0, 4]) == -1
        assert call([-1]) == -1
        assert call([0], n=0) == -1
        assert call([0], dst=0) == -1
        assert call([0], nbytes=3 * 176 * 144 + 1) == -1
        assert call([0], exp=_lib.make_export(size=(177, 144)), nbytes=3 * 176 * 144) == -1
        assert call([0], exp=_lib.make_export(matrix=2)) == -1
        assert L.mp2vg_export_slots(ctx.h, None, 1, ctypes.byref(_lib.make_export()), ctypes.c_void_p(buf.data_ptr()),
                                    3 * 176 * 144) == -1
        assert call([3, 0]) == 0
        ctx.synchronize()
        with pytest.raises(ValueError):
            ctx.export_rgb([0], out=torch.empty((1, 3, 144, 176), dtype=torch.float32, device="cuda"))
        with pytest.raises(ValueError):
            ctx.export_rgb([0], out=torch.empty((1, 3, 144, 180), dtype=torch.uint8, device="cuda")[..., :176])
        with pytest.raises(ValueError):
            ctx.export_rgb([0], out=torch.empty((1, 3, 144, 176), dtype=torch.uint8))
        out = torch.empty((1, 144, 176, 3), dtype=torch.uint8, device="cuda")
        assert ctx.export_rgb([0], out=out, layout="nhwc") is out


def test_slots_stream_ordering():
    """decode A, export A, decode B (same slots), export B, one synchronise: the export of A must
    have read A's frames (a batch waits for the exports enqueued before it), the export of B B's.
    The export of A is long (its slot list repeats 512 times), so a decode of B that did not wait
    would overwrite slots under it."""
    import torch
    a, b = gop(1, seed=921), gop(1, seed=922)
    assert a.npics == b.npics
    frames_a, frames_b = decoded_frames(a), decoded_frames(b)
    assert not np.array_equal(frames_a[0][0], frames_b[0][0])
    slots = np.tile(np.arange(a.npics, dtype=np.int32), 512)
    with R.DeviceContext(176, 144, 1, slots=a.npics) as ctx:
        out_a = torch.empty((len(slots), 144, 176, 3), dtype=torch.uint8, device="cuda")
        out_b = torch.empty_like(out_a)
        torch.cuda.synchronize()
        ctx.upload(a.pics, a.mbs, a.coefs)
        ctx.decode()
        ctx.export_rgb(slots, out=out_a, layout="nhwc", matrix=1, sync=False)
        ctx.upload(b.pics, b.mbs, b.coefs)
        ctx.decode()
        ctx.export_rgb(slots, out=out_b, layout="nhwc", matrix=1, sync=False)
        ctx.synchronize()
    idx = torch.from_numpy(slots.astype(np.int64)).cuda()
    for out, frames in ((out_a, frames_a), (out_b, frames_b)):
        want = torch.from_numpy(model_frames(frames, list(range(a.npics)), 1, 1, "linear", "nhwc", None)).cuda()
        assert torch.equal(out, want[idx])


def shifted(parsed, by):
    """The stream's picture records with every slot moved up by `by`."""
    pics = parsed.pics.copy()
    for k in ("dst_slot", "fwd_slot", "bwd_slot"):
        pics[k] = np.where(pics[k] >= 0, pics[k] + by, pics[k])
    return pics


def test_slots_export_then_batches_of_different_set_counts():
    """A long export of 18 slots, then a one-GOP batch (one picture set: one set stream) that
    overwrites slots 0-5, then a two-GOP batch (two sets: two set streams) that overwrites slots
    6-17, with no host synchronise anywhere.  Every set stream, also one that the first batch after
    the export did not use, must wait for the export before it overwrites slots: the exported
    frames are those of the first decode.  (Whether a missing wait shows depends on how the
    streams share the hardware queues; the test pins the sequence and its result.)"""
    import torch

    def stream(n_gops, seed):
        es = R.generate_es(width=176, height=144, chroma_format=1, n_gops=n_gops, gop_n=6, gop_m=3, seed=seed,
                           frame_pred_frame_dct=0)
        return R.Parsed(es, 176, 144, 1)

    a, b1, b2 = stream(3, 931), stream(1, 932), stream(2, 933)
    assert (a.npics, b1.npics, b2.npics) == (18, 6, 12)
    frames_a = decoded_frames(a)
    frames_b = decoded_frames(b1) + decoded_frames(b2)
    assert all(not np.array_equal(fa[0], fb[0]) for fa, fb in zip(frames_a, frames_b))
    slots = np.tile(np.arange(18, dtype=np.int32), 256)  # 350 MB of output: a long export
    with R.DeviceContext(176, 144, 1, slots=18) as ctx:
        out_a = torch.empty((len(slots), 144, 176, 3), dtype=torch.uint8, device="cuda")
        out_b = torch.empty((18, 144, 176, 3), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.upload(a.pics, a.mbs, a.coefs)
        ctx.decode()
        ctx.export_rgb(slots, out=out_a, layout="nhwc", sync=False)
        ctx.upload(b1.pics, b1.mbs, b1.coefs)
        ctx.decode()
        ctx.upload(shifted(b2, 6), b2.mbs, b2.coefs)
        ctx.decode()
        ctx.export_rgb(np.arange(18, dtype=np.int32), out=out_b, layout="nhwc", sync=False)
        ctx.synchronize()
    want_a = torch.from_numpy(model_frames(frames_a, list(range(18)), 1, 1, "linear", "nhwc", None)).cuda()
    want_a = want_a.repeat(64, 1, 1, 1)
    for k in range(0, len(slots), len(want_a)):
        assert torch.equal(out_a[k:k + len(want_a)], want_a), k
    want_b = model_frames(frames_b, list(range(18)), 1, 1, "linear", "nhwc", None)
    assert np.array_equal(out_b.cpu().numpy(), want_b)


# ---- Python interface ----------------------------------------------------------------------------

def host_frames(es, w, h, cf):
    """Display-order [Y, Cb, Cr] visible planes from the host-frame drop-in decoder, and its
    sequence header."""
    got = []

    def render(frame):
        got.append([frame.get_planes(i)[:, :frame.get_width(i)].copy() for i in range(3)])

    d = mp2v_decoder_c(decoder_config_t(w, h, cf), render)
    d.decode(es, len(es))
    sh = d.m_sequence_header
    d.close()
    return got, sh


def test_frame_export_rgb_in_the_render_callback():
    e = next(m for m in load_manifest() if m["name"] == "ipb422_qcif")
    es = read_stream(e)
    w, h, cf = e["width"], e["height"], e["chroma_format"]
    frames, _ = host_frames(es, w, h, cf)
    got = []

    def render(frame):
        layout = "nhwc" if len(got) % 2 else "nchw"
        t = frame.export_rgb(layout=layout, chroma="linear", matrix=5, size=(171, 143))
        got.append((layout, t))

    d = mp2v_decoder_c(decoder_config_t(w, h, cf, device_frames=True), render)
    d.decode(es, len(es))
    d.close()
    assert len(got) == len(frames) == e["frames"]
    for (layout, t), planes in zip(got, frames):
        want = M.export(planes, cf, 5, True, layout == "nhwc", (171, 143))
        assert np.array_equal(t.cpu().numpy()[0], want)

    def host_render(frame):
        with pytest.raises(ValueError):
            frame.export_rgb()

    d = mp2v_decoder_c(decoder_config_t(w, h, cf), host_render)
    d.decode(es, len(es))
    d.close()


def test_decode_rgb_golden_stream():
    import tiny_mp2v_dec_amd
    e = next(m for m in load_manifest() if m["name"] == "ipb420_qcif")
    es = read_stream(e)
    w, h, cf = e["width"], e["height"], e["chroma_format"]
    frames, sh = host_frames(es, w, h, cf)
    sw, sv = int(sh.horizontal_size_value), int(sh.vertical_size_value)
    size = (sw, sv) if 0 < sw <= w and 0 < sv <= h else None
    out = tiny_mp2v_dec_amd.decode_rgb(es, w, h, cf, layout="nhwc", chroma="linear")
    want = np.stack([M.export(p, cf, 1, True, True, size) for p in frames])
    assert str(out.device) == "cuda:0" and tuple(out.shape) == want.shape
    assert np.array_equal(out.cpu().numpy(), want)
    out = tiny_mp2v_dec_amd.decode_rgb(es, w, h, cf, layout="nchw", chroma="nearest", matrix=7)
    want = np.stack([M.export(p, cf, 7, False, False, size) for p in frames])
    assert np.array_equal(out.cpu().numpy(), want)


def test_decode_rgb_in_several_calls_and_without_pictures(monkeypatch):
    """decode_rgb exports at most EXPORT_MAX_FRAMES slots per call: with the limit lowered the
    tensor is the same.  A stream of headers alone gives an empty tensor of the right shape."""
    import tiny_mp2v_dec_amd
    e = next(m for m in load_manifest() if m["name"] == "ipb420_qcif")
    es = read_stream(e)
    w, h, cf = e["width"], e["height"], e["chroma_format"]
    whole = tiny_mp2v_dec_amd.decode_rgb(es, w, h, cf, layout="nhwc")
    monkeypatch.setattr(R, "EXPORT_MAX_FRAMES", 5)
    parts = tiny_mp2v_dec_amd.decode_rgb(es, w, h, cf, layout="nhwc")
    assert parts.shape[0] == e["frames"] and np.array_equal(parts.cpu().numpy(), whole.cpu().numpy())
    empty = tiny_mp2v_dec_amd.decode_rgb(es[:es.find(b"\x00\x00\x01\x00")], w, h, cf)
    assert tuple(empty.shape) == (0, 3, h, w) and str(empty.device) == "cuda:0"
