"""GPU: the tensor export kernel (tensor.hip) through mp2vg_tensor_planes, mp2vg_tensor_slots and the
Python interface.  Every comparison is array_equal on bit patterns against the numpy model
(tests/tensor_model.py): the arithmetic is a bit-exact contract."""
import ctypes
import itertools

import numpy as np
import pytest

import export_model
import tensor_model as T
from conftest import load_manifest, read_stream
from test_gpu_export import FILL, GUARD, decoded_frames, gop, host_frames, random_planes, shifted, visible
from tiny_mp2v_dec_amd import _lib
from tiny_mp2v_dec_amd import records as R
from tiny_mp2v_dec_amd.decoder import decoder_config_t, mp2v_decoder_c

pytestmark = pytest.mark.gpu

E_INVALID = -1
ELEM = {"uint8": 1, "float16": 2, "bfloat16": 2, "float32": 4}
IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
# mean / std per dtype in the sweeps: uint8 takes none, bfloat16 the default x / 255
NORM = {"uint8": (None, None), "float16": IMAGENET, "bfloat16": (None, None), "float32": IMAGENET}


def ratio_ok(src, out):
    return src <= 32 * out


class Source:
    """Source planes on the device, exported with mp2vg_tensor_planes into a guarded buffer; the
    model's Q image of each (chroma, size, crop) is computed once and shared by the dtypes and
    layouts."""

    def __init__(self, planes, cf, cw, ch):
        import torch
        self.torch = torch
        self.t = [torch.from_numpy(np.ascontiguousarray(b)).cuda() for b in planes]
        self.stride = [b.shape[1] for b in planes]
        self.cf, self.cw, self.ch = cf, cw, ch
        self.vis = visible(planes, cf, cw, ch)
        self.q = {}

    def call(self, t, offset=0):
        """(status, result bytes as a flat uint8 array, guards untouched?); offset in elements."""
        torch = self.torch
        elem = (1, 2, 2, 4)[t.dtype]
        nbytes = 3 * t.out_w * t.out_h * elem
        buf = torch.full((GUARD + 16 + nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 16 == 0
        at = GUARD + offset * elem
        ptrs = (ctypes.c_void_p * 3)(*[x.data_ptr() for x in self.t])
        rc = _lib.lib().mp2vg_tensor_planes(0, ptrs, (ctypes.c_int32 * 3)(*self.stride), self.cf, self.cw, self.ch,
                                            ctypes.byref(t), ctypes.c_void_p(buf.data_ptr() + at), nbytes)
        got = buf.cpu().numpy()
        clean = (got[:at] == FILL).all() and (got[at + nbytes:] == FILL).all()
        return rc, got[at:at + nbytes], clean

    def model_q(self, matrix, chroma, size, crop):
        key = (matrix, chroma, size, crop)
        if key not in self.q:
            self.q[key] = T.q_image(self.vis, self.cf, matrix, chroma == "linear", size, crop)
        return self.q[key]

    def check(self, size, crop=None, dtype="uint8", mean=None, std=None, layout="nchw", chroma="linear", matrix=1,
              offset=0, scale_bias=None):
        """One export against the model, or MP2VG_E_INVALID where an axis shrinks by more than 32."""
        t = _lib.make_tensor(size, crop, dtype, mean, std, layout, chroma, matrix)
        if scale_bias is not None:
            for c in range(3):
                t.scale[c], t.bias[c] = float(scale_bias[0][c]), float(scale_bias[1][c])
        what = (self.cf, size, crop, dtype, layout, chroma, matrix, offset)
        sw, sh = (self.cw, self.ch) if crop is None else crop[2:]
        rc, got, clean = self.call(t, offset)
        if not (ratio_ok(sw, size[0]) and ratio_ok(sh, size[1])):
            assert rc == E_INVALID and clean and (got == FILL).all(), what
            return None
        assert rc == 0, (what, _lib.lib().mp2vg_last_error())
        q = self.model_q(matrix, chroma, size, crop)
        want = T.normalise(q, dtype, np.array(t.scale, np.float32), np.array(t.bias, np.float32))
        if layout == "nhwc":
            want = np.moveaxis(want, 0, -1)
        assert np.array_equal(T.bits(got, dtype).reshape(want.shape), want), what
        assert clean, ("bytes outside dst written", what)
        return q


SIZES = [(10, 7), (47, 31), (48, 32), (77, 50), (1, 1)]
CROPS = [None, (1, 1, 45, 29), (5, 3, 16, 9)]


@pytest.mark.parametrize("cf,layout", itertools.product((1, 2, 3), ("nchw", "nhwc")))
def test_planes_all_combinations(cf, layout):
    """chroma format x layout x chroma mode x dtype x output size x crop, coded 48 x 32, stride 64.
    (1, 1) from the whole frame (48:1) and from the 45 x 29 crop (45:1) is above the 32:1 limit:
    those calls must be refused before anything is written."""
    src = Source(random_planes(cf, 48, 32, 64, seed=300 + cf), cf, 48, 32)
    for chroma, dtype, size, crop in itertools.product(("nearest", "linear"), T.DTYPES, SIZES, CROPS):
        src.check(size, crop, dtype, *NORM[dtype], layout=layout, chroma=chroma, matrix=5 if dtype == "bfloat16" else 1)


@pytest.mark.parametrize("cf", (1, 2, 3))
def test_planes_32_to_1(cf):
    """coded 96 x 64 -> 3 x 2: 32:1 on both axes; the middle column has the 64 taps of the extreme
    (the outer columns and both rows are cut to 48 by the frame's edges)."""
    src = Source(random_planes(cf, 96, 64, 128, seed=320 + cf), cf, 96, 64)
    assert _lib.tensor_weights(96, 3)[1].tolist() == [48, 64, 48] and _lib.tensor_weights(64, 2)[1].tolist() == [48, 48]
    for layout, chroma, dtype in itertools.product(("nchw", "nhwc"), ("nearest", "linear"), T.DTYPES):
        src.check((3, 2), None, dtype, *NORM[dtype], layout=layout, chroma=chroma)


@pytest.mark.parametrize("layout", ("nchw", "nhwc"))
def test_planes_rows_longer_than_a_wave_and_a_workgroup_pass(layout):
    """Rows of more source units and of more output elements than the workgroup's 256 lanes."""
    for cw, stride in ((272, 320), (528, 576)):
        src = Source(random_planes(1, cw, 32, stride, seed=cw), 1, cw, 32)
        for w in (271, 257, 130, 17):
            src.check((w, 32), None, "uint8", layout=layout)
            src.check((w, 13), (3, 1, cw - 5, 30), "float16", *IMAGENET, layout=layout, matrix=5, offset=1)


def test_planes_rows_of_several_segments():
    """A source row wider than the 2048 columns a workgroup keeps: the row is split into segments
    of output columns (identity, downscale, and the 32:1 limit where a tap range is 65 wide)."""
    cw = 4128
    for cf in (1, 3):
        src = Source(random_planes(cf, cw, 16, cw + 32, seed=330 + cf), cf, cw, 16)
        for w, crop in ((4128, None), (1000, None), (129, None), (4099, (7, 1, 4099, 13))):
            src.check((w, 5), crop, "float32", *IMAGENET, layout="nhwc")
        src.check((4128, 16), None, "uint8", layout="nchw")


@pytest.mark.parametrize("cf", (1, 2, 3))
def test_planes_dst_offsets_and_guards(cf):
    """dst one and three elements past an aligned address, odd out_w: the guards on both sides
    stay untouched (dst is aligned to the element size and no more)."""
    src = Source(random_planes(cf, 48, 32, 64, seed=340 + cf), cf, 48, 32)
    for layout, dtype, offset in itertools.product(("nhwc", "nchw"), T.DTYPES, (0, 1, 3)):
        src.check((45, 29), None, dtype, *NORM[dtype], layout=layout, offset=offset)
        src.check((7, 5), (5, 3, 16, 9), dtype, *NORM[dtype], layout=layout, chroma="nearest", offset=offset)


def ramp_frame():
    """4:4:4 256 x 8: luma ramps under several constant and one ramping chroma, so that upscaled
    64 times horizontally the three channels pass through every value of Q."""
    x = np.arange(256)
    Y = np.stack([x, x[::-1], (x * 7) % 256, x, x, x[::-1], x, x]).astype(np.uint8)
    Cb = np.full((8, 256), 128, np.uint8)
    Cr = Cb.copy()
    Cb[3], Cr[4], Cb[5], Cr[6], Cr[7] = 100, 160, 200, 90, x
    return [Y, Cb, Cr]


def test_normalise_every_q_value():
    """ImageNet mean / std, a scale whose float16 result overflows to infinity, and a bias that makes
    results negative, on an image whose Q takes every value 0..16320 (asserted from the model)."""
    src = Source(ramp_frame(), 3, 256, 8)
    cases = [("float16", T.scale_bias(*IMAGENET)), ("bfloat16", T.scale_bias(*IMAGENET)),
             ("float32", T.scale_bias(*IMAGENET)),
             ("float16", (np.float32([300.0, 257.0, 1000.0]), np.float32([0.0, -70000.0, 0.125]))),  # to +-inf
             ("bfloat16", (np.float32([3e36, 1.0, 1e-40]), np.float32([0.0, -300.0, 0.0]))),         # float32 inf, subnormal
             ("float32", (np.float32([1 / 3, -0.7, 2.0 ** -140]), np.float32([-50.0, 0.1, 0.0]))),   # negative, subnormal
             ("float16", (np.float32([2.0 ** -20] * 3), np.float32([0.0, -2.0 ** -14, 2.0 ** -24]))),  # float16 subnormals
             ("uint8", None)]
    seen = np.zeros(T.QMAX + 1, bool)
    for layout, (dtype, sb) in itertools.product(("nchw", "nhwc"), cases):
        q = src.check((16384, 8), None, dtype, layout=layout, chroma="nearest", scale_bias=sb)
        seen[np.unique(q)] = True
    assert seen.all(), np.flatnonzero(~seen)[:20]
    inf16 = T.lut(*cases[3][1], "float16")
    assert (inf16[0] == 0x7C00).any() and (inf16[1] == 0xFC00).any() and (inf16[2] == 0x7C00).any()
    assert (T.lut(*cases[4][1], "float32")[0] == 0x7F800000).any()
    assert (T.lut(*cases[5][1], "float32").view(np.float32)[0] < 0).any()


# ---- mp2vg_tensor_slots ----------------------------------------------------------------------------

def model_tensor(frames, slots, cf, matrix, chroma, layout, size, crop, dtype, mean, std):
    s, b = T.scale_bias(mean, std, dtype)
    one = {k: T.tensor(frames[k], cf, matrix, chroma == "linear", layout == "nhwc", size, crop, dtype, s, b)
           for k in set(slots)}
    return np.stack([one[k] for k in slots])


@pytest.mark.parametrize("cf", (1, 2))
def test_slots_decoded_content(cf):
    """Decode, then export with no host synchronise in between: a permuted slot list with a repeat.
    The identity-size uint8 tensor is the RGB export's bytes."""
    import torch
    parsed = gop(cf, seed=940 + cf)
    slots = [int(d) for d in parsed.display][::-1] + [int(parsed.display[1])]
    kinds = (("nchw", "linear", 1, (50, 40), None, "float16", *IMAGENET),
             ("nhwc", "linear", 5, (64, 36), (3, 5, 170, 135), "bfloat16", None, None),
             ("nchw", "nearest", 7, (200, 150), (0, 0, 170, 139), "float32", *IMAGENET),
             ("nhwc", "nearest", 4, (176, 144), None, "uint8", None, None))
    with R.DeviceContext(176, 144, cf, slots=parsed.npics) as ctx:
        ctx.upload(parsed.pics, parsed.mbs, parsed.coefs)
        ctx.decode()
        outs = [ctx.export_tensor(slots, k[3], crop=k[4], dtype=k[5], mean=k[6], std=k[7], layout=k[0], chroma=k[1],
                                  matrix=k[2], sync=False) for k in kinds]
        rgb = ctx.export_rgb(slots, layout="nhwc", chroma="nearest", matrix=4, sync=False)
        ctx.synchronize()
        frames = [ctx.download(s) for s in range(parsed.npics)]
    for (layout, chroma, matrix, size, crop, dtype, mean, std), out in zip(kinds, outs):
        assert str(out.dtype) == "torch." + dtype
        assert tuple(out.shape) == ((7, 3, size[1], size[0]) if layout == "nchw" else (7, size[1], size[0], 3))
        want = model_tensor(frames, slots, cf, matrix, chroma, layout, size, crop, dtype, mean, std)
        got = out.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[ELEM[dtype]])
        assert np.array_equal(T.bits(got.cpu().numpy(), dtype), want), (layout, chroma, matrix, dtype)
    assert np.array_equal(outs[3].cpu().numpy(), rgb.cpu().numpy())


def test_slots_validation():
    """Argument checks that need a context: slot range, rectangle, ratio, dst_bytes, alignment, n."""
    import torch
    L = _lib.lib()
    buf = torch.zeros(3 * 176 * 144 * 4 * 2, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with R.DeviceContext(176, 144, 1, slots=4) as ctx:
        def call(slots, t=None, nbytes=None, n=None, dst=buf.data_ptr()):
            s = np.array(slots, np.int32)
            t = t or _lib.make_tensor((44, 36))
            n = len(s) if n is None else n
            nbytes = n * 3 * t.out_w * t.out_h * (1, 2, 2, 4)[t.dtype] if nbytes is None else nbytes
            return L.mp2vg_tensor_slots(ctx.h, s.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), n, ctypes.byref(t),
                                        ctypes.c_void_p(dst), nbytes)
        assert call([0, 4]) == -1
        assert call([-1]) == -1
        assert call([0], n=0) == -1
        assert call([0], dst=0) == -1
        assert call([0], dst=buf.data_ptr() + 1) == -1
        assert call([0], nbytes=3 * 44 * 36 * 2 + 2) == -1
        assert call([0], t=_lib.make_tensor((44, 36), (0, 0, 177, 144))) == -1
        assert call([0], t=_lib.make_tensor((5, 36))) == -1  # 176 / 5 above 32
        assert call([0], t=_lib.make_tensor((44, 36), matrix=2)) == -1
        assert L.mp2vg_tensor_slots(ctx.h, None, 1, ctypes.byref(_lib.make_tensor((44, 36))),
                                    ctypes.c_void_p(buf.data_ptr()), 3 * 44 * 36 * 2) == -1
        assert call([3, 0]) == 0
        ctx.synchronize()
        with pytest.raises(ValueError):
            ctx.export_tensor([0], (44, 36), out=torch.empty((1, 3, 36, 44), dtype=torch.float32, device="cuda"))
        with pytest.raises(ValueError):
            ctx.export_tensor([0], (44, 36), out=torch.empty((1, 3, 36, 48), dtype=torch.float16, device="cuda")[..., :44])
        with pytest.raises(ValueError):
            ctx.export_tensor([0], (44, 36), out=torch.empty((1, 3, 36, 44), dtype=torch.float16))
        out = torch.empty((1, 36, 44, 3), dtype=torch.bfloat16, device="cuda")
        assert ctx.export_tensor([0], (44, 36), dtype=torch.bfloat16, layout="nhwc", out=out) is out


def rgb_frames(frames, n):
    return np.stack([export_model.export(frames[s], 1, 1, True, True) for s in range(n)])


def test_slots_stream_ordering():
    """decode A, tensor export A, decode B (same slots), tensor export B, one synchronise: the export
    of A must have read A's frames (a batch waits for the exports enqueued before it), the export
    of B B's.  The export of A is long (its slot list repeats 512 times), so a decode of B that did
    not wait would overwrite slots under it.  Identity size, uint8: the RGB export's bytes."""
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
        ctx.export_tensor(slots, (176, 144), dtype="uint8", layout="nhwc", out=out_a, sync=False)
        ctx.upload(b.pics, b.mbs, b.coefs)
        ctx.decode()
        ctx.export_tensor(slots, (176, 144), dtype="uint8", layout="nhwc", out=out_b, sync=False)
        ctx.synchronize()
    idx = torch.from_numpy(slots.astype(np.int64)).cuda()
    for out, frames in ((out_a, frames_a), (out_b, frames_b)):
        want = torch.from_numpy(rgb_frames(frames, a.npics)).cuda()
        assert torch.equal(out, want[idx])


def test_slots_export_then_batches_of_different_set_counts():
    """A long tensor export of 18 slots, then a one-GOP batch (one set stream) that overwrites slots
    0-5, then a two-GOP batch (two set streams) that overwrites slots 6-17, with no host
    synchronise anywhere: the exported frames are those of the first decode, and a tensor export
    after the batches sees theirs (resized, against the model)."""
    import torch

    def stream(n_gops, seed):
        es = R.generate_es(width=176, height=144, chroma_format=1, n_gops=n_gops, gop_n=6, gop_m=3, seed=seed,
                           frame_pred_frame_dct=0)
        return R.Parsed(es, 176, 144, 1)

    a, b1, b2 = stream(3, 931), stream(1, 932), stream(2, 933)
    assert (a.npics, b1.npics, b2.npics) == (18, 6, 12)
    frames_a = decoded_frames(a)
    frames_b = decoded_frames(b1) + decoded_frames(b2)
    slots = np.tile(np.arange(18, dtype=np.int32), 256)
    with R.DeviceContext(176, 144, 1, slots=18) as ctx:
        out_a = torch.empty((len(slots), 144, 176, 3), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.upload(a.pics, a.mbs, a.coefs)
        ctx.decode()
        ctx.export_tensor(slots, (176, 144), dtype="uint8", layout="nhwc", out=out_a, sync=False)
        ctx.upload(b1.pics, b1.mbs, b1.coefs)
        ctx.decode()
        ctx.upload(shifted(b2, 6), b2.mbs, b2.coefs)
        ctx.decode()
        out_b = ctx.export_tensor(np.arange(18, dtype=np.int32), (44, 36), dtype="float32", mean=IMAGENET[0],
                                  std=IMAGENET[1], layout="nhwc", sync=False)
        ctx.synchronize()
    want_a = torch.from_numpy(rgb_frames(frames_a, 18)).cuda().repeat(64, 1, 1, 1)
    for k in range(0, len(slots), len(want_a)):
        assert torch.equal(out_a[k:k + len(want_a)], want_a), k
    want_b = model_tensor(frames_b, list(range(18)), 1, 1, "linear", "nhwc", (44, 36), None, "float32", *IMAGENET)
    assert np.array_equal(T.bits(out_b.cpu().numpy(), "float32"), want_b)


# ---- Python interface ------------------------------------------------------------------------------

def test_decode_tensor_golden_stream():
    import torch
    import tiny_mp2v_dec_amd
    e = next(m for m in load_manifest() if m["name"] == "ipb420_qcif")
    es = read_stream(e)
    w, h, cf = e["width"], e["height"], e["chroma_format"]
    frames, sh = host_frames(es, w, h, cf)
    sw, sv = int(sh.horizontal_size_value), int(sh.vertical_size_value)
    crop = (0, 0, sw, sv) if 0 < sw <= w and 0 < sv <= h else None
    out = tiny_mp2v_dec_amd.decode_tensor(es, w, h, cf, (56, 48), dtype=torch.float16, mean=IMAGENET[0], std=IMAGENET[1])
    want = model_tensor(frames, list(range(len(frames))), cf, 1, "linear", "nchw", (56, 48), crop, "float16", *IMAGENET)
    assert str(out.device) == "cuda:0" and out.dtype == torch.float16 and tuple(out.shape) == want.shape
    assert np.array_equal(T.bits(out.view(torch.int16).cpu().numpy(), "float16"), want)
    out = tiny_mp2v_dec_amd.decode_tensor(es, w, h, cf, (40, 30), crop=(11, 7, 120, 90), dtype="uint8", layout="nhwc",
                                          chroma="nearest", matrix=7)
    want = model_tensor(frames, list(range(len(frames))), cf, 7, "nearest", "nhwc", (40, 30), (11, 7, 120, 90), "uint8",
                        None, None)
    assert np.array_equal(out.cpu().numpy(), want)
    empty = tiny_mp2v_dec_amd.decode_tensor(es[:es.find(b"\x00\x00\x01\x00")], w, h, cf, (56, 48))
    assert tuple(empty.shape) == (0, 3, 48, 56) and empty.dtype == torch.float16


def test_frame_export_tensor_in_the_render_callback():
    import torch
    e = next(m for m in load_manifest() if m["name"] == "ipb422_qcif")
    es = read_stream(e)
    w, h, cf = e["width"], e["height"], e["chroma_format"]
    frames, _ = host_frames(es, w, h, cf)
    got = []

    def render(frame):
        layout = "nhwc" if len(got) % 2 else "nchw"
        got.append((layout, frame.export_tensor((60, 45), crop=(1, 1, 171, 141), dtype=torch.bfloat16, mean=IMAGENET[0],
                                                std=IMAGENET[1], layout=layout, matrix=5)))

    d = mp2v_decoder_c(decoder_config_t(w, h, cf, device_frames=True), render)
    d.decode(es, len(es))
    d.close()
    assert len(got) == len(frames) == e["frames"]
    for (layout, t), planes in zip(got, frames):
        want = model_tensor([planes], [0], cf, 5, "linear", layout, (60, 45), (1, 1, 171, 141), "bfloat16", *IMAGENET)
        assert np.array_equal(T.bits(t.view(torch.int16).cpu().numpy(), "bfloat16"), want)

    def host_render(frame):
        with pytest.raises(ValueError):
            frame.export_tensor((60, 45))

    d = mp2v_decoder_c(decoder_config_t(w, h, cf), host_render)
    d.decode(es, len(es))
    d.close()
