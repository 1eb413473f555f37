"""GPU: the residual export (residual.hip through mp2vg_residual_batch / DeviceContext.export_residual)
against the numpy model of its definition (tests/residual_model.py, the oracle's entry points) and
against the reconstruct kernels (two decodes over constant reference slots), array_equal
everywhere.  Every destination is prefilled with FILL and sits between guard bytes that are checked
afterwards."""
import ctypes
import json
import os

import numpy as np
import pytest

import directed_idct as I
import residual_model as RM
import slot_state as SS
from conftest import GOLDEN, load_manifest, read_stream
from helpers import oracle_frames
from test_gpu_export import FILL, GUARD
from test_gpu_motion import dense_batch, drop_words
from tiny_mp2v_dec_amd import _lib
from tiny_mp2v_dec_amd import records as R
from tiny_mp2v_dec_amd._lib import MB_FWD, MB_INTRA

pytestmark = pytest.mark.gpu

MANIFEST = {e["name"]: e for e in load_manifest()}
E_INVALID, E_STATE = -1, -5
CODES = {"int16": 0, "int8": 1}


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    """torch brings its own HIP runtime: it is loaded and initialised before this module's first
    context, the order decode_residual uses (an export's tensors exist first)."""
    import torch
    torch.cuda.init()


class Src:
    """Records (of a stream, or hand-built) with the model of every picture, computed once."""

    def __init__(self, es, w, h, cf, records=None):
        self.es, self.w, self.h, self.cf = es, w, h, cf
        if records is None:
            self.parsed = R.Parsed(es, w, h, cf)
            records = (self.parsed.pics, self.parsed.mbs, self.parsed.coefs)
        self.pics, self.mbs, self.coefs = records
        self.npics = len(self.pics)
        self._want = {}

    def want(self, dtype="int16", zero_intra=False):
        key = (dtype, zero_intra)
        if key not in self._want:
            self._want[key] = RM.model(self.pics, self.mbs, self.coefs, self.w, self.h, self.cf, dtype=dtype,
                                       zero_intra=zero_intra)
        return self._want[key]

    def context(self, slots=None):
        return R.DeviceContext(self.w, self.h, self.cf, slots=slots or self.npics)

    def upload(self, ctx, path):
        if path == "es":
            with R.Scan(self.es, self.w, self.h, self.cf) as scan:
                ctx.upload_es(scan)
        else:
            ctx.upload(self.pics, self.mbs, self.coefs)


_cache = {}


def golden(name):
    if name not in _cache:
        e = MANIFEST[name]
        _cache[name] = Src(read_stream(e), e["width"], e["height"], e["chroma_format"])
    return _cache[name]


def generated(w, h, cf, **kw):
    key = (w, h, cf, tuple(sorted(kw.items())))
    if key not in _cache:
        args = dict(width=w, height=h, chroma_format=cf, n_gops=1, gop_n=4, gop_m=2, seed=3, frame_pred_frame_dct=0,
                    big_level_permille=200)
        args.update(kw)
        _cache[key] = Src(R.generate_es(**args), w, h, cf)
    return _cache[key]


def raw_export(ctx, order, dtype="int16", flags=0, outputs=(True, True, True), offset=0, n=None, sizes=None, code=None):
    """mp2vg_residual_batch itself into guarded buffers at data_ptr + GUARD + offset.  Returns
    (status, [array or None per plane], guards and unwanted buffers untouched?, [destination bytes
    untouched? per plane])."""
    import torch
    order = np.ascontiguousarray(order, np.int32)
    n = len(order) if n is None else n
    shp = _lib.residual_shapes(ctx.width, ctx.height, ctx.chroma_format, max(len(order), 1))
    nbytes = [int(np.prod(s)) * np.dtype(dtype).itemsize for s in shp]
    bufs = [torch.full((GUARD + offset + b + GUARD,), FILL, dtype=torch.uint8, device="cuda") for b in nbytes]
    torch.cuda.synchronize()
    ptrs = [ctypes.c_void_p(t.data_ptr() + GUARD + offset) if want else None for t, want in zip(bufs, outputs)]
    given = (ctypes.c_uint64 * 3)(*(nbytes if sizes is None else sizes))
    rc = _lib.lib().mp2vg_residual_batch(ctx.h, order.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), n,
                                         CODES[dtype] if code is None else code, flags, ptrs[0], ptrs[1], ptrs[2], given)
    ctx.synchronize()
    host = [t.cpu().numpy() for t in bufs]
    at = GUARD + offset
    clean = all((b[:at] == FILL).all() and (b[at + nb:] == FILL).all() and (want or (b == FILL).all())
                for b, nb, want in zip(host, nbytes, outputs))
    got = [b[at:at + nb].copy().view(dtype).reshape(s) if want else None
           for b, nb, s, want in zip(host, nbytes, shp, outputs)]
    fresh = [(b[at:at + nb] == FILL).all() for b, nb in zip(host, nbytes)]
    return rc, got, clean, fresh


def first_difference(g, w):
    f, y, x = [int(t[0]) for t in np.nonzero(g != w)]
    return "%d samples differ, first at picture %d line %d column %d (MB %d, %d): got %d, expected %d" % (
        int((g != w).sum()), f, y, x, x // 16, y // 16, g[f, y, x], w[f, y, x])


def check(ctx, src, order, dtype="int16", zero_intra=False, outputs=(True, True, True)):
    rc, got, clean, _ = raw_export(ctx, order, dtype, 1 if zero_intra else 0, outputs)
    assert rc == 0, _lib.lib().mp2vg_last_error()
    assert clean
    idx = np.asarray(order, np.int64)
    for name, g, w in zip(("y", "cb", "cr"), got, src.want(dtype, zero_intra)):
        if g is not None:
            assert g.dtype == w.dtype
            assert np.array_equal(g, w[idx]), (name, dtype, first_difference(g, w[idx]))


def check_all(ctx, src, order):
    """int16 and int8, with and without chroma, luma alone and chroma alone."""
    check(ctx, src, order)
    check(ctx, src, order, "int8")
    check(ctx, src, order, outputs=(True, False, False))
    check(ctx, src, order, "int8", outputs=(False, True, True))


@pytest.mark.parametrize("path", ["records", "es"])
@pytest.mark.parametrize("name", sorted(MANIFEST))
def test_golden_streams_by_both_upload_paths(name, path):
    s = golden(name)
    display = [int(d) for d in s.parsed.display]
    with s.context() as ctx:
        s.upload(ctx, path)
        check_all(ctx, s, display)
        # the Python entry point: every picture in batch order
        for dtype in ("int16", "int8"):
            got = ctx.export_residual(dtype=dtype)
            for g, w in zip(got, s.want(dtype)):
                assert np.array_equal(g.cpu().numpy(), w)
        y, cb, cr = ctx.export_residual([display[0]], chroma=False)
        assert cb is None and cr is None and np.array_equal(y.cpu().numpy(), s.want()[0][[display[0]]])


@pytest.mark.parametrize("cf", [1, 2, 3])
@pytest.mark.parametrize("size", [16, 48])
@pytest.mark.parametrize("path", ["records", "es"])
def test_smallest_geometries(size, cf, path):
    """One MB, and 3 x 3 MBs: a partial row tile."""
    s = generated(size, size, cf)
    with s.context() as ctx:
        s.upload(ctx, path)
        check_all(ctx, s, list(range(s.npics)) + [1])


@pytest.mark.parametrize("cf", [1, 2, 3])
@pytest.mark.parametrize("mbw", [3, 4, 5, 7, 8, 9, 17])
@pytest.mark.parametrize("path", ["records", "es"])
def test_row_widths(mbw, cf, path):
    """One MB row of 3, 4, 5 and 9 MBs: a partial 4-MB group of the word layout, a full one, one
    more, two and one.  The kernel tiles a row at 8 MBs per workgroup: 7, 8 and 9 are one partial
    tile, one full tile and a full tile with a one-MB tile behind it; 17 is two full tiles and one
    MB."""
    s = generated(16 * mbw, 16, cf)
    with s.context() as ctx:
        s.upload(ctx, path)
        check(ctx, s, list(range(s.npics)))
        check(ctx, s, list(range(s.npics)), "int8")


IDCT_SIZES = [(128, 16), (80, 32)]


def _directed(bt):
    key = ("directed",) + bt.key()
    if key not in _cache:
        _cache[key] = Src(None, bt.width, bt.height, bt.cf, (bt.pics, bt.mbs, bt.coefs))
    return _cache[key]


@pytest.mark.parametrize("cf", [1, 2, 3])
@pytest.mark.parametrize("launch", ["I", "P", "B", "mixed"])
@pytest.mark.parametrize("size", IDCT_SIZES, ids=lambda s: "%dx%d" % s)
def test_idct_witnesses(cf, launch, size):
    """The saturating witness vectors of every node of both passes in every coded-block slot, MB
    kind and DCT type, through the export's own transform; 80 wide: a tile of 5 MBs."""
    s = _directed(I.idct_batch(size[0], size[1], cf, launch))
    with s.context() as ctx:
        s.upload(ctx, "records")
        check(ctx, s, list(range(s.npics)))
        check(ctx, s, list(range(s.npics)), "int8", outputs=(True, False, False))


@pytest.mark.parametrize("cf", [1, 2, 3])
@pytest.mark.parametrize("launch", ["I", "P", "B", "mixed"])
def test_stale_lds(cf, launch):
    """512 x 16: dense blocks, then single-coefficient blocks; and with zero_intra, blocks that are
    transformed in one tile and written as zeros in the next."""
    s = _directed(I.stale_batch(cf, launch))
    with s.context() as ctx:
        s.upload(ctx, "records")
        check(ctx, s, list(range(s.npics)))
        check(ctx, s, list(range(s.npics)), zero_intra=True)


def skipped_picture_batch(w, h, cf):
    """An I picture of DC-only MBs, then a P picture of only skipped MBs (forward, zero vector,
    nothing coded)."""
    mbw, mbh, nb = w // 16, h // 16, RM.NB[cf]
    M = mbw * mbh
    pics = np.zeros(2, R.PIC_DTYPE)
    for p in range(2):
        pics[p]["dst_slot"], pics[p]["fwd_slot"], pics[p]["bwd_slot"] = p, (-1, 0)[p], -1
        pics[p]["picture_coding_type"], pics[p]["mb_first"] = p + 1, p * M
        pics[p]["mb_width"], pics[p]["mb_height"], pics[p]["W"] = mbw, mbh, 16
    mbs = np.zeros(2 * M, R.MB_DTYPE)
    coefs = []
    for k in range(2 * M):
        m = mbs[k]
        m["x"], m["y"], m["qscale"], m["coef_off"] = (k % M) % mbw, (k % M) // mbw, 4, len(coefs)
        if k < M:
            m["flags"], m["cbp"] = MB_INTRA, (1 << nb) - 1
            coefs += [int(_lib.coef_pack(900 + 8 * b + k, 0, b, _lib.COEF_DC, m["x"])) for b in range(nb)]
        else:
            m["flags"] = MB_FWD
        m["ncoef"] = len(coefs) - int(m["coef_off"])
    return pics, mbs, np.array(coefs, np.uint32)


def test_sparse_and_dense_words():
    """A P picture of only skipped MBs is all zeros; rows and a picture without words; the most
    words a record can carry (ncoef = 768, every scan position of every block, a level of -32768)."""
    s = Src(None, 80, 32, 2, skipped_picture_batch(80, 32, 2))
    assert all(not p[1].any() for p in s.want()) and s.want()[0][0].any()
    with s.context() as ctx:
        s.upload(ctx, "records")
        check_all(ctx, s, [1, 0, 1])
    t = generated(64, 48, 1)
    pics, mbs, coefs, k = drop_words(t)
    d = Src(None, 64, 48, 1, (pics, mbs, coefs))
    assert not d.want()[0][k].any() and d.want()[0][k - 1].any() and d.want()[0][k + 1].any()
    with d.context() as ctx:
        d.upload(ctx, "records")
        check_all(ctx, d, list(range(d.npics)))
    w, h, pics, mbs, coefs = dense_batch()
    assert int(mbs["ncoef"].max()) == 768
    d = Src(None, w, h, 3, (pics, mbs, coefs))
    with d.context() as ctx:
        d.upload(ctx, "records")
        check_all(ctx, d, [0, 0])


@pytest.mark.parametrize("path", ["records", "es"])
def test_skip_runs_stream(path):
    """tests/golden/syntax/skip_runs.m2v: P and B pictures of skipped runs, nearly every MB
    without words."""
    with open(os.path.join(GOLDEN, "syntax", "manifest.json")) as f:
        e = next(m for m in json.load(f) if m["name"] == "skip_runs")
    with open(os.path.join(GOLDEN, "syntax", e["file"]), "rb") as f:
        s = Src(f.read(), e["width"], e["height"], e["chroma_format"])
    with s.context() as ctx:
        s.upload(ctx, path)
        check_all(ctx, s, [int(d) for d in s.parsed.display])


def test_order_and_sub_ranges():
    """Several pictures per launch in an order that repeats and reverses; upload_es of pictures
    [k, k + m) with k > 0."""
    es = R.generate_es(width=64, height=48, chroma_format=1, n_gops=2, gop_n=4, gop_m=2, seed=9, frame_pred_frame_dct=0)
    s = Src(es, 64, 48, 1)
    k = int(np.nonzero(s.pics["picture_coding_type"] == 1)[0][1])
    m = s.npics - k
    assert k > 0 and m > 1
    with s.context() as ctx:
        s.upload(ctx, "records")
        order = list(range(s.npics))[::-1] + [2, 2, 0, s.npics - 1, 2]
        check_all(ctx, s, order)
        with R.Scan(es, 64, 48, 1) as scan:
            ctx.upload_es(scan, first=k, npics=m)
        sub = Src(None, 64, 48, 1, (s.pics[k:], s.mbs, s.coefs))
        sub._want = {key: tuple(p[k:] for p in s.want(*key)) for key in (("int16", False), ("int8", False))}
        check(ctx, sub, list(range(m))[::-1] + [0])
        check(ctx, sub, [m - 1, 0], "int8")
        rc, _, clean, fresh = raw_export(ctx, [m])
        assert rc == E_INVALID and clean and all(fresh)


def test_zero_intra():
    s = golden("ipb420_qcif")
    M = (s.w // 16) * (s.h // 16)
    k = next(i for i, p in enumerate(s.pics) if int(p["picture_coding_type"]) == 2 and
             (s.mbs["flags"][int(p["mb_first"]):int(p["mb_first"]) + M] & MB_INTRA).any())
    a, b = s.want()[0][k], s.want("int16", True)[0][k]
    assert a.any() and b.any() and not np.array_equal(a, b)  # intra MBs in a P picture that also has inter residual
    with s.context() as ctx:
        s.upload(ctx, "es")
        check(ctx, s, [k, 0, k], zero_intra=True)
        check(ctx, s, [k, 0], "int8", zero_intra=True)
        got = ctx.export_residual([0, k], zero_intra=True)
        for g, w in zip(got, s.want("int16", True)):
            assert np.array_equal(g.cpu().numpy(), w[[0, k]])
        assert not got[0][0].any()  # the I picture: all intra


@pytest.mark.parametrize("size", [(48, 48, 1), (64, 32, 2)], ids=lambda s: "%dx%d_cf%d" % s)
def test_against_the_reconstruct_kernels(size):
    """The check that ties the export to the decode: every P and B picture predicts from one slot
    outside the batch's destinations, written as constant 0 and then as constant 255; the export of
    the same resident records equals dec0 + dec255 - 255 on non-intra MBs, and clip(R, 0, 255) equals
    the decode on intra MBs."""
    w, h, cf = size
    s = generated(w, h, cf, gop_n=6, gop_m=3)
    ref = s.npics
    pics = RM.constant_reference(s.pics, ref)
    assert {int(t) for t in pics["picture_coding_type"]} == {1, 2, 3}
    shapes = RM.plane_shapes(w, h, cf)
    dec = {}
    with s.context(slots=ref + 1) as ctx:
        for c in (0, 255):
            SS.write_slot(ctx, ref, [np.full(sh, c, np.uint8) for sh in shapes], 5 + c)
            ctx.invalidate(ref)
            ctx.upload(pics, s.mbs, s.coefs)
            ctx.decode()
            ctx.synchronize()
            dec[c] = [ctx.download(int(p["dst_slot"])) for p in pics]
        got = [g.cpu().numpy() for g in ctx.export_residual()]
    for g, wnt in zip(got, s.want()):
        assert np.array_equal(g, wnt)
    for i, p in enumerate(pics):
        RM.check_identity([g[i] for g in got], dec[0][i], dec[255][i], RM.intra_mask(p, s.mbs, w, h, cf))


def test_bank_reuse_and_decode_order():
    """An export enqueued without a wait survives two more uploads (the second reuses its bank and
    must wait for it); an export between upload and decode equals one after it, and the decode's
    frames stay those of the oracle."""
    a = golden("ipb420_field")
    b = generated(176, 144, 1, seed=21)
    c = generated(176, 144, 1, seed=22)
    assert (a.w, a.h, a.cf) == (176, 144, 1)
    with R.DeviceContext(176, 144, 1, slots=max(a.npics, b.npics, c.npics)) as ctx:
        a.upload(ctx, "es")
        outs = ctx.export_residual(sync=False)
        b.upload(ctx, "records")
        c.upload(ctx, "es")
        ctx.synchronize()
        for g, w in zip(outs, a.want()):
            assert np.array_equal(g.cpu().numpy(), w)
        check(ctx, c, list(range(c.npics)))
        a.upload(ctx, "records")
        before = [t.cpu().numpy() for t in ctx.export_residual()]
        ctx.decode()
        after = [t.cpu().numpy() for t in ctx.export_residual()]
        for x, y, w in zip(before, after, a.want()):
            assert np.array_equal(x, y) and np.array_equal(x, w)
        frames = [ctx.download(int(p["dst_slot"])) for p in a.pics]
    exp = oracle_frames(a.parsed)
    for f, e in zip(frames, exp):
        assert all(np.array_equal(x, y) for x, y in zip(f, e))


def test_rejections():
    s = golden("ipb422_qcif")
    with s.context() as ctx:
        rc, _, clean, fresh = raw_export(ctx, [0])
        assert rc == E_STATE and clean and all(fresh)  # a fresh context: no batch
        with pytest.raises(_lib.Mp2vgError) as e:
            ctx.export_residual()
        assert e.value.status == E_STATE
        s.upload(ctx, "records")
        for dtype in ("int16", "int8"):
            right = [int(np.prod(sh)) * np.dtype(dtype).itemsize for sh in _lib.residual_shapes(s.w, s.h, s.cf, 1)]
            assert tuple(right) == R.residual_bytes(s.w, s.h, s.cf, 1, dtype)
            cases = [dict(order=[s.npics]), dict(order=[-1]), dict(order=[0, s.npics]), dict(order=[0], n=0),
                     dict(order=[0], n=-1), dict(order=[0], n=65536), dict(order=[0], outputs=(False, False, False)),
                     dict(order=[0], outputs=(True, True, False)), dict(order=[0], outputs=(False, False, True)),
                     dict(order=[0], outputs=(True, False, True)), dict(order=[0], offset=2), dict(order=[0], offset=8),
                     dict(order=[0], code=2), dict(order=[0], code=-1), dict(order=[0], flags=2), dict(order=[0], flags=3),
                     dict(order=[0], flags=-2)]
            for t in range(3):
                for wrong in (right[t] - 1, right[t] + 2, 0, 2 * right[t]):
                    sizes = list(right)
                    sizes[t] = wrong
                    cases.append(dict(order=[0], sizes=sizes))
            for kw in cases:
                rc, _, clean, fresh = raw_export(ctx, dtype=dtype, **kw)
                assert rc == E_INVALID and clean and all(fresh), kw
                assert _lib.lib().mp2vg_last_error()
        # a wrong size of planes that are not wanted is not looked at; the batch is still resident
        right = list(R.residual_bytes(s.w, s.h, s.cf, 1))
        rc, got, clean, _ = raw_export(ctx, [1], outputs=(True, False, False), sizes=[right[0], 0, 7])
        assert rc == 0 and clean and np.array_equal(got[0], s.want()[0][[1]])
        assert _lib.lib().mp2vg_residual_batch(None, None, 1, 0, 0, None, None, None, None) == E_INVALID
        with pytest.raises(ValueError):
            ctx.export_residual(dtype="int32")


def test_decode_residual():
    e = MANIFEST["ipb420_field"]
    s = golden("ipb420_field")
    es = read_stream(e)
    display = np.asarray(s.parsed.display)
    host = R.residual_host(s.pics, s.mbs, s.coefs, s.w, s.h, s.cf)
    dev = R.decode_residual(es, s.w, s.h, s.cf)
    by_host = R.decode_residual(es, s.w, s.h, s.cf, parse="host")
    for name, w in zip(("y", "cb", "cr"), host):
        assert dev[name].is_cuda and np.array_equal(dev[name].cpu().numpy(), w[display]), name
        assert np.array_equal(by_host[name].cpu().numpy(), w[display]), name
    assert np.array_equal(dev["types"], s.pics["picture_coding_type"][display])
    subset = [5, 0, 3]
    part = R.decode_residual(es, s.w, s.h, s.cf, pictures=subset, dtype="int8", chroma=False, zero_intra=True)
    w8 = R.residual_host(s.pics, s.mbs, s.coefs, s.w, s.h, s.cf, dtype="int8", zero_intra=True)
    assert part["cb"] is None and part["cr"] is None
    assert np.array_equal(part["y"].cpu().numpy(), w8[0][display[subset]])
    assert np.array_equal(part["types"], s.pics["picture_coding_type"][display[subset]])
    with pytest.raises(ValueError):
        R.decode_residual(es, s.w, s.h, s.cf, parse="gpu")
