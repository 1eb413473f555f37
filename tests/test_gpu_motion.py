"""GPU: the motion export (motion.hip through mp2vg_motion_batch / DeviceContext.export_motion)
against the numpy model of its definition (tests/motion_model.py), array_equal everywhere.  Every
destination is prefilled with FILL and sits between guard bytes that are checked afterwards."""
import ctypes
import os

import numpy as np
import pytest

import motion_model as MM
from conftest import GOLDEN, load_manifest, read_stream
from test_gpu_export import FILL, GUARD
from tiny_mp2v_dec_amd import _lib
from tiny_mp2v_dec_amd import records as R
from tiny_mp2v_dec_amd._lib import COEF_DC, MB_INTRA

pytestmark = pytest.mark.gpu

MANIFEST = {e["name"]: e for e in load_manifest()}
NB = {1: 6, 2: 8, 3: 12}
DTYPES = (np.int16, np.uint16, np.int32)
E_INVALID, E_STATE = -1, -5


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    """torch brings its own HIP runtime: it is loaded and initialised before this module's first
    context, the order decode_rgb and decode_motion use (an export's tensors exist first)."""
    import torch
    torch.cuda.init()


class Src:
    """A stream with its host records and the model of every picture (computed once)."""

    def __init__(self, es, w, h, cf):
        self.es, self.w, self.h, self.cf = es, w, h, cf
        self.parsed = R.Parsed(es, w, h, cf)
        self.npics = self.parsed.npics
        self.want = MM.model(self.parsed.pics, self.parsed.mbs, self.parsed.coefs, cf)

    def context(self):
        return R.DeviceContext(self.w, self.h, self.cf, slots=self.npics)

    def upload(self, ctx, path):
        if path == "es":
            with R.Scan(self.es, self.w, self.h, self.cf) as scan:
                ctx.upload_es(scan)
        else:
            ctx.upload(self.parsed.pics, self.parsed.mbs, self.parsed.coefs)


_cache = {}


def golden(name):
    if name not in _cache:
        e = MANIFEST[name]
        _cache[name] = Src(read_stream(e), e["width"], e["height"], e["chroma_format"])
    return _cache[name]


def generated(w, h, cf, **kw):
    key = (w, h, cf, tuple(sorted(kw.items())))
    if key not in _cache:
        args = dict(width=w, height=h, chroma_format=cf, n_gops=1, gop_n=4, gop_m=2, seed=3, frame_pred_frame_dct=0)
        args.update(kw)
        _cache[key] = Src(R.generate_es(**args), w, h, cf)
    return _cache[key]


def shapes(ctx, n):
    mbw, mbh, nb = ctx.width // 16, ctx.height // 16, NB[ctx.chroma_format]
    return [(n, 8, mbh, mbw), (n, 4, mbh, mbw), (n, 2, nb, mbh, mbw)]


def raw_export(ctx, order, outputs=(True, True, True), offset=0, n=None, sizes=None, sync=True):
    """mp2vg_motion_batch itself into guarded buffers at data_ptr + GUARD + offset.  Returns
    (status, [array or None per output], guards and unwanted buffers untouched?, [destination
    bytes untouched? per output])."""
    import torch
    order = np.ascontiguousarray(order, np.int32)
    n = len(order) if n is None else n
    shp = shapes(ctx, max(len(order), 1))
    nbytes = [int(np.prod(s)) * np.dtype(d).itemsize for s, d in zip(shp, DTYPES)]
    bufs = [torch.full((GUARD + offset + b + GUARD,), FILL, dtype=torch.uint8, device="cuda") for b in nbytes]
    torch.cuda.synchronize()
    ptrs = [ctypes.c_void_p(t.data_ptr() + GUARD + offset) if want else None for t, want in zip(bufs, outputs)]
    given = (ctypes.c_uint64 * 3)(*(nbytes if sizes is None else sizes))
    rc = _lib.lib().mp2vg_motion_batch(ctx.h, order.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), n, ptrs[0], ptrs[1],
                                       ptrs[2], given)
    if sync:
        ctx.synchronize()
    host = [t.cpu().numpy() for t in bufs]
    at = GUARD + offset
    clean = all((b[:at] == FILL).all() and (b[at + nb:] == FILL).all() and (want or (b == FILL).all())
                for b, nb, want in zip(host, nbytes, outputs))
    got = [b[at:at + nb].copy().view(d).reshape(s) if want else None
           for b, nb, d, s, want in zip(host, nbytes, DTYPES, shp, outputs)]
    fresh = [(b[at:at + nb] == FILL).all() for b, nb in zip(host, nbytes)]
    return rc, got, clean, fresh


def check(ctx, want, order, outputs=(True, True, True), offset=0):
    rc, got, clean, _ = raw_export(ctx, order, outputs, offset)
    assert rc == 0, _lib.lib().mp2vg_last_error()
    assert clean
    idx = np.asarray(order, np.int64)
    for name, g, w in zip(("mv", "info", "act"), got, want):
        if g is not None:
            assert np.array_equal(g, w[idx]), name


GOLDEN_NAMES = ["ipb420_field", "w80_422_field", "w48_444", "ipb422_qcif", "intra444_dense", "stress_mv_fcode4",
                "ipb420_qcif_openb"]


@pytest.mark.parametrize("path", ["records", "es"])
@pytest.mark.parametrize("name", GOLDEN_NAMES)
def test_golden_streams_by_both_upload_paths(name, path):
    s = golden(name)
    display = [int(d) for d in s.parsed.display]
    with s.context() as ctx:
        s.upload(ctx, path)
        check(ctx, s.want, display)
        check(ctx, s.want, display[::-1] + [display[0], display[0]])
        check(ctx, s.want, [display[-1]])
        # the Python entry point: every picture in batch order
        mv, info, act = ctx.export_motion()
        for g, w in zip((mv, info, act), s.want):
            assert np.array_equal(g.cpu().numpy(), w)


@pytest.mark.parametrize("cf", [1, 2, 3])
@pytest.mark.parametrize("size", [16, 48])
@pytest.mark.parametrize("path", ["records", "es"])
def test_smallest_geometries(size, cf, path):
    """M = 1: every plane after a tensor's first starts on an odd 2-byte boundary; M = 9."""
    s = generated(size, size, cf)
    order = list(range(s.npics)) + [1]
    with s.context() as ctx:
        s.upload(ctx, path)
        for t in range(3):
            check(ctx, s.want, order, tuple(k == t for k in range(3)))
        check(ctx, s.want, order, offset=4)
        check(ctx, s.want, [2], offset=4)


def widest():
    for w in (4096, 4080):
        try:
            return generated(w, 16, 1, mix=1, intra_coefs_min=20, intra_coefs_max=40, gop_n=2, gop_m=1)
        except _lib.Mp2vgError:
            continue
    raise AssertionError("no wide stream")


@pytest.mark.parametrize("which", ["w1040", "widest"])
@pytest.mark.parametrize("path", ["records", "es"])
def test_wide_rows(which, path):
    """65 MBs: one row crosses a wave; the widest one-row picture: the row fills the activity
    kernel's tile."""
    s = generated(1040, 16, 1, mix=1, intra_coefs_min=20, intra_coefs_max=40) if which == "w1040" else widest()
    assert s.w >= 4080 or which == "w1040"
    assert int(s.parsed.mbs["ncoef"].min()) >= 6 and s.parsed.mbs["ncoef"].mean() > 60
    with s.context() as ctx:
        s.upload(ctx, path)
        check(ctx, s.want, list(range(s.npics))[::-1])


@pytest.mark.parametrize("path", ["records", "es"])
def test_more_than_one_workgroup_per_picture(path):
    """M > 1024 cells: the mv / info kernel runs a second workgroup per picture.  1072 x 272 has
    M = 67 x 17 = 1139, odd: the planes that start on a 2-byte boundary cross wave and workgroup
    boundaries, where a wave's last lane stores its own last value and the next wave's first
    lane its own first; 4 does not divide M, so the last run is partial.  The golden 720 x 480
    field stream (M = 1350) is the even case."""
    s = generated(1072, 272, 1, gop_n=3)
    assert (s.w // 16) * (s.h // 16) == 1139
    with s.context() as ctx:
        s.upload(ctx, path)
        check(ctx, s.want, list(range(s.npics))[::-1] + [1])
        check(ctx, s.want, [1, 0], offset=4)
    g = golden("sd480_420_field")
    with g.context() as ctx:
        g.upload(ctx, path)
        check(ctx, g.want, [int(d) for d in g.parsed.display][:4])


def dense_batch():
    """4:4:4, 32 x 32, one intra picture whose every block has a DC word and all 63 AC words:
    ncoef = 768, the most a record can carry."""
    w = h = 32
    pics = np.zeros(1, R.PIC_DTYPE)
    pics[0]["dst_slot"], pics[0]["fwd_slot"], pics[0]["bwd_slot"], pics[0]["picture_coding_type"] = 0, -1, -1, 1
    pics[0]["mb_width"] = pics[0]["mb_height"] = 2
    pics[0]["W"] = 16
    rng = np.random.default_rng(11)
    mbs = np.zeros(4, R.MB_DTYPE)
    coefs = []
    for k in range(4):
        m = mbs[k]
        m["x"], m["y"], m["flags"], m["cbp"], m["qscale"], m["coef_off"] = k % 2, k // 2, MB_INTRA, 0xFFF, 2, len(coefs)
        for b in range(12):
            levels = rng.integers(-2048, 2048, 64)
            levels[1] = -32768 if k == 3 else levels[1]  # |level| needs 32 bits
            for pos in range(64):
                coefs.append((int(levels[pos]) & 0xFFFF) | (pos << 16) | (b << 22) | (COEF_DC if pos == 0 else 0) |
                             ((k % 2) << 26))
        m["ncoef"] = len(coefs) - int(m["coef_off"])
    return w, h, pics, mbs, np.array(coefs, np.uint32)


def test_dense_words():
    w, h, pics, mbs, coefs = dense_batch()
    assert int(mbs["ncoef"].max()) == 768
    want = MM.model(pics, mbs, coefs, 3)
    assert int(want[2][0, 1].max()) >= 32768 and int(want[2][0, 0].min()) == 64
    with R.DeviceContext(w, h, 3, slots=1) as ctx:
        ctx.upload(pics, mbs, coefs)
        check(ctx, want, [0, 0])
    # the writer's densest intra stream, by both paths
    s = generated(64, 48, 3, mix=1, intra_coefs_min=63, intra_coefs_max=63, gop_n=1, gop_m=1)
    assert int(s.parsed.mbs["ncoef"].max()) > 128
    for path in ("records", "es"):
        with s.context() as ctx:
            s.upload(ctx, path)
            check(ctx, s.want, [0])


@pytest.mark.parametrize("path", ["records", "es"])
def test_rows_and_pictures_without_words(path):
    """tests/golden/syntax/skip_runs.m2v: P and B pictures of skipped runs (the writer codes at
    least one coefficient per coded block, so the empty rows come from the directed stream)."""
    import json
    with open(os.path.join(GOLDEN, "syntax", "manifest.json")) as f:
        e = next(m for m in json.load(f) if m["name"] == "skip_runs")
    with open(os.path.join(GOLDEN, "syntax", e["file"]), "rb") as f:
        s = Src(f.read(), e["width"], e["height"], e["chroma_format"])
    p = s.parsed
    inter = np.repeat(p.pics["picture_coding_type"] > 1, (s.w // 16) * (s.h // 16))
    assert s.h == 16 and (p.mbs["ncoef"][inter] == 0).mean() > 0.9  # one row, nearly every MB without words
    with s.context() as ctx:
        s.upload(ctx, path)
        check(ctx, s.want, [int(d) for d in p.display])
    if path == "es":
        return
    # rows and a whole picture with no words at all: the records of a stream with the words of its
    # first inter picture dropped (one row in skip_runs, three in the generated stream)
    for t in (s, generated(64, 48, 1)):
        pics, mbs, coefs, k = drop_words(t)
        want = MM.model(pics, mbs, coefs, t.cf)
        assert not want[2][k].any() and want[2][k - 1].any() and want[2][k + 1].any()
        with t.context() as ctx:
            ctx.upload(pics, mbs, coefs)
            check(ctx, want, list(range(t.npics)))


def drop_words(s):
    """(pics, mbs, coefs, k): the stream's records with every word of its first inter picture k
    removed (its intra MBs, which must code every block, become predicted MBs with a zero vector)."""
    p = s.parsed
    k = int(np.nonzero(p.pics["picture_coding_type"] > 1)[0][0])
    M = (s.w // 16) * (s.h // 16)
    mbs = p.mbs.copy()
    own = slice(int(p.pics[k]["mb_first"]), int(p.pics[k]["mb_first"]) + M)
    first, last = int(mbs[own]["coef_off"][0]), int(mbs[own]["coef_off"][-1]) + int(mbs[own]["ncoef"][-1])
    assert last > first
    mbs["cbp"][own], mbs["ncoef"][own], mbs["coef_off"][own] = 0, 0, first
    intra = np.nonzero(mbs["flags"][own] & MB_INTRA)[0] + own.start
    mbs["flags"][intra], mbs["mv"][intra] = (2 if int(p.pics[k]["fwd_slot"]) >= 0 else 4), 0
    later = mbs["coef_off"] >= last
    later[own] = False
    mbs["coef_off"][later] -= last - first
    return p.pics, mbs, np.concatenate([p.coefs[:first], p.coefs[last:]]), k


def test_sub_ranges():
    """upload_es of pictures [k, k + m) with k > 0, and a host batch whose pictures' records are
    not in batch order (mb_first != 0 for the first picture)."""
    es = R.generate_es(width=64, height=48, chroma_format=1, n_gops=2, gop_n=4, gop_m=2, seed=9, frame_pred_frame_dct=0)
    s = Src(es, 64, 48, 1)
    k = int(np.nonzero(s.parsed.pics["picture_coding_type"] == 1)[0][1])
    m = s.npics - k
    assert k > 0 and m > 1
    sub = tuple(w[k:] for w in s.want)
    with s.context() as ctx:
        with R.Scan(es, 64, 48, 1) as scan:
            ctx.upload_es(scan, first=k, npics=m)
        check(ctx, sub, list(range(m))[::-1])
        mv, _, _ = ctx.export_motion(info=False, act=False)
        assert np.array_equal(mv.cpu().numpy(), sub[0])
        rc, _, clean, fresh = raw_export(ctx, [m])
        assert rc == E_INVALID and clean and all(fresh)
    M = 12
    p = s.parsed
    pics = p.pics.copy()
    mbs = np.zeros_like(p.mbs)
    for i in range(s.npics):
        to = (s.npics - 1 - i) * M
        mbs[to:to + M] = p.mbs[i * M:(i + 1) * M]
        pics[i]["mb_first"] = to
    assert pics[0]["mb_first"] != 0
    want = MM.model(pics, mbs, p.coefs, 1)
    for a, b in zip(want, s.want):
        assert np.array_equal(a, b)
    with s.context() as ctx:
        ctx.upload(pics, mbs, p.coefs)
        check(ctx, want, list(range(s.npics)))


def test_bank_reuse_and_decode_order():
    """An export enqueued without a wait survives two more uploads (the second reuses its bank and
    must wait for it), and an export before decode() equals one after it."""
    a = golden("ipb420_field")
    b = generated(176, 144, 1, seed=21)
    c = generated(176, 144, 1, seed=22)
    assert (a.w, a.h, a.cf) == (176, 144, 1)
    with R.DeviceContext(176, 144, 1, slots=max(a.npics, b.npics, c.npics)) as ctx:
        a.upload(ctx, "es")
        outs = ctx.export_motion(sync=False)
        b.upload(ctx, "records")
        c.upload(ctx, "es")
        ctx.synchronize()
        for g, w in zip(outs, a.want):
            assert np.array_equal(g.cpu().numpy(), w)
        check(ctx, c.want, list(range(c.npics)))
        a.upload(ctx, "records")
        before = [t.cpu().numpy() for t in ctx.export_motion()]
        ctx.decode()
        after = [t.cpu().numpy() for t in ctx.export_motion()]
        for x, y, w in zip(before, after, a.want):
            assert np.array_equal(x, y) and np.array_equal(x, w)
        frames = [ctx.download(int(p["dst_slot"])) for p in a.parsed.pics]
    from helpers import yuv_md5
    assert [yuv_md5(frames[d]) for d in a.parsed.display] == MANIFEST["ipb420_field"]["md5"]


def test_rejections():
    s = golden("ipb422_qcif")
    with s.context() as ctx:
        rc, _, clean, fresh = raw_export(ctx, [0])
        assert rc == E_STATE and clean and all(fresh)  # a fresh context: no batch
        with pytest.raises(_lib.Mp2vgError) as e:
            ctx.export_motion()
        assert e.value.status == E_STATE
        s.upload(ctx, "records")
        right = [int(np.prod(sh)) * np.dtype(d).itemsize for sh, d in zip(shapes(ctx, 1), DTYPES)]
        assert tuple(right) == R.motion_bytes(s.w, s.h, s.cf, 1)
        cases = [dict(order=[s.npics]), dict(order=[-1]), dict(order=[0, s.npics]), dict(order=[0], n=0),
                 dict(order=[0], n=-1), dict(order=[0], n=65536), dict(order=[0], outputs=(False, False, False)),
                 dict(order=[0], offset=2)]
        for t in range(3):
            for wrong in (right[t] - 1, right[t] + 2, 0, 2 * right[t]):
                sizes = list(right)
                sizes[t] = wrong
                cases.append(dict(order=[0], sizes=sizes))
        for kw in cases:
            rc, _, clean, fresh = raw_export(ctx, **kw)
            assert rc == E_INVALID and clean and all(fresh), kw
            assert _lib.lib().mp2vg_last_error()
        # a wrong size of a tensor that is not wanted is not looked at; the batch is still resident
        rc, got, clean, _ = raw_export(ctx, [1], outputs=(True, False, True), sizes=[right[0], 0, right[2]])
        assert rc == 0 and clean and np.array_equal(got[0], s.want[0][[1]]) and np.array_equal(got[2], s.want[2][[1]])
        assert _lib.lib().mp2vg_motion_batch(None, None, 1, None, None, None, None) == E_INVALID


def test_decode_motion():
    e = MANIFEST["ipb420_field"]
    s = golden("ipb420_field")
    es = read_stream(e)
    dev = R.decode_motion(es, e["width"], e["height"], e["chroma_format"])
    host = R.decode_motion(es, e["width"], e["height"], e["chroma_format"], parse="host")
    display = s.parsed.display
    for name, w in zip(("mv", "info", "act"), s.want):
        assert dev[name].is_cuda and np.array_equal(dev[name].cpu().numpy(), w[display]), name
        assert np.array_equal(host[name].cpu().numpy(), w[display]), name
    assert dev["dist"].dtype == np.int32 and dev["dist"].shape == (s.npics, 2)
    assert np.array_equal(dev["dist"], host["dist"])
    assert np.array_equal(dev["dist"], R.reference_distances(s.parsed.pics, display))
    with pytest.raises(ValueError):
        R.decode_motion(es, e["width"], e["height"], e["chroma_format"], parse="gpu")
