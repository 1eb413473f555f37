"""CPU: the residual export's definition (include/mp2vg.h "residual export") through its host twin,
mp2vg_residual_records: the numpy model over the oracle (residual_model.py) against the twin on
every golden stream, the independent writer's records and the directed IDCT / dequant batches; the
whole-picture identity through the oracle's reconstruct (two decodes over a constant reference);
literal cases from hand-built records; the arguments; and the twin under AddressSanitizer +
UndefinedBehaviorSanitizer in a stand-alone program (tests/fuzz/residual_check.cpp)."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import _oracle
import directed_dequant as Q
import directed_idct as I
import directed_syntax as DS
import residual_model as RM
from conftest import GOLDEN, load_manifest, read_stream
from helpers import fill_mb
from tiny_mp2v_dec_amd import _lib
from tiny_mp2v_dec_amd import records as R
from tiny_mp2v_dec_amd._lib import COEF_DC, COEF_FIRST1S, MB_BWD, MB_DCT_FIELD, MB_FWD, MB_INTRA

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "tiny_mp2v_dec_amd", "csrc")
MANIFEST = load_manifest()
SYNTAX = os.path.join(GOLDEN, "syntax")
with open(os.path.join(SYNTAX, "manifest.json")) as _f:
    SYNTAX_POSITIVE = [e for e in json.load(_f) if e["md5"] is not None]
NB = RM.NB


def both(pics, mbs, coefs, w, h, cf, order=None, zero_intra=False):
    """(y, cb, cr) int16 of the model after checking that the twin gives the same at both dtypes."""
    out = None
    for dtype in ("int16", "int8"):
        want = RM.model(pics, mbs, coefs, w, h, cf, order, dtype, zero_intra)
        got = R.residual_host(pics, mbs, coefs, w, h, cf, order, dtype, zero_intra)
        for name, a, b in zip(("y", "cb", "cr"), got, want):
            assert a.dtype == b.dtype and a.shape == b.shape, name
            assert np.array_equal(a, b), (name, dtype)
        out = out or want
    return out


# ---- model against the host twin --------------------------------------------------------------
@pytest.fixture(scope="module")
def parsed_streams():
    cache = {}

    def get(name):
        if name not in cache:
            e = next(m for m in MANIFEST if m["name"] == name)
            cache[name] = R.Parsed(read_stream(e), e["width"], e["height"], e["chroma_format"])
        return cache[name]
    return get


@pytest.mark.parametrize("entry", MANIFEST, ids=[e["name"] for e in MANIFEST])
def test_golden_streams_model_equals_twin(parsed_streams, entry):
    p = parsed_streams(entry["name"])
    both(p.pics, p.mbs, p.coefs, p.width, p.height, p.chroma_format)


@pytest.fixture(scope="module")
def syntax_streams():
    return {S.name: S for S in DS.build_all()}


@pytest.mark.parametrize("entry", SYNTAX_POSITIVE, ids=[e["name"] for e in SYNTAX_POSITIVE])
def test_directed_syntax_records_model_equals_twin(syntax_streams, entry):
    """Records from the independent writer's own expectation, pictures from the library's scan."""
    S = syntax_streams[entry["name"]]
    mbs, coefs = DS.records(S)
    with R.Scan(S.es, S.width, S.height, S.cf) as scan:
        pics = scan.pics.copy()
    both(pics, mbs.astype(R.MB_DTYPE), coefs, S.width, S.height, S.cf)


@pytest.mark.parametrize("cf", [1, 2, 3])
def test_directed_idct_batch_model_equals_twin(cf):
    """The saturating witness vectors in every coded-block slot, DCT type and MB kind."""
    for launch in ("I", "mixed"):
        bt = I.idct_batch(80, 32, cf, launch)
        y, _, _ = both(bt.pics, bt.mbs, bt.coefs, bt.width, bt.height, cf)
        assert y.max() == 255 and y.min() == -255


def test_directed_dequant_batch_model_equals_twin():
    bt = Q.dequant_batch(128, 16, 2, "P")
    both(bt.pics, bt.mbs, bt.coefs, bt.width, bt.height, 2)
    both(bt.pics, bt.mbs, bt.coefs, bt.width, bt.height, 2, zero_intra=True)


def random_batch(w, h, cf, seed):
    """I, P, B pictures of helpers.fill_mb records with saturating levels and large matrices."""
    rng = np.random.default_rng(seed)
    mbw, mbh = w // 16, h // 16
    n = mbw * mbh
    pics = np.zeros(3, R.PIC_DTYPE)
    mbs = np.zeros(3 * n, R.MB_DTYPE)
    coefs = []
    for p in range(3):
        pics[p]["dst_slot"], pics[p]["fwd_slot"], pics[p]["bwd_slot"] = p, (-1, 0, 0)[p], (-1, -1, 1)[p]
        pics[p]["picture_coding_type"], pics[p]["mb_first"] = p + 1, p * n
        pics[p]["mb_width"], pics[p]["mb_height"] = mbw, mbh
        pics[p]["alternate_scan"] = rng.integers(0, 2)
        pics[p]["W"] = rng.integers(1, 256, size=(4, 64))
        for k in range(n):
            m = mbs[p * n + k]
            m["x"], m["y"] = k % mbw, k // mbw
            fill_mb(rng, m, coefs, w, h, cf, p == 0, [MB_FWD, MB_BWD, MB_FWD | MB_BWD] if p == 2 else [MB_FWD], True, True)
    return pics, mbs, np.array(coefs, np.uint32)


@pytest.mark.parametrize("cf", [1, 2, 3])
def test_random_records_reach_the_rails(cf):
    """Model = twin on random records, and the coverage the int8 clamp needs: some element at each
    int16 rail, and int16 values beyond both int8 rails (so int8 cannot pass by never clamping)."""
    pics, mbs, coefs = random_batch(80, 48, cf, 40 + cf)
    R.validate_batch(80, 48, cf, 3, pics, mbs, coefs)
    for zi in (False, True):
        planes = both(pics, mbs, coefs, 80, 48, cf, zero_intra=zi)
        for p in planes:
            assert (p == 255).any() and (p == -255).any() and (p > 127).any() and (p < -128).any()
    y8 = R.residual_host(pics, mbs, coefs, 80, 48, cf, dtype="int8")[0]
    assert (y8 == 127).any() and (y8 == -128).any()


# ---- the whole-picture identity: a second yardstick, independent of the block walk ------------
def decoded_over_constant(pics, mbs, coefs, w, h, cf, c):
    """Decode-order frames of the oracle when every P / B picture predicts from a slot of constant c."""
    ref = len(pics)
    g = _oracle.geometry(w, h, cf)
    pool = np.zeros(int(g.slot_bytes) * (ref + 1) + 64, np.uint8)
    pool[ref * int(g.slot_bytes):(ref + 1) * int(g.slot_bytes)] = c
    _oracle.reconstruct(w, h, cf, RM.constant_reference(pics, ref), mbs, coefs, ref + 1, pool=pool)
    out = []
    for p in pics:
        base = int(p["dst_slot"]) * int(g.slot_bytes)
        out.append([pool[base + g.plane_off[k]:base + g.plane_off[k] + g.stride[k] * g.ph[k]]
                    .reshape(g.ph[k], g.stride[k])[:, :g.pw[k]].copy() for k in range(3)])
    return out


def identity(pics, mbs, coefs, w, h, cf):
    got = R.residual_host(pics, mbs, coefs, w, h, cf)
    d0, d255 = (decoded_over_constant(pics, mbs, coefs, w, h, cf, c) for c in (0, 255))
    for i, p in enumerate(pics):
        RM.check_identity([g[i] for g in got], d0[i], d255[i], RM.intra_mask(p, mbs, w, h, cf))


@pytest.mark.parametrize("name", ["ipb420_field", "ipb422_field", "ipb444_field", "stress_saturation", "w80_422_field",
                                  "ipb420_qcif_openb"])
def test_whole_picture_identity_golden(parsed_streams, name):
    p = parsed_streams(name)
    assert len({int(s) for s in p.pics["dst_slot"]}) == p.npics and (p.pics["picture_coding_type"] > 1).any()
    identity(p.pics, p.mbs, p.coefs, p.width, p.height, p.chroma_format)


@pytest.mark.parametrize("cf", [1, 2, 3])
def test_whole_picture_identity_random(cf):
    pics, mbs, coefs = random_batch(80, 48, cf, 50 + cf)
    identity(pics, mbs, coefs, 80, 48, cf)


# ---- literal cases ----------------------------------------------------------------------------
def build(w, h, cf, pictures):
    """pictures: [(type, {MB index: (flags, cbp, qscale, [(level, pos, block, word flags)])})]; MBs
    not named are intra DC-128 MBs in an I picture and skipped MBs (forward, zero vector) otherwise."""
    mbw, mbh, nb = w // 16, h // 16, NB[cf]
    M = mbw * mbh
    pics = np.zeros(len(pictures), R.PIC_DTYPE)
    mbs = np.zeros(len(pictures) * M, R.MB_DTYPE)
    coefs = []
    for p, (t, named) in enumerate(pictures):
        pics[p]["dst_slot"], pics[p]["fwd_slot"], pics[p]["bwd_slot"] = p, (0 if t > 1 else -1), (1 if t == 3 else -1)
        pics[p]["picture_coding_type"], pics[p]["mb_first"] = t, p * M
        pics[p]["mb_width"], pics[p]["mb_height"], pics[p]["W"] = mbw, mbh, 16
        for k in range(M):
            m = mbs[p * M + k]
            m["x"], m["y"], m["coef_off"] = k % mbw, k // mbw, len(coefs)
            flags, cbp, qs, words = named.get(k, (MB_INTRA, (1 << nb) - 1, 8, [(1024, 0, b, COEF_DC) for b in range(nb)])
                                              if t == 1 else (MB_FWD, 0, 8, []))
            m["flags"], m["cbp"], m["qscale"] = flags, cbp, qs
            coefs += [int(_lib.coef_pack(lv, pos, b, fl, m["x"])) for lv, pos, b, fl in words]
            m["ncoef"] = len(coefs) - int(m["coef_off"])
    coefs = np.array(coefs, np.uint32)
    R.validate_batch(w, h, cf, len(pictures), pics, mbs, coefs)
    return pics, mbs, coefs


def hand(F):
    """clip(r, -255, 255) of hand-written QFS through the oracle's IDCT alone."""
    F = np.asarray(F, np.int16)
    return (_oracle.idct(F, np.zeros(64, np.uint8)).astype(np.int16) +
            _oracle.idct(F, np.full(64, 255, np.uint8)).astype(np.int16) - 255).reshape(8, 8)


def qfs(**at):
    F = np.zeros(64, np.int16)
    for k, v in at.items():
        F[int(k[1:])] = v
    return F


def test_literal_rails_wordless_and_ones():
    """32 x 32, 4:2:0, an I and a P picture.  P MB 0: block 0 one word of level 2047 at position 0
    (W 16, qscale 1: ((2 * 2047 + 1) * 16) >> 5 = 2047), block 1 the same with -2047, blocks 2 and 3
    coded without words.  P MB 1: skipped.  P MB 2: intra.  P MB 3: block 5 alone, a '1s' word of
    level -1 (qscale 8: (3 * 16 * 8) >> 5 = 12)."""
    nb = 6
    intra_words = [(8 * (100 + b), 0, b, COEF_DC) for b in range(nb)]
    named = {0: (MB_FWD, 0b001111, 1, [(2047, 0, 0, 0), (-2047, 0, 1, 0)]),
             2: (MB_INTRA, 63, 8, intra_words),
             3: (MB_FWD, 1 << 5, 8, [(-1, 0, 5, COEF_FIRST1S)])}
    pics, mbs, coefs = build(32, 32, 1, [(1, {}), (2, named)])
    y, cb, cr = both(pics, mbs, coefs, 32, 32, 1)
    y8 = R.residual_host(pics, mbs, coefs, 32, 32, 1, dtype="int8")[0]
    assert (y[1, 0:8, 0:8] == 255).all() and (y8[1, 0:8, 0:8] == 127).all()          # 2047, odd: no toggle
    assert (y[1, 0:8, 8:16] == -255).all() and (y8[1, 0:8, 8:16] == -128).all()      # r = -256 before the clamp
    assert np.array_equal(y[1, 8:16, 0:8], hand(qfs(p63=1)))                          # wordless: position 63 toggled to 1
    assert np.array_equal(y[1, 8:16, 8:16], hand(qfs(p63=1))) and not cb[1, 0:8, 0:8].any()  # blocks 4, 5: not coded
    assert not y[1, 0:16, 16:32].any() and not cb[1, 0:8, 8:16].any()                 # the skipped MB
    assert np.array_equal(cr[1, 8:16, 8:16], hand(qfs(p0=-12, p63=1)))                # '1s': -12, even sum: toggle
    assert not cb[1, 8:16, 8:16].any() and not y[1, 16:32, 16:32].any()               # the other blocks of MB 3
    # the intra MB of the P picture: clip8(R) is its decoded sample (DC 800 + 8 b, mismatch toggle)
    for b, (pl, ys, xs) in enumerate([(y, slice(16, 24), slice(0, 8)), (y, slice(16, 24), slice(8, 16)),
                                      (y, slice(24, 32), slice(0, 8)), (y, slice(24, 32), slice(8, 16)),
                                      (cb, slice(8, 16), slice(0, 8)), (cr, slice(8, 16), slice(0, 8))]):
        want = hand(qfs(p0=8 * (100 + b), p63=1))
        assert np.array_equal(pl[1, ys, xs], want) and want.min() >= 99 + b
    # zero_intra: the intra MB (and the whole I picture) is zeros, everything else is unchanged
    zy, zcb, zcr = both(pics, mbs, coefs, 32, 32, 1, zero_intra=True)
    assert not zy[0].any() and not zy[1, 16:32, 0:16].any() and not zcb[1, 8:16, 0:8].any()
    keep = np.ones((32, 32), bool)
    keep[16:32, 0:16] = False
    assert np.array_equal(zy[1][keep], y[1][keep]) and np.array_equal(zcr[1, 8:16, 8:16], cr[1, 8:16, 8:16])


@pytest.mark.parametrize("cf", [1, 2])
def test_literal_field_dct(cf):
    """One intra MB with MP2VG_MB_DCT_FIELD, each block a different DC: luma lines interleave; 4:2:0
    chroma does not, 4:2:2 chroma does."""
    nb = NB[cf]
    words = [(8 * (40 + 10 * b), 0, b, COEF_DC) for b in range(nb)]
    pics, mbs, coefs = build(16, 16, cf, [(1, {0: (MB_INTRA | MB_DCT_FIELD, (1 << nb) - 1, 8, words)})])
    y, cb, cr = both(pics, mbs, coefs, 16, 16, cf)
    flat = [hand(qfs(p0=8 * (40 + 10 * b), p63=1)) for b in range(nb)]
    assert len({int(f[0, 0]) for f in flat}) == nb
    assert np.array_equal(y[0, 0::2, 0:8], flat[0]) and np.array_equal(y[0, 0::2, 8:16], flat[1])
    assert np.array_equal(y[0, 1::2, 0:8], flat[2]) and np.array_equal(y[0, 1::2, 8:16], flat[3])
    if cf == 1:
        assert np.array_equal(cb[0], flat[4]) and np.array_equal(cr[0], flat[5])
    else:
        assert np.array_equal(cb[0, 0::2], flat[4]) and np.array_equal(cb[0, 1::2], flat[6])
        assert np.array_equal(cr[0, 0::2], flat[5]) and np.array_equal(cr[0, 1::2], flat[7])
    # the same MB with frame DCT: blocks above each other
    mbs["flags"][0] = MB_INTRA
    y, cb, cr = both(pics, mbs, coefs, 16, 16, cf)
    assert np.array_equal(y[0, 0:8, 0:8], flat[0]) and np.array_equal(y[0, 8:16, 8:16], flat[3])
    if cf == 2:
        assert np.array_equal(cb[0, 0:8], flat[4]) and np.array_equal(cr[0, 8:16], flat[7])


# ---- arguments --------------------------------------------------------------------------------
def test_residual_bytes():
    assert R.residual_bytes(176, 144, 1, 5) == (5 * 176 * 144 * 2, 5 * 88 * 72 * 2, 5 * 88 * 72 * 2)
    assert R.residual_bytes(176, 144, 2, 5, "int8") == (5 * 176 * 144, 5 * 88 * 144, 5 * 88 * 144)
    assert R.residual_bytes(176, 144, 3, 1) == (176 * 144 * 2,) * 3
    assert R.residual_bytes(16, 16, 1, 1, "int8") == (256, 64, 64)
    assert R.residual_bytes(4096, 2176, 3, 65535)[2] == 65535 * 4096 * 2176 * 2
    for n in (0, -1, 65536):
        with pytest.raises(_lib.Mp2vgError) as e:
            R.residual_bytes(176, 144, 1, n)
        assert e.value.status == -1
    with pytest.raises(_lib.Mp2vgError):
        R.residual_bytes(100, 64, 1, 1)
    with pytest.raises(ValueError):
        R.residual_bytes(176, 144, 1, 1, "uint8")
    cfg = _lib.make_config(176, 144, 1)
    b = (ctypes.c_uint64 * 3)()
    assert _lib.lib().mp2vg_residual_bytes(ctypes.byref(cfg), 1, 0, None) == -1
    assert _lib.lib().mp2vg_residual_bytes(None, 1, 0, b) == -1
    assert _lib.lib().mp2vg_residual_bytes(ctypes.byref(cfg), 1, 2, b) == -1


def test_order_repeats_and_reverse(parsed_streams):
    p = parsed_streams("ipb420_field")
    full = R.residual_host(p.pics, p.mbs, p.coefs, p.width, p.height, 1)
    for order in (list(range(p.npics))[::-1], [2, 2, 0, p.npics - 1, 2], [1], list(p.display)):
        got = both(p.pics, p.mbs, p.coefs, p.width, p.height, 1, order)
        for a, b in zip(got, full):
            assert np.array_equal(a, b[np.array(order)])


def raw_records(p, order, n=None, dtype=0, flags=0, outs=(True, True, True), pics=None, cfg=None):
    """(status, the three sentinel-filled destinations) of the C entry point itself."""
    L = _lib.lib()
    cfg = cfg or _lib.make_config(p.width, p.height, p.chroma_format)
    order = np.ascontiguousarray(order, np.int32)
    n = len(order) if n is None else n
    nbytes = R.residual_bytes(p.width, p.height, p.chroma_format, max(1, min(len(order), 8)), "int8" if dtype == 1 else "int16")
    dst = [np.full(b, 0xA5, np.uint8) for b in nbytes]
    vp = ctypes.c_void_p
    pics = p.pics if pics is None else pics
    rc = L.mp2vg_residual_records(ctypes.byref(cfg), pics.ctypes.data_as(vp), len(pics), p.mbs.ctypes.data_as(vp),
                                  len(p.mbs), p.coefs.ctypes.data_as(vp), len(p.coefs),
                                  order.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), n, dtype, flags,
                                  *[d.ctypes.data_as(vp) if want else None for d, want in zip(dst, outs)])
    return rc, dst


def test_rejected_arguments_leave_destinations_untouched(parsed_streams):
    p = parsed_streams("ipb420_qcif")
    clean = lambda dst: all((d == 0xA5).all() for d in dst)  # noqa: E731
    rc, dst = raw_records(p, [0, 1])
    assert rc == 0 and not any((d == 0xA5).all() for d in dst)
    rc, dst = raw_records(p, [0], outs=(True, False, False))  # luma alone
    assert rc == 0 and clean(dst[1:]) and not (dst[0] == 0xA5).all()
    rc, dst = raw_records(p, [0], dtype=1, outs=(False, True, True))  # chroma alone
    assert rc == 0 and clean(dst[:1]) and not (dst[1] == 0xA5).all() and not (dst[2] == 0xA5).all()
    for order in ([0, p.npics], [-1], [0, 1 << 30]):
        rc, dst = raw_records(p, order)
        assert rc == -1 and clean(dst) and b"order[" in _lib.lib().mp2vg_last_error()
    for n in (0, -3, 65536):
        rc, dst = raw_records(p, [0], n=n)
        assert rc == -1 and clean(dst)
    for kw in (dict(outs=(False, False, False)), dict(outs=(True, True, False)), dict(outs=(True, False, True)),
               dict(outs=(False, False, True)), dict(dtype=2), dict(dtype=-1), dict(flags=2), dict(flags=-1)):
        rc, dst = raw_records(p, [0], **kw)
        assert rc == -1 and clean(dst) and _lib.lib().mp2vg_last_error(), kw
    # a record batch the upload refuses is refused alike, with its reason
    bad = p.pics.copy()
    bad[1]["mb_first"] = len(p.mbs)
    rc, dst = raw_records(p, [0], pics=bad)
    assert rc == -1 and clean(dst) and b"picture MB range outside the batch" in _lib.lib().mp2vg_last_error()
    mbs = p.mbs.copy()
    k = int(np.nonzero(mbs["ncoef"] > 0)[0][-1])
    mbs[k]["coef_off"] = len(p.coefs)
    for fn in (R.residual_host, R.motion_host):  # exactly as mp2vg_motion_records does
        with pytest.raises(_lib.Mp2vgError) as e:
            fn(p.pics, mbs, p.coefs, p.width, p.height, 1)
        assert e.value.status == -1 and "coefficient range outside the batch" in str(e.value)
    rc, dst = raw_records(p, [0], cfg=_lib.make_config(192, 144, 1))
    assert rc == -1 and clean(dst)


# ---- the twin under the sanitizers ------------------------------------------------------------
@pytest.fixture(scope="module")
def residual_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("san_residual") / "residual_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I", CSRC,
           "-I", os.path.join(REPO, "include"), os.path.join(REPO, "tests", "fuzz", "residual_check.cpp"),
           os.path.join(CSRC, "residual.cpp"), os.path.join(CSRC, "parse.cpp"), os.path.join(CSRC, "tables.cpp"),
           os.path.join(CSRC, "runtime.cpp"), "-o", exe, "-pthread", "-L/opt/rocm/lib", "-lamdhip64",
           "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        pytest.fail(f"sanitizer build failed:\n{r.stderr[-2000:]}")
    return exe


def test_twin_under_sanitizers(residual_check):
    args = []
    for name in ("ipb420_field", "w80_422_field", "w48_444"):
        e = next(m for m in MANIFEST if m["name"] == name)
        args += [os.path.join(GOLDEN, "streams", e["file"]), str(e["width"]), str(e["height"]), str(e["chroma_format"])]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([residual_check] + args, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["streams"] == 3 and res["exports"] > 0 and res["rejected"] > 0 and res["mutants"] > 0
