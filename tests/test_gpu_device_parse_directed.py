"""GPU: what only the device build of the parse runs (parse.hip, parse_dev.cpp, and the
__HIP_DEVICE_COMPILE__ branches of slice_parse.h), against the host emitter and the CPU twin:
every slice-level rejection reason, which slice is blamed when several fail, the scan kernel's
multi-slice lanes (more than 1024 slices), the reader at every start residue and tail length,
buffer growth across calls, and mutants at the end of a sub-range.  Every comparison is exact.

Every stream sent to the device has gone through the twin first (which asserts sp_iter_bound and
returns a status), and once a call here returns MP2VG_E_HIP the rest of the file is skipped."""
import numpy as np
import pytest

import parse_mutants as PM
from conftest import load_manifest, read_stream
from helpers import oracle_frames
from tiny_mp2v_dec_amd import _lib
from tiny_mp2v_dec_amd import records as R

pytestmark = pytest.mark.gpu

BY_NAME = {e["name"]: e for e in load_manifest()}
FIX = PM.load_fixture()
E_HIP, E_STATE = -3, -5
_HIP = {"failed": False}


@pytest.fixture(scope="module", autouse=True)
def _torch_runtime_first():
    """torch brings its own HIP runtime: it has to open the device before the library's does, or
    torch finds no GPU when this file runs on its own (as in test_gpu_device_parse.py)."""
    import torch
    torch.zeros(1, device="cuda")


@pytest.fixture(scope="module", autouse=True)
def _watch_for_hip_errors():
    """every library status that records.py checks in this file passes through here"""
    real = R.check

    def check(status, what):
        if status == E_HIP:
            _HIP["failed"] = True
        return real(status, what)

    mp = pytest.MonkeyPatch()
    mp.setattr(R, "check", check)
    yield
    mp.undo()


@pytest.fixture(autouse=True)
def _nothing_more_after_a_hip_error(_watch_for_hip_errors):
    if _HIP["failed"]:
        pytest.skip("an earlier call in this file returned MP2VG_E_HIP: nothing more is launched on the device")


class Contexts:
    """one DeviceContext per geometry, kept for the module: uploads of different sizes, accepted
    and rejected, follow each other on the same context, as they do in use"""

    def __init__(self):
        self.by_geom = {}

    def get(self, w, h, cf):
        key = (w, h, cf)
        if key not in self.by_geom:  # slots for the longest stream of the geometry used below
            self.by_geom[key] = R.DeviceContext(w, h, cf, slots=3073 if (w, h) == (16, 16) else 32)
        return self.by_geom[key]

    def close(self):
        for c in self.by_geom.values():
            c.close()


@pytest.fixture(scope="module")
def contexts():
    c = Contexts()
    yield c
    c.close()


def _assert_frames_equal(got, want):
    assert len(got) == len(want)
    for d, (a, b) in enumerate(zip(got, want)):
        for p in range(3):
            assert np.array_equal(a[p], b[p]), (d, p)


def _assert_records_equal(got, want):
    assert got[0].tobytes() == want[0].tobytes(), "macroblock records differ"
    assert got[1].tobytes() == want[1].tobytes(), "coefficient words differ"


def _rejection(ctx, scan, first=0, npics=None):
    """(status, message detail) of an upload_es that must fail, and the decode after it must say
    that no batch is resident"""
    with pytest.raises(_lib.Mp2vgError) as dev:
        ctx.upload_es(scan, first, npics)
    with pytest.raises(_lib.Mp2vgError) as st:
        ctx.decode()
    assert st.value.status == E_STATE
    return dev.value.status, PM.detail(str(dev.value))


def _upload_decode(ctx, es, w, h, cf):
    """(host-parsed records, device records, frames in decode order, launch count) of the whole
    stream through upload_es on ctx"""
    parsed, scan = R.Parsed(es, w, h, cf), R.Scan(es, w, h, cf)
    scan.parse_host()  # the twin first
    ctx.upload_es(scan)
    rec = ctx.download_records()
    ctx.decode()
    ctx.synchronize()
    frames = [ctx.download(int(p["dst_slot"])) for p in scan.pics]
    return parsed, rec, frames, len(ctx.launch_times_ms())


# ---- B: rejection parity ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bases():
    """per base stream: (bytes, w, h, cf, Parsed, oracle frames)"""
    out = []
    for es, w, h, cf in PM.base_streams():
        p = R.Parsed(es, w, h, cf)
        out.append((es, w, h, cf, p, oracle_frames(p)))
    return out


def _clean_stream_decodes(ctx, es, w, h, cf, want_frames):
    parsed, rec, frames, _ = _upload_decode(ctx, es, w, h, cf)
    _assert_records_equal(rec, (parsed.mbs, parsed.coefs))
    _assert_frames_equal(frames, want_frames)


@pytest.mark.parametrize("reason", PM.SLICE_REASONS)
def test_each_rejection_reason_has_the_twins_status_and_message(contexts, bases, reason):
    entries = FIX["rejected"][reason]
    assert len(entries) >= 3
    used = []
    for si, pos, val, status, det, by_scan in entries:
        es, w, h, cf, parsed, _ = bases[si]
        b = PM.mutate(es, pos, val)
        ts, tm, _, scanned = PM.twin(b, w, h, cf)
        assert not scanned and (ts, PM.detail(tm)) == (status, det)  # (the fixture is current)
        ctx = contexts.get(w, h, cf)
        assert _rejection(ctx, R.Scan(b, w, h, cf)) == (ts, PM.detail(tm))
        if si not in used:
            used.append(si)
    for si in used:  # the contexts stay usable: the unmutated streams decode to the oracle's frames
        es, w, h, cf, _, want = bases[si]
        _clean_stream_decodes(contexts.get(w, h, cf), es, w, h, cf, want)


def test_intra_vlc_format_zero_has_the_twins_status_and_message(contexts):
    es, w, h, cf = PM.vlc0_stream()
    ts, tm, _, scanned = PM.twin(es, w, h, cf)
    assert not scanned and ts == -2 and PM.VLC0_REASON in tm
    assert (ts, PM.detail(tm)) == (FIX["intra_vlc_format0"]["status"], FIX["intra_vlc_format0"]["detail"])
    ctx = contexts.get(w, h, cf)
    assert _rejection(ctx, R.Scan(es, w, h, cf)) == (ts, PM.detail(tm))
    good = R.generate_es(**PM.VLC0_STREAM)
    _clean_stream_decodes(ctx, good, w, h, cf, oracle_frames(R.Parsed(good, w, h, cf)))


def test_accepted_mutants_give_the_host_emitters_records(contexts, bases):
    """mutants the host emitter accepts with records unlike the base stream's: parser paths the
    generator never emits"""
    assert len(FIX["accepted"]) >= 24
    for si, pos, val, *_ in FIX["accepted"]:
        es, w, h, cf, base, _ = bases[si]
        b = PM.mutate(es, pos, val)
        hs, hm, p = PM.host(b, w, h, cf)
        ts, tm, rec, _ = PM.twin(b, w, h, cf)
        assert hs == 0 and ts == 0 and PM.same_records(p, rec) and not PM.same_records(base, rec)
        ctx = contexts.get(w, h, cf)
        ctx.upload_es(R.Scan(b, w, h, cf))
        _assert_records_equal(ctx.download_records(), (p.mbs, p.coefs))


# ---- B: which slice is blamed -----------------------------------------------------------------------------
# n = 2049: 1024 scan lanes of chunk 3, slices 3 t .. 3 t + 2 in lane t.  301 and 302 are the
# second and third slice of lane 100's chunk; 2047 and 4 sit in lanes 682 and 1.
BLAMED = [
    (130, (0,)), (130, (63,)), (130, (64,)), (130, (129,)), (130, (70, 5)), (130, (64, 63)),
    (2049, (1,)), (2049, (301,)), (2049, (302,)), (2049, (301, 302)), (2049, (2048,)), (2049, (2047, 4)),
]


@pytest.fixture(scope="module")
def one_slice_streams():
    return {n: PM.one_slice_pictures(n, n) for n in (130, 2049)}


@pytest.mark.parametrize("n,ks", BLAMED, ids=[f"{n}-{'+'.join(map(str, ks))}" for n, ks in BLAMED])
def test_the_first_failing_slice_in_stream_order_is_blamed(contexts, one_slice_streams, n, ks):
    es = one_slice_streams[n]
    bad, why = PM.stream_with_failing_slices(es, 16, 16, 1, ks)
    k = min(ks)
    if len(ks) == 2:
        assert why[min(ks)] != why[max(ks)]  # a reason read from the wrong slice shows
    hs, hm, _ = PM.host(bad, 16, 16, 1)
    ts, tm, _, scanned = PM.twin(bad, 16, 16, 1)
    assert hs != 0 and PM.blamed_picture(hm) == (k, PM.slice_starts(es)[k]) and why[k] in hm
    assert not scanned and (ts, PM.detail(tm)) == (hs, PM.detail(hm))
    scan = R.Scan(bad, 16, 16, 1)
    assert scan.nslices == n
    assert _rejection(contexts.get(16, 16, 1), scan) == (ts, PM.detail(tm))


# ---- C: more than 1024 slices ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1023, 1024, 1025, 2047, 2048, 2049, 3073])
def test_scan_kernel_lanes_with_several_slices(contexts, n):
    """one slice per picture; the scan kernel's 1024 lanes take ceil(n / 1024) slices each: 1 up
    to 1024, 2 from 1025 (lanes from 513 idle, lane 512 with one slice), 3 at 2049 (lane 683 on
    idle), 4 at 3073 (lane 768 with one slice).  The coefficient words are where the host emitter
    puts them only if base[] is right inside every chunk."""
    es = PM.one_slice_pictures(n, 5000 + n)
    parsed, rec, frames, _ = _upload_decode(contexts.get(16, 16, 1), es, 16, 16, 1)
    assert parsed.npics == n and R.Scan(es, 16, 16, 1).nslices == n
    assert len(np.unique(parsed.mbs["ncoef"])) > 4  # the slices' word counts differ: base[] is no constant stride
    _assert_records_equal(rec, (parsed.mbs, parsed.coefs))
    _assert_frames_equal(frames, oracle_frames(parsed))


def test_more_than_1024_pictures_of_two_slices_with_references():
    """32x32 I/P/B, 1032 pictures, 2064 slices: the scan kernel's per-picture loop over the
    reference usage bits reaches pictures 1024 and up (its second trip), where the bits are not
    zero; the plan made from them has the launches of the same batch uploaded from host records"""
    w, h, cf = 32, 32, 1
    es = R.generate_es(width=w, height=h, chroma_format=cf, n_gops=172, gop_n=6, gop_m=3, seed=31)
    with R.DeviceContext(w, h, cf, slots=1032) as ctx:
        parsed, rec, frames, nlaunch = _upload_decode(ctx, es, w, h, cf)
        assert parsed.npics >= 1030 and R.Scan(es, w, h, cf).nslices == 2 * parsed.npics
        late = parsed.pics["picture_coding_type"][1024:]
        assert np.any(late == 2) and np.any(late == 3)
        _assert_records_equal(rec, (parsed.mbs, parsed.coefs))
        _assert_frames_equal(frames, oracle_frames(parsed))
    with R.DeviceContext(w, h, cf, slots=1032) as ctx:
        ctx.upload(parsed.pics, parsed.mbs, parsed.coefs)
        ctx.decode()
        ctx.synchronize()
        assert nlaunch == len(ctx.launch_times_ms())


# ---- D: reader residues, the tail, growth --------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(4))
def test_reader_start_residues_with_stuffing_before_a_start_code(contexts, k):
    """k zero bytes in front of the second slice's start code: every later slice starts k bytes
    further, so over k = 0..3 each of them meets each residue of the reader's aligned loads"""
    w, h, cf = PM.geom(PM.STUFF_STREAM)
    es = R.generate_es(**PM.STUFF_STREAM)
    b = PM.stuffed(es, k)
    assert all(PM.slice_residues(b)), PM.slice_residues(b)
    s = PM.slice_starts(b)
    assert (s[1] - s[0]) & 3 == (PM.slice_starts(es)[1] - s[0] + k) & 3
    hs, _, p = PM.host(b, w, h, cf)
    assert hs == 0
    parsed, rec, frames, _ = _upload_decode(contexts.get(w, h, cf), b, w, h, cf)
    _assert_records_equal(rec, (p.mbs, p.coefs))
    _assert_frames_equal(frames, oracle_frames(parsed))


def test_reader_tail_of_a_sub_range_is_followed_by_the_next_pictures_headers(contexts):
    w, h, cf = 64, 32, 1
    es = PM.tail_stream(PM.TAIL_SEEDS[1])
    parsed, scan = R.Parsed(es, w, h, cf), R.Scan(es, w, h, cf)
    ctx = contexts.get(w, h, cf)
    for npics in range(1, parsed.npics):
        want = PM.range_of_whole(parsed, 0, npics)
        _assert_records_equal(scan.parse_host(0, npics), want)
        ctx.upload_es(scan, 0, npics)
        _assert_records_equal(ctx.download_records(), want)


def test_buffers_grow_and_are_reused_across_uploads():
    """one context: a 1-picture range, then the whole stream (every device buffer of the parse is
    freed and reallocated), then a 1-picture range again with first > 0 (the large buffers reused)"""
    e = BY_NAME["ipb420_qcif"]
    es, w, h, cf = read_stream(e), e["width"], e["height"], e["chroma_format"]
    parsed, scan = R.Parsed(es, w, h, cf), R.Scan(es, w, h, cf)
    want_frames = oracle_frames(parsed)
    with R.DeviceContext(w, h, cf, slots=parsed.npics) as ctx:
        for first, n in ((0, 1), (0, parsed.npics), (9, 1), (0, parsed.npics)):
            want = PM.range_of_whole(parsed, first, n)
            _assert_records_equal(scan.parse_host(first, n), want)
            ctx.upload_es(scan, first, n)
            _assert_records_equal(ctx.download_records(), want)
            if n == parsed.npics:
                ctx.decode()
                ctx.synchronize()
                _assert_frames_equal([ctx.download(int(p["dst_slot"])) for p in scan.pics], want_frames)


# ---- E: mutants at the end of a sub-range ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", PM.SUBRANGE_CASES, ids=[c[0] for c in PM.SUBRANGE_CASES])
def test_mutants_in_the_last_slice_of_a_sub_range(contexts, case):
    """past the range's end the device reads the zeros of its pad, as the twin does: the first 8
    rejected and the first 8 accepted mutants of the CPU test of the same name"""
    name, first, n, seed = case
    e = BY_NAME[name]
    es, w, h, cf = read_stream(e), e["width"], e["height"], e["chroma_format"]
    ms = [m for m in PM.subrange_mutants(es, w, h, cf, first, n, seed) if not m[6]]
    rejected, accepted = [m for m in ms if m[4] != 0][:8], [m for m in ms if m[4] == 0][:8]
    assert len(rejected) == 8 and len(accepted) == 8
    ctx = contexts.get(w, h, cf)
    for pos, val, _, _, ts, tm, _, _ in rejected:
        assert _rejection(ctx, R.Scan(PM.mutate(es, pos, val), w, h, cf), first, n) == (ts, PM.detail(tm))
    for pos, val, *_ in accepted:
        scan = R.Scan(PM.mutate(es, pos, val), w, h, cf)
        want = scan.parse_host(first, n)
        ctx.upload_es(scan, first, n)
        _assert_records_equal(ctx.download_records(), want)
