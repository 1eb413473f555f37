"""Shared by the CPU tests, the GPU tests and tests/golden/make_parse_mutants.py: the base streams
of the byte-mutant sweep and the walk over their mutants, the host emitter / CPU twin wrappers,
and the directed streams of the device-parse tests (a chosen slice made to fail, start-code
stuffing, mutants at the end of a sub-range).  One place, so that the three cannot drift apart."""
import json
import os
import re

import numpy as np

from tiny_mp2v_dec_amd import _lib
from tiny_mp2v_dec_amd.records import Parsed, Scan, generate_es

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "parse_mutants.json")

# generator parameters of the four base streams; stream si is walked with the seed WALK_SEED + si
STREAMS = [
    dict(width=176, height=48, chroma_format=1, n_gops=1, gop_n=6, gop_m=3, seed=7, frame_pred_frame_dct=0, f_code=2),
    dict(width=64, height=48, chroma_format=3, n_gops=1, gop_n=6, gop_m=3, seed=8, frame_pred_frame_dct=0, f_code=3,
         escape_permille=200),
    dict(width=80, height=48, chroma_format=2, n_gops=1, gop_n=4, gop_m=1, seed=9, leading_b=0,
         frame_pred_frame_dct=0, f_code=1),
    dict(width=176, height=48, chroma_format=1, n_gops=1, gop_n=3, gop_m=1, seed=10, leading_b=0, mix=1),
]
WALK_SEED = 1000
MUTANTS_PER_STREAM = 900  # the CPU sweep (test_device_parse_cpu.py)
# The committed fixture walks the same sequences further: among the first 900 mutants per stream
# only one is rejected with "bad coded_block_pattern" and two with "slice does not cover the
# whole macroblock row"; the first 1500 hold three of each.
FIXTURE_MUTANTS_PER_STREAM = 1500
# the stream whose intra_vlc_format bits are cleared (clear_intra_vlc_format)
VLC0_STREAM = dict(width=176, height=144, chroma_format=1, n_gops=1, gop_n=2, gop_m=1, leading_b=0, mix=1)

SLICE_REASONS = [
    "macroblock beyond the end of the row", "bad macroblock_address_increment", "slice does not start at column 0",
    "skipped macroblock in an I picture", "skip run beyond the end of the row",
    "skipped MB reads outside the reference", "bad macroblock_type", "dual-prime prediction",
    "reserved frame_motion_type", "4:4:4 field DCT", "bad motion_code", "prediction from a missing reference",
    "motion vector reads outside the reference", "bad coded_block_pattern",
    "bad DCT coefficient code", "coefficient run past position 63",
    "slice does not cover the whole macroblock row",
]
# Not in the list: "bad dct_dc_size" cannot happen (B.12 and B.13 are complete prefix codes: every
# 9- / 10-bit window decodes), "intra_vlc_format=0" and the truncated slice have their own streams,
# and "slice overruns the buffer" needs a macroblock that ends more than 8 bytes past its slice
# without meeting any other error first, which no mutant here does.
VLC0_REASON = "intra_vlc_format=0"


def geom(kw):
    return kw["width"], kw["height"], kw["chroma_format"]


def host(es, w, h, cf):
    """(status, message, Parsed or None) of the host emitter; one thread, so that the slice blamed
    is the first failing one in stream order, as in the scan and the twin."""
    try:
        return 0, "", Parsed(es, w, h, cf, threads=1)
    except _lib.Mp2vgError as e:
        return e.status, str(e), None


def twin(es, w, h, cf, first=0, npics=None):
    """(status, message, (mbs, coefs) or None, rejected by the scan itself) of the CPU twin of the
    device parse over pictures [first, first + npics)"""
    try:
        sc = Scan(es, w, h, cf)
    except _lib.Mp2vgError as e:
        return e.status, str(e), None, True
    try:
        return 0, "", sc.parse_host(first, npics), False
    except _lib.Mp2vgError as e:
        return e.status, str(e), None, False


def detail(msg):
    """the library's own message: the text inside the outer parentheses of Mp2vgError"""
    return msg.split("(", 1)[1][:-1] if "(" in msg else msg


def same_records(p, rec):
    return rec[0].tobytes() == p.mbs.tobytes() and rec[1].tobytes() == p.coefs.tobytes()


def range_of_whole(p, first, n):
    """(mbs, coefs) of pictures [first, first + n) of a Parsed, rebased to the range (record 0,
    word 0): what a sub-range parse must give"""
    per = len(p.mbs) // p.npics
    mbs = p.mbs[first * per:(first + n) * per].copy()
    c0 = int(mbs["coef_off"][0])
    c1 = int(p.mbs["coef_off"][(first + n) * per]) if (first + n) * per < len(p.mbs) else len(p.coefs)
    mbs["coef_off"] -= c0
    return mbs, p.coefs[c0:c1].copy()


def start_codes(es, code):
    pat = b"\x00\x00\x01" + bytes([code])
    out, i = [], es.find(pat)
    while i >= 0:
        out.append(i)
        i = es.find(pat, i + 1)
    return out


def slice_starts(es):
    """byte offsets of the slice start codes (00 00 01 01..AF), found without the library"""
    return [m.start() for m in re.finditer(rb"\x00\x00\x01[\x01-\xaf]", es)]


def mutate(es, pos, val):
    b = bytearray(es)
    b[pos] = val
    return bytes(b)


def base_streams():
    """[(bytes, width, height, chroma format)] of STREAMS"""
    return [(generate_es(**kw),) + geom(kw) for kw in STREAMS]


def walk(si, es, count=MUTANTS_PER_STREAM):
    """the first `count` (byte position, byte value) of stream si's mutant sequence"""
    rng = np.random.default_rng(WALK_SEED + si)
    first_slice = es.find(b"\x00\x00\x01\x01")
    for _ in range(count):
        pos = int(rng.integers(first_slice + 4, len(es)))
        yield pos, int(rng.integers(0, 256))


def set_bit(es, byte_off, bit, value):
    b = bytearray(es)
    pos = byte_off * 8 + bit
    mask = 0x80 >> (pos % 8)
    b[pos // 8] = (b[pos // 8] | mask) if value else (b[pos // 8] & ~mask & 0xFF)
    return bytes(b)


def clear_intra_vlc_format(es):
    """every picture_coding_extension's intra_vlc_format bit cleared"""
    for o in [o + 4 for o in start_codes(es, 0xB5) if (es[o + 4] >> 4) == 8]:
        es = set_bit(es, o, 28, 0)
    return es


def vlc0_stream():
    return (clear_intra_vlc_format(generate_es(**VLC0_STREAM)),) + geom(VLC0_STREAM)


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


# ---- a chosen slice made to fail ------------------------------------------------------------------
def one_slice_pictures(n, seed):
    """I-only stream of n one-row 16x16 pictures: slice j is picture j"""
    return generate_es(width=16, height=16, chroma_format=1, n_gops=n, gop_n=1, gop_m=1, mix=1, leading_b=0, seed=seed)


def blamed_picture(msg):
    m = re.search(r"picture (\d+) slice @(\d+)", msg)
    return (int(m.group(1)), int(m.group(2))) if m else None


def failing_substitution(es, w, h, cf, k, other_than=None):
    """The first single-byte substitution (positions ascending, then values ascending) in the
    payload of slice k of a one-slice-per-picture stream that the scan lets through and the twin
    rejects with a slice-level reason, optionally a reason other than `other_than`.
    Returns (position, value, reason text)."""
    sc = Scan(es, w, h, cf)
    n = sc.npics
    starts = slice_starts(es)
    assert len(starts) == n
    lo = starts[k] + 4
    nxt = es.find(b"\x00\x00\x01", lo)
    hi = nxt if nxt >= 0 else len(es)
    for pos in range(lo, hi):
        for val in range(256):
            if val == es[pos]:
                continue
            b = mutate(es, pos, val)
            try:
                s2 = Scan(b, w, h, cf)
            except _lib.Mp2vgError:
                continue
            if s2.npics != n or s2.nslices != n:
                continue
            try:
                s2.parse_host(k, 1)
            except _lib.Mp2vgError as e:
                why = detail(str(e)).split(": ", 1)[1]
                if any(r in why for r in SLICE_REASONS) and why != other_than:
                    return pos, val, why
    raise AssertionError(f"no single-byte substitution makes slice {k} fail")


def stream_with_failing_slices(es, w, h, cf, ks):
    """es with slices `ks` made to fail, each by failing_substitution; the later ones for reasons
    other than the earliest one's, so that a status or reason read from the wrong slice shows.
    Returns (bytes, {k: reason})."""
    ks = sorted(ks)
    out, why = es, {}
    for k in ks:
        pos, val, r = failing_substitution(es, w, h, cf, k, other_than=why.get(ks[0]))
        out = mutate(out, pos, val)
        why[k] = r
    return out, why


# ---- next_start_code() stuffing: zero bytes in front of a start code --------------------------------
STUFF_STREAM = dict(width=176, height=144, chroma_format=1, n_gops=1, gop_n=6, gop_m=3, seed=21)


def stuffed(es, k):
    """k zero bytes inserted immediately before the second slice's start code"""
    o = slice_starts(es)[1]
    return es[:o] + bytes(k) + es[o:]


def slice_residues(es):
    """count of slices per (byte_off - first slice's byte_off) & 3: the residue of the address the
    device reader starts the slice at (the uploaded span starts at the first slice)"""
    s = slice_starts(es)
    return [sum(1 for o in s if (o - s[0]) & 3 == r) for r in range(4)]


# ---- the reader's tail: streams whose last slice ends at the buffer's last byte --------------------
TAIL_SEEDS = [4, 5, 3, 2]  # the first seeds whose span length (tail_span) is 0, 1, 2, 3 mod 4


def tail_stream(seed):
    """64x32 I/P stream without its sequence_end_code"""
    es = generate_es(width=64, height=32, chroma_format=1, n_gops=1, gop_n=4, gop_m=1, leading_b=0, seed=seed)
    assert es.endswith(b"\x00\x00\x01\xb7")
    return es[:-4]


def tail_span(es):
    """bytes from the first slice's start code to the end: what upload_es sends for the whole stream"""
    return len(es) - slice_starts(es)[0]


# ---- mutants confined to the last slice of a sub-range ------------------------------------------------
SUBRANGE_CASES = [  # golden stream, first picture, pictures, walk seed
    ("ipb420_qcif", 5, 7, 4100),
    ("ipb422_field", 2, 6, 4101),
]
SUBRANGE_MUTANTS = 300


def subrange_walk(es, w, h, cf, first, n, seed):
    """(position, value) of SUBRANGE_MUTANTS single-byte mutants inside the last slice of pictures
    [first, first + n): from after its start code to the next start code"""
    starts = slice_starts(es)
    rows = h // 16
    j = (first + n) * rows - 1  # one slice per row in the golden streams
    lo = starts[j] + 4
    hi = es.find(b"\x00\x00\x01", lo)
    rng = np.random.default_rng(seed)
    for _ in range(SUBRANGE_MUTANTS):
        yield int(rng.integers(lo, hi)), int(rng.integers(0, 256))


def subrange_mutants(es, w, h, cf, first, n, seed):
    """[(position, value, host status, host message, twin status, twin message, rejected by the
    scan, records equal the range of the whole's or None)]: the host emitter on the whole mutated
    stream against the twin on pictures [first, first + n) of it"""
    out = []
    for pos, val in subrange_walk(es, w, h, cf, first, n, seed):
        b = mutate(es, pos, val)
        hs, hm, p = host(b, w, h, cf)
        ts, tm, rec, by_scan = twin(b, w, h, cf, first, n)
        same = None
        if hs == 0 and ts == 0:
            want = range_of_whole(p, first, n)
            same = want[0].tobytes() == rec[0].tobytes() and want[1].tobytes() == rec[1].tobytes()
        out.append((pos, val, hs, hm, ts, tm, by_scan, same))
    return out
