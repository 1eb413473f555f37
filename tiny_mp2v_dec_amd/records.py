"""Host side of the record path: stream generation, ES -> records parsing, and the device
context (frame pool + record batch + level-scheduled launches), mirroring the reference's
mp2v_decoder_c / frame_c vocabulary where it has one.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import MB_DTYPE, PIC_DTYPE, check, lib


def gen_params(**kw):
    p = _lib.GenParams()
    lib().mp2vg_gen_default_params(ctypes.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise KeyError(k)
        setattr(p, k, v)
    return p


def _copy_out(ptr, nbytes, dtype=np.uint8):
    """Copy nbytes at a library-owned pointer into a new array.  ctypes.string_at takes a C int size,
    which goes negative (or wraps) past 2 GiB; a numpy view over the pointer has no such limit."""
    if not nbytes:
        return np.zeros(0, dtype)
    raw = np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctypes.c_uint8)), shape=(nbytes,))
    return raw.view(dtype).copy()


def generate_es(**kw):
    """Write a synthetic elementary stream of the reference's decodable subset (bytes)."""
    p = gen_params(**kw)
    ptr, n = ctypes.c_void_p(), ctypes.c_uint64()
    check(lib().mp2vg_generate_es(ctypes.byref(p), ctypes.byref(ptr), ctypes.byref(n)), "generate_es")
    try:
        return _copy_out(ptr, n.value).tobytes()
    finally:
        lib().mp2vg_free(ptr)


def check_count(status, what):
    """An entry point that returns a count (>= 0) or an MP2VG_E_* status."""
    if status < 0:
        check(status, what)
    return status


def _damage_array(call, what):
    """The structured array (_lib.DAMAGE_DTYPE) of a damage query: a counts call, then the entries."""
    n = ctypes.c_int32()
    check(call(None, 0, ctypes.byref(n)), what)
    out = np.zeros(n.value, _lib.DAMAGE_DTYPE)
    if n.value:
        check(call(out.ctypes.data_as(ctypes.c_void_p), n.value, ctypes.byref(n)), what)
    return out


def damage_reason(reason):
    """The rejection text of a damage entry's reason code (mp2vg_damage_reason_string)."""
    return lib().mp2vg_damage_reason_string(int(reason)).decode()


def effective_pictures(pics, damage):
    """Picture records as a conceal=True batch decodes them: a damaged I picture that carries a
    conceal reference is a P picture from it (what the library makes resident), and every other I
    picture reads nothing (its fwd_slot, kept for slot lifetimes, is cleared here)."""
    pics = np.array(pics, PIC_DTYPE)
    hit = np.zeros(len(pics), bool)
    hit[np.asarray(damage["pic"], np.int64)] = True
    i_pic = pics["picture_coding_type"] == 1
    pics["picture_coding_type"][i_pic & hit & (pics["fwd_slot"] >= 0)] = 2
    pics["fwd_slot"][pics["picture_coding_type"] == 1] = -1
    return pics


class Parsed:
    """Records of a whole elementary stream (pictures in decode order; slot = decode index).
    conceal=True (MP2VG_PARSE_CONCEAL, include/mp2vg.h): damaged slices and missing rows are
    replaced row by row instead of failing the parse; .damage lists them (_lib.DAMAGE_DTYPE).
    standard=True (MP2VG_PARSE_STANDARD): quantiser matrices from the sequence header, the
    defaults and partial extensions as the standard rules them, and intra_vlc_format = 0.
    slices=True (MP2VG_PARSE_SLICES): any number of slices per macroblock row."""

    def __init__(self, es: bytes, width, height, chroma_format, threads=0, reordering=True, conceal=False,
                 standard=False, slices=False):
        self.width, self.height, self.chroma_format = width, height, chroma_format
        cfg = _lib.make_config(width, height, chroma_format, threads=threads, reordering=reordering,
                               flags=_lib.parse_flags(conceal, standard, slices))
        buf = np.frombuffer(es, dtype=np.uint8)
        h = ctypes.c_void_p()
        check(lib().mp2vg_parse_es(buf.ctypes.data_as(ctypes.c_void_p), len(es), ctypes.byref(cfg),
                                   ctypes.byref(h)), "parse_es")
        try:
            npics, nmbs, ncoefs = ctypes.c_int32(), ctypes.c_uint64(), ctypes.c_uint64()
            lib().mp2vg_parsed_counts(h, ctypes.byref(npics), ctypes.byref(nmbs), ctypes.byref(ncoefs))
            n, m, c = npics.value, nmbs.value, ncoefs.value
            self.pics = _copy_out(lib().mp2vg_parsed_pictures(h), n * 288, PIC_DTYPE)
            self.mbs = _copy_out(lib().mp2vg_parsed_mbs(h), m * 32, MB_DTYPE)
            self.coefs = _copy_out(lib().mp2vg_parsed_coefs(h), c * 4, np.uint32)
            order = (ctypes.c_int32 * max(n, 1))()
            lib().mp2vg_parsed_display_order(h, order, n)
            self.display = np.array(order[:n], dtype=np.int32)
            gop = (ctypes.c_int32 * max(n, 1))()
            lib().mp2vg_parsed_gop_index(h, gop, n)
            self.gop = np.array(gop[:n], dtype=np.int32)
            flags = (ctypes.c_uint32 * max(n, 1))()
            check_count(lib().mp2vg_parsed_picture_flags(h, flags, n), "parsed_picture_flags")
            self.flags = np.array(flags[:n], dtype=np.uint32)  # MP2VG_PIC_* per picture, decode order
            shard = (ctypes.c_int32 * max(n, 1))()
            self.nshards = check_count(lib().mp2vg_parsed_shards(h, shard, n), "parsed_shards")
            self.shard = np.array(shard[:n], dtype=np.int32)
            self.headers = _lib.StreamHeaders()
            check(lib().mp2vg_parsed_stream_headers(h, ctypes.byref(self.headers)), "parsed_stream_headers")
            self.damage = _damage_array(lambda o, m, c: lib().mp2vg_parsed_damage(h, o, m, c), "parsed_damage")
        finally:
            lib().mp2vg_parsed_free(h)

    @property
    def npics(self):
        return len(self.pics)


class Scan:
    """Host scan of an elementary stream (mp2vg_scan_es): what Parsed holds except the MB records
    and coefficient words, which DeviceContext.upload_es has the device parse from the bitstream
    (parse_host: the same parser on the CPU).  Keeps the stream's bytes alive.  conceal=True
    (MP2VG_PARSE_CONCEAL): the scan lets missing rows through and carries the flag to parse_host and
    DeviceContext.upload_es, which replace damaged rows; the damage of an upload is
    DeviceContext.last_damage().  standard=True (MP2VG_PARSE_STANDARD) as for Parsed; the scan
    carries it to parse_host and DeviceContext.upload_es too.  slices=True (MP2VG_PARSE_SLICES)
    likewise: a row's slices are consecutive entries of the slice table."""

    def __init__(self, es: bytes, width, height, chroma_format, reordering=True, conceal=False, standard=False,
                 slices=False):
        self.width, self.height, self.chroma_format = width, height, chroma_format
        self.conceal = bool(conceal)
        self.standard = bool(standard)
        self.slices = bool(slices)
        cfg = _lib.make_config(width, height, chroma_format, reordering=reordering,
                               flags=_lib.parse_flags(conceal, standard, slices))
        self._buf = np.frombuffer(es, dtype=np.uint8)
        self.h = ctypes.c_void_p()
        check(lib().mp2vg_scan_es(self._buf.ctypes.data_as(ctypes.c_void_p), len(es), ctypes.byref(cfg),
                                  ctypes.byref(self.h)), "scan_es")
        npics, nslices = ctypes.c_int32(), ctypes.c_uint64()
        lib().mp2vg_scan_counts(self.h, ctypes.byref(npics), ctypes.byref(nslices))
        n, self.nslices = npics.value, nslices.value
        self.pics = _copy_out(lib().mp2vg_scan_pictures(self.h), n * 288, PIC_DTYPE)
        order = (ctypes.c_int32 * max(n, 1))()
        lib().mp2vg_scan_display_order(self.h, order, n)
        self.display = np.array(order[:n], dtype=np.int32)
        gop = (ctypes.c_int32 * max(n, 1))()
        lib().mp2vg_scan_gop_index(self.h, gop, n)
        self.gop = np.array(gop[:n], dtype=np.int32)
        flags = (ctypes.c_uint32 * max(n, 1))()
        check_count(lib().mp2vg_scan_picture_flags(self.h, flags, n), "scan_picture_flags")
        self.flags = np.array(flags[:n], dtype=np.uint32)  # MP2VG_PIC_* per picture, decode order
        shard = (ctypes.c_int32 * max(n, 1))()
        self.nshards = check_count(lib().mp2vg_scan_shards(self.h, shard, n), "scan_shards")
        self.shard = np.array(shard[:n], dtype=np.int32)
        self.headers = _lib.StreamHeaders()
        check(lib().mp2vg_scan_stream_headers(self.h, ctypes.byref(self.headers)), "scan_stream_headers")

    @property
    def npics(self):
        return len(self.pics)

    def parse_host(self, first=0, npics=None):
        """(mbs, coefs) of pictures [first, first + npics) from the CPU twin of the device parse
        (mp2vg_scan_parse_host): a counts call, then arrays of exactly the counted sizes."""
        npics = self.npics - first if npics is None else npics
        if npics == 0:  # (a stream without pictures scans, as it parses: nothing to do)
            return np.zeros(0, MB_DTYPE), np.zeros(0, np.uint32)
        nm, nc = ctypes.c_uint64(), ctypes.c_uint64()
        check(lib().mp2vg_scan_parse_host(self.h, first, npics, None, 0, None, 0, ctypes.byref(nm), ctypes.byref(nc)),
              "scan_parse_host")
        mbs, coefs = np.zeros(nm.value, MB_DTYPE), np.zeros(nc.value, np.uint32)
        vp = ctypes.c_void_p
        check(lib().mp2vg_scan_parse_host(self.h, first, npics, mbs.ctypes.data_as(vp), len(mbs),
                                          coefs.ctypes.data_as(vp) if len(coefs) else None, len(coefs), None, None),
              "scan_parse_host")
        return mbs, coefs

    def close(self):
        if self.h:
            lib().mp2vg_scan_free(self.h)
            self.h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def plan_batch(width, height, chroma_format, nslots, pics, mbs, coefs, one_stream=False):
    """mp2vg_batch_validate: the upload's host-side record validation and launch planning, with no
    device.  Returns (launch index of each picture, kernel mode of each launch: 0 I, 1 P, 2 B,
    3 mixed, 4 I without tile stores); raises Mp2vgError for a batch the upload would refuse."""
    cfg = _lib.make_config(width, height, chroma_format, pool=nslots,
                           flags=_lib.MP2VG_CTX_ONE_STREAM if one_stream else 0)
    pics = np.ascontiguousarray(pics, PIC_DTYPE)
    mbs = np.ascontiguousarray(mbs, MB_DTYPE)
    coefs = np.ascontiguousarray(coefs, np.uint32)
    vp = ctypes.c_void_p
    n = ctypes.c_int32()
    of_pic = np.zeros(len(pics), np.int32)
    mode = np.zeros(4096, np.int32)
    i32p = ctypes.POINTER(ctypes.c_int32)
    check(lib().mp2vg_batch_validate(ctypes.byref(cfg), nslots, pics.ctypes.data_as(vp), len(pics),
                                     mbs.ctypes.data_as(vp), len(mbs),
                                     coefs.ctypes.data_as(vp) if len(coefs) else None, len(coefs),
                                     ctypes.byref(n), of_pic.ctypes.data_as(i32p), mode.ctypes.data_as(i32p),
                                     len(mode)), "batch_validate")
    return of_pic, mode[:min(n.value, len(mode))].copy()


def plan_dump(width, height, chroma_format, nslots, pics, mbs, coefs, one_stream=False):
    """mp2vg_batch_plan: the whole plan the upload would make resident, with no device.  A dict of
    int arrays: slices (n, 4: pic, mb_begin, mb_count, flag bits), launches (n, 6: begin, end,
    mode, level, set, mates), writes (npics, 2: slot, tiles), ext_reads (n, 2: slot, set), post
    (n, 2: launch, slot), foot (list of slot arrays, one per set).  Raises Mp2vgError for a batch
    the upload would refuse."""
    cfg = _lib.make_config(width, height, chroma_format, pool=nslots,
                           flags=_lib.MP2VG_CTX_ONE_STREAM if one_stream else 0)
    pics = np.ascontiguousarray(pics, PIC_DTYPE)
    mbs = np.ascontiguousarray(mbs, MB_DTYPE)
    coefs = np.ascontiguousarray(coefs, np.uint32)
    vp = ctypes.c_void_p
    plan = _lib.Plan()

    def call():
        check(lib().mp2vg_batch_plan(ctypes.byref(cfg), nslots, pics.ctypes.data_as(vp), len(pics),
                                     mbs.ctypes.data_as(vp), len(mbs),
                                     coefs.ctypes.data_as(vp) if len(coefs) else None, len(coefs),
                                     ctypes.byref(plan)), "batch_plan")

    call()  # counts only
    width_of = {"slices": 4, "launches": 6, "writes": 2, "ext_reads": 2, "post": 2, "foot": 2}
    out = {}
    for name, k in width_of.items():
        n = getattr(plan, "n" + name if name != "ext_reads" else "next_reads")
        a = np.zeros((n, k), np.uint32 if name == "slices" else np.int32)
        out[name] = a
        setattr(plan, "max_" + name, n)
        ct = ctypes.c_uint32 if name == "slices" else ctypes.c_int32
        setattr(plan, name, a.ctypes.data_as(ctypes.POINTER(ct)) if n else None)
    call()
    out["slices"] = out["slices"].astype(np.int64)
    ft = out["foot"]
    out["foot"] = [ft[ft[:, 0] == s, 1].copy() for s in range(plan.nsets)]
    return out


def validate_batch(width, height, chroma_format, nslots, pics, mbs, coefs):
    """Number of kernel launches of a valid batch (plan_batch); raises Mp2vgError otherwise."""
    return len(plan_batch(width, height, chroma_format, nslots, pics, mbs, coefs)[1])


class DeviceContext:
    """mp2vg_ctx_t: a frame pool in HBM plus a resident record batch on one GPU."""

    def __init__(self, width, height, chroma_format, slots, device=0, one_stream=False):
        self.width, self.height, self.chroma_format = width, height, chroma_format
        self.cfg = _lib.make_config(width, height, chroma_format, pool=slots, device=device,
                                    flags=_lib.MP2VG_CTX_ONE_STREAM if one_stream else 0)
        self.h = ctypes.c_void_p()
        check(lib().mp2vg_create(ctypes.byref(self.cfg), ctypes.byref(self.h)), "create")
        self.pw, self.ph, self.stride, self.slot_bytes = _lib.geometry(width, height, chroma_format)
        self.nslots = slots
        self.batch_pictures = 0  # pictures of the resident batch (export_motion's default order)

    def close(self):
        if self.h:
            lib().mp2vg_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reserve(self, nslots):
        """Grow the pool to nslots slots (mp2vg_reserve_slots): the slots it has keep their
        addresses and contents, the new ones read as zero; never shrinks."""
        check(lib().mp2vg_reserve_slots(self.h, int(nslots)), "reserve_slots")
        self.nslots = max(self.nslots, int(nslots))

    def slot_ptr(self, slot):
        """Device address of a slot's frame (mp2vg_slot_device_ptr); after writing through it, call
        invalidate(slot)."""
        p = ctypes.c_void_p()
        check(lib().mp2vg_slot_device_ptr(self.h, int(slot), ctypes.byref(p)), "slot_device_ptr")
        return p.value

    def invalidate(self, slot):
        """The slot's frame was written from outside the decode (mp2vg_invalidate_slot): the next
        batch that predicts from it rebuilds its anchor tiles first."""
        check(lib().mp2vg_invalidate_slot(self.h, int(slot)), "invalidate_slot")

    def upload(self, pics, mbs, coefs):
        pics = np.ascontiguousarray(pics, PIC_DTYPE)
        mbs = np.ascontiguousarray(mbs, MB_DTYPE)
        coefs = np.ascontiguousarray(coefs, np.uint32)
        vp = ctypes.c_void_p
        self.batch_pictures = 0
        check(lib().mp2vg_batch_upload(self.h, pics.ctypes.data_as(vp), len(pics), mbs.ctypes.data_as(vp), len(mbs),
                                       coefs.ctypes.data_as(vp) if len(coefs) else None, len(coefs)), "batch_upload")
        self.batch_pictures = len(pics)

    def upload_es(self, scan, first=0, npics=None, pics=None):
        """Pictures [first, first + npics) of a Scan as the resident batch, their slices parsed on
        the device (mp2vg_batch_upload_es).  pics: the range's picture records with the caller's
        slots and mb_first (default: the scan's, mb_first rebased to the range)."""
        npics = scan.npics - first if npics is None else npics
        ptr = None
        if pics is not None:
            pics = np.ascontiguousarray(pics, PIC_DTYPE)
            if len(pics) != npics:
                raise ValueError("pics must hold one record per picture of the range")
            ptr = pics.ctypes.data_as(ctypes.c_void_p)
        self.batch_pictures = 0
        check(lib().mp2vg_batch_upload_es(self.h, scan.h, ptr, int(first), int(npics)), "batch_upload_es")
        self.batch_pictures = int(npics)

    def last_damage(self):
        """The rows the last upload_es replaced (mp2vg_last_upload_damage; _lib.DAMAGE_DTYPE, pic
        relative to the uploaded range): empty for a clean upload or a scan without conceal=True."""
        return _damage_array(lambda o, m, c: lib().mp2vg_last_upload_damage(self.h, o, m, c), "last_upload_damage")

    def download_records(self):
        """(mbs, coefs) of the resident batch, copied from HBM (mp2vg_batch_download_records)."""
        nm, nc = ctypes.c_uint64(), ctypes.c_uint64()
        check(lib().mp2vg_batch_record_counts(self.h, ctypes.byref(nm), ctypes.byref(nc)), "batch_record_counts")
        mbs, coefs = np.zeros(nm.value, MB_DTYPE), np.zeros(nc.value, np.uint32)
        vp = ctypes.c_void_p
        check(lib().mp2vg_batch_download_records(self.h, mbs.ctypes.data_as(vp), len(mbs),
                                                 coefs.ctypes.data_as(vp) if len(coefs) else None, len(coefs)),
              "batch_download_records")
        return mbs, coefs

    def parse_times_ms(self):
        """Device ms of the last upload_es: [count pass, scan, emit pass] (mp2vg_last_parse_times)."""
        ms = (ctypes.c_float * 3)()
        check(lib().mp2vg_last_parse_times(self.h, ms), "last_parse_times")
        return list(ms)

    def decode(self):
        check(lib().mp2vg_batch_decode(self.h), "batch_decode")

    def synchronize(self):
        check(lib().mp2vg_synchronize(self.h), "synchronize")

    def launch_times_ms(self):
        buf = (ctypes.c_float * 256)()
        n = ctypes.c_int32()
        check(lib().mp2vg_last_launch_times(self.h, buf, 256, ctypes.byref(n)), "last_launch_times")
        return list(buf[:min(n.value, 256)])

    def batch_time_ms(self):
        """Device time of the whole last batch_decode (first launch start -> last launch end)."""
        ms = ctypes.c_float()
        check(lib().mp2vg_last_batch_time(self.h, ctypes.byref(ms)), "last_batch_time")
        return ms.value

    def batch_times(self, back=0):
        """(batch span ms, [per-launch ms]) of the batch decoded `back` decodes ago (0 = last; the
        last 64 are kept), read from the HIP events recorded when it ran."""
        ms = ctypes.c_float()
        buf = (ctypes.c_float * 256)()
        n = ctypes.c_int32()
        check(lib().mp2vg_batch_times(self.h, int(back), ctypes.byref(ms), buf, 256, ctypes.byref(n)), "batch_times")
        return ms.value, list(buf[:min(n.value, 256)])

    def batches_span(self, back_first, back_last=0):
        """Device ms from the start of the batch decoded `back_first` decodes ago to the end of the
        one `back_last` decodes ago (back-to-back batches overlap set by set)."""
        ms = ctypes.c_float()
        check(lib().mp2vg_batches_span(self.h, int(back_first), int(back_last), ctypes.byref(ms)), "batches_span")
        return ms.value

    def pool_probe(self, rw=True, reps=4):
        """Diagnostics: GB/s of each pool block (frames, tiles, frames, ... in allocation order)
        under `reps` load(+store-back) sweeps; rw=2 / 3: one rate for random / same-offset 1-KB
        reads over the pool; rw=4: per block, random 1-KB reads inside it; rw=5: the two record
        banks' MB records and coefficient words; contents kept
        (mp2vg_pool_probe)."""
        n = ctypes.c_int32()
        check(lib().mp2vg_pool_probe(self.h, int(rw), int(reps), None, 0, ctypes.byref(n)), "pool_probe")
        n.value = 1 if int(rw) in (2, 3, 6, 7) else (4 if int(rw) == 5 else n.value)
        out = np.zeros(n.value, np.float64)
        check(lib().mp2vg_pool_probe(self.h, int(rw), int(reps), out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                     n.value, ctypes.byref(n)), "pool_probe")
        return out

    def placement(self):
        """The pool placement calibration of this context (mp2vg_pool_placement): (batch ms of
        each candidate pool, round 0 then round 1; index of the pool kept, -1 if it did not run)."""
        n, kept = ctypes.c_int32(), ctypes.c_int32()
        buf = (ctypes.c_float * 16)()
        check(lib().mp2vg_pool_placement(self.h, buf, 16, ctypes.byref(n), ctypes.byref(kept)), "pool_placement")
        return [round(float(v), 4) for v in buf[:min(n.value, 16)]], kept.value

    def download(self, slot):
        """Visible planes of one slot: [Y, U, V] numpy arrays (height x width)."""
        planes = [np.empty((self.ph[i], self.pw[i]), np.uint8) for i in range(3)]
        ptrs = (ctypes.c_void_p * 3)(*[p.ctypes.data for p in planes])
        check(lib().mp2vg_download_slot(self.h, slot, ptrs, None), "download_slot")
        return planes

    def frame_bytes(self):
        """Bytes of one frame in the packed write_yuv layout (Y, U, V visible planes)."""
        return sum(self.pw[i] * self.ph[i] for i in range(3))

    def copy_packed(self, slot, dst_ptr, on_device):
        """Visible planes of `slot`, packed Y|U|V, into dst_ptr (HBM of this context's device when
        on_device, e.g. a torch tensor's data_ptr(); else host memory)."""
        check(lib().mp2vg_copy_slot_packed(self.h, int(slot), ctypes.c_void_p(dst_ptr), 1 if on_device else 0),
              "copy_slot_packed")

    def export_rgb(self, slots, out=None, layout="nchw", chroma="linear", matrix=1, size=None, sync=True):
        """Frames of `slots` (any order, repeats allowed) as one torch.uint8 RGB tensor on this
        context's device (mp2vg_export_slots: one kernel launch, no PCIe): (n, 3, h, w) for layout
        "nchw", (n, h, w, 3) for "nhwc"; chroma "linear" / "nearest" upsampling; matrix = a
        matrix_coefficients code (1 BT.709, 4 FCC, 5 / 6 BT.601, 7 SMPTE 240M); size = (width,
        height) of the top-left rectangle exported (None: the coded size).  Writes into `out` when
        given.  The export is enqueued behind the decodes enqueued so far; with sync=False it is
        complete only after synchronize().

        The export runs on the context's own (non-blocking) stream, which is not ordered with
        torch's streams: work torch has enqueued on `out` (a fill, or the last kernels that used a
        block the caching allocator hands back) must have finished before the call
        (torch.cuda.synchronize() or a stream synchronise; the producer side is the caller's job),
        and with sync=False torch must not read the tensor before synchronize().  At most 65535
        slots per call."""
        slots = np.ascontiguousarray(slots, np.int32).ravel()
        exp = _lib.make_export(layout, chroma, matrix, size)
        shape = _lib.export_shape(exp, len(slots), self.width, self.height)
        t = _lib.export_out(out, shape, self.cfg.device)
        check(lib().mp2vg_export_slots(self.h, slots.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), len(slots),
                                       ctypes.byref(exp), ctypes.c_void_p(t.data_ptr()), t.numel()), "export_slots")
        if sync:
            self.synchronize()
        return t

    def export_tensor(self, slots, size, crop=None, dtype="float16", mean=None, std=None, layout="nchw",
                      chroma="linear", matrix=1, out=None, sync=True, fields=None, place=None, fit=None,
                      pixel_aspect=(1, 1), pad=(0, 0, 0)):
        """Frames of `slots` (any order, repeats allowed) as one model-input tensor on this
        context's device (mp2vg_tensor_slots_fields: one fused kernel launch): cropped to crop = (x, y, w,
        h) in luma pixels (None: the coded frame), resized to size = (width, height) with the
        bit-exact antialiased triangle filter of include/mp2vg.h, normalised per channel and cast to
        dtype (torch.float16 / "float16", bfloat16, float32 or uint8).  With mean / std (0..1
        units) the value is (x / 255 - mean) / std, computed as fmaf(x, scale, bias) with scale =
        float32(1 / (255 std)), bias = float32(-mean / std); without them x / 255 (uint8: x).
        (n, 3, h, w) for layout "nchw", (n, h, w, 3) for "nhwc"; chroma and matrix as export_rgb.
        Writes into `out` when given.  fields: the field mode of interlaced frames (include/mp2vg.h
        "Field modes"): None, one of "progressive" / "top" / "bottom" / "weave" for every frame, or
        one of those (or the MP2VG_FIELD_* integers) per slot; a slot listed twice with "top" and
        "bottom" gives both fields of its picture.

        Placement (include/mp2vg.h "Placement", mp2vg_tensor_slots_placed, still one launch): place =
        (x, y, w, h) puts the resized picture at that rectangle of the size[0] x size[1] output and
        writes pad = (R, G, B), 8-bit, normalised like a pixel, everywhere else.  fit = "contain"
        computes the centred rectangle that keeps the shape of the crop shown with pixels of
        pixel_aspect = (n, d), width : height (records.pixel_aspect gives a stream's); "cover" the
        centre crop of that shape that fills the output; "stretch" is the export without fit.  place
        and fit exclude each other; without either the call is the one without a placement.

        Stream ordering is export_rgb's: the export runs on the context's own stream behind the
        decodes enqueued so far; work torch has enqueued on `out` must have finished before the
        call, and with sync=False torch must not read the tensor before synchronize().  At most
        65535 slots per call."""
        slots = np.ascontiguousarray(slots, np.int32).ravel()
        modes = _lib.field_modes(fields, len(slots))
        crop, pl = _lib.placement(size, crop, (self.pw[0], self.ph[0]), place, fit, pixel_aspect, pad)
        t = _lib.make_tensor(size, crop, dtype, mean, std, layout, chroma, matrix)
        o = _lib.tensor_out(out, _lib.tensor_shape(t, len(slots)), dtype, self.cfg.device)
        i32p = ctypes.POINTER(ctypes.c_int32)
        fp = None if modes is None else modes.ctypes.data_as(i32p)
        if pl is None:
            check(lib().mp2vg_tensor_slots_fields(self.h, slots.ctypes.data_as(i32p), fp, len(slots), ctypes.byref(t),
                                                  ctypes.c_void_p(o.data_ptr()), o.numel() * o.element_size()),
                  "tensor_slots_fields")
        else:
            check(lib().mp2vg_tensor_slots_placed(self.h, slots.ctypes.data_as(i32p), fp, len(slots), ctypes.byref(t),
                                                  ctypes.byref(pl), ctypes.c_void_p(o.data_ptr()),
                                                  o.numel() * o.element_size()), "tensor_slots_placed")
        if sync:
            self.synchronize()
        return o

    def export_items(self, slots, size, crops, flips=None, fields=None, clip_len=1, dtype="float16", mean=None,
                     std=None, layout="nchw", chroma="linear", matrix=1, out=None, sync=True):
        """One image per item in one kernel launch (mp2vg_tensor_items, include/mp2vg.h "Items"):
        item i is frame slots[i] (any order, repeats allowed) in field mode fields[i], cropped to
        crops[i] = (x, y, w, h) in luma pixels (None: the coded frame), resized to size = (width,
        height), mirrored left to right when flips[i], then normalised and cast as export_tensor
        does (dtype, mean, std, chroma, matrix as there).  slots, flips and fields also take one
        value for every item (_lib.make_items).  The random-resized-crop and flip of every sample
        of a batch, or every box of a detector, is one call.
        (n, 3, h, w) for layout "nchw", (n, h, w, 3) for "nhwc"; with clip_len = T > 1 the planar
        result is (n / T, 3, T, h, w), the clip layout of video models: item i is frame i % T of
        clip i / T.  Writes into `out` when given.  Stream ordering, sync and the limit of 65535
        items per call as export_tensor."""
        items = _lib.make_items(slots, crops, flips, fields)
        t = _lib.make_tensor(size, None, dtype, mean, std, layout, chroma, matrix)
        o = _lib.tensor_out(out, _lib.items_shape(t, len(items), int(clip_len)), dtype, self.cfg.device)
        check(lib().mp2vg_tensor_items(self.h, items, len(items), ctypes.byref(t), int(clip_len),
                                       ctypes.c_void_p(o.data_ptr()), o.numel() * o.element_size()), "tensor_items")
        if sync:
            self.synchronize()
        return o

    def export_motion(self, order=None, mv=True, info=True, act=True, sync=True):
        """The resident batch's motion field and block activity as torch tensors on this context's
        device (mp2vg_motion_batch, include/mp2vg.h "motion export"): (mv int16 (n, 8, mbh, mbw),
        info uint16 (n, 4, mbh, mbw), act int32 (n, 2, B, mbh, mbw)), None for one not asked for.
        order: indices into the batch's pictures, any order, repeats allowed (None: every picture
        in batch order).  Reads the records, not the slots: no decode() is needed.  Stream ordering
        and sync as export_rgb."""
        import torch
        if order is None:
            order = np.arange(self.batch_pictures, dtype=np.int32)
        order = np.ascontiguousarray(order, np.int32).ravel()
        n, mbw, mbh = len(order), self.width // 16, self.height // 16
        nb = {1: 6, 2: 8, 3: 12}[self.chroma_format]
        dev = torch.device("cuda", self.cfg.device)
        shapes = [((n, 8, mbh, mbw), torch.int16), ((n, 4, mbh, mbw), torch.uint16), ((n, 2, nb, mbh, mbw), torch.int32)]
        outs = [torch.empty(s, dtype=d, device=dev) if want else None
                for (s, d), want in zip(shapes, (mv, info, act))]
        torch.cuda.synchronize(dev)  # the allocator's earlier users of these blocks have finished
        bytes3 = (ctypes.c_uint64 * 3)(*[0 if t is None else t.numel() * t.element_size() for t in outs])
        ptrs = [None if t is None else ctypes.c_void_p(t.data_ptr()) for t in outs]
        check(lib().mp2vg_motion_batch(self.h, order.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), n, ptrs[0],
                                       ptrs[1], ptrs[2], bytes3), "motion_batch")
        if sync:
            self.synchronize()
        return tuple(outs)

    def motion_time_ms(self):
        """Device ms of the kernels of the last export_motion (mp2vg_last_motion_time)."""
        ms = ctypes.c_float()
        check(lib().mp2vg_last_motion_time(self.h, ctypes.byref(ms)), "last_motion_time")
        return ms.value

    def export_residual(self, order=None, dtype="int16", chroma=True, zero_intra=False, sync=True):
        """The resident batch's coded prediction error as torch tensors on this context's device
        (mp2vg_residual_batch, include/mp2vg.h "residual export"): (y (n, H, W), cb, cr (n, ch, cw))
        of int16 (clamped to -255 .. 255) or int8 (-128 .. 127); cb and cr are None without chroma.
        order: indices into the batch's pictures, any order, repeats allowed (None: every picture
        in batch order).  zero_intra: intra macroblocks are written as zeros.  Reads the records,
        not the slots: no decode() is needed.  Stream ordering and sync as export_rgb."""
        import torch
        name, code = _lib.residual_dtype(dtype)
        if order is None:
            order = np.arange(self.batch_pictures, dtype=np.int32)
        order = np.ascontiguousarray(order, np.int32).ravel()
        dev = torch.device("cuda", self.cfg.device)
        shapes = _lib.residual_shapes(self.width, self.height, self.chroma_format, len(order))
        outs = [torch.empty(s, dtype=getattr(torch, name), device=dev) if want else None
                for s, want in zip(shapes, (True, chroma, chroma))]
        torch.cuda.synchronize(dev)  # the allocator's earlier users of these blocks have finished
        bytes3 = (ctypes.c_uint64 * 3)(*[0 if t is None else t.numel() * t.element_size() for t in outs])
        ptrs = [None if t is None else ctypes.c_void_p(t.data_ptr()) for t in outs]
        check(lib().mp2vg_residual_batch(self.h, order.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), len(order), code,
                                         _lib.RESIDUAL_ZERO_INTRA if zero_intra else 0, ptrs[0], ptrs[1], ptrs[2],
                                         bytes3), "residual_batch")
        if sync:
            self.synchronize()
        return tuple(outs)

    def residual_time_ms(self):
        """Device ms of the kernel of the last export_residual (mp2vg_last_residual_time)."""
        ms = ctypes.c_float()
        check(lib().mp2vg_last_residual_time(self.h, ctypes.byref(ms)), "last_residual_time")
        return ms.value

    def digests(self, slots):
        slots = np.ascontiguousarray(slots, np.int32)
        out = np.zeros(len(slots), np.uint64)
        check(lib().mp2vg_slot_digests(self.h, slots.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), len(slots),
                                       out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))), "slot_digests")
        return out


EXPORT_MAX_FRAMES = 65535  # frames per mp2vg_export_slots call (include/mp2vg.h)


def export_matrix(headers):
    """The matrix_coefficients code to export a stream with (mp2vg_export_matrix): the stream's own
    when it carries a usable one, else 1 (BT.709)."""
    m = ctypes.c_int32()
    check(lib().mp2vg_export_matrix(ctypes.byref(headers), ctypes.byref(m)), "export_matrix")
    return m.value


def pixel_aspect(headers):
    """(n, d), the pixel's width : height of a stream from its aspect_ratio_information
    (mp2vg_stream_pixel_aspect); Mp2vgError for a code that gives none."""
    n, d = ctypes.c_int32(), ctypes.c_int32()
    check(lib().mp2vg_stream_pixel_aspect(ctypes.byref(headers), ctypes.byref(n), ctypes.byref(d)),
          "stream_pixel_aspect")
    return n.value, d.value


stream_pixel_aspect = pixel_aspect  # for functions with a `pixel_aspect` argument


def _open_stream(es, width, height, chroma_format, device_parse, conceal, standard=False, slices=False):
    return (Scan if device_parse else Parsed)(es, width, height, chroma_format, conceal=conceal, standard=standard,
                                              slices=slices)


def probe(es):
    """What a stream says about itself before anything is parsed (mp2vg_probe_es): a dict with the
    coded `width` and `height` and the `chroma_format` every other entry point asks for, the
    `display_width` and `display_height` (the 14-bit horizontal_size and vertical_size) and the
    stream `headers` (_lib.StreamHeaders: sequence header, sequence extension and, when one
    follows them, the sequence display extension).  Mp2vgError for an MPEG-1 stream, a size outside
    the limits, or a buffer without a sequence header."""
    buf = np.frombuffer(es, dtype=np.uint8)
    cfg, hd = _lib.make_config(0, 0, 0), _lib.StreamHeaders()
    check(lib().mp2vg_probe_es(buf.ctypes.data_as(ctypes.c_void_p), len(es), ctypes.byref(cfg), ctypes.byref(hd)),
          "probe_es")
    sh, se = hd.sequence_header, hd.sequence_extension
    return {"width": cfg.width, "height": cfg.height, "chroma_format": cfg.chroma_format,
            "display_width": int(sh.horizontal_size_value | se.horizontal_size_extension << 12),
            "display_height": int(sh.vertical_size_value | se.vertical_size_extension << 12), "headers": hd}


def _make_resident(ctx, parsed, device_parse):
    """Upload a Scan (device parse) or a Parsed; returns the damage list of a conceal=True stream."""
    if device_parse:
        ctx.upload_es(parsed)
        return ctx.last_damage()
    ctx.upload(parsed.pics, parsed.mbs, parsed.coefs)
    return parsed.damage


def decode_rgb(es, width, height, chroma_format, layout="nchw", chroma="linear", matrix=None, device=0,
               device_parse=False, conceal=False, return_damage=False, standard=False, slices=False):
    """Decode a whole elementary stream (coded size width x height) and return its pictures in
    display order as one torch.uint8 RGB tensor on cuda:<device>, cropped to the sequence header's
    horizontal_size_value x vertical_size_value when these are set and no larger than the coded
    size.  matrix=None takes the stream's matrix_coefficients (export_matrix).  The stream is one
    batch in a context of as many slots as it has pictures; a stream without pictures gives an
    empty tensor, and one of more than 65535 pictures is exported in several calls.
    device_parse=True scans the stream on the host and parses its slices on the device (Scan,
    DeviceContext.upload_es) instead of uploading host-parsed records; the result is the same.
    conceal=True decodes a damaged stream (MP2VG_PARSE_CONCEAL: damaged rows are replaced instead of
    failing the call); return_damage=True returns (tensor, damage), damage as Parsed.damage.
    standard=True (MP2VG_PARSE_STANDARD) admits streams of ordinary encoders, as for Parsed;
    slices=True (MP2VG_PARSE_SLICES) any number of slices per macroblock row."""
    parsed = _open_stream(es, width, height, chroma_format, device_parse, conceal, standard, slices)
    sh = parsed.headers.sequence_header
    w, h = int(sh.horizontal_size_value), int(sh.vertical_size_value)
    size = (w, h) if 0 < w <= width and 0 < h <= height else None
    if matrix is None:
        matrix = export_matrix(parsed.headers)
    exp = _lib.make_export(layout, chroma, matrix, size)
    out = _lib.export_out(None, _lib.export_shape(exp, parsed.npics, width, height), device)
    if not parsed.npics:
        return (out, np.zeros(0, _lib.DAMAGE_DTYPE)) if return_damage else out
    with DeviceContext(width, height, chroma_format, slots=parsed.npics, device=device) as ctx:
        damage = _make_resident(ctx, parsed, device_parse)
        ctx.decode()
        for i in range(0, parsed.npics, EXPORT_MAX_FRAMES):  # mp2vg_export_slots takes 65535 per call
            part = parsed.display[i:i + EXPORT_MAX_FRAMES]
            ctx.export_rgb(part, out=out[i:i + len(part)], layout=layout, chroma=chroma, matrix=matrix, size=size,
                           sync=False)
        ctx.synchronize()
        return (out, damage) if return_damage else out


def items_plan(width, height, chroma_format, size, crops, flips=None, fields=None, clip_len=1, slots=0, dtype="float16",
               layout="nchw", items=None):
    """What an items launch (DeviceContext.export_items) stages and launches, with no device
    (mp2vg_tensor_items_plan): a dict of htab / vtab (the tap table of each item per axis, tables
    numbered in order of first use), n_htab / n_vtab (distinct tables), grid_x (the largest segment
    count of any item) and words (int32 words staged: the item records, then the tables).  Raises
    Mp2vgError where the launch would be refused.  items: a ready (_lib.Item * n) array instead of
    slots / crops / flips / fields."""
    if items is None:
        items = _lib.make_items(slots, crops, flips, fields)
    n = len(items)
    cfg = _lib.make_config(width, height, chroma_format)
    t = _lib.make_tensor(size, None, dtype, layout=layout)
    htab, vtab, summary = np.zeros(n, np.int32), np.zeros(n, np.int32), (ctypes.c_int32 * 4)()
    i32p = ctypes.POINTER(ctypes.c_int32)
    check(lib().mp2vg_tensor_items_plan(ctypes.byref(cfg), ctypes.byref(t), items, n, int(clip_len),
                                        htab.ctypes.data_as(i32p), vtab.ctypes.data_as(i32p), summary),
          "tensor_items_plan")
    return {"htab": htab, "vtab": vtab, "n_htab": summary[0], "n_vtab": summary[1], "grid_x": summary[2],
            "words": summary[3]}


def field_plan(display, flags, fields):
    """(slots, modes) of decode_tensor's `fields`: the display-order slot list, each picture once or
    ("both") twice, and the MP2VG_FIELD_* mode of each entry (None: no list)."""
    display = np.asarray(display, np.int32)
    if fields is None:
        return display, None
    if fields in ("weave", "top", "bottom"):
        return display, np.full(len(display), _lib.FIELDS[fields], np.int32)
    if fields not in ("first", "both"):
        raise ValueError(f"fields {fields!r}: expected None, 'weave', 'top', 'bottom', 'first' or 'both'")
    fl = np.asarray(flags, np.uint32)[display]
    progressive = (fl & _lib.PIC_PROGRESSIVE_FRAME) != 0
    tff = (fl & _lib.PIC_TOP_FIELD_FIRST) != 0
    first = np.where(progressive, _lib.FIELD_PROGRESSIVE, np.where(tff, _lib.FIELD_TOP, _lib.FIELD_BOTTOM))
    if fields == "first":
        return display, first.astype(np.int32)
    second = np.where(progressive, _lib.FIELD_PROGRESSIVE, np.where(tff, _lib.FIELD_BOTTOM, _lib.FIELD_TOP))
    return np.repeat(display, 2), np.stack([first, second], axis=1).ravel().astype(np.int32)


def decode_tensor(es, width, height, chroma_format, size, crop=None, dtype="float16", mean=None, std=None,
                  layout="nchw", chroma="linear", matrix=None, device=0, device_parse=False, fields=None, fit=None,
                  pad=(0, 0, 0), pixel_aspect="stream", conceal=False, return_damage=False, standard=False,
                  slices=False):
    """Decode a whole elementary stream (coded size width x height) and return its pictures in
    display order as one model-input tensor on cuda:<device> (DeviceContext.export_tensor: size,
    dtype, mean / std, layout and chroma as there).  crop=None takes the sequence header's
    horizontal_size_value x vertical_size_value at the top left when these are set and no larger
    than the coded size, else the coded frame; matrix=None takes the stream's matrix_coefficients.
    A stream without pictures gives an empty tensor, and one of more than 65535 pictures is
    exported in several calls.  device_parse as in decode_rgb.

    fields (include/mp2vg.h "Field modes"): None exports every picture as a progressive frame;
    "weave", "top" or "bottom" that mode for every picture; "first" a progressive frame for pictures
    with progressive_frame = 1 and else the picture's first field (the top field if
    top_field_first, else the bottom one), n frames; "both" 2n frames in temporal order: an
    interlaced picture gives its first field, then its second, a progressive picture its frame
    twice.  repeat_first_field (3:2 pulldown) is reported in Parsed.flags but ignored here: no
    field is repeated.

    fit (DeviceContext.export_tensor): "contain" letterboxes the source rectangle (crop, or the
    rectangle picked above) into size with the pad colour around it, "cover" fills size with its
    centre crop, both at the shape the stream is shown at: pixel_aspect="stream" takes the stream's
    own (records.pixel_aspect; a stream whose aspect code gives none raises Mp2vgError, it is not
    guessed at), a tuple (n, d) overrides it.

    conceal, return_damage, standard and slices as in decode_rgb."""
    parsed = _open_stream(es, width, height, chroma_format, device_parse, conceal, standard, slices)
    sh = parsed.headers.sequence_header
    w, h = int(sh.horizontal_size_value), int(sh.vertical_size_value)
    if crop is None and 0 < w <= width and 0 < h <= height:
        crop = (0, 0, w, h)
    if matrix is None:
        matrix = export_matrix(parsed.headers)
    slots, modes = field_plan(parsed.display, parsed.flags, fields)
    place = None
    if fit is not None:
        if isinstance(pixel_aspect, str) and pixel_aspect != "stream":
            raise ValueError(f"pixel_aspect {pixel_aspect!r}: expected 'stream' or (n, d)")
        par = stream_pixel_aspect(parsed.headers) if pixel_aspect == "stream" else pixel_aspect
        pw, ph, _, _ = _lib.geometry(width, height, chroma_format)
        crop, place = _lib.tensor_fit(fit, (0, 0, pw[0], ph[0]) if crop is None else crop, par, size)
    t = _lib.make_tensor(size, crop, dtype, mean, std, layout, chroma, matrix)
    out = _lib.tensor_out(None, _lib.tensor_shape(t, len(slots)), dtype, device)
    if not parsed.npics:
        return (out, np.zeros(0, _lib.DAMAGE_DTYPE)) if return_damage else out
    with DeviceContext(width, height, chroma_format, slots=parsed.npics, device=device) as ctx:
        damage = _make_resident(ctx, parsed, device_parse)
        ctx.decode()
        for i in range(0, len(slots), EXPORT_MAX_FRAMES):  # mp2vg_tensor_slots_fields takes 65535 per call
            part = slots[i:i + EXPORT_MAX_FRAMES]
            ctx.export_tensor(part, size, crop=crop, dtype=dtype, mean=mean, std=std, layout=layout, chroma=chroma,
                              matrix=matrix, out=out[i:i + len(part)], sync=False,
                              fields=None if modes is None else modes[i:i + len(part)], place=place, pad=pad)
        ctx.synchronize()
        return (out, damage) if return_damage else out


def motion_bytes(width, height, chroma_format, n):
    """(mv, info, act) byte sizes of n pictures (mp2vg_motion_bytes)."""
    cfg = _lib.make_config(width, height, chroma_format)
    b = (ctypes.c_uint64 * 3)()
    check(lib().mp2vg_motion_bytes(ctypes.byref(cfg), int(n), b), "motion_bytes")
    return tuple(int(v) for v in b)


def motion_host(pics, mbs, coefs, width, height, chroma_format, order=None):
    """numpy (mv, info, act) of host records through the host twin of the motion export
    (mp2vg_motion_records; include/mp2vg.h "motion export"), no device: mv int16 (n, 8, mbh, mbw),
    info uint16 (n, 4, mbh, mbw), act int32 (n, 2, B, mbh, mbw).  order: indices into pics (None:
    every picture in batch order).  Raises Mp2vgError for a batch the upload would refuse."""
    cfg = _lib.make_config(width, height, chroma_format)
    pics = np.ascontiguousarray(pics, PIC_DTYPE)
    mbs = np.ascontiguousarray(mbs, MB_DTYPE)
    coefs = np.ascontiguousarray(coefs, np.uint32)
    order = np.arange(len(pics), dtype=np.int32) if order is None else np.ascontiguousarray(order, np.int32).ravel()
    n, mbw, mbh = len(order), width // 16, height // 16
    nb = {1: 6, 2: 8, 3: 12}[chroma_format]
    mv = np.zeros((n, 8, mbh, mbw), np.int16)
    info = np.zeros((n, 4, mbh, mbw), np.uint16)
    act = np.zeros((n, 2, nb, mbh, mbw), np.int32)
    vp = ctypes.c_void_p
    check(lib().mp2vg_motion_records(ctypes.byref(cfg), pics.ctypes.data_as(vp), len(pics), mbs.ctypes.data_as(vp),
                                     len(mbs), coefs.ctypes.data_as(vp) if len(coefs) else None, len(coefs),
                                     order.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), n, mv.ctypes.data_as(vp),
                                     info.ctypes.data_as(vp), act.ctypes.data_as(vp)), "motion_records")
    return mv, info, act


def reference_pictures(pics):
    """int32 (n, 2): per picture of a batch, the batch index of its forward and of its backward
    reference: the last earlier picture that wrote fwd_slot / bwd_slot, -1 if there is none."""
    out = np.full((len(pics), 2), -1, np.int32)
    writer = {}
    for i, p in enumerate(pics):
        for s, name in enumerate(("fwd_slot", "bwd_slot")):
            out[i, s] = writer.get(int(p[name]), -1) if int(p[name]) >= 0 else -1
        writer[int(p["dst_slot"])] = i
    return out


def reference_distances(pics, display):
    """int32 (n, 2), in display order: the signed display-order distance from each picture to its
    forward and backward reference (reference_pictures), 0 where there is none."""
    display = np.asarray(display, np.int64)
    pos = np.zeros(len(pics), np.int64)
    pos[display] = np.arange(len(display))
    ref = reference_pictures(pics)[display].astype(np.int64)
    here = np.arange(len(display))[:, None]
    return np.where(ref >= 0, pos[np.maximum(ref, 0)] - here, 0).astype(np.int32)


def decode_motion(es, width, height, chroma_format, parse="device", device=0, conceal=False, standard=False,
                  slices=False):
    """The motion field and block activity of a whole elementary stream in display order, with no
    reconstruction: scan (parse="device": slices parsed on the device, DeviceContext.upload_es) or
    parse (parse="host": Parsed, upload) the stream, make it resident and export
    (DeviceContext.export_motion).  A dict of mv, info and act (torch tensors on cuda:<device>) and
    dist, numpy int32 (n, 2): the signed display-order distance from each picture to its forward
    and backward reference, 0 where there is none (vectors per frame: mv / dist).  At most 65535
    pictures.  conceal=True (MP2VG_PARSE_CONCEAL) exports a damaged stream, its replaced rows as
    the records that replace them; the dict then holds 'damage' (as Parsed.damage), and dist follows
    the pictures as decoded (effective_pictures: a re-typed I picture has a forward reference)."""
    if parse not in ("device", "host"):
        raise ValueError(f"parse {parse!r}: expected 'device' or 'host'")
    import torch
    torch.cuda.init()  # torch's runtime before the context's first HIP call, as in decode_rgb
    parsed = _open_stream(es, width, height, chroma_format, parse == "device", conceal, standard, slices)
    if not parsed.npics:
        raise ValueError("the stream has no pictures")
    with DeviceContext(width, height, chroma_format, slots=parsed.npics, device=device) as ctx:
        damage = _make_resident(ctx, parsed, parse == "device")
        mv, info, act = ctx.export_motion(parsed.display)
    pics = effective_pictures(parsed.pics, damage) if conceal else parsed.pics
    out = {"mv": mv, "info": info, "act": act, "dist": reference_distances(pics, parsed.display)}
    if conceal:
        out["damage"] = damage
    return out


def residual_bytes(width, height, chroma_format, n, dtype="int16"):
    """(y, cb, cr) byte sizes of n pictures (mp2vg_residual_bytes)."""
    cfg = _lib.make_config(width, height, chroma_format)
    b = (ctypes.c_uint64 * 3)()
    check(lib().mp2vg_residual_bytes(ctypes.byref(cfg), int(n), _lib.residual_dtype(dtype)[1], b), "residual_bytes")
    return tuple(int(v) for v in b)


def residual_host(pics, mbs, coefs, width, height, chroma_format, order=None, dtype="int16", zero_intra=False):
    """numpy (y, cb, cr) of host records through the host twin of the residual export
    (mp2vg_residual_records; include/mp2vg.h "residual export"), no device: y (n, H, W), cb and cr
    (n, ch, cw) of int16 or int8.  order: indices into pics (None: every picture in batch order).
    Raises Mp2vgError for a batch the upload would refuse."""
    name, code = _lib.residual_dtype(dtype)
    cfg = _lib.make_config(width, height, chroma_format)
    pics = np.ascontiguousarray(pics, PIC_DTYPE)
    mbs = np.ascontiguousarray(mbs, MB_DTYPE)
    coefs = np.ascontiguousarray(coefs, np.uint32)
    order = np.arange(len(pics), dtype=np.int32) if order is None else np.ascontiguousarray(order, np.int32).ravel()
    outs = [np.zeros(s, name) for s in _lib.residual_shapes(width, height, chroma_format, len(order))]
    vp = ctypes.c_void_p
    check(lib().mp2vg_residual_records(ctypes.byref(cfg), pics.ctypes.data_as(vp), len(pics), mbs.ctypes.data_as(vp),
                                       len(mbs), coefs.ctypes.data_as(vp) if len(coefs) else None, len(coefs),
                                       order.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), len(order), code,
                                       _lib.RESIDUAL_ZERO_INTRA if zero_intra else 0, outs[0].ctypes.data_as(vp),
                                       outs[1].ctypes.data_as(vp), outs[2].ctypes.data_as(vp)), "residual_records")
    return tuple(outs)


def decode_residual(es, width, height, chroma_format, pictures=None, dtype="int16", chroma=True, zero_intra=False,
                    parse="device", device=0, conceal=False, standard=False, slices=False):
    """The coded prediction error of an elementary stream's pictures in display order, with no
    reconstruction: scan (parse="device": slices parsed on the device, DeviceContext.upload_es) or
    parse (parse="host": Parsed, upload) the stream, make it resident and export once
    (DeviceContext.export_residual).  pictures: display indices (None: all of them).  A dict of y, cb
    and cr (torch tensors on cuda:<device>, cb and cr None without chroma) and types, numpy int32:
    the picture_coding_type (1 I, 2 P, 3 B) of each exported picture.  Size: a 4:2:0 picture at
    int16 is 2 x 1.5 x W x H bytes (half that at int8), so a long stream is exported in ranges of
    pictures.  At most 65535 pictures.  conceal=True (MP2VG_PARSE_CONCEAL) exports a damaged stream:
    the dict then holds 'damage' (as Parsed.damage), and types are those of the pictures as decoded
    (a re-typed I picture is 2)."""
    if parse not in ("device", "host"):
        raise ValueError(f"parse {parse!r}: expected 'device' or 'host'")
    import torch
    torch.cuda.init()  # torch's runtime before the context's first HIP call, as in decode_rgb
    parsed = _open_stream(es, width, height, chroma_format, parse == "device", conceal, standard, slices)
    if not parsed.npics:
        raise ValueError("the stream has no pictures")
    display = np.asarray(parsed.display, np.int32)
    order = display if pictures is None else display[np.asarray(pictures, np.int64)]
    with DeviceContext(width, height, chroma_format, slots=parsed.npics, device=device) as ctx:
        damage = _make_resident(ctx, parsed, parse == "device")
        y, cb, cr = ctx.export_residual(order, dtype=dtype, chroma=chroma, zero_intra=zero_intra)
    pics = effective_pictures(parsed.pics, damage) if conceal else parsed.pics
    out = {"y": y, "cb": cb, "cr": cr, "types": np.asarray(pics["picture_coding_type"], np.int32)[order]}
    if conceal:
        out["damage"] = damage
    return out


def frame_yuv_bytes(planes):
    """The reference sample's write_yuv layout (tiny_mp2v_dec.cpp:11-17): Y, U, V rows of width."""
    return b"".join(np.ascontiguousarray(p).tobytes() for p in planes)


def _mix64(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def planes_digest(planes):
    """Host twin of the device digest (recon.hip digest_kernel): sum over visible dwords d at
    (row_id, byte x), rows numbered across Y, U, V, of mix64(mix64((row_id << 32) | x) ^ d), mod 2^64
    (mixed after combining: paired small errors cannot cancel)."""
    total = np.uint64(0)
    row0 = 0
    with np.errstate(over="ignore"):
        for p in planes:
            p = np.ascontiguousarray(p)
            h, w = p.shape
            d = p.view("<u4").astype(np.uint64)  # (h, w/4)
            rows = (np.arange(h, dtype=np.uint64) + np.uint64(row0))[:, None]
            xs = (np.arange(w // 4, dtype=np.uint64) * np.uint64(4))[None, :]
            total = total + np.sum(_mix64(_mix64((rows << np.uint64(32)) | xs) ^ d), dtype=np.uint64)
            row0 += h
    return int(total)
