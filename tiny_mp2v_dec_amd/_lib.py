"""ctypes binding of the C ABI (include/mp2vg.h) and numpy views of the record stream.

The native library is REQUIRED: there is no Python or CPU fallback for the reconstruct path.
Loading fails loudly when libmp2vg.so is missing (run tiny_mp2v_dec_amd/build.py).
"""
import ctypes
import os

import numpy as np

PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MP2VG_LIB") or os.path.join(PKG, "_build", "libmp2vg.so")  # override: dev A/B builds

# ---- record dtypes (must match include/mp2vg.h) ------------------------------------------
MB_DTYPE = np.dtype([("x", "<u2"), ("y", "<u2"), ("flags", "<u2"), ("cbp", "<u2"), ("qscale", "u1"),
                     ("reserved", "u1"), ("ncoef", "<u2"), ("coef_off", "<u4"), ("mv", "<i2", (2, 2, 2))])
assert MB_DTYPE.itemsize == 32
PIC_DTYPE = np.dtype([("dst_slot", "<i4"), ("fwd_slot", "<i4"), ("bwd_slot", "<i4"),
                      ("picture_coding_type", "<i4"), ("mb_first", "<u4"), ("mb_width", "<u2"),
                      ("mb_height", "<u2"), ("alternate_scan", "u1"), ("reserved0", "u1", (3,)),
                      ("temporal_reference", "<i4"), ("W", "u1", (4, 64))])
assert PIC_DTYPE.itemsize == 288
DAMAGE_DTYPE = np.dtype([("pic", "<i4"), ("mb_row", "<i4"), ("status", "<i4"), ("reason", "<i4"),
                         ("byte_off", "<u8")])  # mp2vg_damage_t
assert DAMAGE_DTYPE.itemsize == 24

MB_INTRA, MB_FWD, MB_BWD, MB_FIELD_MC, MB_DCT_FIELD = 1, 2, 4, 8, 16
COEF_FIRST1S, COEF_DC = 1 << 29, 1 << 30


def mb_fs_bit(r, s):
    return 1 << (8 + 2 * r + s)


def coef_pack(level, pos, block, flags=0, mbx=0):
    """Coefficient word (include/mp2vg.h); mbx = the MB's column (bits 26-28 carry mbx & 7)."""
    return (np.uint32(np.int64(level) & 0xFFFF) | np.uint32(pos << 16) | np.uint32(block << 22) |
            np.uint32(flags) | np.uint32((int(mbx) & 7) << 26))


STATUS = {0: "ok", -1: "invalid argument", -2: "unsupported stream", -3: "HIP error", -4: "out of memory",
          -5: "call out of order", -6: "bitstream error"}


class Mp2vgError(RuntimeError):
    def __init__(self, status, what, detail=""):
        self.status = status
        super().__init__(f"{what}: {STATUS.get(status, status)} ({detail})")


class Config(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("chroma_format", ctypes.c_int32),
                ("pictures_pool_size", ctypes.c_int32), ("num_threads", ctypes.c_int32),
                ("reordering", ctypes.c_int32), ("device", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class GenParams(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in (
        "width", "height", "chroma_format", "n_gops", "gop_n", "gop_m")] + [("seed", ctypes.c_uint32)] + [
        (n, ctypes.c_int32) for n in (
            "frame_pred_frame_dct", "alternate_scan", "q_scale_type", "intra_dc_precision", "coefs_min",
            "coefs_max", "intra_coefs_min", "intra_coefs_max", "big_level_permille", "escape_permille",
            "quant_permille", "f_code", "mix", "leading_b", "big_matrix_permille", "top_field_first")] + [
        ("reserved", ctypes.c_int32 * 4)]


class Frame(ctypes.Structure):
    _fields_ = [("planes", ctypes.POINTER(ctypes.c_uint8) * 3), ("width", ctypes.c_int32 * 3),
                ("height", ctypes.c_int32 * 3), ("stride", ctypes.c_int32 * 3),
                ("picture_coding_type", ctypes.c_int32), ("decode_index", ctypes.c_int32),
                ("device", ctypes.c_int32)]


class SequenceHeader(ctypes.Structure):  # mp2vg_sequence_header_t (reference mp2v_hdr.h:61-75)
    _fields_ = [(n, ctypes.c_uint32) for n in (
        "sequence_header_code", "horizontal_size_value", "vertical_size_value", "aspect_ratio_information",
        "frame_rate_code", "bit_rate_value", "vbv_buffer_size_value", "constrained_parameters_flag",
        "load_intra_quantiser_matrix")] + [("intra_quantiser_matrix", ctypes.c_uint8 * 64),
                                           ("load_non_intra_quantiser_matrix", ctypes.c_uint32),
                                           ("non_intra_quantiser_matrix", ctypes.c_uint8 * 64)]


class SequenceExtension(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in (
        "extension_start_code", "extension_start_code_identifier", "profile_and_level_indication",
        "progressive_sequence", "chroma_format", "horizontal_size_extension", "vertical_size_extension",
        "bit_rate_extension", "vbv_buffer_size_extension", "low_delay", "frame_rate_extension_n",
        "frame_rate_extension_d")]


class SequenceDisplayExtension(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in (
        "extension_start_code_identifier", "video_format", "colour_description", "colour_primaries",
        "transfer_characteristics", "matrix_coefficients", "display_horizontal_size", "display_vertical_size")]


class GopHeader(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in ("group_start_code", "time_code", "closed_gop", "broken_link")]


class StreamHeaders(ctypes.Structure):  # mp2vg_stream_headers_t
    _fields_ = [("have_sequence_display_extension", ctypes.c_int32),
                ("have_group_of_pictures_header", ctypes.c_int32),
                ("sequence_header", SequenceHeader), ("sequence_extension", SequenceExtension),
                ("sequence_display_extension", SequenceDisplayExtension),
                ("group_of_pictures_header", GopHeader)]


class Export(ctypes.Structure):  # mp2vg_export_t
    _fields_ = [("layout", ctypes.c_int32), ("matrix", ctypes.c_int32), ("chroma", ctypes.c_int32),
                ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("reserved", ctypes.c_int32 * 3)]


class Plan(ctypes.Structure):  # mp2vg_plan_t
    _fields_ = [("slices", ctypes.POINTER(ctypes.c_uint32))] + [
        (n, ctypes.POINTER(ctypes.c_int32)) for n in ("launches", "writes", "ext_reads", "post", "foot")] + [
        (n, ctypes.c_int32) for n in (
            "max_slices", "max_launches", "max_writes", "max_ext_reads", "max_post", "max_foot",
            "nslices", "nlaunches", "nwrites", "next_reads", "npost", "nfoot", "nsets", "reserved")]


EXPORT_RGB_PLANAR, EXPORT_RGB_PACKED = 0, 1
EXPORT_CHROMA_NEAREST, EXPORT_CHROMA_LINEAR = 0, 1

class Tensor(ctypes.Structure):  # mp2vg_tensor_t
    _fields_ = [("layout", ctypes.c_int32), ("matrix", ctypes.c_int32), ("chroma", ctypes.c_int32),
                ("src_x", ctypes.c_int32), ("src_y", ctypes.c_int32), ("src_w", ctypes.c_int32),
                ("src_h", ctypes.c_int32), ("out_w", ctypes.c_int32), ("out_h", ctypes.c_int32),
                ("dtype", ctypes.c_int32), ("scale", ctypes.c_float * 3), ("bias", ctypes.c_float * 3),
                ("reserved", ctypes.c_int32 * 4)]


class Place(ctypes.Structure):  # mp2vg_tensor_place_t
    _fields_ = [("dst_x", ctypes.c_int32), ("dst_y", ctypes.c_int32), ("dst_w", ctypes.c_int32),
                ("dst_h", ctypes.c_int32), ("pad", ctypes.c_uint8 * 3), ("reserved0", ctypes.c_uint8),
                ("reserved", ctypes.c_int32 * 3)]


assert ctypes.sizeof(Place) == 32


class Item(ctypes.Structure):  # mp2vg_tensor_item_t
    _fields_ = [(n, ctypes.c_int32) for n in ("slot", "field", "src_x", "src_y", "src_w", "src_h", "flags", "reserved")]


assert ctypes.sizeof(Item) == 32
ITEM_HFLIP = 1  # MP2VG_ITEM_*
FIT_STRETCH, FIT_CONTAIN, FIT_COVER = 0, 1, 2  # MP2VG_FIT_*
FITS = {"stretch": FIT_STRETCH, "contain": FIT_CONTAIN, "cover": FIT_COVER}
TENSOR_U8, TENSOR_F16, TENSOR_BF16, TENSOR_F32 = 0, 1, 2, 3
TENSOR_MAX_TAPS = 65
FIELD_PROGRESSIVE, FIELD_TOP, FIELD_BOTTOM, FIELD_WEAVE = 0, 1, 2, 3  # MP2VG_FIELD_*
FIELDS = {"progressive": FIELD_PROGRESSIVE, "top": FIELD_TOP, "bottom": FIELD_BOTTOM, "weave": FIELD_WEAVE}
PIC_PROGRESSIVE_FRAME, PIC_TOP_FIELD_FIRST, PIC_REPEAT_FIRST_FIELD = 1, 2, 4  # MP2VG_PIC_*
PIC_CONCEALED, PIC_RETYPED_I = 8, 16
TENSOR_DTYPES = {"uint8": (TENSOR_U8, 1), "float16": (TENSOR_F16, 2), "bfloat16": (TENSOR_BF16, 2),
                 "float32": (TENSOR_F32, 4)}  # name -> (MP2VG_TENSOR_*, element size)

RENDER_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.POINTER(Frame))

# every symbol declared in include/mp2vg.h
EXPORTS = [
    "mp2vg_abi_version", "mp2vg_status_string", "mp2vg_last_error", "mp2vg_create", "mp2vg_destroy",
    "mp2vg_frame_geometry", "mp2vg_reserve_slots", "mp2vg_batch_upload", "mp2vg_batch_validate", "mp2vg_batch_plan", "mp2vg_batch_decode",
    "mp2vg_synchronize", "mp2vg_last_launch_times", "mp2vg_last_batch_time", "mp2vg_batch_times", "mp2vg_batches_span", "mp2vg_download_slot", "mp2vg_copy_slot_packed", "mp2vg_slot_device_ptr", "mp2vg_sink_device_ptr", "mp2vg_clock_probe", "mp2vg_pool_probe", "mp2vg_pool_placement", "mp2vg_cpu_budget", "mp2vg_invalidate_slot",
    "mp2vg_slot_digests", "mp2vg_parse_es", "mp2vg_parsed_counts", "mp2vg_parsed_pictures", "mp2vg_parsed_mbs",
    "mp2vg_parsed_coefs", "mp2vg_parsed_display_order", "mp2vg_parsed_gop_index", "mp2vg_parsed_stream_headers",
    "mp2vg_parsed_shards", "mp2vg_parsed_free", "mp2vg_vlc_decode",
    "mp2vg_gen_default_params", "mp2vg_generate_es", "mp2vg_free", "mp2vg_decoder_create",
    "mp2vg_decoder_create_multi", "mp2vg_decoder_decode", "mp2vg_decoder_stream_headers",
    "mp2vg_decoder_lane_frames", "mp2vg_decoder_frames_allocated", "mp2vg_decoder_handoff_stats",
    "mp2vg_decoder_destroy",
    "mp2vg_export_coefficients", "mp2vg_export_matrix", "mp2vg_export_bytes", "mp2vg_export_slots",
    "mp2vg_export_planes",
    "mp2vg_tensor_weights", "mp2vg_tensor_bytes", "mp2vg_tensor_slots", "mp2vg_tensor_planes",
    "mp2vg_tensor_slots_fields", "mp2vg_tensor_planes_field", "mp2vg_parsed_picture_flags", "mp2vg_scan_picture_flags",
    "mp2vg_tensor_slots_placed", "mp2vg_tensor_planes_placed", "mp2vg_tensor_fit", "mp2vg_stream_pixel_aspect",
    "mp2vg_tensor_items", "mp2vg_tensor_planes_items", "mp2vg_tensor_items_plan",
    "mp2vg_scan_es", "mp2vg_scan_counts", "mp2vg_scan_pictures", "mp2vg_scan_display_order",
    "mp2vg_scan_gop_index", "mp2vg_scan_shards", "mp2vg_scan_stream_headers", "mp2vg_scan_free",
    "mp2vg_scan_parse_host", "mp2vg_batch_upload_es", "mp2vg_batch_record_counts",
    "mp2vg_batch_download_records", "mp2vg_last_parse_times",
    "mp2vg_motion_bytes", "mp2vg_motion_records", "mp2vg_motion_batch", "mp2vg_last_motion_time",
    "mp2vg_residual_bytes", "mp2vg_residual_records", "mp2vg_residual_batch", "mp2vg_last_residual_time",
    "mp2vg_parsed_damage", "mp2vg_last_upload_damage", "mp2vg_damage_reason_string", "mp2vg_decoder_damage_count",
    "mp2vg_probe_es",
]

_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"native library {LIB_PATH} is missing: run `python tiny_mp2v_dec_amd/build.py` "
                           "(there is no CPU fallback for the reconstruct path)")
    L = ctypes.CDLL(LIB_PATH)
    P, I32, U64, VP = ctypes.POINTER, ctypes.c_int32, ctypes.c_uint64, ctypes.c_void_p
    sig = {
        "mp2vg_abi_version": ([], ctypes.c_int),
        "mp2vg_status_string": ([ctypes.c_int], ctypes.c_char_p),
        "mp2vg_last_error": ([], ctypes.c_char_p),
        "mp2vg_create": ([P(Config), P(VP)], ctypes.c_int),
        "mp2vg_destroy": ([VP], ctypes.c_int),
        "mp2vg_frame_geometry": ([P(Config), P(I32), P(I32), P(I32), P(U64)], ctypes.c_int),
        "mp2vg_reserve_slots": ([VP, I32], ctypes.c_int),
        "mp2vg_batch_upload": ([VP, VP, I32, VP, U64, VP, U64], ctypes.c_int),
        "mp2vg_batch_validate": ([P(Config), I32, VP, I32, VP, U64, VP, U64, P(I32), P(I32), P(I32), I32],
                                 ctypes.c_int),
        "mp2vg_batch_plan": ([P(Config), I32, VP, I32, VP, U64, VP, U64, P(Plan)], ctypes.c_int),
        "mp2vg_batch_decode": ([VP], ctypes.c_int),
        "mp2vg_synchronize": ([VP], ctypes.c_int),
        "mp2vg_last_launch_times": ([VP, P(ctypes.c_float), I32, P(I32)], ctypes.c_int),
        "mp2vg_last_batch_time": ([VP, P(ctypes.c_float)], ctypes.c_int),
        "mp2vg_batch_times": ([VP, I32, P(ctypes.c_float), P(ctypes.c_float), I32, P(I32)], ctypes.c_int),
        "mp2vg_batches_span": ([VP, I32, I32, P(ctypes.c_float)], ctypes.c_int),
        "mp2vg_download_slot": ([VP, I32, P(ctypes.c_void_p), P(I32)], ctypes.c_int),
        "mp2vg_copy_slot_packed": ([VP, I32, VP, I32], ctypes.c_int),
        "mp2vg_slot_device_ptr": ([VP, I32, P(VP)], ctypes.c_int),
        "mp2vg_sink_device_ptr": ([VP, P(VP)], ctypes.c_int),
        "mp2vg_clock_probe": ([I32, P(ctypes.c_double)], ctypes.c_int),
        "mp2vg_pool_probe": ([VP, I32, I32, P(ctypes.c_double), I32, P(I32)], ctypes.c_int),
        "mp2vg_pool_placement": ([VP, P(ctypes.c_float), I32, P(I32), P(I32)], ctypes.c_int),
        "mp2vg_cpu_budget": ([], ctypes.c_int),
        "mp2vg_invalidate_slot": ([VP, I32], ctypes.c_int),
        "mp2vg_slot_digests": ([VP, P(I32), I32, P(ctypes.c_uint64)], ctypes.c_int),
        "mp2vg_parse_es": ([VP, U64, P(Config), P(VP)], ctypes.c_int),
        "mp2vg_parsed_counts": ([VP, P(I32), P(U64), P(U64)], ctypes.c_int),
        "mp2vg_parsed_pictures": ([VP], VP),
        "mp2vg_parsed_mbs": ([VP], VP),
        "mp2vg_parsed_coefs": ([VP], VP),
        "mp2vg_parsed_display_order": ([VP, P(I32), I32], ctypes.c_int),
        "mp2vg_parsed_gop_index": ([VP, P(I32), I32], ctypes.c_int),
        "mp2vg_parsed_stream_headers": ([VP, P(StreamHeaders)], ctypes.c_int),
        "mp2vg_parsed_shards": ([VP, P(I32), I32], ctypes.c_int),
        "mp2vg_parsed_free": ([VP], None),
        "mp2vg_vlc_decode": ([I32, U64, P(I32), P(I32), P(I32)], ctypes.c_int),
        "mp2vg_gen_default_params": ([P(GenParams)], None),
        "mp2vg_generate_es": ([P(GenParams), P(VP), P(U64)], ctypes.c_int),
        "mp2vg_free": ([VP], None),
        "mp2vg_decoder_create": ([P(Config), RENDER_FN, VP, P(VP)], ctypes.c_int),
        "mp2vg_decoder_create_multi": ([P(Config), P(I32), I32, RENDER_FN, VP, P(VP)], ctypes.c_int),
        "mp2vg_decoder_decode": ([VP, VP, U64], ctypes.c_int),
        "mp2vg_decoder_stream_headers": ([VP, P(StreamHeaders)], ctypes.c_int),
        "mp2vg_decoder_lane_frames": ([VP, P(I32), I32], ctypes.c_int),
        "mp2vg_decoder_frames_allocated": ([VP], ctypes.c_int),
        "mp2vg_decoder_handoff_stats": ([VP, P(I32), P(I32), P(I32), P(I32)], ctypes.c_int),
        "mp2vg_decoder_destroy": ([VP], ctypes.c_int),
        "mp2vg_export_coefficients": ([I32, P(I32)], ctypes.c_int),
        "mp2vg_export_matrix": ([P(StreamHeaders), P(I32)], ctypes.c_int),
        "mp2vg_export_bytes": ([P(Config), P(Export), I32, P(U64)], ctypes.c_int),
        "mp2vg_export_slots": ([VP, P(I32), I32, P(Export), VP, U64], ctypes.c_int),
        "mp2vg_export_planes": ([I32, P(VP), P(I32), I32, I32, I32, P(Export), VP, U64], ctypes.c_int),
        "mp2vg_tensor_weights": ([I32, I32, P(I32), P(I32), P(I32), I32], ctypes.c_int),
        "mp2vg_tensor_bytes": ([P(Config), P(Tensor), I32, P(U64)], ctypes.c_int),
        "mp2vg_tensor_slots": ([VP, P(I32), I32, P(Tensor), VP, U64], ctypes.c_int),
        "mp2vg_tensor_planes": ([I32, P(VP), P(I32), I32, I32, I32, P(Tensor), VP, U64], ctypes.c_int),
        "mp2vg_tensor_slots_fields": ([VP, P(I32), P(I32), I32, P(Tensor), VP, U64], ctypes.c_int),
        "mp2vg_tensor_planes_field": ([I32, P(VP), P(I32), I32, I32, I32, I32, P(Tensor), VP, U64], ctypes.c_int),
        "mp2vg_tensor_slots_placed": ([VP, P(I32), P(I32), I32, P(Tensor), P(Place), VP, U64], ctypes.c_int),
        "mp2vg_tensor_planes_placed": ([I32, P(VP), P(I32), I32, I32, I32, I32, P(Tensor), P(Place), VP, U64],
                                       ctypes.c_int),
        "mp2vg_tensor_fit": ([I32, P(I32), I32, I32, I32, I32, P(I32), P(I32)], ctypes.c_int),
        "mp2vg_stream_pixel_aspect": ([P(StreamHeaders), P(I32), P(I32)], ctypes.c_int),
        "mp2vg_tensor_items": ([VP, P(Item), I32, P(Tensor), I32, VP, U64], ctypes.c_int),
        "mp2vg_tensor_planes_items": ([I32, P(VP), P(I32), I32, I32, I32, P(Item), I32, P(Tensor), I32, VP, U64],
                                      ctypes.c_int),
        "mp2vg_tensor_items_plan": ([P(Config), P(Tensor), P(Item), I32, I32, P(I32), P(I32), P(I32)], ctypes.c_int),
        "mp2vg_parsed_picture_flags": ([VP, P(ctypes.c_uint32), I32], ctypes.c_int),
        "mp2vg_scan_picture_flags": ([VP, P(ctypes.c_uint32), I32], ctypes.c_int),
        "mp2vg_scan_es": ([VP, U64, P(Config), P(VP)], ctypes.c_int),
        "mp2vg_scan_counts": ([VP, P(I32), P(U64)], ctypes.c_int),
        "mp2vg_scan_pictures": ([VP], VP),
        "mp2vg_scan_display_order": ([VP, P(I32), I32], ctypes.c_int),
        "mp2vg_scan_gop_index": ([VP, P(I32), I32], ctypes.c_int),
        "mp2vg_scan_shards": ([VP, P(I32), I32], ctypes.c_int),
        "mp2vg_scan_stream_headers": ([VP, P(StreamHeaders)], ctypes.c_int),
        "mp2vg_scan_free": ([VP], None),
        "mp2vg_scan_parse_host": ([VP, I32, I32, VP, U64, VP, U64, P(U64), P(U64)], ctypes.c_int),
        "mp2vg_batch_upload_es": ([VP, VP, VP, I32, I32], ctypes.c_int),
        "mp2vg_batch_record_counts": ([VP, P(U64), P(U64)], ctypes.c_int),
        "mp2vg_batch_download_records": ([VP, VP, U64, VP, U64], ctypes.c_int),
        "mp2vg_last_parse_times": ([VP, P(ctypes.c_float)], ctypes.c_int),
        "mp2vg_motion_bytes": ([P(Config), I32, P(U64)], ctypes.c_int),
        "mp2vg_motion_records": ([P(Config), VP, I32, VP, U64, VP, U64, P(I32), I32, VP, VP, VP], ctypes.c_int),
        "mp2vg_motion_batch": ([VP, P(I32), I32, VP, VP, VP, P(U64)], ctypes.c_int),
        "mp2vg_last_motion_time": ([VP, P(ctypes.c_float)], ctypes.c_int),
        "mp2vg_residual_bytes": ([P(Config), I32, I32, P(U64)], ctypes.c_int),
        "mp2vg_residual_records": ([P(Config), VP, I32, VP, U64, VP, U64, P(I32), I32, I32, I32, VP, VP, VP],
                                   ctypes.c_int),
        "mp2vg_residual_batch": ([VP, P(I32), I32, I32, I32, VP, VP, VP, P(U64)], ctypes.c_int),
        "mp2vg_last_residual_time": ([VP, P(ctypes.c_float)], ctypes.c_int),
        "mp2vg_parsed_damage": ([VP, VP, I32, P(I32)], ctypes.c_int),
        "mp2vg_last_upload_damage": ([VP, VP, I32, P(I32)], ctypes.c_int),
        "mp2vg_damage_reason_string": ([I32], ctypes.c_char_p),
        "mp2vg_decoder_damage_count": ([VP], ctypes.c_int),
        "mp2vg_probe_es": ([VP, U64, P(Config), P(StreamHeaders)], ctypes.c_int),
    }
    for name, (args, res) in sig.items():
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = res
    _lib = L
    return L


def check(status, what):
    if status != 0:
        detail = lib().mp2vg_last_error().decode(errors="replace")
        raise Mp2vgError(status, what, detail)
    return status


MP2VG_DECODER_DEVICE_FRAMES, MP2VG_CTX_ONE_STREAM = 1, 2  # mp2vg_config_t.reserved flags
MP2VG_DECODER_DEVICE_PARSE = 4  # drop-in decoder: slices parsed on the device (mp2vg_batch_upload_es)
MP2VG_PARSE_CONCEAL = 8  # parse / scan / drop-in decoder: damaged rows are replaced, not rejected
MP2VG_PARSE_STANDARD = 16  # the same three: default / sequence-header matrices, intra_vlc_format = 0
MP2VG_PARSE_SLICES = 32  # the same three: any number of slices per macroblock row


def parse_flags(conceal=False, standard=False, slices=False):
    """mp2vg_config_t.reserved of a parse or scan."""
    return ((MP2VG_PARSE_CONCEAL if conceal else 0) | (MP2VG_PARSE_STANDARD if standard else 0) |
            (MP2VG_PARSE_SLICES if slices else 0))
RESIDUAL_DTYPES = {"int16": 0, "int8": 1}  # MP2VG_RESIDUAL_I16 / I8
RESIDUAL_ZERO_INTRA = 1


def residual_dtype(dtype):
    """MP2VG_RESIDUAL_* code of 'int16' / 'int8' (or of a numpy / torch dtype of that name)."""
    name = str(dtype).replace("torch.", "")
    if name not in RESIDUAL_DTYPES:
        raise ValueError(f"residual dtype {dtype!r}: expected 'int16' or 'int8'")
    return name, RESIDUAL_DTYPES[name]


def residual_shapes(width, height, chroma_format, n):
    """Shapes of the y, cb and cr planes of n pictures."""
    cw = width if chroma_format == 3 else width // 2
    ch = height // 2 if chroma_format == 1 else height
    return (n, height, width), (n, ch, cw), (n, ch, cw)


def make_config(width, height, chroma_format, pool=10, threads=0, reordering=True, device=0, flags=0):
    return Config(width, height, chroma_format, pool, threads, 1 if reordering else 0, device, flags)


def make_export(layout="nchw", chroma="linear", matrix=1, size=None):
    """mp2vg_export_t from the Python spelling: layout "nchw" (planar) / "nhwc" (packed), chroma
    "linear" / "nearest", matrix = a matrix_coefficients code, size = (width, height) or None for
    the coded size."""
    layouts = {"nchw": EXPORT_RGB_PLANAR, "nhwc": EXPORT_RGB_PACKED}
    modes = {"nearest": EXPORT_CHROMA_NEAREST, "linear": EXPORT_CHROMA_LINEAR}
    if layout not in layouts:
        raise ValueError(f"layout {layout!r}: expected 'nchw' or 'nhwc'")
    if chroma not in modes:
        raise ValueError(f"chroma {chroma!r}: expected 'linear' or 'nearest'")
    w, h = (0, 0) if size is None else (int(size[0]), int(size[1]))
    return Export(layouts[layout], int(matrix), modes[chroma], w, h, (ctypes.c_int32 * 3)())


def export_shape(exp, n, coded_w, coded_h):
    """Tensor shape of n frames exported with `exp` from coded_w x coded_h frames."""
    w, h = exp.width or coded_w, exp.height or coded_h
    return (n, 3, h, w) if exp.layout == EXPORT_RGB_PLANAR else (n, h, w, 3)


def export_out(out, shape, device):
    """The tensor an export writes: `out` after checking device, dtype, shape and contiguity, or
    a new torch.uint8 tensor on cuda:<device>.  torch is imported here, not with the package."""
    import torch
    dev = torch.device("cuda", device)
    if out is None:
        return torch.empty(shape, dtype=torch.uint8, device=dev)
    if not isinstance(out, torch.Tensor) or out.device != dev or out.dtype != torch.uint8:
        raise ValueError(f"out must be a torch.uint8 tensor on {dev}")
    if tuple(out.shape) != tuple(shape) or not out.is_contiguous():
        raise ValueError(f"out must be contiguous with shape {tuple(shape)}, got {tuple(out.shape)}")
    return out


def tensor_dtype_name(dtype):
    """"uint8" / "float16" / "bfloat16" / "float32" from that name or the torch dtype."""
    name = str(dtype).replace("torch.", "")
    if name not in TENSOR_DTYPES:
        raise ValueError(f"dtype {dtype!r}: expected uint8, float16, bfloat16 or float32")
    return name


def make_tensor(size, crop=None, dtype="float16", mean=None, std=None, layout="nchw", chroma="linear", matrix=1):
    """mp2vg_tensor_t from the Python spelling: size = (out_w, out_h); crop = (x, y, w, h) in luma
    pixels or None for the coded frame; dtype a name or torch dtype; mean / std per channel in 0..1
    units (both or neither): scale = float32(1 / (255 std)), bias = float32(-mean / std), computed
    in float64 and rounded once; without them scale 1 / 255 and bias 0 (uint8: 1 and 0, and mean /
    std are refused); layout, chroma, matrix as make_export."""
    e = make_export(layout, chroma, matrix)
    name = tensor_dtype_name(dtype)
    if (mean is None) != (std is None):
        raise ValueError("mean and std go together")
    if name == "uint8":
        if mean is not None:
            raise ValueError("uint8 output takes no mean / std")
        scale, bias = [1.0] * 3, [0.0] * 3
    elif mean is None:
        scale, bias = [1.0 / 255.0] * 3, [0.0] * 3
    else:
        mean, std = [float(v) for v in mean], [float(v) for v in std]
        if len(mean) != 3 or len(std) != 3:
            raise ValueError("mean and std have one entry per channel")
        scale, bias = [1.0 / (255.0 * s) for s in std], [-m / s for m, s in zip(mean, std)]
    x, y, w, h = (0, 0, 0, 0) if crop is None else (int(v) for v in crop)
    return Tensor(e.layout, e.matrix, e.chroma, x, y, w, h, int(size[0]), int(size[1]), TENSOR_DTYPES[name][0],
                  (ctypes.c_float * 3)(*scale), (ctypes.c_float * 3)(*bias), (ctypes.c_int32 * 4)())


def make_place(rect, pad=(0, 0, 0)):
    """mp2vg_tensor_place_t: rect = (x, y, w, h) of the picture inside the output, pad = the 8-bit
    (R, G, B) of every element outside it."""
    x, y, w, h = (int(v) for v in rect)
    pad = [int(v) for v in pad]
    if len(pad) != 3 or any(v < 0 or v > 255 for v in pad):
        raise ValueError(f"pad {pad!r}: expected three values 0..255 (R, G, B)")
    return Place(x, y, w, h, (ctypes.c_uint8 * 3)(*pad), 0, (ctypes.c_int32 * 3)())


def tensor_fit(mode, src, par, size):
    """(src_out, dst_out) of mp2vg_tensor_fit: mode "stretch" / "contain" / "cover" (or MP2VG_FIT_*),
    src = (x, y, w, h) the source rectangle, par = (n, d) the pixel's width : height, size =
    (out_w, out_h).  src_out is the crop to export, dst_out the picture's rectangle in the output."""
    if isinstance(mode, str):
        if mode not in FITS:
            raise ValueError(f"fit {mode!r}: expected 'stretch', 'contain' or 'cover'")
        mode = FITS[mode]
    s, so, do = (ctypes.c_int32 * 4)(*[int(v) for v in src]), (ctypes.c_int32 * 4)(), (ctypes.c_int32 * 4)()
    check(lib().mp2vg_tensor_fit(int(mode), s, int(par[0]), int(par[1]), int(size[0]), int(size[1]), so, do),
          "tensor_fit")
    return tuple(so), tuple(do)


def placement(size, crop, coded, place=None, fit=None, pixel_aspect=(1, 1), pad=(0, 0, 0)):
    """(crop, Place or None) of an export's place / fit / pixel_aspect / pad arguments: `place` is
    the picture's rectangle in the output; `fit` computes it (and, for "cover", the crop) from the
    shape crop (None: the coded frame, coded = (w, h)) is shown at with pixels of pixel_aspect.
    Neither: (crop, None), the export without a placement."""
    if place is not None and fit is not None:
        raise ValueError("place and fit exclude each other")
    if fit is not None:
        src = (0, 0, int(coded[0]), int(coded[1])) if crop is None else tuple(int(v) for v in crop)
        crop, place = tensor_fit(fit, src, pixel_aspect, size)
    return crop, None if place is None else make_place(place, pad)


def field_mode(field):
    """MP2VG_FIELD_* from "progressive" / "top" / "bottom" / "weave" or the integer itself."""
    if isinstance(field, str):
        if field not in FIELDS:
            raise ValueError(f"field {field!r}: expected 'progressive', 'top', 'bottom' or 'weave'")
        return FIELDS[field]
    if int(field) not in FIELDS.values():
        raise ValueError(f"field {field!r}: expected 0..3 (MP2VG_FIELD_*)")
    return int(field)


def field_modes(fields, n):
    """The int32 field list of n frames from None (no list: all progressive), one mode for every
    frame, or a sequence of n modes (names or integers)."""
    if fields is None:
        return None
    if isinstance(fields, (str, int, np.integer)):
        return np.full(n, field_mode(fields), np.int32)
    out = np.array([field_mode(f) for f in fields], np.int32)
    if len(out) != n:
        raise ValueError("fields must hold one mode per slot")
    return out


def make_items(slots, crops, flips=None, fields=None, n=None):
    """(mp2vg_tensor_item_t * n) from the Python spelling.  slots: None (every item slot 0, the
    planes call), one slot for every item or n slots; crops: None (every item the whole coded frame)
    or n entries, each (x, y, w, h) in luma pixels or None; flips: None, one bool for every item or
    n of them (True: MP2VG_ITEM_HFLIP); fields as field_modes.  n defaults to the length of crops,
    else of slots."""
    if n is None:
        n = len(crops) if crops is not None else len(slots)
    n = int(n)

    def per_item(v, what, scalar):
        if v is None or isinstance(v, scalar):
            return [v] * n
        if len(v) != n:
            raise ValueError(f"{what} must hold one entry per item ({n})")
        return list(v)

    slots = per_item(slots, "slots", (int, np.integer))
    flips = per_item(flips, "flips", (bool, np.bool_))
    modes = field_modes(fields, n)
    if crops is not None and len(crops) != n:
        raise ValueError(f"crops must hold one entry per item ({n})")
    items = (Item * n)()
    for i in range(n):
        x, y, w, h = (0, 0, 0, 0) if crops is None or crops[i] is None else (int(v) for v in crops[i])
        items[i] = Item(int(slots[i] or 0), 0 if modes is None else int(modes[i]), x, y, w, h,
                        ITEM_HFLIP if flips[i] else 0, 0)
    return items


def items_shape(t, n, clip_len):
    """Shape of an items launch: (n, h, w, 3) packed; planar (n, 3, h, w), or (n / T, 3, T, h, w) in
    clip order for clip_len = T > 1."""
    if t.layout != EXPORT_RGB_PLANAR or clip_len == 1:
        return tensor_shape(t, n)
    if clip_len < 1 or n % clip_len:
        raise ValueError(f"clip_len {clip_len} must be at least 1 and divide the number of items ({n})")
    return (n // clip_len, 3, clip_len, t.out_h, t.out_w)


def tensor_shape(t, n):
    return (n, 3, t.out_h, t.out_w) if t.layout == EXPORT_RGB_PLANAR else (n, t.out_h, t.out_w, 3)


def tensor_out(out, shape, dtype, device):
    """The tensor a tensor export writes: `out` after checking device, dtype, shape and contiguity,
    or a new tensor of that dtype on cuda:<device>."""
    import torch
    dev, want = torch.device("cuda", device), getattr(torch, tensor_dtype_name(dtype))
    if out is None:
        return torch.empty(shape, dtype=want, device=dev)
    if not isinstance(out, torch.Tensor) or out.device != dev or out.dtype != want:
        raise ValueError(f"out must be a {want} tensor on {dev}")
    if tuple(out.shape) != tuple(shape) or not out.is_contiguous():
        raise ValueError(f"out must be contiguous with shape {tuple(shape)}, got {tuple(out.shape)}")
    return out


def tensor_weights(src, out):
    """(first, count, weights[out][max count]) of one axis (mp2vg_tensor_weights)."""
    first, count = np.zeros(out, np.int32), np.zeros(out, np.int32)
    w = np.zeros((out, TENSOR_MAX_TAPS), np.int32)
    i32p = ctypes.POINTER(ctypes.c_int32)
    check(lib().mp2vg_tensor_weights(src, out, first.ctypes.data_as(i32p), count.ctypes.data_as(i32p),
                                     w.ctypes.data_as(i32p), TENSOR_MAX_TAPS), "tensor_weights")
    return first, count, w[:, :int(count.max())]


def geometry(width, height, chroma_format):
    c = make_config(width, height, chroma_format)
    w, h, s = (ctypes.c_int32 * 3)(), (ctypes.c_int32 * 3)(), (ctypes.c_int32 * 3)()
    sb = ctypes.c_uint64()
    check(lib().mp2vg_frame_geometry(ctypes.byref(c), w, h, s, ctypes.byref(sb)), "frame_geometry")
    return list(w), list(h), list(s), sb.value
