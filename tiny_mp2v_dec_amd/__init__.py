"""tiny_mp2v_dec_amd — MI355X-native MPEG-2 macroblock reconstruct path.

Host record emitter + HIP/CDNA4 kernels behind the C ABI of include/mp2vg.h, with the
reference's decoder API (mp2v_decoder_c / frame_c / decoder_config_t) mirrored in decoder.py.
"""
from ._lib import MB_DTYPE, PIC_DTYPE, Mp2vgError, lib  # noqa: F401
from .records import (DeviceContext, Parsed, decode_motion, decode_residual, decode_rgb, decode_tensor,  # noqa: F401
                      generate_es, motion_host, reference_pictures, residual_bytes, residual_host)

__all__ = ["DeviceContext", "Parsed", "decode_motion", "decode_residual", "decode_rgb", "decode_tensor", "generate_es",
           "motion_host", "reference_pictures", "residual_bytes", "residual_host", "MB_DTYPE", "PIC_DTYPE",
           "Mp2vgError", "lib"]
