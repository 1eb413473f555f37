"""CPU: the C-ABI library loads, exports exactly what include/*.h declares, and fails loudly (no
CPU fallback) when device work is requested without a GPU."""
import ctypes
import os
import re
import subprocess

import pytest

from tiny_mp2v_dec_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_functions():
    text = open(os.path.join(REPO, "include", "mp2vg.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mp2vg_[a-z_0-9]+)\s*\(", text)) - {"mp2vg_mb", "mp2vg_picture"})


def test_header_and_binding_agree():
    assert declared_functions() == sorted(_lib.EXPORTS)


def test_every_declared_symbol_exported():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared_functions():
        assert hasattr(lib, name), name
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (mp2vg_\w+)", out))
    assert set(declared_functions()) <= exported


def test_library_is_gfx950_code_object():
    """The embedded HIP fat binary carries a gfx950 code object (and no other target)."""
    blob = open(_lib.LIB_PATH, "rb").read()
    targets = set(re.findall(rb"amdgcn-amd-amdhsa--(gfx[0-9a-f]+)", blob))
    assert targets == {b"gfx950"}


def test_abi_version_and_status_strings():
    L = _lib.lib()
    assert L.mp2vg_abi_version() == 2  # 2: coefficient-word bit layout of round 2
    for s in (0, -1, -2, -3, -4, -5, -6):
        assert L.mp2vg_status_string(s)


def test_struct_layouts():
    assert _lib.MB_DTYPE.itemsize == 32
    assert _lib.PIC_DTYPE.itemsize == 288
    assert ctypes.sizeof(_lib.Config) == 32


def test_frame_geometry_matches_reference_frame_c():
    """frame_c (reference decoder.cpp:44-68): stride = round_up(w, 64); chroma = round_up(stride/2, 64)"""
    w, h, s, slot = _lib.geometry(1920, 1088, 1)
    assert (w, h, s) == ([1920, 960, 960], [1088, 544, 544], [1920, 960, 960])
    assert slot == 1920 * 1088 + 2 * 960 * 544
    w, h, s, _ = _lib.geometry(176, 144, 2)
    assert (w, h, s) == ([176, 88, 88], [144, 144, 144], [192, 128, 128])
    w, h, s, _ = _lib.geometry(3840, 2160 + 16 - 2160 % 16, 3)
    assert s == [3840, 3840, 3840]
    with pytest.raises(_lib.Mp2vgError):
        _lib.geometry(100, 64, 1)


def _host_entry_points(w, h, cf, es, pics, mbs, coefs):
    """Every entry point that takes a config and needs no device, as (name, call) on a w x h
    config.  The calls raise Mp2vgError when the library refuses."""
    import numpy as np

    from tiny_mp2v_dec_amd import records as R

    def raw_bytes(fn, desc):
        cfg, out = _lib.make_config(w, h, cf), ctypes.c_uint64()
        _lib.check(getattr(_lib.lib(), fn)(ctypes.byref(cfg), ctypes.byref(desc), 1, ctypes.byref(out)), fn)
        return out.value

    one = np.zeros(1, np.int32)
    # a tensor export of the far corner (the resize ratio is limited to 32:1)
    if w > h:
        size, crop = (224, 8), (max(w - 448, 0), 0, min(w, 448), 16)
    else:
        size, crop = (8, 224), (0, max(h - 448, 0), 16, min(h, 448))
    return [
        ("mp2vg_frame_geometry", lambda: _lib.geometry(w, h, cf)),
        ("mp2vg_parse_es", lambda: R.Parsed(es, w, h, cf)),
        ("mp2vg_scan_es", lambda: R.Scan(es, w, h, cf).close()),
        ("mp2vg_batch_validate", lambda: R.plan_batch(w, h, cf, len(pics), pics, mbs, coefs)),
        ("mp2vg_batch_plan", lambda: R.plan_dump(w, h, cf, len(pics), pics, mbs, coefs)),
        ("mp2vg_export_bytes", lambda: raw_bytes("mp2vg_export_bytes", _lib.make_export())),
        ("mp2vg_tensor_bytes", lambda: raw_bytes("mp2vg_tensor_bytes", _lib.make_tensor(size, crop))),
        ("mp2vg_tensor_items_plan",
         lambda: R.items_plan(w, h, cf, size, [crop])),
        ("mp2vg_motion_bytes", lambda: R.motion_bytes(w, h, cf, 1)),
        ("mp2vg_motion_records", lambda: R.motion_host(pics, mbs, coefs, w, h, cf, order=one)),
        ("mp2vg_residual_bytes", lambda: R.residual_bytes(w, h, cf, 1)),
        ("mp2vg_residual_records", lambda: R.residual_host(pics, mbs, coefs, w, h, cf, order=one)),
    ]


def _i_picture(w, h, cf):
    from tiny_mp2v_dec_amd import records as R
    es = R.generate_es(width=w, height=h, chroma_format=cf, n_gops=1, gop_n=1, gop_m=1, seed=16384 + cf)
    p = R.Parsed(es, w, h, cf)
    return es, p.pics, p.mbs, p.coefs


def test_geometry_limit_slot_sizes():
    """MP2VG_MAX_DIMENSION: 16384 is accepted in either dimension and in both, with the slot size
    the frame_c formula gives; the header's constant is the one the library applies."""
    text = open(os.path.join(REPO, "include", "mp2vg.h")).read()
    assert re.search(r"#define\s+MP2VG_MAX_DIMENSION\s+16384\b", text)
    for cf, chroma in ((1, 0.5), (2, 1.0), (3, 2.0)):
        for w, h in ((16384, 16), (16, 16384), (16384, 16384)):
            pw, ph, st, slot = _lib.geometry(w, h, cf)
            s0 = (w + 63) & ~63
            s1 = s0 if cf == 3 else ((s0 >> 1) + 63) & ~63
            assert st == [s0, s1, s1]
            assert slot == s0 * h + 2 * s1 * (h // 2 if cf == 1 else h)
            if w == h:
                assert slot == int(16384 * 16384 * (1 + chroma))
    assert _lib.geometry(16384, 16384, 3)[3] == 805306368


@pytest.mark.parametrize("size", [(16384, 16), (16, 16384)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("cf", [1, 2, 3])
def test_geometry_limit_accepted_by_every_host_entry_point(size, cf):
    """A 1024-MB row and 1024 one-MB rows (one I picture from the stream writer) pass every host-only
    entry point that takes a config."""
    w, h = size
    es, pics, mbs, coefs = _i_picture(w, h, cf)
    assert (int(pics[0]["mb_width"]), int(pics[0]["mb_height"]), len(mbs)) == (w // 16, h // 16, 1024)
    for name, call in _host_entry_points(w, h, cf, es, pics, mbs, coefs):
        call()


@pytest.mark.parametrize("size", [(16400, 16), (16, 16400), (1 << 20, 16), (16, 1 << 20), (1 << 20, 1 << 20)],
                         ids=lambda s: "%dx%d" % s)
def test_geometry_above_the_limit_refused_by_every_host_entry_point(size):
    """16400 and 1 << 20 in either dimension: MP2VG_E_INVALID with a message that names the limit,
    from every host-only entry point that takes a config, before any record or stream byte is read
    (the records and the stream are those of a 16 x 16 picture)."""
    w, h = size
    es, pics, mbs, coefs = _i_picture(16, 16, 1)
    for name, call in _host_entry_points(w, h, 1, es, pics, mbs, coefs):
        if name in ("mp2vg_motion_records", "mp2vg_residual_records") and w * h > 1 << 26:
            continue  # the wrapper would allocate the output planes of the refused size first
        with pytest.raises(_lib.Mp2vgError, match="16384") as e:
            call()
        assert e.value.status == -1, name  # MP2VG_E_INVALID


def test_stream_writer_sizes():
    """The stream writer reaches 16384 in either dimension and refuses what no stream can carry: a
    size above 16384, and a height above 2800 that the reference's slice-extension rule (the 12-bit
    vertical_size_value above 2800) cannot address."""
    from tiny_mp2v_dec_amd import records as R
    for w, h in ((16400, 16), (16, 16400), (16, 4112), (16, 6896), (16, 8208)):
        with pytest.raises(_lib.Mp2vgError) as e:
            R.generate_es(width=w, height=h, chroma_format=1, n_gops=1, gop_n=1, gop_m=1)
        assert e.value.status == -1, (w, h)
    for w, h, hs, vs in ((16384, 16, 16383, 16), (16368, 32, 16368, 32), (16, 16384, 16, 16383), (32, 8192, 32, 8191),
                         (16, 2816, 16, 2816), (4096, 16, 4095, 16), (16, 6912, 16, 6912)):
        es = R.generate_es(width=w, height=h, chroma_format=1, n_gops=1, gop_n=1, gop_m=1)
        hd = R.Parsed(es, w, h, 1).headers
        assert (hd.sequence_header.horizontal_size_value | hd.sequence_extension.horizontal_size_extension << 12,
                hd.sequence_header.vertical_size_value | hd.sequence_extension.vertical_size_extension << 12) == (hs, vs)


def test_invalid_arguments_rejected():
    L = _lib.lib()
    assert L.mp2vg_create(None, None) == -1
    assert L.mp2vg_batch_decode(None) == -1
    assert L.mp2vg_destroy(None) == -1
    n = ctypes.c_int32()
    assert L.mp2vg_pool_probe(None, 1, 1, None, 0, ctypes.byref(n)) == -1
    assert L.mp2vg_clock_probe(0, None) == -1
    assert L.mp2vg_sink_device_ptr(None, None) == -1


def test_no_silent_cpu_fallback_without_gpu():
    """Without a device the context cannot be created: the product path has no CPU fallback."""
    try:
        import torch
        if torch.cuda.is_available():
            pytest.skip("a GPU is present")
    except ImportError:
        pass
    cfg = _lib.make_config(176, 144, 1)
    h = ctypes.c_void_p()
    rc = _lib.lib().mp2vg_create(ctypes.byref(cfg), ctypes.byref(h))
    assert rc == -3  # MP2VG_E_HIP


def test_cpu_budget_within_the_process_cpus():
    """mp2vg_cpu_budget (the decoder's default thread count): at least 1, at most the CPUs this
    process may run on, and at most a cgroup v2 cpu.max quota when one is set."""
    import os
    n = _lib.lib().mp2vg_cpu_budget()
    assert 1 <= n <= len(os.sched_getaffinity(0))
    try:
        q, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            assert n <= max(1, int(q) // int(period))
    except (OSError, ValueError):
        pass
