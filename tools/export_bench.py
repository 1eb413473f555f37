#!/usr/bin/env python3
"""Speed of the RGB export (mp2vg_export_slots) at 1080p 4:2:0 against a device-to-device copy of
the same traffic, measured in one process.

256 slots are filled by a generated 1920 x 1088 stream and exported to 1920 x 1080, both layouts x
both chroma modes.  Each repetition is a host clock around export_slots + mp2vg_synchronize; it
alternates with a hipMemcpyAsync of (bytes read + bytes written) / 2 bytes, which moves the same
HBM traffic.  Bytes are algorithmic: 1.5 B read and 3 B written per exported pixel.  The kernel's
static VALU instructions per pixel are counted from the gfx950 ISA of export.hip (a thread makes 4
pixels).  Writes export.json and README.md into --out.

    python tools/export_bench.py --out profiles/export        # on an MI355X
    python tools/export_bench.py --isa-only                   # the ISA counts alone, no GPU
"""
import argparse
import ctypes
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

W, H, CODED_H, CF, SLOTS = 1920, 1080, 1088, 1, 256
PIXELS_PER_THREAD = 4
VARIANTS = [(layout, chroma) for layout in ("nchw", "nhwc") for chroma in ("nearest", "linear")]


def isa_counts():
    """Static instruction counts of each 4:2:0 kernel variant: {(layout, chroma): {class: n}}."""
    from tiny_mp2v_dec_amd import build as B
    csrc = os.path.join(REPO, "tiny_mp2v_dec_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "export.s")
        subprocess.check_call([B._hipcc(), "-x", "hip", f"--offload-arch={B.ARCH}", "-O3", "-std=c++17", "-I", csrc,
                               "-I", os.path.join(REPO, "include"), "--offload-device-only", "-S", os.path.join(csrc, "export.hip"), "-o", asm],
                              stderr=subprocess.DEVNULL)
        text = open(asm).read()
    out = {}
    for layout, chroma in VARIANTS:
        name = f"export_kernelILi{CF}ELb{int(layout == 'nhwc')}ELb{int(chroma == 'linear')}E"
        m = re.search(r"^(_ZN\w*%s\w*):[^\n]*\n(.*?)^\.Lfunc_end" % name, text, re.S | re.M)
        if not m:
            raise RuntimeError(f"kernel {name} not found in the ISA")
        ops = re.findall(r"^\s+([a-z][a-z0-9_]+)\b", m.group(2), re.M)
        cls = {"valu": 0, "salu": 0, "vmem_load": 0, "vmem_store": 0, "other": 0}
        for op in ops:
            if op.startswith("v_"):
                cls["valu"] += 1
            elif op.startswith("s_") and not op.startswith(("s_load", "s_waitcnt", "s_nop", "s_cbranch", "s_branch")):
                cls["salu"] += 1
            elif op.startswith(("global_load", "flat_load", "buffer_load")):
                cls["vmem_load"] += 1
            elif op.startswith(("global_store", "flat_store", "buffer_store")):
                cls["vmem_store"] += 1
            else:
                cls["other"] += 1
        cls["valu_per_pixel"] = round(cls["valu"] / PIXELS_PER_THREAD, 2)
        out[(layout, chroma)] = cls
    return out


def measure(reps, warmup):
    import torch
    from tiny_mp2v_dec_amd import records as R
    from tiny_mp2v_dec_amd.decoder import _hip_lib
    es = R.generate_es(width=W, height=CODED_H, chroma_format=CF, n_gops=SLOTS // 16, gop_n=16, gop_m=4, seed=5)
    parsed = R.Parsed(es, W, CODED_H, CF)
    assert parsed.npics == SLOTS
    read_b = SLOTS * (W * H + 2 * (W // 2) * (H // 2))
    write_b = SLOTS * 3 * W * H
    copy_b = (read_b + write_b) // 2
    hip = _hip_lib()
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    hip.hipStreamSynchronize.argtypes = [ctypes.c_void_p]
    src = torch.randint(0, 256, (copy_b,), dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)

    def copy_once():
        t0 = time.perf_counter()
        if hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), copy_b, 3, None) or hip.hipStreamSynchronize(None):
            raise RuntimeError("device-to-device copy failed")
        return time.perf_counter() - t0

    slots = parsed.display
    rows = []
    with R.DeviceContext(W, CODED_H, CF, slots=SLOTS) as ctx:
        ctx.upload(parsed.pics, parsed.mbs, parsed.coefs)
        ctx.decode()
        ctx.synchronize()
        for layout, chroma in VARIANTS:
            out = torch.empty((SLOTS, 3, H, W) if layout == "nchw" else (SLOTS, H, W, 3), dtype=torch.uint8,
                              device="cuda")

            def export_once():
                t0 = time.perf_counter()
                ctx.export_rgb(slots, out=out, layout=layout, chroma=chroma, matrix=1, size=(W, H), sync=True)
                return time.perf_counter() - t0

            for _ in range(warmup):
                export_once()
                copy_once()
            te, tc = [], []
            for _ in range(reps):
                te.append(export_once())
                tc.append(copy_once())
            e_ms, c_ms = statistics.median(te) * 1e3, statistics.median(tc) * 1e3
            rows.append({"layout": layout, "chroma": chroma, "frames": SLOTS, "width": W, "height": H,
                         "reps": reps, "export_ms": round(e_ms, 4), "export_ms_min": round(min(te) * 1e3, 4),
                         "export_ms_max": round(max(te) * 1e3, 4),
                         "bytes_read": read_b, "bytes_written": write_b,
                         "export_tbps": round((read_b + write_b) / (e_ms * 1e9), 3),
                         "copy_bytes": copy_b, "copy_ms": round(c_ms, 4),
                         "copy_tbps": round(2 * copy_b / (c_ms * 1e9), 3),
                         "export_rate_over_copy_rate": round(c_ms / e_ms, 3),
                         "frames_per_s": round(SLOTS / (e_ms * 1e-3))})
            del out
    return rows


def write_readme(path, rows, isa, device):
    lines = ["# RGB export: measured speed", "",
             "Written by `tools/export_bench.py`.  1080p 4:2:0, 256 slots filled by a generated stream,",
             "exported to 1920 x 1080 in one `mp2vg_export_slots` call; host clock around the call plus",
             "`mp2vg_synchronize`, median of the repetitions, alternated in the same process with a",
             "device-to-device `hipMemcpyAsync` of (bytes read + bytes written) / 2 bytes (the same HBM",
             "traffic).  TB/s counts algorithmic bytes: 1.5 B read and 3 B written per pixel; the copy's",
             "TB/s counts its bytes read plus written.  VALU per pixel is the kernel's static VALU",
             "instruction count in the gfx950 ISA over the 4 pixels a thread makes (head / tail byte-store",
             "paths included, so it is an upper bound for an interior unit).", ""]
    if rows:
        lines += [f"Device: {device}.", "",
                  "| layout | chroma | export ms | export TB/s | copy ms | copy TB/s | export / copy rate | frames/s | VALU / pixel |",
                  "|---|---|---|---|---|---|---|---|---|"]
        for r in rows:
            k = isa[(r["layout"], r["chroma"])]
            lines.append(f"| {r['layout']} | {r['chroma']} | {r['export_ms']:.3f} | {r['export_tbps']:.2f} | "
                         f"{r['copy_ms']:.3f} | {r['copy_tbps']:.2f} | {r['export_rate_over_copy_rate']:.2f} | "
                         f"{r['frames_per_s']} | {k['valu_per_pixel']} |")
        slow = [r for r in rows if r["export_rate_over_copy_rate"] < 0.5]
        lines.append("")
        if slow:
            lines.append("Below half the copy's rate: " + ", ".join(f"{r['layout']}/{r['chroma']}" for r in slow) +
                         ".  Static instruction classes of those kernels (per thread = 4 pixels):")
            for r in slow:
                k = isa[(r["layout"], r["chroma"])]
                lines.append(f"- {r['layout']}/{r['chroma']}: VALU {k['valu']}, SALU {k['salu']}, loads "
                             f"{k['vmem_load']}, stores {k['vmem_store']}")
            lines += ["", "About 22 VALU lane-ops per pixel fit under the HBM peak and 28 under a copy's rate",
                      "(256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz against 4.5 B per pixel), so the ISA count blames",
                      "the VALU class: beside the matrix itself, the clamp and shift of every unaligned source",
                      "load, the 64-bit row addresses, and the med3 + shift + or byte pack."]
        else:
            lines.append("Every variant runs at half the copy's rate or better.")
    else:
        lines += ["Not measured (no GPU in this run).  Static instruction counts only:", ""]
        for (layout, chroma), k in isa.items():
            lines.append(f"- {layout}/{chroma}: VALU {k['valu']} per thread = {k['valu_per_pixel']} per pixel, "
                         f"loads {k['vmem_load']}, stores {k['vmem_store']}")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "export"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--isa-only", action="store_true")
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    isa = isa_counts()
    rows, device = [], None
    if not a.isa_only:
        import torch
        if not torch.cuda.is_available():
            sys.exit("export_bench: no GPU (a measurement does not fall back; --isa-only counts instructions)")
        device = torch.cuda.get_device_name(0)
        rows = measure(a.reps, a.warmup)
    os.makedirs(a.out, exist_ok=True)
    doc = {"device": device, "rows": rows,
           "isa": [{"layout": k[0], "chroma": k[1], **v} for k, v in isa.items()]}
    with open(os.path.join(a.out, "export.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    write_readme(os.path.join(a.out, "README.md"), rows, isa, device)
    for r in rows:
        print(json.dumps(r))
    for k, v in isa.items():
        print(json.dumps({"layout": k[0], "chroma": k[1], **v}))


if __name__ == "__main__":
    main()
