#!/usr/bin/env python3
"""Speed of the fused tensor export (mp2vg_tensor_slots) at 1080p 4:2:0 against the unfused path
and against a device copy of the source bytes, measured in one process.

256 slots are filled by a generated 1920 x 1088 stream; the visible 1920 x 1080 of each is exported
to 224 x 224 and to 640 x 360 float16 NCHW, LINEAR chroma, ImageNet mean / std.  Each repetition is
a host clock around work that ends in a device synchronise, and the three candidates alternate:

    fused     DeviceContext.export_tensor (one kernel launch)
    unfused   DeviceContext.export_rgb, then torch on the same device: float(), interpolate(
              mode="bilinear", antialias=True), (x / 255 - mean) / std, half()
    copy      hipMemcpyAsync, device to device, of the source bytes (1.5 B per source pixel): the
              read-once floor

The two results are compared (they are not equal to the bit: torch filters in float32 with its
own weights; the largest difference is reported in 8-bit steps).  The kernel's static VALU / SALU /
LDS / memory instruction counts, VGPRs and LDS bytes are read from the gfx950 ISA of tensor.hip.
Writes tensor.json and tensor.md into --out.

    python tools/tensor_bench.py --out profiles/export        # on an MI355X
    python tools/tensor_bench.py --isa-only                   # the ISA figures alone, no GPU
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
SIZES = [(224, 224), (640, 360)]
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
KERNEL = "tensor_kernelILi1ELb1ELb0ELi1EE"  # 4:2:0, LINEAR, planar, F16


def isa_figures():
    """Static figures of the measured kernel variant from the gfx950 ISA."""
    from tiny_mp2v_dec_amd import build as B
    csrc = os.path.join(REPO, "tiny_mp2v_dec_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "tensor.s")
        subprocess.check_call([B._hipcc(), "-x", "hip", f"--offload-arch={B.ARCH}", "-O3", "-std=c++17", "-I", csrc,
                               "-I", os.path.join(REPO, "include"), "--offload-device-only", "-S",
                               os.path.join(csrc, "tensor.hip"), "-o", asm], stderr=subprocess.DEVNULL)
        text = open(asm).read()
    m = re.search(r"^(_ZN\w*%s\w*):[^\n]*\n(.*?)^\.Lfunc_end" % KERNEL, text, re.S | re.M)
    if not m:
        raise RuntimeError(f"kernel {KERNEL} not found in the ISA")
    name, body = m.group(1), m.group(2)
    cls = {"valu": 0, "salu": 0, "lds": 0, "vmem_load": 0, "vmem_store": 0, "other": 0}
    for op in re.findall(r"^\s+([a-z][a-z0-9_]+)\b", body, re.M):
        if op.startswith("v_"):
            cls["valu"] += 1
        elif op.startswith("s_") and not op.startswith(("s_load", "s_waitcnt", "s_nop", "s_cbranch", "s_branch")):
            cls["salu"] += 1
        elif op.startswith("ds_"):
            cls["lds"] += 1
        elif op.startswith(("global_load", "flat_load", "buffer_load")):
            cls["vmem_load"] += 1
        elif op.startswith(("global_store", "flat_store", "buffer_store")):
            cls["vmem_store"] += 1
        else:
            cls["other"] += 1
    meta = re.search(r"\.name:\s+%s\n(?:(?!\.name:).)*?\n\s+\.vgpr_count:\s+(\d+)" % re.escape(name), text, re.S)
    block = text[text.index(f".amdhsa_kernel {name}"):]
    block = block[:block.index(".end_amdhsa_kernel")]
    num = lambda key: int(re.search(r"\.amdhsa_%s\s+(\d+)" % key, block).group(1))  # noqa: E731
    cls.update({"kernel": name, "vgprs": int(meta.group(1)) if meta else num("next_free_vgpr"),
                "lds_bytes": num("group_segment_fixed_size"), "scratch_bytes": num("private_segment_fixed_size")})
    return cls


def measure(reps, warmup):
    import torch
    from tiny_mp2v_dec_amd import records as R
    from tiny_mp2v_dec_amd.decoder import _hip_lib
    es = R.generate_es(width=W, height=CODED_H, chroma_format=CF, n_gops=SLOTS // 16, gop_n=16, gop_m=4, seed=5)
    parsed = R.Parsed(es, W, CODED_H, CF)
    assert parsed.npics == SLOTS
    src_b = SLOTS * (W * H + 2 * (W // 2) * (H // 2))
    hip = _hip_lib()
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    hip.hipStreamSynchronize.argtypes = [ctypes.c_void_p]
    csrc = torch.randint(0, 256, (src_b,), dtype=torch.uint8, device="cuda")
    cdst = torch.empty_like(csrc)
    mean = torch.tensor(MEAN, device="cuda").view(1, 3, 1, 1)
    std = torch.tensor(STD, device="cuda").view(1, 3, 1, 1)
    slots = parsed.display
    rows = []
    with R.DeviceContext(W, CODED_H, CF, slots=SLOTS) as ctx:
        ctx.upload(parsed.pics, parsed.mbs, parsed.coefs)
        ctx.decode()
        ctx.synchronize()
        rgb = torch.empty((SLOTS, 3, H, W), dtype=torch.uint8, device="cuda")
        for ow, oh in SIZES:
            fused_out = torch.empty((SLOTS, 3, oh, ow), dtype=torch.float16, device="cuda")
            torch.cuda.synchronize()
            keep = {}

            def fused():
                t0 = time.perf_counter()
                ctx.export_tensor(slots, (ow, oh), crop=(0, 0, W, H), dtype=torch.float16, mean=MEAN, std=STD,
                                  out=fused_out, sync=True)
                return time.perf_counter() - t0

            def unfused():
                t0 = time.perf_counter()
                ctx.export_rgb(slots, out=rgb, layout="nchw", chroma="linear", matrix=1, size=(W, H), sync=True)
                x = torch.nn.functional.interpolate(rgb.float(), size=(oh, ow), mode="bilinear", antialias=True)
                keep["out"] = ((x / 255 - mean) / std).half()
                torch.cuda.synchronize()
                return time.perf_counter() - t0

            def copy():
                t0 = time.perf_counter()
                if hip.hipMemcpyAsync(cdst.data_ptr(), csrc.data_ptr(), src_b, 3, None) or hip.hipStreamSynchronize(None):
                    raise RuntimeError("device-to-device copy failed")
                return time.perf_counter() - t0

            for _ in range(warmup):
                fused(), unfused(), copy()
            tf, tu, tc = [], [], []
            for _ in range(reps):
                tf.append(fused()), tu.append(unfused()), tc.append(copy())
            f_ms, u_ms, c_ms = (statistics.median(t) * 1e3 for t in (tf, tu, tc))
            diff = (fused_out.float() - keep["out"].float()).abs() * (255 * std)
            rows.append({"frames": SLOTS, "src": [W, H], "out": [ow, oh], "reps": reps,
                         "fused_ms": round(f_ms, 4), "fused_ms_min": round(min(tf) * 1e3, 4),
                         "fused_ms_max": round(max(tf) * 1e3, 4),
                         "unfused_ms": round(u_ms, 4), "unfused_ms_min": round(min(tu) * 1e3, 4),
                         "unfused_ms_max": round(max(tu) * 1e3, 4),
                         "copy_ms": round(c_ms, 4), "source_bytes": src_b,
                         "unfused_over_fused": round(u_ms / f_ms, 2), "fused_over_copy": round(f_ms / c_ms, 2),
                         "fused_source_tbps": round(src_b / (f_ms * 1e9), 3),
                         "frames_per_s": round(SLOTS / (f_ms * 1e-3)),
                         "max_abs_diff_8bit_steps": round(float(diff.max()), 3)})
            del fused_out, keep
    return rows


def write_md(path, rows, isa, device):
    lines = ["# Tensor export: fused kernel against the unfused path", "",
             "Written by `tools/tensor_bench.py`.  1080p 4:2:0, 256 slots filled by a generated stream; the",
             "visible 1920 x 1080 of each to float16 NCHW with ImageNet mean / std, LINEAR chroma.  Host",
             "clock around work that ends in a device synchronise, median of the repetitions, the three",
             "candidates alternated in one process: *fused* = one `mp2vg_tensor_slots` call; *unfused* =",
             "`export_rgb`, then torch `float()`, `interpolate(mode=\"bilinear\", antialias=True)`,",
             "normalise and `half()` on the same device (what a user had before); *copy* = a device-to-device",
             "`hipMemcpyAsync` of the source bytes (1.5 B per source pixel), the read-once floor.  The",
             "difference column is the largest |fused - unfused| in 8-bit steps (torch filters in float32",
             "and rounds the result to float16; the fused result is defined to the bit by include/mp2vg.h).", ""]
    if rows:
        lines += [f"Device: {device}.", "",
                  "| output | fused ms (min .. max) | unfused ms (min .. max) | copy ms | unfused / fused | fused / copy | "
                  "source TB/s (fused) | frames/s (fused) | max diff |",
                  "|---|---|---|---|---|---|---|---|---|"]
        for r in rows:
            lines.append(f"| {r['out'][0]} x {r['out'][1]} | {r['fused_ms']:.3f} ({r['fused_ms_min']:.3f} .. "
                         f"{r['fused_ms_max']:.3f}) | {r['unfused_ms']:.3f} ({r['unfused_ms_min']:.3f} .. "
                         f"{r['unfused_ms_max']:.3f}) | {r['copy_ms']:.3f} | {r['unfused_over_fused']:.2f} | "
                         f"{r['fused_over_copy']:.2f} | {r['fused_source_tbps']:.2f} | {r['frames_per_s']} | "
                         f"{r['max_abs_diff_8bit_steps']:.3f} |")
        lines.append("")
        lose = [r for r in rows if r["unfused_over_fused"] <= 1.0]
        if lose:
            lines.append("The fused call does NOT beat the unfused path at: " +
                         ", ".join(f"{r['out'][0]} x {r['out'][1]}" for r in lose) + ".")
        else:
            lines.append("The fused call beats the unfused path at every size measured.")
    else:
        lines.append("Not measured (no GPU in this run).  Static figures only.")
    lines += ["", f"Static figures of `{KERNEL}` (4:2:0, LINEAR, planar, F16; gfx950 ISA, whole kernel): "
              f"VGPRs {isa['vgprs']}, LDS {isa['lds_bytes']} B per workgroup, scratch {isa['scratch_bytes']} B; "
              f"instructions: VALU {isa['valu']}, SALU {isa['salu']}, LDS {isa['lds']}, global loads "
              f"{isa['vmem_load']}, global stores {isa['vmem_store']}.", "",
              "The distance to the copy floor (not profiled with counters): the vertical pass converts every",
              "source row an output row touches to R'G'B' (the RGB export's arithmetic, about 60 VALU per pixel",
              "with LINEAR chroma; profiles/export/README.md) before it weights it.  A workgroup makes two",
              "adjacent output rows from one conversion of the union of their source rows, so when downscaling",
              "a source row is converted about 1.5 times, and the kernel still issues more VALU work per source",
              "pixel than the RGB export while it moves a third of its bytes.", "",
              "Splits measured before this one, same workload and method (224 x 224 / 640 x 360): one output",
              "row per workgroup 1.477 / 1.687 ms; two rows per workgroup with each lane looping over its own",
              "tap count in the horizontal pass 1.240 / 1.701 ms (now every lane runs the axis' longest count",
              "over zero-padded weights, which keeps several tap loads in flight)."]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "export"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--isa-only", action="store_true")
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    isa = isa_figures()
    rows, device = [], None
    if not a.isa_only:
        import torch
        if not torch.cuda.is_available():
            sys.exit("tensor_bench: no GPU (a measurement does not fall back; --isa-only gives the static figures)")
        device = torch.cuda.get_device_name(0)
        rows = measure(a.reps, a.warmup)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "tensor.json"), "w") as f:
        json.dump({"device": device, "rows": rows, "isa": isa}, f, indent=1)
        f.write("\n")
    write_md(os.path.join(a.out, "tensor.md"), rows, isa, device)
    for r in rows:
        print(json.dumps(r))
    print(json.dumps(isa))


if __name__ == "__main__":
    main()
