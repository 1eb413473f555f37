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

Field modes (mp2vg_tensor_slots_fields): the 224 x 224 export again with every frame PROGRESSIVE, TOP
and WEAVE, alternated the same way, and the static figures of the field-mode kernel.  --ab ROOT
compares the PROGRESSIVE 224 x 224 figure with another checkout's (the parent commit, built): worker
processes of the two trees alternate on the same stream, each reports its median, and the margin is
the spread of the other checkout's own medians.

Placement (mp2vg_tensor_slots_placed): the 640 x 640 canvas with the 640 x 360 picture (CONTAIN,
square pixels) against the 640 x 360 export without placement, and against that export followed by
torch (a fill of the canvas and a copy into rows 140..499), alternated the same way; the static
figures of the placed kernel.  With --ab, both sizes of the table are compared with the other checkout.

    python tools/tensor_bench.py --out profiles/export        # on an MI355X
    python tools/tensor_bench.py --isa-only                   # the ISA figures alone, no GPU
    python tools/tensor_bench.py --isa-from DIR/tensor.json   # measure; static figures from that run
    python tools/tensor_bench.py --ab ../parent-checkout      # adds the A/B section
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
KERNEL = "tensor_kernelILi1ELb1ELb0ELi1ELb0ELb0EE"  # 4:2:0, LINEAR, planar, F16, without field modes
KERNEL_FIELDS = "tensor_kernelILi1ELb1ELb0ELi1ELb1ELb0EE"  # the same with the field row walk
KERNEL_PLACED = "tensor_kernelILi1ELb1ELb0ELi1ELb1ELb1EE"  # the same placed (always with the field row walk)
CANVAS = (640, 640)  # the placed measurement: SIZES[1] letterboxed into a square
FIELD_MODES = ("progressive", "top", "weave")
AB_ROUNDS = 4


_ISA = []  # the gfx950 ISA of tensor.hip, compiled once per run


def isa_text():
    from tiny_mp2v_dec_amd import build as B
    if not _ISA:
        csrc = os.path.join(REPO, "tiny_mp2v_dec_amd", "csrc")
        with tempfile.TemporaryDirectory() as tmp:
            asm = os.path.join(tmp, "tensor.s")
            subprocess.check_call([B._hipcc(), "-x", "hip", f"--offload-arch={B.ARCH}", "-O3", "-std=c++17", "-I", csrc,
                                   "-I", os.path.join(REPO, "include"), "--offload-device-only", "-S",
                                   os.path.join(csrc, "tensor.hip"), "-o", asm], stderr=subprocess.DEVNULL)
            _ISA.append(open(asm).read())
    return _ISA[0]


def isa_figures(kernel=KERNEL):
    """Static figures of one kernel variant from the gfx950 ISA."""
    text = isa_text()
    m = re.search(r"^(_ZN\w*%s\w*):[^\n]*\n(.*?)^\.Lfunc_end" % kernel, text, re.S | re.M)
    if not m:
        raise RuntimeError(f"kernel {kernel} not found in the ISA")
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
            print(f"tensor_bench: {rows[-1]}", file=sys.stderr, flush=True)  # progress: a long run stays audible
            del fused_out, keep
        field_rows = measure_fields(ctx, slots, reps, warmup)
        place_row = measure_place(ctx, slots, reps, warmup)
    return rows, field_rows, place_row


def measure_fields(ctx, slots, reps, warmup):
    """The 224 x 224 export of the same slots with one field mode for every frame, modes alternated."""
    import torch
    ow, oh = SIZES[0]
    out = torch.empty((SLOTS, 3, oh, ow), dtype=torch.float16, device="cuda")
    torch.cuda.synchronize()

    def run(mode):
        t0 = time.perf_counter()
        ctx.export_tensor(slots, (ow, oh), crop=(0, 0, W, H), dtype=torch.float16, mean=MEAN, std=STD, out=out,
                          sync=True, fields=mode)
        return time.perf_counter() - t0

    for _ in range(warmup):
        for mode in FIELD_MODES:
            run(mode)
    t = {mode: [] for mode in FIELD_MODES}
    for _ in range(reps):
        for mode in FIELD_MODES:
            t[mode].append(run(mode))
    return [{"mode": mode, "out": [ow, oh], "reps": reps, "ms": round(statistics.median(t[mode]) * 1e3, 4),
             "ms_min": round(min(t[mode]) * 1e3, 4), "ms_max": round(max(t[mode]) * 1e3, 4)} for mode in FIELD_MODES]


def measure_place(ctx, slots, reps, warmup):
    """(a) the placed CANVAS export of the SIZES[1] picture, (b) the SIZES[1] export without placement,
    (c) = (b), then torch: the canvas filled with the normalised pad colour and the picture copied
    into its rows; alternated.  (a) and (c) must be equal to the bit."""
    import torch
    from tiny_mp2v_dec_amd import _lib
    (ow, oh), (cw, ch) = SIZES[1], CANVAS
    crop, rect = _lib.tensor_fit("contain", (0, 0, W, H), (1, 1), CANVAS)
    assert crop == (0, 0, W, H) and rect == (0, (ch - oh) // 2, ow, oh), rect
    placed = torch.empty((SLOTS, 3, ch, cw), dtype=torch.float16, device="cuda")
    plain = torch.empty((SLOTS, 3, oh, ow), dtype=torch.float16, device="cuda")
    canvas = torch.empty_like(placed)
    pad = torch.tensor([-m / s for m, s in zip(MEAN, STD)], dtype=torch.float32, device="cuda").half().view(1, 3, 1, 1)
    torch.cuda.synchronize()
    kw = dict(crop=(0, 0, W, H), dtype=torch.float16, mean=MEAN, std=STD, sync=True)

    def a():
        t0 = time.perf_counter()
        ctx.export_tensor(slots, CANVAS, out=placed, place=rect, pad=(0, 0, 0), **kw)
        return time.perf_counter() - t0

    def b():
        t0 = time.perf_counter()
        ctx.export_tensor(slots, (ow, oh), out=plain, **kw)
        return time.perf_counter() - t0

    def c():
        t0 = time.perf_counter()
        ctx.export_tensor(slots, (ow, oh), out=plain, **kw)
        canvas.copy_(pad.expand_as(canvas))
        canvas[:, :, rect[1]:rect[1] + oh, :].copy_(plain)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for _ in range(warmup):
        a(), b(), c()
    ta, tb, tc = [], [], []
    for _ in range(reps):
        ta.append(a()), tb.append(b()), tc.append(c())
    ms = lambda t: {"ms": round(statistics.median(t) * 1e3, 4), "ms_min": round(min(t) * 1e3, 4),  # noqa: E731
                    "ms_max": round(max(t) * 1e3, 4)}
    row = {"canvas": list(CANVAS), "picture": [ow, oh], "rect": list(rect), "reps": reps, "placed": ms(ta),
           "unplaced": ms(tb), "unplaced_then_torch": ms(tc), "equal_to_torch_path": bool(torch.equal(placed, canvas))}
    row["placed_over_unplaced"] = round(row["placed"]["ms"] / row["unplaced"]["ms"], 3)
    row["placed_over_torch_path"] = round(row["placed"]["ms"] / row["unplaced_then_torch"]["ms"], 3)
    return row


def fused_worker(root, stream, reps, warmup):
    """One process of the A/B: the package of the checkout at `root`, the stream file, the fused
    exports of SIZES without field modes or placement, alternated; prints the median, minimum and
    maximum (ms) of each size."""
    sys.path.insert(0, root)
    import torch
    from tiny_mp2v_dec_amd import records as R
    es = open(stream, "rb").read()
    parsed = R.Parsed(es, W, CODED_H, CF)
    with R.DeviceContext(W, CODED_H, CF, slots=SLOTS) as ctx:
        ctx.upload(parsed.pics, parsed.mbs, parsed.coefs)
        ctx.decode()
        ctx.synchronize()
        outs = [torch.empty((SLOTS, 3, oh, ow), dtype=torch.float16, device="cuda") for ow, oh in SIZES]
        torch.cuda.synchronize()
        t = [[] for _ in SIZES]
        for i in range(warmup + reps):
            for k, (ow, oh) in enumerate(SIZES):
                t0 = time.perf_counter()
                ctx.export_tensor(parsed.display, (ow, oh), crop=(0, 0, W, H), dtype=torch.float16, mean=MEAN, std=STD,
                                  out=outs[k], sync=True)
                if i >= warmup:
                    t[k].append(time.perf_counter() - t0)
    print(json.dumps([{"ms": round(statistics.median(x) * 1e3, 4), "ms_min": round(min(x) * 1e3, 4),
                       "ms_max": round(max(x) * 1e3, 4)} for x in t]))


def ab(parent_root, reps, warmup):
    """Worker processes of the other checkout and of this one, alternated on one stream; a worker
    that fails ends the comparison (nothing more is started)."""
    from tiny_mp2v_dec_amd import records as R
    es = R.generate_es(width=W, height=CODED_H, chroma_format=CF, n_gops=SLOTS // 16, gop_n=16, gop_m=4, seed=5)
    runs = {"parent": [], "this": []}
    with tempfile.TemporaryDirectory() as tmp:
        stream = os.path.join(tmp, "stream.m2v")
        with open(stream, "wb") as f:
            f.write(es)
        pair = (("parent", os.path.abspath(parent_root)), ("this", REPO))
        for k in range(AB_ROUNDS):
            for who, root in (pair if k % 2 == 0 else pair[::-1]):  # parent, this; this, parent; ...
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--fused-worker", root, stream, "--reps",
                                    str(reps), "--warmup", str(warmup)], capture_output=True, text=True, timeout=300)
                if r.returncode != 0:
                    sys.exit(f"tensor_bench --ab: the {who} worker failed ({r.returncode}):\n{r.stderr[-2000:]}")
                runs[who].append(json.loads(r.stdout.strip().splitlines()[-1]))
                print(f"tensor_bench --ab: round {k}, {who}: {runs[who][-1]}", file=sys.stderr, flush=True)
    out = []
    for k, size in enumerate(SIZES):
        med = {who: [x[k]["ms"] for x in runs[who]] for who in runs}
        spread = max(med["parent"]) - min(med["parent"])
        delta = statistics.median(med["this"]) - statistics.median(med["parent"])
        out.append({"out": list(size), "reps": reps, "rounds": AB_ROUNDS, "parent_ms": med["parent"],
                    "this_ms": med["this"], "parent_spread_ms": round(spread, 4), "delta_ms": round(delta, 4),
                    "within_spread": abs(delta) <= spread})
    return out


def field_lines(field_rows, isa_fields, ab_result):
    lines = ["", "## Field modes", "",
             "`mp2vg_tensor_slots_fields`, the 224 x 224 export of the same 256 slots with one field mode for",
             "every frame, the modes alternated in one process (same clock and method as above).  A launch",
             "whose modes are all PROGRESSIVE runs the kernel without field modes, whose gfx950 instruction",
             "stream is the one from before the field modes existed; any other launch runs the field-mode",
             "kernel for all its frames.  TOP and BOTTOM convert only their field's lines (about half the",
             "rows) and add one rounded average per interpolated row; WEAVE converts every row, as",
             "PROGRESSIVE does, with the chroma taps of its own field.", ""]
    if field_rows:
        lines += ["| mode | ms (min .. max) | against PROGRESSIVE |", "|---|---|---|"]
        base = field_rows[0]["ms"]
        for r in field_rows:
            lines.append(f"| {r['mode'].upper()} | {r['ms']:.3f} ({r['ms_min']:.3f} .. {r['ms_max']:.3f}) | "
                         f"{r['ms'] / base:.2f} |")
        top = next(r for r in field_rows if r["mode"] == "top")
        if top["ms"] > base:
            lines += ["", "TOP is slower than PROGRESSIVE in this run although it converts half the rows; the cause was",
                      "not profiled."]
    else:
        lines.append("Not measured (no GPU in this run).  Static figures only.")
    lines += ["", f"Static figures of `{KERNEL_FIELDS}` (the same variant with field modes): VGPRs "
              f"{isa_fields['vgprs']}, LDS {isa_fields['lds_bytes']} B per workgroup, scratch "
              f"{isa_fields['scratch_bytes']} B; instructions: VALU {isa_fields['valu']}, SALU {isa_fields['salu']}, "
              f"LDS {isa_fields['lds']}, global loads {isa_fields['vmem_load']}, global stores "
              f"{isa_fields['vmem_store']}.  The LDS sets 6 waves per SIMD; up to 80 VGPRs keep that."]
    if ab_result:
        a = ab_result[0]
        lines += ["", "### PROGRESSIVE against the parent commit", "",
                  f"`--ab`: {a['rounds']} worker processes of the parent commit's checkout and {a['rounds']} of this",
                  "one, alternated (the order swapped every round) on one box and one stream, each the median of "
                  f"{a['reps']} fused 224 x 224 exports without field modes.", "",
                  "| checkout | medians of the runs, ms |", "|---|---|",
                  "| parent | " + ", ".join(f"{v:.3f}" for v in a["parent_ms"]) + " |",
                  "| this | " + ", ".join(f"{v:.3f}" for v in a["this_ms"]) + " |", "",
                  f"Margin = the spread of the parent's own medians: {a['parent_spread_ms']:.3f} ms.  Median of this "
                  f"checkout's medians minus the parent's: {a['delta_ms']:+.3f} ms: "
                  + ("inside the margin." if a["within_spread"] else "OUTSIDE the margin.")]
    return lines


def place_lines(place_row, isa_placed, ab_result):
    lines = ["", "## Placement", "",
             "`mp2vg_tensor_slots_placed`: the 640 x 360 picture of the same 256 slots letterboxed into a 640 x 640",
             "float16 canvas (CONTAIN, square pixels: rows 140..499, pad colour black) in one launch, against (b)",
             "the 640 x 360 export without placement and (c) that export followed by torch on the same device: a",
             "fill of the canvas with the normalised pad colour and a copy of the picture into its rows.  The",
             "three alternate in one process (same clock and method as above).  A placed launch runs the placed",
             "kernel, which always has the field row walk; launches without placement run the kernels they ran",
             "before, whose gfx950 instruction streams are unchanged.  A workgroup whose two canvas rows are both",
             "pad skips the vertical pass and only stores.", ""]
    if place_row:
        r = place_row
        f = lambda x: f"{x['ms']:.3f} ({x['ms_min']:.3f} .. {x['ms_max']:.3f})"  # noqa: E731
        lines += ["| candidate | ms (min .. max) |", "|---|---|",
                  f"| (a) placed 640 x 640 canvas, 640 x 360 picture | {f(r['placed'])} |",
                  f"| (b) unplaced 640 x 360 | {f(r['unplaced'])} |",
                  f"| (c) (b), then torch fill + copy | {f(r['unplaced_then_torch'])} |", "",
                  f"a / b = {r['placed_over_unplaced']:.3f}, a / c = {r['placed_over_torch_path']:.3f}.  "
                  + ("(a) and (c) are equal to the bit." if r["equal_to_torch_path"] else "(a) and (c) DIFFER.")]
        if r["placed_over_torch_path"] >= 1.0:
            lines += ["", "The placed launch is NOT faster than the export followed by torch."]
    else:
        lines.append("Not measured (no GPU in this run).  Static figures only.")
    lines += ["", f"Static figures of `{KERNEL_PLACED}` (the same variant placed): VGPRs {isa_placed['vgprs']}, LDS "
              f"{isa_placed['lds_bytes']} B per workgroup, scratch {isa_placed['scratch_bytes']} B; instructions: VALU "
              f"{isa_placed['valu']}, SALU {isa_placed['salu']}, LDS {isa_placed['lds']}, global loads "
              f"{isa_placed['vmem_load']}, global stores {isa_placed['vmem_store']}."]
    if ab_result:
        lines += ["", "### The exports without placement against the parent commit", "",
                  f"`--ab`: {ab_result[0]['rounds']} worker processes of the parent commit's checkout and as many of this",
                  "one, alternated (the order swapped every round) on one box and one stream; each worker alternates",
                  f"the two sizes and reports the median of {ab_result[0]['reps']} fused exports of each.  Margin = the "
                  "spread of the", "parent's own medians.", "",
                  "| output | parent medians, ms | this checkout's medians, ms | margin ms | median - median ms | |",
                  "|---|---|---|---|---|---|"]
        for a in ab_result:
            lines.append(f"| {a['out'][0]} x {a['out'][1]} | " + ", ".join(f"{v:.3f}" for v in a["parent_ms"]) + " | "
                         + ", ".join(f"{v:.3f}" for v in a["this_ms"]) + f" | {a['parent_spread_ms']:.3f} | "
                         f"{a['delta_ms']:+.3f} | " + ("inside" if a["within_spread"] else "OUTSIDE") + " |")
    return lines


def write_md(path, rows, isa, device, field_rows=None, isa_fields=None, ab_result=None, place_row=None,
             isa_placed=None):
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
    if isa_fields:
        lines += field_lines(field_rows, isa_fields, ab_result)
    if isa_placed:
        lines += place_lines(place_row, isa_placed, ab_result)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "export"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--isa-only", action="store_true")
    ap.add_argument("--isa-from", metavar="JSON", help="take the static figures from the tensor.json of an earlier "
                    "--isa-only run of the same source instead of compiling tensor.hip again")
    ap.add_argument("--ab", metavar="ROOT", help="a built checkout of the parent commit to compare PROGRESSIVE with")
    ap.add_argument("--fused-worker", nargs=2, metavar=("ROOT", "STREAM"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    if a.fused_worker:
        return fused_worker(a.fused_worker[0], a.fused_worker[1], a.reps, a.warmup)
    if a.isa_from:
        with open(a.isa_from) as f:
            prior = json.load(f)
        isa, isa_fields, isa_placed = prior["isa"], prior["isa_fields"], prior["isa_placed"]
    else:
        isa, isa_fields, isa_placed = isa_figures(), isa_figures(KERNEL_FIELDS), isa_figures(KERNEL_PLACED)
    rows, field_rows, place_row, ab_result, device = [], [], None, None, None
    if not a.isa_only:
        import torch
        if not torch.cuda.is_available():
            sys.exit("tensor_bench: no GPU (a measurement does not fall back; --isa-only gives the static figures)")
        device = torch.cuda.get_device_name(0)
        rows, field_rows, place_row = measure(a.reps, a.warmup)
        if a.ab:
            ab_result = ab(a.ab, a.reps, a.warmup)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "tensor.json"), "w") as f:
        json.dump({"device": device, "rows": rows, "isa": isa, "field_rows": field_rows, "isa_fields": isa_fields,
                   "place_row": place_row, "isa_placed": isa_placed, "ab": ab_result}, f, indent=1)
        f.write("\n")
    write_md(os.path.join(a.out, "tensor.md"), rows, isa, device, field_rows, isa_fields, ab_result, place_row,
             isa_placed)
    for r in rows + field_rows + ([place_row] if place_row else []):
        print(json.dumps(r))
    print(json.dumps(isa))
    print(json.dumps(isa_fields))
    print(json.dumps(isa_placed))
    if ab_result:
        print(json.dumps(ab_result))


if __name__ == "__main__":
    main()
