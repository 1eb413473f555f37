#!/usr/bin/env python3
"""Speed of the residual export (mp2vg_residual_batch, residual.hip) over a resident batch parsed on
the device, against the only way to obtain the same tensors without it: two mp2vg_batch_decode runs
of the same pictures over a constant reference slot (all 0, then all 255) and the torch combine
dec0 + dec255 - 255.

The workload is the first --gops (64) GOPs of bench.py's c2 stream (1920 x 1088 4:2:0, N = 12,
M = 3), resident through mp2vg_batch_upload_es with every P and B picture predicting from one extra
slot (the records' words and vectors are the stream's; the export does not look at slots).  The
first --pictures pictures in display order are exported (default: all; 2 x 1.5 x W x H bytes each at
int16).  After one warm-up of every arm, --reps (5) alternating repetitions; the figures are device
times from HIP events: the library's own around its kernel (mp2vg_last_residual_time) and around
each decode (mp2vg_last_batch_time), torch's around the combine.  Copying the decoded slots into
torch tensors is left out of the baseline's time.

  (a) export int16        (b) export int8        (c) the two-decode baseline
  I / P / B: (a) over the pictures of one type only

The baseline's tensors are compared with (a) to the bit on non-intra MBs; on intra MBs clip(R, 0,
255) is compared with the decode.  Bytes a run must move: 32 per MB record and 4 per coefficient
word read, the planes written; the fraction is of 8 TB/s.

Writes residual.json and residual.md into --out.

    python tools/residual_bench.py --out profiles/export        # on an MI355X
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

W, H, CF = 1920, 1088, 1
GOP = dict(gop_n=12, gop_m=3, leading_b=1)  # bench.py CONFIGS["c2"]
ROOF = 8e12


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms)}


def measure(gops, reps, pictures):
    import numpy as np
    import torch
    from tiny_mp2v_dec_amd import records as R
    from tiny_mp2v_dec_amd.decoder import _hip_lib
    es = R.generate_es(width=W, height=H, chroma_format=CF, n_gops=gops, seed=1729, **GOP)
    mbw, mbh = W // 16, H // 16
    M = mbw * mbh
    res = {"source": f"{W}x{H} 4:2:0, {gops} GOPs of N=12 M=3, resident via upload_es", "reps": reps}
    with R.Scan(es, W, H, CF) as scan, R.DeviceContext(W, H, CF, slots=scan.npics + 1) as ctx:
        ref = scan.npics
        pics = scan.pics.copy()
        assert ref not in pics["dst_slot"]
        types = pics["picture_coding_type"].astype(np.int64)
        pics["fwd_slot"] = np.where(types > 1, ref, -1)
        pics["bwd_slot"] = np.where(types == 3, ref, -1)
        display = np.ascontiguousarray(scan.display, np.int32)
        order = display[:pictures] if pictures else display
        n = len(order)
        ctx.upload_es(scan, pics=pics)
        ctx.synchronize()
        mbs_h, coefs_h = ctx.download_records()
        ncoef = mbs_h["ncoef"].astype(np.int64).reshape(scan.npics, M)
        intra_h = (mbs_h["flags"] & 1).astype(bool).reshape(scan.npics, mbh, mbw)
        frame = ctx.frame_bytes()
        fill = {c: np.full(int(ctx.slot_bytes), c, np.uint8) for c in (0, 255)}
        keep = {}

        def export(dtype, sub=None):
            keep[dtype] = ctx.export_residual(order if sub is None else sub, dtype=dtype)
            return ctx.residual_time_ms()

        def decode_over(c, out):
            assert _hip_lib().hipMemcpy(ctx.slot_ptr(ref), fill[c].ctypes.data, fill[c].nbytes, 1) == 0
            ctx.invalidate(ref)
            ctx.decode()
            ctx.synchronize()
            ms = ctx.batch_time_ms()
            for i, p in enumerate(order):  # outside the clock
                ctx.copy_packed(int(pics[p]["dst_slot"]), out[i].data_ptr(), True)
            return ms

        d0 = torch.empty((n, frame), dtype=torch.uint8, device="cuda")
        d255 = torch.empty((n, frame), dtype=torch.uint8, device="cuda")

        def baseline():
            t0 = decode_over(0, d0)
            t1 = decode_over(255, d255)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            keep["base"] = d0.to(torch.int16) + d255.to(torch.int16) - 255
            e1.record()
            torch.cuda.synchronize()
            keep["parts"] = (t0, t1, e0.elapsed_time(e1))
            return t0 + t1 + keep["parts"][2]

        by_type = {name: order[types[order] == t] for name, t in (("I", 1), ("P", 2), ("B", 3))}
        arms = {"a: export int16": lambda: export("int16"), "b: export int8": lambda: export("int8"),
                "c: two decodes + combine": baseline}
        for name, sub in by_type.items():
            arms[f"{name}: export int16, {len(sub)} {name} pictures"] = (lambda s=sub: export("int16", s))
        for fn in arms.values():
            fn()
        ms = {k: [] for k in arms}
        for _ in range(reps):
            for k, fn in arms.items():
                ms[k].append(fn())
        # equality: (a) against the baseline on non-intra MBs, against the decode on intra MBs
        export("int16")
        y, cb, cr = keep["int16"]
        R16 = torch.cat([y.view(n, -1), cb.view(n, -1), cr.view(n, -1)], 1)
        it = torch.from_numpy(intra_h[order]).cuda()
        my = it.repeat_interleave(16, 1).repeat_interleave(16, 2).view(n, -1)
        mc = it.repeat_interleave(8, 1).repeat_interleave(8, 2).view(n, -1)
        mask = torch.cat([my, mc, mc], 1)
        assert R16.shape == keep["base"].shape == mask.shape
        for i in range(0, n, 32):  # in chunks of pictures: elementwise, no gathers of billions of elements
            r, b, m, a0, a255 = (t[i:i + 32] for t in (R16, keep["base"], mask, d0, d255))
            intra_ok = (r.clamp(0, 255) == a0.to(torch.int16)) & (a0 == a255)
            assert bool(torch.where(m, intra_ok, r == b).all()), f"pictures {i} .. {i + 31}"
        y8 = ctx.export_residual(order, dtype="int8")[0]
        assert torch.equal(y8.to(torch.int16), y.clamp(-128, 127))
        res["outputs_equal"] = True
        res["intra_mb_fraction"] = float(intra_h[order].mean())
        res["coded_sample_fraction"] = float(torch.count_nonzero(R16)) / R16.numel()

        def moved(sub, el):
            return int(len(sub) * M * 32 + 4 * ncoef[sub].sum()), int(len(sub) * frame * el)

        res.update(pictures=n, pictures_resident=int(scan.npics), words=int(ncoef[order].sum()),
                   parse_ms=ctx.parse_times_ms(), decode_parts_ms=list(keep["parts"]))
        res["variants"] = {}
        for k, v in ms.items():
            s = summary(v)
            if k[0] != "c":
                sub = order if k[0] in "ab" else by_type[k[0]]
                s["bytes_read"], s["bytes_written"] = moved(sub, 1 if k[0] == "b" else 2)
                s["roofline_fraction"] = (s["bytes_read"] + s["bytes_written"]) / (s["median_ms"] * 1e-3 * ROOF)
                s["us_per_picture"] = 1e3 * s["median_ms"] / len(sub)
            res["variants"][k] = s
        a, c = res["variants"]["a: export int16"], res["variants"]["c: two decodes + combine"]
        res["a_not_slower_than_c"] = a["median_ms"] <= c["median_ms"]
        res["ratio_c_over_a"] = c["median_ms"] / a["median_ms"]
    return res


def markdown(res):
    f = lambda v: f"{v:.3f}"  # noqa: E731
    lines = ["# Residual export (tools/residual_bench.py)", "",
             f"MI355X, {res['source']}: {res['pictures']} of {res['pictures_resident']} resident pictures exported in "
             f"display order, {res['words']} coefficient words, {100 * res['intra_mb_fraction']:.1f} % of the MBs intra, "
             f"{100 * res['coded_sample_fraction']:.1f} % of the samples non-zero.  Device times from HIP events (the "
             f"library's around its kernel and around each decode, torch's around the combine), one warm-up, then "
             f"{res['reps']} alternating repetitions; the baseline compared equal to (a) to the bit on non-intra MBs, "
             "the decode equal to clip(R, 0, 255) on intra MBs, int8 equal to clamp(int16).", "",
             "    python tools/residual_bench.py --out profiles/export", "",
             "| variant | median ms | min | max | us / picture | bytes read | bytes written | of 8 TB/s |",
             "|---|---|---|---|---|---|---|---|"]
    for k, v in res["variants"].items():
        if "bytes_read" in v:
            lines.append(f"| {k} | {f(v['median_ms'])} | {f(v['min_ms'])} | {f(v['max_ms'])} | {v['us_per_picture']:.2f} | "
                         f"{v['bytes_read']} | {v['bytes_written']} | {100 * v['roofline_fraction']:.1f} % |")
        else:
            lines.append(f"| {k} | {f(v['median_ms'])} | {f(v['min_ms'])} | {f(v['max_ms'])} | | | | |")
    a, c = res["variants"]["a: export int16"], res["variants"]["c: two decodes + combine"]
    verdict = "holds" if res["a_not_slower_than_c"] else "DOES NOT HOLD"
    lines += ["", f"Condition (a) <= (c): {verdict}: {f(a['median_ms'])} ms against {f(c['median_ms'])} ms "
              f"({res['ratio_c_over_a']:.1f} x).  The last baseline run: decode over 0 "
              f"{f(res['decode_parts_ms'][0])} ms, decode over 255 {f(res['decode_parts_ms'][1])} ms, combine "
              f"{f(res['decode_parts_ms'][2])} ms; the copies of the decoded slots into tensors are not in it.  The "
              f"device parse of the batch took {' + '.join(f(v) for v in res['parse_ms'])} ms (count, scan, emit).",
              "", "Reading the fractions: the repetitions export the same resident batch; its records and words are read "
              "once per run and the planes are written once, so the fraction is of the HBM roofline, but part of the "
              "reads of a repetition can be Infinity Cache hits left by the one before.  The I / P / B rows are launches "
              "over the pictures of one type."]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "export"))
    ap.add_argument("--gops", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pictures", type=int, default=0, help="export the first N pictures in display order (0: all)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("residual_bench: no GPU (there is no CPU measurement of a GPU time)")
    torch.cuda.init()
    res = measure(args.gops, args.reps, args.pictures)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "residual.json"), "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    with open(os.path.join(args.out, "residual.md"), "w") as fh:
        fh.write(markdown(res))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
