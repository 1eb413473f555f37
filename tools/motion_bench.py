#!/usr/bin/env python3
"""Speed of the motion export (mp2vg_motion_batch, motion.hip) over a resident batch parsed on the
device, against the same tensors computed by torch on the same device from the same record bytes.

The workload is the first --gops (64) GOPs of bench.py's c2 stream (1920 x 1088 4:2:0, N = 12,
M = 3), resident through mp2vg_batch_upload_es, every picture exported in display order.  After one
warm-up of every variant, --reps (5) alternating repetitions; the figures are device times from HIP
events: the library's own around its kernels (mp2vg_last_motion_time) and torch's around the
baseline on torch's stream.

  (a) mv + info only        (b) act only        (c) all three
  (d) the unfused baseline: the bank's records and words copied to torch tensors on the device
      (mp2vg_batch_download_records, then one host-to-device copy outside the clock); mv / info by
      views, masks, where and permute().contiguous(); act by index_add_ over a per-word MB index
      from repeat_interleave.  Its outputs are compared with (c) to the bit.

Bytes a variant must move, per MB: 32 read and 24 written for mv + info; for act 32 read (the
record's coef_off / ncoef), 4 per coefficient word and 8 B written; the fraction is of 8 TB/s.
Also times decode_motion end to end (host clock, stream in host memory to tensors in HBM).

Writes motion.json and motion.md into --out.

    python tools/motion_bench.py --out profiles/export        # on an MI355X
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

W, H, CF, NB = 1920, 1088, 1, 6
GOP = dict(gop_n=12, gop_m=3, leading_b=1)  # bench.py CONFIGS["c2"]
ROOF = 8e12


def baseline(torch, mbs, coefs, first, n, M):
    """(mv, info, act) of pictures whose first records are first[n], in torch ops."""
    dev = mbs.device
    idx = (first[:, None] + torch.arange(M, device=dev)[None, :]).reshape(-1)
    rec = mbs[idx]                                   # (n M, 32) uint8
    r16 = rec.view(torch.int16)                      # (n M, 16)
    flags = r16[:, 2].to(torch.int32) & 0xFFFF
    ncoef = r16[:, 5].to(torch.int32) & 0xFFFF
    off = rec.view(torch.int32)[:, 3].to(torch.int64)
    vec = r16[:, 8:16].reshape(-1, 2, 2, 2).to(torch.int32)  # [r][s][k]
    inter = (flags & 1) == 0
    used = [inter & (((flags & 2) != 0) | ((flags & 4) == 0)), inter & ((flags & 4) != 0)]
    field = (flags & 8) != 0
    chans = []
    for s in range(2):
        for r in range(2):
            sel = (flags >> (8 + 2 * r + s)) & 1
            x = torch.where(field, vec[:, r, s, 0], vec[:, 0, s, 0])
            y = torch.where(field, 2 * vec[:, r, s, 1] + 2 * (sel - r), vec[:, 0, s, 1])
            zero = torch.zeros_like(x)
            chans += [torch.where(used[s], x, zero), torch.where(used[s], y, zero)]
    mv = torch.stack(chans, 1).to(torch.int16).view(n, M, 8).permute(0, 2, 1).contiguous()
    info = torch.stack([flags & 0x0F1F, r16[:, 3].to(torch.int32) & 0xFFFF, rec[:, 8].to(torch.int32), ncoef], 1)
    info = info.to(torch.int16).view(n, M, 4).permute(0, 2, 1).contiguous()  # the uint16 bits
    # activity: one entry per coefficient word of the exported pictures
    cells = torch.arange(n * M, device=dev)
    nc = ncoef.to(torch.int64)
    mb = torch.repeat_interleave(cells, nc)
    start = torch.cumsum(nc, 0) - nc
    word = off[mb] + (torch.arange(mb.numel(), device=dev) - start[mb])
    w = coefs[word]                                  # int32 bits
    b = ((w >> 22) & 15).to(torch.int64)
    level = (w << 16) >> 16
    mag = torch.where((w & (1 << 30)) != 0, torch.zeros_like(level), level.abs())
    f, cell = mb // M, mb % M
    at = ((f * 2) * NB + b) * M + cell
    act = torch.zeros(n * 2 * NB * M, dtype=torch.int32, device=dev)
    act.index_add_(0, at, torch.ones_like(mag))
    act.index_add_(0, at + NB * M, mag)
    return mv, info, act.view(n, 2, NB, M)


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms)}


def measure(gops, reps):
    import numpy as np
    import torch
    from tiny_mp2v_dec_amd import records as R
    es = R.generate_es(width=W, height=H, chroma_format=CF, n_gops=gops, seed=1729, **GOP)
    mbw, mbh = W // 16, H // 16
    M = mbw * mbh
    res = {"source": f"{W}x{H} 4:2:0, {gops} GOPs of N=12 M=3, resident via upload_es", "reps": reps}
    with R.Scan(es, W, H, CF) as scan, R.DeviceContext(W, H, CF, slots=scan.npics) as ctx:
        n = scan.npics
        order = np.ascontiguousarray(scan.display, np.int32)
        ctx.upload_es(scan)
        ctx.synchronize()
        mbs_h, coefs_h = ctx.download_records()
        words = int(mbs_h["ncoef"].astype(np.int64).sum())
        assert words == len(coefs_h)
        res.update(pictures=n, mbs=n * M, words=words, parse_ms=ctx.parse_times_ms())
        mbs_t = torch.from_numpy(mbs_h.view(np.uint8).reshape(-1, 32)).cuda()
        coefs_t = torch.from_numpy(coefs_h.view(np.int32)).cuda()
        first = torch.from_numpy((scan.pics["mb_first"].astype(np.int64) - int(scan.pics["mb_first"][0]))[order]).cuda()
        torch.cuda.synchronize()
        keep = {}

        def fused(mv, info, act):
            keep["fused"] = ctx.export_motion(order, mv=mv, info=info, act=act)
            return ctx.motion_time_ms()

        def unfused():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            keep["base"] = baseline(torch, mbs_t, coefs_t, first, n, M)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1)

        arms = {"a: mv + info": lambda: fused(True, True, False), "b: act": lambda: fused(False, False, True),
                "c: mv + info + act": lambda: fused(True, True, True), "d: torch baseline": unfused}
        for fn in arms.values():
            fn()
        ms = {k: [] for k in arms}
        for _ in range(reps):
            for k, fn in arms.items():
                ms[k].append(fn())
        mv, info, act = keep["fused"]
        bmv, binfo, bact = keep["base"]
        assert torch.equal(mv.view(n, 8, M), bmv) and torch.equal(info.view(torch.int16).view(n, 4, M), binfo)
        assert torch.equal(act.view(n, 2, NB, M), bact)
        res["outputs_equal"] = True
        nm = n * M
        moved = {"a: mv + info": nm * (32 + 24), "b: act": nm * (32 + 8 * NB) + 4 * words,
                 "c: mv + info + act": nm * (32 + 24 + 8 * NB) + 4 * words}
        moved["d: torch baseline"] = moved["c: mv + info + act"]
        res["variants"] = {}
        for k, v in ms.items():
            s = summary(v)
            s["bytes"] = moved[k]
            s["roofline_fraction"] = moved[k] / (s["median_ms"] * 1e-3 * ROOF)
            res["variants"][k] = s
        c, d = res["variants"]["c: mv + info + act"], res["variants"]["d: torch baseline"]
        res["c_not_slower_than_d"] = c["median_ms"] <= d["median_ms"]
        res["pictures_per_s_c"] = n / (c["median_ms"] * 1e-3)
        del keep["fused"], keep["base"], mbs_t, coefs_t
        torch.cuda.empty_cache()
    # decode_motion end to end, host clock: scan, device parse, export, contexts and all
    e2e = []
    for _ in range(3):
        t0 = time.perf_counter()
        out = R.decode_motion(es, W, H, CF)
        torch.cuda.synchronize()
        e2e.append((time.perf_counter() - t0) * 1e3)
        del out
    res["decode_motion_ms"] = e2e[1:]
    res["decode_motion_pictures_per_s"] = n / (min(e2e[1:]) * 1e-3)
    res["stream_bytes"] = len(es)
    return res


def markdown(res):
    f = lambda v: f"{v:.3f}"  # noqa: E731
    lines = ["# Motion export (tools/motion_bench.py)", "",
             f"MI355X, {res['source']}: {res['pictures']} pictures in display order, {res['mbs']} MB records, "
             f"{res['words']} coefficient words.  Device times from HIP events (the library's around its kernels, "
             f"torch's around the baseline), one warm-up, then {res['reps']} alternating repetitions; the baseline's "
             "tensors compared equal to (c) to the bit.", "",
             "    python tools/motion_bench.py --out profiles/export", "",
             "| variant | median ms | min | max | bytes moved | of 8 TB/s |", "|---|---|---|---|---|---|"]
    for k, v in res["variants"].items():
        lines.append(f"| {k} | {f(v['median_ms'])} | {f(v['min_ms'])} | {f(v['max_ms'])} | {v['bytes']} | "
                     f"{100 * v['roofline_fraction']:.1f} % |")
    c, d = res["variants"]["c: mv + info + act"], res["variants"]["d: torch baseline"]
    verdict = ("holds" if res["c_not_slower_than_d"] else "DOES NOT HOLD")
    lines += ["", f"Condition (c) <= (d): {verdict}: {f(c['median_ms'])} ms against {f(d['median_ms'])} ms "
              f"({d['median_ms'] / c['median_ms']:.1f} x).  (c) is {res['pictures_per_s_c']:.0f} pictures/s of export; "
              f"the device parse of the same batch took {' + '.join(f(v) for v in res['parse_ms'])} ms (count, scan, emit).",
              "", "Reading the fractions: the repetitions export the same resident batch, whose MB records (32 bytes "
              "each) are smaller than the 256 MB Infinity Cache, so part of the reads of a repetition can be cache "
              "hits left by the one before; the fractions are of the HBM roofline but are not pure HBM rates.  The "
              "activity kernel is the larger share: per word it does a search in LDS and LDS atomics.",
              "", f"decode_motion end to end (host clock; scan on the host, {res['stream_bytes']} stream bytes to the "
              f"device, parse, export; a context per call): {', '.join(f(v) for v in res['decode_motion_ms'])} ms, "
              f"{res['decode_motion_pictures_per_s']:.0f} pictures/s."]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "export"))
    ap.add_argument("--gops", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("motion_bench: no GPU (there is no CPU measurement of a GPU time)")
    torch.cuda.init()
    res = measure(args.gops, args.reps)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "motion.json"), "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    with open(os.path.join(args.out, "motion.md"), "w") as fh:
        fh.write(markdown(res))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
