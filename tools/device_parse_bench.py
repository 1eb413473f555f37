#!/usr/bin/env python3
"""Speed of the device parse (mp2vg_batch_upload_es) against the host record emitter, on one box.

The stream is the first 64 GOPs (768 pictures, 1080p 4:2:0 IPB) of bench.py's default c2 stream
(`bench.py --prepare` writes it; it is generated with the same parameters when absent).  After one
warm-up of each candidate, the candidates alternate for --reps repetitions; each figure is a host
clock around work that ends in a device synchronise, reported as median [min, max]:

  (a) host path    Parsed(threads=mp2vg_cpu_budget()) wall, upload, decode
      device path  Scan wall, upload_es (copy, count pass, scan, emit pass, plan), decode
  (b) the three parse-pass device times (HIP events) and the decode's launches
  (c) the drop-in decoder end to end with and without MP2VG_DECODER_DEVICE_PARSE, with host
      frames and with device frames

There is no threshold: the flag is opt-in either way.  Writes device_parse.json and README.md
into --out.  --conceal runs every parse under MP2VG_PARSE_CONCEAL (the cost of the flag on an
undamaged stream, profiles/device_parse/conceal.md), --standard under MP2VG_PARSE_STANDARD
(profiles/device_parse/standard.md; the c2 stream carries full extensions and intra_vlc_format 1, so
the flag changes none of its records); --no-dropin leaves (c) out.

    python tools/device_parse_bench.py --out profiles/device_parse        # on an MI355X
    python tools/device_parse_bench.py --from-json profiles/device_parse/device_parse.json   # README.md again
"""
import argparse
import json
import os
import socket
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

GOPS = 64


def first_gops(es, n):
    """the stream up to its (n + 1)th group_of_pictures_header, closed with a sequence_end_code"""
    at = -1
    for _ in range(n + 1):
        at = es.find(b"\x00\x00\x01\xb8", at + 1)
        if at < 0:
            return es
    return es[:at] + b"\x00\x00\x01\xb7"


def stat(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def fmt(s, unit="ms"):
    return f"{s['median']:.2f} [{s['min']:.2f}, {s['max']:.2f}] {unit}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "device_parse"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--gops", type=int, default=GOPS)
    ap.add_argument("--from-json", help="render README.md again from a device_parse.json; no GPU needed")
    ap.add_argument("--conceal", action="store_true", help="parse, scan and decode under MP2VG_PARSE_CONCEAL")
    ap.add_argument("--standard", action="store_true", help="parse, scan and decode under MP2VG_PARSE_STANDARD")
    ap.add_argument("--no-dropin", action="store_true", help="skip the drop-in decoder runs")
    args = ap.parse_args()
    if args.from_json:
        with open(args.from_json) as fh:
            write_readme(json.load(fh), args.out)
        return

    import torch  # torch's HIP runtime opens the device before the library's
    torch.zeros(1, device="cuda")
    import bench
    from tiny_mp2v_dec_amd import _lib
    from tiny_mp2v_dec_amd import records as R
    from tiny_mp2v_dec_amd.decoder import decoder_config_t, mp2v_decoder_c

    w, h, cf = bench.CONFIGS["c2"][:3]
    es = first_gops(bench.bench_stream("c2", bench.DEFAULT_GOPS["c2"], 1729), args.gops)
    threads = _lib.lib().mp2vg_cpu_budget()
    ms = lambda t0: (time.perf_counter() - t0) * 1e3  # noqa: E731
    flag = {"conceal": True} if args.conceal else {}
    if args.standard:
        flag["standard"] = True

    t = {k: [] for k in ("parsed", "upload", "decode_host", "scan", "upload_es", "decode_dev", "host_total",
                         "dev_total", "pass_count", "pass_scan", "pass_emit", "launch_sum", "batch_span")}
    nlaunch = npics = nslices = nrec = 0
    with R.DeviceContext(w, h, cf, slots=args.gops * 12) as ctx:
        for rep in range(-1, args.reps):  # -1: warm-up (allocations, the pool's placement calibration)
            t0 = time.perf_counter()
            parsed = R.Parsed(es, w, h, cf, threads=threads, **flag)
            a = ms(t0)
            t1 = time.perf_counter()
            ctx.upload(parsed.pics, parsed.mbs, parsed.coefs)
            b = ms(t1)
            t1 = time.perf_counter()
            ctx.decode()
            ctx.synchronize()
            c = ms(t1)
            host_total = ms(t0)
            npics, nrec = parsed.npics, parsed.mbs.nbytes + parsed.coefs.nbytes
            del parsed

            t0 = time.perf_counter()
            scan = R.Scan(es, w, h, cf, **flag)
            d = ms(t0)
            t1 = time.perf_counter()
            ctx.upload_es(scan)
            e = ms(t1)
            t1 = time.perf_counter()
            ctx.decode()
            ctx.synchronize()
            f = ms(t1)
            dev_total = ms(t0)
            passes, launches, span = ctx.parse_times_ms(), ctx.launch_times_ms(), ctx.batch_time_ms()
            nlaunch, nslices = len(launches), scan.nslices
            scan.close()
            if rep < 0:
                continue
            for k, v in zip(("parsed", "upload", "decode_host", "host_total", "scan", "upload_es", "decode_dev",
                             "dev_total", "pass_count", "pass_scan", "pass_emit", "launch_sum", "batch_span"),
                            (a, b, c, host_total, d, e, f, dev_total, *passes, sum(launches), span)):
                t[k].append(v)

    dropin = {}
    for dev_frames in (() if args.no_dropin else (False, True)):
        for dev_parse in (False, True):
            key = f"{'device' if dev_frames else 'host'}_frames_{'device' if dev_parse else 'host'}_parse"
            frames = [0]

            def render(fr):
                frames[0] += 1

            dec = mp2v_decoder_c(decoder_config_t(w, h, cf, device_frames=dev_frames, device_parse=dev_parse, **flag),
                                 render)
            runs = []
            try:
                for rep in range(-1, min(args.reps, 3)):
                    frames[0] = 0
                    t0 = time.perf_counter()
                    dec.decode(es)
                    if rep >= 0:
                        runs.append(ms(t0))
                    assert frames[0] == npics
            finally:
                dec.close()
            dropin[key] = {"ms": stat(runs), "frames_per_s": npics / (statistics.median(runs) / 1e3)}

    res = {
        "box": socket.gethostname(), "device": torch.cuda.get_device_name(0), "cpu_budget": threads,
        "stream": {"config": "c2", "gops": args.gops, "pictures": npics, "slices": nslices, "bytes": len(es),
                   "record_bytes": nrec},
        "reps": args.reps, "conceal": bool(args.conceal), "standard": bool(args.standard), "launches": nlaunch, "ms": {k: stat(v) for k, v in t.items()}, "dropin": dropin,
        "provenance": __import__("tiny_mp2v_dec_amd.build", fromlist=["provenance"]).provenance(),
    }
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "device_parse.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    if dropin:  # (README.md reads all three parts)
        write_readme(res, args.out)
    m = res["ms"]
    print(json.dumps({"host_total_ms": m["host_total"]["median"], "device_total_ms": m["dev_total"]["median"],
                      "passes_ms": [m["pass_count"]["median"], m["pass_scan"]["median"], m["pass_emit"]["median"]],
                      "dropin": {k: round(v["frames_per_s"]) for k, v in dropin.items()}}))


def write_readme(res, out):
    """README.md from the measured figures alone (--from-json renders it again without a GPU)"""
    m, dropin, st = res["ms"], res["dropin"], res["stream"]
    npics, nslices, threads = st["pictures"], st["slices"], res["cpu_budget"]
    fps = lambda k: npics / (m[k]["median"] / 1e3)  # noqa: E731
    passes_total = m["pass_count"]["median"] + m["pass_scan"]["median"] + m["pass_emit"]["median"]
    lines = [
        "# Device parse against the host record emitter",
        "",
        f"`tools/device_parse_bench.py` on {res['box']} ({res['device']}, {threads} CPUs for the process): the first "
        f"{st['gops']} GOPs of the bench's c2 stream, {npics} pictures of 1080p 4:2:0, {nslices} slices, "
        f"{st['bytes'] / 1e6:.1f} MB of bitstream against {st['record_bytes'] / 1e6:.1f} MB of records.  One warm-up, "
        f"then {res['reps']} alternating repetitions; median [min, max] of host clocks that end in a device "
        "synchronise.",
        "",
        "## (a) From the stream to decoded frames",
        "",
        "| step | host path | device path |",
        "|---|---|---|",
        f"| parse / scan on the host | `Parsed(threads={threads})` {fmt(m['parsed'])} | `Scan` {fmt(m['scan'])} |",
        f"| upload | `upload` {fmt(m['upload'])} | `upload_es` {fmt(m['upload_es'])} |",
        f"| decode + synchronise | {fmt(m['decode_host'])} | {fmt(m['decode_dev'])} |",
        f"| total | {fmt(m['host_total'])} = {fps('host_total'):,.0f} frames/s | {fmt(m['dev_total'])} = "
        f"{fps('dev_total'):,.0f} frames/s |",
        "",
        "## (b) Inside `upload_es` and the decode (device times, HIP events)",
        "",
        f"- count pass {fmt(m['pass_count'])}, scan {fmt(m['pass_scan'])}, emit pass {fmt(m['pass_emit'])}: "
        f"{nslices / (m['pass_count']['median'] / 1e3) / 1e6:.2f} M slices/s in the count pass, "
        f"{npics / (passes_total / 1e3):,.0f} frames/s over the three passes;",
        f"- the decode of the device-parsed batch: {res['launches']} launches, {fmt(m['launch_sum'])} summed, batch "
        f"span {fmt(m['batch_span'])}.",
        "",
        "## (c) The drop-in decoder end to end",
        "",
        "| frames | parse | decode() | frames/s | ms per 16-picture chunk |",
        "|---|---|---|---|---|",
    ]
    chunks = max(1, (npics + 15) // 16)
    for key, v in dropin.items():
        fr, _, pa, _ = key.split("_")
        lines.append(f"| {fr} | {pa} | {fmt(v['ms'])} | {v['frames_per_s']:,.0f} | {v['ms']['median'] / chunks:.2f} |")
    host_fps, dev_fps = fps("host_total"), fps("dev_total")
    ratios = [dropin[f"{fr}_frames_device_parse"]["frames_per_s"] / dropin[f"{fr}_frames_host_parse"]["frames_per_s"]
              for fr in ("host", "device")]
    lines += [
        "",
        "## Reading",
        "",
        f"(a) Whole batch: from the stream to decoded frames the device path runs at {dev_fps / host_fps:.2f} times "
        "the host path's rate on this box: the device path "
        + ("wins." if dev_fps > host_fps else "loses: the lane-per-slice parse is slower than this box's host threads."),
        "",
        f"(c) Drop-in: with the flag decode() runs at {ratios[0]:.2f} (host frames) and {ratios[1]:.2f} (device "
        "frames) times its rate without it: the flag "
        + ("wins" if min(ratios) > 1 else "loses" if max(ratios) < 1 else "wins one and loses one")
        + f" here.  A 16-picture chunk has 16 x {nslices // max(1, npics)} slices, a few waves, and "
        "`mp2vg_batch_upload_es` is synchronous, so the chunk loop waits for a count and an emit pass per chunk; a "
        f"chunk costs about what the three passes cost over the whole {npics}-picture batch ({passes_total:.2f} ms), "
        "which suggests that a pass lasts as long as its slowest lane however few slices it has (an inference from "
        "these totals: no pass was timed per chunk).  One lane per slice pays off with tens of thousands of slices "
        "in flight, which `upload_es` on a long range has and the drop-in's chunks do not.",
        "",
        "The flag stays opt-in either way, and no threshold is set.  What bounds the count and emit passes (lane "
        "divergence, table loads through L1 / L2; the kernels use no scratch memory) is unprofiled: no counter run "
        "was made.",
        "",
    ]
    with open(os.path.join(out, "README.md"), "w") as fh:
        fh.write("\n".join(lines))


if __name__ == "__main__":
    main()
