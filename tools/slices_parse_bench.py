#!/usr/bin/env python3
"""Device parse under MP2VG_PARSE_SLICES: what the flag costs and what more slices per row do.
A sibling of tools/device_parse_bench.py; the figures go into profiles/device_parse/slices.md.

  --write DIR      (no GPU) write one set of picture models (1920 x 1088, 4:2:0, I P B B P B B P) with
                   1, 2 and 4 slices per macroblock row, with the independent writer of
                   tests/slices_streams.py: DIR/rows1.m2v, rows2.m2v, rows4.m2v
  (default)        on an MI355X: the parse passes (HIP events: count [+ row, conceal], scan, emit) and
                   the host clock around upload_es, median [min, max] over --reps after a warm-up, for
                     the first --gops GOPs of bench.py's c2 stream with the flag clear and set, and
                     every stream of --streams DIR under the flag.
  --clear-only     only the c2 stream with the flag clear, --runs times in one process (each run a new
                   context): the figure to compare across two commits on one box, with its spread.
                   Uses nothing a commit before the flag lacks, so the same file runs from a checkout
                   of the parent commit (--stream FILE gives both the same bytes: bench.py keys its
                   prepared stream by the library's stamp).
Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import socket
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]


def stat(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def write_streams(out):
    import directed_syntax as DS
    import slices_streams as SL
    os.makedirs(out, exist_ok=True)
    ref = None
    for n in (1, 2, 4):
        S = SL.SlStream(f"rows{n}", 1920, 1088, 1, "ms")
        rng = DS._rng("slices_parse_bench")  # the same models for every n
        cut_at = [S.mbw * k // 4 for k in range(1, 4)]  # the model keeps these columns coded for every n
        use = {1: [], 2: cut_at[1:2], 4: cut_at}[n]
        pics = []
        for pct in (1, 2, 3, 3, 2, 3, 3, 2):
            rows = []
            for y in range(S.mbh):
                row = SL.gen_row(S, rng, pct, y, cut_at, qcode=5 + y % 20)
                row.cuts = [SL.Cut(x) for x in use]
                rows.append(row)
            pics.append(DS.Pic(pct, rows, fpfd=0))
        es = S.write(pics, [0, 3, 1, 2, 6, 4, 5, 7])
        if ref is None:
            ref = (S.mbs, S.coefs)
        assert (S.mbs, S.coefs) == ref
        with open(os.path.join(out, f"rows{n}.m2v"), "wb") as f:
            f.write(es)
        print(f"rows{n}: {S.nslices} slices, {len(es)} bytes")


def first_gops(es, n):
    at = -1
    for _ in range(n + 1):
        at = es.find(b"\x00\x00\x01\xb8", at + 1)
        if at < 0:
            return es
    return es[:at] + b"\x00\x00\x01\xb7"


def measure(R, es, w, h, cf, slots, reps, **flag):
    t = {k: [] for k in ("upload_es", "pass_count", "pass_scan", "pass_emit")}
    with R.DeviceContext(w, h, cf, slots=slots) as ctx:
        scan = R.Scan(es, w, h, cf, **flag)
        for rep in range(-1, reps):
            t0 = time.perf_counter()
            ctx.upload_es(scan)
            ms = (time.perf_counter() - t0) * 1e3
            passes = ctx.parse_times_ms()
            if rep >= 0:
                for k, v in zip(t, (ms, *passes)):
                    t[k].append(v)
        out = {"pictures": int(scan.npics), "slices": int(scan.nslices), "bytes": len(es), "ms": {k: stat(v) for k, v in t.items()}}
        scan.close()
    p = out["ms"]
    out["passes_ms"] = p["pass_count"]["median"] + p["pass_scan"]["median"] + p["pass_emit"]["median"]
    out["frames_per_s"] = out["pictures"] / (out["passes_ms"] / 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--write")
    ap.add_argument("--streams")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "device_parse", "slices_bench.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--gops", type=int, default=32)
    ap.add_argument("--stream", help="the c2 stream as a file (default: bench.py's prepared stream of this checkout)")
    ap.add_argument("--clear-only", action="store_true")
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()
    if args.write:
        return write_streams(args.write)

    import torch  # torch's HIP runtime opens the device before the library's
    torch.zeros(1, device="cuda")
    import bench
    from tiny_mp2v_dec_amd import records as R
    w, h, cf = bench.CONFIGS["c2"][:3]
    if args.stream:
        with open(args.stream, "rb") as fh:
            es = first_gops(fh.read(), args.gops)
    else:
        es = first_gops(bench.bench_stream("c2", bench.DEFAULT_GOPS["c2"], 1729), args.gops)
    res = {"box": socket.gethostname(), "device": torch.cuda.get_device_name(0), "gops": args.gops, "reps": args.reps,
           "provenance": __import__("tiny_mp2v_dec_amd.build", fromlist=["provenance"]).provenance()}
    if args.clear_only:
        res["c2_clear_runs"] = [measure(R, es, w, h, cf, args.gops * 12, args.reps) for _ in range(args.runs)]
    else:
        res["c2_clear"] = measure(R, es, w, h, cf, args.gops * 12, args.reps)
        res["c2_slices"] = measure(R, es, w, h, cf, args.gops * 12, args.reps, slices=True)
        res["c2_slices_conceal"] = measure(R, es, w, h, cf, args.gops * 12, args.reps, slices=True, conceal=True)
        res["rows"] = {}
        for n in (1, 2, 4):
            path = os.path.join(args.streams or "", f"rows{n}.m2v")
            if args.streams and os.path.exists(path):
                with open(path, "rb") as f:
                    res["rows"][str(n)] = measure(R, f.read(), 1920, 1088, 1, 8, args.reps, slices=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
