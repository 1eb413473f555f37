#!/usr/bin/env python3
"""Speed of the items launch of the tensor export (mp2vg_tensor_items) on decoded 1080p 4:2:0 slots,
against what the entry points from before it can do, measured in one process.

64 slots are filled by a generated 1920 x 1088 stream.  Every figure is a host clock around work
that ends in a device synchronise (the context's stream is its own, so device events of the caller
cannot bracket it; tools/tensor_bench.py measures the same way), the candidates of one comparison
alternate, every shape is warmed up first, and the outputs of the candidates are compared to the bit.

  (a) many rectangles: 256 items with random-resized-crop rectangles (area 8 to 100 %, aspect 3/4 to
      4/3, fixed seed) of the visible 1920 x 1080 to 224 x 224 float16, ImageNet mean / std:
        items       one mp2vg_tensor_items launch
        singles     256 mp2vg_tensor_slots launches with n = 1 (arguments prepared outside the clock),
                    one synchronise behind the last
        items+clip  one items launch with flips and clip_len = 8: [32, 3, 8, 224, 224]
        singles+torch  singles, then torch on the same device: flip of the flagged images and the
                    permute to [32, 3, 8, 224, 224], contiguous
  (b) the same rectangle for every item: the items launch against mp2vg_tensor_slots with n = 256 on
      the same input, five repeats each (a repeat is the median of --reps timings), and the spread
      of the old path's five.  A third candidate attributes the difference: mp2vg_tensor_slots_fields
      with one frame of the 256 in mode WEAVE, which puts the old entry point on the field row walk
      the items kernel always rides (255 frames do the same work in both; the outputs of those are
      compared).
  (c) unshared tables: 256 items whose rectangles are all distinct in both sizes against the same
      origins (moved into the frame where needed) with eight distinct sizes: launch time and staged
      bytes (mp2vg_tensor_items_plan).

Writes items.json and items.md into --out.

    python tools/items_bench.py --out profiles/export        # on an MI355X
"""
import argparse
import ctypes
import json
import math
import os
import random
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

W, H, CODED_H, CF, SLOTS, N = 1920, 1080, 1088, 1, 64, 256
SIZE, CLIP = (224, 224), 8
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def random_resized_crops(n, seed):
    """torchvision's RandomResizedCrop sampling in integers: area 8 .. 100 % of W x H, aspect
    3/4 .. 4/3 log-uniform, ten tries, else the centre crop of the nearest allowed aspect."""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        for _ in range(10):
            area = W * H * rng.uniform(0.08, 1.0)
            aspect = math.exp(rng.uniform(math.log(3 / 4), math.log(4 / 3)))
            w, h = int(round(math.sqrt(area * aspect))), int(round(math.sqrt(area / aspect)))
            if 0 < w <= W and 0 < h <= H:
                out.append((rng.randint(0, W - w), rng.randint(0, H - h), w, h))
                break
        else:
            h = H
            w = min(W, int(round(h * 4 / 3)))
            out.append(((W - w) // 2, 0, w, h))
    return out


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def alternate(arms, reps, warmup):
    """{name: [ms] * reps}: every arm warmed up, then the arms in turn, reps times."""
    for fn in arms.values():
        for _ in range(warmup):
            fn()
    ms = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            ms[k].append(timed(fn))
    return ms


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms)}


def measure(reps, warmup):
    import torch
    from tiny_mp2v_dec_amd import _lib
    from tiny_mp2v_dec_amd import records as R
    lib = _lib.lib()
    es = R.generate_es(width=W, height=CODED_H, chroma_format=CF, n_gops=SLOTS // 16, gop_n=16, gop_m=4, seed=5)
    parsed = R.Parsed(es, W, CODED_H, CF)
    assert parsed.npics == SLOTS
    slots = [int(parsed.display[i % SLOTS]) for i in range(N)]
    crops = random_resized_crops(N, seed=2026)
    flips = [bool(random.Random(7 + i).getrandbits(1)) for i in range(N)]
    ow, oh = SIZE
    res = {"source": f"{W}x{H} 4:2:0, {SLOTS} decoded slots", "items": N, "size": list(SIZE), "dtype": "float16",
           "reps": reps, "warmup": warmup}
    with R.DeviceContext(W, CODED_H, CF, slots=SLOTS) as ctx:
        ctx.upload(parsed.pics, parsed.mbs, parsed.coefs)
        ctx.decode()
        ctx.synchronize()
        out_items = torch.empty((N, 3, oh, ow), dtype=torch.float16, device="cuda")
        out_single = torch.empty_like(out_items)
        out_clip = torch.empty((N // CLIP, 3, CLIP, oh, ow), dtype=torch.float16, device="cuda")
        torch.cuda.synchronize()
        nbytes = 3 * oh * ow * 2

        def items_call(its, out, clip_len=1):
            t = _lib.make_tensor(SIZE, None, "float16", MEAN, STD)
            _lib.check(lib.mp2vg_tensor_items(ctx.h, its, len(its), ctypes.byref(t), clip_len,
                                              ctypes.c_void_p(out.data_ptr()), out.numel() * 2), "tensor_items")
            ctx.synchronize()

        # (a) ----------------------------------------------------------------------------------------
        its_plain = _lib.make_items(slots, crops)
        its_flip = _lib.make_items(slots, crops, flips)
        single_args = []
        for i in range(N):
            single_args.append(((ctypes.c_int32 * 1)(slots[i]), _lib.make_tensor(SIZE, crops[i], "float16", MEAN, STD),
                                ctypes.c_void_p(out_single.data_ptr() + i * nbytes)))

        def singles():
            for s, t, dst in single_args:
                rc = lib.mp2vg_tensor_slots(ctx.h, s, 1, ctypes.byref(t), dst, nbytes)
                if rc:
                    _lib.check(rc, "tensor_slots")
            ctx.synchronize()

        mask = torch.tensor(flips, device="cuda").view(N // CLIP, CLIP, 1, 1, 1)
        keep = {}

        def singles_torch():
            singles()
            x = out_single.view(N // CLIP, CLIP, 3, oh, ow)
            keep["clip"] = torch.where(mask, x.flip(-1), x).permute(0, 2, 1, 3, 4).contiguous()
            torch.cuda.synchronize()

        ms = alternate({"items": lambda: items_call(its_plain, out_items), "singles": singles,
                        "items+clip": lambda: items_call(its_flip, out_clip, CLIP), "singles+torch": singles_torch},
                       reps, warmup)
        assert torch.equal(out_items, out_single), "items and single launches differ"
        assert torch.equal(out_clip, keep["clip"]), "items with flips and clip order differs from singles + torch"
        res["a"] = {k: summary(v) for k, v in ms.items()}
        res["a"]["outputs_equal"] = True
        pa = R.items_plan(W, CODED_H, CF, SIZE, None, items=its_plain)
        res["a"]["staged_bytes"] = 4 * pa["words"]
        res["a"]["tables"] = [pa["n_htab"], pa["n_vtab"]]

        # (b) ----------------------------------------------------------------------------------------
        rect = (0, 0, W, H)
        its_same = _lib.make_items(slots, [rect] * N)
        sl = (ctypes.c_int32 * N)(*slots)
        t_old = _lib.make_tensor(SIZE, rect, "float16", MEAN, STD)

        def old_path():
            _lib.check(lib.mp2vg_tensor_slots(ctx.h, sl, N, ctypes.byref(t_old), ctypes.c_void_p(out_single.data_ptr()),
                                              N * nbytes), "tensor_slots")
            ctx.synchronize()

        modes = (ctypes.c_int32 * N)(*([_lib.FIELD_WEAVE] + [_lib.FIELD_PROGRESSIVE] * (N - 1)))
        out_walk = torch.empty_like(out_items)
        torch.cuda.synchronize()

        def old_path_field_walk():
            _lib.check(lib.mp2vg_tensor_slots_fields(ctx.h, sl, modes, N, ctypes.byref(t_old),
                                                     ctypes.c_void_p(out_walk.data_ptr()), N * nbytes),
                       "tensor_slots_fields")
            ctx.synchronize()

        rounds = {"items": [], "tensor_slots": [], "tensor_slots_fields (field walk)": []}
        for _ in range(5):
            ms = alternate({"items": lambda: items_call(its_same, out_items), "tensor_slots": old_path,
                            "tensor_slots_fields (field walk)": old_path_field_walk}, reps, warmup)
            for k in rounds:
                rounds[k].append(statistics.median(ms[k]))
        assert torch.equal(out_items, out_single), "items and mp2vg_tensor_slots differ on one common rectangle"
        assert torch.equal(out_items[1:], out_walk[1:]), "the PROGRESSIVE frames of the field-walk launch differ"
        res["b"] = {k: {"repeat_medians_ms": v, "median_ms": statistics.median(v)} for k, v in rounds.items()}
        res["b"]["old_path_spread_ms"] = max(rounds["tensor_slots"]) - min(rounds["tensor_slots"])
        res["b"]["items_minus_old_ms"] = res["b"]["items"]["median_ms"] - res["b"]["tensor_slots"]["median_ms"]
        res["b"]["outputs_equal"] = True

        # (c) ----------------------------------------------------------------------------------------
        rng = random.Random(31)
        ws, hs = rng.sample(range(400, 1400), N), rng.sample(range(300, 900), N)
        distinct = [(rng.randint(0, W - w), rng.randint(0, H - h), w, h) for w, h in zip(ws, hs)]
        w8, h8 = sorted(ws)[::N // 8][:8], sorted(hs)[::N // 8][:8]
        eight = [(min(x, W - w8[i % 8]), min(y, H - h8[i % 8]), w8[i % 8], h8[i % 8])
                 for i, (x, y, _, _) in enumerate(distinct)]
        lists = {"all distinct": _lib.make_items(slots, distinct), "eight sizes": _lib.make_items(slots, eight)}
        ms = alternate({k: (lambda v=v: items_call(v, out_items)) for k, v in lists.items()}, reps, warmup)
        res["c"] = {}
        for k, v in lists.items():
            p = R.items_plan(W, CODED_H, CF, SIZE, None, items=v)
            res["c"][k] = dict(summary(ms[k]), staged_bytes=4 * p["words"], tables=[p["n_htab"], p["n_vtab"]])
    return res


def markdown(res):
    a, b, c = res["a"], res["b"], res["c"]
    f = lambda v: f"{v:.3f}"  # noqa: E731
    lines = [
        "# Items launch of the tensor export (tools/items_bench.py)", "",
        f"MI355X, {res['source']}; {res['items']} items to {res['size'][0]} x {res['size'][1]} {res['dtype']}, ImageNet "
        f"mean / std.  Host clock around work that ends in a device synchronise, candidates alternating, "
        f"{res['warmup']} warm-up and {res['reps']} timed repetitions each.  Outputs of the candidates compared equal "
        "to the bit.", "",
        "    python tools/items_bench.py --out profiles/export", "",
        "## (a) 256 random-resized-crop rectangles", "",
        "| candidate | median ms | min | max |", "|---|---|---|---|"]
    for k in ("items", "singles", "items+clip", "singles+torch"):
        lines.append(f"| {k} | {f(a[k]['median_ms'])} | {f(a[k]['min_ms'])} | {f(a[k]['max_ms'])} |")
    lines += ["", f"Staged by the items launch: {a['staged_bytes']} bytes ({a['tables'][0]} horizontal and "
              f"{a['tables'][1]} vertical tables).", "",
              "## (b) one common rectangle (the whole visible frame), 256 frames", "",
              "| candidate | median of 5 repeats, ms | the repeats |", "|---|---|---|"]
    for k in ("items", "tensor_slots", "tensor_slots_fields (field walk)"):
        lines.append(f"| {k} | {f(b[k]['median_ms'])} | {', '.join(f(v) for v in b[k]['repeat_medians_ms'])} |")
    lines += ["", f"Run-to-run spread of the old path: {f(b['old_path_spread_ms'])} ms; items minus old path: "
              f"{f(b['items_minus_old_ms'])} ms.", "",
              "## (c) unshared tables", "",
              "| item list | median ms | min | max | staged bytes | tables (h, v) |", "|---|---|---|---|---|---|"]
    for k, v in c.items():
        lines.append(f"| {k} | {f(v['median_ms'])} | {f(v['min_ms'])} | {f(v['max_ms'])} | {v['staged_bytes']} | "
                     f"{v['tables'][0]}, {v['tables'][1]} |")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "export"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("items_bench: no GPU (there is no CPU measurement of a GPU time)")
    res = measure(args.reps, args.warmup)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "items.json"), "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    with open(os.path.join(args.out, "items.md"), "w") as fh:
        fh.write(markdown(res))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
