"""Generate the directed slice-syntax fixtures, pinned by the REAL reference decoder.

Run in the build container (needs oracle/_ref/ref_decode, built from the reference by
`make -C oracle ref`).  For every stream of tests/directed_syntax.py (written by its own bit
writer, not by the library's): decode it with the compiled reference at one thread and store
  tests/golden/syntax/<name>.m2v       the stream
  tests/golden/syntax/manifest.json    geometry, per-frame MD5 of the reference's YUV output in
                                       display order, and the stream's syntax event log
The negative streams are stored too (no MD5: nothing decodes them).

As in make_stream_fixtures.py the reference's scheduler can deliver a stale frame even at one
thread; such a run is recognised by a frame that repeats an earlier one.  That test relies on no
two frames of a stream being equal, which a directed stream could break (a P picture of skips
only), so this maker asserts on the reference's own frames that every picture of a stream
differs from every other, and the writer gives every picture a macroblock that changes pixels.
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
REF = os.path.join(REPO, "oracle", "_ref", "ref_decode")
OUT = os.path.join(HERE, "syntax")
RUNS = 6

import directed_syntax as DS  # noqa: E402


def ref_md5s(path, w, h, cf, out):
    r = subprocess.run([REF, path, str(w), str(h), str(cf), "1", out], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"reference failed on {path}: {r.returncode} {r.stderr[-400:]}")
    frames = json.loads(r.stdout.strip().splitlines()[-1])["frames"]
    cw = w if cf == 3 else w // 2
    ch = h if cf != 1 else h // 2
    fb = w * h + 2 * cw * ch
    data = open(out, "rb").read()
    assert len(data) == fb * frames, path
    return [hashlib.md5(data[k * fb:(k + 1) * fb]).hexdigest() for k in range(frames)]


def main():
    if not os.path.exists(REF):
        sys.exit("build the reference first: make -C oracle ref")
    os.makedirs(OUT, exist_ok=True)
    manifest = []
    with tempfile.TemporaryDirectory() as tmp:
        yuv = os.path.join(tmp, "a.yuv")
        for S in DS.build_all():
            path = os.path.join(OUT, S.name + ".m2v")
            with open(path, "wb") as f:
                f.write(S.es)
            runs = [ref_md5s(path, S.width, S.height, S.cf, yuv) for _ in range(RUNS)]
            good = [r for r in runs if len(r) == S.npics and len(set(r)) == len(r)]
            if not good:
                raise RuntimeError(f"{S.name}: no reference run with {S.npics} pairwise different frames: {runs[0]}")
            if any(r != good[0] for r in good):
                raise RuntimeError(f"{S.name}: clean reference runs disagree")
            stale = sum(1 for r in runs if r != good[0])
            if stale:
                print(f"WARNING {S.name}: {stale} of {RUNS} reference runs delivered a stale frame")
            manifest.append(dict(name=S.name, file=S.name + ".m2v", width=S.width, height=S.height,
                                 chroma_format=S.cf, frames=S.npics, bytes=len(S.es), md5=good[0],
                                 events=sorted(S.events)))
            print(f"{S.name}: {S.npics} frames, {len(S.es)} bytes")
        for build, status, reason in DS.NEGATIVE:
            S = build()
            with open(os.path.join(OUT, S.name + ".m2v"), "wb") as f:
                f.write(S.es)
            manifest.append(dict(name=S.name, file=S.name + ".m2v", width=S.width, height=S.height,
                                 chroma_format=S.cf, frames=0, bytes=len(S.es), md5=None, status=status,
                                 reason=reason, events=[]))
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1)
        f.write("\n")
    # the streams at the geometry limits: under 400 KB each and 1 MB together; all others 256 KB together
    limit = {n + ".m2v": os.path.getsize(os.path.join(OUT, n + ".m2v")) for n in DS.LIMIT_NAMES}
    assert max(limit.values()) < 400 * 1024 and sum(limit.values()) < 1024 * 1024, limit
    total = sum(os.path.getsize(os.path.join(OUT, n)) for n in os.listdir(OUT) if n not in limit)
    assert total < 256 * 1024, total
    print(f"{len(manifest)} streams, {total} + {sum(limit.values())} bytes")


if __name__ == "__main__":
    main()
