"""Generate the twin-stream fixtures of MP2VG_PARSE_SLICES, pinned by the REAL reference decoder.

Run in the build container (needs oracle/_ref/ref_decode, built from the reference by
`make -C oracle ref`).  For every pair of tests/slices_streams.py (written by the bit writer of
tests/directed_syntax.py, not by the library's): "ms", rows cut into several slices, which the
reference cannot pin, and "ref", the same picture model with one slice per row.  The compiled
reference decodes "ref" at one thread, and this stores
  tests/golden/slices/<name>.ms.m2v    the multi-slice form
  tests/golden/slices/<name>.ref.m2v   its twin
  tests/golden/slices/<name>.m2v       the negative streams (no twin, no MD5: nothing decodes them)
  tests/golden/slices/manifest.json    geometry, per-frame MD5 of the reference's YUV output of the
                                       twin in display order, the event log of the ms form, and for
                                       the negative streams status, reason and blamed slice
The guard against stale frames is make_syntax_fixtures.py's.
"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [REPO, os.path.join(REPO, "tests"), HERE]

import slices_streams as SL  # noqa: E402
from make_syntax_fixtures import REF, RUNS, ref_md5s  # noqa: E402

OUT = SL.GOLDEN


def main():
    if not os.path.exists(REF):
        sys.exit("build the reference first: make -C oracle ref")
    os.makedirs(OUT, exist_ok=True)
    manifest = []
    with tempfile.TemporaryDirectory() as tmp:
        yuv = os.path.join(tmp, "a.yuv")
        for ms, ref in SL.build_all():
            assert (ms.mbs, ms.coefs) == (ref.mbs, ref.coefs), ms.name  # one picture model
            files = {}
            for form, S in (("ms", ms), ("ref", ref)):
                files[form] = f"{S.name}.{form}.m2v"
                with open(os.path.join(OUT, files[form]), "wb") as f:
                    f.write(S.es)
            path = os.path.join(OUT, files["ref"])
            runs = [ref_md5s(path, ref.width, ref.height, ref.cf, yuv) for _ in range(RUNS)]
            good = [r for r in runs if len(r) == ref.npics and len(set(r)) == len(r)]
            if not good:
                raise RuntimeError(f"{ref.name}: no reference run with {ref.npics} pairwise different frames: {runs[0]}")
            if any(r != good[0] for r in good):
                raise RuntimeError(f"{ref.name}: clean reference runs disagree")
            manifest.append(dict(name=ms.name, ms=files["ms"], ref=files["ref"], width=ms.width, height=ms.height,
                                 chroma_format=ms.cf, frames=ms.npics, slices=ms.nslices, md5=good[0],
                                 events=sorted(ms.events)))
            print(f"{ms.name}: {ms.npics} frames, {ms.nslices} slices, {len(ms.es)} + {len(ref.es)} bytes")
        for build, status, reason, blamed in SL.NEGATIVE:
            S = build()
            with open(os.path.join(OUT, S.name + ".m2v"), "wb") as f:
                f.write(S.es)
            manifest.append(dict(name=S.name, ms=S.name + ".m2v", ref=None, width=S.width, height=S.height,
                                 chroma_format=S.cf, frames=0, slices=S.nslices, md5=None, status=status, reason=reason,
                                 blamed_slice=blamed, events=[]))
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1)
        f.write("\n")
    total = sum(os.path.getsize(os.path.join(OUT, n)) for n in os.listdir(OUT))
    assert total < 1024 * 1024, total
    print(f"{len(manifest)} streams, {total} bytes")


if __name__ == "__main__":
    main()
