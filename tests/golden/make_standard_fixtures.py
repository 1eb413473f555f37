"""Generate the twin-stream fixtures of MP2VG_PARSE_STANDARD, pinned by the REAL reference decoder.

Run in the build container (needs oracle/_ref/ref_decode, built from the reference by
`make -C oracle ref`).  For every pair of tests/standard_streams.py (written by the bit writer of
tests/directed_syntax.py, not by the library's): S' in the standard's form, which the reference
cannot decode, and S, the same pictures in the reference's subset (intra_vlc_format 1, a full
quant_matrix_extension with each picture's effective matrices).  The compiled reference decodes S
at one thread, and this stores
  tests/golden/standard/<name>.std.m2v   S'
  tests/golden/standard/<name>.ref.m2v   S
  tests/golden/standard/manifest.json    geometry, per-frame MD5 of the reference's YUV output of S
                                         in display order, and the event log of S'
The refused 4:2:2 stream is stored too (no twin, no MD5: nothing decodes it).

The guard against stale frames is make_syntax_fixtures.py's: the reference's scheduler can deliver
a stale frame even at one thread; such a run repeats an earlier frame, every picture of a stream
differs from every other (asserted on the reference's own frames), and the clean runs must agree.
"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [REPO, os.path.join(REPO, "tests"), HERE]

import standard_streams as SS  # noqa: E402
from make_syntax_fixtures import REF, RUNS, ref_md5s  # noqa: E402

OUT = SS.GOLDEN


def main():
    if not os.path.exists(REF):
        sys.exit("build the reference first: make -C oracle ref")
    os.makedirs(OUT, exist_ok=True)
    manifest = []
    with tempfile.TemporaryDirectory() as tmp:
        yuv = os.path.join(tmp, "a.yuv")
        for std, ref in SS.build_all():
            assert (std.mbs, std.coefs, std.W) == (ref.mbs, ref.coefs, ref.W), std.name  # one picture model
            files = {}
            for form, S in (("std", std), ("ref", ref)):
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
            stale = sum(1 for r in runs if r != good[0])
            if stale:
                print(f"WARNING {ref.name}: {stale} of {RUNS} reference runs delivered a stale frame")
            manifest.append(dict(name=std.name, std=files["std"], ref=files["ref"], width=std.width, height=std.height,
                                 chroma_format=std.cf, frames=std.npics, md5=good[0], events=sorted(std.events)))
            print(f"{std.name}: {std.npics} frames, {len(std.es)} + {len(ref.es)} bytes")
        S = SS.refused_422()
        with open(os.path.join(OUT, S.name + ".std.m2v"), "wb") as f:
            f.write(S.es)
        manifest.append(dict(name=S.name, std=S.name + ".std.m2v", ref=None, width=S.width, height=S.height,
                             chroma_format=S.cf, frames=0, md5=None, status=-2, reason=SS.REFUSED_422_REASON,
                             events=[]))
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1)
        f.write("\n")
    total = sum(os.path.getsize(os.path.join(OUT, n)) for n in os.listdir(OUT))
    assert total < 256 * 1024, total
    print(f"{len(manifest)} streams, {total} bytes")


if __name__ == "__main__":
    main()
