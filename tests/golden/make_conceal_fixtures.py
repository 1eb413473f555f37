"""Generate the concealment fixtures, pinned by the REAL reference decoder.

Run in the build container (needs oracle/_ref/ref_decode, built from the reference by
`make -C oracle ref`).  For every case of tests/conceal_streams.py REPAIR_CASES: the stream of
REPAIR with one slice of a P or of a B picture made to fail (conceal_streams.damaged_stream), and
its repaired twin, in which that slice is replaced, byte-spliced between start codes, by a slice
from the independent writer of tests/directed_syntax.py that codes the replacement row legally
(first and last macroblock "MC, not coded" with zero vectors, a skip run between).  The reference
decodes the repaired stream at one thread; stored are
  tests/golden/conceal/<name>_damaged.m2v, <name>_repaired.m2v
  tests/golden/conceal/manifest.json    geometry, the damaged (picture, row), the unflagged
                                        rejection's reason, per-frame MD5 of the reference's YUV
                                        output of the repaired stream in display order
As in make_syntax_fixtures.py a reference run that delivers a stale frame is recognised by a
repeated frame and dropped; the clean runs must agree.
"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [REPO, os.path.join(REPO, "tests"), HERE]
OUT = os.path.join(HERE, "conceal")
RUNS = 6

import conceal_streams as CS  # noqa: E402
from make_syntax_fixtures import REF, ref_md5s  # noqa: E402
from tiny_mp2v_dec_amd.records import Parsed  # noqa: E402


def main():
    if not os.path.exists(REF):
        sys.exit("build the reference first: make -C oracle ref")
    os.makedirs(OUT, exist_ok=True)
    manifest = []
    with tempfile.TemporaryDirectory() as tmp:
        yuv = os.path.join(tmp, "a.yuv")
        for name, (pct, (pic, row)) in CS.REPAIR_CASES.items():
            bad, es, w, h, cf, why = CS.damaged_stream(CS.REPAIR, [(pic, row)])
            pristine = Parsed(es, w, h, cf)
            assert int(pristine.pics["picture_coding_type"][pic]) == pct and int(pristine.pics["fwd_slot"][pic]) >= 0
            fixed = CS.repaired(bad, w, h, cf, pct, pic, row)
            files = {k: f"{name}_{k}.m2v" for k in ("damaged", "repaired")}
            for k, data in (("damaged", bad), ("repaired", fixed)):
                with open(os.path.join(OUT, files[k]), "wb") as f:
                    f.write(data)
            path = os.path.join(OUT, files["repaired"])
            runs = [ref_md5s(path, w, h, cf, yuv) for _ in range(RUNS)]
            good = [r for r in runs if len(r) == pristine.npics and len(set(r)) == len(r)]
            if not good or any(r != good[0] for r in good):
                raise RuntimeError(f"{name}: no agreeing clean reference runs: {runs[0]}")
            manifest.append(dict(name=name, width=w, height=h, chroma_format=cf, picture=pic, row=row,
                                 picture_coding_type=pct, reason=why[(pic, row)], frames=pristine.npics,
                                 md5=good[0], **files))
            print(f"{name}: picture {pic} row {row} ({why[(pic, row)]}), {len(bad)} bytes")
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1)
        f.write("\n")
    total = sum(os.path.getsize(os.path.join(OUT, n)) for n in os.listdir(OUT))
    assert total < 64 * 1024, total
    print(f"{len(manifest)} pairs, {total} bytes")


if __name__ == "__main__":
    main()
