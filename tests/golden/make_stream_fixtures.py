"""Generate the whole-stream golden fixtures from the REAL reference decoder.

Run in the build container (needs oracle/_ref/ref_decode, built from /root/reference by
`make -C oracle ref`).  For every case below: write the elementary stream with our stream
writer (accepted subset only), decode it with the compiled reference at 1 and 4
threads (outputs must agree), and store
  tests/golden/streams/<name>.m2v           the input stream
  tests/golden/streams/manifest.json        geometry + per-frame MD5 of the reference's YUV
                                            output in display order (reference
                                            tiny_mp2v_dec.cpp:11-17 write_yuv layout)
The reference itself does not travel to the GPU box; these files do.
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
REF = os.path.join(REPO, "oracle", "_ref", "ref_decode")
OUT = os.path.join(HERE, "streams")

from tiny_mp2v_dec_amd.records import generate_es  # noqa: E402

CASES = [
    # name, width, height, chroma_format, generator params
    ("i420_cif_intra", 352, 288, 1, dict(n_gops=1, gop_n=3, gop_m=1, mix=1, seed=1729)),
    ("ipb420_qcif", 176, 144, 1, dict(n_gops=2, gop_n=12, gop_m=3, leading_b=1, seed=1730)),
    ("ipb420_qcif_openb", 176, 144, 1, dict(n_gops=1, gop_n=10, gop_m=3, leading_b=0, seed=1731)),
    ("ipb420_field", 176, 144, 1, dict(n_gops=1, gop_n=12, gop_m=3, frame_pred_frame_dct=0, seed=1732)),
    ("ipb422_qcif", 176, 144, 2, dict(n_gops=1, gop_n=12, gop_m=3, seed=1733)),
    ("ipb422_field", 176, 144, 2, dict(n_gops=1, gop_n=12, gop_m=3, frame_pred_frame_dct=0, seed=1734)),
    ("ipb444_qcif", 176, 144, 3, dict(n_gops=1, gop_n=12, gop_m=3, seed=1735)),
    # 4:4:4 field MC (16x8 chroma per field, no chroma MV scaling); dct_type stays 0 (the writer
    # never emits 4:4:4 field DCT: the reference misplaces blocks 10/11, mb_decoder.cpp:193-194)
    ("ipb444_field", 176, 144, 3, dict(n_gops=1, gop_n=12, gop_m=3, frame_pred_frame_dct=0, seed=1741)),
    ("stress_saturation", 352, 288, 1, dict(n_gops=1, gop_n=9, gop_m=2, frame_pred_frame_dct=0,
                                            big_level_permille=250, escape_permille=300,
                                            big_matrix_permille=400, coefs_max=30, intra_coefs_max=50,
                                            seed=1736)),
    ("stress_mv_fcode4", 352, 288, 2, dict(n_gops=1, gop_n=9, gop_m=3, f_code=4, quant_permille=400,
                                           frame_pred_frame_dct=0, seed=1737)),
    ("mc_heavy_fcode1", 176, 144, 1, dict(n_gops=1, gop_n=12, gop_m=3, f_code=1, mix=2, seed=1738)),
    ("tall_2816_vpos_ext", 64, 2816, 1, dict(n_gops=1, gop_n=4, gop_m=3, leading_b=0, seed=1739)),
    ("hd1080_420_ipb", 1920, 1088, 1, dict(n_gops=1, gop_n=4, gop_m=3, leading_b=0, seed=1740)),
    # high-bitrate intra: I-picture blocks of 18-50 coefficients (up to 200 per mille escape-sized
    # levels), in both scans, next to P/B pictures, in every chroma format
    ("intra444_dense", 176, 144, 3, dict(n_gops=1, gop_n=3, gop_m=1, mix=1, intra_coefs_min=20,
                                          intra_coefs_max=40, alternate_scan=-1, seed=1742)),
    ("intra422_dense_alt", 352, 288, 2, dict(n_gops=1, gop_n=2, gop_m=1, mix=1, intra_coefs_min=18,
                                              intra_coefs_max=50, alternate_scan=1, big_level_permille=200,
                                              seed=1743)),
    ("ipb420_dense_i", 176, 144, 1, dict(n_gops=2, gop_n=6, gop_m=3, intra_coefs_min=20, intra_coefs_max=40,
                                          alternate_scan=-1, seed=1744)),
    # row widths no other stream has: 45 MBs (720 px, remainder 1 mod the kernel's 4-MB group),
    # 5 MBs (one full group and a one-MB group) and 3 MBs (narrower than one group)
    ("sd480_420_field", 720, 480, 1, dict(n_gops=1, gop_n=6, gop_m=3, frame_pred_frame_dct=0, seed=1745)),
    ("w80_422_field", 80, 48, 2, dict(n_gops=1, gop_n=12, gop_m=3, frame_pred_frame_dct=0, seed=1746)),
    ("w48_444", 48, 32, 3, dict(n_gops=1, gop_n=12, gop_m=3, seed=1747)),
    # the geometry limits (MP2VG_MAX_DIMENSION): 1024 MB rows, slices in all eight values of
    # slice_vertical_position_extension, vertical_size 16383 (value 4095, extension 3); and 1024-MB
    # rows with f_code 9 vectors, horizontal_size 16383.  I, P and B with field MC / DCT.
    ("tall_16384_420", 16, 16384, 1, dict(n_gops=1, gop_n=3, gop_m=2, leading_b=0, frame_pred_frame_dct=0,
                                          seed=1748)),
    ("wide_16384_422", 16384, 16, 2, dict(n_gops=1, gop_n=3, gop_m=2, leading_b=0, frame_pred_frame_dct=0,
                                          f_code=9, seed=1749)),
]


def ref_decode(path, w, h, cf, threads, out):
    r = subprocess.run([REF, path, str(w), str(h), str(cf), str(threads), out], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"reference failed on {path}: {r.returncode} {r.stderr[-400:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    if not os.path.exists(REF):
        sys.exit("build the reference first: make -C oracle ref")
    os.makedirs(OUT, exist_ok=True)
    # names on the command line: only those cases are written, the others keep their manifest entry
    only = set(sys.argv[1:])
    assert only <= {c[0] for c in CASES}, only
    kept = {}
    if only:
        kept = {e["name"]: e for e in json.load(open(os.path.join(OUT, "manifest.json")))}
    manifest = []
    with tempfile.TemporaryDirectory() as tmp:
        for name, w, h, cf, params in CASES:
            if only and name not in only:
                manifest.append(kept[name])
                continue
            es = generate_es(width=w, height=h, chroma_format=cf, **params)
            path = os.path.join(OUT, name + ".m2v")
            with open(path, "wb") as f:
                f.write(es)
            y1, y4 = os.path.join(tmp, "a.yuv"), os.path.join(tmp, "b.yuv")
            cw = w if cf == 3 else w // 2
            ch = h if cf != 1 else h // 2
            fb = w * h + 2 * cw * ch

            def md5s(path, frames):
                data = open(path, "rb").read()
                assert len(data) == fb * frames, name
                return [hashlib.md5(data[k * fb:(k + 1) * fb]).hexdigest() for k in range(frames)]

            # golden = the single-threaded reference.  Its scheduler is racy even at
            # num_threads=1: the render thread polls the next pool slot (threads.cpp:172-187) and
            # takes a picture that create_task just reset (threads.cpp:162-170; no slices yet, so
            # done_slices == slices_tasks.size() == 0) before the parser has added its slices, and
            # renders that slot's STALE frame (seen: ipb420_field frame 9 == frame 2, byte for
            # byte, in 2 of 8 one-thread runs).  Such a run is recognisable: one of its frames
            # repeats an earlier frame exactly, which a synthetic random stream never does.  The
            # golden is a run with no repeated frame; every clean run must agree with it, and the
            # racy runs (1-thread and 4-thread) are recorded in the manifest, not hidden.
            def clean(m):
                return len(set(m)) == len(m)

            runs = []
            for _ in range(8):
                info = ref_decode(path, w, h, cf, 1, y1)
                runs.append(md5s(y1, info["frames"]))
            good = [r for r in runs if clean(r)]
            if not good:
                raise RuntimeError(f"{name}: no race-free reference run")
            md5 = good[0]
            if any(r != md5 for r in good):
                raise RuntimeError(f"{name}: race-free reference runs disagree")
            st_mismatch = [[k for k in range(len(md5)) if r[k] != md5[k]] for r in runs if r != md5]
            for bad in st_mismatch:
                print(f"WARNING {name}: a racy 1-thread reference run (stale frame) differs at frames {bad}")
            mt_mismatch = []
            for _ in range(3):
                info4 = ref_decode(path, w, h, cf, 4, y4)
                md5b = md5s(y4, info4["frames"])
                if md5b != md5:
                    bad = [k for k in range(min(len(md5), len(md5b))) if md5[k] != md5b[k]]
                    mt_mismatch.append(bad)
                    print(f"WARNING {name}: 4-thread reference differs from the golden at frames {bad}"
                          f"{' (stale frame)' if not clean(md5b) else ''}")
            manifest.append(dict(name=name, file=name + ".m2v", width=w, height=h, chroma_format=cf,
                                 frames=info["frames"], bytes=len(es), params=params, md5=md5,
                                 ref_mt_mismatch=mt_mismatch, ref_st_mismatch=st_mismatch))
            print(f"{name}: {info['frames']} frames, {len(es)} bytes")
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1)


if __name__ == "__main__":
    main()
