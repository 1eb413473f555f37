"""bench.py's plain run, --full, --dump-outputs and the stream kept for it by `bench.py --prepare`."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_stream_is_kept_and_read_back_identical():
    """bench_stream writes the stream it generates under _build/bench_streams/ and a second call
    reads the same bytes back; `bench.py --prepare` (what build() runs) does that with no GPU."""
    bench = importlib.import_module("bench")
    from tiny_mp2v_dec_amd import records as R
    stamp = bench._library_stamp()
    assert stamp  # conftest built the library, and build.py stamps it
    d = os.path.join(REPO, "tiny_mp2v_dec_amd", "_build", "bench_streams")
    path = os.path.join(d, f"c2_g1_s4321_{stamp[:16]}.m2v")
    try:
        width, height, cf, gparams, _ = bench.CONFIGS["c2"]
        es = R.generate_es(width=width, height=height, chroma_format=cf, n_gops=1, seed=4321, **gparams)
        assert bench.bench_stream("c2", 1, 4321) == es and os.path.exists(path)
        with open(path, "rb") as fh:
            assert fh.read() == es
        assert bench.bench_stream("c2", 1, 4321) == es
    finally:
        if os.path.exists(path):
            os.unlink(path)
    prepared = os.path.join(d, f"c1_g1_s1729_{stamp[:16]}.m2v")
    try:
        r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--prepare", "--config", "c1", "--gops", "1"],
                           capture_output=True, text=True, timeout=120, cwd=REPO)
        assert r.returncode == 0 and r.stdout == "", r.stderr[-2000:]
        assert os.path.getsize(prepared) > 0
    finally:
        if os.path.exists(prepared):
            os.unlink(prepared)


def _run_bench(*extra):
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--gops", "2"] + list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_batch(tmp_path):
    """A plain run reports the headline figures of its --steps timed steps and none of the --full
    measurements; --dump-outputs writes float32 / float64 arrays under 64 MB whose sampled frames
    carry the digests the device computed for them (records.planes_digest is the host twin)."""
    from tiny_mp2v_dec_amd import records as R
    line = _run_bench("--dump-outputs", str(tmp_path))
    assert line["steps"] == 3 and line["warmup"] == 1 and line["unit"] == "frames/s" and line["dtype"] == "u8"
    assert line["higher_is_better"] is True and line["ms_per_step"] > 0 and line["roofline"]["frac"] > 0
    # value = frames per step / the step's time; both are rounded in the line (ms_per_step to 1e-4 ms)
    assert line["value"] == pytest.approx(24 * 1000.0 / line["ms_per_step"], rel=1e-2)
    for moved in ("parity", "cpu_baseline", "e2e_dropin", "frame_digest_of_digests", "frame_gather"):
        assert moved not in line
    assert "per_kernel" not in line["roofline"]
    files = sorted(os.listdir(tmp_path))
    assert files == ["frame_digests.npy", "frame_slots.npy", "frames_u.npy", "frames_v.npy", "frames_y.npy"]
    out = {f[:-4]: np.load(os.path.join(tmp_path, f)) for f in files}
    assert sum(a.nbytes for a in out.values()) <= 64 << 20
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    assert out["frame_digests"].shape == (24, 2) and out["frames_y"].shape[1:] == (1088, 1920)
    assert out["frames_u"].shape == out["frames_v"].shape == (len(out["frame_slots"]), 544, 960)
    dig = (out["frame_digests"][:, 0].astype(np.uint64) << np.uint64(32)) | out["frame_digests"][:, 1].astype(np.uint64)
    for k, slot in enumerate(out["frame_slots"].astype(int)):
        planes = [out[n][k].astype(np.uint8) for n in ("frames_y", "frames_u", "frames_v")]
        assert all(np.array_equal(p, out[n][k]) for p, n in zip(planes, ("frames_y", "frames_u", "frames_v")))
        assert R.planes_digest(planes) == int(dig[slot])


@pytest.mark.gpu
def test_full_run_adds_the_checks_and_baselines():
    """--full keeps every measurement the line carried before the option existed."""
    line = _run_bench("--full")
    assert line["parity"]["status"] in ("bit-exact", "unchecked")
    assert line["roofline"]["per_kernel"] and line["roofline"]["one_stream_span_ms"] > 0
    assert line["cpu_baseline"]["value"] > 0 and line["e2e_dropin"]["value"] > 0
    assert line["e2e_dropin_device_frames"]["value"] > 0 and "frame_digest_of_digests" in line
